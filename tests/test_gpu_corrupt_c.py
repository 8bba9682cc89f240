"""fav_op_corrupt_c on the device against tests/corrupt_c_ref.py: the five exact kinds bit for bit, speckle and the two blurs
within derived bounds of float64, determinism and sharding, the rejections, and Backend.robustness_report.

Shapes: a single pixel; H = 1; odd widths with no full 4-pixel group; frames smaller than every blur radius; a frame that
spans several 32-wide tiles with ragged edges; several frames under one block.

Two of the issue's cases are held to a bound instead of to equality, because they are not identities in fp32:
  * contrast at a = 1 computes fl(fl(x - m) + m): two roundings of values in [0, 1], at most 2^-25 each, so 2^-24 from x; a
    constant frame has m = fl(double(S) / (H W 255)), the correctly rounded v / 255, while x = fl(v * fl(1 / 255)) can be
    its neighbour: |out - x| <= 2^-23.
  * pixelate at a = 1 is fl(v) / fl(255), correctly rounded, against the same x: |out - x| <= 2^-23.
Both are also compared with the fp32 restatement bit for bit, which is the real check."""
import ctypes as C
import math

import numpy as np
import pytest

pytestmark = pytest.mark.gpu

torch = pytest.importorskip("torch")
import corrupt_c_ref as R  # noqa: E402
from conftest import note  # noqa: E402
from failure_aware_vision_amd import _lib  # noqa: E402
from failure_aware_vision_amd.corrupt import Corruptor  # noqa: E402

f32 = np.float32
SHAPES, SEEDS, FIRST = R.SHAPES, R.SEEDS, R.FIRST_INDEX
ids = lambda s: "x".join(map(str, s)) if isinstance(s, tuple) else str(s)  # noqa: E731
EPS = 2.0 ** -23


@pytest.fixture(scope="module")
def lib():
    return _lib.load()


def device(frames, kind, a, b=0.0, seed=0, first=FIRST):
    out = Corruptor(seed=seed).imagenet_c(torch.from_numpy(frames).cuda(), kind, a=a, b=b, first_index=first)
    assert out.dtype == torch.float32 and tuple(out.shape) == frames.shape and out.is_cuda
    return out.cpu().numpy()


def same_bits(got, want):
    return got.dtype == want.dtype == f32 and np.array_equal(got, want) and not np.isnan(got).any()


# ---- the exact kinds -------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("shape", SHAPES, ids=ids)
def test_impulse_bit_exact(shape):
    frames = R.frames_of(shape)
    for seed in SEEDS:
        for sev in (1, 2, 3, 4, 5):
            a, _ = R.params("impulse_noise", sev)
            assert same_bits(device(frames, "impulse_noise", a, seed=seed), R.impulse(frames, a, seed, FIRST)[0]), (hex(seed), sev)
        assert same_bits(device(frames, "impulse_noise", 0.0, seed=seed), R.x_of(frames))         # a = 0: the identity
        ones = device(frames, "impulse_noise", 1.0, seed=seed)                                   # a = 1: every value hit
        assert same_bits(ones, R.impulse(frames, 1.0, seed, FIRST)[0]) and np.isin(ones, (0.0, 1.0)).all()


def test_impulse_hit_share():
    """a = .27 on a grey (1, 64, 80) frame, where a value is hit iff it is 0 or 1: the share of the N = 15360 values that are
    hit lies within 4 binomial standard errors sqrt(.27 * .73 / N) = 0.0036 of .27, on the device and in the reference's draw."""
    frames = np.full((1, 64, 80, 3), 128, np.uint8)
    a, _ = R.params("impulse_noise", 5)
    se = math.sqrt(a * (1 - a) / frames.size)
    for seed in SEEDS:
        got = device(frames, "impulse_noise", a, seed=seed)
        want, hit = R.impulse(frames, a, seed, FIRST)
        assert same_bits(got, want)
        share = np.isin(got, (0.0, 1.0)).mean()
        note(f"corrupt_c: impulse a = {a:.2f} seed {seed:#x}: hit share {share:.4f} (reference {hit.mean():.4f}, 4 se = {4 * se:.4f})")
        assert abs(hit.mean() - a) <= 4 * se and abs(share - a) <= 4 * se
        assert 0.4 < (got[np.isin(got, (0.0, 1.0))] == 1.0).mean() < 0.6


@pytest.mark.parametrize("shape", SHAPES, ids=ids)
def test_contrast_bit_exact(shape):
    frames = R.frames_of(shape)
    const = np.full(shape + (3,), 77, np.uint8)
    const[..., 1] = 200
    for sev in (1, 2, 3, 4, 5):
        a, _ = R.params("contrast", sev)
        assert same_bits(device(frames, "contrast", a), R.contrast(frames, a)), sev
        got = device(const, "contrast", a)                                                       # a constant frame: out == x
        assert same_bits(got, R.contrast(const, a)) and np.abs(got - R.x_of(const)).max() <= EPS
    got = device(frames, "contrast", 1.0)                                                        # a = 1: the identity
    assert same_bits(got, R.contrast(frames, 1.0)) and np.abs(got - R.x_of(frames)).max() <= EPS
    got = device(frames, "contrast", 0.0)                                                        # a = 0: the channel means
    assert same_bits(got, R.contrast(frames, 0.0)) and all((got[f, ..., c] == got[f, 0, 0, c]).all()
                                                           for f in range(shape[0]) for c in range(3))


@pytest.mark.parametrize("shape", SHAPES, ids=ids)
def test_pixelate_bit_exact(shape):
    frames = R.frames_of(shape)
    for sev in (1, 2, 3, 4, 5):
        a, _ = R.params("pixelate", sev)
        assert same_bits(device(frames, "pixelate", a), R.pixelate(frames, a)), sev
    got = device(frames, "pixelate", 1.0)                                                        # a = 1: one pixel a cell
    assert same_bits(got, R.pixelate(frames, 1.0)) and np.abs(got - R.x_of(frames)).max() <= EPS
    a = 0.01                                                                                     # hd = wd = 1: the frame mean
    assert R.cell_map(shape[1], a)[0] == 1 and R.cell_map(shape[2], a)[0] == 1
    got = device(frames, "pixelate", a)
    mean = (frames.astype(np.int64).sum(axis=(1, 2)).astype(f32) / f32(shape[1] * shape[2] * 255))[:, None, None, :]
    assert same_bits(got, R.pixelate(frames, a)) and same_bits(got, np.broadcast_to(mean, got.shape).copy())


@pytest.mark.parametrize("kind", ("brightness", "saturate"))
@pytest.mark.parametrize("shape", SHAPES, ids=ids)
def test_hsv_kinds_bit_exact(shape, kind):
    frames = R.frames_of(shape)                        # black, white, grey and primary-colour pixels come first
    cases = [R.params(kind, sev) for sev in (1, 2, 3, 4, 5)]
    cases += [(0.0, 0.0), (1.0, 0.0)] if kind == "brightness" else [(0.0, 0.0), (1.0, 0.0), (1.0, -1.0), (0.0, 1.0), (3.0, -0.5)]
    for a, b in cases:
        want = R.brightness(frames, a) if kind == "brightness" else R.saturate(frames, a, b)
        assert same_bits(device(frames, kind, a, b), want), (a, b)
    if kind == "brightness":
        assert np.abs(device(frames, kind, 0.0) - R.x_of(frames)).max() <= EPS                  # x * (V / V)
        black = device(np.zeros((1, 2, 3, 3), np.uint8), kind, 0.3)
        assert (black == f32(0.3)).all()                                                         # V == 0: grey of value a
    else:
        grey = np.full((1, 2, 3, 3), 128, np.uint8)
        assert same_bits(device(grey, kind, 5.0, 0.0), R.x_of(grey))                             # grey stays grey while S2 = 0
        red = device(grey, kind, 5.0, 1.0)                                                       # S2 = 1 at hue 0: (V, 0, 0)
        assert (red[..., 0] == R.x_of(grey)[..., 0]).all() and (red[..., 1:] == 0.0).all()


# ---- speckle ---------------------------------------------------------------------------------------------------------
# The fp32 CPU restatement (corrupt_c_ref.speckle(..., dtype=float32)) of the same formula is within 1.6e-7 / 2.1e-7 / 3.6e-7 /
# 4.3e-7 / 5.76e-7 of the float64 one at severities 1..5, the maximum over these shapes and seeds; four times the severity-5
# figure is the bound, which leaves the device's logf / sqrtf / cosf / sinf a factor of four, as GAUSSIAN_TOL does in
# test_gpu_corrupt_edges.py.  The device's own maximum per severity is noted by the test; on an MI355X it is
# 1.602e-7 / 2.152e-7 / 3.309e-7 / 4.310e-7 / 5.330e-7 at severities 1..5 (DEVICE_MAX), at or below the CPU restatement's.
SPECKLE_F32_VS_F64_SEV5 = 5.76e-7
SPECKLE_TOL = 4 * SPECKLE_F32_VS_F64_SEV5            # 2.304e-6
#: max |device - float64| per severity over all shapes and seeds, from the MI355X run of this file
DEVICE_MAX = (1.602e-7, 2.152e-7, 3.309e-7, 4.310e-7, 5.330e-7)


@pytest.mark.parametrize("severity", (1, 2, 3, 4, 5))
def test_speckle_against_float64(severity):
    a, _ = R.params("speckle_noise", severity)
    worst = 0.0
    for shape in SHAPES:
        frames = R.frames_of(shape)
        for seed in SEEDS:
            got = device(frames, "speckle_noise", a, seed=seed)
            ref = R.speckle(frames, a, seed, FIRST)
            worst = max(worst, float(np.abs(got.astype(np.float64) - ref).max()))
            assert got.min() >= 0.0 and got.max() <= 1.0 and np.isfinite(got).all()
            assert (got[frames == 0] == 0.0).all()                                               # black stays exactly 0
    note(f"corrupt_c: speckle severity {severity} (sigma {a:.2f}): max |device - float64| = {worst:.3e} (bound {SPECKLE_TOL:.3e})")
    assert worst <= SPECKLE_TOL


# ---- the two blurs ---------------------------------------------------------------------------------------------------
def gauss_bound(R_):
    """n = 2R+1 products and n additions of values in [0,1] with weights that sum to 1 cost at most (n + 2) 2^-23 a pass; the
    second pass carries the first pass's error through weights that sum to 1."""
    return 2 * (2 * R_ + 3) * EPS


def defocus_bound(R_):
    return ((2 * R_ + 1) ** 2 + 2) * EPS


@pytest.mark.parametrize("severity", (1, 2, 3, 4, 5))
@pytest.mark.parametrize("shape", SHAPES, ids=ids)
def test_gaussian_blur_against_float64(lib, shape, severity):
    a, b = R.params("gaussian_blur", severity)
    st, taps, rad = R.lib_taps(lib, "gaussian_blur", a, b)
    assert st == 0 and rad == R.GAUSS_RADII[severity - 1]
    frames = R.frames_of(shape)
    got = device(frames, "gaussian_blur", a)
    worst = float(np.abs(got.astype(np.float64) - R.gaussian_blur(frames, taps)).max())
    note(f"corrupt_c: gaussian blur {ids(shape)} R = {rad}: max |device - float64| = {worst:.3e} (bound {gauss_bound(rad):.3e})")
    assert worst <= gauss_bound(rad) and got.min() >= 0.0 and got.max() <= 1.0
    const = np.full(shape + (3,), 201, np.uint8)
    assert np.abs(device(const, "gaussian_blur", a).astype(np.float64) - float(f32(201) * f32(1 / 255))).max() <= gauss_bound(rad)
    swapped = device(np.ascontiguousarray(frames.transpose(0, 2, 1, 3)), "gaussian_blur", a)
    assert np.abs(swapped.transpose(0, 2, 1, 3).astype(np.float64) - got).max() <= gauss_bound(rad)


@pytest.mark.parametrize("severity", (1, 2, 3, 4, 5))
@pytest.mark.parametrize("shape", SHAPES, ids=ids)
def test_defocus_blur_against_float64(lib, shape, severity):
    """(1,1,1) and (2,1,5) reflect more than once at every radius; (3,7,13) from R = 7 on."""
    a, b = R.params("defocus_blur", severity)
    st, taps, rad = R.lib_taps(lib, "defocus_blur", a, b)
    assert st == 0 and rad == R.DEFOCUS_RADII[severity - 1]
    frames = R.frames_of(shape)
    got = device(frames, "defocus_blur", a, b)
    worst = float(np.abs(got.astype(np.float64) - R.defocus_blur(frames, taps)).max())
    note(f"corrupt_c: defocus {ids(shape)} R = {rad}: max |device - float64| = {worst:.3e} (bound {defocus_bound(rad):.3e})")
    assert worst <= defocus_bound(rad) and got.min() >= 0.0 and got.max() <= 1.0
    if shape == (1, 1, 1):
        assert np.abs(got.astype(np.float64) - R.x_of(frames)).max() <= defocus_bound(rad)       # one pixel: itself
    const = np.full(shape + (3,), 201, np.uint8)
    assert np.abs(device(const, "defocus_blur", a, b).astype(np.float64) - float(f32(201) * f32(1 / 255))).max() <= defocus_bound(rad)


def test_blur_limits(lib):
    """The largest radii the ABI takes: gaussian R = 32 (sigma 8.1) and defocus R = 14 (radius 12), on ragged tiles."""
    frames = R.frames_of((2, 33, 31))
    for kind, a, b, rad, bound, ref in (("gaussian_blur", 8.1, 0.0, 32, gauss_bound, R.gaussian_blur),
                                        ("defocus_blur", 12.0, 0.5, 14, defocus_bound, R.defocus_blur)):
        st, taps, r = R.lib_taps(lib, kind, a, b)
        assert st == 0 and r == rad
        got = device(frames, kind, a, b)
        assert np.abs(got.astype(np.float64) - ref(frames, taps)).max() <= bound(rad)
    one = device(frames, "gaussian_blur", 0.1)                                                   # R = 0: one tap of 1
    assert same_bits(one, R.x_of(frames))


# ---- determinism and sharding ----------------------------------------------------------------------------------------
def raw_call(lib, frames_dev, out_dev, kind, a, b, seed, first):
    n, H, W, _ = frames_dev.shape
    d = _lib.FavCorruptionDesc(32, R.KINDS.index(kind), a, b, seed, first)
    st = lib.fav_op_corrupt_c(frames_dev.data_ptr(), out_dev.data_ptr(), n, H, W, C.byref(d), torch.cuda.current_stream().cuda_stream)
    torch.cuda.synchronize()
    return st


@pytest.mark.parametrize("kind", R.KINDS)
def test_determinism_and_sharding(lib, kind):
    """Frames [2:5] of (5, 9, 13) start 702 bytes into the buffer: the shard's input is not dword aligned, and written into
    rows 2..4 of a whole-size output it lands where the three-float4 path applies; into a fresh tensor, where it does not."""
    frames = R.frames_of((5, 9, 13))
    dev = torch.from_numpy(frames).cuda()
    a, b = R.params(kind, 3)
    seed = SEEDS[1]
    cor = Corruptor(seed=seed)
    whole = cor.imagenet_c(dev, kind, 3, first_index=FIRST)
    assert torch.equal(whole, cor.imagenet_c(dev, kind, 3, first_index=FIRST))                   # two identical calls
    assert torch.equal(cor.imagenet_c(dev[2:5], kind, 3, first_index=FIRST + 2), whole[2:5])
    buf = torch.full((5, 9, 13, 3), float("nan"), device="cuda")
    assert raw_call(lib, dev[2:5], buf[2:5], kind, a, b, seed, FIRST + 2) == 0
    assert torch.equal(buf[2:5], whole[2:5]) and bool(torch.isnan(buf[:2]).all())                # nothing outside the shard
    assert raw_call(lib, dev[1:2], buf[1:2], kind, a, b, seed, FIRST + 1) == 0                   # 351 bytes in: a = 3
    assert torch.equal(buf[1:2], whole[1:2]) and bool(torch.isnan(buf[:1]).all())
    if kind in ("impulse_noise", "speckle_noise"):
        lo = cor.imagenet_c(dev, kind, 3, first_index=5)
        assert torch.equal(cor.imagenet_c(dev, kind, 3, first_index=2 ** 32 + 5), lo)            # the low 32 bits count
        assert not torch.equal(lo, whole)
        assert not torch.equal(Corruptor(seed=seed + 1).imagenet_c(dev, kind, 3, first_index=FIRST), whole)
    else:
        assert torch.equal(Corruptor(seed=seed + 1).imagenet_c(dev, kind, 3, first_index=77), whole)   # no draw: no seed


@pytest.mark.parametrize("kind", ("impulse_noise", "speckle_noise", "brightness", "saturate", "contrast"))
def test_staged_stores_behind_a_head(lib, kind):
    """The four-pixel kernels send a chunk of 256 full groups through LDS.  Frames [1:3] of (3, 41, 43) start 5289 bytes into
    the buffer (a = 1: one head pixel, which takes the position behind the last aligned group) and hold 3526 pixels (contrast:
    1763 a frame, heads of 1 and 2 pixels), and written into rows 1..2 of a whole-size output the aligned pixels land on 16
    bytes: staged chunks, a partial chunk and the head in one call.  Against the restatement and against the whole call."""
    frames = R.frames_of((3, 41, 43))
    dev = torch.from_numpy(frames).cuda()
    a, b = R.params(kind, 3)
    seed = SEEDS[1]
    whole = Corruptor(seed=seed).imagenet_c(dev, kind, 3, first_index=FIRST)
    ref = R.reference(frames, kind, a, b, seed, FIRST, lib)
    if kind == "speckle_noise":
        assert np.abs(whole.cpu().numpy().astype(np.float64) - ref).max() <= SPECKLE_TOL
    else:
        assert same_bits(whole.cpu().numpy(), ref)
    assert dev[1:3].data_ptr() % 4 == 1
    buf = torch.full((3, 41, 43, 3), float("nan"), device="cuda")
    assert (buf[1:3].data_ptr() + 12) % 16 == 0
    assert raw_call(lib, dev[1:3], buf[1:3], kind, a, b, seed, FIRST + 1) == 0
    assert torch.equal(buf[1:3], whole[1:3]) and bool(torch.isnan(buf[:1]).all())
    assert raw_call(lib, dev[2:3], buf[0:1], kind, a, b, seed, FIRST + 2) == 0                   # a = 2, output aligned for a = 0: scalar stores
    assert torch.equal(buf[0], whole[2])


# ---- rejections ------------------------------------------------------------------------------------------------------
NAN, INF = math.nan, math.inf
REJECTED = [("null input", dict(inp=None)), ("null output", dict(out=None)), ("null desc", dict(desc=None)),
            ("n == 0", dict(n=0)), ("H == 0", dict(H=0)), ("W == 0", dict(W=0)), ("n < 0", dict(n=-1)),
            ("struct_size", dict(size=28)), ("kind -1", dict(kind=-1)), ("kind 8", dict(kind=8)),
            ("a nan", dict(kind=6, a=NAN)), ("b nan", dict(kind=6, a=0.5, b=NAN)), ("a inf", dict(kind=1, a=INF)),
            ("b inf", dict(kind=6, a=0.5, b=INF)),
            ("impulse a < 0", dict(kind=0, a=-0.1)), ("impulse a > 1", dict(kind=0, a=1.1)),
            ("speckle a < 0", dict(kind=1, a=-0.1)),
            ("gaussian a == 0", dict(kind=2, a=0.0)), ("gaussian a < 0", dict(kind=2, a=-1.0)), ("gaussian R 33", dict(kind=2, a=8.2)),
            ("defocus r 0", dict(kind=3, a=0.9, b=0.5)), ("defocus r 13", dict(kind=3, a=13.0, b=0.5)),
            ("defocus b == 0", dict(kind=3, a=3.0, b=0.0)), ("defocus b < 0", dict(kind=3, a=3.0, b=-0.5)),
            ("contrast a < 0", dict(kind=4, a=-0.1)), ("contrast a > 1", dict(kind=4, a=1.5)),
            ("pixelate a == 0", dict(kind=5, a=0.0)), ("pixelate a > 1", dict(kind=5, a=1.01)),
            ("brightness a < 0", dict(kind=6, a=-0.1)), ("brightness a > 1", dict(kind=6, a=1.1)),
            ("saturate a < 0", dict(kind=7, a=-1.0)), ("saturate b < -1", dict(kind=7, a=1.0, b=-1.1)),
            ("saturate b > 1", dict(kind=7, a=1.0, b=1.1)),
            # the two limits beyond the parameter ranges (include/fav.h): pixelate's width, the output's alignment
            ("pixelate W 2049", dict(kind=5, a=0.5, n=1, H=1, W=2049)), ("out + 2 bytes", dict(out_offset=2))]


@pytest.mark.parametrize("why,kw", REJECTED, ids=[r[0] for r in REJECTED])
def test_rejections_launch_nothing(lib, why, kw):
    inp = torch.full((3 * 2049,), 100, dtype=torch.uint8, device="cuda")                         # room for the widest case
    out = torch.full((3 * 2049 * 4 + 4,), 0xA5, dtype=torch.uint8, device="cuda")
    stream = torch.cuda.current_stream().cuda_stream
    d = _lib.FavCorruptionDesc(kw.get("size", 32), kw.get("kind", 6), kw.get("a", 0.5), kw.get("b", 0.0), 1, 0)
    lib.fav_corruption_params(0, 1, C.byref(C.c_float()), C.byref(C.c_float()))                  # a call that succeeds in between
    status = lib.fav_op_corrupt_c(None if "inp" in kw else inp.data_ptr(), None if "out" in kw else out.data_ptr() + kw.get("out_offset", 0),
                                  kw.get("n", 2), kw.get("H", 4), kw.get("W", 8), None if "desc" in kw else C.byref(d), stream)
    torch.cuda.synchronize()
    assert status == 1, why                                                                      # FAV_ERR_INVALID_ARG
    assert b"fav_op_corrupt_c" in lib.fav_last_error(None)
    assert bool((out == 0xA5).all()), f"{why}: something was written"
    ok = _lib.FavCorruptionDesc(32, 6, 0.0, 0.0, 1, 0)                                           # brightness a = 0 on grey: x
    assert lib.fav_op_corrupt_c(inp.data_ptr(), out.data_ptr(), 2, 4, 8, C.byref(ok), stream) == 0
    torch.cuda.synchronize()
    assert bool((out[:768].view(torch.float32) == float(f32(100) * f32(1 / 255))).all()) and bool((out[768:] == 0xA5).all())


def test_imagenet_c_arguments():
    cor = Corruptor(seed=1)
    dev = torch.from_numpy(R.frames_of((2, 4, 8))).cuda()
    for bad in (dict(kind="fog", severity=1), dict(kind="contrast"), dict(kind="contrast", severity=0),
                dict(kind="contrast", severity=6)):
        with pytest.raises(ValueError):
            cor.imagenet_c(dev, **bad)
    with pytest.raises(ValueError):
        cor.imagenet_c(dev.float(), "contrast", 1)
    with pytest.raises(_lib.FavError, match="fav_op_corrupt_c"):
        cor.imagenet_c(dev, "contrast", a=2.0)
    assert torch.equal(cor.imagenet_c(dev, "saturate", 4), cor.imagenet_c(dev, "saturate", a=5.0, b=float(f32(0.1))))
    assert torch.equal(cor.imagenet_c(dev, "gaussian_noise", 3, first_index=9), cor.gaussian(dev, 3, first_index=9))


# ---- the report ------------------------------------------------------------------------------------------------------
def same_row(x, y):
    return set(x) == set(y) and all(x[k] == y[k] or (math.isnan(x[k]) and math.isnan(y[k])) for k in x)


def test_robustness_report(r18_blob):
    from failure_aware_vision_amd import Backend, synth
    from failure_aware_vision_amd.calibration import unpack_cells
    from failure_aware_vision_amd.robustness import COLUMNS, summarize, table
    blob, _ = r18_blob
    frames = synth.synthetic_frames_u8(16, 32, 32, seed=5)
    be = Backend("resnet18_cifar", blob, max_batch=8, temperature=1.3, tau=0.3)                  # two batches a row
    dev = torch.from_numpy(frames).cuda()
    pred, conf = be.classify(dev[:8])
    labels = np.concatenate([pred.cpu().numpy(), np.arange(8) % 10]).astype(np.int64)            # right ones and arbitrary ones
    kinds, sevs, seed, first = ("contrast", "gaussian_blur", "gaussian_noise"), (1, 5), 7, 40
    rows = be.robustness_report(frames, labels, corruptions=kinds, severities=sevs, seed=seed, first_index=first)
    assert list(rows) == [("clean", 0)] + [(k, s) for k in kinds for s in sevs]
    cor = Corruptor(seed=seed)
    for (kind, s), row in rows.items():
        fr = dev if kind == "clean" else cor.imagenet_c(dev, kind, s, first_index=first)
        c = unpack_cells(be.calibration_sweep(fr, labels, [be.cfg.temperature], first).cpu().numpy())
        assert same_row(row, summarize(c["label"][:, 0], c["confidence"][:, 0], c["nll"][:, 0], labels, 0.3)), (kind, s)
        assert set(row) == set(COLUMNS)
    rep = be.calibration_report(frames, labels, first)
    assert rows[("clean", 0)]["accuracy"] == rep["accuracy"] and rows[("clean", 0)]["nll"] == rep["nll"]
    assert rows[("clean", 0)]["accuracy"] >= 0.5
    assert (be.cfg.temperature, be.cfg.tau) == (float(f32(1.3)), float(f32(0.3)))
    after, conf_after = be.classify(dev[:8])                                                      # the handle's own settings too
    assert torch.equal(after, pred) and torch.equal(conf_after, conf)
    assert len(table(rows).splitlines()) == 2 + len(rows)
    # imagenet_c's output feeds classify as it is, and as the same array uploaded from the host
    blurred = cor.imagenet_c(dev[:8], "gaussian_blur", 2)
    l_dev, c_dev = be.classify(blurred)
    l_host, c_host = be.classify(blurred.cpu().numpy())
    assert np.array_equal(l_dev.cpu().numpy(), l_host) and np.array_equal(c_dev.cpu().numpy(), c_host)
    be.close()
