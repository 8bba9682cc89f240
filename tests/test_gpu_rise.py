"""RISE saliency on the device (include/fav.h): fav_op_rise_mask and fav_op_rise_accumulate against
tests/rise_ref.py, bit for bit with guard bytes around every output, fav_classify_rise against the composition of the ops
through the C ABI, and Backend.classify_rise.  The class-probability head is the one piece that is not new; it is used on both
sides of every comparison here, so everything is compared as bits.  Nothing here says anything about WHERE a synthetic
checkpoint's map peaks: what is verified is the algebra and the bits."""
import ctypes as C

import numpy as np
import pytest

pytestmark = pytest.mark.gpu

import torch  # noqa: E402
import rise_ref as R  # noqa: E402
from perturb_gpu import PAT, Out, dev, frames_of, host, last_error, stream  # noqa: E402
from failure_aware_vision_amd import Backend, _lib, faithfulness, synth, views, weights  # noqa: E402

U8, F32 = _lib.LAYOUT_NHWC_U8, _lib.LAYOUT_NHWC_F32
ids = lambda s: "x".join(map(str, s)) if isinstance(s, tuple) else str(s)  # noqa: E731


@pytest.fixture(scope="module")
def lib():
    assert torch.cuda.is_available(), "GPU tests need a MI355X"
    return _lib.load()


def c_desc(d, struct_size=None):
    c = _lib.FavRise()
    c.struct_size = C.sizeof(_lib.FavRise) if struct_size is None else struct_size
    c.n_masks, c.grid, c.keep, c.seed = d.n_masks, d.grid, d.keep, d.seed
    for k in range(3):
        c.fill_u8[k], c.fill_f32_bits[k] = d.fill_u8[k], d.fill_f32_bits[k]
    return c


def desc_of(dtype, **kw):
    """A descriptor whose fills are awkward: bytes at both ends under uint8; a NaN payload, -0 and 0.5 under fp32."""
    return R.Desc(fill_u8=(17, 255, 0), fill_f32_bits=(0x7FC12345, 0x80000000, 0x3F000000), **kw)


# ---- fav_op_rise_mask ----------------------------------------------------------------------------------------------------
def run_mask(lib, frames, d, first, m0, m1, in_off=0, out_off=0, single=False):
    """-> the output [m1 - m0, n, H, W, 3] (guards checked).  single: one launch a mask, each into its slice."""
    n, H_, W, _ = frames.shape
    raw = np.ascontiguousarray(frames).view(np.uint8).ravel()
    inbuf = torch.zeros(raw.size + 32, dtype=torch.uint8, device="cuda")
    inbuf[in_off:in_off + raw.size] = torch.from_numpy(raw).cuda()
    out = Out(raw.size * (m1 - m0), out_off)
    layout = U8 if frames.dtype == np.uint8 else F32
    cd = c_desc(d)
    for a, b in ([(m, m + 1) for m in range(m0, m1)] if single else [(m0, m1)]):
        st = lib.fav_op_rise_mask(inbuf.data_ptr() + in_off, out.ptr + (a - m0) * raw.size, n, H_, W, layout, C.byref(cd), first, a, b,
                                  stream())
        assert st == 0, last_error(lib)
    torch.cuda.synchronize()
    return out.get(frames.dtype, (m1 - m0, n, H_, W, 3))


def masked_equal(got, want, mq):
    """uint8: equal.  fp32: an element under mq 0 or 256 is a copy and compares as bits; an element under a partial weight
    compares as bits unless the reference is a NaN, and then the device's must be one too."""
    if got.shape != want.shape or got.dtype != want.dtype:
        return False
    if got.dtype == np.uint8:
        return bool(np.array_equal(got, want))
    g, w = got.view(np.uint32), want.view(np.uint32)
    copied = np.broadcast_to(((mq == 0) | (mq == 256))[..., None], got.shape)
    nan = np.isnan(want) & ~copied
    return bool((g[~nan] == w[~nan]).all() and np.isnan(got[nan]).all())


MASK_SIZES = ((1, 1), (5, 7), (8, 12), (13, 9), (32, 32))


@pytest.mark.parametrize("hw", MASK_SIZES, ids=ids)
def test_op_rise_mask_bit_exact(lib, hw):
    H_, W = hw
    for dtype in (np.uint8, np.float32):
        for n in (1, 3):
            frames = frames_of(n, H_, W, dtype, seed=n)
            for g in (1, 2, 7, 15):
                if g > min(H_, W):
                    continue
                for keep in (1, 128, 255):
                    d = desc_of(dtype, n_masks=5, grid=g, keep=keep, seed=(g << 40) | (keep << 8) | n)
                    first = 3 + 100 * n
                    want, mq = R.rise_mask(frames, d, first, 0, 5)
                    what = (dtype.__name__, n, g, keep)
                    assert masked_equal(run_mask(lib, frames, d, first, 0, 5), want, mq), what
                    if keep == 128:
                        assert masked_equal(run_mask(lib, frames, d, first, 0, 5, single=True), want, mq), what
                        assert masked_equal(run_mask(lib, frames, d, first, 1, 4), want[1:4], mq[1:4]), what      # a range in the middle


def test_op_rise_mask_more_masks_than_a_staged_chunk(lib):
    frames = frames_of(2, 13, 9, np.uint8)
    d = desc_of(np.uint8, n_masks=21, grid=3, keep=128, seed=77)
    want, mq = R.rise_mask(frames, d, 5, 0, 21)
    assert masked_equal(run_mask(lib, frames, d, 5, 0, 21), want, mq)
    assert masked_equal(run_mask(lib, frames, d, 5, 2, 19), want[2:19], mq[2:19])


@pytest.mark.parametrize("in_off,out_off", ((0, 0), (1, 0), (2, 3), (3, 1), (0, 2)))
def test_op_rise_mask_u8_byte_offsets(lib, in_off, out_off):
    frames = frames_of(3, 9, 13, np.uint8, seed=in_off)
    d = desc_of(np.uint8, n_masks=3, grid=2, keep=128, seed=in_off * 4 + out_off)
    want, mq = R.rise_mask(frames, d, 9, 0, 3)
    assert masked_equal(run_mask(lib, frames, d, 9, 0, 3, in_off, out_off), want, mq)
    assert ((mq > 0) & (mq < 256)).any()


@pytest.mark.parametrize("dtype", (np.uint8, np.float32), ids=("u8", "f32"))
def test_op_rise_mask_one_large_frame_size(lib, dtype):
    frames = frames_of(2, 224, 224, dtype)
    d = desc_of(dtype, n_masks=3, grid=7, keep=128, seed=224)
    want, mq = R.rise_mask(frames, d, 40, 0, 3)
    assert masked_equal(run_mask(lib, frames, d, 40, 0, 3), want, mq)


def test_op_rise_mask_frame_index_wraps_with_the_low_word(lib):
    frames = frames_of(3, 13, 9, np.uint8)
    d = desc_of(np.uint8, n_masks=2, grid=3, keep=128, seed=0xABCDEF0123456789)
    first = 2 ** 32 - 2                                                         # frames -2, -1 and 0 of the low word
    want, mq = R.rise_mask(frames, d, first, 0, 2)
    got = run_mask(lib, frames, d, first, 0, 2)
    assert masked_equal(got, want, mq)
    assert np.array_equal(got[:, 2:], run_mask(lib, frames[2:], d, 0, 0, 2))    # the third frame has index 0
    assert np.array_equal(got, run_mask(lib, frames, d, first + 5 * 2 ** 32, 0, 2))   # only the low word counts
    assert not np.array_equal(got[:, :1], run_mask(lib, frames[:1], d, 0, 0, 2))


@pytest.mark.parametrize("hw,g", (((5, 7), 2), ((32, 32), 7), ((33, 47), 15)), ids=ids)
def test_op_rise_mask_of_ones_over_a_zero_fill_is_the_mask_itself(lib, hw, g):
    H_, W = hw
    ones = np.ones((2, H_, W, 3), np.float32)
    d = R.Desc(n_masks=4, grid=g, keep=128, seed=31, fill_f32_bits=(0, 0, 0))
    got = run_mask(lib, ones, d, 17, 0, 4)
    mq = R.masks(d, 17, 2, H_, W, 0, 4)
    assert np.array_equal(got, np.repeat((mq / 256.0).astype(np.float32)[..., None], 3, axis=-1))
    assert ((mq > 0) & (mq < 256)).any()


def test_op_rise_mask_refusals_launch_nothing(lib):
    frame_bytes = 8 * 8 * 3
    frames = torch.full((2 * frame_bytes * 4 + 64,), 7, dtype=torch.uint8, device="cuda")
    out = torch.full((5 * 2 * frame_bytes * 4 + 64,), PAT, dtype=torch.uint8, device="cuda")
    f, o = frames.data_ptr(), out.data_ptr()
    ok = R.Desc(n_masks=5, grid=3, keep=128, seed=1, fill_u8=(1, 2, 3))

    def args(frames_=f, out_=o, n=2, H_=8, W=8, layout=U8, d=ok, first=0, m0=0, m1=5, struct_size=None, null_desc=False):
        return (frames_, out_, n, H_, W, layout, None if null_desc else C.byref(c_desc(d, struct_size)), first, m0, m1)
    cases = [("null frames", args(frames_=None), "null"), ("null out", args(out_=None), "null"), ("null desc", args(null_desc=True), "NULL"),
             ("struct_size", args(struct_size=40), "struct_size"), ("m0 == m1", args(m0=3, m1=3), "masks [3, 3)"),
             ("m0 > m1", args(m0=4, m1=3), "masks [4, 3)"), ("m0 < 0", args(m0=-1, m1=3), "masks [-1, 3)"), ("m1 > N", args(m1=6), "masks [0, 6)"),
             ("N 0", args(d=ok._replace(n_masks=0)), "n_masks=0"), ("N 8193", args(d=ok._replace(n_masks=8193)), "n_masks=8193"),
             ("g 0", args(d=ok._replace(grid=0)), "grid=0"), ("g 16", args(d=ok._replace(grid=16)), "grid=16"),
             ("g above the frame", args(d=ok._replace(grid=9)), "grid=9 above min(H, W)=8"), ("keep 0", args(d=ok._replace(keep=0)), "keep=0"),
             ("keep 256", args(d=ok._replace(keep=256)), "keep=256"), ("fill 256", args(d=ok._replace(fill_u8=(1, 256, 3))), "fill[1]=256"),
             ("n 0", args(n=0), "at least 1"), ("H 0", args(H_=0), "at least 1"), ("layout", args(layout=2), "layout"),
             ("f32 frames + 2", args(frames_=f + 2, layout=F32, m1=1), "aligned"), ("f32 out + 1", args(out_=o + 1, layout=F32, m1=1), "aligned"),
             ("out == frames", args(out_=f, m1=1), "overlaps"), ("out in frames", args(out_=f + 2 * frame_bytes - 1, m1=1), "overlaps"),
             ("frames in out", args(frames_=o + 3 * frame_bytes), "overlaps"),
             ("out end on frames", args(frames_=o + 2 * 2 * frame_bytes - 1, m1=2), "overlaps")]
    for why, a, text in cases:
        st = lib.fav_op_rise_mask(*a, stream())
        torch.cuda.synchronize()
        msg = last_error(lib)
        assert st == 1 and "fav_op_rise_mask" in msg and text in msg, (why, msg)
        assert bool((out == PAT).all()) and bool((frames == 7).all()), why
    # the fill's range is uint8's alone, and touching ranges do not overlap
    assert lib.fav_op_rise_mask(*args(layout=F32, d=ok._replace(fill_u8=(1, 256, 3)), m1=1), stream()) == 0
    assert lib.fav_op_rise_mask(*args(frames_=o + 2 * 2 * frame_bytes, m1=2), stream()) == 0
    torch.cuda.synchronize()


# ---- fav_op_rise_accumulate ----------------------------------------------------------------------------------------------
def run_acc(lib, prob, classes, d, first, H_, W, mh, mw, num_classes=0):
    n = prob.shape[1]
    mp, rec = Out(n * mh * mw * 4), Out(n * 32)
    p, c = dev(np.asarray(prob, np.float32)), dev(np.asarray(classes, np.int32))       # kept alive until the launch has run
    st = lib.fav_op_rise_accumulate(p.data_ptr(), c.data_ptr(), n, C.byref(c_desc(d)), first, H_, W, mh, mw, num_classes, mp.ptr, rec.ptr,
                                    stream())
    assert st == 0, last_error(lib)
    torch.cuda.synchronize()
    return mp.get(np.float32, (n, mh * mw)), rec.get(np.int32, (n, 8))


def same_map_bits(got, want):
    g, w = np.ascontiguousarray(got).view(np.uint32), np.ascontiguousarray(want).view(np.uint32)
    return got.shape == want.shape and bool(((g == w) | (np.isnan(got) & np.isnan(want))).all())


def planes(N, n, seed, specials=False):
    """fp32 [N + 1, n] probabilities; specials: frame 0 keeps numbers, the others meet NaN, both infinities and -0 on the way."""
    rng = np.random.default_rng(seed)
    p = rng.random((N + 1, n)).astype(np.float32)
    if specials:
        vals = np.array([np.nan, np.inf, -np.inf, -0.0], np.float32)
        for i in range(1, n):
            rows = rng.permutation(N)[:min(N, 2)] + 1
            p[rows, i] = vals[(np.arange(rows.size) + 2 * i) % 4]
        if N >= 2:
            p[1, 0] = -0.0
    return p


ACC_MAPS = ((1, 1), (1, 2), (7, 7), (14, 14), (32, 32))


@pytest.mark.parametrize("n", (1, 3))
@pytest.mark.parametrize("N", (1, 2, 65, 300))
def test_op_rise_accumulate_bit_exact(lib, N, n):
    combos = [(size, m) for size in (32, 224) for m in ACC_MAPS] if N <= 65 else [(224, (14, 14)), (32, (32, 32)), (32, (1, 2))]
    for k, (size, (mh, mw)) in enumerate(combos):
        d = R.Desc(n_masks=N, grid=(1, 3, 7, 15)[k % 4], keep=(128, 40, 230)[k % 3], seed=1000 * N + k)
        prob = planes(N, n, seed=N + k, specials=k % 2 == 1)
        classes = np.arange(n, dtype=np.int32) + k
        want_map, want_rec, _ = R.accumulate(prob, classes, d, 50 + k, size, size, mh, mw)
        got_map, got_rec = run_acc(lib, prob, classes, d, 50 + k, size, size, mh, mw)
        what = (size, mh, mw, d.grid, d.keep)
        assert same_map_bits(got_map, want_map), what
        assert R.same_records(got_rec, want_rec), (what, got_rec, want_rec)


def test_op_rise_accumulate_carries_non_finite_probabilities(lib):
    N, n = 9, 4
    d = R.Desc(n_masks=N, grid=3, keep=200, seed=3)
    prob = np.random.default_rng(1).random((N + 1, n)).astype(np.float32)
    prob[4, 0], prob[2, 1], prob[7, 1], prob[5, 2] = np.nan, np.inf, -np.inf, -0.0
    prob[0, 3] = np.nan                                                         # p_full alone
    want_map, want_rec, cov = R.accumulate(prob, np.zeros(n, np.int32), d, 0, 32, 32, 7, 7)
    got_map, got_rec = run_acc(lib, prob, np.zeros(n, np.int32), d, 0, 32, 32, 7, 7)
    assert same_map_bits(got_map, want_map) and R.same_records(got_rec, want_rec)
    assert np.isnan(got_map[0]).all() and np.isnan(got_map[1]).any() and not np.isnan(got_map[2:]).any()
    # an all-NaN map has no peak: the scans' starting values stand
    assert got_rec[0, 3] == -1 and got_rec[0, 6] == 0 and got_rec[0, 7] == -1
    assert got_rec[0, 2:3].view(np.float32)[0] == -np.inf and got_rec[0, 4:5].view(np.float32)[0] == np.inf
    assert np.isnan(got_rec[3, 1:2].view(np.float32)[0]) and not np.isnan(got_rec[3, 5:6].view(np.float32)[0])


def test_op_rise_accumulate_cells_without_coverage_are_plus_zero(lib):
    d = R.Desc(n_masks=2, grid=1, keep=1, seed=11)
    hit = None
    for first in range(0, 4096, 4):                      # keep = 1: one grid bit in 256 is ON - look for frames with some coverage
        _, _, cov = R.accumulate(np.ones((3, 4), np.float32), np.zeros(4, np.int32), d, first, 32, 32, 4, 4)
        if (cov > 0).any():
            hit = first
            break
    assert hit is not None
    prob = planes(2, 4, seed=2)
    want_map, want_rec, cov = R.accumulate(prob, np.zeros(4, np.int32), d, hit, 32, 32, 4, 4)
    got_map, got_rec = run_acc(lib, prob, np.zeros(4, np.int32), d, hit, 32, 32, 4, 4)
    assert (cov == 0).any() and (cov > 0).any()
    assert same_map_bits(got_map, want_map) and R.same_records(got_rec, want_rec)
    assert (got_map.view(np.uint32)[cov == 0] == 0).all()


@pytest.mark.parametrize("N", (65, 300))
def test_op_rise_accumulate_of_a_constant_probability_is_that_constant(lib, N):
    k = np.float32(0.3)
    d = R.Desc(n_masks=N, grid=7, keep=128, seed=N)
    prob = np.full((N + 1, 2), k, np.float32)
    _, _, cov = R.accumulate(prob, np.zeros(2, np.int32), d, 0, 224, 224, 14, 14)
    got_map, got_rec = run_acc(lib, prob, np.zeros(2, np.int32), d, 0, 224, 224, 14, 14)
    err = np.abs(got_map[cov > 0].astype(np.float64) - float(k))
    print(f"N={N}: max |M - k| = {err.max():.3e}, bound {2 * N * float(np.spacing(k)):.3e}")
    assert (cov > 0).all() and err.max() <= 2 * N * float(np.spacing(k))      # N rounded additions: the bound is not tuned


def test_op_rise_accumulate_class_outside_the_range(lib):
    N, n = 5, 4
    d = R.Desc(n_masks=N, grid=3, keep=128, seed=9)
    prob = planes(N, n, seed=4)
    classes = np.array([-1, 10, 9, 2 ** 31 - 1], np.int32)
    bad = [-1, R.NAN_BITS, R.NAN_BITS, -1, R.NAN_BITS, R.NAN_BITS, 0, -1]
    for num_classes, out_of_range in ((0, (0,)), (10, (0, 1, 3))):
        want_map, want_rec, _ = R.accumulate(prob, classes, d, 1, 32, 32, 4, 4, num_classes)
        got_map, got_rec = run_acc(lib, prob, classes, d, 1, 32, 32, 4, 4, num_classes)
        assert same_map_bits(got_map, want_map) and R.same_records(got_rec, want_rec)
        for i in range(n):
            assert (got_rec[i].tolist() == bad) == (i in out_of_range), (num_classes, i)


def test_op_rise_accumulate_refusals_launch_nothing(lib):
    ok = R.Desc(n_masks=4, grid=3, keep=128, seed=1)
    p, c = dev(np.zeros((5, 3), np.float32)), dev(np.zeros(3, np.int32))
    mp, rec = Out(3 * 16 * 4), Out(3 * 32)

    def args(prob=p.data_ptr(), classes=c.data_ptr(), n=3, d=ok, first=0, H_=32, W=32, mh=4, mw=4, num_classes=0, map_=mp.ptr, rec_=rec.ptr,
             null_desc=False):
        return (prob, classes, n, None if null_desc else C.byref(c_desc(d)), first, H_, W, mh, mw, num_classes, map_, rec_)
    for why, a, text in (("null prob", args(prob=None), "null"), ("null classes", args(classes=None), "null"), ("null map", args(map_=None), "null"),
                         ("null rec", args(rec_=None), "null"), ("null desc", args(null_desc=True), "NULL"), ("n 0", args(n=0), "at least 1"),
                         ("N 0", args(d=ok._replace(n_masks=0)), "n_masks=0"), ("g 16", args(d=ok._replace(grid=16)), "grid=16"),
                         ("keep 256", args(d=ok._replace(keep=256)), "keep=256"), ("g above the frame", args(H_=2), "grid=3 above min(H, W)=2"),
                         ("map 0", args(mh=0), "map 0x4"), ("map 1025", args(mh=25, mw=41, H_=64, W=64), "map 25x41"),
                         ("map side", args(mh=257, mw=1, H_=300), "map 257x1"), ("map finer than the frame", args(mh=33, mw=4), "finer"),
                         ("num_classes", args(num_classes=-1), "num_classes=-1"), ("rec + 4", args(rec_=rec.ptr + 4), "8-byte"),
                         ("map + 2", args(map_=mp.ptr + 2), "4-byte"), ("prob + 1", args(prob=p.data_ptr() + 1), "4-byte")):
        st = lib.fav_op_rise_accumulate(*a, stream())
        torch.cuda.synchronize()
        assert st == 1 and "fav_op_rise_accumulate" in last_error(lib) and text in last_error(lib), (why, last_error(lib))
        assert mp.untouched() and rec.untouched(), why
    assert lib.fav_op_rise_accumulate(*args(), stream()) == 0
    torch.cuda.synchronize()


# ---- through a handle ----------------------------------------------------------------------------------------------------
MAX_BATCH, FIRST, D, MAP = R.E2E_MAX_BATCH, R.E2E_FIRST, R.E2E_DESC, R.E2E_MAP
HANDLES = ("resnet18_mc", "vit_tiny", "ensemble")


def make_backend(kind, **kw):
    if kind == "vit_tiny":
        blob, _ = weights.make_synthetic_vit("vit_tiny", seed=3)
        return Backend("vit_tiny", blob, max_batch=MAX_BATCH, **kw), 64
    if kind == "ensemble":
        blobs = [weights.make_synthetic("resnet18_cifar", seed=s)[0] for s in (1, 2)]
        return Backend("resnet18_cifar", blobs, max_batch=MAX_BATCH, **kw), 32
    blob, _ = weights.make_synthetic("resnet18_cifar", seed=1)
    if kind == "resnet18_mc":
        kw = dict(kw, n_samples=3, dropout_policy="all_blocks", dropout_p=0.1, seed=4)
    return Backend("resnet18_cifar", blob, max_batch=MAX_BATCH, **kw), 32


def set_e2e(be):
    be.set_rise(D.n_masks, grid=D.grid, keep=D.keep / 256.0, seed=D.seed, fill=(0.25, 0.5, 1.0))


@pytest.fixture(scope="module", params=HANDLES)
def handle(request):
    """(backend with the end-to-end descriptor set, its frames uint8 [MAX_BATCH, S, S, 3] on the device)."""
    be, size = make_backend(request.param, temperature=1.3)
    assert size in R.E2E_SIZES
    set_e2e(be)
    yield request.param, be, dev(synth.synthetic_frames_u8(MAX_BATCH, size, size, seed=21))
    be.close()


def call_rise(be, frames_dev, classes, first, mhw=MAP):
    """fav_classify_rise through the C ABI -> (map, records, label, confidence), numpy, guards checked."""
    n = int(frames_dev.shape[0])
    layout = U8 if frames_dev.dtype == torch.uint8 else F32
    mp, rec, lab, conf = Out(n * mhw[0] * mhw[1] * 4), Out(n * 32), Out(n * 4), Out(n * 4)
    cls = dev(np.asarray(classes, np.int32)) if classes is not None else None
    _lib.check(be.lib.fav_classify_rise(be._h, frames_dev.data_ptr(), n, layout, first, cls.data_ptr() if cls is not None else None, mhw[0],
                                        mhw[1], lab.ptr, conf.ptr, mp.ptr, rec.ptr, stream()), be._h)
    torch.cuda.synchronize()
    return mp.get(np.float32, (n, mhw[0] * mhw[1])), rec.get(np.int32, (n, 8)), lab.get(np.int32, (n,)), conf.get(np.float32, (n,))


def compose(be, frames_dev, classes, first, mhw=MAP):
    """fav_classify_rise restated with the public ops through the C ABI -> (map, records, label, confidence), numpy."""
    lib, h, s = be.lib, be._h, stream()
    n, fh, fw = (int(v) for v in frames_dev.shape[:3])
    layout = U8 if frames_dev.dtype == torch.uint8 else F32
    Cc = int(be.cfg.num_classes)
    ld = (Cc + 3) // 4 * 4
    cd = c_desc(D)
    masked = torch.empty_like(frames_dev)
    prob = torch.empty((D.n_masks + 1, n), dtype=torch.float32, device="cuda")
    lab0 = torch.empty(n, dtype=torch.int32, device="cuda")
    conf0 = torch.empty(n, dtype=torch.float32, device="cuda")
    scratch_l, scratch_c = torch.empty_like(lab0), torch.empty_like(conf0)
    cls = dev(np.asarray(classes, np.int32)) if classes is not None else lab0
    for k in range(D.n_masks + 1):
        src = frames_dev
        if k > 0:
            _lib.check(lib.fav_op_rise_mask(frames_dev.data_ptr(), masked.data_ptr(), n, fh, fw, layout, C.byref(cd), first, k - 1, k, s))
            src = masked
        _lib.check(lib.fav_classify_ex(h, src.data_ptr(), n, layout, first, (lab0 if k == 0 else scratch_l).data_ptr(),
                                       (conf0 if k == 0 else scratch_c).data_ptr(), None, None, s), h)
        lg = be.logits()
        padded = torch.full((lg.shape[0], n, ld), float("nan"), dtype=torch.float32, device="cuda")
        padded[:, :, :Cc] = lg
        _lib.check(lib.fav_op_head_class_prob(padded.data_ptr(), int(lg.shape[0]), n, Cc, ld, float(be.cfg.temperature), cls.data_ptr(),
                                              prob[k].data_ptr(), None, s))
    mp = torch.empty((n, mhw[0] * mhw[1]), dtype=torch.float32, device="cuda")
    rec = torch.empty((n, 8), dtype=torch.int32, device="cuda")
    _lib.check(lib.fav_op_rise_accumulate(prob.data_ptr(), cls.data_ptr(), n, C.byref(cd), first, fh, fw, mhw[0], mhw[1], Cc, mp.data_ptr(),
                                          rec.data_ptr(), s))
    torch.cuda.synchronize()
    return mp.cpu().numpy(), rec.cpu().numpy(), lab0.cpu().numpy(), conf0.cpu().numpy(), prob.cpu().numpy()


@pytest.mark.parametrize("n", (1, 3, MAX_BATCH))
def test_classify_rise_equals_the_composition_of_the_ops(handle, n):
    kind, be, frames = handle
    fd = frames[:n].contiguous()
    Cc = int(be.cfg.num_classes)
    plain_lab, plain_conf = (host(v) for v in be.classify_detect(fd, first_index=FIRST)[:2])
    for classes in (None, (np.arange(n, dtype=np.int32) * 3 + 1) % Cc):
        mp, rec, lab, conf = call_rise(be, fd, classes, FIRST)
        wmp, wrec, wlab, wconf, prob = compose(be, fd, classes, FIRST)
        assert same_map_bits(mp, wmp) and R.same_records(rec, wrec), (kind, n, rec, wrec)
        # the unmasked pass is a plain fav_classify_ex call on the frames
        assert np.array_equal(lab, plain_lab) and np.array_equal(conf.view(np.uint32), plain_conf.view(np.uint32)), kind
        assert np.array_equal(wlab, plain_lab) and np.array_equal(wconf.view(np.uint32), plain_conf.view(np.uint32)), kind
        assert np.array_equal(rec[:, 0], plain_lab if classes is None else classes)
        # the head itself against numpy, on the probabilities the composition saw; tests/test_rise_host.py holds cov > 0 here
        ref_map, ref_rec, cov = R.accumulate(prob, rec[:, 0], D, FIRST, int(fd.shape[1]), int(fd.shape[2]), *MAP, Cc)
        assert (cov > 0).all() and same_map_bits(mp, ref_map) and R.same_records(rec, ref_rec), kind
        assert not np.isnan(mp).any()
        # the same call again: every pass of a frame draws the same MC-Dropout masks
        mp2, rec2, lab2, conf2 = call_rise(be, fd, classes, FIRST)
        assert same_map_bits(mp2, mp) and np.array_equal(rec2, rec) and np.array_equal(lab2, lab), kind
    # afterwards the logits are the last masked pass's
    call_rise(be, fd, None, FIRST)
    last = host(be.logits())
    masked = torch.empty_like(fd)
    _lib.check(be.lib.fav_op_rise_mask(fd.data_ptr(), masked.data_ptr(), n, int(fd.shape[1]), int(fd.shape[2]), U8, C.byref(c_desc(D)), FIRST,
                                       D.n_masks - 1, D.n_masks, stream()))
    be.classify_detect(masked, first_index=FIRST)
    assert np.array_equal(last.view(np.uint32), host(be.logits()).view(np.uint32)), kind


def test_classify_rise_takes_fp32_frames_and_classes_outside_the_range(handle):
    kind, be, frames = handle
    twins = (frames[:3].to(torch.float32) / 255.0).contiguous()
    mp, rec, lab, conf = call_rise(be, twins, None, 7)
    wmp, wrec, wlab, wconf, _ = compose(be, twins, None, 7)
    assert same_map_bits(mp, wmp) and R.same_records(rec, wrec) and np.array_equal(lab, wlab), kind
    Cc = int(be.cfg.num_classes)
    mp, rec, _, _ = call_rise(be, frames[:4].contiguous(), np.array([0, Cc, -1, Cc - 1], np.int32), FIRST)
    bad = [-1, R.NAN_BITS, R.NAN_BITS, -1, R.NAN_BITS, R.NAN_BITS, 0, -1]
    assert rec[1].tolist() == bad and rec[2].tolist() == bad and np.isnan(mp[1:3]).all(), kind
    assert rec[0, 0] == 0 and rec[3, 0] == Cc - 1 and not np.isnan(mp[[0, 3]]).any()


# ---- a frame size neither the grid nor the map divides -------------------------------------------------------------------
ODD_HW = (31, 45)


@pytest.fixture(scope="module")
def odd_handle():
    """One ResNet-18 MC-Dropout handle at 31 x 45 with the end-to-end descriptor: grid 3, so a mask cell is ceil(31 / 3) = 11 by
    ceil(45 / 3) = 15 pixels and the 4 x 4 grid of shifted cells overhangs the frame on both axes."""
    be, _ = make_backend("resnet18_mc", in_hw=ODD_HW, temperature=1.3)
    assert R.cell_sizes(*ODD_HW, D.grid) == (11, 15)
    set_e2e(be)
    yield be, synth.synthetic_frames_u8(3, *ODD_HW, seed=21)
    be.close()


@pytest.mark.parametrize("dtype", ("u8", "f32"))
@pytest.mark.parametrize("mhw", ((4, 4), (2, 3)), ids=ids)
def test_classify_rise_at_an_odd_frame_size(odd_handle, lib, mhw, dtype):
    be, frames = odd_handle
    n = frames.shape[0]
    fd = dev(frames) if dtype == "u8" else dev(frames.astype(np.float32) / np.float32(255.0))
    Cc = int(be.cfg.num_classes)
    plain_lab, plain_conf = (host(v) for v in be.classify_detect(fd, first_index=FIRST)[:2])
    # the masked frames of this size are the reference's, not those of a square
    got = run_mask(lib, host(fd), D, FIRST, 0, D.n_masks)
    want, mq = R.rise_mask(host(fd), D, FIRST, 0, D.n_masks)
    assert masked_equal(got, want, mq)
    for classes in (None, (np.arange(n, dtype=np.int32) * 3 + 1) % Cc):
        mp, rec, lab, conf = call_rise(be, fd, classes, FIRST, mhw)
        wmp, wrec, wlab, wconf, prob = compose(be, fd, classes, FIRST, mhw)
        assert same_map_bits(mp, wmp) and R.same_records(rec, wrec), (rec, wrec)
        assert np.array_equal(lab, plain_lab) and np.array_equal(conf.view(np.uint32), plain_conf.view(np.uint32))
        assert np.array_equal(wlab, plain_lab) and np.array_equal(wconf.view(np.uint32), plain_conf.view(np.uint32))
        assert np.array_equal(rec[:, 0], plain_lab if classes is None else classes)
        ref_map, ref_rec, _ = R.accumulate(prob, rec[:, 0], D, FIRST, ODD_HW[0], ODD_HW[1], mhw[0], mhw[1], Cc)
        assert same_map_bits(mp, ref_map) and R.same_records(rec, ref_rec)
        assert not np.isnan(mp).any() and mp.any()


def test_handle_refusals():
    be, size = make_backend("resnet18_mc")
    try:
        frames = dev(synth.synthetic_frames_u8(MAX_BATCH + 1, size, size, seed=3))
        with pytest.raises(_lib.FavError, match="FAV_ERR_INVALID_ARG.*fav_classify_rise: no RISE descriptor set"):
            be.classify_rise(frames[:3])
        with pytest.raises(_lib.FavError, match="FAV_ERR_INVALID_ARG.*fav_set_rise: n_masks=8193"):
            be.set_rise(8193)
        with pytest.raises(_lib.FavError, match="FAV_ERR_INVALID_ARG.*fav_set_rise: grid=16 outside"):
            be.set_rise(4, grid=16)
        with pytest.raises(_lib.FavError, match="FAV_ERR_INVALID_ARG.*fav_set_rise: keep=256"):
            be.set_rise(4, keep=1.0)
        with pytest.raises(_lib.FavError, match="FAV_ERR_INVALID_ARG.*fav_set_rise: fill.*above 255"):
            be.set_rise(4, fill=1.5)
        set_e2e(be)
        be.set_rise(2 * D.n_masks)                                               # replacing
        set_e2e(be)
        be.set_curve(4)                                                          # independent of the curve descriptor
        s = stream()
        mp = torch.full((MAX_BATCH + 1, 1024), 7.0, dtype=torch.float32, device="cuda")
        rec = torch.full((MAX_BATCH + 1, 8), 7, dtype=torch.int32, device="cuda")

        def call(n=3, layout=U8, first=0, mh=MAP[0], mw=MAP[1], frames_=frames.data_ptr(), map_=mp.data_ptr(), rec_=rec.data_ptr(), classes=None):
            st = be.lib.fav_classify_rise(be._h, frames_, n, layout, first, classes, mh, mw, None, None, map_, rec_, s)
            torch.cuda.synchronize()
            return st, be.lib.fav_last_error(be._h).decode()
        for why, kw, text in (("n above max_batch", dict(n=MAX_BATCH + 1), "n=9 outside [1, max_batch=8]"), ("n 0", dict(n=0), "n=0"),
                              ("1025 cells", dict(mh=25, mw=41), "map 25x41"), ("a side of 257", dict(mh=257, mw=1), "map 257x1"),
                              ("finer than the frame", dict(mh=33, mw=2), "finer"), ("map 0", dict(mw=0), "map 4x0"),
                              ("layout", dict(layout=3), "layout"), ("first", dict(first=-1), "first_image_index"),
                              ("first + n", dict(first=2 ** 32 - 3), "first_image_index"), ("null frames", dict(frames_=None), "null"),
                              ("null map", dict(map_=None), "null"), ("null rec", dict(rec_=None), "null"),
                              ("map + 2", dict(map_=mp.data_ptr() + 2), "misaligned"), ("rec + 4", dict(rec_=rec.data_ptr() + 4), "misaligned"),
                              ("classes + 2", dict(classes=rec.data_ptr() + 2), "misaligned"),
                              ("f32 frames + 2", dict(layout=F32, frames_=frames.data_ptr() + 2), "aligned")):
            st, msg = call(**kw)
            assert st == 1 and "fav_classify_rise" in msg and text in msg, (why, msg)
            assert bool((mp == 7.0).all()) and bool((rec == 7).all()), why
        assert call()[0] == 0
        # views against a RISE descriptor, in both orders; the curve descriptor has its own say
        be.set_curve(None)
        with pytest.raises(_lib.FavError, match="FAV_ERR_UNSUPPORTED.*fav_set_views: a RISE descriptor is set"):
            be.set_views(views.hflip())
        be.set_rise(None)
        be.set_rise(None)
    finally:
        be.close()
    be, size = make_backend("resnet18")                                          # a handle that takes views
    try:
        be.set_views(views.hflip())
        with pytest.raises(_lib.FavError, match="FAV_ERR_UNSUPPORTED.*fav_set_rise: views are set"):
            set_e2e(be)
        be.set_views(None)
        set_e2e(be)
        with pytest.raises(_lib.FavError, match="FAV_ERR_UNSUPPORTED.*fav_set_views: a RISE descriptor is set"):
            be.set_views(views.hflip())
        got = be.classify_rise(dev(synth.synthetic_frames_u8(3, size, size, seed=3)), map_hw=MAP)
        assert not np.isnan(host(got["map"])).any()
    finally:
        be.close()


def test_a_rise_descriptor_changes_no_classify_call():
    be, size = make_backend("resnet18_mc")
    try:
        frames = dev(synth.synthetic_frames_u8(5, size, size, seed=3))

        def snapshot():
            be.set_profiling(True)
            lab, conf, fail, score = (host(v) for v in be.classify_detect(frames, first_index=5))
            prof = be.get_profile()
            ops = [(r["op_index"], r["kind"], r["launches"]) for r in be.get_op_profile()]
            be.set_profiling(False)
            return lab, conf, fail, score, host(be.logits()), {k: v["launches"] for k, v in prof.items()}, ops
        before = snapshot()
        set_e2e(be)
        during = snapshot()
        be.classify_rise(frames, map_hw=MAP)
        be.set_rise(3, grid=2)                                                   # replacing
        replaced = snapshot()
        be.set_rise(None)
        after = snapshot()
        for other in (during, replaced, after):
            for a, b in zip(before[:5], other[:5]):
                assert a.shape == b.shape and np.array_equal(a.view(np.uint8), b.view(np.uint8))
            assert before[5] == other[5] and before[6] == other[6]
    finally:
        be.close()


@pytest.mark.parametrize("dtype", ("u8", "f32"))
def test_the_curve_and_rise_heads_share_a_handle_without_cross_talk(dtype):
    """The two heads share a record type and a driver: with both descriptors in force every output of either is, bit for bit,
    what a handle holding that descriptor alone gives, in any order of the calls and after the other descriptor is cleared."""
    n, backends = 3, [make_backend("resnet18")[0] for _ in range(3)]
    both, curve_only, rise_only = backends
    try:
        u8 = synth.synthetic_frames_u8(n, 32, 32, seed=3)
        frames = dev(u8) if dtype == "u8" else dev(u8.astype(np.float32) / np.float32(255.0))
        maps = dev(faithfulness.random_maps(n, (4, 4), 0))

        def bits(r):
            return {k: (v.shape, v.dtype.str, np.ascontiguousarray(v).tobytes()) for k, v in ((k, host(v)) for k, v in r.items())}

        def curve(be):
            return [bits(be.classify_curve(frames, maps, None, mode, first_index=FIRST)) for mode in _lib.CURVE_MODES]

        def rise(be):
            return bits(be.classify_rise(frames, map_hw=(4, 4), heatmap=True, first_index=FIRST))
        for be in (both, curve_only):
            be.set_curve(4)
        for be in (both, rise_only):
            be.set_rise(5, grid=2)
        want_curve, want_rise = curve(curve_only), rise(rise_only)
        assert curve(both) == want_curve
        assert rise(both) == want_rise
        assert curve(both) == want_curve
        both.set_rise(None)
        assert curve(both) == want_curve
        both.set_rise(5, grid=2)
        both.set_curve(None)
        assert rise(both) == want_rise
    finally:
        for be in backends:
            be.close()


def records_of(r):
    cols = [np.ascontiguousarray(host(r[k])) for k in R.REC_NAMES]
    return np.stack([c.view(np.int32) for c in cols], axis=1)


def test_backend_classify_rise(handle, lib):
    kind, be, frames = handle
    size = int(frames.shape[1])
    many = np.concatenate([host(frames), host(frames)[:3]])                      # 11 frames on a handle of 8, numpy in and out
    got = be.classify_rise(many, map_hw=MAP, heatmap=True, first_index=FIRST)
    assert all(isinstance(v, np.ndarray) for v in got.values())
    assert got["map"].shape == (11, *MAP) and got["heatmap"].shape == (11, size, size) and got["heatmap"].dtype == np.uint8
    mp, rec, lab, conf = call_rise(be, frames, None, FIRST)
    assert same_map_bits(got["map"][:MAX_BATCH].reshape(MAX_BATCH, -1), mp) and R.same_records(records_of(got)[:MAX_BATCH], rec)
    assert np.array_equal(got["label"][:MAX_BATCH], lab) and np.array_equal(got["confidence"][:MAX_BATCH].view(np.uint32), conf.view(np.uint32))
    tail = call_rise(be, frames[:3].contiguous(), None, FIRST + MAX_BATCH)       # the second call has first_index advanced
    assert same_map_bits(got["map"][MAX_BATCH:].reshape(3, -1), tail[0]) and R.same_records(records_of(got)[MAX_BATCH:], tail[1])
    # the heatmap is fav_op_cam_heatmap on the returned map and record
    heat = Out(11 * size * size)
    m, r = dev(got["map"]), dev(records_of(got))
    _lib.check(lib.fav_op_cam_heatmap(m.data_ptr(), r.data_ptr(), 11, MAP[0], MAP[1], size, size, heat.ptr, stream()))
    torch.cuda.synchronize()
    assert np.array_equal(heat.get(np.uint8, (11, size, size)), got["heatmap"])
    # torch frames in, torch results out, and a named class
    t = be.classify_rise(frames[:3], classes=np.array([1, 2, 3]), map_hw=(2, 3), first_index=FIRST)
    assert all(torch.is_tensor(v) and v.is_cuda for v in t.values()) and tuple(t["map"].shape) == (3, 2, 3)
    assert host(t["class_id"]).tolist() == [1, 2, 3]


def test_the_rise_map_feeds_faithfulness_report_on_an_ensemble():
    be, size = make_backend("ensemble")
    try:
        frames = dev(synth.synthetic_frames_u8(5, size, size, seed=8))
        set_e2e(be)
        rise_map = be.classify_rise(frames, map_hw=MAP)["map"]
        rep = be.faithfulness_report(frames, steps=4, maps=rise_map)
        assert rep["n"] == 5 and rep["n_nonfinite"] == 0 and rep["map_hw"] == MAP
        for key in ("deletion_auc", "insertion_auc", "random_deletion_auc", "random_insertion_auc"):
            assert np.isfinite(rep[key]), key
        again = be.faithfulness_report(frames, steps=4, maps=be.classify_rise(frames, map_hw=MAP)["map"])
        assert again["deletion_auc"] == rep["deletion_auc"] and again["insertion_auc"] == rep["insertion_auc"]
    finally:
        be.close()
