"""The oldest kernels of the ResNet path at their edges, through the C ABI (fav_op_*): maxpool3x3s2_kernel and
avgpool_kernel at every small / odd / ragged shape against references written here, and the MC-Dropout descriptor
(include/fav.h fav_dropout_desc) on every kernel that draws a mask - the average pool, the entry dropout, the two conv
epilogues, the entry reduce and the bottleneck tail - bit for bit against tests/dropout_ref.py on every entry of
EDGE_DESCRIPTORS.  Each of those kernels computes the Philox counter (chunk, frame, sample, site) with arithmetic of its own;
they all have to land on the reference's.  Then every out-of-range descriptor and every empty shape: refused before anything
is launched.

Which conv shapes reach which epilogue (launch_conv, fav.hip): a launch with a residual that does not take the 256 x 256
tile runs the staged epilogue (EPI = 0, fp32 tile through LDS, one Philox call per 16 channels of a row); every other launch
runs the register epilogue (EPI = 1), where Cout % 128 != 0 selects 64-column tiles whose lanes hold 8 channels (the odd
quad takes draws 8..15 of the call) and Cout % 128 == 0 selects 128-column tiles whose lanes hold all 16.  1 x 1, K = 64:
32-deep steps, three stages.  CONV_VARIANTS names the four.

What the first run on an MI355X showed.  No kernel drew another mask than the reference at any edge: v0 + rows = 2^31 - 1
(fastdiv still exact), t = 2^31 - 2 in entry_dropout_kernel's int, the wrapping frame word, every seed and site.  bf16
subnormals pass the max pool unchanged and are summed, scaled and rounded as the reference does by the average pool and the
entry dropout.  The defects were all in the argument checks: fav_op_avgpool and fav_op_entry_dropout took any v0, no entry
point looked at threshold, scale or n_img, and the pools, the entry dropout and fav_op_stem_im2col launched on empty shapes
(71 of the 73 cases of test_rejections_launch_nothing were not refused before)."""
import ctypes as C

import numpy as np
import pytest

pytestmark = pytest.mark.gpu

torch = pytest.importorskip("torch")
import dropout_ref as R  # noqa: E402
from failure_aware_vision_amd import _lib  # noqa: E402
from oracle import fav_oracle as O  # noqa: E402
from test_gpu_ops import assert_one_ulp, dev_bf16, drop_desc, run_conv  # noqa: E402
from test_gpu_tail import CASES as TAIL_CASES, run_tail  # noqa: E402

GUARD = 4096                     # bf16 elements on either side of an output
FILL = 3.0                       # bf16 0x4040
BF16_MAX = float(O.bf16_from_bits(np.array([0x7F7F], np.uint16))[0])


@pytest.fixture(scope="module")
def lib():
    assert torch.cuda.is_available(), "GPU tests need a MI355X"
    return _lib.load()


def dev_bits(x):
    """fp32 array of bf16-representable values -> device bf16 tensor with exactly those bits (no conversion on the way:
    subnormals, infinities and -0 arrive as they are)."""
    x = np.ascontiguousarray(x, np.float32)
    assert not (x.view(np.uint32) & np.uint32(0xFFFF)).any(), "not bf16-representable"
    return torch.from_numpy(O.bf16_bits(x).view(np.int16).reshape(x.shape)).cuda().view(torch.bfloat16)


def host_bits(t):
    """device bf16 tensor -> fp32 array, bit for bit."""
    return O.bf16_from_bits(t.contiguous().view(torch.int16).cpu().numpy().view(np.uint16))


class Guarded:
    """A bf16 output of `shape` with GUARD (or more) filled elements on either side."""

    def __init__(self, shape, guard=GUARD):
        self.shape, self.guard = tuple(shape), guard
        self.big = torch.full((int(np.prod(shape)) + 2 * guard,), FILL, dtype=torch.bfloat16, device="cuda")
        self.ptr = self.big.data_ptr() + 2 * guard

    def value(self):
        g = self.guard
        assert bool((self.big[:g] == FILL).all()) and bool((self.big[-g:] == FILL).all()), "the guard band was written"
        return host_bits(self.big[g:-g]).reshape(self.shape)


def cdesc(d):
    return drop_desc(d.site, d.threshold, float(R.scale_of(d.threshold)), d.seed, d.v0, d.n_img, d.first_image_index)


def spread(rng, shape, positive=False):
    """bf16 values of mixed sign with magnitudes spread over 2^-8 .. 2^8: the order of an fp32 sum shows."""
    v = rng.uniform(1.0, 2.0, shape) * np.exp2(rng.integers(-8, 9, shape))
    if not positive:
        v = v * rng.choice([-1.0, 1.0], shape)
    return O.bf16_round(v.astype(np.float32))


def subnormals(rng, shape):
    """bf16 subnormals of either sign (mantissa 1..127, exponent field 0)."""
    bits = rng.integers(1, 128, shape).astype(np.uint16) | (rng.integers(0, 2, shape).astype(np.uint16) << 15)
    return O.bf16_from_bits(bits)


# ---------------------------------------------------------------------------------------------------------------------
# max pool
# ---------------------------------------------------------------------------------------------------------------------
def maxpool_taps(x):
    """[9, n, Ho, Wo, C]: the nine taps of every 3x3 / stride 2 / pad 1 window, -inf outside the frame."""
    n, H, W, Cc = x.shape
    Ho, Wo = (H - 1) // 2 + 1, (W - 1) // 2 + 1
    xp = np.full((n, 2 * Ho + 1, 2 * Wo + 1, Cc), -np.inf, np.float32)
    xp[:, 1:1 + H, 1:1 + W] = x
    return np.stack([xp[:, r:r + 2 * Ho:2, s:s + 2 * Wo:2] for r in range(3) for s in range(3)])


def maxpool_ref(x):
    return maxpool_taps(x).max(axis=0)           # order-free; the pool rounds nothing; a NaN tap inside the frame gives NaN (np.max)


def maxpool_inputs(rng, n, H, W, Cc):
    shape = (n, H, W, Cc)
    out = {}
    out["all_negative"] = -spread(rng, shape, positive=True)          # a zero padding value would win at every border
    x = spread(rng, shape)
    x[rng.random(shape) < 0.15] = np.inf
    x[rng.random(shape) < 0.30] = -np.inf
    x[0, :, :, 0] = -np.inf                                           # a channel whose every window is -inf throughout
    out["infinities"] = x
    x = spread(rng, shape)
    x[rng.random(shape) < 0.2] = BF16_MAX
    x[rng.random(shape) < 0.2] = -BF16_MAX
    out["largest_finite"] = x
    out["subnormals"] = subnormals(rng, shape)                        # must come through unchanged, not flushed
    # NaNs of either sign (0x7FC0, 0xFFC0 - the matrix unit makes the latter) beside finite values and both infinities: a window
    # with a NaN tap is NaN whatever else it holds; channel 1 of frame 0 has none
    x = spread(rng, shape)
    x[rng.random(shape) < 0.1] = np.inf
    x[rng.random(shape) < 0.1] = -np.inf
    nans = O.bf16_from_bits(np.array([0x7FC0, 0xFFC0], np.uint16))
    sel = rng.random(shape)
    x[sel < 0.08], x[sel > 0.92] = nans[0], nans[1]
    if Cc > 1:
        x[0, :, :, 1] = spread(rng, (H, W))
    out["nans"] = x
    # every (frame, channel) plane a permutation of distinct integers (exact in bf16 up to 256): the maximum of a window
    # is at exactly one tap, and which one changes from window to window
    assert H * W <= 256
    out["distinct"] = (rng.permuted(np.tile(np.arange(H * W, dtype=np.float32), (n, Cc, 1)), axis=2)
                       .reshape(n, Cc, H, W).transpose(0, 2, 3, 1) - np.float32(H * W // 2)).copy()
    return out


def run_maxpool(lib, x):
    n, H, W, Cc = x.shape
    y = Guarded((n, (H - 1) // 2 + 1, (W - 1) // 2 + 1, Cc))
    xd = dev_bits(x)
    _lib.check(lib.fav_op_maxpool3x3s2(xd.data_ptr(), y.ptr, n, H, W, Cc, None))
    torch.cuda.synchronize()
    return y.value()


SMALL, SECOND = (1, 2, 3, 4, 5, 8), (1, 2, 7)
MAXPOOL_HW = sorted({(a, b) for a in SMALL for b in SECOND} | {(b, a) for a in SMALL for b in SECOND})


@pytest.mark.parametrize("H,W", MAXPOOL_HW, ids=[f"{h}x{w}" for h, w in MAXPOOL_HW])
def test_maxpool_small_frames_bit_exact(lib, H, W):
    rng = np.random.default_rng(H * 16 + W)
    for Cc in (8, 24, 64):                       # 24: a multiple of 8 that is not a multiple of 16
        for n in (1, 3):
            for kind, x in maxpool_inputs(rng, n, H, W, Cc).items():
                ref = maxpool_ref(x)
                got = run_maxpool(lib, x)
                assert got.shape == ref.shape
                # by value: -0 == +0 (fmaxf does not order them); a NaN equals a NaN whatever its pattern
                assert np.array_equal(got, ref, equal_nan=True), f"{kind} n={n} C={Cc}: {np.mean(got != ref):.4f} of elements differ"
                if kind == "nans":
                    assert np.isnan(ref).any() == np.isnan(x).any() and not np.isnan(ref[0, :, :, 1]).any()
                if kind == "subnormals":
                    assert np.all(got != 0) and np.all(np.abs(got) < np.finfo(np.float32).tiny)
                if kind == "all_negative":
                    assert np.all(got < 0)


def test_maxpool_ragged_launch_and_every_tap(lib):
    """More than 256 work items (8 channels of one output pixel each), not a multiple of 256: a ragged last block; and on
    the distinct-valued frame the maximum sits at each of the nine taps somewhere."""
    n, H, W, Cc = 3, 9, 11, 24
    items = n * 5 * 6 * (Cc // 8)
    assert items > 256 and items % 256 != 0
    rng = np.random.default_rng(911)
    for kind, x in maxpool_inputs(rng, n, H, W, Cc).items():
        got = run_maxpool(lib, x)
        assert np.array_equal(got, maxpool_ref(x), equal_nan=True), kind
    taps = maxpool_taps(maxpool_inputs(rng, n, H, W, Cc)["distinct"])
    assert set(np.unique(taps.argmax(axis=0))) == set(range(9))


# ---------------------------------------------------------------------------------------------------------------------
# average pool
# ---------------------------------------------------------------------------------------------------------------------
def avgpool_seq(x):
    """The contract (O.global_avgpool states it): sequential fp32 sum over HW in row order, times fp32(1 / HW); fp32, not yet
    rounded.  x [n, HW, C]."""
    n, HW, Cc = x.shape
    acc = np.zeros((n, Cc), np.float32)
    for i in range(HW):
        acc = acc + x[:, i, :]
    inv = np.float32(1.0) / np.float32(HW)
    assert inv == np.float32(1.0 / HW)
    return acc * inv


def avgpool_bound(x):
    """|result - float64 mean| allowed, from the inputs alone.  The fp32 sum is off by at most A = (HW - 1) 2^-24 sum|x|; the
    multiply by fp32(1 / HW) (two fp32 roundings, 2^-24 each, and one more for 1 / HW itself) and the bf16 rounding (half an
    ulp of 8 significant bits: 2^-8) are relative to a value within A / HW of the mean; 2^-134 is half the spacing of the
    bf16 subnormals, where the rounding is absolute."""
    HW = x.shape[1]
    x64 = x.astype(np.float64) if x.size < (1 << 24) else None
    sabs = np.abs(x64).sum(axis=1) if x64 is not None else np.abs(x).sum(axis=1, dtype=np.float64)
    mean = x64.sum(axis=1) / HW if x64 is not None else x.sum(axis=1, dtype=np.float64) / HW
    a = (HW - 1) * 2.0 ** -24 * sabs / HW
    return mean, a + (np.abs(mean) + a) * (2.0 ** -8 + 3 * 2.0 ** -24) + 2.0 ** -134


def run_avgpool(lib, x, drop=None):
    n, HW, Cc = x.shape
    y = Guarded((n, Cc))
    xd = dev_bits(x)
    _lib.check(lib.fav_op_avgpool(xd.data_ptr(), y.ptr, n, HW, Cc, C.byref(drop) if drop is not None else None, None))
    torch.cuda.synchronize()
    return y.value()


def tiled_spread(rng, shape):
    """spread() for tensors too large to draw element by element: one block of a prime length repeated, so that no two
    columns of the pool see the same sequence."""
    size = int(np.prod(shape))
    if size <= 1000003:
        return spread(rng, shape)
    return np.resize(spread(rng, (1000003,)), size).reshape(shape)


@pytest.mark.parametrize("n", [1, 33])
@pytest.mark.parametrize("Cc", [16, 64, 2048])
@pytest.mark.parametrize("HW", [1, 2, 49, 64, 196, 3136])
def test_avgpool_shapes_bit_exact_and_f64_bound(lib, HW, Cc, n):
    """n = 33 at C = 2048: 4224 work items (16 channels each), several blocks and a ragged last one."""
    rng = np.random.default_rng(HW * 7 + Cc + n)
    x = tiled_spread(rng, (n, HW, Cc))
    ref32 = avgpool_seq(x)
    ref = O.bf16_round(ref32)
    got = run_avgpool(lib, x)
    assert np.array_equal(got.view(np.uint32), ref.view(np.uint32)), f"{np.mean(got != ref):.5f} of elements differ"
    mean, bound = avgpool_bound(x)
    err_ref, err_got = np.abs(ref.astype(np.float64) - mean), np.abs(got.astype(np.float64) - mean)
    print(f"HW {HW} C {Cc} n {n}: max err/bound reference {np.max(err_ref / bound):.4f} kernel {np.max(err_got / bound):.4f}")
    assert np.all(err_ref <= bound), "the reference itself misses the derived bound"
    assert np.all(err_got <= bound)


@pytest.mark.parametrize("HW", [1, 2])
def test_avgpool_subnormal_inputs(lib, HW):
    """HW = 1: the mean of one bf16 subnormal is that subnormal (times 1.0f) - it must come through unchanged.  HW = 2: the
    sum and the halving stay exact in fp32, and the one rounding to a bf16 subnormal is the reference's."""
    rng = np.random.default_rng(77 + HW)
    x = subnormals(rng, (5, HW, 48))
    got = run_avgpool(lib, x)
    ref = O.bf16_round(avgpool_seq(x))
    assert np.array_equal(got.view(np.uint32), ref.view(np.uint32))
    if HW == 1:
        assert np.array_equal(got.view(np.uint32), x[:, 0, :].view(np.uint32)) and np.all(got != 0)
    mean, bound = avgpool_bound(x)
    assert np.all(np.abs(ref.astype(np.float64) - mean) <= bound) and np.all(np.abs(got.astype(np.float64) - mean) <= bound)


@pytest.mark.parametrize("desc", R.EDGE_DESCRIPTORS, ids=R.EDGE_IDS)
def test_avgpool_dropout_edge_descriptors(lib, desc):
    """avgpool_kernel: v = v0 + row through fastdiv, chunk = channel / 16."""
    rng = np.random.default_rng(5)
    x = spread(rng, (desc.rows, 5, 48))
    ref = R.apply_rows(desc, avgpool_seq(x))
    got = run_avgpool(lib, x, cdesc(desc))
    assert np.array_equal(got.view(np.uint32), ref.view(np.uint32)), f"{np.mean(got != ref):.5f} of elements differ"


# ---------------------------------------------------------------------------------------------------------------------
# entry dropout
# ---------------------------------------------------------------------------------------------------------------------
def entry_input(rng, n_img, E):
    x = spread(rng, (n_img, E))
    x[:, ::7] = subnormals(rng, x[:, ::7].shape)              # kept subnormals are scaled, not flushed
    return x


def run_entry_dropout(lib, x, desc, guard=GUARD):
    n_img, E = x.shape
    out = Guarded((desc.rows, E), guard)
    xd = dev_bits(x)
    d = cdesc(desc)
    _lib.check(lib.fav_op_entry_dropout(xd.data_ptr(), out.ptr, E, desc.rows, C.byref(d), None))
    torch.cuda.synchronize()
    return out.value()


@pytest.mark.parametrize("desc", R.EDGE_DESCRIPTORS, ids=R.EDGE_IDS)
@pytest.mark.parametrize("E", [16, 48, 3136 * 4])
def test_entry_dropout_edge_descriptors(lib, E, desc):
    """entry_dropout_kernel carries t and the frame directly (no fastdiv), t in an int.  The guard band is at least a whole
    sample wide: a row outside [v0, v0 + n_out) of a sample the window only touches would land in it."""
    rng = np.random.default_rng(E + 3)
    x = entry_input(rng, desc.n_img, E)
    ref = np.stack([R.apply(desc, r, x[R.row_index(desc, r)[1]]) for r in range(desc.rows)])
    got = run_entry_dropout(lib, x, desc, guard=max(GUARD, desc.n_img * E))
    assert np.array_equal(got.view(np.uint32), ref.view(np.uint32)), f"{np.mean(got != ref):.5f} of elements differ"


# ---------------------------------------------------------------------------------------------------------------------
# the two conv epilogues that draw masks
# ---------------------------------------------------------------------------------------------------------------------
CONV_VARIANTS = [
    # id (the kernel the shape selects), Cout, residual
    ("igemm_128x64x32_epi1_regs_8ch", 64, False),
    ("igemm_128x128x32_epi1_regs_16ch", 128, False),
    ("igemm_128x64x32_epi0_staged", 64, True),
    ("igemm_128x128x32_epi0_staged", 128, True),
]


@pytest.fixture(scope="module")
def conv_operands():
    """One set of operands per variant, made once: non-negative inputs and weights and a bias of 0.5, so that the undropped
    output is strictly positive and a zero in the output is a dropped element.  5 frames of 5 x 3 pixels: the descriptors use
    the first `rows` of them (M <= 75 rows, one partial tile; HWo = 15 is no power of two)."""
    ops = {}
    for name, cout, use_res in CONV_VARIANTS:
        rng = np.random.default_rng(cout + int(use_res))
        x = O.bf16_round(np.abs(rng.standard_normal((5, 5, 3, 64))).astype(np.float32))
        w = O.bf16_round((np.abs(rng.standard_normal((cout, 1, 1, 64))) * 0.2).astype(np.float32))
        b = np.full(cout, 0.5, np.float32)
        res = O.bf16_round(np.abs(rng.standard_normal((5, 5, 3, cout))).astype(np.float32)) if use_res else None
        acc = O.conv_acc(x, O.ConvLayer(cout, 64, 1, 1, 1, 0, w, b))
        plain = O.epilogue(acc, b, res=res, relu=True)
        assert np.all(plain > 0)
        ops[name] = (x, w, b, res, acc, plain)
    return ops


@pytest.mark.parametrize("desc", R.EDGE_DESCRIPTORS, ids=R.EDGE_IDS)
@pytest.mark.parametrize("variant", [v[0] for v in CONV_VARIANTS])
def test_conv_fused_dropout_edge_descriptors(lib, conv_operands, variant, desc):
    x, w, b, res, acc, plain = conv_operands[variant]
    n = desc.rows
    keep = np.stack([R.keep_mask(desc, r, plain[r].size).reshape(plain[r].shape) for r in range(n)])
    ref = O.epilogue(acc[:n], b, res=None if res is None else res[:n], relu=True, keep=keep, scale=R.scale_of(desc.threshold))
    got = run_conv(lib, x[:n], w, b, None if res is None else res[:n], 1, 0, relu=1, drop=cdesc(desc))
    assert np.array_equal(got == 0, ~keep), f"{np.mean((got == 0) != ~keep):.5f} of the mask differs from the reference"
    assert_one_ulp(got, ref)


# ---------------------------------------------------------------------------------------------------------------------
# entry reduce and bottleneck tail
# ---------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("desc", R.EDGE_DESCRIPTORS, ids=R.EDGE_IDS)
def test_entry_reduce_edge_descriptors(lib, desc):
    """entry_reduce_kernel (C = 256, Nred = 64, the smallest frame: 5 x 3) carries t and the frame directly: y bit for bit the
    reference, and bit for bit what fav_op_entry_dropout writes for the same descriptor."""
    rng = np.random.default_rng(desc.rows + 40)
    Cc, nred, HW = 256, 64, 15
    x = spread(rng, (desc.n_img, HW * Cc), positive=True)
    wa = dev_bf16(O.bf16_round((rng.standard_normal((nred, Cc)) * np.sqrt(2.0 / Cc)).astype(np.float32)))
    ba = torch.from_numpy((rng.standard_normal(nred) * 0.2).astype(np.float32)).cuda()
    xd, d = dev_bits(x), cdesc(desc)
    y, t1 = Guarded((desc.rows, HW * Cc), max(GUARD, desc.n_img * HW * Cc)), Guarded((desc.rows, HW * nred), max(GUARD, desc.n_img * HW * nred))
    _lib.check(lib.fav_op_entry_reduce(xd.data_ptr(), y.ptr, wa.data_ptr(), ba.data_ptr(), t1.ptr, Cc, nred, HW, desc.rows,
                                       C.byref(d), None))
    torch.cuda.synchronize()
    got = y.value()
    t1.value()                                                 # its guard band
    keep = np.stack([R.keep_mask(desc, r, HW * Cc) for r in range(desc.rows)])
    assert np.array_equal(got == 0, ~keep), "zero pattern differs from the reference mask"
    ref = np.stack([R.apply(desc, r, x[R.row_index(desc, r)[1]]) for r in range(desc.rows)])
    assert np.array_equal(got.view(np.uint32), ref.view(np.uint32))
    assert np.array_equal(got.view(np.uint32), run_entry_dropout(lib, x, desc).view(np.uint32))


TAIL_CASE = min(TAIL_CASES, key=lambda c: c[3] * c[4] * c[5])[:6]        # (cmid, nred, has3x3, H, W, n): the fewest rows


@pytest.mark.parametrize("desc", R.EDGE_DESCRIPTORS, ids=R.EDGE_IDS)
def test_tail_edge_descriptors(lib, desc):
    """bottleneck_tail_kernel on the smallest case of test_gpu_tail.CASES, n_frames = the descriptor's rows.
    (a) operands as test_gpu_tail.py builds them: y bit for bit the MFMA-model oracle under the REFERENCE's mask, and its zero
        pattern the reference's wherever the undropped output (the same launch without a site) is non-zero;
    (b) integer-valued operands, whose undropped output is exact in bf16, so that the tail's single rounding bf16(v * scale)
        and fav_op_entry_dropout's bf16(bf16(v) * scale) are the same operation: y bitwise equal to fav_op_entry_dropout
        of the undropped output on the same descriptor."""
    cmid, nred, has3x3, H, W, _ = TAIL_CASE
    assert (nred, has3x3) == (0, False)
    n, cout = desc.rows, 4 * cmid
    E = H * W * cout
    scale = R.scale_of(desc.threshold)
    keep = np.stack([R.keep_mask(desc, r, E) for r in range(n)]).reshape(n, H, W, cout)
    # (a)
    rng = np.random.default_rng(cmid * 31 + H * W + n)
    x = O.bf16_round(np.maximum(rng.standard_normal((n, H, W, cmid)) * np.exp2(rng.integers(-2, 3, (n, H, W, cmid))), -0.2).astype(np.float32))
    wc = O.bf16_round((rng.standard_normal((cout, 1, 1, cmid)) * np.sqrt(1.0 / cmid)).astype(np.float32))
    bc = (rng.standard_normal(cout) * 0.2).astype(np.float32)
    res = O.bf16_round(np.maximum(rng.standard_normal((n, H, W, cout)), 0).astype(np.float32))
    y, _ = run_tail(lib, x, None, None, wc, bc, res, None, None, drop=cdesc(desc))
    y0, _ = run_tail(lib, x, None, None, wc, bc, res, None, None)
    live = y0 != 0
    assert live.mean() > 0.5
    assert np.array_equal((y == 0)[live], ~keep[live]), "zero pattern differs from the reference mask"
    oy = O.epilogue(O.conv_acc_exact(x, wc, 1, 1, 1, 0, mode="mfma"), bc, res=res, relu=True, keep=keep, scale=scale)
    assert np.array_equal(y, oy), f"{np.mean(y != oy):.5f} of elements differ from the oracle under the reference mask"
    # (b) x in 0..7, four unit weights per output channel, bias 1, residual 0..3: every output an integer in 1 .. 32
    xi = rng.integers(0, 8, (n, H, W, cmid)).astype(np.float32)
    wi = np.zeros((cout, 1, 1, cmid), np.float32)
    for c in range(cout):
        wi[c, 0, 0, rng.choice(cmid, 4, replace=False)] = 1.0
    bi = np.ones(cout, np.float32)
    ri = rng.integers(0, 4, (n, H, W, cout)).astype(np.float32)
    yi0, _ = run_tail(lib, xi, None, None, wi, bi, ri, None, None)
    exact = np.einsum("nhwk,ck->nhwc", xi, wi[:, 0, 0, :]) + 1.0 + ri
    assert np.array_equal(yi0, exact) and exact.min() >= 1 and exact.max() <= 32
    yi, _ = run_tail(lib, xi, None, None, wi, bi, ri, None, None, drop=cdesc(desc))
    # the cached frames of the entry dropout: frame i = v % n_img of row r holds row r's undropped output
    cached = np.zeros((desc.n_img, E), np.float32)
    for r in range(n):
        cached[R.row_index(desc, r)[1]] = yi0[r].reshape(-1)
    if len({R.row_index(desc, r)[1] for r in range(n)}) == n:
        ed = run_entry_dropout(lib, cached, desc)
    else:                                                      # a window longer than a sample: one launch per row
        ed = np.concatenate([run_entry_dropout(lib, yi0[r].reshape(1, -1).repeat(desc.n_img, axis=0),
                                               desc._replace(v0=desc.v0 + r, rows=1)) for r in range(n)])
    assert np.array_equal(yi.reshape(n, -1).view(np.uint32), ed.view(np.uint32)), "tail and entry dropout drew different masks"
    assert np.array_equal(yi == 0, ~keep)


# ---------------------------------------------------------------------------------------------------------------------
# rejections
# ---------------------------------------------------------------------------------------------------------------------
V31 = 1 << 31
BAD_DESCRIPTORS = [
    # what is wrong, fields of the descriptor (the rest: site 3, threshold 64, its scale, n_img 2, v0 0); every op launches 2 rows
    ("threshold 256", dict(thr=256)),
    ("threshold 2^32-1", dict(thr=(1 << 32) - 1)),
    ("scale +inf", dict(scale=float("inf"))),
    ("scale NaN", dict(scale=float("nan"))),
    ("scale 0", dict(scale=0.0)),
    ("scale -1", dict(scale=-1.0)),
    ("n_img 0", dict(n_img=0)),
    ("n_img -3", dict(n_img=-3)),
    ("v0 -1", dict(v0=-1)),
    ("v0 + n = 2^31", dict(v0=V31 - 2)),
    ("v0 = 2^40", dict(v0=1 << 40)),
]
DESC_OPS = ("fav_op_conv2d", "fav_op_bottleneck_tail", "fav_op_avgpool", "fav_op_entry_dropout", "fav_op_entry_reduce")
BAD_SHAPES = [
    # op, what is wrong, arguments that differ from the accepted call
    ("fav_op_maxpool3x3s2", "n 0", dict(n=0)), ("fav_op_maxpool3x3s2", "n -1", dict(n=-1)),
    ("fav_op_maxpool3x3s2", "H 0", dict(H=0)), ("fav_op_maxpool3x3s2", "W 0", dict(W=0)), ("fav_op_maxpool3x3s2", "H -2", dict(H=-2)),
    ("fav_op_avgpool", "n 0", dict(n=0)), ("fav_op_avgpool", "n -1", dict(n=-1)),
    ("fav_op_avgpool", "HW 0", dict(HW=0)), ("fav_op_avgpool", "HW -1", dict(HW=-1)),
    ("fav_op_entry_dropout", "n_out 0", dict(n_out=0)), ("fav_op_entry_dropout", "n_out -1", dict(n_out=-1)),
    ("fav_op_entry_dropout", "elems_per_frame 0", dict(elems=0)), ("fav_op_entry_dropout", "elems_per_frame -16", dict(elems=-16)),
    ("fav_op_stem_im2col", "n 0", dict(n=0)), ("fav_op_stem_im2col", "n -1", dict(n=-1)),
    ("fav_op_stem_im2col", "H 0", dict(H=0)), ("fav_op_stem_im2col", "W 0", dict(W=0)), ("fav_op_stem_im2col", "W -1", dict(W=-1)),
]
REJECTED = [(op, why, dict(desc=kw)) for op in DESC_OPS for why, kw in BAD_DESCRIPTORS] + BAD_SHAPES


def call_op(lib, op, src, dst, stream, n=2, H=4, W=4, HW=16, n_out=2, elems=1024, desc=None):
    """One call of `op` on small shapes: every input at src (zeros), every output at dst.  The largest thing an unvalidated
    launch of these arguments could write is a few rows of 4 x 4 x 256 bf16 - far inside dst."""
    dk = dict(site=3, thr=64, scale=float(R.scale_of(64)), seed=7, v0=0, n_img=2, first=0)
    dk.update(desc or {})
    d = _lib.FavDropoutDesc(dk["site"], dk["thr"], dk["scale"], dk["seed"], dk["v0"], dk["n_img"], dk["first"])
    if op == "fav_op_conv2d":
        cd = _lib.FavConvDesc(src, src, src, None, dst, n, H, W, 64, 64, 1, 1, 1, 0, 1, 0, 0, d)
        return lib.fav_op_conv2d(C.byref(cd), stream)
    if op == "fav_op_bottleneck_tail":
        td = _lib.FavTailDesc(src, None, None, src, src, src, dst, None, None, None, n, H, W, 64, 0, d)
        return lib.fav_op_bottleneck_tail(C.byref(td), stream)
    if op == "fav_op_avgpool":
        return lib.fav_op_avgpool(src, dst, n, HW, 64, C.byref(d), stream)
    if op == "fav_op_entry_dropout":
        return lib.fav_op_entry_dropout(src, dst, elems, n_out, C.byref(d), stream)
    if op == "fav_op_entry_reduce":
        return lib.fav_op_entry_reduce(src, dst, src, src, dst + (1 << 20), 256, 64, HW, n_out, C.byref(d), stream)
    if op == "fav_op_maxpool3x3s2":
        return lib.fav_op_maxpool3x3s2(src, dst, n, H, W, 64, stream)
    if op == "fav_op_stem_im2col":
        mean, istd = (C.c_float * 3)(0.5, 0.5, 0.5), (C.c_float * 3)(2.0, 2.0, 2.0)
        return lib.fav_op_stem_im2col(src, 0, n, H, W, 3, 3, 1, 1, 64, mean, istd, dst, stream)
    raise AssertionError(op)


@pytest.mark.parametrize("op,why,kw", REJECTED, ids=[f"{r[0]}-{r[1]}" for r in REJECTED])
def test_rejections_launch_nothing(lib, op, why, kw):
    """FAV_ERR_INVALID_ARG, a message that names the function, and a guard-filled output nobody wrote; then the same buffers
    in contract are accepted and written: the rejection was the argument's."""
    src = torch.zeros(1 << 20, dtype=torch.bfloat16, device="cuda")
    dst = torch.full((1 << 21,), FILL, dtype=torch.bfloat16, device="cuda")
    stream = torch.cuda.current_stream().cuda_stream
    status = call_op(lib, op, src.data_ptr(), dst.data_ptr(), stream, **kw)
    torch.cuda.synchronize()
    assert status == 1, f"{op}, {why}: status {status}"                     # FAV_ERR_INVALID_ARG
    assert op.encode() in lib.fav_last_error(None), lib.fav_last_error(None)
    assert bool((dst == FILL).all()), f"{op}, {why}: something was written"
    assert call_op(lib, op, src.data_ptr(), dst.data_ptr(), stream) == 0
    torch.cuda.synchronize()
    assert not bool((dst == FILL).all())
