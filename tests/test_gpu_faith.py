"""Deletion / insertion curves on the device (include/fav.h): the four fav_op_* kernels against
tests/faith_ref.py, bit for bit with guard bytes around every output, fav_classify_curve against the composition of the ops
through the C ABI, and Backend.faithfulness_report.  The class-probability head is the one exception to bits - expf rules them
out - and is held to heads_ref's PROB_TOL; with classes NULL it is head_unc_kernel's mean_prob bit for bit.  Nothing here says
anything about the SIGN of a gain: on synthetic checkpoints it carries no meaning."""
import ctypes as C
import itertools

import numpy as np
import pytest

pytestmark = pytest.mark.gpu

import torch  # noqa: E402
import faith_ref as R  # noqa: E402
import heads_ref as H  # noqa: E402
from perturb_gpu import PAT, Out, dev, frames_of, host, last_error, stream  # noqa: E402
from failure_aware_vision_amd import Backend, _lib, faithfulness, synth, views, weights  # noqa: E402
from failure_aware_vision_amd.backend import unpack_uncertainty  # noqa: E402

U8, F32 = _lib.LAYOUT_NHWC_U8, _lib.LAYOUT_NHWC_F32
ids = lambda s: "x".join(map(str, s)) if isinstance(s, tuple) else str(s)  # noqa: E731


@pytest.fixture(scope="module")
def lib():
    assert torch.cuda.is_available(), "GPU tests need a MI355X"
    return _lib.load()


def fill_words(fill):
    return (C.c_uint32 * 3)(*[int(v) for v in fill])


# ---- fav_op_rank_cells ---------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("n", (1, 3))
@pytest.mark.parametrize("cells", (1, 2, 49, 196, 1024))
def test_op_rank_cells(lib, cells, n):
    maps = R.tricky_maps(n, cells, seed=7 * cells + n)
    out = Out(n * cells * 4)
    m = dev(maps)
    assert lib.fav_op_rank_cells(m.data_ptr(), n, cells, out.ptr, stream()) == 0, last_error(lib)
    torch.cuda.synchronize()
    got = out.get(np.int32, (n, cells))
    assert np.array_equal(got, R.rank_cells(maps))
    for i in range(n):
        assert np.array_equal(np.sort(got[i]), np.arange(cells))


def test_op_rank_cells_refusals_launch_nothing(lib):
    m = dev(np.zeros((2, 8), np.float32))
    out = Out(2 * 8 * 4)
    for why, args, text in (("null map", (None, 2, 8, out.ptr), "null"), ("null rank", (m.data_ptr(), 2, 8, None), "null"),
                            ("n 0", (m.data_ptr(), 0, 8, out.ptr), "at least 1"), ("cells 0", (m.data_ptr(), 2, 0, out.ptr), "cells=0"),
                            ("cells 1025", (m.data_ptr(), 2, 1025, out.ptr), "cells=1025"),
                            ("rank + 2", (m.data_ptr(), 2, 8, out.ptr + 2), "aligned")):
        st = lib.fav_op_rank_cells(*args, stream())
        torch.cuda.synchronize()
        assert st == 1 and "fav_op_rank_cells" in last_error(lib) and text in last_error(lib), (why, last_error(lib))
        assert out.untouched(), why


# ---- fav_op_occlude ------------------------------------------------------------------------------------------------------
def fill_for(dtype):
    return (17, 255, 0) if dtype == np.uint8 else (0x7FC12345, 0x80000000, 0x3F000000)     # fp32: a NaN payload, -0, 0.5


def run_occlude(lib, frames, rank, mh, mw, mode, S, s0, s1, fill, in_off=0, out_off=0, single_steps=False):
    """-> the output [s1 - s0, n, H, W, 3] (guards checked).  single_steps: one launch a step, each into its slice."""
    n, H_, W, _ = frames.shape
    raw = np.ascontiguousarray(frames).view(np.uint8).ravel()
    inbuf = torch.zeros(raw.size + 32, dtype=torch.uint8, device="cuda")
    inbuf[in_off:in_off + raw.size] = torch.from_numpy(raw).cuda()
    out = Out(raw.size * (s1 - s0), out_off)
    layout = U8 if frames.dtype == np.uint8 else F32
    r = dev(np.asarray(rank, np.int32))
    for a, b in ([(s, s + 1) for s in range(s0, s1)] if single_steps else [(s0, s1)]):
        st = lib.fav_op_occlude(inbuf.data_ptr() + in_off, out.ptr + (a - s0) * raw.size, n, H_, W, layout, r.data_ptr(), mh, mw, mode, S,
                                a, b, fill_words(fill), stream())
        assert st == 0, last_error(lib)
    torch.cuda.synchronize()
    return out.get(frames.dtype, (s1 - s0, n, H_, W, 3))


def bits_equal(a, b):
    return a.shape == b.shape and a.dtype == b.dtype and np.array_equal(a.view(np.uint8), b.view(np.uint8))


SIZES = [(hw, m) for hw in ((1, 1), (5, 7), (32, 32), (33, 47)) for m in ((1, 1), (3, 5), (7, 7), (14, 14))] + [((5, 7), (32, 32))]


@pytest.mark.parametrize("hw,mhw", SIZES, ids=ids)
def test_op_occlude_bit_exact(lib, hw, mhw):
    (H_, W), (mh, mw) = hw, mhw
    cells = mh * mw
    steps = [1, 2, 16] + ([cells + 3] if cells + 3 <= 256 else [])           # an S above the cell count: some steps add no cell
    rng = np.random.default_rng(H_ * 1000 + W * 10 + cells)
    for dtype, mode, n in itertools.product((np.uint8, np.float32), (R.DELETION, R.INSERTION), (1, 3)):
        frames = frames_of(n, H_, W, dtype, seed=n)
        rank = np.stack([rng.permutation(cells) for _ in range(n)]).astype(np.int32)
        fill = fill_for(dtype)
        for S in steps:
            want = R.occlude(frames, rank, mh, mw, mode, S, 0, S + 1, fill)
            what = (dtype.__name__, mode, n, S)
            assert bits_equal(run_occlude(lib, frames, rank, mh, mw, mode, S, 0, S + 1, fill), want), what
            assert bits_equal(run_occlude(lib, frames, rank, mh, mw, mode, S, 0, S + 1, fill, single_steps=True), want), what
        # a range in the middle
        S = 16
        want = R.occlude(frames, rank, mh, mw, mode, S, 5, 9, fill)
        assert bits_equal(run_occlude(lib, frames, rank, mh, mw, mode, S, 5, 9, fill), want)


@pytest.mark.parametrize("in_off,out_off", ((1, 0), (2, 3), (3, 1), (0, 2)))
def test_op_occlude_u8_byte_offsets(lib, in_off, out_off):
    frames = frames_of(3, 9, 13, np.uint8, seed=in_off)
    rng = np.random.default_rng(in_off * 4 + out_off)
    rank = np.stack([rng.permutation(15) for _ in range(3)]).astype(np.int32)
    for mode in (R.DELETION, R.INSERTION):
        want = R.occlude(frames, rank, 3, 5, mode, 4, 0, 5, (1, 2, 3))
        assert bits_equal(run_occlude(lib, frames, rank, 3, 5, mode, 4, 0, 5, (1, 2, 3), in_off, out_off), want)


def test_op_occlude_copies_nan_payloads_and_negative_zero(lib):
    words = np.array([0x7FC00001, 0xFFC12345, 0x7F800001, 0x80000000, 0x00000001, 0xFF800000], np.uint32)
    frames = np.resize(words, 2 * 6 * 10 * 3).reshape(2, 6, 10, 3).view(np.float32)
    rank = np.stack([np.arange(4), np.arange(4)[::-1]]).astype(np.int32)
    fill = (0x7FC0BEEF, 0x80000000, 0)
    for mode in (R.DELETION, R.INSERTION):
        got = run_occlude(lib, frames, rank, 2, 2, mode, 4, 0, 5, fill)
        assert bits_equal(got, R.occlude(frames, rank, 2, 2, mode, 4, 0, 5, fill))
    assert bits_equal(got[4], frames) and (got[0].view(np.uint32) == np.array(fill, np.uint32)).all()


def test_op_occlude_takes_a_rank_array_that_is_no_permutation(lib):
    frames = frames_of(2, 12, 12, np.uint8)
    rank = np.array([[0, 0, 0, 5, -7, 2 ** 31 - 1, 8, 8, 3], [9, 9, 9, 9, 9, 9, 9, 9, 9]], np.int32)
    for mode in (R.DELETION, R.INSERTION):
        want = R.occlude(frames, rank, 3, 3, mode, 3, 0, 4, (9, 8, 7))
        assert bits_equal(run_occlude(lib, frames, rank, 3, 3, mode, 3, 0, 4, (9, 8, 7)), want)
    assert (want[3][1] == np.array((9, 8, 7), np.uint8)).all()               # rank 9 is never below k: insertion shows nothing


@pytest.mark.parametrize("dtype", (np.uint8, np.float32), ids=("u8", "f32"))
def test_op_occlude_one_large_frame_size(lib, dtype):
    frames = frames_of(2, 224, 224, dtype)
    rng = np.random.default_rng(224)
    rank = np.stack([rng.permutation(196) for _ in range(2)]).astype(np.int32)
    for mode in (R.DELETION, R.INSERTION):
        want = R.occlude(frames, rank, 14, 14, mode, 4, 0, 5, fill_for(dtype))
        assert bits_equal(run_occlude(lib, frames, rank, 14, 14, mode, 4, 0, 5, fill_for(dtype)), want)


def test_op_occlude_refusals_launch_nothing(lib):
    frame_bytes = 8 * 8 * 3
    frames = torch.full((2 * frame_bytes * 4 + 64,), 7, dtype=torch.uint8, device="cuda")
    out = torch.full((17 * 2 * frame_bytes * 4 + 64,), PAT, dtype=torch.uint8, device="cuda")
    rank = dev(np.zeros((2, 4), np.int32))
    f, o, r = frames.data_ptr(), out.data_ptr(), rank.data_ptr()
    ok, big = fill_words((1, 2, 3)), fill_words((1, 256, 3))

    def args(frames_=f, out_=o, n=2, H_=8, W=8, layout=U8, rank_=r, mh=2, mw=2, mode=0, S=16, s0=0, s1=17, fill=ok):
        return (frames_, out_, n, H_, W, layout, rank_, mh, mw, mode, S, s0, s1, fill)
    cases = [("null frames", args(frames_=None), "null"), ("null out", args(out_=None), "null"), ("null rank", args(rank_=None), "null"),
             ("null fill", args(fill=None), "null"), ("s0 == s1", args(s0=3, s1=3), "steps [3, 3)"), ("s0 > s1", args(s0=4, s1=3), "steps [4, 3)"),
             ("s0 < 0", args(s0=-1, s1=3), "steps [-1, 3)"), ("s1 > S + 1", args(s1=18), "steps [0, 18)"), ("S 0", args(S=0, s1=1), "steps=0"),
             ("S 257", args(S=257), "steps=257"), ("fill 256", args(fill=big), "fill[1]=256"), ("n 0", args(n=0), "at least 1"),
             ("H 0", args(H_=0), "at least 1"), ("layout", args(layout=2), "layout"), ("mode", args(mode=2), "mode=2"),
             ("map 0", args(mh=0), "map 0x2"), ("map 1025", args(mh=25, mw=41), "map 25x41"), ("map side", args(mh=257, mw=1), "map 257x1"),
             ("f32 frames + 2", args(frames_=f + 2, layout=F32, s1=1), "aligned"), ("f32 out + 1", args(out_=o + 1, layout=F32, s1=1), "aligned"),
             ("rank + 2", args(rank_=r + 2), "aligned"),
             ("out == frames", args(out_=f, s1=1), "overlaps"), ("out in frames", args(out_=f + 2 * frame_bytes - 1, s1=1), "overlaps"),
             ("frames in out", args(frames_=o + 5 * frame_bytes), "overlaps"),
             ("out end on frames", args(frames_=o + 2 * 2 * frame_bytes - 1, s1=2), "overlaps")]
    for why, a, text in cases:
        st = lib.fav_op_occlude(*a, stream())
        torch.cuda.synchronize()
        msg = last_error(lib)
        assert st == 1 and "fav_op_occlude" in msg and text in msg, (why, msg)
        assert bool((out == PAT).all()) and bool((frames == 7).all()), why
    # the fill's range is uint8's alone, and touching ranges do not overlap
    assert lib.fav_op_occlude(*args(layout=F32, fill=big, s1=2), stream()) == 0
    assert lib.fav_op_occlude(*args(frames_=o + 2 * 2 * frame_bytes, s1=2), stream()) == 0
    torch.cuda.synchronize()


# ---- fav_op_head_class_prob ----------------------------------------------------------------------------------------------
def dev_logits(lg, extra=0):
    """[T, n, C] -> device [T, n, ld], ld = C rounded up to 4 plus extra, garbage (NaN) in the padding columns."""
    T, n, Cc = lg.shape
    ld = (Cc + 3) // 4 * 4 + extra
    full = np.full((T, n, ld), np.nan, np.float32)
    full[:, :, :Cc] = lg
    return dev(full), ld


def op_class_prob(lib, d, T, n, Cc, ld, temp, classes):
    prob, lab = Out(n * 4), Out(n * 4)
    cls = dev(np.asarray(classes, np.int32)) if classes is not None else None
    st = lib.fav_op_head_class_prob(d.data_ptr(), T, n, Cc, ld, temp, cls.data_ptr() if cls is not None else None, prob.ptr, lab.ptr, stream())
    assert st == 0, last_error(lib)
    torch.cuda.synchronize()
    return prob.get(np.float32, (n,)), lab.get(np.int32, (n,))


def op_unc(lib, d, T, n, Cc, ld, temp):
    rec = Out(n * 72)
    _lib.check(lib.fav_op_head_uncertainty(d.data_ptr(), T, n, Cc, ld, temp, 0, 0.5, rec.ptr, None, None, stream()))
    torch.cuda.synchronize()
    return unpack_uncertainty(rec.get(np.int32, (n, 18)))


def class_prob_inputs():
    out = []
    for Cc in (1, 10, 37, 1000, 1024):
        for T in (1, 3, 5):
            out.append((f"gaussian_C{Cc}_T{T}", H.gaussian(T, 6, Cc, 31 * Cc + T), 0))
        out.append((f"ladder_C{Cc}", H.ladder(3, 6, Cc, 5 + Cc), 8))
    for c in H.nonfinite_cases() + H.overflow_cases():
        out.append((c["name"], c["logits"], 4, c["temperature"]))
    return out


@pytest.mark.parametrize("case", class_prob_inputs(), ids=lambda c: c[0])
def test_op_head_class_prob(lib, case):
    name, lg, extra = case[:3]
    temp = case[3] if len(case) > 3 else H.TEMPERATURE
    T, n, Cc = lg.shape
    d, ld = dev_logits(lg, extra)
    ref = H.heads_ref(lg, temp)
    unc = op_unc(lib, d, T, n, Cc, ld, temp)
    bad = ref["nonfinite"]
    rows = np.arange(n)
    rng = np.random.default_rng(Cc)
    for classes in (np.zeros(n, np.int32), np.full(n, Cc - 1, np.int32), np.full(n, -1, np.int32), np.full(n, Cc, np.int32),
                    rng.integers(-1, Cc + 1, n).astype(np.int32)):
        prob, lab = op_class_prob(lib, d, T, n, Cc, ld, temp, classes)
        inside = (classes >= 0) & (classes < Cc)
        want = np.where(inside & ~bad, ref["pbar"][rows, np.clip(classes, 0, Cc - 1)], np.nan)
        assert np.array_equal(np.isnan(prob), np.isnan(want)), (name, classes)           # NaN exactly where the rule says
        err = np.abs(prob[~np.isnan(want)].astype(np.float64) - want[~np.isnan(want)])
        assert err.size == 0 or err.max() <= H.PROB_TOL, (name, classes, err.max())
        assert np.array_equal(lab, unc["label"]), name                                   # the label is still written
        assert (lab[bad] == 0).all()
    # classes NULL: the frame's own label - mean_prob and label of the uncertainty head, bit for bit
    prob, lab = op_class_prob(lib, d, T, n, Cc, ld, temp, None)
    assert np.array_equal(lab, unc["label"]) and R.same_bits(prob, np.ascontiguousarray(unc["mean_prob"])), name
    assert np.isnan(prob[bad]).all() and not np.isnan(prob[~bad]).any()
    # naming the label gives the same bits as asking for it
    prob2, _ = op_class_prob(lib, d, T, n, Cc, ld, temp, lab)
    assert R.same_bits(prob2[~bad], prob[~bad])


def test_op_head_class_prob_refusals_launch_nothing(lib):
    d, ld = dev_logits(H.gaussian(2, 3, 10, 1))
    prob, cls = Out(12), dev(np.zeros(3, np.int32))
    for why, args, text in (("null logits", (None, 2, 3, 10, ld, 1.0, cls.data_ptr(), prob.ptr, None), "null"),
                            ("null prob", (d.data_ptr(), 2, 3, 10, ld, 1.0, cls.data_ptr(), None, None), "null"),
                            ("T 0", (d.data_ptr(), 0, 3, 10, ld, 1.0, None, prob.ptr, None), "T"),
                            ("T 4097", (d.data_ptr(), 4097, 3, 10, ld, 1.0, None, prob.ptr, None), "T"),
                            ("C 1025", (d.data_ptr(), 2, 3, 1025, 1028, 1.0, None, prob.ptr, None), "num_classes"),
                            ("ld", (d.data_ptr(), 2, 3, 10, 10, 1.0, None, prob.ptr, None), "stride"),
                            ("temperature", (d.data_ptr(), 2, 3, 10, ld, 0.0, None, prob.ptr, None), "temperature")):
        st = lib.fav_op_head_class_prob(*args, stream())
        torch.cuda.synchronize()
        assert st == 1 and "fav_op_head_class_prob" in last_error(lib) and text in last_error(lib), (why, last_error(lib))
        assert prob.untouched(), why


# ---- fav_op_curve --------------------------------------------------------------------------------------------------------
def run_curve(lib, prob, labels, classes, S, cells, mode):
    n = prob.shape[1]
    cv, rec = Out(n * (S + 1) * 4), Out(n * 32)
    p, l, c = dev(prob), dev(labels), dev(classes)                             # kept alive until the launch has run
    st = lib.fav_op_curve(p.data_ptr(), l.data_ptr(), c.data_ptr(), n, S, cells, mode, cv.ptr, rec.ptr, stream())
    assert st == 0, last_error(lib)
    torch.cuda.synchronize()
    return cv.get(np.float32, (n, S + 1)), rec.get(np.int32, (n, 8))


@pytest.mark.parametrize("n", (1, 5))
@pytest.mark.parametrize("S", (1, 2, 16, 256))
def test_op_curve(lib, S, n):
    rng = np.random.default_rng(S * 10 + n)
    prob = rng.random((S + 1, n)).astype(np.float32)
    classes = rng.integers(0, 3, n).astype(np.int32)
    labels = np.repeat(classes[None, :], S + 1, axis=0)                        # no flip under deletion, flip at 0 under insertion
    if n > 1:
        labels[:, 1] = classes[1] + 1                                          # flip at step 0 under deletion, none under insertion
        labels[S // 2:, 2] = classes[2] + 1                                    # flip in the middle
        prob[S // 2, 3] = np.nan                                               # a NaN in the middle of a curve
        classes[4] = -1                                                        # the class outside the range
    for mode in (R.DELETION, R.INSERTION):
        cv, rec = run_curve(lib, prob, labels, classes, S, 196, mode)
        wcv, wrec = R.curve(prob, labels, classes, S, 196, mode)
        assert R.same_bits(cv, wcv) and R.same_records(rec, wrec), (mode, rec, wrec)
    # what the cases are there for
    cv, rec = run_curve(lib, prob, labels, classes, S, 196, R.DELETION)
    assert rec[0, 3] == -1 and rec[0, 6] == -1
    if n > 1:
        assert rec[1, 3] == 0 and rec[1, 6] == 0 and rec[2, 3] == S // 2 and rec[2, 6] == (S // 2) * 196 // S
        assert np.isnan(rec[3:4, 1].view(np.float32)).all() and not np.isnan(rec[3:4, 5].view(np.float32)).any()
        assert rec[4].tolist() == [-1, R.NAN_BITS, R.NAN_BITS, -1, R.NAN_BITS, R.NAN_BITS, -1, 0]


def test_op_curve_refusals_launch_nothing(lib):
    p, l, c = dev(np.zeros((5, 3), np.float32)), dev(np.zeros((5, 3), np.int32)), dev(np.zeros(3, np.int32))
    cv, rec = Out(3 * 5 * 4), Out(3 * 32)
    a = dict(prob=p.data_ptr(), labels=l.data_ptr(), classes=c.data_ptr(), n=3, S=4, cells=49, mode=0, curve=cv.ptr, rec=rec.ptr)
    for why, over, text in (("null prob", dict(prob=None), "null"), ("null labels", dict(labels=None), "null"),
                            ("null classes", dict(classes=None), "null"), ("null curve", dict(curve=None), "null"),
                            ("null rec", dict(rec=None), "null"), ("n 0", dict(n=0), "at least 1"), ("S 0", dict(S=0), "steps=0"),
                            ("S 257", dict(S=257), "steps=257"), ("cells 0", dict(cells=0), "cells=0"),
                            ("cells 1025", dict(cells=1025), "cells=1025"), ("mode", dict(mode=-1), "mode=-1"),
                            ("rec + 4", dict(rec=rec.ptr + 4), "8-byte"), ("curve + 2", dict(curve=cv.ptr + 2), "4-byte")):
        st = lib.fav_op_curve(*{**a, **over}.values(), stream())
        torch.cuda.synchronize()
        assert st == 1 and "fav_op_curve" in last_error(lib) and text in last_error(lib), (why, last_error(lib))
        assert cv.untouched() and rec.untouched(), why


# ---- through a handle ----------------------------------------------------------------------------------------------------
MAX_BATCH, N, STEPS, FIRST = 8, 5, 4, 1000
HANDLES = ("resnet18", "resnet18_mc", "ensemble", "vit_tiny")


def make_backend(kind, **kw):
    if kind == "vit_tiny":
        blob, _ = weights.make_synthetic_vit("vit_tiny", seed=3)
        return Backend("vit_tiny", blob, max_batch=MAX_BATCH, **kw), 64, (4, 4)
    if kind == "ensemble":
        blobs = [weights.make_synthetic("resnet18_cifar", seed=s)[0] for s in (1, 2)]
        return Backend("resnet18_cifar", blobs, max_batch=MAX_BATCH, **kw), 32, (4, 4)
    blob, _ = weights.make_synthetic("resnet18_cifar", seed=1)
    if kind == "resnet18_mc":
        kw = dict(kw, n_samples=3, dropout_policy="all_blocks", dropout_p=0.1, seed=4)
    return Backend("resnet18_cifar", blob, max_batch=MAX_BATCH, **kw), 32, (4, 4)


@pytest.fixture(scope="module", params=HANDLES)
def handle(request):
    """(backend with a curve of STEPS steps, its frames uint8 [N, S, S, 3], maps fp32 [N, mh, mw] with ties and a NaN)."""
    be, size, mhw = make_backend(request.param, temperature=1.3)
    be.set_curve(STEPS, fill=(0.25, 0.5, 1.0))
    frames = synth.synthetic_frames_u8(N, size, size, seed=21)
    maps = R.tricky_maps(N, mhw[0] * mhw[1], seed=5)[::-1].reshape(N, *mhw).copy()      # the all-NaN map first
    maps[2] = faithfulness.random_maps(1, mhw, 9)[0]
    yield request.param, be, frames, maps
    be.close()


def compose(be, frames_dev, maps_dev, classes, mode, first, fill):
    """fav_classify_curve restated with the public ops through the C ABI -> (curve, records, label, confidence), numpy."""
    lib, h, s = be.lib, be._h, stream()
    n, fh, fw = (int(v) for v in frames_dev.shape[:3])
    mh, mw = int(maps_dev.shape[1]), int(maps_dev.shape[2])
    layout = U8 if frames_dev.dtype == torch.uint8 else F32
    S, Cc, cells = STEPS, int(be.cfg.num_classes), mh * mw
    ld = (Cc + 3) // 4 * 4
    rank = torch.empty((n, cells), dtype=torch.int32, device="cuda")
    _lib.check(lib.fav_op_rank_cells(maps_dev.data_ptr(), n, cells, rank.data_ptr(), s))
    occ = torch.empty_like(frames_dev)
    prob = torch.empty((S + 1, n), dtype=torch.float32, device="cuda")
    lab = torch.empty((S + 1, n), dtype=torch.int32, device="cuda")
    lab0 = torch.empty(n, dtype=torch.int32, device="cuda")
    conf0 = torch.empty(n, dtype=torch.float32, device="cuda")
    scratch_l, scratch_c = torch.empty_like(lab0), torch.empty_like(conf0)
    cls = dev(np.asarray(classes, np.int32)) if classes is not None else lab0
    for k in range(S + 1):
        step = k if mode == R.DELETION else S - k
        _lib.check(lib.fav_op_occlude(frames_dev.data_ptr(), occ.data_ptr(), n, fh, fw, layout, rank.data_ptr(), mh, mw, mode, S, step,
                                      step + 1, fill_words(fill), s))
        _lib.check(lib.fav_classify_ex(h, occ.data_ptr(), n, layout, first, (lab0 if k == 0 else scratch_l).data_ptr(),
                                       (conf0 if k == 0 else scratch_c).data_ptr(), None, None, s), h)
        lg = be.logits()
        padded = torch.full((lg.shape[0], n, ld), float("nan"), dtype=torch.float32, device="cuda")
        padded[:, :, :Cc] = lg
        _lib.check(lib.fav_op_head_class_prob(padded.data_ptr(), int(lg.shape[0]), n, Cc, ld, float(be.cfg.temperature), cls.data_ptr(),
                                              prob[step].data_ptr(), lab[step].data_ptr(), s))
    curve = torch.empty((n, S + 1), dtype=torch.float32, device="cuda")
    rec = torch.empty((n, 8), dtype=torch.int32, device="cuda")
    _lib.check(lib.fav_op_curve(prob.data_ptr(), lab.data_ptr(), cls.data_ptr(), n, S, cells, mode, curve.data_ptr(), rec.data_ptr(), s))
    torch.cuda.synchronize()
    return curve.cpu().numpy(), rec.cpu().numpy(), lab0.cpu().numpy(), conf0.cpu().numpy(), rank.cpu().numpy()


def records_of(r):
    names = ("class_id", "auc", "p_first", "flip_step", "p_last", "p_min", "flip_cells")
    cols = [np.asarray(r[k].cpu().numpy() if hasattr(r[k], "cpu") else r[k]) for k in names]
    return np.stack([c.view(np.int32) for c in cols] + [np.zeros_like(cols[0], dtype=np.int32)], axis=1)


U8_FILL = (64, 128, 255)                                  # round(255 * (0.25, 0.5, 1.0))
F32_FILL = tuple(int(np.float32(v).view(np.uint32)) for v in (0.25, 0.5, 1.0))


def test_classify_curve_equals_the_composition_of_the_ops(handle):
    kind, be, frames, maps = handle
    fd, md = dev(frames), dev(maps)
    Cc = int(be.cfg.num_classes)
    plain = be.classify_uncertainty(fd, first_index=FIRST)
    plain_lab, plain_conf = (host(v) for v in be.classify_detect(fd, first_index=FIRST)[:2])
    res = {}
    for mode_name, mode in (("deletion", R.DELETION), ("insertion", R.INSERTION)):
        for classes in (None, np.array([0, Cc - 1, 3, 1, 2], np.int32)):
            got = be.classify_curve(fd, md, classes, mode_name, first_index=FIRST)
            curve, rec, lab0, conf0, _ = compose(be, fd, md, classes, mode, FIRST, U8_FILL)
            assert R.same_bits(host(got["curve"]), curve), (kind, mode_name)
            assert R.same_records(records_of(got), rec), (kind, mode_name)
            # the unoccluded pass is a plain fav_classify_ex call on the frames
            assert np.array_equal(host(got["label"]), plain_lab) and R.same_bits(host(got["confidence"]), plain_conf)
            assert np.array_equal(lab0, plain_lab) and R.same_bits(conf0, plain_conf)
            if classes is None:
                res[mode_name] = {k: host(v) for k, v in got.items()}
                assert np.array_equal(res[mode_name]["class_id"], plain_lab)
            else:
                assert np.array_equal(host(got["class_id"]), classes)
    # the unoccluded step is the plain frame at the same first_index: under MC-Dropout, the steps share the masks
    mean_prob = host(plain["mean_prob"])
    assert R.same_bits(res["deletion"]["p_first"], mean_prob) and R.same_bits(res["insertion"]["p_last"], mean_prob), kind
    assert R.same_bits(res["deletion"]["curve"][:, 0], mean_prob)
    # fully occluded is fully occluded, whichever way it was reached
    assert R.same_bits(res["deletion"]["p_last"], res["insertion"]["p_first"]), kind
    assert not np.isnan(res["deletion"]["curve"]).any()
    # afterwards the logits are the last pass's: the fully occluded frames
    blank = np.broadcast_to(np.array(U8_FILL, np.uint8), frames.shape).copy()
    be.classify_curve(fd, md, None, "deletion", first_index=FIRST)
    last = host(be.logits())
    be.classify_detect(dev(blank), first_index=FIRST)
    assert R.same_bits(last, host(be.logits())), kind


def test_classes_outside_the_range_through_a_handle(handle):
    kind, be, frames, maps = handle
    Cc = int(be.cfg.num_classes)
    got = be.classify_curve(dev(frames), dev(maps), np.array([0, Cc, -1, Cc - 1, 2 ** 31 - 1], np.int32), "deletion")
    rec = records_of(got)
    for i in (1, 2, 4):
        assert rec[i].tolist() == [-1, R.NAN_BITS, R.NAN_BITS, -1, R.NAN_BITS, R.NAN_BITS, -1, 0], (kind, i)
        assert np.isnan(host(got["curve"])[i]).all()
    assert rec[0, 0] == 0 and rec[3, 0] == Cc - 1 and not np.isnan(host(got["curve"])[[0, 3]]).any()


def test_u8_frames_and_their_f32_twins_occlude_the_same_pixels(handle, lib):
    kind, be, frames, maps = handle
    fd, md = dev(frames), dev(maps)
    twins = dev(frames.astype(np.float32) / np.float32(255.0))
    for mode in (R.DELETION, R.INSERTION):
        _, _, _, _, rank_u8 = compose(be, fd, md, np.zeros(N, np.int32), mode, 0, U8_FILL)
        _, _, _, _, rank_f32 = compose(be, twins, md, np.zeros(N, np.int32), mode, 0, F32_FILL)
        assert np.array_equal(rank_u8, rank_f32) and np.array_equal(rank_u8, R.rank_cells(maps.reshape(N, -1)))
        size, (mh, mw) = frames.shape[1], maps.shape[1:]
        a = run_occlude(lib, frames, rank_u8, mh, mw, mode, STEPS, 0, STEPS + 1, U8_FILL)
        b = run_occlude(lib, host(twins), rank_u8, mh, mw, mode, STEPS, 0, STEPS + 1, F32_FILL)
        for s in range(STEPS + 1):
            m = R.occluded_mask(rank_u8, size, size, mh, mw, STEPS, s)
            filled = m if mode == R.DELETION else ~m
            assert (a[s][filled] == np.array(U8_FILL, np.uint8)).all() and (a[s][~filled] == frames[~filled]).all()
            assert (b[s][filled] == np.array([0.25, 0.5, 1.0], np.float32)).all() and bits_equal(b[s][~filled], host(twins)[~filled])
    # and the handle takes the twins: a curve of finite probabilities whose unoccluded pass is the plain call on them
    got = be.classify_curve(twins, md, None, "insertion", first_index=7)
    plain = be.classify_uncertainty(twins, first_index=7)
    assert R.same_bits(host(got["p_last"]), host(plain["mean_prob"])), kind


def test_chunked_calls_equal_one_call(handle):
    kind, be, frames, maps = handle
    fd, md = dev(frames), dev(maps)
    whole = be.classify_curve(fd, md, None, "deletion", first_index=FIRST)
    a = be.classify_curve(fd[:2], md[:2], None, "deletion", first_index=FIRST)
    b = be.classify_curve(fd[2:], md[2:], None, "deletion", first_index=FIRST + 2)
    for k in ("curve", "label", "confidence", "auc", "class_id", "flip_step", "p_min"):
        joined = np.concatenate([host(a[k]), host(b[k])])
        assert (R.same_bits(joined, host(whole[k])) if joined.dtype == np.float32 else np.array_equal(joined, host(whole[k]))), (kind, k)
    # Backend batches over frames_per_call by itself: 11 frames on a handle of 8, numpy in and out
    many = np.concatenate([frames, frames, frames[:1]])
    mm = np.concatenate([maps, maps, maps[:1]])
    got = be.classify_curve(many, mm, None, "deletion", first_index=FIRST)
    assert isinstance(got["curve"], np.ndarray) and got["curve"].shape == (11, STEPS + 1)
    assert R.same_bits(got["curve"][:N], host(whole["curve"]))
    if kind != "resnet18_mc":                                                   # other global indices, other masks
        assert R.same_bits(got["curve"][N:2 * N], host(whole["curve"]))


# ---- a frame size no cell grid divides -------------------------------------------------------------------------------------
ODD_HW = (31, 45)


@pytest.fixture(scope="module")
def odd_handle():
    """One ResNet-18 MC-Dropout handle at 31 x 45 (every stage odd: 31 x 45, 16 x 23, 8 x 12, 4 x 6) with a curve of STEPS steps."""
    blob, _ = weights.make_synthetic("resnet18_cifar", seed=1)
    be = Backend("resnet18_cifar", blob, in_hw=ODD_HW, max_batch=MAX_BATCH, temperature=1.3, n_samples=3, dropout_policy="all_blocks",
                 dropout_p=0.1, seed=4)
    be.set_curve(STEPS, fill=(0.25, 0.5, 1.0))
    yield be, synth.synthetic_frames_u8(N, *ODD_HW, seed=21)
    be.close()


@pytest.mark.parametrize("dtype", ("u8", "f32"))
@pytest.mark.parametrize("mhw", ((4, 4), (2, 3)), ids=ids)
def test_classify_curve_at_an_odd_frame_size(odd_handle, lib, mhw, dtype):
    """31 x 45 under 4 x 4 and 2 x 3 cells: neither grid divides the frame (a cell is 7.75 x 11.25 or 15.5 x 15 pixels).  The
    handle's curve is the composition of the ops, the unoccluded pass is the plain call, and the occluded pixels are
    faith_ref's cells of the frame, not of a square."""
    be, frames = odd_handle
    maps = R.tricky_maps(N, mhw[0] * mhw[1], seed=5)[::-1].reshape(N, *mhw).copy()
    maps[2] = faithfulness.random_maps(1, mhw, 9)[0]
    fd = dev(frames) if dtype == "u8" else dev(frames.astype(np.float32) / np.float32(255.0))
    fill = U8_FILL if dtype == "u8" else F32_FILL
    md = dev(maps)
    plain_lab, plain_conf = (host(v) for v in be.classify_detect(fd, first_index=FIRST)[:2])
    mean_prob = host(be.classify_uncertainty(fd, first_index=FIRST)["mean_prob"])
    res = {}
    for mode_name, mode in (("deletion", R.DELETION), ("insertion", R.INSERTION)):
        got = be.classify_curve(fd, md, None, mode_name, first_index=FIRST)
        curve, rec, lab0, conf0, rank = compose(be, fd, md, None, mode, FIRST, fill)
        assert R.same_bits(host(got["curve"]), curve) and R.same_records(records_of(got), rec), mode_name
        assert np.array_equal(host(got["label"]), plain_lab) and R.same_bits(host(got["confidence"]), plain_conf)
        assert np.array_equal(lab0, plain_lab) and R.same_bits(conf0, plain_conf)
        assert np.array_equal(rank, R.rank_cells(maps.reshape(N, -1)))
        assert not np.isnan(curve).any()
        res[mode_name] = {k: host(v) for k, v in got.items()}
        # the pixels the op fills at this frame size: whole steps, against the reference's mask of an H x W frame
        src = host(fd)
        occ = run_occlude(lib, src, rank, mhw[0], mhw[1], mode, STEPS, 0, STEPS + 1, fill)
        assert bits_equal(occ, R.occlude(src, rank, mhw[0], mhw[1], mode, STEPS, 0, STEPS + 1, fill))
        for s in range(STEPS + 1):
            m = R.occluded_mask(rank, ODD_HW[0], ODD_HW[1], mhw[0], mhw[1], STEPS, s)
            filled = m if mode == R.DELETION else ~m
            assert bits_equal(occ[s][~filled], src[~filled])
    assert R.same_bits(res["deletion"]["p_first"], mean_prob) and R.same_bits(res["insertion"]["p_last"], mean_prob)
    assert R.same_bits(res["deletion"]["p_last"], res["insertion"]["p_first"])
    # chunked over the frames: other first_index, the same masks for the same global frame
    a = be.classify_curve(fd[:2], md[:2], None, "deletion", first_index=FIRST)
    b = be.classify_curve(fd[2:], md[2:], None, "deletion", first_index=FIRST + 2)
    assert R.same_bits(np.concatenate([host(a["curve"]), host(b["curve"])]), res["deletion"]["curve"])


def test_handle_refusals():
    be, size, mhw = make_backend("resnet18")
    try:
        frames = dev(synth.synthetic_frames_u8(N, size, size, seed=3))
        maps = dev(faithfulness.random_maps(N, mhw, 0))
        with pytest.raises(_lib.FavError, match="FAV_ERR_INVALID_ARG.*fav_classify_curve: no curve descriptor set"):
            be.classify_curve(frames, maps)
        with pytest.raises(_lib.FavError, match="FAV_ERR_INVALID_ARG.*fav_set_curve: steps=257"):
            be.set_curve(257)
        with pytest.raises(_lib.FavError, match="FAV_ERR_INVALID_ARG.*fav_set_curve: fill.*above 255"):
            be.set_curve(4, fill=1.5)
        be.set_curve(STEPS)
        be.set_curve(2 * STEPS)                                                  # replacing
        be.set_curve(STEPS)
        s = stream()
        curve = torch.full((MAX_BATCH + 1, STEPS + 1), 7.0, dtype=torch.float32, device="cuda")
        rec = torch.full((MAX_BATCH + 1, 8), 7, dtype=torch.int32, device="cuda")
        big = dev(synth.synthetic_frames_u8(MAX_BATCH + 1, size, size, seed=3))
        bigmap = dev(np.zeros((MAX_BATCH + 1, 1025), np.float32))

        def call(n=N, layout=U8, first=0, mh=mhw[0], mw=mhw[1], mode=0, frames_=big.data_ptr(), maps_=bigmap.data_ptr(), classes=None,
                 curve_=curve.data_ptr(), rec_=rec.data_ptr()):
            st = be.lib.fav_classify_curve(be._h, frames_, n, layout, first, maps_, mh, mw, classes, mode, None, None, curve_, rec_, s)
            torch.cuda.synchronize()
            return st, be.lib.fav_last_error(be._h).decode()
        for why, kw, text in (("n above max_batch", dict(n=MAX_BATCH + 1), "n=9 outside [1, max_batch=8]"), ("n 0", dict(n=0), "n=0"),
                              ("1025 cells", dict(mh=25, mw=41), "map 25x41"), ("a side of 257", dict(mh=257, mw=1), "map 257x1"),
                              ("map 0", dict(mw=0), "map 4x0"), ("mode", dict(mode=2), "mode=2"), ("layout", dict(layout=3), "layout"),
                              ("first", dict(first=-1), "first_image_index"), ("first + n", dict(first=2 ** 32 - 3), "first_image_index"),
                              ("null frames", dict(frames_=None), "null"), ("null maps", dict(maps_=None), "null"),
                              ("null curve", dict(curve_=None), "null"), ("null rec", dict(rec_=None), "null"),
                              ("maps + 2", dict(maps_=bigmap.data_ptr() + 2), "misaligned"),
                              ("curve + 2", dict(curve_=curve.data_ptr() + 2), "misaligned"), ("rec + 4", dict(rec_=rec.data_ptr() + 4), "misaligned"),
                              ("classes + 2", dict(classes=rec.data_ptr() + 2), "misaligned"),
                              ("f32 frames + 2", dict(layout=F32, frames_=big.data_ptr() + 2), "aligned")):
            st, msg = call(**kw)
            assert st == 1 and "fav_classify_curve" in msg and text in msg, (why, msg)
            assert bool((curve == 7.0).all()) and bool((rec == 7).all()), why
        assert call()[0] == 0
        # views against a curve descriptor, in both orders
        with pytest.raises(_lib.FavError, match="FAV_ERR_UNSUPPORTED.*fav_set_views: a curve descriptor is set"):
            be.set_views(views.hflip())
        be.set_curve(None)
        be.set_curve(None)
        be.set_views(views.hflip())
        with pytest.raises(_lib.FavError, match="FAV_ERR_UNSUPPORTED.*fav_set_curve: views are set"):
            be.set_curve(STEPS)
        be.set_views(None)
        be.set_curve(STEPS)
        assert call()[0] == 0
    finally:
        be.close()


def test_a_curve_descriptor_changes_no_classify_call():
    be, size, _ = make_backend("resnet18_mc")
    try:
        frames = dev(synth.synthetic_frames_u8(N, size, size, seed=3))

        def snapshot():
            be.set_profiling(True)
            lab, conf, fail, score = (host(v) for v in be.classify_detect(frames, first_index=5))
            prof = be.get_profile()
            ops = [(r["op_index"], r["kind"], r["launches"]) for r in be.get_op_profile()]
            be.set_profiling(False)
            return lab, conf, fail, score, host(be.logits()), {k: v["launches"] for k, v in prof.items()}, ops
        before = snapshot()
        be.set_curve(STEPS)
        during = snapshot()
        be.classify_curve(frames, dev(faithfulness.random_maps(N, (4, 4), 0)))
        be.set_curve(None)
        after = snapshot()
        for other in (during, after):
            for a, b in zip(before[:5], other[:5]):
                assert bits_equal(a, b)
            assert before[5] == other[5] and before[6] == other[6]
    finally:
        be.close()


@pytest.mark.parametrize("kind", ("resnet18", "vit_tiny"))
def test_faithfulness_report(kind):
    be, size, _ = make_backend(kind)
    try:
        frames = dev(synth.synthetic_frames_u8(N, size, size, seed=8))
        rep = be.faithfulness_report(frames, steps=STEPS, seed=3)
        again = be.faithfulness_report(frames, steps=STEPS, seed=3)
        other = be.faithfulness_report(frames, steps=STEPS, seed=4)
        assert not be._map_tap_on and not be._attn_tap_on                        # the tap went on and off around the call
        mh, mw = rep["map_hw"]
        assert rep["n"] + rep["n_nonfinite"] == N and rep["steps"] == STEPS
        pf = rep["per_frame"]
        keep = np.ones(N, bool)
        for r in pf.values():
            keep &= ~np.isnan(r["auc"])
        assert keep.sum() == rep["n"]
        for key, run in (("deletion_auc", "map_deletion"), ("insertion_auc", "map_insertion"), ("random_deletion_auc", "random_deletion"),
                         ("random_insertion_auc", "random_insertion")):
            assert rep[key] == pytest.approx(float(np.mean(pf[run]["auc"][keep].astype(np.float64))), rel=1e-12), key
            assert again[key] == rep[key]
            assert R.same_bits(again["per_frame"][run]["curve"], pf[run]["curve"])
        assert rep["deletion_gain"] == pytest.approx(rep["random_deletion_auc"] - rep["deletion_auc"])
        assert rep["insertion_gain"] == pytest.approx(rep["insertion_auc"] - rep["random_insertion_auc"])
        fc = pf["map_deletion"]["flip_cells"]
        flipped = keep & (fc >= 0)
        if flipped.any():
            assert rep["flip_fraction"] == pytest.approx(float(np.mean(fc[flipped] / (mh * mw))))
        else:
            assert np.isnan(rep["flip_fraction"])
        # the random ranking is a function of the seed: the same maps, hence the same curves, and another seed's differ
        rnd = faithfulness.random_maps(N, (mh, mw), 3)
        direct = be.classify_curve(frames, rnd, None, "deletion")
        assert R.same_bits(host(direct["curve"]), pf["random_deletion"]["curve"])
        assert R.same_bits(other["per_frame"]["map_deletion"]["curve"], pf["map_deletion"]["curve"])
        assert not np.array_equal(faithfulness.random_maps(N, (mh, mw), 4), rnd)
        # the caller's own maps
        own = be.faithfulness_report(frames, steps=STEPS, seed=3, maps=rnd)
        assert R.same_bits(own["per_frame"]["map_deletion"]["curve"], pf["random_deletion"]["curve"])
        assert own["deletion_gain"] == 0.0 and own["insertion_gain"] == 0.0
    finally:
        be.close()


def test_faithfulness_report_on_an_ensemble_needs_maps():
    be, size, mhw = make_backend("ensemble")
    try:
        frames = dev(synth.synthetic_frames_u8(N, size, size, seed=8))
        with pytest.raises(ValueError, match="pass maps="):
            be.faithfulness_report(frames, steps=STEPS)
        rep = be.faithfulness_report(frames, steps=STEPS, maps=faithfulness.random_maps(N, mhw, 1))
        assert rep["n"] + rep["n_nonfinite"] == N
    finally:
        be.close()
