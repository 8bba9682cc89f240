"""Deletion / insertion curves, the part that needs no GPU: fav_check_curve's ranges, the new symbols in include/fav.h and in
the library, the numpy reference (tests/faith_ref.py) against independent numpy, and the host helpers of
failure_aware_vision_amd.faithfulness."""
import ctypes as C
import os
import re

import numpy as np
import pytest

import faith_ref as R
from failure_aware_vision_amd import _lib, faithfulness

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
NEW_SYMBOLS = ("fav_check_curve", "fav_set_curve", "fav_classify_curve", "fav_op_rank_cells", "fav_op_occlude",
               "fav_op_head_class_prob", "fav_op_curve")
U8, F32 = _lib.LAYOUT_NHWC_U8, _lib.LAYOUT_NHWC_F32


def desc(steps=16, fill_u8=(128, 128, 128), struct_size=None):
    d = _lib.FavCurve()
    d.struct_size = C.sizeof(_lib.FavCurve) if struct_size is None else struct_size
    d.steps = steps
    for c in range(3):
        d.fill_u8[c] = fill_u8[c]
        d.fill_f32_bits[c] = 0x7FC00001          # any word is legal here: a NaN with a payload
    return d


def check(d, H=32, W=32, layout=U8):
    err = C.create_string_buffer(256)
    st = _lib.load().fav_check_curve(C.byref(d) if d is not None else None, H, W, layout, err, len(err))
    return st, err.value.decode()


def test_check_curve_accepts_and_refuses_what_the_header_says():
    assert C.sizeof(_lib.FavCurve) == 32 and C.sizeof(_lib.FavCurveRecord) == 32
    for steps in (1, 16, 256):
        assert check(desc(steps)) == (0, "")
    assert check(desc(16, (255, 0, 255))) == (0, "")
    for d, text in ((desc(0), "steps=0"), (desc(257), "steps=257"), (desc(-1), "steps=-1"), (desc(struct_size=28), "struct_size"),
                    (desc(struct_size=0), "struct_size"), (desc(16, (256, 0, 0)), "fill[0]=256"), (desc(16, (0, 0, 1000)), "fill[2]=1000"),
                    (None, "NULL")):
        st, msg = check(d)
        assert st == 1 and text in msg, (text, msg)
    # the byte range is uint8's alone: under fp32 the other three words are the fill
    assert check(desc(16, (256, 0, 0)), layout=F32) == (0, "")
    for kw, text in ((dict(H=0), "at least 1"), (dict(W=0), "at least 1"), (dict(layout=2), "layout"),
                     (dict(H=20000, W=20000), "2^31")):
        st, msg = check(desc(), **kw)
        assert st == 1 and text in msg, (kw, msg)
    assert _lib.load().fav_check_curve(C.byref(desc(0)), 32, 32, U8, None, 0) == 1      # err may be NULL


def test_new_symbols_are_declared_and_exported_and_the_abi_stays_2():
    lib = _lib.load()
    header = open(os.path.join(ROOT, "include", "fav.h")).read()
    for name in NEW_SYMBOLS:
        assert re.search(r"\bfav_status\s+%s\s*\(" % name, header), name
        assert hasattr(lib, name) and name in _lib._SIGNATURES, name
    for text in ("fav_curve_record", "FAV_CURVE_DELETION = 0", "FAV_CURVE_INSERTION = 1", "typedef struct fav_curve {"):
        assert text in header, text
    assert lib.fav_abi_version() == 2 and "#define FAV_ABI_VERSION 2" in header


@pytest.mark.parametrize("cells", (1, 2, 7, 49, 196))
def test_reference_ranks_equal_lexsort(cells):
    maps = R.tricky_maps(3, cells, seed=cells)
    got = R.rank_cells(maps)
    for i in range(3):
        m = maps[i]
        order = np.lexsort((np.arange(cells), -m, np.isnan(m)))        # NaNs last, then by value descending, then by index
        want = np.empty(cells, np.int32)
        want[order] = np.arange(cells)
        assert np.array_equal(got[i], want), i
        assert sorted(got[i]) == list(range(cells))
    # the vectorised rows agree with the rule cell by cell
    m = maps[0]
    with np.errstate(invalid="ignore"):
        for c in range(min(cells, 12)):
            assert got[0, c] == sum(R.before(m[a], a, m[c], c) for a in range(cells))


def test_reference_orders_signed_zeros_by_index_and_nans_behind_minus_infinity():
    m = np.array([[-0.0, 0.0, np.nan, -np.inf, 0.0, np.nan, np.inf]], np.float32)
    assert R.rank_cells(m)[0].tolist() == [1, 2, 5, 4, 3, 6, 0]


@pytest.mark.parametrize("hw,mhw,S", (((5, 7), (3, 5), 4), ((33, 47), (7, 7), 16), ((5, 7), (32, 32), 16), ((8, 8), (2, 2), 9),
                                        ((1, 1), (1, 1), 1)))
def test_reference_occlusion_sets_nest_and_complement(hw, mhw, S):
    (H, W), (mh, mw) = hw, mhw
    cells = mh * mw
    rng = np.random.default_rng(S)
    n = 2
    rank = np.stack([rng.permutation(cells) for _ in range(n)]).astype(np.int32)
    k = R.step_counts(S, cells)
    assert k[0] == 0 and k[S] == cells and (np.diff(k) >= 0).all()
    frames = rng.integers(0, 256, (n, H, W, 3), dtype=np.uint8)
    fill = (7, 300 & 255, 9)
    prev = np.zeros((n, H, W), bool)
    dele = R.occlude(frames, rank, mh, mw, R.DELETION, S, 0, S + 1, fill)
    ins = R.occlude(frames, rank, mh, mw, R.INSERTION, S, 0, S + 1, fill)
    px = np.array(fill, np.uint8)
    for s in range(S + 1):
        m = R.occluded_mask(rank, H, W, mh, mw, S, s)
        assert (m | ~prev).all()                                      # nested: what was occluded stays occluded
        assert m.reshape(n, -1).sum(axis=1).tolist() == [int((rank[i][R.cell_of(H, W, mh, mw)] < k[s]).sum()) for i in range(n)]
        prev = m
        # deletion step s and insertion step s are complementary: together they show every pixel once, and fill it once
        assert (np.where(m[..., None], ins[s], dele[s]) == frames).all()
        assert (np.where(m[..., None], dele[s], ins[s]) == px).all()
    assert not R.occluded_mask(rank, H, W, mh, mw, S, 0).any() and R.occluded_mask(rank, H, W, mh, mw, S, S).all()   # the union
    assert (dele[0] == frames).all() and (ins[S] == frames).all() and (dele[S] == px).all() and (ins[0] == px).all()
    # single steps concatenate to the whole
    parts = np.concatenate([R.occlude(frames, rank, mh, mw, R.DELETION, S, s, s + 1, fill) for s in range(S + 1)])
    assert np.array_equal(parts, dele)


@pytest.mark.parametrize("S", (1, 2, 16, 256))
def test_reference_auc_is_the_trapezoid_rule(S):
    rng = np.random.default_rng(S)
    n = 6
    prob = rng.random((S + 1, n)).astype(np.float32)
    labels = rng.integers(0, 3, (S + 1, n)).astype(np.int32)
    classes = np.array([0, 1, 2, 0, 1, -1], np.int32)
    for mode in (R.DELETION, R.INSERTION):
        cv, rec = R.curve(prob, labels, classes, S, 49, mode)
        assert np.array_equal(cv, prob.T)
        auc = rec[:, 1].view(np.float32)
        trapz = getattr(np, "trapezoid", None) or np.trapz
        want = trapz(prob.astype(np.float64), dx=1.0 / S, axis=0)
        assert np.abs(auc[:5] - want[:5]).max() <= 1e-6 * np.abs(want[:5]).max()
        assert np.array_equal(rec[:5, 2].view(np.float32), prob[0, :5]) and np.array_equal(rec[:5, 4].view(np.float32), prob[S, :5])
        assert np.array_equal(rec[:5, 5].view(np.float32), prob.min(axis=0)[:5])
        for i in range(5):
            hit = (labels[:, i] == classes[i]) if mode == R.INSERTION else (labels[:, i] != classes[i])
            flip = int(np.argmax(hit)) if hit.any() else -1
            assert rec[i, 3] == flip and rec[i, 6] == (-1 if flip < 0 else flip * 49 // S) and rec[i, 7] == 0
        assert rec[5].tolist() == [-1, R.NAN_BITS, R.NAN_BITS, -1, R.NAN_BITS, R.NAN_BITS, -1, 0]


def test_unpack_curve_records_and_random_maps():
    rec = np.arange(16, dtype=np.int32).reshape(2, 8)
    rec[:, 1] = np.array([0.25, 0.5], np.float32).view(np.int32)
    u = faithfulness.unpack_curve_records(rec)
    assert set(u) == {"class_id", "auc", "p_first", "flip_step", "p_last", "p_min", "flip_cells"}
    assert u["auc"].dtype == np.float32 and u["auc"].tolist() == [0.25, 0.5] and u["class_id"].tolist() == [0, 8]
    assert u["flip_cells"].tolist() == [6, 14] and np.shares_memory(u["auc"], rec)
    with pytest.raises(ValueError):
        faithfulness.unpack_curve_records(np.zeros((2, 7), np.int32))
    a, b, c = faithfulness.random_maps(4, (7, 7), 3), faithfulness.random_maps(4, (7, 7), 3), faithfulness.random_maps(4, (7, 7), 4)
    assert a.dtype == np.float32 and a.shape == (4, 7, 7) and np.array_equal(a, b) and not np.array_equal(a, c)
    for i in range(4):
        assert sorted(a[i].ravel().tolist()) == list(range(49))        # a permutation: no ties
    assert not np.array_equal(a[0], a[1])
    with pytest.raises(ValueError):
        faithfulness.random_maps(1, (33, 32), 0)


def test_summarize_curves_leaves_nan_frames_out():
    def res(auc, flip=(3, -1, 5)):
        return dict(auc=np.array(auc, np.float32), flip_cells=np.array(flip, np.int32))
    rep = faithfulness.summarize_curves(res([0.2, 0.4, np.nan]), res([0.6, 0.8, 0.1]), res([0.5, 0.5, 0.5]), res([0.3, 0.5, 0.2]), 10)
    assert rep["n"] == 2 and rep["n_nonfinite"] == 1
    assert rep["deletion_auc"] == pytest.approx(0.3) and rep["insertion_auc"] == pytest.approx(0.7)
    assert rep["deletion_gain"] == pytest.approx(0.2) and rep["insertion_gain"] == pytest.approx(0.3)
    assert rep["flip_fraction"] == pytest.approx(0.3)


# ---- refusal texts, word for word.  fav_check_curve and every refusal of fav_op_occlude and fav_op_views come before any
# launch, so none needs a device and an address only has to look like one.  FB: the bytes of an 8 x 8 uint8 frame.  The last
# cases of each op hold the order of its refusals: the frames' alignment, the op's own complaint, n * count, the overlap.
FRAMES, OUT, RANK, FB = 0x10000, 0x100000, 0x200000, 8 * 8 * 3
CHECK_CURVE_TEXTS = (
    (dict(steps=0), "steps=0 outside [1, 256]"),
    (dict(steps=257), "steps=257 outside [1, 256]"),
    (dict(steps=-1), "steps=-1 outside [1, 256]"),
    (dict(struct_size=28), "struct_size is not sizeof(fav_curve)"),
    (dict(struct_size=0), "struct_size is not sizeof(fav_curve)"),
    (dict(fill_u8=(256, 0, 0)), "fill[0]=256 is above 255, the largest uint8"),
    (dict(fill_u8=(0, 0, 1000)), "fill[2]=1000 is above 255, the largest uint8"),
    (None, "desc is NULL"),
)
CHECK_CURVE_FRAME_TEXTS = (
    (dict(H=0), "frame size 0x32: H and W must be at least 1"),
    (dict(W=0), "frame size 32x0: H and W must be at least 1"),
    (dict(layout=2), "unknown layout"),
    (dict(H=20000, W=20000), "H * W above (2^31 - 1) / 12 pixels"),
)
OCCLUDE_TEXTS = (
    (dict(frames=None), "fav_op_occlude: null pointer"),
    (dict(out=None), "fav_op_occlude: null pointer"),
    (dict(rank=None), "fav_op_occlude: null pointer"),
    (dict(fill=None), "fav_op_occlude: null pointer"),
    (dict(s0=3, s1=3), "fav_op_occlude: steps [3, 3) outside 0 <= s0 < s1 <= S + 1 = 17"),
    (dict(s0=4, s1=3), "fav_op_occlude: steps [4, 3) outside 0 <= s0 < s1 <= S + 1 = 17"),
    (dict(s0=-1, s1=3), "fav_op_occlude: steps [-1, 3) outside 0 <= s0 < s1 <= S + 1 = 17"),
    (dict(s1=18), "fav_op_occlude: steps [0, 18) outside 0 <= s0 < s1 <= S + 1 = 17"),
    (dict(S=0, s1=1), "fav_op_occlude: steps=0 outside [1, 256]"),
    (dict(S=257), "fav_op_occlude: steps=257 outside [1, 256]"),
    (dict(fill=(1, 256, 3)), "fav_op_occlude: fill[1]=256 is above 255, the largest uint8"),
    (dict(n=0), "fav_op_occlude: n must be at least 1"),
    (dict(H=0), "fav_op_occlude: frame size 0x8: H and W must be at least 1"),
    (dict(layout=2), "fav_op_occlude: unknown layout"),
    (dict(mode=2), "fav_op_occlude: mode=2 is not a fav_curve_mode value"),
    (dict(mh=0), "fav_op_occlude: map 0x2: needs 1 <= mh, mw <= 256 and mh * mw <= 1024 cells"),
    (dict(mh=25, mw=41), "fav_op_occlude: map 25x41: needs 1 <= mh, mw <= 256 and mh * mw <= 1024 cells"),
    (dict(mh=257, mw=1), "fav_op_occlude: map 257x1: needs 1 <= mh, mw <= 256 and mh * mw <= 1024 cells"),
    (dict(frames=FRAMES + 2, layout=F32, s1=1), "fav_op_occlude: fp32 frames and out must be 4-byte aligned"),
    (dict(out=OUT + 1, layout=F32, s1=1), "fav_op_occlude: fp32 frames and out must be 4-byte aligned"),
    (dict(rank=RANK + 2), "fav_op_occlude: rank_dev must be 4-byte aligned"),
    (dict(n=2 ** 31 - 1, s1=2), "fav_op_occlude: n * (s1 - s0) above 2^31 - 1"),
    (dict(out=FRAMES, s1=1), "fav_op_occlude: out overlaps frames"),
    (dict(out=FRAMES + 2 * FB - 1, s1=1), "fav_op_occlude: out overlaps frames"),
    (dict(frames=OUT + 5 * FB), "fav_op_occlude: out overlaps frames"),
    (dict(frames=OUT + 2 * 2 * FB - 1, s1=2), "fav_op_occlude: out overlaps frames"),
    (dict(frames=OUT + 2, out=OUT + 1, layout=F32, rank=RANK + 2, n=2 ** 31 - 1),
     "fav_op_occlude: fp32 frames and out must be 4-byte aligned"),
    (dict(out=FRAMES, rank=RANK + 2, n=2 ** 31 - 1), "fav_op_occlude: rank_dev must be 4-byte aligned"),
    (dict(out=FRAMES, n=2 ** 31 - 1), "fav_op_occlude: n * (s1 - s0) above 2^31 - 1"),
)
VIEWS_TEXTS = (
    (dict(n_views=65), "fav_op_views: n_views=65 outside [1, FAV_MAX_VIEWS=64]"),
    (dict(n_views=0), "fav_op_views: n_views=0 outside [1, FAV_MAX_VIEWS=64]"),
    (dict(frames=None), "fav_op_views: null pointer"),
    (dict(out=None), "fav_op_views: null pointer"),
    (dict(view=None), "fav_op_views: views is NULL"),
    (dict(n=0), "fav_op_views: n, H and W must be at least 1"),
    (dict(H=0), "fav_op_views: n, H and W must be at least 1"),
    (dict(layout=2), "fav_op_views: unknown layout"),
    (dict(W=4, view=(0, 0, 1, 0, 0, 0)), "fav_op_views: view 0: transpose needs H == W, the frames are 8x4"),
    (dict(view=(0, 0, 0, 0, 0, 3)), "fav_op_views: view 0: border=3 is not a fav_border value"),
    (dict(frames=FRAMES + 2, layout=F32), "fav_op_views: fp32 frames and out must be 4-byte aligned"),
    (dict(out=OUT + 1, layout=F32), "fav_op_views: fp32 frames and out must be 4-byte aligned"),
    (dict(H=20000, W=20000), "fav_op_views: H * W above (2^31 - 1) / 12 pixels"),
    (dict(n=2 ** 31 - 1, n_views=2), "fav_op_views: n * n_views above 2^31 - 1"),
    (dict(out=FRAMES), "fav_op_views: out overlaps frames"),
    (dict(out=FRAMES + 2 * FB - 1), "fav_op_views: out overlaps frames"),
    (dict(frames=OUT + 3 * FB, n_views=5), "fav_op_views: out overlaps frames"),
    (dict(frames=OUT + 2 * 2 * FB - 1, n_views=2), "fav_op_views: out overlaps frames"),
    (dict(frames=OUT + 2, layout=F32, H=20000, W=20000, n=2 ** 31 - 1, n_views=2),
     "fav_op_views: fp32 frames and out must be 4-byte aligned"),
    (dict(out=FRAMES, H=20000, W=20000, n=2 ** 31 - 1, n_views=2), "fav_op_views: H * W above (2^31 - 1) / 12 pixels"),
    (dict(out=FRAMES, n=2 ** 31 - 1, n_views=2), "fav_op_views: n * n_views above 2^31 - 1"),
)


def op_text(fn, args):
    assert fn(*args, None) == 1, args
    return _lib.load().fav_last_error(None).decode()


def test_check_curve_refusal_texts():
    for kw, text in CHECK_CURVE_TEXTS:
        assert check(None if kw is None else desc(**kw)) == (1, text), kw
    for kw, text in CHECK_CURVE_FRAME_TEXTS:
        assert check(desc(), **kw) == (1, text), kw


def test_op_occlude_refusal_texts():
    def args(frames=FRAMES, out=OUT, n=2, H=8, W=8, layout=U8, rank=RANK, mh=2, mw=2, mode=0, S=16, s0=0, s1=17, fill=(1, 2, 3)):
        return (frames, out, n, H, W, layout, rank, mh, mw, mode, S, s0, s1, None if fill is None else (C.c_uint32 * 3)(*fill))
    for kw, text in OCCLUDE_TEXTS:
        assert op_text(_lib.load().fav_op_occlude, args(**kw)) == text, kw


def test_op_views_refusal_texts():
    def args(frames=FRAMES, out=OUT, n=2, H=8, W=8, layout=U8, view=(0, 0, 0, 0, 0, 0), n_views=1):
        return (frames, out, n, H, W, layout, None if view is None else (_lib.FavView * 65)(*[_lib.FavView(*view)] * 65), n_views)
    for kw, text in VIEWS_TEXTS:
        assert op_text(_lib.load().fav_op_views, args(**kw)) == text, kw
