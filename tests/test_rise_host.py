"""RISE saliency, the part that needs no GPU: the numpy reference's own properties (tests/rise_ref.py), fav_check_rise's ranges,
the new symbols in include/fav.h and in the library, the record unpacking, and the coverage condition the end-to-end GPU tests
rely on."""
import ctypes as C
import os
import re

import numpy as np
import pytest

import rise_ref as R
from failure_aware_vision_amd import _lib, rise

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
NEW_SYMBOLS = ("fav_check_rise", "fav_set_rise", "fav_classify_rise", "fav_op_rise_mask", "fav_op_rise_accumulate")
U8, F32 = _lib.LAYOUT_NHWC_U8, _lib.LAYOUT_NHWC_F32
SIZES = ((1, 1), (5, 7), (13, 9), (32, 32))
GRIDS = (1, 2, 3, 7, 15)
CASES = [(hw, g) for hw in SIZES for g in GRIDS if g <= min(hw)]
ids = lambda s: "x".join(map(str, s)) if isinstance(s, tuple) else str(s)  # noqa: E731


# ---- the reference's own properties
@pytest.mark.parametrize("hw,g", CASES, ids=ids)
def test_reference_mask_stays_in_range_and_its_mean_is_keep(hw, g):
    H, W = hw
    total, count = 0, 0
    for keep in (1, 77, 128, 255):
        d = R.Desc(n_masks=40, grid=g, keep=keep, seed=1234 + keep)
        for m in range(d.n_masks):
            mq = R.mask(d, 7, m, H, W)
            assert mq.shape == (H, W) and mq.min() >= 0 and mq.max() <= 256
            if keep == 128:
                total, count = total + int(mq.sum()), count + mq.size
    # the mean is keep / 256 within sampling noise: 40 masks of at least 4 grid bits each, 6 sigma of a single bit's spread
    assert abs(total / count / 256.0 - 0.5) <= 6 * 0.5 / np.sqrt(40.0)


@pytest.mark.parametrize("hw,g", CASES, ids=ids)
def test_reference_all_on_is_256_all_off_is_0_and_the_shift_stays_inside_a_cell(hw, g):
    H, W = hw
    ch, cw = R.cell_sizes(H, W, g)
    assert ch * g >= H and cw * g >= W and (ch - 1) * g < H and (cw - 1) * g < W
    on, off = np.ones((g + 1, g + 1), np.int64), np.zeros((g + 1, g + 1), np.int64)
    for dy in range(ch):
        for dx in range(cw):
            assert (R.upsample(on, g, H, W, dy, dx) == 256).all()
            assert (R.upsample(off, g, H, W, dy, dx) == 0).all()
    seen = set()
    for m in range(64):
        dy, dx = R.shift(g, 99, 5, m, H, W)
        assert 0 <= dy < ch and 0 <= dx < cw
        seen.add((dy, dx))
    assert len(seen) > 1 or ch * cw == 1


def test_reference_bilinear_weights_at_a_single_on_cell():
    # g = 2 on an 8 x 8 frame: cells of 4 pixels.  One ON grid point in the middle, no shift: a tent around pixel 5.5 whose values
    # are the products of the two axes' half-pixel weights
    bits = np.zeros((3, 3), np.int64)
    bits[1, 1] = 1
    mq = R.upsample(bits, 2, 8, 8, 0, 0)
    w = np.array([0, 0, 1, 3, 5, 7, 7, 5], np.int64)           # (2 * 4 - |2p + 1 - 12|) clipped: eighths along an axis
    assert np.array_equal(mq, (256 * w[:, None] * w[None, :] + 32) // 64)


def test_reference_draws_take_the_dropout_byte_order_and_depend_on_every_key():
    from oracle.fav_oracle import philox4x32_10
    x, y, z, w = (int(v) for v in philox4x32_10(np.uint32(2), np.uint32(9), np.uint32(4), np.uint32(R.SITE), 0xDEADBEEF, 0x1234))
    b = R.draws(9, 4, 0x1234DEADBEEF, [2])[0]
    assert [int(v) for v in b[:5]] == [x & 255, (x >> 8) & 255, (x >> 16) & 255, x >> 24, y & 255] and int(b[15]) == w >> 24
    base = R.grid_bits(15, 128, 1, 2, 3)
    assert base.shape == (16, 16)
    for other in (R.grid_bits(15, 128, 2, 2, 3), R.grid_bits(15, 128, 1, 3, 3), R.grid_bits(15, 128, 1, 2, 4),
                  R.grid_bits(15, 128, 1 << 32 | 1, 2, 3)):
        assert not np.array_equal(base, other)
    # the frame index is the low word of first_image_index + i
    assert R.frame_index(2 ** 32 - 1, 1) == 0 and R.frame_index(2 ** 32 + 5, 2) == 7


@pytest.mark.parametrize("size", (1, 5, 7, 13, 32, 224))
def test_reference_sample_pixels_lie_in_their_own_cell(size):
    for m in range(1, min(size, 256) + 1):
        cell = (np.arange(size, dtype=np.int64) * m) // size
        s = R.sample_pixels(size, m)
        for c in range(m):
            lo, hi = R.cell_span(c, size, m)
            own = np.nonzero(cell == c)[0]
            assert own.size and lo == own[0] and hi == own[-1] and cell[s[c]] == c


def test_reference_blend_endpoints_and_rounding():
    d = R.Desc(1, 1, 128, 0, fill_u8=(17, 255, 0), fill_f32_bits=(0x7FC12345, 0x80000000, 0x3F000000))
    rng = np.random.default_rng(0)
    u8 = rng.integers(0, 256, (1, 4, 5, 3), dtype=np.uint8)
    for q, want in ((256, u8), (0, np.broadcast_to(np.array(d.fill_u8, np.uint8), u8.shape))):
        assert np.array_equal(R.blend(u8, np.full((1, 4, 5), q, np.int64), d), want)
    half = R.blend(u8, np.full((1, 4, 5), 128, np.int64), d).astype(np.int64)
    assert np.abs(2 * half - (u8.astype(np.int64) + np.array(d.fill_u8))).max() <= 1
    f32 = rng.integers(0, 2 ** 32, (1, 4, 5, 3), dtype=np.uint32).view(np.float32)
    assert np.array_equal(R.blend(f32, np.full((1, 4, 5), 256, np.int64), d).view(np.uint32), f32.view(np.uint32))
    assert (R.blend(f32, np.zeros((1, 4, 5), np.int64), d).view(np.uint32) == np.array(d.fill_f32_bits, np.uint32)).all()
    ones = np.ones((1, 4, 5, 3), np.float32)
    zero = R.Desc(1, 1, 128, 0, fill_f32_bits=(0, 0, 0))
    mq = rng.integers(0, 257, (1, 4, 5)).astype(np.int64)
    assert np.array_equal(R.blend(ones, mq, zero), np.repeat((mq / 256.0).astype(np.float32)[..., None], 3, axis=-1))


def test_reference_accumulate_of_a_constant_probability_is_that_constant():
    d = R.Desc(n_masks=65, grid=3, keep=100, seed=5)
    k = np.float32(0.3)
    prob = np.full((66, 2), k, np.float32)
    m, rec, cov = R.accumulate(prob, np.array([1, 2], np.int32), d, 11, 32, 32, 7, 7)
    assert (cov > 0).all() and np.abs(m - k).max() <= 2 * 65 * np.spacing(k)
    assert rec[:, 0].tolist() == [1, 2] and (rec[:, 1].view(np.float32) == k).all()
    assert np.abs(rec[:, 5].view(np.float32) - k).max() <= 65 * np.spacing(k)
    # no coverage at all: the +0 rule, a map without a peak above its floor
    none = R.Desc(n_masks=2, grid=1, keep=1, seed=5)
    m, rec, cov = R.accumulate(prob[:3], np.array([1, -1], np.int32), none, 0, 32, 32, 4, 4)
    assert (cov == 0).all() and (m.view(np.uint32) == 0).all()
    assert rec[0].tolist() == [1, R.bits(k), 0, 0, 0, R.bits(np.float32(np.float32(k + k) * np.float32(0.5))), 0, -1]
    assert rec[1].tolist() == [-1, R.NAN_BITS, R.NAN_BITS, -1, R.NAN_BITS, R.NAN_BITS, 0, -1]


# ---- fav_check_rise
def desc(n_masks=64, grid=7, keep=128, seed=1, fill_u8=(128, 128, 128), struct_size=None):
    d = _lib.FavRise()
    d.struct_size = C.sizeof(_lib.FavRise) if struct_size is None else struct_size
    d.n_masks, d.grid, d.keep, d.seed = n_masks, grid, keep, seed
    for c in range(3):
        d.fill_u8[c] = fill_u8[c]
        d.fill_f32_bits[c] = 0x7FC00001          # any word is legal here: a NaN with a payload
    return d


def check(d, H=32, W=32, layout=U8):
    err = C.create_string_buffer(256)
    st = _lib.load().fav_check_rise(C.byref(d) if d is not None else None, H, W, layout, err, len(err))
    return st, err.value.decode()


def test_check_rise_accepts_and_refuses_what_the_header_says():
    assert C.sizeof(_lib.FavRise) == 48 and C.sizeof(_lib.FavRiseRecord) == 32 and _lib.FavRise.seed.offset == 16
    src = open(os.path.join(ROOT, "failure_aware_vision_amd", "csrc", "fav.hip")).read()
    assert "static_assert(sizeof(fav_rise) == 48" in src and "static_assert(sizeof(fav_rise_record) == 32" in src
    for kw in (dict(n_masks=1), dict(n_masks=8192), dict(grid=1), dict(grid=15), dict(keep=1), dict(keep=255),
               dict(fill_u8=(255, 0, 255)), dict(seed=2 ** 64 - 1)):
        assert check(desc(**kw)) == (0, ""), kw
    assert check(desc(grid=1), H=1, W=1) == (0, "") and check(desc(grid=5), H=5, W=7) == (0, "")
    for d, text in ((None, "NULL"), (desc(struct_size=44), "struct_size"), (desc(struct_size=0), "struct_size"),
                    (desc(n_masks=0), "n_masks=0"), (desc(n_masks=8193), "n_masks=8193"), (desc(n_masks=-1), "n_masks=-1"),
                    (desc(grid=0), "grid=0"), (desc(grid=16), "grid=16"), (desc(keep=0), "keep=0"), (desc(keep=256), "keep=256"),
                    (desc(fill_u8=(256, 0, 0)), "fill[0]=256"), (desc(fill_u8=(0, 0, 1000)), "fill[2]=1000")):
        st, msg = check(d)
        assert st == 1 and text in msg, (text, msg)
    # the grid against the frame
    for kw, text in ((dict(H=6, W=32), "grid=7 above min(H, W)=6"), (dict(H=32, W=3), "grid=7 above min(H, W)=3")):
        st, msg = check(desc(), **kw)
        assert st == 1 and text in msg, (kw, msg)
    # the byte range is uint8's alone: under fp32 the other three words are the fill
    assert check(desc(fill_u8=(256, 0, 0)), layout=F32) == (0, "")
    for kw, text in ((dict(H=0), "at least 1"), (dict(W=0), "at least 1"), (dict(W=-3), "at least 1"), (dict(layout=2), "layout"),
                     (dict(H=20000, W=20000), "2^31")):
        st, msg = check(desc(), **kw)
        assert st == 1 and text in msg, (kw, msg)
    # the 32-bit arithmetic of the kernels: 1026 ch cw must stay below 2^31
    assert check(desc(grid=1), H=1446, W=1447) == (0, "")                           # 2092362 cells' worth
    st, msg = check(desc(grid=1), H=1447, W=1447)
    assert st == 1 and "2^31" in msg and "grid=1" in msg, msg
    assert check(desc(grid=15), H=4000, W=4000) == (0, "")
    assert _lib.load().fav_check_rise(C.byref(desc(grid=0)), 32, 32, U8, None, 0) == 1      # err may be NULL


def test_new_symbols_are_declared_and_exported_and_the_abi_stays_2():
    lib = _lib.load()
    header = open(os.path.join(ROOT, "include", "fav.h")).read()
    for name in NEW_SYMBOLS:
        assert re.search(r"\bfav_status\s+%s\s*\(" % name, header), name
        assert hasattr(lib, name) and name in _lib._SIGNATURES, name
    for text in ("typedef struct fav_rise {", "typedef struct fav_rise_record {", "byte first, the order of the dropout draws", "0x715E"):
        assert text in header, text
    assert lib.fav_abi_version() == 2 and "#define FAV_ABI_VERSION 2" in header


def test_unpack_rise_records_and_the_ranges():
    rec = np.arange(16, dtype=np.int32).reshape(2, 8)
    rec[:, 1] = np.array([0.25, 0.5], np.float32).view(np.int32)
    rec[0, 7], rec[1, 7] = -1, 1 | 2 << 8 | 3 << 16 | 4 << 24
    u = rise.unpack_rise_records(rec)
    assert set(u) == set(R.REC_NAMES) | {"x0", "y0", "x1", "y1"}
    assert u["p_full"].dtype == np.float32 and u["p_full"].tolist() == [0.25, 0.5] and u["class_id"].tolist() == [0, 8]
    assert u["n_above"].tolist() == [6, 14] and np.shares_memory(u["p_full"], rec)
    assert [u[k].tolist() for k in ("x0", "y0", "x1", "y1")] == [[-1, 1], [-1, 2], [-1, 3], [-1, 4]]
    with pytest.raises(ValueError):
        rise.unpack_rise_records(np.zeros((2, 7), np.int32))
    assert rise.RISE_RECORD_DWORDS * 4 == C.sizeof(_lib.FavRiseRecord)
    assert (rise.RISE_MAX_MASKS, rise.RISE_MAX_GRID, rise.RISE_KEEP_RANGE) == (8192, 15, (1, 255))
    assert rise.keep_threshold(0.5) == 128 and rise.keep_threshold(1 / 256) == 1 and rise.keep_threshold(0.997) == 255
    assert check(desc(n_masks=rise.RISE_MAX_MASKS + 1))[0] == 1 and check(desc(grid=rise.RISE_MAX_GRID + 1))[0] == 1


# ---- a condition the GPU tests rely on
def test_the_end_to_end_inputs_cover_every_cell():
    d, (mh, mw) = R.E2E_DESC, R.E2E_MAP
    assert (d.n_masks, d.grid, (mh, mw)) == (6, 3, (4, 4))
    for size in R.E2E_SIZES:
        prob = np.full((d.n_masks + 1, R.E2E_MAX_BATCH), 0.5, np.float32)
        for first in (R.E2E_FIRST, 0):
            _, _, cov = R.accumulate(prob, np.zeros(R.E2E_MAX_BATCH, np.int32), d, first, size, size, mh, mw)
            assert cov.shape == (R.E2E_MAX_BATCH, mh * mw) and (cov > 0).all(), (size, first, cov.min())


# ---- refusal texts, word for word.  fav_check_rise and every refusal of fav_op_rise_mask come before any launch, so none
# needs a device and an address only has to look like one.  FB: the bytes of an 8 x 8 uint8 frame.  The last cases of the op hold
# the order of its refusals: the frames' alignment, n * (m1 - m0), the overlap.
FRAMES, OUT, FB = 0x10000, 0x100000, 8 * 8 * 3
CHECK_RISE_TEXTS = (
    (None, "desc is NULL"),
    (dict(struct_size=44), "struct_size is not sizeof(fav_rise)"),
    (dict(struct_size=0), "struct_size is not sizeof(fav_rise)"),
    (dict(n_masks=0), "n_masks=0 outside [1, 8192]"),
    (dict(n_masks=8193), "n_masks=8193 outside [1, 8192]"),
    (dict(n_masks=-1), "n_masks=-1 outside [1, 8192]"),
    (dict(grid=0), "grid=0 outside [1, 15]"),
    (dict(grid=16), "grid=16 outside [1, 15]"),
    (dict(keep=0), "keep=0 outside [1, 255]"),
    (dict(keep=256), "keep=256 outside [1, 255]"),
    (dict(fill_u8=(256, 0, 0)), "fill[0]=256 is above 255, the largest uint8"),
    (dict(fill_u8=(0, 0, 1000)), "fill[2]=1000 is above 255, the largest uint8"),
)
CHECK_RISE_FRAME_TEXTS = (
    (dict(H=6, W=32), "grid=7 above min(H, W)=6"),
    (dict(H=32, W=3), "grid=7 above min(H, W)=3"),
    (dict(H=0), "frame size 0x32: H and W must be at least 1"),
    (dict(W=0), "frame size 32x0: H and W must be at least 1"),
    (dict(W=-3), "frame size 32x-3: H and W must be at least 1"),
    (dict(layout=2), "unknown layout"),
    (dict(H=20000, W=20000), "H * W above (2^31 - 1) / 12 pixels"),
)
MASK_TEXTS = (
    (dict(frames=None), "fav_op_rise_mask: null pointer"),
    (dict(out=None), "fav_op_rise_mask: null pointer"),
    (dict(d=None), "fav_op_rise_mask: desc is NULL"),
    (dict(d=dict(struct_size=40)), "fav_op_rise_mask: struct_size is not sizeof(fav_rise)"),
    (dict(m0=3, m1=3), "fav_op_rise_mask: masks [3, 3) outside 0 <= m0 < m1 <= n_masks = 5"),
    (dict(m0=4, m1=3), "fav_op_rise_mask: masks [4, 3) outside 0 <= m0 < m1 <= n_masks = 5"),
    (dict(m0=-1, m1=3), "fav_op_rise_mask: masks [-1, 3) outside 0 <= m0 < m1 <= n_masks = 5"),
    (dict(m1=6), "fav_op_rise_mask: masks [0, 6) outside 0 <= m0 < m1 <= n_masks = 5"),
    (dict(d=dict(n_masks=0)), "fav_op_rise_mask: n_masks=0 outside [1, 8192]"),
    (dict(d=dict(n_masks=8193)), "fav_op_rise_mask: n_masks=8193 outside [1, 8192]"),
    (dict(d=dict(grid=0)), "fav_op_rise_mask: grid=0 outside [1, 15]"),
    (dict(d=dict(grid=16)), "fav_op_rise_mask: grid=16 outside [1, 15]"),
    (dict(d=dict(grid=9)), "fav_op_rise_mask: grid=9 above min(H, W)=8"),
    (dict(d=dict(keep=0)), "fav_op_rise_mask: keep=0 outside [1, 255]"),
    (dict(d=dict(keep=256)), "fav_op_rise_mask: keep=256 outside [1, 255]"),
    (dict(d=dict(fill_u8=(1, 256, 3))), "fav_op_rise_mask: fill[1]=256 is above 255, the largest uint8"),
    (dict(n=0), "fav_op_rise_mask: n must be at least 1"),
    (dict(H=0), "fav_op_rise_mask: frame size 0x8: H and W must be at least 1"),
    (dict(layout=2), "fav_op_rise_mask: unknown layout"),
    (dict(frames=FRAMES + 2, layout=F32, m1=1), "fav_op_rise_mask: fp32 frames and out must be 4-byte aligned"),
    (dict(out=OUT + 1, layout=F32, m1=1), "fav_op_rise_mask: fp32 frames and out must be 4-byte aligned"),
    (dict(n=2 ** 31 - 1, m1=2), "fav_op_rise_mask: n * (m1 - m0) above 2^31 - 1"),
    (dict(out=FRAMES, m1=1), "fav_op_rise_mask: out overlaps frames"),
    (dict(out=FRAMES + 2 * FB - 1, m1=1), "fav_op_rise_mask: out overlaps frames"),
    (dict(frames=OUT + 3 * FB), "fav_op_rise_mask: out overlaps frames"),
    (dict(frames=OUT + 2 * 2 * FB - 1, m1=2), "fav_op_rise_mask: out overlaps frames"),
    (dict(frames=OUT + 2, layout=F32, n=2 ** 31 - 1), "fav_op_rise_mask: fp32 frames and out must be 4-byte aligned"),
    (dict(out=FRAMES, n=2 ** 31 - 1), "fav_op_rise_mask: n * (m1 - m0) above 2^31 - 1"),
)


def test_check_rise_refusal_texts():
    for kw, text in CHECK_RISE_TEXTS:
        assert check(None if kw is None else desc(**kw)) == (1, text), kw
    for kw, text in CHECK_RISE_FRAME_TEXTS:
        assert check(desc(), **kw) == (1, text), kw


def test_op_rise_mask_refusal_texts():
    lib = _lib.load()

    def args(frames=FRAMES, out=OUT, n=2, H=8, W=8, layout=U8, d=dict(), first=0, m0=0, m1=5):      # d: what differs from a good descriptor
        return (frames, out, n, H, W, layout, None if d is None else C.byref(desc(**dict(dict(n_masks=5, grid=3, fill_u8=(1, 2, 3)), **d))),
                first, m0, m1, None)
    for kw, text in MASK_TEXTS:
        assert lib.fav_op_rise_mask(*args(**kw)) == 1, kw
        assert lib.fav_last_error(None).decode() == text, kw
