"""tests/dropout_ref.py on the CPU: the reference of the MC-Dropout descriptor agrees with the oracle's dropout_keep
wherever that is defined, its edge list holds the edges it claims, and its masks have the statistics MC-Dropout needs -
the kept share, and independence across every counter word.  tests/test_gpu_pool_dropout_edges.py demands bit-equality of
every kernel with this reference, so what is shown here carries over to the kernels without a statistical GPU test.
Needs no GPU; the fav_create rejection at the end runs before a device is looked for."""
import ctypes as C
import math

import numpy as np
import pytest

import dropout_ref as R
from oracle import fav_oracle as O

N_STAT = 1 << 18                 # elements per mask of the statistical tests
SIGMAS = 5.0                     # a fair generator leaves a 5-sigma band once in 1.7 million draws
THRESHOLDS = (0, 1, 26, 64, 128, 255)


def test_edge_list_holds_the_edges_it_claims():
    E = R.EDGE_DESCRIPTORS
    assert len(set(R.EDGE_IDS)) == len(E)
    assert {0, 1, 128, 255} <= {d.threshold for d in E}
    assert {0, R.M32 - 1, R.M32, (1 << 64) - 1} <= {d.seed for d in E}
    assert {0, 16, (1 << 31) - 1} <= {d.site for d in E}
    assert {0, R.M32 - 2, (1 << 40) + 5} <= {d.first_image_index for d in E}
    assert any(d.n_img == 1 for d in E)
    assert any(d.v0 % d.n_img != 0 for d in E)
    assert any(d.rows < d.n_img and d.v0 // d.n_img != (d.v0 + d.rows - 1) // d.n_img for d in E)
    assert any(d.v0 + d.rows == R.V_MAX for d in E)
    for d in E:                                                   # every entry is inside the documented ranges
        assert 0 <= d.site < 1 << 31 and 0 <= d.threshold <= 255 and d.n_img >= 1 and d.rows >= 1
        assert 0 <= d.v0 and d.v0 + d.rows <= R.V_MAX
        assert math.isfinite(float(R.scale_of(d.threshold))) and R.scale_of(d.threshold) > 0
        assert R.scale_of(d.threshold) == O.dropout_scale(d.threshold)
    wrap = next(d for d in E if d.name == "first_2p32m2")
    assert [R.row_index(wrap, r)[2] for r in range(wrap.rows)] == [R.M32 - 2, R.M32 - 1, 0, 1]
    win = next(d for d in E if d.name == "window_wraps")
    assert [R.row_index(win, r)[:2] for r in range(win.rows)] == [(0, 2), (1, 0)]
    assert R.row_index(next(d for d in E if d.name == "first_2p40p5"), 1)[2] == 6
    assert R.row_index(next(d for d in E if d.name == "v_max_n_img1"), 2)[0] == (1 << 31) - 2


@pytest.mark.parametrize("desc", R.EDGE_DESCRIPTORS, ids=R.EDGE_IDS)
@pytest.mark.parametrize("n_elem", [16, 48, 1000])
def test_reference_agrees_with_the_oracle_where_it_is_defined(desc, n_elem):
    """O.dropout_keep takes the frame index as a uint32: it is defined where first_image_index + i needs no reduction."""
    compared = 0
    for r in range(desc.rows):
        t, i, frame = R.row_index(desc, r)
        if desc.first_image_index + i >= R.M32:
            continue
        ne16 = (n_elem + 15) // 16 * 16
        ref = O.dropout_keep(desc.seed, t, desc.site, np.array([desc.first_image_index + i]), ne16, desc.threshold)[0]
        assert np.array_equal(R.keep_mask(desc, r, n_elem), ref[:n_elem]), (desc.name, r)
        compared += 1
    undefined = {"first_2p32m2": 2, "first_2p40p5": desc.rows}.get(desc.name, 0)
    assert compared == desc.rows - undefined


def test_reduced_frame_word_is_the_low_32_bits():
    """Frames 2^32 apart share their masks, and the draws are what Philox gives for the reduced word."""
    a = R._d("a", first=(1 << 40) + 5)
    b = R._d("b", first=5)
    for r in range(3):
        assert np.array_equal(R.draws(a, r, 64), R.draws(b, r, 64))
    w = O.philox4x32_10(np.uint32(2), np.uint32(5), np.uint32(0), np.uint32(3), 0x90ABCDEF, 0x12345678)
    assert list(R.draws(b, 0, 48)[32:36]) == [(int(w[0]) >> s) & 0xFF for s in (0, 8, 16, 24)]
    assert int(R.draws(b, 0, 48)[47]) == int(w[3]) >> 24


def test_apply_scales_rounds_once_and_drops_to_plus_zero():
    d = R._d("x", threshold=26)
    x = O.bf16_round(np.linspace(-3, 3, 64).astype(np.float32))
    y = R.apply(d, 0, x)
    keep = R.keep_mask(d, 0, 64)
    assert 0 < keep.sum() < 64
    assert np.array_equal(y[keep], O.bf16_round(x[keep] * R.scale_of(26)))
    assert not np.signbit(y[~keep]).any() and not y[~keep].any()
    assert np.array_equal(R.apply(R._d("z", threshold=0), 0, x), x)          # threshold 0: the identity


def binom_sigma(q, n):
    return math.sqrt(q * (1.0 - q) / n)


def pair_cases(thr):
    """(name, descriptor a, row a, descriptor b, row b): two masks whose counters differ in exactly one word."""
    k = dict(threshold=thr)
    s = R._d("s", n_img=1, v0=11, rows=2, **k)                               # rows 0, 1: samples t = 11, 12 of one frame
    f = R._d("f", n_img=2, v0=0, rows=2, **k)                                # rows 0, 1: frames 40, 41 of one sample
    w = R._d("w", n_img=2, v0=0, rows=2, first=R.M32 - 1, **k)               # frame words 2^32 - 1 and 0
    return [("samples t, t+1", s, 0, s, 1),
            ("two sites", R._d("a", site=3, **k), 0, R._d("b", site=4, **k), 0),
            ("consecutive frames", f, 0, f, 1),
            ("frames 2^32-1 and 0", w, 0, w, 1)]


@pytest.mark.parametrize("thr", THRESHOLDS)
def test_mask_statistics(thr):
    """Kept share within five binomial standard deviations of 1 - thr/256; the share of equal bits between two masks whose
    counters differ in ONE word within five binomial standard deviations (of that share, over N_STAT independent pairs) of
    p^2 + (1-p)^2.  A generator that ignored the word would give equality 1.0.  At thr = 0 both bands have width zero:
    everything is kept and every pair is equal."""
    p = thr / 256.0
    q = p * p + (1.0 - p) * (1.0 - p)
    for name, da, ra, db, rb in pair_cases(thr):
        ma, mb = R.keep_mask(da, ra, N_STAT), R.keep_mask(db, rb, N_STAT)
        for m in (ma, mb):
            share = float(m.mean())
            print(f"thr {thr} {name}: kept {share:.6f} expected {1 - p:.6f} band {SIGMAS * binom_sigma(p, N_STAT):.6f}")
            assert abs(share - (1.0 - p)) <= SIGMAS * binom_sigma(p, N_STAT), (name, share)
        eq = float((ma == mb).mean())
        print(f"thr {thr} {name}: equal {eq:.6f} expected {q:.6f} band {SIGMAS * binom_sigma(q, N_STAT):.6f}")
        assert abs(eq - q) <= SIGMAS * binom_sigma(q, N_STAT), (name, eq)
        if thr:
            assert eq < 1.0
            assert not np.array_equal(R.draws(da, ra, 4096), R.draws(db, rb, 4096))


def test_chunk_word_and_seed_halves_matter():
    """The remaining inputs of the counter and the key: consecutive chunks, and seeds that differ in one half only."""
    d = R._d("c", threshold=128)
    dr = R.draws(d, 0, N_STAT).reshape(-1, 16)
    eq = float(((dr[:-1] >= 128) == (dr[1:] >= 128)).mean())
    assert abs(eq - 0.5) <= SIGMAS * binom_sigma(0.5, dr[:-1].size)
    for other in (d.seed ^ 1, d.seed ^ (1 << 32)):
        eq = float((R.keep_mask(d, 0, N_STAT) == R.keep_mask(d._replace(seed=other), 0, N_STAT)).mean())
        assert abs(eq - 0.5) <= SIGMAS * binom_sigma(0.5, N_STAT)


def test_fav_create_refuses_a_dropout_p_that_rounds_to_256():
    """round(256 p) = 256 would drop every element with an infinite scale: refused by fav_create itself, before any device
    is looked for; the largest p below it is still a configuration error of no kind here."""
    pytest.importorskip("torch")
    from failure_aware_vision_amd import _lib
    lib = _lib.load()
    cfg = _lib.FavConfig()
    lib.fav_default_config(C.byref(cfg), _lib.ARCH_RESNET18_CIFAR)
    cfg.struct_size = C.sizeof(_lib.FavConfig)
    cfg.num_classes, cfg.in_h, cfg.in_w, cfg.max_batch = 10, 32, 32, 2
    cfg.n_samples, cfg.site_mask, cfg.dropout_p = 2, 1, 0.999
    h = C.c_void_p()
    assert lib.fav_create(C.byref(cfg), C.byref(h)) == 1 and not h.value
    msg = lib.fav_last_error(None)
    assert b"fav_create" in msg and b"dropout_p" in msg and b"256" in msg
    cfg.dropout_p, cfg.device = 0.99, 1 << 20                     # round(253.44) = 253 gets past this check, as far as
    assert lib.fav_create(C.byref(cfg), C.byref(h)) == 5          # the device ordinal nobody has: FAV_ERR_NO_DEVICE
    assert b"dropout_p" not in lib.fav_last_error(None)
