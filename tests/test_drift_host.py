"""CPU-side checks of the window-level drift test: the fav_drift_ref / fav_drift_record layouts (C vs ctypes) and the new
symbols, fav_check_drift_ref (host only) range by range and at the edges of its norm band, fav_drift_workspace_bytes,
DriftReference and build_drift_reference, the record unpacking, and the numpy reference (tests/drift_ref.py) that the GPU file
compares bits with: its identities, its tie rule, and its behaviour as a test - calibrated under exchangeability, and
detecting a clear shift every time."""
import ctypes as C
import fractions
import os
import subprocess

import numpy as np
import pytest

import drift_ref as DR
import knn_ref as K

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


@pytest.fixture(scope="module")
def lib():
    from failure_aware_vision_amd import _lib
    if not os.path.exists(_lib.LIB_PATH):
        import __graft_entry__ as g
        g.build()
    return _lib.load()


_LAYOUT_C = r"""
#include <stddef.h>
#include <stdio.h>
#include "fav.h"
int main(void) {
    printf("ref_size %zu\n", sizeof(fav_drift_ref));
    printf("record_size %zu\n", sizeof(fav_drift_record));
    printf("record_align %zu\n", _Alignof(fav_drift_record));
    printf("config_size %zu\n", sizeof(fav_config));
#define F(x) printf("b.%s %zu\n", #x, offsetof(fav_drift_ref, x));
    F(struct_size) F(D) F(R) F(n_perm) F(rows) F(seed) F(alpha)
#define G(x) printf("r.%s %zu\n", #x, offsetof(fav_drift_record, x));
    G(statistic) G(s_ab) G(s_aa) G(s_bb) G(p_value) G(n_exceed) G(drift) G(n_degenerate)
    printf("abi %d\nkcount %d\n", (int)FAV_ABI_VERSION, (int)FAV_K_COUNT);
    return 0;
}
"""

SYMBOLS = ("fav_check_drift_ref", "fav_set_drift", "fav_classify_drift", "fav_drift_workspace_bytes", "fav_op_drift_test")


def test_layouts_symbols_and_abi(lib, tmp_path):
    from failure_aware_vision_amd import _lib
    src = tmp_path / "layout.c"
    src.write_text(_LAYOUT_C)
    exe = str(tmp_path / "layout")
    subprocess.check_call(["gcc", "-std=c11", "-Wall", "-Werror", "-I" + os.path.join(ROOT, "include"), str(src), "-o", exe])
    out = dict(line.split() for line in subprocess.check_output([exe], text=True).splitlines())
    assert int(out["ref_size"]) == C.sizeof(_lib.FavDriftRef) == 40
    assert int(out["record_size"]) == C.sizeof(_lib.FavDriftRecord) == 48 and int(out["record_align"]) == 8
    for name in ("struct_size", "D", "R", "n_perm", "rows", "seed", "alpha"):
        assert int(out["b." + name]) == getattr(_lib.FavDriftRef, name).offset, name
    for name in ("statistic", "s_ab", "s_aa", "s_bb", "p_value", "n_exceed", "drift", "n_degenerate"):
        assert int(out["r." + name]) == getattr(_lib.FavDriftRecord, name).offset, name
    # what this feature must not move: the ABI version, fav_config, the kernel classes
    assert int(out["abi"]) == 2 == lib.fav_abi_version()
    assert int(out["config_size"]) == C.sizeof(_lib.FavConfig) == 120
    assert int(out["kcount"]) == 6 == _lib.K_COUNT
    header = open(os.path.join(ROOT, "include", "fav.h")).read()
    for sym in SYMBOLS:
        assert sym in _lib._SIGNATURES and hasattr(lib, sym) and sym + "(" in header, sym
        assert getattr(lib, sym).argtypes == _lib._SIGNATURES[sym][1]
    import failure_aware_vision_amd as pkg
    for name in ("DriftReference", "build_drift_reference", "unpack_drift_record"):
        assert hasattr(pkg, name), name
    for name in ("fit_drift", "set_drift", "drift_reference", "classify_drift", "drift_report"):
        assert hasattr(pkg.Backend, name), name


def test_entry_points_refuse_a_null_handle(lib):
    assert lib.fav_set_drift(None, None) == 1
    assert lib.fav_classify_drift(None, None, 2, 0, 0, None, None, None, None, None, None) == 1


# ---- fav_check_drift_ref ----------------------------------------------------------------------------------------------
def unit_rows(rng, R, D):
    x = rng.standard_normal((R, D))
    return K.f32_to_bf16_bits((x / np.linalg.norm(x, axis=1, keepdims=True)).astype(np.float32))


def ref(D=64, R=5, **kw):
    from failure_aware_vision_amd.ood import DriftReference
    return DriftReference(unit_rows(np.random.default_rng(D + R), R, D), **kw)


def refusal(lib, b, D_expected=-1, patch=None):
    c = b.to_c()
    if patch:
        patch(c)
    err = C.create_string_buffer(256)
    st = lib.fav_check_drift_ref(C.byref(c), D_expected, err, len(err))
    return st, err.value.decode()


def test_check_accepts_the_corners(lib):
    for b in (ref(), ref(D=4096, R=2), ref(R=2048, n_perm=9999), ref(n_perm=1), ref(alpha=0.0), ref(alpha=1.0),
              ref(seed=(1 << 64) - 1)):
        assert refusal(lib, b) == (0, "")
        b.check()
    assert refusal(lib, ref(D=128), D_expected=128) == (0, "")
    assert lib.fav_check_drift_ref(C.byref(ref().to_c()), -1, None, 0) == 0          # no message buffer


def test_check_refuses_each_range_and_names_the_field(lib):
    nan = float("nan")
    cases = [(ref(), lambda c: setattr(c, "struct_size", 36), "struct_size=36"),
             (ref(), lambda c: setattr(c, "D", 32), "D=32"), (ref(), lambda c: setattr(c, "D", 96), "D=96"),
             (ref(), lambda c: setattr(c, "D", 4160), "D=4160"), (ref(), lambda c: setattr(c, "D", 0), "D=0"),
             (ref(), lambda c: setattr(c, "R", 1), "R=1"), (ref(), lambda c: setattr(c, "R", 2049), "R=2049"),
             (ref(), lambda c: setattr(c, "n_perm", 0), "n_perm=0"), (ref(), lambda c: setattr(c, "n_perm", 10000), "n_perm=10000"),
             (ref(alpha=-0.001), None, "alpha"), (ref(alpha=1.001), None, "alpha"), (ref(alpha=nan), None, "alpha"),
             (ref(), lambda c: setattr(c, "rows", None), "rows is NULL")]
    for b, patch, text in cases:
        st, msg = refusal(lib, b, patch=patch)
        assert st == 1 and text in msg, (text, msg)
    st, msg = refusal(lib, ref(D=128), D_expected=64)
    assert st == 1 and "D=128" in msg and "64" in msg
    assert lib.fav_check_drift_ref(None, -1, None, 0) == 1
    for bits in (0x7F80, 0xFF80, 0x7FC0, 0x7F81):                                    # +inf, -inf, two NaNs
        b = ref()
        b.rows[3, 7] = bits
        st, msg = refusal(lib, b)
        assert st == 1 and "rows" in msg and "row 3" in msg, (hex(bits), msg)
        with pytest.raises(ValueError, match="rows"):
            b.check()


def test_check_norm_band_at_its_edges(lib):
    """Squared norms of exactly 0.5 and exactly 2 pass; the next bf16 value on the far side of either does not.  Powers of
    two, so the float64 sum is exact."""
    from failure_aware_vision_amd.ood import DriftReference
    bits = lambda v: int(K.f32_to_bf16_bits(np.array([v], np.float32))[0])            # noqa: E731

    def with_row(row):
        rows = unit_rows(np.random.default_rng(1), 4, 64)
        rows[2] = 0
        for j, v in row.items():
            rows[2, j] = v
        return DriftReference(rows)

    half = {0: bits(0.5), 1: bits(0.5)}                                               # 0.25 + 0.25
    two = {0: bits(1.0), 63: bits(-1.0)}                                              # 1 + 1
    assert refusal(lib, with_row(half)) == (0, "") and refusal(lib, with_row(two)) == (0, "")
    below = {0: bits(0.5), 1: bits(0.5) - 1}                                          # one bf16 step less
    above = {0: bits(1.0), 63: bits(-1.0) + 1}
    for row in (below, above, {}):                                                    # and a zero row
        st, msg = refusal(lib, with_row(row))
        assert st == 1 and "norm" in msg and "row 2" in msg and "[0.5, 2]" in msg, msg


def test_workspace_bytes(lib):
    """Host only.  The pool, the similarities of the whole pool and the quantised distances must fit; 0 out of range."""
    f = lib.fav_drift_workspace_bytes
    for n, D, R, P in ((2, 64, 2, 1), (33, 2048, 130, 8), (1024, 4096, 2048, 9999), (70, 256, 300, 64)):
        ld = (R + n + 63) // 64 * 64
        need = ld * D * 2 + 2 * (R + n) * ld * 4 + (R + n) * 8 + (P + 1) * 16
        assert need <= f(n, D, R, P) <= need + 3 * ld * 4 + n * 4 + 10 * 256, (n, D, R, P)
    assert f(1, 64, 2, 1) == f(1025, 64, 2, 1) == f(2, 32, 2, 1) == f(2, 96, 2, 1) == f(2, 4160, 2, 1) == 0
    assert f(2, 64, 1, 1) == f(2, 64, 2049, 1) == f(2, 64, 2, 0) == f(2, 64, 2, 10000) == f(-1, 64, 2, 1) == 0
    assert f(3, 64, 62, 1) > f(2, 64, 62, 1) and f(2, 64, 2, 2000) > f(2, 64, 2, 1)


# ---- the dataclass ------------------------------------------------------------------------------------------------------
def test_reference_round_trip_and_alpha(tmp_path):
    from failure_aware_vision_amd.ood import DriftReference
    b = ref(n_perm=199, alpha=0.05, seed=(1 << 63) + 12345)
    path = str(tmp_path / "ref.npz")
    b.save(path)
    z = DriftReference.load(path)
    assert np.array_equal(z.rows, b.rows) and (z.n_perm, z.alpha, z.seed) == (199, float(np.float32(0.05)), (1 << 63) + 12345)
    c = b.to_c()
    assert (c.D, c.R, c.n_perm, c.seed, c.struct_size) == (64, 5, 199, (1 << 63) + 12345, 40) and c.alpha == np.float32(0.05)
    t = b.with_alpha(0.5)
    assert t.alpha == 0.5 and t.n_perm == 199 and t.seed == b.seed and np.array_equal(t.rows, b.rows)
    d = DriftReference(b.rows)
    assert (d.n_perm, d.alpha, d.seed) == (999, 0.01, 0)
    with pytest.raises(ValueError, match="uint16"):
        DriftReference(np.zeros((3, 64), np.float32))
    with pytest.raises(ValueError, match="matrix"):
        DriftReference(np.zeros(64, np.uint16))
    with pytest.raises(ValueError, match="64-bit"):
        DriftReference(b.rows, seed=-1)


def test_build_agrees_with_the_bank():
    from failure_aware_vision_amd.ood import build_drift_reference, build_knn_bank
    rng = np.random.default_rng(3)
    F = rng.standard_normal((40, 64)) * rng.uniform(1e-3, 1e3, (40, 1))
    a = build_drift_reference(F)
    assert np.array_equal(a.rows, build_knn_bank(F).rows) and (a.R, a.D, a.n_perm, a.alpha, a.seed) == (40, 64, 999, 0.01, 0)
    a.check()
    s = build_drift_reference(F, max_rows=12, seed=5, n_perm=99, alpha=0.05)
    assert np.array_equal(s.rows, build_knn_bank(F, k=3, max_rows=12, seed=5).rows) and (s.R, s.n_perm, s.alpha, s.seed) == (12, 99, 0.05, 5)
    assert build_drift_reference(np.tile(F, (30, 1))).R == 1024                       # the default max_rows
    assert build_drift_reference(np.tile(F, (30, 1)), max_rows=None).R == 1200
    G = F.copy()
    G[4] = 0
    with pytest.raises(ValueError, match="row 4 is zero"):
        build_drift_reference(G)
    G[4, 0] = np.inf
    with pytest.raises(ValueError, match="non-finite"):
        build_drift_reference(G)
    with pytest.raises(ValueError, match="two rows"):
        build_drift_reference(F[:1])
    with pytest.raises(ValueError, match="max_rows"):
        build_drift_reference(F, max_rows=0)


def test_unpack_record():
    from failure_aware_vision_amd.ood import unpack_drift_record
    rec = dict(statistic=np.float64(0.125), s_ab=(1 << 44) + 3, s_aa=5, s_bb=7, p_value=np.float32(0.25), n_exceed=24, drift=0,
               n_degenerate=0)
    out = unpack_drift_record(DR.record_words(rec))
    assert out == dict(statistic=0.125, s_ab=(1 << 44) + 3, s_aa=5, s_bb=7, p_value=0.25, n_exceed=24, drift=False, n_degenerate=0)
    bad = DR.record_words(dict(statistic=np.nan, s_ab=0, s_aa=0, s_bb=0, p_value=np.nan, n_exceed=-1, drift=1, n_degenerate=3))
    assert bad.view(np.uint32).tolist() == [0, 0x7FF80000, 0, 0, 0, 0, 0, 0, 0x7FC00000, 0xFFFFFFFF, 1, 3]
    out = unpack_drift_record(bad.reshape(1, 12))
    assert np.isnan(out["statistic"]) and np.isnan(out["p_value"]) and (out["n_exceed"], out["drift"], out["n_degenerate"]) == (-1, True, 3)
    torch = pytest.importorskip("torch")
    assert unpack_drift_record(torch.from_numpy(bad))["n_degenerate"] == 3
    with pytest.raises(ValueError, match="int32"):
        unpack_drift_record(np.zeros(6, np.int32))


# ---- the reference itself ----------------------------------------------------------------------------------------------
def random_u(rng, Np, top=1 << 22):
    u = np.triu(rng.integers(0, top, (Np, Np)), 1)
    return u + u.T


def test_row_sum_identity_equals_the_direct_sums():
    rng = np.random.default_rng(11)
    for Np, n in ((4, 2), (9, 2), (9, 7), (40, 13), (130, 64)):
        u = random_u(rng, Np)
        for B in (np.arange(Np - n, Np), np.sort(rng.choice(Np, n, replace=False)), np.arange(n)):
            assert DR.sums_by_rows(u, B) == DR.sums_direct(u, B), (Np, n)
    u = np.full((3072, 3072), (1 << 22) - 1, np.int64)                                # the largest sums the contract allows
    np.fill_diagonal(u, 0)
    ab, aa, bb = DR.sums_by_rows(u, np.arange(2048, 3072))
    top = (1 << 22) - 1
    assert (ab, aa, bb) == (2048 * 1024 * top, 2048 * 2047 // 2 * top, 1024 * 1023 // 2 * top) and max(ab, aa, bb) < 1 << 45


def test_integer_comparison_agrees_with_exact_rationals():
    """T is E times R^2 n^2 / 2, exactly: ordering by the 128-bit integer is ordering by the exact energy statistic, where
    float64 would tie or flip."""
    F = fractions.Fraction
    rng = np.random.default_rng(12)

    def E(ab, aa, bb, R, n):
        return F(2 * ab, R * n) - F(2 * aa, R * R) - F(2 * bb, n * n)

    for R, n in ((2, 2), (64, 16), (2048, 1024), (2047, 1023), (130, 33)):
        sums = [tuple(int(v) for v in rng.integers(0, 1 << 45, 3)) for _ in range(50)]
        base = sums[0]
        sums += [(base[0] + 1, base[1], base[2]), (base[0], base[1] + 1, base[2]), (base[0] + n, base[1] + R, base[2])]
        for s in sums:
            assert F(2 * DR.T(*s, R, n), R * R * n * n) == E(*s, R, n)
            assert (DR.T(*s, R, n) >= DR.T(*base, R, n)) == (E(*s, R, n) >= E(*base, R, n))
    assert abs(DR.T((1 << 45) - 1, 0, 0, 2048, 1024)) >= 1 << 64                      # 64 bits do not hold it
    # float64 of step 8 on small exact cases
    assert DR.statistic(0, 0, 0, 5, 3) == 0.0 and not np.signbit(DR.statistic(0, 0, 0, 5, 3))
    assert DR.statistic(6 << 20, 0, 0, 3, 2) == 2.0 and DR.statistic(0, 9 << 20, 4 << 20, 3, 2) == -4.0


def test_group_of_a_permutation_with_ties_in_the_high_word():
    """Keys (high << 32 | index): four indices share the high word that straddles the n-th place; the low word decides."""
    high = [5, 3, 3, 9, 3, 1, 3]
    key_row = np.array([(h << 32) | i for i, h in enumerate(high)], np.uint64)
    assert DR.group_of(key_row, 3).tolist() == [1, 2, 5]                              # 1 first, then two of the four 3s
    assert DR.group_of(key_row, 4).tolist() == [1, 2, 4, 5] and DR.group_of(key_row, 1).tolist() == [5]
    assert DR.group_of(key_row, 5).tolist() == [1, 2, 4, 5, 6] and DR.group_of(key_row, 6).tolist() == [0, 1, 2, 4, 5, 6]
    ks = DR.keys(80, 7, (9 << 32) | 4)
    assert ks.shape == (7, 80) and ks.dtype == np.uint64 and (ks & np.uint64(0xFFFFFFFF) == np.arange(80, dtype=np.uint64)).all()
    from oracle import fav_oracle as O
    assert int(ks[3, 17]) >> 32 == int(O.philox4x32_10(17, 3, 0, 0x5F17, 4, 9)[0])
    assert not np.array_equal(ks >> np.uint64(32), DR.keys(80, 7, 5) >> np.uint64(32))


def test_reference_on_known_answers():
    """One-hot rows: every product is exact.  e_a and e_b are sqrt(2) apart, a row and itself 0."""
    D = 64
    eye = np.eye(D, dtype=np.float32)
    ref_bits = K.f32_to_bf16_bits(np.stack([eye[1], eye[1], eye[1]]))
    step = int(np.rint(np.float32(np.sqrt(np.float32(2.0))) * np.float32(1048576.0)))
    feat = np.stack([3 * eye[1], 0.5 * eye[1]])[None]                                 # the same direction: identical rows
    rec, perm = DR.test(K.f32_to_bf16_bits(feat), ref_bits, 9, 0, 0.5)
    assert (rec["s_ab"], rec["s_aa"], rec["s_bb"], rec["n_exceed"], rec["n_degenerate"]) == (0, 0, 0, 9, 0)
    assert rec["statistic"] == 0.0 and not np.signbit(rec["statistic"]) and rec["p_value"] == 1.0 and rec["drift"] == 0
    assert not perm.any()
    feat = np.stack([eye[2], eye[2]])[None]                                           # a window somewhere else
    rec, perm = DR.test(K.f32_to_bf16_bits(feat), ref_bits, 9, 0, 0.5)
    assert (rec["s_ab"], rec["s_aa"], rec["s_bb"]) == (6 * step, 0, 0)
    assert rec["statistic"] == np.float64(2 * 6 * step) / 6.0 * 2.0 ** -20 and perm.shape == (9, 2)
    # of the C(5, 2) = 10 groupings only the observed one reaches T_obs: n_exceed counts the permutations that drew it
    hits = sum(DR.group_of(k, 2).tolist() == [3, 4] for k in DR.keys(5, 9, 0))
    assert rec["n_exceed"] == hits and rec["p_value"] == np.float32((1 + hits) / 10)
    feat[0, 1, 2] = np.inf
    rec, perm = DR.test(K.f32_to_bf16_bits(feat), ref_bits, 9, 0, 0.5)
    assert perm is None and DR.record_words(rec).view(np.uint32).tolist() == [0, 0x7FF80000, 0, 0, 0, 0, 0, 0, 0x7FC00000,
                                                                             0xFFFFFFFF, 1, 1]


# ---- the test as a test ------------------------------------------------------------------------------------------------
CAL = dict(R=64, n=16, P=99, D=64)


def cluster_rows(rng, count, centres):
    return centres[rng.integers(0, len(centres), count)] + 0.5 * rng.standard_normal((count, centres.shape[1]))


def test_calibration_under_exchangeability():
    """200 windows, each with a reference drawn afresh from the same mixture (seed 1000 + w for the data, w for the
    permutations): at most 20 have p <= 0.05.  A Binomial(200, 0.05) exceeds 20 with probability below 1e-3, so a test that
    is calibrated passes and one that rejects twice as often as it should does not."""
    from failure_aware_vision_amd.ood import build_drift_reference
    centres = np.random.default_rng(99).standard_normal((4, CAL["D"]))
    low = 0
    ps = []
    for w in range(200):
        rng = np.random.default_rng(1000 + w)
        rows = cluster_rows(rng, CAL["R"] + CAL["n"], centres)
        ref_bits = build_drift_reference(rows[:CAL["R"]]).rows
        feat = K.f32_to_bf16_bits(rows[CAL["R"]:].astype(np.float32))[None]
        rec, _ = DR.test(feat, ref_bits, CAL["P"], w, 0.05)
        ps.append(rec["p_value"])
        low += rec["drift"]
    print(f"p <= 0.05 in {low} of 200 exchangeable windows; mean p {np.mean(ps):.3f}")
    assert low == sum(p <= np.float32(0.05) for p in ps) and low <= 20               # p = 5/100 counts: both sides are float32
    assert 0.4 <= np.mean(ps) <= 0.6                                                  # uniform on (0, 1]: mean 0.505, sd 0.02


def test_every_clearly_shifted_window_is_flagged():
    """50 windows moved by 1.5 along one direction, a third of the distance between two centres: p = 1 / 100 every time."""
    from failure_aware_vision_amd.ood import build_drift_reference
    centres = np.random.default_rng(99).standard_normal((4, CAL["D"]))
    shift = np.zeros(CAL["D"])
    shift[:16] = 1.5
    for w in range(50):
        rng = np.random.default_rng(5000 + w)
        rows = cluster_rows(rng, CAL["R"] + CAL["n"], centres)
        ref_bits = build_drift_reference(rows[:CAL["R"]]).rows
        feat = K.f32_to_bf16_bits((rows[CAL["R"]:] + shift).astype(np.float32))[None]
        rec, _ = DR.test(feat, ref_bits, CAL["P"], w, 0.05)
        assert rec["drift"] == 1 and rec["p_value"] <= np.float32(0.05) and rec["statistic"] > 0, (w, rec)
