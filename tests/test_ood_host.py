"""CPU-side checks of the feature-space OOD scoring: the fav_ood_model / fav_ood_record layouts (C vs ctypes) and the new
symbols, fav_check_ood_model (host only) range by range, the float64 fit against the closed-form Mahalanobis distance, the
metrics on hand-made arrays with ties, and the .npz round trip.  The numpy reference (tests/ood_ref.py) that the GPU file
compares bits with is exercised here on cases whose answers are known."""
import ctypes as C
import math
import os
import subprocess

import numpy as np
import pytest

import ood_ref as R

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
    printf("model_size %zu\n", sizeof(fav_ood_model));
    printf("record_size %zu\n", sizeof(fav_ood_record));
    printf("config_size %zu\n", sizeof(fav_config));
#define F(x) printf("m.%s %zu\n", #x, offsetof(fav_ood_model, x));
    F(struct_size) F(D) F(k) F(R) F(mu) F(P) F(M) F(class_id) F(threshold)
#define G(x) printf("r.%s %zu\n", #x, offsetof(fav_ood_record, x));
    G(min_dist) G(min_class) G(label_dist) G(ood)
    printf("abi %d\nkcount %d\nccount %d\n", (int)FAV_ABI_VERSION, (int)FAV_K_COUNT, (int)FAV_C_COUNT);
    return 0;
}
"""

SYMBOLS = ("fav_set_feature_tap", "fav_get_features", "fav_check_ood_model", "fav_set_ood", "fav_classify_ood", "fav_op_ood_score")


def test_layouts_symbols_and_abi(lib, tmp_path):
    from failure_aware_vision_amd import _lib
    src = tmp_path / "layout.c"
    src.write_text(_LAYOUT_C)
    exe = str(tmp_path / "layout")
    subprocess.check_call(["gcc", "-std=c99", "-Wall", "-Werror", "-I" + os.path.join(ROOT, "include"), str(src), "-o", exe])
    out = dict(line.split() for line in subprocess.check_output([exe], text=True).splitlines())
    assert int(out["model_size"]) == C.sizeof(_lib.FavOodModel) == 56
    assert int(out["record_size"]) == C.sizeof(_lib.FavOodRecord) == 16
    for name in ("struct_size", "D", "k", "R", "mu", "P", "M", "class_id", "threshold"):
        assert int(out["m." + name]) == getattr(_lib.FavOodModel, name).offset, name
    for name in ("min_dist", "min_class", "label_dist", "ood"):
        assert int(out["r." + name]) == getattr(_lib.FavOodRecord, name).offset, name
    # what this feature must not move: the ABI version, fav_config, the kernel classes, the corruption kinds
    assert int(out["abi"]) == 2 == lib.fav_abi_version()
    assert int(out["config_size"]) == C.sizeof(_lib.FavConfig) == 120
    assert int(out["kcount"]) == 6 == _lib.K_COUNT and int(out["ccount"]) == 8
    header = open(os.path.join(ROOT, "include", "fav.h")).read()
    for sym in SYMBOLS:
        assert sym in _lib._SIGNATURES and hasattr(lib, sym) and sym + "(" in header, sym
        assert getattr(lib, sym).argtypes == _lib._SIGNATURES[sym][1]


def test_entry_points_refuse_a_null_handle(lib):
    n = C.c_int32(-1)
    assert lib.fav_set_feature_tap(None, 1) == 1
    assert lib.fav_get_features(None, None, C.byref(n), None, None, None) == 1 and n.value == -1
    assert lib.fav_set_ood(None, None) == 1
    assert lib.fav_classify_ood(None, None, 1, 0, 0, None, None, None, None, None, None) == 1


# ---- fav_check_ood_model ----------------------------------------------------------------------------------------------
def model(D=16, k=3, R=2, **kw):
    from failure_aware_vision_amd.ood import OODModel
    rng = np.random.default_rng(5)
    m = dict(mu=rng.standard_normal(D), P=rng.standard_normal((k, D)), M=rng.standard_normal((R, k)),
             class_id=np.arange(R), threshold=math.inf)
    m.update(kw)
    return OODModel(**{f: m[f] for f in ("mu", "P", "M", "class_id", "threshold")})


def check(lib, c, D_expected=-1):
    err = C.create_string_buffer(256)
    st = lib.fav_check_ood_model(C.byref(c) if c is not None else None, D_expected, err, len(err))
    return st, err.value.decode()


def test_check_accepts_the_edges(lib):
    for D, k, R in ((16, 1, 1), (4096, 1, 1), (16, 2048, 1), (16, 1, 4096), (48, 16, 33)):
        assert check(lib, model(D, k, R).to_c()) == (0, ""), (D, k, R)
    assert check(lib, model(threshold=-math.inf).to_c()) == (0, "")
    assert check(lib, model(threshold=0.0).to_c(), 16) == (0, "")
    assert check(lib, model(class_id=np.array([-1, 7])).to_c()) == (0, "")
    model().check(16)                                                              # the Python spelling


def _poke(field, value, where=0):
    m = model()
    arr = getattr(m, field)
    arr.ravel()[where] = value
    return m.to_c()


def _dims(**kw):
    c = model().to_c()
    for f, v in kw.items():
        setattr(c, f, v)
    return c


REFUSED = [
    ("struct_size", lambda: _dims(struct_size=52), "struct_size"),
    ("D 0", lambda: _dims(D=0), "D=0"), ("D 8", lambda: _dims(D=8), "D=8"), ("D 24", lambda: _dims(D=24), "D=24"),
    ("D 4112", lambda: _dims(D=4112), "D=4112"), ("D -16", lambda: _dims(D=-16), "D=-16"),
    ("k 0", lambda: _dims(k=0), "k=0"), ("k 2049", lambda: _dims(k=2049), "k=2049"),
    ("R 0", lambda: _dims(R=0), "R=0"), ("R 4097", lambda: _dims(R=4097), "R=4097"),
    ("mu nan", lambda: _poke("mu", np.nan, 3), "mu"), ("mu inf", lambda: _poke("mu", np.inf, 15), "mu"),
    ("P nan", lambda: _poke("P", np.nan, 47), "P holds"), ("P -inf", lambda: _poke("P", -np.inf), "P holds"),
    ("M nan", lambda: _poke("M", np.nan, 5), "M holds"), ("M inf", lambda: _poke("M", np.inf), "M holds"),
    ("threshold nan", lambda: model(threshold=math.nan).to_c(), "threshold"),
    ("class_id -2", lambda: _poke("class_id", -2, 1), "class_id[1]=-2"),
]


@pytest.mark.parametrize("why,make,text", REFUSED, ids=[r[0] for r in REFUSED])
def test_check_refuses(lib, why, make, text):
    st, msg = check(lib, make())
    assert st == 1 and text in msg, (why, msg)


def test_check_edges(lib):
    assert check(lib, None) == (1, "model is NULL")
    st, msg = check(lib, model().to_c(), 512)
    assert st == 1 and "D=16" in msg and "512" in msg                               # not the arch's feature width
    c = model().to_c()
    c.mu = None
    st, msg = check(lib, c)
    assert st == 1 and "NULL" in msg
    assert lib.fav_check_ood_model(C.byref(_dims(k=0)), -1, None, 0) == 1           # the message is optional
    from failure_aware_vision_amd.ood import OODModel
    with pytest.raises(ValueError, match="threshold is NaN"):
        model(threshold=math.nan).check()                                           # the Python spelling raises the message
    with pytest.raises(ValueError):
        OODModel(np.zeros(16), np.zeros((3, 8)), np.zeros((2, 3)), np.zeros(2))    # P does not fit mu


# ---- the fit against the closed form ----------------------------------------------------------------------------------
@pytest.fixture(scope="module")
def gaussians():
    rng = np.random.default_rng(0)
    D, R, N = 16, 3, 3000
    A = rng.standard_normal((D, D))
    Sigma = A @ A.T / D + 0.1 * np.eye(D)
    L = np.linalg.cholesky(Sigma)
    means = 2 * rng.standard_normal((R, D))
    y = rng.integers(0, R, N)
    F = means[y] + rng.standard_normal((N, D)) @ L.T
    y2 = rng.integers(0, R, 500)
    fresh = means[y2] + rng.standard_normal((500, D)) @ L.T
    return dict(F=F, y=y, fresh=fresh, shifted=fresh + 3 * (L @ np.ones(D)), D=D, R=R)


def test_fit_matches_the_closed_form(gaussians):
    from failure_aware_vision_amd.ood import OODModel, fit_mahalanobis
    G = gaussians
    m = fit_mahalanobis(G["F"], G["y"])
    assert (m.D, m.k, m.R) == (16, 16, 3) and m.class_id.tolist() == [0, 1, 2] and m.threshold == math.inf
    assert m.mu.dtype == m.P.dtype == m.M.dtype == np.float32 and m.class_id.dtype == np.int32
    ref = R.fit64(G["F"], G["y"])
    np.testing.assert_allclose(m.mu, ref["mu"], rtol=1e-6, atol=1e-7)
    # the reference's fp32 chains on fp32 features against (f - mu_c)^T S'^-1 (f - mu_c) in float64 on the same features
    f32 = G["fresh"].astype(np.float32)
    _, d = R.distances(f32[None], m.mu, m.P, m.M)
    exact = R.mahalanobis64(f32, ref["means"], ref["Sigma"])
    rel = np.abs(d - exact) / exact
    print("largest relative error of the reference's distances:", rel.max())
    assert rel.max() < 1e-5
    # the tests' own float64 fit says the same (P is unique up to the sign of a row: compare what it is for)
    _, d_ref = R.distances(f32[None], ref["mu"], ref["P"], ref["M"])
    assert (np.abs(d_ref - exact) / exact).max() < 1e-5
    # separation: the same frames shifted by 3 standard deviations along every whitened axis
    _, d_far = R.distances(G["shifted"].astype(np.float32)[None], m.mu, m.P, m.M)
    near, far = d.min(axis=1), d_far.min(axis=1)
    print("mean min-distance:", near.mean(), "against", far.mean())
    assert OODModel.auroc(near, far) == 1.0 == R.auroc(near, far)
    assert OODModel.fpr_at_tpr(near, far, 0.95) == 0.0


def test_fit_options_and_refusals(gaussians):
    from failure_aware_vision_amd.ood import fit_mahalanobis
    G = gaussians
    m = fit_mahalanobis(G["F"], G["y"] * 5 + 2, k=4, shrinkage=0.0)                   # classes 2, 7, 12; the top 4 directions
    assert (m.k, m.R) == (4, 3) and m.class_id.tolist() == [2, 7, 12]
    ref = R.fit64(G["F"], G["y"] * 5 + 2, k=4, shrinkage=0.0)
    _, d = R.distances(G["fresh"].astype(np.float32)[None], m.mu, m.P, m.M)
    _, d_ref = R.distances(G["fresh"].astype(np.float32)[None], ref["mu"], ref["P"], ref["M"])
    np.testing.assert_allclose(d, d_ref, rtol=1e-4)
    # the rows of P whiten: P S' P^T = I_k
    np.testing.assert_allclose(m.P.astype(np.float64) @ ref["Sigma"] @ m.P.astype(np.float64).T, np.eye(4), atol=1e-5)
    F, y = G["F"][:50], G["y"][:50]
    for bad_F, bad_y in ((F[:1], y[:1]), (np.where(np.arange(16) == 3, np.nan, F), y), (np.where(np.arange(16) == 0, np.inf, F), y),
                         (F, y - 1), (F, y[:-1]), (F, y.astype(np.float64))):
        with pytest.raises(ValueError):
            fit_mahalanobis(bad_F, bad_y)
    for kw in (dict(k=0), dict(k=17), dict(shrinkage=-0.1), dict(shrinkage=1.5)):
        with pytest.raises(ValueError):
            fit_mahalanobis(F, y, **kw)


# ---- the metrics on hand-made arrays ----------------------------------------------------------------------------------
def test_threshold_for_tpr():
    from failure_aware_vision_amd.ood import OODModel
    s = np.array([5.0, 1.0, 3.0, 3.0, 2.0, 9.0, 3.0, 7.0, 4.0, 8.0])                # sorted: 1 2 3 3 3 4 5 7 8 9
    assert OODModel.threshold_for_tpr(s, 1.0) == 9.0
    assert OODModel.threshold_for_tpr(s, 0.9) == 8.0                                # ceil(9) = 9th smallest
    assert OODModel.threshold_for_tpr(s, 0.85) == 8.0                               # ceil(8.5) = 9
    assert OODModel.threshold_for_tpr(s, 0.7) == 5.0                                # 0.7 * 10 is 7.000000000000001 in binary: still the 7th
    assert OODModel.threshold_for_tpr(s, 0.4) == 3.0 == OODModel.threshold_for_tpr(s, 0.3)   # inside the tie
    assert OODModel.threshold_for_tpr(s, 0.05) == 1.0
    for tpr in (0.05, 0.3, 0.4, 0.7, 0.85, 0.9, 1.0):
        assert np.mean(s <= OODModel.threshold_for_tpr(s, tpr)) >= tpr
    for bad in (0.0, -0.1, 1.1):
        with pytest.raises(ValueError):
            OODModel.threshold_for_tpr(s, bad)
    with pytest.raises(ValueError, match="NaN"):
        OODModel.threshold_for_tpr([1.0, np.nan], 0.5)
    with pytest.raises(ValueError, match="empty"):
        OODModel.threshold_for_tpr([], 0.5)


def test_auroc_and_fpr_with_ties():
    from failure_aware_vision_amd.ood import OODModel
    assert OODModel.auroc([1, 2, 3], [4, 5]) == 1.0 and OODModel.auroc([4, 5], [1, 2, 3]) == 0.0
    assert OODModel.auroc([1, 1, 1], [1, 1]) == 0.5
    # id 1 2 2 3 against ood 2 3 4: above 1 + 1 + 3 + 4 = 9 ... pair by pair: (2: >1, =2, =2, <3) (3: >1 >2 >2 =3) (4: all)
    want = ((1 + 0.5 + 0.5 + 0) + (3 + 0.5) + 4) / 12
    assert OODModel.auroc([1, 2, 2, 3], [2, 3, 4]) == want == R.auroc([1, 2, 2, 3], [2, 3, 4])
    rng = np.random.default_rng(2)
    a, b = rng.integers(0, 6, 40).astype(np.float64), rng.integers(2, 9, 31).astype(np.float64)
    assert abs(OODModel.auroc(a, b) - R.auroc(a, b)) < 1e-15
    assert math.isinf(OODModel.threshold_for_tpr([1.0, math.inf], 1.0)) and OODModel.auroc([1, math.inf], [math.inf]) == 0.75
    # threshold at tpr 0.75 of 1 2 2 3 is the 3rd smallest, 2: the OOD scores 2 pass, 3 and 4 do not
    assert OODModel.fpr_at_tpr([1, 2, 2, 3], [2, 3, 4], 0.75) == 1 / 3
    assert OODModel.fpr_at_tpr([1, 2, 2, 3], [2, 3, 4], 1.0) == 2 / 3
    assert OODModel.fpr_at_tpr([1, 2, 3], [4, 5]) == 0.0
    with pytest.raises(ValueError):
        OODModel.auroc([1.0], [np.nan])


def test_separation_report_on_hand_made_scores():
    from failure_aware_vision_amd.ood import OODModel, separation_report
    a, b = [0, 1, 1, 2, 5], [1, 3, 5, 6]
    # above + half the ties, OOD score by OOD score: 1: 1 + 2/2; 3: 4; 5: 4 + 1/2; 6: 5
    rep = separation_report(a, b, 2)
    assert rep["auroc"] == 15.5 / 20 and rep["fpr_at_tpr95"] == OODModel.fpr_at_tpr(a, b) == 0.75   # the 5th smallest, 5: 1, 3, 5 pass
    assert rep["id_flagged"] == 0.2 and rep["ood_flagged"] == 0.75 and (rep["n_id"], rep["n_ood"]) == (5, 4)
    assert rep["id_mean_dist"] == 1.8 and rep["ood_mean_dist"] == 3.75 and rep["threshold"] == 2
    assert set(rep) == {"auroc", "fpr_at_tpr95", "id_mean_dist", "ood_mean_dist", "threshold", "id_flagged", "ood_flagged",
                        "n_id", "n_ood"}
    assert separation_report(a, b, math.inf)["ood_flagged"] == 0.0 and separation_report(a, b, -1.0)["id_flagged"] == 1.0


def test_module_level_metrics_are_the_static_methods():
    from failure_aware_vision_amd import ood
    rng = np.random.default_rng(5)
    for _ in range(20):
        a, b = rng.integers(0, 6, 40).astype(np.float64), rng.integers(2, 9, 31).astype(np.float32)   # ties within and across
        assert ood.auroc(a, b) == ood.OODModel.auroc(a, b) == R.auroc(a, b)
        for tpr in (0.05, 0.5, 0.95, 1.0):
            assert ood.threshold_for_tpr(a, tpr) == ood.OODModel.threshold_for_tpr(a, tpr)
            assert ood.fpr_at_tpr(a, b, tpr) == ood.OODModel.fpr_at_tpr(a, b, tpr)
    m = model(16, 2, 3)
    assert m.threshold_for_tpr([3.0, 1.0, 2.0], 0.5) == 2.0                         # on an instance, as Backend.calibrate_ood did
    for fn in (ood.auroc, ood.OODModel.auroc, ood.fpr_at_tpr, ood.OODModel.fpr_at_tpr,
               lambda x, y: ood.separation_report(x, y, 1.0)):
        with pytest.raises(ValueError, match="id_scores is empty"):
            fn([], [1.0])
        with pytest.raises(ValueError, match="ood_scores is empty"):
            fn([1.0], [])
        with pytest.raises(ValueError, match="id_scores holds a NaN"):
            fn([1.0, np.nan], [1.0])
        with pytest.raises(ValueError, match="ood_scores holds a NaN"):
            fn([1.0], [np.nan, 2.0])
    for fn in (ood.threshold_for_tpr, ood.OODModel.threshold_for_tpr):
        with pytest.raises(ValueError, match="id_scores is empty"):
            fn([], 0.5)
        with pytest.raises(ValueError, match="id_scores holds a NaN"):
            fn([np.nan], 0.5)


def test_npz_round_trip_and_records(tmp_path):
    from failure_aware_vision_amd.ood import OODModel, unpack_records
    m = model(48, 5, 7, threshold=12.5, class_id=np.array([3, 3, -1, 0, 9, 2, 2]))
    path = tmp_path / "model.npz"
    m.save(path)
    back = OODModel.load(path)
    for f in ("mu", "P", "M", "class_id"):
        a, b = getattr(m, f), getattr(back, f)
        assert a.dtype == b.dtype and np.array_equal(a, b), f
    assert back.threshold == 12.5 and (back.D, back.k, back.R) == (48, 5, 7)
    m.with_threshold(math.inf).save(path)
    assert OODModel.load(path).threshold == math.inf
    c = back.to_c()
    assert (c.struct_size, c.D, c.k, c.R) == (56, 48, 5, 7) and c.P[47] == back.P[0, 47] and c.class_id[2] == -1
    rec = np.zeros((2, 4), np.int32)
    rec[:, 0] = np.array([1.5, np.inf], np.float32).view(np.int32)
    rec[:, 1] = (4, -1)
    rec[:, 2] = np.array([2.5, np.nan], np.float32).view(np.int32)
    rec[:, 3] = (0, 1)
    u = unpack_records(rec)
    assert u["min_dist"].tolist() == [1.5, math.inf] and u["nearest_class"].tolist() == [4, -1] and u["ood"].tolist() == [0, 1]
    assert u["label_dist"][0] == 2.5 and math.isnan(u["label_dist"][1])
    with pytest.raises(ValueError):
        unpack_records(np.zeros((2, 5), np.int32))


# ---- the reference on cases with known answers ------------------------------------------------------------------------
def test_reference_known_answers():
    # D = 16, identity-like projection onto the first two axes; means at (0, 0), (3, 4), (3, 4) again, and (1, 0)
    P = np.zeros((2, 16), np.float32)
    P[0, 0] = P[1, 1] = 1
    M = np.array([[0, 0], [3, 4], [3, 4], [1, 0]], np.float32)
    cls = np.array([5, 9, 9, -1], np.int32)
    feat = np.zeros((2, 3, 16), np.float32)
    feat[:, 0, :2] = [[3, 4], [3, 4]]                                               # on rows 1 and 2: the lower one wins
    feat[:, 1, :2] = [[0, 0], [1, 0]]                                               # mean (0.5, 0): rows 0 and 3 tie at 0.25
    feat[0, 2, 0] = np.nan                                                          # a NaN never wins: row -1
    out = R.score(R.f32_to_bf16_bits(feat), np.zeros(16, np.float32), P, M, cls, np.array([9, 7, 5]), 0.25)
    assert out["min_dist"].tolist() == [0.0, 0.25, math.inf] and out["min_class"].tolist() == [9, 5, -1]
    assert out["label_dist"][0] == 0.0 and math.isnan(out["label_dist"][1]) and math.isnan(out["label_dist"][2])
    assert out["ood"].tolist() == [0, 0, 1]                                         # 0.25 <= 0.25 passes
    assert R.score(R.f32_to_bf16_bits(feat), np.zeros(16, np.float32), P, M, cls, None, -math.inf)["ood"].tolist() == [1, 1, 1]
    rec = R.records(out)
    assert rec.shape == (3, 4) and rec.dtype == np.int32 and np.array_equal(rec, R.canon_records(rec))
    x = np.array([1.0, -2.5, 65280.0, -0.0, math.inf], np.float32)                # bf16 values survive the round trip
    assert np.array_equal(R.bf16_to_f32(R.f32_to_bf16_bits(x)).view(np.uint32), x.view(np.uint32))
    assert R.bf16_to_f32(R.f32_to_bf16_bits(np.array([1.00390625], np.float32)))[0] == 1.0   # a tie rounds to even
