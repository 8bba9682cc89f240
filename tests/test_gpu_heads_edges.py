"""The four confidence heads at their edges, on the GPU: fav_op_head, fav_op_head_uncertainty, fav_op_head_sets (LAC, APS,
RAPS) and fav_op_head_sweep against the one float64 reference tests/heads_ref.py, on the inputs that module builds
(tests/test_heads_ref_host.py checks the reference, the closed forms and the caps on the same inputs without a GPU).

For every case: (a) each head against heads_ref; (b) label, confidence, fail and score bit-identical across the four heads
(the sweep at its temperature; kind 2 only where T >= 2 and C >= 2); (c) every output buffer is prefilled with a pattern
and carries guard rows, and nothing outside the frames' slots is written.  The logits' padding columns hold NaN: the
heads must never read them.

Tolerances, fp32 device arithmetic against float64 that shares the contract's two roundings (inv_temp, z): probabilities
2e-6, entropies and mutual information 2e-5, prob_std 1e-5 (test_gpu_uncertainty.py), conformal scores 1e-5 and set mass
2e-5 (test_gpu_conformal.py), nll / brier 9e-6 on |dev - ref| / max(1, |ref|) (test_gpu_calibration.py).  A confidence of
kind 1 / 2 is 1 - H / ln K, so its bound is the entropy's divided by ln K where ln K < 1 (K = 2: 2.9e-5).  On saturated and
flat rows the bounds tighten to the exact values of the closed forms.  Labels, top-5 and fail are compared under the
filters of heads_ref.py on the random cases and without any on the constructed ones.  Every case prints a MEASURED line
with its largest errors before it asserts.

MEASURED on an MI355X, the largest error over all cases of this module (case), against the bound - none was widened:
  probabilities 2.0e-7 (T = 4096, C = 10) / 2e-6;  entropies and MI 1.4e-6 (temperature 1e4, C = 1000) / 2e-5;
  prob_std 5.8e-8 / 1e-5;  confidence kind 0 / 1 / 2: 2.0e-7 / 2.2e-7 / 1.3e-6;  nll 5.6e-7 (T = 4096) and brier 2.5e-7 / 9e-6;
  conformal score 8.1e-6 (flat row, C = 1000: a running fp32 sum of 999 terms of 1e-3, format estimate 999 x 2^-24 x 0.5 =
  3e-5) / 1e-5;  set mass 2.4e-7 / 2e-5;  agreement, and every closed form of the saturated rows, exact.
T = 4096 (1024 sequential additions per wave) and |z| of a few thousand needed no extra room."""
import ctypes as C
import math

import numpy as np
import pytest

pytestmark = pytest.mark.gpu

torch = pytest.importorskip("torch")
from failure_aware_vision_amd import Backend, _lib, synth, weights  # noqa: E402
from failure_aware_vision_amd.calibration import fit_temperature, unpack_cells  # noqa: E402
from failure_aware_vision_amd.conformal import Conformal, unpack_sets  # noqa: E402
import heads_ref as H  # noqa: E402

GUARD = 2                       # guard rows before and after every output buffer
PAT32, PAT8 = 0x5A5A5A5A, 0xA5


@pytest.fixture(scope="module")
def lib():
    assert torch.cuda.is_available(), "GPU tests need a MI355X"
    return _lib.load()


class Out:
    """A device output buffer of n rows with GUARD rows of pattern on either side; ptr addresses row 0 of the payload."""
    def __init__(self, n, width=1, dtype=torch.int32):
        self.n, self.pat = n, PAT8 if dtype == torch.uint8 else PAT32
        self.t = torch.full((n + 2 * GUARD, width), self.pat, dtype=dtype, device="cuda")
        self.ptr = self.t[GUARD:].data_ptr()

    def get(self, written=True):
        a = self.t.cpu().numpy()
        assert np.all(a[:GUARD] == self.pat) and np.all(a[GUARD + self.n:] == self.pat), "a guard row was written"
        a = a[GUARD:GUARD + self.n]
        if written:
            assert not np.any(a == self.pat), "a slot was left unwritten"
        return a[:, 0] if a.shape[1] == 1 else a


def f32(a):
    return np.ascontiguousarray(a).view(np.float32)


def dev_logits(lg, extra=0):
    """[T, n, C] -> device [T, n, ld], ld = C rounded up to 4 plus extra, NaN in the padding columns."""
    T, n, Cc = lg.shape
    ld = (Cc + 3) // 4 * 4 + extra
    full = np.full((T, n, ld), np.nan, np.float32)
    full[:, :, :Cc] = lg
    return torch.from_numpy(full).cuda(), ld


def op_head(lib, d, T, n, Cc, ld, temp, kind, tau):
    lab, conf, fail, score = Out(n), Out(n), Out(n, dtype=torch.uint8), Out(n)
    _lib.check(lib.fav_op_head(d.data_ptr(), T, n, Cc, ld, temp, kind, tau, lab.ptr, conf.ptr, fail.ptr, score.ptr, None))
    torch.cuda.synchronize()
    return dict(label=lab.get(), confidence=f32(conf.get()), fail=fail.get(), score=f32(score.get()))


def op_unc(lib, d, T, n, Cc, ld, temp, kind, tau):
    rec, fail, score = Out(n, 18), Out(n, dtype=torch.uint8), Out(n)
    _lib.check(lib.fav_op_head_uncertainty(d.data_ptr(), T, n, Cc, ld, temp, kind, tau, rec.ptr, fail.ptr, score.ptr, None))
    torch.cuda.synchronize()
    r = rec.get()
    out = dict(label=r[:, 0], top_label=r[:, 8:13], top_prob=f32(r[:, 13:18]), fail=fail.get(), score=f32(score.get()))
    for i, k in enumerate(H.REC_FLOATS, start=1):
        out[k] = f32(r[:, i])
    return out


def op_sets(lib, d, T, n, Cc, ld, temp, kind, tau, y, score_kind="aps", qhat=math.inf, lam=0.0, k_reg=0, randomized=False, seed=0,
            first_index=0):
    cp = Conformal(kind=score_kind, randomized=randomized, lam=lam, k_reg=k_reg, qhat=qhat, seed=seed)
    rec, ts, fail, score = Out(n, 40), Out(n), Out(n, dtype=torch.uint8), Out(n)
    lab = torch.from_numpy(np.asarray(y, np.int32)).cuda()
    _lib.check(lib.fav_op_head_sets(d.data_ptr(), T, n, Cc, ld, temp, kind, tau, first_index, cp.to_c(), lab.data_ptr(), ts.ptr,
                                    rec.ptr, fail.ptr, score.ptr, None))
    torch.cuda.synchronize()
    r = rec.get()
    words = r[:, 8:40].view(np.uint32)
    bits = ((words[:, :, None] >> np.arange(32, dtype=np.uint32)) & 1).reshape(n, 1024).astype(bool)
    assert not bits[:, Cc:].any(), "a membership bit at or above num_classes"
    assert np.all(r[:, 5:8] == 0)
    out = dict(unpack_sets(r, Cc), fail=fail.get(), score=f32(score.get()), true_scores=f32(ts.get()))
    assert np.array_equal(out["members"], bits[:, :Cc])
    return out


def op_sweep(lib, d, T, n, Cc, ld, temps, kind, y):
    t = np.ascontiguousarray(np.asarray(temps, np.float32))
    cells = Out(n, 4 * t.size)
    lab = torch.from_numpy(np.asarray(y, np.int32)).cuda()
    _lib.check(lib.fav_op_head_sweep(d.data_ptr(), T, n, Cc, ld, t.ctypes.data_as(C.POINTER(C.c_float)), t.size, kind,
                                     lab.data_ptr(), cells.ptr, None))
    torch.cuda.synchronize()
    raw = np.ascontiguousarray(cells.get()).reshape(n, t.size, 4)
    return dict(unpack_cells(raw), raw=raw)


def kinds_of(T, Cc):
    return (0, 1, 2) if T >= 2 and Cc >= 2 else (0, 1)


def conf_tol(kind, T, Cc):
    if kind == 0:
        return H.PROB_TOL
    K = Cc if kind == 1 else min(Cc, T)
    return H.ENT_TOL / min(1.0, math.log(K)) if K > 1 else 0.0


class Errors(dict):
    def add(self, name, dev, ref, measure=None):
        dev, ref = np.asarray(dev, np.float64), np.asarray(ref, np.float64)
        assert np.array_equal(np.isnan(dev), np.isnan(ref)), (name, dev, ref)
        ok = ~np.isnan(ref)
        e = (np.abs(dev - ref) if measure is None else measure(dev, ref))[ok]
        e = float(e.max()) if e.size else 0.0
        self[name] = max(self.get(name, 0.0), e)
        return e


BITS = ("label", "confidence", "fail", "score")


def same_bits(a, b, what):
    for k in BITS:
        x, y = np.ascontiguousarray(a[k]), np.ascontiguousarray(b[k])
        assert np.array_equal(x.view(np.uint8), y.view(np.uint8)), (what, k, x, y)


def check_core(got, r, kind, T, Cc, tau, random, err):
    """label / confidence / fail / score of any head against the reference."""
    ok = r["label_ok"] if random else np.ones(len(r["label"]), bool)
    assert np.array_equal(got["label"][ok], r["label"][ok]), (got["label"], r["label"])
    tol = conf_tol(kind, T, Cc)
    assert err.add(f"conf{kind}", got["confidence"], r["confidence"]) <= tol
    assert err.add(f"conf{kind}", got["score"], r["score"]) <= tol
    fok = r["fail_ok"] if random else np.ones(len(r["label"]), bool)
    assert np.array_equal(got["fail"][fok], r["fail"][fok])
    assert np.array_equal(got["fail"], ((got["confidence"] < np.float32(tau)) | r["nonfinite"]).astype(np.uint8))
    assert np.all((got["score"] >= 0) & (got["score"] <= 1))
    neg = got["confidence"] < 0                                     # a flat row's entropy confidence may round below 0
    assert np.all(got["score"][neg] == 1.0)


def check_unc(got, r, random, err):
    n = len(r["label"])
    ok = r["label_ok"] if random else np.ones(n, bool)
    ok5 = r["top_ok"] if random else np.ones(n, bool)
    assert np.array_equal(got["top_label"][ok5], r["top_label"][ok5]), (got["top_label"], r["top_label"])
    assert np.array_equal(got["top_label"] < 0, r["top_label"] < 0)
    err.add("agreement", got["agreement"][ok], r["agreement"][ok].astype(np.float32))
    assert err["agreement"] == 0.0
    assert err.add("prob", got["mean_prob"], r["mean_prob"]) <= H.PROB_TOL
    assert err.add("prob", got["top_prob"], r["top_prob"]) <= H.PROB_TOL
    # prob_std follows the device's label: where a near-tie lets it differ, the reference's std is another class's
    assert err.add("prob_std", got["prob_std"][ok], r["prob_std"][ok]) <= H.STD_TOL
    for k in ("pred_entropy", "expected_entropy", "mutual_info"):
        assert err.add("entropy", got[k], r[k]) <= H.ENT_TOL, k
    fin = ~r["nonfinite"]
    assert np.all(got["mutual_info"][fin] >= 0) and np.all(np.diff(got["top_prob"], axis=1) <= 0)


def check_sets(got, r, kw, y, random, err):
    s = H.sets_ref(r, true_labels=y, **kw)
    n, Cc = r["pbar"].shape
    cmp = H.members_comparable(r, s["s"], kw["qhat"])
    st = H.rank_stable(r, y)
    if not random:                                                  # a constructed case: every class and every frame is compared
        assert cmp.all() and st.all()
    assert np.array_equal(got["members"][cmp], s["members"][cmp]), np.argwhere(got["members"] != s["members"])[:8]
    assert np.array_equal(got["members"].sum(axis=1), got["set_size"])
    assert np.array_equal(np.isnan(got["true_scores"]), np.isnan(s["true_scores"]))
    assert err.add("cp_score", got["true_scores"][st], s["true_scores"][st]) <= H.SCORE_TOL
    mass = np.where(got["members"], np.nan_to_num(r["pbar"]), 0.0).sum(axis=1)
    assert err.add("set_mass", got["set_mass"], mass) <= H.MASS_TOL
    assert np.array_equal(got["u"], s["u"].astype(np.float32))
    fin = ~r["nonfinite"]
    assert np.all(got["set_size"][~fin] == 0) and np.all(got["set_mass"][~fin] == 0)
    if kw["qhat"] == math.inf:
        assert np.all(got["set_size"][fin] == Cc)
    if kw["qhat"] < 0:
        assert np.all(got["set_size"] == 0)


def check_sweep_cells(w, k, r, err):
    assert err.add("nll", w["nll"][:, k], r["nll"], H.error_measure) <= H.NLL_TOL
    assert err.add("brier", w["brier"][:, k], r["brier"], H.error_measure) <= H.NLL_TOL


def run_case(lib, case, extra=0, sweep_all_kinds=False):
    lg, temp, tau, y, random = case["logits"], case["temperature"], case["tau"], case["labels"], case["random"]
    T, n, Cc = lg.shape
    d, ld = dev_logits(lg, extra)
    err = Errors()
    outs = {}
    for kind in kinds_of(T, Cc):
        r = H.heads_ref(lg, temp, kind, tau, true_labels=y)
        h = op_head(lib, d, T, n, Cc, ld, temp, kind, tau)
        u = op_unc(lib, d, T, n, Cc, ld, temp, kind, tau)
        s = op_sets(lib, d, T, n, Cc, ld, temp, kind, tau, y, **H.sets_configs(Cc)[1])
        w = op_sweep(lib, d, T, n, Cc, ld, [temp], kind, y)
        same_bits(u, h, "uncertainty head")
        same_bits(s, h, "sets head")
        assert np.array_equal(w["label"][:, 0], h["label"]), "sweep head label"
        assert np.array_equal(w["confidence"][:, 0].view(np.int32), h["confidence"].view(np.int32)), "sweep head confidence"
        check_core(h, r, kind, T, Cc, tau, random, err)
        check_unc(u, r, random, err)
        check_sweep_cells(w, 0, r, err)
        if kind == 0:
            assert np.array_equal(u["mean_prob"].view(np.int32)[~r["nonfinite"]], h["confidence"].view(np.int32)[~r["nonfinite"]])
            for kw in H.sets_configs(Cc):
                check_sets(op_sets(lib, d, T, n, Cc, ld, temp, 0, tau, y, **kw), r, kw, y, random, err)
        outs[kind] = dict(head=h, unc=u, sets=s, sweep=w, ref=r)
    # the sweep head at K = 5 temperatures (a group of 4 and a group of 1): K single launches, and the plain heads
    for kind in kinds_of(T, Cc) if sweep_all_kinds else (0,):
        five = op_sweep(lib, d, T, n, Cc, ld, H.SWEEP_FIVE, kind, y)
        for k, t in enumerate(H.SWEEP_FIVE):
            one = op_sweep(lib, d, T, n, Cc, ld, [t], kind, y)
            assert np.array_equal(five["raw"][:, k], one["raw"][:, 0]), (kind, k)
            h = op_head(lib, d, T, n, Cc, ld, float(t), kind, tau)
            assert np.array_equal(five["label"][:, k], h["label"]), (kind, k)
            assert np.array_equal(five["confidence"][:, k].view(np.int32), h["confidence"].view(np.int32)), (kind, k)
            check_sweep_cells(five, k, H.heads_ref(lg, float(t), kind, tau, true_labels=y), err)
    print(f"MEASURED {case['name']} ld {ld}: " + " ".join(f"{k} {v:.3e}" for k, v in sorted(err.items())))
    return outs


def named(cases):
    return [pytest.param(c, id=c["name"]) for c in cases]


@pytest.mark.parametrize("extra", [0, 64])
@pytest.mark.parametrize("case", named(H.class_count_cases()))
def test_class_counts(lib, case, extra):
    outs = run_case(lib, case, extra)
    T, n, Cc = case["logits"].shape
    u = outs[0]["unc"]
    k = min(5, Cc)
    assert np.all(u["top_label"][:, k:] == -1) and np.all(u["top_prob"][:, k:] == 0)     # the slots past C hold (-1, 0)
    if Cc == 1:
        for kind in (0, 1):
            o = outs[kind]
            assert np.all(o["head"]["label"] == 0) and np.all(o["head"]["confidence"] == 1.0)
            assert np.all(o["unc"]["mean_prob"] == 1.0)
            assert np.array_equal(o["unc"]["top_label"], np.tile([0, -1, -1, -1, -1], (n, 1)))


@pytest.mark.parametrize("case", named(H.sample_count_cases()))
def test_sample_counts(lib, case):
    run_case(lib, case, sweep_all_kinds=True)


def test_uncertainty_head_rejects_4097_samples(lib):
    d = torch.zeros((4097, 1, 12), dtype=torch.float32, device="cuda")
    rec = Out(1, 18)
    assert lib.fav_op_head_uncertainty(d.data_ptr(), 4097, 1, 10, 12, 1.0, 0, 0.5, rec.ptr, None, None, None) == 1
    rec.get(written=False)
    assert np.all(rec.t.cpu().numpy() == PAT32)


@pytest.mark.parametrize("case", named(H.sweep_staging_cases()))
def test_sweep_staging_boundary(lib, case):
    run_case(lib, case, sweep_all_kinds=True)


@pytest.mark.parametrize("case", named(H.temperature_cases()))
def test_temperatures(lib, case):
    run_case(lib, case)


@pytest.mark.parametrize("case", named(H.saturated_cases()))
def test_saturated_rows_are_exact(lib, case):
    outs = run_case(lib, case)
    lg = case["logits"]
    T, n, Cc = lg.shape
    d, ld = dev_logits(lg)
    win, y = case["winner"], case["labels"]
    if "agree" in case["name"]:
        for kind, o in outs.items():
            for head in ("head", "unc", "sets"):
                g = o[head]
                assert np.array_equal(g["label"], win) and np.all(g["confidence"] == 1.0) and np.all(g["score"] == 0.0), (kind, head)
                assert np.all(g["fail"] == 0)
            u = o["unc"]
            for k in ("pred_entropy", "expected_entropy", "mutual_info", "prob_std"):
                assert np.all(u[k] == 0.0), k
            assert np.all(u["agreement"] == 1.0) and np.all(u["mean_prob"] == 1.0)
            assert np.array_equal(u["top_prob"], np.tile([1.0, 0, 0, 0, 0], (n, 1)).astype(np.float32))
            right = y == win
            w = o["sweep"]
            assert np.all(w["nll"][right, 0] == 0.0) and np.all(w["brier"][right, 0] == 0.0)
            # -logf(FLT_MIN) = 87.3365..: within one fp32 ulp (7.6e-6) of the float64 value, whatever logf rounds to
            assert np.all(np.abs(w["nll"][~right, 0].astype(np.float64) + math.log(H.FLT_MIN)) <= 7.7e-6) and np.all(w["brier"][~right, 0] == 2.0)
        # LAC: score 0 for the winner, 1 for the rest.  APS: u for the winner, 1 for the rest - the winner alone for u <= qhat < 1
        args = (lib, d, T, n, Cc, ld, case["temperature"], 0, case["tau"])
        assert np.all(op_sets(*args, win, score_kind="lac", qhat=0.5)["true_scores"] == 0.0)
        assert np.all(op_sets(*args, (win + 1) % Cc, score_kind="lac", qhat=0.5)["true_scores"] == 1.0)
        onehot = np.zeros((n, Cc), bool)
        onehot[np.arange(n), win] = True
        for qhat in (0.0, 0.5, float(np.nextafter(np.float32(1), np.float32(0)))):
            assert np.array_equal(op_sets(*args, win, score_kind="lac", qhat=qhat)["members"], onehot)
            g = op_sets(*args, win, score_kind="aps", qhat=qhat, randomized=True, seed=5)
            assert np.array_equal(g["true_scores"], g["u"])
            assert np.array_equal(g["members"], onehot & (g["u"] <= np.float32(qhat))[:, None])
            g = op_sets(*args, win, score_kind="aps", qhat=qhat)
            assert np.all(g["true_scores"] == 1.0) and not g["members"].any()           # u = 1: s(winner) = 1 > qhat
            assert np.all(op_sets(*args, (win + 1) % Cc, score_kind="aps", qhat=qhat, randomized=True, seed=5)["true_scores"] == 1.0)
    else:
        other = case["other"]
        for kind, o in outs.items():
            for head in ("head", "unc", "sets"):
                assert np.array_equal(o[head]["label"], win), (kind, head)
        u = outs[0]["unc"]
        assert np.all(u["mean_prob"] == 0.5) and np.all(u["agreement"] == 0.5) and np.all(u["prob_std"] == 0.5)
        assert np.all(u["expected_entropy"] == 0.0)
        for i in range(n):
            rest = [k for k in range(Cc) if k not in (win[i], other[i])][:3]
            assert u["top_label"][i].tolist() == [win[i], other[i]] + rest
        assert np.array_equal(u["top_prob"], np.tile([0.5, 0.5, 0, 0, 0], (n, 1)).astype(np.float32))
        # the sort order: rank 1 is the higher index of the tie (A = 0.5), then every other class by index (A = 1)
        args = (lib, d, T, n, Cc, ld, case["temperature"], 0, case["tau"])
        assert np.all(op_sets(*args, win, score_kind="aps", qhat=0.6)["true_scores"] == 0.5)
        g = op_sets(*args, other, score_kind="aps", qhat=0.6, lam=1.0, k_reg=0)       # score = u p + A + (rank + 1)
        assert np.all(g["true_scores"] == 3.0)
        third = np.array([[k for k in range(Cc) if k not in (win[i], other[i])][0] for i in range(n)])
        assert np.all(op_sets(*args, third, score_kind="aps", qhat=0.6, lam=1.0, k_reg=0)["true_scores"] == 4.0)
        last = np.array([[k for k in range(Cc) if k not in (win[i], other[i])][-1] for i in range(n)])
        assert np.all(op_sets(*args, last, score_kind="aps", qhat=0.6, lam=1.0, k_reg=0)["true_scores"] == 1.0 + Cc)


@pytest.mark.parametrize("case", named(H.flat_cases()))
def test_flat_rows(lib, case):
    outs = run_case(lib, case)
    lg = case["logits"]
    T, n, Cc = lg.shape
    for kind, o in outs.items():
        for head in ("head", "unc", "sets"):
            assert np.all(o[head]["label"] == 0), (kind, head)
    u = outs[1]["unc"]
    assert np.array_equal(u["top_label"], np.tile(np.arange(5), (n, 1)))
    assert np.all(np.abs(u["mean_prob"].astype(np.float64) - 1.0 / Cc) <= H.PROB_TOL) and np.all(u["top_prob"] == u["top_prob"][:, :1])
    assert np.all(np.abs(u["pred_entropy"].astype(np.float64) - math.log(Cc)) <= H.ENT_TOL)
    assert np.all(np.abs(u["confidence"]) <= H.ENT_TOL) and np.all(u["agreement"] == 1.0)
    if Cc in (10, 257):
        # APS scores by class: one launch per class as the 'true' label; non-decreasing in class index
        d, ld = dev_logits(lg)
        sc = np.stack([op_sets(lib, d, T, n, Cc, ld, case["temperature"], 0, case["tau"], np.full(n, c, np.int32), score_kind="aps",
                               qhat=0.5)["true_scores"] for c in range(Cc)], axis=1)
        assert np.all(np.diff(sc, axis=1) >= 0)
        assert np.all(np.abs(sc[:, -1].astype(np.float64) - 1.0) <= H.MASS_TOL)
    if Cc == 1000:
        # the 1024-wide sort: classes either side of its 256 / 512 / 768 exchanges
        d, ld = dev_logits(lg)
        picks = [0, 1, 254, 255, 256, 257, 510, 511, 512, 513, 766, 767, 768, 769, 998, 999]
        sc = np.stack([op_sets(lib, d, T, n, Cc, ld, case["temperature"], 0, case["tau"], np.full(n, c, np.int32), score_kind="aps",
                               qhat=0.5)["true_scores"] for c in picks], axis=1)
        assert np.all(np.diff(sc, axis=1) > 0)
        assert np.all(np.abs(sc.astype(np.float64) - (np.array(picks) + 1) / 1000.0) <= H.SCORE_TOL)


@pytest.mark.parametrize("case", named(H.masked_cases()))
def test_masked_classes(lib, case):
    outs = run_case(lib, case)
    if "mask" not in case:
        return                                                      # -inf in some samples only: finite behaviour, checked above
    lg, mask = case["logits"], case["mask"]
    T, n, Cc = lg.shape
    live, dead = np.flatnonzero(~mask), np.flatnonzero(mask)
    d, ld = dev_logits(lg)
    args = (lib, d, T, n, Cc, ld, case["temperature"], 0, case["tau"])
    for kind, o in outs.items():
        for head in ("head", "unc", "sets"):
            assert not mask[o[head]["label"]].any(), (kind, head)
        # the other outputs equal those of the same logits with the masked classes removed
        small = H.heads_ref(lg[:, :, live], case["temperature"], kind, case["tau"])
        assert np.array_equal(o["head"]["label"], live[small["label"]])
        # kind 1 divides by ln C of the full class count: recomputed from the compacted entropy
        want = 1.0 - small["pred_entropy"] / math.log(Cc) if kind == 1 else small["confidence"]
        assert np.abs(o["head"]["confidence"] - want).max() <= conf_tol(kind, T, Cc)
        for k, tol in (("mean_prob", H.PROB_TOL), ("prob_std", H.STD_TOL), ("pred_entropy", H.ENT_TOL), ("expected_entropy", H.ENT_TOL),
                       ("mutual_info", H.ENT_TOL), ("agreement", 0.0)):
            assert np.abs(o["unc"][k] - (small[k].astype(np.float32) if k == "agreement" else small[k])).max() <= tol, k
    # pbar of a masked class is exactly 0: its LAC score is exactly 1, and it enters no set with qhat < 1
    for c in dead[:3]:
        assert np.all(op_sets(*args, np.full(n, c, np.int32), score_kind="lac", qhat=0.5)["true_scores"] == 1.0)
    for kw in (dict(score_kind="lac", qhat=float(np.nextafter(np.float32(1), np.float32(0)))), dict(score_kind="aps", qhat=0.999)):
        assert not op_sets(*args, case["labels"], **kw)["members"][:, mask].any()
    u = outs[0]["unc"]
    if live.size < 5:                                               # top-5: the live classes, then the masked ones in index order
        k = live.size
        assert np.all(np.isin(u["top_label"][:, :k], live)) and np.all(u["top_prob"][:, :k] > 0)
        assert np.array_equal(u["top_label"][:, k:], np.tile(dead[:5 - k], (n, 1))) and np.all(u["top_prob"][:, k:] == 0)


def test_tau_edges(lib):
    """tau exactly at a frame's device confidence, one ulp above it, +inf and -inf: fail = 0, 1, 1, 0 in every head that takes tau."""
    case = next(c for c in H.class_count_cases() if c["name"] == "C257_T3")
    lg, temp, y = case["logits"], case["temperature"], case["labels"]
    T, n, Cc = lg.shape
    d, ld = dev_logits(lg)
    for kind in kinds_of(T, Cc):
        conf = op_head(lib, d, T, n, Cc, ld, temp, kind, 0.5)["confidence"]
        for i in (0, n - 1):
            c = conf[i]
            for tau, want in ((float(c), 0), (float(np.nextafter(c, np.float32(np.inf))), 1), (math.inf, 1), (-math.inf, 0)):
                got = [op_head(lib, d, T, n, Cc, ld, temp, kind, tau), op_unc(lib, d, T, n, Cc, ld, temp, kind, tau),
                       op_sets(lib, d, T, n, Cc, ld, temp, kind, tau, y)]
                for g in got:
                    assert g["fail"][i] == want and g["confidence"][i] == c, (kind, i, tau)
                    assert np.array_equal(g["fail"], (conf < np.float32(tau)).astype(np.uint8))


def check_rule(outs, bad, tau_any=True):
    """Every head's outputs on the non-finite frames `bad`."""
    qnan = np.isnan
    for kind, o in outs.items():
        for head in ("head", "unc", "sets"):
            g = o[head]
            assert np.all(g["label"][bad] == 0) and np.all(g["confidence"][bad] == 0.0), (kind, head, g["label"], g["confidence"])
            assert np.all(g["fail"][bad] == 1) and np.all(g["score"][bad] == 1.0), (kind, head)
        u, s, w = o["unc"], o["sets"], o["sweep"]
        for k in ("mean_prob", "prob_std", "pred_entropy", "expected_entropy", "mutual_info", "agreement"):
            assert qnan(u[k][bad]).all(), (kind, k)
        assert np.all(u["top_label"][bad] == -1) and np.all(u["top_prob"][bad] == 0)
        assert np.all(s["set_size"][bad] == 0) and np.all(s["set_mass"][bad] == 0) and not s["members"][bad].any()
        assert np.all(s["u"][bad] == 1.0) and qnan(s["true_scores"][bad]).all()
        assert np.all(w["label"][bad, 0] == 0) and np.all(w["confidence"][bad, 0] == 0.0)
        assert qnan(w["nll"][bad, 0]).all() and qnan(w["brier"][bad, 0]).all()


@pytest.mark.parametrize("case", named(H.nonfinite_cases() + H.overflow_cases()))
def test_nonfinite_frames(lib, case):
    """The rule of include/fav.h for non-finite frames, in all four heads and every conf kind; fail = 1 at tau = -inf too; the
    ordinary frames of the launch have the bits of a launch that holds only them."""
    lg, y = case["logits"], case["labels"]
    T, n, Cc = lg.shape
    good = case["good"]
    bad = np.setdiff1d(np.arange(n), good)
    outs = run_case(lib, case)
    check_rule(outs, bad)
    sub = dict(case, logits=np.ascontiguousarray(lg[:, good]), labels=y[good], name=case["name"] + "_good_only")
    souts = run_case(lib, sub)
    for kind in outs:
        for head in ("head", "unc", "sets", "sweep"):
            for k, v in outs[kind][head].items():
                a, b = np.ascontiguousarray(v[good]), np.ascontiguousarray(souts[kind][head][k])
                assert np.array_equal(a.view(np.uint8), b.view(np.uint8)), (kind, head, k)
    low = dict(case, tau=-math.inf, name=case["name"] + "_tau_-inf")
    louts = run_case(lib, low)
    check_rule(louts, bad)
    for kind in louts:
        for head in ("head", "unc", "sets"):
            assert np.all(louts[kind][head]["fail"][good] == 0)
    # the calibration entry points refuse such a batch through their existing checks
    d, ld = dev_logits(lg)
    from failure_aware_vision_amd.conformal import calibrate_qhat
    with pytest.raises(ValueError, match="NaN"):
        calibrate_qhat(op_sets(lib, d, T, n, Cc, ld, case["temperature"], 0, 0.5, np.zeros(n, np.int32))["true_scores"], 0.1)
    with pytest.raises(ValueError, match="NaN"):
        fit_temperature(lambda t: unpack_cells(op_sweep(lib, d, T, n, Cc, ld, t, 0, np.zeros(n, np.int32))["raw"])["nll"]
                        .astype(np.float64).mean(axis=0))


def test_through_a_handle(lib):
    """A finite checkpoint whose classifier bias overflows at temperature 0.5: every classify entry point flags every frame by
    the rule; at temperature 1 the same handle returns that class with confidence 1."""
    sd, meta = weights.make_synthetic_state_dict("resnet18_cifar", seed=1)
    sd["fc.bias"] = sd["fc.bias"].copy()
    sd["fc.bias"][3] = 3e38
    blob, _ = weights.from_state_dict(meta["arch"], sd, bn_eps=meta["bn_eps"], mean=meta["mean"], std=meta["std"])
    n = 8
    x = torch.from_numpy(synth.synthetic_frames_u8(n, 32, 32, seed=11)).cuda()
    y = np.zeros(n, np.int32)
    for kw in (dict(), dict(n_samples=3, dropout_policy="all_blocks", dropout_p=0.1, seed=4, conf_kind="mutual_info"),
               dict(conf_kind="entropy", tau=-math.inf)):
        be = Backend("resnet18_cifar", blob, max_batch=n, temperature=0.5, **kw)
        lab, conf, fail, score = (t.cpu().numpy() for t in be.classify_detect(x))
        assert np.all(lab == 0) and np.all(conf == 0.0) and np.all(fail == 1) and np.all(score == 1.0), kw
        u = {k: v.cpu().numpy() for k, v in be.classify_uncertainty(x).items()}
        assert np.all(u["label"] == 0) and np.all(u["confidence"] == 0.0) and np.all(u["fail"] == 1) and np.all(u["score"] == 1.0)
        assert np.isnan(u["mean_prob"]).all() and np.isnan(u["mutual_info"]).all() and np.all(u["top_label"] == -1)
        s = {k: v.cpu().numpy() for k, v in be.classify_sets(x, Conformal(kind="aps", qhat=math.inf)).items()}
        assert np.all(s["label"] == 0) and np.all(s["confidence"] == 0.0) and np.all(s["fail"] == 1) and np.all(s["score"] == 1.0)
        assert np.all(s["set_size"] == 0) and not s["members"].any() and np.all(s["ambiguous"])
        cells = unpack_cells(be.calibration_sweep(x, y, [0.5, 0.25, 0.9]).cpu().numpy())
        assert np.all(cells["label"][:, :2] == 0) and np.all(cells["confidence"][:, :2] == 0.0)
        assert np.isnan(cells["nll"][:, :2]).all() and np.isnan(cells["brier"][:, :2]).all()
        # 3e38 / 0.9 is still finite: that temperature's cells are ordinary
        assert np.all(cells["label"][:, 2] == 3) and np.all(cells["confidence"][:, 2] == 1.0) and np.isfinite(cells["nll"][:, 2]).all()
        with pytest.raises(ValueError, match="NaN"):
            be.calibrate_conformal(x, y, alpha=0.1)
        with pytest.raises(ValueError, match="NaN"):
            be.calibrate_temperature(x, y, lo=0.25, hi=0.9)
        be.set_temperature(1.0)
        lab, conf, fail, score = (t.cpu().numpy() for t in be.classify_detect(x))
        assert np.all(lab == 3) and np.all(conf == 1.0) and np.all(fail == 0) and np.all(score == 0.0), kw
        be.close()
