"""tests/heads_ref.py on the CPU: the one float64 reference of the four confidence heads against the four older
restatements of pbar (oracle.fav_oracle.confidence_head, uncertainty_ref, conformal_ref, calibration_ref) on their
Gaussian cases, against the closed forms of the constructed edge cases, and the caps - the shares of the random cases
that survive the near-tie filters - on exactly the inputs tests/test_gpu_heads_edges.py runs on the GPU."""
import numpy as np
import pytest

import calibration_ref
import conformal_ref
import heads_ref as H
import uncertainty_ref
from oracle import fav_oracle as O

GAUSS = [(1, 5, 1000), (30, 9, 1000), (3, 4, 10), (7, 3, 257), (2, 5, 7)]


@pytest.mark.parametrize("T,n,C", GAUSS)
def test_agrees_with_the_four_existing_references(T, n, C):
    lg = (np.random.default_rng(T * 100 + C).standard_normal((T, n, C)) * 4).astype(np.float32)
    y = np.random.default_rng(C).integers(-1, C + 1, n)
    for kind in (0, 1, 2):
        r = H.heads_ref(lg, 1.3, kind, 0.4, true_labels=y)
        assert not r["nonfinite"].any()
        u = uncertainty_ref.head_uncertainty(lg, 1.3, kind, 0.4)     # same roundings: equal up to float64 summation order
        for k in ("label", "top_label", "fail"):
            assert np.array_equal(r[k], u[k]), k
        for k in uncertainty_ref.FLOAT_FIELDS + ("top_prob", "score"):
            if T == 1 and k in ("expected_entropy", "mutual_info"):
                continue                                             # heads_ref states the T = 1 identity, uncertainty_ref sums
            np.testing.assert_allclose(r[k], u[k], rtol=0, atol=1e-12, err_msg=k)
        c = calibration_ref.cells_of(lg, y, 1.3, kind)               # keeps the float64 product: differs by |z| 2^-24
        ok = r["label_ok"]
        assert np.array_equal(r["label"][ok], c["label"][ok])
        np.testing.assert_allclose(r["confidence"], c["confidence"], rtol=0, atol=H.ENT_TOL)
        bad = np.isnan(c["nll"])
        assert np.array_equal(np.isnan(r["nll"]), bad) and np.array_equal(np.isnan(r["brier"]), bad)
        assert H.error_measure(r["nll"][~bad], c["nll"][~bad]).max() <= H.NLL_TOL
        assert H.error_measure(r["brier"][~bad], c["brier"][~bad]).max() <= H.NLL_TOL
    r = H.heads_ref(lg, 1.3, 0, 0.4, true_labels=y)
    pb = conformal_ref.pbar_of(lg, 1.3)
    np.testing.assert_allclose(r["pbar"], pb, rtol=0, atol=1e-15)
    for kw in (dict(kind="lac"), dict(kind="aps"), dict(kind="aps", lam=0.02, k_reg=3), dict(kind="aps", randomized=True, seed=9, first_index=4)):
        s_ref, u_ref, order, rank = conformal_ref.scores(pb, **kw)
        mine = dict(kw)
        mine["score_kind"] = mine.pop("kind")
        s = H.sets_ref(r, qhat=0.8, true_labels=y, **mine)
        np.testing.assert_allclose(s["s"], s_ref, rtol=0, atol=1e-12)
        assert np.array_equal(s["rank"], rank) and np.array_equal(r["order"], order) and np.array_equal(s["u"], u_ref)
        assert np.array_equal(s["members"], s_ref <= 0.8)
    for kind in (O.CONF_MAX_SOFTMAX, O.CONF_ENTROPY):                # the fp32 oracle, per sample set [T, n, C]
        ol, oc, opb = O.confidence_head(lg, 1.3, kind)
        rr = H.heads_ref(lg, 1.3, kind)
        assert np.array_equal(ol[rr["label_ok"]], rr["label"][rr["label_ok"]])
        np.testing.assert_allclose(opb, rr["pbar"], rtol=0, atol=H.PROB_TOL)
        np.testing.assert_allclose(oc, rr["confidence"], rtol=0, atol=H.PROB_TOL if kind == 0 else H.ENT_TOL)


def by_name(cases):
    return {c["name"]: c for c in cases}


def ref_of(c, kind=0):
    return H.heads_ref(c["logits"], c["temperature"], kind, c["tau"], true_labels=c["labels"])


@pytest.mark.parametrize("name", [c["name"] for c in H.saturated_cases()])
def test_saturated_rows_closed_forms(name):
    c = by_name(H.saturated_cases())[name]
    T, n, C = c["logits"].shape
    z = H.scaled(c["logits"], c["temperature"]).astype(np.float64)
    srt = np.sort(z, axis=2)
    assert np.all(srt[:, :, -1] - srt[:, :, -2] >= 104.0)            # every other exponential is exactly 0 in fp32
    win = c["winner"]
    rows = np.arange(n)
    tiny = 1e-50        # float64 keeps exp(-130) = 1e-57 where fp32 has an exact 0: the closed forms hold to that in the reference
    if "agree" in name:
        for kind in (0, 1, 2):
            r = ref_of(c, kind)
            onehot = np.zeros((n, C))
            onehot[rows, win] = 1.0
            assert np.abs(r["pbar"] - onehot).max() < tiny and np.array_equal(r["label"], win)
            assert np.all(r["confidence"] == 1.0) and np.all(r["score"] == 0.0) and np.all(r["fail"] == 0)
            for k in ("pred_entropy", "expected_entropy", "mutual_info", "prob_std"):
                assert np.all(np.abs(r[k]) < tiny), k
            assert np.all(r["agreement"] == 1.0) and np.all(r["mean_prob"] == 1.0)
            right = c["labels"] == win
            assert np.all(np.abs(r["nll"][right]) < tiny) and np.all(r["brier"][right] < tiny)
            assert np.all(r["nll"][~right] == -np.log(H.FLT_MIN)) and np.all(np.abs(r["brier"][~right] - 2.0) < 1e-15)
        r = ref_of(c)
        lac = H.sets_ref(r, "lac", qhat=0.5)
        assert np.abs(lac["s"] - (1.0 - onehot)).max() < tiny and np.array_equal(lac["members"], onehot == 1)
        # APS: s(winner) = u * 1 + 0 = u, every other score is exactly 1: the set is the winner alone for u <= qhat < 1
        aps = H.sets_ref(r, "aps", qhat=np.nextafter(1.0, 0.0), randomized=True, seed=5)
        assert np.all(aps["u"] < 1.0) and np.abs(aps["s"] - np.where(onehot == 1, aps["u"][:, None], 1.0)).max() < 1e-15
        assert np.array_equal(aps["members"], onehot == 1)
        assert not H.sets_ref(r, "aps", qhat=np.nextafter(1.0, 0.0))["members"].any()   # u = 1: s(winner) = 1 > qhat
    else:
        r = ref_of(c)
        other = c["other"]
        assert np.all(r["pbar"][rows, win] == 0.5) and np.all(r["pbar"][rows, other] == 0.5) and np.all(r["pbar"].sum(axis=1) - 1.0 < tiny)
        assert np.array_equal(r["label"], win) and np.array_equal(r["top_label"][:, 1], other)
        assert np.array_equal(r["order"][:, 0], win) and np.array_equal(r["order"][:, 1], other)
        assert np.all(r["agreement"] == 0.5) and np.all(r["prob_std"] == 0.5)
        np.testing.assert_allclose(r["pred_entropy"], np.log(2.0), rtol=0, atol=1e-15)
        assert np.all(np.abs(r["expected_entropy"]) < tiny)


@pytest.mark.parametrize("name", [c["name"] for c in H.flat_cases()])
def test_flat_rows_closed_forms(name):
    c = by_name(H.flat_cases())[name]
    T, n, C = c["logits"].shape
    r = ref_of(c, 1)
    assert np.all(r["pbar"] == r["pbar"][:, :1]) and np.abs(r["pbar"] - 1.0 / C).max() < 1e-15 and np.all(r["label"] == 0)
    assert np.array_equal(r["top_label"], np.tile(np.arange(5), (n, 1)))
    np.testing.assert_allclose(r["pred_entropy"], np.log(C), rtol=0, atol=1e-12)
    np.testing.assert_allclose(r["confidence"], 0.0, rtol=0, atol=1e-12)
    assert np.all(r["mutual_info"] <= 1e-12) and np.all(r["agreement"] == 1.0)
    aps = H.sets_ref(ref_of(c), "aps", qhat=0.5)
    assert np.all(np.diff(aps["s"], axis=1) >= 0)                    # non-decreasing in class index


def test_one_class_closed_form():
    c = by_name(H.class_count_cases())["C1_T3"]
    for kind in (0, 1):
        r = ref_of(c, kind)
        assert np.all(r["label"] == 0) and np.all(r["pbar"] == 1.0) and np.all(r["confidence"] == 1.0)
        assert np.array_equal(r["top_label"], np.tile([0, -1, -1, -1, -1], (16, 1)))
        assert np.array_equal(r["top_prob"], np.tile([1.0, 0, 0, 0, 0], (16, 1)))


@pytest.mark.parametrize("name", [c["name"] for c in H.masked_cases() if "some" not in c["name"]])
def test_masked_classes_closed_forms(name):
    c = by_name(H.masked_cases())[name]
    mask = c["mask"]
    live = np.flatnonzero(~mask)
    for kind in (0, 1, 2):
        r = ref_of(c, kind)
        assert not r["nonfinite"].any()
        assert np.all(r["pbar"][:, mask] == 0.0) and not mask[r["label"]].any()
        small = H.heads_ref(c["logits"][:, :, live], c["temperature"], kind, c["tau"])
        assert np.array_equal(r["label"], live[small["label"]])
        for k in ("mean_prob", "prob_std", "pred_entropy", "expected_entropy", "mutual_info", "agreement"):
            np.testing.assert_allclose(r[k], small[k], rtol=0, atol=1e-12, err_msg=k)
        if kind == 0:
            np.testing.assert_allclose(r["confidence"], small["confidence"], rtol=0, atol=1e-12)
        # the order: every class with a pbar the device holds as positive first, then the device zeros - all masked classes
        # among them - by index
        zero = r["pbar"] < H.ZERO_BELOW
        assert zero[:, mask].all()
        for i in range(r["pbar"].shape[0]):
            k = int((~zero[i]).sum())
            assert r["order"][i, k:].tolist() == np.flatnonzero(zero[i]).tolist() and not zero[i, r["order"][i, :k]].any()
    r = ref_of(c)
    for kind in ("lac", "aps"):
        s = H.sets_ref(r, kind, qhat=0.999)
        assert not s["members"][:, mask].any()
        # the masked classes score 1 (LAC) or at least the whole mass (APS): well clear of qhat = 0.999
        assert np.all(s["s"][:, mask] >= 1.0 - 1e-12)


@pytest.mark.parametrize("name", [c["name"] for c in H.nonfinite_cases() + H.overflow_cases()])
def test_nonfinite_frames_follow_the_rule(name):
    c = by_name(H.nonfinite_cases() + H.overflow_cases())[name]
    n = c["logits"].shape[1]
    good = c["good"]
    bad = np.setdiff1d(np.arange(n), good)
    assert np.isfinite(c["logits"]).all() == ("overflow" in name)
    for kind in (0, 1, 2) if c["logits"].shape[0] >= 2 else (0, 1):
        for tau in (c["tau"], -np.inf):
            r = H.heads_ref(c["logits"], c["temperature"], kind, tau, true_labels=c["labels"])
            assert np.flatnonzero(r["nonfinite"]).tolist() == bad.tolist()
            assert np.all(r["label"][bad] == 0) and np.all(r["confidence"][bad] == 0) and np.all(r["fail"][bad] == 1)
            assert np.all(r["score"][bad] == 1.0)
            for k in ("mean_prob", "prob_std", "pred_entropy", "expected_entropy", "mutual_info", "agreement", "nll", "brier"):
                assert np.isnan(r[k][bad]).all(), k
            assert np.all(r["top_label"][bad] == -1) and np.all(r["top_prob"][bad] == 0)
            sub = H.heads_ref(c["logits"][:, good], c["temperature"], kind, tau, true_labels=c["labels"][good])
            for k in ("label", "confidence", "fail", "score", "mean_prob", "pred_entropy", "top_label", "top_prob", "nll"):
                assert np.array_equal(r[k][good], sub[k], equal_nan=True), k
        s = H.sets_ref(H.heads_ref(c["logits"], c["temperature"], true_labels=c["labels"]), "aps", qhat=np.inf,
                       true_labels=np.zeros(n, np.int32))
        assert np.all(s["set_size"][bad] == 0) and np.all(s["set_mass"][bad] == 0) and np.isnan(s["true_scores"][bad]).all()
        assert np.all(s["set_size"][good] == c["logits"].shape[2])


def kinds_of(c):
    T, _, C = c["logits"].shape
    return (0, 1, 2) if T >= 2 and C >= 2 else (0, 1)


def test_caps_on_the_random_cases():
    """At least 98 % of the frames keep their label comparison, 95 % their top-5 comparison and 95 % their fail comparison
    (every conf kind) - on the reference alone, over all random cases."""
    label_ok, top_ok, fail_ok = [], [], []
    for c in H.random_cases():
        r = ref_of(c)
        assert not r["nonfinite"].any(), c["name"]
        label_ok.append(r["label_ok"])
        top_ok.append(r["top_ok"])
        fail_ok += [ref_of(c, kind)["fail_ok"] for kind in kinds_of(c)]
    shares = [float(np.concatenate(x).mean()) for x in (label_ok, top_ok, fail_ok)]
    print(f"MEASURED caps: frames {np.concatenate(label_ok).size} label {shares[0]:.4f} top-5 {shares[1]:.4f} fail {shares[2]:.4f}")
    assert shares[0] >= 0.98 and shares[1] >= 0.95 and shares[2] >= 0.95


def test_constructed_cases_leave_nothing_out():
    """The constructed cases are compared without a filter: wherever the reference's ranks are not far apart they are
    exact ties by construction (flat rows, the 2:2 split, zeros), which the device reproduces with the lowest-index rule;
    the cases built on Gaussian logits (masked, non-finite, overflow) have no near-tie at all."""
    for c in H.constructed_cases():
        for kind in kinds_of(c):
            r = ref_of(c, kind)
            assert r["fail_ok"].all(), (c["name"], kind)
        r = ref_of(c)
        if c["name"].startswith(("masked", "nonfinite", "overflow")):
            assert r["label_ok"].all() and r["top_ok"].all(), c["name"]
        else:
            srt = np.take_along_axis(r["pbar"], r["order"][:, :6], axis=1)
            d = srt[:, :-1] - srt[:, 1:]
            assert np.all((d > H.TIE_GAP) | (d == 0) | (srt[:, :-1] < H.ZERO_BELOW)), c["name"]


def test_constructed_cases_have_no_score_at_the_threshold():
    """The prediction sets of a constructed case are compared without a filter too - membership of every class, the
    calibration score of every frame: under every set configuration the GPU test runs, no reference score lies within
    SCORE_TOL of qhat, no near-tied run straddles a set's boundary, and every true label's rank is stable."""
    cases = H.constructed_cases()
    # the launches of the non-finite cases' ordinary frames alone (a randomized draw is keyed by the frame's place)
    cases += [dict(c, logits=c["logits"][:, c["good"]], labels=c["labels"][c["good"]]) for c in cases if "good" in c]
    for c in cases:
        r = ref_of(c)
        assert H.rank_stable(r, c["labels"]).all(), c["name"]
        for kw in H.sets_configs(c["logits"].shape[2]):
            s = H.sets_ref(r, true_labels=c["labels"], **kw)
            assert H.members_comparable(r, s["s"], kw["qhat"]).all(), (c["name"], kw)
