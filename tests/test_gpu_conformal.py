"""The conformal prediction-set head on the GPU (fav_op_head_sets, fav_classify_sets, fav_conformal_scores,
Backend.classify_sets / calibrate_conformal, classify_sharded(sets=...)) against the tests' float64 reference
(conformal_ref.py), against the existing heads (label and confidence bit for bit), and against itself (the calibration
score is the value the membership test compares, so the self-consistency checks are exact).

Tolerances (fp32 device arithmetic vs float64): membership is exact except for classes whose reference score lies within
SCORE_TOL of qhat, and except inside a run of classes whose pbar differ by less than TIE_GAP (fp32 may order them either
way) when the run straddles the set's boundary."""
import math
import os
import subprocess
import sys

import numpy as np
import pytest

pytestmark = pytest.mark.gpu

torch = pytest.importorskip("torch")
from failure_aware_vision_amd import Backend, Conformal, _lib, calibrate_qhat, synth, unpack_sets, weights  # noqa: E402
from failure_aware_vision_amd.corrupt import Corruptor  # noqa: E402
from conformal_ref import draws, pbar_of, scores  # noqa: E402

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
TIE_GAP = 1e-5
SCORE_TOL = 1e-5
MASS_TOL = 2e-5
#: the synthetic checkpoints spread pbar thinly over 1000 classes, so an APS boundary often falls inside a long near-tie run
MODEL_FRAC = 0.5

CASES = {"lac": Conformal(kind="lac", qhat=0.9),
         "aps": Conformal(kind="aps", randomized=True, qhat=0.9, seed=77),
         "raps": Conformal(kind="aps", randomized=True, lam=0.01, k_reg=2, qhat=0.95, seed=5)}


@pytest.fixture(scope="module")
def lib():
    assert torch.cuda.is_available(), "GPU tests need a MI355X"
    return _lib.load()


def ref_kw(cp, first_index=0):
    return dict(kind=cp.kind, randomized=cp.randomized, lam=cp.lam, k_reg=cp.k_reg, seed=cp.seed, first_index=first_index)


def op_sets(lib, lg, T, n, Cc, ld, temp, kind, tau, cp, first_index=0, labels=None, records=True):
    """-> (unpacked numpy records or None, fail, score, true_scores or None, status)."""
    d = torch.from_numpy(np.ascontiguousarray(lg)).cuda()
    rec = torch.full((n, 40), -7, dtype=torch.int32, device="cuda") if records else None
    fail = torch.empty(n, dtype=torch.uint8, device="cuda")
    score = torch.empty(n, dtype=torch.float32, device="cuda")
    lab = torch.from_numpy(np.asarray(labels, np.int32)).cuda() if labels is not None else None
    ts = torch.full((n,), -5.0, dtype=torch.float32, device="cuda") if labels is not None else None
    c = cp.to_c() if isinstance(cp, Conformal) else cp
    st = lib.fav_op_head_sets(d.data_ptr(), T, n, Cc, ld, temp, kind, tau, first_index, c,
                              lab.data_ptr() if lab is not None else None, ts.data_ptr() if ts is not None else None,
                              rec.data_ptr() if rec is not None else None, fail.data_ptr(), score.data_ptr(), None)
    torch.cuda.synchronize()
    got = unpack_sets(rec.cpu().numpy(), Cc) if records else None
    return got, fail.cpu().numpy(), score.cpu().numpy(), (ts.cpu().numpy() if ts is not None else None), st


def comparable(pb, s_ref, member_ref, qhat):
    """Classes whose reference membership the device must reproduce exactly (see the module docstring)."""
    n, Cc = pb.shape
    ok = np.abs(s_ref - qhat) > SCORE_TOL
    order = np.stack([np.lexsort((np.arange(Cc), -row)) for row in pb])
    srt = np.take_along_axis(pb, order, axis=1)
    m_rank = np.take_along_axis(member_ref, order, axis=1)
    for i in range(n):
        g0 = 0
        for r in range(1, Cc + 1):
            if r == Cc or srt[i, r - 1] - srt[i, r] >= TIE_GAP:
                if not (m_rank[i, g0:r].all() or not m_rank[i, g0:r].any()):
                    ok[i, order[i, g0:r]] = False         # a near-tie run across the boundary
                g0 = r
    return ok


def assert_prefix(got, pb):
    """Every set is a prefix of the sort order: set_size counts the members, and no class outside the set has a pbar
    above a member's (beyond a near-tie of TIE_GAP, which fp32 may order either way)."""
    m = got["members"]
    assert np.array_equal(m.sum(axis=1), got["set_size"])
    for i in range(m.shape[0]):
        if m[i].any() and not m[i].all():
            assert pb[i][m[i]].min() >= pb[i][~m[i]].max() - TIE_GAP, i


def check_vs_reference(got, lg, temp, cp, first_index=0):
    pb = pbar_of(lg, temp)
    s_ref, u_ref, _, _ = scores(pb, **ref_kw(cp, first_index))
    member_ref = s_ref <= cp.qhat
    ok = comparable(pb, s_ref, member_ref, cp.qhat)
    assert np.array_equal(got["members"][ok], member_ref[ok]), np.argwhere(got["members"] != member_ref)[:10]
    near = (np.abs(s_ref - cp.qhat) <= SCORE_TOL).sum(axis=1)          # classes either side may take
    assert np.all(np.abs(got["set_size"] - member_ref.sum(axis=1)) <= near)
    mass_ref = (pb * got["members"]).sum(axis=1)
    np.testing.assert_allclose(got["set_mass"], mass_ref, rtol=0, atol=MASS_TOL)
    if cp.kind == "lac":
        assert np.all(got["u"] == 0)
    else:
        assert np.array_equal(got["u"], u_ref.astype(np.float32))
    return ok.mean()


def logits_case(T, n, Cc, ld, seed):
    """A frame's own class preferences plus per-sample noise: pbar spread like a model's, not flat over the classes."""
    rng = np.random.default_rng(seed)
    lg = np.zeros((T, n, ld), np.float32)
    base = rng.standard_normal((1, n, Cc)) * 3
    lg[:, :, :Cc] = (base + rng.standard_normal((T, n, Cc)) * 1.5).astype(np.float32)
    lg[:, :, Cc:] = 1e9  # padding columns must be ignored
    return lg


@pytest.mark.parametrize("T,n,Cc,ld", [(1, 6, 1000, 1024), (2, 5, 7, 8), (30, 9, 1000, 1024), (64, 3, 100, 128),
                                       (2, 4, 10, 64), (30, 4, 1024, 1024), (1, 7, 257, 260)])
@pytest.mark.parametrize("name", ["lac", "aps", "raps"])
def test_op_vs_float64_reference(lib, T, n, Cc, ld, name):
    cp = CASES[name]
    lg = logits_case(T, n, Cc, ld, T * 1000 + Cc)
    got, fail, score, _, st = op_sets(lib, lg, T, n, Cc, ld, 1.3, 0, 0.4, cp, first_index=17)
    assert st == 0
    frac = check_vs_reference(got, lg[:, :, :Cc], 1.3, cp, first_index=17)
    assert frac > 0.99
    assert_prefix(got, pbar_of(lg[:, :, :Cc], 1.3))
    assert np.array_equal(fail, (got["confidence"] < np.float32(0.4)).astype(np.uint8))


@pytest.mark.parametrize("T,n,Cc,ld", [(1, 5, 1000, 1024), (30, 9, 1000, 1024), (3, 4, 10, 64), (7, 3, 257, 320),
                                       (64, 2, 1024, 1024)])
def test_label_and_confidence_bitwise_vs_existing_heads(lib, T, n, Cc, ld):
    rng = np.random.default_rng(T + Cc)
    lg = np.zeros((T, n, ld), np.float32)
    lg[:, :, :Cc] = (rng.standard_normal((T, n, Cc)) * 4).astype(np.float32)
    for kind in (0, 1, 2):
        got, fail, score, _, st = op_sets(lib, lg, T, n, Cc, ld, 1.3, kind, 0.4, CASES["aps"])
        assert st == 0
        if kind < 2:
            labels = torch.empty(n, dtype=torch.int32, device="cuda")
            conf = torch.empty(n, dtype=torch.float32, device="cuda")
            hf = torch.empty(n, dtype=torch.uint8, device="cuda")
            hs = torch.empty(n, dtype=torch.float32, device="cuda")
            d = torch.from_numpy(lg).cuda()
            _lib.check(lib.fav_op_head(d.data_ptr(), T, n, Cc, ld, 1.3, kind, 0.4, labels.data_ptr(), conf.data_ptr(),
                                       hf.data_ptr(), hs.data_ptr(), None))
            labels, conf, hf, hs = (t.cpu().numpy() for t in (labels, conf, hf, hs))
        else:
            d = torch.from_numpy(lg).cuda()
            rec = torch.empty((n, 18), dtype=torch.int32, device="cuda")
            hf = torch.empty(n, dtype=torch.uint8, device="cuda")
            hs = torch.empty(n, dtype=torch.float32, device="cuda")
            _lib.check(lib.fav_op_head_uncertainty(d.data_ptr(), T, n, Cc, ld, 1.3, kind, 0.4, rec.data_ptr(), hf.data_ptr(),
                                                   hs.data_ptr(), None))
            r = rec.cpu().numpy()
            labels, conf, hf, hs = r[:, 0], r[:, 1].view(np.float32), hf.cpu().numpy(), hs.cpu().numpy()
        assert np.array_equal(got["label"], labels), kind
        assert np.array_equal(got["confidence"].view(np.int32), conf.view(np.int32)), kind
        assert np.array_equal(fail, hf) and np.array_equal(score.view(np.int32), hs.view(np.int32)), kind


@pytest.mark.parametrize("Cc,T", [(10, 8), (1000, 30), (100, 1)])
def test_self_consistency_is_exact(lib, Cc, T):
    """qhat = s(y) from the calibration path puts y in the set; one ulp below leaves it out; sets are prefixes; a set
    of size k <= 5 is the uncertainty head's top-k."""
    n, ld = 12, (Cc + 3) // 4 * 4
    lg = logits_case(T, n, Cc, ld, Cc + T)
    rng = np.random.default_rng(Cc)
    y = rng.integers(0, Cc, n).astype(np.int32)
    y[:3] = [int(np.argmax(pbar_of(lg[:, i:i + 1, :Cc])[0])) for i in range(3)]     # the label itself too
    d = torch.from_numpy(lg).cuda()
    urec = torch.empty((n, 18), dtype=torch.int32, device="cuda")
    _lib.check(lib.fav_op_head_uncertainty(d.data_ptr(), T, n, Cc, ld, 1.0, 0, 0.5, urec.data_ptr(), None, None, None))
    top = urec.cpu().numpy()[:, 8:13]
    for name, base in CASES.items():
        _, _, _, sy, st = op_sets(lib, lg, T, n, Cc, ld, 1.0, 0, 0.5, base, first_index=40, labels=y, records=False)
        assert st == 0 and np.all(np.isfinite(sy))
        for i in range(n):
            one = lg[:, i:i + 1]
            for q, inside in ((float(sy[i]), True), (float(np.nextafter(np.float32(sy[i]), np.float32(-np.inf))), False)):
                cp = Conformal(kind=base.kind, randomized=base.randomized, lam=base.lam, k_reg=base.k_reg, qhat=q, seed=base.seed)
                got, _, _, _, st = op_sets(lib, one, T, 1, Cc, ld, 1.0, 0, 0.5, cp, first_index=40 + i)
                assert st == 0
                assert bool(got["members"][0, y[i]]) == inside, (name, i, q)
                k = int(got["set_size"][0])
                # a prefix of the device's own order: the top-k set of pbar is the set of the k classes the
                # uncertainty head ranks first (checked here up to k = 5) and never skips a class
                if 1 <= k <= 5:
                    assert set(np.flatnonzero(got["members"][0]).tolist()) == set(top[i, :k].tolist()), (name, i, k)
                assert_prefix(got, pbar_of(one[:, :, :Cc]))


def test_ties_follow_the_lowest_index_rule(lib):
    T, n, Cc, ld = 2, 3, 50, 64
    lg = np.zeros((T, n, ld), np.float32)
    lg[:, 0, :] = 0.0                                   # flat: every class 1/50, ranked by index
    lg[:, 1, [40, 7, 23]] = 30.0                        # three tied leaders carry all the mass: 7, 23, 40
    lg[:, 2, :Cc] = np.arange(Cc, dtype=np.float32) * 0  # flat again
    cp = Conformal(kind="aps", qhat=3.5 / 50)           # mass ahead + pbar: rank r has score (r + 1) / 50
    got, _, _, _, _ = op_sets(lib, lg, T, n, Cc, ld, 1.0, 0, 0.5, cp)
    assert np.flatnonzero(got["members"][0]).tolist() == [0, 1, 2]
    assert got["label"].tolist() == [0, 7, 0]
    cp = Conformal(kind="aps", qhat=0.5)                # leaders: 1/3 ahead of 7, 2/3 ahead of 23 -> {7} only
    got, _, _, _, _ = op_sets(lib, lg, T, n, Cc, ld, 1.0, 0, 0.5, cp)
    assert np.flatnonzero(got["members"][1]).tolist() == [7]
    cp = Conformal(kind="aps", qhat=0.7)
    got, _, _, _, _ = op_sets(lib, lg, T, n, Cc, ld, 1.0, 0, 0.5, cp)
    assert np.flatnonzero(got["members"][1]).tolist() == [7, 23]
    lac = Conformal(kind="lac", qhat=1.0 - 1.0 / 50)    # LAC on a flat frame: every class or none
    got, _, _, _, _ = op_sets(lib, lg, T, n, Cc, ld, 1.0, 0, 0.5, lac)
    assert got["set_size"][0] in (0, 50) and got["set_size"][2] == got["set_size"][0]


def test_randomization_is_keyed_by_seed_and_global_frame(lib):
    T, n, Cc, ld = 4, 10, 100, 100
    lg = logits_case(T, n, Cc, ld, 3)
    cp = CASES["aps"]
    whole, _, _, _, _ = op_sets(lib, lg, T, n, Cc, ld, 1.0, 0, 0.5, cp, first_index=1000)
    assert np.array_equal(whole["u"], draws(cp.seed, 1000 + np.arange(n)).astype(np.float32))
    a, _, _, _, _ = op_sets(lib, lg[:, :4], T, 4, Cc, ld, 1.0, 0, 0.5, cp, first_index=1000)
    b, _, _, _, _ = op_sets(lib, lg[:, 4:], T, 6, Cc, ld, 1.0, 0, 0.5, cp, first_index=1004)
    for k in whole:
        assert np.array_equal(np.concatenate([a[k], b[k]]), whole[k]), k
    shifted, _, _, _, _ = op_sets(lib, lg, T, n, Cc, ld, 1.0, 0, 0.5, cp, first_index=1001)
    assert np.array_equal(shifted["u"][:-1], whole["u"][1:])
    other, _, _, _, _ = op_sets(lib, lg, T, n, Cc, ld, 1.0, 0, 0.5, Conformal(kind="aps", randomized=True, qhat=0.9, seed=78),
                                first_index=1000)
    assert not np.array_equal(other["u"], whole["u"])
    plain, _, _, _, _ = op_sets(lib, lg, T, n, Cc, ld, 1.0, 0, 0.5, Conformal(kind="aps", qhat=0.9))
    assert np.all(plain["u"] == 1)


def test_op_misuse(lib):
    lg = torch.zeros((2, 1, 64), dtype=torch.float32, device="cuda")
    rec = torch.zeros((2, 40), dtype=torch.int32, device="cuda")
    good = CASES["aps"].to_c()
    nan_q = Conformal(qhat=float("nan")).to_c()
    bad_size = Conformal(qhat=0.5).to_c()
    bad_size.struct_size = 24
    for c in (nan_q, bad_size):
        assert lib.fav_op_head_sets(lg.data_ptr(), 2, 1, 50, 64, 1.0, 0, 0.5, 0, c, None, None, rec.data_ptr(), None, None, None) == 1
    assert lib.fav_op_head_sets(lg.data_ptr(), 2, 1, 50, 64, 1.0, 0, 0.5, 0, good, None, None, rec.data_ptr() + 4, None, None, None) == 1
    big = torch.zeros((2, 1, 1028), dtype=torch.float32, device="cuda")
    assert lib.fav_op_head_sets(big.data_ptr(), 2, 1, 1025, 1028, 1.0, 0, 0.5, 0, good, None, None, rec.data_ptr(), None, None, None) == 1
    # calibration labels outside [0, C) score NaN
    lgs = logits_case(2, 4, 10, 12, 1)
    _, _, _, sy, st = op_sets(_lib.load(), lgs, 2, 4, 10, 12, 1.0, 0, 0.5, CASES["raps"], labels=[3, -1, 10, 9], records=False)
    assert st == 0 and np.isfinite(sy[[0, 3]]).all() and np.isnan(sy[[1, 2]]).all()
    with pytest.raises(ValueError):
        calibrate_qhat(sy, 0.1)


def test_backend_misuse(r18_blob):
    blob, _ = r18_blob
    be = Backend("resnet18_cifar", blob, max_batch=4, n_samples=3, dropout_policy="all_blocks", dropout_p=0.1, seed=4)
    x = torch.from_numpy(synth.synthetic_frames_u8(5, 32, 32, seed=1)).cuda()
    rec = torch.zeros((6, 40), dtype=torch.int32, device="cuda")
    good = CASES["aps"].to_c()
    assert be.lib.fav_classify_sets(be._h, x.data_ptr(), 2, 0, 0, good, rec.data_ptr() + 4, None, None, None) == 1
    assert be.lib.fav_classify_sets(be._h, x.data_ptr(), 2, 0, 0, good, None, None, None, None) == 1
    assert be.lib.fav_classify_sets(be._h, x.data_ptr(), 5, 0, 0, good, rec.data_ptr(), None, None, None) == 1
    assert be.lib.fav_classify_sets(be._h, x.data_ptr(), 2, 0, 0, Conformal(qhat=float("nan")).to_c(), rec.data_ptr(),
                                    None, None, None) == 1
    with pytest.raises(_lib.FavError):
        be.classify_sets(x, CASES["aps"])                              # n > max_batch
    with pytest.raises(ValueError):
        be.classify_sets(x[:2], CASES["aps"], out=rec[:2, :39])
    with pytest.raises(_lib.FavError):
        be.classify_sets(x[:2], Conformal(kind="lac", randomized=True, qhat=0.5))
    s = be.conformal_scores(x, torch.tensor([0, 1, 99, -3, 2], dtype=torch.int32, device="cuda"), CASES["lac"])
    s = s.cpu().numpy()
    assert np.isnan(s[[2, 3]]).all() and np.isfinite(s[[0, 1, 4]]).all()
    be.close()


def backend_vs_reference(be, frames, cp):
    """classify_sets vs classify_detect (label / conf bits) and vs the float64 reference of the logits the same call
    produced."""
    out = be.classify_sets(frames, cp)
    lg = be.logits().cpu().numpy()
    got = {k: v.cpu().numpy() for k, v in out.items()}
    labels, conf, fail, score = (t.cpu().numpy() for t in be.classify_detect(frames))
    assert np.array_equal(got["label"], labels)
    assert np.array_equal(got["confidence"].view(np.int32), conf.view(np.int32))
    assert np.array_equal(got["fail"], fail) and np.array_equal(got["score"].view(np.int32), score.view(np.int32))
    assert np.array_equal(got["ambiguous"], got["set_size"] != 1)
    frac = check_vs_reference(got, lg, be.cfg.temperature, cp)
    print(f"{cp.kind} lam={cp.lam}: {frac:.4f} of the classes compared exactly, mean set size {got['set_size'].mean():.1f}")
    return got, frac


def test_resnet50_headline_sets(r50_blob):
    """ResNet-50, MC-Dropout T = 30 all_blocks p = 0.1, 64 severity-3 Gaussian-noise frames."""
    blob, _ = r50_blob
    u8 = torch.from_numpy(synth.synthetic_frames_u8(64, 224, 224, seed=21)).cuda()
    frames = Corruptor(seed=3).gaussian(u8, 3)
    be = Backend("resnet50", blob, max_batch=64, n_samples=30, dropout_policy="all_blocks", dropout_p=0.1, seed=4)
    for cp in CASES.values():
        got, frac = backend_vs_reference(be, frames, cp)
        assert frac > MODEL_FRAC
        assert_prefix(got, pbar_of(be.logits().cpu().numpy(), be.cfg.temperature))
    be.close()


def test_ensemble_members_are_the_samples(r50_members):
    x = torch.from_numpy(synth.synthetic_frames_u8(16, 224, 224, seed=21)).cuda()
    ens = Backend("resnet50", [b for b, _ in r50_members], max_batch=16)
    got, frac = backend_vs_reference(ens, x, CASES["raps"])
    assert frac > MODEL_FRAC and ens.logits().shape[0] == 5
    ens.close()


def test_vit_single_pass():
    vblob, _ = weights.make_synthetic_vit("vit_tiny", seed=3)
    frames = synth.synthetic_frames_u8(4, 64, 64, seed=11)
    vit = Backend("vit_tiny", vblob, max_batch=4, temperature=1.5, conf_kind="entropy")
    got, frac = backend_vs_reference(vit, torch.from_numpy(frames).cuda(), CASES["aps"])
    assert frac > MODEL_FRAC and vit.logits().shape[0] == 1
    host = vit.classify_sets(frames, CASES["aps"])                     # numpy in: numpy out, synchronous
    assert isinstance(host["members"], np.ndarray) and np.array_equal(host["members"], got["members"])
    vit.close()


def test_coverage_on_labels_drawn_from_the_model(r18_blob):
    """Labels y ~ Categorical(pbar) make the model calibrated by construction; split conformal at alpha = 0.1 must cover
    about 90 % of the test half (seeds fixed: deterministic)."""
    blob, _ = r18_blob
    n_half, alpha = 600, 0.1
    be = Backend("resnet18_cifar", blob, max_batch=200, n_samples=8, dropout_policy="all_blocks", dropout_p=0.2, seed=4,
                 temperature=0.25)
    frames = torch.from_numpy(synth.synthetic_frames_u8(2 * n_half, 32, 32, seed=9)).cuda()
    pbs = []
    for b in range(0, 2 * n_half, 200):
        be.classify(frames[b:b + 200], first_index=b)
        pbs.append(pbar_of(be.logits().cpu().numpy(), be.cfg.temperature))
    pb = np.concatenate(pbs)
    rng = np.random.default_rng(2024)
    y = np.array([rng.choice(pb.shape[1], p=row / row.sum()) for row in pb], np.int32)
    assert len(set(y.tolist())) > 3                                    # not a degenerate model
    cal, test = slice(0, n_half), slice(n_half, 2 * n_half)
    for method in ("lac", "aps"):
        cp = be.calibrate_conformal(frames[cal], torch.from_numpy(y[cal]).cuda(), alpha, method=method, randomized=True,
                                    seed=11)
        s = be.conformal_scores(frames[cal], torch.from_numpy(y[cal]).cuda(), cp).cpu().numpy()
        assert (s <= np.float32(cp.qhat)).mean() >= math.ceil((n_half + 1) * (1 - alpha)) / n_half
        covered = []
        for b in range(n_half, 2 * n_half, 200):
            r = be.classify_sets(frames[b:b + 200], cp, first_index=b)
            m = r["members"].cpu().numpy()
            covered.append(m[np.arange(m.shape[0]), y[b:b + 200]])
        cov = np.concatenate(covered).mean()
        print(f"coverage {method}: {cov:.4f} (qhat {cp.qhat:.6f})")
        assert 0.84 <= cov <= 0.96, (method, cov)
    be.close()


_SHARD_WORKER = r"""
import os, sys
sys.path.insert(0, {root!r})
import torch, torch.distributed as dist
from failure_aware_vision_amd import Backend, Conformal, classify_sharded, shard_range, synth, weights
rank, world = int(os.environ["RANK"]), int(os.environ["WORLD_SIZE"])
dist.init_process_group("gloo", rank=rank, world_size=world)
torch.cuda.set_device(0)
blob, _ = weights.make_synthetic("resnet18_cifar", seed=1)
be = Backend("resnet18_cifar", blob, max_batch=11, n_samples=5, dropout_policy="all_blocks", dropout_p=0.1, seed=4)
cp = Conformal(kind="aps", randomized=True, lam=0.01, k_reg=1, qhat=0.8, seed=3)
for n in (11, 8):
    x = torch.from_numpy(synth.synthetic_frames_u8(n, 32, 32, seed=5)).cuda()
    full = be.classify_sets(x, cp)
    s, e = shard_range(n, rank, world)
    got = classify_sharded(be, x[s:e].contiguous(), n, rank, world, sets=cp)
    assert set(got) == set(full) - {{"fail", "score", "ambiguous"}}
    for k in got:
        a, b = got[k].contiguous(), full[k].contiguous()
        assert torch.equal(a if a.dtype == torch.bool else a.view(torch.int32),
                           b if b.dtype == torch.bool else b.view(torch.int32)), (n, k)
be.close()
dist.barrier(); dist.destroy_process_group()
print("rank", rank, "ok")
"""


def test_sharded_sets_bitwise_two_gloo_ranks(tmp_path):
    script = tmp_path / "worker.py"
    script.write_text(_SHARD_WORKER.format(root=ROOT))
    env = dict(os.environ, MASTER_ADDR="127.0.0.1", MASTER_PORT="29559", WORLD_SIZE="2", OMP_NUM_THREADS="2")
    procs = [subprocess.Popen([sys.executable, str(script)], env=dict(env, RANK=str(r)), stdout=subprocess.PIPE,
                              stderr=subprocess.STDOUT) for r in range(2)]
    try:
        outs = [p.communicate(timeout=300)[0].decode() for p in procs]
    finally:
        for p in procs:
            if p.poll() is None:
                p.kill()
    for p, o in zip(procs, outs):
        assert p.returncode == 0, o
