"""ONE float64 reference of everything the four confidence heads return (head_kernel, head_unc_kernel, head_sets_kernel,
head_sweep_kernel; include/fav.h), written from the documented contract alone, and
the inputs of the heads' edge tests (tests/test_heads_ref_host.py checks the reference and the inputs on the CPU,
tests/test_gpu_heads_edges.py the kernels against them).

Rounding.  The reference rounds where the contract rounds and nowhere else: inv_temp = fp32(1 / temperature),
z = fp32(logit * inv_temp); everything after that is float64.  The device's single rounding of z is therefore not an error of
the kernel, whatever |z| is.

Non-finite frames.  A frame is non-finite when, in any of its T samples, z holds a NaN or +inf among its C values or is -inf
throughout.  Then label = 0, confidence = 0, fail = 1 whatever tau is, score = 1; the uncertainty statistics are NaN and the
top-5 (-1, 0); every conformal score is NaN (empty set, mass 0); nll and brier are NaN.  -inf in some classes of a row is
finite input (probability 0 in that sample).

Filters (the caps).  fp32 may order a near-tie of the reference's pbar either way, so on RANDOM cases labels (and what hangs on
them) are compared where the reference's top-1 / top-2 gap exceeds TIE_GAP, top-5 rows where every gap between consecutive
ranks among the top 6 does, and fail where |confidence - tau| > TIE_GAP.  A pair of pbar that are both below ZERO_BELOW =
1e-55 in float64 is no near-tie: such a class has exp(z - max) <= 1e-55 x T x C <= 4.2e-49 in every sample, below half the
smallest fp32 denormal (7e-46), so the device holds two exact zeros and the lowest-index rule decides on both sides.  On
CONSTRUCTED cases nothing is filtered."""
import numpy as np

from conformal_ref import draws

FLT_MIN = float(np.finfo(np.float32).tiny)
TIE_GAP = 1e-5
ZERO_BELOW = 1e-55
PROB_TOL, ENT_TOL, STD_TOL = 2e-6, 2e-5, 1e-5       # the constants of test_gpu_uncertainty.py
SCORE_TOL, MASS_TOL = 1e-5, 2e-5                    # the constants of test_gpu_conformal.py
NLL_TOL = 9e-6                                      # TOL of test_gpu_calibration.py, on error_measure
REC_FLOATS = ("confidence", "mean_prob", "prob_std", "pred_entropy", "expected_entropy", "mutual_info", "agreement")


def error_measure(dev, ref):
    """|dev - ref| / max(1, |ref|), elementwise (test_gpu_calibration.py's measure for nll and brier)."""
    dev, ref = np.asarray(dev, np.float64), np.asarray(ref, np.float64)
    return np.abs(dev - ref) / np.maximum(1.0, np.abs(ref))


def scaled(logits, temperature):
    """z = fp32(logit * fp32(1 / temperature)), the contract's two roundings."""
    with np.errstate(over="ignore", invalid="ignore"):
        return np.asarray(logits, np.float32) * (np.float32(1.0) / np.float32(temperature))


def nonfinite_frames(z):
    """bool[n]: the frames of z [T, n, C] that the rule calls non-finite."""
    bad_row = np.isnan(z).any(axis=2) | (z == np.inf).any(axis=2) | (z == -np.inf).all(axis=2)
    return bad_row.any(axis=0)


def _entropy(q, axis=-1):
    with np.errstate(divide="ignore", invalid="ignore"):
        return -np.where(q > 0, q * np.log(np.where(q > 0, q, 1.0)), 0.0).sum(axis=axis)


def _gap_ok(srt):
    """Consecutive ranks of srt [n, k] (descending) that fp32 must order like float64: far apart, both exact zeros on the device, or an
    exact tie (equal by construction - the same operations on the same values - and ordered by index on both sides)."""
    d = srt[:, :-1] - srt[:, 1:]
    return (d > TIE_GAP) | (d == 0) | ((srt[:, :-1] < ZERO_BELOW) & (srt[:, 1:] < ZERO_BELOW))


def heads_ref(logits, temperature=1.0, kind=0, tau=0.5, true_labels=None):
    """logits fp32 [T, n, C] (padding columns cut) -> dict of per-frame float64 / int fields:
      nonfinite, pbar [n, C], order [n, C] (rank -> class), label, confidence, fail, score,
      mean_prob, prob_std, pred_entropy, expected_entropy, mutual_info, agreement, top_label / top_prob [n, 5],
      nll, brier (NaN without true_labels or where the label is outside [0, C)),
      label_ok, top_ok, fail_ok (the filters of the module docstring)."""
    z32 = scaled(logits, temperature)
    T, n, C = z32.shape
    bad = nonfinite_frames(z32)
    z = np.where(bad[None, :, None], 0.0, z32.astype(np.float64))
    with np.errstate(invalid="ignore"):
        e = np.exp(z - z.max(axis=2, keepdims=True))
    p = e / e.sum(axis=2, keepdims=True)
    pbar = p.mean(axis=0)
    idx = np.arange(C)
    # the sort key treats what the device holds as exact zeros (module docstring) as zeros: ordered by index
    key = np.where(pbar < ZERO_BELOW, 0.0, pbar)
    order = np.stack([np.lexsort((idx, -key[i])) for i in range(n)])
    label = order[:, 0].astype(np.int32)
    rows = np.arange(n)
    pe = _entropy(pbar)
    ee = pe.copy() if T == 1 else _entropy(p).mean(axis=0)
    mi = np.maximum(pe - ee, 0.0)
    votes = np.where(bad[None, :, None], 0.0, z32).argmax(axis=2)        # per-sample argmax of the fp32 z, first index on ties
    agreement = (votes == label[None, :]).sum(axis=0) / T
    prob_std = p[:, rows, label].std(axis=0)
    mean_prob = pbar[rows, label]
    if kind == 0:
        conf = mean_prob.copy()
    elif kind == 1:
        conf = 1.0 - pe / np.log(C) if C > 1 else np.ones(n)
    else:
        K = min(C, T)
        conf = 1.0 - mi / np.log(K) if K > 1 else np.ones(n)
    k = min(5, C)
    top_label = np.full((n, 5), -1, np.int32)
    top_prob = np.zeros((n, 5))
    top_label[:, :k] = order[:, :k]
    top_prob[:, :k] = np.take_along_axis(pbar, order[:, :k], axis=1)
    srt = np.take_along_axis(pbar, order[:, :min(6, C)], axis=1)
    label_ok = _gap_ok(srt[:, :2]).all(axis=1)
    top_ok = _gap_ok(srt).all(axis=1)
    nll = np.full(n, np.nan)
    brier = np.full(n, np.nan)
    if true_labels is not None:
        y = np.asarray(true_labels).astype(np.int64).ravel()
        ok = (y >= 0) & (y < C)
        yc = np.where(ok, y, 0)
        onehot = np.zeros((n, C))
        onehot[rows, yc] = 1.0
        nll = np.where(ok, -np.log(np.maximum(pbar[rows, yc], FLT_MIN)), np.nan)
        brier = np.where(ok, ((pbar - onehot) ** 2).sum(axis=1), np.nan)
    # the rule for non-finite frames
    nan = np.nan
    label = np.where(bad, 0, label).astype(np.int32)
    conf = np.where(bad, 0.0, conf)
    pbar = np.where(bad[:, None], nan, pbar)
    out = dict(nonfinite=bad, pbar=pbar, order=order, label=label, confidence=conf,
               fail=(bad | (conf < tau)).astype(np.uint8), score=np.clip(1.0 - conf, 0.0, 1.0),
               top_label=np.where(bad[:, None], -1, top_label).astype(np.int32), top_prob=np.where(bad[:, None], 0.0, top_prob),
               nll=np.where(bad, nan, nll), brier=np.where(bad, nan, brier),
               label_ok=label_ok | bad, top_ok=top_ok | bad, fail_ok=bad | (np.abs(conf - tau) > TIE_GAP))
    for name, v in (("mean_prob", mean_prob), ("prob_std", prob_std), ("pred_entropy", pe), ("expected_entropy", ee),
                    ("mutual_info", mi), ("agreement", agreement)):
        out[name] = np.where(bad, nan, v)
    return out


def sets_ref(r, score_kind="aps", lam=0.0, k_reg=0, qhat=np.inf, randomized=False, seed=0, first_index=0, true_labels=None):
    """The prediction sets of a heads_ref result r -> dict s [n, C] (score by class), rank [n, C], members bool[n, C], set_size,
    set_mass, u (as the record reports it: 0 under LAC), true_scores (s(y), NaN outside [0, C); NaN without labels).
    LAC s = 1 - pbar; APS s = u pbar + A + lam max(0, rank + 1 - k_reg), A the mass ahead in rank order.  A non-finite frame:
    every score NaN, no members."""
    pbar, order, bad = r["pbar"], r["order"], r["nonfinite"]
    n, C = pbar.shape
    rank = np.empty_like(order)
    np.put_along_axis(rank, order, np.arange(C)[None, :].repeat(n, 0), axis=1)
    if score_kind == "lac":
        s, u_rec = 1.0 - pbar, np.zeros(n)
    else:
        srt = np.take_along_axis(pbar, order, axis=1)
        ahead = np.concatenate([np.zeros((n, 1)), np.cumsum(srt, axis=1)[:, :-1]], axis=1)
        u_rec = draws(seed, first_index + np.arange(n)) if randomized else np.ones(n)
        s_rank = u_rec[:, None] * srt + ahead + lam * np.maximum(0, np.arange(C)[None, :] + 1 - k_reg)
        s = np.take_along_axis(s_rank, rank, axis=1)
    with np.errstate(invalid="ignore"):
        members = (s <= qhat) & ~bad[:, None]
    true_scores = np.full(n, np.nan)
    if true_labels is not None:
        y = np.asarray(true_labels).astype(np.int64).ravel()
        ok = (y >= 0) & (y < C)
        true_scores = np.where(ok, s[np.arange(n), np.where(ok, y, 0)], np.nan)
    return dict(s=s, rank=rank, members=members, set_size=members.sum(axis=1), u=u_rec,
                set_mass=np.where(members, np.nan_to_num(pbar), 0.0).sum(axis=1), true_scores=true_scores)


def rank_stable(r, y):
    """bool[n]: the frames where fp32 must give class y[i] the reference's rank (and hence the same classes ahead of it): no
    other class has a pbar within TIE_GAP of pbar[y], exact ties and pairs of device zeros (ordered by index on both sides)
    apart.  A RAPS score moves by lambda per rank, an APS score by the mass of whatever changes sides, so the calibration
    score s(y) is compared to the reference only on these frames.  Labels outside [0, C) and non-finite frames: True."""
    pbar = r["pbar"]
    n, C = pbar.shape
    y = np.asarray(y).astype(np.int64).ravel()
    out = np.ones(n, bool)
    for i in range(n):
        if r["nonfinite"][i] or not 0 <= y[i] < C:
            continue
        p, py = pbar[i], pbar[i, y[i]]
        near = (np.abs(p - py) <= TIE_GAP) & (p != py) & ~((p < ZERO_BELOW) & (py < ZERO_BELOW))
        out[i] = not near.any()
    return out


QHAT = 0.7321           # no multiple of 1 / C for any class count of the cases: flat rows' cumulative scores stay clear of it


def sets_configs(C):
    """The prediction-set configurations every case runs: keyword arguments of sets_ref."""
    out = [dict(score_kind="lac", qhat=QHAT), dict(score_kind="aps", qhat=QHAT),
           dict(score_kind="aps", qhat=np.inf), dict(score_kind="aps", qhat=-1.0),
           dict(score_kind="aps", qhat=QHAT, randomized=True, seed=3, first_index=11)]
    return out + [dict(score_kind="aps", qhat=0.8123, lam=0.01, k_reg=k) for k in (0, 1, C, C + 5)]


def members_comparable(r, s, qhat):
    """bool[n, C]: the classes whose reference membership the device must reproduce exactly on a RANDOM case - score further
    than SCORE_TOL from qhat, and not inside a run of near-tied pbar (consecutive gaps below TIE_GAP) that straddles the
    set's boundary (test_gpu_conformal.py's rule; an exact tie, or two device zeros, is ordered by index on both sides and ends
    a run)."""
    pbar, order = r["pbar"], r["order"]
    n, C = pbar.shape
    with np.errstate(invalid="ignore"):
        ok = np.abs(s - qhat) > SCORE_TOL
        member = s <= qhat
    for i in range(n):
        if r["nonfinite"][i]:
            ok[i] = True
            continue
        srt, m = pbar[i, order[i]], member[i, order[i]]
        g0 = 0
        for k in range(1, C + 1):
            if k == C or srt[k - 1] - srt[k] >= TIE_GAP or srt[k - 1] == srt[k] or srt[k - 1] < ZERO_BELOW:
                if m[g0:k].any() and not m[g0:k].all():
                    ok[i, order[i, g0:k]] = False
                g0 = k
    return ok


# ---- the inputs: every case is a dict name, logits fp32 [T, n, C], temperature, tau, labels int32[n], random (bool) ---------
TEMPERATURE, TAU = 1.3, 0.4
CLASS_COUNTS = (1, 2, 3, 4, 5, 255, 256, 257, 260, 1021, 1023, 1024)
SWEEP_FIVE = np.array([0.3, 0.9, 1.3, 2.7, 7.5], np.float32)        # K = 5: one group of 4 and one of 1


def _case(name, lg, random, temperature=TEMPERATURE, tau=TAU, seed=0):
    lg = np.ascontiguousarray(lg, np.float32)
    T, n, C = lg.shape
    y = np.random.default_rng(1000 + seed).integers(0, C, n).astype(np.int32)
    if n >= 4:
        y[-1], y[-2] = C, -1                                         # two labels outside [0, C)
    return dict(name=name, logits=lg, temperature=float(temperature), tau=float(tau), labels=y, random=random)


def gaussian(T, n, C, seed, scale=1.0, noise=1.5):
    """A frame's own class preferences (std 3) plus per-sample noise (std noise), times scale."""
    rng = np.random.default_rng(seed)
    return (scale * (rng.standard_normal((1, n, C)) * 3 + rng.standard_normal((T, n, C)) * noise)).astype(np.float32)


def ladder(T, n, C, seed, step=1.5, live=8, background=-25.0):
    """Logits without a near-tie, for the constructed cases (which are compared unfiltered): in every frame `live` classes
    at random places stand on a ladder, `step` apart, moved by up to a tenth of a step from sample to sample; every other
    class holds `background` in every sample, so those classes' pbar tie EXACTLY, in float64 as on the device (the same
    operations on the same values), and the lowest-index rule orders them on both sides."""
    rng = np.random.default_rng(seed)
    lg = np.full((T, n, C), background, np.float32)
    k = min(live, C)
    for i in range(n):
        cls = rng.choice(C, k, replace=False)
        lg[:, i, cls] = step * (k / 2.0 - np.arange(k))[None, :] + step * rng.uniform(-0.1, 0.1, (T, k))
    return lg


def class_count_cases():
    return [_case(f"C{C}_T{T}", gaussian(T, 16, C, 100 * C + T), True, seed=C + T) for C in CLASS_COUNTS for T in (1, 3, 30)]


def sample_count_cases():
    return [_case(f"T{T}_C10", gaussian(T, 2, 10, 7 + T), True, seed=T) for T in (1, 2, 3, 4, 5, 8, 4096)]


def sweep_staging_cases():
    """T around the sweep head's staging limit: 140 KB / row bytes = 35 rows at C = 1000 and at C = 1024."""
    return [_case(f"staging_C{C}_T{T}", gaussian(T, 2, C, C + T), True, seed=C + T) for C in (1000, 1024) for T in (34, 35, 36, 37)]


def temperature_cases():
    out = []
    for C, n, temps in ((10, 2, (0.01, 0.05, 1.0, 20.0, 1e4)), (1000, 2, (0.01, 0.05, 1.0)), (1000, 1, (20.0, 1e4))):
        for temp in temps:
            for scale in (4.0, 40.0):
                lg = gaussian(3, n, C, int(C + scale), scale=scale / 3.0, noise=0.3)      # class preferences of std scale, |z| up to thousands
                out.append(_case(f"temp{temp:g}_x{scale:g}_C{C}", lg, True, temperature=temp, seed=C))
    return out


def random_cases():
    return class_count_cases() + sample_count_cases() + sweep_staging_cases() + temperature_cases()


SAT_LEAD = 170.0        # > 104 * TEMPERATURE = 135.2: every other exponential is exactly 0 in fp32 (and below ZERO_BELOW in float64)


def saturated_cases():
    """One class leads every other by SAT_LEAD in every sample.  'agree': the same winner in every sample (labels: even
    frames carry the winner, odd frames a wrong class).  'split': T = 4, winners a, b, a, b - pbar ties at exactly 0.5."""
    out = []
    for C, T in ((10, 1), (10, 4), (1000, 4), (256, 3), (257, 3)):
        rng = np.random.default_rng(C + T)
        n = 6
        lg = rng.standard_normal((T, n, C)).astype(np.float32)
        win = rng.integers(0, C, n)
        for i in range(n):
            lg[:, i, win[i]] = lg[:, i, :].max() + SAT_LEAD
        c = _case(f"saturated_agree_C{C}_T{T}", lg, False)
        c["winner"] = win
        c["labels"] = np.where(np.arange(n) % 2 == 0, win, (win + 1) % C).astype(np.int32)
        out.append(c)
    for C in (10, 1000):
        rng = np.random.default_rng(C)
        n = 4
        lg = rng.standard_normal((4, n, C)).astype(np.float32)
        a = np.array([7, 0, C - 1, 3])
        b = np.array([2, C - 1, 4, 8])
        for i in range(n):
            top = lg[:, i, :].max() + SAT_LEAD
            lg[0::2, i, a[i]] = top
            lg[1::2, i, b[i]] = top
        c = _case(f"saturated_split_C{C}", lg, False)
        c["winner"] = np.minimum(a, b)
        c["other"] = np.maximum(a, b)
        out.append(c)
    return out


def flat_cases():
    out = []
    for C in (10, 256, 257, 1000):
        for T in (1, 3):
            lg = np.zeros((T, 3, C), np.float32)
            lg[:, 1, :] = 1e4
            lg[:, 2, :] = -1e4
            out.append(_case(f"flat_C{C}_T{T}", lg, False))
    return out


def masked_cases():
    """-inf in the same classes of every sample ('same': the case carries mask bool[C]), in only three classes kept
    ('few': the masked classes reach the top-5), and in some samples only ('some': ordinary finite input)."""
    out = []
    for C, seed in ((10, 1), (1000, 2), (257, 3)):
        rng = np.random.default_rng(seed)
        mask = rng.random(C) < 0.3
        mask[0] = True
        mask[C - 1] = True
        lg = ladder(3, 6, C, 50 + seed, background=-400.0)    # exact zeros on the device, like the masked classes
        lg[:, :, mask] = -np.inf
        c = _case(f"masked_same_C{C}", lg, False)
        c["mask"] = mask
        out.append(c)
    for C in (10, 1000):
        mask = np.ones(C, bool)
        mask[[2, 5, C - 2]] = False
        lg = gaussian(3, 4, C, 60 + C)
        lg[:, :, mask] = -np.inf
        c = _case(f"masked_few_C{C}", lg, False)
        c["mask"] = mask
        out.append(c)
    for C in (10, 1000):
        lg = ladder(4, 6, C, 70 + C, background=-400.0)      # background: exact zeros on the device whatever is masked
        rng = np.random.default_rng(C)
        lg[0][:, rng.random(C) < 0.5] = -np.inf
        lg[2][:, rng.random(C) < 0.2] = -np.inf
        out.append(_case(f"masked_some_C{C}", lg, False))
    return out


def nonfinite_cases():
    """Six frames, three of them bad: frame 1 has a NaN in one class of one sample, frame 3 a +inf, frame 4 one sample's
    whole row at -inf.  Frames 0, 2 and 5 are ordinary (the case carries good = [0, 2, 5])."""
    out = []
    for C in (10, 1000):
        for T in (1, 7):
            lg = ladder(T, 6, C, 90 + C + T)
            lg[T // 2, 1, C // 3] = np.nan
            lg[T - 1, 3, C - 1] = np.inf
            lg[T // 3, 4, :] = -np.inf
            c = _case(f"nonfinite_C{C}_T{T}", lg, False)
            c["good"] = np.array([0, 2, 5])
            out.append(c)
    return out


def overflow_cases():
    """Finite logits that overflow when scaled: 3e38 at temperature 0.5 (z = +inf: frames 0 and 2 are non-finite), and
    -3e38 (z = -inf: a masked class, frame 1 stays finite)."""
    out = []
    for C in (10, 1000):
        for T in (1, 7):
            lg = ladder(T, 4, C, 95 + C + T, step=0.75, background=-400.0)    # device zeros, like the class at -3e38
            lg[:, 0, C // 2] = 3e38
            lg[T - 1, 2, 0] = 3e38
            lg[:, 1, 1] = -3e38
            c = _case(f"overflow_C{C}_T{T}", lg, False, temperature=0.5)
            c["good"] = np.array([1, 3])
            out.append(c)
    return out


def constructed_cases():
    return saturated_cases() + flat_cases() + masked_cases() + nonfinite_cases() + overflow_cases()
