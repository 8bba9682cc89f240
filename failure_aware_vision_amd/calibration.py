"""Host side of temperature / tau calibration (include/fav.h fav_calib_cell).

The per-frame work - the confidence head at K trial temperatures, the negative log-likelihood and Brier score of every
frame at each of them - happens in one launch of the sweep head (fav_classify_sweep / fav_op_head_sweep).  What is left
for the host is small and lives here, numpy only: the grid search that fits the temperature on the mean NLL, the metrics
that show what the confidence is worth (ECE / MCE, the risk-coverage curve and its area), and the choice of the failure
threshold tau for a target selective risk, empirically or with the exact binomial guarantee of Geifman and El-Yaniv
("Selective classification for deep neural networks", NeurIPS 2017).  Importing this module needs no GPU.

Order of calibration: the temperature first, then tau and the conformal qhat - both depend on pbar, hence on the
temperature."""
from __future__ import annotations

import dataclasses
import math

import numpy as np

#: dwords of one fav_calib_cell (include/fav.h): label, confidence, nll, brier
CELL_DWORDS = 4
#: FAV_SWEEP_MAX_TEMPS
MAX_TEMPS = 32


def unpack_cells(cells) -> dict:
    """int32[n, K, 4] fav_calib_cell records (numpy, or a torch tensor on any device) -> dict of views ``label``
    int32[n, K], ``confidence`` / ``nll`` / ``brier`` fp32[n, K] (bit-cast).  Nothing is copied."""
    if cells.ndim != 3 or int(cells.shape[2]) != CELL_DWORDS:
        raise ValueError(f"expected int32[n, K, {CELL_DWORDS}] cells, got shape {tuple(cells.shape)}")
    if isinstance(cells, np.ndarray):
        if cells.dtype != np.int32:
            raise TypeError(f"cells must be int32, got {cells.dtype}")
        f32 = np.float32
    else:
        import torch
        if cells.dtype != torch.int32:
            raise TypeError(f"cells must be int32, got {cells.dtype}")
        f32 = torch.float32
    return {"label": cells[:, :, 0], "confidence": cells[:, :, 1].view(f32), "nll": cells[:, :, 2].view(f32),
            "brier": cells[:, :, 3].view(f32)}


def temperature_grid(lo: float, hi: float, K: int = MAX_TEMPS) -> np.ndarray:
    """K temperatures spaced evenly in ln t from lo to hi: fp32(lo * (hi / lo) ** (k / (K - 1))), computed in float64."""
    lo, hi, K = float(lo), float(hi), int(K)
    if not (math.isfinite(lo) and math.isfinite(hi) and 0.0 < lo <= hi):
        raise ValueError(f"need 0 < lo <= hi, both finite; got lo={lo}, hi={hi}")
    if not 1 <= K <= MAX_TEMPS:
        raise ValueError(f"K must be in [1, {MAX_TEMPS}], got {K}")
    if K == 1:
        return np.array([lo], np.float32)
    return (lo * (hi / lo) ** (np.arange(K, dtype=np.float64) / (K - 1))).astype(np.float32)


@dataclasses.dataclass(frozen=True)
class TemperatureFit:
    temperature: float      #: the fitted temperature (an fp32 value)
    nll: float              #: its mean NLL
    at_bound: bool          #: the minimum sits on ``lo`` or ``hi``: the true minimum may lie outside the range
    rounds: int             #: grids evaluated


def fit_temperature(nll_of, lo: float = 0.25, hi: float = 8.0, K: int = MAX_TEMPS, rtol: float = 1e-3,
                    max_rounds: int = 6) -> TemperatureFit:
    """Minimise the mean NLL over the temperature by repeated grid refinement.  ``nll_of(temps fp32[K]) -> float64[K]``.

    1. evaluate ``temperature_grid(lo, hi, K)`` and take the argmin k*, lowest index on ties;
    2. the next grid spans [t[k* - 1], t[k* + 1]], clipped to the ends of the current one;
    3. stop when t[k* + 1] / t[k* - 1] <= 1 + rtol, or after max_rounds grids.

    With the defaults that is 3 grids: the step ratio goes 1.118, 1.0072, 1.00047."""
    K = int(K)
    if K < 3:
        raise ValueError("fit_temperature needs K >= 3 (a bracket around the minimum)")
    if int(max_rounds) < 1:
        raise ValueError("max_rounds must be >= 1")
    lo0, hi0 = np.float32(lo), np.float32(hi)
    rounds = 0
    while True:
        t = temperature_grid(lo, hi, K)
        v = np.asarray(nll_of(t), np.float64)
        rounds += 1
        if v.shape != (K,) or np.isnan(v).any():
            raise ValueError("nll_of must return K values, none NaN (a label outside [0, num_classes), or a non-finite frame?)")
        k = int(np.argmin(v))                       # the first of equal minima
        a, b = float(t[max(k - 1, 0)]), float(t[min(k + 1, K - 1)])
        if b / a <= 1.0 + rtol or rounds >= max_rounds:
            best = float(t[k])
            return TemperatureFit(best, float(v[k]), bool(best <= lo0 or best >= hi0), rounds)
        lo, hi = a, b


def _as_conf_correct(conf, correct):
    conf = np.asarray(conf, np.float32).ravel()
    correct = np.asarray(correct).astype(bool).ravel()
    if conf.shape != correct.shape or conf.size == 0:
        raise ValueError("conf and correct must be non-empty and of one length")
    if np.isnan(conf).any():
        raise ValueError("conf holds NaN")
    return conf, correct


def reliability(conf, correct, bins: int = 15) -> dict:
    """Reliability of the confidence as a probability of being right: ``bins`` equal-width bins on [0, 1] (bin b holds
    b / bins <= conf < (b + 1) / bins, conf = 1 in the last; values outside [0, 1] go to the end bins) ->
    ``ece`` = sum_b (count_b / n) |acc_b - conf_b|, ``mce`` = max_b over the non-empty bins, and per bin ``count``,
    ``mean_conf``, ``accuracy`` (NaN where empty)."""
    conf, correct = _as_conf_correct(conf, correct)
    bins = int(bins)
    idx = np.clip(np.floor(conf.astype(np.float64) * bins), 0, bins - 1).astype(np.int64)
    count = np.bincount(idx, minlength=bins)
    sc = np.bincount(idx, weights=conf.astype(np.float64), minlength=bins)
    sa = np.bincount(idx, weights=correct.astype(np.float64), minlength=bins)
    full = count > 0
    mean_conf = np.full(bins, np.nan)
    acc = np.full(bins, np.nan)
    mean_conf[full] = sc[full] / count[full]
    acc[full] = sa[full] / count[full]
    gap = np.abs(acc[full] - mean_conf[full])
    return {"ece": float((count[full] / conf.size * gap).sum()), "mce": float(gap.max()), "count": count,
            "mean_conf": mean_conf, "accuracy": acc}


def risk_coverage(conf, correct) -> dict:
    """The selective classifier {accept iff conf >= t} at every distinct observed confidence t, highest first:
    ``threshold`` fp32, ``coverage`` = accepted / n, ``risk`` = errors among the accepted / accepted, ``accepted`` /
    ``errors`` (the integer counts behind them), and ``aurc``, the area under risk over coverage as a step function
    (sum_i risk_i (coverage_i - coverage_{i-1}), coverage_0 = 0; without ties this is the usual mean of the n prefix risks)."""
    conf, correct = _as_conf_correct(conf, correct)
    order = np.argsort(-conf.astype(np.float64), kind="stable")
    c, wrong = conf[order], ~correct[order]
    last = np.flatnonzero(np.append(c[1:] != c[:-1], True))      # last frame of every run of equal confidences
    accepted = (last + 1).astype(np.float64)
    errors = np.cumsum(wrong)[last].astype(np.float64)
    coverage = accepted / conf.size
    risk = errors / accepted
    aurc = float((risk * np.diff(np.concatenate([[0.0], coverage]))).sum())
    return {"threshold": c[last], "coverage": coverage, "risk": risk, "aurc": aurc,
            "accepted": (last + 1).astype(np.int64), "errors": np.cumsum(wrong)[last].astype(np.int64)}


def _log_binom_cdf(e: int, m: int, b: float) -> float:
    """ln P[Bin(m, b) <= e], 0 < b < 1, in log space."""
    lb, l1b = math.log(b), math.log1p(-b)
    terms = [math.lgamma(m + 1) - math.lgamma(j + 1) - math.lgamma(m - j + 1) + j * lb + (m - j) * l1b for j in range(e + 1)]
    mx = max(terms)
    return mx + math.log(sum(math.exp(x - mx) for x in terms))


def binomial_upper_bound(errors: int, m: int, level: float) -> float:
    """The exact (Clopper-Pearson) upper confidence bound on a binomial proportion: the b with
    P[Bin(m, b) <= errors] = level; 1 when errors = m.  The true risk exceeds it with probability at most ``level``."""
    errors, m = int(errors), int(m)
    if not (0 <= errors <= m and m >= 1 and 0.0 < level < 1.0):
        raise ValueError("need 0 <= errors <= m, m >= 1, 0 < level < 1")
    if errors == m:
        return 1.0
    lo, hi, target = errors / m, 1.0, math.log(level)
    for _ in range(200):                            # the CDF falls as b grows
        mid = 0.5 * (lo + hi)
        if mid <= lo or mid >= hi:
            break
        if _log_binom_cdf(errors, m, mid) > target:
            lo = mid
        else:
            hi = mid
    return 0.5 * (lo + hi)


def tau_for_risk(conf, correct, target_risk: float, delta: float | None = None) -> dict:
    """The failure threshold for a target selective risk: among the observed fp32 confidences, the smallest tau whose
    accepted set {conf >= tau} has risk <= target_risk -> dict ``tau``, ``coverage``, ``risk`` (empirical, of that set)
    and ``bound``.  tau is an observed fp32 confidence, so ``conf < tau`` on the device splits the calibration frames
    exactly as here.

    delta = None: the empirical risk decides (every distinct confidence is tried); ``bound`` = ``risk``.
    delta given: selection with guaranteed risk (Geifman and El-Yaniv 2017): a bisection over the sorted distinct
    confidences of at most k = ceil(log2 n) candidates, each accepted when its Clopper-Pearson upper bound at level
    delta / k is <= target_risk; by the union bound the true risk of the returned classifier exceeds ``bound`` with
    probability at most delta.

    No candidate qualifies: tau = +inf, coverage 0 (risk and bound NaN)."""
    conf, correct = _as_conf_correct(conf, correct)
    target_risk = float(target_risk)
    rc = risk_coverage(conf, correct)
    th, cov, risk = rc["threshold"][::-1], rc["coverage"][::-1], rc["risk"][::-1]      # ascending thresholds
    accepted, errors = rc["accepted"][::-1], rc["errors"][::-1]
    none = {"tau": math.inf, "coverage": 0.0, "risk": math.nan, "bound": math.nan}
    if delta is None:
        ok = np.flatnonzero(risk <= target_risk)
        if ok.size == 0:
            return none
        i = int(ok[0])
        return {"tau": float(th[i]), "coverage": float(cov[i]), "risk": float(risk[i]), "bound": float(risk[i])}
    if not 0.0 < float(delta) < 1.0:
        raise ValueError("delta must be in (0, 1)")
    n = conf.size
    k = max(1, math.ceil(math.log2(n)))
    lo, hi, best = 0, th.size - 1, none
    for _ in range(k):
        if lo > hi:
            break
        mid = (lo + hi) // 2
        b = binomial_upper_bound(int(errors[mid]), int(accepted[mid]), float(delta) / k)
        if b <= target_risk:
            best = {"tau": float(th[mid]), "coverage": float(cov[mid]), "risk": float(risk[mid]), "bound": b}
            hi = mid - 1                            # a lower threshold covers more
        else:
            lo = mid + 1
    return best


@dataclasses.dataclass(frozen=True)
class Calibration:
    """What calibration fixes: apply with ``Backend.apply``.  ``metrics``: whatever the caller measured on the way."""
    temperature: float
    tau: float
    metrics: dict = dataclasses.field(default_factory=dict)


def report_from_cells(cells, labels) -> dict:
    """The metrics of one temperature from its cells (int32[n, 1, 4] or one column of a sweep, numpy) and the true labels:
    accuracy, mean confidence, mean NLL, mean Brier score (float64 sums), ECE, MCE, AURC."""
    c = unpack_cells(np.ascontiguousarray(cells))
    if c["label"].shape[1] != 1:
        raise ValueError("one temperature: cells int32[n, 1, 4]")
    correct = c["label"][:, 0] == np.asarray(labels).ravel()
    conf = c["confidence"][:, 0]
    rel = reliability(conf, correct)
    return {"accuracy": float(correct.mean()), "mean_confidence": float(conf.astype(np.float64).mean()),
            "nll": float(c["nll"][:, 0].astype(np.float64).mean()), "brier": float(c["brier"][:, 0].astype(np.float64).mean()),
            "ece": rel["ece"], "mce": rel["mce"], "aurc": risk_coverage(conf, correct)["aurc"]}
