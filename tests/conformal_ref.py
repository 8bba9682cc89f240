"""float64 reference of the conformal prediction-set head (include/fav.h fav_conformal / fav_pred_set; DESIGN.md section 2,
item 5b), written for the tests from the definitions alone: z_t = fp32(logit_t * fp32(1 / temperature)),
p_t = softmax(z_t) in float64, pbar = mean_t p_t; classes ranked by pbar descending, lowest index first on ties;
A = mass ahead in rank order; LAC s = 1 - pbar, APS s = u pbar + A + lambda max(0, rank + 1 - k_reg); member iff s <= qhat.
u is the Philox4x32-10 draw of the contract (oracle.fav_oracle.philox4x32_10, counter (0, frame, 0, 0xC0F0))."""
import math

import numpy as np

from oracle.fav_oracle import philox4x32_10

SITE = 0xC0F0


def pbar_of(logits, temperature=1.0):
    lg = np.asarray(logits, np.float32)
    z = (lg * (np.float32(1.0) / np.float32(temperature))).astype(np.float64)
    e = np.exp(z - z.max(axis=2, keepdims=True))
    return (e / e.sum(axis=2, keepdims=True)).mean(axis=0)          # [n, C]


def sort_order(pbar):
    idx = np.arange(pbar.shape[1])
    return np.stack([np.lexsort((idx, -row)) for row in pbar])       # [n, C]: rank -> class


def draws(seed, frames):
    """u of the global frames (uint32 array-like)."""
    seed = int(seed)
    x0 = philox4x32_10(0, np.asarray(frames, np.uint32), 0, SITE, seed & 0xFFFFFFFF, seed >> 32)[0]
    return (x0 >> np.uint32(8)).astype(np.float64) * 2.0 ** -24


def scores(pbar, kind="aps", randomized=False, lam=0.0, k_reg=0, seed=0, first_index=0):
    """-> (s [n, C] by class, u [n], order [n, C], rank [n, C] by class)."""
    n, C = pbar.shape
    order = sort_order(pbar)
    rank = np.empty_like(order)
    np.put_along_axis(rank, order, np.arange(C)[None, :].repeat(n, 0), axis=1)
    if kind == "lac":
        return 1.0 - pbar, np.zeros(n), order, rank
    srt = np.take_along_axis(pbar, order, axis=1)
    ahead = np.concatenate([np.zeros((n, 1)), np.cumsum(srt, axis=1)[:, :-1]], axis=1)   # by rank
    u = draws(seed, first_index + np.arange(n)) if randomized else np.ones(n)
    s_rank = u[:, None] * srt + ahead + lam * np.maximum(0, np.arange(C)[None, :] + 1 - k_reg)
    return np.take_along_axis(s_rank, rank, axis=1), u, order, rank


def prediction_sets(s, qhat):
    """Boolean [n, C] membership s <= qhat."""
    return s <= qhat


def qhat_of(cal_scores, alpha):
    n = len(cal_scores)
    k = math.ceil((n + 1) * (1 - alpha))
    return math.inf if k > n else float(np.sort(cal_scores)[k - 1])
