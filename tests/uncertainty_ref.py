"""float64 reference of the uncertainty head (include/fav.h fav_uncertainty), written for the
tests from the definitions alone: z_t = fp32(logit_t * fp32(1 / temperature)), p_t = softmax(z_t) in float64, pbar = mean_t p_t."""
import numpy as np

FLOAT_FIELDS = ("confidence", "mean_prob", "prob_std", "pred_entropy", "expected_entropy", "mutual_info", "agreement")


def _entropy(q, axis=-1):
    with np.errstate(divide="ignore", invalid="ignore"):
        t = np.where(q > 0, q * np.log(np.where(q > 0, q, 1.0)), 0.0)
    return -t.sum(axis=axis)


def head_uncertainty(logits, temperature=1.0, kind=0, tau=0.5):
    """logits fp32 [T, n, C] -> dict of per-frame fields (float64 where fp32 on the device), fail / score, and two gaps
    of pbar for tests that must tell a near-tie from an error: ``gap`` (top-1 minus top-2) and ``top_gap`` (the smallest
    gap between consecutive ranks among the top 6)."""
    lg = np.asarray(logits, np.float32)
    T, n, C = lg.shape
    inv = np.float32(1.0) / np.float32(temperature)
    z = lg * inv                                           # fp32, as the kernel scales
    z64 = z.astype(np.float64)
    e = np.exp(z64 - z64.max(axis=2, keepdims=True))
    p = e / e.sum(axis=2, keepdims=True)                   # [T, n, C]
    pbar = p.mean(axis=0)                                  # [n, C]
    idx = np.arange(C)
    order = np.stack([np.lexsort((idx, -pbar[i])) for i in range(n)])   # descending, lowest index first on ties
    label = order[:, 0].astype(np.int32)
    pe = _entropy(pbar)
    ee = _entropy(p).mean(axis=0)
    mi = np.maximum(pe - ee, 0.0)
    votes = z.argmax(axis=2)                               # per-sample argmax of the scaled fp32 z, first index on ties
    agreement = (votes == label[None, :]).sum(axis=0) / T
    pl = p[:, np.arange(n), label]                         # [T, n]
    prob_std = pl.std(axis=0)
    mean_prob = pbar[np.arange(n), label]
    if kind == 0:
        conf = mean_prob
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
    top_gap = np.diff(-srt, axis=1).min(axis=1) if srt.shape[1] > 1 else np.full(n, np.inf)
    gap = srt[:, 0] - srt[:, 1] if srt.shape[1] > 1 else np.full(n, np.inf)
    return dict(label=label, confidence=conf, mean_prob=mean_prob, prob_std=prob_std, pred_entropy=pe, expected_entropy=ee,
                mutual_info=mi, agreement=agreement, top_label=top_label, top_prob=top_prob,
                fail=(conf < tau).astype(np.uint8), score=np.clip(1.0 - conf, 0.0, 1.0), gap=gap, top_gap=top_gap)


def pack_records(fields):
    """dict of per-frame fields -> int32[n, 18] records in the fav_uncertainty layout (floats rounded to fp32, bit-cast)."""
    n = len(fields["label"])
    rec = np.zeros((n, 18), np.int32)
    rec[:, 0] = np.asarray(fields["label"], np.int32)
    for i, name in enumerate(FLOAT_FIELDS, start=1):
        rec[:, i] = np.asarray(fields[name], np.float32).view(np.int32)
    rec[:, 8:13] = np.asarray(fields["top_label"], np.int32)
    rec[:, 13:18] = np.ascontiguousarray(np.asarray(fields["top_prob"], np.float32)).view(np.int32)
    return rec
