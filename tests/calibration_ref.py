"""float64 reference of the temperature-sweep head (include/fav.h fav_calib_cell), written
for the tests from the definitions alone: z_t = float64(logit_t) * float64(fp32(1 / temperature)), p_t = softmax(z_t),
pbar = mean_t p_t; label = argmax pbar (lowest index on ties); confidence by kind (0: max pbar, 1: 1 - H(pbar) / ln C,
2: 1 - max(H(pbar) - mean_t H(p_t), 0) / ln min(C, T)); nll = -ln max(pbar[y], FLT_MIN);
brier = sum_c (pbar[c] - [c == y])^2; y outside [0, C): nll = brier = NaN."""
import numpy as np

FLT_MIN = float(np.finfo(np.float32).tiny)


def _entropy(p, axis):
    with np.errstate(divide="ignore", invalid="ignore"):
        return -np.where(p > 0, p * np.log(p), 0.0).sum(axis=axis)


def cells_of(logits, labels, temperature, kind=0):
    """logits [T, n, C] (any padding columns already cut), labels int[n] -> dict of float64[n] label / confidence / nll / brier."""
    lg = np.asarray(logits, np.float32).astype(np.float64)
    T, n, C = lg.shape
    z = lg * np.float64(np.float32(1.0) / np.float32(temperature))
    e = np.exp(z - z.max(axis=2, keepdims=True))
    pt = e / e.sum(axis=2, keepdims=True)
    pb = pt.mean(axis=0)
    label = pb.argmax(axis=1)
    if kind == 0:
        conf = pb.max(axis=1)
    else:
        hh = _entropy(pb, 1)
        if kind == 1:
            conf = 1.0 - hh / np.log(C) if C > 1 else np.ones(n)
        else:
            mi = np.maximum(hh - _entropy(pt, 2).mean(axis=0), 0.0)
            conf = 1.0 - mi / np.log(min(C, T)) if min(C, T) > 1 else np.ones(n)
    y = np.asarray(labels).astype(np.int64).ravel()
    ok = (y >= 0) & (y < C)
    yc = np.where(ok, y, 0)
    py = pb[np.arange(n), yc]
    onehot = np.zeros((n, C))
    onehot[np.arange(n), yc] = 1.0
    nll = np.where(ok, -np.log(np.maximum(py, FLT_MIN)), np.nan)
    brier = np.where(ok, ((pb - onehot) ** 2).sum(axis=1), np.nan)
    return {"label": label, "confidence": conf, "nll": nll, "brier": brier}


def sweep_of(logits, labels, temps, kind=0):
    """-> dict of float64[n, K]."""
    cols = [cells_of(logits, labels, t, kind) for t in np.asarray(temps, np.float32)]
    return {k: np.stack([c[k] for c in cols], axis=1) for k in cols[0]}


def mean_nll_of(logits, labels):
    """-> nll_of(temps) for calibration.fit_temperature, in float64."""
    return lambda temps: sweep_of(logits, labels, temps)["nll"].mean(axis=0)


def error_measure(dev, ref):
    """|dev - ref| / max(1, |ref|), elementwise."""
    dev, ref = np.asarray(dev, np.float64), np.asarray(ref, np.float64)
    return np.abs(dev - ref) / np.maximum(1.0, np.abs(ref))


def fit_case(T, n, C, scale, seed):
    """Synthetic logits with a known best temperature: base ~ N(0, 2^2)[n, C], labels drawn from softmax(base),
    logits[t] = scale * (base + N(0, 0.3^2)) -> (logits fp32 [T, n, C], labels int32[n])."""
    rng = np.random.default_rng(seed)
    base = rng.standard_normal((n, C)) * 2.0
    p = np.exp(base - base.max(axis=1, keepdims=True))
    p /= p.sum(axis=1, keepdims=True)
    labels = np.array([rng.choice(C, p=p[i]) for i in range(n)], np.int32)
    logits = (scale * (base[None] + rng.standard_normal((T, n, C)) * 0.3)).astype(np.float32)
    return logits, labels
