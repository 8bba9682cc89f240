"""numpy restatement of the feature-space OOD contract (include/fav.h beside fav_ood_record),
written from the contract alone: every step one numpy float32 operation, hence one rounding, in the contract's order.  A
float32 ufunc rounds each element's result once and never fuses a product into a sum, so `g = g + P[:, j] * x[:, j]` is the
contract's `g = g + P[r][j] * x[j]` for every (frame, r) at once.  Plus the float64 fit, restated from its definition."""
import numpy as np

NAN = np.float32(np.nan)


def bf16_to_f32(bits):
    """uint16 bf16 bit patterns -> float32."""
    return (np.asarray(bits, np.uint16).astype(np.uint32) << 16).view(np.float32)


def f32_to_bf16_bits(x):
    """float32 -> bf16 bit patterns, round to nearest even (finite values and infinities; a NaN stays a NaN)."""
    u = np.ascontiguousarray(x, np.float32).view(np.uint32)
    r = ((u + 0x7FFF + ((u >> 16) & 1)) >> 16).astype(np.uint16)
    nan = np.isnan(x)
    r[nan] = ((u[nan] >> 16) | 0x40).astype(np.uint16)
    return r


def distances(feat, mu, P, M):
    """feat float32 [S, n, D] -> (g float32 [n, k], d float32 [n, R]): steps 1 - 4."""
    feat = np.asarray(feat, np.float32)
    mu, P, M = (np.asarray(a, np.float32) for a in (mu, P, M))
    S, n, D = feat.shape
    k, R = P.shape[0], M.shape[0]
    with np.errstate(all="ignore"):
        fbar = np.zeros((n, D), np.float32)
        for s in range(S):
            fbar = fbar + feat[s]
        fbar = fbar * np.float32(1.0 / S)
        x = fbar - mu[None, :]
        g = np.zeros((n, k), np.float32)
        for j in range(D):
            g = g + P[None, :, j] * x[:, j, None]
        d = np.zeros((n, R), np.float32)
        for r in range(k):
            t = g[:, r, None] - M[None, :, r]
            d = d + t * t
    assert g.dtype == np.float32 and d.dtype == np.float32
    return g, d


def select(d, class_id, labels, threshold):
    """d float32 [n, R] -> dict min_dist, min_class, label_dist, ood: steps 5 - 7, the serial scan as written."""
    n, R = d.shape
    class_id = np.asarray(class_id, np.int32)
    best = np.full(n, np.inf, np.float32)
    row = np.full(n, -1, np.int64)
    for c in range(R):
        m = d[:, c] < best                     # False for a NaN: it never wins
        best[m] = d[m, c]
        row[m] = c
    min_class = np.where(row < 0, -1, class_id[np.maximum(row, 0)]).astype(np.int32)
    label_dist = np.full(n, NAN, np.float32)
    if labels is not None:
        for i, y in enumerate(np.asarray(labels).ravel()):
            rows = np.flatnonzero(class_id == y)
            if rows.size:
                label_dist[i] = d[i, rows[0]]
    with np.errstate(invalid="ignore"):
        ood = (~(best <= np.float32(threshold))).astype(np.int32)
    return dict(min_dist=best, min_class=min_class, label_dist=label_dist, ood=ood)


def score(feat_bits, mu, P, M, class_id, labels, threshold):
    """The whole head on bf16 bit patterns [S, n, D] (uint16)."""
    _, d = distances(bf16_to_f32(feat_bits), mu, P, M)
    return select(d, class_id, labels, threshold)


def records(out):
    """The dict of `select` as int32 [n, 4] fav_ood_record dwords, every NaN the canonical one (so that NaN equals NaN)."""
    rec = np.zeros((out["min_dist"].shape[0], 4), np.int32)
    rec[:, 0] = canon(out["min_dist"]).view(np.int32)
    rec[:, 1] = out["min_class"]
    rec[:, 2] = canon(out["label_dist"]).view(np.int32)
    rec[:, 3] = out["ood"]
    return rec


def canon(x):
    x = np.array(x, np.float32)
    x[np.isnan(x)] = NAN
    return x


def canon_records(rec):
    """Device records int32 [n, 4] with their NaNs made canonical."""
    rec = np.array(rec, np.int32)
    for col in (0, 2):
        rec[:, col] = canon(rec[:, col].view(np.float32)).view(np.int32)
    return rec


# ---- the fit, float64
def fit64(F, y, k=None, shrinkage=0.01):
    """-> dict mu [D], means [R, D], classes [R], Sigma [D, D] (the shrunk tied covariance), P [k, D], M [R, k], float64."""
    F = np.asarray(F, np.float64)
    y = np.asarray(y).ravel()
    N, D = F.shape
    k = D if k is None else k
    mu = F.sum(axis=0) / N
    classes = np.array(sorted(set(y.tolist())))
    means = np.stack([F[y == c].sum(axis=0) / (y == c).sum() for c in classes])
    S = np.zeros((D, D))
    for c, m in zip(classes, means):
        Z = F[y == c] - m
        S += Z.T @ Z
    S /= N
    Sigma = (1.0 - shrinkage) * S + shrinkage * (np.trace(S) / D) * np.eye(D)
    lam, U = np.linalg.eigh(Sigma)
    lam, U = lam[::-1][:k], U[:, ::-1][:, :k]
    P = (U * lam ** -0.5).T
    return dict(mu=mu, means=means, classes=classes, Sigma=Sigma, P=P, M=(means - mu) @ P.T)


def mahalanobis64(f, means, Sigma):
    """f [n, D] -> (f - mu_c)^T Sigma^-1 (f - mu_c), float64 [n, R], through np.linalg.inv."""
    inv = np.linalg.inv(Sigma)
    z = np.asarray(f, np.float64)[:, None, :] - means[None, :, :]
    return np.einsum("ncd,de,nce->nc", z, inv, z)


def auroc(id_scores, ood_scores):
    """Mann-Whitney by the definition: pairs, ties 1/2."""
    a, b = np.asarray(id_scores, np.float64)[:, None], np.asarray(ood_scores, np.float64)[None, :]
    return float(((b > a).sum() + 0.5 * (b == a).sum()) / (a.size * b.size))
