"""numpy restatement of the drift-test contract (include/fav.h beside fav_drift_record), written
from the contract alone: step 1 is knn_ref.query, step 3 the oracle's bit-exact model of the production GEMM, step 4 one numpy
float32 operation, hence one rounding, per contract operation, steps 5 and 7 Python integers, step 6 the oracle's Philox and a
sort of the 64-bit keys, step 8 numpy float64."""
import numpy as np

import knn_ref as K
from oracle import fav_oracle as O

NAN64_BITS = 0x7FF8000000000000
NAN32_BITS = 0x7FC00000
SALT = 0x5F17


def similarities(pool):
    """pool float32 [Np, D] holding bf16 values -> G float32 [Np, Np]; only j <= i is the contract's (step 3)."""
    return O.gemm_acc(pool, pool, "mfma") + np.float32(0)


def quantise(G):
    """G [Np, Np] -> u int64 [Np, Np], symmetric with a zero diagonal, from the lower triangle of G alone (step 4)."""
    G = np.asarray(G, np.float32)
    L = np.tril(G)
    Gl = L + np.tril(G, -1).T                                            # G[i][j] of j <= i on both sides
    g = np.diagonal(G).copy()
    hi, lo = np.maximum.outer(np.arange(len(g)), np.arange(len(g))), np.minimum.outer(np.arange(len(g)), np.arange(len(g)))
    d2 = np.maximum((g[hi] + g[lo]) - np.float32(2.0) * Gl, np.float32(0.0))
    assert d2.dtype == np.float32
    dd = np.sqrt(d2.astype(np.float64)).astype(np.float32)               # correctly rounded: 53 >= 2 * 24 + 2
    assert np.array_equal(dd, np.sqrt(d2))
    u = np.rint(dd * np.float32(1048576.0)).astype(np.int64)
    np.fill_diagonal(u, 0)
    assert np.array_equal(u, u.T)
    return u


def keys(Np, P, seed):
    """-> uint64 [P, Np]: key(i) of every permutation (step 6)."""
    i, p = np.meshgrid(np.arange(Np, dtype=np.uint32), np.arange(P, dtype=np.uint32))
    x0 = O.philox4x32_10(i, p, 0, SALT, seed & 0xFFFFFFFF, (seed >> 32) & 0xFFFFFFFF)[0]
    return (x0.astype(np.uint64) << np.uint64(32)) | i.astype(np.uint64)


def group_of(key_row, n):
    """The n pool indices with the smallest keys, ascending by index."""
    key_row = np.asarray(key_row, np.uint64)
    assert len(set(key_row.tolist())) == len(key_row)
    return np.sort(np.argsort(key_row, kind="stable")[:n])


def sums_direct(u, B):
    """(S_AB, S_AA, S_BB) of the group B by their definitions: Python ints."""
    mask = np.zeros(u.shape[0], bool)
    mask[B] = True
    bb = int(u[np.ix_(mask, mask)].sum()) // 2
    aa = int(u[np.ix_(~mask, ~mask)].sum()) // 2
    ab = int(u[np.ix_(~mask, mask)].sum())
    return ab, aa, bb


def sums_by_rows(u, B):
    """The same through the row sums (step 5): one gather-sum over B x B and n row sums."""
    r = u.sum(axis=1)
    tot = int(r.sum())
    assert tot % 2 == 0
    bb = int(u[np.ix_(B, B)].sum()) // 2
    ab = int(r[B].sum()) - 2 * bb
    return ab, tot // 2 - bb - ab, bb


def T(ab, aa, bb, R, n):
    return int(ab) * (R * n) - int(aa) * (n * n) - int(bb) * (R * R)


def statistic(ab, aa, bb, R, n):
    """Step 8, numpy float64: every operation rounded on its own."""
    f = np.float64
    e = ((f(2.0) * f(ab)) / f(R * n) - (f(2.0) * f(aa)) / f(R * R)) - (f(2.0) * f(bb)) / f(n * n)
    return f(e * f(2.0 ** -20))


def test_from_u(u, R, n, P, seed, alpha):
    """The test on a quantised distance matrix -> (record dict, perm_sums int64 [P, 2])."""
    Np = R + n
    assert u.shape == (Np, Np)
    ab, aa, bb = sums_by_rows(u, np.arange(R, Np))
    t_obs = T(ab, aa, bb, R, n)
    ks = keys(Np, P, seed)
    perm = np.zeros((P, 2), np.int64)
    n_exceed = 0
    for p in range(P):
        pab, paa, pbb = sums_by_rows(u, group_of(ks[p], n))
        perm[p] = (pbb, pab)
        n_exceed += T(pab, paa, pbb, R, n) >= t_obs
    p_value = np.float32(np.float64(1 + n_exceed) / np.float64(P + 1))
    rec = dict(statistic=statistic(ab, aa, bb, R, n), s_ab=ab, s_aa=aa, s_bb=bb, p_value=p_value, n_exceed=int(n_exceed),
               drift=int(p_value <= np.float32(alpha)), n_degenerate=0)
    return rec, perm


def test(feat_bits, ref_bits, P, seed, alpha):
    """The whole contract: feat bf16 bits [S, n, D], ref bf16 bits [R, D] -> (record dict, perm_sums int64 [P, 2] or None for a
    window with a degenerate frame)."""
    q, _, bad = K.query(feat_bits)
    if bad.any():
        return dict(statistic=np.float64(np.nan), s_ab=0, s_aa=0, s_bb=0, p_value=np.float32(np.nan), n_exceed=-1, drift=1,
                    n_degenerate=int(bad.sum())), None
    R, n = ref_bits.shape[0], q.shape[0]
    pool = np.concatenate([K.bf16_to_f32(ref_bits), q])
    u = quantise(similarities(pool))
    assert u.max() < 1 << 22
    return test_from_u(u, R, n, P, seed, alpha)


test.__test__ = test_from_u.__test__ = False          # helpers, not pytest's


def record_words(rec):
    """The dict of `test` as the int32 [12] dwords of a fav_drift_record, NaNs canonical."""
    w = np.zeros(6, np.uint64)
    st = np.float64(rec["statistic"])
    w[0] = NAN64_BITS if np.isnan(st) else st.reshape(1).view(np.uint64)[0]
    for k, name in enumerate(("s_ab", "s_aa", "s_bb")):
        w[1 + k] = np.int64(rec[name]).reshape(1).view(np.uint64)[0]
    out = w.view(np.int32).copy()
    pv = np.float32(rec["p_value"])
    out[8] = np.int32(NAN32_BITS) if np.isnan(pv) else pv.reshape(1).view(np.int32)[0]
    out[9], out[10], out[11] = rec["n_exceed"], rec["drift"], rec["n_degenerate"]
    return out


def canon_words(words):
    """Device record int32 [12] with its NaNs made canonical."""
    out = np.array(words, np.int32).ravel().copy()
    if np.isnan(out[:2].view(np.float64)[0]):
        out[:2] = np.array([NAN64_BITS], np.uint64).view(np.int32)
    if np.isnan(out[8:9].view(np.float32)[0]):
        out[8] = NAN32_BITS
    return out
