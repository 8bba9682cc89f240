"""numpy restatement of the nearest-neighbour OOD contract (include/fav.h beside fav_knn_record; DESIGN.md section 2, item
5g), written from the contract alone: steps 1 - 3 one numpy float32 operation, hence one rounding, per contract operation,
the p[l] loops over j exactly as written; step 4 the oracle's bit-exact model of the production GEMM; step 5 a sort and an
argmax."""
import numpy as np

from oracle import fav_oracle as O

NAN = np.float32(np.nan)


def bf16_to_f32(bits):
    """uint16 bf16 bit patterns -> float32."""
    return (np.asarray(bits, np.uint16).astype(np.uint32) << 16).view(np.float32)


def f32_to_bf16_bits(x):
    """float32 -> bf16 bit patterns, round to nearest even (finite values and infinities; a NaN stays a NaN)."""
    x = np.ascontiguousarray(x, np.float32)
    u = x.view(np.uint32)
    r = ((u + 0x7FFF + ((u >> 16) & 1)) >> 16).astype(np.uint16)
    nan = np.isnan(x)
    r[nan] = ((u[nan] >> 16) | 0x40).astype(np.uint16)
    return r


def query(feat_bits):
    """bf16 bits [S, n, D] -> (q float32 [n, D] holding bf16 values, ss float32 [n], degenerate bool [n]): steps 1 - 3, 7."""
    feat = bf16_to_f32(feat_bits)
    S, n, D = feat.shape
    with np.errstate(all="ignore"):
        fbar = np.zeros((n, D), np.float32)
        for s in range(S):
            fbar = fbar + feat[s]
        fbar = fbar * np.float32(1.0 / S)
        p = np.zeros((n, 16), np.float32)
        for l in range(16):
            for j in range(l, D, 16):
                p[:, l] = p[:, l] + fbar[:, j] * fbar[:, j]
        ss = p[:, 0]
        for l in range(1, 16):
            ss = ss + p[:, l]
        bad = ~((ss > 0) & (ss < np.inf))
        inv = np.float32(1.0) / np.sqrt(ss)
        q = fbar * inv[:, None]
    assert fbar.dtype == p.dtype == ss.dtype == inv.dtype == q.dtype == np.float32
    q[bad] = 0
    return bf16_to_f32(f32_to_bf16_bits(q)), ss, bad


def similarities(q, bank_bits):
    """q [n, D], bank bf16 bits [N, D] -> sim float32 [n, N]: step 4."""
    return O.gemm_acc(q, bf16_to_f32(bank_bits), "mfma") + np.float32(0)


def score(feat_bits, bank_bits, k, class_id, threshold):
    """The whole head -> dict kth_dist, kth_sim, nn_sim float32 [n], nn_row, nn_class, ood int32 [n]."""
    q, _, bad = query(feat_bits)
    sim = similarities(q, bank_bits)
    assert sim.dtype == np.float32 and np.isfinite(sim[~bad]).all()
    kth_sim = np.sort(sim, axis=1)[:, ::-1][:, k - 1].copy()
    nn_row = np.argmax(sim, axis=1).astype(np.int32)                # the first, that is the lowest, row of the maximum
    nn_sim = sim[np.arange(sim.shape[0]), nn_row].copy()
    nn_class = (np.full(nn_row.shape, -1) if class_id is None else np.asarray(class_id)[nn_row]).astype(np.int32)
    kth_dist = np.maximum(np.float32(2.0) - np.float32(2.0) * kth_sim, np.float32(0.0))
    with np.errstate(invalid="ignore"):
        ood = (~(kth_dist <= np.float32(threshold))).astype(np.int32)
    assert kth_dist.dtype == np.float32
    kth_sim[bad] = nn_sim[bad] = kth_dist[bad] = NAN
    nn_row[bad] = nn_class[bad] = -1
    ood[bad] = 1
    return dict(kth_dist=kth_dist, kth_sim=kth_sim, nn_sim=nn_sim, nn_row=nn_row, nn_class=nn_class, ood=ood)


def canon(x):
    x = np.array(x, np.float32)
    x[np.isnan(x)] = NAN
    return x


def records(out):
    """The dict of `score` as int32 [n, 6] fav_knn_record dwords, every NaN the canonical one (so that NaN equals NaN)."""
    rec = np.zeros((out["kth_dist"].shape[0], 6), np.int32)
    for col, name in enumerate(("kth_dist", "kth_sim", "nn_sim")):
        rec[:, col] = canon(out[name]).view(np.int32)
    rec[:, 3], rec[:, 4], rec[:, 5] = out["nn_row"], out["nn_class"], out["ood"]
    return rec


def canon_records(rec):
    """Device records int32 [n, 6] with their NaNs made canonical."""
    rec = np.array(rec, np.int32)
    for col in (0, 1, 2):
        rec[:, col] = canon(rec[:, col].view(np.float32)).view(np.int32)
    return rec
