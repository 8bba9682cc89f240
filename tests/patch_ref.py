"""numpy restatement of the patch-level anomaly contract (include/fav.h beside fav_patch_record; DESIGN.md section 2, item
5m), written from the contract alone.  Steps 1 and 2 are the k-NN head's (tests/knn_ref.py ``query`` and ``similarities``, the
oracle's bit-exact model of the production GEMM) with a cell for a frame; step 3 an argmax; step 4 the record's scans written
out as stated, one numpy float32 operation, hence one rounding, per contract operation.  Nothing here knows of chunks."""
import numpy as np

import knn_ref as K
from map_ref import cells_above

F32 = np.float32
QNAN_BITS = 0x7FC00000
RECORD_DWORDS = 8


def cells(maps_bits, bank_bits):
    """maps uint16 [S, n, HW, C], bank uint16 [N, C] -> (dist float32 [n, HW], nn_row int32 [n, HW], nn_sim float32 [n, HW],
    degenerate bool [n, HW]): steps 1 - 3."""
    maps_bits = np.asarray(maps_bits, np.uint16)
    S, n, HW, C = maps_bits.shape
    q, _, bad = K.query(maps_bits.reshape(S, n * HW, C))
    sim = K.similarities(q, bank_bits)
    assert sim.dtype == F32 and np.isfinite(sim[~bad]).all()
    nn_row = np.argmax(sim, axis=1).astype(np.int32)                # the first, that is the lowest, row of the maximum
    nn_sim = sim[np.arange(sim.shape[0]), nn_row].copy()
    dist = np.maximum(F32(2.0) - F32(2.0) * nn_sim, F32(0.0))
    assert dist.dtype == F32
    dist[bad] = nn_sim[bad] = np.uint32(QNAN_BITS).view(F32)
    nn_row[bad] = -1
    return dist.reshape(n, HW), nn_row.reshape(n, HW), nn_sim.reshape(n, HW), bad.reshape(n, HW)


def records(dist, nn_row, Wf, threshold) -> np.ndarray:
    """Step 4 on dist float32 [n, HW] and nn_row int32 [n, HW] -> int32 [n, 8] fav_patch_record records."""
    dist = np.asarray(dist, F32)
    n, HW = dist.shape
    rec = np.zeros((n, RECORD_DWORDS), np.int32)
    f = rec.view(F32)
    with np.errstate(all="ignore"):
        for i in range(n):
            total = F32(0)
            peak, cell, floor = F32(-np.inf), -1, F32(np.inf)
            for hw in range(HW):
                v = dist[i, hw]
                total = total + v
                if v > peak:
                    peak, cell = v, hw
                if v < floor:
                    floor = v
            n_above, box = cells_above(dist[i], F32(threshold), Wf)
            rec[i, 0] = int((nn_row[i] == -1).sum())
            f[i, 1], f[i, 2], f[i, 4] = total * F32(1.0 / HW), peak, floor
            rec[i, 3], rec[i, 5] = cell, (nn_row[i, cell] if cell >= 0 else -1)
            rec[i, 6], rec[i, 7] = n_above, box
    return rec


def score(maps_bits, bank_bits, Wf, threshold):
    """The whole head -> (dist float32 [n, HW], nn_row int32 [n, HW], records int32 [n, 8])."""
    dist, nn_row, _, _ = cells(maps_bits, bank_bits)
    return dist, nn_row, records(dist, nn_row, Wf, threshold)


def canon_records(rec) -> np.ndarray:
    """Records int32 [n, 8] with the NaNs of their three floats made canonical (so that a NaN equals a NaN)."""
    rec = np.array(rec, np.int32)
    for col in (1, 2, 4):
        rec[:, col] = K.canon(rec[:, col].view(F32)).view(np.int32)
    return rec


def canon_map(dist) -> np.ndarray:
    """A dist map's bits, every NaN the canonical one."""
    return K.canon(dist).view(np.int32)
