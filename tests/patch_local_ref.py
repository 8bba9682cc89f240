"""numpy restatement of the locally aware patch query (include/fav.h beside fav_patch_site),
written from the contract alone: steps 1 to 3 one numpy float32 operation, hence one rounding, per contract operation, rows
and columns outside the map skipped; step 4 is the squared norm of tests/knn_ref.py ``query`` - its sixteen strided chains,
their sum in index order, the square root and the reciprocal - run on the aggregate.  ``score_at`` is tests/patch_ref.py with
this query in front."""
import numpy as np

import knn_ref as K
import patch_ref as P

F32 = np.float32


def mean_cells(maps_bits) -> np.ndarray:
    """maps uint16 [S, n, Hf, Wf, C] -> m float32 [n, Hf, Wf, C]: step 1."""
    x = K.bf16_to_f32(maps_bits)
    with np.errstate(all="ignore"):
        m = np.zeros(x.shape[1:], F32)
        for s in range(x.shape[0]):
            m = m + x[s]
        m = m * F32(1.0 / x.shape[0])
    assert m.dtype == F32
    return m


def aggregate(maps_bits, radius) -> np.ndarray:
    """maps uint16 [S, n, Hf, Wf, C] -> a float32 [n, Hf, Wf, C]: steps 1 to 3, written cell by cell as the contract states them."""
    m = mean_cells(maps_bits)
    n, Hf, Wf, _ = m.shape
    r = int(radius)
    with np.errstate(all="ignore"):
        v = np.zeros_like(m)
        for y in range(Hf):
            for dy in range(-r, r + 1):
                if 0 <= y + dy < Hf:
                    v[:, y] = v[:, y] + m[:, y + dy]
        a = np.zeros_like(m)
        for x in range(Wf):
            for dx in range(-r, r + 1):
                if 0 <= x + dx < Wf:
                    a[:, :, x] = a[:, :, x] + v[:, :, x + dx]
    assert v.dtype == a.dtype == F32
    return a


def normalise(a):
    """a float32 [M, D] -> (q float32 [M, D] holding bf16 values, ss float32 [M], degenerate bool [M]): step 4, with the lines of
    ``knn_ref.query`` behind its mean."""
    a = np.asarray(a, F32)
    M, D = a.shape
    with np.errstate(all="ignore"):
        p = np.zeros((M, 16), F32)
        for l in range(16):
            for j in range(l, D, 16):
                p[:, l] = p[:, l] + a[:, j] * a[:, j]
        ss = p[:, 0]
        for l in range(1, 16):
            ss = ss + p[:, l]
        bad = ~((ss > 0) & (ss < np.inf))
        inv = F32(1.0) / np.sqrt(ss)
        q = a * inv[:, None]
    assert p.dtype == ss.dtype == inv.dtype == q.dtype == F32
    q[bad] = 0
    return K.bf16_to_f32(K.f32_to_bf16_bits(q)), ss, bad


def query(maps_bits, grid, radius):
    """maps uint16 [S, n, HW, C], grid (Hf, Wf) -> (q float32 [n * HW, C], ss float32 [n * HW], degenerate bool [n * HW])."""
    maps_bits = np.asarray(maps_bits, np.uint16)
    S, n, HW, C = maps_bits.shape
    assert grid[0] * grid[1] == HW
    return normalise(aggregate(maps_bits.reshape(S, n, grid[0], grid[1], C), radius).reshape(n * HW, C))


def cells_at(maps_bits, bank_bits, grid, radius):
    """``patch_ref.cells`` with the locally aware query: (dist, nn_row, nn_sim float32/int32 [n, HW], degenerate bool [n, HW])."""
    S, n, HW, C = np.asarray(maps_bits).shape
    q, _, bad = query(maps_bits, grid, radius)
    sim = K.similarities(q, bank_bits)
    assert sim.dtype == F32 and np.isfinite(sim[~bad]).all()
    nn_row = np.argmax(sim, axis=1).astype(np.int32)
    nn_sim = sim[np.arange(sim.shape[0]), nn_row].copy()
    dist = np.maximum(F32(2.0) - F32(2.0) * nn_sim, F32(0.0))
    dist[bad] = nn_sim[bad] = np.uint32(P.QNAN_BITS).view(F32)
    nn_row[bad] = -1
    return dist.reshape(n, HW), nn_row.reshape(n, HW), nn_sim.reshape(n, HW), bad.reshape(n, HW)


def score_at(maps_bits, bank_bits, Wf, threshold, radius):
    """The whole head at a site -> (dist float32 [n, HW], nn_row int32 [n, HW], records int32 [n, 8])."""
    HW = np.asarray(maps_bits).shape[2]
    dist, nn_row, _, _ = cells_at(maps_bits, bank_bits, (HW // Wf, Wf), radius)
    return dist, nn_row, P.records(dist, nn_row, Wf, threshold)
