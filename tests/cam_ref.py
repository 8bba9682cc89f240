"""numpy restatement of the class-activation-map contract of include/fav.h (beside fav_cam_record and fav_op_cam_heatmap),
operation by operation: every product and every sum is one float32 numpy operation, so each is rounded on its own, in the
order the contract fixes.  The GPU tests compare bits with it; tests/test_cam_host.py checks it against float64 and torch.

  1. lane partials   l < 64: p[l] = +0; for s = 0..S-1, m = 0..C/512-1, e = 0..7, ch = 512 m + 8 l + e:
                     p[l] = p[l] + fp32(w[c][ch]) * fp32(x[s][i][hw][ch])
  2. six halvings    h = 32, 16, 8, 4, 2, 1: p[l] = p[l] + p[l + h] for l < h;  M[hw] = p[0] * (float)(1.0 / S)
  3. logit_mean      +0 plus M[hw] in index order, times (float)(1.0 / HW), plus bias[c]
  4. peak, floor     strict > (<) scans in index order from -inf (+inf); ties to the lowest cell, a NaN never wins
  5. pos_sum         +0 plus fmax(M[hw], +0) in index order; thr = 0.2f * peak; n_above and the inclusive box of the cells
                     with M[hw] >= thr, only when peak > 0 - the box of ALL such cells, not of a connected component
  6. a class outside [0, n_classes): map all 0x7FC00000, class_id -1, peak_cell -1, n_above 0, box -1, floats NaN
The partition does not depend on any grid or block geometry.  A NaN's payload and sign are not part of the contract:
``same_bits`` compares bits everywhere else and NaN-ness where either side is a NaN."""
import numpy as np

from map_ref import cells_above, same_bits  # noqa: F401  (same_bits: for the tests that compare with this module)

F32 = np.float32
QNAN_BITS = 0x7FC00000
RECORD_DWORDS = 8


def bf16_bits_to_f32(bits) -> np.ndarray:
    return (np.asarray(bits, np.uint16).astype(np.uint32) << 16).view(np.float32)


def f32_to_bf16_bits(x) -> np.ndarray:
    """finite float32 -> bf16 bit patterns, round to nearest even."""
    u = np.ascontiguousarray(x, np.float32).view(np.uint32)
    return ((u + 0x7FFF + ((u >> 16) & 1)) >> 16).astype(np.uint16)


def cam_maps(x_bits, w_bits, classes, n_classes) -> np.ndarray:
    """Steps 1, 2 and the map half of 6.  x_bits uint16 [S, n, HW, C]; w_bits uint16 [rows, ldw] (ldw >= C); classes int
    [n, K] -> M float32 [n, K, HW]."""
    x = bf16_bits_to_f32(x_bits)
    w = bf16_bits_to_f32(w_bits)
    S, n, HW, C = x.shape
    classes = np.asarray(classes, np.int64).reshape(n, -1)
    valid = (classes >= 0) & (classes < n_classes)
    rows = w[np.where(valid, classes, 0)]                    # [n, K, ldw]
    lanes = 8 * np.arange(64)
    p = np.zeros((n, classes.shape[1], HW, 64), F32)
    with np.errstate(all="ignore"):
        for s in range(S):
            for m in range(C // 512):
                for e in range(8):
                    ch = 512 * m + lanes + e
                    prod = rows[:, :, None, ch] * x[s][:, None, :, ch]      # one rounding
                    p = p + prod                                            # one rounding
        for h in (32, 16, 8, 4, 2, 1):
            p = p[..., :h] + p[..., h:2 * h]
        M = p[..., 0] * F32(1.0 / S)
    M[~valid] = np.uint32(QNAN_BITS).view(F32)
    return M


def cam_records(M, classes, bias, n_classes, Wf) -> np.ndarray:
    """Steps 3 - 6 on maps M float32 [n, K, HW] -> int32 [n, K, 8] fav_cam_record records."""
    M = np.asarray(M, F32)
    n, K, HW = M.shape
    classes = np.asarray(classes, np.int64).reshape(n, K)
    bias = np.asarray(bias, F32)
    rec = np.zeros((n, K, RECORD_DWORDS), np.int32)
    f = rec.view(F32)
    with np.errstate(all="ignore"):
        for i in range(n):
            for k in range(K):
                c = int(classes[i, k])
                if not 0 <= c < n_classes:
                    rec[i, k] = (-1, QNAN_BITS, QNAN_BITS, -1, QNAN_BITS, QNAN_BITS, 0, -1)
                    continue
                m = M[i, k]
                total, pos = F32(0), F32(0)
                peak, cell, floor = F32(-np.inf), -1, F32(np.inf)
                for hw in range(HW):
                    v = m[hw]
                    total = total + v
                    if v > peak:
                        peak, cell = v, hw
                    if v < floor:
                        floor = v
                    pos = pos + np.fmax(v, F32(0))
                logit = total * F32(1.0 / HW) + bias[c]
                n_above, box = 0, -1
                if peak > 0:
                    n_above, box = cells_above(m, F32(0.2) * peak, Wf)
                rec[i, k, 0], rec[i, k, 3], rec[i, k, 6], rec[i, k, 7] = c, cell, n_above, box
                f[i, k, 1], f[i, k, 2], f[i, k, 4], f[i, k, 5] = logit, peak, floor, pos
    return rec


def cam(x_bits, w_bits, bias, classes, n_classes, Wf):
    """The whole head -> (M float32 [n, K, HW], records int32 [n, K, 8])."""
    M = cam_maps(x_bits, w_bits, classes, n_classes)
    return M, cam_records(M, classes, bias, n_classes, Wf)


def _taps(size_out, size_in):
    """One axis of the bilinear resize: (i0, i1, lo, hi) for every output index, float32 as the contract orders it."""
    o = np.arange(size_out).astype(F32)
    scale = F32(size_in) / F32(size_out)
    src = np.fmax((o + F32(0.5)) * scale - F32(0.5), F32(0))
    i0 = np.minimum(src.astype(np.int32), size_in - 1)
    i1 = np.minimum(i0 + 1, size_in - 1)
    lo = src - i0.astype(F32)
    hi = F32(1) - lo
    return i0, i1, lo, hi


def heatmap(M, records, Hf, Wf, H, W) -> np.ndarray:
    """fav_op_cam_heatmap: maps float32 [m, Hf * Wf] and their records int32 [m, 8] -> uint8 [m, H, W]."""
    M = np.asarray(M, F32).reshape(-1, Hf, Wf)
    rec = np.asarray(records, np.int32).reshape(-1, RECORD_DWORDS)
    peak, floor = rec[:, 2].view(F32), rec[:, 4].view(F32)
    y0, y1, ly, hy = _taps(H, Hf)
    x0, x1, lx, hx = _taps(W, Wf)
    out = np.zeros((M.shape[0], H, W), np.uint8)
    with np.errstate(all="ignore"):
        for j in range(M.shape[0]):
            if not peak[j] > floor[j]:
                continue
            m = M[j]
            top = hx[None, :] * m[y0][:, x0] + lx[None, :] * m[y0][:, x1]
            bot = hx[None, :] * m[y1][:, x0] + lx[None, :] * m[y1][:, x1]
            v = hy[:, None] * top + ly[:, None] * bot
            t = (v - floor[j]) / (peak[j] - floor[j])
            out[j] = np.rint(np.fmin(np.fmax(t, F32(0)), F32(1)) * F32(255)).astype(np.uint8)
    return out


def pool(x_bits) -> np.ndarray:
    """avgpool_kernel's stated contract on maps uint16 [..., HW, C]: a sequential fp32 sum over HW, times fp32(1 / HW), one
    bf16 rounding -> uint16 [..., C]."""
    x = bf16_bits_to_f32(x_bits)
    HW = x.shape[-2]
    acc = np.zeros(x.shape[:-2] + x.shape[-1:], F32)
    for hw in range(HW):
        acc = acc + x[..., hw, :]
    return f32_to_bf16_bits(acc * F32(1.0 / HW))
