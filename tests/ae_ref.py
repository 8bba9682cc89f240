"""The autoencoder sensor restated in numpy (include/fav.h, beside fav_ae_record).

Every GEMM goes through oracle.fav_oracle - ``normalize_input``, ``conv_acc(..., "mfma")`` for the 3-channel layer,
``conv_acc_exact(..., "mfma")``, ``epilogue``, ``expf_exact`` - and everything behind the last accumulator is plain numpy in the
contract's order.  ``forward`` carries the activations twice: as spatial tensors, through an explicit pixel shuffle a decoder
step, and as the row-order matrices the device holds, through a flat reshape; ``row_to_pixel`` is the formula between them.
"""
import numpy as np

from oracle import fav_oracle as O

ONE = np.float32(1.0)
F255 = np.float32(255.0)


def grid_sizes(H, W, levels):
    h, w = [H], [W]
    for _ in range(levels):
        h.append((h[-1] - 1) // 2 + 1)
        w.append((w[-1] - 1) // 2 + 1)
    return h, w


def row_to_pixel(r, hL, wL, m):
    """Row(s) r of the last hidden matrix [n hL wL 4^m] -> (i, y, x) on the 2^m hL x 2^m wL level-1 grid."""
    r = np.asarray(r, np.int64)
    base, rem = r // 4 ** m, r % 4 ** m
    i, y, x = base // (hL * wL), (base // wL) % hL, base % wL
    for j in range(1, m + 1):
        d = (rem // 4 ** (m - j)) % 4
        y, x = 2 * y + d // 2, 2 * x + d % 2
    return i, y, x


def pixel_shuffle(y4, c):
    """[n, h, w, 4 c] with channel (2a + b) c + co -> [n, 2h, 2w, c]."""
    n, h, w, _ = y4.shape
    return y4.reshape(n, h, w, 2, 2, c).transpose(0, 1, 3, 2, 4, 5).reshape(n, 2 * h, 2 * w, c)


def frame_bytes(frames):
    """The frame in the units of step 5: u8 as it is; fp32 sanitised, clamped to [0, 1], times 255, rounded to even."""
    if frames.dtype == np.uint8:
        return frames.astype(np.int64)
    px = np.clip(O.sanitize_pixels(frames), np.float32(0), ONE).astype(np.float32)
    return np.rint(px * F255).astype(np.int64)


def sigmoid_bytes(acc12, bias3):
    """Steps 2 - 4 on acc [..., 12]: column (2a + b) 3 + co gets bias[co]."""
    z = (np.asarray(acc12, np.float32) + np.tile(np.asarray(bias3, np.float32), 4)).astype(np.float32)
    e = O.expf_exact((-z).astype(np.float32)).astype(np.float32).reshape(z.shape)
    s = (ONE / (ONE + e).astype(np.float32)).astype(np.float32)
    return np.rint(s * F255).astype(np.int64)


def dec1_acc(hidden, wg12):
    """Step 1: hidden [R, 64] (fp32 holding bf16 values) x wg12 [12, 64] -> acc [R, 12], the production accumulator."""
    R = hidden.shape[0]
    return O.conv_acc_exact(hidden.reshape(1, R, 1, 64), np.asarray(wg12, np.float32).reshape(12, 1, 1, 64), 1, 1, 1, 0, "mfma").reshape(R, 12)


def compare(q_full, frames, cell, threshold):
    """Steps 5 - 9 on the uncropped bytes q_full [n, >= H, >= W, 3] -> dict of recon, cell_sse, err_map and the record fields."""
    n, H, W, _ = frames.shape
    recon = q_full[:, :H, :W]
    e2 = (recon - frame_bytes(frames)) ** 2
    gh, gw = -(-H // cell), -(-W // cell)
    pad = np.zeros((n, gh * cell, gw * cell, 3), np.int64)
    pad[:, :H, :W] = e2
    cell_sse = pad.reshape(n, gh, cell, gw, cell, 3).sum(axis=(2, 4, 5))
    ins_y = np.minimum(cell, H - cell * np.arange(gh))
    ins_x = np.minimum(cell, W - cell * np.arange(gw))
    inside = ins_y[:, None] * ins_x[None, :]
    err_map = (cell_sse.astype(np.float64) / ((3 * inside).astype(np.float64) * 65025.0)).astype(np.float32)
    sse = cell_sse.sum(axis=(1, 2))
    flat = err_map.reshape(n, gh * gw)
    out = dict(recon=recon.astype(np.uint8), cell_sse=cell_sse.astype(np.uint32), err_map=err_map, sse=sse,
               mse=(sse.astype(np.float64) / (np.float64(3 * H * W) * 65025.0)).astype(np.float32),
               peak=flat.max(axis=1), peak_cell=flat.argmax(axis=1).astype(np.int32), floor=flat.min(axis=1))
    n_above, box = np.zeros(n, np.int32), np.full(n, -1, np.int32)
    for i in range(n):
        ys, xs = np.nonzero(err_map[i] >= np.float32(threshold))
        n_above[i] = ys.size
        if ys.size:
            box[i] = np.uint32(xs.min() | ys.min() << 8 | xs.max() << 16 | ys.max() << 24).astype(np.int32)
    out.update(n_above=n_above, box=box)
    return out


def records(c):
    """The dict of ``compare`` -> int32 [n, 8] fav_ae_record."""
    n = c["sse"].shape[0]
    rec = np.zeros((n, 8), np.int32)
    rec[:, 0] = (c["sse"] & 0xFFFFFFFF).astype(np.uint32).view(np.int32)
    rec[:, 1] = c["mse"].view(np.int32)
    rec[:, 2] = c["peak"].astype(np.float32).view(np.int32)
    rec[:, 3] = c["peak_cell"]
    rec[:, 4] = c["floor"].astype(np.float32).view(np.int32)
    rec[:, 5] = (c["sse"] >> 32).astype(np.uint32).view(np.int32)
    rec[:, 6] = c["n_above"]
    rec[:, 7] = c["box"]
    return rec


def decode_compare(hidden, n, hL, wL, m, wg12, bias3, frames, cell, threshold=np.inf):
    """fav_op_ae_decode_compare: hidden [n hL wL 4^m, 64] in the device's row order."""
    q = sigmoid_bytes(dec1_acc(np.asarray(hidden, np.float32), wg12), bias3)          # [R, 12]
    i, y, x = row_to_pixel(np.arange(hidden.shape[0]), hL, wL, m)
    hg, wg = hL << m, wL << m
    q_full = np.zeros((n, 2 * hg, 2 * wg, 3), np.int64)
    for a in range(2):
        for b in range(2):
            q_full[i, 2 * y + a, 2 * x + b] = q[:, (2 * a + b) * 3:(2 * a + b) * 3 + 3]
    return compare(q_full, frames, cell, threshold)


def forward(layers, levels, frames, cell=16, threshold=np.inf):
    """The whole sensor.  layers: ``autoencoder.parse_blob``'s.  -> the dict of ``compare`` plus ``hidden`` (the last hidden
    matrix in row order, fp32 holding bf16 values), ``hidden_spatial`` [n, 2^m hL, 2^m wL, 64] and ``rows`` (every layer's
    output as the device's matrix)."""
    n, H, W, _ = frames.shape
    L = levels
    h, w = grid_sizes(H, W, L)
    xn = O.normalize_input(frames, (0.0, 0.0, 0.0), (1.0, 1.0, 1.0))
    w1, b1 = layers[0]
    L1 = O.ConvLayer(64, 3, 3, 3, 2, 1, np.ascontiguousarray(w1[:, :27].reshape(64, 3, 3, 3)), b1)
    x = O.epilogue(O.conv_acc(xn, L1, "mfma"), b1, relu=True)
    rows = [x.reshape(-1, 64)]
    for l in range(2, L + 1):
        wl, bl = layers[l - 1]
        x = O.epilogue(O.conv_acc_exact(x, wl, 3, 3, 2, 1, "mfma"), bl, relu=True)
        rows.append(x.reshape(-1, x.shape[-1]))
    spatial, mat = x, x.reshape(-1, x.shape[-1])
    for j, l in enumerate(range(L, 1, -1)):
        wg, bg = layers[L + j]
        c_in, c_out = mat.shape[1], wg.shape[0] // 4
        y4 = O.epilogue(O.conv_acc_exact(mat.reshape(1, -1, 1, c_in), wg.reshape(4 * c_out, 1, 1, c_in), 1, 1, 1, 0, "mfma"), bg, relu=True)
        y4 = y4.reshape(-1, 4 * c_out)
        mat = y4.reshape(-1, c_out)                                                   # the device's view: four times the rows
        # the spatial view: the same GEMM is a per-pixel map, so apply the shuffle to the matrix laid out over the old grid
        ns, hs, ws_, _ = spatial.shape
        ys = O.epilogue(O.conv_acc_exact(spatial, wg.reshape(4 * c_out, 1, 1, c_in), 1, 1, 1, 0, "mfma"), bg, relu=True)
        spatial = pixel_shuffle(ys.reshape(ns, hs, ws_, 4 * c_out), c_out)
        rows.append(mat)
    wg12, b3 = layers[2 * L - 1]
    q = sigmoid_bytes(O.conv_acc_exact(spatial, wg12.reshape(12, 1, 1, 64), 1, 1, 1, 0, "mfma"), b3)   # [n, hg, wg, 12]
    out = compare(pixel_shuffle(q, 3), frames, cell, threshold)
    out.update(hidden=mat, hidden_spatial=spatial, rows=rows, h=h, w=w)
    return out
