"""A numpy restatement of the RISE contracts of include/fav.h (fav_rise, fav_op_rise_mask, fav_op_rise_accumulate and
fav_rise_record), written from the header text alone on oracle.fav_oracle.philox4x32_10: the reference of
tests/test_rise_host.py and tests/test_gpu_rise.py.  The mask runs in int64, the mathematical integer of the contract; loops
where the header states an order; nothing here is written for speed."""
import collections

import numpy as np

from map_ref import cells_above
from oracle.fav_oracle import philox4x32_10

SITE = 0x715E
SHIFT_CHUNK = 16
NAN_BITS = 0x7FC00000
REC_NAMES = ("class_id", "p_full", "peak", "peak_cell", "floor", "p_mean", "n_above", "box")

#: the descriptor: n_masks, grid, keep (in 256ths), seed, and the fill words of either layout
Desc = collections.namedtuple("Desc", "n_masks grid keep seed fill_u8 fill_f32_bits", defaults=((128, 128, 128), (0x3F000000,) * 3))


def cell_sizes(H, W, g):
    """(ch, cw) = (ceil(H / g), ceil(W / g))."""
    return -(-H // g), -(-W // g)


def draws(F, m, seed, chunks):
    """uint8 [len(chunks), 16]: the bytes of philox4x32_10((chunk, F, m, 0x715E), seed), x's low byte first."""
    x, y, z, w = philox4x32_10(np.asarray(chunks, np.uint32), np.uint32(F & 0xFFFFFFFF), np.uint32(m), np.uint32(SITE),
                               seed & 0xFFFFFFFF, (seed >> 32) & 0xFFFFFFFF)
    words = np.stack([x, y, z, w], axis=-1).astype("<u4")
    return words.view(np.uint8).reshape(len(chunks), 16)


def grid_bits(g, keep, seed, F, m):
    """int64 [g+1, g+1] of 0 / 1: cell j = gy * (g+1) + gx is ON iff byte j % 16 of chunk j / 16 is < keep."""
    cells = (g + 1) * (g + 1)
    b = draws(F, m, seed, np.arange((cells + 15) // 16)).reshape(-1)[:cells]
    return (b < keep).astype(np.int64).reshape(g + 1, g + 1)


def shift(g, seed, F, m, H, W):
    """(dy, dx) = (mulhi32(x, ch), mulhi32(y, cw)) of chunk 16's draw."""
    ch, cw = cell_sizes(H, W, g)
    words = draws(F, m, seed, [SHIFT_CHUNK]).reshape(16).view("<u4")
    return (int(words[0]) * ch) >> 32, (int(words[1]) * cw) >> 32


def axis(p, c, g):
    """Shifted pixel positions p (int64 array) along an axis of cell size c -> (i0, i1, f)."""
    num = np.maximum(2 * p + 1 - c, 0)
    i0, f = num // (2 * c), num % (2 * c)
    over = i0 >= g
    i0 = np.where(over, g, i0)
    f = np.where(over, 0, f)
    return i0, np.minimum(i0 + 1, g), f


def upsample(bits, g, H, W, dy, dx, ys=None, xs=None):
    """mq int64 [len(ys), len(xs)] of the grid `bits` at the pixel rows ys and columns xs (default: every pixel)."""
    ch, cw = cell_sizes(H, W, g)
    ys = np.arange(H, dtype=np.int64) if ys is None else np.asarray(ys, np.int64)
    xs = np.arange(W, dtype=np.int64) if xs is None else np.asarray(xs, np.int64)
    y0, y1, fy = axis(ys + dy, ch, g)
    x0, x1, fx = axis(xs + dx, cw, g)
    top = (2 * cw - fx)[None, :] * bits[y0][:, x0] + fx[None, :] * bits[y0][:, x1]
    bot = (2 * cw - fx)[None, :] * bits[y1][:, x0] + fx[None, :] * bits[y1][:, x1]
    num2 = (2 * ch - fy)[:, None] * top + fy[:, None] * bot
    assert num2.min() >= 0 and num2.max() <= 4 * ch * cw
    return (256 * num2 + 2 * ch * cw) // (4 * ch * cw)


def frame_index(first_index, i):
    return (int(first_index) + i) & 0xFFFFFFFF


def mask(d, F, m, H, W, ys=None, xs=None):
    """mq of frame index F under mask m."""
    dy, dx = shift(d.grid, d.seed, F, m, H, W)
    return upsample(grid_bits(d.grid, d.keep, d.seed, F, m), d.grid, H, W, dy, dx, ys, xs)


def masks(d, first_index, n, H, W, m0, m1):
    """int64 [m1 - m0, n, H, W]."""
    return np.stack([np.stack([mask(d, frame_index(first_index, i), m, H, W) for i in range(n)]) for m in range(m0, m1)])


def blend(frames, mq, d):
    """frames [n, H, W, 3] uint8 or fp32 under mq int64 [n, H, W] -> the same shape and dtype."""
    mq = mq[..., None]
    if frames.dtype == np.uint8:
        fill = (np.asarray(d.fill_u8, np.int64) & 255)[None, None, None, :]
        return ((frames.astype(np.int64) * mq + fill * (256 - mq) + 128) >> 8).astype(np.uint8)
    f32 = np.float32
    f = np.asarray(d.fill_f32_bits, np.uint32).view(f32)[None, None, None, :]
    w = (mq.astype(f32) * f32(2.0 ** -8)).astype(f32)
    with np.errstate(invalid="ignore", over="ignore"):
        diff = (frames - f).astype(f32)
        part = (f + (w * diff).astype(f32)).astype(f32)
    out = np.where(mq == 256, frames.view(np.uint32), np.where(mq == 0, np.broadcast_to(f, frames.shape).view(np.uint32), part.view(np.uint32)))
    return out.astype(np.uint32).view(f32)


def rise_mask(frames, d, first_index, m0, m1):
    """fav_op_rise_mask -> ([m1 - m0, n, H, W, 3], mq int64 [m1 - m0, n, H, W])."""
    frames = np.ascontiguousarray(frames)
    n, H, W, _ = frames.shape
    mq = masks(d, first_index, n, H, W, m0, m1)
    return np.stack([blend(frames, mq[k], d) for k in range(m1 - m0)]), mq


def cell_span(c, size, m):
    """(lo, hi) of the pixels p with p * m // size == c, by the header's closed form."""
    return -(-(c * size) // m), -(-((c + 1) * size) // m) - 1


def sample_pixels(size, m):
    """int64 [m]: the sample pixel of every cell along an axis."""
    return np.array([sum(cell_span(c, size, m)) // 2 for c in range(m)], np.int64)


def bits(v):
    return int(np.array(v, np.float32).view(np.int32))


def accumulate(prob, classes, d, first_index, H, W, mh, mw, num_classes=0):
    """prob fp32 [N + 1, n], classes int32 [n] -> (map fp32 [n, mh * mw], records int32 [n, 8], cov int64 [n, mh * mw])."""
    prob = np.asarray(prob, np.float32)
    f32 = np.float32
    N, n, cells = d.n_masks, prob.shape[1], mh * mw
    assert prob.shape[0] == N + 1
    ys, xs = sample_pixels(H, mh), sample_pixels(W, mw)
    out = np.zeros((n, cells), f32)
    rec = np.zeros((n, 8), np.int32)
    covs = np.zeros((n, cells), np.int64)
    inv_n = f32(1.0 / N)
    with np.errstate(invalid="ignore", over="ignore", divide="ignore"):
        for i in range(n):
            F = frame_index(first_index, i)
            acc, cov, psum = np.zeros(cells, f32), np.zeros(cells, np.int64), f32(0.0)
            for m in range(N):
                wq = mask(d, F, m, H, W, ys, xs).reshape(cells)
                p = prob[1 + m, i]
                acc = (acc + (p * (wq.astype(f32) * f32(2.0 ** -8)).astype(f32)).astype(f32)).astype(f32)
                cov += wq
                psum = f32(psum + p)
            M = np.where(cov > 0, (acc / (cov.astype(f32) * f32(2.0 ** -8)).astype(f32)).astype(f32), f32(0.0)).astype(f32)
            out[i], covs[i] = M, cov
            cls = int(classes[i])
            if cls < 0 or (num_classes > 0 and cls >= num_classes):
                rec[i] = (-1, NAN_BITS, NAN_BITS, -1, NAN_BITS, NAN_BITS, 0, -1)
                continue
            peak, flo, peak_cell = f32(-np.inf), f32(np.inf), -1
            for c in range(cells):
                if M[c] > peak:
                    peak, peak_cell = M[c], c
                if M[c] < flo:
                    flo = M[c]
            n_above, box = 0, -1
            if peak > flo:
                n_above, box = cells_above(M, f32(flo + f32(f32(0.5) * f32(peak - flo))), mw)
            rec[i] = (cls, bits(prob[0, i]), bits(peak), peak_cell, bits(flo), bits(f32(psum * inv_n)), n_above, box)
    return out, rec, covs


def same_records(got, want):
    """int32 [n, 8] records: the float dwords (1, 2, 4, 5) equal as bits or both NaN, the others equal."""
    got, want = np.asarray(got, np.int32), np.asarray(want, np.int32)
    if got.shape != want.shape:
        return False
    fl, it = [1, 2, 4, 5], [0, 3, 6, 7]
    g, w = np.ascontiguousarray(got[:, fl]), np.ascontiguousarray(want[:, fl])
    gf, wf = g.view(np.float32), w.view(np.float32)
    return bool(((g == w) | (np.isnan(gf) & np.isnan(wf))).all()) and bool(np.array_equal(got[:, it], want[:, it]))


# ---- the end-to-end inputs of tests/test_gpu_rise.py (fav_classify_rise through a handle).  tests/test_rise_host.py checks that
# every cell of every frame gets some coverage under them, so that the +0 rule cannot hide a wrong map there.
E2E_DESC = Desc(n_masks=6, grid=3, keep=128, seed=0x5EED0001C0FFEE, fill_u8=(64, 128, 255),
                fill_f32_bits=tuple(int(np.float32(v).view(np.uint32)) for v in (0.25, 0.5, 1.0)))
E2E_MAP = (4, 4)
E2E_FIRST = 1000
E2E_MAX_BATCH = 8
E2E_SIZES = (32, 64)            # the CIFAR ResNet-18 and its ensemble; ViT-tiny
