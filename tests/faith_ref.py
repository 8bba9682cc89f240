"""A numpy restatement of the deletion / insertion curve contracts of include/fav.h (fav_op_rank_cells, fav_op_occlude,
fav_op_curve and fav_curve_record), written from the header text alone: the reference of tests/test_faith_host.py and
tests/test_gpu_faith.py.  Loops where the header states an order; nothing here is written for speed."""
import numpy as np

DELETION, INSERTION = 0, 1
NAN_BITS = 0x7FC00000
REC_NAMES = ("class_id", "auc", "p_first", "flip_step", "p_last", "p_min", "flip_cells", "reserved")


def before(va, a, vb, b):
    """Does cell a (value va) come before cell b (value vb) in the order "more salient first"?"""
    na, nb = np.isnan(va), np.isnan(vb)
    if not na and nb:
        return True
    if not na and not nb and va > vb:
        return True
    neither = (va == vb) or (na and nb)          # equal values (+0 against -0 among them), or both NaN
    return bool(neither and a < b)


def rank_cells(maps):
    """maps fp32 [n, cells] -> int32 [n, cells]: the number of cells that come before each cell."""
    maps = np.asarray(maps, np.float32)
    n, cells = maps.shape
    out = np.zeros((n, cells), np.int32)
    idx = np.arange(cells)
    with np.errstate(invalid="ignore"):
        for i in range(n):
            m = maps[i]
            na = np.isnan(m)
            for c in range(cells):                       # before(m[a], a, m[c], c) for every a at once
                v, nc = m[c], bool(na[c])
                front = (~na & nc) | (~na & (not nc) & (m > v)) | (((m == v) | (na & nc)) & (idx < c))
                out[i, c] = int(front.sum())
    return out


def cell_of(H, W, mh, mw):
    """int [H, W]: the cell of every pixel."""
    y = (np.arange(H, dtype=np.int64) * mh) // H
    x = (np.arange(W, dtype=np.int64) * mw) // W
    return y[:, None] * mw + x[None, :]


def step_counts(S, cells):
    """k_s for s = 0 .. S."""
    return (np.arange(S + 1, dtype=np.int64) * cells) // S


def occluded_mask(rank, H, W, mh, mw, S, s):
    """bool [n, H, W]: the pixels whose cell has rank < k_s."""
    k = int(step_counts(S, mh * mw)[s])
    return np.asarray(rank)[:, cell_of(H, W, mh, mw)] < k


def fill_pixel(fill, dtype):
    """The three words of `fill` as a pixel of the frames' dtype: the low byte under uint8, the word's bits under fp32."""
    w = np.asarray(fill, np.uint32)
    return (w & 255).astype(np.uint8) if dtype == np.uint8 else w.view(np.float32)


def occlude(frames, rank, mh, mw, mode, S, s0, s1, fill):
    """frames [n, H, W, 3] (uint8 or fp32) -> [s1 - s0, n, H, W, 3], every kept element bit for bit."""
    frames = np.ascontiguousarray(frames)
    n, H, W, _ = frames.shape
    word = np.uint8 if frames.dtype == np.uint8 else np.uint32
    src = frames.view(word)
    px = fill_pixel(fill, frames.dtype).view(word)
    out = np.empty((s1 - s0, n, H, W, 3), word)
    for s in range(s0, s1):
        m = occluded_mask(rank, H, W, mh, mw, S, s)
        filled = m if mode == DELETION else ~m
        out[s - s0] = np.where(filled[..., None], px[None, None, None, :], src)
    return out.view(frames.dtype)


def curve(prob, labels, classes, S, cells, mode):
    """prob fp32 [S+1, n], labels int32 [S+1, n], classes int32 [n] -> (curve fp32 [n, S+1], records int32 [n, 8]).  A class
    below 0 is the class outside the range (the op is not told the class count)."""
    prob = np.asarray(prob, np.float32)
    labels = np.asarray(labels, np.int32)
    n = prob.shape[1]
    f32 = np.float32
    half = f32(0.5 / S)
    cv = np.ascontiguousarray(prob.T)
    rec = np.zeros((n, 8), np.int32)

    def bits(v):
        return int(np.array(v, np.float32).view(np.int32))

    with np.errstate(invalid="ignore", over="ignore"):
        for i in range(n):
            p = prob[:, i]
            cls = int(classes[i])
            if cls < 0:
                rec[i] = (-1, NAN_BITS, NAN_BITS, -1, NAN_BITS, NAN_BITS, -1, 0)
                continue
            acc = f32(0.0)
            for s in range(S):
                acc = f32(acc + f32(p[s] + p[s + 1]))
            auc = f32(acc * half)
            best = f32(np.inf)
            for s in range(S + 1):
                if p[s] < best:
                    best = p[s]
            flip = -1
            for s in range(S + 1):
                same = int(labels[s, i]) == cls
                if same == (mode == INSERTION):
                    flip = s
                    break
            rec[i] = (cls, bits(auc), bits(p[0]), flip, bits(p[S]), bits(best), -1 if flip < 0 else flip * cells // S, 0)
    return cv, rec


def same_bits(got, want):
    """Equal as bits, except that a NaN equals any NaN (fp32 arrays), or plain equality (integer arrays)."""
    got, want = np.ascontiguousarray(got), np.ascontiguousarray(want)
    if got.shape != want.shape or got.dtype != want.dtype:
        return False
    if got.dtype == np.float32:
        g, w = got.view(np.uint32), want.view(np.uint32)
        return bool(((g == w) | (np.isnan(got) & np.isnan(want))).all())
    return bool(np.array_equal(got, want))


def same_records(got, want):
    """int32 [n, 8] records: the float dwords (1, 2, 4, 5) as same_bits, the others equal."""
    got, want = np.asarray(got, np.int32), np.asarray(want, np.int32)
    if got.shape != want.shape:
        return False
    fl = [1, 2, 4, 5]
    it = [0, 3, 6, 7]
    return same_bits(np.ascontiguousarray(got[:, fl]).view(np.float32), np.ascontiguousarray(want[:, fl]).view(np.float32)) and \
        bool(np.array_equal(got[:, it], want[:, it]))


def tricky_maps(n, cells, seed):
    """fp32 [n, cells] maps with runs of equal values, +0 against -0, both infinities, several NaNs; the last frame all NaN
    when n > 1."""
    rng = np.random.default_rng(seed)
    m = rng.integers(-3, 4, (n, cells)).astype(np.float32)          # few distinct values: long runs of ties
    specials = np.array([0.0, -0.0, np.inf, -np.inf, np.nan, np.nan, 1.5, -0.0], np.float32)
    for i in range(n):
        k = min(cells, specials.size)
        where = rng.permutation(cells)[:k]
        m[i, where] = specials[rng.permutation(specials.size)[:k]]
    if n > 1:
        m[-1] = np.nan
    return m
