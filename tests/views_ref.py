"""numpy restatement of the view contract (include/fav.h above fav_set_views), written from
the contract's five steps and not from the kernels.  A view is a dict / object with flip_x, flip_y, transpose, dy, dx and
border (0 reflect-101, 1 replicate, 2 zero); frames are [n, H, W, 3] arrays of any dtype and are only ever indexed, so every
element keeps its bits."""
import numpy as np

REFLECT101, REPLICATE, ZERO = 0, 1, 2
BORDER_NAMES = ("reflect101", "replicate", "zero")


def V(flip_x=0, flip_y=0, transpose=0, dy=0, dx=0, border=REFLECT101):
    return dict(flip_x=int(flip_x), flip_y=int(flip_y), transpose=int(transpose), dy=int(dy), dx=int(dx), border=int(border))


def as_dict(v):
    """A views.View (border by name) or a dict -> the dict form."""
    if isinstance(v, dict):
        return v
    b = v.border
    return V(v.flip_x, v.flip_y, v.transpose, v.dy, v.dx, BORDER_NAMES.index(b) if isinstance(b, str) else b)


def border_index(i, n, border):
    """Step 2 for one index against a dimension of n -> (index, inside?)."""
    if border == REFLECT101:
        if n == 1:
            return 0, True
        p = 2 * (n - 1)
        m = i % p                        # python's % is non-negative for p > 0
        return (m if m < n else p - m), True
    if border == REPLICATE:
        return min(max(i, 0), n - 1), True
    if border == ZERO:
        return (i, True) if 0 <= i < n else (0, False)
    raise ValueError(border)


def axis_map(n, d, border, flip):
    """Steps 1 to 3 along one axis of length n: output index i -> (source index, inside?)."""
    idx, ok = np.zeros(n, np.int64), np.zeros(n, bool)
    for i in range(n):
        s, ok[i] = border_index(i - d, n, border)
        idx[i] = n - 1 - s if flip else s
    return idx, ok


def source_map(view, H, W):
    """-> (u[H, W], v[H, W], inside[H, W]): the source pixel of every output pixel, steps 1 to 4."""
    view = as_dict(view)
    if view["transpose"] and H != W:
        raise ValueError("transpose needs H == W")
    uy, oky = axis_map(H, view["dy"], view["border"], view["flip_y"])      # u from y, against H
    vx, okx = axis_map(W, view["dx"], view["border"], view["flip_x"])      # v from x, against W
    u = np.broadcast_to(uy[:, None], (H, W))
    v = np.broadcast_to(vx[None, :], (H, W))
    inside = oky[:, None] & okx[None, :]
    if view["transpose"]:
        u, v = v, u                                                          # step 4: swap u and v
    return u, v, inside


def apply_view(frames, view):
    """[n, H, W, 3] -> the view of every frame, same dtype, bits untouched."""
    n, H, W, C = frames.shape
    u, v, inside = source_map(view, H, W)
    out = frames[:, u, v, :].copy()
    out[:, ~inside, :] = np.zeros((), frames.dtype)
    return out


def apply_views(frames, views):
    """-> [len(views), n, H, W, 3]: view a of frame i at [a, i]."""
    return np.stack([apply_view(frames, v) for v in views])


def asymmetric_frame(H, W, dtype=np.uint8):
    """One frame whose pixels are all different (as long as H * W <= 2^16 for uint8): pixel (y, x) holds its own index."""
    idx = np.arange(H * W, dtype=np.int64).reshape(H, W)
    if dtype == np.uint8:
        f = np.stack([idx & 255, (idx >> 8) & 255, (idx * 7 + 3) & 255], axis=-1).astype(np.uint8)
    else:
        f = np.stack([idx, idx + 0.25, -idx - 0.5], axis=-1).astype(dtype)
    return f[None]
