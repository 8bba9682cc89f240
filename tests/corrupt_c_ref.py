"""The tests' restatement of the ImageNet-C style corruption family (fav_op_corrupt_c), numpy only.

The exact kinds (impulse, contrast, pixelate, brightness, saturate) follow the fp32 operation order of the definitions and are
compared bit for bit; speckle and the two blurs are restated in float64, on the kernel's own 24-bit uniforms and on the fp32
taps fav_corruption_taps hands out, and are compared within a derived bound.  x_c = fp32(u8) * fp32(1 / 255) in all of them."""
import ctypes as C

import numpy as np

from oracle.corrupt_oracle import u01
from oracle.fav_oracle import philox4x32_10

f32 = np.float32
KINDS = ("impulse_noise", "speckle_noise", "gaussian_blur", "defocus_blur", "contrast", "pixelate", "brightness", "saturate")
#: the issue's severity table, (a, b) at severities 1..5
TABLE = {
    "impulse_noise": ((.03, 0), (.06, 0), (.09, 0), (.17, 0), (.27, 0)),
    "speckle_noise": ((.15, 0), (.2, 0), (.35, 0), (.45, 0), (.6, 0)),
    "gaussian_blur": ((1, 0), (2, 0), (3, 0), (4, 0), (6, 0)),
    "defocus_blur": ((3, .1), (4, .5), (6, .5), (8, .5), (10, .5)),
    "contrast": ((.4, 0), (.3, 0), (.2, 0), (.1, 0), (.05, 0)),
    "pixelate": ((.6, 0), (.5, 0), (.4, 0), (.3, 0), (.25, 0)),
    "brightness": ((.1, 0), (.2, 0), (.3, 0), (.4, 0), (.5, 0)),
    "saturate": ((.3, 0), (.1, 0), (2, 0), (5, .1), (20, .2)),
}
GAUSS_RADII = (4, 8, 12, 16, 24)
DEFOCUS_RADII = (4, 5, 7, 9, 12)


def params(kind, severity):
    """(a, b) of the table as the fp32 values the C ABI carries."""
    a, b = TABLE[kind][severity - 1]
    return float(f32(a)), float(f32(b))


def lib_taps(lib, kind, a, b, cap=4096):
    """fav_corruption_taps -> (status, fp32 taps, R); the taps are [2R+1] or [2R+1, 2R+1]."""
    buf = (C.c_float * max(cap, 1))()
    R = C.c_int32(-1)
    st = lib.fav_corruption_taps(KINDS.index(kind), a, b, buf, cap, C.byref(R))
    if st != 0:
        return st, None, R.value
    S = 2 * R.value + 1
    t = np.frombuffer(buf, f32, S if kind == "gaussian_blur" else S * S).copy()
    return st, (t if kind == "gaussian_blur" else t.reshape(S, S)), R.value


def gauss_taps_f64(a):
    """exp(-0.5 (d / a)^2) for d in [-R, R], R = (int)(4 a + 0.5), normalised; float64."""
    a = float(f32(a))
    R = int(4.0 * a + 0.5)
    w = np.exp(-0.5 * (np.arange(-R, R + 1, dtype=np.float64) / a) ** 2)
    return w / w.sum(), R


def disk_taps_f64(a, b):
    """The disk dx^2 + dy^2 <= r^2 on the (2R+1)^2 grid, normalised, smoothed separably with zero padding by the
    (2ks+1)-tap Gaussian of sigma b, renormalised to sum 1; float64."""
    a, b = float(f32(a)), float(f32(b))
    r = int(a)
    ks = 1 if r <= 8 else 2
    R = r + ks
    d = np.arange(-R, R + 1)
    disk = ((d[:, None] ** 2 + d[None, :] ** 2) <= r * r).astype(np.float64)
    disk /= disk.sum()
    g = np.exp(-0.5 * (np.arange(-ks, ks + 1, dtype=np.float64) / b) ** 2)
    g /= g.sum()
    S = 2 * R + 1
    pad = np.zeros((S, S + 2 * ks))
    pad[:, ks:ks + S] = disk
    rows = sum(g[k] * pad[:, k:k + S] for k in range(2 * ks + 1))
    pad = np.zeros((S + 2 * ks, S))
    pad[ks:ks + S] = rows
    out = sum(g[k] * pad[k:k + S] for k in range(2 * ks + 1))
    return out / out.sum(), R


def cell_map(n, a):
    """Pixelate along one dimension of n pixels: (cells hd, the cell of every pixel)."""
    hd = max(1, int(float(n) * float(f32(a))))
    i = np.arange(n, dtype=np.int64)
    return hd, ((2 * i + 1) * hd) // (2 * n)


def reflect101(i, n):
    """Reflect-101 with period 2(n-1), any distance; a dimension of 1 maps to 0."""
    i = np.asarray(i, np.int64)
    if n == 1:
        return np.zeros_like(i)
    p = 2 * (n - 1)
    m = np.mod(i, p)
    return np.where(m < n, m, p - m)


def _draws(shape, stream, seed, first_index):
    n, H, W = shape
    px = np.arange(H * W, dtype=np.uint32)[None, :]
    fr = np.arange(n, dtype=np.uint64) + np.uint64(int(first_index) & 0xFFFFFFFF)
    fr = (fr & np.uint64(0xFFFFFFFF)).astype(np.uint32)[:, None]
    return philox4x32_10(px, fr, np.uint32(stream), np.uint32(0), seed & 0xFFFFFFFF, (seed >> 32) & 0xFFFFFFFF)


def x_of(frames):
    return frames.astype(f32) * f32(1.0 / 255.0)


def clamp(v):
    return np.minimum(np.maximum(v, v.dtype.type(0)), v.dtype.type(1))


def impulse(frames, a, seed, first_index):
    n, H, W, _ = frames.shape
    u = _draws((n, H, W), 16, seed, first_index)
    hit = np.stack([u01(u[c]) < f32(a) for c in range(3)], axis=-1).reshape(frames.shape)
    val = np.stack([((u[3] >> np.uint32(c)) & np.uint32(1)).astype(f32) for c in range(3)], axis=-1).reshape(frames.shape)
    return np.where(hit, val, x_of(frames)).astype(f32), hit


def speckle(frames, a, seed, first_index, dtype=np.float64):
    """clamp(x + (x a) z), z Box-Muller on stream 17: float64 on the 24-bit uniforms, or the fp32 restatement."""
    n, H, W, _ = frames.shape
    u = _draws((n, H, W), 17, seed, first_index)
    if dtype == np.float64:
        v = [(w >> np.uint32(8)).astype(np.float64) / 16777216.0 for w in u]
        r0, r1 = np.sqrt(-2.0 * np.log(1.0 - v[0])), np.sqrt(-2.0 * np.log(1.0 - v[2]))
        t0, t1 = 2.0 * np.pi * v[1], 2.0 * np.pi * v[3]
        z = np.stack([r0 * np.cos(t0), r0 * np.sin(t0), r1 * np.cos(t1)], axis=-1).reshape(frames.shape)
        x = x_of(frames).astype(np.float64)
        return clamp(x + (x * float(f32(a))) * z)
    r0 = np.sqrt(f32(-2.0) * np.log(f32(1.0) - u01(u[0])), dtype=f32)
    r1 = np.sqrt(f32(-2.0) * np.log(f32(1.0) - u01(u[2])), dtype=f32)
    t0, t1 = f32(6.2831853071795864) * u01(u[1]), f32(6.2831853071795864) * u01(u[3])
    z = np.stack([r0 * np.cos(t0), r0 * np.sin(t0), r1 * np.cos(t1)], axis=-1).astype(f32).reshape(frames.shape)
    x = x_of(frames)
    return clamp(x + (x * f32(a)) * z)


def contrast(frames, a):
    n, H, W, _ = frames.shape
    S = frames.astype(np.int64).sum(axis=(1, 2))                                   # [n, 3], exact
    m = (S.astype(np.float64) / (float(H) * W * 255.0)).astype(f32)[:, None, None, :]
    return clamp((x_of(frames) - m) * f32(a) + m)


def brightness(frames, a):
    x = x_of(frames)
    V = x.max(axis=-1, keepdims=True)
    V2 = np.minimum(V + f32(a), f32(1.0))
    with np.errstate(divide="ignore", invalid="ignore"):
        s = V2 / V
        scaled = np.minimum(x * s, f32(1.0))
    return np.where(V == 0, np.broadcast_to(V2, x.shape), scaled).astype(f32)


def saturate(frames, a, b):
    x = x_of(frames)
    V, m = x.max(axis=-1, keepdims=True), x.min(axis=-1, keepdims=True)
    with np.errstate(divide="ignore", invalid="ignore"):
        S = np.where(V > 0, (V - m) / V, f32(0.0)).astype(f32)
        S2 = clamp(S * f32(a) + f32(b))
        grey = np.broadcast_to(np.array([0.0, 1.0, 1.0], f32), x.shape)
        k = np.where(V > m, (V - x) / (V - m), grey).astype(f32)
    return clamp(V * (f32(1.0) - S2 * k))


def pixelate(frames, a):
    n, H, W, _ = frames.shape
    hd, cy = cell_map(H, a)
    wd, cx = cell_map(W, a)
    cell = (cy[:, None] * wd + cx[None, :]).ravel()
    count = np.bincount(cell, minlength=hd * wd)
    out = np.empty(frames.shape, f32)
    flat = frames.reshape(n, H * W, 3).astype(np.int64)
    for f in range(n):
        for c in range(3):
            s = np.zeros(hd * wd, np.int64)
            np.add.at(s, cell, flat[f, :, c])
            val = s.astype(f32) / (count * 255).astype(f32)
            out[f, :, :, c] = val[cell].reshape(H, W)
    return out


def gaussian_blur(frames, taps):
    """Row pass, then column pass, replicate borders, float64 on the fp32 taps."""
    t = np.asarray(taps, np.float64)
    R = (t.size - 1) // 2
    n, H, W, _ = frames.shape
    x = x_of(frames).astype(np.float64)
    ix = np.clip(np.arange(-R, W + R), 0, W - 1)
    iy = np.clip(np.arange(-R, H + R), 0, H - 1)
    xp = x[:, :, ix]
    rows = sum(t[k] * xp[:, :, k:k + W] for k in range(2 * R + 1))
    rp = rows[:, iy]
    return clamp(sum(t[k] * rp[:, k:k + H] for k in range(2 * R + 1)))


def defocus_blur(frames, taps):
    """The (2R+1)^2 taps over reflect-101 borders, float64 on the fp32 taps."""
    t = np.asarray(taps, np.float64)
    R = (t.shape[0] - 1) // 2
    n, H, W, _ = frames.shape
    x = x_of(frames).astype(np.float64)
    xp = x[:, reflect101(np.arange(-R, H + R), H)][:, :, reflect101(np.arange(-R, W + R), W)]
    out = np.zeros(x.shape)
    for dy in range(2 * R + 1):
        for dx in range(2 * R + 1):
            out += t[dy, dx] * xp[:, dy:dy + H, dx:dx + W]
    return clamp(out)


def reference(frames, kind, a, b, seed, first_index, lib=None):
    """The reference for (kind, a, b): fp32 for the exact kinds, float64 for speckle and the blurs (which read the library's
    own fp32 taps through ``lib``)."""
    if kind == "impulse_noise":
        return impulse(frames, a, seed, first_index)[0]
    if kind == "speckle_noise":
        return speckle(frames, a, seed, first_index)
    if kind == "contrast":
        return contrast(frames, a)
    if kind == "brightness":
        return brightness(frames, a)
    if kind == "saturate":
        return saturate(frames, a, b)
    if kind == "pixelate":
        return pixelate(frames, a)
    st, taps, _ = lib_taps(lib, kind, a, b)
    assert st == 0
    return gaussian_blur(frames, taps) if kind == "gaussian_blur" else defocus_blur(frames, taps)


SHAPES = ((1, 1, 1), (2, 1, 5), (3, 7, 13), (2, 33, 31), (1, 64, 80))
SEEDS = (0, 0xABCDEF0123, 2 ** 64 - 1)
FIRST_INDEX = 3
SPECIAL_PIXELS = ((0, 0, 0), (255, 255, 255), (128, 128, 128), (255, 0, 0), (0, 255, 0), (0, 0, 255), (1, 1, 1), (255, 255, 0),
                  (0, 255, 255), (254, 255, 255))


def frames_of(shape, seed=11):
    """Random uint8 frames whose first pixels are black, white, grey and the primary colours (as many as fit)."""
    frames = np.random.default_rng(seed).integers(0, 256, tuple(shape) + (3,), dtype=np.uint8)
    flat = frames.reshape(-1, 3)
    k = min(len(SPECIAL_PIXELS), flat.shape[0])
    flat[:k] = np.array(SPECIAL_PIXELS[:k], np.uint8)
    return frames
