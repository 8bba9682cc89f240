"""Integer reference of the fused signal-statistics pass (include/fav.h fav_signal_stats; signal_stats_kernel), written for
the tests from the definitions alone and independent of oracle/signal_oracle.py: every sum is an integer, the borders are
explicit index arithmetic, and float64 enters only in the four derived numbers at the end."""
import numpy as np


def gray_plane(frame):
    """uint8 BGR [H, W, 3] -> uint8 [H, W]: cv2.COLOR_BGR2GRAY's 8-bit fixed point."""
    f = np.asarray(frame).astype(np.uint32)
    return ((np.uint32(1868) * f[..., 0] + np.uint32(9617) * f[..., 1] + np.uint32(4899) * f[..., 2] + np.uint32(8192))
            >> np.uint32(14)).astype(np.uint8)


def laplacian_i64(gray):
    """4-neighbour Laplacian with reflect-101 borders (index -1 -> 1, H -> H-2, likewise in x), int64 [H, W]."""
    H, W = gray.shape
    g = gray.astype(np.int64)
    y, x = np.arange(H), np.arange(W)
    yu, yd = y - 1, y + 1
    yu[0], yd[H - 1] = 1, H - 2
    xl, xr = x - 1, x + 1
    xl[0], xr[W - 1] = 1, W - 2
    return g[yu, :] + g[yd, :] + g[:, xl] + g[:, xr] - 4 * g


def entropy_f64(hist):
    """Shannon entropy in bits of an integer histogram, float64."""
    h = np.asarray(hist, np.int64)
    n = int(h.sum())
    p = h[h > 0].astype(np.float64) / float(n)
    return float(-(p * np.log2(p)).sum())


def derived(sum_gray, sum_absdiff, sum_lap, sum_lap2, npx, has_prev):
    """The float64 expressions the kernel evaluates from its integer sums: (mean, mean_diff, lap_var)."""
    N = float(npx)
    m = float(sum_lap) / N
    return float(sum_gray) / N, (float(sum_absdiff) / N if has_prev else 0.0), float(sum_lap2) / N - m * m


def frame_stats(frame, prev_gray=None):
    """One frame -> dict with the exact integers (hist, sum_gray, sum_absdiff, sum_lap, sum_lap2, has_prev), the gray
    plane, and the derived float64 numbers (mean, mean_diff, lap_var, entropy).  prev_gray: the preceding gray plane."""
    gray = gray_plane(frame)
    lap = laplacian_i64(gray)
    hist = np.bincount(gray.ravel(), minlength=256).astype(np.int64)
    has_prev = prev_gray is not None
    sum_absdiff = int(np.abs(gray.astype(np.int64) - prev_gray.astype(np.int64)).sum()) if has_prev else 0
    r = {"gray": gray, "hist": hist, "sum_gray": int(gray.astype(np.int64).sum()), "sum_absdiff": sum_absdiff,
         "sum_lap": int(lap.sum()), "sum_lap2": int((lap * lap).sum()), "has_prev": 1 if has_prev else 0}
    r["mean"], r["mean_diff"], r["lap_var"] = derived(r["sum_gray"], sum_absdiff, r["sum_lap"], r["sum_lap2"], gray.size,
                                                      has_prev)
    r["entropy"] = entropy_f64(hist)
    return r


def stream_stats(frames, prev_gray=None):
    """Consecutive frames uint8 [n, H, W, 3] -> list of frame_stats, each diffed against its predecessor."""
    out = []
    for fr in frames:
        out.append(frame_stats(fr, prev_gray))
        prev_gray = out[-1]["gray"]
    return out


# (n, H, W): the smallest frames at which each mechanism of the kernel can break (256 threads a frame, four pixels a dword,
# H*W <= 150000): fewer quads than threads, W == 4 (both x reflections inside one quad), H == 3, exactly one quad a
# thread, ragged last passes, the LDS limit square and at both aspect extremes, and many blocks in one launch.
EDGE_SHAPES = ((1, 3, 4), (5, 3, 8), (4, 5, 12), (3, 16, 64), (3, 17, 60), (2, 300, 500), (1, 3, 50000), (1, 37500, 4),
               (40, 8, 8))
