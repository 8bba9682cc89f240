"""What the numpy restatements of the two localisation heads share (tests/cam_ref.py, tests/rollout_ref.py): the comparison of
bits, and the last step of either record - the cells of a map at or above a threshold and the box around them.  Each head's
threshold rule and its scans stay in its own restatement."""
import numpy as np


def same_bits(a, b) -> bool:
    """Equal shapes, equal bits wherever neither value is a NaN, and NaNs in the same places."""
    a, b = np.asarray(a), np.asarray(b)
    if a.shape != b.shape or a.dtype != b.dtype:
        return False
    if a.dtype != np.float32:
        return bool(np.array_equal(a, b))
    na, nb = np.isnan(a), np.isnan(b)
    return bool(np.array_equal(na, nb) and np.array_equal(a.view(np.uint32)[~na], b.view(np.uint32)[~nb]))


def cells_above(m, thr, width):
    """(n_above, box) of the cells of a map m float32 [cells], rows of ``width`` cells, with m >= thr (a NaN is not one): the
    inclusive box of ALL such cells, x0 | y0 << 8 | x1 << 16 | y1 << 24 as an int32, -1 when there is none."""
    cells = np.nonzero(m >= thr)[0]
    if not cells.size:
        return 0, -1
    xs, ys = cells % width, cells // width
    packed = int(xs.min()) | int(ys.min()) << 8 | int(xs.max()) << 16 | int(ys.max()) << 24
    return int(cells.size), packed - (1 << 32) if packed >= 1 << 31 else packed
