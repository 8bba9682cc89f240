"""Plain numpy statement of the MC-Dropout descriptor (include/fav.h fav_dropout_desc), written from
the documented contract alone, and the descriptors of the dropout edge tests (tests/test_dropout_ref_host.py checks the
reference on the CPU, tests/test_gpu_pool_dropout_edges.py every kernel that draws a mask against it, bit for bit).

Contract.  Row r of a launch is virtual frame v = v0 + r: sample t = v // n_img of frame i = v % n_img, whose global index
is first_image_index + i; only the low 32 bits of that index enter the counter.  Element e of the row draws byte e % 16
(little endian over the four words) of Philox4x32-10(counter = (e // 16, frame, t, site), key = (seed low, seed high)) and
is kept iff the byte is >= threshold.  A kept value is bf16(fp32(x) * scale), a dropped one +0.

All index arithmetic is done in Python integers and reduced mod 2^32 BEFORE it meets a numpy type: the edges are exactly
the values numpy's casts refuse."""
from collections import namedtuple

import numpy as np

from oracle import fav_oracle as O

M32 = 1 << 32
V_MAX = (1 << 31) - 1            # v0 + rows may reach this and no more: the kernels hold v and t in 32 bits

# rows: the launch's row count (n_frames of a conv / tail / average pool, n_out of the entry ops)
Desc = namedtuple("Desc", "name site threshold seed v0 n_img first_image_index rows")


def scale_of(threshold):
    """fp32(1 / (1 - threshold/256)); 1 at threshold 0 (site enabled, nothing dropped)."""
    return np.float32(1.0 / (1.0 - threshold / 256.0)) if threshold > 0 else np.float32(1.0)


def row_index(desc, row):
    """(t, i, frame) of row `row`: sample, frame inside the batch, the 32-bit frame word of the counter."""
    v = int(desc.v0) + int(row)
    t, i = divmod(v, int(desc.n_img))
    return t, i, (int(desc.first_image_index) + i) % M32


def draws(desc, row, n_elem):
    """The 8-bit draws of the first n_elem elements of row `row`, uint32 [n_elem]."""
    t, _, frame = row_index(desc, row)
    seed = int(desc.seed)
    n_chunks = (int(n_elem) + 15) // 16
    assert 0 <= t < M32 and 0 <= int(desc.site) < M32 and n_chunks <= M32
    chunk = np.arange(n_chunks, dtype=np.uint64).astype(np.uint32)
    w = O.philox4x32_10(chunk, np.uint32(frame), np.uint32(t), np.uint32(int(desc.site)), seed % M32, (seed >> 32) % M32)
    d = np.empty((n_chunks, 16), np.uint32)
    for q in range(4):
        for b in range(4):
            d[:, 4 * q + b] = (w[q] >> np.uint32(8 * b)) & np.uint32(0xFF)
    return d.reshape(-1)[:n_elem]


def keep_mask(desc, row, n_elem):
    """bool [n_elem]: element e of row `row` is kept."""
    return draws(desc, row, n_elem) >= np.uint32(int(desc.threshold))


def apply(desc, row, x):
    """One row through the site: x fp32 (any shape, flattened in memory order) -> bf16(x * scale) where kept, +0 elsewhere."""
    x = np.ascontiguousarray(x, np.float32)
    keep = keep_mask(desc, row, x.size).reshape(x.shape)
    return np.where(keep, O.bf16_round(x * scale_of(desc.threshold)), np.float32(0.0)).astype(np.float32)


def apply_rows(desc, x_rows):
    """x_rows [rows, ...]: row r of the launch through the site."""
    return np.stack([apply(desc, r, x_rows[r]) for r in range(len(x_rows))])


def _d(name, site=3, threshold=64, seed=0x1234567890ABCDEF, v0=0, n_img=3, first=40, rows=3):
    return Desc(name, site, threshold, seed, v0, n_img, first, rows)


# One descriptor per edge; whatever an entry does not name is an ordinary value.  Both test files run the whole list.
EDGE_DESCRIPTORS = [
    _d("thr0", threshold=0),                                   # site enabled, nothing dropped, scale 1
    _d("thr1", threshold=1),
    _d("thr128", threshold=128),
    _d("thr255", threshold=255),                               # one draw in 256 survives, scale 256
    _d("seed0", seed=0),
    _d("seed_2p32m1", seed=M32 - 1),                           # high key word 0
    _d("seed_2p32", seed=M32),                                 # low key word 0
    _d("seed_2p64m1", seed=(1 << 64) - 1),
    _d("site0", site=0),
    _d("site16", site=16),
    _d("site_2p31m1", site=(1 << 31) - 1),
    _d("first0", first=0),
    _d("first_2p32m2", first=M32 - 2, n_img=4, rows=4),        # frame words 2^32-2, 2^32-1, 0, 1: the wrap inside the launch
    _d("first_2p40p5", first=(1 << 40) + 5),                   # only the low 32 bits count
    _d("n_img1", n_img=1, v0=5, rows=4),                       # every row a new sample
    _d("v0_unaligned", n_img=3, v0=7, rows=5),                 # starts and ends inside a sample
    _d("window_wraps", n_img=3, v0=2, rows=2),                 # rows < n_img across a sample boundary: frames 2 and 0
    _d("v_max", n_img=3, v0=V_MAX - 4, rows=4),                # v0 + rows = 2^31 - 1, the largest accepted index
    _d("v_max_n_img1", n_img=1, v0=V_MAX - 3, rows=3),         # ... with t = v: the largest sample index
]
EDGE_IDS = [d.name for d in EDGE_DESCRIPTORS]
