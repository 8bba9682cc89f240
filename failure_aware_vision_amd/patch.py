"""Patch-level anomaly maps (include/fav.h fav_patch_bank, fav_patch_record; PatchCore, Roth et
al. 2022): the host side of ``Backend.fit_patch_bank``, ``set_patch_bank`` and ``classify_patch`` - the bank of in-distribution
patch features, how it is made from tapped feature maps, and the record unpacking.

The feature-space heads (``ood.py``) see a frame through the average pool, which dilutes a local fault 49 to 1 on a 7 x 7 map;
the localisation heads (``cam.py``, ``rollout.py``, ``rise.py``) explain the classifier's decision, not the frame's novelty.
Here every cell of the last feature map is scored on its own: the squared distance of its normalised feature to the nearest
row of a bank of in-distribution cells.  The map of those distances is an anomaly heat map and its peak a frame score.

The bank is a subsample of the cells: by default a seeded random draw, with ``select="coreset"`` PatchCore's greedy k-centre
selection, run on the device (``coreset.py``; item 5n), which covers the feature space where a draw samples its density - a
rare in-distribution texture keeps a row and stops being reported as an anomaly."""
from __future__ import annotations

import ctypes as C
import dataclasses
import math

import numpy as np

from . import _lib
from .coreset import check_select, select_coreset
from .ood import _bf16_bits, _check, _subsample, _subsample_count, _take_indices

#: dwords of one fav_patch_record (include/fav.h)
PATCH_RECORD_DWORDS = 8
_FIELDS = ("n_degenerate", "mean_dist", "peak", "peak_cell", "floor", "peak_row", "n_above", "box")
_FLOAT_DWORDS = (1, 2, 4)


@dataclasses.dataclass(frozen=True)
class PatchBank:
    """``rows`` uint16[N, D]: L2-normalised in-distribution patch features as bf16 bit patterns; ``threshold``: a cell counts
    as above when dist >= threshold (+inf: never); ``chunk_rows``: the bank rows one slab of similarities covers, 0 for the
    library's rule (nothing in a result depends on it); ``grid``: the (hf, wf) map the rows were cut from, or None;
    ``n_dropped``: the zero and non-finite cells ``build_patch_bank`` left out; ``selection``: the
    ``coreset.CoresetSelection`` that chose the rows (``select="coreset"``; its indices count the cells that were not dropped),
    else None; it is not saved; ``stage``, ``radius``: the site the rows were cut at (fav_patch_site) - the
    residual stage 1 .. 4 whose map the stage tap holds, None: the last map, through the map tap - and the half width 0 .. 2
    of the neighbourhood every cell was aggregated over (``aggregate_cells``).  Both are saved when they are not the defaults."""
    rows: np.ndarray
    threshold: float = math.inf
    chunk_rows: int = 0
    grid: tuple | None = None
    n_dropped: int = 0
    selection: object | None = None
    stage: int | None = None
    radius: int = 0

    def __post_init__(self):
        if np.asarray(self.rows).dtype != np.uint16:
            raise ValueError("rows are bf16 bit patterns: uint16 (build_patch_bank makes them from feature maps)")
        object.__setattr__(self, "rows", np.ascontiguousarray(self.rows, np.uint16))
        object.__setattr__(self, "threshold", float(self.threshold))
        object.__setattr__(self, "chunk_rows", int(self.chunk_rows))
        object.__setattr__(self, "n_dropped", int(self.n_dropped))
        if self.grid is not None:
            object.__setattr__(self, "grid", (int(self.grid[0]), int(self.grid[1])))
        if self.rows.ndim != 2:
            raise ValueError("rows is a matrix [N, D]")
        object.__setattr__(self, "stage", None if self.stage is None else int(self.stage))
        object.__setattr__(self, "radius", int(self.radius))
        if self.stage is None and self.radius != 0:
            raise ValueError("a neighbourhood radius needs a stage (stage=4 is the last map)")

    @property
    def N(self) -> int:
        return int(self.rows.shape[0])

    @property
    def D(self) -> int:
        return int(self.rows.shape[1])

    def with_threshold(self, threshold: float) -> "PatchBank":
        return dataclasses.replace(self, threshold=float(threshold))

    def take(self, indices) -> "PatchBank":
        """The bank of the rows ``indices`` (in that order); ``threshold``, ``chunk_rows``, ``grid`` and ``n_dropped`` are kept."""
        return PatchBank(self.rows[_take_indices(indices, self.N)], self.threshold, self.chunk_rows, self.grid, self.n_dropped,
                         stage=self.stage, radius=self.radius)

    def save(self, path):
        extra = {} if self.grid is None else {"grid": np.asarray(self.grid, np.int32)}
        if self.stage is not None:                     # a plain bank's file keeps the keys it always had
            extra.update(stage=np.int32(self.stage), radius=np.int32(self.radius))
        np.savez(path, rows=self.rows, threshold=np.float32(self.threshold), chunk_rows=np.int32(self.chunk_rows),
                 n_dropped=np.int64(self.n_dropped), **extra)

    @classmethod
    def load(cls, path) -> "PatchBank":
        with np.load(path) as z:
            grid = tuple(int(v) for v in z["grid"]) if "grid" in z.files else None
            stage = int(z["stage"]) if "stage" in z.files else None
            radius = int(z["radius"]) if "radius" in z.files else 0
            return cls(z["rows"], float(z["threshold"]), int(z["chunk_rows"]), grid, int(z["n_dropped"]), stage=stage, radius=radius)

    def site_to_c(self):
        """The fav_patch_site of this bank, None for a plain bank (``stage`` None)."""
        if self.stage is None:
            return None
        s = _lib.FavPatchSite()
        s.struct_size = C.sizeof(_lib.FavPatchSite)
        s.stage, s.radius = self.stage, self.radius
        return s

    def to_c(self) -> _lib.FavPatchBank:
        """The fav_patch_bank that points into this bank's rows (which it keeps alive)."""
        b = _lib.FavPatchBank()
        b.struct_size = C.sizeof(_lib.FavPatchBank)
        b.D, b.N, b.chunk_rows = self.D, self.N, self.chunk_rows
        b.rows = self.rows.ctypes.data_as(C.POINTER(C.c_uint16))
        b.threshold = self.threshold
        b._keep = self
        return b

    def check(self, D_expected: int = -1):
        """fav_check_patch_bank (host only); raises ValueError with the library's message."""
        _check("fav_check_patch_bank", self.to_c(), D_expected)


def _maps_f64(maps) -> np.ndarray:
    """bf16 maps as a torch tensor, as uint16 bit patterns or as numpy floats -> float64, same shape."""
    if hasattr(maps, "detach"):
        import torch
        return maps.detach().to(device="cpu", dtype=torch.float64).numpy()
    a = np.asarray(maps)
    if a.dtype == np.uint16:
        return (a.astype(np.uint32) << 16).view(np.float32).astype(np.float64)
    return a.astype(np.float64)


def aggregate_cells(maps, radius: int) -> np.ndarray:
    """maps [S, n, Hf, Wf, C] (bf16 torch tensor, uint16 bits or floats) -> float32 [n, Hf, Wf, C]: steps 1 to 3 of the
    contract beside fav_patch_site in their order, one float32 rounding an operation - the mean over the samples (the sum in
    sample order, times float32(1 / S)), the sum down the 2 radius + 1 rows around a cell, then along the 2 radius + 1 columns,
    rows and columns outside the map skipped.  No division by the count: the normalisation that follows removes it."""
    radius = int(radius)
    if radius < 0 or radius > 2:
        raise ValueError(f"radius={radius} outside [0, 2]")
    x = _maps_f64(maps).astype(np.float32)
    if x.ndim != 5 or x.shape[0] < 1:
        raise ValueError(f"maps must be [S, n, Hf, Wf, C], got shape {x.shape}")
    S, n, Hf, Wf, Cc = x.shape
    with np.errstate(all="ignore"):
        m = np.zeros(x.shape[1:], np.float32)
        for s in range(S):
            m = m + x[s]
        m = m * np.float32(1.0 / S)
        v = np.zeros_like(m)
        for d in range(-radius, radius + 1):
            lo, hi = max(0, -d), min(Hf, Hf - d)                 # the rows y with y + d inside the map
            if lo < hi:
                v[:, lo:hi] = v[:, lo:hi] + m[:, lo + d:hi + d]
        a = np.zeros_like(m)
        for d in range(-radius, radius + 1):
            lo, hi = max(0, -d), min(Wf, Wf - d)
            if lo < hi:
                a[:, :, lo:hi] = a[:, :, lo:hi] + v[:, :, lo + d:hi + d]
    assert a.dtype == np.float32
    return a


def cell_rows(maps, radius: int | None = None):
    """maps [S, n, HW, C] or [S, n, Hf, Wf, C] -> (rows uint16 [n * HW, C], ok bool [n * HW], grid or None): the mean over the
    samples of every cell, divided by its Euclidean norm in float64, rounded to bf16 (nearest even).  ``ok`` is False for a
    cell that has no direction - a zero cell, a non-finite value - whose row is all zero.  ``radius`` (not None; the maps with
    both map axes): every cell is first replaced by ``aggregate_cells`` of its neighbourhood."""
    if radius is not None:
        maps = aggregate_cells(maps, radius)[None]
    x = _maps_f64(maps)
    if x.ndim not in (4, 5) or x.shape[0] < 1:
        raise ValueError(f"maps must be [S, n, HW, C] or [S, n, Hf, Wf, C], got shape {x.shape}")
    grid = (int(x.shape[2]), int(x.shape[3])) if x.ndim == 5 else None
    with np.errstate(all="ignore"):
        f = x.mean(axis=0).reshape(-1, x.shape[-1])
        norm = np.sqrt((f * f).sum(axis=1))
        ok = np.isfinite(f).all(axis=1) & (norm > 0) & np.isfinite(norm)
        unit = np.where(ok[:, None], f / np.where(ok, norm, 1.0)[:, None], 0.0)
    return _bf16_bits(unit.astype(np.float32)), ok, grid


def bank_from_rows(rows, ok, max_rows: int | None = None, seed: int = 0, grid=None, threshold: float = math.inf,
                   chunk_rows: int = 0, select: str = "random", device=None, stage=None, radius: int = 0) -> PatchBank:
    """What ``cell_rows`` made, of one batch or of several concatenated -> the bank: the cells without a direction dropped
    and counted, then ``max_rows`` of the rest kept in their original order, chosen as ``ood.build_knn_bank`` chooses them:
    ``select="random"`` draws them without replacement by ``np.random.default_rng(seed)``; ``select="coreset"`` picks them by
    ``coreset.select_coreset(rows, max_rows, seed)`` on ``device`` and keeps the picks and the coverage curve in
    ``bank.selection`` (``max_rows`` None or at least the cells there are: everything is kept and no device touched)."""
    check_select(select)
    rows, ok = np.asarray(rows, np.uint16), np.asarray(ok, bool)
    if rows.ndim != 2 or ok.shape != (rows.shape[0],):
        raise ValueError(f"shapes do not fit: rows {rows.shape}, ok {ok.shape}")
    kept = rows[ok]
    if kept.shape[0] < 1:
        raise ValueError("no cell has a direction: every one is zero or non-finite")
    if select == "coreset" and _subsample_count(kept.shape[0], max_rows) is not None:
        selection = select_coreset(kept, int(max_rows), seed, device=device)
        full = PatchBank(kept, threshold, chunk_rows, grid, int((~ok).sum()), stage=stage, radius=radius)
        return dataclasses.replace(full.take(selection.indices), selection=selection)
    kept, _ = _subsample(kept, max_rows, seed)
    return PatchBank(kept, threshold, chunk_rows, grid, int((~ok).sum()), stage=stage, radius=radius)


def build_patch_bank(maps, max_rows: int | None = None, seed: int = 0, **kw) -> PatchBank:
    """bf16 feature maps [S, n, HW, C] (or [S, n, Hf, Wf, C], as ``Backend.maps()`` gives them) of in-distribution frames ->
    the bank: ``bank_from_rows`` of ``cell_rows``.  ``bank.n_dropped`` counts the zero and non-finite cells left out.  The
    subsample is random by default; ``select="coreset"`` (and ``device``) makes it the greedy k-centre selection."""
    rows, ok, grid = cell_rows(maps)
    kw.setdefault("grid", grid)
    return bank_from_rows(rows, ok, max_rows, seed, **kw)


def unpack_patch_records(records) -> dict:
    """int32[..., 8] fav_patch_record records (torch tensor or numpy) -> ``n_degenerate`` int32, ``mean_dist``, ``peak`` fp32,
    ``peak_cell`` int32, ``floor`` fp32, ``peak_row``, ``n_above``, ``box`` int32 (packed; -1: none), each [...] and a view of the
    record buffer, plus the box unpacked to ``x0``, ``y0``, ``x1``, ``y1`` (inclusive map cells; all -1 when the box is -1) and
    ``anomalous`` = (n_above > 0) | (n_degenerate > 0): a cell at or above the threshold, or one that could not be scored."""
    if records.ndim < 1 or int(records.shape[-1]) != PATCH_RECORD_DWORDS:
        raise ValueError(f"expected int32[..., {PATCH_RECORD_DWORDS}] records, got shape {tuple(records.shape)}")
    if isinstance(records, np.ndarray):
        f32, where = np.float32, np.where
    else:
        import torch
        f32, where = torch.float32, torch.where
    out = {name: records[..., j].view(f32) if j in _FLOAT_DWORDS else records[..., j] for j, name in enumerate(_FIELDS)}
    box = out["box"]
    none = box == -1
    for name, shift in (("x0", 0), ("y0", 8), ("x1", 16), ("y1", 24)):
        out[name] = where(none, box, (box >> shift) & 0xFF)
    out["anomalous"] = (out["n_above"] > 0) | (out["n_degenerate"] > 0)
    return out
