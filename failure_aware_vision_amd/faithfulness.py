"""Deletion / insertion curves (include/fav.h fav_curve_record; Petsiuk et al. 2018): the host
side of ``Backend.classify_curve`` and ``Backend.faithfulness_report`` - the record unpacking, the random ranking a map is
compared with, and the means a report is made of.

A map's cells are removed from the frame most salient first (deletion) or revealed most salient first on a filled frame
(insertion); the probability of one class is followed over the steps and integrated.  A faithful map gives a LOWER deletion
AUC and a HIGHER insertion AUC than a random ranking of the same cells.  What the tests of this package verify is that algebra
and its bits on synthetic checkpoints, where the sign of a gain carries no meaning; whether a map is faithful is a property of
trained weights."""
from __future__ import annotations

import numpy as np

from .cam import _unpack_fields

#: dwords of one fav_curve_record
CURVE_RECORD_DWORDS = 8
#: the most cells of a map, steps of a curve
CURVE_MAX_CELLS = 1024
CURVE_MAX_STEPS = 256

_FIELDS = ("class_id", "auc", "p_first", "flip_step", "p_last", "p_min", "flip_cells", "reserved")


def unpack_curve_records(records) -> dict:
    """int32[..., 8] fav_curve_record records (torch tensor or numpy) -> ``class_id`` int32, ``auc``, ``p_first`` fp32,
    ``flip_step`` int32 (-1: the label never flipped), ``p_last``, ``p_min`` fp32, ``flip_cells`` int32, each [...] and a view
    of the record buffer."""
    out, _ = _unpack_fields(records, _FIELDS)
    del out["reserved"]
    return out


def random_maps(n: int, map_hw, seed: int = 0) -> np.ndarray:
    """fp32 [n, mh, mw] maps whose ranking is a uniformly random order of the cells, a pure function of ``(n, map_hw, seed)``:
    frame i holds a permutation of 0 .. cells-1, so no two cells tie."""
    mh, mw = (int(v) for v in map_hw)
    if n < 0 or mh < 1 or mw < 1 or mh * mw > CURVE_MAX_CELLS:
        raise ValueError(f"random_maps: n={n}, map {mh}x{mw}: needs n >= 0 and 1 <= mh * mw <= {CURVE_MAX_CELLS}")
    rng = np.random.default_rng(np.random.SeedSequence([0xFA17, int(seed)]))
    out = np.empty((n, mh * mw), dtype=np.float32)
    for i in range(n):
        out[i] = rng.permutation(mh * mw)
    return out.reshape(n, mh, mw)


def summarize_curves(map_del: dict, map_ins: dict, rnd_del: dict, rnd_ins: dict, cells: int) -> dict:
    """The four per-frame results of ``Backend.classify_curve`` (a map and a random ranking, deletion and insertion; numpy) ->
    the report: mean ``deletion_auc``, ``insertion_auc``, ``random_deletion_auc``, ``random_insertion_auc``, ``deletion_gain`` =
    random - map, ``insertion_gain`` = map - random, ``flip_fraction`` the mean of flip_cells / cells under deletion over the
    frames whose label flipped (NaN when none did).  A frame with a NaN AUC in any of the four is left out of every mean and
    counted in ``n_nonfinite``; ``n`` is the number of frames kept."""
    aucs = [np.asarray(r["auc"], dtype=np.float32) for r in (map_del, map_ins, rnd_del, rnd_ins)]
    keep = np.ones(aucs[0].shape, dtype=bool)
    for a in aucs:
        keep &= ~np.isnan(a)

    def mean(a):
        return float(np.mean(a[keep].astype(np.float64))) if keep.any() else float("nan")

    d, i, rd, ri = (mean(a) for a in aucs)
    fc = np.asarray(map_del["flip_cells"])
    flipped = keep & (fc >= 0)
    return dict(deletion_auc=d, insertion_auc=i, random_deletion_auc=rd, random_insertion_auc=ri,
                deletion_gain=rd - d, insertion_gain=i - ri,
                flip_fraction=float(np.mean(fc[flipped].astype(np.float64) / cells)) if flipped.any() else float("nan"),
                n=int(keep.sum()), n_nonfinite=int((~keep).sum()))
