"""RISE saliency (include/fav.h fav_rise, fav_rise_record; Petsiuk et al. 2018): the host side of
``Backend.set_rise`` and ``Backend.classify_rise`` - the record unpacking and the descriptor's ranges.

The classifier is a black box: the frames are classified under N random smooth masks, every mask is weighted by the probability
the class got under it, and the weighted masks are summed.  No tap, no backward pass: the map exists for every arch, a deep
ensemble included, and for any class.  What the tests of this package verify is that algebra and its bits on synthetic
checkpoints; where a map peaks is a property of trained weights."""
from __future__ import annotations

from .cam import _unpack_map_records

#: dwords of one fav_rise_record
RISE_RECORD_DWORDS = 8
#: the ranges of a fav_rise descriptor (fav_check_rise is the one place they are enforced)
RISE_MAX_MASKS = 8192
RISE_MAX_GRID = 15
RISE_KEEP_RANGE = (1, 255)
#: the most cells of a map and the longest side, as for the curves
RISE_MAX_CELLS = 1024
RISE_MAX_SIDE = 256


def unpack_rise_records(records) -> dict:
    """int32[..., 8] fav_rise_record records (torch tensor or numpy) -> ``class_id`` int32, ``p_full`` (the class probability
    on the unmasked frame), ``peak`` fp32, ``peak_cell`` int32, ``floor``, ``p_mean`` (its mean over the masks) fp32,
    ``n_above`` int32 (cells at the midpoint between floor and peak or above), ``box`` int32 (packed; -1: none), each [...] and
    a view of the record buffer, plus the box unpacked to ``x0``, ``y0``, ``x1``, ``y1`` (int32, inclusive map cells; all -1
    when the box is -1)."""
    return _unpack_map_records(records, ("class_id", "p_full", "peak", "peak_cell", "floor", "p_mean", "n_above", "box"))


def keep_threshold(keep: float) -> int:
    """The probability that a grid cell is ON -> the descriptor's ``keep``, in 256ths: round(256 keep)."""
    return int(round(256.0 * float(keep)))
