"""Attention rollout (include/fav.h fav_rollout_record; Abnar & Zuidema 2020): the host side of
``Backend.rollout`` and ``Backend.classify_rollout`` - the record unpacking and the patch box in input pixels.

Each encoder layer's attention is averaged over its heads, mixed half and half with the identity for the residual connection,
and the layers are multiplied together; the class token's row of the product says how much each patch fed the decision.  What
the tests of this package verify is that algebra and its bits on synthetic checkpoints; whether the maps localise objects is a
property of trained weights."""
from __future__ import annotations

from .cam import _unpack_map_records

#: dwords of one fav_rollout_record
ROLLOUT_RECORD_DWORDS = 8
#: the patch side of both ViT arches (include/fav.h FAV_ARCH_VIT_B16, FAV_ARCH_VIT_TINY)
VIT_PATCH = 16


def unpack_rollout_records(records) -> dict:
    """int32[..., 8] fav_rollout_record records (torch tensor or numpy) -> ``n_layers`` int32, ``cls_mass``, ``peak`` fp32,
    ``peak_cell`` int32, ``floor``, ``patch_sum`` fp32, ``n_above`` int32 (cells at the midpoint between floor and peak or
    above), ``box`` int32 (packed; -1: none), each [...] and a view of the record buffer, plus the box unpacked to ``x0``,
    ``y0``, ``x1``, ``y1`` (int32, inclusive patch cells; all -1 when the box is -1)."""
    return _unpack_map_records(records, ("n_layers", "cls_mass", "peak", "peak_cell", "floor", "patch_sum", "n_above", "box"))


def patch_box_to_pixels(box, patch: int = VIT_PATCH):
    """An inclusive box of patch cells (x0, y0, x1, y1) -> the half-open pixel box (left, top, right, bottom) it covers: patch
    x spans pixels [x * patch, (x + 1) * patch).  None for the empty box (any coordinate negative)."""
    x0, y0, x1, y1 = (int(v) for v in box)
    if min(x0, y0, x1, y1) < 0:
        return None
    if not (x0 <= x1 and y0 <= y1) or patch < 1:
        raise ValueError(f"box {(x0, y0, x1, y1)} with patch {patch} is not a box of patch cells")
    return (x0 * patch, y0 * patch, (x1 + 1) * patch, (y1 + 1) * patch)
