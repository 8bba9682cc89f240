"""Attention rollout (include/fav.h fav_rollout_record; Abnar & Zuidema 2020): the host side of
``Backend.rollout`` and ``Backend.classify_rollout`` - the record unpacking and the patch box in input pixels.

Each encoder layer's attention is averaged over its heads, mixed half and half with the identity for the residual connection,
and the layers are multiplied together; the class token's row of the product says how much each patch fed the decision.  What
the tests of this package verify is that algebra and its bits on synthetic checkpoints; whether the maps localise objects is a
property of trained weights."""
from __future__ import annotations

import numpy as np

#: dwords of one fav_rollout_record
ROLLOUT_RECORD_DWORDS = 8
#: the patch side of both ViT arches (include/fav.h FAV_ARCH_VIT_B16, FAV_ARCH_VIT_TINY)
VIT_PATCH = 16


def unpack_rollout_records(records) -> dict:
    """int32[..., 8] fav_rollout_record records (torch tensor or numpy) -> ``n_layers`` int32, ``cls_mass``, ``peak`` fp32,
    ``peak_cell`` int32, ``floor``, ``patch_sum`` fp32, ``n_above`` int32 (cells at the midpoint between floor and peak or
    above), ``box`` int32 (packed; -1: none), each [...] and a view of the record buffer, plus the box unpacked to ``x0``,
    ``y0``, ``x1``, ``y1`` (int32, inclusive patch cells; all -1 when the box is -1)."""
    if records.ndim < 1 or int(records.shape[-1]) != ROLLOUT_RECORD_DWORDS:
        raise ValueError(f"expected int32[..., {ROLLOUT_RECORD_DWORDS}] records, got shape {tuple(records.shape)}")
    if isinstance(records, np.ndarray):
        f32 = np.float32
        where = np.where
    else:
        import torch
        f32 = torch.float32
        where = torch.where
    box = records[..., 7]
    none = box == -1
    out = {"n_layers": records[..., 0], "cls_mass": records[..., 1].view(f32), "peak": records[..., 2].view(f32),
           "peak_cell": records[..., 3], "floor": records[..., 4].view(f32), "patch_sum": records[..., 5].view(f32),
           "n_above": records[..., 6], "box": box}
    for name, shift in (("x0", 0), ("y0", 8), ("x1", 16), ("y1", 24)):
        out[name] = where(none, box, (box >> shift) & 0xFF)
    return out


def patch_box_to_pixels(box, patch: int = VIT_PATCH):
    """An inclusive box of patch cells (x0, y0, x1, y1) -> the half-open pixel box (left, top, right, bottom) it covers: patch
    x spans pixels [x * patch, (x + 1) * patch).  None for the empty box (any coordinate negative)."""
    x0, y0, x1, y1 = (int(v) for v in box)
    if min(x0, y0, x1, y1) < 0:
        return None
    if not (x0 <= x1 and y0 <= y1) or patch < 1:
        raise ValueError(f"box {(x0, y0, x1, y1)} with patch {patch} is not a box of patch cells")
    return (x0 * patch, y0 * patch, (x1 + 1) * patch, (y1 + 1) * patch)
