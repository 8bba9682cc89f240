"""Class activation maps (include/fav.h fav_cam_record; Zhou et al. 2016): the host side of
``Backend.cam`` and ``Backend.classify_cam`` - the record unpacking, the map box in input pixels, and the share of a map's
positive evidence that falls inside a caller's box (a pointing-game-style measure for robustness reports).

On a ResNet the logit of class c is the spatial mean of ``w_c . F(h, w)`` over the last feature map plus the bias, so the map
``M_c(h, w) = w_c . F(h, w)`` decomposes the logit over image regions exactly.  What the tests of this package verify is that
algebra and its bits; whether the maps localise objects depends on the trained weights."""
from __future__ import annotations

import numpy as np

#: dwords of one fav_cam_record
CAM_RECORD_DWORDS = 8
#: the most classes a frame one call of the head takes
CAM_MAX_CLASSES = 8


def _unpack_fields(records, names) -> tuple:
    """int32[..., len(names)] records (torch tensor or numpy) -> (the fields under ``names``, each [...] and a view of the record
    buffer - dwords 1, 2, 4 and 5 as fp32, the others int32, the layout every localisation and curve record has -, the module
    the records are of: numpy or torch)."""
    if records.ndim < 1 or int(records.shape[-1]) != len(names):
        raise ValueError(f"expected int32[..., {len(names)}] records, got shape {tuple(records.shape)}")
    if isinstance(records, np.ndarray):
        xp = np
    else:
        import torch as xp
    return {name: records[..., j].view(xp.float32) if j in (1, 2, 4, 5) else records[..., j] for j, name in enumerate(names)}, xp


def _unpack_map_records(records, names) -> dict:
    """The layout fav_cam_record and fav_rollout_record share, under the eight field ``names`` of one of them: the last is the
    packed box (-1: none), which also comes unpacked to ``x0`` .. ``y1``."""
    out, xp = _unpack_fields(records, names)
    box = out[names[7]]
    none = box == -1
    for name, shift in (("x0", 0), ("y0", 8), ("x1", 16), ("y1", 24)):
        out[name] = xp.where(none, box, (box >> shift) & 0xFF)
    return out


def unpack_cam_records(records) -> dict:
    """int32[..., 8] fav_cam_record records (torch tensor or numpy) -> ``class_id`` int32, ``logit_mean``, ``peak`` fp32,
    ``peak_cell`` int32, ``floor``, ``pos_sum`` fp32, ``n_above`` int32, ``box`` int32 (packed; -1: none), each [...] and a view
    of the record buffer, plus the box unpacked to ``x0``, ``y0``, ``x1``, ``y1`` (int32, inclusive map cells; all -1 when the
    box is -1)."""
    return _unpack_map_records(records, ("class_id", "logit_mean", "peak", "peak_cell", "floor", "pos_sum", "n_above", "box"))


def box_to_pixels(box, in_hw, map_hw):
    """An inclusive box of map cells (x0, y0, x1, y1) -> the half-open pixel box (left, top, right, bottom) it covers in an
    ``in_hw`` = (H, W) frame whose map has ``map_hw`` = (Hf, Wf) cells: cell x spans pixels [x W / Wf, (x + 1) W / Wf), rounded
    outwards.  None for the empty box (any coordinate negative)."""
    x0, y0, x1, y1 = (int(v) for v in box)
    (H, W), (Hf, Wf) = in_hw, map_hw
    if min(x0, y0, x1, y1) < 0:
        return None
    if not (x0 <= x1 < Wf and y0 <= y1 < Hf):
        raise ValueError(f"box {(x0, y0, x1, y1)} does not lie in a {Hf} x {Wf} map")
    return (x0 * W // Wf, y0 * H // Hf, -((-(x1 + 1) * W) // Wf), -((-(y1 + 1) * H) // Hf))


def evidence_share(cam_map, box) -> float:
    """The share of a map's positive evidence - the sum of max(M, 0), the record's ``pos_sum`` - that lies inside the
    inclusive cell box (x0, y0, x1, y1); NaN when the map has no positive evidence.  ``cam_map``: [Hf, Wf]."""
    m = np.asarray(cam_map.cpu() if hasattr(cam_map, "cpu") else cam_map, np.float64)
    if m.ndim != 2:
        raise ValueError(f"expected one [Hf, Wf] map, got shape {m.shape}")
    x0, y0, x1, y1 = (int(v) for v in box)
    pos = np.maximum(m, 0.0)
    total = pos.sum()
    if not total > 0:
        return float("nan")
    if min(x0, y0, x1, y1) < 0:
        return 0.0
    return float(pos[y0:y1 + 1, x0:x1 + 1].sum() / total)
