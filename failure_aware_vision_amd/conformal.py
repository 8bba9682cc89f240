"""Split-conformal prediction sets over the confidence head's mean distribution pbar (include/fav.h fav_conformal /
fav_pred_set).

Calibrate once on held-out labelled frames (``Backend.calibrate_conformal``): the score of each frame's true class is
computed on the GPU, and ``calibrate_qhat`` takes the ceil((n+1)(1-alpha))-th smallest.  After that every frame gets a
set of classes (``Backend.classify_sets``) that holds the true class with probability >= 1 - alpha, for any model, as
long as calibration and test frames are exchangeable.  A set of size 1 means the model commits; a larger or an empty
set means it does not.
"""
from __future__ import annotations

import ctypes as C
import dataclasses
import math

import numpy as np

from . import _lib

#: dwords of one fav_pred_set record (include/fav.h)
PRED_SET_DWORDS = 40
#: fav_cp_score by name
SCORE_KINDS = {"lac": _lib.CP_LAC, "aps": _lib.CP_APS, "raps": _lib.CP_APS}


@dataclasses.dataclass(frozen=True)
class Conformal:
    """A conformal score and its threshold.  ``kind``: "lac" (s = 1 - pbar[c]) or "aps" (s = u pbar[c] + mass ahead of c,
    plus ``lam`` * max(0, rank + 1 - ``k_reg``): RAPS when ``lam`` > 0).  ``randomized``: u is a per-frame Philox draw
    keyed by (``seed``, global frame index) instead of 1.  ``qhat``: the calibrated threshold (+inf: every class)."""
    kind: str = "aps"
    randomized: bool = False
    lam: float = 0.0
    k_reg: int = 0
    qhat: float = math.inf
    seed: int = 0

    def to_c(self) -> _lib.FavConformal:
        if self.kind not in SCORE_KINDS:
            raise ValueError(f"unknown conformal score kind {self.kind!r} (one of {sorted(SCORE_KINDS)})")
        c = _lib.FavConformal()
        c.struct_size = C.sizeof(_lib.FavConformal)
        c.score_kind = SCORE_KINDS[self.kind]
        c.randomized = 1 if self.randomized else 0
        c.k_reg = int(self.k_reg)
        c.lambda_ = float(self.lam)
        c.qhat = float(self.qhat)
        c.seed = int(self.seed) & 0xFFFFFFFFFFFFFFFF
        return c


def calibrate_qhat(scores, alpha: float) -> float:
    """The split-conformal threshold: the ceil((n+1)(1-alpha))-th smallest of the n calibration scores, +inf when that
    rank exceeds n (too few frames for this alpha).  NaN scores (a label outside the classes) and alpha outside (0, 1)
    are rejected."""
    alpha = float(alpha)
    if not 0.0 < alpha < 1.0:
        raise ValueError(f"alpha must lie in (0, 1), got {alpha}")
    s = np.asarray(scores, np.float32).ravel()
    if s.size == 0:
        raise ValueError("no calibration scores")
    if np.isnan(s).any():
        raise ValueError(f"{int(np.isnan(s).sum())} calibration scores are NaN (labels outside [0, num_classes), or non-finite frames?)")
    n = s.size
    k = math.ceil((n + 1) * (1.0 - alpha))
    if k > n:
        return math.inf
    return float(np.partition(s, k - 1)[k - 1])


def unpack_sets(records, num_classes: int = 1024) -> dict:
    """int32[n, 40] fav_pred_set records (torch tensor on any device, or numpy) -> dict: ``label`` int32[n],
    ``confidence`` / ``set_mass`` / ``u`` fp32[n] (views of the records), ``set_size`` int32[n] and ``members``
    bool[n, num_classes] (class c in the set: bit c % 32 of member word c / 32)."""
    if not 1 <= int(num_classes) <= 1024:
        raise ValueError(f"num_classes must lie in [1, 1024], got {num_classes}")
    if records.ndim != 2 or int(records.shape[1]) != PRED_SET_DWORDS:
        raise ValueError(f"expected int32[n, {PRED_SET_DWORDS}] records, got shape {tuple(records.shape)}")
    if isinstance(records, np.ndarray):
        if records.dtype != np.int32:
            raise TypeError(f"records must be int32, got {records.dtype}")
        words = records[:, 8:40].view(np.uint32)
        bits = (words[:, :, None] >> np.arange(32, dtype=np.uint32)) & np.uint32(1)
        members = bits.reshape(records.shape[0], 1024)[:, :int(num_classes)].astype(bool)
        f32 = np.float32
    else:
        import torch
        if records.dtype != torch.int32:
            raise TypeError(f"records must be int32, got {records.dtype}")
        shifts = torch.arange(32, dtype=torch.int32, device=records.device)
        members = ((records[:, 8:40, None] >> shifts) & 1).reshape(records.shape[0], 1024)[:, :int(num_classes)].to(torch.bool)
        f32 = torch.float32
    return {"label": records[:, 0], "confidence": records[:, 1].view(f32), "set_size": records[:, 2],
            "set_mass": records[:, 3].view(f32), "u": records[:, 4].view(f32), "members": members}
