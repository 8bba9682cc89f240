"""CPU restatement of the reference's live-mode scorer for the tests of
failure_aware_vision_amd/signal.py.  TEST INFRASTRUCTURE ONLY.

PARITY UNPINNED: the reference has no test of SignalAnalyzer and its pixel arithmetic lives
in a third-party dependency that is absent here — opencv-python-headless==4.10.0.84
(platform/backend/requirements.txt:4; call sites signal_analyzer.py:62,65,77,101).  This file
restates OpenCV's published 8-bit semantics for those four calls:

* cv2.cvtColor(BGR2GRAY), uint8: (1868*B + 9617*G + 4899*R + 8192) >> 14
* cv2.Laplacian(gray, CV_64F), ksize=1: kernel [[0,1,0],[1,-4,1],[0,1,0]], BORDER_REFLECT_101
* cv2.absdiff on uint8; cv2.calcHist 256 bins over [0,256) -> float32 counts
and follows signal_analyzer.py:62-143,145-171 for everything after them.
"""
from __future__ import annotations

import numpy as np


def bgr2gray(frame: np.ndarray) -> np.ndarray:
    f = frame.astype(np.uint32)
    return ((1868 * f[..., 0] + 9617 * f[..., 1] + 4899 * f[..., 2] + 8192) >> 14).astype(np.uint8)


def laplacian(gray: np.ndarray) -> np.ndarray:
    g = np.pad(gray.astype(np.float64), 1, mode="reflect")  # numpy 'reflect' == BORDER_REFLECT_101
    return g[:-2, 1:-1] + g[2:, 1:-1] + g[1:-1, :-2] + g[1:-1, 2:] - 4.0 * g[1:-1, 1:-1]


class SignalOracle:
    """signal_analyzer.py:18-171, with the cv2 calls replaced by the functions above."""
    W = (0.35, 0.25, 0.15, 0.25)

    def __init__(self):
        self.prev = None
        self.frozen = 0

    def raw(self, frame):
        gray = bgr2gray(frame)
        lap_var = float(laplacian(gray).var())
        mean = float(np.mean(gray))
        mean_diff = None
        if self.prev is not None:
            mean_diff = float(np.mean(np.abs(self.prev.astype(np.int16) - gray.astype(np.int16)).astype(np.uint8)))
        self.prev = gray.copy()
        hist = np.bincount(gray.ravel(), minlength=256).astype(np.float32)
        p = hist / np.float32(hist.sum())
        p = p[p > 0]
        entropy = float(-np.sum(p * np.log2(p)))
        return gray, lap_var, mean, mean_diff, entropy, np.bincount(gray.ravel(), minlength=256)

    def analyze_frame(self, frame):
        _, lap_var, mean, mean_diff, entropy, _ = self.raw(frame)
        res, self.frozen = score(lap_var, mean, mean_diff, entropy, self.frozen)
        return res


def score(lap_var, mean, mean_diff, entropy, frozen):
    """The scalar half of analyze_frame (signal_analyzer.py:66-143,145-171) on the raw numbers; mean_diff None = first
    frame.  Returns (result dict, new frozen run)."""
    blur = max(0.0, min(1.0, 1.0 - lap_var / 500.0))
    bright = max(0.0, min(1.0, abs(mean - 128.0) / 128.0))
    if mean_diff is not None:
        frozen = frozen + 1 if mean_diff < 1.0 else 0
        freeze = 1.0 if frozen >= 5 else (0.3 * (frozen / 5) if frozen > 0 else 0.0)
    else:
        freeze, mean_diff = 0.0, 10.0
    if entropy < 4.0:
        ent = max(0.0, min(1.0, (4.0 - entropy) / 4.0))
    elif entropy > 7.0:
        ent = max(0.0, min(1.0, (entropy - 7.0) / 1.5))
    else:
        ent = 0.0
    w = SignalOracle.W
    total = max(0.0, min(1.0, w[0] * blur + w[1] * bright + w[2] * freeze + w[3] * ent))
    if mean < 15 or mean > 245:
        status = "VISION_BLANK"
    elif frozen >= 5:
        status = "VISION_FROZEN"
    elif entropy < 2.0 or entropy > 7.5:
        status = "VISION_CORRUPTED"
    else:
        status = "VISION_OK"
    return {"anomaly_score": round(total, 6), "vision_status": status,
            "metrics": {"blur": round(blur, 4), "brightness": round(bright, 4), "freeze": round(freeze, 4),
                        "entropy": round(ent, 4),
                        "raw": {"laplacian_var": round(lap_var, 2), "mean_brightness": round(mean, 1),
                                "frame_diff": round(mean_diff, 2), "entropy": round(entropy, 3)}}}, frozen
