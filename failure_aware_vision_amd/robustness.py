"""Robustness report: what the confidence is worth as a corruption gets worse.

``Backend.robustness_report`` corrupts labelled frames on the device (``Corruptor.imagenet_c``) for every (kind, severity),
classifies each corrupted set with a one-temperature sweep and hands the result to ``summarize``; ``table`` renders the rows.
This module is the host side, numpy only; importing it needs no GPU."""
from __future__ import annotations

import math

import numpy as np

from .calibration import risk_coverage

#: the keys of a row, in the order ``table`` prints them
COLUMNS = ("accuracy", "mean_confidence", "nll", "aurc", "fail_rate", "error_recall", "flag_precision")


def summarize(pred, conf, nll, labels, tau) -> dict:
    """One row of the report from per-frame predictions, confidences, negative log-likelihoods and true labels:
    ``accuracy``, ``mean_confidence``, ``nll`` (float64 means), ``aurc`` (``calibration.risk_coverage``), ``fail_rate`` (the
    share with conf < tau), ``error_recall`` (the share of wrong frames that are flagged; NaN when nothing is wrong) and
    ``flag_precision`` (the share of flagged frames that are wrong; NaN when nothing is flagged)."""
    pred, labels = np.asarray(pred).ravel(), np.asarray(labels).ravel()
    conf = np.asarray(conf, np.float32).ravel()
    nll = np.asarray(nll, np.float32).ravel()
    if not (pred.shape == labels.shape == conf.shape == nll.shape) or pred.size == 0:
        raise ValueError("pred, conf, nll and labels must be non-empty and of one length")
    correct = pred == labels
    wrong = ~correct
    flagged = conf < np.float32(tau)
    n_wrong, n_flagged = int(wrong.sum()), int(flagged.sum())
    hit = int((wrong & flagged).sum())
    return {"accuracy": float(correct.mean()), "mean_confidence": float(conf.astype(np.float64).mean()),
            "nll": float(nll.astype(np.float64).mean()), "aurc": risk_coverage(conf, correct)["aurc"],
            "fail_rate": n_flagged / pred.size,
            "error_recall": hit / n_wrong if n_wrong else math.nan,
            "flag_precision": hit / n_flagged if n_flagged else math.nan}


def table(rows) -> str:
    """``{(kind, severity): summarize(...)}`` (as ``Backend.robustness_report`` returns it) -> a text table, one line a row."""
    head = f"{'corruption':<16}{'sev':>4}" + "".join(f"{c:>16}" for c in COLUMNS)
    lines = [head, "-" * len(head)]
    for (kind, sev), row in rows.items():
        lines.append(f"{kind:<16}{sev:>4}" + "".join(f"{row[c]:>16.4f}" for c in COLUMNS))
    return "\n".join(lines)
