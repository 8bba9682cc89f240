"""Feature-space OOD scoring (include/fav.h fav_ood_model): a class-conditional Gaussian with a
tied covariance on the pooled features the final fc layer reads (Mahalanobis distance; Lee et al. 2018).

The fit is host work in float64 and happens once; the model it produces is a whitening projection ``P`` and the projected
class means ``M``, so that the device head (fav_op_ood_score) computes ``|P (f - mu) - M[c]|^2`` as two plain chains of
fp32 products and sums.  The metrics below are the usual ones for a detector whose score grows with strangeness.

Its non-parametric companion (item 5g; deep nearest neighbours, Sun et al. 2022) is at the end of the file: ``KNNBank``, a bank of
L2-normalised features as bf16 rows that ``build_knn_bank`` makes, scored on the device by fav_op_knn_score as the distance to the
k-th nearest row, with the same metrics.

Behind it (item 5h) what judges a window of frames and not a frame: ``DriftReference``, held-out in-distribution rows made the same
way by ``build_drift_reference``, against which fav_op_drift_test runs a permutation test on the energy distance of a call's frames."""
from __future__ import annotations

import ctypes as C
import dataclasses
import math

import numpy as np

from . import _lib

#: dwords of one fav_ood_record (include/fav.h)
OOD_RECORD_DWORDS = 4
#: dwords of one fav_knn_record
KNN_RECORD_DWORDS = 6

# ---- metrics: a score grows with strangeness; in-distribution frames should score low ------------------------------------------
def _scores(v, name: str) -> np.ndarray:
    s = np.asarray(v, np.float64).ravel()
    if s.size == 0:
        raise ValueError(f"{name} is empty")
    if np.isnan(s).any():
        raise ValueError(f"{name} holds a NaN")
    return s


def threshold_for_tpr(id_scores, tpr: float) -> float:
    """The ceil(tpr * n)-th smallest in-distribution score: at least ``tpr`` of those frames pass ``score <= threshold``."""
    s = _scores(id_scores, "id_scores")
    if not 0.0 < tpr <= 1.0:
        raise ValueError(f"tpr must be in (0, 1], got {tpr}")
    rank = min(s.size, max(1, math.ceil(tpr * s.size - 1e-9)))
    return float(np.sort(s)[rank - 1])


def auroc(id_scores, ood_scores) -> float:
    """P(an OOD frame scores above an in-distribution one), ties counting 1/2 (Mann-Whitney)."""
    a, b = np.sort(_scores(id_scores, "id_scores")), _scores(ood_scores, "ood_scores")
    below = np.searchsorted(a, b, side="left")
    equal = np.searchsorted(a, b, side="right") - below
    return float((below.sum() + 0.5 * equal.sum()) / (a.size * b.size))


def fpr_at_tpr(id_scores, ood_scores, tpr: float = 0.95) -> float:
    """The share of OOD frames that pass the threshold which keeps ``tpr`` of the in-distribution frames."""
    thr = threshold_for_tpr(id_scores, tpr)
    return float(np.mean(_scores(ood_scores, "ood_scores") <= thr))


def separation_report(id_scores, ood_scores, threshold: float) -> dict:
    """How well a score separates OOD frames from in-distribution ones: auroc, fpr_at_tpr95, the mean scores and, at
    ``threshold``, the share of each set that is flagged (not score <= threshold)."""
    a, b = np.asarray(id_scores), np.asarray(ood_scores)
    return dict(auroc=auroc(a, b), fpr_at_tpr95=fpr_at_tpr(a, b, 0.95),
                id_mean_dist=float(a.mean()), ood_mean_dist=float(b.mean()), threshold=threshold,
                id_flagged=float(np.mean(~(a <= threshold))), ood_flagged=float(np.mean(~(b <= threshold))),
                n_id=int(a.size), n_ood=int(b.size))


def _check(fn: str, c, D_expected: int):
    """The library's host-only check ``fn`` of the C struct ``c``; raises ValueError with the library's message."""
    err = C.create_string_buffer(256)
    if getattr(_lib.load(), fn)(C.byref(c), int(D_expected), err, len(err)) != _lib.FAV_OK:
        raise ValueError(err.value.decode("utf-8", "replace"))


def _f32_of(records, dwords: int):
    """int32[n, dwords] records (torch tensor or numpy), or ValueError -> the fp32 type their float fields are viewed as."""
    if records.ndim != 2 or int(records.shape[1]) != dwords:
        raise ValueError(f"expected int32[n, {dwords}] records, got shape {tuple(records.shape)}")
    if isinstance(records, np.ndarray):
        return np.float32
    import torch
    return torch.float32



@dataclasses.dataclass(frozen=True)
class OODModel:
    """``mu`` fp32[D] global feature mean, ``P`` fp32[k, D] whitening projection, ``M`` fp32[R, k] projected class means,
    ``class_id`` int32[R] (-1: class-agnostic), ``threshold``: a frame is flagged when not (min_dist <= threshold)."""
    mu: np.ndarray
    P: np.ndarray
    M: np.ndarray
    class_id: np.ndarray
    threshold: float = math.inf

    def __post_init__(self):
        object.__setattr__(self, "mu", np.ascontiguousarray(self.mu, np.float32))
        object.__setattr__(self, "P", np.ascontiguousarray(self.P, np.float32))
        object.__setattr__(self, "M", np.ascontiguousarray(self.M, np.float32))
        object.__setattr__(self, "class_id", np.ascontiguousarray(self.class_id, np.int32))
        object.__setattr__(self, "threshold", float(self.threshold))
        if self.mu.ndim != 1 or self.P.ndim != 2 or self.M.ndim != 2 or self.class_id.ndim != 1:
            raise ValueError("mu and class_id are vectors, P and M matrices")
        if self.P.shape[1] != self.mu.shape[0] or self.M.shape[1] != self.P.shape[0] or self.class_id.shape[0] != self.M.shape[0]:
            raise ValueError(f"shapes do not fit: mu {self.mu.shape}, P {self.P.shape}, M {self.M.shape}, class_id {self.class_id.shape}")

    @property
    def D(self) -> int:
        return int(self.P.shape[1])

    @property
    def k(self) -> int:
        return int(self.P.shape[0])

    @property
    def R(self) -> int:
        return int(self.M.shape[0])

    def with_threshold(self, threshold: float) -> "OODModel":
        return dataclasses.replace(self, threshold=float(threshold))

    def save(self, path):
        np.savez(path, mu=self.mu, P=self.P, M=self.M, class_id=self.class_id, threshold=np.float32(self.threshold))

    @classmethod
    def load(cls, path) -> "OODModel":
        with np.load(path) as z:
            return cls(z["mu"], z["P"], z["M"], z["class_id"], float(z["threshold"]))

    def to_c(self) -> _lib.FavOodModel:
        """The fav_ood_model that points into this model's arrays (which it keeps alive)."""
        m = _lib.FavOodModel()
        m.struct_size = C.sizeof(_lib.FavOodModel)
        m.D, m.k, m.R = self.D, self.k, self.R
        fp = C.POINTER(C.c_float)
        m.mu, m.P, m.M = self.mu.ctypes.data_as(fp), self.P.ctypes.data_as(fp), self.M.ctypes.data_as(fp)
        m.class_id = self.class_id.ctypes.data_as(C.POINTER(C.c_int32))
        m.threshold = self.threshold
        m._keep = self
        return m

    def check(self, D_expected: int = -1):
        """fav_check_ood_model (host only); raises ValueError with the library's message."""
        _check("fav_check_ood_model", self.to_c(), D_expected)

    # the metrics below, under the names they have always had here
    threshold_for_tpr = staticmethod(threshold_for_tpr)
    auroc = staticmethod(auroc)
    fpr_at_tpr = staticmethod(fpr_at_tpr)


def fit_mahalanobis(features, labels, k: int | None = None, shrinkage: float = 0.01) -> OODModel:
    """features [N, D], labels int[N] -> the model, computed in float64: the global mean ``mu``; one mean per class that
    occurs; the tied covariance S = (1/N) sum (f - mu_y)(f - mu_y)^T; S' = (1 - rho) S + rho (tr S / D) I with rho =
    ``shrinkage``; its eigenpairs, eigenvalues descending, the top ``k`` (default D) kept; P = diag(lambda^-1/2) U_k^T and
    M = (mu_c - mu) P^T, cast to fp32.  With k = D the distance is (f - mu_c)^T S'^-1 (f - mu_c)."""
    F = np.asarray(features, np.float64)
    y = np.asarray(labels).ravel()
    if F.ndim != 2 or y.shape[0] != F.shape[0]:
        raise ValueError("features must be [N, D] with one label per row")
    N, D = F.shape
    if N < 2:
        raise ValueError(f"at least 2 feature rows are needed, got {N}")
    if not np.isfinite(F).all():
        raise ValueError("features hold a non-finite value")
    if not np.issubdtype(y.dtype, np.integer):
        raise ValueError("labels must be integers")
    if (y < 0).any():
        raise ValueError("labels must not be negative")
    if not 0.0 <= shrinkage <= 1.0:
        raise ValueError(f"shrinkage must be in [0, 1], got {shrinkage}")
    k = D if k is None else int(k)
    if not 1 <= k <= D:
        raise ValueError(f"k must be in [1, D={D}], got {k}")
    mu = F.mean(axis=0)
    classes, inv = np.unique(y, return_inverse=True)
    means = np.stack([F[inv == c].mean(axis=0) for c in range(classes.size)])
    Z = F - means[inv]
    S = Z.T @ Z / N
    S = (1.0 - shrinkage) * S + shrinkage * (np.trace(S) / D) * np.eye(D)
    lam, U = np.linalg.eigh(S)
    order = np.argsort(lam)[::-1][:k]
    lam, U = lam[order], U[:, order]
    if not (lam > 0).all():
        raise ValueError("the shrunk covariance is singular in the kept directions; raise shrinkage or lower k")
    P = (U / np.sqrt(lam)).T
    M = (means - mu) @ P.T
    return OODModel(mu.astype(np.float32), P.astype(np.float32), M.astype(np.float32), classes.astype(np.int32))


def unpack_records(records) -> dict:
    """int32[n, 4] fav_ood_record records (torch tensor or numpy) -> ``min_dist`` fp32[n], ``nearest_class`` int32[n],
    ``label_dist`` fp32[n], ``ood`` int32[n]; views of the record buffer."""
    f32 = _f32_of(records, OOD_RECORD_DWORDS)
    return {"min_dist": records[:, 0].view(f32), "nearest_class": records[:, 1], "label_dist": records[:, 2].view(f32),
            "ood": records[:, 3]}


# ---- nearest-neighbour scoring (include/fav.h fav_knn_bank) ------------------------------------
def _bf16_bits(x: np.ndarray) -> np.ndarray:
    """finite float32 -> bf16 bit patterns, round to nearest even (the integer recipe of the device and the oracle)."""
    u = np.ascontiguousarray(x, np.float32).view(np.uint32)
    return ((u + 0x7FFF + ((u >> 16) & 1)) >> 16).astype(np.uint16)


@dataclasses.dataclass(frozen=True)
class KNNBank:
    """``rows`` uint16[N, D]: L2-normalised in-distribution features as bf16 bit patterns, ``class_id`` int32[N] or None, ``k``:
    which neighbour's distance is the score, ``threshold``: a frame is flagged when not (kth_dist <= threshold), ``selection``:
    the ``coreset.CoresetSelection`` that chose the rows (``select="coreset"``), else None; it is not saved."""
    rows: np.ndarray
    class_id: np.ndarray | None = None
    k: int = 10
    threshold: float = math.inf
    selection: object | None = None

    def __post_init__(self):
        if np.asarray(self.rows).dtype != np.uint16:
            raise ValueError("rows are bf16 bit patterns: uint16 (build_knn_bank makes them from features)")
        object.__setattr__(self, "rows", np.ascontiguousarray(self.rows, np.uint16))
        if self.class_id is not None:
            object.__setattr__(self, "class_id", np.ascontiguousarray(self.class_id, np.int32))
        object.__setattr__(self, "k", int(self.k))
        object.__setattr__(self, "threshold", float(self.threshold))
        if self.rows.ndim != 2:
            raise ValueError("rows is a matrix [N, D]")
        if self.class_id is not None and self.class_id.shape != (self.rows.shape[0],):
            raise ValueError(f"shapes do not fit: rows {self.rows.shape}, class_id {self.class_id.shape}")

    @property
    def N(self) -> int:
        return int(self.rows.shape[0])

    @property
    def D(self) -> int:
        return int(self.rows.shape[1])

    def with_threshold(self, threshold: float) -> "KNNBank":
        return dataclasses.replace(self, threshold=float(threshold))

    def take(self, indices) -> "KNNBank":
        """The bank of the rows ``indices`` (in that order) and their ``class_id``; ``k`` and ``threshold`` are kept, ``k`` is
        checked against the new N."""
        idx = _take_indices(indices, self.N)
        if not 1 <= self.k <= idx.shape[0]:
            raise ValueError(f"k must be in [1, N={idx.shape[0]}], got {self.k}")
        return KNNBank(self.rows[idx], None if self.class_id is None else self.class_id[idx], self.k, self.threshold)

    def save(self, path):
        extra = {} if self.class_id is None else {"class_id": self.class_id}
        np.savez(path, rows=self.rows, k=np.int32(self.k), threshold=np.float32(self.threshold), **extra)

    @classmethod
    def load(cls, path) -> "KNNBank":
        with np.load(path) as z:
            return cls(z["rows"], z["class_id"] if "class_id" in z.files else None, int(z["k"]), float(z["threshold"]))

    def to_c(self) -> _lib.FavKnnBank:
        """The fav_knn_bank that points into this bank's arrays (which it keeps alive)."""
        b = _lib.FavKnnBank()
        b.struct_size = C.sizeof(_lib.FavKnnBank)
        b.D, b.N, b.k = self.D, self.N, self.k
        b.rows = self.rows.ctypes.data_as(C.POINTER(C.c_uint16))
        if self.class_id is not None:
            b.class_id = self.class_id.ctypes.data_as(C.POINTER(C.c_int32))
        b.threshold = self.threshold
        b._keep = self
        return b

    def check(self, D_expected: int = -1):
        """fav_check_knn_bank (host only); raises ValueError with the library's message."""
        _check("fav_check_knn_bank", self.to_c(), D_expected)


def build_knn_bank(features, labels=None, k: int = 10, max_rows: int | None = None, seed: int = 0, select: str = "random",
                   device=None) -> KNNBank:
    """features [N, D] (one row per in-distribution frame: the mean over the samples of its features), labels int[N] or None
    -> the bank: every row divided by its Euclidean norm in float64, then rounded to bf16 (nearest even).  ``max_rows``: keep
    that many rows, in their original order.  ``select="random"``: drawn without replacement by
    ``np.random.default_rng(seed)``.  ``select="coreset"``: every row is normalised and rounded first, then
    ``coreset.select_coreset(rows, max_rows, seed)`` picks them on ``device`` - greedy k-centre selection, which covers the
    feature space where a draw samples its density - and ``bank.selection`` keeps the picks and the coverage curve; with
    ``max_rows`` None or at least N it keeps everything, as the draw does, and touches no device.  Refuses a non-finite value
    and a zero row."""
    from .coreset import check_select, select_coreset
    check_select(select)
    F = np.asarray(features, np.float64)
    if F.ndim != 2 or F.shape[0] < 1:
        raise ValueError("features must be [N, D] with at least one row")
    if not np.isfinite(F).all():
        raise ValueError("features hold a non-finite value")
    y = None
    if labels is not None:
        y = np.asarray(labels).ravel()
        if y.shape[0] != F.shape[0]:
            raise ValueError("one label per feature row")
        if not np.issubdtype(y.dtype, np.integer):
            raise ValueError("labels must be integers")
        if (y < 0).any():
            raise ValueError("labels must not be negative")
    if select == "coreset" and _subsample_count(F.shape[0], max_rows) is not None:
        full = KNNBank(_unit_rows_bf16(F), None if y is None else y.astype(np.int32), k=k)
        selection = select_coreset(full.rows, int(max_rows), seed, device=device)
        return dataclasses.replace(full.take(selection.indices), selection=selection)
    F, keep = _subsample(F, max_rows, seed)
    if keep is not None and y is not None:
        y = y[keep]
    rows = _unit_rows_bf16(F)
    if not 1 <= k <= F.shape[0]:
        raise ValueError(f"k must be in [1, N={F.shape[0]}], got {k}")
    return KNNBank(rows, None if y is None else y.astype(np.int32), k=k)


def _subsample_count(N: int, max_rows):
    """-> how many of N rows ``max_rows`` keeps, or None when it keeps them all; refuses a count below 1."""
    if max_rows is None:
        return None
    if max_rows < 1:
        raise ValueError(f"max_rows must be at least 1, got {max_rows}")
    return None if max_rows >= N else int(max_rows)


def _subsample(F: np.ndarray, max_rows, seed: int):
    """-> (the rows kept, their indices or None when all are): ``max_rows`` of them, drawn without replacement by
    ``np.random.default_rng(seed)`` and kept in their original order."""
    count = _subsample_count(F.shape[0], max_rows)
    if count is None:
        return F, None
    keep = np.sort(np.random.default_rng(seed).choice(F.shape[0], size=count, replace=False))
    return F[keep], keep


def _take_indices(indices, N: int) -> np.ndarray:
    """``indices`` of a bank's ``take`` -> int64 [m], m >= 1, every one a row of the bank."""
    idx = np.asarray(indices)
    if idx.ndim != 1 or idx.shape[0] < 1 or not np.issubdtype(idx.dtype, np.integer):
        raise ValueError("indices is a non-empty vector of integers")
    idx = idx.astype(np.int64)
    if (idx < 0).any() or (idx >= N).any():
        raise ValueError(f"indices must be in [0, N={N})")
    return idx


def _unit_rows_bf16(F: np.ndarray) -> np.ndarray:
    """float64 [N, D] -> every row divided by its Euclidean norm in float64, then rounded to bf16 bits (nearest even): what a
    bank and a drift reference hold.  Refuses a zero row."""
    norm = np.sqrt((F * F).sum(axis=1))
    if not (norm > 0).all():
        raise ValueError(f"feature row {int(np.flatnonzero(~(norm > 0))[0])} is zero: it has no direction")
    return _bf16_bits((F / norm[:, None]).astype(np.float32))


def unpack_knn_records(records) -> dict:
    """int32[n, 6] fav_knn_record records (torch tensor or numpy) -> ``kth_dist``, ``kth_sim``, ``nn_sim`` fp32[n], ``nn_row``,
    ``nn_class``, ``ood`` int32[n]; views of the record buffer."""
    f32 = _f32_of(records, KNN_RECORD_DWORDS)
    return {"kth_dist": records[:, 0].view(f32), "kth_sim": records[:, 1].view(f32), "nn_sim": records[:, 2].view(f32),
            "nn_row": records[:, 3], "nn_class": records[:, 4], "ood": records[:, 5]}


# ---- window-level drift detection (include/fav.h fav_drift_ref) ---------------------------------
#: dwords of the one fav_drift_record of a call
DRIFT_RECORD_DWORDS = 12


@dataclasses.dataclass(frozen=True)
class DriftReference:
    """``rows`` uint16[R, D]: L2-normalised held-out in-distribution features as bf16 bit patterns, ``n_perm``: permutations of
    the test, ``alpha``: a window is flagged when p_value <= alpha, ``seed``: the Philox key of the permutations."""
    rows: np.ndarray
    n_perm: int = 999
    alpha: float = 0.01
    seed: int = 0

    def __post_init__(self):
        if np.asarray(self.rows).dtype != np.uint16:
            raise ValueError("rows are bf16 bit patterns: uint16 (build_drift_reference makes them from features)")
        object.__setattr__(self, "rows", np.ascontiguousarray(self.rows, np.uint16))
        object.__setattr__(self, "n_perm", int(self.n_perm))
        object.__setattr__(self, "alpha", float(self.alpha))
        object.__setattr__(self, "seed", int(self.seed))
        if self.rows.ndim != 2:
            raise ValueError("rows is a matrix [R, D]")
        if not 0 <= self.seed < 1 << 64:
            raise ValueError("seed is a 64-bit unsigned integer")

    @property
    def R(self) -> int:
        return int(self.rows.shape[0])

    @property
    def D(self) -> int:
        return int(self.rows.shape[1])

    def with_alpha(self, alpha: float) -> "DriftReference":
        return dataclasses.replace(self, alpha=float(alpha))

    def save(self, path):
        np.savez(path, rows=self.rows, n_perm=np.int32(self.n_perm), alpha=np.float32(self.alpha), seed=np.uint64(self.seed))

    @classmethod
    def load(cls, path) -> "DriftReference":
        with np.load(path) as z:
            return cls(z["rows"], int(z["n_perm"]), float(z["alpha"]), int(z["seed"]))

    def to_c(self) -> _lib.FavDriftRef:
        """The fav_drift_ref that points into this reference's rows (which it keeps alive)."""
        b = _lib.FavDriftRef()
        b.struct_size = C.sizeof(_lib.FavDriftRef)
        b.D, b.R, b.n_perm = self.D, self.R, self.n_perm
        b.rows = self.rows.ctypes.data_as(C.POINTER(C.c_uint16))
        b.seed = self.seed
        b.alpha = self.alpha
        b._keep = self
        return b

    def check(self, D_expected: int = -1):
        """fav_check_drift_ref (host only); raises ValueError with the library's message."""
        _check("fav_check_drift_ref", self.to_c(), D_expected)


def build_drift_reference(features, max_rows: int | None = 1024, n_perm: int = 999, alpha: float = 0.01, seed: int = 0) -> DriftReference:
    """features [N, D] (one row per held-out in-distribution frame: the mean over the samples of its features) -> the
    reference: rows normalised and rounded exactly as ``build_knn_bank``'s, at most ``max_rows`` of them, drawn as there.
    ``seed`` draws the rows and keys the permutations.  Refuses a non-finite value and a zero row."""
    F = np.asarray(features, np.float64)
    if F.ndim != 2 or F.shape[0] < 2:
        raise ValueError("features must be [N, D] with at least two rows")
    if not np.isfinite(F).all():
        raise ValueError("features hold a non-finite value")
    F, _ = _subsample(F, max_rows, seed)
    return DriftReference(_unit_rows_bf16(F), n_perm=n_perm, alpha=alpha, seed=seed)


def unpack_drift_record(record) -> dict:
    """int32[12] (or [1, 12]) fav_drift_record (torch tensor or numpy) -> ``statistic`` (float), ``s_ab``, ``s_aa``, ``s_bb``,
    ``n_exceed``, ``n_degenerate`` (int), ``p_value`` (float), ``drift`` (bool).  Reads the record on the host: a device
    tensor is copied, which waits for the call that wrote it."""
    if not isinstance(record, np.ndarray):
        record = record.cpu().numpy()
    rec = np.ascontiguousarray(record, np.int32).ravel()
    if rec.shape[0] != DRIFT_RECORD_DWORDS:
        raise ValueError(f"expected the int32[{DRIFT_RECORD_DWORDS}] of one fav_drift_record, got shape {tuple(record.shape)}")
    q = rec[:8].view(np.int64)
    return {"statistic": float(rec[:2].view(np.float64)[0]), "s_ab": int(q[1]), "s_aa": int(q[2]), "s_bb": int(q[3]),
            "p_value": float(rec[8:9].view(np.float32)[0]), "n_exceed": int(rec[9]), "drift": bool(rec[10]),
            "n_degenerate": int(rec[11])}
