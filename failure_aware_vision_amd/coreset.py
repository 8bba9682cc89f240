"""Greedy coreset selection on the device (include/fav.h fav_check_coreset, fav_op_coreset_select; DESIGN.md section 2, item
5n; the k-centre selection of PatchCore, Roth et al. 2022): WHICH rows a ``patch.PatchBank`` or an ``ood.KNNBank`` keeps.

A seeded uniform draw (``ood._subsample``) keeps rows in proportion to how often they occur: the dominant texture gets nearly
all of a bank and the rare in-distribution modes none, and those are then the cells and frames reported as anomalous.
Farthest-point sampling covers the feature space instead: every pick is the row farthest from the rows picked so far.  That
is M serial steps, each a pass over the whole pool, so it runs on the device; there is no CPU fallback.

``select_coreset`` is the whole interface; ``select="coreset"`` of ``ood.build_knn_bank``, ``patch.bank_from_rows``,
``patch.build_patch_bank``, ``Backend.fit_knn`` and ``Backend.fit_patch_bank`` goes through it.  Out of scope: PatchCore's
random projection before the selection, pools that do not fit device memory, selection over several GPUs."""
from __future__ import annotations

import dataclasses

import numpy as np

from . import _lib

#: what ``select=`` of the bank builders takes
SELECT_MODES = ("random", "coreset")


@dataclasses.dataclass(frozen=True)
class CoresetSelection:
    """``order`` int32[m]: the rows in the order picked, ``order[0]`` = ``start_row``; ``radius`` float32[m + 1]: ``radius[0]``
    +inf, ``radius[t]`` the distance of pick t from the picks before it (never increasing), ``radius[m]`` the covering radius
    of the whole selection.  The first m' entries are the selection of m' rows: ``radius`` is the coverage curve from which
    ``max_rows`` is chosen."""
    order: np.ndarray
    radius: np.ndarray
    start_row: int

    def __post_init__(self):
        object.__setattr__(self, "order", np.ascontiguousarray(self.order, np.int32))
        object.__setattr__(self, "radius", np.ascontiguousarray(self.radius, np.float32))
        object.__setattr__(self, "start_row", int(self.start_row))
        if self.order.ndim != 1 or self.radius.shape != (self.order.shape[0] + 1,):
            raise ValueError(f"shapes do not fit: order {self.order.shape}, radius {self.radius.shape}")

    @property
    def indices(self) -> np.ndarray:
        """``order`` sorted ascending: the rows kept in their original order, as a random subsample keeps them."""
        return np.sort(self.order)

    @property
    def cover_radius(self) -> float:
        """No row of the pool is farther than this (squared distance) from its nearest selected row."""
        return float(self.radius[-1])


def check_select(select: str) -> str:
    if select not in SELECT_MODES:
        raise ValueError(f"select must be one of {SELECT_MODES}, got {select!r}")
    return select


def _check_dims(N: int, D: int, m: int, start_row: int):
    """fav_check_coreset (host only); raises ValueError with the library's message."""
    import ctypes as C
    err = C.create_string_buffer(256)
    if _lib.load().fav_check_coreset(N, D, m, start_row, err, len(err)) != _lib.FAV_OK:
        raise ValueError(err.value.decode("utf-8", "replace"))


def select_coreset(rows, m: int, seed: int = 0, start_row: int | None = None, device=None) -> CoresetSelection:
    """rows uint16 [N, D] (numpy) or a CUDA int16 / uint16 tensor [N, D]: bf16 bit patterns of unit rows -> the greedy
    k-centre selection of ``m`` of them (fav_op_coreset_select), bit for bit what include/fav.h defines.  ``start_row``: the
    first pick, by default ``np.random.default_rng(seed).integers(N)``.  ``device``: where a numpy pool is uploaded (the
    current device by default); a tensor is used where it lives.  Refuses, before anything touches a device, a non-finite
    value, an all-zero row and ``m`` outside [1, N].  Synchronous: the result is read back."""
    is_tensor = hasattr(rows, "is_cuda")
    if is_tensor:
        import torch
        if not rows.is_cuda or rows.dtype not in (torch.int16, torch.uint16) or rows.ndim != 2:
            raise ValueError("a tensor pool is a CUDA int16 or uint16 tensor [N, D] of bf16 bit patterns")
        bits = rows.contiguous().view(torch.int16)
        N, D = int(bits.shape[0]), int(bits.shape[1])
    else:
        bits = np.asarray(rows)
        if bits.dtype != np.uint16 or bits.ndim != 2:
            raise ValueError("rows are bf16 bit patterns: uint16 [N, D]")
        bits = np.ascontiguousarray(bits)
        N, D = bits.shape
    if N < 1:
        raise ValueError("rows must hold at least one row")
    m = int(m)
    if not 1 <= m <= N:
        raise ValueError(f"m must be in [1, N={N}], got {m}")
    if is_tensor:
        nonfinite = ((bits & 0x7F80) == 0x7F80).any(dim=1)
        zero = ((bits & 0x7FFF) == 0).all(dim=1)
        bad = [int(torch.nonzero(v)[0]) if bool(v.any()) else None for v in (nonfinite, zero)]
    else:
        nonfinite = ((bits & 0x7F80) == 0x7F80).any(axis=1)
        zero = ((bits & 0x7FFF) == 0).all(axis=1)
        bad = [int(np.flatnonzero(v)[0]) if v.any() else None for v in (nonfinite, zero)]
    if bad[0] is not None:
        raise ValueError(f"rows holds a non-finite value (row {bad[0]})")
    if bad[1] is not None:
        raise ValueError(f"row {bad[1]} is zero: it has no direction")
    start = int(np.random.default_rng(seed).integers(N)) if start_row is None else int(start_row)
    _check_dims(N, D, m, start)

    import torch
    if not torch.cuda.is_available():
        raise RuntimeError("select_coreset runs on a gfx950 GPU and none is available; there is no CPU fallback")
    lib = _lib.load()
    if not is_tensor:
        dev = torch.device("cuda", torch.cuda.current_device() if device is None else
                           (device if isinstance(device, int) else torch.device(device).index or 0))
        bits = torch.from_numpy(bits.view(np.int16)).to(dev)
    with torch.cuda.device(bits.device):
        need = lib.fav_coreset_workspace_bytes(N, D, m)
        ws = torch.empty(need, dtype=torch.uint8, device=bits.device)
        order = torch.empty(m, dtype=torch.int32, device=bits.device)
        radius = torch.empty(m + 1, dtype=torch.float32, device=bits.device)
        _lib.check(lib.fav_op_coreset_select(bits.data_ptr(), N, D, m, start, ws.data_ptr(), need, order.data_ptr(),
                                             radius.data_ptr(), torch.cuda.current_stream(bits.device).cuda_stream))
        return CoresetSelection(order.cpu().numpy(), radius.cpu().numpy(), start)
