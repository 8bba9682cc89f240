"""Batch sharding across the GPUs of one node.

Every frame is independent (BatchNorm is folded, dropout masks are keyed by the
GLOBAL frame index), so rank r classifies frames [start_r, stop_r) of the batch
with fully replicated weights and the only exchange is one small all-gather of
packed 8-byte (int32 label, fp32 confidence) records — 2 KiB for 256 frames,
latency-bound on xGMI, so a single ``all_gather_into_tensor`` (RCCL when the
backend is "nccl") and no ring/bucket machinery.  The reference is a single
process (SURVEY.md §5 "Distributed communication backend: None").
"""
from __future__ import annotations

import numpy as np


def shard_range(n_total: int, rank: int, world: int):
    """Contiguous shard [start, stop) of rank; the first n_total % world ranks get one extra frame."""
    q, r = divmod(int(n_total), int(world))
    start = rank * q + min(rank, r)
    return start, start + q + (1 if rank < r else 0)


def pack_records(labels, conf):
    """(int32[n], fp32[n]) torch tensors -> int32[n, 2] records (confidence bit-cast)."""
    import torch
    return torch.stack([labels.to(torch.int32), conf.to(torch.float32).view(torch.int32)], dim=1).contiguous()


def unpack_records(rec):
    import torch
    return rec[:, 0].contiguous(), rec[:, 1].contiguous().view(torch.float32)


def classify_sharded(classifier, local_frames, n_total: int, rank: int, world: int, group=None, detail: bool = False,
                     sets=None):
    """Each rank classifies its own shard (global frame indices [start, stop)) and all ranks receive the full
    (labels[n_total], conf[n_total]).

    ``classifier`` is a ``Backend`` on a GPU rank: its confidence head writes the packed 8-byte records straight into
    this rank's slot of the all-gather send buffer (``Backend.classify_records``), one ``all_gather_into_tensor``
    (RCCL) moves them, and the results are views of the receive buffer - no pack, pad or concatenate launches.
    A plain function ``classify_fn(frames, first_index=...) -> (labels, conf)`` is accepted too (CPU tensors / gloo:
    the tests that stand the oracle in for the per-rank classifier), and a ``Backend`` handed HOST frames (a NumPy
    array, or a tensor that is not on its GPU) goes through its ordinary ``classify`` (which uploads them).

    Lifetime of the results: on the direct path with equal shards (and with ``world == 1``) the two tensors are stride-2
    VIEWS of one freshly allocated [n, 2] int32 record buffer - no copy is made; call ``.contiguous()`` before handing a raw
    ``data_ptr()`` to something that assumes dense arrays.  Every call allocates its own buffers, so results stay valid
    across later calls.

    ``detail=True``: the same exchange with the 72-byte uncertainty records (include/fav.h fav_uncertainty) in place of the
    8-byte ones - ``Backend.classify_uncertainty`` writes them into this rank's slot of the send buffer - and the result is
    ``unpack_uncertainty`` of the gathered int32[n_total, 18] records (a dict of per-field views).  A plain function
    ``fn(frames, first_index=...) -> int32[n, 18]`` records is accepted there too.

    ``sets=cp`` (a ``conformal.Conformal``): the same exchange with the 160-byte prediction-set records (include/fav.h
    fav_pred_set) - ``Backend.classify_sets`` writes them into this rank's slot - and the result is ``unpack_sets`` of the
    gathered int32[n_total, 40] records.  A plain function ``fn(frames, first_index=...) -> int32[n, 40]`` records is
    accepted there too.  The randomized draw is keyed by the global frame index, so the gathered sets are those of one
    rank classifying every frame."""
    if sets is not None:
        from .conformal import PRED_SET_DWORDS, unpack_sets
        num_classes = int(classifier.cfg.num_classes) if hasattr(classifier, "classify_sets") else 1024
        method = None
        if hasattr(classifier, "classify_sets"):
            method = lambda frames, first_index=0, out=None: classifier.classify_sets(frames, sets, first_index=first_index,  # noqa: E731
                                                                                    out=out)
        return _gather_records(classifier, method, local_frames, n_total, rank, world, group, PRED_SET_DWORDS,
                               lambda rec: unpack_sets(rec, num_classes))
    if detail:
        return _classify_sharded_detail(classifier, local_frames, n_total, rank, world, group)
    import torch
    import torch.distributed as dist
    start, stop = shard_range(n_total, rank, world)
    n_local = stop - start
    if n_local > 0 and int(local_frames.shape[0]) != n_local:
        raise ValueError(f"rank {rank} owns frames [{start},{stop}) but was handed {int(local_frames.shape[0])}")
    cap = -(-n_total // world)  # every shard padded to the largest
    direct = hasattr(classifier, "classify_records") and hasattr(local_frames, "is_cuda") and bool(local_frames.is_cuda) and \
        local_frames.device.index == getattr(classifier, "device", local_frames.device.index)
    if not direct and hasattr(classifier, "classify_records"):
        backend = classifier
        classifier = lambda frames, first_index=0: backend.classify(frames, first_index=first_index)   # noqa: E731  (host frames: upload + classify)
    if direct:
        dev = local_frames.device
        send = torch.empty((cap, 2), dtype=torch.int32, device=dev) if n_local == cap else \
            torch.zeros((cap, 2), dtype=torch.int32, device=dev)
        if n_local > 0:
            classifier.classify_records(local_frames, first_index=start, out=send[:n_local])
    else:
        if n_local > 0:
            labels, conf = classifier(local_frames, first_index=start)
            if isinstance(labels, np.ndarray):
                labels, conf = torch.from_numpy(labels), torch.from_numpy(conf)
            rec = pack_records(labels, conf)
            dev = rec.device
        else:
            dev = local_frames.device if hasattr(local_frames, "device") and not isinstance(local_frames, np.ndarray) else "cpu"
            rec = torch.zeros((0, 2), dtype=torch.int32, device=dev)
        send = torch.zeros((cap, 2), dtype=torch.int32, device=dev)
        send[:n_local] = rec
    if world == 1:
        return unpack_records(send[:n_local]) if not direct else (send[:n_local, 0], send[:n_local, 1].view(torch.float32))
    recv = torch.empty((world * cap, 2), dtype=torch.int32, device=dev)
    if dist.get_backend(group) == "gloo" and send.is_cuda:
        # rehearsal only (several ranks sharing one GPU, where RCCL cannot run): the 8-byte records cross the host
        host = torch.empty((world * cap, 2), dtype=torch.int32)
        dist.all_gather_into_tensor(host, send.cpu(), group=group)
        recv.copy_(host)
    else:
        dist.all_gather_into_tensor(recv, send, group=group)
    if n_total == world * cap:                 # equal shards: the receive buffer IS the result
        return recv[:, 0], recv[:, 1].view(torch.float32)
    parts = []
    for r in range(world):
        s, e = shard_range(n_total, r, world)
        parts.append(recv[r * cap:r * cap + (e - s)])
    return unpack_records(torch.cat(parts, dim=0))


def _classify_sharded_detail(classifier, local_frames, n_total: int, rank: int, world: int, group=None):
    """classify_sharded(..., detail=True): one all-gather of int32[cap, 18] uncertainty records per rank."""
    from .backend import UNCERTAINTY_DWORDS, unpack_uncertainty
    method = classifier.classify_uncertainty if hasattr(classifier, "classify_uncertainty") else None
    return _gather_records(classifier, method, local_frames, n_total, rank, world, group, UNCERTAINTY_DWORDS,
                           unpack_uncertainty)


def _gather_records(classifier, method, local_frames, n_total: int, rank: int, world: int, group, W: int, unpack):
    """One all-gather of int32[cap, W] records per rank.  ``method(frames, first_index=, out=)``: the Backend method that
    writes the records into this rank's slot of the send buffer (None: ``classifier`` is a plain function returning
    int32[n, W] records); ``unpack``: records -> the result dict."""
    import torch
    import torch.distributed as dist
    start, stop = shard_range(n_total, rank, world)
    n_local = stop - start
    if n_local > 0 and int(local_frames.shape[0]) != n_local:
        raise ValueError(f"rank {rank} owns frames [{start},{stop}) but was handed {int(local_frames.shape[0])}")
    cap = -(-n_total // world)  # every shard padded to the largest
    if method is not None:
        # a Backend: host frames (or frames on another device) are uploaded to its GPU first
        dev = torch.device(f"cuda:{classifier.device}")
        if isinstance(local_frames, np.ndarray):
            local_frames = torch.from_numpy(np.ascontiguousarray(local_frames))
        local_frames = local_frames.to(dev)
        send = torch.empty((cap, W), dtype=torch.int32, device=dev) if n_local == cap else \
            torch.zeros((cap, W), dtype=torch.int32, device=dev)
        if n_local > 0:
            method(local_frames, first_index=start, out=send[:n_local])
    else:
        if n_local > 0:
            rec = classifier(local_frames, first_index=start)
            rec = torch.from_numpy(np.ascontiguousarray(rec)) if isinstance(rec, np.ndarray) else rec
            if rec.dtype != torch.int32 or tuple(rec.shape) != (n_local, W):
                raise ValueError(f"the classifier must return int32[{n_local}, {W}] records, got {rec.dtype} {tuple(rec.shape)}")
            dev = rec.device
        else:
            dev = local_frames.device if hasattr(local_frames, "device") and not isinstance(local_frames, np.ndarray) else "cpu"
            rec = torch.zeros((0, W), dtype=torch.int32, device=dev)
        send = torch.zeros((cap, W), dtype=torch.int32, device=dev)
        send[:n_local] = rec
    if world == 1:
        return unpack(send[:n_local])
    recv = torch.empty((world * cap, W), dtype=torch.int32, device=dev)
    if dist.get_backend(group) == "gloo" and send.is_cuda:
        # rehearsal only (several ranks sharing one GPU, where RCCL cannot run): the records cross the host
        host = torch.empty((world * cap, W), dtype=torch.int32)
        dist.all_gather_into_tensor(host, send.cpu(), group=group)
        recv.copy_(host)
    else:
        dist.all_gather_into_tensor(recv, send, group=group)
    if n_total == world * cap:                 # equal shards: the receive buffer IS the result
        return unpack(recv)
    parts = []
    for r in range(world):
        s, e = shard_range(n_total, r, world)
        parts.append(recv[r * cap:r * cap + (e - s)])
    return unpack(torch.cat(parts, dim=0))
