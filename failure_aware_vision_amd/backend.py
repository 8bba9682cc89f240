"""Host side of the drop-in: ``Backend.classify(images) -> (labels, confidences)``.

Mirrors the reference's scorer interface so it plugs into the same seam:

* construction per connection / ``reset()`` / drop on disconnect —
  platform/backend/main.py:110-118, :284-291, :310-317;
* ``analyze_frame(frame) -> {'anomaly_score', 'vision_status', 'metrics'}`` —
  the shape of SignalAnalyzer.analyze_frame, platform/backend/signal_analyzer.py:47-143,
  whose result is fed to ``TrustEngine.update(vision_status, anomaly_score, dt)``
  (main.py:160-168);
* errors at the seam: a malformed frame raises (a caller bug); a failure of the GPU
  path is reported as a NON-OK ``vision_status`` with a numeric ``anomaly_score``
  (main.py:169 rounds the score, and an unseen frame must not count as healthy:
  trust_engine.py:179-190); ``classify`` itself raises.

All arithmetic happens in the HIP library behind include/fav.h.  torch is used
only for device buffers and the current stream.
"""
from __future__ import annotations

import ctypes as C
import dataclasses

import numpy as np

from . import _lib, views as _views, weights as _weights
from .corrupt import CORRUPTIONS

_ARCH = {"resnet18_cifar": _lib.ARCH_RESNET18_CIFAR, "resnet50": _lib.ARCH_RESNET50, "vit_b16": _lib.ARCH_VIT_B16,
         "vit_tiny": _lib.ARCH_VIT_TINY}
_CONF = {"max_softmax": _lib.CONF_MAX_SOFTMAX, "entropy": _lib.CONF_ENTROPY, "mutual_info": _lib.CONF_MUTUAL_INFO}
#: dwords of one fav_uncertainty record (include/fav.h)
UNCERTAINTY_DWORDS = 18
_MATH = {"bf16": _lib.MATH_BF16, "f32_exact": _lib.MATH_F32_EXACT}


def _to_numpy(x) -> np.ndarray:
    """A numpy array as it is, a torch tensor copied to the host (which synchronises its stream)."""
    return x if isinstance(x, np.ndarray) else x.cpu().numpy()


class Backend:
    def __init__(self, arch: str = "resnet50", blob: bytes | None = None, *, seed_weights: int = 1, device: int | None = None,
                 in_hw=None, max_batch: int = 256, num_classes: int | None = None,
                 n_samples: int = 1, dropout_policy: str = "none", dropout_p: float = 0.0, seed: int = 0,
                 site_mask: int | None = None, temperature: float = 1.0, conf_kind: str = "max_softmax",
                 tau: float = 0.5, math_mode: str = "bf16", mean=None, std=None,
                 chunk_a: int = 0, chunk_b: int = 0, regroup_block: int = -1,
                 tail_min_rows: int = 0, ens_grouped_max: int = 0, vit_streams: int = 0, stem_fused: int = 0, views=None):
        import torch
        self._torch = torch
        self._h = None
        self._rules = None
        self.lib = _lib.load()
        if not torch.cuda.is_available():
            raise RuntimeError("failure_aware_vision_amd.Backend needs a gfx950 GPU (torch.cuda.is_available() is "
                               "False); the path has no CPU fallback")
        self.device = torch.cuda.current_device() if device is None else int(device)
        self.arch = arch
        cfg = _lib.FavConfig()
        self.lib.fav_default_config(C.byref(cfg), _ARCH[arch])
        cfg.device = self.device
        if in_hw is not None:
            cfg.in_h, cfg.in_w = int(in_hw[0]), int(in_hw[1])
        if num_classes is not None:
            cfg.num_classes = int(num_classes)
        cfg.max_batch = int(max_batch)
        if mean is not None:
            cfg.mean[:] = [float(m) for m in mean]
        if std is not None:
            cfg.stdev[:] = [float(s) for s in std]
        cfg.n_samples = int(n_samples)
        cfg.site_mask = int(site_mask) if site_mask is not None else _weights.site_mask_for(_ARCH[arch], dropout_policy)
        cfg.dropout_p = float(dropout_p)
        cfg.seed = int(seed)
        cfg.temperature = float(temperature)
        cfg.conf_kind = _CONF[conf_kind]
        cfg.tau = float(tau)
        cfg.math_mode = _MATH[math_mode]
        cfg.chunk_a, cfg.chunk_b, cfg.regroup_block = int(chunk_a), int(chunk_b), int(regroup_block)
        # schedule choices (fav_config, ABI 2): 0 = the build's measured default; results never depend on them, nor on the
        # chunks and the regroup point above (tests/test_gpu_schedule_sweep.py sweeps them all on the device, bit for bit)
        cfg.tail_min_rows, cfg.ens_grouped_max = int(tail_min_rows), int(ens_grouped_max)
        cfg.vit_streams, cfg.stem_fused = int(vit_streams), int(stem_fused)
        members = list(blob) if isinstance(blob, (list, tuple)) else None   # deep ensemble: one blob per member
        cfg.n_members = len(members) if members else 1
        self.mc = cfg.site_mask != 0 and round(cfg.dropout_p * 256) > 0
        views = list(views) if views else []
        # mutual information over views alone: fav_create refuses the kind on a single-sample handle, so the handle is created
        # with another kind and gets this one once the views are set
        kind_after_views = None
        if cfg.conf_kind == _lib.CONF_MUTUAL_INFO and len(views) >= 2 and cfg.n_members == 1 and not self.mc:
            kind_after_views, cfg.conf_kind = conf_kind, _lib.CONF_MAX_SOFTMAX
        self.cfg = cfg
        h = C.c_void_p()
        _lib.check(self.lib.fav_create(C.byref(cfg), C.byref(h)))
        self._h = h
        if members:
            for i, b in enumerate(members):
                self.load_weights(b, member=i)
        else:
            if blob is None and _ARCH[arch] in _weights.VIT_CFG:
                blob, self.weights_info = _weights.make_synthetic_vit(arch, seed=seed_weights, num_classes=cfg.num_classes,
                                                                     in_hw=(cfg.in_h, cfg.in_w))
            elif blob is None:
                blob, self.weights_info = _weights.make_synthetic(arch, seed=seed_weights, num_classes=cfg.num_classes)
            self.load_weights(blob)
        self._T_head = cfg.n_samples if self.mc else max(1, cfg.n_members)
        self._tap, self._ood, self._knn = False, None, None   # the caller's own feature tap; the ood.OODModel, the ood.KNNBank in force
        self._drift = None                                    # the ood.DriftReference in force
        self._patch = None                                    # the patch.PatchBank in force
        self._map_hw = None                                   # (Hf, Wf) of the map tap, known from the first set_map_tap(True) on
        self._attn_grid = None                                # (gh, gw) of the attention tap, known from the first set_attn_tap(True) on
        self._map_tap_on = self._attn_tap_on = False          # the two localisation taps as this object last set them
        self._stage_tap = 0                                   # the stage tap as this object last set it (0: off)
        self._curve_steps = None                              # the steps of the curve descriptor in force (set_curve)
        self._views = ()
        if views:
            self.set_views(views)
        if kind_after_views is not None:
            self.set_conf_kind(kind_after_views)
        self._rules = None   # SignalAnalyzerHIP, created on the first analyze_frame

    # -- test-time augmentation (views.py; include/fav.h fav_set_views) ----------------------------------------------------
    @property
    def views(self) -> tuple:
        """The views in force (``views.View``), () when off."""
        return self._views

    @property
    def T(self) -> int:
        """The samples the head averages: MC-Dropout passes or ensemble members, times the views."""
        return self._T_head * max(1, len(self._views))

    @property
    def frames_per_call(self) -> int:
        """The most frames one call takes: max_batch // max(1, number of views)."""
        return int(self.cfg.max_batch) // max(1, len(self._views))

    def set_views(self, views):
        """Classify every frame under each of ``views`` (a sequence of ``views.View``, e.g. ``views.hflip()``) and average
        the softmax outputs as further samples, from the next call on; None or empty: off.  Every classify method then takes
        at most ``frames_per_call`` frames a call and costs ``len(views)`` forward passes a frame.  Refused on a handle that
        draws MC-Dropout masks."""
        vs = list(views) if views else []
        arr, n = _views.to_c_array(vs)
        _lib.check(self.lib.fav_set_views(self._h, arr if n else None, n), self._h)
        self._views = tuple(vs)

    def set_conf_kind(self, kind: str):
        """The confidence kind ("max_softmax", "entropy", "mutual_info") of the calls made from now on; "mutual_info" needs
        at least two samples (``T``) and two classes."""
        _lib.check(self.lib.fav_set_conf_kind(self._h, _CONF[kind]), self._h)
        self.cfg.conf_kind = _CONF[kind]

    # -- lifecycle ------------------------------------------------------------
    def load_weights(self, blob: bytes, member: int = 0):
        buf = (C.c_char * len(blob)).from_buffer_copy(blob)
        _lib.check(self.lib.fav_load_member_weights(self._h, int(member), buf, len(blob)), self._h)

    def reset(self):
        """Scorer reset on mode switch (main.py:222,227,242,288).  The classifier is stateless; the rule
        scorer's previous-gray / frozen-run state is cleared like SignalAnalyzer.reset (signal_analyzer.py:37-39)."""
        if self._rules is not None:
            self._rules.reset()

    def close(self):
        if self._h is not None:
            self.lib.fav_destroy(self._h)
            self._h = None

    def __del__(self):
        try:
            self.close()
        except Exception:
            pass

    # -- the hot path ------------------------------------------------------------
    def _layout_of(self, images) -> int:
        torch = self._torch
        dt = images.dtype
        if dt in (torch.uint8, np.uint8):
            return _lib.LAYOUT_NHWC_U8
        if dt in (torch.float32, np.float32):
            return _lib.LAYOUT_NHWC_F32
        raise TypeError(f"frames must be uint8 or float32 NHWC, got {dt}")

    def _check_shape(self, images):
        if images.ndim != 4 or images.shape[1] != self.cfg.in_h or images.shape[2] != self.cfg.in_w or images.shape[3] != 3:
            raise ValueError(f"expected frames of shape (n, {self.cfg.in_h}, {self.cfg.in_w}, 3), got {tuple(images.shape)}")

    def _frames_on_device(self, images, refuse_host: str | None = None):
        """-> (frames on this Backend's GPU, True when they came from the host).  refuse_host: the message with which
        host frames are refused like frames on another device."""
        if isinstance(images, np.ndarray) and refuse_host is None:
            return self._torch.from_numpy(np.ascontiguousarray(images)).to(f"cuda:{self.device}"), True
        if isinstance(images, np.ndarray) or not images.is_cuda or images.device.index != self.device:
            raise ValueError(refuse_host or f"frames must live on cuda:{self.device}")
        return images.contiguous(), False

    def _classify_args(self, images, keep_host: bool = False, refuse_host: str | None = None):
        """The prelude of every classify method -> (frames, from the host?, n, layout, stream).  The frames are on this
        Backend's GPU and the stream is its current one, except with keep_host, where host frames stay a contiguous numpy
        array and the stream is None."""
        self._check_shape(images)
        layout = self._layout_of(images)
        n = int(images.shape[0])
        if keep_host and isinstance(images, np.ndarray):
            return np.ascontiguousarray(images), True, n, layout, None
        img, host = self._frames_on_device(images, refuse_host)
        return img, host, n, layout, self._torch.cuda.current_stream(img.device).cuda_stream

    def _records_out(self, out, n: int, width: int, dev):
        """-> ``out``, or a new buffer when it is None: a contiguous int32[n, width] tensor on the frames' device."""
        torch = self._torch
        if out is None:
            return torch.empty((n, width), dtype=torch.int32, device=dev)
        if out.dtype != torch.int32 or tuple(out.shape) != (n, width) or not out.is_contiguous() or out.device != dev:
            raise ValueError(f"out must be a contiguous int32[n, {width}] tensor on the frames' device")
        return out

    def _batches(self, n: int):
        """(b, e) over n frames, frames_per_call at a time."""
        mb = self.frames_per_call
        return ((b, min(n, b + mb)) for b in range(0, n, mb))

    def _detect_buffers(self, n: int, dev, first: int = 0) -> tuple:
        """-> new (labels int32[n], conf fp32[n], fail uint8[n], score fp32[n]) on ``dev``: what fav_classify_ex writes.
        ``first`` = 2: the (fail, score) half alone, for a head that writes labels and confidences into its records."""
        torch = self._torch
        dtypes = (torch.int32, torch.float32, torch.uint8, torch.float32)
        return tuple(torch.empty(n, dtype=dt, device=dev) for dt in dtypes[first:])

    def classify_detect(self, images, first_index: int = 0):
        """-> (labels int32[n], confidences fp32[n], fail uint8[n], anomaly_score fp32[n]).
        torch CUDA tensors in -> torch CUDA tensors out (asynchronous on the current
        stream); numpy in -> numpy out (synchronous)."""
        img, host, n, layout, stream = self._classify_args(images, keep_host=True)
        if host:
            labels = np.empty(n, np.int32); conf = np.empty(n, np.float32)
            fail = np.empty(n, np.uint8); score = np.empty(n, np.float32)
            _lib.check(self.lib.fav_classify_host(self._h, img.ctypes.data, n, layout, int(first_index),
                                                  labels.ctypes.data, conf.ctypes.data, fail.ctypes.data,
                                                  score.ctypes.data), self._h)
            return labels, conf, fail, score
        labels, conf, fail, score = self._detect_buffers(n, img.device)
        _lib.check(self.lib.fav_classify_ex(self._h, img.data_ptr(), n, layout, int(first_index), labels.data_ptr(),
                                            conf.data_ptr(), fail.data_ptr(), score.data_ptr(), stream), self._h)
        return labels, conf, fail, score

    def classify_records(self, images, first_index: int = 0, out=None):
        """frames (CUDA tensor) -> int32[n, 2] CUDA tensor of packed (label, confidence bits) records, written by the
        confidence head itself (fav_classify_records).  ``out``: a contiguous int32[n, 2] view to write into - e.g. this
        rank's slot of an all-gather send buffer (distributed.classify_sharded), so nothing is packed or copied."""
        img, _, n, layout, stream = self._classify_args(images, refuse_host=f"classify_records takes frames on cuda:{self.device}")
        out = self._records_out(out, n, 2, img.device)
        _lib.check(self.lib.fav_classify_records(self._h, img.data_ptr(), n, layout, int(first_index), out.data_ptr(),
                                                 None, None, stream), self._h)
        return out

    def classify_uncertainty(self, images, first_index: int = 0, out=None) -> dict:
        """frames -> the uncertainty decomposition of the T samples (fav_classify_uncertainty; fields: include/fav.h
        fav_uncertainty): a dict of ``label``, ``confidence``, ``mean_prob``, ``prob_std``, ``pred_entropy``,
        ``expected_entropy``, ``mutual_info``, ``agreement`` ([n]), ``top_label``, ``top_prob`` ([n, 5]) - views of one
        int32[n, 18] record buffer (``unpack_uncertainty``) - plus ``fail`` (uint8[n]) and ``score`` (fp32[n]).
        torch CUDA frames in -> CUDA tensors out, asynchronous on the current stream; numpy in -> numpy out (the frames
        are uploaded, the call is synchronous).  ``out``: a contiguous int32[n, 18] tensor on the frames' device to write
        the records into (e.g. this rank's slot of an all-gather send buffer).
        A non-finite frame (include/fav.h: a NaN or +inf among a sample's scaled logits, or a sample -inf throughout):
        label 0, confidence 0, fail 1 whatever tau is, score 1; the other statistics NaN, top_label -1, top_prob 0."""
        img, host, n, layout, stream = self._classify_args(images)
        out = self._records_out(out, n, UNCERTAINTY_DWORDS, img.device)
        fail, score = self._detect_buffers(n, img.device, first=2)
        _lib.check(self.lib.fav_classify_uncertainty(self._h, img.data_ptr(), n, layout, int(first_index), out.data_ptr(),
                                                     fail.data_ptr(), score.data_ptr(), stream), self._h)
        if host:
            out, fail, score = out.cpu().numpy(), fail.cpu().numpy(), score.cpu().numpy()   # synchronises the stream
        return dict(unpack_uncertainty(out), fail=fail, score=score)

    # -- conformal prediction sets (conformal.py; include/fav.h fav_classify_sets) ---------------------------------------
    def conformal_scores(self, images, labels, cp, first_index: int = 0):
        """Calibration scores s(y) of the true classes ``labels`` (int[n]) under ``cp`` (a ``conformal.Conformal``; its qhat
        is not used), fp32[n], NaN where a label lies outside [0, num_classes).  Frame i has global index first_index + i
        (the key of a randomized score's draw); batches of frames_per_call frames.  torch CUDA frames in -> CUDA tensor out,
        asynchronous on the current stream; numpy in -> numpy out, synchronous."""
        torch = self._torch
        img, host, n, layout, stream = self._classify_args(images)
        lab = self._labels_on(labels, n, img.device)
        out = torch.empty(n, dtype=torch.float32, device=img.device)
        c = cp.to_c()
        for b, e in self._batches(n):
            _lib.check(self.lib.fav_conformal_scores(self._h, img[b:e].data_ptr(), e - b, layout, int(first_index) + b,
                                                     C.byref(c), lab[b:e].data_ptr(), out[b:e].data_ptr(), stream), self._h)
        return out.cpu().numpy() if host else out

    def calibrate_conformal(self, images, labels, alpha: float, method: str = "aps", randomized: bool = True,
                            lam: float = 0.0, k_reg: int = 0, first_index: int = 0, seed: int = 0):
        """Split-conformal calibration on held-out labelled frames -> a ``conformal.Conformal`` with ``qhat`` set, so that
        ``classify_sets`` covers the true class with probability >= 1 - alpha.  ``method``: "lac", "aps" or "raps"
        (APS with ``lam`` > 0 and ``k_reg``); ``randomized`` (APS / RAPS only) draws u per frame from ``seed``."""
        from .conformal import Conformal, calibrate_qhat
        if method not in ("lac", "aps", "raps"):
            raise ValueError(f"method must be 'lac', 'aps' or 'raps', got {method!r}")
        kind = "lac" if method == "lac" else "aps"
        cp = Conformal(kind=kind, randomized=bool(randomized) and kind == "aps", lam=float(lam), k_reg=int(k_reg), seed=int(seed))
        s = _to_numpy(self.conformal_scores(images, labels, cp, first_index=first_index))
        return dataclasses.replace(cp, qhat=calibrate_qhat(s, alpha))

    def classify_sets(self, images, cp, first_index: int = 0, out=None) -> dict:
        """frames -> their conformal prediction sets under ``cp`` (fav_classify_sets): ``unpack_sets`` of one int32[n, 40]
        record buffer (``label``, ``confidence``, ``set_size``, ``set_mass``, ``u``, ``members`` bool[n, num_classes])
        plus ``fail`` (uint8[n], conf < tau), ``score`` (fp32[n]) and ``ambiguous`` (set_size != 1: the set-valued
        failure flag).  torch CUDA frames in -> CUDA tensors out, asynchronous on the current stream; numpy in -> numpy
        out, synchronous.  ``out``: a contiguous int32[n, 40] tensor on the frames' device to write the records into
        (e.g. this rank's slot of an all-gather send buffer).
        A non-finite frame (include/fav.h): label 0, confidence 0, fail 1 whatever tau is, score 1, an empty set
        (set_size 0, set_mass 0, hence ambiguous); its calibration score is NaN, which calibrate_conformal refuses."""
        from .conformal import PRED_SET_DWORDS, unpack_sets
        img, host, n, layout, stream = self._classify_args(images)
        out = self._records_out(out, n, PRED_SET_DWORDS, img.device)
        fail, score = self._detect_buffers(n, img.device, first=2)
        c = cp.to_c()
        _lib.check(self.lib.fav_classify_sets(self._h, img.data_ptr(), n, layout, int(first_index), C.byref(c),
                                              out.data_ptr(), fail.data_ptr(), score.data_ptr(), stream), self._h)
        if host:
            out, fail, score = out.cpu().numpy(), fail.cpu().numpy(), score.cpu().numpy()   # synchronises the stream
        r = unpack_sets(out, self.cfg.num_classes)
        return dict(r, fail=fail, score=score, ambiguous=r["set_size"] != 1)

    # -- temperature / tau calibration (calibration.py; include/fav.h fav_classify_sweep) --------------------------------
    def _labels_on(self, labels, n: int, dev):
        torch = self._torch
        if int(np.shape(labels)[0] if isinstance(labels, np.ndarray) else labels.shape[0]) != n:
            raise ValueError("one label per frame")
        return (torch.from_numpy(np.asarray(labels)) if isinstance(labels, np.ndarray) else labels).to(dev, torch.int32).contiguous()

    @staticmethod
    def _temps_c(temperatures):
        t = np.ascontiguousarray(np.asarray(temperatures, np.float32).ravel())
        if not 1 <= t.size <= _lib.SWEEP_MAX_TEMPS:
            raise ValueError(f"between 1 and {_lib.SWEEP_MAX_TEMPS} temperatures per sweep, got {t.size}")
        return t, t.ctypes.data_as(C.POINTER(C.c_float))

    def _sweep_logits(self, lg, lab, temps):
        """The sweep head alone (fav_op_head_sweep) on fp32 logits [T, n, ld] kept on the device, of which the first
        num_classes columns count -> int32[n, K, 4] cells."""
        torch = self._torch
        t, tp = self._temps_c(temps)
        T, n, ld = (int(x) for x in lg.shape)
        cells = torch.empty((n, t.size, 4), dtype=torch.int32, device=lg.device)
        _lib.check(self.lib.fav_op_head_sweep(lg.data_ptr(), T, n, self.cfg.num_classes, ld, tp, t.size, self.cfg.conf_kind,
                                              lab.data_ptr(), cells.data_ptr(), torch.cuda.current_stream(lg.device).cuda_stream))
        return cells

    def calibration_sweep(self, images, labels, temperatures, first_index: int = 0, _keep_logits=None):
        """The confidence head at every one of ``temperatures`` (1 to 32 of them) in one launch per batch
        (fav_classify_sweep): int32[n, K, 4] cells, ``calibration.unpack_cells`` -> label, confidence, nll, brier per
        (frame, temperature), ``labels`` (int[n]) being the frames' true classes.  The handle's own temperature is not
        used.  Batches of frames_per_call frames; torch CUDA frames in -> CUDA tensor out, asynchronous on the current stream;
        numpy in -> numpy out, synchronous.  A frame that is non-finite at a temperature (include/fav.h) has label 0,
        confidence 0 and NaN nll / brier in that cell; the temperature fit refuses a set that holds one."""
        torch = self._torch
        img, host, n, layout, stream = self._classify_args(images)
        dev = img.device
        lab = self._labels_on(labels, n, dev)
        t, tp = self._temps_c(temperatures)
        cells = torch.empty((n, t.size, 4), dtype=torch.int32, device=dev)
        for b, e in self._batches(n):
            _lib.check(self.lib.fav_classify_sweep(self._h, img[b:e].data_ptr(), e - b, layout, int(first_index) + b,
                                                   lab[b:e].data_ptr(), tp, t.size, cells[b:e].data_ptr(), stream), self._h)
            if _keep_logits is not None:
                lg = self.logits()                                  # [T, e - b, C], this batch's
                ld = (lg.shape[2] + 3) // 4 * 4                     # the head reads rows of a multiple of 4 floats
                if ld != lg.shape[2]:
                    lg = torch.nn.functional.pad(lg, (0, ld - lg.shape[2]))
                _keep_logits.append((lg, lab[b:e]))
        return cells.cpu().numpy() if host else cells

    def calibrate_temperature(self, images, labels, lo: float = 0.25, hi: float = 8.0, rtol: float = 1e-3,
                              first_index: int = 0, logits_budget_bytes: int = 8 << 30):
        """Fit the softmax temperature on held-out labelled frames by minimum mean NLL (``calibration.fit_temperature``)
        -> a ``TemperatureFit`` (temperature, nll, at_bound, rounds).  ONE forward pass per batch: the first grid runs
        through fav_classify_sweep, its logits stay on the device, and the finer grids run the sweep head alone on them
        (fav_op_head_sweep).  A calibration set whose logits exceed ``logits_budget_bytes`` is refused.  The handle is
        not changed: see ``set_temperature`` / ``apply``."""
        from .calibration import fit_temperature, unpack_cells
        n = int(images.shape[0])
        need = 4 * self.T * n * ((int(self.cfg.num_classes) + 3) // 4 * 4)
        if need > int(logits_budget_bytes):
            raise ValueError(f"calibrate_temperature keeps the calibration set's logits on the device: {self.T} samples (views "
                             f"included) x {n} "
                             f"frames x {self.cfg.num_classes} classes = {need} bytes ({need / 2**30:.2f} GiB) exceed "
                             f"logits_budget_bytes = {int(logits_budget_bytes)}; calibrate on fewer frames")
        kept = []

        def sum_nll(cells):
            return unpack_cells(_to_numpy(cells))["nll"].astype(np.float64).sum(axis=0)

        def nll_of(temps):
            if not kept:
                return sum_nll(self.calibration_sweep(images, labels, temps, first_index, _keep_logits=kept)) / n
            return sum(sum_nll(self._sweep_logits(lg, lab, temps)) for lg, lab in kept) / n
        return fit_temperature(nll_of, lo=lo, hi=hi, rtol=rtol)

    def _detect_batched(self, images, first_index: int = 0):
        """classify_detect over batches of frames_per_call frames -> numpy (labels, conf)."""
        out_l, out_c = [], []
        for b, e in self._batches(int(images.shape[0])):
            l, c, _, _ = self.classify_detect(images[b:e], int(first_index) + b)
            out_l.append(_to_numpy(l))
            out_c.append(_to_numpy(c))
        return np.concatenate(out_l), np.concatenate(out_c)

    def calibrate_tau(self, images, labels, target_risk: float, delta: float | None = None, first_index: int = 0) -> dict:
        """The failure threshold for a target selective risk at the handle's CURRENT temperature (calibrate that first):
        classify the held-out frames, then ``calibration.tau_for_risk`` -> dict tau, coverage, risk, bound.  ``delta``:
        the guarantee's failure probability (None: the empirical risk decides).  The handle is not changed."""
        from .calibration import tau_for_risk
        pred, conf = self._detect_batched(images, first_index)
        return tau_for_risk(conf, pred == np.asarray(_to_numpy(labels)).ravel(), target_risk, delta)

    def calibration_report(self, images, labels, first_index: int = 0) -> dict:
        """What the confidence is worth on labelled frames at the current temperature (a one-temperature sweep):
        accuracy, mean_confidence, nll, brier, ece, mce, aurc."""
        from .calibration import report_from_cells
        cells = self.calibration_sweep(images, labels, [self.cfg.temperature], first_index)
        return report_from_cells(_to_numpy(cells), _to_numpy(labels))

    def robustness_report(self, frames_u8, labels, corruptions=CORRUPTIONS, severities=(1, 2, 3, 4, 5), seed: int = 0,
                          first_index: int = 0) -> dict:
        """How accuracy, confidence and the failure flag hold up as corruptions get worse: a ``"clean"`` row and one row
        per (kind, severity) of ``corruptions`` (default ``corrupt.CORRUPTIONS``) -> ``{("clean", 0): row, (kind, s): row}``,
        each row ``robustness.summarize`` at the handle's current temperature and tau (``robustness.table`` prints them).
        ``frames_u8``: labelled uint8 frames (numpy or CUDA); they are corrupted on the device in batches of frames_per_call
        (``Corruptor(seed).imagenet_c``, frame i at global index first_index + i) and each batch runs through
        ``calibration_sweep`` as fp32 frames.  The handle is not changed."""
        from .calibration import unpack_cells
        from .corrupt import Corruptor
        from .robustness import summarize
        torch = self._torch
        self._check_shape(frames_u8)
        if self._layout_of(frames_u8) != _lib.LAYOUT_NHWC_U8:
            raise TypeError("robustness_report takes uint8 frames")
        img, _ = self._frames_on_device(frames_u8)
        n = int(img.shape[0])
        lab = self._labels_on(labels, n, img.device)
        lab_host = lab.cpu().numpy()
        cor = Corruptor(seed=seed)
        temps = [self.cfg.temperature]

        def row(make):
            cells = [self.calibration_sweep(make(img[b:e], int(first_index) + b), lab[b:e], temps, int(first_index) + b)
                     for b, e in self._batches(n)]
            c = unpack_cells(torch.cat(cells).cpu().numpy())
            return summarize(c["label"][:, 0], c["confidence"][:, 0], c["nll"][:, 0], lab_host, self.cfg.tau)

        rows = {("clean", 0): row(lambda fr, first: fr)}
        for kind in corruptions:
            for s in severities:
                rows[(kind, int(s))] = row(lambda fr, first: cor.imagenet_c(fr, kind, int(s), first_index=first))
        return rows

    def set_temperature(self, temperature: float):
        """Softmax temperature of the calls made from now on (finite, > 0); calls already enqueued keep the old one."""
        _lib.check(self.lib.fav_set_temperature(self._h, float(temperature)), self._h)
        self.cfg.temperature = float(temperature)

    def set_tau(self, tau: float):
        """Failure threshold (fail = conf < tau) of the calls made from now on; not NaN."""
        _lib.check(self.lib.fav_set_tau(self._h, float(tau)), self._h)
        self.cfg.tau = float(tau)

    def apply(self, cal):
        """Adopt a ``calibration.Calibration``: its temperature and tau."""
        self.set_temperature(cal.temperature)
        self.set_tau(cal.tau)

    def classify(self, images, first_index: int = 0):
        """The drop-in: frames -> (labels, confidences)."""
        labels, conf, _, _ = self.classify_detect(images, first_index)
        return labels, conf

    def logits(self):
        """fp32 [T, n, num_classes] logits of the last classify call (torch CUDA tensor)."""
        torch = self._torch
        t, n = C.c_int32(), C.c_int32()
        _lib.check(self.lib.fav_get_logits(self._h, None, C.byref(t), C.byref(n), None), self._h)
        out = torch.empty((t.value, n.value, self.cfg.num_classes), dtype=torch.float32, device=f"cuda:{self.device}")
        stream = torch.cuda.current_stream(out.device).cuda_stream
        _lib.check(self.lib.fav_get_logits(self._h, out.data_ptr(), None, None, stream), self._h)
        return out

    # -- feature tap and feature-space OOD scoring (ood.py; include/fav.h fav_set_ood) -----------------------------------
    def set_feature_tap(self, enable: bool):
        """Keep the rows the final fc layer reads (fav_set_feature_tap) from the next call on; ``features()`` reads them.
        Turning it off is refused while an OOD model is set, which reads it."""
        _lib.check(self.lib.fav_set_feature_tap(self._h, 1 if enable else 0), self._h)
        self._tap = bool(enable)

    def features(self):
        """fp32 [S, n, D] features of the last classify call made with the tap on (torch CUDA tensor), indexed like
        ``logits()``: the pooled features the fc layer read (post-dropout when the pooled-feature site is active), or the
        ViT's final class tokens."""
        torch = self._torch
        s, n, d = C.c_int32(), C.c_int32(), C.c_int32()
        _lib.check(self.lib.fav_get_features(self._h, None, C.byref(s), C.byref(n), C.byref(d), None), self._h)
        out = torch.empty((s.value, n.value, d.value), dtype=torch.float32, device=f"cuda:{self.device}")
        stream = torch.cuda.current_stream(out.device).cuda_stream
        _lib.check(self.lib.fav_get_features(self._h, out.data_ptr(), None, None, None, stream), self._h)
        return out

    # -- class activation maps (cam.py; include/fav.h fav_set_map_tap, fav_cam) ---------------------------------------------
    def set_map_tap(self, enable: bool, budget_bytes: int = 2 << 30):
        """Keep the feature maps the average pool reads (fav_set_map_tap) from the next call on; ``maps()``, ``cam()`` and
        ``classify_cam()`` read them.  The buffer is allocated here, for max_batch frames (``map_tap_info()['bytes']``), and
        refused above ``budget_bytes``; turning the tap off frees it.  Refused on a ViT arch and on a deep ensemble."""
        _lib.check(self.lib.fav_set_map_tap(self._h, 1 if enable else 0, int(budget_bytes)), self._h)
        self._map_tap_on = bool(enable)
        if enable and self._map_hw is None:
            info = self.map_tap_info()                 # the planner, once: classify_cam sizes its outputs from this
            self._map_hw = (info["hf"], info["wf"])

    def map_tap_info(self) -> dict:
        """What the map tap of this configuration holds, from the planner alone (fav_map_tap_info; no device work):
        ``bytes`` of the buffer, ``samples`` a frame has in it (without views), and the map's ``hf``, ``wf``, ``c``."""
        return self._tap_info(self.lib.fav_map_tap_info, ("samples", "hf", "wf", "c"))

    def _map_sizes(self) -> tuple:
        """(S, n, Hf, Wf, C) of the maps the last tapped call left."""
        v = [C.c_int32() for _ in range(5)]
        _lib.check(self.lib.fav_get_maps(self._h, None, *(C.byref(x) for x in v), None), self._h)
        return tuple(x.value for x in v)

    def maps(self):
        """bf16 [S, n, Hf, Wf, C] feature maps of the last classify call made with the map tap on (torch CUDA tensor),
        indexed like ``logits()``: what the average pool read - behind the dropout of every block site, in front of the
        pooled-feature site's (S = 1 when that is the only site)."""
        torch = self._torch
        shape = self._map_sizes()
        out = torch.empty(shape, dtype=torch.bfloat16, device=f"cuda:{self.device}")
        stream = torch.cuda.current_stream(out.device).cuda_stream
        _lib.check(self.lib.fav_get_maps(self._h, out.data_ptr(), None, None, None, None, None, stream), self._h)
        return out

    # -- the stage tap (include/fav.h fav_set_stage_tap) ---------------------------------------------------
    def stage_tap_info(self, stage: int) -> dict:
        """What the stage tap of this configuration holds for residual stage 1 .. 4 (torchvision's layer1 .. layer4), from the
        planner alone (fav_stage_tap_info; no device work): ``bytes``, ``samples``, ``hf``, ``wf``, ``c``."""
        return self._tap_info(lambda cfg, *rest: self.lib.fav_stage_tap_info(cfg, int(stage), *rest), ("samples", "hf", "wf", "c"))

    def set_stage_tap(self, stage: int, budget_bytes: int = 2 << 30):
        """Keep the output of residual stage ``stage``'s last block (fav_set_stage_tap) from the next call on; ``stage_maps()``
        reads it, and so does a patch bank at that stage.  0: off.  One stage at a time; another stage reallocates.  Refused on
        a ViT arch, on a deep ensemble, above ``budget_bytes`` and for a stage whose map has more than 1024 cells."""
        _lib.check(self.lib.fav_set_stage_tap(self._h, int(stage), int(budget_bytes)), self._h)
        self._stage_tap = int(stage)

    def stage_maps(self):
        """bf16 [S, n, Hf, Wf, C] maps of the last classify call made with the stage tap on (torch CUDA tensor), indexed like
        ``maps()``: the output of the tapped stage's last block."""
        torch = self._torch
        v = [C.c_int32() for _ in range(6)]
        _lib.check(self.lib.fav_get_stage_maps(self._h, None, *(C.byref(x) for x in v), None), self._h)
        out = torch.empty(tuple(x.value for x in v[1:]), dtype=torch.bfloat16, device=f"cuda:{self.device}")
        stream = torch.cuda.current_stream(out.device).cuda_stream
        _lib.check(self.lib.fav_get_stage_maps(self._h, out.data_ptr(), None, None, None, None, None, None, stream), self._h)
        return out

    def cam(self, classes) -> dict:
        """Class activation maps of the LAST classify call for the classes named per frame (fav_cam; no second forward
        pass): ``classes`` int [n, K] or [n], K <= 8 -> ``map`` fp32 [n, K, Hf, Wf] (the mean over the samples of
        w_c . F(h, w): its spatial mean plus the bias is the class's mean logit) plus the record fields of
        ``cam.unpack_cam_records``, each [n, K]: ``class_id``, ``logit_mean``, ``peak``, ``peak_cell``, ``floor``, ``pos_sum``,
        ``n_above`` (cells at 20 % of the peak or more), ``box`` and its ``x0``, ``y0``, ``x1``, ``y1``.  A class outside
        [0, num_classes) gives a NaN map and class_id -1.  torch CUDA classes in -> CUDA tensors out, asynchronous on the
        current stream; numpy in -> numpy out.  Needs the map tap; refused while views are set."""
        from .cam import CAM_RECORD_DWORDS, unpack_cam_records
        torch = self._torch
        host = isinstance(classes, np.ndarray) or not hasattr(classes, "is_cuda")
        dev = torch.device(f"cuda:{self.device}")
        cls = torch.as_tensor(np.asarray(classes) if host else classes).to(device=dev, dtype=torch.int32)
        if cls.ndim == 1:
            cls = cls[:, None]
        cls = cls.contiguous()
        v = [C.c_int32() for _ in range(5)]
        if self.lib.fav_get_maps(self._h, None, *(C.byref(x) for x in v), None) != _lib.FAV_OK:
            # no maps to size the outputs by (the tap is off, or no call since it went on): fav_cam says so in its own words
            _lib.check(self.lib.fav_cam(self._h, cls.data_ptr(), 1, cls.data_ptr(), cls.data_ptr(), None), self._h)
            raise RuntimeError("fav_get_maps has no maps, yet fav_cam accepted the call")
        _, n, hf, wf, _ = (x.value for x in v)
        if cls.ndim != 2 or int(cls.shape[0]) != n:
            raise ValueError(f"classes must be [n, K] or [n] for the n={n} frames of the last call, got {tuple(cls.shape)}")
        K = int(cls.shape[1])
        cam = torch.empty((n, K, hf, wf), dtype=torch.float32, device=dev)
        rec = torch.empty((n, K, CAM_RECORD_DWORDS), dtype=torch.int32, device=dev)
        stream = torch.cuda.current_stream(dev).cuda_stream
        _lib.check(self.lib.fav_cam(self._h, cls.data_ptr(), K, cam.data_ptr(), rec.data_ptr(), stream), self._h)
        if host:
            cam, rec = cam.cpu().numpy(), rec.cpu().numpy()
        return dict(unpack_cam_records(rec), map=cam)

    def classify_cam(self, images, heatmap: bool = False, first_index: int = 0) -> dict:
        """frames -> ``label``, ``conf``, ``fail``, ``score`` as ``classify_detect`` gives them, plus the class activation
        map of each frame's predicted class (fav_classify_cam: the class is read on the device, nothing synchronises):
        ``map`` fp32 [n, Hf, Wf] and the record fields of ``cam()``, each [n].  ``heatmap``: also ``heatmap`` uint8 [n, H, W],
        the map resized to the frame (bilinear) and normalised from its floor to its peak - the overlay a dashboard draws.
        torch CUDA frames in -> CUDA tensors out, asynchronous on the current stream; numpy in -> numpy out, synchronous.
        Needs the map tap; refused while views are set."""
        from .cam import CAM_RECORD_DWORDS, unpack_cam_records
        # never tapped: fav_classify_cam refuses before it writes anything
        return self._classify_map_head(self.lib.fav_classify_cam, (), self._map_hw or (1, 1), CAM_RECORD_DWORDS, unpack_cam_records,
                                       images, heatmap, first_index)

    # -- attention rollout (rollout.py; include/fav.h fav_set_attn_tap, fav_rollout) --------------------------------------------
    def set_attn_tap(self, enable: bool, budget_bytes: int = 2 << 30):
        """Keep every encoder layer's head-mean attention (fav_set_attn_tap) from the next call on; ``attention()``,
        ``rollout()`` and ``classify_rollout()`` read it.  The buffer is allocated here, for max_batch frames
        (``attn_tap_info()['bytes']``), and refused above ``budget_bytes``; turning the tap off frees it.  Refused on a ResNet
        arch, on a deep ensemble and in the exact math mode."""
        _lib.check(self.lib.fav_set_attn_tap(self._h, 1 if enable else 0, int(budget_bytes)), self._h)
        self._attn_tap_on = bool(enable)
        if enable and self._attn_grid is None:
            info = self.attn_tap_info()                # the planner, once: classify_rollout sizes its outputs from this
            from .rollout import VIT_PATCH
            self._attn_grid = (int(self.cfg.in_h) // VIT_PATCH, int(self.cfg.in_w) // VIT_PATCH)
            assert self._attn_grid[0] * self._attn_grid[1] + 1 == info["tokens"]

    def attn_tap_info(self) -> dict:
        """What the attention tap of this configuration holds, from the planner alone (fav_attn_tap_info; no device work):
        ``bytes`` of the buffer, its ``layers``, the ``tokens`` of a frame and the row pitch ``ld`` (tokens rounded up to 16)."""
        return self._tap_info(self.lib.fav_attn_tap_info, ("layers", "tokens", "ld"))

    def attention(self):
        """fp32 [L, n, T, T] head-mean attention of the last classify call made with the attention tap on (torch CUDA tensor,
        a view of the padded buffer with the padding cut off): row t of layer l is how query token t spreads over the keys,
        token 0 the class token.  Under views n is frames x views, indexed like ``logits()``."""
        torch = self._torch
        v = [C.c_int32() for _ in range(4)]
        _lib.check(self.lib.fav_get_attention(self._h, None, *(C.byref(x) for x in v), None), self._h)
        L, n, T, ld = (x.value for x in v)
        out = torch.empty((L, n, T, ld), dtype=torch.float32, device=f"cuda:{self.device}")
        stream = torch.cuda.current_stream(out.device).cuda_stream
        _lib.check(self.lib.fav_get_attention(self._h, out.data_ptr(), None, None, None, None, stream), self._h)
        return out[..., :T]

    def rollout(self, first_layer: int = 0) -> dict:
        """Attention rollout of the LAST classify call (fav_rollout; no second forward pass), over the layers
        ``first_layer`` .. L-1: ``map`` fp32 [n, gh, gw] (how much each patch fed the class token) plus the record fields of
        ``rollout.unpack_rollout_records``, each [n].  CUDA tensors, asynchronous on the current stream.  Needs the attention
        tap; refused while views are set."""
        from .rollout import ROLLOUT_RECORD_DWORDS, unpack_rollout_records
        torch = self._torch
        dev = torch.device(f"cuda:{self.device}")
        stream = torch.cuda.current_stream(dev).cuda_stream
        v = [C.c_int32() for _ in range(4)]
        if self.lib.fav_get_attention(self._h, None, *(C.byref(x) for x in v), None) != _lib.FAV_OK:
            # nothing to size the outputs by (the tap is off, or no call since it went on): fav_rollout says so in its own words
            dummy = torch.empty(8, dtype=torch.int32, device=dev)
            _lib.check(self.lib.fav_rollout(self._h, int(first_layer), dummy.data_ptr(), dummy.data_ptr(), stream), self._h)
            raise RuntimeError("fav_get_attention has nothing, yet fav_rollout accepted the call")
        n = v[1].value
        gh, gw = self._attn_grid
        m = torch.empty((n, gh, gw), dtype=torch.float32, device=dev)
        rec = torch.empty((n, ROLLOUT_RECORD_DWORDS), dtype=torch.int32, device=dev)
        _lib.check(self.lib.fav_rollout(self._h, int(first_layer), m.data_ptr(), rec.data_ptr(), stream), self._h)
        return dict(unpack_rollout_records(rec), map=m)

    def classify_rollout(self, images, heatmap: bool = False, first_layer: int = 0, first_index: int = 0) -> dict:
        """frames -> ``label``, ``conf``, ``fail``, ``score`` as ``classify_detect`` gives them, plus the attention rollout of
        each frame (fav_classify_rollout; nothing synchronises): ``map`` fp32 [n, gh, gw] and the record fields of
        ``rollout()``, each [n].  ``heatmap``: also ``heatmap`` uint8 [n, H, W], the map resized to the frame (bilinear) and
        normalised from its floor to its peak by fav_op_cam_heatmap - the overlay a dashboard draws.  torch CUDA frames in ->
        CUDA tensors out, asynchronous on the current stream; numpy in -> numpy out, synchronous.  Needs the attention tap;
        refused while views are set."""
        from .rollout import ROLLOUT_RECORD_DWORDS, unpack_rollout_records
        # never tapped: fav_classify_rollout refuses before it writes anything
        return self._classify_map_head(self.lib.fav_classify_rollout, (int(first_layer),), self._attn_grid or (1, 1),
                                       ROLLOUT_RECORD_DWORDS, unpack_rollout_records, images, heatmap, first_index)

    # -- deletion / insertion curves (faithfulness.py; include/fav.h fav_set_curve, fav_classify_curve) -------------------------
    def set_curve(self, steps: int | None = 16, fill=None):
        """Prepare the handle for ``classify_curve`` (fav_set_curve): curves of ``steps`` steps (1 .. 256), an occluded pixel
        becoming ``fill`` - a number in [0, 1] or a 3-tuple of them, stored as round(255 fill) in uint8 frames and as the fp32
        itself in fp32 frames; default 128 / 255 for uint8 frames, 0.5 for fp32 ones.  Everything a later call needs is allocated
        here, for max_batch frames.  ``steps`` None: clear.  Refused while views are set, and views are refused while this is."""
        if steps is None:
            _lib.check(self.lib.fav_set_curve(self._h, None), self._h)
            self._curve_steps = None
            return
        d = _lib.FavCurve()
        d.struct_size = C.sizeof(_lib.FavCurve)
        d.steps = int(steps)
        d.fill_u8[:], d.fill_f32_bits[:] = self._fill_words(fill)
        _lib.check(self.lib.fav_set_curve(self._h, C.byref(d)), self._h)
        self._curve_steps = int(steps)

    def classify_curve(self, frames, maps, classes=None, mode: str = "deletion", first_index: int = 0) -> dict:
        """The deletion or insertion curve of every frame under its map (fav_classify_curve): ``maps`` fp32 [n, mh, mw], at most
        1024 cells (``classify_cam()['map']``, ``classify_rollout()['map']`` or the caller's own); ``classes`` int [n], or None:
        each frame's label on the unoccluded frame, read on the device.  -> ``curve`` fp32 [n, steps + 1] (the class probability
        after each step), the record fields of ``faithfulness.unpack_curve_records``, each [n], and ``label``, ``confidence`` of
        the unoccluded pass.  Costs steps + 1 forward passes a frame; every pass of a frame draws the same MC-Dropout masks.
        Frames beyond ``frames_per_call`` go in further calls with ``first_index`` advanced.  torch CUDA frames in -> CUDA tensors
        out, asynchronous on the current stream; numpy in -> numpy out.  Needs ``set_curve``."""
        from .faithfulness import CURVE_RECORD_DWORDS, unpack_curve_records
        if mode not in _lib.CURVE_MODES:
            raise ValueError(f"mode must be one of {_lib.CURVE_MODES}, got {mode!r}")
        args = self._classify_args(frames)
        n = args[2]
        m = self._torch.as_tensor(maps).to(device=args[0].device, dtype=self._torch.float32).contiguous()
        if m.ndim != 3 or int(m.shape[0]) != n:
            raise ValueError(f"maps must be [n, mh, mw] for the n={n} frames, got {tuple(m.shape)}")
        mh, mw = int(m.shape[1]), int(m.shape[2])
        S = self._curve_steps if self._curve_steps is not None else 0     # never set: fav_classify_curve refuses before it writes
        return self._classify_perturb_head(
            lambda b, e, img, k, layout, first, cls, labels, conf, curve, rec, stream: self.lib.fav_classify_curve(
                self._h, img, k, layout, first, m[b:e].data_ptr(), mh, mw, cls, _lib.CURVE_MODES.index(mode), labels, conf, curve, rec,
                stream),
            args, classes, "curve", (S + 1,), CURVE_RECORD_DWORDS, unpack_curve_records, False, first_index)

    def faithfulness_report(self, frames, steps: int = 16, seed: int = 0, fill=None, maps=None) -> dict:
        """Is this checkpoint's saliency map faithful on these frames?  The maps come from ``classify_cam`` (ResNet) or
        ``classify_rollout`` (ViT), the needed tap going on and off around the call if it was off; ``maps=`` fp32 [n, mh, mw]
        brings the caller's own (a deep ensemble has no tap and must).  Deletion and insertion curves of ``steps`` steps are run
        on those maps and on ``faithfulness.random_maps(n, (mh, mw), seed)``, each for the frame's own label.  -> the means of
        ``faithfulness.summarize_curves`` - ``deletion_auc``, ``insertion_auc``, ``random_deletion_auc``,
        ``random_insertion_auc``, ``deletion_gain`` = random - map, ``insertion_gain`` = map - random (both positive for a
        faithful map), ``flip_fraction`` - plus ``n``, ``n_nonfinite`` (frames with a NaN curve, left out), ``steps``,
        ``map_hw`` and under ``per_frame`` the four per-frame results.  Leaves the curve descriptor set.  On synthetic
        checkpoints the sign of a gain means nothing."""
        from .faithfulness import random_maps, summarize_curves
        n = int(frames.shape[0])
        if maps is None:
            if int(self.cfg.n_members) > 1:
                raise ValueError("faithfulness_report: a deep ensemble has no map tap; pass maps=")
            vit = int(self.cfg.arch) in (_lib.ARCH_VIT_B16, _lib.ARCH_VIT_TINY)
            tap, head = (self.set_attn_tap, self.classify_rollout) if vit else (self.set_map_tap, self.classify_cam)
            was_on = (self._attn_tap_on if vit else self._map_tap_on)
            if not was_on:
                tap(True)
            try:
                parts = [_to_numpy(head(frames[b:e], first_index=b)["map"]) for b, e in self._batches(n)]
            finally:
                if not was_on:
                    tap(False)
            maps = np.concatenate(parts, axis=0)
        maps = np.ascontiguousarray(_to_numpy(maps), dtype=np.float32)
        mh, mw = int(maps.shape[1]), int(maps.shape[2])
        rnd = random_maps(n, (mh, mw), seed)
        self.set_curve(steps, fill)
        runs = {}
        for name, mp in (("map", maps), ("random", rnd)):
            for mode in _lib.CURVE_MODES:
                r = self.classify_curve(frames, mp, None, mode)
                runs[f"{name}_{mode}"] = {k: _to_numpy(v) for k, v in r.items()}
        rep = summarize_curves(runs["map_deletion"], runs["map_insertion"], runs["random_deletion"], runs["random_insertion"], mh * mw)
        return dict(rep, steps=int(steps), map_hw=(mh, mw), per_frame=runs)

    # -- RISE saliency (rise.py; include/fav.h fav_set_rise, fav_classify_rise) --------------------------------------------------
    def set_rise(self, n_masks: int | None = 256, grid: int = 7, keep: float = 0.5, seed: int = 0, fill=None):
        """Prepare the handle for ``classify_rise`` (fav_set_rise): ``n_masks`` random masks (1 .. 8192) a frame, each a
        (grid+1) x (grid+1) grid of cells (``grid`` 1 .. 15, at most the frame's shorter side) that are ON with probability
        ``keep`` - stored as round(256 keep), 1 .. 255 -, shifted at random and upsampled bilinearly; ``seed`` keys the draws.  A
        masked-out pixel becomes ``fill`` as in ``set_curve``.  Everything a later call needs is allocated here, for max_batch
        frames.  ``n_masks`` None: clear.  Refused while views are set, and views are refused while this is; independent of
        ``set_curve``."""
        from .rise import keep_threshold
        if n_masks is None:
            _lib.check(self.lib.fav_set_rise(self._h, None), self._h)
            return
        d = _lib.FavRise()
        d.struct_size = C.sizeof(_lib.FavRise)
        d.n_masks, d.grid, d.keep, d.seed = int(n_masks), int(grid), keep_threshold(keep), int(seed) & 0xFFFFFFFFFFFFFFFF
        d.fill_u8[:], d.fill_f32_bits[:] = self._fill_words(fill)
        _lib.check(self.lib.fav_set_rise(self._h, C.byref(d)), self._h)

    def classify_rise(self, frames, classes=None, map_hw=(14, 14), heatmap: bool = False, first_index: int = 0) -> dict:
        """The RISE saliency map of every frame (fav_classify_rise): ``classes`` int [n], or None: each frame's label on the
        unmasked frame, read on the device; ``map_hw`` the cells of the map, at most 1024 and no finer than the frame.  ->
        ``map`` fp32 [n, mh, mw] (the class probability averaged over the masks, weighted by how much of the cell each mask
        showed), the record fields of ``rise.unpack_rise_records``, each [n], and ``label``, ``confidence`` of the unmasked pass.
        ``heatmap``: also ``heatmap`` uint8 [n, H, W], the overlay fav_op_cam_heatmap draws from the map and its record.  Costs
        n_masks + 1 forward passes a frame; every pass of a frame draws the same MC-Dropout masks.  Works on every arch, a deep
        ensemble included: ``faithfulness_report(frames, maps=classify_rise(frames)["map"])`` scores the map.  Frames beyond
        ``frames_per_call`` go in further calls with ``first_index`` advanced.  torch CUDA frames in -> CUDA tensors out,
        asynchronous on the current stream; numpy in -> numpy out.  Needs ``set_rise``."""
        from .rise import RISE_RECORD_DWORDS, unpack_rise_records
        args = self._classify_args(frames)
        mh, mw = (int(v) for v in map_hw)
        if mh < 1 or mw < 1:
            raise ValueError(f"map_hw must be two positive sizes, got {map_hw!r}")
        return self._classify_perturb_head(
            lambda b, e, img, k, layout, first, cls, labels, conf, m, rec, stream: self.lib.fav_classify_rise(
                self._h, img, k, layout, first, cls, mh, mw, labels, conf, m, rec, stream),
            args, classes, "map", (mh, mw), RISE_RECORD_DWORDS, unpack_rise_records, heatmap, first_index)

    # what the two perturbation heads (the curves, RISE) share
    @staticmethod
    def _fill_words(fill) -> tuple:
        """``fill`` - a number in [0, 1], a 3-tuple of them, or None: mid grey - -> (fill_u8, fill_f32_bits), the three words
        each of a fav_curve or fav_rise descriptor."""
        if fill is None:
            u8, f32 = (128, 128, 128), (0.5, 0.5, 0.5)
        else:
            f32 = tuple(float(v) for v in (fill if np.ndim(fill) else (fill,) * 3))
            if len(f32) != 3:
                raise ValueError("fill is a number or a 3-tuple")
            u8 = tuple(int(round(255.0 * v)) for v in f32)
        return [v & 0xFFFFFFFF for v in u8], [int(np.float32(v).view(np.uint32)) for v in f32]

    def _classify_perturb_head(self, call, args, classes, key: str, shape: tuple, record_dwords: int, unpack, heatmap: bool,
                               first_index: int) -> dict:
        """fav_classify_curve / fav_classify_rise behind ``call(b, e, frames, e - b, layout, first_index + b, classes, labels,
        conf, out, records, stream)``, once for every ``frames_per_call`` frames [b, e) of ``args``, the frames'
        ``_classify_args``; ``classes`` int [n] or None.  -> ``unpack`` of the head's int32[n, record_dwords] records plus
        ``label``, ``confidence`` and under ``key`` the head's fp32 [n, *shape] output, with ``heatmap`` its overlay too; numpy
        frames in -> numpy out.  The counterpart of ``_classify_map_head``."""
        torch = self._torch
        img, host, n, layout, stream = args
        dev = img.device
        cls = None
        if classes is not None:
            cls = torch.as_tensor(np.asarray(classes) if not hasattr(classes, "is_cuda") else classes).to(device=dev, dtype=torch.int32)
            cls = cls.contiguous()
            if tuple(cls.shape) != (n,):
                raise ValueError(f"classes must be [n] for the n={n} frames, got {tuple(cls.shape)}")
        res = torch.empty((n, *shape), dtype=torch.float32, device=dev)
        rec = torch.empty((n, record_dwords), dtype=torch.int32, device=dev)
        labels = torch.empty(n, dtype=torch.int32, device=dev)
        conf = torch.empty(n, dtype=torch.float32, device=dev)
        for b, e in (self._batches(n) if n else ()):
            _lib.check(call(b, e, img[b:e].data_ptr(), e - b, layout, int(first_index) + b, cls[b:e].data_ptr() if cls is not None else None,
                            labels[b:e].data_ptr(), conf[b:e].data_ptr(), res[b:e].data_ptr(), rec[b:e].data_ptr(), stream), self._h)
        return self._map_result(unpack, rec, {key: res, "label": labels, "confidence": conf}, host, shape if heatmap else None, stream)

    def _map_result(self, unpack, rec, out: dict, host: bool, heatmap_hw, stream) -> dict:
        """What a head with records hands back: ``unpack(rec)`` plus ``out``, with ``heatmap_hw`` = (mh, mw) also ``heatmap``
        uint8 [n, H, W], the overlay fav_op_cam_heatmap draws from ``out['map']`` and the records; all numpy when ``host``."""
        if heatmap_hw is not None:
            n, H, W = int(rec.shape[0]), int(self.cfg.in_h), int(self.cfg.in_w)
            out["heatmap"] = self._torch.empty((n, H, W), dtype=self._torch.uint8, device=rec.device)
            if n:
                _lib.check(self.lib.fav_op_cam_heatmap(out["map"].data_ptr(), rec.data_ptr(), n, *heatmap_hw, H, W,
                                                       out["heatmap"].data_ptr(), stream))
        if host:
            out = {k: v.cpu().numpy() for k, v in out.items()}
            rec = rec.cpu().numpy()
        return dict(unpack(rec), **out)

    # what the two localisation taps (the map tap with its CAM head, the attention tap with its rollout head) share
    def _tap_info(self, fn, names) -> dict:
        """fav_map_tap_info / fav_attn_tap_info (``fn``) -> ``bytes`` of the buffer and the int32 sizes under ``names``."""
        nbytes, sizes = C.c_size_t(), [C.c_int32() for _ in names]
        err = C.create_string_buffer(256)
        st = fn(C.byref(self.cfg), C.byref(nbytes), *(C.byref(x) for x in sizes), err, len(err))
        if st != _lib.FAV_OK:
            raise _lib.FavError(st, err.value.decode("utf-8", "replace"))
        return dict(bytes=nbytes.value, **{name: x.value for name, x in zip(names, sizes)})

    def _classify_map_head(self, fn, head_args: tuple, map_hw: tuple, record_dwords: int, unpack, images, heatmap: bool,
                           first_index: int) -> dict:
        """fav_classify_cam / fav_classify_rollout (``fn``; ``head_args``: the head's own integers, in front of its outputs) ->
        ``unpack`` of the head's int32[n, record_dwords] records plus ``label``, ``conf``, ``fail``, ``score``, ``map`` fp32
        [n, *map_hw] and, with ``heatmap``, the overlay fav_op_cam_heatmap draws from either record; numpy frames in -> numpy
        out.  The counterpart of ``_classify_feature_head``."""
        torch = self._torch
        img, host, n, layout, stream = self._classify_args(images)
        labels, conf, fail, score = self._detect_buffers(n, img.device)
        m = torch.empty((n, *map_hw), dtype=torch.float32, device=img.device)
        rec = torch.empty((n, record_dwords), dtype=torch.int32, device=img.device)
        _lib.check(fn(self._h, img.data_ptr(), n, layout, int(first_index), labels.data_ptr(), conf.data_ptr(), fail.data_ptr(),
                      score.data_ptr(), *head_args, m.data_ptr(), rec.data_ptr(), stream), self._h)
        return self._map_result(unpack, rec, dict(label=labels, conf=conf, fail=fail, score=score, map=m), host,
                                map_hw if heatmap else None, stream)

    # what the two feature heads (the Mahalanobis model, the k-NN bank) share
    @staticmethod
    def _frame_labels(labels, frames) -> np.ndarray:
        lab = np.asarray(_to_numpy(labels)).ravel()
        if lab.shape[0] != int(frames.shape[0]):
            raise ValueError("one label per frame")
        return lab

    def _tapped_mean_features(self, frames) -> np.ndarray:
        """Batches of frames_per_call frames through the classifier with the tap on -> float64 [n, D], the mean over the
        samples of each frame's features.  A tap that only this call needs goes off again."""
        own_tap = self._ood is None and self._knn is None and self._drift is None and not self._tap
        if own_tap:
            self.set_feature_tap(True)
        try:
            rows = []
            for b, e in self._batches(int(frames.shape[0])):
                self.classify_detect(frames[b:e], b)
                rows.append(self.features().to(self._torch.float64).mean(dim=0).cpu().numpy())
        finally:
            if own_tap:
                self.set_feature_tap(False)
        return np.concatenate(rows)

    def _classify_feature_head(self, fn, record_dwords: int, unpack, images, first_index: int) -> dict:
        """fav_classify_ood / fav_classify_knn (``fn``) -> ``unpack`` of the head's int32[n, record_dwords] records plus
        ``label``, ``conf``, ``fail``, ``score``; numpy frames in -> numpy out."""
        img, host, n, layout, stream = self._classify_args(images)
        labels, conf, fail, score = self._detect_buffers(n, img.device)
        rec = self._torch.empty((n, record_dwords), dtype=self._torch.int32, device=img.device)
        _lib.check(fn(self._h, img.data_ptr(), n, layout, int(first_index), labels.data_ptr(), conf.data_ptr(), fail.data_ptr(),
                      score.data_ptr(), rec.data_ptr(), stream), self._h)
        if host:
            labels, conf, fail, score, rec = (t.cpu().numpy() for t in (labels, conf, fail, score, rec))
        return dict(unpack(rec), label=labels, conf=conf, fail=fail, score=score)

    def _head_distances(self, classify, key: str, frames) -> np.ndarray:
        """``classify`` (classify_ood, classify_knn) over batches of frames_per_call frames -> its ``key`` of every frame."""
        return np.concatenate([_to_numpy(classify(frames[b:e], b)[key]) for b, e in self._batches(int(frames.shape[0]))])

    @property
    def ood_model(self):
        """The ``ood.OODModel`` in force, None when off."""
        return self._ood

    def fit_ood(self, frames, labels, **kw):
        """Fit an ``ood.OODModel`` on labelled in-distribution frames: batches of frames_per_call frames run through the
        classifier with the tap on, the mean over the samples of each frame's features goes to ``ood.fit_mahalanobis``
        (``k``, ``shrinkage``).  The handle is left as it was: see ``set_ood``."""
        from .ood import fit_mahalanobis
        lab = self._frame_labels(labels, frames)
        return fit_mahalanobis(self._tapped_mean_features(frames), lab, **kw)

    def set_ood(self, model):
        """Adopt an ``ood.OODModel`` (fav_set_ood: copied to the device, the tap goes on), or None: off.  Refused on a deep
        ensemble, and for a model whose D is not this arch's feature width."""
        if model is None:
            _lib.check(self.lib.fav_set_ood(self._h, None), self._h)
        else:
            c = model.to_c()
            _lib.check(self.lib.fav_set_ood(self._h, C.byref(c)), self._h)
        self._ood = model

    def classify_ood(self, images, first_index: int = 0) -> dict:
        """frames -> ``label``, ``conf``, ``fail``, ``score`` as ``classify_detect`` gives them, plus the OOD record of each
        frame (fav_classify_ood): ``min_dist`` (squared Mahalanobis distance to the nearest class mean), ``nearest_class``,
        ``label_dist`` (the distance to the predicted class; NaN when the model has no row for it) and ``ood`` (not
        min_dist <= threshold).  torch CUDA frames in -> CUDA tensors out, asynchronous on the current stream; numpy in ->
        numpy out, synchronous."""
        from .ood import OOD_RECORD_DWORDS, unpack_records
        return self._classify_feature_head(self.lib.fav_classify_ood, OOD_RECORD_DWORDS, unpack_records, images, first_index)

    def calibrate_ood(self, frames, tpr: float = 0.95) -> float:
        """Set the model's threshold so that at least ``tpr`` of these in-distribution frames pass, and return it."""
        if self.ood_model is None:
            raise ValueError("calibrate_ood needs a model: set_ood first")
        from .ood import threshold_for_tpr
        thr = threshold_for_tpr(self._head_distances(self.classify_ood, "min_dist", frames), tpr)
        self.set_ood(self.ood_model.with_threshold(thr))
        return thr

    def ood_report(self, id_frames, ood_frames) -> dict:
        """How well min_dist separates ``ood_frames`` from ``id_frames``: auroc, fpr_at_tpr95, the mean distances and, at the
        model's current threshold, the share of each set that is flagged."""
        if self.ood_model is None:
            raise ValueError("ood_report needs a model: set_ood first")
        from .ood import separation_report
        return separation_report(self._head_distances(self.classify_ood, "min_dist", id_frames),
                                 self._head_distances(self.classify_ood, "min_dist", ood_frames), self.ood_model.threshold)

    # -- nearest-neighbour OOD scoring (ood.py KNNBank; include/fav.h fav_set_knn) ----------------------------------------
    @property
    def knn_bank(self):
        """The ``ood.KNNBank`` in force, None when off."""
        return self._knn

    def fit_knn(self, frames, labels=None, **kw):
        """Build an ``ood.KNNBank`` from in-distribution frames: batches of frames_per_call frames run through the classifier
        with the tap on, the mean over the samples of each frame's features goes to ``ood.build_knn_bank`` (``k``,
        ``max_rows``, ``seed``, ``select``: ``"coreset"`` picks the ``max_rows`` rows by greedy k-centre selection on this
        Backend's device).  The handle is left as it was: see ``set_knn``."""
        from .ood import build_knn_bank
        lab = None if labels is None else self._frame_labels(labels, frames)
        kw.setdefault("device", self.device)
        return build_knn_bank(self._tapped_mean_features(frames), lab, **kw)

    def set_knn(self, bank):
        """Adopt an ``ood.KNNBank`` (fav_set_knn: copied to the device, the workspace allocated, the tap goes on), or None:
        off.  Refused on a deep ensemble, and for a bank whose D is not this arch's feature width."""
        if bank is None:
            _lib.check(self.lib.fav_set_knn(self._h, None), self._h)
        else:
            c = bank.to_c()
            _lib.check(self.lib.fav_set_knn(self._h, C.byref(c)), self._h)
        self._knn = bank

    def classify_knn(self, images, first_index: int = 0) -> dict:
        """frames -> ``label``, ``conf``, ``fail``, ``score`` as ``classify_detect`` gives them, plus the k-NN record of each
        frame (fav_classify_knn): ``kth_dist`` (squared distance of the normalised feature to its k-th nearest bank row),
        ``kth_sim``, ``nn_sim``, ``nn_row``, ``nn_class`` (the nearest row, its class or -1) and ``ood`` (not kth_dist <=
        threshold).  torch CUDA frames in -> CUDA tensors out, asynchronous on the current stream; numpy in -> numpy out,
        synchronous."""
        from .ood import KNN_RECORD_DWORDS, unpack_knn_records
        return self._classify_feature_head(self.lib.fav_classify_knn, KNN_RECORD_DWORDS, unpack_knn_records, images, first_index)

    def calibrate_knn(self, frames, tpr: float = 0.95) -> float:
        """Set the bank's threshold so that at least ``tpr`` of these in-distribution frames pass, and return it."""
        if self.knn_bank is None:
            raise ValueError("calibrate_knn needs a bank: set_knn first")
        from .ood import threshold_for_tpr
        thr = threshold_for_tpr(self._head_distances(self.classify_knn, "kth_dist", frames), tpr)
        self.set_knn(self.knn_bank.with_threshold(thr))
        return thr

    def knn_report(self, id_frames, ood_frames) -> dict:
        """How well kth_dist separates ``ood_frames`` from ``id_frames``: the keys of ``ood_report``."""
        if self.knn_bank is None:
            raise ValueError("knn_report needs a bank: set_knn first")
        from .ood import separation_report
        return separation_report(self._head_distances(self.classify_knn, "kth_dist", id_frames),
                                 self._head_distances(self.classify_knn, "kth_dist", ood_frames), self.knn_bank.threshold)

    # -- patch-level anomaly maps (patch.py PatchBank; include/fav.h fav_set_patch_bank) -------------------------------------
    @property
    def patch_bank(self):
        """The ``patch.PatchBank`` in force, None when off."""
        return self._patch

    def _patch_grid(self) -> tuple:
        """(Hf, Wf) of the map a patch bank is cut from, from the planner (refused on a ViT arch and on a deep ensemble)."""
        if self._map_hw is None:
            info = self.map_tap_info()
            self._map_hw = (info["hf"], info["wf"])
        return self._map_hw

    def _with_map_tap(self, run, stage=None):
        """``run()`` with the map tap on - with ``stage`` the stage tap at that stage; a tap that only this call needs goes
        off again, and a stage tap that stood at another stage goes back to it."""
        if stage is not None:
            was = self._stage_tap
            if was != stage:
                self.set_stage_tap(stage)
            try:
                return run()
            finally:
                if was != stage:
                    self.set_stage_tap(was)
        was_on = self._map_tap_on
        if not was_on:
            self.set_map_tap(True)
        try:
            return run()
        finally:
            if not was_on:
                self.set_map_tap(False)

    def _site_grid(self, stage) -> tuple:
        """(Hf, Wf) of the map a bank at ``stage`` is cut from (None: the last map)."""
        if stage is None:
            return self._patch_grid()
        info = self.stage_tap_info(stage)
        return (info["hf"], info["wf"])

    def fit_patch_bank(self, frames, stage=None, radius: int = 0, **kw):
        """Build a ``patch.PatchBank`` from in-distribution frames: batches of frames_per_call frames run through the
        classifier with the map tap on, every cell of every map goes through ``patch.cell_rows`` and all of them to
        ``patch.bank_from_rows`` (``max_rows``, ``seed``, ``threshold``, ``chunk_rows``, ``select``).  The subsample is random
        by default; ``select="coreset"`` picks the ``max_rows`` cells by greedy k-centre selection on this Backend's device
        (``coreset.select_coreset``) and ``bank.selection.radius`` is the coverage curve.  The handle is left as it was, the
        map tap included: see ``set_patch_bank``.  ``stage`` (1 .. 4; with ``radius`` 0 .. 2): the bank of a SITE - the cells
        of that residual stage's map through the stage tap, each replaced by ``patch.aggregate_cells`` of its neighbourhood
        before it is normalised; ``stage=None, radius=0`` is the plain bank of the last map."""
        from .patch import bank_from_rows, cell_rows
        if stage is None and int(radius) != 0:
            raise ValueError("a neighbourhood radius needs a stage (stage=4 is the last map)")
        grid = self._site_grid(stage)
        kw.setdefault("device", self.device)

        def run():
            parts = []
            for b, e in self._batches(int(frames.shape[0])):
                self.classify_detect(frames[b:e], b)
                parts.append(cell_rows(self.maps())[:2] if stage is None else cell_rows(self.stage_maps(), int(radius))[:2])
            return parts
        parts = self._with_map_tap(run, stage)
        if stage is not None:
            kw.update(stage=int(stage), radius=int(radius))
        return bank_from_rows(np.concatenate([p[0] for p in parts]), np.concatenate([p[1] for p in parts]), grid=grid, **kw)

    def set_patch_bank(self, bank):
        """Adopt a ``patch.PatchBank`` (fav_set_patch_bank: copied to the device, the workspace allocated for max_batch frames;
        the map tap is not touched), or None: off.  Refused on a ViT arch and on a deep ensemble, for a bank whose D is not
        the map's channel count, and for a bank cut from another grid than this configuration's map."""
        if bank is None:
            _lib.check(self.lib.fav_set_patch_bank(self._h, None), self._h)
        else:
            if bank.grid is not None:
                try:
                    grid = tuple(self._site_grid(bank.stage))
                except _lib.FavError:
                    grid = bank.grid               # no map here: the setter refuses the configuration in its own words
                if grid != tuple(bank.grid):
                    raise ValueError(f"the bank was cut from a {bank.grid} map, this configuration's is {grid}")
            c, site = bank.to_c(), bank.site_to_c()
            if site is None:
                _lib.check(self.lib.fav_set_patch_bank(self._h, C.byref(c)), self._h)
            else:
                _lib.check(self.lib.fav_set_patch_bank_at(self._h, C.byref(c), C.byref(site)), self._h)
        self._patch = bank

    def classify_patch(self, images, heatmap: bool = False, first_index: int = 0) -> dict:
        """frames -> ``label``, ``conf``, ``fail``, ``score`` as ``classify_detect`` gives them, plus the anomaly map of each
        frame (fav_classify_patch): ``dist`` fp32 [n, Hf, Wf], the squared distance of every cell's normalised feature to its
        nearest bank row (NaN for a cell without a direction), ``nn_row`` int32 [n, Hf, Wf], that row (-1 there), and the record
        fields of ``patch.unpack_patch_records``, each [n]: ``n_degenerate``, ``mean_dist``, ``peak`` (the frame's score),
        ``peak_cell``, ``floor``, ``peak_row``, ``n_above`` (cells at the bank's threshold or above), ``box`` and its ``x0``,
        ``y0``, ``x1``, ``y1``, ``anomalous``.  ``heatmap``: also ``heatmap`` uint8 [n, H, W], ``dist`` resized to the frame and
        normalised from its floor to its peak (fav_op_cam_heatmap).  The map tap goes on for the call if it is off, and off
        again.  torch CUDA frames in -> CUDA tensors out, asynchronous on the current stream; numpy in -> numpy out,
        synchronous.  Needs a bank; refused while views are set."""
        from .patch import PATCH_RECORD_DWORDS, unpack_patch_records
        torch = self._torch
        if self._patch is None:
            raise _lib.FavError(_lib.FAV_ERR_INVALID_ARG, "classify_patch: no patch bank set (set_patch_bank)")
        hw = self._site_grid(self._patch.stage)

        def run():
            img, host, n, layout, stream = self._classify_args(images)
            labels, conf, fail, score = self._detect_buffers(n, img.device)
            dist = torch.empty((n, *hw), dtype=torch.float32, device=img.device)
            row = torch.empty((n, *hw), dtype=torch.int32, device=img.device)
            rec = torch.empty((n, PATCH_RECORD_DWORDS), dtype=torch.int32, device=img.device)
            _lib.check(self.lib.fav_classify_patch(self._h, img.data_ptr(), n, layout, int(first_index), labels.data_ptr(), conf.data_ptr(),
                                                   fail.data_ptr(), score.data_ptr(), dist.data_ptr(), row.data_ptr(), rec.data_ptr(),
                                                   stream), self._h)
            out = dict(label=labels, conf=conf, fail=fail, score=score, dist=dist, nn_row=row)
            if heatmap:
                H, W = int(self.cfg.in_h), int(self.cfg.in_w)
                heat = torch.empty((n, H, W), dtype=torch.uint8, device=img.device)
                _lib.check(self.lib.fav_op_cam_heatmap(dist.data_ptr(), rec.data_ptr(), n, *hw, H, W, heat.data_ptr(), stream))
                out["heatmap"] = heat
            if host:
                out = {k: v.cpu().numpy() for k, v in out.items()}
                rec = rec.cpu().numpy()
            return dict(unpack_patch_records(rec), **out)
        return self._with_map_tap(run, self._patch.stage)

    def calibrate_patch(self, frames, tpr: float = 0.95) -> float:
        """Set the bank's threshold so that at least ``tpr`` of these in-distribution frames have no cell above it - the
        ceil(tpr * n)-th smallest ``peak``, raised by one float32 step, since a cell counts at equality - and return it."""
        if self.patch_bank is None:
            raise ValueError("calibrate_patch needs a bank: set_patch_bank first")
        from .ood import threshold_for_tpr
        peaks = self._patch_peaks(frames)
        thr = float(np.nextafter(np.float32(threshold_for_tpr(peaks, tpr)), np.float32(np.inf)))
        self.set_patch_bank(self.patch_bank.with_threshold(thr))
        return thr

    def patch_report(self, id_frames, ood_frames) -> dict:
        """How well ``peak`` separates ``ood_frames`` from ``id_frames``: the keys of ``ood_report``."""
        if self.patch_bank is None:
            raise ValueError("patch_report needs a bank: set_patch_bank first")
        from .ood import separation_report
        return separation_report(self._patch_peaks(id_frames), self._patch_peaks(ood_frames), self.patch_bank.threshold)

    def _patch_peaks(self, frames) -> np.ndarray:
        """``classify_patch`` over batches of frames_per_call frames -> every frame's ``peak``, the map tap staying on throughout."""
        return self._with_map_tap(lambda: self._head_distances(lambda f, b: self.classify_patch(f, first_index=b), "peak", frames),
                                  self._patch.stage)

    # -- window-level drift detection (ood.py DriftReference; include/fav.h fav_set_drift) -------------------------------
    @property
    def drift_reference(self):
        """The ``ood.DriftReference`` in force, None when off."""
        return self._drift

    def fit_drift(self, frames, **kw):
        """Build an ``ood.DriftReference`` from held-out in-distribution frames, as ``fit_knn`` builds a bank: the mean over
        the samples of each frame's tapped features goes to ``ood.build_drift_reference`` (``max_rows``, ``n_perm``,
        ``alpha``, ``seed``).  The handle is left as it was: see ``set_drift``."""
        from .ood import build_drift_reference
        return build_drift_reference(self._tapped_mean_features(frames), **kw)

    def set_drift(self, ref):
        """Adopt an ``ood.DriftReference`` (fav_set_drift: copied to the device, its own block of distances computed, the
        workspace allocated, the tap goes on), or None: off.  Refused on a deep ensemble, for a reference whose D is not this
        arch's feature width, and on a handle whose max_batch lies outside [2, 1024]."""
        if ref is None:
            _lib.check(self.lib.fav_set_drift(self._h, None), self._h)
        else:
            c = ref.to_c()
            _lib.check(self.lib.fav_set_drift(self._h, C.byref(c)), self._h)
        self._drift = ref

    def classify_drift(self, images, first_index: int = 0) -> dict:
        """frames -> ``label``, ``conf``, ``fail``, ``score`` as ``classify_detect`` gives them, plus ``record``: the one
        fav_drift_record of the call as int32[12] (``ood.unpack_drift_record`` reads it).  One call is one window: the
        permutation test is between the reference and exactly these frames, 2 to ``frames_per_call`` of them; more is a
        ValueError.  torch CUDA frames in -> CUDA tensors out, asynchronous on the current stream; numpy in -> numpy out,
        synchronous."""
        from .ood import DRIFT_RECORD_DWORDS
        n = int(images.shape[0])
        if n > self.frames_per_call:
            raise ValueError(f"classify_drift: a call is one window and takes at most frames_per_call={self.frames_per_call} "
                             f"frames, got {n}")
        img, host, n, layout, stream = self._classify_args(images)
        labels, conf, fail, score = self._detect_buffers(n, img.device)
        rec = self._torch.empty((DRIFT_RECORD_DWORDS,), dtype=self._torch.int32, device=img.device)
        _lib.check(self.lib.fav_classify_drift(self._h, img.data_ptr(), n, layout, int(first_index), labels.data_ptr(),
                                               conf.data_ptr(), fail.data_ptr(), score.data_ptr(), rec.data_ptr(), stream), self._h)
        if host:
            labels, conf, fail, score, rec = (t.cpu().numpy() for t in (labels, conf, fail, score, rec))
        return dict(record=rec, label=labels, conf=conf, fail=fail, score=score)

    def drift_report(self, id_frames, shifted_frames, window: int) -> dict:
        """Cut both sets into windows of ``window`` frames (a rest shorter than that is dropped), test each: ``id_p`` and
        ``shifted_p`` (the p-values), ``false_alarm_rate`` and ``detection_rate`` (the share of each set's windows with
        drift set, at the reference's alpha), ``alpha``, ``window``."""
        if self.drift_reference is None:
            raise ValueError("drift_report needs a reference: set_drift first")
        if not 2 <= window <= self.frames_per_call:
            raise ValueError(f"window must be in [2, frames_per_call={self.frames_per_call}], got {window}")
        from .ood import unpack_drift_record

        def run(frames):
            recs = [unpack_drift_record(self.classify_drift(frames[b:b + window], b)["record"])
                    for b in range(0, int(frames.shape[0]) - window + 1, window)]
            if not recs:
                raise ValueError(f"fewer than window={window} frames")
            return np.array([r["p_value"] for r in recs], np.float32), float(np.mean([r["drift"] for r in recs]))

        id_p, far = run(id_frames)
        sh_p, det = run(shifted_frames)
        return dict(id_p=id_p, shifted_p=sh_p, false_alarm_rate=far, detection_rate=det, alpha=self.drift_reference.alpha,
                    window=int(window))

    # -- profiling (bench.py roofline leg) ----------------------------------------
    def set_profiling(self, enable: bool):
        _lib.check(self.lib.fav_set_profiling(self._h, 1 if enable else 0), self._h)

    def get_profile(self, reset: bool = True) -> dict:
        p = _lib.FavProfile()
        _lib.check(self.lib.fav_get_profile(self._h, C.byref(p), 1 if reset else 0), self._h)
        return {name: dict(ms=p.ms[i], flops=p.flops[i], bytes=p.bytes[i], launches=p.launches[i])
                for i, name in enumerate(_lib.KERNEL_CLASS_NAMES)}

    def get_op_profile(self) -> list:
        """Per-op rows of the static schedule (call after get_profile)."""
        n = C.c_int32()
        _lib.check(self.lib.fav_get_op_profile(self._h, None, 0, C.byref(n)), self._h)
        arr = (_lib.FavOpProfile * n.value)()
        _lib.check(self.lib.fav_get_op_profile(self._h, arr, n.value, C.byref(n)), self._h)
        return [{f: getattr(r, f) for f, _ in _lib.FavOpProfile._fields_ if f != "reserved"} for r in arr]

    # -- the reference seam ----------------------------------------------------------
    #: what the seam reports when the GPU path itself fails (never 'VISION_OK': the trust engine must not recover
    #: reliability on a frame nobody looked at, trust_engine.py:179-190)
    FAILED_STATUS = "VISION_CORRUPTED"

    def analyze_frame(self, frame: np.ndarray, status_provider=None) -> dict:
        """ONE call at the seam (main.py:160): a uint8 HxWx3 frame -> the dict SignalAnalyzer.analyze_frame returns
        (signal_analyzer.py:128-143), with the SAME keys the caller reads (main.py:163-177: ``anomaly_score``,
        ``vision_status``, ``metrics['blur']``, ``metrics['brightness']``, ...).  ``vision_status`` and the
        ``metrics`` entries of the reference are the rule scorer's (computed on the GPU by the fused
        signal-statistics kernel, signal.py); ``anomaly_score`` is the classifier's clamp(1 - confidence), rounded
        to 6 places, always a number (main.py:169 rounds it); ``metrics['classifier']`` = {label, confidence, fail,
        samples} and ``metrics['rule_anomaly_score']`` carry the rest.

        The frame is uploaded once; both kernels are queued on one stream and the host synchronises once.
        ``status_provider(frame) -> str`` replaces the built-in rules (the reference's metric keys are then 0.0).

        Errors.  A frame of the wrong type, dtype or shape is a caller bug: TypeError / ValueError, as
        ``classify`` raises.  A failure of the GPU path (FavError, a HIP error surfacing through torch) does NOT
        read as a healthy frame: the result is ``vision_status = FAILED_STATUS``, ``anomaly_score = 1.0`` and
        ``metrics['error']`` - the engine then decays trust at its corrupted-frame rate (trust_engine.py:218-224) -
        and the rule scorer's previous-frame state is left as it was before the call."""
        torch = self._torch
        if not isinstance(frame, np.ndarray):
            raise TypeError(f"analyze_frame takes a numpy uint8 HxWx3 frame (video_source.py:144-148), got {type(frame).__name__}")
        if frame.dtype != np.uint8:
            raise TypeError(f"analyze_frame takes uint8 pixels, got {frame.dtype}")
        if frame.shape != (self.cfg.in_h, self.cfg.in_w, 3):
            raise ValueError(f"expected a frame of shape ({self.cfg.in_h}, {self.cfg.in_w}, 3), got {tuple(frame.shape)}")
        fr = np.ascontiguousarray(frame)
        ref_metrics = {"blur": 0.0, "brightness": 0.0, "freeze": 0.0, "entropy": 0.0, "raw": {}}
        rule_score = None
        rules, saved = None, None
        # the caller's callback runs OUTSIDE the guarded region: an exception in it is the caller's bug and propagates; only the
        # device path below fails closed
        status = status_provider(frame) if status_provider is not None else None
        try:
            if status_provider is not None:
                labels, conf, fail, score = self.classify_detect(fr[None])
                l0, c0, f0, s0 = int(labels[0]), float(conf[0]), bool(fail[0]), float(score[0])
            else:
                if self._rules is None:
                    from .signal import SignalAnalyzerHIP
                    self._rules = SignalAnalyzerHIP(self.device)
                rules, saved = self._rules, self._rules.save_state()
                dev = torch.from_numpy(fr[None]).to(f"cuda:{self.device}")
                stats_dev = rules.launch_stats(dev)
                labels, conf, fail, score = self.classify_detect(dev)
                packed = torch.stack([labels.to(torch.float32), conf, fail.to(torch.float32), score])   # [4, 1]
                host = torch.cat([stats_dev, packed.view(torch.uint8).flatten()]).cpu().numpy()          # the one sync
                nstat = stats_dev.numel()
                rule = rules.score_stats(rules.parse_stats(host[:nstat].tobytes(), 1))[0]
                status, ref_metrics, rule_score = rule["vision_status"], dict(rule["metrics"]), rule["anomaly_score"]
                vals = host[nstat:].view(np.float32)
                l0, c0, f0, s0 = int(vals[0]), float(vals[1]), bool(vals[2]), float(vals[3])
        except (_lib.FavError, RuntimeError) as e:       # the device path failed: fail closed (see the docstring)
            if rules is not None:
                rules.restore_state(saved)
            return {"anomaly_score": 1.0, "vision_status": self.FAILED_STATUS,
                    "metrics": dict(ref_metrics, error=f"{type(e).__name__}: {e}")}
        metrics = dict(ref_metrics)
        metrics["classifier"] = {"label": l0, "confidence": round(c0, 4), "fail": f0, "samples": self.T}
        if rule_score is not None:
            metrics["rule_anomaly_score"] = rule_score
        return {"anomaly_score": round(s0, 6), "vision_status": status, "metrics": metrics}


def unpack_uncertainty(records) -> dict:
    """int32[n, 18] fav_uncertainty records (torch tensor on any device, or numpy) -> dict of per-field views:
    ``label`` int32[n], ``confidence`` / ``mean_prob`` / ``prob_std`` / ``pred_entropy`` / ``expected_entropy`` /
    ``mutual_info`` / ``agreement`` fp32[n] (bit-cast), ``top_label`` int32[n, 5], ``top_prob`` fp32[n, 5].  Nothing is
    copied: the fields alias the record buffer."""
    if records.ndim != 2 or int(records.shape[1]) != UNCERTAINTY_DWORDS:
        raise ValueError(f"expected int32[n, {UNCERTAINTY_DWORDS}] records, got shape {tuple(records.shape)}")
    if isinstance(records, np.ndarray):
        if records.dtype != np.int32:
            raise TypeError(f"records must be int32, got {records.dtype}")
        f32 = np.float32
    else:
        import torch
        if records.dtype != torch.int32:
            raise TypeError(f"records must be int32, got {records.dtype}")
        f32 = torch.float32
    out = {"label": records[:, 0]}
    for i, name in enumerate(("confidence", "mean_prob", "prob_std", "pred_entropy", "expected_entropy", "mutual_info",
                              "agreement"), start=1):
        out[name] = records[:, i].view(f32)
    out["top_label"] = records[:, 8:13]
    out["top_prob"] = records[:, 13:18].view(f32)
    return out


def anomaly_score_from_confidence(conf):
    """score = clamp(1 - conf, 0, 1): same [0,1] range contract as signal_analyzer.py:121."""
    return np.clip(1.0 - np.asarray(conf, np.float32), 0.0, 1.0).astype(np.float32)
