"""The autoencoder anomaly sensor (include/fav.h fav_ae_*).

The reference's design has one learned model: an unsupervised convolutional autoencoder, "Conv2d -> ReLU -> ConvTranspose2d",
trained on normal frames only, whose ``anomaly_score = MSE(recon, frame)`` is the signal the trust engine integrates
(docs/system_notes.md 6.1).  ``Autoencoder`` is that sensor: it needs no classifier checkpoint, works at the platform's own
frame size and says where the frame is wrong, a cell at a time.

Scoring runs in the HIP library.  PyTorch is the plumbing: ``torch_module`` is the model as an ``nn.Module``, ``fit`` trains
it with Adam on whatever torch device is at hand, ``blob_from_state_dict`` converts the result to the device layouts.  The
model is indifferent to the order of the three channels as long as training and scoring agree (the reference hands BGR).
"""
from __future__ import annotations

import ctypes as C
import struct

import numpy as np

from . import _lib

AE_RECORD_DWORDS = 8
_FIELDS = ("sse_lo", "mse", "peak", "peak_cell", "floor", "sse_hi", "n_above", "box")
_FLOAT_DWORDS = (1, 2, 4)
BLOB_MAGIC = 0x41564146   # "FAVA" little endian
BLOB_HEADER = 64
MAX_LEVELS = 3


def width(level: int) -> int:
    """C_l = 64 * 2^(l-1), l = 1 .. 3."""
    return 64 << (level - 1)


def _check_levels(levels: int) -> int:
    if int(levels) != levels or not 1 <= levels <= MAX_LEVELS:
        raise ValueError(f"levels must be 1 .. {MAX_LEVELS}, got {levels}")
    return int(levels)


def _bf16_bits(x) -> np.ndarray:
    x = np.ascontiguousarray(x, np.float32)
    u = x.view(np.uint32).astype(np.uint64)
    return ((u + 0x7FFF + ((u >> 16) & 1)) >> 16).astype(np.uint16)


def _bf16_to_f32(bits) -> np.ndarray:
    return (np.asarray(bits, np.uint16).astype(np.uint32) << 16).view(np.float32)


def _np(t) -> np.ndarray:
    return np.asarray(t.detach().cpu().numpy() if hasattr(t, "detach") else t, np.float32)


# ---- the model -----------------------------------------------------------------------------------------------------
def torch_module(levels: int = 2):
    """The model as an ``nn.Module`` on [n, 3, H, W] pixels in [0, 1]: ``enc[l-1]`` is enc_l, ``dec[0]`` dec_L and ``dec[-1]``
    dec_1; the output is cropped to the input's H x W."""
    import torch
    from torch import nn

    levels = _check_levels(levels)

    class ConvAutoencoder(nn.Module):
        def __init__(self):
            super().__init__()
            self.enc = nn.ModuleList([nn.Conv2d(3 if l == 1 else width(l - 1), width(l), 3, stride=2, padding=1)
                                      for l in range(1, levels + 1)])
            self.dec = nn.ModuleList([nn.ConvTranspose2d(width(l), 3 if l == 1 else width(l - 1), 2, stride=2)
                                      for l in range(levels, 0, -1)])

        def forward(self, x):
            h, w = x.shape[-2:]
            for e in self.enc:
                x = torch.relu(e(x))
            for d in self.dec[:-1]:
                x = torch.relu(d(x))
            return torch.sigmoid(self.dec[-1](x))[..., :h, :w]

    return ConvAutoencoder()


def layer_shapes(levels: int) -> list:
    """[(weight shape, bias length)] in the blob's order: enc_1 .. enc_L, dec_L .. dec_2, dec_1, device layouts."""
    levels = _check_levels(levels)
    out = [((64, 64), 64)]
    out += [((width(l), 3, 3, width(l - 1)), width(l)) for l in range(2, levels + 1)]
    out += [((4 * width(l - 1), width(l)), 4 * width(l - 1)) for l in range(levels, 1, -1)]
    return out + [((12, 64), 3)]


def device_layers(sd, levels: int) -> list:
    """A ``torch_module(levels)`` state dict (torch tensors or numpy) -> [(bf16 bits in the device layout, fp32 bias)] in the
    blob's order.  A 2x2 / stride-2 transposed convolution is a 1x1 GEMM to four times the channels: row (2a + b) C + co of
    the weight holds wt[:, co, a, b] and the bias is tiled four times."""
    levels = _check_levels(levels)
    layers = []
    w = _np(sd["enc.0.weight"])                                           # [64, 3, 3, 3] = [co, c, r, s]
    if w.shape != (64, 3, 3, 3):
        raise ValueError(f"enc.0.weight has shape {w.shape}, expected (64, 3, 3, 3)")
    w1 = np.zeros((64, 64), np.float32)
    w1[:, :27] = w.transpose(0, 2, 3, 1).reshape(64, 27)                  # k = (r 3 + s) 3 + c
    layers.append((_bf16_bits(w1), _np(sd["enc.0.bias"]).copy()))
    for l in range(2, levels + 1):
        w = _np(sd[f"enc.{l - 1}.weight"])                                # [C_l, C_{l-1}, 3, 3]
        if w.shape != (width(l), width(l - 1), 3, 3):
            raise ValueError(f"enc.{l - 1}.weight has shape {w.shape}")
        layers.append((_bf16_bits(w.transpose(0, 2, 3, 1)), _np(sd[f"enc.{l - 1}.bias"]).copy()))
    for j, l in enumerate(range(levels, 0, -1)):
        wt = _np(sd[f"dec.{j}.weight"])                                   # [C_l, C_out, 2, 2] = [ci, co, a, b]
        cout = 3 if l == 1 else width(l - 1)
        if wt.shape != (width(l), cout, 2, 2):
            raise ValueError(f"dec.{j}.weight has shape {wt.shape}")
        wg = wt.transpose(2, 3, 1, 0).reshape(4 * cout, width(l))         # row (2a + b) cout + co
        b = _np(sd[f"dec.{j}.bias"])
        layers.append((_bf16_bits(wg), b.copy() if l == 1 else np.tile(b, 4)))
    for (bits, b), (ws, bl) in zip(layers, layer_shapes(levels)):
        assert bits.shape == ws and b.shape == (bl,)
    return layers


def _align(n: int) -> int:
    return (n + 63) // 64 * 64


def pack_blob(layers, levels: int) -> bytes:
    """[(bf16 bits, fp32 bias)] in the blob's order -> a FAVA v1 blob (fav.h, beside fav_ae_check_blob)."""
    levels = _check_levels(levels)
    if len(layers) != 2 * levels:
        raise ValueError(f"{levels} levels have {2 * levels} layers, got {len(layers)}")
    at = _align(BLOB_HEADER + 16 * len(layers))
    table, chunks = [], []
    for bits, bias in layers:
        wb = np.ascontiguousarray(bits, np.uint16).tobytes()
        bb = np.ascontiguousarray(bias, np.float32).tobytes()
        table.append((at, at + _align(len(wb))))
        chunks += [wb.ljust(_align(len(wb)), b"\0"), bb.ljust(_align(len(bb)), b"\0")]
        at += _align(len(wb)) + _align(len(bb))
    head = struct.pack("<4IQ", BLOB_MAGIC, 1, levels, len(layers), at).ljust(BLOB_HEADER, b"\0")
    head += b"".join(struct.pack("<2Q", *t) for t in table)
    return head.ljust(_align(len(head)), b"\0") + b"".join(chunks)


def blob_from_state_dict(sd, levels: int) -> bytes:
    """A ``torch_module(levels)`` state dict -> the blob ``Autoencoder`` loads; the weights are rounded to bf16."""
    return pack_blob(device_layers(sd, levels), levels)


def parse_blob(blob: bytes) -> tuple:
    """A FAVA blob -> (levels, [(weights fp32 holding the bf16 values, device layout; fp32 bias)])."""
    magic, version, levels, nl, total = struct.unpack_from("<4IQ", blob, 0)
    if magic != BLOB_MAGIC or version != 1 or not 1 <= levels <= MAX_LEVELS or nl != 2 * levels or total != len(blob):
        raise ValueError("not a FAVA v1 blob")
    layers = []
    for k, (ws, bl) in enumerate(layer_shapes(levels)):
        w_off, b_off = struct.unpack_from("<2Q", blob, BLOB_HEADER + 16 * k)
        w = _bf16_to_f32(np.frombuffer(blob, np.uint16, int(np.prod(ws)), w_off)).reshape(ws)
        layers.append((w.copy(), np.frombuffer(blob, np.float32, bl, b_off).copy()))
    return levels, layers


def make_synthetic_state_dict(levels: int = 2, seed: int = 1) -> dict:
    """He-normal weights rounded to bf16 and small random biases, as numpy arrays under ``torch_module``'s names."""
    levels = _check_levels(levels)
    rng = np.random.default_rng([int(seed), levels, 0xAE])
    sd = {}

    def he(shape, fan_in):
        return _bf16_to_f32(_bf16_bits(rng.standard_normal(shape) * np.sqrt(2.0 / fan_in))).reshape(shape)
    for l in range(1, levels + 1):
        cin = 3 if l == 1 else width(l - 1)
        sd[f"enc.{l - 1}.weight"] = he((width(l), cin, 3, 3), 9 * cin)
        sd[f"enc.{l - 1}.bias"] = rng.uniform(-0.05, 0.05, width(l)).astype(np.float32)
    for j, l in enumerate(range(levels, 0, -1)):
        cout = 3 if l == 1 else width(l - 1)
        sd[f"dec.{j}.weight"] = he((width(l), cout, 2, 2), width(l))
        sd[f"dec.{j}.bias"] = rng.uniform(-0.05, 0.05, cout).astype(np.float32)
    return sd


def make_synthetic_ae(levels: int = 2, seed: int = 1) -> bytes:
    """The blob of ``make_synthetic_state_dict``: a checkpoint for parity tests (it has learned nothing)."""
    return blob_from_state_dict(make_synthetic_state_dict(levels, seed), levels)


def train_state_dict(frames_u8, levels: int = 2, steps: int = 300, lr: float = 1e-3, seed: int = 0, batch: int = 32, device=None) -> dict:
    """Train ``torch_module(levels)`` on uint8 [n, H, W, 3] normal frames: Adam on the mean squared error of [0, 1] pixels,
    ``steps`` batches drawn with ``seed``.  -> the state dict (CPU tensors)."""
    import torch
    frames_u8 = np.ascontiguousarray(frames_u8)
    if frames_u8.ndim != 4 or frames_u8.shape[3] != 3 or frames_u8.dtype != np.uint8 or frames_u8.shape[0] < 1:
        raise ValueError("fit takes uint8 frames of shape (n, H, W, 3)")
    dev = torch.device(device if device is not None else ("cuda" if torch.cuda.is_available() else "cpu"))
    gen = torch.Generator().manual_seed(int(seed))
    state = torch.random.get_rng_state()
    torch.manual_seed(int(seed))
    try:
        net = torch_module(levels).to(dev)
    finally:
        torch.random.set_rng_state(state)
    x = torch.from_numpy(frames_u8).to(dev).permute(0, 3, 1, 2).float() / 255.0
    opt = torch.optim.Adam(net.parameters(), lr=lr)
    for _ in range(int(steps)):
        idx = torch.randint(0, x.shape[0], (min(int(batch), x.shape[0]),), generator=gen).to(dev)
        xb = x[idx]
        loss = torch.mean((net(xb) - xb) ** 2)
        opt.zero_grad()
        loss.backward()
        opt.step()
    return {k: v.detach().cpu() for k, v in net.state_dict().items()}


# ---- records -------------------------------------------------------------------------------------------------------
def unpack_ae_records(records) -> dict:
    """int32[..., 8] fav_ae_record records (torch tensor or numpy) -> ``mse``, ``peak``, ``floor`` fp32, ``peak_cell``,
    ``n_above``, ``box`` int32 (packed; -1: none), ``sse_lo``, ``sse_hi`` int32, each [...] and a view of the record buffer,
    plus ``sse`` int64 (the frame's integer sum), the box unpacked to ``x0``, ``y0``, ``x1``, ``y1`` (inclusive cells; all -1
    when the box is -1) and ``anomalous`` = n_above > 0."""
    if records.ndim < 1 or int(records.shape[-1]) != AE_RECORD_DWORDS:
        raise ValueError(f"expected int32[..., {AE_RECORD_DWORDS}] records, got shape {tuple(records.shape)}")
    if isinstance(records, np.ndarray):
        if records.dtype != np.int32:
            raise TypeError(f"records must be int32, got {records.dtype}")
        f32, where = np.float32, np.where
        wide = lambda a: a.astype(np.int64)   # noqa: E731
    else:
        import torch
        if records.dtype != torch.int32:
            raise TypeError(f"records must be int32, got {records.dtype}")
        f32, where = torch.float32, torch.where
        wide = lambda a: a.to(torch.int64)    # noqa: E731
    out = {name: records[..., j].view(f32) if j in _FLOAT_DWORDS else records[..., j] for j, name in enumerate(_FIELDS)}
    out["sse"] = (wide(out["sse_lo"]) & 0xFFFFFFFF) | ((wide(out["sse_hi"]) & 0xFFFFFFFF) << 32)
    box = out["box"]
    none = box == -1
    for name, shift in (("x0", 0), ("y0", 8), ("x1", 16), ("y1", 24)):
        out[name] = where(none, box, (box >> shift) & 0xFF)
    out["anomalous"] = out["n_above"] > 0
    return out


def geometry(in_hw=(240, 320), levels: int = 2, cell: int = 16, max_batch: int = 32) -> dict:
    """fav_ae_info (host only): ``h``, ``w`` (levels + 1 grid sides each), ``gh``, ``gw``, ``workspace_bytes``.  A config the
    library refuses raises FavError with its message, which names the field."""
    cfg = _lib.FavAeConfig(C.sizeof(_lib.FavAeConfig), int(in_hw[0]), int(in_hw[1]), int(levels), int(max_batch), int(cell))
    h, w = (C.c_int32 * 4)(), (C.c_int32 * 4)()
    gh, gw, ws = C.c_int32(), C.c_int32(), C.c_size_t()
    err = C.create_string_buffer(256)
    st = _lib.load().fav_ae_info(C.byref(cfg), h, w, C.byref(gh), C.byref(gw), C.byref(ws), err, len(err))
    if st != _lib.FAV_OK:
        raise _lib.FavError(st, err.value.decode("utf-8", "replace"))
    n = int(levels) + 1
    return dict(h=list(h)[:n], w=list(w)[:n], gh=gh.value, gw=gw.value, workspace_bytes=ws.value)


def check_blob(blob: bytes) -> str:
    """fav_ae_check_blob (host only): '' for a blob the library accepts, else its message."""
    err = C.create_string_buffer(256)
    st = _lib.load().fav_ae_check_blob(blob, len(blob), err, len(err))
    return "" if st == _lib.FAV_OK else (err.value.decode("utf-8", "replace") or "refused")


def seam_result(status: str, ref_metrics: dict, rule_score, mse: float, peak: float, peak_cell: int) -> dict:
    """The dict of the reference's seam (signal_analyzer.py:128-143) with the sensor's score in it:
    ``anomaly_score = round(min(mse, 1), 6)`` and ``metrics['autoencoder'] = {mse, peak, peak_cell}``."""
    metrics = dict(ref_metrics)
    metrics["autoencoder"] = {"mse": float(mse), "peak": float(peak), "peak_cell": int(peak_cell)}
    if rule_score is not None:
        metrics["rule_anomaly_score"] = rule_score
    return {"anomaly_score": round(min(float(mse), 1.0), 6), "vision_status": status, "metrics": metrics}


class Autoencoder:
    """The sensor on one GPU.  ``blob``: a FAVA blob (``blob_from_state_dict``, ``fit``); None: ``make_synthetic_ae(levels,
    seed_weights)``, which has learned nothing.  There is no CPU fallback."""

    #: what the seam reports when the GPU path itself fails, as Backend.FAILED_STATUS
    FAILED_STATUS = "VISION_CORRUPTED"

    def __init__(self, blob: bytes | None = None, *, in_hw=(240, 320), levels: int = 2, cell: int = 16, max_batch: int = 32,
                 seed_weights: int = 1, device: int | None = None):
        import torch
        self._torch = torch
        self._h = None
        self.lib = _lib.load()
        self.levels = _check_levels(levels)
        self.in_hw = (int(in_hw[0]), int(in_hw[1]))
        self.cell, self.max_batch = int(cell), int(max_batch)
        geo = geometry(self.in_hw, self.levels, self.cell, self.max_batch)       # refuses a bad config without a device
        self.grid = (geo["gh"], geo["gw"])
        self.geometry = geo
        if not torch.cuda.is_available():
            raise RuntimeError("Autoencoder needs a gfx950 GPU; there is no CPU fallback")
        self.device = torch.cuda.current_device() if device is None else int(device)
        self.threshold = float("inf")
        self._rules = None
        cfg = _lib.FavAeConfig(C.sizeof(_lib.FavAeConfig), self.in_hw[0], self.in_hw[1], self.levels, self.max_batch, self.cell)
        h = C.c_void_p()
        with torch.cuda.device(self.device):
            _lib.check(self.lib.fav_ae_create(C.byref(cfg), C.byref(h)))
        self._h = h
        self.load(blob if blob is not None else make_synthetic_ae(self.levels, seed_weights))

    def load(self, blob: bytes):
        """Load a FAVA blob (fav_ae_load_weights); a refused blob leaves the weights in force."""
        _lib.check(self.lib.fav_ae_load_weights(self._h, blob, len(blob)))
        self.blob = bytes(blob)

    def close(self):
        if self._h is not None:
            self.lib.fav_ae_destroy(self._h)
            self._h = None

    def __del__(self):
        try:
            self.close()
        except Exception:
            pass

    def reset(self):
        """Clear the rule scorer's previous-frame state, as Backend.reset."""
        if self._rules is not None:
            self._rules.reset()

    def set_threshold(self, thr: float):
        """The cell threshold: a cell with err_map >= thr counts in ``n_above`` and ``box``."""
        _lib.check(self.lib.fav_ae_set_threshold(self._h, float(thr)))
        self.threshold = float(thr)

    # -- scoring ------------------------------------------------------------------
    def _frames(self, frames):
        torch = self._torch
        if frames.ndim != 4 or tuple(frames.shape[1:]) != (*self.in_hw, 3):
            raise ValueError(f"expected frames of shape (n, {self.in_hw[0]}, {self.in_hw[1]}, 3), got {tuple(frames.shape)}")
        if frames.dtype in (torch.uint8, np.uint8):
            layout = _lib.LAYOUT_NHWC_U8
        elif frames.dtype in (torch.float32, np.float32):
            layout = _lib.LAYOUT_NHWC_F32
        else:
            raise TypeError(f"frames must be uint8 or float32 NHWC, got {frames.dtype}")
        if isinstance(frames, np.ndarray):
            return torch.from_numpy(np.ascontiguousarray(frames)).to(f"cuda:{self.device}"), True, layout
        if not frames.is_cuda or frames.device.index != self.device:
            raise ValueError(f"frames must live on cuda:{self.device}")
        return frames.contiguous(), False, layout

    def score(self, frames, recon: bool = False) -> dict:
        """frames uint8 or fp32 [n, H, W, 3] -> ``mse`` fp32 [n] (the reference's anomaly_score on [0, 1] pixels), ``err_map``
        fp32 [n, gh, gw], ``peak``, ``peak_cell``, ``floor``, ``n_above``, ``box`` (and ``x0`` .. ``y1``, ``anomalous``),
        ``sse`` int64 [n], and with ``recon`` the reconstruction uint8 [n, H, W, 3].  Any n: the call runs ``max_batch`` frames
        at a time.  torch CUDA frames in -> CUDA tensors out, asynchronous on the current stream; numpy in -> numpy out."""
        torch = self._torch
        img, host, layout = self._frames(frames)
        n = int(img.shape[0])
        gh, gw = self.grid
        err_map = torch.empty((n, gh, gw), dtype=torch.float32, device=img.device)
        rec = torch.empty((n, AE_RECORD_DWORDS), dtype=torch.int32, device=img.device)
        rc = torch.empty((n, *self.in_hw, 3), dtype=torch.uint8, device=img.device) if recon else None
        stream = torch.cuda.current_stream(img.device).cuda_stream
        for b in range(0, n, self.max_batch):
            e = min(n, b + self.max_batch)
            _lib.check(self.lib.fav_ae_score(self._h, img[b:e].data_ptr(), e - b, layout, err_map[b:e].data_ptr(), rec[b:e].data_ptr(),
                                             rc[b:e].data_ptr() if recon else None, stream))
        out = dict(err_map=err_map)
        if recon:
            out["recon"] = rc
        if host:
            out = {k: v.cpu().numpy() for k, v in out.items()}
            rec = rec.cpu().numpy()
        return dict(unpack_ae_records(rec), **out)

    def calibrate(self, frames, tpr: float = 0.95) -> float:
        """Set the cell threshold so that at least ``tpr`` of these normal frames have no cell above it - the ceil(tpr * n)-th
        smallest ``peak``, raised by one float32 step, since a cell counts at equality - and return it."""
        from .ood import threshold_for_tpr
        peaks = self.score(frames)["peak"]
        peaks = np.asarray(peaks if isinstance(peaks, np.ndarray) else peaks.cpu().numpy(), np.float32)
        thr = float(np.nextafter(np.float32(threshold_for_tpr(peaks, tpr)), np.float32(np.inf)))
        self.set_threshold(thr)
        return thr

    def fit(self, frames_u8, steps: int = 300, lr: float = 1e-3, seed: int = 0, batch: int = 32) -> dict:
        """Train ``torch_module(levels)`` on these normal frames (``train_state_dict``) and load the converted weights.
        -> the state dict."""
        frames_u8 = np.asarray(frames_u8.cpu() if hasattr(frames_u8, "cpu") else frames_u8)
        if tuple(frames_u8.shape[1:]) != (*self.in_hw, 3):
            raise ValueError(f"expected frames of shape (n, {self.in_hw[0]}, {self.in_hw[1]}, 3), got {tuple(frames_u8.shape)}")
        sd = train_state_dict(frames_u8, self.levels, steps, lr, seed, batch)
        self.load(blob_from_state_dict(sd, self.levels))
        return sd

    # -- the reference seam -----------------------------------------------------------
    def _score_one(self, fr: np.ndarray, use_rules: bool):
        """One uint8 frame -> (mse, peak, peak_cell, the rule scorer's dict or None): one upload, one stream, one sync."""
        torch = self._torch
        dev = torch.from_numpy(fr[None]).to(f"cuda:{self.device}")
        stats_dev = None
        if use_rules:
            if self._rules is None:
                from .signal import SignalAnalyzerHIP
                self._rules = SignalAnalyzerHIP(self.device)
            stats_dev = self._rules.launch_stats(dev)
        out = self.score(dev)
        packed = torch.stack([out["mse"], out["peak"], out["peak_cell"].view(torch.float32)]).view(torch.uint8).flatten()
        host = (torch.cat([stats_dev, packed]) if use_rules else packed).cpu().numpy()
        nstat = stats_dev.numel() if use_rules else 0
        rule = self._rules.score_stats(self._rules.parse_stats(host[:nstat].tobytes(), 1))[0] if use_rules else None
        vals = host[nstat:].copy()
        return float(vals.view(np.float32)[0]), float(vals.view(np.float32)[1]), int(vals.view(np.int32)[2]), rule

    def analyze_frame(self, frame: np.ndarray, status_provider=None) -> dict:
        """ONE call at the reference's seam (main.py:160), the dict shape of ``Backend.analyze_frame``: ``vision_status`` and
        the reference's metric keys from the rule scorer (``SignalAnalyzerHIP``; ``status_provider(frame) -> str`` replaces
        it), ``anomaly_score = round(min(mse, 1), 6)``, ``metrics['autoencoder'] = {mse, peak, peak_cell}``.  This is the
        reference's live loop: rules plus the learned score.  A failure of the GPU path fails closed, as there:
        ``vision_status = FAILED_STATUS``, ``anomaly_score = 1.0``, ``metrics['error']``."""
        if not isinstance(frame, np.ndarray):
            raise TypeError(f"analyze_frame takes a numpy uint8 HxWx3 frame, got {type(frame).__name__}")
        if frame.dtype != np.uint8:
            raise TypeError(f"analyze_frame takes uint8 pixels, got {frame.dtype}")
        if frame.shape != (*self.in_hw, 3):
            raise ValueError(f"expected a frame of shape ({self.in_hw[0]}, {self.in_hw[1]}, 3), got {tuple(frame.shape)}")
        fr = np.ascontiguousarray(frame)
        ref_metrics = {"blur": 0.0, "brightness": 0.0, "freeze": 0.0, "entropy": 0.0, "raw": {}}
        status = status_provider(frame) if status_provider is not None else None
        rules = self._rules
        saved = rules.save_state() if rules is not None else None
        rule_score = None
        try:
            mse, peak, peak_cell, rule = self._score_one(fr, status_provider is None)
            if rule is not None:
                status, ref_metrics, rule_score = rule["vision_status"], dict(rule["metrics"]), rule["anomaly_score"]
        except (_lib.FavError, RuntimeError) as e:       # the device path failed: fail closed
            if rules is not None:
                rules.restore_state(saved)
            return {"anomaly_score": 1.0, "vision_status": self.FAILED_STATUS,
                    "metrics": dict(ref_metrics, error=f"{type(e).__name__}: {e}")}
        return seam_result(status, ref_metrics, rule_score, mse, peak, peak_cell)
