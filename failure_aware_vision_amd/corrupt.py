"""On-device corruption generator, the host mirror of the reference's
``VisionSimulator`` controls (platform/backend/vision_simulator.py:12-60): ``set_mode``
(normal / frozen / blank / corrupted), ``set_noise``, ``set_brightness``, ``get_vision_status``,
plus ``apply(frames)`` which actually produces the corrupted frames on the GPU
(``fav_op_corrupt``) — what the browser canvas does in the reference (app.js:782-857) — and
``gaussian(frames, severity)`` for ImageNet-C style noise.  Deterministic in (seed, frame index);
the generator keeps the low 32 bits of the frame index, so frame 2**32 + k repeats frame k.

``imagenet_c(frames, kind, severity)`` is the ImageNet-C style family (``fav_op_corrupt_c``):
the eight ``CORRUPTIONS`` kinds plus ``"gaussian_noise"`` (the Gaussian mode above), severities 1..5 from ``SEVERITY``.
"""
from __future__ import annotations

import ctypes as C
from collections.abc import Mapping

from . import _lib
from .synth import GAUSSIAN_NOISE_SIGMA

VALID_MODES = ("normal", "frozen", "blank", "corrupted")
#: the kinds ``Corruptor.imagenet_c`` takes: fav_corruption in enum order, then the Gaussian mode of fav_op_corrupt
CORRUPTIONS = _lib.CORRUPTION_KINDS + ("gaussian_noise",)


class _SeverityTable(Mapping):
    """``SEVERITY[kind][severity - 1] -> (a, b)``: the library's own table (fav_corruption_params), read on first use so
    that importing the package does not load the library; ``"gaussian_noise"``: (sigma, 0) of synth.GAUSSIAN_NOISE_SIGMA."""

    def __init__(self):
        self._table = None

    def _load(self):
        if self._table is None:
            lib = _lib.load()
            table = {}
            for k, name in enumerate(_lib.CORRUPTION_KINDS):
                rows = []
                for sev in range(1, 6):
                    a, b = C.c_float(), C.c_float()
                    _lib.check(lib.fav_corruption_params(k, sev, C.byref(a), C.byref(b)))
                    rows.append((a.value, b.value))
                table[name] = tuple(rows)
            table["gaussian_noise"] = tuple((float(s), 0.0) for s in GAUSSIAN_NOISE_SIGMA)
            self._table = table
        return self._table

    def __getitem__(self, kind):
        return self._load()[kind]

    def __iter__(self):
        return iter(CORRUPTIONS)

    def __len__(self):
        return len(CORRUPTIONS)


SEVERITY = _SeverityTable()

_STATUS = {"normal": "VISION_OK", "frozen": "VISION_FROZEN", "blank": "VISION_BLANK", "corrupted": "VISION_CORRUPTED"}


class Corruptor:
    def __init__(self, seed: int = 0, device: int | None = None):
        import torch
        self._torch = torch
        self.lib = _lib.load()
        if not torch.cuda.is_available():
            raise RuntimeError("Corruptor needs a gfx950 GPU; there is no CPU fallback")
        self.lib.fav_op_corrupt.restype = C.c_int
        self.lib.fav_op_corrupt.argtypes = [C.c_void_p, C.c_void_p, C.c_int32, C.c_int32, C.c_int32, C.c_int32, C.c_float,
                                            C.c_float, C.c_float, C.c_uint64, C.c_int64, C.c_void_p]
        self.seed = int(seed)
        self.reset()

    def reset(self):
        self.mode, self.noise_level, self.brightness = "normal", 0.0, 0.5
        self._last = None          # last frame shown (what "frozen" repeats)
        self._frame_index = 0

    def set_mode(self, mode: str):
        if mode in VALID_MODES:
            self.mode = mode

    def set_noise(self, level: float):
        self.noise_level = max(0.0, min(1.0, float(level)))

    def set_brightness(self, level: float):
        self.brightness = max(0.0, min(1.0, float(level)))

    def get_vision_status(self) -> str:
        return _STATUS[self.mode]

    def _run(self, frames, mode, out_dtype, sigma=0.0, first_index=None):
        torch = self._torch
        frames = frames.contiguous()
        n, H, W, _ = frames.shape
        out = torch.empty(frames.shape, dtype=out_dtype, device=frames.device)
        idx = self._frame_index if first_index is None else int(first_index)
        stream = torch.cuda.current_stream(frames.device).cuda_stream
        _lib.check(self.lib.fav_op_corrupt(frames.data_ptr(), out.data_ptr(), n, H, W, mode, self.noise_level,
                                           self.brightness / 0.5, float(sigma), self.seed, idx, stream))
        return out

    def apply(self, frames):
        """uint8 CUDA frames [n, H, W, 3] of a stream -> the frames the current mode shows."""
        torch = self._torch
        n = int(frames.shape[0])
        if self.mode == "frozen" and self._last is not None:
            out = self._last.unsqueeze(0).expand(n, -1, -1, -1).contiguous()
        else:
            code = {"normal": 0, "frozen": 0, "blank": 1, "corrupted": 2}[self.mode]
            out = self._run(frames, code, torch.uint8)
        self._last = out[-1].clone()
        self._frame_index += n
        return out

    def gaussian(self, frames, severity: int, first_index: int = 0):
        """uint8 frames -> fp32 [0,1] frames with Gaussian noise of ImageNet-C severity 1..5."""
        return self._run(frames, 3, self._torch.float32, GAUSSIAN_NOISE_SIGMA[severity - 1], first_index)

    def imagenet_c(self, frames, kind: str, severity: int | None = None, *, a: float | None = None, b: float | None = None,
                   first_index: int = 0):
        """uint8 CUDA frames [n, H, W, 3] -> fp32 [0,1] CUDA frames under corruption ``kind`` (one of ``CORRUPTIONS``), at
        ``severity`` 1..5 (``SEVERITY[kind]``) or at explicit parameters ``a`` (and ``b``; a parameter left None comes from
        ``severity`` when that is given, else it is 0).  Frame i has global index first_index + i; the result is a pure
        function of (seed, global index), so shards of a set agree with the whole.  One launch on the current stream."""
        if kind not in CORRUPTIONS:
            raise ValueError(f"kind must be one of {CORRUPTIONS}, got {kind!r}")
        if severity is None and a is None:
            raise ValueError("give a severity (1..5) or the parameter a")
        if severity is not None and not 1 <= int(severity) <= 5:
            raise ValueError(f"severity must be in 1..5, got {severity}")
        ta, tb = SEVERITY[kind][int(severity) - 1] if severity is not None else (0.0, 0.0)
        a = ta if a is None else float(a)
        b = tb if b is None else float(b)
        torch = self._torch
        if kind == "gaussian_noise":
            return self._run(frames, 3, torch.float32, a, first_index)
        if frames.dtype != torch.uint8 or frames.ndim != 4 or frames.shape[3] != 3 or not frames.is_cuda:
            raise ValueError("imagenet_c takes uint8 CUDA frames [n, H, W, 3]")
        frames = frames.contiguous()
        n, H, W, _ = frames.shape
        out = torch.empty(frames.shape, dtype=torch.float32, device=frames.device)
        d = _lib.FavCorruptionDesc(C.sizeof(_lib.FavCorruptionDesc), _lib.CORRUPTION_KINDS.index(kind), a, b, self.seed,
                                   int(first_index))
        stream = torch.cuda.current_stream(frames.device).cuda_stream
        _lib.check(self.lib.fav_op_corrupt_c(frames.data_ptr(), out.data_ptr(), n, H, W, C.byref(d), stream))
        return out
