"""Test-time augmentation views (include/fav.h ``fav_view``): label-preserving copies of a
frame - mirror images, quarter turns, small shifts - whose softmax outputs the heads average like MC-Dropout samples or
ensemble members, so that ``mutual_info``, ``agreement`` and ``prob_std`` carry information on any checkpoint.

A ``View`` mirrors ``fav_view``: for output pixel (y, x), (u, v) = (y - dy, x - dx), the border rule, the flips, the swap of
``transpose`` (square frames only), then ``out[y][x] = in[u][v]``.  ``Backend(views=...)`` / ``Backend.set_views`` turn them
on for every classify method; ``apply(frames, views)`` makes the view frames themselves (``fav_op_views``).
"""
from __future__ import annotations

import ctypes as C
import dataclasses

from . import _lib

BORDERS = ("reflect101", "replicate", "zero")
MAX_VIEWS = _lib.MAX_VIEWS


@dataclasses.dataclass(frozen=True)
class View:
    flip_x: bool = False
    flip_y: bool = False
    transpose: bool = False
    dy: int = 0
    dx: int = 0
    border: str = "reflect101"

    def to_c(self) -> "_lib.FavView":
        if self.border not in BORDERS:
            raise ValueError(f"border must be one of {BORDERS}, got {self.border!r}")
        return _lib.FavView(int(bool(self.flip_x)), int(bool(self.flip_y)), int(bool(self.transpose)), int(self.dy), int(self.dx),
                            BORDERS.index(self.border))

    @staticmethod
    def from_c(v) -> "View":
        return View(bool(v.flip_x), bool(v.flip_y), bool(v.transpose), int(v.dy), int(v.dx), BORDERS[v.border])


def to_c_array(views):
    """A sequence of ``View`` -> (ctypes array of fav_view, count)."""
    views = list(views)
    return (_lib.FavView * max(1, len(views)))(*[v.to_c() for v in views]), len(views)


def identity():
    return [View()]


def hflip():
    """The frame and its mirror image."""
    return [View(), View(flip_x=True)]


def d4():
    """The eight symmetries of the square: the four quarter turns and their mirror images (square frames only)."""
    return [View(flip_x=fx, flip_y=fy, transpose=t) for t in (False, True) for fy in (False, True) for fx in (False, True)]


def shifts(k: int, border: str = "reflect101"):
    """The frame and its four shifts by ``k`` pixels along the axes."""
    k = int(k)
    return [View(border=border)] + [View(dy=dy, dx=dx, border=border) for dy, dx in ((-k, 0), (k, 0), (0, -k), (0, k))]


def product(a, b):
    """Every view of ``a`` combined with every view of ``b`` (``a`` outer): the flags are combined with exclusive or and the
    shifts added, as one fav_view applies them (shift, then flips, then transpose) - it is a pairing of the two presets'
    parameters, not the composition of the two maps.  The border is ``b``'s where ``b`` shifts, else ``a``'s."""
    out = []
    for va in a:
        for vb in b:
            out.append(View(va.flip_x ^ vb.flip_x, va.flip_y ^ vb.flip_y, va.transpose ^ vb.transpose, va.dy + vb.dy,
                            va.dx + vb.dx, vb.border if (vb.dy or vb.dx) else va.border))
    return out


def check(views, H: int, W: int):
    """fav_check_views: raises ``FavError`` with the library's message when ``views`` are not valid for H x W frames."""
    arr, n = to_c_array(views)
    err = C.create_string_buffer(256)
    st = _lib.load().fav_check_views(arr, n, int(H), int(W), err, len(err))
    if st != _lib.FAV_OK:
        raise _lib.FavError(st, err.value.decode("utf-8", "replace"))


def apply(frames, views):
    """CUDA frames [n, H, W, 3] (uint8 or float32) -> their views [len(views), n, H, W, 3], view a of frame i at [a, i]
    (``fav_op_views``: at most two launches on the current stream, no host round trip)."""
    import torch
    if not frames.is_cuda or frames.ndim != 4 or frames.shape[3] != 3 or frames.dtype not in (torch.uint8, torch.float32):
        raise ValueError("apply takes uint8 or float32 CUDA frames [n, H, W, 3]")
    frames = frames.contiguous()
    n, H, W, _ = (int(x) for x in frames.shape)
    arr, count = to_c_array(views)
    out = torch.empty((count, n, H, W, 3), dtype=frames.dtype, device=frames.device)
    layout = _lib.LAYOUT_NHWC_U8 if frames.dtype == torch.uint8 else _lib.LAYOUT_NHWC_F32
    stream = torch.cuda.current_stream(frames.device).cuda_stream
    _lib.check(_lib.load().fav_op_views(frames.data_ptr(), out.data_ptr(), n, H, W, layout, arr, count, stream))
    return out
