"""CPU-side checks of the test-time-augmentation views: the properties of the numpy reference (tests/views_ref.py) that the
GPU file's bit-exact comparisons rest on, fav_check_views (host only), the fav_view layout (C vs ctypes), the presets of
failure_aware_vision_amd.views, and that the new entry points are bound."""
import ctypes as C
import os
import subprocess

import numpy as np
import pytest

import views_ref as R

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


@pytest.fixture(scope="module")
def lib():
    from failure_aware_vision_amd import _lib
    if not os.path.exists(_lib.LIB_PATH):
        import __graft_entry__ as g
        g.build()
    return _lib.load()


# ---- the reference's own properties --------------------------------------------------------------------------------------
@pytest.mark.parametrize("shape", ((1, 1), (1, 5), (3, 4), (7, 9), (8, 8)))
def test_identity_and_double_flip(shape):
    rng = np.random.default_rng(3)
    frames = rng.integers(0, 256, (2,) + shape + (3,), dtype=np.uint8)
    assert np.array_equal(R.apply_view(frames, R.V()), frames)
    for border in (R.REFLECT101, R.REPLICATE, R.ZERO):
        assert np.array_equal(R.apply_view(frames, R.V(border=border)), frames)
    once = R.apply_view(frames, R.V(flip_x=1))
    assert np.array_equal(once, frames[:, :, ::-1])
    assert np.array_equal(R.apply_view(once, R.V(flip_x=1)), frames)
    assert np.array_equal(R.apply_view(frames, R.V(flip_y=1)), frames[:, ::-1])


def test_d4_views_are_distinct_permutations():
    from failure_aware_vision_amd import views
    frame = R.asymmetric_frame(6, 6)
    outs = [R.apply_view(frame, v) for v in views.d4()]
    assert len(outs) == 8
    pixels = sorted(map(tuple, frame.reshape(-1, 3)))
    assert len(set(pixels)) == 36
    for i, a in enumerate(outs):
        assert sorted(map(tuple, a.reshape(-1, 3))) == pixels, i                 # a permutation of the pixels
        for b in outs[:i]:
            assert not np.array_equal(a, b)
    # the group itself: identity, the three other turns and the four mirror images, as numpy spells them
    want = [frame, frame[:, :, ::-1], frame[:, ::-1], frame[:, ::-1, ::-1]]
    t = frame.transpose(0, 2, 1, 3)
    want += [t, t[:, :, ::-1], t[:, ::-1], t[:, ::-1, ::-1]]
    for w in want:
        assert any(np.array_equal(w, o) for o in outs)


def test_transpose_follows_the_flips():
    """Steps 3 and 4 in the contract's order: out[y][x] = in[fx(x)][fy(y)]."""
    frame = R.asymmetric_frame(5, 5)
    got = R.apply_view(frame, R.V(flip_x=1, transpose=1))
    S = 5
    for y in range(S):
        for x in range(S):
            assert np.array_equal(got[0, y, x], frame[0, S - 1 - x, y])
    with pytest.raises(ValueError):
        R.apply_view(R.asymmetric_frame(4, 5), R.V(transpose=1))


def test_reflect101_beyond_one_period():
    n = 4                                             # period 6: 0 1 2 3 2 1 | 0 1 2 3 2 1
    want = [0, 1, 2, 3, 2, 1]
    for i in range(-25, 26):
        assert R.border_index(i, n, R.REFLECT101) == (want[i % 6], True), i
    assert all(R.border_index(i, 1, R.REFLECT101) == (0, True) for i in (-7, 0, 9))
    frame = R.asymmetric_frame(4, 4)
    for d in (2 * 3 + 1, -(2 * 3 + 1), 9, -13):       # beyond 2(n-1)
        got = R.apply_view(frame, R.V(dx=d))
        for x in range(4):
            assert np.array_equal(got[0, :, x], frame[0, :, want[(x - d) % 6]])
    assert np.array_equal(R.apply_view(frame, R.V(dx=6, dy=-6)), frame)          # a whole period is the identity


def test_replicate_and_zero_borders():
    frame = R.asymmetric_frame(3, 5).astype(np.uint8) | 1                       # no pixel is all zero
    for dy, dx in ((0, 0), (1, 0), (0, -2), (2, 3), (-3, 1), (0, 5), (7, -9)):
        got = R.apply_view(frame, R.V(dy=dy, dx=dx, border=R.ZERO))
        rows = max(0, 3 - abs(dy))
        cols = max(0, 5 - abs(dx))
        zero = (got == 0).all(axis=-1)
        assert int(zero.sum()) == 15 - rows * cols, (dy, dx)                     # the zero border counts
        rep = R.apply_view(frame, R.V(dy=dy, dx=dx, border=R.REPLICATE))
        assert not (rep == 0).all(axis=-1).any()
        for y in range(3):
            for x in range(5):
                assert np.array_equal(rep[0, y, x], frame[0, min(max(y - dy, 0), 2), min(max(x - dx, 0), 4)])
    f32 = np.array([[[[np.nan, -0.0, 1.0]]]], np.float32)
    out = R.apply_view(f32, R.V(dx=1, border=R.ZERO))
    assert out.view(np.uint32).tolist() == [[[[0, 0, 0]]]]                        # +0.0f, not -0.0f


# ---- fav_check_views --------------------------------------------------------------------------------------------------
def check(lib, views, H, W):
    from failure_aware_vision_amd import _lib
    arr = (_lib.FavView * max(1, len(views)))(*[_lib.FavView(v["flip_x"], v["flip_y"], v["transpose"], v["dy"], v["dx"], v["border"])
                                                for v in views])
    err = C.create_string_buffer(256)
    st = lib.fav_check_views(arr, len(views), H, W, err, len(err))
    return st, err.value.decode()


def test_check_views_accepts_the_presets(lib):
    from failure_aware_vision_amd import views
    for name, vs, hw in (("identity", views.identity(), (7, 9)), ("hflip", views.hflip(), (7, 9)), ("d4", views.d4(), (8, 8)),
                         ("shifts", views.shifts(2), (7, 9)), ("shifts zero", views.shifts(65535, "zero"), (1, 1)),
                         ("shifts replicate", views.shifts(1, "replicate"), (3, 4)),
                         ("product", views.product(views.d4(), views.shifts(1)), (32, 32)),
                         ("64 views", views.product(views.d4(), views.d4()), (5, 5))):
        views.check(vs, *hw)                                                       # raises when refused
        assert check(lib, [R.as_dict(v) for v in vs], *hw) == (0, ""), name
    assert len(views.d4()) == 8 and len(views.shifts(3)) == 5 and len(views.product(views.d4(), views.shifts(1))) == 40
    assert views.shifts(2)[0] == views.View() and {(v.dy, v.dx) for v in views.shifts(2)} == {(0, 0), (-2, 0), (2, 0), (0, -2), (0, 2)}
    assert views.View.from_c(views.View(True, False, True, -3, 4, "zero").to_c()) == views.View(True, False, True, -3, 4, "zero")
    with pytest.raises(ValueError):
        views.View(border="wrap").to_c()


REFUSED = [("flip_x 2", [R.V(flip_x=2)], "flip_x"), ("flip_y -1", [R.V(flip_y=-1)], "flip_y"),
           ("transpose 3", [R.V(), R.V(transpose=3)], "view 1: transpose=3"),
           ("dy 65536", [R.V(dy=65536)], "dy=65536"), ("dy -65536", [R.V(dy=-65536)], "dy=-65536"),
           ("dx 65536", [R.V(dx=65536)], "dx=65536"), ("dx -65536", [R.V(dx=-65536)], "dx=-65536"),
           ("border 3", [R.V(border=3)], "border=3"), ("border -1", [R.V(border=-1)], "border=-1"),
           ("no views", [], "n_views=0"), ("65 views", [R.V()] * 65, "n_views=65")]


@pytest.mark.parametrize("why,views,text", REFUSED, ids=[r[0] for r in REFUSED])
def test_check_views_refuses(lib, why, views, text):
    st, msg = check(lib, views, 8, 8)
    assert st == 1 and text in msg, (why, msg)


def test_check_views_edges(lib):
    from failure_aware_vision_amd import _lib
    assert check(lib, [R.V(dy=65535, dx=-65535)], 8, 8) == (0, "")
    st, msg = check(lib, [R.V(), R.V(transpose=1)], 24, 32)
    assert st == 1 and "transpose needs H == W" in msg and "24x32" in msg
    assert check(lib, [R.V(transpose=1)], 32, 32) == (0, "")
    st, msg = check(lib, [R.V()], 0, 8)
    assert st == 1 and "H and W" in msg
    err = C.create_string_buffer(64)
    assert lib.fav_check_views(None, 1, 8, 8, err, len(err)) == 1 and b"NULL" in err.value
    one = (_lib.FavView * 1)(_lib.FavView(2, 0, 0, 0, 0, 0))
    assert lib.fav_check_views(one, 1, 8, 8, None, 0) == 1                        # the message is optional
    messages = {check(lib, v, 8, 8)[1] for _, v, _ in REFUSED} | {msg}
    assert len(messages) == len(REFUSED) + 1                                       # each refusal has its own message


# ---- the interface -----------------------------------------------------------------------------------------------------
_LAYOUT_C = r"""
#include <stddef.h>
#include <stdio.h>
#include "fav.h"
int main(void) {
    printf("size %zu\n", sizeof(fav_view));
#define F(x) printf("v.%s %zu\n", #x, offsetof(fav_view, x));
    F(flip_x) F(flip_y) F(transpose) F(dy) F(dx) F(border)
    printf("borders %d %d %d\n", (int)FAV_BORDER_REFLECT101, (int)FAV_BORDER_REPLICATE, (int)FAV_BORDER_ZERO);
    printf("max %d\n", (int)FAV_MAX_VIEWS);
    printf("abi %d\n", (int)FAV_ABI_VERSION);
    return 0;
}
"""


def test_layout_symbols_and_abi(lib, tmp_path):
    from failure_aware_vision_amd import _lib, views
    src = tmp_path / "layout.c"
    src.write_text(_LAYOUT_C)
    exe = str(tmp_path / "layout")
    subprocess.check_call(["gcc", "-std=c99", "-Wall", "-Werror", "-I" + os.path.join(ROOT, "include"), str(src), "-o", exe])
    out = {ln.split()[0]: ln.split()[1:] for ln in subprocess.check_output([exe], text=True).splitlines()}
    assert int(out["size"][0]) == 24 == C.sizeof(_lib.FavView)
    for name in ("flip_x", "flip_y", "transpose", "dy", "dx", "border"):
        assert int(out["v." + name][0]) == getattr(_lib.FavView, name).offset, name
    assert [int(v) for v in out["borders"]] == [0, 1, 2] == [_lib.BORDER_REFLECT101, _lib.BORDER_REPLICATE, _lib.BORDER_ZERO]
    assert views.BORDERS == R.BORDER_NAMES
    assert int(out["max"][0]) == 64 == _lib.MAX_VIEWS == views.MAX_VIEWS
    assert int(out["abi"][0]) == 2 == lib.fav_abi_version()                        # the ABI version does not change
    header = open(os.path.join(ROOT, "include", "fav.h")).read()
    for sym in ("fav_set_views", "fav_get_views", "fav_set_conf_kind", "fav_check_views", "fav_op_views"):
        assert sym in _lib._SIGNATURES and hasattr(lib, sym) and sym + "(" in header, sym
        assert getattr(lib, sym).argtypes == _lib._SIGNATURES[sym][1]
    assert C.sizeof(_lib.FavConfig) == 120 and C.sizeof(_lib.FavProfile) == 192  # fav_config and fav_profile do not change


def test_setters_refuse_a_null_handle(lib):
    from failure_aware_vision_amd import _lib
    one = (_lib.FavView * 1)(_lib.FavView())
    n = C.c_int32(-1)
    assert lib.fav_set_views(None, one, 1) == 1
    assert lib.fav_get_views(None, one, 1, C.byref(n)) == 1 and n.value == -1
    assert lib.fav_set_conf_kind(None, 0) == 1
