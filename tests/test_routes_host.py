"""Host side of the route report (fav_op_last_route, fav.h): the argument checks of fav_op_conv2d and
fav_op_bottleneck_tail - a refusal returns before anything touches the runtime, so these run without a device - and
the list of routes the production build can take, each of which some GPU case must expect by name."""
import ctypes as C

import pytest

from failure_aware_vision_amd import _lib

INVALID_ARG = 1


@pytest.fixture(scope="module")
def lib():
    return _lib.load()


@pytest.fixture(scope="module")
def ptr():
    """An address that is not NULL; a refused descriptor's pointers are never read."""
    buf = C.create_string_buffer(64)
    yield C.addressof(buf)
    del buf


def conv_desc(ptr, **kw):
    a = dict(n_frames=1, H=8, W=8, Cin=64, Cout=64, kh=3, kw=3, stride=1, pad=1, relu=1, out_f32=0, math_mode=0)
    a.update(kw)
    return _lib.FavConvDesc(ptr, ptr, ptr, None, ptr, a["n_frames"], a["H"], a["W"], a["Cin"], a["Cout"], a["kh"], a["kw"],
                            a["stride"], a["pad"], a["relu"], a["out_f32"], a["math_mode"], _lib.FavDropoutDesc(-1, 0, 1.0, 0, 0, 1, 0))


def last_error(lib):
    return lib.fav_last_error(None).decode()


SIZES = "conv: n_frames, H and W must be >= 1"
WINDOW = "conv: kh, kw and stride must be >= 1 and pad >= 0"
FIT = "conv: the window does not fit the padded frame"
COUT = "conv: Cout must be >= 1 and the padded Cout must cover it"
CONV_REFUSALS = [
    (dict(n_frames=0), SIZES), (dict(n_frames=-3), SIZES), (dict(H=0), SIZES), (dict(W=0), SIZES), (dict(H=-8), SIZES),
    (dict(kh=0), WINDOW), (dict(kw=0), WINDOW), (dict(kh=-3), WINDOW),
    (dict(stride=0), WINDOW),                        # divides by zero in conv_out
    (dict(stride=-1), WINDOW),
    (dict(pad=-1), WINDOW),
    (dict(H=1, W=1, pad=0), FIT),                    # conv_out truncates towards zero: Ho = Wo = -1, M = n_frames > 0
    (dict(H=2, W=8, pad=0), FIT), (dict(H=8, W=2, pad=0), FIT),
    (dict(H=1, W=8, kh=7, kw=1, pad=2), FIT),        # H + 2 pad = 5 < 7
    (dict(relu=-1), "conv: relu must be 0 (none), 1 (ReLU) or 2 (GELU)"), (dict(relu=3), "conv: relu must be 0 (none), 1 (ReLU) or 2 (GELU)"),
    (dict(out_f32=2), "conv: out_f32 must be 0 or 1"), (dict(out_f32=-1), "conv: out_f32 must be 0 or 1"),
    (dict(math_mode=2), "conv: unknown math_mode"), (dict(math_mode=-1), "conv: unknown math_mode"),
    (dict(Cin=0), "conv: Cin must be a multiple of 64 and >= 64"), (dict(Cin=-64), "conv: Cin must be a multiple of 64 and >= 64"),
    (dict(Cout=0), COUT),                            # tiles_n = 0: an empty grid
    (dict(Cout=-64), COUT),                          # tiles_n = -1: a grid of (unsigned)-1
]


@pytest.mark.parametrize("change,message", CONV_REFUSALS, ids=[",".join(f"{k}={v}" for k, v in ch.items()) for ch, _ in CONV_REFUSALS])
def test_conv_refuses_before_any_launch(lib, ptr, change, message):
    d = conv_desc(ptr, **change)
    assert lib.fav_op_conv2d(C.byref(d), None) == INVALID_ARG
    assert last_error(lib) == "fav_op_conv2d: " + message
    assert _lib.last_route() == ""


@pytest.mark.parametrize("change", [dict(n_frames=0), dict(n_frames=-1), dict(H=0), dict(W=0), dict(H=-56), dict(W=-1)],
                         ids=lambda ch: ",".join(f"{k}={v}" for k, v in ch.items()))
def test_tail_refuses_empty_shapes_before_any_launch(lib, ptr, change):
    a = dict(n_frames=2, H=8, W=8)
    a.update(change)
    d = _lib.FavTailDesc(ptr, ptr, ptr, ptr, ptr, ptr, ptr, None, None, None, a["n_frames"], a["H"], a["W"], 64, 0,
                         _lib.FavDropoutDesc(-1, 0, 1.0, 0, 0, 1, 0), 0, 0)
    assert lib.fav_op_bottleneck_tail(C.byref(d), None) == INVALID_ARG
    assert last_error(lib) == "fav_op_bottleneck_tail: bottleneck tail: n_frames, H and W must be >= 1"
    assert _lib.last_route() == ""


def test_last_route_checks_its_buffer(lib):
    assert lib.fav_op_last_route(None, 64) == INVALID_ARG
    assert last_error(lib) == "fav_op_last_route: null or empty buffer"
    buf = C.create_string_buffer(b"x" * 7, 8)
    assert lib.fav_op_conv2d(None, None) == INVALID_ARG and last_error(lib) == "fav_op_conv2d: null pointer"
    assert lib.fav_op_last_route(buf, 0) == INVALID_ARG
    assert last_error(lib) == "fav_op_last_route: null or empty buffer"          # its own message, not the earlier call's
    assert lib.fav_op_last_route(buf, 8) == 0 and buf.value == b""      # nothing launched on this thread: empty


# Every route name the production build can produce through fav_op_*, read off the launchers of csrc/fav.hip:
#  launch_conv   128-row tiles: BN 64 | 128 (Cout % 128), BK 32 with a three-stage or 64 with a two-stage ring (conv_bk), the
#                staged epilogue exactly with a residual, two math modes, with / without the GELU: 32 names.
#                256 x 256 tile (conv_big): always the register epilogue; the ping-pong loop exactly in the production mode.
#                staged-patch 3x3: Cin = Cout 64 | 128, 256-pixel tiles, two math modes.
#  launch_proj   256 -> 512 on 4 waves, 512 -> 1024 on 8.
#  launch_tail   the FAV_TAIL arms; one or two Wc buffers as tail_geometry's LDS budget decides: the single buffer is
#                reached only by 64/64 (W 116..147), 64/128 (W 52..83) and 128/128 (W 56..87) with the 3x3.
#  attention, entry reduce, fused stem.
# Not reachable through the op ABI ("Routes"): the ViT tile rule (needs a handle) and grouped launches.
REACHABLE_ROUTES = (
    [f"conv_igemm<128,{bn},{bk},{3 if bk == 32 else 2},{mode},epi{epi}{gelu}>"
     for bn in (64, 128) for bk in (32, 64) for mode in ("bf16", "f32") for epi in (0, 1) for gelu in ("", ",gelu")] +
    ["conv_igemm<256,256,64,2,bf16,epi1,pp>", "conv_igemm<256,256,64,2,bf16,epi1,pp,gelu>",
     "conv_igemm<256,256,64,2,f32,epi1>", "conv_igemm<256,256,64,2,f32,epi1,gelu>",
     "conv3x3_halo<64,64,256,3,bf16>", "conv3x3_halo<64,64,256,3,f32>", "conv3x3_halo<128,128,256,2,bf16>", "conv3x3_halo<128,128,256,2,f32>",
     "proj<256,512,nw4>", "proj<512,1024,nw8>",
     "tail<64,0,3x3,nw4,wc2>", "tail<64,64,3x3,nw4,wc2>", "tail<64,64,3x3,nw4,wc1>", "tail<64,128,3x3,nw4,wc2>", "tail<64,128,3x3,nw4,wc1>",
     "tail<64,0,1x1,nw4,wc2>", "tail<64,64,1x1,nw4,wc2>", "tail<64,128,1x1,nw4,wc2>",
     "tail<128,0,3x3,nw8,wc2>", "tail<128,128,3x3,nw8,wc2>", "tail<128,128,3x3,nw8,wc1>", "tail<128,0,1x1,nw8,wc2>", "tail<128,128,1x1,nw8,wc2>",
     "tail<256,0,3x3,nw8,wc2>", "tail<256,0,1x1,nw4,wc2>", "tail<256,256,1x1,nw8,wc2,rp16>", "tail<512,0,1x1,nw8,wc2>",
     "tail<64,64,3x3,nw4,wc2,res_entry>", "tail<64,64,3x3,nw4,wc1,res_entry>",
     "attention<bf16,13,full>", "attention<bf16,13>", "attention<bf16,16>", "attention<f32,13>", "attention<f32,16>",
     "entry_reduce<256,64>", "stem7_pool<u8>", "stem7_pool<f32>"])


def expected_routes():
    """The routes the GPU suite's tables expect (their modules need torch; nothing else in this file does)."""
    pytest.importorskip("torch")
    import test_gpu_conv_routes
    import test_gpu_exact
    import test_gpu_ops
    import test_gpu_tail
    import test_gpu_vit_f64
    routes = {c.route for c in test_gpu_conv_routes.CASES}
    routes |= {case[-1] for case in test_gpu_tail.CASES} | {case[-1] for case in test_gpu_tail.RES_ENTRY_CASES}
    routes |= {test_gpu_tail.WIDE_PROJ_ROUTE, test_gpu_ops.ENTRY_REDUCE_ROUTE} | set(test_gpu_exact.STEM_POOL_ROUTES)
    routes |= {test_gpu_vit_f64.attention_route(T, mode) for T, _ in test_gpu_vit_f64.ATTENTION_CASES for mode in (0, 1)}
    return routes


def test_every_reachable_route_is_expected_by_a_gpu_case():
    assert len(set(REACHABLE_ROUTES)) == len(REACHABLE_ROUTES) == 69
    expected = expected_routes()
    missing = [r for r in REACHABLE_ROUTES if r not in expected]
    assert not missing, f"no GPU case expects {missing}"
    unknown = sorted(expected - set(REACHABLE_ROUTES))
    assert not unknown, f"a GPU case expects a route the list does not hold: {unknown}"
