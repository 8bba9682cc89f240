"""Host side of the route report (fav_op_last_route, fav.h) and of the selector behind it (csrc/fav_route.hpp, asked through
fav_route_*): the argument checks of fav_op_conv2d and fav_op_bottleneck_tail - a refusal returns before anything touches
the runtime, so these run without a device; the list of routes the production build can take, which a sweep of the selector
must produce exactly and each of which some GPU case must expect by name; the route every GPU case expects, asked of the
selector here; and the rules no fav_op_* reaches - the ViT encoder's tiles and the thresholds of a grouped launch."""
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


NO_DROP = (-1, 0, 1.0, 0, 0, 1, 0)


def conv_desc(ptr, res=False, **kw):
    a = dict(n_frames=1, H=8, W=8, Cin=64, Cout=64, kh=3, kw=3, stride=1, pad=1, relu=1, out_f32=0, math_mode=0)
    a.update(kw)
    return _lib.FavConvDesc(ptr, ptr, ptr, ptr if res else None, ptr, a["n_frames"], a["H"], a["W"], a["Cin"], a["Cout"], a["kh"], a["kw"],
                            a["stride"], a["pad"], a["relu"], a["out_f32"], a["math_mode"], _lib.FavDropoutDesc(*NO_DROP))


def tail_desc(ptr, n, H, W, cmid, nred, has3x3, drop=NO_DROP, res_entry=0, entry_site=0):
    wb, wa = (ptr if has3x3 else None), (ptr if nred else None)
    return _lib.FavTailDesc(ptr, wb, wb, ptr, ptr, ptr, ptr, wa, wa, wa, n, H, W, cmid, nred, _lib.FavDropoutDesc(*drop), res_entry, entry_site)


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


@pytest.mark.parametrize("change,message", CONV_REFUSALS, ids=[",".join(f"{k}={v}" for k, v in ch.items()) for ch, _ in CONV_REFUSALS])
def test_conv_query_refuses_with_the_same_text(lib, ptr, change, message):
    assert _lib.route_conv2d(conv_desc(ptr, **change)) == (INVALID_ARG, message)
    assert _lib.last_route() == ""


TAIL_EMPTY = [dict(n_frames=0), dict(n_frames=-1), dict(H=0), dict(W=0), dict(H=-56), dict(W=-1)]


@pytest.mark.parametrize("change", TAIL_EMPTY, ids=lambda ch: ",".join(f"{k}={v}" for k, v in ch.items()))
def test_tail_query_refuses_with_the_same_text(lib, ptr, change):
    a = dict(n_frames=2, H=8, W=8)
    a.update(change)
    assert _lib.route_bottleneck_tail(tail_desc(ptr, a["n_frames"], a["H"], a["W"], 64, 0, True)) == \
        (INVALID_ARG, "bottleneck tail: n_frames, H and W must be >= 1")
    assert _lib.last_route() == ""


def test_queries_apply_the_gates_of_the_ops(lib, ptr):
    """NULL pointers and Cout % 64, as fav_op_conv2d and fav_op_bottleneck_tail refuse them, before the selector is asked."""
    assert lib.fav_route_conv2d(None, 0, 1, C.create_string_buffer(96), 96) == INVALID_ARG
    d = conv_desc(ptr)
    d.bias = None
    assert _lib.route_conv2d(d) == (INVALID_ARG, "null pointer")
    assert lib.fav_op_conv2d(C.byref(d), None) == INVALID_ARG and last_error(lib) == "fav_op_conv2d: null pointer"
    assert _lib.route_conv2d(conv_desc(ptr, Cout=100)) == (INVALID_ARG, "Cout must be a multiple of 64")
    assert _lib.route_conv2d(conv_desc(ptr), groups=0) == (INVALID_ARG, "groups must be >= 1")
    t = tail_desc(ptr, 2, 8, 8, 64, 64, True)
    t.t1n = None                                     # wa without its output
    assert _lib.route_bottleneck_tail(t) == (INVALID_ARG, "null pointer")
    assert lib.fav_op_bottleneck_tail(C.byref(t), None) == INVALID_ARG and last_error(lib) == "fav_op_bottleneck_tail: null pointer"
    assert _lib.route_bottleneck_tail(tail_desc(ptr, 2, 8, 8, 96, 0, False)) == (INVALID_ARG, "bottleneck tail: unsupported shape")
    assert _lib.route_attention(1, 257, 128, 2) == _lib.route_attention(1, 16, 100, 2) == \
        (INVALID_ARG, "attention: need 1 <= tokens <= 256 and 64-wide heads")
    d = conv_desc(ptr)
    small = C.create_string_buffer(b"x" * 7, 8)      # a buffer the name does not fit: refused, nothing written
    assert lib.fav_route_conv2d(C.byref(d), 0, 1, small, 8) == INVALID_ARG and small.value == b"x" * 7
    assert _lib.last_route() == ""


@pytest.mark.parametrize("change", TAIL_EMPTY, ids=lambda ch: ",".join(f"{k}={v}" for k, v in ch.items()))
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


# Every route name the production build can produce through fav_op_*.  The list is checked against the selector
# (csrc/fav_route.hpp): test_the_selector_reaches_exactly_the_listed_routes sweeps fav_route_* over a grid of descriptors
# and must find these names and no other; the last three belong to launchers with one kernel family and no selector.
#  route_conv       128-row tiles: BN 64 | 128 (Cout % 128), BK 32 with a three-stage or 64 with a two-stage ring (conv_bk),
#                   the staged epilogue exactly with a residual, two math modes, with / without the GELU: 32 names.
#                   256 x 256 tile (conv_big): always the register epilogue; the ping-pong loop exactly in the production mode.
#                   staged-patch 3x3: Cin = Cout 64 | 128, 256-pixel tiles, two math modes.
#                   projection: 256 -> 512 on 4 waves, 512 -> 1024 on 8.
#  route_tail       one kernel per (Cmid, Nred, 3x3); one or two Wc buffers as tail_geometry's LDS budget decides: the single
#                   buffer is reached only by 64/64 (W 116..147), 64/128 (W 52..83) and 128/128 (W 56..87) with the 3x3.
#  route_attention  13 key tiles up to 208 tokens (unmasked at exactly 13 in the production mode), 16 above.
#  entry reduce, fused stem.
# The ViT tile rule and grouped launches take names of this list by rules of their own: pinned below, on the host.
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
NO_SELECTOR = {"entry_reduce<256,64>", "stem7_pool<u8>", "stem7_pool<f32>"}


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


def routed(answer):
    """The name of a served query; a served query leaves fav_op_last_route alone."""
    status, text = answer
    assert status == 0, text
    assert _lib.last_route() == ""
    return text


# n, H, W: one row; 143 rows; both sides of 2048 rows (staged-patch 3x3; turned, for its LDS fit at 128 channels), of 4096
# (projection), of 512 big tiles at Cout 2048 (16 384 rows) and at Cout 512 (65 536 rows); 131 072 rows and more (wide projection)
SWEEP_FRAMES = [(1, 1, 1), (1, 11, 13), (1, 21, 25), (1, 23, 89), (1, 89, 23), (1, 32, 64), (1, 64, 32), (1, 63, 65), (1, 64, 64),
                (1, 125, 129), (1, 127, 127), (1, 127, 129), (1, 128, 128), (240, 16, 17), (241, 16, 17), (672, 28, 28), (700, 14, 14)]
SWEEP_WIDTHS = [1, 7, 28, 51, 52, 55, 56, 83, 84, 87, 88, 115, 116, 147, 148, 300]


def test_the_selector_reaches_exactly_the_listed_routes(lib, ptr):
    """vit = 0, one member, this build's knobs, every required pointer non-NULL: what fav_op_* can reach."""
    found = set()
    for cin in (64, 128, 256, 512, 1024):
        for cout in (64, 128, 192, 256, 320, 512, 1024, 2048):
            for k, stride, pad in ((1, 1, 0), (1, 2, 0), (3, 1, 1), (3, 2, 1)):
                for res in (False, True):
                    for relu in (0, 1, 2):
                        for mode in (0, 1):
                            for n, H, W in SWEEP_FRAMES:
                                found.add(routed(_lib.route_conv2d(conv_desc(ptr, res=res, n_frames=n, H=H, W=W, Cin=cin, Cout=cout, kh=k, kw=k,
                                                                             stride=stride, pad=pad, relu=relu, math_mode=mode))))
    for cmid in (64, 128, 256, 512):
        for nred in (0, 64, 128, 256):
            for has3x3 in (False, True):
                for W in SWEEP_WIDTHS:
                    status, text = _lib.route_bottleneck_tail(tail_desc(ptr, 3, 7, W, cmid, nred, has3x3))
                    assert (status, text) == (INVALID_ARG, "bottleneck tail: unsupported shape") or status == 0, text
                    if status == 0:
                        found.add(text)
    for W in (56, 120):
        found.add(routed(_lib.route_bottleneck_tail(tail_desc(ptr, 6, 3, W, 64, 64, True, drop=(3, 26, 1.1, 0, 0, 2, 0), res_entry=1, entry_site=2))))
    for T in range(1, 257):
        for mode in (0, 1):
            found.add(routed(_lib.route_attention(2, T, 128, 2, mode)))
    assert _lib.last_route() == ""
    listed = set(REACHABLE_ROUTES) - NO_SELECTOR
    assert sorted(found - listed) == [], "the selector reaches routes the list lacks: add them, and a GPU case for each"
    assert sorted(listed - found) == [], "listed routes the selector never gives"


def test_the_selector_gives_the_route_every_gpu_case_expects(lib, ptr):
    """The descriptor of every case of the GPU route tables, asked of the selector without a device."""
    pytest.importorskip("torch")
    import test_gpu_conv_routes
    import test_gpu_tail
    import test_gpu_vit_f64
    for c in test_gpu_conv_routes.CASES:
        d = conv_desc(ptr, res=c.res, n_frames=c.n, H=c.H, W=c.W, Cin=c.cin, Cout=c.cout, kh=c.kh, kw=c.kw, stride=c.stride, pad=c.pad,
                      relu=c.relu, math_mode=c.mode)
        assert routed(_lib.route_conv2d(d)) == c.route, c.name
    for cmid, nred, has3x3, H, W, n, route in test_gpu_tail.CASES:
        for drop in (NO_DROP, (5, 26, 1.1, 0x1234567ABC, 3, n + 1, 40)):       # the test's two variants
            assert routed(_lib.route_bottleneck_tail(tail_desc(ptr, n, H, W, cmid, nred, has3x3, drop=drop))) == route
    for H, W, n_img, v0, n_out, route in test_gpu_tail.RES_ENTRY_CASES:
        d = tail_desc(ptr, n_out, H, W, 64, 64, True, drop=(3, 26, 1.1, 0x1234567ABC, v0, n_img, 40), res_entry=1, entry_site=2)
        assert routed(_lib.route_bottleneck_tail(d)) == route
    for stride, H, W, n in ((2, 28, 28, 672), (1, 14, 14, 700)):                # the wide projection's two shapes
        d = conv_desc(ptr, n_frames=n, H=H, W=W, Cin=512, Cout=1024, kh=1, kw=1, stride=stride, pad=0, relu=0)
        assert routed(_lib.route_conv2d(d)) == test_gpu_tail.WIDE_PROJ_ROUTE
        d.out_f32 = 1
        assert routed(_lib.route_conv2d(d)) == "conv_igemm<256,256,64,2,bf16,epi1,pp>"
    for T, heads in test_gpu_vit_f64.ATTENTION_CASES:
        for mode in (0, 1):
            assert routed(_lib.route_attention(7, T, heads * 64, heads, mode)) == test_gpu_vit_f64.attention_route(T, mode)


def gemm_desc(ptr, frames, rows, K, N, res=False, act=0, mode=0):
    """A GEMM of the ViT encoder as run_vit describes it: `rows` tokens per frame as a 1x1 convolution over rows x 1 frames."""
    return conv_desc(ptr, res=res, n_frames=frames, H=rows, W=1, Cin=K, Cout=N, kh=1, kw=1, stride=1, pad=0, relu=act, math_mode=mode)


BIG, BIG_GELU = "conv_igemm<256,256,64,2,bf16,epi1,pp>", "conv_igemm<256,256,64,2,bf16,epi1,pp,gelu>"
VIT_RULE = [
    # frames, rows per frame, K, N, residual, activation, the route as a GEMM of the encoder, the route as any other convolution
    # the 256 x 256 tile from 50 big tiles up, whatever M - 49 against 50 at one column tile, 48 against 51 at ViT-B's 768 columns
    (1, 12799, 768, 256, False, 0, "conv_igemm<128,128,32,3,bf16,epi1>", "conv_igemm<128,128,64,2,bf16,epi1>"),
    (1, 12800, 768, 256, False, 0, BIG, "conv_igemm<128,128,64,2,bf16,epi1>"),
    (22, 197, 768, 768, True, 0, "conv_igemm<128,128,32,3,bf16,epi0>", "conv_igemm<128,128,32,3,bf16,epi0>"),
    (23, 197, 768, 768, True, 0, BIG, "conv_igemm<128,128,32,3,bf16,epi0>"),
    (7, 197, 768, 3072, False, 2, BIG_GELU, "conv_igemm<128,128,64,2,bf16,epi1,gelu>"),     # 5 x 12 = 60 tiles of 1379 rows
    (64, 197, 256, 768, False, 0, "conv_igemm<128,128,32,3,bf16,epi1>", "conv_igemm<128,128,32,3,bf16,epi1>"),   # K = 256 stays on 128 rows at 147 tiles
    # below the threshold: 32-deep steps, even at K = 3072 where any other convolution takes 64-deep ones
    (6, 197, 3072, 768, True, 0, "conv_igemm<128,128,32,3,bf16,epi0>", "conv_igemm<128,128,64,2,bf16,epi0>"),
    (6, 197, 768, 2304, False, 0, "conv_igemm<128,128,32,3,bf16,epi1>", "conv_igemm<128,128,64,2,bf16,epi1>"),
    (23, 197, 768, 768, True, 0, "conv_igemm<256,256,64,2,f32,epi1>", "conv_igemm<128,128,32,3,f32,epi0>"),       # validation mode: no ping-pong
]


@pytest.mark.parametrize("case", VIT_RULE, ids=lambda c: f"{c[0]}x{c[1]}-k{c[2]}-n{c[3]}")
def test_vit_tile_rule(lib, ptr, case):
    """launch_conv's rule for the encoder's GEMMs (route_conv, vit): expected values read off the rule as the commit before
    the selector had it in launch_conv (h->vit), and equal in that commit's dump."""
    frames, rows, K, N, res, act, as_vit, as_conv = case
    mode = 1 if "f32" in as_vit else 0
    d = gemm_desc(ptr, frames, rows, K, N, res=res, act=act, mode=mode)
    assert routed(_lib.route_conv2d(d, vit=1)) == as_vit
    assert routed(_lib.route_conv2d(d, vit=0)) == as_conv


HALO64, GEN64 = "conv3x3_halo<64,64,256,3,bf16>", "conv_igemm<128,64,64,2,bf16,epi1>"
PROJ, GEN_PROJ = "proj<256,512,nw4>", "conv_igemm<128,128,32,3,bf16,epi1>"
EXPAND = "conv_igemm<128,128,32,3,bf16,epi0>"      # a 512-deep 1x1 with a residual on 128-row tiles
GROUPED = [
    # what, descriptor fields, {members: route}: the thresholds count rows x members
    ("halo-2048", dict(H=32, W=32), {1: GEN64, 2: HALO64}),                                  # 1024 rows
    ("halo-2048-below", dict(H=31, W=33), {1: GEN64, 2: GEN64, 5: HALO64}),                  # 1023 rows: 2046, 5115
    ("halo-2048-five", dict(H=409, W=1), {5: GEN64}),                                        # 5 x 409 = 2045
    ("halo-2048-five-above", dict(H=10, W=41), {5: HALO64}),                                 # 5 x 410 = 2050
    ("proj-4096", dict(H=32, W=64, Cin=256, Cout=512, kh=1, kw=1, pad=0, relu=0), {1: GEN_PROJ, 2: PROJ}),          # 2048 rows
    ("proj-4096-below", dict(H=23, W=89, Cin=256, Cout=512, kh=1, kw=1, pad=0, relu=0), {1: GEN_PROJ, 2: GEN_PROJ}),   # 2 x 2047
    ("proj-4096-five", dict(H=9, W=91, Cin=256, Cout=512, kh=1, kw=1, pad=0, relu=0), {5: GEN_PROJ}),               # 5 x 819 = 4095
    ("proj-4096-five-above", dict(H=20, W=41, Cin=256, Cout=512, kh=1, kw=1, pad=0, relu=0), {5: PROJ}),            # 5 x 820 = 4100
    # the 256 x 256 tile needs 8192 rows: at Cout 8192 (32 column tiles) the tile count is met long before
    ("big-min-rows", dict(res=True, H=64, W=64, Cin=512, Cout=8192, kh=1, kw=1, pad=0), {1: EXPAND, 2: BIG}),       # 4096 rows
    ("big-min-rows-below", dict(res=True, H=63, W=65, Cin=512, Cout=8192, kh=1, kw=1, pad=0), {1: EXPAND, 2: EXPAND, 5: BIG}),   # 2 x 4095 = 8190
    # ... and 512 big tiles: at Cout 2048 (8 column tiles) that is 16 384 rows
    ("big-tiles", dict(res=True, H=64, W=128, Cin=512, Cout=2048, kh=1, kw=1, pad=0), {1: EXPAND, 2: BIG}),         # 8192 rows
    ("big-tiles-below", dict(res=True, H=90, W=91, Cin=512, Cout=2048, kh=1, kw=1, pad=0), {1: EXPAND, 2: EXPAND}),  # 2 x 8190: 63 x 8 = 504
    ("big-tiles-five", dict(res=True, H=36, W=91, Cin=512, Cout=2048, kh=1, kw=1, pad=0), {5: EXPAND}),             # 5 x 3276 = 16 380
    ("big-tiles-five-above", dict(res=True, H=29, W=113, Cin=512, Cout=2048, kh=1, kw=1, pad=0), {5: BIG}),         # 5 x 3277 = 16 385
]


@pytest.mark.parametrize("name,fields,routes", GROUPED, ids=[g[0] for g in GROUPED])
def test_grouped_launch_thresholds_count_rows_times_members(lib, ptr, name, fields, routes):
    """A grouped launch (Group::n members in one launch) meets the staged-patch, projection and big-tile thresholds with its
    rows x members; expected values read off launch_conv / launch_proj / conv_big of the commit before the selector (M * G.n)."""
    for members, route in routes.items():
        assert routed(_lib.route_conv2d(conv_desc(ptr, **fields), groups=members)) == route, members
