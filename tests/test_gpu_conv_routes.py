"""Every kernel instantiation fav_op_conv2d can launch in the production build, pinned by name.

launch_conv picks among the 128-row implicit-GEMM tiles (BN 64 / 128 x BK 32 / 64 x staged / register epilogue x two math
modes x with / without the GELU), the 256 x 256 tile, the staged-patch 3x3 and the row-owning projection by shape
thresholds.  One table: each case is a descriptor, the route it must take (fav_op_last_route, fav.h) and the oracle it must
equal bit for bit - O.conv_acc_exact(mode="mfma") for math_mode 0, the f32 chain for math_mode 1, then O.epilogue or
O.gelu_exact.  Every case asserts the route, the bits, and that the guard regions in front of and behind the output are
untouched.  Shapes are the smallest that reach the route; thresholds are taken from both sides.  A shape that moves to
another kernel fails on the route line, a kernel that is wrong fails on the bits.

The big-tile cases are checked against the oracle over their WHOLE output: at their sizes (17 - 19 G multiply-adds) the
multithreaded oracle takes about two seconds on 16 CPUs, so no rows are left to a sliced comparison."""
import ctypes as C
from collections import namedtuple

import numpy as np
import pytest

torch = pytest.importorskip("torch")
from failure_aware_vision_amd import _lib  # noqa: E402
from oracle import fav_oracle as O  # noqa: E402

# n frames of H x W x cin -> cout channels through a kh x kw window; res: with a residual; relu 0 none, 1 ReLU, 2 GELU;
# mode: fav_math_mode; device: operands drawn on the device (the large cases)
Case = namedtuple("Case", "name n H W cin cout kh kw stride pad res relu mode route device", defaults=(False,))
MODE_NAME = ("bf16", "f32")
GUARD = 4096              # bf16 elements in front of and behind the output
GUARD_VALUE = 3.0


def igemm(bm, bn, bk, ns, mode, epi, pp=False, gelu=False):
    return f"conv_igemm<{bm},{bn},{bk},{ns},{MODE_NAME[mode]},epi{epi}" + (",pp" if pp else "") + (",gelu" if gelu else "") + ">"


def generic_cases():
    """The 32 instantiations of the 128-row tile: the shape is chosen per (BN, BK, residual) by the rules in launch_conv's
    comments - BN 64 unless Cout is a multiple of 128; 64-deep steps for a window, for K >= 512 without a residual and for
    K >= 1024 with one; the staged epilogue (epi0) with a residual - and the route is spelled from the intended instantiation.
    M = 143 rows: two row tiles, the second one ragged."""
    shapes = {
        # (BN, BK, residual): cin, cout, k, stride, pad
        (64, 32, False): (64, 192, 1, 1, 0),      # K = 64: two K steps in a three-stage ring; three column tiles
        (64, 32, True): (256, 320, 1, 1, 0),      # five column tiles
        (64, 64, False): (64, 192, 3, 1, 1),
        (64, 64, True): (1024, 64, 1, 1, 0),      # K >= 1024 with a residual
        (128, 32, False): (128, 256, 1, 1, 0),
        (128, 32, True): (128, 128, 1, 1, 0),
        (128, 64, False): (512, 128, 1, 1, 0),
        (128, 64, True): (64, 256, 3, 2, 1),
    }
    out = []
    for (bn, bk, res), (cin, cout, k, stride, pad) in shapes.items():
        H, W = (11, 13) if stride == 1 else (21, 25)      # 143 output pixels either way
        for mode in (0, 1):
            for gelu in (False, True):
                name = f"generic-bn{bn}-bk{bk}-{'res' if res else 'nores'}-{MODE_NAME[mode]}{'-gelu' if gelu else ''}"
                out.append(Case(name, 1, H, W, cin, cout, k, k, stride, pad, res, 2 if gelu else 1, mode,
                                igemm(128, bn, bk, 3 if bk == 32 else 2, mode, 0 if res else 1, gelu=gelu)))
    return out


def threshold_cases():
    out = []
    # staged-patch 3x3 (3x3 / 1 / 1, Cin = Cout in {64, 128}, no residual) from 2048 rows - if its LDS image fits 160 KB: the
    # patch of 256 + 2 W + 2 pixels beside four weight stages admits W <= 60 at 128 channels, so 32 x 64 frames stay on the
    # generic kernel there and the threshold is crossed with the frames turned (89 x 23 against 64 x 32)
    for c, ns in ((64, 3), (128, 2)):
        bn = 64 if c == 64 else 128
        out.append(Case(f"halo-c{c}-2047", 1, 23, 89, c, c, 3, 3, 1, 1, False, 1, 0, igemm(128, bn, 64, 2, 0, 1)))
        for mode in (0, 1):
            halo = f"conv3x3_halo<{c},{c},256,{ns},{MODE_NAME[mode]}>"
            out.append(Case(f"halo-c{c}-2048-{MODE_NAME[mode]}", 1, 32, 64, c, c, 3, 3, 1, 1, False, 1, mode,
                            halo if c == 64 else igemm(128, bn, 64, 2, mode, 1)))
            if c == 128:
                out.append(Case(f"halo-c{c}-2048-narrow-{MODE_NAME[mode]}", 1, 64, 32, c, c, 3, 3, 1, 1, False, 1, mode, halo))
    out.append(Case("halo-c128-2047-narrow", 1, 89, 23, 128, 128, 3, 3, 1, 1, False, 1, 0, igemm(128, 128, 64, 2, 0, 1)))
    # row-owning projection (1x1, 256 -> 512, no residual, no ReLU, production mode) from 4096 output pixels
    out.append(Case("proj-s1-4095", 1, 63, 65, 256, 512, 1, 1, 1, 0, False, 0, 0, igemm(128, 128, 32, 3, 0, 1)))
    out.append(Case("proj-s1-4096", 1, 64, 64, 256, 512, 1, 1, 1, 0, False, 0, 0, "proj<256,512,nw4>"))
    out.append(Case("proj-s2-4095", 1, 125, 129, 256, 512, 1, 1, 2, 0, False, 0, 0, igemm(128, 128, 32, 3, 0, 1)))
    out.append(Case("proj-s2-4096", 1, 127, 127, 256, 512, 1, 1, 2, 0, False, 0, 0, "proj<256,512,nw4>"))
    out.append(Case("proj-s1-4096-f32-stays-generic", 1, 64, 64, 256, 512, 1, 1, 1, 0, False, 0, 1, igemm(128, 128, 32, 3, 1, 1)))
    # 256 x 256 tile from (M / 256) * (Cout / 256) = 512 big tiles
    big, big_f32 = igemm(256, 256, 64, 2, 0, 1, pp=True), igemm(256, 256, 64, 2, 1, 1)
    #   1x1, 512 -> 2048, with a residual: 63 x 8 = 504 against 64 x 8 = 512
    out.append(Case("big-1x1-res-16383", 1, 127, 129, 512, 2048, 1, 1, 1, 0, True, 1, 0, igemm(128, 128, 32, 3, 0, 0), True))
    out.append(Case("big-1x1-res-16384", 1, 128, 128, 512, 2048, 1, 1, 1, 0, True, 1, 0, big, True))
    out.append(Case("big-1x1-res-16500-ragged", 1, 125, 132, 512, 2048, 1, 1, 1, 0, True, 1, 0, big, True))
    out.append(Case("big-1x1-gelu-16384", 1, 128, 128, 512, 2048, 1, 1, 1, 0, False, 2, 0, igemm(256, 256, 64, 2, 0, 1, pp=True, gelu=True), True))
    out.append(Case("big-1x1-gelu-res-16384-f32", 1, 128, 128, 512, 2048, 1, 1, 1, 0, True, 2, 1, igemm(256, 256, 64, 2, 1, 1, gelu=True), True))
    #   3x3 without a residual, 64 -> 512: 255 x 2 = 510 against 256 x 2 = 512 (frames of 16 x 17: a ragged last tile of 16 rows)
    out.append(Case("big-3x3-65280", 240, 16, 17, 64, 512, 3, 3, 1, 1, False, 1, 0, igemm(128, 128, 64, 2, 0, 1), True))
    out.append(Case("big-3x3-65552-ragged", 241, 16, 17, 64, 512, 3, 3, 1, 1, False, 1, 0, big, True))
    out.append(Case("big-3x3-65552-ragged-f32", 241, 16, 17, 64, 512, 3, 3, 1, 1, False, 1, 1, big_f32, True))
    return out


def geometry_cases():
    """Geometry the generic kernel accepts and no network uses; 64 -> 64 channels, both math modes."""
    shapes = [
        # name, n, H, W, kh, kw, stride, pad
        ("1x1-frame-3x3-s1", 3, 1, 1, 3, 3, 1, 1),
        ("1x1-frame-3x3-s2", 3, 1, 1, 3, 3, 2, 1),
        ("2x2-frame-3x3-s1", 3, 2, 2, 3, 3, 1, 1),
        ("2x2-frame-3x3-s2", 3, 2, 2, 3, 3, 2, 1),
        ("row-frame-1x37", 2, 1, 37, 3, 3, 1, 1),
        ("column-frame-37x1", 2, 37, 1, 3, 3, 1, 1),
        ("7x7-s2", 2, 15, 15, 7, 7, 2, 3),
        ("1x3-pad0", 2, 9, 11, 1, 3, 1, 0),
        ("1x3-pad1", 2, 9, 11, 1, 3, 1, 1),
        ("3x1-pad0", 2, 9, 11, 3, 1, 1, 0),
        ("3x1-pad1", 2, 9, 11, 3, 1, 1, 1),
    ]
    out = []
    for mode in (0, 1):
        for name, n, H, W, kh, kw, stride, pad in shapes:
            out.append(Case(f"geom-{name}-{MODE_NAME[mode]}", n, H, W, 64, 64, kh, kw, stride, pad, False, 1, mode,
                            igemm(128, 64, 64, 2, mode, 1)))
        out.append(Case(f"geom-one-row-{MODE_NAME[mode]}", 1, 1, 1, 64, 64, 1, 1, 1, 0, False, 1, mode, igemm(128, 64, 32, 3, mode, 1)))
    return out


CASES = generic_cases() + threshold_cases() + geometry_cases()


@pytest.fixture(scope="module")
def lib():
    assert torch.cuda.is_available(), "GPU tests need a MI355X"
    return _lib.load()


def out_hw(c):
    return (c.H + 2 * c.pad - c.kh) // c.stride + 1, (c.W + 2 * c.pad - c.kw) // c.stride + 1


def case_seed(c):
    return sum(ord(ch) * (i + 1) for i, ch in enumerate(c.name))


def host_operands(c):
    """[x, w, bias, residual] of a case drawn on the host: fp32 arrays of bf16 values (bias: any fp32); no device needed."""
    assert not c.device
    ho, wo = out_hw(c)
    k = c.kh * c.kw * c.cin
    rng = np.random.default_rng(case_seed(c))
    x = O.bf16_round((rng.standard_normal((c.n, c.H, c.W, c.cin)) * np.exp2(rng.integers(-2, 3, (c.n, c.H, c.W, c.cin)))).astype(np.float32))
    w = O.bf16_round((rng.standard_normal((c.cout, c.kh, c.kw, c.cin)) * np.sqrt(2.0 / k)).astype(np.float32))
    b = (rng.standard_normal(c.cout) * 0.2).astype(np.float32)
    r = O.bf16_round(rng.standard_normal((c.n, ho, wo, c.cout)).astype(np.float32)) if c.res else None
    return [x, w, b, r]


def operands(c):
    """x, w, bias, residual as fp32 arrays of bf16 values (bias: any fp32), and their device tensors."""
    ho, wo = out_hw(c)
    seed = case_seed(c)
    k = c.kh * c.kw * c.cin
    if c.device:
        g = torch.Generator(device="cuda").manual_seed(seed)
        xd = (torch.randn((c.n, c.H, c.W, c.cin), device="cuda", generator=g) * 0.7).to(torch.bfloat16)
        wd = (torch.randn((c.cout, c.kh, c.kw, c.cin), device="cuda", generator=g) * (2.0 / k) ** 0.5).to(torch.bfloat16)
        bd = torch.randn((c.cout,), device="cuda", generator=g) * 0.2
        rd = torch.randn((c.n, ho, wo, c.cout), device="cuda", generator=g).to(torch.bfloat16) if c.res else None
        host = [t.float().cpu().numpy() if t is not None else None for t in (xd, wd, bd, rd)]
    else:
        host = x, w, b, r = host_operands(c)
        xd, wd, bd = (torch.from_numpy(x).cuda().to(torch.bfloat16), torch.from_numpy(w).cuda().to(torch.bfloat16),
                      torch.from_numpy(b).cuda())
        rd = torch.from_numpy(r).cuda().to(torch.bfloat16) if c.res else None
    return host, (xd, wd, bd, rd), (ho, wo)


def expected(c, x, w, b, r):
    acc = O.conv_acc_exact(x, w, c.kh, c.kw, c.stride, c.pad, mode="mfma" if c.mode == 0 else True)
    if c.relu == 2:     # ((acc + bias) + residual) -> GELU -> one bf16 rounding
        pre = acc + b
        if r is not None:
            pre = pre + r
        return O.bf16_round(O.gelu_exact(pre.astype(np.float32)))
    return O.epilogue(acc, b, res=r, relu=bool(c.relu))


@pytest.mark.gpu
@pytest.mark.parametrize("c", CASES, ids=[c.name for c in CASES])
def test_conv_route_bits_and_guards(lib, c):
    (x, w, b, r), (xd, wd, bd, rd), (ho, wo) = operands(c)
    count = c.n * ho * wo * c.cout
    ybig = torch.full((count + 2 * GUARD,), GUARD_VALUE, dtype=torch.bfloat16, device="cuda")
    d = _lib.FavConvDesc(xd.data_ptr(), wd.data_ptr(), bd.data_ptr(), rd.data_ptr() if rd is not None else None,
                         ybig.data_ptr() + 2 * GUARD, c.n, c.H, c.W, c.cin, c.cout, c.kh, c.kw, c.stride, c.pad, c.relu, 0, c.mode,
                         _lib.FavDropoutDesc(-1, 0, 1.0, 0, 0, 1, 0))
    _lib.check(lib.fav_op_conv2d(C.byref(d), None))
    route = _lib.last_route()
    assert _lib.route_conv2d(d) == (0, route) and _lib.last_route() == route     # the selector, asked without a launch, names what ran
    torch.cuda.synchronize()
    assert route == c.route
    assert bool((ybig[:GUARD] == GUARD_VALUE).all()) and bool((ybig[-GUARD:] == GUARD_VALUE).all()), "wrote outside the output"
    got = ybig[GUARD:-GUARD].reshape(c.n, ho, wo, c.cout).float().cpu().numpy()
    exp = expected(c, x, w, b, r)
    assert got.shape == exp.shape
    assert np.array_equal(got, exp), f"{np.mean(got != exp):.6f} of elements differ, max {np.abs(got - exp).max()}"


@pytest.mark.gpu
def test_route_is_of_the_last_op_only(lib):
    """A fav_op_* whose launcher has a single kernel, and a refused call, leave no route of an earlier launch behind."""
    c = CASES[0]
    _, (xd, wd, bd, _), (ho, wo) = operands(c)
    y = torch.empty((c.n, ho, wo, c.cout), dtype=torch.bfloat16, device="cuda")
    none = _lib.FavDropoutDesc(-1, 0, 1.0, 0, 0, 1, 0)
    d = _lib.FavConvDesc(xd.data_ptr(), wd.data_ptr(), bd.data_ptr(), None, y.data_ptr(), c.n, c.H, c.W, c.cin, c.cout, c.kh, c.kw,
                         c.stride, c.pad, c.relu, 0, c.mode, none)
    _lib.check(lib.fav_op_conv2d(C.byref(d), None))
    assert _lib.last_route() == c.route
    p = torch.empty((c.n, (ho - 1) // 2 + 1, (wo - 1) // 2 + 1, c.cout), dtype=torch.bfloat16, device="cuda")
    _lib.check(lib.fav_op_maxpool3x3s2(y.data_ptr(), p.data_ptr(), c.n, ho, wo, c.cout, None))
    assert _lib.last_route() == ""
    _lib.check(lib.fav_op_conv2d(C.byref(d), None))
    assert _lib.last_route() == c.route
    # a buffer one byte short of the name: refused with a message of its own, the buffer left empty, the route kept
    small = C.create_string_buffer(b"x" * (len(c.route) - 1), len(c.route))
    assert lib.fav_op_last_route(small, len(c.route)) == 1 and small.value == b""
    assert lib.fav_last_error(None).decode() == f"fav_op_last_route: the name needs {len(c.route) + 1} bytes, the buffer has {len(c.route)}"
    exact = C.create_string_buffer(len(c.route) + 1)
    assert lib.fav_op_last_route(exact, len(c.route) + 1) == 0 and exact.value.decode() == c.route
    # a classify call refused at its gate (no handle) clears the route as a served one does
    assert lib.fav_classify_ex(None, None, 1, 0, 0, None, None, None, None, None) == 1
    assert _lib.last_route() == ""
    _lib.check(lib.fav_op_conv2d(C.byref(d), None))
    assert _lib.last_route() == c.route
    d.Cin = 96
    assert lib.fav_op_conv2d(C.byref(d), None) == 1
    assert _lib.last_route() == ""
    torch.cuda.synchronize()
