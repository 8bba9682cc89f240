"""NaN and the infinities through every epilogue, pool and ViT op, and through whole handles, to the non-finite frame rule
(include/fav.h beside fav_op_conv2d).

Op level: one poisoned problem per epilogue family (tests/nonfinite_ref.py builds them; tests/test_nonfinite_host.py shows on the
CPU that each reaches every class and leaves at least half of its elements clean - asserted again here, on the very arrays that
are launched).  Every case asserts the route by name, the class of EVERY output element against the float64 reference, the
bits of every clean element against the existing oracle on the clean operands, and the guard bands.  The tail cases also demand
the bits - NaN patterns included - of the separate launches they replace, which take the staged and the register epilogues.

What the device does with a NaN (recorded by test_device_nan_patterns, printed with -s; DESIGN.md has the findings): the matrix
unit answers with a NaN whose sign bit is SET.  Hence contract point 3: a handle can hold sign-set NaNs, so every ReLU keeps a
NaN of either sign - one fp32 maximum at every site - and the cases below hold the ReLU epilogues to the reference's classes for
the sign-clear and the sign-set NaN alike.

Handle level: overflowing twins of the fixtures (two consecutive layers scaled by 2^100, every weight finite, accepted by
fav_check_blob) must end in the non-finite frame rule in every configuration of batch, route and schedule, and equal the
repaired oracle; a twin scaled by 2^40 on one layer is huge but finite and must match the oracle bit for bit, no frame flagged."""
import ctypes as C

import numpy as np
import pytest

pytestmark = pytest.mark.gpu

torch = pytest.importorskip("torch")
import nonfinite_ref as N  # noqa: E402
from failure_aware_vision_amd import Backend, _lib, synth, weights  # noqa: E402
from failure_aware_vision_amd.conformal import Conformal  # noqa: E402
from oracle import fav_oracle as O  # noqa: E402
from test_gpu_ops import drop_desc  # noqa: E402
from test_gpu_pool_dropout_edges import Guarded, dev_bits, host_bits  # noqa: E402

GUARD_F32 = 4096


@pytest.fixture(scope="module")
def lib():
    assert torch.cuda.is_available(), "GPU tests need a MI355X"
    return _lib.load()


def bits32(v):
    return np.ascontiguousarray(v, np.float32).view(np.uint32)


def assert_classes(got, ref_cls, what):
    gc = N.classes(got)
    bad = gc != ref_cls
    assert not bad.any(), (f"{what}: {int(bad.sum())} of {bad.size} elements in the wrong class; first at {tuple(np.argwhere(bad)[0])}: "
                           f"device {N.CLASS_NAMES[gc[bad][0]]}, reference {N.CLASS_NAMES[ref_cls[bad][0]]}")


def assert_clean_bits(got, exp, clean, what):
    d = bits32(got)[clean] != bits32(exp)[clean]
    assert not d.any(), f"{what}: {d.mean():.6f} of the clean elements differ from the oracle on the clean operands"


def nan_report(got, what):
    """The NaN patterns of an output, for the record."""
    b = bits32(got)[np.isnan(got)]
    pats = sorted({hex(int(v)) for v in np.unique(b)})
    print(f"[nan-pattern] {what}: {b.size} NaNs, patterns {pats}")
    return b


# ---------------------------------------------------------------------------------------------------------------------
# convolutions
# ---------------------------------------------------------------------------------------------------------------------
def launch_conv(lib, c, mode, x, w, b, r, drop=None):
    """-> (output as fp32 with the device's bits, route).  bf16 operands go up bit for bit."""
    ho, wo = (c.H + 2 * c.pad - c.k) // c.stride + 1, (c.W + 2 * c.pad - c.k) // c.stride + 1
    shape = (c.n, ho, wo, c.cout)
    xd, wd, bd = dev_bits(x), dev_bits(w), torch.from_numpy(b).cuda()
    rd = dev_bits(r) if r is not None else None
    if c.out_f32:
        big = torch.full((int(np.prod(shape)) + 2 * GUARD_F32,), 3.0, dtype=torch.float32, device="cuda")
        ptr = big.data_ptr() + 4 * GUARD_F32
    else:
        y = Guarded(shape)
        ptr = y.ptr
    d = _lib.FavConvDesc(xd.data_ptr(), wd.data_ptr(), bd.data_ptr(), rd.data_ptr() if rd is not None else None, ptr, c.n, c.H, c.W,
                         c.cin, c.cout, c.k, c.k, c.stride, c.pad, c.act, c.out_f32, mode, drop or drop_desc())
    _lib.check(lib.fav_op_conv2d(C.byref(d), None))
    route = _lib.last_route()
    assert _lib.route_conv2d(d) == (0, route)
    torch.cuda.synchronize()
    if c.out_f32:
        assert bool((big[:GUARD_F32] == 3.0).all()) and bool((big[-GUARD_F32:] == 3.0).all()), "the guard band was written"
        return big[GUARD_F32:-GUARD_F32].cpu().numpy().reshape(shape), route
    return y.value(), route


def conv_expected(c, mode, x, w, b, r):
    """The existing oracle on finite operands (tests/test_gpu_conv_routes.py: expected)."""
    acc = O.conv_acc_exact(x, w, c.k, c.k, c.stride, c.pad, mode="mfma" if mode == 0 else True)
    if c.out_f32 or c.act == 2:
        pre = acc + b
        if r is not None:
            pre = pre + r
        if c.act == 2:
            return O.bf16_round(O.gelu_exact(pre.astype(np.float32)))
        return np.maximum(pre, np.float32(0.0)) if c.act == 1 else pre
    return O.epilogue(acc, b, res=r, relu=bool(c.act))


def device_operands(c):
    """The large case's operands, drawn on the device as tests/test_gpu_conv_routes.py draws them."""
    g = torch.Generator(device="cuda").manual_seed(len(c.name) * 977)
    kk = c.k * c.k * c.cin
    ho, wo = (c.H + 2 * c.pad - c.k) // c.stride + 1, (c.W + 2 * c.pad - c.k) // c.stride + 1
    xd = (torch.randn((c.n, c.H, c.W, c.cin), device="cuda", generator=g) * 0.7).clamp(-4, 4).to(torch.bfloat16)
    wd = (torch.randn((c.cout, c.k, c.k, c.cin), device="cuda", generator=g) * (2.0 / kk) ** 0.5).to(torch.bfloat16)
    bd = torch.randn((c.cout,), device="cuda", generator=g) * 0.2
    rd = torch.randn((c.n, ho, wo, c.cout), device="cuda", generator=g).to(torch.bfloat16) if c.res else None
    return [t.float().cpu().numpy() if t is not None else None for t in (xd, wd, bd, rd)]


CONV_PARAMS = [(c, m) for c in N.CONV_CASES for m in c.modes]


@pytest.mark.parametrize("c,mode", CONV_PARAMS, ids=[f"{c.name}-{N.MODE_NAME[m]}" for c, m in CONV_PARAMS])
def test_conv_epilogues_keep_the_ieee_class(lib, c, mode):
    if c.name.startswith("big"):
        x, w, b, r = device_operands(c)
    else:
        x, w, b, r = N.conv_operands(c, np.random.default_rng(sum(map(ord, c.name))))
    p, clean = N.conv_problem(c, x, w, b, r)
    ref_cls, pre_cls = N.conv_case_ref(c, p)
    N.assert_covers(ref_cls, pre_cls, clean["mask"], c.act, c.name)
    got, route = launch_conv(lib, c, mode, p["x"], p["w"], p["b"], p["res"])
    assert route == c.route.format(m=N.MODE_NAME[mode])
    nan_report(got, f"{c.name} {N.MODE_NAME[mode]}")
    assert_classes(got, ref_cls, c.name)
    assert_clean_bits(got, conv_expected(c, mode, clean["x"], p["w"], clean["b"], clean["res"]), clean["mask"], c.name)


def test_device_nan_patterns(lib):
    """The record behind contract point 3, on the no-ReLU register epilogue - nothing between the
    accumulator and the store but the bias add and the rounding - and, for the same problems, the ReLU one: which NaN the matrix
    unit makes (kind pair: +inf and -inf products in one accumulator; +inf on a zero weight: inf x 0), which the vector unit makes
    (a bias of -inf under an accumulator of +inf) and what becomes of a caller's NaN of either sign.  The patterns are printed
    (-s); asserted is what the contract needs: whatever the pattern and its sign, every one of these NaNs is still a NaN behind
    the ReLU.  Measured on an MI355X: v_mfma_f32_16x16x32_bf16 answers 0xFFC00000 - sign SET - for a NaN it makes and for one
    it is given, so a ReLU that drops sign-set NaNs (an integer maximum on the bits) would lose every NaN the network makes."""
    norelu = next(k for k in N.CONV_CASES if k.name == "register-norelu")
    relu = next(k for k in N.CONV_CASES if k.name == "register-nores")
    x, w, b, _ = N.conv_operands(norelu, np.random.default_rng(5))
    hexes = lambda a: [hex(int(v)) for v in np.unique(bits32(a))]      # noqa: E731
    for mode in norelu.modes:
        rec = {}
        for kind in ("pair", "nan", "nan_neg", "+inf"):
            p = dict(x=x.copy(), w=w.copy(), b=b.copy(), res=None, geom=(1, 1, 1, 0))
            N.poison(p, kind, (0, 4, 4))
            if kind == "+inf":
                p["w"][0::2, ..., 3] = 0.0                       # inf x 0 in the even output channels
                p["w"][1::2, ..., 3] = np.float32(0.5)           # +inf in the odd ones, under a bias of -inf: the epilogue's add makes the NaN
                p["b"][1::2] = -np.inf
            px = launch_conv(lib, norelu, mode, p["x"], p["w"], p["b"], None)[0][0, 4, 4]
            assert np.isnan(px).all(), kind
            if kind == "+inf":
                rec["inf x 0 (matrix unit)"], rec["+inf + -inf (vector add)"] = hexes(px[0::2]), hexes(px[1::2])
            else:
                rec[{"pair": "+inf - inf (matrix unit)", "nan": "0x7FC0 in", "nan_neg": "0xFFC0 in"}[kind]] = hexes(px)
            px = launch_conv(lib, relu, mode, p["x"], p["w"], p["b"], None)[0][0, 4, 4]
            assert np.isnan(px).all(), f"{kind}: a NaN was lost in the ReLU"
        print(f"[nan-record] {N.MODE_NAME[mode]}: {rec}")


# ---------------------------------------------------------------------------------------------------------------------
# bottleneck tails, entry reduce
# ---------------------------------------------------------------------------------------------------------------------
TAIL_CASES = [   # cmid, nred, has3x3, H, W, n, route: the smallest shape of each arm in tests/test_gpu_tail.py
    (64, 64, True, 7, 9, 37, "tail<64,64,3x3,nw4,wc2>"),
    (128, 0, False, 9, 11, 3, "tail<128,0,1x1,nw8,wc2>"),
    (256, 256, False, 5, 7, 9, "tail<256,256,1x1,nw8,wc2,rp16>"),
    (512, 0, False, 8, 10, 3, "tail<512,0,1x1,nw8,wc2>"),
]


def conv_bits(lib, x, w, b, res, stride, pad, relu, drop=None):
    n, H, W, cin = x.shape
    c = N.ConvCase("", n, H, W, cin, w.shape[0], w.shape[1], stride, pad, res is not None, relu, 0, (0,), "")
    return launch_conv(lib, c, 0, x, w, b, res, drop)


def tail_bits(lib, t, drop=None, res_entry=None):
    n, H, W, cmid = t["x"].shape
    cout = 4 * cmid
    nred = t["wa"].shape[0] if t["wa"] is not None else 0
    dv = {k: dev_bits(t[k]) for k in ("x", "wc", "res") + (("wb",) if t["wb"] is not None else ()) + (("wa",) if nred else ())}
    fb = {k: torch.from_numpy(t[k]).cuda() for k in ("bb", "bc", "ba") if t[k] is not None}
    y, t1n = Guarded((n, H, W, cout)), Guarded((n, H, W, max(nred, 1)))
    ptr = lambda k, src: src[k].data_ptr() if k in src else None      # noqa: E731
    d = _lib.FavTailDesc(dv["x"].data_ptr(), ptr("wb", dv), ptr("bb", fb), dv["wc"].data_ptr(), fb["bc"].data_ptr(), dv["res"].data_ptr(),
                         y.ptr, ptr("wa", dv), ptr("ba", fb), t1n.ptr if nred else None, n, H, W, cmid, nred, drop or drop_desc(),
                         *(res_entry or ()))
    _lib.check(lib.fav_op_bottleneck_tail(C.byref(d), None))
    route = _lib.last_route()
    torch.cuda.synchronize()
    return y.value(), (t1n.value() if nred else None), route


def tail_keep(n, H, W, cout, thr, seed, site, v0, n_img, first):
    v = v0 + np.arange(n)
    return np.stack([O.dropout_keep(seed, int(tt), site, np.array([ii]), H * W * cout, thr)[0] for tt, ii in zip(v // n_img, v % n_img + first)])


@pytest.mark.parametrize("with_drop", [False, True])
@pytest.mark.parametrize("cmid,nred,has3x3,H,W,n,route", TAIL_CASES, ids=[c[6] for c in TAIL_CASES])
def test_tails_keep_the_class_and_equal_the_separate_launches(lib, cmid, nred, has3x3, H, W, n, route, with_drop):
    """The fused tail against the three fav_op_conv2d launches it replaces on the SAME poisoned problem: identical bits, NaN
    patterns included (the separate conv_c takes the staged epilogue, the tail its own); every class as the reference says;
    clean pixels as the oracle on the clean operands."""
    t = N.tail_problem(np.random.default_rng(cmid + nred + H), cmid, nred, has3x3, H, W, n)
    cout = 4 * cmid
    thr, seed, site, v0, first = 26, 0x1234567ABC, 5, 3, 40
    scale = O.dropout_scale(thr)
    dd = drop_desc(site, thr, float(scale), seed, v0, n + 1, first) if with_drop else None
    keep = tail_keep(n, H, W, cout, thr, seed, site, v0, n + 1, first) if with_drop else None
    y, t1n, got_route = tail_bits(lib, t, dd)
    assert got_route == route
    t2 = conv_bits(lib, t["x"], t["wb"], t["bb"], None, 1, 1, 1)[0] if has3x3 else t["x"]
    y_sep, sep_route = conv_bits(lib, t2, t["wc"], t["bc"], t["res"], 1, 0, 1, dd)
    assert "epi0" in sep_route
    assert np.array_equal(bits32(y), bits32(y_sep)), f"Y: {np.mean(bits32(y) != bits32(y_sep)):.6f} of the bits differ from the separate launches"
    if nred:
        t1_sep = conv_bits(lib, y_sep, t["wa"], t["ba"], None, 1, 0, 1)[0]
        assert np.array_equal(bits32(t1n), bits32(t1_sep))
    nan_report(y, route)
    ycls, t1cls, clean_px = N.tail_ref(t, keep, scale)
    assert_classes(y, ycls, route + " Y")
    if nred:
        assert_classes(t1n, t1cls, route + " t1n")
    assert clean_px.mean() >= 0.5 and {N.NAN, N.FIN} <= set(np.unique(ycls).tolist())
    # clean pixels against the oracle on the clean operands
    o2 = O.epilogue(O.conv_acc_exact(t["x_clean"], t["wb"], 3, 3, 1, 1, mode="mfma"), t["bb"]) if has3x3 else t["x_clean"]
    oy = O.epilogue(O.conv_acc_exact(o2, t["wc"], 1, 1, 1, 0, mode="mfma"), t["bc"], res=t["res_clean"], relu=True, keep=keep, scale=scale)
    assert_clean_bits(y, oy, np.broadcast_to(clean_px[..., None], y.shape), route + " Y")
    if nred:
        ot = O.epilogue(O.conv_acc_exact(oy, t["wa"], 1, 1, 1, 0, mode="mfma"), t["ba"])
        assert_clean_bits(t1n, ot, np.broadcast_to(clean_px[..., None], t1n.shape), route + " t1n")


def test_entry_reduce_and_res_entry_tail_keep_the_class(lib):
    """entry_reduce<256,64> (entry dropout + the 1x1 reduce, packed ReLU) and the res_entry tail behind it on a cached prefix
    output that holds the specials: the dropped copies are a select (a dropped NaN is 0, a kept one stays NaN), the reduce's
    classes are the reference's, and both equal the separate launches bit for bit."""
    rng = np.random.default_rng(31)
    n_img, H, W, v0, n_out, Cc, nred = 3, 7, 9, 2, 7, 256, 64
    thr, seed, first, site_e, site_o = 26, 77, 40, 1, 3
    scale = O.dropout_scale(thr)
    x0 = np.maximum(N.finite_bf16(rng, (n_img, H, W, Cc)), 0)
    x = x0.copy()
    for i, kind in enumerate(("+inf", "nan", "+inf", "nan")):               # what a ReLU output can hold, at four pixels of frame 1:
        x[1, 1 + i, 2, slice(3, 4) if i in (0, 3) else slice(3 + i, 200, 16)] = N.special(kind)      # one channel, or thirteen
    wa = O.bf16_round((rng.standard_normal((nred, 1, 1, Cc)) * np.sqrt(2.0 / Cc)).astype(np.float32))
    ba = (rng.standard_normal(nred) * 0.2).astype(np.float32)
    de = drop_desc(site_e, thr, float(scale), seed, v0, n_img, first)
    xd, wd, bd = dev_bits(x), dev_bits(wa), torch.from_numpy(ba).cuda()
    y, t1 = Guarded((n_out, H, W, Cc)), Guarded((n_out, H, W, nred))
    _lib.check(lib.fav_op_entry_reduce(xd.data_ptr(), y.ptr, wd.data_ptr(), bd.data_ptr(), t1.ptr, Cc, nred, H * W, n_out, C.byref(de), None))
    assert _lib.last_route() == "entry_reduce<256,64>"
    torch.cuda.synchronize()
    y, t1 = y.value(), t1.value()
    y2 = Guarded((n_out, H * W * Cc))
    _lib.check(lib.fav_op_entry_dropout(xd.data_ptr(), y2.ptr, H * W * Cc, n_out, C.byref(de), None))
    torch.cuda.synchronize()
    y_sep = y2.value().reshape(n_out, H, W, Cc)
    assert np.array_equal(bits32(y), bits32(y_sep))
    t1_sep = conv_bits(lib, y_sep, wa, ba, None, 1, 0, 1)[0]
    assert np.array_equal(bits32(t1), bits32(t1_sep))
    v = v0 + np.arange(n_out)
    keep = np.stack([O.dropout_keep(seed, int(tt), site_e, np.array([ii]), H * W * Cc, thr)[0]
                     for tt, ii in zip(v // n_img, v % n_img + first)]).reshape(n_out, H, W, Cc)
    src = x[v % n_img]
    ycls = N.dropout_ref(src, keep, scale)
    assert_classes(y, ycls, "entry dropout")
    special_in = ~np.isfinite(src)
    assert (special_in & keep).any() and (special_in & ~keep).any(), "the mask neither keeps nor drops a special value"
    assert (bits32(y)[special_in & ~keep] == 0).all()
    yv = N.epilogue_values(src, 0.0, None, 0, keep, scale)
    t1cls = N.classes(N.epilogue_values(N.dot_values(yv.reshape(-1, Cc), wa.reshape(nred, Cc)), ba, None, 1)).reshape(t1.shape)
    assert_classes(t1, t1cls, "entry reduce t1")
    assert {N.NAN, N.PINF, N.FIN} <= set(np.unique(t1cls).tolist())
    clean = (v % n_img) != 1
    oy = O.bf16_round(np.where(keep, x0[v % n_img] * scale, 0).astype(np.float32))
    assert_clean_bits(y, oy, np.broadcast_to(clean[:, None, None, None], y.shape), "entry dropout")
    assert_clean_bits(t1, O.epilogue(O.conv_acc_exact(oy, wa, 1, 1, 1, 0, mode="mfma"), ba), np.broadcast_to(clean[:, None, None, None], t1.shape), "t1")
    # the res_entry tail: its residual is the cached x (specials included) under the entry mask, recomputed in the epilogue
    t = N.tail_problem(rng, 64, 64, True, H, W, n_out)
    do = drop_desc(site_o, thr, float(scale), seed, v0, n_img, first)
    stored = dict(t, x=t1, x_clean=t1, res=y, res_clean=y)
    y_ref, t1n_ref, _ = tail_bits(lib, stored, do)
    recomputed = dict(stored, res=x)
    y_re, t1n_re, route = tail_bits(lib, recomputed, do, res_entry=(1, site_e))
    assert route == "tail<64,64,3x3,nw4,wc2,res_entry>"
    assert np.array_equal(bits32(y_re), bits32(y_ref)) and np.array_equal(bits32(t1n_re), bits32(t1n_ref))
    assert np.isnan(y_re).any()


# ---------------------------------------------------------------------------------------------------------------------
# the fused ImageNet stem
# ---------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("layout", [0, 1])
def test_stem_pool_overflows_by_its_weights(lib, layout):
    """Pixels cannot be non-finite, the weights can be huge: frames of constant 255 (normalised pixels of 2.2 - 2.6) against output
    channels whose weights are all +2^127 (every product overflows fp32: +inf), all -2^127 (-inf, +0 behind the ReLU) and
    both (channel 2: +2^127 in the window's first row, -2^127 elsewhere).  The products are finite, so the last is no NaN by
    IEEE: the accumulator saturates with the first products it meets and finite products cannot move an infinity.  The
    expectation is the repaired oracle's; the max pool then spreads +inf and keeps the clean channels' bits."""
    n, H, W = 2, 33, 47
    rng = np.random.default_rng(7 + layout)
    img = np.full((n, H, W, 3), 255, np.uint8) if layout == 0 else np.ones((n, H, W, 3), np.float32)
    mean, std = (0.485, 0.456, 0.406), (0.229, 0.224, 0.225)
    istd = O.inv_std32(std)
    w = O.bf16_round((rng.standard_normal((64, 7, 7, 3)) * np.sqrt(2.0 / 147)).astype(np.float32))
    big = np.float32(2.0 ** 127)
    w[0], w[1], w[2] = big, -big, -big
    w[2, 0] = big
    w[3].reshape(-1)[0::2], w[3].reshape(-1)[1::2] = big, -big      # channel 3: both signs inside every step of 8 products
    b = (rng.standard_normal(64) * 0.2).astype(np.float32)
    cols, ho, wo = O._im2col(O.normalize_input(img, mean, istd), 7, 7, 2, 3)
    a = np.zeros((n, ho, wo, 192), np.float32)
    a[..., :147] = cols.reshape(n, ho, wo, 147)
    wp = np.zeros((64, 1, 1, 192), np.float32)
    wp[:, 0, 0, :147] = w.reshape(64, 147)
    conv = O.epilogue(O.conv_acc_exact(a, wp, 1, 1, 1, 0, mode="mfma"), b, res=None, relu=True)
    assert (conv[..., 0] == np.inf).all() and (conv[..., 1] == 0).all() and not np.isfinite(conv[..., 2]).all()
    ref = O.maxpool3x3s2(conv)
    out = Guarded(ref.shape)
    m3, i3 = (C.c_float * 3)(*mean), (C.c_float * 3)(*[float(v) for v in istd])
    wd, bd = dev_bits(wp.reshape(64, 192)), torch.from_numpy(b).cuda()
    imgd = torch.from_numpy(img).cuda()
    _lib.check(lib.fav_op_stem_pool(imgd.data_ptr(), layout, n, H, W, wd.data_ptr(), bd.data_ptr(), m3, i3, out.ptr, None))
    assert _lib.last_route() == ("stem7_pool<u8>", "stem7_pool<f32>")[layout]
    torch.cuda.synchronize()
    got = out.value()
    nan_report(got, f"stem7_pool layout {layout}")
    for ch in (2, 3):
        print(f"[stem] channel {ch} classes (nan, +inf, -inf, finite): device {np.bincount(N.classes(got[..., ch]).ravel(), minlength=4)}, "
              f"oracle {np.bincount(N.classes(ref[..., ch]).ravel(), minlength=4)}")
    assert_classes(got, N.classes(ref), "stem7_pool")
    assert np.isnan(got[..., 2:4]).any(), "products beyond the fp32 range count as infinities: both signs in one sum are a NaN"
    assert np.array_equal(bits32(got[..., 4:]), bits32(ref[..., 4:]))


# ---------------------------------------------------------------------------------------------------------------------
# pools, entry dropout
# ---------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("n,H,W,Cc", [(3, 5, 7, 24), (4, 9, 11, 64)])
def test_pools_keep_the_class(lib, n, H, W, Cc):
    rng = np.random.default_rng(H * W + Cc)
    p, x = N.pool_input(rng, n, H, W, Cc)
    # max pool: NaN when any tap inside the frame is NaN
    ref = N.maxpool_ref(p)
    assert set(np.unique(ref).tolist()) == {N.NAN, N.PINF, N.NINF, N.FIN}
    y = Guarded((n, (H - 1) // 2 + 1, (W - 1) // 2 + 1, Cc))
    pd = dev_bits(p)
    _lib.check(lib.fav_op_maxpool3x3s2(pd.data_ptr(), y.ptr, n, H, W, Cc, None))
    torch.cuda.synchronize()
    got = y.value()
    assert_classes(got, ref, "max pool")
    clean = np.zeros(ref.shape, bool)
    clean[0] = True
    assert_clean_bits(got, O.maxpool3x3s2(x), clean, "max pool")
    fin = ref == N.FIN
    assert np.array_equal(got[fin], O.maxpool3x3s2(np.where(np.isnan(p), -np.inf, p))[fin]), "a finite maximum beside the specials"
    # average pool, without and with dropout
    if Cc % 16:                                   # the average pool takes 16-channel chunks
        return
    thr = O.dropout_threshold(0.5)
    scale = O.dropout_scale(thr)
    keep = np.stack([O.dropout_keep(77, (2 + i) // 5, 16, np.array([40 + (2 + i) % 5]), Cc, thr)[0] for i in range(n)])
    for drop, kp in ((None, None), (drop_desc(16, thr, float(scale), 77, 2, 5, 40), keep)):
        ya = Guarded((n, Cc))
        _lib.check(lib.fav_op_avgpool(pd.data_ptr(), ya.ptr, n, H * W, Cc, C.byref(drop) if drop is not None else None, None))
        torch.cuda.synchronize()
        ga = ya.value()
        ra = N.avgpool_ref(p.reshape(n, H * W, Cc), kp, scale)
        if kp is None:
            assert set(np.unique(ra).tolist()) == {N.NAN, N.PINF, N.NINF, N.FIN}
        assert_classes(ga, ra, "average pool")
        exp = O.global_avgpool(x)
        exp = O.bf16_round(exp if kp is None else np.where(kp, exp * scale, 0).astype(np.float32))
        cl = np.zeros(ra.shape, bool)
        cl[0] = True
        assert_clean_bits(ga, exp, cl, "average pool")


def test_entry_dropout_is_a_select(lib):
    rng = np.random.default_rng(6)
    n_img, E, n_out, v0 = 6, 7 * 7 * 64, 13, 2
    p, x = N.rows_input(rng, n_img, E)
    p[1, ::5], p[3, 1::5], p[5, 2::5] = np.inf, N.special("nan"), N.special("nan_neg")      # enough specials for both sides of the mask
    thr = O.dropout_threshold(0.4)
    scale = O.dropout_scale(thr)
    d = drop_desc(2, thr, float(scale), 5, v0, n_img, 9)
    out = Guarded((n_out, E))
    pd = dev_bits(p)
    _lib.check(lib.fav_op_entry_dropout(pd.data_ptr(), out.ptr, E, n_out, C.byref(d), None))
    torch.cuda.synchronize()
    got = out.value()
    v = v0 + np.arange(n_out)
    keep = np.stack([O.dropout_keep(5, int(t), 2, np.array([9 + int(i)]), E, thr)[0] for t, i in zip(v // n_img, v % n_img)])
    src = p[v % n_img]
    ref = N.dropout_ref(src, keep, scale)
    assert set(np.unique(ref).tolist()) == {N.NAN, N.PINF, N.NINF, N.FIN}
    assert_classes(got, ref, "entry dropout")
    sp = ~np.isfinite(src)
    assert (sp & keep).any() and (sp & ~keep).any() and (bits32(got)[sp & ~keep] == 0).all(), "a dropped special value is +0"
    nan_report(got, "entry dropout (0x7FC0 and 0xFFC0 in)")
    exp = O.bf16_round(np.where(keep, x[v % n_img] * scale, 0).astype(np.float32))
    assert_clean_bits(got, exp, np.isfinite(src) | ~keep, "entry dropout")


# ---------------------------------------------------------------------------------------------------------------------
# ViT ops
# ---------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("with_res", [False, True])
@pytest.mark.parametrize("act", [0, 1, 2])
def test_linear_streamk_keeps_the_class(lib, act, with_res):
    rows, K, Nn = 5505, 768, 768
    p, clean = N.linear_problem(np.random.default_rng(act * 2 + with_res), rows, K, Nn, with_res)
    x, w, r = p["x"].reshape(rows, K), p["w"].reshape(Nn, K), None if not with_res else p["res"].reshape(rows, Nn)
    ref = N.linear_ref(x, w, p["b"], r, act)
    pre = N.linear_ref(x, w, p["b"], r, 0)
    mask = clean["mask"].reshape(rows, Nn)
    N.assert_covers(ref, pre, mask, act, f"linear act {act}")
    y = Guarded((rows, Nn))
    ybuf = y.big[y.guard:-y.guard].view(rows, Nn)
    if with_res:
        ybuf.copy_(dev_bits(r))                                   # the residual is read in place
    xd, wd, bd = dev_bits(x), dev_bits(w), torch.from_numpy(p["b"]).cuda()
    ld = _lib.FavLinearDesc(xd.data_ptr(), wd.data_ptr(), bd.data_ptr(), y.ptr if with_res else None, y.ptr, rows, K, Nn, act)
    _lib.check(lib.fav_op_linear_streamk(C.byref(ld), None))
    torch.cuda.synchronize()
    got = y.value()
    assert_classes(got, ref, f"linear act {act}")
    acc = O.conv_acc_exact(clean["x"], p["w"], 1, 1, 1, 0, mode="mfma").reshape(rows, Nn)
    cr = None if not with_res else clean["res"].reshape(rows, Nn)
    if act == 2:
        exp = O.bf16_round(O.gelu_exact((acc + clean["b"] + (cr if cr is not None else 0)).astype(np.float32)))
    else:
        exp = O.epilogue(acc, clean["b"], res=cr, relu=bool(act))
    assert_clean_bits(got, exp, mask, f"linear act {act}")


@pytest.mark.parametrize("rows,D", [(6, 128), (9, 768)])
def test_layernorm_rows_with_a_special_value_are_nan(lib, rows, D):
    rng = np.random.default_rng(rows + D)
    p, x = N.rows_input(rng, rows, D)
    g, b = (1 + 0.1 * rng.standard_normal(D)).astype(np.float32), (0.05 * rng.standard_normal(D)).astype(np.float32)
    y = Guarded((rows, D))
    pd, gd, bd = dev_bits(p), torch.from_numpy(g).cuda(), torch.from_numpy(b).cuda()
    _lib.check(lib.fav_op_layernorm(pd.data_ptr(), D, gd.data_ptr(), bd.data_ptr(), y.ptr, rows, D, C.c_float(1e-6), None))
    torch.cuda.synchronize()
    got = y.value()
    ref = N.layernorm_ref(p)
    assert (ref == N.NAN).any(axis=1).sum() == 4
    assert_classes(got, ref, "layernorm")
    assert_clean_bits(got, O.bf16_round(O.layernorm_exact(x, g, b)), ref == N.FIN, "layernorm")


@pytest.mark.parametrize("mode", [0, 1])
@pytest.mark.parametrize("T", [197, 5])
def test_attention_keeps_the_class(lib, T, mode):
    n, heads = 4, 2
    D = heads * 64
    p, x = N.attention_input(np.random.default_rng(T), n, T, heads)
    ref = N.attention_ref(p, heads)
    clean = N.attention_clean(p, x, heads)
    assert set(np.unique(ref).tolist()) == {N.NAN, N.PINF, N.NINF, N.FIN} and clean.mean() >= 0.5 and (ref[clean] == N.FIN).all()
    out = Guarded((n, T, D))
    pd = dev_bits(p)
    _lib.check(lib.fav_op_attention(pd.data_ptr(), out.ptr, n, T, D, heads, mode, None))
    assert _lib.route_attention(n, T, D, heads, mode) == (0, _lib.last_route())
    torch.cuda.synchronize()
    got = out.value()
    nan_report(got, f"attention T {T} mode {mode}")
    assert_classes(got, ref, f"attention T {T}")
    assert_clean_bits(got, O.attention(x, heads, exact="mfma" if mode == 0 else True), clean, "attention")
    # the repaired oracle agrees on the poisoned input, class by class
    assert_classes(O.attention(p, heads, exact="mfma" if mode == 0 else True), ref, "oracle attention")


def test_vit_assemble_adds_by_ieee(lib):
    rng = np.random.default_rng(9)
    n, ntok, D = 3, 17, 128
    emb = N.finite_bf16(rng, (n, ntok - 1, D))
    pos = (0.2 * rng.standard_normal((ntok, D))).astype(np.float32)
    p = emb.copy()
    for i, kind in enumerate(("+inf", "-inf", "nan", "nan_neg")):
        p[1, 2 + i, 5 * i + 1] = N.special(kind)
    pos_p = pos.copy()
    pos_p[4, 9], pos_p[0, 3] = N.ROUND_BIAS, -N.ROUND_BIAS              # finite fp32 above the bf16 range: +-inf after the one rounding
    x = Guarded((n, ntok, D))
    pd, posd = dev_bits(p), torch.from_numpy(pos_p).cuda()
    _lib.check(lib.fav_op_vit_assemble(pd.data_ptr(), posd.data_ptr(), x.ptr, n, ntok, D, None))
    torch.cuda.synchronize()
    got = x.value()
    full = np.empty((n, ntok, D), np.float64)
    full[:, 0], full[:, 1:] = pos_p[0], p.astype(np.float64) + pos_p[1:]
    ref = N.classes(O.bf16_round(full.astype(np.float32)))
    assert set(np.unique(ref).tolist()) == {N.NAN, N.PINF, N.NINF, N.FIN}
    assert_classes(got, ref, "vit_assemble")
    exp = np.empty((n, ntok, D), np.float32)
    exp[:, 0], exp[:, 1:] = pos[0], emb + pos[1:]
    assert_clean_bits(got, O.bf16_round(exp), ref == N.FIN, "vit_assemble")


# ---------------------------------------------------------------------------------------------------------------------
# handles
# ---------------------------------------------------------------------------------------------------------------------
TWINS = {   # arch: (frame size, the two consecutive layers that get 2^100 each, the layer of the 2^40 twin)
    "resnet18_cifar": (32, (5, 6), 5),           # layer2.0.conv1, layer2.0.conv2
    "resnet50": (64, (11, 12), 11),              # layer2.0.conv1, layer2.0.conv2
    "vit_tiny": (64, (6, 7), 6),                 # block 0: fc1, fc2
}
_BLOBS = {}


def twin(arch, which):
    """-> (blob, model) of a fixture's clean / overflowing / huge twin, made once per session."""
    if (arch, which) not in _BLOBS:
        if (arch, "clean") not in _BLOBS:
            blob = weights.make_synthetic_vit(arch, seed=3)[0] if arch == "vit_tiny" else weights.make_synthetic(arch, seed=1)[0]
            _BLOBS[(arch, "clean")] = (blob, O.parse_blob(blob))
        blob = _BLOBS[(arch, "clean")][0]
        _, (a, b), h = TWINS[arch]
        if which == "overflow":
            blob = N.scale_layer(N.scale_layer(blob, a, 100), b, 100)
        elif which == "huge":
            blob = N.scale_layer(blob, h, 40)
        _BLOBS[(arch, which)] = (blob, O.parse_blob(blob))
    return _BLOBS[(arch, which)]


def blob_accepted(lib, blob):
    buf = (C.c_char * len(blob)).from_buffer_copy(blob)
    return lib.fav_check_blob(buf, len(blob), None, 0) == 0


def assert_rule(be, frames, n_classes, what):
    """Every head's answer on frames that must all be non-finite: the rule of include/fav.h above fav_classify."""
    n = frames.shape[0]
    labels, conf, fail, score = (t.cpu().numpy() for t in be.classify_detect(frames))
    lg = be.logits().cpu().numpy()
    assert lg.shape[-2] == n
    bad = O.nonfinite_frames(lg.reshape(-1, n, lg.shape[-1])[..., :n_classes], float(be.cfg.temperature))
    assert bad.all(), f"{what}: frames {np.flatnonzero(~bad).tolist()} have a finite logit row"
    assert (labels == 0).all() and (conf == 0).all() and (fail == 1).all() and (score == 1).all(), what
    l2, c2 = (t.cpu().numpy() for t in be.classify(frames))
    assert (l2 == 0).all() and (c2 == 0).all()
    u = {k: (v.cpu().numpy() if hasattr(v, "cpu") else v) for k, v in be.classify_uncertainty(frames).items()}
    assert (u["label"] == 0).all() and (u["confidence"] == 0).all() and (u["fail"] == 1).all() and (u["score"] == 1).all(), what
    for k in ("mean_prob", "prob_std", "pred_entropy", "expected_entropy", "mutual_info", "agreement"):
        assert np.isnan(u[k]).all(), f"{what}: {k}"
    assert (u["top_label"] == -1).all() and (u["top_prob"] == 0).all()
    s = {k: (v.cpu().numpy() if hasattr(v, "cpu") else v) for k, v in be.classify_sets(frames, Conformal(kind="aps", randomized=False, qhat=0.9)).items()}
    assert (s["label"] == 0).all() and (s["confidence"] == 0).all() and (s["fail"] == 1).all() and (s["score"] == 1).all(), what
    assert (s["set_size"] == 0).all() and (s["set_mass"] == 0).all() and not s["members"].any() and s["ambiguous"].all()
    return lg


HANDLE_CONFIGS = [
    # arch, math, extra Backend arguments
    ("resnet18_cifar", "bf16", dict()),
    ("resnet18_cifar", "f32_exact", dict()),
    ("resnet18_cifar", "bf16", dict(n_samples=3, dropout_policy="all_blocks", dropout_p=0.1, seed=4, chunk_a=3, chunk_b=5)),
    ("resnet18_cifar", "f32_exact", dict(n_samples=3, dropout_policy="all_blocks", dropout_p=0.1, seed=4, chunk_a=3, chunk_b=5)),
    ("resnet50", "bf16", dict(tail_min_rows=-1)),
    ("resnet50", "bf16", dict(tail_min_rows=1 << 30, stem_fused=-1)),
    ("resnet50", "f32_exact", dict()),
    ("resnet50", "bf16", dict(n_samples=3, dropout_policy="all_blocks", dropout_p=0.1, seed=4, chunk_a=2, chunk_b=3, tail_min_rows=-1)),
    ("vit_tiny", "bf16", dict(vit_streams=1)),
    ("vit_tiny", "bf16", dict(vit_streams=3)),
    ("vit_tiny", "f32_exact", dict()),
]


@pytest.mark.parametrize("arch,math,kw", HANDLE_CONFIGS, ids=[f"{a}-{m}-{'-'.join(f'{k}{v}' for k, v in kw.items()) or 'plain'}" for a, m, kw in HANDLE_CONFIGS])
def test_overflowing_checkpoint_ends_in_the_rule(lib, arch, math, kw):
    hw = TWINS[arch][0]
    blob, model = twin(arch, "overflow")
    assert blob_accepted(lib, blob), "every weight of the twin is finite"
    max_batch = 5
    frames = synth.synthetic_frames_u8(max_batch, hw, hw, seed=11)
    be = Backend(arch, blob, in_hw=(hw, hw), max_batch=max_batch, math_mode=math, **kw)
    try:
        for n in (1, max_batch):
            lg = assert_rule(be, torch.from_numpy(frames[:n]).cuda(), model.num_classes, f"{arch} {math} {kw} n={n}")
            if n == max_batch and not kw.get("n_samples"):
                # the repaired oracle: the same frames are non-finite there, in the mode's own model
                ol, oc, olg, _ = O.classify(model, frames, O.ClassifyConfig(exact="mfma" if math == "bf16" else True), return_logits=True)
                assert O.nonfinite_frames(olg).all() and (ol == 0).all() and (oc == 0).all()
                assert np.array_equal(N.classes(lg.reshape(olg.shape)), N.classes(olg)), "logit classes differ from the oracle"
    finally:
        be.close()


@pytest.mark.parametrize("grouped", [0, -1], ids=["grouped", "member-streams"])
def test_overflowing_ensemble_member_ends_in_the_rule(lib, grouped):
    """A 2-member ensemble whose second member overflows: every frame is non-finite (one sample suffices), grouped and on member streams."""
    clean, _ = twin("resnet18_cifar", "clean")
    bad, model = twin("resnet18_cifar", "overflow")
    frames = synth.synthetic_frames_u8(4, 32, 32, seed=11)
    be = Backend("resnet18_cifar", [clean, bad], max_batch=4, ens_grouped_max=grouped)
    try:
        for n in (1, 4):
            assert_rule(be, torch.from_numpy(frames[:n]).cuda(), model.num_classes, f"ensemble grouped={grouped} n={n}")
    finally:
        be.close()


@pytest.mark.parametrize("arch", list(TWINS))
def test_huge_but_finite_checkpoint_raises_no_alarm(lib, arch):
    """2^40 on one layer: activations of 1e12 and more, finite everywhere.  Bit for bit the MFMA-model oracle, no frame flagged
    as non-finite - the fixes change no finite result and raise no false alarm."""
    hw = TWINS[arch][0]
    blob, model = twin(arch, "huge")
    assert blob_accepted(lib, blob)
    frames = synth.synthetic_frames_u8(3, hw, hw, seed=11)
    be = Backend(arch, blob, in_hw=(hw, hw), max_batch=3)
    try:
        labels, conf, fail, score = (t.cpu().numpy() for t in be.classify_detect(torch.from_numpy(frames).cuda()))
        lg = be.logits().cpu().numpy()
    finally:
        be.close()
    ol, oc, olg, _ = O.classify(model, frames, O.ClassifyConfig(exact="mfma"), return_logits=True)
    assert np.isfinite(olg).all(), "the twin is not finite"
    if arch != "vit_tiny":                                 # (the ViT's last LayerNorm brings the logits back to size)
        assert np.abs(olg).max() > 1e6, "the twin is not huge"
    assert np.array_equal(bits32(lg.reshape(olg.shape)), bits32(olg)), "logits differ from the MFMA-model oracle"
    assert not O.nonfinite_frames(olg).any() and (conf > 0).all() and np.array_equal(labels, ol)
