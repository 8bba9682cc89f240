"""The ResNet path on the device against float64 arithmetic that knows nothing of the kernels (tests/resnet_ref.py).

The other ResNet tests compare the device with oracle/ bit for bit, and oracle/ shares the kernels' rules (im2col and padding
geometry, epilogue order, stride placement, pool window, normalisation): a mistake made in both places passes there.  Here every
assertion compares the device with float64 written from the definitions: whole networks through Backend at odd sizes and at
224 x 224, and fav_op_conv2d, fav_op_bottleneck_tail, fav_op_stem_pool, fav_op_entry_reduce and the two pools one launch at a
time.  Every bound is derived in a comment (here or in resnet_ref.py) or measured on the CPU against the float64 reference
(resnet_ref.E2E_BOUND; tests/test_resnet_f64_host.py holds the oracle to the same bounds without a device) - none is tuned to
what the device gives - and every test shows that its bound rejects plausibly wrong references computed from the same device
output.  The float64 references run on the CPU; at these sizes each takes well under a second."""
import ctypes as C

import numpy as np
import pytest

pytestmark = pytest.mark.gpu

torch = pytest.importorskip("torch")
from conftest import note  # noqa: E402
from failure_aware_vision_amd import Backend, _lib  # noqa: E402
import resnet_ref as R  # noqa: E402
import test_gpu_conv_routes as RT  # noqa: E402
import test_gpu_tail as TT  # noqa: E402
from test_gpu_ops import ENTRY_REDUCE_ROUTE, dev_bf16, drop_desc  # noqa: E402
from test_gpu_exact import STEM_POOL_ROUTES  # noqa: E402
from test_gpu_pool_dropout_edges import Guarded  # noqa: E402
from test_resnet_f64_host import (AVGPOOL_HW, CONV_CASES, DROP, MAXPOOL_SHAPES, avgpool_bound, avgpool_input, check_e2e,  # noqa: E402
                                  conv_reference, conv_variants, drop_scale, maxpool_input)

F = torch.nn.functional


@pytest.fixture(scope="module")
def lib():
    assert torch.cuda.is_available(), "GPU tests need a MI355X"
    return _lib.load()


# ---------------------------------------------------------------------------------------------------------------------------------
# a. whole networks through Backend
# ---------------------------------------------------------------------------------------------------------------------------------
NET_CASES = ([(a, hw, False) for a in R.E2E_SIZES for hw in R.E2E_SIZES[a]] + [("resnet50", (224, 224), False)]
             + [(a, R.MC_CASES[a], True) for a in R.MC_CASES])


@pytest.fixture(scope="module")
def handles():
    """One handle per (arch, size, math mode, MC-Dropout or not), made on first use, closed with the module."""
    made = {}

    def get(arch, hw, math_mode, mc):
        key = (arch, hw, math_mode, mc)
        if key not in made:
            n = 2 if hw == (224, 224) else R.N_FRAMES
            made[key] = Backend(arch, R.checkpoint(arch)[1], in_hw=hw, max_batch=n, math_mode=math_mode, **(R.MC if mc else {}))
        return made[key]
    yield get
    for be in made.values():
        be.close()


@pytest.mark.parametrize("math_mode", ["bf16", "f32_exact"])
@pytest.mark.parametrize("arch,hw,mc", NET_CASES, ids=[f"{a}-{h}x{w}{'-mc' if mc else ''}" for a, (h, w), mc in NET_CASES])
def test_network_vs_float64(handles, arch, hw, mc, math_mode):
    """Logits, labels, confidences and classify_uncertainty's pred_entropy under resnet_ref.E2E_BOUND (twice the distance of the
    bf16 contract's CPU port from float64), for uint8 and fp32 frames; the MC-Dropout cases at first_index 0 and 7.  The three
    negative controls (frames with H and W swapped, ceil-mode max pool, stride on the 1x1) are applied to the device's logits
    inside check_e2e."""
    be = handles(arch, hw, math_mode, mc)
    n = 2 if hw == (224, 224) else R.N_FRAMES
    bound = R.E2E_BOUND[arch]
    for layout in ("u8", "f32"):
        for first in (R.MC_FIRST if mc else (0,)):
            ref = R.reference(arch, hw, n, layout, mc, first)
            x = torch.from_numpy(ref["frames"]).cuda()
            labels, conf = be.classify(x, first_index=first)
            lg = be.logits().cpu().numpy().astype(np.float64)
            assert lg.shape == ref["logits"].shape
            what = f"{arch} {hw[0]}x{hw[1]} {math_mode} {layout}" + (f" all_blocks T=3 first_index {first}" if mc else "")
            check_e2e(what, lg, labels.cpu().numpy(), ref, arch)
            hd = R.head_of_samples(ref["logits"])
            clear = hd["gap"] > R.E2E_GAP
            conf_err = np.abs(conf.cpu().numpy().astype(np.float64) - hd["pbar"].max(1)).max()
            unc = be.classify_uncertainty(x, first_index=first)
            ent_err = np.abs(unc["pred_entropy"].cpu().numpy().astype(np.float64) - hd["entropy"]).max()
            note(f"{what} device head vs float64: confidence {conf_err:.5f} (bound {bound['conf']:.4f}), pred_entropy {ent_err:.5f} "
                 f"nats (bound {bound['entropy']:.4f})")
            assert conf_err <= bound["conf"]
            assert ent_err <= bound["entropy"]
            assert np.array_equal(unc["label"].cpu().numpy()[clear], hd["label"][clear])


# ---------------------------------------------------------------------------------------------------------------------------------
# b. fav_op_conv2d: the cases, the bound and the controls of tests/test_resnet_f64_host.py (a, b), on the route each case must take
# ---------------------------------------------------------------------------------------------------------------------------------
def conv_drop_desc(c):
    return drop_desc(DROP["site"], DROP["thr"], drop_scale(), DROP["seed"], DROP["v0"], c.n + 1, DROP["first"])


def launch_conv(lib, c, dev, with_drop, f32_out):
    """One fav_op_conv2d of a case between guard bands -> the output [n, Ho, Wo, Cout] as a float64 CPU tensor."""
    xd, wd, bd, rd = dev
    ho, wo = RT.out_hw(c)
    count = c.n * ho * wo * c.cout
    dtype = torch.float32 if f32_out else torch.bfloat16
    esz = 4 if f32_out else 2
    ybig = torch.full((count + 2 * RT.GUARD,), RT.GUARD_VALUE, dtype=dtype, device="cuda")
    d = _lib.FavConvDesc(xd.data_ptr(), wd.data_ptr(), bd.data_ptr(), rd.data_ptr() if rd is not None else None,
                         ybig.data_ptr() + esz * RT.GUARD, c.n, c.H, c.W, c.cin, c.cout, c.kh, c.kw, c.stride, c.pad, c.relu,
                         int(f32_out), c.mode, conv_drop_desc(c) if with_drop else drop_desc())
    _lib.check(lib.fav_op_conv2d(C.byref(d), None))
    route = _lib.last_route()
    torch.cuda.synchronize()
    assert route == c.route          # neither a dropout site nor fp32 output moves a generic case to another kernel
    assert bool((ybig[:RT.GUARD] == RT.GUARD_VALUE).all()) and bool((ybig[-RT.GUARD:] == RT.GUARD_VALUE).all()), "wrote outside the output"
    return ybig[RT.GUARD:-RT.GUARD].reshape(c.n, ho, wo, c.cout).double().cpu()


@pytest.mark.parametrize("c", CONV_CASES, ids=[c.name for c in CONV_CASES])
def test_conv2d_vs_float64(lib, c):
    (x, w, b, r), dev, _ = RT.operands(c)
    for tag, keep, f32_out in conv_variants(c):
        ref, bound, controls = conv_reference(c, x, w, b, r, keep, f32_out)
        out = launch_conv(lib, c, dev, keep is not None, f32_out)
        ratio = R.violation(out, ref, bound)
        what = f"fav_op_conv2d {c.name}{tag}"
        note(f"{what}: worst |err| / bound {ratio:.3f}")
        assert ratio <= 1.0, what
        if keep is not None:
            assert bool(((out == 0) | torch.from_numpy(keep).reshape(out.shape)).all()), "a dropped element is not 0"
        R.assert_controls_rejected(out, controls, what, note)


# ---------------------------------------------------------------------------------------------------------------------------------
# c. fav_op_bottleneck_tail
# ---------------------------------------------------------------------------------------------------------------------------------
# Y = dropout(relu(conv_c(t2) + bias_c + res)), t2 = relu(conv_b(x) + bias_b), in float64 with no rounding in between.  The device
# rounds t2 to bf16, so its conv_c sums t2 + e with |e| <= E = 2^-8 |t2| + Kb 2^-24 mass_b + tiny (conv_b's own bound; the ReLU is
# 1-Lipschitz).  That moves conv_c's sum by at most sum E |wc| = 2^-8 sum |t2| |wc| + sum (Kb 2^-24 mass_b + tiny) |wc|: the
# upstream rounding.  conv_c's own fp32 summation adds Kc 2^-24 (sum |t2 + e| |wc| + |bias_c| + |res|) <= Kc 2^-24 (1 + 2^-7)
# mass_c, the dropout scale multiplies all of that (and adds its product's 2^-24 |Y|), and the one rounding of Y adds 2^-8 |Y|:
#     |Y_dev - Y| <= 2^-8 |Y| + scale (2^-8 sum |t2| |wc| + sum (Kb 2^-24 mass_b + tiny) |wc| + Kc 2^-24 (1 + 2^-7) mass_c) + 2^-24 |Y| + tiny
# Without the 3x3 (wb == NULL) x is conv_c's input as it is and the bound is resnet_ref.conv_bound.
# t1' = relu(conv_a(Y) + bias_a) is computed in float64 from the DEVICE's Y (teacher-forced), so it has one rounding point and
# resnet_ref.conv_bound holds as for a single launch.
TAIL_CASES = [c[:6] for c in TT.CASES if c[5] * c[3] * c[4] <= 8000]


def tail_reference(x, wb, bb, wc, bc, res, keep, scale, relu_b=True, relu_first=False):
    """-> (Y in float64, its bound); relu_b = False and relu_first = True are the negative controls."""
    cmid = x.shape[-1]
    if wb is None:
        y, mass = R.conv(x, wc, bc, res, True, keep, scale, relu_first=relu_first)
        return y, R.conv_bound(y, mass, cmid, True, scale)
    t2, mass_b = R.conv(x, wb, bb, None, relu_b, pad=1)
    e_fp32 = 9 * cmid * 2.0 ** -24 * mass_b + R.CONV_TINY
    wca = R.f64(wc).abs()
    y, mass_c = R.conv(t2, wc, bc, res, True, keep, scale, relu_first=relu_first)
    up = 2.0 ** -8 * R.conv_sum(t2.abs(), wca)[0] + R.conv_sum(e_fp32, wca)[0]
    return y, 2.0 ** -8 * y.abs() + scale * (up + cmid * 2.0 ** -24 * (1 + 2.0 ** -7) * mass_c) + 2.0 ** -24 * y.abs() + R.CONV_TINY


def check_tail(what, y, t1n, ops, keep, log=note):
    """y, t1n: the launch's outputs (fp32 arrays of bf16 values); ops: TT.tail_operands; keep: the mask [n, H*W*4*Cmid] or None."""
    x, wb, bb, wc, bc, res, wa, ba = ops
    scale = 1.0 / (1.0 - TT.TAIL_DROP["thr"] / 256.0) if keep is not None else 1.0
    ref, bound = tail_reference(x, wb, bb, wc, bc, res, keep, scale)
    ratio = R.violation(y, ref, bound)
    log(f"{what}: Y worst |err| / bound {ratio:.3f}")
    assert ratio <= 1.0, what
    if keep is not None:
        assert not y[~keep.reshape(y.shape)].any(), "a dropped element is not 0"
    controls = [("the residual added after the ReLU", dict(relu_first=True))] + ([("conv_b without its ReLU", dict(relu_b=False))] if wb is not None else [])
    for name, kw in controls:
        wrong, wbound = tail_reference(x, wb, bb, wc, bc, res, keep, scale, **kw)
        r = R.violation(y, wrong, wbound)
        log(f"{what}: control '{name}' at {r:.1f} x its bound")
        assert r >= R.CONTROL_FACTOR, f"{what}: the bound does not reject '{name}'"
    if wa is not None:
        t1, mass = R.conv(y, wa, ba, None, True)
        tb = R.conv_bound(t1, mass, wa.shape[-1])
        ratio = R.violation(t1n, t1, tb)
        log(f"{what}: t1' (teacher-forced) worst |err| / bound {ratio:.3f}")
        assert ratio <= 1.0, what
        wrong, mass = R.conv(y, wa, ba, None, False)                      # control: the reduce without its ReLU
        assert R.violation(t1n, wrong, R.conv_bound(wrong, mass, wa.shape[-1])) >= R.CONTROL_FACTOR


@pytest.mark.parametrize("cmid,nred,has3x3,H,W,n", TAIL_CASES)
@pytest.mark.parametrize("with_drop", [False, True])
def test_bottleneck_tail_vs_float64(lib, cmid, nred, has3x3, H, W, n, with_drop):
    ops = TT.tail_operands(cmid, nred, has3x3, H, W, n)
    y, t1n = TT.run_tail(lib, *ops, drop=TT.tail_drop_desc(n) if with_drop else None)
    assert _lib.last_route() == TT.ROUTE_OF[(cmid, nred, has3x3, H, W, n)]
    keep = TT.tail_keep(n, H * W * 4 * cmid) if with_drop else None
    check_tail(f"tail cmid {cmid} nred {nred} {'3x3' if has3x3 else '1x1'} {n}x{H}x{W}{' + dropout' if with_drop else ''}", y, t1n, ops, keep)


# ---------------------------------------------------------------------------------------------------------------------------------
# d. fav_op_stem_pool
# ---------------------------------------------------------------------------------------------------------------------------------
# out = maxpool3x3s2(relu(conv7x7s2p3(xn, w) + bias)), xn = (pixel - mean) / std, in float64.  Per convolution element:
#   - the device rounds xn to bf16 before the convolution: 2^-8 sum |xn| |w|;
#   - it computes xn in fp32 (uint8: pixel x fp32(1/255); minus mean; times fp32(1 / fp32(std))): six roundings of 2^-24 relative,
#     each of a magnitude <= (|pixel| + |mean|) / std, and x - mean may cancel, so the term is 6 2^-24 sum ((|pixel| + |mean|) / std) |w|;
#   - the fp32 summation, K = 147 products and the bias: K 2^-24 (1 + 2^-7) mass;
#   - the one rounding of the result, 2^-8 |ref|; the ReLU is 1-Lipschitz.
# The max pool is 1-Lipschitz in the max norm of its window and rounds nothing, so a pooled element's bound is the largest bound
# in its window (a max pool of the bounds over the same windows).
STEM_SHAPES = [(2, 224, 224), (3, 64, 80), (1, 33, 47), (5, 9, 7), (1, 8, 225)]


def stem_operands(layout, n, H, W):
    rng = np.random.default_rng(H * 1000 + W + n)
    img = rng.integers(0, 256, (n, H, W, 3), dtype=np.uint8) if layout == 0 else rng.random((n, H, W, 3), dtype=np.float32)
    w = torch.from_numpy((rng.standard_normal((64, 7, 7, 3)) * np.sqrt(2.0 / 147)).astype(np.float32)).to(torch.bfloat16).float().numpy()
    b = (rng.standard_normal(64) * 0.2).astype(np.float32)
    return img, w, b


def stem_reference(img, w, b, divide_std=True, pool_pad=1):
    """-> (pooled float64 result, its bound); divide_std = False and pool_pad = 0 (a window that starts one pixel late) are the
    negative controls."""
    x01 = R.f64(img) / 255.0 if img.dtype == np.uint8 else R.f64(img)
    mean, std = torch.tensor(R.MEAN, dtype=torch.float64), torch.tensor(R.STD, dtype=torch.float64)
    xn = (x01 - mean) / std if divide_std else x01 - mean
    ref, mass = R.conv(xn, w, b, None, True, stride=2, pad=3)
    wabs = R.f64(w).abs()
    bound = (2.0 ** -8 * ref.abs() + 2.0 ** -8 * R.conv_sum(xn.abs(), wabs, 2, 3)[0]
             + 6 * 2.0 ** -24 * R.conv_sum((x01.abs() + mean) / std, wabs, 2, 3)[0] + 147 * 2.0 ** -24 * (1 + 2.0 ** -7) * mass + R.CONV_TINY)
    pool = lambda t: F.max_pool2d(t.permute(0, 3, 1, 2), 3, 2, pool_pad).permute(0, 2, 3, 1)
    return pool(ref), pool(bound)


def check_stem(what, out, img, w, b, log=note):
    """out: the launch's output [n, Hp, Wp, 64] (fp32 array of bf16 values)."""
    ref, bound = stem_reference(img, w, b)
    assert tuple(out.shape) == tuple(ref.shape)
    ratio = R.violation(out, ref, bound)
    log(f"{what}: worst |err| / bound {ratio:.3f}")
    assert ratio <= 1.0, what
    for name, kw in (("mean subtracted, std not divided", dict(divide_std=False)), ("pool window one pixel late", dict(pool_pad=0))):
        wrong, wbound = stem_reference(img, w, b, **kw)
        h, ww = wrong.shape[1], wrong.shape[2]
        if h == 0 or ww == 0:          # frames so small that the late window has no output
            continue
        r = R.violation(R.f64(out)[:, :h, :ww], wrong, wbound)
        log(f"{what}: control '{name}' at {r:.1f} x its bound")
        assert r >= R.CONTROL_FACTOR, f"{what}: the bound does not reject '{name}'"


@pytest.mark.parametrize("layout", [0, 1])
@pytest.mark.parametrize("n,H,W", STEM_SHAPES)
def test_stem_pool_vs_float64(lib, layout, n, H, W):
    img, w, b = stem_operands(layout, n, H, W)
    hc, wc = (H - 1) // 2 + 1, (W - 1) // 2 + 1
    out = Guarded((n, (hc - 1) // 2 + 1, (wc - 1) // 2 + 1, 64))
    wp = np.zeros((64, 192), np.float32)
    wp[:, :147] = w.reshape(64, 147)                   # k = (r * 7 + s) * 3 + c, zero for k >= 147 (include/fav.h)
    wd, bd, imgd = dev_bf16(wp), torch.from_numpy(b).cuda(), torch.from_numpy(img).cuda()
    m3 = (C.c_float * 3)(*R.MEAN)
    i3 = (C.c_float * 3)(*[float(np.float32(1.0) / np.float32(s)) for s in R.STD])
    _lib.check(lib.fav_op_stem_pool(imgd.data_ptr(), layout, n, H, W, wd.data_ptr(), bd.data_ptr(), m3, i3, out.ptr, None))
    assert _lib.last_route() == STEM_POOL_ROUTES[layout]
    torch.cuda.synchronize()
    check_stem(f"fav_op_stem_pool {'u8' if layout == 0 else 'f32'} {n}x{H}x{W}", out.value(), img, w, b)


# ---------------------------------------------------------------------------------------------------------------------------------
# e. fav_op_entry_reduce
# ---------------------------------------------------------------------------------------------------------------------------------
# y[r] = x[v % n_img] / (1 - thr / 256) where kept, 0 where dropped (v = v0 + r: sample v // n_img of frame first + v % n_img), after
# one rounding: the device multiplies by fp32(1 / (1 - thr / 256)) in fp32 (two roundings of 2^-24 relative) and rounds to bf16,
# |y_dev - y| <= (2^-8 + 2^-23) |y|, and a dropped element is exactly 0.  t1 = relu(conv1x1(y_dev) + bias) from the device's own y.
ENTRY_CASES = [(3, 7, 9, 2, 7), (9, 5, 3, 4, 1)]     # n_img, H, W, v0, n_out
ENTRY = dict(site=1, p=0.1, seed=77, first=40)


def entry_operands(n_img, H, W, v0):
    rng = np.random.default_rng(n_img * 100 + H + v0)
    bf = lambda a: torch.from_numpy(a.astype(np.float32)).to(torch.bfloat16).float().numpy()
    x = bf(np.maximum(rng.standard_normal((n_img, H, W, 256)) * np.exp2(rng.integers(-2, 3, (n_img, H, W, 256))), -0.1))
    wa = bf(rng.standard_normal((64, 1, 1, 256)) * np.sqrt(2.0 / 256))
    ba = (rng.standard_normal(64) * 0.2).astype(np.float32)
    return x, wa, ba


def entry_reference(x, v0, n_out, thr, scale, first=ENTRY["first"]):
    n_img = x.shape[0]
    v = v0 + np.arange(n_out)
    keep = np.stack([R.dropout_keep(ENTRY["seed"], int(t), ENTRY["site"], np.array([first + i]), x[0].size, thr)[0]
                     for t, i in zip(v // n_img, v % n_img)]).reshape((n_out,) + x.shape[1:])
    return R.f64(x[v % n_img]) * torch.from_numpy(keep) * scale, keep


def check_entry(what, y, t1, x, wa, ba, v0, log=note):
    thr = R.dropout_threshold(ENTRY["p"])
    ref, keep = entry_reference(x, v0, y.shape[0], thr, 1.0 / (1.0 - thr / 256.0))
    bound = lambda r: (2.0 ** -8 + 2.0 ** -23) * r.abs() + 1e-30
    ratio = R.violation(y, ref, bound(ref))
    log(f"{what}: y worst |err| / bound {ratio:.3f}; kept {keep.mean():.3f} of the elements")
    assert ratio <= 1.0, what
    assert not y[~keep].any(), "a dropped element is not 0"
    # controls: a scale of 1; the masks drawn without first_image_index
    wrong = entry_reference(x, v0, y.shape[0], thr, 1.0)[0]
    assert R.violation(y, wrong, bound(wrong)) >= R.CONTROL_FACTOR
    wrong = entry_reference(x, v0, y.shape[0], thr, 1.0 / (1.0 - thr / 256.0), first=0)[0]
    assert R.violation(y, wrong, bound(wrong)) >= R.CONTROL_FACTOR
    t1ref, mass = R.conv(y, wa, ba, None, True)
    ratio = R.violation(t1, t1ref, R.conv_bound(t1ref, mass, 256))
    log(f"{what}: t1 (teacher-forced) worst |err| / bound {ratio:.3f}")
    assert ratio <= 1.0, what
    wrong, mass = R.conv(y, wa, ba, None, False)                          # control: the reduce without its ReLU
    assert R.violation(t1, wrong, R.conv_bound(wrong, mass, 256)) >= R.CONTROL_FACTOR


@pytest.mark.parametrize("n_img,H,W,v0,n_out", ENTRY_CASES)
def test_entry_reduce_vs_float64(lib, n_img, H, W, v0, n_out):
    x, wa, ba = entry_operands(n_img, H, W, v0)
    thr = R.dropout_threshold(ENTRY["p"])
    d = drop_desc(ENTRY["site"], thr, 1.0 / (1.0 - thr / 256.0), ENTRY["seed"], v0, n_img, ENTRY["first"])
    xd, wd, bd = dev_bf16(x), dev_bf16(wa), torch.from_numpy(ba).cuda()
    y, t1 = Guarded((n_out, H, W, 256)), Guarded((n_out, H, W, 64))
    _lib.check(lib.fav_op_entry_reduce(xd.data_ptr(), y.ptr, wd.data_ptr(), bd.data_ptr(), t1.ptr, 256, 64, H * W, n_out, C.byref(d), None))
    assert _lib.last_route() == ENTRY_REDUCE_ROUTE
    torch.cuda.synchronize()
    check_entry(f"fav_op_entry_reduce {n_img} frames {H}x{W} v0 {v0} rows {n_out}", y.value(), t1.value(), x, wa, ba, v0)


# ---------------------------------------------------------------------------------------------------------------------------------
# f. the pools
# ---------------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("n,H,W", MAXPOOL_SHAPES)
def test_maxpool_equals_float64(lib, n, H, W):
    """A max of bf16 values rounds nothing: equal.  The 15 x 9 case is negative throughout: zero padding would show."""
    x = maxpool_input(n, H, W)
    ref = R.maxpool3x3s2(x).numpy()
    out = Guarded(ref.shape)
    _lib.check(lib.fav_op_maxpool3x3s2(dev_bf16(x).data_ptr(), out.ptr, n, H, W, 64, None))
    torch.cuda.synchronize()
    got = out.value().astype(np.float64)
    assert np.array_equal(got, ref)
    if (H, W) == (15, 9):
        xt = torch.from_numpy(x).double().permute(0, 3, 1, 2)
        assert not np.array_equal(got, F.max_pool2d(F.pad(xt, (1, 1, 1, 1)), 3, 2, 0).permute(0, 2, 3, 1).numpy())     # zero padding
        late = F.max_pool2d(xt, 3, 2, 0).permute(0, 2, 3, 1).numpy()                                                  # one pixel late
        assert not np.array_equal(got[:, :late.shape[1], :late.shape[2]], late)


@pytest.mark.parametrize("H,W", AVGPOOL_HW)
def test_avgpool_vs_float64(lib, H, W):
    """The mean pool under test_resnet_f64_host.avgpool_bound, then its dropout arm with the masks as inputs: a kept element is the
    mean times 1 / (1 - thr / 256) (the bound scales with it, plus the product's 2^-24), a dropped one exactly 0."""
    x = avgpool_input(H, W)
    n, Cc = x.shape[0], x.shape[-1]
    ref = R.avgpool(x)
    xd = dev_bf16(x)
    out = Guarded((n, Cc))
    _lib.check(lib.fav_op_avgpool(xd.data_ptr(), out.ptr, n, H * W, Cc, None, None))
    torch.cuda.synchronize()
    got = out.value()
    ratio = R.violation(got, ref, avgpool_bound(x, ref))
    if H * W > 1:
        assert R.violation(got, ref * (H * W), avgpool_bound(x, ref * (H * W))) > R.CONTROL_FACTOR            # control: not divided
        short = R.f64(x).reshape(n, H * W, -1)[:, :-1].sum(1) / (H * W)
        assert R.violation(got, short, avgpool_bound(x, short)) > R.CONTROL_FACTOR                            # control: one pixel short
    thr, seed, site, v0, first = 128, 77, 16, 2, 40
    scale = 1.0 / (1.0 - thr / 256.0)
    v = v0 + np.arange(n)
    keep = np.stack([R.dropout_keep(seed, int(t), site, np.array([first + i]), Cc, thr)[0] for t, i in zip(v // n, v % n)])
    d = drop_desc(site, thr, scale, seed, v0, n, first)
    out2 = Guarded((n, Cc))
    _lib.check(lib.fav_op_avgpool(xd.data_ptr(), out2.ptr, n, H * W, Cc, C.byref(d), None))
    torch.cuda.synchronize()
    got2 = out2.value()
    dref = ref * torch.from_numpy(keep) * scale
    dbound = lambda r: scale * avgpool_bound(x, r / scale) + 2.0 ** -24 * r.abs()
    dratio = R.violation(got2, dref, dbound(dref))
    note(f"fav_op_avgpool {H}x{W}: worst |err| / bound {ratio:.3f}; with dropout {dratio:.3f}, kept {keep.mean():.3f}")
    assert ratio <= 1.0 and dratio <= 1.0
    assert not got2[~keep].any(), "a dropped element is not 0"
    wrong = ref * torch.from_numpy(keep)                                                                      # control: a scale of 1
    assert R.violation(got2, wrong, avgpool_bound(x, wrong)) > R.CONTROL_FACTOR
