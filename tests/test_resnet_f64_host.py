"""The ResNet path's oracle against float64 arithmetic that knows nothing of the kernels (tests/resnet_ref.py); no device.

Almost every ResNet assertion of the GPU suite is "bit for bit against oracle/", and oracle/ restates the kernels' rules: the
im2col and padding geometry, the epilogue order, where a bottleneck's stride sits, the max pool's window, the normalisation.  A
mistake made in both places passes there.  This module holds the oracle itself to float64 at the shapes the GPU tests use; it
fixes the bounds tests/test_gpu_resnet_f64.py holds the device to, and shows that the oracle alone stays inside them and that
each bound rejects the plausible mistakes (computed from the same oracle output).

Worst |error| / bound of the oracle, measured here (both accumulation models; the bound and its derivation: resnet_ref.conv_bound):
  a. convolutions   the 16 generic cases 0.986, the 14 threshold cases (halo, proj) 0.985, the 24 geometry cases 0.971 - the
                    bf16 rounding term, attained as it must be (a result half a step from a bf16 value at the bottom of a
                    binade); with fp32 output 0.032 (the fp32 summation term alone: no real order comes near K worst-case
                    roundings); with fused dropout 0.981
  b. controls       the smallest ratio of each to its own bound: ReLU before the residual add 214 x; frame with H and W
                    swapped 4044 x; kh and kw swapped 40302 x; stride 2 on the odd pixels 786 x (the wrong references are
                    unrelated numbers, often near 0 where the bound is tiny); dropout scale 1: 29 x (0.113 / 2^-8 at most)
  c. pools          max pool: equal; mean pool 0.996 at HW = 2, 0.980 at 49, 0.894 at 35 (again the rounding), 0 at HW = 1
  d. networks       resnet_ref.py lists the distances per size"""
import dataclasses
import functools

import numpy as np
import pytest

torch = pytest.importorskip("torch")
from conftest import note  # noqa: E402
from failure_aware_vision_amd import weights  # noqa: E402
from oracle import fav_oracle as O, torch_cpu  # noqa: E402
import resnet_ref as R  # noqa: E402
import test_gpu_conv_routes as RT  # noqa: E402

# ---------------------------------------------------------------------------------------------------------------------------------
# a, b. one convolution launch: every host-drawn case of test_gpu_conv_routes.CASES with a ReLU or no activation (the GELU
# cases belong to test_gpu_vit_f64.py), each under both accumulation models of the oracle whatever mode the case names
# ---------------------------------------------------------------------------------------------------------------------------------
CONV_CASES = [c for c in RT.CASES if not c.device and c.relu != 2]
DROP = dict(site=3, thr=26, seed=0x1234567ABC, v0=3, first=40)       # the fused-dropout arm: virtual frames 3 .. 3 + n of n + 1 frames
#: the cases that also run with a fused dropout site / with fp32 output (tests/test_gpu_resnet_f64.py runs the same on the device)
DROP_CASES = ("generic-bn128-bk64-res-bf16", "generic-bn64-bk32-nores-f32")
F32_OUT_CASES = ("generic-bn128-bk32-nores-bf16", "generic-bn64-bk64-res-f32")


def drop_keep(c):
    """The keep mask [n, Ho * Wo * Cout] of DROP for a case: row r is virtual frame v = v0 + r, sample v // n_img of frame
    first + v % n_img (include/fav.h, fav_dropout_desc), n_img = n + 1."""
    ho, wo = RT.out_hw(c)
    v = DROP["v0"] + np.arange(c.n)
    return np.stack([O.dropout_keep(DROP["seed"], int(t), DROP["site"], np.array([i]), ho * wo * c.cout, DROP["thr"])[0]
                     for t, i in zip(v // (c.n + 1), v % (c.n + 1) + DROP["first"])])


def drop_scale():
    return 1.0 / (1.0 - DROP["thr"] / 256.0)


def conv_variants(c):
    """(tag, keep mask or None, fp32 output?) a case runs under."""
    out = [("", None, False)]
    if c.name in DROP_CASES:
        out.append((" + dropout", drop_keep(c), False))
    if c.name in F32_OUT_CASES:
        out.append((" fp32 out", None, True))
    return out


def conv_reference(c, x, w, b, r, keep, f32_out):
    """-> (float64 result, its bound, the controls)."""
    K = c.kh * c.kw * c.cin
    scale = drop_scale() if keep is not None else 1.0
    ref, mass = R.conv(x, w, b, r, bool(c.relu), keep, scale, c.stride, c.pad)
    return (ref, R.conv_bound(ref, mass, K, not f32_out, scale),
            R.conv_controls(x, w, b, r, bool(c.relu), c.stride, c.pad, keep, scale, not f32_out))


@pytest.mark.parametrize("c", CONV_CASES, ids=[c.name for c in CONV_CASES])
def test_conv_oracle_vs_float64(c):
    x, w, b, r = RT.host_operands(c)
    for tag, keep, f32_out in conv_variants(c):
        ref, bound, controls = conv_reference(c, x, w, b, r, keep, f32_out)
        for mode in ("mfma", True):
            acc = O.conv_acc_exact(x, w, c.kh, c.kw, c.stride, c.pad, mode=mode)
            if f32_out:      # fp32 output: ((acc + bias) + residual), ReLU, no rounding
                out = acc + b if r is None else (acc + b) + r
                out = np.maximum(out, np.float32(0)) if c.relu else out
            else:
                out = O.epilogue(acc, b, res=r, relu=bool(c.relu), keep=keep, scale=np.float32(drop_scale()))
            ratio = R.violation(out, ref, bound)
            what = f"oracle {'MFMA model' if mode == 'mfma' else 'f32 chain'} {c.name}{tag}"
            note(f"{what}: worst |err| / bound {ratio:.3f}")
            assert ratio <= 1.0, what
            R.assert_controls_rejected(out, controls, what, note)


def test_every_control_is_exercised():
    """Each of the five controls applies to some case (a control no case reaches would prove nothing)."""
    seen = set()
    for c in CONV_CASES:
        x, w, b, r = RT.host_operands(c)
        if c.n * c.H * c.W * c.cin * c.cout > 1 << 28:      # the large cases add no kind of control
            continue
        for _, keep, f32_out in conv_variants(c):
            seen |= {name for name, *_ in R.conv_controls(x, w, b, r, bool(c.relu), c.stride, c.pad, keep, drop_scale(), not f32_out)}
    assert seen == {"ReLU before the residual add", "frame with H and W swapped", "kh and kw swapped",
                    "stride 2 on the odd rows and columns", "dropout scale 1"}


# ---------------------------------------------------------------------------------------------------------------------------------
# c. pools
# ---------------------------------------------------------------------------------------------------------------------------------
MAXPOOL_SHAPES = [(2, 1, 1), (2, 2, 2), (2, 1, 37), (2, 37, 1), (1, 15, 9), (1, 33, 47)]       # n, H, W; 64 channels


def maxpool_input(n, H, W, C=64):
    """bf16 values; the 15 x 9 case is negative throughout, so a zero in place of the -inf padding would win every border window."""
    rng = np.random.default_rng(H * 100 + W)
    x = rng.standard_normal((n, H, W, C)) * np.exp2(rng.integers(-3, 4, (n, H, W, C)))
    if (H, W) == (15, 9):
        x = -np.abs(x) - 2.0 ** -10
    return O.bf16_round(x.astype(np.float32))


@pytest.mark.parametrize("n,H,W", MAXPOOL_SHAPES)
def test_maxpool_oracle_equals_float64(n, H, W):
    """A max of bf16 values rounds nothing: equal, not close."""
    x = maxpool_input(n, H, W)
    ref = R.maxpool3x3s2(x).numpy()
    got = O.maxpool3x3s2(x)
    assert got.shape == ref.shape == (n, (H - 1) // 2 + 1, (W - 1) // 2 + 1, 64)
    assert np.array_equal(got.astype(np.float64), ref)
    if (H, W) == (15, 9):
        # negative controls: zero padding, and a window that starts one pixel late (pad 0), are both rejected
        assert (ref < 0).all()
        xt = torch.from_numpy(x).double().permute(0, 3, 1, 2)
        zero_pad = torch.nn.functional.max_pool2d(torch.nn.functional.pad(xt, (1, 1, 1, 1)), 3, 2, 0).permute(0, 2, 3, 1).numpy()
        assert not np.array_equal(got, zero_pad)
        late = torch.nn.functional.max_pool2d(xt, 3, 2, 0).permute(0, 2, 3, 1).numpy()
        assert not np.array_equal(got[:, :late.shape[1], :late.shape[2]], late)


AVGPOOL_HW = [(1, 1), (1, 2), (7, 7), (5, 7)]        # HW 1, 2, 49, 35


def avgpool_input(H, W, n=3, C=128):
    rng = np.random.default_rng(H * 10 + W)
    return O.bf16_round(np.maximum(rng.standard_normal((n, H, W, C)) * np.exp2(rng.integers(-2, 3, (n, H, W, C))), -0.3).astype(np.float32))


def avgpool_bound(x, ref):
    """HW 2^-24 mean|x| + 2^-8 |ref|.  HW - 1 fp32 additions of partial sums that never exceed sum|x| = HW mean|x|, each rounded by
    2^-24 relative, then divided by HW: (HW - 1) 2^-24 mean|x|; the product with fp32(1 / HW) rounds twice more (<= 2^-23 |ref|);
    one rounding to bf16, 2^-8 |ref|.  A worst-case count is thus (HW + 1) 2^-24 mean|x|; the bound is held one unit tighter,
    which bf16 addends permit: 8 significant bits each, so the first additions of a sum are exact in fp32 (all of them for
    avgpool_input's magnitudes, 2^-2 .. 2^2 at HW <= 49), and at HW <= 2 the factor 1 or 1/2 is exact too."""
    x = R.f64(x)
    hw = x.shape[1] * x.shape[2]
    return hw * 2.0 ** -24 * x.abs().reshape(x.shape[0], hw, -1).mean(1) + 2.0 ** -8 * ref.abs() + 1e-30


@pytest.mark.parametrize("H,W", AVGPOOL_HW)
def test_avgpool_oracle_vs_float64(H, W):
    x = avgpool_input(H, W)
    ref = R.avgpool(x)
    got = O.bf16_round(O.global_avgpool(x))
    ratio = R.violation(got, ref, avgpool_bound(x, ref))
    note(f"oracle mean pool {H}x{W}: worst |err| / bound {ratio:.3f}")
    assert ratio <= 1.0
    if H * W > 1:
        # negative controls: a sum that is not divided, and a mean over one pixel too few
        assert R.violation(got, ref * (H * W), avgpool_bound(x, ref * (H * W))) > R.CONTROL_FACTOR
        short = R.f64(x).reshape(3, H * W, -1)[:, :-1].sum(1) / (H * W)
        assert R.violation(got, short, avgpool_bound(x, short)) > R.CONTROL_FACTOR


# ---------------------------------------------------------------------------------------------------------------------------------
# d. whole networks
# ---------------------------------------------------------------------------------------------------------------------------------
E2E_CASES = [(a, hw, False) for a in R.E2E_SIZES for hw in R.E2E_SIZES[a]] + [(a, R.MC_CASES[a], True) for a in R.MC_CASES]
METRICS = ("rel_rms", "max_abs", "conf", "entropy")


@functools.lru_cache(maxsize=None)
def model_of(arch):
    model = O.parse_blob(R.checkpoint(arch)[1])
    return model, torch_cpu.TorchNet(model)


def oracle_config(arch, mc):
    if not mc:
        return O.ClassifyConfig()
    return O.ClassifyConfig(n_samples=R.MC["n_samples"], site_mask=weights.site_mask_for(R.ARCH_ID[arch], R.MC["dropout_policy"]),
                            p=R.MC["dropout_p"], seed=R.MC["seed"])


def check_e2e(what, lg, labels, ref, arch):
    """The assertions tests/test_gpu_resnet_f64.py shares: logits [T, n, C] inside E2E_BOUND, labels equal where the float64
    top-2 gap is clear (and at least half of the frames are), every control outside the bound."""
    bound = R.E2E_BOUND[arch]
    d = R.distance(lg, ref["logits"])
    hd = R.head_of_samples(ref["logits"])
    clear = hd["gap"] > R.E2E_GAP
    ctl = {k: R.distance(lg, v)["rel_rms"] for k, v in ref["controls"].items()}
    note(f"{what} vs float64: " + ", ".join(f"{k} {d[k]:.5f} (bound {bound[k]:.4f})" for k in METRICS)
         + f"; labels {int((np.asarray(labels) == hd['label']).sum())} / {len(clear)} ({int(clear.sum())} clear); controls (rel. RMS): "
         + ", ".join(f"{k} {v:.3f}" for k, v in ctl.items()))
    for k in METRICS:
        assert d[k] <= bound[k], (what, k, d[k])
    assert 2 * clear.sum() >= len(clear), f"{what}: fewer than half of the frames have a clear float64 label"
    assert np.array_equal(np.asarray(labels)[clear], hd["label"][clear]), what
    for k, v in ctl.items():
        assert v > bound["rel_rms"], f"{what}: the bound does not reject '{k}'"
    return d


@pytest.mark.parametrize("arch,hw,mc", E2E_CASES, ids=[f"{a}-{h}x{w}{'-mc' if mc else ''}" for a, (h, w), mc in E2E_CASES])
def test_network_oracle_vs_float64(arch, hw, mc):
    model, port_net = model_of(arch)
    cfg = oracle_config(arch, mc)
    for first in (R.MC_FIRST if mc else (0,)):
        ref = R.reference(arch, hw, mc=mc, first_index=first)
        ids = first + np.arange(R.N_FRAMES)
        case = f"{arch} {hw[0]}x{hw[1]}" + (f" all_blocks T=3 first_index {first}" if mc else "")
        # the bf16 contract's own distance: the torch CPU port, none of the device's or the MFMA model's arithmetic.  What it
        # measures here is printed beside the recorded figure; the order of torch's CPU convolution changes with the thread count
        # and moves it by a few per cent (one thread: max_abs 0.1303 where eight give 0.1292) - the very effect the factor 2 is
        # for - so the port is held to the bound like everything else, not to the recorded figure
        port = torch_cpu.classify(model, ref["frames"], cfg, img_ids=ids, return_logits=True, net=port_net)[2]
        d = R.distance(port, ref["logits"])
        note(f"{case} torch CPU port vs float64: " + ", ".join(f"{k} {d[k]:.5f} (recorded max {R.CONTRACT_DISTANCE[arch][k]})" for k in METRICS))
        for k in METRICS:
            assert d[k] <= R.E2E_BOUND[arch][k], f"{k}: the CPU port of the contract lies outside the bound"
        for exact in ("mfma", True):
            labels, _, lg, _ = O.classify(model, ref["frames"], dataclasses.replace(cfg, exact=exact), img_ids=ids, return_logits=True)
            check_e2e(f"{case} oracle {'MFMA model' if exact == 'mfma' else 'f32 chain'}", lg, labels, ref, arch)


def test_reference_checkpoint_is_the_suite_s_checkpoint(r18_blob):
    """resnet_ref.checkpoint folds the same state_dict the float64 network loads; the blob is weights.make_synthetic's."""
    assert R.checkpoint("resnet18_cifar")[1] == r18_blob[0]


def test_recorded_bounds_are_twice_the_recorded_distances():
    for arch, d in R.CONTRACT_DISTANCE.items():
        assert R.E2E_BOUND[arch] == {k: 2.0 * v for k, v in d.items()}


def test_mc_reference_draws_masks_by_global_frame_index():
    """The float64 MC-Dropout pass: samples differ, and frame i at first_index 7 draws what frame i + 7 - k draws at first_index
    k (the masks are keyed by first_index + i, include/fav.h)."""
    arch, hw = "resnet18_cifar", R.MC_CASES["resnet18_cifar"]
    a = R.reference(arch, hw, mc=True, first_index=0)["logits"]
    b = R.reference(arch, hw, mc=True, first_index=7)["logits"]
    assert a.shape == (3, R.N_FRAMES, 10) and not np.allclose(a[0], a[1]) and not np.allclose(a, b)
    net, _ = R.checkpoint(arch)
    xn = R.normalize(R.frames_of(hw), R.MEAN, R.STD)
    kw = dict(site_mask=weights.site_mask_for(0, "all_blocks"), p=0.1, n_samples=3, seed=4)
    one = R.logits(net, xn[2:3], first_index=9, **kw).numpy()          # frame 2 alone, as global frame 9 = 7 + 2
    assert np.allclose(one[:, 0], b[:, 2], rtol=0, atol=1e-9)
