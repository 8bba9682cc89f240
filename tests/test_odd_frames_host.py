"""Odd frame sizes, asked of the planner alone (no device): fav_create takes any in_h, in_w >= 8 for the two ResNet
architectures, and everything between the plan and the kernels - the walk that chains conv_out, the arenas sized from it, the
map geometry fav_map_tap_info reports - sees whatever size the caller has.

  1. the map geometry, for both architectures and every (H, W) in range(8, 72) x {8, 33, 47, 64, 71}: hf, wf, c and bytes of
     fav_map_tap_info against the shape of the last block's output - the oracle's, run on one zero frame, up to 40 x 40; above
     that PyTorch's documented convolution arithmetic, floor((x + 2p - k) / s) + 1, chained over the checkpoint's own layer
     table (and held to the oracle's shape wherever the oracle ran);
  2. the cases tests/test_gpu_odd_frames.py runs on the device (the tables below are the ones it iterates): which op kinds and
     flags each plan holds, so that a later planner change cannot quietly move these sizes onto the unfused schedule."""
import numpy as np
import pytest

torch = pytest.importorskip("torch")
from failure_aware_vision_amd import _lib, weights  # noqa: E402
from oracle import fav_oracle as O  # noqa: E402
from test_cam_host import tap_info  # noqa: E402
from test_gpu_schedule_sweep import mc_schedules, plan_of  # noqa: E402

R50, R18 = _lib.ARCH_RESNET50, _lib.ARCH_RESNET18_CIFAR
R50_ALL, R18_ALL = weights.site_mask_for(R50, "all_blocks"), weights.site_mask_for(R18, "all_blocks")

# ---- the device cases (tests/test_gpu_odd_frames.py) ---------------------------------------------------------------------
N = 5
# the last one is very wide: the fused stem's pool output is 2 x 57, eight 8 x 8 pool tiles in a row, the last with one column
R50_SIZES = [(8, 8), (9, 11), (33, 47), (47, 33), (63, 65), (8, 225)]
# defaults; chunks 2,7; a ragged last pass; entry_alone; tail_min_rows = -1; unfused stem; max_batch above the call
R50_SCHEDULES = (1, 3, 5, 7, 10, 12, 13)
R50_POOLED_FIRST = 1 << 16                        # one more site mask: the first (and only) site is the pooled vector
R18_SIZES = [(8, 8), (9, 11), (31, 45)]
R18_SCHEDULES = (3,)                              # chunks 2,7
ENS_HW, ENS_MEMBERS = (33, 47), 3
ENS_SCHEDULES = {"grouped": dict(), "member streams": dict(ens_grouped_max=-1), "grouped, chunks 2,2": dict(chunk_a=2, chunk_b=2)}
VIT_SIZES = [(16, 16), (16, 240)]                 # 2 tokens; 16 tokens: exactly one full key tile


@pytest.fixture(scope="module")
def lib():
    return _lib.load()


# ---- 1. the map geometry --------------------------------------------------------------------------------------------------
HEIGHTS, WIDTHS, ORACLE_MAX = range(8, 72), (8, 33, 47, 64, 71), 40
GEOM_BATCH = 3


def conv_out(x, k, s, p):
    """PyTorch's Conv2d / MaxPool2d output size (dilation 1): floor((x + 2p - k) / s) + 1."""
    return (x + 2 * p - k) // s + 1


def chained_shape(net, h, w):
    """(hf, wf, c) behind the last block, from the checkpoint's layer table alone: the stem (and the ImageNet stem's 3x3/2
    max pool, padding 1), then the main path of every block.  A projection shortcut must arrive at the main path's size -
    the stride-2 3x3 (padding 1) and the 1x1/2 (padding 0) round the same way."""
    L = net.m.layers[0]
    h, w = conv_out(h, L.kh, L.stride, L.pad), conv_out(w, L.kw, L.stride, L.pad)
    if net.cfg["stem"] == "imagenet":
        h, w = conv_out(h, 3, 2, 1), conv_out(w, 3, 2, 1)
    c = L.cout
    for main, down in net.blocks:
        hm, wm = h, w
        for L in main:
            hm, wm = conv_out(hm, L.kh, L.stride, L.pad), conv_out(wm, L.kw, L.stride, L.pad)
        if down is not None:
            assert (conv_out(h, down.kh, down.stride, down.pad), conv_out(w, down.kw, down.stride, down.pad)) == (hm, wm)
            assert down.cout == main[-1].cout
        h, w, c = hm, wm, main[-1].cout
    return h, w, c


def oracle_shape(net, h, w):
    act = net.stem(np.zeros((1, h, w, 3), np.float32))
    for i in range(net.nb):
        act = net.block(i, act)
    return act.shape[1:]


@pytest.mark.parametrize("arch", [R50, R18], ids=["resnet50", "resnet18_cifar"])
def test_map_tap_geometry_at_every_size(lib, arch, r50_blob, r18_blob, monkeypatch):
    # shapes are all this test reads: the epilogue's NumPy specification serves, without a thread team for every tiny tensor
    monkeypatch.setattr(O, "epilogue", O.epilogue_numpy)
    net = O.OracleNet(O.parse_blob((r50_blob if arch == R50 else r18_blob)[0]))
    mc = dict(n_samples=3, dropout_p=0.1, site_mask=weights.site_mask_for(arch, "all_blocks"))
    n_oracle = 0
    for h in HEIGHTS:
        for w in WIDTHS:
            want = chained_shape(net, h, w)
            if h <= ORACLE_MAX and w <= ORACLE_MAX:
                assert tuple(oracle_shape(net, h, w)) == want, (h, w)
                n_oracle += 1
            assert min(want) >= 1
            for S, kw in ((1, {}), (3, mc)):
                st, dims, msg = tap_info(lib, arch, in_h=h, in_w=w, max_batch=GEOM_BATCH, **kw)
                assert st == 0, (h, w, msg)
                assert dims[1:] == (S,) + want, (h, w, dims)
                assert dims[0] == S * GEOM_BATCH * want[0] * want[1] * want[2] * 2, (h, w, dims)
    assert n_oracle == 2 * (ORACLE_MAX - 8 + 1)
    # the two maps the device tests compare with the oracle
    if arch == R50:
        assert chained_shape(net, 33, 47) == (2, 2, 2048) and chained_shape(net, 64, 64) == (2, 2, 2048)
    else:
        assert chained_shape(net, 31, 45) == (4, 6, 512) and chained_shape(net, 32, 32) == (4, 4, 512)


# ---- 2. the plans of the device cases -----------------------------------------------------------------------------------
def flags_of(ops):
    tails = [o for o in ops if o["kind"] == 5]
    return dict(kinds={o["kind"] for o in ops}, tails=len(tails), tails_with_reduce=sum(o["la"] >= 0 for o in tails),
                tails_with_3x3=sum(o["layer"] >= 0 for o in tails), rese=sum(o["rese"] for o in tails),
                skipy=sum(o["kind"] == 6 and o["skipy"] == 1 for o in ops), entry_reduce=sum(o["kind"] == 6 for o in ops),
                entry_alone=sum(o["kind"] == 4 for o in ops), phases=len({o["phase"] for o in ops}))


def headline_flags():
    """The same questions asked of 224 x 224, where the schedule was measured and profiled."""
    return {name: flags_of(plan_of("resnet50", (224, 224), "bf16", R50_ALL, **kw))
            for name, kw in mc_schedules(N, R50_ALL, 16, R50_SCHEDULES).items()}


@pytest.mark.parametrize("hw", R50_SIZES, ids=lambda s: f"{s[0]}x{s[1]}")
def test_resnet50_odd_sizes_are_planned_like_224(hw):
    """Every plan the device test runs at this size holds the ops the same schedule holds at 224 x 224: the fused stem (kind
    7), fused tails that carry the next reduce (kind 5, la >= 0), the entry reduce (kind 6) that skips y (skipy = 1) and the
    tail that takes its residual from the cached tensor (rese = 1)."""
    single = flags_of(plan_of("resnet50", hw, "bf16", max_batch=N))
    assert single == flags_of(plan_of("resnet50", (224, 224), "bf16", max_batch=N))
    assert 7 in single["kinds"] and not single["kinds"] & {0, 2, 4, 6}
    assert (single["tails"], single["tails_with_reduce"], single["tails_with_3x3"], single["phases"]) == (13, 6, 6, 2)
    exact = flags_of(plan_of("resnet50", hw, "f32_exact", max_batch=N))
    assert exact["kinds"] == {0, 1, 2, 3} and exact["tails"] == 0                  # the validation mode: layer by layer
    want = headline_flags()
    seen = set()
    for name, kw in mc_schedules(N, R50_ALL, 16, R50_SCHEDULES).items():
        f = flags_of(plan_of("resnet50", hw, "bf16", R50_ALL, **kw))
        assert f == want[name], (hw, name, f, want[name])
        if name.startswith("07"):                                                  # entry_alone: the dropout takes no reduce
            assert (f["entry_alone"], f["entry_reduce"], f["rese"], f["phases"]) == (1, 0, 0, 2)
        else:
            assert (f["entry_reduce"], f["skipy"], f["rese"], f["entry_alone"], f["phases"]) == (1, 1, 1, 0, 3)
        assert ({0, 2} <= f["kinds"] and 7 not in f["kinds"]) if name.startswith("12") else (7 in f["kinds"] and not f["kinds"] & {0, 2})
        # tail_min_rows -1: the 3x3 of layer 3's identity blocks and layer 4's expanding 1x1 join the tails
        assert (f["tails"], f["tails_with_3x3"]) == ((16, 11) if name.startswith("10") else (13, 6)), (hw, name, f)
        assert f["tails_with_reduce"] == 5                       # every tail of layers 1-2 but the one in front of the entry
        seen.add(name[:2])
    assert seen == {f"{k:02d}" for k in R50_SCHEDULES}
    pooled = flags_of(plan_of("resnet50", hw, "bf16", R50_POOLED_FIRST, max_batch=N))
    assert pooled["entry_alone"] == 1 and 7 in pooled["kinds"] and pooled["tails"] == 13


@pytest.mark.parametrize("hw", R18_SIZES, ids=lambda s: f"{s[0]}x{s[1]}")
def test_resnet18_odd_sizes_keep_the_im2col_stem(hw):
    for mask, kw in ((0, dict(max_batch=N)), (R18_ALL, mc_schedules(N, R18_ALL, 8, R18_SCHEDULES)["03 chunks 2,7"])):
        ops = plan_of("resnet18_cifar", hw, "bf16", mask, **kw)
        f = flags_of(ops)
        assert {0, 1, 3} <= f["kinds"] and not f["kinds"] & {2, 5, 6, 7}, (hw, f)  # im2col + GEMM, basic blocks: no tails
        assert f["entry_alone"] == (1 if mask else 0)
        assert flags_of(plan_of("resnet18_cifar", (32, 32), "bf16", mask, **kw)) == f


def test_ensemble_at_33x47_is_planned_grouped():
    for name, kw in ENS_SCHEDULES.items():
        f = flags_of(plan_of("resnet50", ENS_HW, n_members=ENS_MEMBERS, max_batch=N, **kw))
        assert 7 in f["kinds"] and f["tails"] == 13 and f["tails_with_reduce"] == 6, (name, f)
        assert f == flags_of(plan_of("resnet50", (224, 224), n_members=ENS_MEMBERS, max_batch=N, **kw))


def test_stages_that_are_ragged_at_33x47():
    """What makes 33 x 47 the size to test - the numbers DESIGN.md names: the stem's convolution gives 17 x 24, its pool
    9 x 12 (a second 8 x 8 pool tile with one row), and the four layers run at 9 x 12, 5 x 6, 3 x 3 and 2 x 2."""
    h, w = conv_out(33, 7, 2, 3), conv_out(47, 7, 2, 3)
    assert (h, w) == (17, 24)
    sizes = [(conv_out(h, 3, 2, 1), conv_out(w, 3, 2, 1))]
    for _ in range(3):
        sizes.append((conv_out(sizes[-1][0], 3, 2, 1), conv_out(sizes[-1][1], 3, 2, 1)))
    assert sizes == [(9, 12), (5, 6), (3, 3), (2, 2)]
    assert all(n * hh * ww % 128 for n in (1, N) for hh, ww in sizes)      # no layer's rows fill the 128-row tail tile
