"""Odd frame sizes end to end: every network and every schedule form at sizes where every stage is ragged, bit for bit against
the oracle.

fav_create takes any in_h, in_w >= 8 for the two ResNet architectures, and the kernels are pinned at odd shapes one at a time
(fav_op_*: stem 33 x 47, conv 13 x 9 and 15 x 15, tails 7 x 9).  This module runs the code between the plan and the kernels -
ResNetWalk chaining conv_out, alloc_workspace sizing the arenas from out_elems * chunk, run_chunks turning a plan into
pointers and windows, the member strides of grouped launches, the tap copies - at sizes no dimension of which stays even:
at 33 x 47 the fused stem's pool output is 9 x 12 (a second 8 x 8 pool tile with one row), the stride-2 3x3 and the 1x1/2
projection shortcut must agree on ceil at 9 -> 5 -> 3 -> 2, and layer 4's tails run on 2 x 2 frames; at 8 x 8 layers 2-4 are
1 x 1.  tests/test_odd_frames_host.py holds the planner to the fused schedule for exactly the tables iterated here.

The method and the three rules are test_gpu_schedule_sweep's (_reference, _check_call; no tolerance is new): the oracle once
per (arch, size, mask, math mode), keyed by global frame id; logits np.array_equal; labels equal wherever the oracle's top-2
gap is >= 1e-6 - and for these inputs that rule leaves out no frame (asserted); confidences within 3e-6.  Frames:
synth.synthetic_frames_u8(5, H, W, seed=9), ids 1000 .. 1004, checkpoints of seed 1.  Smallest top-2 gap of the oracle's mean
softmax over the five frames, ResNet-50 (single pass bf16 / f32 chain; all_blocks T = 3 bf16 / f32 chain): 8 x 8: 0.19 / 0.19;
0.0011 / 0.0011.  9 x 11: 0.013 / 0.015; 0.0026 / 0.0021.  33 x 47: 0.098 / 0.107; 0.0037 / 0.0042.  47 x 33: 0.011 / 0.0069;
0.013 / 0.014.  63 x 65: 0.18 / 0.15; 0.020 / 0.027.  8 x 225 (one size more: a pool output of 2 x 57, eight pool tiles in a
row, the last of one column): 0.020 / 0.022; 0.0015 / 0.0014.  The smallest of all the references below: ResNet-18 all_blocks at
9 x 11, bf16, 1.7e-4, and the ViT miniature at 16 x 240, 2.1e-4 - two orders of magnitude above the rule's 1e-6."""
import numpy as np
import pytest

pytestmark = pytest.mark.gpu

torch = pytest.importorskip("torch")
import cam_ref  # noqa: E402
from failure_aware_vision_amd import Backend, weights  # noqa: E402
from oracle import fav_oracle as O  # noqa: E402
from test_gpu_ood import assert_fc_of_features_is_logits, fc_of  # noqa: E402
from test_gpu_schedule_sweep import FIRST, P_DROP, SEED, T, _check_call, _reference, mc_schedules, plan_of  # noqa: E402
from test_odd_frames_host import (ENS_HW, ENS_MEMBERS, ENS_SCHEDULES, N, R18_ALL, R18_SCHEDULES, R18_SIZES, R50_ALL,  # noqa: E402
                                  R50_POOLED_FIRST, R50_SCHEDULES, R50_SIZES, VIT_SIZES)

MATHS = ["bf16", "f32_exact"]


def size_id(hw):
    return f"{hw[0]}x{hw[1]}"


def reference(arch, blobs, hw, n, mask, math):
    ref = _reference(arch, blobs, hw, n, mask, math)          # frame seed 9
    assert not ref.tie.any(), (arch, hw, mask, math)          # the label rule leaves out no frame
    return ref


def run_schedules(arch, blob, hw, mask, math, schedules, follow_up=()):
    """One handle per schedule, all N frames; on the schedules named in follow_up, frames [1, 4) behind it on the same
    handle, with first_index moved, then all N again."""
    ref = reference(arch, blob, hw, N, mask, math)
    if mask:
        assert ref.logits.shape[0] == T and not np.array_equal(ref.logits[0], ref.logits[1])      # the masks are drawn
    x = torch.tensor(ref.frames, device="cuda")
    mc = dict(n_samples=T, site_mask=mask, dropout_p=P_DROP, seed=SEED) if mask else {}
    bad = []
    for name, kw in schedules.items():
        plan_of(arch, hw, math, mask, **kw)                    # the planner takes it (asserted in _plan)
        be = Backend(arch, blob, in_hw=hw, math_mode=math, **mc, **kw)
        try:
            _check_call(be, x, ref, 0, N, bad, name)
            if name[:2] in follow_up:
                _check_call(be, x, ref, 1, 4, bad, name + " / frames [1, 4)")
                _check_call(be, x, ref, 0, N, bad, name + " / all frames again")
        finally:
            be.close()
    assert not bad, "\n".join(bad)


# ---- ResNet-50 ---------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("math", MATHS)
@pytest.mark.parametrize("hw", R50_SIZES, ids=size_id)
def test_resnet50_single_pass(r50_blob, hw, math):
    run_schedules("resnet50", r50_blob[0], hw, 0, math,
                  {"01 defaults": dict(max_batch=N), "13 max_batch 2n+3, chunks 2,7": dict(max_batch=2 * N + 3, chunk_a=2, chunk_b=7)},
                  follow_up=("13",))


@pytest.mark.parametrize("math", MATHS)
@pytest.mark.parametrize("hw", R50_SIZES, ids=size_id)
def test_resnet50_all_blocks_under_every_schedule_form(r50_blob, hw, math):
    run_schedules("resnet50", r50_blob[0], hw, R50_ALL, math, mc_schedules(N, R50_ALL, 16, R50_SCHEDULES), follow_up=("01", "13"))


@pytest.mark.parametrize("math", MATHS)
@pytest.mark.parametrize("hw", R50_SIZES, ids=size_id)
def test_resnet50_first_site_is_the_pooled_vector(r50_blob, hw, math):
    run_schedules("resnet50", r50_blob[0], hw, R50_POOLED_FIRST, math, mc_schedules(N, R50_POOLED_FIRST, 16, (1, 3)))


# ---- ResNet-18 CIFAR: the im2col buffer's rows at odd Ho * Wo ---------------------------------------------------------------
@pytest.mark.parametrize("math", MATHS)
@pytest.mark.parametrize("hw", R18_SIZES, ids=size_id)
def test_resnet18_single_pass_and_all_blocks(r18_blob, hw, math):
    run_schedules("resnet18_cifar", r18_blob[0], hw, 0, math, {"01 defaults": dict(max_batch=N)})
    run_schedules("resnet18_cifar", r18_blob[0], hw, R18_ALL, math, mc_schedules(N, R18_ALL, 8, R18_SCHEDULES), follow_up=("03",))


# ---- three-member ResNet-50 ensemble at 33 x 47 --------------------------------------------------------------------------
def test_ensemble_member_strides_at_33x47(r50_members):
    """A grouped launch finds member g's tensors a constant stride behind member 0's, and its rows are frames x Ho x Wo a
    member: 108, 30, 9 and 4 rows a frame in the four layers at 33 x 47, so with 5, 3 or 2 frames a member no member's rows end
    on a tile boundary (128 rows) as they did at the even sizes."""
    blobs = [b for b, _ in r50_members[:ENS_MEMBERS]]
    ref = reference("resnet50", blobs, ENS_HW, N, 0, "bf16")
    assert ref.logits.shape[0] == ENS_MEMBERS and not np.array_equal(ref.logits[0], ref.logits[1])
    x = torch.tensor(ref.frames, device="cuda")
    bad = []
    for name, kw in ENS_SCHEDULES.items():
        be = Backend("resnet50", blobs, in_hw=ENS_HW, max_batch=N, **kw)
        try:
            _check_call(be, x, ref, 0, N, bad, name)
            _check_call(be, x, ref, 1, 4, bad, name + " / frames [1, 4)")
        finally:
            be.close()
    assert not bad, "\n".join(bad)


# ---- ViT miniature ---------------------------------------------------------------------------------------------------------
_VIT_BLOBS = {}
VIT_N = 17           # vit_streams = 2 splits a call from 16 frames on; the first 5 frames alone are one part


@pytest.mark.parametrize("streams", [1, 2])
@pytest.mark.parametrize("math", MATHS)
@pytest.mark.parametrize("hw", VIT_SIZES, ids=size_id)
def test_vit_at_two_and_at_sixteen_tokens(hw, math, streams):
    if hw not in _VIT_BLOBS:
        _VIT_BLOBS[hw] = weights.make_synthetic_vit("vit_tiny", seed=1, in_hw=hw)[0]
    bad = []
    for n in (N, VIT_N):
        ref = reference("vit_tiny", _VIT_BLOBS[hw], hw, n, 0, math)
        x = torch.tensor(ref.frames, device="cuda")
        be = Backend("vit_tiny", _VIT_BLOBS[hw], in_hw=hw, math_mode=math, max_batch=n, vit_streams=streams)
        try:
            _check_call(be, x, ref, 0, n, bad, f"{n} frames")
            _check_call(be, x, ref, 1, 4, bad, f"frames [1, 4) of {n}")
        finally:
            be.close()
    assert not bad, "\n".join(bad)


# ---- the map tap against the oracle -------------------------------------------------------------------------------------------
TAPS = {"r50_33x47": ("resnet50", (33, 47), (2, 2, 2048)), "r18_31x45": ("resnet18_cifar", (31, 45), (4, 6, 512))}


def bits_of(t):
    return t.view(torch.int16).cpu().numpy().view(np.uint16)


@pytest.mark.parametrize("case", list(TAPS))
def test_map_tap_is_the_oracle_activation_behind_the_last_block(case, r18_blob, r50_blob):
    arch, hw, (hf, wf, c) = TAPS[case]
    blob = (r50_blob if arch == "resnet50" else r18_blob)[0]
    ref = reference(arch, blob, hw, N, 0, "bf16")
    net = O.OracleNet(O.parse_blob(blob), exact="mfma")
    cfg = O.ClassifyConfig()
    act = net.stem(O.normalize_input(ref.frames, cfg.mean, O.inv_std32(cfg.std)))
    for i in range(net.nb):
        act = net.block(i, act)
    assert act.shape == (N, hf, wf, c) and (act > 0).mean() > 0.05
    assert np.array_equal(net.logits(net.pool(act))[None], ref.logits)            # the same pass the logits came from
    for kw in (dict(), dict(chunk_a=2, chunk_b=3)):
        be = Backend(arch, blob, in_hw=hw, max_batch=N + 2, **kw)
        try:
            info = be.map_tap_info()
            assert info == dict(bytes=(N + 2) * hf * wf * c * 2, samples=1, hf=hf, wf=wf, c=c)
            be.set_map_tap(True)
            be.set_feature_tap(True)
            bad = []
            x = torch.tensor(ref.frames, device="cuda")
            _check_call(be, x, ref, 0, N, bad, "taps on")
            assert not bad, "\n".join(bad)
            maps = be.maps()
            assert tuple(maps.shape) == (1, N, hf, wf, c) and maps.dtype == torch.bfloat16
            assert np.array_equal(bits_of(maps)[0], cam_ref.f32_to_bf16_bits(act))
            assert np.array_equal(cam_ref.bf16_bits_to_f32(bits_of(maps)[0]).view(np.uint32), act.view(np.uint32))
            feats = be.features().cpu().numpy()
            assert feats.shape == (1, N, c) and np.array_equal(feats[0].view(np.uint32), net.pool(act).view(np.uint32))
            # a shorter call behind it: frames [1, 4) only, the rest of the buffer is not part of the answer
            _check_call(be, x, ref, 1, 4, bad, "taps on, frames [1, 4)")
            assert not bad, "\n".join(bad)
            assert np.array_equal(bits_of(be.maps())[0], cam_ref.f32_to_bf16_bits(act[1:4]))
        finally:
            be.close()


@pytest.mark.parametrize("case", list(TAPS))
def test_map_tap_under_all_blocks_pools_to_the_features_the_fc_read(case, r18_blob, r50_blob):
    arch, hw, (hf, wf, c) = TAPS[case]
    blob = (r50_blob if arch == "resnet50" else r18_blob)[0]
    mask = R50_ALL if arch == "resnet50" else R18_ALL
    ref = reference(arch, blob, hw, N, mask, "bf16")
    be = Backend(arch, blob, in_hw=hw, max_batch=N, n_samples=T, site_mask=mask, dropout_p=P_DROP, seed=SEED, chunk_a=2, chunk_b=7)
    try:
        assert be.map_tap_info() == dict(bytes=T * N * hf * wf * c * 2, samples=T, hf=hf, wf=wf, c=c)
        be.set_map_tap(True)
        be.set_feature_tap(True)
        lg, ft = assert_fc_of_features_is_logits(be, ref.frames.copy(), [fc_of(blob)], first=FIRST)   # the reference stays read-only
        assert np.array_equal(lg, ref.logits)
        maps = be.maps()
        assert tuple(maps.shape) == (T, N, hf, wf, c)
        xb = bits_of(maps).reshape(T, N, hf * wf, c)
        assert np.array_equal(cam_ref.pool(xb), cam_ref.f32_to_bf16_bits(ft))
        assert not np.array_equal(xb[0], xb[1])                                    # every sample has its own maps
    finally:
        be.close()
