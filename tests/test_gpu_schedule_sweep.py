"""How a call is scheduled never changes its result: every schedule knob, swept on the device, bit for bit against the oracle.

The kernels are pinned one by one at their edges (fav_op_*), and the planner is replayed symbolically on the host
(test_host.py).  This module covers the code between the two - run_chunks / run_phases / run_grouped / run_lanes /
run_vit_call in csrc/fav.hip - which turns a plan into pointers, virtual-frame windows (v0, n_img, first_image_index),
member strides, tap copies and stream forks.  The method is the same in every part: the oracle's logits once per
(arch, frame size, site mask, math mode) - its dropout masks are keyed by global frame id, so one run also serves sub-batches
and shifted first_index - then one Backend per schedule, whose logits must be bit-equal, whose labels must be equal wherever
the top-2 gap of the oracle's mean softmax is >= 1e-6 and whose confidences must lie within 3e-6 (the two head bounds of
test_gpu_exact._exact_case; none is new).

  1. ResNet-50 MC-Dropout: site masks x 13 schedules (chunks, regroup points, tail_min_rows, stem_fused, max_batch above the
     call) at 32 x 32 (layer 4 is 1 x 1) and 48 x 80, plus three follow-up calls on one handle;
  2. what part 1 exercised, asked of the planner (fav_plan_schedule): every op kind and flag the executor branches on;
  3. ResNet-18 (CIFAR stem, basic blocks, the im2col buffer);
  4. a three-member deep ensemble: grouped launches / member streams x chunks x tail_min_rows x stem_fused x max_batch;
  5. ViT calls split over 1-4 streams into even and uneven parts, and the feature tap across the split."""
import collections

import numpy as np
import pytest

pytestmark = pytest.mark.gpu

torch = pytest.importorskip("torch")
from failure_aware_vision_amd import Backend, _lib, synth, weights  # noqa: E402
from oracle import fav_oracle as O  # noqa: E402
from test_host import _plan  # noqa: E402

T, P_DROP, SEED, FIRST = 3, 0.1, 4, 1000
MATH = {"bf16": "mfma", "f32_exact": True}       # Backend math_mode -> the oracle's `exact`
Ref = collections.namedtuple("Ref", "frames logits labels conf tie")
_REFS = {}
_RAN = {}        # (arch, math mode, size, mask, schedule) -> the ops of every MC-Dropout handle that ran a call in this session


def _freeze(*arrays):
    for a in arrays:
        a.flags.writeable = False
    return arrays


def _head_ref(frames, logits):
    labels, conf, pbar = O.confidence_head(logits)
    srt = np.sort(pbar, axis=1)
    tie = (srt[:, -1] - srt[:, -2]) < 1e-6          # the head's expf may differ by an ulp from NumPy's
    return Ref(*_freeze(frames, logits, labels, conf, tie))


def _reference(arch, blobs, hw, n, mask, math, frame_seed=9):
    """The oracle's answer for frames FIRST .. FIRST + n - 1, computed once and shared read-only.  blobs: one checkpoint, or
    the members of an ensemble (logits [M, n, C], one oracle run per member)."""
    key = (arch, hw, n, mask, math, len(blobs) if isinstance(blobs, list) else 0)
    if key not in _REFS:
        frames = synth.synthetic_frames_u8(n, hw[0], hw[1], seed=frame_seed)
        cfg = O.ClassifyConfig(n_samples=T if mask else 1, site_mask=mask, p=P_DROP if mask else 0.0, seed=SEED, exact=MATH[math])
        ids = np.arange(FIRST, FIRST + n)
        if isinstance(blobs, list):
            logits = np.stack([O.classify(O.parse_blob(b), frames, cfg, img_ids=ids, return_logits=True)[2][0] for b in blobs])
        else:
            logits = O.classify(O.parse_blob(blobs), frames, cfg, img_ids=ids, return_logits=True)[2]
        assert np.isfinite(logits).all()
        _REFS[key] = _head_ref(frames, logits)
    return _REFS[key]


def _check_call(be, x, ref, lo, hi, bad, what):
    """Frames [lo, hi) of the reference through `be`; a mismatch is appended to `bad` (so that one run names every schedule
    that is wrong), a refused or failed call raises."""
    labels, conf = be.classify(x[lo:hi], first_index=FIRST + lo)
    lg = be.logits().cpu().numpy()
    olg = ref.logits[:, lo:hi]
    if lg.shape != olg.shape:
        bad.append(f"{what}: logits of shape {lg.shape}, expected {olg.shape}")
        return
    if not np.array_equal(lg, olg):
        bad.append(f"{what}: {np.mean(lg != olg):.4f} of the logits differ, max {np.abs(lg - olg).max():.3g}")
    keep = ~ref.tie[lo:hi]
    if not np.array_equal(labels.cpu().numpy()[keep], ref.labels[lo:hi][keep]):
        bad.append(f"{what}: labels differ")
    err = np.abs(conf.cpu().numpy() - ref.conf[lo:hi]).max()
    if not err <= 3e-6:
        bad.append(f"{what}: confidence off by {err:.3g}")


# ---- the schedules of the MC-Dropout parts ---------------------------------------------------------------------------
def _first_site(mask):
    return (mask & -mask).bit_length() - 1


def mc_schedules(n, mask, nb, which=None):
    """name -> Backend keyword arguments; max_batch = n unless the schedule says otherwise."""
    fs = _first_site(mask)
    inside = dict(chunk_a=2, chunk_b=7)              # windows start and end inside a sample
    ones = dict(chunk_a=1, chunk_b=1)
    s = {
        "01 defaults": {},
        "02 chunks 1,1": ones,
        "03 chunks 2,7": inside,
        "04 chunks n,2n (whole samples)": dict(chunk_a=n, chunk_b=2 * n),
        "05 chunks n+1,3n (ragged last pass; one pass)": dict(chunk_a=n + 1, chunk_b=3 * n),
        "06 regroup 0": dict(regroup_block=0),
        "07 regroup first_site+1 (entry_alone)": dict(regroup_block=fs + 1),
        "08 regroup first_site+2": dict(regroup_block=fs + 2),
        "09 regroup at the pool": dict(regroup_block=nb),
        "10 tail_min_rows -1, chunks 2,7": dict(tail_min_rows=-1, **inside),
        "11 tail_min_rows 2^30": dict(tail_min_rows=1 << 30),
        "12 stem_fused -1, chunks 1,1": dict(stem_fused=-1, **ones),
        "13 max_batch 2n+3, chunks 2,7": dict(max_batch=2 * n + 3, **inside),
    }
    return {k: dict(dict(max_batch=n), **v) for k, v in s.items() if which is None or int(k[:2]) in which}


def plan_of(arch, hw, math="bf16", mask=0, n_members=1, **kw):
    """The plan fav_create makes for these Backend arguments (fav_plan_schedule: the same plan_resnet call, no device)."""
    cfg = dict(in_h=hw[0], in_w=hw[1], math_mode=0 if math == "bf16" else 1, n_members=n_members, **kw)
    if mask:
        cfg.update(site_mask=mask, n_samples=T, dropout_p=P_DROP, seed=SEED)
    return _plan(_lib.load(), weights.ARCH_IDS[arch], 0, **cfg)


def _mc_sweep(arch, blob, hw, n, mask, math, which=None):
    ref = _reference(arch, blob, hw, n, mask, math)
    assert not np.array_equal(ref.logits[0], ref.logits[1])          # the samples differ: the masks are drawn
    x = torch.tensor(ref.frames, device="cuda")
    bad = []
    for name, kw in mc_schedules(n, mask, weights.n_blocks(weights.ARCH_IDS[arch]), which).items():
        ops = plan_of(arch, hw, math, mask, **kw)                    # the planner takes it (asserted in _plan)
        be = Backend(arch, blob, in_hw=hw, math_mode=math, n_samples=T, site_mask=mask, dropout_p=P_DROP, seed=SEED, **kw)
        try:
            _check_call(be, x, ref, 0, n, bad, name)
            if name.startswith("13"):
                # the handle again: a window that starts behind frame 0, one frame, then everything - whatever a call leaves
                # behind (a stride of the call's n, rows of a longer call in the workspace) shows up in the next one
                _check_call(be, x, ref, 1, n - 1, bad, name + " / frames [1, n-1)")
                _check_call(be, x, ref, n - 1, n, bad, name + " / frame n-1 alone")
                _check_call(be, x, ref, 0, n, bad, name + " / all n again")
            _RAN[(arch, math, hw, mask, name)] = ops
        finally:
            be.close()
    assert not bad, "\n".join(bad)


# ---- 1. ResNet-50, MC-Dropout: site masks x schedules -------------------------------------------------------------------
R50_ALL = weights.site_mask_for(1, "all_blocks")
# bit b: the site behind block b; bit 16: the pooled features.  mask -> what the default schedule's entry op is: (op kind,
# skip_y, tails with res_entry) - test_the_resnet50_sweep_reaches_every_executor_path holds the planner to this column
R50_ENTRY = {
    1: (6, 0, 0),                        # entry_reduce that stores y: nobody draws at block 1
    0b11: (6, 1, 1),                     # entry_reduce with skip_y + the res_entry tail
    0b110: (6, 0, 0),                    # one block later: the reduce again, but block 2's tail feeds layer 2 (128 channels), so y is stored
    1 << 2: (4, 0, 0),                   # entry dropout alone in front of layer 2
    (1 << 3) | (1 << 9): (4, 0, 0),      # entry dropout alone inside layer 2, and a late second site
    (1 << 6) | (1 << 7): (4, 0, 0),      # entry dropout alone at the layer-2/3 seam (the default regroup point: entry_alone)
    (1 << 12) | (1 << 16): (4, 0, 0),    # a site in layer 3 and the pooled-feature site
    1 << 15: (4, 0, 0),                  # the suffix starts behind the last block
    1 << 16: (4, 0, 0),                  # the suffix starts behind the pool
    R50_ALL: (6, 1, 1),
}
R50_MASKS = list(R50_ENTRY)
# 32 x 32: layer 1 is 8 x 8 and layer 4 is 1 x 1; with n = 4 a sample of layer 1 is 256 rows, a multiple of the 128-row tail
# tile, so whole-sample chunks reach the sample-minor tile order.  48 x 80: not square, layer 1 is 12 x 20, a sample of
# 5 frames is never a multiple of 128 rows
R50_SIZES = [((32, 32), 4), ((48, 80), 5)]


def _mask_id(m):
    return "all_blocks" if m in (R50_ALL, weights.site_mask_for(0, "all_blocks")) else bin(m)


@pytest.mark.parametrize("hw,n", R50_SIZES, ids=["32x32", "48x80"])
@pytest.mark.parametrize("mask", R50_MASKS, ids=_mask_id)
def test_resnet50_site_mask_under_every_schedule(r50_blob, mask, hw, n):
    _mc_sweep("resnet50", r50_blob[0], hw, n, mask, "bf16")


@pytest.mark.parametrize("hw,n", R50_SIZES, ids=["32x32", "48x80"])
@pytest.mark.parametrize("mask", [R50_ALL, 0b11], ids=_mask_id)
def test_resnet50_site_mask_under_schedules_validation_mode(r50_blob, mask, hw, n):
    _mc_sweep("resnet50", r50_blob[0], hw, n, mask, "f32_exact", which=(1, 3, 9))


# ---- 2. what part 1 exercised --------------------------------------------------------------------------------------------
def _r50_layer_block():
    """conv layer index (blob order) -> residual block, ResNet-50."""
    out, idx = {}, 1
    for b, (nmain, ds) in enumerate(O.block_table(1)):
        for _ in range(nmain + (1 if ds else 0)):
            out[idx] = b
            idx += 1
    return out


def part1_plans():
    """(size, mask, schedule) -> ops, for exactly the pairs test_resnet50_site_mask_under_every_schedule runs."""
    return {(hw, mask, name): plan_of("resnet50", hw, "bf16", mask, **kw)
            for hw, n in R50_SIZES for mask in R50_MASKS for name, kw in mc_schedules(n, mask, 16).items()}


def test_the_resnet50_sweep_reaches_every_executor_path():
    """Part 1 iterates mc_schedules over R50_MASKS x R50_SIZES, and so does this test: the plans below are the plans of
    the handles part 1 runs, and every handle of it that ran in this session recorded the plan it ran with - the same one.
    Each op kind and flag run_chunks branches on must occur in at least one of them."""
    plans = part1_plans()
    assert len(plans) == len(R50_SIZES) * len(R50_MASKS) * 13
    ran = {k[2:]: ops for k, ops in _RAN.items() if k[:2] == ("resnet50", "bf16")}
    assert set(ran) <= set(plans) and all(plans[k] == ops for k, ops in ran.items())
    print(f"part 1: {len(ran)} of the {len(plans)} handles ran before this test")
    block_of = _r50_layer_block()
    seen = collections.Counter()
    for (hw, mask, name), ops in plans.items():
        kinds = {o["kind"] for o in ops}
        seen["entry dropout alone"] += 4 in kinds
        seen["entry reduce, y skipped"] += any(o["kind"] == 6 and o["skipy"] == 1 for o in ops)
        seen["entry reduce, y stored"] += any(o["kind"] == 6 and o["skipy"] == 0 for o in ops)
        seen["fused stem"] += 7 in kinds
        seen["im2col stem + max pool"] += {0, 2} <= kinds
        assert (7 in kinds) != ({0, 2} <= kinds)
        tails = [o for o in ops if o["kind"] == 5]
        if name.startswith("01"):
            entry = [o for o in ops if o["kind"] in (4, 6)]
            assert len(entry) == 1 and (entry[0]["kind"], entry[0]["skipy"], sum(o["rese"] for o in tails)) == R50_ENTRY[mask], (hw, mask)
        seen["tail, res_entry"] += any(o["rese"] == 1 for o in tails)
        seen["tail with the next reduce"] += any(o["la"] >= 0 for o in tails)
        seen["tail without the next reduce"] += any(o["la"] < 0 for o in tails)
        l3 = any(o["layer"] >= 0 and 7 <= block_of[o["lc"]] <= 12 for o in tails)      # conv_b inside a layer-3 tail
        l4 = any(block_of[o["lc"]] >= 13 for o in tails)
        seen["layer-3 tail with its 3x3"] += l3
        seen["layer-4 tail"] += l4
        # at these frame sizes both need the caller's word: the planned launch is far below two blocks per CU
        assert not (l3 or l4) or name.startswith("10"), (hw, mask, name)
        seen[f"{len({o['phase'] for o in ops})} phases"] += 1
        # the suffix is marked on the ops behind the first site only
        assert any(o["suffix"] for o in ops) and not ops[0]["suffix"]
    for what in ("entry dropout alone", "entry reduce, y skipped", "entry reduce, y stored", "fused stem", "im2col stem + max pool",
                 "tail, res_entry", "tail with the next reduce", "tail without the next reduce", "layer-3 tail with its 3x3",
                 "layer-4 tail", "2 phases", "3 phases"):
        assert seen[what] > 0, (what, dict(seen))
    # Four phases (fav_plan.hpp kMaxPhases: "prefix and suffix, each split at most once") cannot occur: a configuration has ONE
    # regroup point (plan_resnet, `int regroup = std::min(c.regroup_block < 0 ? ... : c.regroup_block, P.nblocks)`), which lies
    # either in the prefix or in the suffix, so one of the two is split and the other is not; and directly behind the entry
    # op it splits nothing (entry_alone: two phases).  One phase cannot occur with MC-Dropout: the entry op closes the prefix.
    assert seen["4 phases"] == 0 and seen["1 phases"] == 0
    print("part 1:", len(plans), "(configuration, schedule) pairs,", len({str(v) for v in plans.values()}), "distinct plans;",
          dict(seen))


# ---- 3. ResNet-18 --------------------------------------------------------------------------------------------------------
R18_ALL = weights.site_mask_for(0, "all_blocks")
R18_MASKS = [1, 0b11, 1 << 4, (1 << 7) | (1 << 8), 1 << 8, R18_ALL]
R18_SCHEDULES = (1, 2, 3, 4, 5, 6, 9, 13)


@pytest.mark.parametrize("mask", R18_MASKS, ids=_mask_id)
def test_resnet18_site_mask_under_every_schedule(r18_blob, mask):
    _mc_sweep("resnet18_cifar", r18_blob[0], (32, 32), 6, mask, "bf16", which=R18_SCHEDULES)


def test_resnet18_all_blocks_under_every_schedule_validation_mode(r18_blob):
    _mc_sweep("resnet18_cifar", r18_blob[0], (32, 32), 6, R18_ALL, "f32_exact", which=R18_SCHEDULES)


# ---- 4. deep ensemble ---------------------------------------------------------------------------------------------------
ENS_N, ENS_FOLLOW_UP = 5, 2


@pytest.mark.parametrize("max_batch", [5, 9])
@pytest.mark.parametrize("chunks", [(0, 0), (1, 1), (2, 3)], ids=lambda c: f"chunks{c[0]}-{c[1]}")
@pytest.mark.parametrize("grouped_max", [-1, 0, 3])
@pytest.mark.parametrize("hw", [(32, 32), (64, 64)], ids=["32x32", "64x64"])
def test_ensemble_members_under_every_schedule(r50_members, hw, grouped_max, chunks, max_batch):
    """Three ResNet-50 members, 5 frames, no dropout: member streams (ens_grouped_max -1), grouped launches (0), and both
    on one handle (3: the 5-frame call runs by lanes, the 2-frame call behind it grouped - on a plan made for lanes)."""
    blobs = [b for b, _ in r50_members[:3]]
    ref = _reference("resnet50", blobs, hw, ENS_N, 0, "bf16", frame_seed=12)
    assert not np.array_equal(ref.logits[0], ref.logits[1])          # the members are different networks
    x = torch.tensor(ref.frames, device="cuda")
    bad = []
    for tail_min_rows in (0, -1):
        for stem_fused in (0, -1):
            kw = dict(max_batch=max_batch, ens_grouped_max=grouped_max, chunk_a=chunks[0], chunk_b=chunks[1],
                      tail_min_rows=tail_min_rows, stem_fused=stem_fused)
            kinds = {o["kind"] for o in plan_of("resnet50", hw, n_members=3, **kw)}
            # stem_fused -1: im2col + GEMM + max pool, and will_group (fav_plan.hpp) then refuses every call of the handle
            assert ({0, 2} <= kinds and 7 not in kinds) if stem_fused < 0 else (7 in kinds and not kinds & {0, 2}), kw
            what = f"tail_min_rows={tail_min_rows} stem_fused={stem_fused}"
            be = Backend("resnet50", blobs, in_hw=hw, **kw)
            try:
                _check_call(be, x, ref, 0, ENS_N, bad, what)
                _check_call(be, x, ref, 0, ENS_FOLLOW_UP, bad, what + f" / {ENS_FOLLOW_UP} frames on the same handle")
            finally:
                be.close()
    assert not bad, "\n".join(bad)


# ---- 5. ViT parts --------------------------------------------------------------------------------------------------------
VIT_N = 37
VIT_SIZES = [(64, 64), (48, 80)]      # 17 tokens; 16 tokens: exactly one key tile


_VIT_BLOBS = {}


def _vit_reference(hw, math):
    if hw not in _VIT_BLOBS:
        _VIT_BLOBS[hw] = weights.make_synthetic_vit("vit_tiny", seed=3, in_hw=hw)[0]
    return _VIT_BLOBS[hw], _reference("vit_tiny", _VIT_BLOBS[hw], hw, VIT_N, 0, math, frame_seed=11)


@pytest.mark.parametrize("streams", [1, 2, 3, 4])
@pytest.mark.parametrize("math", ["bf16", "f32_exact"])
@pytest.mark.parametrize("hw", VIT_SIZES, ids=["64x64", "48x80"])
def test_vit_call_split_into_parts(hw, math, streams):
    """run_vit_call splits a call of n >= 8 s frames into s parts [n p / s, n (p + 1) / s) on s streams: one frame below the
    rule, even parts, uneven parts, the whole workspace - and the first call again, all on one handle."""
    blob, ref = _vit_reference(hw, math)
    x = torch.tensor(ref.frames, device="cuda")
    bad = []
    be = Backend("vit_tiny", blob, in_hw=hw, math_mode=math, max_batch=VIT_N, vit_streams=streams)
    try:
        for n in (8 * streams - 1, 8 * streams, 8 * streams + 1, VIT_N, 8 * streams - 1):
            _check_call(be, x, ref, 0, n, bad, f"{n} frames")
    finally:
        be.close()
    assert not bad, "\n".join(bad)


@pytest.mark.parametrize("math", ["bf16", "f32_exact"])
@pytest.mark.parametrize("hw", VIT_SIZES, ids=["64x64", "48x80"])
def test_vit_feature_tap_across_the_split(hw, math):
    blob, ref = _vit_reference(hw, math)
    x = torch.tensor(ref.frames, device="cuda")
    bad, feats = [], {}
    for streams in (1, 4):
        be = Backend("vit_tiny", blob, in_hw=hw, math_mode=math, max_batch=VIT_N, vit_streams=streams)
        try:
            be.set_feature_tap(True)
            _check_call(be, x, ref, 0, VIT_N, bad, f"vit_streams={streams}, tap on")
            feats[streams] = be.features().cpu().numpy()
        finally:
            be.close()
    assert not bad, "\n".join(bad)
    assert feats[1].shape == (1, VIT_N, 128) and np.isfinite(feats[1]).all() and not np.array_equal(feats[1][0, 0], feats[1][0, 1])
    assert np.array_equal(feats[1], feats[4])
