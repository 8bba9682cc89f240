"""Attention rollout on the device: fav_op_attn_mean and fav_op_attn_rollout against tests/rollout_ref.py, the attention tap
and the Backend methods end to end, the maps against float64, and the refusals.

Bits are compared with the numpy restatement throughout (R.same_bits).  The contract (include/fav.h beside fav_set_attn_tap and
fav_rollout_record) fixes every product and every sum, so A, maps and records must be the reference's dwords.

Shapes of the tap: T in {2, 5, 16, 17, 100, 197, 256} - one key tile, the 16 / 17 tile edge, 7 tiles, the production 13 tiles,
the full 16 - covers the four instantiations (up to 2 key tiles, exactly 13, exactly 16, and any other count with run-time
guards), blocks whose last waves have no query tile (13 tiles in groups of 4) and several blocks a frame; heads in {1, 2, 12}
covers no second K buffer, one swap and the production count."""
import ctypes as C

import numpy as np
import pytest

pytestmark = pytest.mark.gpu

torch = pytest.importorskip("torch")
import cam_ref  # noqa: E402
import rollout_ref as R  # noqa: E402
from conftest import note  # noqa: E402
from failure_aware_vision_amd import Backend, _lib, synth, views, weights  # noqa: E402
from failure_aware_vision_amd.rollout import patch_box_to_pixels, unpack_rollout_records  # noqa: E402

GUARD = 256
FILL = 0x5A


@pytest.fixture(scope="module")
def lib():
    assert torch.cuda.is_available(), "GPU tests need a MI355X"
    return _lib.load()


def dev(a):
    return torch.from_numpy(np.ascontiguousarray(a)).cuda()


def guarded(nbytes):
    buf = torch.full((GUARD + nbytes + GUARD,), FILL, dtype=torch.uint8, device="cuda")
    assert buf.data_ptr() % 16 == 0
    return buf


def guards_ok(buf, nbytes):
    host = buf.cpu().numpy()
    return bool((host[:GUARD] == FILL).all() and (host[GUARD + nbytes:] == FILL).all())


def stream():
    return torch.cuda.current_stream().cuda_stream


def bf16_values(x):
    return torch.from_numpy(np.ascontiguousarray(x, np.float32)).to(torch.bfloat16).float().numpy()


def bits_of(t):
    return t.contiguous().view(torch.int32).cpu().numpy().view(np.uint32)


# ---- fav_op_attn_mean --------------------------------------------------------------------------------------------------------
def qkv_problem(seed, n, T, heads):
    """bf16 values [n, T, 3 D]: Q scaled by 2, so the scaled scores have a standard deviation of 2 and the rows are peaked."""
    rng = np.random.default_rng(seed)
    x = rng.standard_normal((n, T, 3 * 64 * heads)).astype(np.float32)
    x[:, :, :64 * heads] *= 2.0
    return bf16_values(x)


def run_attn_mean(lib, qkv, n_heads, **over):
    """-> (status, A float32 [n, T, ld], guards untouched?, output untouched?).  over: sizes passed instead of the arrays' own."""
    n, T, d3 = qkv.shape
    ld = R.attn_ld(T)
    q = torch.from_numpy(qkv).cuda().to(torch.bfloat16).contiguous()
    nbytes = n * T * ld * 4
    a = guarded(nbytes)
    args = dict(n=n, T=T, D=d3 // 3, heads=n_heads)
    null = over.pop("null", ())
    off = over.pop("off", dict())
    args.update(over)
    st = lib.fav_op_attn_mean(None if "qkv" in null else q.data_ptr() + off.get("qkv", 0),
                              None if "a" in null else a.data_ptr() + GUARD + off.get("a", 0),
                              args["n"], args["T"], args["D"], args["heads"], stream())
    torch.cuda.synchronize()
    body = a.cpu().numpy()[GUARD:GUARD + nbytes]
    return st, body.copy().view(np.float32).reshape(n, T, ld), guards_ok(a, nbytes), bool((body == FILL).all())


@pytest.mark.parametrize("n", [1, 3])
@pytest.mark.parametrize("heads", [1, 2, 12])
@pytest.mark.parametrize("T", [2, 5, 16, 17, 100, 197, 256])
def test_op_attn_mean_matches_the_reference(lib, T, heads, n):
    qkv = qkv_problem(T * 100 + heads * 4 + n, n, T, heads)
    st, A, guards, _ = run_attn_mean(lib, qkv, heads)
    assert st == 0 and guards
    want = R.attn_mean(qkv, heads)
    assert R.same_bits(A, want)
    assert not A[:, :, T:].view(np.uint32).any()                 # the padded columns: +0, not -0
    sums = A.astype(np.float64).sum(-1)
    assert np.abs(sums - 1.0).max() < 1e-4                       # rounding: 256 * 2^-23 ~ 3e-5; a dropped key tile is far off
    if heads == 1 and T >= 16:
        assert A[:, :, :T].max() > 4.0 / T                       # one head's rows are peaked, not flat


def poisoned_qkv(seed, n, T, heads):
    """qkv_problem with, in every head of every frame, one query row whose scores are all NaN (a NaN in Q) and one whose scores
    are all -inf (+inf in a Q channel where every key holds -1): both rows come out NaN, every other row stays finite."""
    qkv = qkv_problem(seed, n, T, heads)
    D = 64 * heads
    for h in range(heads):
        qkv[:, :, D + 64 * h + 7] = -1.0
        qkv[:, 0, 64 * h + 3] = np.nan
        qkv[:, T - 1, 64 * h + 7] = np.inf
    return qkv


# The tap calls fav_attn_softmax; attention_kernel holds the same statements in place.  The tap's four instantiations - T = 2
# and 17: up to 2 key tiles (one masked tile with one real key beside the class token; two tiles, one live key in the last);
# 197: exactly 13; 250: 16 with run-time guards; 256: exactly 16 - and the production route of the same shape, each against its
# oracle on an input with a NaN score row and a -inf score row: NaNs where the oracle has them, its bits everywhere else.
@pytest.mark.parametrize("T", [2, 17, 197, 250, 256])
def test_the_tap_and_production_attention_share_their_softmax(lib, T):
    from oracle import fav_oracle as O
    n, heads = 2, 2
    D = 64 * heads
    qkv = poisoned_qkv(T, n, T, heads)
    bad = np.zeros(T, bool)
    bad[[0, T - 1]] = True
    # the tap
    st, A, guards, _ = run_attn_mean(lib, qkv, heads)
    assert st == 0 and guards
    want = R.attn_mean(qkv, heads)
    assert np.isnan(want[:, bad, :T]).all() and np.isfinite(want[:, ~bad]).all()
    assert R.same_bits(A[:, :, :T], want[:, :, :T])
    assert not A[:, ~bad, T:].view(np.uint32).any()
    # production, mode 0: the tap restates its score product
    q = torch.from_numpy(qkv).cuda().to(torch.bfloat16).contiguous()
    out = torch.empty((n, T, D), dtype=torch.bfloat16, device="cuda")
    _lib.check(lib.fav_op_attention(q.data_ptr(), out.data_ptr(), n, T, D, heads, 0, None))
    assert _lib.route_attention(n, T, D, heads, 0) == (0, _lib.last_route())
    torch.cuda.synchronize()
    exp = O.attention(qkv, heads, exact="mfma")
    assert np.isnan(exp[:, bad]).all() and np.isfinite(exp[:, ~bad]).all()
    assert R.same_bits(out.float().cpu().numpy(), exp)


def test_op_attn_mean_refusals_launch_nothing(lib):
    qkv = qkv_problem(1, 2, 17, 2)
    assert run_attn_mean(lib, qkv, 2)[0] == 0
    bad = [(dict(n=0), "n must"), (dict(T=1), "T=1"), (dict(T=257), "T=257"), (dict(heads=0), "heads=0"), (dict(heads=65, D=65 * 64), "heads=65"),
           (dict(D=192), "D=192"), (dict(D=64), "D=64"), (dict(null=("qkv",)), "null"), (dict(null=("a",)), "null"),
           (dict(off=dict(qkv=8)), "16-byte"), (dict(off=dict(a=4)), "16-byte")]
    for over, text in bad:
        st, _, guards, untouched = run_attn_mean(lib, qkv, 2, **over)
        msg = lib.fav_last_error(None).decode()
        assert st == 1 and "fav_op_attn_mean" in msg and text in msg, (over, msg)
        assert guards and untouched, over


# ---- fav_op_attn_rollout -----------------------------------------------------------------------------------------------------
def attention_problem(seed, L, n, T, ld):
    """Random row-stochastic fp32 A [L, n, T, ld] (softmax of N(0, 4) scores), columns >= T +0."""
    rng = np.random.default_rng(seed)
    s = rng.standard_normal((L, n, T, T)) * 2.0
    e = np.exp(s - s.max(-1, keepdims=True))
    A = np.zeros((L, n, T, ld), np.float32)
    A[..., :T] = (e / e.sum(-1, keepdims=True)).astype(np.float32)
    return A


def run_rollout(lib, A, grid_h, grid_w, first, **over):
    """-> (status, maps float32 [n, gh gw], records int32 [n, 8], guards untouched?, outputs untouched?)."""
    L, n, T, ld = A.shape
    HW = grid_h * grid_w
    a = dev(A)
    map_bytes, rec_bytes = n * HW * 4, n * 32
    m, rec = guarded(map_bytes), guarded(rec_bytes)
    args = dict(L=L, n=n, gh=grid_h, gw=grid_w, ld=ld, first_layer=first)
    null = over.pop("null", ())
    off = over.pop("off", dict())
    args.update(over)
    st = lib.fav_op_attn_rollout(None if "a" in null else a.data_ptr() + off.get("a", 0), args["L"], args["n"], args["gh"], args["gw"],
                                 args["ld"], args["first_layer"], None if "map" in null else m.data_ptr() + GUARD + off.get("map", 0),
                                 None if "rec" in null else rec.data_ptr() + GUARD + off.get("rec", 0), stream())
    torch.cuda.synchronize()
    mh, rh = m.cpu().numpy()[GUARD:GUARD + map_bytes], rec.cpu().numpy()[GUARD:GUARD + rec_bytes]
    untouched = bool((mh == FILL).all() and (rh == FILL).all())
    return (st, mh.copy().view(np.float32).reshape(n, HW), rh.copy().view(np.int32).reshape(n, 8),
            guards_ok(m, map_bytes) and guards_ok(rec, rec_bytes), untouched)


def records_equal(got, want):
    f = (1, 2, 4, 5)
    return bool(np.array_equal(np.delete(got, f, axis=-1), np.delete(want, f, axis=-1)) and
                R.same_bits(np.ascontiguousarray(got[..., f]).view(np.float32), np.ascontiguousarray(want[..., f]).view(np.float32)))


ROLL_CASES = [(hw, L, fl, n) for hw in [(1, 1), (2, 2), (4, 4), (14, 14), (15, 17)] for L in [1, 2, 12]
              for fl in sorted({0, L - 1}) for n in [1, 5]]


@pytest.mark.parametrize("hw,L,first_layer,n", ROLL_CASES)
def test_op_attn_rollout_matches_the_reference(lib, hw, L, first_layer, n):
    gh, gw = hw
    T = gh * gw + 1
    ld = R.attn_ld(T) if n == 1 else 4 * ((T + 3) // 4) + 4       # the tap's pitch, and another multiple of 4
    A = attention_problem(T * 1000 + L * 10 + n, L, n, T, ld)
    st, M, rec, guards, _ = run_rollout(lib, A, gh, gw, first_layer)
    assert st == 0 and guards
    Mr, rr = R.rollout(A, gh, gw, first_layer)
    assert R.same_bits(M, Mr)
    assert records_equal(rec, rr)
    r = unpack_rollout_records(rec)
    assert (r["n_layers"] == L - first_layer).all()
    if first_layer == L - 1:                                      # the raw last-layer class-token attention, mixed once
        assert R.same_bits(M, np.float32(0.5) * A[L - 1, :, 0, 1:T] + np.float32(0))
    # the overlay: fav_op_cam_heatmap takes the rollout records as they are
    H, W = 16 * gh, 16 * gw
    out = guarded(n * H * W)
    md, rd = dev(M), dev(rec)
    assert lib.fav_op_cam_heatmap(md.data_ptr(), rd.data_ptr(), n, gh, gw, H, W, out.data_ptr() + GUARD, stream()) == 0
    torch.cuda.synchronize()
    heat = out.cpu().numpy()[GUARD:GUARD + n * H * W].reshape(n, H, W)
    assert guards_ok(out, n * H * W) and np.array_equal(heat, cam_ref.heatmap(Mr, rr, gh, gw, H, W))
    if gh * gw > 1:
        # the pixel nearest the peak cell's centre lies 1 / 32 of a cell from it on either axis: weight (31 / 32)^2 on the peak
        assert heat.max() >= 239 and (r["peak"] > r["floor"]).all() and (r["n_above"] >= 1).all()
    else:
        assert not heat.any() and (r["box"] == -1).all()


def test_op_attn_rollout_refusals_launch_nothing(lib):
    A = attention_problem(3, 3, 2, 17, 32)
    assert run_rollout(lib, A, 4, 4, 0)[0] == 0
    bad = [(dict(L=0), "L=0"), (dict(L=65), "L=65"), (dict(n=0), "n must"), (dict(gh=0), "gh=0"), (dict(gw=-1), "gw=-1"),
           (dict(gh=16, gw=16), "cells"), (dict(gh=1, gw=256), "sides"), (dict(ld=16), "ld=16"), (dict(ld=18), "ld=18"),
           (dict(first_layer=-1), "first_layer=-1"), (dict(first_layer=3), "first_layer=3"),
           (dict(null=("a",)), "null"), (dict(null=("map",)), "null"), (dict(null=("rec",)), "null"),
           (dict(off=dict(a=2)), "4-byte"), (dict(off=dict(map=2)), "4-byte"), (dict(off=dict(rec=4)), "8-byte")]
    for over, text in bad:
        st, _, _, guards, untouched = run_rollout(lib, A, 4, 4, 0, **over)
        msg = lib.fav_last_error(None).decode()
        assert st == 1 and "fav_op_attn_rollout" in msg and text in msg, (over, msg)
        assert guards and untouched, over


# ---- end to end on synthetic checkpoints ---------------------------------------------------------------------------------------
QK_GAIN = 2.0            # the synthetic checkpoints of these tests: scaled scores of standard deviation ~4, peaked attention


@pytest.fixture(scope="module")
def b16_blobs():
    return {seed: weights.make_synthetic_vit("vit_b16", seed=seed, qk_gain=QK_GAIN)[0] for seed in (1, 2)}


def vit_case(case, b16_blobs, seed=1):
    """-> (arch, blob, (H, W), frames of a plain call)."""
    if case == "vit_b16":
        return "vit_b16", b16_blobs[seed], (224, 224), 2
    hw = {"tiny_32": (32, 32), "tiny_64": (64, 64), "tiny_48x64": (48, 64)}[case]
    return "vit_tiny", weights.make_synthetic_vit("vit_tiny", seed=seed, in_hw=hw, qk_gain=QK_GAIN)[0], hw, 3


@pytest.mark.parametrize("case", ["tiny_32", "tiny_64", "tiny_48x64", "vit_b16"])
def test_end_to_end(case, b16_blobs):
    arch, blob, (H, W), n = vit_case(case, b16_blobs)
    gh, gw = H // 16, W // 16
    T, HW = gh * gw + 1, gh * gw
    L = 12 if arch == "vit_b16" else 2
    many = torch.from_numpy(synth.synthetic_frames_u8(16, H, W, seed=11)).cuda()
    frames = many[:n]
    be = Backend(arch, blob, max_batch=16, in_hw=(H, W))
    try:
        assert be.attn_tap_info() == dict(bytes=L * 16 * T * R.attn_ld(T) * 4, layers=L, tokens=T, ld=R.attn_ld(T))
        # 1. the tap changes no result
        off = [t.cpu().numpy() for t in be.classify_detect(frames)] + [bits_of(be.logits())]
        off16 = bits_of((be.classify(many), be.logits())[1])
        be.set_attn_tap(True)
        be.set_feature_tap(True)
        on = [t.cpu().numpy() for t in be.classify_detect(frames)] + [bits_of(be.logits())]
        for a, b in zip(off, on):
            assert np.array_equal(a, b)
        # 2. the tapped A: its shape, its rows, and fav_rollout on it against the numpy rollout of it
        A = be.attention()
        assert tuple(A.shape) == (L, n, T, T) and A.dtype == torch.float32
        Ah = A.cpu().numpy()
        assert np.isfinite(Ah).all() and np.abs(Ah.astype(np.float64).sum(-1) - 1.0).max() < 1e-4
        for fl in (0, L - 1):
            got = be.rollout(first_layer=fl)
            Mr, rr = R.rollout(Ah, gh, gw, fl)
            assert R.same_bits(got["map"].cpu().numpy().reshape(n, HW), Mr), fl
            for key, v in unpack_rollout_records(rr).items():
                assert R.same_bits(got[key].cpu().numpy(), np.ascontiguousarray(v)), (fl, key)
        Mr, rr = R.rollout(Ah, gh, gw, 0)
        want = unpack_rollout_records(rr)
        # 3. classify_rollout: fav_classify_ex unchanged, then the head; the overlay from the rollout records
        out = be.classify_rollout(frames, heatmap=True)
        for a, key in zip(on, ("label", "conf", "fail", "score")):
            assert np.array_equal(a, out[key].cpu().numpy()), key
        assert np.array_equal(bits_of(be.attention()), Ah.view(np.uint32))
        assert R.same_bits(out["map"].cpu().numpy().reshape(n, HW), Mr)
        for key, v in want.items():
            assert R.same_bits(out[key].cpu().numpy(), np.ascontiguousarray(v)), key
        assert np.array_equal(out["heatmap"].cpu().numpy(), cam_ref.heatmap(Mr, rr, gh, gw, H, W))
        host = be.classify_rollout(frames.cpu().numpy())             # numpy in -> numpy out
        assert isinstance(host["map"], np.ndarray) and R.same_bits(host["map"], out["map"].cpu().numpy())
        for i in range(n):
            box = tuple(int(want[k][i]) for k in ("x0", "y0", "x1", "y1"))
            px = patch_box_to_pixels(box)
            assert (px is None) == (box[0] < 0) and (px is None or (0 <= px[0] < px[2] <= W and 0 <= px[1] < px[3] <= H))
        # 4. sixteen frames in one call - two parts on two streams, each at its frame offset - against sixteen calls of one
        big = be.classify_rollout(many)
        assert np.array_equal(bits_of(be.logits()), off16)
        A16 = bits_of(be.attention())
        assert A16.shape == (L, 16, T, T)
        for i in range(16):
            one = be.classify_rollout(many[i:i + 1])
            assert np.array_equal(bits_of(be.attention())[:, 0], A16[:, i]), i
            for key in ("map", "n_layers", "cls_mass", "peak", "peak_cell", "floor", "patch_sum", "n_above", "box"):
                assert R.same_bits(one[key].cpu().numpy()[0], big[key].cpu().numpy()[i]), (i, key)
        # 5. off and on again
        be.set_attn_tap(False)
        with pytest.raises(_lib.FavError, match="attention tap is off"):
            be.attention()
        assert np.array_equal(bits_of((be.classify(frames), be.logits())[1]), on[4])
        be.set_attn_tap(True)
        again = be.classify_rollout(frames)
        assert R.same_bits(again["map"].cpu().numpy().reshape(n, HW), Mr)
        assert np.array_equal(bits_of(be.attention()), Ah.view(np.uint32))
    finally:
        be.close()


# ---- the maps against float64 ------------------------------------------------------------------------------------------------------
# The device map of a frame against tests/rollout_ref.py's float64 rollout of the float64 encoder on the same frame, as the worst
# absolute difference over the map relative to the float64 map's peak - floor.  The bound cannot be derived (bf16 at every tensor
# boundary, up to 12 layers deep); it is 4x the worst value measured on an MI355X over the test's frames and the two checkpoint
# seeds, the margin being for other seeds.  Measured (checkpoints built with qk_gain = 2): vit_tiny at 64 x 64, 8 frames a
# seed, 1.905e-02; vit_b16 at 224 x 224, 2 frames a seed, 6.363e-03.  On the same frames the float64 map without the identity
# term lies at least 0.614 (vit_tiny) and 0.264 (vit_b16) from the float64 rollout, the last layer alone 0.282 and 0.753.
F64_MEASURED = {"tiny_64": 1.905e-02, "vit_b16": 6.363e-03}
F64_BOUND = {k: 4.0 * v for k, v in F64_MEASURED.items()}


@pytest.mark.parametrize("case", ["tiny_64", "vit_b16"])
def test_maps_against_float64(case, b16_blobs):
    worst, least_noid, least_last = 0.0, np.inf, np.inf
    for seed in (1, 2):
        arch, blob, (H, W), _ = vit_case(case, b16_blobs, seed)
        n = 2 if arch == "vit_b16" else 8
        u8 = synth.synthetic_frames_u8(n, H, W, seed=31)
        be = Backend(arch, blob, max_batch=n, in_hw=(H, W))
        try:
            be.set_attn_tap(True)
            got = be.classify_rollout(torch.from_numpy(u8).cuda())["map"].cpu().numpy().reshape(n, -1).astype(np.float64)
        finally:
            be.close()
        A64 = R.classify_attention_f64(blob, u8, device="cuda")
        ref = R.rollout_f64(A64)
        span = ref.max(1) - ref.min(1)
        rel = lambda m: np.abs(m - ref).max(1) / span
        worst = max(worst, rel(got).max())
        least_noid = min(least_noid, rel(R.rollout_f64(A64, identity=False)).min())
        least_last = min(least_last, rel(R.rollout_f64(A64, first_layer=A64.shape[0] - 1)).min())
    note(f"rollout {case} vs float64: worst |device - float64| / (peak - floor) {worst:.3e} (bound {F64_BOUND[case]:.3e}); "
         f"float64 without the identity term at least {least_noid:.3e} away, last layer only at least {least_last:.3e}")
    assert worst < F64_BOUND[case]
    # the bound discriminates: forgetting the residual connection's identity, or rolling out one layer only, lies farther away
    assert least_noid > F64_BOUND[case] and least_last > F64_BOUND[case]


# ---- refusals --------------------------------------------------------------------------------------------------------------------
def test_tap_refused_on_a_resnet_an_ensemble_and_the_exact_mode(r18_blob):
    r18 = Backend("resnet18_cifar", r18_blob[0], max_batch=4)
    try:
        with pytest.raises(_lib.FavError, match="FAV_ERR_UNSUPPORTED.*fav_set_attn_tap.*ResNet"):
            r18.set_attn_tap(True)
        r18.set_attn_tap(False)                                 # turning it off is never refused
        with pytest.raises(_lib.FavError, match="FAV_ERR_UNSUPPORTED.*fav_attn_tap_info.*ResNet"):
            r18.attn_tap_info()
    finally:
        r18.close()
    ens = Backend("resnet18_cifar", [r18_blob[0], r18_blob[0]], max_batch=4)
    try:
        with pytest.raises(_lib.FavError, match="FAV_ERR_UNSUPPORTED.*fav_set_attn_tap.*ensemble"):
            ens.set_attn_tap(True)
        ens.set_attn_tap(False)
    finally:
        ens.close()
    vblob, _ = weights.make_synthetic_vit("vit_tiny", seed=3)
    exact = Backend("vit_tiny", vblob, max_batch=4, math_mode="f32_exact")
    try:
        with pytest.raises(_lib.FavError, match="FAV_ERR_UNSUPPORTED.*fav_set_attn_tap.*FAV_MATH_F32_EXACT"):
            exact.set_attn_tap(True)
        exact.set_attn_tap(False)
    finally:
        exact.close()


def test_handle_refusals():
    vblob, _ = weights.make_synthetic_vit("vit_tiny", seed=3)
    frames = torch.from_numpy(synth.synthetic_frames_u8(4, 64, 64, seed=3)).cuda()
    be = Backend("vit_tiny", vblob, max_batch=8)
    try:
        m = torch.full((4, 16), 7.0, dtype=torch.float32, device="cuda")
        rec = torch.full((4, 8), 7, dtype=torch.int32, device="cuda")

        def fav_rollout(first_layer=0):
            st = be.lib.fav_rollout(be._h, first_layer, m.data_ptr(), rec.data_ptr(), stream())
            return st, be.lib.fav_last_error(be._h).decode()
        be.classify(frames)
        # the tap off
        st, msg = fav_rollout()
        assert st == 1 and "fav_rollout: the attention tap is off" in msg
        with pytest.raises(_lib.FavError, match="FAV_ERR_INVALID_ARG.*fav_rollout: the attention tap is off"):
            be.rollout()
        with pytest.raises(_lib.FavError, match="FAV_ERR_INVALID_ARG.*fav_classify_rollout: the attention tap is off"):
            be.classify_rollout(frames)
        # over the budget: both numbers
        need = 2 * 8 * 17 * 32 * 4
        assert be.attn_tap_info()["bytes"] == need
        with pytest.raises(_lib.FavError, match=f"FAV_ERR_INVALID_ARG.*fav_set_attn_tap.*{need} bytes.*max_bytes={need - 1}"):
            be.set_attn_tap(True, budget_bytes=need - 1)
        be.set_attn_tap(True, budget_bytes=need)
        # before a tapped call
        st, msg = fav_rollout()
        assert st == 1 and "fav_rollout: no classify call since the tap was turned on" in msg
        with pytest.raises(_lib.FavError, match="fav_get_attention: no classify call"):
            be.attention()
        with pytest.raises(_lib.FavError, match="FAV_ERR_INVALID_ARG.*fav_rollout: no classify call"):
            be.rollout()
        be.classify(frames)
        st, msg = fav_rollout(first_layer=2)
        assert st == 1 and "fav_rollout: first_layer=2" in msg
        st, msg = fav_rollout(first_layer=-1)
        assert st == 1 and "fav_rollout: first_layer=-1" in msg
        torch.cuda.synchronize()
        assert (m == 7.0).all() and (rec == 7).all()             # nothing has been launched so far
        assert fav_rollout()[0] == 0
        plain = bits_of(be.attention())
        # views: the attention is there, the head is not
        be.set_views(views.hflip())                              # the frame and its mirror image
        st, msg = fav_rollout()
        assert st == 6 and "fav_rollout: views are set" in msg
        with pytest.raises(_lib.FavError, match="FAV_ERR_UNSUPPORTED.*fav_classify_rollout: views are set"):
            be.classify_rollout(frames)
        be.classify(frames)
        A = be.attention()
        assert tuple(A.shape) == (2, 8, 17, 17)                  # frames x views rows, [view][frame] like the logits
        assert np.array_equal(bits_of(A[:, :4]), plain)          # the identity's rows first
        assert not np.array_equal(bits_of(A[:, 4:]), plain)
        be.set_views(None)
        st, msg = fav_rollout()
        assert st == 6 and "fav_rollout: the last call ran under views" in msg
        be.classify(frames)
        assert fav_rollout()[0] == 0
        be.set_attn_tap(False)
        be.set_attn_tap(False)
    finally:
        be.close()
