"""Mid-level patch maps on the device: fav_op_patch_query against tests/patch_local_ref.py, the
stage tap against the oracle walked block by block, and a bank at a site end to end.

Everything here is an equality of bits.  The query's every operation is fixed by the contract beside fav_patch_site, so q and
the flags are the reference's; the stage tap is a copy of a tensor the oracle models bit for bit.

Shapes of the op: the grids 1x1 (every neighbour out of range), 1x5, 5x1, 2x3, 3x3, 7x7, 14x9, 28x28, 4x256 and 256x4; C in
{64, 192, 512, 1024, 4096}; S in {1, 3}; n in {1, 2, 5}; radius in {0, 1, 2} - a subset of the product that holds each value,
plus every grid at C = 64, radius 2.  A block owns a frame row and works through channel slices where a row does not fit its
64 KB of LDS: 4x256 at C = 64 is two slices (48 + 16 channels), 28x28 at C = 1024 two (560 + 464), 14x9 at C = 4096 three,
256x4 at C = 4096 two, the last one sixteen channels wide.  Every output lies between guard bytes."""
import ctypes as C

import numpy as np
import pytest

pytestmark = pytest.mark.gpu

torch = pytest.importorskip("torch")
import cam_ref  # noqa: E402
import knn_ref as K  # noqa: E402
import patch_local_ref as L  # noqa: E402
import patch_ref as R  # noqa: E402
from failure_aware_vision_amd import Backend, _lib, synth, weights  # noqa: E402
from failure_aware_vision_amd.patch import PatchBank  # noqa: E402
from oracle import fav_oracle as O  # noqa: E402
from test_gpu_patch import (FILL, MC, bits_of, dev, guarded, guards_ok, numpy_of, records_of, run_op, same,  # noqa: E402
                            unit_rows)


@pytest.fixture(scope="module")
def lib():
    assert torch.cuda.is_available(), "GPU tests need a MI355X"
    return _lib.load()


def stream():
    return torch.cuda.current_stream().cuda_stream


def run_query(lib, maps_bits, grid, radius, q_off=0, flags_off=0, null=(), **over):
    """fav_op_patch_query -> (status, q uint16 [n * HW, C], flags int32 [n * HW], guard bytes untouched?).  Each output lies
    behind a guard in a buffer filled with FILL, *_off bytes further in.  over: S, n, Hf, Wf, C as passed, where they differ
    from the array's; null: arguments to pass as NULL."""
    S0, n0, HW, C0 = maps_bits.shape
    Hf, Wf = grid
    assert Hf * Wf == HW
    mbuf = dev(maps_bits.ravel().view(np.int16))
    assert mbuf.data_ptr() % 16 == 0
    nq, nf = 2 * n0 * HW * C0, 4 * n0 * HW
    qbuf, qlo = guarded(nq, q_off)
    fbuf, flo = guarded(nf, flags_off)
    ptr = dict(maps=mbuf.data_ptr(), q=qbuf.data_ptr() + qlo, flags=fbuf.data_ptr() + flo)
    for name in null:
        ptr[name] = None
    st = lib.fav_op_patch_query(ptr["maps"], over.get("S", S0), over.get("n", n0), over.get("Hf", Hf), over.get("Wf", Wf),
                                over.get("C", C0), radius, ptr["q"], ptr["flags"], stream())
    torch.cuda.synchronize()
    qh, fh = qbuf.cpu().numpy(), fbuf.cpu().numpy()
    guards = guards_ok(qh, qlo, nq) and guards_ok(fh, flo, nf)
    return (st, qh[qlo:qlo + nq].copy().view(np.uint16).reshape(n0 * HW, C0), fh[flo:flo + nf].copy().view(np.int32), guards)


def want_query(maps_bits, grid, radius):
    q, _, bad = L.query(maps_bits, grid, radius)
    return K.f32_to_bf16_bits(q), bad.astype(np.int32)


def maps_of(Cc, grid, n, S, seed=0):
    rng = np.random.default_rng(1000 * Cc + 100 * grid[0] + grid[1] + 10 * S + n + seed)
    return K.f32_to_bf16_bits(rng.standard_normal((S, n, grid[0] * grid[1], Cc)).astype(np.float32))


GRIDS = [(1, 1), (1, 5), (5, 1), (2, 3), (3, 3), (7, 7), (14, 9), (28, 28), (4, 256), (256, 4)]
# (grid, C, S, n, radius): every value at least once, the slicing cases of the module's docstring among them
SHAPES = [((1, 1), 64, 1, 1, 0), ((1, 5), 192, 3, 2, 1), ((5, 1), 512, 1, 5, 2), ((2, 3), 1024, 3, 1, 1), ((3, 3), 4096, 1, 2, 2),
          ((7, 7), 512, 3, 5, 1), ((14, 9), 4096, 1, 1, 1), ((28, 28), 1024, 1, 2, 1), ((28, 28), 512, 3, 1, 0), ((4, 256), 64, 3, 1, 1),
          ((256, 4), 4096, 1, 1, 0), ((256, 4), 192, 1, 2, 2), ((7, 7), 2048, 1, 2, 0)]
SHAPES += [(g, 64, 1, 2, 2) for g in GRIDS]


@pytest.mark.parametrize("shape", SHAPES, ids=["-".join(str(v).replace(", ", "x").strip("()") for v in s) for s in SHAPES])
def test_query_bit_exact(lib, shape):
    grid, Cc, S, n, radius = shape
    maps = maps_of(Cc, grid, n, S)
    wq, wf = want_query(maps, grid, radius)
    st, q, flags, guards = run_query(lib, maps, grid, radius)
    assert st == 0 and guards
    assert np.array_equal(flags, wf) and not wf.any()
    assert np.array_equal(q, wq), np.flatnonzero((q != wq).any(axis=1))[:8]


@pytest.mark.parametrize("radius", (0, 1, 2))
def test_query_never_reads_across_a_frame(lib, radius):
    """The frames around frame 1 hold values 2^20 times larger: one read across a frame boundary changes bits."""
    grid = (3, 4)
    maps = maps_of(128, grid, 3, 2, seed=radius)
    rng = np.random.default_rng(9)
    for i in (0, 2):
        maps[:, i] = K.f32_to_bf16_bits((rng.standard_normal((2, 12, 128)) * 2.0 ** 20).astype(np.float32))
    wq, wf = want_query(maps, grid, radius)
    alone, _ = want_query(maps[:, 1:2], grid, radius)
    assert np.array_equal(wq[12:24], alone)                                          # the reference itself: frame 1 on its own
    st, q, flags, guards = run_query(lib, maps, grid, radius)
    assert st == 0 and guards and np.array_equal(q, wq) and np.array_equal(flags, wf)


@pytest.mark.parametrize("radius", (1, 2))
def test_query_an_overflowing_cell_stays_in_its_neighbourhood(lib, radius):
    """One cell holds bf16 max in a channel: the squared norm of every neighbourhood that holds it is not finite - flag 1 and a
    zero row - and the cells farther than the radius are what they are without it.  Frame 1 is all zero: every cell flagged."""
    grid = (7, 6)
    clean = maps_of(64, grid, 2, 1, seed=3)
    clean[:, 1] = 0
    maps = clean.copy()
    maps[0, 0, 3 * 6 + 2, 5] = 0x7F7F                                                # cell (3, 2) of frame 0
    wq, wf = want_query(maps, grid, radius)
    cq, _ = want_query(clean, grid, radius)
    hit = np.zeros((7, 6), bool)
    hit[3 - radius:3 + radius + 1, max(0, 2 - radius):2 + radius + 1] = True
    assert np.array_equal(wf[:42].reshape(7, 6).astype(bool), hit) and wf[42:].all()
    st, q, flags, guards = run_query(lib, maps, grid, radius)
    assert st == 0 and guards and np.array_equal(flags, wf) and np.array_equal(q, wq)
    assert (q[:42][hit.ravel()] == 0).all() and (q[42:] == 0).all()
    assert np.array_equal(q[:42][~hit.ravel()], cq[:42][~hit.ravel()])              # cells beyond the radius: untouched


def test_query_a_zero_cell_with_neighbours_has_a_direction(lib):
    grid = (4, 4)
    maps = maps_of(64, grid, 1, 3, seed=4)
    maps[:, 0, 5] = 0
    for radius, flag in ((0, 1), (1, 0), (2, 0)):
        wq, wf = want_query(maps, grid, radius)
        st, q, flags, guards = run_query(lib, maps, grid, radius)
        assert st == 0 and guards and np.array_equal(q, wq) and np.array_equal(flags, wf) and flags[5] == flag and flags.sum() == flag


@pytest.mark.parametrize("shape", [((2, 3), 64, 3, 5), ((7, 7), 512, 1, 2), ((4, 4), 2048, 3, 2)])
def test_radius_0_is_the_existing_query_path(lib, shape):
    """fav_op_patch_score leaves the k-NN head's q and flags at the front of its workspace (q at 0, the flags behind it on the
    next 256-byte boundary): fav_op_patch_query at radius 0 gives the same bytes, and fav_op_patch_score_at(.., 0, ..) the same
    dist, row and records as fav_op_patch_score."""
    grid, Cc, S, n = shape
    maps = maps_of(Cc, grid, n, S, seed=5)
    maps[:, 0, 1] = 0                                                                # a degenerate cell
    bank = unit_rows(np.random.default_rng(5), 70, Cc)
    M = n * grid[0] * grid[1]
    thr = 1.0

    def score(radius):
        need = lib.fav_patch_workspace_bytes(M, Cc, 70, 64)
        ws = torch.full((need,), FILL, dtype=torch.uint8, device="cuda")
        mbuf, bbuf = dev(maps.ravel().view(np.int16)), dev(bank.ravel().view(np.int16))
        d = torch.empty((n, M // n), dtype=torch.float32, device="cuda")
        r = torch.empty((n, M // n), dtype=torch.int32, device="cuda")
        c = torch.empty((n, 8), dtype=torch.int32, device="cuda")
        head = (mbuf.data_ptr(), S, n, grid[0], grid[1], Cc, bbuf.data_ptr(), 70, 64, thr)
        tail = (ws.data_ptr(), need, d.data_ptr(), r.data_ptr(), c.data_ptr(), stream())
        st = lib.fav_op_patch_score(*head, *tail) if radius is None else lib.fav_op_patch_score_at(*head, radius, *tail)
        torch.cuda.synchronize()
        assert st == 0, lib.fav_last_error(None).decode()
        w = ws.cpu().numpy()
        flags_at = (M * Cc * 2 + 255) & ~255
        return (d.cpu().numpy(), r.cpu().numpy(), c.cpu().numpy(), w[:M * Cc * 2].copy().view(np.uint16).reshape(M, Cc),
                w[flags_at:flags_at + 4 * M].copy().view(np.int32))
    old, new = score(None), score(0)
    for a, b in zip(old, new):
        assert np.array_equal(a.view(np.uint8), b.view(np.uint8))
    st, q, flags, guards = run_query(lib, maps, grid, 0)
    assert st == 0 and guards and np.array_equal(q, old[3]) and np.array_equal(flags, old[4]) and flags[1] == 1
    assert same(old[:3], R.score(maps, bank, grid[1], thr))
    # and at a radius the whole head is the reference's
    got = score(1)
    assert same(got[:3], L.score_at(maps, bank, grid[1], thr, 1))


QUERY_REFUSALS = [("radius 3", 3, dict(), "radius=3"), ("radius -1", -1, dict(), "radius=-1"), ("C 96", 1, dict(C=96), "C=96"),
                  ("C 4160", 1, dict(C=4160), "C=4160"), ("q + 8", 1, dict(q_off=8), "16-byte"), ("flags NULL", 1, dict(null=("flags",)), "null"),
                  ("q NULL", 1, dict(null=("q",)), "null"), ("maps NULL", 1, dict(null=("maps",)), "null"), ("flags + 2", 1, dict(flags_off=2), "4-byte"),
                  ("S 0", 1, dict(S=0), "S=0"), ("n 0", 1, dict(n=0), "n must"), ("HW 1025", 1, dict(Hf=25, Wf=41), "Hf=25 x Wf=41"),
                  ("Wf 257", 1, dict(Hf=1, Wf=257), "Wf=257")]


@pytest.mark.parametrize("why,radius,kw,text", QUERY_REFUSALS, ids=[r[0] for r in QUERY_REFUSALS])
def test_query_refusals_launch_nothing(lib, why, radius, kw, text):
    maps = maps_of(64, (2, 3), 2, 1)
    st, q, flags, guards = run_query(lib, maps, (2, 3), radius, **kw)
    msg = lib.fav_last_error(None).decode()
    assert st == 1 and "fav_op_patch_query" in msg and text in msg, (why, msg)
    assert guards and (q.view(np.uint8) == FILL).all() and (flags.view(np.uint8) == FILL).all()


def test_score_at_refusals(lib):
    maps, bank = maps_of(64, (2, 3), 2, 1), unit_rows(np.random.default_rng(0), 17, 64)
    need = lib.fav_patch_workspace_bytes(12, 64, 17, 0)
    ws = torch.full((need,), FILL, dtype=torch.uint8, device="cuda")
    mbuf, bbuf = torch.zeros(maps.size + 8, dtype=torch.int16, device="cuda"), dev(bank.ravel().view(np.int16))
    d = torch.full((2, 6), 3.0, dtype=torch.float32, device="cuda")
    c = torch.full((2, 8), 77, dtype=torch.int32, device="cuda")
    for radius, off, text in ((3, 0, "radius=3"), (-1, 0, "radius=-1"), (1, 2, "maps_bf16 must be 16-byte aligned")):
        st = lib.fav_op_patch_score_at(mbuf.data_ptr() + off, 1, 2, 2, 3, 64, bbuf.data_ptr(), 17, 0, 1.0, radius, ws.data_ptr(), need,
                                       d.data_ptr(), None, c.data_ptr(), stream())
        msg = lib.fav_last_error(None).decode()
        assert st == 1 and "fav_op_patch_score_at" in msg and text in msg, msg
    torch.cuda.synchronize()
    assert (d == 3.0).all() and (c == 77).all() and (ws == FILL).all()


# ---- the stage tap ---------------------------------------------------------------------------------------------------------------
STAGE_ENDS = {"resnet50": (2, 6, 12, 15), "resnet18_cifar": (1, 3, 5, 7)}
TAP = {"r18_32": dict(arch="resnet18_cifar", hw=(32, 32), n=5), "r18_31x45": dict(arch="resnet18_cifar", hw=(31, 45), n=5),
       "r50_64": dict(arch="resnet50", hw=(64, 64), n=2), "r50_33x47": dict(arch="resnet50", hw=(33, 47), n=2)}
_WALKS = {}


def oracle_stages(case, blob, mc):
    """The oracle walked block by block -> {stage: float32 [S, n, H, W, C]} for stages 1 .. 4, once per (case, mode), shared
    read-only.  Single pass: S = 1.  MC-Dropout over all blocks: block 0 runs once, its dropped copies (the entry dropout)
    feed blocks 1 .. of every sample, each drawing its own site."""
    key = (case, mc)
    if key not in _WALKS:
        c = TAP[case]
        net = O.OracleNet(O.parse_blob(blob), exact="mfma")
        frames = synth.synthetic_frames_u8(c["n"], c["hw"][0], c["hw"][1], seed=11)
        cfg = O.ClassifyConfig()
        xn = O.normalize_input(frames, cfg.mean, O.inv_std32(cfg.std))
        ids = np.arange(c["n"])
        ends = STAGE_ENDS[c["arch"]]
        out = {s: [] for s in (1, 2, 3, 4)}
        act = net.stem(xn)
        if not mc:
            for i in range(net.nb):
                act = net.block(i, act)
                if i in ends:
                    out[ends.index(i) + 1].append(act)
        else:
            mask = weights.site_mask_for(weights.ARCH_IDS[c["arch"]], "all_blocks")
            thr = O.dropout_threshold(MC["dropout_p"])
            scale = O.dropout_scale(thr)
            act = net.block(0, act)
            for t in range(MC["n_samples"]):
                keep = O.dropout_keep(MC["seed"], t, 0, ids, int(np.prod(act.shape[1:])), thr)
                a = O.bf16_round(np.where(keep.reshape(act.shape), act * scale, np.float32(0.0)).astype(np.float32))
                for i in range(1, net.nb):
                    a = net._block_with_site(i, a, t, ids, mask, MC["seed"], thr, scale)
                    if i in ends:
                        out[ends.index(i) + 1].append(a)
        _WALKS[key] = {s: np.stack(v) for s, v in out.items()}
        for v in _WALKS[key].values():
            v.flags.writeable = False
        _WALKS[key]["frames"] = frames
    return _WALKS[key]


def stage_sizes(be):
    v = [C.c_int32() for _ in range(6)]
    st = be.lib.fav_get_stage_maps(be._h, None, *(C.byref(x) for x in v), None)
    return st, tuple(x.value for x in v)


@pytest.mark.parametrize("mc", (False, True), ids=["single", "mc"])
@pytest.mark.parametrize("case", list(TAP))
def test_stage_tap_is_the_oracles_block_output(lib, case, mc, r18_blob, r50_blob):
    c = TAP[case]
    blob = (r18_blob if c["arch"] == "resnet18_cifar" else r50_blob)[0]
    want = oracle_stages(case, blob, mc)
    frames = dev(want["frames"])
    n, S = c["n"], (MC["n_samples"] if mc else 1)
    be = Backend(c["arch"], blob, max_batch=8, in_hw=c["hw"], **(MC if mc else {}))
    try:
        plain = [t.cpu().numpy() for t in be.classify_detect(frames)]
        plain_logits = be.logits().cpu().numpy()
        for stage in (2, 3, 4):
            info = be.stage_tap_info(stage)
            be.set_stage_tap(stage)
            got = [t.cpu().numpy() for t in be.classify_detect(frames)]
            for a, b in zip(plain, got):                                             # labels, confidences, flags, scores: unchanged
                assert np.array_equal(a.view(np.uint8), b.view(np.uint8))
            assert np.array_equal(plain_logits.view(np.uint8), be.logits().cpu().numpy().view(np.uint8))
            maps = be.stage_maps()
            assert stage_sizes(be) == (0, (stage, S, n, info["hf"], info["wf"], info["c"])) and info["samples"] == S
            assert tuple(maps.shape) == (S, n, info["hf"], info["wf"], info["c"]) == want[stage].shape
            assert info["bytes"] == S * 8 * info["hf"] * info["wf"] * info["c"] * 2
            assert np.array_equal(bits_of(maps), K.f32_to_bf16_bits(want[stage])), stage
        # stage 4 is the map tap, with both on
        be.set_map_tap(True)
        be.classify(frames)
        assert np.array_equal(bits_of(be.stage_maps()), bits_of(be.maps()))
        assert be.map_tap_info() == be.stage_tap_info(4)
        # changing the stage empties the tap; off: fav_get_stage_maps refuses
        be.set_stage_tap(3)
        st, _ = stage_sizes(be)
        assert st == 1 and "no classify call since the tap was turned on" in lib.fav_last_error(be._h).decode()
        be.classify(frames)
        assert stage_sizes(be)[1][0] == 3 and np.array_equal(bits_of(be.stage_maps()), K.f32_to_bf16_bits(want[3]))
        be.set_stage_tap(0)
        assert stage_sizes(be)[0] == 1 and "the stage tap is off (fav_set_stage_tap)" in lib.fav_last_error(be._h).decode()
        assert lib.fav_get_maps(be._h, None, None, None, None, None, None, None) == 0   # the map tap is its own affair
    finally:
        be.close()


@pytest.mark.parametrize("case", ("r18_32", "r50_64"))
def test_stage_tap_does_not_depend_on_the_passes(lib, case, r18_blob, r50_blob):
    """MC-Dropout over all blocks: handles whose phases run in several passes (chunks 2,7 and 1,1, max_batch above the call) and
    whose low-resolution group starts on either side of the tapped stage's last block give the tap bytes of a one-pass handle."""
    c = TAP[case]
    blob = (r18_blob if c["arch"] == "resnet18_cifar" else r50_blob)[0]
    frames = dev(synth.synthetic_frames_u8(c["n"], c["hw"][0], c["hw"][1], seed=11))
    n = c["n"]

    def taps(**kw):
        be = Backend(c["arch"], blob, in_hw=c["hw"], **dict(dict(max_batch=n), **kw), **MC)
        try:
            out = {}
            for stage in (2, 3, 4):
                be.set_stage_tap(stage)
                be.classify(frames)
                out[stage] = bits_of(be.stage_maps())
            return out
        finally:
            be.close()
    one = taps()
    ends = STAGE_ENDS[c["arch"]]
    knobs = [dict(chunk_a=2, chunk_b=7), dict(chunk_a=1, chunk_b=1), dict(max_batch=2 * n + 3, chunk_a=2, chunk_b=7)]
    knobs += [dict(regroup_block=ends[s - 1] + d, chunk_a=2, chunk_b=3) for s in (2, 3) for d in (0, 1)]
    for kw in knobs:
        got = taps(**kw)
        for stage in (2, 3, 4):
            assert np.array_equal(got[stage], one[stage]), (kw, stage)


def test_stage_tap_refusals(lib, r18_blob, r50_blob):
    vblob, _ = weights.make_synthetic_vit("vit_tiny", seed=3)
    vit = Backend("vit_tiny", vblob, max_batch=4)
    ens = Backend("resnet18_cifar", [r18_blob[0], weights.make_synthetic("resnet18_cifar", seed=2)[0]], max_batch=4)
    be = Backend("resnet18_cifar", r18_blob[0], max_batch=8)
    big = Backend("resnet50", r50_blob[0], max_batch=2, in_hw=(224, 224))
    try:
        for h, word in ((vit, "ViT"), (ens, "ensemble")):
            assert lib.fav_set_stage_tap(h._h, 2, 0) == 6 and word in lib.fav_last_error(h._h).decode()
            with pytest.raises(_lib.FavError, match="FAV_ERR_UNSUPPORTED.*fav_set_stage_tap"):
                h.set_stage_tap(2)
            assert lib.fav_set_stage_tap(h._h, 0, 0) == 0                              # off is never refused
        for stage in (-1, 5):
            assert lib.fav_set_stage_tap(be._h, stage, 0) == 1 and f"stage={stage} outside [0, 4]" in lib.fav_last_error(be._h).decode()
        # the budget refusal carries the numbers: stage 2 of max_batch = 8 frames is 8 x 16 x 16 x 128 x 2 bytes
        info = be.stage_tap_info(2)
        assert info["bytes"] == 8 * 16 * 16 * 128 * 2
        with pytest.raises(_lib.FavError, match=rf"fav_set_stage_tap: .*{info['bytes']} bytes, above max_bytes={info['bytes'] - 1}"):
            be.set_stage_tap(2, info["bytes"] - 1)
        assert be._stage_tap == 0 and stage_sizes(be)[0] == 1
        be.set_stage_tap(2, info["bytes"])
        # a refused change of stage leaves the tap as it was
        frames = dev(synth.synthetic_frames_u8(3, 32, 32, seed=1))
        be.classify(frames)
        with pytest.raises(_lib.FavError, match="above max_bytes=1"):
            be.set_stage_tap(3, 1)
        assert stage_sizes(be) == (0, (2, 1, 3, 16, 16, 128))
        # a map the patch head cannot take: stage 1 of a 224 x 224 frame has 56 x 56 = 3136 cells
        assert big.stage_tap_info(1)["hf"] == 56
        with pytest.raises(_lib.FavError, match=r"fav_set_stage_tap: stage 1: Hf=56 x Wf=56: a map has 1 to 1024 cells"):
            big.set_stage_tap(1)
        big.set_stage_tap(2)
    finally:
        for h in (vit, ens, be, big):
            h.close()


# ---- a bank at a site, end to end -----------------------------------------------------------------------------------------------
E2E = {"r18_single": ("r18_32", False), "r50_mc": ("r50_64", True), "r18_31x45_mc": ("r18_31x45", True), "r50_33x47_single": ("r50_33x47", False)}


@pytest.mark.parametrize("site", [(2, 0), (2, 1), (3, 0), (3, 1)], ids=lambda s: f"stage{s[0]}-r{s[1]}")
@pytest.mark.parametrize("case", list(E2E))
def test_end_to_end_at_a_site(lib, case, site, r18_blob, r50_blob):
    tap, mc = E2E[case]
    c = TAP[tap]
    stage, radius = site
    blob = (r18_blob if c["arch"] == "resnet18_cifar" else r50_blob)[0]
    n, hw = c["n"], c["hw"]
    frames = dev(synth.synthetic_frames_u8(n, hw[0], hw[1], seed=11))
    fit = dev(synth.synthetic_frames_u8(11, hw[0], hw[1], seed=12))                  # two batches of max_batch = 8
    be = Backend(c["arch"], blob, max_batch=8, in_hw=hw, **(MC if mc else {}))
    try:
        info = be.stage_tap_info(stage)
        Hf, Wf, Cc, S = info["hf"], info["wf"], info["c"], info["samples"]
        plain = [t.cpu().numpy() for t in be.classify_detect(frames)]
        bank = be.fit_patch_bank(fit, stage=stage, radius=radius, max_rows=100, seed=3)
        assert (bank.N, bank.D, bank.grid, bank.stage, bank.radius) == (min(100, 11 * Hf * Wf - bank.n_dropped), Cc, (Hf, Wf), stage, radius)
        assert be._stage_tap == 0 and stage_sizes(be)[0] == 1                        # fit_patch_bank left the tap as it was: off
        be.set_patch_bank(bank)
        assert be.patch_bank is bank and stage_sizes(be)[0] == 1                     # the setter does not touch the tap
        first = numpy_of(be.classify_patch(frames, heatmap=True))                    # the tap goes on for the call, and off again
        assert be._stage_tap == 0 and stage_sizes(be)[0] == 1
        be.set_stage_tap(stage)
        got = numpy_of(be.classify_patch(frames, heatmap=True))
        assert be._stage_tap == stage
        for key in got:
            assert np.array_equal(first[key], got[key], equal_nan=True), key
        for key, want in zip(("label", "conf", "fail", "score"), plain):            # fav_classify_ex, unchanged
            assert np.array_equal(got[key].view(np.uint8), want.view(np.uint8)), key
        maps = be.stage_maps()
        assert tuple(maps.shape) == (S, n, Hf, Wf, Cc)
        xb = bits_of(maps).reshape(S, n, Hf * Wf, Cc)
        dist, row, rec = L.score_at(xb, bank.rows, Wf, bank.threshold, radius)
        assert got["dist"].shape == (n, Hf, Wf) and got["nn_row"].shape == (n, Hf, Wf)
        assert same((got["dist"].reshape(n, -1), got["nn_row"].reshape(n, -1), records_of(got)), (dist, row, rec))
        assert np.array_equal(got["heatmap"], cam_ref.heatmap(dist, rec, Hf, Wf, hw[0], hw[1]))
        assert (np.nan_to_num(dist) > 0).any()
        # fav_patch on the maps of the last call: the same bytes
        d2 = torch.empty((n, Hf * Wf), dtype=torch.float32, device="cuda")
        r2 = torch.empty((n, Hf * Wf), dtype=torch.int32, device="cuda")
        c2 = torch.empty((n, 8), dtype=torch.int32, device="cuda")
        assert lib.fav_patch(be._h, d2.data_ptr(), r2.data_ptr(), c2.data_ptr(), stream()) == 0
        assert same((d2.cpu().numpy(), r2.cpu().numpy(), c2.cpu().numpy()), (dist, row, rec))
        # a threshold inside the range of the cells, through the handle
        thr = float(np.sort(dist.ravel())[dist.size // 2])
        be.set_patch_bank(bank.with_threshold(thr))
        flagged = numpy_of(be.classify_patch(frames))
        assert same((flagged["dist"].reshape(n, -1), flagged["nn_row"].reshape(n, -1), records_of(flagged)),
                    L.score_at(xb, bank.rows, Wf, thr, radius))
        assert 0 < flagged["n_above"].sum() < dist.size
        be.set_patch_bank(None)
        assert be.patch_bank is None and stage_sizes(be)[0] == 0                     # clearing the bank leaves the caller's tap
    finally:
        be.close()


def test_site_4_0_is_the_plain_bank_and_site_refusals(lib, r18_blob):
    frames = dev(synth.synthetic_frames_u8(4, 32, 32, seed=3))
    be = Backend("resnet18_cifar", r18_blob[0], max_batch=8)
    try:
        plain = be.fit_patch_bank(frames, max_rows=40, seed=1)
        be.set_patch_bank(plain)
        want = numpy_of(be.classify_patch(frames))
        # a plain bank behaves as before with a stage tap on, at any stage
        be.set_stage_tap(2)
        also = numpy_of(be.classify_patch(frames))
        assert all(np.array_equal(want[k], also[k], equal_nan=True) for k in want) and be._stage_tap == 2 and not be._map_tap_on
        be.set_stage_tap(0)
        # the same rows at site {4, 0}: the records of the plain bank
        at4 = PatchBank(plain.rows, plain.threshold, plain.chunk_rows, plain.grid, stage=4, radius=0)
        be.set_patch_bank(at4)
        got = numpy_of(be.classify_patch(frames))
        assert all(np.array_equal(want[k], got[k], equal_nan=True) for k in want)
        fit4 = be.fit_patch_bank(frames, stage=4, radius=0, max_rows=40, seed=1)
        assert np.array_equal(fit4.rows, plain.rows) and fit4.stage == 4
        # fav_classify_patch with the stage tap off or at the wrong stage: refused, naming both stages
        dist = torch.full((4, 16), 3.0, dtype=torch.float32, device="cuda")
        rec = torch.full((4, 8), 77, dtype=torch.int32, device="cuda")
        lab, conf = (torch.empty(4, dtype=dt, device="cuda") for dt in (torch.int32, torch.float32))

        def calls():
            a = lib.fav_classify_patch(be._h, frames.data_ptr(), 4, _lib.LAYOUT_NHWC_U8, 0, lab.data_ptr(), conf.data_ptr(), None, None,
                                       dist.data_ptr(), None, rec.data_ptr(), stream())
            ma = lib.fav_last_error(be._h).decode()
            b = lib.fav_patch(be._h, dist.data_ptr(), None, rec.data_ptr(), stream())
            return a, ma, b, lib.fav_last_error(be._h).decode()
        for tap in (0, 3):
            be.set_stage_tap(tap)
            be.set_map_tap(True)                                                     # the map tap does not stand in for it
            a, ma, b, mb = calls()
            assert a == 1 and b == 1 and f"fav_classify_patch: the bank is at stage 4, the stage tap at stage {tap}" in ma
            assert f"fav_patch: the bank is at stage 4, the stage tap at stage {tap}" in mb
            be.set_map_tap(False)
        torch.cuda.synchronize()
        assert (dist == 3.0).all() and (rec == 77).all()
        be.set_stage_tap(4)
        a, _, b, _ = calls()
        assert a == 0 and b == 0
        be.set_stage_tap(0)
        # a bank of another stage's grid or width is refused, the handle left as it was
        before = numpy_of(be.classify_patch(frames))
        with pytest.raises(ValueError, match="cut from a"):
            be.set_patch_bank(PatchBank(at4.rows, grid=(4, 4), stage=3, radius=1))   # stage 3 is 8 x 8
        with pytest.raises(_lib.FavError, match="FAV_ERR_INVALID_ARG.*fav_set_patch_bank_at: D=512 is not the map width 256"):
            be.set_patch_bank(PatchBank(at4.rows, stage=3, radius=1))
        for kw, text in ((dict(stage=5), "stage=5"), (dict(stage=2, radius=3), "radius=3")):
            with pytest.raises(_lib.FavError, match="fav_set_patch_bank_at: " + text):
                be.set_patch_bank(PatchBank(unit_rows(np.random.default_rng(0), 3, 128), **kw))
        assert be.patch_bank is at4
        after = numpy_of(be.classify_patch(frames))
        assert all(np.array_equal(before[k], after[k], equal_nan=True) for k in before)
        # site NULL is fav_set_patch_bank
        cbank = plain.to_c()
        assert lib.fav_set_patch_bank_at(be._h, C.byref(cbank), None) == 0
        be._patch = plain
        back = numpy_of(be.classify_patch(frames))
        assert all(np.array_equal(want[k], back[k], equal_nan=True) for k in want)
    finally:
        be.close()
