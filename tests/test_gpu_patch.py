"""Patch-level anomaly maps on the device: fav_op_patch_score against tests/patch_ref.py, and the Backend methods end to end.

Everything here is an equality of bits (a NaN counts as equal to any NaN).  The query is the k-NN head's, the similarity the
production GEMM accumulator, which the oracle models bit for bit, and the maximum of (similarity, -row) is a value: a dist map,
a row map and a record must be the reference's dwords whatever the chunk.

Shapes of the op: C in {64, 512, 2048}, Hf x Wf in {1x1, 2x3, 4x4, 7x7}, n in {1, 2, 5, 37}, S in {1, 3}, N in {1, 15, 63, 64,
65, 257, 1000}, chunk_rows in {0, 64, 128}, every value beside an awkward partner, each case below 2e8 multiply-adds for the
oracle.  The GEMM reads the bank in tiles of 64 rows, in place up to the last multiple of 64 and through a zero-padded tile
behind it; the fold reads 256 columns a wave step, 4 a lane, four cells a block (1, 5, 6, 30, 49, 98, 222 and 1813 cells:
part blocks and many).  N = 257 at 64 is five chunks, the last one column wide.

The outputs lie between guard bytes, and the workspace is filled with a pattern that reads as 1.5e16: a fold that read a
padding column, a degenerate cell's row or a state nobody wrote would report it as the nearest neighbour."""
import ctypes as C
import math

import numpy as np
import pytest

pytestmark = pytest.mark.gpu

torch = pytest.importorskip("torch")
import cam_ref  # noqa: E402
import knn_ref as K  # noqa: E402
import patch_ref as R  # noqa: E402
from failure_aware_vision_amd import Backend, _lib, synth, views, weights  # noqa: E402
from failure_aware_vision_amd.ood import threshold_for_tpr  # noqa: E402
from failure_aware_vision_amd.patch import PatchBank, unpack_patch_records  # noqa: E402

GUARD = 64
FILL = 0x5A


@pytest.fixture(scope="module")
def lib():
    assert torch.cuda.is_available(), "GPU tests need a MI355X"
    return _lib.load()


def dev(a):
    return torch.from_numpy(np.ascontiguousarray(a)).cuda()


def guarded(nbytes, off=0):
    """A device buffer of FILL bytes -> (tensor, the offset of an output of nbytes behind a guard, `off` bytes further in)."""
    buf = torch.full((GUARD + 16 + nbytes + GUARD,), FILL, dtype=torch.uint8, device="cuda")
    assert buf.data_ptr() % 16 == 0
    return buf, GUARD + off


def guards_ok(host, lo, nbytes):
    return bool((host[:lo] == FILL).all() and (host[lo + nbytes:] == FILL).all())


def run_op(lib, maps_bits, bank_bits, grid, thr, chunk=0, rows=True, rec_off=0, dist_off=0, row_off=0, bank_off=0, ws_off=0,
           ws_short=0, null=(), **over):
    """fav_op_patch_score -> (status, dist float32 [n, HW], nn_row int32 [n, HW] or None, records int32 [n, 8], guard bytes
    untouched?, workspace untouched?).  Each output lies behind a guard in a buffer filled with FILL, *_off bytes further in,
    and so does the workspace, ws_short bytes shorter than fav_patch_workspace_bytes asks.  rows=False: row_dev is NULL.
    over: S, n, Hf, Wf, C, N as passed, where they differ from the arrays'; null: arguments to pass as NULL."""
    S0, n0, HW, C0 = maps_bits.shape
    Hf, Wf = grid
    assert Hf * Wf == HW
    N0 = bank_bits.shape[0]
    mbuf = dev(maps_bits.ravel().view(np.int16))
    bbuf = torch.zeros(bank_bits.size + 16, dtype=torch.int16, device="cuda")
    assert mbuf.data_ptr() % 16 == 0 and bbuf.data_ptr() % 16 == 0
    bbuf[bank_off:bank_off + bank_bits.size] = dev(bank_bits.ravel().view(np.int16))
    need = lib.fav_patch_workspace_bytes(n0 * HW, C0, N0, chunk if chunk % 64 == 0 and 0 <= chunk <= 262144 else 0)
    assert need > 0
    ws = torch.full((256 + need + GUARD,), FILL, dtype=torch.uint8, device="cuda")
    assert ws.data_ptr() % 256 == 0
    nd, nr = 4 * n0 * HW, 32 * n0
    dbuf, dlo = guarded(nd, dist_off)
    rbuf, rlo = guarded(nd, row_off)
    cbuf, clo = guarded(nr, rec_off)
    ptr = dict(maps=mbuf.data_ptr(), bank=bbuf[bank_off:].data_ptr(), ws=ws.data_ptr() + ws_off, dist=dbuf.data_ptr() + dlo,
               row=rbuf.data_ptr() + rlo if rows else None, rec=cbuf.data_ptr() + clo)
    for name in null:
        ptr[name] = None
    st = lib.fav_op_patch_score(ptr["maps"], over.get("S", S0), over.get("n", n0), over.get("Hf", Hf), over.get("Wf", Wf),
                                over.get("C", C0), ptr["bank"], over.get("N", N0), chunk, thr, ptr["ws"], need - ws_short,
                                ptr["dist"], ptr["row"], ptr["rec"], torch.cuda.current_stream().cuda_stream)
    torch.cuda.synchronize()
    dh, rh, ch, wh = dbuf.cpu().numpy(), rbuf.cpu().numpy(), cbuf.cpu().numpy(), ws.cpu().numpy()
    guards = (guards_ok(dh, dlo, nd) and guards_ok(ch, clo, nr) and (guards_ok(rh, rlo, nd) if rows else bool((rh == FILL).all())) and
              bool((wh[:ws_off] == FILL).all() and (wh[ws_off + need:] == FILL).all()))
    dist = dh[dlo:dlo + nd].copy().view(np.float32).reshape(n0, HW)
    row = rh[rlo:rlo + nd].copy().view(np.int32).reshape(n0, HW)
    rec = ch[clo:clo + nr].copy().view(np.int32).reshape(n0, 8)
    return st, dist, row if rows else None, rec, guards, bool((wh == FILL).all())


def unit_rows(rng, N, D):
    x = rng.standard_normal((N, D))
    return K.f32_to_bf16_bits((x / np.linalg.norm(x, axis=1, keepdims=True)).astype(np.float32))


def problem(Cc, grid, n, S, N, seed=0):
    """Signed maps and signed bank rows: the similarities are negative as well as positive."""
    rng = np.random.default_rng(1000 * Cc + 100 * grid[0] + 10 * N + S + n + seed)
    maps = K.f32_to_bf16_bits(rng.standard_normal((S, n, grid[0] * grid[1], Cc)).astype(np.float32))
    return maps, unit_rows(rng, N, Cc)


def same(got, want):
    """(dist, row or None, rec) of the device against (dist, row, rec) of the reference."""
    d, r, c = got
    return (np.array_equal(R.canon_map(d), R.canon_map(want[0])) and (r is None or np.array_equal(r, want[1])) and
            np.array_equal(R.canon_records(c), R.canon_records(want[2])))


# (C, Hf x Wf, n, S, N, chunk_rows): every value beside an awkward partner
SHAPES = [(64, (1, 1), 1, 1, 1, 0), (64, (2, 3), 5, 3, 15, 64), (512, (4, 4), 2, 1, 63, 128), (2048, (7, 7), 1, 1, 64, 0),
          (64, (7, 7), 37, 1, 65, 64), (512, (2, 3), 37, 3, 257, 64), (2048, (4, 4), 5, 1, 1000, 128), (64, (4, 4), 2, 3, 1000, 0),
          (512, (7, 7), 2, 1, 257, 128), (2048, (1, 1), 5, 3, 15, 0), (512, (1, 1), 1, 1, 65, 128), (64, (2, 3), 1, 1, 64, 64)]


@pytest.mark.parametrize("shape", SHAPES, ids=["-".join(str(v).replace(", ", "x").strip("()") for v in s) for s in SHAPES])
def test_op_bit_exact(lib, shape):
    Cc, grid, n, S, N, chunk = shape
    maps, bank = problem(Cc, grid, n, S, N)
    dist = R.cells(maps, bank)[0]
    thr = float(np.sort(dist.ravel())[dist.size // 2])                               # one cell at equality, both outcomes around it
    want = R.score(maps, bank, grid[1], thr)
    above = unpack_patch_records(want[2])["n_above"]
    assert dist.size < 3 or 0 < above.sum() < dist.size
    st, d, r, c, guards, _ = run_op(lib, maps, bank, grid, thr, chunk)
    assert st == 0 and guards
    assert same((d, r, c), want), np.flatnonzero((R.canon_records(c) != R.canon_records(want[2])).any(axis=1))[:8]
    st, d, r, c, guards, _ = run_op(lib, maps, bank, grid, thr, chunk, rows=False, rec_off=8)   # no row map; records 8-byte aligned only
    assert st == 0 and guards and r is None and same((d, r, c), want)


def test_op_the_chunk_changes_no_byte(lib):
    """N = 257 in chunks of 64 (five, the last one column wide), of 128 (three) and by the default rule (one)."""
    maps, bank = problem(64, (2, 3), 5, 1, 257, seed=1)
    want = R.score(maps, bank, 3, 1.0)
    outs = [run_op(lib, maps, bank, (2, 3), 1.0, chunk) for chunk in (64, 128, 0)]
    for st, d, r, c, guards, _ in outs:
        assert st == 0 and guards and same((d, r, c), want)
    for o in outs[1:]:
        assert all(np.array_equal(a.view(np.uint8), b.view(np.uint8)) for a, b in zip(o[1:4], outs[0][1:4]))
    assert lib.fav_patch_chunk_rows(30, 257, 64) == 64 and lib.fav_patch_chunk_rows(30, 257, 0) == 320


def test_op_ties_keep_the_lower_row(lib):
    rng = np.random.default_rng(7)
    bank = unit_rows(rng, 130, 64)
    bank[67] = bank[3]                                                               # either side of the boundary of chunks of 64
    bank[10] = bank[9]                                                               # inside one chunk
    bank[129] = bank[128] = bank[70]                                                 # three chunks, the last through the part tile
    maps = np.stack([bank[3], bank[9], bank[70], bank[40]])[None, None]              # one frame of 2 x 2 cells, each a bank row
    want = R.score(maps, bank, 2, math.inf)
    assert want[1].tolist() == [[3, 9, 70, 40]]
    sim = K.similarities(K.query(maps.reshape(1, 4, 64))[0], bank)
    assert sim[0, 3] == sim[0, 67] == sim[0].max() and sim[1, 9] == sim[1, 10] and sim[2, 70] == sim[2, 128] == sim[2, 129] == sim[2].max()
    for chunk in (64, 128, 0):
        st, d, r, c, guards, _ = run_op(lib, maps, bank, (2, 2), math.inf, chunk)
        assert st == 0 and guards and same((d, r, c), want), chunk
        assert r.tolist() == [[3, 9, 70, 40]]
    # a bank whose rows are all identical, over two whole tiles and a part tile: row 0 everywhere
    flat = np.repeat(bank[:1], 150, axis=0)
    want = R.score(maps, flat, 2, math.inf)
    assert (want[1] == 0).all()
    st, d, r, c, guards, _ = run_op(lib, maps, flat, (2, 2), math.inf, 64)
    assert st == 0 and guards and same((d, r, c), want)


@pytest.mark.parametrize("N", (15, 63, 65))
def test_op_a_padding_row_never_wins(lib, N):
    """Every similarity negative: the zero rows that pad the GEMM's tile score 0, above all of them."""
    rng = np.random.default_rng(N)
    maps = K.f32_to_bf16_bits(np.abs(rng.standard_normal((3, 5, 6, 64))).astype(np.float32))
    x = -np.abs(rng.standard_normal((N, 64)))
    bank = K.f32_to_bf16_bits((x / np.linalg.norm(x, axis=1, keepdims=True)).astype(np.float32))
    dist, row, nn_sim, bad = R.cells(maps, bank)
    assert not bad.any() and (nn_sim < 0).all() and (dist > 2).all()
    want = (dist, row, R.records(dist, row, 3, 2.5))
    for chunk in (0, 64):
        st, d, r, c, guards, _ = run_op(lib, maps, bank, (2, 3), 2.5, chunk)
        assert st == 0 and guards and same((d, r, c), want)
        assert (d > 2).all() and (r >= 0).all() and (r < N).all()


def test_op_degenerate_cells_stay_in_their_cell(lib):
    maps, bank = problem(128, (2, 3), 3, 3, 257, seed=2)
    clean = R.score(maps, bank, 3, 0.0)
    maps[:, 1, 2, :] = 0                                                             # a zero cell
    maps[0, 1, 4, 40] = 0x7FC1                                                       # a NaN cell
    maps[:, 2] = 0                                                                   # a frame whose cells are all degenerate
    maps[1, 2, 3, 5] = 0x7F80                                                        # ... one of them by an infinity
    dist, row, rec = want = R.score(maps, bank, 3, 0.0)                              # threshold 0: every scored cell is above
    assert R.cells(maps, bank)[3].tolist() == [[False] * 6, [False, False, True, False, True, False], [True] * 6]
    out = unpack_patch_records(rec)
    assert out["n_degenerate"].tolist() == [0, 2, 6] and out["n_above"].tolist() == [6, 4, 0]     # counted there, not here
    assert out["peak_cell"][1] not in (2, 4) and out["peak"][1] == np.nanmax(dist[1]) and out["floor"][1] == np.nanmin(dist[1])
    assert (out["peak"][2], out["floor"][2], out["peak_cell"][2], out["peak_row"][2], out["box"][2]) == (-np.inf, np.inf, -1, -1, -1)
    for chunk in (64, 0):
        st, d, r, c, guards, _ = run_op(lib, maps, bank, (2, 3), 0.0, chunk)
        assert st == 0 and guards and same((d, r, c), want)
        assert (d.view(np.int32)[1, [2, 4]] == 0x7FC00000).all() and (d.view(np.int32)[2] == 0x7FC00000).all()   # the contract's NaN
        assert r[1, [2, 4]].tolist() == [-1, -1] and (r[2] == -1).all()
        # every other cell and frame is what it is without them
        keep = [0, 1, 3, 5]
        assert np.array_equal(d[0], clean[0][0]) and np.array_equal(r[0], clean[1][0]) and np.array_equal(c[0], clean[2][0])
        assert np.array_equal(d[1, keep], clean[0][1, keep]) and np.array_equal(r[1, keep], clean[1][1, keep])
    # the overlay of the all-degenerate frame is all 0, and the others' are the reference's
    heat = torch.full((3, 9, 11), 7, dtype=torch.uint8, device="cuda")
    d_dev, c_dev = dev(d), dev(c)
    assert lib.fav_op_cam_heatmap(d_dev.data_ptr(), c_dev.data_ptr(), 3, 2, 3, 9, 11, heat.data_ptr(), None) == 0
    torch.cuda.synchronize()
    assert np.array_equal(heat.cpu().numpy(), cam_ref.heatmap(dist, rec, 2, 3, 9, 11)) and (heat[2] == 0).all() and (heat[0] != 0).any()


def test_op_thresholds(lib):
    maps, bank = problem(64, (4, 4), 2, 1, 63, seed=3)
    dist, row, _, _ = R.cells(maps, bank)
    t = np.sort(dist[1])[8]                                                          # the ninth smallest of frame 1's sixteen
    below = float(np.nextafter(t, np.float32(0))), float(np.nextafter(t, np.float32(4)))
    for thr in (float(t), *below, math.inf, -math.inf, 0.0):
        want = (dist, row, R.records(dist, row, 4, thr))
        n_above = unpack_patch_records(want[2])["n_above"]
        if thr == float(t):
            assert n_above[1] == 8 == (dist[1] >= t).sum() == (dist[1] > t).sum() + 1   # both outcomes in the call; equality counts
        st, d, r, c, guards, _ = run_op(lib, maps, bank, (4, 4), thr, 64)
        assert st == 0 and guards and same((d, r, c), want), thr
    at = unpack_patch_records(run_op(lib, maps, bank, (4, 4), float(t))[3])
    up = unpack_patch_records(run_op(lib, maps, bank, (4, 4), below[1])[3])
    assert at["n_above"][1] == up["n_above"][1] + 1                                  # one ulp above: the cell no longer counts
    inf = unpack_patch_records(run_op(lib, maps, bank, (4, 4), math.inf)[3])
    assert inf["n_above"].tolist() == [0, 0] and inf["box"].tolist() == [-1, -1] and not inf["anomalous"].any()
    assert unpack_patch_records(run_op(lib, maps, bank, (4, 4), -math.inf)[3])["n_above"].tolist() == [16, 16]


REFUSALS = [("maps", dict(null=("maps",)), "null"), ("bank", dict(null=("bank",)), "null"), ("ws", dict(null=("ws",)), "null"),
            ("dist", dict(null=("dist",)), "null"), ("rec", dict(null=("rec",)), "null"),
            ("S 0", dict(S=0), "S=0"), ("S 4097", dict(S=4097), "S=4097"), ("n 0", dict(n=0), "n must"), ("n -1", dict(n=-1), "n must"),
            ("Hf 0", dict(Hf=0), "Hf=0"), ("HW 1025", dict(Hf=25, Wf=41), "Hf=25 x Wf=41"), ("Wf 257", dict(Hf=1, Wf=257), "Wf=257"),
            ("cells 2^31", dict(n=2097152, Hf=32, Wf=32), "2^31"),
            ("C 32", dict(C=32), "D=32"), ("C 96", dict(C=96), "D=96"), ("C 4160", dict(C=4160), "D=4160"),
            ("N 0", dict(N=0), "N=0"), ("N 262145", dict(N=262145), "N=262145"),
            ("chunk 32", dict(chunk=32), "chunk_rows=32"), ("chunk 96", dict(chunk=96), "chunk_rows=96"),
            ("chunk -64", dict(chunk=-64), "chunk_rows=-64"), ("chunk 262208", dict(chunk=262208), "chunk_rows=262208"),
            ("threshold NaN", dict(thr=math.nan), "threshold"), ("workspace a byte short", dict(ws_short=1), "ws_bytes"),
            ("workspace + 128", dict(ws_off=128), "256-byte"), ("bank + 8", dict(bank_off=4), "16-byte"),
            ("dist + 2", dict(dist_off=2), "4-byte"), ("row + 2", dict(row_off=2), "4-byte"), ("rec + 4", dict(rec_off=4), "8-byte")]


@pytest.mark.parametrize("why,kw,text", REFUSALS, ids=[r[0] for r in REFUSALS])
def test_op_refusals_launch_nothing(lib, why, kw, text):
    maps, bank = problem(64, (2, 3), 5, 1, 17)
    kw = dict(kw)
    thr, chunk = kw.pop("thr", 1.0), kw.pop("chunk", 0)
    st, d, r, c, guards, ws_untouched = run_op(lib, maps, bank, (2, 3), thr, chunk, **kw)
    msg = lib.fav_last_error(None).decode()
    assert st == 1 and "fav_op_patch_score" in msg and text in msg, (why, msg)
    assert guards and ws_untouched                                                   # neither guards nor workspace touched
    assert all((a.view(np.uint8) == FILL).all() for a in (d, r, c))                  # ... nor any output


# ---- end to end ---------------------------------------------------------------------------------------------------------
def bits_of(t):
    """a bf16 CUDA tensor -> its bits on the host."""
    return t.view(torch.int16).cpu().numpy().view(np.uint16)


def numpy_of(out):
    return {k: v.cpu().numpy() for k, v in out.items()}


def records_of(out):
    """classify_patch's dict (numpy values) -> int32 [n, 8] records."""
    return np.stack([out["n_degenerate"], out["mean_dist"].view(np.int32), out["peak"].view(np.int32), out["peak_cell"],
                     out["floor"].view(np.int32), out["peak_row"], out["n_above"], out["box"]], axis=1)


def maps_are_tapped(be):
    """fav_get_maps answers with the sizes only while the map tap is on and a call has filled it."""
    return be.lib.fav_get_maps(be._h, None, None, None, None, None, None, None) == 0


MC = dict(n_samples=3, dropout_policy="all_blocks", dropout_p=0.1, seed=4)
E2E = {"r18_single": dict(arch="resnet18_cifar", hw=(32, 32), n=5, kw=dict(), S=1, map=(4, 4, 512)),
       "r18_mc": dict(arch="resnet18_cifar", hw=(32, 32), n=5, kw=MC, S=3, map=(4, 4, 512)),
       "r50_single": dict(arch="resnet50", hw=(64, 64), n=2, kw=dict(), S=1, map=(2, 2, 2048)),
       "r50_mc": dict(arch="resnet50", hw=(64, 64), n=2, kw=MC, S=3, map=(2, 2, 2048)),
       # odd frame sizes: the 2 x 2 map of a 33 x 47 frame, the 4 x 6 map of a 31 x 45 one, their heat maps upsampled to the frame
       "r50_33x47": dict(arch="resnet50", hw=(33, 47), n=2, kw=MC, S=3, map=(2, 2, 2048)),
       "r18_31x45": dict(arch="resnet18_cifar", hw=(31, 45), n=5, kw=dict(), S=1, map=(4, 6, 512))}


@pytest.mark.parametrize("case", list(E2E))
def test_end_to_end(lib, case, r18_blob, r50_blob):
    c = E2E[case]
    blob = (r18_blob if c["arch"] == "resnet18_cifar" else r50_blob)[0]
    n, hw = c["n"], c["hw"]
    frames = dev(synth.synthetic_frames_u8(n, hw[0], hw[1], seed=11))
    fit = dev(synth.synthetic_frames_u8(11, hw[0], hw[1], seed=12))                  # two batches of max_batch = 8
    be = Backend(c["arch"], blob, max_batch=8, in_hw=hw, **c["kw"])
    try:
        # the map's geometry: fav_map_tap_info's (tests/test_odd_frames_host.py holds it to the oracle's shapes at every size)
        info = be.map_tap_info()
        Hf, Wf, Cc = info["hf"], info["wf"], info["c"]
        assert (Hf, Wf, Cc) == c["map"] and info["samples"] == c["S"] and info["bytes"] == c["S"] * 8 * Hf * Wf * Cc * 2
        plain = [t.cpu().numpy() for t in be.classify_detect(frames)]
        bank = be.fit_patch_bank(fit, max_rows=100, seed=3)
        assert (bank.N, bank.D, bank.grid) == (min(100, 11 * Hf * Wf - bank.n_dropped), Cc, (Hf, Wf))
        assert not be._map_tap_on and not maps_are_tapped(be)                        # fit_patch_bank left the tap as it was: off
        bank.check(Cc)
        be.set_patch_bank(bank)
        assert be.patch_bank is bank and not maps_are_tapped(be)                     # the setter does not touch the tap
        first = numpy_of(be.classify_patch(frames, heatmap=True))                    # the tap goes on for the call, and off again
        assert not be._map_tap_on and not maps_are_tapped(be)
        be.set_map_tap(True)
        got = numpy_of(be.classify_patch(frames, heatmap=True))
        assert be._map_tap_on and maps_are_tapped(be)
        for key in got:
            assert np.array_equal(first[key], got[key], equal_nan=True), key
        for key, want in zip(("label", "conf", "fail", "score"), plain):            # fav_classify_ex, unchanged
            assert np.array_equal(got[key].view(np.uint8), want.view(np.uint8)), key
        # the maps and the records: the reference on the tapped maps of the same call
        maps = be.maps()
        lab, conf = be.classify(frames)
        assert np.array_equal(lab.cpu().numpy(), got["label"]) and np.array_equal(conf.cpu().numpy(), got["conf"])
        assert tuple(maps.shape) == (c["S"], n, Hf, Wf, Cc)
        xb = bits_of(maps).reshape(c["S"], n, Hf * Wf, Cc)
        dist, row, rec = R.score(xb, bank.rows, Wf, bank.threshold)
        assert got["dist"].shape == (n, Hf, Wf) and got["nn_row"].shape == (n, Hf, Wf)
        assert same((got["dist"].reshape(n, -1), got["nn_row"].reshape(n, -1), records_of(got)), (dist, row, rec))
        assert np.array_equal(got["heatmap"], cam_ref.heatmap(dist, rec, Hf, Wf, hw[0], hw[1]))
        assert (np.nan_to_num(dist) > 0).any()
        # fav_patch on the maps of the last call: the same bytes, no second pass; and the op on those maps
        d2 = torch.empty((n, Hf * Wf), dtype=torch.float32, device="cuda")
        r2 = torch.empty((n, Hf * Wf), dtype=torch.int32, device="cuda")
        c2 = torch.empty((n, 8), dtype=torch.int32, device="cuda")
        assert lib.fav_patch(be._h, d2.data_ptr(), r2.data_ptr(), c2.data_ptr(), torch.cuda.current_stream().cuda_stream) == 0
        assert same((d2.cpu().numpy(), r2.cpu().numpy(), c2.cpu().numpy()), (dist, row, rec))
        st, d3, r3, c3, guards, _ = run_op(lib, xb, bank.rows, (Hf, Wf), bank.threshold, 64)
        assert st == 0 and guards and same((d3, r3, c3), (dist, row, rec))
        # numpy frames in -> numpy out, the same bits
        host = be.classify_patch(frames.cpu().numpy())
        assert isinstance(host["dist"], np.ndarray) and np.array_equal(records_of(host), records_of(got)) and "heatmap" not in host
        # a threshold inside the range of the cells: both outcomes, through the handle
        thr = float(np.sort(dist.ravel())[dist.size // 2])
        be.set_patch_bank(bank.with_threshold(thr))
        flagged = numpy_of(be.classify_patch(frames))
        assert same((flagged["dist"].reshape(n, -1), flagged["nn_row"].reshape(n, -1), records_of(flagged)), R.score(xb, bank.rows, Wf, thr))
        assert 0 < flagged["n_above"].sum() < dist.size and flagged["anomalous"].any()
        if case == "r18_single":
            rep = be.faithfulness_report(frames, steps=4, maps=got["dist"])          # the dist map is a saliency map like another
            assert rep["map_hw"] == (Hf, Wf) and rep["n"] == n
        be.set_patch_bank(None)
        assert be.patch_bank is None and maps_are_tapped(be)                         # clearing the bank leaves the caller's tap
    finally:
        be.close()


def test_calibrate_and_report(lib, r18_blob):
    """tpr = 0.9 of 40 frames: the quantile rule takes the ceil(0.9 * 40) = 36th smallest peak, q; the threshold is one float32
    step above it, since a cell counts at equality; so the frames flagged are those with peak > q: at most 4, and exactly 4
    when no other peak ties with q."""
    frames = dev(synth.synthetic_frames_u8(40, 32, 32, seed=31))
    be = Backend("resnet18_cifar", r18_blob[0], max_batch=16)
    try:
        with pytest.raises(ValueError, match="set_patch_bank first"):
            be.calibrate_patch(frames)
        be.set_patch_bank(be.fit_patch_bank(dev(synth.synthetic_frames_u8(24, 32, 32, seed=32)), max_rows=200))
        peaks = np.concatenate([be.classify_patch(frames[b:b + 16], first_index=b)["peak"].cpu().numpy() for b in (0, 16, 32)])
        q = np.float32(threshold_for_tpr(peaks, 0.9))
        assert q == np.sort(peaks)[35]
        thr = be.calibrate_patch(frames, tpr=0.9)
        assert thr == float(np.nextafter(q, np.float32(np.inf))) == be.patch_bank.threshold and not be._map_tap_on
        out = [numpy_of(be.classify_patch(frames[b:b + 16], first_index=b)) for b in (0, 16, 32)]
        flagged = np.concatenate([o["n_above"] > 0 for o in out])
        assert np.array_equal(flagged | np.concatenate([o["n_degenerate"] > 0 for o in out]), np.concatenate([o["anomalous"] for o in out]))
        assert np.array_equal(flagged, peaks > q) and flagged.sum() == 40 - (peaks <= q).sum() <= 4
        assert flagged.sum() == 4 or (peaks == q).sum() > 1
        rep = be.patch_report(frames[:16], 255 - frames[16:32])
        assert 0.0 <= rep["auroc"] <= 1.0 and rep["n_id"] == rep["n_ood"] == 16 and rep["threshold"] == thr
    finally:
        be.close()


def test_handle_refusals(lib, r18_blob):
    frames = dev(synth.synthetic_frames_u8(4, 32, 32, seed=3))
    be = Backend("resnet18_cifar", r18_blob[0], max_batch=8)
    try:
        dist = torch.full((4, 16), 3.0, dtype=torch.float32, device="cuda")
        row = torch.full((4, 16), 77, dtype=torch.int32, device="cuda")
        rec = torch.full((4, 8), 77, dtype=torch.int32, device="cuda")
        s = torch.cuda.current_stream().cuda_stream
        lab, conf = (torch.empty(4, dtype=dt, device="cuda") for dt in (torch.int32, torch.float32))

        def fav_patch(d=None, r=None, c=None):
            st = lib.fav_patch(be._h, d or dist.data_ptr(), r or row.data_ptr(), c or rec.data_ptr(), s)
            return st, lib.fav_last_error(be._h).decode()

        def fav_classify_patch():
            st = lib.fav_classify_patch(be._h, frames.data_ptr(), 4, _lib.LAYOUT_NHWC_U8, 0, lab.data_ptr(), conf.data_ptr(), None, None,
                                        dist.data_ptr(), row.data_ptr(), rec.data_ptr(), s)
            return st, lib.fav_last_error(be._h).decode()
        # no bank
        with pytest.raises(_lib.FavError, match="no patch bank"):
            be.classify_patch(frames)
        be.set_map_tap(True)
        be.classify(frames)
        for call, fn in ((fav_patch, "fav_patch"), (fav_classify_patch, "fav_classify_patch")):
            st, msg = call()
            assert st == 1 and f"{fn}: no patch bank set" in msg
        be.set_map_tap(False)
        # a bank of the wrong width
        with pytest.raises(_lib.FavError, match="FAV_ERR_INVALID_ARG.*fav_set_patch_bank: D=64"):
            be.set_patch_bank(PatchBank(unit_rows(np.random.default_rng(0), 3, 64)))
        with pytest.raises(ValueError, match="cut from a"):
            be.set_patch_bank(PatchBank(unit_rows(np.random.default_rng(0), 3, 512), grid=(7, 7)))
        assert be.patch_bank is None
        bank = PatchBank(unit_rows(np.random.default_rng(0), 70, 512), grid=(4, 4))
        be.set_patch_bank(bank)
        # the tap off, at the C level
        for call, fn in ((fav_patch, "fav_patch"), (fav_classify_patch, "fav_classify_patch")):
            st, msg = call()
            assert st == 1 and f"{fn}: the map tap is off" in msg
        be.set_map_tap(True)
        st, msg = fav_patch()
        assert st == 1 and "fav_patch: no classify call since the tap was turned on" in msg
        be.classify(frames)
        # NULL and misaligned buffers (row_dev may be NULL)
        for kw in (dict(d=dist.data_ptr() + 2), dict(r=row.data_ptr() + 2), dict(c=rec.data_ptr() + 4)):
            st, msg = fav_patch(**kw)
            assert st == 1 and "fav_patch" in msg
        assert lib.fav_patch(be._h, None, row.data_ptr(), rec.data_ptr(), s) == 1 and lib.fav_patch(be._h, dist.data_ptr(), None, None, s) == 1
        torch.cuda.synchronize()
        assert (dist == 3.0).all() and (row == 77).all() and (rec == 77).all()       # nothing was launched so far
        assert lib.fav_patch(be._h, dist.data_ptr(), None, rec.data_ptr(), s) == 0
        torch.cuda.synchronize()
        assert (row == 77).all() and not (rec == 77).all()
        # views: the maps are there, the head is not
        be.set_views(views.hflip())
        for call, fn in ((fav_patch, "fav_patch"), (fav_classify_patch, "fav_classify_patch")):
            st, msg = call()
            assert st == 6 and f"{fn}: views are set" in msg
        with pytest.raises(_lib.FavError, match="FAV_ERR_UNSUPPORTED.*fav_classify_patch: views are set"):
            be.classify_patch(frames)
        be.classify(frames)
        be.set_views(None)
        st, msg = fav_patch()
        assert st == 6 and "fav_patch: the last call ran under views" in msg
        assert fav_classify_patch()[0] == 0 and fav_patch()[0] == 0
        # a rejected bank leaves the handle as it was
        before = numpy_of(be.classify_patch(frames))
        with pytest.raises(_lib.FavError, match="chunk_rows=96"):
            be.set_patch_bank(PatchBank(bank.rows, chunk_rows=96))
        assert be.patch_bank is bank
        after = numpy_of(be.classify_patch(frames))
        assert all(np.array_equal(before[k], after[k], equal_nan=True) for k in before)
    finally:
        be.close()


def test_vit_and_ensemble_refuse_the_bank_and_go_on_working(lib, r18_blob):
    vblob, _ = weights.make_synthetic_vit("vit_tiny", seed=3)
    vframes = dev(synth.synthetic_frames_u8(3, 64, 64, seed=19))
    vit = Backend("vit_tiny", vblob, max_batch=4)
    ens = Backend("resnet18_cifar", [r18_blob[0], weights.make_synthetic("resnet18_cifar", seed=2)[0]], max_batch=4)
    try:
        for be, fr, D, word in ((vit, vframes, 128, "ViT"), (ens, dev(synth.synthetic_frames_u8(3, 32, 32, seed=13)), 512, "ensemble")):
            before = [t.cpu().numpy() for t in be.classify_detect(fr)]
            bank = PatchBank(unit_rows(np.random.default_rng(0), 7, D))
            c = bank.to_c()
            assert lib.fav_set_patch_bank(be._h, C.byref(c)) == 6 and word in lib.fav_last_error(be._h).decode()
            with pytest.raises(_lib.FavError, match="FAV_ERR_UNSUPPORTED.*fav_set_patch_bank"):
                be.set_patch_bank(bank)
            assert be.patch_bank is None
            assert lib.fav_set_patch_bank(be._h, None) == 0                           # clearing is never refused
            after = [t.cpu().numpy() for t in be.classify_detect(fr)]
            assert all(np.array_equal(a.view(np.uint8), b.view(np.uint8)) for a, b in zip(before, after))
    finally:
        vit.close()
        ens.close()


def test_a_workspace_above_the_limit_is_refused_with_the_numbers(lib, r18_blob):
    """max_batch = 64 frames of 4 x 4 cells against 262144 rows in ONE chunk: a slab of 1 GiB alone.  Refused on the host before
    anything is allocated; the handle stays as it was.  By the default rule the same bank fits: the slab stays at 256 MiB."""
    be = Backend("resnet18_cifar", r18_blob[0], max_batch=64)
    try:
        rows = np.zeros((262144, 512), np.uint16)
        rows[:, 0] = 0x3F80                                                          # 1.0: unit rows
        with pytest.raises(_lib.FavError, match=r"max_batch=64 frames of 4 x 4 cells.*N=262144.*chunks of 262144.*above the limit of 1073741824"):
            be.set_patch_bank(PatchBank(rows, chunk_rows=262144))
        assert be.patch_bank is None
        need = lib.fav_patch_workspace_bytes(64 * 16, 512, 262144, 262144)
        assert need > 1 << 30 and lib.fav_patch_workspace_bytes(64 * 16, 512, 262144, 0) < 1 << 30
        frames = dev(synth.synthetic_frames_u8(2, 32, 32, seed=1))
        with pytest.raises(_lib.FavError, match="no patch bank"):
            be.classify_patch(frames)
        be.set_patch_bank(PatchBank(rows))                                           # chunks of 65536 rows: four GEMMs, four folds
        out = numpy_of(be.classify_patch(frames))
        assert ((out["nn_row"] == 0) | (out["nn_row"] == -1)).all() and (out["nn_row"] == 0).any()   # every row is the same: the lowest
    finally:
        be.close()


def test_a_knn_bank_and_a_patch_bank_together(lib, r18_blob):
    frames = dev(synth.synthetic_frames_u8(6, 32, 32, seed=23))
    be = Backend("resnet18_cifar", r18_blob[0], max_batch=8)
    try:
        knn = be.fit_knn(frames, k=2)
        pb = be.fit_patch_bank(frames[:3], max_rows=40)
        be.set_knn(knn)
        knn_alone = numpy_of(be.classify_knn(frames))
        be.set_knn(None)
        be.set_patch_bank(pb)
        patch_alone = numpy_of(be.classify_patch(frames))
        be.set_knn(knn)
        both_knn = numpy_of(be.classify_knn(frames))
        both_patch = numpy_of(be.classify_patch(frames))
        assert all(np.array_equal(knn_alone[k], both_knn[k], equal_nan=True) for k in knn_alone)
        assert all(np.array_equal(patch_alone[k], both_patch[k], equal_nan=True) for k in patch_alone)
        assert be.features().shape == (1, 6, 512)                                    # the k-NN bank's feature tap is its own affair
        be.set_patch_bank(None)
        assert all(np.array_equal(knn_alone[k], v, equal_nan=True) for k, v in numpy_of(be.classify_knn(frames)).items())
        be.set_knn(None)
        with pytest.raises(_lib.FavError, match="feature tap is off"):
            be.features()
    finally:
        be.close()
