"""Greedy coreset selection on the device: fav_op_coreset_select against tests/coreset_ref.py, and ``select="coreset"`` through
the Backend end to end.

Everything here is an equality of dwords.  The contract fixes the order of every sum, the distance is three rounded operations
and the pick a maximum of values with the lowest row on a tie: order[] and radius[] must be the reference's bits.

Shapes of the op.  D in {64, 128, 512, 576, 1024, 1088, 2048, 2112, 4096}: at 64 only 8 chains carry data, 512 is exactly one
step, 576 a step and a part step; a wave takes four rows at a time up to D = 1024, two up to 2048 and one above, so 1024 |
1088 and 2048 | 2112 stand either side of the two changes of kernel.  N in {1, 2, 63, 64, 65, 257, 1000, 5003}; M in {1, 2, 17,
N}; start_row first, last and in the middle; every value beside an awkward partner.  The grid has at most 1024 blocks of four
waves: 70 001 rows of D = 64 (four a wave), 8 203 of D = 2048 (two) and 5 003 of D = 4096 (one) each wrap the grid-stride loop
and end in a part-full group.  The rows are signed, so the similarities are negative as well as positive.

The outputs lie between guard bytes, and the workspace is filled with a pattern - or with zeros, which read as the distance
0.0 and as the best possible partial - so that a launch that read what it had not written would show."""
import numpy as np
import pytest

pytestmark = pytest.mark.gpu

torch = pytest.importorskip("torch")
import coreset_ref as R  # noqa: E402
from failure_aware_vision_amd import Backend, _lib, select_coreset, synth  # noqa: E402

GUARD = 64
FILL = 0x5A


@pytest.fixture(scope="module")
def lib():
    assert torch.cuda.is_available(), "GPU tests need a MI355X"
    return _lib.load()


def dev(a):
    return torch.from_numpy(np.ascontiguousarray(a)).cuda()


def unit_rows(rng, N, D):
    x = rng.standard_normal((N, D))
    return R.f32_to_bf16_bits((x / np.linalg.norm(x, axis=1, keepdims=True)).astype(np.float32))


def guards_ok(host, lo, nbytes):
    return bool((host[:lo] == FILL).all() and (host[lo + nbytes:] == FILL).all())


def run_op(lib, bits, M, start, ws=None, ws_fill=FILL, rows_off=0, ws_off=0, ws_short=0, order_off=0, radius_off=0, null=(), **over):
    """fav_op_coreset_select -> (status, order int32 [M0], radius float32 [M0 + 1], guard bytes untouched?, workspace
    untouched?), M0 the M the buffers were sized for.  order and radius each lie behind a guard in a buffer of FILL bytes,
    *_off bytes further in, with a guard behind them; the workspace is ``ws`` (a uint8 CUDA tensor, used as it is) or a fresh
    one of ``ws_fill`` bytes with GUARD bytes beyond the asked size, ws_short bytes shorter than the library asks.  M and start
    are passed as they are (the buffers are sized for M = 1 when M is out of range); over: N, D as passed, where they differ
    from the array's; null: arguments to pass as NULL."""
    N0, D0 = bits.shape
    M0 = M if 1 <= M <= N0 else 1
    rbuf = torch.zeros(bits.size + 16, dtype=torch.int16, device="cuda")
    rbuf[rows_off:rows_off + bits.size] = dev(bits.ravel().view(np.int16))
    need = lib.fav_coreset_workspace_bytes(N0, D0, M0)
    assert need > 0
    fresh = ws is None
    if fresh:
        ws = torch.full((256 + need + GUARD,), ws_fill, dtype=torch.uint8, device="cuda")
    assert ws.data_ptr() % 256 == 0 and rbuf.data_ptr() % 16 == 0 and ws.numel() >= ws_off + need
    before = ws.cpu().numpy()
    no, nr = 4 * M0, 4 * (M0 + 1)
    obuf = torch.full((GUARD + 16 + no + GUARD,), FILL, dtype=torch.uint8, device="cuda")
    qbuf = torch.full((GUARD + 16 + nr + GUARD,), FILL, dtype=torch.uint8, device="cuda")
    olo, qlo = GUARD + order_off, GUARD + radius_off
    ptr = dict(rows=rbuf[rows_off:].data_ptr(), ws=ws.data_ptr() + ws_off, order=obuf.data_ptr() + olo, radius=qbuf.data_ptr() + qlo)
    for name in null:
        ptr[name] = None
    st = lib.fav_op_coreset_select(ptr["rows"], over.get("N", N0), over.get("D", D0), M, start,
                                   ptr["ws"], need - ws_short, ptr["order"], ptr["radius"], torch.cuda.current_stream().cuda_stream)
    torch.cuda.synchronize()
    oh, qh, wh = obuf.cpu().numpy(), qbuf.cpu().numpy(), ws.cpu().numpy()
    guards = guards_ok(oh, olo, no) and guards_ok(qh, qlo, nr) and bool((wh[:ws_off] == before[:ws_off]).all() and
                                                                        (wh[ws_off + need:] == before[ws_off + need:]).all())
    order = oh[olo:olo + no].copy().view(np.int32)
    radius = qh[qlo:qlo + nr].copy().view(np.float32)
    return st, order, radius, guards, bool((wh == before).all())


def same(got, want):
    return np.array_equal(got[0], want[0]) and np.array_equal(got[1].view(np.uint32), want[1].view(np.uint32))


# (D, N, M, start_row): every value beside an awkward partner
SHAPES = [(64, 1, 1, 0), (4096, 2, 2, 1), (2048, 2, 1, 0), (576, 63, 63, 31), (64, 63, 2, 62), (512, 64, 64, 0), (128, 65, 65, 64),
          (4096, 65, 17, 32), (1088, 65, 2, 0), (2112, 65, 17, 64), (2048, 257, 17, 128), (128, 257, 257, 256), (1024, 257, 2, 0),
          (576, 1000, 17, 0), (2048, 1000, 2, 999), (128, 1000, 1, 500), (64, 5003, 17, 2501), (512, 5003, 2, 5002),
          (4096, 5003, 1, 0), (2048, 8203, 2, 4100)]


@pytest.mark.parametrize("shape", SHAPES, ids=["-".join(str(v) for v in s) for s in SHAPES])
def test_op_bit_exact(lib, shape):
    D, N, M, start = shape
    bits = unit_rows(np.random.default_rng(1000 * D + 10 * N + M), N, D)
    want = R.select(bits, M, start)
    if N > 2:
        assert (R.sims(bits, start) < 0).any() and (R.sims(bits, start) > 0).any()
    st, order, radius, guards, _ = run_op(lib, bits, M, start)
    assert st == 0 and guards
    assert same((order, radius), want), (np.flatnonzero(order != want[0])[:4], order[:4], want[0][:4], radius[:3], want[1][:3])


def test_op_a_pool_larger_than_one_pass_of_the_grid(lib):
    """70 001 rows of D = 64, four a wave: 17 501 groups over 4 096 waves, so the grid-stride loop wraps four times and the
    last group holds one row."""
    bits = unit_rows(np.random.default_rng(70001), 70001, 64)
    want = R.select(bits, 9, 35000)
    st, order, radius, guards, _ = run_op(lib, bits, 9, 35000)
    assert st == 0 and guards and same((order, radius), want)
    st, order, radius, guards, _ = run_op(lib, bits, 2, 70000)                       # the last row, alone in its group, is the centre
    assert st == 0 and guards and same((order, radius), R.select(bits, 2, 70000))


def test_op_a_pool_above_four_gigabytes(lib):
    """2^20 + 3 rows of D = 2048: 4.3 GB, so a row's element offset passes 2^31 and its byte offset 2^32.  The pool is gathered
    on the device from 512 distinct rows, and the reference computes a step's similarities on those and spreads them, which
    gives the same values: a similarity depends on the two rows' contents only.  The row opposite to the start row stands
    only near the end of the pool, so the second pick has to come from there."""
    N, D, U, M = (1 << 20) + 3, 2048, 512, 4
    rng = np.random.default_rng(4)
    uniq = unit_rows(rng, U, D)
    idx = rng.integers(0, U - 1, N)
    start = N - 1
    uniq[U - 1] = uniq[idx[start]] ^ 0x8000                                          # the start row, negated
    idx[N - 5] = U - 1
    want = R.select(np.empty((N, 0), np.uint16), M, start, sims_fn=lambda _, c: R.sims(uniq, int(idx[c]))[idx])
    assert want[0][1] == N - 5 and want[1][1] > 3.9
    pool = dev(uniq.view(np.int16))[dev(idx)]
    assert pool.data_ptr() % 16 == 0 and pool.numel() > 1 << 31
    need = lib.fav_coreset_workspace_bytes(N, D, M)
    ws = torch.full((need,), FILL, dtype=torch.uint8, device="cuda")
    order = torch.full((M,), -7, dtype=torch.int32, device="cuda")
    radius = torch.full((M + 1,), -7.0, dtype=torch.float32, device="cuda")
    assert lib.fav_op_coreset_select(pool.data_ptr(), N, D, M, start, ws.data_ptr(), need, order.data_ptr(), radius.data_ptr(),
                                     torch.cuda.current_stream().cuda_stream) == 0
    assert same((order.cpu().numpy(), radius.cpu().numpy()), want)


def test_op_ties_and_exhaustion(lib):
    rng = np.random.default_rng(7)
    # every row the same: each pick ties over all rows left, the lowest wins, and the last step finds none
    flat = np.repeat(unit_rows(rng, 1, 128), 70, axis=0)
    want = R.select(flat, 70, 33)
    assert want[0].tolist() == [33] + [r for r in range(70) if r != 33] and want[1][70] == 0.0
    st, order, radius, guards, _ = run_op(lib, flat, 70, 33)
    assert st == 0 and guards and same((order, radius), want)
    # duplicated blocks of rows, over several blocks of the grid: a duplicate of a centre is never farther than a new direction
    base = unit_rows(rng, 300, 576)
    pool = np.concatenate([base, base[:200], base[100:]])                            # 700 rows, each direction two or three times
    for M, start in ((300, 650), (17, 0), (700, 299)):
        want = R.select(pool, M, start)
        st, order, radius, guards, _ = run_op(lib, pool, M, start)
        assert st == 0 and guards and same((order, radius), want), (M, start)
        assert len(set(order.tolist())) == M
    assert want[1][700] == 0.0 and sorted(want[0].tolist()) == list(range(700))      # M = N: a permutation, radius 0
    # exactly unit rows (+-1/8 at D = 64): a duplicate lies at distance 0.0, equal to every other duplicate's
    signs = R.f32_to_bf16_bits((rng.choice([-1.0, 1.0], (40, 64)) / 8.0).astype(np.float32))
    pool = np.concatenate([signs, signs])
    want = R.select(pool, 80, 41)
    assert (want[1][41:] == 0.0).all()
    st, order, radius, guards, _ = run_op(lib, pool, 80, 41)
    assert st == 0 and guards and same((order, radius), want)


def test_op_workspace_hygiene(lib):
    rng = np.random.default_rng(9)
    a, b = unit_rows(rng, 1000, 128), unit_rows(rng, 777, 2048)
    fresh_a, fresh_b = run_op(lib, a, 17, 3), run_op(lib, b, 30, 776)
    assert same(fresh_a[1:3], R.select(a, 17, 3)) and same(fresh_b[1:3], R.select(b, 30, 776))
    assert fresh_a[3] and fresh_b[3]                                                 # GUARD bytes beyond the asked size: untouched
    # two different problems back to back in one workspace: each is what a fresh run gives
    need = max(lib.fav_coreset_workspace_bytes(1000, 128, 17), lib.fav_coreset_workspace_bytes(777, 2048, 30))
    ws = torch.full((need + GUARD,), FILL, dtype=torch.uint8, device="cuda")
    for bits, M, start, fresh in ((a, 17, 3, fresh_a), (b, 30, 776, fresh_b), (a, 17, 3, fresh_a), (a, 16, 4, None)):
        st, order, radius, guards, _ = run_op(lib, bits, M, start, ws=ws)
        assert st == 0 and guards
        assert same((order, radius), fresh[1:3] if fresh else R.select(bits, M, start))
    # a workspace of zeros - distance 0.0 everywhere, and no better partial - changes nothing either
    st, order, radius, guards, _ = run_op(lib, a, 17, 3, ws_fill=0)
    assert st == 0 and guards and same((order, radius), fresh_a[1:3])


REFUSALS = [("rows", dict(null=("rows",)), "null"), ("ws", dict(null=("ws",)), "null"), ("order", dict(null=("order",)), "null"),
            ("radius", dict(null=("radius",)), "null"),
            ("D 0", dict(D=0), "D=0"), ("D 32", dict(D=32), "D=32"), ("D 96", dict(D=96), "D=96"), ("D 4160", dict(D=4160), "D=4160"),
            ("N 0", dict(N=0), "N=0"), ("N -1", dict(N=-1), "N=-1"), ("N 2^24 + 1", dict(N=(1 << 24) + 1), "N=16777217"),
            ("M 0", dict(M=0), "M=0"), ("M N + 1", dict(M=18), "M=18"), ("M 262145", dict(N=1 << 20, M=262145), "M=262145"),
            ("start -1", dict(start=-1), "start_row=-1"), ("start N", dict(start=17), "start_row=17"),
            ("workspace a byte short", dict(ws_short=1), "ws_bytes"), ("workspace + 128", dict(ws_off=128), "256-byte"),
            ("rows + 8", dict(rows_off=4), "16-byte"), ("order + 4", dict(order_off=4), "16-byte"), ("radius + 8", dict(radius_off=8), "16-byte")]


@pytest.mark.parametrize("why,kw,text", REFUSALS, ids=[r[0] for r in REFUSALS])
def test_op_refusals_launch_nothing(lib, why, kw, text):
    bits = unit_rows(np.random.default_rng(17), 17, 64)
    kw = dict(kw)
    st, order, radius, guards, ws_untouched = run_op(lib, bits, kw.pop("M", 5), kw.pop("start", 2), **kw)
    msg = lib.fav_last_error(None).decode()
    assert st == 1 and "fav_op_coreset_select" in msg and text in msg, (why, msg)
    assert guards and ws_untouched                                                   # neither guards nor workspace touched
    assert (order.view(np.uint8) == FILL).all() and (radius.view(np.uint8) == FILL).all()   # ... nor any output


# ---- Python -------------------------------------------------------------------------------------------------------------
def test_select_coreset(lib):
    bits = unit_rows(np.random.default_rng(21), 500, 512)
    start = int(np.random.default_rng(6).integers(500))
    want = R.select(bits, 40, start)
    sel = select_coreset(bits, 40, seed=6)                                           # numpy in: uploaded
    assert sel.start_row == start and same((sel.order, sel.radius), want)
    assert sel.indices.tolist() == sorted(want[0].tolist()) and sel.cover_radius == float(want[1][40])
    for view in (torch.int16, torch.uint16):                                         # a CUDA tensor: used where it lives
        sel = select_coreset(dev(bits.view(np.int16)).view(view), 40, start_row=7)
        assert sel.start_row == 7 and same((sel.order, sel.radius), R.select(bits, 40, 7))
    bad = dev(bits.view(np.int16)).clone()
    bad[3, 5] = 0x7F80
    with pytest.raises(ValueError, match=r"non-finite value \(row 3\)"):
        select_coreset(bad, 4)
    bad[3] = 0
    with pytest.raises(ValueError, match="row 3 is zero"):
        select_coreset(bad, 4)


# ---- end to end ---------------------------------------------------------------------------------------------------------
def numpy_of(out):
    return {k: v.cpu().numpy() for k, v in out.items()}


def maps_are_tapped(be):
    return be.lib.fav_get_maps(be._h, None, None, None, None, None, None, None) == 0


def features_are_tapped(be):
    try:
        be.features()
    except _lib.FavError as e:
        assert "feature tap is off" in str(e)
        return False
    return True


def test_end_to_end_patch_bank(lib, r18_blob):
    frames = dev(synth.synthetic_frames_u8(5, 32, 32, seed=11))
    fit = dev(synth.synthetic_frames_u8(11, 32, 32, seed=12))                        # two batches of max_batch = 8: 176 cells
    be = Backend("resnet18_cifar", r18_blob[0], max_batch=8)
    try:
        full = be.fit_patch_bank(fit)
        assert full.selection is None and full.N == 11 * 16 - full.n_dropped
        m, seed = 40, 5
        bank = be.fit_patch_bank(fit, max_rows=m, select="coreset", seed=seed, threshold=0.5)
        assert not be._map_tap_on and not maps_are_tapped(be)                        # the tap is as it was: off
        start = int(np.random.default_rng(seed).integers(full.N))
        ref_order, ref_radius = R.select(full.rows, m, start)
        assert np.array_equal(bank.rows, full.rows[sorted(ref_order.tolist())])
        assert bank.selection.start_row == start and same((bank.selection.order, bank.selection.radius), (ref_order, ref_radius))
        assert (bank.N, bank.grid, bank.threshold, bank.n_dropped) == (m, full.grid, 0.5, full.n_dropped)
        # the draw is what it was: named, and not named
        plain = be.fit_patch_bank(fit, max_rows=m, seed=seed)
        named = be.fit_patch_bank(fit, max_rows=m, seed=seed, select="random")
        keep = np.sort(np.random.default_rng(seed).choice(full.N, size=m, replace=False))
        assert np.array_equal(plain.rows, full.rows[keep]) and np.array_equal(named.rows, plain.rows)
        assert plain.selection is None and named.selection is None and not np.array_equal(plain.rows, bank.rows)
        # the bank is a bank like another
        bank.check(512)
        be.set_patch_bank(bank)
        out = numpy_of(be.classify_patch(frames))
        assert out["dist"].shape == (5, 4, 4) and (out["nn_row"] < m).all() and (out["nn_row"] >= 0).all()
        # with the tap on before, it stays on
        be.set_map_tap(True)
        again = be.fit_patch_bank(fit, max_rows=m, select="coreset", seed=seed, threshold=0.5)
        assert be._map_tap_on and np.array_equal(again.rows, bank.rows)
        with pytest.raises(ValueError, match="select must be one of"):
            be.fit_patch_bank(fit, max_rows=m, select="kcentre")
    finally:
        be.close()


def test_end_to_end_knn_bank(lib, r18_blob):
    frames = dev(synth.synthetic_frames_u8(40, 32, 32, seed=13))
    labels = np.arange(40) % 7
    be = Backend("resnet18_cifar", r18_blob[0], max_batch=16)
    try:
        full = be.fit_knn(frames, labels, k=3)
        m, seed = 12, 2
        bank = be.fit_knn(frames, labels, k=3, max_rows=m, select="coreset", seed=seed)
        assert not features_are_tapped(be)                                           # the tap is as it was: off
        start = int(np.random.default_rng(seed).integers(40))
        ref_order, ref_radius = R.select(full.rows, m, start)
        idx = sorted(ref_order.tolist())
        assert np.array_equal(bank.rows, full.rows[idx]) and np.array_equal(bank.class_id, full.class_id[idx]) and bank.k == 3
        assert same((bank.selection.order, bank.selection.radius), (ref_order, ref_radius))
        plain = be.fit_knn(frames, labels, k=3, max_rows=m, seed=seed)
        named = be.fit_knn(frames, labels, k=3, max_rows=m, seed=seed, select="random")
        keep = np.sort(np.random.default_rng(seed).choice(40, size=m, replace=False))
        assert np.array_equal(plain.rows, full.rows[keep]) and np.array_equal(plain.class_id, full.class_id[keep])
        assert np.array_equal(named.rows, plain.rows) and np.array_equal(named.class_id, plain.class_id) and plain.selection is None
        with pytest.raises(ValueError, match=r"k must be in \[1, N=2\]"):
            be.fit_knn(frames, labels, k=3, max_rows=2, select="coreset")
        be.set_knn(bank)
        out = numpy_of(be.classify_knn(frames[:8]))
        assert out["kth_dist"].shape == (8,) and (out["nn_row"] < m).all() and set(out["nn_class"].tolist()) <= set(range(7))
    finally:
        be.close()
