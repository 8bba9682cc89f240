"""Greedy coreset selection without a device: the properties of the numpy restatement (tests/coreset_ref.py), the motivating
case, the host-only ABI (fav_check_coreset, fav_coreset_workspace_bytes) and the Python plumbing (``take``, ``select=``)."""
import ctypes as C
import math
import os
import re

import numpy as np
import pytest

import coreset_ref as R
from failure_aware_vision_amd import CoresetSelection, KNNBank, PatchBank, coreset, ood, patch, select_coreset

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


@pytest.fixture(scope="module")
def lib():
    from failure_aware_vision_amd import _lib
    return _lib.load()


def unit_rows(rng, N, D):
    x = rng.standard_normal((N, D))
    return R.f32_to_bf16_bits((x / np.linalg.norm(x, axis=1, keepdims=True)).astype(np.float32))


def sign_rows(rng, N, D):
    """Rows of +-1 / sqrt(D), D a power of four: exactly unit in bf16, every similarity exact, a duplicate at distance 0.0."""
    return R.f32_to_bf16_bits((rng.choice([-1.0, 1.0], (N, D)) / math.sqrt(D)).astype(np.float32))


def cover_radius_f64(bits, chosen) -> float:
    """max over the rows that were not chosen of the squared distance to the nearest chosen row, as 2 - 2 a.b in float64
    clamped at 0: what d states in exact arithmetic.  A chosen row lies on a centre, itself, whatever 2 - 2 |a|^2 makes of a
    row that rounding to bf16 took off the unit sphere; with every row chosen the radius is 0."""
    a = R.bits_to_f32(bits).astype(np.float64)
    rest = np.setdiff1d(np.arange(a.shape[0]), np.asarray(chosen))
    if rest.size == 0:
        return 0.0
    return float(np.maximum(2.0 - 2.0 * (a[rest] @ a[np.asarray(chosen)].T), 0.0).min(axis=1).max())


def d_rounding_bound(D: int) -> float:
    """How far one fp32 d = 2 - 2 sim can lie from its exact value.  sim is a sum of D exact products along a path of
    k = 8 * ceil(D / 512) + 6 additions (a chain, then the six halving steps), each rounding by at most u = 2^-24 relative:
    |sim - exact| <= k u / (1 - k u) * sum |a_j b_j| <= 1.01 k u * |a| |b|, and a row rounded to bf16 from a unit vector has
    |a| <= 1 + 2^-8, so |a| |b| < 1.008.  2 * sim is exact; the difference, at most 4 in size, rounds by at most 4 u; the
    clamp at 0 moves nothing away.  The maximum over rows of the minimum over centres moves by no more than one d does."""
    k = 8 * -(-D // 512) + 6
    u = 2.0 ** -24
    return 2.0 * 1.01 * k * u * 1.008 + 4.0 * u


# ---- the reference's properties ------------------------------------------------------------------------------------------
@pytest.mark.parametrize("N,D,M,start", [(257, 64, 40, 0), (300, 576, 33, 299), (129, 2048, 17, 64), (65, 128, 65, 7)])
def test_reference_properties(N, D, M, start):
    bits = unit_rows(np.random.default_rng(N + D), N, D)
    order, radius = R.select(bits, M, start)
    assert order.dtype == np.int32 and radius.dtype == np.float32 and order.shape == (M,) and radius.shape == (M + 1,)
    assert order[0] == start and radius[0] == np.inf
    assert (np.diff(radius[1:]) <= 0).all()                                          # never increases
    assert len(set(order.tolist())) == M and order.min() >= 0 and order.max() < N    # no repeats
    exact = cover_radius_f64(bits, order)
    assert abs(float(radius[M]) - exact) <= d_rounding_bound(D), (radius[M], exact)
    # a shorter selection is a prefix of a longer one
    o2, r2 = R.select(bits, max(1, M // 2), start)
    assert np.array_equal(o2, order[:o2.size]) and np.array_equal(r2[:-1], radius[:o2.size])
    if M == N:
        assert radius[N] == 0.0 and sorted(order.tolist()) == list(range(N))


def test_reference_sims_is_the_stated_order():
    """One row pair by a scalar loop: the chains, then the halving steps."""
    rng = np.random.default_rng(3)
    for D in (64, 576, 1024):
        bits = unit_rows(rng, 3, D)
        a, b = R.bits_to_f32(bits[2]), R.bits_to_f32(bits[1])
        s = [np.float32(0.0)] * 64
        for j in range(D):
            s[(j // 8) % 64] = np.float32(s[(j // 8) % 64] + np.float32(a[j] * b[j]))
        w = 32
        while w >= 1:
            for l in range(w):
                s[l] = np.float32(s[l] + s[l + w])
            w //= 2
        assert R.sims(bits, 1)[2].view(np.uint32) == s[0].view(np.uint32)


def test_reference_ties_and_taken_rows():
    base = sign_rows(np.random.default_rng(11), 6, 64)
    bits = np.concatenate([base, base, base[:3]])                                    # rows 6..11 and 12..14 repeat rows 0..5
    order, radius = R.select(bits, 15, 8)                                            # start on a duplicate of row 2
    assert sorted(order.tolist()) == list(range(15)) and radius[15] == 0.0
    first = order[:6].tolist()
    assert first[0] == 8 and sorted(r % 6 for r in first) == list(range(6))          # six distinct directions first
    assert all(r < 6 for r in first[1:])                                             # each by its lowest index
    assert (radius[6:15] == 0.0).all()                                               # what is left lies on a centre
    assert order[6:].tolist() == sorted(order[6:].tolist())                          # and goes by ascending index
    flat = np.repeat(base[:1], 9, axis=0)
    order, radius = R.select(flat, 9, 4)
    assert order.tolist() == [4, 0, 1, 2, 3, 5, 6, 7, 8] and (radius[1:] == 0.0).all()


# ---- the motivating case ----------------------------------------------------------------------------------------------------
def clustered_pool():
    rng = np.random.default_rng(0)
    N, D = 4096, 64
    centres = rng.standard_normal((13, D))
    label = np.zeros(N, np.int64)
    rare = rng.choice(N, 36, replace=False)
    label[rare] = 1 + np.arange(36) // 3                                             # 12 rare clusters of 3 rows
    x = centres[label] + 0.05 * rng.standard_normal((N, D))
    x /= np.linalg.norm(x, axis=1, keepdims=True)
    return R.f32_to_bf16_bits(x.astype(np.float32)), label


def test_greedy_covers_the_rare_modes_and_a_random_draw_does_not():
    bits, label = clustered_pool()
    order, radius = R.select(bits, 32, 7)
    assert len(set(label[order[:13]].tolist())) == 13                                # the first 13 picks: 13 distinct clusters
    assert radius[32] < 0.02
    a = R.bits_to_f32(bits).astype(np.float64)
    best, most = math.inf, 0
    for seed in range(200):
        keep = ood._subsample(bits, 32, seed)[1]
        cover = float(np.maximum(2.0 - 2.0 * (a @ a[keep].T), 0.0).min(axis=1).max())
        best, most = min(best, cover), max(most, len(set(label[keep].tolist())))
    print(f"greedy cover {float(radius[32]):.4f}; best random cover {best:.3f}, most clusters hit {most}")
    assert best >= 1.0


# ---- the host-only ABI -----------------------------------------------------------------------------------------------------
def check(lib, N, D, M, start):
    err = C.create_string_buffer(256)
    st = lib.fav_check_coreset(N, D, M, start, err, len(err))
    return st, err.value.decode()


def test_check_coreset_ranges(lib):
    for args in ((1, 64, 1, 0), (1 << 24, 4096, 262144, (1 << 24) - 1), (5, 576, 5, 4), (262144, 64, 262144, 0)):
        assert check(lib, *args) == (0, ""), args
    for args, word in (((5, 0, 1, 0), "D=0"), ((5, 96, 1, 0), "D=96"), ((5, 4160, 1, 0), "D=4160"), ((5, -64, 1, 0), "D=-64"),
                       ((0, 64, 1, 0), "N=0"), (((1 << 24) + 1, 64, 1, 0), "N=16777217"), ((-3, 64, 1, 0), "N=-3"),
                       ((5, 64, 0, 0), "M=0"), ((5, 64, 6, 0), "M=6"), ((1 << 20, 64, 262145, 0), "M=262145"),
                       ((5, 64, 1, -1), "start_row=-1"), ((5, 64, 1, 5), "start_row=5")):
        st, msg = check(lib, *args)
        assert st == 1 and word in msg, (args, msg)
    assert lib.fav_check_coreset(5, 96, 1, 0, None, 0) == 1                           # err may be NULL


def test_workspace_bytes(lib):
    assert lib.fav_coreset_workspace_bytes(0, 64, 1) == 0 and lib.fav_coreset_workspace_bytes(5, 96, 1) == 0
    assert lib.fav_coreset_workspace_bytes(5, 64, 6) == 0 and lib.fav_coreset_workspace_bytes((1 << 24) + 1, 64, 1) == 0
    sizes = [lib.fav_coreset_workspace_bytes(N, 64, 1) for N in (1, 2, 63, 64, 65, 1000, 70001, 1 << 24)]
    assert all(s > 0 and s % 256 == 0 for s in sizes) and sizes == sorted(sizes) and sizes[-1] > sizes[0]
    assert sizes[-1] >= 4 << 24                                                       # a key a row
    assert lib.fav_coreset_workspace_bytes(1000, 64, 1) == lib.fav_coreset_workspace_bytes(1000, 4096, 1000)


def test_symbols_are_declared_and_exported(lib):
    hdr = open(os.path.join(ROOT, "include", "fav.h")).read()
    names = set(re.findall(r"\b(fav_[a-z0-9_]+)\s*\(", hdr))
    for n in ("fav_check_coreset", "fav_coreset_workspace_bytes", "fav_op_coreset_select"):
        assert n in names and hasattr(lib, n), n


def test_op_refuses_without_a_device(lib):
    """A refusal is decided on the host: nothing is launched, so no device is needed to see it."""
    assert lib.fav_op_coreset_select(None, 5, 64, 1, 0, None, 0, None, None, None) == 1
    assert b"fav_op_coreset_select" in lib.fav_last_error(None)
    assert lib.fav_op_coreset_select(4096, 5, 96, 1, 0, 4096, 1 << 20, 4096, 4096, None) == 1
    assert b"D=96" in lib.fav_last_error(None)


# ---- the Python plumbing ---------------------------------------------------------------------------------------------------
def test_selection_dataclass():
    s = CoresetSelection([5, 2, 9], [np.inf, 1.5, 0.5, 0.25], 5)
    assert s.order.dtype == np.int32 and s.radius.dtype == np.float32 and s.start_row == 5
    assert s.indices.tolist() == [2, 5, 9] and s.cover_radius == 0.25
    with pytest.raises(ValueError, match="shapes do not fit"):
        CoresetSelection([1, 2], [np.inf, 1.0], 1)
    with pytest.raises(dataclass_frozen_error()):
        s.start_row = 1


def dataclass_frozen_error():
    import dataclasses
    return dataclasses.FrozenInstanceError


def test_take_on_both_banks():
    rng = np.random.default_rng(5)
    rows = unit_rows(rng, 10, 64)
    knn = KNNBank(rows, np.arange(10, dtype=np.int32) * 3, k=3, threshold=0.7)
    t = knn.take([7, 2, 9, 2])
    assert np.array_equal(t.rows, rows[[7, 2, 9, 2]]) and t.class_id.tolist() == [21, 6, 27, 6]
    assert (t.k, t.threshold, t.selection) == (3, 0.7, None)
    assert KNNBank(rows, k=3).take(np.array([1, 2, 3])).class_id is None
    with pytest.raises(ValueError, match=r"k must be in \[1, N=2\], got 3"):
        knn.take([0, 1])
    pb = PatchBank(rows, threshold=0.4, chunk_rows=128, grid=(2, 5), n_dropped=3)
    t = pb.take(np.array([9, 0]))
    assert np.array_equal(t.rows, rows[[9, 0]]) and (t.threshold, t.chunk_rows, t.grid, t.n_dropped, t.selection) == (0.4, 128, (2, 5), 3, None)
    for bank in (knn, pb):
        for bad in ([], [10], [-1], [[1, 2]], [0.5]):
            with pytest.raises(ValueError, match="indices"):
                bank.take(bad)


def test_select_argument():
    rng = np.random.default_rng(6)
    F = rng.standard_normal((40, 64))
    y = rng.integers(0, 5, 40)
    rows, ok = unit_rows(rng, 50, 64), np.ones(50, bool)
    ok[[3, 17]] = False
    with pytest.raises(ValueError, match="select must be one of"):
        ood.build_knn_bank(F, y, k=2, select="nonsense")
    with pytest.raises(ValueError, match="select must be one of"):
        patch.bank_from_rows(rows, ok, select="nonsense")
    with pytest.raises(ValueError, match="select must be one of"):
        patch.build_patch_bank(R.bits_to_f32(rows).reshape(1, 5, 10, 64), select="greedy")
    # "random" is what it was: the rows _subsample draws, for several seeds, named or not
    for seed in (0, 1, 2, 99):
        keep = np.sort(np.random.default_rng(seed).choice(40, size=12, replace=False))
        for bank in (ood.build_knn_bank(F, y, k=2, max_rows=12, seed=seed), ood.build_knn_bank(F, y, k=2, max_rows=12, seed=seed, select="random")):
            assert np.array_equal(bank.rows, ood._unit_rows_bf16(F[keep])) and np.array_equal(bank.class_id, y[keep]) and bank.selection is None
        keep = np.sort(np.random.default_rng(seed).choice(48, size=12, replace=False))
        for bank in (patch.bank_from_rows(rows, ok, 12, seed), patch.bank_from_rows(rows, ok, 12, seed, select="random")):
            assert np.array_equal(bank.rows, rows[ok][keep]) and bank.n_dropped == 2 and bank.selection is None
    # "coreset" with nothing to leave out keeps everything and touches no device
    for max_rows in (None, 40, 1000):
        bank = ood.build_knn_bank(F, y, k=2, max_rows=max_rows, select="coreset")
        assert np.array_equal(bank.rows, ood._unit_rows_bf16(F)) and np.array_equal(bank.class_id, y) and bank.selection is None
    for max_rows in (None, 48, 1000):
        bank = patch.bank_from_rows(rows, ok, max_rows, select="coreset")
        assert np.array_equal(bank.rows, rows[ok]) and bank.selection is None
    for select in ("random", "coreset"):
        with pytest.raises(ValueError, match="max_rows must be at least 1"):
            ood.build_knn_bank(F, y, k=2, max_rows=0, select=select)
        with pytest.raises(ValueError, match="max_rows must be at least 1"):
            patch.bank_from_rows(rows, ok, 0, select=select)


def test_a_selection_is_not_saved(tmp_path):
    rows = unit_rows(np.random.default_rng(1), 4, 64)
    sel = CoresetSelection([1, 0], [np.inf, 1.0, 0.5], 1)
    import dataclasses
    for bank, cls in ((dataclasses.replace(KNNBank(rows, k=1), selection=sel), KNNBank), (dataclasses.replace(PatchBank(rows), selection=sel), PatchBank)):
        assert bank.with_threshold(0.5).selection is sel
        bank.save(tmp_path / "bank.npz")
        back = cls.load(tmp_path / "bank.npz")
        assert back.selection is None and np.array_equal(back.rows, rows)


def test_select_coreset_refuses_before_any_device_call(monkeypatch):
    from failure_aware_vision_amd import _lib

    class NoDevice:
        """The host-only check passes through; anything else would be a device call."""
        def __init__(self, real):
            self.fav_check_coreset = real.fav_check_coreset

    monkeypatch.setattr(_lib, "load", lambda real=_lib.load(): NoDevice(real))
    rows = unit_rows(np.random.default_rng(2), 9, 64)
    for m in (0, 10, -1):
        with pytest.raises(ValueError, match=r"m must be in \[1, N=9\]"):
            select_coreset(rows, m)
    for value in (0x7F80, 0xFF80, 0x7FC1):
        bad = rows.copy()
        bad[4, 9] = value
        with pytest.raises(ValueError, match=r"non-finite value \(row 4\)"):
            select_coreset(bad, 3)
    bad = rows.copy()
    bad[6] = 0
    bad[6, 3] = 0x8000                                                               # -0 is zero too
    with pytest.raises(ValueError, match="row 6 is zero"):
        select_coreset(bad, 3)
    with pytest.raises(ValueError, match="uint16"):
        select_coreset(rows.astype(np.float32), 3)
    with pytest.raises(ValueError, match="start_row=9"):
        select_coreset(rows, 3, start_row=9)
    with pytest.raises(ValueError, match="D=72"):
        select_coreset(np.full((9, 72), 0x3F80, np.uint16), 3)
    assert coreset.SELECT_MODES == ("random", "coreset")
