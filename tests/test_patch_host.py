"""Patch-level anomaly maps without a device: the host-only entry points (fav_check_patch_bank, fav_patch_workspace_bytes,
fav_patch_chunk_rows), the Python side (patch.PatchBank, build_patch_bank, unpack_patch_records) and the numpy restatement
tests/patch_ref.py on maps made by hand."""
import ctypes as C
import math

import numpy as np
import pytest

import knn_ref as K
import patch_ref as R
from failure_aware_vision_amd import _lib, patch
from failure_aware_vision_amd.patch import PatchBank, build_patch_bank, unpack_patch_records

MIB = 1 << 20


@pytest.fixture(scope="module")
def lib():
    return _lib.load()


def unit_rows(rng, N, D):
    x = rng.standard_normal((N, D))
    return K.f32_to_bf16_bits((x / np.linalg.norm(x, axis=1, keepdims=True)).astype(np.float32))


def check(lib, bank, D_expected=-1):
    err = C.create_string_buffer(256)
    c = bank.to_c()
    return lib.fav_check_patch_bank(C.byref(c), D_expected, err, len(err)), err.value.decode()


# ---- fav_check_patch_bank: every range, the message naming the field -----------------------------------------------------------
def test_check_accepts_a_bank_in_range(lib):
    rows = unit_rows(np.random.default_rng(0), 5, 64)
    for kw in (dict(), dict(chunk_rows=64), dict(chunk_rows=262144), dict(threshold=0.0), dict(threshold=-math.inf)):
        assert check(lib, PatchBank(rows, **kw)) == (0, ""), kw
    assert check(lib, PatchBank(rows), 64) == (0, "")
    PatchBank(rows).check(64)


@pytest.mark.parametrize("make,text", [
    (lambda r: PatchBank(r[:, :32]), "D=32"), (lambda r: PatchBank(np.zeros((2, 96), np.uint16)), "D=96"),
    (lambda r: PatchBank(np.zeros((1, 4160), np.uint16)), "D=4160"), (lambda r: PatchBank(r[:0]), "N=0"),
    (lambda r: PatchBank(r, chunk_rows=32), "chunk_rows=32"), (lambda r: PatchBank(r, chunk_rows=96), "chunk_rows=96"),
    (lambda r: PatchBank(r, chunk_rows=-64), "chunk_rows=-64"), (lambda r: PatchBank(r, chunk_rows=262208), "chunk_rows=262208"),
    (lambda r: PatchBank(r, threshold=math.nan), "threshold"),
], ids=["D 32", "D 96", "D 4160", "N 0", "chunk 32", "chunk 96", "chunk -64", "chunk 262208", "threshold NaN"])
def test_check_names_the_field(lib, make, text):
    st, msg = check(lib, make(unit_rows(np.random.default_rng(0), 5, 64)))
    assert st == 1 and text in msg, msg


def test_check_the_rest(lib):
    rows = unit_rows(np.random.default_rng(0), 5, 64)
    st, msg = check(lib, PatchBank(rows), 128)
    assert st == 1 and "D=64" in msg and "128" in msg
    for bits in (0x7F80, 0xFF80, 0x7FC0):                                            # +inf, -inf, a NaN, in row 3
        bad = rows.copy()
        bad[3, 9] = bits
        st, msg = check(lib, PatchBank(bad))
        assert st == 1 and "non-finite" in msg and "row 3" in msg
        with pytest.raises(ValueError, match="non-finite"):
            PatchBank(bad).check()
    c = PatchBank(rows).to_c()
    c.struct_size -= 1
    err = C.create_string_buffer(256)
    assert lib.fav_check_patch_bank(C.byref(c), -1, err, len(err)) == 1 and b"struct_size" in err.value
    c = PatchBank(rows).to_c()
    c.rows = None
    assert lib.fav_check_patch_bank(C.byref(c), -1, err, len(err)) == 1 and b"rows is NULL" in err.value
    assert lib.fav_check_patch_bank(None, -1, err, len(err)) == 1 and b"bank is NULL" in err.value
    assert lib.fav_check_patch_bank(None, -1, None, 0) == 1                           # err may be NULL
    big = np.zeros((262145, 64), np.uint16)
    st, msg = check(lib, PatchBank(big))
    assert st == 1 and "N=262145" in msg


def test_struct_layouts():
    assert C.sizeof(_lib.FavPatchRecord) == 32 and C.sizeof(_lib.FavPatchBank) == 32
    assert _lib.FavPatchRecord.peak.offset == _lib.FavCamRecord.peak.offset == 8
    assert _lib.FavPatchRecord.floor.offset == _lib.FavCamRecord.floor.offset == 16
    assert [f[0] for f in _lib.FavPatchRecord._fields_] == list(patch._FIELDS)


# ---- the workspace and the chunk rule -------------------------------------------------------------------------------------------
def test_workspace_bytes_zero_out_of_range_and_monotone(lib):
    ws = lib.fav_patch_workspace_bytes
    assert ws(49, 512, 1000, 0) > 0
    for args in ((0, 512, 1000, 0), (-1, 512, 1000, 0), (49, 32, 1000, 0), (49, 96, 1000, 0), (49, 4160, 1000, 0), (49, 512, 0, 0),
                 (49, 512, 262145, 0), (49, 512, 1000, 32), (49, 512, 1000, 96), (49, 512, 1000, -64), (49, 512, 1000, 262208)):
        assert ws(*args) == 0, args
    sizes = [ws(49, 512, 1000, c) for c in range(64, 1280, 64)]
    assert all(a <= b for a, b in zip(sizes, sizes[1:])) and sizes[0] < sizes[-1]
    assert ws(49, 512, 1000, 1024) == ws(49, 512, 1000, 2048) == ws(49, 512, 1000, 262144)   # at most the padded bank
    # the parts: q, flags, bias, the part tile, the state, the slab, each on a 256-byte boundary
    al = lambda v: (v + 255) & ~255  # noqa: E731
    assert ws(49, 512, 1000, 128) == al(49 * 512 * 2) + al(49 * 4) + al(128 * 4) + 64 * 512 * 2 + al(49 * 8) + al(49 * 128 * 4)
    assert ws(49, 512, 1024, 128) == al(49 * 512 * 2) + al(49 * 4) + al(128 * 4) + al(49 * 8) + al(49 * 128 * 4)   # no part tile
    assert ws(3, 64, 1, 0) == ws(3, 64, 1, 64) == ws(3, 64, 63, 128)                                             # one tile of 64


def test_default_chunk_rule_at_its_edges(lib):
    chunk = lib.fav_patch_chunk_rows
    N = 262144
    # a slab exactly at 256 MiB: 131072 cells x 512 columns x 4 bytes
    assert 131072 * 512 * 4 == 256 * MIB
    assert chunk(131072, N, 0) == 512
    assert chunk(131073, N, 0) == 384 and 131073 * 384 * 4 <= 256 * MIB < 131073 * 512 * 4
    assert chunk(131071, N, 0) == 512                                                # 131071 x 640 x 4 is above
    # cells so many that 128 columns exceed it: the floor of 128
    assert 524288 * 128 * 4 == 256 * MIB and chunk(524288, N, 0) == 128
    assert chunk(524289, N, 0) == 128 and 524289 * 128 * 4 > 256 * MIB
    assert chunk(2 ** 31 - 1, N, 0) == 128
    # at most the padded bank, which may be below 128
    assert chunk(1, 1, 0) == 64 and chunk(1, 65, 0) == 128 and chunk(1, 1000, 0) == 1024 and chunk(1, N, 0) == N
    # the headline: 256 frames of 49 cells
    assert chunk(256 * 49, 16384, 0) == 5248 and 12544 * 5248 * 4 <= 256 * MIB < 12544 * (5248 + 128) * 4
    # the caller's own, cut to the padded bank
    assert chunk(12544, 16384, 64) == 64 and chunk(12544, 1000, 4096) == 1024 and chunk(524289, N, 256) == 256
    assert chunk(0, N, 0) == 0 and chunk(1, 0, 0) == 0 and chunk(1, N + 1, 0) == 0 and chunk(1, N, 96) == 0
    # the workspace follows the rule
    assert lib.fav_patch_workspace_bytes(131072, 64, N, 0) == lib.fav_patch_workspace_bytes(131072, 64, N, 512)
    assert lib.fav_patch_workspace_bytes(131073, 64, N, 0) == lib.fav_patch_workspace_bytes(131073, 64, N, 384)


# ---- PatchBank, build_patch_bank, unpack_patch_records ------------------------------------------------------------------------
def test_bank_round_trip_and_to_c(tmp_path):
    rows = unit_rows(np.random.default_rng(1), 7, 128)
    bank = PatchBank(rows, threshold=0.75, chunk_rows=128, grid=(4, 4), n_dropped=3)
    assert (bank.N, bank.D) == (7, 128)
    bank.save(tmp_path / "bank.npz")
    back = PatchBank.load(tmp_path / "bank.npz")
    assert np.array_equal(back.rows, rows) and (back.threshold, back.chunk_rows, back.grid, back.n_dropped) == (0.75, 128, (4, 4), 3)
    PatchBank(rows).save(tmp_path / "plain.npz")
    plain = PatchBank.load(tmp_path / "plain.npz")
    assert plain.grid is None and plain.threshold == math.inf and plain.chunk_rows == 0
    c = bank.to_c()
    assert (c.struct_size, c.D, c.N, c.chunk_rows, c.threshold) == (32, 128, 7, 128, 0.75)
    assert np.array_equal(np.ctypeslib.as_array(c.rows, shape=(7, 128)), rows)
    other = bank.with_threshold(1.5)
    assert other.threshold == 1.5 and bank.threshold == 0.75 and other.rows is bank.rows and other.grid == (4, 4)
    with pytest.raises(ValueError, match="uint16"):
        PatchBank(rows.astype(np.float32))
    with pytest.raises(ValueError, match="matrix"):
        PatchBank(rows.ravel())


def test_build_patch_bank():
    rng = np.random.default_rng(2)
    S, n, Hf, Wf, Cc = 3, 4, 2, 3, 64
    x = K.bf16_to_f32(K.f32_to_bf16_bits(rng.standard_normal((S, n, Hf, Wf, Cc)).astype(np.float32)))
    x[:, 1, 0, 1] = 0                                                                # a zero cell
    x[1, 2, 1, 2, 5] = np.nan                                                        # a NaN in one sample
    x[0, 3, 0, 0, 7] = np.inf                                                        # an infinity in one sample
    bits = K.f32_to_bf16_bits(x)
    bank = build_patch_bank(bits)
    assert (bank.N, bank.D, bank.grid, bank.n_dropped) == (n * Hf * Wf - 3, Cc, (2, 3), 3)
    assert bank.threshold == math.inf and bank.chunk_rows == 0
    bank.check(Cc)
    # unit norms to bf16's rounding, and the rows are the float64 recipe
    rows = K.bf16_to_f32(bank.rows).astype(np.float64)
    assert np.abs(np.linalg.norm(rows, axis=1) - 1.0).max() < 2.0 ** -8
    f = x.astype(np.float64).mean(axis=0).reshape(-1, Cc)
    keep = [r for r in range(n * Hf * Wf) if r not in (1 * 6 + 1, 2 * 6 + 5, 3 * 6 + 0)]
    want = K.f32_to_bf16_bits((f[keep] / np.sqrt((f[keep] * f[keep]).sum(axis=1))[:, None]).astype(np.float32))
    assert np.array_equal(bank.rows, want)
    # the flat layout, floats, and a torch bf16 tensor give the same bank (but no grid without the two map axes)
    flat = build_patch_bank(bits.reshape(S, n, Hf * Wf, Cc))
    assert np.array_equal(flat.rows, bank.rows) and flat.grid is None
    assert np.array_equal(build_patch_bank(x).rows, bank.rows)
    torch = pytest.importorskip("torch")
    t = torch.from_numpy(bits.view(np.int16)).view(torch.bfloat16)
    assert np.array_equal(build_patch_bank(t).rows, bank.rows)
    # the seeded subsample: that of build_knn_bank - drawn without replacement, kept in order
    sub = build_patch_bank(bits, max_rows=8, seed=5, threshold=0.5, chunk_rows=64)
    idx = np.sort(np.random.default_rng(5).choice(len(keep), size=8, replace=False))
    assert np.array_equal(sub.rows, want[idx]) and sub.n_dropped == 3 and (sub.threshold, sub.chunk_rows) == (0.5, 64)
    assert np.array_equal(build_patch_bank(bits, max_rows=8, seed=5).rows, sub.rows)
    assert not np.array_equal(build_patch_bank(bits, max_rows=8, seed=6).rows, sub.rows)
    assert build_patch_bank(bits, max_rows=1000).N == len(keep)
    with pytest.raises(ValueError, match="no cell has a direction"):
        build_patch_bank(np.zeros((1, 2, 4, 64), np.uint16))
    with pytest.raises(ValueError, match="maps must be"):
        build_patch_bank(np.zeros((2, 4, 64), np.uint16))


def test_unpack_patch_records():
    rec = np.zeros((3, 8), np.int32)
    f = rec.view(np.float32)
    rec[0] = (0, 0, 0, 5, 0, 17, 2, 1 | 0 << 8 | 2 << 16 | 1 << 24)
    f[0, 1], f[0, 2], f[0, 4] = 0.25, 1.5, 0.125
    rec[1] = (0, 0, 0, 0, 0, 3, 0, -1)                                               # nothing above, nothing degenerate
    rec[2] = (4, 0x7FC00000, 0, -1, 0, -1, 0, -1)                                    # all degenerate
    f[2, 2], f[2, 4] = -np.inf, np.inf
    out = unpack_patch_records(rec)
    assert out["mean_dist"].dtype == out["peak"].dtype == out["floor"].dtype == np.float32
    assert out["peak_row"].dtype == out["n_degenerate"].dtype == np.int32
    assert (out["mean_dist"][0], out["peak"][0], out["floor"][0]) == (0.25, 1.5, 0.125)
    assert out["peak_cell"].tolist() == [5, 0, -1] and out["peak_row"].tolist() == [17, 3, -1]
    assert [out[k][0] for k in ("x0", "y0", "x1", "y1")] == [1, 0, 2, 1] and [out[k][1] for k in ("x0", "y0", "x1", "y1")] == [-1] * 4
    assert out["anomalous"].tolist() == [True, False, True]
    assert np.isnan(out["mean_dist"][2]) and out["peak"][2] == -np.inf and out["floor"][2] == np.inf
    torch = pytest.importorskip("torch")
    t = unpack_patch_records(torch.from_numpy(rec))
    for key, v in out.items():
        assert np.array_equal(t[key].numpy(), v, equal_nan=True), key
    with pytest.raises(ValueError, match="int32"):
        unpack_patch_records(np.zeros((3, 6), np.int32))


# ---- the reference on maps made by hand ---------------------------------------------------------------------------------------
def axis_bits(D, j, value=1.0):
    v = np.zeros(D, np.float32)
    v[j] = value
    return K.f32_to_bf16_bits(v)


def test_reference_on_hand_made_maps():
    """One frame of 2 x 2 cells along the axes of a 64-wide space, a bank of axes: every similarity is 0 or +-1 exactly."""
    D = 64
    bank = np.stack([axis_bits(D, 0), axis_bits(D, 1), axis_bits(D, 0), axis_bits(D, 2, -1.0)])   # rows 0 and 2 tie
    maps = np.stack([axis_bits(D, 0, 3.0), axis_bits(D, 1, 0.5), axis_bits(D, 2, 2.0), axis_bits(D, 5, 7.0)])[None, None]
    dist, row, nn_sim, bad = R.cells(maps, bank)
    assert not bad.any()
    assert nn_sim.tolist() == [[1.0, 1.0, 0.0, 0.0]] and dist.tolist() == [[0.0, 0.0, 2.0, 2.0]]
    assert row.tolist() == [[0, 1, 0, 0]]                                            # the tie of rows 0 and 2: the lower; all 0: row 0
    # cell 2 is the opposite of row 3 (sim -1) and orthogonal to the rest: its nearest is at 0, not at -1
    rec = R.records(dist, row, 2, 2.0)                                               # a threshold at equality counts the cell
    out = unpack_patch_records(rec)
    assert (out["n_degenerate"][0], out["mean_dist"][0], out["peak"][0], out["peak_cell"][0], out["floor"][0]) == (0, 1.0, 2.0, 2, 0.0)
    assert (out["peak_row"][0], out["n_above"][0]) == (0, 2) and [out[k][0] for k in ("x0", "y0", "x1", "y1")] == [0, 1, 1, 1]
    above = unpack_patch_records(R.records(dist, row, 2, float(np.nextafter(np.float32(2.0), np.float32(3.0)))))
    assert above["n_above"][0] == 0 and above["box"][0] == -1 and not above["anomalous"][0]
    assert unpack_patch_records(R.records(dist, row, 2, math.inf))["n_above"][0] == 0
    assert unpack_patch_records(R.records(dist, row, 2, 0.0))["n_above"][0] == 4


def test_reference_degenerate_cells():
    D = 64
    bank = np.stack([axis_bits(D, 0), axis_bits(D, 1)])
    maps = np.stack([axis_bits(D, 0), np.zeros(D, np.uint16), axis_bits(D, 1), axis_bits(D, 3)])[None, None].copy()
    maps = np.concatenate([maps, np.zeros_like(maps)], axis=1)                       # frame 1: every cell zero
    maps[0, 0, 2, 9] = 0x7FC1                                                        # a NaN cell in frame 0
    dist, row, rec = R.score(maps, bank, 2, 2.0)
    assert np.isnan(dist[0, [1, 2]]).all() and row[0].tolist() == [0, -1, -1, 0] and dist[0, [0, 3]].tolist() == [0.0, 2.0]
    out = unpack_patch_records(rec)
    assert out["n_degenerate"].tolist() == [2, 4] and np.isnan(out["mean_dist"]).all()
    assert (out["peak"][0], out["peak_cell"][0], out["peak_row"][0], out["floor"][0], out["n_above"][0]) == (2.0, 3, 0, 0.0, 1)
    assert [out[k][0] for k in ("x0", "y0", "x1", "y1")] == [1, 1, 1, 1]
    assert (out["peak"][1], out["floor"][1], out["peak_cell"][1], out["peak_row"][1], out["n_above"][1], out["box"][1]) == \
        (-np.inf, np.inf, -1, -1, 0, -1)
    assert out["anomalous"].tolist() == [True, True]
    assert (R.canon_records(rec)[:, 1] == 0x7FC00000).all()
