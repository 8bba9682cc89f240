"""CPU-side checks of the nearest-neighbour OOD scoring: the fav_knn_bank / fav_knn_record layouts (C vs ctypes) and the new
symbols, fav_check_knn_bank (host only) range by range, fav_knn_workspace_bytes, build_knn_bank, the record unpacking, the
.npz round trip, and the numpy reference (tests/knn_ref.py) that the GPU file compares bits with: on cases whose answers
are known, and as a detector on clustered data."""
import ctypes as C
import math
import os
import subprocess

import numpy as np
import pytest

import knn_ref as R

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


@pytest.fixture(scope="module")
def lib():
    from failure_aware_vision_amd import _lib
    if not os.path.exists(_lib.LIB_PATH):
        import __graft_entry__ as g
        g.build()
    return _lib.load()


_LAYOUT_C = r"""
#include <stddef.h>
#include <stdio.h>
#include "fav.h"
int main(void) {
    printf("bank_size %zu\n", sizeof(fav_knn_bank));
    printf("record_size %zu\n", sizeof(fav_knn_record));
    printf("config_size %zu\n", sizeof(fav_config));
#define F(x) printf("b.%s %zu\n", #x, offsetof(fav_knn_bank, x));
    F(struct_size) F(D) F(N) F(k) F(rows) F(class_id) F(threshold)
#define G(x) printf("r.%s %zu\n", #x, offsetof(fav_knn_record, x));
    G(kth_dist) G(kth_sim) G(nn_sim) G(nn_row) G(nn_class) G(ood)
    printf("abi %d\nkcount %d\n", (int)FAV_ABI_VERSION, (int)FAV_K_COUNT);
    return 0;
}
"""

SYMBOLS = ("fav_check_knn_bank", "fav_set_knn", "fav_classify_knn", "fav_knn_workspace_bytes", "fav_op_knn_score")


def test_layouts_symbols_and_abi(lib, tmp_path):
    from failure_aware_vision_amd import _lib
    src = tmp_path / "layout.c"
    src.write_text(_LAYOUT_C)
    exe = str(tmp_path / "layout")
    subprocess.check_call(["gcc", "-std=c99", "-Wall", "-Werror", "-I" + os.path.join(ROOT, "include"), str(src), "-o", exe])
    out = dict(line.split() for line in subprocess.check_output([exe], text=True).splitlines())
    assert int(out["bank_size"]) == C.sizeof(_lib.FavKnnBank) == 40
    assert int(out["record_size"]) == C.sizeof(_lib.FavKnnRecord) == 24
    for name in ("struct_size", "D", "N", "k", "rows", "class_id", "threshold"):
        assert int(out["b." + name]) == getattr(_lib.FavKnnBank, name).offset, name
    for name in ("kth_dist", "kth_sim", "nn_sim", "nn_row", "nn_class", "ood"):
        assert int(out["r." + name]) == getattr(_lib.FavKnnRecord, name).offset, name
    # what this feature must not move: the ABI version, fav_config, the kernel classes
    assert int(out["abi"]) == 2 == lib.fav_abi_version()
    assert int(out["config_size"]) == C.sizeof(_lib.FavConfig) == 120
    assert int(out["kcount"]) == 6 == _lib.K_COUNT
    header = open(os.path.join(ROOT, "include", "fav.h")).read()
    for sym in SYMBOLS:
        assert sym in _lib._SIGNATURES and hasattr(lib, sym) and sym + "(" in header, sym
        assert getattr(lib, sym).argtypes == _lib._SIGNATURES[sym][1]


def test_entry_points_refuse_a_null_handle(lib):
    assert lib.fav_set_knn(None, None) == 1
    assert lib.fav_classify_knn(None, None, 1, 0, 0, None, None, None, None, None, None) == 1


# ---- fav_check_knn_bank -----------------------------------------------------------------------------------------------
def bank(D=64, N=5, k=2, class_id=True, **kw):
    from failure_aware_vision_amd.ood import KNNBank
    rng = np.random.default_rng(D + N)
    rows = R.f32_to_bf16_bits((rng.standard_normal((N, D)) / np.sqrt(D)).astype(np.float32))
    return KNNBank(rows, (np.arange(N) % 3) if class_id else None, k=k, **kw)


def refusal(lib, b, D_expected=-1, patch=None):
    c = b.to_c()
    if patch:
        patch(c)
    err = C.create_string_buffer(256)
    st = lib.fav_check_knn_bank(C.byref(c), D_expected, err, len(err))
    return st, err.value.decode()


def test_check_accepts_the_corners(lib):
    for b in (bank(), bank(D=4096, N=1, k=1), bank(N=300, k=256), bank(class_id=False), bank(threshold=-math.inf),
              bank(threshold=0.5)):
        assert refusal(lib, b) == (0, "")
        b.check()
    assert refusal(lib, bank(D=128), D_expected=128) == (0, "")
    assert lib.fav_check_knn_bank(C.byref(bank().to_c()), -1, None, 0) == 0          # no message buffer


def test_check_refuses_each_range_and_names_the_field(lib):
    cases = [(bank(), lambda c: setattr(c, "struct_size", 36), "struct_size=36"),
             (bank(), lambda c: setattr(c, "D", 32), "D=32"), (bank(), lambda c: setattr(c, "D", 96), "D=96"),
             (bank(), lambda c: setattr(c, "D", 4160), "D=4160"), (bank(), lambda c: setattr(c, "D", 0), "D=0"),
             (bank(), lambda c: setattr(c, "N", 0), "N=0"), (bank(), lambda c: setattr(c, "N", 262145), "N=262145"),
             (bank(), lambda c: setattr(c, "k", 0), "k=0"), (bank(), lambda c: setattr(c, "k", 6), "k=6"),
             (bank(N=300), lambda c: setattr(c, "k", 257), "k=257"),
             (bank(), lambda c: setattr(c, "rows", None), "rows is NULL"),
             (bank(threshold=math.nan), None, "threshold")]
    for b, patch, text in cases:
        st, msg = refusal(lib, b, patch=patch)
        assert st == 1 and text in msg, (text, msg)
    st, msg = refusal(lib, bank(D=128), D_expected=64)
    assert st == 1 and "D=128" in msg and "64" in msg
    assert lib.fav_check_knn_bank(None, -1, None, 0) == 1
    for bits in (0x7F80, 0xFF80, 0x7FC0, 0x7F81):                                    # +inf, -inf, two NaNs
        b = bank()
        b.rows[3, 7] = bits
        st, msg = refusal(lib, b)
        assert st == 1 and "rows" in msg and "row 3" in msg, (hex(bits), msg)
        with pytest.raises(ValueError, match="rows"):
            b.check()
    b = bank()
    b.class_id[4] = -2
    st, msg = refusal(lib, b)
    assert st == 1 and "class_id[4]=-2" in msg
    b.class_id[4] = -1
    assert refusal(lib, b) == (0, "")


def test_workspace_bytes(lib):
    """Host only.  q bf16 [n][D], a flag a frame, a zero bias and the fp32 similarities [n][Npad] must fit, and a 64-row tile
    when the bank does not end on a multiple of 64 rows; 0 for sizes out of range."""
    f = lib.fav_knn_workspace_bytes
    for n, D, N in ((1, 64, 1), (17, 2048, 4099), (67, 768, 64), (256, 2048, 262144)):
        npad = (N + 63) // 64 * 64
        need = n * D * 2 + n * 4 + npad * 4 + n * npad * 4 + (64 * D * 2 if N % 64 else 0)
        assert need <= f(n, D, N) <= need + 4 * 256, (n, D, N)
    assert f(0, 64, 1) == f(1, 32, 1) == f(1, 64, 0) == f(1, 64, 262145) == f(-1, 64, 1) == 0
    assert f(2, 64, 64) > f(1, 64, 64) and f(1, 64, 65) > f(1, 64, 64)


# ---- build_knn_bank ----------------------------------------------------------------------------------------------------
def test_build_unit_norm_to_within_bf16():
    from failure_aware_vision_amd.ood import build_knn_bank
    rng = np.random.default_rng(0)
    F = rng.standard_normal((50, 128)) * rng.uniform(1e-3, 1e3, (50, 1))
    y = rng.integers(0, 7, 50)
    b = build_knn_bank(F, y, k=4)
    assert b.rows.dtype == np.uint16 and b.rows.shape == (50, 128) and b.k == 4 and b.threshold == math.inf
    assert np.array_equal(b.class_id, y) and b.class_id.dtype == np.int32
    rows = R.bf16_to_f32(b.rows).astype(np.float64)
    unit = F / np.linalg.norm(F, axis=1, keepdims=True)
    # RNE to 8 significant bits: half an ulp is 2^-8 of the power of two below the value, so at most 2^-8 of the value (the
    # rounding to fp32 in front of it moves a value by 2^-24 of itself); the norm of the row moves by no more than its error's
    assert (np.abs(rows - unit) <= np.abs(unit) * (2.0 ** -8 + 2.0 ** -23)).all()
    assert np.array_equal(b.rows, R.f32_to_bf16_bits(unit.astype(np.float32)))
    assert np.abs(np.linalg.norm(rows, axis=1) - 1.0).max() <= 2.0 ** -8 + 2.0 ** -23
    assert build_knn_bank(F).class_id is None
    b.check()


def test_build_subsample_is_deterministic_and_without_replacement():
    from failure_aware_vision_amd.ood import build_knn_bank
    rng = np.random.default_rng(1)
    F = rng.standard_normal((40, 64))
    y = np.arange(40)                                                                 # a label names its row
    a, b, c = (build_knn_bank(F, y, k=3, max_rows=12, seed=s) for s in (5, 5, 6))
    assert a.N == 12 and np.array_equal(a.rows, b.rows) and np.array_equal(a.class_id, b.class_id)
    assert not np.array_equal(a.class_id, c.class_id)
    assert len(set(a.class_id.tolist())) == 12 and (np.diff(a.class_id) > 0).all()   # no row twice, original order
    assert np.array_equal(a.rows, build_knn_bank(F, y, k=3).rows[a.class_id])
    assert build_knn_bank(F, y, k=3, max_rows=40).N == build_knn_bank(F, y, k=3, max_rows=99).N == 40


def test_build_refusals():
    from failure_aware_vision_amd.ood import KNNBank, build_knn_bank
    F = np.random.default_rng(2).standard_normal((6, 64))
    for bad, text in ((np.nan, "non-finite"), (np.inf, "non-finite")):
        G = F.copy()
        G[2, 3] = bad
        with pytest.raises(ValueError, match=text):
            build_knn_bank(G)
    G = F.copy()
    G[4] = 0
    with pytest.raises(ValueError, match="row 4 is zero"):
        build_knn_bank(G)
    for kw, text in ((dict(k=0), "k must"), (dict(k=7), "k must"), (dict(max_rows=0), "max_rows"), (dict(k=4, max_rows=3), "k must")):
        with pytest.raises(ValueError, match=text):
            build_knn_bank(F, **kw)
    with pytest.raises(ValueError, match="one label"):
        build_knn_bank(F, np.arange(5))
    with pytest.raises(ValueError, match="negative"):
        build_knn_bank(F, -np.arange(6))
    with pytest.raises(ValueError, match="integers"):
        build_knn_bank(F, np.arange(6) * 0.5)
    with pytest.raises(ValueError, match="N, D"):
        build_knn_bank(F[0])
    with pytest.raises(ValueError, match="uint16"):
        KNNBank(F.astype(np.float32))
    with pytest.raises(ValueError, match="shapes"):
        KNNBank(np.zeros((3, 64), np.uint16), np.zeros(4))


def test_bank_round_trip_and_threshold(tmp_path):
    from failure_aware_vision_amd.ood import KNNBank
    for b in (bank(threshold=0.25), bank(class_id=False, k=5)):
        path = str(tmp_path / "bank.npz")
        b.save(path)
        z = KNNBank.load(path)
        assert np.array_equal(z.rows, b.rows) and z.k == b.k and z.threshold == b.threshold
        assert (z.class_id is None) == (b.class_id is None) and (b.class_id is None or np.array_equal(z.class_id, b.class_id))
    t = bank().with_threshold(1.5)
    assert t.threshold == 1.5 and t.k == 2 and np.array_equal(t.rows, bank().rows)


def test_unpack_records():
    from failure_aware_vision_amd.ood import unpack_knn_records
    rec = np.zeros((3, 6), np.int32)
    rec[:, 0] = np.array([0.5, 0.0, np.nan], np.float32).view(np.int32)
    rec[:, 1] = np.array([0.75, 1.0, np.nan], np.float32).view(np.int32)
    rec[:, 2] = np.array([0.875, 1.0, np.nan], np.float32).view(np.int32)
    rec[:, 3], rec[:, 4], rec[:, 5] = [4, 0, -1], [7, -1, -1], [0, 0, 1]
    out = unpack_knn_records(rec)
    assert out["kth_dist"].dtype == np.float32 and out["kth_dist"][:2].tolist() == [0.5, 0.0] and np.isnan(out["kth_dist"][2])
    assert out["kth_sim"][:2].tolist() == [0.75, 1.0] and out["nn_sim"][0] == 0.875
    assert out["nn_row"].tolist() == [4, 0, -1] and out["nn_class"].tolist() == [7, -1, -1] and out["ood"].tolist() == [0, 0, 1]
    torch = pytest.importorskip("torch")
    t = unpack_knn_records(torch.from_numpy(rec))
    assert t["kth_sim"].dtype == torch.float32 and t["nn_row"].tolist() == [4, 0, -1]
    with pytest.raises(ValueError, match="int32"):
        unpack_knn_records(np.zeros((3, 4), np.int32))


# ---- the reference itself ----------------------------------------------------------------------------------------------
def test_reference_on_known_answers():
    """One-hot features against one-hot rows: every product is exact, so every figure can be said in advance."""
    D = 64
    eye = np.eye(D, dtype=np.float32)
    bank_bits = R.f32_to_bf16_bits(np.stack([eye[3], eye[5], eye[3], -eye[3], eye[9]]))
    feat = np.zeros((2, 4, D), np.float32)
    feat[:, 0, 3] = [4.0, 2.0]          # frame 0: 3 e3 after the mean -> e3: rows 0 and 2 at sim 1, row 3 at -1
    feat[0, 1, 5] = -0.5                # frame 1: -e5
    feat[:, 3, 9] = [np.inf, 1.0]       # frame 3 degenerate; frame 2 too (zero)
    out = R.score(R.f32_to_bf16_bits(feat), bank_bits, 2, [10, 11, 12, 13, 14], 1.0)
    assert out["kth_sim"][:2].tolist() == [1.0, 0.0] and out["nn_sim"][:2].tolist() == [1.0, 0.0]
    assert out["nn_row"].tolist() == [0, 0, -1, -1] and out["nn_class"].tolist() == [10, 10, -1, -1]
    assert out["kth_dist"][:2].tolist() == [0.0, 2.0] and out["ood"].tolist() == [0, 1, 1, 1]
    assert np.isnan(out["kth_dist"][2:]).all() and np.isnan(out["kth_sim"][2:]).all() and np.isnan(out["nn_sim"][2:]).all()
    last = R.score(R.f32_to_bf16_bits(feat), bank_bits, 5, None, math.inf)
    assert last["kth_sim"][:2].tolist() == [-1.0, -1.0] and last["kth_dist"][:2].tolist() == [4.0, 4.0]
    assert last["nn_class"].tolist() == [-1] * 4 and last["ood"].tolist() == [0, 0, 1, 1]
    assert not np.signbit(last["nn_sim"][1])                                         # + 0.0f: never -0
    rec = R.records(out)
    assert rec.shape == (4, 6) and rec[2].tolist() == [0x7FC00000] * 3 + [-1, -1, 1]


@pytest.mark.parametrize("seed", range(5))
def test_reference_separates_clusters_from_noise(seed):
    """10 Gaussian clusters in D = 64 with noise 0.3: 500 bank rows, 200 in-distribution test rows, 200 isotropic random rows
    as OOD, k = 5.  AUROC of kth_dist >= 0.99."""
    from failure_aware_vision_amd.ood import OODModel, build_knn_bank
    rng = np.random.default_rng(seed)
    D = 64
    centres = rng.standard_normal((10, D))

    def draw(n):
        c = rng.integers(0, 10, n)
        return centres[c] + 0.3 * rng.standard_normal((n, D)), c

    F, y = draw(500)
    b = build_knn_bank(F, y, k=5)
    ident, _ = draw(200)
    ood = rng.standard_normal((200, D))
    d = [R.score(R.f32_to_bf16_bits(x.astype(np.float32))[None], b.rows, b.k, b.class_id, math.inf)["kth_dist"] for x in (ident, ood)]
    auroc = OODModel.auroc(d[0], d[1])
    print(f"seed {seed}: auroc {auroc:.4f}, id mean {d[0].mean():.3f}, ood mean {d[1].mean():.3f}")
    assert auroc >= 0.99
