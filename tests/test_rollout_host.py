"""CPU-side checks of the attention rollout: the fav_rollout_record layout (C vs ctypes, and against fav_cam_record, whose
peak and floor offsets fav_op_cam_heatmap reads) and the new symbols, fav_attn_tap_info through the loaded library (the
planner alone, no device), the numpy reference (tests/rollout_ref.py) that the GPU file compares bits with - on hand-made
attention and against float64 - and the host helpers of failure_aware_vision_amd.rollout."""
import ctypes as C
import os
import subprocess

import numpy as np
import pytest

import rollout_ref as R

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
F32 = np.float32


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
    printf("record_size %zu\n", sizeof(fav_rollout_record));
    printf("record_align %zu\n", _Alignof(fav_rollout_record));
    printf("config_size %zu\n", sizeof(fav_config));
#define G(x) printf("r.%s %zu\n", #x, offsetof(fav_rollout_record, x));
    G(n_layers) G(cls_mass) G(peak) G(peak_cell) G(floor) G(patch_sum) G(n_above) G(box)
    printf("cam.peak %zu\ncam.floor %zu\n", offsetof(fav_cam_record, peak), offsetof(fav_cam_record, floor));
    printf("abi %d\nkcount %d\n", (int)FAV_ABI_VERSION, (int)FAV_K_COUNT);
    return 0;
}
"""

SYMBOLS = ("fav_set_attn_tap", "fav_get_attention", "fav_attn_tap_info", "fav_op_attn_mean", "fav_op_attn_rollout", "fav_rollout",
           "fav_classify_rollout")
FIELDS = ("n_layers", "cls_mass", "peak", "peak_cell", "floor", "patch_sum", "n_above", "box")


def test_layout_symbols_and_abi(lib, tmp_path):
    from failure_aware_vision_amd import _lib
    src = tmp_path / "layout.c"
    src.write_text(_LAYOUT_C)
    exe = str(tmp_path / "layout")
    subprocess.check_call(["gcc", "-std=c11", "-Wall", "-Werror", "-I" + os.path.join(ROOT, "include"), str(src), "-o", exe])
    out = dict(line.split() for line in subprocess.check_output([exe], text=True).splitlines())
    assert int(out["record_size"]) == C.sizeof(_lib.FavRolloutRecord) == 32 == 4 * R.RECORD_DWORDS
    assert int(out["record_align"]) == 4
    for i, name in enumerate(FIELDS):
        assert int(out["r." + name]) == getattr(_lib.FavRolloutRecord, name).offset == 4 * i, name
    # fav_op_cam_heatmap reads peak and floor of either record
    assert int(out["r.peak"]) == int(out["cam.peak"]) == _lib.FavCamRecord.peak.offset == 8
    assert int(out["r.floor"]) == int(out["cam.floor"]) == _lib.FavCamRecord.floor.offset == 16
    # what this feature must not move: the ABI version, fav_config, the kernel classes
    assert int(out["abi"]) == 2 == lib.fav_abi_version()
    assert int(out["config_size"]) == C.sizeof(_lib.FavConfig) == 120
    assert int(out["kcount"]) == 6 == _lib.K_COUNT
    header = open(os.path.join(ROOT, "include", "fav.h")).read()
    for sym in SYMBOLS:
        assert sym in _lib._SIGNATURES and hasattr(lib, sym) and sym + "(" in header, sym
        assert getattr(lib, sym).argtypes == _lib._SIGNATURES[sym][1]
    import failure_aware_vision_amd as pkg
    for name in ("unpack_rollout_records", "patch_box_to_pixels", "rollout"):
        assert hasattr(pkg, name), name
    for name in ("set_attn_tap", "attn_tap_info", "attention", "rollout", "classify_rollout"):
        assert hasattr(pkg.Backend, name), name


def test_entry_points_refuse_a_null_handle(lib):
    assert lib.fav_set_attn_tap(None, 1, 0) == 1
    assert lib.fav_get_attention(None, None, None, None, None, None, None) == 1
    assert lib.fav_rollout(None, 0, None, None, None) == 1
    assert lib.fav_classify_rollout(None, None, 1, 0, 0, None, None, None, None, 0, None, None, None) == 1


# ---- fav_attn_tap_info: the planner alone, no device -----------------------------------------------------------------------
def tap_info(lib, arch, **kw):
    from failure_aware_vision_amd import _lib
    cfg = _lib.FavConfig()
    lib.fav_default_config(C.byref(cfg), arch)
    for k, v in kw.items():
        setattr(cfg, k, v)
    nbytes, layers, tokens, ld = C.c_size_t(), C.c_int32(), C.c_int32(), C.c_int32()
    err = C.create_string_buffer(256)
    st = lib.fav_attn_tap_info(C.byref(cfg), C.byref(nbytes), C.byref(layers), C.byref(tokens), C.byref(ld), err, len(err))
    return st, (nbytes.value, layers.value, tokens.value, ld.value), err.value.decode()


def test_attn_tap_info_needs_no_device(lib):
    from failure_aware_vision_amd import _lib
    st, got, msg = tap_info(lib, _lib.ARCH_VIT_B16)               # 224 x 224, max_batch 256
    assert st == 0 and msg == "" and got == (12 * 256 * 197 * 208 * 4, 12, 197, 208)
    st, got, _ = tap_info(lib, _lib.ARCH_VIT_B16, max_batch=8)
    assert st == 0 and got == (12 * 8 * 197 * 208 * 4, 12, 197, 208)
    st, got, _ = tap_info(lib, _lib.ARCH_VIT_TINY, max_batch=4)   # the miniature at 64 x 64
    assert st == 0 and got == (2 * 4 * 17 * 32 * 4, 2, 17, 32)
    st, got, _ = tap_info(lib, _lib.ARCH_VIT_TINY, max_batch=4, in_h=48, in_w=64)
    assert st == 0 and got == (2 * 4 * 13 * 16 * 4, 2, 13, 16)
    st, got, _ = tap_info(lib, _lib.ARCH_VIT_TINY, max_batch=1, in_h=240, in_w=272)       # 255 patches: the most the path takes
    assert st == 0 and got == (2 * 256 * 256 * 4, 2, 256, 256)
    cfg = _lib.FavConfig()
    lib.fav_default_config(C.byref(cfg), _lib.ARCH_VIT_B16)
    assert lib.fav_attn_tap_info(C.byref(cfg), None, None, None, None, None, 0) == 0


def test_attn_tap_info_refusals(lib):
    from failure_aware_vision_amd import _lib
    for arch in (_lib.ARCH_RESNET50, _lib.ARCH_RESNET18_CIFAR):
        st, _, msg = tap_info(lib, arch)
        assert st == 6 and "fav_attn_tap_info" in msg and "ResNet" in msg, msg
    for arch in (_lib.ARCH_VIT_B16, _lib.ARCH_RESNET50):
        st, _, msg = tap_info(lib, arch, n_members=5)
        assert st == 6 and "fav_attn_tap_info" in msg and "ensemble" in msg, msg
    st, _, msg = tap_info(lib, _lib.ARCH_VIT_B16, math_mode=_lib.MATH_F32_EXACT)
    assert st == 6 and "FAV_MATH_F32_EXACT" in msg, msg
    st, _, msg = tap_info(lib, _lib.ARCH_VIT_B16, struct_size=8)
    assert st == 1 and "struct_size" in msg
    st, _, msg = tap_info(lib, _lib.ARCH_VIT_B16, max_batch=0)
    assert st == 1 and "fav_attn_tap_info" in msg
    st, _, msg = tap_info(lib, _lib.ARCH_VIT_B16, in_h=230)
    assert st == 1 and "patch" in msg, msg
    st, _, msg = tap_info(lib, _lib.ARCH_VIT_B16, in_h=512, in_w=512)
    assert st == 6 and "256 tokens" in msg, msg
    assert lib.fav_attn_tap_info(None, None, None, None, None, None, 0) == 1


# ---- the numpy rollout on hand-made attention --------------------------------------------------------------------------------
def test_identity_attention_keeps_everything_on_the_class_token():
    L, n, gh, gw = 5, 2, 3, 4
    T = gh * gw + 1
    A = np.zeros((L, n, T, R.attn_ld(T)), F32)
    A[:, :, np.arange(T), np.arange(T)] = 1.0
    for fl in (0, 2, L - 1):
        M, rec = R.rollout(A, gh, gw, fl)
        r = rec.view(F32)
        assert not M.view(np.uint32).any()                            # all +0
        assert (r[:, 1] == 1.0).all() and (rec[:, 0] == L - fl).all()  # cls_mass, n_layers
        assert (r[:, 2] == 0).all() and (r[:, 4] == 0).all() and (r[:, 5] == 0).all() and (rec[:, 3] == 0).all()
        assert (rec[:, 6] == 0).all() and (rec[:, 7] == -1).all()     # a flat map: nothing above, no box


def test_one_patch_worked_by_hand():
    """T = 2 (the class token and one patch), L = 2.  A_1 = [[3/4, 1/4], [.., ..]], A_0 = [[1/2, 1/2], [1/4, 3/4]]:
    A~_1 row 0 = (7/8, 1/8); A~_0 = [[3/4, 1/4], [1/8, 7/8]]; r = (7/8 * 3/4 + 1/8 * 1/8, 7/8 * 1/4 + 1/8 * 7/8)
    = (43/64, 21/64) - every value exact in float32."""
    A = np.zeros((2, 1, 2, 4), F32)
    A[1, 0, :, :2] = [[0.75, 0.25], [0.5, 0.5]]
    A[0, 0, :, :2] = [[0.5, 0.5], [0.25, 0.75]]
    M, rec = R.rollout(A, 1, 1, 0)
    r = rec.view(F32)
    assert M.shape == (1, 1) and M[0, 0] == F32(21 / 64) and r[0, 1] == F32(43 / 64)
    assert rec[0, 0] == 2 and r[0, 2] == r[0, 4] == r[0, 5] == F32(21 / 64) and rec[0, 3] == 0
    assert rec[0, 6] == 0 and rec[0, 7] == -1                          # one cell: peak == floor, no box
    M, rec = R.rollout(A, 1, 1, 1)                                     # the last layer alone
    assert M[0, 0] == F32(0.125) and rec.view(F32)[0, 1] == F32(0.875) and rec[0, 0] == 1


def test_record_rules():
    """Ties go to the lowest cell, a NaN never wins, the threshold is the midpoint and the box spans ALL cells at or above it."""
    gh, gw = 3, 4
    M = np.array([[0.1, 0.5, 0.2, 0.5, 0.1, 0.1, 0.3, 0.1, 0.05, 0.1, 0.1, 0.4]], F32)
    rec = R.rollout_records(M, np.array([0.25], F32), 7, gw)
    r = rec.view(F32)
    assert rec[0, 0] == 7 and r[0, 1] == F32(0.25) and r[0, 2] == F32(0.5) and rec[0, 3] == 1 and r[0, 4] == F32(0.05)
    thr = F32(0.05) + F32(0.5) * (F32(0.5) - F32(0.05))
    cells = np.nonzero(M[0] >= thr)[0]
    assert list(cells) == [1, 3, 6, 11] and rec[0, 6] == 4
    assert rec[0, 7] == (1 | 0 << 8 | 3 << 16 | 2 << 24)
    total = F32(0)
    for v in M[0]:
        total = total + v
    assert r[0, 5] == total
    M[0, 2] = np.nan
    rec = R.rollout_records(M, np.array([0.25], F32), 7, gw)
    assert rec[0, 3] == 1 and rec.view(F32)[0, 2] == F32(0.5) and np.isnan(rec.view(F32)[0, 5]) and rec[0, 6] == 4


@pytest.mark.parametrize("L,gh,gw", [(1, 2, 2), (4, 4, 4), (12, 14, 14)])
def test_reference_against_float64(L, gh, gw):
    """Random row-stochastic matrices.  Every entry of r and of A~ lies in [0, 1] and r sums to at most 1 + rounding, so each of
    the 2 T operations of a column's chain errs by at most u = 2^-24 times a partial sum <= 1 (+ the 2 roundings of A~):
    a layer adds at most (2 T + 2) u to an entry, and the error a layer inherits passes through a stochastic matrix, whose
    columns may gather all of it: |err| <= L * T * (2 T + 2) * u, crude and sufficient."""
    n, T = 3, gh * gw + 1
    rng = np.random.default_rng(L * 100 + T)
    s = rng.standard_normal((L, n, T, T)) * 2.0
    e = np.exp(s - s.max(-1, keepdims=True))
    A = np.zeros((L, n, T, R.attn_ld(T)), F32)
    A[..., :T] = (e / e.sum(-1, keepdims=True)).astype(F32)
    A64 = A[..., :T].astype(np.float64)
    for fl in sorted({0, L - 1}):
        M, rec = R.rollout(A, gh, gw, fl)
        M64 = R.rollout_f64(A64, fl)
        err = np.abs(M.astype(np.float64) - M64).max()
        assert err <= L * T * (2 * T + 2) * 2.0 ** -24, err
        if L - fl > 1:
            assert err > 0                                            # a float32 chain, not the float64 answer rounded
        # the record's sums: the map and the class token's mass make up the row, which sums to 1
        r = rec.view(F32)
        assert np.abs(r[:, 1].astype(np.float64) + r[:, 5] - 1.0).max() < 1e-5
    # without the identity term, or with one layer only, the float64 map is another map
    if L > 1:
        assert np.abs(R.rollout_f64(A64, 0, identity=False) - R.rollout_f64(A64, 0)).max() > 1e-3
        assert np.abs(R.rollout_f64(A64, L - 1) - R.rollout_f64(A64, 0)).max() > 1e-3


def test_attn_mean_reference_against_float64():
    """The float32 head-mean attention of the oracle's score and softmax models against softmax(q k^T / 8) in float64: the
    exponential's polynomial is good to 2.9e-6 relative, the scores to fp32 rounding (a few 1e-6 at these magnitudes)."""
    import torch
    rng = np.random.default_rng(5)
    n, T, heads = 2, 21, 3
    x = rng.standard_normal((n, T, 3 * 64 * heads)).astype(F32)
    x[:, :, :64 * heads] *= 2.0
    x = torch.from_numpy(x).to(torch.bfloat16).float().numpy()
    A = R.attn_mean(x, heads)
    assert A.shape == (n, T, 32) and not A[:, :, T:].view(np.uint32).any()
    D = 64 * heads
    q = x[:, :, :D].reshape(n, T, heads, 64).transpose(0, 2, 1, 3).astype(np.float64)
    k = x[:, :, D:2 * D].reshape(n, T, heads, 64).transpose(0, 2, 1, 3).astype(np.float64)
    s = q @ k.transpose(0, 1, 3, 2) / 8.0
    e = np.exp(s - s.max(-1, keepdims=True))
    ref = (e / e.sum(-1, keepdims=True)).mean(1)
    assert np.abs(A[:, :, :T] - ref).max() < 2e-5 and A[:, :, :T].max() > 0.3


# ---- failure_aware_vision_amd.rollout -------------------------------------------------------------------------------------------
def test_unpack_and_patch_box():
    from failure_aware_vision_amd.rollout import ROLLOUT_RECORD_DWORDS, VIT_PATCH, patch_box_to_pixels, unpack_rollout_records
    assert ROLLOUT_RECORD_DWORDS == R.RECORD_DWORDS and VIT_PATCH == 16
    M = np.array([[0.1, 0.5, 0.2, 0.5, 0.1, 0.1, 0.3, 0.1, 0.05, 0.1, 0.1, 0.4], [0.2] * 12], F32)
    rec = R.rollout_records(M, np.array([0.25, 0.5], F32), 3, 4)
    u = unpack_rollout_records(rec)
    assert list(u["n_layers"]) == [3, 3] and list(u["peak_cell"]) == [1, 0] and list(u["n_above"]) == [4, 0]
    assert u["cls_mass"].dtype == np.float32 and list(u["cls_mass"]) == [0.25, 0.5]
    assert [int(u[k][0]) for k in ("x0", "y0", "x1", "y1")] == [1, 0, 3, 2]
    assert [int(u[k][1]) for k in ("x0", "y0", "x1", "y1")] == [-1, -1, -1, -1] and u["box"][1] == -1
    assert patch_box_to_pixels((1, 0, 3, 2)) == (16, 0, 64, 48)
    assert patch_box_to_pixels((0, 0, 0, 0), patch=8) == (0, 0, 8, 8)
    assert patch_box_to_pixels((-1, -1, -1, -1)) is None
    with pytest.raises(ValueError):
        patch_box_to_pixels((3, 0, 1, 2))
    with pytest.raises(ValueError):
        unpack_rollout_records(np.zeros((2, 7), np.int32))
    import torch
    t = unpack_rollout_records(torch.from_numpy(rec))
    for key, v in u.items():
        assert np.array_equal(t[key].numpy(), v), key


def test_qk_gain_defaults_to_the_checkpoint_as_it_was():
    from failure_aware_vision_amd import weights
    from oracle import fav_oracle as O
    a, _ = weights.make_synthetic_vit("vit_tiny", seed=3)
    b, _ = weights.make_synthetic_vit("vit_tiny", seed=3, qk_gain=1.0)
    c, _ = weights.make_synthetic_vit("vit_tiny", seed=3, qk_gain=2.0)
    assert a == b and a != c and len(a) == len(c)
    la, lc = O.parse_blob(a).layers, O.parse_blob(c).layers
    D = 128
    for i, (x, y) in enumerate(zip(la, lc)):
        if x.cout == 3 * D:                                           # a qkv layer: Q and K rows doubled (exact in bf16), V as it was
            wa, wc = x.w.reshape(3 * D, -1), y.w.reshape(3 * D, -1)
            assert np.array_equal(wc[:2 * D], 2 * wa[:2 * D]) and np.array_equal(wc[2 * D:], wa[2 * D:])
            assert np.array_equal(y.b[:2 * D], 2 * x.b[:2 * D]) and np.array_equal(y.b[2 * D:], x.b[2 * D:])
        else:
            assert np.array_equal(x.w, y.w) and np.array_equal(x.b, y.b), i


def test_documents_state_the_measured_cost():
    """DESIGN.md item 5j sets the measured tap cost and the float64 figures beside the expectation, from the records the tools wrote."""
    design = open(os.path.join(ROOT, "DESIGN.md")).read()
    item = design[design.index("5j. Attention rollout"):design.index("6. ViT: bf16 at every tensor boundary")]
    assert "profiles/rollout_tap_bench.txt" in item and "profiles/rollout_tapoff_ab.txt" in item
    assert "1.905e-02" in item and "6.363e-03" in item           # the measured values behind test_gpu_rollout.py's F64_BOUND
    profile = open(os.path.join(ROOT, "profiles", "rollout_tap_bench.txt")).read()
    rows = [line for line in profile.splitlines() if line.startswith(("classify_", "rollout "))]
    assert len(rows) == 10 and "gfx950" in profile
    for line in rows:
        if line.startswith("classify_detect"):
            assert line[32:].split()[0] in item, line                # the medians of the record are the figures of the document
    assert os.path.exists(os.path.join(ROOT, "profiles", "rollout_tapoff_ab.txt"))
