"""Mid-level patch maps without a device: the numpy restatement tests/patch_local_ref.py held to
the k-NN head's query at radius 0, to a float64 direct sum, and to the locality the contract states; the stage geometry of the
planner (fav_stage_tap_info) against the oracle's block outputs; the layout of fav_patch_site over fav.h; fav_check_patch_site;
the new symbols; the Python side (patch.aggregate_cells, PatchBank's site)."""
import ctypes as C
import os
import subprocess

import numpy as np
import pytest

import knn_ref as K
import patch_local_ref as L
from failure_aware_vision_amd import _lib, patch, weights
from failure_aware_vision_amd.patch import PatchBank
from oracle import fav_oracle as O

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
R50, R18 = _lib.ARCH_RESNET50, _lib.ARCH_RESNET18_CIFAR


@pytest.fixture(scope="module")
def lib():
    return _lib.load()


def bits(rng, shape, scale=1.0):
    return K.f32_to_bf16_bits((rng.standard_normal(shape) * scale).astype(np.float32))


# ---- the reference -----------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("S", (1, 3))
def test_radius_0_is_the_knn_query_bit_for_bit(S):
    rng = np.random.default_rng(S)
    maps = bits(rng, (S, 2, 3 * 4, 128))
    maps[:, 1, 5] = 0                                                                # a degenerate cell
    q, ss, bad = L.query(maps, (3, 4), 0)
    q0, ss0, bad0 = K.query(maps.reshape(S, 24, 128))
    assert bad[17] and np.array_equal(bad, bad0)
    assert np.array_equal(q.view(np.uint32), q0.view(np.uint32)) and np.array_equal(ss.view(np.uint32), ss0.view(np.uint32))


@pytest.mark.parametrize("radius", (1, 2))
def test_aggregate_against_a_float64_direct_sum(radius):
    """The direct (non-separable) sum over the neighbourhood in float64 of the float64 mean.  The reference adds S values
    (S - 1 roundings that count, the first addition to +0 is exact) and multiplies once, adds at most 2r + 1 rows (2r roundings)
    and at most 2r + 1 columns (2r roundings): with u = 2^-24 every rounding is relative u of a partial sum, which is at most
    the sum of the absolute values A of the terms of the cell; the constant (float)(1.0 / S) is itself a rounding of 1 / S.
    |error| <= ((S - 1) + 2 + 4r) * u * A * (1 + u)^(S + 1 + 4r)."""
    rng = np.random.default_rng(radius)
    S, n, Hf, Wf, Cc = 3, 2, 5, 6, 64
    maps = bits(rng, (S, n, Hf * Wf, Cc))
    a = L.aggregate(maps.reshape(S, n, Hf, Wf, Cc), radius).astype(np.float64)
    x = K.bf16_to_f32(maps).astype(np.float64).reshape(S, n, Hf, Wf, Cc)
    m, mabs = x.sum(axis=0) / S, np.abs(x).sum(axis=0) / S
    want, A = np.zeros_like(m), np.zeros_like(m)
    for y in range(Hf):
        for xx in range(Wf):
            y0, y1, x0, x1 = max(0, y - radius), min(Hf, y + radius + 1), max(0, xx - radius), min(Wf, xx + radius + 1)
            want[:, y, xx] = m[:, y0:y1, x0:x1].sum(axis=(1, 2))
            A[:, y, xx] = mabs[:, y0:y1, x0:x1].sum(axis=(1, 2))
    u = 2.0 ** -24
    bound = (S + 1 + 4 * radius) * u * A * (1 + u) ** (S + 1 + 4 * radius)
    assert (np.abs(a - want) <= bound).all() and np.abs(a - want).max() > 0
    # the library's own numpy function is the same additions
    assert np.array_equal(patch.aggregate_cells(maps.reshape(S, n, Hf, Wf, Cc), radius).view(np.uint32), a.astype(np.float32).view(np.uint32))


@pytest.mark.parametrize("radius", (0, 1, 2))
def test_a_frame_does_not_see_its_neighbours(radius):
    rng = np.random.default_rng(5)
    maps = bits(rng, (2, 3, 3 * 3, 64))
    q = L.query(maps, (3, 3), radius)[0].reshape(3, 9, 64)
    other = maps.copy()
    other[:, 0], other[:, 2] = bits(rng, (2, 9, 64), 2.0 ** 20), bits(rng, (2, 9, 64), 2.0 ** 20)
    q2 = L.query(other, (3, 3), radius)[0].reshape(3, 9, 64)
    assert np.array_equal(q[1].view(np.uint32), q2[1].view(np.uint32)) and not np.array_equal(q[0], q2[0])


@pytest.mark.parametrize("radius,k,at", [(1, 1, (3, 3)), (2, 2, (2, 4)), (1, 2, (0, 0)), (2, 1, (6, 7)), (0, 2, (5, 1))])
def test_a_changed_block_changes_exactly_its_surroundings(radius, k, at):
    """A k x k block of changed cells changes the (k + 2r)^2 cells around it, clipped at the border, and no other."""
    Hf, Wf = 7, 8
    rng = np.random.default_rng(11)
    maps = bits(rng, (1, 1, Hf * Wf, 64)).reshape(1, 1, Hf, Wf, 64)
    changed = maps.copy()
    y, x = at
    changed[0, 0, y:y + k, x:x + k] = bits(rng, (k, k, 64), 3.0)
    q = L.query(maps.reshape(1, 1, -1, 64), (Hf, Wf), radius)[0].reshape(Hf, Wf, 64)
    q2 = L.query(changed.reshape(1, 1, -1, 64), (Hf, Wf), radius)[0].reshape(Hf, Wf, 64)
    differs = (q != q2).any(axis=2)
    want = np.zeros((Hf, Wf), bool)
    want[max(0, y - radius):min(Hf, y + k + radius), max(0, x - radius):min(Wf, x + k + radius)] = True
    assert np.array_equal(differs, want)
    assert want.sum() == (min(Hf, y + k + radius) - max(0, y - radius)) * (min(Wf, x + k + radius) - max(0, x - radius))


def test_degenerate_is_a_property_of_the_neighbourhood():
    maps = np.zeros((1, 1, 5 * 5, 64), np.uint16).reshape(1, 1, 5, 5, 64)
    maps[0, 0, 0, 1] = bits(np.random.default_rng(0), (64,))                         # one non-zero cell, at (0, 1)
    flat = maps.reshape(1, 1, 25, 64)
    for radius, live in ((0, {(0, 1)}), (1, {(y, x) for y in (0, 1) for x in (0, 1, 2)}), (2, {(y, x) for y in (0, 1, 2) for x in (0, 1, 2, 3)})):
        q, ss, bad = L.query(flat, (5, 5), radius)
        got = {(i // 5, i % 5) for i in np.flatnonzero(~bad)}
        assert got == live, radius                                                   # a zero cell with a non-zero neighbour has a direction
        assert (q[bad] == 0).all() and (ss[bad] == 0).all()
    # an overflowing neighbourhood is degenerate too: bf16 max squared is not finite in fp32
    maps[0, 0, 4, 4, 0] = 0x7F7F
    bad = L.query(maps.reshape(1, 1, 25, 64), (5, 5), 1)[2].reshape(5, 5)
    assert bad[3:, 3:].all() and not bad[0, 1]


# ---- the planner's stage geometry ---------------------------------------------------------------------------------------------
def stage_info(lib, arch, stage, **kw):
    cfg = _lib.FavConfig()
    lib.fav_default_config(C.byref(cfg), arch)
    for k, v in kw.items():
        setattr(cfg, k, v)
    nbytes, s, hf, wf, c = C.c_size_t(), C.c_int32(), C.c_int32(), C.c_int32(), C.c_int32()
    err = C.create_string_buffer(256)
    st = lib.fav_stage_tap_info(C.byref(cfg), stage, C.byref(nbytes), C.byref(s), C.byref(hf), C.byref(wf), C.byref(c), err, len(err))
    return st, (nbytes.value, s.value, hf.value, wf.value, c.value), err.value.decode()


def conv_out(x, k, s, p):
    return (x + 2 * p - k) // s + 1


STAGE_ENDS = {R50: (2, 6, 12, 15), R18: (1, 3, 5, 7)}                                 # the last block of torchvision's layer1 .. layer4
GEOM_SIZES = [(32, 32), (64, 64), (33, 47), (63, 65), (224, 224)]
ORACLE_MAX = 65                                                                       # the oracle itself runs up to here


def chained_shapes(net, h, w):
    """(h, w, c) behind every block, from the oracle's own layer table (PyTorch's convolution arithmetic)."""
    Lr = net.m.layers[0]
    h, w = conv_out(h, Lr.kh, Lr.stride, Lr.pad), conv_out(w, Lr.kw, Lr.stride, Lr.pad)
    if net.cfg["stem"] == "imagenet":
        h, w = conv_out(h, 3, 2, 1), conv_out(w, 3, 2, 1)
    out = []
    for main, _ in net.blocks:
        for Lr in main:
            h, w = conv_out(h, Lr.kh, Lr.stride, Lr.pad), conv_out(w, Lr.kw, Lr.stride, Lr.pad)
        out.append((h, w, main[-1].cout))
    return out


@pytest.mark.parametrize("arch", [R50, R18], ids=["resnet50", "resnet18_cifar"])
def test_stage_geometry_is_the_oracles(lib, arch, r50_blob, r18_blob, monkeypatch):
    monkeypatch.setattr(O, "epilogue", O.epilogue_numpy)                              # shapes are all this test reads
    net = O.OracleNet(O.parse_blob((r50_blob if arch == R50 else r18_blob)[0]))
    assert net.nb == STAGE_ENDS[arch][3] + 1
    mc = dict(n_samples=3, dropout_p=0.1, site_mask=weights.site_mask_for(arch, "all_blocks"))
    for h, w in GEOM_SIZES:
        shapes = chained_shapes(net, h, w)
        if max(h, w) <= ORACLE_MAX:
            act = net.stem(np.zeros((1, h, w, 3), np.float32))
            for i in range(net.nb):
                act = net.block(i, act)
                assert tuple(act.shape[1:]) == shapes[i], (h, w, i)
        for stage in (1, 2, 3, 4):
            want = shapes[STAGE_ENDS[arch][stage - 1]]
            for S, kw in ((1, {}), (3, mc)):
                st, dims, msg = stage_info(lib, arch, stage, in_h=h, in_w=w, max_batch=3, **kw)
                assert st == 0 and msg == "", (h, w, stage, msg)
                assert dims == (S * 3 * want[0] * want[1] * want[2] * 2, S) + want, (h, w, stage, dims)
    # stage 4 is the map tap's
    from test_cam_host import tap_info
    assert stage_info(lib, arch, 4, in_h=33, in_w=47, max_batch=3, **mc)[1] == tap_info(lib, arch, in_h=33, in_w=47, max_batch=3, **mc)[1]
    if arch == R50:
        assert [stage_info(lib, arch, s)[1][2:] for s in (1, 2, 3, 4)] == [(56, 56, 256), (28, 28, 512), (14, 14, 1024), (7, 7, 2048)]


def test_stage_tap_info_refusals(lib):
    for stage in (0, 5, -1):
        st, _, msg = stage_info(lib, R50, stage)
        assert st == 1 and f"fav_stage_tap_info: stage={stage}" in msg
    st, _, msg = stage_info(lib, _lib.ARCH_VIT_B16, 2)
    assert st == 6 and "ViT" in msg
    st, _, msg = stage_info(lib, R50, 2, n_members=2)
    assert st == 6 and "ensemble" in msg
    cfg = _lib.FavConfig()
    lib.fav_default_config(C.byref(cfg), R50)
    assert lib.fav_stage_tap_info(C.byref(cfg), 3, None, None, None, None, None, None, 0) == 0      # every pointer may be NULL
    assert lib.fav_set_stage_tap(None, 2, 0) == 1 and lib.fav_get_stage_maps(None, None, None, None, None, None, None, None, None) == 1
    assert lib.fav_set_patch_bank_at(None, None, None) == 1


def test_the_mark_changes_no_schedule(lib):
    """Op::stage_out is a mark: the dumps of fav_plan_schedule hold what they held (its fields are listed, the mark is not one)."""
    from test_gpu_schedule_sweep import plan_of
    ops = plan_of("resnet50", (64, 64), "bf16", max_batch=4)
    assert ops and all("stage" not in "".join(o) for o in ops)


# ---- fav_patch_site -------------------------------------------------------------------------------------------------------------
_LAYOUT_C = r"""
#include <stddef.h>
#include <stdio.h>
#include "fav.h"
int main(void) {
    printf("site_size %zu\nbank_size %zu\nrecord_size %zu\nconfig_size %zu\n", sizeof(fav_patch_site), sizeof(fav_patch_bank),
           sizeof(fav_patch_record), sizeof(fav_config));
    printf("stage %zu\nradius %zu\n", offsetof(fav_patch_site, stage), offsetof(fav_patch_site, radius));
    printf("abi %d\nkcount %d\n", (int)FAV_ABI_VERSION, (int)FAV_K_COUNT);
    return 0;
}
"""
SYMBOLS = ("fav_stage_tap_info", "fav_set_stage_tap", "fav_get_stage_maps", "fav_op_patch_query", "fav_op_patch_score_at",
           "fav_check_patch_site", "fav_set_patch_bank_at")


def test_layout_symbols_and_abi(lib, tmp_path):
    src = tmp_path / "layout.c"
    src.write_text(_LAYOUT_C)
    exe = str(tmp_path / "layout")
    subprocess.check_call(["gcc", "-std=c11", "-Wall", "-Werror", "-I" + os.path.join(ROOT, "include"), str(src), "-o", exe])
    out = dict(line.split() for line in subprocess.check_output([exe], text=True).splitlines())
    assert int(out["site_size"]) == 12 == C.sizeof(_lib.FavPatchSite)
    assert (int(out["stage"]), int(out["radius"])) == (4, 8) == (_lib.FavPatchSite.stage.offset, _lib.FavPatchSite.radius.offset)
    assert int(out["bank_size"]) == 32 == C.sizeof(_lib.FavPatchBank) and int(out["record_size"]) == 32
    assert int(out["abi"]) == 2 == lib.fav_abi_version() and int(out["config_size"]) == 120 and int(out["kcount"]) == 6
    header = open(os.path.join(ROOT, "include", "fav.h")).read()
    for sym in SYMBOLS:
        assert sym in _lib._SIGNATURES and hasattr(lib, sym) and sym + "(" in header, sym
        assert getattr(lib, sym).argtypes == _lib._SIGNATURES[sym][1]
    import failure_aware_vision_amd as pkg
    for name in ("stage_tap_info", "set_stage_tap", "stage_maps"):
        assert hasattr(pkg.Backend, name), name


def check_site(lib, **kw):
    s = _lib.FavPatchSite()
    s.struct_size, s.stage, s.radius = 12, 2, 1
    for k, v in kw.items():
        setattr(s, k, v)
    err = C.create_string_buffer(256)
    return lib.fav_check_patch_site(C.byref(s), err, len(err)), err.value.decode()


def test_check_patch_site(lib):
    for stage in (1, 2, 3, 4):
        for radius in (0, 1, 2):
            assert check_site(lib, stage=stage, radius=radius) == (0, "")
    for kw, text in ((dict(stage=0), "stage=0"), (dict(stage=5), "stage=5"), (dict(stage=-1), "stage=-1"), (dict(radius=-1), "radius=-1"),
                     (dict(radius=3), "radius=3"), (dict(struct_size=8), "struct_size=8"), (dict(struct_size=16), "struct_size=16")):
        st, msg = check_site(lib, **kw)
        assert st == 1 and text in msg, (kw, msg)
    err = C.create_string_buffer(64)
    assert lib.fav_check_patch_site(None, err, len(err)) == 1 and b"site is NULL" in err.value
    assert lib.fav_check_patch_site(None, None, 0) == 1


# ---- the Python side -------------------------------------------------------------------------------------------------------------
def test_patch_bank_site_round_trip(tmp_path):
    rows = K.f32_to_bf16_bits(np.eye(5, 64, dtype=np.float32))
    plain = PatchBank(rows, grid=(2, 2))
    assert plain.stage is None and plain.radius == 0 and plain.site_to_c() is None
    plain.save(tmp_path / "plain.npz")
    with np.load(tmp_path / "plain.npz") as z:
        assert sorted(z.files) == ["chunk_rows", "grid", "n_dropped", "rows", "threshold"]   # a plain bank's file is what it was
    back = PatchBank.load(tmp_path / "plain.npz")
    assert back.stage is None and back.radius == 0
    bank = PatchBank(rows, threshold=0.5, grid=(4, 4), stage=3, radius=1)
    bank.save(tmp_path / "site.npz")
    back = PatchBank.load(tmp_path / "site.npz")
    assert (back.stage, back.radius, back.grid, back.threshold) == (3, 1, (4, 4), 0.5)
    s = bank.site_to_c()
    assert (s.struct_size, s.stage, s.radius) == (12, 3, 1)
    assert (bank.with_threshold(1.0).stage, bank.take([0, 2]).radius, bank.take([0, 2]).stage) == (3, 1, 3)
    with pytest.raises(ValueError, match="needs a stage"):
        PatchBank(rows, radius=1)


def test_cell_rows_with_a_radius():
    rng = np.random.default_rng(3)
    maps = bits(rng, (2, 2, 3, 4, 64))
    rows, ok, grid = patch.cell_rows(maps, 1)
    q, _, bad = L.query(maps.reshape(2, 2, 12, 64), (3, 4), 1)
    assert grid == (3, 4) and ok.all() and not bad.any()
    # float64 normalisation of the same aggregate: the rows agree with the device's query to a bf16 step
    assert np.abs(K.bf16_to_f32(rows).astype(np.float64) - q).max() <= 2.0 ** -8
    assert np.array_equal(patch.cell_rows(maps, 0)[0], patch.cell_rows(maps.reshape(2, 2, 12, 64))[0])
    with pytest.raises(ValueError, match="radius=3"):
        patch.aggregate_cells(maps, 3)
