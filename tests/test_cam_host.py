"""CPU-side checks of the class activation maps: the fav_cam_record layout (C vs ctypes) and the new symbols, the numpy
reference (tests/cam_ref.py) that the GPU file compares bits with - against float64 within the bound of its chain lengths,
its heatmap against torch's bilinear resize, its record rules - the host helpers of failure_aware_vision_amd.cam, and
fav_map_tap_info through the loaded library (the planner alone, no device)."""
import ctypes as C
import os
import subprocess

import numpy as np
import pytest

import cam_ref as R

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
    printf("record_size %zu\n", sizeof(fav_cam_record));
    printf("record_align %zu\n", _Alignof(fav_cam_record));
    printf("config_size %zu\n", sizeof(fav_config));
#define G(x) printf("r.%s %zu\n", #x, offsetof(fav_cam_record, x));
    G(class_id) G(logit_mean) G(peak) G(peak_cell) G(floor) G(pos_sum) G(n_above) G(box)
    printf("abi %d\nkcount %d\n", (int)FAV_ABI_VERSION, (int)FAV_K_COUNT);
    return 0;
}
"""

SYMBOLS = ("fav_set_map_tap", "fav_get_maps", "fav_map_tap_info", "fav_cam", "fav_classify_cam", "fav_op_cam", "fav_op_cam_heatmap")
FIELDS = ("class_id", "logit_mean", "peak", "peak_cell", "floor", "pos_sum", "n_above", "box")


def test_layout_symbols_and_abi(lib, tmp_path):
    from failure_aware_vision_amd import _lib
    src = tmp_path / "layout.c"
    src.write_text(_LAYOUT_C)
    exe = str(tmp_path / "layout")
    subprocess.check_call(["gcc", "-std=c11", "-Wall", "-Werror", "-I" + os.path.join(ROOT, "include"), str(src), "-o", exe])
    out = dict(line.split() for line in subprocess.check_output([exe], text=True).splitlines())
    assert int(out["record_size"]) == C.sizeof(_lib.FavCamRecord) == 32 == 4 * R.RECORD_DWORDS
    # the record holds 4-byte fields only; the 8-byte alignment is what the head asks of rec_dev, for its 8-byte stores
    assert int(out["record_align"]) == 4
    for i, name in enumerate(FIELDS):
        assert int(out["r." + name]) == getattr(_lib.FavCamRecord, name).offset == 4 * i, name
    # what this feature must not move: the ABI version, fav_config, the kernel classes
    assert int(out["abi"]) == 2 == lib.fav_abi_version()
    assert int(out["config_size"]) == C.sizeof(_lib.FavConfig) == 120
    assert int(out["kcount"]) == 6 == _lib.K_COUNT
    header = open(os.path.join(ROOT, "include", "fav.h")).read()
    for sym in SYMBOLS:
        assert sym in _lib._SIGNATURES and hasattr(lib, sym) and sym + "(" in header, sym
        assert getattr(lib, sym).argtypes == _lib._SIGNATURES[sym][1]
    import failure_aware_vision_amd as pkg
    for name in ("unpack_cam_records", "box_to_pixels", "evidence_share", "cam"):
        assert hasattr(pkg, name), name
    for name in ("set_map_tap", "map_tap_info", "maps", "cam", "classify_cam"):
        assert hasattr(pkg.Backend, name), name


def test_entry_points_refuse_a_null_handle(lib):
    assert lib.fav_set_map_tap(None, 1, 0) == 1
    assert lib.fav_get_maps(None, None, None, None, None, None, None, None) == 1
    assert lib.fav_cam(None, None, 1, None, None, None) == 1
    assert lib.fav_classify_cam(None, None, 1, 0, 0, None, None, None, None, None, None, None) == 1


# ---- the reference -------------------------------------------------------------------------------------------------------
def random_case(seed, S, n, HW, C, n_classes, ldw=None, scale=1.0):
    """-> (x_bits [S, n, HW, C], w_bits [n_classes, ldw], bias): ReLU-like maps (half the values zero), signed weights."""
    rng = np.random.default_rng(seed)
    ldw = ldw or C
    x = np.maximum(rng.standard_normal((S, n, HW, C)), 0.0).astype(np.float32) * np.float32(scale)
    w = (rng.standard_normal((n_classes, ldw)) * 0.05).astype(np.float32)
    return R.f32_to_bf16_bits(x), R.f32_to_bf16_bits(w), rng.standard_normal(n_classes).astype(np.float32)


@pytest.mark.parametrize("S,C", [(1, 512), (3, 2048), (7, 1024)])
def test_reference_maps_against_float64(S, C):
    n, HW, NC = 2, 9, 11
    xb, wb, _ = random_case(S * 1000 + C, S, n, HW, C, NC)
    classes = np.array([[0, 10, 3], [5, 5, 7]])
    M = R.cam_maps(xb, wb, classes, NC)
    x64, w64 = R.bf16_bits_to_f32(xb).astype(np.float64), R.bf16_bits_to_f32(wb).astype(np.float64)
    prod = np.einsum("snhc,nkc->snkhc", x64, w64[classes])          # exact: a product of two bf16 values has 16 bits
    M64 = prod.sum(axis=(0, 4)) / S
    mag = np.abs(prod).sum(axis=(0, 4)) / S
    # a lane's chain has S * C / 64 additions, the halving six more, the scaling one rounding (inside the + 6's slack of the
    # standard (length) * u * sum|terms| bound at u = 2^-24)
    bound = (S * C / 64 + 6) * 2.0 ** -24 * mag
    err = np.abs(M.astype(np.float64) - M64)
    assert (err <= bound).all(), (err / bound).max()
    assert err.max() > 0          # and it is a float32 chain, not the float64 answer rounded


def test_reference_partition_is_the_stated_one():
    """One nonzero channel: the map is that single product whichever lane holds it; two channels of one lane add in step order
    before anything of another lane does (a sum that differs from the other order in float32)."""
    S, n, HW, C = 1, 1, 1, 512
    x = np.zeros((S, n, HW, C), np.float32)
    w = np.zeros((1, C), np.float32)
    # lane 0 holds channels 0..7; lane 1 holds 8..15.  a + b is absorbed, then - a leaves 0; in the other order b survives
    x[..., 0], x[..., 1], x[..., 8] = 1.0, 1.0, 1.0
    w[0, 0], w[0, 1], w[0, 8] = 2.0 ** 30, 1.0, -(2.0 ** 30)
    M = R.cam_maps(R.f32_to_bf16_bits(x), R.f32_to_bf16_bits(w), [[0]], 1)
    assert M[0, 0, 0] == 0.0      # (2^30 + 1) rounds to 2^30 inside lane 0, then lane 1's -2^30 arrives in the halving


def torch_heatmap(M, rec, Hf, Wf, H, W):
    import torch
    m = torch.from_numpy(np.asarray(M, np.float64).reshape(-1, 1, Hf, Wf))
    v = torch.nn.functional.interpolate(m, size=(H, W), mode="bilinear", align_corners=False)[:, 0].numpy()
    peak = rec[:, 2].view(np.float32).astype(np.float64)[:, None, None]
    floor = rec[:, 4].view(np.float32).astype(np.float64)[:, None, None]
    with np.errstate(all="ignore"):
        t = np.clip((v - floor) / (peak - floor), 0.0, 1.0) * 255.0
    return t


@pytest.mark.parametrize("hw_in,hw_out", [((7, 7), (224, 224)), ((4, 4), (32, 32)), ((8, 10), (240, 320)), ((1, 1), (5, 3)),
                                          ((3, 5), (7, 4))])
def test_reference_heatmap_against_torch(hw_in, hw_out):
    (Hf, Wf), (H, W) = hw_in, hw_out
    rng = np.random.default_rng(Hf * 100 + Wf)
    M = rng.standard_normal((3, 1, Hf * Wf)).astype(np.float32)
    rec = R.cam_records(M, np.zeros((3, 1), int), np.zeros(1, np.float32), 1, Wf)[:, 0]
    got = R.heatmap(M[:, 0], rec, Hf, Wf, H, W)
    assert got.shape == (3, H, W) and got.dtype == np.uint8
    if Hf * Wf == 1:
        assert not got.any()      # a single cell: peak == floor, a flat map
        return
    want = torch_heatmap(M[:, 0], rec, Hf, Wf, H, W)
    # fp32 error is far below 1 / 255: only a rounding boundary can move, by one grey level
    assert np.abs(got.astype(np.float64) - np.rint(want)).max() <= 1
    assert np.abs(got.astype(np.float64) - want).max() <= 0.5 + 1e-3


def test_reference_heatmap_flat_nan_and_invalid_maps_are_black():
    M = np.array([[2.5] * 4, [np.nan] * 4, [1, np.nan, 3, 2]], np.float32)[:, None, :]
    rec = R.cam_records(M, [[0], [0], [0]], [0.0], 1, 2)[:, 0]
    out = R.heatmap(M[:, 0], rec, 2, 2, 6, 6)
    assert not out[0].any() and not out[1].any()
    assert out[2].any()           # NaN cells never win the peak or the floor; pixels that touch them are 0
    assert out[2][0, 5] == 0 and out[2][5, 0] == 255 and out[2][0, 0] == 0
    bad = R.cam_records(np.zeros((1, 1, 4), np.float32), [[7]], [0.0], 1, 2)[:, 0]
    assert not R.heatmap(np.zeros((1, 4), np.float32), bad, 2, 2, 4, 4).any()


def test_reference_record_rules():
    from failure_aware_vision_amd.cam import unpack_cam_records
    Wf = 3
    maps = np.array([
        [0.5, 4.0, 1.0, 4.0, -2.0, 0.79, 0.8, -2.0, 0.0],           # two equal peaks; thr = 0.8: cells 1, 2, 3, 6
        [-1.0, -3.0, -0.5, -3.0, -2.0, -1.0, -1.0, -1.0, -1.0],     # all negative
        [np.nan] * 9,                                               # all NaN
        [1.0, np.nan, 2.0, 0.0, 0.0, 0.0, 0.0, 0.0, 0.0],           # one NaN: the chains carry it, the scans skip it
        [1.0] * 9,                                                  # out-of-range class below
    ], np.float32)[None]
    rec = R.cam_records(maps, [[0, 1, 1, 0, 2]], [0.25, -1.0], 2, Wf)
    r = {k: v[0] for k, v in unpack_cam_records(rec).items()}
    assert list(r["class_id"]) == [0, 1, 1, 0, -1]
    assert r["peak"][0] == 4.0 and r["peak_cell"][0] == 1 and r["floor"][0] == -2.0
    assert r["n_above"][0] == 4 and (r["x0"][0], r["y0"][0], r["x1"][0], r["y1"][0]) == (0, 0, 2, 2)
    assert r["pos_sum"][0] == np.float32(0.5 + 4 + 1 + 4) + np.float32(0.79) + np.float32(0.8)
    total = np.float32(0)
    for v in maps[0, 0]:
        total = total + v
    assert r["logit_mean"][0] == total * np.float32(1.0 / 9) + np.float32(0.25)
    # all negative: a peak, no extent
    assert r["peak"][1] == -0.5 and r["peak_cell"][1] == 2 and r["floor"][1] == -3.0 and r["pos_sum"][1] == 0.0
    assert r["n_above"][1] == 0 and r["box"][1] == -1 and r["x0"][1] == r["y1"][1] == -1
    # all NaN: nothing wins
    assert r["peak"][2] == -np.inf and r["peak_cell"][2] == -1 and r["floor"][2] == np.inf and r["n_above"][2] == 0
    assert r["box"][2] == -1 and np.isnan(r["logit_mean"][2]) and r["pos_sum"][2] == 0.0
    # one NaN: sums are NaN, fmax drops it from pos_sum, the scans and the extent ignore the cell
    assert np.isnan(r["logit_mean"][3]) and r["pos_sum"][3] == 3.0 and r["peak"][3] == 2.0 and r["peak_cell"][3] == 2
    assert r["n_above"][3] == 2 and (r["x0"][3], r["y0"][3], r["x1"][3], r["y1"][3]) == (0, 0, 2, 0)
    # an out-of-range class
    assert r["peak_cell"][4] == -1 and r["n_above"][4] == 0 and r["box"][4] == -1
    for name in ("logit_mean", "peak", "floor", "pos_sum"):
        assert r[name][4:5].view(np.uint32)[0] == R.QNAN_BITS, name
    Mx = R.cam_maps(np.zeros((1, 1, 9, 512), np.uint16), np.zeros((2, 512), np.uint16), [[0, 2, -1]], 2)
    assert (Mx[0, 0] == 0).all() and (Mx[0, 1:].view(np.uint32) == R.QNAN_BITS).all()


def test_reference_box_packs_coordinates_above_127():
    from failure_aware_vision_amd.cam import unpack_cam_records
    M = np.zeros((1, 1, 200 * 5), np.float32)
    M[0, 0, 199 * 5 + 4] = 1.0
    M[0, 0, 130 * 5 + 1] = 0.5
    r = unpack_cam_records(R.cam_records(M, [[0]], [0.0], 1, 5))
    assert r["box"][0, 0] < -1 and (r["x0"][0, 0], r["y0"][0, 0], r["x1"][0, 0], r["y1"][0, 0]) == (1, 130, 4, 199)


# ---- failure_aware_vision_amd.cam ---------------------------------------------------------------------------------------
def test_unpack_cam_records_numpy_and_torch():
    import torch
    from failure_aware_vision_amd.cam import unpack_cam_records
    rec = np.zeros((2, 3, 8), np.int32)
    rec[..., 0] = [[1, 2, -1]] * 2
    rec.view(np.float32)[..., 1] = 0.5
    rec.view(np.float32)[..., 2] = 3.0
    rec[..., 3] = 7
    rec.view(np.float32)[..., 4] = -1.0
    rec.view(np.float32)[..., 5] = 9.0
    rec[..., 6] = 4
    rec[..., 7] = 1 | 2 << 8 | 5 << 16 | 6 << 24
    rec[1, 2, 7] = -1
    for r in (unpack_cam_records(rec), {k: v.numpy() for k, v in unpack_cam_records(torch.from_numpy(rec)).items()}):
        assert r["class_id"].shape == (2, 3) and r["class_id"][0, 2] == -1
        assert r["logit_mean"].dtype == np.float32 and (r["logit_mean"] == 0.5).all() and (r["peak"] == 3.0).all()
        assert (r["peak_cell"] == 7).all() and (r["floor"] == -1.0).all() and (r["pos_sum"] == 9.0).all() and (r["n_above"] == 4).all()
        assert (r["x0"][0, 0], r["y0"][0, 0], r["x1"][0, 0], r["y1"][0, 0]) == (1, 2, 5, 6)
        assert (r["x0"][1, 2], r["y0"][1, 2], r["x1"][1, 2], r["y1"][1, 2]) == (-1, -1, -1, -1)
    one = unpack_cam_records(rec[:, 0])                 # [n, 8], as classify_cam has them
    assert one["box"].shape == (2,) and one["x1"][0] == 5
    with pytest.raises(ValueError):
        unpack_cam_records(np.zeros((2, 4), np.int32))


def test_box_to_pixels_and_evidence_share():
    from failure_aware_vision_amd.cam import box_to_pixels, evidence_share
    assert box_to_pixels((0, 0, 6, 6), (224, 224), (7, 7)) == (0, 0, 224, 224)
    assert box_to_pixels((2, 3, 2, 3), (224, 224), (7, 7)) == (64, 96, 96, 128)
    assert box_to_pixels((1, 0, 2, 1), (240, 320), (8, 10)) == (32, 0, 96, 60)
    assert box_to_pixels((1, 1, 1, 1), (10, 10), (3, 3)) == (3, 3, 7, 7)       # rounded outwards
    assert box_to_pixels((-1, -1, -1, -1), (224, 224), (7, 7)) is None
    with pytest.raises(ValueError):
        box_to_pixels((0, 0, 7, 6), (224, 224), (7, 7))
    m = np.array([[1.0, -5.0, 0.0], [3.0, 0.0, 4.0]], np.float32)
    assert evidence_share(m, (0, 0, 0, 1)) == 0.5
    assert evidence_share(m, (0, 0, 2, 1)) == 1.0
    assert evidence_share(m, (1, 0, 1, 0)) == 0.0
    assert evidence_share(m, (-1, -1, -1, -1)) == 0.0
    assert np.isnan(evidence_share(-np.ones((2, 2)), (0, 0, 1, 1)))
    with pytest.raises(ValueError):
        evidence_share(np.zeros(4), (0, 0, 0, 0))


# ---- fav_map_tap_info: the planner alone, no device -----------------------------------------------------------------------
def tap_info(lib, arch, **kw):
    from failure_aware_vision_amd import _lib
    cfg = _lib.FavConfig()
    lib.fav_default_config(C.byref(cfg), arch)
    for k, v in kw.items():
        setattr(cfg, k, v)
    nbytes, s, hf, wf, c = C.c_size_t(), C.c_int32(), C.c_int32(), C.c_int32(), C.c_int32()
    err = C.create_string_buffer(256)
    st = lib.fav_map_tap_info(C.byref(cfg), C.byref(nbytes), C.byref(s), C.byref(hf), C.byref(wf), C.byref(c), err, len(err))
    return st, (nbytes.value, s.value, hf.value, wf.value, c.value), err.value.decode()


def test_map_tap_info_needs_no_device(lib):
    from failure_aware_vision_amd import _lib, weights
    r50, r18 = _lib.ARCH_RESNET50, _lib.ARCH_RESNET18_CIFAR
    mc = dict(n_samples=30, dropout_p=0.1, max_batch=256)
    # the headline config: every sample has its own maps
    st, dims, _ = tap_info(lib, r50, site_mask=weights.site_mask_for(r50, "all_blocks"), **mc)
    assert st == 0 and dims == (30 * 256 * 49 * 2048 * 2, 30, 7, 7, 2048)
    assert dims[0] == 1_541_406_720
    # the pooled-feature site alone: the pool runs once a frame, the map is the same for every sample
    st, dims, _ = tap_info(lib, r50, site_mask=weights.site_mask_for(r50, "last_layer"), **mc)
    assert st == 0 and dims == (256 * 49 * 2048 * 2, 1, 7, 7, 2048)
    # a single pass (51 MB), and a site mask with no dropout probability
    st, dims, _ = tap_info(lib, r50, max_batch=256)
    assert st == 0 and dims == (51_380_224, 1, 7, 7, 2048)
    st, dims, _ = tap_info(lib, r50, site_mask=weights.site_mask_for(r50, "all_blocks"), n_samples=30, dropout_p=0.0, max_batch=256)
    assert st == 0 and dims[1] == 1
    # block sites and the pooled-feature site together: the maps are still one a sample
    st, dims, _ = tap_info(lib, r50, site_mask=weights.site_mask_for(r50, "layer4+fc"), **mc)
    assert st == 0 and dims[1:] == (30, 7, 7, 2048)
    # ResNet-18 CIFAR at 32 x 32, other frame sizes
    st, dims, _ = tap_info(lib, r18, max_batch=8)
    assert st == 0 and dims == (8 * 16 * 512 * 2, 1, 4, 4, 512)
    st, dims, _ = tap_info(lib, r18, max_batch=8, n_samples=3, dropout_p=0.1, site_mask=weights.site_mask_for(r18, "all_blocks"))
    assert st == 0 and dims == (3 * 8 * 16 * 512 * 2, 3, 4, 4, 512)
    st, dims, _ = tap_info(lib, r50, max_batch=3, in_h=64, in_w=64)
    assert st == 0 and dims == (3 * 4 * 2048 * 2, 1, 2, 2, 2048)
    st, dims, _ = tap_info(lib, r50, max_batch=1, in_h=240, in_w=320)
    assert st == 0 and dims[2:] == (8, 10, 2048)
    # size pointers may be NULL
    cfg = _lib.FavConfig()
    lib.fav_default_config(C.byref(cfg), r50)
    assert lib.fav_map_tap_info(C.byref(cfg), None, None, None, None, None, None, 0) == 0


def test_map_tap_info_refusals(lib):
    from failure_aware_vision_amd import _lib
    for arch in (_lib.ARCH_VIT_B16, _lib.ARCH_VIT_TINY):
        st, _, msg = tap_info(lib, arch)
        assert st == 6 and "fav_map_tap_info" in msg and "ViT" in msg, msg
    st, _, msg = tap_info(lib, _lib.ARCH_RESNET50, n_members=5)
    assert st == 6 and "fav_map_tap_info" in msg and "ensemble" in msg, msg
    st, _, msg = tap_info(lib, _lib.ARCH_RESNET50, struct_size=8)
    assert st == 1 and "struct_size" in msg
    st, _, msg = tap_info(lib, _lib.ARCH_RESNET50, max_batch=0)
    assert st == 1 and "fav_map_tap_info" in msg
    st, _, msg = tap_info(lib, _lib.ARCH_RESNET50, site_mask=1 << 20, dropout_p=0.1, n_samples=2)
    assert st == 1 and "site_mask" in msg, msg
    assert lib.fav_map_tap_info(None, None, None, None, None, None, None, 0) == 1


def test_documents_state_the_measured_cost():
    """DESIGN.md item 5i sets the measured overhead beside the derived one, from the profile the tool wrote."""
    design = open(os.path.join(ROOT, "DESIGN.md")).read()
    item = design[design.index("5i. Class activation maps"):design.index("6. ViT: bf16 at every tensor boundary")]
    assert "PLACEHOLDER" not in design and "TODO" not in item
    assert "about 1.2 ms" in item and "profiles/cam_bench.txt" in item and "profiles/cam_tapoff_ab.txt" in item
    profile = open(os.path.join(ROOT, "profiles", "cam_bench.txt")).read()
    rows = {line[:32].strip(): line[32:].split() for line in profile.splitlines() if line.startswith(("classify_", "cam,"))}
    assert set(rows) == {"classify_detect, tap off", "classify_detect, tap on", "classify_cam", "classify_cam, heatmap",
                         "cam, K = 1 (the head alone)", "cam, K = 5 (the head alone)"}
    for name in ("classify_detect, tap off", "classify_detect, tap on", "classify_cam"):
        assert rows[name][0] in item, name        # the medians of the record are the figures of the document
    assert "gfx950" in profile
    assert os.path.exists(os.path.join(ROOT, "profiles", "cam_tapoff_ab.txt"))
