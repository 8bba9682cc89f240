"""The autoencoder sensor without a GPU: the geometry, the row order, the config and blob checks, the numpy reference against
the fp32 torch module, and the sensor doing its job after training - through the reference, so with every bf16 rounding point
and the integer error of the device path.

The measured tolerance.  ``MSE_GAP_BOUND`` bounds |reference mse - fp32 torch mse| per frame.  It is twice the largest gap
measured over this file's frames (synthetic and trained weights, levels 1 to 3) on the CPU the feature was written on; the
factor allows for other BLAS builds and thread counts in the fp32 model.  The gap is the bf16 rounding of weights and
activations and the rounding of the reconstruction to bytes; the run prints it (conftest.note)."""
import ctypes as C
import struct

import numpy as np
import pytest

torch = pytest.importorskip("torch")
import ae_ref as R  # noqa: E402
from conftest import note  # noqa: E402
from failure_aware_vision_amd import _lib, autoencoder as A, synth  # noqa: E402

#: twice the largest per-frame gap measured: 1.055e-4 (synthetic weights, 2 levels, MSEs of 0.061 to 0.144); the others were
#: 9.9e-5 (1 level), 5.7e-5 (3 levels) and 2.5e-5 on the trained weights at MSEs of 0.00096 to 0.0111
MSE_GAP_BOUND = 2.11e-4

SIZES = [(1, 1), (8, 8), (33, 47), (63, 65), (224, 224), (240, 320)]


def torch_mse(sd, levels, frames):
    """The fp32 module's reconstruction error per frame, pixels in [0, 1]."""
    net = A.torch_module(levels)
    net.load_state_dict({k: torch.as_tensor(np.asarray(v)) for k, v in sd.items()})
    x = torch.from_numpy(frames).permute(0, 3, 1, 2).float() / 255.0
    with torch.no_grad():
        rc = net(x)
    return ((rc - x) ** 2).mean(dim=(1, 2, 3)).numpy().astype(np.float64), rc.permute(0, 2, 3, 1).numpy()


# ---- geometry ---------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("levels", [1, 2, 3])
@pytest.mark.parametrize("hw", SIZES, ids=[f"{h}x{w}" for h, w in SIZES])
def test_geometry_is_the_torch_modules(hw, levels):
    H, W = hw
    cell = 8 if max(H, W) < 64 else 16
    g = A.geometry(hw, levels, cell, 2)
    net = A.torch_module(levels)
    x = torch.zeros(1, 3, H, W)
    hs, ws = [H], [W]
    with torch.no_grad():
        for e in net.enc:
            x = e(x)
            hs.append(x.shape[2])
            ws.append(x.shape[3])
        for d in net.dec:
            x = d(x)
    assert g["h"] == hs and g["w"] == ws == R.grid_sizes(H, W, levels)[1]
    assert tuple(x.shape[2:]) == (hs[-1] << levels, ws[-1] << levels) and x.shape[2] >= H and x.shape[3] >= W
    assert (g["gh"], g["gw"]) == (-(-H // cell), -(-W // cell))
    # two rotating buffers that hold the largest activation matrix of 2 frames
    rows = 2 * hs[-1] * ws[-1] * 4 ** (levels - 1)
    assert g["workspace_bytes"] >= 2 * max(rows * 128, 2 * hs[1] * ws[1] * 128) and g["workspace_bytes"] % 256 == 0


def test_row_order_is_a_pixel_shuffle():
    """An index tensor through m explicit pixel shuffles against the formula, and the reference's two views of one network."""
    for m, hL, wL, n in ((0, 3, 2, 2), (1, 3, 2, 2), (2, 2, 3, 1), (2, 1, 1, 3)):
        rows = n * hL * wL * 4 ** m
        ids = np.arange(rows, dtype=np.int64)
        # undo the flat reshape a step at a time: [n, h, w, 4 c] holds (2a + b) c + rest
        grid = ids.reshape(n, hL, wL, 4 ** m)
        for j in range(m):
            grid = R.pixel_shuffle(grid, 4 ** (m - j - 1))
        spatial = grid[..., 0]
        i, y, x = R.row_to_pixel(ids, hL, wL, m)
        assert np.array_equal(spatial[i, y, x], ids)
        assert sorted(zip(i.tolist(), y.tolist(), x.tolist())) == [(a, b, c) for a in range(n) for b in range(hL << m) for c in range(wL << m)]
    for levels in (2, 3):
        _, layers = A.parse_blob(A.make_synthetic_ae(levels, 3))
        out = R.forward(layers, levels, synth.synthetic_frames_u8(2, 9, 8, seed=1), cell=8)
        i, y, x = R.row_to_pixel(np.arange(out["hidden"].shape[0]), out["h"][levels], out["w"][levels], levels - 1)
        assert np.array_equal(out["hidden"], out["hidden_spatial"][i, y, x])


# ---- the checks -------------------------------------------------------------------------------------------------------
def test_config_refusals_name_the_field():
    lib = _lib.load()

    def why(**kw):
        c = dict(in_h=240, in_w=320, levels=2, max_batch=4, cell=16)
        c.update(kw)
        cfg = _lib.FavAeConfig(kw.get("struct_size", C.sizeof(_lib.FavAeConfig)), c["in_h"], c["in_w"], c["levels"], c["max_batch"], c["cell"])
        err = C.create_string_buffer(256)
        st = lib.fav_check_ae_config(C.byref(cfg), err, len(err))
        err2 = C.create_string_buffer(256)
        st2 = lib.fav_ae_info(C.byref(cfg), None, None, None, None, None, err2, len(err2))
        assert (st == 0) == (err.value == b"") and (st2 != 0 or st == 0)
        return st, err.value.decode()
    assert why() == (0, "")
    for kw, word in ((dict(in_h=0), "in_h=0"), (dict(in_h=4097), "in_h=4097"), (dict(in_w=0), "in_w=0"), (dict(in_w=5000), "in_w=5000"),
                     (dict(levels=0), "levels=0"), (dict(levels=4), "levels=4"), (dict(max_batch=0), "max_batch=0"),
                     (dict(cell=12), "cell=12"), (dict(cell=8, in_h=264, in_w=264), "cell=8 gives a grid of 33 x 33"),
                     (dict(cell=8, in_h=8, in_w=2056), "cell=8 gives a grid of 1 x 257"), (dict(struct_size=20), "struct_size")):
        st, msg = why(**kw)
        assert st == _lib.FAV_ERR_INVALID_ARG and word in msg, (kw, msg)
    assert why(cell=8, in_h=256, in_w=256) == (0, "")                  # exactly 1024 cells
    with pytest.raises(_lib.FavError, match=r"workspace of \d+ bytes, above 1073741824"):
        A.geometry((224, 224), 3, 16, 2560)
    assert A.geometry((224, 224), 2, 16, 256)["workspace_bytes"] <= 1 << 30


def test_blob_round_trip_and_refusals():
    for levels in (1, 2, 3):
        sd = A.make_synthetic_state_dict(levels, seed=7)
        blob = A.blob_from_state_dict({k: torch.from_numpy(v) for k, v in sd.items()}, levels)
        assert blob == A.make_synthetic_ae(levels, seed=7) and A.check_blob(blob) == ""
        lv, layers = A.parse_blob(blob)
        assert lv == levels and [(w.shape, b.shape[0]) for w, b in layers] == A.layer_shapes(levels)
        w1 = sd["enc.0.weight"]
        assert np.array_equal(layers[0][0][:, :27].reshape(64, 3, 3, 3), w1.transpose(0, 2, 3, 1)) and not layers[0][0][:, 27:].any()
        for l in range(2, levels + 1):
            assert np.array_equal(layers[l - 1][0], sd[f"enc.{l - 1}.weight"].transpose(0, 2, 3, 1))
        for j, l in enumerate(range(levels, 0, -1)):
            wt, (wg, bg) = sd[f"dec.{j}.weight"], layers[levels + j]
            co = wt.shape[1]
            for a in range(2):
                for b in range(2):
                    assert np.array_equal(wg[(2 * a + b) * co:(2 * a + b + 1) * co], wt[:, :, a, b].T)
            assert np.array_equal(bg, sd[f"dec.{j}.bias"] if l == 1 else np.tile(sd[f"dec.{j}.bias"], 4))
    blob = A.make_synthetic_ae(2, seed=7)
    w_off, b_off = struct.unpack_from("<2Q", blob, 64 + 16)

    def patched(at, fmt, *v):
        b = bytearray(blob)
        struct.pack_into(fmt, b, at, *v)
        return bytes(b)
    for bad, word in ((blob[:32], "too small"), (blob[:-1], "truncated"), (blob + b"\0", "truncated"), (patched(0, "<I", 0x57564146), "not a FAVA"),
                      (patched(4, "<I", 2), "not a FAVA"), (patched(8, "<I", 4), "levels=4"), (patched(8, "<I", 3), "layers=4"),
                      (patched(12, "<I", 5), "layers=5"), (patched(64 + 16, "<Q", w_off + 2), "layer 1: weight offset"),
                      (patched(64 + 24, "<Q", b_off + 32), "layer 1: bias offset"), (patched(64 + 16, "<Q", len(blob)), "layer 1: weight data out of range"),
                      (patched(64 + 8, "<Q", 64), "layer 0: bias data out of range"), (patched(w_off + 10, "<H", 0x7F80), "layer 1 holds a non-finite weight"),
                      (patched(w_off, "<H", 0xFFC0), "layer 1 holds a non-finite weight"), (patched(b_off + 4, "<f", float("nan")), "layer 1 holds a non-finite bias"),
                      (patched(b_off, "<f", float("inf")), "layer 1 holds a non-finite bias")):
        assert word in A.check_blob(bad), (word, A.check_blob(bad))
    err = C.create_string_buffer(64)
    assert _lib.load().fav_ae_check_blob(blob[:-1], len(blob) - 1, err, len(err)) == 2      # FAV_ERR_BAD_BLOB


# ---- the reference against the fp32 module ---------------------------------------------------------------------------
@pytest.fixture(scope="module")
def trained():
    """192 normal 32 x 32 frames, 300 steps of Adam on the CPU -> (state dict, parsed layers, the 64 held-out frames)."""
    train = synth.synthetic_frames_u8(192, 32, 32, seed=21)
    held = synth.synthetic_frames_u8(64, 32, 32, seed=21, start_id=192)
    sd = A.train_state_dict(train, levels=2, steps=300, lr=1e-3, seed=0, batch=32, device="cpu")
    _, layers = A.parse_blob(A.blob_from_state_dict(sd, 2))
    return sd, layers, held


def test_reference_against_the_fp32_module(trained):
    gaps = {}
    for levels in (1, 2, 3):
        sd = A.make_synthetic_state_dict(levels, seed=levels)
        frames = synth.synthetic_frames_u8(4, 33, 47, seed=levels)
        _, layers = A.parse_blob(A.blob_from_state_dict(sd, levels))
        out = R.forward(layers, levels, frames, cell=8)
        mse_t, rc = torch_mse(sd, levels, frames)
        assert np.abs(out["recon"].astype(np.float64) / 255.0 - rc).max() < 0.03           # the same picture, byte for byte nearly
        gaps[f"synthetic L{levels}"] = (float(np.abs(out["mse"].astype(np.float64) - mse_t).max()), float(mse_t.min()), float(mse_t.max()))
    sd, layers, held = trained
    out = R.forward(layers, 2, held, cell=8)
    mse_t, _ = torch_mse(sd, 2, held)
    gaps["trained L2"] = (float(np.abs(out["mse"].astype(np.float64) - mse_t).max()), float(mse_t.min()), float(mse_t.max()))
    for name, (gap, lo, hi) in gaps.items():
        note(f"test_ae_host: {name}: largest |reference mse - fp32 torch mse| = {gap:.3e} on MSEs of {lo:.3e} to {hi:.3e} (bound {MSE_GAP_BOUND:.1e})")
    assert max(g for g, _, _ in gaps.values()) <= MSE_GAP_BOUND, gaps


def test_the_sensor_does_its_job_after_training(trained):
    """Through the reference: every held-out normal frame scores below every noisy one, and a planted white block is where the
    error map peaks."""
    _, layers, held = trained
    normal = R.forward(layers, 2, held, cell=8)
    noisy = R.forward(layers, 2, synth.gaussian_noise_f32(held, 3, seed=5), cell=8)
    rng = np.random.default_rng(8)
    planted, where = held.copy(), []
    for i in range(held.shape[0]):
        cy, cx = int(rng.integers(0, 4)), int(rng.integers(0, 4))
        planted[i, 8 * cy:8 * cy + 8, 8 * cx:8 * cx + 8] = 255
        where.append(4 * cy + cx)
    hits = int((R.forward(layers, 2, planted, cell=8)["peak_cell"] == np.array(where)).sum())
    note(f"test_ae_host: held-out mse max {normal['mse'].max():.4f}, gaussian_noise severity 3 mse min {noisy['mse'].min():.4f}; "
         f"planted 8 x 8 block found in {hits} of {held.shape[0]} frames")
    assert normal["mse"].max() < noisy["mse"].min()
    assert hits >= 0.9 * held.shape[0]


# ---- the seam ---------------------------------------------------------------------------------------------------------
def test_analyze_frame_shape_and_rounding_on_a_stub():
    ae = A.Autoencoder.__new__(A.Autoencoder)
    ae.in_hw, ae._rules, ae._h = (4, 6), None, None
    rule = {"vision_status": "VISION_DEGRADED", "anomaly_score": 0.25,
            "metrics": {"blur": 0.1, "brightness": 0.2, "freeze": 0.0, "entropy": 0.3, "raw": {"laplacian_var": 1.0}}}
    seen = []

    def score_one(fr, use_rules):
        seen.append((fr.shape, fr.flags["C_CONTIGUOUS"], use_rules))
        return 0.0123456789, 0.5, 3, rule if use_rules else None
    ae._score_one = score_one
    frame = np.zeros((4, 6, 3), np.uint8)
    res = ae.analyze_frame(frame[:, ::1])
    assert res == {"anomaly_score": 0.012346, "vision_status": "VISION_DEGRADED",
                   "metrics": dict(rule["metrics"], autoencoder={"mse": 0.0123456789, "peak": 0.5, "peak_cell": 3}, rule_anomaly_score=0.25)}
    res = ae.analyze_frame(frame, status_provider=lambda f: "VISION_OK")
    assert res["vision_status"] == "VISION_OK" and res["metrics"]["blur"] == 0.0 and "rule_anomaly_score" not in res["metrics"]
    assert seen == [((4, 6, 3), True, True), ((4, 6, 3), True, False)]
    ae._score_one = lambda fr, use_rules: (7.5, 9.0, 0, None)
    assert ae.analyze_frame(frame, status_provider=lambda f: "VISION_OK")["anomaly_score"] == 1.0      # min(mse, 1)

    def broken(fr, use_rules):
        raise _lib.FavError(4, "the device went away")
    ae._score_one = broken
    res = ae.analyze_frame(frame)
    assert res["anomaly_score"] == 1.0 and res["vision_status"] == A.Autoencoder.FAILED_STATUS and "FavError" in res["metrics"]["error"]
    with pytest.raises(TypeError):
        ae.analyze_frame(frame.astype(np.float32))
    with pytest.raises(ValueError):
        ae.analyze_frame(np.zeros((4, 5, 3), np.uint8))


def test_unpack_ae_records_aliases_the_buffer():
    rec = np.zeros((2, 8), np.int32)
    rec[1] = (np.uint32(0xFFFFFFFE).astype(np.int32), np.float32(0.5).view(np.int32), np.float32(0.75).view(np.int32), 5,
              np.float32(0.125).view(np.int32), 3, 2, 1 | 2 << 8 | 3 << 16 | 4 << 24)
    rec[0, 7] = -1
    u = A.unpack_ae_records(rec)
    assert u["sse"].tolist() == [0, 3 * 2 ** 32 + 0xFFFFFFFE] and u["mse"][1] == 0.5 and u["peak"][1] == 0.75 and u["floor"][1] == 0.125
    assert (u["x0"][1], u["y0"][1], u["x1"][1], u["y1"][1]) == (1, 2, 3, 4) and u["x0"][0] == -1 and u["anomalous"].tolist() == [False, True]
    rec[1, 3] = 9
    assert u["peak_cell"][1] == 9
    t = A.unpack_ae_records(torch.from_numpy(rec))
    assert t["sse"].tolist() == u["sse"].tolist() and float(t["mse"][1]) == 0.5
    with pytest.raises(ValueError):
        A.unpack_ae_records(np.zeros((2, 7), np.int32))
