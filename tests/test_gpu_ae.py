"""The autoencoder sensor on the device: fav_op_ae_decode_compare and fav_ae_score against tests/ae_ref.py, and ``Autoencoder``
end to end.

Every comparison is an equality of bits.  The contract fixes the accumulator (the production MFMA chain), the bias addition,
the exponential, the division and the rounding to a byte; behind the byte everything is an integer sum, whose order is free.

Shapes of the op.  The hidden matrix has 1, 15, 16 and 17 rows (one row: a 1 x 1 frame at one level) and multiples beside
them; m = 0, 1, 2 decode steps in front; frames of 33 x 47, 63 x 65 and 9 x 8, no multiple of 2^L or of the cell, so the last
cells are part-full and level-1 pixels hang over the frame; cells of 8 (one tile, one wave), 16 (four tiles, four waves) and
32 (sixteen tiles, four a wave); a grid of exactly 1024 cells; 1 and 3 frames; u8 frames, and fp32 frames with NaN, values
above 1 and negative pixels; a threshold that splits the cells and the default +inf; the optional outputs present and NULL.
Every output lies between guard bytes."""
import ctypes as C

import numpy as np
import pytest

pytestmark = pytest.mark.gpu

torch = pytest.importorskip("torch")
import ae_ref as R  # noqa: E402
from failure_aware_vision_amd import Autoencoder, _lib, autoencoder as A, synth, unpack_ae_records  # noqa: E402

GUARD = 64
FILL = 0x5A


@pytest.fixture(scope="module")
def lib():
    assert torch.cuda.is_available(), "GPU tests need a MI355X"
    return _lib.load()


def dev(a):
    return torch.from_numpy(np.ascontiguousarray(a)).cuda()


class Guarded:
    """nbytes of device memory between two guards of FILL bytes, ``off`` bytes further in."""

    def __init__(self, nbytes, off=0):
        self.n, self.lo = nbytes, GUARD + off
        self.buf = torch.full((GUARD + 16 + nbytes + GUARD,), FILL, dtype=torch.uint8, device="cuda")
        assert self.buf.data_ptr() % 16 == 0

    @property
    def ptr(self):
        return self.buf.data_ptr() + self.lo

    def read(self, dtype):
        host = self.buf.cpu().numpy()
        ok = bool((host[:self.lo] == FILL).all() and (host[self.lo + self.n:] == FILL).all())
        return host[self.lo:self.lo + self.n].copy().view(dtype), ok


def bf16_values(x):
    return A._bf16_to_f32(A._bf16_bits(x)).reshape(np.shape(x))


def make_case(seed, n, hL, wL, m, H, W, layout):
    rng = np.random.default_rng(seed)
    rows = n * hL * wL * 4 ** m
    hidden = bf16_values(np.maximum(rng.standard_normal((rows, 64)), -0.25).astype(np.float32))
    wg = bf16_values((rng.standard_normal((12, 64)) * np.sqrt(2.0 / 64)).astype(np.float32))
    bias = rng.uniform(-0.3, 0.3, 3).astype(np.float32)
    if layout == 0:
        frames = rng.integers(0, 256, (n, H, W, 3), dtype=np.uint8)
    else:
        frames = rng.uniform(-0.2, 1.2, (n, H, W, 3)).astype(np.float32)
        flat = frames.reshape(-1)
        flat[::7] = np.nan
        flat[3::11] = 70.0
        flat[5::13] = -np.inf
    return hidden, wg, bias, frames


def run_op(lib, hidden, n, hL, wL, m, wg, bias, frames, cell, thr, want_recon=True, want_sse=True, null=(), off=None):
    """-> (status, dict of cell_sse / err_map / rec / recon as written, every guard untouched?)"""
    off = off or {}
    H, W = frames.shape[1:3]
    cells = -(-H // cell) * -(-W // cell)
    layout = 0 if frames.dtype == np.uint8 else 1
    hd, wd, bd, fd = dev(A._bf16_bits(hidden).view(np.int16)), dev(A._bf16_bits(wg).view(np.int16)), dev(bias), dev(frames)
    out = dict(err_map=Guarded(4 * n * cells, off.get("err_map", 0)), rec=Guarded(32 * n, off.get("rec", 0)),
               recon=Guarded(n * H * W * 3), cell_sse=Guarded(4 * n * cells, off.get("cell_sse", 0)))
    ptr = dict(hidden=hd.data_ptr() + off.get("hidden", 0), wg=wd.data_ptr(), bias=bd.data_ptr(), frames=fd.data_ptr() + off.get("frames", 0),
               err_map=out["err_map"].ptr, rec=out["rec"].ptr, recon=out["recon"].ptr if want_recon else None,
               cell_sse=out["cell_sse"].ptr if want_sse else None)
    for name in null:
        ptr[name] = None
    st = lib.fav_op_ae_decode_compare(ptr["hidden"], n, hL, wL, m, ptr["wg"], ptr["bias"], ptr["frames"], layout, H, W, cell, thr,
                                      ptr["cell_sse"], ptr["err_map"], ptr["rec"], ptr["recon"], torch.cuda.current_stream().cuda_stream)
    torch.cuda.synchronize()
    got, ok = {}, True
    for name, dt in (("err_map", np.uint32), ("rec", np.int32), ("recon", np.uint8), ("cell_sse", np.uint32)):
        got[name], g = out[name].read(dt)
        ok = ok and g
    return st, got, ok


def untouched(a):
    return bool((a.view(np.uint8) == FILL).all())


def check_against(got, want, n, want_recon=True, want_sse=True):
    assert np.array_equal(got["err_map"], want["err_map"].reshape(-1).view(np.uint32)), "err_map"
    assert np.array_equal(got["rec"].reshape(n, 8), R.records(want)), (got["rec"].reshape(n, 8), R.records(want))
    if want_recon:
        assert np.array_equal(got["recon"], want["recon"].reshape(-1)), "recon"
    else:
        assert untouched(got["recon"])
    if want_sse:
        assert np.array_equal(got["cell_sse"], want["cell_sse"].reshape(-1)), "cell_sse"
    else:
        assert untouched(got["cell_sse"])


# (n, hL, wL, m, H, W, cell, layout): rows = n hL wL 4^m
OP_CASES = [
    (1, 1, 1, 0, 1, 1, 8, 0),           # one row: L = 1 on a 1 x 1 frame
    (1, 3, 5, 0, 6, 9, 8, 0),           # 15 rows
    (1, 4, 4, 0, 8, 8, 8, 1),           # 16 rows, one full cell
    (1, 17, 1, 0, 33, 2, 16, 0),        # 17 rows
    (3, 17, 24, 0, 33, 47, 8, 0),       # 33 x 47 at every m and cell
    (1, 9, 12, 1, 33, 47, 16, 1),
    (3, 5, 6, 2, 33, 47, 32, 0),
    (1, 32, 33, 0, 63, 65, 32, 1),      # 63 x 65
    (3, 16, 17, 1, 63, 65, 8, 0),
    (1, 8, 9, 2, 63, 65, 16, 0),
    (3, 5, 4, 0, 9, 8, 8, 1),           # 9 x 8
    (1, 3, 2, 1, 9, 8, 16, 0),
    (1, 2, 1, 2, 9, 8, 32, 0),
    (1, 63, 64, 1, 249, 255, 8, 0),     # exactly 32 x 32 = 1024 cells
]


@pytest.mark.parametrize("case", OP_CASES, ids=["-".join(str(v) for v in c) for c in OP_CASES])
def test_op_bit_exact(lib, case):
    n, hL, wL, m, H, W, cell, layout = case
    hidden, wg, bias, frames = make_case(100 + OP_CASES.index(case), n, hL, wL, m, H, W, layout)
    base = R.decode_compare(hidden, n, hL, wL, m, wg, bias, frames, cell)
    assert len(np.unique(base["recon"])) > min(20, base["recon"].size // 4), "the bytes must have something to compare"
    # the default +inf: no cell is above; everything optional present
    st, got, guards = run_op(lib, hidden, n, hL, wL, m, wg, bias, frames, cell, float("inf"))
    assert st == 0 and guards
    check_against(got, base, n)
    assert (R.records(base)[:, 6] == 0).all() and (R.records(base)[:, 7] == -1).all()
    # a threshold that splits the cells; the optional outputs NULL
    thr = float(np.median(base["err_map"]))
    want = R.decode_compare(hidden, n, hL, wL, m, wg, bias, frames, cell, thr)
    if base["err_map"].size > 1:
        assert 0 < want["n_above"].sum() < base["err_map"].size
    st, got, guards = run_op(lib, hidden, n, hL, wL, m, wg, bias, frames, cell, thr, want_recon=False, want_sse=False)
    assert st == 0 and guards
    check_against(got, want, n, want_recon=False, want_sse=False)


def test_op_fp32_pixels_are_sanitised_and_clamped(lib):
    """NaN -> 0, above 1 -> 255, negative -> 0: the reference's bytes say so and the device agrees."""
    hidden, wg, bias, frames = make_case(5, 1, 4, 4, 0, 8, 8, 1)
    frames[0, 0, 0] = (np.nan, 2.0, -3.0)
    assert np.array_equal(R.frame_bytes(frames)[0, 0, 0], (0, 255, 0))
    want = R.decode_compare(hidden, 1, 4, 4, 0, wg, bias, frames, 8)
    st, got, guards = run_op(lib, hidden, 1, 4, 4, 0, wg, bias, frames, 8, float("inf"))
    assert st == 0 and guards
    check_against(got, want, 1)


def test_op_refusals_launch_nothing(lib):
    hidden, wg, bias, frames = make_case(6, 1, 4, 4, 0, 8, 8, 1)
    args = (hidden, 1, 4, 4, 0, wg, bias, frames)

    def refused(word, *a, **kw):
        st, got, guards = run_op(lib, *a, **kw)
        msg = lib.fav_last_error(None).decode()
        assert st == _lib.FAV_ERR_INVALID_ARG and guards and all(untouched(v) for v in got.values()), msg
        assert msg.startswith("fav_op_ae_decode_compare: ") and word in msg, msg
    for name in ("hidden", "wg", "bias", "frames", "err_map", "rec"):
        refused("null pointer", *args, 8, 1.0, null=(name,))
    refused("cell=12", *args, 12, 1.0)
    refused("threshold is NaN", *args, 8, float("nan"))
    refused("m=3", hidden, 1, 4, 4, 3, wg, bias, frames, 8, 1.0)
    refused("smaller than the frame", hidden, 1, 3, 4, 0, wg, bias, frames, 8, 1.0)
    refused("n must be", hidden, 0, 4, 4, 0, wg, bias, frames, 8, 1.0)
    refused("16-byte aligned", *args, 8, 1.0, off=dict(hidden=8))
    refused("4-byte aligned", *args, 8, 1.0, off=dict(err_map=2))
    refused("4-byte aligned", *args, 8, 1.0, off=dict(cell_sse=1))
    refused("4-byte aligned", *args, 8, 1.0, off=dict(frames=2))
    refused("8-byte aligned", *args, 8, 1.0, off=dict(rec=4))
    st, got, guards = run_op(lib, *args, 8, float("inf"))            # and the op is as usable as before
    assert st == 0 and guards
    check_against(got, R.decode_compare(hidden, 1, 4, 4, 0, wg, bias, frames, 8), 1)


# ---- the handle, end to end ------------------------------------------------------------------------------------------
def ref_for(blob, frames, cell, thr=np.inf):
    levels, layers = A.parse_blob(blob)
    return R.forward(layers, levels, frames, cell, thr)


def same_as_ref(out, want):
    for k in ("mse", "peak", "floor", "err_map"):
        assert np.array_equal(np.asarray(out[k]).view(np.uint32), want[k].astype(np.float32).view(np.uint32)), k
    for k in ("sse", "peak_cell", "n_above", "box"):
        assert np.array_equal(np.asarray(out[k]), want[k]), k
    assert np.array_equal(out["recon"], want["recon"]), "recon"


E2E = [(L, hw, nb) for L in (1, 2, 3) for hw, nb in (((8, 8), 3), ((33, 47), 3), ((240, 320), 1))]


@pytest.mark.parametrize("levels,hw,max_batch", E2E, ids=[f"L{L}-{hw[0]}x{hw[1]}" for L, hw, _ in E2E])
def test_score_bit_exact(lib, levels, hw, max_batch):
    blob = A.make_synthetic_ae(levels, seed=levels)
    frames = synth.synthetic_frames_u8(max_batch, hw[0], hw[1], seed=17)
    cell = 8 if hw[0] < 64 else 16
    ae = Autoencoder(blob, in_hw=hw, levels=levels, cell=cell, max_batch=max_batch)
    try:
        want = ref_for(blob, frames, cell)
        assert len(np.unique(want["recon"])) > 20
        out = ae.score(frames, recon=True)                              # n = max_batch
        same_as_ref(out, want)
        again = ae.score(frames, recon=True)                            # a second call on the handle: equal bits
        for k in out:
            assert np.array_equal(np.asarray(out[k]), np.asarray(again[k])), k
        if max_batch > 1:                                               # n = 1, fp32 pixels, a threshold that splits the cells
            f32 = (frames[1:2].astype(np.float32) / np.float32(255.0)).astype(np.float32)
            thr = float(np.median(ref_for(blob, f32, cell)["err_map"]))
            ae.set_threshold(thr)
            same_as_ref(ae.score(f32, recon=True), ref_for(blob, f32, cell, thr))
    finally:
        ae.close()


def test_score_refusals_leave_the_handle_usable(lib):
    blob = A.make_synthetic_ae(2, seed=2)
    frames = synth.synthetic_frames_u8(2, 33, 47, seed=3)
    ae = Autoencoder(blob, in_hw=(33, 47), levels=2, cell=16, max_batch=2)
    try:
        want = ref_for(blob, frames, 16)
        fd = dev(frames)
        gh, gw = ae.grid
        err_map, rec = Guarded(4 * 2 * gh * gw), Guarded(64)
        stream = torch.cuda.current_stream().cuda_stream

        def call(images=fd.data_ptr(), n=2, layout=0, em=err_map.ptr, rc=rec.ptr):
            st = lib.fav_ae_score(ae._h, images, n, layout, em, rc, None, stream)
            torch.cuda.synchronize()
            return st, lib.fav_last_error(None).decode()
        for kw, word in ((dict(n=3), "n=3 outside [1, max_batch=2]"), (dict(n=0), "n=0"), (dict(images=None), "null pointer"),
                         (dict(em=None), "null pointer"), (dict(rc=None), "null pointer"), (dict(layout=2), "unknown layout"),
                         (dict(em=err_map.ptr + 2), "err_map_dev must be 4-byte aligned"), (dict(rc=rec.ptr + 4), "rec_dev must be 8-byte aligned"),
                         (dict(images=fd.data_ptr() + 1, layout=1), "fp32 frames must be 4-byte aligned")):
            st, msg = call(**kw)
            assert st == _lib.FAV_ERR_INVALID_ARG and msg.startswith("fav_ae_score: ") and word in msg, (kw, msg)
            assert untouched(err_map.read(np.uint8)[0]) and untouched(rec.read(np.uint8)[0]), kw
        # a blob of another level count, a truncated one: refused, and the weights in force stay
        for bad in (A.make_synthetic_ae(1, seed=2), blob[:-64]):
            with pytest.raises(_lib.FavError) as ei:
                ae.load(bad)
            assert ei.value.status == 2 and "fav_ae_load_weights" in str(ei.value)
        with pytest.raises(_lib.FavError, match="NaN"):
            ae.set_threshold(float("nan"))
        st, _ = call()
        assert st == 0
        em, g1 = err_map.read(np.uint32)
        rc, g2 = rec.read(np.int32)
        assert g1 and g2
        assert np.array_equal(em, want["err_map"].reshape(-1).view(np.uint32)) and np.array_equal(rc.reshape(2, 8), R.records(want))
    finally:
        ae.close()


def test_score_chunks_like_one_call(lib):
    blob = A.make_synthetic_ae(1, seed=5)
    frames = synth.synthetic_frames_u8(5, 9, 8, seed=5)
    whole, parts = Autoencoder(blob, in_hw=(9, 8), levels=1, cell=8, max_batch=5), Autoencoder(blob, in_hw=(9, 8), levels=1, cell=8, max_batch=2)
    try:
        a, b = whole.score(frames, recon=True), parts.score(dev(frames), recon=True)
        assert set(a) == set(b)
        for k in a:
            assert np.array_equal(np.asarray(a[k]), b[k].cpu().numpy()), k
        same_as_ref(a, ref_for(blob, frames, 8))
        rec = np.zeros((5, 8), np.int32)
        assert unpack_ae_records(rec)["sse"].dtype == np.int64
    finally:
        whole.close()
        parts.close()


def test_calibrate_and_analyze_frame_on_a_real_frame(lib):
    blob = A.make_synthetic_ae(2, seed=1)
    frames = synth.synthetic_frames_u8(4, 64, 96, seed=9)
    ae = Autoencoder(blob, in_hw=(64, 96), levels=2, cell=16, max_batch=4)
    try:
        want = ref_for(blob, frames, 16)
        thr = ae.calibrate(frames, tpr=0.75)
        assert thr == float(np.nextafter(np.sort(want["peak"])[2], np.float32(np.inf)))
        assert np.array_equal(ae.score(frames)["anomalous"], want["peak"] >= np.float32(thr))
        res = ae.analyze_frame(frames[0])
        assert set(res) == {"anomaly_score", "vision_status", "metrics"} and isinstance(res["vision_status"], str)
        assert res["anomaly_score"] == round(min(float(want["mse"][0]), 1.0), 6)
        assert res["metrics"]["autoencoder"] == {"mse": float(want["mse"][0]), "peak": float(want["peak"][0]), "peak_cell": int(want["peak_cell"][0])}
        assert {"blur", "brightness", "freeze", "entropy", "raw", "rule_anomaly_score"} <= set(res["metrics"])
        res2 = ae.analyze_frame(frames[1], status_provider=lambda f: "VISION_OK")
        assert res2["vision_status"] == "VISION_OK" and res2["anomaly_score"] == round(min(float(want["mse"][1]), 1.0), 6)
        with pytest.raises(ValueError):
            ae.analyze_frame(frames[0, :32])
    finally:
        ae.close()
