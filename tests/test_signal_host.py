"""CPU checks of the signal path: the integer reference of the fused statistics pass (tests/signal_ref.py) and the
restated scorer (oracle/signal_oracle.py) pin each other on every edge shape of tests/test_gpu_signal_edges.py, and
signal.score_frame is held to the restated scoring rule by rule (signal_analyzer.py:66-171), on both sides of every
threshold and at it."""
import numpy as np
import pytest

import signal_ref as SR
from failure_aware_vision_amd.signal import score_frame
from oracle import signal_oracle as SO


@pytest.mark.parametrize("shape", SR.EDGE_SHAPES, ids=lambda s: "x".join(map(str, s)))
def test_integer_reference_and_restated_scorer_agree(shape):
    n, H, W = shape
    rng = np.random.default_rng(H * 1000003 + W)
    frames = rng.integers(0, 256, (n, H, W, 3), dtype=np.uint8)
    orc = SO.SignalOracle()
    for i, (fr, ref) in enumerate(zip(frames, SR.stream_stats(frames))):
        lap = SO.laplacian(SO.bgr2gray(fr))                  # float64 holding integers (np.pad borders)
        gray, lap_var, mean, mean_diff, entropy, hist = orc.raw(fr)
        assert np.array_equal(gray, ref["gray"]) and gray.dtype == np.uint8
        assert np.array_equal(hist, ref["hist"])
        assert np.array_equal(lap, SR.laplacian_i64(ref["gray"]).astype(np.float64))
        assert int(lap.sum()) == ref["sum_lap"] and int((lap * lap).sum()) == ref["sum_lap2"]
        assert int(gray.astype(np.int64).sum()) == ref["sum_gray"]
        assert ref["has_prev"] == (1 if i else 0)
        if i:
            assert round(mean_diff * H * W) == ref["sum_absdiff"] and abs(mean_diff - ref["mean_diff"]) <= 1e-12
        else:
            assert mean_diff is None and ref["sum_absdiff"] == 0 and ref["mean_diff"] == 0.0
        assert abs(mean - ref["mean"]) <= 1e-12
        assert abs(lap_var - ref["lap_var"]) <= 1e-12 * lap_var   # one-pass E[x^2] - E[x]^2 against numpy's two-pass .var()
        # The restated scorer works in float32.  Rounding p and log2(p) costs a term at most p * (2 |log2 p| + 1.45) * 2^-24,
        # (2 * 8 + 1.45) * 2^-24 = 1.04e-6 over all bins at the largest entropy 8; numpy's blocked float32 sum of 256 terms
        # adds less than as much again.  Observed: at most 7.5e-7 on these shapes.
        assert abs(entropy - ref["entropy"]) <= 2e-6


def test_reference_on_frames_whose_sums_are_known():
    """The two figures the GPU edge tests lean on, from first principles: a 0/255 checkerboard has |lap| = 1020 on interior
    pixels, and at 300x500 its sum of squares is 36 times 2^32."""
    H, W = 300, 500
    yy, xx = np.mgrid[:H, :W]
    board = np.repeat((((yy + xx) & 1) * 255).astype(np.uint8)[..., None], 3, axis=2)
    a = SR.frame_stats(board)
    assert np.array_equal(a["gray"], board[..., 0])
    lap = SR.laplacian_i64(a["gray"])
    assert np.all(np.abs(lap[1:-1, 1:-1]) == 1020) and np.all(np.abs(lap) == 1020)   # reflect-101 keeps the parity
    assert a["sum_lap2"] == 156_060_000_000 == 1020 * 1020 * H * W and a["sum_lap2"] > 36 * 2 ** 32
    assert a["sum_lap"] == 0 and a["lap_var"] == 1020.0 * 1020.0
    b = SR.frame_stats(255 - board, a["gray"])
    assert b["sum_absdiff"] == 255 * H * W and b["mean_diff"] == 255.0
    assert a["entropy"] == 1.0
    flat = SR.frame_stats(np.full((3, 4, 3), 128, np.uint8))
    assert flat["entropy"] == 0.0 and flat["lap_var"] == 0.0 and flat["hist"][128] == 12
    ramp = np.repeat(np.repeat(np.arange(256, dtype=np.uint8), 4).reshape(16, 64)[..., None], 3, axis=2)
    assert SR.frame_stats(ramp)["entropy"] == 8.0 and np.all(SR.frame_stats(ramp)["hist"] == 4)


def both(lap_var, mean, mean_diff, entropy, frozen):
    """score_frame and the restated scorer on the same raw numbers: equal dicts, equal frozen run."""
    got, run = score_frame(lap_var, mean, mean_diff, entropy, frozen)
    ref, ref_run = SO.score(lap_var, mean, mean_diff, entropy, frozen)
    assert got == ref and run == ref_run, (lap_var, mean, mean_diff, entropy, frozen)
    return got, run


# lap_var, mean, mean_diff, entropy, frozen run before -> status, frozen run after, and the metrics the row is about
RULES = [
    # blank: mean < 15 or mean > 245, strict on both sides
    (600.0, 14.9, 5.0, 5.0, 0, "VISION_BLANK", 0, {"brightness": 0.8836}),
    (600.0, 15.0, 5.0, 5.0, 0, "VISION_OK", 0, {"brightness": 0.8828}),
    (600.0, 245.0, 5.0, 5.0, 0, "VISION_OK", 0, {"brightness": 0.9141}),
    (600.0, 245.1, 5.0, 5.0, 0, "VISION_BLANK", 0, {"brightness": 0.9148}),
    # freeze: mean_diff < 1.0 extends the run, 1.0 itself ends it
    (600.0, 128.0, 0.99, 5.0, 0, "VISION_OK", 1, {"freeze": 0.06}),
    (600.0, 128.0, 1.0, 5.0, 3, "VISION_OK", 0, {"freeze": 0.0}),
    (600.0, 128.0, 0.99, 5.0, 3, "VISION_OK", 4, {"freeze": 0.24}),
    (600.0, 128.0, 0.99, 5.0, 4, "VISION_FROZEN", 5, {"freeze": 1.0}),
    (600.0, 128.0, 0.0, 5.0, 5, "VISION_FROZEN", 6, {"freeze": 1.0}),
    (600.0, 128.0, 1.0, 5.0, 6, "VISION_OK", 0, {"freeze": 0.0}),
    # entropy: status bounds 2.0 and 7.5 (strict), metric ramps below 4.0 and above 7.0
    (600.0, 128.0, 5.0, 1.99, 0, "VISION_CORRUPTED", 0, {"entropy": 0.5025}),
    (600.0, 128.0, 5.0, 2.0, 0, "VISION_OK", 0, {"entropy": 0.5}),
    (600.0, 128.0, 5.0, 3.99, 0, "VISION_OK", 0, {"entropy": 0.0025}),
    (600.0, 128.0, 5.0, 4.0, 0, "VISION_OK", 0, {"entropy": 0.0}),
    (600.0, 128.0, 5.0, 7.0, 0, "VISION_OK", 0, {"entropy": 0.0}),
    (600.0, 128.0, 5.0, 7.01, 0, "VISION_OK", 0, {"entropy": 0.0067}),
    (600.0, 128.0, 5.0, 7.5, 0, "VISION_OK", 0, {"entropy": 0.3333}),
    (600.0, 128.0, 5.0, 7.51, 0, "VISION_CORRUPTED", 0, {"entropy": 0.34}),
    (600.0, 128.0, 5.0, 0.0, 0, "VISION_CORRUPTED", 0, {"entropy": 1.0}),
    (600.0, 128.0, 5.0, 8.0, 0, "VISION_CORRUPTED", 0, {"entropy": 0.6667}),
    # blur: 1 - lap_var / 500 clipped to [0, 1]
    (0.0, 128.0, 5.0, 5.0, 0, "VISION_OK", 0, {"blur": 1.0}),
    (250.0, 128.0, 5.0, 5.0, 0, "VISION_OK", 0, {"blur": 0.5}),
    (500.0, 128.0, 5.0, 5.0, 0, "VISION_OK", 0, {"blur": 0.0}),
    (5000.0, 128.0, 5.0, 5.0, 0, "VISION_OK", 0, {"blur": 0.0}),
    # priority: blank beats frozen beats corrupted
    (600.0, 5.0, 0.0, 1.0, 7, "VISION_BLANK", 8, {"freeze": 1.0}),
    (600.0, 250.0, 0.0, 7.9, 4, "VISION_BLANK", 5, {"freeze": 1.0}),
    (600.0, 128.0, 0.0, 1.0, 4, "VISION_FROZEN", 5, {"freeze": 1.0}),
    (600.0, 128.0, 0.0, 7.9, 3, "VISION_CORRUPTED", 4, {"freeze": 0.24}),
]


@pytest.mark.parametrize("row", RULES, ids=lambda r: f"lv{r[0]}-m{r[1]}-d{r[2]}-e{r[3]}-run{r[4]}")
def test_score_frame_rule_table(row):
    lap_var, mean, mean_diff, entropy, frozen, status, run_after, metrics = row
    got, run = both(lap_var, mean, mean_diff, entropy, frozen)
    assert got["vision_status"] == status and run == run_after
    for k, v in metrics.items():
        assert got["metrics"][k] == v, (k, got["metrics"][k])


def test_score_frame_first_frame_placeholder_and_run_sequence():
    """No previous frame: frame_diff shows the placeholder 10.0, freeze is 0 and the frozen run is left alone.  Then the run
    0 -> 6 on still frames (freeze 0.3 * run / 5 until 5, then 1.0 and VISION_FROZEN) and one moving frame resets it."""
    got, run = both(600.0, 128.0, None, 5.0, 0)
    assert got["metrics"]["raw"]["frame_diff"] == 10.0 and got["metrics"]["freeze"] == 0.0 and run == 0
    assert got["vision_status"] == "VISION_OK" and got["anomaly_score"] == 0.0
    got, run = both(600.0, 128.0, None, 5.0, 3)               # as after reset() of the analyzer only; the run is not touched
    assert run == 3 and got["metrics"]["freeze"] == 0.0
    run, seen = 0, []
    for _ in range(6):
        got, run = both(600.0, 128.0, 0.5, 5.0, run)
        seen.append((run, got["metrics"]["freeze"], got["vision_status"], got["anomaly_score"]))
    ok, fz = "VISION_OK", "VISION_FROZEN"
    assert seen == [(1, 0.06, ok, 0.009), (2, 0.12, ok, 0.018), (3, 0.18, ok, 0.027), (4, 0.24, ok, 0.036),
                    (5, 1.0, fz, 0.15), (6, 1.0, fz, 0.15)]
    got, run = both(600.0, 128.0, 30.0, 5.0, run)
    assert run == 0 and got["vision_status"] == ok and got["metrics"]["freeze"] == 0.0 and got["anomaly_score"] == 0.0


def test_score_frame_fusion_weights_and_roundings():
    """Each weight alone (0.35 blur, 0.25 brightness, 0.15 freeze, 0.25 entropy), the clipped sum, and the rounding of every
    key: score to 6 places, the four metrics to 4, laplacian_var and frame_diff to 2, mean_brightness to 1, entropy to 3."""
    assert both(0.0, 128.0, 5.0, 5.0, 0)[0]["anomaly_score"] == 0.35
    assert both(600.0, 0.0, 5.0, 5.0, 0)[0]["anomaly_score"] == 0.25
    assert both(600.0, 128.0, 0.0, 5.0, 4)[0]["anomaly_score"] == 0.15
    assert both(600.0, 128.0, 5.0, 0.0, 0)[0]["anomaly_score"] == 0.25
    assert both(250.0, 128.0, None, 5.0, 0)[0]["anomaly_score"] == 0.175
    assert both(0.0, 256.0, 0.0, 0.0, 4)[0]["anomaly_score"] == 1.0
    got, _ = both(123.456789, 100.06, 3.14159, 5.4321987, 0)
    m = got["metrics"]
    assert m["raw"] == {"laplacian_var": 123.46, "mean_brightness": 100.1, "frame_diff": 3.14, "entropy": 5.432}
    assert m["blur"] == 0.7531 and m["brightness"] == 0.2183 and m["freeze"] == 0.0 and m["entropy"] == 0.0
    assert got["anomaly_score"] == round(0.35 * (1 - 123.456789 / 500) + 0.25 * (27.94 / 128), 6) == 0.318151
    got, _ = both(499.99, 127.99, 0.994, 3.9999, 0)           # values that round onto a threshold keep their unrounded rule
    assert got["metrics"]["raw"] == {"laplacian_var": 499.99, "mean_brightness": 128.0, "frame_diff": 0.99, "entropy": 4.0}
    assert got["metrics"]["blur"] == 0.0 and got["metrics"]["brightness"] == 0.0001 and got["metrics"]["entropy"] == 0.0
    assert got["anomaly_score"] == round(0.35 * (1 - 499.99 / 500) + 0.25 * (0.01 / 128) + 0.15 * 0.06
                                         + 0.25 * (4.0 - 3.9999) / 4.0, 6)


def test_entry_points_reject_before_touching_the_device():
    """The argument checks of fav_op_signal_stats and fav_op_corrupt return before any HIP call, so their verdicts can be
    seen without a GPU (tests/test_gpu_*_edges.py add that nothing was written).  The pointers are never dereferenced."""
    import ctypes as C
    import os
    from failure_aware_vision_amd import _lib
    if not os.path.exists(_lib.LIB_PATH):
        import __graft_entry__ as g
        g.build()
    lib = _lib.load()
    fn = lib.fav_op_signal_stats
    fn.restype = C.c_int
    fn.argtypes = [C.c_void_p, C.c_int32, C.c_int32, C.c_int32, C.c_void_p, C.c_void_p, C.c_void_p, C.c_void_p]
    A = 0x10000
    for args in ((A, 2, 2, 8, A, A, A), (A, 2, 4, 6, A, A, A), (A, 2, 4, 0, A, A, A), (A, 0, 4, 8, A, A, A),
                 (A, 2, 37501, 4, A, A, A), (None, 2, 4, 8, A, A, A), (A, 2, 4, 8, A, A, None),
                 (A + 1, 2, 4, 8, A, A, A), (A + 2, 2, 4, 8, None, None, A), (A, 2, 4, 8, A + 1, A, A),
                 (A, 2, 4, 8, A, A + 2, A), (A, 2, 4, 8, A, A, A + 4)):
        assert fn(*args, None) == 1 and b"fav_op_signal_stats" in lib.fav_last_error(None), args
    fc = lib.fav_op_corrupt
    fc.restype = C.c_int
    fc.argtypes = [C.c_void_p, C.c_void_p, C.c_int32, C.c_int32, C.c_int32, C.c_int32, C.c_float, C.c_float, C.c_float,
                   C.c_uint64, C.c_int64, C.c_void_p]
    for args in ((A, A, 2, 4, 8, -1), (A, A, 2, 4, 8, 4), (A, A, 0, 4, 8, 0), (A, A, 2, 0, 8, 0), (A, A, 2, 4, 0, 0),
                 (None, A, 2, 4, 8, 0), (A, None, 2, 4, 8, 0)):
        assert fc(*args, 0.0, 1.0, 0.0, 1, 0, None) == 1 and b"fav_op_corrupt" in lib.fav_last_error(None), args
