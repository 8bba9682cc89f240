"""corrupt_kernel at its edges.  The uint8 modes are fp32 arithmetic in a fixed order on Philox draws (the library is built
with -ffp-contract=off) and must equal oracle/corrupt_oracle.py bit for bit: rounding ties, both clamps, blocks that span
frames, odd widths, frames shorter than a bar, the 32-bit frame counter.  Gaussian noise is held to 2e-6 of a float64
Box-Muller on the same 24-bit uniforms, at all five severities."""
import numpy as np
import pytest

pytestmark = pytest.mark.gpu

torch = pytest.importorskip("torch")
from conftest import note  # noqa: E402
from failure_aware_vision_amd import _lib  # noqa: E402
from failure_aware_vision_amd.corrupt import Corruptor  # noqa: E402
from failure_aware_vision_amd.synth import GAUSSIAN_NOISE_SIGMA  # noqa: E402
from oracle import corrupt_oracle as CO  # noqa: E402
from oracle.fav_oracle import philox4x32_10  # noqa: E402

f32 = np.float32
# 35 pixels a frame puts several frames under one 256-thread block; 1x1x1, H == 1 and the odd widths have no full quad or row
SHAPES = ((1, 1, 1), (3, 1, 5), (2, 7, 3), (37, 5, 7), (5, 9, 13), (2, 16, 16), (1, 240, 320))
# (brightness, noise level) as set on the Corruptor -> (gain = brightness / 0.5, level)
PARAMS = {"ties": (0.25, 0.0), "zero": (0.0, 0.0), "identity": (0.5, 0.0), "clamps": (1.0, 1.0), "usual": (0.6, 0.4)}
SEEDS = (0, 0xABCDEF0123, 2 ** 64 - 1)


def frames_of(shape, seed):
    return np.random.default_rng(seed).integers(0, 256, shape + (3,), dtype=np.uint8)


def device_corrupt(frames, mode, brightness, level, seed, first_index):
    c = Corruptor(seed=seed)
    c.set_brightness(brightness); c.set_noise(level)
    out = c._run(torch.from_numpy(frames).cuda(), mode, torch.uint8, first_index=first_index)
    return out.cpu().numpy(), f32(c.brightness / 0.5), c.noise_level


def combos(shape):
    """Every (parameters, seed) for the small shapes; two of them at 240x320, where the Philox oracle costs the most."""
    if shape == (1, 240, 320):
        return [("ties", SEEDS[1]), ("clamps", SEEDS[2])]
    return [(p, s) for p in PARAMS for s in SEEDS]


@pytest.mark.parametrize("shape", SHAPES, ids=lambda s: "x".join(map(str, s)))
@pytest.mark.parametrize("mode", (0, 2))
def test_uint8_modes_bit_exact(mode, shape):
    frames = frames_of(shape, 11)
    big = shape[0] * shape[1] * shape[2] >= 64                 # enough pixels for the case to show what it is there for
    for name, seed in combos(shape):
        got, gain, level = device_corrupt(frames, mode, *PARAMS[name], seed, 3)
        want = CO.corrupt(frames, mode, level, gain, 0, seed, 3)
        assert got.dtype == np.uint8 and got.shape == frames.shape
        assert np.array_equal(got, want), (name, hex(seed), int((got != want).sum()))
        if mode == 0 and name == "ties" and big:
            v = frames.astype(f32) * gain                      # level 0: no noise, v = c / 2 exactly
            tie = v - np.floor(v) == f32(0.5)
            half_up = np.floor(v + f32(0.5)).astype(np.uint8)
            assert gain == 0.5 and tie.any() and (half_up != want).any()     # round-half-up would differ on these
            assert np.array_equal(want, np.rint(v).astype(np.uint8))
        if mode == 0 and name == "identity":
            assert np.array_equal(want, frames)
        if mode == 0 and name == "zero":
            assert not want.any()
        if mode == 0 and name == "clamps" and big:
            assert gain == 2.0 and level == 1.0 and (want == 0).any() and (want == 255).any()
            assert (want[frames >= 192] == 255).all()          # 2c - 127.5 >= 256.5: clamped from above


def bars(seed, frame, H):
    """The six bars of one frame as the kernel draws them: (first row, height) with height 2..13."""
    q = philox4x32_10(np.arange(6, dtype=np.uint32), np.uint32(frame), np.uint32(7), np.uint32(0), seed & 0xFFFFFFFF,
                      (seed >> 32) & 0xFFFFFFFF)
    by = np.floor(CO.u01(q[0]) * f32(H)).astype(int)
    bh = np.floor(f32(2.0) + CO.u01(q[1]) * f32(12.0)).astype(int)
    return list(zip(by.tolist(), bh.tolist()))


@pytest.mark.parametrize("shape,seed", [((3, 1, 5), 1), ((4, 2, 6), 2), ((5, 9, 13), 3), ((2, 9, 4), 0xABCDEF0123)],
                         ids=lambda v: "x".join(map(str, v)) if isinstance(v, tuple) else hex(v))
def test_bars_on_frames_shorter_than_a_bar(shape, seed):
    """H of 1, 2 and 9 against bars 2..13 rows high: some bar must start within two rows of the bottom and run past it,
    and some row must lie under two bars (their blends compose in bar order)."""
    n, H, W = shape
    first = 40
    cut = overlap = False
    for f in range(n):
        cover = np.zeros(H, int)
        for by, bh in bars(seed, first + f, H):
            assert 2 <= bh <= 13 and 0 <= by < H
            cut |= by >= H - 2 and by + bh > H
            cover[by:by + bh] += 1
        overlap |= bool((cover >= 2).any())
    assert cut and overlap
    frames = frames_of(shape, 12)
    for name in ("identity", "usual"):
        got, gain, level = device_corrupt(frames, 2, *PARAMS[name], seed, first)
        want = CO.corrupt(frames, 2, level, gain, 0, seed, first)
        assert np.array_equal(got, want), (name, int((got != want).sum()))
    assert (want[..., 1] == 0).any()                           # glitched pixels are there as well


def test_frame_counter_keeps_the_low_32_bits():
    """frame = low 32 bits of first_index + f: a run that starts at 2^32 - 2 draws frames 0 and 1 as its last two, and
    2^32 + 5 is 5.  The same two input frames repeat, so equal draws give equal output."""
    two = frames_of((2, 5, 7), 13)
    frames = np.concatenate([two, two])
    for mode in (0, 2):
        out = {}
        for first in (0, 5, 2 ** 31, 2 ** 32 - 2, 2 ** 32 + 5):
            got, gain, level = device_corrupt(frames, mode, 0.6, 0.4, SEEDS[1], first)
            assert np.array_equal(got, CO.corrupt(frames, mode, level, gain, 0, SEEDS[1], first)), (mode, first)
            out[first] = got
        assert np.array_equal(out[2 ** 32 - 2][2:], out[0][:2])
        assert not np.array_equal(out[2 ** 32 - 2][:2], out[0][:2]) and not np.array_equal(out[2 ** 31], out[0])
        assert np.array_equal(out[2 ** 32 + 5], out[5]) and not np.array_equal(out[5], out[0])
    c = Corruptor(seed=9)                                       # Gaussian mode shares the counter
    dev = torch.from_numpy(frames).cuda()
    g0, gw = c.gaussian(dev, 2, first_index=0).cpu().numpy(), c.gaussian(dev, 2, first_index=2 ** 32 - 2).cpu().numpy()
    assert np.array_equal(gw[2:], g0[:2]) and not np.array_equal(gw[:2], g0[:2])
    assert np.array_equal(c.gaussian(dev, 2, first_index=2 ** 32 + 5).cpu().numpy(), c.gaussian(dev, 2, first_index=5).cpu().numpy())


@pytest.mark.parametrize("shape", [s for s in SHAPES if s != (2, 16, 16) and s != (1, 240, 320)],
                         ids=lambda s: "x".join(map(str, s)))
def test_blank_is_2_2_4_everywhere(shape):
    got, _, _ = device_corrupt(frames_of(shape, 14), 1, 0.6, 0.4, 5, 0)
    assert got.shape == shape + (3,) and (got == np.array([2, 2, 4], np.uint8)).all()


def gaussian_f64(frames, sigma, seed, first_index):
    """Box-Muller in float64 on the kernel's own 24-bit uniforms: clip(c / 255 + sigma * z, 0, 1), z from
    sqrt(-2 ln(1 - u)) * (cos, sin)(2 pi u').  sigma is the float32 the C ABI carries.  Also returns the unclipped value."""
    n, H, W, _ = frames.shape
    px = np.arange(H * W, dtype=np.uint32)[None, :]
    fr = np.arange(n, dtype=np.uint64) + np.uint64(first_index & 0xFFFFFFFF)
    fr = (fr & np.uint64(0xFFFFFFFF)).astype(np.uint32)[:, None]
    a = philox4x32_10(px, fr, np.uint32(3), np.uint32(0), seed & 0xFFFFFFFF, (seed >> 32) & 0xFFFFFFFF)
    u = [(x >> np.uint32(8)).astype(np.float64) / 16777216.0 for x in a]
    r0, r1 = np.sqrt(-2.0 * np.log(1.0 - u[0])), np.sqrt(-2.0 * np.log(1.0 - u[2]))
    t0, t1 = 2.0 * np.pi * u[1], 2.0 * np.pi * u[3]
    z = np.stack([r0 * np.cos(t0), r0 * np.sin(t0), r1 * np.cos(t1)], axis=-1)
    raw = frames.reshape(n, H * W, 3).astype(np.float64) / 255.0 + float(f32(sigma)) * z
    return np.clip(raw, 0.0, 1.0).reshape(frames.shape), raw.reshape(frames.shape)


def gaussian_frames():
    """(2, 64, 64): row 0 black, row 1 white, row 2 random, the rest mid-gray 128 - the sample for the noise statistics,
    chosen by the clean value alone so that the choice does not depend on the draw."""
    frames = np.full((2, 64, 64, 3), 128, np.uint8)
    frames[:, 0], frames[:, 1] = 0, 255
    frames[:, 2] = np.random.default_rng(15).integers(0, 256, (2, 64, 3), dtype=np.uint8)
    return frames


# The float32 CPU restatement of the same formula is within 1.4e-7 / 1.8e-7 / 2.4e-7 / 3.6e-7 / 5.2e-7 of float64 at severities
# 1..5 on these frames, which leaves the bound a factor of four for the device's logf / sqrtf / cosf / sinf.  The test prints
# the device's own maximum per severity;
# the device figure is not yet written here: record it from the first MI355X run of this file.
GAUSSIAN_TOL = 2e-6


@pytest.mark.parametrize("severity", (1, 2, 3, 4, 5))
def test_gaussian_against_float64_box_muller(severity):
    sigma = GAUSSIAN_NOISE_SIGMA[severity - 1]
    frames, seed, first = gaussian_frames(), 77, 1000
    c = Corruptor(seed=seed)
    out = c.gaussian(torch.from_numpy(frames).cuda(), severity, first_index=first).cpu().numpy()
    ref, raw = gaussian_f64(frames, sigma, seed, first)
    assert out.dtype == np.float32 and out.shape == frames.shape
    worst = float(np.abs(out.astype(np.float64) - ref).max())
    note(f"corrupt edges: gaussian severity {severity} (sigma {sigma}): max |device - float64| = {worst:.3e}")
    assert worst <= GAUSSIAN_TOL
    assert np.isfinite(out).all() and out.min() >= 0.0 and out.max() <= 1.0
    assert (out == 0.0).any() and (out == 1.0).any()
    assert (out[:, 0] == 0.0).mean() > 0.4 and (out[:, 1] == 1.0).mean() > 0.4      # half the draws push past each clamp
    # Noise statistics on the N = 2 * 61 * 64 * 3 = 23424 mid-gray values (clean value 128 / 255, clamp window
    # [-0.502, +0.498] around it).  The clamp only moves residuals beyond the window onto its edges, so:
    #  * the residual's quantiles at Phi(-1) and Phi(+1) are untouched at every severity (sigma <= 0.38 < 0.498), and half
    #    their distance estimates sigma with standard error 0.96 sigma / sqrt(N) = 0.63 %: 3 % is 4.8 standard errors;
    #  * the mean of the clamped residual has standard error below sigma / sqrt(N) = 0.65 % of sigma and a bias below
    #    0.004 * P(residual > 0.498) < 4e-4 from the window's asymmetry, inside the 1e-3 of the bound; the bound
    #    0.01 sigma + 1e-3 is 3.4 standard errors at severity 1 and 1.9 at severity 5.  The draw is fixed by (seed, frame
    #    index), so the test is deterministic: the float64 reference's own mean is asserted to lie inside the same bound.
    #  * where no mid-gray value can be clamped often enough to matter (4 sigma <= 0.498: severities 1 and 2, truncation
    #    bias of the standard deviation below 0.1 %), the plain standard deviation of the unclipped residuals is held to the
    #    same 3 %, standard error 1 / sqrt(2 N) = 0.46 %.
    mid = np.zeros(frames.shape, bool)
    mid[:, 3:] = True
    clean = 128.0 / 255.0
    resid = out.astype(np.float64)[mid] - clean
    lo, hi = np.quantile(resid, [0.15865525393145707, 0.8413447460685429])
    assert abs((hi - lo) / 2.0 - sigma) <= 0.03 * sigma, ((hi - lo) / 2.0, sigma)
    assert abs((ref[mid] - clean).mean()) < 0.01 * sigma + 1e-3
    assert abs(resid.mean()) < 0.01 * sigma + 1e-3, resid.mean()
    if 4.0 * sigma <= 0.498:
        unclipped = mid & (raw > 0.0) & (raw < 1.0)
        r = out.astype(np.float64)[unclipped] - clean
        assert unclipped.sum() > 0.999 * mid.sum() and abs(r.std() - sigma) <= 0.03 * sigma


def test_corruptor_state():
    frames = frames_of((5, 6, 10), 16)
    dev = torch.from_numpy(frames).cuda()
    c = Corruptor(seed=21)
    c.set_noise(0.4); c.set_brightness(0.6)
    c.set_mode("frozen")                                       # nothing shown yet: behaves as normal
    first = c.apply(dev[:2]).cpu().numpy()
    assert np.array_equal(first, CO.corrupt(frames[:2], 0, 0.4, f32(0.6 / 0.5), 0, 21, 0))
    assert c.get_vision_status() == "VISION_FROZEN"
    held = c.apply(dev[2:]).cpu().numpy()                       # now it repeats the last frame shown
    assert all(np.array_equal(h, first[-1]) for h in held) and c._frame_index == 5
    c.reset()
    assert (c.mode, c.noise_level, c.brightness, c._frame_index, c._last) == ("normal", 0.0, 0.5, 0, None)
    c.set_noise(0.4); c.set_brightness(0.6)
    whole = CO.corrupt(frames, 0, 0.4, f32(0.6 / 0.5), 0, 21, 0)
    a, b = c.apply(dev[:2]).cpu().numpy(), c.apply(dev[2:]).cpu().numpy()          # 2 + 3 frames == 5 frames
    assert np.array_equal(np.concatenate([a, b]), whole) and c._frame_index == 5
    nxt = c.apply(dev[:1]).cpu().numpy()
    assert np.array_equal(nxt, CO.corrupt(frames[:1], 0, 0.4, f32(0.6 / 0.5), 0, 21, 5))
    c.reset()
    c.set_noise(0.4); c.set_brightness(0.6)
    assert np.array_equal(c.apply(dev).cpu().numpy(), whole)   # reset() restarts the index
    c.set_mode("corrupted"); c.set_mode("sideways"); c.set_mode(None)
    assert c.mode == "corrupted" and c.get_vision_status() == "VISION_CORRUPTED"
    for setter, attr in ((c.set_noise, "noise_level"), (c.set_brightness, "brightness")):
        for given, kept in ((-0.5, 0.0), (0.0, 0.0), (0.3, 0.3), (1.0, 1.0), (1.5, 1.0)):
            setter(given)
            assert getattr(c, attr) == kept


REJECTED = [("mode -1", dict(mode=-1)), ("mode 4", dict(mode=4)), ("n == 0", dict(n=0)), ("H == 0", dict(H=0)),
            ("W == 0", dict(W=0)), ("null input", dict(inp=None)), ("null output", dict(out=None))]


@pytest.mark.parametrize("why,kw", REJECTED, ids=[r[0] for r in REJECTED])
def test_rejections_launch_nothing(why, kw):
    c = Corruptor(seed=1)                                       # sets the argument types of fav_op_corrupt
    fn = c.lib.fav_op_corrupt
    inp = torch.full((2 * 4 * 8 * 3,), 100, dtype=torch.uint8, device="cuda")
    out = torch.full((2 * 4 * 8 * 3 * 4,), 0xA5, dtype=torch.uint8, device="cuda")  # room for fp32 output
    stream = torch.cuda.current_stream().cuda_stream
    status = fn(None if "inp" in kw else inp.data_ptr(), None if "out" in kw else out.data_ptr(), kw.get("n", 2),
                kw.get("H", 4), kw.get("W", 8), kw.get("mode", 0), 0.0, 1.0, 0.0, 1, 0, stream)
    torch.cuda.synchronize()
    assert status == 1, why                                    # FAV_ERR_INVALID_ARG
    assert b"fav_op_corrupt" in _lib.load().fav_last_error(None)
    assert bool((out == 0xA5).all()), f"{why}: something was written"
    assert fn(inp.data_ptr(), out.data_ptr(), 2, 4, 8, 0, 0.0, 1.0, 0.0, 1, 0, stream) == 0      # in contract: accepted
    torch.cuda.synchronize()
    assert bool((out[:192] == 100).all()) and bool((out[192:] == 0xA5).all())
