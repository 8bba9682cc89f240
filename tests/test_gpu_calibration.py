"""The temperature-sweep head and the calibration built on it, on the GPU: fav_op_head_sweep against the existing heads
(label and confidence bit for bit at every temperature), against the tests' float64 reference (calibration_ref.py: nll,
brier), against itself (the grouping of temperatures never changes a result), the temperature fit on synthetic logits with
a known answer, and Backend.calibration_sweep / calibrate_temperature / calibrate_tau / calibration_report / apply and
the setters.

TOL, the bound on |dev - ref| / max(1, |ref|) of nll and brier (fp32 device arithmetic against float64).  The rule is: measure
the maximum over every case of test_label_and_confidence_bitwise_and_nll_brier_vs_float64 (the shapes below, conf kinds
0 / 1 / 2, K = 32 and K = 1) and the three fit cases, adopt 4 x that rounded up to one significant digit, at most 1e-4.
Measured on an MI355X: the maximum is 2.1e-6 (nll 2.011e-6, brier 1.888e-6, both in the fit case T = 1, n = 2000, C = 100;
the item-1 shapes stay below 3.5e-7), so TOL = 4 x 2.011e-6 = 8.04e-6, rounded up to one digit: 9e-6.  The error is what
the formats predict: the device rounds z = logit * inv_temp to fp32 where the reference keeps the float64 product, up to
|z| 2^-24 absolute, which goes straight into ln pbar[y].  Every check prints a MEASURED line before it asserts."""
import ctypes as C
import math

import numpy as np
import pytest

pytestmark = pytest.mark.gpu

torch = pytest.importorskip("torch")
from failure_aware_vision_amd import Backend, Calibration, _lib, synth, weights  # noqa: E402
from failure_aware_vision_amd.calibration import fit_temperature, temperature_grid, unpack_cells  # noqa: E402
import calibration_ref as ref  # noqa: E402

TOL = 9e-6
SHAPES = [(1, 6, 1000, 1024), (2, 5, 7, 8), (30, 9, 1000, 1024), (64, 3, 100, 128), (2, 4, 10, 64), (30, 4, 1024, 1024),
          (1, 7, 257, 260)]
FIT_CASES = [(1, 2000, 100, 2.5, 1, 2.57), (8, 2000, 100, 2.5, 2, 2.52), (30, 512, 1000, 3.0, 3, 2.99)]
GRID = temperature_grid(0.25, 8.0)


@pytest.fixture(scope="module")
def lib():
    assert torch.cuda.is_available(), "GPU tests need a MI355X"
    return _lib.load()


def logits_case(T, n, Cc, ld, seed):
    """A frame's own class preferences plus per-sample noise; the padding columns hold 1e9 and must be ignored."""
    rng = np.random.default_rng(seed)
    lg = np.zeros((T, n, ld), np.float32)
    base = rng.standard_normal((1, n, Cc)) * 3
    lg[:, :, :Cc] = (base + rng.standard_normal((T, n, Cc)) * 1.5).astype(np.float32)
    lg[:, :, Cc:] = 1e9
    return lg


def labels_case(n, Cc, seed):
    """True labels, the last two outside [0, C)."""
    y = np.random.default_rng(seed).integers(0, Cc, n).astype(np.int32)
    y[-1], y[-2] = Cc, -1
    return y


def sweep(lib, d, T, n, Cc, ld, temps, kind, y):
    """fav_op_head_sweep on device logits d -> int32[n, K, 4] numpy cells (prefilled with a pattern: every cell is written)."""
    t = np.ascontiguousarray(np.asarray(temps, np.float32))
    cells = torch.full((n, t.size, 4), -7, dtype=torch.int32, device="cuda")
    lab = torch.from_numpy(np.asarray(y, np.int32)).cuda()
    _lib.check(lib.fav_op_head_sweep(d.data_ptr(), T, n, Cc, ld, t.ctypes.data_as(C.POINTER(C.c_float)), t.size, kind,
                                     lab.data_ptr(), cells.data_ptr(), None))
    torch.cuda.synchronize()
    return cells.cpu().numpy()


def heads(lib, d, T, n, Cc, ld, temp, kind):
    """(label, confidence) of the existing heads at one temperature: fav_op_head (kinds 0, 1), fav_op_head_uncertainty (2)."""
    if kind < 2:
        labels = torch.empty(n, dtype=torch.int32, device="cuda")
        conf = torch.empty(n, dtype=torch.float32, device="cuda")
        _lib.check(lib.fav_op_head(d.data_ptr(), T, n, Cc, ld, float(temp), kind, 0.5, labels.data_ptr(), conf.data_ptr(),
                                   None, None, None))
        return labels.cpu().numpy(), conf.cpu().numpy()
    rec = torch.empty((n, 18), dtype=torch.int32, device="cuda")
    _lib.check(lib.fav_op_head_uncertainty(d.data_ptr(), T, n, Cc, ld, float(temp), kind, 0.5, rec.data_ptr(), None, None, None))
    r = rec.cpu().numpy()
    return r[:, 0].copy(), r[:, 1].copy().view(np.float32)


def check_nll_brier(cells, lg, y, temps, what):
    """nll and brier of the cells against float64, within TOL; NaN exactly where the label is out of range.  Prints the
    measured maximum before asserting."""
    c = unpack_cells(cells)
    r = ref.sweep_of(lg, y, temps)
    bad = np.isnan(r["nll"])
    assert np.array_equal(np.isnan(c["nll"]), bad) and np.array_equal(np.isnan(c["brier"]), bad)
    e_nll = ref.error_measure(c["nll"][~bad], r["nll"][~bad]).max()
    e_brier = ref.error_measure(c["brier"][~bad], r["brier"][~bad]).max()
    print(f"MEASURED {what}: nll_err {e_nll:.3e} brier_err {e_brier:.3e}")
    assert e_nll <= TOL and e_brier <= TOL, (what, e_nll, e_brier)
    return max(e_nll, e_brier)


@pytest.mark.parametrize("T,n,Cc,ld", SHAPES)
def test_label_and_confidence_bitwise_and_nll_brier_vs_float64(lib, T, n, Cc, ld):
    """Items 1 and 2: every cell's label and confidence equal the existing heads' at that temperature on the bits, no
    tolerance and no cell left out; nll / brier within TOL of float64; out-of-range labels give NaN in both and leave
    label / confidence intact."""
    lg = logits_case(T, n, Cc, ld, T * 1000 + Cc)
    y = labels_case(n, Cc, Cc + T)
    d = torch.from_numpy(lg).cuda()
    for kind in (0, 1, 2):
        if kind == 2 and (T < 2 or Cc < 2):
            continue
        for temps in (GRID, GRID[13:14]):
            cells = sweep(lib, d, T, n, Cc, ld, temps, kind, y)
            c = unpack_cells(cells)
            for k, temp in enumerate(temps):
                hl, hc = heads(lib, d, T, n, Cc, ld, temp, kind)
                assert np.array_equal(c["label"][:, k], hl), (kind, k)
                assert np.array_equal(c["confidence"][:, k].view(np.int32), hc.view(np.int32)), (kind, k)
            check_nll_brier(cells, lg[:, :, :Cc], y, temps, f"shape {(T, n, Cc, ld)} kind {kind} K {len(temps)}")


@pytest.mark.parametrize("T,n,Cc,ld", [(30, 9, 1000, 1024), (64, 3, 100, 128), (2, 5, 7, 8), (1, 7, 257, 260)])
def test_schedule_invariance(lib, T, n, Cc, ld):
    """Item 3: the cells of one launch with K temperatures equal, bit for bit, those of K launches with one each - for
    K = 32 and for K = 5, which no group size divides."""
    lg = logits_case(T, n, Cc, ld, 7 * T + Cc)
    y = labels_case(n, Cc, 3)
    d = torch.from_numpy(lg).cuda()
    for kind in (0, 2) if T >= 2 else (0, 1):
        single = np.concatenate([sweep(lib, d, T, n, Cc, ld, GRID[k:k + 1], kind, y) for k in range(32)], axis=1)
        assert np.array_equal(sweep(lib, d, T, n, Cc, ld, GRID, kind, y), single), kind
        five = GRID[[3, 9, 14, 20, 31]]
        assert np.array_equal(sweep(lib, d, T, n, Cc, ld, five, kind, y), single[:, [3, 9, 14, 20, 31]]), kind


def test_more_rows_than_the_lds_holds(lib):
    """T x C beyond the staged rows: the rest are re-read from global memory, with the same bits as one launch each."""
    T, n, Cc, ld = 80, 2, 1000, 1024            # 80 rows of 4000 B: 35 fit in 140 KB
    lg = logits_case(T, n, Cc, ld, 5)
    y = np.array([3, 999], np.int32)
    d = torch.from_numpy(lg).cuda()
    temps = GRID[[0, 8, 13, 20, 31]]
    cells = sweep(lib, d, T, n, Cc, ld, temps, 0, y)
    for k, temp in enumerate(temps):
        hl, hc = heads(lib, d, T, n, Cc, ld, temp, 0)
        assert np.array_equal(cells[:, k, 0], hl) and np.array_equal(cells[:, k, 1], hc.view(np.int32))
    check_nll_brier(cells, lg[:, :, :Cc], y, temps, "T=80 beyond the LDS")


def fit_check(nll_dev_of, nll_ref_of, what):
    """Item 4's criterion: the device's fitted temperature is, on the float64 curve, at most 2 TOL max(1, NLL) above the
    float64 fit's; neither fit is at a bound.  Returns the two fits."""
    fd, fr = fit_temperature(nll_dev_of), fit_temperature(nll_ref_of)
    at_dev, at_ref = (float(nll_ref_of(np.array([t], np.float32))[0]) for t in (fd.temperature, fr.temperature))
    print(f"MEASURED fit {what}: t_dev {fd.temperature:.6f} t_ref {fr.temperature:.6f} ratio {fd.temperature / fr.temperature:.6f} "
          f"NLL_ref(t_dev) - NLL_ref(t_ref) {at_dev - at_ref:.3e} rounds {fd.rounds}")
    assert not fd.at_bound and not fr.at_bound and fd.rounds == 3
    assert at_dev - at_ref <= 2 * TOL * max(1.0, at_ref)
    return fd, fr


@pytest.mark.parametrize("T,n,Cc,scale,seed,t_star", FIT_CASES)
def test_fit_on_synthetic_logits(lib, T, n, Cc, scale, seed, t_star):
    """Item 4: logits built so that the best temperature is known (about t_star); the mean NLL over the first grid is
    unimodal with an interior minimum; the fit through the device sweep obeys fit_check against the float64 fit."""
    lg, y = ref.fit_case(T, n, Cc, scale, seed)
    nll_ref_of = ref.mean_nll_of(lg, y)
    curve = nll_ref_of(GRID)
    k = int(np.argmin(curve))
    assert 0 < k < 31 and np.all(np.diff(curve[:k + 1]) < 0) and np.all(np.diff(curve[k:]) > 0)
    assert abs(GRID[k] / t_star - 1.0) < 0.12                       # one grid step
    d = torch.from_numpy(lg).cuda()
    check_nll_brier(sweep(lib, d, T, n, Cc, Cc, GRID, 0, y), lg, y, GRID, f"fit case {(T, n, Cc)}")

    def nll_dev_of(temps):
        return unpack_cells(sweep(lib, d, T, n, Cc, Cc, temps, 0, y))["nll"].astype(np.float64).mean(axis=0)
    fd, _ = fit_check(nll_dev_of, nll_ref_of, (T, n, Cc))
    assert abs(fd.temperature / t_star - 1.0) < 0.02
    # the fitted temperature is where mean confidence meets accuracy; at temperature 1 the model is overconfident
    at = ref.cells_of(lg, y, fd.temperature)
    one = ref.cells_of(lg, y, 1.0)
    acc = float((at["label"] == y).mean())
    print(f"MEASURED fit {(T, n, Cc)}: accuracy {acc:.3f} mean conf at fit {at['confidence'].mean():.3f} at 1 {one['confidence'].mean():.3f}")
    assert abs(at["confidence"].mean() - acc) < 0.05 < one["confidence"].mean() - acc


# ---- through the Backend ---------------------------------------------------------------------------------------------
def make_backend(which, **kw):
    if which == "mc":
        blob, _ = weights.make_synthetic("resnet18_cifar", seed=1)
        return Backend("resnet18_cifar", blob, max_batch=96, n_samples=8, dropout_policy="all_blocks", dropout_p=0.1, seed=4, **kw), 32
    if which == "vit":
        blob, _ = weights.make_synthetic_vit("vit_tiny", seed=3)
        return Backend("vit_tiny", blob, max_batch=96, **kw), 64
    blobs = [weights.make_synthetic("resnet18_cifar", seed=s)[0] for s in (1, 2)]
    return Backend("resnet18_cifar", blobs, max_batch=96, **kw), 32


def detect_all(be, x):
    outs = [be.classify_detect(x[b:b + 96], first_index=b) for b in range(0, x.shape[0], 96)]
    return [torch.cat([o[i] for o in outs]).cpu().numpy() for i in range(4)]


def labelled_frames(be, hw, n=256):
    """256 synthetic frames (three batches of max_batch = 96); the 128 the model is most confident about at temperature 1
    keep its own label, the rest get (label + 1) % C: accuracy exactly 0.5, errors at low confidence."""
    x = torch.from_numpy(synth.synthetic_frames_u8(n, hw, hw, seed=13)).cuda()
    lab, conf, _, _ = detect_all(be, x)
    order = np.lexsort((np.arange(n), -conf.astype(np.float64)))    # confidence descending, ties by frame index
    y = (lab + 1) % be.cfg.num_classes
    y[order[:n // 2]] = lab[order[:n // 2]]
    return x, y.astype(np.int32)


def batch_logits(be, x, b):
    """[T, nb, ld] device logits of batch b (rows padded to a multiple of 4 floats) after a classify call on it."""
    be.classify_detect(x[b:b + 96], first_index=b)
    lg = be.logits()
    pad = -lg.shape[2] % 4
    return torch.nn.functional.pad(lg, (0, pad)).contiguous() if pad else lg


@pytest.mark.parametrize("which", ["mc", "vit", "ens"])
def test_backend_sweep_bits_and_apply(lib, which):
    be, hw = make_backend(which)
    x, y = labelled_frames(be, hw)
    Cc = be.cfg.num_classes
    cells = be.calibration_sweep(x, y, GRID).cpu().numpy()
    assert cells.shape == (256, 32, 4)
    for b in range(0, 256, 96):
        lg = batch_logits(be, x, b)
        T, nb, ld = lg.shape
        assert T == be.T
        assert np.array_equal(cells[b:b + nb], sweep(lib, lg, T, nb, Cc, ld, GRID, be.cfg.conf_kind, y[b:b + nb])), b
    # numpy in -> numpy out, the same cells
    assert np.array_equal(be.calibration_sweep(x.cpu().numpy(), y, GRID[:5]), cells[:, :5])
    # apply: the handle then classifies exactly as a fresh one constructed with the calibrated values
    cal = Calibration(temperature=float(GRID[17]), tau=0.3)
    be.apply(cal)
    assert (be.cfg.temperature, be.cfg.tau) == (np.float32(cal.temperature), np.float32(cal.tau))
    fresh, _ = make_backend(which, temperature=cal.temperature, tau=cal.tau)
    for got, want in zip(detect_all(be, x), detect_all(fresh, x)):
        assert np.array_equal(got.view(np.uint8), want.view(np.uint8))
    fresh.close()
    be.close()


def test_backend_calibration_end_to_end(lib):
    """Item 5 on resnet18_cifar, MC-Dropout T = 8: one forward pass per batch in calibrate_temperature, its fit against
    the float64 fit on the same logits, calibration_report against float64, calibrate_tau's risk and coverage exact."""
    be, hw = make_backend("mc")
    x, y = labelled_frames(be, hw)
    n, Cc = 256, be.cfg.num_classes
    logits = np.concatenate([batch_logits(be, x, b)[:, :, :Cc].cpu().numpy() for b in range(0, n, 96)], axis=1)
    # one forward pass per batch: count the calls of fav_classify_sweep and the head launches of the whole fit
    calls = []
    orig = be.lib
    proxy = _Proxy(orig, calls)
    be.lib = proxy
    be.set_profiling(True)
    be.get_profile()
    fit = be.calibrate_temperature(x, y)
    prof = be.get_profile()
    be.set_profiling(False)
    be.lib = orig
    assert calls == [96, 96, 64]
    assert prof["head"]["launches"] == 3 and prof["conv_igemm"]["launches"] > 0     # later rounds run on the kept logits
    ref_of = ref.mean_nll_of(logits, y)

    fr = fit_temperature(ref_of)
    at_dev, at_ref = (float(ref_of(np.array([t], np.float32))[0]) for t in (fit.temperature, fr.temperature))
    print(f"MEASURED backend fit: t_dev {fit.temperature:.6f} t_ref {fr.temperature:.6f} diff {at_dev - at_ref:.3e} "
          f"at_bound {fit.at_bound}/{fr.at_bound} rounds {fit.rounds}")
    assert not fit.at_bound and not fr.at_bound and fit.rounds == 3 == fr.rounds
    assert at_dev - at_ref <= 2 * TOL * max(1.0, at_ref)
    assert be.cfg.temperature == 1.0                                # the handle is not changed
    # a set too large for the budget is refused, with its size
    with pytest.raises(ValueError, match=str(4 * 8 * 256 * 12)):
        be.calibrate_temperature(x, y, logits_budget_bytes=1000)

    be.set_temperature(fit.temperature)
    rep = be.calibration_report(x, y)
    r = ref.cells_of(logits, y, fit.temperature, be.cfg.conf_kind)
    correct = r["label"] == y
    from failure_aware_vision_amd import reliability, risk_coverage
    rel = reliability(r["confidence"], correct)
    edges = np.arange(16) / 15.0
    near = int((np.abs(r["confidence"][:, None] - edges[None, :]).min(axis=1) <= 1e-5).sum())
    print(f"MEASURED report: {rep} ref ece {rel['ece']:.6f} frames near a bin edge {near}")
    assert near <= 0.02 * n
    assert rep["accuracy"] == correct.mean()
    assert ref.error_measure(rep["nll"], r["nll"].mean()) <= TOL and ref.error_measure(rep["brier"], r["brier"].mean()) <= TOL
    assert abs(rep["ece"] - rel["ece"]) <= TOL + near / n
    assert abs(rep["mean_confidence"] - r["confidence"].mean()) <= 2e-5
    # AURC: fp32 and float64 confidences order the frames alike except within near-ties; a frame that changes places
    # moves one prefix risk by at most 1 / accepted, weighted 1 / n
    srt = np.sort(r["confidence"])
    tied = int((np.diff(srt) <= 1e-5).sum())
    print(f"MEASURED report: aurc {rep['aurc']:.6f} ref {risk_coverage(r['confidence'], correct)['aurc']:.6f} near-tied pairs {tied}")
    assert abs(rep["aurc"] - risk_coverage(r["confidence"], correct)["aurc"]) <= TOL + 2 * tied / n

    got = be.calibrate_tau(x, y, target_risk=0.3)
    print(f"MEASURED calibrate_tau(0.3): {got}")
    assert math.isfinite(got["tau"]) and got["coverage"] > 0
    be.set_tau(got["tau"])
    lab, conf, fail, _ = detect_all(be, x)
    acc = fail == 0
    assert np.array_equal(acc, conf >= np.float32(got["tau"]))
    risk = float((lab[acc] != y[acc]).sum()) / float(acc.sum())
    assert risk <= 0.3 and risk == got["risk"] and float(acc.sum()) / n == got["coverage"]
    g = be.calibrate_tau(x, y, target_risk=0.45, delta=0.05)
    print(f"MEASURED calibrate_tau(0.45, delta=0.05): {g}")
    if math.isfinite(g["tau"]):
        assert g["bound"] <= 0.45 and g["risk"] < g["bound"] and g["tau"] >= be.calibrate_tau(x, y, target_risk=0.45)["tau"]
    be.close()


class _Proxy:
    """The library with fav_classify_sweep's calls counted (their n recorded)."""
    def __init__(self, lib, calls):
        self._lib, self._calls = lib, calls

    def __getattr__(self, name):
        fn = getattr(self._lib, name)
        if name != "fav_classify_sweep":
            return fn

        def counted(*a):
            self._calls.append(a[2])
            return fn(*a)
        return counted


def test_setters(lib):
    """Item 6: a setter between two calls on one stream changes the second call only; rejected values leave the handle
    as it was and fav_last_error names them."""
    be, hw = make_backend("mc")
    x = torch.from_numpy(synth.synthetic_frames_u8(64, hw, hw, seed=3)).cuda()
    a = be.classify_detect(x)                       # enqueued at temperature 1, tau 0.5 ...
    be.set_temperature(2.5)                         # ... and not synchronised before the setters run
    be.set_tau(0.2)
    b = be.classify_detect(x)
    torch.cuda.synchronize()
    old, _ = make_backend("mc")
    new, _ = make_backend("mc", temperature=2.5, tau=0.2)
    for got, want in zip(a, old.classify_detect(x)):
        assert torch.equal(got, want)
    for got, want in zip(b, new.classify_detect(x)):
        assert torch.equal(got, want)
    assert not torch.equal(a[1], b[1])
    for bad in (0.0, -1.0, math.nan, math.inf):
        with pytest.raises(_lib.FavError, match="fav_set_temperature") as ei:
            be.set_temperature(bad)
        assert ei.value.status == 1 and be.cfg.temperature == np.float32(2.5)
    with pytest.raises(_lib.FavError, match="fav_set_tau"):
        be.set_tau(math.nan)
    assert be.cfg.tau == np.float32(0.2)
    for got, want in zip(be.classify_detect(x), b):  # the handle is as it was
        assert torch.equal(got, want)
    be.set_tau(-math.inf)                           # any non-NaN threshold is legal: nothing fails
    assert int(be.classify_detect(x)[2].sum()) == 0
    for o in (be, old, new):
        o.close()
