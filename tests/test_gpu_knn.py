"""Nearest-neighbour OOD scoring on the device: fav_op_knn_score against tests/knn_ref.py, and the Backend methods end to end.

Everything here is an equality of bits.  The contract (include/fav.h beside fav_knn_record) fixes every product and every
sum of the query, the similarity is the production GEMM accumulator, which the oracle models bit for bit, and the k-th
largest of a multiset is a value: a record must be the reference's dwords (a NaN counts as equal to any NaN).

Shapes of the op: D in {64, 128, 768, 2048}, N in {1, 15, 17, 63, 64, 65, 128, 257, 1000, 4099}, k in {1, 2, 10, 256, N}, S in
{1, 3}, n in {1, 2, 5, 17, 67, 4099} (the last for 4099 different norms through the square root and the division, and 33 row
tiles of the GEMM).  The GEMM reads the bank in tiles of 64 or 128 rows (128 when the rows it reads in place are a
multiple of 128), in place up to the last multiple of 64 and through a zero-padded tile behind it, and its row tile is 128
frames; the select reads 4096 columns a block pass, 4 a thread.  k == N with N no multiple of 64 (15, 63, 65) asks for the
most negative similarity, which a zero padding row would displace.

The records lie between guard bytes, and the workspace is filled with a pattern that reads as 1.5e16: a select that read a
padding column, or a row of the workspace nobody wrote, would report it as the nearest neighbour."""
import ctypes as C
import math

import numpy as np
import pytest

pytestmark = pytest.mark.gpu

torch = pytest.importorskip("torch")
import knn_ref as R  # noqa: E402
import ood_ref  # noqa: E402
from failure_aware_vision_amd import Backend, _lib, synth, views, weights  # noqa: E402
from failure_aware_vision_amd.ood import KNNBank, OODModel  # noqa: E402

GUARD = 64
FILL = 0x5A


@pytest.fixture(scope="module")
def lib():
    assert torch.cuda.is_available(), "GPU tests need a MI355X"
    return _lib.load()


def dev(a):
    return torch.from_numpy(np.ascontiguousarray(a)).cuda()


def run_op(lib, feat_bits, bank_bits, k, cls, thr, rec_off=0, S=None, n=None, D=None, N=None, null=(), feat_off=0, bank_off=0,
           ws_off=0, ws_short=0):
    """fav_op_knn_score -> (status, records int32 [n, 6], guard bytes untouched?, workspace untouched?).  The records lie
    rec_off bytes behind a guard in a buffer filled with FILL, and so does the workspace, ws_off bytes in and ws_short bytes
    shorter than fav_knn_workspace_bytes asks.  S .. N override the sizes passed; null: arguments to pass as NULL; feat_off /
    bank_off: the features / the bank start that many bf16 values into their buffers."""
    S0, n0, D0 = feat_bits.shape
    N0 = bank_bits.shape[0]
    fbuf = torch.zeros(feat_bits.size + 16, dtype=torch.int16, device="cuda")
    bbuf = torch.zeros(bank_bits.size + 16, dtype=torch.int16, device="cuda")
    assert fbuf.data_ptr() % 16 == 0 and bbuf.data_ptr() % 16 == 0
    fbuf[feat_off:feat_off + feat_bits.size] = dev(feat_bits.ravel().view(np.int16))
    bbuf[bank_off:bank_off + bank_bits.size] = dev(bank_bits.ravel().view(np.int16))
    cls_t = None if cls is None else dev(np.asarray(cls, np.int32))
    need = lib.fav_knn_workspace_bytes(n0, D0, N0)
    assert need > 0
    ws = torch.full((256 + need + GUARD,), FILL, dtype=torch.uint8, device="cuda")
    assert ws.data_ptr() % 256 == 0
    nbytes = 24 * n0
    buf = torch.full((GUARD + 16 + nbytes + GUARD,), FILL, dtype=torch.uint8, device="cuda")
    assert buf.data_ptr() % 16 == 0
    lo = GUARD + rec_off
    ptr = dict(feat=fbuf[feat_off:].data_ptr(), bank=bbuf[bank_off:].data_ptr(), cls=None if cls_t is None else cls_t.data_ptr(),
               ws=ws.data_ptr() + ws_off, records=buf.data_ptr() + lo)
    for name in null:
        ptr[name] = None
    st = lib.fav_op_knn_score(ptr["feat"], S0 if S is None else S, n0 if n is None else n, D0 if D is None else D, ptr["bank"],
                              N0 if N is None else N, k, ptr["cls"], thr, ptr["ws"], need - ws_short, ptr["records"],
                              torch.cuda.current_stream().cuda_stream)
    torch.cuda.synchronize()
    host, ws_host = buf.cpu().numpy(), ws.cpu().numpy()
    guards = bool((host[:lo] == FILL).all() and (host[lo + nbytes:] == FILL).all() and (ws_host[:ws_off] == FILL).all() and
                  (ws_host[ws_off + need:] == FILL).all())
    return st, host[lo:lo + nbytes].copy().view(np.int32).reshape(n0, 6), guards, bool((ws_host == FILL).all())


def unit_rows(rng, N, D):
    x = rng.standard_normal((N, D))
    return R.f32_to_bf16_bits((x / np.linalg.norm(x, axis=1, keepdims=True)).astype(np.float32))


def problem(D, N, k, S, n, seed=0):
    """Signed features and signed bank rows: the similarities are negative as well as positive."""
    rng = np.random.default_rng(1000 * D + 10 * N + k + S + n + seed)
    feat = R.f32_to_bf16_bits(rng.standard_normal((S, n, D)).astype(np.float32))
    cls = rng.integers(-1, max(2, N // 2), N).astype(np.int32)
    return feat, unit_rows(rng, N, D), cls


def same_records(got, want):
    return np.array_equal(R.canon_records(got), want)


# (D, N, k, S, n): every value beside an awkward partner
SHAPES = [(64, 1, 1, 1, 1), (64, 15, 15, 3, 5), (128, 17, 2, 1, 67), (128, 63, 63, 3, 2), (64, 65, 65, 1, 5), (768, 65, 10, 1, 17),
          (128, 64, 64, 1, 2), (128, 128, 10, 3, 5), (768, 257, 256, 3, 5), (2048, 1000, 256, 1, 2), (2048, 4099, 10, 3, 17),
          (64, 4099, 1, 1, 67), (2048, 17, 17, 1, 1), (64, 17, 2, 1, 4099)]


@pytest.mark.parametrize("shape", SHAPES, ids=["x".join(map(str, s)) for s in SHAPES])
def test_op_bit_exact(lib, shape):
    D, N, k, S, n = shape
    feat, bank, cls = problem(*shape)
    want = R.score(feat, bank, k, cls, 0.0)
    thr = float(np.median(want["kth_dist"]))                                         # both outcomes of the flag, one frame at equality
    want = R.score(feat, bank, k, cls, thr)
    assert n < 3 or 0 < want["ood"].sum() < n
    st, got, guards, _ = run_op(lib, feat, bank, k, cls, thr)
    assert st == 0 and guards
    assert same_records(got, R.records(want)), np.flatnonzero((R.canon_records(got) != R.records(want)).any(axis=1))[:8]
    st, got, guards, _ = run_op(lib, feat, bank, k, None, thr, rec_off=8)            # no class ids; records 8-byte aligned only
    assert st == 0 and guards and same_records(got, R.records(R.score(feat, bank, k, None, thr)))
    assert (got[:, 4] == -1).all()


def test_op_k_equal_n_reports_the_most_negative_similarity(lib):
    """N = 15, 63 and 65 rows, k = N: the GEMM's tile holds zero padding rows, whose similarity of 0 lies above the minimum."""
    for D, N, S, n in ((64, 15, 3, 5), (128, 63, 3, 2), (64, 65, 1, 5)):
        feat, bank, cls = problem(D, N, N, S, n)
        want = R.score(feat, bank, N, cls, math.inf)
        assert (want["kth_sim"] < 0).all()
        st, got, guards, _ = run_op(lib, feat, bank, N, cls, math.inf)
        assert st == 0 and guards and same_records(got, R.records(want))
        assert (got[:, 1].view(np.float32) < 0).all()


@pytest.mark.parametrize("feat_off", (1, 4, 7))
def test_op_features_off_a_16_byte_boundary(lib, feat_off):
    """The query kernel loads the features value by value, so 2, 8 and 14 bytes off a 16-byte boundary is the same path; the
    case stays as a pin for a later wide-load path."""
    for shape in ((64, 17, 2, 3, 5), (768, 65, 10, 1, 3)):
        feat, bank, cls = problem(*shape, seed=4)
        st, got, guards, _ = run_op(lib, feat, bank, shape[2], cls, 1.0, feat_off=feat_off)
        assert st == 0 and guards and same_records(got, R.records(R.score(feat, bank, shape[2], cls, 1.0))), shape


def test_op_ties(lib):
    rng = np.random.default_rng(7)
    D = 128
    feat = R.f32_to_bf16_bits(rng.standard_normal((1, 5, D)).astype(np.float32))
    # every distinct row four times: the 6th largest similarity sits inside the second run of four equal values
    bank = np.repeat(unit_rows(rng, 10, D), 4, axis=0)
    want = R.score(feat, bank, 6, None, math.inf)
    sims = np.sort(R.similarities(R.query(feat)[0], bank), axis=1)[:, ::-1]
    assert np.array_equal(sims[:, 4], sims[:, 7]) and np.array_equal(want["kth_sim"], sims[:, 5]) and (sims[:, 3] > sims[:, 4]).all()
    st, got, guards, _ = run_op(lib, feat, bank, 6, None, math.inf)
    assert st == 0 and guards and same_records(got, R.records(want))
    assert (got[:, 3] % 4 == 0).all()                                                # the first row of the best run
    # a bank whose rows are all identical, over a whole tile and a part tile
    same = np.repeat(unit_rows(rng, 1, D), 70, axis=0)
    want = R.score(feat, same, 33, None, math.inf)
    assert np.array_equal(want["kth_sim"], want["nn_sim"]) and (want["nn_row"] == 0).all()
    st, got, guards, _ = run_op(lib, feat, same, 33, None, math.inf)
    assert st == 0 and guards and same_records(got, R.records(want))
    # a query equal to a bank row, which three rows hold: in one thread's columns (5 and 4101), in another wave's (700)
    big = unit_rows(rng, 4200, D)
    big[700] = big[4101] = big[5]
    q = big[[5, 40]][None]
    cls = np.arange(4200, dtype=np.int32)
    want = R.score(q, big, 3, cls, math.inf)
    assert want["nn_row"].tolist() == [5, 40] and want["kth_sim"][0] == want["nn_sim"][0] and want["kth_sim"][1] < want["nn_sim"][1]
    st, got, guards, _ = run_op(lib, q, big, 3, cls, math.inf)
    assert st == 0 and guards and same_records(got, R.records(want))
    assert got[:, 3].tolist() == [5, 40] and got[:, 4].tolist() == [5, 40]           # the lower row of the shared maximum


def test_op_degenerate_frames_stay_in_their_frame(lib):
    feat, bank, cls = problem(128, 257, 10, 3, 9, seed=2)
    clean = R.score(feat, bank, 10, cls, 1.0)
    feat[:, 1, :] = 0                                                                # a zero row
    feat[0, 2, 40] = 0x7FC1                                                          # a NaN
    feat[1, 4, 5] = 0x7F80                                                           # +inf
    feat[2, 5, 0] = 0xFF80                                                           # -inf and +inf in two samples of one frame
    feat[0, 5, 0] = 0x7F80
    feat[:, 7, 127] = R.f32_to_bf16_bits(np.array([3e20], np.float32))[0]            # finite, its square is not
    bad = [1, 2, 4, 5, 7]
    want = R.score(feat, bank, 10, cls, 1.0)
    assert R.query(feat)[2].nonzero()[0].tolist() == bad
    assert (R.records(want)[bad] == np.array([0x7FC00000] * 3 + [-1, -1, 1], np.int32)).all()
    st, got, guards, _ = run_op(lib, feat, bank, 10, cls, 1.0)
    assert st == 0 and guards and same_records(got, R.records(want))
    keep = [0, 3, 6, 8]
    assert np.array_equal(R.canon_records(got)[keep], R.records(clean)[keep])        # the neighbours are unaffected
    assert (got[bad, :3] == 0x7FC00000).all()                                        # the contract's NaN, bit for bit


def test_op_thresholds(lib):
    feat, bank, cls = problem(64, 17, 2, 1, 5, seed=3)
    d = R.score(feat, bank, 2, cls, 0.0)["kth_dist"]
    for thr, flags in ((math.inf, [0] * 5), (-math.inf, [1] * 5), (float(d[3]), (~(d <= d[3])).astype(int).tolist()),
                       (float(np.nextafter(d[3], np.float32(0))), (~(d < d[3])).astype(int).tolist())):
        st, got, guards, _ = run_op(lib, feat, bank, 2, cls, thr)
        assert st == 0 and guards and got[:, 5].tolist() == flags, thr
    assert run_op(lib, feat, bank, 2, cls, float(d[3]))[1][3, 5] == 0                # exactly at the threshold: not flagged
    assert run_op(lib, feat, bank, 2, cls, float(np.nextafter(d[3], np.float32(0))))[1][3, 5] == 1   # one ulp below: flagged


REFUSALS = [("feat", dict(null=("feat",)), "null"), ("bank", dict(null=("bank",)), "null"), ("ws", dict(null=("ws",)), "null"),
            ("records", dict(null=("records",)), "null"),
            ("S 0", dict(S=0), "S=0"), ("S 4097", dict(S=4097), "S=4097"), ("n 0", dict(n=0), "n must"), ("n -1", dict(n=-1), "n must"),
            ("D 32", dict(D=32), "D=32"), ("D 96", dict(D=96), "D=96"), ("D 4160", dict(D=4160), "D=4160"),
            ("N 0", dict(N=0), "N=0"), ("N 262145", dict(N=262145), "N=262145"),
            ("k 0", dict(k=0), "k=0"), ("k N + 1", dict(k=18), "k=18"), ("k 257", dict(k=257, N=300), "k=257"),
            ("threshold NaN", dict(thr=math.nan), "threshold"), ("workspace a byte short", dict(ws_short=1), "ws_bytes"),
            ("workspace + 128", dict(ws_off=128), "256-byte"), ("bank + 8", dict(bank_off=4), "16-byte"),
            ("records + 4", dict(rec_off=4), "8-byte")]


@pytest.mark.parametrize("why,kw,text", REFUSALS, ids=[r[0] for r in REFUSALS])
def test_op_refusals_launch_nothing(lib, why, kw, text):
    feat, bank, cls = problem(64, 17, 2, 1, 5)
    kw = dict(kw)
    thr, k = kw.pop("thr", 1.0), kw.pop("k", 2)
    st, got, guards, ws_untouched = run_op(lib, feat, bank, k, cls, thr, **kw)
    msg = lib.fav_last_error(None).decode()
    assert st == 1 and "fav_op_knn_score" in msg and text in msg, (why, msg)
    assert guards and (got.view(np.uint8) == FILL).all() and ws_untouched            # neither records nor workspace touched


# ---- end to end ---------------------------------------------------------------------------------------------------------
@pytest.fixture(scope="module")
def r18_b(r18_blob):
    return r18_blob[0]


def features_of(be, frames):
    be.classify(dev(frames))
    return be.features().cpu().numpy()


def records_of(out):
    """classify_knn's dict (numpy values) -> int32 [n, 6] records."""
    return np.stack([out["kth_dist"].view(np.int32), out["kth_sim"].view(np.int32), out["nn_sim"].view(np.int32), out["nn_row"],
                     out["nn_class"], out["ood"]], axis=1)


def ood_records_of(out):
    """classify_ood's dict (numpy values) -> int32 [n, 4] records, NaNs canonical."""
    return ood_ref.canon_records(np.stack([out["min_dist"].view(np.int32), out["nearest_class"], out["label_dist"].view(np.int32),
                                           out["ood"]], axis=1))


def numpy_of(out):
    return {k: v.cpu().numpy() for k, v in out.items()}


def tap_is_on(be, lib):
    """after a classify call: fav_get_features answers with the sizes only while the tap is on."""
    return lib.fav_get_features(be._h, None, None, None, None, None) == 0


def test_backend_end_to_end(lib, r18_b):
    frames = synth.synthetic_frames_u8(64, 32, 32, seed=17)
    y = np.arange(64) % 10
    be = Backend("resnet18_cifar", r18_b, max_batch=32)
    plain = [t.cpu().numpy() for t in be.classify_detect(dev(frames[:32]), 7)]
    with pytest.raises(_lib.FavError, match="no k-NN bank"):
        be.classify_knn(dev(frames[:4]))
    bank = be.fit_knn(dev(frames[:61]), y[:61], k=5)                                 # two batches; 61 rows: the copy is padded
    assert (bank.D, bank.N, bank.k) == (512, 61, 5) and np.array_equal(bank.class_id, y[:61])
    assert not tap_is_on(be, lib)                                                    # fit_knn left the tap as it was: off
    bank.check(512)
    with pytest.raises(_lib.FavError, match="D=64"):
        be.set_knn(KNNBank(np.zeros((3, 64), np.uint16), k=1))
    assert be.knn_bank is None
    be.set_knn(bank)
    with pytest.raises(_lib.FavError, match="clear it first"):                      # the bank reads the tap
        be.set_feature_tap(False)
    got = numpy_of(be.classify_knn(dev(frames[:32]), 7))
    for name, want in zip(("label", "conf", "fail", "score"), plain):               # fav_classify_ex, unchanged
        assert np.array_equal(got[name].view(np.uint8), want.view(np.uint8)), name
    # the records: the reference on the tapped features, and the op on them
    ft = be.features()
    assert tuple(ft.shape) == (1, 32, 512)
    bits = R.f32_to_bf16_bits(ft.cpu().numpy())
    rec = records_of(got)
    assert same_records(rec, R.records(R.score(bits, bank.rows, 5, bank.class_id, math.inf)))
    st, op_rec, guards, _ = run_op(lib, bits, bank.rows, 5, bank.class_id, math.inf)
    assert st == 0 and guards and np.array_equal(R.canon_records(op_rec), R.canon_records(rec))
    assert got["ood"].sum() == 0 and (got["nn_class"] == y[got["nn_row"]]).all()     # threshold +inf
    assert (got["nn_sim"][:32] > 0.99).all()                                         # the frames are in the bank
    # numpy frames in -> numpy out, the same bits
    host = be.classify_knn(frames[:32], 7)
    assert isinstance(host["kth_dist"], np.ndarray) and np.array_equal(records_of(host), rec)
    # calibration: the reference's threshold and the reference's flags
    all_d = np.concatenate([R.score(R.f32_to_bf16_bits(f), bank.rows, 5, bank.class_id, 0.0)["kth_dist"]
                            for f in (features_of(be, frames[:32]), features_of(be, frames[32:]))])
    thr = be.calibrate_knn(dev(frames), tpr=0.9)
    assert thr == OODModel.threshold_for_tpr(all_d, 0.9) == be.knn_bank.threshold and np.mean(all_d <= thr) >= 0.9
    flags = np.concatenate([be.classify_knn(dev(frames[b:b + 32]))["ood"].cpu().numpy() for b in (0, 32)])
    assert np.array_equal(flags, (~(all_d <= np.float32(thr))).astype(np.int32)) and flags.sum() <= 6   # at least 58 of 64 pass
    rep = be.knn_report(dev(frames[:32]), dev(255 - frames[32:]))
    assert 0.0 <= rep["auroc"] <= 1.0 and rep["n_id"] == rep["n_ood"] == 32 and rep["threshold"] == thr
    # a Mahalanobis model beside the bank: each gives the records it gives alone, and knn_report has ood_report's keys
    knn_alone = records_of(numpy_of(be.classify_knn(dev(frames[:32]), 7)))
    model = be.fit_ood(dev(frames), y)
    be.set_ood(model)
    assert set(be.ood_report(dev(frames[:32]), dev(255 - frames[32:]))) == set(rep)
    both_knn = records_of(numpy_of(be.classify_knn(dev(frames[:32]), 7)))
    both_ood = numpy_of(be.classify_ood(dev(frames[:32]), 7))
    assert np.array_equal(R.canon_records(both_knn), R.canon_records(knn_alone))
    # the tap rules: clearing one head keeps the tap while the other is set
    be.set_knn(None)
    assert be.knn_bank is None
    ood_alone = numpy_of(be.classify_ood(dev(frames[:32]), 7))
    assert np.array_equal(ood_records_of(both_ood), ood_records_of(ood_alone))
    assert tap_is_on(be, lib)
    with pytest.raises(_lib.FavError, match="no k-NN bank"):
        be.classify_knn(dev(frames[:4]))
    be.set_knn(be.fit_knn(dev(frames[:61]), k=5))                                    # fit with a model set: its tap serves
    assert be.knn_bank.class_id is None
    be.set_ood(None)
    assert numpy_of(be.classify_knn(dev(frames[:32]), 7))["nn_class"].tolist() == [-1] * 32 and tap_is_on(be, lib)
    with pytest.raises(_lib.FavError, match="clear it first"):
        be.set_feature_tap(False)
    # both off: plain behaviour, the tap that the heads turned on included
    be.set_knn(None)
    assert not tap_is_on(be, lib)
    again = [t.cpu().numpy() for t in be.classify_detect(dev(frames[:32]), 7)]
    assert all(np.array_equal(a.view(np.uint8), b.view(np.uint8)) for a, b in zip(plain, again))
    assert not tap_is_on(be, lib)
    # a tap the caller turned on outlives both heads
    be.set_feature_tap(True)
    be.set_knn(bank)
    be.set_ood(model)
    be.set_knn(None)
    be.set_ood(None)
    assert features_of(be, frames[:3]).shape == (1, 3, 512)
    be.set_feature_tap(False)
    # ... and a tap a head turned on does not outlive the heads, whichever goes last
    be.set_ood(model)
    be.set_knn(bank)
    be.set_ood(None)
    be.classify(dev(frames[:3]))
    assert tap_is_on(be, lib)
    be.set_knn(None)
    assert not tap_is_on(be, lib)
    be.close()


def test_views_double_the_samples(lib, r18_b):
    frames = synth.synthetic_frames_u8(9, 32, 32, seed=18)
    be = Backend("resnet18_cifar", r18_b, max_batch=16, views=views.hflip())
    bank = be.fit_knn(dev(frames), k=3)
    be.set_knn(bank)
    got = numpy_of(be.classify_knn(dev(frames[:5])))
    ft = be.features().cpu().numpy()
    assert ft.shape == (2, 5, 512) and not np.array_equal(ft[0], ft[1])
    want = R.score(R.f32_to_bf16_bits(ft), bank.rows, 3, None, math.inf)
    assert same_records(records_of(got), R.records(want))
    be.close()


def test_vit_miniature(lib):
    vblob, _ = weights.make_synthetic_vit("vit_tiny", seed=3)
    frames = synth.synthetic_frames_u8(19, 64, 64, seed=19)
    be = Backend("vit_tiny", vblob, max_batch=20)
    plain = [t.cpu().numpy() for t in be.classify_detect(dev(frames))]
    bank = be.fit_knn(dev(frames[:15]), np.arange(15) % 4, k=2)
    assert (bank.D, bank.N) == (128, 15)
    be.set_knn(bank)
    got = numpy_of(be.classify_knn(dev(frames)))
    for name, want in zip(("label", "conf", "fail", "score"), plain):
        assert np.array_equal(got[name].view(np.uint8), want.view(np.uint8)), name
    bits = R.f32_to_bf16_bits(be.features().cpu().numpy())
    assert bits.shape == (1, 19, 128)
    assert same_records(records_of(got), R.records(R.score(bits, bank.rows, 2, bank.class_id, math.inf)))
    be.close()


def test_ensemble_refuses_the_bank_and_goes_on_working(lib, r18_b):
    blobs = [r18_b, weights.make_synthetic("resnet18_cifar", seed=2)[0]]
    frames = synth.synthetic_frames_u8(3, 32, 32, seed=13)
    be = Backend("resnet18_cifar", blobs, max_batch=4, ens_grouped_max=-1, chunk_a=2, chunk_b=2)
    before = [t.cpu().numpy() for t in be.classify_detect(dev(frames))]
    bank = KNNBank(unit_rows(np.random.default_rng(0), 7, 512), k=2)
    c = bank.to_c()
    assert be.lib.fav_set_knn(be._h, C.byref(c)) == 6 and b"ensemble" in be.lib.fav_last_error(be._h)
    with pytest.raises(_lib.FavError, match="UNSUPPORTED"):
        be.set_knn(bank)
    assert be.knn_bank is None
    after = [t.cpu().numpy() for t in be.classify_detect(dev(frames))]
    assert all(np.array_equal(a.view(np.uint8), b.view(np.uint8)) for a, b in zip(before, after))
    with pytest.raises(_lib.FavError, match="no k-NN bank"):
        be.classify_knn(dev(frames))
    be.close()


def test_a_workspace_above_the_limit_is_refused_with_the_numbers(lib):
    """max_batch = 1024 frames against 262144 rows: 1 GiB of similarities alone.  Refused on the host before anything is
    allocated; the handle stays as it was."""
    vblob, _ = weights.make_synthetic_vit("vit_tiny", seed=3)
    be = Backend("vit_tiny", vblob, max_batch=1024)
    rows = np.zeros((262144, 128), np.uint16)
    rows[:, 0] = 0x3F80                                                              # 1.0: unit rows
    with pytest.raises(_lib.FavError, match="max_batch=1024.*N=262144"):
        be.set_knn(KNNBank(rows, k=10))
    assert be.knn_bank is None
    be.classify(dev(synth.synthetic_frames_u8(2, 64, 64, seed=1)))
    assert not tap_is_on(be, lib)
    be.close()


# ---- the tap's ownership: on iff the caller asked for it or a head reads it -------------------------------------------------
def tap_heads():
    """(setter name, head) of the two heads that read the tap, each as small as its checks allow."""
    return (("set_knn", KNNBank(unit_rows(np.random.default_rng(0), 7, 512), k=2)),
            ("set_ood", OODModel(np.zeros(512), np.eye(2, 512), np.zeros((1, 2)), np.zeros(1))))


def tap_sizes(be, lib):
    """fav_get_features without a buffer -> (status, (S, n, D) as it reported them)."""
    s, n, d = C.c_int32(-1), C.c_int32(-1), C.c_int32(-1)
    st = lib.fav_get_features(be._h, None, C.byref(s), C.byref(n), C.byref(d), None)
    return st, (s.value, n.value, d.value)


def test_a_tap_the_caller_adopts_outlives_the_head_that_turned_it_on(lib, r18_b):
    frames = synth.synthetic_frames_u8(3, 32, 32, seed=21)
    be = Backend("resnet18_cifar", r18_b, max_batch=4)
    for setter, head in tap_heads():
        set_head = getattr(be, setter)
        set_head(head)                                                               # the head turns the tap on
        be.classify(dev(frames))
        assert tap_is_on(be, lib)
        be.set_feature_tap(True)                                                     # ... and the caller makes it their own
        set_head(None)
        assert tap_is_on(be, lib) and features_of(be, frames).shape == (1, 3, 512)
        be.set_feature_tap(False)
        be.classify(dev(frames))
        assert not tap_is_on(be, lib), setter
    be.close()


def test_the_tap_forgets_the_last_call_when_it_goes_on_and_at_no_other_time(lib, r18_b):
    frames = synth.synthetic_frames_u8(3, 32, 32, seed=22)
    (_, bank), (_, model) = tap_heads()
    be = Backend("resnet18_cifar", r18_b, max_batch=4)
    be.set_ood(model)
    be.classify(dev(frames))
    assert tap_sizes(be, lib) == (0, (1, 3, 512))
    be.set_knn(bank)                                                                 # a second head on a tap that is on
    assert tap_sizes(be, lib) == (0, (1, 3, 512))
    be.set_ood(None)
    assert tap_sizes(be, lib) == (0, (1, 3, 512))                                    # the bank still reads it
    be.set_knn(None)                                                                 # off with the last head ...
    assert tap_sizes(be, lib)[0] == 1 and "the feature tap is off" in lib.fav_last_error(be._h).decode()
    be.set_ood(model)                                                                # ... and on again: nothing to read yet
    assert tap_sizes(be, lib) == (1, (-1, -1, -1))
    assert "no classify call since the tap was turned on" in lib.fav_last_error(be._h).decode()
    be.classify(dev(frames[:2]))
    assert tap_sizes(be, lib) == (0, (1, 2, 512))
    be.set_feature_tap(True)                                                         # the caller adopts a tap that is on
    assert tap_sizes(be, lib) == (0, (1, 2, 512))
    be.set_ood(None)
    assert tap_sizes(be, lib) == (0, (1, 2, 512))
    be.close()
