"""The window-level drift test on the device: fav_op_drift_test against tests/drift_ref.py, and the Backend methods end to end.

Everything here is an equality of bits.  The contract (include/fav.h beside fav_drift_record) fixes every operation of the
window's rows, the similarity is the production GEMM accumulator, which the oracle models bit for bit, and from the quantised
distances on every figure is an exact integer: the record must be the reference's twelve dwords and perm_sums its P pairs.

The record and perm_sums lie between guard bytes, and the workspace is filled with a pattern: a kernel that read a distance
nobody wrote would sum 0x5A5A5A5A into its group."""
import ctypes as C

import numpy as np
import pytest

pytestmark = pytest.mark.gpu

torch = pytest.importorskip("torch")
import drift_ref as DR  # noqa: E402
import knn_ref as K  # noqa: E402
from failure_aware_vision_amd import Backend, _lib, synth, views, weights  # noqa: E402
from failure_aware_vision_amd.ood import DriftReference, KNNBank, OODModel, unpack_drift_record  # noqa: E402

GUARD = 64
FILL = 0x5A


@pytest.fixture(scope="module")
def lib():
    assert torch.cuda.is_available(), "GPU tests need a MI355X"
    return _lib.load()


def dev(a):
    return torch.from_numpy(np.ascontiguousarray(a)).cuda()


def run_op(lib, feat_bits, ref_bits, P, seed=0, alpha=0.05, rec_off=0, S=None, n=None, D=None, R=None, null=(), feat_off=0,
           ref_off=0, ws_off=0, ws_short=0, sums_off=0, sums=True, ws=None):
    """fav_op_drift_test -> (status, record int32 [12], perm_sums int64 [P, 2], guard bytes untouched?, workspace untouched?).
    The record lies rec_off bytes behind a guard in a buffer filled with FILL, perm_sums sums_off bytes, and so does the
    workspace, ws_off bytes in and ws_short bytes shorter than fav_drift_workspace_bytes asks.  S .. R override the sizes
    passed; null: arguments to pass as NULL; feat_off / ref_off: the arrays start that many bf16 values into their buffers;
    ws: a workspace to use again (so that a call runs on what the last one left)."""
    S0, n0, D0 = feat_bits.shape
    R0 = ref_bits.shape[0]
    fbuf = torch.zeros(feat_bits.size + 16, dtype=torch.int16, device="cuda")
    rbuf = torch.zeros(ref_bits.size + 16, dtype=torch.int16, device="cuda")
    assert fbuf.data_ptr() % 16 == 0 and rbuf.data_ptr() % 16 == 0
    fbuf[feat_off:feat_off + feat_bits.size] = dev(feat_bits.ravel().view(np.int16))
    rbuf[ref_off:ref_off + ref_bits.size] = dev(ref_bits.ravel().view(np.int16))
    need = lib.fav_drift_workspace_bytes(n0, D0, R0, P)
    assert need > 0
    if ws is None:
        ws = torch.full((256 + need + GUARD,), FILL, dtype=torch.uint8, device="cuda")
    assert ws.data_ptr() % 256 == 0 and ws.numel() == 256 + need + GUARD
    buf = torch.full((GUARD + 16 + 48 + GUARD,), FILL, dtype=torch.uint8, device="cuda")
    sbuf = torch.full((GUARD + 16 + 16 * P + GUARD,), FILL, dtype=torch.uint8, device="cuda")
    assert buf.data_ptr() % 16 == 0 and sbuf.data_ptr() % 16 == 0
    lo, slo = GUARD + rec_off, GUARD + sums_off
    ptr = dict(feat=fbuf[feat_off:].data_ptr(), ref=rbuf[ref_off:].data_ptr(), ws=ws.data_ptr() + ws_off, record=buf.data_ptr() + lo,
               sums=sbuf.data_ptr() + slo if sums else None)
    for name in null:
        ptr[name] = None
    st = lib.fav_op_drift_test(ptr["feat"], S0 if S is None else S, n0 if n is None else n, D0 if D is None else D, ptr["ref"],
                               R0 if R is None else R, P, seed, alpha, ptr["ws"], need - ws_short, ptr["record"], ptr["sums"],
                               torch.cuda.current_stream().cuda_stream)
    torch.cuda.synchronize()
    host, shost, ws_host = buf.cpu().numpy(), sbuf.cpu().numpy(), ws.cpu().numpy()
    guards = bool((host[:lo] == FILL).all() and (host[lo + 48:] == FILL).all() and (shost[:slo] == FILL).all() and
                  (shost[slo + 16 * P:] == FILL).all() and (ws_host[:ws_off] == FILL).all() and (ws_host[ws_off + need:] == FILL).all())
    return (st, host[lo:lo + 48].copy().view(np.int32), shost[slo:slo + 16 * P].copy().view(np.int64).reshape(P, 2), guards,
            bool((ws_host == FILL).all()))


def unit_rows(rng, N, D):
    x = rng.standard_normal((N, D))
    return K.f32_to_bf16_bits((x / np.linalg.norm(x, axis=1, keepdims=True)).astype(np.float32))


def problem(D, R, n, S, seed=0, shift=0.0):
    """Signed features around a common mean direction, so that distances spread; shift moves the window."""
    rng = np.random.default_rng(1000 * D + 10 * R + n + S + seed)
    base = rng.standard_normal(D)
    ref = unit_rows_of(base + rng.standard_normal((R, D)))
    feat = K.f32_to_bf16_bits((base + shift + rng.standard_normal((S, n, D))).astype(np.float32) * np.float32(3.0))
    return feat, ref


def unit_rows_of(x):
    return K.f32_to_bf16_bits((x / np.linalg.norm(x, axis=1, keepdims=True)).astype(np.float32))


def same_record(got, want):
    return np.array_equal(DR.canon_words(got), DR.record_words(want))


def check_against_reference(lib, feat, ref, P, seed=0, alpha=0.05, **kw):
    want, want_sums = DR.test(feat, ref, P, seed, alpha)
    st, got, sums, guards, _ = run_op(lib, feat, ref, P, seed, alpha, **kw)
    assert st == 0 and guards
    assert same_record(got, want), (unpack_drift_record(got), want)
    assert np.array_equal(sums, want_sums), np.flatnonzero((sums != want_sums).any(axis=1))[:8]
    return want, want_sums


# (D, R, n, S, P): the smallest legal problem; a pool of exactly one tile; one that crosses it; a pool of 128; S > 1; a pool
# several tiles wide; the production width
SHAPES = [(64, 2, 2, 1, 1), (64, 62, 2, 1, 16), (64, 63, 2, 1, 16), (64, 65, 63, 1, 33), (128, 64, 64, 3, 50), (256, 300, 70, 2, 64),
          (2048, 130, 33, 1, 8)]


@pytest.mark.parametrize("shape", SHAPES, ids=["x".join(map(str, s)) for s in SHAPES])
def test_op_bit_exact(lib, shape):
    D, R, n, S, P = shape
    feat, ref = problem(D, R, n, S)
    want, _ = check_against_reference(lib, feat, ref, P, seed=(7 << 32) | 3)
    assert want["n_degenerate"] == 0 and want["s_ab"] > 0
    check_against_reference(lib, feat, ref, P, seed=(7 << 32) | 3, rec_off=8, sums_off=8)      # 8-byte aligned only
    st, got, sums, guards, _ = run_op(lib, feat, ref, P, (7 << 32) | 3, sums=False)            # perm_sums is optional
    assert st == 0 and guards and same_record(got, want) and (sums.view(np.uint8) == FILL).all()


def test_op_largest_pool_the_reference_finishes_quickly(lib):
    """(D, R, n, S, P) = (128, 2048, 1024, 1, 12): the largest pool there is, 3072 rows - 48 tiles, a sort of 4096 keys with
    four keys a thread, three pool indices a thread in the compaction, 523776 pairs a group.  The reference takes about two
    seconds on a CPU (the oracle's model of the matrix pipe runs 3072 x 3072 x 128 products in a second), so the limit of ten
    is not what bounds the shape: the contract is."""
    feat, ref = problem(128, 2048, 1024, 1, seed=5, shift=0.05)
    check_against_reference(lib, feat, ref, 12, seed=99)
    # ... and a pool that ends inside a tile and a sort that is not full: 1280 + 3 rows, 2048 keys
    feat, ref = problem(64, 900, 383, 1, seed=5)
    check_against_reference(lib, feat, ref, 24, seed=98)


def test_op_at_the_limits_properties(lib):
    """R = 2048, n = 1024, P = 2: no reference at this size; the identity of step 5 ties the call to a small one."""
    D = 64
    feat, ref = problem(D, 2048, 1024, 1, seed=6)
    st, got, sums, guards, _ = run_op(lib, feat, ref, 2, seed=1)
    assert st == 0 and guards
    big = unpack_drift_record(got)
    st, got2, _, guards, _ = run_op(lib, feat[:, :2], ref, 2, seed=1)
    assert st == 0 and guards
    small = unpack_drift_record(got2)
    assert big["s_aa"] == small["s_aa"] > 0                                          # the reference's own pairs: the same pairs
    assert 0 < big["p_value"] <= 1 and big["n_degenerate"] == 0 and 0 <= big["n_exceed"] <= 2
    assert min(big["s_ab"], big["s_aa"], big["s_bb"]) >= 0 and (sums >= 0).all()
    top = (1 << 22) - 1
    assert big["s_ab"] <= 2048 * 1024 * top and big["s_bb"] <= 1024 * 1023 // 2 * top and (sums[:, 0] <= 1024 * 1023 // 2 * top).all()
    # every grouping splits the same total: S_AA of a permutation, through the identity, is non-negative as well
    total = big["s_ab"] + big["s_aa"] + big["s_bb"]
    assert (total - sums[:, 0] - sums[:, 1] >= 0).all()
    assert big["p_value"] == float(np.float32((1 + big["n_exceed"]) / 3))


def test_op_every_row_identical(lib):
    rng = np.random.default_rng(8)
    feat = np.repeat(K.f32_to_bf16_bits(rng.standard_normal((1, 128)).astype(np.float32)), 9, axis=0)[None]
    q_bits = K.f32_to_bf16_bits(K.query(feat)[0])
    ref = np.repeat(q_bits[:1], 70, axis=0)                                           # the reference is the window's q, 70 times
    assert (q_bits == q_bits[0]).all()
    P = 20
    want, _ = check_against_reference(lib, feat, ref, P)
    st, got, sums, guards, _ = run_op(lib, feat, ref, P)
    rec = unpack_drift_record(got)
    assert (rec["s_ab"], rec["s_aa"], rec["s_bb"], rec["n_exceed"], rec["p_value"], rec["drift"]) == (0, 0, 0, P, 1.0, False)
    assert got[0] == 0 and got[1] == 0 and not sums.any()                             # E = +0, bit for bit


def test_op_duplicated_rows_inside_and_across_the_groups(lib):
    feat, ref = problem(128, 40, 12, 1, seed=9)
    feat[0, 7] = feat[0, 2]                                                           # inside the window
    q_bits = K.f32_to_bf16_bits(K.query(feat)[0])
    ref[5] = ref[17] = ref[30]                                                        # inside the reference
    ref[8] = q_bits[3]                                                                # across: a reference row is a window row's q
    ref[31] = ref[0] = q_bits[11]
    pool = np.concatenate([K.bf16_to_f32(ref), K.query(feat)[0]])
    u = DR.quantise(DR.similarities(pool))
    for a, b in ((5, 17), (5, 30), (8, 40 + 3), (40 + 7, 40 + 2), (40 + 11, 31), (40 + 11, 0), (31, 0)):
        assert u[a, b] == 0 and np.array_equal(u[a], u[b])                            # distance exactly 0, and the same row
    check_against_reference(lib, feat, ref, 40, seed=2)


def test_op_near_and_far_windows(lib):
    """A window that copies reference rows is not flagged; one far away has no permutation that reaches it: p = 1 / 200."""
    rng = np.random.default_rng(10)
    D, R, n, P = 128, 100, 20, 199
    base = rng.standard_normal(D)
    ref = unit_rows_of(base + 0.5 * rng.standard_normal((R, D)))
    near = ref[rng.choice(R, n, replace=False)][None]
    far = unit_rows_of(-base + 0.5 * rng.standard_normal((n, D)))[None]
    want, _ = check_against_reference(lib, near, ref, P, alpha=0.01)
    assert want["drift"] == 0 and want["n_exceed"] > 2
    want, _ = check_against_reference(lib, far, ref, P, alpha=0.01)
    assert want["n_exceed"] == 0 and want["p_value"] == np.float32(1 / 200) and want["drift"] == 1 and want["statistic"] > 1.0


def test_op_alpha(lib):
    feat, ref = problem(64, 30, 10, 1, seed=11)
    P = 30
    p = DR.test(feat, ref, P, 4, 0.5)[0]["p_value"]
    assert 0 < p < 1
    below = float(np.nextafter(p, np.float32(0)))
    for alpha, flag in ((float(p), 1), (below, 0), (0.0, 0), (1.0, 1)):
        st, got, _, guards, _ = run_op(lib, feat, ref, P, 4, alpha)
        assert st == 0 and guards and got[10] == flag and got[8] == p.reshape(1).view(np.int32)[0], alpha
        assert same_record(got, DR.test(feat, ref, P, 4, alpha)[0])


def test_op_seed(lib):
    feat, ref = problem(64, 50, 14, 1, seed=12)
    a = run_op(lib, feat, ref, 25, seed=1)
    b = run_op(lib, feat, ref, 25, seed=1)
    c = run_op(lib, feat, ref, 25, seed=2)
    d = run_op(lib, feat, ref, 25, seed=1 << 32)                                      # the high word is part of the key
    assert a[0] == b[0] == c[0] == d[0] == 0
    assert np.array_equal(a[2], b[2]) and np.array_equal(a[1], b[1])
    assert not np.array_equal(a[2], c[2]) and not np.array_equal(a[2], d[2]) and not np.array_equal(c[2], d[2])
    assert np.array_equal(a[1][:8], c[1][:8])                                         # the observed sums do not depend on it
    for seed, got in ((2, c), (1 << 32, d)):
        assert np.array_equal(got[2], DR.test(feat, ref, 25, seed, 0.05)[1])


@pytest.mark.parametrize("where", ("first", "last"))
def test_op_degenerate_frame(lib, where):
    """The record of step 1, perm_sums untouched; a clean call on the same workspace afterwards is bit-exact."""
    feat, ref = problem(128, 70, 9, 2, seed=13)
    clean = feat.copy()
    row = 0 if where == "first" else 8
    feat[:, row, :] = 0
    feat[1, 4, 3] = 0x7FC1                                                            # and a NaN elsewhere: two frames
    want, want_sums = DR.test(feat, ref, 12, 0, 0.05)
    assert want_sums is None and want["n_degenerate"] == 2
    need = lib.fav_drift_workspace_bytes(9, 128, 70, 12)
    ws = torch.full((256 + need + GUARD,), FILL, dtype=torch.uint8, device="cuda")
    st, got, sums, guards, _ = run_op(lib, feat, ref, 12, ws=ws)
    assert st == 0 and guards and same_record(got, want)
    assert got.view(np.uint32).tolist() == [0, 0x7FF80000, 0, 0, 0, 0, 0, 0, 0x7FC00000, 0xFFFFFFFF, 1, 2]
    assert (sums.view(np.uint8) == FILL).all()                                        # the permutation kernel wrote nothing
    check_against_reference(lib, clean, ref, 12, ws=ws)


@pytest.mark.parametrize("feat_off", (1, 4, 7))
def test_op_features_off_a_16_byte_boundary(lib, feat_off):
    """The query kernel loads the features value by value: 2, 8 and 14 bytes off a 16-byte boundary is the same path; the case
    stays as a pin for a later wide-load path."""
    feat, ref = problem(64, 20, 5, 3, seed=14)
    check_against_reference(lib, feat, ref, 10, feat_off=feat_off)


REFUSALS = [("feat", dict(null=("feat",)), "null"), ("ref", dict(null=("ref",)), "null"), ("ws", dict(null=("ws",)), "null"),
            ("record", dict(null=("record",)), "null"),
            ("S 0", dict(S=0), "S=0"), ("S 4097", dict(S=4097), "S=4097"), ("n 0", dict(n=0), "n must"), ("n 1", dict(n=1), "n=1"),
            ("n 1025", dict(n=1025), "n=1025"), ("D 32", dict(D=32), "D=32"), ("D 96", dict(D=96), "D=96"),
            ("D 4160", dict(D=4160), "D=4160"), ("R 1", dict(R=1), "R=1"), ("R 2049", dict(R=2049), "R=2049"),
            ("P 0", dict(P=0), "n_perm=0"), ("P 10000", dict(P=10000), "n_perm=10000"),
            ("alpha NaN", dict(alpha=float("nan")), "alpha"), ("alpha -0.1", dict(alpha=-0.1), "alpha"),
            ("alpha 1.1", dict(alpha=1.1), "alpha"), ("workspace a byte short", dict(ws_short=1), "ws_bytes"),
            ("workspace + 128", dict(ws_off=128), "256-byte"), ("ref + 8", dict(ref_off=4), "16-byte"),
            ("record + 4", dict(rec_off=4), "8-byte"), ("perm_sums + 4", dict(sums_off=4), "perm_sums")]


@pytest.mark.parametrize("why,kw,text", REFUSALS, ids=[r[0] for r in REFUSALS])
def test_op_refusals_launch_nothing(lib, why, kw, text):
    feat, ref = problem(64, 17, 5, 1)
    kw = dict(kw)
    P = kw.pop("P", 6)
    if not 1 <= P <= 9999:                                                            # the buffers are sized for a legal P
        st = lib.fav_op_drift_test(1 << 12, 1, 5, 64, 1 << 12, 17, P, 0, 0.05, 1 << 12, 1 << 40, 1 << 12, None, None)
        msg = lib.fav_last_error(None).decode()
        assert st == 1 and "fav_op_drift_test" in msg and text in msg, (why, msg)
        return
    st, got, sums, guards, ws_untouched = run_op(lib, feat, ref, P, **kw)
    msg = lib.fav_last_error(None).decode()
    assert st == 1 and "fav_op_drift_test" in msg and text in msg, (why, msg)
    assert guards and (got.view(np.uint8) == FILL).all() and (sums.view(np.uint8) == FILL).all() and ws_untouched


# ---- end to end ---------------------------------------------------------------------------------------------------------
@pytest.fixture(scope="module")
def r18_b(r18_blob):
    return r18_blob[0]


def numpy_of(out):
    return {k: v.cpu().numpy() for k, v in out.items()}


def tap_is_on(be, lib):
    """after a classify call: fav_get_features answers with the sizes only while the tap is on."""
    return lib.fav_get_features(be._h, None, None, None, None, None) == 0


def test_backend_end_to_end(lib, r18_b):
    frames = synth.synthetic_frames_u8(96, 32, 32, seed=17)
    be = Backend("resnet18_cifar", r18_b, max_batch=32)
    plain = [t.cpu().numpy() for t in be.classify_detect(dev(frames[:32]), 7)]
    with pytest.raises(_lib.FavError, match="no drift reference"):
        be.classify_drift(dev(frames[:4]))
    ref = be.fit_drift(dev(frames[32:93]), n_perm=49, alpha=0.05, seed=3)             # two batches; 61 rows: a part tile
    assert (ref.D, ref.R, ref.n_perm, ref.alpha, ref.seed) == (512, 61, 49, 0.05, 3)
    assert not tap_is_on(be, lib)                                                    # fit_drift left the tap as it was: off
    ref.check(512)
    with pytest.raises(_lib.FavError, match="D=64"):
        be.set_drift(DriftReference(unit_rows(np.random.default_rng(0), 3, 64)))
    assert be.drift_reference is None
    be.set_drift(ref)
    with pytest.raises(_lib.FavError, match="clear it first"):                      # the reference reads the tap
        be.set_feature_tap(False)
    got = numpy_of(be.classify_drift(dev(frames[:32]), 7))
    for name, want in zip(("label", "conf", "fail", "score"), plain):               # fav_classify_ex, unchanged
        assert np.array_equal(got[name].view(np.uint8), want.view(np.uint8)), name
    # the record: the reference on the tapped features, and the op on them, which computes the reference's block itself
    ft = be.features()
    assert tuple(ft.shape) == (1, 32, 512)
    bits = K.f32_to_bf16_bits(ft.cpu().numpy())
    want, _ = DR.test(bits, ref.rows, 49, 3, 0.05)
    assert got["record"].shape == (12,) and same_record(got["record"], want)
    st, op_rec, _, guards, _ = run_op(lib, bits, ref.rows, 49, 3, 0.05)
    assert st == 0 and guards and np.array_equal(op_rec, got["record"])
    # a smaller window after a larger one, then the larger one again: nothing of a call outlives it
    small = numpy_of(be.classify_drift(dev(frames[:5]), 7))
    bits5 = K.f32_to_bf16_bits(be.features().cpu().numpy())
    assert same_record(small["record"], DR.test(bits5, ref.rows, 49, 3, 0.05)[0])
    assert np.array_equal(numpy_of(be.classify_drift(dev(frames[:32]), 7))["record"], got["record"])
    # numpy frames in -> numpy out, the same bits
    host = be.classify_drift(frames[:32], 7)
    assert isinstance(host["record"], np.ndarray) and np.array_equal(host["record"], got["record"])
    # one call is one window
    with pytest.raises(ValueError, match="frames_per_call=32"):
        be.classify_drift(dev(frames[:33]))
    with pytest.raises(_lib.FavError, match="n=1 is below 2"):
        be.classify_drift(dev(frames[:1]))
    # the report: held-out frames against their negatives
    rep = be.drift_report(dev(frames[:64]), dev(255 - frames[:64]), window=16)
    assert rep["id_p"].shape == rep["shifted_p"].shape == (4,) and rep["window"] == 16 and rep["alpha"] == 0.05
    assert 0.0 <= rep["false_alarm_rate"] <= 1.0 and 0.0 <= rep["detection_rate"] <= 1.0
    for key, src, rate in (("id_p", frames[:64], "false_alarm_rate"), ("shifted_p", 255 - frames[:64], "detection_rate")):
        recs = [unpack_drift_record(be.classify_drift(dev(src[b:b + 16]))["record"]) for b in range(0, 64, 16)]
        assert rep[key].tolist() == [np.float32(r["p_value"]) for r in recs] and rep[rate] == np.mean([r["drift"] for r in recs])
    with pytest.raises(ValueError, match="window"):
        be.drift_report(dev(frames[:64]), dev(frames[:64]), window=33)
    # a model, a bank and a reference together: each gives the records it gives alone
    y = np.arange(96) % 10
    be.set_knn(be.fit_knn(dev(frames[:61]), y[:61], k=5))
    be.set_ood(be.fit_ood(dev(frames), y))
    knn_rec = numpy_of(be.classify_knn(dev(frames[:32]), 7))
    ood_rec = numpy_of(be.classify_ood(dev(frames[:32]), 7))
    assert np.array_equal(numpy_of(be.classify_drift(dev(frames[:32]), 7))["record"], got["record"])
    be.set_drift(None)
    assert be.drift_reference is None and tap_is_on(be, lib)
    with pytest.raises(_lib.FavError, match="no drift reference"):
        be.classify_drift(dev(frames[:4]))
    for name in ("kth_dist", "nn_row"):
        assert np.array_equal(numpy_of(be.classify_knn(dev(frames[:32]), 7))[name], knn_rec[name], equal_nan=True)
    assert np.array_equal(numpy_of(be.classify_ood(dev(frames[:32]), 7))["min_dist"], ood_rec["min_dist"], equal_nan=True)
    # the tap rules with three readers: it goes off with the last of them, whichever that is
    be.set_drift(ref)
    be.set_knn(None)
    be.set_ood(None)
    be.classify(dev(frames[:3]))
    assert tap_is_on(be, lib)
    with pytest.raises(_lib.FavError, match="drift reference is set"):
        be.set_feature_tap(False)
    be.set_drift(ref.with_alpha(1.0))                                                # replaced: the tap stays, the new alpha holds
    assert tap_is_on(be, lib)
    again = numpy_of(be.classify_drift(dev(frames[:32]), 7))["record"]
    assert again[10] == 1 and np.array_equal(again[:10], got["record"][:10])
    be.set_drift(None)
    assert not tap_is_on(be, lib)
    after = [t.cpu().numpy() for t in be.classify_detect(dev(frames[:32]), 7)]
    assert all(np.array_equal(a.view(np.uint8), b.view(np.uint8)) for a, b in zip(plain, after))
    assert not tap_is_on(be, lib)
    # a tap the caller turned on outlives the reference
    be.set_feature_tap(True)
    be.set_drift(ref)
    be.set_drift(None)
    be.classify(dev(frames[:3]))
    assert tap_is_on(be, lib)
    be.set_feature_tap(False)
    # a rejected reference leaves the one in force
    be.set_drift(ref)
    bad = DriftReference(ref.rows.copy())
    bad.rows[0] = 0
    with pytest.raises(_lib.FavError, match="norm"):
        be.set_drift(bad)
    assert be.drift_reference is ref
    assert np.array_equal(numpy_of(be.classify_drift(dev(frames[:32]), 7))["record"], got["record"])
    be.close()


def test_views_double_the_samples(lib, r18_b):
    frames = synth.synthetic_frames_u8(30, 32, 32, seed=18)
    be = Backend("resnet18_cifar", r18_b, max_batch=16, views=views.hflip())
    ref = be.fit_drift(dev(frames[:20]), n_perm=19)
    be.set_drift(ref)
    assert be.frames_per_call == 8
    with pytest.raises(ValueError, match="frames_per_call=8"):
        be.classify_drift(dev(frames[20:29]))
    got = numpy_of(be.classify_drift(dev(frames[20:27])))
    ft = be.features().cpu().numpy()
    assert ft.shape == (2, 7, 512) and not np.array_equal(ft[0], ft[1])
    assert same_record(got["record"], DR.test(K.f32_to_bf16_bits(ft), ref.rows, 19, 0, 0.01)[0])
    be.close()


def test_vit_miniature(lib):
    vblob, _ = weights.make_synthetic_vit("vit_tiny", seed=3)
    frames = synth.synthetic_frames_u8(34, 64, 64, seed=19)
    be = Backend("vit_tiny", vblob, max_batch=20)
    plain = [t.cpu().numpy() for t in be.classify_detect(dev(frames[:19]))]
    ref = be.fit_drift(dev(frames[19:]), n_perm=29, seed=5)
    assert (ref.D, ref.R) == (128, 15)
    be.set_drift(ref)
    got = numpy_of(be.classify_drift(dev(frames[:19])))
    for name, want in zip(("label", "conf", "fail", "score"), plain):
        assert np.array_equal(got[name].view(np.uint8), want.view(np.uint8)), name
    bits = K.f32_to_bf16_bits(be.features().cpu().numpy())
    assert bits.shape == (1, 19, 128)
    assert same_record(got["record"], DR.test(bits, ref.rows, 29, 5, 0.01)[0])
    be.close()


def test_ensemble_refuses_the_reference_and_goes_on_working(lib, r18_b):
    blobs = [r18_b, weights.make_synthetic("resnet18_cifar", seed=2)[0]]
    frames = synth.synthetic_frames_u8(3, 32, 32, seed=13)
    be = Backend("resnet18_cifar", blobs, max_batch=4, ens_grouped_max=-1, chunk_a=2, chunk_b=2)
    before = [t.cpu().numpy() for t in be.classify_detect(dev(frames))]
    ref = DriftReference(unit_rows(np.random.default_rng(0), 7, 512))
    c = ref.to_c()
    assert be.lib.fav_set_drift(be._h, C.byref(c)) == 6 and b"ensemble" in be.lib.fav_last_error(be._h)
    with pytest.raises(_lib.FavError, match="UNSUPPORTED"):
        be.set_drift(ref)
    assert be.drift_reference is None
    after = [t.cpu().numpy() for t in be.classify_detect(dev(frames))]
    assert all(np.array_equal(a.view(np.uint8), b.view(np.uint8)) for a, b in zip(before, after))
    with pytest.raises(_lib.FavError, match="no drift reference"):
        be.classify_drift(dev(frames))
    be.close()


def test_max_batch_outside_the_window_sizes_is_refused_with_the_numbers(lib, r18_b):
    ref = DriftReference(unit_rows(np.random.default_rng(0), 7, 512))
    for mb in (1, 1025):
        be = Backend("resnet18_cifar", r18_b, max_batch=mb)
        with pytest.raises(_lib.FavError, match=rf"max_batch={mb} outside \[2, 1024\]"):
            be.set_drift(ref)
        assert be.drift_reference is None
        be.classify(dev(synth.synthetic_frames_u8(1, 32, 32, seed=1)))
        assert not tap_is_on(be, lib)
        be.close()


def test_the_tap_with_a_replaced_and_a_cleared_reference(lib, r18_b):
    """What the k-NN tests expect of a bank holds for a reference: a second head on a tap that is on does not forget the last
    call, the last head to go turns it off, and turning it on again has nothing to read."""
    frames = synth.synthetic_frames_u8(3, 32, 32, seed=22)
    ref = DriftReference(unit_rows(np.random.default_rng(0), 7, 512), n_perm=5)
    bank = KNNBank(unit_rows(np.random.default_rng(0), 7, 512), k=2)
    model = OODModel(np.zeros(512), np.eye(2, 512), np.zeros((1, 2)), np.zeros(1))

    def sizes():
        s, n, d = C.c_int32(-1), C.c_int32(-1), C.c_int32(-1)
        st = lib.fav_get_features(be._h, None, C.byref(s), C.byref(n), C.byref(d), None)
        return st, (s.value, n.value, d.value)

    be = Backend("resnet18_cifar", r18_b, max_batch=4)
    be.set_knn(bank)
    be.classify(dev(frames))
    assert sizes() == (0, (1, 3, 512))
    be.set_drift(ref)                                                                # a second head on a tap that is on
    assert sizes() == (0, (1, 3, 512))
    be.set_drift(ref.with_alpha(0.5))                                                # replaced
    assert sizes() == (0, (1, 3, 512))
    be.set_knn(None)
    assert sizes() == (0, (1, 3, 512))                                               # the reference still reads it
    be.set_drift(None)                                                               # off with the last head ...
    assert sizes()[0] == 1 and "the feature tap is off" in lib.fav_last_error(be._h).decode()
    be.set_drift(ref)                                                                # ... and on again: nothing to read yet
    assert sizes() == (1, (-1, -1, -1))
    be.set_ood(model)
    be.classify_drift(dev(frames[:2]))
    assert sizes() == (0, (1, 2, 512))
    be.set_feature_tap(True)                                                         # the caller adopts a tap that is on
    be.set_drift(None)
    be.set_ood(None)
    assert sizes() == (0, (1, 2, 512))
    be.close()
