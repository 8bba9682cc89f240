"""Feature-space OOD scoring on the device: fav_op_ood_score against tests/ood_ref.py, the feature tap against the oracle,
and the Backend methods end to end.

Everything here is an equality of bits.  The contract (include/fav.h beside fav_ood_record) fixes every product and every
sum, so a record must be the reference's dwords (a NaN counts as equal to any NaN).  The tap is checked through the layer
that reads it: for every sample, the oracle's bit-exact model of the production fc GEMM on the tapped features, plus the
bias, must be the logits fav_get_logits reports - which pins the rows, their order and their offsets in one comparison.

Shapes of the op: D in {16, 48, 2048, 4096}, k in {1, 3, 64, 257, 2048}, R in {1, 2, 33, 1000, 4096}, S in {1, 3}, n in
{1, 2, 3, 5, 67}.  The kernel runs 4, 2 or 1 frames a block (4 from n = 4, 2 from n = 2, fewer when x and g of that many
frames do not fit 64 KB of LDS: D = 4096 with k = 64), 1024 columns a block pass (k = 2048 and R = 4096 take several) and 64
lanes a wave; none of them divides 67, 5, 257, 33 or 1000.

The head has no global workspace (x and g live in LDS), so the sentinel check the issue asks for behind the g workspace has
nothing to guard; the sentinels behind records[n] are checked in every op call."""
import ctypes as C
import math

import numpy as np
import pytest

pytestmark = pytest.mark.gpu

torch = pytest.importorskip("torch")
import ood_ref as R  # noqa: E402
from failure_aware_vision_amd import Backend, _lib, synth, views, weights  # noqa: E402
from failure_aware_vision_amd.ood import OODModel  # noqa: E402
from oracle import fav_oracle as O  # noqa: E402

GUARD = 64
FILL = 0x5A


@pytest.fixture(scope="module")
def lib():
    assert torch.cuda.is_available(), "GPU tests need a MI355X"
    return _lib.load()


def dev(a):
    return torch.from_numpy(np.ascontiguousarray(a)).cuda()


def run_op(lib, feat_bits, mu, P, M, cls, labels, thr, rec_off=0, S=None, n=None, D=None, k=None, R_=None, null=(), feat_off=0):
    """fav_op_ood_score with P and M transposed here -> (status, records int32 [n, 4], guard bytes untouched?).  The records
    lie rec_off bytes behind a guard in a buffer filled with FILL.  S .. R_ override the sizes passed; null: arguments to
    pass as NULL; feat_off: the features start that many bf16 values into their buffer."""
    S0, n0, D0 = feat_bits.shape
    fbuf = torch.zeros(feat_bits.size + 16, dtype=torch.int16, device="cuda")
    assert fbuf.data_ptr() % 16 == 0
    fbuf[feat_off:feat_off + feat_bits.size] = dev(feat_bits.ravel().view(np.int16))
    t = dict(feat=fbuf[feat_off:], mu=dev(np.asarray(mu, np.float32)), Pt=dev(np.asarray(P, np.float32).T),
             Mt=dev(np.asarray(M, np.float32).T), cls=dev(np.asarray(cls, np.int32)),
             labels=None if labels is None else dev(np.asarray(labels, np.int32)))
    nbytes = 16 * n0
    buf = torch.full((GUARD + 16 + nbytes + GUARD,), FILL, dtype=torch.uint8, device="cuda")
    assert buf.data_ptr() % 16 == 0
    lo = GUARD + rec_off
    ptr = {name: (None if (v is None or name in null) else v.data_ptr()) for name, v in t.items()}
    st = lib.fav_op_ood_score(ptr["feat"], S0 if S is None else S, n0 if n is None else n, D0 if D is None else D,
                              P.shape[0] if k is None else k, M.shape[0] if R_ is None else R_, ptr["mu"], ptr["Pt"], ptr["Mt"],
                              ptr["cls"], ptr["labels"], thr, None if "records" in null else buf.data_ptr() + lo,
                              torch.cuda.current_stream().cuda_stream)
    torch.cuda.synchronize()
    host = buf.cpu().numpy()
    guards = bool((host[:lo] == FILL).all() and (host[lo + nbytes:] == FILL).all())
    return st, host[lo:lo + nbytes].copy().view(np.int32).reshape(n0, 4), guards


def problem(D, k, R_, S, n, seed=0):
    rng = np.random.default_rng(1000 * D + 10 * k + R_ + S + n + seed)
    feat = R.f32_to_bf16_bits(rng.standard_normal((S, n, D)).astype(np.float32))
    mu = (0.1 * rng.standard_normal(D)).astype(np.float32)
    P = (rng.standard_normal((k, D)) / np.sqrt(D)).astype(np.float32)
    M = rng.standard_normal((R_, k)).astype(np.float32)
    cls = rng.integers(-1, max(2, R_ // 2), R_).astype(np.int32)                     # duplicates and class-agnostic rows
    labels = rng.integers(0, max(2, R_ // 2) + 1, n).astype(np.int32)                 # some labels have no row
    return feat, mu, P, M, cls, labels


def same_records(got, want):
    return np.array_equal(R.canon_records(got), want)


# (D, k, R, S, n): every value beside an awkward partner
SHAPES = [(16, 1, 1, 1, 1), (16, 3, 2, 3, 5), (16, 257, 33, 3, 67), (48, 64, 33, 1, 67), (48, 257, 1000, 3, 5), (48, 3, 1000, 1, 3),
          (2048, 257, 33, 1, 67), (2048, 3, 1000, 3, 1), (2048, 64, 2, 1, 5), (2048, 1, 1, 3, 2), (4096, 64, 33, 1, 5),
          (16, 2048, 4096, 1, 2)]


@pytest.mark.parametrize("shape", SHAPES, ids=["x".join(map(str, s)) for s in SHAPES])
def test_op_bit_exact(lib, shape):
    D, k, R_, S, n = shape
    feat, mu, P, M, cls, labels = problem(*shape)
    want = R.score(feat, mu, P, M, cls, labels, 0.0)
    thr = float(np.median(want["min_dist"]))                                         # both outcomes of the flag, one frame at equality
    want = R.score(feat, mu, P, M, cls, labels, thr)
    assert n < 3 or 0 < want["ood"].sum() < n
    st, got, guards = run_op(lib, feat, mu, P, M, cls, labels, thr)
    assert st == 0 and guards
    assert same_records(got, R.records(want)), np.flatnonzero((R.canon_records(got) != R.records(want)).any(axis=1))[:8]
    st, got, guards = run_op(lib, feat, mu, P, M, cls, None, thr, rec_off=8)        # labels NULL; records 8-byte aligned only
    assert st == 0 and guards and same_records(got, R.records(R.score(feat, mu, P, M, cls, None, thr)))
    assert np.isnan(got[:, 2].view(np.float32)).all()


@pytest.mark.parametrize("feat_off", (1, 4, 7))
def test_op_features_off_a_16_byte_boundary(lib, feat_off):
    """The kernel loads a sample's eight neighbouring values as one 16-byte word only when the features are 16-byte aligned:
    2, 8 and 14 bytes off, it loads them one by one."""
    for shape in ((48, 3, 33, 3, 5), (16, 1, 2, 1, 1), (2048, 64, 33, 3, 3)):
        feat, mu, P, M, cls, labels = problem(*shape, seed=4)
        st, got, guards = run_op(lib, feat, mu, P, M, cls, labels, 10.0, feat_off=feat_off)
        assert st == 0 and guards and same_records(got, R.records(R.score(feat, mu, P, M, cls, labels, 10.0))), shape


def test_op_ties_labels_and_duplicate_classes(lib):
    feat, mu, P, M, _, _ = problem(48, 3, 6, 1, 5, seed=1)
    g, _ = R.distances(R.bf16_to_f32(feat), mu, P, M)
    M[1] = M[4] = g[2]                                                               # two identical rows, and frame 2 sits on both
    cls = np.array([7, 3, 9, 3, 8, 9], np.int32)                                     # classes 3 and 9 twice
    labels = np.array([9, 3, 8, 5, -1], np.int32)                                    # 5 and -1 have no row
    want = R.score(feat, mu, P, M, cls, labels, math.inf)
    assert want["min_dist"][2] == 0.0 and want["min_class"][2] == 3
    _, d = R.distances(R.bf16_to_f32(feat), mu, P, M)
    assert np.array_equal(d[:, 1], d[:, 4])
    assert want["label_dist"][0] == d[0, 2] and want["label_dist"][1] == d[1, 1] and want["label_dist"][2] == d[2, 4]
    assert np.isnan(want["label_dist"][3:]).all()
    st, got, guards = run_op(lib, feat, mu, P, M, cls, labels, math.inf)
    assert st == 0 and guards and same_records(got, R.records(want))
    assert not (got[:, 1] == 8).any() and got[:, 3].tolist() == [0] * 5              # row 4 never beats row 1; +inf flags nobody
    cls[3] = -1                                                                      # a label of -1 does match a class-agnostic row
    st, got, _ = run_op(lib, feat, mu, P, M, cls, labels, math.inf)
    assert st == 0 and same_records(got, R.records(R.score(feat, mu, P, M, cls, labels, math.inf)))
    assert got[4, 2].view(np.float32) == d[4, 3]


def test_op_non_finite_features_stay_in_their_frame(lib):
    feat, mu, P, M, cls, labels = problem(48, 64, 33, 3, 7, seed=2)
    clean = R.score(feat, mu, P, M, cls, labels, 50.0)
    feat[1, 2, 5] = 0x7F80                                                           # +inf in frame 2
    feat[0, 4, 40] = 0x7FC1                                                          # a NaN in frame 4
    feat[2, 5, 0] = 0xFF80                                                           # -inf and +inf in frame 5: NaN from the sum
    feat[0, 5, 0] = 0x7F80
    want = R.score(feat, mu, P, M, cls, labels, 50.0)
    assert want["min_class"][[2, 4, 5]].tolist() == [-1, -1, -1] and np.isinf(want["min_dist"][[2, 4, 5]]).all()
    assert want["ood"][[2, 4, 5]].tolist() == [1, 1, 1]
    st, got, guards = run_op(lib, feat, mu, P, M, cls, labels, 50.0)
    assert st == 0 and guards and same_records(got, R.records(want))
    keep = [0, 1, 3, 6]
    assert np.array_equal(R.canon_records(got)[keep], R.records(clean)[keep])        # the neighbours are unaffected


def test_op_thresholds(lib):
    feat, mu, P, M, cls, labels = problem(16, 3, 2, 1, 5, seed=3)
    d = R.score(feat, mu, P, M, cls, labels, 0.0)["min_dist"]
    for thr, flags in ((math.inf, [0] * 5), (-math.inf, [1] * 5), (float(d[3]), (~(d <= d[3])).astype(int).tolist()),
                       (float(np.nextafter(d[3], np.float32(0))), (~(d < d[3])).astype(int).tolist())):
        st, got, guards = run_op(lib, feat, mu, P, M, cls, labels, thr)
        assert st == 0 and guards and got[:, 3].tolist() == flags, thr
    assert run_op(lib, feat, mu, P, M, cls, labels, float(d[3]))[1][3, 3] == 0       # exactly at the threshold: not flagged


REFUSALS = [("feat", dict(null=("feat",)), "null"), ("mu", dict(null=("mu",)), "null"), ("Pt", dict(null=("Pt",)), "null"),
            ("Mt", dict(null=("Mt",)), "null"), ("class_id", dict(null=("cls",)), "null"), ("records", dict(null=("records",)), "null"),
            ("S 0", dict(S=0), "S=0"), ("S 4097", dict(S=4097), "S=4097"), ("n 0", dict(n=0), "n must"), ("n -1", dict(n=-1), "n must"),
            ("D 8", dict(D=8), "D=8"), ("D 24", dict(D=24), "D=24"), ("D 4112", dict(D=4112), "D=4112"),
            ("k 0", dict(k=0), "k=0"), ("k 2049", dict(k=2049), "k=2049"), ("R 0", dict(R_=0), "R=0"), ("R 4097", dict(R_=4097), "R=4097"),
            ("threshold NaN", dict(thr=math.nan), "threshold"), ("records + 4", dict(rec_off=4), "8-byte")]


@pytest.mark.parametrize("why,kw,text", REFUSALS, ids=[r[0] for r in REFUSALS])
def test_op_refusals_launch_nothing(lib, why, kw, text):
    feat, mu, P, M, cls, labels = problem(16, 3, 2, 1, 5)
    kw = dict(kw)
    thr = kw.pop("thr", 1.0)
    st, got, guards = run_op(lib, feat, mu, P, M, cls, labels, thr, **kw)
    msg = lib.fav_last_error(None).decode()
    assert st == 1 and "fav_op_ood_score" in msg and text in msg, (why, msg)
    assert guards and (got.view(np.uint8) == FILL).all()                             # the records are untouched


# ---- the tap ------------------------------------------------------------------------------------------------------------
@pytest.fixture(scope="module")
def r18_b(r18_blob):
    return r18_blob[0]


@pytest.fixture(scope="module")
def r18_second():
    return weights.make_synthetic("resnet18_cifar", seed=2)[0]


def fc_of(blob):
    model = O.parse_blob(blob)
    return model.layers[-1]


def logits_from_features(feat, fcs, members_of):
    """feat fp32 [S, n, D] -> the production fc GEMM (the oracle's bit-exact MFMA model) plus bias, [S, n, classes]; sample s
    runs through fcs[members_of(s)]."""
    out = []
    for s in range(feat.shape[0]):
        fc = fcs[members_of(s)]
        out.append(O.gemm_acc(feat[s], fc.w.reshape(fc.cout, -1), "mfma") + fc.b)
    return np.stack(out).astype(np.float32)


def tapped(be, frames, first=0):
    """classify with the tap on -> (labels, conf, logits, features), numpy."""
    lab, conf = be.classify(dev(frames), first)
    lg, ft = be.logits().cpu().numpy(), be.features().cpu().numpy()
    return lab.cpu().numpy(), conf.cpu().numpy(), lg, ft


def assert_fc_of_features_is_logits(be, frames, fcs, members_of=lambda s: 0, first=0):
    _, _, lg, ft = tapped(be, frames, first)
    assert ft.shape[:2] == lg.shape[:2] and ft.dtype == np.float32
    assert np.array_equal(R.bf16_to_f32(R.f32_to_bf16_bits(ft)).view(np.uint32), ft.view(np.uint32))   # bf16 values
    want = logits_from_features(ft, fcs, members_of)
    assert np.array_equal(want.view(np.uint32), lg.view(np.uint32))
    return lg, ft


def test_tap_single_pass_is_the_oracle_pool(lib, r18_b):
    frames = synth.synthetic_frames_u8(3, 32, 32, seed=11)
    be = Backend("resnet18_cifar", r18_b, max_batch=4)
    n = C.c_int32(-1)
    assert lib.fav_get_features(be._h, None, C.byref(n), None, None, None) == 1 and n.value == -1      # the tap is off
    assert b"tap is off" in lib.fav_last_error(be._h)
    lab0, conf0 = (t.cpu().numpy() for t in be.classify(dev(frames)))
    lg0 = be.logits().cpu().numpy()
    be.set_feature_tap(True)
    assert lib.fav_get_features(be._h, None, C.byref(n), None, None, None) == 1                        # on, but no call yet
    assert b"no classify call" in lib.fav_last_error(be._h)
    lab, conf, lg, ft = tapped(be, frames)
    assert ft.shape == (1, 3, 512)
    for a, b in ((lab0, lab), (conf0, conf), (lg0, lg)):                                              # the tap changes no result
        assert np.array_equal(a.view(np.uint8), b.view(np.uint8))
    model = O.parse_blob(r18_b)
    net = O.OracleNet(model, exact="mfma")
    act = net.stem(O.normalize_input(frames, O.ClassifyConfig().mean, O.inv_std32(O.ClassifyConfig().std)))
    for i in range(net.nb):
        act = net.block(i, act)
    assert np.array_equal(net.pool(act).view(np.uint32), ft[0].view(np.uint32))
    be.set_feature_tap(False)
    assert lib.fav_get_features(be._h, None, None, None, None, None) == 1
    lab1, conf1 = (t.cpu().numpy() for t in be.classify(dev(frames)))
    assert np.array_equal(lab1, lab0) and np.array_equal(conf1.view(np.uint32), conf0.view(np.uint32))
    be.close()


NB18 = 8
MC_MASKS = {"pooled site only": 1 << NB18, "all blocks and pooled": (1 << (NB18 + 1)) - 1, "all blocks": (1 << NB18) - 1,
            "last block": 1 << (NB18 - 1)}


@pytest.mark.parametrize("mask", MC_MASKS.values(), ids=list(MC_MASKS))
def test_tap_mc_dropout_chunks(r18_b, mask):
    """T = 3 samples of n frames through chunks of 4 virtual frames: 3 n is no multiple of 4, a chunk crosses samples."""
    fcs = [fc_of(r18_b)]
    be = Backend("resnet18_cifar", r18_b, max_batch=6, n_samples=3, site_mask=mask, dropout_p=0.2, seed=9, chunk_a=4, chunk_b=4)
    be.set_feature_tap(True)
    for n in (3, 5):
        frames = synth.synthetic_frames_u8(n, 32, 32, seed=12 + n)
        lg, ft = assert_fc_of_features_is_logits(be, frames, fcs, first=100)
        assert ft.shape == (3, n, 512)
        if mask >> NB18 & 1:                                                         # post-dropout: zeros, and samples that differ
            assert (ft == 0).mean() > 0.1 and not np.array_equal(ft[0], ft[1])
    be.set_feature_tap(False)
    lab0, conf0 = (t.cpu().numpy() for t in be.classify(dev(frames), 100))
    lg0 = be.logits().cpu().numpy()
    assert np.array_equal(lg0.view(np.uint32), lg.view(np.uint32))                   # tap on or off: the same logits
    be.close()


def test_tap_ensemble_one_stream_a_member(r18_b, r18_second):
    blobs = [r18_b, r18_second]
    fcs = [fc_of(b) for b in blobs]
    be = Backend("resnet18_cifar", blobs, max_batch=4, ens_grouped_max=-1, chunk_a=2, chunk_b=2)
    be.set_feature_tap(True)
    frames = synth.synthetic_frames_u8(3, 32, 32, seed=13)
    _, ft = assert_fc_of_features_is_logits(be, frames, fcs, members_of=lambda s: s)
    assert ft.shape == (2, 3, 512) and not np.array_equal(ft[0], ft[1])
    # an OOD model is refused on an ensemble; the tap goes on working
    m = OODModel(np.zeros(512), np.zeros((2, 512)), np.zeros((1, 2)), np.zeros(1))
    c = m.to_c()
    assert be.lib.fav_set_ood(be._h, C.byref(c)) == 6 and b"ensemble" in be.lib.fav_last_error(be._h)
    with pytest.raises(_lib.FavError, match="UNSUPPORTED"):
        be.set_ood(m)
    assert_fc_of_features_is_logits(be, frames, fcs, members_of=lambda s: s)
    be.close()


def test_tap_ensemble_grouped(r50_members):
    """Every op one launch over both members (the one-launch ImageNet stem is what a grouped call needs: ResNet-50)."""
    blobs = [b for b, _ in r50_members[:2]]
    fcs = [fc_of(b) for b in blobs]
    frames = synth.synthetic_frames_u8(3, 64, 64, seed=14)
    be = Backend("resnet50", blobs, in_hw=(64, 64), max_batch=4, chunk_a=2, chunk_b=2)
    be.set_feature_tap(True)
    lg, ft = assert_fc_of_features_is_logits(be, frames, fcs, members_of=lambda s: s)
    assert ft.shape == (2, 3, 2048) and not np.array_equal(ft[0], ft[1])
    be.close()
    lanes = Backend("resnet50", blobs, in_hw=(64, 64), max_batch=4, ens_grouped_max=-1)
    lanes.set_feature_tap(True)
    lg2, ft2 = assert_fc_of_features_is_logits(lanes, frames, fcs, members_of=lambda s: s)
    assert np.array_equal(ft.view(np.uint32), ft2.view(np.uint32)) and np.array_equal(lg.view(np.uint32), lg2.view(np.uint32))
    lanes.close()


@pytest.mark.parametrize("streams", (1, 2))
def test_tap_vit_stream_parts(streams):
    vblob, _ = weights.make_synthetic_vit("vit_tiny", seed=3)
    fcs = [fc_of(vblob)]
    be = Backend("vit_tiny", vblob, max_batch=20, vit_streams=streams)
    be.set_feature_tap(True)
    for n in (3, 19):                                                                # 19 >= 8 * 2: two parts of 9 and 10 frames
        frames = synth.synthetic_frames_u8(n, 64, 64, seed=15 + n)
        _, ft = assert_fc_of_features_is_logits(be, frames, fcs)
        assert ft.shape == (1, n, 128)
    be.close()


def test_tap_with_views(r18_b, r18_second):
    """hflip doubles S, and the samples come in the order of the logits: member m under view a at s = m * 2 + a."""
    frames = synth.synthetic_frames_u8(3, 32, 32, seed=16)
    be = Backend("resnet18_cifar", r18_b, max_batch=8, views=views.hflip())
    be.set_feature_tap(True)
    _, ft = assert_fc_of_features_is_logits(be, frames, [fc_of(r18_b)])
    assert ft.shape == (2, 3, 512) and not np.array_equal(ft[0], ft[1])
    be.set_views(None)
    _, flipped = assert_fc_of_features_is_logits(be, frames[:, :, ::-1], [fc_of(r18_b)])
    assert np.array_equal(flipped[0].view(np.uint32), ft[1].view(np.uint32))         # view 1 is the mirrored frame
    be.close()
    blobs = [r18_b, r18_second]
    ens = Backend("resnet18_cifar", blobs, max_batch=8, views=views.hflip())
    ens.set_feature_tap(True)
    _, ft = assert_fc_of_features_is_logits(ens, frames, [fc_of(b) for b in blobs], members_of=lambda s: s // 2)
    assert ft.shape == (4, 3, 512)
    ens.close()


# ---- end to end ---------------------------------------------------------------------------------------------------------
def test_backend_end_to_end(lib, r18_b):
    frames = synth.synthetic_frames_u8(64, 32, 32, seed=17)
    y = np.arange(64) % 10
    be = Backend("resnet18_cifar", r18_b, max_batch=32)
    plain = [t.cpu().numpy() for t in be.classify_detect(dev(frames[:32]), 7)]
    with pytest.raises(_lib.FavError, match="no OOD model"):
        be.classify_ood(dev(frames[:4]))
    model = be.fit_ood(dev(frames), y)                                               # two batches of 32
    assert (model.D, model.k, model.R) == (512, 512, 10) and model.class_id.tolist() == list(range(10))
    assert lib.fav_get_features(be._h, None, None, None, None, None) == 1            # fit_ood left the tap as it was: off
    model.check(512)
    wrong = OODModel(np.zeros(16), np.zeros((2, 16)), np.zeros((1, 2)), np.zeros(1))
    with pytest.raises(_lib.FavError, match="D=16"):
        be.set_ood(wrong)
    assert be.ood_model is None
    be.set_ood(model)
    with pytest.raises(_lib.FavError, match="clear it first"):                      # the model reads the tap
        be.set_feature_tap(False)
    out = be.classify_ood(dev(frames[:32]), 7)
    got = {k: v.cpu().numpy() for k, v in out.items()}
    for name, want in zip(("label", "conf", "fail", "score"), plain):               # fav_classify_ex, unchanged
        assert np.array_equal(got[name].view(np.uint8), want.view(np.uint8)), name
    # the records: the op on the tapped features, and the reference
    ft = be.features()
    assert tuple(ft.shape) == (1, 32, 512)
    bits = R.f32_to_bf16_bits(ft.cpu().numpy())
    want = R.score(bits, model.mu, model.P, model.M, model.class_id, got["label"], math.inf)
    rec = np.stack([got["min_dist"].view(np.int32), got["nearest_class"], got["label_dist"].view(np.int32), got["ood"]], axis=1)
    assert same_records(rec, R.records(want))
    st, op_rec, guards = run_op(lib, bits, model.mu, model.P, model.M, model.class_id, got["label"], math.inf)
    assert st == 0 and guards and np.array_equal(R.canon_records(op_rec), R.canon_records(rec))
    # label_dist is the distance to the class this call predicted
    _, d = R.distances(R.bf16_to_f32(bits), model.mu, model.P, model.M)
    assert np.array_equal(got["label_dist"], d[np.arange(32), got["label"]])
    assert got["ood"].sum() == 0                                                     # threshold +inf
    # numpy frames in -> numpy out, the same bits
    host = be.classify_ood(frames[:32], 7)
    assert isinstance(host["min_dist"], np.ndarray) and np.array_equal(host["min_dist"].view(np.int32), rec[:, 0])
    # calibration: the reference's threshold and the reference's flags
    all_d = np.concatenate([R.score(R.f32_to_bf16_bits(f), model.mu, model.P, model.M, model.class_id, None, 0.0)["min_dist"]
                            for f in (features_of(be, frames[:32]), features_of(be, frames[32:]))])
    thr = be.calibrate_ood(dev(frames), tpr=0.9)
    assert thr == OODModel.threshold_for_tpr(all_d, 0.9) == be.ood_model.threshold and np.mean(all_d <= thr) >= 0.9
    flags = np.concatenate([be.classify_ood(dev(frames[b:b + 32]))["ood"].cpu().numpy() for b in (0, 32)])
    assert np.array_equal(flags, (~(all_d <= np.float32(thr))).astype(np.int32)) and 0 < flags.sum() <= 6
    rep = be.ood_report(dev(frames[:32]), dev(255 - frames[32:]))
    assert set(rep) >= {"auroc", "fpr_at_tpr95"} and 0.0 <= rep["auroc"] <= 1.0 and rep["n_id"] == rep["n_ood"] == 32
    # off again: plain behaviour, the tap that the model turned on included
    be.set_ood(None)
    assert be.ood_model is None and lib.fav_get_features(be._h, None, None, None, None, None) == 1
    again = [t.cpu().numpy() for t in be.classify_detect(dev(frames[:32]), 7)]
    assert all(np.array_equal(a.view(np.uint8), b.view(np.uint8)) for a, b in zip(plain, again))
    with pytest.raises(_lib.FavError, match="no OOD model"):
        be.classify_ood(dev(frames[:4]))
    # a tap the caller turned on outlives a model
    be.set_feature_tap(True)
    be.set_ood(model)
    be.set_ood(None)
    assert features_of(be, frames[:3]).shape == (1, 3, 512)
    be.close()


def features_of(be, frames):
    be.classify(dev(frames))
    return be.features().cpu().numpy()
