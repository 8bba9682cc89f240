"""tests/nonfinite_ref.py on the CPU: the reference's classes on hand-made cases, its rule for sums of products against an
element-by-element float64 sum, and the condition that keeps tests/test_gpu_nonfinite.py from comparing nothing - every poisoned
problem used there reaches every class and leaves at least half of its elements clean.  A poisoned problem holds all its
poison kinds at pixels of their own, so "every class at least once" is asked of the problem: of its outputs, except that no
-inf survives a ReLU (and the GELU sequence turns -inf into NaN), where the values in front of the activation are looked at
(nonfinite_ref.assert_covers).  Then scale_layer: exact, zeros left alone, a round trip, and a blob fav_check_blob accepts."""
import ctypes as C

import numpy as np
import pytest

import nonfinite_ref as N
from failure_aware_vision_amd import _lib, weights
from oracle import fav_oracle as O

NAN, PINF, NINF, FIN = N.NAN, N.PINF, N.NINF, N.FIN
inf, nan = np.inf, np.nan


def test_classes_and_bit_helpers():
    v = np.array([nan, inf, -inf, 0.0, -0.0, 3e38, -1.0], np.float32)
    assert N.classes(v).tolist() == [NAN, PINF, NINF, FIN, FIN, FIN, FIN]
    both = N.from_bits([N.QNAN_POS, N.QNAN_NEG])
    assert np.isnan(both).all() and N.sign_set(both).tolist() == [False, True]
    assert N.to_bits(both).tolist() == [N.QNAN_POS, N.QNAN_NEG]
    assert N.sign_set(N.special("nan_neg")) and not N.sign_set(N.special("nan")) and N.special("+inf") == inf


def test_sum_of_products_by_hand():
    a = np.array([[1.0, 2.0, 0.0, -1.0]])
    w = np.array([[1.0, 1.0, 1.0, 1.0]])
    cases = [   # (a, w, class)
        (a, w, FIN),
        ([[inf, 1, 0, 0]], [[2, 1, 1, 1]], PINF), ([[inf, 1, 0, 0]], [[-2, 1, 1, 1]], NINF),
        ([[inf, 1, 0, 0]], [[0, 1, 1, 1]], NAN),                       # inf x 0
        ([[0, 1, 0, 0]], [[inf, 1, 1, 1]], NAN),                       # 0 x inf
        ([[inf, -inf, 0, 0]], [[1, 1, 1, 1]], NAN),                    # infinities of both signs meet
        ([[inf, -inf, 0, 0]], [[1, -1, 1, 1]], PINF),
        ([[nan, 1, 0, 0]], [[0, 1, 1, 1]], NAN), ([[1, 1, 0, 0]], [[nan, 1, 1, 1]], NAN),
        ([[-inf, 3, 0, 0]], [[-inf, 1, 1, 1]], PINF),
    ]
    for aa, ww, want in cases:
        cls, _ = N.dot_classes(np.array(aa, np.float64), np.array(ww, np.float64))
        assert cls.tolist() == [[want]], (aa, ww)
    # the start value takes part: +inf products under a start of -inf
    assert N.dot_classes(np.array([[inf, 0.0]]), np.array([[1.0, 1.0]]), start=np.array([[-inf]]))[0].tolist() == [[NAN]]
    assert N.dot_classes(np.array([[1.0, 0.0]]), np.array([[1.0, 1.0]]), start=np.array([[-inf]]))[0].tolist() == [[NINF]]
    cls, fin = N.dot_classes(a, w)
    assert fin[0, 0] == 2.0


def test_epilogue_by_hand():
    acc = np.array([[nan, inf, -inf, -2.0, inf, 1.0, 1.0, 1.0]])
    res = np.array([[0.0, 0.0, 0.0, 0.0, -inf, 0.0, 0.0, 0.0]])
    bias = np.array([0, 0, 0, 0, 0, 0, N.ROUND_BIAS, -N.ROUND_BIAS], np.float32)
    none = N.classes(N.epilogue_values(acc, bias, res, 0))
    assert none.tolist() == [[NAN, PINF, NINF, FIN, NAN, FIN, PINF, NINF]]           # the bf16 rounding makes +-inf of +-3.4e38
    assert N.classes(N.epilogue_values(acc, bias, res, 0, out_f32=True)).tolist() == [[NAN, PINF, NINF, FIN, NAN, FIN, FIN, FIN]]
    relu = N.epilogue_values(acc, bias, res, 1)
    assert N.classes(relu).tolist() == [[NAN, PINF, FIN, FIN, NAN, FIN, PINF, FIN]]  # ReLU: -inf -> +0, +inf and NaN stay
    assert relu[0, 2] == 0 and relu[0, 3] == 0 and relu[0, 7] == 0
    gelu = N.classes(N.epilogue_values(acc, bias, res, 2))
    assert gelu[0, :3].tolist() == [NAN, PINF, NAN]                                   # the sequence: -inf x Phi(-4.25) = -inf x 0
    keep = np.array([[0, 1, 1, 0, 0, 1, 1, 0]], bool)
    drop = N.epilogue_values(acc, bias, res, 0, keep, 1.25)
    assert N.classes(drop).tolist() == [[FIN, PINF, NINF, FIN, FIN, FIN, PINF, FIN]] and drop[0, 0] == 0 and drop[0, 4] == 0
    # the oracle's two epilogues agree with it, and with each other bit for bit (NaN = NaN)
    a32, r32 = acc.astype(np.float32), res.astype(np.float32)
    with np.errstate(all="ignore"):
        for relu_on, want in ((False, none), (True, N.classes(relu))):
            e1, e2 = O.epilogue(a32, bias, res=r32, relu=relu_on), O.epilogue_numpy(a32, bias, res=r32, relu=relu_on)
            assert np.array_equal(e1, e2, equal_nan=True) and N.classes(e1).tolist() == want.tolist()


def test_pools_layernorm_attention_by_hand():
    x = np.zeros((1, 3, 3, 4), np.float32)
    x[0, 0, 0] = [nan, inf, -inf, 1.0]
    x[0, 2, 2, 0] = 5.0
    mp = N.maxpool_ref(x)                     # 2 x 2 outputs; (0, 0) sees pixel (0, 0), (1, 1) does not
    assert mp[0, 0, 0].tolist() == [NAN, PINF, FIN, FIN] and mp[0, 1, 1].tolist() == [FIN] * 4
    allneg = np.full((1, 2, 2, 1), -inf, np.float32)
    assert (N.maxpool_ref(allneg) == NINF).all()
    ap = N.avgpool_ref(x.reshape(1, 9, 4))
    assert ap.tolist() == [[NAN, PINF, NINF, FIN]]
    both = x.reshape(1, 9, 4).copy()
    both[0, 5, 1] = -inf
    assert N.avgpool_ref(both)[0, 1] == NAN
    assert N.avgpool_ref(x.reshape(1, 9, 4), keep=np.array([[0, 1, 0, 1]], bool), scale=2.0).tolist() == [[FIN, PINF, FIN, FIN]]
    rows = np.ones((3, 8), np.float32)
    rows[1, 2] = inf
    assert N.layernorm_ref(rows).tolist() == [[FIN] * 8, [NAN] * 8, [FIN] * 8]
    rng = np.random.default_rng(0)
    p, clean = N.attention_input(rng, 4, 5, 2)
    cls = N.attention_ref(p, 2)
    assert (cls[0] == FIN).all() and (cls[3] == FIN).all()
    assert (cls[1, 1, :64] == NAN).all() and (cls[1, [0, 2, 3, 4], :64] == FIN).all()       # the NaN query alone
    assert (cls[1, :, 64 + 5] == PINF).all() and (np.delete(cls[1, :, 64:], 5, axis=1) == FIN).all()
    q1 = p[2, :, 1]                                                                        # the Q channel that meets K's -inf
    assert np.array_equal(cls[2, :, 0] == NAN, q1 <= 0) and (q1 > 0).any() and (q1 < 0).any()
    assert (cls[2, :, 64 + 7] == NAN).all() and (cls[2, :, 64 + 9] == NINF).all()
    assert N.attention_clean(p, clean, 2).mean() >= 0.5


def test_rule_equals_an_element_by_element_float64_sum():
    c = N.CONV_CASES[0]
    x, w, b, r = N.conv_operands(c, np.random.default_rng(3))
    p, _ = N.conv_problem(c, x, w, b, r)
    cols, _, _ = N.im2col(p["x"], c.k, c.k, c.stride, c.pad)
    w2 = p["w"].reshape(c.cout, -1).astype(np.float64)
    with np.errstate(all="ignore"):
        plain = np.einsum("mk,nk->mn", cols, w2)          # no BLAS: one IEEE multiply-add per product
    cls, fin = N.dot_classes(cols, w2)
    assert np.array_equal(cls, N.classes(plain))
    ok = cls == FIN
    assert np.allclose(fin[ok], plain[ok], rtol=1e-12, atol=1e-12)


@pytest.mark.parametrize("c", [k for k in N.CONV_CASES], ids=[k.name for k in N.CONV_CASES])
def test_conv_problems_reach_every_class(c):
    x, w, b, r = N.conv_operands(c, np.random.default_rng(sum(map(ord, c.name))))
    assert max(np.abs(x).max(), np.abs(w).max()) <= 4
    p, clean = N.conv_problem(c, x, w, b, r)
    assert set(p["placed"]) == set(N.conv_kinds(c))
    out, pre = N.conv_case_ref(c, p)
    N.assert_covers(out, pre, clean["mask"], c.act, c.name)
    # the repaired oracle gives the same classes in both of its models (the small cases; the large one runs on the GPU machine)
    if c.n * c.H * c.W <= 4096:
        for mode in ("mfma", True):
            acc = O.conv_acc_exact(p["x"], p["w"], c.k, c.k, c.stride, c.pad, mode=mode)
            assert np.array_equal(N.classes(acc + np.float32(0)), N.conv_ref(p["x"], p["w"], np.zeros(c.cout, np.float32), None, c.k, c.k, c.stride, c.pad, 0, out_f32=True)[0])


@pytest.mark.parametrize("cmid,nred,has3x3,H,W,n", [(64, 64, True, 7, 9, 37), (128, 0, False, 9, 11, 3), (256, 256, False, 5, 7, 9), (512, 0, False, 8, 10, 3)])
def test_tail_problems(cmid, nred, has3x3, H, W, n):
    t = N.tail_problem(np.random.default_rng(cmid + nred + H), cmid, nred, has3x3, H, W, n)
    ycls, t1cls, clean = N.tail_ref(t)
    have = set(np.unique(ycls).tolist())
    assert {NAN, FIN} <= have and (has3x3 or PINF in have) and clean.mean() >= 0.5
    assert (ycls[clean] == FIN).all() and (t1cls is None or (t1cls[clean] == FIN).all())


def test_other_problems_reach_every_class():
    rng = np.random.default_rng(1)
    every = {NAN, PINF, NINF, FIN}
    p, _ = N.pool_input(rng, 3, 5, 7, 16)
    assert set(np.unique(N.maxpool_ref(p)).tolist()) == every and set(np.unique(N.avgpool_ref(p.reshape(3, 35, 16))).tolist()) == every
    assert (N.maxpool_ref(p)[0] == FIN).all()
    p, x = N.rows_input(rng, 6, 128)
    assert (N.layernorm_ref(p) == NAN).all(axis=1).tolist() == [False, True, False, True, True, True]
    for T in (5, 197):
        p, x = N.attention_input(rng, 4, T, 2)
        cls, clean = N.attention_ref(p, 2), N.attention_clean(p, x, 2)
        assert set(np.unique(cls).tolist()) == every and clean.mean() >= 0.5 and (cls[clean] == FIN).all()
    for with_res in (False, True):
        p, clean = N.linear_problem(rng, 5505, 768, 768, with_res)
        x2, w2 = p["x"].reshape(5505, 768), p["w"].reshape(768, 768)
        r2 = None if not with_res else p["res"].reshape(5505, 768)
        for act in (0, 1, 2):
            N.assert_covers(N.linear_ref(x2, w2, p["b"], r2, act), N.linear_ref(x2, w2, p["b"], r2, 0), clean["mask"].reshape(5505, 768), act, "linear")


# ---------------------------------------------------------------------------------------------------------------------
# scale_layer
# ---------------------------------------------------------------------------------------------------------------------
@pytest.fixture(scope="module")
def r18_blob():
    return weights.make_synthetic("resnet18_cifar", seed=1)[0]


def test_scale_layer_is_exact_and_round_trips(r18_blob):
    m0 = O.parse_blob(r18_blob)
    up = N.scale_layer(r18_blob, 5, 100)
    m1 = O.parse_blob(up)
    assert np.array_equal(m1.layers[5].w.astype(np.float64), m0.layers[5].w.astype(np.float64) * 2.0 ** 100)
    assert np.isfinite(m1.layers[5].w).all() and np.abs(m1.layers[5].w).max() > 1e25
    for i, (a, b) in enumerate(zip(m0.layers, m1.layers)):
        assert np.array_equal(a.b, b.b) and (i == 5 or np.array_equal(a.w, b.w))
    assert N.scale_layer(up, 5, -100) == r18_blob
    # zeros stay zeros, of either sign
    z = bytearray(r18_blob)
    cout, cin, kh, kw, _, _, _, _, w_off, _ = __import__("struct").unpack_from("<8I2Q", r18_blob, 32 + 48 * 5)
    z[w_off:w_off + 4] = bytes([0x00, 0x00, 0x00, 0x80])                 # +0, -0
    zs = np.frombuffer(N.scale_layer(bytes(z), 5, 100), np.uint16, 2, w_off)
    assert zs.tolist() == [0x0000, 0x8000]
    with pytest.raises(AssertionError):
        N.scale_layer(r18_blob, 5, 200)                                   # would leave the bf16 range: refused, not wrapped


def test_scaled_blobs_pass_check_blob(r18_blob):
    lib = _lib.load()
    blobs = {"resnet18_cifar": r18_blob, "vit_tiny": weights.make_synthetic_vit("vit_tiny", seed=3)[0]}
    for arch, (a, b) in (("resnet18_cifar", (5, 6)), ("vit_tiny", (6, 7))):
        for blob in (N.scale_layer(N.scale_layer(blobs[arch], a, 100), b, 100), N.scale_layer(blobs[arch], a, 40)):
            buf = (C.c_char * len(blob)).from_buffer_copy(blob)
            assert lib.fav_check_blob(buf, len(blob), None, 0) == 0
    with pytest.raises(AssertionError):
        N.scale_layer(blobs["vit_tiny"], 2, 1)                            # a LayerNorm row holds fp32 vectors
