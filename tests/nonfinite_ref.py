"""What NaN and the infinities must do between the stem and the logits, as a plain float64
reference, and the poisoned problems of tests/test_gpu_nonfinite.py (tests/test_nonfinite_host.py checks both on the CPU).

The reference answers with the CLASS of every output element - NaN, +inf, -inf or finite - not with its value: the class does
not depend on the summation order as long as no finite partial sum comes near the fp32 range, which the problems guarantee by
drawing their finite operands with |x| <= 4.  The finite elements are the existing oracle's business (bit for bit, on the clean
operands); this file only says which elements those are (`clean`).

A sum of products is classified by rule, not by running it: a product is NaN when an operand is NaN or it is inf x 0, +-inf when
one operand is infinite and the other is not zero; the sum is NaN when a product or the start value is NaN or infinities of both
signs meet, else the infinity present, else finite.  The counts behind the rule are products of 0 / 1 matrices, exact in any
summation order, so the rule scales to the largest launch; tests/test_nonfinite_host.py holds it against an element-by-element
float64 sum of the same products.

Rounding points are the contract's: the epilogue's value is an fp32, the one rounding to bf16 turns a finite fp32 above the bf16
range into +-inf."""
import struct
from collections import namedtuple

import numpy as np

from oracle import fav_oracle as O

NAN, PINF, NINF, FIN = 0, 1, 2, 3
CLASS_NAMES = ("nan", "+inf", "-inf", "finite")
QNAN_POS, QNAN_NEG = 0x7FC0, 0xFFC0            # bf16 quiet NaNs with a clear / a set sign bit
KINDS = ("+inf", "-inf", "nan", "nan_neg", "pair", "res", "round")
ROUND_BIAS = np.float32(3.4e38)                # finite in fp32 (max 3.4028e38), above the bf16 range (max 3.3895e38; the tie to 2^128 is at 3.3961e38)


def classes(v):
    """Class per element of a float array."""
    v = np.asarray(v)
    return np.where(np.isnan(v), NAN, np.where(v == np.inf, PINF, np.where(v == -np.inf, NINF, FIN))).astype(np.int8)


def from_bits(bits):
    """bf16 bit patterns (uint16) -> fp32, NaN payloads and signs as they are."""
    return (np.asarray(bits, np.uint16).astype(np.uint32) << 16).view(np.float32)


def to_bits(x):
    """fp32 holding bf16 values -> uint16 bit patterns (truncation: the low half is zero)."""
    x = np.ascontiguousarray(x, np.float32)
    assert not (x.view(np.uint32) & np.uint32(0xFFFF)).any(), "not bf16-representable"
    return (x.view(np.uint32) >> 16).astype(np.uint16)


def special(kind):
    """The fp32 value a value-kind puts into a tensor."""
    return {"+inf": np.float32(np.inf), "-inf": np.float32(-np.inf), "nan": from_bits([QNAN_POS])[0], "nan_neg": from_bits([QNAN_NEG])[0]}[kind]


def sign_set(v):
    return (np.ascontiguousarray(v, np.float32).view(np.uint32) >> 31).astype(bool)


# ---------------------------------------------------------------------------------------------------------------------
# sums of products
# ---------------------------------------------------------------------------------------------------------------------
def _ind(m):
    return m.astype(np.float64)


def dot_classes(a, w, start=None):
    """Class of start + a[M, K] @ w[N, K]^T per element, by the rule of the module docstring.  -> (classes [M, N],
    finite part [M, N] float64: the sum of the finite products, meaningful where the class is finite)."""
    a, w = np.asarray(a, np.float64), np.asarray(w, np.float64)
    rows = ~np.isfinite(a).all(axis=1)
    if np.isfinite(w).all() and not rows.all():
        # finite weights: only the rows of a that hold a special value can leave the finite class; the finite part of a large
        # product is taken in fp32 (its value only matters far from the fp32 range)
        big = a.shape[0] * a.shape[1] * w.shape[0] > 1 << 30
        af = np.where(rows[:, None], 0.0, a)
        fin = (af.astype(np.float32) @ w.astype(np.float32).T).astype(np.float64) if big else af @ w.T
        cls = np.full(fin.shape, FIN, np.int8)
        st = None if start is None else np.broadcast_to(np.asarray(start, np.float64), fin.shape)
        if rows.any():
            cls[rows], fin[rows] = dot_classes(a[rows], w, None if st is None else st[rows])
        if st is not None:                      # a finite sum takes the start value's class
            keep = ~rows
            sc = classes(st[keep])
            cls[keep] = sc
            fin[keep] = fin[keep] + np.where(sc == FIN, st[keep], 0.0)
        return cls, fin
    an, wn = np.isnan(a), np.isnan(w)
    ai, wi = np.isinf(a), np.isinf(w)
    az, wz = a == 0, w == 0
    ones_a, ones_w = np.ones_like(a), np.ones_like(w)
    n_nan = _ind(an) @ ones_w.T + ones_a @ _ind(wn).T + _ind(ai) @ _ind(wz).T + _ind(az) @ _ind(wi).T
    apos, aneg = (a > 0), (a < 0)                  # infinities included; NaN in neither
    wpos, wneg = (w > 0), (w < 0)
    n_pinf = (_ind(ai & apos) @ _ind(wpos).T + _ind(ai & aneg) @ _ind(wneg).T + _ind(apos & ~ai) @ _ind(wi & wpos).T
              + _ind(aneg & ~ai) @ _ind(wi & wneg).T)
    n_ninf = (_ind(ai & apos) @ _ind(wneg).T + _ind(ai & aneg) @ _ind(wpos).T + _ind(apos & ~ai) @ _ind(wi & wneg).T
              + _ind(aneg & ~ai) @ _ind(wi & wpos).T)
    fin = np.where(an | ai, 0.0, a) @ np.where(wn | wi, 0.0, w).T
    if start is not None:
        start = np.broadcast_to(np.asarray(start, np.float64), fin.shape)
        n_nan = n_nan + np.isnan(start)
        n_pinf = n_pinf + (start == np.inf)
        n_ninf = n_ninf + (start == -np.inf)
        fin = fin + np.where(np.isfinite(start), start, 0.0)
    cls = np.where((n_nan > 0) | ((n_pinf > 0) & (n_ninf > 0)), NAN, np.where(n_pinf > 0, PINF, np.where(n_ninf > 0, NINF, FIN)))
    return cls.astype(np.int8), fin


def with_class(cls, fin):
    """float64 values: the finite part where the class is finite, the special value elsewhere."""
    return np.where(cls == FIN, fin, np.where(cls == NAN, np.nan, np.where(cls == PINF, np.inf, -np.inf)))


def dot_values(a, w, start=None):
    return with_class(*dot_classes(a, w, start))


def im2col(x, kh, kw, stride, pad):
    """[n, H, W, C] -> ([n * Ho * Wo, kh * kw * C] float64 with zeros for the padding taps, Ho, Wo)."""
    n, H, W, Cc = x.shape
    ho, wo = (H + 2 * pad - kh) // stride + 1, (W + 2 * pad - kw) // stride + 1
    xp = np.zeros((n, H + 2 * pad, W + 2 * pad, Cc), np.float64)
    xp[:, pad:pad + H, pad:pad + W] = x
    cols = np.stack([xp[:, r:r + stride * ho:stride, s:s + stride * wo:stride] for r in range(kh) for s in range(kw)], axis=3)
    return cols.reshape(n * ho * wo, kh * kw * Cc), ho, wo


def epilogue_values(acc, bias, res=None, act=0, keep=None, scale=1.0, out_f32=False):
    """The contract's epilogue on float64 accumulator values, with the fp32 and bf16 range where the contract rounds:
    ((acc + bias) + residual) as fp32, ReLU (act 1: -inf -> +0, +inf and NaN stay) or GELU (act 2: O.gelu_exact, the
    device's sequence), the dropout select (a dropped NaN is 0), one rounding to bf16 unless the output is fp32."""
    with np.errstate(all="ignore"):
        y = np.asarray(acc, np.float64) + np.asarray(bias, np.float64)
        if res is not None:
            y = y + np.asarray(res, np.float64)
        y = y.astype(np.float32)
        if act == 1:
            y = np.where(y < 0, np.float32(0.0), y)
        elif act == 2:
            y = O.gelu_exact(y)
        if keep is not None:
            y = np.where(np.asarray(keep, bool).reshape(y.shape), (y.astype(np.float64) * float(scale)).astype(np.float32), np.float32(0.0))
        return y if out_f32 else O.bf16_round(y)


def conv_ref(x, w, b, res, kh, kw, stride, pad, act, keep=None, scale=1.0, out_f32=False):
    """-> (output classes, pre-activation classes), both [n, Ho, Wo, Cout]."""
    cols, ho, wo = im2col(x, kh, kw, stride, pad)
    acc = dot_values(cols, np.asarray(w).reshape(w.shape[0], -1))
    shape = (x.shape[0], ho, wo, w.shape[0])
    r = None if res is None else np.asarray(res).reshape(acc.shape)
    out = epilogue_values(acc, b, r, act, None if keep is None else np.asarray(keep).reshape(acc.shape), scale, out_f32)
    pre = epilogue_values(acc, b, r, 0, None, 1.0, True)
    return classes(out).reshape(shape), classes(pre).reshape(shape)


def linear_ref(x, w, b, res, act):
    """x [rows, K], w [N, K] -> classes [rows, N] of the bf16 output (act as in epilogue_values)."""
    return classes(epilogue_values(dot_values(x, w), b, res, act))


def maxpool_ref(x):
    """3x3 / 2 / pad 1: NaN when any tap inside the frame is NaN, else the maximum's class."""
    n, H, W, Cc = x.shape
    ho, wo = (H - 1) // 2 + 1, (W - 1) // 2 + 1
    xp = np.full((n, 2 * ho + 1, 2 * wo + 1, Cc), -np.inf, np.float64)
    xp[:, 1:1 + H, 1:1 + W] = x
    taps = np.stack([xp[:, r:r + 2 * ho:2, s:s + 2 * wo:2] for r in range(3) for s in range(3)])
    return classes(np.where(np.isnan(taps).any(axis=0), np.nan, np.where(np.isnan(taps), -np.inf, taps).max(axis=0)))


def avgpool_ref(x, keep=None, scale=1.0):
    """x [n, HW, C] -> classes [n, C]: the sum over HW (a sum of products with ones), x fp32(1 / HW), dropout, bf16."""
    n, HW, Cc = x.shape
    v = np.stack([dot_values(np.asarray(x[i], np.float64).T, np.ones((1, HW)))[:, 0] for i in range(n)])
    with np.errstate(all="ignore"):
        v = (v * (1.0 / HW)).astype(np.float32)
    return classes(epilogue_values(v, 0.0, None, 0, keep, scale))


def dropout_ref(x, keep, scale):
    """The entry dropout on bf16 values: a select, then x scale, one rounding."""
    return classes(epilogue_values(x, 0.0, None, 0, keep, scale))


def layernorm_ref(x):
    """x [rows, D]: a row with any non-finite value is NaN throughout (inf - mean is NaN or the variance is)."""
    bad = ~np.isfinite(x).all(axis=1)
    return np.where(bad[:, None], NAN, FIN).astype(np.int8) * np.ones(x.shape, np.int8)


def attention_ref(qkv, heads):
    """qkv [n, T, 3 D] -> classes [n, T, D] of softmax(Q K^T / 8) V per frame and head in float64 IEEE arithmetic: a query whose
    scores hold a NaN or +inf (inf - inf in the shifted exponent), or are -inf throughout, has NaN probabilities; a -inf score beside
    finite ones has probability 0; then the product with V by the rule (0 x inf is NaN)."""
    n, T, d3 = qkv.shape
    D = d3 // 3
    out = np.empty((n, T, D), np.int8)
    for i in range(n):
        for h in range(heads):
            q, k, v = (qkv[i, :, j * D + h * 64:j * D + (h + 1) * 64] for j in range(3))
            s = dot_values(q, k) / 8.0
            with np.errstate(all="ignore"):
                p = np.exp(s - s.max(axis=1, keepdims=True))        # NaN rows by IEEE: max propagates NaN, inf - inf is NaN
                p = p / p.sum(axis=1, keepdims=True)
            out[i, :, h * 64:(h + 1) * 64] = dot_classes(p, np.asarray(v, np.float64).T)[0]
    return out


# ---------------------------------------------------------------------------------------------------------------------
# poisoned problems
# ---------------------------------------------------------------------------------------------------------------------
def poison(p, kind, where):
    """Poisons the convolution / linear problem p (dict: x [n, H, W, C], w [N, kh, kw, C], b [N], res [n, Ho, Wo, N] or None;
    modified in place) with one kind at input pixel where = (frame, y, x) and returns the channels it used.
      +inf, -inf, nan, nan_neg   one channel of the pixel gets the value (weights of mixed sign: +inf gives both infinities)
      pair    +inf and -inf in two channels whose weights are forced positive: the NaN is made inside the op
      res     +inf in a channel with positive weights, and a residual of -inf in the even output channels of the pixel's
              central output: the NaN is made by the epilogue's add
      round   a bias of +-3.4e38 on output channels 1 and 2: finite in fp32, infinite after the one rounding to bf16
    The channel is a function of the kind, so several kinds can share one problem at different pixels."""
    f, y, xx = where
    x, w = p["x"], p["w"]
    ch = {"+inf": 3, "-inf": 4, "nan": 5, "nan_neg": 6, "pair": 8, "res": 10}
    if kind in ("+inf", "-inf", "nan", "nan_neg"):
        x[f, y, xx, ch[kind]] = special(kind)
        return (ch[kind],)
    if kind == "pair":
        x[f, y, xx, 8], x[f, y, xx, 9] = np.inf, -np.inf
        w[..., 8:10] = np.maximum(np.abs(w[..., 8:10]), np.float32(2.0 ** -6))
        return (8, 9)
    if kind == "res":
        assert p["res"] is not None
        x[f, y, xx, 10] = np.inf
        w[..., 10] = np.maximum(np.abs(w[..., 10]), np.float32(2.0 ** -6))
        kh, kw, stride, pad = p["geom"]
        oy, ox = (y + pad - kh // 2) // stride, (xx + pad - kw // 2) // stride        # the output whose window is centred here
        assert (oy * stride - pad + kh // 2, ox * stride - pad + kw // 2) == (y, xx), "res: the pixel is no window centre"
        p["res"][f, oy, ox, 0::2] = -np.inf
        return (10,)
    if kind == "round":
        p["b"][1], p["b"][2] = ROUND_BIAS, -ROUND_BIAS
        return ()
    raise ValueError(kind)


def clean_outputs(p, x_clean, b_clean, res_clean):
    """bool [n, Ho, Wo, N]: the outputs whose receptive field, bias and residual hold what the clean problem holds (compared as
    bits: a NaN differs from the finite value it replaced)."""
    kh, kw, stride, pad = p["geom"]
    touched = (np.ascontiguousarray(p["x"]).view(np.uint32) != np.ascontiguousarray(x_clean).view(np.uint32)).any(axis=3, keepdims=True)
    cols, ho, wo = im2col(touched, kh, kw, stride, pad)
    n, N = p["x"].shape[0], p["w"].shape[0]
    dirty = np.broadcast_to((cols.sum(axis=1) > 0).reshape(n, ho, wo, 1), (n, ho, wo, N)).copy()
    dirty |= (p["b"].view(np.uint32) != b_clean.view(np.uint32))[None, None, None, :]
    if p["res"] is not None:
        dirty |= p["res"].view(np.uint32) != res_clean.view(np.uint32)
    return ~dirty


def spread_pixels(n, H, W, count, kh=1, kw=1, stride=1):
    """`count` input pixels (frame, y, x) on even coordinates four apart: each is the centre of an output's window at stride 1 and 2
    (pad = k // 2), and the windows of two of them (up to 3 x 3) share no output."""
    assert kh <= 3 and kw <= 3 and stride <= 2
    def coords(L):
        return list(range(2, L - 1, 4)) or [0]
    spots = [(f, y, x) for f in range(n) for y in coords(H) for x in coords(W)]
    assert len(spots) >= count, f"{len(spots)} spots for {count} poisons in {n} x {H} x {W}"
    return spots[:count]


def poison_all(p, kinds):
    """Every kind of `kinds` at a pixel of its own (spread_pixels).  -> {kind: pixel}."""
    kh, kw, stride, pad = p["geom"]
    n, H, W, _ = p["x"].shape
    value_kinds = [k for k in kinds if k != "round"]
    spots = spread_pixels(n, H, W, len(value_kinds), kh, kw, stride)
    placed = {}
    for k, s in zip(value_kinds, spots):
        poison(p, k, s)
        placed[k] = s
    if "round" in kinds:
        poison(p, "round", (0, 0, 0))
        placed["round"] = None
    return placed


# ---------------------------------------------------------------------------------------------------------------------
# overflowing checkpoints
# ---------------------------------------------------------------------------------------------------------------------
def scale_layer(blob, layer, k):
    """The FAVW blob with 2^k multiplied into every bf16 weight of table row `layer` (weights.pack_blob's layout): k added to the
    exponent field, exact, zeros left alone.  Refuses a weight that would leave the normal range (the scaling would not be exact)."""
    magic, version, arch, ncls, nlayers = struct.unpack_from("<5I", blob, 0)
    assert magic == O.BLOB_MAGIC and 0 <= layer < nlayers
    cout, cin, kh, kw, stride, pad, _, _, w_off, b_off = struct.unpack_from("<8I2Q", blob, 32 + 48 * layer)
    assert kh > 0, "a vector row (LayerNorm, position table) holds fp32, not bf16 weights"
    count = cout * kh * kw * cin
    out = bytearray(blob)
    wts = np.frombuffer(out, np.uint16, count, w_off)            # a writable view into `out`
    e = ((wts >> 7) & 0xFF).astype(np.int32)
    nz = (wts & 0x7FFF) != 0
    assert not (nz & (e == 0)).any(), "a subnormal weight cannot be scaled through its exponent field"
    e2 = e + k
    assert ((e2[nz] >= 1) & (e2[nz] <= 254)).all(), "the scaled weights leave the normal bf16 range"
    wts[nz] = ((wts[nz] & 0x807F) | (e2[nz].astype(np.uint16) << 7)).astype(np.uint16)
    return bytes(out)


# ---------------------------------------------------------------------------------------------------------------------
# the convolution problems of tests/test_gpu_nonfinite.py: one per epilogue family, at the smallest shape that reaches its
# route (tests/test_gpu_conv_routes.py); 143 output pixels = two row tiles, the second one ragged
# ---------------------------------------------------------------------------------------------------------------------
ConvCase = namedtuple("ConvCase", "name n H W cin cout k stride pad res act out_f32 modes route")
MODE_NAME = ("bf16", "f32")
CONV_CASES = [
    ConvCase("staged-res", 1, 11, 13, 256, 320, 1, 1, 0, True, 1, 0, (0, 1), "conv_igemm<128,64,32,3,{m},epi0>"),
    ConvCase("register-nores", 1, 11, 13, 64, 192, 1, 1, 0, False, 1, 0, (0, 1), "conv_igemm<128,64,32,3,{m},epi1>"),
    ConvCase("register-norelu", 1, 11, 13, 64, 192, 1, 1, 0, False, 0, 0, (0, 1), "conv_igemm<128,64,32,3,{m},epi1>"),
    ConvCase("register-f32out-relu", 1, 11, 13, 64, 192, 1, 1, 0, False, 1, 1, (0, 1), "conv_igemm<128,64,32,3,{m},epi1>"),
    ConvCase("staged-f32out-relu", 1, 11, 13, 256, 320, 1, 1, 0, True, 1, 1, (0, 1), "conv_igemm<128,64,32,3,{m},epi0>"),
    ConvCase("register-gelu", 1, 11, 13, 64, 192, 1, 1, 0, False, 2, 0, (0, 1), "conv_igemm<128,64,32,3,{m},epi1,gelu>"),
    ConvCase("window-3x3-s2-res", 1, 21, 25, 64, 256, 3, 2, 1, True, 1, 0, (0, 1), "conv_igemm<128,128,64,2,{m},epi0>"),
    ConvCase("halo-32x64", 1, 32, 64, 64, 64, 3, 1, 1, False, 1, 0, (0, 1), "conv3x3_halo<64,64,256,3,{m}>"),
    ConvCase("proj-64x64", 1, 64, 64, 256, 512, 1, 1, 0, False, 0, 0, (0,), "proj<256,512,nw4>"),
    ConvCase("big-1x1-res-16384", 1, 128, 128, 512, 2048, 1, 1, 0, True, 1, 0, (0,), "conv_igemm<256,256,64,2,bf16,epi1,pp>"),
]


def conv_kinds(c):
    """The poison kinds that apply to a case: `res` needs a residual, `round` a bf16 output."""
    return tuple(k for k in KINDS if (k != "res" or c.res) and (k != "round" or not c.out_f32))


def conv_operands(c, rng):
    """x, w, bias, residual of a case: fp32 arrays of bf16 values (bias: any fp32), finite, |x| <= 4."""
    ho, wo = (c.H + 2 * c.pad - c.k) // c.stride + 1, (c.W + 2 * c.pad - c.k) // c.stride + 1
    kk = c.k * c.k * c.cin
    x = O.bf16_round(np.clip(rng.standard_normal((c.n, c.H, c.W, c.cin)) * np.exp2(rng.integers(-2, 2, (c.n, c.H, c.W, c.cin))), -4, 4).astype(np.float32))
    w = O.bf16_round((rng.standard_normal((c.cout, c.k, c.k, c.cin)) * np.sqrt(2.0 / kk)).astype(np.float32))
    b = (rng.standard_normal(c.cout) * 0.2).astype(np.float32)
    r = O.bf16_round(rng.standard_normal((c.n, ho, wo, c.cout)).astype(np.float32)) if c.res else None
    return x, w, b, r


def conv_problem(c, x, w, b, r):
    """The poisoned problem of a case from its finite operands: -> (p, clean) with p the poisoned operands (poison_all of
    conv_kinds(c); the weight channels forced positive belong to the clean problem too) and clean = dict(x, b, res, mask)."""
    p = dict(x=x.copy(), w=w.copy(), b=b.copy(), res=None if r is None else r.copy(), geom=(c.k, c.k, c.stride, c.pad))
    p["placed"] = poison_all(p, conv_kinds(c))
    clean = dict(x=x, b=b, res=r, mask=clean_outputs(p, x, b, r))
    return p, clean


def conv_case_ref(c, p):
    return conv_ref(p["x"], p["w"], p["b"], p["res"], c.k, c.k, c.stride, c.pad, c.act, out_f32=bool(c.out_f32))


def assert_covers(out_cls, pre_cls, clean_mask, act, what):
    """The condition that keeps a comparison from comparing nothing: the poisoned problem reaches every class - in its outputs,
    except that no -inf survives a ReLU (and the GELU sequence turns -inf into NaN), where the value in front of the activation
    is looked at - and at least half of its elements stay clean."""
    have = set(np.unique(out_cls).tolist())
    need = {NAN, PINF, FIN} | ({NINF} if act == 0 else set())
    assert need <= have, f"{what}: output classes {sorted(have)}"
    assert set(np.unique(pre_cls).tolist()) == {NAN, PINF, NINF, FIN}, f"{what}: classes in front of the activation"
    assert clean_mask.mean() >= 0.5, f"{what}: only {clean_mask.mean():.3f} of the elements are clean"
    assert (out_cls[clean_mask] == FIN).all(), f"{what}: a clean element is not finite"


# ---------------------------------------------------------------------------------------------------------------------
# the other ops' poisoned inputs.  Each builder returns (poisoned input, clean input); an op's clean outputs are those whose
# inputs are bit-equal in the two, which the tests work out from the op's own geometry.
# ---------------------------------------------------------------------------------------------------------------------
def finite_bf16(rng, shape, scale=1.0):
    return O.bf16_round(np.clip(rng.standard_normal(shape) * scale, -4, 4).astype(np.float32))


def pool_input(rng, n, H, W, Cc):
    """A max / average pool input [n, H, W, C], n >= 3: frame 0 clean; frame 1: +inf, -inf and the two NaNs in channels 0..3 of pixel
    (0, 0), and a channel (4) that is -inf throughout; frame 2: +inf and -inf in ONE channel (5) at two pixels, a NaN beside
    +inf in channel 6."""
    x = finite_bf16(rng, (n, H, W, Cc))
    p = x.copy()
    for ch, kind in enumerate(("+inf", "-inf", "nan", "nan_neg")):
        p[1, 0, 0, ch] = special(kind)
    p[1, :, :, 4] = -np.inf
    p[2, 0, 0, 5], p[2, H - 1, W - 1, 5] = np.inf, -np.inf
    p[2, 0, 0, 6], p[2, 0, W - 1, 6] = special("nan"), np.inf
    return p, x


def rows_input(rng, rows, D):
    """LayerNorm / dropout rows [rows, D], rows >= 6: rows 1, 3, 4, 5 hold +inf, NaN, -inf and the sign-set NaN in one element."""
    x = finite_bf16(rng, (rows, D), 2.0)
    p = x.copy()
    for r, kind in ((1, "+inf"), (3, "nan"), (4, "-inf"), (5, "nan_neg")):
        p[r, (7 * r) % D] = special(kind)
    return p, x


def attention_input(rng, n, T, heads):
    """qkv [n, T, 3 D], n >= 3, T >= 5, heads >= 2: frame 0 clean; frame 1: a NaN in Q of token 1, head 0 (that query alone), +inf in
    V of token 2, head 1 (one channel of every query); frame 2: -inf in K of token 0, head 0 (queries by the sign of their Q
    channel: NaN, or finite with probability 0), a sign-set NaN and -inf in V of tokens 1 and 3, head 1."""
    D = heads * 64
    x = finite_bf16(rng, (n, T, 3 * D), 1.2)
    p = x.copy()
    p[1, 1, 3] = special("nan")
    p[1, 2, 2 * D + 64 + 5] = np.inf
    p[2, 0, D + 1] = -np.inf
    p[2, 1, 2 * D + 64 + 7] = special("nan_neg")
    p[2, 3, 2 * D + 64 + 9] = -np.inf
    return p, x


def attention_clean(p, x, heads):
    """bool [n, T, D]: per frame and head, a query is clean when its Q row and the head's K and V are."""
    n, T, d3 = p.shape
    D = d3 // 3
    same = np.ascontiguousarray(p).view(np.uint32) == np.ascontiguousarray(x).view(np.uint32)
    out = np.empty((n, T, D), bool)
    for h in range(heads):
        q, k, v = (same[:, :, j * D + h * 64:j * D + (h + 1) * 64] for j in range(3))
        kv = k.all(axis=(1, 2)) & v.all(axis=(1, 2))
        out[:, :, h * 64:(h + 1) * 64] = (q.all(axis=2) & kv[:, None])[:, :, None]
    return out


def linear_problem(rng, rows, K, N, with_res):
    """A linear layer as a 1 x 1 convolution over a column of `rows` pixels: poison_all places its kinds on rows of their own."""
    c = ConvCase("linear", 1, rows, 1, K, N, 1, 1, 0, with_res, 0, 0, (0,), "")
    x, w, b, r = conv_operands(c, rng)
    p, clean = conv_problem(c, x, w, b, r)
    return p, clean


def tail_problem(rng, cmid, nred, has3x3, H, W, n):
    """The bottleneck tail's operands (tests/test_gpu_tail.py), finite; x poisoned by poison_all with the kinds of a residual launch
    except `round` (through the geometry of the tail's first convolution; `res` poisons conv_c's residual at the pixel).
    -> dict(x, x_clean, wb, bb, wc, bc, res, res_clean, wa, ba)."""
    cout = 4 * cmid
    t = dict(wb=None, bb=None, wa=None, ba=None)
    x = O.bf16_round(np.clip(np.maximum(rng.standard_normal((n, H, W, cmid)) * np.exp2(rng.integers(-2, 2, (n, H, W, cmid))), -0.2), -4, 4).astype(np.float32))
    if has3x3:
        t["wb"] = O.bf16_round((rng.standard_normal((cmid, 3, 3, cmid)) * np.sqrt(2.0 / (9 * cmid))).astype(np.float32))
        t["bb"] = (rng.standard_normal(cmid) * 0.2).astype(np.float32)
    t["wc"] = O.bf16_round((rng.standard_normal((cout, 1, 1, cmid)) * np.sqrt(1.0 / cmid)).astype(np.float32))
    t["bc"] = (rng.standard_normal(cout) * 0.2).astype(np.float32)
    res = O.bf16_round(np.maximum(rng.standard_normal((n, H, W, cout)), 0).astype(np.float32))
    if nred:
        t["wa"] = O.bf16_round((rng.standard_normal((nred, 1, 1, cout)) * np.sqrt(2.0 / cout)).astype(np.float32))
        t["ba"] = (rng.standard_normal(nred) * 0.2).astype(np.float32)
    first = "wb" if has3x3 else "wc"
    p = dict(x=x.copy(), w=t[first], b=np.zeros(t[first].shape[0], np.float32), res=res.copy(), geom=(3, 3, 1, 1) if has3x3 else (1, 1, 1, 0))
    p["placed"] = poison_all(p, tuple(k for k in KINDS if k != "round"))
    t.update(x=p["x"], x_clean=x, res=p["res"], res_clean=res, placed=p["placed"])
    return t


def tail_ref(t, keep=None, scale=1.0):
    """-> (classes of y, classes of t1n or None, clean pixels bool [n, H, W]) of the tail on t: conv_b (3x3, ReLU), conv_c (1x1 +
    residual, ReLU, dropout), conv_a (1x1, ReLU), chained through the reference's own values."""
    x = t["x"]
    n, H, W, cmid = x.shape
    dirty = (np.ascontiguousarray(x).view(np.uint32) != np.ascontiguousarray(t["x_clean"]).view(np.uint32)).any(axis=3)
    v = np.asarray(x, np.float64)
    if t["wb"] is not None:
        cols, _, _ = im2col(x, 3, 3, 1, 1)
        v = epilogue_values(dot_values(cols, t["wb"].reshape(cmid, -1)), t["bb"], None, 1).reshape(n, H, W, cmid)
        dcols, _, _ = im2col(dirty[..., None], 3, 3, 1, 1)
        dirty = (dcols.sum(axis=1) > 0).reshape(n, H, W)
    dirty = dirty | (t["res"].view(np.uint32) != t["res_clean"].view(np.uint32)).any(axis=3)
    cout = t["wc"].shape[0]
    y = epilogue_values(dot_values(v.reshape(-1, cmid), t["wc"].reshape(cout, cmid)), t["bc"], t["res"].reshape(-1, cout), 1,
                        None if keep is None else np.asarray(keep).reshape(-1, cout), scale)
    t1n = None
    if t["wa"] is not None:
        t1n = classes(epilogue_values(dot_values(y, t["wa"].reshape(-1, cout)), t["ba"], None, 1)).reshape(n, H, W, -1)
    return classes(y).reshape(n, H, W, cout), t1n, ~dirty
