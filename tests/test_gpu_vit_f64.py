"""The ViT-B/16 path (BASELINE configs[4]) against float64 arithmetic that knows nothing of the kernels.

tests/test_gpu_vit.py checks the kernels bit for bit against oracle/, which restates their polynomial exp and GELU and their attention
key order - a mistake made in both places passes there.  Here every assertion compares the device with tests/vit_ref.py or plain
float64 arithmetic written from the definitions: the whole encoder at its real size and batch shapes, and the attention, LayerNorm and
GELU kernels at the inputs where they go wrong.  Every bound is derived below, and each test also shows that its bound rejects a
plausibly wrong reference (tanh GELU, LayerNorm eps 1e-5, softmax without the 1/8, temperature 1.0) computed from the same device
output."""
import ctypes as C
import math

import numpy as np
import pytest

pytestmark = pytest.mark.gpu

torch = pytest.importorskip("torch")
from conftest import note  # noqa: E402
from failure_aware_vision_amd import Backend, _lib, synth, weights  # noqa: E402
import vit_ref  # noqa: E402


@pytest.fixture(scope="module")
def lib():
    return _lib.load()


def bf16_values(x):
    """float array -> float32 array of the nearest bf16 values (round to nearest even)."""
    return torch.from_numpy(np.ascontiguousarray(x, np.float32)).to(torch.bfloat16).float().numpy()


def half_ulp_bf16(v):
    """Half a bf16 step at |v| (an upper bound of the rounding error of a value of that magnitude)."""
    a = torch.clamp(v.abs(), min=2.0 ** -126)
    return torch.exp2(torch.floor(torch.log2(a)) - 8)


# ---------------------------------------------------------------------------------------------------------------------------------
# a. the encoder end to end at 224x224 - both math modes, three batch shapes
# ---------------------------------------------------------------------------------------------------------------------------------
# Measured on an MI355X over the 64 frames, both math modes: rel. RMS <= 0.0082, max abs <= 0.191 at a logit spread of ~5, entropy
# confidence within 0.0073, pred_entropy within 0.050 nats.  The bounds are ~2x that; temperature 1.0 instead of 1.5 moves the
# confidences by up to 0.31.
E2E_REL_RMS, E2E_MAX_ABS, E2E_CONF, E2E_GAP = 0.02, 0.4, 0.015, 0.01
E2E_N = 64


@pytest.fixture(scope="module")
def e2e_case():
    """ViT-B/16 seed 1, 64 frames at 224x224 alternating clean / Gaussian-corrupted (severity 3), and their float64 logits."""
    blob, _ = weights.make_synthetic_vit("vit_b16", seed=1)
    u8 = synth.synthetic_frames_u8(E2E_N // 2, 224, 224, seed=21)
    frames = np.empty((E2E_N, 224, 224, 3), np.float32)
    frames[0::2] = u8.astype(np.float32) * np.float32(1.0 / 255.0)
    frames[1::2] = synth.gaussian_noise_f32(u8, 3, seed=3)
    ref = vit_ref.classify(blob, frames, device="cuda")
    return blob, torch.from_numpy(frames).cuda(), ref


@pytest.fixture(scope="module")
def vit_backends(e2e_case):
    blob = e2e_case[0]
    made = {}

    def get(math_mode):
        if math_mode not in made:
            made[math_mode] = Backend("vit_b16", blob, max_batch=E2E_N, math_mode=math_mode, temperature=1.5, conf_kind="entropy")
        return made[math_mode]
    yield get
    for be in made.values():
        be.close()


# Dispatch (fav.hip classify_on_stream / run_vit / launch_conv): 2 frames run on one stream, every GEMM on 128-row tiles; 37 and 64
# frames split into two streams (18 + 19, 32 + 32), whose GEMMs take the chained stream-K kernel in bf16 mode and the 256 x 256 tile
# in f32_exact mode; 37 leaves ragged last tiles everywhere.
@pytest.mark.parametrize("n", [2, 37, 64])
@pytest.mark.parametrize("math_mode", ["bf16", "f32_exact"])
def test_vit_b16_vs_float64(e2e_case, vit_backends, math_mode, n):
    _, frames, ref_all = e2e_case
    be = vit_backends(math_mode)
    labels, conf = be.classify(frames[:n])
    lg = be.logits().cpu().numpy()
    assert lg.shape == (1, n, 1000)
    lg = lg[0].astype(np.float64)
    ref = ref_all[:n]
    hd = vit_ref.head(ref, 1.5)
    err = lg - ref
    rel_rms = np.sqrt(np.mean(err ** 2)) / ref.std()
    conf = conf.cpu().numpy().astype(np.float64)
    conf_err = np.abs(conf - hd["confidence"]).max()
    clear = hd["gap"] > E2E_GAP
    labels = labels.cpu().numpy()
    unc = be.classify_uncertainty(frames[:n])
    ent_err = np.abs(unc["pred_entropy"].cpu().numpy().astype(np.float64) - hd["entropy"]).max()
    note(f"vit_b16 {math_mode} n={n} vs float64: rel. RMS {rel_rms:.4f} (bound {E2E_REL_RMS}), max abs {np.abs(err).max():.3f} "
         f"(bound {E2E_MAX_ABS}), confidence {conf_err:.4f} (bound {E2E_CONF}), pred_entropy {ent_err:.4f} nats "
         f"(bound {E2E_CONF * math.log(1000):.4f}), labels {int((labels == hd['label']).sum())} / {n} ({int(clear.sum())} clear)")
    assert rel_rms < E2E_REL_RMS
    assert np.abs(err).max() < E2E_MAX_ABS
    assert clear.sum() >= n // 2
    assert np.array_equal(labels[clear], hd["label"][clear])
    assert conf_err < E2E_CONF
    # fav_classify_uncertainty, one sample: pred_entropy = H(pbar) in nats, the same bound as 1 - H / ln C
    assert ent_err < E2E_CONF * math.log(1000)
    assert np.array_equal(unc["label"].cpu().numpy()[clear], hd["label"][clear])
    # negative control: the confidence bound rejects a head that forgot the temperature
    assert np.abs(conf - vit_ref.head(ref, 1.0)["confidence"]).max() > E2E_CONF


# ---------------------------------------------------------------------------------------------------------------------------------
# b. attention (fav_op_attention) against softmax(Q K^T / 8) V in float64
# ---------------------------------------------------------------------------------------------------------------------------------
# Bound per output element: |out - ref| <= c * sum_k p_k |v_k| + tiny.  The inputs are bf16, the scores exact to fp32 rounding
# (relative 2^-24 per term of q.k: ~1e-4 in p at std 16), the exponential relative 2.9e-6; what remains is two bf16 roundings:
# of every p_k (relative <= 2^-8, so <= 2^-8 sum p_k |v_k| after the second product) and of the output (<= 2^-8 |out| <=
# 2^-8 sum p_k |v_k|).  c = 2^-6 is twice their sum; measured worst 2^-7.24 in both modes.
ATTN_C, ATTN_TINY = 2.0 ** -6, 1e-7
ATTN_GUARD = 64           # guard rows of qkv on each side
OUT_GUARD = 4096          # guard elements of the output on each side
QKV_GUARD_VALUE = 30000.0
OUT_GUARD_VALUE = 1234.0


def attention_qkv(n_kinds, T, heads, seed):
    """[7, T, 3D] bf16 values, one row type per frame: scores of std ~1.2^2, 4^2, 8^2, 16^2 (16: nearly one-hot rows), keys all
    equal (uniform softmax), one dominant key, V = 0."""
    rng = np.random.default_rng(seed)
    D = heads * 64
    qkv = np.empty((n_kinds, T, 3 * D), np.float64)
    for f, std in enumerate((1.2, 4.0, 8.0, 16.0)):
        qkv[f] = rng.standard_normal((T, 3 * D)) * std
    qkv[4] = rng.standard_normal((T, 3 * D)) * 4.0
    qkv[4, :, D:2 * D] = qkv[4, :1, D:2 * D]                                     # every key equal: p = 1 / T
    qkv[5] = rng.standard_normal((T, 3 * D))
    qkv[5, :, :D] = np.abs(qkv[5, :, :D])                                        # q > 0 ...
    qkv[5, T // 2, D:2 * D] = 2.0                                                # ... so key T / 2 scores ~2 sum |q| / 8 ~ 13 above the rest
    qkv[6] = rng.standard_normal((T, 3 * D)) * 4.0
    qkv[6, :, 2 * D:] = 0.0                                                      # V = 0: the output is exactly 0
    return bf16_values(qkv)


def attention_f64(qkv, heads, scale=0.125):
    """-> (softmax(Q K^T * scale) V, softmax(Q K^T * scale) |V|), float64 [n, T, D]."""
    n, T, d3 = qkv.shape
    q, k, v = qkv.double().reshape(n, T, 3, heads, 64).permute(2, 0, 3, 1, 4)
    p = vit_ref.attention_probs(q, k, scale)
    back = lambda t: t.transpose(1, 2).reshape(n, T, d3 // 3)
    return back(torch.matmul(p, v)), back(torch.matmul(p, v.abs()))


def attention_violation(out, qkv, heads, scale=0.125):
    """max over elements of |out - ref| / (c sum p|v| + tiny): <= 1 within the bound."""
    ref, mass = attention_f64(qkv, heads, scale)
    return float(((out.double() - ref).abs() / (ATTN_C * mass + ATTN_TINY)).max())


ATTENTION_CASES = [(1, 1), (16, 2), (17, 3), (32, 1), (33, 2), (196, 4), (197, 12), (208, 2), (224, 3), (256, 12)]   # T, heads
# the instantiation each T must take (fav_op_last_route), production mode and validation mode: the kernel compiled for 13 key
# tiles of 16 up to 208 tokens - without masking when there are exactly 13 (T 193..208) - and the one for 16 above
ATTENTION_ROUTES = {
    1: ("attention<bf16,13>", "attention<f32,13>"), 16: ("attention<bf16,13>", "attention<f32,13>"),
    17: ("attention<bf16,13>", "attention<f32,13>"), 32: ("attention<bf16,13>", "attention<f32,13>"),
    33: ("attention<bf16,13>", "attention<f32,13>"), 196: ("attention<bf16,13,full>", "attention<f32,13>"),
    197: ("attention<bf16,13,full>", "attention<f32,13>"), 208: ("attention<bf16,13,full>", "attention<f32,13>"),
    224: ("attention<bf16,16>", "attention<f32,16>"), 256: ("attention<bf16,16>", "attention<f32,16>"),
}


def attention_route(T, mode):
    return ATTENTION_ROUTES[T][mode]


@pytest.mark.parametrize("T,heads", ATTENTION_CASES)
@pytest.mark.parametrize("mode", [0, 1])
def test_attention_vs_float64(lib, T, heads, mode):
    n = 7
    D = heads * 64
    qkv = torch.from_numpy(attention_qkv(n, T, heads, seed=T * 16 + heads)).cuda()
    rows = n * T
    # qkv with guard rows of large finite values in front of the first and behind the last token, the output with guard elements
    # on both sides: a key or query past a frame's last token, or a store outside n * T * D, shows
    big = torch.full(((rows + 2 * ATTN_GUARD) * 3 * D,), QKV_GUARD_VALUE, dtype=torch.bfloat16, device="cuda")
    big.view(-1, 3 * D)[1::2] *= -1
    big.view(-1, 3 * D)[ATTN_GUARD:ATTN_GUARD + rows] = qkv.reshape(rows, 3 * D).to(torch.bfloat16)
    obig = torch.full((rows * D + 2 * OUT_GUARD,), OUT_GUARD_VALUE, dtype=torch.bfloat16, device="cuda")
    _lib.check(lib.fav_op_attention(big.data_ptr() + ATTN_GUARD * 3 * D * 2, obig.data_ptr() + OUT_GUARD * 2, n, T, D, heads,
                                    mode, None))
    assert _lib.last_route() == attention_route(T, mode)
    tight_in = qkv.to(torch.bfloat16).contiguous()
    tight = torch.empty((n, T, D), dtype=torch.bfloat16, device="cuda")
    _lib.check(lib.fav_op_attention(tight_in.data_ptr(), tight.data_ptr(), n, T, D, heads, mode, None))
    torch.cuda.synchronize()
    assert bool((obig[:OUT_GUARD] == OUT_GUARD_VALUE).all()) and bool((obig[-OUT_GUARD:] == OUT_GUARD_VALUE).all()), \
        "attention wrote outside n * T * D"
    out = obig[OUT_GUARD:-OUT_GUARD].view(n, T, D)
    assert torch.equal(out.view(torch.int16), tight.view(torch.int16)), "guard rows around the tokens changed the output"
    out = out.float()
    assert bool(torch.isfinite(out).all())
    worst = attention_violation(out, qkv, heads)
    per_kind = [attention_violation(out[f:f + 1], qkv[f:f + 1], heads) for f in range(n)]
    note(f"attention mode {mode} T={T} heads={heads}: worst |err| / sum p|v| = 2^{math.log2(max(worst, 1e-30) * ATTN_C):.2f} "
         f"(bound 2^-6); by row type {' '.join(f'{w:.3f}' for w in per_kind)} of the bound")
    assert worst <= 1.0
    assert bool((out[6] == 0).all())                                            # V = 0
    if T > 1:
        # negative control: softmax(Q K^T) V without the 1/8 is rejected (rows of random scores)
        assert attention_violation(out[:4], qkv[:4], heads, scale=1.0) > 1.0


# ---------------------------------------------------------------------------------------------------------------------------------
# c. LayerNorm (fav_op_layernorm) against float64 with eps 1e-6
# ---------------------------------------------------------------------------------------------------------------------------------
# y = t + b with t = (x - m) rstd g.  In fp32 the mean carries a relative error of at most ~(D/64 + 7) 2^-24 (sequential lane sums,
# a 6-level butterfly, one division), which x - m passes on as an absolute error of that times |m|: in the output, a multiple of
# 2^-24 |m| rstd |g|.  The variance and rstd carry ~(D/64 + 10) 2^-24 relative, scale and shift a few 2^-24 more: <= 2^-19 (|t| +
# |b|) at D <= 1024.  The bf16 rounding of the result adds half a step, <= 2^-8 |y|.  So
#     |y_dev - y| <= 2^-8 |y| + 2^-16 (|t| + |m| rstd |g| + |b|)
# with 8x headroom on the fp32 part; only the terms' magnitudes enter, never the (possibly cancelled) result's alone.  The rounding
# half is attained (measured worst ratio 0.992, a half step at the bottom of a binade); eps 1e-5 exceeds the bound >= 400x.
LN_EPS = 1e-6
LN_KINDS = ("tiny spread", "unit", "nearly constant", "offset 100", "constant", "offset 1000", "spread 1e4", "mixed scales")


def layernorm_rows(rows, D, seed):
    """[rows, D] bf16 values cycling through LN_KINDS."""
    rng = np.random.default_rng(seed)
    x = rng.standard_normal((rows, D))
    kind = np.arange(rows) % len(LN_KINDS)
    x[kind == 0] *= 1e-3                                                         # var ~1e-6 = eps: rstd depends on eps
    x[kind == 2] = 1.5
    x[kind == 2, rng.integers(0, D)] = 1.5 + 2.0 ** -7                           # one bf16 step off a constant: var << eps
    x[kind == 3] += 100.0
    x[kind == 4] = rng.standard_normal((int((kind == 4).sum()), 1)) * 3          # exactly constant: var = 0, rstd = eps^-1/2
    x[kind == 5] = x[kind == 5] * 3 + 1000.0
    x[kind == 6] *= 1e4
    x[kind == 7] *= np.exp2(rng.integers(-12, 12, ((kind == 7).sum(), D)))
    return bf16_values(x)


def layernorm_f64(x, g, b, eps=LN_EPS):
    """-> (y, t, |m| rstd |g|), float64."""
    x = x.double()
    m = x.mean(-1, keepdim=True)
    rstd = 1.0 / torch.sqrt(((x - m) ** 2).mean(-1, keepdim=True) + eps)
    t = (x - m) * rstd * g
    return t + b, t, m.abs() * rstd * g.abs()


def layernorm_violation(y, x, g, b, eps=LN_EPS):
    """Per row: max over the row of |y_dev - y| / bound."""
    g, b = g.double(), b.double()
    ref, t, mterm = layernorm_f64(x, g, b, eps)
    bound = 2.0 ** -8 * ref.abs() + 2.0 ** -16 * (t.abs() + mterm + b.abs()) + 1e-30
    return ((y.double() - ref).abs() / bound).amax(-1)


# rows straddle the switch from one row per wave to four at 4096 (fav.hip launch_layernorm)
@pytest.mark.parametrize("rows,D,stride_mul", [(r, d, 1) for r in (1, 3, 4095, 4096, 4097, 20000) for d in (4, 128, 768, 1024)] +
                         [(4097, 768, 2), (9, 1024, 3), (5000, 4, 5)])
def test_layernorm_vs_float64(lib, rows, D, stride_mul):
    rng = np.random.default_rng(rows * 7 + D)
    x = torch.from_numpy(layernorm_rows(rows, D, seed=rows + D)).cuda()
    g = torch.from_numpy((1 + 0.1 * rng.standard_normal(D)).astype(np.float32)).cuda()
    b = torch.from_numpy((0.05 * rng.standard_normal(D)).astype(np.float32)).cuda()
    xs = torch.full((rows, stride_mul * D), -5e4, dtype=torch.bfloat16, device="cuda")   # what lies between strided rows
    xs[:, :D] = x.to(torch.bfloat16)
    guard = 1024
    ybig = torch.full((rows * D + guard,), OUT_GUARD_VALUE, dtype=torch.bfloat16, device="cuda")
    _lib.check(lib.fav_op_layernorm(xs.data_ptr(), stride_mul * D, g.data_ptr(), b.data_ptr(), ybig.data_ptr(), rows, D,
                                    C.c_float(LN_EPS), None))
    torch.cuda.synchronize()
    assert bool((ybig[-guard:] == OUT_GUARD_VALUE).all()), "layernorm wrote past rows * D"
    y = ybig[:-guard].view(rows, D).float()
    viol = layernorm_violation(y, x, g, b)
    kind = torch.arange(rows, device="cuda") % len(LN_KINDS)
    by_kind = {LN_KINDS[k]: float(viol[kind == k].max()) for k in range(min(rows, len(LN_KINDS)))}
    note(f"layernorm rows={rows} D={D} ldx={stride_mul}D: worst |err| / bound {float(viol.max()):.3f}; "
         + ", ".join(f"{k} {v:.3f}" for k, v in by_kind.items()))
    assert float(viol.max()) <= 1.0
    assert torch.equal(y[kind == 4], b.expand(int((kind == 4).sum()), D).to(torch.bfloat16).float())   # constant rows: exactly beta
    # negative control: eps 1e-5 instead of 1e-6 is rejected (the tiny-spread rows, and the nearly constant ones)
    assert float(layernorm_violation(y, x, g, b, eps=1e-5).max()) > 1.0


# ---------------------------------------------------------------------------------------------------------------------------------
# d. the GELU epilogue, swept densely
# ---------------------------------------------------------------------------------------------------------------------------------
# A linear layer with identity weights (bf16 I, one nonzero product per output) hands the epilogue exactly x, plus an fp32 bias per
# channel, so the pre-activation is any bf16 value or an fp32 value that is none.  Contract (fav_kernels.hpp, fav_gelu):
# |x Phi_poly(x) - GELU(x)| <= 8.6e-5; fp32 evaluation adds a few ulp of |x| (2^-21 |x|), the bf16 rounding of the output half a
# step.  Measured worst ratio 0.998 (x = 2.03: the polynomial's 8.5e-5 moves the result across a bf16 midpoint), on every path and
# in both modes.  The tanh form is 4.7e-4 away from the erf form, 4.7x the bound at x = -3.03 where |GELU(x)| is small.
GELU_CONTRACT = 8.6e-5


def gelu_inputs(rows, ch):
    """[rows, ch] bf16 values and fp32 bias [ch]: channels < ch/2 sweep every bf16 value in [-8, 8] plus +-1e4, 0 and -0 with no bias;
    channels >= ch/2 hold +-4.25 (the clamp) and a coarse subset of the sweep, with biases k 2^-21 for k in [-ch/4, ch/4): the fp32
    neighbours of the clamp point."""
    bits = np.arange(1 << 16, dtype=np.uint32)
    allv = (bits << 16).view(np.float32)
    sweep = allv[np.isfinite(allv) & (np.abs(allv) <= 8)]
    sweep = np.concatenate([sweep, np.float32([1e4, -1e4, 0.0, -0.0])])
    h = ch // 2
    assert rows * h >= sweep.size
    x = np.empty((rows, ch), np.float32)
    x[:, :h] = np.resize(sweep, rows * h).reshape(rows, h)
    side = np.concatenate([np.float32([4.25, -4.25] * 8), sweep[::97]])
    x[:, h:] = np.resize(side, rows)[:, None]
    bias = np.zeros(ch, np.float32)
    bias[h:] = (np.arange(ch - h) - (ch - h) // 2).astype(np.float32) * np.float32(2.0 ** -21)
    return bf16_values(x), bias


def gelu_violation(y, x, bias, form=vit_ref.gelu):
    """max of |y_dev - GELU(x + b)| / (contract + half a bf16 step + 2^-21 |x + b|)."""
    pre = x.double() + bias.double()
    ref = form(pre)
    bound = GELU_CONTRACT + half_ulp_bf16(torch.maximum(y.double().abs(), ref.abs())) + 2.0 ** -21 * pre.abs()
    return float(((y.double() - ref).abs() / bound).max())


def _conv_gelu(lib, x, bias, math_mode):
    rows, ch = x.shape
    xd = x.to(torch.bfloat16).contiguous()
    w = torch.eye(ch, device="cuda").to(torch.bfloat16).contiguous()         # [Cout][1][1][Cin]
    y = torch.empty((rows, ch), dtype=torch.bfloat16, device="cuda")
    nd = _lib.FavDropoutDesc(-1, 0, 1.0, 0, 0, 1, 0)
    d = _lib.FavConvDesc(xd.data_ptr(), w.data_ptr(), bias.data_ptr(), None, y.data_ptr(), 1, rows, 1, ch, ch, 1, 1, 1, 0, 2, 0,
                         math_mode, nd)
    _lib.check(lib.fav_op_conv2d(C.byref(d), None))
    torch.cuda.synchronize()
    return y.float()


def _streamk_gelu(lib, x, bias):
    rows, K = x.shape
    xd = x.to(torch.bfloat16).contiguous()
    w = torch.eye(K, device="cuda").to(torch.bfloat16).contiguous()          # [N][K]
    y = torch.empty((rows, K), dtype=torch.bfloat16, device="cuda")
    ld = _lib.FavLinearDesc(xd.data_ptr(), w.data_ptr(), bias.data_ptr(), None, y.data_ptr(), rows, K, K, 2)
    _lib.check(lib.fav_op_linear_streamk(C.byref(ld), None))
    torch.cuda.synchronize()
    return y.float()


# path, rows, channels: the 128-row tile (K = 256 < 512 keeps conv_big off), the 256 x 256 tile (1x1, K = Cout = 768, M = 43776:
# (M / 256) (Cout / 256) = 513 >= 512, fav.hip conv_big), and the chained stream-K GEMM (12608 x 768: 594 tiles of 128 x 128)
@pytest.mark.parametrize("path,rows,ch,math_mode", [
    ("conv 128-row tile", 512, 256, 0), ("conv 128-row tile", 512, 256, 1),
    ("conv 256x256 tile", 43776, 768, 0), ("conv 256x256 tile", 43776, 768, 1),
    ("stream-K", 12608, 768, 0)])
def test_gelu_epilogue_vs_float64(lib, path, rows, ch, math_mode):
    xn, bn = gelu_inputs(rows, ch)
    x, bias = torch.from_numpy(xn).cuda(), torch.from_numpy(bn).cuda()
    y = _streamk_gelu(lib, x, bias) if path == "stream-K" else _conv_gelu(lib, x, bias, math_mode)
    worst = gelu_violation(y, x, bias)
    pre = x.double() + bias.double()
    err = (y.double() - vit_ref.gelu(pre)).abs()
    note(f"gelu {path} mode {math_mode}: worst |err| / bound {worst:.3f}, max |err| {float(err.max()):.3g}, "
         f"max |err| where |x| <= 8: {float(err[pre.abs() <= 8].max()):.3g}")
    assert worst <= 1.0
    pre32 = x + bias                                                                    # the epilogue's fp32 input
    assert bool((y[pre32 >= 4.25] == pre32[pre32 >= 4.25].to(torch.bfloat16).float()).all())   # Phi clamps to exactly 1 ...
    assert bool((y[pre32 <= -4.25] == 0).all())                                                # ... and 0
    # negative control: the tanh form of GELU is rejected
    assert gelu_violation(y, x, bias, form=vit_ref.gelu_tanh) > 1.0
