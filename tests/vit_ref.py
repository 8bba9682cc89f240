"""float64 reference of the ViT path (BASELINE configs[4]), written for the tests from the definitions alone:
x = (frame - mean) / std; patch embedding = a PxP convolution of stride P; token 0 = the class token (folded into position 0),
token 1 + p = patch p + position 1 + p; pre-norm blocks x += proj(MHA(LN1(x))), x += fc2(GELU(fc1(LN2(x)))) with
LayerNorm(eps = 1e-6, biased variance), attention softmax(Q K^T / sqrt(64)) V per 64-wide head and the erf form of GELU;
final LayerNorm on the class token, linear head; pbar = softmax(z / temperature), entropy confidence 1 - H(pbar) / ln C.

Nothing here knows how the kernels compute (no bf16 rounding, no polynomial exp or GELU, no key order): it reads only the
weights of a blob.  It runs on any torch device in float64 (the GPU tests run it on the GPU)."""
import math

import numpy as np
import torch

from oracle.fav_oracle import parse_blob   # reads the weights of a blob; nothing else comes from oracle/

F = torch.nn.functional
LN_EPS = 1e-6
HEAD = 64
#: dim, depth, heads, MLP width, patch of the two ViT arches (include/fav.h FAV_ARCH_VIT_B16 = 2, FAV_ARCH_VIT_TINY = 3)
VIT_CFG = {2: dict(dim=768, depth=12, heads=12, mlp=3072, patch=16),
           3: dict(dim=128, depth=2, heads=2, mlp=256, patch=16)}


def layer_norm(x, gamma, beta, eps=LN_EPS):
    m = x.mean(-1, keepdim=True)
    var = ((x - m) ** 2).mean(-1, keepdim=True)
    return (x - m) / torch.sqrt(var + eps) * gamma + beta


def gelu(x):
    """The erf form: x Phi(x)."""
    return 0.5 * x * (1.0 + torch.erf(x / math.sqrt(2.0)))


def gelu_tanh(x):
    """The tanh approximation (a plausible mistake; 4.7e-4 from the erf form at its worst)."""
    return 0.5 * x * (1.0 + torch.tanh(math.sqrt(2.0 / math.pi) * (x + 0.044715 * x ** 3)))


def attention_probs(q, k, scale=1.0 / math.sqrt(HEAD)):
    """q [..., Tq, 64], k [..., Tk, 64] -> softmax(q k^T * scale) over the keys."""
    return torch.softmax(torch.matmul(q, k.transpose(-1, -2)) * scale, dim=-1)


def attention(qkv, heads, scale=1.0 / math.sqrt(HEAD)):
    """qkv [b, T, 3D] (Q | K | V, head h = columns 64h .. 64h + 63 of each) -> [b, T, D]."""
    b, t, d3 = qkv.shape
    q, k, v = qkv.reshape(b, t, 3, heads, HEAD).permute(2, 0, 3, 1, 4)   # [b, heads, T, 64] each
    return torch.matmul(attention_probs(q, k, scale), v).transpose(1, 2).reshape(b, t, d3 // 3)


def normalize(frames, mean, std, device="cpu"):
    """NHWC uint8 (0..255) or float32 in [0, 1] -> (frame - mean) / std, float64 on `device`."""
    x = torch.as_tensor(np.ascontiguousarray(frames)).to(device)
    x = x.double() / 255.0 if x.dtype == torch.uint8 else x.double()
    return (x - torch.tensor(mean, dtype=torch.float64, device=device)) / torch.tensor(std, dtype=torch.float64, device=device)


def vit_logits(model, xn):
    """model = parse_blob(blob) of a ViT checkpoint, xn = normalised frames [b, H, W, 3] float64 (torch) -> logits [b, C]."""
    c, Ls = VIT_CFG[model.arch], model.layers
    dev = xn.device
    t = lambda a: torch.from_numpy(np.ascontiguousarray(a)).to(dev, torch.float64)
    b = xn.shape[0]
    p, d, heads = c["patch"], c["dim"], c["heads"]
    x = F.conv2d(xn.permute(0, 3, 1, 2), t(Ls[0].w).permute(0, 3, 1, 2), t(Ls[0].b), stride=p)    # [b, d, gh, gw]
    x = x.flatten(2).transpose(1, 2)
    pos = t(Ls[1].w).reshape(-1, d)
    if pos.shape[0] != x.shape[1] + 1:
        raise ValueError("position table does not match the input size")
    x = torch.cat([pos[:1].expand(b, 1, d), x + pos[1:]], 1)
    lin = lambda y, L: F.linear(y, t(L.w).reshape(L.cout, -1), t(L.b))
    li = 2
    for _ in range(c["depth"]):
        ln1, qkv, proj, ln2, fc1, fc2 = Ls[li:li + 6]
        li += 6
        x = x + lin(attention(lin(layer_norm(x, t(ln1.w), t(ln1.b)), qkv), heads), proj)
        x = x + lin(gelu(lin(layer_norm(x, t(ln2.w), t(ln2.b)), fc1)), fc2)
    return lin(layer_norm(x[:, 0], t(Ls[li].w), t(Ls[li].b)), Ls[li + 1])


def torch_vit_logits(model, xn):
    """numpy in (normalised frames [b, H, W, 3]), numpy out: the float64 encoder on the CPU."""
    return vit_logits(model, torch.from_numpy(np.ascontiguousarray(xn)).double()).numpy()


def classify(blob, frames, mean=(0.485, 0.456, 0.406), std=(0.229, 0.224, 0.225), device="cpu", chunk=16):
    """Frames (numpy NHWC uint8 or float32 in [0, 1]) -> float64 logits [n, C] (numpy), `chunk` frames at a time."""
    model = parse_blob(blob)
    out = []
    with torch.no_grad():
        for i in range(0, len(frames), chunk):
            out.append(vit_logits(model, normalize(frames[i:i + chunk], mean, std, device)).cpu().numpy())
    return np.concatenate(out)


def head(logits, temperature=1.0):
    """float64 logits [n, C] -> dict: pbar = softmax(z / temperature), label, entropy (nats), entropy confidence
    1 - H / ln C, and gap = top-1 minus top-2 of pbar (a near-tie cannot decide a label)."""
    z = np.asarray(logits, np.float64) / temperature
    e = np.exp(z - z.max(1, keepdims=True))
    pbar = e / e.sum(1, keepdims=True)
    with np.errstate(divide="ignore", invalid="ignore"):
        h = -np.where(pbar > 0, pbar * np.log(np.where(pbar > 0, pbar, 1.0)), 0.0).sum(1)
    srt = np.sort(pbar, 1)
    return dict(pbar=pbar, label=pbar.argmax(1), entropy=h, confidence=1.0 - h / math.log(pbar.shape[1]),
                gap=srt[:, -1] - srt[:, -2])
