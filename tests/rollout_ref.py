"""References of the attention tap and the rollout head (include/fav.h beside fav_set_attn_tap and fav_rollout_record).

1. A numpy restatement of both contracts, operation by operation: the head-mean attention from the oracle's model of the
   production score product (``O.gemm_acc(q, k, "mfma")``) and of the production softmax in front of its rounding to bf16
   (``O.attn_softmax_exact``), head sum in head order, one multiplication by float32(1 / heads); then the rollout chain and
   the record, every product and every sum one float32 numpy operation.  The GPU tests compare bits with it.
2. A float64 reference written from the definitions alone (Abnar & Zuidema 2020): a forward pass built from vit_ref's helpers
   that keeps each layer's head-mean attention, and the rollout in float64.  Nothing in it knows how the kernels compute."""
import numpy as np
import torch

import vit_ref as V
from map_ref import cells_above, same_bits  # noqa: F401  (same_bits: for the tests that compare with this module)
from oracle import fav_oracle as O

F32 = np.float32
RECORD_DWORDS = 8


def attn_ld(T) -> int:
    return 16 * ((T + 15) // 16)


# ---- 1. the contracts, in float32 ---------------------------------------------------------------------------------------------
def attn_mean(qkv, heads) -> np.ndarray:
    """qkv float32 [n, T, 3 D] holding bf16 values, D = 64 heads -> A float32 [n, T, ldT], columns >= T +0."""
    qkv = np.asarray(qkv, F32)
    n, T, d3 = qkv.shape
    D = d3 // 3
    assert D == 64 * heads
    A = np.zeros((n, T, attn_ld(T)), F32)
    inv = F32(1.0 / heads)
    with np.errstate(all="ignore"):
        for i in range(n):
            acc = np.zeros((T, T), F32)
            for h in range(heads):
                q = qkv[i, :, 64 * h:64 * h + 64]
                k = qkv[i, :, D + 64 * h:D + 64 * h + 64]
                acc = acc + O.attn_softmax_exact(O.gemm_acc(q, k, "mfma"))
            A[i, :, :T] = acc * inv
    return A


def rollout_rows(A, first_layer=0) -> np.ndarray:
    """Steps 1 - 3: A float32 [L, n, T, ld >= T] -> r float32 [n, T], the class token's row of the product."""
    A = np.asarray(A, F32)
    L, n, T = A.shape[:3]
    eye = np.eye(T, dtype=F32) * F32(0.5)                     # 0.5f on the diagonal, +0 elsewhere
    with np.errstate(all="ignore"):
        mix = lambda l: F32(0.5) * A[l, :, :, :T] + eye[None]     # [n, T, T]; one product, one sum
        r = mix(L - 1)[:, 0, :]
        for l in range(L - 2, first_layer - 1, -1):
            At = mix(l)
            nxt = np.zeros((n, T), F32)
            for t in range(T):
                nxt = nxt + r[:, t:t + 1] * At[:, t, :]
            r = nxt
    return r


def rollout_records(M, r0, n_layers, gw) -> np.ndarray:
    """Steps 4 - 6 on maps M float32 [n, HW] and class-token masses r0 [n] -> int32 [n, 8] fav_rollout_record records."""
    M = np.asarray(M, F32)
    n, HW = M.shape
    rec = np.zeros((n, RECORD_DWORDS), np.int32)
    f = rec.view(F32)
    with np.errstate(all="ignore"):
        for i in range(n):
            m = M[i]
            total = F32(0)
            peak, cell, floor = F32(-np.inf), -1, F32(np.inf)
            for p in range(HW):
                v = m[p]
                total = total + v
                if v > peak:
                    peak, cell = v, p
                if v < floor:
                    floor = v
            n_above, box = 0, -1
            if peak > floor:
                n_above, box = cells_above(m, floor + F32(0.5) * (peak - floor), gw)
            rec[i, 0], rec[i, 3], rec[i, 6], rec[i, 7] = n_layers, cell, n_above, box
            f[i, 1], f[i, 2], f[i, 4], f[i, 5] = r0[i], peak, floor, total
    return rec


def rollout(A, gh, gw, first_layer=0):
    """The whole head: A float32 [L, n, T, ld] with T = gh gw + 1 -> (M float32 [n, gh gw], records int32 [n, 8])."""
    A = np.asarray(A, F32)
    assert A.shape[2] == gh * gw + 1
    r = rollout_rows(A, first_layer)
    M = np.ascontiguousarray(r[:, 1:])
    return M, rollout_records(M, r[:, 0], A.shape[0] - first_layer, gw)


# ---- 2. from the definitions, in float64 ----------------------------------------------------------------------------------------
def vit_attention_f64(model, xn) -> torch.Tensor:
    """model = parse_blob(blob) of a ViT checkpoint, xn = normalised frames [b, H, W, 3] float64 (torch) -> the head-mean
    attention of every layer, float64 [L, b, T, T]: vit_ref.vit_logits' forward pass, keeping mean_h softmax(q_h k_h^T / 8)."""
    c, Ls = V.VIT_CFG[model.arch], model.layers
    dev = xn.device
    t = lambda a: torch.from_numpy(np.ascontiguousarray(a)).to(dev, torch.float64)
    lin = lambda y, L: V.F.linear(y, t(L.w).reshape(L.cout, -1), t(L.b))
    b = xn.shape[0]
    p, d, heads = c["patch"], c["dim"], c["heads"]
    x = V.F.conv2d(xn.permute(0, 3, 1, 2), t(Ls[0].w).permute(0, 3, 1, 2), t(Ls[0].b), stride=p).flatten(2).transpose(1, 2)
    pos = t(Ls[1].w).reshape(-1, d)
    x = torch.cat([pos[:1].expand(b, 1, d), x + pos[1:]], 1)
    T = x.shape[1]
    out = []
    li = 2
    for _ in range(c["depth"]):
        ln1, qkv_l, proj, ln2, fc1, fc2 = Ls[li:li + 6]
        li += 6
        qkv = lin(V.layer_norm(x, t(ln1.w), t(ln1.b)), qkv_l)
        q, k, v = qkv.reshape(b, T, 3, heads, V.HEAD).permute(2, 0, 3, 1, 4)      # [b, heads, T, 64] each
        P = V.attention_probs(q, k)
        out.append(P.mean(1))
        x = x + lin(torch.matmul(P, v).transpose(1, 2).reshape(b, T, d), proj)
        x = x + lin(V.gelu(lin(V.layer_norm(x, t(ln2.w), t(ln2.b)), fc1)), fc2)
    return torch.stack(out)


def rollout_f64(A, first_layer=0, identity=True) -> np.ndarray:
    """A float64 [L, n, T, T] -> the class token's row of prod_l (A_l + I) / 2 over l = first_layer .. L-1, patches only:
    float64 [n, T - 1].  identity=False: the product of the raw A_l (the residual connection forgotten)."""
    A = np.asarray(A, np.float64)
    L, n, T = A.shape[:3]
    mix = (lambda a: 0.5 * a + 0.5 * np.eye(T)) if identity else (lambda a: a)
    r = mix(A[L - 1])[:, 0, :]
    for l in range(L - 2, first_layer - 1, -1):
        r = np.einsum("nt,ntu->nu", r, mix(A[l]))
    return r[:, 1:]


def classify_attention_f64(blob, frames, mean=(0.485, 0.456, 0.406), std=(0.229, 0.224, 0.225), device="cpu") -> np.ndarray:
    """Frames (numpy NHWC uint8) -> float64 head-mean attention [L, n, T, T] (numpy)."""
    with torch.no_grad():
        return vit_attention_f64(O.parse_blob(blob), V.normalize(frames, mean, std, device)).cpu().numpy()
