"""CPU checks of the ViT oracle (BASELINE configs[4]).  The oracle is the specification (PARITY UNPINNED:
the reference has no classifier), so it is cross-checked against torch on CPU - exp, GELU, LayerNorm and
softmax against float64 formulas, the whole encoder against a torch.nn.functional implementation - and the
synthetic checkpoints are pinned by checksum."""
import json
import os

import numpy as np
import pytest

from failure_aware_vision_amd import synth, weights
from oracle import fav_oracle as O

torch = pytest.importorskip("torch")
F = torch.nn.functional
import vit_ref  # noqa: E402
from vit_ref import torch_vit_logits  # noqa: E402


def test_exact_exp_and_gelu_are_accurate():
    x = np.concatenate([np.linspace(-80, 88, 200001), np.linspace(-1, 1, 100001)]).astype(np.float32)
    e = O.expf_exact(x).astype(np.float64)
    ref = np.exp(x.astype(np.float64))
    assert np.max(np.abs(e - ref) / ref) < 4e-7                      # ~3 ulp of fp32
    assert O.expf_exact(np.array([-81.0, -1e30, -np.inf], np.float32)).tolist() == [0.0, 0.0, 0.0]
    xg = np.linspace(-12, 12, 240001).astype(np.float32)
    g = O.gelu_exact(xg).astype(np.float64)
    refg = F.gelu(torch.from_numpy(xg).double()).numpy()              # the erf form, torch.nn.GELU's default
    assert np.max(np.abs(g - refg)) < 1e-4                           # (the tanh form is 4.7e-4 away from it)
    assert O.gelu_exact(np.array([-30.0, 30.0], np.float32)).tolist() == [-0.0, 30.0]


def test_layernorm_and_softmax_vs_torch():
    rng = np.random.default_rng(0)
    for d in (128, 768, 1024):
        x = (rng.standard_normal((9, d)) * 3 + 1).astype(np.float32)
        g, b = rng.standard_normal(d).astype(np.float32), rng.standard_normal(d).astype(np.float32)
        ref = F.layer_norm(torch.from_numpy(x).double(), (d,), torch.from_numpy(g).double(), torch.from_numpy(b).double(), 1e-6)
        assert np.abs(O.layernorm_exact(x, g, b) - ref.numpy()).max() < 2e-5
    s = (rng.standard_normal((11, 197)) * 4).astype(np.float32)
    p = O.attn_softmax_exact(s)                                      # raw scores in, softmax(s / 8) out
    assert np.abs(p - torch.softmax(torch.from_numpy(s).double() / 8, -1).numpy()).max() < 3e-6


@pytest.mark.parametrize("exact", [False, True, "mfma"])
def test_vit_tiny_oracle_vs_torch(exact):
    blob, info = weights.make_synthetic_vit("vit_tiny", seed=3)
    model = O.parse_blob(blob)
    frames = synth.synthetic_frames_u8(5, 64, 64, seed=11)
    cfg = O.ClassifyConfig(exact=exact, temperature=1.5, conf_kind=O.CONF_ENTROPY)
    xn = O.normalize_input(frames, cfg.mean, O.inv_std32(cfg.std))
    labels, conf, lg, pbar = O.classify(model, frames, cfg, return_logits=True)
    ref = torch_vit_logits(model, xn)
    # bf16 activations vs an fp64 network: small relative to the logits' spread, same winners where the gap is clear
    assert np.sqrt(np.mean((lg[0] - ref) ** 2)) < 0.03 * ref.std()
    pr = torch.softmax(torch.from_numpy(ref) / 1.5, -1).numpy()
    srt = np.sort(pr, 1)
    clear = (srt[:, -1] - srt[:, -2]) > 0.05
    assert np.array_equal(labels[clear], pr.argmax(1)[clear])
    ent = 1.0 + (pr * np.log(np.maximum(pr, 1e-300))).sum(1) / np.log(pr.shape[1])
    assert np.abs(conf - ent).max() < 0.02


def test_vit_b16_oracle_vs_float64():
    """The production-mode oracle (= the device's bits, tests/test_gpu_vit.py) of the full ViT-B/16 - 12 layers, 768 wide, 12 heads -
    at 64x64 (17 tokens) against the float64 restatement of tests/vit_ref.py, on clean and Gaussian-corrupted frames.  Measured:
    rel. RMS 0.0080 of the logits' spread, max abs 0.16 (spread ~5), entropy confidence within 0.0061; the bounds are ~2.5x that."""
    blob, _ = weights.make_synthetic_vit("vit_b16", seed=1, in_hw=(64, 64))
    u8 = synth.synthetic_frames_u8(4, 64, 64, seed=21)
    frames = np.concatenate([u8.astype(np.float32) / np.float32(255.0), synth.gaussian_noise_f32(u8, 3, seed=3)])
    cfg = O.ClassifyConfig(exact="mfma", temperature=1.5, conf_kind=O.CONF_ENTROPY)
    labels, conf, lg, _ = O.classify(O.parse_blob(blob), frames, cfg, return_logits=True)
    ref = vit_ref.classify(blob, frames)
    err = lg[0].astype(np.float64) - ref
    assert np.sqrt(np.mean(err ** 2)) < 0.02 * ref.std()
    assert np.abs(err).max() < 0.4
    hd = vit_ref.head(ref, 1.5)
    clear = hd["gap"] > 0.01
    assert clear.sum() >= 6
    assert np.array_equal(labels[clear], hd["label"][clear])
    assert np.abs(conf - hd["confidence"]).max() < 0.015
    # negative control: the same confidences are far from what temperature 1.0 would give
    assert np.abs(conf - vit_ref.head(ref, 1.0)["confidence"]).max() > 0.015


def test_vit_checkpoints_are_machine_independent():
    path = os.path.join(os.path.dirname(__file__), "golden", "blob_sha256.json")
    pins = json.load(open(path))
    assert weights.make_synthetic_vit("vit_tiny", seed=1)[1]["sha256"] == pins["vit_tiny_seed1"]
    assert weights.make_synthetic_vit("vit_b16", seed=1)[1]["sha256"] == pins["vit_b16_seed1"]


def test_attention_key_order_is_a_block_permutation():
    """Slot order of the second attention product: a permutation inside every 32-key block, identity on the block index,
    keys 4g .. 4g + 3 and 16 + 4g .. 16 + 4g + 3 in lane group g's eight slots."""
    for t in (1, 17, 32, 197, 256):
        order = O.attn_key_order(t)
        assert order.size == (t + 31) // 32 * 32
        assert np.array_equal(np.sort(order), np.arange(order.size))
        assert np.array_equal(order >> 5, np.arange(order.size) >> 5)
    assert O.attn_key_order(32)[:16].tolist() == [0, 1, 2, 3, 16, 17, 18, 19, 4, 5, 6, 7, 20, 21, 22, 23]


def test_attention_does_not_depend_on_how_keys_are_padded():
    """attention() pads keys to a multiple of 32 with zero probabilities: two token counts with the same real keys and queries
    give the same rows (what lets the device mask only the last key tile)."""
    rng = np.random.default_rng(4)
    qkv = O.bf16_round((rng.standard_normal((1, 40, 3 * 64)) * 1.1).astype(np.float32))
    full = O.attention(qkv, 1, exact="mfma")
    again = O.attention(qkv.copy(), 1, exact="mfma")
    assert np.array_equal(full, again)
    ref = np.einsum("qk,kd->qd", torch.softmax(torch.from_numpy(qkv[0, :, :64] @ qkv[0, :, 64:128].T).double() / 8, -1).numpy(),
                    qkv[0, :, 128:].astype(np.float64))
    assert np.abs(full[0] - ref).max() < 0.03
