"""Pins the CPU oracle: Philox known-answer vectors (Random123), bf16 rounding,
and the NumPy restatement against torch.nn.functional on CPU (SURVEY.md §8c:
the reference pins nothing on this path, so the oracle is cross-checked against
an independent implementation instead)."""
import os
import numpy as np
import pytest
import torch
import torch.nn.functional as F

from failure_aware_vision_amd import synth, weights
from oracle import fav_oracle as O
from oracle import torch_cpu as TC


def test_philox_known_answers():
    # Random123 kat_vectors: philox4x32 10 rounds
    kat = [
        ((0, 0, 0, 0), (0, 0), (0x6627e8d5, 0xe169c58d, 0xbc57ac4c, 0x9b00dbd8)),
        ((0xffffffff,) * 4, (0xffffffff, 0xffffffff), (0x408f276d, 0x41c83b0e, 0xa20bc7c6, 0x6d5451fd)),
        ((0x243f6a88, 0x85a308d3, 0x13198a2e, 0x03707344), (0xa4093822, 0x299f31d0),
         (0xd16cfe09, 0x94fdcceb, 0x5001e420, 0x24126ea1)),
    ]
    for ctr, key, exp in kat:
        out = O.philox4x32_10(*[np.uint32(c) for c in ctr], key[0], key[1])
        assert tuple(int(o) for o in out) == exp


def test_bf16_round_matches_torch():
    rng = np.random.default_rng(0)
    x = np.concatenate([rng.standard_normal(100000).astype(np.float32) * 10,
                        np.float32([0.0, -0.0, 1.0, 1.00390625, 1.0039062, 1.0117188, 3.3895314e38])])
    ref = torch.from_numpy(x).to(torch.bfloat16).to(torch.float32).numpy()
    assert np.array_equal(O.bf16_round(x), ref)


def test_dropout_mask_rate_and_determinism():
    thr = O.dropout_threshold(0.1)
    k1 = O.dropout_keep(4, 3, 2, np.arange(5, 9), 4096, thr)
    k2 = O.dropout_keep(4, 3, 2, np.arange(5, 9), 4096, thr)
    assert np.array_equal(k1, k2)
    assert abs(1.0 - k1.mean() - 0.1) < 0.01
    # mask of an image does not depend on which shard it is in
    k3 = O.dropout_keep(4, 3, 2, np.array([7]), 4096, thr)
    assert np.array_equal(k3[0], k1[2])
    assert not np.array_equal(O.dropout_keep(4, 4, 2, np.array([7]), 4096, thr), k3)


@pytest.mark.parametrize("cin,cout,k,stride,pad,hw", [(3, 64, 7, 2, 3, 32), (64, 64, 3, 1, 1, 14), (64, 128, 3, 2, 1, 15),
                                                      (128, 256, 1, 1, 0, 9), (64, 256, 1, 2, 0, 14)])
def test_conv_vs_torch(cin, cout, k, stride, pad, hw):
    rng = np.random.default_rng(1)
    x = O.bf16_round(rng.standard_normal((2, hw, hw, cin)).astype(np.float32))
    w = O.bf16_round(rng.standard_normal((cout, k, k, cin)).astype(np.float32) * 0.1)
    L = O.ConvLayer(cout, cin, k, k, stride, pad, w, np.zeros(cout, np.float32))
    acc = O.conv_acc(x, L)
    ref = F.conv2d(torch.from_numpy(x.transpose(0, 3, 1, 2).copy()), torch.from_numpy(w.transpose(0, 3, 1, 2).copy()),
                   None, stride, pad).numpy().transpose(0, 2, 3, 1)
    np.testing.assert_allclose(acc, ref, rtol=1e-4, atol=1e-4)


def test_pools_vs_torch():
    rng = np.random.default_rng(2)
    x = O.bf16_round(rng.standard_normal((2, 13, 13, 64)).astype(np.float32))
    xt = torch.from_numpy(x.transpose(0, 3, 1, 2).copy())
    ref = F.max_pool2d(xt, 3, 2, 1).numpy().transpose(0, 2, 3, 1)
    assert np.array_equal(O.maxpool3x3s2(x), ref)
    np.testing.assert_allclose(O.global_avgpool(x), F.adaptive_avg_pool2d(xt, 1).numpy()[:, :, 0, 0], rtol=1e-5, atol=1e-6)


def test_head_vs_torch():
    rng = np.random.default_rng(3)
    lg = (rng.standard_normal((5, 7, 1000)) * 4).astype(np.float32)
    lab, conf, pbar = O.confidence_head(lg, temperature=1.5, kind=O.CONF_MAX_SOFTMAX)
    ref = torch.softmax(torch.from_numpy(lg) / 1.5, -1).mean(0)
    np.testing.assert_allclose(pbar, ref.numpy(), rtol=2e-5, atol=1e-7)
    assert np.array_equal(lab, ref.argmax(-1).numpy())
    _, cent, _ = O.confidence_head(lg, temperature=1.5, kind=O.CONF_ENTROPY)
    h = -(ref * torch.log(ref)).sum(-1) / np.log(1000)
    np.testing.assert_allclose(cent, 1 - h.numpy(), rtol=1e-4, atol=1e-5)
    # tie -> lowest index
    z = np.zeros((1, 1, 8), np.float32); z[0, 0, [2, 5]] = 1.0
    assert O.confidence_head(z)[0][0] == 2
    fail, score = O.failure_detect(np.float32([0.2, 0.5, 0.9]), 0.5)
    assert fail.tolist() == [1, 0, 0] and np.allclose(score, [0.8, 0.5, 0.1])


def _agree(lab_a, conf_a, pbar_a, lab_b, conf_b, tol=6e-2):
    """Two bf16 pipelines that sum in different orders differ by one bf16 ulp on a
    growing fraction of activations (a 1-ulp flip perturbs every downstream sum),
    so end-to-end agreement is statistical: labels equal wherever the top-2 gap
    exceeds tol, confidences within tol.  Per-layer agreement is tight, see
    test_single_block_tight."""
    srt = np.sort(pbar_a, axis=1)
    gap = srt[:, -1] - srt[:, -2]
    assert np.all((lab_a == lab_b) | (gap < tol))
    np.testing.assert_allclose(conf_a, conf_b, atol=tol)


def test_single_conv_tight(r18_blob):
    """Same bf16 input -> one conv + epilogue (one rounding point): the two
    implementations agree to one bf16 ulp and differ on well under 1% of elements."""
    blob, info = r18_blob
    m = O.parse_blob(blob)
    rng = np.random.default_rng(5)
    for li in (1, 5, 7):  # 3x3 s1, 3x3 s2, 1x1 s2 downsample
        L = m.layers[li]
        x = O.bf16_round(np.abs(rng.standard_normal((4, 16, 16, L.cin))).astype(np.float32))
        res = O.bf16_round(rng.standard_normal((4, 16 // L.stride, 16 // L.stride, L.cout)).astype(np.float32))
        ya = O.epilogue(O.conv_acc(x, L), L.b, res=res)
        xt = torch.from_numpy(np.ascontiguousarray(x.transpose(0, 3, 1, 2)))
        wt = torch.from_numpy(np.ascontiguousarray(L.w.transpose(0, 3, 1, 2)))
        yb = TC.TorchNet._conv(xt, (wt, torch.from_numpy(L.b), L.stride, L.pad),
                               res=torch.from_numpy(np.ascontiguousarray(res.transpose(0, 3, 1, 2))))
        yb = yb.numpy().transpose(0, 2, 3, 1)
        d = np.abs(ya - yb)
        assert (d > 0).mean() < 0.01
        assert np.all(d <= np.maximum(np.abs(ya), np.abs(yb)) * 2.0 ** -7 + 1e-5)


def test_resnet18_numpy_vs_torch(r18_blob):
    """BASELINE config 1: ResNet-18, 32x32, batch 32, single pass, max-softmax."""
    blob, info = r18_blob
    m = O.parse_blob(blob)
    fr = synth.synthetic_frames_u8(32, 32, 32, seed=7)
    cfg = O.ClassifyConfig()
    la, ca, lga, pa = O.classify(m, fr, cfg, return_logits=True)
    lb, cb, lgb, pb = TC.classify(m, fr, cfg, return_logits=True)
    _agree(la, ca, pa, lb, cb)
    assert np.sqrt(((lga - lgb) ** 2).mean()) < 0.05 * lga.std()  # same graph, different summation order
    assert len(set(la.tolist())) >= 5  # the synthetic model is not degenerate


def test_resnet18_mc_dropout_numpy_vs_torch(r18_blob):
    blob, info = r18_blob
    m = O.parse_blob(blob)
    fr = synth.synthetic_frames_u8(6, 32, 32, seed=8)
    for policy in ("last_layer", "layer4+fc", "all_blocks"):
        cfg = O.ClassifyConfig(n_samples=3, site_mask=weights.site_mask_for(0, policy), p=0.1, seed=4)
        ids = np.arange(10, 16)
        la, ca, lga, pa = O.classify(m, fr, cfg, img_ids=ids, return_logits=True)
        lb, cb, lgb, pb = TC.classify(m, fr, cfg, img_ids=ids, return_logits=True)
        assert lga.shape == (3, 6, 10)
        _agree(la, ca, pa, lb, cb)
        assert not np.allclose(lga[0], lga[1])  # samples differ
        # shard invariance: images 2..4 alone give the same logits as inside the batch
        lc = O.classify(m, fr[2:5], cfg, img_ids=ids[2:5], return_logits=True)[2]
        np.testing.assert_allclose(lc, lga[:, 2:5], rtol=1e-4, atol=1e-4)


def test_resnet50_small_numpy_vs_torch(r50_blob):
    blob, info = r50_blob
    m = O.parse_blob(blob)
    fr = synth.synthetic_frames_u8(2, 64, 64, seed=9)
    cfg = O.ClassifyConfig(n_samples=2, site_mask=weights.site_mask_for(1, "all_blocks"), p=0.1, seed=4)
    la, ca, lga, pa = O.classify(m, fr, cfg, return_logits=True)
    lb, cb, lgb, pb = TC.classify(m, fr, cfg, return_logits=True)
    _agree(la, ca, pa, lb, cb)
    assert np.sqrt(((lga - lgb) ** 2).mean()) < 0.05 * lga.std()  # same graph, different summation order


def test_blob_is_machine_independent(r18_blob, r50_blob):
    """Checksums of the synthetic checkpoints every fixture was generated with."""
    import json, os
    path = os.path.join(os.path.dirname(__file__), "golden", "blob_sha256.json")
    pinned = json.load(open(path))
    assert r18_blob[1]["sha256"] == pinned["resnet18_cifar_seed1"]
    assert r50_blob[1]["sha256"] == pinned["resnet50_seed1"]


def test_bf16_mfma_model_reproduces_recorded_instruction_outputs():
    """oracle/fav_exact.c models v_mfma_f32_16x16x32_bf16 (the instruction the production kernels
    accumulate with).  tests/golden/mfma_kat.npz holds raw outputs of that instruction recorded on an
    MI355X (tools/mfma_probe*.py: random, wide-range, sparse, accumulator-dominant, carry-out and
    leading-bit-loss operands); the model must reproduce every one bit for bit."""
    import ctypes
    import os
    lib = O._exact_lib()
    kat = np.load(os.path.join(os.path.dirname(__file__), "golden", "mfma_kat.npz"))
    names = sorted(set(k[:-2] for k in kat.files))
    assert len(names) >= 40
    total = 0
    for n in names:
        tof = lambda b: np.ascontiguousarray((b.astype(np.uint32) << 16).view(np.float32))
        A, B, C, D = tof(kat[n + "_A"]), tof(kat[n + "_B"]), np.ascontiguousarray(kat[n + "_C"]), kat[n + "_D"]
        out = np.empty_like(D)
        lib.fav_bf16mfma_replay(A.ctypes.data, B.ctypes.data, C.ctypes.data, out.ctypes.data, A.shape[0])
        assert np.array_equal(out, D), n
        # the AVX-512 form of the same arithmetic (what the fixture generators run where the CPU has it)
        out2 = np.full_like(D, np.nan)
        lib.fav_bf16mfma_replay_avx512.restype = ctypes.c_int
        lib.fav_bf16mfma_replay_avx512.argtypes = [ctypes.c_void_p] * 4 + [ctypes.c_int]
        if lib.fav_bf16mfma_replay_avx512(A.ctypes.data, B.ctypes.data, C.ctypes.data, out2.ctypes.data, A.shape[0]) == 0:
            assert np.array_equal(out2.view(np.uint32), D.view(np.uint32)), n + " (AVX-512 form)"
        total += D.size
    assert total > 100000


def test_bf16_mfma_model_vector_form_equals_scalar_form_on_convolutions():
    """The AVX-512 path of fav_bf16mfma_conv_acc against the scalar one (FAV_ORACLE_SCALAR=1 in a child
    process: the choice is cached per process), on activations with ReLU zeros, wide-range values and padding."""
    import subprocess
    import sys
    code = r"""
import sys, numpy as np
sys.path.insert(0, %r)
from oracle import fav_oracle as O
rng = np.random.default_rng(7)
outs = []
for (b, h, c, n, kh, s, p) in ((2, 9, 64, 40, 3, 1, 1), (1, 8, 128, 256, 1, 1, 0), (2, 10, 64, 64, 3, 2, 1)):
    x = rng.standard_normal((b, h, h, c)).astype(np.float32) * np.exp2(rng.integers(-12, 6, (b, h, h, c))).astype(np.float32)
    x = np.where(rng.random(x.shape) < 0.45, 0.0, x).astype(np.float32)
    w = (rng.standard_normal((n, kh, kh, c)) * np.exp2(rng.integers(-6, 2, (n, 1, 1, 1)))).astype(np.float32)
    w[:, :, :, ::7] = 0
    outs.append(O.conv_acc_exact(O.bf16_round(x), O.bf16_round(w), kh, kh, s, p, mode="mfma"))
np.save(sys.argv[1], np.concatenate([o.ravel() for o in outs]))
""" % os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
    import tempfile
    res = {}
    with tempfile.TemporaryDirectory() as td:
        for tag, env in (("vector", {}), ("scalar", {"FAV_ORACLE_SCALAR": "1"})):
            out = os.path.join(td, tag + ".npy")
            subprocess.check_call([sys.executable, "-c", code, out], env={**os.environ, **env})
            res[tag] = np.load(out)
    assert np.isfinite(res["scalar"]).all() and np.abs(res["scalar"]).max() > 0
    assert np.array_equal(res["vector"].view(np.uint32), res["scalar"].view(np.uint32))


def test_c_epilogue_equals_the_numpy_specification():
    rng = np.random.default_rng(3)
    acc = (rng.standard_normal((3, 5, 7, 64)) * np.exp2(rng.integers(-20, 10, (3, 5, 7, 64)))).astype(np.float32)
    bias = rng.standard_normal(64).astype(np.float32)
    res = O.bf16_round(rng.standard_normal(acc.shape).astype(np.float32))
    keep = rng.random(acc.shape) > 0.1
    scale = O.dropout_scale(O.dropout_threshold(0.1))
    for kw in (dict(), dict(res=res), dict(res=res, keep=keep, scale=scale), dict(relu=False), dict(keep=keep, scale=scale)):
        a = O.epilogue(acc, bias, **kw)
        b = O.epilogue_numpy(acc, bias, **kw)
        assert a.dtype == np.float32 and np.array_equal(a.view(np.uint32), b.view(np.uint32)), kw.keys()


def test_committed_fixtures_belong_to_the_current_checkpoint_and_oracle(r50_blob):
    """Every ResNet-50 fixture under tests/golden/ records the checkpoint it was made with, and the first frames of the
    10,000-frame fixtures are replayed through the oracle as it is NOW: a fixture generated by another state of the
    oracle (a different summation order, say) or of the weights fails here, on the CPU, before any GPU run."""
    import glob
    import zlib
    blob, info = r50_blob
    gold = os.path.join(os.path.dirname(__file__), "golden")
    names = sorted(glob.glob(os.path.join(gold, "r50_*.npz")))
    assert len(names) >= 8
    for path in names:
        d = np.load(path)
        assert str(d["blob_sha256"]) == info["sha256"], os.path.basename(path) + " was generated with a different checkpoint"
    model = O.parse_blob(blob)
    u8 = synth.synthetic_frames_u8(2, 224, 224, seed=21, start_id=0)
    x = synth.gaussian_noise_f32(u8, 3, seed=3, start_id=0)
    d = np.load(os.path.join(gold, "r50_mfma_10k_noise3.npz"))
    l, c, lg, pb = O.classify(model, x, O.ClassifyConfig(exact="mfma"), return_logits=True)
    crc = np.array([zlib.crc32(np.ascontiguousarray(lg[:, i, :]).tobytes()) for i in range(2)], np.uint32)
    assert np.array_equal(crc, d["logit_crc32"][:2]), "the production-mode fixture does not match the MFMA-model oracle"
    assert np.array_equal(l, d["labels"][:2]) and np.abs(c - d["conf"][:2]).max() < 1e-6
    d = np.load(os.path.join(gold, "r50_exact_10k_noise3.npz"))
    l, c = O.classify(model, x, O.ClassifyConfig(exact=True))
    assert np.array_equal(l, d["labels"][:2]) and np.abs(c - d["conf"][:2]).max() < 1e-6
    # The independent fixtures against the production fixture, frame by frame (the GPU test proves the kernels equal the latter
    # bit for bit, so these are the production path's agreement figures; measured 9,955 and 9,890 of 10,000 labels)
    prod = np.load(os.path.join(gold, "r50_mfma_10k_noise3.npz"))
    for name, floor, dmax in (("r50_torchcpu_10k.npz", 9920, 0.04), ("r50_fp32_module_10k.npz", 9840, 0.12)):
        ind = np.load(os.path.join(gold, name))
        assert len(ind["labels"]) == len(prod["labels"]) == 10000
        same = prod["labels"].astype(np.int64) == ind["labels"].astype(np.int64)
        assert same.sum() >= floor, (name, int(same.sum()))
        assert (prod["labels"][~same] == ind["second"][~same]).mean() >= 0.9          # disagreements sit on the other model's runner-up
        assert np.abs(prod["conf"] - ind["conf"]).max() < dmax


# ---------------------------------------------------------------------------------------------------------------------
# NaN and the infinities (the float64 reference of the classes is tests/nonfinite_ref.py)
# ---------------------------------------------------------------------------------------------------------------------
def test_c_epilogue_equals_the_numpy_specification_on_non_finite_values():
    """np.maximum keeps a NaN; so does the C restatement: bit for bit the specification, a NaN counting as equal whatever
    its payload, on an accumulator that holds both NaNs, both infinities, +inf under a residual of -inf and a finite fp32
    above the bf16 range."""
    import nonfinite_ref as N
    rng = np.random.default_rng(4)
    acc = rng.standard_normal((2, 3, 5, 64)).astype(np.float32)
    res = O.bf16_round(rng.standard_normal(acc.shape).astype(np.float32))
    acc[0, 0, 0, :6] = [N.special("nan"), N.special("nan_neg"), np.inf, -np.inf, np.inf, 3.4e38]
    res[0, 0, 0, 4] = -np.inf
    acc[1, ..., 7], acc[1, ..., 8], acc[1, ..., 9] = np.nan, np.inf, -np.inf
    bias = rng.standard_normal(64).astype(np.float32)
    keep = rng.random(acc.shape) > 0.3
    scale = O.dropout_scale(O.dropout_threshold(0.3))
    with np.errstate(all="ignore"):
        for kw in (dict(), dict(res=res), dict(res=res, keep=keep, scale=scale), dict(relu=False), dict(res=res, relu=False), dict(keep=keep, scale=scale)):
            a, b = O.epilogue(acc, bias, **kw), O.epilogue_numpy(acc, bias, **kw)
            nan = np.isnan(b)
            assert np.array_equal(np.isnan(a), nan) and np.array_equal(a.view(np.uint32)[~nan], b.view(np.uint32)[~nan]), kw.keys()
            relu = kw.get("relu", True)
            want = [N.NAN, N.NAN, N.PINF, N.FIN if relu else N.NINF, N.NAN if "res" in kw else N.PINF, N.PINF]
            kept = keep[0, 0, 0, :6] if "keep" in kw else np.ones(6, bool)
            assert N.classes(a[0, 0, 0, :6]).tolist() == [w if k else N.FIN for w, k in zip(want, kept)], kw.keys()
            assert np.isnan(a).sum() > 10 or "keep" in kw


@pytest.mark.parametrize("kh,stride,pad", [(1, 1, 0), (3, 1, 1), (3, 2, 1)])
def test_mfma_model_gives_the_ieee_class_for_non_finite_operands(kh, stride, pad):
    """fav_bf16mfma_conv_acc on inputs that hold NaN and the infinities: every output's class is float64's (the rule of
    tests/nonfinite_ref.py) and the f32-chain mode's, and a pixel with a clean receptive field keeps the bits it has on the
    clean input.  Also an accumulator that overflows on finite operands, and products beyond the fp32 range."""
    import nonfinite_ref as N
    rng = np.random.default_rng(kh * 10 + stride)
    x = O.bf16_round(np.clip(rng.standard_normal((2, 9, 10, 64)), -4, 4).astype(np.float32))
    x = np.where(rng.random(x.shape) < 0.3, np.float32(0), x)            # ReLU zeros: inf x 0 on the weight side stays out, 0 x w is 0
    w = O.bf16_round((rng.standard_normal((40, kh, kh, 64)) * 0.1).astype(np.float32))
    w[:, :, :, ::9] = 0                                                   # zero weights: inf x 0 is a NaN
    p = x.copy()
    for i, kind in enumerate(("+inf", "-inf", "nan", "nan_neg")):
        p[0, 2 * i + 1, 2, 3 * i + 1] = N.special(kind)
    p[0, 4, 7, 0] = np.inf                                                # on a zero weight (channel 0)
    p[0, 7, 6, 11], p[0, 7, 6, 12] = np.inf, -np.inf
    cols, ho, wo = N.im2col(p, kh, kh, stride, pad)
    ref, _ = N.dot_classes(cols, w.reshape(40, -1))
    ref = ref.reshape(2, ho, wo, 40)
    assert set(np.unique(ref).tolist()) == {N.NAN, N.PINF, N.NINF, N.FIN}
    clean_acc = O.conv_acc_exact(x, w, kh, kh, stride, pad, mode="mfma")
    got = O.conv_acc_exact(p, w, kh, kh, stride, pad, mode="mfma")
    chain = O.conv_acc_exact(p, w, kh, kh, stride, pad, mode=True)
    assert np.array_equal(N.classes(got), ref) and np.array_equal(N.classes(chain), ref)
    untouched = ref == N.FIN
    dirty, _, _ = N.im2col((p.view(np.uint32) != x.view(np.uint32)).any(axis=3, keepdims=True), kh, kh, stride, pad)
    untouched = np.broadcast_to((dirty.sum(axis=1) == 0).reshape(2, ho, wo, 1), ref.shape)
    assert untouched.mean() > 0.5 and np.array_equal(got.view(np.uint32)[untouched], clean_acc.view(np.uint32)[untouched])
    assert np.array_equal(got[1].view(np.uint32), clean_acc[1].view(np.uint32))                # the frame without poison
    if kh == 1:
        # finite operands: an accumulator that overflows stays infinite (finite products cannot move it) ...
        big = np.full((1, 1, 1, 64), 2.0 ** 60, np.float32)
        wb = np.zeros((3, 1, 1, 64), np.float32)
        wb[0, ..., :32], wb[0, ..., 32:] = 2.0 ** 64, -(2.0 ** 20)
        wb[1] = -wb[0]
        wb[2, ..., :8] = 1.0
        out = O.conv_acc_exact(big, wb, 1, 1, 1, 0, mode="mfma").ravel()
        assert out[0] == np.inf and out[1] == -np.inf and out[2] == np.float32(2.0 ** 63)
        assert np.array_equal(N.classes(O.conv_acc_exact(big, wb, 1, 1, 1, 0, mode=True).ravel()), N.classes(out))
        # ... and a product beyond the fp32 range is an infinity of its sign: both signs in one accumulator are a NaN
        # (measured on the matrix unit; the fmaf chain rounds once per step and answers with the first infinity it reaches)
        px = np.full((1, 1, 1, 64), 2.25, np.float32)
        wh = np.zeros((3, 1, 1, 64), np.float32)
        wh[0], wh[1] = 2.0 ** 127, 2.0 ** 127
        wh[1, ..., 40:] = -(2.0 ** 127)
        wh[2] = 2.0 ** 126                                                 # 2.25 x 2^126 < 2^128: finite products, the sum overflows
        out = O.conv_acc_exact(px, wh, 1, 1, 1, 0, mode="mfma").ravel()
        assert out[0] == np.inf and np.isnan(out[1]) and out[2] == np.inf


@pytest.mark.parametrize("exact", ["mfma", True], ids=["mfma", "f32-chain"])
def test_overflowing_checkpoint_ends_in_the_non_finite_frame_rule(r18_blob, exact):
    """layer2.0.conv1 and layer2.0.conv2 of the ResNet-18 fixture scaled by 2^100: every weight is finite, the activations
    overflow bf16, +inf meets weights of both signs.  O.classify answers with non-finite logits and the non-finite frame
    rule - label 0, confidence 0, hence fail and score 1 - on every frame, in both exact modes; it used to answer label 0 with
    a confidence of 0.75 - 0.84."""
    import nonfinite_ref as N
    blob = N.scale_layer(N.scale_layer(r18_blob[0], 5, 100), 6, 100)
    model = O.parse_blob(blob)
    assert all(np.isfinite(L.w).all() and np.isfinite(L.b).all() for L in model.layers)
    frames = synth.synthetic_frames_u8(3, 32, 32, seed=11)
    labels, conf, lg, pbar = O.classify(model, frames, O.ClassifyConfig(exact=exact), return_logits=True)
    assert not np.isfinite(lg).any(axis=-1).all() and O.nonfinite_frames(lg).all()
    assert (labels == 0).all() and (conf == 0).all() and np.isnan(pbar).all()
    fail, score = O.failure_detect(conf, 0.5)
    assert (fail == 1).all() and (score == 1).all()
    # a finite frame beside it keeps what it had: the rule touches the non-finite frames alone
    mixed = np.concatenate([lg, np.zeros_like(lg[:, :1])], axis=1)
    mixed[0, -1, 3] = 5.0
    l2, c2, p2 = O.confidence_head(mixed)
    l1, c1, p1 = O.confidence_head(mixed[:, -1:])
    assert l2[-1] == l1[0] == 3 and c2[-1] == c1[0] > 0.5 and (l2[:-1] == 0).all() and (c2[:-1] == 0).all()
