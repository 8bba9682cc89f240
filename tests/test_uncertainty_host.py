"""CPU-side checks of the uncertainty head's interface: the fav_uncertainty record layout (C vs ctypes), the new
symbols, fav_create's validation of conf_kind 2 (FAV_CONF_MUTUAL_INFO, checked before the device probe), the tests'
own float64 reference (uncertainty_ref.py) on cases with known answers, unpack_uncertainty, and the detail=True
shard / gather logic under a 2-rank gloo group with a stand-in classifier."""
import ctypes as C
import math
import os
import subprocess
import sys

import numpy as np
import pytest

from uncertainty_ref import FLOAT_FIELDS, head_uncertainty, pack_records

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
FIELDS = ("label", "confidence", "mean_prob", "prob_std", "pred_entropy", "expected_entropy", "mutual_info", "agreement",
          "top_label", "top_prob")


@pytest.fixture(scope="module")
def lib():
    from failure_aware_vision_amd import _lib
    if not os.path.exists(_lib.LIB_PATH):
        import __graft_entry__ as g
        g.build()
    return _lib.load()


_LAYOUT_C = r"""
#include <stddef.h>
#include <stdio.h>
#include "fav.h"
int main(void) {
    printf("size %zu\n", sizeof(fav_uncertainty));
#define F(x) printf("%s %zu\n", #x, offsetof(fav_uncertainty, x));
    F(label) F(confidence) F(mean_prob) F(prob_std) F(pred_entropy) F(expected_entropy) F(mutual_info) F(agreement)
    F(top_label) F(top_prob)
    printf("kind %d\n", (int)FAV_CONF_MUTUAL_INFO);
    return 0;
}
"""


def test_record_layout_matches_ctypes_and_symbols_exported(lib, tmp_path):
    from failure_aware_vision_amd import _lib
    src = tmp_path / "layout.c"
    src.write_text(_LAYOUT_C)
    exe = str(tmp_path / "layout")
    subprocess.check_call(["gcc", "-std=c99", "-Wall", "-Werror", "-I" + os.path.join(ROOT, "include"), str(src), "-o", exe])
    out = dict(line.split() for line in subprocess.check_output([exe], text=True).splitlines())
    assert int(out["size"]) == 72 == C.sizeof(_lib.FavUncertainty)
    for name in FIELDS:
        assert int(out[name]) == getattr(_lib.FavUncertainty, name).offset, name
    assert int(out["kind"]) == _lib.CONF_MUTUAL_INFO == 2
    for sym in ("fav_classify_uncertainty", "fav_op_head_uncertainty"):
        assert hasattr(lib, sym), sym
    assert lib.fav_abi_version() == 2


def _cfg(lib, arch=0, **kw):
    from failure_aware_vision_amd import _lib
    c = _lib.FavConfig()
    lib.fav_default_config(C.byref(c), arch)
    for k, v in kw.items():
        setattr(c, k, v)
    return c


def test_create_rejects_mutual_info_without_samples(lib):
    """conf_kind 2 needs T >= 2 samples over >= 2 classes; the check runs before the device probe (any machine)."""
    from failure_aware_vision_amd import _lib, weights
    h = C.c_void_p()
    mask = weights.site_mask_for(1, "all_blocks")
    cases = [
        _cfg(lib, 1, conf_kind=2),                                                     # one pass, one member
        _cfg(lib, 1, conf_kind=2, n_samples=30, site_mask=mask, dropout_p=0.0),        # no dropout drawn: T = 1
        _cfg(lib, 1, conf_kind=2, n_samples=30, site_mask=0, dropout_p=0.1),           # no active site
        _cfg(lib, 1, conf_kind=2, n_samples=30, site_mask=mask, dropout_p=0.001),      # round(256 p) = 0
        _cfg(lib, 1, conf_kind=2, n_samples=1, site_mask=mask, dropout_p=0.1),         # T = 1
        _cfg(lib, 1, conf_kind=2, n_samples=30, site_mask=mask, dropout_p=0.1, num_classes=1),
        _cfg(lib, _lib.ARCH_VIT_TINY, conf_kind=2),                                    # ViT: single pass
    ]
    for c in cases:
        assert lib.fav_create(C.byref(c), C.byref(h)) == 1
        assert b"mutual information" in lib.fav_last_error(None)
    assert lib.fav_create(C.byref(_cfg(lib, 1, conf_kind=3)), C.byref(h)) == 1


def test_create_accepts_mutual_info_with_samples_up_to_the_device_probe(lib):
    import torch
    if torch.cuda.is_available():
        pytest.skip("GPU present")
    from failure_aware_vision_amd import weights
    h = C.c_void_p()
    mc = _cfg(lib, 1, conf_kind=2, n_samples=30, site_mask=weights.site_mask_for(1, "all_blocks"), dropout_p=0.1)
    assert lib.fav_create(C.byref(mc), C.byref(h)) == 5
    assert b"no CPU fallback" in lib.fav_last_error(None)
    ens = _cfg(lib, 1, conf_kind=2, n_members=5)
    assert lib.fav_create(C.byref(ens), C.byref(h)) == 5


def test_reference_identical_samples_have_no_mutual_information():
    rng = np.random.default_rng(3)
    one = (rng.standard_normal((1, 4, 50)) * 3).astype(np.float32)
    r = head_uncertainty(np.repeat(one, 7, axis=0), temperature=1.0, kind=2)
    np.testing.assert_allclose(r["mutual_info"], 0.0, atol=1e-12)
    np.testing.assert_allclose(r["pred_entropy"], r["expected_entropy"], atol=1e-12)
    assert np.array_equal(r["agreement"], np.ones(4)) and np.allclose(r["prob_std"], 0.0)
    np.testing.assert_allclose(r["confidence"], 1.0)
    single = head_uncertainty(one, kind=2)          # T = 1: the same, by definition
    assert np.array_equal(single["agreement"], np.ones(4)) and np.all(single["mutual_info"] == 0)


@pytest.mark.parametrize("T,Cc", [(2, 10), (5, 10), (10, 10), (7, 1000)])
def test_reference_one_hot_samples_on_distinct_classes(T, Cc):
    lg = np.zeros((T, 1, Cc), np.float32)
    for t in range(T):
        lg[t, 0, (3 * t + 1) % Cc] = 1e4            # p_t one-hot (exp(-1e4) = 0 in float64)
    r = head_uncertainty(lg, kind=2)
    assert abs(r["mutual_info"][0] - math.log(T)) < 1e-12 and abs(r["pred_entropy"][0] - math.log(T)) < 1e-12
    assert r["expected_entropy"][0] == 0.0
    assert abs(r["confidence"][0]) < 1e-12
    assert r["agreement"][0] == 1.0 / T
    assert r["label"][0] == min((3 * t + 1) % Cc for t in range(T))      # tie over T classes: lowest index
    assert list(r["top_label"][0][:min(5, T)]) == sorted((3 * t + 1) % Cc for t in range(T))[:5]


def test_reference_top5_pads_past_num_classes():
    r = head_uncertainty(np.array([[[0.0, 2.0, 2.0]]], np.float32))
    assert list(r["top_label"][0]) == [1, 2, 0, -1, -1] and list(r["top_prob"][0][3:]) == [0.0, 0.0]


def _known_records(n=6):
    rng = np.random.default_rng(11)
    f = {"label": rng.integers(0, 1000, n), "top_label": rng.integers(-1, 1000, (n, 5)),
         "top_prob": rng.random((n, 5)).astype(np.float32)}
    for name in FLOAT_FIELDS:
        f[name] = rng.standard_normal(n).astype(np.float32)
    f["prob_std"][0] = -0.0                         # bits, not values: -0 must stay -0
    return f, pack_records(f)


def _check_unpacked(u, f, to_np):
    assert set(u) == set(FIELDS)
    assert np.array_equal(to_np(u["label"]), f["label"].astype(np.int32))
    assert np.array_equal(to_np(u["top_label"]), f["top_label"].astype(np.int32))
    for name in FLOAT_FIELDS:
        a = to_np(u[name])
        assert a.dtype == np.float32 and np.array_equal(a.view(np.int32), f[name].view(np.int32)), name
    assert np.array_equal(to_np(u["top_prob"]).view(np.int32), f["top_prob"].view(np.int32))


def test_unpack_uncertainty_round_trips_known_bits():
    import torch
    from failure_aware_vision_amd import unpack_uncertainty
    f, rec = _known_records()
    _check_unpacked(unpack_uncertainty(rec), f, lambda a: np.ascontiguousarray(a))
    t = torch.from_numpy(rec.copy())
    u = unpack_uncertainty(t)
    _check_unpacked(u, f, lambda a: a.contiguous().numpy())
    assert u["confidence"].data_ptr() == t.data_ptr() + 4        # views of the record buffer, nothing copied
    with pytest.raises(ValueError):
        unpack_uncertainty(rec[:, :17])
    with pytest.raises(TypeError):
        unpack_uncertainty(rec.astype(np.int64))


_WORKER = r"""
import os, sys
sys.path.insert(0, {root!r}); sys.path.insert(0, {tests!r})
import numpy as np, torch, torch.distributed as dist
from failure_aware_vision_amd import classify_sharded, shard_range, unpack_uncertainty
from uncertainty_ref import head_uncertainty, pack_records
rank, world = int(os.environ["RANK"]), int(os.environ["WORLD_SIZE"])
dist.init_process_group("gloo", rank=rank, world_size=world)
for n in (11, 8):
    lg = (np.random.default_rng(5).standard_normal((4, n, 20)) * 3).astype(np.float32)
    full = pack_records(head_uncertainty(lg, kind=1))
    def stand_in(local, first_index=0):   # plays Backend.classify_uncertainty: records of global frames [first, first + len)
        assert np.array_equal(local, np.arange(first_index, first_index + local.shape[0]))
        return full[first_index:first_index + local.shape[0]]
    s, e = shard_range(n, rank, world)
    got = classify_sharded(stand_in, np.arange(s, e), n, rank, world, detail=True)
    ref = unpack_uncertainty(torch.from_numpy(full))
    assert set(got) == set(ref)
    for k in ref:
        assert torch.equal(got[k].contiguous().view(torch.int32), ref[k].contiguous().view(torch.int32)), (n, k)
    labels, conf = classify_sharded(lambda f, first_index=0: (torch.from_numpy(full[first_index:first_index + f.shape[0], 0]),
                                    torch.from_numpy(full[first_index:first_index + f.shape[0], 1].view(np.float32))),
                                    np.arange(s, e), n, rank, world)          # the 8-byte default path alongside
    assert torch.equal(labels, ref["label"]) and torch.equal(conf, ref["confidence"])
dist.barrier(); dist.destroy_process_group()
print("rank", rank, "ok")
"""


def test_sharded_detail_gloo_world2(tmp_path):
    script = tmp_path / "worker.py"
    script.write_text(_WORKER.format(root=ROOT, tests=os.path.join(ROOT, "tests")))
    env = dict(os.environ, MASTER_ADDR="127.0.0.1", MASTER_PORT="29547", WORLD_SIZE="2", OMP_NUM_THREADS="2")
    procs = [subprocess.Popen([sys.executable, str(script)], env=dict(env, RANK=str(r)), stdout=subprocess.PIPE,
                              stderr=subprocess.STDOUT) for r in range(2)]
    try:
        outs = [p.communicate(timeout=300)[0].decode() for p in procs]
    finally:
        for p in procs:
            if p.poll() is None:
                p.kill()
    for p, o in zip(procs, outs):
        assert p.returncode == 0, o
