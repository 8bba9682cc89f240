"""CPU-side checks of the conformal prediction-set head's interface: the fav_conformal / fav_pred_set layouts (C vs
ctypes), the new symbols, calibrate_qhat, unpack_sets, the tests' own float64 reference (conformal_ref.py) on cases with
known answers, fav_op_head_sets' rejection of a bad fav_conformal before any launch, and the sets=... shard / gather
logic under a 2-rank gloo group with a stand-in classifier."""
import ctypes as C
import math
import os
import subprocess
import sys

import numpy as np
import pytest

from conformal_ref import draws, pbar_of, prediction_sets, qhat_of, scores

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


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
    printf("set_size %zu\n", sizeof(fav_pred_set));
    printf("cp_size %zu\n", sizeof(fav_conformal));
#define F(x) printf("set.%s %zu\n", #x, offsetof(fav_pred_set, x));
    F(label) F(confidence) F(set_size) F(set_mass) F(u) F(reserved) F(member)
#define G(x) printf("cp.%s %zu\n", #x, offsetof(fav_conformal, x));
    G(struct_size) G(score_kind) G(randomized) G(k_reg) G(lambda) G(qhat) G(seed)
    printf("lac %d\naps %d\n", (int)FAV_CP_LAC, (int)FAV_CP_APS);
    return 0;
}
"""


def test_layouts_match_ctypes_and_symbols_exported(lib, tmp_path):
    from failure_aware_vision_amd import _lib
    src = tmp_path / "layout.c"
    src.write_text(_LAYOUT_C)
    exe = str(tmp_path / "layout")
    subprocess.check_call(["gcc", "-std=c99", "-Wall", "-Werror", "-I" + os.path.join(ROOT, "include"), str(src), "-o", exe])
    out = dict(line.split() for line in subprocess.check_output([exe], text=True).splitlines())
    assert int(out["set_size"]) == 160 == C.sizeof(_lib.FavPredSet)
    assert int(out["cp_size"]) == 32 == C.sizeof(_lib.FavConformal)
    for name in ("label", "confidence", "set_size", "set_mass", "u", "reserved", "member"):
        assert int(out["set." + name]) == getattr(_lib.FavPredSet, name).offset, name
    for name in ("struct_size", "score_kind", "randomized", "k_reg", "lambda", "qhat", "seed"):
        assert int(out["cp." + name]) == getattr(_lib.FavConformal, "lambda_" if name == "lambda" else name).offset, name
    assert (int(out["lac"]), int(out["aps"])) == (_lib.CP_LAC, _lib.CP_APS) == (0, 1)
    for sym in ("fav_classify_sets", "fav_conformal_scores", "fav_op_head_sets"):
        assert hasattr(lib, sym), sym
    assert lib.fav_abi_version() == 2


def test_calibrate_qhat():
    from failure_aware_vision_amd import calibrate_qhat
    # n = 5, alpha = 0.1: ceil(6 * 0.9) = 6 > 5 -> inf; alpha = 0.5: ceil(3) = 3rd smallest
    s = np.array([0.9, 0.1, 0.5, 0.3, 0.7], np.float32)
    assert calibrate_qhat(s, 0.1) == math.inf
    assert calibrate_qhat(s, 0.5) == np.float32(0.5)
    # n = 19, alpha = 0.1: ceil(20 * 0.9) = 18th smallest
    s = np.random.default_rng(3).permutation(np.arange(19, dtype=np.float32))
    assert calibrate_qhat(s, 0.1) == 17.0 == qhat_of(s, 0.1)
    assert calibrate_qhat(s, 0.05) == 18.0                      # ceil(20 * 0.95) = 19: the largest
    assert calibrate_qhat(s, 0.04) == math.inf                  # ceil(20 * 0.96) = 20 > 19
    for bad in (0.0, 1.0, -0.1, 1.5):
        with pytest.raises(ValueError):
            calibrate_qhat(s, bad)
    with pytest.raises(ValueError, match="NaN"):
        calibrate_qhat(np.array([0.1, np.nan, 0.2], np.float32), 0.5)
    with pytest.raises(ValueError):
        calibrate_qhat(np.array([], np.float32), 0.5)


def _known_records(n=4):
    rng = np.random.default_rng(7)
    rec = np.zeros((n, 40), np.int32)
    rec[:, 0] = rng.integers(0, 1000, n)
    rec[:, 1] = rng.random(n).astype(np.float32).view(np.int32)
    rec[:, 3] = rng.random(n).astype(np.float32).view(np.int32)
    rec[:, 4] = rng.random(n).astype(np.float32).view(np.int32)
    members = rng.random((n, 1000)) < 0.05
    members[0, [0, 31, 32, 999]] = True                          # word edges and bit 31 (the sign bit of an int32 word)
    words = np.zeros((n, 32), np.uint32)
    for c in range(1000):
        words[:, c // 32] |= members[:, c].astype(np.uint32) << np.uint32(c % 32)
    rec[:, 8:40] = words.view(np.int32)
    rec[:, 2] = members.sum(axis=1)
    return rec, members


def test_unpack_sets_round_trips_known_bits():
    import torch
    from failure_aware_vision_amd import unpack_sets
    rec, members = _known_records()
    u = unpack_sets(rec, 1000)
    assert np.array_equal(u["members"], members) and u["members"].dtype == bool
    assert np.array_equal(u["set_size"], members.sum(axis=1))
    assert np.array_equal(u["label"], rec[:, 0])
    for i, k in ((1, "confidence"), (3, "set_mass"), (4, "u")):
        assert u[k].dtype == np.float32 and np.array_equal(u[k].view(np.int32), rec[:, i]), k
    t = unpack_sets(torch.from_numpy(rec.copy()), 1000)
    assert np.array_equal(t["members"].numpy(), members)
    assert t["confidence"].dtype == torch.float32 and np.array_equal(t["confidence"].contiguous().view(torch.int32).numpy(), rec[:, 1])
    assert unpack_sets(rec)["members"].shape == (4, 1024)
    with pytest.raises(ValueError):
        unpack_sets(rec[:, :39])
    with pytest.raises(TypeError):
        unpack_sets(rec.astype(np.int64))


def test_reference_sets_grow_with_qhat_and_are_prefixes():
    rng = np.random.default_rng(5)
    lg = (rng.standard_normal((6, 16, 40)) * 3).astype(np.float32)
    pb = pbar_of(lg)
    for kw in (dict(kind="lac"), dict(kind="aps"), dict(kind="aps", randomized=True, seed=9),
               dict(kind="aps", lam=0.05, k_reg=2)):
        s, u, order, rank = scores(pb, **kw)
        prev = np.zeros_like(s, bool)
        for q in (-1.0, 0.2, 0.5, 0.8, 0.95, 1.0, 1.5, math.inf):
            m = prediction_sets(s, q)
            assert np.all(m >= prev)                            # nested in qhat
            prev = m
            k = m.sum(axis=1)
            by_rank = np.take_along_axis(m, order, axis=1)
            assert np.all(by_rank == (np.arange(40)[None, :] < k[:, None])), kw       # a prefix of the sort order
        assert prev.all()                                       # qhat = inf: every class
    s, u, _, _ = scores(pb, kind="aps", randomized=True, seed=9)
    assert np.all((u >= 0) & (u < 1)) and len(set(u.tolist())) == 16


def test_reference_lac_is_the_pbar_threshold_set():
    pb = pbar_of((np.random.default_rng(1).standard_normal((3, 8, 25)) * 2).astype(np.float32))
    s, _, _, _ = scores(pb, kind="lac")
    for q in (0.5, 0.9, 0.99):
        assert np.array_equal(prediction_sets(s, q), pb >= 1.0 - q)


def test_reference_draw_is_keyed_by_global_frame():
    a = draws(123, np.arange(10))
    b = draws(123, np.arange(4, 10))
    assert np.array_equal(a[4:], b) and not np.array_equal(a, draws(124, np.arange(10)))


def test_op_rejects_bad_conformal_before_any_launch(lib):
    """fav_op_head_sets checks cp on the host, before touching any pointer: the dummy addresses are never dereferenced."""
    from failure_aware_vision_amd import _lib

    def cp(**kw):
        c = _lib.FavConformal()
        c.struct_size, c.score_kind, c.qhat = C.sizeof(_lib.FavConformal), _lib.CP_APS, 0.9
        for k, v in kw.items():
            setattr(c, k, v)
        return c

    bad = [cp(struct_size=28), cp(struct_size=0), cp(qhat=float("nan")), cp(lambda_=-0.1), cp(lambda_=float("inf")),
           cp(lambda_=float("nan")), cp(k_reg=-1), cp(score_kind=_lib.CP_LAC, randomized=1),
           cp(score_kind=_lib.CP_LAC, lambda_=0.1), cp(score_kind=2), cp(randomized=2)]
    fake = 0x1000
    for c in bad:
        st = lib.fav_op_head_sets(fake, 2, 1, 10, 16, 1.0, 0, 0.5, 0, C.byref(c), None, None, fake, None, None, None)
        assert st == 1
        assert b"conformal" in lib.fav_last_error(None)
    assert lib.fav_op_head_sets(fake, 2, 1, 10, 16, 1.0, 0, 0.5, 0, None, None, None, fake, None, None, None) == 1
    good = cp()
    # shape / buffer misuse, also before any launch
    assert lib.fav_op_head_sets(fake, 2, 1, 1025, 1028, 1.0, 0, 0.5, 0, C.byref(good), None, None, fake, None, None, None) == 1
    assert lib.fav_op_head_sets(fake, 2, 1, 10, 16, 1.0, 0, 0.5, 0, C.byref(good), None, None, fake + 4, None, None, None) == 1
    assert lib.fav_op_head_sets(fake, 2, 1, 10, 16, 1.0, 0, 0.5, 0, C.byref(good), None, None, None, None, None, None) == 1
    assert lib.fav_op_head_sets(fake, 2, 1, 10, 16, 1.0, 0, 0.5, 0, C.byref(good), fake, None, None, None, None, None) == 1
    assert lib.fav_op_head_sets(fake, 2, 1, 10, 16, 1.0, 3, 0.5, 0, C.byref(good), None, None, fake, None, None, None) == 1
    assert lib.fav_op_head_sets(fake, 2, 1, 10, 16, 1.0, 0, 0.5, -1, C.byref(good), None, None, fake, None, None, None) == 1


def test_conformal_dataclass_to_c():
    from failure_aware_vision_amd import Conformal, _lib
    c = Conformal(kind="raps", randomized=True, lam=0.01, k_reg=5, qhat=0.7, seed=2 ** 40 + 3).to_c()
    assert (c.struct_size, c.score_kind, c.randomized, c.k_reg) == (32, _lib.CP_APS, 1, 5)
    assert c.lambda_ == np.float32(0.01) and c.qhat == np.float32(0.7) and c.seed == 2 ** 40 + 3
    assert math.isinf(Conformal().to_c().qhat)
    with pytest.raises(ValueError):
        Conformal(kind="thr").to_c()


_WORKER = r"""
import os, sys
sys.path.insert(0, {root!r}); sys.path.insert(0, {tests!r})
import numpy as np, torch, torch.distributed as dist
from failure_aware_vision_amd import Conformal, classify_sharded, shard_range, unpack_sets
rank, world = int(os.environ["RANK"]), int(os.environ["WORLD_SIZE"])
dist.init_process_group("gloo", rank=rank, world_size=world)
rng = np.random.default_rng(5)
for n in (11, 8):
    full = rng.integers(-2 ** 31, 2 ** 31 - 1, (n, 40)).astype(np.int32)
    def stand_in(local, first_index=0):   # plays Backend.classify_sets: records of global frames [first, first + len)
        assert np.array_equal(local, np.arange(first_index, first_index + local.shape[0]))
        return full[first_index:first_index + local.shape[0]]
    s, e = shard_range(n, rank, world)
    got = classify_sharded(stand_in, np.arange(s, e), n, rank, world, sets=Conformal(qhat=0.9))
    ref = unpack_sets(torch.from_numpy(full))
    assert set(got) == set(ref)
    for k in ref:
        a, b = got[k].contiguous(), ref[k].contiguous()
        assert torch.equal(a if a.dtype == torch.bool else a.view(torch.int32),
                           b if b.dtype == torch.bool else b.view(torch.int32)), (n, k)
dist.barrier(); dist.destroy_process_group()
print("rank", rank, "ok")
"""


def test_sharded_sets_gloo_world2(tmp_path):
    script = tmp_path / "worker.py"
    script.write_text(_WORKER.format(root=ROOT, tests=os.path.join(ROOT, "tests")))
    env = dict(os.environ, MASTER_ADDR="127.0.0.1", MASTER_PORT="29557", WORLD_SIZE="2", OMP_NUM_THREADS="2")
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
