"""The confidence head with and without conformal prediction sets, on the GPU.

(1) fav_op_head vs fav_op_head_uncertainty vs fav_op_head_sets (kind 0, records written; randomized APS, qhat 0.9) on
    random fp32 logits at (T, n, C) = (30, 256, 1000) (MC-Dropout headline) and (1, 512, 1000) (ViT): HIP events around
    ITERS back-to-back launches after warm-up, the three heads alternating for ROUNDS rounds; median and spread of the
    per-launch time.
(2) Backend.classify_detect vs Backend.classify_sets on the headline config (ResNet-50 224x224, MC-Dropout T = 30
    all_blocks p = 0.1, 256 severity-3 frames), alternating call by call, HIP events per call.

Prints one JSON line per measurement (and writes them to --out).  --e2e-rounds 0 skips (2); --ops 0 skips (1)."""
import argparse
import json
import os
import statistics
import sys

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
import numpy as np  # noqa: E402
import torch  # noqa: E402
from failure_aware_vision_amd import Backend, Conformal, _lib, synth  # noqa: E402
from failure_aware_vision_amd.corrupt import Corruptor  # noqa: E402

ap = argparse.ArgumentParser()
ap.add_argument("--ops", type=int, default=1)
ap.add_argument("--rounds", type=int, default=10)
ap.add_argument("--iters", type=int, default=50)
ap.add_argument("--e2e-rounds", type=int, default=15)
ap.add_argument("--out", default="")
a = ap.parse_args()
assert torch.cuda.is_available(), "sets_bench needs a GPU"
CP = Conformal(kind="aps", randomized=True, qhat=0.9, seed=1)
lib = _lib.load()
lines = []


def emit(d):
    s = json.dumps(d)
    print(s, flush=True)
    lines.append(s)


def time_launches(fn, iters):
    e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    e0.record()
    for _ in range(iters):
        fn()
    e1.record()
    e1.synchronize()
    return e0.elapsed_time(e1) * 1e3 / iters     # us per launch


def stats(xs):
    return {"median": statistics.median(xs), "min": min(xs), "max": max(xs)}


if a.ops:
    for T, n, Cc in ((30, 256, 1000), (1, 512, 1000)):
        ld = 1024
        rng = np.random.default_rng(1)
        lg = torch.from_numpy((rng.standard_normal((T, n, ld)) * 4).astype(np.float32)).cuda()
        labels = torch.empty(n, dtype=torch.int32, device="cuda")
        conf = torch.empty(n, dtype=torch.float32, device="cuda")
        fail = torch.empty(n, dtype=torch.uint8, device="cuda")
        score = torch.empty(n, dtype=torch.float32, device="cuda")
        rec = torch.empty((n, 18), dtype=torch.int32, device="cuda")
        srec = torch.empty((n, 40), dtype=torch.int32, device="cuda")
        cp = CP.to_c()
        stream = torch.cuda.current_stream().cuda_stream

        def head():
            return lib.fav_op_head(lg.data_ptr(), T, n, Cc, ld, 1.0, 0, 0.5, labels.data_ptr(), conf.data_ptr(), fail.data_ptr(),
                                   score.data_ptr(), stream)

        def unc():
            return lib.fav_op_head_uncertainty(lg.data_ptr(), T, n, Cc, ld, 1.0, 0, 0.5, rec.data_ptr(), fail.data_ptr(),
                                               score.data_ptr(), stream)

        def sets():
            return lib.fav_op_head_sets(lg.data_ptr(), T, n, Cc, ld, 1.0, 0, 0.5, 0, cp, None, None, srec.data_ptr(),
                                        fail.data_ptr(), score.data_ptr(), stream)
        for fn in (head, unc, sets):
            _lib.check(fn())
            time_launches(fn, a.iters)           # warm-up
        th, tu, ts = [], [], []
        for _ in range(a.rounds):
            th.append(time_launches(head, a.iters))
            tu.append(time_launches(unc, a.iters))
            ts.append(time_launches(sets, a.iters))
        sh, su, ss = stats(th), stats(tu), stats(ts)
        emit({"measure": "head_op_us", "T": T, "n": n, "C": Cc, "iters": a.iters, "rounds": a.rounds,
              "head_kernel": sh, "head_unc_kernel": su, "head_sets_kernel": ss, "sets_vs_head": ss["median"] / sh["median"],
              "sets_vs_unc": ss["median"] / su["median"]})

if a.e2e_rounds:
    from failure_aware_vision_amd import weights
    blob, _ = weights.make_synthetic("resnet50", seed=1)
    u8 = torch.from_numpy(synth.synthetic_frames_u8(256, 224, 224, seed=21)).cuda()
    frames = Corruptor(seed=3).gaussian(u8, 3)
    be = Backend("resnet50", blob, max_batch=256, n_samples=30, dropout_policy="all_blocks", dropout_p=0.1, seed=4)
    rec = torch.empty((256, 40), dtype=torch.int32, device="cuda")
    det = lambda: be.classify_detect(frames)                          # noqa: E731
    cls = lambda: be.classify_sets(frames, CP, out=rec)               # noqa: E731
    for fn in (det, cls, det, cls):
        fn()
    torch.cuda.synchronize()
    td, tu = [], []
    for _ in range(a.e2e_rounds):
        td.append(time_launches(det, 1) / 1e3)
        tu.append(time_launches(cls, 1) / 1e3)
    sd, su = stats(td), stats(tu)
    emit({"measure": "e2e_ms_per_call", "workload": "ResNet-50 224x224, MC-Dropout T=30 all_blocks p=0.1, 256 severity-3 frames",
          "calls_each": a.e2e_rounds, "classify_detect": sd, "classify_sets": su,
          "slowdown_pct_median": 100.0 * (su["median"] / sd["median"] - 1.0),
          "slowdown_pct_mean": 100.0 * (statistics.mean(tu) / statistics.mean(td) - 1.0)})
    be.close()

if a.out:
    os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
    with open(a.out, "w") as f:
        f.write("\n".join(lines) + "\n")
