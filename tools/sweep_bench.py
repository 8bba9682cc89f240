"""One launch of the temperature-sweep head at K = 32 temperatures against the 32 fav_op_head launches it replaces, on the GPU.

Random fp32 logits at (T, n, C) = (30, 256, 1000) (MC-Dropout headline), (1, 512, 1000) (ViT) and (5, 256, 1000)
(5-member ensemble), row stride 1024.  Per shape: warm-up, then ROUNDS rounds in which the two alternatives alternate;
each round times ITERS back-to-back repetitions between two HIP events (one repetition = one sweep launch, or the 32 head
launches).  Reported: median, min and max of the per-repetition time over the rounds, the ratio of the medians, whether the
spreads overlap, the sweep's GB/s on the algorithmic T C 4 bytes per frame, and next to each event time the time the host spent
enqueuing a repetition: where that equals the event time, the figure is the host's launch rate (32 ctypes calls), not GPU time -
which is still what a caller of the do-nothing alternative would wait for.

Prints one JSON line per shape (and writes them to --out)."""
import argparse
import ctypes as C
import json
import os
import statistics
import sys
import time

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
import numpy as np  # noqa: E402
import torch  # noqa: E402
from failure_aware_vision_amd import _lib  # noqa: E402
from failure_aware_vision_amd.calibration import temperature_grid  # noqa: E402

ap = argparse.ArgumentParser()
ap.add_argument("--rounds", type=int, default=10)
ap.add_argument("--iters", type=int, default=20)
ap.add_argument("--kind", type=int, default=0)
ap.add_argument("--out", default="")
a = ap.parse_args()
assert torch.cuda.is_available(), "sweep_bench needs a GPU"
lib = _lib.load()
lines = []
K = 32
temps = temperature_grid(0.25, 8.0, K)
temps_p = temps.ctypes.data_as(C.POINTER(C.c_float))


def time_reps(fn, iters):
    """-> (us per repetition between two HIP events, us per repetition the host spent enqueuing)."""
    e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    torch.cuda.synchronize()
    e0.record()
    h0 = time.perf_counter()
    for _ in range(iters):
        fn()
    h1 = time.perf_counter()
    e1.record()
    e1.synchronize()
    return e0.elapsed_time(e1) * 1e3 / iters, (h1 - h0) * 1e6 / iters


def stats(xs):
    return {"median": statistics.median(xs), "min": min(xs), "max": max(xs)}


for T, n, Cc in ((30, 256, 1000), (1, 512, 1000), (5, 256, 1000)):
    if a.kind == 2 and T < 2:
        continue                                 # mutual information needs T >= 2 samples
    ld = 1024
    rng = np.random.default_rng(1)
    lg = torch.from_numpy((rng.standard_normal((T, n, ld)) * 4).astype(np.float32)).cuda()
    y = torch.from_numpy(rng.integers(0, Cc, n).astype(np.int32)).cuda()
    labels = torch.empty((K, n), dtype=torch.int32, device="cuda")
    conf = torch.empty((K, n), dtype=torch.float32, device="cuda")
    cells = torch.empty((n, K, 4), dtype=torch.int32, device="cuda")
    stream = torch.cuda.current_stream().cuda_stream

    def sweep():
        return lib.fav_op_head_sweep(lg.data_ptr(), T, n, Cc, ld, temps_p, K, a.kind, y.data_ptr(), cells.data_ptr(), stream)

    def heads():
        st = 0
        for k in range(K):
            st |= lib.fav_op_head(lg.data_ptr(), T, n, Cc, ld, float(temps[k]), a.kind, 0.5, labels[k].data_ptr(),
                                  conf[k].data_ptr(), None, None, stream)
        return st
    for fn in (sweep, heads):
        _lib.check(fn())
        time_reps(fn, a.iters)                   # warm-up
    torch.cuda.synchronize()
    # the two alternatives compute the same labels and confidences
    c = cells.cpu().numpy()
    assert np.array_equal(c[:, :, 0].T, labels.cpu().numpy()) and np.array_equal(c[:, :, 1].T, conf.cpu().numpy().view(np.int32))
    ts, th, hs, hh = [], [], [], []
    for _ in range(a.rounds):
        g, h = time_reps(sweep, a.iters)
        ts.append(g); hs.append(h)
        g, h = time_reps(heads, a.iters)
        th.append(g); hh.append(h)
    ss, sh = stats(ts), stats(th)
    host_s, host_h = statistics.median(hs), statistics.median(hh)
    s = json.dumps({"measure": "sweep_vs_32_heads_us", "T": T, "n": n, "C": Cc, "K": K, "conf_kind": a.kind, "iters": a.iters,
                    "rounds": a.rounds, "sweep_1_launch": ss, "head_32_launches": sh,
                    "host_enqueue_us": {"sweep_1_launch": host_s, "head_32_launches": host_h},
                    # the 32-launch figure is the host's launch rate, not GPU time, when enqueuing takes as long as the events say
                    "head_32_launches_host_bound": host_h >= 0.9 * sh["median"],
                    "ratio_median_heads_over_sweep": sh["median"] / ss["median"],
                    "spreads_overlap": not (ss["max"] < sh["min"] or sh["max"] < ss["min"]),
                    "sweep_GBps_on_TC4_bytes": 4.0 * T * n * Cc / (ss["median"] * 1e-6) / 1e9,
                    "heads_GBps_on_K_TC4_bytes": K * 4.0 * T * n * Cc / (sh["median"] * 1e-6) / 1e9})
    print(s, flush=True)
    lines.append(s)

if a.out:
    os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
    with open(a.out, "w") as f:
        f.write("\n".join(lines) + "\n")
