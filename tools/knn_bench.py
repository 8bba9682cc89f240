"""Time Backend.classify_knn against Backend.classify on the same handle: ResNet-50, single pass, 224 x 224, 256 frames a call,
with banks of N = 4096, 65536 and 262144 rows and k = 10 and 100.  The bank is random unit rows: the head's time does not
depend on the values (the radix select makes four passes whatever they are).  What the difference pays for: the
device-to-device copies of the tapped rows and the head's three launches.

One process; every figure is the median [min, max] over --rounds rounds, in which the two calls alternate, of (HIP-event
time of --reps back-to-back calls) / reps, after --warmup calls.  The three launches are timed apart, in a fresh child process
per (N, k) under `rocprofv3 --kernel-trace --stats` that runs fav_op_knn_score alone on features of the same shape (--child);
tracing slows the host, so its figures are kernel times only.  There is no pass / fail threshold; the output file is the record.

    python tools/knn_bench.py [--out profiles/knn_bench.txt] [--rows 4096,65536,262144] [--k 10,100] [--no-kernels]"""
import argparse
import csv
import glob
import os
import statistics
import subprocess
import sys
import tempfile

import numpy as np
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
from failure_aware_vision_amd import Backend, _lib  # noqa: E402
from failure_aware_vision_amd.ood import KNNBank  # noqa: E402

D = 2048
KERNELS = (("query", "knn_query_kernel"), ("gemm", "conv_igemm_kernel"), ("select", "knn_select_kernel"))


def random_bank_bits(N, seed=0):
    """uint16 [N, D] on the device: random unit rows as bf16 bit patterns."""
    g = torch.Generator("cuda").manual_seed(seed)
    out = torch.empty((N, D), dtype=torch.bfloat16, device="cuda")
    for b in range(0, N, 65536):
        x = torch.randn((min(65536, N - b), D), device="cuda", generator=g)
        out[b:b + x.shape[0]] = (x / x.norm(dim=1, keepdim=True)).to(torch.bfloat16)
    return out.view(torch.int16)


def child(N, k, n, reps):
    """fav_op_knn_score alone, reps times after one warm-up call: what a kernel trace of this process holds is the head."""
    lib = _lib.load()
    bank = random_bank_bits(N)
    feat = torch.randn((1, n, D), device="cuda").to(torch.bfloat16)
    ws = torch.empty(lib.fav_knn_workspace_bytes(n, D, N), dtype=torch.uint8, device="cuda")
    rec = torch.empty((n, 6), dtype=torch.int32, device="cuda")
    for _ in range(reps + 1):
        st = lib.fav_op_knn_score(feat.data_ptr(), 1, n, D, bank.data_ptr(), N, k, None, float("inf"), ws.data_ptr(), ws.numel(),
                                  rec.data_ptr(), torch.cuda.current_stream().cuda_stream)
        assert st == 0, lib.fav_last_error(None)
    torch.cuda.synchronize()


def kernel_times(N, k, n, reps):
    """-> {launch: average microseconds} from a child process under rocprofv3, None where the trace has no such kernel."""
    with tempfile.TemporaryDirectory() as d:
        cmd = ["rocprofv3", "--kernel-trace", "--stats", "--output-format", "csv", "-d", d, "--", sys.executable, os.path.abspath(__file__),
               "--child", f"{N},{k}", "--n", str(n), "--reps", str(reps)]
        r = subprocess.run(cmd, stdout=subprocess.PIPE, stderr=subprocess.STDOUT, text=True, timeout=300)
        files = glob.glob(os.path.join(d, "**", "*kernel_stats.csv"), recursive=True)
        if r.returncode != 0 or not files:
            raise SystemExit(f"the kernel trace of N={N}, k={k} failed (exit status {r.returncode}):\n{r.stdout[-2000:]}")
        print(f"traced N={N} k={k}", file=sys.stderr, flush=True)
        rows = list(csv.DictReader(open(files[0])))
    out = {}
    for key, name in KERNELS:
        hit = [r for r in rows if name in r.get("Name", "")]
        # the first call is the warm-up: its launch is in the average too, one of reps + 1
        out[key] = sum(float(r["TotalDurationNs"]) for r in hit) / sum(int(r["Calls"]) for r in hit) / 1e3 if hit else None
    return out


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--rows", default="4096,65536,262144")
    ap.add_argument("--k", default="10,100")
    ap.add_argument("--n", type=int, default=256)
    ap.add_argument("--reps", type=int, default=3)
    ap.add_argument("--rounds", type=int, default=5)
    ap.add_argument("--warmup", type=int, default=2)
    ap.add_argument("--no-kernels", action="store_true", help="skip the per-launch kernel traces")
    ap.add_argument("--child", default=None, help=argparse.SUPPRESS)
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "knn_bench.txt"))
    args = ap.parse_args()
    rows_list = [int(v) for v in args.rows.split(",")]
    k_list = [int(v) for v in args.k.split(",")]
    # the traces first, before this process touches the device: the child processes never share it with this one's handle
    traces = {}
    if not args.child and not args.no_kernels:
        for N in rows_list:
            for k in k_list:
                traces[N, k] = kernel_times(N, k, args.n, args.reps)
    if not torch.cuda.is_available():
        raise SystemExit("knn_bench needs a gfx950 GPU; a CPU run measures nothing")
    if args.child:
        N, k = (int(v) for v in args.child.split(","))
        return child(N, k, args.n, args.reps)

    def rounds_of(calls):
        for launch in calls.values():
            for _ in range(args.warmup):
                launch()
        torch.cuda.synchronize()
        ms = {k: [] for k in calls}
        for _ in range(args.rounds):
            for k, launch in calls.items():
                e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
                e0.record()
                for _ in range(args.reps):
                    launch()
                e1.record()
                e1.synchronize()
                ms[k].append(e0.elapsed_time(e1) / args.reps)
        return {k: (statistics.median(v), min(v), max(v)) for k, v in ms.items()}

    lines = [f"classify_knn against classify, ResNet-50 single pass, {args.n} frames of 224 x 224 a call, D = {D}, {torch.cuda.get_device_name(0)}",
             f"median [min, max] ms per call of {args.rounds} rounds of {args.reps} back-to-back calls (HIP events), {args.warmup} "
             "warm-up calls; the two calls alternate inside a round; 'classify (tap on)' is the plain call on the handle that holds "
             "the bank",
             "query / gemm / select: average kernel time in microseconds of the head's three launches, rocprofv3 --kernel-trace --stats "
             f"of a child process that runs fav_op_knn_score alone ({args.reps} + 1 calls)",
             "", f"{'N':>8}{'k':>5}{'classify (tap on) ms':>30}{'classify_knn ms':>30}{'difference ms':>15}{'ratio':>9}"
                 f"{'query us':>10}{'gemm us':>10}{'select us':>11}"]
    g = torch.Generator("cuda").manual_seed(3)
    frames = torch.randint(0, 256, (args.n, 224, 224, 3), dtype=torch.uint8, device="cuda", generator=g)
    be = Backend(arch="resnet50", max_batch=args.n)
    base = rounds_of({"classify": lambda: be.classify(frames)})["classify"]
    lines.append(f"{'-':>8}{'-':>5}{f'{base[0]:.3f} [{base[1]:.3f}, {base[2]:.3f}] (off)':>30}")
    for N in rows_list:
        bits = random_bank_bits(N).cpu().numpy().view(np.uint16)
        for k in k_list:
            be.set_knn(KNNBank(bits, k=k, threshold=1.0))
            r = rounds_of({"classify": lambda: be.classify(frames), "knn": lambda: be.classify_knn(frames)})
            c, o = r["classify"], r["knn"]
            t = traces.get((N, k), {})
            us = "".join(f"{'-' if t.get(key) is None else format(t[key], '.1f'):>{w}}" for key, w in (("query", 10), ("gemm", 10), ("select", 11)))
            lines.append(f"{N:>8}{k:>5}{f'{c[0]:.3f} [{c[1]:.3f}, {c[2]:.3f}]':>30}{f'{o[0]:.3f} [{o[1]:.3f}, {o[2]:.3f}]':>30}"
                         f"{o[0] - c[0]:>15.3f}{o[0] / c[0]:>9.4f}{us}")
        be.set_knn(None)
    be.close()
    text = "\n".join(lines) + "\n"
    os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
    with open(args.out, "w") as f:
        f.write(text)
    print(text)


if __name__ == "__main__":
    main()
