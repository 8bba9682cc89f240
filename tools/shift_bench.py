"""Time Backend.classify_drift against Backend.classify on the same handle: ResNet-50, single pass, 224 x 224, 256 frames a
call - one window - with references of R = 256, 1024 and 2048 rows and P = 199 and 999 permutations, and one row at the
largest window, n = 1024.  The reference is random unit rows: the head's time does not depend on the values (the sort and
the gather make the same passes whatever they are).  What the difference pays for: the device-to-device copies of the tapped
rows and the head's six launches.

One process; every figure is the median [min, max] over --rounds rounds, in which the two calls alternate, of (HIP-event
time of --reps back-to-back calls) / reps, after --warmup calls.  The launches are timed apart, in a fresh child process per
row under `rocprofv3 --kernel-trace --stats` that runs fav_op_drift_test alone on features of the same shape (--child);
tracing slows the host, so its figures are kernel times only, and the op's GEMM is the whole pool against itself where the
handle's is the window's rows only.  There is no pass / fail threshold; the output file is the record.

    python tools/shift_bench.py [--out profiles/drift_bench.txt] [--rows 256,1024,2048] [--perms 199,999] [--no-kernels]"""
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
from failure_aware_vision_amd.ood import DriftReference  # noqa: E402

D = 2048
KERNELS = (("query", "knn_query_kernel"), ("gemm", "conv_igemm_kernel"), ("quant", "drift_quant_kernel"),
           ("rowsum", "drift_rowsum_kernel"), ("perm", "drift_perm_kernel"), ("final", "drift_final_kernel"))


def random_ref_bits(R, seed=0):
    """uint16 [R, D] on the device: random unit rows as bf16 bit patterns."""
    g = torch.Generator("cuda").manual_seed(seed)
    x = torch.randn((R, D), device="cuda", generator=g)
    return (x / x.norm(dim=1, keepdim=True)).to(torch.bfloat16).view(torch.int16)


def child(R, P, n, reps):
    """fav_op_drift_test alone, reps times after one warm-up call: what a kernel trace of this process holds is the head."""
    lib = _lib.load()
    ref = random_ref_bits(R)
    feat = torch.randn((1, n, D), device="cuda").to(torch.bfloat16)
    ws = torch.empty(lib.fav_drift_workspace_bytes(n, D, R, P), dtype=torch.uint8, device="cuda")
    rec = torch.empty((12,), dtype=torch.int32, device="cuda")
    for _ in range(reps + 1):
        st = lib.fav_op_drift_test(feat.data_ptr(), 1, n, D, ref.data_ptr(), R, P, 0, 0.01, ws.data_ptr(), ws.numel(), rec.data_ptr(),
                                   None, torch.cuda.current_stream().cuda_stream)
        assert st == 0, lib.fav_last_error(None)
    torch.cuda.synchronize()


def kernel_times(R, P, n, reps):
    """-> {launch: average microseconds} from a child process under rocprofv3, None where the trace has no such kernel."""
    with tempfile.TemporaryDirectory() as d:
        cmd = ["rocprofv3", "--kernel-trace", "--stats", "--output-format", "csv", "-d", d, "--", sys.executable, os.path.abspath(__file__),
               "--child", f"{R},{P}", "--n", str(n), "--reps", str(reps)]
        r = subprocess.run(cmd, stdout=subprocess.PIPE, stderr=subprocess.STDOUT, text=True, timeout=300)
        files = glob.glob(os.path.join(d, "**", "*kernel_stats.csv"), recursive=True)
        if r.returncode != 0 or not files:
            raise SystemExit(f"the kernel trace of R={R}, P={P}, n={n} failed (exit status {r.returncode}):\n{r.stdout[-2000:]}")
        print(f"traced R={R} P={P} n={n}", file=sys.stderr, flush=True)
        rows = list(csv.DictReader(open(files[0])))
    out = {}
    for key, name in KERNELS:
        hit = [r for r in rows if name in r.get("Name", "")]
        # the first call is the warm-up: its launch is in the average too, one of reps + 1
        out[key] = sum(float(r["TotalDurationNs"]) for r in hit) / sum(int(r["Calls"]) for r in hit) / 1e3 if hit else None
    return out


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--rows", default="256,1024,2048")
    ap.add_argument("--perms", default="199,999")
    ap.add_argument("--n", type=int, default=256)
    ap.add_argument("--big", default="1024,2048,999", help="n,R,P of the one row at the largest window; '' for none")
    ap.add_argument("--reps", type=int, default=3)
    ap.add_argument("--rounds", type=int, default=5)
    ap.add_argument("--warmup", type=int, default=2)
    ap.add_argument("--no-kernels", action="store_true", help="skip the per-launch kernel traces")
    ap.add_argument("--child", default=None, help=argparse.SUPPRESS)
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "drift_bench.txt"))
    args = ap.parse_args()
    cases = [(args.n, int(R), int(P)) for R in args.rows.split(",") for P in args.perms.split(",")]
    if args.big:
        cases.append(tuple(int(v) for v in args.big.split(",")))
    # the traces first, before this process touches the device: the child processes never share it with this one's handle
    traces = {}
    if not args.child and not args.no_kernels:
        for n, R, P in cases:
            traces[n, R, P] = kernel_times(R, P, n, args.reps)
    if not torch.cuda.is_available():
        raise SystemExit("shift_bench needs a gfx950 GPU; a CPU run measures nothing")
    if args.child:
        R, P = (int(v) for v in args.child.split(","))
        return child(R, P, args.n, args.reps)

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

    lines = [f"classify_drift against classify, ResNet-50 single pass, n frames of 224 x 224 a call, D = {D}, {torch.cuda.get_device_name(0)}",
             f"median [min, max] ms per call of {args.rounds} rounds of {args.reps} back-to-back calls (HIP events), {args.warmup} "
             "warm-up calls; the two calls alternate inside a round; 'classify (tap on)' is the plain call on the handle that holds "
             "the reference",
             "query .. final: average kernel time in microseconds of the head's six launches, rocprofv3 --kernel-trace --stats of a "
             f"child process that runs fav_op_drift_test alone ({args.reps} + 1 calls); its gemm and quant cover the whole pool, the "
             "handle's only the window's rows",
             "", f"{'n':>6}{'R':>6}{'P':>6}{'classify (tap on) ms':>30}{'classify_drift ms':>30}{'difference ms':>15}{'ratio':>9}"
                 + "".join(f"{key + ' us':>11}" for key, _ in KERNELS)]
    be, be_n = None, 0
    for n, R, P in cases:
        if be_n != n:
            if be is not None:
                be.close()
            g = torch.Generator("cuda").manual_seed(3)
            frames = torch.randint(0, 256, (n, 224, 224, 3), dtype=torch.uint8, device="cuda", generator=g)
            be, be_n = Backend(arch="resnet50", max_batch=n), n
            base = rounds_of({"classify": lambda: be.classify(frames)})["classify"]
            lines.append(f"{n:>6}{'-':>6}{'-':>6}{f'{base[0]:.3f} [{base[1]:.3f}, {base[2]:.3f}] (off)':>30}")
        be.set_drift(DriftReference(random_ref_bits(R).cpu().numpy().view(np.uint16), n_perm=P))
        r = rounds_of({"classify": lambda: be.classify(frames), "drift": lambda: be.classify_drift(frames)})
        c, o = r["classify"], r["drift"]
        t = traces.get((n, R, P), {})
        us = "".join(f"{'-' if t.get(key) is None else format(t[key], '.1f'):>11}" for key, _ in KERNELS)
        lines.append(f"{n:>6}{R:>6}{P:>6}{f'{c[0]:.3f} [{c[1]:.3f}, {c[2]:.3f}]':>30}{f'{o[0]:.3f} [{o[1]:.3f}, {o[2]:.3f}]':>30}"
                     f"{o[0] - c[0]:>15.3f}{o[0] / c[0]:>9.4f}{us}")
        be.set_drift(None)
    be.close()
    text = "\n".join(lines) + "\n"
    os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
    with open(args.out, "w") as f:
        f.write(text)
    print(text)


if __name__ == "__main__":
    main()
