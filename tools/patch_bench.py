"""Time Backend.classify_patch against Backend.classify on the same handle: ResNet-50, single pass, 224 x 224, 256 frames a
call (12 544 cells of a 7 x 7 x 2048 map), with patch banks of N = 4096, 16384 and 65536 rows.  The bank is random unit rows:
the head's time does not depend on the values.  What the difference pays for: the head's launches - the query kernel, per
column chunk of the bank a GEMM and a fold, the score kernel.  The map tap is on for both calls, so its copies are in both.

One process; every figure is the median [min, max] over --rounds rounds, in which the two calls alternate, of (HIP-event
time of --reps back-to-back calls) / reps, after --warmup calls.  The launches are timed apart, in a fresh child process per N
under `rocprofv3 --kernel-trace --stats` that runs fav_op_patch_score alone on maps of the same shape (--child); tracing slows
the host, so its figures are kernel times only, summed over the launches of ONE call (a call has one GEMM and one fold a
chunk).  There is no pass / fail threshold; the output file is the record.

    python tools/patch_bench.py [--out profiles/patch_bench.txt] [--rows 4096,16384,65536] [--chunk-rows 0] [--no-kernels]"""
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
from failure_aware_vision_amd.patch import PatchBank  # noqa: E402

HF = WF = 7
D = 2048
KERNELS = (("query", "knn_query_kernel"), ("gemm", "conv_igemm_kernel"), ("fold", "patch_fold_kernel"), ("score", "patch_score_kernel"))


def random_bank_bits(N, seed=0):
    """uint16 [N, D] on the device: random unit rows as bf16 bit patterns."""
    g = torch.Generator("cuda").manual_seed(seed)
    out = torch.empty((N, D), dtype=torch.bfloat16, device="cuda")
    for b in range(0, N, 65536):
        x = torch.randn((min(65536, N - b), D), device="cuda", generator=g)
        out[b:b + x.shape[0]] = (x / x.norm(dim=1, keepdim=True)).to(torch.bfloat16)
    return out.view(torch.int16)


def child(N, n, reps, chunk_rows):
    """fav_op_patch_score alone, reps times after one warm-up call: what a kernel trace of this process holds is the head."""
    lib = _lib.load()
    bank = random_bank_bits(N)
    maps = torch.randn((1, n, HF * WF, D), device="cuda").to(torch.bfloat16)
    ws = torch.empty(lib.fav_patch_workspace_bytes(n * HF * WF, D, N, chunk_rows), dtype=torch.uint8, device="cuda")
    dist = torch.empty((n, HF * WF), dtype=torch.float32, device="cuda")
    row = torch.empty((n, HF * WF), dtype=torch.int32, device="cuda")
    rec = torch.empty((n, 8), dtype=torch.int32, device="cuda")
    for _ in range(reps + 1):
        st = lib.fav_op_patch_score(maps.data_ptr(), 1, n, HF, WF, D, bank.data_ptr(), N, chunk_rows, float("inf"), ws.data_ptr(),
                                    ws.numel(), dist.data_ptr(), row.data_ptr(), rec.data_ptr(), torch.cuda.current_stream().cuda_stream)
        assert st == 0, lib.fav_last_error(None)
    torch.cuda.synchronize()


def kernel_times(N, n, reps, chunk_rows):
    """-> {launch: microseconds a call, summed over its launches} from a child process under rocprofv3, None where the trace has
    no such kernel."""
    with tempfile.TemporaryDirectory() as d:
        cmd = ["rocprofv3", "--kernel-trace", "--stats", "--output-format", "csv", "-d", d, "--", sys.executable, os.path.abspath(__file__),
               "--child", str(N), "--n", str(n), "--reps", str(reps), "--chunk-rows", str(chunk_rows)]
        r = subprocess.run(cmd, stdout=subprocess.PIPE, stderr=subprocess.STDOUT, text=True, timeout=300)
        files = glob.glob(os.path.join(d, "**", "*kernel_stats.csv"), recursive=True)
        if r.returncode != 0 or not files:
            raise SystemExit(f"the kernel trace of N={N} failed (exit status {r.returncode}):\n{r.stdout[-2000:]}")
        print(f"traced N={N}", file=sys.stderr, flush=True)
        rows = list(csv.DictReader(open(files[0])))
    out = {}
    for key, name in KERNELS:
        hit = [r for r in rows if name in r.get("Name", "")]
        # the first call is the warm-up: its launches are in the sum too, one call of reps + 1
        out[key] = sum(float(r["TotalDurationNs"]) for r in hit) / (reps + 1) / 1e3 if hit else None
    return out


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--rows", default="4096,16384,65536")
    ap.add_argument("--chunk-rows", type=int, default=0)
    ap.add_argument("--n", type=int, default=256)
    ap.add_argument("--reps", type=int, default=3)
    ap.add_argument("--rounds", type=int, default=5)
    ap.add_argument("--warmup", type=int, default=2)
    ap.add_argument("--no-kernels", action="store_true", help="skip the per-launch kernel traces")
    ap.add_argument("--child", default=None, help=argparse.SUPPRESS)
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "patch_bench.txt"))
    args = ap.parse_args()
    rows_list = [int(v) for v in args.rows.split(",")]
    # the traces first, before this process touches the device: the child processes never share it with this one's handle
    traces = {}
    if not args.child and not args.no_kernels:
        for N in rows_list:
            traces[N] = kernel_times(N, args.n, args.reps, args.chunk_rows)
    if not torch.cuda.is_available():
        raise SystemExit("patch_bench needs a gfx950 GPU; a CPU run measures nothing")
    if args.child:
        return child(int(args.child), args.n, args.reps, args.chunk_rows)

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

    cells = args.n * HF * WF
    lines = [f"classify_patch against classify, ResNet-50 single pass, {args.n} frames of 224 x 224 a call, {cells} cells of a "
             f"{HF} x {WF} x {D} map, {torch.cuda.get_device_name(0)}",
             f"median [min, max] ms per call of {args.rounds} rounds of {args.reps} back-to-back calls (HIP events), {args.warmup} "
             "warm-up calls; the two calls alternate inside a round; 'classify (tap on)' is the plain call on the handle that holds "
             "the bank, its map tap on",
             "chunk: the bank rows a slab covers (fav_patch_chunk_rows) and the chunks a call makes of them; query / gemm / fold / "
             "score: kernel time in microseconds of one call, summed over its launches, rocprofv3 --kernel-trace --stats of a child "
             f"process that runs fav_op_patch_score alone ({args.reps} + 1 calls)",
             "", f"{'N':>8}{'chunk':>7}{'chunks':>7}{'classify (tap on) ms':>30}{'classify_patch ms':>30}{'difference ms':>15}{'ratio':>9}"
                 f"{'query us':>10}{'gemm us':>10}{'fold us':>10}{'score us':>10}"]
    g = torch.Generator("cuda").manual_seed(3)
    frames = torch.randint(0, 256, (args.n, 224, 224, 3), dtype=torch.uint8, device="cuda", generator=g)
    be = Backend(arch="resnet50", max_batch=args.n)
    base = rounds_of({"classify": lambda: be.classify(frames)})["classify"]
    lines.append(f"{'-':>8}{'-':>7}{'-':>7}{f'{base[0]:.3f} [{base[1]:.3f}, {base[2]:.3f}] (off)':>30}")
    be.set_map_tap(True)
    for N in rows_list:
        bits = random_bank_bits(N).cpu().numpy().view(np.uint16)
        be.set_patch_bank(PatchBank(bits, threshold=1.0, chunk_rows=args.chunk_rows))
        chunk = be.lib.fav_patch_chunk_rows(cells, N, args.chunk_rows)
        r = rounds_of({"classify": lambda: be.classify(frames), "patch": lambda: be.classify_patch(frames)})
        c, o = r["classify"], r["patch"]
        t = traces.get(N, {})
        us = "".join(f"{'-' if t.get(key) is None else format(t[key], '.1f'):>10}" for key, _ in KERNELS)
        lines.append(f"{N:>8}{chunk:>7}{-(-((N + 63) // 64 * 64) // chunk):>7}{f'{c[0]:.3f} [{c[1]:.3f}, {c[2]:.3f}]':>30}"
                     f"{f'{o[0]:.3f} [{o[1]:.3f}, {o[2]:.3f}]':>30}{o[0] - c[0]:>15.3f}{o[0] / c[0]:>9.4f}{us}")
    be.set_patch_bank(None)
    be.close()
    text = "\n".join(lines) + "\n"
    os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
    with open(args.out, "w") as f:
        f.write(text)
    print(text)


if __name__ == "__main__":
    main()
