"""Mid-level patch maps, measured: ResNet-50, single pass, 256 frames of 224 x 224 a call, a bank
of N = 16384 random unit rows (the head's time does not depend on the values) at stage 2 (28 x 28 x 512), stage 3 (14 x 14 x
1024) and stage 4 (7 x 7 x 2048), radius 1.

  1. classify against classify_patch a stage, on the handle that holds the bank, the stage tap on for both, with the launches
     of the head apart: kernel time of one call summed over its launches, from `rocprofv3 --kernel-trace --stats` of a fresh
     child process per stage that runs fav_op_patch_score_at alone on maps of the stage's shape.
  2. the query kernel against the bytes it must move - the map once in, q out - for radius 0, 1, 2 a stage; the yardstick is
     the device-to-device copy of tools/coreset_bench.py, here of the stage's own map (the same bytes read and written).
  3. radius 0 against the k-NN head's query kernel on the stage-2 maps: fav_op_patch_score (knn_query_kernel) and
     fav_op_patch_score_at(.., 0, ..) (patch_local_query_kernel<0>) alternate in one process against a bank of 64 rows, so that
     everything behind the query is one small GEMM, one fold and the score kernel in both; and fav_op_patch_query alone.

One process; every figure is the median [min, max] over --rounds rounds, in which the calls alternate, of (HIP-event time of
--reps back-to-back calls) / reps, after --warmup calls.  No pass / fail threshold; the output file is the record.

    python tools/patch_local_bench.py [--out profiles/patch_local_bench.txt] [--no-kernels]"""
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

STAGES = {2: (28, 28, 512), 3: (14, 14, 1024), 4: (7, 7, 2048)}
KERNELS = (("query", "patch_local_query_kernel"), ("gemm", "conv_igemm_kernel"), ("fold", "patch_fold_kernel"), ("score", "patch_score_kernel"))


def unit_rows(N, D, seed=0):
    g = torch.Generator("cuda").manual_seed(seed)
    x = torch.randn((N, D), device="cuda", generator=g)
    return (x / x.norm(dim=1, keepdim=True)).to(torch.bfloat16).view(torch.int16)


class Head:
    """fav_op_patch_score / fav_op_patch_score_at on random maps of a stage's shape, its buffers allocated once."""

    def __init__(self, lib, stage, n, N):
        self.lib, (self.hf, self.wf, self.c), self.n, self.N = lib, STAGES[stage], n, N
        hw = self.hf * self.wf
        self.bank = unit_rows(N, self.c)
        self.maps = torch.randn((1, n, hw, self.c), device="cuda").to(torch.bfloat16)
        self.ws = torch.empty(lib.fav_patch_workspace_bytes(n * hw, self.c, N, 0), dtype=torch.uint8, device="cuda")
        self.dist = torch.empty((n, hw), dtype=torch.float32, device="cuda")
        self.row = torch.empty((n, hw), dtype=torch.int32, device="cuda")
        self.rec = torch.empty((n, 8), dtype=torch.int32, device="cuda")
        self.q = torch.empty((n * hw, self.c), dtype=torch.bfloat16, device="cuda")
        self.flags = torch.empty((n * hw,), dtype=torch.int32, device="cuda")

    def score(self, radius=None):
        s = torch.cuda.current_stream().cuda_stream
        head = (self.maps.data_ptr(), 1, self.n, self.hf, self.wf, self.c, self.bank.data_ptr(), self.N, 0, float("inf"))
        tail = (self.ws.data_ptr(), self.ws.numel(), self.dist.data_ptr(), self.row.data_ptr(), self.rec.data_ptr(), s)
        st = self.lib.fav_op_patch_score(*head, *tail) if radius is None else self.lib.fav_op_patch_score_at(*head, radius, *tail)
        assert st == 0, self.lib.fav_last_error(None)

    def query(self, radius):
        st = self.lib.fav_op_patch_query(self.maps.data_ptr(), 1, self.n, self.hf, self.wf, self.c, radius, self.q.data_ptr(),
                                         self.flags.data_ptr(), torch.cuda.current_stream().cuda_stream)
        assert st == 0, self.lib.fav_last_error(None)


def child(stage, n, N, radius, reps):
    head = Head(_lib.load(), stage, n, N)
    for _ in range(reps + 1):
        head.score(radius)
    torch.cuda.synchronize()


def kernel_times(stage, n, N, radius, reps):
    """-> {launch: microseconds a call, summed over its launches} from a child process under rocprofv3."""
    with tempfile.TemporaryDirectory() as d:
        cmd = ["rocprofv3", "--kernel-trace", "--stats", "--output-format", "csv", "-d", d, "--", sys.executable, os.path.abspath(__file__),
               "--child", str(stage), "--n", str(n), "--rows", str(N), "--radius", str(radius), "--reps", str(reps)]
        r = subprocess.run(cmd, stdout=subprocess.PIPE, stderr=subprocess.STDOUT, text=True, timeout=300)
        files = glob.glob(os.path.join(d, "**", "*kernel_stats.csv"), recursive=True)
        if r.returncode != 0 or not files:
            raise SystemExit(f"the kernel trace of stage {stage} failed (exit status {r.returncode}):\n{r.stdout[-2000:]}")
        print(f"traced stage {stage}", file=sys.stderr, flush=True)
        rows = list(csv.DictReader(open(files[0])))
    out = {}
    for key, name in KERNELS:
        hit = [r for r in rows if name in r.get("Name", "")]
        out[key] = sum(float(r["TotalDurationNs"]) for r in hit) / (reps + 1) / 1e3 if hit else None
    return out


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--rows", type=int, default=16384)
    ap.add_argument("--radius", type=int, default=1)
    ap.add_argument("--n", type=int, default=256)
    ap.add_argument("--reps", type=int, default=3)
    ap.add_argument("--rounds", type=int, default=5)
    ap.add_argument("--warmup", type=int, default=2)
    ap.add_argument("--no-kernels", action="store_true", help="skip the per-launch kernel traces")
    ap.add_argument("--child", default=None, help=argparse.SUPPRESS)
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "patch_local_bench.txt"))
    args = ap.parse_args()
    traces = {}
    if not args.child and not args.no_kernels:       # before this process touches the device
        for stage in STAGES:
            traces[stage] = kernel_times(stage, args.n, args.rows, args.radius, args.reps)
    if not torch.cuda.is_available():
        raise SystemExit("patch_local_bench needs a gfx950 GPU; a CPU run measures nothing")
    if args.child:
        return child(int(args.child), args.n, args.rows, args.radius, args.reps)

    def rounds_of(calls, reps=args.reps):
        for launch in calls.values():
            for _ in range(args.warmup):
                launch()
        torch.cuda.synchronize()
        ms = {k: [] for k in calls}
        for _ in range(args.rounds):
            for k, launch in calls.items():
                e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
                e0.record()
                for _ in range(reps):
                    launch()
                e1.record()
                e1.synchronize()
                ms[k].append(e0.elapsed_time(e1) / reps)
        return {k: (statistics.median(v), min(v), max(v)) for k, v in ms.items()}

    def f3(t, scale=1.0, digits=3):
        return f"{t[0] * scale:.{digits}f} [{t[1] * scale:.{digits}f}, {t[2] * scale:.{digits}f}]"

    lib = _lib.load()
    name = torch.cuda.get_device_name(0)
    lines = [f"Mid-level patch maps, ResNet-50 single pass, {args.n} frames of 224 x 224 a call, N = {args.rows} random unit rows, {name}",
             f"median [min, max] of {args.rounds} rounds of {args.reps} back-to-back calls (HIP events), {args.warmup} warm-up calls; the "
             "calls of a table row alternate inside a round", "",
             f"1. classify against classify_patch at a site of radius {args.radius}; 'classify (tap on)' is the plain call on the handle "
             "that holds the bank, its stage tap on; query / gemm / fold / score: kernel time in microseconds of one call, summed over "
             f"its launches, rocprofv3 --kernel-trace --stats of a child process that runs fav_op_patch_score_at alone ({args.reps} + 1 calls)",
             f"{'stage':>6}{'map':>16}{'cells':>8}{'chunk':>7}{'chunks':>7}{'classify (tap on) ms':>30}{'classify_patch ms':>30}{'difference ms':>15}"
             f"{'ratio':>9}{'query us':>10}{'gemm us':>11}{'fold us':>10}{'score us':>10}"]
    g = torch.Generator("cuda").manual_seed(3)
    frames = torch.randint(0, 256, (args.n, 224, 224, 3), dtype=torch.uint8, device="cuda", generator=g)
    be = Backend(arch="resnet50", max_batch=args.n)
    base = rounds_of({"classify": lambda: be.classify(frames)})["classify"]
    lines.append(f"{'-':>6}{'-':>16}{'-':>8}{'-':>7}{'-':>7}{f3(base) + ' (off)':>30}")
    for stage, (hf, wf, c) in STAGES.items():
        cells = args.n * hf * wf
        bits = unit_rows(args.rows, c).cpu().numpy().view(np.uint16)
        be.set_stage_tap(stage)
        be.set_patch_bank(PatchBank(bits, threshold=1.0, stage=stage, radius=args.radius))
        chunk = lib.fav_patch_chunk_rows(cells, args.rows, 0)
        r = rounds_of({"classify": lambda: be.classify(frames), "patch": lambda: be.classify_patch(frames)})
        cl, pa = r["classify"], r["patch"]
        t = traces.get(stage, {})
        us = "".join(f"{'-' if t.get(key) is None else format(t[key], '.1f'):>{11 if key == 'gemm' else 10}}" for key, _ in KERNELS)
        lines.append(f"{stage:>6}{f'{hf} x {wf} x {c}':>16}{cells:>8}{chunk:>7}{-(-((args.rows + 63) // 64 * 64) // chunk):>7}{f3(cl):>30}{f3(pa):>30}"
                     f"{pa[0] - cl[0]:>15.3f}{pa[0] / cl[0]:>9.4f}{us}")
        be.set_patch_bank(None)
    be.set_stage_tap(0)
    be.close()

    lines += ["", "2. fav_op_patch_query against the bytes it must move: the map once in and q out; 'copy': a device-to-device copy of the "
              "stage's map (the same bytes read and written); GB/s counts read plus written bytes; 'of copy': the kernel's GB/s over the copy's median",
              f"{'stage':>6}{'MB in + out':>13}{'copy us':>28}{'copy GB/s':>11}" + "".join(f"{f'r={r} us':>28}{'GB/s':>7}{'of copy':>9}" for r in (0, 1, 2))]
    heads = {}
    for stage in STAGES:
        heads[stage] = h = Head(lib, stage, args.n, 64)
        nbytes = 2 * h.maps.numel() * 2
        dst = torch.empty_like(h.maps)
        r = rounds_of({"copy": lambda: dst.copy_(h.maps), **{f"r{k}": (lambda k=k: h.query(k)) for k in (0, 1, 2)}}, reps=10)
        copy_gbs = nbytes / (r["copy"][0] * 1e-3) / 1e9
        row = f"{stage:>6}{nbytes / 1e6:>13.1f}{f3(r['copy'], 1e3, 1):>28}{copy_gbs:>11.0f}"
        for k in (0, 1, 2):
            gbs = nbytes / (r[f"r{k}"][0] * 1e-3) / 1e9
            row += f"{f3(r[f'r{k}'], 1e3, 1):>28}{gbs:>7.0f}{gbs / copy_gbs:>9.2f}"
        lines.append(row)
        del dst

    h = heads[2]
    r = rounds_of({"old": lambda: h.score(None), "new": lambda: h.score(0), "query": lambda: h.query(0)}, reps=10)
    lines += ["", "3. radius 0 against the k-NN head's query kernel, stage-2 maps (200704 cells x 512), a bank of 64 rows: everything behind the "
              "query is the same small GEMM, fold and score launch in both heads",
              f"{'fav_op_patch_score (knn_query_kernel) us':>46}{'fav_op_patch_score_at radius 0 us':>40}{'difference us':>15}{'fav_op_patch_query radius 0 alone us':>40}",
              f"{f3(r['old'], 1e3, 1):>46}{f3(r['new'], 1e3, 1):>40}{(r['new'][0] - r['old'][0]) * 1e3:>15.1f}{f3(r['query'], 1e3, 1):>40}"]
    text = "\n".join(lines) + "\n"
    os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
    with open(args.out, "w") as f:
        f.write(text)
    print(text)


if __name__ == "__main__":
    main()
