"""Time the RISE path: fav_op_rise_mask at 256 x 224 x 224 uint8 frames for m1 - m0 in {1, 8}, beside fav_op_occlude at the same
shape and the same number of output frames (steps), alternating in the same rounds; then one fav_classify_rise call of 64 masks
on resnet50 against 65 plain fav_classify_ex calls on the same frames, which gives the share of a RISE call spent outside the
forward passes (the masks, the class-probability head, the accumulate head).

One process; every figure is the median [min, max] over --rounds rounds of (HIP-event time of --reps back-to-back launches
into one preallocated output) / reps, after --warmup launches.  GB/s counts the algorithmic bytes: the input once and the
output once.  There is no pass / fail threshold; the output file is the record.

    python tools/rise_bench.py [--out profiles/rise_bench.txt]"""
import argparse
import ctypes as C
import os
import statistics
import sys

import numpy as np
import torch

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
from failure_aware_vision_amd import Backend, _lib  # noqa: E402


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--hw", type=int, default=224)
    ap.add_argument("--n", type=int, default=256)
    ap.add_argument("--grid", type=int, default=7)
    ap.add_argument("--map", type=int, default=14, help="the occlusion yardstick's map is map x map cells")
    ap.add_argument("--reps", type=int, default=5)
    ap.add_argument("--rounds", type=int, default=7)
    ap.add_argument("--warmup", type=int, default=2)
    ap.add_argument("--e2e-n", type=int, default=64)
    ap.add_argument("--e2e-masks", type=int, default=64)
    ap.add_argument("--no-e2e", action="store_true", help="skip the resnet50 pair")
    ap.add_argument("--out", default=os.path.join(os.path.dirname(os.path.dirname(os.path.abspath(__file__))), "profiles",
                                                  "rise_bench.txt"))
    args = ap.parse_args()
    if not torch.cuda.is_available():
        raise SystemExit("rise_bench needs a gfx950 GPU; a CPU run measures nothing")
    lib = _lib.load()
    H = W = args.hw
    n, M = args.n, args.map
    stream = torch.cuda.current_stream().cuda_stream

    def rounds_of(calls, reps=args.reps, warmup=args.warmup):
        """calls: {name: launch}; the variants alternate inside every round -> {name: (median, min, max) ms per launch}"""
        for launch in calls.values():
            for _ in range(warmup):
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

    def cell(v):
        return f"{v[0]:.4f} [{v[1]:.4f}, {v[2]:.4f}]"

    lines = [f"fav_op_rise_mask, {n} uint8 frames of {H} x {W} x 3, grid {args.grid}, keep 128, {torch.cuda.get_device_name(0)}",
             f"median [min, max] of {args.rounds} rounds of {args.reps} back-to-back launches (HIP events), {args.warmup} warm-up launches; "
             "the variants alternate inside a round;",
             f"occlude: fav_op_occlude (deletion, {M} x {M} cells, S = 16) writing the same number of output frames from the same input;",
             "GB/s = (input + output bytes) / median", "",
             f"{'masks':<8}{'out MB':>9}{'rise_mask ms':>28}{'GB/s':>7}{'occlude ms':>28}{'GB/s':>7}{'mask / occl':>13}"]
    g = torch.Generator("cuda").manual_seed(3)
    frames = torch.randint(0, 256, (n, H, W, 3), dtype=torch.uint8, device="cuda", generator=g)
    rank = torch.from_numpy(np.stack([np.random.default_rng(i).permutation(M * M) for i in range(n)]).astype(np.int32)).cuda()
    fill = (C.c_uint32 * 3)(128, 128, 128)
    d = _lib.FavRise()
    d.struct_size = C.sizeof(_lib.FavRise)
    d.n_masks, d.grid, d.keep, d.seed = 64, args.grid, 128, 7
    for c in range(3):
        d.fill_u8[c], d.fill_f32_bits[c] = 128, 0x3F000000
    for k in (1, 8):
        out = torch.empty((k,) + tuple(frames.shape), dtype=torch.uint8, device="cuda")
        nbytes = out.numel()
        total = frames.numel() + nbytes

        def mask():
            _lib.check(lib.fav_op_rise_mask(frames.data_ptr(), out.data_ptr(), n, H, W, _lib.LAYOUT_NHWC_U8, C.byref(d), 0, 8, 8 + k, stream))

        def occlude():
            _lib.check(lib.fav_op_occlude(frames.data_ptr(), out.data_ptr(), n, H, W, _lib.LAYOUT_NHWC_U8, rank.data_ptr(), M, M,
                                          _lib.CURVE_DELETION, 16, 4, 4 + k, fill, stream))

        r = rounds_of({"mask": mask, "occlude": occlude})
        a, o = r["mask"], r["occlude"]
        lines.append(f"{k:<8}{nbytes / 1e6:>9.1f}{cell(a):>28}{total / 1e9 / (a[0] * 1e-3):>7.0f}{cell(o):>28}"
                     f"{total / 1e9 / (o[0] * 1e-3):>7.0f}{a[0] / o[0]:>13.2f}")
        del out
    if not args.no_e2e:
        m, N = args.e2e_n, args.e2e_masks
        be = Backend("resnet50", max_batch=m)
        be.set_rise(N, grid=args.grid)
        g = torch.Generator("cuda").manual_seed(5)
        fr = torch.randint(0, 256, (m, H, W, 3), dtype=torch.uint8, device="cuda", generator=g)

        def plain():
            for _ in range(N + 1):
                be.classify(fr)

        r = rounds_of({"rise": lambda: be.classify_rise(fr), "plain": plain}, reps=1, warmup=1)
        c, p = r["rise"], r["plain"]
        lines += ["", f"resnet50 end to end, {m} frames, 14 x 14 cells, {N} masks: ms per call, {args.rounds} rounds of 1 call, 1 warm-up call",
                  f"  fav_classify_rise ({N + 1} passes)       {cell(c)}",
                  f"  {N + 1} x fav_classify_ex               {cell(p)}",
                  f"  share outside the forward passes  {1.0 - p[0] / c[0]:.4f}"]
        be.close()
    text = "\n".join(lines) + "\n"
    os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
    with open(args.out, "w") as f:
        f.write(text)
    print(text)


if __name__ == "__main__":
    main()
