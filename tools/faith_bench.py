"""Time the deletion / insertion curve path: fav_op_occlude at 256 x 224 x 224 uint8 and fp32 frames, S = 16 (all 17 steps in
one launch), against fav_op_views with 17 straight views of the same frames - views_straight_kernel, the nearest streaming
kernel: the same frames in, the same number of output bytes - and against a device-to-device copy of the output's bytes, all
alternating in the same rounds; then one fav_classify_curve call on resnet50 against the same number of plain fav_classify_ex
calls, which gives the share of a curve call spent outside the forward passes (rank, occlusion, class-probability head, curve).

One process; every figure is the median [min, max] over --rounds rounds of (HIP-event time of --reps back-to-back launches
into one preallocated output) / reps, after --warmup launches.  GB/s counts the input once and the output once: (S + 1) writes
of every frame plus one read.  There is no pass / fail threshold; the output file is the record.

    python tools/faith_bench.py [--out profiles/faith_bench.txt]"""
import argparse
import ctypes as C
import os
import statistics
import sys

import numpy as np
import torch

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
from failure_aware_vision_amd import Backend, _lib, faithfulness, views  # noqa: E402


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--hw", type=int, default=224)
    ap.add_argument("--n", type=int, default=256)
    ap.add_argument("--steps", type=int, default=16)
    ap.add_argument("--map", type=int, default=14, help="the map is map x map cells")
    ap.add_argument("--reps", type=int, default=5)
    ap.add_argument("--rounds", type=int, default=7)
    ap.add_argument("--warmup", type=int, default=2)
    ap.add_argument("--e2e-n", type=int, default=64)
    ap.add_argument("--no-e2e", action="store_true", help="skip the resnet50 pair")
    ap.add_argument("--out", default=os.path.join(os.path.dirname(os.path.dirname(os.path.abspath(__file__))), "profiles",
                                                  "faith_bench.txt"))
    args = ap.parse_args()
    if not torch.cuda.is_available():
        raise SystemExit("faith_bench needs a gfx950 GPU; a CPU run measures nothing")
    lib = _lib.load()
    H = W = args.hw
    n, S, M = args.n, args.steps, args.map
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

    lines = [f"fav_op_occlude, {n} frames of {H} x {W} x 3, {M} x {M} cells, S = {S}: {S + 1} steps in one launch, "
             f"{torch.cuda.get_device_name(0)}",
             f"median [min, max] of {args.rounds} rounds of {args.reps} back-to-back launches (HIP events), {args.warmup} warm-up launches; "
             "the variants alternate inside a round;",
             f"views: fav_op_views with {S + 1} straight views (views_straight_kernel) of the same frames, the same output bytes; copy: "
             "a device-to-device hipMemcpyAsync of the output's bytes;",
             "GB/s = (input + output bytes) / median", "",
             f"{'frames':<10}{'mode':<11}{'out MB':>9}{'occlude ms':>28}{'GB/s':>7}{'views ms':>28}{'GB/s':>7}{'copy ms':>28}{'occl / views':>14}"]
    shifts = [views.View(dy=a % 3 - 1, dx=a // 3 % 3 - 1, border="replicate") for a in range(S + 1)]
    arr, A = views.to_c_array(shifts)
    rank = torch.from_numpy(np.stack([np.random.default_rng(i).permutation(M * M) for i in range(n)]).astype(np.int32)).cuda()
    for label, dtype in (("u8", torch.uint8), ("f32", torch.float32)):
        g = torch.Generator("cuda").manual_seed(3)
        frames = torch.randint(0, 256, (n, H, W, 3), dtype=torch.uint8, device="cuda", generator=g)
        if dtype == torch.float32:
            frames = frames.to(torch.float32) / 255
        layout = _lib.LAYOUT_NHWC_U8 if dtype == torch.uint8 else _lib.LAYOUT_NHWC_F32
        fill = (C.c_uint32 * 3)(128, 128, 128) if dtype == torch.uint8 else (C.c_uint32 * 3)(*[0x3F000000] * 3)
        out = torch.empty((S + 1,) + tuple(frames.shape), dtype=dtype, device="cuda")
        src = torch.empty_like(out)
        nbytes = out.numel() * out.element_size()
        total = frames.numel() * frames.element_size() + nbytes

        def copy():
            out.copy_(src, non_blocking=True)

        def view():
            _lib.check(lib.fav_op_views(frames.data_ptr(), out.data_ptr(), n, H, W, layout, arr, A, stream))

        for mode_name, mode in (("deletion", _lib.CURVE_DELETION), ("insertion", _lib.CURVE_INSERTION)):
            def occlude():
                _lib.check(lib.fav_op_occlude(frames.data_ptr(), out.data_ptr(), n, H, W, layout, rank.data_ptr(), M, M, mode, S, 0, S + 1,
                                              fill, stream))

            r = rounds_of({"occlude": occlude, "views": view, "copy": copy})
            o, v, c = r["occlude"], r["views"], r["copy"]
            lines.append(f"{f'{n} {label}':<10}{mode_name:<11}{nbytes / 1e6:>9.1f}{cell(o):>28}{total / 1e9 / (o[0] * 1e-3):>7.0f}"
                         f"{cell(v):>28}{total / 1e9 / (v[0] * 1e-3):>7.0f}{cell(c):>28}{o[0] / v[0]:>14.2f}")
        del out, src
    if not args.no_e2e:
        m = args.e2e_n
        be = Backend("resnet50", max_batch=m)
        be.set_curve(S)
        g = torch.Generator("cuda").manual_seed(5)
        frames = torch.randint(0, 256, (m, H, W, 3), dtype=torch.uint8, device="cuda", generator=g)
        maps = torch.from_numpy(faithfulness.random_maps(m, (7, 7), 0)).cuda()

        def plain():
            for _ in range(S + 1):
                be.classify(frames)

        r = rounds_of({"curve": lambda: be.classify_curve(frames, maps), "plain": plain}, reps=1, warmup=1)
        c, p = r["curve"], r["plain"]
        lines += ["", f"resnet50 end to end, {m} frames, 7 x 7 cells, S = {S}: ms per call, {args.rounds} rounds of 1 call, 1 warm-up call",
                  f"  fav_classify_curve ({S + 1} passes)      {cell(c)}",
                  f"  {S + 1} x fav_classify_ex               {cell(p)}",
                  f"  share outside the forward passes  {1.0 - p[0] / c[0]:.4f}"]
        be.close()
    text = "\n".join(lines) + "\n"
    os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
    with open(args.out, "w") as f:
        f.write(text)
    print(text)


if __name__ == "__main__":
    main()
