"""Time fav_op_views: hflip alone, d4() and shifts(2) on 256 x 224 x 224 uint8 frames and on 64 x 224 x 224 fp32 frames, each
against a device-to-device hipMemcpyAsync of the same OUTPUT bytes in the same rounds (the yardstick: what moving that many
bytes costs when nothing is rearranged), and one end-to-end pair on vit_b16: 64 frames x 4 views in one call against a
views-off call of 256 frames (the same 256 forward passes).

One process; every figure is the median [min, max] over --rounds rounds, in which the variants alternate, of (HIP-event time
of --reps back-to-back launches into one preallocated output) / reps, after --warmup launches.  GB/s counts the input once
and the output once.  There is no pass / fail threshold; the output file is the record.

    python tools/views_bench.py [--out profiles/views_bench.txt]"""
import argparse
import os
import statistics
import sys

import torch

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
from failure_aware_vision_amd import Backend, _lib, views  # noqa: E402


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--hw", type=int, default=224)
    ap.add_argument("--n-u8", type=int, default=256)
    ap.add_argument("--n-f32", type=int, default=64)
    ap.add_argument("--reps", type=int, default=10)
    ap.add_argument("--rounds", type=int, default=7)
    ap.add_argument("--warmup", type=int, default=3)
    ap.add_argument("--no-e2e", action="store_true", help="skip the vit_b16 pair")
    ap.add_argument("--out", default=os.path.join(os.path.dirname(os.path.dirname(os.path.abspath(__file__))), "profiles",
                                                  "views_bench.txt"))
    args = ap.parse_args()
    if not torch.cuda.is_available():
        raise SystemExit("views_bench needs a gfx950 GPU; a CPU run measures nothing")
    lib = _lib.load()
    H = W = args.hw
    stream = torch.cuda.current_stream().cuda_stream

    def rounds_of(calls, reps=args.reps, warmup=args.warmup):
        """calls: {name: launch} or {name: (prepare, launch)}; prepare runs before a variant's warm-up and before each of its
        rounds, outside the events.  The variants alternate inside every round -> {name: (median, min, max) ms per launch}"""
        calls = {k: c if isinstance(c, tuple) else (None, c) for k, c in calls.items()}
        for prepare, launch in calls.values():
            if prepare:
                prepare()
            for _ in range(warmup):
                launch()
        torch.cuda.synchronize()
        ms = {k: [] for k in calls}
        for _ in range(args.rounds):
            for k, (prepare, launch) in calls.items():
                if prepare:
                    prepare()
                e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
                e0.record()
                for _ in range(reps):
                    launch()
                e1.record()
                e1.synchronize()
                ms[k].append(e0.elapsed_time(e1) / reps)
        return {k: (statistics.median(v), min(v), max(v)) for k, v in ms.items()}

    lines = [f"fav_op_views, {H} x {W} x 3 frames, {torch.cuda.get_device_name(0)}",
             f"median [min, max] of {args.rounds} rounds of {args.reps} back-to-back launches (HIP events), {args.warmup} warm-up "
             "launches; views and the copy alternate inside a round; the copy is a device-to-device hipMemcpyAsync of the output's bytes;",
             "GB/s = (input + output bytes) / median", "",
             f"{'frames':<14}{'views':<12}{'A':>3}{'out MB':>9}{'views ms':>28}{'GB/s':>8}{'copy ms':>28}{'views / copy':>14}"]
    presets = (("hflip", views.hflip()), ("d4", views.d4()), ("shifts(2)", views.shifts(2)))
    for label, n, dtype in (("u8", args.n_u8, torch.uint8), ("f32", args.n_f32, torch.float32)):
        g = torch.Generator("cuda").manual_seed(3)
        frames = torch.randint(0, 256, (n, H, W, 3), dtype=torch.uint8, device="cuda", generator=g)
        if dtype == torch.float32:
            frames = frames.to(torch.float32) / 255
        layout = _lib.LAYOUT_NHWC_U8 if dtype == torch.uint8 else _lib.LAYOUT_NHWC_F32
        for name, vs in presets:
            arr, A = views.to_c_array(vs)
            out = torch.empty((A,) + tuple(frames.shape), dtype=dtype, device="cuda")
            src = torch.empty_like(out)
            nbytes = out.numel() * out.element_size()

            def op():
                _lib.check(lib.fav_op_views(frames.data_ptr(), out.data_ptr(), n, H, W, layout, arr, A, stream))

            def copy():
                out.copy_(src, non_blocking=True)           # same device, same dtype, contiguous: one hipMemcpyAsync

            r = rounds_of({"views": op, "copy": copy})
            v, c = r["views"], r["copy"]
            gbs = (frames.numel() * frames.element_size() + nbytes) / 1e9 / (v[0] * 1e-3)
            lines.append(f"{f'{n} {label}':<14}{name:<12}{A:>3}{nbytes / 1e6:>9.1f}{f'{v[0]:.4f} [{v[1]:.4f}, {v[2]:.4f}]':>28}{gbs:>8.0f}"
                         f"{f'{c[0]:.4f} [{c[1]:.4f}, {c[2]:.4f}]':>28}{v[0] / c[0]:>14.2f}")
            del out, src
    if not args.no_e2e:
        be = Backend("vit_b16", max_batch=256)
        g = torch.Generator("cuda").manual_seed(5)
        frames = torch.randint(0, 256, (256, H, W, 3), dtype=torch.uint8, device="cuda", generator=g)
        four = views.product(views.hflip(), [views.View(), views.View(flip_y=True)])

        e2e_reps = max(1, args.reps // 5)
        r = rounds_of({"plain": (lambda: be.set_views(None), lambda: be.classify(frames)),
                       "views": (lambda: be.set_views(four), lambda: be.classify(frames[:64]))}, reps=e2e_reps, warmup=2)
        p, v = r["plain"], r["views"]
        lines += ["", f"vit_b16 end to end, ms per call (256 forward passes each), {args.rounds} rounds of {e2e_reps} calls, 2 warm-up "
                      "calls; the views are set before a round, outside the events",
                  f"  256 frames, views off      {p[0]:.3f} [{p[1]:.3f}, {p[2]:.3f}]",
                  f"  64 frames x 4 views        {v[0]:.3f} [{v[1]:.3f}, {v[2]:.3f}]",
                  f"  views / plain              {v[0] / p[0]:.4f}"]
        be.close()
    text = "\n".join(lines) + "\n"
    os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
    with open(args.out, "w") as f:
        f.write(text)
    print(text)


if __name__ == "__main__":
    main()
