"""Time the attention rollout on ViT-B/16 (224 x 224): Backend.classify_detect with the attention tap off, the same call with
the tap on (one attn_mean_kernel launch a layer and part, in front of the attention launch), Backend.classify_rollout (the tap
plus the head), classify_rollout with the heatmap, and the head alone through Backend.rollout - at 64 and at 512 frames a call.
What the tap pays for is set out in DESIGN.md section 2, item 5j: the score products of every head once more and about 2 MB
of fp32 attention a frame.

One process and ONE handle per batch size, whose tap is turned off and on again in every round (outside the timed windows):
with two handles of one configuration the one created first, its tap off, measured 1.5 ms SLOWER at 64 frames than the second
with its tap on - each handle forks its parts onto two streams of its own, and two handles are not two equal handles (the
supposed cause: a process has only so many hardware queues).  Every figure is the median
[min, max] over --rounds rounds of (HIP-event time of --reps back-to-back calls) / reps; an untimed call of the same kind goes
in front of every timed group, so that no group starts behind a shorter one's idle tail.  There is no pass / fail threshold;
the output file is the record.

    python tools/rollout_bench.py [--out profiles/rollout_tap_bench.txt]"""
import argparse
import os
import statistics
import sys

import torch

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
from failure_aware_vision_amd import Backend  # noqa: E402


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--n", type=int, nargs="+", default=[64, 512])
    ap.add_argument("--reps", type=int, default=20)
    ap.add_argument("--rounds", type=int, default=5)
    ap.add_argument("--warmup", type=int, default=2)
    ap.add_argument("--out", default=os.path.join(os.path.dirname(os.path.dirname(os.path.abspath(__file__))), "profiles",
                                                  "rollout_tap_bench.txt"))
    args = ap.parse_args()
    if not torch.cuda.is_available():
        raise SystemExit("rollout_bench needs a gfx950 GPU; a CPU run measures nothing")

    def rounds_of(be, calls):
        """calls: name -> (tap on?, launch)."""
        ms = {k: [] for k in calls}
        for rnd in range(-1, args.rounds):             # round -1: the warm-up, not kept
            for k, (tap, launch) in calls.items():
                be.set_attn_tap(tap)
                for _ in range(args.warmup if rnd < 0 else 0):
                    launch()
                e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
                launch()
                e0.record()
                for _ in range(args.reps):
                    launch()
                e1.record()
                e1.synchronize()
                if rnd >= 0:
                    ms[k].append(e0.elapsed_time(e1) / args.reps)
        return {k: (statistics.median(v), min(v), max(v)) for k, v in ms.items()}

    prop = torch.cuda.get_device_properties(0)
    device = f"{torch.cuda.get_device_name(0)} ({prop.gcnArchName.split(':')[0]}, {prop.multi_processor_count} CUs)"
    lines = [f"attention rollout on ViT-B/16, 224 x 224, {device}",
             f"median [min, max] ms per call of {args.rounds} rounds of {args.reps} back-to-back calls (HIP events), {args.warmup} "
             "warm-up calls in a round of their own and one untimed call in front of every timed group; the calls alternate inside a round; "
             "one handle, its tap turned off and on between the groups"]
    for n in args.n:
        kw = dict(arch="vit_b16", max_batch=n)
        g = torch.Generator("cuda").manual_seed(3)
        frames = torch.randint(0, 256, (n, 224, 224, 3), dtype=torch.uint8, device="cuda", generator=g)
        be = Backend(**kw)
        info = be.attn_tap_info()
        r = rounds_of(be, {
            "classify_detect, tap off": (False, lambda: be.classify_detect(frames)),
            "classify_detect, tap on": (True, lambda: be.classify_detect(frames)),
            "classify_rollout": (True, lambda: be.classify_rollout(frames)),
            "classify_rollout, heatmap": (True, lambda: be.classify_rollout(frames, heatmap=True)),
            "rollout (the head alone)": (True, lambda: be.rollout()),
        })
        base = r["classify_detect, tap off"][0]
        gb = info["bytes"] / 1e9
        lines += ["", f"{n} frames a call; the attention of a call: [{info['layers']}][{n}][{info['tokens']}][{info['ld']}] fp32 = {gb:.3f} GB",
                  f"{'call':<32}{'ms':>30}{'minus tap off ms':>18}{'percent':>10}{'GB/s of A':>12}"]
        for k, (med, lo, hi) in r.items():
            head = k.startswith("rollout")
            extra = "" if head or k.endswith("tap off") else f"{med - base:.3f}"
            pct = "" if head or k.endswith("tap off") else f"{100.0 * (med - base) / base:.1f}"
            rate = f"{gb / (med * 1e-3):.0f}" if head else ""
            lines.append(f"{k:<32}{f'{med:.3f} [{lo:.3f}, {hi:.3f}]':>30}{extra:>18}{pct:>10}{rate:>12}")
        be.close()
    text = "\n".join(lines) + "\n"
    os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
    with open(args.out, "w") as f:
        f.write(text)
    print(text)


if __name__ == "__main__":
    main()
