"""Time Backend.classify_ood against Backend.classify on the same handle: the headline config (ResNet-50, MC-Dropout T = 30,
224 x 224, 256 frames a call) and ViT-B/16 (256 frames a call), each with an OOD model of k = 64, 256 and the full feature
width, R = 1000 class rows.  The model is random (finite values of a fitted model's size): the head's time does not depend
on the values.  What the difference pays for: the device-to-device copies of the tapped rows and the one scoring launch.

One process; every figure is the median [min, max] over --rounds rounds, in which the two calls alternate, of (HIP-event
time of --reps back-to-back calls) / reps, after --warmup calls.  There is no pass / fail threshold; the output file is the
record.

    python tools/ood_bench.py [--out profiles/ood_bench.txt] [--configs mc30,vit]"""
import argparse
import os
import statistics
import sys

import numpy as np
import torch

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
from failure_aware_vision_amd import Backend  # noqa: E402
from failure_aware_vision_amd.ood import OODModel  # noqa: E402

CONFIGS = {
    "mc30": ("ResNet-50, MC-Dropout T=30", dict(arch="resnet50", n_samples=30, dropout_policy="all_blocks", dropout_p=0.1, seed=4), 2048),
    "vit": ("ViT-B/16", dict(arch="vit_b16"), 768),
}


def random_model(D, k, R, seed=0):
    rng = np.random.default_rng(seed)
    return OODModel(0.1 * rng.standard_normal(D), rng.standard_normal((k, D)) / np.sqrt(D), rng.standard_normal((R, k)),
                    np.arange(R) % 1000, threshold=float(k))


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--configs", default="mc30,vit")
    ap.add_argument("--n", type=int, default=256)
    ap.add_argument("--rows", type=int, default=1000)
    ap.add_argument("--reps", type=int, default=3)
    ap.add_argument("--rounds", type=int, default=5)
    ap.add_argument("--warmup", type=int, default=2)
    ap.add_argument("--out", default=os.path.join(os.path.dirname(os.path.dirname(os.path.abspath(__file__))), "profiles",
                                                  "ood_bench.txt"))
    args = ap.parse_args()
    if not torch.cuda.is_available():
        raise SystemExit("ood_bench needs a gfx950 GPU; a CPU run measures nothing")

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

    lines = [f"classify_ood against classify, {args.n} frames of 224 x 224 a call, {torch.cuda.get_device_name(0)}",
             f"median [min, max] ms per call of {args.rounds} rounds of {args.reps} back-to-back calls (HIP events), {args.warmup} "
             f"warm-up calls; the two calls alternate inside a round; R = {args.rows} class rows; 'classify (tap on)' is the plain "
             "call on the handle that holds the model",
             "", f"{'config':<30}{'D':>6}{'k':>6}{'classify (tap on) ms':>32}{'classify_ood ms':>32}{'difference ms':>15}{'ratio':>9}"]
    g = torch.Generator("cuda").manual_seed(3)
    frames = torch.randint(0, 256, (args.n, 224, 224, 3), dtype=torch.uint8, device="cuda", generator=g)
    for key in args.configs.split(","):
        name, kw, D = CONFIGS[key]
        be = Backend(max_batch=args.n, **kw)
        base = rounds_of({"classify": lambda: be.classify(frames)})["classify"]
        lines.append(f"{name:<30}{D:>6}{'-':>6}{f'{base[0]:.3f} [{base[1]:.3f}, {base[2]:.3f}] (off)':>32}")
        for k in (64, 256, D):
            be.set_ood(random_model(D, k, args.rows))
            r = rounds_of({"classify": lambda: be.classify(frames), "ood": lambda: be.classify_ood(frames)})
            c, o = r["classify"], r["ood"]
            lines.append(f"{name:<30}{D:>6}{k:>6}{f'{c[0]:.3f} [{c[1]:.3f}, {c[2]:.3f}]':>32}{f'{o[0]:.3f} [{o[1]:.3f}, {o[2]:.3f}]':>32}"
                         f"{o[0] - c[0]:>15.3f}{o[0] / c[0]:>9.4f}")
        be.close()
    text = "\n".join(lines) + "\n"
    os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
    with open(args.out, "w") as f:
        f.write(text)
    print(text)


if __name__ == "__main__":
    main()
