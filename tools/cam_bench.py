"""Time the class activation maps on the headline config (ResNet-50, MC-Dropout T = 30, 224 x 224, 256 frames a call):
Backend.classify_detect with the map tap off, the same call with the tap on (the device-to-device copies of the maps the
average pool reads), Backend.classify_cam (those copies plus the head with K = 1), classify_cam with the heatmap, and the head
alone through Backend.cam for K = 1 and K = 5.  What the differences pay for is derived in DESIGN.md section 2, item 5i: three
passes over the 1.54 GB of maps - the copy's read, the copy's write, the head's read.

One process, two handles (tap off, tap on) of the same configuration; every figure is the median [min, max] over --rounds
rounds, in which the calls alternate, of (HIP-event time of --reps back-to-back calls) / reps, after --warmup calls.  There is
no pass / fail threshold; the output file is the record.

    python tools/cam_bench.py [--out profiles/cam_bench.txt]"""
import argparse
import os
import statistics
import sys

import torch

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
from failure_aware_vision_amd import Backend  # noqa: E402


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--n", type=int, default=256)
    ap.add_argument("--samples", type=int, default=30)
    ap.add_argument("--reps", type=int, default=3)
    ap.add_argument("--rounds", type=int, default=5)
    ap.add_argument("--warmup", type=int, default=2)
    ap.add_argument("--out", default=os.path.join(os.path.dirname(os.path.dirname(os.path.abspath(__file__))), "profiles",
                                                  "cam_bench.txt"))
    args = ap.parse_args()
    if not torch.cuda.is_available():
        raise SystemExit("cam_bench needs a gfx950 GPU; a CPU run measures nothing")

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

    kw = dict(arch="resnet50", n_samples=args.samples, dropout_policy="all_blocks", dropout_p=0.1, seed=4, max_batch=args.n)
    g = torch.Generator("cuda").manual_seed(3)
    frames = torch.randint(0, 256, (args.n, 224, 224, 3), dtype=torch.uint8, device="cuda", generator=g)
    off, on = Backend(**kw), Backend(**kw)
    info = on.map_tap_info()
    on.set_map_tap(True)
    top5 = on.classify_uncertainty(frames)["top_label"].contiguous()
    top1 = top5[:, :1].contiguous()
    r = rounds_of({
        "classify_detect, tap off": lambda: off.classify_detect(frames),
        "classify_detect, tap on": lambda: on.classify_detect(frames),
        "classify_cam": lambda: on.classify_cam(frames),
        "classify_cam, heatmap": lambda: on.classify_cam(frames, heatmap=True),
        "cam, K = 1 (the head alone)": lambda: on.cam(top1),
        "cam, K = 5 (the head alone)": lambda: on.cam(top5),
    })
    base = r["classify_detect, tap off"][0]
    prop = torch.cuda.get_device_properties(0)
    device = f"{torch.cuda.get_device_name(0)} ({prop.gcnArchName.split(':')[0]}, {prop.multi_processor_count} CUs)"
    gb = info["bytes"] * args.n / on.cfg.max_batch / 1e9
    lines = [f"class activation maps on the headline config: ResNet-50, MC-Dropout T={args.samples}, {args.n} frames of 224 x 224 a "
             f"call, {device}",
             f"the maps of a call: [{info['samples']}][{args.n}][{info['hf']} x {info['wf']}][{info['c']}] bf16 = {gb:.3f} GB",
             f"median [min, max] ms per call of {args.rounds} rounds of {args.reps} back-to-back calls (HIP events), {args.warmup} "
             "warm-up calls; the calls alternate inside a round; tap off and tap on are two handles of one configuration",
             "", f"{'call':<32}{'ms':>30}{'minus tap off ms':>18}{'GB/s of the maps':>18}"]
    for k, (med, lo, hi) in r.items():
        head = k.startswith("cam,")
        extra = "" if head or k.endswith("tap off") else f"{med - base:.3f}"
        rate = f"{gb / (med * 1e-3):.0f}" if head else ""
        lines.append(f"{k:<32}{f'{med:.3f} [{lo:.3f}, {hi:.3f}]':>30}{extra:>18}{rate:>18}")
    off.close()
    on.close()
    text = "\n".join(lines) + "\n"
    os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
    with open(args.out, "w") as f:
        f.write(text)
    print(text)


if __name__ == "__main__":
    main()
