"""Time fav_op_corrupt_c: every kind at 256 x 224 x 224, severities 3 and 5, beside the Gaussian mode of fav_op_corrupt in
the same process (the yardstick: it moves the same 3 bytes in and 12 bytes out per pixel).

Each figure is the median over --rounds rounds of (HIP-event time of --reps back-to-back launches into one preallocated
output) / reps, after --warmup launches; GB/s counts 15 bytes per pixel.  A call moves 193 MB, less than the 256 MiB
Infinity Cache, so part of every launch's input may be served from it - for the yardstick as well.  There is no pass / fail
threshold; the output file is the record.

    python tools/corrupt_c_bench.py [--out profiles/corrupt_c_bench.txt]

--ab adds the A/B behind the store scheme of the four-pixel kernels (pointwise kinds and contrast): with a library built by
`make EXPERIMENTS=1 OUT=...` and named in FAV_LIB_PATH, the variable FAV_CORRUPT_C_STORE (read at every call) selects staged
stores through LDS (0, what ships), three float4 straight from registers (1) or twelve scalar stores (2); the three and the
Gaussian mode alternate inside every round of one process, and the outputs of the three are compared bit for bit."""
import argparse
import ctypes as C
import os
import statistics
import sys

import torch

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
from failure_aware_vision_amd import SEVERITY, _lib  # noqa: E402
from failure_aware_vision_amd.corrupt import Corruptor  # noqa: E402


MODES = ("0 staged through LDS", "1 float4 from registers", "2 scalar stores")


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--n", type=int, default=256)
    ap.add_argument("--hw", type=int, default=224)
    ap.add_argument("--reps", type=int, default=20)
    ap.add_argument("--rounds", type=int, default=7)
    ap.add_argument("--warmup", type=int, default=5)
    ap.add_argument("--ab", action="store_true", help="A/B the store schemes (needs an EXPERIMENTS build in FAV_LIB_PATH)")
    ap.add_argument("--out", default=os.path.join(os.path.dirname(os.path.dirname(os.path.abspath(__file__))), "profiles",
                                                  "corrupt_c_bench.txt"))
    args = ap.parse_args()
    if not torch.cuda.is_available():
        raise SystemExit("corrupt_c_bench needs a gfx950 GPU; a CPU run measures nothing")
    n, H, W = args.n, args.hw, args.hw
    cor = Corruptor(seed=1)
    lib = cor.lib
    frames = torch.randint(0, 256, (n, H, W, 3), dtype=torch.uint8, device="cuda", generator=torch.Generator("cuda").manual_seed(3))
    out = torch.empty((n, H, W, 3), dtype=torch.float32, device="cuda")
    stream = torch.cuda.current_stream().cuda_stream
    gbytes = 15.0 * n * H * W / 1e9

    def timed(launch):
        for _ in range(args.warmup):
            launch()
        torch.cuda.synchronize()
        ms = []
        for _ in range(args.rounds):
            e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
            e0.record()
            for _ in range(args.reps):
                launch()
            e1.record()
            e1.synchronize()
            ms.append(e0.elapsed_time(e1) / args.reps)
        return statistics.median(ms), min(ms), max(ms)

    def gaussian_mode():
        _lib.check(lib.fav_op_corrupt(frames.data_ptr(), out.data_ptr(), n, H, W, 3, 0.0, 1.0, 0.18, 1, 0, stream))

    def kind_call(k, a, b):
        d = _lib.FavCorruptionDesc(32, k, a, b, 1, 0)
        return lambda: _lib.check(lib.fav_op_corrupt_c(frames.data_ptr(), out.data_ptr(), n, H, W, C.byref(d), stream))

    base = timed(gaussian_mode)
    rows = []
    for k, kind in enumerate(_lib.CORRUPTION_KINDS):
        for sev in (3, 5):
            a, b = SEVERITY[kind][sev - 1]
            rows.append((kind, sev, a, b) + timed(kind_call(k, a, b)))
    base2 = timed(gaussian_mode)
    yard = (base[0] + base2[0]) / 2
    lines = [f"fav_op_corrupt_c, {n} x {H} x {W} x 3 uint8 -> fp32, {torch.cuda.get_device_name(0)}",
             f"median of {args.rounds} rounds of {args.reps} back-to-back launches (HIP events), {args.warmup} warm-up launches; "
             f"GB/s on 15 B per pixel ({gbytes:.4f} GB a call)", "",
             f"{'kind':<16}{'sev':>4}{'a':>8}{'b':>6}{'ms':>10}{'min':>10}{'max':>10}{'GB/s':>10}{'x gaussian mode':>18}"]
    for label, t in (("gaussian mode (before)", base), ("gaussian mode (after)", base2)):
        lines.append(f"{label:<34}{t[0]:>10.4f}{t[1]:>10.4f}{t[2]:>10.4f}{gbytes / (t[0] * 1e-3):>10.1f}{t[0] / yard:>18.2f}")
    for kind, sev, a, b, med, lo, hi in rows:
        lines.append(f"{kind:<16}{sev:>4}{a:>8.3g}{b:>6.2g}{med:>10.4f}{lo:>10.4f}{hi:>10.4f}{gbytes / (med * 1e-3):>10.1f}{med / yard:>18.2f}")
    if args.ab:
        lines += ["", f"A/B of the store scheme, library {os.path.basename(_lib.LIB_PATH)}: ms per launch, median [min, max] of {args.rounds} rounds in "
                      "which the variants alternate", f"{'kind':<16}{'sev':>4}  " + "".join(f"{m:<34}" for m in MODES) + "gaussian mode"]
        for k, kind in ((0, "impulse_noise"), (1, "speckle_noise"), (6, "brightness"), (4, "contrast")):
            a, b = SEVERITY[kind][2]
            call = kind_call(k, a, b)
            outs = []
            for mode in range(3):                      # the same bits from all three, and warm-up
                os.environ["FAV_CORRUPT_C_STORE"] = str(mode)
                for _ in range(args.warmup):
                    call()
                outs.append(out.clone())
            assert torch.equal(outs[0], outs[1]) and torch.equal(outs[0], outs[2]), kind
            ms = [[] for _ in range(4)]
            for _ in range(args.rounds):
                for mode in range(4):
                    os.environ["FAV_CORRUPT_C_STORE"] = str(mode % 3)
                    e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
                    e0.record()
                    for _ in range(args.reps):
                        gaussian_mode() if mode == 3 else call()
                    e1.record()
                    e1.synchronize()
                    ms[mode].append(e0.elapsed_time(e1) / args.reps)
            os.environ["FAV_CORRUPT_C_STORE"] = "0"
            cells = [f"{statistics.median(m):.4f} [{min(m):.4f}, {max(m):.4f}]" for m in ms]
            lines.append(f"{kind:<16}{3:>4}  " + "".join(f"{c:<34}" for c in cells[:3]) + cells[3])
    text = "\n".join(lines) + "\n"
    os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
    with open(args.out, "w") as f:
        f.write(text)
    print(text)


if __name__ == "__main__":
    main()
