"""Time fav_op_coreset_select (greedy coreset selection): microseconds a step and GB/s on the
N * D * 2 bytes a step reads, at pools of (N, D) = (12 544, 2 048), (65 536, 512) and (200 704, 2 048) - 51 MB, 67 MB and 822 MB -
with M = 256.  The pool is random unit rows: a step's time does not depend on the values.

One process; every figure is the median [min, max] over --rounds repetitions of (HIP-event time of the whole chain of M + 1
launches) / M, after one warm-up selection a shape; the host clock around the same call, which returns when the last launch is
enqueued, gives the enqueue time a launch.  The yardstick is measured in the same process: a device-to-device copy of 822 MB,
counted as the bytes it reads plus the bytes it writes.  At the smallest pool the same selection is also run by the vectorised
numpy restatement (tests/coreset_ref.py) on the host, its wall time reported and its picks compared.  There is no pass / fail
threshold; the output file is the record.

    python tools/coreset_bench.py [--out profiles/coreset_bench.txt] [--shapes 12544x2048,65536x512,200704x2048] [--m 256]"""
import argparse
import os
import statistics
import sys
import time

import numpy as np
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tests"))
from failure_aware_vision_amd import _lib  # noqa: E402


def random_pool_bits(N, D, seed=0):
    """int16 [N, D] on the device: random unit rows as bf16 bit patterns."""
    g = torch.Generator("cuda").manual_seed(seed)
    out = torch.empty((N, D), dtype=torch.bfloat16, device="cuda")
    for b in range(0, N, 65536):
        x = torch.randn((min(65536, N - b), D), device="cuda", generator=g)
        out[b:b + x.shape[0]] = (x / x.norm(dim=1, keepdim=True)).to(torch.bfloat16)
    return out.view(torch.int16)


def spread(v):
    return statistics.median(v), min(v), max(v)


def copy_gbs(nbytes, rounds):
    """GB/s of a device-to-device copy of nbytes, read plus written, median [min, max]."""
    src = torch.empty(nbytes, dtype=torch.uint8, device="cuda").random_(0, 256)
    dst = torch.empty_like(src)
    for _ in range(2):
        dst.copy_(src)
    torch.cuda.synchronize()
    out = []
    for _ in range(rounds):
        e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        e0.record()
        for _ in range(4):
            dst.copy_(src)
        e1.record()
        e1.synchronize()
        out.append(2 * nbytes * 4 / (e0.elapsed_time(e1) * 1e-3) / 1e9)
    return spread(out)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--shapes", default="12544x2048,65536x512,200704x2048")
    ap.add_argument("--m", type=int, default=256)
    ap.add_argument("--rounds", type=int, default=5)
    ap.add_argument("--no-reference", action="store_true", help="skip the numpy selection at the smallest pool")
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "coreset_bench.txt"))
    args = ap.parse_args()
    if not torch.cuda.is_available():
        raise SystemExit("coreset_bench needs a gfx950 GPU; a CPU run measures nothing")
    shapes = [tuple(int(v) for v in s.split("x")) for s in args.shapes.split(",")]
    lib = _lib.load()
    M = args.m
    stream = torch.cuda.current_stream().cuda_stream
    copy = copy_gbs(200704 * 2048 * 2, args.rounds)
    lines = [f"fav_op_coreset_select, M = {M} picks (M + 1 launches of coreset_step_kernel), {torch.cuda.get_device_name(0)}",
             f"median [min, max] of {args.rounds} repetitions of (HIP-event time of the whole chain) / M after one warm-up selection; "
             "GB/s on the N * D * 2 bytes a step reads; enqueue: (host clock around the call, which returns once the last launch "
             "is enqueued) / (M + 1)",
             f"yardstick: device-to-device copy of 822 MB, read plus written bytes: {copy[0]:.0f} [{copy[1]:.0f}, {copy[2]:.0f}] GB/s; "
             "'of copy' is the step's GB/s over that median",
             "", f"{'N':>8}{'D':>6}{'pool MB':>9}{'us a step':>28}{'GB/s':>26}{'of copy':>9}{'enqueue us a launch':>28}{'selection ms':>14}"]
    first = None
    for N, D in shapes:
        pool = random_pool_bits(N, D)
        need = lib.fav_coreset_workspace_bytes(N, D, M)
        assert need > 0, (N, D, M)
        ws = torch.empty(need, dtype=torch.uint8, device="cuda")
        order = torch.empty(M, dtype=torch.int32, device="cuda")
        radius = torch.empty(M + 1, dtype=torch.float32, device="cuda")

        def call():
            st = lib.fav_op_coreset_select(pool.data_ptr(), N, D, M, 0, ws.data_ptr(), need, order.data_ptr(), radius.data_ptr(), stream)
            assert st == 0, lib.fav_last_error(None)
        call()
        torch.cuda.synchronize()
        us, host = [], []
        for _ in range(args.rounds):
            e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
            e0.record()
            t0 = time.perf_counter()
            call()
            host.append((time.perf_counter() - t0) * 1e6 / (M + 1))
            e1.record()
            e1.synchronize()
            us.append(e0.elapsed_time(e1) * 1e3 / M)
        u, h = spread(us), spread(host)
        gbs = tuple(N * D * 2 / (v * 1e-6) / 1e9 for v in (u[0], u[2], u[1]))          # the slowest repetition is the lowest rate
        lines.append(f"{N:>8}{D:>6}{N * D * 2 / 1e6:>9.0f}{f'{u[0]:.2f} [{u[1]:.2f}, {u[2]:.2f}]':>28}"
                     f"{f'{gbs[0]:.0f} [{gbs[1]:.0f}, {gbs[2]:.0f}]':>26}{gbs[0] / copy[0]:>9.2f}{f'{h[0]:.2f} [{h[1]:.2f}, {h[2]:.2f}]':>28}"
                     f"{u[0] * M / 1e3:>14.2f}")
        if first is None:
            first = (N, D, pool.cpu().numpy().view(np.uint16), order.cpu().numpy(), radius.cpu().numpy(), u[0] * M / 1e3)
        del pool, ws
    if not args.no_reference:
        import coreset_ref
        N, D, bits, order, radius, ms = first
        t0 = time.perf_counter()
        want = coreset_ref.select(bits, M, 0)
        wall = time.perf_counter() - t0
        equal = np.array_equal(order, want[0]) and np.array_equal(radius.view(np.uint32), want[1].view(np.uint32))
        lines += ["", f"the same selection (N = {N}, D = {D}, M = {M}) by the vectorised numpy restatement on the host: {wall:.1f} s wall, "
                      f"{wall * 1e3 / ms:.0f} times the device's {ms:.2f} ms; order and radius equal bit for bit: {'yes' if equal else 'NO'}"]
    text = "\n".join(lines) + "\n"
    os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
    with open(args.out, "w") as f:
        f.write(text)
    print(text)


if __name__ == "__main__":
    main()
