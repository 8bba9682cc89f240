"""Time the autoencoder sensor: ``Autoencoder.score`` for one 240 x 320 frame (the seam) and for
256 frames of 224 x 224, two levels, cells of 16; fav_op_ae_decode_compare alone on the same shapes, with its achieved GB/s on
its algorithmic bytes (128 bytes of hidden row a level-1 pixel inside the frame, the frame's 3 bytes a pixel, the error map and
the records; without the optional outputs); and the GEMM launch that feeds it (fav_op_conv2d 128 -> 256 on the coarse rows).

One process; every figure is the median [min, max] over --rounds repetitions of (HIP-event time of --iters back-to-back calls)
/ iters after a warm-up; the yardstick, a device-to-device copy of 822 MB counted as read plus written bytes, is measured in
the same process.  The weights are synthetic and the frames random: no time here depends on a value.  There is no pass / fail
threshold; the output file is the record.

    python tools/ae_bench.py [--out profiles/ae_bench.txt] [--rounds 5]"""
import argparse
import ctypes as C
import os
import statistics
import sys

import numpy as np
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
from failure_aware_vision_amd import Autoencoder, _lib, autoencoder as A  # noqa: E402


def spread(v):
    return statistics.median(v), min(v), max(v)


def fmt3(v, digits=1):
    return f"{v[0]:.{digits}f} [{v[1]:.{digits}f}, {v[2]:.{digits}f}]"


def timed_us(call, iters, rounds):
    """us a call: median [min, max] of `rounds` event-timed runs of `iters` calls."""
    for _ in range(3):
        call()
    torch.cuda.synchronize()
    out = []
    for _ in range(rounds):
        e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        e0.record()
        for _ in range(iters):
            call()
        e1.record()
        e1.synchronize()
        out.append(e0.elapsed_time(e1) * 1e3 / iters)
    return spread(out)


def copy_gbs(nbytes, rounds):
    src = torch.empty(nbytes, dtype=torch.uint8, device="cuda").random_(0, 256)
    dst = torch.empty_like(src)
    us = timed_us(lambda: dst.copy_(src), 4, rounds)
    return tuple(2 * nbytes / (v * 1e-6) / 1e9 for v in (us[0], us[2], us[1]))


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--rounds", type=int, default=5)
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "ae_bench.txt"))
    args = ap.parse_args()
    if not torch.cuda.is_available():
        raise SystemExit("ae_bench needs a gfx950 GPU; a CPU run measures nothing")
    lib = _lib.load()
    stream = torch.cuda.current_stream().cuda_stream
    copy = copy_gbs(200704 * 2048 * 2, args.rounds)
    levels, cell = 2, 16
    blob = A.make_synthetic_ae(levels, 1)
    _, layers = A.parse_blob(blob)
    lines = [f"the autoencoder sensor, {levels} levels, cells of {cell}, {torch.cuda.get_device_name(0)}",
             f"median [min, max] of {args.rounds} repetitions of (HIP-event time of `iters` back-to-back calls) / iters, after a warm-up",
             f"yardstick: device-to-device copy of 822 MB, read plus written bytes: {copy[0]:.0f} [{copy[1]:.0f}, {copy[2]:.0f}] GB/s",
             ""]
    for n, hw, iters in ((1, (240, 320), 200), (256, (224, 224), 10)):
        H, W = hw
        ae = Autoencoder(blob, in_hw=hw, levels=levels, cell=cell, max_batch=n)
        g = ae.geometry
        frames = torch.randint(0, 256, (n, H, W, 3), dtype=torch.uint8, device="cuda")
        gh, gw = ae.grid
        err_map = torch.empty((n, gh, gw), dtype=torch.float32, device="cuda")
        rec = torch.empty((n, 8), dtype=torch.int32, device="cuda")

        def score():
            st = lib.fav_ae_score(ae._h, frames.data_ptr(), n, 0, err_map.data_ptr(), rec.data_ptr(), None, stream)
            assert st == 0, lib.fav_last_error(None)
        t_score = timed_us(score, iters, args.rounds)
        t_py = timed_us(lambda: ae.score(frames), iters, args.rounds)
        # the decode launch alone, and the GEMM in front of it
        hL, wL, m = g["h"][levels], g["w"][levels], levels - 1
        rows_c = n * hL * wL
        rows = rows_c * 4 ** m
        hidden = torch.randn((rows, 64), device="cuda").clamp_(min=0).to(torch.bfloat16)
        wg = torch.from_numpy(A._bf16_bits(layers[-1][0]).view(np.int16)).cuda()
        b3 = torch.from_numpy(layers[-1][1]).cuda()

        def decode():
            st = lib.fav_op_ae_decode_compare(hidden.data_ptr(), n, hL, wL, m, wg.data_ptr(), b3.data_ptr(), frames.data_ptr(), 0, H, W, cell,
                                              float("inf"), None, err_map.data_ptr(), rec.data_ptr(), None, stream)
            assert st == 0, lib.fav_last_error(None)
        t_dec = timed_us(decode, iters, args.rounds)
        x = torch.randn((rows_c, 128), device="cuda").to(torch.bfloat16)
        w2 = torch.from_numpy(A._bf16_bits(layers[levels][0]).view(np.int16)).cuda()
        b2 = torch.from_numpy(layers[levels][1]).cuda()
        d = _lib.FavConvDesc()
        d.x, d.w, d.bias, d.res, d.y = x.data_ptr(), w2.data_ptr(), b2.data_ptr(), None, hidden.data_ptr()
        d.n_frames, d.H, d.W, d.Cin, d.Cout, d.kh, d.kw, d.stride, d.pad = n, hL * wL, 1, 128, 256, 1, 1, 1, 0
        d.relu, d.out_f32, d.math_mode = 1, 0, 0
        d.drop.site = -1

        def gemm():
            st = lib.fav_op_conv2d(C.byref(d), stream)
            assert st == 0, lib.fav_last_error(None)
        t_gemm = timed_us(gemm, iters, args.rounds)
        dec_bytes = n * g["h"][1] * g["w"][1] * 128 + n * H * W * 3 + n * gh * gw * 4 + n * 32
        gemm_bytes = rows_c * 128 * 2 + rows * 64 * 2 + 256 * 128 * 2
        gbs = tuple(dec_bytes / (v * 1e-6) / 1e9 for v in (t_dec[0], t_dec[2], t_dec[1]))
        ggbs = gemm_bytes / (t_gemm[0] * 1e-6) / 1e9
        lines += [f"n = {n}, {H} x {W} (iters = {iters}; workspace {g['workspace_bytes'] / 1e6:.0f} MB)",
                  f"  fav_ae_score, {levels + 1 + levels - 1 + 2} launches:          {fmt3(t_score)} us a call, {n / (t_score[0] * 1e-6):.0f} frames/s",
                  f"  Autoencoder.score on device frames:   {fmt3(t_py)} us a call (allocates its outputs, unpacks the records)",
                  f"  fav_op_ae_decode_compare, 2 launches: {fmt3(t_dec)} us a call; {dec_bytes / 1e6:.2f} MB algorithmic: "
                  f"{fmt3(gbs, 0)} GB/s, {gbs[0] / copy[0]:.2f} of the copy",
                  f"  the GEMM in front of it (128 -> 256):  {fmt3(t_gemm)} us a call; {gemm_bytes / 1e6:.2f} MB: {ggbs:.0f} GB/s", ""]
        ae.close()
    text = "\n".join(lines)
    os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
    with open(args.out, "w") as f:
        f.write(text)
    print(text)


if __name__ == "__main__":
    main()
