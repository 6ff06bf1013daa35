#!/usr/bin/env python3
"""Interleaved in-process A/B of the TV prior on the three operator steps, with the headline net (bench.py's: wire,
4 hidden layers, hidden_features=363 -> 256 complex features, omega_0 = 20, s_0 = 30):
    FusedTrainer.step_downsampled(gt, 2, lambda_tv)               512 x 512, O = 3
    FusedTrainer.step_radon(sinogram, thetas, lambda_tv)          512 x 512, O = 1, 17 angles
    FusedTrainer.step_coded(coded, masks, 8, lambda_tv, lambda_tv_t)   128 x 128 x 16, O = 1
each against the same call with lambda 0 (which does not launch the kernel; the video step once with sparse masks and
once with every frame open), and wire_tv_add_grad on its own at 512 x 512 x 1 x 3, at the video step's shape and at a
larger video shape, timed with events on the stream.  Blocks of timed calls alternate between the
variants, so clock / temperature drift hits both alike; every timed window ends in a device synchronise.  A measurement
without a target: it prints what it finds.
    python3 tools/tv_reg_ab.py > profiles/tv_reg_ab.txt
    python3 tools/tv_reg_ab.py --size 64x64 --video 16x16x8 --kernel-video 32x32x8x3 --blocks 2 --reps 10   # small shapes
"""
import argparse
import os
import sys
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
import torch

from wire_amd import _lib
from wire_amd.modules import models
from wire_amd.trainer import FusedTrainer

dev = torch.device("cuda:0")


def timed(fn, reps):
    """Host-clock microseconds per call over reps calls ending in a synchronise."""
    torch.cuda.synchronize()
    t0 = time.perf_counter()
    for _ in range(reps):
        fn()
    torch.cuda.synchronize()
    return (time.perf_counter() - t0) / reps * 1e6


def event_timed(fn, reps):
    """Event microseconds per call: reps back-to-back calls between two events on the stream."""
    a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    torch.cuda.synchronize()
    a.record()
    for _ in range(reps):
        fn()
    b.record()
    torch.cuda.synchronize()
    return a.elapsed_time(b) / reps * 1e3


def net(D, O):
    torch.manual_seed(0)
    return models.get_INR(nonlin="wire", in_features=D, out_features=O, hidden_features=363, hidden_layers=4,
                          first_omega_0=20.0, hidden_omega_0=20.0, scale=30.0).to(dev)


def ab(tag, variants, blocks, reps):
    """variants: {label: fn}, the first the lambda-0 baseline."""
    res = {k: [] for k in variants}
    for _ in range(blocks):
        for k, fn in variants.items():
            timed(fn, 3)
            res[k].append(timed(fn, reps))
    base = None
    for k, v in res.items():
        line = f"{tag}: {k:44s} mean {sum(v) / len(v):9.1f} us  min {min(v):9.1f} us"
        if base is None:
            base = min(v)
        else:
            line += f"  / lambda 0 (min) {min(v) / base:.4f} x  (+{min(v) - base:.1f} us)"
        print(line, flush=True)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--size", default="512x512", help="H x W of the image steps and of the first kernel shape")
    ap.add_argument("--video", default="128x128x16", help="H x W x T of the video step")
    ap.add_argument("--kernel-video", default="256x256x16x3", help="H x W x T x O of the second kernel shape")
    ap.add_argument("--lambda-tv", type=float, default=2.0 ** -20)
    ap.add_argument("--blocks", type=int, default=5)
    ap.add_argument("--reps", type=int, default=50)
    ap.add_argument("--kernel-reps", type=int, default=2000)
    a = ap.parse_args()
    H, W = (int(v) for v in a.size.split("x"))
    VH, VW, VT = (int(v) for v in a.video.split("x"))
    lam = a.lambda_tv
    p = torch.cuda.get_device_properties(dev)
    print(f"# {p.name} ({p.gcnArchName}, {p.multi_processor_count} CUs), torch {torch.__version__}, HIP {torch.version.hip}; "
          f"lambda {lam:g}, {a.blocks} alternating blocks of {a.reps} steps, host clock, each ending in a synchronise",
          flush=True)
    gen = torch.Generator().manual_seed(1)

    # ---- super-resolution
    tr = FusedTrainer(net(2, 3), (H, W), None, lr=1e-4)
    gt = torch.rand((H // 2) * (W // 2), 3, generator=gen).to(dev)
    print(f"# step_downsampled: {H} x {W} x 3, scale 2", flush=True)
    ab("step_downsampled", {"lambda_tv 0": lambda: tr.step_downsampled(gt, 2),
                            "lambda_tv": lambda: tr.step_downsampled(gt, 2, lambda_tv=lam)}, a.blocks, a.reps)
    print(f"step_downsampled: tv_parts [loss, data, tv_s, tv_t] {tr.tv_parts.tolist()}", flush=True)
    del tr

    # ---- CT
    A = 17
    tr = FusedTrainer(net(2, 1), (H, W), None, lr=1e-4)
    th = torch.linspace(0, 180, A)
    sino = torch.rand(A * W, generator=gen).to(dev) * H
    print(f"# step_radon: {H} x {W} x 1, {A} angles", flush=True)
    ab("step_radon", {"lambda_tv 0": lambda: tr.step_radon(sino, th),
                      "lambda_tv": lambda: tr.step_radon(sino, th, lambda_tv=lam)}, a.blocks, a.reps)
    print(f"step_radon: tv_parts [loss, data, tv_s, tv_t] {tr.tv_parts.tolist()}", flush=True)
    del tr

    # ---- video compressive sensing
    nframes = 8
    tr = FusedTrainer(net(3, 1), (VH, VW, VT), None, lr=1e-4)
    Cp = (VT + nframes - 1) // nframes + 1
    coded = torch.rand(Cp * VH * VW, generator=gen).to(dev)
    sparse = (torch.rand(VH * VW * VT, generator=gen) < 1.0 / nframes).float().to(dev)
    # the coding's dL/dy is exactly 0 wherever the mask is closed and the prior's term is dense, so the backward after
    # it sees other data; with every frame open both are dense and the difference is the kernel's own time
    for tag, masks in ((f"1 frame in {nframes} open", sparse), ("every frame open", torch.ones_like(sparse))):
        print(f"# step_coded: {VH} x {VW} x {VT} x 1, nframes {nframes}, masks: {tag}", flush=True)
        ab("step_coded", {"lambdas 0": lambda: tr.step_coded(coded, masks, nframes),
                          "lambda_tv": lambda: tr.step_coded(coded, masks, nframes, lambda_tv=lam),
                          "lambda_tv_t": lambda: tr.step_coded(coded, masks, nframes, lambda_tv_t=lam),
                          "lambda_tv and lambda_tv_t": lambda: tr.step_coded(coded, masks, nframes, lambda_tv=lam,
                                                                             lambda_tv_t=lam / 2)}, a.blocks, a.reps)
        print(f"step_coded: tv_parts [loss, data, tv_s, tv_t] {tr.tv_parts.tolist()}", flush=True)
    del tr

    # ---- the kernel on its own (its reduction launch included)
    L = _lib.lib()
    s = torch.cuda.current_stream(dev).cuda_stream
    part, out4, data = torch.empty(2048, device=dev), torch.empty(4, device=dev), torch.zeros(1, device=dev)
    print(f"# wire_tv_add_grad alone, event time over {a.kernel_reps} back-to-back calls; algorithmic traffic = y in, "
          f"g_y in and out; issued = + the six neighbours of every element", flush=True)
    shapes = [(H, W, 1, 3), (VH, VW, VT, 1), tuple(int(v) for v in a.kernel_video.split("x"))]
    for (h, w, t, o) in shapes:
        n = h * w * t * o
        y = torch.randn(n, generator=gen).to(dev)
        gy = torch.zeros(n, device=dev)
        res = {}
        calls = {"lambda_s and lambda_t": (lam, lam / 2), "lambda_s alone": (lam, 0.0)}
        for _ in range(a.blocks):
            for k, (ls, lt) in calls.items():
                fn = lambda: _lib.check(L.wire_tv_add_grad(s, y.data_ptr(), h, w, t, o, ls, lt, data.data_ptr(),
                                                           gy.data_ptr(), out4.data_ptr(), part.data_ptr()))
                event_timed(fn, 20)
                res.setdefault(k, []).append(event_timed(fn, a.kernel_reps))
        nb = 6 if t > 1 else 4
        for k, v in res.items():
            us = min(v)
            print(f"kernel {h} x {w} x {t} x {o}: {k:24s} mean {sum(v) / len(v):8.1f} us  min {us:8.1f} us  "
                  f"algorithmic {12 * n / 1e6:7.2f} MB = {12 * n / us * 1e-3:7.1f} GB/s; loads + stores issued "
                  f"{4 * n * (3 + nb) / 1e6:7.2f} MB = {4 * n * (3 + nb) / us * 1e-3:7.1f} GB/s", flush=True)
        del y, gy


if __name__ == "__main__":
    main()
