#!/usr/bin/env python3
"""Interleaved in-process timing of the volume-rendering kernels (wire_render.hip): wire_ray_samples,
wire_composite_fwd, wire_composite_bwd and wire_composite_mse_grad at 4096 rays x 64 and x 192 samples with O = 4,
against wire_point_loss_grad ("mse", which forwards to wire_mse_grad) on the same number of rows -- the yardstick: per
row of 4 floats it reads y and a target and writes g_y, 48 B, where the compositing loss kernel reads y, ts and deltas
and writes g_y, 40 B (each buffer counted once: the reverse sweep reads the row a second time, out of cache at these
sizes).  Event time over back-to-back calls, blocks of timed calls alternating
between the variants, the median over the blocks with the spread, the algorithm's bytes and the rate they imply.  Then
one whole step: FusedTrainer.step_rays against step_samples("mse") on R * S rows of the same net (siren 4 x 256 and
wire 4 x 256, D = 3, O = 4).  A measurement, not a gate: it prints what it finds.
    python3 tools/render_ab.py > profiles/render_ab.txt
    python3 tools/render_ab.py --blocks 2 --kernel-reps 50 --reps 5          # a short run
"""
import argparse
import os
import statistics
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


def kernels_at(R, S, a):
    L = _lib.lib()
    s = torch.cuda.current_stream(dev).cuda_stream
    O, Cc, n = 4, 3, R * S
    g = torch.Generator().manual_seed(R + S)
    rays = torch.randn(R, 6, generator=g).to(dev)
    u = torch.rand(R, S, generator=g).to(dev)
    y = torch.randn(n, O, generator=g).to(dev)
    tgt = torch.rand(R, Cc, generator=g).to(dev)
    ptgt = torch.rand(n, O, generator=g).to(dev)
    bg = torch.rand(Cc, generator=g).to(dev)
    coords, ts, dl = torch.empty(n, 3, device=dev), torch.empty(R, S, device=dev), torch.empty(R, S, device=dev)
    gy, loss, part = torch.empty(n, O, device=dev), torch.empty(1, device=dev), torch.empty(4096, device=dev)
    rgb, acc, depth = torch.empty(R, Cc, device=dev), torch.empty(R, device=dev), torch.empty(R, device=dev)
    g_rgb = torch.randn(R, Cc, generator=g).to(dev)
    _lib.check(L.wire_ray_samples(s, rays.data_ptr(), None, 0.5, 4.5, u.data_ptr(), R, S, coords.data_ptr(),
                                  ts.data_ptr(), dl.data_ptr()))
    f4 = 4
    # the algorithm's traffic per call, each buffer counted once
    variants = {
        "wire_point_loss_grad mse (yardstick)": (
            lambda: _lib.check(L.wire_point_loss_grad(s, 0, 1.0, y.data_ptr(), ptgt.data_ptr(), None, 0, None, 0, n, O, 1.0,
                                                      gy.data_ptr(), loss.data_ptr(), None, part.data_ptr())),
            3 * f4 * n * O),
        "wire_ray_samples (jitter)": (
            lambda: _lib.check(L.wire_ray_samples(s, rays.data_ptr(), None, 0.5, 4.5, u.data_ptr(), R, S,
                                                  coords.data_ptr(), ts.data_ptr(), dl.data_ptr())),
            f4 * (6 * R + n + 5 * n)),
        "wire_composite_fwd": (
            lambda: _lib.check(L.wire_composite_fwd(s, y.data_ptr(), ts.data_ptr(), dl.data_ptr(), bg.data_ptr(), R, S, O,
                                                    0, rgb.data_ptr(), acc.data_ptr(), depth.data_ptr())),
            f4 * (n * O + 2 * n + 5 * R)),
        "wire_composite_bwd": (
            lambda: _lib.check(L.wire_composite_bwd(s, y.data_ptr(), ts.data_ptr(), dl.data_ptr(), bg.data_ptr(),
                                                    g_rgb.data_ptr(), None, None, R, S, O, 0, gy.data_ptr())),
            f4 * (2 * n * O + 2 * n + 3 * R)),
        "wire_composite_mse_grad": (
            lambda: _lib.check(L.wire_composite_mse_grad(s, y.data_ptr(), ts.data_ptr(), dl.data_ptr(), bg.data_ptr(),
                                                         tgt.data_ptr(), R, S, O, 0, 1.0, gy.data_ptr(), loss.data_ptr(),
                                                         rgb.data_ptr(), part.data_ptr())),
            f4 * (2 * n * O + 2 * n + 6 * R)),
    }
    res = {k: [] for k in variants}
    for _ in range(a.blocks):
        for k, (fn, _) in variants.items():
            event_timed(fn, 20)
            res[k].append(event_timed(fn, a.kernel_reps))
    tag = f"{R} x {S}"
    print(f"# {tag}: R = {R} rays, S = {S} samples, O = {O} ({n} rows); event time over {a.kernel_reps} back-to-back "
          f"calls, median of {a.blocks} alternating blocks", flush=True)
    base = statistics.median(res["wire_point_loss_grad mse (yardstick)"])
    for k, (_, b) in variants.items():
        v = res[k]
        med = statistics.median(v)
        print(f"{tag}: {k:38s} median {med:8.2f} us  min {min(v):8.2f}  max {max(v):8.2f}  algorithmic "
              f"{b / 1e6:6.2f} MB = {b / med * 1e-3:7.1f} GB/s  / yardstick {med / base:5.2f} x", flush=True)


def steps_at(kind, R, S, a):
    torch.manual_seed(0)
    hp = dict(first_omega_0=30.0, hidden_omega_0=30.0, scale=10.0) if kind == "siren" else \
        dict(first_omega_0=20.0, hidden_omega_0=20.0, scale=30.0)
    model = models.get_INR(nonlin=kind, in_features=3, out_features=4, hidden_features=256, hidden_layers=4,
                           **hp).to(dev)
    tr = FusedTrainer(model, (4, 4, 4), None, lr=1e-5)
    g = torch.Generator().manual_seed(1)
    o = torch.randn(R, 3, generator=g)
    o = 2.5 * o / o.norm(dim=1, keepdim=True)
    d = (torch.rand(R, 3, generator=g) - 0.5) - o
    rays = torch.cat([o, d / d.norm(dim=1, keepdim=True)], 1).to(dev).contiguous()
    tgt = torch.rand(R, 3, generator=g).to(dev)
    xs = (torch.rand(R * S, 3, generator=g) * 2 - 1).to(dev)
    vals = torch.rand(R * S, 4, generator=g).to(dev)
    steps = {"step_samples('mse')": lambda: tr.step_samples(xs, vals, "mse"),
             "step_rays (midpoints)": lambda: tr.step_rays(rays, tgt, 1.5, 3.5, S)}
    res = {k: [] for k in steps}
    for _ in range(a.blocks):
        for k, fn in steps.items():
            timed(fn, 5)
            res[k].append(timed(fn, a.reps))
    print(f"# whole optimizer step, {kind} 4 x 256, D = 3, O = 4, {R} rays x {S} samples = {R * S} rows; host clock over "
          f"{a.reps} steps ending in a synchronise, median of {a.blocks} alternating blocks", flush=True)
    base = statistics.median(res["step_samples('mse')"])
    for k, v in res.items():
        med = statistics.median(v)
        print(f"step {kind} {R} x {S}: {k:24s} median {med:9.1f} us  min {min(v):9.1f}  max {max(v):9.1f}  / "
              f"step_samples {med / base:6.4f} x  ({med - base:+.1f} us)", flush=True)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--blocks", type=int, default=7)
    ap.add_argument("--kernel-reps", type=int, default=500)
    ap.add_argument("--reps", type=int, default=30)
    a = ap.parse_args()
    p = torch.cuda.get_device_properties(dev)
    print(f"# {p.name} ({p.gcnArchName}, {p.multi_processor_count} CUs), torch {torch.__version__}, HIP {torch.version.hip}",
          flush=True)
    for S in (64, 192):
        kernels_at(4096, S, a)
    for kind in ("siren", "wire"):
        steps_at(kind, 4096, 64, a)


if __name__ == "__main__":
    main()
