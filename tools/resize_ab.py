#!/usr/bin/env python3
"""The resize operator: its three kernels per mode, and step_resized against step_downsampled.

At the SISR driver's shape (default a 452 x 680 x 3 image and the factor 4 of wire_SISR.py:46-78) it times, interleaved in
blocks so that clock and temperature drift hit every variant alike, and prints the MEDIAN over the blocks:
    wire_resize_fwd / wire_resize_bwd / wire_resize_mse_grad, per mode                       (events on the stream)
        (nearest, linear, cubic and area down by the factor; nearest, linear and cubic up by it -- the bilinear baseline)
    wire_avgpool_mse_grad on the same image                                                   (events on the stream)
    FusedTrainer.step_resized("area") and ("cubic") against step_downsampled, one net, one grid (host clock + synchronise)
with the algorithmic bytes of each kernel (every operand once; the tables are a few KB and not counted) and the rate they
imply.  A measurement without a pass mark: it prints what it finds, and says whether the whole step under the area
operator is slower than step_downsampled beyond the spread of the blocks.
    python3 tools/resize_ab.py > profiles/resize_ab.txt
    python3 tools/resize_ab.py --shape 64x48x3 --factor 4 --hidden 64 --blocks 2 --reps 5       # a small shape
"""
import argparse
import os
import statistics
import sys
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
import torch

from wire_amd import _lib, functional
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


def medians(variants, blocks, reps, timer):
    res = {k: [] for k in variants}
    for _ in range(blocks):
        for k, fn in variants.items():
            timer(fn, 2)
            res[k].append(timer(fn, reps))
    return {k: (statistics.median(v), min(v), max(v)) for k, v in res.items()}


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--shape", default="452x680x3", help="H x W x C of the high-resolution image")
    ap.add_argument("--factor", type=int, default=4)
    ap.add_argument("--kind", default="wire")
    ap.add_argument("--hidden", type=int, default=256)
    ap.add_argument("--layers", type=int, default=2)
    ap.add_argument("--blocks", type=int, default=5)
    ap.add_argument("--reps", type=int, default=10)
    ap.add_argument("--kernel-reps", type=int, default=50)
    a = ap.parse_args()
    H, W, Cc = (int(v) for v in a.shape.split("x"))
    f = a.factor
    Hl, Wl = H // f, W // f
    assert Hl * f == H and Wl * f == W, "the factor must divide both sides (step_downsampled drops a ragged border)"
    p = torch.cuda.get_device_properties(dev)
    print(f"# {p.name} ({p.gcnArchName}, {p.multi_processor_count} CUs), torch {torch.__version__}, HIP "
          f"{torch.version.hip}; image {H} x {W} x {Cc}, factor {f}; {a.blocks} alternating blocks, median [min .. max]",
          flush=True)
    L = _lib.lib()
    s = torch.cuda.current_stream(dev).cuda_stream
    gen = torch.Generator().manual_seed(1)
    hr = torch.rand(H, W, Cc, generator=gen).to(dev)
    lr = torch.rand(Hl, Wl, Cc, generator=gen).to(dev)
    ghr, glr = torch.empty_like(hr), torch.empty_like(lr)
    loss, part = torch.empty(1, device=dev), torch.empty(1024, device=dev)
    ws = torch.empty(_lib.check(L.wire_resize_mse_grad_ws_bytes(Hl, Wl, Cc)), dtype=torch.uint8, device=dev)
    nhr, nlr = 4 * hr.numel(), 4 * lr.numel()

    variants, algo = {}, {}
    for mode in ("nearest", "linear", "cubic", "area"):
        g = functional.resize_geometry(H, W, (Wl, Hl), None, None, mode)
        tab = functional.resize_tables(g, dev)
        variants[f"fwd {mode} down"] = lambda g=g, tab=tab: _lib.check(
            L.wire_resize_fwd(s, tab.data_ptr(), *g, hr.data_ptr(), Cc, glr.data_ptr()))
        variants[f"bwd {mode} down"] = lambda g=g, tab=tab: _lib.check(
            L.wire_resize_bwd(s, tab.data_ptr(), *g, lr.data_ptr(), Cc, ghr.data_ptr()))
        variants[f"mse_grad {mode} down"] = lambda g=g, tab=tab: _lib.check(
            L.wire_resize_mse_grad(s, tab.data_ptr(), *g, hr.data_ptr(), Cc, lr.data_ptr(), ghr.data_ptr(), None,
                                   loss.data_ptr(), ws.data_ptr(), ws.numel(), part.data_ptr()))
        algo[f"fwd {mode} down"] = algo[f"bwd {mode} down"] = nhr + nlr
        algo[f"mse_grad {mode} down"] = 2 * nhr + 4 * nlr      # y, g_y; gt_lr, the residual written and read, ... once more
        if mode != "area":
            gu = functional.resize_geometry(Hl, Wl, (W, H), None, None, mode)
            tabu = functional.resize_tables(gu, dev)
            variants[f"fwd {mode} up"] = lambda gu=gu, tabu=tabu: _lib.check(
                L.wire_resize_fwd(s, tabu.data_ptr(), *gu, lr.data_ptr(), Cc, ghr.data_ptr()))
            variants[f"bwd {mode} up"] = lambda gu=gu, tabu=tabu: _lib.check(
                L.wire_resize_bwd(s, tabu.data_ptr(), *gu, hr.data_ptr(), Cc, glr.data_ptr()))
            algo[f"fwd {mode} up"] = algo[f"bwd {mode} up"] = nhr + nlr
    variants["wire_avgpool_mse_grad"] = lambda: _lib.check(
        L.wire_avgpool_mse_grad(s, hr.data_ptr(), H, W, Cc, f, lr.data_ptr(), ghr.data_ptr(), None, loss.data_ptr(),
                                part.data_ptr()))
    algo["wire_avgpool_mse_grad"] = 2 * nhr + nlr
    k = medians(variants, a.blocks, a.kernel_reps, event_timed)
    for name, (med, lo, hi) in k.items():
        print(f"kernels: {name:24s} {med:8.1f} us [{lo:8.1f} .. {hi:8.1f}]  algorithmic {algo[name] / 1e6:6.2f} MB = "
              f"{algo[name] / med * 1e-3:8.1f} GB/s", flush=True)
    print(f"kernels: mse_grad area / wire_avgpool_mse_grad {k['mse_grad area down'][0] / k['wire_avgpool_mse_grad'][0]:.2f} x; "
          f"mse_grad cubic / area {k['mse_grad cubic down'][0] / k['mse_grad area down'][0]:.2f} x", flush=True)

    # ---- the step: one net, one grid, the three losses in alternating blocks
    torch.manual_seed(0)
    hp = (8.0, 8.0, 9.0) if a.kind == "wire" else (30.0, 30.0, 10.0)
    model = models.get_INR(nonlin=a.kind, in_features=2, out_features=Cc, hidden_features=a.hidden,
                           hidden_layers=a.layers, first_omega_0=hp[0], hidden_omega_0=hp[1], scale=hp[2]).to(dev)
    tr = FusedTrainer(model, (H, W), None, lr=1e-4)
    gt = lr.reshape(Hl * Wl, Cc).contiguous()
    steps = medians({"step_downsampled": lambda: tr.step_downsampled(gt, f),
                     "step_resized area": lambda: tr.step_resized(gt, (Hl, Wl), "area"),
                     "step_resized cubic": lambda: tr.step_resized(gt, (Hl, Wl), "cubic")}, a.blocks, a.reps, timed)
    print(f"# steps: {a.kind} {a.layers} x {a.hidden}, {H * W} rows, O = {Cc}; the tables of both geometries are built in the "
          f"warm-up calls and reused", flush=True)
    for name, (med, lo, hi) in steps.items():
        print(f"step: {name:20s} {med:10.1f} us [{lo:10.1f} .. {hi:10.1f}]", flush=True)
    d, ra, rc = steps["step_downsampled"], steps["step_resized area"], steps["step_resized cubic"]
    spread = max(d[2] - d[1], ra[2] - ra[1])
    verdict = "slower than" if ra[0] - d[0] > spread else ("faster than" if d[0] - ra[0] > spread else
                                                           "within the blocks' spread of")
    print(f"step: step_resized(area) / step_downsampled {ra[0] / d[0]:.3f} x ({ra[0] - d[0]:+.1f} us, spread {spread:.1f} us): "
          f"{verdict} step_downsampled; cubic / area {rc[0] / ra[0]:.3f} x", flush=True)


if __name__ == "__main__":
    main()
