#!/usr/bin/env python3
"""Interleaved in-process A/B of the SSIM-regularised training step on a 512 x 512, O = 3 grid with the headline net
(bench.py's: wire, 4 hidden layers, hidden_features=363 -> 256 complex features, omega_0 = 20, s_0 = 30):
FusedTrainer.step_ssim(lambda) against FusedTrainer.step_tv(0.0) -- the same full-grid forward and backward with the plain
MSE as the loss -- and the gradient kernels on their own, timed with events on the stream.  Blocks of timed calls
alternate between the variants, so clock / temperature drift hits both alike; every timed window ends in a device
synchronise.  A measurement, not a gate: it prints what it finds.
    python3 tools/ssim_loss_ab.py > profiles/ssim_loss_ab.txt
    python3 tools/ssim_loss_ab.py --size 96x64 --blocks 2 --reps 20          # a small shape
"""
import argparse
import os
import sys
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
import torch

from wire_amd import _lib, functional
from wire_amd.modules import models
from wire_amd.trainer import FusedTrainer

dev = torch.device("cuda:0")
O = 3


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


def report(tag, res, extra=None):
    for k, v in res.items():
        print(f"{tag}: {k:40s} mean {sum(v) / len(v):9.1f} us  min {min(v):9.1f} us"
              + (extra(k, min(v)) if extra else ""), flush=True)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--size", default="512x512")
    ap.add_argument("--lambda-ssim", type=float, default=0.1)
    ap.add_argument("--blocks", type=int, default=5)
    ap.add_argument("--reps", type=int, default=100)
    ap.add_argument("--kernel-reps", type=int, default=2000)
    a = ap.parse_args()
    H, W = (int(v) for v in a.size.split("x"))
    n = H * W
    p = torch.cuda.get_device_properties(dev)
    print(f"# {p.name} ({p.gcnArchName}, {p.multi_processor_count} CUs), torch {torch.__version__}, HIP {torch.version.hip}; "
          f"{H} x {W} x {O}, lambda_ssim {a.lambda_ssim:g}, {a.blocks} alternating blocks", flush=True)
    torch.manual_seed(0)
    model = models.get_INR(nonlin="wire", in_features=2, out_features=O, hidden_features=363, hidden_layers=4,
                           first_omega_0=20.0, hidden_omega_0=20.0, scale=30.0).to(dev)
    target = torch.rand(n, O, generator=torch.Generator().manual_seed(1)).to(dev)
    tr = FusedTrainer(model, (H, W), target, lr=1e-4)
    perm = torch.randperm(n, device=dev)
    half = perm[:n // 2].contiguous()

    # ---- the whole step
    steps = {"step_tv(0.0)": lambda: tr.step_tv(0.0),
             "step_ssim(0.0)": lambda: tr.step_ssim(0.0),
             "step_ssim(lambda)": lambda: tr.step_ssim(a.lambda_ssim),
             "step_ssim(lambda, window='uniform')": lambda: tr.step_ssim(a.lambda_ssim, window="uniform", data_range=1.0),
             "step_ssim(lambda, indices=perm[:n/2])": lambda: tr.step_ssim(a.lambda_ssim, indices=half)}
    res = {k: [] for k in steps}
    for _ in range(a.blocks):
        for k, fn in steps.items():
            timed(fn, 5)
            res[k].append(timed(fn, a.reps))
    print(f"# whole optimizer step, host clock over {a.reps} steps ending in a synchronise", flush=True)
    report("step", res)
    base = min(res["step_tv(0.0)"])
    for k in list(steps)[1:]:
        print(f"step: {k} / step_tv(0.0) (min) {min(res[k]) / base:.4f} x  (+{min(res[k]) - base:.1f} us)", flush=True)
    print(f"step: loss_parts [loss, mse, ssim] after the last step_ssim: {tr.loss_parts.tolist()}", flush=True)

    # ---- the loss and gradient kernels on their own, on the step's own buffers
    L = tr.L
    s = torch.cuda.current_stream(dev).cuda_stream
    y, gy, part, out3 = tr.y.data_ptr(), tr.gy.data_ptr(), tr.partial.data_ptr(), tr.loss_parts.data_ptr()
    t = tr.target.data_ptr()
    one = torch.ones(1, device=dev)
    wins = {k: functional._ssim_window(k) for k in ("gaussian", "uniform")}
    c1, c2 = 1e-4, 9e-4
    ws = torch.empty(max(_lib.check(L.wire_ssim_mse_grad_ws_bytes(H, W, O, 11)), _lib.check(L.wire_ssim_ws_bytes(H, W, O, 7))),
                     dtype=torch.uint8, device=dev)
    wp, wn = ws.data_ptr(), ws.numel()

    def fused(kind, lam, idx=None):
        taps, win, cov = wins[kind]
        return lambda: _lib.check(L.wire_ssim_mse_grad(s, y, H, W, O, t, taps, win, cov, c1, c2,
                                                       None if idx is None else idx.data_ptr(), 0,
                                                       n if idx is None else idx.numel(), lam, gy, out3, None, wp, wn))

    def bwd(kind):
        taps, win, cov = wins[kind]
        return lambda: _lib.check(L.wire_ssim_bwd(s, t, y, H, W, O, taps, win, cov, c1, c2, one.data_ptr(), gy, wp, wn))

    def fwd(kind):
        taps, win, cov = wins[kind]
        return lambda: _lib.check(L.wire_ssim(s, t, y, H, W, O, taps, win, cov, c1, c2, out3, None, wp, wn))

    kernels = {
        "wire_tv_mse_grad lambda 0, all rows": lambda: _lib.check(L.wire_tv_mse_grad(s, y, H, W, O, t, None, 0, n, 0.0, gy,
                                                                                     out3, None, part)),
        "wire_ssim_mse_grad lambda 0, all rows": fused("gaussian", 0.0),
        "wire_ssim_mse_grad gaussian, all rows": fused("gaussian", a.lambda_ssim),
        "wire_ssim_mse_grad uniform, all rows": fused("uniform", a.lambda_ssim),
        "wire_ssim_mse_grad gaussian, idx perm[:n/2]": fused("gaussian", a.lambda_ssim, half),
        "wire_ssim_bwd gaussian": bwd("gaussian"),
        "wire_ssim_bwd uniform": bwd("uniform"),
        "wire_ssim (the metric) gaussian": fwd("gaussian"),
        "wire_ssim (the metric) uniform": fwd("uniform"),
    }
    res = {k: [] for k in kernels}
    for _ in range(a.blocks):
        for k, fn in kernels.items():
            event_timed(fn, 20)
            res[k].append(event_timed(fn, a.kernel_reps))
    print(f"# kernels alone (their reduction launches included), event time over {a.kernel_reps} back-to-back calls",
          flush=True)
    img = 4 * n * O                                          # bytes of one H*W*O float array

    def extra(k, us):
        # the algorithm's traffic: y and target read once, g_y written once (the metric: two reads)
        b = 2 * img if "metric" in k else 3 * img
        return f"  algorithmic {b / 1e6:6.2f} MB = {b / us * 1e-3:7.1f} GB/s"
    report("kernel", res, extra)
    g, f = min(res["wire_ssim_bwd gaussian"]), min(res["wire_ssim (the metric) gaussian"])
    print(f"kernel: wire_ssim_bwd / wire_ssim (gaussian, min) {g / f:.2f} x", flush=True)
    print(f"kernel: wire_ssim_mse_grad gaussian - wire_tv_mse_grad lambda 0 (min) "
          f"{min(res['wire_ssim_mse_grad gaussian, all rows']) - min(res['wire_tv_mse_grad lambda 0, all rows']):.1f} us",
          flush=True)


if __name__ == "__main__":
    main()
