#!/usr/bin/env python3
"""Interleaved in-process A/B of the TV-regularised training step on a 512 x 512, O = 3 grid with the headline net
(bench.py's: wire, 4 hidden layers, hidden_features=363 -> 256 complex features, omega_0 = 20, s_0 = 30):
FusedTrainer.step_tv(lambda) against FusedTrainer.step_downsampled(target, 1) -- the same full-grid forward and backward
with the existing loss kernel (wire_avgpool_mse_grad at scale 1 is the plain full-grid MSE) -- and the two loss kernels on
their own, timed with events on the stream.  Blocks of timed calls alternate between the variants, so clock /
temperature drift hits both alike; every timed window ends in a device synchronise.  A measurement, not a gate: it
prints what it finds.
    python3 tools/tv_ab.py > profiles/tv_ab.txt
    python3 tools/tv_ab.py --size 96x64 --blocks 2 --reps 20          # a small shape
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
        print(f"{tag}: {k:34s} mean {sum(v) / len(v):9.1f} us  min {min(v):9.1f} us"
              + (extra(k, min(v)) if extra else ""), flush=True)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--size", default="512x512")
    ap.add_argument("--lambda-tv", type=float, default=2.0 ** -20)
    ap.add_argument("--blocks", type=int, default=5)
    ap.add_argument("--reps", type=int, default=100)
    ap.add_argument("--kernel-reps", type=int, default=5000)
    a = ap.parse_args()
    H, W = (int(v) for v in a.size.split("x"))
    n = H * W
    p = torch.cuda.get_device_properties(dev)
    print(f"# {p.name} ({p.gcnArchName}, {p.multi_processor_count} CUs), torch {torch.__version__}, HIP {torch.version.hip}; "
          f"{H} x {W} x {O}, lambda_tv {a.lambda_tv:g}, {a.blocks} alternating blocks", flush=True)
    torch.manual_seed(0)
    model = models.get_INR(nonlin="wire", in_features=2, out_features=O, hidden_features=363, hidden_layers=4,
                           first_omega_0=20.0, hidden_omega_0=20.0, scale=30.0).to(dev)
    target = torch.rand(n, O, generator=torch.Generator().manual_seed(1)).to(dev)
    tr = FusedTrainer(model, (H, W), target, lr=1e-4)
    perm = torch.randperm(n, device=dev)
    half = perm[:n // 2].contiguous()

    # ---- the whole step
    steps = {"step_downsampled(target, 1)": lambda: tr.step_downsampled(target, 1),
             "step_tv(lambda)": lambda: tr.step_tv(a.lambda_tv),
             "step_tv(lambda, indices=perm[:n/2])": lambda: tr.step_tv(a.lambda_tv, indices=half)}
    res = {k: [] for k in steps}
    for _ in range(a.blocks):
        for k, fn in steps.items():
            timed(fn, 5)
            res[k].append(timed(fn, a.reps))
    print(f"# whole optimizer step, host clock over {a.reps} steps ending in a synchronise", flush=True)
    report("step", res)
    base = min(res["step_downsampled(target, 1)"])
    for k in list(steps)[1:]:
        print(f"step: {k} / step_downsampled (min) {min(res[k]) / base:.4f} x  "
              f"(+{min(res[k]) - base:.1f} us)", flush=True)
    print(f"step: loss_parts [loss, mse, tv] after the last step_tv: {tr.loss_parts.tolist()}", flush=True)

    # ---- the loss kernels on their own, on the step's own buffers
    L = tr.L
    s = torch.cuda.current_stream(dev).cuda_stream
    y, gy, part, out3 = tr.y.data_ptr(), tr.gy.data_ptr(), tr.partial.data_ptr(), tr.loss_parts.data_ptr()
    t = tr.target.data_ptr()
    kernels = {
        "wire_avgpool_mse_grad scale 1": lambda: _lib.check(L.wire_avgpool_mse_grad(s, y, H, W, O, 1, t, gy, None, out3,
                                                                                    part)),
        "wire_mse_grad all rows": lambda: _lib.check(L.wire_mse_grad(s, y, t, None, 0, n, O, 1.0, gy, out3, None, part)),
        "wire_tv_mse_grad all rows": lambda: _lib.check(L.wire_tv_mse_grad(s, y, H, W, O, t, None, 0, n, a.lambda_tv, gy,
                                                                           out3, None, part)),
        "wire_tv_mse_grad idx perm[:n/2]": lambda: _lib.check(L.wire_tv_mse_grad(s, y, H, W, O, t, half.data_ptr(), 0,
                                                                                 half.numel(), a.lambda_tv, gy, out3,
                                                                                 None, part)),
        "wire_tv_fwd channel-last": lambda: _lib.check(L.wire_tv_fwd(s, y, O, H, W, O, 1, out3, part)),
        "wire_tv_bwd channel-last": lambda: _lib.check(L.wire_tv_bwd(s, y, O, H, W, O, 1, out3, gy)),
    }
    img = 4 * n * O                                          # bytes of one H*W*O float array
    # the algorithm's traffic: y and target read once, g_y written once (idx: + the rows' y, target, g_y again and the
    # indices); the TV function reads the image once, its backward reads it and writes the gradient
    algo = {"wire_avgpool_mse_grad scale 1": 3 * img, "wire_mse_grad all rows": 3 * img,
            "wire_tv_mse_grad all rows": 3 * img, "wire_tv_mse_grad idx perm[:n/2]": 2 * img + 4 * img // 2 + 8 * (n // 2),
            "wire_tv_fwd channel-last": img, "wire_tv_bwd channel-last": 2 * img}
    # what the TV kernels request from the memory system: every element also loads its four neighbours (forward: two)
    req = {"wire_tv_mse_grad all rows": 7 * img, "wire_tv_mse_grad idx perm[:n/2]": 6 * img + 4 * img // 2 + 8 * (n // 2),
           "wire_tv_fwd channel-last": 3 * img, "wire_tv_bwd channel-last": 6 * img}
    res = {k: [] for k in kernels}
    for _ in range(a.blocks):
        for k, fn in kernels.items():
            event_timed(fn, 20)
            res[k].append(event_timed(fn, a.kernel_reps))
    print(f"# loss kernels alone (their reduction launch included), event time over {a.kernel_reps} back-to-back calls",
          flush=True)

    def extra(k, us):
        txt = f"  algorithmic {algo[k] / 1e6:6.2f} MB = {algo[k] / us * 1e-3:7.1f} GB/s"
        if k in req:
            txt += f"; loads + stores issued {req[k] / 1e6:6.2f} MB = {req[k] / us * 1e-3:7.1f} GB/s"
        return txt
    report("kernel", res, extra)
    print(f"kernel: wire_tv_mse_grad / wire_avgpool_mse_grad (min) "
          f"{min(res['wire_tv_mse_grad all rows']) / min(res['wire_avgpool_mse_grad scale 1']):.2f} x", flush=True)


if __name__ == "__main__":
    main()
