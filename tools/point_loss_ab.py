#!/usr/bin/env python3
"""Interleaved in-process A/B of the pointwise data terms (wire_point_loss_grad) against wire_mse_grad on the same
buffers, which moves the same bytes and is the yardstick: per kind and weight form, at the denoise driver's batch
(wire_image_denoise.py: maxpoints = 256 * 256 rows, O = 3) and at the occupancy driver's (wire_occupancy.py: 200 000
rows, O = 1), the loss kernel alone with its final-sum launch, timed with events on the stream over back-to-back calls.
Blocks of timed calls alternate between the variants, so clock / temperature drift hits all alike; the median over the
blocks is reported with the spread, the algorithm's bytes, the rate they imply and the ratio to wire_mse_grad in the
same run.  Then one whole step: FusedTrainer.step_loss("l1") against step_tv(0.0) on the same 256 x 256 grid with the
headline net.  A measurement, not a gate: it prints what it finds.
    python3 tools/point_loss_ab.py > profiles/point_loss_ab.txt
    python3 tools/point_loss_ab.py --blocks 2 --kernel-reps 50 --reps 5          # a short run
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
KINDS = ("mse", "l1", "huber", "logistic")


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


def kernels_at(tag, n, O, use_idx, a):
    L = _lib.lib()
    s = torch.cuda.current_stream(dev).cuda_stream
    g = torch.Generator().manual_seed(n + O)
    T = n
    y = torch.randn(n, O, generator=g).to(dev)
    t = torch.rand(T, O, generator=g).to(dev)
    w_row, w_elem = torch.rand(T, generator=g).to(dev), torch.rand(T, O, generator=g).to(dev)
    idx = torch.randperm(T, generator=g)[:n].to(dev) if use_idx else None
    gy, loss, part = torch.empty(n, O, device=dev), torch.empty(1, device=dev), torch.empty(4096, device=dev)
    ip = None if idx is None else idx.data_ptr()

    def point(kind, w):
        wp, wpe = (None, 0) if w is None else (w.data_ptr(), int(w.dim() == 2))
        code = _lib.LOSS_KIND[kind]
        return lambda: _lib.check(L.wire_point_loss_grad(s, code, 0.3, y.data_ptr(), t.data_ptr(), wp, wpe, ip, 0, n, O,
                                                         1.0, gy.data_ptr(), loss.data_ptr(), None, part.data_ptr()))

    variants = {"wire_mse_grad": (lambda: _lib.check(L.wire_mse_grad(s, y.data_ptr(), t.data_ptr(), ip, 0, n, O, 1.0,
                                                                      gy.data_ptr(), loss.data_ptr(), None,
                                                                      part.data_ptr())), 0)}
    for kind in KINDS:
        for wname, w, wbytes in (("none", None, 0), ("row", w_row, 4 * n), ("elem", w_elem, 4 * n * O)):
            variants[f"point {kind:8s} weight {wname}"] = (point(kind, w), wbytes)
    res = {k: [] for k in variants}
    for _ in range(a.blocks):
        for k, (fn, _) in variants.items():
            event_timed(fn, 20)
            res[k].append(event_timed(fn, a.kernel_reps))
    rows = "idx = a permutation" if use_idx else "a range"
    print(f"# {tag}: n = {n}, O = {O}, rows by {rows}; loss kernel + final sum, event time over {a.kernel_reps} "
          f"back-to-back calls, median of {a.blocks} alternating blocks", flush=True)
    base = statistics.median(res["wire_mse_grad"])
    for k, (_, wbytes) in variants.items():
        v = res[k]
        med = statistics.median(v)
        # the algorithm's traffic: y and target read once, g_y written once, the weight (and the indices) read once
        b = 3 * 4 * n * O + wbytes + (8 * n if use_idx else 0)
        print(f"{tag}: {k:32s} median {med:8.2f} us  min {min(v):8.2f}  max {max(v):8.2f}  algorithmic "
              f"{b / 1e6:6.2f} MB = {b / med * 1e-3:7.1f} GB/s  / wire_mse_grad {med / base:5.2f} x", flush=True)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--blocks", type=int, default=7)
    ap.add_argument("--kernel-reps", type=int, default=2000)
    ap.add_argument("--reps", type=int, default=100)
    a = ap.parse_args()
    p = torch.cuda.get_device_properties(dev)
    print(f"# {p.name} ({p.gcnArchName}, {p.multi_processor_count} CUs), torch {torch.__version__}, HIP {torch.version.hip}",
          flush=True)
    for use_idx in (False, True):
        kernels_at("denoise", 256 * 256, 3, use_idx, a)
        kernels_at("occupancy", 200000, 1, use_idx, a)

    # ---- one whole step on the denoise driver's grid, the headline net (bench.py's)
    H = W = 256
    torch.manual_seed(0)
    model = models.get_INR(nonlin="wire", in_features=2, out_features=3, hidden_features=363, hidden_layers=4,
                           first_omega_0=20.0, hidden_omega_0=20.0, scale=30.0).to(dev)
    target = torch.rand(H * W, 3, generator=torch.Generator().manual_seed(1)).to(dev)
    tr = FusedTrainer(model, (H, W), target, lr=1e-4)
    mask = (torch.rand(H * W, generator=torch.Generator().manual_seed(2)) < 0.5).float().to(dev)
    steps = {"step_tv(0.0)": lambda: tr.step_tv(0.0),
             "step_loss('mse')": lambda: tr.step_loss("mse"),
             "step_loss('l1')": lambda: tr.step_loss("l1"),
             "step_loss('l1', weight=mask)": lambda: tr.step_loss("l1", weight=mask),
             "step_loss('logistic')": lambda: tr.step_loss("logistic")}
    res = {k: [] for k in steps}
    for _ in range(a.blocks):
        for k, fn in steps.items():
            timed(fn, 5)
            res[k].append(timed(fn, a.reps))
    print(f"# whole optimizer step on {H} x {W} x 3, host clock over {a.reps} steps ending in a synchronise, median of "
          f"{a.blocks} alternating blocks", flush=True)
    base = statistics.median(res["step_tv(0.0)"])
    for k, v in res.items():
        med = statistics.median(v)
        print(f"step: {k:32s} median {med:9.1f} us  min {min(v):9.1f}  max {max(v):9.1f}  / step_tv(0.0) "
              f"{med / base:6.4f} x  ({med - base:+.1f} us)", flush=True)


if __name__ == "__main__":
    main()
