#!/usr/bin/env python3
"""Interleaved in-process A/B of the bspline_cubic training step (and the forward-only render) against bspline_form at
the same shape: blocks of timed steps alternate between the two nets, so clock / temperature drift hits both alike.
    python3 tools/bspline_cubic_ab.py [OUT.txt]   # 2 x 256 on 256 x 256 (65 536 rows per step) and 4 x 256 on a
                                                  # 512 x 512 grid (262 144 rows; its render is the 512^2 render)
The spread of the interleaved repetitions (max - min of a net's block means, relative to its median) is the margin the
ratio of the medians is read against."""
import os
import statistics
import sys
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
import torch

from wire_amd.modules import bspline_cubic, models
from wire_amd.trainer import FusedTrainer

dev = torch.device("cuda:0")
REPS = 7


def trainers(L, side):
    out = {}
    torch.manual_seed(0)
    out["bspline_cubic"] = bspline_cubic.INR(2, 256, L, 0, 3, scale=15.0).to(dev)
    torch.manual_seed(0)
    out["bspline_form"] = models.get_INR(nonlin="bspline_form", in_features=2, out_features=3, hidden_features=256,
                                         hidden_layers=L, scale=1 / 9).to(dev)
    target = torch.rand(side * side, 3)
    return {k: FusedTrainer(m, (side, side), target, lr=1e-3, niters=2000) for k, m in out.items()}


def timed(fn, reps):
    torch.cuda.synchronize()
    t0 = time.perf_counter()
    for i in range(reps):
        fn(i)
    torch.cuda.synchronize()
    return (time.perf_counter() - t0) / reps * 1e3


def spread(v):
    return (max(v) - min(v)) / statistics.median(v)


lines = []
for L, side in ((2, 256), (4, 512)):
    trs = trainers(L, side)
    step = {k: [] for k in trs}
    rnd = {k: [] for k in trs}
    for rep in range(REPS):
        for k, tr in trs.items():
            timed(lambda i: tr.step_hashed(rep * 100 + i), 3)
            step[k].append(timed(lambda i: tr.step_hashed(rep * 100 + 10 + i), 15))
            timed(lambda i: tr.render(), 2)
            rnd[k].append(timed(lambda i: tr.render(), 5))
    for k in trs:
        lines.append(f"{k:13s} {L} x 256, {side * side} rows: step median {statistics.median(step[k]):.3f} ms  min "
                     f"{min(step[k]):.3f}  spread {100 * spread(step[k]):.1f} %  |  render median "
                     f"{statistics.median(rnd[k]):.3f} ms  min {min(rnd[k]):.3f}  spread {100 * spread(rnd[k]):.1f} %")
    rs = statistics.median(step["bspline_cubic"]) / statistics.median(step["bspline_form"])
    rr = statistics.median(rnd["bspline_cubic"]) / statistics.median(rnd["bspline_form"])
    lines.append(f"  cubic / form, {L} x 256, {side * side} rows: step {rs:.4f}  render {rr:.4f}  ({REPS} interleaved blocks of "
                 f"15 steps / 5 renders per net)")
print("\n".join(lines))
if len(sys.argv) > 1:
    with open(sys.argv[1], "w") as f:
        f.write("\n".join(lines) + "\n")
