#!/usr/bin/env python3
"""Interleaved in-process A/B of the bspline_form training step (and the forward-only render) against gauss at the same
shape: blocks of timed steps alternate between the two nets, so clock / temperature drift hits both alike.
    python3 tools/bspline_ab.py            # 4 x 256 on a 512 x 512 grid (262 144 rows per step) and the config shape
                                           # 2 x 256 on 256 x 256 (65 536 rows, configs.py Bspline_s9_LR1e3_E2000)"""
import os
import sys
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
import torch

from wire_amd.modules import models
from wire_amd.trainer import FusedTrainer

dev = torch.device("cuda:0")
NETS = {"bspline_form": dict(scale=1 / 9), "gauss": dict(scale=10.0)}


def trainers(L, side):
    out = {}
    for nonlin, kw in NETS.items():
        torch.manual_seed(0)
        model = models.get_INR(nonlin=nonlin, in_features=2, out_features=3, hidden_features=256, hidden_layers=L,
                               **kw).to(dev)
        out[nonlin] = FusedTrainer(model, (side, side), torch.rand(side * side, 3), lr=1e-3, niters=2000)
    return out


def timed(fn, reps):
    torch.cuda.synchronize()
    t0 = time.perf_counter()
    for i in range(reps):
        fn(i)
    torch.cuda.synchronize()
    return (time.perf_counter() - t0) / reps * 1e3


for L, side in ((4, 512), (2, 256)):
    trs = trainers(L, side)
    step = {k: [] for k in trs}
    rnd = {k: [] for k in trs}
    for rep in range(6):
        for k, tr in trs.items():
            timed(lambda i: tr.step_hashed(rep * 100 + i), 3)
            step[k].append(timed(lambda i: tr.step_hashed(rep * 100 + 10 + i), 15))
            timed(lambda i: tr.render(), 2)
            rnd[k].append(timed(lambda i: tr.render(), 5))
    for k in trs:
        print(f"{k:13s} {L} x 256, {side * side} rows: step mean {sum(step[k]) / len(step[k]):.3f} ms  "
              f"min {min(step[k]):.3f} ms  |  render mean {sum(rnd[k]) / len(rnd[k]):.3f} ms  min {min(rnd[k]):.3f} ms")
