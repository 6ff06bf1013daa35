#!/usr/bin/env python3
"""Interleaved in-process A/B of the multiplicative filter network: the HIP net (FusedTrainer step and no_grad render,
WIRE_KIND_MFN) against (a) the same arithmetic in eager PyTorch on the same GPU (written out here: the Gabor filters of
modules/mfn.py with torch ops, torch.optim.Adam) and (b) a siren of the same shape through the same FusedTrainer.  Blocks
of timed steps alternate between the three, so clock / temperature drift hits all alike.
    python3 tools/mfn_ab.py                     # 2 x 256 on 65 536 rows, 4 x 256 on 262 144 rows, 512 x 512 render
    python3 tools/mfn_ab.py --steps 20 --hip-only --layers 2 --rows 65536     # HIP steps only (for a kernel trace)
"""
import argparse
import os
import sys
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
import torch
from torch import nn

from wire_amd.modules import mfn, models
from wire_amd.trainer import FusedTrainer

dev = torch.device("cuda:0")
K = 256


class EagerMfn(nn.Module):
    """The same function in eager PyTorch (the reference's arithmetic, expanded norm included)."""

    def __init__(self, hip):
        super().__init__()
        self.k = hip.k
        self.p = nn.ParameterList([nn.Parameter(t.detach().clone()) for t in hip.param_tensors()])

    def filt(self, i, x):
        mu, gamma, w, c = self.p[4 * i:4 * i + 4]
        norm = (x ** 2).sum(1).unsqueeze(-1) + (mu ** 2).sum(1).unsqueeze(0) - 2 * x @ mu.T
        return torch.exp(-gamma.unsqueeze(0) / 2. * norm) * torch.sin(x @ w.T + c)

    def forward(self, x):
        z = self.filt(0, x)
        for i in range(self.k - 1):
            W, b = self.p[4 * self.k + 2 * i], self.p[4 * self.k + 2 * i + 1]
            z = (z @ W.T + b) * self.filt(i + 1, x)
        return z @ self.p[-2].T + self.p[-1]


def grid(side_h, side_w):
    X, Y = torch.meshgrid(torch.linspace(-1, 1, side_w), torch.linspace(-1, 1, side_h), indexing="xy")
    return torch.hstack((X.reshape(-1, 1), Y.reshape(-1, 1))).to(dev)


def timed(fn, reps):
    torch.cuda.synchronize()
    t0 = time.perf_counter()
    for _ in range(reps):
        fn()
    torch.cuda.synchronize()
    return (time.perf_counter() - t0) / reps * 1e3


def run(L, rows, steps, blocks, hip_only):
    H = 256
    W = rows // H
    torch.manual_seed(0)
    target = torch.rand(rows, 3)
    hip = mfn.INR(2, K, L, 3).to(dev)
    eager = EagerMfn(hip).to(dev)
    tr = FusedTrainer(hip, (H, W), target, lr=1e-4, niters=10 ** 6)
    idx = torch.arange(rows, dtype=torch.int64, device=dev)
    fns = {"mfn-HIP step": lambda: tr.step(idx)}
    if not hip_only:
        x, t = grid(H, W), target.to(dev)
        opt = torch.optim.Adam(eager.parameters(), lr=1e-4)

        def eager_step():
            opt.zero_grad(set_to_none=True)
            ((eager(x) - t) ** 2).mean().backward()
            opt.step()
        sir = models.get_INR(nonlin="siren", in_features=2, out_features=3, hidden_features=K, hidden_layers=L,
                             first_omega_0=30.0, hidden_omega_0=30.0).to(dev)
        ts = FusedTrainer(sir, (H, W), target, lr=1e-4, niters=10 ** 6)
        fns["eager-PyTorch step"] = eager_step
        fns["siren-HIP step"] = lambda: ts.step(idx)
    for fn in fns.values():                      # warm-up
        for _ in range(5):
            fn()
    res = {k: [] for k in fns}
    for _ in range(blocks):
        for k, fn in fns.items():
            res[k].append(timed(fn, steps))
    for k, v in res.items():
        v.sort()
        print(f"{L} x {K}, {rows} rows  {k:20s} median {v[len(v) // 2]:8.3f} ms  min {v[0]:8.3f}  max {v[-1]:8.3f}  "
              f"({blocks} blocks of {steps})", flush=True)


def render(L, side, steps, blocks):
    torch.manual_seed(0)
    hip = mfn.INR(2, K, L, 3).to(dev)
    eager = EagerMfn(hip).to(dev)
    sir = models.get_INR(nonlin="siren", in_features=2, out_features=3, hidden_features=K, hidden_layers=L,
                         first_omega_0=30.0, hidden_omega_0=30.0).to(dev)
    x = grid(side, side)
    fns = {"mfn-HIP render": lambda: hip(x[None]), "eager-PyTorch render": lambda: eager(x),
           "siren-HIP render": lambda: sir(x)}
    with torch.no_grad():
        for fn in fns.values():
            for _ in range(5):
                fn()
        res = {k: [] for k in fns}
        for _ in range(blocks):
            for k, fn in fns.items():
                res[k].append(timed(fn, steps))
    for k, v in res.items():
        v.sort()
        print(f"{L} x {K}, {side} x {side} render  {k:20s} median {v[len(v) // 2]:8.3f} ms  min {v[0]:8.3f}  max {v[-1]:8.3f}",
              flush=True)


if __name__ == "__main__":
    ap = argparse.ArgumentParser()
    ap.add_argument("--steps", type=int, default=10)
    ap.add_argument("--blocks", type=int, default=7)
    ap.add_argument("--layers", type=int, default=0)
    ap.add_argument("--rows", type=int, default=0)
    ap.add_argument("--hip-only", action="store_true")
    a = ap.parse_args()
    if a.layers or a.rows:
        run(a.layers or 2, a.rows or 65536, a.steps, 1 if a.hip_only else a.blocks, a.hip_only)
    else:
        run(2, 65536, a.steps, a.blocks, False)
        run(4, 262144, a.steps, a.blocks, False)
        render(2, 512, a.steps, a.blocks)
