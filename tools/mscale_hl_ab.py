#!/usr/bin/env python3
"""Interleaved in-process A/B of the bspline_mscale_HL training step: the HIP net (FusedTrainer, WIRE_KIND_BSPLINE_MS)
against an eager-PyTorch restatement of the same net (written here: closed-form B with torch ops, torch.optim.Adam) and
against bspline_form 2 x 256 at the same rows.  Blocks of timed steps alternate between the three, so clock /
temperature drift hits all alike.
    python3 tools/mscale_hl_ab.py         # configs.py MscaleHL_s1o9_ST4_3_SHF384_LR8e3_E4000: SHF 384 in [1/9, 1/9, 4],
                                          # 2 hidden x 256, scale 1/9, a 256 x 256 grid (65 536 rows per step)"""
import os
import sys
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
import torch
from torch import nn

from wire_amd.modules import models
from wire_amd.trainer import FusedTrainer

dev = torch.device("cuda:0")
SIDE, K, SHF, HL, S, ST = 256, 256, 384, 2, 1 / 9, [1 / 9, 1 / 9, 4.0]


def bspline(r):
    a = r.abs()
    return torch.where(a <= 0.5, 0.75 - r * r, 0.5 * torch.clamp(1.5 - a, min=0.0) ** 2)


class EagerMS(nn.Module):
    """The same function in eager PyTorch: frozen first stage under no_grad, then Linear + B per layer."""

    def __init__(self, hip):
        super().__init__()
        sd = hip.state_dict()
        self.register_buffer("W0", sd["net.0.linear.weight"].clone())
        self.register_buffer("b0", sd["net.0.linear.bias"].clone())
        g = [0] * 256 + [1 + (j - 256) // ((SHF - 256) // (len(ST) - 1)) for j in range(256, SHF)]
        self.register_buffer("c0", 1.0 / torch.tensor(ST, device=sd["net.0.scale_0"].device).abs()[torch.tensor(g)])
        self.layers = nn.ModuleList(nn.Linear(SHF if l == 0 else K, K) for l in range(HL))
        self.final = nn.Linear(K, 3)
        for l, m in enumerate(self.layers):
            m.load_state_dict({"weight": sd[f"net.{l + 1}.linear.weight"], "bias": sd[f"net.{l + 1}.linear.bias"]})
        self.final.load_state_dict({"weight": sd[f"net.{HL + 1}.weight"], "bias": sd[f"net.{HL + 1}.bias"]})

    def forward(self, x):
        with torch.no_grad():
            h = bspline(torch.addmm(self.b0, x, self.W0.t()) * self.c0)
        for m in self.layers:
            h = bspline(m(h) / S)
        return self.final(h)


def main():
    torch.manual_seed(0)
    ms = models.get_INR("bspline_mscale_HL", 2, K, SHF, HL, 3, scale=S, scale_tensor=torch.tensor(ST)).to(dev)
    eager = EagerMS(ms).to(dev)
    torch.manual_seed(0)
    bs = models.get_INR(nonlin="bspline_form", in_features=2, out_features=3, hidden_features=K, hidden_layers=HL,
                        scale=S).to(dev)
    n = SIDE * SIDE
    target = torch.rand(n, 3)
    tr = {"mscale_HL hip": FusedTrainer(ms, (SIDE, SIDE), target, lr=1e-3, niters=2000),
          "bspline_form 2x256": FusedTrainer(bs, (SIDE, SIDE), target, lr=1e-3, niters=2000)}
    opt = torch.optim.Adam(eager.parameters(), lr=1e-3)
    x = torch.rand(n, 2, device=dev) * 2 - 1
    t = target.to(dev)

    def eager_step(i):
        opt.zero_grad()
        ((eager(x) - t) ** 2).mean().backward()
        opt.step()

    steps = {k: (lambda tr_: lambda i: tr_.step_hashed(i))(v) for k, v in tr.items()}
    steps["mscale_HL eager"] = eager_step

    def timed(fn, reps):
        torch.cuda.synchronize()
        t0 = time.perf_counter()
        for i in range(reps):
            fn(i)
        torch.cuda.synchronize()
        return (time.perf_counter() - t0) / reps * 1e3

    res = {k: [] for k in steps}
    for rep in range(6):
        for k, fn in steps.items():
            timed(fn, 3)
            res[k].append(timed(fn, 15))
    for k, v in res.items():
        print(f"{k:20s} {n} rows: step mean {sum(v) / len(v):.3f} ms  min {min(v):.3f} ms")
    hip, eag = min(res["mscale_HL hip"]), min(res["mscale_HL eager"])
    print(f"eager / hip (min): {eag / hip:.2f} x")


if __name__ == "__main__":
    main()
