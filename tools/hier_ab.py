#!/usr/bin/env python3
"""Interleaved in-process A/B of the bspline_mscale_hier training step: the HIP net (FusedTrainer,
WIRE_KIND_BSPLINE_HIER) against an eager-PyTorch restatement of the same net (written here: closed-form B with torch
ops, one stage per scale joined by torch.cat, a head per stage, torch.optim.Adam over stages and heads) and against
bspline_form 2 x 256 at the same rows.  Blocks of timed steps alternate between them, so clock / temperature drift hits
all alike.
    python3 tools/hier_ab.py            # configs.py MscaleHier_*: 2 hidden x 256, O = 3, 65 536 rows, S = 2 and 3
    python3 tools/hier_ab.py --side 128 --scales 0.111 4
    python3 tools/hier_ab.py --steps 20 --scales 0.111 4   # 20 HIP steps only (for a kernel trace)
"""
import argparse
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
K, HL = 256, 2


def bspline(r):
    a = r.abs()
    return torch.where(a <= 0.5, 0.75 - r * r, 0.5 * torch.clamp(1.5 - a, min=0.0) ** 2)


class EagerHier(nn.Module):
    """The same function in eager PyTorch."""

    def __init__(self, hip, scales):
        super().__init__()
        sd = hip.state_dict()
        self.scales = [float(s) for s in scales]
        self.stages = nn.ModuleList()
        self.heads = nn.ModuleList()
        for s in range(len(scales)):
            widths = [(2, K), (K if s == 0 else 2 * K, K)] + [(K, K)] * (HL - 1)
            stage = nn.ModuleList(nn.Linear(i, o) for i, o in widths)
            for l, m in enumerate(stage):
                m.load_state_dict({"weight": sd[f"stages.{s}.{l}.linear.weight"], "bias": sd[f"stages.{s}.{l}.linear.bias"]})
            self.stages.append(stage)
            head = nn.Linear(K, 3)
            head.load_state_dict(hip.linears[s].state_dict())
            self.heads.append(head)

    def forward(self, x):
        y, prev = 0, None
        for s, (stage, head) in enumerate(zip(self.stages, self.heads)):
            sig = self.scales[s]
            h = x
            for l, m in enumerate(stage):
                if s > 0 and l == 1:
                    h = torch.cat((h, prev), -1)
                h = bspline(m(h) / sig)
            prev = h
            y = y + head(h)
        return y


def timed(fn, reps):
    torch.cuda.synchronize()
    t0 = time.perf_counter()
    for i in range(reps):
        fn(i)
    torch.cuda.synchronize()
    return (time.perf_counter() - t0) / reps * 1e3


def run(side, scales, blocks, steps_only):
    n = side * side
    S = len(scales)
    torch.manual_seed(0)
    hier = models.get_INR("bspline_mscale_hier", 2, K, 0, HL, 3, scale=0.0, scale_tensor=scales).to(dev)
    target = torch.rand(n, 3)
    tr = FusedTrainer(hier, (side, side), target, lr=[1e-3] * S, niters=2000)
    if steps_only:
        for i in range(steps_only):
            tr.step_hashed(i)
        torch.cuda.synchronize()
        return
    eager = EagerHier(hier, scales).to(dev)
    torch.manual_seed(0)
    bs = models.get_INR(nonlin="bspline_form", in_features=2, out_features=3, hidden_features=K, hidden_layers=HL,
                        scale=1 / 9).to(dev)
    trs = {f"hier hip S={S}": tr, "bspline_form": FusedTrainer(bs, (side, side), target, lr=1e-3, niters=2000)}
    opt = torch.optim.Adam(eager.parameters(), lr=1e-3)
    x = torch.rand(n, 2, device=dev) * 2 - 1
    t = target.to(dev)

    def eager_step(i):
        opt.zero_grad()
        ((eager(x) - t) ** 2).mean().backward()
        opt.step()

    steps = {k: (lambda tr_: lambda i: tr_.step_hashed(i))(v) for k, v in trs.items()}
    steps[f"hier eager S={S}"] = eager_step
    res = {k: [] for k in steps}
    for _ in range(blocks):
        for k, fn in steps.items():
            timed(fn, 3)
            res[k].append(timed(fn, 15))
    for k, v in res.items():
        print(f"{k:18s} {n} rows: step mean {sum(v) / len(v):.3f} ms  min {min(v):.3f} ms", flush=True)
    hip, eag = min(res[f"hier hip S={S}"]), min(res[f"hier eager S={S}"])
    print(f"S={S}: eager / hip (min) {eag / hip:.2f} x; hip / bspline_form {hip / min(res['bspline_form']):.2f}", flush=True)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--side", type=int, default=256)
    ap.add_argument("--scales", type=float, nargs="*", default=None)
    ap.add_argument("--blocks", type=int, default=6)
    ap.add_argument("--steps", type=int, default=0)
    a = ap.parse_args()
    for st in ([a.scales] if a.scales else [[1 / 9, 4.0], [1 / 8, 1 / 2, 4.0]]):
        run(a.side, st, a.blocks, a.steps)


if __name__ == "__main__":
    main()
