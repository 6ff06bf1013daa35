#!/usr/bin/env python3
"""Interleaved in-process A/B of the bspline_mscale_2 training step: the HIP net (FusedTrainer, WIRE_KIND_BSPLINE_M2)
against an eager-PyTorch restatement of the same net (written here: closed-form B with torch ops, freq_mlp,
torch.optim.Adam) and against bspline_form 2 x 256 at N rows and at S N rows.  Blocks of timed steps alternate between
them, so clock / temperature drift hits all alike.
    python3 tools/mscale2_ab.py            # configs.py Mscale2_*: 2 hidden x 256, O = 3, 65 536 rows, S = 2 and 3
    python3 tools/mscale2_ab.py --side 128 --scales 0.111 4
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


class EagerM2(nn.Module):
    """The same function in eager PyTorch: the trunk once per scale, the outputs through freq_mlp."""

    def __init__(self, hip, scales):
        super().__init__()
        sd = hip.state_dict()
        self.scales = [float(s) for s in scales]
        self.layers = nn.ModuleList(nn.Linear(2 if l == 0 else K, K) for l in range(HL + 1))
        self.final = nn.Linear(K, 3)
        self.freq = nn.Sequential(nn.Linear(3 * len(scales), 128), nn.ReLU(), nn.Linear(128, 3))
        for l, m in enumerate(self.layers):
            m.load_state_dict({"weight": sd[f"net.{l}.linear.weight"], "bias": sd[f"net.{l}.linear.bias"]})
        self.final.load_state_dict({"weight": sd[f"net.{HL + 1}.weight"], "bias": sd[f"net.{HL + 1}.bias"]})
        self.freq.load_state_dict({k[len("combine_scales.freq_mlp."):]: v for k, v in sd.items()
                                   if k.startswith("combine_scales.freq_mlp.")})

    def forward(self, x):
        outs = []
        for s in self.scales:
            h = x
            for m in self.layers:
                h = bspline(m(h) / s)
            outs.append(self.final(h))
        return self.freq(torch.cat(outs, -1))


def timed(fn, reps):
    torch.cuda.synchronize()
    t0 = time.perf_counter()
    for i in range(reps):
        fn(i)
    torch.cuda.synchronize()
    return (time.perf_counter() - t0) / reps * 1e3


def run(side, scales, blocks):
    n = side * side
    S = len(scales)
    torch.manual_seed(0)
    m2 = models.get_INR("bspline_mscale_2", 2, K, 0, HL, 3, scale=0.0, scale_tensor=torch.tensor(scales)).to(dev)
    eager = EagerM2(m2, scales).to(dev)
    torch.manual_seed(0)
    bs = models.get_INR(nonlin="bspline_form", in_features=2, out_features=3, hidden_features=K, hidden_layers=HL,
                        scale=1 / 9).to(dev)
    torch.manual_seed(0)
    bsS = models.get_INR(nonlin="bspline_form", in_features=2, out_features=3, hidden_features=K, hidden_layers=HL,
                         scale=1 / 9).to(dev)
    target = torch.rand(n, 3)
    # bspline_form at S N rows: a grid S times as tall
    trs = {f"mscale_2 hip S={S}": FusedTrainer(m2, (side, side), target, lr=1e-3, niters=2000),
           "bspline_form N": FusedTrainer(bs, (side, side), target, lr=1e-3, niters=2000),
           f"bspline_form {S}N": FusedTrainer(bsS, (S * side, side), target.repeat(S, 1), lr=1e-3, niters=2000)}
    opt = torch.optim.Adam(eager.parameters(), lr=1e-3)
    x = torch.rand(n, 2, device=dev) * 2 - 1
    t = target.to(dev)

    def eager_step(i):
        opt.zero_grad()
        ((eager(x) - t) ** 2).mean().backward()
        opt.step()

    steps = {k: (lambda tr_: lambda i: tr_.step_hashed(i))(v) for k, v in trs.items()}
    steps[f"mscale_2 eager S={S}"] = eager_step
    res = {k: [] for k in steps}
    for _ in range(blocks):
        for k, fn in steps.items():
            timed(fn, 3)
            res[k].append(timed(fn, 15))
    for k, v in res.items():
        print(f"{k:22s} {n} rows: step mean {sum(v) / len(v):.3f} ms  min {min(v):.3f} ms", flush=True)
    hip, eag = min(res[f"mscale_2 hip S={S}"]), min(res[f"mscale_2 eager S={S}"])
    print(f"S={S}: eager / hip (min) {eag / hip:.2f} x; hip / bspline_form N {hip / min(res['bspline_form N']):.2f}; "
          f"hip / bspline_form {S}N {hip / min(res[f'bspline_form {S}N']):.2f}", flush=True)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--side", type=int, default=256)
    ap.add_argument("--scales", type=float, nargs="*", default=None)
    ap.add_argument("--blocks", type=int, default=6)
    a = ap.parse_args()
    for st in ([a.scales] if a.scales else [[1 / 9, 4.0], [1 / 9, 4.0, 8.0]]):
        run(a.side, st, a.blocks)


if __name__ == "__main__":
    main()
