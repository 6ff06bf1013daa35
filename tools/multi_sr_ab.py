#!/usr/bin/env python3
"""Interleaved in-process A/B of the multi-image super-resolution training step at the driver's shape
(wire_multi_sr.py: 4 frames of 768 x 512, scale 4, 3 outputs, 2 hidden x 256): FusedTrainer.step_frames against the same
loop written here in eager PyTorch through the drop-in modules -- model(coords), torch.nn.AvgPool2d, torch.nn.MSELoss,
torch.optim.Adam -- and the per-batch host-to-device upload of the frames' coordinates against
FusedTrainer.affine_coords, which replaces it.  Blocks of timed steps alternate between the variants, so clock /
temperature drift hits all alike.  A measurement, not a gate: it prints what it finds.
    python3 tools/multi_sr_ab.py                          # wire and siren
    python3 tools/multi_sr_ab.py --nets wire --blocks 3
    python3 tools/multi_sr_ab.py --frames 2 --height 96 --width 64      # a small shape
"""
import argparse
import os
import sys
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
import numpy as np
import torch

from wire_amd.modules import models, motion
from wire_amd.trainer import FusedTrainer

dev = torch.device("cuda:0")
K, HL, O = 256, 2, 3
LR = {"wire": 5e-3, "siren": 1e-3}                    # wire_multi_sr.py:117-124


def timed(fn, reps):
    torch.cuda.synchronize()
    t0 = time.perf_counter()
    for _ in range(reps):
        fn()
    torch.cuda.synchronize()
    return (time.perf_counter() - t0) / reps * 1e3


def build(nonlin):
    torch.manual_seed(0)
    return models.get_INR(nonlin=nonlin, in_features=2, out_features=O, hidden_features=K, hidden_layers=HL,
                          first_omega_0=10.0, hidden_omega_0=10.0, scale=5.0).to(dev)     # wire_multi_sr.py:51-52


def run(nonlin, B, H, W, scale, blocks, reps):
    H2, W2 = H // scale, W // scale
    rng = np.random.default_rng(0)
    thetas = (2 * rng.random(B) - 1) * np.pi / 10
    shifts = rng.integers(-5 * scale, 5 * scale, size=(B, 2))
    thetas[0], shifts[0] = 0.0, 0
    mats = np.stack([motion.getEuclidianMatrix(t, s) for t, s in zip(thetas, shifts)])
    gt = torch.rand(B, H2 * W2, O, device=dev)
    mask = (torch.rand(B, H2 * W2, O, device=dev) > 0.1).float()

    tr = FusedTrainer(build(nonlin), (H, W), None, lr=LR[nonlin], niters=2000)
    coords = tr.affine_coords(mats)
    host = coords.cpu().pin_memory()                    # what the reference's DataLoader(pin_memory=True) hands over

    eager = build(nonlin)
    opt = torch.optim.Adam(lr=LR[nonlin], params=eager.parameters())
    pool, crit = torch.nn.AvgPool2d(scale), torch.nn.MSELoss()

    def hip_step():
        tr.step_frames(coords, gt, scale, mask=mask)

    def eager_step():
        out_hr = eager(coords).reshape(-1, H, W, O).permute(0, 3, 1, 2)
        out = pool(out_hr).permute(0, 2, 3, 1).reshape(-1, H2 * W2, O)
        loss = crit(out * mask, gt * mask)
        opt.zero_grad()
        loss.backward()
        opt.step()

    variants = {"step_frames": hip_step, "eager modules": eager_step,
                "coords H2D upload": lambda: host.to(dev, non_blocking=True),
                "affine_coords": lambda: tr.affine_coords(mats)}
    res = {k: [] for k in variants}
    for _ in range(blocks):
        for k, fn in variants.items():
            timed(fn, 2)
            res[k].append(timed(fn, reps))
    tag = f"{nonlin} {HL}x{K}, {B} x {H} x {W}, scale {scale}"
    for k, v in res.items():
        print(f"{tag}: {k:18s} mean {sum(v) / len(v):9.3f} ms  min {min(v):9.3f} ms", flush=True)
    print(f"{tag}: eager / step_frames (min) {min(res['eager modules']) / min(res['step_frames']):.2f} x; "
          f"upload / affine_coords (min) {min(res['coords H2D upload']) / min(res['affine_coords']):.2f} x; "
          f"upload as a share of a step_frames step {min(res['coords H2D upload']) / min(res['step_frames']):.1%}",
          flush=True)
    del tr, eager, opt
    torch.cuda.empty_cache()


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--nets", nargs="*", default=["wire", "siren"], choices=sorted(LR))
    ap.add_argument("--frames", type=int, default=4)
    ap.add_argument("--height", type=int, default=768)
    ap.add_argument("--width", type=int, default=512)
    ap.add_argument("--scale", type=int, default=4)
    ap.add_argument("--blocks", type=int, default=4)
    ap.add_argument("--reps", type=int, default=5)
    a = ap.parse_args()
    for nonlin in a.nets:
        run(nonlin, a.frames, a.height, a.width, a.scale, a.blocks, a.reps)


if __name__ == "__main__":
    main()
