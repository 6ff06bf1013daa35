#!/usr/bin/env python3
"""Interleaved in-process A/B of the multi-image super-resolution step with a learnable registration at the driver's
shape (wire_multi_sr.py: 4 frames of 768 x 512, scale 4, 3 outputs, 2 hidden x 256): FusedTrainer.step_frames_registered
against FusedTrainer.step_frames on the same frames, and the two warp kernels alone (wire_warp_coords_fwd,
wire_warp_coords_bwd without and with g_in).  What the registered step adds to step_frames is the two warp launches, the
coordinate-gradient part of wire_mlp_bwd_coords and a six-numbers-per-frame Adam launch.  Blocks of timed steps
alternate between the variants, so clock / temperature drift hits all alike.  A measurement, not a gate: it prints
what it finds.
    python3 tools/multi_sr_reg_ab.py                          # wire and siren
    python3 tools/multi_sr_reg_ab.py --nets wire --blocks 3
    python3 tools/multi_sr_reg_ab.py --frames 2 --height 96 --width 64      # a small shape
"""
import argparse
import os
import sys
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
import numpy as np
import torch

from wire_amd import _lib
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

    # two trainers from the same initial weights, so neither variant trains the other's net
    tr = FusedTrainer(build(nonlin), (H, W), None, lr=LR[nonlin], niters=2000)
    trr = FusedTrainer(build(nonlin), (H, W), None, lr=LR[nonlin], niters=2000)
    coords = tr.affine_coords(mats)
    reg = trr.registration(B, lr=1e-4)

    L = _lib.lib()
    n_per = H * W
    theta = reg.theta.clone()
    g_out = 1e-3 * torch.randn(B, n_per, 2, device=dev)
    out, g_in, g_theta = torch.empty_like(coords), torch.empty_like(coords), torch.empty_like(theta)
    ws = torch.empty(L.wire_warp_coords_bwd_ws_bytes(B, n_per), dtype=torch.uint8, device=dev)

    def warp_fwd():
        _lib.check(L.wire_warp_coords_fwd(torch.cuda.current_stream().cuda_stream, coords.data_ptr(), theta.data_ptr(),
                                          B, n_per, out.data_ptr()), "warp_coords_fwd")

    def warp_bwd(gi):
        _lib.check(L.wire_warp_coords_bwd(torch.cuda.current_stream().cuda_stream, coords.data_ptr(), theta.data_ptr(),
                                          g_out.data_ptr(), B, n_per, 1, g_theta.data_ptr(), gi, ws.data_ptr(),
                                          ws.numel()), "warp_coords_bwd")

    variants = {"step_frames": lambda: tr.step_frames(coords, gt, scale, mask=mask),
                "step_frames_registered": lambda: trr.step_frames_registered(reg, coords, gt, scale, mask=mask),
                "warp fwd": warp_fwd,
                "warp bwd (theta)": lambda: warp_bwd(None),
                "warp bwd (+ g_in)": lambda: warp_bwd(g_in.data_ptr())}
    res = {k: [] for k in variants}
    for _ in range(blocks):
        for k, fn in variants.items():
            timed(fn, 2)
            res[k].append(timed(fn, reps))
    tag = f"{nonlin} {HL}x{K}, {B} x {H} x {W}, scale {scale}"
    for k, v in res.items():
        print(f"{tag}: {k:24s} mean {sum(v) / len(v):9.3f} ms  min {min(v):9.3f} ms", flush=True)
    a, b = min(res["step_frames"]), min(res["step_frames_registered"])
    kernels = min(res["warp fwd"]) + min(res["warp bwd (theta)"])
    print(f"{tag}: registered / step_frames (min) {b / a:.3f} x, +{b - a:.3f} ms per step, of which the two warp kernels "
          f"alone {kernels:.3f} ms (timed back to back, launch overhead included)", flush=True)
    del tr, trr
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
