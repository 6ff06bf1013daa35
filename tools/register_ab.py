#!/usr/bin/env python3
"""Interleaved in-process A/B of the device registration (wire_register.hip) against the same iteration written with
torch device ops -- what a user of this library had before: F.grid_sample of (R, Rx, Ry), einsum for the normal
equations, torch.linalg.solve -- at the driver's shape (wire_multi_sr.py: 4 frames of 768 x 512 at full resolution,
192 x 128 at scale 4):
  * one Gauss-Newton iteration: wire_register_gn_step against torch_gn_step (fp32 and fp64), 3 frames onto frame 0;
  * a whole registration: motion.register_stack_ecc (3 levels, 30 iterations) against the same loop on torch_gn_step.
The torch iteration samples central-difference gradient images where the kernel differentiates the interpolant, so the
two agree to the method's discretisation floor, not to rounding; the displacement between their results is printed.
All times are HOST-CLOCK times around a device synchronise, launch overhead included: blocks of timed calls alternate
between the variants, so clock / temperature drift hits all alike.  A measurement, not a gate: it prints what it finds.
    python3 tools/register_ab.py
    python3 tools/register_ab.py --shapes 192x128 --blocks 3
"""
import argparse
import os
import sys
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tests"))
import numpy as np
import torch
import torch.nn.functional as F

from wire_amd import functional
from wire_amd.modules import motion
import register_ref as ref

dev = torch.device("cuda:0")


def timed(fn, reps):
    torch.cuda.synchronize()
    t0 = time.perf_counter()
    for _ in range(reps):
        fn()
    torch.cuda.synchronize()
    return (time.perf_counter() - t0) / reps * 1e3


def torch_gn_step(R3, frames, mats, grid, damping):
    """One Euclidean Gauss-Newton iteration in torch ops.  R3: [1, 3, H, W] = (R, Rx, Ry); frames [B, H, W]; mats
    [B, 2, 3]; grid [H*W, 3] = (j, i, 1); all of one dtype.  Returns the updated matrices (no validity handling)."""
    B, H, W = frames.shape
    uv = torch.einsum("bac,pc->bpa", mats, grid)
    ok = (uv[..., 0] >= 0) & (uv[..., 0] <= W - 1) & (uv[..., 1] >= 0) & (uv[..., 1] <= H - 1)
    gn = torch.stack(((2 * uv[..., 0] + 1) / W - 1, (2 * uv[..., 1] + 1) / H - 1), dim=-1)
    s = F.grid_sample(R3.expand(B, -1, -1, -1), gn[:, None], mode="bilinear", padding_mode="zeros", align_corners=False)
    s = s[:, :, 0]                                                        # [B, 3, n]
    f = frames.reshape(B, -1)
    w = (ok & (f != 0)).to(f.dtype)
    res = s[:, 0] - f
    J = torch.stack((s[:, 1] * grid[:, 0], s[:, 1] * grid[:, 1], s[:, 1], s[:, 2] * grid[:, 0], s[:, 2] * grid[:, 1],
                     s[:, 2]), dim=-1)                                    # [B, n, 6]
    Jw = J * w[..., None]
    Hm = torch.einsum("bpa,bpc->bac", Jw, J)
    g = torch.einsum("bpa,bp->ba", Jw, res)
    th = torch.atan2(mats[:, 1, 0], mats[:, 0, 0])
    c, sn, z, one = torch.cos(th), torch.sin(th), torch.zeros_like(th), torch.ones_like(th)
    P = torch.stack((torch.stack((-sn, -c, z, c, -sn, z), dim=-1), torch.stack((z, z, one, z, z, z), dim=-1),
                     torch.stack((z, z, z, z, z, one), dim=-1)), dim=-1)  # [B, 6, 3]
    A = P.transpose(1, 2) @ Hm @ P
    A = A + damping * torch.diag_embed(torch.diagonal(A, dim1=1, dim2=2))
    d = torch.linalg.solve(A, -(P.transpose(1, 2) @ g[..., None]))[..., 0]
    tn = th + d[:, 0]
    c, sn = torch.cos(tn), torch.sin(tn)
    return torch.stack((torch.stack((c, -sn, mats[:, 0, 2] + d[:, 1]), dim=-1),
                        torch.stack((sn, c, mats[:, 1, 2] + d[:, 2]), dim=-1)), dim=1)


def gradient_image(r):
    """(R, Rx, Ry) [1, 3, H, W] with central differences (one-sided at the border)."""
    rx, ry = torch.gradient(r, dim=1)[0], torch.gradient(r, dim=0)[0]
    return torch.stack((r, rx, ry))[None].contiguous()


def pixel_grid(H, W, dtype):
    return torch.from_numpy(motion._pixel_grid(H, W)).to(dev, dtype)


def torch_register(stack, levels, iters, dtype, damping):
    """motion.register_stack_ecc's loop (one start, Euclidean) on torch_gn_step: matrices at the frames' resolution."""
    x = stack.to(dtype)
    pyr = [(x[0], x[1:])]
    for _ in range(levels - 1):
        r, f = pyr[-1]
        pyr.append((F.avg_pool2d(r[None, None], 2)[0, 0], F.avg_pool2d(f[:, None], 2)[:, 0]))
    B = x.shape[0] - 1
    mats = torch.tensor([[1.0, 0, 0], [0, 1.0, 0]], dtype=dtype, device=dev).repeat(B, 1, 1)
    for lvl, (r, f) in enumerate(pyr[::-1]):
        if lvl:
            mats = motion.rescale_mats(mats, 2.0)
        R3, grid = gradient_image(r), pixel_grid(*r.shape, dtype)
        for _ in range(iters):
            mats = torch_gn_step(R3, f, mats, grid, damping)
    return mats


def run(H, W, pool, blocks, reps, levels, iters):
    truth = ref.host_motions(4, 5, 5 * pool, np.pi / 30)
    stack_np = ref.synth_stack(H * pool, W * pool, truth, pool)
    stack = torch.tensor(stack_np, device=dev)
    r, f = stack[0].contiguous(), stack[1:].contiguous()
    B = f.shape[0]
    start = torch.tensor(ref.rescale_mats(truth[1:], 1 / pool) + [[0, 0, 0.3], [0, 0, -0.2]], device=dev)[:, None].contiguous()
    ws = functional._workspace("wire_register_gn_ws_bytes", dev, B, 1, H, W)
    tag = f"{B} + 1 frames of {H} x {W}"

    variants = {}
    mats = start.clone()
    variants["wire_register_gn_step"] = lambda: functional.register_gn_step(r, f, mats, None, "euclidean", 1e-6, 0.25, ws)
    for dtype, name in ((torch.float32, "torch ops, fp32"), (torch.float64, "torch ops, fp64")):
        R3, grid, ft, m0 = gradient_image(r.to(dtype)), pixel_grid(H, W, dtype), f.to(dtype), start[:, 0].to(dtype)
        variants[name] = (lambda R3=R3, ft=ft, m0=m0, grid=grid: torch_gn_step(R3, ft, m0, grid, 1e-6))
    res = {k: [] for k in variants}
    for _ in range(blocks):
        for k, fn in variants.items():
            mats.copy_(start)
            timed(fn, 3)
            mats.copy_(start)
            res[k].append(timed(fn, reps))
    for k, v in res.items():
        print(f"{tag}: one iteration, {k:24s} host clock mean {sum(v) / len(v) * 1e3:9.1f} us  min {min(v) * 1e3:9.1f} us",
              flush=True)

    whole = {"motion.register_stack_ecc": lambda: motion.register_stack_ecc(stack, (H * pool, W * pool), "euclidean",
                                                                            levels, iters),
             "torch ops, fp32": lambda: torch_register(stack, levels, iters, torch.float32, 1e-6),
             "torch ops, fp64": lambda: torch_register(stack, levels, iters, torch.float64, 1e-6)}
    res = {k: [] for k in whole}
    for _ in range(blocks):
        for k, fn in whole.items():
            timed(fn, 1)
            res[k].append(timed(fn, 2))
    for k, v in res.items():
        print(f"{tag}: whole registration ({levels} levels x {iters} iterations), {k:26s} host clock mean "
              f"{sum(v) / len(v):9.2f} ms  min {min(v):9.2f} ms", flush=True)
    ecc = motion.register_stack_ecc(stack, (H * pool, W * pool), "euclidean", levels, iters)[3]
    for dtype in (torch.float32, torch.float64):
        low = torch_register(stack, levels, iters, dtype, 1e-6).double().cpu().numpy()
        tm = np.concatenate((ecc[:1], ref.rescale_mats(low, float(pool))))
        print(f"{tag}: corner error against the truth at {H * pool} x {W * pool}: device "
              f"{ref.corner_error(ecc, truth, H * pool, W * pool).max():.4f} px, torch ops {str(dtype)[6:]} "
              f"{ref.corner_error(tm, truth, H * pool, W * pool).max():.4f} px", flush=True)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--shapes", nargs="*", default=["192x128", "768x512"])
    ap.add_argument("--blocks", type=int, default=4)
    ap.add_argument("--reps", type=int, default=20)
    ap.add_argument("--levels", type=int, default=3)
    ap.add_argument("--iters", type=int, default=30)
    a = ap.parse_args()
    print(torch.cuda.get_device_name(0), flush=True)
    for s in a.shapes:
        H, W = (int(v) for v in s.split("x"))
        # the 768 x 512 frames are the synthetic image itself; the 192 x 128 ones are it pooled by 4
        run(H, W, 4 if H <= 192 else 1, a.blocks, a.reps, a.levels, a.iters)


if __name__ == "__main__":
    main()
