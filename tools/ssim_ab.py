#!/usr/bin/env python3
"""Interleaved in-process A/B of the SSIM metric at the super-resolution drivers' image sizes (512 x 512 x 3 and
768 x 512 x 3, both windows): wire_ssim (functional.ssim on the channel-last render as it is) against the same arithmetic
written in PyTorch the way pytorch_msssim does it -- a permute of the channel-last images to NCHW, then ten grouped
conv2d calls (two separable passes of five moments) and the pointwise expression.  Blocks of timed calls alternate
between the variants, so clock / temperature drift hits both alike; every timed window ends in a device synchronise.
A measurement, not a gate: it prints what it finds (and the two results, which must agree).
    python3 tools/ssim_ab.py > profiles/ssim_ab.txt
    python3 tools/ssim_ab.py --sizes 96x64 --blocks 2 --reps 20       # a small shape
"""
import argparse
import os
import sys
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
import torch
import torch.nn.functional as F

from wire_amd import functional

dev = torch.device("cuda:0")
O = 3
DATA_RANGE = {"gaussian": 1.0, "uniform": 2.0}


def timed(fn, reps):
    torch.cuda.synchronize()
    t0 = time.perf_counter()
    for _ in range(reps):
        fn()
    torch.cuda.synchronize()
    return (time.perf_counter() - t0) / reps * 1e6


def torch_ssim(rec, gt, H, W, wv, wh, cov, c1, c2):
    x = gt.reshape(1, H, W, O).permute(0, 3, 1, 2)
    y = rec.reshape(1, H, W, O).permute(0, 3, 1, 2)
    m = lambda t: F.conv2d(F.conv2d(t, wv, groups=O), wh, groups=O)
    mx, my = m(x), m(y)
    vx, vy, vxy = cov * (m(x * x) - mx * mx), cov * (m(y * y) - my * my), cov * (m(x * y) - mx * my)
    return (((2 * mx * my + c1) * (2 * vxy + c2)) / ((mx * mx + my * my + c1) * (vx + vy + c2))).mean()


def run(H, W, kind, blocks, reps):
    g = torch.Generator(device="cpu").manual_seed(H * 1000 + W)
    gt = torch.rand(H * W, O, generator=g).to(dev)
    rec = (gt + 0.1 * torch.randn(H * W, O, generator=g).to(dev)).contiguous()
    taps, win, cov = functional._ssim_window(kind)
    L = DATA_RANGE[kind]
    c1, c2 = (0.01 * L) ** 2, (0.03 * L) ** 2
    w = torch.tensor(list(win), dtype=torch.float32, device=dev)
    wv, wh = w.reshape(1, 1, -1, 1).repeat(O, 1, 1, 1), w.reshape(1, 1, 1, -1).repeat(O, 1, 1, 1)
    ws = [None]

    def hip():
        out, ws[0] = functional._ssim(rec, gt, H, W, kind, L, False, ws[0])       # FusedTrainer.ssim's call
        return out

    def hip_full():
        out, ws[0] = functional._ssim(rec, gt, H, W, kind, L, True, ws[0])
        return out

    variants = {"wire_ssim": hip, "wire_ssim + map": hip_full,
                "torch conv2d": lambda: torch_ssim(rec, gt, H, W, wv, wh, cov, c1, c2)}
    res = {k: [] for k in variants}
    for _ in range(blocks):
        for k, fn in variants.items():
            timed(fn, 10)
            res[k].append(timed(fn, reps))
    tag = f"{H} x {W} x {O} {kind} ({taps} taps)"
    a, b = float(hip()), float(variants["torch conv2d"]())
    print(f"{tag}: wire_ssim {a:.7f}  torch {b:.7f}  difference {abs(a - b):.2e}", flush=True)
    nbytes = 2 * H * W * O * 4                                    # the algorithm's traffic: both images read once
    for k, v in res.items():
        extra = (H - taps + 1) * (W - taps + 1) * O * 4 if k.endswith("map") else 0
        print(f"{tag}: {k:16s} mean {sum(v) / len(v):8.1f} us  min {min(v):8.1f} us per call"
              + (f"  ({(nbytes + extra) / min(v) * 1e-3:7.1f} GB/s of algorithmic bytes)" if k.startswith("wire") else ""),
              flush=True)
    print(f"{tag}: torch / wire_ssim (min) {min(res['torch conv2d']) / min(res['wire_ssim']):.2f} x", flush=True)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--sizes", nargs="*", default=["512x512", "768x512"])
    ap.add_argument("--windows", nargs="*", default=["gaussian", "uniform"], choices=sorted(DATA_RANGE))
    ap.add_argument("--blocks", type=int, default=5)
    ap.add_argument("--reps", type=int, default=300)
    a = ap.parse_args()
    p = torch.cuda.get_device_properties(dev)
    print(f"# {p.name} ({p.gcnArchName}, {p.multi_processor_count} CUs), torch {torch.__version__}, HIP {torch.version.hip}; "
          f"host-clock time per call over {a.reps} calls ending in a synchronise, {a.blocks} alternating blocks", flush=True)
    for size in a.sizes:
        H, W = (int(v) for v in size.split("x"))
        for kind in a.windows:
            run(H, W, kind, a.blocks, a.reps)


if __name__ == "__main__":
    main()
