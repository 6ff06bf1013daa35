#!/usr/bin/env python3
"""Interleaved in-process A/B of the video compressive-sensing step on one case (256 x 256 x 32, one output, nframes 8,
a wire net of 2 x 128): the fused loss operator alone (wire_coded_mse_grad) and the whole FusedTrainer.step_coded, each
against the same arithmetic in eager PyTorch on the same device -- the network's [H*W*T, 1] output reshaped and permuted
into the reference's (1, T, H, W), multiplied by the masks, summed in groups of nframes with the last group twice,
((coded - gt)**2).mean(), autograd, torch.optim.Adam.  Timed with device events after a warm-up; blocks alternate
between the variants, so clock / temperature drift hits all alike.  The operator is also reported as algorithmic bytes
(y in + g_y out + mask + gt) over time and as a share of the MI355X's 8.0 TB/s HBM peak.  A measurement, not a gate:
it prints what it finds.
    python3 tools/video_cs_ab.py > profiles/video_cs_ab.txt
    python3 tools/video_cs_ab.py --height 32 --width 32 --frames 8 --blocks 2 --reps 5      # a small shape
"""
import argparse
import os
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
import numpy as np
import torch

from wire_amd import _lib
from wire_amd.modules import lin_inverse, models
from wire_amd.trainer import FusedTrainer

dev = torch.device("cuda:0")
K, HL, O = 128, 2, 1
HBM_PEAK = 8.0e12


def timed(fn, reps):
    """Milliseconds per call between two device events around `reps` calls."""
    a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    torch.cuda.synchronize()
    a.record()
    for _ in range(reps):
        fn()
    b.record()
    b.synchronize()
    return a.elapsed_time(b) / reps


def build():
    torch.manual_seed(0)
    return models.get_INR(nonlin="wire", in_features=3, out_features=O, hidden_features=K, hidden_layers=HL,
                          first_omega_0=10.0, hidden_omega_0=10.0, scale=10.0).to(dev)


def eager_coded(video, masks, nframes):
    """(1, T, H, W) -> (1, C + 1, H, W): groups of nframes frames of video * masks summed, the last group twice."""
    prod = video * masks
    frames = [prod[:, s:s + nframes].sum(1, keepdim=True) for s in range(0, video.shape[1], nframes)]
    return torch.cat(frames + frames[-1:], dim=1)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--height", type=int, default=256)
    ap.add_argument("--width", type=int, default=256)
    ap.add_argument("--frames", type=int, default=32)
    ap.add_argument("--nframes", type=int, default=8)
    ap.add_argument("--blocks", type=int, default=4)
    ap.add_argument("--reps", type=int, default=20)
    ap.add_argument("--op-reps", type=int, default=200)
    a = ap.parse_args()
    H, W, T, nf = a.height, a.width, a.frames, a.nframes
    NP, Cp = H * W, (T + nf - 1) // nf + 1
    p = torch.cuda.get_device_properties(dev)
    print(f"# {p.name} ({p.gcnArchName}, {p.multi_processor_count} CUs), torch {torch.__version__}, HIP "
          f"{torch.version.hip}; device-event time per call, {a.blocks} alternating blocks after a warm-up", flush=True)
    tag = f"{H} x {W} x {T}, O = {O}, nframes {nf}"

    np.random.seed(0)
    masks_np = lin_inverse.get_video_coding_frames((H, W, T), nf)
    masks = torch.tensor(masks_np.astype(np.float32), device=dev)                     # (H, W, T)
    masks_ref = masks.permute(2, 0, 1)[None].contiguous()                             # (1, T, H, W)
    gt = torch.rand(1, Cp, H, W, device=dev)                                          # == [C'][H*W][1]

    # ---- the operator alone
    L = _lib.lib()
    y = torch.randn(NP * T, O, device=dev)
    gy, loss, part = torch.empty_like(y), torch.zeros(1, device=dev), torch.empty(4096, device=dev)
    stream = torch.cuda.current_stream().cuda_stream

    def hip_op():
        _lib.check(L.wire_coded_mse_grad(stream, y.data_ptr(), 0, NP, NP, T, O, nf, 1, masks.data_ptr(), gt.data_ptr(),
                                         gy.data_ptr(), None, loss.data_ptr(), part.data_ptr()), "coded_mse_grad")

    yr = y.clone().requires_grad_(True)

    def eager_op():
        yr.grad = None
        video = yr.reshape(H, W, T).permute(2, 0, 1)[None]
        ((eager_coded(video, masks_ref, nf) - gt) ** 2).mean().backward()

    # ---- the whole step
    tr = FusedTrainer(build(), (H, W, T), None, lr=5e-3, niters=2000)
    eager = build()
    opt = torch.optim.Adam(lr=5e-3, params=eager.parameters())
    coords = torch.stack(torch.meshgrid(torch.linspace(-1, 1, H), torch.linspace(-1, 1, W), torch.linspace(-1, 1, T),
                                        indexing="ij"), dim=-1).reshape(1, -1, 3)[..., [1, 0, 2]].contiguous().to(dev)

    def hip_step():
        tr.step_coded(gt, masks, nf)

    def eager_step():
        video = eager(coords).reshape(H, W, T).permute(2, 0, 1)[None]
        l = ((eager_coded(video, masks_ref, nf) - gt) ** 2).mean()
        opt.zero_grad()
        l.backward()
        opt.step()

    # the two operators compute the same thing
    hip_op(); eager_op()
    torch.cuda.synchronize()
    l_e = float(((eager_coded(y.reshape(H, W, T).permute(2, 0, 1)[None], masks_ref, nf) - gt) ** 2).mean())
    print(f"{tag}: operator loss {float(loss):.7f}  eager {l_e:.7f};  max |g_y - eager grad| "
          f"{float((gy - yr.grad).abs().max()):.2e} of max {float(yr.grad.abs().max()):.2e}", flush=True)

    variants = {"wire_coded_mse_grad": (hip_op, a.op_reps), "eager operator": (eager_op, a.op_reps),
                "step_coded": (hip_step, a.reps), "eager step": (eager_step, a.reps)}
    res = {k: [] for k in variants}
    for k, (fn, reps) in variants.items():
        timed(fn, 5)
    for _ in range(a.blocks):
        for k, (fn, reps) in variants.items():
            timed(fn, 2)
            res[k].append(timed(fn, reps))
    nbytes = 4 * (2 * NP * T * O + NP * T + Cp * NP * O)            # y in + g_y out + mask + gt
    for k, v in res.items():
        print(f"{tag}: {k:20s} mean {sum(v) / len(v):9.4f} ms  min {min(v):9.4f} ms", flush=True)
    t = min(res["wire_coded_mse_grad"]) * 1e-3
    print(f"{tag}: operator {nbytes / 1e6:.2f} MB of algorithmic bytes / min time = {nbytes / t / 1e9:.1f} GB/s, "
          f"{nbytes / t / HBM_PEAK:.1%} of the 8.0 TB/s HBM peak (bandwidth-bound; the two launches included)", flush=True)
    print(f"{tag}: eager / wire_coded_mse_grad (min) "
          f"{min(res['eager operator']) / min(res['wire_coded_mse_grad']):.2f} x; eager / step_coded (min) "
          f"{min(res['eager step']) / min(res['step_coded']):.2f} x", flush=True)


if __name__ == "__main__":
    main()
