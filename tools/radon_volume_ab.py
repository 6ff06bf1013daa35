#!/usr/bin/env python3
"""Volume CT: the batched Radon kernels against the per-slice route, and their share of a training step.

At one CT-like shape (default 128 x 128 x 64, 90 angles, siren 4 x 256) it times, interleaved in blocks so that clock
and temperature drift hit every variant alike, and prints the MEDIAN over the blocks:
    wire_radon_vol_fwd / wire_radon_vol_bwd on [H][W][T] data                               (events on the stream)
    the same work by the existing kernels: transpose to [T][H][W], T launches of wire_radon_fwd / wire_radon_bwd,
        transpose the result back to slice-last (lin_inverse.radon(..., is_3d=True) between two permutes)
    FusedTrainer.step_radon_volume, one pass and in slabs                                    (host clock + synchronise)
with the algorithmic bytes of each kernel (every operand once) and the rate they imply.  A measurement without a
target: it prints what it finds, and says whether the batched operator beats the per-slice route and what share of the
one-pass step the two Radon kernels take.
    python3 tools/radon_volume_ab.py > profiles/radon_volume_ab.txt
    python3 tools/radon_volume_ab.py --shape 24x20x8 --angles 9 --slab 100 --blocks 2 --reps 5     # a small shape
"""
import argparse
import ctypes as C
import os
import statistics
import sys
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
import torch

from wire_amd import _lib
from wire_amd.modules import lin_inverse, models
from wire_amd.trainer import FusedTrainer

dev = torch.device("cuda:0")


def timed(fn, reps):
    """Host-clock microseconds per call over reps calls ending in a synchronise."""
    torch.cuda.synchronize()
    t0 = time.perf_counter()
    for _ in range(reps):
        fn()
    torch.cuda.synchronize()
    return (time.perf_counter() - t0) / reps * 1e6


def event_timed(fn, reps):
    """Event microseconds per call: reps back-to-back calls between two events on the stream."""
    a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    torch.cuda.synchronize()
    a.record()
    for _ in range(reps):
        fn()
    b.record()
    torch.cuda.synchronize()
    return a.elapsed_time(b) / reps * 1e3


def medians(variants, blocks, reps, timer):
    res = {k: [] for k in variants}
    for _ in range(blocks):
        for k, fn in variants.items():
            timer(fn, 2)
            res[k].append(timer(fn, reps))
    return {k: (statistics.median(v), min(v), max(v)) for k, v in res.items()}


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--shape", default="128x128x64", help="H x W x T of the volume")
    ap.add_argument("--angles", type=int, default=90)
    ap.add_argument("--slab", type=int, default=4096, help="pixels per slab of the slabbed step")
    ap.add_argument("--kind", default="siren")
    ap.add_argument("--hidden", type=int, default=256)
    ap.add_argument("--layers", type=int, default=4)
    ap.add_argument("--blocks", type=int, default=5)
    ap.add_argument("--reps", type=int, default=10)
    ap.add_argument("--kernel-reps", type=int, default=50)
    a = ap.parse_args()
    H, W, T = (int(v) for v in a.shape.split("x"))
    A = a.angles
    p = torch.cuda.get_device_properties(dev)
    print(f"# {p.name} ({p.gcnArchName}, {p.multi_processor_count} CUs), torch {torch.__version__}, HIP "
          f"{torch.version.hip}; volume {H} x {W} x {T}, {A} angles; {a.blocks} alternating blocks, median [min .. max]",
          flush=True)
    L = _lib.lib()
    s = torch.cuda.current_stream(dev).cuda_stream
    gen = torch.Generator().manual_seed(1)
    vol = torch.rand(H, W, T, generator=gen).to(dev)
    th = torch.linspace(0, 180, A).to(dev)
    sino = torch.empty(A, W, T, device=dev)
    gvol = torch.empty(H, W, T, device=dev)

    def vol_fwd():
        _lib.check(L.wire_radon_vol_fwd(s, vol.data_ptr(), th.data_ptr(), H, W, T, A, sino.data_ptr()))

    def vol_bwd():
        _lib.check(L.wire_radon_vol_bwd(s, sino.data_ptr(), th.data_ptr(), H, W, T, A, gvol.data_ptr()))

    # the per-slice route on the same slice-last data: lin_inverse.radon's T launches between two transposes
    st = torch.empty(T, A, W, device=dev)
    gt = torch.empty(T, H, W, device=dev)

    def slice_fwd():
        x = vol.permute(2, 0, 1).contiguous()
        for k in range(T):
            _lib.check(L.wire_radon_fwd(s, x[k].data_ptr(), th.data_ptr(), H, W, A, st[k].data_ptr()))
        return st.permute(1, 2, 0).contiguous()

    def slice_bwd():
        g = sino.permute(2, 0, 1).contiguous()
        for k in range(T):
            _lib.check(L.wire_radon_bwd(s, g[k].data_ptr(), th.data_ptr(), H, W, A, gt[k].data_ptr()))
        return gt.permute(1, 2, 0).contiguous()

    vol_fwd()
    same = torch.equal(slice_fwd(), sino)
    print(f"# the per-slice route gives the batched forward's bits: {same}", flush=True)
    k = medians({"wire_radon_vol_fwd": vol_fwd, "wire_radon_vol_bwd": vol_bwd, "per-slice forward": slice_fwd,
                 "per-slice adjoint": slice_bwd}, a.blocks, a.kernel_reps, event_timed)
    bytes_fwd = 4 * (H * W * T + A * W * T)
    for name, (med, lo, hi) in k.items():
        print(f"kernels: {name:22s} {med:9.1f} us [{lo:9.1f} .. {hi:9.1f}]  algorithmic {bytes_fwd / 1e6:7.2f} MB = "
              f"{bytes_fwd / med * 1e-3:8.1f} GB/s", flush=True)
    f, b = k["wire_radon_vol_fwd"][0], k["wire_radon_vol_bwd"][0]
    pf, pb = k["per-slice forward"][0], k["per-slice adjoint"][0]
    print(f"kernels: batched forward {pf / f:.2f} x the per-slice route's speed, batched adjoint {pb / b:.2f} x; "
          f"forward + adjoint {f + b:.1f} us against {pf + pb:.1f} us: the batched operator "
          f"{'beats' if f + b < pf + pb else 'DOES NOT beat'} the per-slice route; adjoint / forward {b / f:.2f}",
          flush=True)

    # ---- the step
    torch.manual_seed(0)
    hp = (30.0, 30.0, 10.0) if a.kind != "wire" else (20.0, 20.0, 30.0)
    model = models.get_INR(nonlin=a.kind, in_features=3, out_features=1, hidden_features=a.hidden,
                           hidden_layers=a.layers, first_omega_0=hp[0], hidden_omega_0=hp[1], scale=hp[2]).to(dev)
    tr = FusedTrainer(model, (H, W, T), None, lr=1e-4)
    with torch.no_grad():
        target = lin_inverse.radon_volume(vol, th).reshape(-1).contiguous()
    slab = min(a.slab, H * W - 1)
    steps = medians({"one pass": lambda: tr.step_radon_volume(target, th),
                     f"slab {slab} px": lambda: tr.step_radon_volume(target, th, slab=slab)}, a.blocks, a.reps, timed)
    d = tr.desc
    act_full = L.wire_act_bytes(C.byref(d), H * W * T, 1)
    act_slab = L.wire_act_bytes(C.byref(d), slab * T, 1)
    print(f"# step_radon_volume: {a.kind} {a.layers} x {a.hidden}, {H * W * T} rows; activations of the storing forward "
          f"{act_full / 2 ** 20:.0f} MiB one pass, {act_slab / 2 ** 20:.0f} MiB per slab of {slab} pixels "
          f"({(H * W + slab - 1) // slab} slabs) + {8 * H * W * T / 2 ** 20:.0f} MiB for the two full-volume buffers",
          flush=True)
    for name, (med, lo, hi) in steps.items():
        print(f"step: {name:16s} {med:10.1f} us [{lo:10.1f} .. {hi:10.1f}]", flush=True)
    one = steps["one pass"][0]
    print(f"step: the two Radon kernels take {100 * (f + b) / one:.1f} % of the one-pass step "
          f"({f + b:.1f} of {one:.1f} us); slabbed / one pass {steps[f'slab {slab} px'][0] / one:.3f} x", flush=True)


if __name__ == "__main__":
    main()
