#!/usr/bin/env python3
"""Interleaved in-process timing of hierarchical ray sampling (wire_composite_weights and wire_ray_resample in
wire_render.hip) at R = 4096 rays, S = 64 coarse and Nf = 128 fine samples, O = 4:

  kernels   wire_composite_weights against wire_composite_fwd on the same R x S rows, and wire_ray_resample against
            wire_ray_samples at R (S + Nf) samples (the same output bytes).  Event time over back-to-back calls, blocks
            alternating between the variants, the median over the blocks with the spread, the algorithm's bytes (each
            buffer counted once; the weights kernel's y counted as the one column it uses) and the rate they imply.
  step      FusedTrainer.step_rays(S = 64, n_importance = 128) against step_rays(S = 192): the same second-pass rows.
            The extra is one forward-only pass over the R S coarse rows plus three launches; the pass and the launches
            are timed alone and printed beside the difference.  step_rays(S = 64) is printed too, to lay beside the
            interval profiles/render_ab.txt records for the commit before n_importance existed.
  quality   on the host, by the fp64 restatements (tests/render_ref.py, tests/resample_ref.py): a thin Gaussian shell
            inside a faint halo, jittered samples, mean |rgb error| against a 4096-sample quadrature for S + Nf uniform
            samples against S coarse + Nf hierarchical ones.

A measurement, not a gate: it prints what it finds.
    python3 tools/resample_ab.py > profiles/resample_ab.txt
    python3 tools/resample_ab.py --blocks 2 --kernel-reps 50 --reps 5          # a short run
    python3 tools/resample_ab.py --quality-only                                # needs no GPU
"""
import argparse
import ctypes as C
import os
import statistics
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tests"))
import numpy as np


def quality():
    import render_ref as rr
    import resample_ref as rs
    R, Q = 512, 4096
    rng = np.random.default_rng(0)
    o = rng.normal(0, 1, (R, 3))
    o = 2.5 * o / np.linalg.norm(o, axis=1, keepdims=True)
    d = rng.uniform(-0.4, 0.4, (R, 3)) - o
    rays = np.concatenate([o, d / np.linalg.norm(d, axis=1, keepdims=True)], 1).astype(np.float32)
    near, far = np.float32(1.0), np.float32(4.0)

    def field(x):
        """(c_raw, sigma) rows: a shell of radius 0.6 and thickness 0.03 (peak density 40) in a halo of width 0.8
        (peak 0.3); the colour varies smoothly with the position."""
        x = x.astype(np.float64)
        rad = np.linalg.norm(x, axis=1)
        sigma = 40.0 * np.exp(-(rad - 0.6) ** 2 / (2 * 0.03 ** 2)) + 0.3 * np.exp(-rad ** 2 / (2 * 0.8 ** 2))
        col = np.clip(0.5 + 0.45 * np.sin(3.0 * x + np.array([0.0, 1.0, 2.0])), 1e-6, 1 - 1e-6)
        return np.concatenate([np.log(col / (1 - col)), sigma[:, None]], 1)

    def render(coords, ts, dl):
        return rr.composite(field(coords), ts, dl, None, "relu")[0]

    ref = render(*rr.ray_samples(rays, near, far, Q))
    print(f"# quality: {R} rays through a Gaussian shell (radius 0.6, thickness 0.03, peak density 40) in a halo (width "
          f"0.8, peak 0.3), [near, far] = [1, 4]; mean |rgb - quadrature({Q} midpoints)| over rays, channels and 8 "
          "jitter seeds; fp64 restatements on the host", flush=True)
    for S, Nf in ((8, 16), (16, 32), (32, 64)):
        eu, eh, ec = [], [], []
        for seed in range(8):
            g = np.random.default_rng(100 + seed)
            uu = g.uniform(0, 1, (R, S + Nf)).astype(np.float32)
            uc, uf = g.uniform(0, 1, (R, S)).astype(np.float32), g.uniform(0, 1, (R, Nf)).astype(np.float32)
            eu.append(np.abs(render(*rr.ray_samples(rays, near, far, S + Nf, uu)) - ref).mean())
            cc, tc, dc = rr.ray_samples(rays, near, far, S, uc)
            ec.append(np.abs(render(cc, tc, dc) - ref).mean())
            w = rr._weights(field(cc), tc, dc, "relu")[5].astype(np.float32)
            eh.append(np.abs(render(*rs.ray_resample(rays, near, far, tc, w, Nf, uf)) - ref).mean())
        print(f"quality S = {S:2d}, Nf = {Nf:2d}: coarse alone ({S}) {np.mean(ec):.3e}   uniform ({S + Nf}) "
              f"{np.mean(eu):.3e}   hierarchical ({S} + {Nf}) {np.mean(eh):.3e}   hierarchical / uniform "
              f"{np.mean(eh) / np.mean(eu):.2f}", flush=True)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--blocks", type=int, default=7)
    ap.add_argument("--kernel-reps", type=int, default=500)
    ap.add_argument("--reps", type=int, default=30)
    ap.add_argument("--quality-only", action="store_true")
    a = ap.parse_args()
    if a.quality_only:
        quality()
        return
    import time

    import torch

    from wire_amd import _lib
    from wire_amd.modules import models
    from wire_amd.trainer import FusedTrainer
    dev = torch.device("cuda:0")
    p = torch.cuda.get_device_properties(dev)
    print(f"# {p.name} ({p.gcnArchName}, {p.multi_processor_count} CUs), torch {torch.__version__}, HIP {torch.version.hip}",
          flush=True)
    L = _lib.lib()
    s = torch.cuda.current_stream(dev).cuda_stream
    R, S, Nf, O = 4096, 64, 128, 4
    M = S + Nf

    def timed(fn, reps):
        torch.cuda.synchronize()
        t0 = time.perf_counter()
        for _ in range(reps):
            fn()
        torch.cuda.synchronize()
        return (time.perf_counter() - t0) / reps * 1e6

    def event_timed(fn, reps):
        e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        torch.cuda.synchronize()
        e0.record()
        for _ in range(reps):
            fn()
        e1.record()
        torch.cuda.synchronize()
        return e0.elapsed_time(e1) / reps * 1e3

    # ---- kernels
    g = torch.Generator().manual_seed(R + S)
    rays = torch.randn(R, 6, generator=g).to(dev)
    uc, uf, um = (torch.rand(R, k, generator=g).to(dev) for k in (S, Nf, M))
    y = torch.randn(R * S, O, generator=g).to(dev)
    bg = torch.rand(O - 1, generator=g).to(dev)
    e = lambda *shape: torch.empty(*shape, device=dev)
    cc, tc, dc, w = e(R * S, 3), e(R, S), e(R, S), e(R, S)
    cm, tm, dm = e(R * M, 3), e(R, M), e(R, M)
    rgb, acc, depth = e(R, O - 1), e(R), e(R)
    _lib.check(L.wire_ray_samples(s, rays.data_ptr(), None, 0.5, 4.5, uc.data_ptr(), R, S, cc.data_ptr(), tc.data_ptr(),
                                  dc.data_ptr()))
    f4, n = 4, R * S
    variants = {
        "wire_composite_fwd (yardstick)": (
            lambda: _lib.check(L.wire_composite_fwd(s, y.data_ptr(), tc.data_ptr(), dc.data_ptr(), bg.data_ptr(), R, S, O,
                                                    0, rgb.data_ptr(), acc.data_ptr(), depth.data_ptr())),
            f4 * (n * O + 2 * n + 5 * R)),
        "wire_composite_weights": (
            lambda: _lib.check(L.wire_composite_weights(s, y.data_ptr(), dc.data_ptr(), R, S, O, 0, w.data_ptr())),
            f4 * 3 * n),
        f"wire_ray_samples x {M} (yardstick)": (
            lambda: _lib.check(L.wire_ray_samples(s, rays.data_ptr(), None, 0.5, 4.5, um.data_ptr(), R, M, cm.data_ptr(),
                                                  tm.data_ptr(), dm.data_ptr())),
            f4 * (6 * R + R * M + 5 * R * M)),
        f"wire_ray_resample {S} + {Nf} (jitter)": (
            lambda: _lib.check(L.wire_ray_resample(s, rays.data_ptr(), None, 0.5, 4.5, tc.data_ptr(), w.data_ptr(),
                                                   uf.data_ptr(), 1e-5, R, S, Nf, cm.data_ptr(), tm.data_ptr(),
                                                   dm.data_ptr())),
            f4 * (6 * R + 2 * n + R * Nf + 5 * R * M)),
        f"wire_ray_samples x {S} (the coarse pass's)": (
            lambda: _lib.check(L.wire_ray_samples(s, rays.data_ptr(), None, 0.5, 4.5, uc.data_ptr(), R, S, cc.data_ptr(),
                                                  tc.data_ptr(), dc.data_ptr())),
            f4 * (6 * R + n + 5 * n)),
    }
    list(variants.values())[1][0]()                        # w holds real weights before the resampler reads it
    res = {k: [] for k in variants}
    for _ in range(a.blocks):
        for k, (fn, _) in variants.items():
            event_timed(fn, 20)
            res[k].append(event_timed(fn, a.kernel_reps))
    print(f"# kernels: R = {R} rays, S = {S}, Nf = {Nf}, O = {O}; event time over {a.kernel_reps} back-to-back calls, "
          f"median of {a.blocks} alternating blocks", flush=True)
    med = {k: statistics.median(v) for k, v in res.items()}
    names = list(variants)
    base = {names[0]: names[0], names[1]: names[0], names[2]: names[2], names[3]: names[2], names[4]: names[2]}
    for k, (_, b) in variants.items():
        v = res[k]
        print(f"kernel: {k:44s} median {med[k]:8.2f} us  min {min(v):8.2f}  max {max(v):8.2f}  algorithmic "
              f"{b / 1e6:6.2f} MB = {b / med[k] * 1e-3:7.1f} GB/s  / its yardstick {med[k] / med[base[k]]:5.2f} x", flush=True)
    launches = med[names[4]] + med[names[1]] + med[names[3]]

    # ---- whole steps
    for kind in ("siren", "wire"):
        torch.manual_seed(0)
        hp = dict(first_omega_0=30.0, hidden_omega_0=30.0, scale=10.0) if kind == "siren" else \
            dict(first_omega_0=20.0, hidden_omega_0=20.0, scale=30.0)
        model = models.get_INR(nonlin=kind, in_features=3, out_features=4, hidden_features=256, hidden_layers=4,
                               **hp).to(dev)
        tr = FusedTrainer(model, (4, 4, 4), None, lr=1e-5)
        gg = torch.Generator().manual_seed(1)
        o = torch.randn(R, 3, generator=gg)
        o = 2.5 * o / o.norm(dim=1, keepdim=True)
        d = (torch.rand(R, 3, generator=gg) - 0.5) - o
        rr_ = torch.cat([o, d / d.norm(dim=1, keepdim=True)], 1).to(dev).contiguous()
        tgt = torch.rand(R, 3, generator=gg).to(dev)
        dp = C.byref(tr.desc)
        ab = _lib.check(L.wire_act_bytes(dp, n, 0))
        act = torch.empty(max(ab, 16), dtype=torch.uint8, device=dev)
        yc = e(n, O)
        steps = {f"step_rays(S={M})": lambda: tr.step_rays(rr_, tgt, 1.5, 3.5, M),
                 f"step_rays(S={S}, n_importance={Nf})": lambda: tr.step_rays(rr_, tgt, 1.5, 3.5, S, n_importance=Nf),
                 f"step_rays(S={S})": lambda: tr.step_rays(rr_, tgt, 1.5, 3.5, S),
                 f"forward-only pass, {n} rows": lambda: _lib.check(L.wire_mlp_fwd(
                     s, dp, tr.packed.data_ptr(), cc.data_ptr(), n, yc.data_ptr(), act.data_ptr(), ab, 0))}
        sres = {k: [] for k in steps}
        for _ in range(a.blocks):
            for k, fn in steps.items():
                timed(fn, 5)
                sres[k].append(timed(fn, a.reps))
        print(f"# whole optimizer step, {kind} 4 x 256, D = 3, O = 4, {R} rays; host clock over {a.reps} calls ending in "
              f"a synchronise, median of {a.blocks} alternating blocks", flush=True)
        sm = {k: statistics.median(v) for k, v in sres.items()}
        for k, v in sres.items():
            print(f"step {kind}: {k:36s} median {sm[k]:9.1f} us  min {min(v):9.1f}  max {max(v):9.1f}", flush=True)
        ks = list(steps)
        extra = sm[ks[1]] - sm[ks[0]]
        print(f"step {kind}: hierarchical - uniform at the same {R * M} second-pass rows: {extra:+.1f} us "
              f"({sm[ks[1]] / sm[ks[0]]:.4f} x); expected = forward-only pass {sm[ks[3]]:.1f} us + three launches "
              f"(samples {med[names[4]]:.1f} + weights {med[names[1]]:.1f} + resample {med[names[3]]:.1f} = "
              f"{launches:.1f} us) = {sm[ks[3]] + launches:.1f} us, less the uniform step's own sampler "
              f"{med[names[2]]:.1f} us", flush=True)
    quality()


if __name__ == "__main__":
    main()
