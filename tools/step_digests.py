#!/usr/bin/env python3
"""SHA-256 digests of what every FusedTrainer step leaves behind, for comparing two builds of the package bit for bit:
with fixed seeds and the small shapes of tests/test_gpu_step_launches.py, three steps of every step kind, and after
each step one line per buffer -- tr.flat, tr.loss, tr.y[:n] and, where the step has them, loss_parts, tv_parts,
reg.theta, rec_lr / est, and the psnr / ssim metric of a render.  It uses the public API alone, so the same file runs
against another checkout:
    python3 tools/step_digests.py > head.txt
    python3 tools/step_digests.py --root ../other-checkout > other.txt       # every line must be identical
step_radon's adjoint adds with float atomics (tests/test_gpu_workspace_fill.py), so its lines are not digests: --save
keeps its tr.flat of every step in a file, and --against prints the maximum relative difference to such a file.  The
yardstick is the same difference between two runs of one build.
    python3 tools/step_digests.py --save radon_a.pt > /dev/null
    python3 tools/step_digests.py --against radon_a.pt | grep radon
"""
import argparse
import hashlib
import os
import sys

ap = argparse.ArgumentParser()
ap.add_argument("--root", default=os.path.dirname(os.path.dirname(os.path.abspath(__file__))),
                help="the checkout whose wire_amd is imported (default: this file's)")
ap.add_argument("--save", help="write step_radon's flat parameters of every step to this file")
ap.add_argument("--against", help="compare step_radon's flat parameters with a file written by --save")
ap.add_argument("--steps", type=int, default=3)
args = ap.parse_args()
sys.path.insert(0, os.path.abspath(args.root))
import torch

from wire_amd.modules import models
from wire_amd.trainer import FusedTrainer

dev = torch.device("cuda:0")


def sha(t):
    return hashlib.sha256(t.detach().contiguous().cpu().numpy().tobytes()).hexdigest()


def rand(*shape, seed):
    return torch.rand(*shape, generator=torch.Generator().manual_seed(seed)).to(dev)


def wire(D, O):
    torch.manual_seed(0)
    return models.get_INR(nonlin="wire", in_features=D, out_features=O, hidden_features=128, hidden_layers=2,
                          first_omega_0=7.0, hidden_omega_0=7.0, scale=6.0).to(dev)


def hier(O):
    torch.manual_seed(0)
    return models.get_INR(nonlin="bspline_mscale_hier", in_features=2, out_features=O, hidden_features=64,
                          scaled_hidden_features=0, hidden_layers=2, first_omega_0=-0.2, hidden_omega_0=-0.2,
                          scale=0.0, scale_tensor=[1 / 9, 4.0]).to(dev)


def mscale2(O):
    torch.manual_seed(0)
    return models.get_INR(nonlin="bspline_mscale_2", in_features=2, out_features=O, hidden_features=64,
                          scaled_hidden_features=0, hidden_layers=2, first_omega_0=-0.2, hidden_omega_0=-0.2,
                          scale=0.0, scale_tensor=torch.tensor([1 / 9, 4.0]).to(dev)).to(dev)


radon_flats = {}


def run(tag, tr, step, n, extras=(), digest=True):
    """``step()`` args.steps times; n = the floats of tr.y the step writes; extras: (name, getter) pairs."""
    for i in range(args.steps):
        step()
        torch.cuda.synchronize()
        if not digest:
            radon_flats[f"{tag} {i}"] = tr.flat.detach().cpu().clone()
            continue
        for name, t in [("flat", tr.flat), ("loss", tr.loss), ("y", tr.y[:n])] + [(k, f()) for k, f in extras]:
            print(f"{tag} step {i} {name:10s} {sha(t)}", flush=True)


def main():
    H, W, O = 8, 6, 3
    n = H * W
    target = rand(n, O, seed=1)

    def image(model=None, lr=1e-3):
        return FusedTrainer(model or wire(2, O), (H, W), target, lr=lr, keep_rec=True)

    tr = image()
    run("step", tr, lambda: tr.step(first=0, count=16), 16 * O)
    tr = image()
    run("step_hashed", tr, lambda: tr.step_hashed(5, first=3, count=20), 20 * O,
        [("psnr", lambda: tr.psnr(tr.render()))])
    tr = image(mscale2(O))            # (its combiner's backward carries the loss partials of its own)
    run("step mscale_2", tr, lambda: tr.step(), n * O)
    gt = rand((H // 2) * (W // 2), O, seed=2)
    rec = torch.zeros_like(gt)
    tr = image()
    run("step_downsampled", tr, lambda: tr.step_downsampled(gt, 2, rec_lr=rec), n * O, [("rec_lr", lambda: rec)])
    tr = image()
    run("step_downsampled tv", tr, lambda: tr.step_downsampled(gt, 2, rec_lr=rec, lambda_tv=.1), n * O,
        [("rec_lr", lambda: rec), ("tv_parts", lambda: tr.tv_parts)])
    tr = image()
    run("step_tv", tr, lambda: tr.step_tv(.1), n * O, [("loss_parts", lambda: tr.loss_parts), ("rec", lambda: tr.rec)])
    idx = torch.randperm(n, generator=torch.Generator().manual_seed(3))[:20].to(dev)
    tr = image()
    run("step_tv indices", tr, lambda: tr.step_tv(.1, indices=idx), n * O, [("loss_parts", lambda: tr.loss_parts)])
    tr = image(hier(O), lr=[6e-3, 2e-2])
    run("step_tv hier", tr, lambda: tr.step_tv(0.), n * O, [("loss_parts", lambda: tr.loss_parts)])

    SH, SW = 12, 13
    for lam in (.1, 0.):
        tr = FusedTrainer(wire(2, O), (SH, SW), rand(SH * SW, O, seed=4), lr=1e-3)
        run(f"step_ssim {lam:g}", tr, lambda: tr.step_ssim(lam), SH * SW * O,
            [("loss_parts", lambda: tr.loss_parts), ("ssim", lambda: tr.ssim(tr.render()))])

    B = 2
    tr = FusedTrainer(wire(2, O), (H, W), None, lr=1e-3)
    xy = tr.affine_coords(torch.tensor([[[1., 0., 0.], [0., 1., 0.]], [[1., 0., .05], [0., 1., -.05]]]))
    gtf, mask = rand(B, (H // 2) * (W // 2), O, seed=5), (rand(B, (H // 2) * (W // 2), O, seed=6) < .8).float()
    recf = torch.zeros_like(gtf)
    run("step_frames", tr, lambda: tr.step_frames(xy, gtf, 2, mask=mask, rec_lr=recf), B * n * O,
        [("rec_lr", lambda: recf)])
    tr = FusedTrainer(wire(2, O), (H, W), None, lr=1e-3)
    reg = tr.registration(B, lr=1e-2)
    run("step_frames_registered", tr, lambda: tr.step_frames_registered(reg, xy, gtf, 2, mask=mask, rec_lr=recf),
        B * n * O, [("rec_lr", lambda: recf), ("theta", lambda: reg.theta), ("g_coords", lambda: tr.g_coords[:B * n])])

    VH, VW, VT, nframes = 4, 5, 6, 2
    NP = VH * VW
    coded = rand((VT // nframes + 1) * NP, seed=7)
    masks = (rand(NP * VT, seed=8) < .5).float()
    est = torch.zeros_like(coded)
    for tag, kw, rows in (("step_coded", {}, NP), ("step_coded tv", dict(lambda_tv=.1, lambda_tv_t=.05), NP),
                          ("step_coded slab 7", dict(slab=7), NP - 2 * 7)):
        tr = FusedTrainer(wire(3, 1), (VH, VW, VT), None, lr=1e-3)
        extras = [("est", lambda: est)] + ([("tv_parts", lambda: tr.tv_parts)] if "tv" in tag else [])
        run(tag, tr, lambda: tr.step_coded(coded, masks, nframes, est=est, **kw), rows * VT, extras)

    A = 5
    sino, th = rand(A * W, seed=9) * H, torch.linspace(0, 180, A)
    for tag, kw in (("step_radon", {}), ("step_radon tv", dict(lambda_tv=.1))):
        tr = FusedTrainer(wire(2, 1), (H, W), None, lr=1e-3)
        run(tag, tr, lambda: tr.step_radon(sino, th, **kw), n, digest=False)
    if args.save:
        torch.save(radon_flats, args.save)
    if args.against:
        saved = torch.load(args.against)
        for k, a in radon_flats.items():
            b = saved[k]
            print(f"{k}: flat max |a - b| / max |b| = {float((a - b).abs().max() / b.abs().max()):.3e}", flush=True)


if __name__ == "__main__":
    main()
