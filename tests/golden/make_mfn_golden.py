#!/usr/bin/env python3
"""Golden vectors of the multiplicative filter network (modules/mfn.py; build container only).

    python3 tests/golden/make_mfn_golden.py        # writes the three files below into tests/golden/

Built with the REFERENCE's own ``modules.mfn`` (imported from the reference checkout, CPU; it needs numpy and torch only).
  * small_mfn.npz: two tiny nets (D = 2 and D = 3 -> 32, 2 hidden, 3 out): the full state_dict, 300 coordinates and
    targets, y, the loss and every MSE gradient -- the coordinates' included -- from autograd, in fp32 (the reference as
    it runs) and fp64;
  * full_mfn_2x256.npz: checksums of the state_dict of ``torch.manual_seed(seed); INR(2, 256, 2, 3)`` for two seeds, the
    names, shapes and the parameter count;
  * psnr_mfn.npz: the drivers' loop (Adam, lr = 5e-2 min(1, maxpoints / (H W)), LambdaLR 0.1^(epoch / niters), one
    torch.randperm per epoch) on a crop of the image stored in psnr_hier.npz, in fp32 and -- same init, same
    permutations -- in fp64: both loss trajectories and the final PSNR.  The generator checks and prints that the fp32
    run's own drift max |loss32 - loss64| / loss64 stays below 1e-2 over the whole run: a trajectory that has already
    diverged between fp32 and fp64 gates nothing.
"""
import os
import sys

import numpy as np
import torch

REF = "/root/reference"
OUT = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, os.path.join(REF, "modules"))
import mfn as rmfn  # noqa: E402  (the reference's own module)

torch.set_num_threads(int(os.environ.get("GOLDEN_THREADS", "8")))
NITERS, CROP, HF, HL, MAXPOINTS, LR = 40, 32, 64, 2, 256 * 256, 5e-2


def checksum(a):
    a = np.asarray(a).astype(np.float64).ravel()
    w = np.cos(np.arange(a.size) * 0.37) + 0.5
    return np.array([a.sum(), np.abs(a).sum(), (a * w).sum()], np.float64)


def small():
    rec = {}
    for D in (2, 3):
        torch.manual_seed(1)
        m = rmfn.INR(D, 32, 2, 3)
        g = torch.Generator().manual_seed(10 + D)
        x = torch.rand(1, 300, D, generator=g) * 2 - 1
        t = torch.rand(1, 300, 3, generator=g)
        tag = f"d{D}"
        for k, v in m.state_dict().items():
            rec[f"{tag}_sd__{k}"] = v.numpy().copy()
        rec[f"{tag}_coords"], rec[f"{tag}_target"] = x[0].numpy(), t[0].numpy()
        for sfx, dt in (("32", torch.float32), ("64", torch.float64)):
            mm = rmfn.INR(D, 32, 2, 3).to(dt)
            mm.load_state_dict({k: v.to(dt) for k, v in m.state_dict().items()})
            xx = x.to(dt).clone().requires_grad_(True)
            y = mm(xx)
            loss = ((y - t.to(dt)) ** 2).mean()
            loss.backward()
            rec[f"{tag}_y{sfx}"] = y[0].detach().numpy()
            rec[f"{tag}_loss{sfx}"] = np.float64(loss.item())
            rec[f"{tag}_gx{sfx}"] = xx.grad[0].numpy()
            for k, p in mm.named_parameters():
                rec[f"{tag}_g{sfx}__{k}"] = p.grad.numpy()
    np.savez_compressed(os.path.join(OUT, "small_mfn.npz"), **rec)


def full():
    rec = {}
    for seed in (0, 3):
        torch.manual_seed(seed)
        m = rmfn.INR(2, 256, 2, 3)
        for k, v in m.state_dict().items():
            rec[f"s{seed}__{k}"] = checksum(v.numpy())
    rec["names"] = np.array(list(m.state_dict().keys()))
    rec["shapes"] = np.array([str(tuple(v.shape)) for v in m.state_dict().values()])
    rec["nparams"] = np.int64(sum(p.numel() for p in m.parameters()))
    np.savez_compressed(os.path.join(OUT, "full_mfn_2x256.npz"), **rec)


def psnr(x, xhat):
    # modules/utils.py:67-82 (max(x), not its square)
    return 10 * np.log10(x.max() / np.mean((x - xhat) ** 2))


def psnr_loop():
    u8 = np.load(os.path.join(OUT, "psnr_hier.npz"))["image_u8"][:CROP, :CROP]
    H, W, _ = u8.shape
    im = np.divide(u8, 255, dtype=np.float32)
    X, Y = torch.meshgrid(torch.linspace(-1, 1, W), torch.linspace(-1, 1, H), indexing="xy")
    coords = torch.hstack((X.reshape(-1, 1), Y.reshape(-1, 1)))[None, ...]
    gt = torch.tensor(im).reshape(H * W, 3)[None, ...]
    res = {}
    torch.manual_seed(0)
    m0 = rmfn.INR(2, HF, HL, 3)
    perms = [torch.randperm(H * W) for _ in range(NITERS)]       # drawn right behind the seeded init
    for tag, dt in (("", torch.float32), ("64", torch.float64)):
        model = rmfn.INR(2, HF, HL, 3).to(dt)
        model.load_state_dict({k: v.to(dt) for k, v in m0.state_dict().items()})
        optim = torch.optim.Adam(lr=LR * min(1, MAXPOINTS / (H * W)), params=model.parameters())
        sched = torch.optim.lr_scheduler.LambdaLR(optim, lambda e: 0.1 ** min(e / NITERS, 1))
        c, g = coords.to(dt), gt.to(dt)
        rec = torch.zeros_like(g)
        losses = []
        for epoch in range(NITERS):
            b = perms[epoch]
            pix = model(c[:, b, ...])
            with torch.no_grad():
                rec[:, b, :] = pix
            loss = ((pix - g[:, b, :]) ** 2).mean()
            optim.zero_grad()
            loss.backward()
            optim.step()
            losses.append(float(loss.item()))
            sched.step()
        res["losses" + tag] = np.array(losses)
        res["psnr" + tag] = np.float64(psnr(im.astype(np.float64), rec[0].reshape(H, W, 3).double().numpy()))
        print(f"mfn{tag}: psnr {float(res['psnr' + tag]):.4f} dB, final loss {losses[-1]:.6f}", flush=True)
    drift = float(np.max(np.abs(res["losses"] - res["losses64"]) / res["losses64"]))
    print(f"fp32 drift over {NITERS} epochs: {drift:.3e} (must stay below 1e-2)", flush=True)
    assert drift < 1e-2, "the fp32 and fp64 trajectories have diverged: shorten the run"
    np.savez_compressed(os.path.join(OUT, "psnr_mfn.npz"), image_u8=u8, niters=np.int64(NITERS),
                        maxpoints=np.int64(MAXPOINTS), seed=np.int64(0), lr=np.float64(LR), hidden_features=np.int64(HF),
                        hidden_layers=np.int64(HL), drift=np.float64(drift),
                        perm_first8=np.stack([p[:8].numpy() for p in perms]),
                        **{"sd0_checksum__" + k: checksum(v.numpy()) for k, v in m0.state_dict().items()}, **res)


if __name__ == "__main__":
    small()
    full()
    psnr_loop()
