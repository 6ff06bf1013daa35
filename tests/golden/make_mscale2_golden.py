#!/usr/bin/env python3
"""Golden vectors of the multi-pass B-spline INR (modules/bspline_mscale_2.py; build container only).

    python3 tests/golden/make_mscale2_golden.py        # writes the three files below into tests/golden/

Built with the REFERENCE's own ``modules.bspline_mscale_2`` (imported from the reference checkout, CPU):
  * small_mscale2.npz: a tiny net (2 -> 32, 2 hidden, 3 out, scale_tensor [0.5, 0.25, 2]), its full state_dict,
    300 coordinates and targets, y and every MSE gradient -- the coordinates' included -- in fp32 (the reference as it
    runs) and fp64 (the same module in double), the parameter names / requires_grad / count_parameters;
  * full_mscale2_st4.npz: the net of configs.py's Mscale2_ST4_LR8e3_E4000 (scale_tensor [1/9, 4], 2 hidden x 256,
    scale 0) -- checksums of the seeded state_dict, y and checksums of the gradients on a 2048-row coordinate subset;
  * psnr_mscale2.npz: the reference's Adam + LambdaLR loop (as the bspline_*.py drivers run it) with that config on a
    64 x 64 crop of the reference's parrot image for NITERS epochs, fp32 and fp64 loss trajectories and the final PSNR.
"""
import os
import sys
import types

import numpy as np
import torch

REF = "/root/reference"
OUT = os.path.dirname(os.path.abspath(__file__))
ROOT = os.path.dirname(os.path.dirname(OUT))
sys.modules.setdefault("cv2", types.ModuleType("cv2"))
sys.path.insert(0, REF)
sys.path.insert(0, ROOT)
from modules import bspline_mscale_2 as m2, utils  # noqa: E402  (the reference's own modules)

torch.set_num_threads(int(os.environ.get("GOLDEN_THREADS", "8")))
NITERS = 100
IMAGE = "data_noisy/parrot_noisy_T30.0_snr2.png"
ST4 = [1 / 9, 4.0]


def checksum(a):
    a = np.asarray(a).astype(np.float64).ravel()
    w = np.cos(np.arange(a.size) * 0.37) + 0.5
    return np.array([a.sum(), np.abs(a).sum(), (a * w).sum()], np.float64)


def build(D, hf, L, O, scale, st, seed=0):
    torch.manual_seed(seed)
    return m2.INR(D, hf, 0, L, O, True, -0.2, -0.2, scale, torch.tensor(st))


def run(model, x, t, dtype):
    m = model.to(dtype)
    m.scale_tensor = m.scale_tensor.to(dtype)
    m.zero_grad()
    xt = torch.tensor(x, dtype=dtype)[None].requires_grad_(True)
    y = m(xt)[0]
    loss = ((y - torch.tensor(t, dtype=dtype)) ** 2).mean()
    loss.backward()
    g = {k: p.grad.detach().numpy().copy() for k, p in m.named_parameters() if p.grad is not None}
    out = y.detach().numpy().copy(), float(loss.item()), g, xt.grad[0].numpy().copy()
    m.to(torch.float32)
    m.scale_tensor = m.scale_tensor.to(torch.float32)
    return out


def meta(D, hf, L, O, scale, st, seed):
    return dict(meta_D=np.int64(D), meta_hidden_features=np.int64(hf), meta_L=np.int64(L), meta_O=np.int64(O),
                meta_scale0=np.float64(scale), meta_scale_tensor=np.array(st, np.float32).astype(np.float64),
                meta_seed=np.int64(seed))


def small():
    D, hf, L, O, s, st = 2, 32, 2, 3, 0.0, [0.5, 0.25, 2.0]
    model = build(D, hf, L, O, s, st)
    rng = np.random.default_rng(1)
    x = rng.uniform(-1, 1, (300, D)).astype(np.float32)
    t = rng.uniform(0, 1, (300, O)).astype(np.float32)
    rec = meta(D, hf, L, O, s, st, 0)
    sd = model.state_dict()
    rec["sd_keys"] = np.array(list(sd.keys()))
    for k, v in sd.items():
        rec["sd__" + k] = v.numpy().copy()
    rec["param_names"] = np.array([k for k, _ in model.named_parameters()])
    rec["param_requires_grad"] = np.array([p.requires_grad for _, p in model.named_parameters()])
    rec["count_parameters"] = np.int64(utils.count_parameters(model))
    rec["coords"], rec["target"] = x, t
    for tag, dt in (("32", torch.float32), ("64", torch.float64)):
        y, loss, g, gx = run(model, x, t, dt)
        rec["y" + tag], rec["loss" + tag], rec["gcoords" + tag] = y, np.float64(loss), gx
        rec["grad_keys" + tag] = np.array(sorted(g))
        for k, v in g.items():
            rec[f"g{tag}__{k}"] = v
    np.savez_compressed(os.path.join(OUT, "small_mscale2.npz"), **rec)


def full():
    D, hf, L, O, s, st = 2, 256, 2, 3, 0.0, ST4
    model = build(D, hf, L, O, s, st)
    rng = np.random.default_rng(2)
    x = rng.uniform(-1, 1, (2048, D)).astype(np.float32)
    t = rng.uniform(0, 1, (2048, O)).astype(np.float32)
    rec = meta(D, hf, L, O, s, st, 0)
    for k, v in model.state_dict().items():
        rec["sd0_checksum__" + k] = checksum(v.numpy())
    rec["coords"], rec["target"] = x, t
    for tag, dt in (("32", torch.float32), ("64", torch.float64)):
        y, loss, g, gx = run(model, x, t, dt)
        rec["y" + tag], rec["loss" + tag] = y, np.float64(loss)
        rec["gcoords_checksum" + tag] = checksum(gx)
        for k, v in g.items():
            rec[f"g{tag}_checksum__{k}"] = checksum(v)
    np.savez_compressed(os.path.join(OUT, "full_mscale2_st4.npz"), **rec)


def psnr_loop():
    from PIL import Image
    u8 = np.ascontiguousarray(np.asarray(Image.open(os.path.join(REF, IMAGE)))[300:364, 500:564, :3])
    H, W, _ = u8.shape
    im = np.divide(u8, 255, dtype=np.float32)
    x = torch.linspace(-1, 1, W)
    y = torch.linspace(-1, 1, H)
    X, Y = torch.meshgrid(x, y, indexing="xy")
    coords = torch.hstack((X.reshape(-1, 1), Y.reshape(-1, 1)))[None, ...]
    gt = torch.tensor(im).reshape(H * W, 3)[None, ...]
    hf, L, s, st, lr, maxpoints = 256, 2, 0.0, ST4, 8e-3, 256 * 256
    lr0 = lr * min(1, maxpoints / (H * W))
    res = {}
    perms = []
    model = build(2, hf, L, 3, s, st)
    sd0 = {k: v.detach().clone() for k, v in model.state_dict().items()}
    for tag, dt in (("", torch.float32), ("64", torch.float64)):
        if tag:
            model.load_state_dict(sd0)
            model = model.to(dt)
            model.scale_tensor = model.scale_tensor.to(dt)
        optim = torch.optim.Adam(lr=lr0, params=model.parameters())
        sched = torch.optim.lr_scheduler.LambdaLR(optim, lambda e: 0.1 ** min(e / NITERS, 1))
        c, g = coords.to(dt), gt.to(dt)
        rec = torch.zeros_like(g)
        losses = []
        for epoch in range(NITERS):
            if not tag:
                perms.append(torch.randperm(H * W))
            indices = perms[epoch]
            for b_idx in range(0, H * W, maxpoints):
                b = indices[b_idx:min(H * W, b_idx + maxpoints)]
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
        res["psnr" + tag] = np.float64(utils.psnr(im, rec[0].reshape(H, W, 3).double().numpy()))
        print(f"mscale_2 psnr{tag}: {float(res['psnr' + tag]):.4f} dB, final loss {losses[-1]:.6f}", flush=True)
    np.savez_compressed(os.path.join(OUT, "psnr_mscale2.npz"), image_u8=u8, niters=np.int64(NITERS),
                        maxpoints=np.int64(maxpoints), seed=np.int64(0), lr=np.float64(lr), hidden_features=np.int64(hf),
                        hidden_layers=np.int64(L), scale=np.float64(s), scale_tensor=np.array(st, np.float64),
                        perm_first8=np.stack([p[:8].numpy() for p in perms]),
                        **{"sd0_checksum__" + k: checksum(v.numpy()) for k, v in sd0.items()}, **res)


if __name__ == "__main__":
    small()
    full()
    psnr_loop()
