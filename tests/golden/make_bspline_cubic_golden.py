#!/usr/bin/env python3
"""Golden vectors of the cubic B-spline INR (modules/bspline_cubic.py; build container only).

    python3 tests/golden/make_bspline_cubic_golden.py          # writes the two files below into tests/golden/

Built with the REFERENCE's own ``modules.bspline_cubic`` (imported from the reference checkout, CPU; the checkout is
REFERENCE_DIR, by default where make_bspline_golden.py finds it).  The net is built through the module's own constructor
in its own positional order -- (in, hidden, hidden_layers, scaled_hidden_features, out, ...): the reference's get_INR
passes hidden_layers and scaled_hidden_features the other way round and cannot build it.
  * small_bspline_cubic.npz: a tiny net (2 -> 32, 2 hidden, 3 out, scale 4), its full state_dict with key order, 300
    coordinates and targets, y and every MSE gradient in fp32 (the reference as it runs: five cubed relus) and in double
    (the same module in double), the reference's parameter names / count_parameters, and the seeded state_dict checksums
    of the class defaults (2 x 256, scale 15);
  * psnr_bspline_cubic.npz: the reference's Adam + LambdaLR loop (wire_image_denoise.py:123-157 shape) on the 64 x 64
    parrot crop stored in psnr_bspline_s9.npz, a 2 x 256 net at scale 15, lr 1e-3, NITERS epochs of one 4096-row batch,
    with the fp32 and double loss trajectories and both final PSNRs.
"""
import os
import sys
import types

import numpy as np
import torch

REF = os.environ.get("REFERENCE_DIR", "/root/reference")
OUT = os.path.dirname(os.path.abspath(__file__))
ROOT = os.path.dirname(os.path.dirname(OUT))
sys.modules.setdefault("cv2", types.ModuleType("cv2"))
sys.path.insert(0, REF)
sys.path.insert(0, ROOT)
from modules import bspline_cubic, utils  # noqa: E402  (the reference's own modules)

torch.set_num_threads(int(os.environ.get("GOLDEN_THREADS", "8")))
NITERS = 150


def checksum(a):
    a = np.asarray(a).astype(np.float64).ravel()
    w = np.cos(np.arange(a.size) * 0.37) + 0.5
    return np.array([a.sum(), np.abs(a).sum(), (a * w).sum()], np.float64)


def build(D, hf, L, O, scale, seed=0, outermost_linear=True):
    torch.manual_seed(seed)
    return bspline_cubic.INR(D, hf, L, 0, O, outermost_linear, -0.2, -0.2, scale)


def run(model, x, t, dtype):
    m = model.to(dtype)
    m.zero_grad()
    y = m(torch.tensor(x, dtype=dtype))
    loss = ((y - torch.tensor(t, dtype=dtype)) ** 2).mean()
    loss.backward()
    g = {k: p.grad.detach().numpy().copy() for k, p in m.named_parameters() if p.grad is not None}
    out = y.detach().numpy().copy(), float(loss.item()), g
    m.to(torch.float32)
    return out


def small():
    D, hf, L, O, s = 2, 32, 2, 3, 4.0
    model = build(D, hf, L, O, s)
    rng = np.random.default_rng(1)
    x = rng.uniform(-1, 1, (300, D)).astype(np.float32)
    t = rng.uniform(0, 1, (300, O)).astype(np.float32)
    rec = dict(meta_D=np.int64(D), meta_hidden_features=np.int64(hf), meta_L=np.int64(L), meta_O=np.int64(O),
               meta_scale0=np.float64(s), meta_seed=np.int64(0))
    sd = model.state_dict()
    rec["sd_keys"] = np.array(list(sd.keys()))
    for k, v in sd.items():
        rec["sd__" + k] = v.numpy().copy()
    rec["param_names"] = np.array([k for k, _ in model.named_parameters()])
    rec["param_requires_grad"] = np.array([p.requires_grad for _, p in model.named_parameters()])
    rec["count_parameters"] = np.int64(utils.count_parameters(model))
    rec["coords"], rec["target"] = x, t
    for tag, dt in (("32", torch.float32), ("64", torch.float64)):
        y, loss, g = run(model, x, t, dt)
        rec["y" + tag], rec["loss" + tag] = y, np.float64(loss)
        for k, v in g.items():
            rec[f"g{tag}__{k}"] = v
    # the class defaults (scale 15) at 2 x 256: checksums of the seeded state_dict
    torch.manual_seed(0)
    dflt = bspline_cubic.INR(2, 256, 2, 0, 3)
    rec["default_sd_keys"] = np.array(list(dflt.state_dict().keys()))
    for k, v in dflt.state_dict().items():
        rec["default_sd0_checksum__" + k] = checksum(v.numpy())
    np.savez_compressed(os.path.join(OUT, "small_bspline_cubic.npz"), **rec)


def psnr_loop():
    u8 = np.load(os.path.join(OUT, "psnr_bspline_s9.npz"), allow_pickle=False)["image_u8"]
    H, W, _ = u8.shape
    im = np.divide(u8, 255, dtype=np.float32)
    x = torch.linspace(-1, 1, W)
    y = torch.linspace(-1, 1, H)
    X, Y = torch.meshgrid(x, y, indexing="xy")
    coords = torch.hstack((X.reshape(-1, 1), Y.reshape(-1, 1)))[None, ...]
    gt = torch.tensor(im).reshape(H * W, 3)[None, ...]
    hf, L, s, lr, maxpoints = 256, 2, 15.0, 1e-3, 4096
    lr0 = lr * min(1, maxpoints / (H * W))
    res = {}
    perms = []
    torch.manual_seed(0)
    model = bspline_cubic.INR(2, hf, L, 0, 3, True, -0.2, -0.2, s)
    sd0 = {k: v.detach().clone() for k, v in model.state_dict().items()}
    for tag, dt in (("", torch.float32), ("64", torch.float64)):
        if tag:
            model.load_state_dict(sd0)
            model = model.to(dt)
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
        print(f"bspline_cubic psnr{tag}: {float(res['psnr' + tag]):.4f} dB, final loss {losses[-1]:.6f}", flush=True)
    dev = np.max(np.abs(res["losses"] - res["losses64"]) / res["losses64"])
    print(f"largest relative deviation of the fp32 loss trajectory from the double one: {dev:.3e}", flush=True)
    np.savez_compressed(os.path.join(OUT, "psnr_bspline_cubic.npz"), niters=np.int64(NITERS),
                        maxpoints=np.int64(maxpoints), seed=np.int64(0), lr=np.float64(lr), hidden_features=np.int64(hf),
                        hidden_layers=np.int64(L), scale=np.float64(s), ref32_dev_vs_double=np.float64(dev),
                        perm_first8=np.stack([p[:8].numpy() for p in perms]),
                        **{"sd0_checksum__" + k: checksum(v.numpy()) for k, v in sd0.items()}, **res)


if __name__ == "__main__":
    small()
    psnr_loop()
