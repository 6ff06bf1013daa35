#!/usr/bin/env python3
"""Golden vectors of the hierarchical B-spline INR (modules/bspline_mscale_hier.py; build container only).

    python3 tests/golden/make_hier_golden.py        # writes the four files below into tests/golden/

Built with the REFERENCE's own ``modules.bspline_mscale_hier`` (imported from the reference checkout, CPU).  Its layer
creates scale_0 on 'cuda'; while the module is built here ``torch.ones`` drops that argument (it draws no random
numbers, so the seeded weights are what a GPU build gets).  The heads ``model.linears`` are a plain list that
``model.to(dtype)`` does not reach: they are converted one by one for the fp64 runs.
  * small_hier.npz: a tiny net (2 -> 32, 2 hidden, 3 out, scale_tensor [0.5, 0.25, 2]): its full state_dict, the heads,
    300 coordinates and targets, y, the loss and every MSE gradient -- the heads' and the coordinates' included -- in
    fp32 (the reference as it runs) and fp64, the parameter names / requires_grad / count_parameters;
  * full_hier_st4.npz, full_hier_st4_3.npz: K = 256, 2 hidden, scale_tensor [1/9, 4] and [1/8, 1/2, 4] -- checksums of
    the seeded tensors, y and checksums of the gradients on 2048 rows, fp32 and fp64;
  * psnr_hier.npz: the drivers' Adam + LambdaLR loop with config MscaleHier_ST4_LR8e3_E4000 on a 64 x 64 crop of the
    reference's parrot image for NITERS epochs, once with the scalar rate 8e-3 (``Adam(model.parameters())``: the heads
    never move) and once with the list [6e-3, 2e-2] of MscaleHier_ST4_LR2e2_2_E4000 (a group per stage and per head):
    fp32 and fp64 loss trajectories, the final PSNR, checksums of the heads before and after.
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
from modules import bspline_mscale_hier as mh, utils  # noqa: E402  (the reference's own modules)

torch.set_num_threads(int(os.environ.get("GOLDEN_THREADS", "8")))
NITERS = 100
IMAGE = "data_noisy/parrot_noisy_T30.0_snr2.png"
ST4 = [1 / 9, 4.0]
ST4_3 = [1 / 8, 1 / 2, 4.0]


def checksum(a):
    a = np.asarray(a).astype(np.float64).ravel()
    w = np.cos(np.arange(a.size) * 0.37) + 0.5
    return np.array([a.sum(), np.abs(a).sum(), (a * w).sum()], np.float64)


def build(D, hf, L, O, st, seed=0):
    ones = torch.ones
    torch.ones = lambda *a, **k: ones(*a, **{q: v for q, v in k.items() if q != "device"})
    try:
        torch.manual_seed(seed)
        return mh.INR(D, hf, 0, L, O, True, -0.2, -0.2, 0.0, st)
    finally:
        torch.ones = ones


def to_dtype(model, dt):
    model.to(dt)
    model.linears = [lin.to(dt) for lin in model.linears]
    return model


def head_items(model):
    for s, lin in enumerate(model.linears):
        yield f"linears.{s}.weight", lin.weight
        yield f"linears.{s}.bias", lin.bias


def run(model, x, t, dtype):
    m = to_dtype(model, dtype)
    m.zero_grad()
    for lin in m.linears:
        lin.zero_grad()
    xt = torch.tensor(x, dtype=dtype)[None].requires_grad_(True)
    y = m(xt)[0]
    loss = ((y - torch.tensor(t, dtype=dtype)) ** 2).mean()
    loss.backward()
    g = {k: p.grad.detach().numpy().copy() for k, p in m.named_parameters() if p.grad is not None}
    g.update({k: p.grad.detach().numpy().copy() for k, p in head_items(m)})
    out = y.detach().numpy().copy(), float(loss.item()), g, xt.grad[0].numpy().copy()
    to_dtype(model, torch.float32)
    return out


def meta(D, hf, L, O, st, seed):
    return dict(meta_D=np.int64(D), meta_hidden_features=np.int64(hf), meta_L=np.int64(L), meta_O=np.int64(O),
                meta_scale0=np.float64(0.0), meta_scale_tensor=np.array(st, np.float32).astype(np.float64),
                meta_seed=np.int64(seed))


def small():
    D, hf, L, O, st = 2, 32, 2, 3, [0.5, 0.25, 2.0]
    model = build(D, hf, L, O, st)
    rng = np.random.default_rng(1)
    x = rng.uniform(-1, 1, (300, D)).astype(np.float32)
    t = rng.uniform(0, 1, (300, O)).astype(np.float32)
    rec = meta(D, hf, L, O, st, 0)
    sd = model.state_dict()
    rec["sd_keys"] = np.array(list(sd.keys()))
    for k, v in sd.items():
        rec["sd__" + k] = v.numpy().copy()
    for k, v in head_items(model):
        rec["head__" + k] = v.detach().numpy().copy()
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
    np.savez_compressed(os.path.join(OUT, "small_hier.npz"), **rec)


def full(name, st, seed):
    D, hf, L, O = 2, 256, 2, 3
    model = build(D, hf, L, O, st)
    rng = np.random.default_rng(seed)
    x = rng.uniform(-1, 1, (2048, D)).astype(np.float32)
    t = rng.uniform(0, 1, (2048, O)).astype(np.float32)
    rec = meta(D, hf, L, O, st, 0)
    for k, v in model.state_dict().items():
        rec["sd0_checksum__" + k] = checksum(v.numpy())
    for k, v in head_items(model):
        rec["head0_checksum__" + k] = checksum(v.detach().numpy())
    rec["coords"], rec["target"] = x, t
    for tag, dt in (("32", torch.float32), ("64", torch.float64)):
        y, loss, g, gx = run(model, x, t, dt)
        rec["y" + tag], rec["loss" + tag] = y, np.float64(loss)
        rec["gcoords_checksum" + tag] = checksum(gx)
        for k, v in g.items():
            rec[f"g{tag}_checksum__{k}"] = checksum(v)
    np.savez_compressed(os.path.join(OUT, name + ".npz"), **rec)


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
    hf, L, st, maxpoints = 256, 2, ST4, 256 * 256
    res = {}
    perms = []
    for mode, lr in (("scalar", 8e-3), ("list", [6e-3, 2e-2])):
        for tag, dt in (("", torch.float32), ("64", torch.float64)):
            model = to_dtype(build(2, hf, L, 3, st), dt)
            if mode == "scalar" and not tag:
                sd0 = {k: v.detach().clone() for k, v in model.state_dict().items()}
                h0 = {k: v.detach().clone() for k, v in head_items(model)}
            f = min(1, maxpoints / (H * W))
            if isinstance(lr, list):          # the drivers' groups: a stage and its head share a rate
                groups = []
                for i, stage in enumerate(model.stages):
                    groups.append({"params": stage.parameters(), "lr": lr[i] * f})
                    groups.append({"params": model.linears[i].parameters(), "lr": lr[i] * f})
                optim = torch.optim.Adam(groups)
            else:
                optim = torch.optim.Adam(lr=lr * f, params=model.parameters())
            sched = torch.optim.lr_scheduler.LambdaLR(optim, lambda e: 0.1 ** min(e / NITERS, 1))
            c, g = coords.to(dt), gt.to(dt)
            rec = torch.zeros_like(g)
            losses = []
            for epoch in range(NITERS):
                if len(perms) <= epoch:
                    perms.append(torch.randperm(H * W))
                indices = perms[epoch]
                for b_idx in range(0, H * W, maxpoints):
                    b = indices[b_idx:min(H * W, b_idx + maxpoints)]
                    pix = model(c[:, b, ...])
                    with torch.no_grad():
                        rec[:, b, :] = pix
                    loss = ((pix - g[:, b, :]) ** 2).mean()
                    optim.zero_grad()
                    for lin in model.linears:
                        lin.zero_grad()
                    loss.backward()
                    optim.step()
                    losses.append(float(loss.item()))
                sched.step()
            key = f"{mode}{tag}"
            res["losses_" + key] = np.array(losses)
            res["psnr_" + key] = np.float64(utils.psnr(im, rec[0].reshape(H, W, 3).double().numpy()))
            for k, v in head_items(model):
                res[f"head_end_checksum_{key}__{k}"] = checksum(v.detach().double().numpy())
            print(f"hier {key}: psnr {float(res['psnr_' + key]):.4f} dB, final loss {losses[-1]:.6f}", flush=True)
    np.savez_compressed(os.path.join(OUT, "psnr_hier.npz"), image_u8=u8, niters=np.int64(NITERS),
                        maxpoints=np.int64(maxpoints), seed=np.int64(0), lr_scalar=np.float64(8e-3),
                        lr_list=np.array([6e-3, 2e-2], np.float64), hidden_features=np.int64(hf),
                        hidden_layers=np.int64(L), scale=np.float64(0.0), scale_tensor=np.array(st, np.float64),
                        perm_first8=np.stack([p[:8].numpy() for p in perms]),
                        **{"sd0_checksum__" + k: checksum(v.numpy()) for k, v in sd0.items()},
                        **{"head0_checksum__" + k: checksum(v.numpy()) for k, v in h0.items()}, **res)


if __name__ == "__main__":
    small()
    full("full_hier_st4", ST4, 2)
    full("full_hier_st4_3", ST4_3, 3)
    psnr_loop()
