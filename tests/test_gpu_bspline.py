"""bspline_form (modules/bspline_form.py) on the MI355X against the fp64 closed form (tests/bspline_ref.py).

Every comparison follows err_build <= 2 err_ref + 1e-6 (tests/_util.within_ref), err_ref being the reference's own fp32
arithmetic (lin / s, four squared relus, autograd of them) against fp64 on the same inputs.  Knob changes sit inside
``tune(...)``.
"""
import os

import numpy as np
import pytest
import torch

import bspline_ref as br
from _util import GOLDEN, checksum, params_np, tune, within_ref, _coords, _errs, _grid_coords, _prof, _target

pytestmark = pytest.mark.gpu
DEV = torch.device("cuda:0")


def _model(D, hf, L, O, s, seed=0, outermost_linear=True, kind="bspline_form"):
    from wire_amd.modules import models
    torch.manual_seed(seed)
    return models.get_INR(nonlin=kind, in_features=D, out_features=O, hidden_features=hf, hidden_layers=L,
                          outermost_linear=outermost_linear, scale=s).to(DEV)


# ---- 1. one layer ---------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("n", [3001, 70001])
@pytest.mark.parametrize("fin,fout", [(2, 256), (256, 256), (256, 250)])
@pytest.mark.parametrize("s", [1 / 9, 1 / 4, 1.0, 15.0])
def test_layer_fwd_bwd(n, fin, fout, s):
    from wire_amd.modules.bspline_form import Bsplines_form
    torch.manual_seed(5)
    layer = Bsplines_form(fin, fout, sigma0=s).to(DEV)
    x = np.random.default_rng(7).uniform(-1, 1, (n, fin)).astype(np.float32)
    gw = np.random.default_rng(8).standard_normal((n, fout)).astype(np.float32)
    xt = torch.tensor(x, device=DEV, requires_grad=True)
    out = layer(xt)
    (out * torch.tensor(gw, device=DEV)).sum().backward()
    W, b = layer.linear.weight.detach().cpu().numpy(), layer.linear.bias.detach().cpu().numpy()
    res = {}
    for dt in (np.float32, np.float64):
        y, cache = br.forward([(W, b)], None, x, s, dt, keep=True)
        gl, _, gx = br.backward([(W, b)], None, cache, gw, s, dt)
        res[dt] = (y, gx, gl[0][0], gl[0][1])
    tag = f"bspline layer {fin}->{fout} n={n} s={s:.4g}"
    got = (out, xt.grad, layer.linear.weight.grad, layer.linear.bias.grad)
    for name, g, a32, a64 in zip(("fwd", "g_x", "g_W", "g_b"), got, res[np.float32], res[np.float64]):
        _errs(f"{tag} {name}", g.detach().cpu().numpy(), a32, a64)


# ---- 2. whole-net forward -------------------------------------------------------------------------------------------
def _oracle_y(model, L, x, s, outermost_linear=True):
    sd = params_np(model)
    layers, final = br.net_from_state(sd, L, outermost_linear)
    return br.forward(layers, final, x, s, np.float32), br.forward(layers, final, x, s, np.float64)


@pytest.mark.parametrize("L", [1, 2, 3, 4])
@pytest.mark.parametrize("K", [256, 250, 128])
def test_net_forward(L, K):
    s = 1 / 4
    model = _model(2, K, L, 3, s)
    x = _coords(8229, 2)
    y32, y64 = _oracle_y(model, L, x, s)
    with torch.no_grad():
        y = model(torch.tensor(x, device=DEV)).cpu().numpy()
        with tune(fused_fwd=0):
            y_l = model(torch.tensor(x, device=DEV)).cpu().numpy()
    _errs(f"bspline net fwd L={L} K={K} default", y, y32, y64)
    _errs(f"bspline net fwd L={L} K={K} fused_fwd=0", y_l, y32, y64)


def test_inference_launch_counts_equal_gauss():
    x = torch.tensor(_coords(65536, 2), device=DEV)
    counts = {}
    for kind, s in (("bspline_form", 0.25), ("gauss", 10.0)):
        m = _model(2, 256, 4, 3, s, kind=kind)
        with torch.no_grad():
            m(x)
            counts[kind] = _prof(lambda: m(x))
    assert counts["bspline_form"] == counts["gauss"], counts
    assert sum(counts["bspline_form"]) >= 1


# ---- 3. training step -----------------------------------------------------------------------------------------------
SHAPES = {"cfg_2x256": (2, 1 / 9, 65536), "4x256": (4, 1 / 4, 262144)}
KNOBS = [{}, {"fused_rstore": 0}, {"fused_bwd": 0}, {"fused_train": 0}, {"wgrad_batch": 0}, {"split_out": 0},
         {"split_f16": 0}, {"split_bf16": 0}]
_ORACLE = {}


def _oracle_step(shape):
    if shape not in _ORACLE:
        L, s, n = SHAPES[shape]
        model = _model(2, 256, L, 3, s)
        sd = params_np(model)
        H = 256
        W = n // H
        x, t = _grid_coords(H, W), _target(n, 3)
        r32 = br.loss_and_grads(sd, L, x, t, s, np.float32)
        r64 = br.loss_and_grads(sd, L, x.astype(np.float64), t.astype(np.float64), s, np.float64)
        _ORACLE[shape] = (x, t, r32, r64, (H, W))
    return _ORACLE[shape]


@pytest.mark.parametrize("shape", list(SHAPES))
@pytest.mark.parametrize("knobs", KNOBS, ids=lambda k: ",".join(f"{a}={b}" for a, b in k.items()) or "default")
def test_training_step(shape, knobs):
    from wire_amd.trainer import FusedTrainer
    L, s, n = SHAPES[shape]
    x, t, r32, r64, (H, W) = _oracle_step(shape)
    tag = f"bspline step {shape} {knobs or 'default'}"
    with tune(**knobs):
        # autograd path: model(coords) + MSE backward
        model = _model(2, 256, L, 3, s)
        y = model(torch.tensor(x, device=DEV))
        loss = ((y - torch.tensor(t, device=DEV)) ** 2).mean()
        loss.backward()
        _errs(f"{tag} autograd y", y.detach().cpu().numpy(), r32[0], r64[0])
        within_ref(abs(loss.item() - r64[1]) / r64[1], abs(r32[1] - r64[1]) / r64[1], f"{tag} autograd loss")
        for k, p in model.named_parameters():
            if p.grad is not None:
                _errs(f"{tag} autograd {k}", p.grad.cpu().numpy(), r32[2][k], r64[2][k])
        # FusedTrainer: one step over every grid point in order
        model = _model(2, 256, L, 3, s)
        names = [k for k, p in model.named_parameters() if p.requires_grad]
        tr = FusedTrainer(model, (H, W), torch.tensor(t), lr=1e-3, niters=100)
        lt = tr.step(torch.arange(n, dtype=torch.int64, device=DEV))
        torch.cuda.synchronize()
        within_ref(abs(float(lt.item()) - r64[1]) / r64[1], abs(r32[1] - r64[1]) / r64[1], f"{tag} trainer loss")
        g = tr.gbuf[0]
        for k, off, sz in zip(names, tr.offsets, tr.sizes):
            _errs(f"{tag} trainer {k}", g[off:off + sz].cpu().numpy().reshape(r64[2][k].shape), r32[2][k], r64[2][k])


@pytest.mark.parametrize("shape", list(SHAPES))
def test_training_step_launch_counts_equal_gauss(shape):
    from wire_amd.trainer import FusedTrainer
    L, s, n = SHAPES[shape]
    H, W = 256, n // 256
    t = torch.tensor(_target(n, 3))
    idx = torch.arange(n, dtype=torch.int64, device=DEV)
    counts = {}
    for kind, sc in (("bspline_form", s), ("gauss", 10.0)):
        tr = FusedTrainer(_model(2, 256, L, 3, sc, kind=kind), (H, W), t, lr=1e-3, niters=100)
        tr.step(idx)
        counts[kind] = _prof(lambda: tr.step(idx))
    assert counts["bspline_form"] == counts["gauss"], counts


# ---- 4. outermost_linear=False ----------------------------------------------------------------------------------------
def test_outermost_activation_layerwise():
    L, s, n = 2, 0.25, 5003
    model = _model(2, 256, L, 3, s, outermost_linear=False)
    sd = params_np(model)
    x, t = _coords(n, 2), _target(n, 3)
    r32 = br.loss_and_grads(sd, L, x, t, s, np.float32, outermost_linear=False)
    r64 = br.loss_and_grads(sd, L, x.astype(np.float64), t.astype(np.float64), s, np.float64, outermost_linear=False)
    y = model(torch.tensor(x, device=DEV))
    ((y - torch.tensor(t, device=DEV)) ** 2).mean().backward()
    _errs("bspline outermost_linear=False y", y.detach().cpu().numpy(), r32[0], r64[0])
    for k, p in model.named_parameters():
        if p.grad is not None:
            _errs(f"bspline outermost_linear=False {k}", p.grad.cpu().numpy(), r32[2][k], r64[2][k])


# ---- 5. coordinate gradients ------------------------------------------------------------------------------------------
@pytest.mark.parametrize("outermost_linear", [True, False])
def test_coordinate_gradients(outermost_linear):
    L, s, n = 2, 0.25, 9001
    model = _model(2, 256, L, 3, s, outermost_linear=outermost_linear)
    layers, final = br.net_from_state(params_np(model), L, outermost_linear)
    x = _coords(n, 2)
    gw = np.random.default_rng(9).standard_normal((n, 3)).astype(np.float32)
    xt = torch.tensor(x, device=DEV, requires_grad=True)
    (model(xt) * torch.tensor(gw, device=DEV)).sum().backward()
    gx = {}
    for dt in (np.float32, np.float64):
        _, cache = br.forward(layers, final, x, s, dt, keep=True)
        gx[dt] = br.backward(layers, final, cache, gw, s, dt)[2]
    _errs(f"bspline coords grad outermost_linear={outermost_linear}", xt.grad.cpu().numpy(), gx[np.float32],
          gx[np.float64])


# ---- 7. quality gate ------------------------------------------------------------------------------------------------
def test_psnr_gate():
    from oracle import wire_oracle as wo
    from wire_amd.trainer import FusedTrainer
    z = np.load(os.path.join(GOLDEN, "psnr_bspline_s9.npz"), allow_pickle=False)
    u8 = z["image_u8"]
    H, W, _ = u8.shape
    im = np.divide(u8, 255, dtype=np.float32)
    niters, maxpoints = int(z["niters"]), int(z["maxpoints"])
    torch.manual_seed(int(z["seed"]))
    from wire_amd.modules import models
    model = models.get_INR(nonlin="bspline_form", in_features=2, out_features=3, hidden_features=int(z["hidden_features"]),
                           scaled_hidden_features=0, hidden_layers=int(z["hidden_layers"]), first_omega_0=-0.2,
                           hidden_omega_0=-0.2, scale=float(z["scale"]), scale_tensor=[0.0])
    for k, v in model.state_dict().items():
        np.testing.assert_allclose(checksum(v.numpy()), z["sd0_checksum__" + k], rtol=1e-12, atol=1e-12)
    model = model.to(DEV)
    lr0 = float(z["lr"]) * min(1, maxpoints / (H * W))
    tr = FusedTrainer(model, (H, W), torch.tensor(im).reshape(H * W, 3), lr=lr0, niters=niters, keep_rec=True)
    losses = []
    for epoch in range(niters):
        indices = torch.randperm(H * W)
        assert np.array_equal(indices[:8].numpy(), z["perm_first8"][epoch])
        idx = indices.to(DEV)
        for b in range(0, H * W, maxpoints):
            losses.append(tr.step(idx[b:min(H * W, b + maxpoints)].contiguous()))
        tr.scheduler_step()
    torch.cuda.synchronize()
    losses = np.array([float(x.item()) for x in losses])
    psnr = wo.psnr(im, tr.rec.cpu().numpy().reshape(H, W, 3))
    ref, l64 = z["losses"], z["losses64"]
    print(f"bspline psnr build {psnr:.4f} dB reference {float(z['psnr']):.4f} dB; loss drift vs fp64 "
          f"build {np.max(np.abs(losses - l64) / l64):.2e} reference {np.max(np.abs(ref - l64) / l64):.2e}")
    assert abs(psnr - float(z["psnr"])) < 0.1
    assert np.all(np.abs(losses - ref) <= 1e-3 * ref)


# ---- 8. scale_0 from a state_dict -----------------------------------------------------------------------------------
def test_load_state_dict_scale():
    L, n = 2, 8192
    model = _model(2, 256, L, 3, 1 / 9)
    sd = model.state_dict()
    for k in sd:
        if k.endswith("scale_0"):
            sd[k] = torch.full((1,), 0.3)
    model.load_state_dict(sd)
    x = _coords(n, 2)
    y32, y64 = _oracle_y(model, L, x, np.float32(0.3))
    with torch.no_grad():
        y = model(torch.tensor(x, device=DEV)).cpu().numpy()
    _errs("bspline load_state_dict scale_0=0.3", y, y32, y64)
