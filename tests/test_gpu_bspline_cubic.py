"""bspline_cubic (modules/bspline_cubic.py) on the MI355X against the fp64 piecewise closed form (tests/bspline_cubic_ref.py).

Every comparison follows err_build <= 2 err_ref + 1e-6 (tests/_util.within_ref) against the fp64 oracle.  err_ref is the
error of the PIECEWISE closed form evaluated in numpy fp32 against fp64 on the same inputs -- an independent restatement,
and the tighter yardstick by two to three orders of magnitude at the class's scale of 15, where the reference's own five
cubed relus cancel from |lin|^3 and are wrong in the third digit.  The five-term fp32 error is logged next to each
comparison (a second line of the ratio log, "[five-term fp32, logged only]"), never asserted against.

Shapes: 4096 rows is where make_route switches to the 16 x 16 x 32 GEMM family, a workgroup is 128 rows (8229 = 64
workgroups + 37 rows), P = 256 is the only width the whole-net kernels take for real nets.  gemmx2_tn_splits gives one
split per 256 rows (at least 256 rows per split, chunks rounded up to 64 rows): 33 splits at the 8245 rows of the
97 x 85 grid, so the cross-split reduce runs behind the cubic loader in every training case here.  Knob changes sit inside
``tune(...)``.
"""
import os

import numpy as np
import pytest
import torch

import bspline_cubic_ref as bc
from _util import (GOLDEN, RATIO_LOG, abi_train_step, checksum, params_np, relmax, tune, within_ref, _coords,
                   _grid_coords, _prof, _target)
from test_gpu_bspline import KNOBS

pytestmark = pytest.mark.gpu
DEV = torch.device("cuda:0")


def _model(D, hf, L, O, s, seed=0, outermost_linear=True):
    from wire_amd.modules import bspline_cubic
    torch.manual_seed(seed)
    return bspline_cubic.INR(D, hf, L, 0, O, outermost_linear, -0.2, -0.2, s).to(DEV)


def _errs3(label, got, p32, f32, r64):
    """The parity bound against the piecewise fp32 yardstick; the five-term fp32 error is logged beside it."""
    got = np.asarray(got)
    eb = relmax(got, r64)
    RATIO_LOG.append((label + " [five-term fp32, logged only]", float(eb), float(relmax(f32, r64))))
    within_ref(eb, relmax(p32, r64), label)


def _loss3(label, got, p32, f32, r64):
    RATIO_LOG.append((label + " [five-term fp32, logged only]", abs(got - r64) / r64, abs(f32 - r64) / r64))
    within_ref(abs(got - r64) / r64, abs(p32 - r64) / r64, label)


def _three(fn):
    """fn(dtype, form) for the piecewise fp32 yardstick, the five-term fp32 arithmetic and the fp64 oracle."""
    return fn(np.float32, "piecewise"), fn(np.float32, "five"), fn(np.float64, "piecewise")


def _oracle_step(sd, L, x, t, s, outermost_linear=True):
    return _three(lambda dt, form: bc.loss_and_grads(sd, L, x.astype(dt), t.astype(dt), s, dt, outermost_linear,
                                                     form=form))


def _check_step(tag, y, loss, grads, ora):
    """y, the MSE loss and every parameter gradient of one step, each against the fp64 oracle."""
    p32, f32, r64 = ora
    if y is not None:
        _errs3(f"{tag} y", y, p32[0], f32[0], r64[0])
    _loss3(f"{tag} loss", loss, p32[1], f32[1], r64[1])
    assert sorted(grads) == sorted(r64[2])
    for k, g in grads.items():
        _errs3(f"{tag} {k}", np.asarray(g).reshape(r64[2][k].shape), p32[2][k], f32[2][k], r64[2][k])


# ---- 1. one layer ---------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("bias_x3", [False, True], ids=["bias", "bias_x3"])
@pytest.mark.parametrize("n", [3001, 8229])
@pytest.mark.parametrize("fin,fout", [(2, 256), (256, 256), (256, 250)])
@pytest.mark.parametrize("s", [1.0, 4.0, 15.0, -4.0])
def test_layer_fwd_bwd(n, fin, fout, s, bias_x3):
    from wire_amd.modules.bspline_cubic import Bsplines_cubic
    torch.manual_seed(5)
    layer = Bsplines_cubic(fin, fout, sigma0=s).to(DEV)
    if bias_x3:                        # a bias the scale must not touch: 3 b moves lin by up to 3 / sqrt(fin)
        with torch.no_grad():
            layer.linear.bias.mul_(3.0)
    x = np.random.default_rng(7).uniform(-1, 1, (n, fin)).astype(np.float32)
    gw = np.random.default_rng(8).standard_normal((n, fout)).astype(np.float32)
    xt = torch.tensor(x, device=DEV, requires_grad=True)
    out = layer(xt)
    (out * torch.tensor(gw, device=DEV)).sum().backward()
    W, b = layer.linear.weight.detach().cpu().numpy(), layer.linear.bias.detach().cpu().numpy()

    def run(dt, form):
        y, cache = bc.forward([(W, b)], None, x, s, dt, keep=True, form=form)
        gl, _, gx = bc.backward([(W, b)], None, cache, gw, s, dt, form=form)
        return y, gx, gl[0][0], gl[0][1]
    p32, f32, r64 = _three(run)
    tag = f"cubic layer {fin}->{fout} n={n} s={s:g}{' 3b' if bias_x3 else ''}"
    got = (out, xt.grad, layer.linear.weight.grad, layer.linear.bias.grad)
    for i, name in enumerate(("fwd", "g_x", "g_W", "g_b")):
        _errs3(f"{tag} {name}", got[i].detach().cpu().numpy(), p32[i], f32[i], r64[i])


# ---- 2. whole-net forward -------------------------------------------------------------------------------------------
def _oracle_y(model, L, x, s, outermost_linear=True):
    layers, final = bc.net_from_state(params_np(model), L, outermost_linear)
    return _three(lambda dt, form: bc.forward(layers, final, x, s, dt, form=form))


def _forward_case(L, K, s, n, tag):
    model = _model(2, K, L, 3, s)
    x = _coords(n, 2)
    ora = _oracle_y(model, L, x, s)
    with torch.no_grad():
        y = model(torch.tensor(x, device=DEV)).cpu().numpy()
        with tune(fused_fwd=0):
            y_l = model(torch.tensor(x, device=DEV)).cpu().numpy()
    _errs3(f"cubic net fwd {tag} default", y, *ora)
    _errs3(f"cubic net fwd {tag} fused_fwd=0", y_l, *ora)


@pytest.mark.parametrize("L", [1, 2, 4])
@pytest.mark.parametrize("K", [256, 250, 128])
def test_net_forward(L, K):
    _forward_case(L, K, 15.0, 8229, f"L={L} K={K} s=15")


def test_net_forward_no_hidden_layer():
    _forward_case(0, 256, 15.0, 3001, "L=0 K=256 s=15 n=3001")


def test_net_forward_negative_scale():
    _forward_case(2, 256, -4.0, 8229, "L=2 K=256 s=-4")


# ---- 3. training step -----------------------------------------------------------------------------------------------
SHAPES = {"2x256_s15": (2, 15.0, (97, 85)), "4x256_s4": (4, 4.0, (97, 85)), "2x256_s15_small": (2, 15.0, (61, 49))}
_ORACLE = {}


def _oracle_shape(shape):
    if shape not in _ORACLE:
        L, s, (H, W) = SHAPES[shape]
        sd = params_np(_model(2, 256, L, 3, s))
        x, t = _grid_coords(H, W), _target(H * W, 3)
        _ORACLE[shape] = (x, t, _oracle_step(sd, L, x, t, s))
    return _ORACLE[shape]


def _training_case(shape, knobs):
    from wire_amd.trainer import FusedTrainer
    L, s, (H, W) = SHAPES[shape]
    n = H * W
    x, t, ora = _oracle_shape(shape)
    tag = f"cubic step {shape} {knobs or 'default'}"
    with tune(**knobs):
        # autograd path: model(coords) + MSE backward
        model = _model(2, 256, L, 3, s)
        y = model(torch.tensor(x, device=DEV))
        loss = ((y - torch.tensor(t, device=DEV)) ** 2).mean()
        loss.backward()
        _check_step(f"{tag} autograd", y.detach().cpu().numpy(), loss.item(),
                    {k: p.grad.cpu().numpy() for k, p in model.named_parameters() if p.grad is not None}, ora)
        # FusedTrainer: one step over every grid point in order
        model = _model(2, 256, L, 3, s)
        names = [k for k, p in model.named_parameters() if p.requires_grad]
        tr = FusedTrainer(model, (H, W), torch.tensor(t), lr=1e-3, niters=100)
        lt = tr.step(torch.arange(n, dtype=torch.int64, device=DEV))
        torch.cuda.synchronize()
        g = tr.gbuf[0]
        _check_step(f"{tag} trainer", None, float(lt.item()),
                    {k: g[off:off + sz].cpu().numpy() for k, off, sz in zip(names, tr.offsets, tr.sizes)}, ora)


@pytest.mark.parametrize("knobs", KNOBS, ids=lambda k: ",".join(f"{a}={b}" for a, b in k.items()) or "default")
def test_training_step(knobs):
    _training_case("2x256_s15", knobs)


@pytest.mark.parametrize("shape", ["4x256_s4", "2x256_s15_small"])
def test_training_step_other_shapes(shape):
    _training_case(shape, {})


# ---- 4. route -------------------------------------------------------------------------------------------------------
def _form_model(L, s):
    from wire_amd.modules import models
    torch.manual_seed(0)
    return models.get_INR(nonlin="bspline_form", in_features=2, out_features=3, hidden_features=256, hidden_layers=L,
                          scale=s).to(DEV)


def test_inference_launch_counts_equal_bspline_form():
    x = torch.tensor(_coords(8229, 2), device=DEV)
    counts = {}
    for kind, m in (("bspline_cubic", _model(2, 256, 2, 3, 15.0)), ("bspline_form", _form_model(2, 1 / 9))):
        with torch.no_grad():
            m(x)
            counts[kind] = _prof(lambda: m(x))
    assert counts["bspline_cubic"] == counts["bspline_form"], counts
    assert sum(counts["bspline_cubic"]) >= 1


def test_training_step_launch_counts_equal_bspline_form():
    from wire_amd.trainer import FusedTrainer
    H, W = 97, 85
    t = torch.tensor(_target(H * W, 3))
    idx = torch.arange(H * W, dtype=torch.int64, device=DEV)
    counts = {}
    for kind, m in (("bspline_cubic", _model(2, 256, 2, 3, 15.0)), ("bspline_form", _form_model(2, 1 / 9))):
        tr = FusedTrainer(m, (H, W), t, lr=1e-3, niters=100)
        tr.step(idx)
        counts[kind] = _prof(lambda: tr.step(idx))
    assert counts["bspline_cubic"] == counts["bspline_form"], counts
    assert sum(counts["bspline_cubic"]) >= 1


# ---- 5. outermost_linear=False ----------------------------------------------------------------------------------------
def test_outermost_activation_layerwise():
    L, s, n = 2, 15.0, 5003
    model = _model(2, 256, L, 3, s, outermost_linear=False)
    x, t = _coords(n, 2), _target(n, 3)
    ora = _oracle_step(params_np(model), L, x, t, s, outermost_linear=False)
    y = model(torch.tensor(x, device=DEV))
    loss = ((y - torch.tensor(t, device=DEV)) ** 2).mean()
    loss.backward()
    _check_step("cubic outermost_linear=False", y.detach().cpu().numpy(), loss.item(),
                {k: p.grad.cpu().numpy() for k, p in model.named_parameters() if p.grad is not None}, ora)


# ---- 6. coordinate gradients ------------------------------------------------------------------------------------------
def _coords_grad_oracle(model, L, x, gw, s, outermost_linear=True):
    layers, final = bc.net_from_state(params_np(model), L, outermost_linear)

    def run(dt, form):
        _, cache = bc.forward(layers, final, x, s, dt, keep=True, form=form)
        return bc.backward(layers, final, cache, gw, s, dt, form=form)[2]
    return _three(run)


@pytest.mark.parametrize("outermost_linear", [True, False])
def test_coordinate_gradients(outermost_linear):
    L, s, n = 2, 15.0, 9001
    model = _model(2, 256, L, 3, s, outermost_linear=outermost_linear)
    x = _coords(n, 2)
    gw = np.random.default_rng(9).standard_normal((n, 3)).astype(np.float32)
    xt = torch.tensor(x, device=DEV, requires_grad=True)
    (model(xt) * torch.tensor(gw, device=DEV)).sum().backward()
    _errs3(f"cubic coords grad outermost_linear={outermost_linear}", xt.grad.cpu().numpy(),
           *_coords_grad_oracle(model, L, x, gw, s, outermost_linear))


# ---- 7. width envelope ------------------------------------------------------------------------------------------------
ENVELOPE = [(1, 2), (3, 1), (4, 5), (4, 8)]
_ENV = {}


def _envelope(D, O):
    if (D, O) not in _ENV:
        L, s, n = 2, 15.0, 4099
        sd = params_np(_model(D, 250, L, O, s))
        x, t = _coords(n, D), _target(n, O)
        _ENV[(D, O)] = (L, s, x, t, _oracle_step(sd, L, x, t, s))
    return _ENV[(D, O)]


@pytest.mark.parametrize("D,O", ENVELOPE)
def test_envelope_training_call(D, O):
    L, s, x, t, ora = _envelope(D, O)
    res = abi_train_step(_model(D, 250, L, O, s), x, t)
    assert np.isfinite(res["y"]).all() and all(np.isfinite(g).all() for g in res["grads"].values())
    _check_step(f"cubic envelope D={D} O={O} training call", res["y"], res["loss"], res["grads"], ora)
    np.testing.assert_array_equal(res["rec"], res["y"])


@pytest.mark.parametrize("D,O", ENVELOPE)
def test_envelope_autograd_with_coordinate_gradients(D, O):
    L, s, x, t, ora = _envelope(D, O)
    model = _model(D, 250, L, O, s)
    xt = torch.tensor(x, device=DEV, requires_grad=True)
    y = model(xt)
    loss = ((y - torch.tensor(t, device=DEV)) ** 2).mean()
    loss.backward()
    tag = f"cubic envelope D={D} O={O} autograd"
    _check_step(tag, y.detach().cpu().numpy(), loss.item(),
                {k: p.grad.cpu().numpy() for k, p in model.named_parameters() if p.grad is not None}, ora)
    gy = (2.0 / t.size) * (ora[2][0] - t.astype(np.float64))          # dL/dy of the fp64 oracle: one upstream for all
    _errs3(f"{tag} g_coords", xt.grad.cpu().numpy(), *_coords_grad_oracle(model, L, x, gy, s))


@pytest.mark.parametrize("D,O", ENVELOPE)
def test_envelope_inference(D, O):
    L, s, x, t, ora = _envelope(D, O)
    model = _model(D, 250, L, O, s)
    with torch.no_grad():
        y = model(torch.tensor(x, device=DEV)).cpu().numpy()
    _errs3(f"cubic envelope D={D} O={O} inference", y, ora[0][0], ora[1][0], ora[2][0])


def test_trainer_step_on_a_3d_grid():
    from wire_amd.modules.utils import axis_tables
    from wire_amd.trainer import FusedTrainer
    H, W, T, L, s = 13, 11, 29, 2, 15.0
    n = H * W * T
    tx, ty, tz = (a.numpy() for a in axis_tables(H, W, T, style="torch"))
    i, j, k = np.unravel_index(np.arange(n), (H, W, T))                # flat index = (i W + j) T + k -> (tx[j], ty[i], tz[k])
    x = np.stack([tx[j], ty[i], tz[k]], 1).astype(np.float32)
    t = _target(n, 1)
    model = _model(3, 256, L, 1, s)
    ora = _oracle_step(params_np(model), L, x, t, s)
    names = [k_ for k_, p in model.named_parameters() if p.requires_grad]
    tr = FusedTrainer(model, (H, W, T), torch.tensor(t), lr=1e-3, niters=100)
    lt = tr.step(torch.arange(n, dtype=torch.int64, device=DEV))
    torch.cuda.synchronize()
    g = tr.gbuf[0]
    _check_step("cubic trainer 3-D grid (13, 11, 29) D=3 O=1", None, float(lt.item()),
                {k_: g[off:off + sz].cpu().numpy() for k_, off, sz in zip(names, tr.offsets, tr.sizes)}, ora)


# ---- 8. state and render ----------------------------------------------------------------------------------------------
def test_load_state_dict_scale_reaches_the_kernels():
    L, n = 2, 8192
    model = _model(2, 256, L, 3, 15.0)
    sd = model.state_dict()
    for k in sd:
        if k.endswith("scale_0"):
            sd[k] = torch.full((1,), 0.3)
    model.load_state_dict(sd)
    x = _coords(n, 2)
    with torch.no_grad():
        y = model(torch.tensor(x, device=DEV)).cpu().numpy()
    _errs3("cubic load_state_dict scale_0=0.3", y, *_oracle_y(model, L, x, np.float32(0.3)))


def test_render_equals_forward():
    from wire_amd.trainer import FusedTrainer
    H, W, L, s = 97, 85, 2, 15.0
    model = _model(2, 256, L, 3, s)
    x = _grid_coords(H, W)
    ora = _oracle_y(model, L, x, s)
    tr = FusedTrainer(model, (H, W), torch.tensor(_target(H * W, 3)), lr=1e-3, niters=100)
    img = tr.render().cpu().numpy()
    with torch.no_grad():
        y = model(torch.tensor(x, device=DEV)).cpu().numpy()
    _errs3("cubic FusedTrainer.render", img, *ora)
    _errs3("cubic model(coords) behind FusedTrainer", y, *ora)
    within_ref(relmax(img, y), 2 * relmax(ora[0], ora[2]), "cubic render against model(coords)", factor=1.0)


# ---- 9. quality gate ------------------------------------------------------------------------------------------------
def test_psnr_gate():
    """150 Adam steps of the reference's loop on the 64 x 64 parrot crop (2 x 256, scale 15, one 4096-row batch per epoch).
    The build's largest relative loss deviation from the reference's DOUBLE trajectory must not exceed the reference's own
    fp32 deviation from it (factor 1, no floor), and the final PSNR must lie within 0.1 dB of the double run's."""
    from oracle import wire_oracle as wo
    from wire_amd.modules import bspline_cubic
    from wire_amd.trainer import FusedTrainer
    z = np.load(os.path.join(GOLDEN, "psnr_bspline_cubic.npz"), allow_pickle=False)
    u8 = np.load(os.path.join(GOLDEN, "psnr_bspline_s9.npz"), allow_pickle=False)["image_u8"]
    H, W, _ = u8.shape
    im = np.divide(u8, 255, dtype=np.float32)
    niters, maxpoints = int(z["niters"]), int(z["maxpoints"])
    torch.manual_seed(int(z["seed"]))
    model = bspline_cubic.INR(2, int(z["hidden_features"]), int(z["hidden_layers"]), 0, 3, True, -0.2, -0.2,
                              float(z["scale"]))
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
    dev_build, dev_ref = np.max(np.abs(losses - l64) / l64), np.max(np.abs(ref - l64) / l64)
    print(f"bspline_cubic psnr build {psnr:.4f} dB, reference fp32 {float(z['psnr']):.4f} dB, double "
          f"{float(z['psnr64']):.4f} dB; largest loss deviation from the double trajectory: build {dev_build:.2e}, "
          f"reference fp32 {dev_ref:.2e}")
    RATIO_LOG.append(("cubic psnr gate: loss deviation from the double trajectory (bound: factor 1, no floor)",
                      float(dev_build), float(dev_ref)))
    assert dev_build <= dev_ref
    assert abs(psnr - float(z["psnr64"])) < 0.1
