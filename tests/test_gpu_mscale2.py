"""bspline_mscale_2 (modules/bspline_mscale_2.py) on the MI355X against the fp64 closed form (tests/mscale2_ref.py).

Every comparison follows err_build <= 2 err_ref + 1e-6 (tests/_util.within_ref), err_ref being the reference's own fp32
arithmetic (lin / s, four squared relus, autograd of them) against fp64 on the same inputs.  The combiner's last bias is
the mean of dL/dy and is held to the forward-propagated bound (final_bias_within_ref).
"""
import ctypes as C
import os

import numpy as np
import pytest
import torch

import mscale2_ref as mr
from _util import (GOLDEN, checksum, final_bias_within_ref, load_golden, relmax, tune, within_ref, _coords,
                   _grid_coords, _prof, _sd, _target)

pytestmark = pytest.mark.gpu
DEV = torch.device("cuda:0")
ST = {2: [1 / 9, 4.0], 3: [1 / 9, 4.0, 8.0]}
# default: the whole-net forward per pass (inference) and the data-gradient chain per pass (training); then the
# layer-by-layer route on 2 x fp16 (no whole-net kernel), and on 3 x bf16
ROUTES = {"fused": {}, "layerwise": {"fused_fwd": 0, "fused_bwd": 0}, "x3": {"split_f16": 0}}
LAST_BIAS = "combine_scales.freq_mlp.2.bias"


def _model(st, K=256, hl=2, seed=0):
    from wire_amd.modules import models
    torch.manual_seed(seed)
    return models.get_INR(nonlin="bspline_mscale_2", in_features=2, out_features=3, hidden_features=K,
                          scaled_hidden_features=0, hidden_layers=hl, first_omega_0=-0.2, hidden_omega_0=-0.2,
                          scale=0.0, scale_tensor=torch.tensor(st).to(DEV)).to(DEV)


def _check_grads(tag, got, r32, r64, n):
    """got: state_dict key -> gradient (numpy)."""
    err_y = relmax(r32[0], r64[0])
    for k, g in got.items():
        if k == LAST_BIAS:
            final_bias_within_ref(g, r64[2][k], err_y, np.abs(r64[0]).max(), 3, f"{tag} {k}",
                                  resid_max=np.abs(r64[0] - r64[4]).max())
        else:
            within_ref(relmax(g, r64[2][k]), relmax(r32[2][k], r64[2][k]), f"{tag} {k}")


_ORACLE = {}


def _oracle(S, n, grid=False):
    key = (S, n, grid)
    if key not in _ORACLE:
        sd = _sd(_model(ST[S]))
        x = _grid_coords(256, n // 256) if grid else _coords(n)
        t = _target(n)
        r32 = mr.loss_and_grads(sd, 2, x, t, ST[S], np.float32)
        r64 = mr.loss_and_grads(sd, 2, x.astype(np.float64), t.astype(np.float64), ST[S], np.float64)
        _ORACLE[key] = (x, t, r32 + (t,), r64 + (t,))
    return _ORACLE[key]


def _autograd(model, x, t, want_x=True):
    xt = torch.tensor(x, device=DEV, requires_grad=want_x)
    y = model(xt[None])[0]
    loss = ((y - torch.tensor(t, device=DEV)) ** 2).mean()
    loss.backward()
    return y.detach().cpu().numpy(), loss.item(), xt.grad


# ---- 1. the small net of the fixtures: forward, every gradient, the coordinates' -------------------------------------
def test_small_against_reference():
    rec = load_golden("small_mscale2")
    from wire_amd.modules import models
    torch.manual_seed(0)
    st = [float(v) for v in rec["meta_scale_tensor"]]
    model = models.get_INR("bspline_mscale_2", 2, 32, 0, 2, 3, True, -0.2, -0.2, 0.0, torch.tensor(st)).to(DEV)
    sd = _sd(model)
    x, t = rec["coords"], rec["target"]
    r32 = mr.loss_and_grads(sd, 2, x, t, st, np.float32) + (t,)
    r64 = mr.loss_and_grads(sd, 2, x.astype(np.float64), t.astype(np.float64), st, np.float64) + (t,)
    np.testing.assert_allclose(r64[0], rec["y64"], rtol=1e-10, atol=1e-12)
    y, loss, gx = _autograd(model, x, t)
    within_ref(relmax(y, r64[0]), relmax(r32[0], r64[0]), "m2 small y")
    within_ref(relmax(gx.cpu().numpy(), r64[3]), relmax(r32[3], r64[3]), "m2 small g_coords")
    got = {k: p.grad.cpu().numpy() for k, p in model.named_parameters() if p.grad is not None}
    assert sorted(got) == sorted(str(k) for k in rec["grad_keys64"])
    _check_grads("m2 small", got, r32, r64, x.shape[0])
    cs = model.combine_scales
    assert cs.scale_weights.grad is None and all(p.grad is None for p in cs.refine.parameters())


# ---- 2. the config shape, every route --------------------------------------------------------------------------------
@pytest.mark.parametrize("S", [2, 3])
@pytest.mark.parametrize("route", list(ROUTES))
def test_config_shape(S, route):
    n = 65536
    x, t, r32, r64 = _oracle(S, n)
    tag = f"m2 S={S} {route}"
    with tune(**ROUTES[route]):
        model = _model(ST[S])
        with torch.no_grad():
            y = model(torch.tensor(x, device=DEV)[None])[0].cpu().numpy()
        within_ref(relmax(y, r64[0]), relmax(r32[0], r64[0]), f"{tag} inference y")
        y, loss, gx = _autograd(model, x, t)
    within_ref(relmax(y, r64[0]), relmax(r32[0], r64[0]), f"{tag} autograd y")
    within_ref(abs(loss - r64[1]) / r64[1], abs(r32[1] - r64[1]) / r64[1], f"{tag} loss")
    within_ref(relmax(gx.cpu().numpy(), r64[3]), relmax(r32[3], r64[3]), f"{tag} g_coords")
    _check_grads(tag, {k: p.grad.cpu().numpy() for k, p in model.named_parameters() if p.grad is not None}, r32, r64, n)
    cs = model.combine_scales
    assert cs.scale_weights.grad is None and all(p.grad is None for p in cs.refine.parameters())


# ---- 3. the trainer: step / step_downsampled agree with autograd, twice the same bits ---------------------------------
@pytest.mark.parametrize("S", [2, 3])
def test_trainer_step(S):
    from wire_amd.trainer import FusedTrainer
    H, W = 256, 256
    n = H * W
    x, t, r32, r64 = _oracle(S, n, grid=True)
    model = _model(ST[S])
    names = [k for k, p in model.named_parameters() if any(p is q for q in model.param_tensors())]
    frozen = {k: p.detach().clone() for k, p in model.named_parameters() if k.startswith(("combine_scales.scale_w",
                                                                                          "combine_scales.refine"))}
    tr = FusedTrainer(model, (H, W), torch.tensor(t), lr=1e-3, niters=100)
    lt = tr.step(torch.arange(n, dtype=torch.int64, device=DEV))
    torch.cuda.synchronize()
    tag = f"m2 S={S} trainer"
    loss0, g0 = float(lt.item()), tr.gbuf[0]
    within_ref(abs(loss0 - r64[1]) / r64[1], abs(r32[1] - r64[1]) / r64[1], f"{tag} loss")
    got = {k: g0[off:off + sz].cpu().numpy().reshape(r64[2][k].shape) for k, off, sz in zip(names, tr.offsets, tr.sizes)}
    _check_grads(tag, got, r32, r64, n)
    for k, v in frozen.items():
        assert torch.equal(dict(model.named_parameters())[k].detach(), v), k


@pytest.mark.parametrize("S", [2, 3])
def test_trainer_bit_identical_and_downsampled(S):
    """The same step twice from the same state gives the same bits; step_downsampled with scale 1 is the MSE over the
    whole grid in raster order -- the same gradients as step() over arange(n), bit for bit."""
    from wire_amd.trainer import FusedTrainer
    H, W = 128, 128
    n = H * W
    t = torch.tensor(_target(n))
    grads = []
    for way in ("step", "step", "down"):
        model = _model(ST[S])
        tr = FusedTrainer(model, (H, W), t, lr=1e-3, niters=100)
        if way == "step":
            tr.step(torch.arange(n, dtype=torch.int64, device=DEV))
        else:
            tr.step_downsampled(t.to(DEV).contiguous(), 1)
        torch.cuda.synchronize()
        grads.append((tr.gbuf[0][:tr.count].clone(), tr.flat.clone()))
    assert torch.equal(grads[0][0], grads[1][0]) and torch.equal(grads[0][1], grads[1][1])
    # the autograd path computes the same function through the same kernels (its combiner reads g_y instead of forming it)
    d = (grads[2][0] - grads[0][0]).abs().max().item() / grads[0][0].abs().max().item()
    assert d < 1e-5, d


def test_trainer_render_and_hashed():
    from wire_amd.trainer import FusedTrainer
    H, W = 128, 128
    n = H * W
    model = _model(ST[2])
    x = _grid_coords(H, W)
    with torch.no_grad():
        y = model(torch.tensor(x, device=DEV)).cpu().numpy()
    tr = FusedTrainer(model, (H, W), torch.tensor(_target(n)), lr=1e-3, niters=100)
    r = tr.render().cpu().numpy()
    assert np.array_equal(r, y)
    l0 = tr.step_hashed(0, 0, n)
    assert np.isfinite(float(l0.item()))


# ---- 4. what runs ---------------------------------------------------------------------------------------------------
def _kernel_names(fn):
    from torch.profiler import ProfilerActivity, profile
    fn()
    torch.cuda.synchronize()
    with profile(activities=[ProfilerActivity.CUDA]) as prof:
        fn()
        torch.cuda.synchronize()
    return [e.name for e in prof.events()]


@pytest.mark.parametrize("S", [2, 3])
def test_fused_route_runs(S):
    """The default route: one whole-net forward per pass at inference, one data-gradient chain per pass in training;
    with the knobs off, neither."""
    from wire_amd.trainer import FusedTrainer
    n = 65536
    model = _model(ST[S])
    x = torch.tensor(_coords(n), device=DEV)
    tr = FusedTrainer(model, (256, 256), torch.tensor(_target(n)), lr=1e-3, niters=100)
    idx = torch.arange(n, dtype=torch.int64, device=DEV)
    for knobs, on in (({}, True), (ROUTES["layerwise"], False)):
        with tune(**knobs):
            with torch.no_grad():
                names = _kernel_names(lambda: model(x))
            assert sum("fused_fwd_kernel" in k for k in names) == (S if on else 0), sorted(set(names))
            names = _kernel_names(lambda: tr.step(idx))
            assert sum("fused_bwd_kernel" in k for k in names) == (S if on else 0), sorted(set(names))


def test_weight_gradient_launches_do_not_grow_with_passes():
    from wire_amd.trainer import FusedTrainer
    n = 65536
    t = torch.tensor(_target(n))
    idx = torch.arange(n, dtype=torch.int64, device=DEV)
    counts = {}
    for S in (2, 3):
        tr = FusedTrainer(_model(ST[S]), (256, 256), t, lr=1e-3, niters=100)
        tr.step(idx)
        counts[S] = _prof(lambda: tr.step(idx))
    assert counts[2][2] == counts[3][2] == 2, counts            # one per hidden layer, over all passes' rows
    assert counts[2][0] == 2 * 2 and counts[3][0] == 3 * 2, counts   # forward GEMMs: per pass


def test_hooked_call_announces_every_tensor_once():
    from wire_amd import _lib
    from wire_amd.trainer import FusedTrainer
    H = W = 128
    n = H * W
    model = _model(ST[3])
    tr = FusedTrainer(model, (H, W), torch.tensor(_target(n)), lr=1e-3, niters=100)
    L, d = _lib.lib(), C.byref(tr.desc)
    stream = torch.cuda.current_stream(DEV).cuda_stream
    coords = torch.tensor(_grid_coords(H, W), device=DEV)
    _lib.check(L.wire_pack_params(stream, d, tr.param_ptrs, tr.packed.data_ptr()), "pack")
    ab = _lib.check(L.wire_act_bytes(d, n, 1))
    sb = _lib.check(L.wire_bwd_scratch_bytes(d, n))
    act = torch.empty(ab, dtype=torch.uint8, device=DEV)
    scr = torch.empty(sb, dtype=torch.uint8, device=DEV)
    y, gy = (torch.empty(n, 3, device=DEV) for _ in range(2))
    loss, part = torch.empty(1, device=DEV), torch.empty(4096, device=DEV)
    seen = []
    cb = _lib.GRAD_READY_FN(lambda user, first, cnt: seen.append((first, cnt)))
    _lib.check(L.wire_train_fwd_bwd_hooked(stream, d, tr.packed.data_ptr(), coords.data_ptr(), n, tr.target.data_ptr(),
                                           None, 0, 1.0, y.data_ptr(), gy.data_ptr(), loss.data_ptr(), None,
                                           part.data_ptr(), act.data_ptr(), ab, scr.data_ptr(), sb, tr.grad_ptrs[0], cb,
                                           None), "hooked")
    torch.cuda.synchronize()
    assert seen[0] == (0, 4)
    flat = [i for f, c in seen for i in range(f, f + c)]
    assert sorted(flat) == list(range(len(tr.offsets))), seen
    assert seen == list(tr._ready_order()), seen


# ---- 5. the pieces on their own: a layer with its scale, the combiner -------------------------------------------------
def test_layer_and_combiner_calls():
    model = _model(ST[2], K=64)
    x = torch.tensor(_coords(5003), device=DEV)
    outs = []
    with torch.no_grad():
        for s in model.scale_tensor:
            h = x
            for layer in model.net[:-1]:
                h = layer(h, s)
            outs.append(model.net[-1](h))
        y = model.combine_scales(outs, 'freq_combine')
        y_whole = model(x)
    assert relmax(y.cpu().numpy(), y_whole.cpu().numpy()) < 1e-5
    # the combiner's backward against torch's own restatement on the same inputs
    ts = [o.clone().requires_grad_(True) for o in outs]
    yc = model.combine_scales(ts, 'freq_combine')
    g = torch.randn_like(yc)
    yc.backward(g)
    fm = model.combine_scales.freq_mlp
    W1, b1, W2, b2 = (p.detach().double().requires_grad_(True) for p in (fm[0].weight, fm[0].bias, fm[2].weight,
                                                                           fm[2].bias))
    td = [o.detach().double().requires_grad_(True) for o in outs]
    yd = torch.relu(torch.cat(td, -1) @ W1.T + b1) @ W2.T + b2
    yd.backward(g.double())
    assert relmax(yc.detach().cpu().numpy(), yd.detach().cpu().numpy()) < 1e-5
    for a, b in zip(ts, td):
        assert relmax(a.grad.cpu().numpy(), b.grad.cpu().numpy()) < 1e-5
    for p, q in zip((fm[0].weight, fm[0].bias, fm[2].weight, fm[2].bias), (W1, b1, W2, b2)):
        assert relmax(p.grad.cpu().numpy(), q.grad.cpu().numpy()) < 1e-5


# ---- 6. quality gate ------------------------------------------------------------------------------------------------
def test_psnr_gate():
    from oracle import wire_oracle as wo
    from wire_amd.modules import models
    from wire_amd.trainer import FusedTrainer
    z = np.load(os.path.join(GOLDEN, "psnr_mscale2.npz"), allow_pickle=False)
    u8 = z["image_u8"]
    H, W, _ = u8.shape
    im = np.divide(u8, 255, dtype=np.float32)
    niters, maxpoints = int(z["niters"]), int(z["maxpoints"])
    torch.manual_seed(int(z["seed"]))
    model = models.get_INR(nonlin="bspline_mscale_2", in_features=2, out_features=3,
                           hidden_features=int(z["hidden_features"]), scaled_hidden_features=0,
                           hidden_layers=int(z["hidden_layers"]), first_omega_0=-0.2, hidden_omega_0=-0.2,
                           scale=float(z["scale"]), scale_tensor=torch.tensor([float(v) for v in z["scale_tensor"]]))
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
    print(f"mscale_2 psnr build {psnr:.4f} dB reference {float(z['psnr']):.4f} dB (fp64 {float(z['psnr64']):.4f}); "
          f"loss drift vs fp64 build {np.max(np.abs(losses - l64) / l64):.2e} reference "
          f"{np.max(np.abs(ref - l64) / l64):.2e}")
    assert abs(psnr - float(z["psnr"])) < 0.15
    within_ref(np.max(np.abs(losses - l64) / l64), np.max(np.abs(ref - l64) / l64), "mscale_2 psnr loop loss drift")


# ---- 7. load_state_dict -----------------------------------------------------------------------------------------------
def test_load_state_dict_round_trip():
    n = 8192
    x = torch.tensor(_coords(n), device=DEV)
    a, b = _model(ST[2], seed=0), _model(ST[2], seed=5)
    with torch.no_grad():
        ya = a(x)
        assert not torch.equal(ya, b(x))
        b.load_state_dict(a.state_dict())
        assert torch.equal(ya, b(x))
    for (ka, va), (kb, vb) in zip(a.state_dict().items(), b.state_dict().items()):
        assert ka == kb and torch.equal(va, vb)
