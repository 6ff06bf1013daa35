"""The multiplicative filter network (wire_amd.modules.mfn, WIRE_KIND_MFN) on the MI355X against the fp64 closed form
(tests/mfn_ref.py).

Every comparison follows err_build <= 2 err_ref + 1e-6 (tests/_util.within_ref), err_ref being the reference's own fp32
arithmetic (the expanded norm, exp, sin and autograd of them, as mfn_ref evaluates it in float32) against fp64 on the
same inputs.  Knob changes sit inside ``tune(...)``.
"""
import ctypes as C
import os

import numpy as np
import pytest
import torch

import mfn_ref as mr
from _util import GOLDEN, params_np, tune, within_ref, _coords, _errs, _grid_coords, _target

pytestmark = pytest.mark.gpu
DEV = torch.device("cuda:0")


def _model(D, K, L, O, seed=0):
    from wire_amd.modules import mfn
    torch.manual_seed(seed)
    return mfn.INR(D, K, L, O).to(DEV)


def _fwd(model, x):
    return model(torch.tensor(x, device=DEV)[None])[0]


# ---- 1. one filter layer --------------------------------------------------------------------------------------------
@pytest.mark.parametrize("n", [3001, 70001])
@pytest.mark.parametrize("D,K", [(2, 256), (3, 256), (2, 250)])
def test_filter_fwd_bwd(n, D, K):
    from wire_amd.modules.mfn import GaborLayer
    torch.manual_seed(5)
    layer = GaborLayer(D, K, 0, alpha=6.0 / 3).to(DEV)      # gamma and w as the constructor draws them (k = 3)
    x = np.random.default_rng(7).uniform(-1, 1, (n, D)).astype(np.float32)
    gw = np.random.default_rng(8).standard_normal((n, K)).astype(np.float32)
    xt = torch.tensor(x, device=DEV, requires_grad=True)
    out = layer(xt)
    (out * torch.tensor(gw, device=DEV)).sum().backward()
    f = tuple(t.detach().cpu().numpy() for t in layer.abi_tensors())
    res = {dt: (mr.filter_fwd(x, f, dt),) + mr.filter_bwd(x, f, gw, dt) for dt in (np.float32, np.float64)}
    got = (out, layer.mu.grad, layer.gamma.grad, layer.linear.weight.grad, layer.linear.bias.grad, xt.grad)
    for name, g, a32, a64 in zip(("fwd", "g_mu", "g_gamma", "g_w", "g_c", "g_x"), got, res[np.float32], res[np.float64]):
        _errs(f"mfn filter {D}->{K} n={n} {name}", g.detach().cpu().numpy(), a32, a64)


# ---- 2. whole-net forward -------------------------------------------------------------------------------------------
@pytest.mark.parametrize("n", [8229, 65536])
@pytest.mark.parametrize("L", [0, 1, 2, 4])
@pytest.mark.parametrize("K", [256, 250, 128])
def test_net_forward(L, K, n):
    model = _model(2, K, L, 3)
    fl, ln = mr.net_from_state(params_np(model), L)
    x = _coords(n, 2)
    y32, y64 = mr.forward(fl, ln, x, np.float32), mr.forward(fl, ln, x, np.float64)
    with torch.no_grad():
        y = _fwd(model, x).cpu().numpy()
        with tune(fused_fwd=0):
            y_l = _fwd(model, x).cpu().numpy()
    _errs(f"mfn net fwd L={L} K={K} n={n}", y, y32, y64)
    assert np.array_equal(y, y_l), "fused_fwd must not change a filter network's forward"
    # the forward that saves for the backward computes the same function
    _errs(f"mfn net fwd(save) L={L} K={K} n={n}", _fwd(model, x).detach().cpu().numpy(), y32, y64)


# ---- 3. training step -----------------------------------------------------------------------------------------------
SHAPES = {"2x256": (2, 65536), "4x256": (4, 262144)}
KNOBS = [{}, {"fused_rstore": 0}, {"fused_bwd": 0}, {"fused_train": 0}, {"wgrad_batch": 0}, {"split_out": 0},
         {"split_f16": 0}, {"split_bf16": 0}]          # = tests/test_gpu_bspline.py::KNOBS
FAMILY_KNOBS = ("split_f16", "split_bf16")
_ORACLE, _DEFAULT = {}, {}


def _oracle_step(shape):
    if shape not in _ORACLE:
        L, n = SHAPES[shape]
        sd = params_np(_model(2, 256, L, 3))
        H = 256
        W = n // H
        x, t = _grid_coords(H, W), _target(n, 3)
        r32 = mr.loss_and_grads(sd, L, x, t, np.float32)
        r64 = mr.loss_and_grads(sd, L, x.astype(np.float64), t.astype(np.float64), np.float64)
        _ORACLE[shape] = (x, t, r32, r64, (H, W))
    return _ORACLE[shape]


def _run_step(shape, knobs):
    """(autograd y, loss, grads), (trainer loss, flat gradient) under the knobs"""
    from wire_amd.trainer import FusedTrainer
    L, n = SHAPES[shape]
    x, t, _, _, (H, W) = _oracle_step(shape)
    with tune(**knobs):
        model = _model(2, 256, L, 3)
        y = _fwd(model, x)
        loss = ((y - torch.tensor(t, device=DEV)) ** 2).mean()
        loss.backward()
        auto = (y.detach().cpu().numpy(), loss.item(), {k: p.grad.cpu().numpy() for k, p in model.named_parameters()})
        model = _model(2, 256, L, 3)
        names = [k for k, _ in model.named_parameters()]
        tr = FusedTrainer(model, (H, W), torch.tensor(t), lr=1e-3, niters=100)
        lt = tr.step(torch.arange(n, dtype=torch.int64, device=DEV))
        torch.cuda.synchronize()
        g = tr.gbuf[0]
        flat = {k: g[off:off + sz].cpu().numpy() for k, off, sz in zip(names, tr.offsets, tr.sizes)}
    return auto, (float(lt.item()), flat)


@pytest.mark.parametrize("shape", list(SHAPES))
@pytest.mark.parametrize("knobs", KNOBS, ids=lambda k: ",".join(f"{a}={b}" for a, b in k.items()) or "default")
def test_training_step(shape, knobs):
    x, t, r32, r64, _ = _oracle_step(shape)
    tag = f"mfn step {shape} {knobs or 'default'}"
    (y, loss, grads), (lt, flat) = _run_step(shape, knobs)
    _errs(f"{tag} autograd y", y, r32[0], r64[0])
    within_ref(abs(loss - r64[1]) / r64[1], abs(r32[1] - r64[1]) / r64[1], f"{tag} autograd loss")
    within_ref(abs(lt - r64[1]) / r64[1], abs(r32[1] - r64[1]) / r64[1], f"{tag} trainer loss")
    assert set(grads) == set(r64[2]) == set(flat)
    for k in r64[2]:
        _errs(f"{tag} autograd {k}", grads[k], r32[2][k], r64[2][k])
        _errs(f"{tag} trainer {k}", flat[k].reshape(r64[2][k].shape), r32[2][k], r64[2][k])
    if not knobs:
        _DEFAULT[shape] = ((y, loss, grads), (lt, flat))
    elif not any(k in FAMILY_KNOBS for k in knobs):
        # the fused-path knobs are routed around: bit-identical to the default
        if shape not in _DEFAULT:
            _DEFAULT[shape] = _run_step(shape, {})
        (y0, l0, g0), (lt0, f0) = _DEFAULT[shape]
        assert np.array_equal(y, y0) and loss == l0 and lt == lt0, tag
        for k in g0:
            assert np.array_equal(grads[k], g0[k]) and np.array_equal(flat[k], f0[k]), f"{tag} {k}"


# ---- 4. coordinate gradients ----------------------------------------------------------------------------------------
@pytest.mark.parametrize("L,D", [(0, 2), (2, 2), (2, 3)])
def test_coords_grad(L, D):
    n = 9001
    model = _model(D, 256, L, 3)
    sd = params_np(model)
    x, gy = _coords(n, D), np.random.default_rng(3).standard_normal((n, 3)).astype(np.float32)
    xt = torch.tensor(x, device=DEV)[None].requires_grad_(True)
    y = model(xt)
    (y[0] * torch.tensor(gy, device=DEV)).sum().backward()
    r32 = mr.loss_and_grads(sd, L, x, None, np.float32, g_y=gy)
    r64 = mr.loss_and_grads(sd, L, x.astype(np.float64), None, np.float64, g_y=gy)
    _errs(f"mfn g_coords L={L} D={D}", xt.grad[0].cpu().numpy(), r32[3], r64[3])
    for k, p in model.named_parameters():
        _errs(f"mfn g_coords L={L} D={D} {k}", p.grad.cpu().numpy(), r32[2][k], r64[2][k])
    # the coordinate gradient alone (frozen parameters)
    for p in model.parameters():
        p.requires_grad_(False)
    xt2 = torch.tensor(x, device=DEV)[None].requires_grad_(True)
    (model(xt2)[0] * torch.tensor(gy, device=DEV)).sum().backward()
    assert torch.equal(xt2.grad, xt.grad)


# ---- 5. the hooked call, 6. determinism -----------------------------------------------------------------------------
def _train_call(model, n, hooked, seed=4):
    from wire_amd import _lib
    L = _lib.lib()
    desc = model.net_desc()
    dp = C.byref(desc)
    params = [p.detach().contiguous() for p in model.param_tensors()]
    f32 = dict(dtype=torch.float32, device=DEV)
    packed = torch.empty(L.wire_packed_floats(dp), **f32)
    st = torch.cuda.current_stream().cuda_stream
    _lib.check(L.wire_pack_params(st, dp, _lib.ptr_array([p.data_ptr() for p in params]), packed.data_ptr()))
    x = torch.tensor(_coords(n, 2, seed), device=DEV)
    t = torch.tensor(_target(n, 3, seed + 1), device=DEV)
    ab, sb = L.wire_act_bytes(dp, n, 1), L.wire_bwd_scratch_bytes(dp, n)
    act, scr = torch.empty(ab, dtype=torch.uint8, device=DEV), torch.empty(sb, dtype=torch.uint8, device=DEV)
    y, gy = torch.empty(n, 3, **f32), torch.empty(n, 3, **f32)
    loss, part = torch.zeros(1, **f32), torch.empty(4096, **f32)
    grads = [torch.full_like(p, float("nan")) for p in params]
    gp = _lib.ptr_array([g.data_ptr() for g in grads])
    seen = []
    cb = _lib.GRAD_READY_FN(lambda user, first, cnt: seen.append((first, cnt)))
    args = (st, dp, packed.data_ptr(), x.data_ptr(), n, t.data_ptr(), None, 0, 1.0, y.data_ptr(), gy.data_ptr(),
            loss.data_ptr(), None, part.data_ptr(), act.data_ptr(), ab, scr.data_ptr(), sb, gp)
    if hooked:
        _lib.check(L.wire_train_fwd_bwd_hooked(*args, cb, None), "hooked")
    else:
        _lib.check(L.wire_train_fwd_bwd(*args), "train")
    torch.cuda.synchronize()
    return [g.cpu().numpy() for g in grads], loss.item(), seen


@pytest.mark.parametrize("L,n", [(0, 5000), (2, 65536), (3, 3000)])
def test_hooked_order_and_determinism(L, n):
    model = _model(2, 256, L, 3)
    g0, l0, _ = _train_call(model, n, False)
    g1, l1, seen = _train_call(model, n, True)
    g2, l2, _ = _train_call(model, n, False)
    nt = 4 * (L + 1) + 2 * L + 2
    want = [(nt - 2, 2)]
    for i in range(L - 1, -1, -1):
        want += [(4 * (L + 1) + 2 * i, 2), (4 * (i + 1), 4)]
    want += [(0, 4)]
    assert seen == want
    assert sorted(t for f, c in seen for t in range(f, f + c)) == list(range(nt))
    assert l0 == l1 == l2
    for a, b, c in zip(g0, g1, g2):
        assert np.isfinite(a).all()
        assert np.array_equal(a, b), "the hooked call's gradients differ from the plain call's"
        assert np.array_equal(a, c), "two runs of the same step differ"


def test_trainer_steps_and_render():
    """FusedTrainer end to end: a few Adam steps lower the loss, render / flat_grad / step_hashed work, mu and gamma move."""
    from wire_amd.trainer import FusedTrainer
    H = W = 64
    model = _model(2, 128, 2, 3)
    t = torch.tensor(_target(H * W, 3))
    tr = FusedTrainer(model, (H, W), t, lr=1e-2, niters=50)
    before = [p.detach().clone() for p in model.param_tensors()]
    idx = torch.arange(H * W, dtype=torch.int64, device=DEV)
    losses = [float(tr.step(idx).item()) for _ in range(20)]
    assert losses[-1] < losses[0]
    assert all(not torch.equal(a, b) for a, b in zip(before, model.param_tensors()))
    img = tr.render()
    with torch.no_grad():
        y = _fwd(model, _grid_coords(H, W))
    assert torch.equal(img.reshape(-1, 3), y.reshape(-1, 3))
    assert tr.flat_grad.numel() >= sum(p.numel() for p in model.parameters())


# ---- 7. quality gate ------------------------------------------------------------------------------------------------
def test_psnr_gate():
    """The reference's loop (tests/golden/make_mfn_golden.py) through FusedTrainer: same init, same permutations.  PSNR
    within 0.1 dB of the reference's; loss drift against the fp64 trajectory within 2 x the fp32 reference's own + 1e-6."""
    from wire_amd.modules import mfn
    from wire_amd.trainer import FusedTrainer
    rec = np.load(os.path.join(GOLDEN, "psnr_mfn.npz"))
    u8 = rec["image_u8"]
    H, W, _ = u8.shape
    im = np.divide(u8, 255, dtype=np.float32)
    niters, maxpoints = int(rec["niters"]), int(rec["maxpoints"])
    torch.manual_seed(int(rec["seed"]))
    model = mfn.INR(2, int(rec["hidden_features"]), int(rec["hidden_layers"]), 3)
    perms = [torch.randperm(H * W) for _ in range(niters)]
    assert np.array_equal(np.stack([p[:8].numpy() for p in perms]), rec["perm_first8"])
    model = model.to(DEV)
    tr = FusedTrainer(model, (H, W), torch.tensor(im).reshape(H * W, 3), lr=float(rec["lr"]) * min(1, maxpoints / (H * W)),
                      gamma=0.1, niters=niters, keep_rec=True)
    losses = []
    for epoch in range(niters):
        losses.append(float(tr.step(perms[epoch].to(DEV)).item()))
        tr.scheduler_step()
    l64, l32 = rec["losses64"], rec["losses"]
    drift = float(np.max(np.abs(np.array(losses) - l64) / l64))
    drift_ref = float(np.max(np.abs(l32 - l64) / l64))
    img = tr.rec.reshape(H, W, 3).double().cpu().numpy()
    psnr = 10 * np.log10(im.max() / np.mean((im.astype(np.float64) - img) ** 2))
    print(f"mfn psnr {psnr:.4f} dB (reference {float(rec['psnr']):.4f}), drift {drift:.3e} (reference fp32 {drift_ref:.3e})")
    assert abs(psnr - float(rec["psnr"])) <= 0.1
    within_ref(drift, drift_ref, "mfn loss drift over the run")
