"""bspline_mscale_hier (modules/bspline_mscale_hier.py) on the MI355X against the fp64 closed form (tests/hier_ref.py).

Every comparison follows err_build <= 2 err_ref + 1e-6 (tests/_util.within_ref), err_ref being the reference's own fp32
arithmetic (lin / s, four squared relus, autograd of them) against fp64 on the same inputs.  Every head's bias gradient
is the mean of dL/dy and is held to the forward-propagated bound (final_bias_within_ref), as the final bias of the
other nets is.
"""
import ctypes as C
import os

import numpy as np
import pytest
import torch

import hier_ref as hr
from _util import (GOLDEN, checksum, final_bias_within_ref, load_golden, relmax, tune, within_ref, _coords,
                   _grid_coords, _prof, _sd, _target)

pytestmark = pytest.mark.gpu
DEV = torch.device("cuda:0")
ST = {1: [0.5], 2: [1 / 9, 4.0], 3: [1 / 8, 1 / 2, 4.0]}
ROUTES = {"x2": {}, "x3": {"split_f16": 0}, "fp32": {"split_bf16": 0}}


def _model(st, K=256, hl=2, seed=0):
    from wire_amd.modules import models
    torch.manual_seed(seed)
    return models.get_INR(nonlin="bspline_mscale_hier", in_features=2, out_features=3, hidden_features=K,
                          scaled_hidden_features=0, hidden_layers=hl, first_omega_0=-0.2, hidden_omega_0=-0.2,
                          scale=0.0, scale_tensor=st).to(DEV)


def _heads(model):
    out = {}
    for s, lin in enumerate(model.linears):
        out[f"linears.{s}.weight"], out[f"linears.{s}.bias"] = lin.weight.detach().cpu().numpy(), lin.bias.detach().cpu().numpy()
    return out


def _both(model, L, x, t, st):
    sd, hd = _sd(model), _heads(model)
    r32 = hr.loss_and_grads(sd, hd, L, x, t, st, np.float32)
    r64 = hr.loss_and_grads(sd, hd, L, x.astype(np.float64), t.astype(np.float64), st, np.float64)
    return r32, r64


def _check_grads(tag, got, r32, r64, t):
    """got: key -> gradient (numpy), stages by state_dict key, heads by "linears.{s}.*".  Nothing is left out."""
    assert sorted(got) == sorted(r64[2]), (sorted(got), sorted(r64[2]))
    err_y = relmax(r32[0], r64[0])
    for k, g in got.items():
        print(f"{tag} {k}: build {relmax(g, r64[2][k]):.3e} reference {relmax(r32[2][k], r64[2][k]):.3e}")
        if k.startswith("linears.") and k.endswith(".bias"):
            final_bias_within_ref(g, r64[2][k], err_y, np.abs(r64[0]).max(), 3, f"{tag} {k}",
                                  resid_max=np.abs(r64[0] - t).max())
        else:
            within_ref(relmax(g, r64[2][k]), relmax(r32[2][k], r64[2][k]), f"{tag} {k}")


def _autograd(model, x, t):
    xt = torch.tensor(x, device=DEV, requires_grad=True)
    y = model(xt[None])[0]
    loss = ((y - torch.tensor(t, device=DEV)) ** 2).mean()
    loss.backward()
    got = {k: p.grad.cpu().numpy() for k, p in model.named_parameters() if p.grad is not None}
    for s, lin in enumerate(model.linears):
        got[f"linears.{s}.weight"], got[f"linears.{s}.bias"] = lin.weight.grad.cpu().numpy(), lin.bias.grad.cpu().numpy()
    return y.detach().cpu().numpy(), loss.item(), xt.grad.cpu().numpy(), got


def _whole(tag, model, L, x, t, st):
    r32, r64 = _both(model, L, x, t, st)
    with torch.no_grad():
        y = model(torch.tensor(x, device=DEV)[None])[0].cpu().numpy()
    within_ref(relmax(y, r64[0]), relmax(r32[0], r64[0]), f"{tag} inference y")
    y, loss, gx, got = _autograd(model, x, t)
    print(f"{tag} y: build {relmax(y, r64[0]):.3e} reference {relmax(r32[0], r64[0]):.3e}")
    within_ref(relmax(y, r64[0]), relmax(r32[0], r64[0]), f"{tag} autograd y")
    within_ref(abs(loss - r64[1]) / r64[1], abs(r32[1] - r64[1]) / r64[1], f"{tag} loss")
    within_ref(relmax(gx, r64[3]), relmax(r32[3], r64[3]), f"{tag} g_coords")
    _check_grads(tag, got, r32, r64, t)
    return r32, r64


# ---- 1. the small net of the fixtures -----------------------------------------------------------------------------
def test_small_against_reference():
    rec = load_golden("small_hier")
    st = [float(v) for v in rec["meta_scale_tensor"]]
    model = _model(st, K=32)
    for k, v in _heads(model).items():
        assert np.array_equal(v, rec["head__" + k]), k
    x, t = rec["coords"], rec["target"]
    r32, r64 = _whole("hier small", model, 2, x, t, st)
    np.testing.assert_allclose(r64[0], rec["y64"], rtol=1e-10, atol=1e-12)
    # the fixture's fp32 run (the reference itself) is the err_ref of record; the oracle's fp32 arithmetic restates it
    y, _, gx, got = _autograd(_model(st, K=32), x, t)
    within_ref(relmax(y, rec["y64"]), relmax(rec["y32"], rec["y64"]), "hier small y (fixture)")
    within_ref(relmax(gx, rec["gcoords64"]), relmax(rec["gcoords32"], rec["gcoords64"]), "hier small g_coords (fixture)")


# ---- 2. the config shapes on every route --------------------------------------------------------------------------
@pytest.mark.parametrize("S", [2, 3])
@pytest.mark.parametrize("route", list(ROUTES))
def test_config_shape(S, route):
    n = 65536
    x, t = _coords(n), _target(n)
    with tune(**ROUTES[route]):
        _whole(f"hier S={S} {route}", _model(ST[S]), 2, x, t, ST[S])


def test_reversed_scales():
    n = 65536
    _whole("hier [4, 1/9]", _model([4.0, 1 / 9]), 2, _coords(n), _target(n), [4.0, 1 / 9])


@pytest.mark.parametrize("route", list(ROUTES))
def test_pad_columns(route):
    """K = 250: P = 256, six pad columns in either half of the join (B(0) = 0.75 there unless masked)."""
    n = 16384
    with tune(**ROUTES[route]):
        _whole(f"hier K=250 {route}", _model(ST[3], K=250), 2, _coords(n), _target(n), ST[3])


def test_single_stage_one_hidden_layer():
    n = 8192
    _whole("hier S=1 L=1", _model(ST[1], K=128, hl=1), 1, _coords(n), _target(n), ST[1])


def test_three_hidden_layers_unused_tail():
    """L = 3: stages[s > 0][3] exists, is never run and never gets a gradient."""
    n = 8192
    model = _model(ST[2], K=64, hl=3)
    _whole("hier L=3", model, 3, _coords(n), _target(n), ST[2])
    assert model.stages[1][3].linear.weight.grad is None


# ---- 3. the trainer ---------------------------------------------------------------------------------------------------
def _trainer_case(S, lr):
    from wire_amd.trainer import FusedTrainer
    H = W = 256
    n = H * W
    x, t = _grid_coords(H, W), _target(n)
    model = _model(ST[S])
    r32, r64 = _both(model, 2, x, t, ST[S])
    sd0, hd0 = _sd(model), _heads(model)
    names = [k for k in sd0 if "scale_0" not in k] + list(hd0)
    tr = FusedTrainer(model, (H, W), torch.tensor(t), lr=lr, niters=100)
    p0 = tr.flat.clone()
    lt = tr.step(torch.arange(n, dtype=torch.int64, device=DEV))
    torch.cuda.synchronize()
    tag = f"hier S={S} trainer"
    loss0 = float(lt.item())
    within_ref(abs(loss0 - r64[1]) / r64[1], abs(r32[1] - r64[1]) / r64[1], f"{tag} loss")
    g0 = tr.flat_grad
    got = {k: g0[off:off + sz].cpu().numpy().reshape(r64[2][k].shape) for k, off, sz in zip(names, tr.offsets, tr.sizes)}
    _check_grads(tag, got, r32, r64, t)
    return tr, names, p0, got, {**sd0, **hd0}


@pytest.mark.parametrize("S", [2, 3])
def test_trainer_scalar_rate_leaves_heads(S):
    lr = 1e-3
    tr, names, p0, got, w0 = _trainer_case(S, lr)
    for k, off, sz in zip(names, tr.offsets, tr.sizes):
        new, old = tr.flat[off:off + sz], p0[off:off + sz]
        if k.startswith("linears."):
            assert torch.equal(new, old), k                       # the heads keep their bits
            continue
        g = got[k].astype(np.float64).ravel()
        want, _, _ = hr.adam_step(w0[k].astype(np.float64).ravel(), g, 0.0, 0.0, lr, 1)
        assert np.abs(new.cpu().numpy() - want).max() <= 1e-6 * max(1.0, np.abs(want).max()) + 2e-7, k
    for s, lin in enumerate(tr.model.linears):                    # the model's heads are views of the flat buffer
        assert torch.equal(lin.weight.detach().reshape(-1).cpu(), torch.tensor(w0[f"linears.{s}.weight"]).reshape(-1))


def test_trainer_rate_list_moves_heads():
    rates = [6e-3, 2e-2]
    tr, names, p0, got, w0 = _trainer_case(2, rates)
    for k, off, sz in zip(names, tr.offsets, tr.sizes):
        s = int(k.split(".")[1])
        g = got[k].astype(np.float64).ravel()
        want, _, _ = hr.adam_step(w0[k].astype(np.float64).ravel(), g, 0.0, 0.0, rates[s], 1)
        new = tr.flat[off:off + sz].cpu().numpy()
        assert np.abs(new - want).max() <= 1e-6 * max(1.0, np.abs(want).max()) + 2e-7, k
        # the first Adam step moves every element with a gradient by the stage's rate
        moved = np.abs(new - w0[k].ravel())[np.abs(g) > 1e-5]
        assert np.allclose(moved, rates[s], rtol=1e-2), (k, moved.min(), moved.max())
    from wire_amd.trainer import FusedTrainer
    with pytest.raises(ValueError):
        FusedTrainer(_model(ST[2]), (64, 64), torch.zeros(4096, 3), lr=[1e-3])
    from wire_amd.modules import models
    plain = models.get_INR("bspline_form", 2, 64, 0, 2, 3, scale=0.5).to(DEV)
    with pytest.raises(ValueError):
        FusedTrainer(plain, (64, 64), torch.zeros(4096, 3), lr=[1e-3, 1e-3])


@pytest.mark.parametrize("S", [2, 3])
def test_trainer_bit_identical_render_and_other_steps(S):
    from wire_amd.trainer import FusedTrainer
    H = W = 128
    n = H * W
    t = torch.tensor(_target(n))
    runs = []
    for way in ("step", "step", "down"):
        model = _model(ST[S])
        tr = FusedTrainer(model, (H, W), t, lr=1e-3, niters=100)
        if way == "step":
            tr.step(torch.arange(n, dtype=torch.int64, device=DEV))
        else:
            tr.step_downsampled(t.to(DEV).contiguous(), 1)
        torch.cuda.synchronize()
        runs.append((tr.flat_grad.clone(), tr.flat.clone()))
    assert torch.equal(runs[0][0], runs[1][0]) and torch.equal(runs[0][1], runs[1][1])
    # step_downsampled with scale 1 is the same loss through wire_mlp_fwd / wire_mlp_bwd
    d = (runs[2][0] - runs[0][0]).abs().max().item() / runs[0][0].abs().max().item()
    assert d < 1e-5, d
    model = _model(ST[S])
    x = _grid_coords(H, W)
    with torch.no_grad():
        y = model(torch.tensor(x, device=DEV)).cpu().numpy()
    tr = FusedTrainer(model, (H, W), t, lr=1e-3, niters=100, keep_rec=True)
    assert np.array_equal(tr.render().cpu().numpy(), y)
    assert np.isfinite(float(tr.step_hashed(0, 0, n).item()))
    p = tr.psnr(tr.rec)
    tr.update_best(tr.loss, tr.rec, force=True)
    assert np.isfinite(float(p.item())) and torch.equal(tr.best_img, tr.rec)


def test_step_radon_runs():
    from wire_amd.modules import models
    from wire_amd.trainer import FusedTrainer
    torch.manual_seed(0)
    model = models.get_INR("bspline_mscale_hier", 2, 64, 0, 2, 1, scale=0.0, scale_tensor=ST[2]).to(DEV)
    H = W = 64
    tr = FusedTrainer(model, (H, W), torch.zeros(H * W, 1), lr=1e-3, niters=100)
    th = torch.linspace(0, 180, 20)
    loss = tr.step_radon(torch.rand(20 * W, device=DEV), th)
    assert np.isfinite(float(loss.item()))


# ---- 4. what runs -----------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("hl", [2, 3])
def test_launch_counts(hl):
    """Per step at S stages, L hidden layers: forward GEMMs L + 2 (S - 1) (the join is ONE GEMM over 2K), weight-gradient
    GEMMs the same number (the join's is one launch, not one per half), data-gradient GEMMs L + 3 (S - 1) (the join's
    two halves have different epilogues).  stages[s > 0][3:] launch nothing: the counts of L = 3 exceed those of L = 2
    by stage 0's one more layer only."""
    from wire_amd.trainer import FusedTrainer
    n = 65536
    t = torch.tensor(_target(n))
    idx = torch.arange(n, dtype=torch.int64, device=DEV)
    for S in (2, 3):
        tr = FusedTrainer(_model(ST[S], hl=hl), (256, 256), t, lr=1e-3, niters=100)
        tr.step(idx)
        c = _prof(lambda: tr.step(idx))
        assert c[0] == hl + 2 * (S - 1) and c[2] == hl + 2 * (S - 1) and c[1] == hl + 3 * (S - 1), (S, hl, c)


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
    nt = len(tr.offsets)
    assert seen[0] == (nt - 6, 6)                                  # the three heads first
    flat = [i for f, c in seen for i in range(f, f + c)]
    assert sorted(flat) == list(range(nt)), seen
    assert seen == list(tr._ready_order()), seen


# ---- 5. load_state_dict -----------------------------------------------------------------------------------------------
def test_load_state_dict_round_trip_with_changed_scales():
    n = 8192
    x = torch.tensor(_coords(n), device=DEV)
    a, b = _model([0.25, 3.0], seed=0), _model(ST[2], seed=5)
    with torch.no_grad():
        ya = a(x)
        b.load_state_dict(a.state_dict())
        for s in range(2):                                         # the heads are not in the state_dict: by hand
            b.linears[s].load_state_dict(a.linears[s].state_dict())
        assert b._scales == [0.25, 3.0]
        assert torch.equal(ya, b(x))
    sd = a.state_dict()
    sd["stages.1.2.scale_0"] = sd["stages.1.2.scale_0"] * 2
    with pytest.raises(NotImplementedError, match="differ"):
        b.load_state_dict(sd)


# ---- 6. quality gates -------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("mode", ["scalar", "list"])
def test_psnr_gate(mode):
    """The criterion of tests/test_gpu_mscale2.py::test_psnr_gate: the final PSNR within 0.15 dB of the reference's fp32
    loop, the loss drift against fp64 through within_ref."""
    from oracle import wire_oracle as wo
    from wire_amd.trainer import FusedTrainer
    z = np.load(os.path.join(GOLDEN, "psnr_hier.npz"), allow_pickle=False)
    u8 = z["image_u8"]
    H, W, _ = u8.shape
    im = np.divide(u8, 255, dtype=np.float32)
    niters, maxpoints = int(z["niters"]), int(z["maxpoints"])
    model = _model([float(v) for v in z["scale_tensor"]], K=int(z["hidden_features"]), hl=int(z["hidden_layers"]),
                   seed=int(z["seed"]))
    for k, v in model.state_dict().items():
        np.testing.assert_allclose(checksum(v.cpu().numpy()), z["sd0_checksum__" + k], rtol=1e-12, atol=1e-12)
    for k, v in _heads(model).items():
        np.testing.assert_allclose(checksum(v), z["head0_checksum__" + k], rtol=1e-12, atol=1e-12)
    f = min(1, maxpoints / (H * W))
    lr = float(z["lr_scalar"]) * f if mode == "scalar" else [float(v) * f for v in z["lr_list"]]
    tr = FusedTrainer(model, (H, W), torch.tensor(im).reshape(H * W, 3), lr=lr, niters=niters, keep_rec=True)
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
    ref, l64 = z["losses_" + mode], z["losses_" + mode + "64"]
    print(f"hier {mode} psnr build {psnr:.4f} dB reference {float(z['psnr_' + mode]):.4f} dB (fp64 "
          f"{float(z['psnr_' + mode + '64']):.4f}); loss drift vs fp64 build {np.max(np.abs(losses - l64) / l64):.2e} "
          f"reference {np.max(np.abs(ref - l64) / l64):.2e}")
    for k, v in _heads(model).items():
        end, start = z[f"head_end_checksum_{mode}__{k}"], z["head0_checksum__" + k]
        if mode == "scalar":                                       # the heads never moved, here as there
            np.testing.assert_allclose(end, start, rtol=1e-12, atol=1e-12)
            np.testing.assert_allclose(checksum(v), start, rtol=1e-12, atol=1e-12)
        else:
            assert not np.allclose(checksum(v), start) and not np.allclose(end, start)
    # test_gpu_mscale2's margin is 0.15 dB; the reference's own fp32 loop sits |psnr32 - psnr64| from its fp64 loop (0.05 dB
    # with the scalar rate, 0.19 dB with the list), and a build as close to fp64 on the other side is twice that from fp32
    gap = abs(float(z["psnr_" + mode]) - float(z["psnr_" + mode + "64"]))
    assert abs(psnr - float(z["psnr_" + mode])) < max(0.15, 2 * gap)
    within_ref(np.max(np.abs(losses - l64) / l64), np.max(np.abs(ref - l64) / l64), f"hier {mode} psnr loop loss drift")
