"""bspline_mscale_HL (modules/bspline_mscale_HL.py) on the MI355X against the fp64 closed form (tests/mscale_ref.py).

Every comparison follows err_build <= 2 err_ref + 1e-6 (tests/_util.within_ref), err_ref being the reference's own fp32
arithmetic (lin / s, four squared relus, autograd of them) against fp64 on the same inputs.
"""
import os

import numpy as np
import pytest
import torch

import mscale_ref as mr
from _util import GOLDEN, checksum, within_ref, _coords, _errs, _grid_coords, _prof, _sd, _target

pytestmark = pytest.mark.gpu
DEV = torch.device("cuda:0")
# (SHF, scale_tensor, hidden scale): the configs.py shapes -- 384 in three groups, 450 in two, 130 inside the first group
NETS = {"shf384": (384, [1 / 9, 1 / 9, 4.0], 1 / 9), "shf450": (450, [1 / 12, 1 / 6], 1 / 9),
        "shf130": (130, [1.0, 2.0], 1.0)}


def _model(shf, st, s, K=256, hl=2, seed=0):
    from wire_amd.modules import models
    torch.manual_seed(seed)
    return models.get_INR(nonlin="bspline_mscale_HL", in_features=2, out_features=3, hidden_features=K,
                          scaled_hidden_features=shf, hidden_layers=hl, first_omega_0=-0.2, hidden_omega_0=-0.2,
                          scale=s, scale_tensor=torch.tensor(st).to(DEV)).to(DEV)


# ---- 1. the first stage alone: every column, across the group boundaries ---------------------------------------------
@pytest.mark.parametrize("shf,st", [(384, [1 / 9, 1 / 9, 4.0]), (450, [1 / 12, 1 / 6]), (130, [1.0, 2.0]),
                                    (320, [0.5, 0.25, 2.0]), (257, [0.3, 3.0])])
def test_first_stage(shf, st):
    from wire_amd.modules.bspline_mscale_HL import Scaled_Bsplines_form
    torch.manual_seed(4)
    layer = Scaled_Bsplines_form(2, shf, sigma0=torch.tensor(st)).to(DEV)
    n = 5003
    x = _coords(n, seed=11)
    xt = torch.tensor(x, device=DEV, requires_grad=True)
    out = layer(xt[None])
    assert out.shape == (1, n, shf) and not out.requires_grad
    W, b = layer.linear.weight.detach().cpu().numpy(), layer.linear.bias.detach().cpu().numpy()
    r32, r64 = (mr.first_stage(W, b, x, st, dt) for dt in (np.float32, np.float64))
    got = out[0].cpu().numpy()
    groups = mr.column_groups(shf, len(st))
    for g in range(len(st)):
        cols = groups == g
        if cols.any():
            _errs(f"mscale first stage SHF={shf} group {g}", got[:, cols], r32[:, cols], r64[:, cols])
    for j in [j for j in range(1, shf) if groups[j] != groups[j - 1]]:     # the columns on either side of a boundary
        _errs(f"mscale first stage SHF={shf} boundary {j}", got[:, j - 1:j + 1], r32[:, j - 1:j + 1],
              r64[:, j - 1:j + 1])


# ---- 2. forward + training step -------------------------------------------------------------------------------------
@pytest.mark.parametrize("net", list(NETS))
@pytest.mark.parametrize("n", [65536, 7777])
def test_forward_and_autograd_step(net, n):
    shf, st, s = NETS[net]
    model = _model(shf, st, s)
    sd = _sd(model)
    x, t = _coords(n), _target(n)
    r32 = mr.loss_and_grads(sd, 2, x, t, st, s, np.float32)
    r64 = mr.loss_and_grads(sd, 2, x.astype(np.float64), t.astype(np.float64), st, s, np.float64)
    tag = f"mscale {net} n={n}"
    with torch.no_grad():
        y = model(torch.tensor(x, device=DEV)[None])[0]
    _errs(f"{tag} inference y", y.cpu().numpy(), r32[0], r64[0])
    xt = torch.tensor(x, device=DEV, requires_grad=True)
    y = model(xt)
    loss = ((y - torch.tensor(t, device=DEV)) ** 2).mean()
    loss.backward()
    _errs(f"{tag} autograd y", y.detach().cpu().numpy(), r32[0], r64[0])
    within_ref(abs(loss.item() - r64[1]) / r64[1], abs(r32[1] - r64[1]) / r64[1], f"{tag} loss")
    assert model.net[0].linear.weight.grad is None and model.net[0].linear.bias.grad is None
    assert xt.grad is None
    for k, p in model.named_parameters():
        if k.startswith("net.0.") or not p.requires_grad:
            continue
        assert p.grad is not None, k
        _errs(f"{tag} autograd {k}", p.grad.cpu().numpy(), r32[2][k], r64[2][k])


@pytest.mark.parametrize("net", list(NETS))
def test_trainer_step(net):
    from wire_amd.trainer import FusedTrainer
    shf, st, s = NETS[net]
    H, W = 256, 256
    n = H * W
    model = _model(shf, st, s)
    sd = _sd(model)
    x, t = _grid_coords(H, W), _target(n)
    r32 = mr.loss_and_grads(sd, 2, x, t, st, s, np.float32)
    r64 = mr.loss_and_grads(sd, 2, x.astype(np.float64), t.astype(np.float64), st, s, np.float64)
    names = [k for k, p in model.named_parameters() if p.requires_grad]
    tr = FusedTrainer(model, (H, W), torch.tensor(t), lr=1e-3, niters=100)
    lt = tr.step(torch.arange(n, dtype=torch.int64, device=DEV))
    torch.cuda.synchronize()
    tag = f"mscale {net} trainer"
    within_ref(abs(float(lt.item()) - r64[1]) / r64[1], abs(r32[1] - r64[1]) / r64[1], f"{tag} loss")
    g = tr.gbuf[0]
    assert len(names) == len(tr.offsets)
    for k, off, sz in zip(names, tr.offsets, tr.sizes):
        got = g[off:off + sz].cpu().numpy()
        if k.startswith("net.0."):
            assert not got.any(), k            # the frozen pair: announced, never written
        else:
            _errs(f"{tag} {k}", got.reshape(r64[2][k].shape), r32[2][k], r64[2][k])


# ---- 3. what runs ---------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("hl", [2, 3])
def test_launch_counts(hl):
    """Forward GEMMs: SHF -> K and the hl - 1 hidden ones; data gradients: the hidden layers only (none for SHF -> K);
    weight-gradient GEMMs: the hidden layers' (the SHF -> K one runs in the profiled span of the first layer's parameter
    gradients, class 3, as a positional-encoding net's does) -- none for the first stage, in the autograd step and the
    trainer's.  The frozen stage itself is one kernel of class 3 in the forward."""
    from wire_amd.trainer import FusedTrainer
    n = 65536
    model = _model(384, [1 / 9, 1 / 9, 4.0], 1 / 9, hl=hl)
    x = torch.tensor(_coords(n), device=DEV)
    t = torch.tensor(_target(n), device=DEV)

    def autograd_step():
        model.zero_grad()
        ((model(x) - t) ** 2).mean().backward()
    autograd_step()
    c = _prof(autograd_step)
    assert c[:3] == [hl, hl - 1, hl - 1], c
    tr = FusedTrainer(model, (256, 256), t.cpu(), lr=1e-3, niters=100)
    idx = torch.arange(n, dtype=torch.int64, device=DEV)
    tr.step(idx)
    c = _prof(lambda: tr.step(idx))
    assert c[:3] == [hl, hl - 1, hl - 1], c


def test_shf_to_k_forward_on_2xfp16_kernel():
    """At 65 536 rows every forward GEMM of the net -- the SHF -> K one included -- is the 2 x fp16 NT kernel."""
    from torch.profiler import ProfilerActivity, profile
    model = _model(384, [1 / 9, 1 / 9, 4.0], 1 / 9)
    x = torch.tensor(_coords(65536), device=DEV)
    with torch.no_grad():
        model(x)
        torch.cuda.synchronize()
        with profile(activities=[ProfilerActivity.CUDA]) as prof:
            model(x)
            torch.cuda.synchronize()
    names = [e.name for e in prof.events()]
    assert sum("gemmx2h_nt_kernel" in k for k in names) == 2, sorted(set(names))
    assert not any("gemmx3" in k and "nt_kernel" in k for k in names), sorted(set(names))
    assert sum("mscale_first_kernel" in k for k in names) == 1, sorted(set(names))


# ---- 4. the first stage stays frozen under the trainer ----------------------------------------------------------------
def test_trainer_keeps_first_stage_bit_identical():
    from wire_amd.trainer import FusedTrainer
    model = _model(384, [1 / 9, 1 / 9, 4.0], 1 / 9)
    W0 = model.net[0].linear.weight.detach().clone()
    b0 = model.net[0].linear.bias.detach().clone()
    W1 = model.net[1].linear.weight.detach().clone()
    H = W = 128
    tr = FusedTrainer(model, (H, W), torch.tensor(_target(H * W)), lr=8e-3, niters=50)
    for _ in range(50):
        tr.step(tr.permutation().contiguous())
        tr.scheduler_step()
    torch.cuda.synchronize()
    assert torch.equal(model.net[0].linear.weight.detach(), W0)
    assert torch.equal(model.net[0].linear.bias.detach(), b0)
    assert not torch.equal(model.net[1].linear.weight.detach(), W1)
    assert model.net[0].scale_0.requires_grad is False


# ---- 5. quality gate ------------------------------------------------------------------------------------------------
def test_psnr_gate():
    from oracle import wire_oracle as wo
    from wire_amd.modules import models
    from wire_amd.trainer import FusedTrainer
    z = np.load(os.path.join(GOLDEN, "psnr_mscale_hl.npz"), allow_pickle=False)
    u8 = z["image_u8"]
    H, W, _ = u8.shape
    im = np.divide(u8, 255, dtype=np.float32)
    niters, maxpoints = int(z["niters"]), int(z["maxpoints"])
    torch.manual_seed(int(z["seed"]))
    model = models.get_INR(nonlin="bspline_mscale_HL", in_features=2, out_features=3,
                           hidden_features=int(z["hidden_features"]),
                           scaled_hidden_features=int(z["scaled_hidden_features"]), hidden_layers=int(z["hidden_layers"]),
                           first_omega_0=-0.2, hidden_omega_0=-0.2, scale=float(z["scale"]),
                           scale_tensor=torch.tensor([float(v) for v in z["scale_tensor"]]))
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
    print(f"mscale_HL psnr build {psnr:.4f} dB reference {float(z['psnr']):.4f} dB; loss drift vs fp64 "
          f"build {np.max(np.abs(losses - l64) / l64):.2e} reference {np.max(np.abs(ref - l64) / l64):.2e}")
    assert abs(psnr - float(z["psnr"])) < 0.1
    # at this learning rate the loop is chaotic enough that the reference's own fp32 trajectory leaves fp64 by ~20 %:
    # the build's is held to that drift, not to the fp32 trajectory step by step
    within_ref(np.max(np.abs(losses - l64) / l64), np.max(np.abs(ref - l64) / l64), "mscale psnr loop loss drift")


# ---- 6. scales from a state_dict --------------------------------------------------------------------------------------
def test_load_state_dict_scales():
    n = 8192
    model = _model(384, [1 / 9, 1 / 9, 4.0], 1 / 9)
    sd = model.state_dict()
    new_st, new_s = [0.2, 0.5, 3.0], 0.3
    sd["net.0.scale_0"] = torch.tensor(new_st)
    for k in sd:
        if k.endswith("scale_0") and k != "net.0.scale_0":
            sd[k] = torch.full((1,), new_s)
    model.load_state_dict(sd)
    d = model.net_desc()
    assert d.scale0 == np.float32(new_s) and list(d._b_base_.scales)[:3] == [np.float32(v) for v in new_st]
    sdn = _sd(model)
    x, t = _coords(n), _target(n)
    y32 = mr.loss_and_grads(sdn, 2, x, t, new_st, np.float32(new_s), np.float32)[0]
    y64 = mr.loss_and_grads(sdn, 2, x.astype(np.float64), t.astype(np.float64), new_st, new_s, np.float64)[0]
    with torch.no_grad():
        y = model(torch.tensor(x, device=DEV)).cpu().numpy()
    _errs("mscale load_state_dict scales", y, y32, y64)
    sd["net.0.scale_0"] = torch.tensor([0.2, 0.0, 3.0])
    with pytest.raises(NotImplementedError):
        model.load_state_dict(sd)
