"""GPU parity tests proper: the HIP path (through the C ABI, via the drop-in
modules) against the oracle / the reference-generated golden vectors.

Tolerances (SURVEY.md section 7 "Precision"): the reference's own fp32 path is
only accurate to err_ref = |y_ref32 - y_ref64| against its fp64 twin, and that
error grows with omega0 and depth.  Whole-network checks therefore require
    err_build = |y_hip - y64| / max|y64|  <=  2 * err_ref + 1e-6        (_util.within_ref)
and per-layer checks on identical inputs require 1e-5 relative to the layer max (forward; 2e-5 backward).
The measured err_build / err_ref of every comparison is written to gpurun_out/parity_ratios.txt.
"""
import ctypes as C
import os
import sys

import numpy as np
import pytest
import torch

from _util import FULL, ROOT, SMALL, build_model, family_ctx, load_golden, meta, oracle_run, params_np, relmax, tune, within_ref, final_bias_within_ref
from oracle import wire_oracle as wo

pytestmark = pytest.mark.gpu
DEV = "cuda"


def load_small(rec, model):
    sd = {k[2:]: torch.tensor(v) for k, v in rec.items() if k.startswith("p:")}
    model.load_state_dict(sd)
    return model.to(DEV)


def hip_forward_backward(model, rec):
    coords = torch.tensor(rec["coords"], device=DEV)
    target = torch.tensor(rec["target"], device=DEV)
    y = model(coords)
    loss = ((y - target) ** 2).mean()
    model.zero_grad()
    loss.backward()
    torch.cuda.synchronize()
    grads = {k: p.grad.detach().cpu().numpy() for k, p in model.named_parameters() if p.grad is not None}
    return y.detach().cpu().numpy(), float(loss.detach()), grads


def _check_grads(grads, g64, g32, label, err_y_ref, y64, extra_ref=None, target=None):
    """Every parameter gradient against the fp64 oracle with the fp32 oracle's own error as yardstick
    (err_build <= 2 err_ref + 1e-6); the final bias through the forward-propagated bound
    (_util.final_bias_within_ref)."""
    last = max(int(k.split(".")[1]) for k in grads)
    O = np.asarray(y64).shape[-1]
    for k, g in grads.items():
        if k == f"net.{last}.bias":
            resid = 0.0 if target is None else np.abs(np.asarray(y64) - np.asarray(target).reshape(np.shape(y64))).max()
            final_bias_within_ref(wo.as_real_pairs(g), wo.as_real_pairs(np.asarray(g64[k])), err_y_ref,
                                  np.abs(y64).max(), O, f"{label} grad {k}", resid_max=resid)
            continue
        ref_err = relmax(g32[k], g64[k])
        if extra_ref is not None:
            ref_err = max(ref_err, extra_ref[k])
        within_ref(relmax(g, g64[k]), ref_err, f"{label} grad {k}")


def test_extension_loaded():
    from wire_amd import _lib
    assert _lib.lib().wire_abi_version() == 1
    assert torch.cuda.is_available()


@pytest.mark.parametrize("name", SMALL)
def test_small_forward_backward(name):
    rec = load_golden(name)
    model = load_small(rec, build_model(rec))
    y, loss, grads = hip_forward_backward(model, rec)
    err_ref = relmax(rec["y"], rec["y64"])
    within_ref(relmax(y, rec["y64"]), err_ref, f"{name} y")
    assert abs(loss - float(rec["loss64"])) <= 1e-5 * abs(float(rec["loss64"])) + 10 * err_ref
    _check_grads(grads, {k: rec["g64:" + k] for k in grads}, {k: rec["g:" + k] for k in grads}, name, err_ref,
                 rec["y64"], target=rec["target"])


@pytest.mark.parametrize("name", FULL)
def test_full_configs(name):
    """BASELINE.json-size networks on the fixture's 256 coordinates."""
    rec = load_golden(name)
    model = build_model(rec).to(DEV)
    P = params_np(model)
    y, loss, grads = hip_forward_backward(model, rec)
    err_ref = relmax(rec["y"], rec["y64"])
    within_ref(relmax(y, rec["y64"]), err_ref, f"{name} y")
    # full gradients against the fp64 oracle on the same weights
    _, _, g64, _ = oracle_run(rec, P, double=True)
    _, _, g32, _ = oracle_run(rec, P, double=False)
    _check_grads(grads, g64, g32, name, err_ref, rec["y64"], target=rec["target"])
    for k, g in grads.items():
        # ... and directly against the heads of the REFERENCE's fp64 gradients held by the fixture
        ref_err = max(relmax(g32[k], g64[k]), 0.5 * err_ref)
        head = g[:8, :8] if g.ndim == 2 else g[:16]
        scale = float(rec["g64norm:" + k])
        assert np.abs(head - rec["g64head:" + k]).max() <= (2 * ref_err + 1e-6) * scale, k


def test_gemm_families_accuracy():
    """Three GEMM families serve the wire layers: split-bf16 on the bf16 MFMA (default), the
    3-multiplication complex product on the fp32 MFMA, the 4-multiplication real-expanded fp32 MFMA.
    Each meets the parity bar on its own, and neither the split nor the 3M form is materially less
    accurate than the plain fp32-MFMA product (the split carries FEWER roundings: tools/bf16x3_numerics.hip)."""
    from wire_amd import _lib
    L = _lib.lib()
    assert L.wire_tune_get(b"split_bf16") == 1 or "WIRE_SPLIT_BF16" in __import__("os").environ
    errs = {}
    fams = {"4m": (0, 0), "3m": (0, 1), "x3": (1, 1)}
    for fam, (sb, c3) in fams.items():
        with tune(split_bf16=sb, complex_3m=c3):
            for name in ("small_wire_hi", "full_cfg2_wire_4x363_lit"):
                rec = load_golden(name)
                model = load_small(rec, build_model(rec)) if name.startswith("small") else build_model(rec).to(DEV)
                y, loss, grads = hip_forward_backward(model, rec)
                err_ref = relmax(rec["y"], rec["y64"])
                e = relmax(y, rec["y64"])
                within_ref(e, err_ref, f"family {fam} {name} y")
                errs[(fam, name)] = (e, err_ref)
    for name in ("small_wire_hi", "full_cfg2_wire_4x363_lit"):
        e4, e3, ex = errs[("4m", name)][0], errs[("3m", name)][0], errs[("x3", name)][0]
        print(f"{name}: err 4M {e4:.3e}  3M {e3:.3e}  split-bf16 {ex:.3e}  reference fp32 {errs[('4m', name)][1]:.3e}")
        assert e3 <= 3 * e4 + 1e-6
        assert ex <= 3 * e4 + 1e-6


@pytest.mark.parametrize("name", ["full_cfg2_wire_4x256_api", "full_cfg4_wire2d_4x256", "full_cfg5_siren_4x256",
                                  "full_cfg5_posenc_4x256"])
def test_fp32_mfma_family_full_configs(name):
    """The fp32-MFMA kernels (split_bf16 = 0) stay covered: same bar as test_full_configs."""
    if name not in FULL:
        pytest.skip(f"no fixture {name}")
    with tune(split_bf16=0, complex_3m=1):
        rec = load_golden(name)
        model = build_model(rec).to(DEV)
        P = params_np(model)
        y, loss, grads = hip_forward_backward(model, rec)
        err_ref = relmax(rec["y"], rec["y64"])
        within_ref(relmax(y, rec["y64"]), err_ref, f"fp32-mfma {name} y")
        _, _, g64, _ = oracle_run(rec, P, double=True)
        _, _, g32, _ = oracle_run(rec, P, double=False)
        _check_grads(grads, g64, g32, f"fp32-mfma {name}", err_ref, rec["y64"], target=rec["target"])


@pytest.mark.parametrize("n", [1, 15, 16, 17, 127, 129, 255, 257, 4095, 4129])
def test_ragged_row_counts_against_oracle(n):
    """Row counts around every boundary of the GEMM kernels (16-row stages and the 32-row split rounding of the
    weight-gradient kernel, 128- and 256-row tiles of the NT kernel; 4129 > 4096 selects the 256-row tile with
    a ragged last tile): forward and all gradients of a 2-hidden-layer wire (K = 90: one full and one ragged
    128-column tile) against the fp64 oracle on the same weights, yardstick = the fp32 oracle's own error."""
    rec = load_golden("small_wire_d2")
    m = meta(rec)
    from wire_amd.modules import models
    torch.manual_seed(3)
    model = models.get_INR(nonlin="wire", in_features=2, out_features=3, hidden_features=128, hidden_layers=2,
                           first_omega_0=m["om1"], hidden_omega_0=m["om"], scale=m["sc"]).to(DEV)
    rng = np.random.default_rng(n)
    fake = {k: v for k, v in rec.items() if k.startswith("meta_")}
    fake["meta_hidden_features"] = np.array(128)
    fake["meta_L"] = np.array(2)
    fake["coords"] = rng.uniform(-1, 1, (n, 2)).astype(np.float32)
    fake["target"] = rng.uniform(0, 1, (n, 3)).astype(np.float32)
    P = params_np(model)
    y, loss, grads = hip_forward_backward(model, fake)
    y64, _, g64, _ = oracle_run(fake, P, double=True)
    y32, _, g32, _ = oracle_run(fake, P, double=False)
    # the yardstick (the reference arithmetic's own fp32 round-off) is a statistic: for a handful of rows take
    # it from 1024 rows of the same distribution through the same weights
    big = dict(fake)
    big["coords"] = rng.uniform(-1, 1, (1024, 2)).astype(np.float32)
    big["target"] = rng.uniform(0, 1, (1024, 3)).astype(np.float32)
    yb32, _, gb32, _ = oracle_run(big, P, double=False)
    yb64, _, gb64, _ = oracle_run(big, P, double=True)
    err_ref = max(relmax(y32, y64), relmax(yb32, yb64))
    # ... and so is the scale: one row's outputs can all be small, its round-off is not
    scale = max(np.abs(y64).max(), np.abs(yb64).max())
    within_ref(np.abs(y - y64).max() / scale, err_ref, f"ragged n={n} y")
    _check_grads(grads, g64, g32, f"ragged n={n}", err_ref, np.array([[scale] * 3]),
                 extra_ref={k: relmax(gb32[k], gb64[k]) for k in grads})


@pytest.mark.parametrize("name", ["small_wire_d2", "small_wire_d3", "small_wire_hi"])
def test_per_layer_identical_inputs(name):
    """ComplexGaborLayer.forward on the reference's own layer inputs: <= 1e-5."""
    rec = load_golden(name)
    model = load_small(rec, build_model(rec))
    L = meta(rec)["L"]
    x = torch.tensor(rec["coords"], device=DEV)
    for i in range(L + 1):
        out = model.net[i](x)
        torch.cuda.synchronize()
        assert out.dtype == torch.complex64
        assert relmax(out.detach().cpu().numpy(), rec[f"act{i}"]) <= 1e-5, f"layer {i}"
        x = torch.tensor(rec[f"act{i}"], device=DEV)   # identical inputs for the next layer


def test_per_layer_backward_matches_oracle():
    rec = load_golden("small_wire_d2")
    model = load_small(rec, build_model(rec))
    m = meta(rec)
    rng = np.random.default_rng(0)
    # hidden layer 1 on the reference's act0
    z = torch.tensor(rec["act0"], device=DEV, requires_grad=True)
    out = model.net[1](z)
    g = (rng.standard_normal(out.shape) + 1j * rng.standard_normal(out.shape)).astype(np.complex64)
    out.backward(torch.tensor(g, device=DEV))
    torch.cuda.synchronize()
    W = rec["p:net.1.linear.weight"].astype(np.complex128)
    b = rec["p:net.1.linear.bias"].astype(np.complex128)
    z64 = rec["act0"].astype(np.complex128).reshape(-1, W.shape[1])
    lin = z64 @ W.T + b
    o = wo.gabor_act(lin, m["om"], m["sc"])
    gl = wo.gabor_act_grad(g.reshape(lin.shape).astype(np.complex128), lin, o, m["om"], m["sc"])
    assert relmax(z.grad.cpu().numpy().reshape(lin.shape[0], -1), gl @ np.conj(W)) < 2e-5
    assert relmax(model.net[1].linear.weight.grad.cpu().numpy(), gl.T @ np.conj(z64)) < 2e-5
    assert relmax(model.net[1].linear.bias.grad.cpu().numpy(), gl.sum(0)) < 2e-5
    # first layer
    x = torch.tensor(rec["coords"], device=DEV)
    model.zero_grad()
    out0 = model.net[0](x)
    g0 = (rng.standard_normal(out0.shape) + 1j * rng.standard_normal(out0.shape)).astype(np.complex64)
    out0.backward(torch.tensor(g0, device=DEV))
    torch.cuda.synchronize()
    W0 = rec["p:net.0.linear.weight"].astype(np.float64)
    b0 = rec["p:net.0.linear.bias"].astype(np.float64)
    x64 = rec["coords"].astype(np.float64).reshape(-1, W0.shape[1])
    u = x64 @ W0.T + b0
    o0 = wo.gabor_act(u, m["om1"], m["sc"])
    gu = wo.gabor_act_grad(g0.reshape(u.shape).astype(np.complex128), u, o0, m["om1"], m["sc"])
    assert relmax(model.net[0].linear.weight.grad.cpu().numpy(), gu.T @ x64) < 2e-5
    assert relmax(model.net[0].linear.bias.grad.cpu().numpy(), gu.sum(0)) < 2e-5


@pytest.mark.parametrize("n", [0, 1, 63, 127, 129, 1000])
def test_ragged_and_empty_batches(n):
    """Tile tails (n not a multiple of 128), a single row and the empty batch;
    [n, D] and [B, n, D] leading shapes (modules/volutils.py:130, wire_multi_sr.py:194)."""
    rec = load_golden("small_wire_d2")
    model = load_small(rec, build_model(rec))
    m = meta(rec)
    P = {k[2:]: v for k, v in rec.items() if k.startswith("p:") and "omega" not in k and "scale_0" not in k}
    rng = np.random.default_rng(n)
    coords = rng.uniform(-1, 1, (n, 2)).astype(np.float32)
    y = model(torch.tensor(coords, device=DEV))
    assert tuple(y.shape) == (n, 3)
    if n == 0:
        return
    y64 = wo.wire_forward(wo.cast_params(P, True), coords.astype(np.float64), m["L"], m["om1"], m["om"], m["sc"])
    assert relmax(y.detach().cpu().numpy(), y64) < 2e-5
    if n >= 2:
        y2 = model(torch.tensor(coords, device=DEV).reshape(2, n // 2, 2) if n % 2 == 0 else
                   torch.tensor(coords, device=DEV)[None])
        np.testing.assert_array_equal(y2.detach().reshape(-1, 3).cpu().numpy()[:n], y.detach().cpu().numpy())


def test_state_dict_roundtrip_and_count():
    rec = load_golden("full_denoise_wire_2x300")
    model = build_model(rec).to(DEV)
    from wire_amd.modules import utils
    assert utils.count_parameters(model) == 91587
    misc = load_golden("misc")
    assert list(model.state_dict().keys()) == [str(k) for k in misc["sd_keys_2x300"]]
    sd = {k: v.clone() for k, v in model.state_dict().items()}
    model2 = build_model(rec).to(DEV)
    model2.load_state_dict(sd)
    x = torch.rand(1, 300, 2, device=DEV) * 2 - 1
    np.testing.assert_array_equal(model(x).detach().cpu().numpy(), model2(x).detach().cpu().numpy())
    assert model.net[0].linear.weight.dtype == torch.float32
    assert model.net[1].linear.weight.dtype == torch.complex64
    assert abs(model.net[0].scale_0.item() - 8.0) < 1e-6


# ---------------------------------------------------------------------------
# BASELINE.json full size (262 144 coordinates, 4 x 256 complex): size-independent
# properties + a sampled comparison with the fp64 oracle
# ---------------------------------------------------------------------------
@pytest.fixture(scope="module")
def big():
    from wire_amd.modules import models
    torch.manual_seed(0)
    model = models.get_INR(nonlin="wire", in_features=2, out_features=3, hidden_features=363,
                           hidden_layers=4, first_omega_0=20.0, hidden_omega_0=20.0, scale=30.0).to(DEV)
    coords = torch.tensor(wo.image_coords(512, 512), device=DEV)
    return model, coords


def test_full_size_rows_are_position_independent(big):
    """Permuting the batch permutes the outputs bit for bit (each row is an
    independent MFMA accumulation chain; no cross-row coupling)."""
    model, coords = big
    with torch.no_grad():
        y = model(coords)
        perm = torch.randperm(coords.shape[0], device=DEV)
        yp = model(coords[perm])
    assert torch.equal(yp, y[perm])


def test_full_size_sampled_vs_oracle(big):
    model, coords = big
    with torch.no_grad():
        y = model(coords)
    idx = torch.arange(0, coords.shape[0], 997, device=DEV)[:384]
    P = params_np(model)
    c = coords[idx].cpu().numpy()
    y64 = wo.wire_forward(wo.cast_params(P, True), c.astype(np.float64), 4, 20.0, 20.0, 30.0)
    y32 = wo.wire_forward(wo.cast_params(P, False), c, 4, np.float32(20.0), np.float32(20.0), np.float32(30.0))
    err_ref = relmax(y32, y64)
    within_ref(relmax(y[idx].cpu().numpy(), y64), err_ref, "full-size sampled y")


def test_full_size_gradient_linearity_and_additivity(big):
    """grads(2 g) == 2 grads(g) (power-of-two scaling commutes with every rounding
    except in the subnormal range, which the s0=30 Gaussian tails do reach, hence
    1e-6 instead of bit equality); grads over a batch == sum of grads over its two
    halves (fp tolerance)."""
    model, coords = big
    n = coords.shape[0]
    torch.manual_seed(1)
    gy = torch.randn(n, 3, device=DEV) / n

    def grads(c, g):
        model.zero_grad()
        model(c).backward(g)
        return [p.grad.detach().clone() for p in model.parameters() if p.grad is not None]

    g1 = grads(coords, gy)
    g2 = grads(coords, 2 * gy)
    for a, b in zip(g1, g2):
        assert (2 * a - b).abs().max().item() <= 1e-6 * b.abs().max().item()
    ga = grads(coords[: n // 2], gy[: n // 2])
    gb = grads(coords[n // 2:], gy[n // 2:])
    for a, b, c in zip(g1, ga, gb):
        s = (b + c)
        assert (a - s).abs().max().item() <= 2e-4 * a.abs().max().item() + 1e-12


# ---------------------------------------------------------------------------
# training glue kernels
# ---------------------------------------------------------------------------
def test_coords_kernel_matches_reference_grids():
    from wire_amd import _lib
    from wire_amd.modules import utils
    L = _lib.lib()
    misc = load_golden("misc")
    s = torch.cuda.current_stream().cuda_stream
    # 2-D image grid, torch.linspace tables (wire_image_denoise.py:63-66)
    tx, ty, _ = utils.axis_tables(5, 7, style="torch")
    tx, ty = tx.to(DEV), ty.to(DEV)
    out = torch.empty(35, 2, device=DEV)
    _lib.check(L.wire_coords_from_index(s, None, 0, 35, tx.data_ptr(), 7, ty.data_ptr(), 5, None, 1, out.data_ptr()))
    np.testing.assert_array_equal(out.cpu().numpy(), misc["coords_img_5_7"])
    # 3-D volume grid, numpy tables (modules/utils.py:171-176), through an index list
    tx, ty, tz = [t.to(DEV) for t in utils.axis_tables(6, 5, 4, style="numpy")]
    idx = torch.randperm(120, device=DEV)
    out3 = torch.empty(120, 3, device=DEV)
    _lib.check(L.wire_coords_from_index(s, idx.data_ptr(), 0, 120, tx.data_ptr(), 5, ty.data_ptr(), 6,
                                        tz.data_ptr(), 4, out3.data_ptr()))
    np.testing.assert_array_equal(out3.cpu().numpy(), misc["coords3d_6_5_4"][idx.cpu().numpy()])
    np.testing.assert_array_equal(utils.get_coords(6, 5, 4).numpy(), misc["coords3d_6_5_4"])
    np.testing.assert_array_equal(utils.get_coords(7, 9).numpy(), misc["coords2d_7_9"])


def test_mse_and_adam_kernels():
    from wire_amd import _lib
    L = _lib.lib()
    s = torch.cuda.current_stream().cuda_stream
    rng = np.random.default_rng(3)
    n, O = 5000, 3
    y = rng.standard_normal((n, O)).astype(np.float32)
    t = rng.standard_normal((7000, O)).astype(np.float32)
    idx = rng.permutation(7000)[:n].astype(np.int64)
    yd, td, idd = torch.tensor(y, device=DEV), torch.tensor(t, device=DEV), torch.tensor(idx, device=DEV)
    gy = torch.empty(n, O, device=DEV)
    loss = torch.zeros(1, device=DEV)
    part = torch.empty(4096, device=DEV)
    rec = torch.zeros(7000, O, device=DEV)
    _lib.check(L.wire_mse_grad(s, yd.data_ptr(), td.data_ptr(), idd.data_ptr(), 0, n, O, 1.0, gy.data_ptr(),
                               loss.data_ptr(), rec.data_ptr(), part.data_ptr()))
    l64, g64 = wo.mse_loss_and_grad(y.astype(np.float64), t[idx].astype(np.float64))
    assert abs(loss.item() - l64) < 1e-5 * l64
    assert relmax(gy.cpu().numpy(), g64) < 1e-6
    np.testing.assert_array_equal(rec.cpu().numpy()[idx], y)
    # Adam: 3 steps against the oracle's restatement of torch.optim.Adam
    cnt = 10007
    p = rng.standard_normal(cnt).astype(np.float32)
    pd = torch.tensor(p, device=DEV)
    m = torch.zeros(cnt, device=DEV)
    v = torch.zeros(cnt, device=DEV)
    pn, mn, vn = p.astype(np.float64), np.zeros(cnt), np.zeros(cnt)
    for step in range(1, 4):
        g = (rng.standard_normal(cnt) * 10.0 ** rng.integers(-6, 1, cnt)).astype(np.float32)
        gd = torch.tensor(g, device=DEV)
        _lib.check(L.wire_adam_step_flat(s, pd.data_ptr(), gd.data_ptr(), m.data_ptr(), v.data_ptr(), cnt,
                                         5e-3, 0.9, 0.999, 1e-8, step))
        pn, mn, vn = wo.adam_step(pn, g.astype(np.float64), mn, vn, step, 5e-3)
    assert np.abs(pd.cpu().numpy() - pn).max() < 2e-6


def test_fused_trainer_matches_autograd_path_and_oracle():
    """FusedTrainer.step == (model(coords) -> MSE -> backward -> torch Adam) on the
    same batch, and its loss trajectory follows the CPU restatement."""
    from oracle import torch_ref
    from wire_amd.trainer import FusedTrainer
    from wire_amd.modules import models
    H = W = 32
    torch.manual_seed(0)
    model = models.get_INR(nonlin="wire", in_features=2, out_features=3, hidden_features=64,
                           hidden_layers=2, first_omega_0=7.0, hidden_omega_0=7.0, scale=6.0)
    p_cpu = {k: v.detach().clone() for k, v in model.state_dict().items() if "omega" not in k and "scale_0" not in k}
    model = model.to(DEV)
    g = torch.Generator().manual_seed(5)
    target = torch.rand(H * W, 3, generator=g)
    tr = FusedTrainer(model, (H, W), target, lr=5e-3, niters=2000, keep_rec=True)
    coords = torch.tensor(wo.image_coords(H, W))
    losses = []
    for _ in range(5):
        losses.append(tr.step())
        tr.scheduler_step()
    torch.cuda.synchronize()
    losses = [float(l.item()) for l in losses]
    ref_losses, ref_p = torch_ref.train_steps(p_cpu, coords[None], target[None], 2, 7.0, 7.0, 6.0, 5e-3, 5, 2000)
    np.testing.assert_allclose(losses, ref_losses, rtol=2e-4)
    for k, v in ref_p.items():
        mine = dict(model.state_dict())[k].cpu().numpy()
        assert np.abs(mine - v.numpy()).max() < 0.05 * 5e-3, k


def _smooth_image(H, W):
    yy, xx = np.meshgrid(np.linspace(-1, 1, H), np.linspace(-1, 1, W), indexing="ij")
    img = np.stack([0.5 + 0.4 * np.sin(3 * xx + 2 * yy), 0.5 + 0.4 * np.cos(4 * xx * yy),
                    0.5 + 0.3 * np.sin(5 * yy) * np.cos(2 * xx)], -1)
    return img.astype(np.float32)


def test_short_schedule_psnr_within_0p1_db_of_cpu_restatement():
    """North-star quality criterion: after a fixed short schedule (150 full-batch Adam steps on a
    48x48 smooth image) the reconstruction PSNR -- utils.psnr, max(x)/mse (modules/utils.py:67-82) --
    is within 0.1 dB of the reference's CPU path on the same seed and data."""
    from oracle import torch_ref
    from wire_amd.trainer import FusedTrainer
    from wire_amd.modules import models, utils
    H = W = 48
    steps = 150
    img = _smooth_image(H, W)
    target = torch.tensor(img.reshape(-1, 3))
    torch.manual_seed(0)
    model = models.get_INR(nonlin="wire", in_features=2, out_features=3, hidden_features=90,
                           hidden_layers=2, first_omega_0=7.0, hidden_omega_0=7.0, scale=6.0)
    p_cpu = {k: v.detach().clone() for k, v in model.state_dict().items() if "omega" not in k and "scale_0" not in k}
    model = model.to(DEV)
    tr = FusedTrainer(model, (H, W), target, lr=5e-3, niters=steps)
    for _ in range(steps):
        tr.step()
        tr.scheduler_step()
    rec = tr.render().cpu().numpy().reshape(H, W, 3)
    coords = torch.tensor(wo.image_coords(H, W))
    _, p_ref = torch_ref.train_steps(p_cpu, coords[None], target[None], 2, 7.0, 7.0, 6.0, 5e-3, steps, steps)
    with torch.no_grad():
        rec_ref = torch_ref.wire_forward(p_ref, coords[None], 2, 7.0, 7.0, 6.0)[0].numpy().reshape(H, W, 3)
    psnr_hip, psnr_ref = utils.psnr(img, rec), utils.psnr(img, rec_ref)
    print(f"PSNR after {steps} steps: HIP {psnr_hip:.3f} dB, CPU restatement {psnr_ref:.3f} dB")
    assert psnr_ref > 25.0                     # the schedule actually fits the image
    assert abs(psnr_hip - psnr_ref) < 0.1


def test_occupancy_style_minibatches_match_oracle():
    """wire_occupancy.py:137-158 shape: D=3, O=1, 3 hidden x 300 (K=212), numpy-linspace grid
    (modules/utils.py:163-176), random index minibatches with a ragged last batch.  Gradients of
    every minibatch against the fp64 oracle; also the render() of the whole volume."""
    from wire_amd.trainer import FusedTrainer
    from wire_amd.modules import models
    H, W, T = 12, 10, 9
    npts = H * W * T
    maxpoints = 400                                    # 1080 = 400 + 400 + 280 (ragged tail)
    rng = np.random.default_rng(0)
    vol = (rng.random((npts, 1)) > 0.5).astype(np.float32)
    torch.manual_seed(0)
    model = models.get_INR(nonlin="wire", in_features=3, out_features=1, hidden_features=300,
                           hidden_layers=3, first_omega_0=20.0, hidden_omega_0=20.0, scale=10.0).to(DEV)
    tr = FusedTrainer(model, (H, W, T), torch.tensor(vol), lr=0.0, coords_style="numpy", keep_rec=True)
    coords_all = wo.volume_coords(H, W, T)
    P64 = wo.cast_params(params_np(model), True)
    P32 = wo.cast_params(params_np(model), False)
    perm = torch.randperm(npts)
    # yardstick: the reference arithmetic's own fp32 round-off.  A 280-400-row minibatch is a small sample of it (one
    # max over few rows; at N = 16 384 and 262 144 the same net measures err_build / err_ref = 0.7 ... 1.45,
    # tests/test_gpu_timed_kernels.py), so it is taken over the minibatch AND over 4096 points of the same cube
    # through the same weights
    # ... and over eight more minibatches of the same size (the error of a 400-row gradient is dominated by its few
    # worst rows -- activations reach exp(omega0^2 / 4 s0^2) = e per layer -- so single minibatches scatter by 2-3x)
    ref_all, err_y_all = {}, 0.0
    for nb in [4096] + [400] * 8:
        cb = rng.uniform(-1, 1, (nb, 3)).astype(np.float32)
        tb = (rng.random((nb, 1)) > 0.5).astype(np.float32)
        ya64, ca64 = wo.wire_forward(P64, cb.astype(np.float64), 3, 20.0, 20.0, 10.0, keep=True)
        ga64 = wo.wire_backward(P64, ca64, wo.mse_loss_and_grad(ya64, tb.astype(np.float64))[1], 3, 20.0, 20.0, 10.0)
        ya32, ca32 = wo.wire_forward(P32, cb, 3, 20.0, 20.0, 10.0, keep=True)
        ga32 = wo.wire_backward(P32, ca32, wo.mse_loss_and_grad(ya32, tb)[1], 3, 20.0, 20.0, 10.0)
        for k in ga64:
            ref_all[k] = max(ref_all.get(k, 0.0), relmax(wo.as_real_pairs(ga32[k]), wo.as_real_pairs(ga64[k])))
        err_y_all = max(err_y_all, relmax(ya32, ya64))
    worst = {}
    for b in range(0, npts, maxpoints):
        idx = perm[b:min(npts, b + maxpoints)]
        loss = tr.step(idx.to(DEV))                    # lr = 0: parameters stay put
        torch.cuda.synchronize()
        c = coords_all[idx.numpy()].astype(np.float64)
        y64, cache = wo.wire_forward(P64, c, 3, 20.0, 20.0, 10.0, keep=True)
        l64, gy = wo.mse_loss_and_grad(y64, vol[idx.numpy()].astype(np.float64))
        g64 = wo.wire_backward(P64, cache, gy, 3, 20.0, 20.0, 10.0)
        # the reference arithmetic in fp32 on the same minibatch: its own round-off is the yardstick
        # (SURVEY section 7 "Precision": omega0 = 20, s0 = 10 amplifies fp32 round-off to ~1e-4)
        y32, cache32 = wo.wire_forward(P32, c.astype(np.float32), 3, 20.0, 20.0, 10.0, keep=True)
        _, gy32 = wo.mse_loss_and_grad(y32, vol[idx.numpy()])
        g32 = wo.wire_backward(P32, cache32, gy32, 3, 20.0, 20.0, 10.0)
        assert abs(float(loss.item()) - l64) < 1e-4 * l64 + 1e-6
        flat = tr.flat_grad.cpu().numpy()
        names = [k for k in model.state_dict().keys() if "omega_0" not in k and "scale_0" not in k]
        for name, off, t in zip(names, tr.offsets, model.param_tensors()):
            g = wo.as_real_pairs(g64[name]).astype(np.float64).ravel()
            mine = flat[off:off + g.size]
            ref_err = np.abs(wo.as_real_pairs(g32[name]).astype(np.float64).ravel() - g).max() / np.abs(g).max()
            if name == "net.4.bias":
                final_bias_within_ref(mine, g, max(relmax(y32, y64), err_y_all), np.abs(y64).max(), 1,
                                      f"occupancy batch {b} grad {name}",
                                      resid_max=np.abs(y64 - vol[idx.numpy()]).max())
            else:
                worst.setdefault(name, [0.0, ref_all[name]])
                worst[name][0] = max(worst[name][0], np.abs(mine - g).max() / np.abs(g).max())
                worst[name][1] = max(worst[name][1], ref_err)
        np.testing.assert_allclose(tr.rec.cpu().numpy()[idx.numpy()], y64, atol=2e-4 * np.abs(y64).max())
    # worst minibatch of the build against the worst of the reference arithmetic (same three minibatches + the sample)
    for name, (eb, er) in worst.items():
        within_ref(eb, er, f"occupancy minibatches grad {name}")
    full = tr.render(tile=333).cpu().numpy()
    y_all = wo.wire_forward(P64, coords_all.astype(np.float64), 3, 20.0, 20.0, 10.0)
    assert relmax(full, y_all) < 2e-4
    # device-side IoU (modules/volutils.py:74-91) against the oracle's restatement; pred untouched
    pred = torch.tensor(full, device=DEV)
    keep = pred.clone()
    iou_dev = float(tr.iou(pred, thres=0.5).item())
    assert abs(iou_dev - wo.iou(full, vol, 0.5)) < 1e-6
    assert torch.equal(pred, keep)


def test_device_psnr_matches_reference_known_answer():
    """wire_eval_metric mode 0 reproduces utils.psnr's known answer generated from the reference
    (tests/golden/misc.npz) -- 10 log10(max(x)/mse), not the max^2 textbook form."""
    from wire_amd.trainer import FusedTrainer
    from wire_amd.modules import models
    misc = load_golden("misc")
    x, xh = misc["psnr_x"], misc["psnr_xhat"]
    H, W = x.shape[0], x.shape[1]
    model = models.get_INR(nonlin="wire", in_features=2, out_features=3, hidden_features=32, hidden_layers=1).to(DEV)
    tr = FusedTrainer(model, (H, W), torch.tensor(x.reshape(-1, 3)))
    val = float(tr.psnr(torch.tensor(xh.reshape(-1, 3), device=DEV)).item())
    assert abs(val - float(misc["psnr_val"])) < 1e-3


@pytest.mark.parametrize("name", ["small_siren", "small_gauss", "small_relu"])
def test_real_layers_identical_inputs_and_backward(name):
    """SineLayer / GaussLayer / ReLULayer .forward (per-layer API used by
    modules/utils.py:246-252) on the reference's own layer inputs, and one layer's backward."""
    rec = load_golden(name)
    model = load_small(rec, build_model(rec))
    m = meta(rec)
    x = torch.tensor(rec["coords"], device=DEV)
    for i in range(m["L"] + 1):
        out = model.net[i](x)
        assert out.dtype == torch.float32
        assert relmax(out.detach().cpu().numpy(), rec[f"act{i}"]) <= 1e-5, f"layer {i}"
        x = torch.tensor(rec[f"act{i}"], device=DEV)
    # backward of hidden layer 1 on the reference's act0
    kind = m["kind"]
    z = torch.tensor(rec["act0"], device=DEV, requires_grad=True)
    out = model.net[1](z)
    rng = np.random.default_rng(1)
    g = rng.standard_normal(tuple(out.shape)).astype(np.float32)
    model.zero_grad()
    out.backward(torch.tensor(g, device=DEV))
    torch.cuda.synchronize()
    W = rec["p:net.1.linear.weight"].astype(np.float64)
    b = rec["p:net.1.linear.bias"].astype(np.float64)
    z64 = rec["act0"].astype(np.float64).reshape(-1, W.shape[1])
    lin = z64 @ W.T + b
    o = wo.real_act(kind, lin, m["om"], m["sc"])
    gl = wo.real_act_grad(kind, g.reshape(lin.shape).astype(np.float64), lin, o, m["om"], m["sc"])
    assert relmax(z.grad.cpu().numpy().reshape(lin.shape[0], -1), gl @ W) < 2e-5
    assert relmax(model.net[1].linear.weight.grad.cpu().numpy(), gl.T @ z64) < 2e-5
    assert relmax(model.net[1].linear.bias.grad.cpu().numpy(), gl.sum(0)) < 2e-5


@pytest.mark.parametrize("H,W,scale", [(24, 24, 3), (26, 21, 4)])
def test_super_resolution_step_matches_oracle(H, W, scale):
    """wire_SISR.py:151-178 shape: full high-resolution grid -> AvgPool2d(scale) -> MSE against the low-resolution
    image -> backward.  The device kernel alone against the oracle's restatement (which test_oracle_golden pins to
    torch.nn.AvgPool2d), then every parameter gradient of FusedTrainer.step_downsampled against the fp64 oracle."""
    from wire_amd import _lib
    from wire_amd.trainer import FusedTrainer
    from wire_amd.modules import models
    import ctypes as C
    L = _lib.lib()
    rng = np.random.default_rng(H + W)
    O, H2, W2 = 3, H // scale, W // scale
    # --- the operator alone
    y = rng.standard_normal((H * W, O)).astype(np.float32)
    gt = rng.standard_normal((H2 * W2, O)).astype(np.float32)
    l64, g64, r64 = wo.avgpool_mse_loss_and_grad(y.astype(np.float64), H, W, scale, gt.astype(np.float64))
    yt, gtt = torch.tensor(y, device=DEV), torch.tensor(gt, device=DEV)
    gy = torch.full((H * W, O), 7.0, device=DEV)
    rec = torch.empty(H2 * W2, O, device=DEV)
    loss = torch.zeros(1, device=DEV)
    part = torch.empty(4096, device=DEV)
    stream = torch.cuda.current_stream().cuda_stream
    _lib.check(L.wire_avgpool_mse_grad(stream, yt.data_ptr(), H, W, O, scale, gtt.data_ptr(), gy.data_ptr(),
                                       rec.data_ptr(), loss.data_ptr(), part.data_ptr()))
    torch.cuda.synchronize()
    assert abs(float(loss) - l64) <= 1e-5 * l64
    np.testing.assert_allclose(gy.cpu().numpy(), g64, rtol=0, atol=1e-6 * np.abs(g64).max() + 1e-12)
    np.testing.assert_allclose(rec.cpu().numpy(), r64, rtol=0, atol=2e-6)
    assert L.wire_avgpool_mse_grad(stream, yt.data_ptr(), H, W, O, H + 1, gtt.data_ptr(), gy.data_ptr(),
                                   None, loss.data_ptr(), part.data_ptr()) < 0      # scale > H: refused
    # --- the whole step (lr = 0: parameters stay put)
    torch.manual_seed(0)
    model = models.get_INR(nonlin="wire", in_features=2, out_features=O, hidden_features=128, hidden_layers=2,
                           first_omega_0=7.0, hidden_omega_0=7.0, scale=6.0).to(DEV)
    tr = FusedTrainer(model, (H, W), torch.zeros(H * W, O), lr=0.0)
    lossd = tr.step_downsampled(gtt, scale)
    torch.cuda.synchronize()
    P64 = wo.cast_params(params_np(model), True)
    coords = wo.image_coords(H, W).astype(np.float64)
    y64, cache = wo.wire_forward(P64, coords, 2, 7.0, 7.0, 6.0, keep=True)
    l64, gy64, _ = wo.avgpool_mse_loss_and_grad(y64, H, W, scale, gt.astype(np.float64))
    g64 = wo.wire_backward(P64, cache, gy64, 2, 7.0, 7.0, 6.0)
    assert abs(float(lossd.item()) - l64) <= 2e-5 * l64
    flat = tr.flat_grad.cpu().numpy()
    names = [k for k in model.state_dict().keys() if "omega_0" not in k and "scale_0" not in k]
    for name, off, t in zip(names, tr.offsets, model.param_tensors()):
        g = wo.as_real_pairs(g64[name]).astype(np.float64).ravel()
        assert np.abs(flat[off:off + g.size] - g).max() <= 5e-5 * np.abs(g).max() + 1e-10, name


def test_random_shapes_against_oracle():
    """tools/fuzz_shapes.py: wire nets of random width / depth / D / O on random row counts, forward and all
    gradients against fp64 relative to the fp32 reference arithmetic's own error.  These are a few hundred rows of
    shallow random nets, where err_ref is one noisy draw of ~1e-6: the worst ratio measured over 60 + 16 cases is 2.48
    (profiles/r02_parity_ratios.txt), so the bound is that measured worst + a 20 % margin -- named as such, it is NOT
    the protocol's 2 x, which the bench-size step tests (tests/test_gpu_timed_kernels.py) hold."""
    import importlib
    sys.path.insert(0, os.path.join(ROOT, "tools"))
    fz = importlib.import_module("fuzz_shapes")
    assert fz.main(16, 11) < 3.0


def test_wire2d_per_layer_identical_inputs():
    """ComplexGaborLayer2D.forward (modules/wire2d.py:56-67) stand-alone, on the reference's own layer inputs
    (what modules/utils.py:246-252 does for visualisation): <= 1e-5 per layer."""
    rec = load_golden("small_wire2d")
    model = load_small(rec, build_model(rec))
    L = meta(rec)["L"]
    x = torch.tensor(rec["coords"], device=DEV)
    for i in range(L + 1):
        out = model.net[i](x)
        torch.cuda.synchronize()
        assert out.dtype == torch.complex64
        assert relmax(out.detach().cpu().numpy(), rec[f"act{i}"]) <= 1e-5, f"layer {i}"
        x = torch.tensor(rec[f"act{i}"], device=DEV)


@pytest.mark.parametrize("is_first", [False, True])
def test_wire2d_layer_backward_matches_autograd(is_first):
    """Stand-alone ComplexGaborLayer2D: every gradient (input, both Linears) against eager fp64 autograd of the
    oracle's restatement (oracle/torch_ref.gabor2d), yardstick = the same in fp32."""
    from oracle import torch_ref
    from wire_amd.modules.wire2d import ComplexGaborLayer2D
    import torch.nn.functional as F
    torch.manual_seed(5)
    n, fin, fout = 300, (2 if is_first else 70), 90
    om, sc = 10.0, 10.0
    layer = ComplexGaborLayer2D(fin, fout, is_first=is_first, omega0=om, sigma0=sc).to(DEV)
    rng = np.random.default_rng(9)
    if is_first:
        x_np = rng.uniform(-1, 1, (n, fin)).astype(np.float32)
    else:
        x_np = (0.3 * (rng.standard_normal((n, fin)) + 1j * rng.standard_normal((n, fin)))).astype(np.complex64)
    g_np = (rng.standard_normal((n, fout)) + 1j * rng.standard_normal((n, fout))).astype(np.complex64)
    x = torch.tensor(x_np, device=DEV, requires_grad=not is_first)
    out = layer(x)
    out.backward(torch.tensor(g_np, device=DEV))
    torch.cuda.synchronize()
    got = {"W": layer.linear.weight.grad, "b": layer.linear.bias.grad, "V": layer.scale_orth.weight.grad,
           "c": layer.scale_orth.bias.grad}
    if not is_first:
        got["x"] = x.grad
    got = {k: v.cpu().numpy() for k, v in got.items()}
    got["out"] = out.detach().cpu().numpy()

    def ref(double):
        cd = torch.complex128 if double else torch.complex64
        rd = torch.float64 if double else torch.float32
        pd = rd if is_first else cd
        W = layer.linear.weight.detach().cpu().to(pd).requires_grad_(True)
        b = layer.linear.bias.detach().cpu().to(pd).requires_grad_(True)
        V = layer.scale_orth.weight.detach().cpu().to(pd).requires_grad_(True)
        c = layer.scale_orth.bias.detach().cpu().to(pd).requires_grad_(True)
        xx = torch.tensor(x_np).to(pd).requires_grad_(not is_first)
        o = torch_ref.gabor2d(F.linear(xx, W, b), F.linear(xx, V, c), om, sc)
        # real loss whose gradient w.r.t. o is g (PyTorch convention: grad = dL/dRe + j dL/dIm)
        gg = torch.tensor(g_np).to(cd)
        (o.real * gg.real + o.imag * gg.imag).sum().backward()
        r = {"W": W.grad, "b": b.grad, "V": V.grad, "c": c.grad, "out": o.detach()}
        if not is_first:
            r["x"] = xx.grad
        return {k: v.numpy() for k, v in r.items()}

    r64, r32 = ref(True), ref(False)
    for k in got:
        within_ref(relmax(got[k], r64[k]), relmax(r32[k], r64[k]), f"wire2d layer is_first={is_first} {k}")


def test_posenc_module_matches_reference_known_answer():
    """PosEncoding.forward (modules/relu.py:62-75) through wire_posenc_fwd -- the HIP kernel of the fused path's first-layer
    prologue -- against the reference-generated vector of tests/golden/misc.npz, and against the oracle on a grid."""
    from _util import load_golden
    from wire_amd.modules.relu import PosEncoding
    misc = load_golden("misc")
    pe = PosEncoding(2, sidelength=512)
    got = pe(torch.tensor(misc["posenc2_in"]).to(DEV)).cpu().numpy()
    np.testing.assert_allclose(got, misc["posenc2_out"], atol=1e-6)
    c = wo.image_coords(33, 47)[None]
    got = pe(torch.tensor(c).to(DEV)).cpu().numpy()
    ref = wo.posenc(c.astype(np.float64), pe.num_frequencies)
    assert got.shape == ref.shape == (1, 33 * 47, 30)
    assert np.abs(got - ref).max() <= 2e-5          # 2^6 pi c rounded to fp32 before sin / cos, as in the reference
