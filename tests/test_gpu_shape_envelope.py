"""Every accepted input and output width on every net kind.

make_plan accepts in_features 1..4 and out_features 1..8 for every kind; the other GPU modules run D in {2, 3} and O in
{1, 3, 4}.  The remaining values do not run the same kernels at another size, they take other code:
  * D = 1, 4: the plain four-term forms of EPI_GABOR_BWD_FIRST / EPI_GABOR2D_BWD_FIRST (the compile-time ``first_dn``
    editions exist for D = 2, 3), D = 4 also the general path behind the lean ``ep.D <= 3`` epilogues of the 32 x 32
    kernels, all four lanes of cg[4], coordgrad_rows_kernel, colreduce_kernel and the 5-float stride of the first-layer sums;
  * O = 5..8: no fused final stage, no whole-net kernel, no data-gradient chain, no batched weight gradients -- training
    runs the layer-by-layer forward, launch_mse_grad and final_bwd_kernel with all eight accumulators, inference ends in
    final_fwd_kernel;
  * O = 2: the OT instantiation of the fused final stage and of the whole-net kernels' final dot product between 1 and 4;
  * the combiner of bspline_mscale_2, the heads of bspline_mscale_hier and the final stage of mfn keep WIRE_MAXO arrays of
    their own.
tests/envelope_ref.py holds the nets (each kind in the regime of its own tests, hidden_layers = 2), the widths
(D, O) in {(1, 8), (4, 2), (4, 5), (3, 7), (2, 6)} and the row counts: 333 (the small-batch 3 x bf16 32 x 32 kernels)
and 4096 + 37 (the smallest batch of the 2 x fp16 route and of the whole-net kernels, ragged last tile).

Three checks per case, all under the protocol of SURVEY.md section 7, err_build <= 2 err_ref + 1e-6 (_util.within_ref),
err_ref = the fp32 restatement's own error against fp64, the larger of its value over the case's rows and over a
4096-row sample through the same weights (as test_gpu_parity.test_ragged_row_counts_against_oracle takes it):
  1. wire_train_fwd_bwd through ctypes on explicit coordinates (_util.abi_train_step): y, loss (1e-5 relative), g_y
     (where the route writes it), the rec scatter and every parameter gradient against the numpy restatement of the kind;
  2. autograd with coords.requires_grad_() and the loss sum(y w): the coordinate gradient and every parameter gradient
     against eager fp64 autograd of the same formulas;
  3. wire_mlp_fwd(save_for_bwd = 0) into a NaN-filled y.
relu follows the forced-decision protocol of test_gpu_timed_kernels.KIND_STEP_CASES.  test_routes keeps the module
honest about which kernels these shapes launch."""
import ctypes as C

import numpy as np
import pytest
import torch

import envelope_ref as er
import test_gpu_coords_grad as cg
from _util import _nt_editions, abi_train_step, family_ctx, final_bias_within_ref, relmax, tune, within_ref
from oracle import torch_ref
from oracle import wire_oracle as wo

pytestmark = pytest.mark.gpu
DEV = "cuda"
L = er.LAYERS
SAMPLE = 4096
CASES = [(net, D, O, n) for net in er.MAIN_NETS for D, O in er.WIDTHS for n in er.ROWS]
CASES += [("relu_posenc", D, O, n) for D, O in ((1, 8), (3, 7)) for n in er.ROWS]
CASES += [("bspline_mscale_2_s8", 4, 8, 333)]
# weight = 0.5 with idx = NULL and first > 0: one fused-final and one unfused case per net
SHIFTED = {(4, 2, 4096 + 37), (1, 8, 333), (4, 8, 333)}
FAMILY_CASE = ("wire_k256", 4, 5, 4096 + 37)
case_id = lambda c: f"{c[0]}-D{c[1]}-O{c[2]}-n{c[3]}"


def _is_relu(net):
    return er.NETS[net]["kind"] == "relu"


def _pairs(a):
    return wo.as_real_pairs(np.asarray(a)).astype(np.float64).ravel()


# ---------------------------------------------------------------------------------------------------------------------
# the yardstick over a 4096-row sample through the same weights: one evaluation per (net, D, O), shared by both row counts
# ---------------------------------------------------------------------------------------------------------------------
_SAMPLE_STEP, _SAMPLE_AUTO = {}, {}


def _sample_step(net, D, O, sd):
    key = (net, D, O)
    if key not in _SAMPLE_STEP:
        x, t = er.case_coords(net, sd, SAMPLE, D, seed=101), er.targets(SAMPLE, O, seed=102)
        m = er.relu_decisions(net, sd, x) if _is_relu(net) else None
        y64, _, g64 = er.np_step(net, sd, x, t, True, m)
        y32, _, g32 = er.np_step(net, sd, x, t, False, m)
        _SAMPLE_STEP[key] = (relmax(y32, y64), {k: relmax(_pairs(g32[k]), _pairs(g64[k])) for k in g64})
    return _SAMPLE_STEP[key]


def _weighted(net, sd, x, w, double, masks):
    wt = torch.as_tensor(w).to(torch.float64 if double else torch.float32)
    return er.eager_grads(net, sd, x, double, lambda y, rows: (y * wt[rows]).sum(), masks)


def _sample_auto(net, D, O, sd):
    key = (net, D, O)
    if key not in _SAMPLE_AUTO:
        x = er.case_coords(net, sd, SAMPLE, D, seed=101)
        w = np.random.default_rng(103).standard_normal((SAMPLE, O))
        m = er.relu_decisions(net, sd, x) if _is_relu(net) else None
        _, gx64, g64 = _weighted(net, sd, x, w, True, m)
        _, gx32, g32 = _weighted(net, sd, x, w, False, m)
        sw = np.abs(w).sum(0).max()
        _SAMPLE_AUTO[key] = (None if gx64 is None else relmax(gx32, gx64),
                             {k: relmax(_pairs(g32[k]), _pairs(g64[k])) for k in g64},
                             {k: float(np.abs(_pairs(g32[k]) - _pairs(g64[k])).max() / sw) for k in er.final_bias_keys(net, sd)})
    return _SAMPLE_AUTO[key]


# ---------------------------------------------------------------------------------------------------------------------
# 1. the training call
# ---------------------------------------------------------------------------------------------------------------------
def _relu_step_masks(model, x, table, idx, first, weight, n):
    """The build's own relu decisions out_l > 0 of a training step, read from its activation buffer; with the final stage
    inside the forward kernel no out_L is stored, so the step runs with "fused_final" off -- the same kernel up to its tail
    (the protocol of test_gpu_timed_kernels.KIND_STEP_CASES)."""
    from wire_amd import _lib
    with tune(fused_final=0):
        r = abi_train_step(model, x, table, idx, first, weight)
    K = model._arch["width"]
    P = (K + 63) // 64 * 64
    a = r["act"].view(torch.float32)
    out = []
    for l in range(L + 1):
        off = _lib.check(r["lib"].wire_act_out_offset(C.byref(r["desc"]), n, l), "wire_act_out_offset")
        out.append((a[off:off + n * P].view(n, P)[:, :K] > 0).cpu().numpy())
    return out


def check_training_call(net, D, O, n, tag):
    model = er.build(net, D, O, DEV)
    sd = er.state(model)
    x = er.case_coords(net, sd, n, D)
    T = n + 64
    table = er.targets(T, O)
    if (D, O, n) in SHIFTED:
        idx, first, weight = None, 37, 0.5
        src = np.arange(first, first + n)
    else:
        idx, first, weight = np.random.default_rng(3).permutation(T)[:n], 0, 1.0
        src = idx
    t = table[src]
    masks = _relu_step_masks(model, x, table, idx, first, weight, n) if _is_relu(net) else None
    r = abi_train_step(model, x, table, idx, first, weight)
    y64, l64, g64 = er.np_step(net, sd, x, t, True, masks)
    y32, _, g32 = er.np_step(net, sd, x, t, False, masks)
    if masks is not None:
        own = er.relu_decisions(net, sd, x)
        diff = [m != o for m, o in zip(masks, own)]
        flips = sum(int(d.sum()) for d in diff)
        lin = wo.realnet_forward("relu", wo.cast_params(sd, True), x.astype(np.float64), L, 30.0, 30.0, 10.0,
                                 er.posenc_freqs(net, D), keep=True)[1]["lin"]
        flipmax = max([float(np.abs(a[d]).max()) for a, d in zip(lin, diff) if d.any()], default=0.0)
        print(f"{tag}: {flips} relu decisions differ from the fp64 oracle's, largest |lin| {flipmax:.2e}")
        assert flips <= 1e-5 * masks[0].size * (L + 1) and flipmax <= 2e-5
    s_y, s_g = _sample_step(net, D, O, sd)
    err_y_ref = max(relmax(y32, y64), s_y)
    y = r["y"]
    assert np.isfinite(y).all()
    print(f"{tag} y: build {relmax(y, y64):.3e} reference {err_y_ref:.3e}")
    within_ref(relmax(y, y64), err_y_ref, f"{tag} step y")
    assert abs(r["loss"] - weight * l64) <= 1e-5 * weight * l64, (r["loss"], weight * l64)
    # g_y = weight 2 / (n O) (y - t) of the call's own y: the factor, the difference and the product round once each.
    # (With O <= 4 the fused final stage keeps dL/dy in registers and leaves g_y alone: include/wire_hip.h.)
    if O > 4 or er.NETS[net]["kind"] in ("bspline_mscale_2", "bspline_mscale_hier", "mfn"):
        gy_own = (weight * 2.0 / (n * O)) * (y.astype(np.float64) - t)
        assert np.abs(r["gy"] - gy_own).max() <= 2.0 ** -22 * np.abs(gy_own).max()
    # the scatter: rec[src[r]] = y[r], nothing else written
    assert np.array_equal(r["rec"][src], y)
    rest = np.ones(T, bool)
    rest[src] = False
    assert np.isnan(r["rec"][rest]).all()
    bias_keys = er.final_bias_keys(net, sd)
    for k, g in r["grads"].items():
        if k not in g64:
            # bspline_mscale_HL: the frozen first stage receives no gradient and the call never writes its slots
            assert net == "bspline_mscale_HL" and k.startswith("net.0.") and np.isnan(g).all(), k
            continue
        assert np.isfinite(g).all(), k
        mine, ref, ref32 = g.ravel() / weight, _pairs(g64[k]), _pairs(g32[k])
        assert np.abs(ref).max() > 0, f"{tag} {k}: the fp64 gradient is zero (a dead net compares nothing)"
        print(f"{tag} {k}: build {relmax(mine, ref):.3e} reference {max(relmax(ref32, ref), s_g[k]):.3e}")
        if k in bias_keys:
            final_bias_within_ref(mine, ref, err_y_ref, np.abs(y64).max(), O, f"{tag} step {k}",
                                  resid_max=np.abs(y64 - t).max())
        else:
            within_ref(relmax(mine, ref), max(relmax(ref32, ref), s_g[k]), f"{tag} step {k}")
    assert set(g64) <= set(r["grads"])


@pytest.mark.parametrize("case", CASES, ids=case_id)
def test_training_call(case):
    check_training_call(*case, tag=f"envelope[{case_id(case)}]")


# ---------------------------------------------------------------------------------------------------------------------
# 2. autograd with coordinate gradients
# ---------------------------------------------------------------------------------------------------------------------
def _backward(model, x, w, want_x):
    for p in model.parameters():
        p.grad = None
    for lin in getattr(model, "linears", []):
        lin.weight.grad = lin.bias.grad = None
    xt = torch.as_tensor(x, device=DEV)[None].requires_grad_(want_x)
    y = model(xt)
    (y[0] * torch.as_tensor(w, dtype=torch.float32, device=DEV)).sum().backward()
    torch.cuda.synchronize()
    from _util import abi_names
    got = {k: t.grad for k, t in zip(abi_names(model), model.param_tensors())}
    return (None if xt.grad is None else xt.grad[0].to(torch.float64).cpu().numpy(),
            {k: (torch.view_as_real(g) if g.is_complex() else g).to(torch.float64).cpu().numpy()
             for k, g in got.items() if g is not None})


def check_autograd(net, D, O, n, tag):
    from wire_amd import _lib
    model = er.build(net, D, O, DEV)
    sd = er.state(model)
    x = er.case_coords(net, sd, n, D)
    w = np.random.default_rng(5).standard_normal((n, O))
    if net == "bspline_mscale_HL":
        # no gradient reaches the coordinates through the frozen first stage: the module detaches them (x.grad stays
        # None), and a request for g_coords through the ABI is WIRE_ERR_ARG -- decided before anything is launched
        gx, got = _backward(model, x, w, True)
        assert gx is None
        lib, desc, xd, nn_, nat, packed, act, ab, s = cg._abi_forward(model, torch.as_tensor(x))
        gyd = torch.as_tensor(w, dtype=torch.float32, device=DEV).contiguous()
        sb = lib.wire_bwd_coords_scratch_bytes(C.byref(desc), n)
        scr = torch.empty(max(sb, 1), dtype=torch.uint8, device=DEV)
        grads = [torch.empty_like(p) for p in nat]
        gxd = torch.full((n, D), float("nan"), device=DEV)
        rc = lib.wire_mlp_bwd_coords(s, C.byref(desc), packed.data_ptr(), xd.data_ptr(), n, gyd.data_ptr(), act.data_ptr(),
                                     ab, scr.data_ptr(), sb, _lib.ptr_array([g.data_ptr() for g in grads]),
                                     gxd.data_ptr())
        torch.cuda.synchronize()
        assert rc == -1, (rc, lib.wire_last_error())                      # WIRE_ERR_ARG
        assert bool(torch.isnan(gxd).all())
    else:
        gx, got = _backward(model, x, w, True)
    masks = cg._relu_masks(model, torch.as_tensor(x), L) if _is_relu(net) else None
    _, gx64, g64 = _weighted(net, sd, x, w, True, masks)
    _, gx32, g32 = _weighted(net, sd, x, w, False, masks)
    s_gx, s_g, s_b = _sample_auto(net, D, O, sd)
    if gx is not None:
        assert gx.shape == (n, D) and np.isfinite(gx).all()
        assert np.abs(gx64).max() > 0 and all(np.abs(gx64[:, j]).max() > 0 for j in range(D)), \
            f"{tag}: the oracle's coordinate gradient is zero (a dead net compares nothing)"
        print(f"{tag} g_coords: build {relmax(gx, gx64):.3e} reference {max(relmax(gx32, gx64), s_gx):.3e}")
        within_ref(relmax(gx, gx64), max(relmax(gx32, gx64), s_gx), f"{tag} coords_grad")
        for j in range(D):           # every coordinate lane on its own scale
            within_ref(relmax(gx[:, j], gx64[:, j]), max(relmax(gx32[:, j], gx64[:, j]), s_gx), f"{tag} coords_grad lane {j}")
    assert sorted(got) == sorted(g64), (sorted(got), sorted(g64))
    bias_keys = er.final_bias_keys(net, sd)
    for k, g in got.items():
        assert np.isfinite(g).all(), k
        mine, ref, ref32 = g.ravel(), _pairs(g64[k]), _pairs(g32[k])
        assert np.abs(ref).max() > 0, f"{tag} {k}: the fp64 gradient is zero"
        if k in bias_keys:
            # under sum(y w) this gradient is sum_n w[n, o]: O numbers that can cancel to nearly nothing, so the error is
            # taken relative to the scale of the summands, max_o sum_n |w[n, o]| (as final_bias_within_ref takes the MSE
            # step's against the scale of dL/dy); the bound is the protocol's, err_ref the eager fp32 sum's own error
            sw = np.abs(w).sum(0).max()
            within_ref(np.abs(mine - ref).max() / sw, max(np.abs(ref32 - ref).max() / sw, s_b[k]),
                       f"{tag} autograd {k} [over sum|w|]")
        else:
            within_ref(relmax(mine, ref), max(relmax(ref32, ref), s_g[k]), f"{tag} autograd {k}")


@pytest.mark.parametrize("case", CASES, ids=case_id)
def test_autograd_with_coordinate_gradients(case):
    check_autograd(*case, tag=f"envelope[{case_id(case)}]")


# ---------------------------------------------------------------------------------------------------------------------
# 3. inference
# ---------------------------------------------------------------------------------------------------------------------
def check_inference(net, D, O, n, tag):
    from wire_amd import _lib
    lib = _lib.lib()
    model = er.build(net, D, O, DEV)
    sd = er.state(model)
    x = er.case_coords(net, sd, n, D)
    t = er.targets(n, O)
    y64, y32 = er.np_step(net, sd, x, t, True)[0], er.np_step(net, sd, x, t, False)[0]
    err_ref = max(relmax(y32, y64), _sample_step(net, D, O, sd)[0])
    desc = model.net_desc()
    dp = C.byref(desc)
    xt = torch.as_tensor(x, device=DEV).contiguous()
    nat = [p.detach().contiguous() for p in model.param_tensors()]
    s = torch.cuda.current_stream().cuda_stream
    packed = torch.empty(lib.wire_packed_floats(dp), dtype=torch.float32, device=DEV)
    _lib.check(lib.wire_pack_params(s, dp, _lib.ptr_array([p.data_ptr() for p in nat]), packed.data_ptr()), "pack")
    ab = _lib.check(lib.wire_act_bytes(dp, n, 0), "wire_act_bytes")
    act = torch.empty(ab, dtype=torch.uint8, device=DEV)
    y = torch.full((n, O), float("nan"), device=DEV)
    _lib.check(lib.wire_mlp_fwd(s, dp, packed.data_ptr(), xt.data_ptr(), n, y.data_ptr(), act.data_ptr(), ab, 0), "fwd")
    torch.cuda.synchronize()
    y = y.cpu().numpy()
    assert np.isfinite(y).all(), f"{tag}: {int((~np.isfinite(y)).sum())} elements of y were not written"
    within_ref(relmax(y, y64), err_ref, f"{tag} inference y")


@pytest.mark.parametrize("case", CASES, ids=case_id)
def test_inference(case):
    check_inference(*case, tag=f"envelope[{case_id(case)}]")


# ---------------------------------------------------------------------------------------------------------------------
# 4. the other GEMM families at D = 4, O = 5
# ---------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("check", [check_training_call, check_autograd, check_inference], ids=lambda f: f.__name__)
@pytest.mark.parametrize("fam", ["x3", "3m", "4m"])
def test_gemm_families(fam, check):
    with family_ctx(fam):
        check(*FAMILY_CASE, tag=f"envelope[{case_id(FAMILY_CASE)} {fam}]")


# ---------------------------------------------------------------------------------------------------------------------
# 5. the positional encoding alone at D = 4
# ---------------------------------------------------------------------------------------------------------------------
def test_posencoding_alone_d4():
    """wire_posenc_fwd / wire_posenc_bwd at D = 4, F = 3 (28 columns) against the oracle's posenc; the tolerance of
    test_gpu_coords_grad.test_posencoding_alone."""
    from wire_amd.modules.relu import PosEncoding
    D, F, n = 4, 3, 4096 + 37
    pe = PosEncoding(D, sidelength=256)
    pe.num_frequencies, pe.out_dim = F, D + 2 * D * F
    coords = cg._coords(n, D)
    w = torch.randn(n, pe.out_dim, dtype=torch.float64, generator=torch.Generator().manual_seed(7))
    x = coords.to(torch.float32).to(DEV).reshape(1, n, D).requires_grad_(True)
    out = pe(x)
    (out * w.to(torch.float32).to(DEV)).sum().backward()
    c32 = coords.to(torch.float32).numpy()
    o64, o32 = wo.posenc(c32.astype(np.float64), F), wo.posenc(c32, F)
    got = out.detach().reshape(n, pe.out_dim).cpu().numpy()
    assert got.shape == o64.shape and np.array_equal(got[:, :D], c32)
    within_ref(relmax(got, o64), relmax(o32, o64), "envelope posenc D=4 F=3 fwd")
    fwd = lambda c, double, rows=None: torch_ref.posenc(c, F)
    g64, g32 = cg.oracle_coords_grad(fwd, coords, w, True), cg.oracle_coords_grad(fwd, coords, w, False)
    assert all(np.abs(g64[:, j]).max() > 0 for j in range(D))
    within_ref(relmax(x.grad.reshape(n, D).cpu().numpy(), g64), relmax(g32, g64), "envelope posenc D=4 F=3 coords_grad")


# ---------------------------------------------------------------------------------------------------------------------
# 6. which kernels these shapes launch
# ---------------------------------------------------------------------------------------------------------------------
def _step_kernels(net, D, O, n=4096 + 37):
    model = er.build(net, D, O, DEV)
    x, table = er.coords(n, D), er.targets(n, O)
    return _nt_editions(lambda: abi_train_step(model, x, table))


EPI_BWD_FIRST, EPI_D2, EPI_D3 = 3, 128, 256                    # wire_gemm.h, as test_gpu_bwd_epilogues names them
WHOLE_NET = ("fused_fwd_kernel", "fused_bwd_kernel", "final_fused_kernel")


def test_routes():
    from wire_amd import _lib
    has = lambda names, what: any(what in k for k in names)
    # D = 4: the plain four-term first-layer data gradient although the knob of the compile-time editions is on
    assert _lib.lib().wire_tune_get(b"first_dn") == 1
    codes, names = _step_kernels("wire_k256", 4, 2)
    first = {c for c in codes if c & 63 == EPI_BWD_FIRST}
    assert first and not any(c & (EPI_D2 | EPI_D3) for c in first), (sorted(codes), sorted(set(names)))
    # ... while D = 2 at the same shape takes the D2 edition (the check can tell them apart)
    codes2, _ = _step_kernels("wire_k256", 2, 2)
    assert any(c & 63 == EPI_BWD_FIRST and c & EPI_D2 for c in codes2), sorted(codes2)
    # O = 2: the fused final stage (this net) or the whole-net training kernel
    assert has(names, "final_fused_kernel") or has(names, "fused_fwd_kernel"), sorted(set(names))
    # O = 5: the unfused sequence and no whole-net kernel
    for net in ("wire_k256", "wire_k90", "siren"):
        _, names5 = _step_kernels(net, 4, 5)
        assert has(names5, "final_fwd_kernel") and has(names5, "final_bwd_kernel"), (net, sorted(set(names5)))
        assert not any(has(names5, k) for k in WHOLE_NET), (net, sorted(set(names5)))
    # a real net at O = 2: the data-gradient chain (and with it the whole-net training forward that feeds it)
    _, names_s = _step_kernels("siren", 4, 2)
    assert has(names_s, "fused_bwd_kernel"), sorted(set(names_s))
