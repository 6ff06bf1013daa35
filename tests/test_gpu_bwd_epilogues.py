"""The data-gradient epilogues of the 16 x 16 x 32 NT GEMMs in their trimmed editions -- layer 1 with the input width a
compile-time constant (knob "first_dn", wire_gemmh_epi.h: h_gabor_bwd_first_dn / h_gabor2d_bwd_first_dn), the hidden
layers with one row block of look-ahead (knob "bwd_lookahead", h_gabor_bwd_la) -- against the plain editions they
replace: one training step and one coordinate-gradient backward must not change by a single bit, and the step's
gradients stay within the parity bound of the fp64 oracle (err_build <= 2 err_ref + 1e-6,
tests/_util.within_ref).

Every case runs the 2 x fp16 route (>= 4096 rows) on 4096 + 37 rows: 17 row tiles of 256, the last one ragged (the
epilogue's `row < M` paths and its clamped coordinate loads).  Widths: K = 256 (P = 512, what bench.py times) and
K = 181 (P = 384: pad features in the last 64-column group, 3 column tiles)."""
import numpy as np
import pytest
import torch

from _util import _nt_editions, final_bias_within_ref, oracle_grads_chunked, params_np, relmax, tune, within_ref
from oracle import wire_oracle as wo

pytestmark = pytest.mark.gpu
DEV = "cuda"
N = 4096 + 37
WIRE = dict(first_omega_0=20.0, hidden_omega_0=20.0, scale=30.0)          # bench.py's regime
# name: (get_INR kwargs, grid the batch is drawn from, knobs the case runs under)
CASES = {
    "wire_k256_d2": (dict(nonlin="wire", hidden_features=363, in_features=2, **WIRE), (80, 80), {}),
    "wire_k256_d3": (dict(nonlin="wire", hidden_features=363, in_features=3, **WIRE), (20, 20, 20), {}),
    "wire_k181_d2": (dict(nonlin="wire", hidden_features=256, in_features=2, **WIRE), (80, 80), {}),
    "wire_k181_d3": (dict(nonlin="wire", hidden_features=256, in_features=3, **WIRE), (20, 20, 20), {}),
    "wire2d_2x128_d2": (dict(nonlin="wire2d", hidden_features=128, in_features=2, first_omega_0=10.0,
                             hidden_omega_0=10.0, scale=10.0), (80, 80), {}),
    # (a real net, with the one-kernel chain off so that its data gradients run the GEMM epilogues: neither knob selects
    #  another kernel for it -- test_knobs_select_the_trimmed_editions -- so the case guards that they leave it alone)
    "siren_2x256_d2": (dict(nonlin="siren", hidden_features=256, in_features=2, first_omega_0=30.0,
                            hidden_omega_0=30.0), (80, 80), dict(fused_bwd=0)),
}
LAYERS, OUT = 2, 3


def _model(kw):
    from wire_amd.modules import models
    torch.manual_seed(5)
    return models.get_INR(out_features=OUT, hidden_layers=LAYERS, **kw).to(DEV)


def _batch(grid):
    g = torch.Generator().manual_seed(11)
    npts = int(np.prod(grid))
    return torch.rand(npts, OUT, generator=g), torch.randperm(npts, generator=g)[:N].contiguous()


KNOBS = ("first_dn", "bwd_lookahead")


def _step(kw, grid, on, knobs):
    """loss, reconstruction and flat gradient of one FusedTrainer.step (lr = 0) on N rows of the grid."""
    from wire_amd.trainer import FusedTrainer
    target, idx = _batch(grid)
    with tune(**{k: on for k in KNOBS}, **knobs):
        model = _model(kw)
        tr = FusedTrainer(model, grid, target, lr=0.0, keep_rec=True, coords_style="numpy" if len(grid) == 3 else "torch")
        loss = tr.step(idx.to(DEV))
        torch.cuda.synchronize()
        return model, tr, loss.clone(), tr.rec.clone(), tr.flat_grad.clone()


@pytest.fixture(scope="module", params=list(CASES))
def stepped(request):
    kw, grid, knobs = CASES[request.param]
    return request.param, kw, grid, _step(kw, grid, 1, knobs), _step(kw, grid, 0, knobs)


def test_knobs_are_on_by_default():
    from wire_amd import _lib
    for k in KNOBS:
        assert _lib.lib().wire_tune_get(k.encode()) == 1, k


EPI_BWD, EPI_BWD_FIRST, EPI_2D_BWD_FIRST = 2, 3, 12            # wire_gemm.h
EPI_CG, EPI_D2, EPI_D3, EPI_LA = 64, 128, 256, 512
# what the data-gradient launches of a step must be with the knobs at 1 / at 0
EDITIONS = {
    "wire_k256_d2": ({EPI_BWD | EPI_LA, EPI_BWD_FIRST | EPI_D2}, {EPI_BWD, EPI_BWD_FIRST}),
    "wire_k181_d3": ({EPI_BWD | EPI_LA, EPI_BWD_FIRST | EPI_D3}, {EPI_BWD, EPI_BWD_FIRST}),
    "wire2d_2x128_d2": ({EPI_2D_BWD_FIRST | EPI_D2}, {EPI_2D_BWD_FIRST}),
    "siren_2x256_d2": (set(), set()),
}


@pytest.mark.parametrize("name", list(EDITIONS))
def test_knobs_select_the_trimmed_editions(name):
    """The identity tests below compare two settings: here, that the settings run DIFFERENT kernels -- the flagged
    instantiations with the knobs at 1, the plain ones at 0 (and no flagged one for the real net)."""
    from wire_amd.trainer import FusedTrainer
    kw, grid, knobs = CASES[name]
    target, idx = _batch(grid)
    flags = EPI_D2 | EPI_D3 | EPI_LA
    got = []
    for on in (1, 0):
        with tune(**{k: on for k in KNOBS}, **knobs):
            tr = FusedTrainer(_model(kw), grid, target, lr=0.0, coords_style="numpy" if len(grid) == 3 else "torch")
            codes, names = _nt_editions(lambda: tr.step(idx.to(DEV)))
            assert codes, sorted(set(names))
            got.append(codes)
    want_on, want_off = EDITIONS[name]
    assert {c for c in got[0] if c & flags} == want_on, got
    assert not {c for c in got[1] if c & flags} and want_off <= got[1], got


def test_step_is_bit_identical_with_and_without_the_knobs(stepped):
    name, _, _, on, off = stepped
    for what, a, b in zip(("loss", "rec", "flat_grad"), on[2:], off[2:]):
        assert torch.equal(a, b), f"{name}: {what} differs between the knobs at 1 and at 0"
    assert bool(torch.isfinite(on[4]).all()) and float(on[4].abs().max()) > 0


def test_step_gradients_vs_fp64_oracle(stepped):
    """Knobs at 1: output and every parameter gradient of the step against the numpy fp64 oracle on the same weights;
    yardstick = the same oracle in fp32 (the bound and the final-bias form of the step cases of
    tests/test_gpu_timed_kernels.py)."""
    name, kw, grid, (model, tr, _, rec, flat), _ = stepped
    target, idx = _batch(grid)
    coords = (wo.volume_coords(*grid) if len(grid) == 3 else wo.image_coords(*grid))[idx.numpy()]
    tgt = target.numpy()[idx.numpy()]
    P = params_np(model)
    a = (kw["nonlin"], P, coords, tgt, LAYERS, kw["first_omega_0"], kw["hidden_omega_0"], kw.get("scale", 10.0))
    y64, _, g64 = oracle_grads_chunked(*a, True)
    y32, _, g32 = oracle_grads_chunked(*a, False)
    tag = f"bwd_epilogues[{name}]"
    err_y_ref = relmax(y32, y64)
    within_ref(relmax(rec.cpu().numpy()[idx.numpy()], y64), err_y_ref, tag + " y")
    flat = flat.cpu().numpy()
    names = [k for k in model.state_dict().keys() if "omega_0" not in k and "scale_0" not in k]
    assert set(names) == set(g64.keys())
    for pname, off in zip(names, tr.offsets):
        ref = wo.as_real_pairs(g64[pname]).astype(np.float64).ravel()
        ref32 = wo.as_real_pairs(g32[pname]).astype(np.float64).ravel()
        mine = flat[off:off + ref.size]
        if pname == f"net.{LAYERS + 1}.bias":
            final_bias_within_ref(mine, ref, err_y_ref, np.abs(y64).max(), OUT, f"{tag} grad {pname}",
                                  resid_max=np.abs(y64 - tgt).max())
        else:
            within_ref(relmax(mine, ref), relmax(ref32, ref), f"{tag} grad {pname}")


@pytest.mark.parametrize("name", list(CASES))
def test_coords_backward_is_bit_identical_with_and_without_the_knobs(name):
    """wire_mlp_bwd_coords (autograd with coords.requires_grad_()): the epilogue's EPI_CG instantiations -- the
    coordinate gradient and every parameter gradient, knobs at 1 against knobs at 0."""
    kw, _, knobs = CASES[name]
    D = kw["in_features"]
    g = torch.Generator().manual_seed(3)
    coords = (torch.rand(N, D, generator=g) * 2 - 1).to(DEV)
    w = torch.randn(N, OUT, generator=g).to(DEV)
    res = []
    for on in (1, 0):
        with tune(**{k: on for k in KNOBS}, **knobs):
            model = _model(kw)
            x = coords.clone().requires_grad_(True)
            (model(x) * w).sum().backward()
            torch.cuda.synchronize()
            res.append([x.grad.clone()] + [p.grad.clone() for p in model.parameters() if p.grad is not None])
    assert len(res[0]) == len(res[1]) > 1
    for i, (a, b) in enumerate(zip(*res)):
        assert torch.equal(a, b), f"{name}: tensor {i} (0 = g_coords) differs between the knobs at 1 and at 0"
    assert bool(torch.isfinite(res[0][0]).all()) and float(res[0][0].abs().max()) > 0
