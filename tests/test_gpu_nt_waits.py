"""The loosened waits of the 2 x fp16 NT GEMMs (wire_gemmx2h.hip) -- knob "nt_bfirst": a stage's weight pieces go out
before the wave's own rows and the stage barrier no longer waits for the rows; knob "epi_early": the first loads of wire's
data-gradient epilogues go out under the MFMAs of the last stage (wire_gemmh_epi.h: h_pre_load) -- against the loop they
replace.
Neither changes a value: for each knob alone and for both together, one training step and one coordinate-gradient
backward must equal the run with both knobs at 0 bit for bit (loss, reconstruction, every gradient), and the step's
gradients with both at 1 stay within the parity bound of the fp64 oracle that tests/test_gpu_bwd_epilogues.py uses
(err_build <= 2 err_ref + 1e-6, tests/_util.within_ref).

Every case runs 4096 + 37 rows, the smallest batch on this route with a ragged last row tile.  Widths: K = 256
(P = 512: 16 stages, what bench.py times), K = 181 (P = 384: pad features, 3 column tiles), K = 212 (P = 448: the last
column tile is a half tile, whose second 64-column group the early loads must not touch), wire2d, and a sine net at
P = 256 with the whole-net kernels off, so that its layers run these GEMMs."""
import re

import numpy as np
import pytest
import torch

from _util import final_bias_within_ref, kernel_names, oracle_grads_chunked, params_np, relmax, tune, within_ref
from oracle import wire_oracle as wo

pytestmark = pytest.mark.gpu
DEV = "cuda"
N = 4096 + 37
GRID = (80, 80)
WIRE = dict(first_omega_0=20.0, hidden_omega_0=20.0, scale=30.0)          # bench.py's regime
EPI_BWD, EPI_BWD_FIRST, EPI_D2, EPI_LA = 2, 3, 128, 512          # wire_gemm.h
# the forms that have early loads: wire's data gradients of a training step (hidden layers with look-ahead, layer 1 at D = 2)
EARLY_FORMS = {EPI_BWD | EPI_LA, EPI_BWD_FIRST | EPI_D2}
# name: (get_INR kwargs, knobs the case runs under, EPI codes with early loads its step must launch)
CASES = {
    "wire_k256": (dict(nonlin="wire", hidden_features=363, in_features=2, **WIRE), {}, EARLY_FORMS),
    "wire_k181": (dict(nonlin="wire", hidden_features=256, in_features=2, **WIRE), {}, EARLY_FORMS),
    "wire_k212": (dict(nonlin="wire", hidden_features=300, in_features=2, **WIRE), {}, EARLY_FORMS),
    "wire2d_2x128": (dict(nonlin="wire2d", hidden_features=128, in_features=2, first_omega_0=10.0,
                          hidden_omega_0=10.0, scale=10.0), {}, set()),
    "siren_p256": (dict(nonlin="siren", hidden_features=256, in_features=2, first_omega_0=30.0,
                        hidden_omega_0=30.0), dict(fused_train=0), set()),
}
LAYERS, OUT = 2, 3
KNOBS = ("nt_bfirst", "epi_early")
SETTINGS = {"off": (0, 0), "nt_bfirst": (1, 0), "epi_early": (0, 1), "both": (1, 1)}


def _model(kw):
    from wire_amd.modules import models
    torch.manual_seed(5)
    return models.get_INR(out_features=OUT, hidden_layers=LAYERS, **kw).to(DEV)


def _batch():
    g = torch.Generator().manual_seed(11)
    npts = int(np.prod(GRID))
    return torch.rand(npts, OUT, generator=g), torch.randperm(npts, generator=g)[:N].contiguous()


def _step(kw, setting, knobs):
    """model, trainer, loss, reconstruction and flat gradient of one FusedTrainer.step (lr = 0) on N rows of the grid."""
    from wire_amd.trainer import FusedTrainer
    target, idx = _batch()
    with tune(**dict(zip(KNOBS, SETTINGS[setting])), **knobs):
        model = _model(kw)
        tr = FusedTrainer(model, GRID, target, lr=0.0, keep_rec=True, coords_style="torch")
        loss = tr.step(idx.to(DEV))
        torch.cuda.synchronize()
        return model, tr, loss.clone(), tr.rec.clone(), tr.flat_grad.clone()


def _coords_backward(kw, setting, knobs):
    """g_coords and every parameter gradient of autograd's backward (wire_mlp_bwd_coords: the EPI_CG instantiations)."""
    D = kw["in_features"]
    g = torch.Generator().manual_seed(3)
    coords = (torch.rand(N, D, generator=g) * 2 - 1).to(DEV)
    w = torch.randn(N, OUT, generator=g).to(DEV)
    with tune(**dict(zip(KNOBS, SETTINGS[setting])), **knobs):
        model = _model(kw)
        x = coords.clone().requires_grad_(True)
        (model(x) * w).sum().backward()
        torch.cuda.synchronize()
        return [x.grad.clone()] + [p.grad.clone() for p in model.parameters() if p.grad is not None]


@pytest.fixture(scope="module", params=list(CASES))
def ran(request):
    """Each net once per setting: the step and the coordinate-gradient backward."""
    kw, knobs, _ = CASES[request.param]
    return request.param, kw, {s: (_step(kw, s, knobs), _coords_backward(kw, s, knobs)) for s in SETTINGS}


def test_knobs_are_on_by_default():
    from wire_amd import _lib
    for k in KNOBS:
        assert _lib.lib().wire_tune_get(k.encode()) == 1, k


def _nt_editions(fn):
    """(EPI code, WT) -- first and last template argument (wire_gemmx2h.hip) -- of the 2 x fp16 NT GEMM kernels one
    call of fn launches."""
    names = kernel_names(fn)
    args = [m.group(1).split(",") for k in names for m in [re.search(r"gemmx2h_nt_kernel<([^>]*)>", k)] if m]
    return {(int(a[0]), int(a[-1])) for a in args}, names


X2_WT_BFIRST, X2_WT_EARLY = 1, 2                                 # wire_gemmx2h.hip


@pytest.mark.parametrize("name", list(CASES))
def test_knobs_select_the_editions(name):
    """The identity tests below compare settings: here, that the settings run DIFFERENT kernels -- every NT GEMM of a
    step is the instantiation whose wait mode WT is what the knobs ask for (early loads: the forms that have some, which
    a wire step must launch), and the plain one (WT = 0) with both knobs at 0."""
    from wire_amd.trainer import FusedTrainer
    kw, knobs, early_forms = CASES[name]
    target, idx = _batch()
    for setting, (bf, early) in SETTINGS.items():
        with tune(**dict(zip(KNOBS, (bf, early))), **knobs):
            tr = FusedTrainer(_model(kw), GRID, target, lr=0.0, coords_style="torch")
            codes, names = _nt_editions(lambda: tr.step(idx.to(DEV)))
        assert len(codes) >= 2, sorted(set(names))               # a forward and a data-gradient form at least
        assert early_forms <= {e for e, _ in codes}, (setting, sorted(codes))
        for e, wt in codes:
            want = (X2_WT_BFIRST if bf else 0) | (X2_WT_EARLY if early and e in early_forms else 0)
            assert wt == want, (setting, e, wt, sorted(codes))


@pytest.mark.parametrize("setting", [s for s in SETTINGS if s != "off"])
def test_step_is_bit_identical(ran, setting):
    name, _, runs = ran
    on, off = runs[setting][0], runs["off"][0]
    for what, a, b in zip(("loss", "rec", "flat_grad"), on[2:], off[2:]):
        assert torch.equal(a, b), f"{name}: {what} differs between {setting} and both knobs at 0"
    assert bool(torch.isfinite(on[4]).all()) and float(on[4].abs().max()) > 0


@pytest.mark.parametrize("setting", [s for s in SETTINGS if s != "off"])
def test_coords_backward_is_bit_identical(ran, setting):
    name, _, runs = ran
    on, off = runs[setting][1], runs["off"][1]
    assert len(on) == len(off) > 1
    for i, (a, b) in enumerate(zip(on, off)):
        assert torch.equal(a, b), f"{name}: tensor {i} (0 = g_coords) differs between {setting} and both knobs at 0"
    assert bool(torch.isfinite(on[0]).all()) and float(on[0].abs().max()) > 0


def test_step_gradients_vs_fp64_oracle(ran):
    """Both knobs at 1: output and every parameter gradient of the step against the numpy fp64 oracle on the same
    weights; yardstick = the same oracle in fp32 (bound and final-bias form of tests/test_gpu_bwd_epilogues.py)."""
    name, kw, runs = ran
    model, tr, _, rec, flat = runs["both"][0]
    target, idx = _batch()
    coords = wo.image_coords(*GRID)[idx.numpy()]
    tgt = target.numpy()[idx.numpy()]
    P = params_np(model)
    a = (kw["nonlin"], P, coords, tgt, LAYERS, kw["first_omega_0"], kw["hidden_omega_0"], kw.get("scale", 10.0))
    y64, _, g64 = oracle_grads_chunked(*a, True)
    y32, _, g32 = oracle_grads_chunked(*a, False)
    tag = f"nt_waits[{name}]"
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
