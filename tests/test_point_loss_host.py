"""Host side of the pointwise data terms: the numpy restatement (tests/point_loss_ref.py) against torch autograd and
torch.nn's losses in fp64, the header and the ctypes binding, every refusal of wire_point_loss_grad before any HIP call
(NULL stream, host buffers), the ports of the reference's mask and noise helpers against recorded draws, and the
argument checks of functional.point_loss, FusedTrainer.step_loss and step_samples -- no device is touched."""
import ctypes as C
import inspect
import os
import re

import numpy as np
import pytest
import torch

from _util import GOLDEN, ROOT
import point_loss_ref as plr

DELTA = 0.3


def _case(seed, n=37, O=3):
    rng = np.random.default_rng(seed)
    y = rng.standard_normal((n, O)).astype(np.float32)
    t = rng.uniform(0, 1, (n, O)).astype(np.float32)
    y[3] = t[3]                                                     # ties: the subgradient of abs at 0
    return y, t, rng.uniform(-0.5, 2.0, n).astype(np.float32), rng.uniform(-0.5, 2.0, (n, O)).astype(np.float32)


def _torch_rho(kind, d, z, t):
    if kind == "mse":
        return d * d
    if kind == "l1":
        return d.abs()
    if kind == "huber":
        return torch.where(d.abs() <= DELTA, 0.5 * d * d, DELTA * (d.abs() - 0.5 * DELTA))
    return torch.clamp(z, min=0) - t * z + torch.log1p(torch.exp(-z.abs()))


@pytest.mark.parametrize("kind", plr.KINDS)
@pytest.mark.parametrize("wform", ["none", "row", "elem"])
def test_restatement_is_autograd_of_the_formula(kind, wform):
    y, t, wr, we = _case(1)
    w = {"none": None, "row": wr, "elem": we}[wform]
    loss, g = plr.loss_and_grad(y, t, w, kind, DELTA, 0.25, True)
    yt = torch.tensor(y, dtype=torch.float64, requires_grad=True)
    tt = torch.tensor(t, dtype=torch.float64)
    wt = torch.ones_like(tt) if w is None else torch.tensor(w, dtype=torch.float64).reshape(y.shape[0], -1).expand_as(tt)
    ref = 0.25 * (wt * _torch_rho(kind, yt - tt, yt, tt)).sum() / y.size
    ref.backward()
    assert abs(loss - float(ref.detach())) <= 1e-14 * abs(float(ref.detach()))
    np.testing.assert_allclose(g, yt.grad.numpy(), rtol=1e-13, atol=1e-16)
    if kind == "l1":
        assert (g[3] == 0).all() and (w is not None or not np.signbit(g[3]).any())   # (-w * +0 is -0)


@pytest.mark.parametrize("kind", plr.KINDS)
def test_restatement_is_the_torch_nn_loss(kind):
    y, t, wr, we = _case(2)
    mod = {"mse": torch.nn.MSELoss(), "l1": torch.nn.L1Loss(), "huber": torch.nn.HuberLoss(delta=DELTA),
           "logistic": torch.nn.BCEWithLogitsLoss()}[kind]
    yt = torch.tensor(y, dtype=torch.float64, requires_grad=True)
    tt = torch.tensor(t, dtype=torch.float64)
    ref = mod(yt, tt)
    ref.backward()
    loss, g = plr.loss_and_grad(y, t, None, kind, DELTA, 1.0, True)
    assert abs(loss - float(ref.detach())) <= 1e-14 * abs(float(ref.detach()))
    np.testing.assert_allclose(g, yt.grad.numpy(), rtol=1e-13, atol=1e-16)
    # with a weight: BCEWithLogitsLoss takes one; MSE is the reference's MSELoss()(out * mask, gt * mask), w = mask^2
    for w in (np.abs(wr), np.abs(we)):
        wt = torch.tensor(w, dtype=torch.float64).reshape(y.shape[0], -1).expand(*y.shape)
        yt = torch.tensor(y, dtype=torch.float64, requires_grad=True)
        if kind == "logistic":
            ref = torch.nn.BCEWithLogitsLoss(weight=wt)(yt, tt)
        elif kind == "mse":
            ref = torch.nn.MSELoss()(yt * wt.sqrt(), tt * wt.sqrt())
        elif kind == "l1":
            ref = torch.nn.L1Loss()(yt * wt, tt * wt)               # |w d| = w |d| for w >= 0
        else:
            continue
        ref.backward()
        loss, g = plr.loss_and_grad(y, t, w, kind, DELTA, 1.0, True)
        assert abs(loss - float(ref.detach())) <= 1e-13 * abs(float(ref.detach()))
        np.testing.assert_allclose(g, yt.grad.numpy(), rtol=1e-12, atol=1e-15)


def test_fp32_twin_is_close_and_logistic_is_finite():
    y, t, wr, _ = _case(3)
    for kind in plr.KINDS:
        l64, g64 = plr.loss_and_grad(y, t, wr, kind, DELTA, 1.0, True)
        l32, g32 = plr.loss_and_grad(y, t, wr, kind, DELTA, 1.0, False)
        assert g32.dtype == np.float32 and g64.dtype == np.float64
        assert abs(l32 - l64) <= 1e-5 * abs(l64) and np.abs(g32 - g64).max() <= 1e-6 * np.abs(g64).max()
    z = np.array([[0, 1e-8, -1e-8, 20, -20, 100, -100, 1e4, -1e4]], np.float32).T.repeat(3, 1)
    tt = np.array([[0, 0.3, 1]], np.float32).repeat(9, 0)
    for double in (True, False):
        loss, g = plr.loss_and_grad(z, tt, None, "logistic", 1.0, 1.0, double)
        assert np.isfinite(loss) and np.isfinite(g).all()


# ---------------------------------------------------------------------------------------------------------------------
# header, binding, refusals
# ---------------------------------------------------------------------------------------------------------------------
PARAMS = ["stream", "kind", "delta", "y", "target", "weight", "weight_per_elem", "idx", "first", "n", "O", "shard", "g_y",
          "loss_out", "rec", "partial"]


def test_header_declares_the_entry_point_and_lib_binds_it():
    from wire_amd import _lib
    text = open(os.path.join(ROOT, "include", "wire_hip.h")).read()
    m = re.search(r"\bint\s+wire_point_loss_grad\s*\(([^)]*)\)\s*;", text)
    assert m, "include/wire_hip.h does not declare wire_point_loss_grad"
    args = [a.strip() for a in m.group(1).replace("\n", " ").split(",")]
    assert [a.split()[-1].lstrip("*") for a in args] == PARAMS
    L = _lib.lib()
    assert "wire_point_loss_grad" in _lib.SYMBOLS and hasattr(L, "wire_point_loss_grad")
    assert len(L.wire_point_loss_grad.argtypes) == len(PARAMS)
    for name, code in (("MSE", "mse"), ("L1", "l1"), ("HUBER", "huber"), ("LOGISTIC", "logistic")):
        m = re.search(r"\bWIRE_LOSS_" + name + r"\s*=\s*(\d+)", text)
        assert m and int(m.group(1)) == _lib.LOSS_KIND[code], name
    assert L.wire_abi_version() == 1 and _lib.ABI_VERSION == 1
    srcs = re.search(r"^SRCS\s*=(.*)$", open(os.path.join(ROOT, "wire_amd", "csrc", "Makefile")).read(), re.M).group(1)
    assert "wire_loss.hip" in srcs.split()


def test_wire_point_loss_grad_refuses_bad_arguments():
    from wire_amd import _lib
    L = _lib.lib()
    buf = (C.c_float * 4096)()
    p = C.addressof(buf)
    nan, inf = float("nan"), float("inf")

    def op(kind=2, delta=0.5, y=p, t=p, w=p, wpe=0, idx=None, first=0, n=4, O=3, shard=1.0, g=p, loss=p, rec=None, part=p):
        return L.wire_point_loss_grad(None, kind, delta, y, t, w, wpe, idx, first, n, O, shard, g, loss, rec, part)

    for kw in (dict(kind=-1), dict(kind=4), dict(kind=99), dict(n=-1), dict(O=0), dict(O=-2),
               dict(delta=0.0), dict(delta=-1.0), dict(delta=nan), dict(delta=inf), dict(delta=-inf),
               dict(shard=nan), dict(shard=inf), dict(shard=-inf), dict(kind=0, shard=nan), dict(kind=3, shard=inf),
               dict(wpe=2), dict(wpe=-1), dict(wpe=2, w=None),
               dict(y=None), dict(t=None), dict(g=None), dict(loss=None), dict(part=None),
               dict(kind=0, w=None, y=None), dict(kind=0, w=None, part=None)):
        assert op(**kw) == -1, kw
        assert b"wire_point_loss_grad" in L.wire_last_error()
    # delta is read by Huber alone, and n == 0 is WIRE_OK without a launch (a NULL stream, host buffers: nothing ran)
    buf[0] = 7.0
    for kind in (0, 1, 3):
        for delta in (0.0, -1.0, nan):
            assert op(kind=kind, delta=delta, n=0) == 0
    assert op(n=0) == 0 and op(n=0, w=None, wpe=1) == 0 and buf[0] == 7.0


# ---------------------------------------------------------------------------------------------------------------------
# the ports of the reference's helpers
# ---------------------------------------------------------------------------------------------------------------------
def test_inpainting_masks_and_impulse_noise_match_the_recorded_draws():
    from wire_amd.modules import utils
    z = np.load(os.path.join(GOLDEN, "inpaint_masks.npz"), allow_pickle=False)
    H, W = (int(v) for v in z["imsize"])
    assert (H, W) == (16, 12)
    for kind in ("random2d", "random1d", "bayer"):
        np.random.seed(int(z["seed_" + kind]))
        m = utils.get_inpainting_mask((H, W), kind, float(z["mask_frac"]))
        assert m.dtype == np.float32 and m.shape == (H, W)
        assert np.array_equal(m, z["mask_" + kind]), kind
        assert np.random.rand() == float(z["next_" + kind]), f"{kind}: np.random consumption differs"
        assert set(np.unique(m)) <= {0.0, 1.0}
    assert (z["mask_random1d"] == z["mask_random1d"][0]).all() and z["mask_bayer"].sum() == (H // 2) * (W // 2)
    np.random.seed(int(z["sp_seed"]))
    noisy = utils.add_salt_and_pepper_noise(z["sp_image"], float(z["salt_prob"]), float(z["pepper_prob"]))
    assert noisy.dtype == np.uint8 and np.array_equal(noisy, z["sp_noisy"])
    assert np.random.rand() == float(z["sp_next"])
    assert not np.shares_memory(noisy, z["sp_image"])
    with pytest.raises(ValueError, match="mask_type"):
        utils.get_inpainting_mask((H, W), "checker")
    assert list(inspect.signature(utils.get_inpainting_mask).parameters) == ["imsize", "mask_type", "mask_frac"]
    assert list(inspect.signature(utils.add_salt_and_pepper_noise).parameters) == ["image", "salt_prob", "pepper_prob"]


def test_rsnr_is_its_formula():
    from wire_amd.modules import utils
    rng = np.random.default_rng(4)
    x = rng.standard_normal((5, 7, 3))
    xhat = x + 0.01 * rng.standard_normal(x.shape)
    want = 20 * np.log10(np.sqrt((x ** 2).sum()) / np.sqrt(((x - xhat) ** 2).sum()))
    assert abs(utils.rsnr(x, xhat) - want) < 1e-12
    assert abs(utils.rsnr(x, 0.9 * x) - 20.0) < 1e-9              # ||x|| / ||0.1 x|| = 10
    assert list(inspect.signature(utils.rsnr).parameters) == ["x", "xhat"]


# ---------------------------------------------------------------------------------------------------------------------
# the Python layer refuses before it touches a device
# ---------------------------------------------------------------------------------------------------------------------
def test_point_loss_refuses_without_a_device():
    from wire_amd import _lib, functional
    y, t = torch.zeros(5, 3), torch.zeros(5, 3)
    for kind in ("L1", "bce", None, 1):
        with pytest.raises(ValueError, match="kind"):
            functional.point_loss(y, t, kind)
    for delta in (0.0, -1.0, float("nan"), float("inf")):
        with pytest.raises(ValueError, match="delta"):
            functional.point_loss(y, t, "huber", delta=delta)
    with pytest.raises(ValueError, match="y must be"):
        functional.point_loss(y.double(), t)
    with pytest.raises(ValueError, match="y must be"):
        functional.point_loss(y.reshape(-1), t)
    with pytest.raises(ValueError, match="y must be"):
        functional.point_loss(torch.zeros(3, 5).t(), t)
    with pytest.raises(ValueError, match="target must be"):
        functional.point_loss(y, torch.zeros(5, 2))
    with pytest.raises(ValueError, match="target must be"):
        functional.point_loss(y, t.double())
    for w in (torch.zeros(3), torch.zeros(5, 1), torch.zeros(5, 3, dtype=torch.float64), torch.zeros(3, 5).t(), 1.0):
        with pytest.raises(ValueError, match="weight must be"):
            functional.point_loss(y, t, "l1", weight=w)
    for kind in ("mse", "l1", "huber", "logistic"):                 # everything else in order: the device is what is missing
        with pytest.raises(_lib.WireHipError):
            functional.point_loss(y, t, kind, weight=torch.zeros(5))
    assert [p for p in inspect.signature(functional.point_loss).parameters] == ["y", "target", "kind", "weight", "delta"]


class _Bare:
    """The attributes the two steps read before they touch the device."""

    def __init__(self, grid=(4, 5), world=1, O=3, target=True, D=2):
        self.grid, self.world, self.O = grid, world, O
        self.npoints = int(np.prod(grid))
        self.target = torch.zeros(self.npoints, O) if target else None
        self.rec = None
        self.desc = type("D", (), {"in_features": D})()


def _call(name, bare, *a, **kw):
    from wire_amd.trainer import FusedTrainer
    tr = object.__new__(FusedTrainer)
    tr.__dict__.update(bare.__dict__)
    return getattr(tr, name)(*a, **kw)


def test_steps_refuse_without_a_device():
    from wire_amd.trainer import FusedTrainer
    sig = inspect.signature(FusedTrainer.step_loss)
    assert list(sig.parameters)[1:] == ["kind", "indices", "first", "count", "weight", "delta"]
    assert sig.parameters["delta"].default == 1.0 and sig.parameters["weight"].default is None
    sig = inspect.signature(FusedTrainer.step_samples)
    assert list(sig.parameters)[1:] == ["coords", "values", "kind", "weight", "delta"]
    assert sig.parameters["kind"].default == "mse"
    xy, val = torch.zeros(6, 2), torch.zeros(6, 3)
    for name, args in (("step_loss", ()), ("step_samples", (xy, val))):
        with pytest.raises(NotImplementedError, match="single-process"):
            _call(name, _Bare(world=2), *args, kind="l1")
        with pytest.raises(ValueError, match="kind"):
            _call(name, _Bare(), *args, kind="l2")
        for delta in (0.0, float("nan"), float("inf"), -2.0):
            with pytest.raises(ValueError, match="delta"):
                _call(name, _Bare(), *args, kind="huber", delta=delta)
    with pytest.raises(ValueError, match="needs the trainer's target"):
        _call("step_loss", _Bare(target=False), "l1")
    with pytest.raises(ValueError, match="outside the grid"):
        _call("step_loss", _Bare(), "l1", first=15, count=6)
    with pytest.raises(ValueError, match="outside the grid"):
        _call("step_loss", _Bare(), "l1", first=-1, count=2)
    with pytest.raises(ValueError, match="at least one row"):
        _call("step_loss", _Bare(), "l1", first=3, count=0)
    with pytest.raises(ValueError, match="indices must be"):
        _call("step_loss", _Bare(), "l1", indices=torch.arange(4))
    for w in (torch.zeros(19), torch.zeros(20, 2), torch.zeros(20, dtype=torch.float64), [1.0] * 20):
        with pytest.raises(ValueError, match="weight must be"):
            _call("step_loss", _Bare(), "logistic", weight=w)
    # step_samples: a CPU tensor, a wrong dtype, width, rank or stride is named
    for c in (xy, xy.double(), torch.zeros(6, 3), torch.zeros(12), torch.zeros(2, 6).t(), torch.zeros(0, 2), None):
        with pytest.raises(ValueError, match="coords must be"):
            _call("step_samples", _Bare(target=False), c, val)
