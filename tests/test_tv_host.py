"""CPU-only checks of the total-variation regulariser: the restatement of tests/tv_ref.py against the value and the
autograd gradient the reference itself produces (tests/golden/tv.npz), the three new entry points' refusal of bad
arguments (before any HIP call, so on a machine without a GPU), and the refusals of FusedTrainer.step_tv and of the
drop-in function that need no device."""
import ctypes as C

import numpy as np
import pytest
import torch

from _util import ROOT, load_golden  # noqa: F401  (puts the repository on sys.path)
import tv_ref as ref


def test_restatement_reproduces_golden_value():
    """The same torch expression in fp32 gives the reference's bits; the fp64 restatement (numpy and torch) is within
    1e-6 relative; the image holds ties, so s(0) occurs."""
    z = load_golden("tv")
    img = z["image"]
    assert img.shape == (1, 3, 37, 29) and img.dtype == np.float32 and z["tv"].dtype == np.float32
    t32 = ref.total_variation(torch.tensor(img), double=False)
    assert t32.dtype == torch.float32 and t32.numpy().tobytes() == z["tv"].tobytes()
    for tv64 in (float(ref.total_variation(img, True)), float(ref.total_variation(torch.tensor(img), True))):
        assert abs(tv64 - float(z["tv"])) <= 1e-6 * tv64
    n32 = ref.total_variation(img, double=False)
    assert n32.dtype == np.float32 and abs(float(n32) - float(z["tv"])) <= 1e-6 * float(z["tv"])
    for c, i, j, right in z["ties"]:
        assert img[0, c, i + (1 - right), j + right] == img[0, c, i, j]


def test_closed_form_gradient_equals_golden_gradient():
    """The closed form equals the reference's autograd gradient exactly, in fp32 and fp64, and scales with g."""
    z = load_golden("tv")
    k = ref.tv_sign_pattern(z["image"])
    assert k.dtype == np.int8 and np.abs(k).max() == 4
    assert np.array_equal(ref.total_variation_grad(z["image"], 1.0, False), z["grad"])
    assert np.array_equal(ref.total_variation_grad(z["image"], 1.0, True), z["grad"].astype(np.float64))
    assert np.array_equal(ref.total_variation_grad(z["image"], 0.25, False), 0.25 * z["grad"])
    # a tie contributes nothing: the pattern of a constant image is zero, and H == 1 / W == 1 have one direction only
    assert not ref.tv_sign_pattern(np.ones((2, 4, 5), np.float32)).any()
    row = np.array([[1.0, 3.0, 2.0]], np.float32)
    assert np.array_equal(ref.tv_sign_pattern(row), [[-1, 2, -1]])
    assert np.array_equal(ref.tv_sign_pattern(row.T), [[-1], [2], [-1]])
    assert float(ref.total_variation(row)) == 3.0 and float(ref.total_variation(np.zeros((1, 1)))) == 0.0


def test_regularised_loss_restatement_matches_autograd():
    """tv_mse_loss_and_grad in fp64 == the torch expression of the loop (mse on the selected rows + lambda * the
    reference's TV on the permuted view) with autograd, to 1e-12; unselected rows carry lambda * the integer pattern."""
    H, W, O, lam = 6, 5, 3, 2.0 ** -4
    rng = np.random.default_rng(3)
    y = np.round(rng.standard_normal((H * W, O)) * 4) / 4
    t = rng.standard_normal((H * W, O))
    rows = rng.permutation(H * W)[:11]
    yt = torch.tensor(y, requires_grad=True)
    img = yt.reshape(1, H, W, O).permute(0, 3, 1, 2)
    loss = ((yt[rows] - torch.tensor(t)[rows]) ** 2).mean() + lam * ref.total_variation(img, True)
    loss.backward()
    l64, mse, tv, g64 = ref.tv_mse_loss_and_grad(y, t, rows, lam, H, W, O, double=True)
    assert abs(loss.item() - l64) <= 1e-12 * abs(l64) and abs(mse + lam * tv - l64) <= 1e-12 * abs(l64)
    assert np.abs(yt.grad.numpy() - g64).max() <= 1e-12 * np.abs(g64).max()
    rest = np.setdiff1d(np.arange(H * W), rows)
    k = ref.tv_sign_pattern(ref.channel_first(y, H, W, O)).transpose(1, 2, 0).reshape(H * W, O)
    assert np.array_equal(g64[rest], lam * k[rest]) and (k == 0).any()
    # no rows: the TV term alone and mse == 0; pattern_from replaces the comparisons' image
    l0, m0, tv0, g0 = ref.tv_mse_loss_and_grad(y, t, [], lam, H, W, O, double=False)
    assert m0 == 0 and l0 == np.float32(lam) * tv0 and np.array_equal(g0, (lam * k).astype(np.float32))
    _, _, _, gp = ref.tv_mse_loss_and_grad(y + 1e-9 * rng.standard_normal(y.shape), t, [], lam, H, W, O, True,
                                           pattern_from=y)
    assert np.array_equal(gp, lam * k)


def test_new_entry_points_refuse_bad_arguments():
    """wire_tv_fwd, wire_tv_bwd and wire_tv_mse_grad return -1 and name themselves in wire_last_error(), before any HIP
    call (NULL stream, host buffers): H, W, planes or O < 1, O > 8, n_mse < 0, a range outside the grid, strides < 1
    and a NULL pointer other than idx / rec."""
    from wire_amd import _lib
    L = _lib.lib()
    buf = (C.c_float * 4096)()
    p = C.addressof(buf)

    def fwd(fn, x=p, planes=3, H=4, W=5, ps=3, qs=1, a=p, b=p):
        return fn(None, x, planes, H, W, ps, qs, a, b)

    for fn, name in ((L.wire_tv_fwd, b"wire_tv_fwd"), (L.wire_tv_bwd, b"wire_tv_bwd")):
        for kw in (dict(planes=0), dict(H=0), dict(W=0), dict(planes=-1), dict(H=-3), dict(W=-1), dict(ps=0), dict(qs=0),
                   dict(ps=-1), dict(qs=-5), dict(x=None), dict(a=None), dict(b=None),
                   dict(H=1 << 30, W=1 << 30, ps=1 << 40), dict(planes=1 << 30, qs=1 << 62)):
            assert fwd(fn, **kw) == -1, (name, kw)
            assert name in L.wire_last_error()

    H, W, O = 4, 5, 3

    def op(y=p, H=H, W=W, O=O, t=p, idx=None, first=0, n=H * W, lam=0.5, g=p, loss=p, rec=None, part=p):
        return L.wire_tv_mse_grad(None, y, H, W, O, t, idx, first, n, lam, g, loss, rec, part)

    for kw in (dict(H=0), dict(W=0), dict(O=0), dict(O=9), dict(H=-1), dict(n=-1), dict(first=-1, n=3), dict(first=1),
               dict(first=18, n=3), dict(first=21, n=0), dict(n=H * W + 1), dict(idx=p, n=H * W + 1), dict(y=None),
               dict(t=None), dict(g=None), dict(loss=None), dict(part=None)):
        assert op(**kw) == -1, kw
        assert b"wire_tv_mse_grad" in L.wire_last_error()


class _Bare:
    """The attributes step_tv reads before it touches the device."""

    def __init__(self, grid, world=1, target=True):
        self.grid, self.world = grid, world
        self.tz = object() if len(grid) == 3 else None
        self.target = torch.zeros(grid[0] * grid[1], 3) if target else None


def test_step_tv_refusals_without_a_device():
    """A 3-D grid, target=None, indices that are not a 1-D contiguous CUDA int64 tensor, a range outside the grid and a
    non-finite lambda_tv are ValueErrors that name the argument; world > 1 is NotImplementedError."""
    from wire_amd.trainer import FusedTrainer

    def step(bare, *a, **kw):
        tr = object.__new__(FusedTrainer)
        tr.__dict__.update(bare.__dict__)
        return tr.step_tv(*a, **kw)

    with pytest.raises(ValueError, match="2-D grid"):
        step(_Bare((4, 5, 6)), 0.1)
    with pytest.raises(NotImplementedError, match="step_tv is single-process"):
        step(_Bare((4, 5), world=2), 0.1)
    with pytest.raises(ValueError, match="target"):
        step(_Bare((4, 5), target=False), 0.1)
    for bad in (float("nan"), float("inf"), -float("inf")):
        with pytest.raises(ValueError, match="lambda_tv"):
            step(_Bare((4, 5)), bad)
    for idx in (torch.arange(4), torch.arange(4, dtype=torch.int32), torch.zeros(2, 2, dtype=torch.int64), [0, 1]):
        with pytest.raises(ValueError, match="indices"):
            step(_Bare((4, 5)), 0.1, indices=idx)
    for kw in (dict(first=-1, count=3), dict(first=18, count=3), dict(first=21), dict(count=21), dict(count=-1)):
        with pytest.raises(ValueError, match="outside the grid"):
            step(_Bare((4, 5)), 0.1, **kw)


def test_drop_in_refuses_cpu_tensors():
    """utils.total_variation_loss exists on the drop-in modules; a CPU tensor raises WireHipError like the rest of the
    package, a wrong rank ValueError."""
    from wire_amd import _lib, functional
    from wire_amd.modules import utils
    assert callable(functional.total_variation)
    with pytest.raises(_lib.WireHipError):
        utils.total_variation_loss(torch.zeros(1, 3, 8, 8))
    with pytest.raises(ValueError):
        utils.total_variation_loss(torch.zeros(3, 8, 8))
