"""CPU-only checks of the differentiable SSIM loss: the closed form the kernels implement against fp64 autograd of the
restatement (tests/ssim_grad_ref.py), the new C-ABI symbols and their argument checks (they return before any HIP call),
and the refusals of functional.ssim_loss and FusedTrainer.step_ssim."""
import ctypes as C
import math

import numpy as np
import pytest
import torch

import ssim_grad_ref as gref
import ssim_ref as ref

# the shapes of tests/test_gpu_ssim.py and the ones tests/test_gpu_ssim_loss.py adds for the gradient's own tiles
SHAPES = [(11, 11, 1), (7, 7, 1), (12, 29, 3), (33, 8, 2), (15, 16, 8), (47, 81, 3), (17, 44, 8), (18, 45, 5),
          (18, 35, 2), (49, 99, 1)]
CASES = [(s, k) for s in SHAPES for k in ("gaussian", "uniform") if min(s[0], s[1]) >= len(ref.window(k)[0])]
NEW = ("wire_ssim_bwd_ws_bytes", "wire_ssim_bwd", "wire_ssim_mse_grad_ws_bytes", "wire_ssim_mse_grad")


@pytest.mark.parametrize("shape,kind", CASES)
def test_closed_form_matches_fp64_autograd(shape, kind):
    """(T(A) + 2 y T(B) + x T(C)) / (Ho Wo O) == autograd of the restatement's mean, to 1e-12 of max|g|."""
    for sigma in ref.SIGMAS:
        c = gref.case(shape, sigma, kind)
        g = gref.closed_form_grad(c["gt"], c["rec"], c["win"], c["cov"], c["data_range"])
        err = np.abs(g - c["g64"]).max() / np.abs(c["g64"]).max()
        print(f"closed form {shape} {kind} sigma={sigma}: {err:.2e} of max|g|; fp32 autograd {c['err_ref']:.2e}")
        assert g.shape == shape and err <= 1e-12


def test_one_window_is_a_scaled_outer_product():
    """An image of exactly one window: A, B and C are scalars, so the gradient is the outer product of the taps times
    (A + 2 B y + C x) -- it lies in the span of three known images."""
    for shape, kind in (((11, 11, 1), "gaussian"), ((7, 7, 1), "uniform")):
        c = gref.case(shape, 0.1, kind)
        w = c["win"].double().numpy()
        ww = np.outer(w, w)
        g = c["g64"][:, :, 0]
        x, y = c["gt"][:, :, 0].astype(np.float64), c["rec"][:, :, 0].astype(np.float64)
        basis = np.stack([ww.ravel(), (2 * y * ww).ravel(), (x * ww).ravel()], 1)
        coef, res, *_ = np.linalg.lstsq(basis, g.ravel(), rcond=None)
        assert np.abs(basis @ coef - g.ravel()).max() <= 1e-12 * np.abs(g).max()


def test_regularised_loss_restatement():
    """ssim_mse_loss_and_grad: loss = mse + lam (1 - ssim); with no rows the gradient is -lam dssim/dy, with lam = 0 the
    plain MSE gradient on the selected rows and zero elsewhere."""
    H, W, O = 20, 13, 3
    gt, rec = ref.inputs((H, W, O), 0.1)
    win, cov = ref.window("gaussian")
    rows = np.random.default_rng(1).permutation(H * W)[:100]
    g, _ = gref.autograd_grad(gt, rec, win, cov, 1.0, torch.float64)
    loss, mse, ssim, gy = gref.ssim_mse_loss_and_grad(rec, gt, rows, 0.25, H, W, O, win, cov, 1.0)
    assert abs(loss - (mse + 0.25 * (1 - ssim))) <= 1e-14
    _, m0, _, g0 = gref.ssim_mse_loss_and_grad(rec, gt, [], 0.25, H, W, O, win, cov, 1.0)
    assert m0 == 0 and np.abs(g0 + 0.25 * g.reshape(H * W, O)).max() <= 1e-15
    _, _, _, g1 = gref.ssim_mse_loss_and_grad(rec, gt, rows, 0.0, H, W, O, win, cov, 1.0)
    want = np.zeros((H * W, O))
    d = rec.reshape(H * W, O).astype(np.float64) - gt.reshape(H * W, O)
    want[rows] = 2 * d[rows] / (len(rows) * O)
    assert np.abs(g1 - want).max() <= 1e-15
    assert np.abs(gy - (g1 + g0)).max() <= 1e-15


def test_abi_symbols_and_workspace_sizes():
    from wire_amd import _lib
    L = _lib.lib()
    for name in NEW:
        assert name in _lib.SYMBOLS and hasattr(L, name)
    assert L.wire_abi_version() == 1
    for fn in (L.wire_ssim_bwd_ws_bytes, L.wire_ssim_mse_grad_ws_bytes):
        prev = 0
        for n in (11, 12, 27, 43, 100, 512, 4096):
            b = fn(n, n, 3, 11)
            assert b > 0 and b >= prev
            prev = b
        for bad in [(10, 40, 3, 11), (40, 10, 3, 11), (40, 40, 0, 11), (40, 40, 9, 11), (40, 40, 3, 4), (40, 40, 3, 1),
                    (40, 40, 3, 13)]:
            assert fn(*bad) == -1
            assert b"_ws_bytes" in L.wire_last_error()
    # the fused call keeps two partial sums per tile of 16 x 32 input pixels (at least 1024 for the rows of an index list)
    assert L.wire_ssim_mse_grad_ws_bytes(512, 512, 3, 11) >= 2 * 32 * 16 * 4


def test_abi_rejects_bad_arguments_before_any_hip_call():
    """Every refusal of include/wire_hip.h, on a machine without a GPU: the pointers are never dereferenced."""
    from wire_amd import _lib
    L = _lib.lib()
    win = (C.c_float * 11)(*ref.window("gaussian")[0].tolist())
    p = 4096                                  # stands for a device pointer; never read
    shape_bad = [dict(taps=4), dict(taps=10), dict(taps=1), dict(taps=13), dict(H=10), dict(W=10),
                 dict(H=6, W=6, taps=7), dict(O=0), dict(O=9),
                 dict(c1=math.nan), dict(c1=math.inf), dict(c2=math.nan), dict(c2=-math.inf), dict(cov=math.nan),
                 dict(cov=math.inf), dict(window=None), dict(ws=None)]

    def run(fn, name, good, bad, ws_bytes):
        order = list(good)
        for change in bad:
            args = dict(good, **change)
            L.wire_tune_get(b"no such knob")       # leaves another message behind
            assert fn(*[args[k] for k in order]) == -1, (name, change)
            assert name in L.wire_last_error(), (name, change)
        args = dict(good, ws_bytes=ws_bytes - 1)
        assert fn(*[args[k] for k in order]) == -3
        assert b"ws too small" in L.wire_last_error()

    wb = L.wire_ssim_bwd_ws_bytes(40, 40, 3, 11)
    good = dict(stream=None, x=p, y=p, H=40, W=40, O=3, taps=11, window=win, cov=1.0, c1=1e-4, c2=9e-4, g_ssim=p, g_y=p,
                ws=p, ws_bytes=wb)
    run(L.wire_ssim_bwd, b"wire_ssim_bwd", good,
        shape_bad + [dict(x=None), dict(y=None), dict(g_ssim=None), dict(g_y=None)], wb)

    wf = L.wire_ssim_mse_grad_ws_bytes(40, 40, 3, 11)
    good = dict(stream=None, y=p, H=40, W=40, O=3, target=p, taps=11, window=win, cov=1.0, c1=1e-4, c2=9e-4, idx=None,
                first=0, n_mse=1600, lam=0.1, g_y=p, loss=p, rec=None, ws=p, ws_bytes=wf)
    run(L.wire_ssim_mse_grad, b"wire_ssim_mse_grad", good,
        shape_bad + [dict(y=None), dict(target=None), dict(g_y=None), dict(loss=None), dict(lam=math.nan),
                     dict(lam=math.inf), dict(lam=-math.inf), dict(n_mse=-1), dict(n_mse=1601), dict(idx=p, n_mse=1601),
                     dict(first=-1, n_mse=3), dict(first=1), dict(first=1598, n_mse=3), dict(first=1601, n_mse=0)], wf)


def test_ssim_loss_checks_its_arguments():
    from wire_amd import _lib, functional
    assert callable(functional.ssim_loss)
    a, b = torch.zeros(20 * 24, 3, requires_grad=True), torch.zeros(20 * 24, 3)
    with pytest.raises(_lib.WireHipError):
        functional.ssim_loss(a, b, 20, 24)
    with pytest.raises(_lib.WireHipError):
        functional.ssim_loss(a.reshape(20, 24, 3), b.reshape(1, 20 * 24, 3), 20, 24, window="uniform", data_range=2.0)
    with pytest.raises(ValueError, match="data_range"):
        functional.ssim_loss(a, b, 20, 24, window="uniform")
    with pytest.raises(ValueError, match="smaller than"):
        functional.ssim_loss(torch.zeros(100, 3), torch.zeros(100, 3), 10, 10)
    with pytest.raises(ValueError):
        functional.ssim_loss(a, b[:-1], 20, 24)
    with pytest.raises(ValueError):
        functional.ssim_loss(a, b, 20, 24, window=(4, 1.5))
    with pytest.raises(ValueError):
        functional.ssim_loss(a.reshape(24, 20, 3), b, 20, 24)


class _Bare:
    """The attributes step_ssim reads before it touches the device."""

    def __init__(self, grid, world=1, target=True, O=3):
        self.grid, self.world, self.O = grid, world, O
        self.tz = object() if len(grid) == 3 else None
        self.target = torch.zeros(grid[0] * grid[1], O) if target else None


def test_step_ssim_refusals_without_a_device():
    """A 3-D grid, target=None, a grid smaller than the window, a bad window, a uniform window without data_range,
    indices that are not a 1-D contiguous CUDA int64 tensor, a range outside the grid and a non-finite lambda_ssim are
    ValueErrors that name the argument; world > 1 is NotImplementedError."""
    from wire_amd.trainer import FusedTrainer

    def step(bare, *a, **kw):
        tr = object.__new__(FusedTrainer)
        tr.__dict__.update(bare.__dict__)
        return tr.step_ssim(*a, **kw)

    with pytest.raises(ValueError, match="2-D grid"):
        step(_Bare((14, 15, 16)), 0.1)
    with pytest.raises(NotImplementedError, match="step_ssim is single-process"):
        step(_Bare((14, 15), world=2), 0.1)
    with pytest.raises(ValueError, match="target"):
        step(_Bare((14, 15), target=False), 0.1)
    for bad in (float("nan"), float("inf"), -float("inf")):
        with pytest.raises(ValueError, match="lambda_ssim"):
            step(_Bare((14, 15)), bad)
    for grid in ((10, 15), (15, 10)):
        with pytest.raises(ValueError, match="smaller than"):
            step(_Bare(grid), 0.1)
    with pytest.raises(ValueError, match="smaller than"):
        step(_Bare((6, 15)), 0.1, window="uniform", data_range=2.0)
    with pytest.raises(ValueError, match="data_range"):
        step(_Bare((14, 15)), 0.1, window="uniform")
    with pytest.raises(ValueError, match="window"):
        step(_Bare((14, 15)), 0.1, window="box")
    with pytest.raises(ValueError, match="taps"):
        step(_Bare((14, 15)), 0.1, window=(4, 1.5))
    for idx in (torch.arange(4), torch.arange(4, dtype=torch.int32), torch.zeros(2, 2, dtype=torch.int64), [0, 1]):
        with pytest.raises(ValueError, match="indices"):
            step(_Bare((14, 15)), 0.1, indices=idx)
    for kw in (dict(first=-1, count=3), dict(first=208, count=3), dict(first=211), dict(count=211), dict(count=-1)):
        with pytest.raises(ValueError, match="outside the grid"):
            step(_Bare((14, 15)), 0.1, **kw)
