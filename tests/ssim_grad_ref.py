"""The gradient of the mean SSIM of tests/ssim_ref.py with respect to the reconstruction: torch autograd of
``ssim_ref.ssim_map`` on the CPU in fp64 and in fp32 (the fp32 one is the reference arithmetic whose own error is the
yardstick of the GPU tests), the closed form the kernels implement in fp64, and the loss of the SSIM-regularised step,
mse + lambda (1 - ssim), with its gradient."""
import functools
import warnings

import numpy as np
import torch
import torch.nn.functional as F

import ssim_ref as ref


def uniform_window(taps):
    """``taps`` equal fp32 weights with the sample covariance, as functional._ssim_window((taps, None))"""
    return torch.full((taps,), 1.0 / taps, dtype=torch.float32), taps * taps / (taps * taps - 1.0)


def _map(x, y, win, cov, data_range, dtype):
    """ssim_ref.ssim_map's map with its graph (the float() of its mean warns when the map requires a gradient)"""
    with warnings.catch_warnings():
        warnings.simplefilter("ignore", UserWarning)
        return ref.ssim_map(x, y, win, cov, data_range, dtype)[1]


def autograd_grad(gt, rec, win, cov, data_range, dtype):
    """d mean(S) / d rec by autograd through ssim_ref.ssim_map in ``dtype``; returns (gradient [H, W, O] as a float64
    array, mean as a float)."""
    y = torch.as_tensor(rec).to(dtype).clone().requires_grad_(True)
    mean = _map(gt, y, win, cov, data_range, dtype).mean()
    mean.backward()
    return y.grad.numpy().astype(np.float64), float(mean.detach())


def closed_form_grad(gt, rec, win, cov, data_range):
    """The closed form in fp64: A, B, C over the valid region, T = the transpose of the separable valid convolution
    (conv_transpose2d with the same window), g = (T(A) + 2 y T(B) + x T(C)) / (Ho Wo O).  Returns [H, W, O]."""
    dt = torch.float64
    x = torch.as_tensor(gt).to(dt).permute(2, 0, 1).unsqueeze(1)
    y = torch.as_tensor(rec).to(dt).permute(2, 0, 1).unsqueeze(1)
    w = torch.as_tensor(win).to(dt)
    wv, wh = w.reshape(1, 1, -1, 1), w.reshape(1, 1, 1, -1)
    m = lambda t: F.conv2d(F.conv2d(t, wv), wh)
    T = lambda t: F.conv_transpose2d(F.conv_transpose2d(t, wh), wv)
    c1, c2 = (0.01 * data_range) ** 2, (0.03 * data_range) ** 2
    mx, my = m(x), m(y)
    vx, vy, vxy = cov * (m(x * x) - mx * mx), cov * (m(y * y) - my * my), cov * (m(x * y) - mx * my)
    n1, n2, d1, d2 = 2 * mx * my + c1, 2 * vxy + c2, mx * mx + my * my + c1, vx + vy + c2
    S = n1 * n2 / (d1 * d2)
    dmy, dvy, dvxy = 2 * mx * n2 / (d1 * d2) - 2 * my * S / d1, -S / d2, 2 * n1 / (d1 * d2)
    A = dmy - 2 * cov * my * dvy - cov * mx * dvxy
    B, Cc = cov * dvy, cov * dvxy
    g = (T(A) + 2 * y * T(B) + x * T(Cc)) / S.numel()
    return g.squeeze(1).permute(1, 2, 0).contiguous().numpy()


def grads(gt, rec, win, cov, data_range):
    """dict(g64, g32, scale, err_ref): both autograd gradients and the fp32 one's error, max|g32 - g64| / scale with
    scale = max|g64| -- or 1, an absolute error, when g64 is fp64 rounding noise (below 1e-9: rec = gt, where the
    gradient vanishes; a gradient that is one has entries of 1 / (Ho Wo O) times numbers of order one and above)."""
    g64, mean64 = autograd_grad(gt, rec, win, cov, data_range, torch.float64)
    g32, _ = autograd_grad(gt, rec, win, cov, data_range, torch.float32)
    scale = np.abs(g64).max()
    scale = scale if scale > 1e-9 else 1.0
    return dict(g64=g64, g32=g32, scale=scale, err_ref=np.abs(g32 - g64).max() / scale, mean64=mean64)


@functools.lru_cache(maxsize=None)
def case(shape, sigma, kind):
    """ssim_ref.case plus the gradients; computed once and shared (callers must not modify them)."""
    c = dict(ref.case(shape, sigma, kind))
    c.update(grads(c["gt"], c["rec"], c["win"], c["cov"], c["data_range"]))
    return c


def ssim_mse_loss_and_grad(y, target, rows, lam, H, W, O, win, cov, data_range, dtype=torch.float64):
    """loss = mse(rows) + lam (1 - ssim(target, y)) of a full-grid [H*W, O] reconstruction by autograd in ``dtype``.
    Returns (loss, mse, ssim, g_y [H*W, O] float64 array)."""
    yt = torch.as_tensor(y).to(dtype).reshape(H * W, O).clone().requires_grad_(True)
    t = torch.as_tensor(target).to(dtype).reshape(H * W, O)
    rows = torch.as_tensor(np.asarray(rows, np.int64))
    mse = ((yt[rows] - t[rows]) ** 2).mean() if len(rows) else (yt.sum() * 0)
    ssim = _map(t.reshape(H, W, O), yt.reshape(H, W, O), win, cov, data_range, dtype).mean()
    loss = mse + lam * (1 - ssim)
    loss.backward()
    return float(loss.detach()), float(mse.detach()), float(ssim.detach()), yt.grad.numpy().astype(np.float64)
