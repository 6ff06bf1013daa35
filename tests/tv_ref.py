"""The total-variation regulariser (utils.total_variation_loss, modules/utils.py:360-369) restated on numpy or torch, its
gradient in closed form, and the loss of the regularised loop.  The yardstick of tests/test_tv_host.py (which pins it to
the value and the autograd gradient the reference itself produces, tests/golden/tv.npz) and of tests/test_gpu_tv.py
(precedent: tests/video_cs_ref.py).

    tv(x) = sum |x[..., 1:, :] - x[..., :-1, :]| + sum |x[..., :, 1:] - x[..., :, :-1]|         (a sum, not a mean)
    dtv/dx[i][j] = s(x[i][j] - x[i-1][j]) - s(x[i+1][j] - x[i][j]) + s(x[i][j] - x[i][j-1]) - s(x[i][j+1] - x[i][j])

with s = sign, s(0) = 0 (torch's derivative of abs), a term whose neighbour lies outside the image being 0.  s is taken
by comparison, so the pattern is a small integer whatever the precision.
"""
import numpy as np


def total_variation(image, double=True):
    """The reference's four lines on a (..., H, W) numpy array or torch tensor, in fp64 (``double``) or fp32; the result
    is a 0-dim array / tensor of that precision."""
    if isinstance(image, np.ndarray):
        x = image.astype(np.float64 if double else np.float32)
        diff_x = x[..., 1:, :] - x[..., :-1, :]
        diff_y = x[..., :, 1:] - x[..., :, :-1]
        return np.sum(np.abs(diff_x), dtype=x.dtype) + np.sum(np.abs(diff_y), dtype=x.dtype)
    import torch
    x = image.to(torch.float64 if double else torch.float32)
    diff_x = x[..., 1:, :] - x[..., :-1, :]
    diff_y = x[..., :, 1:] - x[..., :, :-1]
    return torch.sum(torch.abs(diff_x)) + torch.sum(torch.abs(diff_y))


def tv_sign_pattern(image):
    """dtv/dx of a (..., H, W) numpy array as int8 in -4 .. 4, from comparisons of the values as they are."""
    x = np.asarray(image)
    k = np.zeros(x.shape, np.int8)
    sv = (x[..., 1:, :] > x[..., :-1, :]).astype(np.int8) - (x[..., 1:, :] < x[..., :-1, :]).astype(np.int8)
    sh = (x[..., :, 1:] > x[..., :, :-1]).astype(np.int8) - (x[..., :, 1:] < x[..., :, :-1]).astype(np.int8)
    k[..., 1:, :] += sv
    k[..., :-1, :] -= sv
    k[..., :, 1:] += sh
    k[..., :, :-1] -= sh
    return k


def total_variation_grad(image, g=1.0, double=True):
    """g * dtv/dx: the integer pattern times the upstream gradient, one rounding per entry."""
    dt = np.float64 if double else np.float32
    return dt(g) * tv_sign_pattern(image).astype(dt)


def channel_first(y, H, W, O):
    """[H*W, O] rows (row i*W + j) -> (O, H, W), the drivers' reshape(1, H, W, O).permute(0, 3, 1, 2) without the 1."""
    return np.asarray(y).reshape(H, W, O).transpose(2, 0, 1)


def tv_mse_loss_and_grad(y, target, rows, lambda_tv, H, W, O, double=True, pattern_from=None):
    """The regularised loss on a full-grid reconstruction y [H*W, O] against target [H*W, O]:

        mse  = sum_{r in rows, o} (y - target)[r][o]^2 / (len(rows) O)          (0 for no rows)
        loss = mse + lambda_tv tv(y)
        g_y  = [row selected] 2 (y - target) / (len(rows) O) + lambda_tv dtv/dy

    rows: distinct flat grid indices.  ``pattern_from`` (optional, [H*W, O]): the image whose comparisons give the sign
    pattern of the TV gradient instead of y -- s is discontinuous, so an oracle in another precision takes the pattern of
    the image the kernel saw.  Returns (loss, mse, tv, g_y [H*W, O]) in fp64 or fp32."""
    dt = np.float64 if double else np.float32
    y = np.asarray(y, dt).reshape(H * W, O)
    t = np.asarray(target, dt).reshape(H * W, O)
    rows = np.asarray(rows, np.int64).reshape(-1)
    tv = total_variation(channel_first(y, H, W, O), double)
    k = tv_sign_pattern(channel_first(y if pattern_from is None else np.asarray(pattern_from), H, W, O))
    g = dt(lambda_tv) * k.transpose(1, 2, 0).reshape(H * W, O).astype(dt)
    mse = dt(0)
    if rows.size:
        d = y[rows] - t[rows]
        mse = np.sum(np.square(d), dtype=dt) / dt(d.size)
        g[rows] += (dt(2.0) / dt(d.size)) * d
    return dt(mse + dt(lambda_tv) * tv), mse, tv, g
