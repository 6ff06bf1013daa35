"""Restatement of the two SSIM definitions the reference's drivers use, from the libraries' published behaviour, in
torch on the CPU (fp64 or fp32), and the inputs the SSIM tests share.

"gaussian": pytorch_msssim.ssim(gt, rec, data_range=1, size_average=True) -- 11 taps exp(-(i-5)^2 / (2 1.5^2))
normalised in fp32, valid separable convolution, population covariance.
"uniform": skimage.metrics.structural_similarity(gt, rec, multichannel=True) -- a 7 x 7 uniform filter cropped by 3 at
each side (= the valid region), sample covariance NP / (NP - 1), NP = 49.
Both: C1 = (0.01 L)^2, C2 = (0.03 L)^2, S = (2 mx my + C1)(2 vxy + C2) / ((mx^2 + my^2 + C1)(vx + vy + C2)), mean over
all pixels and channels."""
import functools

import numpy as np
import torch
import torch.nn.functional as F

SIGMAS = (0.01, 0.1, 0.5)
# data range per window: 1 is what the drivers pass to pytorch_msssim; 2 is what the skimage release they were written
# against derives for float images
DATA_RANGE = {"gaussian": 1.0, "uniform": 2.0}


def window(kind):
    """(fp32 weights, covariance factor)"""
    if kind == "gaussian":
        c = torch.arange(11, dtype=torch.float32) - 5
        g = torch.exp(-(c ** 2) / (2 * 1.5 ** 2))
        return g / g.sum(), 1.0
    if kind == "uniform":
        return torch.full((7,), 1.0 / 7.0, dtype=torch.float32), 49.0 / 48.0
    raise ValueError(kind)


def ssim_map(x, y, win, cov, data_range, dtype):
    """x, y: [H, W, O] arrays or tensors; win: 1-D weights (cast to ``dtype``: the fp32 window's own rounding is then
    part of neither precision's error).  Returns (mean as a Python float, map [H', W', O] tensor of ``dtype``)."""
    x = torch.as_tensor(x).to(dtype).permute(2, 0, 1).unsqueeze(1)        # [O, 1, H, W]: the channels as the batch
    y = torch.as_tensor(y).to(dtype).permute(2, 0, 1).unsqueeze(1)
    w = torch.as_tensor(win).to(dtype)
    wv, wh = w.reshape(1, 1, -1, 1), w.reshape(1, 1, 1, -1)

    def m(t):
        return F.conv2d(F.conv2d(t, wv), wh)

    c1, c2 = (0.01 * data_range) ** 2, (0.03 * data_range) ** 2
    mx, my = m(x), m(y)
    vx = cov * (m(x * x) - mx * mx)
    vy = cov * (m(y * y) - my * my)
    vxy = cov * (m(x * y) - mx * my)
    s = ((2 * mx * my + c1) * (2 * vxy + c2)) / ((mx * mx + my * my + c1) * (vx + vy + c2))
    s = s.squeeze(1).permute(1, 2, 0).contiguous()
    return float(s.mean()), s


def inputs(shape, sigma):
    """gt[i, j, c] = 0.5 + 0.4 sin(0.3 j + 0.2 i + c), rec = gt + sigma N(0, 1); fp32, seeded from the shape."""
    H, W, O = shape
    i, j, c = np.meshgrid(np.arange(H), np.arange(W), np.arange(O), indexing="ij")
    gt = (0.5 + 0.4 * np.sin(0.3 * j + 0.2 * i + c)).astype(np.float32)
    rng = np.random.default_rng((H * 1009 + W) * 16 + O)
    rec = (gt + np.float32(sigma) * rng.standard_normal(shape).astype(np.float32)).astype(np.float32)
    return gt, rec


@functools.lru_cache(maxsize=None)
def case(shape, sigma, kind):
    """The inputs and both restatements of one case, computed once and shared (callers must not modify them)."""
    gt, rec = inputs(shape, sigma)
    win, cov = window(kind)
    L = DATA_RANGE[kind]
    mean64, map64 = ssim_map(gt, rec, win, cov, L, torch.float64)
    mean32, map32 = ssim_map(gt, rec, win, cov, L, torch.float32)
    return dict(gt=gt, rec=rec, win=win, cov=cov, data_range=L, mean64=mean64, map64=map64.numpy(), mean32=mean32,
                map32=map32.numpy().astype(np.float64))
