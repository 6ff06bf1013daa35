"""Harness helpers on the hot path's contract (reference modules/utils.py).

Only the functions the training/eval loop of wire_image_denoise.py and
wire_occupancy.py touch are provided: coordinate grids, PSNR, parameter count,
normalisation, the noise model, the total-variation regulariser, ``resize`` (the per-channel INTER_AREA of
modules/utils.py:179-200, on the device) and logging.  Plotting / montage / table helpers
are out of scope -- except ``get_layer_outputs`` + ``build_montage``, the per-layer
visualisation query SURVEY section 8 (f)3 names.
"""
from datetime import datetime

import numpy as np
import torch


def log(msg):                                   # modules/utils.py:291-292
    print(f"{datetime.now()} - {msg}")


def normalize(x, fullnormalize=False):          # modules/utils.py:21-38
    if x.sum() == 0:
        return x
    xmax = x.max()
    xmin = x.min() if fullnormalize else 0
    return (x - xmin) / (xmax - xmin)


def psnr(x, xhat):
    """10 log10(max(x) / mse) -- max(x), not max(x)^2 (modules/utils.py:67-82)."""
    err = np.asarray(x) - np.asarray(xhat)
    return 10 * np.log10(np.max(x) / np.mean(err ** 2))


def rsnr(x, xhat):
    """Reconstruction SNR in dB, 20 log10(||x|| / ||x - xhat||) (modules/utils.py:49-64)."""
    x, xhat = np.asarray(x), np.asarray(xhat)
    return 20 * np.log10(np.linalg.norm(x.reshape(-1)) / np.linalg.norm((x - xhat).reshape(-1)))


def add_salt_and_pepper_noise(image, salt_prob, pepper_prob):
    """Impulse noise on a copy of an (H, W, C) image, same np.random call order as modules/utils.py:114-129: one
    np.random.random((H, W)) draw sets whole pixels to 255, a second one sets whole pixels to 0 (pepper wins where both
    fall).  An image on a 0..1 scale gets its salt as 255 too, as there; a driver on that scale sets the pixels itself
    from the two masks.  The data term for such noise is ``FusedTrainer.step_loss("l1")`` or ``"huber"``."""
    image = np.asarray(image)
    noisy = np.copy(image)
    noisy[np.random.random(image.shape[:2]) < salt_prob] = 255
    noisy[np.random.random(image.shape[:2]) < pepper_prob] = 0
    return noisy


def resize(cube, scale):
    """A multi-channel image stack (H, W, nchan) scaled by ``fx = fy = scale`` per channel with ``INTER_AREA``
    (modules/utils.py:179-200), on the device: ``functional.resize(cube, None, fx=scale, fy=scale, "area")``, so the
    output is ``rint(H * scale) x rint(W * scale)`` (round half to even).  A numpy array comes back as a numpy array of
    the same dtype (it is computed in float32 on the current CUDA device); a CUDA float32 tensor comes back as a tensor.
    ``scale > 1`` is a ValueError: cv2's INTER_AREA silently becomes a linear variant when it up-scales and this
    library does not imitate it.  The operator is built from cv2's documented formulas and has not been measured
    against cv2; a non-integer factor keeps the partial overlaps below 1e-3 that cv2 drops without renormalising."""
    from .. import functional
    if getattr(cube, "ndim", 0) != 3:
        raise ValueError("resize expects an (H, W, nchan) image stack")
    functional.resize_geometry(cube.shape[0], cube.shape[1], None, scale, scale, "area")   # its ValueErrors, before a device
    if isinstance(cube, torch.Tensor):
        return functional.resize(cube, None, fx=scale, fy=scale, interpolation="area")
    cube = np.asarray(cube)
    dev = torch.from_numpy(np.ascontiguousarray(cube, dtype=np.float32)).to("cuda")
    out = functional.resize(dev, None, fx=scale, fy=scale, interpolation="area")
    return out.cpu().numpy().astype(cube.dtype, copy=False)


def get_inpainting_mask(imsize, mask_type='random2d', mask_frac=0.5):
    """A float32 (H, W) mask of kept pixels for image inpainting (modules/utils.py:203-226), with the same np.random
    consumption: 'random2d' keeps a pixel when np.random.rand(H, W) < mask_frac, 'random1d' draws one row of W and
    repeats it, 'bayer' keeps the even rows and columns and draws nothing.  An unknown ``mask_type`` is a ValueError
    (the reference runs into an UnboundLocalError).  The mask, flattened (and repeated per channel, or one channel's
    sites per channel for a true mosaic), is the ``weight`` of ``FusedTrainer.step_loss``."""
    H, W = imsize
    if mask_type == 'random2d':
        mask = np.random.rand(H, W) < mask_frac
    elif mask_type == 'random1d':
        mask = np.ones((H, 1)).dot(np.random.rand(1, W) < mask_frac)
    elif mask_type == 'bayer':
        mask = np.zeros((H, W))
        mask[::2, ::2] = 1
    else:
        raise ValueError(f"mask_type {mask_type!r}: one of 'random2d', 'random1d', 'bayer'")
    return mask.astype(np.float32)


def measure(x, noise_snr=40, tau=100):
    """Photon + readout noise, same np.random call order as modules/utils.py:85-112."""
    meas = np.copy(x)
    noise = np.random.randn(meas.size).reshape(meas.shape) * noise_snr
    if tau != float('Inf'):
        meas = meas * tau
        pos = x > 0
        meas[pos] = np.random.poisson(meas[pos])
        meas[~pos] = -np.random.poisson(-meas[~pos])
        return (meas + noise) / tau
    return meas + noise


def total_variation_loss(image):
    """Anisotropic total variation of a (B, C, H, W) image (modules/utils.py:360-369): the sum -- not the mean -- of
    the absolute differences of vertical and of horizontal neighbours, a 0-dim device tensor, differentiable with respect
    to ``image`` (``functional.total_variation``: one HIP pass each way, instead of the slicing, ``abs`` and ``sum``
    launches of the torch expression).  The drivers' ``model(coords).reshape(1, H, W, 3).permute(0, 3, 1, 2)`` is read
    as the view it is, without a copy.  The reference's drivers evaluate this term under ``torch.no_grad()``
    (bspline_image_denoise.py:160-172), where it changes the reported loss and no gradient; a loop in which it acts on
    the weights is ``FusedTrainer.step_tv``."""
    from .. import functional
    return functional.total_variation(image)


def count_parameters(model):                    # modules/utils.py:159-160
    return sum(p.numel() for p in model.parameters() if p.requires_grad)


def get_coords(H, W, T=None):
    """2-D / 3-D grids in [-1, 1] (modules/utils.py:163-176): np.linspace in
    fp64, 'xy' meshgrid, flattened row-major, cast to fp32."""
    axes = [np.linspace(-1, 1, W), np.linspace(-1, 1, H)]
    if T is not None:
        axes.append(np.linspace(-1, 1, T))
    grids = np.meshgrid(*axes)
    coords = np.hstack([g.reshape(-1, 1) for g in grids])
    return torch.tensor(coords.astype(np.float32))


def axis_tables(H, W, T=None, style="numpy"):
    """Per-axis coordinate tables for the on-device generator
    (wire_coords_from_index).  style='numpy' reproduces get_coords above;
    style='torch' reproduces torch.linspace(-1, 1, n) of
    wire_image_denoise.py:63-64 bit for bit."""
    def ax(n):
        if style == "torch":
            return torch.linspace(-1, 1, n)
        return torch.tensor(np.linspace(-1, 1, n).astype(np.float32))
    return ax(W), ax(H), (ax(T) if T is not None else None)


def get_rays(H, W, focal, c2w):
    """Pinhole camera rays as [H*W, 6] = (origin, direction), float32, row i*W + j: in the camera's frame pixel (i, j)
    looks along ((j - W/2) / focal, -(i - H/2) / focal, -1) -- x right, y up, the camera looking down -z, the convention
    of the NeRF loaders -- and ``c2w`` ([3, 4] or [4, 4], array or tensor) rotates it into the world and gives the
    origin.  Directions are not normalised (``functional.ray_samples`` folds their length into ``deltas``).  The rays
    live on the device of ``c2w`` when that is a tensor.  Plain torch ops: this is not on a step's path."""
    c2w = torch.as_tensor(c2w).to(torch.float32)
    if c2w.dim() != 2 or c2w.shape[0] not in (3, 4) or c2w.shape[1] != 4:
        raise ValueError("c2w must be [3, 4] or [4, 4]")
    H, W = int(H), int(W)
    if H < 1 or W < 1 or not float(focal) > 0:
        raise ValueError("get_rays needs H, W >= 1 and focal > 0")
    i, j = torch.meshgrid(torch.arange(H, dtype=torch.float32, device=c2w.device),
                          torch.arange(W, dtype=torch.float32, device=c2w.device), indexing="ij")
    dirs = torch.stack([(j - 0.5 * W) / float(focal), -(i - 0.5 * H) / float(focal), -torch.ones_like(i)], dim=-1)
    d = (dirs[..., None, :] * c2w[:3, :3]).sum(dim=-1).reshape(H * W, 3)
    o = c2w[:3, 3].expand(H * W, 3)
    return torch.cat([o, d], dim=1).contiguous()


def ray_box(rays, lo=-1.0, hi=1.0):
    """(near, far) [R] of ``rays`` [R, 6] against the cube [lo, hi]^3 by the slab method, near clamped at 0 (the ray
    starts at its origin).  A ray that misses the cube gets far <= near, which ``functional.ray_samples`` turns into
    zero-length samples.  An axis the ray runs parallel to bounds nothing when the origin lies inside its slab, and
    rules the ray out otherwise."""
    if not isinstance(rays, torch.Tensor) or rays.dim() != 2 or rays.shape[1] != 6:
        raise ValueError("rays must be a tensor [R, 6]")
    o, d = rays[:, :3].to(torch.float32), rays[:, 3:].to(torch.float32)
    inf = torch.full_like(o, float("inf"))
    par = d == 0
    safe = torch.where(par, torch.ones_like(d), d)
    t0, t1 = (float(lo) - o) / safe, (float(hi) - o) / safe
    inside = (o >= float(lo)) & (o <= float(hi))
    tmin = torch.where(par, torch.where(inside, -inf, inf), torch.minimum(t0, t1))
    tmax = torch.where(par, torch.where(inside, inf, -inf), torch.maximum(t0, t1))
    near = tmin.max(dim=1).values.clamp_min(0.0)
    far = tmax.min(dim=1).values
    miss = ~(far > near)                                   # finite bounds for a miss: its samples sit at the origin
    zero = torch.zeros_like(near)
    return torch.where(miss, zero, near).contiguous(), torch.where(miss, zero, far).contiguous()


def build_montage(images):
    """Tile ``images`` [n, H, W] (each min-max normalised, ``normalize(.., True)``) row by row into a
    ceil(sqrt(n))-row grid; unused cells stay 0 (modules/utils.py:131-156)."""
    images = np.asarray(images)
    n, H, W = images.shape
    nrows = int(np.ceil(np.sqrt(n)))
    ncols = int(np.ceil(n / nrows))
    out = np.zeros((H * nrows, W * ncols), dtype=np.float32)
    for k in range(n):
        r, c = divmod(k, ncols)
        out[r * H:(r + 1) * H, c * W:(c + 1) * W] = normalize(images[k], True)
    return out


@torch.no_grad()
def get_layer_outputs(model, coords, imsize, nfilters_vis=16, get_imag=False):
    """Activation images after each layer, for visualisation (modules/utils.py:229-288).  Every layer runs through its
    own HIP entry point -- ``model.net[idx](x)`` -> wire_gabor_fwd / wire_real_layer_fwd / wire_gabor2d_fwd, the kernels
    of the fused path -- on the previous layer's (complex) output; the rest is the reference's host-side bookkeeping:
    the first ``nfilters_vis`` filters ('all': every filter), real or imaginary part, sign chosen so that the larger
    excursion is positive, filters ordered by standard deviation, each min-max normalised with a white frame, tiled by
    ``build_montage``.  Returns one montage per activation layer."""
    H, W = imsize
    if getattr(model, "pos_encode", False):
        coords = model.positional_encoding(coords)
    montages = []
    x = coords
    for idx in range(len(model.net) - 1):
        x = model.net[idx](x)
        imgs = x.reshape(1, H, W, -1)[0]
        if nfilters_vis != 'all':
            imgs = imgs[..., :nfilters_vis]
        atoms = imgs.detach().cpu().numpy()
        atoms = atoms.imag if get_imag else atoms.real
        lo = atoms.min(0, keepdims=True).min(1, keepdims=True)
        hi = atoms.max(0, keepdims=True).max(1, keepdims=True)
        atoms = (1 - 2 * (abs(lo) > abs(hi))) * atoms
        atoms = atoms[..., np.argsort(atoms.std((0, 1)))]
        lo = atoms.min(0, keepdims=True).min(1, keepdims=True)
        hi = atoms.max(0, keepdims=True).max(1, keepdims=True)
        atoms = (atoms - lo) / np.maximum(1e-14, hi - lo)
        atoms[:, [0, -1], :] = 1
        atoms[[0, -1], :, :] = 1
        montages.append(build_montage(np.transpose(atoms, [2, 0, 1])))
    return montages
