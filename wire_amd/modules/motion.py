"""Data path of the multi-image super-resolution driver (reference modules/motion.py, wire_multi_sr.py:74-110).

Only what that driver's data path needs and what depends on nothing beyond numpy and torch: the frame dataset
(``ImageSRDataset``), the flat grid (``xy_mgrid``), rigid 2 x 3 matrices and their inverses (``getEuclidianMatrix``,
``invert_regstack``, ``affine2rigid``) and ``get_transformed_coords``.  The frames' coordinate stack itself --
``get_imstack``'s ``Xstack`` / ``Ystack`` at scale 1 -- is a HIP kernel (wire_affine_coords, reached through
``FusedTrainer.affine_coords``), and the loop's loss is ``FusedTrainer.step_frames``.

Registration and resampling run on the device, without cv2 / kornia / pystackreg: ``get_imstack``
builds the simulated stack with ``functional.remap`` (wire_remap_bilinear_fwd), ``register_stack_ecc`` recovers the
frames' matrices from their intensities by a coarse-to-fine, multi-start Gauss-Newton registration
(wire_register_gn_step) -- a plain least-squares criterion, NOT cv2's enhanced correlation coefficient -- and
``prune_stack``, ``interp_lr``, ``mat2coords`` and ``param2theta`` sit on the same pieces.  The chain into training is
``register_stack_ecc`` -> ``ecc_mats`` -> ``FusedTrainer.affine_coords`` -> ``step_frames`` / ``step_frames_registered``.
Still out of scope: homographies, ``ecc_flow`` itself, pystackreg's ``register_stack``, Farneback flow (``fb_flow``,
``flow2rgb``).

A LEARNABLE registration -- what the reference's ``param2theta`` / ``get_transformed_coords`` / ``interp_lr`` were the
pieces of -- is not in this module: a per-frame ``theta`` [B, 2, 3] of ``get_transformed_coords``' convention (a matrix on
the normalised coordinates, identity ``[[1, 0, 0], [0, 1, 0]]``) applied to any base coordinates is
``functional.warp_coords(coords, theta)``, differentiable for a torch optimiser, and training it jointly with the net in
one sync-free step is ``FusedTrainer.step_frames_registered`` (both HIP: wire_warp_coords_fwd / wire_warp_coords_bwd).
"""
from __future__ import annotations

import numpy as np
import torch
import torch.nn.functional as F
from torch.utils.data import Dataset


class ImageSRDataset(Dataset):
    """One item per low-resolution frame (modules/motion.py:22-76): ``(coords, pixels, mask[, idx])``.

    imstack: (nimg, 3, Hl, Wl) frames -> pixels [Hl*Wl, 3], channel last, row i*Wl + j;
    Xstack / Ystack: (nimg, H, W) normalised coordinates -> coords [H*W, 2] = (x, y); masks: shaped like imstack ->
    mask shaped like pixels.  A stack that was not given comes back as ``torch.zeros(1)``.  ``jitter`` / ``xjitter`` /
    ``yjitter`` are stored and, as in the reference, not used by ``__getitem__``."""

    def __init__(self, imstack, Xstack=None, Ystack=None, masks=None, jitter=False, xjitter=None, yjitter=None,
                 get_indices=False):
        super().__init__()
        self.imstack, self.Xstack, self.Ystack, self.masks = imstack, Xstack, Ystack, masks
        self.jitter, self.get_indices = jitter, get_indices
        self.nimg, _, self.H, self.W = imstack.shape
        self.xjitter = 1 / self.W if xjitter is None else xjitter
        self.yjitter = 1 / self.H if xjitter is None else yjitter

    def __len__(self):
        return self.nimg

    @staticmethod
    def _channel_last(a):
        return torch.tensor(a).permute(1, 2, 0).reshape(-1, 3)

    def __getitem__(self, idx):
        pixels = self._channel_last(self.imstack[idx])
        mask = self._channel_last(self.masks[idx]) if self.masks is not None else torch.zeros(1)
        if self.Xstack is not None:
            coords = torch.stack((torch.tensor(self.Xstack[idx]), torch.tensor(self.Ystack[idx])), dim=-1).reshape(-1, 2)
        else:
            coords = torch.zeros(1)
        return (coords, pixels, mask, idx) if self.get_indices else (coords, pixels, mask)


def xy_mgrid(H, W):
    """[H*W, 2] grid of (x, y) in [-1, 1], row i*W + j -> (x_j, y_i) (modules/motion.py:79-92)."""
    y, x = torch.linspace(-1, 1, H), torch.linspace(-1, 1, W)
    return torch.stack((x[None, :].expand(H, W), y[:, None].expand(H, W)), dim=-1).reshape(-1, 2)


def getEuclidianMatrix(theta, shift):
    """2 x 3 matrix of a rotation by ``theta`` followed by the translation ``shift`` (modules/motion.py:95-102)."""
    c, s = np.cos(theta), np.sin(theta)
    return np.array([[c, -s, shift[0]], [s, c, shift[1]]])


def invert_regstack(regstack):
    """Inverse of every 2 x 3 affine matrix of a (nimg, 2, 3) stack (modules/motion.py:432-446; ``numpy.linalg.inv``
    where the reference calls scipy's)."""
    out = np.zeros_like(regstack)
    for i in range(regstack.shape[0]):
        full = np.eye(3)
        full[:2] = regstack[i]
        out[i] = np.linalg.inv(full)[:2]
    return out


def affine2rigid(mats):
    """(angles, translations) of (nmats, 2, 3) rigid matrices: arccos of the first entry and the last column
    (modules/motion.py:523-541)."""
    return np.arccos(mats[:, 0, 0]), mats[:, :, 2]


def get_transformed_coords(theta, imsize):
    """``F.affine_grid`` of (B, 2, 3) matrices on an (H, W) image as [B, H*W, 2] (modules/motion.py:544-551)."""
    H, W = imsize
    return F.affine_grid(theta, (theta.shape[0], 1, H, W), align_corners=False).reshape(-1, H * W, 2)


# ---------------------------------------------------------------------------
# registration and resampling on the device (functional.remap, functional.register_gn_step)
# ---------------------------------------------------------------------------
def _pixel_grid(H, W):
    """(j, i, 1) of every pixel of an (H, W) image, [H*W, 3] float64, row i*W + j."""
    Y, X = np.mgrid[:H, :W]
    return np.stack((X.reshape(-1), Y.reshape(-1), np.ones(H * W)), axis=1).astype(np.float64)


def _device_image(im, device):
    """A numpy array or tensor as a contiguous float32 tensor on the device."""
    return torch.as_tensor(np.ascontiguousarray(im) if isinstance(im, np.ndarray) else im).detach() \
        .to(device, torch.float32).contiguous()


def get_imstack(im, scale, shift_max=10, theta_max=np.pi / 12, nshifts=5, device="cuda"):
    """Synthetic stack of ``nshifts`` rigidly moved copies of ``im`` (H, W, C) (modules/motion.py:264-320):
    ``(imstack, Xstack, Ystack, mats)`` = (nshifts, H, W, C) float32 frames, (nshifts, H, W) float32 normalised
    coordinates ``2 X / W - 1``, ``2 Y / H - 1`` and the (nshifts, 2, 3) matrices, ``frame_f(i, j) = im(mats[f] (j, i, 1))``.

    ``np.random`` is consumed exactly as the reference consumes it -- ``randint(-shift_max, shift_max, [nshifts, 2])``
    then ``rand(nshifts)`` -- and frame 0 is pinned to the identity.  The frames are ``functional.remap`` of the device
    image (wire_remap_bilinear_fwd) at the float32 coordinates, zero outside the image: its bilinear weights are exact,
    where ``cv2.remap`` quantises them to 1/32 pixel, so the frames differ from cv2's in the last bits of a blend.  Only
    ``scale == 1``, the one way the driver calls it (wire_multi_sr.py:74-78); any other scale raises
    NotImplementedError (the reference resizes the coordinate maps with cv2 there)."""
    from .. import functional
    if scale != 1:
        raise NotImplementedError("get_imstack: only scale == 1 (the driver's call); resize the frames afterwards")
    H, W, _ = im.shape
    shifts = np.random.randint(-shift_max, shift_max, size=[nshifts, 2])
    thetas = (2 * np.random.rand(nshifts) - 1) * theta_max
    shifts[0, :] = 0
    thetas[0] = 0
    coords = _pixel_grid(H, W)
    img = _device_image(im, device)
    imstack = np.zeros((nshifts, H, W, im.shape[2]), dtype=np.float32)
    Xstack = np.zeros((nshifts, H, W), dtype=np.float32)
    Ystack = np.zeros_like(Xstack)
    mats = np.zeros((nshifts, 2, 3))
    for idx in range(nshifts):
        mat = getEuclidianMatrix(thetas[idx], shifts[idx, :])
        mats[idx, ...] = mat
        new = mat.dot(coords.T).T                                          # [H*W, 2] = (Xnew, Ynew)
        xy = torch.from_numpy(new.astype(np.float32)).to(img.device)
        imstack[idx, ...] = functional.remap(img, xy).reshape(H, W, -1).cpu().numpy()
        Xstack[idx, ...] = (2 * new[:, 0] / W - 1).reshape(H, W)
        Ystack[idx, ...] = (2 * new[:, 1] / H - 1).reshape(H, W)
    return imstack, Xstack, Ystack, mats


def rescale_mats(mats, s):
    """2 x 3 pixel-space matrices of an image as the matrices of the same image sampled ``s`` times finer (pixel centre
    ``X = s x + (s - 1) / 2``): the linear part stays, ``t <- s t + (s - 1) / 2 - A ((s - 1) / 2, (s - 1) / 2)``.
    ``s = 2`` is one pyramid level finer; ``s = 1 / k`` goes coarser.  numpy float64 or torch tensors [..., 2, 3]."""
    out = mats.clone() if isinstance(mats, torch.Tensor) else np.array(mats, dtype=np.float64)
    h = (s - 1) / 2
    out[..., 2] = s * mats[..., 2] + h - (mats[..., 0] + mats[..., 1]) * h
    return out


def _pool2(x):
    """[B, H, W] -> [B, H//2, W//2] by 2 x 2 means (an odd last row / column is dropped)."""
    return F.avg_pool2d(x[:, None], 2)[:, 0].contiguous()


def _method_name(method):
    from .. import functional, _lib
    m = functional._motion_model(method)
    return next(k for k, v in _lib.MOTION_MODEL.items() if v == m)


def register_stack_ecc(imstack, full_res, method="euclidean", levels=3, iters=30, seeds=None, weight=None,
                       damping=1e-6, min_cover=0.25, device="cuda"):
    """Register every frame of ``imstack`` onto frame 0 from the intensities (the role of modules/motion.py:575-642):
    ``(Xstack, Ystack, mask, ecc_mats, alignment_err)``.

    ``imstack``: (nimg, H, W) or (nimg, C, H, W), channels averaged.  ``ecc_mats`` (nimg, 2, 3), float64, are pixel-space
    matrices AT ``full_res`` = (Hr, Wr) with ``frame_f(x) = frame_0(ecc_mats[f] x)`` -- what ``get_imstack`` calls
    ``mats`` and ``FusedTrainer.affine_coords`` takes.  ``Xstack`` / ``Ystack`` (nimg, H, W) float32 are the normalised
    coordinates ``2 X / Wr - 1``, ``2 Y / Hr - 1`` of every low-resolution pixel's centre.  ``mask[f] = 0`` where no
    start candidate gave a valid system (the frame then keeps the identity); ``alignment_err[f]`` is the mean |residual|
    over the covered pixels at the frames' own resolution, at the matrix the frame ends with -- reported for a masked
    frame too, where the reference leaves 0.  Frame 0 is the identity with error 0.

    The method: a pyramid of ``levels`` levels by 2 x 2 means; at the coarsest, ``iters`` Gauss-Newton iterations
    (wire_register_gn_step) on ``K = len(seeds)`` start candidates per frame -- rotations by the ``seeds`` angles about
    the image centre, default ``(0,)`` -- then, per frame, the valid candidate of least residual (one ``argmin`` on the
    device); ``iters`` iterations at every finer level after ``t <- 2 t + 1/2 - A (1/2, 1/2)``, and the same map with the
    factor ``Hr / H`` to ``full_res``.  Registration runs at the frames' OWN resolution, not on copies upsampled to
    ``full_res`` as the reference does: the upsampling adds no information and 16 x the pixels.  It minimises a plain
    weighted least-squares criterion -- not cv2.findTransformECC's enhanced correlation coefficient -- with no Gaussian
    pre-filter and a fixed iteration count.  ``method``: "translation" | "euclidean" | "affine", or cv2's integers
    0 / 1 / 2; homography (3) raises NotImplementedError.  ``weight``: (nimg, H, W) per-pixel weights or None; a pixel
    whose frame value is exactly 0 never counts (the resampler's border fill)."""
    from .. import functional
    model = _method_name(method)
    x = _device_image(imstack, device)
    if x.dim() == 4:
        x = x.mean(dim=1)
    if x.dim() != 3 or x.shape[0] < 1:
        raise ValueError("imstack must be (nimg, H, W) or (nimg, C, H, W)")
    nimg, H, W = (int(v) for v in x.shape)
    Hr, Wr = (int(v) for v in full_res)
    if Hr * W != Wr * H or Hr < H:
        raise ValueError(f"full_res {(Hr, Wr)} must be one factor >= 1 times the frames' {(H, W)}")
    levels, iters = int(levels), int(iters)
    if levels < 1 or iters < 1 or min(H, W) >> (levels - 1) < 4:
        raise ValueError("levels and iters must be >= 1, and the coarsest level at least 4 pixels a side")
    seeds = (0.0,) if seeds is None else tuple(float(a) for a in np.asarray(seeds, dtype=np.float64).reshape(-1))
    if len(seeds) < 1:
        raise ValueError("seeds must hold at least one angle")
    wt = None
    if weight is not None:
        wt = _device_image(weight, device)
        if tuple(wt.shape) != (nimg, H, W):
            raise ValueError(f"weight must be {(nimg, H, W)}")
    ecc_mats = np.zeros((nimg, 2, 3))
    ecc_mats[:, 0, 0] = ecc_mats[:, 1, 1] = 1
    mask, alignment_err = np.zeros(nimg), np.zeros(nimg)
    mask[0] = 1
    if nimg > 1:
        B = nimg - 1
        pyr = [(x[0].contiguous(), x[1:].contiguous(), None if wt is None else wt[1:].contiguous())]
        for _ in range(levels - 1):
            r, f, w = pyr[-1]
            pyr.append((_pool2(r[None])[0].contiguous(), _pool2(f), None if w is None else _pool2(w)))
        # start candidates at the coarsest level: rotations about the image centre
        r, f, w = pyr[-1]
        cy, cx = (r.shape[0] - 1) / 2, (r.shape[1] - 1) / 2
        start = np.stack([np.array([[np.cos(a), -np.sin(a), cx - np.cos(a) * cx + np.sin(a) * cy],
                                    [np.sin(a), np.cos(a), cy - np.sin(a) * cx - np.cos(a) * cy]]) for a in seeds])
        mats = torch.from_numpy(np.broadcast_to(start, (B, len(seeds), 2, 3)).copy()).to(x.device)
        for _ in range(iters):
            functional.register_gn_step(r, f, mats, w, model, damping, min_cover)
        st = functional.register_gn_step(r, f, mats.clone(), w, model, damping, min_cover)
        cost = torch.where(st[..., 3] > 0, st[..., 0], torch.full_like(st[..., 0], float("inf")))
        best = cost.argmin(dim=1)
        found = torch.isfinite(cost.gather(1, best[:, None])[:, 0])
        mats = mats.gather(1, best[:, None, None, None].expand(B, 1, 2, 3)).contiguous()
        for r, f, w in pyr[-2::-1]:
            mats = rescale_mats(mats, 2.0).contiguous()
            for _ in range(iters):
                functional.register_gn_step(r, f, mats, w, model, damping, min_cover)
        r, f, w = pyr[0]
        st = functional.register_gn_step(r, f, mats.clone(), w, model, damping, min_cover)
        found = found & (st[:, 0, 3] > 0)
        # a frame without a valid candidate keeps the identity; the mean |residual| over the pixels the registration
        # counts is reported for every frame, at the matrix it ends with
        ident = torch.tensor([[1.0, 0.0, 0.0], [0.0, 1.0, 0.0]], dtype=torch.float64, device=x.device)
        low = torch.where(found[:, None, None], mats[:, 0], ident)
        jj = torch.arange(W, dtype=torch.float64, device=x.device)[None, None, :, None]
        ii = torch.arange(H, dtype=torch.float64, device=x.device)[None, :, None, None]
        uv = (low[:, None, None, :, 0] * jj + low[:, None, None, :, 1] * ii + low[:, None, None, :, 2]).reshape(B, H * W, 2)
        inside = ((uv[..., 0] >= 0) & (uv[..., 0] <= W - 1) & (uv[..., 1] >= 0) & (uv[..., 1] <= H - 1)).reshape(B, H, W)
        count = inside & (f != 0) if w is None else inside & (f != 0) & (w != 0)
        warped = functional.remap(r[:, :, None].contiguous(), uv.to(torch.float32).contiguous()).reshape(B, H, W)
        err = ((warped - f).abs() * count).sum(dim=(1, 2)) / count.sum(dim=(1, 2)).clamp(min=1)
        mask[1:] = found.cpu().numpy()
        alignment_err[1:] = err.double().cpu().numpy()
        ecc_mats[1:] = rescale_mats(low.cpu().numpy(), Hr / H)
    Xstack, Ystack = _centre_coords(ecc_mats, (Hr, Wr), (H, W))
    return Xstack, Ystack, mask, ecc_mats, alignment_err


def _centre_coords(mats, full_res, low_res):
    """Normalised full-resolution coordinates of the low-resolution pixels' centres under ``mats`` (at full_res)."""
    (H, W), (Hl, Wl) = full_res, low_res
    if H % Hl or W % Wl or H // Hl != W // Wl:
        raise ValueError(f"{full_res} must be one integer factor times {low_res}")
    s = H // Hl
    m = np.asarray(mats, dtype=np.float64)[:, :, None, None, :]                # [nimg, 2, 1, 1, 3]
    xc = (s * np.arange(Wl) + (s - 1) / 2)[None, None, None, :]
    yc = (s * np.arange(Hl) + (s - 1) / 2)[None, None, :, None]
    new = m[..., 0] * xc + m[..., 1] * yc + m[..., 2]                            # [nimg, 2, Hl, Wl]
    Xstack = (2 * new[:, 0] / W - 1).astype(np.float32)
    Ystack = (2 * new[:, 1] / H - 1).astype(np.float32)
    return Xstack, Ystack


def mat2coords(reg_stack, full_res, low_res):
    """Normalised coordinates ``(Xstack, Ystack)``, (nimg, Hl, Wl) float32, from (nimg, 2, 3) registration matrices
    (modules/motion.py:449-483): the INVERSE of every matrix applied to the full-resolution pixel grid, ``2 X / W - 1``,
    ``2 Y / H - 1``, brought to ``low_res`` by ``cv2.resize(..., INTER_AREA)``.  For an integer factor INTER_AREA is the
    block mean, and the block mean of an affine map is the map at the block's centre ``s j + (s - 1) / 2`` -- which is
    what this evaluates, in float64.  Other factors raise ValueError."""
    return _centre_coords(invert_regstack(np.asarray(reg_stack, dtype=np.float64)), full_res, low_res)


def param2theta(params, w, h):
    """Pixel-space (nimg, 2, 3) matrices as the ``theta`` of ``F.affine_grid`` (modules/motion.py:486-520, verbatim
    arithmetic: the inverse matrix with its off-diagonal entries scaled by the aspect and its translation normalised)."""
    last_row = np.zeros((1, 3), dtype=np.float32)
    last_row[0, 2] = 1
    theta = np.zeros_like(params)
    for idx in range(params.shape[0]):
        param = np.linalg.inv(np.vstack((params[idx, ...], last_row)))
        theta[idx, 0, 0] = param[0, 0]
        theta[idx, 0, 1] = param[0, 1] * h / w
        theta[idx, 0, 2] = param[0, 2] * 2 / w + theta[idx, 0, 0] + theta[idx, 0, 1] - 1
        theta[idx, 1, 0] = param[1, 0] * w / h
        theta[idx, 1, 1] = param[1, 1]
        theta[idx, 1, 2] = param[1, 2] * 2 / h + theta[idx, 1, 0] + theta[idx, 1, 1] - 1
    return theta


def interp_lr(imref, coords, renderer):
    """Frames seen through ``coords`` and integrated down (modules/motion.py:554-572): ``imref`` (1, C, H, W), ``coords``
    (B, Hc, Wc, 2) normalised -> ``renderer.integrator`` of the (B, C, Hc, Wc) samples.  The reference's
    ``F.grid_sample(mode='bilinear', align_corners=False)`` is ``functional.remap(..., normalized=True)``, so a gradient
    reaches ``coords`` (and not ``imref``)."""
    from .. import functional
    img = imref[0].permute(1, 2, 0).contiguous()
    im_hr = functional.remap(img, coords.contiguous(), normalized=True).permute(0, 3, 1, 2)
    return renderer.integrator(im_hr)


def prune_stack(imstack, ecc_mats, full_res, thres=None, device="cuda"):
    """Drop the frames that are not well registered (modules/motion.py:645-682): ``(imstack, ecc_mats, mask, imdiff)``
    of the kept frames, ``mask`` over all of them.  ``imstack``: (nimg, Hl, Wl); ``ecc_mats``: (nimg, 2, 3) at
    ``full_res``.  Frame 0 is warped onto every frame's grid -- ``functional.remap`` of frame 0 at the matrices brought to
    the frames' resolution, where the reference upsamples frame 0 and calls ``kornia.warp_affine`` -- and a frame is kept
    when the mean of ``|warped - frame| / (frame + 0.01 max)`` is below ``thres`` (default 1)."""
    from .. import functional
    imstack = np.asarray(imstack)
    nimg, Hl, Wl = imstack.shape
    H, W = full_res
    if H * Wl != W * Hl:
        raise ValueError(f"full_res {full_res} must be one factor times the frames' {(Hl, Wl)}")
    if thres is None:
        thres = 1
    low = rescale_mats(np.asarray(ecc_mats, dtype=np.float64), Hl / H)
    ref = _device_image(imstack[0], device)
    uv = np.einsum("fac,pc->fpa", low, _pixel_grid(Hl, Wl)).astype(np.float32)
    imtrans = functional.remap(ref[:, :, None].contiguous(), torch.from_numpy(uv).to(ref.device))
    imdiff = np.abs(imtrans.reshape(nimg, Hl, Wl).cpu().numpy() - imstack)
    diff_array = (imdiff / (imstack + 1e-2 * imstack.max())).mean(-1).mean(-1)
    mask = diff_array < thres
    return (np.copy(imstack[mask == 1, ...], order="C"), np.copy(np.asarray(ecc_mats)[mask == 1, ...], order="C"), mask,
            imdiff[mask == 1, ...])
