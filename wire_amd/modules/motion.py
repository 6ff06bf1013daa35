"""Data path of the multi-image super-resolution driver (reference modules/motion.py, wire_multi_sr.py:74-110).

Only what that driver's data path needs and what depends on nothing beyond numpy and torch: the frame dataset
(``ImageSRDataset``), the flat grid (``xy_mgrid``), rigid 2 x 3 matrices and their inverses (``getEuclidianMatrix``,
``invert_regstack``, ``affine2rigid``) and ``get_transformed_coords``.  The frames' coordinate stack itself --
``get_imstack``'s ``Xstack`` / ``Ystack`` at scale 1 -- is a HIP kernel (wire_affine_coords, reached through
``FusedTrainer.affine_coords``), and the loop's loss is ``FusedTrainer.step_frames``.  Registration and resampling
(``register_stack``, ``register_stack_ecc``, ``ecc_flow``, ``fb_flow``, ``get_imstack``'s ``cv2.remap``, ``prune_stack``,
``interp_lr``: cv2, kornia, pystackreg) are out of scope, as are ``mat2coords``, ``param2theta`` and ``flow2rgb``.

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
