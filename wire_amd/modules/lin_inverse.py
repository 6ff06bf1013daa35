"""Linear inverse-problem operators on the hot path's contract (reference modules/lin_inverse.py).

``radon``: the CT forward operator the WIRE driver uses (wire_ct.py:128-133).  The reference rotates the image once
per angle with ``kornia.geometry.rotate`` and sums over the rows; here the rotate-and-sum and its adjoint are one HIP
kernel each (wire_radon_fwd / wire_radon_bwd), wrapped in an autograd.Function so that ``loss.backward()`` reaches
the model.  ``radon_volume`` is the volume form (the reference's ``is_3d=True``) on slice-last data: one launch each way
(wire_radon_vol_fwd / wire_radon_vol_bwd), the adjoint a gather without atomics.

``get_video_coding_frames`` / ``video2codedvideo``: video compressive sensing, the per-pixel coded exposure of Hitomi
et al. (modules/lin_inverse.py:42-95).  The masks are host numpy with the reference's random draw (the same
``np.random.seed`` gives the same masks); the coding and its adjoint are one HIP kernel each (wire_coded_fwd /
wire_coded_bwd) behind an autograd.Function.  A training loop does not need either tensor form: in the row order of
the 3-D grid ``FusedTrainer.step_coded`` computes the coded loss and its gradient in one pass over the network's
output (wire_coded_mse_grad), without the ``reshape(H, W, T).permute(2, 0, 1)`` into this layout.
"""
from __future__ import annotations

import numpy as np
import torch

from .. import _lib


class _RadonFunction(torch.autograd.Function):
    @staticmethod
    def forward(ctx, img, angles):
        L = _lib.lib()
        if not img.is_cuda:
            raise _lib.WireHipError("radon: tensors must be on the MI355X ('cuda'); wire_amd has no CPU path")
        H, W = img.shape[-2], img.shape[-1]
        x = img.detach().to(torch.float32).contiguous().reshape(-1, H, W)
        ang = angles.detach().to(img.device, torch.float32).contiguous()
        A = ang.numel()
        out = torch.empty(x.shape[0], A, W, dtype=torch.float32, device=img.device)
        stream = torch.cuda.current_stream(img.device).cuda_stream
        for i in range(x.shape[0]):
            _lib.check(L.wire_radon_fwd(stream, x[i].data_ptr(), ang.data_ptr(), H, W, A, out[i].data_ptr()),
                       "wire_radon_fwd")
        ctx.save_for_backward(ang)
        ctx.shape = (tuple(img.shape), H, W, A)
        return out

    @staticmethod
    def backward(ctx, g):
        L = _lib.lib()
        (ang,) = ctx.saved_tensors
        shape, H, W, A = ctx.shape
        gg = g.detach().to(torch.float32).contiguous().reshape(-1, A, W)
        gi = torch.empty(gg.shape[0], H, W, dtype=torch.float32, device=g.device)
        stream = torch.cuda.current_stream(g.device).cuda_stream
        for i in range(gg.shape[0]):
            _lib.check(L.wire_radon_bwd(stream, gg[i].data_ptr(), ang.data_ptr(), H, W, A, gi[i].data_ptr()),
                       "wire_radon_bwd")
        return gi.reshape(shape), None


def radon(imten, angles, is_3d=False):
    """Forward Radon transform (modules/lin_inverse.py:19-40).

    imten: (1, nimg, H, W) image tensor; angles: (nangles) degrees, same device.
    Returns the sinogram: (nangles, W) for one image (the reference's ``.squeeze()``), (nimg, nangles, W) with
    ``is_3d=True``."""
    if imten.dim() != 4 or imten.shape[0] != 1:
        raise ValueError("radon expects imten of shape (1, nimg, H, W)")
    sino = _RadonFunction.apply(imten[0], angles)          # (nimg, nangles, W)
    if is_3d:
        return sino
    return sino.permute(1, 0, 2).squeeze()


class _RadonVolumeFunction(torch.autograd.Function):
    @staticmethod
    def forward(ctx, vol, angles):
        L = _lib.lib()
        H, W, T = vol.shape
        x = vol.detach().to(torch.float32).contiguous()
        ang = angles.detach().to(vol.device, torch.float32).contiguous().reshape(-1)
        A = ang.numel()
        out = torch.empty(A, W, T, dtype=torch.float32, device=vol.device)
        stream = torch.cuda.current_stream(vol.device).cuda_stream
        _lib.check(L.wire_radon_vol_fwd(stream, x.data_ptr(), ang.data_ptr(), H, W, T, A, out.data_ptr()),
                   "wire_radon_vol_fwd")
        ctx.save_for_backward(ang)
        ctx.args = (H, W, T, A, vol.dtype)
        return out

    @staticmethod
    def backward(ctx, g):
        L = _lib.lib()
        (ang,) = ctx.saved_tensors
        H, W, T, A, dtype = ctx.args
        gg = g.detach().to(torch.float32).contiguous()
        gv = torch.empty(H, W, T, dtype=torch.float32, device=g.device)
        stream = torch.cuda.current_stream(g.device).cuda_stream
        _lib.check(L.wire_radon_vol_bwd(stream, gg.data_ptr(), ang.data_ptr(), H, W, T, A, gv.data_ptr()),
                   "wire_radon_vol_bwd")
        return gv.to(dtype), None


def radon_volume(vol, angles):
    """The Radon transform of every slice of a volume stored slice-last (ours; the layout of a 3-D grid's rows).

    vol: (H, W, T) tensor on the MI355X, slice k being ``vol[:, :, k]``; angles: (nangles) degrees.  Returns the
    (nangles, W, T) float32 stack of sinograms.  In the reference's layout this is

        radon(v.permute(2, 0, 1)[None], angles, is_3d=True).permute(1, 2, 0)

    bit for bit, as one launch over contiguous memory (wire_radon_vol_fwd) instead of one per slice and two transposes.
    The backward is the gather adjoint (wire_radon_vol_bwd): no atomics, the same bits on every call, which ``radon``'s
    scatter does not give.  The gradient flows to ``vol`` only."""
    if not isinstance(vol, torch.Tensor) or vol.dim() != 3 or min(vol.shape) < 1:
        raise ValueError("radon_volume expects vol of shape (H, W, T)")
    if not isinstance(angles, torch.Tensor) or angles.numel() < 1:
        raise ValueError("radon_volume expects at least one angle")
    if not vol.is_cuda:
        raise _lib.WireHipError("radon_volume: tensors must be on the MI355X ('cuda'); wire_amd has no CPU path")
    return _RadonVolumeFunction.apply(vol, angles)


def get_video_coding_frames(video_size, nframes):
    """Masks for video compressive sensing (modules/lin_inverse.py:42-63): every pixel is open in one random frame of
    each group of ``nframes`` frames, the same frame in every group.

    video_size: (H, W, totalframes).  Returns the float64 (H, W, totalframes) array of zeros and ones.  The one random
    draw is ``np.random.randint(0, nframes, (H, W))``, so the same ``np.random.seed`` gives the reference's masks."""
    H, W, totalframes = (int(v) for v in video_size)
    nframes = int(nframes)
    open_frame = np.random.randint(0, nframes, (H, W))
    group = (np.arange(nframes) == open_frame[..., None]).astype(np.float64)
    return np.tile(group, (1, 1, totalframes // nframes + 1))[..., :totalframes]


class _CodedVideoFunction(torch.autograd.Function):
    @staticmethod
    def forward(ctx, video, masks, nframes, dup_last):
        L = _lib.lib()
        T, H, W = video.shape
        x = video.detach().to(torch.float32).contiguous()
        C = (T + nframes - 1) // nframes
        out = torch.empty(C + dup_last, H, W, dtype=torch.float32, device=video.device)
        stream = torch.cuda.current_stream(video.device).cuda_stream
        _lib.check(L.wire_coded_fwd(stream, x.data_ptr(), masks.data_ptr(), T, H * W, nframes, dup_last,
                                    out.data_ptr()), "wire_coded_fwd")
        ctx.save_for_backward(masks)
        ctx.args = (T, H, W, nframes, dup_last, video.dtype)
        return out

    @staticmethod
    def backward(ctx, g):
        L = _lib.lib()
        (masks,) = ctx.saved_tensors
        T, H, W, nframes, dup_last, dtype = ctx.args
        gg = g.detach().to(torch.float32).contiguous()
        gv = torch.empty(T, H, W, dtype=torch.float32, device=g.device)
        stream = torch.cuda.current_stream(g.device).cuda_stream
        _lib.check(L.wire_coded_bwd(stream, gg.data_ptr(), masks.data_ptr(), T, H * W, nframes, dup_last,
                                    gv.data_ptr()), "wire_coded_bwd")
        return gv.to(dtype), None, None, None


def video2codedvideo(video_ten, masks_ten, nframes, dup_last=True):
    """Video to coded video (modules/lin_inverse.py:65-95): every group of ``nframes`` frames of ``video_ten * masks_ten``
    summed into one coded frame.

    video_ten, masks_ten: (1, totalframes, H, W) tensors on the MI355X.  Returns (1, C + 1, H, W) float32 with
    C = ceil(totalframes / nframes): as in the reference, whose trailing ``if idx < video_ten.shape[1]`` always holds,
    the last group comes twice.  ``dup_last=False`` (ours) gives the plain C frames.  The gradient flows to
    ``video_ten`` only."""
    if video_ten.dim() != 4 or video_ten.shape[0] != 1:
        raise ValueError("video2codedvideo expects video_ten of shape (1, totalframes, H, W)")
    if tuple(masks_ten.shape) != tuple(video_ten.shape):
        raise ValueError("masks_ten must have the shape of video_ten")
    if not video_ten.is_cuda or not masks_ten.is_cuda:
        raise _lib.WireHipError("video2codedvideo: tensors must be on the MI355X ('cuda'); wire_amd has no CPU path")
    nframes = int(nframes)
    if nframes < 1:
        raise ValueError("nframes must be >= 1")
    masks = masks_ten.detach()[0].to(torch.float32).contiguous()
    return _CodedVideoFunction.apply(video_ten[0], masks, nframes, int(bool(dup_last)))[None]
