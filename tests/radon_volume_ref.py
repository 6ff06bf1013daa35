"""The volume form of the CT operator (wire_radon_vol_fwd / wire_radon_vol_bwd, include/wire_hip.h) in numpy: the
direct Radon form of tests/glue_ref.py and its adjoint, applied slice by slice to channel-last data.  fp64, or fp32 as
the yardstick of a comparison.  tests/test_radon_volume_host.py pins it on the CPU, tests/test_gpu_radon_volume.py
compares the kernels and FusedTrainer.step_radon_volume with it."""
import numpy as np

import glue_ref as gr

ANGLES = gr.ANGLES

# (H, W) of the GPU checks: no pair, one row, one column, all corners, the CT test's image, an odd one, and a width past
# one 256-thread workgroup at C = 1
SHAPES = [(1, 1), (1, 7), (7, 1), (2, 2), (24, 30), (33, 17), (5, 257)]
# channels: one (the 2-D operator), odd, the 16-byte vector width and one past it, one wave of the adjoint's channel
# lanes and one past it, and a multiple of 4 that is not a multiple of 64
CHANNELS = [1, 3, 4, 5, 64, 65, 68]


def radon_volume(vol, angles_deg, dtype=np.float64):
    """vol [H][W][C] -> [A][W][C]: glue_ref.radon on every slice vol[:, :, c]."""
    vol = np.asarray(vol)
    return np.stack([gr.radon(vol[:, :, c], angles_deg, dtype) for c in range(vol.shape[2])], axis=2)


def radon_volume_adjoint(g_sino, angles_deg, H, W, dtype=np.float64):
    """g_sino [A][W][C] -> [H][W][C]: glue_ref.radon_adjoint on every slice."""
    g = np.asarray(g_sino)
    return np.stack([gr.radon_adjoint(g[:, :, c], angles_deg, H, W, dtype) for c in range(g.shape[2])], axis=2)


def case(H, W, C, A=len(gr.ANGLES)):
    """(volume, sinogram-side stack, angles): positive values, as glue_ref.radon_case draws them, so that no sum
    cancels and a relative bound on the result is a bound on the operator."""
    rng = np.random.default_rng(H * 100003 + W * 1009 + C * 17 + A)
    return (rng.random((H, W, C)).astype(np.float32), (0.25 + rng.random((A, W, C))).astype(np.float32),
            gr.ANGLES[len(gr.ANGLES) - A:].copy())


def smooth_volume(H, W, T):
    """The smooth synthetic volume of the step checks: test_ct_radon.py's image, its phase moving with the slice."""
    yy, xx, tt = np.meshgrid(np.linspace(-1, 1, H), np.linspace(-1, 1, W), np.linspace(-1, 1, T), indexing="ij")
    return (0.5 + 0.4 * np.sin(3 * xx + tt) * np.cos(2 * yy - 0.5 * tt)).astype(np.float32)
