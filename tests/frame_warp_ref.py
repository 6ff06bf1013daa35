"""The learnable registration of frames (wire_warp_coords_fwd / wire_warp_coords_bwd, include/wire_hip.h) restated in
numpy.  The yardstick of tests/test_frame_warp_host.py (which pins it to torch autograd of the einsum and to
motion.get_transformed_coords) and of tests/test_gpu_frame_warp.py (precedent: tests/multi_sr_ref.py).

    out[f][p]       = theta[f] (x, y, 1)^T            fp64, left to right, rounded to fp32 once
    S[f][a][c]      = sum_p g_out[f][p][a] v_c        v = (x, y, 1); every product of two fp32 values is exact in fp64
    g_in[f][p]      = theta[f][:, :2]^T g_out[f][p]   fp64, left to right, rounded to fp32 once
"""
import math

import numpy as np


def warp(coords, theta):
    """coords [B, n, 2], theta [B, 2, 3] (fp32 values) -> fp32 [B, n, 2], the bits of wire_warp_coords_fwd."""
    c = np.asarray(coords, np.float32).astype(np.float64)
    t = np.asarray(theta, np.float32).astype(np.float64)
    x, y = c[..., 0], c[..., 1]
    out = np.empty(c.shape, np.float32)
    for a in range(2):
        out[..., a] = (t[:, a, 0, None] * x + t[:, a, 1, None] * y + t[:, a, 2, None]).astype(np.float32)
    return out


def warp_bwd(coords, theta, g_out, pin_first):
    """-> (S fp64 [B, 2, 3], the exactly rounded sums by math.fsum with frame 0 zeroed when pin_first;
           A fp64 [B, 2, 3], the sums of |terms| (not pinned);
           g_in fp32 [B, n, 2], the bits of wire_warp_coords_bwd)."""
    c = np.asarray(coords, np.float32).astype(np.float64)
    t = np.asarray(theta, np.float32).astype(np.float64)
    g = np.asarray(g_out, np.float32).astype(np.float64)
    B = c.shape[0]
    v = np.concatenate([c, np.ones(c.shape[:2] + (1,))], axis=-1)                  # [B, n, 3]
    S, A = np.zeros((B, 2, 3)), np.zeros((B, 2, 3))
    for f in range(B):
        for a in range(2):
            for k in range(3):
                terms = g[f, :, a] * v[f, :, k]                                     # exact
                S[f, a, k] = math.fsum(terms)
                A[f, a, k] = math.fsum(np.abs(terms))
    if pin_first:
        S[0] = 0.0
    gx, gy = g[..., 0], g[..., 1]
    g_in = np.empty(c.shape, np.float32)
    g_in[..., 0] = (t[:, 0, 0, None] * gx + t[:, 1, 0, None] * gy).astype(np.float32)
    g_in[..., 1] = (t[:, 0, 1, None] * gx + t[:, 1, 1, None] * gy).astype(np.float32)
    return S, A, g_in


def g_theta_bound(S, A, n_per):
    """|g_theta - S| <= 2^-24 |S| + n_per 2^-52 sum|terms|: one fp32 rounding plus the fp64 accumulation bound."""
    return 2.0 ** -24 * np.abs(S) + n_per * 2.0 ** -52 * A


def base_grid(H, W):
    """The align_corners=False grid of F.affine_grid on an (H, W) image: fp32 [H*W, 2], x = (2 j + 1) / W - 1."""
    i, j = np.mgrid[:H, :W].astype(np.float64)
    return np.stack([(2 * j + 1) / W - 1, (2 * i + 1) / H - 1], axis=-1).reshape(H * W, 2).astype(np.float32)
