"""The multi-image super-resolution loss (wire_multi_sr.py:190-208) and the frames' coordinate stack
(modules/motion.py:284-318 at scale = 1) restated in numpy.  The yardstick of tests/test_multi_sr_host.py (which pins it
to torch.nn.AvgPool2d + torch.nn.MSELoss + autograd) and tests/test_gpu_multi_sr.py (precedent: tests/mfn_ref.py).

    rec[f] = mean of every scale x scale window of frame f ([H, W, O], row i*W + j), ragged borders dropped
    d      = rec * m - gt * m
    loss   = sum d^2 / (B H2 W2 O)                  -- the mean runs over every element, masked ones included
    dL/drec = 2 d m / (B H2 W2 O)                   -- the mask enters through d and through the product rule
    dL/dy   = dL/drec / scale^2 on every pixel of the window, 0 in the ragged borders
"""
import numpy as np


def frames_loss_and_grad(y, B, H, W, scale, gt_lr, mask=None, double=True):
    """y [B, H*W, O] (any shape of that size), gt_lr / mask [B, H2*W2, O] -> (loss, g_y [B, H*W, O], rec [B, H2*W2, O]).
    double=True: fp64 throughout.  double=False: fp32 in the reference's operation order -- the window summed row by
    row and divided by scale^2 (AvgPool2d), both products rounded before the subtraction (output*mask, gt*mask), the
    loss gradient 2 d / N times the mask, then divided by scale^2."""
    dt = np.float64 if double else np.float32
    y = np.asarray(y, dt)
    O = y.size // (B * H * W)
    H2, W2 = H // scale, W // scale
    img = y.reshape(B, H, W, O)[:, :H2 * scale, :W2 * scale].reshape(B, H2, scale, W2, scale, O)
    acc = np.zeros((B, H2, W2, O), dt)
    for a in range(scale):
        for b in range(scale):
            acc = acc + img[:, :, a, :, b, :]
    rec = acc / dt(scale * scale)
    gt = np.asarray(gt_lr, dt).reshape(B, H2, W2, O)
    m = np.ones_like(gt) if mask is None else np.asarray(mask, dt).reshape(B, H2, W2, O)
    d = rec * m - gt * m
    loss = np.mean(np.square(d), dtype=dt)
    g_rec = (dt(2.0) / dt(d.size)) * d * m
    g = np.zeros((B, H, W, O), dt)
    g[:, :H2 * scale, :W2 * scale] = np.repeat(np.repeat(g_rec / dt(scale * scale), scale, axis=1), scale, axis=2)
    return dt(loss), g.reshape(B, H * W, O), rec.reshape(B, H2 * W2, O)


def affine_coords(mats, H, W):
    """mats [B, 2, 3] -> fp64 [B, H*W, 2]: pixel (i, j) of frame f goes to Xn = m00 j + m01 i + m02,
    Yn = m10 j + m11 i + m12, normalised as (2 Xn / W - 1, 2 Yn / H - 1)."""
    mats = np.asarray(mats, np.float64)
    i, j = np.mgrid[:H, :W].astype(np.float64)
    out = np.empty((mats.shape[0], H, W, 2), np.float64)
    for f, m in enumerate(mats):
        xn = m[0, 0] * j + m[0, 1] * i + m[0, 2]
        yn = m[1, 0] * j + m[1, 1] * i + m[1, 2]
        out[f, ..., 0] = 2.0 * xn / W - 1.0
        out[f, ..., 1] = 2.0 * yn / H - 1.0
    return out.reshape(mats.shape[0], H * W, 2)


def make_mask(rng, B, H2W2, O):
    """Mask values 0, 1 and 0.5, with the last frame masked entirely."""
    m = rng.choice(np.array([0.0, 1.0, 0.5], np.float32), size=(B, H2W2, O))
    if B > 1:
        m[-1] = 0.0
    else:
        m[0, ::3] = 0.0
    return m.astype(np.float32)
