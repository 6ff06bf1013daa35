"""A numpy fp64 restatement of the volume-rendering operator (wire_amd/csrc/wire_render.hip): the sampler with the
device's order of operations and its single rounding, the emission-absorption compositing, and its closed-form adjoint.
"""
import numpy as np


def ray_samples(rays, near, far, S, jitter=None):
    """rays [R, 6] fp32, near / far scalars or [R] fp32, jitter None or [R, S] fp32 in [0, 1) ->
    (coords [R*S, 3], ts [R, S], deltas [R, S]) fp32: fp64 arithmetic, left to right, rounded once."""
    rays = np.asarray(rays, np.float32).astype(np.float64)
    R = rays.shape[0]
    o, d = rays[:, None, 0:3], rays[:, None, 3:6]
    nr = np.broadcast_to(np.asarray(near, np.float32).astype(np.float64), (R,))[:, None]
    fr = np.broadcast_to(np.asarray(far, np.float32).astype(np.float64), (R,))[:, None]
    u = np.full((R, S), 0.5) if jitter is None else np.asarray(jitter, np.float32).astype(np.float64)
    s = np.arange(S, dtype=np.float64)[None, :]
    with np.errstate(invalid="ignore", over="ignore"):
        t = nr + ((s + u) * (fr - nr)) / float(S)
        t1 = np.concatenate([t[:, 1:], np.broadcast_to(fr, (R, 1))], axis=1)
        norm = np.sqrt(d[..., 0] * d[..., 0] + d[..., 1] * d[..., 1] + d[..., 2] * d[..., 2])
        dl = (t1 - t) * norm
    hit = fr > nr
    t = np.where(hit, t, np.broadcast_to(nr, (R, S)))
    dl = np.where(hit, dl, 0.0)
    coords = o + t[..., None] * d
    return (coords.reshape(R * S, 3).astype(np.float32), t.astype(np.float32), dl.astype(np.float32))


def _sigmoid(x):
    e = np.exp(-np.abs(x))
    return np.where(x >= 0, 1.0 / (1.0 + e), e / (1.0 + e))


def _density(x, density):
    if density == "softplus":
        return np.maximum(x, 0.0) + np.log1p(np.exp(-np.abs(x))), _sigmoid(x)
    if density == "relu":
        return np.maximum(x, 0.0), (x > 0).astype(np.float64)
    raise ValueError(density)


def _weights(y, ts, deltas, density):
    R, S = ts.shape
    y = np.asarray(y, np.float64).reshape(R, S, -1)
    ts, deltas = np.asarray(ts, np.float64), np.asarray(deltas, np.float64)
    c = _sigmoid(y[..., :-1])
    sigma, dsigma = _density(y[..., -1], density)
    a = sigma * deltas
    tau1 = np.cumsum(a, axis=1)                                  # tau_{s+1}
    tau =np.concatenate([np.zeros((R, 1)), tau1[:, :-1]], axis=1)
    T, T1 = np.exp(-tau), np.exp(-tau1)
    w = T * -np.expm1(-a)
    return c, dsigma, ts, deltas, T1, w


def composite(y, ts, deltas, bg=None, density="softplus"):
    """y [R*S, O] (or [R, S, O]), ts / deltas [R, S] -> (rgb [R, C], acc [R], depth [R]) in fp64."""
    c, _, ts, _, T1, w = _weights(y, ts, deltas, density)
    TS = T1[:, -1]
    rgb = (w[..., None] * c).sum(axis=1)
    if bg is not None:
        rgb = rgb + TS[:, None] * np.asarray(bg, np.float64)[None, :]
    return rgb, 1.0 - TS, (w * ts).sum(axis=1)


def composite_bwd(y, ts, deltas, g_rgb, g_acc=None, g_depth=None, bg=None, density="softplus"):
    """The closed-form adjoint: g_y [R*S, O] in fp64.  acc = 1 - T_S depends on the densities through T_S alone, so
    g_acc enters q_bg (with a minus sign) and not q_s:
        q_s = <c_s, g_rgb> + t_s g_depth,    q_bg = <bg, g_rgb> - g_acc
        d/dsigma_s = delta_s (T_{s+1} q_s - sum_{j>s} w_j q_j - T_S q_bg),    d/dc_raw_s = w_s g_rgb c (1 - c)"""
    c, dsigma, ts, deltas, T1, w = _weights(y, ts, deltas, density)
    R, S = ts.shape
    g_rgb = np.asarray(g_rgb, np.float64)
    ga = np.zeros(R) if g_acc is None else np.asarray(g_acc, np.float64)
    gd = np.zeros(R) if g_depth is None else np.asarray(g_depth, np.float64)
    q = (c * g_rgb[:, None, :]).sum(axis=2) + ts * gd[:, None]
    q_bg = -ga
    if bg is not None:
        q_bg = q_bg + g_rgb @ np.asarray(bg, np.float64)
    wq = w * q
    later = np.concatenate([np.cumsum(wq[:, ::-1], axis=1)[:, ::-1][:, 1:], np.zeros((R, 1))], axis=1)
    g_sigma = deltas * (T1 * q - later - (T1[:, -1] * q_bg)[:, None])
    g = np.empty((R, S, c.shape[2] + 1))
    g[..., :-1] = w[..., None] * g_rgb[:, None, :] * c * (1.0 - c)
    g[..., -1] = g_sigma * dsigma
    return g.reshape(R * S, -1)


def mse_and_grad(rgb, target):
    """loss = mean (rgb - target)^2 and d loss / d rgb, fp64."""
    d = np.asarray(rgb, np.float64) - np.asarray(target, np.float64)
    return float((d * d).mean()), 2.0 * d / d.size


def torch_composite(y, ts, deltas, bg=None, density="softplus"):
    """The cumsum / cumprod form in eager torch, in the dtype of ``y``: the autograd yardstick in fp64 and the error
    scale (err_ref) in fp32."""
    import torch
    R, S = ts.shape
    y = y.reshape(R, S, -1)
    c = torch.sigmoid(y[..., :-1])
    sigma = torch.nn.functional.softplus(y[..., -1]) if density == "softplus" else torch.relu(y[..., -1])
    alpha = 1.0 - torch.exp(-sigma * deltas)
    T = torch.cumprod(torch.cat([torch.ones_like(alpha[:, :1]), 1.0 - alpha], dim=1), dim=1)
    w = T[:, :-1] * alpha
    rgb = (w[..., None] * c).sum(dim=1)
    if bg is not None:
        rgb = rgb + T[:, -1:] * bg[None, :]
    return rgb, 1.0 - T[:, -1], (w * ts).sum(dim=1)
