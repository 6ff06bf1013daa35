"""Closed form of the multiplicative filter network (modules/mfn.py) in numpy, in a chosen dtype: forward, MSE loss and
every gradient.  The oracle of tests/test_mfn_host.py and tests/test_gpu_mfn.py (precedent: tests/bspline_ref.py).

    g_i(x)_j = exp(-gamma_ij / 2 * nrm_ij) sin(x . w_ij + c_ij),  nrm = |x|^2 + |mu|^2 - 2 x . mu   (mfn.py:24-26, the
                                                                  reference's expanded form, kept: in fp32 it is the
                                                                  reference's own arithmetic, err_ref of the protocol)
    z_0 = g_0(x);  lin_i = z_i W_i^T + b_i,  z_{i+1} = lin_i g_{i+1}(x);  y = z_L W_f^T + b_f        (mfn.py:46-54)

Backward, with f = e sin a, e = exp(-gamma nrm / 2), a = x . w + c and h the upstream gradient of a filter's output:
    g_gamma = sum_r h (-nrm / 2) f     g_mu = sum_r h gamma (x - mu) f     g_c = sum_r h e cos a     g_w = sum_r h e cos a x
    g_x    += sum_j h (-gamma (x - mu) f + e cos a w)
Rows are processed in chunks (the sums accumulate in the working dtype), so the 262 144-row shapes fit in memory.
"""
import numpy as np


def net_from_state(sd, L):
    """state_dict (numpy) -> (filters [(mu, gamma, w, c)] x (L + 1), linears [(W, b)] x (L + 1))"""
    fl = [tuple(sd[f"gabon_filters.{i}.{k}"] for k in ("mu", "gamma", "linear.weight", "linear.bias")) for i in range(L + 1)]
    ln = [(sd[f"linear.{i}.weight"], sd[f"linear.{i}.bias"]) for i in range(L + 1)]
    return fl, ln


def _cast(fl, ln, dt):
    return [tuple(np.asarray(t, dt) for t in f) for f in fl], [tuple(np.asarray(t, dt) for t in l) for l in ln]


def filter_parts(x, f):
    mu, gamma, w, c = f
    nrm = (x ** 2).sum(1)[:, None] + (mu ** 2).sum(1)[None, :] - 2 * x @ mu.T
    e = np.exp(-gamma[None, :] / 2 * nrm)
    a = x @ w.T + c[None, :]
    return nrm, e, np.sin(a), np.cos(a)


def filter_fwd(x, f, dt):
    x = np.asarray(x, dt)
    f = tuple(np.asarray(t, dt) for t in f)
    _, e, sn, _ = filter_parts(x, f)
    return e * sn


def filter_bwd(x, f, h, dt):
    """upstream gradient h [n][K] -> (g_mu, g_gamma, g_w, g_c, g_x)"""
    x, h = np.asarray(x, dt), np.asarray(h, dt)
    mu, gamma, w, c = f = tuple(np.asarray(t, dt) for t in f)
    nrm, e, sn, cs = filter_parts(x, f)
    hf, hc = h * (e * sn), h * (e * cs)
    g_gamma = (hf * (-nrm / 2)).sum(0)
    g_c = hc.sum(0)
    g_w = hc.T @ x
    hfg = hf * gamma[None, :]
    g_mu = hfg.T @ x - hfg.sum(0)[:, None] * mu
    g_x = hc @ w - (hfg.sum(1)[:, None] * x - hfg @ mu)
    return g_mu, g_gamma, g_w, g_c, g_x


def forward(fl, ln, x, dt, chunk=16384):
    fl, ln = _cast(fl, ln, dt)
    x = np.asarray(x, dt)
    out = []
    for r in range(0, len(x), chunk):
        xc = x[r:r + chunk]
        z = filter_fwd(xc, fl[0], dt)
        for i in range(len(fl) - 1):
            z = (z @ ln[i][0].T + ln[i][1]) * filter_fwd(xc, fl[i + 1], dt)
        out.append(z @ ln[-1][0].T + ln[-1][1])
    return np.concatenate(out, 0)


def loss_and_grads(sd, L, x, t, dt, chunk=16384, g_y=None):
    """(y, loss, grads keyed like the state_dict, g_x) of mean((y - t)^2); g_y given: its backward instead (loss None)"""
    fl, ln = _cast(*net_from_state(sd, L), dt)
    x = np.asarray(x, dt)
    n = len(x)
    O = ln[-1][0].shape[0]
    grads = {k: np.zeros(v.shape, dt) for k, v in sd.items()}
    ys, gxs, sq = [], [], dt(0)
    for r in range(0, n, chunk):
        xc = x[r:r + chunk]
        g = [filter_fwd(xc, f, dt) for f in fl]
        z, lin = [g[0]], []
        for i in range(L):
            lin.append(z[i] @ ln[i][0].T + ln[i][1])
            z.append(lin[i] * g[i + 1])
        y = z[L] @ ln[L][0].T + ln[L][1]
        ys.append(y)
        if g_y is None:
            d = y - np.asarray(t[r:r + chunk], dt)
            sq += (d * d).sum()
            gy = d * dt(2.0 / (n * O))
        else:
            gy = np.asarray(g_y[r:r + chunk], dt)
        grads[f"linear.{L}.weight"] += gy.T @ z[L]
        grads[f"linear.{L}.bias"] += gy.sum(0)
        gz = gy @ ln[L][0]
        gx = np.zeros_like(xc)
        for i in range(L, -1, -1):
            h = gz * lin[i - 1] if i > 0 else gz
            g_mu, g_gamma, g_w, g_c, gxi = filter_bwd(xc, fl[i], h, dt)
            for k, v in zip(("mu", "gamma", "linear.weight", "linear.bias"), (g_mu, g_gamma, g_w, g_c)):
                grads[f"gabon_filters.{i}.{k}"] += v
            gx += gxi
            if i > 0:
                gl = gz * g[i]
                grads[f"linear.{i - 1}.weight"] += gl.T @ z[i - 1]
                grads[f"linear.{i - 1}.bias"] += gl.sum(0)
                gz = gl @ ln[i - 1][0]
        gxs.append(gx)
    loss = None if g_y is not None else float(sq / (n * O))
    return np.concatenate(ys, 0), loss, grads, np.concatenate(gxs, 0)
