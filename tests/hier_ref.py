"""numpy restatement of the hierarchical B-spline INR (modules/bspline_mscale_hier.py) for the bspline_mscale_hier tests.

Stage s divides every pre-activation by st[s].  Stage 0 runs its L + 1 layers on the coordinates; stage s > 0 runs its
layer 0 on the coordinates, its layer 1 on [that | x_{s-1}] and its layer 2; y = sum_s (x_s Wh_s^T + bh_s).  fp64 uses the
closed form of B, fp32 the reference's own four-relu arithmetic (bspline_ref._form).  ``sd`` holds the state_dict's
arrays by key, ``heads`` the heads' by "linears.{s}.weight" / "linears.{s}.bias".
"""
import numpy as np

import bspline_ref as br


def used_layers(s, L):
    return range(L + 1) if s == 0 else range(3)


def _wb(sd, s, l, dt):
    return np.asarray(sd[f"stages.{s}.{l}.linear.weight"], dt), np.asarray(sd[f"stages.{s}.{l}.linear.bias"], dt)


def forward(sd, heads, L, x, st, dt, keep=False):
    f = br._form(dt)
    x = np.asarray(x, dt)
    y, prev, caches = None, None, []
    for s, sig in enumerate(st):
        sv = dt(sig)
        h, cache = x, []
        for l in used_layers(s, L):
            W, b = _wb(sd, s, l, dt)
            if s > 0 and l == 1:
                h = np.concatenate([h, prev], -1)
            r = (h @ W.T + b) / sv
            cache.append((h, r))
            h = br.bspline(r, f)
        prev = h
        caches.append((cache, h))
        v = h @ np.asarray(heads[f"linears.{s}.weight"], dt).T + np.asarray(heads[f"linears.{s}.bias"], dt)
        y = v if y is None else y + v
    return (y, caches) if keep else y


def _chunk(sd, heads, L, x, t, size, st, dt):
    f = br._form(dt)
    y, caches = forward(sd, heads, L, x, st, dt, keep=True)
    gy = (dt(2.0) / dt(size)) * (y - np.asarray(t, dt))
    g = {}
    gx = np.zeros_like(np.asarray(x, dt))
    carry = None
    K = caches[0][1].shape[1]
    for s in range(len(st) - 1, -1, -1):
        sv = dt(st[s])
        cache, xs = caches[s]
        g[f"linears.{s}.weight"], g[f"linears.{s}.bias"] = gy.T @ xs, gy.sum(0)
        gh = gy @ np.asarray(heads[f"linears.{s}.weight"], dt)
        if carry is not None:
            gh = gh + carry
        carry = None
        for l in reversed(list(used_layers(s, L))):
            h, r = cache[l]
            W, _ = _wb(sd, s, l, dt)
            gl = gh * br.bspline_d(r, f) / sv
            g[f"stages.{s}.{l}.linear.weight"], g[f"stages.{s}.{l}.linear.bias"] = gl.T @ h, gl.sum(0)
            gh = gl @ W
            if s > 0 and l == 1:
                gh, carry = gh[:, :K], gh[:, K:]
        gx = gx + gh
    return y, g, gx


def loss_and_grads(sd, heads, L, x, t, st, dt, chunk=8192):
    """y, the MSE loss, every gradient (stages by state_dict key, heads by "linears.{s}.*") and g_x over all rows, in
    row chunks."""
    n = x.shape[0]
    ys, gxs, grads = [], [], None
    for a in range(0, n, chunk):
        y, g, gx = _chunk(sd, heads, L, x[a:a + chunk], t[a:a + chunk], t.size, st, dt)
        ys.append(y)
        gxs.append(gx)
        grads = g if grads is None else {k: grads[k] + g[k] for k in g}
    y = np.concatenate(ys, 0)
    return y, float(np.mean(np.square(y.astype(np.float64) - t))), grads, np.concatenate(gxs, 0)


def adam_step(p, g, m, v, lr, t, b1=0.9, b2=0.999, eps=1e-8):
    """torch.optim.Adam's update of one tensor (fp64); returns (p, m, v)."""
    m = b1 * m + (1 - b1) * g
    v = b2 * v + (1 - b2) * g * g
    step = lr / (1 - b1 ** t)
    return p - step * m / (np.sqrt(v) / np.sqrt(1 - b2 ** t) + eps), m, v
