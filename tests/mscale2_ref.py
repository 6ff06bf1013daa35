"""numpy restatement of the multi-pass B-spline INR (modules/bspline_mscale_2.py) for the bspline_mscale_2 tests.

The trunk is bspline_form's (tests/bspline_ref.py), run once per entry s_k of scale_tensor with lin / s_k; the S
outputs of a row, [t_0 | t_1 | ..], go through freq_mlp = Linear(S O -> 128), ReLU, Linear(128 -> O).  fp64 uses the
closed form of B, fp32 the reference's own four-relu arithmetic (bspline_ref._form).  ``mask`` (optional, [n][128]
bool) replaces the ReLU's own decisions h > 0.
"""
import numpy as np

import bspline_ref as br

COMB = ("combine_scales.freq_mlp.0.weight", "combine_scales.freq_mlp.0.bias", "combine_scales.freq_mlp.2.weight",
        "combine_scales.freq_mlp.2.bias")


def trunk_from_state(sd, L):
    layers = [(sd[f"net.{l}.linear.weight"], sd[f"net.{l}.linear.bias"]) for l in range(L + 1)]
    return layers, (sd[f"net.{L + 1}.weight"], sd[f"net.{L + 1}.bias"])


def forward(sd, L, x, st, dt, mask=None, keep=False):
    layers, final = trunk_from_state(sd, L)
    W1, b1, W2, b2 = (np.asarray(sd[k], dt) for k in COMB)
    outs, caches = [], []
    for s in st:
        t, cache = br.forward(layers, final, x, dt(s), dt, keep=True)
        outs.append(t)
        caches.append(cache)
    X = np.concatenate(outs, -1)
    h = X @ W1.T + b1
    m = (h > 0) if mask is None else mask
    a = np.where(m, h, dt(0))
    y = a @ W2.T + b2
    return (y, (X, m, a, caches)) if keep else y


def loss_and_grads(sd, L, x, t, st, dt, mask=None, chunk=8192):
    """y, the MSE loss, every parameter gradient that the reference's loop produces (by state_dict key) and g_x, over
    all rows in row chunks (rows are independent)."""
    n = x.shape[0]
    ys, gxs, grads = [], [], None
    for a in range(0, n, chunk):
        y, g, gx = _chunk(sd, L, x[a:a + chunk], t[a:a + chunk], t.size, st, dt,
                          None if mask is None else mask[a:a + chunk])
        ys.append(y)
        gxs.append(gx)
        grads = g if grads is None else {k: grads[k] + g[k] for k in g}
    y = np.concatenate(ys, 0)
    return y, float(np.mean(np.square(y.astype(np.float64) - t))), grads, np.concatenate(gxs, 0)


def _chunk(sd, L, x, t, size, st, dt, mask):
    x = np.asarray(x, dt)
    layers, final = trunk_from_state(sd, L)
    W1, W2 = np.asarray(sd[COMB[0]], dt), np.asarray(sd[COMB[2]], dt)
    y, (X, m, a, caches) = forward(sd, L, x, st, dt, mask, keep=True)
    gy = (dt(2.0) / dt(size)) * (y - np.asarray(t, dt))
    g = {COMB[2]: gy.T @ a, COMB[3]: gy.sum(0)}
    gh = np.where(m, gy @ W2, dt(0))
    g[COMB[0]], g[COMB[1]] = gh.T @ X, gh.sum(0)
    gX = gh @ W1
    O = y.shape[1]
    gx = np.zeros_like(x)
    for k, s in enumerate(st):
        gl, gf, gxk = br.backward(layers, final, caches[k], gX[:, k * O:(k + 1) * O], dt(s), dt)
        for key, v in br.grads_by_key(gl, gf, L).items():
            g[key] = g[key] + v if key in g else v
        gx = gx + gxk
    return y, g, gx
