"""numpy restatement of the multi-scale B-spline INR (modules/bspline_mscale_HL.py) for the bspline_mscale_HL tests.

The first stage divides column j of lin = x W0^T + b0 by scale_tensor[g(j)] (``column_groups``) and applies B; it passes
no gradient.  Behind it the net is the bspline_form chain of tests/bspline_ref.py (SHF -> K, K -> K, final linear), in
the same two arithmetics: fp64 closed form (the oracle) and the reference's fp32 four-term form.
"""
import numpy as np

import bspline_ref as br


def column_groups(shf, T):
    if shf <= 256:
        return np.zeros(shf, np.int64)
    split = (shf - 256) // (T - 1)
    j = np.arange(shf)
    return np.where(j < 256, 0, 1 + (j - 256) // max(split, 1)).astype(np.int64)


def first_stage(W0, b0, x, scales, dt=np.float64):
    lin = np.asarray(x, dt) @ np.asarray(W0, dt).T + np.asarray(b0, dt)
    div = np.asarray(scales, dt)[column_groups(W0.shape[0], len(scales))]
    return br.bspline(lin / div, "four" if dt == np.float32 else "closed")


def net_from_state(sd, hidden_layers):
    """(W0, b0), [(W, b)] of the layers behind the first stage, (W_f, b_f) from a state_dict of numpy arrays."""
    nl = 1 + max(hidden_layers - 1, 0)
    layers = [(sd[f"net.{l}.linear.weight"], sd[f"net.{l}.linear.bias"]) for l in range(1, nl + 1)]
    final = (sd[f"net.{nl + 1}.weight"], sd[f"net.{nl + 1}.bias"])
    return (sd["net.0.linear.weight"], sd["net.0.linear.bias"]), layers, final


def loss_and_grads(sd, hidden_layers, x, t, scales, s, dt, chunk=16384):
    """y, MSE loss and the gradient of every parameter that receives one (by state_dict key), over all rows."""
    (W0, b0), layers, final = net_from_state(sd, hidden_layers)
    nl = len(layers)
    n = x.shape[0]
    ys, grads = [], None
    for a in range(0, n, chunk):
        h0 = first_stage(W0, b0, x[a:a + chunk], scales, dt)
        y, cache = br.forward(layers, final, h0, s, dt, keep=True)
        ys.append(y)
        gy = (dt(2.0) / dt(t.size)) * (y - np.asarray(t[a:a + chunk], dt))
        gl, gf, _ = br.backward(layers, final, cache, gy, s, dt)
        g = {}
        for l, (gw, gb) in enumerate(gl):
            g[f"net.{l + 1}.linear.weight"], g[f"net.{l + 1}.linear.bias"] = gw, gb
        g[f"net.{nl + 1}.weight"], g[f"net.{nl + 1}.bias"] = gf
        grads = g if grads is None else {k: grads[k] + g[k] for k in g}
    y = np.concatenate(ys, 0)
    return y, float(np.mean(np.square(y.astype(np.float64) - t))), grads
