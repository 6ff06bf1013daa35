"""numpy restatement of the quadratic B-spline INR (modules/bspline_form.py) for the bspline_form tests.

Two arithmetics of the same function:
  * ``closed`` (fp64 oracle): B(r) = 0.75 - r^2 (|r| <= 0.5), 0.5 (1.5 - |r|)^2 (0.5 <= |r| <= 1.5), 0 otherwise;
  * ``four`` (the reference's own fp32 arithmetic, bspline_form.py:38-49): lin / s, then
    0.5 relu(r+1.5)^2 - 1.5 relu(r+0.5)^2 + 1.5 relu(r-0.5)^2 - 0.5 relu(r-1.5)^2, and its autograd derivative
    relu(r+1.5) - 3 relu(r+0.5) + 3 relu(r-0.5) - relu(r-1.5), divided by s.
The nets are lists of (W, b) per activation layer plus the final (W_f, b_f) (None when outermost_linear=False).
"""
import numpy as np


def bspline(r, form="closed"):
    r = np.asarray(r)
    if form == "four":
        t = r.dtype.type
        q = lambda x: np.square(np.maximum(x, t(0)))
        return t(0.5) * q(r + t(1.5)) - t(1.5) * q(r + t(0.5)) + t(1.5) * q(r - t(0.5)) - t(0.5) * q(r - t(1.5))
    a = np.abs(r)
    return np.where(a <= 0.5, 0.75 - r * r, np.where(a < 1.5, 0.5 * np.square(1.5 - a), 0.0)).astype(r.dtype)


def bspline_d(r, form="closed"):
    r = np.asarray(r)
    if form == "four":
        t = r.dtype.type
        p = lambda x: np.maximum(x, t(0))
        # d/dr of c relu(x)^2 = 2 c relu(x)
        return p(r + t(1.5)) - t(3.0) * p(r + t(0.5)) + t(3.0) * p(r - t(0.5)) - p(r - t(1.5))
    a = np.abs(r)
    return np.where(a <= 0.5, -2.0 * r, np.where(a < 1.5, -np.sign(r) * (1.5 - a), 0.0)).astype(r.dtype)


def _form(dt):
    return "four" if dt == np.float32 else "closed"


def forward(layers, final, x, s, dt=np.float64, keep=False):
    """y of the net; layers = [(W, b)], final = (W_f, b_f) or None; s = the reference's sigma0 (a divisor)."""
    f = _form(dt)
    h = np.asarray(x, dt)
    sv = dt(s)
    cache = []
    for W, b in layers:
        lin = h @ np.asarray(W, dt).T + np.asarray(b, dt)
        r = lin / sv
        cache.append((h, r))
        h = bspline(r, f)
    if final is not None:
        cache.append((h, None))
        h = h @ np.asarray(final[0], dt).T + np.asarray(final[1], dt)
    return (h, cache) if keep else h


def backward(layers, final, cache, gy, s, dt=np.float64):
    """Gradients [(g_W, g_b)] of the activation layers, (g_Wf, g_bf) or None, and g_x."""
    f = _form(dt)
    g = np.asarray(gy, dt)
    sv = dt(s)
    gf = None
    if final is not None:
        h = cache[-1][0]
        gf = (g.T @ h, g.sum(0))
        g = g @ np.asarray(final[0], dt)
    out = []
    for l in range(len(layers) - 1, -1, -1):
        h, r = cache[l]
        gl = g * bspline_d(r, f) / sv
        out.append((gl.T @ h, gl.sum(0)))
        g = gl @ np.asarray(layers[l][0], dt)
    return out[::-1], gf, g


def mse(y, t):
    d = y - t
    return float(np.mean(np.square(d.astype(np.float64)))), (y.dtype.type(2.0) / y.dtype.type(d.size)) * d


def net_from_state(sd, L, outermost_linear=True):
    """(layers, final) from a bspline_form state_dict of numpy arrays."""
    layers = [(sd[f"net.{l}.linear.weight"], sd[f"net.{l}.linear.bias"]) for l in range(L + 1)]
    if outermost_linear:
        return layers, (sd[f"net.{L + 1}.weight"], sd[f"net.{L + 1}.bias"])
    layers.append((sd[f"net.{L + 1}.linear.weight"], sd[f"net.{L + 1}.linear.bias"]))
    return layers, None


def grads_by_key(gl, gf, L, outermost_linear=True):
    out = {}
    for l, (gw, gb) in enumerate(gl):
        out[f"net.{l}.linear.weight"], out[f"net.{l}.linear.bias"] = gw, gb
    if gf is not None:
        out[f"net.{L + 1}.weight"], out[f"net.{L + 1}.bias"] = gf
    return out


def loss_and_grads(sd, L, x, t, s, dt, outermost_linear=True, chunk=16384):
    """y, MSE loss and every parameter gradient (by state_dict key) over all rows, in row chunks."""
    layers, final = net_from_state(sd, L, outermost_linear)
    n = x.shape[0]
    ys, grads = [], None
    for a in range(0, n, chunk):
        y, cache = forward(layers, final, x[a:a + chunk], s, dt, keep=True)
        ys.append(y)
        gy = (dt(2.0) / dt(t.size)) * (y - np.asarray(t[a:a + chunk], dt))
        gl, gf, _ = backward(layers, final, cache, gy, s, dt)
        g = grads_by_key(gl, gf, L, outermost_linear)
        grads = g if grads is None else {k: grads[k] + g[k] for k in g}
    y = np.concatenate(ys, 0)
    return y, float(np.mean(np.square(y.astype(np.float64) - t))), grads
