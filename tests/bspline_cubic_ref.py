"""numpy restatement of the cubic B-spline INR (modules/bspline_cubic.py) for the bspline_cubic tests.

One layer: lin = s (x W^T) + b -- the scale multiplies the layer's INPUT, the bias is not scaled, the sign of s matters.
Two arithmetics of the same activation, each in fp32 or fp64 (``form=``):
  * ``piecewise`` (the closed form; in fp64 the oracle, in fp32 the yardstick ``err_ref`` of the parity protocol):
      B(l)  = 2/3 - l^2 + |l|^3 / 2 (|l| < 1),  (2 - |l|)^3 / 6 (1 <= |l| < 2),  0 otherwise
      B'(l) = -2 l + (3/2) l |l|,               -sign(l) (2 - |l|)^2 / 2,        0
  * ``five`` (the reference's own arithmetic, bspline_cubic.py:44-52): linear(s * x), then
      (1/6) relu(l+2)^3 - (2/3) relu(l+1)^3 + relu(l)^3 - (2/3) relu(l-1)^3 + (1/6) relu(l-2)^3
    and its autograd derivative (1/2) relu(l+2)^2 - 2 relu(l+1)^2 + 3 relu(l)^2 - 2 relu(l-1)^2 + (1/2) relu(l-2)^2.
    For |l| > 2 its terms cancel from |l|^3: in fp32 it is wrong in the third digit at the class's scale of 15.
The nets are lists of (W, b) per activation layer plus the final (W_f, b_f) (None when outermost_linear=False), the
interface of tests/bspline_ref.py.
"""
import numpy as np

FORMS = ("piecewise", "five")


def bspline3(l, form="piecewise"):
    l = np.asarray(l)
    t = l.dtype.type
    if form == "five":
        def c(x):                                    # relu(x) ** 3 as torch evaluates it: r * r * r (numpy's ** calls pow)
            r = np.maximum(x, t(0))
            return r * r * r
        return (t(1 / 6) * c(l + t(2)) - t(2 / 3) * c(l + t(1)) + c(l) - t(2 / 3) * c(l - t(1)) + t(1 / 6) * c(l - t(2)))
    a = np.abs(l)
    u = np.maximum(t(2) - a, t(0))
    inner = t(2 / 3) - a * a + t(0.5) * a * a * a
    return np.where(a < 1, inner, u * u * u * t(1 / 6)).astype(l.dtype)


def bspline3_d(l, form="piecewise"):
    l = np.asarray(l)
    t = l.dtype.type
    if form == "five":
        q = lambda x: np.square(np.maximum(x, t(0)))
        # d/dl of c relu(x)^3 = 3 c relu(x)^2
        return (t(0.5) * q(l + t(2)) - t(2) * q(l + t(1)) + t(3) * q(l) - t(2) * q(l - t(1)) + t(0.5) * q(l - t(2)))
    a = np.abs(l)
    u = np.maximum(t(2) - a, t(0))
    inner = t(-2) * l + t(1.5) * l * a
    return np.where(a < 1, inner, -np.sign(l) * t(0.5) * u * u).astype(l.dtype)


def forward(layers, final, x, s, dt=np.float64, keep=False, form="piecewise"):
    """y of the net; layers = [(W, b)], final = (W_f, b_f) or None; s = scale_0, the multiplier of every layer's input."""
    h = np.asarray(x, dt)
    sv = dt(s)
    cache = []
    for W, b in layers:
        hs = sv * h                                  # linear(scale_0 * input), as the reference orders it
        lin = hs @ np.asarray(W, dt).T + np.asarray(b, dt)
        cache.append((hs, lin))
        h = bspline3(lin, form)
    if final is not None:
        cache.append((h, None))
        h = h @ np.asarray(final[0], dt).T + np.asarray(final[1], dt)
    return (h, cache) if keep else h


def backward(layers, final, cache, gy, s, dt=np.float64, form="piecewise"):
    """Gradients [(g_W, g_b)] of the activation layers, (g_Wf, g_bf) or None, and g_x."""
    g = np.asarray(gy, dt)
    sv = dt(s)
    gf = None
    if final is not None:
        h = cache[-1][0]
        gf = (g.T @ h, g.sum(0))
        g = g @ np.asarray(final[0], dt)
    out = []
    for l in range(len(layers) - 1, -1, -1):
        hs, lin = cache[l]
        gl = g * bspline3_d(lin, form)
        out.append((gl.T @ hs, gl.sum(0)))           # g_W = g_lin^T (s x): the factor once; g_b = sum g_lin
        g = sv * (gl @ np.asarray(layers[l][0], dt)) # g_x = s g_lin W
    return out[::-1], gf, g


def mse(y, t):
    d = y - t
    return float(np.mean(np.square(d.astype(np.float64)))), (y.dtype.type(2.0) / y.dtype.type(d.size)) * d


def net_from_state(sd, L, outermost_linear=True):
    """(layers, final) from a bspline_cubic state_dict of numpy arrays."""
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


def loss_and_grads(sd, L, x, t, s, dt, outermost_linear=True, chunk=16384, form="piecewise"):
    """y, MSE loss and every parameter gradient (by state_dict key) over all rows, in row chunks."""
    layers, final = net_from_state(sd, L, outermost_linear)
    n = x.shape[0]
    ys, grads = [], None
    for a in range(0, n, chunk):
        y, cache = forward(layers, final, x[a:a + chunk], s, dt, keep=True, form=form)
        ys.append(y)
        gy = (dt(2.0) / dt(t.size)) * (y - np.asarray(t[a:a + chunk], dt))
        gl, gf, _ = backward(layers, final, cache, gy, s, dt, form=form)
        g = grads_by_key(gl, gf, L, outermost_linear)
        grads = g if grads is None else {k: grads[k] + g[k] for k in g}
    y = np.concatenate(ys, 0)
    return y, float(np.mean(np.square(y.astype(np.float64) - t))), grads
