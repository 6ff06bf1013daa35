"""The TV prior of the operator steps (wire_tv_add_grad) restated on numpy: the spatial and the temporal sum of an
(H, W, T) grid of O channels in the network's own rows, their exact integer sign patterns and the gradient accumulated
onto one that is already there.  The yardstick of tests/test_tv_reg_host.py and tests/test_gpu_tv_reg.py (precedent:
tests/tv_ref.py, whose 2-D functions the spatial part is checked against).

    y [H*W*T, O], element (i, j, k, o) at ((i W + j) T + k) O + o;   T = 1: an image
    tv_s = sum |y[i+1,j,k,o] - y[i,j,k,o]| + sum |y[i,j+1,k,o] - y[i,j,k,o]|     (utils.total_variation_loss per frame)
    tv_t = sum |y[i,j,k+1,o] - y[i,j,k,o]|
    k_s  = s(y - up) - s(down - y) + s(y - left) - s(right - y)   in -4 .. 4
    k_t  = s(y - previous) - s(next - y)                          in -2 .. 2
    g_out = g_in + (lambda_s k_s + lambda_t k_t);   loss = data + lambda_s tv_s + lambda_t tv_t

with s = sign by comparison, s(0) = 0, a term whose neighbour lies outside the grid being 0.
"""
import numpy as np


def grid4(y, H, W, T, O):
    """[H*W*T, O] rows (any shape of that size) -> the (H, W, T, O) view."""
    return np.asarray(y).reshape(H, W, T, O)


def _pair_sign(x, axis):
    """s(x[n + 1] - x[n]) along ``axis`` as int8, from comparisons of the values as they are."""
    hi = np.take(x, np.arange(1, x.shape[axis]), axis)
    lo = np.take(x, np.arange(0, x.shape[axis] - 1), axis)
    return (hi > lo).astype(np.int8) - (hi < lo).astype(np.int8)


def pair_signs(y, H, W, T, O):
    """The sign of every neighbour pair, one int8 array per axis (vertical, horizontal, temporal)."""
    x = grid4(y, H, W, T, O)
    return [_pair_sign(x, a) for a in range(3)]


def tv_sums(y, H, W, T, O, double=True):
    """(tv_s, tv_t) in fp64 or fp32 (numpy's pairwise sums)."""
    dt = np.float64 if double else np.float32
    x = grid4(y, H, W, T, O).astype(dt)
    dv, dh, dk = (np.abs(np.diff(x, axis=a)) for a in range(3))
    return np.sum(dv, dtype=dt) + np.sum(dh, dtype=dt), np.sum(dk, dtype=dt)


def sign_patterns(y, H, W, T, O):
    """(k_s, k_t): int8 arrays [H*W*T, O], k_s in -4 .. 4 and k_t in -2 .. 2."""
    x = grid4(y, H, W, T, O)
    ks, kt = np.zeros(x.shape, np.int8), np.zeros(x.shape, np.int8)
    for axis, k in ((0, ks), (1, ks), (2, kt)):
        s = _pair_sign(x, axis)
        n = x.shape[axis]
        hi = [slice(None)] * 4
        lo = [slice(None)] * 4
        hi[axis], lo[axis] = slice(1, n), slice(0, n - 1)
        k[tuple(hi)] += s                      # the pair's upper element: + s(own - lower)
        k[tuple(lo)] -= s                      # its lower element:       - s(upper - own)
    return ks.reshape(H * W * T, O), kt.reshape(H * W * T, O)


def tv_add_grad(y, g_in, H, W, T, O, lambda_s, lambda_t, data=0.0, double=True, pattern_from=None):
    """wire_tv_add_grad restated.  ``pattern_from`` (optional, shaped like y): the fp32 image whose comparisons give the
    sign patterns instead of y -- s is discontinuous, so an oracle in another precision takes the pattern of the image
    the kernel saw.  double=False follows the kernel's roundings: p = fl(lambda_s k_s), q = fma(lambda_t, k_t, p)
    (evaluated in fp64 and rounded once: both products are exact there), g = fl(g_in + q); loss =
    fl(fl(data + fl(lambda_s tv_s)) + fl(lambda_t tv_t)).  Returns (loss, tv_s, tv_t, g_out [H*W*T, O])."""
    dt = np.float64 if double else np.float32
    ks, kt = sign_patterns(y if pattern_from is None else pattern_from, H, W, T, O)
    tvs, tvt = tv_sums(y, H, W, T, O, double)
    g = np.asarray(g_in, dt).reshape(H * W * T, O)
    ls, lt = np.float32(lambda_s), np.float32(lambda_t)
    if double:
        g_out = g + (np.float64(ls) * ks + np.float64(lt) * kt)
        loss = np.float64(data) + np.float64(ls) * tvs + np.float64(lt) * tvt
    else:
        p = ls * ks.astype(np.float32)
        q = (np.float64(lt) * kt + p.astype(np.float64)).astype(np.float32)
        g_out = g + q
        loss = total_loss(data, ls, tvs, lt, tvt)
    return dt(loss), tvs, tvt, g_out


def total_loss(data, lambda_s, tv_s, lambda_t, tv_t):
    """The header's fp32 expression of loss_out[0] from the other three entries, every operation rounded once."""
    f = np.float32
    return f(f(f(data) + f(f(lambda_s) * f(tv_s))) + f(f(lambda_t) * f(tv_t)))
