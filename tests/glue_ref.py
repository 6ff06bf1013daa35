"""Restatements of the training glue, the metrics, the layout helpers and the CT operator in numpy -- fp64, and fp32
where a comparison needs the reference arithmetic's own error as its yardstick.  Each follows the text of
include/wire_hip.h, not the kernels; tests/test_glue_host.py pins them on the CPU, tests/test_gpu_glue.py compares the
kernels with them."""
import numpy as np

from _util import ROOT  # noqa: F401  (puts the repository on sys.path)
from oracle import wire_oracle as wo

mse_loss_and_grad = wo.mse_loss_and_grad
avgpool_mse_loss_and_grad = wo.avgpool_mse_loss_and_grad
iou = wo.iou
psnr = wo.psnr
posenc = wo.posenc

# the angle set of the CT checks (degrees): the axes, a diagonal, a negative angle, more than one turn, a fraction
ANGLES = np.array([0.0, 90.0, 180.0, 45.0, -30.0, 270.0, 377.0, 12.5], np.float32)


def dtype_of(double):
    return np.float64 if double else np.float32


# ---------------------------------------------------------------------------------------------------------------------
# Adam
# ---------------------------------------------------------------------------------------------------------------------
def adam_steps(param, grads, m, v, first_step, lr, beta1=0.9, beta2=0.999, eps=1e-8, double=True):
    """len(grads) consecutive torch.optim.Adam steps (oracle.adam_step), the first one numbered ``first_step``
    (1-based), from the given moments.  The hyper-parameters are the fp32 values the C ABI receives, so fp64 measures
    the arithmetic and not their rounding; the bias corrections are taken in fp64 in both precisions, as the entry
    point does on the host.  Returns (param, exp_avg, exp_avg_sq) in the chosen precision."""
    dt = dtype_of(double)
    lr, beta1, beta2, eps = (float(np.float32(a)) for a in (lr, beta1, beta2, eps))
    p, m, v = (np.array(a, dt) for a in (param, m, v))
    for k, g in enumerate(grads):
        step = first_step + k
        if double:
            p, m, v = wo.adam_step(p, np.asarray(g, dt), m, v, step, lr, beta1, beta2, eps)
        else:
            f = np.float32
            g = np.asarray(g, f)
            m = f(beta1) * m + (f(1) - f(beta1)) * g
            v = f(beta2) * v + (f(1) - f(beta2)) * g * g
            bc1, bc2 = 1.0 - beta1 ** step, 1.0 - beta2 ** step
            denom = np.sqrt(v) * f(1.0 / np.sqrt(bc2)) + f(eps)
            p = p - f(lr / bc1) * (m / denom)
            assert p.dtype == m.dtype == v.dtype == np.float32
    return p, m, v


# ---------------------------------------------------------------------------------------------------------------------
# metrics
# ---------------------------------------------------------------------------------------------------------------------
def metric_sums(rec, gt):
    """mode 0 of wire_eval_metric in fp64: (sum (gt - rec)^2, max(gt)); the maximum is a value of gt, exact."""
    d = gt.astype(np.float64) - rec.astype(np.float64)
    return float(np.square(d).sum()), gt.max()


def iou_counts(rec, gt, thres):
    """mode 1: (|rec >= thres AND gt != 0|, |rec >= thres OR gt != 0|) as integers.  NaN >= thres is false and
    NaN != 0 is true, -0.0 != 0 is false: numpy's comparisons are the IEEE ones."""
    with np.errstate(invalid="ignore"):
        p, q = rec >= np.float32(thres), gt != 0
    return int(np.logical_and(p, q).sum()), int(np.logical_or(p, q).sum())


def sigmoid64(x):
    """1 / (1 + exp(-x)) in fp64, written so that neither tail overflows; NaN stays NaN."""
    x = np.asarray(x, np.float64)
    with np.errstate(over="ignore", invalid="ignore"):
        e = np.exp(-np.abs(x))
        return np.where(np.isnan(x), np.nan, np.where(x >= 0, 1.0 / (1.0 + e), e / (1.0 + e)))


# ---------------------------------------------------------------------------------------------------------------------
# CT operator: the formula of include/wire_hip.h, written directly
# ---------------------------------------------------------------------------------------------------------------------
# (H, W, A) of the GPU test; a shape with A < 8 takes the LAST A angles of ANGLES (a single angle is then 12.5
# degrees and not the identity)
RADON_SHAPES = [(9, 300, 8), (5, 256, 8), (5, 257, 8), (2, 2, 8), (1, 7, 3), (7, 1, 3), (37, 52, 1)]


def radon_case(H, W, A):
    """(image, sinogram-side vector, angles).  Both vectors are positive, so that <A x, y> is a sum of positive terms and
    a relative bound on it is a bound on the operator and not on how far a random sum happened to cancel."""
    rng = np.random.default_rng(H * 1000 + W * 10 + A)
    return (rng.random((H, W)).astype(np.float32), (0.25 + rng.random((A, W))).astype(np.float32),
            ANGLES[len(ANGLES) - A:].copy())


def _radon_taps(angles_deg, H, W, dtype):
    """The four taps of every sample: lists of (row index, column index, weight, valid) over [A][H][W]."""
    dt = np.dtype(dtype).type
    th = np.asarray(angles_deg, dt) * dt(np.pi / 180.0)
    c, s = np.cos(th)[:, None, None], np.sin(th)[:, None, None]
    cx, cy = dt(0.5) * dt(W - 1), dt(0.5) * dt(H - 1)
    xj = (np.arange(W, dtype=dt) - cx)[None, None, :]
    yi = (np.arange(H, dtype=dt) - cy)[None, :, None]
    x = c * xj - s * yi + cx
    y = s * xj + c * yi + cy
    assert x.dtype == np.dtype(dtype)
    xf, yf = np.floor(x), np.floor(y)
    x0, y0 = xf.astype(np.int64), yf.astype(np.int64)
    wx1, wy1 = x - xf, y - yf
    wx0, wy0 = dt(1) - wx1, dt(1) - wy1
    taps = []
    for dy, wy in ((0, wy0), (1, wy1)):
        for dx, wx in ((0, wx0), (1, wx1)):
            yy, xx = y0 + dy, x0 + dx
            ok = (yy >= 0) & (yy < H) & (xx >= 0) & (xx < W)           # zero padding: one pixel of border still counts
            taps.append((np.clip(yy, 0, H - 1), np.clip(xx, 0, W - 1), wy * wx, ok))
    return taps


def radon(img, angles_deg, dtype=np.float64):
    """sino[a][j] = sum_i bilinear(img, x = c xj - s yi + cx, y = s xj + c yi + cy), xj = j - cx, yi = i - cy,
    (cx, cy) = ((W-1)/2, (H-1)/2), c / s = cos / sin of the angle: img [H][W] -> [A][W], every operation in ``dtype``.
    Taps outside the image read zero.  No division by W - 1 or H - 1: a side of 1 is an ordinary case."""
    img = np.asarray(img, dtype)
    H, W = img.shape
    acc = np.zeros((len(angles_deg), H, W), dtype)
    for yy, xx, w, ok in _radon_taps(angles_deg, H, W, dtype):
        acc += np.where(ok, w * img[yy, xx], np.dtype(dtype).type(0))
    out = np.zeros((len(angles_deg), W), dtype)
    for i in range(H):                                                 # rows in order, as a thread of the kernel adds them
        out += acc[:, i, :]
    return out


def radon_adjoint(g_sino, angles_deg, H, W, dtype=np.float64):
    """The adjoint of radon: g_img[y][x] += g_sino[a][j] * weight for every tap.  [A][W] -> [H][W]."""
    g = np.asarray(g_sino, dtype)
    out = np.zeros((H, W), dtype)
    gb = np.broadcast_to(g[:, None, :], (g.shape[0], H, W))
    for yy, xx, w, ok in _radon_taps(angles_deg, H, W, dtype):
        np.add.at(out, (yy[ok], xx[ok]), (gb * w)[ok])
    return out


# ---------------------------------------------------------------------------------------------------------------------
# blocked-planar layout
# ---------------------------------------------------------------------------------------------------------------------
def blocked_width(K):
    return (2 * K + 63) // 64 * 64


def to_blocked(z):
    """complex [n][K] -> float32 [n][P], P = roundup(2 K, 64): group g of 32 features occupies columns [64 g, 64 g + 32)
    (real parts) and [64 g + 32, 64 g + 64) (imaginary parts); pads are +0.0."""
    z = np.asarray(z, np.complex64)
    n, K = z.shape
    out = np.zeros((n, blocked_width(K)), np.float32)
    for o in range(K):
        g, r = divmod(o, 32)
        out[:, 64 * g + r] = z[:, o].real
        out[:, 64 * g + 32 + r] = z[:, o].imag
    return out


def from_blocked(b, K):
    """float32 [n][P] -> complex64 [n][K]; the pad columns are not read."""
    b = np.asarray(b, np.float32)
    out = np.empty((b.shape[0], K), np.complex64)
    for o in range(K):
        g, r = divmod(o, 32)
        out[:, o] = b[:, 64 * g + r] + 1j * b[:, 64 * g + 32 + r]
    return out


# ---------------------------------------------------------------------------------------------------------------------
# trainable omega_0 / scale_0 of the two Gabor layers: closed forms
# ---------------------------------------------------------------------------------------------------------------------
def _layer_dtypes(W, double):
    c = np.complex128 if double else np.complex64
    return (c if np.iscomplexobj(W) else dtype_of(double)), c


def gabor_hparam_grads(x, W, b, g, omega0, scale0, double=True):
    """ComplexGaborLayer (modules/wire.py:88-93): out = exp(j w0 lin - s0^2 |lin|^2), lin = x W^T + b, so
    d out / d w0 = j lin out and d out / d s0 = -2 s0 |lin|^2 out; with c = conj(out) g (g = dL/dRe + j dL/dIm)
        dL/dw0 = sum (Re lin Im c - Im lin Re c),   dL/ds0 = -2 s0 sum |lin|^2 Re c.
    Returns ((dL/dw0, dL/ds0), (sum |terms| of each)): the second pair is the scale rounding errors are relative to."""
    lt, ct = _layer_dtypes(W, double)
    rt = dtype_of(double)
    lin = x.astype(lt) @ W.astype(lt).T + b.astype(lt)
    out = wo.gabor_act(lin, rt(omega0), rt(scale0)).astype(ct)
    c = np.conj(out) * g.astype(ct)
    tw = lin.real * c.imag - lin.imag * c.real
    ts = np.square(np.abs(lin)) * c.real
    k = rt(-2.0) * rt(scale0)
    assert tw.dtype == ts.dtype == rt
    return (tw.sum(dtype=rt), k * ts.sum(dtype=rt)), (float(np.abs(tw).sum()), float(abs(k) * np.abs(ts).sum()))


def gabor2d_hparam_grads(x, W, b, V, cc, g, omega0, scale0, double=True):
    """ComplexGaborLayer2D (modules/wire2d.py:56-67): out = exp(j w0 lin) exp(-s0^2 (|lin|^2 + |sy|^2)), sy = x V^T + c:
        dL/dw0 = sum (Re lin Im c - Im lin Re c),   dL/ds0 = -2 s0 sum (|lin|^2 + |sy|^2) Re c."""
    lt, ct = _layer_dtypes(W, double)
    rt = dtype_of(double)
    xx = x.astype(lt)
    lin = xx @ W.astype(lt).T + b.astype(lt)
    sy = xx @ V.astype(lt).T + cc.astype(lt)
    out = wo.gabor2d_act(lin, sy, rt(omega0), rt(scale0)).astype(ct)
    c = np.conj(out) * g.astype(ct)
    tw = lin.real * c.imag - lin.imag * c.real
    ts = (np.square(np.abs(lin)) + np.square(np.abs(sy))) * c.real
    k = rt(-2.0) * rt(scale0)
    assert tw.dtype == ts.dtype == rt
    return (tw.sum(dtype=rt), k * ts.sum(dtype=rt)), (float(np.abs(tw).sum()), float(abs(k) * np.abs(ts).sum()))
