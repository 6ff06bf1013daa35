"""The pointwise data terms of wire_point_loss_grad (include/wire_hip.h) in numpy, in a requested precision: fp64 is the
reference of a comparison, the fp32 twin its yardstick (err_ref of _util.within_ref).  The formulas are the header's,
not the kernel's code; tests/test_point_loss_host.py pins them against torch autograd and torch.nn's losses on the CPU,
tests/test_gpu_point_loss.py compares the kernel, functional.point_loss and the trainer's steps with them."""
import numpy as np

KINDS = ("mse", "l1", "huber", "logistic")


def rho(d_or_z, t, kind, delta, rdt):
    """(rho, rho') per element.  For "logistic" the first argument is the logit z and ``t`` the target; for the other
    kinds it is the residual d = y - t and ``t`` is not read."""
    x = d_or_z
    if kind == "mse":
        return x * x, rdt(2) * x
    if kind == "l1":
        return np.abs(x), np.sign(x) + rdt(0)                       # (+ 0: -0.0 of sign(-0.0) becomes +0.0)
    if kind == "huber":
        dl = rdt(delta)
        a = np.abs(x)
        return np.where(a <= dl, rdt(0.5) * x * x, dl * (a - rdt(0.5) * dl)), np.clip(x, -dl, dl)
    if kind == "logistic":
        e = np.exp(-np.abs(x))
        sig = np.where(x >= 0, rdt(1) / (rdt(1) + e), e / (rdt(1) + e))
        return np.maximum(x, rdt(0)) - t * x + np.log1p(e), sig - t
    raise ValueError(kind)


def loss_and_grad(y, t, w, kind, delta=1.0, shard=1.0, double=True):
    """loss = shard * sum_e w_e rho(d_e) / (n O) and g_y = shard * w_e rho'(d_e) / (n O) of y, t [n, O] and a weight
    w that is None, [n] or [n, O]; fp32 inputs are cast to the precision of the evaluation (``double``: fp64).  Returns
    (loss as a Python float, g_y [n, O] in that precision)."""
    rdt = np.float64 if double else np.float32
    y, t = np.asarray(y).astype(rdt), np.asarray(t).astype(rdt)
    n, O = y.shape
    v, g = rho(y if kind == "logistic" else y - t, t, kind, delta, rdt)
    v, g = v.astype(rdt), g.astype(rdt)
    if w is not None:
        w = np.asarray(w).astype(rdt)
        w = w[:, None] if w.ndim == 1 else w
        v, g = w * v, w * g
    scale = rdt(shard) * rdt(1.0 / (float(n) * float(O)))
    return float(scale * v.sum(dtype=rdt)), (scale * g).astype(rdt)
