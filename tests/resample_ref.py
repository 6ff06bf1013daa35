"""A numpy fp64 restatement of the hierarchical resampler (wire_ray_resample in wire_amd/csrc/wire_render.hip, DESIGN
section 33): bin edges at the midpoints of the coarse samples, an unnormalised CDF of the clamped weights (np.cumsum),
the inverse at the stratified draws (np.searchsorted), a stable sort of (coarse, fine) for the merge, and the sampler's
recipe on the merged list.  Every output is rounded to fp32 once."""
import numpy as np

FLT_MAX = float(np.finfo(np.float32).max)


def _f64(a):
    return np.asarray(a, np.float32).astype(np.float64)


def mass(w, eps=1e-5):
    """p = min(max(w, 0), FLT_MAX) + eps with NaN counted as 0 -> (p [R, S], c [R, S+1] with c_0 = 0)."""
    w = _f64(w)
    with np.errstate(invalid="ignore"):
        p = np.minimum(np.where(w > 0, w, 0.0), FLT_MAX) + float(np.float32(eps))
    c = np.concatenate([np.zeros((w.shape[0], 1)), np.cumsum(p, axis=1)], axis=1)
    return p, c


def edges(near, far, ts_c):
    """e [R, S+1]: near, the midpoints of consecutive coarse samples, far."""
    tc = _f64(ts_c)
    R = tc.shape[0]
    nr = np.broadcast_to(_f64(near), (R,))[:, None]
    fr = np.broadcast_to(_f64(far), (R,))[:, None]
    return np.concatenate([nr, (tc[:, :-1] + tc[:, 1:]) / 2.0, fr], axis=1)


def fine_samples(near, far, ts_c, w, Nf, jitter=None, eps=1e-5):
    """The Nf inverse-CDF draws of every ray, unrounded -> (tf [R, Nf] fp64, bins [R, Nf] int)."""
    p, c = mass(w, eps)
    e = edges(near, far, ts_c)
    R, S = p.shape
    v = np.full((R, Nf), 0.5) if jitter is None else _f64(jitter)
    u = ((np.arange(Nf, dtype=np.float64)[None, :] + v) / float(Nf)) * c[:, -1:]
    s = np.stack([np.clip(np.searchsorted(c[r], u[r], side="right") - 1, 0, S - 1) for r in range(R)])
    c0, c1 = np.take_along_axis(c, s, 1), np.take_along_axis(c, s + 1, 1)
    e0, e1 = np.take_along_axis(e, s, 1), np.take_along_axis(e, s + 1, 1)
    den = c1 - c0
    with np.errstate(invalid="ignore", divide="ignore"):
        f = np.where(den > 0, (u - c0) / np.where(den > 0, den, 1.0), 0.0)   # an empty bin (eps lost beside 1e30): f = 0
        f = np.minimum(np.where(f > 0, f, 0.0), 1.0)
        t = np.minimum(e0 + f * (e1 - e0), e1)                               # f = 1 may round past the edge
    return t, s


def ray_resample(rays, near, far, ts_c, w, Nf, jitter=None, eps=1e-5):
    """rays [R, 6], near / far scalars or [R], ts_c and w [R, S] fp32, jitter None or [R, Nf] ->
    (coords [R*(S+Nf), 3], ts [R, S+Nf], deltas [R, S+Nf]) fp32."""
    rays = _f64(rays)
    tc = _f64(ts_c)
    R, S = tc.shape
    M = S + Nf
    o, d = rays[:, None, 0:3], rays[:, None, 3:6]
    nr = np.broadcast_to(_f64(near), (R,))[:, None]
    fr = np.broadcast_to(_f64(far), (R,))[:, None]
    tf, _ = fine_samples(near, far, ts_c, w, Nf, jitter, eps)
    both = np.concatenate([tc, tf], axis=1)
    t = np.take_along_axis(both, np.argsort(both, axis=1, kind="stable"), 1)  # coarse first on a tie
    with np.errstate(invalid="ignore", over="ignore"):
        hit = fr > nr
        t = np.where(hit, t, np.broadcast_to(nr, (R, M)))
        t1 = np.concatenate([t[:, 1:], np.broadcast_to(fr, (R, 1))], axis=1)
        norm = np.sqrt(d[..., 0] * d[..., 0] + d[..., 1] * d[..., 1] + d[..., 2] * d[..., 2])
        dl = np.where(hit, (t1 - t) * norm, 0.0)
        coords = o + t[..., None] * d
    return coords.reshape(R * M, 3).astype(np.float32), t.astype(np.float32), dl.astype(np.float32)


def kappa(w, near, far, eps=1e-5):
    """The fp64 conditioning of the inverse where the CDF is flattest, per ray [R]: 8 S 2^-52 (tot / eps) (far - near)."""
    p, c = mass(w, eps)
    R, S = p.shape
    span = np.abs(np.broadcast_to(_f64(far), (R,)) - np.broadcast_to(_f64(near), (R,)))
    return 8.0 * S * 2.0 ** -52 * (c[:, -1] / float(np.float32(eps))) * span


def ulp32(x):
    """The fp32 spacing at |x|."""
    return np.spacing(np.abs(np.asarray(x, np.float64)).astype(np.float32)).astype(np.float64)
