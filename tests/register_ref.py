"""fp64 numpy restatement of wire_register.hip: the bilinear resampler and its coordinate gradient, the 29 sums of one
Gauss-Newton iteration, the projected Cholesky solve, and the whole of motion.register_stack_ecc as a "twin".

The restatement performs the kernels' operations in the kernels' order (numpy contracts nothing), so the resampler's
outputs are reproduced to the bit; the sums are added exactly (math.fsum), which is what the kernels' fixed tree is
measured against.  Also here: the synthetic image and stack the registration tests share."""
import functools
import math

import numpy as np

NSUM = 29
MODELS = {"translation": 0, "euclidean": 1, "affine": 2}


# ---- the shared sampler ----------------------------------------------------------------------------------------
def cell(x, n, inside):
    fl = np.floor(x)
    i0 = fl.astype(np.int64)
    f = x - fl
    if inside:
        last = i0 == n - 1
        i0 = np.where(last, n - 2, i0)
        f = np.where(last, 1.0, f)
    return i0, f


def bilinear(img, ch, x0, fx, y0, fy):
    """(v, dv/dx, dv/dy) in fp64 of channel ch of img [H, W, C] float32 on the cells (x0, fx), (y0, fy)."""
    H, W, _ = img.shape

    def tap(y, x):
        ok = (x >= 0) & (x < W) & (y >= 0) & (y < H)
        return np.where(ok, img[np.clip(y, 0, H - 1), np.clip(x, 0, W - 1), ch].astype(np.float64), 0.0)

    a, b, c, d = tap(y0, x0), tap(y0, x0 + 1), tap(y0 + 1, x0), tap(y0 + 1, x0 + 1)
    gx, gy = 1.0 - fx, 1.0 - fy
    top = gx * a + fx * b
    bot = gx * c + fx * d
    return gy * top + fy * bot, gy * (b - a) + fy * (d - c), bot - top


def _pixel(xy, H, W, normalized):
    x, y = xy[:, 0].astype(np.float64), xy[:, 1].astype(np.float64)
    if normalized:
        x = ((x + 1.0) * float(W) - 1.0) * 0.5
        y = ((y + 1.0) * float(H) - 1.0) * 0.5
    with np.errstate(invalid="ignore"):
        ok = (x >= -1.0) & (x < float(W)) & (y >= -1.0) & (y < float(H))
    return np.where(ok, x, 0.0), np.where(ok, y, 0.0), ok


def remap(img, xy, normalized=False):
    """wire_remap_bilinear_fwd: img [H, W, C] float32, xy [n, 2] float32 -> [n, C] float32."""
    H, W, C = img.shape
    x, y, ok = _pixel(xy, H, W, normalized)
    x0, fx = cell(x, W, False)
    y0, fy = cell(y, H, False)
    out = np.zeros((xy.shape[0], C), dtype=np.float32)
    for c in range(C):
        out[:, c] = np.where(ok, bilinear(img, c, x0, fx, y0, fy)[0].astype(np.float32), np.float32(0))
    return out


def remap_bwd_xy(img, xy, g_out, normalized=False, dtype=np.float32):
    """wire_remap_bilinear_bwd_xy: [n, 2] of ``dtype`` (float32: the kernel's bits; float64: before the rounding)."""
    H, W, C = img.shape
    x, y, ok = _pixel(xy, H, W, normalized)
    x0, fx = cell(x, W, False)
    y0, fy = cell(y, H, False)
    sx, sy = np.zeros(xy.shape[0]), np.zeros(xy.shape[0])
    for c in range(C):
        _, dx, dy = bilinear(img, c, x0, fx, y0, fy)
        gc = g_out[:, c].astype(np.float64)
        sx = sx + gc * dx
        sy = sy + gc * dy
    if normalized:
        sx = sx * (float(W) * 0.5)
        sy = sy * (float(H) * 0.5)
    g = np.stack((np.where(ok, sx, 0.0), np.where(ok, sy, 0.0)), axis=1)
    return g.astype(dtype)


def remap_bwd_terms(img, xy, g_out, normalized=False):
    """sum_c |g_c d_c| per row and axis [n, 2] (scaled like the gradient): the C-term sum's condition."""
    H, W, C = img.shape
    x, y, ok = _pixel(xy, H, W, normalized)
    x0, fx = cell(x, W, False)
    y0, fy = cell(y, H, False)
    t = np.zeros((xy.shape[0], 2))
    for c in range(C):
        _, dx, dy = bilinear(img, c, x0, fx, y0, fy)
        gc = np.abs(g_out[:, c].astype(np.float64))
        t[:, 0] += gc * np.abs(dx)
        t[:, 1] += gc * np.abs(dy)
    if normalized:
        t *= np.array([W * 0.5, H * 0.5])
    return t * ok[:, None]


# ---- one Gauss-Newton iteration ----------------------------------------------------------------------------------
def gn_terms(ref, frame, weight, M):
    """The 29 per-pixel terms of one (frame, candidate), [n_counted, 29] fp64, in the kernel's operations."""
    H, W = ref.shape
    Y, X = np.mgrid[:H, :W]
    xj, yi = X.reshape(-1).astype(np.float64), Y.reshape(-1).astype(np.float64)
    M = np.asarray(M, dtype=np.float64)
    u = M[0, 0] * xj + M[0, 1] * yi + M[0, 2]
    v = M[1, 0] * xj + M[1, 1] * yi + M[1, 2]
    f = frame.reshape(-1)
    w = np.ones(H * W) if weight is None else weight.reshape(-1).astype(np.float64)
    with np.errstate(invalid="ignore"):
        ok = (u >= 0.0) & (u <= W - 1.0) & (v >= 0.0) & (v <= H - 1.0) & (w != 0.0) & (f != 0)
    xj, yi, u, v, f, w = (a[ok] for a in (xj, yi, u, v, f, w))
    x0, fx = cell(u, W, True)
    y0, fy = cell(v, H, True)
    val, dx, dy = bilinear(ref[:, :, None], 0, x0, fx, y0, fy)
    res = val - f.astype(np.float64)
    J = [dx * xj, dx * yi, dx, dy * xj, dy * yi, dy]
    T = np.zeros((u.shape[0], NSUM))
    t = 0
    for a in range(6):
        wa = w * J[a]
        for b in range(a, 6):
            T[:, t] = wa * J[b]
            t += 1
        T[:, 21 + a] = wa * res
    T[:, 27] = (w * res) * res
    T[:, 28] = w
    return T


def gn_sums(ref, frames, weight, mats, exact=True):
    """S and sum |terms|, both [B, K, 29]; exact=True adds with math.fsum (one rounding)."""
    B, K = mats.shape[:2]
    S, A = np.zeros((B, K, NSUM)), np.zeros((B, K, NSUM))
    for b in range(B):
        for k in range(K):
            T = gn_terms(ref, frames[b], None if weight is None else weight[b], mats[b, k])
            if exact:
                S[b, k] = [math.fsum(T[:, t]) for t in range(NSUM)]
            else:
                S[b, k] = T.sum(axis=0)
            A[b, k] = np.abs(T).sum(axis=0)
    return S, A


def gn_solve(S, M, H, W, model, damping=0.0, min_cover=0.0):
    """reg_solve_kernel's thread 0: (new matrix, stats[4]) from the 29 sums and the input matrix."""
    M = np.asarray(M, dtype=np.float64)
    wsum = S[28]
    mean = S[27] / wsum if wsum > 0 else 0.0
    cover = wsum / (float(H) * float(W))
    bad = (M.copy(), np.array([mean, cover, 0.0, 0.0]))
    if not (wsum > 0 and np.isfinite(mean) and np.isfinite(cover) and cover >= min_cover):
        return bad
    Hm = np.zeros((6, 6))
    t = 0
    for a in range(6):
        for b in range(a, 6):
            Hm[a, b] = Hm[b, a] = S[t]
            t += 1
    th = math.atan2(M[1, 0], M[0, 0])
    cs, sn = math.cos(th), math.sin(th)
    if model == 0:
        P = np.zeros((6, 2))
        P[2, 0] = P[5, 1] = 1.0
    elif model == 1:
        P = np.zeros((6, 3))
        P[:, 0] = [-sn, -cs, 0.0, cs, -sn, 0.0]
        P[2, 1] = P[5, 2] = 1.0
    else:
        P = np.eye(6)
    A = P.T @ (Hm @ P)
    g = P.T @ S[21:27]
    A[np.diag_indices_from(A)] += damping * np.diag(A)
    if not np.all(np.isfinite(A)):
        return bad
    try:
        Lc = np.linalg.cholesky(A)
    except np.linalg.LinAlgError:
        return bad
    delta = np.linalg.solve(Lc.T, np.linalg.solve(Lc, -g))
    out = M.copy()
    if model == 0:
        out[0, 2] += delta[0]
        out[1, 2] += delta[1]
    elif model == 1:
        c, s = math.cos(th + delta[0]), math.sin(th + delta[0])
        out = np.array([[c, -s, M[0, 2] + delta[1]], [s, c, M[1, 2] + delta[2]]])
    else:
        out = M + delta.reshape(2, 3)
    norm = float(np.sqrt((delta * delta).sum()))
    if not (np.all(np.isfinite(out)) and np.isfinite(norm)):
        return bad
    return out, np.array([mean, cover, norm, 1.0])


def gn_step(ref, frames, weight, mats, model, damping=0.0, min_cover=0.0, exact=False):
    """wire_register_gn_step: (new mats [B, K, 2, 3], stats [B, K, 4], S [B, K, 29])."""
    H, W = ref.shape
    S, _ = gn_sums(ref, frames, weight, mats, exact=exact)
    out, stats = np.array(mats, dtype=np.float64), np.zeros(mats.shape[:2] + (4,))
    for b in range(mats.shape[0]):
        for k in range(mats.shape[1]):
            out[b, k], stats[b, k] = gn_solve(S[b, k], mats[b, k], H, W, model, damping, min_cover)
    return out, stats, S


# ---- the twin of motion.register_stack_ecc -------------------------------------------------------------------------
def rescale_mats(mats, s):
    out = np.array(mats, dtype=np.float64)
    h = (s - 1) / 2
    out[..., 2] = s * mats[..., 2] + h - (mats[..., 0] + mats[..., 1]) * h
    return out


def pool2(x):
    """[B, H, W] float32 -> 2 x 2 means, an odd last row / column dropped."""
    B, H, W = x.shape
    x = x[:, :H // 2 * 2, :W // 2 * 2].astype(np.float32)
    return ((x[:, 0::2, 0::2] + x[:, 0::2, 1::2] + x[:, 1::2, 0::2] + x[:, 1::2, 1::2]) * np.float32(0.25)).astype(np.float32)


def seed_mats(seeds, H, W):
    cy, cx = (H - 1) / 2, (W - 1) / 2
    return np.stack([np.array([[np.cos(a), -np.sin(a), cx - np.cos(a) * cx + np.sin(a) * cy],
                               [np.sin(a), np.cos(a), cy - np.sin(a) * cx - np.cos(a) * cy]]) for a in seeds])


def register_stack_twin(imstack, full_res, method="euclidean", levels=3, iters=30, seeds=(0.0,), weight=None,
                        damping=1e-6, min_cover=0.25):
    """motion.register_stack_ecc in numpy: (mask, ecc_mats at full_res, alignment_err)."""
    model = MODELS[method] if isinstance(method, str) else int(method)
    x = np.asarray(imstack, dtype=np.float32)
    if x.ndim == 4:
        x = x.mean(axis=1, dtype=np.float32)
    nimg, H, W = x.shape
    Hr, _ = full_res
    ecc = np.zeros((nimg, 2, 3))
    ecc[:, 0, 0] = ecc[:, 1, 1] = 1
    mask, err = np.zeros(nimg), np.zeros(nimg)
    mask[0] = 1
    if nimg == 1:
        return mask, ecc, err
    B = nimg - 1
    wt = None if weight is None else np.asarray(weight, dtype=np.float32)[1:]
    pyr = [(x[0], x[1:], wt)]
    for _ in range(levels - 1):
        r, f, w = pyr[-1]
        pyr.append((pool2(r[None])[0], pool2(f), None if w is None else pool2(w)))
    r, f, w = pyr[-1]
    mats = np.broadcast_to(seed_mats(seeds, *r.shape), (B, len(seeds), 2, 3)).copy()
    for _ in range(iters):
        mats, _, _ = gn_step(r, f, w, mats, model, damping, min_cover)
    _, st, _ = gn_step(r, f, w, mats, model, damping, min_cover)
    cost = np.where(st[..., 3] > 0, st[..., 0], np.inf)
    best = cost.argmin(axis=1)
    found = np.isfinite(cost[np.arange(B), best])
    mats = mats[np.arange(B), best][:, None]
    for r, f, w in pyr[-2::-1]:
        mats = rescale_mats(mats, 2.0)
        for _ in range(iters):
            mats, _, _ = gn_step(r, f, w, mats, model, damping, min_cover)
    r, f, w = pyr[0]
    _, st, _ = gn_step(r, f, w, mats, model, damping, min_cover)
    found = found & (st[:, 0, 3] > 0)
    for b in range(B):
        M = mats[b, 0] if found[b] else ecc[0]
        T = gn_terms(r, f[b], None if w is None else w[b], M)
        # |residual| from the terms: T[:, 27] = w res^2, T[:, 28] = w
        res = np.sqrt(T[:, 27] / T[:, 28])
        err[b + 1] = res.mean() if res.size else 0.0
        ecc[b + 1] = rescale_mats(M, Hr / H)
    mask[1:] = found
    return mask, ecc, err


# ---- the shared synthetic scene ------------------------------------------------------------------------------------
def synth_image_fn(H, W, seed=0, sigma=(0.04, 0.15)):
    """A smooth image on the pixel plane as a function (x, y) -> value, evaluable anywhere: a seeded sum of 40 Gaussians
    plus two sinusoids, offset so that no value is 0."""
    rng = np.random.default_rng(seed)
    cx, cy = rng.uniform(-0.1 * W, 1.1 * W, 40), rng.uniform(-0.1 * H, 1.1 * H, 40)
    sg = rng.uniform(sigma[0], sigma[1], 40) * min(H, W)
    am = rng.uniform(0.2, 1.0, 40)

    def fn(x, y):
        v = np.full(np.broadcast(x, y).shape, 0.5)
        for k in range(40):
            v = v + am[k] * np.exp(-((x - cx[k]) ** 2 + (y - cy[k]) ** 2) / (2 * sg[k] ** 2))
        v = v + 0.15 * np.sin(2 * np.pi * (3 * x / W + 2 * y / H)) + 0.1 * np.sin(2 * np.pi * (5 * y / H - x / W))
        return v / 4.0
    return fn


def euclid(theta, shift):
    c, s = np.cos(theta), np.sin(theta)
    return np.array([[c, -s, shift[0]], [s, c, shift[1]]])


def synth_stack(H, W, mats, pool, seed=0, sigma=(0.04, 0.15)):
    """frame_f = the synthetic H x W image at mats[f] (j, i, 1), pooled by ``pool``: (nimg, H/pool, W/pool) float32."""
    fn = synth_image_fn(H, W, seed, sigma)
    Y, X = np.mgrid[:H, :W].astype(np.float64)
    out = []
    for M in mats:
        v = fn(M[0, 0] * X + M[0, 1] * Y + M[0, 2], M[1, 0] * X + M[1, 1] * Y + M[1, 2])
        out.append(v.reshape(H // pool, pool, W // pool, pool).mean(axis=(1, 3)))
    return np.stack(out).astype(np.float32)


def host_motions(n=7, seed=5, shift=6, angle=np.pi / 30):
    """The host test's motions: frame 0 the identity, then n - 1 Euclidean motions, shifts from randint(-shift, shift),
    |angle| <= ``angle``."""
    rs = np.random.RandomState(seed)
    shifts = rs.randint(-shift, shift, size=[n, 2])
    thetas = (2 * rs.rand(n) - 1) * angle
    shifts[0], thetas[0] = 0, 0
    return np.stack([euclid(t, s) for t, s in zip(thetas, shifts)])


def corner_error(A, B, H, W):
    """Worst displacement, over the four corners of an H x W image, between two stacks of 2 x 3 matrices: [nimg]."""
    c = np.array([[0, 0, 1], [W - 1, 0, 1], [0, H - 1, 1], [W - 1, H - 1, 1]], dtype=np.float64)
    d = np.einsum("fac,pc->fpa", np.asarray(A) - np.asarray(B), c)
    return np.sqrt((d ** 2).sum(axis=-1)).max(axis=1)


# ---- the two registration cases the host and GPU tests share (computed once) -----------------------------------------
HOST_SHAPE = (96, 128)           # pooled by 2: frames of 48 x 64
MULTI_SHAPE = (192, 256)         # pooled by 4: frames of 48 x 64
MULTI_SEEDS = tuple(np.deg2rad(np.arange(-18, 19, 6)).tolist())
MULTI_SIGMA = (0.02, 0.06)       # finer blobs than the host case: a narrower basin


@functools.lru_cache(maxsize=None)
def host_stack():
    return synth_stack(*HOST_SHAPE, host_motions(), 2)


@functools.lru_cache(maxsize=None)
def host_case(method):
    """(mask, ecc_mats, alignment_err) of the twin on host_stack(): 3 levels, 30 iterations, one start."""
    return register_stack_twin(host_stack(), HOST_SHAPE, method, 3, 30)


def multi_motions():
    return host_motions(7, 11, 20, np.pi / 12)


@functools.lru_cache(maxsize=None)
def multi_stack():
    return synth_stack(*MULTI_SHAPE, multi_motions(), 4, sigma=MULTI_SIGMA)


@functools.lru_cache(maxsize=None)
def multi_start_case():
    """(true mats, mask, ecc_mats, corner error with the seeds, corner error from the identity alone) of the twin on the
    multi-start stack: shifts up to 20 px, |angle| <= pi / 12, 3 levels, 30 iterations."""
    mats = multi_motions()
    mask, ecc, _ = register_stack_twin(multi_stack(), MULTI_SHAPE, "euclidean", 3, 30, MULTI_SEEDS)
    _, ecc1, _ = register_stack_twin(multi_stack(), MULTI_SHAPE, "euclidean", 3, 30, (0.0,))
    return mats, mask, ecc, corner_error(ecc, mats, *MULTI_SHAPE), corner_error(ecc1, mats, *MULTI_SHAPE)
