"""The video compressive-sensing operator (modules/lin_inverse.py:42-95, per-pixel coded exposure) and its MSE restated
in numpy.  The yardstick of tests/test_video_cs_host.py (which pins it to torch ops + autograd in float64 and to the
coded video the reference itself makes, tests/golden/video_cs.npz) and of tests/test_gpu_video_cs.py (precedent:
tests/multi_sr_ref.py).

    C = ceil(T / nframes);  chunk c = frames [c nframes, min(T, (c + 1) nframes));  C' = C + dup_last
    est[c][p][o] = sum_{k in chunk c} m[p][k] y[p T + k][o]        (est[C] = est[C - 1] when dup_last: the reference
                                                                    appends its last chunk a second time)
    d = est - gt;   loss = sum d^2 / (C' NP O)
    dL/dy[p T + k][o] = m[p][k] 2 / (C' NP O) (d[c(k)][p][o] + (dup_last and c(k) == C - 1 ? d[C][p][o] : 0))
"""
import numpy as np


def nchunks(T, nframes):
    return (T + nframes - 1) // nframes


def coded_estimate(y, mask, T, nframes, dup_last=True, double=True):
    """y [NP*T, O] (any shape of that size; row p*T + k), mask [NP, T] -> est [C', NP, O].  double=False: fp32, every
    product rounded, the chunk summed frame by frame in order."""
    dt = np.float64 if double else np.float32
    m = np.asarray(mask, dt).reshape(-1, T)
    NP = m.shape[0]
    y = np.asarray(y, dt).reshape(NP, T, -1)
    C = nchunks(T, nframes)
    est = np.zeros((C + int(bool(dup_last)), NP, y.shape[2]), dt)
    for c in range(C):
        acc = np.zeros((NP, y.shape[2]), dt)
        for k in range(c * nframes, min(T, (c + 1) * nframes)):
            acc = acc + m[:, k, None] * y[:, k, :]
        est[c] = acc
    if dup_last:
        est[C] = est[C - 1]
    return est


def coded_loss_and_grad(y, mask, gt, T, nframes, dup_last=True, double=True):
    """y [NP*T, O], mask [NP, T], gt [C', NP, O] (any shapes of those sizes) -> (loss, g_y [NP*T, O], est [C', NP, O])."""
    dt = np.float64 if double else np.float32
    est = coded_estimate(y, mask, T, nframes, dup_last, double)
    Cp, NP, O = est.shape
    C = nchunks(T, nframes)
    d = est - np.asarray(gt, dt).reshape(est.shape)
    loss = np.sum(np.square(d), dtype=dt) / dt(d.size)
    dc = d[:C].copy()
    if dup_last:
        dc[C - 1] = dc[C - 1] + d[C]
    scale = dt(2.0) / dt(d.size)
    m = np.asarray(mask, dt).reshape(NP, T)
    chunk_of = np.arange(T) // nframes
    g = m[:, :, None] * (scale * dc[chunk_of].transpose(1, 0, 2))            # [NP, T, O]
    return dt(loss), g.reshape(NP * T, O), est


def coded_adjoint(g_coded, masks, T, nframes, dup_last=True):
    """Frame-major adjoint in fp64: g_coded [C', NP], masks [T, NP] -> g_video [T, NP]."""
    g = np.asarray(g_coded, np.float64).reshape(nchunks(T, nframes) + int(bool(dup_last)), -1)
    m = np.asarray(masks, np.float64).reshape(T, -1)
    C = nchunks(T, nframes)
    gc = g[:C].copy()
    if dup_last:
        gc[C - 1] = gc[C - 1] + g[C]
    return m * gc[np.arange(T) // nframes]


def make_mask(rng, NP, T):
    """Mask values 0, 0.5 and 1 in (NP, T) order, with pixel 0 closed in every frame."""
    m = rng.choice(np.array([0.0, 0.5, 1.0], np.float32), size=(NP, T))
    m[0] = 0.0
    return m.astype(np.float32)
