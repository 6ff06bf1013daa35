"""CPU-only checks behind tests/test_gpu_glue.py: the restatements of tests/glue_ref.py against the oracle (the direct
Radon form and its adjoint against oracle/torch_ref.radon and fp64 autograd, the layout round trip, the fp32 yardsticks
being non-zero), and the argument refusals of the glue, metric, CT, layout and hyper-parameter-gradient entry points as
include/wire_hip.h states them -- before any HIP call, so with a NULL stream and host buffers."""
import ctypes as C

import numpy as np
import pytest
import torch

from _util import ROOT, relmax  # noqa: F401  (puts the repository on sys.path)
import glue_ref as ref
from oracle import torch_ref, wire_oracle as wo

RADON_HOST_SHAPES = [(37, 52), (9, 300), (5, 257)]


@pytest.mark.parametrize("H,W", RADON_HOST_SHAPES)
def test_direct_radon_equals_the_oracle(H, W):
    """The header's formula written directly == oracle/torch_ref.radon (kornia's rotate restated with ATen ops) in fp64
    to 1e-12 relative, and its adjoint == fp64 autograd of the oracle, on the eight angles of the GPU test."""
    img, g, _ = ref.radon_case(H, W, 8)
    x = torch.tensor(img, dtype=torch.float64, requires_grad=True)
    s = torch_ref.radon(x, torch.tensor(ref.ANGLES))
    s.backward(torch.tensor(g, dtype=torch.float64))
    mine = ref.radon(img, ref.ANGLES, np.float64)
    assert mine.shape == (8, W) and mine.dtype == np.float64
    assert relmax(mine, s.detach().numpy()) <= 1e-12
    adj = ref.radon_adjoint(g, ref.ANGLES, H, W, np.float64)
    assert relmax(adj, x.grad.numpy()) <= 1e-12
    # <A x, y> == <x, A^T y>
    lhs, rhs = float((mine * g).sum()), float((adj * img).sum())
    assert abs(lhs - rhs) <= 1e-12 * abs(lhs)


def test_direct_radon_known_answers():
    """Angle 0 is the column sums; 180 degrees reverses them; a side of 1 is an ordinary case of the direct form (the
    oracle divides by W - 1 and H - 1 there)."""
    img = np.random.default_rng(1).random((6, 5))
    z = ref.radon(img, np.array([0.0, 180.0], np.float32))
    assert np.abs(z[0] - img.sum(0)).max() <= 1e-14 and np.abs(z[1] - img.sum(0)[::-1]).max() <= 1e-12
    row = np.array([[1.0, 2.0, 4.0]])
    assert np.array_equal(ref.radon(row, np.array([0.0], np.float32)), row)
    assert np.array_equal(ref.radon(row.T, np.array([0.0], np.float32)), [[7.0]])
    # a single pixel: centre (0, 0), every angle samples it at (0, 0) exactly
    assert np.array_equal(ref.radon(np.array([[3.0]]), ref.ANGLES), np.full((8, 1), 3.0))
    with pytest.raises(ZeroDivisionError):
        torch_ref.radon(torch.ones(1, 3, dtype=torch.float64), torch.zeros(1))


@pytest.mark.parametrize("H,W,A", ref.RADON_SHAPES)
def test_radon_yardstick_is_not_zero(H, W, A):
    """The fp32 restatement differs from the fp64 one at every shape of the GPU test, forward and adjoint, so that
    within_ref's bound there is 2 x a real error + 1e-6 and not the floor alone.  Measured here (max |d| / max |ref|),
    forward / adjoint: (9,300,8) 1.7e-06 / 3.1e-06, (5,256,8) 2.4e-06 / 3.1e-06, (5,257,8) 2.3e-06 / 2.0e-06,
    (2,2,8) 1.1e-07 / 9.4e-08, (1,7,3) 2.8e-07 / 1.0e-07, (7,1,3) 4.1e-07 / 1.4e-07, (37,52,1) 2.9e-07 / 3.9e-06 (the
    larger figures are the fp32 rounding of the angle and of the sample positions, times the lever of the far columns)."""
    img, g, ang = ref.radon_case(H, W, A)
    assert len(ang) == A
    ef = relmax(ref.radon(img, ang, np.float32), ref.radon(img, ang, np.float64))
    eb = relmax(ref.radon_adjoint(g, ang, H, W, np.float32), ref.radon_adjoint(g, ang, H, W, np.float64))
    print(f"radon yardstick {(H, W, A)}: fwd {ef:.2e}  adjoint {eb:.2e}")
    assert 0 < ef < 1e-5 and 0 < eb < 1e-5


@pytest.mark.parametrize("K", [1, 31, 32, 33, 64, 90])
def test_layout_restatement_round_trips(K):
    """to_blocked puts feature o of group g = o // 32 at columns 64 g + o % 32 (real) and 64 g + 32 + o % 32 (imaginary),
    pads are +0.0, and from_blocked is its inverse bit for bit."""
    rng = np.random.default_rng(K)
    z = (rng.standard_normal((5, K)) + 1j * rng.standard_normal((5, K))).astype(np.complex64)
    b = ref.to_blocked(z)
    P = ref.blocked_width(K)
    assert b.shape == (5, P) and b.dtype == np.float32 and P % 64 == 0 and 2 * K <= P < 2 * K + 64
    o = K - 1
    assert b[3, 64 * (o // 32) + o % 32] == z[3, o].real and b[3, 64 * (o // 32) + 32 + o % 32] == z[3, o].imag
    assert np.count_nonzero(b) == 2 * 5 * K and not np.signbit(b[b == 0]).any()
    assert ref.from_blocked(b, K).tobytes() == z.tobytes()
    noisy = b.copy()
    noisy[b == 0] = np.nan                                          # the pads are not read on the way back
    assert ref.from_blocked(noisy, K).tobytes() == z.tobytes()


def test_small_restatements():
    """sigmoid64 at its tails, the IoU counts on the IEEE edge values, Adam's fp32 twin close to fp64 and returning the
    moments, the closed forms of the hyper-parameter gradients against fp64 autograd."""
    s = ref.sigmoid64(np.array([0.0, np.inf, -np.inf, 800.0, -800.0, np.nan, -87.4]))
    assert s[0] == 0.5 and s[1] == 1.0 and s[2] == 0.0 and s[3] == 1.0 and s[4] == 0.0 and np.isnan(s[5])
    assert 0 < s[6] < 2.0 ** -126
    rec = np.array([0.5, 0.5, 0.4, np.nan, 0.7, 0.7, 0.2], np.float32)
    gt = np.array([1.0, -0.0, -2.0, 1.0, np.nan, 0.0, 0.0], np.float32)
    assert ref.iou_counts(rec, gt, 0.5) == (2, 6)
    assert ref.iou_counts(rec, gt, 0.5) == (int(np.logical_and(rec >= 0.5, gt != 0).sum()),
                                            int(np.logical_or(rec >= 0.5, gt != 0).sum()))
    rng = np.random.default_rng(0)
    # the counts and sums give the oracle's IoU and PSNR; the oracle's posenc is the eager reference's
    pr, g = rng.random(400).astype(np.float32), (rng.random(400) < 0.3).astype(np.float32)
    inter, union = ref.iou_counts(pr, g, 0.5)
    assert 0 < inter < union and inter / union == ref.iou(pr, g, 0.5)
    sq, mx = ref.metric_sums(pr, g)
    assert abs(10 * np.log10(mx / (sq / 400)) - ref.psnr(g.astype(np.float64), pr.astype(np.float64))) <= 1e-12
    c = rng.uniform(-1, 1, (5, 3))
    assert relmax(ref.posenc(c, 10), torch_ref.posenc(torch.tensor(c), 10).numpy()) <= 1e-12
    p, m, v = rng.standard_normal(50), 0.01 * rng.standard_normal(50), 1e-4 * rng.random(50)
    gs = [rng.standard_normal(50) for _ in range(3)]
    a64 = ref.adam_steps(p, gs, m, v, 1000, 5e-3, double=True)
    a32 = ref.adam_steps(p, gs, m, v, 1000, 5e-3, double=False)
    for x64, x32 in zip(a64, a32):
        assert x32.dtype == np.float32 and x64.dtype == np.float64 and 0 < relmax(x32, x64) < 1e-6
    q, mm, vv = wo.adam_step(p, gs[0], m, v, 1000, float(np.float32(5e-3)), float(np.float32(0.9)),
                             float(np.float32(0.999)), float(np.float32(1e-8)))
    one = ref.adam_steps(p, gs[:1], m, v, 1000, 5e-3)
    assert np.array_equal(one[0], q) and np.array_equal(one[1], mm) and np.array_equal(one[2], vv)
    # closed forms against autograd
    n, fin, out, w0, s0 = 7, 3, 5, 9.0, 4.0
    for first in (True, False):
        cplx = lambda *sh: rng.standard_normal(sh) + 1j * rng.standard_normal(sh)
        x = rng.uniform(-1, 1, (n, fin)) if first else 0.5 * cplx(n, fin)
        Wt, b = (0.3 * rng.standard_normal((out, fin)), 0.1 * rng.standard_normal(out)) if first else \
            (0.3 * cplx(out, fin), 0.1 * cplx(out))
        V, cc = (0.3 * rng.standard_normal((out, fin)), 0.1 * rng.standard_normal(out)) if first else \
            (0.3 * cplx(out, fin), 0.1 * cplx(out))
        g = cplx(n, out)
        om = torch.tensor(w0, dtype=torch.float64, requires_grad=True)
        sc = torch.tensor(s0, dtype=torch.float64, requires_grad=True)
        T = lambda a: torch.tensor(a)
        lin = T(x).to(T(Wt).dtype) @ T(Wt).T + T(b)
        o1 = torch.exp(1j * om * lin - (sc * lin).abs().square())
        (o1.real * T(g.real) + o1.imag * T(g.imag)).sum().backward()
        (gw, gs_), (aw, as_) = ref.gabor_hparam_grads(x, Wt, b, g, w0, s0)
        assert abs(gw - om.grad.item()) <= 1e-12 * aw and abs(gs_ - sc.grad.item()) <= 1e-12 * as_
        om.grad = sc.grad = None
        sy = T(x).to(T(V).dtype) @ T(V).T + T(cc)
        o2 = torch.exp(1j * om * lin) * torch.exp(-sc * sc * (lin.abs().square() + sy.abs().square()))
        (o2.real * T(g.real) + o2.imag * T(g.imag)).sum().backward()
        (gw, gs_), (aw, as_) = ref.gabor2d_hparam_grads(x, Wt, b, V, cc, g, w0, s0)
        assert abs(gw - om.grad.item()) <= 1e-12 * aw and abs(gs_ - sc.grad.item()) <= 1e-12 * as_
        (fw, fs), _ = ref.gabor2d_hparam_grads(x, Wt, b, V, cc, g, w0, s0, double=False)
        assert fw.dtype == np.float32 and abs(fw - gw) <= 1e-5 * aw and abs(fs - gs_) <= 1e-5 * as_


# ---------------------------------------------------------------------------------------------------------------------
# argument refusals
# ---------------------------------------------------------------------------------------------------------------------
def _lib():
    from wire_amd import _lib
    return _lib.lib()


_BUF = (C.c_float * 8192)()
P = (C.addressof(_BUF) + 63) & ~63                   # a 64-byte aligned host address: never dereferenced by a refusal


def _refused(L, fn, name, cases, call, rc=-1):
    for kw in cases:
        assert call(**kw) == rc, (name, kw)
        if name is not None:
            assert name.encode() in L.wire_last_error(), (name, kw, L.wire_last_error())


def test_training_glue_refusals():
    """wire_coords_from_index, wire_mse_grad, wire_avgpool_mse_grad, wire_adam_step_flat: every size below its minimum,
    scale > min(H, W), step < 1 and each NULL pointer that is not optional return WIRE_ERR_ARG and name the entry point."""
    L = _lib()

    def coords(idx=None, first=0, n=4, tx=P, W=3, ty=P, H=2, tz=None, T=1, out=P):
        return L.wire_coords_from_index(None, idx, first, n, tx, W, ty, H, tz, T, out)
    _refused(L, coords, "wire_coords_from_index",
             [dict(n=-1), dict(W=0), dict(H=0), dict(W=-2), dict(H=-1), dict(tz=P, T=0), dict(tz=P, T=-1), dict(tx=None),
              dict(ty=None), dict(out=None)], coords)

    def mse(y=P, t=P, idx=None, first=0, n=4, O=3, w=1.0, g=P, loss=P, rec=None, part=P):
        return L.wire_mse_grad(None, y, t, idx, first, n, O, w, g, loss, rec, part)
    _refused(L, mse, "wire_mse_grad", [dict(n=-1), dict(O=0), dict(O=-1), dict(y=None), dict(t=None), dict(g=None),
                                       dict(loss=None), dict(part=None)], mse)

    def pool(y=P, H=6, W=8, O=3, scale=2, gt=P, g=P, rec=None, loss=P, part=P):
        return L.wire_avgpool_mse_grad(None, y, H, W, O, scale, gt, g, rec, loss, part)
    _refused(L, pool, "wire_avgpool_mse_grad",
             [dict(H=0), dict(W=0), dict(O=0), dict(scale=0), dict(H=-1), dict(W=-1), dict(O=-1), dict(scale=-2),
              dict(scale=7), dict(scale=9), dict(H=8, W=6, scale=7), dict(y=None), dict(gt=None), dict(g=None),
              dict(loss=None), dict(part=None)], pool)

    def adam(p=P, g=P, m=P, v=P, count=8, lr=5e-3, b1=0.9, b2=0.999, eps=1e-8, step=1):
        return L.wire_adam_step_flat(None, p, g, m, v, count, lr, b1, b2, eps, step)
    _refused(L, adam, "wire_adam_step_flat", [dict(count=-1), dict(step=0), dict(step=-5), dict(p=None), dict(g=None),
                                              dict(m=None), dict(v=None)], adam)


def test_metric_and_tracking_refusals():
    """wire_eval_metric (mode outside {0, 1}, count < 1, NULL), wire_track_best (NULL scalars, count < 0, NULL or
    misaligned src / dst with count > 0) and wire_sigmoid_inplace (count < 0, NULL with count > 0)."""
    L = _lib()

    def metric(mode=0, rec=P, gt=P, count=16, thres=0.5, out=P, part=P):
        return L.wire_eval_metric(None, mode, rec, gt, count, thres, out, part)
    _refused(L, metric, "wire_eval_metric", [dict(mode=2), dict(mode=-1), dict(count=0), dict(count=-3), dict(rec=None),
                                             dict(gt=None), dict(out=None), dict(part=None)], metric)

    def best(metric=P, best_=P, force=0, src=P, dst=P + 64, count=8, upd=None):
        return L.wire_track_best(None, metric, best_, force, src, dst, count, upd)
    _refused(L, best, "wire_track_best", [dict(metric=None), dict(best_=None), dict(count=-1), dict(src=None),
                                          dict(dst=None)], best)
    # the copy moves 16 bytes per thread: both pointers must be 16-byte aligned when there is something to copy
    for kw in (dict(src=P + 4), dict(src=P + 8), dict(src=P + 12), dict(dst=P + 68), dict(dst=P + 72), dict(dst=P + 76),
               dict(src=P + 4, dst=P + 68), dict(src=P + 4, count=1), dict(dst=P + 68, count=3)):
        assert best(**kw) == -1, kw
        assert b"16-byte aligned" in L.wire_last_error()

    def sig(x=P, count=4):
        return L.wire_sigmoid_inplace(None, x, count)
    _refused(L, sig, "wire_sigmoid_inplace", [dict(count=-1), dict(x=None)], sig)


def test_ct_layout_and_encoding_refusals():
    """wire_radon_fwd / _bwd (a size < 1, NULL), wire_c64_to_blocked / wire_blocked_to_c64 (n < 0, K < 1, NULL; their
    message does not name them), wire_posenc_bwd (n < 0, D outside 1..4, F outside 0..30, NULL with n > 0)."""
    L = _lib()
    for fn, name in ((L.wire_radon_fwd, "wire_radon_fwd"), (L.wire_radon_bwd, "wire_radon_bwd")):
        def radon(a=P, ang=P, H=4, W=5, A=3, b=P, fn=fn):
            return fn(None, a, ang, H, W, A, b)
        _refused(L, radon, name, [dict(H=0), dict(W=0), dict(A=0), dict(H=-1), dict(W=-1), dict(A=-1), dict(a=None),
                                  dict(ang=None), dict(b=None)], radon)
    for fn in (L.wire_c64_to_blocked, L.wire_blocked_to_c64):
        def conv(src=P, n=2, K=5, dst=P, fn=fn):
            return fn(None, src, n, K, dst)
        _refused(L, conv, None, [dict(n=-1), dict(K=0), dict(K=-1), dict(src=None), dict(dst=None)], conv)
    assert [L.wire_blocked_width(K) for K in (1, 31, 32, 33, 64, 90)] == [64, 64, 64, 128, 128, 192]
    assert all(L.wire_blocked_width(K) == ref.blocked_width(K) for K in range(1, 300))

    def pe(c=P, n=4, D=3, F=10, g=P, out=P):
        return L.wire_posenc_bwd(None, c, n, D, F, g, out)
    _refused(L, pe, "wire_posenc_bwd", [dict(n=-1), dict(D=0), dict(D=5), dict(D=-1), dict(F=-1), dict(F=31),
                                        dict(c=None), dict(g=None), dict(out=None)], pe)


def test_hparam_grad_refusals():
    """wire_gabor_hparam_grad / wire_gabor2d_hparam_grad: n, in_features or out_features < 1 or a NULL pointer is
    WIRE_ERR_ARG; a workspace below the size query is WIRE_ERR_SIZE; is_first with more than 4 inputs is WIRE_ERR_ARG."""
    L = _lib()
    n, fin, out = 40, 3, 8
    ws1, ws2 = L.wire_layer_ws_bytes(n, fin, out), L.wire_layer2d_ws_bytes(n, fin, out)
    assert ws1 > 0 and ws2 > 0

    def h1(g=P, x=P, W=P, b=P, n=n, fin=fin, out=out, first=0, o2=P, ws=P, wsb=ws1):
        return L.wire_gabor_hparam_grad(None, g, x, W, b, 9.0, 4.0, n, fin, out, first, o2, ws, wsb)

    def h2(g=P, x=P, W=P, b=P, V=P, c=P, n=n, fin=fin, out=out, first=0, o2=P, ws=P, wsb=ws2):
        return L.wire_gabor2d_hparam_grad(None, g, x, W, b, V, c, 6.0, 3.0, n, fin, out, first, o2, ws, wsb)

    common = [dict(n=0), dict(n=-1), dict(fin=0), dict(out=0), dict(fin=-1), dict(out=-1), dict(g=None), dict(x=None),
              dict(W=None), dict(b=None), dict(o2=None), dict(ws=None)]
    _refused(L, h1, "wire_gabor_hparam_grad", common, h1)
    _refused(L, h2, "wire_gabor2d_hparam_grad", common + [dict(V=None), dict(c=None)], h2)
    for fn, full in ((h1, L.wire_layer_ws_bytes(n, 5, out)), (h2, L.wire_layer2d_ws_bytes(n, 5, out))):
        assert fn(wsb=1024) == -3 and b"workspace too small" in L.wire_last_error()
        assert fn(first=1, fin=5, wsb=full) == -1 and b"in_features <= 4" in L.wire_last_error()
