"""GPU checks of the kernels around the net that every training run and every reported number goes through -- the MSE and
pooled losses, flat Adam, the metrics, best-so-far tracking, the sigmoid of the mesh export, coordinate generation, the CT
operator and its adjoint, the layout helpers, the positional encoding's backward and the sums behind a trainable
omega_0 / scale_0 -- each alone, through the C ABI, against the restatements of tests/glue_ref.py.

The standard of tests/test_gpu_tv.py: shapes from the launchers' own block arithmetic (one thread per element in
256-thread blocks, at most 1024 blocks, so a block loops above 262 144 elements), outputs and scratch pre-filled with 7.0
or NaN, a guard of 256 floats behind every buffer the kernel writes (scratch allocated at exactly the size
include/wire_hip.h documents), and every call made twice for the same bits -- except wire_radon_bwd, whose float atomics
the header declares."""
import math

import numpy as np
import pytest
import torch

import _util
from _util import relmax, within_ref
import glue_ref as ref
from oracle import torch_ref

pytestmark = pytest.mark.gpu
DEV = torch.device("cuda:0")
FILL, GUARD, NG = 7.0, -13.0, 256
NAN = float("nan")


def _lib():
    from wire_amd import _lib
    return _lib, _lib.lib()


def _stream():
    return torch.cuda.current_stream().cuda_stream


def _dev(a, dtype=None):
    return torch.tensor(np.ascontiguousarray(a), device=DEV, dtype=dtype)


class _Out:
    """A device buffer of ``numel`` elements pre-filled with ``fill`` and NG guard elements behind it."""

    def __init__(self, numel, fill, dtype=torch.float32):
        self.n = int(numel)
        self.full = torch.empty(self.n + NG, dtype=dtype, device=DEV)
        self.full[:self.n] = fill
        self.full[self.n:] = GUARD
        self.ptr = self.full.data_ptr()

    def get(self):
        """The buffer on the host; the guard must hold its bits."""
        a = self.full.cpu().numpy()
        assert (a[self.n:] == a.dtype.type(GUARD)).all(), "the kernel wrote behind its buffer"
        return a[:self.n]


def _same(a, b):
    return a.tobytes() == b.tobytes()


# ---------------------------------------------------------------------------------------------------------------------
# wire_mse_grad
# ---------------------------------------------------------------------------------------------------------------------
# (n, O):  (1, 1) one element; (85, 3) 255 elements, one ragged block; (256, 1) one full block; (86, 3) a block boundary
# inside row 85; (33, 8) the widest O; (262144, 1) 1024 full blocks, the last size without a loop; (87382, 3) 262 146
# elements: threads 0 and 1 of block 0 loop a second time; (32769, 8) 262 152 elements, the same with O = 8.
MSE_SHAPES = [(1, 1), (85, 3), (256, 1), (86, 3), (33, 8), (262144, 1), (87382, 3), (32769, 8)]


def _mse_call(L, lib, y, t, idx, first, n, O, w, rec_rows):
    gy, loss, part = _Out(n * O, FILL), _Out(1, NAN), _Out(4096, FILL)
    rec = None if rec_rows is None else _Out(rec_rows * O, NAN)
    lib.check(L.wire_mse_grad(_stream(), y.data_ptr(), t.data_ptr(), None if idx is None else idx.data_ptr(), first, n, O,
                              w, gy.ptr, loss.ptr, None if rec is None else rec.ptr, part.ptr), "wire_mse_grad")
    torch.cuda.synchronize()
    part.get()
    return gy.get(), loss.get(), None if rec is None else rec.get()


@pytest.mark.parametrize("n,O", MSE_SHAPES)
def test_mse_grad(n, O):
    """Loss within 1e-5 relative of fp64 and g_y within 1e-6 max|g|, for an index list (a slice of a permutation of a
    longer table), rows 0 .. n and rows 37 .. 37 + n, weights 1, 0.25 and 3/7, rec NULL and given (selected rows == y bit
    for bit, the others keep their NaN)."""
    lib, L = _lib()
    T = n + 100
    rng = np.random.default_rng(n * 10 + O)
    y = rng.standard_normal((n, O)).astype(np.float32)
    t = rng.standard_normal((T, O)).astype(np.float32)
    perm = rng.permutation(T)[:n].astype(np.int64)
    yd, td, pd = _dev(y), _dev(t), _dev(perm)
    worst_l = worst_g = 0.0
    for label, idx, first in (("index list", pd, 0), ("first = 0", None, 0), ("first = 37", None, 37)):
        rows = perm if idx is not None else first + np.arange(n)
        l1, g1 = ref.mse_loss_and_grad(y.astype(np.float64), t[rows].astype(np.float64))
        for w in (1.0, 0.25, 3.0 / 7.0):
            w32 = float(np.float32(w))
            for rec_rows in (None, T):
                a = _mse_call(L, lib, yd, td, idx, first, n, O, w, rec_rows)
                b = _mse_call(L, lib, yd, td, idx, first, n, O, w, rec_rows)
                assert _same(a[0], b[0]) and _same(a[1], b[1]) and (rec_rows is None or _same(a[2], b[2]))
                gy, loss, rec = a
                el = abs(float(loss[0]) - w32 * l1) / (w32 * l1)
                eg = np.abs(gy.reshape(n, O) - w32 * g1).max() / np.abs(w32 * g1).max()
                worst_l, worst_g = max(worst_l, el), max(worst_g, eg)
                assert el <= 1e-5, (label, w, el)
                assert eg <= 1e-6, (label, w, eg)
                if rec is not None:
                    rec = rec.reshape(T, O)
                    sel = np.zeros(T, bool)
                    sel[rows] = True
                    assert _same(rec[rows], y) and np.isnan(rec[~sel]).all()
    print(f"mse_grad {(n, O)}: worst loss rel {worst_l:.2e}  worst g_y / max|g| {worst_g:.2e}")


def test_mse_grad_no_rows_touches_nothing():
    """n == 0 returns WIRE_OK and writes neither g_y, loss_out, rec nor partial."""
    lib, L = _lib()
    y = _dev(np.ones((4, 3), np.float32))
    gy, loss, rec, part = _Out(12, FILL), _Out(1, FILL), _Out(12, FILL), _Out(4096, FILL)
    for idx in (None, _dev(np.arange(4))):
        assert L.wire_mse_grad(_stream(), y.data_ptr(), y.data_ptr(), None if idx is None else idx.data_ptr(), 0, 0, 3,
                               1.0, gy.ptr, loss.ptr, rec.ptr, part.ptr) == 0
        torch.cuda.synchronize()
        for b in (gy, loss, rec, part):
            assert (b.get() == FILL).all()


# ---------------------------------------------------------------------------------------------------------------------
# wire_avgpool_mse_grad
# ---------------------------------------------------------------------------------------------------------------------
# (H, W, O, scale):  (1, 1, 1, 1) one element; (5, 7, 2, 1) scale 1 is the plain full-grid MSE; (6, 9, 1, 6) scale ==
# min(H, W): one window and three ragged columns; (16, 16, 8, 2) the widest O; (26, 21, 3, 4) ragged on both sides;
# (513, 512, 1, 1) and (1026, 1024, 1, 2): 262 656 pooled elements, blocks 0 and 1 loop a second time.
POOL_SHAPES = [(1, 1, 1, 1), (5, 7, 2, 1), (6, 9, 1, 6), (16, 16, 8, 2), (26, 21, 3, 4), (513, 512, 1, 1),
               (1026, 1024, 1, 2)]


@pytest.mark.parametrize("H,W,O,scale", POOL_SHAPES)
def test_avgpool_mse_grad(H, W, O, scale):
    """Loss 1e-5 relative, g_y 1e-6 max|g|, rec_lr 2e-6 against the fp64 restatement; ragged borders of g_y exactly
    +0.0 over the 7.0 pre-fill; rec_lr NULL and given."""
    lib, L = _lib()
    H2, W2 = H // scale, W // scale
    rng = np.random.default_rng(H * 7 + W * 3 + O + scale)
    y = rng.standard_normal((H * W, O)).astype(np.float32)
    gt = rng.standard_normal((H2 * W2, O)).astype(np.float32)
    l64, g64, r64 = ref.avgpool_mse_loss_and_grad(y.astype(np.float64), H, W, scale, gt.astype(np.float64))
    yd, gd = _dev(y), _dev(gt)
    for with_rec in (False, True):
        res = []
        for _ in range(2):
            gy, loss, part = _Out(H * W * O, FILL), _Out(1, NAN), _Out(1024, FILL)
            rec = _Out(H2 * W2 * O, NAN) if with_rec else None
            lib.check(L.wire_avgpool_mse_grad(_stream(), yd.data_ptr(), H, W, O, scale, gd.data_ptr(), gy.ptr,
                                              rec.ptr if rec else None, loss.ptr, part.ptr), "wire_avgpool_mse_grad")
            torch.cuda.synchronize()
            part.get()
            res.append((gy.get(), loss.get(), rec.get() if rec else np.zeros(0, np.float32)))
        assert all(_same(p, q) for p, q in zip(*res))
        gy, loss, rec = res[0]
        el = abs(float(loss[0]) - l64) / l64
        eg = np.abs(gy.reshape(H * W, O) - g64).max() / np.abs(g64).max()
        print(f"avgpool_mse_grad {(H, W, O, scale)} rec={with_rec}: loss rel {el:.2e}  g_y / max|g| {eg:.2e}")
        assert el <= 1e-5 and eg <= 1e-6
        img = gy.reshape(H, W, O)
        for border in (img[H2 * scale:], img[:, W2 * scale:]):
            assert _same(np.ascontiguousarray(border), np.zeros(border.shape, np.float32))
        if with_rec:
            er = np.abs(rec.reshape(H2 * W2, O) - r64).max()
            print(f"avgpool_mse_grad {(H, W, O, scale)}: rec_lr abs {er:.2e}")
            assert er <= 2e-6


# ---------------------------------------------------------------------------------------------------------------------
# wire_adam_step_flat
# ---------------------------------------------------------------------------------------------------------------------
ADAM_SETTINGS = {"default": dict(lr=5e-3), "beta1 = 0": dict(lr=5e-3, beta1=0.0), "lr = 0": dict(lr=0.0)}


@pytest.mark.parametrize("setting", list(ADAM_SETTINGS))
@pytest.mark.parametrize("step0", [1, 1000, 10 ** 6])
def test_adam_step_flat(step0, setting):
    """Three consecutive steps from non-zero moments at counts around one block: param within 2e-6 absolute of fp64
    (p ~ N(0, 1), lr 5e-3), exp_avg and exp_avg_sq within 2 x the fp32 restatement's own error + 1e-6; with lr == 0
    param keeps its bits."""
    lib, L = _lib()
    kw = dict(beta1=0.9, beta2=0.999, eps=1e-8)
    kw.update(ADAM_SETTINGS[setting])
    for cnt in (1, 255, 256, 257, 10007):
        rng = np.random.default_rng(cnt + step0 % 1000)
        p0 = rng.standard_normal(cnt).astype(np.float32)
        m0 = (0.01 * rng.standard_normal(cnt)).astype(np.float32)
        v0 = (1e-4 * rng.random(cnt) + 1e-8).astype(np.float32)
        gs = [(rng.standard_normal(cnt) * 10.0 ** rng.integers(-6, 1, cnt)).astype(np.float32) for _ in range(3)]
        gds = [_dev(g) for g in gs]
        res = []
        for _ in range(2):
            p, m, v = _Out(cnt, 0.0), _Out(cnt, 0.0), _Out(cnt, 0.0)
            for buf, a in ((p, p0), (m, m0), (v, v0)):
                buf.full[:cnt] = _dev(a)
            for k in range(3):
                lib.check(L.wire_adam_step_flat(_stream(), p.ptr, gds[k].data_ptr(), m.ptr, v.ptr, cnt, kw["lr"],
                                                kw["beta1"], kw["beta2"], kw["eps"], step0 + k), "wire_adam_step_flat")
            torch.cuda.synchronize()
            res.append((p.get(), m.get(), v.get()))
        assert all(_same(a, b) for a, b in zip(*res))
        p, m, v = res[0]
        p64, m64, v64 = ref.adam_steps(p0, gs, m0, v0, step0, double=True, **kw)
        _, m32, v32 = ref.adam_steps(p0, gs, m0, v0, step0, double=False, **kw)
        ep = np.abs(p - p64).max()
        print(f"adam count {cnt} step {step0} {setting}: param abs {ep:.2e}")
        assert ep <= 2e-6
        tag = f"glue adam count={cnt} step0={step0} {setting}"
        within_ref(relmax(m, m64), relmax(m32, m64), tag + " exp_avg")
        within_ref(relmax(v, v64), relmax(v32, v64), tag + " exp_avg_sq")
        if kw["lr"] == 0.0:
            assert _same(p, p0)
        if kw["beta1"] == 0.0:
            assert _same(m, gs[2])


# ---------------------------------------------------------------------------------------------------------------------
# wire_eval_metric
# ---------------------------------------------------------------------------------------------------------------------
METRIC_COUNTS = [1, 255, 256, 257, 262144, 262145, 786432]


def _metric(L, lib, mode, rec, gt, count, thres):
    res = []
    for _ in range(2):
        out, part = _Out(2, NAN), _Out(2048, FILL)
        lib.check(L.wire_eval_metric(_stream(), mode, rec.data_ptr(), gt.data_ptr(), count, thres, out.ptr, part.ptr),
                  "wire_eval_metric")
        torch.cuda.synchronize()
        part.get()
        res.append(out.get())
    assert _same(*res)
    return res[0]


@pytest.mark.parametrize("count", METRIC_COUNTS)
def test_eval_metric_psnr_sums(count):
    """Mode 0: the sum of squares within 1e-5 relative of fp64, the maximum bit-equal to max(gt), also when every gt is
    negative (the running maximum must not start at 0)."""
    lib, L = _lib()
    rng = np.random.default_rng(count)
    rec = rng.standard_normal(count).astype(np.float32)
    for label, gt in (("mixed", rng.standard_normal(count).astype(np.float32)),
                      ("all negative", (-0.5 - rng.random(count)).astype(np.float32))):
        out = _metric(L, lib, 0, _dev(rec), _dev(gt), count, 0.0)
        s64, mx = ref.metric_sums(rec, gt)
        es = abs(float(out[0]) - s64) / s64
        print(f"eval_metric mode 0 count {count} {label}: sum rel {es:.2e}  max {out[1]}")
        assert es <= 1e-5
        assert _same(out[1:2], np.array([mx], np.float32))


def _iou_inputs(count, rng):
    rec = rng.random(count).astype(np.float32)
    gt = (rng.random(count) < 0.3).astype(np.float32)
    # rec == thres (counts), gt == -0.0 (is zero), a negative gt (is not), NaN in rec (below), NaN in gt (not zero)
    edge_rec = np.array([0.5, 0.5, 0.9, 0.2, 0.9, NAN, NAN, 0.9, 0.2], np.float32)
    edge_gt = np.array([1.0, 0.0, -0.0, -0.0, -3.0, 1.0, 0.0, NAN, NAN], np.float32)
    k = min(count, len(edge_rec))
    pos = np.arange(k) * max(1, (count - 1) // max(1, k - 1)) if k > 1 else np.zeros(1, np.int64)
    rec[pos], gt[pos] = edge_rec[:k], edge_gt[:k]
    return rec, gt


@pytest.mark.parametrize("count", METRIC_COUNTS + [1 << 24])
def test_eval_metric_iou_counts_are_exact(count):
    """Mode 1: both counts equal numpy's integers exactly, with rec == thres, gt == -0.0, a negative gt and NaN in either
    input among the elements; at 2^24 elements -- the slab modules/volutils.get_I_and_U feeds it -- as well."""
    lib, L = _lib()
    rec, gt = _iou_inputs(count, np.random.default_rng(count + 1))
    inter, union = ref.iou_counts(rec, gt, 0.5)
    out = _metric(L, lib, 1, _dev(rec), _dev(gt), count, 0.5)
    print(f"eval_metric mode 1 count {count}: {out} expected {(inter, union)}")
    assert float(out[0]) == inter and float(out[1]) == union
    assert count < 9 or (0 < inter < union < count)


# ---------------------------------------------------------------------------------------------------------------------
# wire_track_best
# ---------------------------------------------------------------------------------------------------------------------
# (force, metric, best, taken)
BEST_CASES = {"forced": (1, 5.0, 1.0, True), "below": (0, 0.5, 1.0, True), "equal": (0, 1.0, 1.0, False),
              "above": (0, 2.0, 1.0, False), "NaN metric": (0, NAN, 1.0, False), "best = +inf": (0, 3.0, math.inf, True)}


@pytest.mark.parametrize("count", [0, 1, 3, 4, 5, 1023, 1024, 1025, 4099])
def test_track_best(count):
    """Taken: dst == src bit for bit, best_metric == metric, updated == 1.  Not taken: dst keeps its pre-fill, best_metric
    its value, updated == 0.  Nothing behind dst[count - 1] is written at any tail of the 4-wide copy."""
    lib, L = _lib()
    src = np.random.default_rng(count).standard_normal(count).astype(np.float32)
    srcd = _dev(np.concatenate([src, np.zeros(4, np.float32)]))           # never empty: a valid, aligned pointer
    assert srcd.data_ptr() % 16 == 0
    for label, (force, metric, best, taken) in BEST_CASES.items():
        md = _dev(np.array([metric], np.float32))
        for with_upd in (False, True):
            res = []
            for _ in range(2):
                dst, bm = _Out(count, FILL), _Out(1, best)
                upd = _Out(1, -5, dtype=torch.int32) if with_upd else None
                assert dst.ptr % 16 == 0
                lib.check(L.wire_track_best(_stream(), md.data_ptr(), bm.ptr, force,
                                            srcd.data_ptr(), dst.ptr, count, upd.ptr if upd else None), "wire_track_best")
                torch.cuda.synchronize()
                res.append((dst.get(), bm.get(), upd.get() if upd else np.zeros(1, np.int32)))
            assert all(_same(a, b) for a, b in zip(*res)), label
            d, b, u = res[0]
            if taken:
                assert _same(d, src) and _same(b, np.array([metric], np.float32)), label
            else:
                assert (d == FILL).all() and _same(b, np.array([best], np.float32)), label
            if with_upd:
                assert u[0] == int(taken), label


# ---------------------------------------------------------------------------------------------------------------------
# wire_sigmoid_inplace
# ---------------------------------------------------------------------------------------------------------------------
_SPECIAL = np.array([0.0, 1e-8, 17.0, 87.3, 88.7, 88.72, 88.8, 103.9, 104.0, 200.0, 1e30, math.inf], np.float32)
SIGMOID_SPECIAL = np.concatenate([_SPECIAL, -_SPECIAL, [np.float32(NAN)]]).astype(np.float32)
SIGMOID_SWEEP = (np.arange(-120 * 64, 120 * 64 + 1) / 64.0).astype(np.float32)


def _sigmoid_values(count):
    if count == 1:
        return np.array([-95.0], np.float32)          # 1 / (1 + wire_exp(95)) is NaN: inf * tl + inf with tl = -1.4e-6
    pool = np.concatenate([SIGMOID_SPECIAL, SIGMOID_SWEEP if count > 20000 else SIGMOID_SWEEP[::67]])
    assert len(pool) <= count
    return np.resize(pool, count)


@pytest.mark.parametrize("count", [1, 255, 256, 257, 65537])
def test_sigmoid_inplace(count):
    """NaN -> NaN; +inf and every x >= 17 -> exactly 1; -inf -> exactly 0; x <= -87.4 -> a value in [0, 2^-126] (the
    true value is denormal); elsewhere within 2^-21 relative of fp64 (wire_exp's 1 to 2 ulp, one add, one divide).  The
    largest count holds the whole sweep -120 .. 120 in steps of 1/64 and every special value, both signs."""
    lib, L = _lib()
    x = _sigmoid_values(count)
    res = []
    for _ in range(2):
        buf = _Out(count, 0.0)
        buf.full[:count] = _dev(x)
        lib.check(L.wire_sigmoid_inplace(_stream(), buf.ptr, count), "wire_sigmoid_inplace")
        torch.cuda.synchronize()
        res.append(buf.get())
    assert _same(*res)
    got = res[0]
    want = ref.sigmoid64(x)
    nan, one, low = np.isnan(x), x >= 17.0, x <= np.float32(-87.4)
    rest = ~(nan | one | low)
    bad_nan = int(np.isnan(got[~nan]).sum())
    if bad_nan:
        bx = x[~nan][np.isnan(got[~nan])]
        print(f"sigmoid count {count}: NaN for {bad_nan} finite or infinite inputs, from {bx.min()} to {bx.max()}")
    assert np.isnan(got[nan]).all() and bad_nan == 0
    assert (got[one] == 1.0).all()
    assert (got[x == -math.inf] == 0.0).all()
    assert ((got[low] >= 0.0) & (got[low] <= np.float32(2.0 ** -126))).all()
    if rest.any():
        rel = np.abs(got[rest].astype(np.float64) - want[rest]) / want[rest]
        k = int(rel.argmax())
        print(f"sigmoid count {count}: worst rel err {rel.max():.3e} = {rel.max() * 2 ** 24:.2f} x 2^-24 at x = {x[rest][k]}")
        _util.RATIO_LOG.append((f"glue sigmoid count={count} worst rel err | bound 2^-21", float(rel.max()), 2.0 ** -21))
        assert rel.max() <= 2.0 ** -21


# ---------------------------------------------------------------------------------------------------------------------
# wire_coords_from_index
# ---------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("n", [1, 255, 256, 257, 1000])
@pytest.mark.parametrize("dims", [2, 3])
def test_coords_from_index(dims, n):
    """Bit-equal to the table look-ups (2-D: idx = i W + j -> (tx[j], ty[i]); 3-D: idx = (i W + j) T + k -> (tx[j],
    ty[i], tz[k])) for an index list that tiles the (5, 7) / (6, 5, 4) grid with repeats, and for the ranges first = 0
    and first = 37, whose grid gets as many rows as first + n needs (a range cannot repeat)."""
    lib, L = _lib()
    rng = np.random.default_rng(dims * 10000 + n)
    for label, use_idx, first in (("index list", True, 0), ("first = 0", False, 0), ("first = 37", False, 37)):
        W, T = (7, 1) if dims == 2 else (5, 4)
        H = 5 if dims == 2 else 6
        if not use_idx:
            H = max(H, -(-(first + n) // (W * T)))
        tx, ty, tz = (rng.standard_normal(k).astype(np.float32) for k in (W, H, T))
        ids = rng.integers(0, H * W * T, n).astype(np.int64) if use_idx else first + np.arange(n, dtype=np.int64)
        assert ids.min() >= 0 and ids.max() < H * W * T
        k, ij = ids % T, ids // T
        want = np.stack([tx[ij % W], ty[ij // W]] + ([tz[k]] if dims == 3 else []), 1)
        txd, tyd, tzd, idd = _dev(tx), _dev(ty), _dev(tz), _dev(ids)
        res = []
        for _ in range(2):
            out = _Out(n * dims, NAN)
            lib.check(L.wire_coords_from_index(_stream(), idd.data_ptr() if use_idx else None, first, n, txd.data_ptr(), W,
                                               tyd.data_ptr(), H, tzd.data_ptr() if dims == 3 else None, T, out.ptr),
                      "wire_coords_from_index")
            torch.cuda.synchronize()
            res.append(out.get())
        assert _same(*res) and _same(res[0], want.astype(np.float32)), label


# ---------------------------------------------------------------------------------------------------------------------
# wire_radon_fwd / wire_radon_bwd
# ---------------------------------------------------------------------------------------------------------------------
# (H, W, A): one thread per column in 256-column blocks.  (9, 300, 8) a second block column, ragged; (5, 256, 8) exactly
# one; (5, 257, 8) one column in the second; (2, 2, 8) every sample touches the border; (1, 7, 3) and (7, 1, 3) sides of
# 1, where the header's formula holds as written; (37, 52, 1) a single angle.
@pytest.mark.parametrize("H,W,A", ref.RADON_SHAPES)
def test_radon_fwd_bwd(H, W, A):
    """Forward and adjoint within 2 x the fp32 restatement's own error + 1e-6 of the direct fp64 restatement;
    <A x, y> == <x, A^T y> to 1e-5 relative; the forward gives the same bits twice."""
    lib, L = _lib()
    img, g, ang = ref.radon_case(H, W, A)
    imd, gd, ad = _dev(img), _dev(g), _dev(ang)
    res = []
    for _ in range(2):
        sino, gimg = _Out(A * W, NAN), _Out(H * W, FILL)
        lib.check(L.wire_radon_fwd(_stream(), imd.data_ptr(), ad.data_ptr(), H, W, A, sino.ptr), "wire_radon_fwd")
        lib.check(L.wire_radon_bwd(_stream(), gd.data_ptr(), ad.data_ptr(), H, W, A, gimg.ptr), "wire_radon_bwd")
        torch.cuda.synchronize()
        res.append((sino.get().reshape(A, W), gimg.get().reshape(H, W)))
    assert _same(res[0][0], res[1][0])
    s64, s32 = ref.radon(img, ang, np.float64), ref.radon(img, ang, np.float32)
    b64, b32 = ref.radon_adjoint(g, ang, H, W, np.float64), ref.radon_adjoint(g, ang, H, W, np.float32)
    for sino, gimg in res:
        within_ref(relmax(sino, s64), relmax(s32, s64), f"glue radon fwd {(H, W, A)}")
        within_ref(relmax(gimg, b64), relmax(b32, b64), f"glue radon adjoint {(H, W, A)}")
        lhs = float((sino.astype(np.float64) * g).sum())
        rhs = float((gimg.astype(np.float64) * img).sum())
        print(f"radon {(H, W, A)}: <Ax, y> {lhs:.9e}  <x, A^T y> {rhs:.9e}  rel {abs(lhs - rhs) / abs(lhs):.2e}")
        assert abs(lhs - rhs) <= 1e-5 * abs(lhs)


# ---------------------------------------------------------------------------------------------------------------------
# wire_c64_to_blocked / wire_blocked_to_c64
# ---------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("n", [1, 5])
@pytest.mark.parametrize("K", [1, 31, 32, 33, 64, 90])
def test_layout_helpers(K, n):
    """The blocked image is bit-equal to the restatement, its pad columns +0.0 over a NaN pre-fill; the way back is
    bit-exact; wire_blocked_width(K) is the row length."""
    lib, L = _lib()
    rng = np.random.default_rng(K * 10 + n)
    z = (rng.standard_normal((n, K)) + 1j * rng.standard_normal((n, K))).astype(np.complex64)
    want = ref.to_blocked(z)
    P = L.wire_blocked_width(K)
    assert P == want.shape[1]
    zd = _dev(z.view(np.float32))
    res = []
    for _ in range(2):
        blk, back = _Out(n * P, NAN), _Out(n * 2 * K, NAN)
        lib.check(L.wire_c64_to_blocked(_stream(), zd.data_ptr(), n, K, blk.ptr), "wire_c64_to_blocked")
        lib.check(L.wire_blocked_to_c64(_stream(), blk.ptr, n, K, back.ptr), "wire_blocked_to_c64")
        torch.cuda.synchronize()
        res.append((blk.get(), back.get()))
    assert all(_same(a, b) for a, b in zip(*res))
    assert _same(res[0][0], want) and _same(res[0][1], z.view(np.float32))


# ---------------------------------------------------------------------------------------------------------------------
# wire_posenc_bwd
# ---------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("n", [1, 3, 4, 5])
def test_posenc_bwd(n):
    """D = 3, F = 10 (63 inputs, the reference's own count for three coordinates) at row counts around the four rows of
    a block: within 2 x the fp32 eager reference's own error + 1e-6 of its fp64 autograd gradient, the bound of
    test_gpu_shape_envelope.test_posencoding_alone_d4."""
    lib, L = _lib()
    D, F = 3, 10
    width = D + 2 * D * F
    gen = torch.Generator().manual_seed(n)
    coords = (torch.rand(n, D, generator=gen, dtype=torch.float64) * 2 - 1).to(torch.float32)
    w = torch.randn(n, width, generator=gen, dtype=torch.float64).to(torch.float32)

    def grad(dt):
        c = coords.to(dt).clone().requires_grad_(True)
        (torch_ref.posenc(c, F) * w.to(dt)).sum().backward()
        return c.grad.to(torch.float64).numpy()
    g64, g32 = grad(torch.float64), grad(torch.float32)
    cd, wd = coords.to(DEV), w.to(DEV)
    res = []
    for _ in range(2):
        out = _Out(n * D, NAN)
        lib.check(L.wire_posenc_bwd(_stream(), cd.data_ptr(), n, D, F, wd.data_ptr(), out.ptr), "wire_posenc_bwd")
        torch.cuda.synchronize()
        res.append(out.get())
    assert _same(*res)
    within_ref(relmax(res[0].reshape(n, D), g64), relmax(g32, g64), f"glue posenc_bwd D=3 F=10 n={n}")


# ---------------------------------------------------------------------------------------------------------------------
# wire_gabor_hparam_grad / wire_gabor2d_hparam_grad
# ---------------------------------------------------------------------------------------------------------------------
HP_ROWS = 4133          # 129 full blocks of 32 rows and one of 5: several partial sums and a ragged block


def _hparam_inputs(first, seed):
    rng = np.random.default_rng(seed)
    fin, out = (3, 40) if first else (24, 40)
    cplx = lambda *sh: (rng.standard_normal(sh) + 1j * rng.standard_normal(sh)).astype(np.complex64)
    if first:
        x = rng.uniform(-1, 1, (HP_ROWS, fin)).astype(np.float32)
        mk = lambda *sh: (0.3 * rng.standard_normal(sh)).astype(np.float32)
    else:
        x = (0.5 * cplx(HP_ROWS, fin)).astype(np.complex64)
        mk = lambda *sh: (0.06 * cplx(*sh)).astype(np.complex64)
    return x, mk(out, fin), mk(out), mk(out, fin), mk(out), cplx(HP_ROWS, out), fin, out


def _raw(a):
    return _dev(a.view(np.float32) if np.iscomplexobj(a) else a)


@pytest.mark.parametrize("first", [False, True])
@pytest.mark.parametrize("layer", ["gabor", "gabor2d"])
def test_hparam_grads(layer, first):
    """{dL/d omega_0, dL/d scale_0} of a hidden and a first layer on 4133 rows against the fp64 closed forms.  Each is one
    number, a sum of 165 320 terms that partly cancel, so the error is taken relative to the sum of the terms'
    magnitudes -- the scale any summation order's rounding is proportional to -- and bounded by 2 x the same error of
    the fp32 restatement + 1e-6.  The workspace is pre-filled with NaN bytes."""
    lib, L = _lib()
    x, W, b, V, c, g, fin, out = _hparam_inputs(first, 5 if layer == "gabor" else 6)
    w0, s0 = (9.0, 4.0) if layer == "gabor" else (6.0, 3.0)
    if layer == "gabor":
        v64, a64 = ref.gabor_hparam_grads(x, W, b, g, w0, s0, True)
        v32 = ref.gabor_hparam_grads(x, W, b, g, w0, s0, False)[0]
        wsb = lib.check(L.wire_layer_ws_bytes(HP_ROWS, fin, out), "wire_layer_ws_bytes")
    else:
        v64, a64 = ref.gabor2d_hparam_grads(x, W, b, V, c, g, w0, s0, True)
        v32 = ref.gabor2d_hparam_grads(x, W, b, V, c, g, w0, s0, False)[0]
        wsb = lib.check(L.wire_layer2d_ws_bytes(HP_ROWS, fin, out), "wire_layer2d_ws_bytes")
    assert min(a64) > 0 and all(abs(v) > 1e-3 * a for v, a in zip(v64, a64))       # the sums do not cancel to nothing
    xd, Wd, bd, Vd, cd, gd = (_raw(a) for a in (x, W, b, V, c, g))
    res = []
    for _ in range(2):
        out2 = _Out(2, FILL)
        ws = torch.full((wsb + 4 * NG,), 255, dtype=torch.uint8, device=DEV)
        ws[wsb:] = 0x5A
        if layer == "gabor":
            lib.check(L.wire_gabor_hparam_grad(_stream(), gd.data_ptr(), xd.data_ptr(), Wd.data_ptr(), bd.data_ptr(), w0,
                                               s0, HP_ROWS, fin, out, int(first), out2.ptr, ws.data_ptr(), wsb),
                      "wire_gabor_hparam_grad")
        else:
            lib.check(L.wire_gabor2d_hparam_grad(_stream(), gd.data_ptr(), xd.data_ptr(), Wd.data_ptr(), bd.data_ptr(),
                                                 Vd.data_ptr(), cd.data_ptr(), w0, s0, HP_ROWS, fin, out, int(first),
                                                 out2.ptr, ws.data_ptr(), wsb), "wire_gabor2d_hparam_grad")
        torch.cuda.synchronize()
        assert bool((ws[wsb:] == 0x5A).all()), "the kernels wrote behind the workspace"
        res.append(out2.get())
    assert _same(*res)
    for k, name in enumerate(("omega_0", "scale_0")):
        eb = abs(float(res[0][k]) - float(v64[k])) / a64[k]
        er = abs(float(v32[k]) - float(v64[k])) / a64[k]
        print(f"hparam {layer} first={first} dL/d{name}: {res[0][k]:.6e} (fp64 {float(v64[k]):.6e}) err {eb:.2e} ref {er:.2e}")
        within_ref(eb, er, f"glue hparam {layer} {'first' if first else 'hidden'} dL/d{name} [relative to sum |terms|]")
