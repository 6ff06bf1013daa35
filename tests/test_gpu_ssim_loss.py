"""GPU checks of the differentiable SSIM loss: wire_ssim_bwd against fp64 autograd of the restatement with the fp32
autograd's own error as the yardstick, wire_ssim_mse_grad against the fp64 restatement of the
regularised loss, functional.ssim_loss, and FusedTrainer.step_ssim -- every parameter gradient against the fp64
oracle, patterned on the step_tv tests of tests/test_gpu_tv.py."""
import ctypes as C

import numpy as np
import pytest
import torch

from _util import _grid_coords, _sd, params_np, relmax, within_ref
import hier_ref as hr
import ssim_grad_ref as gref
import ssim_ref as ref
from oracle import wire_oracle as wo

pytestmark = pytest.mark.gpu
DEV = torch.device("cuda:0")
FILL = 7.0

# (H, W, O).  The first eight are the shapes of tests/test_gpu_ssim.py, taken over as they are; (11, 11, 1) and
# (7, 7, 1) hold one window, so A, B and C are scalars.  The gradient kernel tiles the INPUT: one workgroup owns
# 16 x 32 pixels (wire_ssim_bwd.hip, SSIMB_TR x SSIMB_TC) and stages a halo of taps - 1 = 10 (Gaussian) / 6 (uniform)
# further pixels on every side that the image has.  What the shapes are for, in those numbers:
#   every single-tile shape  the halo is cut by all four edges at once; (33, 8, 2), (11, 11, 1), (15, 16, 8) are narrower
#                            than a tile;
#   (47, 81, 3)  3 x 3 tiles of 16 / 16 / 15 rows and 32 / 32 / 17 columns: the edge tiles' halos are cut by one or two
#                edges each; the middle tile's reaches rows 6 .. 41 and columns 22 .. 73, cut by none (Gaussian: the
#                valid region ends at row 36, so the windows below it are the zero slots);
#   (49, 99, 1)  4 x 4 tiles: two interior tiles per axis, and a last tile of 1 row / 3 columns that owns no window;
#   (17, 44, 8)  the channel limit.  The kernel takes one channel at a time, so its LDS footprint (58 320 B at 11 taps)
#                does not depend on O; O = 8 is the longest channel loop.  The second tile has 12 columns and 1 row;
#   (18, 35, 2)  a second tile of 3 columns and 2 rows: less than the halo of 10 (or 6) it shares with its neighbour, so
#                every window that covers its pixels begins in the neighbour's tile;
#   (18, 45, 5)  an odd channel count on a ragged second tile (13 columns, 2 rows).
SHAPES = [(11, 11, 1), (7, 7, 1), (12, 29, 3), (33, 8, 2), (15, 16, 8), (47, 81, 3), (17, 44, 8), (18, 45, 5),
          (18, 35, 2), (49, 99, 1)]
CASES = [(s, k) for s in SHAPES for k in ("gaussian", "uniform") if min(s[0], s[1]) >= len(ref.window(k)[0])]


def _bwd(x, y, win, cov, data_range, up=1.0):
    """wire_ssim_bwd on two [H, W, O] arrays with the upstream gradient ``up``; g_y is prefilled with FILL."""
    from wire_amd import _lib
    L = _lib.lib()
    H, W, O = x.shape
    taps = len(win)
    xt, yt = torch.tensor(x, device=DEV), torch.tensor(y, device=DEV)
    gy = torch.full((H, W, O), FILL, device=DEV)
    g = torch.full((1,), float(up), device=DEV)
    ws_bytes = _lib.check(L.wire_ssim_bwd_ws_bytes(H, W, O, taps), "ws_bytes")
    ws = torch.empty(ws_bytes, dtype=torch.uint8, device=DEV)
    wh = (C.c_float * taps)(*win.tolist())
    _lib.check(L.wire_ssim_bwd(torch.cuda.current_stream().cuda_stream, xt.data_ptr(), yt.data_ptr(), H, W, O, taps, wh,
                               cov, (0.01 * data_range) ** 2, (0.03 * data_range) ** 2, g.data_ptr(), gy.data_ptr(),
                               ws.data_ptr(), ws_bytes), "wire_ssim_bwd")
    torch.cuda.synchronize()
    return gy.cpu().numpy()


def _check_grad(label, gy, c, up=1.0):
    """max|g_y - up g64| / (|up| max|g64|) within 2 x the fp32 autograd's own error + 1e-6; no element keeps FILL."""
    assert gy.shape == c["g64"].shape and not (gy == FILL).any() and np.isfinite(gy).all()
    eb = np.abs(gy.astype(np.float64) - up * c["g64"]).max() / (abs(up) * c["scale"])
    print(f"{label}: err_build {eb:.3e}  err_ref {c['err_ref']:.3e}  max|g64| {c['scale']:.3e}")
    within_ref(eb, c["err_ref"], label)


@pytest.mark.parametrize("shape,kind", CASES)
def test_ssim_bwd_matches_fp64_autograd(shape, kind):
    for sigma in ref.SIGMAS:
        c = gref.case(shape, sigma, kind)
        win, cov, L = c["win"], c["cov"], c["data_range"]
        gy = _bwd(c["gt"], c["rec"], win, cov, L)
        _check_grad(f"ssim_bwd {shape} {kind} sigma={sigma}", gy, c)
        assert _bwd(c["gt"], c["rec"], win, cov, L).tobytes() == gy.tobytes()          # the same call twice
    # a non-unit upstream gradient (the last sigma), also twice
    gu = _bwd(c["gt"], c["rec"], win, cov, L, up=-2.5)
    _check_grad(f"ssim_bwd {shape} {kind} upstream -2.5", gu, c, up=-2.5)
    assert _bwd(c["gt"], c["rec"], win, cov, L, up=-2.5).tobytes() == gu.tobytes()
    # rec = gt: fp64 gives ~0, so the errors are absolute and the floor decides
    z = gref.grads(c["gt"], c["gt"], win, cov, L)
    assert np.abs(z["g64"]).max() <= 1e-12 and z["scale"] == 1.0
    g0 = _bwd(c["gt"], c["gt"], win, cov, L)
    _check_grad(f"ssim_bwd {shape} {kind} rec = gt", g0, z)
    assert _bwd(c["gt"], c["gt"], win, cov, L).tobytes() == g0.tobytes()


def test_ssim_bwd_other_window_sizes():
    """The odd sizes between the two definitions' (3, 5, 9 taps; uniform weights, sample covariance) on the 3 x 3-tile
    shape: the same bound, the same bits twice."""
    shape = (47, 81, 3)
    gt, rec = ref.inputs(shape, 0.1)
    for taps in (3, 5, 9):
        win, cov = gref.uniform_window(taps)
        c = gref.grads(gt, rec, win, cov, 1.0)
        gy = _bwd(gt, rec, win, cov, 1.0)
        _check_grad(f"ssim_bwd {shape} {taps} uniform taps", gy, c)
        assert _bwd(gt, rec, win, cov, 1.0).tobytes() == gy.tobytes()


# ---------------------------------------------------------------------------------------------------------------
# wire_ssim_mse_grad
# ---------------------------------------------------------------------------------------------------------------
def _mse_grad(y, t, H, W, O, win, cov, data_range, lam, idx=None, first=0, n=None):
    """wire_ssim_mse_grad on [H*W, O] arrays; every output is prefilled with FILL.  Returns (parts[3], g_y, rec)."""
    from wire_amd import _lib
    L = _lib.lib()
    taps = len(win)
    yt, tt = torch.tensor(y, device=DEV), torch.tensor(t, device=DEV)
    gy, rec = torch.full((H * W, O), FILL, device=DEV), torch.full((H * W, O), FILL, device=DEV)
    out = torch.full((3,), FILL, device=DEV)
    it = None if idx is None else torch.tensor(np.asarray(idx, np.int64), device=DEV)
    n = (len(idx) if idx is not None else H * W - first) if n is None else n
    ws_bytes = _lib.check(L.wire_ssim_mse_grad_ws_bytes(H, W, O, taps), "ws_bytes")
    ws = torch.empty(ws_bytes, dtype=torch.uint8, device=DEV)
    wh = (C.c_float * taps)(*win.tolist())
    _lib.check(L.wire_ssim_mse_grad(torch.cuda.current_stream().cuda_stream, yt.data_ptr(), H, W, O, tt.data_ptr(), taps,
                                    wh, cov, (0.01 * data_range) ** 2, (0.03 * data_range) ** 2,
                                    None if it is None else it.data_ptr(), first, n, lam, gy.data_ptr(), out.data_ptr(),
                                    rec.data_ptr(), ws.data_ptr(), ws_bytes), "wire_ssim_mse_grad")
    torch.cuda.synchronize()
    return out.cpu().numpy(), gy.cpu().numpy(), rec.cpu().numpy()


@pytest.mark.parametrize("kind", ["gaussian", "uniform"])
@pytest.mark.parametrize("lam", [0.0, 0.1, -0.5])
def test_ssim_mse_grad_matches_restatement(kind, lam):
    """40 x 37 x 3 (3 x 2 tiles of the gradient kernel), the rows as an index list and as a range; a partial selection, a
    full one and an empty one.  g_y within 2 x the fp32 restatement's own error + 1e-6 of max|g64|; mse 1e-5 relative
    (the bound of wire_tv_mse_grad); ssim within the metric's bound, 2 x the fp32 restatement's mean |map error| + 1e-6;
    loss == fl(mse + fl(lam fl(1 - ssim))) of the stored parts; rec exactly the selected rows; lam = 0 leaves the index
    out (ssim reported as 0, unselected rows of g_y zero); the same call twice gives the same bits."""
    H, W, O = 40, 37, 3
    n = H * W
    t, y = (a.reshape(n, O) for a in ref.inputs((H, W, O), 0.1))
    win, cov = ref.window(kind)
    L = ref.DATA_RANGE[kind]
    lam = float(np.float32(lam))
    mean64, map64 = ref.ssim_map(t.reshape(H, W, O), y.reshape(H, W, O), win, cov, L, torch.float64)
    _, map32 = ref.ssim_map(t.reshape(H, W, O), y.reshape(H, W, O), win, cov, L, torch.float32)
    ssim_bound = 2.0 * np.abs(map32.numpy().astype(np.float64) - map64.numpy()).mean() + 1e-6
    perm = np.random.default_rng(n).permutation(n)
    first, last = W // 2, n - (W - W // 3)                     # a range that starts and ends mid-row
    cases = {"idx partial": (perm[:n * 5 // 8], 0, n * 5 // 8), "idx full": (perm, 0, n),
             "idx empty": (np.zeros(1, np.int64), 0, 0), "range partial": (None, first, last - first),
             "range full": (None, 0, n), "range empty": (None, n, 0)}
    for label, (idx, a, cnt) in cases.items():
        rows = idx[:cnt] if idx is not None else np.arange(a, a + cnt)
        kw = dict(idx=idx, first=a, n=cnt)
        out, gy, rec = _mse_grad(y, t, H, W, O, win, cov, L, lam, **kw)
        l64, m64, s64, g64 = gref.ssim_mse_loss_and_grad(y, t, rows, lam, H, W, O, win, cov, L)
        _, _, _, g32 = gref.ssim_mse_loss_and_grad(y, t, rows, lam, H, W, O, win, cov, L, torch.float32)
        tag = f"ssim_mse_grad {kind} lam={lam:g} {label}"
        assert not (gy == FILL).any() and not (out == FILL).any()
        mask = np.zeros(n, bool)
        mask[rows] = True
        assert rec[mask].tobytes() == y[mask].tobytes() and (rec[~mask] == FILL).all()
        print(f"{tag}: parts {out}  fp64 {l64:.7e} {m64:.7e} {s64:.7e}")
        assert abs(float(out[1]) - m64) <= 1e-5 * m64 and (len(rows) > 0 or out[1] == 0.0)
        if lam == 0.0:
            assert out[2] == 0.0 and out[0] == out[1] and not gy[~mask].any()
        else:
            assert abs(float(out[2]) - s64) <= ssim_bound
            assert out[0] == np.float32(out[1] + np.float32(np.float32(lam) * np.float32(np.float32(1.0) - out[2])))
        scale = np.abs(g64).max()
        if scale > 0:
            eb, er = np.abs(gy - g64).max() / scale, np.abs(g32 - g64).max() / scale
            print(f"{tag}: g_y err_build {eb:.3e}  err_ref {er:.3e}")
            within_ref(eb, er, tag + " g_y")
        else:
            assert not gy.any()
        again = _mse_grad(y, t, H, W, O, win, cov, L, lam, **kw)
        assert all(p.tobytes() == q.tobytes() for p, q in zip((out, gy, rec), again))


# ---------------------------------------------------------------------------------------------------------------
# functional.ssim_loss
# ---------------------------------------------------------------------------------------------------------------
def test_ssim_loss_value_gradient_and_shapes():
    """The value is 1 - functional.ssim to one fp32 rounding; rec.grad is wire_ssim_bwd's output for the upstream gradient
    -1 (and -3 for 3 * loss), bit for bit; [H*W, O], [1, H*W, O] and [H, W, O] give the same bytes; the target gets no
    gradient; a second-order request raises."""
    from wire_amd import functional
    H, W, O = 40, 37, 3
    gt, rec = ref.inputs((H, W, O), 0.1)
    for kind in ("gaussian", "uniform"):
        win, cov = ref.window(kind)
        L = ref.DATA_RANGE[kind]
        kw = dict(window=kind, data_range=None if kind == "gaussian" else L)
        g = torch.tensor(gt, device=DEV).reshape(H * W, O)
        got = {}
        for shape in ((H * W, O), (1, H * W, O), (H, W, O)):
            r = torch.tensor(rec, device=DEV).reshape(shape).requires_grad_(True)
            loss = functional.ssim_loss(r, g, H, W, **kw)
            assert loss.shape == () and loss.is_cuda and loss.dtype == torch.float32 and loss.requires_grad
            s = functional.ssim(r, g, H, W, **kw)
            assert not s.requires_grad
            assert loss.item() == np.float32(1.0) - np.float32(s.item())
            loss.backward()
            assert r.grad.shape == shape
            got[shape] = (loss.detach().cpu().numpy().tobytes(), r.grad.cpu().numpy().tobytes())
        assert len(set(got.values())) == 1
        assert got[(H, W, O)][1] == _bwd(gt, rec, win, cov, L, up=-1.0).tobytes()
        r = torch.tensor(rec, device=DEV).requires_grad_(True)
        gg = g.clone().requires_grad_(True)
        (3.0 * functional.ssim_loss(r, gg, H, W, **kw)).backward()
        assert gg.grad is None
        assert r.grad.cpu().numpy().tobytes() == _bwd(gt, rec, win, cov, L, up=-3.0).tobytes()
        r = torch.tensor(rec, device=DEV).requires_grad_(True)
        with pytest.raises(NotImplementedError, match="first order"):
            torch.autograd.grad(functional.ssim_loss(r, g, H, W, **kw), r, create_graph=True)
        with torch.no_grad():
            quiet = functional.ssim_loss(r, g, H, W, **kw)
        assert not quiet.requires_grad


def test_ssim_loss_backward_reaches_the_parameters():
    """mse + 0.1 * ssim_loss on a small wire net's output: every parameter receives a finite gradient, and it is the
    gradient torch computes when the same g_y (wire_ssim_bwd's, plus the MSE's) is fed to the net's output."""
    from wire_amd import functional
    from wire_amd.modules import models
    H, W, O = 20, 13, 3
    gt, _ = ref.inputs((H, W, O), 0.1)
    torch.manual_seed(0)
    model = models.get_INR(nonlin="wire", in_features=2, out_features=O, hidden_features=32, hidden_layers=1).to(DEV)
    coords = torch.tensor(_grid_coords(H, W), device=DEV)
    target = torch.tensor(gt, device=DEV).reshape(H * W, O)
    y = model(coords)
    loss = ((y - target) ** 2).mean() + 0.1 * functional.ssim_loss(y, target, H, W)
    model.zero_grad()
    loss.backward()
    got = [p.grad.clone() for p in model.parameters() if p.requires_grad]
    assert got and all(g is not None and torch.isfinite(torch.view_as_real(g) if g.is_complex() else g).all() for g in got)
    assert any(g.abs().max() > 0 for g in got)
    win, cov = ref.window("gaussian")
    yd = y.detach()
    gy = 2.0 * (yd - target) / (H * W * O) + \
        0.1 * torch.tensor(_bwd(gt, yd.cpu().numpy().reshape(H, W, O), win, cov, 1.0, up=-1.0), device=DEV).reshape(H * W, O)
    model.zero_grad()
    model(coords).backward(gy)
    for a, p in zip(got, [p for p in model.parameters() if p.requires_grad]):
        assert relmax(torch.view_as_real(a).cpu().numpy() if a.is_complex() else a.cpu().numpy(),
                      torch.view_as_real(p.grad).cpu().numpy() if a.is_complex() else p.grad.cpu().numpy()) <= 1e-5


# ---------------------------------------------------------------------------------------------------------------
# FusedTrainer.step_ssim
# ---------------------------------------------------------------------------------------------------------------
LAM = 0.1


def _net(kind, O):
    from wire_amd.modules import models
    torch.manual_seed(0)
    hp = (7.0, 7.0, 6.0) if kind == "wire" else (30.0, 30.0, 10.0)
    m = models.get_INR(nonlin=kind, in_features=2, out_features=O, hidden_features=128, hidden_layers=2,
                       first_omega_0=hp[0], hidden_omega_0=hp[1], scale=hp[2])
    return m.to(DEV), hp


def _tensors(model, tr):
    names = [k for k in model.state_dict().keys() if "omega_0" not in k and "scale_0" not in k]
    assert len(names) == len(tr.offsets)
    return list(zip(names, tr.offsets))


class _Case:
    """An lr = 0 trainer on an (H, W) grid whose target is the SSIM tests' image; the oracles run on the coordinates the
    trainer builds, and their g_y is autograd's of mse + lam (1 - ssim) on their own forward."""

    def __init__(self, kind, H, W, O, keep_rec=False, lr=0.0):
        from wire_amd.trainer import FusedTrainer
        self.kind, self.H, self.W, self.O, self.n = kind, H, W, O, H * W
        self.model, self.hp = _net(kind, O)
        self.target = ref.inputs((H, W, O), 0.1)[0].reshape(self.n, O)
        self.tr = FusedTrainer(self.model, (H, W), torch.tensor(self.target), lr=lr, keep_rec=keep_rec)

    def step(self, lam, **kw):
        loss = self.tr.step_ssim(lam, **kw)
        torch.cuda.synchronize()
        self.y = self.tr.y[:self.n * self.O].cpu().numpy().reshape(self.n, self.O).copy()
        self.parts = self.tr.loss_parts.cpu().numpy().copy()
        return float(loss.item()), self.tr.flat_grad.cpu().numpy().copy()

    def oracle(self, lam, rows, double, window="gaussian"):
        dt = np.float64 if double else np.float32
        p = wo.cast_params(params_np(self.model), double)
        a = tuple(dt(v) for v in self.hp)
        x = self.tr.coords[:self.n * 2].reshape(self.n, 2).cpu().numpy().astype(dt)
        if self.kind == "wire":
            y, cache = wo.wire_forward(p, x, 2, *a, keep=True)
        else:
            y, cache = wo.realnet_forward(self.kind, p, x, 2, *a, None, keep=True)
        win, cov = ref.window(window)
        loss, mse, ssim, gy = gref.ssim_mse_loss_and_grad(y, self.target, rows, lam, self.H, self.W, self.O, win, cov,
                                                          ref.DATA_RANGE[window],
                                                          torch.float64 if double else torch.float32)
        gy = gy.reshape(y.shape).astype(dt)
        g = wo.wire_backward(p, cache, gy, 2, *a) if self.kind == "wire" else \
            wo.realnet_backward(self.kind, p, cache, gy, 2, *a)
        return float(loss), g, (float(mse), float(ssim))


def _assert_bf16_bounds(c, loss, flat, l64, g64, label):
    """Loss 2e-5 relative, every gradient 5e-5 max|g| + 1e-10: the bounds of the step_tv tests on the 3 x bf16 family."""
    for name, off in _tensors(c.model, c.tr):
        g = wo.as_real_pairs(g64[name]).astype(np.float64).ravel()
        print(f"{label}: {name} err / max|g| {np.abs(flat[off:off + g.size] - g).max() / np.abs(g).max():.2e}")
    print(f"{label}: loss {loss:.6e} rel {abs(loss - l64) / l64:.2e}")
    assert abs(loss - l64) <= 2e-5 * l64
    for name, off in _tensors(c.model, c.tr):
        g = wo.as_real_pairs(g64[name]).astype(np.float64).ravel()
        assert np.abs(flat[off:off + g.size] - g).max() <= 5e-5 * np.abs(g).max() + 1e-10, name


@pytest.mark.parametrize("H,W", [(20, 13), (40, 37)])
def test_step_ssim_bf16_family_matches_oracle(H, W):
    """wire 2 x 128 on 20 x 13 (one tile of the loss kernel, 10 x 3 windows) and 40 x 37 (3 x 2 tiles), O = 3, the
    3 x bf16 family: all rows, indices = a slice of a permutation, and a range, at the step_tv tests' bounds; loss_parts
    consistent with the loss (the mse part 2e-5 relative, the index 2e-5 of its unit range: the loss's own bound applied
    to each part); with keep_rec the selected rows of self.y go to self.rec."""
    c = _Case("wire", H, W, 3, keep_rec=True)
    perm = np.random.default_rng(8).permutation(c.n)
    k = c.n * 5 // 8
    for label, rows, kw in (("all rows", np.arange(c.n), {}),
                            ("perm slice", perm[:k], dict(indices=torch.tensor(perm[:k], device=DEV))),
                            ("range", np.arange(W // 2, c.n - W // 3), dict(first=W // 2, count=c.n - W // 3 - W // 2))):
        c.tr.rec.fill_(FILL)
        loss, flat = c.step(LAM, **kw)
        l64, g64, (m64, s64) = c.oracle(LAM, rows, True)
        _assert_bf16_bounds(c, loss, flat, l64, g64, f"step_ssim {H}x{W} {label}")
        assert np.abs(flat).max() > 0
        assert c.parts[0] == np.float32(loss) == \
            np.float32(c.parts[1] + np.float32(np.float32(LAM) * np.float32(np.float32(1.0) - c.parts[2])))
        assert abs(c.parts[1] - m64) <= 2e-5 * m64 and abs(c.parts[2] - s64) <= 2e-5
        rec = c.tr.rec.cpu().numpy()
        sel = np.zeros(c.n, bool)
        sel[rows] = True
        assert rec[sel].tobytes() == c.y[sel].tobytes() and (rec[~sel] == FILL).all()
    # the uniform window with its data range
    loss, flat = c.step(LAM, window="uniform", data_range=2.0)
    l64, g64, _ = c.oracle(LAM, np.arange(c.n), True, window="uniform")
    _assert_bf16_bounds(c, loss, flat, l64, g64, f"step_ssim {H}x{W} uniform window")


@pytest.mark.parametrize("kind", ["wire", "siren"])
def test_step_ssim_fp16_family_within_reference_error(kind):
    """72 x 64, O = 3 (4 608 rows, above the 4 096-row switch to the 2 x fp16 family): loss and every gradient within
    3 x the error of the reference's own fp32 arithmetic (the fp32 oracle against fp64) + 1e-6, as the step_tv test."""
    c = _Case(kind, 72, 64, 3)
    loss, flat = c.step(LAM)
    rows = np.arange(c.n)
    l64, g64, _ = c.oracle(LAM, rows, True)
    l32, g32, _ = c.oracle(LAM, rows, False)
    checks = [(f"step_ssim {kind} loss", abs(loss - l64) / l64, abs(l32 - l64) / l64)]
    for name, off in _tensors(c.model, c.tr):
        g = wo.as_real_pairs(g64[name]).astype(np.float64).ravel()
        r = wo.as_real_pairs(g32[name]).astype(np.float64).ravel()
        checks.append((f"step_ssim {kind} {name}", relmax(flat[off:off + g.size], g), relmax(r, g)))
    for label, eb, er in checks:
        print(f"{label}: err_build {eb:.3e}  err_ref {er:.3e}  ratio {eb / er if er > 0 else float('inf'):.2f}")
    for label, eb, er in checks:
        within_ref(eb, er, label, factor=3.0)


def test_step_ssim_zero_lambda_is_step_tv_zero():
    """step_ssim(0.0, ...) leaves the parameters torch.equal to those step_tv(0.0, ...) leaves with the same arguments:
    two steps each of all rows, an index list and a range, on trainers built from the same seed; the index is not
    evaluated (loss_parts[2] == 0, loss == mse)."""
    H, W = 40, 37
    perm = torch.tensor(np.random.default_rng(3).permutation(H * W)[:700], device=DEV)
    for kw in ({}, dict(indices=perm), dict(first=50, count=900)):
        a, b = _Case("wire", H, W, 3, lr=5e-3), _Case("wire", H, W, 3, lr=5e-3)
        assert torch.equal(a.tr.flat, b.tr.flat)
        p0 = a.tr.flat.clone()
        for _ in range(2):
            la, lb = a.tr.step_ssim(0.0, **kw), b.tr.step_tv(0.0, **kw)
        torch.cuda.synchronize()
        assert torch.equal(a.tr.flat, b.tr.flat) and not torch.equal(a.tr.flat, p0)
        assert torch.equal(a.tr.flat_grad, b.tr.flat_grad)
        parts = a.tr.loss_parts.cpu().numpy()
        assert parts[2] == 0.0 and parts[0] == parts[1]
        assert abs(float(la) - float(lb)) <= 1e-6 * float(lb)


def test_step_ssim_hier_with_stage_rates():
    """A bspline_mscale_hier trainer with one rate per stage takes a step, and its gradients (of the parameters before the
    step) meet the bf16 family's bounds against the fp64 closed form of tests/hier_ref.py -- driven with the
    pseudo-target t' = y64 - g_y H W O / 2, for which its MSE gradient 2 (y64 - t') / (H W O) is the regularised g_y."""
    from wire_amd.modules import models
    from wire_amd.trainer import FusedTrainer
    H, W, O, st, L = 24, 20, 3, [1 / 9, 4.0], 2
    n = H * W
    torch.manual_seed(0)
    model = models.get_INR(nonlin="bspline_mscale_hier", in_features=2, out_features=O, hidden_features=64,
                           scaled_hidden_features=0, hidden_layers=L, first_omega_0=-0.2, hidden_omega_0=-0.2,
                           scale=0.0, scale_tensor=st).to(DEV)
    target = ref.inputs((H, W, O), 0.1)[0].reshape(n, O)
    tr = FusedTrainer(model, (H, W), torch.tensor(target), lr=[6e-3, 2e-2], niters=100)
    sd = _sd(model)
    heads = {}
    for s, lin in enumerate(model.linears):
        heads[f"linears.{s}.weight"] = lin.weight.detach().cpu().numpy().copy()
        heads[f"linears.{s}.bias"] = lin.bias.detach().cpu().numpy().copy()
    names = [k for k in sd if "scale_0" not in k] + list(heads)
    p0 = tr.flat.clone()
    loss = float(tr.step_ssim(LAM).item())
    torch.cuda.synchronize()
    assert not torch.equal(tr.flat, p0)                                   # both stages and their heads moved
    x = tr.coords[:n * 2].reshape(n, 2).cpu().numpy().astype(np.float64)
    y64 = hr.forward(sd, heads, L, x, st, np.float64)
    win, cov = ref.window("gaussian")
    l64, _, _, gy = gref.ssim_mse_loss_and_grad(y64, target, np.arange(n), LAM, H, W, O, win, cov, 1.0)
    pseudo = y64 - gy * (n * O / 2.0)
    _, _, g64, _ = hr.loss_and_grads(sd, heads, L, x, pseudo, st, np.float64)
    flat = tr.flat_grad.cpu().numpy()
    print(f"step_ssim hier: loss {loss:.6e} rel {abs(loss - l64) / l64:.2e}")
    assert abs(loss - l64) <= 2e-5 * l64
    assert len(names) == len(tr.offsets)
    for k, off, sz in zip(names, tr.offsets, tr.sizes):
        g = g64[k].ravel()
        print(f"step_ssim hier: {k} err / max|g| {np.abs(flat[off:off + sz] - g).max() / np.abs(g).max():.2e}")
    for k, off, sz in zip(names, tr.offsets, tr.sizes):
        g = g64[k].ravel()
        assert np.abs(flat[off:off + sz] - g).max() <= 5e-5 * np.abs(g).max() + 1e-10, k


def test_step_ssim_refusals():
    """A 3-D grid, a trainer built with target=None, a grid smaller than the window and a non-finite lambda_ssim raise
    ValueError naming the argument (world > 1 is checked on the host, tests/test_ssim_loss_host.py); an empty range is
    legal: the SSIM term alone."""
    from wire_amd.modules import models
    from wire_amd.trainer import FusedTrainer
    m3 = models.get_INR(nonlin="wire", in_features=3, out_features=1, hidden_features=32, hidden_layers=1).to(DEV)
    with pytest.raises(ValueError, match="2-D grid"):
        FusedTrainer(m3, (4, 5, 6), torch.zeros(120, 1)).step_ssim(0.1)
    m2 = lambda: models.get_INR(nonlin="wire", in_features=2, out_features=1, hidden_features=32, hidden_layers=1).to(DEV)
    with pytest.raises(ValueError, match="target"):
        FusedTrainer(m2(), (14, 15), None).step_ssim(0.1)
    with pytest.raises(ValueError, match="smaller than"):
        FusedTrainer(m2(), (10, 15), torch.zeros(150, 1)).step_ssim(0.1)
    tr = FusedTrainer(m2(), (14, 15), torch.rand(210, 1))
    for bad in (float("nan"), float("inf")):
        with pytest.raises(ValueError, match="lambda_ssim"):
            tr.step_ssim(bad)
    with pytest.raises(ValueError, match="outside the grid"):
        tr.step_ssim(0.1, first=209, count=3)
    t0 = tr.t
    tr.step_ssim(0.1, first=210, count=0)
    torch.cuda.synchronize()
    parts = tr.loss_parts.cpu().numpy()
    assert tr.t == t0 + 1 and parts[1] == 0.0 and -1.0 <= parts[2] <= 1.0 and parts[2] != 0.0
