"""Results do not depend on what the caller's workspaces held before the call (include/wire_hip.h, "Workspaces").

Every call of the C ABI works in buffers the caller allocates -- ``packed``, ``act``, ``scratch`` and ``partial`` of the
whole-net calls, the ``ws`` of the per-layer, combiner, filter and SSIM calls, the ``partial`` of the loss and metric
kernels -- and the library must define every byte it later reads: tail rows of a 128-row tile, pad columns, slabs of
unused splits, maximum slots, partials beyond the number of blocks.  The rest of the suite allocates with ``torch.empty``
and cannot see a violation.  Here every call runs with its workspaces filled by tests/workspace_fill.py: ZERO twice (the
same call gives the same bits), then ONES (NaN, the largest unsigned), BIG (2^127: survives fmaxf and relu) and STALE (the
leftovers of a previous, larger call on the other GEMM family) must reproduce the ZERO run BIT FOR BIT.  Outputs are
prefilled with NaN; inputs, weights, targets and indices are never touched.  The accuracy of the ZERO run against fp64 is
the business of the other test files.

The one exception is step_radon, whose adjoint adds with float atomics: see test_step_radon."""
import ctypes as C

import numpy as np
import pytest
import torch

import dispatch_cases as dc
import workspace_fill as wf
from _util import _coords, tune
from workspace_fill import PATTERNS, STALE, STALE_GAIN, ZERO, check_patterns, fill, fill_all, nan_like

pytestmark = pytest.mark.gpu
DEV = "cuda"
GRID = (72, 64)                                   # 4608 points
NPTS = GRID[0] * GRID[1]
# 4133 = 32 x 128 + 37: above the 4096-row line of the 2 x fp16 family, a 37-row last tile, a ragged 256-row split;
# 4096: at the line; 1000 = 7 x 128 + 104: below it; 129: one tile and one row
ROWS = (4133, 4096, 1000, 129)
O = dc.OUT


class _Data:
    """Targets and the permutation of the grid, made once."""
    _d = None

    @classmethod
    def get(cls):
        if cls._d is None:
            g = torch.Generator().manual_seed(11)
            target = torch.rand(NPTS, O, generator=g)
            perm = torch.randperm(NPTS, generator=g).to(DEV)
            cls._d = (target, perm)
        return cls._d


def _collect(failures, fn):
    try:
        fn()
    except AssertionError as e:
        failures.append(str(e))


def _step_rows(case, label, rows=ROWS):
    """FusedTrainer.step on perm[:n] for every n of ``rows`` under the four patterns; the STALE call is the step on the
    whole grid."""
    _, perm = _Data.get()
    failures = []
    for n in rows:
        idx = perm[:n].contiguous()
        step = lambda tr: tr.step(idx)
        outs = lambda tr: dict(rec=tr.rec, flat_grad=tr.flat_grad, y=tr.y[:n * tr.O])
        _collect(failures, lambda: check_patterns(lambda p: case.run(step, outs, p),
                                                  lambda: case.stale(lambda tr: tr.step(perm)), f"{label} n={n}"))
    assert not failures, "\n".join(failures)


# ---- (a) the training step on every route ----------------------------------------------------------------------------
ROUTES = sorted({(kind, hf, k) for kind in dc.KINDS for cid, hf, n, kv in dc.case_ids(kind)
                 for k in [cid.rsplit("/", 1)[1]]})
ALL_KNOBS = dict(dc.KNOBS, **dc.WIRE_KNOBS)


@pytest.mark.parametrize("kind,hf,knob", ROUTES, ids=[f"{k}-hf{h}-{kn}" for k, h, kn in ROUTES])
def test_train_step(kind, hf, knob):
    """Every net kind, width and GEMM-family knob of tests/dispatch_cases.py at 4133, 4096, 1000 and 129 rows of a
    72 x 64 grid: loss, rec, flat_grad and y."""
    target, _ = _Data.get()
    case = wf.TrainerCase(dc.model_of(kind, hf), GRID, target, ALL_KNOBS[knob])
    _step_rows(case, f"step {kind} hf{hf} {knob}")


def test_the_patterns_reach_the_call():
    """Negative control of this file's method: with the workspaces' own words counted among the outputs -- ``partial``, of
    whose 4096 floats a step writes a few, and ``act``, reserved for 4608 rows and used for 129 -- the comparison must
    object under every pattern, and must still find ZERO twice identical.  If it did not, the fills would not be in place
    when the call runs and every other test here would pass vacuously."""
    target, perm = _Data.get()
    case = wf.TrainerCase(dc.model_of("siren", 64), GRID, target, {})
    idx = perm[:129].contiguous()
    words = case.tr.act.numel() // 4 * 4
    outs = lambda tr: dict(flat_grad=tr.flat_grad, partial=tr.partial, act=tr.act[:words].view(torch.float32))
    with pytest.raises(AssertionError) as e:
        check_patterns(lambda p: case.run(lambda tr: tr.step(idx), outs, p), lambda: case.stale(lambda tr: tr.step(perm)),
                       "control")
    msg = str(e.value)
    assert "ONES: partial" in msg and "BIG: partial" in msg and "STALE: " in msg and "ZERO twice" not in msg, msg


# ---- (b) the scaled and multi-pass kinds -----------------------------------------------------------------------------
def _scaled_model(kind, K):
    """The smallest configuration of the kind's own GPU test file (test_gpu_mscale_hl / _mscale2 / _hier)."""
    from wire_amd.modules import models
    torch.manual_seed(0)
    shf, st, s = {"bspline_mscale_HL": (130, [1.0, 2.0], 1.0), "bspline_mscale_2": (0, [1 / 9, 4.0], 0.0),
                  "bspline_mscale_hier": (0, [1 / 9, 4.0], 0.0)}[kind]
    return models.get_INR(nonlin=kind, in_features=2, out_features=O, hidden_features=K, scaled_hidden_features=shf,
                          hidden_layers=2, first_omega_0=-0.2, hidden_omega_0=-0.2, scale=s,
                          scale_tensor=torch.tensor(st).to(DEV)).to(DEV)


SCALED = ("bspline_mscale_HL", "bspline_mscale_2", "bspline_mscale_hier")


@pytest.mark.parametrize("knob", list(dc.KNOBS))
@pytest.mark.parametrize("K", [256, 64])
@pytest.mark.parametrize("kind", SCALED)
def test_train_step_scaled_kinds(kind, K, knob):
    """bspline_mscale_HL (its frozen first stage's gradient slices are left alone), bspline_mscale_2 (S n rows and the
    extra tile of the chain) and bspline_mscale_hier (the joined layers' weight maxima): width 256 takes the whole-net
    route, 64 goes layer by layer."""
    target, _ = _Data.get()
    case = wf.TrainerCase(_scaled_model(kind, K), GRID, target, dc.KNOBS[knob])
    _step_rows(case, f"step {kind} K{K} {knob}", rows=(4133, 1000))


# ---- (c) the other steps --------------------------------------------------------------------------------------------
def _net(kind, D, Oo, hf=128):
    from wire_amd.modules import models
    torch.manual_seed(0)
    hp = (7.0, 7.0, 6.0) if kind == "wire" else (30.0, 30.0, 10.0)
    return models.get_INR(nonlin=kind, in_features=D, out_features=Oo, hidden_features=hf, hidden_layers=2,
                          first_omega_0=hp[0], hidden_omega_0=hp[1], scale=hp[2]).to(DEV)


def _full_grid_outputs(n, extra=None):
    def outs(tr):
        d = dict(flat_grad=tr.flat_grad, y=tr.y[:n * tr.O])
        d.update(extra(tr) if extra else {})
        return d
    return outs


def _check_step(case, label, step, stale_step, outs):
    check_patterns(lambda p: case.run(step, outs, p), lambda: case.stale(stale_step), label)


def _rand(shape, seed):
    return torch.tensor(np.random.default_rng(seed).uniform(0, 1, shape).astype(np.float32), device=DEV)


@pytest.mark.parametrize("kind", ["wire", "siren"])
@pytest.mark.parametrize("H,W,scale", [(26, 21, 4), (74, 67, 4)])
def test_step_downsampled(H, W, scale, kind):
    """546 rows (the shape of test_super_resolution_step_matches_oracle) and 4958: both have ragged borders on both axes,
    which take the memset path of wire_avgpool_mse_grad."""
    case = wf.TrainerCase(_net(kind, 2, 3), (H, W), None, {}, keep_rec=False)
    gt = _rand(((H // scale) * (W // scale), 3), 3)
    rec = nan_like(gt.shape)

    def step(tr):
        rec.fill_(float("nan"))
        return tr.step_downsampled(gt, scale, rec_lr=rec)
    _check_step(case, f"step_downsampled {kind} {H}x{W}/{scale}", step,
                lambda tr: tr.step_downsampled(gt * STALE_GAIN, scale), _full_grid_outputs(H * W, lambda tr: dict(rec_lr=rec)))


def _frames_case(kind, B, H, W, scale, Oo):
    from multi_sr_ref import make_mask
    case = wf.TrainerCase(_net(kind, 2, Oo), (H, W), None, {}, keep_rec=False, reserve=B * H * W)
    rng = np.random.default_rng(5)
    th, sh = [0.0, np.pi / 10, -np.pi / 12][:B], [(0, 0), (3, -2), (-4, 1)][:B]
    mats = np.array([[[np.cos(a), -np.sin(a), dx], [np.sin(a), np.cos(a), dy]] for a, (dx, dy) in zip(th, sh)])
    coords = case.tr.affine_coords(mats)
    H2, W2 = H // scale, W // scale
    gt = torch.tensor(rng.uniform(0, 1, (B, H2 * W2, Oo)).astype(np.float32), device=DEV)
    mask = torch.tensor(np.asarray(make_mask(rng, B, H2 * W2, Oo), np.float32), device=DEV).reshape(B, H2 * W2, Oo).clone()
    mask[B - 1] = 0.0                                      # an all-zero frame
    return case, coords, gt, mask


def _check_frames(case, label, coords, gt, mask, scale, stale_args):
    B = coords.shape[0]
    rec = nan_like(gt.shape)

    def step(tr):
        rec.fill_(float("nan"))
        return tr.step_frames(coords, gt, scale, mask=mask, rec_lr=rec)
    sc, sg, sm = stale_args
    _check_step(case, label, step, lambda tr: tr.step_frames(sc, sg * STALE_GAIN, scale, mask=sm),
                _full_grid_outputs(B * coords.shape[1], lambda tr: dict(rec_lr=rec)))


@pytest.mark.parametrize("kind", ["wire", "siren"])
@pytest.mark.parametrize("B,H,W,scale", [(3, 26, 21, 4), (2, 50, 49, 4)])
def test_step_frames_lds_path(B, H, W, scale, kind):
    """1638 rows (the shape of test_step_frames_bf16_family_matches_oracle) and 4900, O = 3, the last frame's mask all
    zero.  Then that frame ALONE, as a smaller last batch: every g_y is exactly zero, so is every g_lin, and the maximum
    slots of the 2 x fp16 operands stay 0."""
    case, coords, gt, mask = _frames_case(kind, B, H, W, scale, 3)
    failures = []
    _collect(failures, lambda: _check_frames(case, f"step_frames {kind} B={B} {H}x{W}/{scale}", coords, gt, mask, scale,
                                             (coords, gt, torch.ones_like(mask))))
    last = slice(B - 1, B)
    _collect(failures, lambda: _check_frames(case, f"step_frames {kind} zero frame alone {H}x{W}/{scale}",
                                             coords[last].contiguous(), gt[last].contiguous(), mask[last].contiguous(),
                                             scale, (coords, gt, torch.ones_like(mask))))
    assert not failures, "\n".join(failures)


@pytest.mark.parametrize("kind", ["wire", "siren"])
def test_step_frames_direct_path(kind):
    """scale O = 129 x 8 = 1032 > 1024 floats per pooled row: the direct path of wire_avgpool_mse_grad_frames; 2 frames
    of 130 x 129 (33 540 rows), the second one's mask all zero."""
    case, coords, gt, mask = _frames_case(kind, 2, 130, 129, 129, 8)
    _check_frames(case, f"step_frames {kind} direct path", coords, gt, mask, 129, (coords, gt, torch.ones_like(mask)))


@pytest.mark.parametrize("kind", ["wire", "siren"])
@pytest.mark.parametrize("H,W,T,Oo,nframes", [(12, 10, 9, 1, 4), (24, 24, 8, 3, 4)])
def test_step_coded(H, W, T, Oo, nframes, kind):
    """1080 rows with a ragged last group of one frame, and 4608 rows (the shapes of test_gpu_video_cs.py)."""
    from video_cs_ref import make_mask
    case = wf.TrainerCase(_net(kind, 3, Oo), (H, W, T), None, {}, keep_rec=False)
    rng = np.random.default_rng(11)
    NP, Cp = H * W, (T + nframes - 1) // nframes + 1
    gt = torch.tensor(rng.uniform(0, 1, (Cp, NP, Oo)).astype(np.float32), device=DEV)
    mask = torch.tensor(np.asarray(make_mask(rng, NP, T), np.float32).reshape(-1), device=DEV)
    est = nan_like(gt.shape)

    def step(tr):
        est.fill_(float("nan"))
        return tr.step_coded(gt, mask, nframes, est=est)
    _check_step(case, f"step_coded {kind} {H}x{W}x{T}", step, lambda tr: tr.step_coded(gt * STALE_GAIN, mask, nframes),
                _full_grid_outputs(NP * T, lambda tr: dict(est=est)))


@pytest.mark.parametrize("kind", ["wire", "siren"])
@pytest.mark.parametrize("H,W", [(24, 20), (72, 64)])
def test_step_tv(H, W, kind):
    """480 and 4608 rows (the shapes of test_gpu_tv.py), lambda 2^-14; the MSE over a ragged slice of a permutation (the
    two-launch path of wire_tv_mse_grad), then over a row range (the one-pass path)."""
    n = H * W
    g = torch.Generator().manual_seed(21)
    case = wf.TrainerCase(_net(kind, 2, 3), (H, W), torch.rand(n, 3, generator=g), {})
    idx = torch.randperm(n, generator=g)[:n - n // 3 - 1].to(DEV).contiguous()
    lam = 2.0 ** -14
    outs = _full_grid_outputs(n, lambda tr: dict(rec=tr.rec, loss_parts=tr.loss_parts))
    failures = []
    for tag, kw in (("indices", dict(indices=idx)), ("range", dict(first=n // 5, count=n // 2 + 1))):
        _collect(failures, lambda: _check_step(case, f"step_tv {kind} {H}x{W} {tag}", lambda tr: tr.step_tv(lam, **kw),
                                               lambda tr: tr.step_tv(lam * 8), outs))
    assert not failures, "\n".join(failures)


RADON_BOUND = 1e-5     # twice the 5e-6 that test_device_radon_adjoint grants each run of the adjoint against fp64


def _relmax(a, b):
    d, s = (a.double() - b.double()).abs().max().item(), b.double().abs().max().item()
    return d / s if s > 0 else d


@pytest.mark.parametrize("kind", ["wire", "siren"])
@pytest.mark.parametrize("H,W", [(24, 30), (72, 64)])
def test_step_radon(H, W, kind):
    """720 rows (the shape of test_ct_driver_loop_and_fused_step) and 4608, 17 angles.  wire_radon_bwd adds with float
    atomics, so bit identity does not hold for this step: every output finite and max|a - b| / max|b| <= 1e-5 against the
    ZERO run.  The two ZERO runs are held to the same bound first: if THEY differ by more, the bound is wrong, not the
    kernel, and the patterns are not judged."""
    A = 17
    case = wf.TrainerCase(_net(kind, 2, 1), (H, W), None, {}, keep_rec=False)
    tr = case.tr
    th = torch.linspace(0, 180, A)
    sino = _rand((A * W,), 7) * H
    tr.step_radon(sino, th)                                             # allocates the sinogram buffers
    case._after()
    case.bufs.update(sino=tr._sino, gsino=tr._gsino)
    step = lambda t: t.step_radon(sino, th)
    outs = _full_grid_outputs(H * W)
    base = case.run(step, outs, ZERO)
    again = case.run(step, outs, ZERO)
    spread = {k: _relmax(again[k], base[k]) for k in base}
    print(f"step_radon {kind} {H}x{W}: ZERO twice, relmax {spread}")
    assert all(torch.isfinite(v).all() for v in base.values())
    assert max(spread.values()) <= RADON_BOUND, f"two ZERO runs differ by {spread}: the bound is wrong, not the kernel"
    bad = []
    for p in PATTERNS[1:]:
        if p == STALE:
            case.stale(lambda t: t.step_radon(sino * STALE_GAIN, th))
        got = case.run(step, outs, p)
        err = {k: _relmax(got[k], base[k]) if torch.isfinite(got[k]).all() else float("inf") for k in base}
        print(f"step_radon {kind} {H}x{W}: {p} against ZERO, relmax {err}")
        bad += [f"{p} {k}: {e:.3e}" for k, e in err.items() if not e <= RADON_BOUND]
    assert not bad, f"step_radon {kind} {H}x{W}: " + "; ".join(bad)


# ---- (d) the forward and autograd paths through ctypes ---------------------------------------------------------------
# functional.py allocates inside the call, so these run what it runs (wire_amd/functional.py: _INRFunction) on buffers
# the test owns -- reserved for the whole 4608-row grid, as a trainer's are, and used for n rows.
ABI_NETS = [(k, hf) for k in dc.KINDS for hf in dc.WIDTHS.get(k, (256, 64))] + [(k, K) for k in SCALED for K in (256, 64)]


def _abi_model(kind, hf):
    return _scaled_model(kind, hf) if kind in SCALED else dc.model_of(kind, hf)


@pytest.mark.parametrize("kind,hf", ABI_NETS, ids=[f"{k}-hf{h}" for k, h in ABI_NETS])
def test_abi_forward_and_backward(kind, hf):
    """wire_mlp_fwd with save_for_bwd 0 and 1, wire_mlp_bwd, wire_mlp_bwd_coords with and without grads_host, at
    n = 4133 and 129.  Before each backward the scratch is filled again, so that none of them works in what the one
    before defined.  bspline_mscale_HL has no coordinate gradient (WIRE_ERR_ARG): its two wire_mlp_bwd_coords calls are
    left out."""
    with_coords = kind != "bspline_mscale_HL"
    net = wf.AbiNet(_abi_model(kind, hf), NPTS, with_coords)
    bufs = net.buffers()
    g = torch.Generator().manual_seed(3)
    x_all = torch.tensor(_coords(NPTS, 2), device=DEV)
    gy_all = (torch.randn(NPTS, O, generator=g) / NPTS).to(DEV)

    def calls(x, gy, pattern):
        out = {}
        net.pack()
        out["y_infer"] = net.fwd(x, 0)
        out["y"] = net.fwd(x, 1)
        out.update({"bwd." + k: v for k, v in net.bwd(x, gy).items()})
        if with_coords:
            for tag, wg in (("bwd_coords.", True), ("bwd_coords_only.", False)):
                if pattern != STALE:
                    fill(net.scratch, pattern)
                out.update({tag + k: v for k, v in net.bwd(x, gy, coords=True, with_grads=wg).items()})
        torch.cuda.synchronize()
        return out

    failures = []
    for n in (4133, 129):
        x, gy = x_all[:n].contiguous(), gy_all[:n].contiguous()

        def run(p):
            if p != STALE:
                fill_all(bufs, p)
            return calls(x, gy, p)

        def stale():
            with tune(**wf.other_family({})):
                calls(x_all, gy_all * STALE_GAIN, STALE)
        _collect(failures, lambda: check_patterns(run, stale, f"abi {kind} hf{hf} n={n}"))
    assert not failures, "\n".join(failures)


# ---- (e) calls with their own ws or partial --------------------------------------------------------------------------
class Out:
    """An output of an entry point: a fresh NaN tensor of this shape per call."""

    def __init__(self, name, *shape):
        self.name, self.shape = name, shape


WS, WSB = object(), object()                       # the workspace pointer and its size in bytes


def _call(fn, args, ws):
    from wire_amd import _lib
    L = _lib.lib()
    outs, a = {}, []
    for v in args:
        if isinstance(v, Out):
            outs[v.name] = nan_like(v.shape)
            a.append(outs[v.name].data_ptr())
        elif isinstance(v, torch.Tensor):
            a.append(v.data_ptr())
        elif v is WS:
            a.append(ws.data_ptr())
        elif v is WSB:
            a.append(ws.numel() * ws.element_size())
        else:
            a.append(v)
    _lib.check(getattr(L, fn)(torch.cuda.current_stream().cuda_stream, *a), fn)
    torch.cuda.synchronize()
    return outs


def _check_entry(label, fn, args, ws, stale=None):
    """``args``: the call; ``stale``: (fn, args) of the previous call in the same workspace (default: the same call), made
    on the other GEMM family."""
    def run(p):
        if p != STALE:
            fill(ws, p)
        return _call(fn, args, ws)

    def prev():
        with tune(**wf.other_family({})):
            _call(*(stale or (fn, args)), ws)
    check_patterns(run, prev, label)


def _ws(nbytes):
    return torch.empty(int(nbytes), dtype=torch.uint8, device=DEV)


def _partial(floats):
    return torch.empty(int(floats), dtype=torch.float32, device=DEV)


def _rn(gen, *shape, scale=1.0):
    return (torch.randn(*shape, generator=gen) * scale).to(DEV).contiguous()


LAYER_SHAPES = [(4133, 101, 77), (129, 77, 101)]   # ragged n on either side of the 4096-row line, odd feature counts


@pytest.mark.parametrize("n,fin,fout", LAYER_SHAPES)
def test_gabor_layer_calls(n, fin, fout):
    """wire_gabor_fwd / _bwd / _hparam_grad, hidden (complex input) and first (real input, in = 3), and
    wire_gabor_bwd_first_coords."""
    from wire_amd import _lib
    L = _lib.lib()
    g = torch.Generator().manual_seed(n)
    om, sc = 7.0, 6.0
    failures = []
    for first in (0, 1):
        i = 3 if first else fin
        c = () if first else (2,)
        x, W, b = _rn(g, n, i, *c), _rn(g, fout, i, *c, scale=0.5 / i ** 0.5), _rn(g, fout, *c, scale=0.1)
        ga = _rn(g, n, fout, 2)
        ws = _ws(_lib.check(L.wire_layer_ws_bytes(n, i, fout)))
        tag = f"{'first' if first else 'hidden'} n={n} {i}->{fout}"
        lin = Out("lin", n, fout, *c)
        fwd = [x, W, b, om, sc, n, i, fout, first, lin, Out("act", n, fout, 2), WS, WSB]
        gx = None if first else Out("g_x", n, i, 2)
        bwd = lambda gain: [ga * gain, x, W, b, om, sc, n, i, fout, first, gx, Out("g_W", fout, i, *c),
                            Out("g_b", fout, *c), WS, WSB]
        hp = lambda gain: [ga * gain, x, W, b, om, sc, n, i, fout, first, Out("out2", 2), WS, WSB]
        _collect(failures, lambda: _check_entry(f"wire_gabor_fwd {tag}", "wire_gabor_fwd", fwd, ws,
                                                ("wire_gabor_bwd", bwd(STALE_GAIN))))
        _collect(failures, lambda: _check_entry(f"wire_gabor_bwd {tag}", "wire_gabor_bwd", bwd(1.0), ws,
                                                ("wire_gabor_bwd", bwd(STALE_GAIN))))
        _collect(failures, lambda: _check_entry(f"wire_gabor_hparam_grad {tag}", "wire_gabor_hparam_grad", hp(1.0), ws,
                                                ("wire_gabor_bwd", bwd(STALE_GAIN))))
        if first:
            fc = lambda gain, wg: [ga * gain, x, W, b, om, sc, n, i, fout, Out("g_x", n, i),
                                   Out("g_W", fout, i) if wg else None, Out("g_b", fout) if wg else None, WS, WSB]
            for wg in (True, False):
                _collect(failures, lambda: _check_entry(f"wire_gabor_bwd_first_coords grads={wg} {tag}",
                                                        "wire_gabor_bwd_first_coords", fc(1.0, wg), ws,
                                                        ("wire_gabor_bwd_first_coords", fc(STALE_GAIN, True))))
    assert not failures, "\n".join(failures)


@pytest.mark.parametrize("n,fin,fout", LAYER_SHAPES)
def test_gabor2d_layer_calls(n, fin, fout):
    """wire_gabor2d_fwd / _bwd / _hparam_grad, hidden and first, and wire_gabor2d_bwd_first_coords."""
    from wire_amd import _lib
    L = _lib.lib()
    g = torch.Generator().manual_seed(n + 1)
    om, sc = 7.0, 6.0
    failures = []
    for first in (0, 1):
        i = 3 if first else fin
        c = () if first else (2,)
        x = _rn(g, n, i, *c)
        W, V = (_rn(g, fout, i, *c, scale=0.5 / i ** 0.5) for _ in range(2))
        b, cc = (_rn(g, fout, *c, scale=0.1) for _ in range(2))
        ga = _rn(g, n, fout, 2)
        ws = _ws(_lib.check(L.wire_layer2d_ws_bytes(n, i, fout)))
        tag = f"{'first' if first else 'hidden'} n={n} {i}->{fout}"
        pg = lambda: [Out("g_W", fout, i, *c), Out("g_b", fout, *c), Out("g_V", fout, i, *c), Out("g_c", fout, *c)]
        fwd = [x, W, b, V, cc, om, sc, n, i, fout, first, Out("act", n, fout, 2), WS, WSB]
        gx = None if first else Out("g_x", n, i, 2)
        bwd = lambda gain: [ga * gain, x, W, b, V, cc, om, sc, n, i, fout, first, gx, *pg(), WS, WSB]
        hp = [ga, x, W, b, V, cc, om, sc, n, i, fout, first, Out("out2", 2), WS, WSB]
        prev = ("wire_gabor2d_bwd", bwd(STALE_GAIN))
        _collect(failures, lambda: _check_entry(f"wire_gabor2d_fwd {tag}", "wire_gabor2d_fwd", fwd, ws, prev))
        _collect(failures, lambda: _check_entry(f"wire_gabor2d_bwd {tag}", "wire_gabor2d_bwd", bwd(1.0), ws, prev))
        _collect(failures, lambda: _check_entry(f"wire_gabor2d_hparam_grad {tag}", "wire_gabor2d_hparam_grad", hp, ws, prev))
        if first:
            fc = lambda gain, wg: [ga * gain, x, W, b, V, cc, om, sc, n, i, fout, Out("g_x", n, i),
                                   *(pg() if wg else [None] * 4), WS, WSB]
            for wg in (True, False):
                _collect(failures, lambda: _check_entry(f"wire_gabor2d_bwd_first_coords grads={wg} {tag}",
                                                        "wire_gabor2d_bwd_first_coords", fc(1.0, wg), ws,
                                                        ("wire_gabor2d_bwd_first_coords", fc(STALE_GAIN, True))))
    assert not failures, "\n".join(failures)


@pytest.mark.parametrize("n,fin", [(4133, 101), (129, 77)])
def test_final_layer_calls(n, fin):
    """wire_final_fwd / _bwd, O = 3."""
    from wire_amd import _lib
    L = _lib.lib()
    g = torch.Generator().manual_seed(n + 2)
    z, Wf, bf, gy = _rn(g, n, fin, 2), _rn(g, O, fin, 2, scale=0.1), _rn(g, O, 2), _rn(g, n, O)
    ws = _ws(_lib.check(L.wire_layer_ws_bytes(n, fin, O)))
    bwd = lambda gain: [gy * gain, z, Wf, n, fin, O, Out("g_z", n, fin, 2), Out("g_Wf", O, fin, 2), Out("g_bf", O, 2), WS, WSB]
    prev = ("wire_final_bwd", bwd(STALE_GAIN))
    failures = []
    _collect(failures, lambda: _check_entry(f"wire_final_fwd n={n}", "wire_final_fwd",
                                            [z, Wf, bf, n, fin, O, Out("y", n, O), WS, WSB], ws, prev))
    _collect(failures, lambda: _check_entry(f"wire_final_bwd n={n}", "wire_final_bwd", bwd(1.0), ws, prev))
    assert not failures, "\n".join(failures)


@pytest.mark.parametrize("kind", ["siren", "gauss", "relu"])
@pytest.mark.parametrize("n,fin,fout", LAYER_SHAPES)
def test_real_layer_calls(n, fin, fout, kind):
    """wire_real_layer_fwd / _bwd."""
    from wire_amd import _lib
    L = _lib.lib()
    g = torch.Generator().manual_seed(n + 3)
    om, sc = (30.0, 10.0) if kind != "gauss" else (30.0, 3.0)
    x, W, b, ga = _rn(g, n, fin), _rn(g, fout, fin, scale=0.3 / fin ** 0.5), _rn(g, fout, scale=0.1), _rn(g, n, fout)
    ws = _ws(_lib.check(L.wire_layer_ws_bytes(n, fin, fout)))
    k = _lib.KIND[kind]
    bwd = lambda gain: [k, ga * gain, x, W, b, om, sc, n, fin, fout, Out("g_x", n, fin), Out("g_W", fout, fin),
                        Out("g_b", fout), WS, WSB]
    prev = ("wire_real_layer_bwd", bwd(STALE_GAIN))
    failures = []
    _collect(failures, lambda: _check_entry(f"wire_real_layer_fwd {kind} n={n}", "wire_real_layer_fwd",
                                            [k, x, W, b, om, sc, n, fin, fout, Out("act", n, fout), WS, WSB], ws, prev))
    _collect(failures, lambda: _check_entry(f"wire_real_layer_bwd {kind} n={n}", "wire_real_layer_bwd", bwd(1.0), ws, prev))
    assert not failures, "\n".join(failures)


@pytest.mark.parametrize("n", [4133, 129])
def test_m2_combine_bwd(n):
    from wire_amd import _lib
    L = _lib.lib()
    S = 2
    g = torch.Generator().manual_seed(n + 4)
    W1, b1, W2, b2 = _rn(g, 128, S * O, scale=0.4), _rn(g, 128, scale=0.1), _rn(g, O, 128, scale=0.1), _rn(g, O)
    t, gy = _rn(g, S, n, O), _rn(g, n, O)
    ws = _ws(_lib.check(L.wire_m2_combine_ws_bytes(S, O, n)))
    a = lambda gain: [S, O, W1, b1, W2, b2, t, n, gy * gain, Out("g_t", S, n, O), Out("gW1", 128, S * O), Out("gb1", 128),
                      Out("gW2", O, 128), Out("gb2", O), WS, WSB]
    _check_entry(f"wire_m2_combine_bwd n={n}", "wire_m2_combine_bwd", a(1.0), ws, ("wire_m2_combine_bwd", a(STALE_GAIN)))


@pytest.mark.parametrize("n,fout", [(4133, 77), (129, 101)])
def test_mfn_filter_bwd(n, fout):
    from wire_amd import _lib
    L = _lib.lib()
    D = 2
    g = torch.Generator().manual_seed(n + 5)
    x, mu, w, c = _rn(g, n, D, scale=0.5), _rn(g, fout, D, scale=0.5), _rn(g, fout, D, scale=3.0), _rn(g, fout)
    gamma, go = _rn(g, fout).abs() + 0.5, _rn(g, n, fout)
    ws = _ws(_lib.check(L.wire_mfn_filter_ws_bytes(n, fout)))
    a = lambda gain: [go * gain, x, mu, gamma, w, c, n, D, fout, Out("g_mu", fout, D), Out("g_gamma", fout),
                      Out("g_w", fout, D), Out("g_c", fout), Out("g_x", n, D), WS, WSB]
    _check_entry(f"wire_mfn_filter_bwd n={n}", "wire_mfn_filter_bwd", a(1.0), ws, ("wire_mfn_filter_bwd", a(STALE_GAIN)))


@pytest.mark.parametrize("H,W,Oo,taps", [(37, 53, 3, 11), (64, 70, 1, 7)])
def test_ssim(H, W, Oo, taps):
    from wire_amd import _lib
    L = _lib.lib()
    g = torch.Generator().manual_seed(H)
    x = torch.rand(H, W, Oo, generator=g).to(DEV)
    y = (x + 0.1 * torch.randn(H, W, Oo, generator=g).to(DEV)).contiguous()
    if taps == 11:
        wv = np.exp(-(np.arange(11) - 5.0) ** 2 / (2 * 1.5 ** 2)).astype(np.float32)
        wv, cov = wv / wv.sum(dtype=np.float32), 1.0
    else:
        wv, cov = np.full(7, 1 / 7, np.float32), 49.0 / 48.0
    win = (C.c_float * taps)(*wv.tolist())
    ws = _ws(_lib.check(L.wire_ssim_ws_bytes(H, W, Oo, taps)))
    a = lambda gain: [x * gain, y * gain, H, W, Oo, taps, win, cov, 1e-4, 9e-4, Out("ssim", 1),
                      Out("map", H - taps + 1, W - taps + 1, Oo), WS, WSB]
    _check_entry(f"wire_ssim {H}x{W}x{Oo} taps {taps}", "wire_ssim", a(1.0), ws, ("wire_ssim", a(STALE_GAIN)))


# every partial below has exactly the size include/wire_hip.h asks for
def test_mse_grad_partial():
    """n O = 255 (one element short of filling a 256-thread block) and 1024 x 256 + 1 (one element more than the cap of
    1024 blocks holds at one element per thread), the second with idx and rec."""
    g = torch.Generator().manual_seed(9)
    part = _partial(4096)
    nb, Ob = 52429, 5                                                    # 262 145 = 1024 x 256 + 1 elements
    yb, tb = _rn(g, nb, Ob), _rn(g, nb, Ob)
    idx = torch.randperm(nb, generator=g).to(DEV)
    big = lambda gain: [yb * gain, tb, idx, 0, nb, Ob, 1.0, Out("g_y", nb, Ob), Out("loss", 1), Out("rec", nb, Ob), WS]
    ys, ts = _rn(g, 85, 3), _rn(g, 100, 3)
    small = [ys, ts, None, 7, 85, 3, 0.5, Out("g_y", 85, 3), Out("loss", 1), None, WS]
    failures = []
    _collect(failures, lambda: _check_entry("wire_mse_grad n O = 255", "wire_mse_grad", small, part,
                                            ("wire_mse_grad", big(STALE_GAIN))))
    _collect(failures, lambda: _check_entry("wire_mse_grad n O = 262145", "wire_mse_grad", big(1.0), part,
                                            ("wire_mse_grad", big(STALE_GAIN))))
    assert not failures, "\n".join(failures)


def test_avgpool_mse_grad_partial():
    H, W, scale = 26, 21, 4
    g = torch.Generator().manual_seed(10)
    y, gt = _rn(g, H * W, O), _rn(g, (H // scale) * (W // scale), O)
    a = lambda gain: [y * gain, H, W, O, scale, gt, Out("g_y", H * W, O), Out("rec_lr", *gt.shape), Out("loss", 1), WS]
    _check_entry("wire_avgpool_mse_grad", "wire_avgpool_mse_grad", a(1.0), _partial(1024),
                 ("wire_avgpool_mse_grad", a(STALE_GAIN)))


@pytest.mark.parametrize("B,H,W,Oo,scale", [(3, 10, 13, 3, 4), (2, 40, 37, 30, 35)])
def test_avgpool_mse_grad_frames_partial(B, H, W, Oo, scale):
    """The LDS path and the direct path (scale O = 1050 > 1024), shapes of test_gpu_multi_sr.py; the last frame masked."""
    g = torch.Generator().manual_seed(12)
    m = (H // scale) * (W // scale)
    y, gt = _rn(g, B, H * W, Oo), _rn(g, B, m, Oo)
    mask = (torch.rand(B, m, Oo, generator=g) > 0.3).float().to(DEV)
    mask[B - 1] = 0
    a = lambda gain: [y * gain, B, H, W, Oo, scale, gt, mask, Out("g_y", B, H * W, Oo), Out("rec_lr", B, m, Oo),
                      Out("loss", 1), WS]
    _check_entry(f"wire_avgpool_mse_grad_frames {B}x{H}x{W}x{Oo}/{scale}", "wire_avgpool_mse_grad_frames", a(1.0),
                 _partial(1024), ("wire_avgpool_mse_grad_frames", a(STALE_GAIN)))


@pytest.mark.parametrize("H,W,T,Oo,nframes", [(5, 7, 10, 1, 4), (6, 6, 8, 3, 4)])
def test_coded_mse_grad_partial(H, W, T, Oo, nframes):
    g = torch.Generator().manual_seed(13)
    NP, Cp = H * W, (T + nframes - 1) // nframes + 1
    y, gt = _rn(g, NP * T, Oo), _rn(g, Cp, NP, Oo)
    mask = (torch.randint(0, 3, (NP, T), generator=g).float() / 2).to(DEV)
    a = lambda gain: [y * gain, 0, NP, NP, T, Oo, nframes, 1, mask, gt, Out("g_y", NP * T, Oo), Out("est", Cp, NP, Oo),
                      Out("loss", 1), WS]
    _check_entry(f"wire_coded_mse_grad {H}x{W}x{T}x{Oo}", "wire_coded_mse_grad", a(1.0), _partial(1024),
                 ("wire_coded_mse_grad", a(STALE_GAIN)))


@pytest.mark.parametrize("H,W,Oo", [(33, 65, 1), (130, 70, 8)])
def test_tv_partials(H, W, Oo):
    """wire_tv_fwd (1024 floats) and wire_tv_mse_grad (2048), with a range and with indices."""
    g = torch.Generator().manual_seed(14)
    n = H * W
    y, t = _rn(g, n, Oo), _rn(g, n, Oo)
    idx = torch.randperm(n, generator=g)[:n // 2 + 1].to(DEV).contiguous()
    fw = lambda gain: [y * gain, Oo, H, W, Oo, 1, Out("tv", 1), WS]
    mg = lambda gain, ix: [y * gain, H, W, Oo, t, ix, 0 if ix is not None else n // 4, idx.numel() if ix is not None
                           else n // 2, 2.0 ** -10, Out("g_y", n, Oo), Out("loss", 3), Out("rec", n, Oo), WS]
    failures = []
    _collect(failures, lambda: _check_entry(f"wire_tv_fwd {H}x{W}x{Oo}", "wire_tv_fwd", fw(1.0), _partial(1024),
                                            ("wire_tv_fwd", fw(STALE_GAIN))))
    for ix in (None, idx):
        _collect(failures, lambda: _check_entry(f"wire_tv_mse_grad {H}x{W}x{Oo} idx={ix is not None}", "wire_tv_mse_grad",
                                                mg(1.0, ix), _partial(2048), ("wire_tv_mse_grad", mg(STALE_GAIN, idx))))
    assert not failures, "\n".join(failures)


@pytest.mark.parametrize("count", [1, 257])
@pytest.mark.parametrize("mode", [0, 1])
def test_eval_metric_partial(mode, count):
    g = torch.Generator().manual_seed(15)
    big = 70001
    rec, gt = torch.rand(big, generator=g).to(DEV), (torch.rand(big, generator=g) > 0.4).float().to(DEV)
    a = lambda cnt, gain: [mode, rec * gain, gt * gain, cnt, 0.5, Out("out2", 2), WS]
    _check_entry(f"wire_eval_metric mode {mode} count {count}", "wire_eval_metric", a(count, 1.0), _partial(2048),
                 ("wire_eval_metric", a(big, STALE_GAIN)))
