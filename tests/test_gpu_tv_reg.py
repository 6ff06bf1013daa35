"""GPU checks of the TV prior of the operator steps: wire_tv_add_grad against the restatement of tests/tv_reg_ref.py on
every path of its launcher, and FusedTrainer.step_downsampled / step_coded / step_radon with their lambda keywords --
every parameter gradient against the fp64 oracle, the data term from the oracle's own forward and the TV sign pattern
from the trainer's self.y (the protocol of tests/test_gpu_tv.py)."""
import numpy as np
import pytest
import torch

from _util import kernel_names, params_np, relmax, within_ref, _sd
import hier_ref as hr
import tv_reg_ref as ref
import video_cs_ref as vref
from oracle import torch_ref, wire_oracle as wo

pytestmark = pytest.mark.gpu
DEV = torch.device("cuda:0")

# (H, W, T, O).  One thread per FLAT element, 256-element blocks, at most 1024 of them: a block loops above 262 144
# elements, and a block boundary falls wherever 256 elements end.
#   (1, 1, 1, 1)     no pair                        (16, 16, 1, 1)   exactly one block
#   (1, 1, 5, 2)     temporal pairs only            (32, 16, 1, 1)   two full blocks meeting on a row boundary
#   (1, 7, 1, 2)     horizontal pairs only          (8, 8, 4, 1)     one block, T > 1
#   (7, 1, 1, 3)     vertical pairs only            (6, 5, 4, 8)     the widest O
#   (2, 2, 2, 1)     every element a corner         (512, 512, 1, 1) 1024 full blocks, the last size without a loop
#   (5, 7, 3, 3)     two ragged blocks              (300, 301, 1, 3) blocks loop, T = 1
#   (20, 13, 2, 3)   block boundaries between the channels of one pixel
#   (64, 64, 13, 5)  blocks loop, T > 1
OP_SHAPES = [(1, 1, 1, 1), (1, 1, 5, 2), (1, 7, 1, 2), (7, 1, 1, 3), (2, 2, 2, 1), (5, 7, 3, 3), (20, 13, 2, 3),
             (16, 16, 1, 1), (32, 16, 1, 1), (8, 8, 4, 1), (6, 5, 4, 8), (512, 512, 1, 1), (300, 301, 1, 3),
             (64, 64, 13, 5)]
FILL = 7.0
GUARD = 64
LS, LT = float(np.float32(0.3)), float(np.float32(0.07))
RADON_BOUND = 1e-5      # what test_gpu_workspace_fill.py::test_step_radon holds the same call repeated to


def _lib():
    from wire_amd import _lib
    return _lib, _lib.lib()


def _stream():
    return torch.cuda.current_stream().cuda_stream


class _Op:
    """wire_tv_add_grad on one image, uploaded once; g_y and loss_out carry GUARD floats of 7.0 behind them."""

    def __init__(self, y, H, W, T, O):
        self.lib, self.L = _lib()
        self.y, self.dims, self.n = torch.tensor(y, device=DEV), (H, W, T, O), y.size
        self.part = torch.empty(2048, device=DEV)
        self.data = torch.tensor([0.625], device=DEV)

    def call(self, g_in, ls, lt, data=True):
        g = torch.full((self.n + GUARD,), FILL, device=DEV)
        g[:self.n] = torch.tensor(g_in.reshape(-1), device=DEV)
        out = torch.full((4 + GUARD,), FILL, device=DEV)
        self.lib.check(self.L.wire_tv_add_grad(_stream(), self.y.data_ptr(), *self.dims, ls, lt,
                                               self.data.data_ptr() if data else None, g.data_ptr(), out.data_ptr(),
                                               self.part.data_ptr()), "wire_tv_add_grad")
        torch.cuda.synchronize()
        g, out = g.cpu().numpy(), out.cpu().numpy()
        assert (g[self.n:] == FILL).all() and (out[4:] == FILL).all(), "wire_tv_add_grad wrote past its outputs"
        return out[:4], g[:self.n].reshape(g_in.shape)


@pytest.mark.parametrize("quantised", [True, False])
@pytest.mark.parametrize("H,W,T,O", OP_SHAPES)
def test_tv_add_grad_matches_restatement(H, W, T, O, quantised):
    """g_y prefilled with normal draws and with zeros; both lambdas (0.3, 0.07), each alone, and both zero.
    |g - g64| <= 3 * 2^-24 (|g_in| + 4 |lambda_s| + 2 |lambda_t|) per element (three roundings, each at most half an ulp
    of a partial sum no larger than the bracket); tv_s and tv_t 1e-5 relative to fp64; loss_out[0] the header's fp32
    expression of the other three, bit for bit; data = data_loss[0], 0 for NULL; zero lambdas leave g_y up to the sign
    of a zero; the same call twice gives the same bits; T = 1, zero prefill, lambda_s = 2^-2 is wire_tv_bwd bit for bit."""
    n = H * W * T
    rng = np.random.default_rng(H * 1000 + W * 10 + T * 100 + O)
    y = rng.standard_normal((n, O)).astype(np.float32)
    if quantised:
        y = (np.round(y * 4) / 4).astype(np.float32)
    op = _Op(y, H, W, T, O)
    tvs64, tvt64 = ref.tv_sums(y, H, W, T, O)
    ks, kt = ref.sign_patterns(y, H, W, T, O)
    if quantised and n * O >= 100:
        assert (ks == 0).any()                                   # ties are frequent: s(0) occurs
    for g_in in (rng.standard_normal((n, O)).astype(np.float32), np.zeros((n, O), np.float32)):
        for ls, lt in ((LS, LT), (LS, 0.0), (0.0, LT)):
            out, g = op.call(g_in, ls, lt)
            _, _, _, g64 = ref.tv_add_grad(y, g_in, H, W, T, O, ls, lt)
            bound = 3 * 2.0 ** -24 * (np.abs(g_in).astype(np.float64) + 4 * abs(ls) + 2 * abs(lt))
            err = np.abs(g.astype(np.float64) - g64)
            print(f"tv_add_grad {(H, W, T, O)} quantised={quantised} lambdas {ls:g} {lt:g}: worst err / bound "
                  f"{(err / bound).max():.3f}  parts {out}")
            assert (err <= bound).all()
            for got, want in ((out[2], tvs64), (out[3], tvt64)):
                assert abs(float(got) - want) <= 1e-5 * want if want > 0 else got == 0.0
            assert out[1] == np.float32(0.625)
            assert out[0].tobytes() == ref.total_loss(out[1], ls, out[2], lt, out[3]).tobytes()
            again = op.call(g_in, ls, lt)
            assert out.tobytes() == again[0].tobytes() and g.tobytes() == again[1].tobytes()
        out, g = op.call(g_in, LS, LT, data=False)
        assert out[1] == 0.0 and out[0].tobytes() == ref.total_loss(0.0, LS, out[2], LT, out[3]).tobytes()
        out0, g0 = op.call(g_in, 0.0, 0.0)
        assert np.array_equal(g0, g_in)                          # -0 == +0
        assert out0[0] == out0[1] and out0[2] == out[2] and out0[3] == out[3]
    if (H, W, T, O) == (1, 1, 1, 1):
        assert out[2] == 0.0 and out[3] == 0.0
    if T == 1:
        lib, L = _lib()
        out, g = op.call(np.zeros((n, O), np.float32), 0.25, 0.0)
        up = torch.tensor([0.25], device=DEV)
        gx = torch.full((n * O,), FILL, device=DEV)
        lib.check(L.wire_tv_bwd(_stream(), op.y.data_ptr(), O, H, W, O, 1, up.data_ptr(), gx.data_ptr()), "wire_tv_bwd")
        torch.cuda.synchronize()
        assert g.tobytes() == gx.cpu().numpy().tobytes()
        assert g.tobytes() == (np.float32(0.25) * ks.astype(np.float32)).tobytes()


# ---------------------------------------------------------------------------------------------------------------
# the trainer
# ---------------------------------------------------------------------------------------------------------------
def _net(kind, D, O, hf=128, hp=None):
    from wire_amd.modules import models
    torch.manual_seed(0)
    hp = hp or ((7.0, 7.0, 6.0) if kind == "wire" else (30.0, 30.0, 10.0))
    m = models.get_INR(nonlin=kind, in_features=D, out_features=O, hidden_features=hf, hidden_layers=2,
                       first_omega_0=hp[0], hidden_omega_0=hp[1], scale=hp[2])
    return m.to(DEV), hp


def _tensors(model, tr):
    names = [k for k in model.state_dict().keys() if "omega_0" not in k and "scale_0" not in k]
    assert len(names) == len(tr.offsets)
    return list(zip(names, tr.offsets))


def _pow2_near(v):
    """The power of two nearest (in log) to v: within a factor sqrt(2) of it."""
    return 2.0 ** int(np.round(np.log2(v)))


def _assert_few_flips(y_dev, y64, dims, label):
    """At most 0.1 % of all neighbour pairs, along every axis the case has, differ in sign between the trainer's fp32
    image and the fp64 oracle's, so that the borrowed pattern cannot hide a wrong image."""
    a = np.concatenate([s.ravel() for s in ref.pair_signs(y_dev, *dims)])
    b = np.concatenate([s.ravel() for s in ref.pair_signs(y64, *dims)])
    H, W, T, O = dims
    assert a.size == O * ((H - 1) * W * T + H * (W - 1) * T + H * W * (T - 1))
    flips = int((a != b).sum())
    print(f"{label}: {flips} of {a.size} pairs differ in sign between self.y and the fp64 oracle")
    assert flips <= 1e-3 * a.size


def _assert_balanced(gy_data, lams, label):
    """The largest data term of g_y lies within 0.1 x .. 10 x of every nonzero lambda: neither term hides."""
    gm = float(np.abs(gy_data).max())
    for lam in lams:
        print(f"{label}: max data term of g_y {gm:.2e}, TV unit {lam:.2e}")
        assert 0.1 <= gm / lam <= 10


def _assert_bf16_bounds(model, tr, loss, flat, l64, g64, label):
    """Loss 2e-5 relative, every gradient 5e-5 max|g| + 1e-10 (test_gpu_tv.py's _assert_bf16_bounds)."""
    for name, off in _tensors(model, tr):
        g = wo.as_real_pairs(g64[name]).astype(np.float64).ravel()
        print(f"{label}: {name} err / max|g| {np.abs(flat[off:off + g.size] - g).max() / np.abs(g).max():.2e}")
    print(f"{label}: loss {loss:.6e} rel {abs(loss - l64) / l64:.2e}")
    assert abs(loss - l64) <= 2e-5 * l64
    for name, off in _tensors(model, tr):
        g = wo.as_real_pairs(g64[name]).astype(np.float64).ravel()
        assert np.abs(flat[off:off + g.size] - g).max() <= 5e-5 * np.abs(g).max() + 1e-10, name


def _assert_parts(tr, loss, ls, lt, data64, tvs64, tvt64):
    p = tr.tv_parts.cpu().numpy()
    assert p[0] == np.float32(loss) and p[0].tobytes() == ref.total_loss(p[1], ls, p[2], lt, p[3]).tobytes()
    assert abs(p[1] - data64) <= 2e-5 * data64 and abs(p[2] - tvs64) <= 2e-5 * tvs64
    assert abs(p[3] - tvt64) <= 2e-5 * tvt64 if tvt64 > 0 else p[3] == 0.0


class _Net:
    """A wire or real net and the numpy oracle's forward and backward of it, in fp64 or fp32."""

    def __init__(self, kind, D, O, hf=128, hp=None):
        self.kind = kind
        self.model, self.hp = _net(kind, D, O, hf, hp)

    def forward(self, x, double):
        dt = np.float64 if double else np.float32
        p = wo.cast_params(params_np(self.model), double)
        a = tuple(dt(v) for v in self.hp)
        if self.kind == "wire":
            y, cache = wo.wire_forward(p, x.astype(dt), 2, *a, keep=True)
        else:
            y, cache = wo.realnet_forward(self.kind, p, x.astype(dt), 2, *a, None, keep=True)
        return y, (p, cache, a, dt)

    def backward(self, ctx, gy):
        p, cache, a, dt = ctx
        gy = np.asarray(gy, dt)
        return wo.wire_backward(p, cache, gy, 2, *a) if self.kind == "wire" else \
            wo.realnet_backward(self.kind, p, cache, gy, 2, *a)


# ---- step_downsampled -----------------------------------------------------------------------------------------
class _SisrCase:
    """An lr = 0 trainer on an (H, W) grid and a low-resolution target; the plain step runs first (it builds the
    coordinates the oracles run on), and the lambda is the power of two nearest the fp64 oracle's largest data term."""

    def __init__(self, kind, H, W, O, scale, seed):
        from wire_amd.trainer import FusedTrainer
        self.H, self.W, self.O, self.scale, self.n = H, W, O, scale, H * W
        self.net = _Net(kind, 2, O)
        self.tr = FusedTrainer(self.net.model, (H, W), None, lr=0.0)
        self.gt = np.random.default_rng(seed).uniform(0, 1, ((H // scale) * (W // scale), O)).astype(np.float32)
        self.gt_dev = torch.tensor(self.gt, device=DEV)
        self.loss0 = self.tr.step_downsampled(self.gt_dev, scale)
        torch.cuda.synchronize()
        self.flat0 = self.tr.flat_grad.cpu().numpy().copy()
        self.x = self.tr.coords[:self.n * 2].reshape(self.n, 2).cpu().numpy()
        y64, _ = self.net.forward(self.x, True)
        _, gy, _ = wo.avgpool_mse_loss_and_grad(y64, H, W, scale, self.gt.astype(np.float64))
        self.lam = _pow2_near(np.abs(gy).max())

    def step(self):
        loss = self.tr.step_downsampled(self.gt_dev, self.scale, lambda_tv=self.lam)
        torch.cuda.synchronize()
        self.y = self.tr.y[:self.n * self.O].cpu().numpy().reshape(self.n, self.O).copy()
        return float(loss.item()), self.tr.flat_grad.cpu().numpy().copy()

    def oracle(self, double, label=None):
        dt = np.float64 if double else np.float32
        y, ctx = self.net.forward(self.x, double)
        dims = (self.H, self.W, 1, self.O)
        if label:
            _assert_few_flips(self.y, y, dims, label)
        data, gy, _ = wo.avgpool_mse_loss_and_grad(y, self.H, self.W, self.scale, self.gt.astype(dt))
        if label:
            _assert_balanced(gy, [self.lam], label)
        loss, tvs, tvt, g = ref.tv_add_grad(y, gy, *dims, self.lam, 0.0, data=data, double=double, pattern_from=self.y)
        return float(loss), self.net.backward(ctx, g.reshape(y.shape)), (float(data), float(tvs), float(tvt))


def test_step_downsampled_bf16_family_matches_oracle():
    """Case 1: wire 2 x 128 (omega_0 = 7, s_0 = 6) on 24 x 20, O = 3, scale 2: loss 2e-5 relative, every gradient
    5e-5 max|g| + 1e-10 against the fp64 oracle; tv_parts consistent with the returned loss; a plain step afterwards
    returns the plain loss again."""
    c = _SisrCase("wire", 24, 20, 3, 2, 31)
    loss, flat = c.step()
    l64, g64, (d64, tvs64, tvt64) = c.oracle(True, "step_downsampled (1)")
    _assert_bf16_bounds(c.net.model, c.tr, loss, flat, l64, g64, "step_downsampled (1)")
    _assert_parts(c.tr, loss, c.lam, 0.0, d64, tvs64, tvt64)
    assert loss > float(c.loss0.item()) and not np.array_equal(flat, c.flat0)
    again = c.tr.step_downsampled(c.gt_dev, 2)
    assert again.cpu().numpy().tobytes() == c.loss0.cpu().numpy().tobytes()


def test_step_downsampled_fp16_family_within_reference_error():
    """Case 2: siren on 72 x 64 (4 608 rows, the 2 x fp16 family), O = 3, scale 2: loss and every gradient within 3 x the
    error of the fp32 oracle against fp64 + 1e-6."""
    c = _SisrCase("siren", 72, 64, 3, 2, 32)
    loss, flat = c.step()
    l64, g64, _ = c.oracle(True, "step_downsampled (2)")
    l32, g32, _ = c.oracle(False)
    checks = [("step_downsampled tv siren loss", abs(loss - l64) / l64, abs(l32 - l64) / l64)]
    for name, off in _tensors(c.net.model, c.tr):
        g = wo.as_real_pairs(g64[name]).astype(np.float64).ravel()
        r = wo.as_real_pairs(g32[name]).astype(np.float64).ravel()
        checks.append((f"step_downsampled tv siren {name}", relmax(flat[off:off + g.size], g), relmax(r, g)))
    for label, eb, er in checks:
        print(f"{label}: err_build {eb:.3e}  err_ref {er:.3e}  ratio {eb / er if er > 0 else float('inf'):.2f}")
    for label, eb, er in checks:
        within_ref(eb, er, label, factor=3.0)


def test_step_downsampled_hier_at_scale_1():
    """Case 3: a bspline_mscale_hier trainer with one rate per stage (built as test_step_tv_hier_with_stage_rates builds
    it) at scale 1, where the pooled loss is the full-grid MSE: the gradients of the parameters before the step meet
    case 1's bounds against the fp64 closed form of tests/hier_ref.py, driven with the pseudo-target
    t' = y64 - g_y H W O / 2, for which its MSE gradient is the regularised g_y."""
    from wire_amd.modules import models
    from wire_amd.trainer import FusedTrainer
    H, W, O, st, L = 24, 20, 3, [1 / 9, 4.0], 2
    n = H * W
    torch.manual_seed(0)
    model = models.get_INR(nonlin="bspline_mscale_hier", in_features=2, out_features=O, hidden_features=64,
                           scaled_hidden_features=0, hidden_layers=L, first_omega_0=-0.2, hidden_omega_0=-0.2,
                           scale=0.0, scale_tensor=st).to(DEV)
    gt = np.random.default_rng(33).uniform(0, 1, (n, O)).astype(np.float32)
    tr = FusedTrainer(model, (H, W), None, lr=[6e-3, 2e-2], niters=100)
    sd = _sd(model)
    heads = {}
    for s, lin in enumerate(model.linears):
        heads[f"linears.{s}.weight"] = lin.weight.detach().cpu().numpy().copy()
        heads[f"linears.{s}.bias"] = lin.bias.detach().cpu().numpy().copy()
    names = [k for k in sd if "scale_0" not in k] + list(heads)
    # the lambda from the oracle on the drivers' coordinates; the comparison below runs on the rows the trainer builds
    y64 = hr.forward(sd, heads, L, wo.image_coords(H, W).astype(np.float64), st, np.float64)
    lam = _pow2_near(np.abs(wo.mse_loss_and_grad(y64, gt.astype(np.float64))[1]).max())
    p0 = tr.flat.clone()
    loss = float(tr.step_downsampled(torch.tensor(gt, device=DEV), 1, lambda_tv=lam).item())
    torch.cuda.synchronize()
    assert not torch.equal(tr.flat, p0)
    x = tr.coords[:n * 2].reshape(n, 2).cpu().numpy().astype(np.float64)
    y64 = hr.forward(sd, heads, L, x, st, np.float64)
    d64, gy_data = wo.mse_loss_and_grad(y64, gt.astype(np.float64))
    _assert_balanced(gy_data, [lam], "step_downsampled (3) hier")
    y_dev = tr.y[:n * O].cpu().numpy().reshape(n, O)
    _assert_few_flips(y_dev, y64, (H, W, 1, O), "step_downsampled (3) hier")
    l64, _, _, gy = ref.tv_add_grad(y64, gy_data, H, W, 1, O, lam, 0.0, data=d64, pattern_from=y_dev)
    pseudo = y64 - gy * (n * O / 2.0)
    _, _, g64, _ = hr.loss_and_grads(sd, heads, L, x, pseudo, st, np.float64)
    flat = tr.flat_grad.cpu().numpy()
    print(f"step_downsampled (3) hier: loss {loss:.6e} rel {abs(loss - l64) / l64:.2e}")
    assert abs(loss - l64) <= 2e-5 * l64
    assert len(names) == len(tr.offsets)
    for k, off, sz in zip(names, tr.offsets, tr.sizes):
        g = g64[k].ravel()
        print(f"step_downsampled (3) hier: {k} err / max|g| {np.abs(flat[off:off + sz] - g).max() / np.abs(g).max():.2e}")
    for k, off, sz in zip(names, tr.offsets, tr.sizes):
        g = g64[k].ravel()
        assert np.abs(flat[off:off + sz] - g).max() <= 5e-5 * np.abs(g).max() + 1e-10, k


# ---- step_coded -----------------------------------------------------------------------------------------------
def test_step_coded_with_both_priors_matches_oracle():
    """test_gpu_video_cs.py's case (a) -- wire 2 x 128 on 12 x 10 x 9, nframes 4, O = 1 -- with lambda_tv != lambda_tv_t,
    both nonzero (the power of two nearest the largest data term of g_y, and half of it): the bounds of
    test_step_coded_bf16_family_matches_oracle; tv_parts consistent with the returned loss; a slab that splits the grid
    raises with a nonzero lambda."""
    from wire_amd.trainer import FusedTrainer
    H, W, T, O, nframes = 12, 10, 9, 1, 4
    NP, n = H * W, H * W * T
    rng = np.random.default_rng(11)
    net = _Net("wire", 3, O)
    tr = FusedTrainer(net.model, (H, W, T), None, lr=0.0)
    Cp = vref.nchunks(T, nframes) + 1
    gt = rng.uniform(0, 1, (Cp, NP, O)).astype(np.float32)
    mask = vref.make_mask(rng, NP, T)
    gt_dev, mask_dev = torch.tensor(gt, device=DEV), torch.tensor(mask, device=DEV)
    plain = tr.step_coded(gt_dev, mask_dev, nframes)
    torch.cuda.synchronize()
    x = tr.coords[:n * 3].reshape(n, 3).cpu().numpy()
    y64, ctx = net.forward(x, True)
    d64, gy_data, _ = vref.coded_loss_and_grad(y64, mask, gt, T, nframes, True, double=True)
    ls = _pow2_near(np.abs(gy_data).max())
    lt = ls / 2
    _assert_balanced(gy_data, [ls, lt], "step_coded tv")
    loss = float(tr.step_coded(gt_dev, mask_dev, nframes, lambda_tv=ls, lambda_tv_t=lt).item())
    torch.cuda.synchronize()
    flat = tr.flat_grad.cpu().numpy().copy()
    y_dev = tr.y[:n * O].cpu().numpy().reshape(n, O).copy()
    _assert_few_flips(y_dev, y64, (H, W, T, O), "step_coded tv")
    l64, tvs64, tvt64, gy = ref.tv_add_grad(y64, gy_data, H, W, T, O, ls, lt, data=d64, pattern_from=y_dev)
    g64 = net.backward(ctx, gy.reshape(y64.shape))
    _assert_bf16_bounds(net.model, tr, loss, flat, float(l64), g64, "step_coded tv")
    _assert_parts(tr, loss, ls, lt, float(d64), float(tvs64), float(tvt64))
    assert loss > float(plain.item())
    # each prior alone moves the gradient, and differently
    for kw in (dict(lambda_tv=ls), dict(lambda_tv_t=lt)):
        one = float(tr.step_coded(gt_dev, mask_dev, nframes, slab=NP, **kw).item())
        torch.cuda.synchronize()
        l1, _, _, g1 = ref.tv_add_grad(y64, gy_data, H, W, T, O, kw.get("lambda_tv", 0.0), kw.get("lambda_tv_t", 0.0),
                                       data=d64, pattern_from=y_dev)
        _assert_bf16_bounds(net.model, tr, one, tr.flat_grad.cpu().numpy(), float(l1),
                            net.backward(ctx, g1.reshape(y64.shape)), f"step_coded tv {sorted(kw)}")
    for kw in (dict(lambda_tv=ls), dict(lambda_tv_t=lt), dict(lambda_tv=ls, lambda_tv_t=lt)):
        with pytest.raises(ValueError, match="slab"):
            tr.step_coded(gt_dev, mask_dev, nframes, slab=50, **kw)
    for kw in (dict(lambda_tv=float("nan")), dict(lambda_tv_t=float("inf"))):
        with pytest.raises(ValueError, match=next(iter(kw)) + " must be finite"):
            tr.step_coded(gt_dev, mask_dev, nframes, **kw)


# ---- step_radon -----------------------------------------------------------------------------------------------
class _CtCase:
    """The 24 x 30, 17-angle, 2 x 64 wire setting of test_ct_radon.py on an lr = 0 trainer."""
    H, W, A, hp = 24, 30, 17, (3.0, 3.0, 12.0)

    def __init__(self):
        from wire_amd.trainer import FusedTrainer
        H, W = self.H, self.W
        self.n = H * W
        yy, xx = np.meshgrid(np.linspace(-1, 1, H), np.linspace(-1, 1, W), indexing="ij")
        self.img = (0.5 + 0.4 * np.sin(3 * xx) * np.cos(2 * yy)).astype(np.float32)
        self.thetas = np.linspace(0, 180, self.A, dtype=np.float32)
        self.sino = torch_ref.radon(torch.tensor(self.img), torch.tensor(self.thetas)).numpy()      # fp32 data
        self.net = _Net("wire", 2, 1, hf=64, hp=self.hp)
        self.tr = FusedTrainer(self.net.model, (H, W), None, lr=0.0)
        self.sino_dev, self.th_dev = torch.tensor(self.sino, device=DEV), torch.tensor(self.thetas, device=DEV)

    def step(self, **kw):
        loss = self.tr.step_radon(self.sino_dev, self.th_dev, **kw)
        torch.cuda.synchronize()
        self.y = self.tr.y[:self.n].cpu().numpy().reshape(self.n, 1).copy()
        return float(loss.item()), self.tr.flat_grad.cpu().numpy().copy()

    def data_term(self):
        """The fp64 oracle's image, its data loss and dL/dy by fp64 autograd of torch_ref.radon."""
        x = self.tr.coords[:self.n * 2].reshape(self.n, 2).cpu().numpy()
        y64, ctx = self.net.forward(x, True)
        est = torch.tensor(y64.reshape(self.H, self.W), requires_grad=True)
        loss = ((torch.tensor(self.sino).double() - torch_ref.radon(est, torch.tensor(self.thetas))) ** 2).mean()
        loss.backward()
        return y64, ctx, float(loss.item()), est.grad.numpy().reshape(self.n, 1)

    def errors(self, loss, flat, l64, g64):
        errs = {"loss": abs(loss - l64) / l64}
        for name, off in _tensors(self.net.model, self.tr):
            g = wo.as_real_pairs(g64[name]).astype(np.float64).ravel()
            errs[name] = (np.abs(flat[off:off + g.size] - g).max(), np.abs(g).max())
        return errs


def test_step_radon_with_prior_matches_oracle():
    """No existing test bounds this step's parameter gradients, so the comparison is first measured at lambda_tv = 0, a
    path that runs only the code of before, and the lambda_tv > 0 case is allowed 2 x that error per tensor (the TV term
    adds one exact-integer product per element; the factor covers the atomics' run-to-run spread), never less than the
    bf16 bounds: loss 2e-5, gradients 5e-5 max|g| + 1e-10.  Both columns are printed (profiles/tv_reg_parity.txt).
    lambda_tv = 0.0 stays within 1e-5 of the call without the keyword (float atomics: no bit equality)."""
    c = _CtCase()
    loss0, flat0 = c.step()
    y64, ctx, d64, gy_data = c.data_term()
    e0 = c.errors(loss0, flat0, d64, c.net.backward(ctx, gy_data))
    lossz, flatz = c.step(lambda_tv=0.0)
    assert relmax(flatz, flat0) <= RADON_BOUND and abs(lossz - loss0) <= RADON_BOUND * loss0
    lam = _pow2_near(np.abs(gy_data).max())
    _assert_balanced(gy_data, [lam], "step_radon tv")
    loss, flat = c.step(lambda_tv=lam)
    _assert_few_flips(c.y, y64, (c.H, c.W, 1, 1), "step_radon tv")
    l64, tvs64, tvt64, gy = ref.tv_add_grad(y64, gy_data, c.H, c.W, 1, 1, lam, 0.0, data=d64, pattern_from=c.y)
    e1 = c.errors(loss, flat, float(l64), c.net.backward(ctx, gy))
    print(f"step_radon parity 24x30, 17 angles, wire 2x64, lambda_tv {lam:g}: err / max|g|   lambda 0    lambda > 0")
    print(f"step_radon parity: {'loss (relative)':28s} {e0['loss']:.3e}   {e1['loss']:.3e}")
    for k in e0:
        if k != "loss":
            print(f"step_radon parity: {k:28s} {e0[k][0] / e0[k][1]:.3e}   {e1[k][0] / e1[k][1]:.3e}")
    assert e1["loss"] <= max(2 * e0["loss"], 2e-5)
    for k in e0:
        if k != "loss":
            assert e1[k][0] <= max(2 * e0[k][0] / e0[k][1], 5e-5) * e1[k][1] + 1e-10, k
    _assert_parts(c.tr, loss, lam, 0.0, d64, float(tvs64), 0.0)
    assert loss > loss0 and not np.array_equal(flat, flat0)
    with pytest.raises(ValueError, match="lambda_tv must be finite"):
        c.step(lambda_tv=float("nan"))


def test_ct_loop_with_prior_follows_autograd():
    """The 8-step loss trajectory of test_ct_driver_loop_and_fused_step with lambda_tv > 0: the autograd side is
    mse + lambda * utils.total_variation_loss(img_estim) on the drop-in modules, held at that test's rtol = 2e-3."""
    from torch.optim.lr_scheduler import LambdaLR
    from wire_amd.modules import lin_inverse, models, utils
    from wire_amd.trainer import FusedTrainer
    H, W, nmeas, niters, lr = 24, 30, 17, 8, 5e-3
    omega0, sigma0 = 3.0, 12.0
    yy, xx = np.meshgrid(np.linspace(-1, 1, H), np.linspace(-1, 1, W), indexing="ij")
    img = (0.5 + 0.4 * np.sin(3 * xx) * np.cos(2 * yy)).astype(np.float32)
    imten = torch.tensor(img)[None, None, ...].cuda()
    thetas = torch.tensor(np.linspace(0, 180, nmeas, dtype=np.float32)).cuda()

    def build():
        torch.manual_seed(0)
        return models.get_INR(nonlin="wire", in_features=2, out_features=1, hidden_features=64, hidden_layers=2,
                              first_omega_0=omega0, hidden_omega_0=omega0, scale=sigma0, pos_encode=False,
                              sidelength=nmeas).cuda()
    model = build()
    with torch.no_grad():
        sinogram_ten = lin_inverse.radon(imten, thetas).detach()
    x = torch.linspace(-1, 1, W).cuda()
    y = torch.linspace(-1, 1, H).cuda()
    X, Y = torch.meshgrid(x, y, indexing='xy')
    coords = torch.hstack((X.reshape(-1, 1), Y.reshape(-1, 1)))[None, ...]
    # the lambda: the power of two nearest the largest data term of dL/d(img_estim) at the first step
    est = model(coords).reshape(-1, H, W)[None, ...].detach().requires_grad_(True)
    ((sinogram_ten - lin_inverse.radon(est, thetas)) ** 2).mean().backward()
    lam = _pow2_near(float(est.grad.abs().max().item()))
    optimizer = torch.optim.Adam(lr=lr, params=model.parameters())
    scheduler = LambdaLR(optimizer, lambda x: 0.1 ** min(x / niters, 1))
    losses, plain = [], []
    for idx in range(niters):
        img_estim = model(coords).reshape(-1, H, W)[None, ...]
        mse = ((sinogram_ten - lin_inverse.radon(img_estim, thetas)) ** 2).mean()
        loss = mse + lam * utils.total_variation_loss(img_estim)
        optimizer.zero_grad()
        loss.backward()
        optimizer.step()
        scheduler.step()
        losses.append(loss.item())
        plain.append(mse.item())
    tr = FusedTrainer(build(), (H, W), None, lr=lr, niters=niters)
    fused = []
    for idx in range(niters):
        fused.append(tr.step_radon(sinogram_ten, thetas, lambda_tv=lam))
        tr.scheduler_step()
    torch.cuda.synchronize()
    fused = [float(l.item()) for l in fused]
    print(f"ct loop, lambda_tv {lam:g}: autograd {losses}\n fused {fused}\n mse part {plain}")
    assert min(l - m for l, m in zip(losses, plain)) > 0                        # the prior is part of every loss
    np.testing.assert_allclose(fused, losses, rtol=2e-3)


# ---- zero lambdas ---------------------------------------------------------------------------------------------
def _two_trainers(D, O, grid):
    from wire_amd.trainer import FusedTrainer
    return [FusedTrainer(_net("wire", D, O)[0], grid, None, lr=1e-3) for _ in range(2)]


def _assert_same_bits(a, b):
    torch.cuda.synchronize()
    assert a.flat_grad.cpu().numpy().tobytes() == b.flat_grad.cpu().numpy().tobytes()
    assert a.flat.cpu().numpy().tobytes() == b.flat.cpu().numpy().tobytes()
    assert a.loss.cpu().numpy().tobytes() == b.loss.cpu().numpy().tobytes()


def test_zero_lambdas_are_the_plain_steps_bit_for_bit():
    """step_downsampled(..., lambda_tv=0.0) and step_coded(..., lambda_tv=0.0, lambda_tv_t=0.0) leave the flat_grad,
    parameter and loss bits of the call without the keywords over two optimizer steps, and launch no TV kernel."""
    H, W, O = 24, 20, 3
    gt = torch.rand(12 * 10, O, generator=torch.Generator().manual_seed(3)).to(DEV)
    a, b = _two_trainers(2, O, (H, W))
    for _ in range(2):
        a.step_downsampled(gt, 2)
        b.step_downsampled(gt, 2, lambda_tv=0.0)
        _assert_same_bits(a, b)
    names = kernel_names(lambda: b.step_downsampled(gt, 2, lambda_tv=0.0))
    assert names and not any("tv_add" in k for k in names), names
    names = kernel_names(lambda: b.step_downsampled(gt, 2, lambda_tv=0.5))
    assert sum("tv_add_grad_kernel" in k for k in names) == 1 and sum("tv_add_final_kernel" in k for k in names) == 1

    H, W, T, nframes = 12, 10, 9, 4
    rng = np.random.default_rng(4)
    coded = torch.tensor(rng.uniform(0, 1, (4, H * W, 1)).astype(np.float32), device=DEV)
    mask = torch.tensor(vref.make_mask(rng, H * W, T), device=DEV)
    a, b = _two_trainers(3, 1, (H, W, T))
    for slab in (None, 50):
        for _ in range(2):
            a.step_coded(coded, mask, nframes, slab=slab)
            b.step_coded(coded, mask, nframes, slab=slab, lambda_tv=0.0, lambda_tv_t=0.0)
            _assert_same_bits(a, b)
    names = kernel_names(lambda: b.step_coded(coded, mask, nframes, lambda_tv=0.0, lambda_tv_t=0.0))
    assert names and not any("tv_add" in k for k in names), names
