"""GPU checks of the total-variation regulariser (utils.total_variation_loss, modules/utils.py:360-369): wire_tv_fwd /
wire_tv_bwd and the fused regularised loss wire_tv_mse_grad against the restatement of tests/tv_ref.py on every path of
their launchers, the drop-in utils.total_variation_loss against the value and the autograd gradient the reference itself
produced (tests/golden/tv.npz), and FusedTrainer.step_tv -- every parameter gradient against the fp64 oracle -- in both
GEMM families and for bspline_mscale_hier."""
import numpy as np
import pytest
import torch

from _util import kernel_names, load_golden, params_np, relmax, within_ref, _sd
import hier_ref as hr
import tv_ref as ref
from oracle import wire_oracle as wo

pytestmark = pytest.mark.gpu
DEV = torch.device("cuda:0")

# (H, W, O).  The launchers have no 2-D tiles: wire_tv_bwd and wire_tv_mse_grad run one thread per FLAT element in
# 256-element blocks (the plane index fastest on the channel-last layout, the pixel index fastest on the planar one), at
# most 1024 blocks, so a block loops above 262 144 elements; wire_tv_fwd runs one thread per PIXEL (the planes added in
# order), a block looping above 262 144 pixels.  A block boundary is wherever 256 elements (pixels) end.
#   (1, 1, 1)      no pair at all: 0 and a zero gradient
#   (1, 7, 2)      H == 1: horizontal pairs only
#   (7, 1, 3)      W == 1: vertical pairs only
#   (2, 2, 1)      every pixel is a corner
#   (5, 7, 3)      one ragged block; odd sizes, 3 planes
#   (33, 65, 1)    9 blocks whose boundaries fall inside rows (256 is no multiple of 65); ragged last block
#   (130, 70, 8)   the widest O; 285 blocks of elements, 36 of pixels; a pixel's 8 planes never straddle a block
#   (32, 16, 1)    two full blocks whose boundary IS a row boundary: every vertical pair of rows 15 / 16 crosses it
#   (20, 13, 3)    780 elements: block boundaries fall between the planes of one pixel (256 is no multiple of 3)
#   (512, 512, 1)  262 144 elements = 1024 full blocks: the last size at which no block loops
#   (300, 301, 3)  270 900 elements: blocks 0 .. 34 of the flat kernels loop a second time (90 300 pixels: fwd does not)
#   (513, 512, 1)  262 656 pixels: blocks 0, 1 of every kernel loop a second time
OP_SHAPES = [(1, 1, 1), (1, 7, 2), (7, 1, 3), (2, 2, 1), (5, 7, 3), (33, 65, 1), (130, 70, 8), (32, 16, 1),
             (20, 13, 3), (512, 512, 1), (300, 301, 3), (513, 512, 1)]
FILL = 7.0


def _draw(H, W, O, quantised, seed=0):
    """[H*W, O] standard normal; quantised to multiples of 0.25 so that ties (s(0)) are frequent."""
    y = np.random.default_rng(H * 1000 + W * 10 + O + seed).standard_normal((H * W, O)).astype(np.float32)
    return (np.round(y * 4) / 4).astype(np.float32) if quantised else y


def _lib():
    from wire_amd import _lib
    return _lib, _lib.lib()


def _stream():
    return torch.cuda.current_stream().cuda_stream


class _Layout:
    """An (O, H, W) image in device memory under one of the stride forms, and the way back."""

    def __init__(self, name, img):
        O, H, W = img.shape
        self.name, self.shape = name, (O, H, W)
        if name == "channel_last":                         # the network's own [H*W][O]
            self.buf = torch.tensor(np.ascontiguousarray(img.transpose(1, 2, 0)), device=DEV)
            self.ps, self.qs = O, 1
        elif name == "planar":                             # a contiguous (1, O, H, W)
            self.buf = torch.tensor(np.ascontiguousarray(img), device=DEV)
            self.ps, self.qs = 1, H * W
        else:                                              # "padded": [H*W][O + 1], the last column is not the image's
            b = np.full((H, W, O + 1), FILL, np.float32)
            b[..., :O] = img.transpose(1, 2, 0)
            self.buf = torch.tensor(b, device=DEV)
            self.ps, self.qs = O + 1, 1

    def image(self, buf):
        """(O, H, W) numpy view of a device buffer of this layout; the padding column of "padded" is checked."""
        O, H, W = self.shape
        a = buf.cpu().numpy()
        if self.name == "channel_last":
            return a.reshape(H, W, O).transpose(2, 0, 1)
        if self.name == "planar":
            return a.reshape(O, H, W)
        a = a.reshape(H, W, O + 1)
        assert (a[..., O] == FILL).all(), "wire_tv_bwd wrote between the addressed elements"
        return a[..., :O].transpose(2, 0, 1)


@pytest.mark.parametrize("quantised", [True, False])
@pytest.mark.parametrize("H,W,O", OP_SHAPES)
def test_tv_fwd_bwd_match_restatement(H, W, O, quantised):
    """wire_tv_fwd within 1e-5 relative of the fp64 restatement (the neighbouring operators' loss bound; the fp32
    restatement alone stays at <= 9e-8) and wire_tv_bwd with g_tv = 2^-2 bit-equal to it (every entry is k * g with
    |k| <= 4: exact), in the channel-last, the planar and a padded stride form; the three forms give the same forward bits;
    the same call twice gives the same bits; outputs are pre-filled with 7.0."""
    lib, L = _lib()
    img = ref.channel_first(_draw(H, W, O, quantised), H, W, O)
    tv64 = float(ref.total_variation(img, True))
    g = 0.25
    want = ref.total_variation_grad(img, g, double=False)
    assert want.dtype == np.float32
    if quantised and H * W >= 35:                                # ties are frequent: s(0) occurs
        assert (ref.tv_sign_pattern(img) == 0).any()
    part = torch.empty(1024, device=DEV)
    g_dev = torch.full((1,), g, device=DEV)
    bits = []
    for name in ("channel_last", "planar", "padded"):
        lay = _Layout(name, img)
        outs = []
        for _ in range(2):
            tv = torch.full((1,), FILL, device=DEV)
            gx = torch.full_like(lay.buf, FILL)
            lib.check(L.wire_tv_fwd(_stream(), lay.buf.data_ptr(), O, H, W, lay.ps, lay.qs, tv.data_ptr(),
                                    part.data_ptr()), "wire_tv_fwd")
            lib.check(L.wire_tv_bwd(_stream(), lay.buf.data_ptr(), O, H, W, lay.ps, lay.qs, g_dev.data_ptr(),
                                    gx.data_ptr()), "wire_tv_bwd")
            torch.cuda.synchronize()
            outs.append((tv.cpu().numpy(), lay.image(gx)))
        tvv = float(outs[0][0][0])
        err = abs(tvv - tv64) / tv64 if tv64 > 0 else abs(tvv)
        print(f"tv op {(H, W, O)} {name} quantised={quantised}: tv {tvv:.6e} rel {err:.2e}")
        assert err <= 1e-5
        assert np.ascontiguousarray(outs[0][1]).tobytes() == want.tobytes()
        assert outs[0][0].tobytes() == outs[1][0].tobytes()
        assert np.ascontiguousarray(outs[1][1]).tobytes() == want.tobytes()
        bits.append(outs[0][0].tobytes())
    assert bits[0] == bits[1] == bits[2]
    if (H, W, O) == (1, 1, 1):
        assert tvv == 0.0 and not want.any()


class _MseOp:
    """wire_tv_mse_grad on one image and target, uploaded once."""

    def __init__(self, y, t, H, W, O):
        self.lib, self.L = _lib()
        self.y, self.t, self.H, self.W, self.O = torch.tensor(y, device=DEV), torch.tensor(t, device=DEV), H, W, O
        self.part = torch.empty(2048, device=DEV)

    def call(self, lam, idx=None, first=0, n=0):
        gy, rec = torch.full_like(self.y, FILL), torch.full_like(self.y, FILL)
        out = torch.full((3,), FILL, device=DEV)
        ix = None if idx is None else torch.tensor(idx, device=DEV, dtype=torch.int64)
        self.lib.check(self.L.wire_tv_mse_grad(_stream(), self.y.data_ptr(), self.H, self.W, self.O, self.t.data_ptr(),
                                               None if ix is None else ix.data_ptr(), first, n, lam, gy.data_ptr(),
                                               out.data_ptr(), rec.data_ptr(), self.part.data_ptr()), "wire_tv_mse_grad")
        torch.cuda.synchronize()
        return out.cpu().numpy(), gy.cpu().numpy(), rec.cpu().numpy()


@pytest.mark.parametrize("quantised", [True, False])
@pytest.mark.parametrize("H,W,O", OP_SHAPES)
def test_tv_mse_grad_matches_restatement(H, W, O, quantised):
    """n_mse = 0 with lambda_tv = 2^-3: g_y bit-equal to the restatement, mse == 0 and loss == lambda * tv exactly.  All
    rows, a range that starts and ends mid-row and idx = a slice of a permutation, lambda_tv = fl32(0.3): loss 1e-5
    relative, g_y 1e-6 max|g64| absolute (the bounds of the neighbouring operators), the unselected rows the TV term alone
    bit for bit, rec exactly the selected rows; the same call twice gives the same bits."""
    n = H * W
    y = _draw(H, W, O, quantised)
    t = _draw(H, W, O, False, seed=5)
    op = _MseOp(y, t, H, W, O)
    lam = 0.125
    for idx in (None, np.zeros(1, np.int64)):          # n_mse = 0 with and without an index array
        out, gy, rec = op.call(lam, idx=idx)
        _, _, tv32, g32 = ref.tv_mse_loss_and_grad(y, t, [], lam, H, W, O, double=False)
        assert gy.tobytes() == g32.tobytes()
        assert out[1] == 0.0 and out[0] == np.float32(lam) * out[2]
        tv64 = float(ref.total_variation(ref.channel_first(y, H, W, O), True))
        assert abs(float(out[2]) - tv64) <= 1e-5 * tv64
        assert (rec == FILL).all()
    lam = float(np.float32(0.3))
    k = ref.tv_sign_pattern(ref.channel_first(y, H, W, O)).transpose(1, 2, 0).reshape(n, O).astype(np.float32)
    first = min(W // 2, n - 1)
    last = max(first + 1, n - (W - W // 3))                      # one past the range: mid-row when W > 2
    cases = {"all rows": (None, 0, n), "mid-row range": (None, first, last - first),
             "permutation slice": (np.random.default_rng(n).permutation(n)[:max(1, n * 5 // 8)], 0, None)}
    for label, (idx, a, cnt) in cases.items():
        rows = np.arange(a, a + cnt) if idx is None else idx
        out, gy, rec = op.call(lam, idx=idx, first=a, n=len(rows))
        l64, m64, tv64, g64 = ref.tv_mse_loss_and_grad(y, t, rows, lam, H, W, O, double=True)
        el = abs(float(out[0]) - l64) / l64
        eg = np.abs(gy - g64).max() / np.abs(g64).max()
        print(f"tv_mse_grad {(H, W, O)} quantised={quantised} {label} ({len(rows)} rows): loss rel {el:.2e}  "
              f"g_y / max|g64| {eg:.2e}  parts {out}")
        assert el <= 1e-5
        assert abs(float(out[1]) - m64) <= 1e-5 * m64 and abs(float(out[2]) - tv64) <= 1e-5 * max(tv64, 1e-30)
        assert out[0] == np.float32(out[1] + np.float32(np.float32(lam) * out[2]))
        np.testing.assert_allclose(gy, g64, rtol=0, atol=1e-6 * np.abs(g64).max())
        sel = np.zeros(n, bool)
        sel[rows] = True
        assert gy[~sel].tobytes() == (np.float32(lam) * k[~sel]).tobytes()
        assert rec[sel].tobytes() == y[sel].tobytes() and (rec[~sel] == FILL).all()
        again = op.call(lam, idx=idx, first=a, n=len(rows))
        assert all(p.tobytes() == q.tobytes() for p, q in zip((out, gy, rec), again))


# ---------------------------------------------------------------------------------------------------------------
# the drop-in function
# ---------------------------------------------------------------------------------------------------------------
def test_total_variation_loss_matches_golden():
    """utils.total_variation_loss on the golden image: the reference's value to 1e-6 relative, image.grad to
    1e-6 max|g| of the reference's own autograd; under no_grad the result has no graph; a float64 tensor is refused."""
    from wire_amd.modules import utils
    z = load_golden("tv")
    img = torch.tensor(z["image"], device=DEV, requires_grad=True)
    tv = utils.total_variation_loss(img)
    assert tv.dim() == 0 and tv.dtype == torch.float32 and tv.requires_grad
    tv.backward()
    torch.cuda.synchronize()
    err = abs(float(tv.item()) - float(z["tv"])) / float(z["tv"])
    eg = np.abs(img.grad.cpu().numpy() - z["grad"]).max() / np.abs(z["grad"]).max()
    print(f"total_variation_loss golden: value rel {err:.2e}  grad / max|g| {eg:.2e}")
    assert err <= 1e-6
    np.testing.assert_allclose(img.grad.cpu().numpy(), z["grad"], rtol=0, atol=1e-6 * np.abs(z["grad"]).max())
    # an upstream gradient scales it: (3 tv).backward()
    img2 = torch.tensor(z["image"], device=DEV, requires_grad=True)
    (3.0 * utils.total_variation_loss(img2)).backward()
    assert np.array_equal(img2.grad.cpu().numpy(), 3.0 * z["grad"])
    with torch.no_grad():
        quiet = utils.total_variation_loss(img)
    assert not quiet.requires_grad and quiet.grad_fn is None and quiet.item() == tv.item()
    with pytest.raises(ValueError, match="float32"):
        utils.total_variation_loss(img.detach().double())


def test_total_variation_loss_reads_the_permuted_view_in_place():
    """The drivers' model(coords).reshape(1, H, W, 3).permute(0, 3, 1, 2), a view over [H*W][O] memory, gives the bits of
    its contiguous copy, forward and backward, and launches no copy kernel: the two kernels of wire_tv_fwd and nothing
    else forward, one wire_tv_bwd kernel backward; a view whose strides do not fit is made contiguous and gives the same bits."""
    from wire_amd.modules import utils
    H, W, O = 37, 29, 3
    flat = torch.tensor(_draw(H, W, O, True), device=DEV)
    view = flat.reshape(1, H, W, O).permute(0, 3, 1, 2)
    assert not view.is_contiguous()
    copy = view.contiguous()
    a, b = view.clone().requires_grad_(True), copy.clone().requires_grad_(True)     # clone keeps the strides
    assert a.stride() == view.stride() and b.is_contiguous()
    ta, tb = utils.total_variation_loss(a), utils.total_variation_loss(b)
    ta.backward()
    tb.backward()
    assert ta.detach().cpu().numpy().tobytes() == tb.detach().cpu().numpy().tobytes()
    assert torch.equal(a.grad, b.grad)
    want = ref.total_variation_grad(ref.channel_first(flat.cpu().numpy(), H, W, O), 1.0, False)
    assert np.array_equal(a.grad[0].cpu().numpy(), want)
    with torch.no_grad():
        names = kernel_names(lambda: utils.total_variation_loss(view))
    names = [k for k in names if not k.startswith("hip")]         # device work: kernels and copies, not the runtime's calls
    print("total_variation_loss(view) launches:", names)
    assert names and all("tv_fwd_kernel" in k or "tv_final_kernel" in k for k in names), names
    assert sum("tv_fwd_kernel" in k for k in names) == 1 and sum("tv_final_kernel" in k for k in names) == 1

    def fwd_bwd():
        v = view.detach().requires_grad_(True)
        utils.total_variation_loss(v).backward(torch.ones((), device=DEV))
    names = kernel_names(fwd_bwd)
    print("total_variation_loss(view) + backward launches:", names)
    assert sum("tv_bwd_kernel" in k for k in names) == 1 and sum("tv_fwd_kernel" in k for k in names) == 1
    # every second column: W-stride 2 O but H-stride W O -- not of the (pix_stride, plane_stride) form
    odd = view[:, :, :, ::2]
    t_odd, t_c = utils.total_variation_loss(odd), utils.total_variation_loss(odd.contiguous())
    assert t_odd.cpu().numpy().tobytes() == t_c.cpu().numpy().tobytes()


# ---------------------------------------------------------------------------------------------------------------
# FusedTrainer.step_tv
# ---------------------------------------------------------------------------------------------------------------
def _net(kind, O):
    from wire_amd.modules import models
    torch.manual_seed(0)
    hp = (7.0, 7.0, 6.0) if kind == "wire" else (30.0, 30.0, 10.0)
    m = models.get_INR(nonlin=kind, in_features=2, out_features=O, hidden_features=128, hidden_layers=2,
                       first_omega_0=hp[0], hidden_omega_0=hp[1], scale=hp[2])
    return m.to(DEV), hp


def _pair_signs(y, H, W, O):
    img = ref.channel_first(y, H, W, O)
    sv = (img[:, 1:, :] > img[:, :-1, :]).astype(np.int8) - (img[:, 1:, :] < img[:, :-1, :]).astype(np.int8)
    sh = (img[:, :, 1:] > img[:, :, :-1]).astype(np.int8) - (img[:, :, 1:] < img[:, :, :-1]).astype(np.int8)
    return np.concatenate([sv.ravel(), sh.ravel()])


def _assert_few_flips(y_dev, y64, H, W, O, label):
    """The pairs whose sign in the trainer's fp32 image differs from the fp64 oracle's: at most 0.1 % of all pairs, so
    that taking the pattern from the trainer's image cannot hide a wrong image."""
    a, b = _pair_signs(y_dev, H, W, O), _pair_signs(y64, H, W, O)
    flips = int((a != b).sum())
    print(f"{label}: {flips} of {a.size} pairs differ in sign between self.y and the fp64 oracle")
    assert a.size == O * ((H - 1) * W + H * (W - 1))
    assert flips <= 1e-3 * a.size


def _tensors(model, tr):
    names = [k for k in model.state_dict().keys() if "omega_0" not in k and "scale_0" not in k]
    assert len(names) == len(tr.offsets)
    return list(zip(names, tr.offsets))


class _Case:
    """An lr = 0 trainer on an (H, W) grid with a target; the oracles run on the coordinates the trainer builds, their g_y
    takes the MSE term from their own forward and the TV sign pattern from the trainer's self.y."""

    def __init__(self, kind, H, W, O, seed, keep_rec=False):
        from wire_amd.trainer import FusedTrainer
        self.kind, self.H, self.W, self.O, self.n = kind, H, W, O, H * W
        self.model, self.hp = _net(kind, O)
        self.target = np.random.default_rng(seed).uniform(0, 1, (self.n, O)).astype(np.float32)
        self.tr = FusedTrainer(self.model, (H, W), torch.tensor(self.target), lr=0.0, keep_rec=keep_rec)

    def step(self, lam, **kw):
        loss = self.tr.step_tv(lam, **kw)
        torch.cuda.synchronize()
        self.y = self.tr.y[:self.n * self.O].cpu().numpy().reshape(self.n, self.O).copy()
        self.parts = self.tr.loss_parts.cpu().numpy().copy()
        return float(loss.item()), self.tr.flat_grad.cpu().numpy().copy()

    def oracle(self, lam, rows, double, check_flips=None):
        dt = np.float64 if double else np.float32
        p = wo.cast_params(params_np(self.model), double)
        a = tuple(dt(v) for v in self.hp)
        x = self.tr.coords[:self.n * 2].reshape(self.n, 2).cpu().numpy().astype(dt)
        if self.kind == "wire":
            y, cache = wo.wire_forward(p, x, 2, *a, keep=True)
        else:
            y, cache = wo.realnet_forward(self.kind, p, x, 2, *a, None, keep=True)
        if check_flips:
            _assert_few_flips(self.y, y, self.H, self.W, self.O, check_flips)
        loss, mse, tv, gy = ref.tv_mse_loss_and_grad(y, self.target, rows, lam, self.H, self.W, self.O, double,
                                                     pattern_from=self.y)
        gy = gy.reshape(y.shape).astype(dt)
        g = wo.wire_backward(p, cache, gy, 2, *a) if self.kind == "wire" else \
            wo.realnet_backward(self.kind, p, cache, gy, 2, *a)
        return float(loss), g, (float(mse), float(tv))


def _assert_bf16_bounds(c, loss, flat, l64, g64, label):
    """Loss 2e-5 relative, every gradient 5e-5 max|g| + 1e-10: the bounds of test_step_coded_bf16_family_matches_oracle."""
    for name, off in _tensors(c.model, c.tr):
        g = wo.as_real_pairs(g64[name]).astype(np.float64).ravel()
        print(f"{label}: {name} err / max|g| {np.abs(flat[off:off + g.size] - g).max() / np.abs(g).max():.2e}")
    print(f"{label}: loss {loss:.6e} rel {abs(loss - l64) / l64:.2e}")
    assert abs(loss - l64) <= 2e-5 * l64
    for name, off in _tensors(c.model, c.tr):
        g = wo.as_real_pairs(g64[name]).astype(np.float64).ravel()
        assert np.abs(flat[off:off + g.size] - g).max() <= 5e-5 * np.abs(g).max() + 1e-10, name


@pytest.fixture(scope="module")
def case_a():
    """Case (a): wire 2 x 128 (omega_0 = 7, s_0 = 6) on 24 x 20, O = 3 (480 rows, the 3 x bf16 family)."""
    return _Case("wire", 24, 20, 3, 21, keep_rec=True)


LAM_A = 2.0 ** -11        # near 1 / (H W O) = 1 / 1440: the two terms of g_y are of one size


def test_step_tv_bf16_family_matches_oracle(case_a):
    """Case (a) with all rows and with indices = perm[:300]: loss 2e-5 relative and every gradient 5e-5 max|g| + 1e-10
    against the fp64 oracle; loss_parts consistent with the loss; at most 0.1 % of the pairs differ in sign between
    self.y and the oracle; with keep_rec the selected rows of self.y go to self.rec."""
    c = case_a
    perm = np.random.default_rng(8).permutation(c.n)
    for label, rows, kw in (("all rows", np.arange(c.n), {}),
                            ("perm[:300]", perm[:300], dict(indices=torch.tensor(perm[:300], device=DEV)))):
        c.tr.rec.fill_(FILL)
        loss, flat = c.step(LAM_A, **kw)
        l64, g64, (m64, tv64) = c.oracle(LAM_A, rows, True, check_flips=f"step_tv (a) {label}")
        _assert_bf16_bounds(c, loss, flat, l64, g64, f"step_tv (a) {label}")
        assert np.abs(flat).max() > 0
        # the two terms of g_y are of one size, so neither hides behind the other
        gm = 2.0 * np.abs(c.y - c.target).max() / (len(rows) * c.O)
        print(f"step_tv (a) {label}: max MSE term of g_y {gm:.2e}, TV unit {LAM_A:.2e}; parts {c.parts}")
        assert 0.1 <= gm / LAM_A <= 10
        assert c.parts[0] == np.float32(loss) == np.float32(c.parts[1] + np.float32(np.float32(LAM_A) * c.parts[2]))
        assert abs(c.parts[1] - m64) <= 2e-5 * m64 and abs(c.parts[2] - tv64) <= 2e-5 * tv64
        rec = c.tr.rec.cpu().numpy()
        sel = np.zeros(c.n, bool)
        sel[rows] = True
        assert rec[sel].tobytes() == c.y[sel].tobytes() and (rec[~sel] == FILL).all()
    # a range is the same selection as its indices
    loss_r, flat_r = c.step(LAM_A, first=130, count=200)
    loss_i, flat_i = c.step(LAM_A, indices=torch.arange(130, 330, device=DEV))
    l64, g64, _ = c.oracle(LAM_A, np.arange(130, 330), True)
    _assert_bf16_bounds(c, loss_r, flat_r, l64, g64, "step_tv (a) rows 130..330")
    _assert_bf16_bounds(c, loss_i, flat_i, l64, g64, "step_tv (a) arange(130, 330)")


@pytest.mark.parametrize("kind", ["wire", "siren"])
def test_step_tv_fp16_family_within_reference_error(kind):
    """Case (b): 72 x 64, O = 3 (4 608 rows, above the 4 096-row switch to the 2 x fp16 family), lambda_tv = 2^-14: loss
    and every gradient within 3 x the error of the reference's own fp32 arithmetic (the fp32 oracle against fp64) + 1e-6,
    as test_step_coded_fp16_family_within_reference_error."""
    c = _Case(kind, 72, 64, 3, 22)
    lam = 2.0 ** -14
    loss, flat = c.step(lam)
    rows = np.arange(c.n)
    l64, g64, _ = c.oracle(lam, rows, True, check_flips=f"step_tv (b) {kind}")
    l32, g32, _ = c.oracle(lam, rows, False)
    checks = [(f"step_tv {kind} loss", abs(loss - l64) / l64, abs(l32 - l64) / l64)]
    for name, off in _tensors(c.model, c.tr):
        g = wo.as_real_pairs(g64[name]).astype(np.float64).ravel()
        r = wo.as_real_pairs(g32[name]).astype(np.float64).ravel()
        checks.append((f"step_tv {kind} {name}", relmax(flat[off:off + g.size], g), relmax(r, g)))
    for label, eb, er in checks:
        print(f"{label}: err_build {eb:.3e}  err_ref {er:.3e}  ratio {eb / er if er > 0 else float('inf'):.2f}")
    for label, eb, er in checks:
        within_ref(eb, er, label, factor=3.0)


def test_step_tv_zero_lambda_is_the_plain_mse_step(case_a):
    """Case (c): step_tv(0.0) on all rows against the oracle with no TV term (the plain full-grid MSE), at (a)'s bounds;
    loss_parts[0] == loss_parts[1] and tv is still reported."""
    c = case_a
    loss, flat = c.step(0.0)
    p = wo.cast_params(params_np(c.model), True)
    x = c.tr.coords[:c.n * 2].reshape(c.n, 2).cpu().numpy().astype(np.float64)
    y64, cache = wo.wire_forward(p, x, 2, *c.hp, keep=True)
    l64, gy = wo.mse_loss_and_grad(y64, c.target.astype(np.float64))
    g64 = wo.wire_backward(p, cache, gy, 2, *c.hp)
    _assert_bf16_bounds(c, loss, flat, float(l64), g64, "step_tv (c) lambda = 0")
    assert c.parts[0] == c.parts[1] and c.parts[2] > 0


def test_step_tv_hier_with_stage_rates():
    """Case (d): a bspline_mscale_hier trainer with one rate per stage takes a step, and its gradients (of the
    parameters before the step) meet (a)'s bounds against the fp64 closed form of tests/hier_ref.py -- driven with the
    pseudo-target t' = y64 - g_y H W O / 2, for which its MSE gradient 2 (y64 - t') / (H W O) is the regularised g_y."""
    from wire_amd.modules import models
    from wire_amd.trainer import FusedTrainer
    H, W, O, st, L = 24, 20, 3, [1 / 9, 4.0], 2
    n = H * W
    torch.manual_seed(0)
    model = models.get_INR(nonlin="bspline_mscale_hier", in_features=2, out_features=O, hidden_features=64,
                           scaled_hidden_features=0, hidden_layers=L, first_omega_0=-0.2, hidden_omega_0=-0.2,
                           scale=0.0, scale_tensor=st).to(DEV)
    target = np.random.default_rng(23).uniform(0, 1, (n, O)).astype(np.float32)
    tr = FusedTrainer(model, (H, W), torch.tensor(target), lr=[6e-3, 2e-2], niters=100)
    sd = _sd(model)
    heads = {}
    for s, lin in enumerate(model.linears):
        heads[f"linears.{s}.weight"] = lin.weight.detach().cpu().numpy().copy()
        heads[f"linears.{s}.bias"] = lin.bias.detach().cpu().numpy().copy()
    names = [k for k in sd if "scale_0" not in k] + list(heads)
    p0 = tr.flat.clone()
    lam = LAM_A
    loss = float(tr.step_tv(lam).item())
    torch.cuda.synchronize()
    assert not torch.equal(tr.flat, p0)                                   # both stages and their heads moved
    y_dev = tr.y[:n * O].cpu().numpy().reshape(n, O)
    x = tr.coords[:n * 2].reshape(n, 2).cpu().numpy().astype(np.float64)
    y64 = hr.forward(sd, heads, L, x, st, np.float64)
    _assert_few_flips(y_dev, y64, H, W, O, "step_tv (d) hier")
    l64, _, _, gy = ref.tv_mse_loss_and_grad(y64, target, np.arange(n), lam, H, W, O, True, pattern_from=y_dev)
    pseudo = y64 - gy * (n * O / 2.0)
    _, _, g64, _ = hr.loss_and_grads(sd, heads, L, x, pseudo, st, np.float64)
    flat = tr.flat_grad.cpu().numpy()
    print(f"step_tv (d) hier: loss {loss:.6e} rel {abs(loss - l64) / l64:.2e}")
    assert abs(loss - l64) <= 2e-5 * l64
    assert len(names) == len(tr.offsets)
    for k, off, sz in zip(names, tr.offsets, tr.sizes):
        g = g64[k].ravel()
        e = np.abs(flat[off:off + sz] - g).max()
        print(f"step_tv (d) hier: {k} err / max|g| {e / np.abs(g).max():.2e}")
    for k, off, sz in zip(names, tr.offsets, tr.sizes):
        g = g64[k].ravel()
        assert np.abs(flat[off:off + sz] - g).max() <= 5e-5 * np.abs(g).max() + 1e-10, k


def test_step_tv_refusals(case_a):
    """Case (e): a 3-D grid, a trainer built with target=None, indices that are not a 1-D contiguous CUDA int64 tensor, a
    range outside the grid and a non-finite lambda_tv raise ValueError naming the argument (world > 1 is checked on the
    host, tests/test_tv_host.py)."""
    from wire_amd.modules import models
    from wire_amd.trainer import FusedTrainer
    tr = case_a.tr
    m3 = models.get_INR(nonlin="wire", in_features=3, out_features=1, hidden_features=32, hidden_layers=1).to(DEV)
    with pytest.raises(ValueError, match="2-D grid"):
        FusedTrainer(m3, (4, 5, 6), torch.zeros(120, 1)).step_tv(0.1)
    m2 = models.get_INR(nonlin="wire", in_features=2, out_features=1, hidden_features=32, hidden_layers=1).to(DEV)
    with pytest.raises(ValueError, match="target"):
        FusedTrainer(m2, (4, 5), None).step_tv(0.1)
    good = torch.arange(10, device=DEV)
    for bad in (good.cpu(), good.int(), good.reshape(2, 5), torch.arange(20, device=DEV)[::2], good.float(),
                torch.arange(481, device=DEV)):
        with pytest.raises(ValueError, match="indices"):
            tr.step_tv(0.1, indices=bad)
    for kw in (dict(first=-1, count=3), dict(first=478, count=3), dict(first=481), dict(count=481)):
        with pytest.raises(ValueError, match="outside the grid"):
            tr.step_tv(0.1, **kw)
    for bad in (float("nan"), float("inf")):
        with pytest.raises(ValueError, match="lambda_tv"):
            tr.step_tv(bad)
    t0 = tr.t
    tr.step_tv(0.1, first=480, count=0)            # an empty range is legal: the TV term alone
    torch.cuda.synchronize()
    assert tr.t == t0 + 1 and float(tr.loss_parts[1]) == 0.0
