"""GPU checks of the video compressive-sensing step (modules/lin_inverse.py:42-95): the fused coded loss
(wire_coded_mse_grad) against the fp64 restatement of tests/video_cs_ref.py on every path of its launcher, the drop-in
lin_inverse.video2codedvideo against the coded video the reference makes (tests/golden/video_cs.npz), and
FusedTrainer.step_coded -- every parameter gradient against the fp64 oracle -- in both GEMM families and in slabs."""
import numpy as np
import pytest
import torch

from _util import load_golden, params_np, relmax, within_ref
import video_cs_ref as ref
from oracle import wire_oracle as wo

pytestmark = pytest.mark.gpu
DEV = torch.device("cuda:0")

# (H, W, T, O, nframes).  The launcher stages a tile of whole pixels in LDS while a pixel's T * O floats, padded to an
# odd stride, fit its 1024-float tile, one block per tile up to 1024 blocks, and runs a direct kernel otherwise:
#   (5, 7, 10, 1, 4)     one tile; ragged last chunk (frames 8, 9)
#   (6, 6, 8, 3, 4)      one tile; exact chunks, 3 channels
#   (3, 4, 5, 1, 8)      nframes > T: one chunk
#   (4, 5, 6, 2, 1)      nframes = 1: every frame its own chunk
#   (70, 90, 4, 1, 2)    31 tiles of 204 pixels, the last one ragged (180): one block per tile
#   (180, 180, 32, 1, 8) 1046 tiles of 31 pixels, more than the grid's 1024 blocks: a block loops over tiles
#   (2, 3, 341, 3, 64)   a pixel of 1023 floats: the widest staged span, one pixel per tile
#   (2, 3, 512, 2, 64)   a pixel of 1024 floats (padded 1025): the narrowest span of the direct kernel
#   (2, 3, 700, 2, 64)   a pixel of 1400 floats: the direct kernel, ragged last chunk
# (The direct kernel's own grid-stride loop starts at 262 144 (pixel, channel) pairs of more than 1024 floats each, over
#  1 GB of y: not a shape for this suite.)
OP_SHAPES = [(5, 7, 10, 1, 4), (6, 6, 8, 3, 4), (3, 4, 5, 1, 8), (4, 5, 6, 2, 1), (70, 90, 4, 1, 2),
             (180, 180, 32, 1, 8), (2, 3, 341, 3, 64), (2, 3, 512, 2, 64), (2, 3, 700, 2, 64)]


class _Op:
    """The operator's device inputs, uploaded once per case."""

    def __init__(self, y, mask, gt, NP, T, O, nframes, dup):
        from wire_amd import _lib
        self.lib, self.L = _lib, _lib.lib()
        self.y, self.mask, self.gt = (torch.tensor(a, device=DEV) for a in (y, mask, gt))
        self.NP, self.T, self.O, self.nframes, self.dup = NP, T, O, nframes, dup
        self.part = torch.empty(4096, device=DEV)

    def call(self, p0=0, n_pix=None, want_est=True, est=None, fill=7.0):
        """Pixels [p0, p0 + n_pix) -> (loss [1], g_y [n_pix*T, O] slab-local, est [C', NP, O] whole video)."""
        n_pix = self.NP if n_pix is None else n_pix
        T, O = self.T, self.O
        Cp = ref.nchunks(T, self.nframes) + self.dup
        gy = torch.full((n_pix * T, O), fill, device=DEV)
        if want_est and est is None:
            est = torch.full((Cp, self.NP, O), fill, device=DEV)
        loss = torch.zeros(1, device=DEV)
        ys = self.y.reshape(self.NP * T, O)[p0 * T:(p0 + n_pix) * T]
        assert ys.is_contiguous()
        self.lib.check(self.L.wire_coded_mse_grad(torch.cuda.current_stream().cuda_stream, ys.data_ptr(), p0, n_pix,
                                                  self.NP, T, O, self.nframes, self.dup, self.mask.data_ptr(),
                                                  self.gt.data_ptr(), gy.data_ptr(),
                                                  est.data_ptr() if want_est else None, loss.data_ptr(),
                                                  self.part.data_ptr()), "coded_mse_grad")
        torch.cuda.synchronize()
        return loss.cpu().numpy(), gy.cpu().numpy(), est.cpu().numpy() if want_est else None


@pytest.mark.parametrize("dup", [1, 0])
@pytest.mark.parametrize("H,W,T,O,nframes", OP_SHAPES)
def test_coded_loss_operator_matches_restatement(H, W, T, O, nframes, dup):
    """Loss relative 1e-5, g_y absolute 1e-6 max|g64|, est absolute 1e-6 max|est64| (est is a sum of up to 64 terms, not
    a mean) -- the bounds of the neighbouring operator's test; the fp32 restatement alone stays at <= 1.5e-7 on these
    measures.  g_y and est are pre-filled with 7.0 so that an unwritten element shows."""
    rng = np.random.default_rng(H * 1000 + W + T)
    NP = H * W
    Cp = ref.nchunks(T, nframes) + dup
    y = rng.standard_normal((NP * T, O)).astype(np.float32)
    gt = rng.standard_normal((Cp, NP, O)).astype(np.float32)
    mask = ref.make_mask(rng, NP, T)
    l64, g64, e64 = ref.coded_loss_and_grad(y, mask, gt, T, nframes, dup, double=True)
    op = _Op(y, mask, gt, NP, T, O, nframes, dup)
    loss, gy, est = op.call()
    el = abs(float(loss[0]) - l64) / l64
    eg, ee = np.abs(gy - g64).max() / np.abs(g64).max(), np.abs(est - e64).max() / np.abs(e64).max()
    print(f"coded op {(H, W, T, O, nframes)} dup={dup}: loss rel {el:.2e}  g_y / max|g64| {eg:.2e}  "
          f"est / max|est64| {ee:.2e}")
    assert el <= 1e-5
    np.testing.assert_allclose(gy, g64, rtol=0, atol=1e-6 * np.abs(g64).max())
    np.testing.assert_allclose(est, e64, rtol=0, atol=1e-6 * np.abs(e64).max())
    if dup:
        assert np.array_equal(est[-1], est[-2])
    # a pixel whose mask is zero in every frame receives exactly no gradient (make_mask closes pixel 0)
    assert not mask[0].any() and not gy[:T].any()
    # the same call twice: the same bits
    again = op.call()
    assert loss.tobytes() == again[0].tobytes() and gy.tobytes() == again[1].tobytes() \
        and est.tobytes() == again[2].tobytes()
    # est == NULL: the same loss and g_y bits
    noest = op.call(want_est=False)
    assert loss.tobytes() == noest[0].tobytes() and gy.tobytes() == noest[1].tobytes()
    # two slabs: g_y bit-equal to the one-pass rows, est filled between them, losses that add up
    n1 = max(1, NP // 3)
    est2 = torch.full((Cp, NP, O), 7.0, device=DEV)
    la, ga, _ = op.call(0, n1, est=est2)
    lb, gb, es = op.call(n1, NP - n1, est=est2)
    assert ga.tobytes() == gy[:n1 * T].tobytes() and gb.tobytes() == gy[n1 * T:].tobytes()
    assert es.tobytes() == est.tobytes()
    lsum = float(la[0]) + float(lb[0])
    print(f"coded op {(H, W, T, O, nframes)} dup={dup}: slab losses {float(la[0]):.6e} + {float(lb[0]):.6e} "
          f"vs {float(loss[0]):.6e}")
    assert abs(lsum - float(loss[0])) <= 1e-6 * float(loss[0])


def test_video2codedvideo_matches_golden_and_adjoint():
    """lin_inverse.video2codedvideo on the golden video and masks == the coded video the reference made, to 1e-6 max; its
    backward == the restatement's adjoint for a random g_coded at 1e-6 max|g64|; dup_last=False drops the last frame; the
    gradient flows to the video only."""
    from wire_amd.modules import lin_inverse
    z = load_golden("video_cs")
    H, W, T = (int(v) for v in z["video_size"])
    nframes = int(z["nframes"])
    C = ref.nchunks(T, nframes)
    masks = torch.tensor(z["masks"].astype(np.float32)).permute(2, 0, 1)[None].to(DEV)          # (1, T, H, W)
    for dup in (True, False):
        video = torch.tensor(z["video"], device=DEV, requires_grad=True)
        mk = masks.clone().requires_grad_(True)
        coded = lin_inverse.video2codedvideo(video, mk, nframes) if dup else \
            lin_inverse.video2codedvideo(video, mk, nframes, dup_last=False)
        assert coded.shape == (1, C + int(dup), H, W) and coded.dtype == torch.float32
        want = z["coded"][:, :C + int(dup)]
        err = np.abs(coded.detach().cpu().numpy() - want).max() / np.abs(want).max()
        print(f"video2codedvideo dup_last={dup}: err / max {err:.2e}")
        assert err <= 1e-6
        g = np.random.default_rng(4).standard_normal(tuple(coded.shape)).astype(np.float32)
        coded.backward(torch.tensor(g, device=DEV))
        g64 = ref.coded_adjoint(g[0].reshape(C + int(dup), H * W), masks[0].cpu().numpy().reshape(T, H * W), T,
                                nframes, dup)
        got = video.grad.cpu().numpy()[0].reshape(T, H * W)
        print(f"video2codedvideo backward dup_last={dup}: err / max|g64| {np.abs(got - g64).max() / np.abs(g64).max():.2e}")
        np.testing.assert_allclose(got, g64, rtol=0, atol=1e-6 * np.abs(g64).max())
        assert mk.grad is None
    with pytest.raises(ValueError):
        lin_inverse.video2codedvideo(masks[0], masks[0], nframes)
    with pytest.raises(ValueError):
        lin_inverse.video2codedvideo(masks, masks[:, :-1], nframes)


# ---------------------------------------------------------------------------------------------------------------
# FusedTrainer.step_coded
# ---------------------------------------------------------------------------------------------------------------
def _net(kind, O):
    from wire_amd.modules import models
    torch.manual_seed(0)
    hp = (7.0, 7.0, 6.0) if kind == "wire" else (30.0, 30.0, 10.0)
    m = models.get_INR(nonlin=kind, in_features=3, out_features=O, hidden_features=128, hidden_layers=2,
                       first_omega_0=hp[0], hidden_omega_0=hp[1], scale=hp[2])
    return m.to(DEV), hp


def _oracle(kind, P, hp, coords, T, nframes, dup, gt, mask, double):
    """Forward of the numpy oracle on the trainer's rows, the restatement of the coded loss, the oracle's backward."""
    dt = np.float64 if double else np.float32
    p = wo.cast_params(P, double)
    a = tuple(dt(v) for v in hp)
    x = coords.astype(dt)
    if kind == "wire":
        y, cache = wo.wire_forward(p, x, 2, *a, keep=True)
    else:
        y, cache = wo.realnet_forward(kind, p, x, 2, *a, None, keep=True)
    loss, gy, _ = ref.coded_loss_and_grad(y, mask, gt, T, nframes, dup, double=double)
    gy = gy.reshape(y.shape).astype(dt)
    g = wo.wire_backward(p, cache, gy, 2, *a) if kind == "wire" else wo.realnet_backward(kind, p, cache, gy, 2, *a)
    return float(loss), g


def _tensors(model, tr):
    names = [k for k in model.state_dict().keys() if "omega_0" not in k and "scale_0" not in k]
    assert len(names) == len(tr.offsets)
    return list(zip(names, tr.offsets))


class _Case:
    """An lr = 0 trainer on an (H, W, T) grid with a coded target and masks; the oracles are computed once, on the
    coordinates the trainer builds."""

    def __init__(self, kind, H, W, T, O, nframes, seed, dup=True):
        from wire_amd.trainer import FusedTrainer
        self.kind, self.grid, self.T, self.O, self.nframes, self.dup = kind, (H, W, T), T, O, nframes, dup
        rng = np.random.default_rng(seed)
        self.NP = H * W
        self.Cp = ref.nchunks(T, nframes) + int(dup)
        self.model, self.hp = _net(kind, O)
        self.tr = FusedTrainer(self.model, self.grid, None, lr=0.0)
        self.gt = rng.uniform(0, 1, (self.Cp, self.NP, O)).astype(np.float32)
        self.mask = ref.make_mask(rng, self.NP, T)
        self.gt_dev = torch.tensor(self.gt, device=DEV)
        self.mask_dev = torch.tensor(self.mask, device=DEV)

    def step(self, **kw):
        loss = self.tr.step_coded(self.gt_dev, kw.pop("masks", self.mask_dev), self.nframes, dup_last=self.dup, **kw)
        torch.cuda.synchronize()
        return float(loss.item()), self.tr.flat_grad.cpu().numpy().copy()

    def coords(self):
        """The rows of the last one-pass step."""
        n = self.NP * self.T
        return self.tr.coords[:n * 3].reshape(n, 3).cpu().numpy()

    def oracle(self, double):
        return _oracle(self.kind, params_np(self.model), self.hp, self.coords(), self.T, self.nframes, self.dup,
                       self.gt, self.mask, double)


@pytest.fixture(scope="module")
def case_a():
    """Case (a): wire 2 x 128 (omega_0 = 7, s_0 = 6) on 12 x 10 x 9 (1 080 rows, the 3 x bf16 family), nframes 4 (a
    ragged last chunk of one frame), O = 1: the one-pass step and the fp64 oracle, shared by the tests below."""
    c = _Case("wire", 12, 10, 9, 1, 4, 11)
    c.loss, c.flat = c.step()
    c.y = c.tr.y[:c.NP * c.T * c.O].cpu().numpy().copy()
    c.l64, c.g64 = c.oracle(True)
    return c


def _assert_case_a(c, loss, flat, label):
    worst = 0.0
    for name, off in _tensors(c.model, c.tr):
        g = wo.as_real_pairs(c.g64[name]).astype(np.float64).ravel()
        e = np.abs(flat[off:off + g.size] - g).max() / np.abs(g).max()
        worst = max(worst, e)
        print(f"{label}: {name} err / max|g| {e:.2e}")
    print(f"{label}: loss rel {abs(loss - c.l64) / c.l64:.2e}  worst gradient {worst:.2e}")
    assert abs(loss - c.l64) <= 2e-5 * c.l64
    for name, off in _tensors(c.model, c.tr):
        g = wo.as_real_pairs(c.g64[name]).astype(np.float64).ravel()
        assert np.abs(flat[off:off + g.size] - g).max() <= 5e-5 * np.abs(g).max() + 1e-10, name


def test_step_coded_bf16_family_matches_oracle(case_a):
    """Case (a): loss 2e-5 relative and every gradient 5e-5 max|g| + 1e-10 against the fp64 oracle -- the bounds of
    test_step_frames_bf16_family_matches_oracle."""
    _assert_case_a(case_a, case_a.loss, case_a.flat, "step_coded (a)")
    assert np.abs(case_a.flat).max() > 0


@pytest.mark.parametrize("kind", ["wire", "siren"])
def test_step_coded_fp16_family_within_reference_error(kind):
    """Case (b): 24 x 24 x 8 (4 608 rows, above the 4 096-row switch to the 2 x fp16 family), nframes 4, O = 3: loss and
    every gradient within 3 x the error of the reference's own fp32 arithmetic (the fp32 oracle and restatement against
    fp64) + 1e-6, as test_step_frames_fp16_family_within_reference_error."""
    c = _Case(kind, 24, 24, 8, 3, 4, 12)
    loss, flat = c.step()
    l64, g64 = c.oracle(True)
    l32, g32 = c.oracle(False)
    checks = [(f"step_coded {kind} loss", abs(loss - l64) / l64, abs(l32 - l64) / l64)]
    for name, off in _tensors(c.model, c.tr):
        g = wo.as_real_pairs(g64[name]).astype(np.float64).ravel()
        r = wo.as_real_pairs(g32[name]).astype(np.float64).ravel()
        checks.append((f"step_coded {kind} {name}", relmax(flat[off:off + g.size], g), relmax(r, g)))
    for label, eb, er in checks:
        print(f"{label}: err_build {eb:.3e}  err_ref {er:.3e}  ratio {eb / er if er > 0 else float('inf'):.2f}")
    for label, eb, er in checks:
        within_ref(eb, er, label, factor=3.0)


def test_step_coded_slabs(case_a):
    """Case (c): slab=50 (does not divide the 120 pixels) meets the bounds of (a); slab=120 is the one-pass path, bit for
    bit; est= receives the coded estimate of the step's video; the numpy masks of get_video_coding_frames' kind are
    uploaded once and give the bits of the device tensor."""
    c = case_a
    loss50, flat50 = c.step(slab=50)
    _assert_case_a(c, loss50, flat50, "step_coded (c) slab=50")
    loss120, flat120 = c.step(slab=120)
    assert loss120 == c.loss and flat120.tobytes() == c.flat.tobytes()
    lossbig, flatbig = c.step(slab=1000)
    assert lossbig == c.loss and flatbig.tobytes() == c.flat.tobytes()
    est = torch.full((c.Cp, c.NP, c.O), 7.0, device=DEV)
    c.step(est=est)
    e64 = ref.coded_estimate(c.y, c.mask, c.T, c.nframes, c.dup, double=True)
    got = est.cpu().numpy()
    print(f"step_coded (c) est: err / max {np.abs(got - e64).max() / np.abs(e64).max():.2e}")
    np.testing.assert_allclose(got, e64, rtol=0, atol=1e-6 * np.abs(e64).max())
    # in slabs est is filled as well
    est50 = torch.full((c.Cp, c.NP, c.O), 7.0, device=DEV)
    c.step(slab=50, est=est50)
    np.testing.assert_allclose(est50.cpu().numpy(), e64, rtol=0, atol=1e-6 * np.abs(e64).max())
    # a host array in (H, W, T) order, float64 as get_video_coding_frames returns it
    host = c.mask.astype(np.float64).reshape(c.grid)
    lossh, flath = c.step(masks=host)
    assert lossh == c.loss and flath.tobytes() == c.flat.tobytes()
    dev_masks = c.tr._coded_masks_dev
    c.step(masks=host)
    assert c.tr._coded_masks_dev is dev_masks


def test_step_coded_refusals(case_a):
    """Case (d): a 2-D trainer, a wrong coded or masks size and nframes = 0 raise ValueError."""
    from wire_amd.modules import models
    from wire_amd.trainer import FusedTrainer
    c = case_a
    m2 = models.get_INR(nonlin="wire", in_features=2, out_features=1, hidden_features=32, hidden_layers=1).to(DEV)
    tr2 = FusedTrainer(m2, (12, 10), None)
    with pytest.raises(ValueError, match="3-D"):
        tr2.step_coded(c.gt_dev, c.mask_dev, 4)
    with pytest.raises(ValueError, match="coded"):
        c.tr.step_coded(c.gt_dev[:-1], c.mask_dev, 4)
    with pytest.raises(ValueError, match="coded"):
        c.tr.step_coded(c.gt_dev, c.mask_dev, 4, dup_last=False)
    with pytest.raises(ValueError, match="coded"):
        c.tr.step_coded(c.gt_dev.double(), c.mask_dev, 4)
    with pytest.raises(ValueError, match="masks"):
        c.tr.step_coded(c.gt_dev, c.mask_dev[:-1], 4)
    with pytest.raises(ValueError, match="masks"):
        c.tr.step_coded(c.gt_dev, c.mask[:-1], 4)
    with pytest.raises(ValueError, match="masks"):
        c.tr.step_coded(c.gt_dev, c.mask_dev.cpu(), 4)
    with pytest.raises(ValueError, match="nframes"):
        c.tr.step_coded(c.gt_dev, c.mask_dev, 0)
    with pytest.raises(ValueError, match="est"):
        c.tr.step_coded(c.gt_dev, c.mask_dev, 4, est=torch.zeros(3, device=DEV))
    with pytest.raises(ValueError, match="slab"):
        c.tr.step_coded(c.gt_dev, c.mask_dev, 4, slab=0)
