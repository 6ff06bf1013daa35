"""GPU checks of the multi-image super-resolution step (wire_multi_sr.py:190-208): the masked, batched pooled loss
(wire_avgpool_mse_grad_frames) and the frames' coordinates (wire_affine_coords) against the fp64 restatement of
tests/multi_sr_ref.py, and FusedTrainer.step_frames -- every parameter gradient against the fp64 oracle -- in both GEMM
families."""
import ctypes as C

import numpy as np
import pytest
import torch

from _util import params_np, relmax, within_ref
import multi_sr_ref as ref
from oracle import wire_oracle as wo

pytestmark = pytest.mark.gpu
DEV = torch.device("cuda:0")

# (B, H, W, O, scale).  The first two are the shapes the loss is specified on: ragged in both directions (one strip tile
# per frame row), and exact with one output.  The others are the smallest shapes of the kernel's remaining paths:
# two column tiles per strip with a ragged right border in the second (1024 / (4 * 3) = 85 pooled columns per tile),
# more strips than the grid's 1024 blocks (a block loops over strips), and a window row wider than the LDS tile
# (scale * O = 1050 > 1024 floats: the direct kernel, with the launcher zeroing the borders).
OP_SHAPES = [(3, 10, 13, 3, 4), (2, 24, 24, 1, 3), (1, 9, 350, 3, 4), (2, 600, 5, 1, 1), (2, 40, 37, 30, 35)]


def _frames_call(y, B, H, W, O, scale, gt, mask, fill=7.0, want_rec=True):
    from wire_amd import _lib
    L = _lib.lib()
    H2, W2 = H // scale, W // scale
    yt, gtt = torch.tensor(y, device=DEV), torch.tensor(gt, device=DEV)
    mt = torch.tensor(mask, device=DEV) if mask is not None else None
    gy = torch.full((B, H * W, O), fill, device=DEV)
    rec = torch.full((B, H2 * W2, O), fill, device=DEV) if want_rec else None
    loss = torch.zeros(1, device=DEV)
    part = torch.empty(4096, device=DEV)
    stream = torch.cuda.current_stream().cuda_stream
    _lib.check(L.wire_avgpool_mse_grad_frames(stream, yt.data_ptr(), B, H, W, O, scale, gtt.data_ptr(),
                                              mt.data_ptr() if mt is not None else None, gy.data_ptr(),
                                              rec.data_ptr() if rec is not None else None, loss.data_ptr(),
                                              part.data_ptr()), "frames")
    torch.cuda.synchronize()
    return loss.cpu().numpy(), gy.cpu().numpy(), rec.cpu().numpy() if rec is not None else None


@pytest.mark.parametrize("B,H,W,O,scale", OP_SHAPES)
def test_frames_loss_operator_matches_restatement(B, H, W, O, scale):
    """Loss relative 1e-5, g_y absolute 1e-6 max|g64|, rec_lr absolute 2e-6 -- the bounds of
    test_super_resolution_step_matches_oracle (the arithmetic is the same plus one exact multiply).  g_y is pre-filled
    with 7.0 so that an unwritten border pixel shows; mask NULL == a mask of ones, and the same call twice, bit for bit."""
    rng = np.random.default_rng(B * 1000 + H + W)
    H2, W2 = H // scale, W // scale
    y = rng.standard_normal((B, H * W, O)).astype(np.float32)
    gt = rng.standard_normal((B, H2 * W2, O)).astype(np.float32)
    m = ref.make_mask(rng, B, H2 * W2, O)
    for mask in (m, None):
        l64, g64, r64 = ref.frames_loss_and_grad(y, B, H, W, scale, gt, mask, double=True)
        loss, gy, rec = _frames_call(y, B, H, W, O, scale, gt, mask)
        el, eg, er = abs(float(loss[0]) - l64) / l64, np.abs(gy - g64).max() / np.abs(g64).max(), np.abs(rec - r64).max()
        print(f"frames op {(B, H, W, O, scale)} mask={'yes' if mask is not None else 'NULL'}: loss rel {el:.2e}  "
              f"g_y / max|g64| {eg:.2e}  rec abs {er:.2e}")
        assert el <= 1e-5
        np.testing.assert_allclose(gy, g64, rtol=0, atol=1e-6 * np.abs(g64).max())
        np.testing.assert_allclose(rec, r64, rtol=0, atol=2e-6)
        # the ragged borders hold exactly 0 (not 7.0, not -0.0 + something)
        g4 = gy.reshape(B, H, W, O)
        assert not g4[:, H2 * scale:].any() and not g4[:, :, W2 * scale:].any()
        again = _frames_call(y, B, H, W, O, scale, gt, mask)
        assert loss.tobytes() == again[0].tobytes() and gy.tobytes() == again[1].tobytes() \
            and rec.tobytes() == again[2].tobytes()
        if mask is None:
            ones = _frames_call(y, B, H, W, O, scale, gt, np.ones_like(gt), want_rec=False)
            assert loss.tobytes() == ones[0].tobytes() and gy.tobytes() == ones[1].tobytes()
    # a frame that is masked entirely receives no gradient at all
    if B > 1:
        _, gy, _ = _frames_call(y, B, H, W, O, scale, gt, m)
        assert not gy[-1].any()


def _mats(thetas, shifts):
    from wire_amd.modules import motion
    return np.stack([motion.getEuclidianMatrix(t, s) for t, s in zip(thetas, shifts)])


def test_affine_coords_match_restatement():
    """B = 3 frames of 16 x 24, theta in {0, pi/10, -pi/12}, shifts up to +-20 pixels: every value within one fp32 ulp
    of the fp64 restatement; frame 0 (the identity) bit-equal to 2 j / W - 1, 2 i / H - 1 cast to fp32."""
    from wire_amd import _lib
    L = _lib.lib()
    B, H, W = 3, 16, 24
    mats = _mats([0.0, np.pi / 10, -np.pi / 12], [(0, 0), (20, -13), (-20, 7)])
    mt = torch.tensor(mats, dtype=torch.float64, device=DEV)
    out = torch.full((B, H * W, 2), 7.0, device=DEV)
    _lib.check(L.wire_affine_coords(torch.cuda.current_stream().cuda_stream, mt.data_ptr(), B, H, W, out.data_ptr()))
    torch.cuda.synchronize()
    got = out.cpu().numpy()
    want = ref.affine_coords(mats, H, W)
    ulp = np.spacing(np.abs(want).astype(np.float32)).astype(np.float64)
    print(f"affine coords: worst error {np.abs(got - want).max():.3e}, in ulp {(np.abs(got - want) / ulp).max():.3f}")
    assert (np.abs(got.astype(np.float64) - want) <= ulp).all()
    i, j = np.mgrid[:H, :W]
    assert got[0, :, 0].tobytes() == (2.0 * j / W - 1).astype(np.float32).tobytes()
    assert got[0, :, 1].tobytes() == (2.0 * i / H - 1).astype(np.float32).tobytes()
    # the trainer's wrapper is the same call
    from wire_amd.modules import models
    from wire_amd.trainer import FusedTrainer
    model = models.get_INR(nonlin="wire", in_features=2, out_features=3, hidden_features=32, hidden_layers=1).to(DEV)
    c = FusedTrainer(model, (H, W), None).affine_coords(mats)
    assert c.shape == (B, H * W, 2) and c.dtype == torch.float32 and c.is_contiguous()
    assert c.cpu().numpy().tobytes() == got.tobytes()


def _net(kind, O):
    from wire_amd.modules import models
    torch.manual_seed(0)
    if kind == "wire":
        hp = (7.0, 7.0, 6.0)
        m = models.get_INR(nonlin="wire", in_features=2, out_features=O, hidden_features=128, hidden_layers=2,
                           first_omega_0=hp[0], hidden_omega_0=hp[1], scale=hp[2])
    else:
        hp = (30.0, 30.0, 10.0)
        m = models.get_INR(nonlin="siren", in_features=2, out_features=O, hidden_features=128, hidden_layers=2,
                           first_omega_0=hp[0], hidden_omega_0=hp[1], scale=hp[2])
    return m.to(DEV), hp


def _oracle(kind, P, hp, coords, B, H, W, scale, gt, mask, double):
    """Forward of the numpy oracle on the frames' rows, the restatement of the loss, the oracle's backward."""
    dt = np.float64 if double else np.float32
    p = wo.cast_params(P, double)
    a = tuple(dt(v) for v in hp)
    x = coords.reshape(-1, 2).astype(dt)
    if kind == "wire":
        y, cache = wo.wire_forward(p, x, 2, *a, keep=True)
    else:
        y, cache = wo.realnet_forward(kind, p, x, 2, *a, None, keep=True)
    loss, gy, _ = ref.frames_loss_and_grad(y, B, H, W, scale, gt, mask, double=double)
    gy = gy.reshape(y.shape).astype(dt)
    g = wo.wire_backward(p, cache, gy, 2, *a) if kind == "wire" else wo.realnet_backward(kind, p, cache, gy, 2, *a)
    return float(loss), g


def _step_case(kind, B, H, W, scale, seed):
    """One lr = 0 step_frames on rigidly moved frames -> (trainer, model, loss, flat gradient, inputs)."""
    from wire_amd.trainer import FusedTrainer
    O = 3
    rng = np.random.default_rng(seed)
    H2, W2 = H // scale, W // scale
    model, hp = _net(kind, O)
    tr = FusedTrainer(model, (H, W), None, lr=0.0)
    thetas = [0.0, np.pi / 10, -np.pi / 12][:B]
    shifts = [(0, 0), (3, -2), (-4, 1)][:B]
    coords = tr.affine_coords(_mats(thetas, shifts))
    gt = rng.uniform(0, 1, (B, H2 * W2, O)).astype(np.float32)
    mask = ref.make_mask(rng, B + 1, H2 * W2, O)[:B]           # zeros, halves and ones in every frame
    loss = tr.step_frames(coords, torch.tensor(gt, device=DEV), scale, mask=torch.tensor(mask, device=DEV))
    torch.cuda.synchronize()
    return tr, model, hp, float(loss.item()), tr.flat_grad.cpu().numpy().copy(), coords.cpu().numpy(), gt, mask


def _tensors(model, tr):
    names = [k for k in model.state_dict().keys() if "omega_0" not in k and "scale_0" not in k]
    assert len(names) == len(tr.offsets)
    return list(zip(names, tr.offsets))


def test_step_frames_bf16_family_matches_oracle():
    """Case (a): wire 2 x 128 (omega_0 = 7, s_0 = 6), B = 3 frames of 26 x 21, scale 4, a mask with zeros: 1 638 rows, the
    3 x bf16 family.  Loss 2e-5 relative and every gradient 5e-5 max|g| + 1e-10 against the fp64 oracle -- the bounds of
    test_super_resolution_step_matches_oracle."""
    B, H, W, scale = 3, 26, 21, 4
    tr, model, hp, loss, flat, coords, gt, mask = _step_case("wire", B, H, W, scale, 5)
    assert (mask == 0).any()
    l64, g64 = _oracle("wire", params_np(model), hp, coords, B, H, W, scale, gt, mask, True)
    print(f"step_frames (a): loss rel {abs(loss - l64) / l64:.2e}")
    worst = {}
    for name, off in _tensors(model, tr):
        g = wo.as_real_pairs(g64[name]).astype(np.float64).ravel()
        worst[name] = np.abs(flat[off:off + g.size] - g).max() / np.abs(g).max()
        print(f"step_frames (a): {name} err / max|g| {worst[name]:.2e}")
    assert abs(loss - l64) <= 2e-5 * l64
    for name, off in _tensors(model, tr):
        g = wo.as_real_pairs(g64[name]).astype(np.float64).ravel()
        assert np.abs(flat[off:off + g.size] - g).max() <= 5e-5 * np.abs(g).max() + 1e-10, name
    # the high-resolution frames stay in tr.y
    assert tr.y.numel() >= B * H * W * 3


@pytest.mark.parametrize("kind", ["wire", "siren"])
def test_step_frames_fp16_family_within_reference_error(kind):
    """Case (b): B = 2 frames of 48 x 48, scale 4: 4 608 rows, above the 4 096-row switch to the 2 x fp16 family that the
    driver's size runs.  Loss and every gradient within 3 x the error of the reference's own fp32 arithmetic (the fp32
    oracle and restatement against fp64) + 1e-6 -- the bound test_random_shapes_against_oracle uses for nets of a few
    thousand rows, for the reason its docstring gives."""
    B, H, W, scale = 2, 48, 48, 4
    tr, model, hp, loss, flat, coords, gt, mask = _step_case(kind, B, H, W, scale, 6)
    P = params_np(model)
    l64, g64 = _oracle(kind, P, hp, coords, B, H, W, scale, gt, mask, True)
    l32, g32 = _oracle(kind, P, hp, coords, B, H, W, scale, gt, mask, False)
    checks = [(f"step_frames {kind} loss", abs(loss - l64) / l64, abs(l32 - l64) / l64)]
    for name, off in _tensors(model, tr):
        g = wo.as_real_pairs(g64[name]).astype(np.float64).ravel()
        r = wo.as_real_pairs(g32[name]).astype(np.float64).ravel()
        checks.append((f"step_frames {kind} {name}", relmax(flat[off:off + g.size], g), relmax(r, g)))
    for label, eb, er in checks:
        print(f"{label}: err_build {eb:.3e}  err_ref {er:.3e}  ratio {eb / er if er > 0 else float('inf'):.2f}")
    for label, eb, er in checks:
        within_ref(eb, er, label, factor=3.0)


def test_step_frames_smaller_last_batch_and_no_target():
    """A second call with B = 1 after B = 3 gives the gradients of a fresh trainer at B = 1 (buffers are reserved for
    the largest B seen); with target=None step_frames runs and step / step_hashed / psnr without gt raise ValueError."""
    from wire_amd.modules import models
    from wire_amd.trainer import FusedTrainer
    H, W, scale, O = 12, 10, 2, 3
    rng = np.random.default_rng(8)
    mats = _mats([0.0, 0.2, -0.1], [(0, 0), (2, 1), (-1, 3)])
    gt = torch.tensor(rng.uniform(0, 1, (3, (H // scale) * (W // scale), O)).astype(np.float32), device=DEV)
    mask = torch.tensor(ref.make_mask(rng, 4, (H // scale) * (W // scale), O)[:3], device=DEV)

    def fresh():
        torch.manual_seed(3)
        model = models.get_INR(nonlin="wire", in_features=2, out_features=O, hidden_features=64, hidden_layers=2,
                               first_omega_0=7.0, hidden_omega_0=7.0, scale=6.0).to(DEV)
        return FusedTrainer(model, (H, W), None, lr=0.0)

    tr = fresh()
    coords = tr.affine_coords(mats)
    tr.step_frames(coords, gt, scale, mask=mask)
    l1 = tr.step_frames(coords[1:2].contiguous(), gt[1:2].contiguous(), scale, mask=mask[1:2].contiguous())
    torch.cuda.synchronize()
    g1 = tr.flat_grad.cpu().numpy().copy()
    tr2 = fresh()
    l2 = tr2.step_frames(coords[1:2].contiguous(), gt[1:2].contiguous(), scale, mask=mask[1:2].contiguous())
    torch.cuda.synchronize()
    g2 = tr2.flat_grad.cpu().numpy()
    print(f"smaller batch: max |g1 - g2| {np.abs(g1 - g2).max():.3e} of max|g| {np.abs(g2).max():.3e}")
    assert float(l1.item()) == float(l2.item()) and np.array_equal(g1, g2)
    assert np.abs(g2).max() > 0
    # rec_lr receives the pooled frames of the step
    rec = torch.zeros_like(gt)
    tr2.step_frames(coords, gt, scale, rec_lr=rec)
    torch.cuda.synchronize()
    y = tr2.y[:3 * H * W * O].reshape(3, H, W, O).cpu().numpy()
    want = y.reshape(3, H // scale, scale, W // scale, scale, O).mean(axis=(2, 4)).reshape(3, -1, O)
    np.testing.assert_allclose(rec.cpu().numpy(), want, rtol=0, atol=2e-6)
    # target=None
    for call in (lambda: tr2.step(), lambda: tr2.step_hashed(0), lambda: tr2.psnr(rec)):
        with pytest.raises(ValueError, match="target"):
            call()
    with pytest.raises(ValueError, match="coords"):
        tr2.step_frames(coords[:, :-1], gt, scale)
    with pytest.raises(ValueError, match="gt_lr"):
        tr2.step_frames(coords, gt[:2], scale)
    with pytest.raises(ValueError, match="scale"):
        tr2.step_frames(coords, gt, 0)
