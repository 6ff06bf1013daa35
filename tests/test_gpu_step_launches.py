"""The library calls of every FusedTrainer step, in order.  A recording proxy stands in for ``tr.L``: each entry point
appends its name (without the ``wire_`` prefix) and calls through; the host size queries (``*_bytes``, ``*_floats``)
are not recorded.  The steps share one frame ("The step skeleton"): these tables pin what each step puts
into it -- a prior kernel only with a nonzero weight, one pack for all the slabs of step_coded, step_ssim's loss kernel
also at weight 0, two Adam launches per stage with the per-stage rates of bspline_mscale_hier."""
import pytest
import torch

pytestmark = pytest.mark.gpu
DEV = torch.device("cuda:0")

ADAM = "adam_step_flat"
PACK, COORDS, FWD, BWD = "pack_params", "coords_from_index", "mlp_fwd", "mlp_bwd"


class _Recorder:
    def __init__(self, lib):
        self._lib, self.calls = lib, []

    def __getattr__(self, name):
        fn = getattr(self._lib, name)
        if name.endswith(("_bytes", "_floats")):
            return fn

        def call(*a, **kw):
            self.calls.append(name[len("wire_"):])
            return fn(*a, **kw)
        return call


def _trainer(D, O, grid, target=True):
    """The smallest wire net of tests/test_gpu_tv_reg.py on ``grid``, its library behind a recorder."""
    from wire_amd.modules import models
    from wire_amd.trainer import FusedTrainer
    torch.manual_seed(0)
    m = models.get_INR(nonlin="wire", in_features=D, out_features=O, hidden_features=128, hidden_layers=2,
                       first_omega_0=7.0, hidden_omega_0=7.0, scale=6.0).to(DEV)
    n = 1
    for v in grid:
        n *= v
    tgt = torch.rand(n, O, generator=torch.Generator().manual_seed(1)) if target else None
    tr = FusedTrainer(m, grid, tgt, lr=1e-3)
    tr.L = _Recorder(tr.L)
    return tr


def _calls(tr, fn):
    tr.L.calls.clear()
    fn()
    torch.cuda.synchronize()
    return list(tr.L.calls)


def _rand(*shape, seed=2):
    return torch.rand(*shape, generator=torch.Generator().manual_seed(seed)).to(DEV)


def _with(seq, extra, after):
    i = seq.index(after) + 1
    return seq[:i] + [extra] + seq[i:]


def test_image_steps():
    H, W, O = 8, 6, 3
    tr = _trainer(2, O, (H, W))
    gt = _rand((H // 2) * (W // 2), O)
    plain = [PACK, COORDS, FWD, "avgpool_mse_grad", BWD, ADAM]
    assert _calls(tr, lambda: tr.step_downsampled(gt, 2)) == plain
    assert _calls(tr, lambda: tr.step_downsampled(gt, 2, lambda_tv=.1)) == \
        _with(plain, "tv_add_grad", "avgpool_mse_grad")
    assert _calls(tr, lambda: tr.step_downsampled(gt, 2, lambda_tv=0.)) == plain
    tv = [PACK, COORDS, FWD, "tv_mse_grad", BWD, ADAM]
    assert _calls(tr, lambda: tr.step_tv(.1)) == tv
    idx = torch.randperm(H * W, generator=torch.Generator().manual_seed(3))[:20].to(DEV)
    assert _calls(tr, lambda: tr.step_tv(.1, indices=idx)) == tv
    assert _calls(tr, lambda: tr.step(first=0, count=16)) == [PACK, COORDS, "train_fwd_bwd", ADAM]


def test_step_ssim():
    tr = _trainer(2, 3, (12, 13))
    seq = [PACK, COORDS, FWD, "ssim_mse_grad", BWD, ADAM]
    assert _calls(tr, lambda: tr.step_ssim(.1)) == seq
    assert _calls(tr, lambda: tr.step_ssim(0.)) == seq


def test_frame_steps():
    H, W, O, B = 8, 6, 3, 2
    tr = _trainer(2, O, (H, W), target=False)
    xy = tr.affine_coords(torch.tensor([[[1., 0., 0.], [0., 1., 0.]], [[1., 0., .05], [0., 1., -.05]]]))
    gt = _rand(B, (H // 2) * (W // 2), O)
    assert _calls(tr, lambda: tr.step_frames(xy, gt, 2)) == [PACK, FWD, "avgpool_mse_grad_frames", BWD, ADAM]
    reg = tr.registration(B)
    assert _calls(tr, lambda: tr.step_frames_registered(reg, xy, gt, 2)) == \
        [PACK, "warp_coords_fwd", FWD, "avgpool_mse_grad_frames", "mlp_bwd_coords", "warp_coords_bwd", ADAM, ADAM]


def test_step_radon():
    H, W, A = 8, 6, 5
    tr = _trainer(2, 1, (H, W), target=False)
    sino, th = _rand(A * W), torch.linspace(0, 180, A)
    plain = [PACK, COORDS, FWD, "radon_fwd", "mse_grad", "radon_bwd", BWD, ADAM]
    assert _calls(tr, lambda: tr.step_radon(sino, th)) == plain
    assert _calls(tr, lambda: tr.step_radon(sino, th, lambda_tv=.1)) == _with(plain, "tv_add_grad", "radon_bwd")


def test_step_coded():
    H, W, T, nframes = 4, 5, 6, 2
    tr = _trainer(3, 1, (H, W, T), target=False)
    coded = _rand((T // nframes + 1) * H * W)
    masks = (_rand(H * W * T, seed=4) < .5).float()
    one = [PACK, COORDS, FWD, "coded_mse_grad", BWD, ADAM]
    assert _calls(tr, lambda: tr.step_coded(coded, masks, nframes)) == one
    assert _calls(tr, lambda: tr.step_coded(coded, masks, nframes, lambda_tv_t=.1)) == \
        _with(one, "tv_add_grad", "coded_mse_grad")
    # 20 pixels in slabs of 7: one pack, three passes, one Adam
    assert _calls(tr, lambda: tr.step_coded(coded, masks, nframes, slab=7)) == \
        [PACK] + 3 * [COORDS, FWD, "coded_mse_grad", BWD] + [ADAM]


def test_hier_stage_rates():
    """One rate per stage: Adam steps stage s and head s on their own, 2 S launches."""
    from wire_amd.modules import models
    from wire_amd.trainer import FusedTrainer
    H, W, O, st = 8, 6, 3, [1 / 9, 4.0]
    torch.manual_seed(0)
    model = models.get_INR(nonlin="bspline_mscale_hier", in_features=2, out_features=O, hidden_features=64,
                           scaled_hidden_features=0, hidden_layers=2, first_omega_0=-0.2, hidden_omega_0=-0.2,
                           scale=0.0, scale_tensor=st).to(DEV)
    tr = FusedTrainer(model, (H, W), _rand(H * W, O), lr=[6e-3, 2e-2], niters=100)
    tr.L = _Recorder(tr.L)
    assert _calls(tr, lambda: tr.step_tv(0.)) == [PACK, COORDS, FWD, "tv_mse_grad", BWD] + 2 * len(st) * [ADAM]
