"""GPU checks of FusedTrainer.step_resized: dL/dy and the loss of one step against the fp64 restatement of
tests/resize_ref.py evaluated on that step's own reconstruction, the TV prior's switch and its parts, a 200-step run
against the fp64 oracle's run from the same initial state, and the refusals that come before the first device access."""
import numpy as np
import pytest
import torch

from _util import relmax, within_ref
import resize_ref as ref
import tv_reg_ref as tvref

pytestmark = pytest.mark.gpu
DEV = torch.device("cuda:0")


def _net(kind, O, hf=64):
    from wire_amd.modules import models
    torch.manual_seed(0)
    hp = (7.0, 7.0, 6.0) if kind == "wire" else (30.0, 30.0, 10.0)
    return models.get_INR(nonlin=kind, in_features=2, out_features=O, hidden_features=hf, hidden_layers=2,
                          first_omega_0=hp[0], hidden_omega_0=hp[1], scale=hp[2]).to(DEV)


class _Recorder:
    """tests/test_gpu_step_launches.py's proxy: the names of the library calls of a step, in order."""

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


def _trainer(kind, H, W, O, lr=0.0):
    from wire_amd.trainer import FusedTrainer
    tr = FusedTrainer(_net(kind, O), (H, W), None, lr=lr)
    tr.L = _Recorder(tr.L)
    return tr


CASES = [("siren", 16, 16, 1, 5, 7, m) for m in ("nearest", "linear", "cubic", "area")] + \
        [("wire", 12, 10, 3, 5, 4, m) for m in ("area", "cubic", "linear", 0)]


@pytest.mark.parametrize("kind,H,W,O,Hl,Wl,mode", CASES)
def test_one_step_gradient_and_loss(kind, H, W, O, Hl, Wl, mode):
    """One step at a non-integer factor.  From the step's own self.y the restatement gives the fp64 loss, dL/dy and the
    resized image; self.gy, the returned loss and rec_lr meet err_build <= 2 err_ref + 1e-6, err_ref being the
    restatement's fp32 evaluation of the same.  The step's calls are the skeleton's with wire_resize_mse_grad as the loss."""
    tr = _trainer(kind, H, W, O)
    r = ref.Resize(mode, H, W, Hl, Wl)
    gt = np.random.default_rng(H + Hl).uniform(0, 1, (Hl * Wl, O)).astype(np.float32)
    gtd = torch.tensor(gt, device=DEV)
    rec = torch.full((Hl * Wl, O), float("nan"), device=DEV)
    loss = tr.step_resized(gtd, (Hl, Wl), mode, rec_lr=rec)
    torch.cuda.synchronize()
    assert tr.L.calls == ["resize_tables", "pack_params", "coords_from_index", "mlp_fwd", "resize_mse_grad", "mlp_bwd",
                          "adam_step_flat"]
    y = tr.y[:H * W * O].cpu().numpy().reshape(H, W, O)
    gy = tr.gy[:H * W * O].cpu().numpy().reshape(H, W, O)
    assert np.abs(y).max() > 1e-3
    g3 = gt.reshape(Hl, Wl, O)
    l64, g64, rec64 = r.mse_grad64(y, g3)
    rec32 = r.fwd32(y)
    d32 = rec32 - g3
    l32 = float(np.sum(d32 * d32, dtype=np.float32) * np.float32(1.0 / d32.size))
    g32 = r.bwd32(np.float32(2.0 / d32.size) * d32)
    label = f"step_resized {kind} {H}x{W}->{Hl}x{Wl}x{O} {mode}"
    lossv = float(loss.item())
    print(f"{label}: loss {lossv:.6e} rel err {abs(lossv - l64) / l64:.2e} (ref {abs(l32 - l64) / l64:.2e})  "
          f"g_y err {relmax(gy, g64):.2e} (ref {relmax(g32, g64):.2e})")
    within_ref(abs(lossv - l64) / l64, abs(l32 - l64) / l64, label + " loss")
    within_ref(relmax(gy, g64), relmax(g32, g64), label + " g_y")
    within_ref(relmax(rec.cpu().numpy().reshape(Hl, Wl, O), rec64), relmax(rec32, rec64), label + " rec_lr")
    tr.L.calls.clear()
    again = tr.step_resized(gtd, (Hl, Wl), mode)                             # lr = 0: the same step, the tables reused
    torch.cuda.synchronize()
    assert tr.L.calls[0] == "pack_params" and again.cpu().numpy().tobytes() == loss.cpu().numpy().tobytes()
    assert tr.gy[:H * W * O].cpu().numpy().tobytes() == gy.tobytes()


@pytest.mark.parametrize("kind,H,W,O,Hl,Wl,mode", [CASES[2], CASES[4]])
def test_tv_prior_switch_and_parts(kind, H, W, O, Hl, Wl, mode):
    """lambda_tv = 0.0 launches no TV kernel and gives the bits of the plain step; lambda_tv != 0 launches it between the
    loss and the backward, tv_parts = [loss, mse, tv, 0] with mse the plain step's loss bit for bit, tv the total variation
    of self.y (2e-5 relative to fp64) and loss = fl(fl(mse + fl(lambda tv)) + fl(0 * 0)), the header's expression."""
    tr = _trainer(kind, H, W, O)
    gtd = torch.tensor(np.random.default_rng(1).uniform(0, 1, (Hl * Wl, O)).astype(np.float32), device=DEV)
    plain = tr.step_resized(gtd, (Hl, Wl), mode)
    torch.cuda.synchronize()
    gy0, flat0 = tr.gy[:H * W * O].clone(), tr.flat_grad.clone()
    tr.L.calls.clear()
    zero = tr.step_resized(gtd, (Hl, Wl), mode, lambda_tv=0.0)
    torch.cuda.synchronize()
    assert "tv_add_grad" not in tr.L.calls
    assert torch.equal(zero, plain) and torch.equal(tr.gy[:H * W * O], gy0) and torch.equal(tr.flat_grad, flat0)
    lam = float(np.float32(2.0 ** -12))
    tr.L.calls.clear()
    loss = tr.step_resized(gtd, (Hl, Wl), mode, lambda_tv=lam)
    torch.cuda.synchronize()
    assert tr.L.calls == ["pack_params", "coords_from_index", "mlp_fwd", "resize_mse_grad", "tv_add_grad", "mlp_bwd",
                          "adam_step_flat"]
    p = tr.tv_parts.cpu().numpy()
    y = tr.y[:H * W * O].cpu().numpy().reshape(H * W, O)
    tvs64, _ = tvref.tv_sums(y, H, W, 1, O)
    print(f"step_resized tv {kind} {mode}: parts {p}, tv64 {tvs64:.6e}")
    assert p[0] == np.float32(loss.item()) and p[1].tobytes() == plain.cpu().numpy().tobytes() and p[3] == 0.0
    assert abs(p[2] - tvs64) <= 2e-5 * tvs64 and tvs64 > 0
    assert p[0].tobytes() == tvref.total_loss(p[1], lam, p[2], 0.0, p[3]).tobytes()
    assert not torch.equal(tr.gy[:H * W * O], gy0)


def test_short_run_against_the_fp64_oracle():
    """200 Adam steps (lr 2e-4, constant) recover a smooth 16 x 16 image -- two low-frequency sinusoids -- from its 2 x
    bicubic down-sampling, from the same initial state_dict as the fp64 oracle (oracle/torch_ref's siren forward under the
    dense R of tests/resize_ref.py, torch.optim.Adam), which runs here on the CPU as well.  The GPU's final loss is at
    most 2 x the oracle's (200 Adam steps in fp32 and fp64 do not follow the same path) and below its own first loss;
    the oracle must have trained: its final loss below a tenth of its first.
    #   $ python tests/resize_ref.py
    #   fp64 oracle, {... 'lr': 0.0002, 'steps': 200}: first loss 3.736330e-01, loss of step 200 6.008684e-05
    # (the learning rate is 2e-4, not the trainer's default 5e-3: at 5e-4 and above the oracle's loss falls to 1e-11 and
    # then moves up and down from step to step, where a factor between two runs means nothing; at 2e-4 it falls
    # monotonically over the last 100 steps and an fp32 run of the same loop on the CPU ends at 1.000 x the fp64 loss)"""
    from wire_amd.trainer import FusedTrainer
    S = ref.SR
    cpu = ref.sr_model()
    state = {k: v.detach().clone().numpy() for k, v in cpu.state_dict().items()}
    _, gt, _ = ref.sr_image()
    tr = FusedTrainer(cpu.to(DEV), (S["H"], S["W"]), None, lr=S["lr"])
    gtd = torch.tensor(gt, device=DEV)
    losses = [tr.step_resized(gtd, (S["Hl"], S["Wl"]), S["mode"]) for _ in range(S["steps"])]
    coords = tr.coords[:S["H"] * S["W"] * 2].reshape(-1, 2).cpu().numpy()
    first, last = float(losses[0].item()), float(losses[-1].item())
    want = ref.sr_oracle_losses(state, coords)
    print(f"step_resized run: GPU first {first:.6e} last {last:.6e}; fp64 oracle first {want[0]:.6e} last {want[-1]:.6e}; "
          f"ratio {last / want[-1]:.3f}")
    assert want[-1] < 0.1 * want[0], "the oracle did not train"
    assert abs(want[-1] - 6.008684e-05) <= 1e-3 * 6.008684e-05               # the number in the docstring is this run's
    assert abs(first - want[0]) <= 1e-4 * want[0]
    assert last <= 2.0 * want[-1] and last < first


def test_refusals_come_before_the_device(monkeypatch):
    from wire_amd.modules import models
    from wire_amd.trainer import FusedTrainer
    tr = _trainer("siren", 16, 16, 1)
    x = torch.zeros(35, 1, device=DEV)

    def refused(exc, match, *a, **kw):
        tr.L.calls.clear()
        with pytest.raises(exc, match=match):
            tr.step_resized(*a, **kw)
        assert tr.L.calls == []

    refused(ValueError, "gt_lr must be", torch.zeros(34, 1, device=DEV), (5, 7), "linear")
    refused(ValueError, "gt_lr must be", x.cpu(), (5, 7), "linear")
    refused(ValueError, "does not up-scale", torch.zeros(17 * 7, 1, device=DEV), (17, 7), "area")
    refused(ValueError, "lambda_tv must be finite", x, (5, 7), "linear", lambda_tv=float("nan"))
    refused(ValueError, "interpolation must be", x, (5, 7), "lanczos")
    refused(ValueError, "rec_lr must be", x, (5, 7), "linear", rec_lr=torch.zeros(3, device=DEV))
    monkeypatch.setattr(tr, "world", 2)
    refused(NotImplementedError, "step_resized is single-process", x, (5, 7), "linear")
    torch.manual_seed(0)
    m3 = models.get_INR(nonlin="siren", in_features=3, out_features=1, hidden_features=64, hidden_layers=2,
                        first_omega_0=30.0, hidden_omega_0=30.0, scale=10.0).to(DEV)
    tr = FusedTrainer(m3, (4, 5, 6), None)
    tr.L = _Recorder(tr.L)
    refused(ValueError, "2-D grid", x, (2, 2), "linear")
