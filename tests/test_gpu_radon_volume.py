"""GPU checks of volume CT: wire_radon_vol_fwd / wire_radon_vol_bwd against the 2-D kernel (bits), the fp64
restatement of tests/radon_volume_ref.py and each other (the adjoint is the forward's transpose, tap for tap),
lin_inverse.radon_volume, and FusedTrainer.step_radon_volume -- one pass and in slabs, with and without the TV prior --
against the fp64 oracle and against autograd through the drop-in modules."""
import numpy as np
import pytest
import torch

from _util import params_np, relmax, within_ref
import radon_volume_ref as ref
import tv_reg_ref as tvref
from oracle import torch_ref, wire_oracle as wo

pytestmark = pytest.mark.gpu
DEV = torch.device("cuda:0")
A8 = len(ref.ANGLES)


def _lib():
    from wire_amd import _lib
    return _lib, _lib.lib()


def _stream():
    return torch.cuda.current_stream().cuda_stream


def _vol_fwd(vol, ang, out=None):
    """vol [H][W][C] device tensor -> [A][W][C]; ``out``: a preallocated result (a view tests the unaligned path)."""
    lib, L = _lib()
    H, W, Cn = vol.shape
    if out is None:
        out = torch.full((ang.numel(), W, Cn), float("nan"), device=DEV)
    lib.check(L.wire_radon_vol_fwd(_stream(), vol.data_ptr(), ang.data_ptr(), H, W, Cn, ang.numel(), out.data_ptr()),
              "wire_radon_vol_fwd")
    return out


def _vol_bwd(g, ang, H, fill):
    lib, L = _lib()
    A, W, Cn = g.shape
    out = torch.full((H, W, Cn), fill, device=DEV)
    lib.check(L.wire_radon_vol_bwd(_stream(), g.data_ptr(), ang.data_ptr(), H, W, Cn, A, out.data_ptr()),
              "wire_radon_vol_bwd")
    return out


def _slice_fwd(img, ang):
    lib, L = _lib()
    H, W = img.shape
    out = torch.full((ang.numel(), W), float("nan"), device=DEV)
    lib.check(L.wire_radon_fwd(_stream(), img.data_ptr(), ang.data_ptr(), H, W, ang.numel(), out.data_ptr()),
              "wire_radon_fwd")
    return out


# ---------------------------------------------------------------------------------------------------------------
# the two kernels
# ---------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("Cn", ref.CHANNELS)
@pytest.mark.parametrize("H,W", ref.SHAPES)
def test_forward_has_the_bits_of_the_slice_kernel(H, W, Cn):
    """Channel c of wire_radon_vol_fwd == wire_radon_fwd on slice c, bit for bit, and within 2 x the fp32 numpy error
    + 1e-6 of fp64.  C % 4 == 0 runs the 16-byte path; the same data through a result that is 4 bytes off a 16-byte
    boundary runs the scalar path and must give the same bits again."""
    vol, _, angles = ref.case(H, W, Cn)
    ang = torch.tensor(angles, device=DEV)
    v = torch.tensor(vol, device=DEV)
    out = _vol_fwd(v, ang)
    per = torch.stack([_slice_fwd(v[:, :, c].contiguous(), ang) for c in range(Cn)], dim=2)
    torch.cuda.synchronize()
    got = out.cpu().numpy()
    assert not np.isnan(got).any()
    assert got.tobytes() == per.cpu().numpy().tobytes()
    r64 = ref.radon_volume(vol, angles)
    within_ref(relmax(got, r64), relmax(ref.radon_volume(vol, angles, np.float32), r64),
               f"radon_vol_fwd {(H, W, Cn)}")
    if Cn % 4 == 0:
        buf = torch.full((A8 * W * Cn + 1,), float("nan"), device=DEV)
        assert buf.data_ptr() % 16 == 0
        off = _vol_fwd(v, ang, out=buf[1:].view(A8, W, Cn))
        torch.cuda.synchronize()
        assert off.cpu().numpy().tobytes() == got.tobytes()


@pytest.mark.parametrize("Cn", ref.CHANNELS)
@pytest.mark.parametrize("H,W", ref.SHAPES)
def test_adjoint_matches_fp64_and_repeats_its_bits(H, W, Cn):
    """Within 2 x the fp32 numpy error + 1e-6 of radon_adjoint per slice; called into a buffer of NaN and into one of
    7.0 it gives identical bits, so every element is written and nothing of the buffer is read."""
    _, g, angles = ref.case(H, W, Cn)
    ang = torch.tensor(angles, device=DEV)
    gd = torch.tensor(g, device=DEV)
    a = _vol_bwd(gd, ang, H, float("nan"))
    b = _vol_bwd(gd, ang, H, 7.0)
    torch.cuda.synchronize()
    a, b = a.cpu().numpy(), b.cpu().numpy()
    assert not np.isnan(a).any()
    assert a.tobytes() == b.tobytes()
    r64 = ref.radon_volume_adjoint(g, angles, H, W)
    within_ref(relmax(a, r64), relmax(ref.radon_volume_adjoint(g, angles, H, W, np.float32), r64),
               f"radon_vol_bwd {(H, W, Cn)}")


@pytest.mark.parametrize("H,W", [(5, 6), (6, 5), (1, 7), (7, 1)])
def test_adjoint_is_the_forward_transposed_tap_for_tap(H, W):
    """The whole matrix twice: from the forward, the H W one-hot images as the channels of one call; from the adjoint,
    the A W one-hot sinograms as the channels of one call.  Equal zero patterns, and entries within 8 * 2^-24 |entry|:
    with identical taps and weights an entry is a sum of at most about six positive terms in two orders, each reordering
    costing at most one rounding of 2^-24 of the sum."""
    ang = torch.tensor(ref.ANGLES, device=DEV)
    n, m = H * W, A8 * W
    fwd = _vol_fwd(torch.eye(n, device=DEV).reshape(H, W, n).contiguous(), ang)           # [A][W][(y, x)]
    bwd = _vol_bwd(torch.eye(m, device=DEV).reshape(A8, W, m).contiguous(), ang, H, float("nan"))   # [H][W][(a, j)]
    torch.cuda.synchronize()
    Mf = fwd.cpu().numpy().reshape(m, n).astype(np.float64)
    Mb = bwd.cpu().numpy().reshape(n, m).astype(np.float64).T
    assert not np.isnan(Mf).any() and not np.isnan(Mb).any()
    # (every pixel is a tap of the sample that angle 0 puts on it; a sample may fall outside a one-row image)
    assert (Mf >= 0).all() and (Mb >= 0).all() and (Mf > 0).sum() >= n
    gap = np.abs(Mf - Mb) / np.where(Mf > 0, Mf, 1.0)
    print(f"radon_volume transpose {(H, W)}: {int((Mf != 0).sum())} nonzero entries, "
          f"{int(((Mf != 0) != (Mb != 0)).sum())} pattern mismatches, worst gap {gap.max() / 2.0 ** -24:.2f} x 2^-24")
    assert np.array_equal(Mf != 0, Mb != 0)
    assert (np.abs(Mf - Mb) <= 8 * 2.0 ** -24 * np.abs(Mf)).all()


def test_indices_past_31_bits():
    """H W C = 2 x 32768 x 32772 elements, past 2^31: at angle 0 the forward is the sum of the two rows and the
    adjoint copies the sinogram into both, exactly (every weight is 0 or 1)."""
    H, W, Cn = 2, 32768, 32772
    assert H * W * Cn > 2 ** 31
    ang = torch.zeros(1, device=DEV)
    vol = torch.rand(H, W, Cn, device=DEV)
    out = _vol_fwd(vol, ang)
    assert torch.equal(out[0], vol[0] + vol[1])
    del vol
    back = _vol_bwd(out, ang, H, float("nan"))
    assert torch.equal(back[0], out[0]) and torch.equal(back[1], out[0])


def test_radon_volume_autograd_against_the_reference_layout():
    """lin_inverse.radon_volume == lin_inverse.radon(..., is_3d=True) in the reference's layout, permuted: the forward
    bit for bit, the gradient within 2 x the fp32 numpy error + 1e-6 of the fp64 adjoint."""
    from wire_amd.modules import lin_inverse
    H, W, T = 24, 30, 5
    vol, g, angles = ref.case(H, W, T)
    ang = torch.tensor(angles, device=DEV)
    v = torch.tensor(vol, device=DEV, requires_grad=True)
    out = lin_inverse.radon_volume(v, ang)
    assert tuple(out.shape) == (A8, W, T)
    with torch.no_grad():
        want = lin_inverse.radon(v.permute(2, 0, 1)[None], ang, is_3d=True).permute(1, 2, 0)
    assert out.detach().cpu().numpy().tobytes() == want.contiguous().cpu().numpy().tobytes()
    out.backward(torch.tensor(g, device=DEV))
    assert lin_inverse.radon_volume(v, ang.cpu()).shape == out.shape                 # angles from the host are moved
    r64 = ref.radon_volume_adjoint(g, angles, H, W)
    within_ref(relmax(v.grad.cpu().numpy(), r64), relmax(ref.radon_volume_adjoint(g, angles, H, W, np.float32), r64),
               "radon_volume autograd")


# ---------------------------------------------------------------------------------------------------------------
# the step
# ---------------------------------------------------------------------------------------------------------------
ADAM = "adam_step_flat"
PACK, COORDS, FWD, BWD = "pack_params", "coords_from_index", "mlp_fwd", "mlp_bwd"
OPERATOR = ["radon_vol_fwd", "mse_grad", "radon_vol_bwd"]


class _Recorder:
    """tests/test_gpu_step_launches.py's proxy: every library call of the trainer, by name."""

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


def _pow2_near(v):
    return 2.0 ** int(np.round(np.log2(v)))


class _VolCase:
    """Grid (12, 10, 5), 7 angles, wire 2 x 64 with 3 inputs (test_ct_radon.py's omega_0 = 3, s_0 = 12) on an lr = 0
    trainer; the data are the fp32 sinograms of a smooth synthetic volume.  The fp64 side is computed once."""
    H, W, T, A, hp = 12, 10, 5, 7, (3.0, 3.0, 12.0)

    def __init__(self):
        from wire_amd.modules import models
        from wire_amd.trainer import FusedTrainer
        H, W, T = self.H, self.W, self.T
        self.NP, self.n = H * W, H * W * T
        self.thetas = np.linspace(0, 180, self.A, dtype=np.float32)
        vol = torch.tensor(ref.smooth_volume(H, W, T))
        self.sino = torch.stack([torch_ref.radon(vol[:, :, k], torch.tensor(self.thetas)) for k in range(T)],
                                dim=2).numpy()
        torch.manual_seed(0)
        self.model = models.get_INR(nonlin="wire", in_features=3, out_features=1, hidden_features=64, hidden_layers=2,
                                    first_omega_0=self.hp[0], hidden_omega_0=self.hp[1], scale=self.hp[2]).to(DEV)
        self.tr = FusedTrainer(self.model, (H, W, T), None, lr=0.0)
        self.tr.L = _Recorder(self.tr.L)
        self.sino_dev, self.th_dev = torch.tensor(self.sino, device=DEV), torch.tensor(self.thetas, device=DEV)
        self.step()                                              # builds the coordinates the oracle runs on
        x = self.tr.coords[:self.n * 3].reshape(self.n, 3).cpu().numpy()
        self.p64 = wo.cast_params(params_np(self.model), True)
        self.y64, self.cache = wo.wire_forward(self.p64, x.astype(np.float64), 2, *self.hp, keep=True)
        est = torch.tensor(self.y64.reshape(H, W, T), requires_grad=True)
        s = torch.stack([torch_ref.radon(est[:, :, k], torch.tensor(self.thetas)) for k in range(T)], dim=2)
        loss = ((torch.tensor(self.sino).double() - s) ** 2).mean()
        loss.backward()
        self.d64, self.gy64 = float(loss.item()), est.grad.numpy().reshape(self.n, 1)

    def step(self, **kw):
        """(loss, flat gradient, the step's volume, library calls)."""
        self.tr.L.calls.clear()
        loss = self.tr.step_radon_volume(self.sino_dev, self.th_dev, **kw)
        torch.cuda.synchronize()
        slab = kw.get("slab")
        y = self.tr.y if slab is None or slab >= self.NP else self.tr.y_vol
        return (loss.cpu().numpy().copy(), self.tr.flat_grad.cpu().numpy().copy(),
                y[:self.n].cpu().numpy().reshape(self.n, 1).copy(), list(self.tr.L.calls))

    def backward(self, gy):
        return wo.wire_backward(self.p64, self.cache, np.asarray(gy, np.float64), 2, *self.hp)

    def check(self, label, loss, flat, l64, g64):
        """Loss 2e-5 relative, every gradient 5e-5 max|g| + 1e-10 (the bounds of tests/test_gpu_tv_reg.py)."""
        names = [k for k in self.model.state_dict().keys() if "omega_0" not in k and "scale_0" not in k]
        assert len(names) == len(self.tr.offsets)
        loss = float(loss[0])
        rows = []
        for name, off in zip(names, self.tr.offsets):
            g = wo.as_real_pairs(g64[name]).astype(np.float64).ravel()
            rows.append((name, np.abs(flat[off:off + g.size] - g).max(), np.abs(g).max()))
            print(f"radon_volume parity {label}: {name:22s} err / max|g| {rows[-1][1] / rows[-1][2]:.3e}")
        print(f"radon_volume parity {label}: {'loss (relative)':22s} {abs(loss - l64) / l64:.3e}")
        assert abs(loss - l64) <= 2e-5 * l64
        for name, err, gmax in rows:
            assert err <= 5e-5 * gmax + 1e-10, name


@pytest.fixture(scope="module")
def case():
    return _VolCase()


def _slabbed(npix, slab, prior=False):
    k = (npix + slab - 1) // slab
    return [PACK] + k * [COORDS, FWD] + OPERATOR + (["tv_add_grad"] if prior else []) + k * [COORDS, FWD, BWD] + [ADAM]


ONE_PASS = [PACK, COORDS, FWD] + OPERATOR + [BWD, ADAM]


@pytest.mark.parametrize("slab", [None, 37, 119, 120])
def test_step_matches_the_fp64_oracle(case, slab):
    """Loss and every parameter gradient against the fp64 oracle (dL/dy by fp64 autograd of torch_ref.radon per slice),
    one pass and in slabs of 37 (not a divisor of 120), 119 and 120 pixels; the launches of each path; the same call
    again gives the same bits (lr = 0), which the 2-D CT step's atomics cannot; slab = 120 is the one-pass path: its
    launches and its bits."""
    loss, flat, y, calls = case.step(slab=slab)
    label = f"slab={slab}"
    case.check(label, loss, flat, case.d64, case.backward(case.gy64))
    assert relmax(y, case.y64) <= 2e-5
    assert calls == (ONE_PASS if slab in (None, 120) else _slabbed(case.NP, slab))
    loss2, flat2, y2, _ = case.step(slab=slab)
    assert loss.tobytes() == loss2.tobytes() and flat.tobytes() == flat2.tobytes() and y.tobytes() == y2.tobytes()
    if slab == 120:
        loss1, flat1, y1, _ = case.step()
        assert loss.tobytes() == loss1.tobytes() and flat.tobytes() == flat1.tobytes() and y.tobytes() == y1.tobytes()
    if slab is not None and slab < case.NP:
        # the slabs sum to the one-pass gradient up to the order of the sums
        _, flat1, _, _ = case.step()
        print(f"radon_volume parity {label}: slabbed vs one-pass gradient {relmax(flat, flat1):.3e}")


@pytest.mark.parametrize("slab", [None, 37])
def test_step_with_the_prior_matches_the_oracle(case, slab):
    """lambda_tv and lambda_tv_t on (the power of two nearest the largest data term of dL/dy, and half of it) against
    tv_reg_ref.tv_add_grad on (H, W, T), the sign pattern taken from the step's own volume: the same bounds, with slabs
    and without; tv_parts adds up; each weight alone launches the prior as well, both zero do not."""
    H, W, T = case.H, case.W, case.T
    ls = _pow2_near(np.abs(case.gy64).max())
    lt = ls / 2
    gm = float(np.abs(case.gy64).max())
    assert 0.1 <= gm / ls <= 10 and 0.1 <= gm / lt <= 10
    plain, _, _, _ = case.step(slab=slab)
    loss, flat, y, calls = case.step(slab=slab, lambda_tv=ls, lambda_tv_t=lt)
    a = np.concatenate([s.ravel() for s in tvref.pair_signs(y, H, W, T, 1)])
    b = np.concatenate([s.ravel() for s in tvref.pair_signs(case.y64, H, W, T, 1)])
    assert int((a != b).sum()) <= 1e-3 * a.size
    l64, tvs64, tvt64, gy = tvref.tv_add_grad(case.y64, case.gy64, H, W, T, 1, ls, lt, data=case.d64, pattern_from=y)
    case.check(f"slab={slab} lambda_tv={ls:g} lambda_tv_t={lt:g}", loss, flat, float(l64),
               case.backward(gy.reshape(case.n, 1)))
    p = case.tr.tv_parts.cpu().numpy()
    assert p[0] == loss[0] and p[0].tobytes() == tvref.total_loss(p[1], ls, p[2], lt, p[3]).tobytes()
    assert p[1].tobytes() == plain[0].tobytes()                               # the data term is the plain step's loss
    assert abs(p[2] - tvs64) <= 2e-5 * tvs64 and abs(p[3] - tvt64) <= 2e-5 * tvt64
    assert loss[0] > plain[0]
    want = _with_prior(ONE_PASS) if slab is None else _slabbed(case.NP, slab, prior=True)
    assert calls == want
    for kw in (dict(lambda_tv=ls), dict(lambda_tv_t=lt)):
        l1, _, _, g1 = tvref.tv_add_grad(case.y64, case.gy64, H, W, T, 1, kw.get("lambda_tv", 0.0),
                                         kw.get("lambda_tv_t", 0.0), data=case.d64, pattern_from=y)
        one, flat1, _, calls1 = case.step(slab=slab, **kw)
        assert calls1 == want
        case.check(f"slab={slab} {sorted(kw)[0]} alone", one, flat1, float(l1), case.backward(g1.reshape(case.n, 1)))
    zero, flatz, _, callz = case.step(slab=slab, lambda_tv=0.0, lambda_tv_t=0.0)
    assert "tv_add_grad" not in callz and zero.tobytes() == plain.tobytes()


def _with_prior(seq):
    i = seq.index("radon_vol_bwd") + 1
    return seq[:i] + ["tv_add_grad"] + seq[i:]


def _trajectory(kind, hp, slab, niters=6, lr=5e-3):
    """The loss of ``niters`` Adam steps: autograd through the drop-in modules and lin_inverse.radon_volume with
    torch.optim.Adam, and step_radon_volume, from the same initial weights on the same coordinates."""
    from torch.optim.lr_scheduler import LambdaLR
    from wire_amd.modules import lin_inverse, models
    from wire_amd.trainer import FusedTrainer
    H, W, T, A = 12, 10, 5, 7
    n = H * W * T
    thetas = torch.tensor(np.linspace(0, 180, A, dtype=np.float32), device=DEV)
    with torch.no_grad():
        sino = lin_inverse.radon_volume(torch.tensor(ref.smooth_volume(H, W, T), device=DEV), thetas)

    def build():
        torch.manual_seed(0)
        return models.get_INR(nonlin=kind, in_features=3, out_features=1, hidden_features=64, hidden_layers=2,
                              first_omega_0=hp[0], hidden_omega_0=hp[1], scale=hp[2]).to(DEV)
    probe = FusedTrainer(build(), (H, W, T), None, lr=0.0)
    probe.step_radon_volume(sino, thetas)
    coords = probe.coords[:n * 3].reshape(1, n, 3).clone()                    # the grid's rows, (i W + j) T + k
    model = build()
    optimizer = torch.optim.Adam(lr=lr, params=model.parameters())
    scheduler = LambdaLR(optimizer, lambda x: 0.1 ** min(x / niters, 1))
    losses = []
    for _ in range(niters):
        est = model(coords).reshape(H, W, T)
        loss = ((sino - lin_inverse.radon_volume(est, thetas)) ** 2).mean()
        optimizer.zero_grad()
        loss.backward()
        optimizer.step()
        scheduler.step()
        losses.append(loss.item())
    tr = FusedTrainer(build(), (H, W, T), None, lr=lr, niters=niters)
    fused = []
    for _ in range(niters):
        fused.append(tr.step_radon_volume(sino, thetas, slab=slab))
        tr.scheduler_step()
    torch.cuda.synchronize()
    fused = [float(l.item()) for l in fused]
    print(f"radon_volume loop {kind} slab={slab}: autograd {losses}\n fused {fused}")
    np.testing.assert_allclose(fused, losses, rtol=2e-3)


@pytest.mark.parametrize("slab", [None, 37])
def test_loop_follows_autograd(slab):
    """Six Adam steps at lr = 5e-3 at rtol = 2e-3, the bound of test_ct_loop_with_prior_follows_autograd."""
    _trajectory("wire", (3.0, 3.0, 12.0), slab)


def test_loop_follows_autograd_on_a_real_kind():
    """The same loop once on siren, in slabs."""
    _trajectory("siren", (30.0, 30.0, 10.0), 37)
