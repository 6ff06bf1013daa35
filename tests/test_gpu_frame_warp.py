"""GPU checks of the learnable registration: wire_warp_coords_fwd / wire_warp_coords_bwd against the numpy restatement of
tests/frame_warp_ref.py (bit for bit where the header promises bits), functional.warp_coords, and
FusedTrainer.step_frames_registered -- loss, every parameter gradient, dL/dcoords and dL/dtheta against the eager oracle
of oracle/torch_ref.py in both GEMM families, the optimiser wiring, a descent against an fp64 twin, and independence of
what the workspaces held."""
import ctypes as C
import functools

import numpy as np
import pytest
import torch
import torch.nn.functional as F

from _util import relmax, within_ref
import frame_warp_ref as ref
import multi_sr_ref
from oracle import torch_ref

pytestmark = pytest.mark.gpu
DEV = torch.device("cuda:0")

# a frame smaller than a workgroup; 26 x 21 rows (no multiple of 256); several 2048-row chunks per frame, the last ragged
KERNEL_SHAPES = [(1, 63), (3, 546), (2, 90000)]


def _stream():
    return torch.cuda.current_stream().cuda_stream


def _kernel_inputs(B, n_per):
    """theta: the identity in frame 0, entries of size 1 elsewhere; coords in [-1.2, 1.2]; g_out ~ 1e-3 N(0, 1) with the
    last frame's all zero (B > 1: a single frame keeps its gradient)."""
    rng = np.random.default_rng(B * 100003 + n_per)
    coords = rng.uniform(-1.2, 1.2, (B, n_per, 2)).astype(np.float32)
    theta = rng.uniform(-1, 1, (B, 2, 3)).astype(np.float32)
    theta[0] = [[1, 0, 0], [0, 1, 0]]
    g = (1e-3 * rng.standard_normal((B, n_per, 2))).astype(np.float32)
    if B > 1:
        g[-1] = 0.0
    return coords, theta, g


def _fwd(coords, theta, inplace=False):
    from wire_amd import _lib
    L = _lib.lib()
    B, n_per = coords.shape[:2]
    c, t = torch.tensor(coords, device=DEV), torch.tensor(theta, device=DEV)
    out = c if inplace else torch.full_like(c, 7.0)
    _lib.check(L.wire_warp_coords_fwd(_stream(), c.data_ptr(), t.data_ptr(), B, n_per, out.data_ptr()), "warp_fwd")
    torch.cuda.synchronize()
    return out.cpu().numpy()


def _bwd(coords, theta, g, pin, want_g_in=True, ws_byte=0):
    from wire_amd import _lib
    L = _lib.lib()
    B, n_per = coords.shape[:2]
    c, t, gt = (torch.tensor(a, device=DEV) for a in (coords, theta, g))
    g_theta = torch.full((B, 2, 3), 7.0, device=DEV)
    g_in = torch.full_like(c, 7.0) if want_g_in else None
    nb = _lib.check(L.wire_warp_coords_bwd_ws_bytes(B, n_per), "ws_bytes")
    ws = torch.full((nb,), ws_byte, dtype=torch.uint8, device=DEV)
    _lib.check(L.wire_warp_coords_bwd(_stream(), c.data_ptr(), t.data_ptr(), gt.data_ptr(), B, n_per, pin,
                                      g_theta.data_ptr(), g_in.data_ptr() if want_g_in else None, ws.data_ptr(), nb),
               "warp_bwd")
    torch.cuda.synchronize()
    return g_theta.cpu().numpy(), g_in.cpu().numpy() if want_g_in else None


@pytest.mark.parametrize("B,n_per", KERNEL_SHAPES)
def test_warp_forward_bits(B, n_per):
    """The forward equals the restatement bit for bit; identity theta returns the input bits; in place gives the same
    bits."""
    coords, theta, _ = _kernel_inputs(B, n_per)
    got = _fwd(coords, theta)
    assert got.tobytes() == ref.warp(coords, theta).tobytes()
    assert got[0].tobytes() == coords[0].tobytes()
    eye = np.broadcast_to(np.array([[1, 0, 0], [0, 1, 0]], np.float32), (B, 2, 3)).copy()
    assert _fwd(coords, eye).tobytes() == coords.tobytes()
    assert _fwd(coords, theta, inplace=True).tobytes() == got.tobytes()


@pytest.mark.parametrize("B,n_per", KERNEL_SHAPES)
def test_warp_backward_against_restatement(B, n_per):
    """|g_theta - S| <= 2^-24 |S| + n_per 2^-52 sum|terms| per entry (one fp32 rounding plus the fp64 accumulation bound);
    the all-zero frame gives exact zeros; pin_first = 1 writes +0.0 into frame 0 and leaves the other frames' bits;
    g_in equals the restatement bit for bit; g_in = NULL, a second call and a ws of 0xFF bytes give the same bits."""
    coords, theta, g = _kernel_inputs(B, n_per)
    S, A, g_in64 = ref.warp_bwd(coords, theta, g, 0)
    g_theta, g_in = _bwd(coords, theta, g, 0)
    err, bound = np.abs(g_theta.astype(np.float64) - S), ref.g_theta_bound(S, A, n_per)
    print(f"warp bwd {(B, n_per)}: worst |g_theta - S| / bound {(err / np.maximum(bound, 1e-300)).max():.3f}, "
          f"max|S| {np.abs(S).max():.3e}")
    assert (err <= bound).all()
    if B > 1:
        assert g_theta[-1].tobytes() == np.zeros((2, 3), np.float32).tobytes()
    assert np.abs(g_theta[:max(B - 1, 1)]).min() > 0                    # frame 0 carries a gradient for pin_first to zero
    assert g_in.tobytes() == g_in64.tobytes()
    pinned, g_in_p = _bwd(coords, theta, g, 1)
    assert pinned[0].tobytes() == np.zeros((2, 3), np.float32).tobytes()
    assert pinned[1:].tobytes() == g_theta[1:].tobytes() and g_in_p.tobytes() == g_in.tobytes()
    assert _bwd(coords, theta, g, 0, want_g_in=False)[0].tobytes() == g_theta.tobytes()
    again = _bwd(coords, theta, g, 0)
    assert again[0].tobytes() == g_theta.tobytes() and again[1].tobytes() == g_in.tobytes()
    assert _bwd(coords, theta, g, 0, ws_byte=0xFF)[0].tobytes() == g_theta.tobytes()


def test_functional_warp_coords_backward_is_the_kernels():
    from wire_amd import functional
    B, n_per = 3, 546
    coords, theta, g = _kernel_inputs(B, n_per)
    g_theta, g_in = _bwd(coords, theta, g, 0)
    c = torch.tensor(coords, device=DEV, requires_grad=True)
    t = torch.tensor(theta, device=DEV, requires_grad=True)
    out = functional.warp_coords(c, t)
    assert out.shape == c.shape and out.dtype == torch.float32
    assert out.detach().cpu().numpy().tobytes() == ref.warp(coords, theta).tobytes()
    out.backward(torch.tensor(g, device=DEV))
    torch.cuda.synchronize()
    assert t.grad.cpu().numpy().tobytes() == g_theta.tobytes() and c.grad.cpu().numpy().tobytes() == g_in.tobytes()
    # coords that do not require a gradient receive none
    c2 = torch.tensor(coords, device=DEV)
    t2 = torch.tensor(theta, device=DEV, requires_grad=True)
    functional.warp_coords(c2, t2).backward(torch.tensor(g, device=DEV))
    torch.cuda.synchronize()
    assert c2.grad is None and t2.grad.cpu().numpy().tobytes() == g_theta.tobytes()
    with pytest.raises(ValueError, match="theta"):
        functional.warp_coords(c2, t2[:2])
    with pytest.raises(ValueError, match="coords"):
        functional.warp_coords(c2[:, :, :1], t2)


# ---------------------------------------------------------------------------------------------------------------------
# the step (helpers copied from tests/test_gpu_multi_sr.py)
# ---------------------------------------------------------------------------------------------------------------------
def _mats(thetas, shifts):
    from wire_amd.modules import motion
    return np.stack([motion.getEuclidianMatrix(t, s) for t, s in zip(thetas, shifts)])


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


def _tensors(model, tr):
    names = [k for k in model.state_dict().keys() if "omega_0" not in k and "scale_0" not in k]
    assert len(names) == len(tr.offsets)
    return list(zip(names, tr.offsets))


def _perturbed_theta(B):
    """The identity, plus a fixed perturbation of size 1e-2 in the frames >= 1."""
    rng = np.random.default_rng(77)
    t = np.broadcast_to(np.array([[1, 0, 0], [0, 1, 0]], np.float32), (B, 2, 3)).copy()
    t[1:] += (1e-2 * rng.uniform(-1, 1, (B - 1, 2, 3))).astype(np.float32)
    return t


def _setup(kind, B, H, W, scale, seed, lr=0.0):
    """A trainer at ``lr``, the base coordinates of rigidly moved frames, targets and a mask with zeros in every frame."""
    from wire_amd.trainer import FusedTrainer
    O = 3
    rng = np.random.default_rng(seed)
    H2, W2 = H // scale, W // scale
    model, hp = _net(kind, O)
    tr = FusedTrainer(model, (H, W), None, lr=lr)
    thetas = [0.0, np.pi / 10, -np.pi / 12][:B]
    shifts = [(0, 0), (3, -2), (-4, 1)][:B]
    coords = tr.affine_coords(_mats(thetas, shifts))
    gt = rng.uniform(0, 1, (B, H2 * W2, O)).astype(np.float32)
    mask = multi_sr_ref.make_mask(rng, B + 1, H2 * W2, O)[:B]
    return tr, model, hp, coords, gt, mask


def _torch_params(model, double):
    P = {k: v.detach().cpu() for k, v in model.state_dict().items() if "omega_0" not in k and "scale_0" not in k}
    return {k: (v.to(torch.complex128 if double else torch.complex64) if v.is_complex()
                else v.to(torch.float64 if double else torch.float32)).clone().requires_grad_(True)
            for k, v in P.items()}


def _eager_loss(kind, p, hp, warped, B, H, W, scale, gt, mask):
    """The eager forward of oracle/torch_ref.py on the warped rows and multi_sr_ref.frames_loss_and_grad's loss in torch:
    AvgPool2d(scale) of every frame, MSELoss()(rec * mask, gt * mask)."""
    x = warped.reshape(-1, 2)
    y = torch_ref.wire_forward(p, x, 2, *hp) if kind == "wire" else torch_ref.realnet_forward(kind, p, x, 2, *hp)
    O = y.shape[-1]
    rec = F.avg_pool2d(y.reshape(B, H, W, O).permute(0, 3, 1, 2), scale).permute(0, 2, 3, 1).reshape(B, -1, O)
    return F.mse_loss(rec * mask, gt * mask)


def _warp_torch(base, theta):
    ones = torch.ones(base.shape[:2] + (1,), dtype=base.dtype)
    return torch.einsum("fak,fpk->fpa", theta, torch.cat([base, ones], dim=-1))


def _oracle(kind, model, hp, base, theta, B, H, W, scale, gt, mask, double):
    """-> loss, {name: gradient as real pairs}, d loss / d warped coords [B*H*W, 2], d loss / d theta [B, 2, 3]."""
    dt = torch.float64 if double else torch.float32
    p = _torch_params(model, double)
    t = torch.tensor(theta, dtype=dt, requires_grad=True)
    with torch.enable_grad():
        warped = _warp_torch(torch.tensor(base, dtype=dt), t)
        warped.retain_grad()
        loss = _eager_loss(kind, p, hp, warped, B, H, W, scale, torch.tensor(gt, dtype=dt), torch.tensor(mask, dtype=dt))
        loss.backward()
    grads = {k: (torch.view_as_real(v.grad) if v.is_complex() else v.grad).to(torch.float64).reshape(-1).numpy()
             for k, v in p.items()}
    return float(loss.detach()), grads, warped.grad.to(torch.float64).reshape(-1, 2).numpy(), t.grad.to(torch.float64).numpy()


@functools.lru_cache(maxsize=None)
def _grad_case(kind, B, H, W, scale, seed, pin):
    """One lr = 0, reg.lr = 0 step on perturbed frames, and the eager oracle in fp64 and fp32, computed once."""
    tr, model, hp, coords, gt, mask = _setup(kind, B, H, W, scale, seed)
    theta = _perturbed_theta(B)
    reg = tr.registration(B, lr=0.0, pin_first=pin, theta=theta)
    loss = tr.step_frames_registered(reg, coords, torch.tensor(gt, device=DEV), scale,
                                     mask=torch.tensor(mask, device=DEV))
    torch.cuda.synchronize()
    n = B * H * W
    base = coords.cpu().numpy()
    out = dict(tr=tr, model=model, B=B, n=n, base=base, theta=theta, pin=pin, loss=float(loss.item()),
               flat=tr.flat_grad.cpu().numpy().copy(), g_coords=tr.g_coords[:n].cpu().numpy().copy(),
               warped=tr.coords[:2 * n].cpu().numpy().reshape(B, H * W, 2).copy(),
               g_theta=reg.grad.cpu().numpy().copy(), theta_after=reg.theta.cpu().numpy().copy(), mask=mask)
    out["o64"] = _oracle(kind, model, hp, base, theta, B, H, W, scale, gt, mask, True)
    out["o32"] = _oracle(kind, model, hp, base, theta, B, H, W, scale, gt, mask, False)
    return out


# case (a): 1 638 rows, the 3 x bf16 family; case (b): 4 608 rows, above the 4 096-row switch to the 2 x fp16 family
GRAD_CASES = [("wire", 3, 26, 21, 4, 5, True), ("wire", 2, 48, 48, 4, 6, False), ("siren", 2, 48, 48, 4, 6, False)]


@pytest.mark.parametrize("kind,B,H,W,scale,seed,pin", GRAD_CASES)
def test_step_registered_gradients_within_reference_error(kind, B, H, W, scale, seed, pin):
    """Loss and every parameter gradient within 3 x the fp32 eager oracle's own error against fp64 + 1e-6 (the bound of
    test_step_frames_fp16_family_within_reference_error); dL/d(warped coords) within 2 x (tests/test_gpu_coords_grad.py);
    reg.grad against the fp64 reduction of the BUILD'S OWN g_coords within the kernel's bound -- six numbers that can
    cancel are not judged by a relative error of their own -- and, as a check of the wiring, against the oracle's
    dL/dtheta within 2 x.  The warped coordinates the step used are the restatement's bits; lr = 0 leaves theta alone."""
    c = _grad_case(kind, B, H, W, scale, seed, pin)
    l64, g64, gc64, gt64 = c["o64"]
    l32, g32, gc32, gt32 = c["o32"]
    assert (c["mask"] == 0).any()
    assert c["warped"].tobytes() == ref.warp(c["base"], c["theta"]).tobytes()
    assert c["theta_after"].tobytes() == c["theta"].tobytes()
    label = f"step_frames_registered {kind} {B}x{H}x{W}"
    checks = [(f"{label} loss", abs(c["loss"] - l64) / l64, abs(l32 - l64) / l64, 3.0)]
    for name, off in _tensors(c["model"], c["tr"]):
        g = g64[name]
        checks.append((f"{label} {name}", relmax(c["flat"][off:off + g.size], g), relmax(g32[name], g), 3.0))
    checks.append((f"{label} g_coords", relmax(c["g_coords"], gc64), relmax(gc32, gc64), 2.0))
    if pin:
        gt64, gt32 = gt64.copy(), gt32.copy()
        gt64[0] = 0.0
        gt32[0] = 0.0
    checks.append((f"{label} g_theta", relmax(c["g_theta"], gt64), relmax(gt32, gt64), 2.0))
    S, A, _ = ref.warp_bwd(c["base"], c["theta"], c["g_coords"].reshape(B, H * W, 2), int(pin))
    err, bound = np.abs(c["g_theta"].astype(np.float64) - S), ref.g_theta_bound(S, A, H * W)
    for lab, eb, er, f in checks:
        print(f"{lab}: err_build {eb:.3e}  err_ref {er:.3e}  ratio {eb / er if er > 0 else float('inf'):.2f}")
    print(f"{label} g_theta vs fp64 sum of own g_coords: worst err / bound {(err / np.maximum(bound, 1e-300)).max():.3f}; "
          f"min|g_theta| / max|g_theta| over free frames {np.abs(gt64[int(pin):]).min() / np.abs(gt64).max():.3f}")
    for lab, eb, er, f in checks:
        within_ref(eb, er, lab, factor=f)
    assert (err <= bound).all()
    if pin:
        assert c["g_theta"][0].tobytes() == np.zeros((2, 3), np.float32).tobytes()


@pytest.mark.parametrize("kind,B,H,W,scale,seed", [("wire", 3, 26, 21, 4, 5), ("siren", 2, 48, 48, 4, 6)])
def test_identity_registration_gives_the_loss_of_step_frames(kind, B, H, W, scale, seed):
    """Identity theta: the forward and the loss kernel are step_frames', and the identity warp is exact, so the loss has
    the same bits.  Whether the parameter gradients (wire_mlp_bwd_coords against wire_mlp_bwd) are bit-equal too is
    printed, not asserted."""
    tr, model, hp, coords, gt, mask = _setup(kind, B, H, W, scale, seed)
    gtt, mt = torch.tensor(gt, device=DEV), torch.tensor(mask, device=DEV)
    l0 = tr.step_frames(coords, gtt, scale, mask=mt)
    torch.cuda.synchronize()
    l0, g0 = l0.cpu().numpy().copy(), tr.flat_grad.cpu().numpy().copy()
    reg = tr.registration(B, lr=0.0)
    l1 = tr.step_frames_registered(reg, coords, gtt, scale, mask=mt)
    torch.cuda.synchronize()
    g1 = tr.flat_grad.cpu().numpy()
    print(f"identity registration {kind}: parameter gradients bit-equal to step_frames': {g0.tobytes() == g1.tobytes()}"
          f" (max |diff| / max|g| {np.abs(g1 - g0).max() / np.abs(g0).max():.2e})")
    assert l1.cpu().numpy().tobytes() == l0.tobytes()
    assert tr.coords[:2 * B * H * W].cpu().numpy().tobytes() == coords.cpu().numpy().tobytes()


def test_registration_adam_step_moves_theta_only():
    """One step with lr = 0 and reg.lr = 1e-3 from the identity: every entry of theta moves by Adam's first step,
    -lr g / (|g| + eps), computed from reg.grad in fp64, within 2 ulp of the entry; the pinned frame 0 stays exactly the
    identity; no net parameter changes, bit for bit."""
    B, H, W, scale = 3, 26, 21, 4
    tr, model, hp, coords, gt, mask = _setup("wire", B, H, W, scale, 5)
    before = tr.flat.cpu().numpy().copy()
    reg = tr.registration(B, lr=1e-3)
    eye = reg.theta.cpu().numpy().copy()
    assert eye.tobytes() == np.broadcast_to(np.array([[1, 0, 0], [0, 1, 0]], np.float32), (B, 2, 3)).tobytes()
    tr.step_frames_registered(reg, coords, torch.tensor(gt, device=DEV), scale, mask=torch.tensor(mask, device=DEV))
    torch.cuda.synchronize()
    g = reg.grad.cpu().numpy().astype(np.float64)
    got = reg.theta.cpu().numpy()
    want = eye.astype(np.float64) - 1e-3 * g / (np.abs(g) + 1e-8)
    ulp = np.spacing(np.abs(want).astype(np.float32)).astype(np.float64)
    print(f"registration Adam step: worst |theta - expected| in ulp {(np.abs(got - want) / ulp).max():.3f}; "
          f"|g| from {np.abs(g[1:]).min():.3e} to {np.abs(g).max():.3e}")
    assert reg.t == 1 and tr.t == 1
    assert np.abs(g[1:]).min() > 0 and not g[0].any()
    assert (np.abs(got - want) <= 2 * ulp).all()
    assert got[0].tobytes() == eye[0].tobytes()
    assert not reg.exp_avg[0].any().item() and not reg.exp_avg_sq[0].any().item()
    assert tr.flat.cpu().numpy().tobytes() == before.tobytes()


def test_registration_descends_like_the_fp64_twin():
    """siren 2 x 128, 3 frames of 26 x 21, scale 4, the net frozen (lr = 0), reg.lr = 1e-3, 11 calls: the loss of call 11
    lies below the loss of call 1 by at least HALF of the decrease of an fp64 eager twin (torch Adam on theta with the
    same betas and eps, frame 0's gradient zeroed).  The twin's decrease over the ten updates is some 1e-4 of a loss of
    0.15, 20 times the 2e-5 relative loss accuracy of the step tests at each end; one half is a condition, the measured
    ratio is printed."""
    kind, B, H, W, scale = "siren", 3, 26, 21, 4
    tr, model, hp, coords, gt, mask = _setup(kind, B, H, W, scale, 5)
    reg = tr.registration(B, lr=1e-3)
    gtt, mt = torch.tensor(gt, device=DEV), torch.tensor(mask, device=DEV)
    losses = [tr.step_frames_registered(reg, coords, gtt, scale, mask=mt) for _ in range(11)]
    torch.cuda.synchronize()
    losses = [float(v.item()) for v in losses]
    # the twin
    p = _torch_params(model, True)
    base = torch.tensor(coords.cpu().numpy(), dtype=torch.float64)
    t = torch.eye(2, 3, dtype=torch.float64).repeat(B, 1, 1).requires_grad_(True)
    opt = torch.optim.Adam([t], lr=1e-3, betas=(0.9, 0.999), eps=1e-8)
    g64, m64 = torch.tensor(gt, dtype=torch.float64), torch.tensor(mask, dtype=torch.float64)
    twin = []
    for _ in range(11):
        opt.zero_grad()
        with torch.enable_grad():
            loss = _eager_loss(kind, p, hp, _warp_torch(base, t), B, H, W, scale, g64, m64)
            loss.backward()
        t.grad[0] = 0.0
        opt.step()
        twin.append(float(loss.detach()))
    drop, want = losses[0] - losses[10], twin[0] - twin[10]
    print(f"registration descent: build {losses[0]:.6f} -> {losses[10]:.6f} ({drop:.3e}), fp64 twin {twin[0]:.6f} -> "
          f"{twin[10]:.6f} ({want:.3e}), ratio {drop / want:.3f}")
    assert want > 0
    assert drop >= 0.5 * want
    assert reg.t == 11 and reg.theta[0].cpu().numpy().tobytes() == np.eye(2, 3, dtype=np.float32).tobytes()


def test_registered_step_ignores_what_the_workspaces_held():
    """After one step (which allocates everything) every workspace is filled with 0xFF bytes; a second step at
    lr = reg.lr = 0 gives the loss, flat_grad and reg.grad bits of a fresh trainer's first step."""
    B, H, W, scale = 3, 26, 21, 4

    def first():
        tr, model, hp, coords, gt, mask = _setup("wire", B, H, W, scale, 5)
        reg = tr.registration(B, lr=0.0, theta=_perturbed_theta(B))
        args = (reg, coords, torch.tensor(gt, device=DEV), scale)
        kw = dict(mask=torch.tensor(mask, device=DEV))
        loss = tr.step_frames_registered(*args, **kw)
        torch.cuda.synchronize()
        return tr, reg, args, kw, (loss.cpu().numpy().tobytes(), tr.flat_grad.cpu().numpy().tobytes(),
                                   reg.grad.cpu().numpy().tobytes())

    _, _, _, _, fresh = first()
    tr, reg, args, kw, one = first()
    assert one == fresh
    for buf in (tr.act, tr.scratch, tr.coords_scratch, tr.warp_ws, tr.g_coords, tr.coords, tr.y, tr.gy, reg.grad):
        buf.view(torch.uint8).fill_(0xFF)
    loss = tr.step_frames_registered(*args, **kw)
    torch.cuda.synchronize()
    assert loss.cpu().numpy().tobytes() == fresh[0]
    assert tr.flat_grad.cpu().numpy().tobytes() == fresh[1]
    assert reg.grad.cpu().numpy().tobytes() == fresh[2]


def test_registered_step_errors():
    from wire_amd.modules import models
    from wire_amd.trainer import FusedTrainer
    H, W, scale, O, B = 12, 10, 2, 3, 3
    torch.manual_seed(3)
    model = models.get_INR(nonlin="wire", in_features=2, out_features=O, hidden_features=64, hidden_layers=2,
                           first_omega_0=7.0, hidden_omega_0=7.0, scale=6.0).to(DEV)
    tr = FusedTrainer(model, (H, W), None, lr=0.0)
    coords = tr.affine_coords(_mats([0.0, 0.2, -0.1], [(0, 0), (2, 1), (-1, 3)]))
    gt = torch.rand(B, (H // scale) * (W // scale), O, device=DEV)
    reg = tr.registration(B)
    with pytest.raises(ValueError, match="frames"):
        tr.step_frames_registered(tr.registration(2), coords, gt, scale)
    with pytest.raises(ValueError, match="FrameRegistration"):
        tr.step_frames_registered(None, coords, gt, scale)
    with pytest.raises(ValueError, match="coords"):
        tr.step_frames_registered(reg, coords[:, :-1], gt, scale)
    with pytest.raises(ValueError, match="gt_lr"):
        tr.step_frames_registered(reg, coords, gt[:2], scale)
    with pytest.raises(ValueError, match="scale"):
        tr.step_frames_registered(reg, coords, gt, 0)
    with pytest.raises(ValueError, match="mask"):
        tr.step_frames_registered(reg, coords, gt, scale, mask=gt[:1])
    with pytest.raises(ValueError, match="rec_lr"):
        tr.step_frames_registered(reg, coords, gt, scale, rec_lr=gt[:, :-1])
    with pytest.raises(ValueError, match=r"theta must be"):
        tr.registration(B, theta=np.zeros((B, 3, 2), np.float32))
    with pytest.raises(ValueError, match="B >= 1"):
        tr.registration(0)
    assert reg.t == 0 and tr.t == 0
    # a 3-D grid
    m3 = models.get_INR(nonlin="wire", in_features=3, out_features=1, hidden_features=32, hidden_layers=1).to(DEV)
    tr3 = FusedTrainer(m3, (4, 5, 3), None, lr=0.0)
    with pytest.raises(ValueError, match="2-D grid"):
        tr3.step_frames_registered(reg, coords, gt, scale)
    with pytest.raises(ValueError, match="2-D grid"):
        tr3.registration(B)
