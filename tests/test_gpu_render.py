"""Volume rendering on the MI355X (wire_amd/csrc/wire_render.hip): the sampler bit for bit against the fp64 restatement
tests/render_ref.py, the compositing operator and its adjoint against the restatement within the error of eager fp32
torch on the same inputs (_util.within_ref: 2 x err_ref + 1e-6), the value edges, determinism and completeness, the
autograd Function, one ``step_rays`` against the fp64 oracle net composed with the restatement, a short training
trajectory against an fp64 eager loop, and ``render_rays``."""
import ctypes as C

import numpy as np
import pytest
import torch

import envelope_ref as er
import render_ref as rr
from _util import family_ctx, relmax, within_ref
from oracle import torch_ref
from oracle import wire_oracle as wo

pytestmark = pytest.mark.gpu
DEV = "cuda"
RPW = 4                          # rays per workgroup (RENDER_RAYS_PER_WG): one wave each
NAN = float("nan")
MODE = {"softplus": 0, "relu": 1}


def _dev(a, dt=torch.float32):
    return None if a is None else torch.as_tensor(np.ascontiguousarray(a)).to(DEV, dt).contiguous()


def _ptr(t):
    return None if t is None else t.data_ptr()


def _call(name, *args):
    from wire_amd import _lib
    _lib.check(getattr(_lib.lib(), name)(torch.cuda.current_stream().cuda_stream, *args), name)


def _full(*shape):
    return torch.full(shape, NAN, dtype=torch.float32, device=DEV)


def abi_samples(rays, near, far, S, jitter):
    R = rays.shape[0]
    r, u = _dev(rays), _dev(jitter)
    bounds = None if np.ndim(near) == 0 else _dev(np.stack([near, far], 1))
    coords, ts, dl = _full(R * S, 3), _full(R, S), _full(R, S)
    _call("wire_ray_samples", r.data_ptr(), _ptr(bounds), 0.0 if bounds is not None else float(near),
          0.0 if bounds is not None else float(far), _ptr(u), R, S, coords.data_ptr(), ts.data_ptr(), dl.data_ptr())
    torch.cuda.synchronize()
    return coords.cpu().numpy(), ts.cpu().numpy(), dl.cpu().numpy()


class Dev:
    """The inputs of a compositing case on the device."""

    def __init__(self, y, ts, dl, bg, density):
        self.R, self.S = ts.shape
        self.O = y.shape[-1]
        self.y, self.ts, self.dl, self.bg, self.mode = _dev(y), _dev(ts), _dev(dl), _dev(bg), MODE[density]

    def fwd(self):
        rgb, acc, depth = _full(self.R, self.O - 1), _full(self.R), _full(self.R)
        _call("wire_composite_fwd", self.y.data_ptr(), self.ts.data_ptr(), self.dl.data_ptr(), _ptr(self.bg), self.R,
              self.S, self.O, self.mode, rgb.data_ptr(), acc.data_ptr(), depth.data_ptr())
        return rgb, acc, depth

    def bwd(self, g_rgb, g_acc=None, g_depth=None):
        g_y = _full(self.R * self.S, self.O)
        _call("wire_composite_bwd", self.y.data_ptr(), self.ts.data_ptr(), self.dl.data_ptr(), _ptr(self.bg),
              g_rgb.data_ptr(), _ptr(g_acc), _ptr(g_depth), self.R, self.S, self.O, self.mode, g_y.data_ptr())
        return g_y

    def mse(self, target, want_rgb=True, fill=NAN):
        g_y = _full(self.R * self.S, self.O)
        loss, rgb = _full(1), (_full(self.R, self.O - 1) if want_rgb else None)
        partial = torch.full((4096,), fill, dtype=torch.float32, device=DEV)
        _call("wire_composite_mse_grad", self.y.data_ptr(), self.ts.data_ptr(), self.dl.data_ptr(), _ptr(self.bg),
              target.data_ptr(), self.R, self.S, self.O, self.mode, 1.0, g_y.data_ptr(), loss.data_ptr(), _ptr(rgb),
              partial.data_ptr())
        return loss, g_y, rgb, partial


def _np(*ts):
    torch.cuda.synchronize()
    return [t.cpu().numpy() for t in ts]


# ---------------------------------------------------------------------------------------------------------------------
# the sampler
# ---------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("R,S", [(1, 1), (3, 63), (4, 64), (5, 65), (257, 130)])
def test_sampler_equals_the_restatement_bit_for_bit(R, S):
    rng = np.random.default_rng(100 * R + S)
    rays = np.concatenate([rng.uniform(-2, 2, (R, 3)), rng.normal(0, 1, (R, 3))], 1).astype(np.float32)
    near_t = rng.uniform(0.1, 1.0, R).astype(np.float32)
    far_t = (near_t + rng.uniform(0.5, 3.0, R)).astype(np.float32)
    if R > 1:
        far_t[R // 2] = near_t[R // 2] - np.float32(0.25)                  # one ray misses: far <= near
    u = rng.uniform(0, 1, (R, S)).astype(np.float32)
    for near, far in ((np.float32(0.3), np.float32(2.7)), (near_t, far_t)):
        for jitter in (None, u):
            got = abi_samples(rays, near, far, S, jitter)
            want = rr.ray_samples(rays, near, far, S, jitter)
            for name, g, w in zip(("coords", "ts", "deltas"), got, want):
                assert g.shape == w.shape and g.tobytes() == w.tobytes(), (name, np.ndim(near), jitter is None)
    if R > 1:
        assert np.all(got[2][R // 2] == 0) and np.all(got[1][R // 2] == near_t[R // 2])


def test_functional_ray_samples_is_the_abi_call():
    from wire_amd import functional
    rng = np.random.default_rng(5)
    rays = rng.normal(0, 1, (9, 6)).astype(np.float32)
    near, far = rng.uniform(0, 1, 9).astype(np.float32), rng.uniform(1, 2, 9).astype(np.float32)
    u = rng.uniform(0, 1, (9, 20)).astype(np.float32)
    coords, ts, dl = functional.ray_samples(_dev(rays), _dev(near), _dev(far), 20, jitter=_dev(u))
    want = rr.ray_samples(rays, near, far, 20, u)
    assert coords.shape == (180, 3) and ts.shape == dl.shape == (9, 20) and not coords.requires_grad
    for g, w in zip(_np(coords, ts, dl), want):
        assert g.tobytes() == w.tobytes()
    coords, ts, dl = functional.ray_samples(_dev(rays), 0.5, 1.5, 20)
    for g, w in zip(_np(coords, ts, dl), rr.ray_samples(rays, np.float32(0.5), np.float32(1.5), 20)):
        assert g.tobytes() == w.tobytes()


# ---------------------------------------------------------------------------------------------------------------------
# compositing, forward and backward, against fp64 within eager fp32's own error
# ---------------------------------------------------------------------------------------------------------------------
def _inputs(R, S, C, seed):
    rng = np.random.default_rng(seed)
    y = rng.normal(0, 1.5, (R * S, C + 1)).astype(np.float32)
    y[:, -1] += np.float32(0.5)
    ts = np.sort(rng.uniform(0.5, 3.0, (R, S)), axis=1).astype(np.float32)
    dl = rng.uniform(0.0, 6.0 / S, (R, S)).astype(np.float32)
    bg = rng.uniform(0, 1, C).astype(np.float32)
    g = [rng.normal(0, 1, (R, C)).astype(np.float32), rng.normal(0, 1, R).astype(np.float32),
         rng.normal(0, 1, R).astype(np.float32)]
    return y, ts, dl, bg, g


def _eager32(y, ts, dl, bg, density, g):
    """Eager torch fp32 (cumsum / cumprod form) on the host: outputs and, by autograd, the adjoint."""
    yt = torch.tensor(y, requires_grad=True)
    out = rr.torch_composite(yt, torch.tensor(ts), torch.tensor(dl), None if bg is None else torch.tensor(bg), density)
    sum((o * torch.tensor(w)).sum() for o, w in zip(out, g)).backward()
    return [o.detach().numpy() for o in out], yt.grad.numpy().reshape(y.shape)


def _check_case(y, ts, dl, bg, density, g, label):
    """Forward and backward of one case: finite everywhere, every element written, within the bound."""
    d = Dev(y, ts, dl, bg, density)
    rgb, acc, depth = d.fwd()
    g_y = d.bwd(*[_dev(v) for v in g])
    rgb, acc, depth, g_y = _np(rgb, acc, depth, g_y)
    for name, v in (("rgb", rgb), ("acc", acc), ("depth", depth), ("g_y", g_y)):
        assert np.isfinite(v).all(), f"{label}: {name} holds a NaN or an inf"
    want = rr.composite(y, ts, dl, bg, density)
    want_g = rr.composite_bwd(y, ts, dl, *g, bg=bg, density=density)
    ref, ref_g = _eager32(y, ts, dl, bg, density, g)
    for name, got, w, r in (("rgb", rgb, want[0], ref[0]), ("acc", acc, want[1], ref[1]),
                            ("depth", depth, want[2], ref[2]), ("g_y", g_y, want_g, ref_g)):
        within_ref(relmax(got, w), relmax(r, w), f"composite {label} {name}")
    return rgb, acc, depth, g_y


@pytest.mark.parametrize("S", [1, 2, 63, 64, 65, 130])
@pytest.mark.parametrize("C", [1, 3, 7])
def test_composite_against_fp64(C, S):
    """Both density modes, bg present and absent, R one fewer than, equal to and one more than the rays of a workgroup;
    S at the chunk and carry edges; O = 2, 4, 8 (rows moved as float2 / float4 / two float4)."""
    for density in ("softplus", "relu"):
        for with_bg in (False, True):
            for R in (RPW - 1, RPW, RPW + 1):
                y, ts, dl, bg, g = _inputs(R, S, C, 7 * S + C + R)
                _check_case(y, ts, dl, bg if with_bg else None, density, g,
                            f"C={C} S={S} R={R} {density} bg={int(with_bg)}")


@pytest.mark.parametrize("C,S", [(2, 65), (4, 7), (5, 130), (6, 64), (3, 4200)])
def test_composite_other_row_widths(C, S):
    """O = 3, 5, 7 (rows moved float by float) and 6 (three float2); S = 4200: 66 chunks, past the 64 whose carries a
    wave keeps in registers, so the adjoint recomputes the last two."""
    y, ts, dl, bg, g = _inputs(9, S, C, 11 * C)
    _check_case(y, ts, dl, bg, "softplus", g, f"C={C} S={S} R=9")


def test_loss_kernel_with_more_workgroups_than_partial_slots():
    """16 389 rays at S = 2: 4 098 workgroups' worth of rays, more than the 4 096 slots of the trainer's ``partial`` and
    than the 2 048 blocks the loss kernel launches, so waves walk several rays.  Loss, g_y and rgb against fp64."""
    R, S, C = 4 * 4096 + 5, 2, 3
    y, ts, dl, bg, _ = _inputs(R, S, C, 77)
    tgt = np.random.default_rng(78).uniform(0, 1, (R, C)).astype(np.float32)
    d = Dev(y, ts, dl, bg, "softplus")
    loss, g_y, rgb, _ = d.mse(_dev(tgt))
    loss, g_y, rgb = _np(loss, g_y, rgb)
    assert np.isfinite(loss).all() and np.isfinite(g_y).all() and np.isfinite(rgb).all()
    want = rr.composite(y, ts, dl, bg)[0]
    l64, g_rgb = rr.mse_and_grad(want, tgt)
    want_g = rr.composite_bwd(y, ts, dl, g_rgb, bg=bg)
    yt = torch.tensor(y, requires_grad=True)
    r32 = rr.torch_composite(yt, torch.tensor(ts), torch.tensor(dl), torch.tensor(bg))[0]
    l32 = ((r32 - torch.tensor(tgt)) ** 2).mean()
    l32.backward()
    l32 = l32.detach()
    within_ref(abs(float(loss[0]) - l64) / l64, abs(float(l32) - l64) / l64, "composite_mse_grad R=16389 loss")
    within_ref(relmax(rgb, want), relmax(r32.detach().numpy(), want), "composite_mse_grad R=16389 rgb")
    within_ref(relmax(g_y, want_g), relmax(yt.grad.numpy(), want_g), "composite_mse_grad R=16389 g_y")


# ---------------------------------------------------------------------------------------------------------------------
# value edges
# ---------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("density", ["softplus", "relu"])
def test_empty_space(density):
    """s_raw = -80 everywhere: acc == 0 and rgb == bg exactly under relu, within the bound under softplus."""
    y, ts, dl, bg, g = _inputs(6, 70, 3, 21)
    y[:, -1] = -80.0
    rgb, acc, depth, g_y = _check_case(y, ts, dl, bg, density, g, f"s_raw=-80 {density}")
    if density == "relu":
        assert np.all(acc == 0) and np.all(depth == 0) and rgb.tobytes() == np.tile(bg, (6, 1)).tobytes()
        assert np.all(g_y == 0)


@pytest.mark.parametrize("density", ["softplus", "relu"])
def test_opaque_first_sample(density):
    """s_raw = +80 at the first sample: the ray is opaque from there on; the later samples' gradients stay finite and
    within the bound."""
    y, ts, dl, bg, g = _inputs(6, 70, 3, 22)
    y.reshape(6, 70, 4)[:, 0, -1] = 80.0
    dl[:, 0] = 0.5
    rgb, acc, depth, g_y = _check_case(y, ts, dl, bg, density, g, f"s_raw=+80 {density}")
    assert np.all(acc == 1)


def test_zero_length_samples():
    """deltas == 0 on whole rays (they give the background and no gradient) and on scattered samples."""
    y, ts, dl, bg, g = _inputs(6, 70, 3, 23)
    dl[1] = 0.0
    dl[4] = 0.0
    dl[2, ::3] = 0.0
    rgb, acc, depth, g_y = _check_case(y, ts, dl, bg, "softplus", g, "deltas=0")
    g_y = g_y.reshape(6, 70, 4)
    for r in (1, 4):
        assert rgb[r].tobytes() == bg.tobytes() and acc[r] == 0 and depth[r] == 0 and np.all(g_y[r] == 0)
    assert np.all(g_y[2, ::3] == 0) and np.abs(g_y[2, 1::3]).min() > 0


def test_saturated_colours():
    y, ts, dl, bg, g = _inputs(6, 70, 3, 24)
    y[::2, :3] = 40.0
    y[1::2, :3] = -40.0
    _check_case(y, ts, dl, bg, "softplus", g, "c_raw=+-40")


# ---------------------------------------------------------------------------------------------------------------------
# determinism and completeness
# ---------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("R,S,C", [(5, 65, 3), (4 * 2048 + 3, 2, 1), (9, 130, 7)])
def test_every_element_written_same_bits_and_both_routes_agree(R, S, C):
    """Outputs prefilled with NaN and ``partial`` with NaN, then 0xFF: every element of g_y, rgb and loss is written,
    two calls give equal bits, and wire_composite_mse_grad gives the bits of wire_composite_fwd -> the residual formed in
    fp32 on the host side -> wire_composite_bwd for g_y and rgb."""
    y, ts, dl, bg, _ = _inputs(R, S, C, 31)
    tgt = _dev(np.random.default_rng(32).uniform(0, 1, (R, C)).astype(np.float32))
    d = Dev(y, ts, dl, bg, "softplus")
    a = _np(*d.mse(tgt)[:3])
    partial_ff = torch.full((4096,), NAN, dtype=torch.float32, device=DEV)
    partial_ff.view(torch.int32).fill_(-1)
    b = _np(*d.mse(tgt)[:3])
    for u, v in zip(a, b):
        assert not np.isnan(u).any() and u.tobytes() == v.tobytes()
    # 0xFF bytes in partial
    g_y, loss, rgb = _full(R * S, C + 1), _full(1), _full(R, C)
    _call("wire_composite_mse_grad", d.y.data_ptr(), d.ts.data_ptr(), d.dl.data_ptr(), _ptr(d.bg), tgt.data_ptr(), R, S,
          C + 1, 0, 1.0, g_y.data_ptr(), loss.data_ptr(), rgb.data_ptr(), partial_ff.data_ptr())
    c = _np(loss, g_y, rgb)
    for u, v in zip(a, c):
        assert u.tobytes() == v.tobytes()
    # the two-launch route
    rgb2, acc2, depth2 = d.fwd()
    scale = np.float32(1.0) * np.float32(1.0 / (float(R) * float(C)))
    g_rgb = (rgb2 - tgt) * float(np.float32(2.0) * scale)
    g2 = d.bwd(g_rgb)
    rgb2b, g2b = _np(*d.fwd()[:1], d.bwd(g_rgb))
    rgb2, acc2, depth2, g2 = _np(rgb2, acc2, depth2, g2)
    assert not np.isnan(g2).any() and not np.isnan(rgb2).any() and not np.isnan(acc2).any() and not np.isnan(depth2).any()
    assert rgb2.tobytes() == rgb2b.tobytes() and g2.tobytes() == g2b.tobytes()
    assert a[2].tobytes() == rgb2.tobytes() and a[1].tobytes() == g2.tobytes()


# ---------------------------------------------------------------------------------------------------------------------
# functional.composite
# ---------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("density", ["softplus", "relu"])
def test_functional_composite_is_the_abi_pair(density):
    from wire_amd import functional
    R, S, C = 7, 66, 3
    y, ts, dl, bg, g = _inputs(R, S, C, 41)
    d = Dev(y, ts, dl, bg, density)
    want = _np(*d.fwd(), d.bwd(*[_dev(v) for v in g]))
    yt = _dev(y).requires_grad_(True)
    out = functional.composite(yt, d.ts, d.dl, background=bg, density=density)
    assert [tuple(o.shape) for o in out] == [(R, C), (R,), (R,)]
    f = sum((o * _dev(w)).sum() for o, w in zip(out, g))
    gy, = torch.autograd.grad(f, yt)
    got = _np(*[o.detach() for o in out], gy)
    for u, v in zip(got, want):
        assert u.tobytes() == v.tobytes()
    # [R, S, O] input: the gradient comes back in that shape; rgb alone: the absent gradients count as zero
    y3 = _dev(y).reshape(R, S, C + 1).requires_grad_(True)
    rgb = functional.composite(y3, d.ts, d.dl, background=bg, density=density)[0]
    g3, = torch.autograd.grad((rgb * _dev(g[0])).sum(), y3)
    want3, = _np(d.bwd(_dev(g[0])))
    assert g3.shape == y3.shape and g3.cpu().numpy().tobytes() == want3.tobytes()
    # refusals
    with pytest.raises(NotImplementedError):
        torch.autograd.grad(functional.composite(yt, d.ts, d.dl)[0].sum(), yt, create_graph=True)
    with pytest.raises(NotImplementedError):
        functional.composite(yt, d.ts.clone().requires_grad_(True), d.dl)
    with pytest.raises(NotImplementedError):
        functional.composite(yt, d.ts, d.dl.clone().requires_grad_(True))
    with pytest.raises(ValueError):
        functional.composite(yt, d.ts, d.dl, background=[0.1, 0.2])
    with pytest.raises(ValueError):
        functional.composite(yt, d.ts, d.dl.cpu())


# ---------------------------------------------------------------------------------------------------------------------
# FusedTrainer.step_rays: one step against the fp64 oracle net composed with the restatement
# ---------------------------------------------------------------------------------------------------------------------
def _rays(R, seed):
    """Rays that start outside the cube [-1, 1]^3 and look at a point inside it."""
    rng = np.random.default_rng(seed)
    o = rng.normal(0, 1, (R, 3))
    o = 2.5 * o / np.linalg.norm(o, axis=1, keepdims=True)
    d = rng.uniform(-0.5, 0.5, (R, 3)) - o
    return np.concatenate([o, d / np.linalg.norm(d, axis=1, keepdims=True)], 1).astype(np.float32)


def _oracle_step(net, sd, coords, ts, dl, tgt, bg, density, double):
    """Loss and every parameter gradient: oracle.wire_oracle's net on the sample points, the restatement's compositing
    and MSE on its rows, the closed-form adjoint, the oracle's backward."""
    c = er.NETS[net]
    dt = np.float64 if double else np.float32
    p = wo.cast_params(sd, double)
    a = tuple(dt(c["kw"][k]) for k in ("first_omega_0", "hidden_omega_0", "scale"))
    x = coords.astype(dt)
    if c["kind"] == "wire":
        y, cache = wo.wire_forward(p, x, er.LAYERS, *a, keep=True)
    else:
        y, cache = wo.realnet_forward(c["kind"], p, x, er.LAYERS, *a, None, keep=True)
    y = np.asarray(y).reshape(coords.shape[0], -1)
    rgb = rr.composite(y, ts, dl, bg, density)[0]
    loss, g_rgb = rr.mse_and_grad(rgb, tgt)
    gy = rr.composite_bwd(y, ts, dl, g_rgb, bg=bg, density=density).astype(dt)
    if c["kind"] == "wire":
        g = wo.wire_backward(p, cache, gy, er.LAYERS, *a)
    else:
        g = wo.realnet_backward(c["kind"], p, cache, gy, er.LAYERS, *a)
    return loss, g


@pytest.mark.parametrize("fam", ["x2", "x3"])
@pytest.mark.parametrize("net", ["siren", "wire_k90"])
def test_step_rays_one_step_matches_the_oracle(net, fam):
    """R = 96 rays x S = 48 jittered samples (4 608 rows) on the envelope tests' siren and wire nets, D = 3, O = 4, in both
    split-GEMM families: the loss and every parameter gradient within 2 x the fp32 oracle's own error + 1e-6."""
    from wire_amd.trainer import FusedTrainer
    R, S = 96, 48
    model = er.build(net, 3, 4, DEV)
    sd = er.state(model)
    rays = _rays(R, 51)
    rng = np.random.default_rng(52)
    near = rng.uniform(1.0, 1.5, R).astype(np.float32)
    far = (near + rng.uniform(1.5, 2.5, R)).astype(np.float32)
    u = rng.uniform(0, 1, (R, S)).astype(np.float32)
    tgt = rng.uniform(0, 1, (R, 3)).astype(np.float32)
    bg = np.float32([0.2, 0.5, 0.8])
    tr = FusedTrainer(model, (4, 4, 4), None, lr=0.0)
    with family_ctx(fam):
        loss = tr.step_rays(_dev(rays), _dev(tgt), _dev(near), _dev(far), S, jitter=_dev(u), background=bg)
        torch.cuda.synchronize()
    loss, flat = float(loss.item()), tr.flat_grad.cpu().numpy().astype(np.float64)
    coords, ts, dl = rr.ray_samples(rays, near, far, S, u)
    assert tr.coords[:R * S * 3].cpu().numpy().tobytes() == coords.tobytes()
    l64, g64 = _oracle_step(net, sd, coords, ts, dl, tgt, bg, "softplus", True)
    l32, g32 = _oracle_step(net, sd, coords, ts, dl, tgt, bg, "softplus", False)
    names =[k for k in model.state_dict().keys() if "omega_0" not in k and "scale_0" not in k]
    assert len(names) == len(tr.offsets) and np.abs(flat).max() > 0
    checks = [(f"step_rays {net} {fam} loss", abs(loss - l64) / l64, abs(l32 - l64) / l64)]
    for name, off in zip(names, tr.offsets):
        g = wo.as_real_pairs(g64[name]).astype(np.float64).ravel()
        r = wo.as_real_pairs(g32[name]).astype(np.float64).ravel()
        checks.append((f"step_rays {net} {fam} {name}", relmax(flat[off:off + g.size], g), relmax(r, g)))
    for lab, eb, e32 in checks:
        print(f"{lab}: err_build {eb:.3e}  err_ref {e32:.3e}  ratio {eb / e32 if e32 > 0 else float('inf'):.2f}")
    for lab, eb, e32 in checks:
        within_ref(eb, e32, lab)
    assert np.isfinite(tr.ray_rgb.cpu().numpy()).all()


# ---------------------------------------------------------------------------------------------------------------------
# a short trajectory on a tiny analytic scene, and render_rays
# ---------------------------------------------------------------------------------------------------------------------
SCENE_S, SCENE_N = 24, 12
HP = (30.0, 30.0, 10.0)


def _scene():
    """Two coloured Gaussian density blobs seen from 4 axis-aligned orthographic views at 12 x 12, rendered by the
    restatement at S = 24 midpoints: (rays [576, 6], near, far, target [576, 3])."""
    ax = np.linspace(-0.9, 0.9, SCENE_N)
    U, V = [a.reshape(-1) for a in np.meshgrid(ax, ax, indexing="ij")]
    one, zero = np.ones_like(U), np.zeros_like(U)
    views = [np.stack([-one, U, V, one, zero, zero], 1), np.stack([one, U, V, -one, zero, zero], 1),
             np.stack([U, -one, V, zero, one, zero], 1), np.stack([U, V, -one, zero, zero, one], 1)]
    rays = np.concatenate(views, 0).astype(np.float32)
    coords, ts, dl = rr.ray_samples(rays, np.float32(0.0), np.float32(2.0), SCENE_S)
    x = coords.astype(np.float64)
    mus, cols = np.array([[-0.35, -0.2, 0.1], [0.4, 0.3, -0.25]]), np.array([[0.9, 0.2, 0.1], [0.1, 0.3, 0.9]])
    dens = [6.0 * np.exp(-((x - m) ** 2).sum(1) / (2 * 0.3 ** 2)) for m in mus]
    sigma = dens[0] + dens[1]
    col = (dens[0][:, None] * cols[0] + dens[1][:, None] * cols[1] + 1e-9 * 0.5) / (sigma[:, None] + 1e-9)
    col = np.clip(col, 1e-6, 1 - 1e-6)
    y = np.concatenate([np.log(col / (1 - col)), sigma[:, None]], 1)
    target = rr.composite(y, ts, dl, None, "relu")[0].astype(np.float32)
    return rays, target


def _small_siren():
    from wire_amd.modules import models
    torch.manual_seed(0)
    return models.get_INR(nonlin="siren", in_features=3, out_features=4, hidden_features=64, hidden_layers=2,
                          first_omega_0=HP[0], hidden_omega_0=HP[1], scale=HP[2])


def _eager_loop(sd, rays, target, steps, lr, double):
    dt = torch.float64 if double else torch.float32
    p = er.tensors(sd, double, requires_grad=True)
    opt = torch.optim.Adam(list(p.values()), lr=lr)
    coords, ts, dl = rr.ray_samples(rays, np.float32(0.0), np.float32(2.0), SCENE_S)
    x, ts, dl, tgt = (torch.tensor(v).to(dt) for v in (coords, ts, dl, target))
    losses = []
    for _ in range(steps):
        opt.zero_grad()
        y = torch_ref.realnet_forward("siren", p, x, 2, *HP, None)
        loss = ((rr.torch_composite(y, ts, dl)[0] - tgt) ** 2).mean()
        loss.backward()
        opt.step()
        losses.append(float(loss.detach()))
    return np.array(losses)


def test_step_rays_trajectory_follows_the_fp64_loop():
    """30 steps of step_rays on the blob scene (576 rays x 24 midpoints, siren 2 x 64, Adam 1e-3): the loss sequence stays
    with the fp64 eager loop by tests/test_gpu_psnr_gate.py's rule -- drift <= 4 x the fp32 eager loop's drift + 2e-5 --
    and the loss falls."""
    from wire_amd.trainer import FusedTrainer
    rays, target = _scene()
    model = _small_siren()
    sd = er.state(model)
    steps, lr = 30, 1e-3
    l64 = _eager_loop(sd, rays, target, steps, lr, True)
    l32 = _eager_loop(sd, rays, target, steps, lr, False)
    tr = FusedTrainer(model.to(DEV), (4, 4, 4), None, lr=lr)
    r, t = _dev(rays), _dev(target)
    losses = [tr.step_rays(r, t, 0.0, 2.0, SCENE_S) for _ in range(steps)]
    torch.cuda.synchronize()
    losses = np.array([float(v.item()) for v in losses])
    drift, drift_ref = np.abs(losses - l64) / l64, np.abs(l32 - l64) / l64
    print(f"step_rays trajectory: loss {losses[0]:.5e} -> {losses[-1]:.5e} (fp64 {l64[0]:.5e} -> {l64[-1]:.5e}); "
          f"drift vs fp64: build max {drift.max():.2e}, fp32 eager max {drift_ref.max():.2e}")
    assert np.isfinite(losses).all()
    assert drift.max() <= 4 * drift_ref.max() + 2e-5
    assert losses[-1] < losses[0]


def test_render_rays_is_composite_fwd_and_does_not_depend_on_the_tiling():
    from wire_amd import _lib
    from wire_amd.trainer import FusedTrainer
    model = _small_siren().to(DEV)
    tr = FusedTrainer(model, (4, 4, 4), None, lr=0.0)
    R, S = 40, 16
    rays = _rays(R, 61)
    rng = np.random.default_rng(62)
    near = rng.uniform(1.0, 1.5, R).astype(np.float32)
    far = (near + rng.uniform(1.5, 2.5, R)).astype(np.float32)
    bg = np.float32([0.3, 0.1, 0.6])
    r, nr, fr = _dev(rays), _dev(near), _dev(far)
    one = _np(*tr.render_rays(r, nr, fr, S, tile_rays=R, background=bg, density="relu"))
    assert [v.shape for v in one] == [(R, 3), (R,), (R,)] and all(np.isfinite(v).all() for v in one)
    # the same through the ABI: the sampler, the net's forward on the trainer's packed parameters, wire_composite_fwd
    L, d = _lib.lib(), C.byref(tr.desc)
    coords, ts, dl = rr.ray_samples(rays, near, far, S)
    x = _dev(coords)
    ab = _lib.check(L.wire_act_bytes(d, R * S, 0))
    act = torch.empty(ab, dtype=torch.uint8, device=DEV)
    y = _full(R * S, 4)
    _call("wire_mlp_fwd", d, tr.packed.data_ptr(), x.data_ptr(), R * S, y.data_ptr(), act.data_ptr(), ab, 0)
    torch.cuda.synchronize()
    want = _np(*Dev(y.cpu().numpy(), ts, dl, bg, "relu").fwd())
    for u, v in zip(one, want):
        assert u.tobytes() == v.tobytes()
    for tile in (7, 16, 10 ** 6):                                           # (all below the 4 096-row family switch)
        for u, v in zip(one, _np(*tr.render_rays(r, nr, fr, S, tile_rays=tile, background=bg, density="relu"))):
            assert u.tobytes() == v.tobytes(), tile
    # scalar bounds
    a = _np(*tr.render_rays(r, 1.2, 3.4, S, tile_rays=9))
    b = _np(*tr.render_rays(r, 1.2, 3.4, S))
    assert all(u.tobytes() == v.tobytes() for u, v in zip(a, b))
