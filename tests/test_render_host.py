"""Host checks of the volume-rendering operator (no GPU): the fp64 restatement tests/render_ref.py against closed forms
and against torch's fp64 autograd, the C ABI's symbols and argument checks (every WIRE_ERR_ARG case returns before the
first HIP call, so fake pointers and a NULL stream serve), the Python surface's refusals, and the ray helpers of
``utils`` against hand-computed values."""
import numpy as np
import pytest
import torch

import render_ref as rr


# ---------------------------------------------------------------------------------------------------------------------
# the restatement against itself
# ---------------------------------------------------------------------------------------------------------------------
def _logit(p):
    return np.log(p / (1.0 - p))


@pytest.mark.parametrize("bg", [None, (0.2, 0.9, 0.4)])
def test_constant_density_slab(bg):
    """sigma constant over a length L: T = exp(-sigma L), rgb = (1 - T) c + T bg, whatever the sampling."""
    S, sigma, col = 37, 1.7, np.array([0.3, 0.6, 0.8])
    rays = np.array([[0, 0, -1, 0, 0, 2.0], [0.1, 0, -1, 0, 0, 0.5]], np.float32)       # |d| = 2 and 0.5
    u = np.random.default_rng(0).uniform(0, 1, (2, S)).astype(np.float32)
    _, ts, deltas = rr.ray_samples(rays, np.float32(0.25), np.float32(1.0), S, u)
    # t_0 > near with jitter: the slab the samples cover starts at t_0
    Ls = deltas.astype(np.float64).sum(axis=1)
    np.testing.assert_allclose(Ls, (1.0 - ts[:, 0].astype(np.float64)) * np.array([2.0, 0.5]), rtol=1e-6)
    y = np.empty((2, S, 4))
    y[..., :3], y[..., 3] = _logit(col), sigma
    rgb, acc, depth = rr.composite(y, ts, deltas, bg, "relu")
    T = np.exp(-sigma * Ls)
    want = (1 - T)[:, None] * col + (T[:, None] * np.asarray(bg) if bg is not None else 0.0)
    np.testing.assert_allclose(rgb, want, rtol=1e-12, atol=1e-14)
    np.testing.assert_allclose(acc, 1 - T, rtol=1e-12)
    assert np.all(depth > ts[:, 0] * acc * 0.999) and np.all(depth < ts[:, -1] * acc * 1.001)


def _case(R, S, C, seed):
    rng = np.random.default_rng(seed)
    y = rng.normal(0, 1.5, (R * S, C + 1))
    ts = np.sort(rng.uniform(0.5, 3.0, (R, S)), axis=1).astype(np.float32)
    deltas = rng.uniform(0.0, 0.4, (R, S)).astype(np.float32)
    return y, ts, deltas, rng


@pytest.mark.parametrize("density", ["softplus", "relu"])
@pytest.mark.parametrize("with_bg", [False, True])
def test_closed_form_backward_is_autograd_of_the_cumsum_form(density, with_bg):
    """The adjoint of render_ref (q_bg = <bg, g_rgb> - g_acc; g_acc nowhere else) against torch fp64 autograd of the
    cumsum / cumprod form, with g_rgb, g_acc and g_depth all nonzero."""
    R, S, C = 5, 11, 3
    y, ts, deltas, rng = _case(R, S, C, 3)
    bg = rng.uniform(0, 1, C) if with_bg else None
    g_rgb, g_acc, g_depth = rng.normal(size=(R, C)), rng.normal(size=R), rng.normal(size=R)
    yt = torch.tensor(y, requires_grad=True)
    rgb, acc, depth = rr.torch_composite(yt, torch.tensor(ts, dtype=torch.float64),
                                         torch.tensor(deltas, dtype=torch.float64),
                                         None if bg is None else torch.tensor(bg), density)
    f = (rgb * torch.tensor(g_rgb)).sum() + (acc * torch.tensor(g_acc)).sum() + (depth * torch.tensor(g_depth)).sum()
    f.backward()
    r2, a2, d2 = rr.composite(y, ts, deltas, bg, density)
    np.testing.assert_allclose(r2, rgb.detach().numpy(), rtol=1e-12, atol=1e-14)
    np.testing.assert_allclose(a2, acc.detach().numpy(), rtol=1e-12, atol=1e-14)
    np.testing.assert_allclose(d2, depth.detach().numpy(), rtol=1e-12, atol=1e-14)
    g = rr.composite_bwd(y, ts, deltas, g_rgb, g_acc, g_depth, bg, density)
    want = yt.grad.numpy()
    assert np.abs(g - want).max() <= 1e-12 * np.abs(want).max()
    # each optional gradient alone, too (the sign of g_acc in q_bg)
    for ga, gd in ((g_acc, None), (None, g_depth)):
        yt.grad = None
        rgb, acc, depth = rr.torch_composite(yt, torch.tensor(ts, dtype=torch.float64),
                                             torch.tensor(deltas, dtype=torch.float64),
                                             None if bg is None else torch.tensor(bg), density)
        ((acc * torch.tensor(ga)).sum() if ga is not None else (depth * torch.tensor(gd)).sum()).backward()
        g = rr.composite_bwd(y, ts, deltas, np.zeros((R, C)), ga, gd, bg, density)
        assert np.abs(g - yt.grad.numpy()).max() <= 1e-12 * np.abs(yt.grad.numpy()).max()


def test_missing_ray_gives_background_and_zero_gradient():
    rays = np.array([[0, 0, -3, 0, 0, 1.0], [0, 0, -3, 0, 0, 1.0]], np.float32)
    near, far = np.array([2.0, 2.5], np.float32), np.array([4.0, 2.5], np.float32)       # ray 1: far <= near
    coords, ts, deltas = rr.ray_samples(rays, near, far, 6)
    assert np.all(deltas[1] == 0) and np.all(ts[1] == np.float32(2.5)) and np.all(deltas[0] > 0)
    np.testing.assert_array_equal(coords.reshape(2, 6, 3)[1], np.tile(np.float32([0, 0, -0.5]), (6, 1)))
    y = np.random.default_rng(1).normal(size=(12, 4))
    bg = np.array([0.1, 0.5, 0.7])
    rgb, acc, depth = rr.composite(y, ts, deltas, bg)
    assert np.array_equal(rgb[1], bg) and acc[1] == 0 and depth[1] == 0 and acc[0] > 0
    g = rr.composite_bwd(y, ts, deltas, np.ones((2, 3)), np.ones(2), np.ones(2), bg).reshape(2, 6, 4)
    assert np.all(g[1] == 0) and np.abs(g[0]).min() > 0


def test_sampler_midpoints_and_last_delta():
    rays = np.array([[1, 2, 3, 0, 3, 4.0]], np.float32)                                 # |d| = 5
    coords, ts, deltas = rr.ray_samples(rays, 1.0, 3.0, 4)
    np.testing.assert_array_equal(ts[0], np.float32([1.25, 1.75, 2.25, 2.75]))
    np.testing.assert_array_equal(deltas[0], np.float32([2.5, 2.5, 2.5, 1.25]))         # the last one runs to far
    np.testing.assert_array_equal(coords[0], np.float32([1, 2 + 3 * 1.25, 3 + 4 * 1.25]))
    assert coords.dtype == ts.dtype == deltas.dtype == np.float32 and coords.shape == (4, 3)


# ---------------------------------------------------------------------------------------------------------------------
# the C ABI
# ---------------------------------------------------------------------------------------------------------------------
NAMES = ["wire_ray_samples", "wire_composite_fwd", "wire_composite_bwd", "wire_composite_mse_grad"]
P = 0x10000            # a fake, 16-byte aligned device pointer: the checks below return before anything reads it
ARG = -1


def test_symbols_declared_and_exported():
    from wire_amd import _lib
    lib = _lib.lib()
    for n in NAMES:
        assert n in _lib.SYMBOLS and hasattr(lib, n)
    assert lib.wire_abi_version() == 1 and _lib.DENSITY_MODE == {"softplus": 0, "relu": 1}


def _samples(lib, **kw):
    a = dict(rays=P, bounds=None, near=0.0, far=1.0, jitter=None, R=4, S=8, coords=P, ts=P, deltas=P)
    a.update(kw)
    return lib.wire_ray_samples(None, a["rays"], a["bounds"], a["near"], a["far"], a["jitter"], a["R"], a["S"],
                                a["coords"], a["ts"], a["deltas"])


def _fwd(lib, **kw):
    a = dict(y=P, ts=P, deltas=P, bg=None, R=4, S=8, O=4, density=0, rgb=P, acc=None, depth=None)
    a.update(kw)
    return lib.wire_composite_fwd(None, a["y"], a["ts"], a["deltas"], a["bg"], a["R"], a["S"], a["O"], a["density"],
                                  a["rgb"], a["acc"], a["depth"])


def _bwd(lib, **kw):
    a = dict(y=P, ts=P, deltas=P, bg=None, g_rgb=P, g_acc=None, g_depth=None, R=4, S=8, O=4, density=0, g_y=P)
    a.update(kw)
    return lib.wire_composite_bwd(None, a["y"], a["ts"], a["deltas"], a["bg"], a["g_rgb"], a["g_acc"], a["g_depth"],
                                  a["R"], a["S"], a["O"], a["density"], a["g_y"])


def _mse(lib, **kw):
    a = dict(y=P, ts=P, deltas=P, bg=None, target=P, R=4, S=8, O=4, density=0, shard=1.0, g_y=P, loss=P, rgb=None,
             partial=P)
    a.update(kw)
    return lib.wire_composite_mse_grad(None, a["y"], a["ts"], a["deltas"], a["bg"], a["target"], a["R"], a["S"], a["O"],
                                       a["density"], a["shard"], a["g_y"], a["loss"], a["rgb"], a["partial"])


BIG_R = 4 * (2 ** 31 - 1) + 1       # one ray more than 2^31 - 1 workgroups of 4 rays hold
COMMON = [dict(R=0), dict(R=-3), dict(S=0), dict(S=-1), dict(R=2 ** 62, S=2 ** 20), dict(R=BIG_R, S=1),
          dict(ts=None), dict(deltas=None), dict(ts=P + 2), dict(deltas=P + 1)]
COMPOSITE = COMMON + [dict(O=1), dict(O=9), dict(O=0), dict(density=2), dict(density=-1), dict(y=None), dict(y=P + 8),
                      dict(y=P + 4), dict(bg=P + 2)]


@pytest.mark.parametrize("bad", COMMON + [dict(rays=None), dict(coords=None), dict(rays=P + 1), dict(coords=P + 2),
                                          dict(bounds=P + 3), dict(jitter=P + 1), dict(near=float("nan")),
                                          dict(far=float("inf")), dict(R=2 ** 31 * 256, S=1)],
                         ids=lambda d: ",".join(f"{k}={v}" for k, v in d.items()))
def test_ray_samples_refuses(bad):
    from wire_amd import _lib
    lib = _lib.lib()
    assert _samples(lib, **bad) == ARG
    assert b"wire_ray_samples" in lib.wire_last_error()


@pytest.mark.parametrize("bad", COMPOSITE + [dict(rgb=None), dict(rgb=P + 1), dict(acc=P + 2), dict(depth=P + 3)],
                         ids=lambda d: ",".join(f"{k}={v}" for k, v in d.items()))
def test_composite_fwd_refuses(bad):
    from wire_amd import _lib
    lib = _lib.lib()
    assert _fwd(lib, **bad) == ARG
    assert b"wire_composite_fwd" in lib.wire_last_error()


@pytest.mark.parametrize("bad", COMPOSITE + [dict(g_rgb=None), dict(g_y=None), dict(g_y=P + 8), dict(g_rgb=P + 2),
                                             dict(g_acc=P + 1), dict(g_depth=P + 2)],
                         ids=lambda d: ",".join(f"{k}={v}" for k, v in d.items()))
def test_composite_bwd_refuses(bad):
    from wire_amd import _lib
    lib = _lib.lib()
    assert _bwd(lib, **bad) == ARG
    assert b"wire_composite_bwd" in lib.wire_last_error()


@pytest.mark.parametrize("bad", COMPOSITE + [dict(target=None), dict(g_y=None), dict(loss=None), dict(partial=None),
                                             dict(g_y=P + 4), dict(target=P + 1), dict(rgb=P + 2), dict(partial=P + 2),
                                             dict(shard=float("inf")), dict(shard=float("nan"))],
                         ids=lambda d: ",".join(f"{k}={v}" for k, v in d.items()))
def test_composite_mse_grad_refuses(bad):
    from wire_amd import _lib
    lib = _lib.lib()
    assert _mse(lib, **bad) == ARG
    assert b"wire_composite_mse_grad" in lib.wire_last_error()


def test_no_workspace_query_is_declared():
    """The kernels need no scratch beyond ``partial`` (2048 floats, inside the trainer's 4096), so the ABI has no
    wire_composite_ws_bytes; the header and SYMBOLS agree on that."""
    from wire_amd import _lib
    assert not any("composite_ws" in s for s in _lib.SYMBOLS)
    assert not hasattr(_lib.lib(), "wire_composite_ws_bytes")


# ---------------------------------------------------------------------------------------------------------------------
# the Python surface
# ---------------------------------------------------------------------------------------------------------------------
def test_functional_refusals_on_the_host():
    from wire_amd import _lib, functional
    rays = torch.zeros(5, 6)
    with pytest.raises(_lib.WireHipError):
        functional.ray_samples(rays, 0.0, 1.0, 4)
    with pytest.raises(_lib.WireHipError):
        functional.ray_samples(rays, torch.zeros(5), torch.ones(5), 4, jitter=torch.zeros(5, 4))
    for bad in (dict(rays=torch.zeros(5, 5)), dict(rays=torch.zeros(5, 6, dtype=torch.float64)),
                dict(rays=torch.zeros(0, 6)), dict(rays=torch.zeros(6, 5).t()), dict(n_samples=0),
                dict(near=torch.zeros(5)), dict(near=torch.zeros(4), far=torch.ones(4)),
                dict(near=torch.zeros(5, dtype=torch.float64), far=torch.ones(5)), dict(far=float("inf")),
                dict(jitter=torch.zeros(5, 3)), dict(jitter=torch.zeros(5, 4, dtype=torch.float64))):
        a = dict(rays=rays, near=0.0, far=1.0, n_samples=4, jitter=None)
        a.update(bad)
        with pytest.raises(ValueError):
            functional.ray_samples(a["rays"], a["near"], a["far"], a["n_samples"], a["jitter"])
    R, S = 3, 4
    y, ts, dl = torch.zeros(R * S, 4), torch.zeros(R, S), torch.zeros(R, S)
    with pytest.raises(_lib.WireHipError):
        functional.composite(y, ts, dl)
    with pytest.raises(_lib.WireHipError):
        functional.composite(y.reshape(R, S, 4), ts, dl, background=[0.1, 0.2, 0.3], density="relu")
    for bad in (dict(y=torch.zeros(R * S, 1)), dict(y=torch.zeros(R * S, 9)), dict(y=torch.zeros(R * S + 1, 4)),
                dict(y=y.double()), dict(ts=torch.zeros(R, S + 1)), dict(dl=torch.zeros(R, S, dtype=torch.float64)),
                dict(ts=torch.zeros(R * S)), dict(bg=[0.1, 0.2]), dict(bg=torch.zeros(4)), dict(density="exp"),
                dict(density=0)):
        a = dict(y=y, ts=ts, dl=dl, bg=None, density="softplus")
        a.update(bad)
        with pytest.raises(ValueError):
            functional.composite(a["y"], a["ts"], a["dl"], a["bg"], a["density"])
    with pytest.raises(NotImplementedError):
        functional.composite(y, ts, dl.clone().requires_grad_(True))
    with pytest.raises(NotImplementedError):
        functional.composite(y, ts.clone().requires_grad_(True), dl)


# ---------------------------------------------------------------------------------------------------------------------
# utils.get_rays / utils.ray_box
# ---------------------------------------------------------------------------------------------------------------------
def test_get_rays_hand_values():
    from wire_amd.modules import utils
    # identity pose at (0, 0, 4): 2 x 4 pixels, focal 2
    c2w = torch.tensor([[1.0, 0, 0, 0], [0, 1, 0, 0], [0, 0, 1, 4]])
    rays = utils.get_rays(2, 4, 2.0, c2w)
    assert rays.shape == (8, 6) and rays.dtype == torch.float32 and rays.is_contiguous()
    assert torch.equal(rays[:, :3], torch.tensor([0.0, 0, 4]).expand(8, 3))
    want = [[(j - 2) / 2, -(i - 1) / 2, -1.0] for i in range(2) for j in range(4)]
    assert torch.equal(rays[:, 3:], torch.tensor(want))
    # a pose that turns the camera to look along +x: camera -z -> world +x, camera x -> world z
    c2w = np.array([[0.0, 0, -1, -3], [0, 1, 0, 0.5], [1, 0, 0, 0], [0, 0, 0, 1]])
    rays = utils.get_rays(1, 2, 1.0, c2w)
    assert torch.equal(rays, torch.tensor([[-3.0, 0.5, 0, 1, 0.5, -1], [-3.0, 0.5, 0, 1, 0.5, 0]]))
    with pytest.raises(ValueError):
        utils.get_rays(2, 2, 1.0, torch.zeros(3, 3))


def test_ray_box_hand_values():
    from wire_amd.modules import utils
    rays = torch.tensor([[-3.0, 0, 0, 1, 0, 0],          # along +x through the centre: [2, 4]
                         [-3.0, 0, 0, 2, 0, 0],          # the same line, |d| = 2: [1, 2]
                         [0.0, 0, 0, 0, 0, 1],           # from inside: [0, 1]
                         [-3.0, 2, 0, 1, 0, 0],          # parallel to the slab, outside it: a miss
                         [-3.0, 0, 0, -1, 0, 0],         # looking away: a miss
                         [-2.0, -2, 0, 1, 1, 0],         # the diagonal of the z = 0 square: [1, 3]
                         [-3.0, 0, 0, 1, 1, 0]])         # enters x at t = 2 where y = 2 already: a miss
    near, far = utils.ray_box(rays)
    assert near.shape == far.shape == (7,) and near.dtype == torch.float32
    hit = [0, 1, 2, 5]
    assert torch.equal(near[hit], torch.tensor([2.0, 1, 0, 1])) and torch.equal(far[hit], torch.tensor([4.0, 2, 1, 3]))
    for m in (3, 4, 6):
        assert far[m] <= near[m] and torch.isfinite(near[m]) and torch.isfinite(far[m])
    near, far = utils.ray_box(rays[:1], lo=-2.0, hi=0.5)
    assert float(near) == 1.0 and float(far) == 3.5
