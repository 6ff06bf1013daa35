"""Hierarchical ray sampling on the MI355X (wire_composite_weights and wire_ray_resample in wire_amd/csrc/wire_render.hip,
DESIGN section 33): the weights against the fp64 restatement within eager fp32's own error and against the forward
kernel's acc; the resampler against tests/resample_ref.py within bounds derived from the formats (one fp32 ulp of the
output plus the fp64 conditioning of the inverse CDF), its exact properties (sorted, coarse values kept, inside the
bounds, the lattice count per bin), the value edges, completeness and determinism; then ``step_rays(n_importance=...)``
in two halves (positions against the restatement fed the device's own weights; loss and gradients against the oracle fed
the device's positions), a short trajectory against eager loops that resample through the restatement, and
``render_rays(n_importance=...)``."""
import ctypes as C

import numpy as np
import pytest
import torch

import envelope_ref as er
import render_ref as rr
import resample_ref as rs
from _util import RATIO_LOG, family_ctx, relmax, within_ref
from oracle import torch_ref
from oracle import wire_oracle as wo
from test_gpu_render import HP, MODE, _oracle_step, _rays, _scene, _small_siren

pytestmark = pytest.mark.gpu
DEV = "cuda"
RPW = 4                          # rays per workgroup of the weights kernel and of the resampler up to S, Nf = 256
NAN = float("nan")


def _dev(a, dt=torch.float32):
    return None if a is None else torch.as_tensor(np.ascontiguousarray(a)).to(DEV, dt).contiguous()


def _ptr(t):
    return None if t is None else t.data_ptr()


def _call(name, *args):
    from wire_amd import _lib
    _lib.check(getattr(_lib.lib(), name)(torch.cuda.current_stream().cuda_stream, *args), name)


def _full(*shape, fill=NAN):
    return torch.full(shape, fill, dtype=torch.float32, device=DEV)


def _np(*ts):
    torch.cuda.synchronize()
    return [t.cpu().numpy() for t in ts]


def abi_weights(y, dl, density, fill=NAN):
    R, S = dl.shape
    yd, dd, w = _dev(y), _dev(dl), _full(R, S, fill=fill)
    _call("wire_composite_weights", yd.data_ptr(), dd.data_ptr(), R, S, y.shape[-1], MODE[density], w.data_ptr())
    return _np(w)[0]


def abi_resample(rays, near, far, tc, w, Nf, jitter=None, eps=1e-5, fill=NAN):
    R, S = tc.shape
    M = S + Nf
    r, t, ww, v = _dev(rays), _dev(tc), _dev(w), _dev(jitter)
    bounds = None if np.ndim(near) == 0 else _dev(np.stack([near, far], 1))
    coords, ts, dl = _full(R * M, 3, fill=fill), _full(R, M, fill=fill), _full(R, M, fill=fill)
    _call("wire_ray_resample", r.data_ptr(), _ptr(bounds), 0.0 if bounds is not None else float(near),
          0.0 if bounds is not None else float(far), t.data_ptr(), ww.data_ptr(), _ptr(v), float(eps), R, S, Nf,
          coords.data_ptr(), ts.data_ptr(), dl.data_ptr())
    return _np(coords, ts, dl)


# ---------------------------------------------------------------------------------------------------------------------
# wire_composite_weights
# ---------------------------------------------------------------------------------------------------------------------
def _inputs(R, S, C, seed):
    """test_gpu_render._inputs' recipe."""
    rng = np.random.default_rng(seed)
    y = rng.normal(0, 1.5, (R * S, C + 1)).astype(np.float32)
    y[:, -1] += np.float32(0.5)
    ts = np.sort(rng.uniform(0.5, 3.0, (R, S)), axis=1).astype(np.float32)
    dl = rng.uniform(0.0, 6.0 / S, (R, S)).astype(np.float32)
    return y, ts, dl


def _eager32_w(y, dl, density):
    """The weights of the cumprod form in eager fp32 torch on the host."""
    R, S = dl.shape
    s_raw = torch.tensor(y).reshape(R, S, -1)[..., -1]
    sigma = torch.nn.functional.softplus(s_raw) if density == "softplus" else torch.relu(s_raw)
    alpha = 1.0 - torch.exp(-sigma * torch.tensor(dl))
    T = torch.cumprod(torch.cat([torch.ones_like(alpha[:, :1]), 1.0 - alpha], dim=1), dim=1)
    return (T[:, :-1] * alpha).numpy()


@pytest.mark.parametrize("S", [1, 2, 63, 64, 65, 130])
@pytest.mark.parametrize("O", [2, 4, 5, 8])
def test_weights_against_fp64_and_the_forward_kernel(O, S):
    """Both density modes, R one fewer than, equal to and one more than the rays of a workgroup: w against the
    restatement within eager fp32's error (the protocol rgb and acc pass; w is their summand), every element written
    (NaN prefill), and sum_s w_s against the forward kernel's acc within (S + 1) 2^-24."""
    for density in ("softplus", "relu"):
        for R in (RPW - 1, RPW, RPW + 1):
            y, ts, dl = _inputs(R, S, O - 1, 7 * S + O + R)
            got = abi_weights(y, dl, density)
            assert got.shape == (R, S) and np.isfinite(got).all(), (density, R)
            want = rr._weights(y, ts, dl, density)[5]
            within_ref(relmax(got, want), relmax(_eager32_w(y, dl, density), want),
                       f"composite_weights O={O} S={S} R={R} {density}")
            rgb, acc = _full(R, O - 1), _full(R)
            yd, td, dd = _dev(y), _dev(ts), _dev(dl)
            _call("wire_composite_fwd", yd.data_ptr(), td.data_ptr(), dd.data_ptr(), None, R, S, O, MODE[density],
                  rgb.data_ptr(), acc.data_ptr(), None)
            acc, = _np(acc)
            err = np.abs(got.astype(np.float64).sum(axis=1) - acc.astype(np.float64)).max()
            RATIO_LOG.append((f"sum w vs acc O={O} S={S} R={R} {density} [err / ((S+1) 2^-24)]", float(err),
                              (S + 1) * 2.0 ** -24))
            assert err <= (S + 1) * 2.0 ** -24


def test_weights_repeat_their_bits_whatever_the_output_held():
    y, ts, dl = _inputs(9, 130, 3, 5)
    a, b = abi_weights(y, dl, "softplus"), abi_weights(y, dl, "softplus", fill=7.0)
    assert not np.isnan(a).any() and a.tobytes() == b.tobytes()


# ---------------------------------------------------------------------------------------------------------------------
# wire_ray_resample: parity with the restatement
# ---------------------------------------------------------------------------------------------------------------------
def _case(R, S, Nf, seed, per_ray, jitter, span=(1.0, 3.0)):
    rng = np.random.default_rng(seed)
    rays = np.concatenate([rng.uniform(-2, 2, (R, 3)), rng.normal(0, 1, (R, 3))], 1).astype(np.float32)
    if per_ray:
        near = rng.uniform(0.1, 1.0, R).astype(np.float32)
        far = (near + rng.uniform(*span, R)).astype(np.float32)
    else:
        near, far = np.float32(0.3), np.float32(2.7)
    uc = rng.uniform(0.1, 0.9, (R, S)).astype(np.float32)
    _, tc, _ = rr.ray_samples(rays, near, far, S, uc)
    w = (rng.uniform(0, 1, (R, S)) ** 8).astype(np.float32)
    if R > 1:
        w[1] = 0.0                                         # an all-zero row: eps alone is the mass
    if R > 2:
        w[2] = 0.0
        w[2, S // 2] = 0.8                                 # a single nonzero weight
    v = rng.uniform(0, 1, (R, Nf)).astype(np.float32) if jitter else None
    return rays, near, far, tc, w, v


def _check_parity(got, want, rays, near, far, w, label, eps=1e-5):
    """|ts - ref| <= ulp(max(|near|, |far|)) + kappa, |deltas - ref| <= ulp(ref) + 2 kappa |d|,
    |coords - ref| <= ulp(max |coord|) + kappa max |d_i|, kappa = 8 S 2^-52 (tot / eps) (far - near) per ray."""
    R = rays.shape[0]
    M = got[1].shape[1]
    k = rs.kappa(w, near, far, eps)[:, None]
    d = rays[:, 3:].astype(np.float64)
    g = [a.astype(np.float64) for a in got]
    x = [a.astype(np.float64) for a in want]
    top = np.maximum(np.abs(np.broadcast_to(near, (R,))), np.abs(np.broadcast_to(far, (R,))))
    b_ts = rs.ulp32(top)[:, None] + k
    b_dl = rs.ulp32(want[2]) + 2 * k * np.linalg.norm(d, axis=1)[:, None]
    cmax = np.abs(x[0]).reshape(R, M * 3).max(axis=1)
    b_co = (rs.ulp32(cmax)[:, None] + k * np.abs(d).max(axis=1)[:, None])
    ratios = [(np.abs(g[1] - x[1]) / b_ts).max(), (np.abs(g[2] - x[2]) / b_dl).max(),
              (np.abs(g[0] - x[0]).reshape(R, M * 3) / b_co).max()]
    for name, q in zip(("ts", "deltas", "coords"), ratios):
        RATIO_LOG.append((f"ray_resample {label} {name} [err / derived bound]", float(q), 1.0))
        print(f"ray_resample {label} {name}: err / bound {q:.3f}")
    for name, q in zip(("ts", "deltas", "coords"), ratios):
        assert q <= 1.0, f"ray_resample {label} {name}: err / bound = {q:.3f}"


# every R of {1, 3, 4, 5, 9}, every S of {1, 2, 63, 64, 65, 130, 1024}, every Nf of {1, 2, 64, 65, 128, 1024}, and the
# sizes either side of the switch between the two editions of the kernel (S, Nf <= 256: four rays per workgroup)
PARITY = [(1, 1, 1), (3, 2, 2), (4, 63, 64), (5, 64, 65), (9, 65, 128), (3, 130, 1), (4, 1024, 2), (5, 1, 1024),
          (9, 1024, 1024), (5, 256, 256), (5, 257, 64), (3, 64, 257), (9, 130, 128)]


@pytest.mark.parametrize("R,S,Nf", PARITY)
def test_resampler_against_the_restatement(R, S, Nf):
    for per_ray in (False, True):
        for jitter in (False, True):
            rays, near, far, tc, w, v = _case(R, S, Nf, 100 * R + 7 * S + Nf, per_ray, jitter)
            got = abi_resample(rays, near, far, tc, w, Nf, v)
            for a in got:
                assert np.isfinite(a).all()
            want = rs.ray_resample(rays, near, far, tc, w, Nf, v)
            _check_parity(got, want, rays, near, far, w, f"R={R} S={S} Nf={Nf} bounds={int(per_ray)} jit={int(jitter)}")


# ---------------------------------------------------------------------------------------------------------------------
# wire_ray_resample: exact properties of the device output
# ---------------------------------------------------------------------------------------------------------------------
def _bits(a):
    return np.ascontiguousarray(a, np.float32).view(np.uint32)


def _check_exact(ts, dl, tc, near, far):
    R = tc.shape[0]
    nr, fr = np.broadcast_to(near, (R,))[:, None], np.broadcast_to(far, (R,))[:, None]
    assert np.all(np.diff(ts, axis=1) >= 0), "ts not sorted"
    assert np.all(ts >= nr) and np.all(ts <= fr), "ts outside [near, far]"
    assert np.all(dl >= 0), "a negative delta"
    for r in range(R):
        vals, counts = np.unique(tc[r], return_counts=True)
        have = dict(zip(*np.unique(_bits(ts[r]), return_counts=True)))
        for val, n in zip(_bits(vals), counts):
            assert have.get(val, 0) >= n, "a coarse sample is missing"


@pytest.mark.parametrize("R,S,Nf", PARITY)
def test_resampler_output_is_sorted_keeps_the_coarse_samples_and_stays_inside(R, S, Nf):
    for per_ray, jitter in ((False, True), (True, False)):
        rays, near, far, tc, w, v = _case(R, S, Nf, 55 * R + 3 * S + Nf, per_ray, jitter)
        _, ts, dl = abi_resample(rays, near, far, tc, w, Nf, v)
        _check_exact(ts, dl, tc, near, far)


@pytest.mark.parametrize("S,Nf", [(1, 64), (2, 65), (65, 128), (130, 1024), (64, 2), (130, 257)])
def test_resampler_lattice_count_per_bin(S, Nf):
    """v = 0.5: bin s holds floor(Nf p_s / tot) or ceil(Nf p_s / tot) draws.  Counted on the fp32 output: the merged
    samples inside the bin widened by one fp32 ulp, less its own coarse sample, are at least the floor, and inside the
    bin narrowed by one ulp at most the ceiling.  The bins are >= 1e-3 wide (span >= 1, jitter in [0.1, 0.9], S <= 130),
    a thousand ulps, and a coarse sample is as far from its bin's edges."""
    R = 5
    rays, near, far, tc, w, _ = _case(R, S, Nf, 13 * S + Nf, True, False)
    _, ts, _ = abi_resample(rays, near, far, tc, w, Nf, None)
    e = rs.edges(near, far, tc)
    assert np.diff(e, axis=1).min() >= 1e-3
    p, c = rs.mass(w)
    ulp = rs.ulp32(np.maximum(np.abs(near), np.abs(far)))
    t = ts.astype(np.float64)
    for r in range(R):
        share = Nf * p[r] / c[r, -1]
        wide = np.array([np.sum((t[r] >= e[r, s] - ulp[r]) & (t[r] <= e[r, s + 1] + ulp[r])) for s in range(S)]) - 1
        tight = np.array([np.sum((t[r] > e[r, s] + ulp[r]) & (t[r] < e[r, s + 1] - ulp[r])) for s in range(S)]) - 1
        assert np.all(wide >= np.floor(share - 1e-9)) and np.all(tight <= np.ceil(share + 1e-9)), r


# ---------------------------------------------------------------------------------------------------------------------
# wire_ray_resample: edges and hygiene
# ---------------------------------------------------------------------------------------------------------------------
def test_missing_rays_and_nan_bounds_stay_at_near():
    R, S, Nf = 6, 65, 70
    rays, near, far, tc, w, v = _case(R, S, Nf, 3, True, True)
    far[1] = near[1] - np.float32(0.25)
    far[3] = near[3]
    far[4] = np.float32(NAN)
    coords, ts, dl = abi_resample(rays, near, far, tc, w, Nf, v)
    want = rs.ray_resample(rays, near, far, tc, w, Nf, v)
    for r in (1, 3, 4):
        assert np.all(ts[r] == near[r]) and np.all(dl[r] == 0)
    assert np.isfinite(coords).all() and np.isfinite(ts).all() and np.isfinite(dl).all()
    assert coords.reshape(R, -1)[[1, 3, 4]].tobytes() == want[0].reshape(R, -1)[[1, 3, 4]].tobytes()
    ok = [0, 2, 5]
    _check_exact(ts[ok], dl[ok], tc[ok], near[ok], far[ok])


def test_hostile_weights_give_finite_sorted_output():
    R, S, Nf = 8, 70, 130
    rays, near, far, tc, w, v = _case(R, S, Nf, 4, True, True)
    w[0, ::3] = NAN
    w[1, 5] = np.inf
    w[2] = -1.0
    w[3, ::2] = np.float32(1e30)                            # eps vanishes beside it: bins of no mass at all
    w[4] = np.inf
    w[5] = NAN
    w[6, 7], w[6, 8] = np.float32(1e30), np.float32(-1e30)
    for jit in (None, v):
        coords, ts, dl = abi_resample(rays, near, far, tc, w, Nf, jit)
        assert np.isfinite(coords).all() and np.isfinite(ts).all() and np.isfinite(dl).all()
        _check_exact(ts, dl, tc, near, far)


def test_unsorted_coarse_samples_give_finite_output():
    """The ABI does not check that ts_c is sorted: shuffled rows give meaningless values, but every element is written
    (NaN prefill) and finite."""
    R, S, Nf = 6, 130, 300
    rays, near, far, tc, w, v = _case(R, S, Nf, 12, True, True)
    rng = np.random.default_rng(13)
    for r in range(R):
        tc[r] = rng.permutation(tc[r])
    tc[0, 3] = np.float32(50.0)                            # and one value far outside [near, far]
    for a in abi_resample(rays, near, far, tc, w, Nf, v):
        assert np.isfinite(a).all()


def test_zero_width_coarse_bins():
    """Repeated coarse samples: bins of zero width.  Parity, and every copy of a repeated value is kept."""
    R, S, Nf = 5, 66, 96
    rays, near, far, tc, w, v = _case(R, S, Nf, 6, True, True)
    tc[0, 10:14] = tc[0, 10]
    tc[1, :] = tc[1, 30]
    tc[2, -3:] = tc[2, -3]
    tc[3, 0:2] = near[3]
    got = abi_resample(rays, near, far, tc, w, Nf, v)
    _check_exact(got[1], got[2], tc, near, far)
    _check_parity(got, rs.ray_resample(rays, near, far, tc, w, Nf, v), rays, near, far, w, "repeated ts_c")


@pytest.mark.parametrize("R,S,Nf", [(5, 65, 130), (7, 300, 70), (2 * 1024 + 3, 2, 3)])
def test_every_element_written_and_the_same_bits_whatever_the_outputs_held(R, S, Nf):
    rays, near, far, tc, w, v = _case(R, S, Nf, 8, True, True)
    a = abi_resample(rays, near, far, tc, w, Nf, v)
    b = abi_resample(rays, near, far, tc, w, Nf, v, fill=-3.0)
    for u, x in zip(a, b):
        assert not np.isnan(u).any() and u.tobytes() == x.tobytes()


def test_functional_calls_are_the_abi_calls():
    from wire_amd import functional
    R, S, Nf = 9, 20, 33
    rays, near, far, tc, w, v = _case(R, S, Nf, 9, True, True)
    want = abi_resample(rays, near, far, tc, w, Nf, v, eps=1e-3)
    got = functional.ray_resample(_dev(rays), _dev(near), _dev(far), _dev(tc), _dev(w), Nf, jitter=_dev(v), eps=1e-3)
    assert [tuple(g.shape) for g in got] == [(R * (S + Nf), 3), (R, S + Nf), (R, S + Nf)]
    assert not any(g.requires_grad for g in got)
    for g, x in zip(_np(*got), want):
        assert g.tobytes() == x.tobytes()
    want = abi_resample(rays, np.float32(0.3), np.float32(2.7), tc, w, Nf)
    for g, x in zip(_np(*functional.ray_resample(_dev(rays), 0.3, 2.7, _dev(tc), _dev(w), Nf)), want):
        assert g.tobytes() == x.tobytes()
    y, ts, dl = _inputs(R, 66, 3, 10)
    for density in ("softplus", "relu"):
        want = abi_weights(y, dl, density)
        yt = _dev(y).requires_grad_(True)
        got = functional.composite_weights(yt, _dev(dl), density=density)
        assert got.shape == (R, 66) and not got.requires_grad
        assert _np(got)[0].tobytes() == want.tobytes()
        assert _np(functional.composite_weights(_dev(y).reshape(R, 66, 4), _dev(dl), density))[0].tobytes() == \
            want.tobytes()


# ---------------------------------------------------------------------------------------------------------------------
# FusedTrainer.step_rays(n_importance=...): one step, in two halves
# ---------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("fam", ["x2", "x3"])
@pytest.mark.parametrize("net", ["siren", "wire_k90"])
def test_step_rays_hierarchical_one_step(net, fam):
    """R = 96 rays, S = 16 jittered coarse and Nf = 32 jittered fine samples (4 608 second-pass rows).  (a) the positions
    the step trained on are the restatement's, fed the device's own ``ray_w`` -- so the sensitivity of the positions to
    the coarse pass does not enter (b): the loss and every parameter gradient against the oracle net composed with the
    compositing restatement AT the device's positions, within 2 x the fp32 oracle's own error + 1e-6."""
    from wire_amd.trainer import FusedTrainer
    R, S, Nf = 96, 16, 32
    M = S + Nf
    model = er.build(net, 3, 4, DEV)
    sd = er.state(model)
    rays = _rays(R, 51)
    rng = np.random.default_rng(52)
    near = rng.uniform(1.0, 1.5, R).astype(np.float32)
    far = (near + rng.uniform(1.5, 2.5, R)).astype(np.float32)
    u = rng.uniform(0, 1, (R, S)).astype(np.float32)
    v = rng.uniform(0, 1, (R, Nf)).astype(np.float32)
    tgt = rng.uniform(0, 1, (R, 3)).astype(np.float32)
    bg = np.float32([0.2, 0.5, 0.8])
    tr = FusedTrainer(model, (4, 4, 4), None, lr=0.0)
    with family_ctx(fam):
        loss = tr.step_rays(_dev(rays), _dev(tgt), _dev(near), _dev(far), S, jitter=_dev(u), background=bg,
                            n_importance=Nf, jitter_fine=_dev(v))
        torch.cuda.synchronize()
    loss, flat = float(loss.item()), tr.flat_grad.cpu().numpy().astype(np.float64)
    # (a) positions
    w_dev = tr.ray_w.cpu().numpy()
    assert w_dev.shape == (R, S) and np.isfinite(w_dev).all() and w_dev.max() > 0
    _, tc, _ = rr.ray_samples(rays, near, far, S, u)
    got = (tr.coords[:R * M * 3].cpu().numpy().reshape(R * M, 3), tr.ray_ts[:R * M].cpu().numpy().reshape(R, M),
           tr.ray_deltas[:R * M].cpu().numpy().reshape(R, M))
    _check_exact(got[1], got[2], tc, near, far)
    _check_parity(got, rs.ray_resample(rays, near, far, tc, w_dev, Nf, v), rays, near, far, w_dev,
                  f"step_rays {net} {fam}")
    # (b) loss and gradients at the device's positions
    coords, ts, dl = got
    l64, g64 = _oracle_step(net, sd, coords, ts, dl, tgt, bg, "softplus", True)
    l32, g32 = _oracle_step(net, sd, coords, ts, dl, tgt, bg, "softplus", False)
    names = [k for k in model.state_dict().keys() if "omega_0" not in k and "scale_0" not in k]
    assert len(names) == len(tr.offsets) and np.abs(flat).max() > 0
    checks = [(f"step_rays hier {net} {fam} loss", abs(loss - l64) / l64, abs(l32 - l64) / l64)]
    for name, off in zip(names, tr.offsets):
        g = wo.as_real_pairs(g64[name]).astype(np.float64).ravel()
        r = wo.as_real_pairs(g32[name]).astype(np.float64).ravel()
        checks.append((f"step_rays hier {net} {fam} {name}", relmax(flat[off:off + g.size], g), relmax(r, g)))
    for lab, eb, e32 in checks:
        print(f"{lab}: err_build {eb:.3e}  err_ref {e32:.3e}  ratio {eb / e32 if e32 > 0 else float('inf'):.2f}")
    for lab, eb, e32 in checks:
        within_ref(eb, e32, lab)
    assert np.isfinite(tr.ray_rgb.cpu().numpy()).all()


def test_n_importance_zero_is_the_step_without_the_argument():
    from wire_amd.trainer import FusedTrainer
    R, S = 40, 12
    rays = _dev(_rays(R, 71))
    rng = np.random.default_rng(72)
    tgt, u = _dev(rng.uniform(0, 1, (R, 3)).astype(np.float32)), _dev(rng.uniform(0, 1, (R, S)).astype(np.float32))
    out = []
    for kw in ({}, dict(n_importance=0), dict(n_importance=0, jitter_fine=None)):
        tr = FusedTrainer(_small_siren().to(DEV), (4, 4, 4), None, lr=1e-3)
        losses = [tr.step_rays(rays, tgt, 1.2, 3.4, S, jitter=u, **kw).clone() for _ in range(3)]
        torch.cuda.synchronize()
        out.append(_np(torch.cat(losses), tr.flat_grad.clone(), tr.coords[:R * S * 3].clone()))
    for other in out[1:]:
        for a, b in zip(out[0], other):
            assert a.tobytes() == b.tobytes()
    with pytest.raises(ValueError):
        tr.step_rays(rays, tgt, 1.2, 3.4, S, jitter_fine=_dev(np.zeros((R, 4), np.float32)))
    with pytest.raises(ValueError):
        tr.step_rays(rays, tgt, 1.2, 3.4, S, n_importance=-1)
    with pytest.raises(ValueError):
        tr.step_rays(rays, tgt, 1.2, 3.4, S, n_importance=2000)
    with pytest.raises(ValueError):
        tr.step_rays(rays, tgt, 1.2, 3.4, S, n_importance=4, jitter_fine=_dev(np.zeros((R, 5), np.float32)))


# ---------------------------------------------------------------------------------------------------------------------
# a short trajectory, and render_rays
# ---------------------------------------------------------------------------------------------------------------------
TRAJ_S, TRAJ_NF = 8, 16


def _eager_loop(sd, rays, target, steps, lr, double):
    """Adam on the hierarchical loss in eager torch: each step resamples from this loop's own coarse pass (its weights
    in the loop's dtype, rounded to fp32 as the device's are) through the restatement."""
    dt = torch.float64 if double else torch.float32
    p = er.tensors(sd, double, requires_grad=True)
    opt = torch.optim.Adam(list(p.values()), lr=lr)
    near, far = np.float32(0.0), np.float32(2.0)
    cc, tc, dc = rr.ray_samples(rays, near, far, TRAJ_S)
    xc, dct, tgt = torch.tensor(cc).to(dt), torch.tensor(dc).to(dt), torch.tensor(target).to(dt)
    R = rays.shape[0]
    losses = []
    for _ in range(steps):
        with torch.no_grad():
            yc = torch_ref.realnet_forward("siren", p, xc, 2, *HP, None).reshape(R, TRAJ_S, -1)
            a = torch.nn.functional.softplus(yc[..., -1]) * dct
            tau = torch.cumsum(a, dim=1) - a
            w = (torch.exp(-tau) * -torch.expm1(-a)).to(torch.float32).numpy()
        coords, ts, dl = rs.ray_resample(rays, near, far, tc, w, TRAJ_NF)
        opt.zero_grad()
        y = torch_ref.realnet_forward("siren", p, torch.tensor(coords).to(dt), 2, *HP, None)
        loss = ((rr.torch_composite(y, torch.tensor(ts).to(dt), torch.tensor(dl).to(dt))[0] - tgt) ** 2).mean()
        loss.backward()
        opt.step()
        losses.append(float(loss.detach()))
    return np.array(losses)


def test_hierarchical_trajectory_follows_the_fp64_loop():
    """30 steps of step_rays(S = 8, n_importance = 16) on test_gpu_render's blob scene (576 rays, siren 2 x 64, Adam
    1e-3): the loss sequence stays with the fp64 eager loop by test_gpu_render's rule -- drift <= 4 x the fp32 eager loop's
    drift + 2e-5, self-calibrating because the fp32 loop resamples with the same conditioning -- and the loss falls."""
    from wire_amd.trainer import FusedTrainer
    rays, target = _scene()
    model = _small_siren()
    sd = er.state(model)
    steps, lr = 30, 1e-3
    l64 = _eager_loop(sd, rays, target, steps, lr, True)
    l32 = _eager_loop(sd, rays, target, steps, lr, False)
    tr = FusedTrainer(model.to(DEV), (4, 4, 4), None, lr=lr)
    r, t = _dev(rays), _dev(target)
    losses = [tr.step_rays(r, t, 0.0, 2.0, TRAJ_S, n_importance=TRAJ_NF) for _ in range(steps)]
    torch.cuda.synchronize()
    losses = np.array([float(v.item()) for v in losses])
    drift, drift_ref = np.abs(losses - l64) / l64, np.abs(l32 - l64) / l64
    print(f"hierarchical trajectory: loss {losses[0]:.5e} -> {losses[-1]:.5e} (fp64 {l64[0]:.5e} -> {l64[-1]:.5e}); "
          f"drift vs fp64: build max {drift.max():.2e}, fp32 eager max {drift_ref.max():.2e}")
    RATIO_LOG.append(("hierarchical trajectory drift [build, 4 x fp32 eager + 2e-5]", float(drift.max()),
                      float(4 * drift_ref.max() + 2e-5)))
    assert np.isfinite(losses).all()
    assert drift.max() <= 4 * drift_ref.max() + 2e-5
    assert losses[-1] < losses[0]


def test_render_rays_hierarchical_is_the_abi_chain_and_does_not_depend_on_the_tiling():
    from wire_amd import _lib
    from wire_amd.trainer import FusedTrainer
    model = _small_siren().to(DEV)
    tr = FusedTrainer(model, (4, 4, 4), None, lr=0.0)
    R, S, Nf = 40, 16, 24
    M = S + Nf
    rays = _rays(R, 61)
    rng = np.random.default_rng(62)
    near = rng.uniform(1.0, 1.5, R).astype(np.float32)
    far = (near + rng.uniform(1.5, 2.5, R)).astype(np.float32)
    bg = np.float32([0.3, 0.1, 0.6])
    r, nr, fr = _dev(rays), _dev(near), _dev(far)
    one = _np(*tr.render_rays(r, nr, fr, S, tile_rays=R, background=bg, density="relu", n_importance=Nf))
    assert [v.shape for v in one] == [(R, 3), (R,), (R,)] and all(np.isfinite(v).all() for v in one)
    # the same through the ABI: sampler, forward, weights, resampler, forward, wire_composite_fwd
    L, d = _lib.lib(), C.byref(tr.desc)
    bounds = _dev(np.stack([near, far], 1))
    ab = _lib.check(L.wire_act_bytes(d, R * M, 0))
    act = torch.empty(max(ab, 16), dtype=torch.uint8, device=DEV)
    xc, tc, dc, yc, w = _full(R * S, 3), _full(R, S), _full(R, S), _full(R * S, 4), _full(R, S)
    x, ts, dl, y = _full(R * M, 3), _full(R, M), _full(R, M), _full(R * M, 4)
    rgb, acc, depth = _full(R, 3), _full(R), _full(R)
    _call("wire_ray_samples", r.data_ptr(), bounds.data_ptr(), 0.0, 0.0, None, R, S, xc.data_ptr(), tc.data_ptr(),
          dc.data_ptr())
    _call("wire_mlp_fwd", d, tr.packed.data_ptr(), xc.data_ptr(), R * S, yc.data_ptr(), act.data_ptr(), ab, 0)
    _call("wire_composite_weights", yc.data_ptr(), dc.data_ptr(), R, S, 4, 1, w.data_ptr())
    _call("wire_ray_resample", r.data_ptr(), bounds.data_ptr(), 0.0, 0.0, tc.data_ptr(), w.data_ptr(), None, 1e-5, R, S,
          Nf, x.data_ptr(), ts.data_ptr(), dl.data_ptr())
    _call("wire_mlp_fwd", d, tr.packed.data_ptr(), x.data_ptr(), R * M, y.data_ptr(), act.data_ptr(), ab, 0)
    _call("wire_composite_fwd", y.data_ptr(), ts.data_ptr(), dl.data_ptr(), _dev(bg).data_ptr(), R, M, 4, 1,
          rgb.data_ptr(), acc.data_ptr(), depth.data_ptr())
    for u, v in zip(one, _np(rgb, acc, depth)):
        assert u.tobytes() == v.tobytes()
    for tile in (7, 16, 10 ** 6):                          # (both passes below the 4 096-row family switch)
        got = _np(*tr.render_rays(r, nr, fr, S, tile_rays=tile, background=bg, density="relu", n_importance=Nf))
        for u, v in zip(one, got):
            assert u.tobytes() == v.tobytes(), tile
    a = _np(*tr.render_rays(r, 1.2, 3.4, S, tile_rays=9, n_importance=Nf))
    b = _np(*tr.render_rays(r, 1.2, 3.4, S, n_importance=Nf))
    assert all(u.tobytes() == v.tobytes() for u, v in zip(a, b))
    zero = _np(*tr.render_rays(r, nr, fr, S, background=bg, n_importance=0))
    plain = _np(*tr.render_rays(r, nr, fr, S, background=bg))
    assert all(u.tobytes() == v.tobytes() for u, v in zip(zero, plain))
