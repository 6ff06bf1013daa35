"""Host checks of the hierarchical resampler (no GPU): the fp64 restatement tests/resample_ref.py against hand values,
its invariants, the lattice property of the stratified draws and an independent torch fp64 implementation; the two new
symbols of the C ABI and their argument checks (every WIRE_ERR_ARG case returns before the first HIP call, so fake
pointers and a NULL stream serve); the refusals of ``functional.composite_weights`` / ``functional.ray_resample``."""
import numpy as np
import pytest
import torch

import render_ref as rr
import resample_ref as rs


# ---------------------------------------------------------------------------------------------------------------------
# the restatement: hand values
# ---------------------------------------------------------------------------------------------------------------------
RAY = np.array([[1, 2, 3, 0, 3, 4.0]], np.float32)                                     # |d| = 5


def test_one_bin_is_near_to_far():
    """S = 1: the only bin is [near, far], so the draws are the strata's midpoints whatever the weight is."""
    for w in (0.0, 0.7, 1e30):
        coords, ts, dl = rs.ray_resample(RAY, 1.0, 3.0, np.float32([[2.5]]), np.float32([[w]]), 4)
        np.testing.assert_array_equal(ts[0], np.float32([1.25, 1.75, 2.25, 2.5, 2.75]))    # the coarse 2.5 among them
        np.testing.assert_array_equal(dl[0], np.float32([2.5, 2.5, 1.25, 1.25, 1.25]))     # the last one runs to far
        np.testing.assert_array_equal(coords[3], np.float32([1, 2 + 3 * 2.5, 3 + 4 * 2.5]))
    assert coords.dtype == ts.dtype == dl.dtype == np.float32 and coords.shape == (5, 3) and ts.shape == (1, 5)


def test_equal_weights_give_draws_uniform_in_the_bins():
    """Four midpoint samples of [0, 4]: the bins are [0, 1], [1, 2], [2, 3], [3, 4]; equal mass -> the draws are the
    midpoints of the Nf strata of [0, 4], and all-zero weights give the same (eps alone is the mass)."""
    tc = np.float32([[0.5, 1.5, 2.5, 3.5]])
    for w in (np.full((1, 4), 0.25, np.float32), np.zeros((1, 4), np.float32)):
        tf, bins = rs.fine_samples(0.0, 4.0, tc, w, 8)
        np.testing.assert_allclose(tf[0], 0.25 + 0.5 * np.arange(8), rtol=0, atol=1e-12)
        np.testing.assert_array_equal(bins[0], [0, 0, 1, 1, 2, 2, 3, 3])
    # a tie: a draw that lands on a coarse value comes after it (coarse first), and both stay in the list
    _, ts, dl = rs.ray_resample(RAY, 0.0, 4.0, tc, np.zeros((1, 4), np.float32), 4)    # draws 0.5, 1.5, 2.5, 3.5
    np.testing.assert_array_equal(ts[0], np.float32([0.5, 0.5, 1.5, 1.5, 2.5, 2.5, 3.5, 3.5]))
    np.testing.assert_allclose(dl[0], np.float32([0, 5, 0, 5, 0, 5, 0, 2.5]), rtol=0, atol=1e-6)   # (unrounded t: f = 0.5 +- an ulp)


def test_one_dominant_bin_takes_the_draws():
    """w = (0, 1, 0, 0) with eps = 1e-5: all but a 3e-5 share of the mass lies in bin 1 = [1, 2]; 8 draws at v = 0.5 all
    land there, at 1 + (k + 0.5) / 8 to within the share."""
    tc = np.float32([[0.5, 1.5, 2.5, 3.5]])
    w = np.float32([[0, 1, 0, 0]])
    tf, bins = rs.fine_samples(0.0, 4.0, tc, w, 8)
    assert np.all(bins[0] == 1)
    np.testing.assert_allclose(tf[0], 1.0 + (np.arange(8) + 0.5) / 8, rtol=0, atol=1e-4)
    p, c = rs.mass(w)
    np.testing.assert_allclose(c[0], np.cumsum([0, 1e-5, 1 + 1e-5, 1e-5, 1e-5]), rtol=1e-6)
    # NaN and negative weights count as 0, +inf as FLT_MAX
    p, _ = rs.mass(np.float32([[np.nan, -3.0, np.inf, 2.0]]), eps=0.5)
    np.testing.assert_array_equal(p[0], [0.5, 0.5, rs.FLT_MAX + 0.5, 2.5])


def test_a_missing_ray_stays_at_near():
    near, far = np.float32([2.0, 2.5, 1.0]), np.float32([4.0, 2.5, np.nan])
    rays = np.tile(np.float32([0, 0, -3, 0, 0, 1.0]), (3, 1))
    tc = np.float32([[2.5, 3.5], [2.5, 2.5], [1.0, 2.0]])
    coords, ts, dl = rs.ray_resample(rays, near, far, tc, np.ones((3, 2), np.float32), 3)
    assert np.all(ts[1] == np.float32(2.5)) and np.all(dl[1] == 0) and np.all(dl[0] >= 0) and dl[0].sum() > 0
    assert np.all(ts[2] == np.float32(1.0)) and np.all(dl[2] == 0) and np.isfinite(coords).all()


# ---------------------------------------------------------------------------------------------------------------------
# the restatement: invariants, the lattice property, an independent implementation
# ---------------------------------------------------------------------------------------------------------------------
def _case(R, S, Nf, seed, jitter):
    rng = np.random.default_rng(seed)
    rays = np.concatenate([rng.uniform(-2, 2, (R, 3)), rng.normal(0, 1, (R, 3))], 1).astype(np.float32)
    near = rng.uniform(0.1, 1.0, R).astype(np.float32)
    far = (near + rng.uniform(0.5, 3.0, R)).astype(np.float32)
    uc = rng.uniform(0.1, 0.9, (R, S)).astype(np.float32)
    _, tc, _ = rr.ray_samples(rays, near, far, S, uc)
    w = (rng.uniform(0, 1, (R, S)) ** 8).astype(np.float32)
    v = rng.uniform(0, 1, (R, Nf)).astype(np.float32) if jitter else None
    return rays, near, far, tc, w, v


@pytest.mark.parametrize("jitter", [False, True])
@pytest.mark.parametrize("Nf", [1, 65, 128])
@pytest.mark.parametrize("S", [1, 2, 65, 130])
def test_restatement_invariants(S, Nf, jitter):
    R = 5
    rays, near, far, tc, w, v = _case(R, S, Nf, 1000 * S + Nf, jitter)
    w[1] = 0.0
    tf, bins = rs.fine_samples(near, far, tc, w, Nf, v)
    assert np.all(np.diff(tf, axis=1) >= 0) and np.all(np.diff(bins, axis=1) >= 0)
    assert np.all(tf >= near[:, None].astype(np.float64)) and np.all(tf <= far[:, None].astype(np.float64))
    e = rs.edges(near, far, tc)
    assert np.all(tf >= np.take_along_axis(e, bins, 1)) and np.all(tf <= np.take_along_axis(e, bins + 1, 1))
    coords, ts, dl = rs.ray_resample(rays, near, far, tc, w, Nf, v)
    assert ts.shape == dl.shape == (R, S + Nf) and coords.shape == (R * (S + Nf), 3)
    assert np.all(np.diff(ts, axis=1) >= 0) and np.all(dl >= 0)
    assert np.all(ts >= near[:, None]) and np.all(ts <= far[:, None])
    for r in range(R):                                     # every coarse value is there with its bits, as often
        vals, counts = np.unique(tc[r], return_counts=True)
        for val, n in zip(vals, counts):
            assert (ts[r].view(np.uint32) == val.view(np.uint32)).sum() >= n


@pytest.mark.parametrize("S,Nf", [(1, 7), (2, 65), (65, 128), (130, 65), (16, 1000)])
def test_lattice_property(S, Nf):
    """v = 0.5: a lattice of spacing 1 / Nf meets the interval of length p_s / tot that bin s takes of the normalised
    CDF in floor(Nf p_s / tot) or ceil(Nf p_s / tot) points (1e-9: the rounding of the sums where the product is whole)."""
    R = 4
    _, near, far, tc, w, _ = _case(R, S, Nf, 7 * S + Nf, False)
    w[2] = 0.0
    _, bins = rs.fine_samples(near, far, tc, w, Nf)
    p, c = rs.mass(w)
    for r in range(R):
        n = np.bincount(bins[r], minlength=S)
        share = Nf * p[r] / c[r, -1]
        assert n.sum() == Nf and np.all(n >= np.floor(share - 1e-9)) and np.all(n <= np.ceil(share + 1e-9)), r


def _torch_resample(rays, near, far, tc, w, Nf, v, eps=1e-5):
    """The same operator in torch fp64: cumsum, searchsorted, sort."""
    f64 = lambda a: torch.tensor(np.asarray(a, np.float32)).double()
    rays, tc, w = f64(rays), f64(tc), f64(w)
    R, S = tc.shape
    nr, fr = f64(near).expand(R)[:, None], f64(far).expand(R)[:, None]
    p = torch.clamp(torch.nan_to_num(w, nan=0.0, posinf=rs.FLT_MAX), 0.0, rs.FLT_MAX) + float(np.float32(eps))
    c = torch.cat([torch.zeros(R, 1, dtype=torch.float64), torch.cumsum(p, 1)], 1)
    e = torch.cat([nr, (tc[:, :-1] + tc[:, 1:]) / 2, fr], 1)
    vv = torch.full((R, Nf), 0.5, dtype=torch.float64) if v is None else f64(v)
    u = (torch.arange(Nf, dtype=torch.float64)[None] + vv) / Nf * c[:, -1:]
    s = (torch.searchsorted(c.contiguous(), u.contiguous(), right=True) - 1).clamp(0, S - 1)
    c0, c1, e0, e1 = c.gather(1, s), c.gather(1, s + 1), e.gather(1, s), e.gather(1, s + 1)
    f = ((u - c0) / (c1 - c0)).clamp(0, 1)
    tf = torch.minimum(e0 + f * (e1 - e0), e1)
    t = torch.sort(torch.cat([tc, tf], 1), dim=1, stable=True)[0]
    t1 = torch.cat([t[:, 1:], fr], 1)
    d = rays[:, 3:]
    dl = (t1 - t) * torch.sqrt(d[:, 0] * d[:, 0] + d[:, 1] * d[:, 1] + d[:, 2] * d[:, 2])[:, None]
    coords = rays[:, None, :3] + t[..., None] * d[:, None, :]
    return coords.reshape(-1, 3).float().numpy(), t.float().numpy(), dl.float().numpy()


@pytest.mark.parametrize("jitter", [False, True])
@pytest.mark.parametrize("S,Nf", [(1, 1), (2, 65), (65, 128), (130, 1)])
def test_restatement_agrees_with_torch_fp64(S, Nf, jitter):
    """cumsum / searchsorted / sort of torch in fp64 on the same inputs: both sum left to right, so the fp32 results
    agree to the last bit of ts (one ulp allowed for deltas and coords, whose last products differ in association)."""
    rays, near, far, tc, w, v = _case(6, S, Nf, 31 * S + Nf, jitter)
    got = rs.ray_resample(rays, near, far, tc, w, Nf, v)
    want = _torch_resample(rays, near, far, tc, w, Nf, v)
    k = rs.kappa(w, near, far)[:, None]
    assert np.all(np.abs(got[1].astype(np.float64) - want[1]) <= rs.ulp32(np.maximum(np.abs(near), np.abs(far)))[:, None] + k)
    norm = np.linalg.norm(rays[:, 3:].astype(np.float64), axis=1)[:, None]
    assert np.all(np.abs(got[2].astype(np.float64) - want[2]) <= rs.ulp32(want[2]) + 2 * k * norm)
    assert np.abs(got[0].astype(np.float64) - want[0]).max() <= rs.ulp32(np.abs(want[0]).max()) + k.max() * np.abs(rays[:, 3:]).max()


# ---------------------------------------------------------------------------------------------------------------------
# the C ABI
# ---------------------------------------------------------------------------------------------------------------------
NAMES = ["wire_composite_weights", "wire_ray_resample"]
P = 0x10000            # a fake, 16-byte aligned device pointer: the checks below return before anything reads it
ARG = -1


def test_symbols_declared_and_exported():
    from wire_amd import _lib
    lib = _lib.lib()
    for n in NAMES:
        assert n in _lib.SYMBOLS and hasattr(lib, n)
    import os
    hdr = open(os.path.join(os.path.dirname(os.path.dirname(os.path.abspath(__file__))), "include", "wire_hip.h")).read()
    assert "int wire_composite_weights(" in hdr and "int wire_ray_resample(" in hdr


def _weights(lib, **kw):
    a = dict(y=P, deltas=P, R=4, S=8, O=4, density=0, w=P)
    a.update(kw)
    return lib.wire_composite_weights(None, a["y"], a["deltas"], a["R"], a["S"], a["O"], a["density"], a["w"])


def _resample(lib, **kw):
    a = dict(rays=P, bounds=None, near=0.0, far=1.0, ts_c=P, w=P, jitter=None, eps=1e-5, R=4, S=8, Nf=16, coords=P,
             ts=P, deltas=P)
    a.update(kw)
    return lib.wire_ray_resample(None, a["rays"], a["bounds"], a["near"], a["far"], a["ts_c"], a["w"], a["jitter"],
                                 a["eps"], a["R"], a["S"], a["Nf"], a["coords"], a["ts"], a["deltas"])


BIG_R = 4 * (2 ** 31 - 1) + 1       # one ray more than 2^31 - 1 workgroups of 4 rays hold
IDS = lambda d: ",".join(f"{k}={v}" for k, v in d.items())


@pytest.mark.parametrize("bad", [dict(R=0), dict(R=-3), dict(S=0), dict(S=-1), dict(R=2 ** 62, S=2 ** 20),
                                 dict(R=BIG_R, S=1), dict(O=1), dict(O=9), dict(O=0), dict(density=2),
                                 dict(density=-1), dict(y=None), dict(y=P + 8), dict(y=P + 4), dict(deltas=None),
                                 dict(deltas=P + 1), dict(w=None), dict(w=P + 2)], ids=IDS)
def test_composite_weights_refuses(bad):
    from wire_amd import _lib
    lib = _lib.lib()
    assert _weights(lib, **bad) == ARG
    assert b"wire_composite_weights" in lib.wire_last_error()


@pytest.mark.parametrize("bad", [dict(R=0), dict(R=-3), dict(S=0), dict(S=-1), dict(Nf=0), dict(Nf=-2), dict(S=1025),
                                 dict(Nf=1025), dict(S=2 ** 31 - 1, Nf=2), dict(R=2 ** 62), dict(R=BIG_R),
                                 dict(R=2 * (2 ** 31 - 1) + 1, S=257),       # two rays per workgroup beyond S = 256
                                 dict(near=float("nan")), dict(far=float("inf")), dict(eps=0.0), dict(eps=-1e-5),
                                 dict(eps=float("nan")), dict(eps=float("inf")), dict(rays=None), dict(ts_c=None),
                                 dict(w=None), dict(coords=None), dict(ts=None), dict(deltas=None), dict(rays=P + 1),
                                 dict(bounds=P + 3), dict(ts_c=P + 2), dict(w=P + 1), dict(jitter=P + 1),
                                 dict(coords=P + 2), dict(ts=P + 2), dict(deltas=P + 3)], ids=IDS)
def test_ray_resample_refuses(bad):
    from wire_amd import _lib
    lib = _lib.lib()
    assert _resample(lib, **bad) == ARG
    assert b"wire_ray_resample" in lib.wire_last_error()


# ---------------------------------------------------------------------------------------------------------------------
# the Python surface
# ---------------------------------------------------------------------------------------------------------------------
def test_functional_refusals_on_the_host():
    from wire_amd import _lib, functional
    R, S, Nf = 5, 4, 6
    rays, ts, w = torch.zeros(R, 6), torch.zeros(R, S), torch.zeros(R, S)
    with pytest.raises(_lib.WireHipError):
        functional.ray_resample(rays, 0.0, 1.0, ts, w, Nf)
    with pytest.raises(_lib.WireHipError):
        functional.ray_resample(rays, torch.zeros(R), torch.ones(R), ts, w, Nf, jitter=torch.zeros(R, Nf), eps=1e-3)
    for bad in (dict(rays=torch.zeros(R, 5)), dict(rays=torch.zeros(R, 6, dtype=torch.float64)),
                dict(rays=torch.zeros(6)), dict(near=torch.zeros(R)), dict(far=float("inf")),
                dict(ts=torch.zeros(R + 1, S)), dict(ts=torch.zeros(R, S, dtype=torch.float64)), dict(ts=torch.zeros(R * S)),
                dict(ts=torch.zeros(R, 0), w=torch.zeros(R, 0)), dict(ts=torch.zeros(S, R).t()),
                dict(w=torch.zeros(R, S + 1)), dict(w=w.double()), dict(w=None), dict(n=0), dict(n=1025),
                dict(ts=torch.zeros(R, 1025), w=torch.zeros(R, 1025)), dict(jitter=torch.zeros(R, S)),
                dict(jitter=torch.zeros(R, Nf, dtype=torch.float64)), dict(eps=0.0), dict(eps=float("nan")),
                dict(eps=-1.0)):
        a = dict(rays=rays, near=0.0, far=1.0, ts=ts, w=w, n=Nf, jitter=None, eps=1e-5)
        a.update(bad)
        with pytest.raises(ValueError):
            functional.ray_resample(a["rays"], a["near"], a["far"], a["ts"], a["w"], a["n"], a["jitter"], a["eps"])
    y, dl = torch.zeros(R * S, 4), torch.zeros(R, S)
    with pytest.raises(_lib.WireHipError):
        functional.composite_weights(y, dl)
    with pytest.raises(_lib.WireHipError):
        functional.composite_weights(y.reshape(R, S, 4).requires_grad_(True), dl, density="relu")
    for bad in (dict(y=torch.zeros(R * S, 1)), dict(y=torch.zeros(R * S, 9)), dict(y=torch.zeros(R * S + 1, 4)),
                dict(y=y.double()), dict(y=None), dict(dl=torch.zeros(R, S + 1)), dict(dl=dl.double()),
                dict(dl=torch.zeros(R * S)), dict(density="exp"), dict(density=1)):
        a = dict(y=y, dl=dl, density="softplus")
        a.update(bad)
        with pytest.raises(ValueError):
            functional.composite_weights(a["y"], a["dl"], a["density"])
