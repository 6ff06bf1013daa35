"""GPU checks of the iso-surface extraction (csrc/wire_iso.hip, functional.iso_surface, volutils.march_and_save /
export_mesh, FusedTrainer.extract_mesh) against the numpy restatement tests/iso_ref.py.

EQUALITY.  Faces are compared as integers.  Vertices: |device - fp64| <= 4 * 2^-24 * (1 + coordinate) per coordinate
(iso_ref.vertex_bound).  Derivation: t = (thres - a) / (b - a) takes three fp32 roundings (the two differences and the
quotient), each a relative 2^-24 of a value with t <= 1; p + t d takes one more, relative to the coordinate.  The bound is
derived, not measured.

The scan's tile is WIRE_SCAN_TILE = 1024 values (csrc/wire_scan.h): a volume of more than 1024 points takes the
three-launch path, one of more than 1024^2 = 1 048 576 points scans its tile sums over several tiles themselves.
"""
import numpy as np
import pytest
import torch

import iso_ref
from _util import ROOT  # noqa: F401
from workspace_fill import ONES, ZERO, fill

pytestmark = pytest.mark.gpu
DEV = "cuda"
SCAN_TILE = 1024
GUARD = 0x5A5A5A5A


def _dev(vol):
    return torch.from_numpy(np.ascontiguousarray(vol, np.float32)).to(DEV)


def _extract(vol, thres):
    from wire_amd import functional
    v, f = functional.iso_surface(_dev(vol), thres)
    assert v.dtype == torch.float32 and f.dtype == torch.int32 and v.is_cuda and f.is_cuda
    return v.cpu().numpy(), f.cpu().numpy()


def _assert_equal(vol, thres, label):
    v, f = _extract(vol, thres)
    rv, rf = iso_ref.extract(vol, thres)
    assert (len(v), len(f)) == (len(rv), len(rf)), label
    np.testing.assert_array_equal(f, rf, err_msg=str(label))
    d = np.abs(v.astype(np.float64) - rv)
    print(f"{label}: {len(v)} vertices, {len(f)} faces, max |dv| / bound = "
          f"{(d / iso_ref.vertex_bound(rv)).max() if len(v) else 0:.3f}")
    assert (d <= iso_ref.vertex_bound(rv)).all(), label
    return v, f, rv, rf


def _abi(vol_t, thres, ws_fill=None, short_v=0, short_f=0, guard=16):
    """wire_iso_count + wire_iso_emit through ctypes with capacities (count - short) and ``guard`` sentinel words behind
    each output.  Returns (return code of emit, counts, verts buffer as int32, faces buffer, capacities)."""
    from wire_amd import _lib
    L = _lib.lib()
    H, W, T = vol_t.shape
    s = torch.cuda.current_stream().cuda_stream
    ws = torch.empty(_lib.check(L.wire_iso_ws_bytes(H, W, T)), dtype=torch.uint8, device=DEV)
    if ws_fill is not None:
        fill(ws, ws_fill)
    counts = torch.full((2,), -7, dtype=torch.int64, device=DEV)
    _lib.check(L.wire_iso_count(s, vol_t.data_ptr(), H, W, T, thres, ws.data_ptr(), counts.data_ptr()), "count")
    nv, nf = counts.tolist()
    cv, cf = max(nv - short_v, 0), max(nf - short_f, 0)
    vb = torch.full((3 * cv + guard,), GUARD, dtype=torch.int32, device=DEV)
    fb = torch.full((3 * cf + guard,), GUARD, dtype=torch.int32, device=DEV)
    rc = L.wire_iso_emit(s, vol_t.data_ptr(), H, W, T, thres, ws.data_ptr(), vb.data_ptr(), cv, fb.data_ptr(), cf)
    torch.cuda.synchronize()
    return rc, (nv, nf), vb.cpu().numpy(), fb.cpu().numpy(), (cv, cf)


def _noise(shape, seed):
    return np.random.default_rng(seed).standard_normal(shape).astype(np.float32)


def _ball(shape, radius, ripple=0.0):
    c = [s / 2 - 0.3 + 0.17 * a for a, s in enumerate(shape)]
    vol = iso_ref.sphere(shape, c, radius)
    if ripple:
        g = np.meshgrid(*[np.arange(n, dtype=np.float64) for n in shape], indexing="ij")
        vol = (vol + ripple * np.sin(0.9 * g[0]) * np.cos(0.7 * g[1] + 0.5 * g[2])).astype(np.float32)
    return vol, c


# ---- equality ---------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("shape", [(9, 8, 7), (5, 17, 3), (2, 2, 65), (33, 2, 2)])
def test_ragged_shapes_equal_restatement(shape):
    """White noise: nearly every cell is cut and every tetrahedron case occurs; the surface runs into the boundary."""
    _assert_equal(_noise(shape, sum(shape)), 0.1, shape)


def test_every_case_of_every_tetrahedron():
    """One cell, each of the 254 mixed sign patterns of its corners with random magnitudes."""
    rng = np.random.default_rng(11)
    for m in range(1, 255):
        sign = np.array([1.0 if (m >> b) & 1 else -1.0 for b in range(8)], np.float32)
        vol = (rng.uniform(0.1, 2.0, 8).astype(np.float32) * sign).reshape(2, 2, 2)
        v, f = _extract(vol, 0.0)
        rv, rf = iso_ref.extract(vol, 0.0)
        np.testing.assert_array_equal(f, rf, err_msg=f"pattern {m}")
        assert (np.abs(v - rv) <= iso_ref.vertex_bound(rv)).all(), m


def test_scan_over_several_tiles():
    """(37, 41, 43): 65 231 points = 63 tiles and 719 values, not a multiple of the tile; the full restatement."""
    shape = (37, 41, 43)
    assert np.prod(shape) % SCAN_TILE and np.prod(shape) > 8 * SCAN_TILE
    vol, _ = _ball(shape, 13.0, ripple=0.08)
    _assert_equal(vol, 0.5, shape)


def test_scan_of_the_tile_sums_spans_tiles():
    """(128, 96, 96): 1 179 648 points = 1152 tiles, so the tile sums themselves are scanned over two tiles (three
    levels).  Counts, every vertex (the restatement's vertices are vectorised), a sample of cells' faces -- the first,
    the last and 60 between -- and the census; not the Python loop over all cells."""
    shape = (128, 96, 96)
    assert np.prod(shape) > SCAN_TILE * SCAN_TILE
    vol, _ = _ball(shape, 40.0)
    v, f = _extract(vol, 0.5)
    assert (len(v), len(f)) == iso_ref.counts(vol, 0.5)
    rv = iso_ref.vertices(vol, 0.5)
    assert (np.abs(v - rv) <= iso_ref.vertex_bound(rv)).all()
    ntri = iso_ref.cell_tri_counts(vol, 0.5)
    off = np.cumsum(ntri.reshape(-1)) - ntri.reshape(-1)
    cut = np.flatnonzero(ntri.reshape(-1))
    pick = np.unique(np.concatenate([cut[:2], cut[-2:], cut[np.linspace(0, len(cut) - 1, 60).astype(int)]]))
    ins, (vid, _) = iso_ref.inside_of(vol, 0.5), iso_ref.vertex_ids(vol, 0.5)
    for c in pick:
        i, j, k = np.unravel_index(c, ntri.shape)
        want = iso_ref.cell_faces(ins, vid, i, j, k)
        np.testing.assert_array_equal(f[off[c]:off[c] + len(want)], np.array(want), err_msg=f"cell {(i, j, k)}")
    assert iso_ref.edge_census(f)[:2] == (0, 0) and iso_ref.euler(len(v), f) == 2


# ---- properties of the device output ----------------------------------------------------------------------------
def test_sphere_is_closed_oriented_and_its_volume_agrees():
    vol, c = _ball((20, 18, 16), 5.5)
    v, f, rv, rf = _assert_equal(vol, 0.5, "sphere")
    assert iso_ref.edge_census(f)[:2] == (0, 0) and iso_ref.euler(len(v), f) == 2
    sv, sr = iso_ref.signed_volume(v, f), iso_ref.signed_volume(rv, rf)
    # dV <= sum over faces of (|b x c| |da| + |a x c| |db| + |a x b| |dc|) / 6 for vertex errors within the bound
    # (first order; the 1 % on top covers the second)
    a, b, cc = rv[rf[:, 0]], rv[rf[:, 1]], rv[rf[:, 2]]
    dn = np.linalg.norm(iso_ref.vertex_bound(rv), axis=1)
    n = lambda x, y: np.linalg.norm(np.cross(x, y), axis=1)
    bound = 1.01 * (n(b, cc) * dn[rf[:, 0]] + n(a, cc) * dn[rf[:, 1]] + n(a, b) * dn[rf[:, 2]]).sum() / 6
    print(f"signed volume {sv:.6f} vs {sr:.6f}, |d| = {abs(sv - sr):.3e}, bound {bound:.3e}")
    assert sv > 0 and abs(sv - sr) <= bound
    nrm = np.cross(v[f[:, 1]] - v[f[:, 0]], v[f[:, 2]] - v[f[:, 0]])
    assert (np.einsum("ij,ij->i", nrm, v[f].mean(1) - np.array(c)) > 0).all()


def test_linear_field_vertices_lie_on_the_plane():
    """A field linear in (i, j, k) with dyadic coefficients is exact in fp32 and linear along every edge: the exact
    crossing lies on the plane, so the device vertex misses it by at most sum |coef| * bound(coordinate)."""
    coef, d0, thres = np.array([0.5, 0.25, -0.375]), 0.0625, float(np.float32(1.7))
    g = np.meshgrid(*[np.arange(n, dtype=np.float64) for n in (11, 9, 10)], indexing="ij")
    vol = (coef[0] * g[0] + coef[1] * g[1] + coef[2] * g[2] + d0).astype(np.float32)
    v, f = _extract(vol, thres)
    assert len(f) > 0
    v = v.astype(np.float64)
    resid = np.abs(v @ coef + d0 - thres)
    assert (resid <= (iso_ref.vertex_bound(v) * np.abs(coef)).sum(1)).all(), resid.max()


def test_threshold_equal_to_data():
    """A binary volume cut at 1.0: crossings sit on lattice points and coincide; closed and consistently wound still."""
    vol = (_ball((14, 13, 12), 4.2)[0] >= 0.5).astype(np.float32)
    v, f, rv, rf = _assert_equal(vol, 1.0, "binary")
    assert len(f) > 0 and iso_ref.edge_census(f)[:2] == (0, 0) and iso_ref.euler(len(v), f) == 2
    assert len(np.unique(v, axis=0)) < len(v)
    assert iso_ref.signed_volume(v, f) > 0


def test_non_finite_data_keeps_counts_and_writes_in_range():
    vol = _noise((6, 5, 7), 3)
    vol[2, 2, 3], vol[0, 0, 0], vol[5, 4, 6] = np.nan, np.inf, -np.inf
    rc, (nv, nf), vb, fb, (cv, cf) = _abi(_dev(vol), 0.0)
    assert rc == 0 and (nv, nf) == iso_ref.counts(vol, 0.0)
    rv, rf = iso_ref.extract(vol, 0.0)
    np.testing.assert_array_equal(fb[:3 * cf].reshape(-1, 3), rf)
    assert (vb[3 * cv:] == GUARD).all() and (fb[3 * cf:] == GUARD).all()


def test_empty_volumes():
    from wire_amd import functional
    for value in (0.0, 1.0):
        vol = torch.full((5, 6, 7), value, device=DEV)
        v, f = functional.iso_surface(vol, 0.5)
        assert tuple(v.shape) == (0, 3) and tuple(f.shape) == (0, 3)
        rc, counts, vb, fb, _ = _abi(vol, 0.5)
        assert rc == 0 and counts == (0, 0) and (vb == GUARD).all() and (fb == GUARD).all()


def test_capacity_one_short_writes_nothing():
    vol = _dev(_noise((9, 8, 7), 24))
    for short_v, short_f in ((1, 0), (0, 1)):
        rc, (nv, nf), vb, fb, _ = _abi(vol, 0.1, short_v=short_v, short_f=short_f)
        assert nv > 0 and nf > 0
        assert rc == -3                                             # WIRE_ERR_SIZE
        assert (vb == GUARD).all() and (fb == GUARD).all()          # the outputs and the guard words behind them
    rc, _, vb, fb, (cv, cf) = _abi(vol, 0.1)
    assert rc == 0 and (vb[3 * cv:] == GUARD).all() and (fb[3 * cf:] == GUARD).all()
    assert (fb[:3 * cf] != GUARD).all()


def test_bit_reproducible_whatever_the_workspace_held():
    vol = _dev(_ball((37, 41, 43), 13.0, ripple=0.08)[0])
    runs = [_abi(vol, 0.5, ws_fill=p) for p in (None, None, ZERO, ONES)]
    for rc, counts, vb, fb, _ in runs:
        assert rc == 0 and counts == runs[0][1]
        assert vb.tobytes() == runs[0][2].tobytes() and fb.tobytes() == runs[0][3].tobytes()


# ---- blur ---------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("shape", [(9, 8, 7), (20, 3, 31)])
def test_gauss3_blur(shape):
    """Tolerance: twice the fp32-vs-fp64 difference of the numpy blur itself on the same input."""
    from wire_amd import functional
    vol = _noise(shape, 2 + shape[0])
    b64, b32 = iso_ref.blur(vol, 1.0, np.float64), iso_ref.blur(vol, 1.0, np.float32)
    tol = 2.0 * np.abs(b32 - b64).max()
    src = _dev(vol)
    got = functional.gauss3_blur(src, 1.0).cpu().numpy()
    print(f"blur {shape}: |device - fp64| = {np.abs(got - b64).max():.3e}, tolerance {tol:.3e}")
    assert np.abs(got - b64).max() <= tol
    np.testing.assert_array_equal(src.cpu().numpy(), vol)           # the input is not written


# ---- the drivers' calls ---------------------------------------------------------------------------------------
def _occupancy():
    return _ball((18, 17, 16), 5.3, ripple=0.05)[0]


@pytest.mark.parametrize("ext,reader", [(".dae", iso_ref.read_dae), (".obj", iso_ref.read_obj),
                                        (".ply", iso_ref.read_ply)])
def test_march_and_save_plain(tmp_path, ext, reader):
    from wire_amd import functional
    from wire_amd.modules import volutils
    occ = _occupancy()
    for arg in (occ, _dev(occ)):                                     # numpy as in the reference, or a device tensor
        path = str(tmp_path / ("plain" + ext))
        assert volutils.march_and_save(arg, 0.5, path) is None
        v, f = reader(path)
        dv, df = functional.iso_surface(_dev(occ), 0.5)
        np.testing.assert_array_equal(v.astype(np.float32), dv.cpu().numpy())
        np.testing.assert_array_equal(f, df.cpu().numpy())


def test_march_and_save_smoothen(tmp_path):
    """The reference's own call, ``march_and_save(best_img, 0.5, "x.dae", True)``: the saved mesh is the device's
    binarise -> blur -> extract at 0, and equals the fp64 restatement of the same chain wherever no blurred value lies
    within the blur tolerance (test_gauss3_blur's) of 0.  Edges with such an end may differ; they are capped at 1 % of
    the restatement's active edges, and away from them a vertex may move by the blur's error over its edge:
    |dt| <= tol / |b - a| (a and b have opposite signs), on top of the fp32 bound."""
    from wire_amd import functional
    from wire_amd.modules import volutils
    occ = _occupancy()
    before = occ.copy()
    path = str(tmp_path / "x.dae")
    volutils.march_and_save(occ, 0.5, path, True)
    np.testing.assert_array_equal(occ, before)                      # the caller's volume is not binarised
    v, f = iso_ref.read_dae(path)
    binar = (occ >= 0.5).astype(np.float32) - 0.5
    blurred = functional.gauss3_blur(_dev(binar), 1.0)
    dv, df = functional.iso_surface(blurred, 0.0)
    np.testing.assert_array_equal(v.astype(np.float32), dv.cpu().numpy())
    np.testing.assert_array_equal(f, df.cpu().numpy())
    # the restatement
    b64 = iso_ref.blur(binar, 1.0, np.float64)
    tol = 2.0 * np.abs(iso_ref.blur(binar, 1.0, np.float32) - b64).max()
    near = np.abs(b64) <= tol
    rid, rn = iso_ref.vertex_ids(b64.astype(np.float32), 0.0)
    did, dn = iso_ref.vertex_ids(blurred.cpu().numpy(), 0.0)
    touched = np.zeros(rid.shape, bool)
    H, W, T = near.shape
    for d, (di, dj, dk) in enumerate(iso_ref.DIRS):
        touched[:H - di, :W - dj, :T - dk, d] = near[:H - di, :W - dj, :T - dk] | near[di:, dj:, dk:]
    share = (touched & (rid >= 0)).sum() / rn
    print(f"smoothen: {rn} edges, {int(near.sum())} lattice values within {tol:.2e} of 0, share {share:.4f}")
    assert share <= 0.01
    keep = (rid >= 0) & ~touched
    assert (did[keep] >= 0).all() and dn == len(v)
    # fp64 positions of the kept edges against the device's, matched by edge
    ref = np.zeros((rn, 3))
    tb = np.zeros(rn)
    for d, (di, dj, dk) in enumerate(iso_ref.DIRS):
        ii, jj, kk = np.nonzero(rid[..., d] >= 0)
        a, b = b64[ii, jj, kk], b64[ii + di, jj + dj, kk + dk]
        t = (0.0 - a) / (b - a)
        ref[rid[ii, jj, kk, d]] = np.stack([ii + t * di, jj + t * dj, kk + t * dk], 1)
        tb[rid[ii, jj, kk, d]] = tol / np.abs(b - a)
    r_idx, d_idx = rid[keep], did[keep]
    err = np.abs(v[d_idx] - ref[r_idx])
    assert (err <= iso_ref.vertex_bound(ref[r_idx]) + tb[r_idx, None]).all(), err.max()
    if not touched.any():
        rv, rf = iso_ref.extract(b64.astype(np.float32), 0.0)
        if np.array_equal(rid >= 0, did >= 0):
            np.testing.assert_array_equal(f, rf)
    assert iso_ref.edge_census(f)[:2] == (0, 0)


def test_export_mesh(tmp_path):
    from wire_amd.modules import models, utils, volutils
    torch.manual_seed(3)
    model = models.get_INR(nonlin="siren", in_features=3, out_features=1, hidden_features=32, hidden_layers=1).to(DEV)
    res = 12
    coords = utils.get_coords(res, res, res)
    cube = volutils.query_occupancy(coords, res, model, batchsize=700)
    thres = float(np.median(cube))
    path = str(tmp_path / "net.dae")
    out = volutils.export_mesh(coords, res, model, 700, path, thres=thres)
    np.testing.assert_array_equal(out, cube)
    v, f = iso_ref.read_dae(path)
    rv, rf = iso_ref.extract(cube, thres)
    assert len(f) > 0
    np.testing.assert_array_equal(f, rf)
    assert (np.abs(v - rv) <= iso_ref.vertex_bound(rv)).all()


def test_trainer_extract_mesh():
    from wire_amd import functional
    from wire_amd.modules import models
    from wire_amd.trainer import FusedTrainer
    torch.manual_seed(4)
    grid = (12, 10, 8)
    model = models.get_INR(nonlin="siren", in_features=3, out_features=1, hidden_features=32, hidden_layers=1).to(DEV)
    target = torch.from_numpy(_ball(grid, 3.4)[0].reshape(-1, 1))
    tr = FusedTrainer(model, grid, target, keep_rec=True)
    tr.step()
    tr.step()
    thres = float(tr.rec.median())
    v, f = tr.extract_mesh(thres)
    wv, wf = functional.iso_surface(tr.rec.reshape(grid), thres)
    assert len(f) > 0 and torch.equal(v, wv) and torch.equal(f, wf)
    rv, rf = iso_ref.extract(tr.rec.reshape(grid).cpu().numpy(), thres)
    np.testing.assert_array_equal(f.cpu().numpy(), rf)
    # an explicit volume, and the best tracked image once there is one
    v2, f2 = tr.extract_mesh(0.5, volume=target.to(DEV))
    assert torch.equal(f2, functional.iso_surface(target.to(DEV).reshape(grid), 0.5)[1])
    tr.update_best(torch.zeros(1, device=DEV), target.to(DEV).contiguous(), force=True)
    assert torch.equal(tr.extract_mesh(0.5)[1], f2)
    with pytest.raises(ValueError):
        FusedTrainer(model, grid, target).extract_mesh()
    m2 = models.get_INR(nonlin="siren", in_features=2, out_features=1, hidden_features=32, hidden_layers=1).to(DEV)
    with pytest.raises(ValueError, match="3-D"):
        FusedTrainer(m2, (12, 10), torch.zeros(120, 1), keep_rec=True).extract_mesh()
