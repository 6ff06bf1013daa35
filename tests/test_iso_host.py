"""CPU-only checks of the iso-surface feature: the numpy restatement (tests/iso_ref.py) satisfies its own properties, the
library's compile-time winding table equals the midpoint rule, the mesh writers round-trip, and bad arguments are
refused before any device access."""
import numpy as np
import pytest
import torch

import iso_ref
from _util import ROOT  # noqa: F401  (puts the repository on sys.path)


def _ball(n):
    """A sigmoid ball of radius 0.37 n around an off-lattice centre in an n^3 volume."""
    return iso_ref.sphere((n, n, n), (n / 2 - 0.3, n / 2 + 0.2, n / 2 - 0.1), 0.37 * n), 0.37 * n


@pytest.fixture(scope="module")
def balls():
    out = {}
    for n in (12, 24):
        vol, r = _ball(n)
        v, f = iso_ref.extract(vol, 0.5)
        out[n] = (vol, r, v, f)
    return out


def test_restatement_is_closed_oriented_sphere(balls):
    for n, (vol, r, v, f) in balls.items():
        assert (len(v), len(f)) == iso_ref.counts(vol, 0.5)
        dup, missing, und = iso_ref.edge_census(f)
        assert (dup, missing) == (0, 0), n                      # every directed edge once, its reverse once
        assert 2 * und == 3 * len(f)
        assert iso_ref.euler(len(v), f) == 2, n
        assert sorted(set(f.reshape(-1).tolist())) == list(range(len(v)))     # no orphan vertex
        # the normals point away from the centre: inside -> outside on a ball
        c = np.array([n / 2 - 0.3, n / 2 + 0.2, n / 2 - 0.1])
        nrm = np.cross(v[f[:, 1]] - v[f[:, 0]], v[f[:, 2]] - v[f[:, 0]])
        assert (np.einsum("ij,ij->i", nrm, v[f].mean(1) - c) > 0).all(), n


def test_restatement_volume_converges(balls):
    """The signed volume is positive and approaches 4/3 pi r^3.  Bound: the mesh lies within one cell of the true sphere,
    so |V - V0| <= area x 1 cell = 4 pi r^2, i.e. 3 / r of V0 (r in cells) -- and the relative error shrinks when the
    resolution doubles."""
    rel = {}
    for n, (vol, r, v, f) in balls.items():
        v0 = 4.0 / 3.0 * np.pi * r ** 3
        sv = iso_ref.signed_volume(v, f)
        assert sv > 0
        rel[n] = abs(sv - v0) / v0
        assert rel[n] <= 3.0 / r, (n, rel[n])
    assert rel[24] < rel[12], rel


def _decode(entry):
    return [tuple(iso_ref.EDGES[(entry >> (2 + 9 * r + 3 * c)) & 7] for c in range(3)) for r in range(entry & 3)]


def test_library_winding_table_is_the_midpoint_rule():
    from wire_amd import _lib
    L = _lib.lib()
    for t in range(6):
        for m in range(16):
            e = L.wire_iso_tet_case(t, m)
            assert e >= 0
            assert _decode(e) == iso_ref.WINDING[t][m], (t, m)
            assert len(iso_ref.WINDING[t][m]) == (0 if m in (0, 15) else 2 if bin(m).count("1") == 2 else 1)
    assert L.wire_iso_tet_case(6, 1) < 0 and L.wire_iso_tet_case(0, 16) < 0


def test_winding_holds_where_thres_equals_data(balls):
    """A binarised field cut at 1.0: every crossing sits ON a lattice point, positions coincide and a geometric winding
    rule has nothing to go by.  The table's winding is still consistent and the surface closed."""
    vol = (balls[12][0] >= 0.5).astype(np.float32)
    v, f = iso_ref.extract(vol, 1.0)
    assert len(f) > 0 and iso_ref.edge_census(f)[:2] == (0, 0) and iso_ref.euler(len(v), f) == 2
    assert len(np.unique(v, axis=0)) < len(v)                   # vertices do coincide
    assert iso_ref.signed_volume(v, f) > 0
    # and on a random field with data equal to the threshold, padded so that the surface stays closed
    rng = np.random.default_rng(5)
    r = np.zeros((7, 8, 6), np.float32)
    r[1:-1, 1:-1, 1:-1] = rng.integers(0, 3, (5, 6, 4)).astype(np.float32) / 2
    v, f = iso_ref.extract(r, 0.5)
    assert len(f) > 0 and iso_ref.edge_census(f)[:2] == (0, 0)


@pytest.mark.parametrize("ext,reader", [(".obj", iso_ref.read_obj), (".ply", iso_ref.read_ply),
                                        (".dae", iso_ref.read_dae)])
def test_writers_round_trip(tmp_path, balls, ext, reader):
    from wire_amd.modules import volutils
    _, _, v, f = balls[12]
    v32 = v.astype(np.float32)
    path = str(tmp_path / ("mesh" + ext))
    volutils.save_mesh(torch.from_numpy(v32), f.astype(np.int32), path)
    v2, f2 = reader(path)
    assert v2.shape == v32.shape and f2.shape == f.shape
    np.testing.assert_array_equal(v2.astype(np.float32), v32)   # %.9g and binary fp32 both round-trip
    np.testing.assert_array_equal(f2[0], f[0])
    np.testing.assert_array_equal(f2[-1], f[-1])
    np.testing.assert_array_equal(f2, f)
    with pytest.raises(ValueError):
        volutils.save_mesh(v32, f, str(tmp_path / "mesh.stl"))


def test_writers_accept_an_empty_mesh(tmp_path):
    from wire_amd.modules import volutils
    for ext, reader in ((".obj", iso_ref.read_obj), (".ply", iso_ref.read_ply), (".dae", iso_ref.read_dae)):
        path = str(tmp_path / ("empty" + ext))
        volutils.save_mesh(np.zeros((0, 3), np.float32), np.zeros((0, 3), np.int32), path)
        v, f = reader(path)
        assert len(v) == 0 and len(f) == 0


def test_argument_errors():
    from wire_amd import _lib, functional
    from wire_amd.modules import volutils
    L = _lib.lib()
    with pytest.raises(ValueError):
        functional.iso_surface(torch.zeros(4, 4), 0.5)                       # rank
    with pytest.raises(ValueError):
        functional.iso_surface(torch.zeros(4, 1, 4), 0.5)                    # a side < 2
    with pytest.raises(_lib.WireHipError):
        functional.iso_surface(torch.zeros(4, 4, 4), 0.5)                    # a CPU tensor
    with pytest.raises(_lib.WireHipError):
        functional.gauss3_blur(torch.zeros(4, 4, 4), 1.0)
    with pytest.raises(ValueError):
        volutils.march_and_save(np.zeros((4, 4), np.float32), 0.5, "x.obj")
    with pytest.raises(_lib.WireHipError):
        volutils.march_and_save(torch.zeros(4, 4, 4), 0.5, "x.obj")
    # the C ABI refuses before any HIP call
    assert L.wire_iso_ws_bytes(1, 5, 5) == -1 and L.wire_iso_ws_bytes(5, 5, 1) == -1
    assert L.wire_iso_ws_bytes(1024, 1024, 257) == -1                        # more than 2^28 points
    assert L.wire_iso_ws_bytes(512, 512, 512) > 9 * 512 ** 3
    assert L.wire_iso_ws_bytes(512, 512, 512) < 9.1 * 512 ** 3
    assert L.wire_iso_count(None, 64, 5, 1, 5, 0.5, 64, 64) == -1
    assert L.wire_iso_count(None, 64, 5, 5, 5, float("nan"), 64, 64) == -1
    assert L.wire_iso_emit(None, 64, 5, 5, 5, 0.5, None, 64, 1, 64, 1) == -1
    assert L.wire_gauss3_blur(None, 64, 4, 4, 4, 0.0, 128, 192) == -1
    assert L.wire_gauss3_blur(None, 64, 4, 4, 4, 9.0, 128, 192) == -1
    assert L.wire_gauss3_blur(None, 64, 4, 4, 4, 1.0, 64, 192) == -1          # in == tmp


def test_blur_restatement_preserves_constants_and_mass():
    w, R = iso_ref.blur_weights(1.0)
    assert R == 4 and len(w) == 9 and abs(float(w.astype(np.float64).sum()) - 1) < 1e-7
    x = np.full((5, 4, 6), 0.25, np.float32)
    np.testing.assert_allclose(iso_ref.blur(x, 1.0, np.float64), 0.25, atol=1e-7)
