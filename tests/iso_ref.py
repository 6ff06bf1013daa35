"""A plain numpy / fp64 restatement of the iso-surface rules (marching tetrahedra on the Kuhn split), its topology checks
and the separable Gaussian blur -- what tests/test_iso_host.py and tests/test_gpu_iso.py compare the library against.

Rules (vol[H][W][T] float32, lattice point (i, j, k)):
  inside        vol >= thres; NaN is outside
  tetrahedra    per cell and permutation (a, b, c) of the axes in lexicographic order:
                v0 = corner 000, v1 = v0 + e_a, v2 = v1 + e_b, v3 = corner 111
  edges         directions DIRS; an edge belongs to its lower end p and is active iff its ends differ in `inside` and
                the far end lies in the volume
  vertices      one per active edge at p + t d, t = (thres - vol[p]) / (vol[p + d] - vol[p]); ids ascend by
                (linear index of p, direction)
  triangles     1 or 3 inside: (ox, oy, oz) around the odd corner o, x < y < z the others; 2 inside: the quad
                (ac, ad, bd, bc), a < b inside, c < d outside, split (q0, q1, q2), (q0, q2, q3); ordered by
                (cell, tetrahedron, triangle)
  winding       as if every crossing sat at its edge's midpoint, normal from the inside to the outside corners; a wrongly
                wound triangle has its last two corners swapped.  A function of (permutation, inside mask): WINDING.
Everything here loops in Python over cells: it is meant for tiny shapes.  The counts alone are vectorised.
"""
import itertools

import numpy as np

DIRS = [(1, 0, 0), (0, 1, 0), (0, 0, 1), (1, 1, 0), (1, 0, 1), (0, 1, 1), (1, 1, 1)]
PERMS = list(itertools.permutations(range(3)))          # lexicographic
EDGES = [(0, 1), (0, 2), (0, 3), (1, 2), (1, 3), (2, 3)]


def tet_corners(perm):
    """The four corners (offsets in the cell) of the tetrahedron of a permutation."""
    a, b, _ = perm
    v0 = np.zeros(3, int)
    v1 = v0.copy(); v1[a] += 1
    v2 = v1.copy(); v2[b] += 1
    return [v0, v1, v2, np.ones(3, int)]


def _unwound(mask):
    """Triangles of a tetrahedron whose corner n is inside iff bit n of mask, as triples of edges (m, n), m < n."""
    ins = [n for n in range(4) if (mask >> n) & 1]
    outs = [n for n in range(4) if not (mask >> n) & 1]
    e = lambda m, n: (min(m, n), max(m, n))
    if len(ins) in (0, 4):
        return []
    if len(ins) == 2:
        (a, b), (c, d) = ins, outs
        q = [e(a, c), e(a, d), e(b, d), e(b, c)]
        return [(q[0], q[1], q[2]), (q[0], q[2], q[3])]
    o = ins[0] if len(ins) == 1 else outs[0]
    return [tuple(e(o, n) for n in range(4) if n != o)]


def _midpoint_flip(perm, mask, tri):
    """True when the triangle, its corners at the midpoints of its edges, has its normal pointing from the outside
    corners to the inside ones."""
    v = [c.astype(np.float64) for c in tet_corners(perm)]
    p = [(v[m] + v[n]) / 2 for m, n in tri]
    ins = np.mean([v[n] for n in range(4) if (mask >> n) & 1], axis=0)
    outs = np.mean([v[n] for n in range(4) if not (mask >> n) & 1], axis=0)
    return float(np.dot(np.cross(p[1] - p[0], p[2] - p[0]), outs - ins)) < 0


def case_triangles(t, mask):
    """The wound triangles of tetrahedron t (index into PERMS) for an inside mask."""
    out = []
    for tri in _unwound(mask):
        out.append((tri[0], tri[2], tri[1]) if _midpoint_flip(PERMS[t], mask, tri) else tri)
    return out


WINDING = [[case_triangles(t, m) for m in range(16)] for t in range(6)]        # the 6 x 16 table


def inside_of(vol, thres):
    with np.errstate(invalid="ignore"):
        return np.asarray(vol, np.float32) >= np.float32(thres)


def vertex_ids(vol, thres):
    """(vid [H, W, T, 7] with -1 at an inactive edge, number of vertices)."""
    ins = inside_of(vol, thres)
    H, W, T = ins.shape
    act = np.zeros((H, W, T, 7), bool)
    for d, (di, dj, dk) in enumerate(DIRS):
        act[:H - di, :W - dj, :T - dk, d] = ins[:H - di, :W - dj, :T - dk] != ins[di:, dj:, dk:]
    flat = act.reshape(-1)
    ids = np.cumsum(flat) - 1
    return np.where(flat, ids, -1).reshape(H, W, T, 7), int(flat.sum())


def cell_tri_counts(vol, thres):
    """Triangles per cell, [H-1, W-1, T-1] (vectorised)."""
    ins = inside_of(vol, thres)
    H, W, T = ins.shape
    corner = lambda c: ins[c[0]:H - 1 + c[0], c[1]:W - 1 + c[1], c[2]:T - 1 + c[2]].astype(int)
    n = np.zeros((H - 1, W - 1, T - 1), int)
    for perm in PERMS:
        k = sum(corner(c) for c in tet_corners(perm))
        n += np.where((k == 1) | (k == 3), 1, 0) + np.where(k == 2, 2, 0)
    return n


def counts(vol, thres):
    return vertex_ids(vol, thres)[1], int(cell_tri_counts(vol, thres).sum())


def cell_faces(ins, vid, i, j, k):
    """The faces of one cell, in order."""
    out = []
    base = np.array([i, j, k])
    for t, perm in enumerate(PERMS):
        cs = [base + c for c in tet_corners(perm)]
        mask = sum(int(ins[tuple(c)]) << n for n, c in enumerate(cs))
        for tri in WINDING[t][mask]:
            f = []
            for m, n in tri:
                d = DIRS.index(tuple(cs[n] - cs[m]))
                f.append(int(vid[cs[m][0], cs[m][1], cs[m][2], d]))
            assert min(f) >= 0
            out.append(f)
    return out


def vertices(vol, thres):
    """[V, 3] float64 positions in index units, t from the float32 data in fp64."""
    vol = np.asarray(vol, np.float32)
    vid, nv = vertex_ids(vol, thres)
    th = np.float64(np.float32(thres))
    out = np.zeros((nv, 3), np.float64)
    v64 = vol.astype(np.float64)
    for d, (di, dj, dk) in enumerate(DIRS):
        ii, jj, kk = np.nonzero(vid[..., d] >= 0)
        a, b = v64[ii, jj, kk], v64[ii + di, jj + dj, kk + dk]
        with np.errstate(invalid="ignore", divide="ignore"):
            t = (th - a) / (b - a)
        out[vid[ii, jj, kk, d]] = np.stack([ii + t * di, jj + t * dj, kk + t * dk], 1)
    return out


def extract(vol, thres):
    """(vertices [V, 3] float64, faces [F, 3] int64) of the whole volume."""
    vol = np.asarray(vol, np.float32)
    ins = inside_of(vol, thres)
    vid, _ = vertex_ids(vol, thres)
    H, W, T = vol.shape
    faces = []
    for i in range(H - 1):
        for j in range(W - 1):
            for k in range(T - 1):
                c = ins[i:i + 2, j:j + 2, k:k + 2]
                if c.all() or not c.any():
                    continue
                faces += cell_faces(ins, vid, i, j, k)
    return vertices(vol, thres), np.array(faces, np.int64).reshape(-1, 3)


def vertex_bound(verts64):
    """|device - fp64| allowed per coordinate: 4 * 2^-24 * (1 + coordinate) -- three fp32 roundings in t, t <= 1, and one
    in p + t d."""
    return 4.0 * 2.0 ** -24 * (1.0 + np.abs(verts64))


# ---- topology -------------------------------------------------------------------------------------------------------
def edge_census(faces):
    """(directed edges that occur more than once, directed edges whose reverse is missing, undirected edges).  A closed,
    consistently oriented surface gives (0, 0, E)."""
    f = np.asarray(faces, np.int64).reshape(-1, 3)
    a = np.concatenate([f[:, 0], f[:, 1], f[:, 2]])
    b = np.concatenate([f[:, 1], f[:, 2], f[:, 0]])
    n = int(max(a.max(), b.max())) + 1 if len(a) else 1
    key, rev = a * n + b, b * n + a
    uniq, cnt = np.unique(key, return_counts=True)
    dup = int((cnt > 1).sum())
    missing = int((~np.isin(rev, uniq)).sum())
    und = len(np.unique(np.minimum(a, b) * n + np.maximum(a, b)))
    return dup, missing, und


def euler(nverts, faces):
    return nverts - edge_census(faces)[2] + len(faces)


def signed_volume(verts, faces):
    v = np.asarray(verts, np.float64)
    f = np.asarray(faces, np.int64)
    return float(np.einsum("ij,ij->i", v[f[:, 0]], np.cross(v[f[:, 1]], v[f[:, 2]])).sum() / 6.0)


# ---- fields ---------------------------------------------------------------------------------------------------------
def sphere(shape, centre, radius, sharp=1.5):
    """A sigmoid ball: > 0.5 inside."""
    g = np.meshgrid(*[np.arange(n, dtype=np.float64) for n in shape], indexing="ij")
    r = np.sqrt(sum((x - c) ** 2 for x, c in zip(g, centre)))
    return (1.0 / (1.0 + np.exp((r - radius) * sharp))).astype(np.float32)


# ---- blur -----------------------------------------------------------------------------------------------------------
def blur_weights(sigma):
    R = int(4.0 * sigma + 0.5)
    x = np.arange(-R, R + 1, dtype=np.float64)
    w = np.exp(-0.5 * x * x / (sigma * sigma))
    return (w / w.sum()).astype(np.float32), R


def blur(vol, sigma, dtype):
    """Separable Gaussian, truncated at 4 sigma, edge values replicated: axis 2, then 1, then 0; per axis the taps added
    from -R to +R in ``dtype`` (float32: product and sum each rounded once), with the float32 weights."""
    w, R = blur_weights(sigma)
    w = w.astype(dtype)
    x = np.asarray(vol, dtype)
    for ax in (2, 1, 0):
        n = x.shape[ax]
        acc = np.zeros_like(x)
        for t in range(-R, R + 1):
            idx = np.clip(np.arange(n) + t, 0, n - 1)
            acc = (acc + w[t + R] * np.take(x, idx, axis=ax)).astype(dtype)
        x = acc
    return x


# ---- mesh files -----------------------------------------------------------------------------------------------------
def read_obj(path):
    v, f = [], []
    for line in open(path):
        p = line.split()
        if p and p[0] == "v":
            v.append([float(s) for s in p[1:4]])
        elif p and p[0] == "f":
            f.append([int(s.split("/")[0]) - 1 for s in p[1:4]])
    return np.array(v, np.float64).reshape(-1, 3), np.array(f, np.int64).reshape(-1, 3)


def read_ply(path):
    data = open(path, "rb").read()
    head, body = data.split(b"end_header\n", 1)
    lines = head.decode("ascii").split("\n")
    assert lines[0] == "ply" and "format binary_little_endian 1.0" in lines
    nv = next(int(l.split()[2]) for l in lines if l.startswith("element vertex"))
    nf = next(int(l.split()[2]) for l in lines if l.startswith("element face"))
    v = np.frombuffer(body, "<f4", 3 * nv).reshape(nv, 3)
    rec = np.frombuffer(body, np.dtype([("n", "u1"), ("i", "<i4", 3)]), nf, 12 * nv)
    assert len(body) == 12 * nv + 13 * nf and (rec["n"] == 3).all()
    return v.astype(np.float64), rec["i"].astype(np.int64).reshape(-1, 3)


def read_dae(path):
    import xml.etree.ElementTree as ET
    ns = {"c": "http://www.collada.org/2005/11/COLLADASchema"}
    root = ET.parse(path).getroot()
    assert root.tag == "{%s}COLLADA" % ns["c"] and root.get("version") == "1.4.1"
    geos = root.findall("c:library_geometries/c:geometry", ns)
    assert len(geos) == 1
    mesh = geos[0].find("c:mesh", ns)
    arrs = mesh.findall("c:source/c:float_array", ns)
    tris = mesh.findall("c:triangles", ns)
    assert len(arrs) == 1 and len(tris) == 1
    v = np.array((arrs[0].text or "").split(), np.float64).reshape(-1, 3)
    assert int(arrs[0].get("count")) == v.size
    f = np.array((tris[0].find("c:p", ns).text or "").split(), np.int64).reshape(-1, 3)
    assert int(tris[0].get("count")) == len(f)
    # the scene must instantiate the geometry, or a reader shows nothing
    inst = root.find("c:library_visual_scenes/c:visual_scene/c:node/c:instance_geometry", ns)
    assert inst is not None and inst.get("url") == "#" + geos[0].get("id")
    return v, f
