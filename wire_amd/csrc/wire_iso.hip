// wire_iso.hip -- the iso-surface {vol >= thres} of a volume vol[H][W][T] as an indexed triangle mesh, on the device
// (what the reference's volutils.march_and_save / export_mesh hand to PyMCubes, modules/volutils.py:94-142), and the
// separable Gaussian blur that march_and_save's `smoothen` uses here.
//
// ALGORITHM: marching tetrahedra on the six-tetrahedron Kuhn (Freudenthal) split of every cell -- no case table to
// carry, the same split in every cell (neighbours agree on their shared face diagonals), closed and consistently
// oriented by construction.
//   inside:     vol >= thres (NaN is outside)
//   tetrahedra: cell (i, j, k), the permutations (a, b, c) of the axes in lexicographic order:
//               v0 = corner 000, v1 = v0 + e_a, v2 = v1 + e_b, v3 = corner 111
//   edges:      7 directions d0 .. d6 = (1,0,0) (0,1,0) (0,0,1) (1,1,0) (1,0,1) (0,1,1) (1,1,1); an edge belongs to its
//               lower end p and is active iff its ends differ and the far end lies in the volume
//   vertices:   one per active edge, at p + t d with t = (thres - a) / (b - a) in fp32 (three roundings; one more in
//               p + t), in index units; ids ascend by (linear index of p, d): welded and ordered by construction
//   triangles:  1 or 3 corners inside: one triangle (ox, oy, oz) around the odd corner o, x < y < z the others;
//               2 inside: the quad (ac, ad, bd, bc), a < b inside, c < d outside, split (q0 q1 q2) (q0 q2 q3);
//               ordered by (cell, tetrahedron, triangle)
//   winding:    as if every crossing sat at its edge's midpoint, the normal from the inside to the outside corners --
//               a function of (permutation, inside mask) alone: ISO_CASES, 6 x 16, built at compile time by
//               iso_case() from that very rule in integer arithmetic.  A wrongly wound triangle has its last two
//               corners swapped.  Never taken from the interpolated positions, which coincide when thres is a data value.
//
// WORKSPACE (wire_iso_ws_bytes; N = H W T lattice points, 9 bytes per point plus the scan's sums):
//   [0, 256)   two int64: the vertex and the face count
//   mask[N]    uint8: bit d = edge d of the point is active, bit 7 = the point is a cell's corner 000 (all seven
//              neighbours lie in the volume).  A cell's corner signs relative to its corner 000 are that corner's
//              seven bits, so the cell's triangle count is a function of ONE byte, and the emit pass reads the volume
//              at a cut cell's corner 000 alone to know which side is inside
//   voff[N]    uint32: exclusive scan of popcount(mask & 0x7f); vertex id of edge (p, d) =
//              voff[p] + popcount(mask[p] & ((1 << d) - 1)) -- no edge -> vertex map (7 x 4 bytes per point) is kept
//   toff[N]    uint32: exclusive scan of the cells' triangle counts (0 at a point that is no cell's corner 000)
//   the scan's sums (wire_scan.h)
//
// PASSES: classify (one thread per FOUR consecutive points of a row: the five values it needs of each of the four
// rows (i, j), (i+1, j), (i, j+1), (i+1, j+1), plain loads through L1 / L2 as in wire_tv.hip, one 4-byte store),
// two scans (wire_scan.h: reduce-then-scan, separate launches, nothing waits on another workgroup), then emit: one
// thread per four cells writes their <= 12 faces each at toff, one thread per four points their <= 7 vertices each at voff.  Counting and writing
// read the same mask, so they agree whatever the data (NaN data can give NaN vertices, never another count).  No
// atomics: the same call gives the same bits, whatever the workspace held before.
//
// The entry points of the C ABI (include/wire_hip.h) are at the end of this file.
#include "wire_dev.h"
#include "wire_plan.h"
#include "wire_scan.h"

#define ISO_MAX_POINTS (1ll << 28)

// ---- the combinatorics, for the host and the device ----------------------------------------------------------------
// corner code: bit 0 = +1 along axis 0 (i), bit 1 = axis 1 (j), bit 2 = axis 2 (k); direction d <-> codes 1 2 4 3 5 6 7
__host__ __device__ constexpr int iso_dir_code(int d) { return d == 0 ? 1 : d == 1 ? 2 : d == 2 ? 4 : d == 3 ? 3 : d == 4 ? 5 : d == 5 ? 6 : 7; }
__host__ __device__ constexpr int iso_code_dir(int c) { return c == 1 ? 0 : c == 2 ? 1 : c == 4 ? 2 : c == 3 ? 3 : c == 5 ? 4 : c == 6 ? 5 : 6; }
// the axes (a, b) of permutation t in lexicographic order: 012 021 102 120 201 210
__host__ __device__ constexpr int iso_perm_a(int t) { return t >> 1; }
__host__ __device__ constexpr int iso_perm_b(int t) {
  return (t & 1) ? (iso_perm_a(t) == 2 ? 1 : 2) : (iso_perm_a(t) == 0 ? 1 : 0);
}
// corner code of vertex n of tetrahedron t
__host__ __device__ constexpr int iso_tet_corner(int t, int n) {
  return n == 0 ? 0 : n == 1 ? (1 << iso_perm_a(t)) : n == 2 ? ((1 << iso_perm_a(t)) | (1 << iso_perm_b(t))) : 7;
}
// edge (m, n), m < n, of a tetrahedron -> 0 .. 5: 01 02 03 12 13 23
__host__ __device__ constexpr int iso_edge_index(int m, int n) { return m == 0 ? n - 1 : m == 1 ? n + 1 : 5; }
__host__ __device__ constexpr int iso_edge_lo(int e) { return e < 3 ? 0 : e < 5 ? 1 : 2; }
__host__ __device__ constexpr int iso_edge_hi(int e) { return e < 3 ? e + 1 : e < 5 ? e - 1 : 3; }

// One entry of ISO_CASES: bits 0-1 = the number of triangles, then three bits per corner (an edge index 0 .. 5), the
// corners of triangle 0 at bits 2, 5, 8 and of triangle 1 at bits 11, 14, 17 -- already wound.
__host__ __device__ constexpr unsigned iso_case(int t, int mask) {
  int in[4] = {0, 0, 0, 0}, out[4] = {0, 0, 0, 0}, ni = 0, no = 0;
  for (int n = 0; n < 4; ++n) {
    if ((mask >> n) & 1) in[ni++] = n; else out[no++] = n;
  }
  if (ni == 0 || ni == 4) return 0u;
  int q[4] = {0, 0, 0, 0}, ntri = 1;
  if (ni == 2) {
    const int a = in[0], b = in[1], c = out[0], d = out[1];
    const int lo_ac = a < c ? a : c, hi_ac = a < c ? c : a, lo_ad = a < d ? a : d, hi_ad = a < d ? d : a;
    const int lo_bd = b < d ? b : d, hi_bd = b < d ? d : b, lo_bc = b < c ? b : c, hi_bc = b < c ? c : b;
    q[0] = iso_edge_index(lo_ac, hi_ac); q[1] = iso_edge_index(lo_ad, hi_ad);
    q[2] = iso_edge_index(lo_bd, hi_bd); q[3] = iso_edge_index(lo_bc, hi_bc);
    ntri = 2;
  } else {
    const int o = ni == 1 ? in[0] : out[0];
    int r = 0;
    for (int n = 0; n < 4; ++n)
      if (n != o) q[r++] = iso_edge_index(n < o ? n : o, n < o ? o : n);
  }
  // the midpoint rule in doubled integer coordinates: a midpoint is the sum of its edge's two corners
  int P[4][3] = {};
  for (int r = 0; r < (ni == 2 ? 4 : 3); ++r) {
    const int c0 = iso_tet_corner(t, iso_edge_lo(q[r])), c1 = iso_tet_corner(t, iso_edge_hi(q[r]));
    for (int x = 0; x < 3; ++x) P[r][x] = ((c0 >> x) & 1) + ((c1 >> x) & 1);
  }
  int D[3] = {0, 0, 0};                              // no * (sum of the outside corners) * ni - ... : inside -> outside
  for (int x = 0; x < 3; ++x) {
    int so = 0, si = 0;
    for (int n = 0; n < no; ++n) so += (iso_tet_corner(t, out[n]) >> x) & 1;
    for (int n = 0; n < ni; ++n) si += (iso_tet_corner(t, in[n]) >> x) & 1;
    D[x] = so * ni - si * no;
  }
  const int u[3] = {P[1][0] - P[0][0], P[1][1] - P[0][1], P[1][2] - P[0][2]};
  const int v[3] = {P[2][0] - P[0][0], P[2][1] - P[0][1], P[2][2] - P[0][2]};
  const int dot = (u[1] * v[2] - u[2] * v[1]) * D[0] + (u[2] * v[0] - u[0] * v[2]) * D[1] +
                  (u[0] * v[1] - u[1] * v[0]) * D[2];
  const bool flip = dot < 0;
  unsigned e = (unsigned)ntri;
  const int t0[3] = {q[0], flip ? q[2] : q[1], flip ? q[1] : q[2]};
  const int t1[3] = {q[0], flip ? q[3] : q[2], flip ? q[2] : q[3]};
  for (int r = 0; r < 3; ++r) e |= (unsigned)t0[r] << (2 + 3 * r);
  if (ntri == 2)
    for (int r = 0; r < 3; ++r) e |= (unsigned)t1[r] << (11 + 3 * r);
  return e;
}
struct IsoCases { unsigned e[6][16]; };
constexpr IsoCases iso_make_cases() {
  IsoCases c = {};
  for (int t = 0; t < 6; ++t)
    for (int m = 0; m < 16; ++m) c.e[t][m] = iso_case(t, m);
  return c;
}
static constexpr IsoCases ISO_CASES_HOST = iso_make_cases();
__constant__ IsoCases ISO_CASES = iso_make_cases();

// triangles of a cell from the seven bits of its corner 000 (corner signs relative to that corner): a tetrahedron
// with 1 or 3 of v1 v2 v3 differing from v0 is cut 1 : 3 (one triangle), with 2 differing 2 : 2 (two)
__host__ __device__ inline unsigned iso_cell_tris(unsigned m) {
  unsigned n = 0;
#pragma unroll
  for (int t = 0; t < 6; ++t) {
    const unsigned k = ((m >> iso_code_dir(iso_tet_corner(t, 1))) & 1u) + ((m >> iso_code_dir(iso_tet_corner(t, 2))) & 1u) +
                       ((m >> 6) & 1u);
    n += k == 0 ? 0u : k == 2 ? 2u : 1u;
  }
  return n;
}

struct IsoGeom {
  int H, W, T, N;          // N = H W T <= 2^28
  int sH, sW;              // floats between two points along axis 0 (W T) and axis 1 (T)
};
WIRE_DEVINL void iso_locate(const IsoGeom& g, int p, int& i, int& j, int& k) {
  const int r = p / g.T;
  k = p - r * g.T;
  i = r / g.W;
  j = r - i * g.W;
}
WIRE_DEVINL int iso_code_off(const IsoGeom& g, int c) { return (c & 1) * g.sH + ((c >> 1) & 1) * g.sW + ((c >> 2) & 1); }

// ---- the scans' inputs: counts derived from the mask bytes ---------------------------------------------------------
struct IsoVertCount {
  const uint8_t* mask;
  __device__ __forceinline__ void load4(long long base, long long n, unsigned (&v)[4]) const {
    if (base + 4 <= n) {
      const unsigned q = *reinterpret_cast<const unsigned*>(mask + base);
#pragma unroll
      for (int r = 0; r < 4; ++r) v[r] = (unsigned)__builtin_popcount((q >> (8 * r)) & 0x7fu);
    } else {
#pragma unroll
      for (int r = 0; r < 4; ++r) v[r] = base + r < n ? (unsigned)__builtin_popcount(mask[base + r] & 0x7fu) : 0u;
    }
  }
};
struct IsoTriCount {
  const uint8_t* mask;
  __device__ __forceinline__ void load4(long long base, long long n, unsigned (&v)[4]) const {
    unsigned q = 0u;
    if (base + 4 <= n) {
      q = *reinterpret_cast<const unsigned*>(mask + base);
    } else {
#pragma unroll
      for (int r = 0; r < 4; ++r) q |= base + r < n ? (unsigned)mask[base + r] << (8 * r) : 0u;
    }
#pragma unroll
    for (int r = 0; r < 4; ++r) {
      const unsigned m = (q >> (8 * r)) & 0xffu;
      v[r] = (m & 0x80u) ? iso_cell_tris(m) : 0u;
    }
  }
};

// ---- pass 1: one mask byte per lattice point ------------------------------------------------------------------------
// the byte of a point: in0 = the point is inside, in[c] = its neighbour at corner code c is (read where room has c's bits)
WIRE_DEVINL unsigned iso_mask_of(bool in0, const bool (&in)[8], int room) {
  unsigned m = room == 7 ? 0x80u : 0u;
#pragma unroll
  for (int d = 0; d < 7; ++d) {
    const int c = iso_dir_code(d);
    if ((room & c) == c && in[c] != in0) m |= 1u << d;
  }
  return m;
}

// One thread per four consecutive points p0 .. p0 + 3 (p0 a multiple of 4; mask is 4-byte aligned).  When the four lie
// in one row of T, the thread loads five consecutive values of each of the rows (i, j), (i+1, j), (i, j+1), (i+1, j+1)
// -- as one 16-byte load and one more value where vec4 says that every row starts on a 16-byte boundary -- and writes
// the four bytes as one word; four points that straddle rows (T no multiple of 4) take their eight values each.
__global__ __launch_bounds__(256) void iso_classify_kernel(const float* __restrict__ vol, IsoGeom g, float thres,
                                                           int vec4, uint8_t* __restrict__ mask) {
  const int p0 = (blockIdx.x * 256 + threadIdx.x) * 4;
  if (p0 >= g.N) return;
  int i, j, k;
  iso_locate(g, p0, i, j, k);
  if (k + 4 <= g.T) {
    const int ri = i + 1 < g.H ? 1 : 0, rj = j + 1 < g.W ? 2 : 0;
    const bool tail = k + 4 < g.T;                       // the fifth value lies in the row
    bool in[4][5];
#pragma unroll
    for (int r = 0; r < 4; ++r) {
      const bool have = ((ri | rj) & r) == r;            // row r = corner code r of (i, j)
      const float* row = vol + p0 + (r & 1) * g.sH + ((r >> 1) & 1) * g.sW;
      float a[5] = {0.f, 0.f, 0.f, 0.f, 0.f};
      if (have) {
        if (vec4) {
          const f32x4 q = *reinterpret_cast<const f32x4*>(row);
          a[0] = q[0]; a[1] = q[1]; a[2] = q[2]; a[3] = q[3];
        } else {
          a[0] = row[0]; a[1] = row[1]; a[2] = row[2]; a[3] = row[3];
        }
        if (tail) a[4] = row[4];
      }
#pragma unroll
      for (int x = 0; x < 5; ++x) in[r][x] = a[x] >= thres;
    }
    unsigned word = 0u;
#pragma unroll
    for (int e = 0; e < 4; ++e) {
      bool nb[8];
#pragma unroll
      for (int c = 1; c < 8; ++c) nb[c] = in[c & 3][e + (c >> 2)];
      nb[0] = false;
      const int room = ri | rj | (e < 3 || tail ? 4 : 0);
      word |= iso_mask_of(in[0][e], nb, room) << (8 * e);
    }
    *reinterpret_cast<unsigned*>(mask + p0) = word;
    return;
  }
  for (int p = p0; p < p0 + 4 && p < g.N; ++p) {
    iso_locate(g, p, i, j, k);
    const int room = (i + 1 < g.H ? 1 : 0) | (j + 1 < g.W ? 2 : 0) | (k + 1 < g.T ? 4 : 0);
    bool nb[8];
    nb[0] = false;
#pragma unroll
    for (int c = 1; c < 8; ++c) nb[c] = (room & c) == c ? vol[p + iso_code_off(g, c)] >= thres : false;
    mask[p] = (uint8_t)iso_mask_of(vol[p] >= thres, nb, room);
  }
}

// ---- pass 2 ----------------------------------------------------------------------------------------------------------
WIRE_DEVINL int iso_sel6(const int (&e)[6], unsigned idx) {
  return idx == 0 ? e[0] : idx == 1 ? e[1] : idx == 2 ? e[2] : idx == 3 ? e[3] : idx == 4 ? e[4] : e[5];
}

// the faces of the cell whose corner 000 is p (m0 = its mask byte: a cell, and cut)
WIRE_DEVINL void iso_cell_faces(const float* __restrict__ vol, const IsoGeom& g, float thres,
                                const uint8_t* __restrict__ mask, const unsigned* __restrict__ voff,
                                const unsigned* __restrict__ toff, long long cap_f, int32_t* __restrict__ faces, int p,
                                unsigned m0) {
  // the seven corners that own edges of this cell: their masks and first vertex ids
  unsigned mc[7], vc[7];
  mc[0] = m0;
  vc[0] = voff[p];
#pragma unroll
  for (int c = 1; c < 7; ++c) {
    const int q = p + iso_code_off(g, c);
    mc[c] = mask[q];
    vc[c] = voff[q];
  }
  const unsigned in000 = vol[p] >= thres ? 1u : 0u;
  unsigned long long out = toff[p];
#pragma unroll
  for (int t = 0; t < 6; ++t) {
    const int c1 = iso_tet_corner(t, 1), c2 = iso_tet_corner(t, 2);
    const unsigned m4 = (in000 | ((in000 ^ ((m0 >> iso_code_dir(c1)) & 1u)) << 1) |
                         ((in000 ^ ((m0 >> iso_code_dir(c2)) & 1u)) << 2) | ((in000 ^ ((m0 >> 6) & 1u)) << 3));
    const unsigned ent = ISO_CASES.e[t][m4];
    const unsigned ntri = ent & 3u;
    if (ntri == 0u) continue;
    int e[6];
#pragma unroll
    for (int x = 0; x < 6; ++x) {
      const int lo = iso_tet_corner(t, iso_edge_lo(x)), hi = iso_tet_corner(t, iso_edge_hi(x));
      const int d = iso_code_dir(lo ^ hi);
      e[x] = (int)(vc[lo] + (unsigned)__builtin_popcount(mc[lo] & ((1u << d) - 1u)));
    }
    for (unsigned r = 0; r < ntri; ++r, ++out) {
      const unsigned b = ent >> (2 + 9 * r);
      if (out < (unsigned long long)cap_f) {
        int32_t* f = faces + 3 * out;
        f[0] = iso_sel6(e, b & 7u);
        f[1] = iso_sel6(e, (b >> 3) & 7u);
        f[2] = iso_sel6(e, (b >> 6) & 7u);
      }
    }
  }
}

// Both emit kernels: one thread per four consecutive points (one 32-bit load of their mask bytes; most words are 0).
// totals: the two counts in the workspace's head.  Nothing is written when either exceeds its capacity; every store
// is guarded by its capacity besides, so that a workspace that was overwritten cannot send one out of range.
__global__ __launch_bounds__(256) void iso_faces_kernel(const float* __restrict__ vol, IsoGeom g, float thres,
                                                        const uint8_t* __restrict__ mask,
                                                        const unsigned* __restrict__ voff,
                                                        const unsigned* __restrict__ toff,
                                                        const int64_t* __restrict__ totals, long long cap_v,
                                                        long long cap_f, int32_t* __restrict__ faces) {
  if (totals[0] > cap_v || totals[1] > cap_f) return;
  const int p0 = (blockIdx.x * 256 + threadIdx.x) * 4;
  if (p0 >= g.N) return;
  const unsigned word = *reinterpret_cast<const unsigned*>(mask + p0);   // (the section is padded to 256 bytes)
  for (int e = 0; e < 4; ++e) {
    const unsigned m0 = (word >> (8 * e)) & 0xffu;
    // a cell's corner 000 whose eight corners do not all lie on one side
    if (p0 + e < g.N && (m0 & 0x80u) && (m0 & 0x7fu))
      iso_cell_faces(vol, g, thres, mask, voff, toff, cap_f, faces, p0 + e, m0);
  }
}

// the vertices of the active edges m (seven bits, not 0) of point p
WIRE_DEVINL void iso_point_verts(const float* __restrict__ vol, const IsoGeom& g, float thres,
                                 const unsigned* __restrict__ voff, long long cap_v, float* __restrict__ verts, int p,
                                 unsigned m) {
  int i, j, k;
  iso_locate(g, p, i, j, k);
  const float a = vol[p], num = __fsub_rn(thres, a);
  unsigned long long out = voff[p];
#pragma unroll
  for (int d = 0; d < 7; ++d) {
    if (!((m >> d) & 1u)) continue;
    const int c = iso_dir_code(d);
    const float b = vol[p + iso_code_off(g, c)];
    const float t = __fdiv_rn(num, __fsub_rn(b, a));
    if (out < (unsigned long long)cap_v) {
      float* v = verts + 3 * out;
      v[0] = (c & 1) ? __fadd_rn((float)i, t) : (float)i;
      v[1] = (c & 2) ? __fadd_rn((float)j, t) : (float)j;
      v[2] = (c & 4) ? __fadd_rn((float)k, t) : (float)k;
    }
    ++out;
  }
}

__global__ __launch_bounds__(256) void iso_verts_kernel(const float* __restrict__ vol, IsoGeom g, float thres,
                                                        const uint8_t* __restrict__ mask,
                                                        const unsigned* __restrict__ voff,
                                                        const int64_t* __restrict__ totals, long long cap_v,
                                                        long long cap_f, float* __restrict__ verts) {
  if (totals[0] > cap_v || totals[1] > cap_f) return;
  const int p0 = (blockIdx.x * 256 + threadIdx.x) * 4;
  if (p0 >= g.N) return;
  const unsigned word = *reinterpret_cast<const unsigned*>(mask + p0) & 0x7f7f7f7fu;
  for (int e = 0; e < 4; ++e) {
    const unsigned m = (word >> (8 * e)) & 0xffu;
    if (p0 + e < g.N && m) iso_point_verts(vol, g, thres, voff, cap_v, verts, p0 + e, m);
  }
}

// ---- separable Gaussian blur, edge values replicated ----------------------------------------------------------------
#define ISO_BLUR_MAXR 32
struct BlurTaps { int R; float w[2 * ISO_BLUR_MAXR + 1]; };

// one axis: out[e] = sum_t w[t] in[clamped neighbour], the taps added in order from -R to +R, product and sum each
// rounded once (no contraction): the order of a plain fp32 loop over the taps
__global__ __launch_bounds__(256) void iso_blur_axis_kernel(const float* __restrict__ in, float* __restrict__ out,
                                                            long long total, int len, long long stride, BlurTaps tp) {
  for (long long e = (long long)blockIdx.x * 256 + threadIdx.x; e < total; e += (long long)gridDim.x * 256) {
    const int pos = (int)((e / stride) % len);
    float acc = 0.f;
    for (int t = -tp.R; t <= tp.R; ++t) {
      int q = pos + t;
      q = q < 0 ? 0 : q >= len ? len - 1 : q;
      acc = __fadd_rn(acc, __fmul_rn(tp.w[t + tp.R], in[e + (long long)(q - pos) * stride]));
    }
    out[e] = acc;
  }
}

// ---- host side -----------------------------------------------------------------------------------------------------
static inline long long iso_rup256(long long v) { return (v + 255) / 256 * 256; }
struct IsoLayout { long long mask, voff, toff, scan, bytes; };

static bool iso_geom(int H, int W, int T, IsoGeom& g, IsoLayout& lay) {
  if (H < 2 || W < 2 || T < 2) return false;
  const long long N = (long long)H * W * T;       // < 2^93 cannot happen: checked stepwise
  if ((long long)H * W > ISO_MAX_POINTS || N > ISO_MAX_POINTS) return false;
  g.H = H; g.W = W; g.T = T; g.N = (int)N; g.sH = W * T; g.sW = T;
  lay.mask = 256;
  lay.voff = lay.mask + iso_rup256(N);
  lay.toff = lay.voff + iso_rup256(4 * N);
  lay.scan = lay.toff + iso_rup256(4 * N);
  lay.bytes = lay.scan + iso_rup256(4 * wire_scan_scratch_words(N));
  return true;
}

static hipError_t launch_iso_count(hipStream_t s, const float* vol, const IsoGeom& g, const IsoLayout& lay,
                                   float thres, char* ws, int64_t* counts) {
  uint8_t* mask = reinterpret_cast<uint8_t*>(ws + lay.mask);
  unsigned* voff = reinterpret_cast<unsigned*>(ws + lay.voff);
  unsigned* toff = reinterpret_cast<unsigned*>(ws + lay.toff);
  unsigned* scan = reinterpret_cast<unsigned*>(ws + lay.scan);
  int64_t* totals = reinterpret_cast<int64_t*>(ws);
  // the mask section is rounded up to 256 bytes, so the last thread's word fits; every row of the volume starts on a
  // 16-byte boundary iff the volume does and T is a multiple of 4
  const int vec4 = ((uintptr_t)vol & 15) == 0 && g.T % 4 == 0;
  hipLaunchKernelGGL(iso_classify_kernel, dim3(cdiv(g.N, 1024)), dim3(256), 0, s, vol, g, thres, vec4, mask);
  hipError_t e = hipGetLastError();
  if (e != hipSuccess) return e;
  if ((e = wire_scan_exclusive(s, IsoVertCount{mask}, (long long)g.N, voff, scan, totals)) != hipSuccess) return e;
  if ((e = wire_scan_exclusive(s, IsoTriCount{mask}, (long long)g.N, toff, scan, totals + 1)) != hipSuccess) return e;
  return hipMemcpyAsync(counts, totals, 2 * sizeof(int64_t), hipMemcpyDeviceToDevice, s);
}

// ---------------------------------------------------------------------------
// entry points of the C ABI
// ---------------------------------------------------------------------------
extern "C" int wire_iso_tet_case(int perm, int inside_mask) {
  if (perm < 0 || perm > 5 || inside_mask < 0 || inside_mask > 15)
    return fail(WIRE_ERR_ARG, "wire_iso_tet_case: permutation %d (0..5), inside mask %d (0..15)", perm, inside_mask);
  return (int)ISO_CASES_HOST.e[perm][inside_mask];
}

extern "C" int64_t wire_iso_ws_bytes(int H, int W, int T) {
  IsoGeom g;
  IsoLayout lay;
  if (!iso_geom(H, W, T, g, lay))
    return fail(WIRE_ERR_ARG, "wire_iso_ws_bytes: a %d x %d x %d volume (every side >= 2, at most 2^28 points)", H, W, T);
  return lay.bytes;
}

extern "C" int wire_iso_count(void* stream, const float* vol, int H, int W, int T, float thres, void* ws,
                              int64_t* counts) {
  IsoGeom g;
  IsoLayout lay;
  if (!iso_geom(H, W, T, g, lay) || thres != thres || !vol || !ws || !counts || ((uintptr_t)ws & 15) ||
      ((uintptr_t)counts & 7))
    return fail(WIRE_ERR_ARG, "bad argument to wire_iso_count (every side >= 2, at most 2^28 points, a threshold that is "
                              "a number, ws 16-byte aligned)");
  ProfScope ps((hipStream_t)stream, 3, 0);
  HIPCHK(launch_iso_count((hipStream_t)stream, vol, g, lay, thres, (char*)ws, counts));
  return WIRE_OK;
}

extern "C" int wire_iso_emit(void* stream, const float* vol, int H, int W, int T, float thres, const void* ws,
                             float* verts, int64_t cap_v, int32_t* faces, int64_t cap_f) {
  IsoGeom g;
  IsoLayout lay;
  if (!iso_geom(H, W, T, g, lay) || thres != thres || !vol || !ws || ((uintptr_t)ws & 15) || cap_v < 0 || cap_f < 0 ||
      (cap_v > 0 && !verts) || (cap_f > 0 && !faces))
    return fail(WIRE_ERR_ARG, "bad argument to wire_iso_emit");
  hipStream_t s = (hipStream_t)stream;
  const char* w = (const char*)ws;
  int64_t totals[2] = {0, 0};
  HIPCHK(hipMemcpyAsync(totals, w, sizeof(totals), hipMemcpyDeviceToHost, s));
  HIPCHK(hipStreamSynchronize(s));
  if (totals[0] < 0 || totals[1] < 0 || totals[0] > 7ll * g.N || totals[1] > 12ll * g.N)
    return fail(WIRE_ERR_ARG, "wire_iso_emit: ws does not hold the counts of a wire_iso_count of this volume");
  if (totals[0] > cap_v || totals[1] > cap_f)
    return fail(WIRE_ERR_SIZE, "wire_iso_emit: %lld vertices and %lld faces do not fit capacities of %lld and %lld",
                (long long)totals[0], (long long)totals[1], (long long)cap_v, (long long)cap_f);
  if (totals[0] == 0) return WIRE_OK;                  // no active edge: no face either
  ProfScope ps(s, 3, 0);
  const uint8_t* mask = reinterpret_cast<const uint8_t*>(w + lay.mask);
  const unsigned* voff = reinterpret_cast<const unsigned*>(w + lay.voff);
  const unsigned* toff = reinterpret_cast<const unsigned*>(w + lay.toff);
  const int64_t* dtot = reinterpret_cast<const int64_t*>(w);
  hipLaunchKernelGGL(iso_faces_kernel, dim3(cdiv(g.N, 1024)), dim3(256), 0, s, vol, g, thres, mask, voff, toff,
                     dtot, (long long)cap_v, (long long)cap_f, faces);
  hipLaunchKernelGGL(iso_verts_kernel, dim3(cdiv(g.N, 1024)), dim3(256), 0, s, vol, g, thres, mask, voff, dtot,
                     (long long)cap_v, (long long)cap_f, verts);
  HIPCHK(hipGetLastError());
  return WIRE_OK;
}

extern "C" int wire_gauss3_blur(void* stream, const float* in, int H, int W, int T, float sigma, float* tmp,
                                float* out) {
  const long long total = (long long)H * W * T;
  if (H < 1 || W < 1 || T < 1 || (long long)H * W > (1ll << 31) || total > (1ll << 40) || !(sigma > 0.f) ||
      !__builtin_isfinite(sigma) || !in || !tmp || !out || in == tmp || in == out || tmp == out)
    return fail(WIRE_ERR_ARG, "bad argument to wire_gauss3_blur");
  BlurTaps tp;
  tp.R = (int)(4.0 * (double)sigma + 0.5);             // truncated at 4 sigma
  if (tp.R > ISO_BLUR_MAXR) return fail(WIRE_ERR_ARG, "wire_gauss3_blur: sigma %g needs more than %d taps a side", (double)sigma, ISO_BLUR_MAXR);
  double wd[2 * ISO_BLUR_MAXR + 1], sum = 0.0;
  for (int t = -tp.R; t <= tp.R; ++t) sum += wd[t + tp.R] = exp(-0.5 * (double)t * t / ((double)sigma * sigma));
  for (int t = 0; t < 2 * ISO_BLUR_MAXR + 1; ++t) tp.w[t] = t <= 2 * tp.R ? (float)(wd[t] / sum) : 0.f;
  hipStream_t s = (hipStream_t)stream;
  ProfScope ps(s, 3, 0);
  const unsigned nb = total < (1ll << 28) ? cdiv(total, 256) : (1u << 20);
  hipLaunchKernelGGL(iso_blur_axis_kernel, dim3(nb), dim3(256), 0, s, in, out, total, T, 1ll, tp);
  hipLaunchKernelGGL(iso_blur_axis_kernel, dim3(nb), dim3(256), 0, s, (const float*)out, tmp, total, W, (long long)T, tp);
  hipLaunchKernelGGL(iso_blur_axis_kernel, dim3(nb), dim3(256), 0, s, (const float*)tmp, out, total, H,
                     (long long)W * T, tp);
  HIPCHK(hipGetLastError());
  return WIRE_OK;
}
