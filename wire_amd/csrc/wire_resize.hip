// wire_resize.hip -- image-to-image resampling in cv2.resize's modes (nearest, linear, cubic, area), its adjoint, and the
// super-resolution loss under that operator (include/wire_hip.h).
//
// The operator is separable, R = R_v (x) R_h on a channel-last image x [H][W][C] -> [Hl][Wl][C], and each axis is one
// table: for output d a contiguous run of distinct source indices start[d] .. start[d] + count[d] - 1 with fp32 weights
// (stride K = the axis' largest count), and for source i the contiguous range lo[i] .. hi[i] of outputs whose run
// contains i (start and start + count are both non-decreasing in d, so that set IS a range; it may be empty).
// wire_resize_tables writes both axes' tables in one launch, computing in fp64 and rounding each weight to fp32 once;
// the forward, the adjoint and the loss read these tables and nothing else about the geometry, so the adjoint is the
// exact transpose of the forward: the same fp32 weights, gathered over lo .. hi instead of scattered.  No atomics.
//
// SHAPE: one thread per output element of its side (forward: [Hl][Wl][C]; adjoint: [H][W][C]), the channel running
// fastest, so a wave's loads of one tap row are contiguous runs of floats.  Tap counts are 1 .. 4 (nearest, linear,
// cubic) or about the scale + 1 (area): no LDS, the taps of neighbouring threads meet in the L1 / L2.  Accumulation in
// fp32, rows outer, columns inner, both ascending:  acc = fma(wv[a], (sum_b fma(wh[b], x[a][b], .)), acc), from +0.0.
//
// rs_axis_out below is the definition; host and device run the same function (no contraction), which is how the host
// knows K, and with it the layout of the tables, without reading the device.
#include <cmath>

#include "wire_dev.h"
#include "wire_plan.h"

#define RS_MAX_BLOCKS (1u << 20)      // forward / adjoint: blocks of 256 elements, looping above 2^28 elements

// ---------------------------------------------------------------------------
// one axis, one output: the run and (w != NULL) its weights
// ---------------------------------------------------------------------------
__host__ __device__ static inline int rs_clampi(int v, int lo, int hi) { return v < lo ? lo : (v > hi ? hi : v); }

// Output d of an axis of n_in sources at scale s -> start, count (count >= 1) and, if w, count weights rounded to
// fp32 once and zeros up to K.  Tap indices are clamped to [0, n_in - 1] and taps that meet after clamping are added,
// in tap order, in fp64.
__host__ __device__ static void rs_axis_out(int mode, int n_in, double s, int d, int& start, int& count, float* w,
                                            int K) {
#pragma clang fp contract(off)
  double tw[4] = {1.0, 0.0, 0.0, 0.0};
  int first = 0, ntaps = 1;
  if (s == 1.0) {                     // f = 0 in every mode: all weight on tap d, the zero-weight neighbours are not kept
    first = d;
  } else if (mode == WIRE_RESIZE_NEAREST) {
    double p = floor((double)d * s);
    if (p > (double)(n_in - 1)) p = (double)(n_in - 1);
    first = (int)p;
  } else if (mode == WIRE_RESIZE_AREA) {
    const double a = (double)d * s;
    double b = ((double)d + 1.0) * s;
    if (b > (double)n_in) b = (double)n_in;
    if (!(b > a)) {                   // an empty cell: refused by rs_geom, kept in bounds here
      double p = floor(a);
      if (!(p < (double)(n_in - 1))) p = (double)(n_in - 1);
      first = (int)p;
    } else {
      int i0 = (int)floor(a), i1 = (int)ceil(b);          // 0 <= a < b <= n_in
      // the taps are the pixels of [i0, i1) whose overlap with the cell is positive: only an end pixel can fail that
      while (i0 < i1 - 1 && !(fmin((double)i0 + 1.0, b) - fmax((double)i0, a) > 0.0)) ++i0;
      while (i1 - 1 > i0 && !(fmin((double)i1, b) - fmax((double)i1 - 1.0, a) > 0.0)) --i1;
      start = rs_clampi(i0, 0, n_in - 1);
      count = rs_clampi(i1 - 1, 0, n_in - 1) - start + 1;
      if (w) {
        const double len = b - a;
        for (int k = 0; k < K; ++k) {
          const double i = (double)(start + k);
          w[k] = k < count ? (float)((fmin(i + 1.0, b) - fmax(i, a)) / len) : 0.f;
        }
      }
      return;
    }
  } else {                            // linear, cubic
    double x = ((double)d + 0.5) * s - 0.5, xi = floor(x), f = x - xi;
    if (xi < -4.0) { xi = -4.0; f = 0.0; }                 // every tap clamps to the same border pixel: weight 1 there
    if (xi > (double)n_in + 4.0) { xi = (double)n_in + 4.0; f = 0.0; }
    const int i = (int)xi;
    if (mode == WIRE_RESIZE_LINEAR) {
      first = i; ntaps = 2;
      tw[0] = 1.0 - f; tw[1] = f;
    } else {
      const double A = -0.75, g = 1.0 - f;
      first = i - 1; ntaps = 4;
      tw[0] = ((A * (f + 1.0) - 5.0 * A) * (f + 1.0) + 8.0 * A) * (f + 1.0) - 4.0 * A;
      tw[1] = ((A + 2.0) * f - (A + 3.0)) * f * f + 1.0;
      tw[2] = ((A + 2.0) * g - (A + 3.0)) * g * g + 1.0;
      tw[3] = 1.0 - tw[0] - tw[1] - tw[2];
    }
  }
  start = rs_clampi(first, 0, n_in - 1);
  count = rs_clampi(first + ntaps - 1, 0, n_in - 1) - start + 1;
  if (w) {
    double acc[4] = {0.0, 0.0, 0.0, 0.0};
    for (int t = 0; t < ntaps; ++t) acc[rs_clampi(first + t, 0, n_in - 1) - start] += tw[t];
    for (int k = 0; k < K; ++k) w[k] = k < count && k < 4 ? (float)acc[k] : 0.f;
  }
}

// ---------------------------------------------------------------------------
// geometry: checked once on the host; the layout of tab in 4-byte words
// ---------------------------------------------------------------------------
struct RsAxis { int n_in, n_out, K; double s; long long start, count, lo, hi, w, end; };   // word offsets into tab
struct RsGeom { int mode; RsAxis v, h; };
struct RsAxisDev { const int* start; const int* count; const int* lo; const int* hi; const float* w; int n_in, n_out, K; };
struct RsDev { RsAxisDev v, h; };

static int rs_axis_K(int mode, int n_in, int n_out, double s) {
  int K = 1;
  if (s == 1.0 || mode == WIRE_RESIZE_NEAREST) return K;
  for (int d = 0; d < n_out; ++d) {
    int st, c;
    rs_axis_out(mode, n_in, s, d, st, c, nullptr, 0);
    if (c > K) K = c;
  }
  return K;
}
static bool rs_axis_ok(int mode, int n_in, int n_out, double s) {
  if (n_in < 1 || n_out < 1 || !std::isfinite(s) || !(s > 0.0)) return false;
  // area: no up-scaling, and every cell [d s, (d + 1) s) must begin inside the source
  if (mode == WIRE_RESIZE_AREA && (n_out > n_in || !((double)(n_out - 1) * s < (double)n_in))) return false;
  return true;
}
// false: a refused geometry (a side < 1, an unknown mode, area up-scaling, a bad scale, sizes beyond 63 bits)
static bool rs_geom(int H, int W, int Hl, int Wl, int mode, double sy, double sx, RsGeom& g) {
  if (mode < WIRE_RESIZE_NEAREST || mode > WIRE_RESIZE_AREA) return false;
  if (!rs_axis_ok(mode, H, Hl, sy) || !rs_axis_ok(mode, W, Wl, sx)) return false;
  // the last geometry's tap counts are kept: a training loop asks for the same one every step
  static thread_local struct { int H, W, Hl, Wl, mode, Kv, Kh; double sy, sx; bool set = false; } last;
  if (!(last.set && last.H == H && last.W == W && last.Hl == Hl && last.Wl == Wl && last.mode == mode && last.sy == sy &&
        last.sx == sx)) {
    last.set = false;
    last.Kv = rs_axis_K(mode, H, Hl, sy);
    last.Kh = rs_axis_K(mode, W, Wl, sx);
    last.H = H; last.W = W; last.Hl = Hl; last.Wl = Wl; last.mode = mode; last.sy = sy; last.sx = sx;
    last.set = true;
  }
  g.mode = mode;
  long long off = 0;
  auto lay = [&](RsAxis& a, int n_in, int n_out, double s, int K) {
    a.n_in = n_in; a.n_out = n_out; a.K = K; a.s = s;
    a.start = off; a.count = a.start + n_out; a.lo = a.count + n_out; a.hi = a.lo + n_in; a.w = a.hi + n_in;
    a.end = a.w + (long long)n_out * K;                    // < 2^31 * 2^31 + 2^33
    off = a.end;
  };
  lay(g.v, H, Hl, sy, last.Kv);
  lay(g.h, W, Wl, sx, last.Kh);
  return true;
}
static RsDev rs_dev(const RsGeom& g, const void* tab) {
  const int* t = (const int*)tab;
  auto ax = [&](const RsAxis& a) {
    return RsAxisDev{t + a.start, t + a.count, t + a.lo, t + a.hi, (const float*)(t + a.w), a.n_in, a.n_out, a.K};
  };
  return RsDev{ax(g.v), ax(g.h)};
}
static bool rs_sides(int H, int W, int Hl, int Wl) { return H >= 1 && W >= 1 && Hl >= 1 && Wl >= 1; }
// n0 * n1 * C, false beyond 63 bits (the cheap checks come before rs_geom, which walks the outputs for K)
static bool rs_total(int n0, int n1, int C, long long& total) {
  return C >= 1 && !__builtin_mul_overflow((long long)n0 * n1, (long long)C, &total);
}

// ---------------------------------------------------------------------------
// the tables: one thread per entry of (v outputs, v sources, h outputs, h sources)
// ---------------------------------------------------------------------------
struct RsAxisTab { int* start; int* count; int* lo; int* hi; float* w; int n_in, n_out, K; double s; };

__device__ static void rs_tab_out(const RsAxisTab& a, int mode, int d) {
  int st, c;
  rs_axis_out(mode, a.n_in, a.s, d, st, c, a.w + (long long)d * a.K, a.K);
  a.start[d] = st;
  a.count[d] = c < a.K ? c : a.K;
}
// lo = the first output whose run ends behind i, hi = the last one whose run starts at or before i (lo = hi + 1: none)
__device__ static void rs_tab_src(const RsAxisTab& a, int mode, int i) {
  int st, c;
  int l = 0, r = a.n_out;                                  // first d in [0, n_out] with start + count > i
  while (l < r) {
    const int m = l + (r - l) / 2;
    rs_axis_out(mode, a.n_in, a.s, m, st, c, nullptr, 0);
    if (st + c > i) r = m; else l = m + 1;
  }
  a.lo[i] = l;
  l = 0; r = a.n_out;                                      // first d in [0, n_out] with start > i
  while (l < r) {
    const int m = l + (r - l) / 2;
    rs_axis_out(mode, a.n_in, a.s, m, st, c, nullptr, 0);
    if (st > i) r = m; else l = m + 1;
  }
  a.hi[i] = l - 1;
}
__global__ __launch_bounds__(256) void resize_tables_kernel(RsAxisTab v, RsAxisTab h, int mode) {
  long long t = (long long)blockIdx.x * 256 + threadIdx.x;
  if (t < v.n_out) { rs_tab_out(v, mode, (int)t); return; }
  t -= v.n_out;
  if (t < v.n_in) { rs_tab_src(v, mode, (int)t); return; }
  t -= v.n_in;
  if (t < h.n_out) { rs_tab_out(h, mode, (int)t); return; }
  t -= h.n_out;
  if (t < h.n_in) rs_tab_src(h, mode, (int)t);
}

// ---------------------------------------------------------------------------
// forward, adjoint, loss
// ---------------------------------------------------------------------------
// (R x)[di][dj][c]: rows outer, columns inner, ascending; indices and counts are held inside the arrays whatever tab holds
template <typename I>
__device__ __forceinline__ float rs_fwd_at(const RsDev& t, const float* __restrict__ x, I C, I di, I dj, I c) {
  const int sv = t.v.start[di], sh = t.h.start[dj];
  const int cv = min(t.v.count[di], t.v.K), ch = min(t.h.count[dj], t.h.K);
  const float* wv = t.v.w + (size_t)di * t.v.K;
  const float* wh = t.h.w + (size_t)dj * t.h.K;
  float acc = 0.f;
  for (int a = 0; a < cv; ++a) {
    const int r = rs_clampi(sv + a, 0, t.v.n_in - 1);
    const float* row = x + (size_t)r * t.h.n_in * C + c;
    float ra = 0.f;
    for (int b = 0; b < ch; ++b) {
      const int q = rs_clampi(sh + b, 0, t.h.n_in - 1);
      ra = __builtin_fmaf(wh[b], row[(size_t)q * C], ra);
    }
    acc = __builtin_fmaf(wv[a], ra, acc);
  }
  return acc;
}
// (R^T g)[i][j][c]: the gather over lo .. hi, in the same order
template <typename I>
__device__ __forceinline__ float rs_bwd_at(const RsDev& t, const float* __restrict__ g, I C, I i, I j, I c) {
  const int l0 = max(t.v.lo[i], 0), l1 = min(t.v.hi[i], t.v.n_out - 1);
  const int m0 = max(t.h.lo[j], 0), m1 = min(t.h.hi[j], t.h.n_out - 1);
  float acc = 0.f;
  for (int dr = l0; dr <= l1; ++dr) {
    const int ka = (int)i - t.v.start[dr];
    if ((unsigned)ka >= (unsigned)t.v.K) continue;
    const float* row = g + (size_t)dr * t.h.n_out * C + c;
    float ra = 0.f;
    for (int dc = m0; dc <= m1; ++dc) {
      const int kb = (int)j - t.h.start[dc];
      if ((unsigned)kb >= (unsigned)t.h.K) continue;
      ra = __builtin_fmaf(t.h.w[(size_t)dc * t.h.K + kb], row[(size_t)dc * C], ra);
    }
    acc = __builtin_fmaf(t.v.w[(size_t)dr * t.v.K + ka], ra, acc);
  }
  return acc;
}

// LOSS = false: y = R x.  LOSS = true: rec = R x, d = rec - gt, res = gscale * d (the adjoint's input), rec_lr
// (optional) = rec, partial[block] = the block's sum of d^2.
template <typename I, bool LOSS>
__global__ __launch_bounds__(256) void resize_fwd_kernel(RsDev t, const float* __restrict__ x, int C, long long total,
                                                         float* __restrict__ y, const float* __restrict__ gt,
                                                         float gscale, float* __restrict__ rec_lr,
                                                         float* __restrict__ partial) {
  __shared__ float red[4];
  const I Cc = (I)C, WC = (I)t.h.n_out * Cc;
  float sq = 0.f;
  for (long long el = (long long)blockIdx.x * 256 + threadIdx.x; el < total; el += (long long)gridDim.x * 256) {
    const I e = (I)el, di = e / WC, rem = e - di * WC, dj = rem / Cc, c = rem - dj * Cc;
    const float v = rs_fwd_at<I>(t, x, Cc, di, dj, c);
    if (LOSS) {
      const float d = v - gt[el];
      y[el] = __fmul_rn(gscale, d);
      if (rec_lr) rec_lr[el] = v;
      sq = __builtin_fmaf(d, d, sq);
    } else {
      y[el] = v;
    }
  }
  if (LOSS) {
    sq = wire_block_sum(sq, red);
    if (threadIdx.x == 0) partial[blockIdx.x] = sq;
  }
}
// g_x = R^T g; FINAL: block 0 also adds the nb partials of the loss forward in a fixed order, loss_out[0] = lscale * sum
template <typename I, bool FINAL>
__global__ __launch_bounds__(256) void resize_bwd_kernel(RsDev t, const float* __restrict__ g, int C, long long total,
                                                         float* __restrict__ g_x, const float* __restrict__ partial,
                                                         int nb, float lscale, float* __restrict__ loss_out) {
  __shared__ float red[4];
  const I Cc = (I)C, WC = (I)t.h.n_in * Cc;
  for (long long el = (long long)blockIdx.x * 256 + threadIdx.x; el < total; el += (long long)gridDim.x * 256) {
    const I e = (I)el, i = e / WC, rem = e - i * WC, j = rem / Cc, c = rem - j * Cc;
    g_x[el] = rs_bwd_at<I>(t, g, Cc, i, j, c);
  }
  if (FINAL && blockIdx.x == 0) {
    float a = 0.f;
    for (int k = threadIdx.x; k < nb; k += 256) a += partial[k];
    a = wire_block_sum(a, red);
    if (threadIdx.x == 0) loss_out[0] = __fmul_rn(a, lscale);
  }
}

static unsigned rs_blocks(long long n) {
  const long long nb = (n + 255) / 256;
  return nb < (long long)RS_MAX_BLOCKS ? (unsigned)nb : RS_MAX_BLOCKS;
}
static bool rs_small(long long a, long long b) { return a < (1ll << 31) && b < (1ll << 31); }   // 32-bit index arithmetic

static hipError_t launch_resize_tables(hipStream_t s, const RsGeom& g, void* tab) {
  int* t = (int*)tab;
  auto ax = [&](const RsAxis& a) {
    return RsAxisTab{t + a.start, t + a.count, t + a.lo, t + a.hi, (float*)(t + a.w), a.n_in, a.n_out, a.K, a.s};
  };
  const long long n = (long long)g.v.n_out + g.v.n_in + g.h.n_out + g.h.n_in;
  hipLaunchKernelGGL(resize_tables_kernel, dim3(cdiv(n, 256)), dim3(256), 0, s, ax(g.v), ax(g.h), g.mode);
  return hipGetLastError();
}
static hipError_t launch_resize_fwd(hipStream_t s, const RsGeom& g, const void* tab, const float* x, int C,
                                    long long n_src, long long n_dst, float* y) {
  const RsDev t = rs_dev(g, tab);
  if (rs_small(n_src, n_dst))
    hipLaunchKernelGGL((resize_fwd_kernel<unsigned, false>), dim3(rs_blocks(n_dst)), dim3(256), 0, s, t, x, C, n_dst, y,
                       nullptr, 0.f, nullptr, nullptr);
  else
    hipLaunchKernelGGL((resize_fwd_kernel<unsigned long long, false>), dim3(rs_blocks(n_dst)), dim3(256), 0, s, t, x, C,
                       n_dst, y, nullptr, 0.f, nullptr, nullptr);
  return hipGetLastError();
}
static hipError_t launch_resize_bwd(hipStream_t s, const RsGeom& g, const void* tab, const float* g_y, int C,
                                    long long n_src, long long n_dst, float* g_x) {
  const RsDev t = rs_dev(g, tab);
  if (rs_small(n_src, n_dst))
    hipLaunchKernelGGL((resize_bwd_kernel<unsigned, false>), dim3(rs_blocks(n_src)), dim3(256), 0, s, t, g_y, C, n_src,
                       g_x, nullptr, 0, 0.f, nullptr);
  else
    hipLaunchKernelGGL((resize_bwd_kernel<unsigned long long, false>), dim3(rs_blocks(n_src)), dim3(256), 0, s, t, g_y,
                       C, n_src, g_x, nullptr, 0, 0.f, nullptr);
  return hipGetLastError();
}
static hipError_t launch_resize_mse_grad(hipStream_t s, const RsGeom& g, const void* tab, const float* y, int O,
                                         long long n_src, long long n_dst, const float* gt_lr, float* g_y,
                                         float* rec_lr, float* loss_out, float* res, float* partial) {
  const RsDev t = rs_dev(g, tab);
  const unsigned nb = mse_blocks(n_dst);                   // <= 1024 blocks: the partials fit `partial`
  const float gscale = (float)(2.0 / (double)n_dst), lscale = (float)(1.0 / (double)n_dst);
  if (rs_small(n_src, n_dst)) {
    hipLaunchKernelGGL((resize_fwd_kernel<unsigned, true>), dim3(nb), dim3(256), 0, s, t, y, O, n_dst, res, gt_lr,
                       gscale, rec_lr, partial);
    hipLaunchKernelGGL((resize_bwd_kernel<unsigned, true>), dim3(rs_blocks(n_src)), dim3(256), 0, s, t, res, O, n_src,
                       g_y, partial, (int)nb, lscale, loss_out);
  } else {
    hipLaunchKernelGGL((resize_fwd_kernel<unsigned long long, true>), dim3(nb), dim3(256), 0, s, t, y, O, n_dst, res,
                       gt_lr, gscale, rec_lr, partial);
    hipLaunchKernelGGL((resize_bwd_kernel<unsigned long long, true>), dim3(rs_blocks(n_src)), dim3(256), 0, s, t, res,
                       O, n_src, g_y, partial, (int)nb, lscale, loss_out);
  }
  return hipGetLastError();
}

// ---------------------------------------------------------------------------
// entry points of the C ABI
// ---------------------------------------------------------------------------
extern "C" int64_t wire_resize_tab_bytes(int H, int W, int Hl, int Wl, int mode, double sy, double sx) {
  RsGeom g;
  if (!rs_geom(H, W, Hl, Wl, mode, sy, sx, g)) return fail(WIRE_ERR_ARG, "bad argument to wire_resize_tab_bytes");
  return (int64_t)(4 * g.h.end);
}
extern "C" int64_t wire_resize_mse_grad_ws_bytes(int Hl, int Wl, int O) {
  long long total;
  if (Hl < 1 || Wl < 1 || !rs_total(Hl, Wl, O, total) || total > (1ll << 60))
    return fail(WIRE_ERR_ARG, "bad argument to wire_resize_mse_grad_ws_bytes");
  return (int64_t)(4 * total);
}
extern "C" int wire_resize_tables(void* stream, int H, int W, int Hl, int Wl, int mode, double sy, double sx,
                                  void* tab) {
  RsGeom g;
  if (!rs_geom(H, W, Hl, Wl, mode, sy, sx, g) || !tab) return fail(WIRE_ERR_ARG, "bad argument to wire_resize_tables");
  ProfScope ps((hipStream_t)stream, 3, 0);
  HIPCHK(launch_resize_tables((hipStream_t)stream, g, tab));
  return WIRE_OK;
}
extern "C" int wire_resize_fwd(void* stream, const void* tab, int H, int W, int Hl, int Wl, int mode, double sy,
                               double sx, const float* x, int C, float* y) {
  RsGeom g;
  long long n_src, n_dst;
  if (!rs_sides(H, W, Hl, Wl) || !rs_total(H, W, C, n_src) || !rs_total(Hl, Wl, C, n_dst) || !tab || !x || !y ||
      !rs_geom(H, W, Hl, Wl, mode, sy, sx, g))
    return fail(WIRE_ERR_ARG, "bad argument to wire_resize_fwd");
  ProfScope ps((hipStream_t)stream, 3, 0);
  HIPCHK(launch_resize_fwd((hipStream_t)stream, g, tab, x, C, n_src, n_dst, y));
  return WIRE_OK;
}
extern "C" int wire_resize_bwd(void* stream, const void* tab, int H, int W, int Hl, int Wl, int mode, double sy,
                               double sx, const float* g_y, int C, float* g_x) {
  RsGeom g;
  long long n_src, n_dst;
  if (!rs_sides(H, W, Hl, Wl) || !rs_total(H, W, C, n_src) || !rs_total(Hl, Wl, C, n_dst) || !tab || !g_y || !g_x ||
      !rs_geom(H, W, Hl, Wl, mode, sy, sx, g))
    return fail(WIRE_ERR_ARG, "bad argument to wire_resize_bwd");
  ProfScope ps((hipStream_t)stream, 3, 0);
  HIPCHK(launch_resize_bwd((hipStream_t)stream, g, tab, g_y, C, n_src, n_dst, g_x));
  return WIRE_OK;
}
extern "C" int wire_resize_mse_grad(void* stream, const void* tab, int H, int W, int Hl, int Wl, int mode, double sy,
                                    double sx, const float* y, int O, const float* gt_lr, float* g_y, float* rec_lr,
                                    float* loss_out, void* ws, int64_t ws_bytes, float* partial) {
  RsGeom g;
  long long n_src, n_dst;
  if (!rs_sides(H, W, Hl, Wl) || !rs_total(H, W, O, n_src) || !rs_total(Hl, Wl, O, n_dst) || n_dst > (1ll << 60) ||
      ws_bytes < 4 * n_dst || !tab || !y || !gt_lr || !g_y || !loss_out || !ws || !partial ||
      !rs_geom(H, W, Hl, Wl, mode, sy, sx, g))
    return fail(WIRE_ERR_ARG, "bad argument to wire_resize_mse_grad");
  ProfScope ps((hipStream_t)stream, 3, 0);
  HIPCHK(launch_resize_mse_grad((hipStream_t)stream, g, tab, y, O, n_src, n_dst, gt_lr, g_y, rec_lr, loss_out,
                                (float*)ws, partial));
  return WIRE_OK;
}
