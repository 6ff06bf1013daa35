// wire_tv.hip -- the anisotropic total variation of an image (utils.total_variation_loss, modules/utils.py:360-369)
//   tv(x) = sum |x[i+1][j] - x[i][j]| + sum |x[i][j+1] - x[i][j]|      (a sum, not a mean; every plane on its own)
// its gradient under torch's d|u|/du = s(u) in {-1, 0, +1}, s(0) = 0
//   dtv/dx[i][j] = s(x[i][j] - x[i-1][j]) - s(x[i+1][j] - x[i][j]) + s(x[i][j] - x[i][j-1]) - s(x[i][j+1] - x[i][j])
// (a term whose neighbour lies outside the image is 0), and the loss of the regularised training loop, mse + lambda tv,
// fused with its backward.  s comes from two comparisons, (a > b) - (a < b), never from the rounded difference: the
// integer k = dtv/dx in -4 .. 4 is exact whatever the denormal mode, and k * g is one rounding.
//
// SHAPE: no tiles and no LDS halo.  Every kernel is one grid-stride pass of 256-thread blocks, at most TV_BLOCKS of
// them; an element's own value and its four neighbours are plain global loads.  Left and right lie in the lane's own or
// the next cache line; up and down are one image row away and are the `own` loads of the threads one row off, in this
// block or a neighbouring one, so they come from the L1 / L2 that those loads filled.  The headline image
// (512 x 512 x 3 floats, 3 MB) fits one XCD's L2 whole; HBM sees each array once.  A staged halo would save L1 / L2
// hits that a launch-bound operator of a few microseconds does not wait for, and would need a 2-D tile per stride form;
// it was not built.
//   wire_tv_bwd, wire_tv_mse_grad: one thread per FLAT element.  A block boundary falls wherever 256 elements end,
//     inside a row as well as between rows, and a block loops once the image has more than TV_BLOCKS * 256 = 262 144
//     elements.  The order of the elements lets lanes write consecutive floats in both layouts the entry points name:
//     the plane index runs fastest when plane_stride < pix_stride (the network's own [H*W][O] output: element e lies at
//     x + e), the pixel index otherwise (a contiguous (B, C, H, W) tensor).
//   wire_tv_fwd: one thread per PIXEL, which adds its planes in order; a block loops above 262 144 pixels.  Which
//     thread adds which term, and in which order, then depends on (planes, H, W) alone and not on the strides: a
//     permuted view and its contiguous copy give the same bits.  (On the channel-last layout a wave's load spans
//     64 * planes floats, of which the loads of the other planes use the rest out of the L1.)
//
// SUMS: a thread's terms in order, the wave by shuffles, the four waves and then the blocks' partials in a fixed
// order (tv_final_kernel).  No atomics: the same call gives the same bits.
//
//   wire_tv_add_grad: the same one thread per flat element on the network's own [H*W*T][O] rows, a third axis (the
//     frames of a video, k of row (i*W + j)*T + k) with its own weight, and the term ADDED to a g_y that an operator's
//     backward has left.  Six neighbours, O, T*O and W*T*O floats away; the first two pairs lie within a few cache
//     lines of the lane's own, the third is one image row of T*O*W floats away and is the `own` load of a thread
//     that far off.  On a large video (256 x 256 x 16 x 3 floats = 12.6 MB, three XCD L2s' worth) whether that load
//     still comes out of the L2 and not the Infinity Cache is UNMEASURED; no halo was built for it either.
//
// The four entry points of the C ABI (include/wire_hip.h) are at the end of this file.
#include "wire_dev.h"
#include "wire_plan.h"

#define TV_BLOCKS 1024

struct TvGeom {
  long long npix, total;       // H * W, planes * H * W
  long long ps, qs;            // pix_stride, plane_stride
  int H, W, planes, plane_fast;
};

__device__ __forceinline__ int tv_sign(float a, float b) { return (int)(a > b) - (int)(a < b); }

// flat element e -> its address, row and column
__device__ __forceinline__ long long tv_locate(const TvGeom& g, long long e, int& i, int& j) {
  long long p, pix;
  if (g.plane_fast) { pix = e / g.planes; p = e - pix * g.planes; }
  else              { p = e / g.npix;     pix = e - p * g.npix; }
  const long long r = pix / g.W;
  i = (int)r;
  j = (int)(pix - r * g.W);
  return p * g.qs + pix * g.ps;
}

// |down - own| + |right - own| of element (i, j) at address a
__device__ __forceinline__ float tv_pair_sum(const float* __restrict__ x, const TvGeom& g, long long a, int i, int j) {
  const float v = x[a];
  float s = 0.f;
  if (i + 1 < g.H) s += fabsf(x[a + g.W * g.ps] - v);
  if (j + 1 < g.W) s += fabsf(x[a + g.ps] - v);
  return s;
}
// dtv/dx of element (i, j) at address a: an integer in -4 .. 4
__device__ __forceinline__ int tv_grad_int(const float* __restrict__ x, const TvGeom& g, long long a, int i, int j,
                                           float v) {
  int k = 0;
  if (i > 0)       k += tv_sign(v, x[a - g.W * g.ps]);
  if (i + 1 < g.H) k -= tv_sign(x[a + g.W * g.ps], v);
  if (j > 0)       k += tv_sign(v, x[a - g.ps]);
  if (j + 1 < g.W) k -= tv_sign(x[a + g.ps], v);
  return k;
}

__global__ __launch_bounds__(256) void tv_fwd_kernel(const float* __restrict__ x, TvGeom g,
                                                     float* __restrict__ partial) {
  __shared__ float red[4];
  float acc = 0.f;
  for (long long pix = (long long)blockIdx.x * 256 + threadIdx.x; pix < g.npix; pix += (long long)gridDim.x * 256) {
    const long long r = pix / g.W;
    const int i = (int)r, j = (int)(pix - r * g.W);
    const long long a = pix * g.ps;
    for (int p = 0; p < g.planes; ++p) acc += tv_pair_sum(x, g, a + p * g.qs, i, j);
  }
  acc = wire_block_sum(acc, red);
  if (threadIdx.x == 0) partial[blockIdx.x] = acc;
}

__global__ __launch_bounds__(256) void tv_bwd_kernel(const float* __restrict__ x, TvGeom g,
                                                     const float* __restrict__ g_tv, float* __restrict__ g_x) {
  const float up = g_tv[0];
  for (long long e = (long long)blockIdx.x * 256 + threadIdx.x; e < g.total; e += (long long)gridDim.x * 256) {
    int i, j;
    const long long a = tv_locate(g, e, i, j);
    g_x[a] = up * (float)tv_grad_int(x, g, a, i, j, x[a]);
  }
}

// The regularised loss on the network's own layout (element e of [H*W][O] lies at y + e): the TV term of every element
// and, for the rows [first, first + n_mse), the MSE term -- both or the TV term alone in ONE store to g_y.  partial[b]
// receives the block's TV sum and partial[TV_BLOCKS + b] its sum of squared residuals.
__global__ __launch_bounds__(256) void tv_mse_grad_kernel(const float* __restrict__ y, TvGeom g,
                                                          const float* __restrict__ target, long long first,
                                                          long long n_mse, float gscale, float lambda,
                                                          float* __restrict__ g_y, float* __restrict__ rec,
                                                          float* __restrict__ partial) {
  __shared__ float red[4];
  const long long e0 = first * g.planes, e1 = (first + n_mse) * g.planes;     // the selected elements
  float tv = 0.f, sq = 0.f;
  for (long long e = (long long)blockIdx.x * 256 + threadIdx.x; e < g.total; e += (long long)gridDim.x * 256) {
    int i, j;
    tv_locate(g, e, i, j);
    const float v = y[e];
    tv += tv_pair_sum(y, g, e, i, j);
    float out = __fmul_rn(lambda, (float)tv_grad_int(y, g, e, i, j, v));
    if (e >= e0 && e < e1) {
      const float d = v - target[e];
      out = __builtin_fmaf(gscale, d, out);
      if (rec) rec[e] = v;
      sq = __builtin_fmaf(d, d, sq);
    }
    g_y[e] = out;
  }
  tv = wire_block_sum(tv, red);
  sq = wire_block_sum(sq, red);
  if (threadIdx.x == 0) {
    partial[blockIdx.x] = tv;
    partial[TV_BLOCKS + blockIdx.x] = sq;
  }
}

// The MSE term of the rows idx[0 .. n_mse) (distinct), added to the TV term that tv_mse_grad_kernel has stored: one
// thread per selected element reads and rewrites its own element of g_y.  partial[TV_BLOCKS + b] = the block's sum of
// squared residuals.
__global__ __launch_bounds__(256) void tv_mse_rows_kernel(const float* __restrict__ y, int O,
                                                          const float* __restrict__ target,
                                                          const int64_t* __restrict__ idx, long long n_mse,
                                                          float gscale, float* __restrict__ g_y,
                                                          float* __restrict__ rec, float* __restrict__ partial) {
  __shared__ float red[4];
  const long long total = n_mse * O;
  float sq = 0.f;
  for (long long t = (long long)blockIdx.x * 256 + threadIdx.x; t < total; t += (long long)gridDim.x * 256) {
    const long long r = t / O;
    const long long e = (long long)idx[r] * O + (t - r * O);
    const float v = y[e];
    const float d = v - target[e];
    g_y[e] = __builtin_fmaf(gscale, d, g_y[e]);
    if (rec) rec[e] = v;
    sq = __builtin_fmaf(d, d, sq);
  }
  sq = wire_block_sum(sq, red);
  if (threadIdx.x == 0) partial[TV_BLOCKS + blockIdx.x] = sq;
}

// out[0] = scale * sum of n_tv partials (wire_tv_fwd: scale 1); with n_sq >= 0 also the three numbers of the
// regularised loss: out[2] = tv, out[1] = mse = lscale * sum of n_sq partials at partial + TV_BLOCKS,
// out[0] = mse + lambda * tv (product and sum each rounded once)
__global__ __launch_bounds__(256) void tv_final_kernel(const float* __restrict__ partial, int n_tv, int n_sq,
                                                       float lscale, float lambda, float* __restrict__ out) {
  __shared__ float red[4];
  float a = 0.f, b = 0.f;
  for (int i = threadIdx.x; i < n_tv; i += 256) a += partial[i];
  for (int i = threadIdx.x; i < n_sq; i += 256) b += partial[TV_BLOCKS + i];
  a = wire_block_sum(a, red);
  b = wire_block_sum(b, red);
  if (threadIdx.x != 0) return;
  if (n_sq < 0) { out[0] = a; return; }
  {  // (no contraction: the stored mse, not the unrounded product b * lscale, is what the loss adds)
#pragma clang fp contract(off)
    const float mse = b * lscale;
    out[0] = mse + lambda * a;
    out[1] = mse;
    out[2] = a;
  }
}

// ---- the TV term of an (H, W, T) grid of O channels, added to a gradient that is already there (wire_tv_add_grad)
struct TvGeom3 {
  long long total, sh, sw;     // H * W * T * O; the floats between two rows (W * T * O) and two columns (T * O)
  int H, W, T, O;
};

// element e = ((i*W + j)*T + k)*O + o.  partial[b] receives the block's spatial sum, partial[TV_BLOCKS + b] its
// temporal one.  g_y[e] = fl(g_y[e] + fma(lambda_t, k_t, fl(lambda_s * k_s))): three roundings.
__global__ __launch_bounds__(256) void tv_add_grad_kernel(const float* __restrict__ y, TvGeom3 g, float lambda_s,
                                                          float lambda_t, float* __restrict__ g_y,
                                                          float* __restrict__ partial) {
  __shared__ float red[4];
  float tvs = 0.f, tvt = 0.f;
  for (long long e = (long long)blockIdx.x * 256 + threadIdx.x; e < g.total; e += (long long)gridDim.x * 256) {
    const long long row = e / g.O, pix = row / g.T, r = pix / g.W;
    const int k = (int)(row - pix * g.T), j = (int)(pix - r * g.W), i = (int)r;
    const float v = y[e];
    int ks = 0, kt = 0;
    if (i > 0) ks += tv_sign(v, y[e - g.sh]);
    if (i + 1 < g.H) { const float d = y[e + g.sh]; ks -= tv_sign(d, v); tvs += fabsf(d - v); }
    if (j > 0) ks += tv_sign(v, y[e - g.sw]);
    if (j + 1 < g.W) { const float d = y[e + g.sw]; ks -= tv_sign(d, v); tvs += fabsf(d - v); }
    if (k > 0) kt += tv_sign(v, y[e - g.O]);
    if (k + 1 < g.T) { const float d = y[e + g.O]; kt -= tv_sign(d, v); tvt += fabsf(d - v); }
    const float term = __builtin_fmaf(lambda_t, (float)kt, __fmul_rn(lambda_s, (float)ks));
    g_y[e] = __fadd_rn(g_y[e], term);
  }
  tvs = wire_block_sum(tvs, red);
  tvt = wire_block_sum(tvt, red);
  if (threadIdx.x == 0) {
    partial[blockIdx.x] = tvs;
    partial[TV_BLOCKS + blockIdx.x] = tvt;
  }
}

// out[2] = tv_s and out[3] = tv_t, the sums of nb partials each; out[1] = data = data_loss[0] (0 when NULL);
// out[0] = fl(fl(data + fl(lambda_s tv_s)) + fl(lambda_t tv_t))
__global__ __launch_bounds__(256) void tv_add_final_kernel(const float* __restrict__ partial, int nb, float lambda_s,
                                                           float lambda_t, const float* __restrict__ data_loss,
                                                           float* __restrict__ out) {
  __shared__ float red[4];
  float a = 0.f, b = 0.f;
  for (int i = threadIdx.x; i < nb; i += 256) a += partial[i];
  for (int i = threadIdx.x; i < nb; i += 256) b += partial[TV_BLOCKS + i];
  a = wire_block_sum(a, red);
  b = wire_block_sum(b, red);
  if (threadIdx.x != 0) return;
  const float data = data_loss ? data_loss[0] : 0.f;
  out[0] = __fadd_rn(__fadd_rn(data, __fmul_rn(lambda_s, a)), __fmul_rn(lambda_t, b));
  out[1] = data;
  out[2] = a;
  out[3] = b;
}

// false: the sizes do not fit 63 bits (the largest offset is total - 1)
static bool tv_geom3(int H, int W, int T, int O, TvGeom3& g) {
  if (H < 1 || W < 1 || T < 1 || O < 1) return false;
  long long sw = (long long)T * O, sh, total;                         // T * O < 2^62
  if (__builtin_mul_overflow(sw, (long long)W, &sh) || __builtin_mul_overflow(sh, (long long)H, &total)) return false;
  g.total = total; g.sh = sh; g.sw = sw;
  g.H = H; g.W = W; g.T = T; g.O = O;
  return true;
}

// false: the sizes or the largest address do not fit 63 bits
static bool tv_geom(int planes, int H, int W, int64_t ps, int64_t qs, TvGeom& g) {
  if (planes < 1 || H < 1 || W < 1 || ps < 1 || qs < 1) return false;
  long long npix = (long long)H * W, total, a, b, last;               // H * W < 2^62
  if (__builtin_mul_overflow(npix, (long long)planes, &total)) return false;
  if (__builtin_mul_overflow(npix - 1, (long long)ps, &a) || __builtin_mul_overflow((long long)planes - 1, (long long)qs, &b) ||
      __builtin_add_overflow(a, b, &last))
    return false;
  g.npix = npix; g.total = total; g.ps = ps; g.qs = qs;
  g.H = H; g.W = W; g.planes = planes; g.plane_fast = qs < ps;
  return true;
}
static unsigned tv_blocks(long long n) { return n < (long long)TV_BLOCKS * 256 ? cdiv(n, 256) : TV_BLOCKS; }

bool tv_shape_ok(int planes, int H, int W, int64_t pix_stride, int64_t plane_stride) {
  TvGeom g;
  return tv_geom(planes, H, W, pix_stride, plane_stride, g);
}

hipError_t launch_tv_fwd(hipStream_t s, const float* x, int planes, int H, int W, int64_t pix_stride,
                         int64_t plane_stride, float* tv_out, float* partial) {
  TvGeom g;
  if (!tv_geom(planes, H, W, pix_stride, plane_stride, g)) return hipErrorInvalidValue;
  const unsigned nb = tv_blocks(g.npix);
  hipLaunchKernelGGL(tv_fwd_kernel, dim3(nb), dim3(256), 0, s, x, g, partial);
  hipLaunchKernelGGL(tv_final_kernel, dim3(1), dim3(256), 0, s, partial, (int)nb, -1, 0.f, 0.f, tv_out);
  return hipGetLastError();
}

hipError_t launch_tv_bwd(hipStream_t s, const float* x, int planes, int H, int W, int64_t pix_stride,
                         int64_t plane_stride, const float* g_tv, float* g_x) {
  TvGeom g;
  if (!tv_geom(planes, H, W, pix_stride, plane_stride, g)) return hipErrorInvalidValue;
  hipLaunchKernelGGL(tv_bwd_kernel, dim3(tv_blocks(g.total)), dim3(256), 0, s, x, g, g_tv, g_x);
  return hipGetLastError();
}

hipError_t launch_tv_mse_grad(hipStream_t s, const float* y, int H, int W, int O, const float* target,
                              const int64_t* idx, int64_t first, int64_t n_mse, float lambda_tv, float* g_y,
                              float* loss_out, float* rec, float* partial) {
  TvGeom g;
  if (!tv_geom(O, H, W, O, 1, g) || n_mse < 0 || n_mse > g.npix) return hipErrorInvalidValue;
  const double count = (double)n_mse * (double)O;
  const float gscale = n_mse ? (float)(2.0 / count) : 0.f, lscale = n_mse ? (float)(1.0 / count) : 0.f;
  const unsigned nb = tv_blocks(g.total);
  // a range is selected inside the one pass; rows given by idx get their MSE term in a second launch over those rows
  hipLaunchKernelGGL(tv_mse_grad_kernel, dim3(nb), dim3(256), 0, s, y, g, target, idx ? 0ll : (long long)first,
                     idx ? 0ll : (long long)n_mse, gscale, lambda_tv, g_y, rec, partial);
  int n_sq = (int)nb;
  if (idx) {
    n_sq = n_mse ? (int)tv_blocks(n_mse * O) : 0;
    if (n_mse)
      hipLaunchKernelGGL(tv_mse_rows_kernel, dim3((unsigned)n_sq), dim3(256), 0, s, y, O, target, idx,
                         (long long)n_mse, gscale, g_y, rec, partial);
  }
  hipLaunchKernelGGL(tv_final_kernel, dim3(1), dim3(256), 0, s, partial, (int)nb, n_sq, lscale, lambda_tv, loss_out);
  return hipGetLastError();
}

hipError_t launch_tv_add_grad(hipStream_t s, const float* y, int H, int W, int T, int O, float lambda_s,
                              float lambda_t, const float* data_loss, float* g_y, float* loss_out, float* partial) {
  TvGeom3 g;
  if (!tv_geom3(H, W, T, O, g)) return hipErrorInvalidValue;
  const unsigned nb = tv_blocks(g.total);
  hipLaunchKernelGGL(tv_add_grad_kernel, dim3(nb), dim3(256), 0, s, y, g, lambda_s, lambda_t, g_y, partial);
  hipLaunchKernelGGL(tv_add_final_kernel, dim3(1), dim3(256), 0, s, partial, (int)nb, lambda_s, lambda_t, data_loss,
                     loss_out);
  return hipGetLastError();
}

// ---------------------------------------------------------------------------
// entry points of the C ABI
// ---------------------------------------------------------------------------
extern "C" int wire_tv_fwd(void* stream, const float* x, int planes, int H, int W, int64_t pix_stride,
                           int64_t plane_stride, float* tv_out, float* partial) {
  if (!tv_shape_ok(planes, H, W, pix_stride, plane_stride) || !x || !tv_out || !partial)
    return fail(WIRE_ERR_ARG, "bad argument to wire_tv_fwd");
  ProfScope ps((hipStream_t)stream, 3, 0);
  HIPCHK(launch_tv_fwd((hipStream_t)stream, x, planes, H, W, pix_stride, plane_stride, tv_out, partial));
  return WIRE_OK;
}
extern "C" int wire_tv_bwd(void* stream, const float* x, int planes, int H, int W, int64_t pix_stride,
                           int64_t plane_stride, const float* g_tv, float* g_x) {
  if (!tv_shape_ok(planes, H, W, pix_stride, plane_stride) || !x || !g_tv || !g_x)
    return fail(WIRE_ERR_ARG, "bad argument to wire_tv_bwd");
  ProfScope ps((hipStream_t)stream, 3, 0);
  HIPCHK(launch_tv_bwd((hipStream_t)stream, x, planes, H, W, pix_stride, plane_stride, g_tv, g_x));
  return WIRE_OK;
}
extern "C" int wire_tv_mse_grad(void* stream, const float* y, int H, int W, int O, const float* target,
                                const int64_t* idx, int64_t first, int64_t n_mse, float lambda_tv, float* g_y,
                                float* loss_out, float* rec, float* partial) {
  const int64_t npix = (int64_t)H * W;
  if (O < 1 || O > WIRE_MAXO || !tv_shape_ok(O, H, W, O, 1) || n_mse < 0 || n_mse > npix ||
      (!idx && (first < 0 || first > npix - n_mse)) || !y || !target || !g_y || !loss_out || !partial)
    return fail(WIRE_ERR_ARG, "bad argument to wire_tv_mse_grad");
  ProfScope ps((hipStream_t)stream, 3, 0);
  HIPCHK(launch_tv_mse_grad((hipStream_t)stream, y, H, W, O, target, idx, first, n_mse, lambda_tv, g_y, loss_out, rec,
                            partial));
  return WIRE_OK;
}
extern "C" int wire_tv_add_grad(void* stream, const float* y, int H, int W, int T, int O, float lambda_s,
                                float lambda_t, const float* data_loss, float* g_y, float* loss_out, float* partial) {
  TvGeom3 g;
  if (O > WIRE_MAXO || !tv_geom3(H, W, T, O, g) || !__builtin_isfinite(lambda_s) || !__builtin_isfinite(lambda_t) ||
      !y || !g_y || !loss_out || !partial)
    return fail(WIRE_ERR_ARG, "bad argument to wire_tv_add_grad");
  ProfScope ps((hipStream_t)stream, 3, 0);
  HIPCHK(launch_tv_add_grad((hipStream_t)stream, y, H, W, T, O, lambda_s, lambda_t, data_loss, g_y, loss_out,
                            partial));
  return WIRE_OK;
}
