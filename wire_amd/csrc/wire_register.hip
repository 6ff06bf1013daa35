// wire_register.hip -- registering the frames of the multi-image super-resolution path on the device: a bilinear
// resampler (cv2.remap / F.grid_sample semantics) with its coordinate gradient, and one Gauss-Newton iteration of an
// intensity-based registration, batched over frames and start candidates.
//   out[p][c]  = bilinear(img, xy[p])[c]                                  (wire_remap_bilinear_fwd)
//   g_xy[p]    = sum_c g_out[p][c] d out_c / d (x, y)                     (wire_remap_bilinear_bwd_xy)
//   M[b][k]   <- M[b][k] + delta,  delta = -(J^T W J + damping diag)^-1 J^T W r     (wire_register_gn_step)
// for E(M) = sum_x w(x) (R(M (j, i, 1)) - F(i, j))^2, R the reference frame and F frame b.
//
// ARITHMETIC: wire_warp.hip's recipe.  Everything is evaluated in fp64 from the fp32 inputs with contraction off, left to
// right as written below, and a result that leaves as fp32 is rounded once: a numpy restatement reproduces the bits
// (tests/register_ref.py).  x0 = floor(x), fx = x - x0 (exact in fp64); with a, b, c, d the taps (x0, y0), (x0 + 1, y0),
// (x0, y0 + 1), (x0 + 1, y0 + 1), a tap outside the image being 0:
//   top = (1 - fx) a + fx b,  bot = (1 - fx) c + fx d,  v = (1 - fy) top + fy bot
//   dv/dx = (1 - fy) (b - a) + fy (d - c),  dv/dy = bot - top
// the derivative of the interpolant on the cell chosen by floor, so the right-hand derivative at integers.
//
// SHAPE: the two remap kernels are one thread per row, no reduction.  The registration is two launches:
//   reg_sums_kernel: a workgroup of 256 threads owns REG_CHUNK consecutive pixels of ONE (frame, candidate); a thread
//     adds its eight pixels, 256 apart, in order into 29 fp64 accumulators (21 of J^T W J, 6 of J^T W r, sum w r^2,
//     sum w), the wave adds them by wire_wave_sum's shuffle tree, the four waves through LDS as (w0 + w1) + (w2 + w3),
//     and the block stores 29 fp64 partials.  58 accumulator registers per thread fit the 256-thread budget of 256 VGPRs
//     without spilling; the kernel is bound by its gathers, not by the fp64 rate.
//   reg_solve_kernel: one workgroup per (frame, candidate).  Wave w owns sums w, w + 4, ...: lane l adds the partials of
//     chunks l, l + 64, ... in order, the wave adds its lanes by the same tree.  Thread 0 then projects the normal
//     equations onto the motion model, damps the diagonal, solves by Cholesky and writes the matrix and the stats.
// SUMS: which thread adds which term, and in which order, depends on (B, K, H, W) alone.  No atomics, no host
// synchronisation; every partial the second launch reads is written by the first, so the same call gives the same bits
// whatever ws held before.
//
// The entry points of the C ABI (include/wire_hip.h) are at the end of this file.
#include "wire_dev.h"
#include "wire_plan.h"

#define REG_CHUNK 2048           // pixels of one (frame, candidate) per workgroup of reg_sums_kernel: 8 per thread
#define REG_NSUM 29              // 21 + 6 + 1 + 1
#define REG_MAX_BLOCKS 2147483647ll
#define REG_MAX_C 8

// ---- the shared sampler ----------------------------------------------------------------------------------------
// The cell of pixel coordinate x (finite, floor(x) in int range) along an axis of n samples.  inside = true moves a
// coordinate that sits exactly on the last sample (x = n - 1) into the last cell INSIDE the image (i0 = n - 2,
// f = 1): the value is the same sample, the derivative the interior one -- what the registration wants of a pixel it
// counts as covered.  The resampler keeps floor's cell, whose right-hand tap is outside.
struct RegCell {
  int i0;
  double f;
};
WIRE_DEVINL RegCell reg_cell(double x, int n, bool inside) {
  const double fl = floor(x);
  RegCell c;
  c.i0 = (int)fl;
  c.f = x - fl;
  if (inside && c.i0 == n - 1) {
    c.i0 = n - 2;
    c.f = 1.0;
  }
  return c;
}
struct RegSample {
  double v, dx, dy;
};
// channel ch of img [H][W][C] on the cell (cx, cy); taps outside the image are 0
WIRE_DEVINL RegSample reg_bilinear(const float* __restrict__ img, int H, int W, int C, int ch, RegCell cx, RegCell cy) {
#pragma clang fp contract(off)
  const bool x0in = cx.i0 >= 0 && cx.i0 < W, x1in = cx.i0 + 1 >= 0 && cx.i0 + 1 < W;
  const bool y0in = cy.i0 >= 0 && cy.i0 < H, y1in = cy.i0 + 1 >= 0 && cy.i0 + 1 < H;
  const long long o = ((long long)cy.i0 * W + cx.i0) * C + ch, dy = (long long)W * C;
  const double a = (x0in && y0in) ? (double)img[o] : 0.0;
  const double b = (x1in && y0in) ? (double)img[o + C] : 0.0;
  const double c = (x0in && y1in) ? (double)img[o + dy] : 0.0;
  const double d = (x1in && y1in) ? (double)img[o + dy + C] : 0.0;
  const double gx = 1.0 - cx.f, gy = 1.0 - cy.f;
  const double top = gx * a + cx.f * b, bot = gx * c + cx.f * d;
  RegSample s;
  s.v = gy * top + cy.f * bot;
  s.dx = gy * (b - a) + cy.f * (d - c);
  s.dy = bot - top;
  return s;
}

// ---- the resampler ---------------------------------------------------------------------------------------------
// pixel coordinates of row r; false when no tap can lie inside the image (NaN and infinities included)
WIRE_DEVINL bool remap_pixel(float2 p, int H, int W, int normalized, double& x, double& y) {
#pragma clang fp contract(off)
  x = (double)p.x;
  y = (double)p.y;
  if (normalized) {
    x = ((x + 1.0) * (double)W - 1.0) * 0.5;
    y = ((y + 1.0) * (double)H - 1.0) * 0.5;
  }
  return x >= -1.0 && x < (double)W && y >= -1.0 && y < (double)H;
}

__global__ __launch_bounds__(256) void remap_fwd_kernel(const float* __restrict__ img, int H, int W, int C,
                                                        const float2* __restrict__ xy, long long n, int normalized,
                                                        float* __restrict__ out) {
  const long long r = (long long)blockIdx.x * 256 + threadIdx.x;
  if (r >= n) return;
  double x, y;
  const bool in = remap_pixel(xy[r], H, W, normalized, x, y);
  RegCell cx = {0, 0.0}, cy = {0, 0.0};
  if (in) {
    cx = reg_cell(x, W, false);
    cy = reg_cell(y, H, false);
  }
  for (int c = 0; c < C; ++c) out[r * C + c] = in ? (float)reg_bilinear(img, H, W, C, c, cx, cy).v : 0.f;
}

__global__ __launch_bounds__(256) void remap_bwd_xy_kernel(const float* __restrict__ img, int H, int W, int C,
                                                           const float2* __restrict__ xy,
                                                           const float* __restrict__ g_out, long long n,
                                                           int normalized, float2* __restrict__ g_xy) {
#pragma clang fp contract(off)
  const long long r = (long long)blockIdx.x * 256 + threadIdx.x;
  if (r >= n) return;
  double x, y;
  float2 g = {0.f, 0.f};
  if (remap_pixel(xy[r], H, W, normalized, x, y)) {
    const RegCell cx = reg_cell(x, W, false), cy = reg_cell(y, H, false);
    double sx = 0.0, sy = 0.0;
    for (int c = 0; c < C; ++c) {
      const RegSample s = reg_bilinear(img, H, W, C, c, cx, cy);
      const double gc = (double)g_out[r * C + c];
      sx = sx + gc * s.dx;
      sy = sy + gc * s.dy;
    }
    if (normalized) {
      sx = sx * ((double)W * 0.5);
      sy = sy * ((double)H * 0.5);
    }
    g.x = (float)sx;
    g.y = (float)sy;
  }
  g_xy[r] = g;
}

// ---- the registration: the 29 sums -----------------------------------------------------------------------------
// A pixel (i, j) of frame b counts when u = M (j, i, 1) lies in [0, W - 1] x [0, H - 1], its weight is not 0 and the
// frame's own value is not 0 -- exact zeros are the resampler's border fill, which the reference masks the same way
// (wire_multi_sr.py: masks = 1 - (imstack == 0); register_stack_ecc: spatial_mask = im2_aligned != 0).
__global__ __launch_bounds__(256) void reg_sums_kernel(const float* __restrict__ ref, const float* __restrict__ frames,
                                                       const float* __restrict__ weight, int K, int H, int W,
                                                       long long chunks, const double* __restrict__ mats,
                                                       double* __restrict__ partial) {
#pragma clang fp contract(off)
  __shared__ double red[4][REG_NSUM];
  const long long bk = blockIdx.x / chunks, ck = blockIdx.x - bk * chunks;
  const long long n = (long long)H * W, base = (bk / K) * n;
  const double* m = mats + bk * 6;
  const double m00 = m[0], m01 = m[1], m02 = m[2], m10 = m[3], m11 = m[4], m12 = m[5];
  const double xmax = (double)(W - 1), ymax = (double)(H - 1);
  double acc[REG_NSUM];
#pragma unroll
  for (int t = 0; t < REG_NSUM; ++t) acc[t] = 0.0;
#pragma unroll
  for (int r = 0; r < REG_CHUNK / 256; ++r) {
    const long long p = ck * REG_CHUNK + threadIdx.x + 256 * r;
    if (p >= n) continue;
    const int i = (int)(p / W), j = (int)(p - (long long)i * W);
    const double xj = (double)j, yi = (double)i;
    const double u = m00 * xj + m01 * yi + m02;
    const double v = m10 * xj + m11 * yi + m12;
    const float f = frames[base + p];
    const double w = weight ? (double)weight[base + p] : 1.0;
    if (!(u >= 0.0 && u <= xmax && v >= 0.0 && v <= ymax) || w == 0.0 || f == 0.f) continue;
    const RegSample s = reg_bilinear(ref, H, W, 1, 0, reg_cell(u, W, true), reg_cell(v, H, true));
    const double res = s.v - (double)f;
    const double J[6] = {s.dx * xj, s.dx * yi, s.dx, s.dy * xj, s.dy * yi, s.dy};
    int t = 0;
#pragma unroll
    for (int a = 0; a < 6; ++a) {
      const double wa = w * J[a];
#pragma unroll
      for (int b = a; b < 6; ++b) {
        acc[t] = acc[t] + wa * J[b];
        ++t;
      }
      acc[21 + a] = acc[21 + a] + wa * res;
    }
    acc[27] = acc[27] + (w * res) * res;
    acc[28] = acc[28] + w;
  }
#pragma unroll
  for (int t = 0; t < REG_NSUM; ++t) acc[t] = wire_wave_sum(acc[t]);
  if ((threadIdx.x & 63) == 0) {
#pragma unroll
    for (int t = 0; t < REG_NSUM; ++t) red[threadIdx.x >> 6][t] = acc[t];
  }
  __syncthreads();
  if (threadIdx.x < REG_NSUM)
    partial[(long long)blockIdx.x * REG_NSUM + threadIdx.x] =
        (red[0][threadIdx.x] + red[1][threadIdx.x]) + (red[2][threadIdx.x] + red[3][threadIdx.x]);
}

// ---- the registration: the solve -------------------------------------------------------------------------------
// Solves (A + damping diag A) delta = -g for the np parameters of the model, A = P^T H P, g = P^T (J^T W r), P the
// 6 x np Jacobian of the six matrix entries (m00 m01 m02 m10 m11 m12) with respect to the parameters:
//   translation (tx, ty): columns e2, e5;  Euclidean (angle, tx, ty): (-s, -c, 0, c, -s, 0), e2, e5;  affine: identity.
// false on a non-positive or non-finite pivot.
__device__ bool reg_solve(const double* S, int model, double damping, double cs, double sn, double* delta, int& np) {
#pragma clang fp contract(off)
  double Hm[6][6], P[6][6], T[6][6], A[6][6], g[6], L[6][6], y[6];
  int t = 0;
  for (int a = 0; a < 6; ++a)
    for (int b = a; b < 6; ++b) {
      Hm[a][b] = S[t];
      Hm[b][a] = S[t];
      ++t;
    }
  for (int a = 0; a < 6; ++a)
    for (int b = 0; b < 6; ++b) P[a][b] = 0.0;
  if (model == 0) {
    np = 2;
    P[2][0] = 1.0;
    P[5][1] = 1.0;
  } else if (model == 1) {
    np = 3;
    P[0][0] = -sn; P[1][0] = -cs; P[3][0] = cs; P[4][0] = -sn;
    P[2][1] = 1.0;
    P[5][2] = 1.0;
  } else {
    np = 6;
    for (int a = 0; a < 6; ++a) P[a][a] = 1.0;
  }
  for (int a = 0; a < 6; ++a)
    for (int q = 0; q < np; ++q) {
      double s = 0.0;
      for (int b = 0; b < 6; ++b) s = s + Hm[a][b] * P[b][q];
      T[a][q] = s;
    }
  for (int p = 0; p < np; ++p) {
    for (int q = 0; q < np; ++q) {
      double s = 0.0;
      for (int a = 0; a < 6; ++a) s = s + P[a][p] * T[a][q];
      A[p][q] = s;
    }
    double s = 0.0;
    for (int a = 0; a < 6; ++a) s = s + P[a][p] * S[21 + a];
    g[p] = s;
  }
  for (int p = 0; p < np; ++p) A[p][p] = A[p][p] + damping * A[p][p];
  for (int q = 0; q < np; ++q) {
    double d = A[q][q];
    for (int k = 0; k < q; ++k) d = d - L[q][k] * L[q][k];
    if (!(d > 0.0) || !isfinite(d)) return false;
    L[q][q] = sqrt(d);
    for (int p = q + 1; p < np; ++p) {
      double s = A[p][q];
      for (int k = 0; k < q; ++k) s = s - L[p][k] * L[q][k];
      L[p][q] = s / L[q][q];
    }
  }
  for (int p = 0; p < np; ++p) {
    double s = -g[p];
    for (int k = 0; k < p; ++k) s = s - L[p][k] * y[k];
    y[p] = s / L[p][p];
  }
  for (int p = np - 1; p >= 0; --p) {
    double s = y[p];
    for (int k = p + 1; k < np; ++k) s = s - L[k][p] * delta[k];
    delta[p] = s / L[p][p];
  }
  return true;
}

// block bk: sums[bk][t] = sum over the chunks of partial[bk][chunk][t]; thread 0 updates mats[bk] and writes stats[bk]
__global__ __launch_bounds__(256) void reg_solve_kernel(const double* __restrict__ partial, long long chunks, int H, int W,
                                                        int model, double damping, double min_cover,
                                                        double* __restrict__ mats, double* __restrict__ stats,
                                                        double* __restrict__ sums) {
#pragma clang fp contract(off)
  __shared__ double S[REG_NSUM];
  const int wave = threadIdx.x >> 6, lane = threadIdx.x & 63;
  for (int t = wave; t < REG_NSUM; t += 4) {
    const double* src = partial + (long long)blockIdx.x * chunks * REG_NSUM + t;
    double s = 0.0;
    for (long long c = lane; c < chunks; c += 64) s = s + src[c * REG_NSUM];
    s = wire_wave_sum(s);
    if (lane == 0) {
      S[t] = s;
      sums[(long long)blockIdx.x * REG_NSUM + t] = s;
    }
  }
  __syncthreads();
  if (threadIdx.x != 0) return;
  double* m = mats + (long long)blockIdx.x * 6;
  double* st = stats + (long long)blockIdx.x * 4;
  const double wsum = S[28];
  const double mean = wsum > 0.0 ? S[27] / wsum : 0.0;
  const double cover = wsum / ((double)H * (double)W);
  bool ok = wsum > 0.0 && isfinite(mean) && isfinite(cover) && cover >= min_cover;
  double delta[6], o[6], norm2 = 0.0;
  const double th = atan2(m[3], m[0]);
  int np = 0;
  if (ok) ok = reg_solve(S, model, damping, cos(th), sin(th), delta, np);
  if (ok) {
    for (int p = 0; p < np; ++p) norm2 = norm2 + delta[p] * delta[p];
    for (int a = 0; a < 6; ++a) o[a] = m[a];
    if (model == 0) {
      o[2] = m[2] + delta[0];
      o[5] = m[5] + delta[1];
    } else if (model == 1) {
      const double tn = th + delta[0], c = cos(tn), s = sin(tn);
      o[0] = c; o[1] = -s; o[2] = m[2] + delta[1];
      o[3] = s; o[4] = c;  o[5] = m[5] + delta[2];
    } else {
      for (int a = 0; a < 6; ++a) o[a] = m[a] + delta[a];
    }
    for (int a = 0; a < 6; ++a) ok = ok && isfinite(o[a]);
    ok = ok && isfinite(norm2);
  }
  if (ok)
    for (int a = 0; a < 6; ++a) m[a] = o[a];
  st[0] = mean;
  st[1] = cover;
  st[2] = ok ? sqrt(norm2) : 0.0;
  st[3] = ok ? 1.0 : 0.0;
}

// ---------------------------------------------------------------------------
// entry points of the C ABI
// ---------------------------------------------------------------------------
static bool reg_aligned8(const void* p) { return ((uintptr_t)p & 7) == 0; }

// blocks of the one-thread-per-row kernels; false when a size does not fit 63 bits or the grid
static bool remap_geom(int H, int W, int C, int64_t n, int normalized, long long& blocks) {
  if (H < 1 || W < 1 || C < 1 || C > REG_MAX_C || n < 1 || (normalized != 0 && normalized != 1)) return false;
  long long bytes;
  if (__builtin_mul_overflow((long long)n, 4ll * C, &bytes)) return false;                    // [n][C] floats
  blocks = ((long long)n - 1) / 256 + 1;
  return blocks <= REG_MAX_BLOCKS;
}

extern "C" int wire_remap_bilinear_fwd(void* stream, const float* img, int H, int W, int C, const float* xy, int64_t n,
                                       int normalized, float* out) {
  long long blocks;
  if (!remap_geom(H, W, C, n, normalized, blocks) || !img || !xy || !out || !reg_aligned8(xy))
    return fail(WIRE_ERR_ARG, "bad argument to wire_remap_bilinear_fwd");
  ProfScope ps((hipStream_t)stream, 3, 0);
  hipLaunchKernelGGL(remap_fwd_kernel, dim3((unsigned)blocks), dim3(256), 0, (hipStream_t)stream, img, H, W, C,
                     (const float2*)xy, (long long)n, normalized, out);
  HIPCHK(hipGetLastError());
  return WIRE_OK;
}

extern "C" int wire_remap_bilinear_bwd_xy(void* stream, const float* img, int H, int W, int C, const float* xy,
                                          const float* g_out, int64_t n, int normalized, float* g_xy) {
  long long blocks;
  if (!remap_geom(H, W, C, n, normalized, blocks) || !img || !xy || !g_out || !g_xy || !reg_aligned8(xy) ||
      !reg_aligned8(g_xy))
    return fail(WIRE_ERR_ARG, "bad argument to wire_remap_bilinear_bwd_xy");
  ProfScope ps((hipStream_t)stream, 3, 0);
  hipLaunchKernelGGL(remap_bwd_xy_kernel, dim3((unsigned)blocks), dim3(256), 0, (hipStream_t)stream, img, H, W, C,
                     (const float2*)xy, g_out, (long long)n, normalized, (float2*)g_xy);
  HIPCHK(hipGetLastError());
  return WIRE_OK;
}

// The geometry of a registration call: false when a size does not fit 63 bits or a grid does not hold the blocks.
struct RegGeom {
  long long bk, chunks, blocks, ws_bytes;
};
static bool reg_geom(int B, int K, int H, int W, RegGeom& g) {
  if (B < 1 || K < 1 || H < 1 || W < 1) return false;
  g.bk = (long long)B * K;                                               // < 2^62
  g.chunks = ((long long)H * W - 1) / REG_CHUNK + 1;
  long long doubles;
  if (__builtin_mul_overflow(g.bk, g.chunks, &g.blocks) || g.blocks > REG_MAX_BLOCKS || g.bk > REG_MAX_BLOCKS)
    return false;
  doubles = (g.blocks + g.bk) * REG_NSUM;                                // the sums, then the partials
  g.ws_bytes = doubles * (long long)sizeof(double);
  return true;
}

extern "C" int64_t wire_register_gn_ws_bytes(int B, int K, int H, int W) {
  RegGeom g;
  if (!reg_geom(B, K, H, W, g)) return fail(WIRE_ERR_ARG, "bad argument to wire_register_gn_ws_bytes");
  return g.ws_bytes;
}

extern "C" int wire_register_gn_step(void* stream, const float* ref, const float* frames, const float* weight, int B,
                                     int K, int H, int W, int model, double damping, double min_cover, double* mats,
                                     double* stats, void* ws, int64_t ws_bytes) {
  RegGeom g;
  if (!reg_geom(B, K, H, W, g) || model < 0 || model > 2 || !(damping >= 0.0) || !(damping <= 1e300) ||
      !(min_cover >= 0.0) || !(min_cover <= 1e300) || !ref || !frames || !mats || !stats || !ws || !reg_aligned8(mats) ||
      !reg_aligned8(stats) || !reg_aligned8(ws))
    return fail(WIRE_ERR_ARG, "bad argument to wire_register_gn_step");
  if (ws_bytes < g.ws_bytes) return fail(WIRE_ERR_SIZE, "wire_register_gn_step: ws too small");
  ProfScope ps((hipStream_t)stream, 3, 0);
  double* sums = (double*)ws;
  double* partial = sums + g.bk * REG_NSUM;
  hipLaunchKernelGGL(reg_sums_kernel, dim3((unsigned)g.blocks), dim3(256), 0, (hipStream_t)stream, ref, frames, weight,
                     K, H, W, g.chunks, (const double*)mats, partial);
  hipLaunchKernelGGL(reg_solve_kernel, dim3((unsigned)g.bk), dim3(256), 0, (hipStream_t)stream, (const double*)partial,
                     g.chunks, H, W, model, damping, min_cover, mats, stats, sums);
  HIPCHK(hipGetLastError());
  return WIRE_OK;
}
