// wire_warp.hip -- a learnable registration of B frames: one 2 x 3 matrix theta[f] per frame acting on the frame's
// NORMALISED coordinates (the convention of motion.get_transformed_coords / F.affine_grid, modules/motion.py), and its
// adjoint.  The layer between per-frame registration parameters and the rows the network evaluates:
//   out[f][p] = theta[f] (x, y, 1)^T                                   (wire_warp_coords_fwd)
//   g_theta[f][a][c] = sum_p g_out[f][p][a] v_c,  v = (x, y, 1)        (wire_warp_coords_bwd)
//   g_in[f][p] = theta[f][:, :2]^T g_out[f][p]                         (optional)
// Everything is evaluated in fp64 and rounded to fp32 once, with contraction off, as affine_coords_kernel
// (wire_train.hip) evaluates the frames' coordinates: a numpy restatement reproduces the bits, and the identity matrix
// returns its input bit for bit (1 x + 0 y + 0 is exact).
//
// SHAPE: both kernels are one thread per row with one 8-byte load per operand and one 8-byte store; they move
// 16 B (forward) and 16 - 24 B (backward) per row and compute next to nothing, so they are bound by the launch and, at
// the driver's 1.6 M rows, by HBM.
//   warp_fwd_kernel: a flat grid over the B * n_per rows; a thread reads its row before it writes it, so out may be
//     coords.
//   warp_bwd_kernel: a workgroup of 256 threads owns WARP_CHUNK consecutive rows of ONE frame (block b -> frame
//     b / chunks, chunk b % chunks: a block never straddles frames).  A thread adds its rows, 256 apart, into six fp64
//     accumulators -- each product of two fp32 values is exact in fp64 -- the wave adds them by __shfl_xor in a fixed
//     tree, the four waves through LDS as (w0 + w1) + (w2 + w3), and the block stores six fp64 partials to
//     ws[f][chunk][6].
//   warp_final_kernel: one workgroup of six waves per frame, wave k owning entry k: lane l adds the partials of chunks
//     l, l + 64, ... in that order, the wave adds its lanes by the same tree, and the sum is rounded to fp32 once.
//     pin_first writes +0.0 over frame 0 here.
// SUMS: which thread adds which term, and in which order, depends on (B, n_per) alone.  No atomics and no
// last-block-done counter: the same call gives the same bits, whatever ws held before (every partial that the second
// launch reads is written by the first).
//
// The three entry points of the C ABI (include/wire_hip.h) are at the end of this file.
#include "wire_dev.h"
#include "wire_plan.h"

#define WARP_CHUNK 2048          // rows of one frame per workgroup of warp_bwd_kernel: 8 per thread
#define WARP_MAX_BLOCKS 2147483647ll

__global__ __launch_bounds__(256) void warp_fwd_kernel(const float2* coords, const float* __restrict__ theta,
                                                       long long n, long long n_per, float2* out) {
#pragma clang fp contract(off)
  const long long r = (long long)blockIdx.x * 256 + threadIdx.x;
  if (r >= n) return;
  const float* t = theta + (r / n_per) * 6;
  const float2 v = coords[r];
  const double x = (double)v.x, y = (double)v.y;
  float2 o;
  o.x = (float)((double)t[0] * x + (double)t[1] * y + (double)t[2]);
  o.y = (float)((double)t[3] * x + (double)t[4] * y + (double)t[5]);
  out[r] = o;
}

__global__ __launch_bounds__(256) void warp_bwd_kernel(const float2* __restrict__ coords,
                                                       const float* __restrict__ theta,
                                                       const float2* __restrict__ g_out, long long n_per,
                                                       long long chunks, float2* __restrict__ g_in,
                                                       double* __restrict__ partial) {
#pragma clang fp contract(off)
  __shared__ double red[4][6];
  const long long f = blockIdx.x / chunks, c = blockIdx.x - f * chunks;
  const long long p0 = c * WARP_CHUNK;
  const long long p1 = p0 + WARP_CHUNK < n_per ? p0 + WARP_CHUNK : n_per;
  const long long base = f * n_per;
  const float* t = theta + f * 6;
  const double t00 = (double)t[0], t01 = (double)t[1], t10 = (double)t[3], t11 = (double)t[4];
  double acc[6] = {0.0, 0.0, 0.0, 0.0, 0.0, 0.0};
  for (long long p = p0 + threadIdx.x; p < p1; p += 256) {
    const float2 v = coords[base + p], g = g_out[base + p];
    const double x = (double)v.x, y = (double)v.y, gx = (double)g.x, gy = (double)g.y;
    acc[0] += gx * x; acc[1] += gx * y; acc[2] += gx;
    acc[3] += gy * x; acc[4] += gy * y; acc[5] += gy;
    if (g_in) {
      float2 o;
      o.x = (float)(t00 * gx + t10 * gy);
      o.y = (float)(t01 * gx + t11 * gy);
      g_in[base + p] = o;
    }
  }
#pragma unroll
  for (int k = 0; k < 6; ++k) acc[k] = wire_wave_sum(acc[k]);
  if ((threadIdx.x & 63) == 0) {
#pragma unroll
    for (int k = 0; k < 6; ++k) red[threadIdx.x >> 6][k] = acc[k];
  }
  __syncthreads();
  if (threadIdx.x < 6)
    partial[(long long)blockIdx.x * 6 + threadIdx.x] =
        (red[0][threadIdx.x] + red[1][threadIdx.x]) + (red[2][threadIdx.x] + red[3][threadIdx.x]);
}

// block f, wave k: g_theta[f][k] = (float) sum over the frame's chunks of partial[f][chunk][k]
__global__ __launch_bounds__(384) void warp_final_kernel(const double* __restrict__ partial, long long chunks,
                                                         int pin_first, float* __restrict__ g_theta) {
  const int k = threadIdx.x >> 6, lane = threadIdx.x & 63;
  const double* src = partial + (long long)blockIdx.x * chunks * 6 + k;
  double s = 0.0;
  for (long long c = lane; c < chunks; c += 64) s += src[c * 6];
  s = wire_wave_sum(s);
  if (lane == 0) g_theta[(long long)blockIdx.x * 6 + k] = (pin_first && blockIdx.x == 0) ? 0.f : (float)s;
}

// The geometry of a call: false when a size does not fit 63 bits or a grid does not hold the blocks.
struct WarpGeom {
  long long n, chunks, fwd_blocks, bwd_blocks;
};
static bool warp_geom(int B, int64_t n_per, WarpGeom& g) {
  if (B < 1 || n_per < 1) return false;
  long long n, bytes;
  if (__builtin_mul_overflow((long long)B, (long long)n_per, &n) || __builtin_mul_overflow(n, 8ll, &bytes))
    return false;                                                      // [B][n_per][2] floats
  g.n = n;
  g.chunks = (n_per - 1) / WARP_CHUNK + 1;
  g.fwd_blocks = (n - 1) / 256 + 1;
  g.bwd_blocks = (long long)B * g.chunks;                              // <= n: no overflow
  return g.fwd_blocks <= WARP_MAX_BLOCKS && g.bwd_blocks <= WARP_MAX_BLOCKS;
}
static bool warp_aligned8(const void* p) { return ((uintptr_t)p & 7) == 0; }

// ---------------------------------------------------------------------------
// entry points of the C ABI
// ---------------------------------------------------------------------------
extern "C" int wire_warp_coords_fwd(void* stream, const float* coords, const float* theta, int B, int64_t n_per,
                                    float* out) {
  WarpGeom g;
  if (!warp_geom(B, n_per, g) || !coords || !theta || !out || !warp_aligned8(coords) || !warp_aligned8(out))
    return fail(WIRE_ERR_ARG, "bad argument to wire_warp_coords_fwd");
  ProfScope ps((hipStream_t)stream, 3, 0);
  hipLaunchKernelGGL(warp_fwd_kernel, dim3((unsigned)g.fwd_blocks), dim3(256), 0, (hipStream_t)stream,
                     (const float2*)coords, theta, g.n, (long long)n_per, (float2*)out);
  HIPCHK(hipGetLastError());
  return WIRE_OK;
}

extern "C" int64_t wire_warp_coords_bwd_ws_bytes(int B, int64_t n_per) {
  WarpGeom g;
  if (!warp_geom(B, n_per, g)) return fail(WIRE_ERR_ARG, "bad argument to wire_warp_coords_bwd_ws_bytes");
  return g.bwd_blocks * 6 * (int64_t)sizeof(double);
}

extern "C" int wire_warp_coords_bwd(void* stream, const float* coords, const float* theta, const float* g_out, int B,
                                    int64_t n_per, int pin_first, float* g_theta, float* g_in, void* ws,
                                    int64_t ws_bytes) {
  WarpGeom g;
  if (!warp_geom(B, n_per, g) || (pin_first != 0 && pin_first != 1) || !coords || !theta || !g_out || !g_theta || !ws ||
      !warp_aligned8(coords) || !warp_aligned8(g_out) || !warp_aligned8(g_in) || !warp_aligned8(ws))
    return fail(WIRE_ERR_ARG, "bad argument to wire_warp_coords_bwd");
  if (ws_bytes < g.bwd_blocks * 6 * (int64_t)sizeof(double))
    return fail(WIRE_ERR_SIZE, "wire_warp_coords_bwd: ws too small");
  ProfScope ps((hipStream_t)stream, 3, 0);
  hipLaunchKernelGGL(warp_bwd_kernel, dim3((unsigned)g.bwd_blocks), dim3(256), 0, (hipStream_t)stream,
                     (const float2*)coords, theta, (const float2*)g_out, (long long)n_per, g.chunks, (float2*)g_in,
                     (double*)ws);
  hipLaunchKernelGGL(warp_final_kernel, dim3((unsigned)B), dim3(384), 0, (hipStream_t)stream, (const double*)ws,
                     g.chunks, pin_first, g_theta);
  HIPCHK(hipGetLastError());
  return WIRE_OK;
}
