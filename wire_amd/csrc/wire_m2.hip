// wire_m2.hip -- the scale combiner of the multi-pass B-spline net (modules/bspline_mscale_2.py:
// AdaptiveScaleCombiner.freq_mlp in its 'freq_combine' mode) and the pass sum of its coordinate gradient.
//
//   x_r = [t_0(r) | t_1(r) | ... | t_{S-1}(r)]   (S.O features: the trunk's outputs of row r in pass order)
//   h_r = W1 x_r + b1 (128), a_r = relu(h_r), y_r = W2 a_r + b2 (O)
//
// The trunk's outputs are stored pass-major, t [S][n][O] (pass k of row r at (k n + r) O), which is the row
// order of the trunk's buffers (wire_api.hip).  The backward reads x again and recomputes h; its weight gradients
// go through per-block partials and a fixed-order reduce: no float atomics, the same bits on every run.
#include "wire_dev.h"
#include "wire_point.h"

#define M2_MAXSO (M2_MAX_SCALES * 8)   // S.O <= 8 x 8
#define M2_ROWS 16                     // rows of one backward tile

int m2_comb_blocks(int64_t n) {
  const int64_t t = (n + M2_ROWS - 1) / M2_ROWS;
  return (int)(t < M2_COMB_MAXBLK ? (t < 1 ? 1 : t) : M2_COMB_MAXBLK);
}

// the weights in LDS: W1 [128][SO], b1 [128], W2 [O][128], b2 [O]
struct M2Lds { float w1[M2_H * M2_MAXSO]; float b1[M2_H]; float w2[8 * M2_H]; float b2[8]; };
WIRE_DEVINL void m2_load_weights(M2Lds& L, const M2Comb& w, int SO, int O) {
  for (int i = threadIdx.x; i < M2_H * SO; i += blockDim.x) L.w1[i] = w.W1[i];
  for (int i = threadIdx.x; i < M2_H; i += blockDim.x) L.b1[i] = w.b1[i];
  for (int i = threadIdx.x; i < O * M2_H; i += blockDim.x) L.w2[i] = w.W2[i];
  if (threadIdx.x < O) L.b2[threadIdx.x] = w.b2[threadIdx.x];
}

// ---- forward: one thread per row
__global__ __launch_bounds__(256) void m2_comb_fwd_kernel(M2Comb w, int S, int O, const float* __restrict__ t,
                                                          long long n, float* __restrict__ y) {
  __shared__ M2Lds L;
  const int SO = S * O;
  m2_load_weights(L, w, SO, O);
  __syncthreads();
  const long long r = (long long)blockIdx.x * blockDim.x + threadIdx.x;
  if (r >= n) return;
  float x[M2_MAXSO];                                   // (static indices only: x stays in registers)
#pragma unroll
  for (int m = 0; m < M2_MAXSO; ++m) {
    x[m] = 0.f;
    if (m < SO) {
      const int k = m / O, o = m - k * O;
      x[m] = t[((long long)k * n + r) * O + o];
    }
  }
  float acc[8];
#pragma unroll
  for (int o = 0; o < 8; ++o) acc[o] = o < O ? L.b2[o] : 0.f;
  for (int j = 0; j < M2_H; ++j) {
    float h = L.b1[j];
    const float* wr = L.w1 + j * SO;
#pragma unroll
    for (int m = 0; m < M2_MAXSO; ++m)
      if (m < SO) h = __builtin_fmaf(wr[m], x[m], h);
    const float a = h > 0.f ? h : 0.f;
#pragma unroll
    for (int o = 0; o < 8; ++o)
      if (o < O) acc[o] = __builtin_fmaf(L.w2[o * M2_H + j], a, acc[o]);
  }
#pragma unroll
  for (int o = 0; o < 8; ++o)
    if (o < O) y[r * O + o] = acc[o];
}

hipError_t launch_m2_comb_fwd(hipStream_t s, const M2Comb& w, int S, int O, const float* t, int64_t n, float* y) {
  if (n <= 0) return hipSuccess;
  if (S < 1 || S > M2_MAX_SCALES || O < 1 || O > 8) return hipErrorInvalidValue;
  hipLaunchKernelGGL(m2_comb_fwd_kernel, dim3(cdiv(n, 256)), dim3(256), 0, s, w, S, O, t, (long long)n, y);
  return hipGetLastError();
}

// ---- backward (with the forward and the MSE in front of it when a target is given)
// Tiles of M2_ROWS rows, grid-strided over the blocks (a fixed assignment).  Per tile: x, h, a = relu(h) and (loss mode)
// y, the loss terms, g_y = gscale (y - target); then g_h = (W2^T g_y) [h > 0], g_x = W1^T g_h -> g_t.  Thread i owns the
// weight-gradient entries i, i + 256, ... of the flat [gW1 | gb1 | gW2 | gb2] and sums them over its block's rows in row
// order; the block writes them to part[block][G] and its loss partial to loss_part[block].  Rows past n carry g_y = 0
// and add nothing.
template <int GQ>
__global__ __launch_bounds__(256) void m2_comb_bwd_kernel(M2Comb w, int S, int O, const float* __restrict__ t,
                                                          long long n, M2Loss ls, const float* __restrict__ g_y_in,
                                                          float* __restrict__ g_t, float* __restrict__ part,
                                                          float* __restrict__ loss_part) {
  __shared__ M2Lds L;
  __shared__ float xs[M2_ROWS][M2_MAXSO];
  __shared__ float gys[M2_ROWS][8];
  __shared__ float as[M2_ROWS][M2_H];
  __shared__ float ghs[M2_ROWS][M2_H];
  __shared__ float red[256];
  const int SO = S * O, tid = threadIdx.x;
  const int G = m2_comb_grad_floats(S, O);
  m2_load_weights(L, w, SO, O);
  float acc[GQ];
#pragma unroll
  for (int q = 0; q < GQ; ++q) acc[q] = 0.f;
  float lacc = 0.f;
  const long long ntiles = (n + M2_ROWS - 1) / M2_ROWS;
  for (long long tile = blockIdx.x; tile < ntiles; tile += gridDim.x) {
    const long long r0 = tile * M2_ROWS;
    __syncthreads();                                   // (the weights; the previous tile's readers)
    for (int i = tid; i < M2_ROWS * SO; i += 256) {
      const int rr = i / SO, m = i - rr * SO, k = m / O, o = m - k * O;
      const long long row = r0 + rr;
      xs[rr][m] = row < n ? t[((long long)k * n + row) * O + o] : 0.f;
    }
    if (!ls.target)
      for (int i = tid; i < M2_ROWS * 8; i += 256) {
        const int rr = i / 8, o = i % 8;
        const long long row = r0 + rr;
        gys[rr][o] = (row < n && o < O) ? g_y_in[row * O + o] : 0.f;
      }
    __syncthreads();
    const int j = tid & (M2_H - 1), rq = tid >> 7;     // unit j of rows rq, rq + 2, ...
    for (int rr = rq; rr < M2_ROWS; rr += 2) {
      float h = L.b1[j];
      for (int m = 0; m < SO; ++m) h = __builtin_fmaf(L.w1[j * SO + m], xs[rr][m], h);
      as[rr][j] = h > 0.f ? h : 0.f;
    }
    if (ls.target) {                                   // y, the loss terms and g_y of the tile
      __syncthreads();
      if (tid < M2_ROWS * 8) {
        const int rr = tid / 8, o = tid % 8;
        const long long row = r0 + rr;
        float g = 0.f;
        if (row < n && o < O) {
          float yv = L.b2[o];
          for (int jj = 0; jj < M2_H; ++jj) yv = __builtin_fmaf(L.w2[o * M2_H + jj], as[rr][jj], yv);
          const long long src = ls.idx ? ls.idx[row] : ls.first + row;
          const float d = yv - ls.target[src * O + o];
          g = ls.gscale * d;
          lacc = __builtin_fmaf(d, d, lacc);
          ls.y[row * O + o] = yv;
          if (ls.g_y) ls.g_y[row * O + o] = g;
          if (ls.rec) ls.rec[src * O + o] = yv;
        }
        gys[rr][o] = g;
      }
    }
    __syncthreads();
    for (int rr = rq; rr < M2_ROWS; rr += 2) {
      float g = 0.f;
      if (as[rr][j] > 0.f)
        for (int o = 0; o < O; ++o) g = __builtin_fmaf(L.w2[o * M2_H + j], gys[rr][o], g);
      ghs[rr][j] = g;
    }
    __syncthreads();
    for (int i = tid; i < M2_ROWS * SO; i += 256) {   // g_x -> the trunk's output gradients
      const int rr = i / SO, m = i - rr * SO, k = m / O, o = m - k * O;
      const long long row = r0 + rr;
      if (row < n) {
        float g = 0.f;
        for (int jj = 0; jj < M2_H; ++jj) g = __builtin_fmaf(L.w1[jj * SO + m], ghs[rr][jj], g);
        g_t[((long long)k * n + row) * O + o] = g;
      }
    }
    if (part) {
#pragma unroll
      for (int q = 0; q < GQ; ++q) {
        const int e = tid + 256 * q;
        if (e < G) {
          float a = acc[q];
          if (e < M2_H * SO) {                           // gW1[j][m] = sum g_h[j] x[m]
            const int jj = e / SO, m = e - jj * SO;
            for (int rr = 0; rr < M2_ROWS; ++rr) a = __builtin_fmaf(ghs[rr][jj], xs[rr][m], a);
          } else if (e < M2_H * SO + M2_H) {             // gb1[j] = sum g_h[j]
            const int jj = e - M2_H * SO;
            for (int rr = 0; rr < M2_ROWS; ++rr) a += ghs[rr][jj];
          } else if (e < M2_H * SO + M2_H + O * M2_H) {  // gW2[o][j] = sum g_y[o] a[j]
            const int f = e - M2_H * SO - M2_H, o = f / M2_H, jj = f - o * M2_H;
            for (int rr = 0; rr < M2_ROWS; ++rr) a = __builtin_fmaf(gys[rr][o], as[rr][jj], a);
          } else {                                       // gb2[o] = sum g_y[o]
            const int o = e - M2_H * SO - M2_H - O * M2_H;
            for (int rr = 0; rr < M2_ROWS; ++rr) a += gys[rr][o];
          }
          acc[q] = a;
        }
      }
    }
  }
  if (part) {
#pragma unroll
    for (int q = 0; q < GQ; ++q) {
      const int e = tid + 256 * q;
      if (e < G) part[(long long)blockIdx.x * G + e] = acc[q];
    }
  }
  if (ls.target && loss_part) {
    __syncthreads();
    lacc = wire_block_tree_sum(lacc, red);
    if (tid == 0) loss_part[blockIdx.x] = lacc;
  }
}

// the blocks' partials in block order -> gW1, gb1, gW2, gb2
__global__ __launch_bounds__(256) void m2_comb_reduce_kernel(const float* __restrict__ part, int nblk, int S, int O,
                                                             M2Grads g) {
  const int SO = S * O, G = m2_comb_grad_floats(S, O);
  const int e = blockIdx.x * blockDim.x + threadIdx.x;
  if (e >= G) return;
  float a = 0.f;
#pragma unroll 16                                     // (the loads ahead of the adds; the adds stay in block order)
  for (int b = 0; b < nblk; ++b) a += part[(long long)b * G + e];
  if (e < M2_H * SO) g.W1[e] = a;
  else if (e < M2_H * SO + M2_H) g.b1[e - M2_H * SO] = a;
  else if (e < M2_H * SO + M2_H + O * M2_H) g.W2[e - M2_H * SO - M2_H] = a;
  else g.b2[e - M2_H * SO - M2_H - O * M2_H] = a;
}

hipError_t launch_m2_comb_bwd(hipStream_t s, const M2Comb& w, int S, int O, const float* t, int64_t n, const M2Loss& ls,
                              const float* g_y, float* g_t, float* part, float* loss_part) {
  if (n <= 0) return hipSuccess;
  if (S < 1 || S > M2_MAX_SCALES || O < 1 || O > 8 || (!ls.target && !g_y)) return hipErrorInvalidValue;
  const int G = m2_comb_grad_floats(S, O), nblk = m2_comb_blocks(n);
#define M2B(GQ_) hipLaunchKernelGGL((m2_comb_bwd_kernel<GQ_>), dim3(nblk), dim3(256), 0, s, w, S, O, t, (long long)n, ls, \
                                    g_y, g_t, part, loss_part)
  if (G <= 8 * 256) M2B(8);
  else if (G <= 16 * 256) M2B(16);
  else M2B(37);                                        // G <= 128 x 64 + 128 + 8 x 128 + 8 = 9352 < 37 x 256
#undef M2B
  return hipGetLastError();
}

hipError_t launch_m2_comb_reduce(hipStream_t s, const float* part, int64_t n, int S, int O, const M2Grads& g) {
  if (n <= 0) return hipSuccess;
  const int G = m2_comb_grad_floats(S, O);
  hipLaunchKernelGGL(m2_comb_reduce_kernel, dim3(cdiv(G, 256)), dim3(256), 0, s, part, m2_comb_blocks(n), S, O, g);
  return hipGetLastError();
}

// ---- out[i] = sum over the passes k, in order, of g[k n D + i]
__global__ __launch_bounds__(256) void m2_sum_passes_kernel(const float* __restrict__ g, int S, long long nd,
                                                            float* __restrict__ out) {
  const long long i = (long long)blockIdx.x * blockDim.x + threadIdx.x;
  if (i >= nd) return;
  float a = g[i];
  for (int k = 1; k < S; ++k) a += g[(long long)k * nd + i];
  out[i] = a;
}
hipError_t launch_m2_sum_passes(hipStream_t s, const float* g, int S, int64_t n, int D, float* out) {
  const int64_t nd = n * D;
  if (nd <= 0) return hipSuccess;
  hipLaunchKernelGGL(m2_sum_passes_kernel, dim3(cdiv(nd, 256)), dim3(256), 0, s, g, S, (long long)nd, out);
  return hipGetLastError();
}
