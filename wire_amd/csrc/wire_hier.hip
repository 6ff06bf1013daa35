// wire_hier.hip -- the point kernels of the hierarchical B-spline net (modules/bspline_mscale_hier.py,
// WIRE_KIND_BSPLINE_HIER): what its stages need around the GEMMs and the existing kernels have no form for.
//
//   stage s:  x_in = B(c_s (coords W0^T + b0))                       hier_first_fwd_kernel (writes with a leading dimension:
//             x_1  = B(c_s ([x_in | x_{s-1}] W1^T + b1))             the left half of the join's [n][2P] input)
//             x_s  = B(c_s (x_1 W2^T + b2))
//   y = sum_s (x_s Wh_s^T + bh_s)                                    hier_head_fwd_kernel, one stage per launch, in order
//
// Backward of a head: g_lin_last(s) = (g_y Wh_s) c_s B'(c_s lin) + T, T = the right half of stage s + 1's join data
// gradient (already multiplied by c_s B'(c_s lin) by that GEMM's epilogue); gWh_s = g_y^T x_s through per-block partials
// in final_bwd_kernel's layout (launch_final_reduce adds them up).  The join's weight W1 [K][2K] is packed with its two
// halves at columns [0, K) and [P, P + K) of a [P][2P] image; its gradient comes back out of [P][2P] slabs the same way.
// No float atomics except the monotone max-|value| slots: every sum runs in a fixed order.
#include "wire_dev.h"
#include "wire_point.h"

#define HIER_FIRST_ROWS 64

// ---- first layer of a stage: one thread per feature, 64 rows per block; pad features are written as 0
__global__ void hier_first_fwd_kernel(const float* __restrict__ coords, long long n, int D, const float* __restrict__ W0,
                                      const float* __restrict__ b0, int K, int P, float c, float* __restrict__ lin,
                                      float* __restrict__ out, int ldo, unsigned* __restrict__ amax_out) {
  const int f = blockIdx.y * blockDim.x + threadIdx.x;
  const bool live = f < P, valid = f < K;
  float w[4] = {0.f, 0.f, 0.f, 0.f}, bb = 0.f, amx = 0.f;
  if (valid) {
    bb = b0[f];
    for (int d = 0; d < D; ++d) w[d] = W0[f * D + d];
  }
  const long long r0 = (long long)blockIdx.x * HIER_FIRST_ROWS;
  long long r1 = r0 + HIER_FIRST_ROWS;
  if (r1 > n) r1 = n;
  for (long long row = r0; row < r1; ++row) {
    float u = bb;
    for (int d = 0; d < D; ++d) u = __builtin_fmaf(coords[row * D + d], w[d], u);
    const float o = valid ? bspline2(c * u) : 0.f;
    amx = __builtin_fmaxf(amx, o);
    if (live) {
      if (lin) lin[row * P + f] = valid ? u : 0.f;
      out[row * (long long)ldo + f] = o;
    }
  }
  if (amax_out) wire_amax_publish(amax_out, amx, threadIdx.x & 63);
}

hipError_t launch_hier_first_fwd(hipStream_t s, const float* coords, int64_t n, int D, const float* W0, const float* b0,
                                 int K, int P, float c, float* lin, float* out, int ldo, unsigned* amax_out) {
  if (n <= 0) return hipSuccess;
  if (D < 1 || D > 4 || ldo < P) return hipErrorInvalidValue;
  const int bx = P >= 256 ? 256 : P;   // P is a multiple of 64
  hipLaunchKernelGGL(hier_first_fwd_kernel, dim3(cdiv(n, HIER_FIRST_ROWS), cdiv(P, bx)), dim3(bx), 0, s, coords,
                     (long long)n, D, W0, b0, K, P, c, lin, out, ldo, amax_out);
  return hipGetLastError();
}

// ---- one head: y = (acc ? y : 0) + (x Wh^T + bh), one wave per row, Wh [O][K] staged zero-padded to [O][P] in LDS.
// ls.target (the last head of a training step): the MSE terms of the finished y, g_y = gscale (y - target), the optional
// scatter, and the block's sum of squares in loss_part[block]
__global__ __launch_bounds__(256) void hier_head_fwd_kernel(const float* __restrict__ x, int ldx,
                                                            const float* __restrict__ Wh, const float* __restrict__ bh,
                                                            long long n, int K, int P, int O, int acc,
                                                            float* __restrict__ y, M2Loss ls,
                                                            float* __restrict__ loss_part) {
  extern __shared__ __attribute__((aligned(16))) float sw[];   // [O][P]
  __shared__ float red[4];
  for (int i = threadIdx.x; i < O * P; i += blockDim.x) {
    const int o = i / P, c = i - o * P;
    sw[i] = c < K ? Wh[(size_t)o * K + c] : 0.f;
  }
  __syncthreads();
  const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
  const long long wstride = (long long)gridDim.x * 4;
  float lacc = 0.f;
  for (long long row = (long long)blockIdx.x * 4 + wave; row < n; row += wstride) {
    float a[WIRE_MAXO];
#pragma unroll
    for (int o = 0; o < WIRE_MAXO; ++o) a[o] = 0.f;
    const float* xr = x + row * (long long)ldx;
    for (int c = lane * 4; c < P; c += 256) {
      const f32x4 xv = *reinterpret_cast<const f32x4*>(xr + c);
#pragma unroll
      for (int o = 0; o < WIRE_MAXO; ++o)
        if (o < O) {
          const f32x4 wv = *reinterpret_cast<const f32x4*>(&sw[o * P + c]);
          a[o] += xv[0] * wv[0] + xv[1] * wv[1] + xv[2] * wv[2] + xv[3] * wv[3];
        }
    }
#pragma unroll
    for (int o = 0; o < WIRE_MAXO; ++o)
      if (o < O) {
        float v = a[o];
#pragma unroll
        for (int sft = 32; sft >= 1; sft >>= 1) v += __shfl_xor(v, sft);
        if (lane == o) {
          v += bh[o];
          if (acc) v = y[row * O + o] + v;
          y[row * O + o] = v;
          if (ls.target) {
            const long long src = ls.idx ? ls.idx[row] : ls.first + row;
            const float d = v - ls.target[src * O + o];
            lacc = __builtin_fmaf(d, d, lacc);
            if (ls.g_y) ls.g_y[row * O + o] = ls.gscale * d;
            if (ls.rec) ls.rec[src * O + o] = v;
          }
        }
      }
  }
  if (ls.target && loss_part) {   // lanes 0 .. O - 1 of each wave hold terms: lane order, then wave order
#pragma unroll
    for (int sft = 32; sft >= 1; sft >>= 1) lacc += __shfl_xor(lacc, sft);
    if (lane == 0) red[wave] = lacc;
    __syncthreads();
    if (threadIdx.x == 0) loss_part[blockIdx.x] = (red[0] + red[1]) + (red[2] + red[3]);
  }
}

int hier_head_blocks(int64_t n) {
  const int64_t b = (n + 3) / 4;
  return (int)(b < 1 ? 1 : b > HIER_HEAD_MAXBLK ? HIER_HEAD_MAXBLK : b);
}
hipError_t launch_hier_head_fwd(hipStream_t s, const float* x, int ldx, const float* Wh, const float* bh, int64_t n, int K,
                                int P, int O, int acc, float* y, const M2Loss& ls, float* loss_part) {
  if (n <= 0) return hipSuccess;
  if (O < 1 || O > WIRE_MAXO || (P & 3) || (ldx & 3) || (size_t)O * P * sizeof(float) > 65536) return hipErrorInvalidValue;
  hipLaunchKernelGGL(hier_head_fwd_kernel, dim3(hier_head_blocks(n)), dim3(256), (size_t)O * P * sizeof(float), s, x, ldx,
                     Wh, bh, (long long)n, K, P, O, acc, y, ls, loss_part);
  return hipGetLastError();
}

// ---- backward of one head: blocks of WIRE_FB_ROWS rows, one thread per feature.
//   part_w != null: the block's partial of gWh = g_y^T x (part_w[block][O][P]) and of gbh (part_b[block][O])
//   g_lin != null:  g_lin[row][f] = (sum_o g_y[row][o] Wh[o][f]) c B'(c lin[row][f]) + (add ? add[row][f] : 0), 0 in the
//                   pad features, and its max |value|
__global__ __launch_bounds__(256) void hier_head_bwd_kernel(const float* __restrict__ g_y, long long n, int O,
                                                            const float* __restrict__ Wh, const float* __restrict__ x,
                                                            int ldx, const float* __restrict__ lin,
                                                            const float* __restrict__ add, int K, int P, float c,
                                                            float* __restrict__ g_lin, float* __restrict__ part_w,
                                                            float* __restrict__ part_b, unsigned* __restrict__ amax_g) {
  __shared__ float sgy[WIRE_FB_ROWS * WIRE_MAXO];
  const long long r0 = (long long)blockIdx.x * WIRE_FB_ROWS;
  long long r1 = r0 + WIRE_FB_ROWS;
  if (r1 > n) r1 = n;
  const int nr = (int)(r1 - r0);
  for (int i = threadIdx.x; i < nr * O; i += blockDim.x) sgy[i] = g_y[r0 * O + i];
  __syncthreads();
  const int f = blockIdx.y * blockDim.x + threadIdx.x;
  float amx = 0.f;
  if (f < P) {
    const bool valid = f < K;
    float w[WIRE_MAXO], a[WIRE_MAXO];
#pragma unroll
    for (int o = 0; o < WIRE_MAXO; ++o) {
      a[o] = 0.f;
      w[o] = (o < O && valid) ? Wh[(size_t)o * K + f] : 0.f;
    }
    // rows in batches of 8: every load of a batch is issued before its first use (as final_bwd_kernel does; a per-row
    // load -> use -> store chain runs at a third of the bandwidth)
    constexpr int RB = 8;
    for (int rb = 0; rb < nr; rb += RB) {
      float xv[RB], lv[RB], av[RB];
#pragma unroll
      for (int q = 0; q < RB; ++q) {
        const long long row = r0 + (rb + q < nr ? rb + q : nr - 1);   // clamped: tail rows re-read the last one
        xv[q] = part_w ? x[row * (long long)ldx + f] : 0.f;
        lv[q] = g_lin ? lin[row * P + f] : 0.f;
        av[q] = (g_lin && add) ? add[row * P + f] : 0.f;
      }
#pragma unroll
      for (int q = 0; q < RB; ++q) {
        const int r = rb + q;
        if (r < nr) {
          float gr = 0.f;
#pragma unroll
          for (int o = 0; o < WIRE_MAXO; ++o)
            if (o < O) {
              const float g = sgy[r * O + o];
              gr = __builtin_fmaf(g, w[o], gr);
              a[o] = __builtin_fmaf(g, xv[q], a[o]);
            }
          if (g_lin) {
            float gl = gr * c * bspline2_d(c * lv[q]) + av[q];
            gl = valid ? gl : 0.f;
            g_lin[(r0 + r) * P + f] = gl;
            amx = __builtin_fmaxf(amx, __builtin_fabsf(gl));
          }
        }
      }
    }
    if (part_w) {
      float* pw = part_w + (size_t)blockIdx.x * O * P;
#pragma unroll
      for (int o = 0; o < WIRE_MAXO; ++o)
        if (o < O) pw[(size_t)o * P + f] = a[o];
    }
  }
  if (part_b && blockIdx.y == 0 && threadIdx.x < O) {
    float sacc = 0.f;
    for (int r = 0; r < nr; ++r) sacc += sgy[r * O + threadIdx.x];
    part_b[(size_t)blockIdx.x * O + threadIdx.x] = sacc;
  }
  if (amax_g) wire_amax_publish(amax_g, amx, threadIdx.x & 63);
}

hipError_t launch_hier_head_bwd(hipStream_t s, const float* g_y, int64_t n, int O, const float* Wh, const float* x, int ldx,
                                const float* lin, const float* add, int K, int P, float c, float* g_lin, float* part_w,
                                float* part_b, unsigned* amax_g) {
  if (n <= 0) return hipSuccess;
  if (O < 1 || O > WIRE_MAXO || (!g_lin && !part_w) || (g_lin && !lin) || (part_w && (!x || !part_b)))
    return hipErrorInvalidValue;
  hipLaunchKernelGGL(hier_head_bwd_kernel, dim3((unsigned)final_bwd_blocks(n), cdiv(P, 256)), dim3(256), 0, s, g_y,
                     (long long)n, O, Wh, x, ldx, lin, add, K, P, c, g_lin, part_w, part_b, amax_g);
  return hipGetLastError();
}

// ---- the join's weight W [K][2K] (x_in columns first) -> its forward image [P][2P] (columns [0, K) and [P, P + K), zero
// elsewhere), its bias [P], and the two halves as contiguous [K][K] matrices (packed like hidden layers for the two
// data-gradient GEMMs)
__global__ void hier_pack_join_kernel(const float* __restrict__ W, const float* __restrict__ b, int K, int P,
                                      float* __restrict__ fwd, float* __restrict__ bias, float* __restrict__ Wa,
                                      float* __restrict__ Wb) {
  const int k = blockIdx.x * blockDim.x + threadIdx.x;   // column of the image
  const int j = blockIdx.y;                              // output feature
  if (k >= 2 * P) return;
  const int half = k >= P ? 1 : 0, kk = k - half * P;
  float v = 0.f;
  if (j < K && kk < K) {
    v = W[(size_t)j * 2 * K + half * K + kk];
    (half ? Wb : Wa)[(size_t)j * K + kk] = v;
  }
  fwd[(size_t)j * 2 * P + k] = v;
  if (k == 0) bias[j] = j < K ? b[j] : 0.f;
}
hipError_t launch_hier_pack_join(hipStream_t s, const float* W, const float* b, int K, int P, float* fwd, float* bias,
                                 float* Wa, float* Wb) {
  hipLaunchKernelGGL(hier_pack_join_kernel, dim3(cdiv(2 * P, 128), (unsigned)P), dim3(128), 0, s, W, b, K, P, fwd, bias, Wa,
                     Wb);
  return hipGetLastError();
}

// ---- the join's weight gradient out of the TN GEMM's slabs [S][P][2P] (+ bslab [S][P]): the splits in order
__global__ __launch_bounds__(256) void hier_join_reduce_kernel(const float* __restrict__ slab, const float* __restrict__ bslab,
                                                               int S, int K, int P, float* __restrict__ gW,
                                                               float* __restrict__ gb) {
  const int j = blockIdx.x * blockDim.x + threadIdx.x;   // native column, 0 .. 2K - 1
  const int o = blockIdx.y;
  if (j < 2 * K) {
    const int col = j < K ? j : P + (j - K);
    const size_t sstride = (size_t)P * 2 * P;
    const float* m = slab + (size_t)o * 2 * P + col;
    float a = 0.f;
#pragma unroll 8
    for (int sp = 0; sp < S; ++sp) a += m[sp * sstride];
    gW[(size_t)o * 2 * K + j] = a;
  }
  if (j == 0) {
    float a = 0.f;
    for (int sp = 0; sp < S; ++sp) a += bslab[(size_t)sp * P + o];
    gb[o] = a;
  }
}
hipError_t launch_hier_join_reduce(hipStream_t s, const float* slab, const float* bslab, int S, int K, int P, float* gW,
                                   float* gb) {
  hipLaunchKernelGGL(hier_join_reduce_kernel, dim3(cdiv(2 * K, 256), (unsigned)K), dim3(256), 0, s, slab, bslab, S, K, P,
                     gW, gb);
  return hipGetLastError();
}
