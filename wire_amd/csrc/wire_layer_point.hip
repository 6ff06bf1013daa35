// wire_layer_point.hip -- what only the per-layer API (wire_layer_api.hip) uses: layout conversion between torch's
// tensors and the blocked rows, the elementwise activation gradients, and the sums behind a trainable omega_0 / scale_0.
#include "wire_dev.h"
#include "wire_point.h"

// ===========================================================================
// layout conversion (per-layer API only; the fused path never leaves the
// blocked layout)
// ===========================================================================
__global__ void c64_to_blocked_kernel(const float* __restrict__ src, long long n, int K, int P,
                                      float* __restrict__ dst) {
  const long long row = blockIdx.x;
  for (int c = threadIdx.x; c < P; c += blockDim.x) {
    int o, part;
    blk_decode(c, o, part);
    dst[row * P + c] = o < K ? src[(row * K + o) * 2 + part] : 0.f;
  }
}
__global__ void blocked_to_c64_kernel(const float* __restrict__ src, long long n, int K, int P,
                                      float* __restrict__ dst) {
  const long long row = blockIdx.x;
  for (int e = threadIdx.x; e < 2 * K; e += blockDim.x) {
    const int o = e >> 1, part = e & 1;
    dst[row * 2 * K + e] = src[row * P + blk_col(o, part)];
  }
}
__global__ void pad_rows_kernel(const float* __restrict__ src, long long n, int K, int P,
                                float* __restrict__ dst) {
  const long long row = blockIdx.x;
  for (int c = threadIdx.x; c < P; c += blockDim.x) dst[row * P + c] = c < K ? src[row * K + c] : 0.f;
}
__global__ void unpad_rows_kernel(const float* __restrict__ src, long long n, int K, int P,
                                  float* __restrict__ dst) {
  const long long row = blockIdx.x;
  for (int c = threadIdx.x; c < K; c += blockDim.x) dst[row * K + c] = src[row * P + c];
}

hipError_t launch_c64_to_blocked(hipStream_t s, const float* src, int64_t n, int K, int P, float* dst) {
  if (n <= 0) return hipSuccess;
  hipLaunchKernelGGL(c64_to_blocked_kernel, dim3((unsigned)n), dim3(256), 0, s, src, (long long)n, K, P, dst);
  return hipGetLastError();
}
hipError_t launch_blocked_to_c64(hipStream_t s, const float* src, int64_t n, int K, int P, float* dst) {
  if (n <= 0) return hipSuccess;
  hipLaunchKernelGGL(blocked_to_c64_kernel, dim3((unsigned)n), dim3(256), 0, s, src, (long long)n, K, P, dst);
  return hipGetLastError();
}
hipError_t launch_pad_rows(hipStream_t s, const float* src, int64_t n, int K, int P, float* dst) {
  if (n <= 0) return hipSuccess;
  hipLaunchKernelGGL(pad_rows_kernel, dim3((unsigned)n), dim3(256), 0, s, src, (long long)n, K, P, dst);
  return hipGetLastError();
}
hipError_t launch_unpad_rows(hipStream_t s, const float* src, int64_t n, int K, int P, float* dst) {
  if (n <= 0) return hipSuccess;
  hipLaunchKernelGGL(unpad_rows_kernel, dim3((unsigned)n), dim3(256), 0, s, src, (long long)n, K, P, dst);
  return hipGetLastError();
}

// ---------------------------------------------------------------------------
// elementwise Gabor gradient (per-layer API; the fused path does this inside
// the data-gradient GEMM's epilogue)
// ---------------------------------------------------------------------------
__global__ void gabor_bwd_point_kernel(const float* __restrict__ g, const float* __restrict__ lin,
                                       const float* __restrict__ out, long long n, int P, float omega,
                                       float scale, float* __restrict__ g_lin) {
  const long long row = blockIdx.x;
  const float m2s2 = -2.f * scale * scale;
  for (int f = threadIdx.x; f < (P >> 1); f += blockDim.x) {
    const size_t c = (size_t)row * P + blk_col(f, 0);
    float gl_re, gl_im;
    gabor_bwd(g[c], g[c + 32], lin[c], lin[c + 32], out[c], out[c + 32], omega, m2s2, gl_re, gl_im);
    g_lin[c] = gl_re;
    g_lin[c + 32] = gl_im;
  }
}
__global__ void gabor_bwd_first_point_kernel(const float* __restrict__ g, const float* __restrict__ out,
                                             const float* __restrict__ coords, int D,
                                             const float* __restrict__ W0, const float* __restrict__ b0,
                                             long long n, int K, int P, float omega, float scale,
                                             float* __restrict__ g_u, int ldu) {
  const long long row = blockIdx.x;
  const float m2s2 = -2.f * scale * scale;
  for (int f = threadIdx.x; f < ldu; f += blockDim.x) {
    float gu = 0.f;
    if (f < K) {
      float u = b0[f];
      for (int d = 0; d < D; ++d) u = __builtin_fmaf(coords[row * D + d], W0[f * D + d], u);
      const size_t c = (size_t)row * P + blk_col(f, 0);
      gu = gabor_bwd_real(g[c], g[c + 32], u, out[c], out[c + 32], omega, m2s2);
    }
    g_u[row * ldu + f] = gu;
  }
}
// 2-D Gabor (modules/wire2d.py:56-67) activation gradient for the per-layer API.
// g, out: [n][P] blocked planar; linsy, g_linsy: [n][2P] in 128-column groups (u | v | p | q) of 32 features.
//   c = conj(out) g, t = -2 s0^2 Re c:  g_lin = t lin - j w0 c,  g_sy = t sy
__global__ void gabor2d_bwd_point_kernel(const float* __restrict__ g, const float* __restrict__ linsy,
                                         const float* __restrict__ out, long long n, int P, float omega,
                                         float scale, float* __restrict__ g_linsy) {
  const long long row = blockIdx.x;
  const float m2s2 = -2.f * scale * scale;
  for (int f = threadIdx.x; f < (P >> 1); f += blockDim.x) {
    const size_t oc = (size_t)row * P + blk_col(f, 0);
    const size_t lc = (size_t)row * 2 * P + ((f >> 5) << 7) + (f & 31);
    const float gr = g[oc], gi = g[oc + 32], pr = out[oc], pi = out[oc + 32];
    const float c_r = __builtin_fmaf(pr, gr, pi * gi);
    const float c_i = __builtin_fmaf(pr, gi, -(pi * gr));
    const float t = m2s2 * c_r;
    g_linsy[lc] = __builtin_fmaf(t, linsy[lc], omega * c_i);
    g_linsy[lc + 32] = __builtin_fmaf(t, linsy[lc + 32], -(omega * c_r));
    g_linsy[lc + 64] = t * linsy[lc + 64];
    g_linsy[lc + 96] = t * linsy[lc + 96];
  }
}
// real first layer of wire2d: u = W0 x + b0, p = V0 x + c0;  g_u = t u + w0 Im c,  g_p = t p;  g_up [n][2 ldu]
__global__ void gabor2d_bwd_first_point_kernel(const float* __restrict__ g, const float* __restrict__ out,
                                               const float* __restrict__ coords, int D,
                                               const float* __restrict__ W0, const float* __restrict__ b0,
                                               const float* __restrict__ V0, const float* __restrict__ c0,
                                               long long n, int K, int P, float omega, float scale,
                                               float* __restrict__ g_up, int ldu) {
  const long long row = blockIdx.x;
  const float m2s2 = -2.f * scale * scale;
  for (int f = threadIdx.x; f < ldu; f += blockDim.x) {
    float gu = 0.f, gp = 0.f;
    if (f < K) {
      float u = b0[f], pp = c0[f];
      for (int d = 0; d < D; ++d) {
        const float x = coords[row * D + d];
        u = __builtin_fmaf(x, W0[f * D + d], u);
        pp = __builtin_fmaf(x, V0[f * D + d], pp);
      }
      const size_t c = (size_t)row * P + blk_col(f, 0);
      const float gr = g[c], gi = g[c + 32], pr = out[c], pi = out[c + 32];
      const float c_r = __builtin_fmaf(pr, gr, pi * gi);
      const float c_i = __builtin_fmaf(pr, gi, -(pi * gr));
      const float t = m2s2 * c_r;
      gu = __builtin_fmaf(t, u, omega * c_i);
      gp = t * pp;
    }
    g_up[row * 2 * ldu + f] = gu;
    g_up[row * 2 * ldu + ldu + f] = gp;
  }
}
hipError_t launch_gabor2d_bwd_point(hipStream_t s, const float* g, const float* linsy, const float* out,
                                    int64_t n, int P, float omega, float scale, float* g_linsy) {
  if (n <= 0) return hipSuccess;
  hipLaunchKernelGGL(gabor2d_bwd_point_kernel, dim3((unsigned)n), dim3(256), 0, s, g, linsy, out, (long long)n, P,
                     omega, scale, g_linsy);
  return hipGetLastError();
}
hipError_t launch_gabor2d_bwd_first_point(hipStream_t s, const float* g, const float* out, const float* coords,
                                          int D, const float* W0, const float* b0, const float* V0,
                                          const float* c0, int64_t n, int K, int P, float omega, float scale,
                                          float* g_up, int ldu) {
  if (n <= 0) return hipSuccess;
  hipLaunchKernelGGL(gabor2d_bwd_first_point_kernel, dim3((unsigned)n), dim3(256), 0, s, g, out, coords, D, W0,
                     b0, V0, c0, (long long)n, K, P, omega, scale, g_up, ldu);
  return hipGetLastError();
}
template <int ACT>
__global__ void real_act_bwd_point_kernel(const float* __restrict__ g, const float* __restrict__ lin,
                                          const float* __restrict__ out, long long n, int P, float omega,
                                          float scale, float* __restrict__ g_lin) {
  const long long row = blockIdx.x;
  for (int c = threadIdx.x; c < P; c += blockDim.x) {
    const size_t i = (size_t)row * P + c;
    g_lin[i] = real_act_bwd<ACT>(g[i], lin[i], out[i], omega, scale);
  }
}
hipError_t launch_real_act_bwd_point(hipStream_t s, int kind, const float* g, const float* lin,
                                     const float* out, int64_t n, int P, float omega, float scale,
                                     float* g_lin) {
  if (n <= 0) return hipSuccess;
  dim3 grid((unsigned)n), blk(256);
  return with_kind(kind, [&](auto k) -> hipError_t {
    if constexpr (kind_is_real(decltype(k)::value)) {
      hipLaunchKernelGGL(real_act_bwd_point_kernel<nk_real_act(decltype(k)::value)>, grid, blk, 0, s, g, lin, out,
                         (long long)n, P, omega, scale, g_lin);
      return hipGetLastError();
    } else {
      return hipErrorInvalidValue;
    }
  });
}
hipError_t launch_gabor_bwd_point(hipStream_t s, const float* g, const float* lin, const float* out,
                                  int64_t n, int P, float omega, float scale, float* g_lin) {
  if (n <= 0) return hipSuccess;
  hipLaunchKernelGGL(gabor_bwd_point_kernel, dim3((unsigned)n), dim3(256), 0, s, g, lin, out,
                     (long long)n, P, omega, scale, g_lin);
  return hipGetLastError();
}
hipError_t launch_gabor_bwd_first_point(hipStream_t s, const float* g, const float* out,
                                        const float* coords, int D, const float* W0, const float* b0,
                                        int64_t n, int K, int P, float omega, float scale, float* g_u,
                                        int ldu) {
  if (n <= 0) return hipSuccess;
  hipLaunchKernelGGL(gabor_bwd_first_point_kernel, dim3((unsigned)n), dim3(256), 0, s, g, out, coords,
                     D, W0, b0, (long long)n, K, P, omega, scale, g_u, ldu);
  return hipGetLastError();
}

// ===========================================================================
// trainable omega_0 / scale_0 of a ComplexGaborLayer (modules/wire.py:80-81, trainable=True):
//   out = exp(j w0 lin - s0^2 |lin|^2)  =>  d out / d w0 = j lin out,  d out / d s0 = -2 s0 |lin|^2 out
// and with c = conj(out) g (g = dL/dRe + j dL/dIm):
//   dL/dw0 = sum Re(conj(g) j lin out) = sum (lin_re c_im - lin_im c_re),   dL/ds0 = -2 s0 sum |lin|^2 Re c.
// lin: complex rows [n][P] blocked planar, or (is_first) real u [n][P/2]; g, out [n][P] blocked planar.
// Two-stage deterministic reduction: partial[2][nblk] then one block.
// ===========================================================================
#define HP_ROWS 32
__global__ __launch_bounds__(256) void gabor_hparam_partial_kernel(const float* __restrict__ g,
                                                                   const float* __restrict__ lin,
                                                                   const float* __restrict__ out, long long n, int K,
                                                                   int P, int is_first, float* __restrict__ partial) {
  __shared__ float red[2][256];
  const long long r0 = (long long)blockIdx.x * HP_ROWS;
  long long r1 = r0 + HP_ROWS;
  if (r1 > n) r1 = n;
  float aw = 0.f, as = 0.f;
  for (long long row = r0; row < r1; ++row)
    for (int f = threadIdx.x; f < K; f += 256) {
      const size_t c = (size_t)row * P + blk_col(f, 0);
      const float gr = g[c], gi = g[c + 32], pr = out[c], pi = out[c + 32];
      float lr, li;
      if (is_first) { lr = lin[(size_t)row * (P >> 1) + f]; li = 0.f; }
      else { lr = lin[c]; li = lin[c + 32]; }
      const float c_r = __builtin_fmaf(pr, gr, pi * gi);
      const float c_i = __builtin_fmaf(pr, gi, -(pi * gr));
      aw += __builtin_fmaf(lr, c_i, -(li * c_r));
      as += __builtin_fmaf(lr, lr, li * li) * c_r;
    }
  red[0][threadIdx.x] = aw;
  red[1][threadIdx.x] = as;
  __syncthreads();
  for (int sft = 128; sft >= 1; sft >>= 1) {
    if ((int)threadIdx.x < sft) {
      red[0][threadIdx.x] += red[0][threadIdx.x + sft];
      red[1][threadIdx.x] += red[1][threadIdx.x + sft];
    }
    __syncthreads();
  }
  if (threadIdx.x == 0) {
    partial[blockIdx.x] = red[0][0];
    partial[gridDim.x + blockIdx.x] = red[1][0];
  }
}
__global__ __launch_bounds__(256) void gabor_hparam_final_kernel(const float* __restrict__ partial, int nblk,
                                                                 float scale, float* __restrict__ out2) {
  __shared__ float red[2][256];
  float aw = 0.f, as = 0.f;
  for (int b = threadIdx.x; b < nblk; b += 256) { aw += partial[b]; as += partial[nblk + b]; }
  red[0][threadIdx.x] = aw;
  red[1][threadIdx.x] = as;
  __syncthreads();
  for (int sft = 128; sft >= 1; sft >>= 1) {
    if ((int)threadIdx.x < sft) {
      red[0][threadIdx.x] += red[0][threadIdx.x + sft];
      red[1][threadIdx.x] += red[1][threadIdx.x + sft];
    }
    __syncthreads();
  }
  if (threadIdx.x == 0) {
    out2[0] = red[0][0];
    out2[1] = -2.f * scale * red[1][0];
  }
}
// the same for ComplexGaborLayer2D (modules/wire2d.py:56-67): out = exp(j w0 lin) exp(-s0^2 (|lin|^2 + |sy|^2))
//   d out / d w0 = j lin out,  d out / d s0 = -2 s0 (|lin|^2 + |sy|^2) out.
// linsy: [n][2P] in 128-column groups (u | v | p | q), or (is_first) real (u | p) [n][2 * P/2].
__global__ __launch_bounds__(256) void gabor2d_hparam_partial_kernel(const float* __restrict__ g,
                                                                     const float* __restrict__ linsy,
                                                                     const float* __restrict__ out, long long n, int K,
                                                                     int P, int is_first, float* __restrict__ partial) {
  __shared__ float red[2][256];
  const long long r0 = (long long)blockIdx.x * HP_ROWS;
  long long r1 = r0 + HP_ROWS;
  if (r1 > n) r1 = n;
  const int Kp = P >> 1;
  float aw = 0.f, as = 0.f;
  for (long long row = r0; row < r1; ++row)
    for (int f = threadIdx.x; f < K; f += 256) {
      const size_t c = (size_t)row * P + blk_col(f, 0);
      const float gr = g[c], gi = g[c + 32], pr = out[c], pi = out[c + 32];
      float u, v = 0.f, pp, qq = 0.f;
      if (is_first) {
        u = linsy[(size_t)row * (2 * Kp) + f];
        pp = linsy[(size_t)row * (2 * Kp) + Kp + f];
      } else {
        const float* L = linsy + (size_t)row * (2 * P) + ((f >> 5) << 7) + (f & 31);
        u = L[0]; v = L[32]; pp = L[64]; qq = L[96];
      }
      const float c_r = __builtin_fmaf(pr, gr, pi * gi);
      const float c_i = __builtin_fmaf(pr, gi, -(pi * gr));
      aw += __builtin_fmaf(u, c_i, -(v * c_r));
      as += (__builtin_fmaf(u, u, v * v) + __builtin_fmaf(pp, pp, qq * qq)) * c_r;
    }
  red[0][threadIdx.x] = aw;
  red[1][threadIdx.x] = as;
  __syncthreads();
  for (int sft = 128; sft >= 1; sft >>= 1) {
    if ((int)threadIdx.x < sft) {
      red[0][threadIdx.x] += red[0][threadIdx.x + sft];
      red[1][threadIdx.x] += red[1][threadIdx.x + sft];
    }
    __syncthreads();
  }
  if (threadIdx.x == 0) {
    partial[blockIdx.x] = red[0][0];
    partial[gridDim.x + blockIdx.x] = red[1][0];
  }
}
int hparam_blocks(int64_t n) { return (int)((n + HP_ROWS - 1) / HP_ROWS); }
hipError_t launch_gabor2d_hparam_grad(hipStream_t s, const float* g, const float* linsy, const float* out, int64_t n,
                                      int K, int P, int is_first, float scale, float* partial, float* out2) {
  if (n <= 0) return hipErrorInvalidValue;
  const int nblk = (int)((n + HP_ROWS - 1) / HP_ROWS);
  hipLaunchKernelGGL(gabor2d_hparam_partial_kernel, dim3((unsigned)nblk), dim3(256), 0, s, g, linsy, out, (long long)n,
                     K, P, is_first, partial);
  hipLaunchKernelGGL(gabor_hparam_final_kernel, dim3(1), dim3(256), 0, s, partial, nblk, scale, out2);
  return hipGetLastError();
}
hipError_t launch_gabor_hparam_grad(hipStream_t s, const float* g, const float* lin, const float* out, int64_t n,
                                    int K, int P, int is_first, float scale, float* partial, float* out2) {
  if (n <= 0) return hipErrorInvalidValue;
  const int nblk = hparam_blocks(n);
  hipLaunchKernelGGL(gabor_hparam_partial_kernel, dim3((unsigned)nblk), dim3(256), 0, s, g, lin, out, (long long)n,
                     K, P, is_first, partial);
  hipLaunchKernelGGL(gabor_hparam_final_kernel, dim3(1), dim3(256), 0, s, partial, nblk, scale, out2);
  return hipGetLastError();
}
