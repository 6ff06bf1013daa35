// wire_first.hip -- what touches the input coordinates: the first layer (D <= 4 inputs), the positional encoding, the
// frozen first stage of the multi-scale B-spline net, and the way back to the coordinates (coordinate gradients, the
// positional encoding's backward).
#include "wire_dev.h"
#include "wire_point.h"

// ===========================================================================
// first layer: coords [n][D] (D <= 4) -> activations.  One thread per output
// feature, 64 rows per block: W0 row in registers, coordinates broadcast.
// ===========================================================================
#define FIRST_ROWS 64
template <int KIND>
__global__ void first_fwd_kernel(const float* __restrict__ coords, long long n, int D,
                                 const float* __restrict__ W0, const float* __restrict__ b0,
                                 const float* __restrict__ V0, const float* __restrict__ c0, int K,
                                 int P, float omega, float scale, float* __restrict__ lin,
                                 float* __restrict__ out, unsigned* __restrict__ amax_out) {
  constexpr bool cplx = (KIND == NK_WIRE || KIND == NK_WIRE2D);
  const int nfeat = cplx ? (P >> 1) : P;
  const int f = blockIdx.y * blockDim.x + threadIdx.x;
  const bool live = f < nfeat;                  // (no early return: the maximum below is a whole-wave reduction)
  const bool valid = f < K;
  float amx = 0.f;
  float w[4] = {0.f, 0.f, 0.f, 0.f}, wv[4] = {0.f, 0.f, 0.f, 0.f};
  float bb = 0.f, bv = 0.f;
  if (valid) {
    bb = b0[f];
    for (int d = 0; d < D; ++d) w[d] = W0[f * D + d];
    if (KIND == NK_WIRE2D) {
      bv = c0[f];
      for (int d = 0; d < D; ++d) wv[d] = V0[f * D + d];
    }
  }
  const long long r0 = (long long)blockIdx.x * FIRST_ROWS;
  long long r1 = r0 + FIRST_ROWS;
  if (r1 > n) r1 = n;
  const int c_re = cplx ? blk_col(f, 0) : f;
  for (long long row = r0; row < r1; ++row) {
    float u = bb, p = bv;
    for (int d = 0; d < D; ++d) {
      const float x = coords[row * D + d];
      u = __builtin_fmaf(x, w[d], u);
      if (KIND == NK_WIRE2D) p = __builtin_fmaf(x, wv[d], p);
    }
    if (KIND == NK_WIRE) {
      float o_re, o_im;
      gabor_fwd_real(u, omega, scale, o_re, o_im);
      o_re = valid ? o_re : 0.f; o_im = valid ? o_im : 0.f;
      amx = __builtin_fmaxf(amx, __builtin_fmaxf(__builtin_fabsf(o_re), __builtin_fabsf(o_im)));
      if (live) {
        out[row * P + c_re] = o_re;
        out[row * P + c_re + 32] = o_im;
        if (lin) lin[row * nfeat + f] = valid ? u : 0.f;      // per-layer API only: real u, [n][P / 2]
      }
    } else if (KIND == NK_WIRE2D) {
      float o_re, o_im;
      gabor2d_fwd(u, 0.f, p, 0.f, omega, scale, o_re, o_im);
      o_re = valid ? o_re : 0.f; o_im = valid ? o_im : 0.f;
      amx = __builtin_fmaxf(amx, __builtin_fmaxf(__builtin_fabsf(o_re), __builtin_fabsf(o_im)));
      if (live) {
        out[row * P + c_re] = o_re;
        out[row * P + c_re + 32] = o_im;
        if (lin) {                                            // per-layer API only: real (u | p), [n][2 * P / 2]
          lin[row * (2 * nfeat) + f] = valid ? u : 0.f;
          lin[row * (2 * nfeat) + nfeat + f] = valid ? p : 0.f;
        }
      }
    } else {
      float o = real_act_fwd<nk_real_act(KIND)>(u, omega, scale);
      o = valid ? o : 0.f;
      amx = __builtin_fmaxf(amx, __builtin_fabsf(o));
      if (live) {
        if (lin) lin[row * P + f] = valid ? u : 0.f;
        out[row * P + f] = o;
      }
    }
  }
  // max |out_0| for the 2 x fp16 split GEMM that reads it (wire_gemmx2h.hip)
  if (amax_out) wire_amax_publish(amax_out, amx, threadIdx.x & 63);
}

hipError_t launch_first_fwd(hipStream_t s, int kind, const float* coords, int64_t n, int D,
                            const float* W0, const float* b0, const float* V0, const float* c0,
                            int K, int P, float omega, float scale, float* lin, float* out, unsigned* amax_out) {
  if (n <= 0) return hipSuccess;
  if (D > 4) return hipErrorInvalidValue;
  const bool cplx = kind_is_cplx(kind);
  const int nfeat = cplx ? P / 2 : P;
  const int bx = nfeat >= 256 ? 256 : ((nfeat + 63) / 64) * 64;
  dim3 grid(cdiv(n, FIRST_ROWS), cdiv(nfeat, bx));
  return with_kind(kind, [&](auto k) -> hipError_t {
    hipLaunchKernelGGL(first_fwd_kernel<decltype(k)::value>, grid, dim3(bx), 0, s, coords, (long long)n, D, W0, b0,
                       V0, c0, K, P, omega, scale, lin, out, amax_out);
    return hipGetLastError();
  });
}

// ===========================================================================
// positional encoding, modules/relu.py:62-75: [c, {sin(2^i pi c_j), cos(2^i pi c_j)}_{i,j}]
// ===========================================================================
__global__ void posenc_kernel(const float* __restrict__ coords, long long n, int D, int F, int Pin,
                              float* __restrict__ dst) {
  const long long row = (long long)blockIdx.x * (blockDim.x / 64) + (threadIdx.x >> 6);
  if (row >= n) return;
  const int c = threadIdx.x & 63;
  for (int col = c; col < Pin; col += 64) {
    float v = 0.f;
    if (col < D) {
      v = coords[row * D + col];
    } else if (col < D + 2 * D * F) {
      const int e = col - D;
      const int i = e / (2 * D);
      const int j = (e % (2 * D)) >> 1;
      const float freq = (float)((double)(1 << i) * 3.14159265358979323846);
      float sn, cs;
      wire_sincos(freq * coords[row * D + j], sn, cs);
      v = (e & 1) ? cs : sn;
    }
    dst[row * Pin + col] = v;
  }
}
hipError_t launch_posenc(hipStream_t s, const float* coords, int64_t n, int D, int F, int Pin,
                         float* dst) {
  if (n <= 0) return hipSuccess;
  hipLaunchKernelGGL(posenc_kernel, dim3(cdiv(n, 4)), dim3(256), 0, s, coords, (long long)n, D, F,
                     Pin, dst);
  return hipGetLastError();
}

// ===========================================================================
// frozen first stage of the multi-scale B-spline net (modules/bspline_mscale_HL.py, Scaled_Bsplines_form.forward):
// B(lin_j / s_g(j)) per column, pad columns exactly 0 (B(0) = 0.75 would leak into the next GEMM otherwise)
// ===========================================================================
// one lane per 4 consecutive columns of a row: the 16-byte unit wire_store_out4 writes (pre-split or fp32)
__global__ __launch_bounds__(256) void mscale_first_kernel(const float* __restrict__ coords, long long n, int D,
                                                           const float* __restrict__ W0, const float* __restrict__ b0,
                                                           int SHF, MscaleC c, int split, int ld, int qpr,
                                                           float split_scale, unsigned* __restrict__ amax,
                                                           float* __restrict__ dst) {
  const long long q = (long long)blockIdx.x * blockDim.x + threadIdx.x;
  const long long row = q / qpr;
  const int col0 = (int)(q - row * qpr) * 4;
  f32x4 v = {0.f, 0.f, 0.f, 0.f};
  if (row < n) {
    float x[4];
#pragma unroll
    for (int d = 0; d < 4; ++d) x[d] = d < D ? coords[row * D + d] : 0.f;
#pragma unroll
    for (int i = 0; i < 4; ++i) {
      const int j = col0 + i;
      if (j < SHF) {
        float lin = b0[j];
#pragma unroll
        for (int d = 0; d < 4; ++d)
          if (d < D) lin = __builtin_fmaf(x[d], W0[(long long)j * D + d], lin);
        const int g = j < 256 ? 0 : 1 + (j - 256) / split;
        v[i] = bspline2(c.c[g] * lin);
      }
    }
    float* p = dst + row * ld + col0;
    if (split_scale != 0.f || (ld & 3) == 0) {
      wire_store_out4(p, v, split_scale);
    } else {
#pragma unroll
      for (int i = 0; i < 4; ++i)
        if (col0 + i < ld) p[i] = v[i];
    }
  }
  if (amax) {   // every lane of the wave takes part in the reduction (B >= 0: the maximum is max |value|)
    const float m = __builtin_fmaxf(__builtin_fmaxf(v[0], v[1]), __builtin_fmaxf(v[2], v[3]));
    wire_amax_publish(amax, m, threadIdx.x & 63);
  }
}
hipError_t launch_mscale_first(hipStream_t s, const float* coords, int64_t n, int D, const float* W0, const float* b0,
                               int SHF, const MscaleC& c, int split, int ld, float split_scale, unsigned* amax,
                               float* dst) {
  if (n <= 0) return hipSuccess;
  if (D < 1 || D > 4 || SHF < 1 || ld < SHF || (SHF > 256 && split < 1) ||
      (split_scale != 0.f && ((ld & 3) || (reinterpret_cast<uintptr_t>(dst) & 15))))
    return hipErrorInvalidValue;
  const int qpr = (ld + 3) / 4;
  hipLaunchKernelGGL(mscale_first_kernel, dim3(cdiv(n * qpr, 256)), dim3(256), 0, s, coords, (long long)n, D, W0, b0,
                     SHF, c, split, ld, qpr, split_scale, amax, dst);
  return hipGetLastError();
}

// ===========================================================================
// coordinate gradients: one wave per row, features strided over the lanes, a fixed butterfly across them (no atomics:
// the same bits every run)
// ===========================================================================
__global__ __launch_bounds__(256) void coordgrad_rows_kernel(const float* __restrict__ G, int ldg,
                                                             const float* __restrict__ G2, const float* __restrict__ W,
                                                             const float* __restrict__ V, int K, int D, long long n,
                                                             float* __restrict__ g_x) {
  const long long row = (long long)blockIdx.x * 4 + (threadIdx.x >> 6);
  if (row >= n) return;
  const int lane = threadIdx.x & 63;
  float a[4] = {0.f, 0.f, 0.f, 0.f};
  const float* g = G + (size_t)row * ldg;
  const float* g2 = G2 ? G2 + (size_t)row * ldg : nullptr;
  for (int k = lane; k < K; k += 64) {
    const float gv = g[k];
#pragma unroll
    for (int d = 0; d < 4; ++d)
      if (d < D) a[d] = __builtin_fmaf(gv, W[k * D + d], a[d]);
    if (g2) {
      const float pv = g2[k];
#pragma unroll
      for (int d = 0; d < 4; ++d)
        if (d < D) a[d] = __builtin_fmaf(pv, V[k * D + d], a[d]);
    }
  }
#pragma unroll
  for (int d = 0; d < 4; ++d) a[d] = wire_wave_sum(a[d]);
  if (lane < D) {
    float v = a[0];
#pragma unroll
    for (int d = 1; d < 4; ++d) v = lane == d ? a[d] : v;
    g_x[row * D + lane] = v;
  }
}
hipError_t launch_coordgrad_rows(hipStream_t s, const float* G, int ldg, const float* G2, const float* W, const float* V,
                                 int K, int D, int64_t n, float* g_x) {
  if (n <= 0) return hipSuccess;
  hipLaunchKernelGGL(coordgrad_rows_kernel, dim3(cdiv(n, 4)), dim3(256), 0, s, G, ldg, G2, W, V, K, D, (long long)n, g_x);
  return hipGetLastError();
}

__global__ __launch_bounds__(256) void coordgrad_reduce_kernel(const float* __restrict__ partial, int ntiles,
                                                               long long count, float* __restrict__ g_x) {
  const long long e = (long long)blockIdx.x * 256 + threadIdx.x;
  if (e >= count) return;
  float v = partial[e];
  for (int t = 1; t < ntiles; ++t) v += partial[(size_t)t * count + e];
  g_x[e] = v;
}
hipError_t launch_coordgrad_reduce(hipStream_t s, const float* partial, int ntiles, int64_t n, int D, float* g_x) {
  if (n <= 0) return hipSuccess;
  const int64_t count = n * D;
  hipLaunchKernelGGL(coordgrad_reduce_kernel, dim3(cdiv(count, 256)), dim3(256), 0, s, partial, ntiles,
                     (long long)count, g_x);
  return hipGetLastError();
}

// d/dx_j of [x, {sin(2^i pi x_j), cos(2^i pi x_j)}]: 1, 2^i pi cos, -2^i pi sin -- posenc_kernel's feature order and its
// fp32 arguments
__global__ __launch_bounds__(256) void posenc_bwd_kernel(const float* __restrict__ coords, long long n, int D, int F,
                                                         const float* __restrict__ g_pe, int ldpe,
                                                         float* __restrict__ g_x) {
  const long long row = (long long)blockIdx.x * 4 + (threadIdx.x >> 6);
  if (row >= n) return;
  const int lane = threadIdx.x & 63;
  float a[4] = {0.f, 0.f, 0.f, 0.f};
  const float* g = g_pe + (size_t)row * ldpe;
  const int Din = D + 2 * D * F;
  for (int c = lane; c < Din; c += 64) {
    int j;
    float v;
    if (c < D) {
      j = c;
      v = g[c];
    } else {
      const int e = c - D;
      const int i = e / (2 * D);
      j = (e % (2 * D)) >> 1;
      const float freq = (float)((double)(1 << i) * 3.14159265358979323846);
      float sn, cs;
      wire_sincos(freq * coords[row * D + j], sn, cs);
      v = g[c] * ((e & 1) ? -freq * sn : freq * cs);
    }
#pragma unroll
    for (int d = 0; d < 4; ++d) a[d] += d == j ? v : 0.f;
  }
#pragma unroll
  for (int d = 0; d < 4; ++d) a[d] = wire_wave_sum(a[d]);
  if (lane < D) {
    float v = a[0];
#pragma unroll
    for (int d = 1; d < 4; ++d) v = lane == d ? a[d] : v;
    g_x[row * D + lane] = v;
  }
}
hipError_t launch_posenc_bwd(hipStream_t s, const float* coords, int64_t n, int D, int F, const float* g_pe, int ldpe,
                             float* g_x) {
  if (n <= 0) return hipSuccess;
  hipLaunchKernelGGL(posenc_bwd_kernel, dim3(cdiv(n, 4)), dim3(256), 0, s, coords, (long long)n, D, F, g_pe, ldpe, g_x);
  return hipGetLastError();
}
