// wire_mfn.hip -- the bandwidth-bound kernels of the multiplicative filter network (WIRE_KIND_MFN, modules/mfn.py):
// the filter table's pack, the Gabor filter of the coordinates as a point kernel (z_0 and the per-layer call), the final
// linear's backward fused with the last multiplicative stage, and the deterministic column sums that give a filter's
// parameter gradients.  The multiplicative epilogues of the GEMMs: wire_gemm_epi.h / wire_gemmh_epi.h (EPI_MFN_*).
#include "wire_dev.h"
#include "wire_point.h"

// a filter's parameters: its table in the packed image (whole-net calls), or the native tensors (per-layer calls)
struct MfnSrc { const float* tab; const float* mu; const float* gamma; const float* w; const float* c; int D; int K; };
WIRE_DEVINL MfnCol mfn_src_load(const MfnSrc& s, int col) {
  if (s.tab) return mfn_load(s.tab, col);
  MfnCol p{};
  if (col < s.K) {
#pragma unroll
    for (int d = 0; d < 4; ++d)
      if (d < s.D) { p.mu[d] = s.mu[col * s.D + d]; p.w[d] = s.w[col * s.D + d]; }
    p.gamma = s.gamma[col]; p.c = s.c[col];
  }
  return p;
}

// ---------------------------------------------------------------------------
// pack: native mu [K][D], gamma [K], w [K][D], c [K] -> tab [P][MFN_TAB]
// ---------------------------------------------------------------------------
__global__ void mfn_pack_table_kernel(const float* __restrict__ mu, const float* __restrict__ gamma,
                                      const float* __restrict__ w, const float* __restrict__ c, int K, int D, int P,
                                      float* __restrict__ tab) {
  const int col = blockIdx.x * blockDim.x + threadIdx.x;
  if (col >= P) return;
  float v[MFN_TAB];
#pragma unroll
  for (int i = 0; i < MFN_TAB; ++i) v[i] = 0.f;
  if (col < K) {
    for (int d = 0; d < D; ++d) { v[d] = mu[col * D + d]; v[4 + d] = w[col * D + d]; }
    v[8] = gamma[col]; v[9] = c[col];
  }
#pragma unroll
  for (int i = 0; i < MFN_TAB; ++i) tab[(size_t)col * MFN_TAB + i] = v[i];
}
hipError_t launch_mfn_pack_table(hipStream_t s, const float* mu, const float* gamma, const float* w, const float* c, int K,
                                 int D, int P, float* tab) {
  if (D < 1 || D > 4) return hipErrorInvalidValue;
  hipLaunchKernelGGL(mfn_pack_table_kernel, dim3(cdiv(P, 128)), dim3(128), 0, s, mu, gamma, w, c, K, D, P, tab);
  return hipGetLastError();
}

// ---------------------------------------------------------------------------
// the filter as a point kernel: out[r][j] = g_j(x_r), j < C (C = the row's stored columns: P with zero pads, or K);
// mul (optional, [n][ldo]): out = mul g -- the multiplicative stage behind a plain linear epilogue.  One thread per
// column, 64 rows per block, the column's parameters in registers.
// ---------------------------------------------------------------------------
#define MFN_ROWS 64
__global__ void mfn_filter_fwd_kernel(MfnSrc src, const float* __restrict__ coords, long long n, int C,
                                      const float* __restrict__ mul, float* __restrict__ out, int ldo,
                                      unsigned* __restrict__ amax_out) {
  const int col = blockIdx.y * blockDim.x + threadIdx.x;
  const bool live = col < C;                    // (no early return: the maximum below is a whole-wave reduction)
  MfnCol fc{};
  if (live) fc = mfn_src_load(src, col);
  const long long r0 = (long long)blockIdx.x * MFN_ROWS;
  long long r1 = r0 + MFN_ROWS;
  if (r1 > n) r1 = n;
  float amx = 0.f;
  for (long long row = r0; row < r1; ++row) {
    float x[4];
    mfn_load_x(coords, row, src.D, x);
    float o = (live && col < src.K) ? mfn_g(fc, x) : 0.f;
    if (live) {
      if (mul) o *= mul[row * ldo + col];
      out[row * ldo + col] = o;
    }
    amx = __builtin_fmaxf(amx, __builtin_fabsf(o));
  }
  if (amax_out) wire_amax_publish(amax_out, amx, threadIdx.x & 63);
}
static hipError_t filter_fwd(hipStream_t s, const MfnSrc& src, const float* coords, int64_t n, int C, const float* mul,
                             float* out, int ldo, unsigned* amax_out) {
  if (n <= 0) return hipSuccess;
  if (src.D < 1 || src.D > 4) return hipErrorInvalidValue;
  const int bx = C >= 256 ? 256 : ((C + 63) / 64) * 64;
  hipLaunchKernelGGL(mfn_filter_fwd_kernel, dim3(cdiv(n, MFN_ROWS), cdiv(C, bx)), dim3(bx), 0, s, src, coords,
                     (long long)n, C, mul, out, ldo, amax_out);
  return hipGetLastError();
}
hipError_t launch_mfn_filter_fwd(hipStream_t s, const float* tab, const float* coords, int64_t n, int D, int K, int P,
                                 const float* mul, float* out, unsigned* amax_out) {
  return filter_fwd(s, MfnSrc{tab, nullptr, nullptr, nullptr, nullptr, D, K}, coords, n, P, mul, out, P, amax_out);
}
hipError_t launch_mfn_filter_fwd_native(hipStream_t s, const float* mu, const float* gamma, const float* w, const float* c,
                                        const float* coords, int64_t n, int D, int K, float* out) {
  return filter_fwd(s, MfnSrc{nullptr, mu, gamma, w, c, D, K}, coords, n, K, nullptr, out, K, nullptr);
}

// ---------------------------------------------------------------------------
// final linear backward fused with the last multiplicative stage: g_z = g_y wf (wf [O][P]); partials of g_y^T z and of
// the column sums of g_y in launch_final_bwd's layout (WIRE_FB_ROWS rows per block, launch_final_reduce adds them up); then
//   lin != null: g_lin = g_z g(x) (the layer below's; its maximum into amax_g) and h = g_z lin (the filter's upstream)
//   lin == null (no hidden layer): h = g_z
// ---------------------------------------------------------------------------
__global__ __launch_bounds__(256) void mfn_final_bwd_kernel(const float* __restrict__ g_y, long long n, int O,
                                                            const float* __restrict__ wf, const float* __restrict__ z,
                                                            const float* __restrict__ lin, const float* __restrict__ tab,
                                                            const float* __restrict__ coords, int D, int P,
                                                            float* __restrict__ g_lin, float* __restrict__ hbuf,
                                                            float* __restrict__ part_w, float* __restrict__ part_b,
                                                            unsigned* __restrict__ amax_g) {
  __shared__ float sgy[WIRE_FB_ROWS * WIRE_MAXO];
  __shared__ float sx[WIRE_FB_ROWS * 4];
  const long long r0 = (long long)blockIdx.x * WIRE_FB_ROWS;
  long long r1 = r0 + WIRE_FB_ROWS;
  if (r1 > n) r1 = n;
  const int nr = (int)(r1 - r0);
  for (int i = threadIdx.x; i < nr * O; i += blockDim.x) sgy[i] = g_y[r0 * O + i];
  for (int i = threadIdx.x; i < nr * 4; i += blockDim.x) {
    const int r = i >> 2, d = i & 3;
    sx[i] = d < D ? coords[(r0 + r) * D + d] : 0.f;
  }
  __syncthreads();
  const int col = blockIdx.y * blockDim.x + threadIdx.x;
  float amx = 0.f;
  if (col < P) {
    float w[WIRE_MAXO], a[WIRE_MAXO];
#pragma unroll
    for (int o = 0; o < WIRE_MAXO; ++o) { a[o] = 0.f; w[o] = o < O ? wf[(size_t)o * P + col] : 0.f; }
    MfnCol fc{};
    if (lin) fc = mfn_load(tab, col);
    for (int r = 0; r < nr; ++r) {
      const long long row = r0 + r;
      const float zv = part_w ? z[row * P + col] : 0.f;
      float gz = 0.f;
#pragma unroll
      for (int o = 0; o < WIRE_MAXO; ++o)
        if (o < O) {
          const float g = sgy[r * O + o];
          gz = __builtin_fmaf(g, w[o], gz);
          a[o] = __builtin_fmaf(g, zv, a[o]);
        }
      if (lin) {
        const float x[4] = {sx[4 * r], sx[4 * r + 1], sx[4 * r + 2], sx[4 * r + 3]};
        const float gl = gz * mfn_g(fc, x);
        g_lin[row * P + col] = gl;
        hbuf[row * P + col] = gz * lin[row * P + col];
        amx = __builtin_fmaxf(amx, __builtin_fabsf(gl));
      } else {
        hbuf[row * P + col] = gz;
      }
    }
    if (part_w) {
      float* pw = part_w + (size_t)blockIdx.x * O * P;
#pragma unroll
      for (int o = 0; o < WIRE_MAXO; ++o)
        if (o < O) pw[(size_t)o * P + col] = a[o];
    }
  }
  if (part_b && blockIdx.y == 0 && threadIdx.x < O) {
    float sacc = 0.f;
    for (int r = 0; r < nr; ++r) sacc += sgy[r * O + threadIdx.x];
    part_b[(size_t)blockIdx.x * O + threadIdx.x] = sacc;
  }
  if (amax_g) wire_amax_publish(amax_g, amx, threadIdx.x & 63);
}
hipError_t launch_mfn_final_bwd(hipStream_t s, const float* g_y, int64_t n, int O, const float* wf, const float* z,
                                const float* lin, const float* tab, const float* coords, int D, int P, float* g_lin,
                                float* hbuf, float* part_w, float* part_b, unsigned* amax_g) {
  if (n <= 0) return hipSuccess;
  if (O > WIRE_MAXO || D < 1 || D > 4) return hipErrorInvalidValue;
  hipLaunchKernelGGL(mfn_final_bwd_kernel, dim3(cdiv(n, WIRE_FB_ROWS), cdiv(P, 256)), dim3(256), 0, s, g_y, (long long)n, O,
                     wf, z, lin, tab, coords, D, P, g_lin, hbuf, part_w, part_b, amax_g);
  return hipGetLastError();
}

// ---------------------------------------------------------------------------
// a filter's parameter gradients from its upstream gradient h [n][ldh] (modules/mfn.py:24-26 differentiated):
//   f = e sin a, e = exp(-gamma nrm / 2), a = x . w + c
//   g_gamma_j = sum_r h (-nrm / 2) f        g_mu_jd = sum_r h gamma (x_d - mu_jd) f
//   g_c_j     = sum_r h e cos a             g_w_jd  = sum_r h e cos a x_d
// One wave per (MFS_ROWS rows, 64 columns): per-block partials part[block][10][C] (q = 0 gamma, 1 c, 2 + d mu_d,
// 6 + d w_d), added up over the blocks in their order by mfn_sums_reduce_kernel -- no atomics, the same bits every run.
// ---------------------------------------------------------------------------
#define MFS_ROWS 512
#define MFS_Q 10
int mfn_sums_blocks(int64_t n) { return (int)((n + MFS_ROWS - 1) / MFS_ROWS); }
__global__ __launch_bounds__(64) void mfn_sums_kernel(MfnSrc src, const float* __restrict__ coords, long long n,
                                                      const float* __restrict__ hbuf, int ldh, float* __restrict__ part) {
  const int C = src.K;
  const int col = blockIdx.y * 64 + threadIdx.x;
  if (col >= C) return;
  const MfnCol fc = mfn_src_load(src, col);
  const long long r0 = (long long)blockIdx.x * MFS_ROWS;
  long long r1 = r0 + MFS_ROWS;
  if (r1 > n) r1 = n;
  float sg = 0.f, sc = 0.f, smu[4] = {0.f, 0.f, 0.f, 0.f}, sw[4] = {0.f, 0.f, 0.f, 0.f};
  for (long long row = r0; row < r1; ++row) {
    float x[4];
    mfn_load_x(coords, row, src.D, x);
    const float hv = hbuf[row * ldh + col];
    float nrm, e, sn, cs;
    mfn_eval(fc, x, nrm, e, sn, cs);
    const float hf = hv * (e * sn), hc = hv * (e * cs);
    sg = __builtin_fmaf(hf, -0.5f * nrm, sg);
    sc += hc;
    const float hfg = hf * fc.gamma;
#pragma unroll
    for (int d = 0; d < 4; ++d) {
      smu[d] = __builtin_fmaf(hfg, x[d] - fc.mu[d], smu[d]);
      sw[d] = __builtin_fmaf(hc, x[d], sw[d]);
    }
  }
  float* p = part + (size_t)blockIdx.x * MFS_Q * C + col;
  p[0] = sg; p[(size_t)C] = sc;
#pragma unroll
  for (int d = 0; d < 4; ++d) { p[(size_t)(2 + d) * C] = smu[d]; p[(size_t)(6 + d) * C] = sw[d]; }
}
__global__ void mfn_sums_reduce_kernel(const float* __restrict__ part, int nblk, int C, int D, float* __restrict__ g_mu,
                                       float* __restrict__ g_gamma, float* __restrict__ g_w, float* __restrict__ g_c) {
  const int col = blockIdx.x * blockDim.x + threadIdx.x, q = blockIdx.y;
  if (col >= C) return;
  const int d = q >= 6 ? q - 6 : q - 2;
  if (q >= 2 && d >= D) return;
  float acc = 0.f;
  for (int b = 0; b < nblk; ++b) acc += part[((size_t)b * MFS_Q + q) * C + col];
  if (q == 0) g_gamma[col] = acc;
  else if (q == 1) g_c[col] = acc;
  else if (q < 6) g_mu[col * D + d] = acc;
  else g_w[col * D + d] = acc;
}
static hipError_t filter_sums(hipStream_t s, const MfnSrc& src, const float* coords, int64_t n, const float* hbuf, int ldh,
                              float* part, float* g_mu, float* g_gamma, float* g_w, float* g_c) {
  if (n <= 0 || src.D < 1 || src.D > 4) return hipErrorInvalidValue;
  const int nblk = mfn_sums_blocks(n);
  hipLaunchKernelGGL(mfn_sums_kernel, dim3((unsigned)nblk, cdiv(src.K, 64)), dim3(64), 0, s, src, coords, (long long)n,
                     hbuf, ldh, part);
  hipLaunchKernelGGL(mfn_sums_reduce_kernel, dim3(cdiv(src.K, 64), MFS_Q), dim3(64), 0, s, part, nblk, src.K, src.D, g_mu,
                     g_gamma, g_w, g_c);
  return hipGetLastError();
}
hipError_t launch_mfn_filter_sums(hipStream_t s, const float* tab, const float* coords, int64_t n, int D, int K,
                                  const float* hbuf, int ldh, float* part, float* g_mu, float* g_gamma, float* g_w,
                                  float* g_c) {
  return filter_sums(s, MfnSrc{tab, nullptr, nullptr, nullptr, nullptr, D, K}, coords, n, hbuf, ldh, part, g_mu, g_gamma,
                     g_w, g_c);
}
hipError_t launch_mfn_filter_sums_native(hipStream_t s, const float* mu, const float* gamma, const float* w, const float* c,
                                         const float* coords, int64_t n, int D, int K, const float* hbuf, float* part,
                                         float* g_mu, float* g_gamma, float* g_w, float* g_c) {
  return filter_sums(s, MfnSrc{nullptr, mu, gamma, w, c, D, K}, coords, n, hbuf, K, part, g_mu, g_gamma, g_w, g_c);
}

// ---------------------------------------------------------------------------
// a filter's share of the coordinate gradient: g_x[r][d] (+)= sum_j h ( -gamma (x_d - mu_jd) f + e cos a w_jd ).
// One wave per row, the lanes over the columns in a fixed order, one butterfly: deterministic.  acc != 0 adds to what
// g_x holds (the filters of a net are processed one after the other on the stream).
// ---------------------------------------------------------------------------
__global__ __launch_bounds__(256) void mfn_gx_kernel(MfnSrc src, const float* __restrict__ coords, long long n,
                                                     const float* __restrict__ hbuf, int ldh, int acc,
                                                     float* __restrict__ g_x) {
  const int lane = threadIdx.x & 63;
  const long long row = (long long)blockIdx.x * 4 + (threadIdx.x >> 6);
  if (row >= n) return;
  float x[4];
  mfn_load_x(coords, row, src.D, x);
  float t[4] = {0.f, 0.f, 0.f, 0.f};
  for (int col = lane; col < src.K; col += 64) {
    const MfnCol fc = mfn_src_load(src, col);
    const float hv = hbuf[row * ldh + col];
    float nrm, e, sn, cs;
    mfn_eval(fc, x, nrm, e, sn, cs);
    const float hf = hv * (e * sn) * fc.gamma, hc = hv * (e * cs);
#pragma unroll
    for (int d = 0; d < 4; ++d) t[d] += __builtin_fmaf(hc, fc.w[d], -(hf * (x[d] - fc.mu[d])));
  }
#pragma unroll
  for (int d = 0; d < 4; ++d) {
    float v = t[d];
#pragma unroll
    for (int o = 32; o; o >>= 1) v += __shfl_xor(v, o);
    if (lane == 0 && d < src.D) g_x[row * src.D + d] = (acc ? g_x[row * src.D + d] : 0.f) + v;
  }
}
hipError_t launch_mfn_filter_gx(hipStream_t s, const float* tab, const float* coords, int64_t n, int D, int K,
                                const float* hbuf, int ldh, int acc, float* g_x) {
  if (n <= 0) return hipSuccess;
  hipLaunchKernelGGL(mfn_gx_kernel, dim3(cdiv(n, 4)), dim3(256), 0, s, MfnSrc{tab, nullptr, nullptr, nullptr, nullptr, D, K},
                     coords, (long long)n, hbuf, ldh, acc, g_x);
  return hipGetLastError();
}
hipError_t launch_mfn_filter_gx_native(hipStream_t s, const float* mu, const float* gamma, const float* w, const float* c,
                                       const float* coords, int64_t n, int D, int K, const float* hbuf, float* g_x) {
  if (n <= 0) return hipSuccess;
  hipLaunchKernelGGL(mfn_gx_kernel, dim3(cdiv(n, 4)), dim3(256), 0, s, MfnSrc{nullptr, mu, gamma, w, c, D, K}, coords,
                     (long long)n, hbuf, K, 0, g_x);
  return hipGetLastError();
}
