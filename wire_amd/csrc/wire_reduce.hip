// wire_reduce.hip -- the deterministic two-stage reductions: per-block partials of the final linear's and the first
// layer's weight gradients (with the pre-reduction both share), and the weight-gradient slabs of the GEMMs (real-expanded
// and 3M).  Fixed summation order, no atomics: the same bits every run.
#include "wire_dev.h"
#include "wire_point.h"

// pre-reduction of per-row-block partials: in[nblk][C] -> out[nchunk][C], chunk c sums blocks
// [c*per, (c+1)*per), at most PRE_CHUNKS of them (wire_point.h: prereduce_room sizes the buffers for it).  Keeps the
// final reductions short (they were latency-bound over 1024 blocks).
__global__ __launch_bounds__(256) void prereduce_kernel(const float* __restrict__ in, int nblk, int C, int per,
                                                        float* __restrict__ out) {
  const int c = blockIdx.x * 256 + threadIdx.x;
  const int ch = blockIdx.y;
  if (c >= C) return;
  const int b0 = ch * per;
  int b1 = b0 + per;
  if (b1 > nblk) b1 = nblk;
  float a0 = 0.f, a1 = 0.f, a2 = 0.f, a3 = 0.f;
  int b = b0;
  for (; b + 3 < b1; b += 4) {
    a0 += in[(size_t)b * C + c];
    a1 += in[(size_t)(b + 1) * C + c];
    a2 += in[(size_t)(b + 2) * C + c];
    a3 += in[(size_t)(b + 3) * C + c];
  }
  for (; b < b1; ++b) a0 += in[(size_t)b * C + c];
  out[(size_t)ch * C + c] = (a0 + a1) + (a2 + a3);
}
// returns the number of blocks left (nblk itself when no pre-reduction was worth it)
static int prereduce(hipStream_t s, const float* in, int nblk, int C, float* out) {
  if (nblk <= 2 * PRE_CHUNKS) return nblk;
  const int per = (nblk + PRE_CHUNKS - 1) / PRE_CHUNKS;
  const int nch = (nblk + per - 1) / per;
  hipLaunchKernelGGL(prereduce_kernel, dim3(cdiv(C, 256), (unsigned)nch), dim3(256), 0, s, in, nblk, C, per, out);
  return nch;
}

// g_Wf = g_y^T conj(z):  re = sum g z_re, im = -sum g z_im;  g_bf = sum g + 0j
// block = 64 columns x 4 partial groups (each group strides over the row blocks), LDS combine
__global__ __launch_bounds__(256) void final_reduce_kernel(int kind, const float* __restrict__ part_w,
                                    const float* __restrict__ part_b, int nblk, int O, int K, int P,
                                    float* __restrict__ gWf, float* __restrict__ gbf) {
  __shared__ float red[2][4][64];
  const int tx = threadIdx.x & 63, ty = threadIdx.x >> 6;
  const int i = blockIdx.x * 64 + tx;
  const int o = blockIdx.y;
  const bool cplx = (kind == NK_WIRE || kind == NK_WIRE2D);
  float sr = 0.f, si = 0.f;
  if (i < K) {
    const int c = cplx ? blk_col(i, 0) : i;
    for (int b = ty; b < nblk; b += 4) {
      const float* pw = part_w + ((size_t)b * O + o) * P;
      sr += pw[c];
      if (cplx) si += pw[c + 32];
    }
  }
  red[0][ty][tx] = sr;
  red[1][ty][tx] = si;
  __syncthreads();
  if (ty == 0 && i < K) {
    sr = (red[0][0][tx] + red[0][1][tx]) + (red[0][2][tx] + red[0][3][tx]);
    si = (red[1][0][tx] + red[1][1][tx]) + (red[1][2][tx] + red[1][3][tx]);
    if (cplx) {
      gWf[((size_t)o * K + i) * 2] = sr;
      gWf[((size_t)o * K + i) * 2 + 1] = -si;
    } else {
      gWf[(size_t)o * K + i] = sr;
    }
  }
  if (blockIdx.x == 0 && threadIdx.x == 0) {
    float sb = 0.f;
    for (int b = 0; b < nblk; ++b) sb += part_b[(size_t)b * O + o];
    if (cplx) { gbf[2 * o] = sb; gbf[2 * o + 1] = 0.f; } else gbf[o] = sb;
  }
}

hipError_t launch_final_reduce(hipStream_t s, int kind, float* part_w, float* part_b,
                               int nblk, int O, int K, int P, float* gWf, float* gbf) {
  // the partial buffers have room for prereduce_room(nblk) blocks: the pre-reduced chunks go behind the nblk blocks
  float* w2 = part_w + (size_t)nblk * O * P;
  float* b2 = part_b + (size_t)nblk * O;
  const int nw = prereduce(s, part_w, nblk, O * P, w2);
  const int nb = prereduce(s, part_b, nblk, O, b2);
  dim3 grid(cdiv(K, 64), (unsigned)O);
  hipLaunchKernelGGL(final_reduce_kernel, grid, dim3(256), 0, s, kind, nw == nblk ? part_w : w2,
                     nb == nblk ? part_b : b2, nw == nblk ? nblk : nw, O, K, P, gWf, gbf);
  return hipGetLastError();
}

// ===========================================================================
// hidden weight-gradient reduction.  M = G^T Z in blocked-planar real form;
//   g_W = g_lin^T conj(z):  re = M[(o,re),(i,re)] + M[(o,im),(i,im)]
//                           im = M[(o,im),(i,re)] - M[(o,re),(i,im)]
// ===========================================================================
// block = 64 input features x 4 groups of row splits (group q sums splits q, q + 4, ... with four loads in
// flight); the four partial sums are combined through LDS in a fixed order (deterministic, no atomics).
// WS (real kinds): g_W is multiplied by ws on the way out, g_b is not (launch_wgrad_reduce: wscale)
template <bool WS>
__global__ __launch_bounds__(256) void wgrad_reduce_kernel(int kind, const float* __restrict__ slab,
                                    const float* __restrict__ bslab, int S, int K, int Kin, int Pm,
                                    int Pn, float* __restrict__ gW, float* __restrict__ gb,
                                    float* __restrict__ gV, float* __restrict__ gc, float ws) {
  __shared__ float red[4][4][64];       // [value][group][feature]
  const int tx = threadIdx.x & 63, q = threadIdx.x >> 6;
  const int i = blockIdx.x * 64 + tx;
  const int o = blockIdx.y;
  const size_t sstride = (size_t)Pm * Pn;
  const bool cplx = (kind == NK_WIRE || kind == NK_WIRE2D);
  const int nmat = (kind == NK_WIRE2D) ? 2 : 1;
  for (int mat = 0; mat < nmat; ++mat) {
    int r_re, r_im = 0;
    if (kind == NK_WIRE) { r_re = blk_col(o, 0); r_im = r_re + 32; }
    else if (kind == NK_WIRE2D) { r_re = ((o >> 5) << 7) + 64 * mat + (o & 31); r_im = r_re + 32; }
    else r_re = o;
    float sr = 0.f, si = 0.f, br = 0.f, bi = 0.f;
    if (i < Kin) {
      if (cplx) {
        const int c_re = blk_col(i, 0), c_im = c_re + 32;
        const size_t a = (size_t)r_re * Pn + c_re, b = (size_t)r_im * Pn + c_im, c = (size_t)r_im * Pn + c_re,
                     d = (size_t)r_re * Pn + c_im;
#pragma unroll 4
        for (int sp = q; sp < S; sp += 4) {
          const float* m = slab + sp * sstride;
          sr += m[a] + m[b];
          si += m[c] - m[d];
        }
      } else {
        const size_t a = (size_t)o * Pn + i;
#pragma unroll 4
        for (int sp = q; sp < S; sp += 4) sr += slab[sp * sstride + a];
      }
    }
    if (tx == 0 && blockIdx.x == 0)
      for (int sp = q; sp < S; sp += 4) {
        br += bslab[(size_t)sp * Pm + r_re];
        if (cplx) bi += bslab[(size_t)sp * Pm + r_im];
      }
    red[0][q][tx] = sr; red[1][q][tx] = si; red[2][q][tx] = br; red[3][q][tx] = bi;
    __syncthreads();
    if (q == 0) {
      float* gWm = mat == 0 ? gW : gV;
      float* gbm = mat == 0 ? gb : gc;
      const float wr = (red[0][0][tx] + red[0][1][tx]) + (red[0][2][tx] + red[0][3][tx]);
      const float wi = (red[1][0][tx] + red[1][1][tx]) + (red[1][2][tx] + red[1][3][tx]);
      if (i < Kin) {
        if (cplx) {
          gWm[((size_t)o * Kin + i) * 2] = wr;
          gWm[((size_t)o * Kin + i) * 2 + 1] = wi;
        } else {
          gWm[(size_t)o * Kin + i] = WS ? ws * wr : wr;
        }
      }
      if (tx == 0 && blockIdx.x == 0) {
        const float b0 = (red[2][0][0] + red[2][1][0]) + (red[2][2][0] + red[2][3][0]);
        const float b1 = (red[3][0][0] + red[3][1][0]) + (red[3][2][0] + red[3][3][0]);
        if (cplx) { gbm[2 * o] = b0; gbm[2 * o + 1] = b1; }
        else gbm[o] = b0;
      }
    }
    __syncthreads();
  }
}

hipError_t launch_wgrad_reduce(hipStream_t s, int kind, const float* slab, const float* bslab,
                               int S, int K, int Kin, int Pm, int Pn, float* gW, float* gb,
                               float* gV, float* gc, float wscale) {
  dim3 grid(cdiv(Kin, 64), (unsigned)K);
  if (wscale != 1.f)
    hipLaunchKernelGGL(wgrad_reduce_kernel<true>, grid, dim3(256), 0, s, kind, slab, bslab, S, K, Kin, Pm,
                       Pn, gW, gb, gV, gc, wscale);
  else
    hipLaunchKernelGGL(wgrad_reduce_kernel<false>, grid, dim3(256), 0, s, kind, slab, bslab, S, K, Kin, Pm,
                       Pn, gW, gb, gV, gc, 1.f);
  return hipGetLastError();
}

// ===========================================================================
// first-layer weight gradient: tall-skinny  G[n][C]^T [x | 1]
//   stage 1: block = 64 column quads (float4) x 4 row lanes over CR_ROWS rows -> partial[blk][C][5]
//   stage 2: block = 64 columns x 4 groups over the row blocks
// ===========================================================================
#define CR_ROWS 256
int colreduce_blocks(int64_t n) { return (int)((n + CR_ROWS - 1) / CR_ROWS); }

__global__ __launch_bounds__(256) void colreduce_kernel(const float* __restrict__ G, int ldg, int C,
                                                        const float* __restrict__ x, int D,
                                                        long long n, float* __restrict__ partial) {
  __shared__ float red[4][64][20];
  const int tx = threadIdx.x & 63, ty = threadIdx.x >> 6;
  const int c0 = (blockIdx.y * 64 + tx) * 4;
  const long long r0 = (long long)blockIdx.x * CR_ROWS;
  long long r1 = r0 + CR_ROWS;
  if (r1 > n) r1 = n;
  float acc[4][5];
#pragma unroll
  for (int q = 0; q < 4; ++q)
#pragma unroll
    for (int d = 0; d < 5; ++d) acc[q][d] = 0.f;
  if (c0 < ldg) {
    for (long long row = r0 + ty; row < r1; row += 4) {
      const f32x4 g = *reinterpret_cast<const f32x4*>(G + row * ldg + c0);
      float xv[4] = {0.f, 0.f, 0.f, 0.f};
      for (int d = 0; d < D; ++d) xv[d] = x[row * D + d];
#pragma unroll
      for (int q = 0; q < 4; ++q) {
#pragma unroll
        for (int d = 0; d < 4; ++d) acc[q][d] = __builtin_fmaf(g[q], xv[d], acc[q][d]);
        acc[q][4] += g[q];
      }
    }
  }
#pragma unroll
  for (int q = 0; q < 4; ++q)
#pragma unroll
    for (int d = 0; d < 5; ++d) red[ty][tx][q * 5 + d] = acc[q][d];
  __syncthreads();
  if (ty == 0) {
#pragma unroll
    for (int q = 0; q < 4; ++q) {
      const int c = c0 + q;
      if (c < C) {
        float* p = partial + ((size_t)blockIdx.x * C + c) * 5;
#pragma unroll
        for (int d = 0; d < 5; ++d)
          p[d] = (red[0][tx][q * 5 + d] + red[1][tx][q * 5 + d]) + (red[2][tx][q * 5 + d] + red[3][tx][q * 5 + d]);
      }
    }
  }
}

template <bool WS>
__global__ __launch_bounds__(256) void colreduce_final_kernel(const float* __restrict__ partial, int nblk,
                                                              int C, int D, float* __restrict__ gW0,
                                                              float* __restrict__ gb0, float ws) {
  __shared__ float red[4][64][5];
  const int tx = threadIdx.x & 63, ty = threadIdx.x >> 6;
  const int c = blockIdx.x * 64 + tx;
  float acc[5] = {0.f, 0.f, 0.f, 0.f, 0.f};
  if (c < C) {
    for (int b = ty; b < nblk; b += 4) {
      const float* p = partial + ((size_t)b * C + c) * 5;
#pragma unroll
      for (int d = 0; d < 5; ++d) acc[d] += p[d];
    }
  }
#pragma unroll
  for (int d = 0; d < 5; ++d) red[ty][tx][d] = acc[d];
  __syncthreads();
  if (ty == 0 && c < C) {
#pragma unroll
    for (int d = 0; d < 5; ++d) acc[d] = (red[0][tx][d] + red[1][tx][d]) + (red[2][tx][d] + red[3][tx][d]);
    for (int d = 0; d < D; ++d) gW0[c * D + d] = WS ? ws * acc[d] : acc[d];
    gb0[c] = acc[4];
  }
}

// stage 2 alone: partial[colreduce_blocks(n)][C][5] already holds the per-256-row sums (written by the data-gradient
// epilogue of wire_gemmx3h.hip, GemmEpiParams::cr_partial)
hipError_t launch_colreduce_final(hipStream_t s, int C, int D, int64_t n, float* partial, float* gW0, float* gb0,
                                  float wscale) {
  return launch_colreduce_final_blocks(s, C, D, colreduce_blocks(n), partial, gW0, gb0, wscale);
}
// the same over nblk blocks of any row count (the data-gradient chain of wire_fused.hip writes one per workgroup); partial
// must have room for prereduce_room(nblk) * C * 5 floats
hipError_t launch_colreduce_final_blocks(hipStream_t s, int C, int D, int nblk, float* partial, float* gW0, float* gb0,
                                         float wscale) {
  if (D > 4 || nblk < 1) return hipErrorInvalidValue;
  float* p2 = partial + (size_t)nblk * C * 5;            // the slack prereduce_room reserves
  const int nb = prereduce(s, partial, nblk, C * 5, p2);
  if (wscale != 1.f)
    hipLaunchKernelGGL(colreduce_final_kernel<true>, dim3(cdiv(C, 64)), dim3(256), 0, s, nb == nblk ? partial : p2, nb,
                       C, D, gW0, gb0, wscale);
  else
    hipLaunchKernelGGL(colreduce_final_kernel<false>, dim3(cdiv(C, 64)), dim3(256), 0, s, nb == nblk ? partial : p2, nb,
                       C, D, gW0, gb0, 1.f);
  return hipGetLastError();
}
hipError_t launch_colreduce(hipStream_t s, const float* G, int ldg, int C, const float* x, int D,
                            int64_t n, float* partial, float* gW0, float* gb0, float wscale) {
  if (D > 4 || (ldg & 3)) return hipErrorInvalidValue;
  const int nblk = colreduce_blocks(n);
  dim3 grid((unsigned)nblk, cdiv(C, 256));
  hipLaunchKernelGGL(colreduce_kernel, grid, dim3(256), 0, s, G, ldg, C, x, D, (long long)n, partial);
  return launch_colreduce_final(s, C, D, n, partial, gW0, gb0, wscale);
}

// ===========================================================================
// 3M complex path (wire_gemm3m.hip): slab reduction
// ===========================================================================
// g_W.re = P1 + P2, g_W.im = P3 - P1 + P2 summed over the row splits; g_b from the column sums
__global__ __launch_bounds__(256) void wgrad3m_reduce_kernel(const float* __restrict__ slab,
                                      const float* __restrict__ bslab, int S, int K, int Kin, int Kp_o,
                                      int Kp_i, float* __restrict__ gW, float* __restrict__ gb) {
  // block = 64 input features x 4 groups of row splits; partial sums combined through LDS
  __shared__ float red[2][4][64];
  const int tx = threadIdx.x & 63, ty = threadIdx.x >> 6;
  const int i = blockIdx.x * 64 + tx;
  const int o = blockIdx.y;
  const size_t plane = (size_t)Kp_o * Kp_i;
  float sr = 0.f, si = 0.f;
  if (i < Kin) {
    for (int s = ty; s < S; s += 4) {
      const float* p = slab + (size_t)s * 3 * plane + (size_t)o * Kp_i + i;
      const float p1 = p[0], p2 = p[plane], p3 = p[2 * plane];
      sr += p1 + p2;
      si += (p3 - p1) + p2;
    }
  }
  red[0][ty][tx] = sr;
  red[1][ty][tx] = si;
  __syncthreads();
  if (ty == 0 && i < Kin) {
    gW[((size_t)o * Kin + i) * 2] = (red[0][0][tx] + red[0][1][tx]) + (red[0][2][tx] + red[0][3][tx]);
    gW[((size_t)o * Kin + i) * 2 + 1] = (red[1][0][tx] + red[1][1][tx]) + (red[1][2][tx] + red[1][3][tx]);
  }
  if (blockIdx.x == 0 && threadIdx.x == 0) {
    float br = 0.f, bi = 0.f;
    for (int s = 0; s < S; ++s) {
      br += bslab[((size_t)s * 2 + 0) * Kp_o + o];
      bi += bslab[((size_t)s * 2 + 1) * Kp_o + o];
    }
    gb[2 * o] = br;
    gb[2 * o + 1] = bi;
  }
}
hipError_t launch_wgrad3m_reduce(hipStream_t s, const float* slab, const float* bslab, int S, int K, int Kin,
                                 int Kp_o, int Kp_i, float* gW, float* gb) {
  dim3 grid(cdiv(Kin, 64), (unsigned)K);
  hipLaunchKernelGGL(wgrad3m_reduce_kernel, grid, dim3(256), 0, s, slab, bslab, S, K, Kin, Kp_o, Kp_i, gW, gb);
  return hipGetLastError();
}
