// wire_gemmh_epi.h -- fused epilogues of the 16 x 16 x 32 NT GEMMs (wire_gemmx3h.hip: 3 x bf16 split, wire_gemmx2h.hip:
// 2 x fp16 split).  Same arithmetic as wire_gemm_epi.h (lean forms of wire_dev.h); what differs is the accumulator
// layout these kernels leave behind and the 16-byte-vector, whole-cache-line global accesses built on it.
// Reference arithmetic: modules/wire.py:88-93, wire2d.py:56-67, siren.py:48-49, gauss.py:27-28, relu.py:28-29 and the
// autograd backward of each.
#pragma once
#include <type_traits>

#include "wire_dev.h"
#include "wire_gemm.h"

// ---------------------------------------------------------------------------
// epilogues.  The MFMAs are issued with the operands SWAPPED (weights as the "A" operand, activations as "B"), so a
// 16 x 16 block leaves the accumulator transposed: lane -> activation ROW lane & 15, registers q = 0..3 -> four
// CONSECUTIVE output columns 4 (lane >> 4) + q.  Stored like that a wave instruction would write 16 rows x 64 bytes
// -- half cache lines.  Two column-adjacent blocks X (columns 0-15) and Y (16-31) are therefore re-paired inside each
// 16-lane row with two DPP moves per register (row_ror:8 under a bank mask):
//     X' = lanes 0-7: X of rows 0-7,  lanes 8-15: Y of rows 0-7        Y' = lanes 0-7: X of rows 8-15, lanes 8-15: Y of rows 8-15
// after which lane (rr = lane & 7, ch = (lane >> 3) & 1, g = lane >> 4) of X' holds row rr, columns 16 ch + 4 g + q:
// eight lanes x 16 bytes = one whole 128-byte line per row, eight rows per instruction, every access a 16-byte
// vector: full-line traffic with 4 x fewer memory instructions than the dword-per-lane epilogues of the 32 x 32
// kernels.  Same arithmetic as wire_gemm_epi.h (lean Gabor forms of wire_dev.h).
// ---------------------------------------------------------------------------
WIRE_DEVINL void h_pair_rows(const f32x4& X, const f32x4& Y, f32x4& Xp, f32x4& Yp) {
#pragma unroll
  for (int q = 0; q < 4; ++q) {
    const int x = __float_as_int(X[q]), y = __float_as_int(Y[q]);
    // row_ror:8 = 0x128; bank_mask 0xC writes lanes 8-15 of every 16-lane row, 0x3 lanes 0-7
    Xp[q] = __int_as_float(__builtin_amdgcn_update_dpp(x, y, 0x128, 0xf, 0xc, false));
    Yp[q] = __int_as_float(__builtin_amdgcn_update_dpp(y, x, 0x128, 0xf, 0x3, false));
  }
}

// X2 (wire_gemmx2h.hip, the 2 x fp16 split GEMM): the accumulators carry the operands' power-of-two scales -- they are
// multiplied by acc_scale = 1 / (s_A s_B) first (exact) -- and the epilogue tracks max |value| of the tensor it writes
// that the NEXT GEMM reads as an operand (out for the forward forms, g_lin for the data-gradient forms) into
// ep.amax_out, from which that GEMM derives ITS operand scale.
WIRE_DEVINL void h_amax4(float& m, const f32x4& v) {
  m = __builtin_fmaxf(m, __builtin_fmaxf(__builtin_fmaxf(__builtin_fabsf(v[0]), __builtin_fabsf(v[1])),
                                         __builtin_fmaxf(__builtin_fabsf(v[2]), __builtin_fabsf(v[3]))));
}

// Coordinate-gradient partials (ep.cg_partial): a row's 128 columns of the tile lie in ONE wave, in the 8 lanes that share
// rr (lane bits 3-5: ch, g).  t = this lane's columns' contribution to the row slot e (= 2 rb + hr, 0 .. 2 NRB - 1) is
// summed over those lanes by a fixed butterfly; lane group j = lane >> 3 keeps slot j's sum.  h_cg_store writes it once
// per row and column tile -- no atomics, the same bits every run.
WIRE_DEVINL void h_cg_add(float (&cg)[4], const float (&t)[4], const int e, const int lane) {
#pragma unroll
  for (int d = 0; d < 4; ++d) {
    float v = t[d];
    v += __shfl_xor(v, 8); v += __shfl_xor(v, 16); v += __shfl_xor(v, 32);
    cg[d] += (lane >> 3) == e ? v : 0.f;
  }
}
template <int NRB>
WIRE_DEVINL void h_cg_store(const float (&cg)[4], const GemmEpiParams& ep, const int M, const int m_w, const int n_w,
                            const int lane) {
  const int j = lane >> 3;
  if (j >= 2 * NRB) return;
  const int row = m_w + 16 * (j >> 1) + 8 * (j & 1) + (lane & 7);
  if (row >= M) return;
  float* dst = ep.cg_partial + ((size_t)(n_w >> 7) * (size_t)M + (size_t)row) * ep.D;
  for (int d = 0; d < ep.D; ++d) dst[d] = cg[d];
}

// ---------------------------------------------------------------------------
// The epilogue's first loads, issued by the GEMM under the MFMAs of its last stage (wire_gemmx2h.hip, knob "epi_early")
// and handed to h_epilogue, which then does not load them again: the same values, one memory round trip earlier.
//   HPreLin   EPI_GABOR_BWD | EPI_LA: lin of row block 0 of the first group ([rows 0-7 | 8-15]; the look-ahead itself
//             loads every later block, the second group's first one included, under the block before it)
//   HPreFirst EPI_GABOR_BWD_FIRST | EPI_D2: the lane's coordinates, W0 / b0 of both groups (below)
// A group outside the matrix (the last column tile of a width that is no multiple of 128) is loaded from group 0's
// addresses and not used.  HPreNone: every other form, and "epi_early" = 0 -- among them the forms whose early
// edition spills: lin of both groups' block 0 for EPI_LA (64 bytes per lane), the layer-1 forms with
// EPI_CG or EPI_D3 (16 - 80), and wire2d's layer-1 forms, which spill as they are; and EPI_GABOR_FWD, whose only
// load is 2 KB of bias per tile: loaded early it moved the forward launches by nothing (1.7588 -> 1.7586 ms per step).
// ---------------------------------------------------------------------------
struct HPreNone {};
struct HPreLin { f32x4 u[2], v[2]; };
template <int DN, int NRB> struct HPreFirst { float xs[2 * NRB][DN], w[2][4][DN], bb[2][4]; };
template <int EPIX, int NRB>
using h_pre_t = std::conditional_t<EPIX == (EPI_GABOR_BWD | EPI_LA), HPreLin,
                                   std::conditional_t<EPIX == (EPI_GABOR_BWD_FIRST | EPI_D2), HPreFirst<2, NRB>, HPreNone>>;

WIRE_DEVINL void h_pre_load(HPreNone&, const GemmEpiParams&, const int, const int, const int, const int, const int) {}
WIRE_DEVINL void h_pre_load(HPreLin& pre, const GemmEpiParams& ep, const int M, const int m_w, const int n_w,
                            const int Nc, const int lane) {
  const int rr = lane & 7, cq = 16 * ((lane >> 3) & 1) + 4 * (lane >> 4);
#pragma unroll
  for (int hr = 0; hr < 2; ++hr) {                                // (= load_lin(0, ..) of h_gabor_bwd_la)
    int row = m_w + 8 * hr + rr;
    row = row < M ? row : M - 1;
    const float* Lp = ep.i0 + (size_t)row * ep.ld0 + n_w + cq;
    pre.u[hr] = *reinterpret_cast<const f32x4*>(Lp);
    pre.v[hr] = *reinterpret_cast<const f32x4*>(Lp + 32);
  }
}

// ---------------------------------------------------------------------------
// The layer-1 data-gradient forms of the complex nets with the input width a compile-time constant DN = 2, 3 (EPI_D2,
// EPI_D3; knob "first_dn").  Same values as the plain forms in h_epilogue below, which run every chain over four terms with
// x[d] = w[d] = +0 for d >= D: fmaf(+0, +0, u) = u for every u but -0 (which it turns into +0: the plain form departs
// from first_fwd_kernel's u there, this one does not), and a sum that starts at +0 and only ever adds g * (+0) stays +0
// for finite g -- written out as the constant below, so cr_partial keeps its [.][5] layout.  What else differs is WHEN
// things are loaded: the coordinates of the lane's 2 NRB rows once per tile instead of once per row and column group, the
// first layer's parameters of both column groups ahead of the first group's arithmetic.  Loads of rows >= M read row
// M - 1 and are not used.  The order of every surviving fmaf chain and of the reductions is that of the plain forms.
// ---------------------------------------------------------------------------
template <int DN>
WIRE_DEVINL void h_cg_add_dn(float (&cg)[4], const float (&t)[DN], const int e, const int lane) {
#pragma unroll
  for (int d = 0; d < DN; ++d) {
    float v = t[d];
    v += __shfl_xor(v, 8); v += __shfl_xor(v, 16); v += __shfl_xor(v, 32);
    cg[d] += (lane >> 3) == e ? v : 0.f;
  }
}
template <int DN, int NRB>
WIRE_DEVINL void h_load_rows_dn(float (&xs)[2 * NRB][DN], const GemmEpiParams& ep, const int M, const int m_w, const int rr) {
#pragma unroll
  for (int e = 0; e < 2 * NRB; ++e) {
    int row = m_w + 8 * e + rr;                                   // = m_w + 16 rb + 8 hr + rr, e = 2 rb + hr
    row = row < M ? row : M - 1;
#pragma unroll
    for (int d = 0; d < DN; ++d) xs[e][d] = ep.coords[(size_t)row * DN + d];
  }
}
// sums over the 8 row lanes of each 16-lane row, then into this wave's [64 features][5] of LDS
template <int DN>
WIRE_DEVINL void h_crs_to_lds_dn(const float (&crs)[4][DN + 1], float* red, const int rr) {
#pragma unroll
  for (int q = 0; q < 4; ++q) {
    float o[5] = {0.f, 0.f, 0.f, 0.f, 0.f};
#pragma unroll
    for (int d = 0; d <= DN; ++d) {
      float v = crs[q][d];
      v += __shfl_xor(v, 1); v += __shfl_xor(v, 2); v += __shfl_xor(v, 4);
      o[d < DN ? d : 4] = v;
    }
    if (rr == 0) {
#pragma unroll
      for (int d = 0; d < 5; ++d) red[q * 5 + d] = o[d];
    }
  }
}

// the lane's coordinates and the first layer's parameters of both column groups (pad features: 0)
template <int DN, int NRB>
WIRE_DEVINL void h_pre_load(HPreFirst<DN, NRB>& pre, const GemmEpiParams& ep, const int M, const int m_w, const int n_w,
                            const int Nc, const int lane) {
  const int rr = lane & 7, cq = 16 * ((lane >> 3) & 1) + 4 * (lane >> 4);
  h_load_rows_dn<DN, NRB>(pre.xs, ep, M, m_w, rr);
#pragma unroll
  for (int G = 0; G < 2; ++G) {
    const int c0 = n_w + 64 * G + cq;
    const int f0 = ((c0 >> 6) << 5) + (c0 & 31);
#pragma unroll
    for (int q = 0; q < 4; ++q) {
      const bool valid = f0 + q < ep.kvalid;
      pre.bb[G][q] = valid ? ep.b0[f0 + q] : 0.f;
#pragma unroll
      for (int d = 0; d < DN; ++d) pre.w[G][q][d] = valid ? ep.W0[(f0 + q) * DN + d] : 0.f;
    }
  }
}

// PRE = HPreFirst<DN, NRB>: the GEMM loaded them (above); HPreNone: loaded here
template <bool CG, int DN, int NRB, typename PRE>
WIRE_DEVINL void h_gabor_bwd_first_dn(const f32x4 (&acc)[NRB][8], const GemmEpiParams& ep, const int M, const int m_w,
                                      const int n_w, const int Nc, const int lane, unsigned char* lds, const int wave,
                                      const int rt, const PRE& pre) {
  const int rr = lane & 7, cq = 16 * ((lane >> 3) & 1) + 4 * (lane >> 4);
  const float w0 = ep.omega, m2s2 = -2.f * ep.scale * ep.scale;
  HPreFirst<DN, NRB> ld;
  if constexpr (std::is_same_v<PRE, HPreFirst<DN, NRB>>) ld = pre;
  else h_pre_load(ld, ep, M, m_w, n_w, Nc, lane);
  const auto& xs = ld.xs;
  const auto& w = ld.w;
  const auto& bb = ld.bb;
  float cg[4] = {0.f, 0.f, 0.f, 0.f};
#pragma unroll
  for (int G = 0; G < 2; ++G) {
    if (n_w + 64 * G >= Nc) continue;
    const int c0 = n_w + 64 * G + cq;                             // this lane's first re column; im = + 32
    const int f0 = ((c0 >> 6) << 5) + (c0 & 31);                  // ... = features f0 .. f0 + 3
    float crs[4][DN + 1];                                         // sums of g_u [x | 1]
#pragma unroll
    for (int q = 0; q < 4; ++q)
#pragma unroll
      for (int d = 0; d <= DN; ++d) crs[q][d] = 0.f;
#pragma unroll
    for (int rb = 0; rb < NRB; ++rb) {
      f32x4 are[2], aim[2];
      h_pair_rows(acc[rb][4 * G], acc[rb][4 * G + 1], are[0], are[1]);
      h_pair_rows(acc[rb][4 * G + 2], acc[rb][4 * G + 3], aim[0], aim[1]);
#pragma unroll
      for (int hr = 0; hr < 2; ++hr) {
        const int e = 2 * rb + hr;
        const int row = m_w + 8 * e + rr;
        float t[DN];
#pragma unroll
        for (int d = 0; d < DN; ++d) t[d] = 0.f;
        if (row < M) {
          f32x4 pr = {0.f, 0.f, 0.f, 0.f}, pi = pr;
          if (!ep.recompute_out) {
            const float* Op = ep.i1 + (size_t)row * ep.ld1 + c0;
            pr = *reinterpret_cast<const f32x4*>(Op);
            pi = *reinterpret_cast<const f32x4*>(Op + 32);
          }
          f32x4 gu;
#pragma unroll
          for (int q = 0; q < 4; ++q) {
            float u = bb[G][q];
#pragma unroll
            for (int d = 0; d < DN; ++d) u = __builtin_fmaf(xs[e][d], w[G][q][d], u);
            if (ep.recompute_out) {
              float a, b;
              gabor_fwd_real(u, w0, ep.scale, a, b);
              pr[q] = a; pi[q] = b;
            }
            const float v = gabor_bwd_real(are[hr][q], aim[hr][q], u, pr[q], pi[q], w0, m2s2);
            gu[q] = f0 + q < ep.kvalid ? v : 0.f;
          }
          if constexpr (CG) {                                     // (w is 0 for pad features)
#pragma unroll
            for (int q = 0; q < 4; ++q)
#pragma unroll
              for (int d = 0; d < DN; ++d) t[d] = __builtin_fmaf(gu[q], w[G][q][d], t[d]);
          }
          if (ep.cr_partial) {
#pragma unroll
            for (int q = 0; q < 4; ++q) {
#pragma unroll
              for (int d = 0; d < DN; ++d) crs[q][d] = __builtin_fmaf(gu[q], xs[e][d], crs[q][d]);
              crs[q][DN] += gu[q];
            }
          } else {
            *reinterpret_cast<f32x4*>(ep.o0 + (size_t)row * ep.ldu + f0) = gu;
          }
        }
        if constexpr (CG) h_cg_add_dn<DN>(cg, t, e, lane);
      }
    }
    if (ep.cr_partial)   // (the main loop is over: every wave has passed its last barrier, the stage buffers are free)
      h_crs_to_lds_dn<DN>(crs, reinterpret_cast<float*>(lds) + (wave * 64 + 32 * G + cq) * 5, rr);
  }
  if (ep.cr_partial) {                                            // the four waves: (w0 + w1) + (w2 + w3)
    __syncthreads();
    const float* red = reinterpret_cast<const float*>(lds);       // [4 waves][64 features][5]
    const int fbase = (n_w >> 6) << 5;                            // first complex feature of this 128-column tile
    for (int e = threadIdx.x; e < 64 * 5; e += 256) {
      const int f = e / 5, d = e - 5 * f;
      const float v = (red[e] + red[64 * 5 + e]) + (red[2 * 64 * 5 + e] + red[3 * 64 * 5 + e]);
      if (fbase + f < ep.cr_C) ep.cr_partial[((size_t)rt * ep.cr_C + fbase + f) * 5 + d] = v;
    }
  }
  if constexpr (CG) h_cg_store<NRB>(cg, ep, M, m_w, n_w, lane);
}

template <bool CG, int DN, int NRB>
WIRE_DEVINL void h_gabor2d_bwd_first_dn(const f32x4 (&acc)[NRB][8], const GemmEpiParams& ep, const int M, const int m_w,
                                        const int n_w, const int Nc, const int lane, unsigned char* lds, const int wave,
                                        const int rt) {
  const int rr = lane & 7, cq = 16 * ((lane >> 3) & 1) + 4 * (lane >> 4);
  const float m2s2 = -2.f * ep.scale * ep.scale, w0 = ep.omega;
  float xs[2 * NRB][DN];
  h_load_rows_dn<DN, NRB>(xs, ep, M, m_w, rr);
  float w[2][4][DN], wv[2][4][DN], bb[2][4], bv2[2][4];
#pragma unroll
  for (int G = 0; G < 2; ++G) {
    const int c0 = n_w + 64 * G + cq;
    const int f0 = ((c0 >> 6) << 5) + (c0 & 31);
#pragma unroll
    for (int q = 0; q < 4; ++q) {
      const bool valid = f0 + q < ep.kvalid;
      bb[G][q] = valid ? ep.b0[f0 + q] : 0.f;
      bv2[G][q] = valid ? ep.b0b[f0 + q] : 0.f;
#pragma unroll
      for (int d = 0; d < DN; ++d) {
        w[G][q][d] = valid ? ep.W0[(f0 + q) * DN + d] : 0.f;
        wv[G][q][d] = valid ? ep.W0b[(f0 + q) * DN + d] : 0.f;
      }
    }
  }
  float cg[4] = {0.f, 0.f, 0.f, 0.f};
#pragma unroll
  for (int G = 0; G < 2; ++G) {
    if (n_w + 64 * G >= Nc) continue;
    const int c0 = n_w + 64 * G + cq;                             // re column of g_out / out; im = + 32
    const int f0 = ((c0 >> 6) << 5) + (c0 & 31);
    float cru[4][DN + 1], crp2[4][DN + 1];                        // sums of g_u [x | 1], g_p [x | 1]
#pragma unroll
    for (int q = 0; q < 4; ++q)
#pragma unroll
      for (int d = 0; d <= DN; ++d) { cru[q][d] = 0.f; crp2[q][d] = 0.f; }
#pragma unroll
    for (int rb = 0; rb < NRB; ++rb) {
      f32x4 are[2], aim[2];
      h_pair_rows(acc[rb][4 * G], acc[rb][4 * G + 1], are[0], are[1]);
      h_pair_rows(acc[rb][4 * G + 2], acc[rb][4 * G + 3], aim[0], aim[1]);
      f32x4 pr[2], pi[2];
#pragma unroll
      for (int hr = 0; hr < 2; ++hr) {
        int row = m_w + 16 * rb + 8 * hr + rr;
        row = row < M ? row : M - 1;
        const float* Op = ep.i1 + (size_t)row * ep.ld1 + c0;
        pr[hr] = *reinterpret_cast<const f32x4*>(Op);
        pi[hr] = *reinterpret_cast<const f32x4*>(Op + 32);
      }
#pragma unroll
      for (int hr = 0; hr < 2; ++hr) {
        const int e = 2 * rb + hr;
        const int row = m_w + 8 * e + rr;
        f32x4 g0, g2;
#pragma unroll
        for (int q = 0; q < 4; ++q) {
          float uu = bb[G][q], p2 = bv2[G][q];
#pragma unroll
          for (int d = 0; d < DN; ++d) {
            uu = __builtin_fmaf(xs[e][d], w[G][q][d], uu);
            p2 = __builtin_fmaf(xs[e][d], wv[G][q][d], p2);
          }
          const float gr = are[hr][q], gi = aim[hr][q];
          const float c_r = __builtin_fmaf(pr[hr][q], gr, pi[hr][q] * gi);
          const float c_i = __builtin_fmaf(pr[hr][q], gi, -(pi[hr][q] * gr));
          const float tt = m2s2 * c_r;
          g0[q] = __builtin_fmaf(tt, uu, w0 * c_i);
          g2[q] = tt * p2;
        }
        if constexpr (CG) {                                       // (w, wv are 0 for pad features)
          float t[DN];
#pragma unroll
          for (int d = 0; d < DN; ++d) t[d] = 0.f;
          if (row < M) {
#pragma unroll
            for (int q = 0; q < 4; ++q)
#pragma unroll
              for (int d = 0; d < DN; ++d)
                t[d] = __builtin_fmaf(g2[q], wv[G][q][d], __builtin_fmaf(g0[q], w[G][q][d], t[d]));
          }
          h_cg_add_dn<DN>(cg, t, e, lane);
        }
        if (row < M) {
#pragma unroll
          for (int q = 0; q < 4; ++q)
            if (!(f0 + q < ep.kvalid)) { g0[q] = 0.f; g2[q] = 0.f; }
          if (ep.cr_partial) {
#pragma unroll
            for (int q = 0; q < 4; ++q) {
#pragma unroll
              for (int d = 0; d < DN; ++d) {
                cru[q][d] = __builtin_fmaf(g0[q], xs[e][d], cru[q][d]);
                crp2[q][d] = __builtin_fmaf(g2[q], xs[e][d], crp2[q][d]);
              }
              cru[q][DN] += g0[q];
              crp2[q][DN] += g2[q];
            }
          } else {
            float* Gp = ep.o0 + (size_t)row * (2 * ep.ldu);
            *reinterpret_cast<f32x4*>(Gp + f0) = g0;
            *reinterpret_cast<f32x4*>(Gp + ep.ldu + f0) = g2;
          }
        }
      }
    }
    if (ep.cr_partial) {                                          // [2 sets][4 waves][64 features][5]
      float* red = reinterpret_cast<float*>(lds) + (wave * 64 + 32 * G + cq) * 5;
      h_crs_to_lds_dn<DN>(cru, red, rr);
      h_crs_to_lds_dn<DN>(crp2, red + 4 * 64 * 5, rr);
    }
  }
  if (ep.cr_partial) {
    __syncthreads();
    const float* red = reinterpret_cast<const float*>(lds);
    const int fbase = (n_w >> 6) << 5;                            // first feature of this 128-column tile
    for (int e = threadIdx.x; e < 2 * 64 * 5; e += 256) {
      const int set = e / (64 * 5), r = e - set * (64 * 5);
      const int f = r / 5, d = r - 5 * f;
      const float* rs = red + set * (4 * 64 * 5);
      const float v = (rs[r] + rs[64 * 5 + r]) + (rs[2 * 64 * 5 + r] + rs[3 * 64 * 5 + r]);
      if (fbase + f < ep.cr_C)
        ep.cr_partial[(size_t)set * ep.cr_set + ((size_t)rt * ep.cr_C + fbase + f) * 5 + d] = v;
    }
  }
  if constexpr (CG) h_cg_store<NRB>(cg, ep, M, m_w, n_w, lane);
}

// ---------------------------------------------------------------------------
// EPI_GABOR_BWD with one row block of look-ahead (EPI_LA; knob "bwd_lookahead").  The plain form in h_epilogue loads lin
// of a 16-row block, computes, stores g_lin and only then loads the next block: nothing tells the compiler that ep.i0 and
// ep.o0 are different buffers, so it may not move a load above the stores before it -- eight serialised round trips to
// memory per wave and tile.  Here the loads of block i + 1 (the next 16 rows, then the second 64-column group) are
// issued in program order BEFORE the arithmetic and stores of block i, into registers of their own (16; the accumulators
// of finished blocks are dead by then).  Same arithmetic on the same values: the caller guarantees that lin and g_lin do
// not overlap (the whole-net calls: activation buffer and scratch).  This edition always evaluates out = act(lin) again
// (ep.recompute_out, the default): with the branch that reads out instead in the same code, the wait counts at the point
// where the two paths meet are those of the reading path, and the look-ahead loads are waited for right after their issue.
// (Tried and dropped: a second copy of the loop with unconditional stores for waves whose rows all lie inside the matrix,
// so that the waits need not allow for a store that was branched over -- the freer schedule spills, 64 - 104 bytes.)
// ---------------------------------------------------------------------------
// PRE = HPreLin: row block 0 came in under the GEMM's last stage (h_pre_load above)
template <bool X2, int NRB, typename PRE>
WIRE_DEVINL void h_gabor_bwd_la(const f32x4 (&acc)[NRB][8], const GemmEpiParams& ep, const int M, const int m_w,
                                const int n_w, const int Nc, const int lane, float& amx, const PRE& pre) {
  constexpr bool EARLY = std::is_same_v<PRE, HPreLin>;
  const int rr = lane & 7, cq = 16 * ((lane >> 3) & 1) + 4 * (lane >> 4);
  const float w0 = ep.omega, w0l2e = ep.omega * 1.44269502f, ns2l2e = -(ep.scale * ep.scale) * 1.44269502f;
  const float m2s2 = -2.f * ep.scale * ep.scale;
  const int ngrp = n_w + 64 >= Nc ? 1 : 2;                        // 64-column groups of this tile inside the matrix
  auto load_lin = [&](const int i, f32x4 (&u)[2], f32x4 (&v)[2]) {
    const int G = i / NRB, rb = i % NRB;
#pragma unroll
    for (int hr = 0; hr < 2; ++hr) {
      int row = m_w + 16 * rb + 8 * hr + rr;
      row = row < M ? row : M - 1;
      const float* Lp = ep.i0 + (size_t)row * ep.ld0 + n_w + 64 * G + cq;
      u[hr] = *reinterpret_cast<const f32x4*>(Lp);
      v[hr] = *reinterpret_cast<const f32x4*>(Lp + 32);
    }
  };
  f32x4 lu[2], lv[2];
  if constexpr (EARLY) { lu[0] = pre.u[0]; lu[1] = pre.u[1]; lv[0] = pre.v[0]; lv[1] = pre.v[1]; }
  else load_lin(0, lu, lv);
#pragma unroll
  for (int i = 0; i < 2 * NRB; ++i) {
    const int G = i / NRB, rb = i % NRB;
    if (G >= ngrp) break;
    const int c0 = n_w + 64 * G + cq;                             // this lane's first re column; im = + 32
    const int f0 = ((c0 >> 6) << 5) + (c0 & 31);                  // ... = features f0 .. f0 + 3
    f32x4 nu[2] = {lu[0], lu[1]}, nv[2] = {lv[0], lv[1]};
    const bool more = i + 1 < 2 * NRB && (i + 1) / NRB < ngrp;
    if (more) load_lin(i + 1, nu, nv);
    f32x4 are[2], aim[2], pr[2], pi[2];
    h_pair_rows(acc[rb][4 * G], acc[rb][4 * G + 1], are[0], are[1]);
    h_pair_rows(acc[rb][4 * G + 2], acc[rb][4 * G + 3], aim[0], aim[1]);
#pragma unroll
    for (int hr = 0; hr < 2; ++hr)
#pragma unroll
      for (int q = 0; q < 4; ++q) {
        float a, b;
        gabor_fwd_lean(lu[hr][q], lv[hr][q], w0, w0l2e, ns2l2e, a, b);
        const bool valid = f0 + q < ep.kvalid;
        pr[hr][q] = valid ? a : 0.f;
        pi[hr][q] = valid ? b : 0.f;
      }
#pragma unroll
    for (int hr = 0; hr < 2; ++hr) {
      const int row = m_w + 16 * rb + 8 * hr + rr;
      f32x4 gl_re, gl_im;
#pragma unroll
      for (int q = 0; q < 4; ++q) {
        const float gr = are[hr][q], gi = aim[hr][q];
        const float c_r = __builtin_fmaf(pr[hr][q], gr, pi[hr][q] * gi);
        const float c_i = __builtin_fmaf(pr[hr][q], gi, -(pi[hr][q] * gr));
        const float tt = m2s2 * c_r;
        gl_re[q] = __builtin_fmaf(tt, lu[hr][q], w0 * c_i);
        gl_im[q] = __builtin_fmaf(tt, lv[hr][q], -(w0 * c_r));
      }
      if constexpr (X2) { h_amax4(amx, gl_re); h_amax4(amx, gl_im); }
      if (row < M) {
        float* Gp = ep.o0 + (size_t)row * ep.ld0 + c0;
        *reinterpret_cast<f32x4*>(Gp) = gl_re;
        *reinterpret_cast<f32x4*>(Gp + 32) = gl_im;
      }
    }
#pragma unroll
    for (int hr = 0; hr < 2; ++hr) { lu[hr] = nu[hr]; lv[hr] = nv[hr]; }
  }
}

// NRB = 16-row blocks of the wave's tile (4: 64 rows per wave, 256-row workgroup tiles; 2: 32 rows per wave, 128-row tiles
// -- not with the first-layer sums (cr_partial), whose per-tile layout is that of the 256-row tile)
// EPIX = an EPI_* code, | EPI_CG for the layer-1 data-gradient forms that also write coordinate-gradient partials
// (ep.cg_partial): a separate instantiation, so the forms without it keep their registers; | EPI_D2 or EPI_D3 for the
// compile-time-width editions of the *_BWD_FIRST forms above; | EPI_LA for the look-ahead edition of GABOR_BWD
// PRE = h_pre_t<EPIX, NRB>: the form's first loads, already issued by the caller (h_pre_load); HPreNone: none
template <int EPIX, bool X2 = false, int NRB = 4, typename PRE = HPreNone>
WIRE_DEVINL void h_epilogue(f32x4 (&acc)[NRB][8], const GemmEpiParams& ep, const int M, const int m_w, const int n_w,
                            const int Nc, const int lane, unsigned char* lds, const int wave, const int rt,
                            const float acc_scale = 1.f, const PRE& pre = PRE{}) {
  constexpr int EPI = EPIX & ~EPI_FLAGS;
  constexpr bool EARLY = !std::is_same_v<PRE, HPreNone>;
  static_assert(!EARLY || std::is_same_v<PRE, h_pre_t<EPIX, NRB>>, "the early loads of this form");
  constexpr bool CG = (EPIX & EPI_CG) != 0;
  constexpr int DN = (EPIX & EPI_D2) ? 2 : (EPIX & EPI_D3) ? 3 : 0;   // compile-time input width of the *_BWD_FIRST forms
  constexpr bool LA = (EPIX & EPI_LA) != 0;
  static_assert(!LA || EPI == EPI_GABOR_BWD, "EPI_LA: the hidden-layer data gradient of the 1-D Gabor net");
  static_assert(DN == 0 || ((EPI == EPI_GABOR_BWD_FIRST || EPI == EPI_GABOR2D_BWD_FIRST) && NRB == 4),
                "EPI_D2 / EPI_D3: the layer-1 forms of the complex nets on the 256-row tile");
  const int rr = lane & 7, ch = (lane >> 3) & 1, g = lane >> 4;
  float amx = 0.f;
  if constexpr (X2) {
#pragma unroll
    for (int i = 0; i < NRB; ++i)
#pragma unroll
      for (int j = 0; j < 8; ++j)
#pragma unroll
        for (int q = 0; q < 4; ++q) acc[i][j][q] *= acc_scale;
  }
  const int cq = 16 * ch + 4 * g;                                 // this lane's first column inside a 32-column span
  if constexpr (EPI == EPI_STORE) {
#pragma unroll
    for (int sp = 0; sp < 4; ++sp) {                              // 32-column spans of the 128-column wave tile
      const int col = n_w + 32 * sp + cq;
      if (n_w + 32 * sp >= Nc) continue;
#pragma unroll
      for (int rb = 0; rb < NRB; ++rb) {
        f32x4 xp, yp;
        h_pair_rows(acc[rb][2 * sp], acc[rb][2 * sp + 1], xp, yp);
        const int row = m_w + 16 * rb + rr;
        if (row < M) *reinterpret_cast<f32x4*>(ep.o0 + (size_t)row * ep.ld0 + col) = xp;
        if (row + 8 < M) *reinterpret_cast<f32x4*>(ep.o0 + (size_t)(row + 8) * ep.ld0 + col) = yp;
      }
    }
  } else if constexpr (epi_real_fwd(EPI)) {
    constexpr int ACT = epi_real_act(EPI);
#pragma unroll
    for (int sp = 0; sp < 4; ++sp) {
      if (n_w + 32 * sp >= Nc) continue;
      const int col = n_w + 32 * sp + cq;
      const f32x4 bv = *reinterpret_cast<const f32x4*>(ep.bias + col);
#pragma unroll
      for (int rb = 0; rb < NRB; ++rb) {
        f32x4 a2[2];
        h_pair_rows(acc[rb][2 * sp], acc[rb][2 * sp + 1], a2[0], a2[1]);
#pragma unroll
        for (int hr = 0; hr < 2; ++hr) {
          const int row = m_w + 16 * rb + 8 * hr + rr;
          f32x4 lin;
#pragma unroll
          for (int q = 0; q < 4; ++q) lin[q] = a2[hr][q] + bv[q];
          if (ep.o0 && row < M) *reinterpret_cast<f32x4*>(ep.o0 + (size_t)row * ep.ld0 + col) = lin;
          if (ep.o1) {                                             // null: last hidden layer of a fused training step
            f32x4 o;
#pragma unroll
            for (int q = 0; q < 4; ++q) {
              const float v = real_act_fwd_lean<ACT>(lin[q], ep.omega, ep.scale);
              o[q] = col + q < ep.kvalid ? v : 0.f;                // pad features are written as 0
            }
            if constexpr (X2) h_amax4(amx, o);
            if (row < M) wire_store_out4(ep.o1 + (size_t)row * ep.ld1 + col, o, X2 ? ep.o1_split : 0.f);
          }
        }
      }
    }
  } else if constexpr (epi_real_bwd(EPI)) {
    constexpr int ACT = epi_real_act(EPI);
    float cg[4] = {0.f, 0.f, 0.f, 0.f};                           // cg_partial: this lane group's row sums of g_lin_0 W0
#pragma unroll
    for (int sp = 0; sp < 4; ++sp) {
      if (n_w + 32 * sp >= Nc) continue;
      const int col = n_w + 32 * sp + cq;
      float crs[4][5];                                            // cr_partial: sums of g_lin_0 [x | 1] over this lane's rows
#pragma unroll
      for (int q = 0; q < 4; ++q)
#pragma unroll
        for (int d = 0; d < 5; ++d) crs[q][d] = 0.f;
#pragma unroll
      for (int rp = 0; rp < NRB; rp += 2) {
        f32x4 lv[4], ov[4], a2[4];
#pragma unroll
        for (int r2 = 0; r2 < 2; ++r2) {
          h_pair_rows(acc[rp + r2][2 * sp], acc[rp + r2][2 * sp + 1], a2[2 * r2], a2[2 * r2 + 1]);
#pragma unroll
          for (int hr = 0; hr < 2; ++hr) {
            int row = m_w + 16 * (rp + r2) + 8 * hr + rr;
            row = row < M ? row : M - 1;
            // siren / B-spline need lin, relu needs out (its lin is never stored), gauss both
            lv[2 * r2 + hr] = (ACT != ACT_RELU) ? *reinterpret_cast<const f32x4*>(ep.i0 + (size_t)row * ep.ld0 + col)
                                                : f32x4{0.f, 0.f, 0.f, 0.f};
            const bool load_out = ACT == ACT_RELU || (ACT == ACT_GAUSS && !ep.recompute_out);
            ov[2 * r2 + hr] = load_out ? *reinterpret_cast<const f32x4*>(ep.i1 + (size_t)row * ep.ld1 + col)
                                       : f32x4{0.f, 0.f, 0.f, 0.f};
          }
        }
        if (ACT == ACT_GAUSS && ep.recompute_out) {                // out = exp(-(s0 lin)^2) again: the forward's lean form
#pragma unroll
          for (int e = 0; e < 4; ++e)
#pragma unroll
            for (int q = 0; q < 4; ++q) {
              const float v = real_act_fwd_lean<ACT>(lv[e][q], ep.omega, ep.scale);
              ov[e][q] = col + q < ep.kvalid ? v : 0.f;
            }
        }
#pragma unroll
        for (int e = 0; e < 4; ++e) {
          const int row = m_w + 16 * (rp + (e >> 1)) + 8 * (e & 1) + rr;
          f32x4 gl;
#pragma unroll
          for (int q = 0; q < 4; ++q) gl[q] = real_act_bwd_lean<ACT>(a2[e][q], lv[e][q], ov[e][q], ep.omega, ep.scale);
          if constexpr (X2) h_amax4(amx, gl);
          if constexpr (CG) {
            float t[4] = {0.f, 0.f, 0.f, 0.f};
            if (row < M) {                                        // (W0 from L1: 16 more registers here spill)
#pragma unroll
              for (int q = 0; q < 4; ++q) {
                if (col + q >= ep.kvalid) continue;
                for (int d = 0; d < ep.D; ++d) t[d] = __builtin_fmaf(gl[q], ep.W0[(col + q) * ep.D + d], t[d]);
              }
            }
            h_cg_add(cg, t, 2 * (rp + (e >> 1)) + (e & 1), lane);
          }
          if (row < M) {
            if (ep.cr_partial) {
              // first layer of a real net: its weight / bias gradient sums g_lin_0 [x | 1] are formed here (what
              // colreduce_kernel would form from the stored g_lin_0 -- which is then never written)
              float x[4] = {0.f, 0.f, 0.f, 0.f};
              for (int d = 0; d < ep.D; ++d) x[d] = ep.coords[(size_t)row * ep.D + d];
#pragma unroll
              for (int q = 0; q < 4; ++q) {
#pragma unroll
                for (int d = 0; d < 4; ++d) crs[q][d] = __builtin_fmaf(gl[q], x[d], crs[q][d]);
                crs[q][4] += gl[q];
              }
            } else {
              *reinterpret_cast<f32x4*>(ep.o0 + (size_t)row * ep.ld0 + col) = gl;
            }
          }
        }
      }
      if (ep.cr_partial) {                                         // 8 row lanes by shuffles; the 4 waves through LDS below
        float* red = reinterpret_cast<float*>(lds);                // [4 waves][128 columns][5]
#pragma unroll
        for (int q = 0; q < 4; ++q)
#pragma unroll
          for (int d = 0; d < 5; ++d) {
            float v = crs[q][d];
            v += __shfl_xor(v, 1); v += __shfl_xor(v, 2); v += __shfl_xor(v, 4);
            if (rr == 0) red[(wave * 128 + 32 * sp + cq + q) * 5 + d] = v;
          }
      }
    }
    if (ep.cr_partial) {
      __syncthreads();
      const float* red = reinterpret_cast<const float*>(lds);
      for (int e = threadIdx.x; e < 128 * 5; e += 256) {
        const int c = e / 5, d = e - 5 * c;
        const float v = (red[e] + red[128 * 5 + e]) + (red[2 * 128 * 5 + e] + red[3 * 128 * 5 + e]);
        if (n_w + c < ep.cr_C) ep.cr_partial[((size_t)rt * ep.cr_C + n_w + c) * 5 + d] = v;
      }
    }
    if constexpr (CG) h_cg_store<NRB>(cg, ep, M, m_w, n_w, lane);
  } else if constexpr (EPI == EPI_MFN_FWD || EPI == EPI_MFN_BWD) {
    // one span of 32 columns at a time: this lane's four columns of the filter table stay in registers over the rows
#pragma unroll 1
    for (int sp = 0; sp < 4; ++sp) {
      if (n_w + 32 * sp >= Nc) continue;
      const int col = n_w + 32 * sp + cq;
      const bool filt = EPI == EPI_MFN_FWD || ep.i0 != nullptr;
      MfnCol fc[4];
      f32x4 bv = {0.f, 0.f, 0.f, 0.f};
      if (filt) {
#pragma unroll
        for (int q = 0; q < 4; ++q) fc[q] = mfn_load(ep.ftab, col + q);
      }
      if constexpr (EPI == EPI_MFN_FWD) bv = *reinterpret_cast<const f32x4*>(ep.bias + col);
#pragma unroll
      for (int rb = 0; rb < NRB; ++rb) {
        f32x4 a2[2];
        // (sp is a runtime index here: the accumulator pair is selected below)
        f32x4 ax = acc[rb][0], ay = acc[rb][1];
        if (sp == 1) { ax = acc[rb][2]; ay = acc[rb][3]; }
        if (sp == 2) { ax = acc[rb][4]; ay = acc[rb][5]; }
        if (sp == 3) { ax = acc[rb][6]; ay = acc[rb][7]; }
        h_pair_rows(ax, ay, a2[0], a2[1]);
#pragma unroll
        for (int hr = 0; hr < 2; ++hr) {
          const int row = m_w + 16 * rb + 8 * hr + rr;
          const int rowc = row < M ? row : M - 1;
          float x[4] = {0.f, 0.f, 0.f, 0.f};
          f32x4 g = {0.f, 0.f, 0.f, 0.f};
          if (filt) {
            mfn_load_x(ep.coords, rowc, ep.D, x);
#pragma unroll
            for (int q = 0; q < 4; ++q) g[q] = mfn_g(fc[q], x);
          }
          if constexpr (EPI == EPI_MFN_FWD) {
            f32x4 lin, o;
#pragma unroll
            for (int q = 0; q < 4; ++q) {
              lin[q] = a2[hr][q] + bv[q];
              o[q] = col + q < ep.kvalid ? lin[q] * g[q] : 0.f;
            }
            if constexpr (X2) h_amax4(amx, o);
            if (row < M) {
              if (ep.o0) *reinterpret_cast<f32x4*>(ep.o0 + (size_t)row * ep.ld0 + col) = lin;
              *reinterpret_cast<f32x4*>(ep.o1 + (size_t)row * ep.ld1 + col) = o;
            }
          } else {
            if (filt) {
              const f32x4 lin = *reinterpret_cast<const f32x4*>(ep.i0 + (size_t)rowc * ep.ld0 + col);
              f32x4 gl, hh;
#pragma unroll
              for (int q = 0; q < 4; ++q) { gl[q] = a2[hr][q] * g[q]; hh[q] = a2[hr][q] * lin[q]; }
              if constexpr (X2) h_amax4(amx, gl);
              if (row < M) {
                *reinterpret_cast<f32x4*>(ep.o0 + (size_t)row * ep.ld0 + col) = gl;
                *reinterpret_cast<f32x4*>(ep.o1 + (size_t)row * ep.ld1 + col) = hh;
              }
            } else if (row < M) {
              *reinterpret_cast<f32x4*>(ep.o1 + (size_t)row * ep.ld1 + col) = a2[hr];
            }
          }
        }
      }
    }
  } else if constexpr (EPI == EPI_GABOR2D_FWD) {
    // the wave's 128 columns = (lin_re | lin_im | sy_re | sy_im) of 32 features (modules/wire2d.py:56-67)
    const int grp = n_w >> 7;
    const int f0 = (grp << 5) + cq;                               // features f0 .. f0 + 3
    const int oc = (grp << 6) + cq;                               // re column in the P-wide output row; im = + 32
    f32x4 bv[4];
#pragma unroll
    for (int k = 0; k < 4; ++k) bv[k] = *reinterpret_cast<const f32x4*>(ep.bias + n_w + 32 * k + cq);
#pragma unroll
    for (int rb = 0; rb < NRB; ++rb) {
      f32x4 part[4][2];
#pragma unroll
      for (int k = 0; k < 4; ++k) h_pair_rows(acc[rb][2 * k], acc[rb][2 * k + 1], part[k][0], part[k][1]);
#pragma unroll
      for (int hr = 0; hr < 2; ++hr) {
        const int row = m_w + 16 * rb + 8 * hr + rr;
        f32x4 u, v, pp, qq;
#pragma unroll
        for (int q = 0; q < 4; ++q) {
          u[q] = part[0][hr][q] + bv[0][q];
          v[q] = part[1][hr][q] + bv[1][q];
          pp[q] = part[2][hr][q] + bv[2][q];
          qq[q] = part[3][hr][q] + bv[3][q];
        }
        if (ep.o0 && row < M) {
          float* Lp = ep.o0 + (size_t)row * ep.ld0 + n_w + cq;
          *reinterpret_cast<f32x4*>(Lp) = u;
          *reinterpret_cast<f32x4*>(Lp + 32) = v;
          *reinterpret_cast<f32x4*>(Lp + 64) = pp;
          *reinterpret_cast<f32x4*>(Lp + 96) = qq;
        }
        if (ep.o1) {                                              // null: last hidden layer of a fused training step
          f32x4 o_re, o_im;
#pragma unroll
          for (int q = 0; q < 4; ++q) {
            float a, b;
            gabor2d_fwd_lean(u[q], v[q], pp[q], qq[q], ep.omega, ep.scale, a, b);
            const bool valid = f0 + q < ep.kvalid;
            o_re[q] = valid ? a : 0.f;
            o_im[q] = valid ? b : 0.f;
          }
          if constexpr (X2) { h_amax4(amx, o_re); h_amax4(amx, o_im); }
          if (row < M) {
            float* Op = ep.o1 + (size_t)row * ep.ld1 + oc;
            wire_store_out4(Op, o_re, X2 ? ep.o1_split : 0.f);
            wire_store_out4(Op + 32, o_im, X2 ? ep.o1_split : 0.f);
          }
        }
      }
    }
  } else if constexpr (EPI == EPI_GABOR_BWD && LA) {
    h_gabor_bwd_la<X2, NRB>(acc, ep, M, m_w, n_w, Nc, lane, amx, pre);
  } else if constexpr (EPI == EPI_GABOR_BWD_FIRST && DN != 0) {
    h_gabor_bwd_first_dn<CG, DN, NRB>(acc, ep, M, m_w, n_w, Nc, lane, lds, wave, rt, pre);
  } else if constexpr (EPI == EPI_GABOR2D_BWD_FIRST && DN != 0) {
    h_gabor2d_bwd_first_dn<CG, DN, NRB>(acc, ep, M, m_w, n_w, Nc, lane, lds, wave, rt);
  } else if constexpr (EPI == EPI_GABOR2D_BWD || EPI == EPI_GABOR2D_BWD_FIRST) {
    // C = g_out (re | im pairs, P wide); writes g_(lin | sy) into the 2P-wide row (or the real g_(u | p) of layer 0)
    const float m2s2 = -2.f * ep.scale * ep.scale, w0 = ep.omega;
    float cg[4] = {0.f, 0.f, 0.f, 0.f};                           // BWD_FIRST with cg_partial: row sums of g_u W0 + g_p V0
#pragma unroll
    for (int G = 0; G < 2; ++G) {
      if (n_w + 64 * G >= Nc) continue;
      const int c0 = n_w + 64 * G + cq;                           // re column of g_out / out; im = + 32
      const int grp = c0 >> 6;
      const int f0 = (grp << 5) + (c0 & 31);
      const int lc = (grp << 7) + (c0 & 31);                      // lin_re column in the 2P row
      float w[4][4], wv[4][4], bb[4], bv2[4];
      float cru[4][5], crp2[4][5];                                // BWD_FIRST with cr_partial: sums of g_u [x | 1], g_p [x | 1]
#pragma unroll
      for (int q = 0; q < 4; ++q)
#pragma unroll
        for (int d = 0; d < 5; ++d) { cru[q][d] = 0.f; crp2[q][d] = 0.f; }
      if constexpr (EPI == EPI_GABOR2D_BWD_FIRST) {
#pragma unroll
        for (int q = 0; q < 4; ++q) {
          const bool valid = f0 + q < ep.kvalid;
          bb[q] = valid ? ep.b0[f0 + q] : 0.f;
          bv2[q] = valid ? ep.b0b[f0 + q] : 0.f;
#pragma unroll
          for (int d = 0; d < 4; ++d) {
            w[q][d] = (valid && d < ep.D) ? ep.W0[(f0 + q) * ep.D + d] : 0.f;
            wv[q][d] = (valid && d < ep.D) ? ep.W0b[(f0 + q) * ep.D + d] : 0.f;
          }
        }
      }
#pragma unroll
      for (int rb = 0; rb < NRB; ++rb) {
        f32x4 are[2], aim[2];
        h_pair_rows(acc[rb][4 * G], acc[rb][4 * G + 1], are[0], are[1]);
        h_pair_rows(acc[rb][4 * G + 2], acc[rb][4 * G + 3], aim[0], aim[1]);
        f32x4 u[2], v[2], pp[2], qq[2], pr[2], pi[2];
        float xs[2][4];                                           // BWD_FIRST: the rows' coordinates
#pragma unroll
        for (int hr = 0; hr < 2; ++hr) {
          int row = m_w + 16 * rb + 8 * hr + rr;
          row = row < M ? row : M - 1;
          const bool recompute = EPI == EPI_GABOR2D_BWD && ep.recompute_out != 0;
          if (!recompute) {
            const float* Op = ep.i1 + (size_t)row * ep.ld1 + c0;
            pr[hr] = *reinterpret_cast<const f32x4*>(Op);
            pi[hr] = *reinterpret_cast<const f32x4*>(Op + 32);
          }
          if constexpr (EPI == EPI_GABOR2D_BWD) {
            const float* Lp = ep.i0 + (size_t)row * ep.ld0 + lc;
            u[hr] = *reinterpret_cast<const f32x4*>(Lp);
            v[hr] = *reinterpret_cast<const f32x4*>(Lp + 32);
            pp[hr] = *reinterpret_cast<const f32x4*>(Lp + 64);
            qq[hr] = *reinterpret_cast<const f32x4*>(Lp + 96);
            if (recompute) {                                      // out = act(lin, sy) again: the forward's lean form
#pragma unroll
              for (int q = 0; q < 4; ++q) {
                float a, b;
                gabor2d_fwd_lean(u[hr][q], v[hr][q], pp[hr][q], qq[hr][q], ep.omega, ep.scale, a, b);
                const bool valid = f0 + q < ep.kvalid;
                pr[hr][q] = valid ? a : 0.f;
                pi[hr][q] = valid ? b : 0.f;
              }
            }
          } else {
            float x[4] = {0.f, 0.f, 0.f, 0.f};
            for (int d = 0; d < ep.D; ++d) x[d] = ep.coords[(size_t)row * ep.D + d];
#pragma unroll
            for (int d = 0; d < 4; ++d) xs[hr][d] = x[d];
#pragma unroll
            for (int q = 0; q < 4; ++q) {
              float uu = bb[q], p2 = bv2[q];
#pragma unroll
              for (int d = 0; d < 4; ++d) { uu = __builtin_fmaf(x[d], w[q][d], uu); p2 = __builtin_fmaf(x[d], wv[q][d], p2); }
              u[hr][q] = uu; pp[hr][q] = p2; v[hr][q] = 0.f; qq[hr][q] = 0.f;
            }
          }
        }
#pragma unroll
        for (int hr = 0; hr < 2; ++hr) {
          const int row = m_w + 16 * rb + 8 * hr + rr;
          f32x4 g0, g1, g2, g3;
#pragma unroll
          for (int q = 0; q < 4; ++q) {
            const float gr = are[hr][q], gi = aim[hr][q];
            const float c_r = __builtin_fmaf(pr[hr][q], gr, pi[hr][q] * gi);
            const float c_i = __builtin_fmaf(pr[hr][q], gi, -(pi[hr][q] * gr));
            const float tt = m2s2 * c_r;
            g0[q] = __builtin_fmaf(tt, u[hr][q], w0 * c_i);      // g_lin = -2 s^2 P lin - j w0 c  (real part / real first layer)
            g1[q] = __builtin_fmaf(tt, v[hr][q], -(w0 * c_r));
            g2[q] = tt * pp[hr][q];                               // g_sy = -2 s^2 P sy
            g3[q] = tt * qq[hr][q];
          }
          if constexpr (X2 && EPI == EPI_GABOR2D_BWD) { h_amax4(amx, g0); h_amax4(amx, g1); h_amax4(amx, g2); h_amax4(amx, g3); }
          if constexpr (EPI == EPI_GABOR2D_BWD_FIRST) {
            if constexpr (CG) {                                   // (w, wv are 0 for pad features and d >= D)
              float t[4] = {0.f, 0.f, 0.f, 0.f};
              if (row < M) {
#pragma unroll
                for (int q = 0; q < 4; ++q)
#pragma unroll
                  for (int d = 0; d < 4; ++d) t[d] = __builtin_fmaf(g2[q], wv[q][d], __builtin_fmaf(g0[q], w[q][d], t[d]));
              }
              h_cg_add(cg, t, 2 * rb + hr, lane);
            }
          }
          if (row < M) {
            if constexpr (EPI == EPI_GABOR2D_BWD) {
              float* Gp = ep.o0 + (size_t)row * ep.ld0 + lc;
              *reinterpret_cast<f32x4*>(Gp) = g0;
              *reinterpret_cast<f32x4*>(Gp + 32) = g1;
              *reinterpret_cast<f32x4*>(Gp + 64) = g2;
              *reinterpret_cast<f32x4*>(Gp + 96) = g3;
            } else {
#pragma unroll
              for (int q = 0; q < 4; ++q)
                if (!(f0 + q < ep.kvalid)) { g0[q] = 0.f; g2[q] = 0.f; }
              if (ep.cr_partial) {
                // first-layer gradient sums (both Linears of the layer) instead of a stored g_(u | p) and two passes
#pragma unroll
                for (int q = 0; q < 4; ++q) {
#pragma unroll
                  for (int d = 0; d < 4; ++d) {
                    cru[q][d] = __builtin_fmaf(g0[q], xs[hr][d], cru[q][d]);
                    crp2[q][d] = __builtin_fmaf(g2[q], xs[hr][d], crp2[q][d]);
                  }
                  cru[q][4] += g0[q];
                  crp2[q][4] += g2[q];
                }
              } else {
                float* Gp = ep.o0 + (size_t)row * (2 * ep.ldu);
                *reinterpret_cast<f32x4*>(Gp + f0) = g0;
                *reinterpret_cast<f32x4*>(Gp + ep.ldu + f0) = g2;
              }
            }
          }
        }
      }
      if constexpr (EPI == EPI_GABOR2D_BWD_FIRST) {
        if (ep.cr_partial) {                                       // 8 row lanes by shuffles; the 4 waves through LDS below
          float* red = reinterpret_cast<float*>(lds);              // [2 sets][4 waves][64 features][5]
#pragma unroll
          for (int q = 0; q < 4; ++q)
#pragma unroll
            for (int d = 0; d < 5; ++d) {
              float a = cru[q][d], b = crp2[q][d];
              a += __shfl_xor(a, 1); a += __shfl_xor(a, 2); a += __shfl_xor(a, 4);
              b += __shfl_xor(b, 1); b += __shfl_xor(b, 2); b += __shfl_xor(b, 4);
              if (rr == 0) {
                red[(wave * 64 + 32 * G + cq + q) * 5 + d] = a;
                red[4 * 64 * 5 + (wave * 64 + 32 * G + cq + q) * 5 + d] = b;
              }
            }
        }
      }
    }
    if constexpr (EPI == EPI_GABOR2D_BWD_FIRST) {
      if (ep.cr_partial) {
        __syncthreads();
        const float* red = reinterpret_cast<const float*>(lds);
        const int fbase = (n_w >> 6) << 5;                          // first feature of this 128-column tile
        for (int e = threadIdx.x; e < 2 * 64 * 5; e += 256) {
          const int set = e / (64 * 5), r = e - set * (64 * 5);
          const int f = r / 5, d = r - 5 * f;
          const float* rs = red + set * (4 * 64 * 5);
          const float v = (rs[r] + rs[64 * 5 + r]) + (rs[2 * 64 * 5 + r] + rs[3 * 64 * 5 + r]);
          if (fbase + f < ep.cr_C)
            ep.cr_partial[(size_t)set * ep.cr_set + ((size_t)rt * ep.cr_C + fbase + f) * 5 + d] = v;
        }
      }
      if constexpr (CG) h_cg_store<NRB>(cg, ep, M, m_w, n_w, lane);
    }
  } else {
    // complex epilogues: 64-column groups (re | im of 32 features) = blocks 4 G, 4 G + 1 (re) and 4 G + 2, 4 G + 3 (im)
    const float w0 = ep.omega, w0l2e = ep.omega * 1.44269502f, ns2l2e = -(ep.scale * ep.scale) * 1.44269502f;
    const float m2s2 = -2.f * ep.scale * ep.scale;
    float cg[4] = {0.f, 0.f, 0.f, 0.f};                           // BWD_FIRST with cg_partial: row sums of g_u W0
#pragma unroll
    for (int G = 0; G < 2; ++G) {
      if (n_w + 64 * G >= Nc) continue;
      const int c0 = n_w + 64 * G + cq;                           // this lane's first re column; im = + 32
      const int f0 = ((c0 >> 6) << 5) + (c0 & 31);                // ... = features f0 .. f0 + 3
      f32x4 b_re = {0.f, 0.f, 0.f, 0.f}, b_im = b_re;
      float w[4][4], bb[4];
      float crs[4][5];                                            // BWD_FIRST with cr_partial: sums of g_u [x | 1]
#pragma unroll
      for (int q = 0; q < 4; ++q)
#pragma unroll
        for (int d = 0; d < 5; ++d) crs[q][d] = 0.f;
      if constexpr (EPI == EPI_GABOR_FWD) {
        b_re = *reinterpret_cast<const f32x4*>(ep.bias + c0);
        b_im = *reinterpret_cast<const f32x4*>(ep.bias + c0 + 32);
      }
      if constexpr (EPI == EPI_GABOR_BWD_FIRST) {
#pragma unroll
        for (int q = 0; q < 4; ++q) {
          const bool valid = f0 + q < ep.kvalid;
          bb[q] = valid ? ep.b0[f0 + q] : 0.f;
#pragma unroll
          for (int d = 0; d < 4; ++d) w[q][d] = (valid && d < ep.D) ? ep.W0[(f0 + q) * ep.D + d] : 0.f;
        }
      }
#pragma unroll
      for (int rb = 0; rb < NRB; ++rb) {
        f32x4 are[2], aim[2];                                     // [0]: rows 0-7 of the block, [1]: rows 8-15
        h_pair_rows(acc[rb][4 * G], acc[rb][4 * G + 1], are[0], are[1]);
        h_pair_rows(acc[rb][4 * G + 2], acc[rb][4 * G + 3], aim[0], aim[1]);
        if constexpr (EPI == EPI_GABOR_FWD) {
#pragma unroll
          for (int hr = 0; hr < 2; ++hr) {
            const int row = m_w + 16 * rb + 8 * hr + rr;
            f32x4 u, v;
#pragma unroll
            for (int q = 0; q < 4; ++q) {
              u[q] = are[hr][q] + b_re[q];
              v[q] = aim[hr][q] + b_im[q];
            }
            if (ep.o0 && row < M) {
              float* Lp = ep.o0 + (size_t)row * ep.ld0 + c0;
              *reinterpret_cast<f32x4*>(Lp) = u;
              *reinterpret_cast<f32x4*>(Lp + 32) = v;
            }
            // o1 = null: the last hidden layer of a fused training step -- the final stage recomputes out from lin
            if (ep.o1) {
              f32x4 o_re, o_im;
#pragma unroll
              for (int q = 0; q < 4; ++q) {
                float a, b;
                gabor_fwd_lean(u[q], v[q], w0, w0l2e, ns2l2e, a, b);
                const bool valid = f0 + q < ep.kvalid;             // pad features are written as 0
                o_re[q] = valid ? a : 0.f;
                o_im[q] = valid ? b : 0.f;
              }
              // (null: out_l is stored pre-split with a scale fixed on the host -- nobody reads its maximum)
              if (X2 && ep.amax_out) { h_amax4(amx, o_re); h_amax4(amx, o_im); }
              if (row < M) {
                float* Op = ep.o1 + (size_t)row * ep.ld1 + c0;
                wire_store_out4(Op, o_re, X2 ? ep.o1_split : 0.f);
                wire_store_out4(Op + 32, o_im, X2 ? ep.o1_split : 0.f);
              }
            }
          }
        } else if constexpr (EPI == EPI_GABOR_BWD) {
          const bool recompute = ep.recompute_out != 0;
          f32x4 lu[2], lv[2], pr[2], pi[2];
#pragma unroll
          for (int hr = 0; hr < 2; ++hr) {                          // all 8 loads of the row block first
            int row = m_w + 16 * rb + 8 * hr + rr;
            row = row < M ? row : M - 1;
            const float* Lp = ep.i0 + (size_t)row * ep.ld0 + c0;
            const float* Op = ep.i1 + (size_t)row * ep.ld1 + c0;
            lu[hr] = *reinterpret_cast<const f32x4*>(Lp);
            lv[hr] = *reinterpret_cast<const f32x4*>(Lp + 32);
            if (!recompute) {
              pr[hr] = *reinterpret_cast<const f32x4*>(Op);
              pi[hr] = *reinterpret_cast<const f32x4*>(Op + 32);
            }
          }
          if (recompute) {
            // out = act(lin) again instead of 8 more bytes per element from HBM: the same lean form as the forward
            // epilogue above, so the value equals the stored one bit for bit when that epilogue produced it
#pragma unroll
            for (int hr = 0; hr < 2; ++hr)
#pragma unroll
              for (int q = 0; q < 4; ++q) {
                float a, b;
                gabor_fwd_lean(lu[hr][q], lv[hr][q], w0, w0l2e, ns2l2e, a, b);
                const bool valid = f0 + q < ep.kvalid;
                pr[hr][q] = valid ? a : 0.f;
                pi[hr][q] = valid ? b : 0.f;
              }
          }
#pragma unroll
          for (int hr = 0; hr < 2; ++hr) {
            const int row = m_w + 16 * rb + 8 * hr + rr;
            f32x4 gl_re, gl_im;
#pragma unroll
            for (int q = 0; q < 4; ++q) {
              const float gr = are[hr][q], gi = aim[hr][q];
              const float c_r = __builtin_fmaf(pr[hr][q], gr, pi[hr][q] * gi);
              const float c_i = __builtin_fmaf(pr[hr][q], gi, -(pi[hr][q] * gr));
              const float tt = m2s2 * c_r;
              gl_re[q] = __builtin_fmaf(tt, lu[hr][q], w0 * c_i);
              gl_im[q] = __builtin_fmaf(tt, lv[hr][q], -(w0 * c_r));
            }
            if constexpr (X2) { h_amax4(amx, gl_re); h_amax4(amx, gl_im); }
            if (row < M) {
              float* Gp = ep.o0 + (size_t)row * ep.ld0 + c0;
              *reinterpret_cast<f32x4*>(Gp) = gl_re;
              *reinterpret_cast<f32x4*>(Gp + 32) = gl_im;
            }
          }
        } else {   // EPI_GABOR_BWD_FIRST: u recomputed from the coordinates (D <= 4); g_u [M][ldu] real
#pragma unroll
          for (int hr = 0; hr < 2; ++hr) {
            const int row = m_w + 16 * rb + 8 * hr + rr;
            float t[4] = {0.f, 0.f, 0.f, 0.f};                    // cg_partial: g_u W0 over this lane's 4 features
            if (row < M) {
              float x[4] = {0.f, 0.f, 0.f, 0.f};
              for (int d = 0; d < ep.D; ++d) x[d] = ep.coords[(size_t)row * ep.D + d];
              // out_0: read back, or (recompute_out) evaluated again from u with first_fwd_kernel's own form -- same
              // fmaf chain for u, same gabor_fwd_real: the same bits, 8 bytes per element less
              f32x4 pr = {0.f, 0.f, 0.f, 0.f}, pi = pr;
              if (!ep.recompute_out) {
                const float* Op = ep.i1 + (size_t)row * ep.ld1 + c0;
                pr = *reinterpret_cast<const f32x4*>(Op);
                pi = *reinterpret_cast<const f32x4*>(Op + 32);
              }
              f32x4 gu;
#pragma unroll
              for (int q = 0; q < 4; ++q) {
                float u = bb[q];
#pragma unroll
                for (int d = 0; d < 4; ++d) u = __builtin_fmaf(x[d], w[q][d], u);
                if (ep.recompute_out) {
                  float a, b;
                  gabor_fwd_real(u, w0, ep.scale, a, b);
                  pr[q] = a; pi[q] = b;
                }
                const float v = gabor_bwd_real(are[hr][q], aim[hr][q], u, pr[q], pi[q], w0, m2s2);
                gu[q] = f0 + q < ep.kvalid ? v : 0.f;
              }
              if constexpr (CG) {                                 // (w is 0 for pad features and d >= D)
#pragma unroll
                for (int q = 0; q < 4; ++q)
#pragma unroll
                  for (int d = 0; d < 4; ++d) t[d] = __builtin_fmaf(gu[q], w[q][d], t[d]);
              }
              if (ep.cr_partial) {
                // first-layer gradient sums of this lane's rows: g_u [x | 1] (what colreduce_kernel would form from
                // the stored g_u -- which is then never written)
#pragma unroll
                for (int q = 0; q < 4; ++q) {
#pragma unroll
                  for (int d = 0; d < 4; ++d) crs[q][d] = __builtin_fmaf(gu[q], x[d], crs[q][d]);
                  crs[q][4] += gu[q];
                }
              } else {
                *reinterpret_cast<f32x4*>(ep.o0 + (size_t)row * ep.ldu + f0) = gu;
              }
            }
            if constexpr (CG) h_cg_add(cg, t, 2 * rb + hr, lane);
          }
        }
      }
      if constexpr (EPI == EPI_GABOR_BWD_FIRST) {
        if (ep.cr_partial) {
          // sum over the 8 row lanes of each 16-lane row (lanes differing in bits 0-2), then over the 4 waves through LDS
          // (the main loop is over: every wave has passed its last barrier, the stage buffers are free)
#pragma unroll
          for (int q = 0; q < 4; ++q)
#pragma unroll
            for (int d = 0; d < 5; ++d) {
              float v = crs[q][d];
              v += __shfl_xor(v, 1); v += __shfl_xor(v, 2); v += __shfl_xor(v, 4);
              crs[q][d] = v;
            }
          float* red = reinterpret_cast<float*>(lds);            // [4 waves][64 features][5]
          const int fl = 32 * G + cq;                             // feature inside the tile's 64: 32 G + 16 ch + 4 g (+ q)
          if (rr == 0) {
#pragma unroll
            for (int q = 0; q < 4; ++q)
#pragma unroll
              for (int d = 0; d < 5; ++d) red[(wave * 64 + fl + q) * 5 + d] = crs[q][d];
          }
#pragma unroll
          for (int q = 0; q < 4; ++q)
#pragma unroll
            for (int d = 0; d < 5; ++d) crs[q][d] = 0.f;
        }
      }
    }
    if constexpr (EPI == EPI_GABOR_BWD_FIRST) {
      if (ep.cr_partial) {
        __syncthreads();
        const float* red = reinterpret_cast<const float*>(lds);
        const int fbase = (n_w >> 6) << 5;                        // first complex feature of this 128-column tile
        for (int e = threadIdx.x; e < 64 * 5; e += 256) {
          const int f = e / 5, d = e - 5 * f;
          const float v = (red[e] + red[64 * 5 + e]) + (red[2 * 64 * 5 + e] + red[3 * 64 * 5 + e]);
          if (fbase + f < ep.cr_C) ep.cr_partial[((size_t)rt * ep.cr_C + fbase + f) * 5 + d] = v;
        }
      }
      if constexpr (CG) h_cg_store<NRB>(cg, ep, M, m_w, n_w, lane);
    }
  }
  if constexpr (X2) {
    if (ep.amax_out) wire_amax_publish(ep.amax_out, amx, lane);
  }
}
