// wire_final.hip -- the final linear (O <= WIRE_MAXO outputs): forward, backward fused with the last hidden activation
// gradient, and the fused final stage of a training step (forward + MSE + backward in one pass over out_L / lin_L).
// The backward forms write per-block partials of g_Wf / g_bf that launch_final_reduce (wire_reduce.hip) adds up.
#include "wire_dev.h"
#include "wire_point.h"

// ===========================================================================
// final linear forward: one wave per row, wf staged in LDS, butterfly reduce.
// ===========================================================================
__global__ __launch_bounds__(256) void final_fwd_kernel(const float* __restrict__ z, long long n,
                                                        int P, int O, const float* __restrict__ wf,
                                                        const float* __restrict__ bfr,
                                                        float* __restrict__ y) {
  extern __shared__ __attribute__((aligned(16))) float swf[];   // [O][P]
  for (int i = threadIdx.x; i < O * P; i += blockDim.x) swf[i] = wf[i];
  __syncthreads();
  const int lane = threadIdx.x & 63;
  const int wave = threadIdx.x >> 6;
  const long long wstride = (long long)gridDim.x * 4;
  for (long long row = (long long)blockIdx.x * 4 + wave; row < n; row += wstride) {
    float acc[WIRE_MAXO];
#pragma unroll
    for (int o = 0; o < WIRE_MAXO; ++o) acc[o] = 0.f;
    const float* zr = z + row * P;
    for (int c = lane * 4; c < P; c += 256) {
      const f32x4 zv = *reinterpret_cast<const f32x4*>(zr + c);
#pragma unroll
      for (int o = 0; o < WIRE_MAXO; ++o)
        if (o < O) {
          const f32x4 wv = *reinterpret_cast<const f32x4*>(&swf[o * P + c]);
          acc[o] += zv[0] * wv[0] + zv[1] * wv[1] + zv[2] * wv[2] + zv[3] * wv[3];
        }
    }
#pragma unroll
    for (int o = 0; o < WIRE_MAXO; ++o)
      if (o < O) {
        float v = acc[o];
#pragma unroll
        for (int sft = 32; sft >= 1; sft >>= 1) v += __shfl_xor(v, sft);
        if (lane == o) y[row * O + o] = v + bfr[o];
      }
  }
}

hipError_t launch_final_fwd(hipStream_t s, const float* z, int64_t n, int P, int O,
                            const float* wf, const float* bfr, float* y) {
  if (n <= 0) return hipSuccess;
  if (O > WIRE_MAXO || (P & 3) || (int64_t)O * P > WIRE_FINAL_MAX_OP) return hipErrorInvalidValue;
  unsigned grid = cdiv(n, 4);
  if (grid > 4096) grid = 4096;
  hipLaunchKernelGGL(final_fwd_kernel, dim3(grid), dim3(256), (size_t)O * P * sizeof(float), s, z,
                     (long long)n, P, O, wf, bfr, y);
  return hipGetLastError();
}

// ===========================================================================
// final linear backward + last hidden activation gradient.
// ===========================================================================
int final_bwd_blocks(int64_t n) { return (int)((n + WIRE_FB_ROWS - 1) / WIRE_FB_ROWS); }

template <int KIND, bool RAW>
__global__ __launch_bounds__(256) void final_bwd_kernel(
    const float* __restrict__ g_y, long long n, int O, const float* __restrict__ wf,
    const float* __restrict__ lin, const float* __restrict__ out, int K, int P, float omega,
    float scale, float* __restrict__ g_lin, float* __restrict__ part_w,
    float* __restrict__ part_b, unsigned* __restrict__ amax_g) {
  constexpr bool cplx = (KIND == NK_WIRE || KIND == NK_WIRE2D);
  __shared__ float sgy[WIRE_FB_ROWS * WIRE_MAXO];
  float amx = 0.f;                                        // max |g_lin| for the 2 x fp16 split GEMMs that read it
  const long long r0 = (long long)blockIdx.x * WIRE_FB_ROWS;
  long long r1 = r0 + WIRE_FB_ROWS;
  if (r1 > n) r1 = n;
  const int nr = (int)(r1 - r0);
  for (int i = threadIdx.x; i < nr * O; i += blockDim.x) sgy[i] = g_y[r0 * O + i];
  __syncthreads();

  const int nfeat = cplx ? (P >> 1) : P;
  const int f = blockIdx.y * blockDim.x + threadIdx.x;
  if (f < nfeat) {
    const int c0 = cplx ? blk_col(f, 0) : f;
    float w0[WIRE_MAXO], w1[WIRE_MAXO], a0[WIRE_MAXO], a1[WIRE_MAXO];
#pragma unroll
    for (int o = 0; o < WIRE_MAXO; ++o) {
      w0[o] = 0.f; w1[o] = 0.f; a0[o] = 0.f; a1[o] = 0.f;
      if (o < O) {
        w0[o] = wf[(size_t)o * P + c0];
        if (cplx) w1[o] = wf[(size_t)o * P + c0 + 32];
      }
    }
    const float m2s2 = -2.f * scale * scale;
    const int Pl = (KIND == NK_WIRE2D) ? 2 * P : P;
    const int lc = (KIND == NK_WIRE2D) ? (((f >> 5) << 7) + (f & 31)) : c0;
    // rows in batches of 8: every load of a batch is issued before its first use (a per-row load -> use -> store
    // chain left this kernel at 2 TB/s; profiles/r02_siren_kernel_stats.csv)
    constexpr int RB = 8;
    for (int rb = 0; rb < nr; rb += RB) {
      float pr[RB], pi[RB], l0[RB], l1[RB], l2[RB], l3[RB];
#pragma unroll
      for (int q = 0; q < RB; ++q) {
        const int r = rb + q < nr ? rb + q : nr - 1;       // clamped: tail rows re-read the last one
        const long long row = r0 + r;
        pr[q] = out[row * P + c0];
        pi[q] = cplx ? out[row * P + c0 + 32] : 0.f;
        l0[q] = l1[q] = l2[q] = l3[q] = 0.f;
        if (!RAW) {
          if (KIND == NK_WIRE2D) {
            const float* L = lin + row * Pl + lc;
            l0[q] = L[0]; l1[q] = L[32]; l2[q] = L[64]; l3[q] = L[96];
          } else if (KIND != NK_RELU) {             // relu: lin is not stored (lin > 0 <=> out > 0)
            l0[q] = lin[row * P + c0];
            if (KIND == NK_WIRE) l1[q] = lin[row * P + c0 + 32];
          }
        }
      }
#pragma unroll
      for (int q = 0; q < RB; ++q) {
        const int r = rb + q;
        if (r < nr) {
          const long long row = r0 + r;
          float gr = 0.f, gi = 0.f;
#pragma unroll
          for (int o = 0; o < WIRE_MAXO; ++o)
            if (o < O) {
              const float g = sgy[r * O + o];
              gr = __builtin_fmaf(g, w0[o], gr);
              if (cplx) gi = __builtin_fmaf(g, w1[o], gi);
              a0[o] = __builtin_fmaf(g, pr[q], a0[o]);
              if (cplx) a1[o] = __builtin_fmaf(g, pi[q], a1[o]);
            }
          if (RAW) {
            g_lin[row * P + c0] = gr;
            if (cplx) g_lin[row * P + c0 + 32] = gi;
          } else if (KIND == NK_WIRE) {
            float gl_re, gl_im;
            gabor_bwd(gr, gi, l0[q], l1[q], pr[q], pi[q], omega, m2s2, gl_re, gl_im);
            g_lin[row * P + c0] = gl_re;
            g_lin[row * P + c0 + 32] = gl_im;
            amx = __builtin_fmaxf(amx, __builtin_fmaxf(__builtin_fabsf(gl_re), __builtin_fabsf(gl_im)));
          } else if (KIND == NK_WIRE2D) {
            const float c_r = __builtin_fmaf(pr[q], gr, pi[q] * gi);
            const float c_i = __builtin_fmaf(pr[q], gi, -(pi[q] * gr));
            const float t = m2s2 * c_r;
            float* Gp = g_lin + row * Pl + lc;
            const float g0 = __builtin_fmaf(t, l0[q], omega * c_i), g1 = __builtin_fmaf(t, l1[q], -(omega * c_r));
            const float g2 = t * l2[q], g3 = t * l3[q];
            Gp[0] = g0; Gp[32] = g1; Gp[64] = g2; Gp[96] = g3;
            amx = __builtin_fmaxf(amx, __builtin_fmaxf(__builtin_fmaxf(__builtin_fabsf(g0), __builtin_fabsf(g1)),
                                                       __builtin_fmaxf(__builtin_fabsf(g2), __builtin_fabsf(g3))));
          } else {
            constexpr int ACT = nk_real_act(KIND);
            const float gl = real_act_bwd<ACT>(gr, l0[q], pr[q], omega, scale);
            g_lin[row * P + c0] = gl;
            amx = __builtin_fmaxf(amx, __builtin_fabsf(gl));
          }
        }
      }
    }
    float* pw = part_w + (size_t)blockIdx.x * O * P;
#pragma unroll
    for (int o = 0; o < WIRE_MAXO; ++o)
      if (o < O) {
        pw[(size_t)o * P + c0] = a0[o];
        if (cplx) pw[(size_t)o * P + c0 + 32] = a1[o];
      }
  }
  // bias partial: thread o < O of the first feature block sums g_y[:, o]
  if (blockIdx.y == 0 && threadIdx.x < O) {
    float sacc = 0.f;
    for (int r = 0; r < nr; ++r) sacc += sgy[r * O + threadIdx.x];
    part_b[(size_t)blockIdx.x * O + threadIdx.x] = sacc;
  }
  if (amax_g) wire_amax_publish(amax_g, amx, threadIdx.x & 63);
}

hipError_t launch_final_bwd(hipStream_t s, int kind, int raw, const float* g_y, int64_t n, int O,
                            const float* wf, const float* lin, const float* out, int K, int P,
                            float omega, float scale, float* g_lin, float* part_w,
                            float* part_b, unsigned* amax_g) {
  if (n <= 0) return hipSuccess;
  if (O > WIRE_MAXO) return hipErrorInvalidValue;
  const bool cplx = kind_is_cplx(kind);
  const int nfeat = cplx ? P / 2 : P;
  dim3 grid((unsigned)final_bwd_blocks(n), cdiv(nfeat, 256));
#define FB_LAUNCH(KK, RR)                                                                        \
  hipLaunchKernelGGL((final_bwd_kernel<KK, RR>), grid, dim3(256), 0, s, g_y, (long long)n, O, wf, \
                     lin, out, K, P, omega, scale, g_lin, part_w, part_b, amax_g)
  if (raw) {
    if (cplx) FB_LAUNCH(NK_WIRE, true); else FB_LAUNCH(NK_RELU, true);
    return hipGetLastError();
  }
  return with_kind(kind, [&](auto k) -> hipError_t {
    FB_LAUNCH(decltype(k)::value, false);
    return hipGetLastError();
  });
#undef FB_LAUNCH
}

// ---------------------------------------------------------------------------
// fused final stage (training path, wire): one wave per row.
// lane l owns features f = 32 g + 4 (l & 7) + j, j = 0..3, of group g = (l >> 3) + 8 pass: its row
// slice is two float4 (re, im).  y_o is a butterfly over the wave; everything after it (loss term,
// dL/dy, g_out, Gabor gradient, g_Wf partials) stays in registers.
// ---------------------------------------------------------------------------
#define FF_MAXO 4
#define FF_MAXPASS 2      // P <= 1024 floats per row
#define FF_MAXROWS 512    // rows of one block (WIRE_FB_ROWS <= rows <= FF_MAXROWS, chosen by the launcher)
// (the kernel keeps 4 O P floats of W_f / partial sums in dynamic LDS: it must fit the 64 KB a launch gets
// without an opt-in -- O = 4 with P = 1024 does not, and runs the unfused sequence instead)
// dynamic LDS of the fused final stage: [4 waves][O][P] g_wf partials, [4][FF_MAXO + 1] bias / loss partials, then the
// block's gathered targets [FF_MAXROWS][FF_MAXO] and source indices [FF_MAXROWS] (int64)
static size_t final_fused_shm(int P, int O) {
  return ((size_t)4 * O * P + 4 * (FF_MAXO + 1) + (size_t)FF_MAXROWS * FF_MAXO) * sizeof(float) + (size_t)FF_MAXROWS * 8;
}
bool final_fused_supported(int P, int O) {
  return (P % 64) == 0 && P <= 512 * FF_MAXPASS && O <= FF_MAXO && final_fused_shm(P, O) <= 65536;
}

// KIND: the activation whose gradient is fused (wire / wire2d: complex pairs (re | im) 32 columns apart; siren / gauss /
//   relu: the two 4-column chunks of a lane are just 8 real features).  wire2d: lin is the 2P-wide (lin | sy) row.
// RECOMP (wire only): out_L is not read -- it is evaluated again from lin_L with the lean forward form (bit-identical
//   to what the 16 x 16 x 32 forward epilogue would have stored; wire_api.hip selects this only when that kernel ran
//   layer L, and then does not let it write out_L at all): 1 GB instead of 1.5 GB of HBM traffic for this pass.
// OT >= O (1..FF_MAXO): the weight / partial-sum registers are sized for the actual number of outputs
// RPW: rows per wave slot -- 2 when a row has at most 256 floats (siren / gauss / relu and wire2d at 256 features):
// lanes 0-31 take one row, lanes 32-63 the next, instead of leaving half the wave idle
WIRE_DEVINL void ff_amax4(float& m, const f32x4& v) {
  m = __builtin_fmaxf(m, __builtin_fmaxf(__builtin_fmaxf(__builtin_fabsf(v[0]), __builtin_fabsf(v[1])),
                                         __builtin_fmaxf(__builtin_fabsf(v[2]), __builtin_fabsf(v[3]))));
}
template <int NPASS, int KIND, bool RECOMP, int OT, int RPW>
__global__ __launch_bounds__(256) void final_fused_kernel(
    const float* __restrict__ out, const float* __restrict__ lin, long long n, int P, int O, int kvalid,
    const float* __restrict__ wf, const float* __restrict__ bfr, const float* __restrict__ target,
    const int64_t* __restrict__ idx, long long first, float gscale, float omega, float scale,
    float* __restrict__ y, float* __restrict__ rec, float* __restrict__ g_lin, float* __restrict__ part_w,
    float* __restrict__ part_b, float* __restrict__ loss_partial, int rows_pb, unsigned* __restrict__ amax_g) {
  static_assert(!RECOMP || KIND != NK_RELU, "relu keeps out and has no lin to recompute it from");
  float amx = 0.f;                                     // max |g_lin| for the 2 x fp16 split GEMMs that read it
  static_assert(RPW == 1 || (RPW == 2 && NPASS == 1), "two rows per wave slot: one pass of at most 256 columns");
  constexpr int RL = 64 / RPW;                         // lanes of one row
  constexpr bool HAS_LIN = (KIND != NK_RELU);          // relu: lin is never stored (lin > 0 <=> out > 0)
  constexpr int NL = (KIND == NK_WIRE2D) ? 4 : 2;      // 4-column chunks of lin per lane and pass
  extern __shared__ float sm[];                        // [4 waves][O][P] g_wf partials + [4][O+1]
  const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
  const int sub = lane / RL, lr_ = lane & (RL - 1);    // row of the slot, lane inside the row
  const int ngrp = P >> 6;
  const int Pl = (KIND == NK_WIRE2D) ? 2 * P : P;      // row stride of lin / g_lin
  const long long r0 = (long long)blockIdx.x * rows_pb;
  long long r1 = r0 + rows_pb;
  if (r1 > n) r1 = n;
  const float m2s2 = -2.f * scale * scale;

  // this lane's columns and weights
  int col[NPASS], lcol[NPASS];
  bool live[NPASS];
  f32x4 wre[NPASS][OT], wim[NPASS][OT];
  f32x4 are[NPASS][OT], aim[NPASS][OT];
#pragma unroll
  for (int ps = 0; ps < NPASS; ++ps) {
    const int g = (lr_ >> 3) + 8 * ps;
    live[ps] = g < ngrp;
    col[ps] = (g << 6) + 4 * (lr_ & 7);
    lcol[ps] = (KIND == NK_WIRE2D) ? (g << 7) + 4 * (lr_ & 7) : col[ps];
#pragma unroll
    for (int o = 0; o < OT; ++o) {
      const f32x4 z4 = {0.f, 0.f, 0.f, 0.f};
      wre[ps][o] = z4; wim[ps][o] = z4; are[ps][o] = z4; aim[ps][o] = z4;
      if (live[ps] && o < O) {
        wre[ps][o] = *reinterpret_cast<const f32x4*>(wf + (size_t)o * P + col[ps]);
        wim[ps][o] = *reinterpret_cast<const f32x4*>(wf + (size_t)o * P + col[ps] + 32);
      }
    }
  }
  float bsum[OT];
#pragma unroll
  for (int o = 0; o < OT; ++o) bsum[o] = 0.f;
  float lsum = 0.f;

  // the block's source indices and targets, gathered once by all 256 threads: inside the row loop the chain
  // idx[row] -> target[src] would be two dependent global loads per row and wave (it bounded the pass)
  float* s_tg = sm + (size_t)4 * O * P + 4 * (FF_MAXO + 1);                       // [FF_MAXROWS][FF_MAXO]
  long long* s_src = reinterpret_cast<long long*>(s_tg + FF_MAXROWS * FF_MAXO);   // [FF_MAXROWS]
  for (int t = threadIdx.x; t < rows_pb; t += 256) {
    const long long grow = r0 + t;
    if (grow < r1) {
      const long long src = idx ? idx[grow] : first + grow;
      s_src[t] = src;
#pragma unroll
      for (int o = 0; o < OT; ++o)
        if (o < O) s_tg[t * FF_MAXO + o] = target[src * O + o];
    }
  }
  __syncthreads();

  // software pipeline over this wave's rows: the loads of the next PF rows of this wave (r + 4, r + 8, ...) are in
  // flight while row r goes through its butterfly / gradient chain -- the pass is bound by memory latency, and one
  // row is only 4 KB (2 KB when out is recomputed) per wave in flight
  constexpr int PF = RECOMP ? 3 : 2;
  f32x4 nzr[PF][NPASS], nzi[PF][NPASS], nl[PF][NPASS][NL];
  auto load_row = [&](const int slot, long long row) {
    row += sub;                                          // this lane's row of the slot
#pragma unroll
    for (int ps = 0; ps < NPASS; ++ps) {
      const f32x4 z4 = {0.f, 0.f, 0.f, 0.f};
      nzr[slot][ps] = z4; nzi[slot][ps] = z4;
#pragma unroll
      for (int c = 0; c < NL; ++c) nl[slot][ps][c] = z4;
      if (live[ps] && row < r1) {
        if (!RECOMP) {
          const size_t o_ = (size_t)row * P + col[ps];
          nzr[slot][ps] = *reinterpret_cast<const f32x4*>(out + o_);
          nzi[slot][ps] = *reinterpret_cast<const f32x4*>(out + o_ + 32);
        }
        if (HAS_LIN) {
          const float* Lp = lin + (size_t)row * Pl + lcol[ps];
#pragma unroll
          for (int c = 0; c < NL; ++c) nl[slot][ps][c] = *reinterpret_cast<const f32x4*>(Lp + 32 * c);
        }
      }
    }
  };
  auto process = [&](const long long row_slot, f32x4 (&zr)[NPASS], f32x4 (&zi)[NPASS],
                     const f32x4 (&ll)[NPASS][NL]) {
    const long long row = row_slot + sub;                // this lane's row; past the end: contributes nothing
    const bool rl = row < r1;
    if (RECOMP && (KIND == NK_WIRE || KIND == NK_WIRE2D)) {
      const float w0l2e = omega * 1.44269502f, ns2l2e = -(scale * scale) * 1.44269502f;
#pragma unroll
      for (int ps = 0; ps < NPASS; ++ps) {
        const int f0 = ((col[ps] >> 6) << 5) + (col[ps] & 31);     // features f0 .. f0 + 3 of this lane
#pragma unroll
        for (int j = 0; j < 4; ++j) {
          float a_, b_;
          if (KIND == NK_WIRE2D)
            gabor2d_fwd_lean(ll[ps][0][j], ll[ps][1][j], ll[ps][NL - 2][j], ll[ps][NL - 1][j], omega, scale, a_, b_);
          else
            gabor_fwd_lean(ll[ps][0][j], ll[ps][1][j], omega, w0l2e, ns2l2e, a_, b_);
          const bool valid = live[ps] && f0 + j < kvalid;          // pad features are 0
          zr[ps][j] = valid ? a_ : 0.f;
          zi[ps][j] = valid ? b_ : 0.f;
        }
      }
    } else if (RECOMP) {                                           // siren / gauss: 8 real features per lane and pass
      constexpr int ACT = nk_real_act(KIND);
#pragma unroll
      for (int ps = 0; ps < NPASS; ++ps)
#pragma unroll
        for (int j = 0; j < 4; ++j) {
          const float a_ = real_act_fwd_lean<ACT>(ll[ps][0][j], omega, scale);
          const float b_ = real_act_fwd_lean<ACT>(ll[ps][1][j], omega, scale);
          zr[ps][j] = (live[ps] && col[ps] + j < kvalid) ? a_ : 0.f;
          zi[ps][j] = (live[ps] && col[ps] + 32 + j < kvalid) ? b_ : 0.f;
        }
    }
    float yo[OT];
#pragma unroll
    for (int o = 0; o < OT; ++o) {
      float acc = 0.f;
#pragma unroll
      for (int ps = 0; ps < NPASS; ++ps)
#pragma unroll
        for (int j = 0; j < 4; ++j)
          acc = __builtin_fmaf(zr[ps][j], wre[ps][o][j], __builtin_fmaf(zi[ps][j], wim[ps][o][j], acc));
      yo[o] = acc;
    }
#pragma unroll
    for (int o = 0; o < OT; ++o)
      if (o < O) {
#pragma unroll
        for (int sft = RL / 2; sft >= 1; sft >>= 1) yo[o] += __shfl_xor(yo[o], sft);
      }
    const int lrow = rl ? (int)(row - r0) : 0;
    const long long src = s_src[lrow];
    float gy[OT];
#pragma unroll
    for (int o = 0; o < OT; ++o) {
      gy[o] = 0.f;
      if (o < O) {
        const float yy = yo[o] + bfr[o];
        const float dlt = rl ? yy - s_tg[lrow * FF_MAXO + o] : 0.f;
        gy[o] = gscale * dlt;
        if (lr_ == o && rl) {
          y[row * O + o] = yy;
          if (rec) rec[src * O + o] = yy;
        }
        lsum = __builtin_fmaf(dlt, dlt, lsum);
        bsum[o] += gy[o];
      }
    }
#pragma unroll
    for (int ps = 0; ps < NPASS; ++ps) {
      if (!live[ps] || !rl) continue;
      f32x4 gr = {0.f, 0.f, 0.f, 0.f}, gi = {0.f, 0.f, 0.f, 0.f};
#pragma unroll
      for (int o = 0; o < OT; ++o)
        if (o < O) {
          gr += gy[o] * wre[ps][o];
          gi += gy[o] * wim[ps][o];
          are[ps][o] += gy[o] * zr[ps];
          aim[ps][o] += gy[o] * zi[ps];
        }
      float* Gp = g_lin + (size_t)row * Pl + lcol[ps];
      if (KIND == NK_WIRE) {
        f32x4 glr, gli;
#pragma unroll
        for (int j = 0; j < 4; ++j) {
          float a_, b_;
          gabor_bwd(gr[j], gi[j], ll[ps][0][j], ll[ps][1][j], zr[ps][j], zi[ps][j], omega, m2s2, a_, b_);
          glr[j] = a_; gli[j] = b_;
        }
        *reinterpret_cast<f32x4*>(Gp) = glr;
        *reinterpret_cast<f32x4*>(Gp + 32) = gli;
        ff_amax4(amx, glr); ff_amax4(amx, gli);
      } else if (KIND == NK_WIRE2D) {
        // c = conj(out) g;  g_lin = -2 s^2 Re(c) lin - j w0 c;  g_sy = -2 s^2 Re(c) sy   (modules/wire2d.py:56-67)
        f32x4 g0, g1, g2, g3;
#pragma unroll
        for (int j = 0; j < 4; ++j) {
          const float c_r = __builtin_fmaf(zr[ps][j], gr[j], zi[ps][j] * gi[j]);
          const float c_i = __builtin_fmaf(zr[ps][j], gi[j], -(zi[ps][j] * gr[j]));
          const float t = m2s2 * c_r;
          g0[j] = __builtin_fmaf(t, ll[ps][0][j], omega * c_i);
          g1[j] = __builtin_fmaf(t, ll[ps][1][j], -(omega * c_r));
          g2[j] = t * ll[ps][NL - 2][j];
          g3[j] = t * ll[ps][NL - 1][j];
        }
        *reinterpret_cast<f32x4*>(Gp) = g0;
        *reinterpret_cast<f32x4*>(Gp + 32) = g1;
        *reinterpret_cast<f32x4*>(Gp + 64) = g2;
        *reinterpret_cast<f32x4*>(Gp + 96) = g3;
        ff_amax4(amx, g0); ff_amax4(amx, g1); ff_amax4(amx, g2); ff_amax4(amx, g3);
      } else {
        // the same forms final_bwd_kernel uses (sin'= w0 cos, gauss' = -2 s^2 lin out, relu' = [out > 0])
        constexpr int ACT = nk_real_act(KIND);
        f32x4 glr, gli;
#pragma unroll
        for (int j = 0; j < 4; ++j) {
          glr[j] = real_act_bwd<ACT>(gr[j], ll[ps][0][j], zr[ps][j], omega, scale);
          gli[j] = real_act_bwd<ACT>(gi[j], ll[ps][1][j], zi[ps][j], omega, scale);
        }
        *reinterpret_cast<f32x4*>(Gp) = glr;
        *reinterpret_cast<f32x4*>(Gp + 32) = gli;
        ff_amax4(amx, glr); ff_amax4(amx, gli);
      }
    }
  };
#pragma unroll
  for (int d = 0; d < PF; ++d) load_row(d, r0 + (wave + 4 * d) * RPW);
  for (long long row = r0 + wave * RPW; row < r1; row += 4 * RPW * PF) {
#pragma unroll
    for (int d = 0; d < PF; ++d) {
      const long long rr_ = row + 4 * RPW * d;
      if (rr_ < r1) {                                   // wave-uniform
        f32x4 zr[NPASS], zi[NPASS], ll[NPASS][NL];
#pragma unroll
        for (int ps = 0; ps < NPASS; ++ps) {
          zr[ps] = nzr[d][ps]; zi[ps] = nzi[d][ps];
#pragma unroll
          for (int c = 0; c < NL; ++c) ll[ps][c] = nl[d][ps][c];
        }
        load_row(d, rr_ + 4 * RPW * PF);
        process(rr_, zr, zi, ll);
      }
    }
  }

  // ---- combine the 4 waves: g_wf partials [O][P], bias partial [O], loss
  float* swf = sm;                                   // [4][O][P]
  float* sb = sm + 4 * O * P;                        // [4][FF_MAXO + 1]
  if (RPW == 2) {                                    // the two half waves hold partial sums of the same columns
#pragma unroll
    for (int o = 0; o < OT; ++o) {
#pragma unroll
      for (int ps = 0; ps < NPASS; ++ps)
#pragma unroll
        for (int j = 0; j < 4; ++j) {
          are[ps][o][j] += __shfl_xor(are[ps][o][j], 32);
          aim[ps][o][j] += __shfl_xor(aim[ps][o][j], 32);
        }
      bsum[o] += __shfl_xor(bsum[o], 32);
    }
    lsum += __shfl_xor(lsum, 32);
  }
#pragma unroll
  for (int ps = 0; ps < NPASS; ++ps)
    if (live[ps] && sub == 0)
#pragma unroll
      for (int o = 0; o < OT; ++o)
        if (o < O) {
          *reinterpret_cast<f32x4*>(swf + ((size_t)wave * O + o) * P + col[ps]) = are[ps][o];
          *reinterpret_cast<f32x4*>(swf + ((size_t)wave * O + o) * P + col[ps] + 32) = aim[ps][o];
        }
  // lsum is identical in every lane only per row-term count; every lane added the same terms -> use lane 0
  if (lane == 0) {
#pragma unroll
    for (int o = 0; o < OT; ++o) sb[wave * (FF_MAXO + 1) + o] = bsum[o];
    sb[wave * (FF_MAXO + 1) + FF_MAXO] = lsum;
  }
  __syncthreads();
  float* pw = part_w + (size_t)blockIdx.x * O * P;
  for (int e = threadIdx.x; e < O * P; e += 256)
    pw[e] = (swf[e] + swf[O * P + e]) + (swf[2 * O * P + e] + swf[3 * O * P + e]);
  if (threadIdx.x < O)
    part_b[(size_t)blockIdx.x * O + threadIdx.x] =
        (sb[threadIdx.x] + sb[(FF_MAXO + 1) + threadIdx.x]) +
        (sb[2 * (FF_MAXO + 1) + threadIdx.x] + sb[3 * (FF_MAXO + 1) + threadIdx.x]);
  if (threadIdx.x == 0)
    loss_partial[blockIdx.x] = (sb[FF_MAXO] + sb[(FF_MAXO + 1) + FF_MAXO]) +
                               (sb[2 * (FF_MAXO + 1) + FF_MAXO] + sb[3 * (FF_MAXO + 1) + FF_MAXO]);
  if (amax_g) wire_amax_publish(amax_g, amx, lane);
}

// kind: NK_*.  out = nullptr (wire only): out_L is recomputed from lin_L (kvalid = number of valid complex
// features).  lin: [n][P] (wire2d: the 2P-wide (lin | sy) rows; relu: unused).  g_lin has the layout of lin.
hipError_t launch_final_fused(hipStream_t s, int kind, const float* out, const float* lin, int64_t n, int P, int O,
                              int kvalid, const float* wf, const float* bfr, const float* target, const int64_t* idx,
                              int64_t first, float weight, float omega, float scale, float* y, float* rec,
                              float* g_lin, float* part_w, float* part_b, float* loss_partial,
                              float* loss_out, unsigned* amax_g) {
  if (n <= 0) return hipSuccess;
  if (!final_fused_supported(P, O)) return hipErrorInvalidValue;
  if (!out && kind == NK_RELU) return hipErrorInvalidValue;
  // Rows per block: the kernel runs 3 blocks per CU (registers), i.e. 768 at a time; 1024 blocks of WIRE_FB_ROWS rows at
  // n = 262 144 would be one full round and a second one on a third of the chip.  So a block takes as many rows as
  // it needs for ONE round (342 -> 767 blocks), within the WIRE_FB_ROWS-block partial-sum layout of launch_final_reduce:
  // fewer blocks than final_bwd_blocks(n), the unused partial slots are zeroed.
  const int nbf = final_bwd_blocks(n);
  int rows_pb = WIRE_FB_ROWS;
  if (nbf > 768) {
    rows_pb = (int)((n + 767) / 768);
    rows_pb = (rows_pb + 7) & ~7;
    if (rows_pb > FF_MAXROWS) rows_pb = FF_MAXROWS;
  }
  const int nblk = (int)((n + rows_pb - 1) / rows_pb);
  if (nblk < nbf) {
    hipError_t e = hipMemsetAsync(part_w + (size_t)nblk * O * P, 0, (size_t)(nbf - nblk) * O * P * sizeof(float), s);
    if (e == hipSuccess) e = hipMemsetAsync(part_b + (size_t)nblk * O, 0, (size_t)(nbf - nblk) * O * sizeof(float), s);
    if (e != hipSuccess) return e;
  }
  const float inv = (float)(1.0 / ((double)n * (double)O));
  const size_t shm = final_fused_shm(P, O);
#define FF_LAUNCH(NP, RW, KD, RC, OT)                                                                        \
  hipLaunchKernelGGL((final_fused_kernel<NP, KD, RC, OT, RW>), dim3((unsigned)nblk), dim3(256), shm, s, out, \
                     lin, (long long)n, P, O, kvalid, wf, bfr, target, idx, (long long)first,                \
                     weight * 2.f * inv, omega, scale, y, rec, g_lin, part_w, part_b, loss_partial, rows_pb, amax_g)
#define FF_LAUNCH_O(NP, RW, KD, RC)                                                                          \
  switch (O) {                                                                                               \
    case 1: FF_LAUNCH(NP, RW, KD, RC, 1); break;                                                             \
    case 2: case 3: FF_LAUNCH(NP, RW, KD, RC, 3); break;                                                     \
    default: FF_LAUNCH(NP, RW, KD, RC, 4); break;                                                            \
  }
  // (relu: out_L cannot be formed again from a lin_L that is not stored -- refused above)
#define FF_LAUNCH_K(NP, RW)                                                                                  \
  if constexpr (KD == NK_RELU) { FF_LAUNCH_O(NP, RW, KD, false); }                                           \
  else if (out) { FF_LAUNCH_O(NP, RW, KD, false); } else { FF_LAUNCH_O(NP, RW, KD, true); }
  const hipError_t err = with_kind(kind, [&](auto k) -> hipError_t {
    constexpr int KD = decltype(k)::value;
    if (P <= 256) { FF_LAUNCH_K(1, 2) } else if (P <= 512) { FF_LAUNCH_K(1, 1) } else { FF_LAUNCH_K(2, 1) }
    return hipSuccess;
  });
  if (err != hipSuccess) return err;
#undef FF_LAUNCH_K
#undef FF_LAUNCH_O
#undef FF_LAUNCH
  // the loss partials are summed by the MSE final kernel (one block, wire_train.hip)
  return launch_mse_final(s, loss_partial, nblk, weight * inv, loss_out);
}
