// wire_api.hip -- the C ABI of libwire_hip.so (include/wire_hip.h): the error channel, the profiler, the pack and the
// launch sequences of the whole-net calls.  The plan and the size queries: wire_plan.hip; the hierarchical net:
// wire_hier_api.hip; the multiplicative filter network: wire_mfn_api.hip; the one-launch entry points: wire_misc_api.hip; the per-layer ones: wire_layer_api.hip.
// No device memory is allocated here; every launch goes on the caller's stream.
#include <cmath>
#include <cstdarg>
#include <cstdio>
#include <string>

#include "wire_plan.h"

// ---------------------------------------------------------------------------
// error plumbing
// ---------------------------------------------------------------------------
static thread_local std::string g_err;
int fail(int code, const char* fmt, ...) {
  char buf[512];
  va_list ap;
  va_start(ap, fmt);
  vsnprintf(buf, sizeof buf, fmt, ap);
  va_end(ap);
  g_err = buf;
  return code;
}
int wire_fail_(int code, const char* msg) { return fail(code, "%s", msg); }   // wire_layer_api.hip

extern "C" int wire_abi_version(void) { return WIRE_ABI_VERSION; }
extern "C" const char* wire_last_error(void) { return g_err.c_str(); }

// ---------------------------------------------------------------------------
// profiling hooks
// ---------------------------------------------------------------------------
std::mutex g_prof_mu;
std::atomic<bool> g_prof_on{false};
std::vector<ProfRec> g_prof_recs;
std::vector<std::pair<hipEvent_t, hipEvent_t>> g_prof_pool;

extern "C" int wire_prof_enable(int on) {
  std::lock_guard<std::mutex> lk(g_prof_mu);
  g_prof_on.store(on != 0);
  return WIRE_OK;
}
extern "C" int wire_prof_read(double* ms_total, int64_t* launches, double* flops_total) {
  std::lock_guard<std::mutex> lk(g_prof_mu);
  for (int i = 0; i < WIRE_PROF_CLASSES; ++i) { ms_total[i] = 0; launches[i] = 0; flops_total[i] = 0; }
  for (auto& r : g_prof_recs) {
    float ms = 0.f;
    if (hipEventSynchronize(r.b) == hipSuccess && hipEventElapsedTime(&ms, r.a, r.b) == hipSuccess) {
      ms_total[r.cls] += ms; launches[r.cls] += 1; flops_total[r.cls] += r.flops;
    }
    g_prof_pool.emplace_back(r.a, r.b);
  }
  g_prof_recs.clear();
  return WIRE_OK;
}

// ---------------------------------------------------------------------------
// tuning knobs (the table: wire_knobs.hip)
// ---------------------------------------------------------------------------
// family the flags select for a net kind (wire_layer_api.hip)
WireFamily wire_family_(int kind) {
  if (knob(K_SPLIT_BF16)) return FAM_X3;
  return (kind == WIRE_KIND_WIRE && knob(K_COMPLEX_3M)) ? FAM_3M : FAM_4M;
}
extern "C" int wire_tune_get(const char* key) {
  if (!key) return fail(WIRE_ERR_ARG, "null key");
  const int v = knob_get(key);
  return v >= 0 ? v : fail(WIRE_ERR_ARG, "unknown tuning key: %s", key);
}
extern "C" int wire_tune_set(const char* key, int value) {
  if (!key) return fail(WIRE_ERR_ARG, "null key");
  if (knob_set(key, value) == 0 || (g_glds_tune && g_glds_tune(key, value) == 0)) return WIRE_OK;
  return fail(WIRE_ERR_ARG, "unknown tuning key or bad value: %s=%d", key, value);
}

// C = A W_l^T (the forward of layer l) or, dg, A W_l (its data gradient) on family f, from f's image of layer l.  The
// 2 x fp16 kernels also take the maximum slots of A, of W_l and of the tensor the epilogue writes (null: none kept)
hipError_t layer_nt(hipStream_t s, const Plan& p, WireFamily f, const float* packed, int l, bool dg, int epi,
                    const float* A, int64_t n, GemmEpiParams ep, const unsigned* amax_a, const unsigned* amax_b,
                    unsigned* amax_out) {
  const int Pin = l == 0 ? p.Pin0 : p.P, Nc = dg ? Pin : p.Pl, Kd = dg ? p.Pl : Pin;
  switch (f) {
    case FAM_X2:
      ep.amax_a = amax_a; ep.amax_b = amax_b; ep.amax_out = amax_out;
      return launch_gemmx2h_nt(s, epi, A, Kd, packed + (dg ? p.off_dg_x2 : p.off_fwd_x2)[l], n, Nc, Kd, ep,
                               x2_waits(p.k_nt_bfirst, p.k_epi_early));
    case FAM_3M:
      return launch_gemm3m_nt(s, epi, A, Kd, packed + (dg ? p.off_dg_3m : p.off_fwd_3m)[l], Kd, n, Nc / 2, Kd / 2, ep);
    case FAM_X3: return launch_gemmx3_nt(s, epi, A, Kd, packed + (dg ? p.off_dg_x3 : p.off_fwd_x3)[l], n, Nc, Kd, ep);
    default: return launch_gemm_nt(s, epi, A, Kd, packed + (dg ? p.off_dg : p.off_fwd)[l], Kd, n, Nc, Kd, ep);
  }
}

// ---------------------------------------------------------------------------
// pack
// ---------------------------------------------------------------------------
// hidden layers share one shape: every family's image of up to PACK_MAXB layers per launch (3 - 4 launches per step
// instead of 4 per layer; this runs once per optimizer step and is all launch gaps).  hW[l], hb[l]: W, b of the plan's
// hidden layer l
int pack_hidden(hipStream_t s, const Plan& p, const void* const* params, float* packed, const std::vector<const float*>& hW,
                const std::vector<const float*>& hb) {
  for (int l0 = 1; l0 <= p.L; l0 += PACK_MAXB) {
    const int nb = (p.L - l0 + 1) < PACK_MAXB ? (p.L - l0 + 1) : PACK_MAXB;
    PackBatch pb{}, p3{};
    X3SplitBatch sf{}, sd{};
    for (int i = 0; i < nb; ++i) {
      const int l = l0 + i;
      pb.W[i] = hW[l];
      pb.b[i] = hb[l];
      pb.V[i] = p.per_layer == 4 ? (const float*)params[p.per_layer * l + 2] : nullptr;
      pb.c[i] = p.per_layer == 4 ? (const float*)params[p.per_layer * l + 3] : nullptr;
      pb.fwd[i] = packed + p.off_fwd[l]; pb.dg[i] = packed + p.off_dg[l]; pb.bias[i] = packed + p.off_bias[l];
      sf.src[i] = packed + p.off_fwd[l]; sf.dst[i] = packed + p.off_fwd_x3[l];
      sd.src[i] = packed + p.off_dg[l]; sd.dst[i] = packed + p.off_dg_x3[l];
      if (p.off_fwd_3m[l] >= 0) {
        p3.W[i] = pb.W[i]; p3.b[i] = pb.b[i];
        p3.fwd[i] = packed + p.off_fwd_3m[l]; p3.dg[i] = packed + p.off_dg_3m[l]; p3.bias[i] = packed + p.off_bias[l];
      }
    }
    HIPCHK(launch_pack_hidden_batch(s, p.kind, pb, nb, p.K, p.K, p.P, p.P, p.ws));   // (everything below reads these images)
    if (p.Pl == p.P) {                                   // forward and transposed images have one shape: one launch
      for (int i = 0; i < nb; ++i) { sf.src[nb + i] = sd.src[i]; sf.dst[nb + i] = sd.dst[i]; }
      HIPCHK(launch_x3_split_b_batch(s, sf, 2 * nb, p.P, p.Pl, p.P));
    } else {
      HIPCHK(launch_x3_split_b_batch(s, sf, nb, p.P, p.Pl, p.P));
      HIPCHK(launch_x3_split_b_batch(s, sd, nb, p.Pl, p.P, p.Pl));
    }
    if (p.off_fwd_3m[l0] >= 0)    // same bias image (blocked planar) as the hidden pack wrote
      HIPCHK(launch_pack3m_batch(s, p3, nb, p.K, p.K, p.Kp, p.Kp));
    {
      // 2 x fp16 images: max |weight| of each layer (the forward and the transposed image hold the same values), then
      // the scaled split of both images
      X2AmaxBatch ab{};
      X2SplitBatch xf{}, xd{};
      for (int i = 0; i < nb; ++i) {
        const int l = l0 + i;
        unsigned* slots = reinterpret_cast<unsigned*>(packed + p.off_wamax + (int64_t)l * WIRE_AMAX_SLOTS);
        ab.src[i] = packed + p.off_fwd[l]; ab.slots[i] = slots;
        xf.src[i] = packed + p.off_fwd[l]; xf.dst[i] = packed + p.off_fwd_x2[l]; xf.slots[i] = slots;
        xd.src[i] = packed + p.off_dg[l]; xd.dst[i] = packed + p.off_dg_x2[l]; xd.slots[i] = slots;
      }
      HIPCHK(launch_amax_batch(s, ab, nb, (int64_t)p.Pl * p.P));
      HIPCHK(launch_x2_split_b_batch(s, xf, nb, p.P, p.Pl, p.P));
      HIPCHK(launch_x2_split_b_batch(s, xd, nb, p.Pl, p.P, p.Pl));
      // the fused forward's edition of the forward image (the multi-pass net: one per pass, its c folded in)
      for (int k = 0; k < p.S2 && p.off_fx >= 0 && fused_pre_scale(p.kind, p.w, pass_c(p, k)) > 0.f; ++k) {
        FxSplitBatch fx{};
        for (int i = 0; i < nb; ++i) {
          const int l = l0 + i;
          fx.src[i] = packed + p.off_fwd[l];
          fx.dst[i] = packed + fx_pass_off(p, k) + (int64_t)(l - 1) * fused_b_image_floats(p.P);
          fx.slots[i] = ab.slots[i];
        }
        HIPCHK(launch_fx_split_b_batch(s, fx, nb, p.P, p.P, fused_pre_scale(p.kind, p.w, pass_c(p, k))));
      }
      if (p.off_fxd >= 0) {                                // the data-gradient chain's: transposed images, layers L .. 1
        FxSplitBatch fd{};
        int m = 0;
        for (int i = 0; i < nb; ++i) {
          const int l = l0 + i;
          fd.src[m] = packed + p.off_dg[l];
          fd.dst[m] = packed + p.off_fxd + (int64_t)(p.L - l) * fused_b_image_floats(p.P);
          fd.slots[m] = ab.slots[i];
          ++m;
        }
        if (m > 0) HIPCHK(launch_fx_split_b_batch(s, fd, m, p.Pl, p.P, 1.f));
      }
    }
  }
  return WIRE_OK;
}

extern "C" int wire_pack_params(void* stream, const wire_net_desc* d, const void* const* params,
                                float* packed) {
  Plan p; if (int rc = make_plan(d, p)) return rc;
  if (!params || !packed) return fail(WIRE_ERR_ARG, "null pointer");
  hipStream_t s = (hipStream_t)stream;
  ProfScope ps(s, 3, 0);
  for (int i = 0; i < p.ntens; ++i)
    if (!params[i]) return fail(WIRE_ERR_ARG, "params[%d] is null", i);
  HIPCHK(hipMemsetAsync(packed + p.off_wamax, 0, (size_t)(p.L + 1) * WIRE_AMAX_SLOTS * sizeof(float), s));
  if (p.first_gemm) {                                    // layer 0 as a GEMM (positional encoding): its own shape
    const float* W = (const float*)params[p.t0];
    const float* b = (const float*)params[p.t0 + 1];
    HIPCHK(launch_pack_hidden(s, p.kind, W, b, nullptr, nullptr, p.K, p.Din, p.P, p.Pin0, packed + p.off_fwd[0],
                              packed + p.off_dg[0], packed + p.off_bias[0]));
    HIPCHK(launch_x3_split_b(s, packed + p.off_fwd[0], p.Pin0, p.Pl, p.Pin0, packed + p.off_fwd_x3[0]));
    HIPCHK(launch_x3_split_b(s, packed + p.off_dg[0], p.Pl, p.Pin0, p.Pl, packed + p.off_dg_x3[0]));
    if (p.off_fx >= 0) {                                   // the fused forward's image of the GEMM first layer + its maximum
      unsigned* slots0 = reinterpret_cast<unsigned*>(packed + p.off_wamax);
      HIPCHK(launch_amax(s, packed + p.off_fwd[0], (int64_t)p.Pl * p.Pin0, slots0));
      FxSplitBatch f0{};
      f0.src[0] = packed + p.off_fwd[0]; f0.dst[0] = packed + p.off_fx; f0.slots[0] = slots0;
      HIPCHK(launch_fx_split_b_batch(s, f0, 1, p.Pin0, p.P, 1.f, p.Pin0));
    }
    if (p.ms) {                                            // the SHF -> K layer's 2 x fp16 forward image + its maximum
      X2AmaxBatch ab{};
      X2SplitBatch xf{};
      ab.src[0] = xf.src[0] = packed + p.off_fwd[0];
      ab.slots[0] = reinterpret_cast<unsigned*>(packed + p.off_wamax);
      xf.dst[0] = packed + p.off_fwd_x2[0]; xf.slots[0] = ab.slots[0];
      HIPCHK(launch_amax_batch(s, ab, 1, (int64_t)p.Pl * p.Pin0));
      HIPCHK(launch_x2_split_b_batch(s, xf, 1, p.Pin0, p.Pl, p.Pin0));
    }
  }
  if (p.hier) return hier_pack(s, p, params, packed);   // wire_hier_api.hip
  if (p.mfn) return mfn_pack(s, p, params, packed);     // wire_mfn_api.hip
  std::vector<const float*> hW(p.L + 1, nullptr), hb(p.L + 1, nullptr);
  for (int l = 1; l <= p.L; ++l) {
    hW[l] = (const float*)params[p.t0 + p.per_layer * l]; hb[l] = (const float*)params[p.t0 + p.per_layer * l + 1];
  }
  if (int rc = pack_hidden(s, p, params, packed, hW, hb)) return rc;
  HIPCHK(launch_pack_final(s, p.kind, (const float*)params[p.ntens - 2],
                           (const float*)params[p.ntens - 1], p.K, p.P, p.O, packed + p.off_wf,
                           packed + p.off_bf));
  if (!p.first_gemm || p.ms)   // (the multi-scale net: its first stage, read by mscale_first_kernel)
    for (int q = 0; q < p.per_layer; ++q) {
      if (q == 0 && p.ws != 1.f) {   // the cubic B-spline net: ws W0, as the hidden images (b0 stays as it is)
        HIPCHK(launch_scale_copy(s, (const float*)params[first_tensor(p, 0)], p.tfloats[first_tensor(p, 0)], p.ws,
                                 packed + first_native_off(p, 0)));
        continue;
      }
      HIPCHK(hipMemcpyAsync(packed + first_native_off(p, q), params[first_tensor(p, q)], p.tfloats[first_tensor(p, q)] * 4,
                            hipMemcpyDeviceToDevice, s));
    }
  if (p.m2) {                  // the combiner, read by the m2_comb kernels
    const M2Comb w = comb_of(p, packed);
    const float* dst[4] = {w.W1, w.b1, w.W2, w.b2};
    for (int q = 0; q < 4; ++q)
      HIPCHK(hipMemcpyAsync(const_cast<float*>(dst[q]), params[q], p.tfloats[q] * 4, hipMemcpyDeviceToDevice, s));
  }
  return WIRE_OK;
}

// ---------------------------------------------------------------------------
// whole-network forward
// ---------------------------------------------------------------------------
// the parameters of the whole-net kernels (wire_fused.hip) that the inference and the training forward share
static FusedFwdParams fused_params(const Plan& p, const float* packed, const float* coords, int64_t n) {
  FusedFwdParams fp;
  fp.coords = coords; fp.n = n;
  if (p.first_gemm) {
    fp.pe_F = p.F; fp.bias0 = packed + p.off_bias[0]; fp.wamax0 = wamax_of(p, packed, 0);
  } else {
    fp.W0 = packed + first_native_off(p, 0); fp.b0 = packed + first_native_off(p, 1);
  }
  fp.wimg = reinterpret_cast<const unsigned char*>(packed + p.off_fx);
  fp.bias = packed + p.off_bias[1]; fp.bias_stride = p.L >= 2 ? p.off_bias[2] - p.off_bias[1] : 0;
  fp.wamax = wamax_of(p, packed, 1); fp.wamax_stride = WIRE_AMAX_SLOTS;
  fp.D = p.D; fp.K = p.K; fp.L = p.L; fp.O = p.O; fp.w1 = p.w1; fp.w = p.w; fp.s = p.s;
  fp.c_first = fused_pre_scale(p.kind, p.w1, p.s); fp.c_hidden = fused_pre_scale(p.kind, p.w, p.s);
  fp.k2_first = p.s * p.s * 1.44269502f / (fp.c_first * fp.c_first);
  fp.k2 = p.s * p.s * 1.44269502f / (fp.c_hidden * fp.c_hidden);
  return fp;
}

// loss (train, r.fused_final): the target and the outputs of the final stage inside the fused training forward
static int mlp_fwd_core(void* stream, const Plan& p, const Route& r, const float* packed, const float* coords, int64_t n,
                        float* y, void* act, int64_t act_bytes, const FusedFwdParams* loss = nullptr) {
  const bool save = r.mode != MODE_INFER;
  if (n < 0) return fail(WIRE_ERR_ARG, "negative n");
  if (n == 0) return WIRE_OK;
  if (!packed || !coords || (!r.fuse && !y) || !act) return fail(WIRE_ERR_ARG, "null pointer");
  const ActLayout a = act_layout(p, n, save);
  if (act_bytes < a.total * 4) return fail(WIRE_ERR_SIZE, "act buffer %lld < %lld bytes",
                                           (long long)act_bytes, (long long)a.total * 4);
  hipStream_t s = (hipStream_t)stream;
  float* A = (float*)act;
  if (r.fused_fwd) {
    FusedFwdParams fp = fused_params(p, packed, coords, n);
    fp.wf = packed + p.off_wf; fp.bfr = packed + p.off_bf; fp.y = y;
    if (p.m2) {
      // once per pass: that pass's images (its c folded in) and c, the trunk's outputs at rows k n; then the combiner
      for (int k = 0; k < p.S2; ++k) {
        FusedFwdParams f = fp;
        f.wimg = reinterpret_cast<const unsigned char*>(packed + fx_pass_off(p, k));
        f.s = pass_c(p, k);
        f.c_first = fused_pre_scale(p.kind, p.w1, f.s); f.c_hidden = fused_pre_scale(p.kind, p.w, f.s);
        f.y = A + a.ytr + (int64_t)k * n * p.O;
        ProfScope ps(s, 0, 2.0 * n * p.Pl * p.P * p.L);
        HIPCHK(launch_fused_fwd(s, p.kind, p.P, f));
      }
      ProfScope ps(s, 3, 0);
      HIPCHK(launch_m2_comb_fwd(s, comb_of(p, packed), p.S2, p.O, A + a.ytr, n, y));
      return WIRE_OK;
    }
    ProfScope ps(s, 0, 2.0 * n * p.Pl * p.P * p.L);
    HIPCHK(launch_fused_fwd(s, p.kind, p.P, fp));
    return WIRE_OK;
  }
  unsigned* const amax = reinterpret_cast<unsigned*>(A + a.amax);            // slots of out_l at amax + 64 l
  if (r.fam == FAM_X2)   // (the multi-scale net's pe slots lie right behind)
    HIPCHK(hipMemsetAsync(amax, 0, (size_t)(p.L + 2 + (p.ms ? 1 : 0)) * WIRE_AMAX_SLOTS * sizeof(unsigned), s));
  unsigned* const pe_amax = reinterpret_cast<unsigned*>(A + a.pe_amax);
  if (p.ms) {
    MscaleC c{};
    for (int g = 0; g < p.T; ++g) c.c[g] = p.sc_c[g];
    ProfScope ps(s, 3, 0);
    HIPCHK(launch_mscale_first(s, coords, n, p.D, packed + first_native_off(p, 0), packed + first_native_off(p, 1), p.SHF,
                               c, p.ms_split, p.Pin0, r.pe_split,
                               r.fam0 == FAM_X2 && r.pe_split == 0.f ? pe_amax : nullptr, A + a.pe));
  } else if (p.first_gemm) {   // (also behind the fused training forward: the first layer's weight gradient reads them)
    ProfScope ps(s, 3, 0);
    HIPCHK(launch_posenc(s, coords, n, p.D, p.F, p.Pin0, A + a.pe));
  }
  if (r.fused_train) {
    // the hidden layers in one kernel that stores lin_l (not relu), out_0 (fp32 + its maximum), out_1 .. out_{L-1}
    // (pre-split pairs; relu: fp32 + maxima, and out_L) -- what the final stage, the data-gradient epilogues and the
    // weight-gradient GEMMs of mlp_bwd_core read
    FusedFwdParams fp = fused_params(p, packed, coords, n);
    fp.inv_c_first = 1.f / fp.c_first; fp.inv_c_hidden = 1.f / fp.c_hidden;
    fp.lin0 = p.cplx ? nullptr : A + a.lin0;
    fp.lin = p.kind == WIRE_KIND_RELU ? nullptr : A + a.lin1; fp.lin_stride = a.np * p.Pl;
    fp.out = A + a.out0; fp.out_stride = a.np * p.P;
    fp.amax_out = amax;
    fp.rstore = r.rstore ? 1 : 0;
    if (r.fused_final) {
      fp.wf = packed + p.off_wf; fp.bfr = packed + p.off_bf;
      fp.target = loss->target; fp.idx = loss->idx; fp.first = loss->first; fp.gscale = loss->gscale;
      fp.y = loss->y; fp.rec = loss->rec; fp.g_lin = loss->g_lin; fp.part_w = loss->part_w; fp.part_b = loss->part_b;
      fp.loss_partial = loss->loss_partial; fp.amax_g = loss->amax_g;
    }
    ProfScope ps(s, 0, 2.0 * n * p.Pl * p.P * p.L);
    HIPCHK(launch_fused_fwd(s, p.kind, p.P, fp));
    return WIRE_OK;
  }
  auto out_l = [&](int l) { return save ? A + a.out0 + (int64_t)l * a.np * p.P : A + ((l & 1) ? a.pong : a.ping); };
  auto lin_l = [&](int l) -> float* {
    // relu: out = max(lin, 0) carries everything its backward needs (lin > 0 <=> out > 0): lin is never written
    if (!save || p.kind == WIRE_KIND_RELU) return nullptr;
    return l == 0 ? A + a.lin0 : A + a.lin1 + (int64_t)(l - 1) * a.np * p.Pl;
  };
  // the multi-pass net: the trunk once per pass k with c = pass_c(p, k), its rows at k n of every buffer (every other kind:
  // one pass, offset 0, c = s); the maxima of the 2 x fp16 kernels gather over the passes (slots zeroed once above)
  auto at = [](float* b, int64_t off) -> float* { return b ? b + off : nullptr; };
  for (int k = 0; k < p.S2; ++k) {
    const float ck = pass_c(p, k);
    const int64_t ro = (int64_t)k * n;
    // ---- layer 0
    if (p.first_gemm) {
      GemmEpiParams ep; ep.bias = packed + p.off_bias[0]; ep.o0 = lin_l(0); ep.o1 = out_l(0);
      ep.ld0 = p.Pl; ep.ld1 = p.P; ep.omega = p.w1; ep.scale = p.s; ep.kvalid = p.K;
      if (r.fam == FAM_X2) ep.amax_out = amax;             // (the 3 x bf16 16 x 16 x 32 kernel tracks the maximum too)
      if (r.pe_split != 0.f) ep.a_split_inv = 1.f / r.pe_split;
      ProfScope ps(s, 0, 2.0 * n * p.Pl * p.Pin0);
      HIPCHK(layer_nt(s, p, r.fam0, packed, 0, false, epi_fwd(p.kind), A + a.pe, n, ep, pe_amax, wamax_of(p, packed, 0),
                      amax));
    } else {
      // W0, b0 [, V0, c0]
      auto first = [&](int q) { return q < p.per_layer ? packed + first_native_off(p, q) : nullptr; };
      ProfScope ps(s, 3, 0);
      HIPCHK(launch_first_fwd(s, p.kind, coords, n, p.D, first(0), first(1), first(2), first(3), p.K, p.P, p.w1, ck,
                              p.cplx ? nullptr : at(lin_l(0), ro * p.P), out_l(0) + ro * p.P,
                              r.fam == FAM_X2 ? amax : nullptr));
    }
    // ---- hidden layers
    for (int l = 1; l <= p.L; ++l) {
      GemmEpiParams ep; ep.bias = packed + p.off_bias[l]; ep.o0 = at(lin_l(l), ro * p.Pl); ep.o1 = out_l(l) + ro * p.P;
      ep.ld0 = p.Pl; ep.ld1 = p.P; ep.omega = p.w; ep.scale = ck; ep.kvalid = p.K;
      if (r.skip_out_L && l == p.L) ep.o1 = nullptr;       // the final stage recomputes it
      // pre-split activations: out_{l-1} read as such, out_l written as such (its maximum slots stay zero: not read)
      const float s_in = r.out_scale[l - 1], s_out = r.out_scale[l];
      if (s_in != 0.f) ep.a_split_inv = 1.f / s_in;
      if (s_out != 0.f) ep.o1_split = s_out;
      ProfScope ps(s, 0, 2.0 * n * p.Pl * p.P);
      HIPCHK(layer_nt(s, p, r.fam, packed, l, false, epi_fwd(p.kind), out_l(l - 1) + ro * p.P, n, ep,
                      amax + (l - 1) * WIRE_AMAX_SLOTS, wamax_of(p, packed, l),
                      s_out != 0.f ? nullptr : amax + l * WIRE_AMAX_SLOTS));
    }
  }
  if (!r.fuse) {
    ProfScope ps(s, 3, 0);
    // (the multi-pass net: the final linear of every pass in one launch, then the combiner -- the training call runs
    // the combiner inside its backward, with the loss)
    HIPCHK(launch_final_fwd(s, out_l(p.L), n * p.S2, p.P, p.O, packed + p.off_wf, packed + p.off_bf,
                            p.m2 ? A + a.ytr : y));
    if (p.m2 && r.mode != MODE_TRAIN) HIPCHK(launch_m2_comb_fwd(s, comb_of(p, packed), p.S2, p.O, A + a.ytr, n, y));
  }
  return WIRE_OK;
}

extern "C" int wire_mlp_fwd(void* stream, const wire_net_desc* d, const float* packed,
                            const float* coords, int64_t n, float* y, void* act, int64_t act_bytes,
                            int save_for_bwd) {
  Plan p; if (int rc = make_plan(d, p)) return rc;
  if (p.hier)
    return hier_fwd_core(stream, p, hier_route(p, n, save_for_bwd ? MODE_AUTOGRAD : MODE_INFER), packed, coords, n, y, act,
                         act_bytes);
  if (p.mfn)
    return mfn_fwd_core(stream, p, mfn_route(p, n, save_for_bwd ? MODE_AUTOGRAD : MODE_INFER), packed, coords, n, y, act,
                        act_bytes);
  return mlp_fwd_core(stream, p, make_route(p, n, save_for_bwd ? MODE_AUTOGRAD : MODE_INFER), packed, coords, n, y, act,
                      act_bytes);
}

// ---------------------------------------------------------------------------
// whole-network backward, in stages that share one context
// ---------------------------------------------------------------------------
namespace {
struct Bwd {
  const Plan& p; const Route& r; hipStream_t s;
  const float* packed; const float* coords; int64_t n;   // (coords: the multi-pass net's per-pass copies, see below)
  int64_t n1;                  // rows of one pass: the multi-pass net runs S2 passes (n = S2 n1), every other kind n1 = n
  const float* g_y;            // null when the training call ran the final stage (r.fuse)
  void* const* grads;          // null (wire_mlp_bwd_coords only): the data gradients and g_coords alone -- no
                               // weight-gradient GEMM, no reduction
  float* g_coords; wire_grad_ready_fn ready; void* user;
  ActLayout a; ScratchLayout sc; CoordLayout cl;
  const float* A; float* Sx;
  float* gcur = nullptr; float* gnext = nullptr;   // g_lin of the current layer and of the one below
  int chain_rows = 0;                              // rows of the chain's workgroups (its first-layer sums)

  const float* out_l(int l) const { return A + a.out0 + (int64_t)l * a.np * p.P; }
  const float* lin_l(int l) const { return l == 0 ? A + a.lin0 : A + a.lin1 + (int64_t)(l - 1) * a.np * p.Pl; }
  const float* first(int q) const { return packed + first_native_off(p, q); }
  unsigned* gslots(int l) const { return reinterpret_cast<unsigned*>(Sx + sc.gamax) + l * WIRE_AMAX_SLOTS; }   // g_lin_l
  const unsigned* oslots(int l) const { return reinterpret_cast<const unsigned*>(A + a.amax) + l * WIRE_AMAX_SLOTS; }
  float* grad(int t) const { return grads ? (float*)grads[t] : nullptr; }
  void done(int t, int count) const { if (ready) ready(user, t, count); }
  int64_t crp_set() const { return (int64_t)prereduce_room(colreduce_blocks(n)) * p.ldu * 5; }   // wire2d: the second set of sums
  // the stages, in launch order
  int final_stage();
  int first_point();
  int chain();
  int wgrad_batch();
  int layers();
  int coords_grad();
  int first_params();
  hipError_t hidden_tn(int l);
};

// 1. final linear + activation gradient of layer L.  r.fuse: the training call ran it already -- g_lin_L and the final
// layer's partial sums are in the scratch (one block per 128-row workgroup when the fused training forward formed them)
int Bwd::final_stage() {
  ProfScope ps(s, 3, 0);
  if (!r.fuse) {
    const float wL = (p.L == 0) ? p.w1 : p.w;
    if (p.L == 0 && p.cplx)   // no hidden layer: g_out0 is needed raw (stage 2)
      HIPCHK(launch_final_bwd(s, p.kind, 1, g_y, n, p.O, packed + p.off_wf, nullptr, out_l(0), p.K, p.P, wL, p.s, gcur,
                              Sx + sc.fpw, Sx + sc.fpb));
    else
      for (int k = 0; k < p.S2; ++k) {   // (the multi-pass net: per pass, with its c; partial blocks side by side)
        const int64_t ro = (int64_t)k * n1, bo = (int64_t)k * final_bwd_blocks(n1);
        HIPCHK(launch_final_bwd(s, p.kind, 0, g_y + ro * p.O, n1, p.O, packed + p.off_wf, lin_l(p.L) + ro * p.Pl,
                                out_l(p.L) + ro * p.P, p.K, p.P, wL, pass_c(p, k), gcur + ro * p.P,
                                Sx + sc.fpw + bo * p.O * p.P, Sx + sc.fpb + bo * p.O,
                                r.fam == FAM_X2 ? gslots(p.L) : nullptr));
      }
    if (!grads) return WIRE_OK;
  }
  const int nbf = r.fused_final ? (int)((n + 127) / 128) : p.S2 * final_bwd_blocks(n1);
  HIPCHK(launch_final_reduce(s, p.kind, Sx + sc.fpw, Sx + sc.fpb, nbf, p.O, p.K, p.P, grad(p.ntens - 2),
                             grad(p.ntens - 1)));
  done(p.ntens - 2, 2);
  return WIRE_OK;
}

// 2. no hidden layer (net = first Gabor layer + final linear): gcur holds the raw g_out0; the first layer's activation
// gradient is an elementwise pass (u recomputed from the coordinates), its column sums follow in stage 7
int Bwd::first_point() {
  ProfScope ps(s, 3, 0);
  if (p.kind == WIRE_KIND_WIRE)
    HIPCHK(launch_gabor_bwd_first_point(s, gcur, out_l(0), coords, p.D, first(0), first(1), n, p.K, p.P, p.w1, p.s,
                                        Sx + sc.gu, p.ldu));
  else
    HIPCHK(launch_gabor2d_bwd_first_point(s, gcur, out_l(0), coords, p.D, first(0), first(1), first(2), first(3), n, p.K,
                                          p.P, p.w1, p.s, Sx + sc.gu, p.ldu));
  return WIRE_OK;
}

// 3. the data gradients of layers L .. 1 as one chain (wire_fused.hip): every g_lin_l (l >= 1) lands in its own buffer,
// the weight-gradient GEMMs read them; the last link forms the first layer's sums g_lin_0^T [x | 1] per workgroup
// (positional encoding: stores g_lin_0 for the first layer's weight-gradient GEMM)
int Bwd::chain() {
  const bool relu = p.kind == WIRE_KIND_RELU;
  FusedBwdParams bp;
  bp.n = n;
  bp.g = Sx + sc.gch; bp.g_stride = sc.gch_stride;
  bp.gamax = gslots(0);
  bp.aux = relu ? A + a.out0 : A + a.lin1 - a.np * p.Pl;   // lin_l at lin1 + (l - 1) * np * Pl
  bp.aux_stride = relu ? a.np * p.P : a.np * p.Pl;
  bp.wimg = reinterpret_cast<const unsigned char*>(packed + p.off_fxd);
  bp.wamax = wamax_of(p, packed, 1); bp.wamax_stride = WIRE_AMAX_SLOTS;
  bp.L = p.L; bp.w = p.w; bp.s = p.s;
  bp.rstore = r.rstore ? 1 : 0; bp.c_hidden = fused_pre_scale(p.kind, p.w, p.s);
  bp.aux0 = relu ? A + a.out0 : A + a.lin0;
  bp.w1 = p.w1;
  if (!p.first_gemm) { bp.coords = coords; bp.D = p.D; bp.crp = Sx + sc.crp; bp.C = p.K; }
  if (p.m2) {
    // once per pass: its rows, its c, its blocks of first-layer sums behind the previous pass's (the coordinates are the
    // same n1 rows for every pass); first_params reduces all S2 sets at once
    bp.n = n1;
    for (int k = 0; k < p.S2; ++k) {
      const int64_t ro = (int64_t)k * n1;
      FusedBwdParams b = bp;
      b.g = bp.g + ro * p.P; b.aux = bp.aux + ro * p.P; b.aux0 = bp.aux0 + ro * p.P;
      b.s = pass_c(p, k); b.c_hidden = fused_pre_scale(p.kind, p.w, pass_c(p, k));
      if (k > 0) b.crp = bp.crp + (int64_t)k * ((n1 + chain_rows - 1) / chain_rows) * p.K * 5;
      ProfScope ps(s, 1, 2.0 * n1 * p.Pl * p.P * p.L);
      HIPCHK(launch_fused_bwd(s, p.kind, p.P, b, &chain_rows));   // (pass 0 sets chain_rows before pass 1 reads it)
    }
    return WIRE_OK;
  }
  ProfScope ps(s, 1, 2.0 * n * p.Pl * p.P * p.L);
  HIPCHK(launch_fused_bwd(s, p.kind, p.P, bp, &chain_rows));
  return WIRE_OK;
}

// 4. the weight-gradient batch of layers wb_l0 .. L (make_route), behind the chain
int Bwd::wgrad_batch() {
  const int l0 = r.wb_l0, nb = r.wb_n;
  const bool rs = r.rstore;
  const float s_z = rs ? 0.f : r.out_scale[l0 - 1];
  ProfScope ps(s, 2, 2.0 * n * p.Pl * p.P * nb);
  HIPCHK(launch_gemmx2_tn(s, Sx + sc.gch + l0 * sc.gch_stride, p.Pl, rs ? lin_l(l0 - 1) : out_l(l0 - 1), rs ? p.Pl : p.P,
                          n, p.Pl, p.P, r.wb_S, Sx + sc.slab, Sx + sc.bslab, gslots(l0), oslots(l0 - 1),
                          rs ? 1.f / 16384.f : (s_z != 0.f ? 1.f / s_z : 0.f), rs ? known_kind(p.kind).z_act : 0,
                          nb, sc.gch_stride, rs ? a.np * p.Pl : a.np * p.P, WIRE_AMAX_SLOTS));
  return WIRE_OK;
}

// the weight-gradient GEMM of hidden layer l on the route's family: slabs of g_lin_l^T [out_{l-1} | 1]
hipError_t Bwd::hidden_tn(int l) {
  const int S = r.tn_S;
  float* slab = Sx + sc.slab;
  float* bslab = Sx + sc.bslab;
  switch (r.tn_fam) {
    case FAM_3M: return launch_gemm3m_tn(s, gcur, p.P, out_l(l - 1), p.P, n, p.Kp, p.Kp, S, slab, bslab);
    case FAM_X2:
      if (r.rstore)   // Z = act(r_{l-1}) evaluated by the loader from the stored pre-activation (no out_{l-1}), scale 2^14
        return launch_gemmx2_tn(s, gcur, p.Pl, lin_l(l - 1), p.Pl, n, p.Pl, p.P, S, slab, bslab, gslots(l), nullptr,
                                1.f / 16384.f, known_kind(p.kind).z_act);
      return launch_gemmx2_tn(s, gcur, p.Pl, out_l(l - 1), p.P, n, p.Pl, p.P, S, slab, bslab, gslots(l), oslots(l - 1),
                              r.out_scale[l - 1] != 0.f ? 1.f / r.out_scale[l - 1] : 0.f);
    case FAM_X3: return launch_gemmx3_tn(s, gcur, p.Pl, out_l(l - 1), p.P, n, p.Pl, p.P, S, slab, bslab);
    default: return launch_gemm_tn(s, gcur, p.Pl, out_l(l - 1), p.P, n, p.Pl, p.P, S, slab, bslab);
  }
}

// 5. hidden layers L .. 1: the layer's weight gradient, then its data gradient (behind the chain: already there)
int Bwd::layers() {
  const int pl = p.per_layer;
  for (int l = p.L; l >= 1; --l) {
    if (r.chain) gcur = Sx + sc.gch + (int64_t)l * sc.gch_stride;
    if (grads) {
      const bool own = l < r.wb_l0;                         // else the batch wrote this layer's slabs: member l - wb_l0
      if (own) {
        ProfScope ps(s, 2, 2.0 * n * p.Pl * p.P);
        HIPCHK(hidden_tn(l));
      }
      const int S = own ? r.tn_S : r.wb_S;
      const int64_t m = own ? 0 : l - r.wb_l0;
      float* const slab = Sx + sc.slab + m * S * p.Pl * p.P;
      float* const bslab = Sx + sc.bslab + m * S * p.Pl;
      auto g = [&](int q) { return q < pl ? grad(p.t0 + pl * l + q) : nullptr; };   // W, b [, V, c] of layer l
      ProfScope ps(s, 3, 0);
      if (r.tn_fam == FAM_3M)
        HIPCHK(launch_wgrad3m_reduce(s, slab, bslab, S, p.K, p.K, p.Kp, p.Kp, g(0), g(1)));
      else
        HIPCHK(launch_wgrad_reduce(s, p.kind, slab, bslab, S, p.K, p.K, p.Pl, p.P, g(0), g(1), g(2), g(3), p.ws));
      done(p.t0 + pl * l, pl);
    }
    if (r.chain) continue;                                  // g_lin_{l-1} (l = 1: the first layer's sums) is already there
    const bool first_sums = grads && r.first_sums;
    GemmEpiParams ep;
    ep.scale = p.s; ep.kvalid = p.K; ep.ld1 = p.P; ep.i1 = out_l(l - 1);
    int epi;
    if (l > 1 || !p.cplx) {
      epi = epi_bwd(p.kind);
      ep.omega = (l - 1 == 0) ? p.w1 : p.w;
      ep.i0 = lin_l(l - 1); ep.o0 = gnext; ep.ld0 = p.Pl;
      ep.recompute_out = r.recompute_out && l >= 2;
      ep.lookahead = r.bwd_lookahead && ep.recompute_out;             // (lin_{l-1}: the activation buffer; g_lin_{l-1}: the scratch)
      // (real nets: the layer-1 epilogue sums g_lin_0 [x | 1] itself)
      if (l == 1 && first_sums) { ep.coords = coords; ep.D = p.D; ep.cr_partial = Sx + sc.crp; ep.cr_C = p.K; }
    } else {
      epi = (p.kind == WIRE_KIND_WIRE) ? EPI_GABOR_BWD_FIRST : EPI_GABOR2D_BWD_FIRST;
      ep.omega = p.w1;
      ep.coords = coords; ep.D = p.D; ep.ldu = p.ldu; ep.o0 = Sx + sc.gu;
      // (wire, wire2d: g_u [x | 1] per 256-row tile instead of storing g_u for a separate pass)
      if (first_sums) { ep.cr_partial = Sx + sc.crp; ep.cr_C = p.K; ep.cr_set = crp_set(); }
      ep.recompute_out = r.recompute_out0;
      ep.first_dn = r.first_dn;
      ep.W0 = first(0); ep.b0 = first(1);
      if (pl == 4) { ep.W0b = first(2); ep.b0b = first(3); }
    }
    if (!p.cplx && l == 1) ep.ld0 = p.P;
    if (l == 1 && g_coords && r.cg_epi) {
      ep.cg_partial = Sx + cl.cgp; ep.D = p.D;
      if (!p.cplx) ep.W0 = first(0);
    }
    // (g_lin_0 feeds no 2 x fp16 GEMM -- no maximum kept -- except the multi-scale net's SHF -> K weight gradient)
    // (the multi-pass net: once per pass, with its c and its rows; g_lin_{l-1}'s maximum gathers over the passes)
    for (int k = 0; k < p.S2; ++k) {
      const int64_t ro = (int64_t)k * n1;
      GemmEpiParams e = ep;
      if (k > 0) { e.scale = pass_c(p, k); e.i0 += ro * p.Pl; e.i1 += ro * p.P; e.o0 += ro * e.ld0; }
      ProfScope ps(s, 1, 2.0 * n1 * p.Pl * p.P);
      HIPCHK(layer_nt(s, p, r.fam, packed, l, true, epi, gcur + ro * p.Pl, n1, e, gslots(l), wamax_of(p, packed, l),
                      l >= 2 || r.tn0 == FAM_X2 ? gslots(l - 1) : nullptr));
    }
    float* t = gcur; gcur = gnext; gnext = t;
  }
  return WIRE_OK;
}

// 6. the coordinate gradient: the layer-1 data-gradient epilogue formed its per-row partials (cg_epi); the other paths
// stored g_lin_0 / g_u / g_p, which coordgrad_rows (positional encoding: the fp32 GEMM with the first layer's
// data-gradient image, then posenc_bwd) contracts
int Bwd::coords_grad() {
  if (!g_coords) return WIRE_OK;
  const float* gu = Sx + sc.gu;
  if (r.cg_epi) {
    HIPCHK(launch_coordgrad_reduce(s, Sx + cl.cgp, cl.ntiles, n, p.D, g_coords));
  } else if (p.kind == WIRE_KIND_WIRE) {
    HIPCHK(launch_coordgrad_rows(s, gu, p.ldu, nullptr, first(0), nullptr, p.K, p.D, n, g_coords));
  } else if (p.kind == WIRE_KIND_WIRE2D) {
    HIPCHK(launch_coordgrad_rows(s, gu, 2 * p.ldu, gu + p.ldu, first(0), first(2), p.K, p.D, n, g_coords));
  } else if (p.m2) {           // every pass's rows, then their sum (g_lin_0 holds each pass's c already)
    HIPCHK(launch_coordgrad_rows(s, gcur, p.P, nullptr, first(0), nullptr, p.K, p.D, n, Sx + cl.cgp));
    HIPCHK(launch_m2_sum_passes(s, Sx + cl.cgp, p.S2, n1, p.D, g_coords));
  } else if (!p.first_gemm) {
    HIPCHK(launch_coordgrad_rows(s, gcur, p.P, nullptr, first(0), nullptr, p.K, p.D, n, g_coords));
  } else {
    // g_pe = g_lin_0 W0 on the fp32 MFMA (the first layer's data-gradient image, Pin0 x P), then the encoding's chain rule
    GemmEpiParams ep;
    ep.o0 = Sx + cl.gpe; ep.ld0 = p.Pin0;
    HIPCHK(layer_nt(s, p, FAM_4M, packed, 0, true, EPI_STORE, gcur, n, ep));
    HIPCHK(launch_posenc_bwd(s, coords, n, p.D, p.F, Sx + cl.gpe, p.Pin0, g_coords));
  }
  return WIRE_OK;
}

// 7. the first layer's parameter gradients
int Bwd::first_params() {
  if (!grads) return WIRE_OK;
  float* const crp = Sx + sc.crp;
  if (p.cplx) {
    const float* gu = Sx + sc.gu;
    if (r.first_sums) {
      HIPCHK(launch_colreduce_final(s, p.K, p.D, n, crp, grad(0), grad(1)));
      if (p.kind == WIRE_KIND_WIRE2D) HIPCHK(launch_colreduce_final(s, p.K, p.D, n, crp + crp_set(), grad(2), grad(3)));
    } else if (p.kind == WIRE_KIND_WIRE) {
      HIPCHK(launch_colreduce(s, gu, p.ldu, p.K, coords, p.D, n, crp, grad(0), grad(1)));
    } else {
      HIPCHK(launch_colreduce(s, gu, 2 * p.ldu, p.K, coords, p.D, n, crp, grad(0), grad(1)));
      HIPCHK(launch_colreduce(s, gu + p.ldu, 2 * p.ldu, p.K, coords, p.D, n, crp, grad(2), grad(3)));
    }
  } else if (!p.first_gemm && r.chain) {
    // (the multi-pass net: S2 sets of blocks, one per pass)
    HIPCHK(launch_colreduce_final_blocks(s, p.K, p.D, p.S2 * (int)((n1 + chain_rows - 1) / chain_rows), crp, grad(p.t0),
                                         grad(p.t0 + 1), p.ws));
  } else if (!p.first_gemm && r.first_sums) {
    HIPCHK(launch_colreduce_final(s, p.K, p.D, n, crp, grad(0), grad(1), p.ws));
  } else if (!p.first_gemm) {   // (the multi-pass net: coords = the per-pass copies, n = all passes' rows)
    HIPCHK(launch_colreduce(s, gcur, p.P, p.K, coords, p.D, n, crp, grad(p.t0), grad(p.t0 + 1), p.ws));   // gcur: g_lin_0 [n][P]
  } else if (r.tn0 == FAM_X2) {                             // the multi-scale net: g_lin_0^T [pe | 1], pe pre-split
    const int S = gemmx2_tn_splits(n, p.P, p.Pin0, sc.S);
    HIPCHK(launch_gemmx2_tn(s, gcur, p.P, A + a.pe, p.Pin0, n, p.P, p.Pin0, S, Sx + sc.slab, Sx + sc.bslab, gslots(0),
                            nullptr, 1.f / r.pe_split));
    HIPCHK(launch_wgrad_reduce(s, p.kind, Sx + sc.slab, Sx + sc.bslab, S, p.K, p.Din, p.P, p.Pin0, grad(p.t0),
                               grad(p.t0 + 1), nullptr, nullptr));
  } else {
    const float* g0 = r.chain ? Sx + sc.gch : gcur;         // the chain stored g_lin_0 in its slot 0
    const bool x3 = r.tn0 == FAM_X3;
    const int S = x3 ? gemmx3_tn_splits(n, p.P, p.Pin0, sc.S) : gemm_tn_splits(n, p.P, p.Pin0, sc.S);
    HIPCHK(x3 ? launch_gemmx3_tn(s, g0, p.P, A + a.pe, p.Pin0, n, p.P, p.Pin0, S, Sx + sc.slab, Sx + sc.bslab)
              : launch_gemm_tn(s, g0, p.P, A + a.pe, p.Pin0, n, p.P, p.Pin0, S, Sx + sc.slab, Sx + sc.bslab));
    HIPCHK(launch_wgrad_reduce(s, p.kind, Sx + sc.slab, Sx + sc.bslab, S, p.K, p.Din, p.P, p.Pin0, grad(p.t0),
                               grad(p.t0 + 1), nullptr, nullptr));
  }
  done(p.t0, p.per_layer);
  if (p.ms) done(0, 2);                                     // the frozen first stage: never written, announced last
  return WIRE_OK;
}
}  // namespace

static int mlp_bwd_core(void* stream, const Plan& p, const Route& r, const float* packed, const float* coords, int64_t n,
                        const float* g_y, const void* act, int64_t act_bytes, void* scratch, int64_t scratch_bytes,
                        void* const* grads, wire_grad_ready_fn ready = nullptr, void* user = nullptr,
                        float* g_coords = nullptr, bool comb_done = false) {
  if (n <= 0) return fail(WIRE_ERR_ARG, "backward needs n > 0");
  // (the multi-pass net's training call ran its combiner's backward with the loss: comb_done, g_y not read)
  if (!packed || !coords || (!r.fuse && !g_y && !comb_done) || !act || !scratch || (!grads && !g_coords))
    return fail(WIRE_ERR_ARG, "null pointer");
  if (grads)
    for (int i = p.ms ? p.t0 : 0; i < p.ntens; ++i) if (!grads[i]) return fail(WIRE_ERR_ARG, "grads[%d] is null", i);
  if (p.ms && g_coords) return fail(WIRE_ERR_ARG, "no coordinate gradient through the frozen first stage of kind %d",
                                    (int)WIRE_KIND_BSPLINE_MS);
  Bwd c{p, r, (hipStream_t)stream, packed, coords, n * p.S2, n, g_y, grads, g_coords, ready, user, act_layout(p, n, 1),
        scratch_layout(p, n), coord_layout(p, n), (const float*)act, (float*)scratch};
  const int64_t need = g_coords ? c.cl.total : c.sc.total;
  if (act_bytes < c.a.total * 4) return fail(WIRE_ERR_SIZE, "act buffer too small");
  if (scratch_bytes < need * 4) return fail(WIRE_ERR_SIZE, "scratch %lld < %lld bytes",
                                            (long long)scratch_bytes, (long long)need * 4);
  c.gcur = c.Sx + c.sc.ga;
  c.gnext = c.Sx + c.sc.gb;
  if (p.m2) {
    // the combiner: g_y -> the trunk's output gradients (all passes) and its weight gradients, announced first; the
    // trunk's backward then reads them as its g_y.  Without the chain its first-layer sums (colreduce over all S2 n1
    // rows) read the coordinates once per pass; the chain reads the n1 rows per pass itself
    ProfScope ps(c.s, 3, 0);
    float* const part = c.Sx + c.sc.cpart;
    if (!comb_done)
      HIPCHK(launch_m2_comb_bwd(c.s, comb_of(p, packed), p.S2, p.O, c.A + c.a.ytr, n, M2Loss{}, g_y, c.Sx + c.sc.gtr,
                                grads ? part : nullptr, nullptr));
    if (r.chain) c.gcur = c.Sx + c.sc.gch + (int64_t)p.L * c.sc.gch_stride;   // g_lin_L where the chain reads it
    if (grads) {
      HIPCHK(launch_m2_comb_reduce(c.s, part, n, p.S2, p.O,
                                   M2Grads{c.grad(0), c.grad(1), c.grad(2), c.grad(3)}));
      c.done(0, 4);
      for (int k = 0; k < p.S2 && !r.chain; ++k)
        HIPCHK(hipMemcpyAsync(c.Sx + c.sc.crep + (int64_t)k * n * p.D, coords, (size_t)n * p.D * sizeof(float),
                              hipMemcpyDeviceToDevice, c.s));
      if (!r.chain) c.coords = c.Sx + c.sc.crep;
    }
    c.g_y = c.Sx + c.sc.gtr;
  }
  // (the fused path zeroed the slots before its final stage published max |g_lin_L|)
  if (r.fam == FAM_X2 && !r.fuse)
    HIPCHK(hipMemsetAsync(c.gslots(0), 0, (size_t)(p.L + 2) * WIRE_AMAX_SLOTS * sizeof(unsigned), c.s));
  int rc = c.final_stage();
  if (!rc && p.L == 0 && p.cplx) rc = c.first_point();
  if (!rc && r.chain) rc = c.chain();
  if (!rc && r.wb_n > 0) rc = c.wgrad_batch();
  if (!rc) rc = c.layers();
  if (rc) return rc;
  ProfScope ps(c.s, 3, 0);                                  // stages 6 and 7: one profiled span
  rc = c.coords_grad();
  return rc ? rc : c.first_params();
}

extern "C" int wire_mlp_bwd(void* stream, const wire_net_desc* d, const float* packed,
                            const float* coords, int64_t n, const float* g_y, const void* act,
                            int64_t act_bytes, void* scratch, int64_t scratch_bytes,
                            void* const* grads) {
  Plan p; if (int rc = make_plan(d, p)) return rc;
  if (!grads) return fail(WIRE_ERR_ARG, "null pointer");
  if (p.hier)
    return hier_bwd_core(stream, p, hier_route(p, n, MODE_AUTOGRAD), packed, coords, n, g_y, act, act_bytes, scratch,
                         scratch_bytes, grads, nullptr, nullptr, nullptr);
  if (p.mfn)
    return mfn_bwd_core(stream, p, mfn_route(p, n, MODE_AUTOGRAD), packed, coords, n, g_y, act, act_bytes, scratch,
                        scratch_bytes, grads, nullptr, nullptr, nullptr);
  return mlp_bwd_core(stream, p, make_route(p, n, MODE_AUTOGRAD), packed, coords, n, g_y, act, act_bytes, scratch,
                      scratch_bytes, grads);
}

extern "C" int wire_mlp_bwd_coords(void* stream, const wire_net_desc* d, const float* packed, const float* coords,
                                   int64_t n, const float* g_y, const void* act, int64_t act_bytes, void* scratch,
                                   int64_t scratch_bytes, void* const* grads_host, float* g_coords) {
  Plan p; if (int rc = make_plan(d, p)) return rc;
  if (!grads_host && !g_coords) return fail(WIRE_ERR_ARG, "wire_mlp_bwd_coords: neither grads_host nor g_coords");
  if (p.hier)
    return hier_bwd_core(stream, p, hier_route(p, n, MODE_AUTOGRAD), packed, coords, n, g_y, act, act_bytes, scratch,
                         scratch_bytes, grads_host, nullptr, nullptr, g_coords);
  if (p.mfn)
    return mfn_bwd_core(stream, p, mfn_route(p, n, MODE_AUTOGRAD), packed, coords, n, g_y, act, act_bytes, scratch,
                        scratch_bytes, grads_host, nullptr, nullptr, g_coords);
  return mlp_bwd_core(stream, p, make_route(p, n, MODE_AUTOGRAD), packed, coords, n, g_y, act, act_bytes, scratch,
                      scratch_bytes, grads_host, nullptr, nullptr, g_coords);
}

// ---------------------------------------------------------------------------
// fused training core: forward -> MSE -> backward in one call
// ---------------------------------------------------------------------------
extern "C" int wire_train_fwd_bwd_hooked(void* stream, const wire_net_desc* d, const float* packed,
                                         const float* coords, int64_t n, const float* target, const int64_t* idx,
                                         int64_t first, float weight, float* y, float* g_y, float* loss_out,
                                         float* rec, float* partial, void* act, int64_t act_bytes, void* scratch,
                                         int64_t scratch_bytes, void* const* grads, wire_grad_ready_fn ready,
                                         void* user) {
  Plan p; if (int rc = make_plan(d, p)) return rc;
  if (n <= 0) return fail(WIRE_ERR_ARG, "wire_train_fwd_bwd needs n > 0");
  if (!target || !y || !g_y || !loss_out || !partial) return fail(WIRE_ERR_ARG, "null pointer");
  hipStream_t s = (hipStream_t)stream;
  if (p.hier) {
    // the stages' forward; the last head's launch finishes y and forms the MSE terms and g_y; then the backward
    const Route hr = hier_route(p, n, MODE_TRAIN);
    const HierScratch sc = hier_scratch(p, n);
    if (!scratch || scratch_bytes < sc.total * 4) return fail(WIRE_ERR_SIZE, "scratch too small");
    float* Sx = (float*)scratch;
    const double inv_no = 1.0 / ((double)n * (double)p.O);
    M2Loss ls;
    ls.target = target; ls.idx = idx; ls.first = first; ls.gscale = (float)(weight * 2.0 * inv_no);
    ls.y = y; ls.g_y = g_y; ls.rec = rec;
    if (int rc = hier_fwd_core(stream, p, hr, packed, coords, n, y, act, act_bytes, &ls, Sx + sc.lpart)) return rc;
    { ProfScope ps(s, 3, 0);
      HIPCHK(launch_mse_final(s, Sx + sc.lpart, hier_head_blocks(n), (float)(weight * inv_no), loss_out)); }
    return hier_bwd_core(stream, p, hr, packed, coords, n, g_y, act, act_bytes, scratch, scratch_bytes, grads, ready, user,
                         nullptr);
  }
  if (p.mfn) {
    // layer by layer: the forward that stores z_l / lin_l, the MSE and its gradient, the backward
    const Route mr = mfn_route(p, n, MODE_TRAIN);
    if (int rc = mfn_fwd_core(stream, p, mr, packed, coords, n, y, act, act_bytes)) return rc;
    { ProfScope ps(s, 3, 0);
      HIPCHK(launch_mse_grad(s, y, target, idx, first, n, p.O, weight, g_y, loss_out, rec, partial)); }
    return mfn_bwd_core(stream, p, mr, packed, coords, n, g_y, act, act_bytes, scratch, scratch_bytes, grads, ready, user,
                        nullptr);
  }
  const Route r = make_route(p, n, MODE_TRAIN);
  if (p.m2) {
    // the trunk's passes; then ONE kernel runs the combiner's forward, the MSE, its gradient and the combiner's backward
    // (g_y of every trunk row + per-block weight-gradient and loss partials); the trunk's backward follows
    const ScratchLayout sc = scratch_layout(p, n);
    if (!scratch || scratch_bytes < sc.total * 4) return fail(WIRE_ERR_SIZE, "scratch too small");
    if (!act || act_bytes < act_layout(p, n, 1).total * 4) return fail(WIRE_ERR_SIZE, "act buffer too small");
    if (int rc = mlp_fwd_core(stream, p, r, packed, coords, n, y, act, act_bytes)) return rc;
    float* Sx = (float*)scratch;
    const int nblk = m2_comb_blocks(n);
    float* const loss_part = Sx + sc.cpart + (int64_t)nblk * m2_comb_grad_floats(p.S2, p.O);
    const double inv_no = 1.0 / ((double)n * (double)p.O);
    M2Loss ls;
    ls.target = target; ls.idx = idx; ls.first = first; ls.gscale = (float)(weight * 2.0 * inv_no);
    ls.y = y; ls.g_y = g_y; ls.rec = rec;
    { ProfScope ps(s, 3, 0);
      HIPCHK(launch_m2_comb_bwd(s, comb_of(p, packed), p.S2, p.O, (const float*)act + act_layout(p, n, 1).ytr, n, ls,
                                nullptr, Sx + sc.gtr, Sx + sc.cpart, loss_part));
      HIPCHK(launch_mse_final(s, loss_part, nblk, (float)(weight * inv_no), loss_out)); }
    return mlp_bwd_core(stream, p, r, packed, coords, n, nullptr, act, act_bytes, scratch, scratch_bytes, grads, ready, user,
                        nullptr, true);
  }
  if (!r.fuse) {
    if (int rc = mlp_fwd_core(stream, p, r, packed, coords, n, y, act, act_bytes)) return rc;
    { ProfScope ps(s, 3, 0);
      HIPCHK(launch_mse_grad(s, y, target, idx, first, n, p.O, weight, g_y, loss_out, rec, partial)); }
    return mlp_bwd_core(stream, p, r, packed, coords, n, g_y, act, act_bytes, scratch, scratch_bytes, grads, ready, user);
  }
  const ActLayout a = act_layout(p, n, 1);
  const ScratchLayout sc = scratch_layout(p, n);
  if (!scratch || scratch_bytes < sc.total * 4) return fail(WIRE_ERR_SIZE, "scratch too small");
  const float* A = (const float*)act;
  float* Sx = (float*)scratch;
  unsigned* const gamax = reinterpret_cast<unsigned*>(Sx + sc.gamax);
  if (r.fam == FAM_X2) HIPCHK(hipMemsetAsync(gamax, 0, (size_t)(p.L + 2) * WIRE_AMAX_SLOTS * sizeof(unsigned), s));
  float* gL = r.chain ? Sx + sc.gch + (int64_t)p.L * sc.gch_stride : Sx + sc.ga;
  // the final stage inside the fused training forward (real nets, r.fused_final)
  FusedFwdParams lp;
  const int fblocks = (int)((n + 127) / 128);
  const double inv_no = 1.0 / ((double)n * (double)p.O);
  lp.target = target; lp.idx = idx; lp.first = first; lp.gscale = (float)(weight * 2.0 * inv_no);
  lp.y = y; lp.rec = rec; lp.g_lin = gL; lp.part_w = Sx + sc.fpw; lp.part_b = Sx + sc.fpb; lp.loss_partial = Sx + sc.crp;
  lp.amax_g = gamax + p.L * WIRE_AMAX_SLOTS;
  if (int rc = mlp_fwd_core(stream, p, r, packed, coords, n, nullptr, act, act_bytes, &lp)) return rc;
  if (r.fused_final) {
    ProfScope ps(s, 3, 0);
    HIPCHK(launch_mse_final(s, Sx + sc.crp, fblocks, (float)(weight * inv_no), loss_out));
  } else {
    // final linear forward + MSE (loss, rec) + final linear backward + activation gradient of layer L: one pass over
    // out_L / lin_L instead of three (r.skip_out_L: out_L evaluated from lin_L, bit for bit what the lean epilogue of
    // the 16 x 16 x 32 forward kernel would have stored -- 1 GB less HBM traffic)
    ProfScope ps(s, 3, 0);
    const float* linL = p.kind == WIRE_KIND_RELU ? nullptr : A + a.lin1 + (int64_t)(p.L - 1) * a.np * p.Pl;
    HIPCHK(launch_final_fused(s, p.kind, r.skip_out_L ? nullptr : A + a.out0 + (int64_t)p.L * a.np * p.P, linL, n, p.P,
                              p.O, p.K, packed + p.off_wf, packed + p.off_bf, target, idx, first, weight,
                              p.w, p.s, y, rec, gL, Sx + sc.fpw, Sx + sc.fpb, Sx + sc.crp, loss_out,
                              r.fam == FAM_X2 ? gamax + p.L * WIRE_AMAX_SLOTS : nullptr));
  }
  return mlp_bwd_core(stream, p, r, packed, coords, n, nullptr, act, act_bytes, scratch, scratch_bytes, grads, ready, user);
}
extern "C" int wire_train_fwd_bwd(void* stream, const wire_net_desc* d, const float* packed,
                                  const float* coords, int64_t n, const float* target, const int64_t* idx,
                                  int64_t first, float weight, float* y, float* g_y, float* loss_out,
                                  float* rec, float* partial, void* act, int64_t act_bytes, void* scratch,
                                  int64_t scratch_bytes, void* const* grads) {
  return wire_train_fwd_bwd_hooked(stream, d, packed, coords, n, target, idx, first, weight, y, g_y, loss_out, rec, partial,
                                   act, act_bytes, scratch, scratch_bytes, grads, nullptr, nullptr);
}
