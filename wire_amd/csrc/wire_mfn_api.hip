// wire_mfn_api.hip -- the host code of the multiplicative filter network (WIRE_KIND_MFN, modules/mfn.py): its part of
// the pack, its forward and backward (layer by layer in every mode), its route and the per-layer
// calls on native tensors.  The kernels: wire_mfn.hip and the EPI_MFN_* epilogues; the plan: wire_plan.hip.
//   z_0 = g_0(x);  lin_l = z_{l-1} W_l^T + b_l,  z_l = lin_l g_l(x)  (l = 1 .. L; W_l = the reference's linear[l - 1]);
//   y = z_L W_f^T + b_f
#include "wire_plan.h"

// the families of make_route, nothing fused, nothing pre-split: the whole-net kernels and the data-gradient chain have
// no multiplicative stage, so the knobs that select them leave a filter network's calls unchanged
Route mfn_route(const Plan& p, int64_t n, RouteMode mode) {
  Route r = make_route(p, n, mode);
  r.fused_fwd = r.fuse = r.fused_train = r.fused_final = r.chain = r.rstore = r.skip_out_L = false;
  r.first_sums = r.cg_epi = r.first_dn = r.bwd_lookahead = r.recompute_out = r.recompute_out0 = false;
  r.wb_l0 = p.L + 1; r.wb_n = 0;
  for (float& v : r.out_scale) v = 0.f;
  return r;
}

// the hidden linears through pack_hidden (every family's image), the final linear, one table per filter
int mfn_pack(hipStream_t s, const Plan& p, const void* const* params, float* packed) {
  std::vector<const float*> hW(p.L + 1, nullptr), hb(p.L + 1, nullptr);
  for (int l = 1; l <= p.L; ++l) { hW[l] = (const float*)params[mfn_tw(p, l)]; hb[l] = (const float*)params[mfn_tw(p, l) + 1]; }
  if (int rc = pack_hidden(s, p, params, packed, hW, hb)) return rc;
  HIPCHK(launch_pack_final(s, p.kind, (const float*)params[p.ntens - 2], (const float*)params[p.ntens - 1], p.K, p.P, p.O,
                           packed + p.off_wf, packed + p.off_bf));
  for (int i = 0; i <= p.L; ++i)
    HIPCHK(launch_mfn_pack_table(s, (const float*)params[4 * i], (const float*)params[4 * i + 1],
                                 (const float*)params[4 * i + 2], (const float*)params[4 * i + 3], p.K, p.D, p.P,
                                 const_cast<float*>(mfn_tab(p, packed, i))));
  return WIRE_OK;
}

int mfn_fwd_core(void* stream, const Plan& p, const Route& r, const float* packed, const float* coords, int64_t n, float* y,
                 void* act, int64_t act_bytes) {
  const bool save = r.mode != MODE_INFER;
  if (n < 0) return fail(WIRE_ERR_ARG, "negative n");
  if (n == 0) return WIRE_OK;
  if (!packed || !coords || !y || !act) return fail(WIRE_ERR_ARG, "null pointer");
  const ActLayout a = act_layout(p, n, save);
  if (act_bytes < a.total * 4) return fail(WIRE_ERR_SIZE, "act buffer %lld < %lld bytes", (long long)act_bytes,
                                           (long long)a.total * 4);
  hipStream_t s = (hipStream_t)stream;
  float* A = (float*)act;
  const bool x2 = r.fam == FAM_X2;
  unsigned* const amax = reinterpret_cast<unsigned*>(A + a.amax);            // slots of z_l at amax + 64 l
  if (x2) HIPCHK(hipMemsetAsync(amax, 0, (size_t)(p.L + 2) * WIRE_AMAX_SLOTS * sizeof(unsigned), s));
  auto z_l = [&](int l) { return save ? A + a.out0 + (int64_t)l * a.np * p.P : A + ((l & 1) ? a.pong : a.ping); };
  auto lin_l = [&](int l) -> float* { return save ? A + a.lin1 + (int64_t)(l - 1) * a.np * p.Pl : nullptr; };
  {
    ProfScope ps(s, 3, 0);
    HIPCHK(launch_mfn_filter_fwd(s, mfn_tab(p, packed, 0), coords, n, p.D, p.K, p.P, nullptr, z_l(0), x2 ? amax : nullptr));
  }
  for (int l = 1; l <= p.L; ++l) {
    GemmEpiParams ep;
    ep.bias = packed + p.off_bias[l]; ep.o0 = lin_l(l); ep.o1 = z_l(l); ep.ld0 = p.P; ep.ld1 = p.P; ep.kvalid = p.K;
    ep.coords = coords; ep.D = p.D; ep.ftab = mfn_tab(p, packed, l);
    ProfScope ps(s, 0, 2.0 * n * p.P * p.P);
    HIPCHK(layer_nt(s, p, r.fam, packed, l, false, EPI_MFN_FWD, z_l(l - 1), n, ep, amax + (l - 1) * WIRE_AMAX_SLOTS,
                    wamax_of(p, packed, l), amax + l * WIRE_AMAX_SLOTS));
  }
  ProfScope ps(s, 3, 0);
  HIPCHK(launch_final_fwd(s, z_l(p.L), n, p.P, p.O, packed + p.off_wf, packed + p.off_bf, y));
  return WIRE_OK;
}

// Announcements (wire_train_fwd_bwd_hooked): the final linear; then for l = L .. 1 the pair {W_l, b_l} followed by the
// four tensors of filter l; filter 0 last.
int mfn_bwd_core(void* stream, const Plan& p, const Route& r, const float* packed, const float* coords, int64_t n,
                 const float* g_y, const void* act, int64_t act_bytes, void* scratch, int64_t scratch_bytes,
                 void* const* grads, wire_grad_ready_fn ready, void* user, float* g_coords) {
  if (n <= 0) return fail(WIRE_ERR_ARG, "backward needs n > 0");
  if (!packed || !coords || !g_y || !act || !scratch || (!grads && !g_coords)) return fail(WIRE_ERR_ARG, "null pointer");
  if (grads)
    for (int i = 0; i < p.ntens; ++i) if (!grads[i]) return fail(WIRE_ERR_ARG, "grads[%d] is null", i);
  const ActLayout a = act_layout(p, n, 1);
  const ScratchLayout sc = scratch_layout(p, n);
  const int64_t need = g_coords ? coord_layout(p, n).total : sc.total;
  if (act_bytes < a.total * 4) return fail(WIRE_ERR_SIZE, "act buffer too small");
  if (scratch_bytes < need * 4) return fail(WIRE_ERR_SIZE, "scratch %lld < %lld bytes", (long long)scratch_bytes,
                                            (long long)need * 4);
  hipStream_t s = (hipStream_t)stream;
  const float* A = (const float*)act;
  float* Sx = (float*)scratch;
  const bool x2 = r.fam == FAM_X2;
  auto z_l = [&](int l) { return A + a.out0 + (int64_t)l * a.np * p.P; };
  auto lin_l = [&](int l) { return A + a.lin1 + (int64_t)(l - 1) * a.np * p.Pl; };
  auto gslots = [&](int l) { return reinterpret_cast<unsigned*>(Sx + sc.gamax) + l * WIRE_AMAX_SLOTS; };   // g_lin_l
  auto oslots = [&](int l) { return reinterpret_cast<const unsigned*>(A + a.amax) + l * WIRE_AMAX_SLOTS; };  // z_l
  auto grad = [&](int t) -> float* { return (float*)grads[t]; };
  auto done = [&](int t, int cnt) { if (ready) ready(user, t, cnt); };
  float* gcur = Sx + sc.ga;
  float* gnext = Sx + sc.gb;
  float* const H = Sx + sc.mh;
  bool gx_started = false;
  // filter i from its upstream gradient in H: the 2 D + 2 column sums and its share of the coordinate gradient
  auto filter = [&](int i) -> int {
    ProfScope ps(s, 3, 0);
    if (grads)
      HIPCHK(launch_mfn_filter_sums(s, mfn_tab(p, packed, i), coords, n, p.D, p.K, H, p.P, Sx + sc.mfp, grad(4 * i),
                                    grad(4 * i + 1), grad(4 * i + 2), grad(4 * i + 3)));
    if (g_coords) {
      HIPCHK(launch_mfn_filter_gx(s, mfn_tab(p, packed, i), coords, n, p.D, p.K, H, p.P, gx_started ? 1 : 0, g_coords));
      gx_started = true;
    }
    return WIRE_OK;
  };
  if (x2) HIPCHK(hipMemsetAsync(gslots(0), 0, (size_t)(p.L + 2) * WIRE_AMAX_SLOTS * sizeof(unsigned), s));
  {
    ProfScope ps(s, 3, 0);
    HIPCHK(launch_mfn_final_bwd(s, g_y, n, p.O, packed + p.off_wf, z_l(p.L), p.L >= 1 ? lin_l(p.L) : nullptr,
                                mfn_tab(p, packed, p.L), coords, p.D, p.P, gcur, H, grads ? Sx + sc.fpw : nullptr,
                                grads ? Sx + sc.fpb : nullptr, x2 ? gslots(p.L) : nullptr));
    if (grads) {
      HIPCHK(launch_final_reduce(s, p.kind, Sx + sc.fpw, Sx + sc.fpb, final_bwd_blocks(n), p.O, p.K, p.P, grad(p.ntens - 2),
                                 grad(p.ntens - 1)));
      done(p.ntens - 2, 2);
    }
  }
  if (int rc = filter(p.L)) return rc;
  for (int l = p.L; l >= 1; --l) {
    if (grads) {   // g_W_l = g_lin_l^T z_{l-1}, g_b_l = its column sums
      {
        ProfScope ps(s, 2, 2.0 * n * p.P * p.P);
        float* slab = Sx + sc.slab;
        float* bslab = Sx + sc.bslab;
        switch (r.tn_fam) {
          case FAM_X2:
            HIPCHK(launch_gemmx2_tn(s, gcur, p.P, z_l(l - 1), p.P, n, p.P, p.P, r.tn_S, slab, bslab, gslots(l), oslots(l - 1)));
            break;
          case FAM_X3: HIPCHK(launch_gemmx3_tn(s, gcur, p.P, z_l(l - 1), p.P, n, p.P, p.P, r.tn_S, slab, bslab)); break;
          default: HIPCHK(launch_gemm_tn(s, gcur, p.P, z_l(l - 1), p.P, n, p.P, p.P, r.tn_S, slab, bslab)); break;
        }
      }
      ProfScope ps(s, 3, 0);
      HIPCHK(launch_wgrad_reduce(s, p.kind, Sx + sc.slab, Sx + sc.bslab, r.tn_S, p.K, p.K, p.P, p.P, grad(mfn_tw(p, l)),
                                 grad(mfn_tw(p, l) + 1), nullptr, nullptr));
      done(mfn_tw(p, l), 2);
      done(4 * l, 4);
    }
    {   // g_z_{l-1} = g_lin_l W_l; its epilogue forms g_lin_{l-1} = g_z g_{l-1}(x) and h = g_z lin_{l-1} (filter 0: h = g_z)
      GemmEpiParams ep;
      ep.kvalid = p.K; ep.ld0 = p.P; ep.ld1 = p.P; ep.coords = coords; ep.D = p.D;
      ep.i0 = l >= 2 ? lin_l(l - 1) : nullptr; ep.o0 = gnext; ep.o1 = H; ep.ftab = mfn_tab(p, packed, l - 1);
      ProfScope ps(s, 1, 2.0 * n * p.P * p.P);
      HIPCHK(layer_nt(s, p, r.fam, packed, l, true, EPI_MFN_BWD, gcur, n, ep, gslots(l), wamax_of(p, packed, l),
                      l >= 2 ? gslots(l - 1) : nullptr));
    }
    if (int rc = filter(l - 1)) return rc;
    float* t = gcur; gcur = gnext; gnext = t;
  }
  if (grads) done(0, 4);
  return WIRE_OK;
}

// ---------------------------------------------------------------------------
// GaborLayer.forward (modules/mfn.py:24-26) and its backward on native tensors
// ---------------------------------------------------------------------------
static int mfn_layer_args(int64_t n, int D, int K) {
  if (n <= 0) return fail(WIRE_ERR_ARG, "wire_mfn_filter: n must be positive");
  if (D < 1 || D > 4) return fail(WIRE_ERR_ARG, "in_features %d outside 1..4", D);
  if (K < 1 || K > 4096) return fail(WIRE_ERR_ARG, "out_features %d outside 1..4096", K);
  return WIRE_OK;
}
extern "C" int wire_mfn_filter_fwd(void* stream, const float* x, const float* mu, const float* gamma, const float* w,
                                   const float* c, int64_t n, int in_features, int out_features, float* out) {
  if (int rc = mfn_layer_args(n, in_features, out_features)) return rc;
  if (!x || !mu || !gamma || !w || !c || !out) return fail(WIRE_ERR_ARG, "null pointer");
  hipStream_t s = (hipStream_t)stream;
  ProfScope ps(s, 3, 0);
  HIPCHK(launch_mfn_filter_fwd_native(s, mu, gamma, w, c, x, n, in_features, out_features, out));
  return WIRE_OK;
}
extern "C" int64_t wire_mfn_filter_ws_bytes(int64_t n, int out_features) {
  if (n < 0 || out_features < 1) return fail(WIRE_ERR_ARG, "bad argument to wire_mfn_filter_ws_bytes");
  return (int64_t)(mfn_sums_blocks(n) + 1) * 10 * out_features * 4;
}
extern "C" int wire_mfn_filter_bwd(void* stream, const float* g_out, const float* x, const float* mu, const float* gamma,
                                   const float* w, const float* c, int64_t n, int in_features, int out_features,
                                   float* g_mu, float* g_gamma, float* g_w, float* g_c, float* g_x, void* ws,
                                   int64_t ws_bytes) {
  if (int rc = mfn_layer_args(n, in_features, out_features)) return rc;
  if (!g_out || !x || !mu || !gamma || !w || !c || !g_mu || !g_gamma || !g_w || !g_c || !ws)
    return fail(WIRE_ERR_ARG, "null pointer");
  if (ws_bytes < wire_mfn_filter_ws_bytes(n, out_features)) return fail(WIRE_ERR_SIZE, "workspace too small");
  hipStream_t s = (hipStream_t)stream;
  ProfScope ps(s, 3, 0);
  HIPCHK(launch_mfn_filter_sums_native(s, mu, gamma, w, c, x, n, in_features, out_features, g_out, (float*)ws, g_mu,
                                       g_gamma, g_w, g_c));
  if (g_x) HIPCHK(launch_mfn_filter_gx_native(s, mu, gamma, w, c, x, n, in_features, out_features, g_out, g_x));
  return WIRE_OK;
}
