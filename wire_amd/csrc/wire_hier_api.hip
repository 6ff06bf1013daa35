// wire_hier_api.hip -- the host code of the hierarchical B-spline net (WIRE_KIND_BSPLINE_HIER): its layouts, its part of
// the pack, its forward and backward cores (layer by layer in every mode) and its route.  The
// kernels: wire_hier.hip; the plan: wire_plan.hip.
#include "wire_plan.h"

static inline int hier_sets(const Plan& p) { return p.HS * (p.HL + 2); }
// Training / autograd: every lin and out has its own buffer; a stage's last out is written straight into the right half
// of the next stage's join input, its first layer's out into the left half.  Inference: two [n][P] and two [n][2P]
// buffers in turns (stage st reads join input st & 1 and writes the right half of the other)
HierAct hier_act(const Plan& p, int64_t n, int save) {
  HierAct a;
  const int S = p.HS, per = p.HL + 2;
  const int64_t nP = n * p.P;
  int64_t off = 0;
  a.amax = off; off += (int64_t)hier_sets(p) * WIRE_AMAX_SLOTS;
  a.lin.resize(S); a.out.resize(S); a.cat.assign(S, -1);
  int64_t tmp[2] = {-1, -1}, catb[2] = {-1, -1};
  if (!save) {
    tmp[0] = off; off += nP; tmp[1] = off; off += nP;
    if (S > 1) { catb[0] = off; off += 2 * nP; catb[1] = off; off += 2 * nP; }
  }
  for (int st = 1; st < S; ++st) {
    if (save) { a.cat[st] = off; off += 2 * nP; } else a.cat[st] = catb[st & 1];
  }
  for (int st = 0; st < S; ++st) {
    const int last = hier_last(p, st);
    a.lin[st].assign(last + 1, -1);
    a.out[st].resize(last + 1);
    for (int l = 0; l <= last; ++l) {
      if (save) { a.lin[st][l] = off; off += nP; }
      HierOut o{};
      if (st > 0 && l == 0) {                 // x_in: the left half of this stage's join input
        o.off = a.cat[st]; o.ld = 2 * p.P; o.aset = st * per;
      } else if (l == last && st + 1 < S) {   // x_st: the right half of the next stage's
        o.off = a.cat[st + 1] + p.P; o.ld = 2 * p.P; o.aset = (st + 1) * per;
      } else {
        o.ld = p.P;
        o.aset = l == last ? -1 : st * per + (st == 0 ? l : 1);
        if (save) { o.off = off; off += nP; } else o.off = tmp[st == 0 ? (l & 1) : (l == 1 ? 0 : 1)];
      }
      a.out[st][l] = o;
    }
  }
  a.total = off;
  return a;
}

HierScratch hier_scratch(const Plan& p, int64_t n) {
  HierScratch s{};
  int64_t off = 0;
  s.gamax = off; off += (int64_t)hier_sets(p) * WIRE_AMAX_SLOTS;
  for (int i = 0; i < 3; ++i) { s.g[i] = off; off += n * p.P; }
  const int pn = p.HS > 1 ? 2 * p.P : p.P;
  auto mx = [](int a, int b) { return a > b ? a : b; };
  const int s_x3k = mx(gemmx3_tn_splits_max(n, p.P, pn, 256), gemmx3_tn_splits_max(n, p.P, p.P, 256));
  const int s_4m = mx(gemm_tn_splits(n, p.P, pn, 64), gemm_tn_splits(n, p.P, p.P, 64));
  const int s_x2 = mx(gemmx2_tn_splits(n, p.P, pn, 256), gemmx2_tn_splits(n, p.P, p.P, 256));
  const int s_x3 = mx(s_x3k, s_x2), s_max = mx(mx(s_x3, s_4m), 1);
  s.S = mx(p.x3 ? s_x3 : s_4m, 1);
  s.slab = off; off += (int64_t)s_max * p.P * pn;
  s.bslab = off; off += (int64_t)s_max * p.P;
  const int nbf = prereduce_room(final_bwd_blocks(n));
  s.fpw = off; off += (int64_t)nbf * p.O * p.P;
  s.fpb = off; off += (int64_t)nbf * p.O + 64;
  s.crp = off; off += (int64_t)prereduce_room(colreduce_blocks(n)) * p.P * 5;
  s.lpart = off; off += HIER_HEAD_MAXBLK;
  s.total = off;
  off = (off + 63) / 64 * 64;
  s.cgp = off; off += (int64_t)p.HS * n * p.D;
  s.total_coords = off;
  return s;
}

// the join's forward GEMM [n][2P] x [P][2P]^T on family f
static hipError_t hier_join_nt(hipStream_t s, const Plan& p, WireFamily f, const float* packed, int st, const float* A, int64_t n,
                        GemmEpiParams ep, const unsigned* amax_a, unsigned* amax_out) {
  const int Kd = 2 * p.P, Nc = p.P;
  switch (f) {
    case FAM_X2:
      ep.amax_a = amax_a; ep.amax_out = amax_out;
      ep.amax_b = reinterpret_cast<const unsigned*>(packed + p.hj_wamax) + st * WIRE_AMAX_SLOTS;
      return launch_gemmx2h_nt(s, EPI_BSPLINE_FWD, A, Kd, packed + p.hj_fwd_x2[st], n, Nc, Kd, ep,
                               x2_waits(p.k_nt_bfirst, p.k_epi_early));
    case FAM_X3: return launch_gemmx3_nt(s, EPI_BSPLINE_FWD, A, Kd, packed + p.hj_fwd_x3[st], n, Nc, Kd, ep);
    default: return launch_gemm_nt(s, EPI_BSPLINE_FWD, A, Kd, packed + p.hj_fwd[st], Kd, n, Nc, Kd, ep);
  }
}
// slabs of G^T [Z | 1], G [n][P], Z [n][Pn] rows of ldz floats, on family f in S splits
static hipError_t hier_tn(hipStream_t s, const Plan& p, WireFamily f, const float* G, const float* Z, int ldz, int Pn, int64_t n,
                   int S, float* slab, float* bslab, const unsigned* amax_g, const unsigned* amax_z) {
  switch (f) {
    case FAM_X2: return launch_gemmx2_tn(s, G, p.P, Z, ldz, n, p.P, Pn, S, slab, bslab, amax_g, amax_z);
    case FAM_X3: return launch_gemmx3_tn(s, G, p.P, Z, ldz, n, p.P, Pn, S, slab, bslab);
    default: return launch_gemm_tn(s, G, p.P, Z, ldz, n, p.P, Pn, S, slab, bslab);
  }
}
static int hier_tn_splits(WireFamily f, int64_t n, int Pm, int Pn, int cap) {
  const int S = f == FAM_X2 ? gemmx2_tn_splits(n, Pm, Pn, cap) : f == FAM_X3 ? gemmx3_tn_splits(n, Pm, Pn, cap)
                                                                             : gemm_tn_splits(n, Pm, Pn, cap);
  return S < 1 ? 1 : S;
}

// forward.  loss (training): the last head's launch forms the MSE terms, g_y and the loss partials
int hier_fwd_core(void* stream, const Plan& p, const Route& r, const float* packed, const float* coords, int64_t n, float* y,
                  void* act, int64_t act_bytes, const M2Loss* loss, float* loss_part) {
  const bool save = r.mode != MODE_INFER;
  if (n < 0) return fail(WIRE_ERR_ARG, "negative n");
  if (n == 0) return WIRE_OK;
  if (!packed || !coords || !y || !act) return fail(WIRE_ERR_ARG, "null pointer");
  const HierAct a = hier_act(p, n, save);
  if (act_bytes < a.total * 4) return fail(WIRE_ERR_SIZE, "act buffer %lld < %lld bytes", (long long)act_bytes,
                                           (long long)a.total * 4);
  hipStream_t s = (hipStream_t)stream;
  float* A = (float*)act;
  const bool x2 = r.fam == FAM_X2;
  unsigned* const slots = reinterpret_cast<unsigned*>(A + a.amax);
  auto sl = [&](int aset) -> unsigned* { return (x2 && aset >= 0) ? slots + (int64_t)aset * WIRE_AMAX_SLOTS : nullptr; };
  if (x2) HIPCHK(hipMemsetAsync(slots, 0, (size_t)hier_sets(p) * WIRE_AMAX_SLOTS * sizeof(unsigned), s));
  for (int st = 0; st < p.HS; ++st) {
    const float c = p.sc_c[st];
    const HierNat nat = hier_nat(p, packed, st);
    const int last = hier_last(p, st);
    auto lin = [&](int l) -> float* { return a.lin[st][l] >= 0 ? A + a.lin[st][l] : nullptr; };
    {
      const HierOut& o = a.out[st][0];
      ProfScope ps(s, 3, 0);
      HIPCHK(launch_hier_first_fwd(s, coords, n, p.D, nat.W0, nat.b0, p.K, p.P, c, lin(0), A + o.off, o.ld, sl(o.aset)));
    }
    for (int l = 1; l <= last; ++l) {
      const HierOut& o = a.out[st][l];
      GemmEpiParams ep;
      ep.o0 = lin(l); ep.o1 = A + o.off; ep.ld0 = p.P; ep.ld1 = o.ld; ep.omega = p.w; ep.scale = c; ep.kvalid = p.K;
      if (st > 0 && l == 1) {
        ep.bias = packed + p.hj_bias[st];
        ProfScope ps(s, 0, 2.0 * n * p.P * 2 * p.P);
        HIPCHK(hier_join_nt(s, p, r.fam, packed, st, A + a.cat[st], n, ep, sl(a.out[st][0].aset), sl(o.aset)));
      } else {
        const int v = hier_v(p, st, l);
        const HierOut& in = a.out[st][l - 1];
        ep.bias = packed + p.off_bias[v];
        ProfScope ps(s, 0, 2.0 * n * p.P * p.P);
        HIPCHK(layer_nt(s, p, r.fam, packed, v, false, EPI_BSPLINE_FWD, A + in.off, n, ep, sl(in.aset), wamax_of(p, packed, v),
                        sl(o.aset)));
      }
    }
    const HierOut& xl = a.out[st][last];
    const bool fin = loss && st == p.HS - 1;
    ProfScope ps(s, 3, 0);
    HIPCHK(launch_hier_head_fwd(s, A + xl.off, xl.ld, nat.Wh, nat.bh, n, p.K, p.P, p.O, st > 0, y, fin ? *loss : M2Loss{},
                                fin ? loss_part : nullptr));
  }
  return WIRE_OK;
}

int hier_bwd_core(void* stream, const Plan& p, const Route& r, const float* packed, const float* coords, int64_t n,
                  const float* g_y, const void* act, int64_t act_bytes, void* scratch, int64_t scratch_bytes,
                  void* const* grads, wire_grad_ready_fn ready, void* user, float* g_coords) {
  if (n <= 0) return fail(WIRE_ERR_ARG, "backward needs n > 0");
  if (!packed || !coords || !g_y || !act || !scratch || (!grads && !g_coords)) return fail(WIRE_ERR_ARG, "null pointer");
  if (grads)
    for (int i = 0; i < p.ntens; ++i) if (!grads[i]) return fail(WIRE_ERR_ARG, "grads[%d] is null", i);
  const HierAct a = hier_act(p, n, 1);
  const HierScratch sc = hier_scratch(p, n);
  const int64_t need = g_coords ? sc.total_coords : sc.total;
  if (act_bytes < a.total * 4) return fail(WIRE_ERR_SIZE, "act buffer too small");
  if (scratch_bytes < need * 4) return fail(WIRE_ERR_SIZE, "scratch %lld < %lld bytes", (long long)scratch_bytes,
                                            (long long)need * 4);
  hipStream_t s = (hipStream_t)stream;
  const float* A = (const float*)act;
  float* Sx = (float*)scratch;
  const int S = p.HS, per = p.HL + 2;
  const bool x2 = r.fam == FAM_X2;
  // weight gradients: the K x K layers on the route's family; the join's [P] x [2P] on 2 x fp16 where that kernel has
  // the shape, else on the family below it
  const WireFamily tnj = (x2 && gemmx2_tn_applies(p.P, 2 * p.P)) ? FAM_X2 : p.x3 ? FAM_X3 : FAM_4M;
  const WireFamily tnk = r.tn_fam == FAM_3M ? FAM_4M : r.tn_fam;
  const int tnk_S = hier_tn_splits(tnk, n, p.P, p.P, sc.S), tnj_S = hier_tn_splits(tnj, n, p.P, 2 * p.P, sc.S);
  unsigned* const gs = reinterpret_cast<unsigned*>(Sx + sc.gamax);
  const unsigned* const os = reinterpret_cast<const unsigned*>(A + a.amax);
  auto gsl = [&](int st, int l) -> unsigned* { return x2 ? gs + (int64_t)(st * per + l) * WIRE_AMAX_SLOTS : nullptr; };
  auto osl = [&](int aset) -> const unsigned* { return (x2 && aset >= 0) ? os + (int64_t)aset * WIRE_AMAX_SLOTS : nullptr; };
  auto grad = [&](int t) -> float* { return (float*)grads[t]; };
  auto done = [&](int t, int cnt) { if (ready) ready(user, t, cnt); };
  if (x2) HIPCHK(hipMemsetAsync(gs, 0, (size_t)hier_sets(p) * WIRE_AMAX_SLOTS * sizeof(unsigned), s));
  // 1. the heads' weight gradients: g_y^T x_st needs nothing of the backward below, so they are final first
  if (grads) {
    ProfScope ps(s, 3, 0);
    for (int st = 0; st < S; ++st) {
      const HierOut& xl = a.out[st][hier_last(p, st)];
      HIPCHK(launch_hier_head_bwd(s, g_y, n, p.O, hier_nat(p, packed, st).Wh, A + xl.off, xl.ld, nullptr, nullptr, p.K, p.P,
                                  p.sc_c[st], nullptr, Sx + sc.fpw, Sx + sc.fpb, nullptr));
      HIPCHK(launch_final_reduce(s, WIRE_KIND_BSPLINE, Sx + sc.fpw, Sx + sc.fpb, final_bwd_blocks(n), p.O, p.K, p.P,
                                 grad(hier_th(p, st)), grad(hier_th(p, st) + 1)));
    }
    done(hier_th(p, 0), 2 * S);
  }
  // 2. the stages from the last to the first
  float* gcur = Sx + sc.g[0];
  float* gnext = Sx + sc.g[1];
  float* const T = Sx + sc.g[2];
  for (int st = S - 1; st >= 0; --st) {
    const float c = p.sc_c[st];
    const HierNat nat = hier_nat(p, packed, st);
    const int last = hier_last(p, st);
    {   // g_lin of the stage's last layer: its head's g_y Wh plus what the next stage's join sent back (T)
      ProfScope ps(s, 3, 0);
      HIPCHK(launch_hier_head_bwd(s, g_y, n, p.O, nat.Wh, nullptr, 0, A + a.lin[st][last], st + 1 < S ? T : nullptr, p.K,
                                  p.P, c, gcur, nullptr, nullptr, gsl(st, last)));
    }
    for (int l = last; l >= 1; --l) {
      const bool join = st > 0 && l == 1;
      if (grads) {
        const int t = hier_t(p, st, l);
        if (join) {   // ONE launch over [x_in | x_{st-1}]
          { ProfScope ps(s, 2, 2.0 * n * p.P * 2 * p.P);
            HIPCHK(hier_tn(s, p, tnj, gcur, A + a.cat[st], 2 * p.P, 2 * p.P, n, tnj_S, Sx + sc.slab, Sx + sc.bslab, gsl(st, l),
                           osl(st * per))); }
          ProfScope ps(s, 3, 0);
          HIPCHK(launch_hier_join_reduce(s, Sx + sc.slab, Sx + sc.bslab, tnj_S, p.K, p.P, grad(t), grad(t + 1)));
        } else {
          const HierOut& in = a.out[st][l - 1];
          { ProfScope ps(s, 2, 2.0 * n * p.P * p.P);
            HIPCHK(hier_tn(s, p, tnk, gcur, A + in.off, in.ld, p.P, n, tnk_S, Sx + sc.slab, Sx + sc.bslab, gsl(st, l),
                           osl(in.aset))); }
          ProfScope ps(s, 3, 0);
          HIPCHK(launch_wgrad_reduce(s, WIRE_KIND_BSPLINE, Sx + sc.slab, Sx + sc.bslab, tnk_S, p.K, p.K, p.P, p.P, grad(t),
                                     grad(t + 1), nullptr, nullptr));
        }
        done(t, 2);
      }
      GemmEpiParams ep;
      ep.kvalid = p.K; ep.ld0 = p.P; ep.ld1 = p.P; ep.omega = p.w;
      if (join) {
        // left half: this stage's first layer; right half: the previous stage's last layer, with ITS c -- T waits there
        // for that stage's head backward to add g_y Wh
        ep.scale = c; ep.i0 = A + a.lin[st][0]; ep.o0 = gnext;
        { ProfScope ps(s, 1, 2.0 * n * p.P * p.P);
          const int v = hier_vhalf(p, st, 0);
          HIPCHK(layer_nt(s, p, r.fam, packed, v, true, EPI_BSPLINE_BWD, gcur, n, ep, gsl(st, l), wamax_of(p, packed, v),
                          nullptr)); }
        ep.scale = p.sc_c[st - 1]; ep.i0 = A + a.lin[st - 1][hier_last(p, st - 1)]; ep.o0 = T;
        ProfScope ps(s, 1, 2.0 * n * p.P * p.P);
        const int v = hier_vhalf(p, st, 1);
        HIPCHK(layer_nt(s, p, r.fam, packed, v, true, EPI_BSPLINE_BWD, gcur, n, ep, gsl(st, l), wamax_of(p, packed, v),
                        nullptr));
      } else {
        ep.scale = c; ep.i0 = A + a.lin[st][l - 1]; ep.o0 = gnext;
        const int v = hier_v(p, st, l);
        ProfScope ps(s, 1, 2.0 * n * p.P * p.P);
        HIPCHK(layer_nt(s, p, r.fam, packed, v, true, EPI_BSPLINE_BWD, gcur, n, ep, gsl(st, l), wamax_of(p, packed, v),
                        l >= 2 ? gsl(st, l - 1) : nullptr));
      }
      float* t = gcur; gcur = gnext; gnext = t;
    }
    // gcur = g_lin_0 of the stage: its first layer's sums and its share of the coordinate gradient
    ProfScope ps(s, 3, 0);
    if (grads) {
      HIPCHK(launch_colreduce(s, gcur, p.P, p.K, coords, p.D, n, Sx + sc.crp, grad(hier_t(p, st, 0)),
                              grad(hier_t(p, st, 0) + 1)));
      done(hier_t(p, st, 0), 2);
    }
    if (g_coords)
      HIPCHK(launch_coordgrad_rows(s, gcur, p.P, nullptr, nat.W0, nullptr, p.K, p.D, n,
                                   S == 1 ? g_coords : Sx + sc.cgp + (int64_t)st * n * p.D));
  }
  if (g_coords && S > 1) {   // stage 0 first, in order
    ProfScope ps(s, 3, 0);
    HIPCHK(launch_m2_sum_passes(s, Sx + sc.cgp, S, n, p.D, g_coords));
  }
  return WIRE_OK;
}

// the route of a hierarchical net: the families of make_route, nothing fused, nothing pre-split
Route hier_route(const Plan& p, int64_t n, RouteMode mode) {
  Route r = make_route(p, n, mode);
  r.fused_fwd = r.fuse = r.fused_train = r.fused_final = r.chain = r.rstore = r.skip_out_L = false;
  r.first_sums = r.cg_epi = r.first_dn = r.bwd_lookahead = false;
  r.wb_l0 = p.L + 1; r.wb_n = 0;
  for (float& v : r.out_scale) v = 0.f;
  return r;
}

// the pack: the joins (their forward image in every family; their halves as two more hidden layers), the K -> K layers of
// every stage (pack_hidden), then every stage's first layer and head in their native layout
int hier_pack(hipStream_t s, const Plan& p, const void* const* params, float* packed) {
  // W, b of the plan's hidden layer l: the K -> K GEMMs of every stage (hier_v / hier_vhalf)
  std::vector<const float*> hW(p.L + 1, nullptr), hb(p.L + 1, nullptr);
  HIPCHK(hipMemsetAsync(packed + p.hj_wamax, 0, (size_t)p.HS * WIRE_AMAX_SLOTS * sizeof(float), s));
  for (int l = 1; l <= p.HL; ++l) {
    hW[l] = (const float*)params[hier_t(p, 0, l)]; hb[l] = (const float*)params[hier_t(p, 0, l) + 1];
  }
  for (int st = 1; st < p.HS; ++st) {
    // the join: its forward image in every family; its halves as two more hidden layers (their transposed images
    // serve the join's two data-gradient GEMMs, their forward images are not used)
    const float* Wj = (const float*)params[hier_t(p, st, 1)];
    const float* bj = (const float*)params[hier_t(p, st, 1) + 1];
    float* Wa = packed + p.hj_half[st];
    float* Wb = Wa + rup(p.K * p.K, 4);
    float* img = packed + p.hj_fwd[st];
    HIPCHK(launch_hier_pack_join(s, Wj, bj, p.K, p.P, img, packed + p.hj_bias[st], Wa, Wb));
    HIPCHK(launch_x3_split_b(s, img, 2 * p.P, p.P, 2 * p.P, packed + p.hj_fwd_x3[st]));
    X2AmaxBatch ab{};
    X2SplitBatch xf{};
    ab.src[0] = xf.src[0] = img;
    ab.slots[0] = reinterpret_cast<unsigned*>(packed + p.hj_wamax) + st * WIRE_AMAX_SLOTS;
    xf.dst[0] = packed + p.hj_fwd_x2[st]; xf.slots[0] = ab.slots[0];
    HIPCHK(launch_amax_batch(s, ab, 1, (int64_t)p.P * 2 * p.P));
    HIPCHK(launch_x2_split_b_batch(s, xf, 1, 2 * p.P, p.P, 2 * p.P));
    hW[hier_v(p, st, 2)] = (const float*)params[hier_t(p, st, 2)];
    hb[hier_v(p, st, 2)] = (const float*)params[hier_t(p, st, 2) + 1];
    hW[hier_vhalf(p, st, 0)] = Wa; hb[hier_vhalf(p, st, 0)] = bj;
    hW[hier_vhalf(p, st, 1)] = Wb; hb[hier_vhalf(p, st, 1)] = bj;
  }
  if (int rc = pack_hidden(s, p, params, packed, hW, hb)) return rc;
  for (int st = 0; st < p.HS; ++st) {
    const HierNat h = hier_nat(p, packed, st);
    const float* dst[4] = {h.W0, h.b0, h.Wh, h.bh};
    const int src[4] = {hier_t(p, st, 0), hier_t(p, st, 0) + 1, hier_th(p, st), hier_th(p, st) + 1};
    for (int q = 0; q < 4; ++q)
      HIPCHK(hipMemcpyAsync(const_cast<float*>(dst[q]), params[src[q]], p.tfloats[src[q]] * 4, hipMemcpyDeviceToDevice,
                            s));
  }
  return WIRE_OK;
}
