// wire_plan.hip -- the plan of a net (include/wire_hip.h: wire_net_desc), host code only: the descriptor's checks, the
// packed image, the activation and scratch layouts, the route of a whole-net call, and the size / offset queries of the
// C ABI that read them.
#include <cmath>

#include "wire_plan.h"

// ---------------------------------------------------------------------------
// network plan
// ---------------------------------------------------------------------------
// the extended descriptor of the three scaled kinds, read once: first_width (the multi-scale net alone has a first stage:
// columns [0, min(256, SHF)) divided by scale_tensor[0], group g >= 1 by scale_tensor[g] over [256 + (g - 1) split,
// 256 + g split); the groups must cover SHF exactly -- the next Linear takes SHF columns), lo .. WIRE_MS_MAX_SCALES scales
static int read_scales(const wire_net_desc_ms* m, int kind, int lo, Plan& p) {
  if (kind == WIRE_KIND_BSPLINE_MS) {
    p.SHF = m->first_width;
    if (p.SHF < 1 || p.SHF > 4096) return fail(WIRE_ERR_ARG, "first_width %d outside 1..4096", p.SHF);
  } else if (m->first_width != 0) {
    return fail(WIRE_ERR_ARG, "first_width %d: kind %d has no first stage", m->first_width, kind);
  }
  p.nsc = m->nscales;
  if (p.nsc < lo || p.nsc > WIRE_MS_MAX_SCALES)
    return fail(WIRE_ERR_ARG, "nscales %d outside %d..%d", p.nsc, lo, WIRE_MS_MAX_SCALES);
  if (p.SHF > 256) {
    p.ms_split = (p.SHF - 256) / (p.nsc - 1);
    if (p.ms_split < 1 || 256 + (p.nsc - 1) * p.ms_split != p.SHF)
      return fail(WIRE_ERR_ARG, "first_width %d is not 256 + %d equal column groups", p.SHF, p.nsc - 1);
  }
  for (int k = 0; k < p.nsc; ++k) {
    const float sk = m->scales[k];
    if (!(std::isfinite(sk) && sk != 0.f)) return fail(WIRE_ERR_ARG, "scales[%d] %g is zero or not finite", k, (double)sk);
    p.sc_c[k] = (float)(1.0 / fabs((double)sk));
  }
  return WIRE_OK;
}

int make_plan(const wire_net_desc* d, Plan& p) {
  if (!d) return fail(WIRE_ERR_ARG, "null descriptor");
  p.kind = d->kind; p.D = d->in_features; p.K = d->width; p.L = d->hidden_layers;
  p.O = d->out_features; p.F = d->posenc_freqs;
  p.w1 = d->first_omega0; p.w = d->hidden_omega0; p.s = d->scale0;
  p.ws = 1.f;
  // a base kind (wire_kinds.h) or one of the composite kinds rewritten onto one below
  if (!kind_row(p.kind) && p.kind != WIRE_KIND_BSPLINE_MS && p.kind != WIRE_KIND_BSPLINE_M2 &&
      p.kind != WIRE_KIND_BSPLINE_HIER && p.kind != WIRE_KIND_MFN)
    return fail(WIRE_ERR_ARG, "unknown kind %d", p.kind);
  if (p.kind == WIRE_KIND_MFN) {
    // modules/mfn.py: the omegas, `scale` and the positional encoding are carried and ignored; the K -> K layers are
    // real linears whose activation is the multiplication by the next filter (EPI_MFN_*)
    p.mfn = true;
    p.kind = WIRE_KIND_RELU;
    p.F = 0;
  }
  if (p.kind == WIRE_KIND_BSPLINE_HIER) {
    // modules/bspline_mscale_hier.py: one stage per entry of scale_tensor, `scale` unused
    const wire_net_desc_ms* m = reinterpret_cast<const wire_net_desc_ms*>(d);
    if (int rc = read_scales(m, WIRE_KIND_BSPLINE_HIER, 1, p)) return rc;
    p.HS = p.nsc;
    p.HL = p.L;
    if (p.HL < 1 || p.HL > 40) return fail(WIRE_ERR_ARG, "hidden_layers %d outside 1..40 (kind %d)", p.HL,
                                           (int)WIRE_KIND_BSPLINE_HIER);
    if (p.HL == 1 && p.HS > 1)
      return fail(WIRE_ERR_ARG, "hidden_layers 1 with %d scales: a later stage runs its layers 0, 1 and 2", p.HS);
    p.hier = true;
    p.kind = WIRE_KIND_BSPLINE;
    p.s = m->scales[0];
    p.L = p.HL + 3 * (p.HS - 1);
  }
  if (p.kind == WIRE_KIND_BSPLINE_M2) {
    // modules/bspline_mscale_2.py: the trunk of bspline_form once per entry of scale_tensor (lin / scale_k), `scale` unused
    const wire_net_desc_ms* m = reinterpret_cast<const wire_net_desc_ms*>(d);
    if (int rc = read_scales(m, WIRE_KIND_BSPLINE_M2, 1, p)) return rc;
    p.S2 = p.nsc;
    p.m2 = true;
    p.kind = WIRE_KIND_BSPLINE;
    p.s = m->scales[0];
    p.t0 = 4;
  }
  if (p.kind == WIRE_KIND_BSPLINE_MS) {
    // modules/bspline_mscale_HL.py: one column group of the first stage per entry of scale_tensor
    const wire_net_desc_ms* m = reinterpret_cast<const wire_net_desc_ms*>(d);
    if (int rc = read_scales(m, WIRE_KIND_BSPLINE_MS, 2, p)) return rc;
    p.ms = true; p.T = p.nsc;
    if (p.L < 0 || p.L > 65) return fail(WIRE_ERR_ARG, "hidden_layers %d outside 0..65", p.L);
    p.L = p.L > 1 ? p.L - 1 : 0;   // K -> K layers behind the SHF -> K one (hidden_layers = 0 builds the net of 1)
    p.kind = WIRE_KIND_BSPLINE;
    p.t0 = 2;
  }
  // the kernels' scale and the factor in the packed weights (kind_scale: sigma0 divides bspline_form's lin, modules/
  // bspline_form.py:44; scale_0 multiplies bspline_cubic's input, modules/bspline_cubic.py:45 -- the whole-net kernels then
  // fold c = 1 and the chain reads fp.s = 1)
  const float scale0 = p.s;
  if (!kind_scale(p.kind, scale0, p.s, p.ws))
    return fail(WIRE_ERR_ARG, "%s scale0 %g is zero or not finite", known_kind(p.kind).name, (double)scale0);
  if (p.D < 1 || p.D > 4) return fail(WIRE_ERR_ARG, "in_features %d outside 1..4", p.D);
  if (p.K < 1 || p.K > 4096) return fail(WIRE_ERR_ARG, "width %d outside 1..4096", p.K);
  if (p.L < 0 || p.L > 64) return fail(WIRE_ERR_ARG, "hidden_layers %d outside 0..64", p.L);
  if (p.O < 1 || p.O > 8) return fail(WIRE_ERR_ARG, "out_features %d outside 1..8", p.O);
  if (p.F < 0 || (p.F > 0 && p.kind != WIRE_KIND_RELU)) return fail(WIRE_ERR_ARG, "posenc only with relu");
  p.cplx = kind_is_cplx(p.kind);
  p.P = p.cplx ? rup(2 * p.K, 64) : rup(p.K, 64);
  // final_fwd_kernel (wire_final.hip) stages W_f as [O][P] floats in the 64 KB of dynamic LDS a launch gets
  if ((int64_t)p.O * p.P > WIRE_FINAL_MAX_OP)
    return fail(WIRE_ERR_ARG, "out_features %d x padded row width %d > %d (the final layer's weights in 64 KB)", p.O, p.P,
                WIRE_FINAL_MAX_OP);
  p.Pl = (p.kind == WIRE_KIND_WIRE2D) ? 2 * p.P : p.P;
  p.ldu = p.P / 2;
  p.Kp = p.P / 2;
  p.x3 = knob(K_SPLIT_BF16) != 0;
  p.x2 = p.x3 && knob(K_SPLIT_F16) != 0;
  p.m3 = (p.kind == WIRE_KIND_WIRE) && knob(K_COMPLEX_3M) && !p.x3;
  // one snapshot of the knobs that decide FORMATS (what the forward stores and the backward of the same call reads): a
  // wire_tune_set from another thread in the middle of wire_train_fwd_bwd must not split a call between two formats
  // (the forward and the backward of the autograd path are separate calls: knobs must not change between them)
  p.k_split_out = knob(K_SPLIT_OUT) != 0; p.k_recompute_out = knob(K_RECOMPUTE_OUT) != 0;
  p.k_first_sums = knob(K_FIRST_SUMS) != 0; p.k_first_dn = knob(K_FIRST_DN) != 0;
  p.k_nt_bfirst = knob(K_NT_BFIRST) != 0; p.k_epi_early = knob(K_EPI_EARLY) != 0;
  p.k_bwd_lookahead = knob(K_BWD_LOOKAHEAD) != 0; p.k_rstore = knob(K_FUSED_RSTORE) != 0; p.k_wgrad_batch = knob(K_WGRAD_BATCH) != 0;
  p.k_fused_fwd = knob(K_FUSED_FWD) != 0; p.k_fused_train = p.k_fused_fwd && knob(K_FUSED_TRAIN);
  p.k_fused_train_p384 = knob(K_FUSED_TRAIN_P384) != 0;
  p.k_fused_bwd = p.k_fused_train && knob(K_FUSED_BWD); p.k_fused_final = p.k_fused_train && knob(K_FUSED_FINAL);
  p.first_gemm = p.F > 0 || p.ms;
  p.Din = p.ms ? p.SHF : p.first_gemm ? p.D + 2 * p.D * p.F : p.D;
  p.Pin0 = p.first_gemm ? rup(p.Din, 64) : 0;
  p.per_layer = (p.kind == WIRE_KIND_WIRE2D) ? 4 : 2;
  p.ntens = p.t0 + p.per_layer * (p.L + 1) + 2;
  p.tfloats.assign(p.ntens, 0);
  if (p.ms) { p.tfloats[0] = (int64_t)p.SHF * p.D; p.tfloats[1] = p.SHF; }
  if (p.m2) {   // freq_mlp.0.weight, .0.bias, .2.weight, .2.bias
    p.tfloats[0] = (int64_t)M2_H * p.S2 * p.O; p.tfloats[1] = M2_H; p.tfloats[2] = (int64_t)p.O * M2_H; p.tfloats[3] = p.O;
  }
  const int64_t K = p.K, cm = p.cplx ? 2 : 1;
  for (int l = 0; l <= p.L; ++l) {
    const int64_t in = (l == 0) ? p.Din : K;
    const int64_t m = (l == 0) ? 1 : cm;   // first layer is real-valued
    for (int q = 0; q < p.per_layer; q += 2) {
      p.tfloats[p.t0 + p.per_layer * l + q] = m * K * in;
      p.tfloats[p.t0 + p.per_layer * l + q + 1] = m * K;
    }
  }
  p.tfloats[p.ntens - 2] = cm * p.O * K;
  p.tfloats[p.ntens - 1] = cm * p.O;
  if (p.mfn) {    // filters 0 .. L (mu, gamma, w, c), the hidden linears, the final linear
    p.ntens = 4 * (p.L + 1) + 2 * p.L + 2;
    p.tfloats.assign(p.ntens, 0);
    for (int i = 0; i <= p.L; ++i) {
      p.tfloats[4 * i] = K * p.D; p.tfloats[4 * i + 1] = K; p.tfloats[4 * i + 2] = K * p.D; p.tfloats[4 * i + 3] = K;
    }
    for (int l = 1; l <= p.L; ++l) { p.tfloats[mfn_tw(p, l)] = K * K; p.tfloats[mfn_tw(p, l) + 1] = K; }
    p.tfloats[p.ntens - 2] = p.O * K; p.tfloats[p.ntens - 1] = p.O;
  }
  if (p.hier) {   // stage 0: HL + 1 pairs; stages s >= 1: three pairs (layer 1: [K][2K]); the HS heads at the end
    p.ntens = 2 * (p.HL + 1) + 6 * (p.HS - 1) + 2 * p.HS;
    p.tfloats.assign(p.ntens, 0);
    for (int st = 0; st < p.HS; ++st)
      for (int l = 0; l <= hier_last(p, st); ++l) {
        p.tfloats[hier_t(p, st, l)] = K * (l == 0 ? p.D : (st > 0 && l == 1) ? 2 * K : K);
        p.tfloats[hier_t(p, st, l) + 1] = K;
      }
    for (int st = 0; st < p.HS; ++st) { p.tfloats[hier_th(p, st)] = p.O * K; p.tfloats[hier_th(p, st) + 1] = p.O; }
  }
  // packed image
  int64_t off = 0;
  p.off_fwd.assign(p.L + 1, -1); p.off_dg.assign(p.L + 1, -1); p.off_bias.assign(p.L + 1, -1);
  p.off_fwd_x3.assign(p.L + 1, -1); p.off_dg_x3.assign(p.L + 1, -1);
  p.off_fwd_3m.assign(p.L + 1, -1); p.off_dg_3m.assign(p.L + 1, -1);
  p.off_fwd_x2.assign(p.L + 1, -1); p.off_dg_x2.assign(p.L + 1, -1);
  for (int l = p.first_gemm ? 0 : 1; l <= p.L; ++l) {
    const int64_t pin = (l == 0) ? p.Pin0 : p.P;
    // every family's image is ALWAYS written by wire_pack_params (real-expanded fp32, its split-bf16 form and,
    // for `wire`, the blocked complex planes of the 3M kernels), so a packed buffer stays valid whatever the
    // tuning flags are when it is used (e.g. changed between a forward and its backward)
    const int64_t img = (int64_t)p.Pl * pin;
    p.off_fwd[l] = off; off += img;
    p.off_dg[l] = off; off += img;
    p.off_bias[l] = off; off += p.Pl;
    p.off_fwd_x3[l] = off; off += gemmx3_b_image_floats(p.Pl, (int)pin);
    p.off_dg_x3[l] = off; off += gemmx3_b_image_floats((int)pin, p.Pl);
    if (p.kind == WIRE_KIND_WIRE && l >= 1) {
      p.off_fwd_3m[l] = off; off += (int64_t)p.Kp * p.P;
      p.off_dg_3m[l] = off; off += (int64_t)p.Kp * p.P;
    }
    if (l >= 1) {                                         // 2 x fp16 images of the hidden layers
      p.off_fwd_x2[l] = off; off += gemmx2_b_image_floats(p.Pl, (int)pin);
      p.off_dg_x2[l] = off; off += gemmx2_b_image_floats((int)pin, p.Pl);
    } else if (p.ms) {                                    // ... and the forward one of the SHF -> K layer (no data gradient)
      p.off_fwd_x2[l] = off; off += gemmx2_b_image_floats(p.Pl, (int)pin);
    }
  }
  p.off_wamax = off; off += (int64_t)(p.L + 1) * WIRE_AMAX_SLOTS;
  p.off_fx = -1;
  // (a positional-encoding net -- relu, 64 padded encoded features -- has its GEMM first layer's image, P x 64, in front)
  // (the multi-pass net: one set of hidden images per pass, each with its own c folded in -- fx_pass_off; the chain's
  // transposed images below carry no c and serve every pass)
  // (the multiplicative filter network runs layer by layer: no whole-net image)
  const bool fx_ok = !p.hier && !p.mfn && p.L >= 1 && fused_fwd_shape(p.kind, p.P) &&
                     (!p.first_gemm || (p.kind == WIRE_KIND_RELU && p.Pin0 == 64));
  if (fx_ok) {
    p.off_fx = off;
    off += (p.first_gemm ? (int64_t)p.P * p.Pin0 : 0) + (int64_t)p.S2 * p.L * fused_b_image_floats(p.P);
  }
  p.off_fxd = -1;
  if (fx_ok && p.L >= 1 && fused_bwd_shape(p.kind, p.P)) { p.off_fxd = off; off += (int64_t)p.L * fused_b_image_floats(p.P); }
  p.off_wf = off; off += (int64_t)p.O * p.P;
  p.off_bf = off; off += 64;
  p.off_first = off;   // native copies of the first layer's tensors (W0,b0[,V0,c0]; the multi-scale net's first stage)
  if (p.hier) {
    for (int st = 1; st < p.HS; ++st) {
      const int64_t img = (int64_t)p.P * 2 * p.P;
      p.hj_fwd[st] = off; off += img;
      p.hj_bias[st] = off; off += p.P;
      p.hj_fwd_x3[st] = off; off += gemmx3_b_image_floats(p.P, 2 * p.P);
      p.hj_fwd_x2[st] = off; off += gemmx2_b_image_floats(p.P, 2 * p.P);
      p.hj_half[st] = off; off += 2 * rup(p.K * p.K, 4);
    }
    p.hj_wamax = off; off += (int64_t)p.HS * WIRE_AMAX_SLOTS;
    p.h_nat = off;                                         // per stage: W0 [K][D], b0 [K], Wh [O][K], bh [O]
    off += (int64_t)p.HS * hier_nat_stride(p);
  } else if (p.mfn) {
    p.mf_tab = off; off += (int64_t)(p.L + 1) * p.P * 12;    // the filters' tables [P][MFN_TAB]
  } else if (!p.first_gemm || p.ms) {
    for (int q = 0; q < p.per_layer; ++q) off += rup((int)p.tfloats[first_tensor(p, q)], 4);
  }
  if (p.m2) {                                              // the combiner's native copy
    p.off_comb = off;
    for (int q = 0; q < 4; ++q) off += rup((int)p.tfloats[q], 4);
  }
  p.total_packed = off;
  return WIRE_OK;
}

ActLayout act_layout(const Plan& p, int64_t n1, int save) {
  ActLayout a{};
  int64_t off = 0;
  const int64_t n = n1 * p.S2;                // the trunk's rows (the multi-pass net: S2 passes of n1)
  a.np = (n + 127) / 128 * 128 + (p.m2 ? 128 : 0);   // (the multi-pass net: the chain's last tiles read past S2 n1)
  a.amax = off; off += (int64_t)(p.L + 2) * WIRE_AMAX_SLOTS;
  a.pe_amax = off; if (p.ms) off += WIRE_AMAX_SLOTS;
  a.pe = off; if (p.first_gemm) off += n * p.Pin0;
  if (save) {
    a.out0 = off; off += a.np * p.P * (p.L + 1);
    a.lin0 = off; if (!p.cplx && !p.mfn) off += a.np * p.P;   // (a filter network's z_0 has no pre-activation)
    a.lin1 = off; off += a.np * p.Pl * p.L;
  } else {
    a.ping = off; off += n * p.P;
    a.pong = off; off += n * p.P;
  }
  a.ytr = off; if (p.m2) off += n * p.O;     // the trunk's outputs [S2][n1][O], the combiner's input
  a.total = off;
  return a;
}

ScratchLayout scratch_layout(const Plan& p, int64_t n1) {
  ScratchLayout s{};
  int64_t off = 0;
  const int64_t n = n1 * p.S2;
  s.gamax = off; off += (int64_t)(p.L + 2) * WIRE_AMAX_SLOTS;   // max |g_lin_l| slots (2 x fp16 GEMMs)
  s.ga = off; off += n * p.Pl;
  s.gb = off; off += n * p.Pl;
  // the data-gradient chain (wire_fused.hip: fused_bwd_kernel) keeps EVERY g_lin_l (l = 1 .. L; the weight-gradient GEMMs
  // run after it), rows padded to 128: g_lin_l at gch + l * gch_stride
  // (the multi-pass net: 128 rows more -- the last pass's whole workgroup tiles start at (S2 - 1) n1)
  s.gch = -1; s.gch_stride = ((n + 127) / 128 * 128 + (p.m2 ? 128 : 0)) * p.Pl;
  if (p.off_fxd >= 0) { s.gch = off; off += (int64_t)(p.L + 1) * s.gch_stride; }
  s.gu = off; if (p.cplx) off += n * p.ldu * (p.kind == WIRE_KIND_WIRE2D ? 2 : 1);
  const int64_t pn = p.first_gemm && p.Pin0 > p.P ? p.Pin0 : p.P;
  // slabs sized for the largest split count of the three GEMM families (flag-independent scratch size)
  // (the split-bf16 kernel may split finer: narrow nets have few tiles and would otherwise leave CUs idle)
  const int s_x3k = gemmx3_tn_splits_max(n, p.Pl, (int)pn, 256), s_4m = gemm_tn_splits(n, p.Pl, (int)pn, 64);
  const int s_x2 = gemmx2_tn_splits(n, p.Pl, (int)pn, 256);      // 0 when the 2 x fp16 kernel has no shape for the widths
  const int s_x3 = s_x3k > s_x2 ? s_x3k : s_x2;                  // split-family slabs: room for either kernel's count
  const int s_max = s_x3 > s_4m ? s_x3 : s_4m;
  if (p.m3) {
    s.S = gemm3m_tn_splits(n, p.Kp, p.Kp, 64);
    int64_t need = (int64_t)s.S * 3 * p.Kp * p.Kp, full = (int64_t)s_max * p.Pl * pn;
    s.slab = off; off += need > full ? need : full;
    need = (int64_t)s.S * 2 * p.Kp; full = (int64_t)s_max * p.Pl;
    s.bslab = off; off += need > full ? need : full;
  } else {
    s.S = p.x3 ? s_x3 : s_4m;
    int64_t need3 = 0, needb3 = 0;
    if (p.kind == WIRE_KIND_WIRE) {
      const int s3 = gemm3m_tn_splits(n, p.Kp, p.Kp, 64);
      need3 = (int64_t)s3 * 3 * p.Kp * p.Kp; needb3 = (int64_t)s3 * 2 * p.Kp;
    }
    int64_t full = (int64_t)s_max * p.Pl * pn;
    s.slab = off; off += need3 > full ? need3 : full;
    full = (int64_t)s_max * p.Pl;
    s.bslab = off; off += needb3 > full ? needb3 : full;
  }
  // + pre-reduction scratch; the training forward with the final stage inside writes one block per 128-row workgroup
  // (the multi-pass net: one set of blocks per pass)
  const int nbf = prereduce_room((p.off_fx >= 0 && !p.cplx ? 2 : 1) * p.S2 * final_bwd_blocks(n1));
  s.fpw = off; off += (int64_t)nbf * p.O * p.P;
  s.fpb = off; off += (int64_t)nbf * p.O + 64;
  // (wire2d: two sets, one per Linear of the first layer, when the data-gradient epilogue forms the sums itself)
  // (the data-gradient chain writes one block of first-layer sums per 64- or 128-row workgroup: 4 x the 256-row blocks)
  s.crp = off; off += (int64_t)prereduce_room((p.off_fxd >= 0 ? 4 : 1) * colreduce_blocks(n)) * (p.cplx ? p.ldu : p.P) * 5 *
                      (p.kind == WIRE_KIND_WIRE2D ? 2 : 1);
  s.gtr = s.cpart = s.crep = off;
  if (p.m2) {
    s.gtr = off; off += n * p.O;
    s.cpart = off; off += (int64_t)m2_comb_blocks(n1) * m2_comb_grad_floats(p.S2, p.O) + M2_COMB_MAXBLK;   // + loss partials
    s.crep = off; off += n * p.D;
  }
  s.mh = s.mfp = off;
  if (p.mfn) {
    s.mh = off; off += n * p.P;
    s.mfp = off; off += (int64_t)(mfn_sums_blocks(n) + 1) * 10 * p.K;
  }
  s.total = off;
  return s;
}

CoordLayout coord_layout(const Plan& p, int64_t n) {
  CoordLayout c{};
  int64_t off = (scratch_layout(p, n).total + 63) / 64 * 64;
  c.ntiles = (p.P + 127) / 128;
  c.cgp = off; off += (int64_t)c.ntiles * n * p.S2 * p.D;
  off = (off + 63) / 64 * 64;
  c.gpe = off; if (p.first_gemm) off += n * p.Pin0;
  c.total = off;
  return c;
}

// ---------------------------------------------------------------------------
// route: what one whole-net call runs, decided once from (plan, n, entry point)
// ---------------------------------------------------------------------------
// Power-of-two split scale of activations with an a-priori bound (bound < 2^e -> 2^(15 - e): |out| scale < 2^15): sine
// and Gaussian <= 1, the B-splines <= 3/4 and 2/3; Gabor |exp(j w lin - s^2 |lin|^2)| = exp(-w v - s^2 (u^2 + v^2)) <= exp((w / 2s)^2), attained at
// lin = -j w / 2 s^2 -- accepted up to 16 (w / s <= 3.33: every configuration of the reference's scripts); 0 beyond it
static float act_bound_scale(const Plan& p) {
  double bound = 1.0;
  if (p.cplx) {
    if (!(p.s > 0.f)) return 0.f;
    const double r = (double)p.w / (2.0 * (double)p.s);
    if (!(r * r <= 2.7725887)) return 0.f;                 // ln 16
    bound = exp(r * r);
  }
  return ldexpf(1.f, 15 - (ilogb(bound) + 1));
}

Route make_route(const Plan& p, int64_t n, RouteMode mode) {
  Route r{};
  r.mode = mode;
  const bool h16_fwd = gemmx3_nt_is_h16(epi_fwd(p.kind), n);
  // 2 x fp16 splits: every forward / data-gradient launch of the hidden layers is then a 16 x 16 x 32 kernel (M >= 4096,
  // x3_h16 bits of the kind), whose epilogues track the maxima the next GEMM scales by
  const bool x2 = p.x2 && p.L >= 1 && h16_fwd && gemmx3_nt_is_h16(epi_bwd(p.kind), n);
  const bool x2tn = x2 && gemmx2_tn_applies(p.Pl, p.P);
  r.fam = x2 ? FAM_X2 : p.m3 ? FAM_3M : p.x3 ? FAM_X3 : FAM_4M;
  r.fam0 = p.x3 ? FAM_X3 : FAM_4M;
  r.tn0 = r.fam0;
  if (p.ms && x2) {
    // the SHF -> K layer is the widest GEMM of the net: its forward joins the hidden layers' family; its weight gradient
    // runs 2 x fp16 where the TN kernel has a shape (and the scratch was sized for it: Pin0 >= P).  Then both readers take
    // the first stage's map pre-split at 2^15 (B <= 0.75 < 2^0: scaled below 2^15, no device-side maximum)
    r.fam0 = FAM_X2;
    if (p.Pin0 >= p.P && gemmx2_tn_applies(p.Pl, p.Pin0)) { r.tn0 = FAM_X2; r.pe_split = 32768.f; }
  }
  r.tn_fam = p.m3 ? FAM_3M : x2tn ? FAM_X2 : p.x3 ? FAM_X3 : FAM_4M;
  // (the multi-pass net: n rows per pass decide the forward and data-gradient kernels, its weight gradients reduce over
  // all S2 n rows at once)
  const int64_t nt = n * p.S2;
  const int S_max = scratch_layout(p, n).S;
  r.tn_S = r.tn_fam == FAM_3M ? S_max
         : r.tn_fam == FAM_X2 ? gemmx2_tn_splits(nt, p.Pl, p.P, S_max)
         : r.tn_fam == FAM_X3 ? gemmx3_tn_splits(nt, p.Pl, p.P, S_max) : gemm_tn_splits(nt, p.Pl, p.P, S_max);
  // a hidden layer whose forward ran the lean 16 x 16 x 32 epilogue: its out = act(lin) again, 8 B / element less (real
  // nets: only below a hidden layer -- the first layer's out comes from first_fwd_kernel's precise form)
  r.recompute_out = p.k_recompute_out && p.x3 && h16_fwd;
  // (relu: the fused kernels take each wave's own maximum; Gabor beyond the bound: the layer-by-layer path runs)
  r.act_scale = (p.kind == WIRE_KIND_RELU || p.kind == WIRE_KIND_WIRE2D) ? 0.f : act_bound_scale(p);
  // the whole-net kernels: a shape that has one, at most 8 hidden layers, a bound on the activations
  const bool fx = x2 && p.off_fx >= 0 && p.L <= 8 && (r.act_scale != 0.f || p.kind == WIRE_KIND_RELU) &&
                  fused_pre_scale(p.kind, p.w1, p.s) > 0.f && fused_pre_scale(p.kind, p.w, p.s) > 0.f;
  r.fused_fwd = mode == MODE_INFER && fx && p.k_fused_fwd && p.O <= 4;
  // The training forward as one kernel that stores lin_l / out_l on the way: the 2 x fp16 family with its pre-split
  // activations and recompute_out (the formats that kernel writes); wire at P = 384 spills in its storing edition.  It
  // decides the FORMAT of the stored out_l (pre-split at scale 1), so it is asked in every mode
  const bool ftrain = fx && x2tn && p.k_fused_train && p.k_split_out && p.k_recompute_out &&
                      !(p.kind == WIRE_KIND_WIRE && p.P > 256 && !p.k_fused_train_p384);
  // (the multi-pass net's loss sits behind its combiner: no final stage with the MSE inside)
  r.fuse = mode == MODE_TRAIN && p.L >= 1 && p.O <= 4 && !p.m2 && final_fused_supported(p.P, p.O);
  r.skip_out_L = r.fuse && r.recompute_out && p.kind != WIRE_KIND_RELU;
  r.fused_train = r.fuse && ftrain && (r.skip_out_L || p.kind == WIRE_KIND_RELU);
  // chain => fused_train, by construction: the chain reads g_lin_L and lin_l / r_l as only the fused training forward
  // stores them.  The multi-pass net's training forward runs layer by layer (its loss sits behind the combiner); that
  // stores every lin_l in fp32 in the reference's units, the form the chain reads without rstore, and its per-pass
  // final backward leaves g_lin_L where the chain reads it: the chain runs once per pass with that pass's c
  const bool m2_chain = p.m2 && mode == MODE_TRAIN && fx && x2tn;
  r.chain = (r.fused_train || m2_chain) && p.k_fused_bwd && p.off_fxd >= 0;
  r.fused_final = r.chain && r.fused_train && !p.cplx && p.k_fused_final;
  r.rstore = r.chain && r.fused_train && p.k_rstore && known_kind(p.kind).rstore;                        // 1.3 GB per step less
  // out_l is stored pre-split (wire_dev.h: wire_store_out4) when the call runs the 2 x fp16 kernels and every reader of
  // out_l understands the format: the forward GEMM of layer l + 1 (pre-split A edition), the weight-gradient GEMM of layer
  // l + 1 (gemmx2_tn16, pre-split Z) and NOTHING else -- the data-gradient epilogue of layer l + 1 must evaluate
  // act(lin_l) again rather than read out_l (recompute_out; sine and B-spline need no out), out_0 comes from first_fwd_kernel, out_L
  // feeds the final linear layer in fp32, relu's out carries its backward's sign decisions
  const bool split = x2tn && p.k_split_out && p.kind != WIRE_KIND_RELU &&
                     (p.k_recompute_out || known_kind(p.kind).split_out_free);
  for (int l = 1; l < p.L; ++l) r.out_scale[l] = !split ? 0.f : ftrain ? 1.f : act_bound_scale(p);
  // the layer-1 data gradient of a native first layer on the 16 x 16 x 32 kernel: its epilogue can sum g_lin_0 (wire:
  // g_u) [x | 1] per tile itself instead of storing it for a separate pass, and form the coordinate-gradient partials
  const int epi1 = p.kind == WIRE_KIND_WIRE ? EPI_GABOR_BWD_FIRST
                 : p.kind == WIRE_KIND_WIRE2D ? EPI_GABOR2D_BWD_FIRST : epi_bwd(p.kind);
  const bool h16_1 = p.x3 && gemmx3_nt_is_h16(epi1, n);
  // (the multi-pass net: its layer-1 data gradient runs once per pass, its first-layer sums over all passes at once)
  r.cg_epi = h16_1 && !p.first_gemm && p.L >= 1 && !p.m2;
  r.first_sums = r.cg_epi && p.k_first_sums;
  r.first_dn = h16_1 && p.cplx && p.k_first_dn;
  r.bwd_lookahead = p.kind == WIRE_KIND_WIRE && p.x3 && gemmx3_nt_is_h16(EPI_GABOR_BWD, n) && p.k_bwd_lookahead;
  r.recompute_out0 = h16_1 && p.kind == WIRE_KIND_WIRE && p.k_recompute_out;
  // behind the chain every g_lin_l exists before the first weight gradient starts: those of layers 2 .. L (same shape,
  // operands a fixed step apart) run as ONE launch, each member accumulating L - 1 times the rows into a third of the
  // slabs (layer 1 joins when its activation operand has the form of the others': r_0 of rstore, relu's fp32 out_0)
  r.wb_l0 = p.L + 1;
  if (r.chain && p.k_wgrad_batch) {                        // (the chain runs on the 2 x fp16 weight-gradient kernel)
    const int l0 = (r.rstore || p.kind == WIRE_KIND_RELU) ? 1 : 2, nb = p.L - l0 + 1;
    const int S = nb >= 2 ? gemmx2_tn_batch_splits(n, p.Pl, p.P, S_max, nb) : 0;
    if (S >= 1 && (int64_t)S * nb <= S_max) { r.wb_l0 = l0; r.wb_n = nb; r.wb_S = S; }
  }
  return r;
}

// ---------------------------------------------------------------------------
// size queries
// ---------------------------------------------------------------------------
extern "C" int wire_num_param_tensors(const wire_net_desc* d) {
  Plan p; if (make_plan(d, p)) return WIRE_ERR_ARG;
  return p.ntens;
}
extern "C" int64_t wire_param_tensor_floats(const wire_net_desc* d, int t) {
  Plan p; if (make_plan(d, p)) return WIRE_ERR_ARG;
  if (t < 0 || t >= p.ntens) return fail(WIRE_ERR_ARG, "tensor index %d out of range", t);
  return p.tfloats[t];
}
extern "C" int64_t wire_packed_floats(const wire_net_desc* d) {
  Plan p; if (make_plan(d, p)) return WIRE_ERR_ARG;
  return p.total_packed;
}
extern "C" int64_t wire_act_bytes(const wire_net_desc* d, int64_t n, int save_for_bwd) {
  Plan p; if (make_plan(d, p)) return WIRE_ERR_ARG;
  if (n < 0) return fail(WIRE_ERR_ARG, "negative n");
  if (p.hier) return hier_act(p, n, save_for_bwd).total * 4 + 256;
  return act_layout(p, n, save_for_bwd).total * 4 + 256;
}
extern "C" int64_t wire_bwd_scratch_bytes(const wire_net_desc* d, int64_t n) {
  Plan p; if (make_plan(d, p)) return WIRE_ERR_ARG;
  if (n < 0) return fail(WIRE_ERR_ARG, "negative n");
  if (p.hier) return hier_scratch(p, n).total * 4 + 256;
  return scratch_layout(p, n).total * 4 + 256;
}
extern "C" int64_t wire_bwd_coords_scratch_bytes(const wire_net_desc* d, int64_t n) {
  Plan p; if (make_plan(d, p)) return WIRE_ERR_ARG;
  if (n < 0) return fail(WIRE_ERR_ARG, "negative n");
  if (p.hier) return hier_scratch(p, n).total_coords * 4 + 256;
  return coord_layout(p, n).total * 4 + 256;
}
extern "C" int wire_blocked_width(int K) { return rup(2 * K, 64); }
// float offset of out_l (rows of P floats, l = 0..L) inside an act buffer laid out for n rows with save_for_bwd = 1
extern "C" int64_t wire_act_out_offset(const wire_net_desc* d, int64_t n, int layer) {
  Plan p; if (make_plan(d, p)) return WIRE_ERR_ARG;
  if (p.hier) return fail(WIRE_ERR_ARG, "wire_act_out_offset: kind %d keeps its activations per stage", (int)WIRE_KIND_BSPLINE_HIER);
  if (n < 0 || layer < 0 || layer > p.L) return fail(WIRE_ERR_ARG, "bad argument to wire_act_out_offset");
  const ActLayout a = act_layout(p, n, 1);
  return a.out0 + (int64_t)layer * a.np * p.P;
}
