// wire_api.hip -- the C ABI of libwire_hip.so (include/wire_hip.h): argument
// checking, buffer carving and the launch sequences of the WIRE hot path.
// No device memory is allocated here; every launch goes on the caller's stream.
#include <hip/hip_runtime.h>

#include <cmath>
#include <cstdarg>
#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <atomic>
#include <mutex>
#include <string>
#include <vector>

#include "../../include/wire_hip.h"
#include "wire_gemm.h"
#include "wire_point.h"

#ifndef WIRE_AMAX_SLOTS
#define WIRE_AMAX_SLOTS 64            // wire_dev.h (device header): sharded max-|value| slots per operand tensor
#endif

// ---------------------------------------------------------------------------
// error plumbing
// ---------------------------------------------------------------------------
static thread_local std::string g_err;
static int fail(int code, const char* fmt, ...) {
  char buf[512];
  va_list ap;
  va_start(ap, fmt);
  vsnprintf(buf, sizeof buf, fmt, ap);
  va_end(ap);
  g_err = buf;
  return code;
}
#define HIPCHK(expr)                                                                   \
  do {                                                                                 \
    hipError_t e_ = (expr);                                                            \
    if (e_ != hipSuccess)                                                              \
      return fail(WIRE_ERR_HIP, "%s failed: %s (%s:%d)", #expr, hipGetErrorString(e_), \
                  __FILE__, __LINE__);                                                 \
  } while (0)

int wire_fail_(int code, const char* msg) { return fail(code, "%s", msg); }   // wire_layer_api.hip

extern "C" int wire_abi_version(void) { return WIRE_ABI_VERSION; }
extern "C" const char* wire_last_error(void) { return g_err.c_str(); }

// ---------------------------------------------------------------------------
// profiling hooks
// ---------------------------------------------------------------------------
namespace {
struct ProfRec { hipEvent_t a, b; int cls; double flops; };
std::mutex g_prof_mu;
std::atomic<bool> g_prof_on{false};
std::vector<ProfRec> g_prof_recs;
std::vector<std::pair<hipEvent_t, hipEvent_t>> g_prof_pool;

struct ProfScope {
  hipStream_t s; int cls; double flops; bool on; hipEvent_t a{}, b{};
  ProfScope(hipStream_t s_, int cls_, double flops_) : s(s_), cls(cls_), flops(flops_), on(false) {
    if (!g_prof_on.load(std::memory_order_relaxed)) return;   // profiling off: no lock on the launch path
    std::lock_guard<std::mutex> lk(g_prof_mu);
    if (!g_prof_on.load(std::memory_order_relaxed)) return;
    on = true;
    if (!g_prof_pool.empty()) {
      a = g_prof_pool.back().first; b = g_prof_pool.back().second; g_prof_pool.pop_back();
    } else {
      (void)hipEventCreate(&a); (void)hipEventCreate(&b);
    }
    (void)hipEventRecord(a, s);
  }
  ~ProfScope() {
    if (!on) return;
    (void)hipEventRecord(b, s);
    std::lock_guard<std::mutex> lk(g_prof_mu);
    g_prof_recs.push_back({a, b, cls, flops});
  }
};
}  // namespace

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

// ---------------------------------------------------------------------------
// network plan
// ---------------------------------------------------------------------------
namespace {
inline int rup(int v, int m) { return (v + m - 1) / m * m; }

struct Plan {
  int kind, D, K, L, O, F;
  float w1, w, s;
  bool cplx, first_gemm, m3, x3, x2;
  int P, Pl, Din, Pin0, ldu, ntens, per_layer, Kp;
  // WIRE_KIND_BSPLINE_MS (kind then reads WIRE_KIND_BSPLINE, the activation of every layer behind the first stage): a frozen
  // first stage D -> SHF (its W0, b0 are tensors 0, 1) feeds layer 0, the GEMM SHF -> K; the plan's own tensors start at t0
  bool ms = false;
  int SHF = 0, T = 0, ms_split = 0, t0 = 0;
  float ms_c[WIRE_MS_MAX_SCALES] = {};
  // WIRE_KIND_BSPLINE_M2 (kind then reads WIRE_KIND_BSPLINE): the trunk runs S2 passes, pass k with c = m2_c[k] (s = the
  // pass-0 value), its rows at k n of buffers sized for S2 n rows; the combiner's four tensors come first (t0 = 4, the
  // trunk's native first layer at t0), their copy in the packed buffer at off_comb.  Every other kind: S2 = 1
  bool m2 = false;
  int S2 = 1;
  float m2_c[WIRE_MS_MAX_SCALES] = {};
  int64_t off_comb = -1;
  // WIRE_KIND_BSPLINE_HIER (kind then reads WIRE_KIND_BSPLINE): HS stages of the reference's HL hidden layers, stage s
  // with c = h_c[s].  Every K -> K GEMM of the net is a "hidden layer" of this plan (L of them, hier_v): stage 0's HL, then
  // per stage s >= 1 its layer 2 and the two halves of its join (packed for the join's two data-gradient GEMMs).  The
  // join's own forward image [P][2P] (all families), bias and max-|weight| slots sit at hj_*[s]; hj_half: the halves as
  // [K][K] matrices; h_nat: native copies of every first layer and head
  bool hier = false;
  int HS = 0, HL = 0;
  float h_c[WIRE_MS_MAX_SCALES] = {};
  int64_t hj_fwd[WIRE_MS_MAX_SCALES] = {}, hj_fwd_x3[WIRE_MS_MAX_SCALES] = {}, hj_fwd_x2[WIRE_MS_MAX_SCALES] = {},
          hj_bias[WIRE_MS_MAX_SCALES] = {}, hj_half[WIRE_MS_MAX_SCALES] = {}, hj_wamax = -1, h_nat = -1;
  // packed image offsets (floats); index l = 0..L (l = 0 only when first_gemm)
  std::vector<int64_t> off_fwd, off_dg, off_bias, off_fwd_x3, off_dg_x3, off_fwd_3m, off_dg_3m, off_fwd_x2, off_dg_x2;
  int64_t off_wf, off_bf, off_first, off_wamax, total_packed;   // off_wamax: max-|weight| slots, WIRE_AMAX_SLOTS per layer
  int64_t off_fx;    // k-permuted 2 x fp16 images of the hidden layers for the fused forward (wire_fused.hip), -1 = no such shape
  bool k_split_out, k_recompute_out, k_first_sums, k_rstore, k_wgrad_batch, k_fused_fwd, k_fused_train, k_fused_bwd, k_fused_final,
       k_fused_train_p384;
  int64_t off_fxd;   // the same of the TRANSPOSED weights of layers L .. 1 (in that order) for the data-gradient chain, -1 = none
  std::vector<int64_t> tfloats;
};

// params[] index of tensor q of the native first layer: the multi-scale net's frozen first stage is tensors 0, 1; the
// multi-pass net's first trunk layer follows the combiner (t0)
inline int first_tensor(const Plan& p, int q) { return p.ms ? q : p.t0 + q; }

// ---- the hierarchical net's index maps
inline int hier_last(const Plan& p, int st) { return st == 0 ? p.HL : 2; }           // index of stage st's last layer
inline int hier_t(const Plan& p, int st, int l) {                                     // params[] index of W of (st, l)
  return st == 0 ? 2 * l : 2 * (p.HL + 1) + 6 * (st - 1) + 2 * l;
}
inline int hier_th(const Plan& p, int st) { return 2 * (p.HL + 1) + 6 * (p.HS - 1) + 2 * st; }   // ... of head st's W
// the plan's hidden-layer index of a K -> K GEMM: stage 0 layer l; stage st >= 1: its layer 2, its join's halves
inline int hier_v(const Plan& p, int st, int l) { return st == 0 ? l : p.HL + 3 * (st - 1) + 1; }
inline int hier_vhalf(const Plan& p, int st, int half) { return p.HL + 3 * (st - 1) + 2 + half; }
inline int64_t hier_nat_stride(const Plan& p) {
  return rup(p.K * p.D, 4) + rup(p.K, 4) + rup(p.O * p.K, 4) + rup(p.O, 4);
}
struct HierNat { const float* W0; const float* b0; const float* Wh; const float* bh; };
inline HierNat hier_nat(const Plan& p, const float* packed, int st) {
  HierNat h;
  const float* c = packed + p.h_nat + (int64_t)st * hier_nat_stride(p);
  h.W0 = c; c += rup(p.K * p.D, 4);
  h.b0 = c; c += rup(p.K, 4);
  h.Wh = c; c += rup(p.O * p.K, 4);
  h.bh = c;
  return h;
}

int make_plan(const wire_net_desc* d, Plan& p) {
  if (!d) return fail(WIRE_ERR_ARG, "null descriptor");
  p.kind = d->kind; p.D = d->in_features; p.K = d->width; p.L = d->hidden_layers;
  p.O = d->out_features; p.F = d->posenc_freqs;
  p.w1 = d->first_omega0; p.w = d->hidden_omega0; p.s = d->scale0;
  if (p.kind < WIRE_KIND_WIRE || (p.kind > WIRE_KIND_BSPLINE_MS && p.kind != WIRE_KIND_BSPLINE_M2 &&
                                  p.kind != WIRE_KIND_BSPLINE_HIER))
    return fail(WIRE_ERR_ARG, "unknown kind %d", p.kind);
  if (p.kind == WIRE_KIND_BSPLINE_HIER) {
    // modules/bspline_mscale_hier.py: one stage per entry of scale_tensor, `scale` unused
    const wire_net_desc_ms* m = reinterpret_cast<const wire_net_desc_ms*>(d);
    if (m->first_width != 0) return fail(WIRE_ERR_ARG, "first_width %d: kind %d has no first stage", m->first_width,
                                         (int)WIRE_KIND_BSPLINE_HIER);
    p.HS = m->nscales;
    if (p.HS < 1 || p.HS > WIRE_MS_MAX_SCALES) return fail(WIRE_ERR_ARG, "nscales %d outside 1..%d", p.HS, WIRE_MS_MAX_SCALES);
    for (int k = 0; k < p.HS; ++k) {
      const float sk = m->scales[k];
      if (!(std::isfinite(sk) && sk != 0.f)) return fail(WIRE_ERR_ARG, "scales[%d] %g is zero or not finite", k, (double)sk);
      p.h_c[k] = (float)(1.0 / fabs((double)sk));
    }
    p.HL = p.L;
    if (p.HL < 1 || p.HL > 40) return fail(WIRE_ERR_ARG, "hidden_layers %d outside 1..40 (kind %d)", p.HL,
                                           (int)WIRE_KIND_BSPLINE_HIER);
    if (p.HL == 1 && p.HS > 1)
      return fail(WIRE_ERR_ARG, "hidden_layers 1 with %d scales: a later stage runs its layers 0, 1 and 2", p.HS);
    if (p.O >= 1 && p.O <= 8 && p.K >= 1 && p.K <= 4096 && (int64_t)p.O * rup(p.K, 64) > 16384)
      return fail(WIRE_ERR_ARG, "out_features %d x padded width %d > 16384 (kind %d)", p.O, rup(p.K, 64),
                  (int)WIRE_KIND_BSPLINE_HIER);
    p.hier = true;
    p.kind = WIRE_KIND_BSPLINE;
    p.s = m->scales[0];
    p.L = p.HL + 3 * (p.HS - 1);
  }
  if (p.kind == WIRE_KIND_BSPLINE_M2) {
    // modules/bspline_mscale_2.py: the trunk of bspline_form once per entry of scale_tensor (lin / scale_k), `scale` unused
    const wire_net_desc_ms* m = reinterpret_cast<const wire_net_desc_ms*>(d);
    if (m->first_width != 0) return fail(WIRE_ERR_ARG, "first_width %d: kind %d has no first stage", m->first_width,
                                         (int)WIRE_KIND_BSPLINE_M2);
    p.S2 = m->nscales;
    if (p.S2 < 1 || p.S2 > WIRE_MS_MAX_SCALES) return fail(WIRE_ERR_ARG, "nscales %d outside 1..%d", p.S2, WIRE_MS_MAX_SCALES);
    for (int k = 0; k < p.S2; ++k) {
      const float sk = m->scales[k];
      if (!(std::isfinite(sk) && sk != 0.f)) return fail(WIRE_ERR_ARG, "scales[%d] %g is zero or not finite", k, (double)sk);
      p.m2_c[k] = (float)(1.0 / fabs((double)sk));
    }
    p.m2 = true;
    p.kind = WIRE_KIND_BSPLINE;
    p.s = m->scales[0];
    p.t0 = 4;
  }
  if (p.kind == WIRE_KIND_BSPLINE_MS) {
    // modules/bspline_mscale_HL.py: columns [0, min(256, SHF)) divided by scale_tensor[0], group g >= 1 by scale_tensor[g]
    // over [256 + (g - 1) split, 256 + g split); the groups must cover SHF exactly (the next Linear takes SHF columns)
    const wire_net_desc_ms* m = reinterpret_cast<const wire_net_desc_ms*>(d);
    p.ms = true; p.SHF = m->first_width; p.T = m->nscales;
    if (p.SHF < 1 || p.SHF > 4096) return fail(WIRE_ERR_ARG, "first_width %d outside 1..4096", p.SHF);
    if (p.T < 2 || p.T > WIRE_MS_MAX_SCALES) return fail(WIRE_ERR_ARG, "nscales %d outside 2..%d", p.T, WIRE_MS_MAX_SCALES);
    if (p.SHF > 256) {
      p.ms_split = (p.SHF - 256) / (p.T - 1);
      if (p.ms_split < 1 || 256 + (p.T - 1) * p.ms_split != p.SHF)
        return fail(WIRE_ERR_ARG, "first_width %d is not 256 + %d equal column groups", p.SHF, p.T - 1);
    }
    for (int g = 0; g < p.T; ++g) {
      const float sg = m->scales[g];
      if (!(std::isfinite(sg) && sg != 0.f)) return fail(WIRE_ERR_ARG, "scales[%d] %g is zero or not finite", g, (double)sg);
      p.ms_c[g] = (float)(1.0 / fabs((double)sg));
    }
    if (p.L < 0 || p.L > 65) return fail(WIRE_ERR_ARG, "hidden_layers %d outside 0..65", p.L);
    p.L = p.L > 1 ? p.L - 1 : 0;   // K -> K layers behind the SHF -> K one (hidden_layers = 0 builds the net of 1)
    p.kind = WIRE_KIND_BSPLINE;
    p.t0 = 2;
  }
  if (p.kind == WIRE_KIND_BSPLINE) {
    // sigma0 divides lin (modules/bspline_form.py:44); B is even, so every kernel multiplies by c = 1 / |sigma0| instead
    if (!(std::isfinite(p.s) && p.s != 0.f)) return fail(WIRE_ERR_ARG, "bspline scale0 %g is zero or not finite", (double)p.s);
    p.s = (float)(1.0 / fabs((double)p.s));
  }
  if (p.D < 1 || p.D > 4) return fail(WIRE_ERR_ARG, "in_features %d outside 1..4", p.D);
  if (p.K < 1 || p.K > 4096) return fail(WIRE_ERR_ARG, "width %d outside 1..4096", p.K);
  if (p.L < 0 || p.L > 64) return fail(WIRE_ERR_ARG, "hidden_layers %d outside 0..64", p.L);
  if (p.O < 1 || p.O > 8) return fail(WIRE_ERR_ARG, "out_features %d outside 1..8", p.O);
  if (p.F < 0 || (p.F > 0 && p.kind != WIRE_KIND_RELU)) return fail(WIRE_ERR_ARG, "posenc only with relu");
  p.cplx = (p.kind == WIRE_KIND_WIRE || p.kind == WIRE_KIND_WIRE2D);
  p.P = p.cplx ? rup(2 * p.K, 64) : rup(p.K, 64);
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
  p.k_first_sums = knob(K_FIRST_SUMS) != 0; p.k_rstore = knob(K_FUSED_RSTORE) != 0; p.k_wgrad_batch = knob(K_WGRAD_BATCH) != 0;
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
  const bool fx_ok = !p.hier && p.L >= 1 && fused_fwd_shape(p.kind, p.P) &&
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

inline int64_t fx_hidden_off(const Plan& p) { return p.off_fx + (p.first_gemm ? (int64_t)p.P * p.Pin0 : 0); }
// the whole-net forward's hidden images of pass k (the multi-pass net; every other kind: k = 0) and that pass's c
inline int64_t fx_pass_off(const Plan& p, int k) { return fx_hidden_off(p) + (int64_t)k * p.L * fused_b_image_floats(p.P); }
inline float pass_c(const Plan& p, int k) { return p.m2 ? p.m2_c[k] : p.s; }
inline int64_t first_native_off(const Plan& p, int q) {
  int64_t off = p.off_first;
  for (int i = 0; i < q; ++i) off += rup((int)p.tfloats[first_tensor(p, i)], 4);
  return off;
}
// the combiner's weights in the packed buffer (the multi-pass net)
inline M2Comb comb_of(const Plan& p, const float* packed) {
  M2Comb w;
  const float* c = packed + p.off_comb;
  w.W1 = c; c += rup((int)p.tfloats[0], 4);
  w.b1 = c; c += rup((int)p.tfloats[1], 4);
  w.W2 = c; c += rup((int)p.tfloats[2], 4);
  w.b2 = c;
  return w;
}

// activation carve (floats)
struct ActLayout {
  int64_t pe, out0, lin0, lin1, total;   // out_l = out0 + l*np*P ; lin_l = lin1 + (l-1)*np*Pl
  int64_t ping, pong;                    // inference
  int64_t amax;                          // max |out_l| slots, WIRE_AMAX_SLOTS per layer l = 0..L (2 x fp16 GEMMs)
  int64_t pe_amax;                       // the multi-scale net: max |pe| slots right behind them (fp32 pe on 2 x fp16)
  int64_t ytr;                           // the multi-pass net: the trunk's outputs
  int64_t np;                            // rows each saved buffer is spaced by: n rounded up to 128 -- the fused training
                                         // forward (wire_fused.hip) stores whole 128-row workgroup tiles unconditionally
};
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
    a.lin0 = off; if (!p.cplx) off += a.np * p.P;
    a.lin1 = off; off += a.np * p.Pl * p.L;
  } else {
    a.ping = off; off += n * p.P;
    a.pong = off; off += n * p.P;
  }
  a.ytr = off; if (p.m2) off += n * p.O;     // the trunk's outputs [S2][n1][O], the combiner's input
  a.total = off;
  return a;
}

// (the multi-pass net: gtr = the combiner's gradient of the trunk's outputs [S2][n1][O], cpart = its weight-gradient
// partials, crep = the coordinates once per pass [S2][n1][D] for the first layer's sums over all rows)
struct ScratchLayout { int64_t ga, gb, gu, slab, bslab, fpw, fpb, crp, gamax, gch, gch_stride, gtr, cpart, crep, total; int S; };
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
  const int nbf = (p.off_fx >= 0 && !p.cplx ? 2 : 1) * p.S2 * final_bwd_blocks(n1) + 32;
  s.fpw = off; off += (int64_t)nbf * p.O * p.P;
  s.fpb = off; off += (int64_t)nbf * p.O + 64;
  // (wire2d: two sets, one per Linear of the first layer, when the data-gradient epilogue forms the sums itself)
  // (the data-gradient chain writes one block of first-layer sums per 64- or 128-row workgroup: 4 x the 256-row blocks)
  s.crp = off; off += (int64_t)((p.off_fxd >= 0 ? 4 : 1) * colreduce_blocks(n) + 32) * (p.cplx ? p.ldu : p.P) * 5 *
                      (p.kind == WIRE_KIND_WIRE2D ? 2 : 1);
  s.gtr = s.cpart = s.crep = off;
  if (p.m2) {
    s.gtr = off; off += n * p.O;
    s.cpart = off; off += (int64_t)m2_comb_blocks(n1) * m2_comb_grad_floats(p.S2, p.O) + M2_COMB_MAXBLK;   // + loss partials
    s.crep = off; off += n * p.D;
  }
  s.total = off;
  return s;
}

// coordinate-gradient scratch (wire_mlp_bwd_coords), behind the backward's own: the per-row partials of the layer-1
// data-gradient epilogue, one set per 128-column tile of that GEMM's output [tile][n][D], and positional-encoding nets'
// g_pe [n][Pin0]
struct CoordLayout { int64_t cgp, gpe, total; int ntiles; };
// (the multi-pass net: cgp holds the per-pass coordinate gradients [S2][n1][D] before their sum)
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

int epi_fwd(int kind) {
  switch (kind) {
    case WIRE_KIND_WIRE: return EPI_GABOR_FWD;
    case WIRE_KIND_WIRE2D: return EPI_GABOR2D_FWD;
    case WIRE_KIND_SIREN: return EPI_SIREN_FWD;
    case WIRE_KIND_GAUSS: return EPI_GAUSS_FWD;
    case WIRE_KIND_BSPLINE: return EPI_BSPLINE_FWD;
    default: return EPI_RELU_FWD;
  }
}
int epi_bwd(int kind) {
  switch (kind) {
    case WIRE_KIND_WIRE: return EPI_GABOR_BWD;
    case WIRE_KIND_WIRE2D: return EPI_GABOR2D_BWD;
    case WIRE_KIND_SIREN: return EPI_SIREN_BWD;
    case WIRE_KIND_GAUSS: return EPI_GAUSS_BWD;
    case WIRE_KIND_BSPLINE: return EPI_BSPLINE_BWD;
    default: return EPI_RELU_BWD;
  }
}

// ---------------------------------------------------------------------------
// route: what one whole-net call runs, decided once from (plan, n, entry point)
// ---------------------------------------------------------------------------
// wire_mlp_fwd with save_for_bwd = 0; wire_mlp_fwd with save_for_bwd = 1, wire_mlp_bwd[_coords]; wire_train_fwd_bwd[_hooked]
enum RouteMode { MODE_INFER, MODE_AUTOGRAD, MODE_TRAIN };
struct Route {
  RouteMode mode;
  WireFamily fam;         // forward and data-gradient GEMMs of the hidden layers
  WireFamily fam0;        // GEMMs of a positional-encoding first layer: 3 x bf16 or fp32 (the multi-scale net's SHF -> K
                          //   forward: 2 x fp16 with the hidden layers)
  WireFamily tn0;         // the multi-scale net: weight gradient of its SHF -> K layer
  float pe_split;         //   ... and the fixed split scale of its first-stage map pe when both read it pre-split, 0 = fp32
  WireFamily tn_fam;      // weight-gradient GEMMs of the hidden layers, in tn_S row splits
  int tn_S;
  bool fused_fwd;         // inference: the whole net in one kernel, activations in registers (wire_fused.hip)
  bool fuse;              // train: final linear + MSE + final backward + activation gradient of layer L in one pass
  bool fused_train;       // train: the hidden layers in one kernel that stores what the backward reads (wire_fused.hip)
  bool fused_final;       //   ... with the final stage inside it (fx_tail_loss): lin_L / out_L are not stored at all
  bool chain;             // the data gradients of layers L .. 1 in one kernel (wire_fused.hip: fused_bwd_kernel)
  bool rstore;            //   ... sine / Gaussian / B-spline: lin_l (l < L) stored as r = c lin, out_l (l < L) not at all
  bool skip_out_L;        // train: out_L is neither written nor read, the final stage evaluates it from lin_L
  bool recompute_out;     // the data-gradient epilogue of layer l >= 2 evaluates out_{l-1} = act(lin_{l-1}) again
  bool recompute_out0;    //   ... and wire's first-layer epilogue out_0 (first_fwd_kernel's own form, the same bits)
  bool first_sums;        // the layer-1 data-gradient epilogue sums the first layer's weight / bias gradient itself
  bool cg_epi;            //   ... and can form the per-row coordinate-gradient partials
  int wb_l0, wb_n, wb_S;  // weight-gradient batch: layers wb_l0 .. L, wb_n members of wb_S splits (wb_l0 = L + 1: none)
  float act_scale;        // split scale of the fused forward's activations, 0 = none known
  float out_scale[65];    // pre-split scale of out_l, l = 0 .. L (L <= 64); 0 = plain fp32
};

// Power-of-two split scale of activations with an a-priori bound (bound < 2^e -> 2^(15 - e): |out| scale < 2^15): sine
// and Gaussian <= 1; Gabor |exp(j w lin - s^2 |lin|^2)| = exp(-w v - s^2 (u^2 + v^2)) <= exp((w / 2s)^2), attained at
// lin = -j w / 2 s^2 -- accepted up to 16 (w / s <= 3.33: every configuration of the reference's scripts); 0 beyond it
float act_bound_scale(const Plan& p) {
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
  r.rstore = r.chain && r.fused_train && p.k_rstore &&
             (p.kind == WIRE_KIND_SIREN || p.kind == WIRE_KIND_GAUSS || p.kind == WIRE_KIND_BSPLINE);   // 1.3 GB per step less
  // out_l is stored pre-split (wire_dev.h: wire_store_out4) when the call runs the 2 x fp16 kernels and every reader of
  // out_l understands the format: the forward GEMM of layer l + 1 (pre-split A edition), the weight-gradient GEMM of layer
  // l + 1 (gemmx2_tn16, pre-split Z) and NOTHING else -- the data-gradient epilogue of layer l + 1 must evaluate
  // act(lin_l) again rather than read out_l (recompute_out; sine and B-spline need no out), out_0 comes from first_fwd_kernel, out_L
  // feeds the final linear layer in fp32, relu's out carries its backward's sign decisions
  const bool split = x2tn && p.k_split_out && p.kind != WIRE_KIND_RELU &&
                     (p.k_recompute_out || p.kind == WIRE_KIND_SIREN || p.kind == WIRE_KIND_BSPLINE);
  for (int l = 1; l < p.L; ++l) r.out_scale[l] = !split ? 0.f : ftrain ? 1.f : act_bound_scale(p);
  // the layer-1 data gradient of a native first layer on the 16 x 16 x 32 kernel: its epilogue can sum g_lin_0 (wire:
  // g_u) [x | 1] per tile itself instead of storing it for a separate pass, and form the coordinate-gradient partials
  const int epi1 = p.kind == WIRE_KIND_WIRE ? EPI_GABOR_BWD_FIRST
                 : p.kind == WIRE_KIND_WIRE2D ? EPI_GABOR2D_BWD_FIRST : epi_bwd(p.kind);
  const bool h16_1 = p.x3 && gemmx3_nt_is_h16(epi1, n);
  // (the multi-pass net: its layer-1 data gradient runs once per pass, its first-layer sums over all passes at once)
  r.cg_epi = h16_1 && !p.first_gemm && p.L >= 1 && !p.m2;
  r.first_sums = r.cg_epi && p.k_first_sums;
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

inline const unsigned* wamax_of(const Plan& p, const float* packed, int l) {   // max |W_l| slots
  return reinterpret_cast<const unsigned*>(packed + p.off_wamax + (int64_t)l * WIRE_AMAX_SLOTS);
}
// C = A W_l^T (the forward of layer l) or, dg, A W_l (its data gradient) on family f, from f's image of layer l.  The
// 2 x fp16 kernels also take the maximum slots of A, of W_l and of the tensor the epilogue writes (null: none kept)
hipError_t layer_nt(hipStream_t s, const Plan& p, WireFamily f, const float* packed, int l, bool dg, int epi,
                    const float* A, int64_t n, GemmEpiParams ep, const unsigned* amax_a = nullptr,
                    const unsigned* amax_b = nullptr, unsigned* amax_out = nullptr) {
  const int Pin = l == 0 ? p.Pin0 : p.P, Nc = dg ? Pin : p.Pl, Kd = dg ? p.Pl : Pin;
  switch (f) {
    case FAM_X2:
      ep.amax_a = amax_a; ep.amax_b = amax_b; ep.amax_out = amax_out;
      return launch_gemmx2h_nt(s, epi, A, Kd, packed + (dg ? p.off_dg_x2 : p.off_fwd_x2)[l], n, Nc, Kd, ep);
    case FAM_3M:
      return launch_gemm3m_nt(s, epi, A, Kd, packed + (dg ? p.off_dg_3m : p.off_fwd_3m)[l], Kd, n, Nc / 2, Kd / 2, ep);
    case FAM_X3: return launch_gemmx3_nt(s, epi, A, Kd, packed + (dg ? p.off_dg_x3 : p.off_fwd_x3)[l], n, Nc, Kd, ep);
    default: return launch_gemm_nt(s, epi, A, Kd, packed + (dg ? p.off_dg : p.off_fwd)[l], Kd, n, Nc, Kd, ep);
  }
}
}  // namespace

// ---------------------------------------------------------------------------
// size queries
// ---------------------------------------------------------------------------
static int64_t hier_act_total(const Plan& p, int64_t n, int save);          // the hierarchical net's layouts, below
static int64_t hier_scratch_total(const Plan& p, int64_t n, bool coords);
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
  if (p.hier) return hier_act_total(p, n, save_for_bwd) * 4 + 256;
  return act_layout(p, n, save_for_bwd).total * 4 + 256;
}
extern "C" int64_t wire_bwd_scratch_bytes(const wire_net_desc* d, int64_t n) {
  Plan p; if (make_plan(d, p)) return WIRE_ERR_ARG;
  if (n < 0) return fail(WIRE_ERR_ARG, "negative n");
  if (p.hier) return hier_scratch_total(p, n, false) * 4 + 256;
  return scratch_layout(p, n).total * 4 + 256;
}
extern "C" int64_t wire_bwd_coords_scratch_bytes(const wire_net_desc* d, int64_t n) {
  Plan p; if (make_plan(d, p)) return WIRE_ERR_ARG;
  if (n < 0) return fail(WIRE_ERR_ARG, "negative n");
  if (p.hier) return hier_scratch_total(p, n, true) * 4 + 256;
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

// ---------------------------------------------------------------------------
// pack
// ---------------------------------------------------------------------------
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
  // W, b of the plan's hidden layer l (the hierarchical net: the K -> K GEMMs of every stage, hier_v / hier_vhalf)
  std::vector<const float*> hW(p.L + 1, nullptr), hb(p.L + 1, nullptr);
  for (int l = 1; l <= p.L && !p.hier; ++l) {
    hW[l] = (const float*)params[p.t0 + p.per_layer * l]; hb[l] = (const float*)params[p.t0 + p.per_layer * l + 1];
  }
  if (p.hier) {
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
  }
  // hidden layers share one shape: every family's image of up to PACK_MAXB layers per launch (3 - 4 launches per step
  // instead of 4 per layer; this runs once per optimizer step and is all launch gaps)
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
    HIPCHK(launch_pack_hidden_batch(s, p.kind, pb, nb, p.K, p.K, p.P, p.P));
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
  if (p.hier) {                // every stage's first layer and head, read in their native layout
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
  HIPCHK(launch_pack_final(s, p.kind, (const float*)params[p.ntens - 2],
                           (const float*)params[p.ntens - 1], p.K, p.P, p.O, packed + p.off_wf,
                           packed + p.off_bf));
  if (!p.first_gemm || p.ms)   // (the multi-scale net: its first stage, read by mscale_first_kernel)
    for (int q = 0; q < p.per_layer; ++q)
      HIPCHK(hipMemcpyAsync(packed + first_native_off(p, q), params[first_tensor(p, q)], p.tfloats[first_tensor(p, q)] * 4,
                            hipMemcpyDeviceToDevice, s));
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
        f.s = p.m2_c[k];
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
    for (int g = 0; g < p.T; ++g) c.c[g] = p.ms_c[g];
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
  // the multi-pass net: the trunk once per pass k with c = m2_c[k], its rows at k n of every buffer (every other kind:
  // one pass, offset 0, c = s); the maxima of the 2 x fp16 kernels gather over the passes (slots zeroed once above)
  auto at = [](float* b, int64_t off) -> float* { return b ? b + off : nullptr; };
  for (int k = 0; k < p.S2; ++k) {
    const float ck = p.m2 ? p.m2_c[k] : p.s;
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

static int hier_fwd_dispatch(void* stream, const Plan& p, const float* packed, const float* coords, int64_t n, float* y,
                             void* act, int64_t act_bytes, int save_for_bwd);   // the hierarchical net, below
extern "C" int wire_mlp_fwd(void* stream, const wire_net_desc* d, const float* packed,
                            const float* coords, int64_t n, float* y, void* act, int64_t act_bytes,
                            int save_for_bwd) {
  Plan p; if (int rc = make_plan(d, p)) return rc;
  if (p.hier) return hier_fwd_dispatch(stream, p, packed, coords, n, y, act, act_bytes, save_for_bwd);
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
  int64_t crp_set() const { return (int64_t)(colreduce_blocks(n) + 32) * p.ldu * 5; }   // wire2d: the second set of sums
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
                                out_l(p.L) + ro * p.P, p.K, p.P, wL, p.m2 ? p.m2_c[k] : p.s, gcur + ro * p.P,
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
      b.s = p.m2_c[k]; b.c_hidden = fused_pre_scale(p.kind, p.w, p.m2_c[k]);
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

// the weight-gradient loader's form of Z = act(r) under rstore (launch_gemmx2_tn, z_act): sine 2, Gaussian 3, B-spline 4
static int rstore_zmode(int kind) { return kind == WIRE_KIND_SIREN ? 2 : kind == WIRE_KIND_GAUSS ? 3 : 4; }

// 4. the weight-gradient batch of layers wb_l0 .. L (make_route), behind the chain
int Bwd::wgrad_batch() {
  const int l0 = r.wb_l0, nb = r.wb_n;
  const bool rs = r.rstore;
  const float s_z = rs ? 0.f : r.out_scale[l0 - 1];
  ProfScope ps(s, 2, 2.0 * n * p.Pl * p.P * nb);
  HIPCHK(launch_gemmx2_tn(s, Sx + sc.gch + l0 * sc.gch_stride, p.Pl, rs ? lin_l(l0 - 1) : out_l(l0 - 1), rs ? p.Pl : p.P,
                          n, p.Pl, p.P, r.wb_S, Sx + sc.slab, Sx + sc.bslab, gslots(l0), oslots(l0 - 1),
                          rs ? 1.f / 16384.f : (s_z != 0.f ? 1.f / s_z : 0.f), rs ? rstore_zmode(p.kind) : 0,
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
                                1.f / 16384.f, rstore_zmode(p.kind));
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
        HIPCHK(launch_wgrad_reduce(s, p.kind, slab, bslab, S, p.K, p.K, p.Pl, p.P, g(0), g(1), g(2), g(3)));
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
      // (real nets: the layer-1 epilogue sums g_lin_0 [x | 1] itself)
      if (l == 1 && first_sums) { ep.coords = coords; ep.D = p.D; ep.cr_partial = Sx + sc.crp; ep.cr_C = p.K; }
    } else {
      epi = (p.kind == WIRE_KIND_WIRE) ? EPI_GABOR_BWD_FIRST : EPI_GABOR2D_BWD_FIRST;
      ep.omega = p.w1;
      ep.coords = coords; ep.D = p.D; ep.ldu = p.ldu; ep.o0 = Sx + sc.gu;
      // (wire, wire2d: g_u [x | 1] per 256-row tile instead of storing g_u for a separate pass)
      if (first_sums) { ep.cr_partial = Sx + sc.crp; ep.cr_C = p.K; ep.cr_set = crp_set(); }
      ep.recompute_out = r.recompute_out0;
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
      if (k > 0) { e.scale = p.m2_c[k]; e.i0 += ro * p.Pl; e.i1 += ro * p.P; e.o0 += ro * e.ld0; }
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
                                         grad(p.t0 + 1)));
  } else if (!p.first_gemm && r.first_sums) {
    HIPCHK(launch_colreduce_final(s, p.K, p.D, n, crp, grad(0), grad(1)));
  } else if (!p.first_gemm) {   // (the multi-pass net: coords = the per-pass copies, n = all passes' rows)
    HIPCHK(launch_colreduce(s, gcur, p.P, p.K, coords, p.D, n, crp, grad(p.t0), grad(p.t0 + 1)));   // gcur: g_lin_0 [n][P]
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


// ---------------------------------------------------------------------------
// the hierarchical B-spline net (WIRE_KIND_BSPLINE_HIER): layer by layer in every mode
// ---------------------------------------------------------------------------
namespace {
// where a layer's activation goes: rows of ld floats (P, or 2P inside a join's input), aset = the max-|value| slot set
// its 2 x fp16 reader scales by (-1: no GEMM reads it)
struct HierOut { int64_t off; int ld; int aset; };
struct HierAct {
  int64_t amax, total;
  std::vector<std::vector<int64_t>> lin;   // [stage][layer]; -1 = not stored (inference)
  std::vector<std::vector<HierOut>> out;   // [stage][layer]
  std::vector<int64_t> cat;                // [stage >= 1]: the join's input [n][2P] = [x_in | x_{stage-1}]
};
inline int hier_sets(const Plan& p) { return p.HS * (p.HL + 2); }
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

// three g buffers [n][P] (the current layer's g_lin, the next one's, and T = the join's right-half gradient on its way to
// the previous stage's head backward), slabs for the widest weight gradient ([P][2P] with a join), the heads' and the
// first layers' pre-reduction blocks, the loss partials; cgp (behind everything, wire_bwd_coords_scratch_bytes): the
// per-stage coordinate gradients before their sum
struct HierScratch { int64_t gamax, g[3], slab, bslab, fpw, fpb, crp, lpart, total, cgp, total_coords; int S; };
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
  const int nbf = final_bwd_blocks(n) + 32;
  s.fpw = off; off += (int64_t)nbf * p.O * p.P;
  s.fpb = off; off += (int64_t)nbf * p.O + 64;
  s.crp = off; off += (int64_t)(colreduce_blocks(n) + 32) * p.P * 5;
  s.lpart = off; off += HIER_HEAD_MAXBLK;
  s.total = off;
  off = (off + 63) / 64 * 64;
  s.cgp = off; off += (int64_t)p.HS * n * p.D;
  s.total_coords = off;
  return s;
}

// the join's forward GEMM [n][2P] x [P][2P]^T on family f
hipError_t hier_join_nt(hipStream_t s, const Plan& p, WireFamily f, const float* packed, int st, const float* A, int64_t n,
                        GemmEpiParams ep, const unsigned* amax_a, unsigned* amax_out) {
  const int Kd = 2 * p.P, Nc = p.P;
  switch (f) {
    case FAM_X2:
      ep.amax_a = amax_a; ep.amax_out = amax_out;
      ep.amax_b = reinterpret_cast<const unsigned*>(packed + p.hj_wamax) + st * WIRE_AMAX_SLOTS;
      return launch_gemmx2h_nt(s, EPI_BSPLINE_FWD, A, Kd, packed + p.hj_fwd_x2[st], n, Nc, Kd, ep);
    case FAM_X3: return launch_gemmx3_nt(s, EPI_BSPLINE_FWD, A, Kd, packed + p.hj_fwd_x3[st], n, Nc, Kd, ep);
    default: return launch_gemm_nt(s, EPI_BSPLINE_FWD, A, Kd, packed + p.hj_fwd[st], Kd, n, Nc, Kd, ep);
  }
}
// slabs of G^T [Z | 1], G [n][P], Z [n][Pn] rows of ldz floats, on family f in S splits
hipError_t hier_tn(hipStream_t s, const Plan& p, WireFamily f, const float* G, const float* Z, int ldz, int Pn, int64_t n,
                   int S, float* slab, float* bslab, const unsigned* amax_g, const unsigned* amax_z) {
  switch (f) {
    case FAM_X2: return launch_gemmx2_tn(s, G, p.P, Z, ldz, n, p.P, Pn, S, slab, bslab, amax_g, amax_z);
    case FAM_X3: return launch_gemmx3_tn(s, G, p.P, Z, ldz, n, p.P, Pn, S, slab, bslab);
    default: return launch_gemm_tn(s, G, p.P, Z, ldz, n, p.P, Pn, S, slab, bslab);
  }
}
int hier_tn_splits(WireFamily f, int64_t n, int Pm, int Pn, int cap) {
  const int S = f == FAM_X2 ? gemmx2_tn_splits(n, Pm, Pn, cap) : f == FAM_X3 ? gemmx3_tn_splits(n, Pm, Pn, cap)
                                                                             : gemm_tn_splits(n, Pm, Pn, cap);
  return S < 1 ? 1 : S;
}

// forward.  loss (training): the last head's launch forms the MSE terms, g_y and the loss partials
int hier_fwd_core(void* stream, const Plan& p, const Route& r, const float* packed, const float* coords, int64_t n, float* y,
                  void* act, int64_t act_bytes, const M2Loss* loss = nullptr, float* loss_part = nullptr) {
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
    const float c = p.h_c[st];
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
                                  p.h_c[st], nullptr, Sx + sc.fpw, Sx + sc.fpb, nullptr));
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
    const float c = p.h_c[st];
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
        ep.scale = p.h_c[st - 1]; ep.i0 = A + a.lin[st - 1][hier_last(p, st - 1)]; ep.o0 = T;
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
  r.first_sums = r.cg_epi = false;
  r.wb_l0 = p.L + 1; r.wb_n = 0;
  for (float& v : r.out_scale) v = 0.f;
  return r;
}
}  // namespace

static int64_t hier_act_total(const Plan& p, int64_t n, int save) { return hier_act(p, n, save).total; }
static int64_t hier_scratch_total(const Plan& p, int64_t n, bool coords) {
  const HierScratch s = hier_scratch(p, n);
  return coords ? s.total_coords : s.total;
}
static int hier_fwd_dispatch(void* stream, const Plan& p, const float* packed, const float* coords, int64_t n, float* y,
                             void* act, int64_t act_bytes, int save_for_bwd) {
  return hier_fwd_core(stream, p, hier_route(p, n, save_for_bwd ? MODE_AUTOGRAD : MODE_INFER), packed, coords, n, y, act,
                       act_bytes);
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

// ---------------------------------------------------------------------------
// training glue
// ---------------------------------------------------------------------------
extern "C" int wire_coords_from_index(void* stream, const int64_t* idx, int64_t first, int64_t n,
                                      const float* tx, int W, const float* ty, int H,
                                      const float* tz, int T, float* coords) {
  if (n < 0 || !tx || !ty || !coords || W < 1 || H < 1 || (tz && T < 1))
    return fail(WIRE_ERR_ARG, "bad argument to wire_coords_from_index");
  ProfScope ps((hipStream_t)stream, 3, 0);
  HIPCHK(launch_coords((hipStream_t)stream, idx, first, n, tx, W, ty, H, tz, T, coords));
  return WIRE_OK;
}
extern "C" int wire_perm_indices(void* stream, uint64_t seed, int64_t n_total, int64_t first, int64_t count,
                                 int64_t* idx_out) {
  if (n_total < 1 || first < 0 || count < 0 || first + count > n_total || (count > 0 && !idx_out))
    return fail(WIRE_ERR_ARG, "bad argument to wire_perm_indices");
  ProfScope ps((hipStream_t)stream, 3, 0);
  HIPCHK(launch_perm_indices((hipStream_t)stream, seed, n_total, first, count, idx_out));
  return WIRE_OK;
}
extern "C" int wire_mse_grad(void* stream, const float* y, const float* target, const int64_t* idx,
                             int64_t first, int64_t n, int O, float weight, float* g_y,
                             float* loss_out, float* rec, float* partial) {
  if (n < 0 || O < 1 || !y || !target || !g_y || !loss_out || !partial)
    return fail(WIRE_ERR_ARG, "bad argument to wire_mse_grad");
  ProfScope ps((hipStream_t)stream, 3, 0);
  HIPCHK(launch_mse_grad((hipStream_t)stream, y, target, idx, first, n, O, weight, g_y, loss_out,
                         rec, partial));
  return WIRE_OK;
}
extern "C" int wire_avgpool_mse_grad(void* stream, const float* y, int H, int W, int O, int scale,
                                     const float* gt_lr, float* g_y, float* rec_lr, float* loss_out,
                                     float* partial) {
  if (H < 1 || W < 1 || O < 1 || scale < 1 || scale > H || scale > W || !y || !gt_lr || !g_y || !loss_out || !partial)
    return fail(WIRE_ERR_ARG, "bad argument to wire_avgpool_mse_grad");
  ProfScope ps((hipStream_t)stream, 3, 0);
  HIPCHK(launch_avgpool_mse_grad((hipStream_t)stream, y, H, W, O, scale, gt_lr, g_y, rec_lr, loss_out, partial));
  return WIRE_OK;
}
extern "C" int wire_adam_step_flat(void* stream, float* param, const float* grad, float* exp_avg,
                                   float* exp_avg_sq, int64_t count, float lr, float beta1,
                                   float beta2, float eps, int64_t step) {
  if (count < 0 || step < 1 || !param || !grad || !exp_avg || !exp_avg_sq)
    return fail(WIRE_ERR_ARG, "bad argument to wire_adam_step_flat");
  const double bc1 = 1.0 - std::pow((double)beta1, (double)step);
  const double bc2 = 1.0 - std::pow((double)beta2, (double)step);
  ProfScope ps((hipStream_t)stream, 3, 0);
  HIPCHK(launch_adam((hipStream_t)stream, param, grad, exp_avg, exp_avg_sq, count,
                     (float)((double)lr / bc1), beta1, beta2, eps, (float)(1.0 / std::sqrt(bc2))));
  return WIRE_OK;
}

extern "C" int wire_eval_metric(void* stream, int mode, const float* rec, const float* gt, int64_t count,
                                float thres, float* out2, float* partial) {
  if ((mode != 0 && mode != 1) || count < 1 || !rec || !gt || !out2 || !partial)
    return fail(WIRE_ERR_ARG, "bad argument to wire_eval_metric");
  ProfScope ps((hipStream_t)stream, 3, 0);
  HIPCHK(launch_metric((hipStream_t)stream, mode, rec, gt, count, thres, out2, partial));
  return WIRE_OK;
}

extern "C" int wire_track_best(void* stream, const float* metric, float* best_metric, int force, const float* src,
                               float* dst, int64_t count, int* updated) {
  if (!metric || !best_metric || count < 0 || (count > 0 && (!src || !dst)))
    return fail(WIRE_ERR_ARG, "bad argument to wire_track_best");
  if (count > 0 && (((uintptr_t)src | (uintptr_t)dst) & 15)) return fail(WIRE_ERR_ARG, "src / dst must be 16-byte aligned");
  ProfScope ps((hipStream_t)stream, 3, 0);
  HIPCHK(launch_track_best((hipStream_t)stream, metric, best_metric, force, src, dst, count, updated));
  return WIRE_OK;
}
extern "C" int wire_radon_fwd(void* stream, const float* img, const float* angles_deg, int H, int W, int nangles,
                              float* sino) {
  if (H < 1 || W < 1 || nangles < 1 || !img || !angles_deg || !sino) return fail(WIRE_ERR_ARG, "bad argument to wire_radon_fwd");
  ProfScope ps((hipStream_t)stream, 3, 0);
  HIPCHK(launch_radon_fwd((hipStream_t)stream, img, angles_deg, H, W, nangles, sino));
  return WIRE_OK;
}
extern "C" int wire_radon_bwd(void* stream, const float* g_sino, const float* angles_deg, int H, int W, int nangles,
                              float* g_img) {
  if (H < 1 || W < 1 || nangles < 1 || !g_sino || !angles_deg || !g_img) return fail(WIRE_ERR_ARG, "bad argument to wire_radon_bwd");
  ProfScope ps((hipStream_t)stream, 3, 0);
  HIPCHK(launch_radon_bwd((hipStream_t)stream, g_sino, angles_deg, H, W, nangles, g_img));
  return WIRE_OK;
}
extern "C" int wire_mscale_first_fwd(void* stream, const float* x, const float* W, const float* b, int64_t n,
                                     int in_features, int out_features, int nscales, const float* scales_host, float* out) {
  if (n < 0 || in_features < 1 || in_features > 4 || (n > 0 && (!x || !W || !b || !out)) || !scales_host)
    return fail(WIRE_ERR_ARG, "bad argument to wire_mscale_first_fwd");
  // the descriptor's checks of the first stage (make_plan), on a net around it
  wire_net_desc_ms m{};
  m.base.kind = WIRE_KIND_BSPLINE_MS; m.base.in_features = in_features; m.base.width = 1; m.base.out_features = 1;
  m.base.scale0 = 1.f; m.first_width = out_features; m.nscales = nscales;
  if (nscales >= 2 && nscales <= WIRE_MS_MAX_SCALES)
    for (int g = 0; g < nscales; ++g) m.scales[g] = scales_host[g];
  Plan p; if (int rc = make_plan(&m.base, p)) return rc;
  MscaleC c{};
  for (int g = 0; g < p.T; ++g) c.c[g] = p.ms_c[g];
  HIPCHK(launch_mscale_first((hipStream_t)stream, x, n, in_features, W, b, p.SHF, c, p.ms_split, p.SHF, 0.f, nullptr, out));
  return WIRE_OK;
}
static bool m2_shape_ok(int S, int O) { return S >= 1 && S <= WIRE_MS_MAX_SCALES && O >= 1 && O <= 8; }
extern "C" int wire_m2_combine_fwd(void* stream, int nscales, int out_features, const float* W1, const float* b1,
                                   const float* W2, const float* b2, const float* t, int64_t n, float* y) {
  if (!m2_shape_ok(nscales, out_features) || n < 0 || !W1 || !b1 || !W2 || !b2 || (n > 0 && (!t || !y)))
    return fail(WIRE_ERR_ARG, "bad argument to wire_m2_combine_fwd");
  ProfScope ps((hipStream_t)stream, 3, 0);
  HIPCHK(launch_m2_comb_fwd((hipStream_t)stream, M2Comb{W1, b1, W2, b2}, nscales, out_features, t, n, y));
  return WIRE_OK;
}
extern "C" int64_t wire_m2_combine_ws_bytes(int nscales, int out_features, int64_t n) {
  if (!m2_shape_ok(nscales, out_features) || n < 0) return fail(WIRE_ERR_ARG, "bad argument to wire_m2_combine_ws_bytes");
  return (int64_t)m2_comb_blocks(n) * m2_comb_grad_floats(nscales, out_features) * 4 + 256;
}
extern "C" int wire_m2_combine_bwd(void* stream, int nscales, int out_features, const float* W1, const float* b1,
                                   const float* W2, const float* b2, const float* t, int64_t n, const float* g_y,
                                   float* g_t, float* gW1, float* gb1, float* gW2, float* gb2, void* ws,
                                   int64_t ws_bytes) {
  if (!m2_shape_ok(nscales, out_features) || n < 1 || !W1 || !b1 || !W2 || !b2 || !t || !g_y || !g_t || !gW1 || !gb1 ||
      !gW2 || !gb2 || !ws)
    return fail(WIRE_ERR_ARG, "bad argument to wire_m2_combine_bwd");
  if (ws_bytes < wire_m2_combine_ws_bytes(nscales, out_features, n)) return fail(WIRE_ERR_SIZE, "ws too small");
  hipStream_t s = (hipStream_t)stream;
  ProfScope ps(s, 3, 0);
  const M2Comb w{W1, b1, W2, b2};
  HIPCHK(launch_m2_comb_bwd(s, w, nscales, out_features, t, n, M2Loss{}, g_y, g_t, (float*)ws, nullptr));
  HIPCHK(launch_m2_comb_reduce(s, (const float*)ws, n, nscales, out_features, M2Grads{gW1, gb1, gW2, gb2}));
  return WIRE_OK;
}
extern "C" int wire_posenc_fwd(void* stream, const float* coords, int64_t n, int D, int F, float* out) {
  if (n < 0 || D < 1 || D > 4 || F < 0 || F > 30 || (n > 0 && (!coords || !out)))
    return fail(WIRE_ERR_ARG, "bad argument to wire_posenc_fwd");
  HIPCHK(launch_posenc((hipStream_t)stream, coords, n, D, F, D + 2 * D * F, out));
  return WIRE_OK;
}
extern "C" int wire_posenc_bwd(void* stream, const float* coords, int64_t n, int D, int F, const float* g_pe,
                               float* g_coords) {
  if (n < 0 || D < 1 || D > 4 || F < 0 || F > 30 || (n > 0 && (!coords || !g_pe || !g_coords)))
    return fail(WIRE_ERR_ARG, "bad argument to wire_posenc_bwd");
  ProfScope ps((hipStream_t)stream, 3, 0);
  HIPCHK(launch_posenc_bwd((hipStream_t)stream, coords, n, D, F, g_pe, D + 2 * D * F, g_coords));
  return WIRE_OK;
}
extern "C" int wire_sigmoid_inplace(void* stream, float* x, int64_t count) {
  if (count < 0 || (count > 0 && !x)) return fail(WIRE_ERR_ARG, "bad argument to wire_sigmoid_inplace");
  HIPCHK(launch_sigmoid((hipStream_t)stream, x, count));
  return WIRE_OK;
}

// ---------------------------------------------------------------------------
// layout helpers
// ---------------------------------------------------------------------------
extern "C" int wire_c64_to_blocked(void* stream, const void* src, int64_t n, int K, float* dst) {
  if (n < 0 || K < 1 || !src || !dst) return fail(WIRE_ERR_ARG, "bad argument");
  HIPCHK(launch_c64_to_blocked((hipStream_t)stream, (const float*)src, n, K, rup(2 * K, 64), dst));
  return WIRE_OK;
}
extern "C" int wire_blocked_to_c64(void* stream, const float* src, int64_t n, int K, void* dst) {
  if (n < 0 || K < 1 || !src || !dst) return fail(WIRE_ERR_ARG, "bad argument");
  HIPCHK(launch_blocked_to_c64((hipStream_t)stream, src, n, K, rup(2 * K, 64), (float*)dst));
  return WIRE_OK;
}
