// wire_plan.h -- internal to the host layer (not installed): what wire_plan.hip, wire_api.hip, wire_hier_api.hip,
// wire_mfn_api.hip, wire_misc_api.hip, wire_layer_api.hip and wire_tv.hip share -- the error channel, the profiler's scope, the plan of a net, its
// buffer layouts and the route of a whole-net call.
#pragma once
#include <hip/hip_runtime.h>

#include <atomic>
#include <mutex>
#include <utility>
#include <vector>

#include "../../include/wire_hip.h"
#include "wire_gemm.h"
#include "wire_point.h"

#ifndef WIRE_AMAX_SLOTS
#define WIRE_AMAX_SLOTS 64            // wire_dev.h (device header): sharded max-|value| slots per operand tensor
#endif

// ---------------------------------------------------------------------------
// error plumbing (wire_api.hip holds the thread's message behind wire_last_error)
// ---------------------------------------------------------------------------
int fail(int code, const char* fmt, ...);
int wire_fail_(int code, const char* msg);
#define HIPCHK(expr)                                                                   \
  do {                                                                                 \
    hipError_t e_ = (expr);                                                            \
    if (e_ != hipSuccess)                                                              \
      return fail(WIRE_ERR_HIP, "%s failed: %s (%s:%d)", #expr, hipGetErrorString(e_), \
                  __FILE__, __LINE__);                                                 \
  } while (0)

// ---------------------------------------------------------------------------
// profiling hooks (state: wire_api.hip, read by wire_prof_read)
// ---------------------------------------------------------------------------
struct ProfRec { hipEvent_t a, b; int cls; double flops; };
extern std::mutex g_prof_mu;
extern std::atomic<bool> g_prof_on;
extern std::vector<ProfRec> g_prof_recs;
extern std::vector<std::pair<hipEvent_t, hipEvent_t>> g_prof_pool;

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

// ---------------------------------------------------------------------------
// network plan (wire_plan.hip)
// ---------------------------------------------------------------------------
inline int rup(int v, int m) { return (v + m - 1) / m * m; }

struct Plan {
  int kind, D, K, L, O, F;
  float w1, w, s;
  // WIRE_KIND_BSPLINE_CUBIC: scale0 multiplies every activation layer's INPUT (lin = ws x W^T + b).  It lives in the packed
  // weights alone: wire_pack_params writes ws W into every image of the hidden layers and into the first layer's native
  // copy (forward, data gradient and coordinate gradient read ws W; the maxima the split GEMMs scale by are taken of
  // ws W), the bias stays as it is, the weight-gradient reductions multiply g_W by ws on the way out, and the kernels'
  // own scale s is 1.  Every other kind: ws = 1, nothing is multiplied
  float ws = 1.f;
  bool cplx, first_gemm, m3, x3, x2;
  int P, Pl, Din, Pin0, ldu, ntens, per_layer, Kp;
  // the three scaled kinds (wire_net_desc_ms): c_k = 1 / |scales[k]|, k < nsc -- per column group (T), pass (S2) or stage (HS)
  int nsc = 0;
  float sc_c[WIRE_MS_MAX_SCALES] = {};
  // WIRE_KIND_BSPLINE_MS (kind then reads WIRE_KIND_BSPLINE, the activation of every layer behind the first stage): a frozen
  // first stage D -> SHF (its W0, b0 are tensors 0, 1) feeds layer 0, the GEMM SHF -> K; the plan's own tensors start at t0
  bool ms = false;
  int SHF = 0, T = 0, ms_split = 0, t0 = 0;
  // WIRE_KIND_BSPLINE_M2 (kind then reads WIRE_KIND_BSPLINE): the trunk runs S2 passes, pass k with c = sc_c[k] (s = the
  // pass-0 value), its rows at k n of buffers sized for S2 n rows; the combiner's four tensors come first (t0 = 4, the
  // trunk's native first layer at t0), their copy in the packed buffer at off_comb.  Every other kind: S2 = 1
  bool m2 = false;
  int S2 = 1;
  int64_t off_comb = -1;
  // WIRE_KIND_BSPLINE_HIER (kind then reads WIRE_KIND_BSPLINE): HS stages of the reference's HL hidden layers, stage s
  // with c = sc_c[s].  Every K -> K GEMM of the net is a "hidden layer" of this plan (L of them, hier_v): stage 0's HL, then
  // per stage s >= 1 its layer 2 and the two halves of its join (packed for the join's two data-gradient GEMMs).  The
  // join's own forward image [P][2P] (all families), bias and max-|weight| slots sit at hj_*[s]; hj_half: the halves as
  // [K][K] matrices; h_nat: native copies of every first layer and head
  bool hier = false;
  int HS = 0, HL = 0;
  int64_t hj_fwd[WIRE_MS_MAX_SCALES] = {}, hj_fwd_x3[WIRE_MS_MAX_SCALES] = {}, hj_fwd_x2[WIRE_MS_MAX_SCALES] = {},
          hj_bias[WIRE_MS_MAX_SCALES] = {}, hj_half[WIRE_MS_MAX_SCALES] = {}, hj_wamax = -1, h_nat = -1;
  // WIRE_KIND_MFN (kind then reads WIRE_KIND_RELU: real K -> K layers without an activation of their own): L + 1 Gabor
  // filters of the coordinates (tensors 4 i .. 4 i + 3: mu, gamma, w, c), the hidden layer l = 1 .. L is the reference's
  // linear[l - 1] (tensors mfn_tw(p, l), + 1), its output multiplied by filter l; the filters' tables [P][MFN_TAB] at mf_tab
  bool mfn = false;
  int64_t mf_tab = -1;
  // packed image offsets (floats); index l = 0..L (l = 0 only when first_gemm)
  std::vector<int64_t> off_fwd, off_dg, off_bias, off_fwd_x3, off_dg_x3, off_fwd_3m, off_dg_3m, off_fwd_x2, off_dg_x2;
  int64_t off_wf, off_bf, off_first, off_wamax, total_packed;   // off_wamax: max-|weight| slots, WIRE_AMAX_SLOTS per layer
  int64_t off_fx;    // k-permuted 2 x fp16 images of the hidden layers for the fused forward (wire_fused.hip), -1 = no such shape
  bool k_split_out, k_recompute_out, k_first_sums, k_first_dn, k_bwd_lookahead, k_nt_bfirst, k_epi_early, k_rstore, k_wgrad_batch, k_fused_fwd, k_fused_train, k_fused_bwd, k_fused_final,
       k_fused_train_p384;
  int64_t off_fxd;   // the same of the TRANSPOSED weights of layers L .. 1 (in that order) for the data-gradient chain, -1 = none
  std::vector<int64_t> tfloats;
};

// params[] index of tensor q of the native first layer: the multi-scale net's frozen first stage is tensors 0, 1; the
// multi-pass net's first trunk layer follows the combiner (t0)
inline int first_tensor(const Plan& p, int q) { return p.ms ? q : p.t0 + q; }

// ---- the multiplicative filter network's index maps: W of hidden layer l >= 1, the table of filter i
inline int mfn_tw(const Plan& p, int l) { return 4 * (p.L + 1) + 2 * (l - 1); }
inline const float* mfn_tab(const Plan& p, const float* packed, int i) { return packed + p.mf_tab + (int64_t)i * p.P * 12; }

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

int make_plan(const wire_net_desc* d, Plan& p);

inline int64_t fx_hidden_off(const Plan& p) { return p.off_fx + (p.first_gemm ? (int64_t)p.P * p.Pin0 : 0); }
// the whole-net forward's hidden images of pass k (the multi-pass net; every other kind: k = 0) and that pass's c
inline int64_t fx_pass_off(const Plan& p, int k) { return fx_hidden_off(p) + (int64_t)k * p.L * fused_b_image_floats(p.P); }
inline float pass_c(const Plan& p, int k) { return p.m2 ? p.sc_c[k] : p.s; }
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
ActLayout act_layout(const Plan& p, int64_t n1, int save);

// (the multi-pass net: gtr = the combiner's gradient of the trunk's outputs [S2][n1][O], cpart = its weight-gradient
// partials, crep = the coordinates once per pass [S2][n1][D] for the first layer's sums over all rows)
// (the multiplicative filter network: mh = the upstream gradient h of the filter in turn [n1][P], mfp = the per-block
// partials of its column sums)
struct ScratchLayout { int64_t ga, gb, gu, slab, bslab, fpw, fpb, crp, gamax, gch, gch_stride, gtr, cpart, crep, mh, mfp, total; int S; };
ScratchLayout scratch_layout(const Plan& p, int64_t n1);

// coordinate-gradient scratch (wire_mlp_bwd_coords), behind the backward's own: the per-row partials of the layer-1
// data-gradient epilogue, one set per 128-column tile of that GEMM's output [tile][n][D], and positional-encoding nets'
// g_pe [n][Pin0]
struct CoordLayout { int64_t cgp, gpe, total; int ntiles; };
// (the multi-pass net: cgp holds the per-pass coordinate gradients [S2][n1][D] before their sum)
CoordLayout coord_layout(const Plan& p, int64_t n);

// hidden-layer epilogues of a plan's kind (a base kind: make_plan refused every other)
inline int epi_fwd(int kind) { return known_kind(kind).epi_fwd; }
inline int epi_bwd(int kind) { return known_kind(kind).epi_bwd; }

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
  bool bwd_lookahead;     // wire: the data-gradient epilogue of layers l >= 2 in its look-ahead edition ("bwd_lookahead")
  bool first_dn;          // wire / wire2d: that epilogue in its compile-time-width edition where D is 2 or 3 ("first_dn")
  int wb_l0, wb_n, wb_S;  // weight-gradient batch: layers wb_l0 .. L, wb_n members of wb_S splits (wb_l0 = L + 1: none)
  float act_scale;        // split scale of the fused forward's activations, 0 = none known
  float out_scale[65];    // pre-split scale of out_l, l = 0 .. L (L <= 64); 0 = plain fp32
};
Route make_route(const Plan& p, int64_t n, RouteMode mode);

inline const unsigned* wamax_of(const Plan& p, const float* packed, int l) {   // max |W_l| slots
  return reinterpret_cast<const unsigned*>(packed + p.off_wamax + (int64_t)l * WIRE_AMAX_SLOTS);
}
// C = A W_l^T (the forward of layer l) or, dg, A W_l (its data gradient) on family f, from f's image of layer l.  The
// 2 x fp16 kernels also take the maximum slots of A, of W_l and of the tensor the epilogue writes (null: none kept)
hipError_t layer_nt(hipStream_t s, const Plan& p, WireFamily f, const float* packed, int l, bool dg, int epi,
                    const float* A, int64_t n, GemmEpiParams ep, const unsigned* amax_a = nullptr,
                    const unsigned* amax_b = nullptr, unsigned* amax_out = nullptr);   // wire_api.hip

// ---------------------------------------------------------------------------
// the multiplicative filter network (wire_mfn_api.hip)
// ---------------------------------------------------------------------------
Route mfn_route(const Plan& p, int64_t n, RouteMode mode);
int mfn_pack(hipStream_t s, const Plan& p, const void* const* params, float* packed);
int mfn_fwd_core(void* stream, const Plan& p, const Route& r, const float* packed, const float* coords, int64_t n, float* y,
                 void* act, int64_t act_bytes);
int mfn_bwd_core(void* stream, const Plan& p, const Route& r, const float* packed, const float* coords, int64_t n,
                 const float* g_y, const void* act, int64_t act_bytes, void* scratch, int64_t scratch_bytes,
                 void* const* grads, wire_grad_ready_fn ready, void* user, float* g_coords);

// ---------------------------------------------------------------------------
// the hierarchical B-spline net (wire_hier_api.hip)
// ---------------------------------------------------------------------------
// where a layer's activation goes: rows of ld floats (P, or 2P inside a join's input), aset = the max-|value| slot set
// its 2 x fp16 reader scales by (-1: no GEMM reads it)
struct HierOut { int64_t off; int ld; int aset; };
struct HierAct {
  int64_t amax, total;
  std::vector<std::vector<int64_t>> lin;   // [stage][layer]; -1 = not stored (inference)
  std::vector<std::vector<HierOut>> out;   // [stage][layer]
  std::vector<int64_t> cat;                // [stage >= 1]: the join's input [n][2P] = [x_in | x_{stage-1}]
};
// three g buffers [n][P] (the current layer's g_lin, the next one's, and T = the join's right-half gradient on its way to
// the previous stage's head backward), slabs for the widest weight gradient ([P][2P] with a join), the heads' and the
// first layers' pre-reduction blocks, the loss partials; cgp (behind everything, wire_bwd_coords_scratch_bytes): the
// per-stage coordinate gradients before their sum
struct HierScratch { int64_t gamax, g[3], slab, bslab, fpw, fpb, crp, lpart, total, cgp, total_coords; int S; };

HierAct hier_act(const Plan& p, int64_t n, int save);
HierScratch hier_scratch(const Plan& p, int64_t n);
Route hier_route(const Plan& p, int64_t n, RouteMode mode);
// the K -> K layers' images of a net, up to PACK_MAXB per launch: hW[l], hb[l] = W, b of the plan's hidden layer l (wire_api.hip)
int pack_hidden(hipStream_t s, const Plan& p, const void* const* params, float* packed, const std::vector<const float*>& hW,
                const std::vector<const float*>& hb);
int hier_pack(hipStream_t s, const Plan& p, const void* const* params, float* packed);
int hier_fwd_core(void* stream, const Plan& p, const Route& r, const float* packed, const float* coords, int64_t n, float* y,
                  void* act, int64_t act_bytes, const M2Loss* loss = nullptr, float* loss_part = nullptr);
int hier_bwd_core(void* stream, const Plan& p, const Route& r, const float* packed, const float* coords, int64_t n,
                  const float* g_y, const void* act, int64_t act_bytes, void* scratch, int64_t scratch_bytes,
                  void* const* grads, wire_grad_ready_fn ready, void* user, float* g_coords);
