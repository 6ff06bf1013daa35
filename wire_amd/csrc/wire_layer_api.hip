// wire_layer_api.hip -- per-layer entry points of the C ABI: one layer's forward / backward on native tensors
// (interleaved complex64, or fp32 for the real kinds and a first layer's coordinates), and the final complex
// Linear + .real.  These serve `model.net[i](x)` (reference modules/utils.py:246-252) and standalone layers; the
// training hot path is wire_mlp_fwd / wire_mlp_bwd, which never leaves the blocked layout.  The backward recomputes
// the layer's forward from x (one extra GEMM) instead of asking the caller to keep lin/act in a private layout.
//
// The file has no kernel and says each thing once:
//   layer_ws       the one workspace table, plain or 2-D
//   LayerGemm      one layer's GEMMs on the selected family, over that table
//   FORMS          what ComplexGaborLayer, ComplexGaborLayer2D and the real layers differ in -- the place to extend
//   Layer          a call: form, shape, arguments and workspace; Layer::open is the preamble every entry point shares
//   layer_forward / layer_bwd / layer_bwd_first / layer_hparam   the four routines, driven by the form
// An extern "C" function is its own argument test (host tests pin every refusal) and a call.
#include <hip/hip_runtime.h>

#include <algorithm>

#include "wire_plan.h"

// GEMM family the tuning flags select (wire_family_, wire_gemm.h): FAM_X3 = split-bf16 (wire_gemmx3.hip, every kind),
// FAM_3M = 3-multiplication complex fp32 MFMA (wire_gemm3m.hip, ComplexGaborLayer only), FAM_4M = 4M fp32 MFMA.
// The per-layer entry points run the SAME kernels as wire_mlp_fwd / wire_mlp_bwd, so the per-layer parity
// tests (protocol step (i)) check the code the bench times.

#define LCHK(expr)                                                   \
  do {                                                               \
    hipError_t e_ = (expr);                                          \
    if (e_ != hipSuccess) return wire_fail_(WIRE_ERR_HIP, hipGetErrorString(e_)); \
  } while (0)

namespace {
inline int64_t rup64(int64_t v, int64_t m) { return (v + m - 1) / m * m; }

// 2 x fp16 family in the per-layer entry points (split_f16, batches the 16 x 16 x 32 kernels take): a region of the
// workspace holds 4 maximum-slot sets (A operand, weights, G, Z) and the two split weight images.  The operand maxima of
// the fused path come from the producers' epilogues; here the tensors arrive from the caller, so one reduction pass
// (launch_amax) per operand precedes the GEMM.
inline int64_t x2_region_floats(int Pout_g, int Pin) {
  return 4 * WIRE_AMAX_SLOTS + gemmx2_b_image_floats(Pout_g, Pin) + gemmx2_b_image_floats(Pin, Pout_g);
}
// weight-gradient row splits of a family (the workspace is sized for the largest: its size must not depend on
// the tuning flags)
inline int layer_splits(int fam, int64_t n, int Pout, int Pin) {
  if (fam == FAM_X3) return gemmx3_tn_splits(n, Pout, Pin, 256);
  if (fam == FAM_3M) return gemm3m_tn_splits(n, Pout / 2, Pin / 2, 64);
  return gemm_tn_splits(n, Pout, Pin, 64);
}

// The workspace of a layer call, in floats from its base.  Pin / Pout are the complex sizing (a real layer's narrower
// rows fit it); Ng is the GEMM's width: Pout, or 2 Pout where the 2-D Gabor layer runs both its Linears as one GEMM
// (lin | sy).  lin / glin rows are Ng wide, gu rows Ng / 2, out / gact rows Pout; fpw / fpb / wf / bfr belong to the final
// layer and are empty in the 2-D table.
struct LayerWs {
  int Pin, Pout, Ng;
  int64_t xb, lin, out, gact, glin, gxb, gu, btf, btd, bias, slab, bslab, fpw, fpb, crp, wf, bfr, btf_x3, btd_x3, x2, total;
};
LayerWs layer_ws(int64_t n, int in, int out, bool two) {
  LayerWs w{};
  w.Pin = rup(2 * in, 64);
  w.Pout = rup(2 * out, 64);
  w.Ng = two ? 2 * w.Pout : w.Pout;
  const int Pmax = w.Pin > w.Pout ? w.Pin : w.Pout;
  // weight-gradient slabs.  The two tables size them by different rules, and wire_layer_ws_bytes / wire_layer2d_ws_bytes
  // are pinned to both (tests/golden/size_queries.json):
  //   plain: room for every family (4M, 3M with its 3 quarter-size products, 3 x bf16, 2 x fp16), for the complex sizing
  //          and for the real layers' own (narrower rows split finer, so neither sizing dominates the other)
  //   2-D:   the larger of the 4M splits and the 3 x bf16 maximum, full-size slabs (the 3M family never runs this layer)
  int64_t slab_f = 0, bslab_f = 0;
  if (two) {
    const int64_t s_max = std::max<int64_t>(gemm_tn_splits(n, w.Ng, w.Pin, 64), gemmx3_tn_splits_max(n, w.Ng, w.Pin, 256));
    slab_f = s_max * w.Ng * w.Pin;
    bslab_f = s_max * w.Ng;
  } else {
    auto fit = [&](int Pm, int Pn) {
      for (int fam = FAM_4M; fam <= FAM_X3; ++fam) {
        int64_t S = fam == FAM_X3 ? gemmx3_tn_splits_max(n, Pm, Pn, 256) : layer_splits(fam, n, Pm, Pn);
        if (fam == FAM_X3 && gemmx2_tn_splits(n, Pm, Pn, 256) > S) S = gemmx2_tn_splits(n, Pm, Pn, 256);
        const int64_t sl = fam == FAM_3M ? S * 3 * (Pm / 2) * (Pn / 2) : S * Pm * Pn;
        if (sl > slab_f) slab_f = sl;
        if (S * Pm > bslab_f) bslab_f = S * Pm;
      }
    };
    fit(w.Pout, w.Pin);
    fit(rup(out, 64), rup(in, 64));
  }
  const int64_t fin = two ? 0 : 1;     // the final layer's regions
  int64_t off = 0;
  auto take = [&](int64_t cnt) { int64_t o = off; off += rup64(cnt, 64); return o; };
  w.xb = take(n * w.Pin);
  w.lin = take(n * w.Ng);
  w.out = take(n * w.Pout);
  w.gact = take(n * w.Pout);
  w.glin = take(n * w.Ng);
  w.gxb = take(n * w.Pin);
  w.gu = take(n * (w.Ng / 2));
  w.btf = take((int64_t)w.Ng * w.Pin);
  w.btd = take((int64_t)w.Ng * w.Pin);
  w.bias = take(w.Ng);
  w.slab = take(slab_f);
  w.bslab = take(bslab_f);
  w.fpw = take(fin * prereduce_room(final_bwd_blocks(n)) * 8 * Pmax);
  w.fpb = take(fin * prereduce_room(final_bwd_blocks(n)) * 8);
  w.crp = take((int64_t)prereduce_room(colreduce_blocks(n)) * (w.Pout / 2) * 5);
  w.wf = take(fin * 8 * Pmax);
  w.bfr = take(fin * 64);
  w.btf_x3 = take(gemmx3_b_image_floats(w.Ng, w.Pin));
  w.btd_x3 = take(gemmx3_b_image_floats(w.Pin, w.Ng));
  w.x2 = take(x2_region_floats(w.Ng, w.Pin));
  w.total = off;
  return w;
}

// What every launching entry point does after its own argument test: the table, the size test, the stream, the base.
struct LayerCall {
  LayerWs w;
  hipStream_t s;
  float* W_;
  float* at(int64_t off) const { return W_ + off; }
  int open(int64_t n, int in, int out, bool two, void* stream, void* ws, int64_t ws_bytes) {
    w = layer_ws(n, in, out, two);
    if (ws_bytes < w.total * 4) return wire_fail_(WIRE_ERR_SIZE, "layer workspace too small");
    s = (hipStream_t)stream;
    W_ = (float*)ws;
    return WIRE_OK;
  }
};

// One layer's GEMMs on the selected family.  All three take blocked rows (wire_dev.h) and leave the same
// outputs; they differ in the weight image (pack_*) and in the slab format of the weight gradient.  The images, the
// bias and the slabs lie where the call's table says: btf / btd hold the fp32 images of the family, btf_x3 / btd_x3 the
// split images.
struct LayerGemm {
  WireFamily fam;
  const LayerCall* c;
  float* x2ws;       // x2_region_floats(...) of the workspace, or null: never the 2 x fp16 kernels
  bool use_x2(int epi, int64_t n) const {
    return fam == FAM_X3 && x2ws && knob(K_SPLIT_F16) && gemmx3_nt_is_h16(epi, n);
  }
  unsigned* slots(int which) const { return reinterpret_cast<unsigned*>(x2ws) + which * WIRE_AMAX_SLOTS; }
  hipError_t pack(int kind, const float* W, const float* b, const float* V, const float* cc, int out, int in, int Pout_g,
                  int Pin, float wscale) const {
    hipStream_t s = c->s;
    float *btf = c->at(c->w.btf), *btd = c->at(c->w.btd), *bias = c->at(c->w.bias);
    if (fam == FAM_3M) return launch_pack3m(s, W, b, out, in, Pout_g / 2, Pin / 2, btf, btd, bias);
    hipError_t e = launch_pack_hidden(s, kind, W, b, V, cc, out, in, kind == NK_WIRE2D ? Pout_g / 2 : Pout_g, Pin,
                                      btf, btd, bias, wscale);
    if (e != hipSuccess || fam != FAM_X3) return e;
    e = launch_x3_split_b(s, btf, Pin, Pout_g, Pin, c->at(c->w.btf_x3));
    if (e != hipSuccess) return e;
    e = launch_x3_split_b(s, btd, Pout_g, Pin, Pout_g, c->at(c->w.btd_x3));
    if (e != hipSuccess || !x2ws || !knob(K_SPLIT_F16)) return e;
    // 2 x fp16 images: max |weight| (the transposed image holds the same values), then both scaled splits
    e = hipMemsetAsync(x2ws, 0, 4 * WIRE_AMAX_SLOTS * sizeof(float), s);
    if (e != hipSuccess) return e;
    e = launch_amax(s, btf, (int64_t)Pout_g * Pin, slots(1));
    if (e != hipSuccess) return e;
    float* img_f = x2ws + 4 * WIRE_AMAX_SLOTS;
    float* img_d = img_f + gemmx2_b_image_floats(Pout_g, Pin);
    X2SplitBatch xf{}, xd{};
    xf.src[0] = btf; xf.dst[0] = img_f; xf.slots[0] = slots(1);
    xd.src[0] = btd; xd.dst[0] = img_d; xd.slots[0] = slots(1);
    e = launch_x2_split_b_batch(s, xf, 1, Pin, Pout_g, Pin);
    if (e != hipSuccess) return e;
    return launch_x2_split_b_batch(s, xd, 1, Pout_g, Pin, Pout_g);
  }
  // C[n][Nc] = A[n][Kd] * image^T + epilogue; dgrad = true uses the transposed-conjugate image
  hipError_t nt(int epi, const float* A, int64_t n, int Nc, int Kd, bool dgrad, const GemmEpiParams& ep) const {
    hipStream_t s = c->s;
    if (use_x2(epi, n)) {
      // forward: image [Nc = Pout_g][Kd = Pin]; data gradient: the transposed image [Nc = Pin][Kd = Pout_g]
      const int Pout_g = dgrad ? Kd : Nc, Pin = dgrad ? Nc : Kd;
      float* img_f = x2ws + 4 * WIRE_AMAX_SLOTS;
      float* img_d = img_f + gemmx2_b_image_floats(Pout_g, Pin);
      unsigned* sa = slots(dgrad ? 2 : 0);
      hipError_t e = hipMemsetAsync(sa, 0, WIRE_AMAX_SLOTS * sizeof(unsigned), s);
      if (e != hipSuccess) return e;
      e = launch_amax(s, A, n * Kd, sa);
      if (e != hipSuccess) return e;
      GemmEpiParams e2 = ep;
      e2.amax_a = sa; e2.amax_b = slots(1);
      return launch_gemmx2h_nt(s, epi, A, Kd, dgrad ? img_d : img_f, n, Nc, Kd, e2,
                               x2_waits(knob(K_NT_BFIRST) != 0, knob(K_EPI_EARLY) != 0));
    }
    if (fam == FAM_X3)
      return launch_gemmx3_nt(s, epi, A, Kd, c->at(dgrad ? c->w.btd_x3 : c->w.btf_x3), n, Nc, Kd, ep);
    const float* img = c->at(dgrad ? c->w.btd : c->w.btf);
    if (fam == FAM_3M) return launch_gemm3m_nt(s, epi, A, Kd, img, Kd, n, Nc / 2, Kd / 2, ep);
    return launch_gemm_nt(s, epi, A, Kd, img, Kd, n, Nc, Kd, ep);
  }
  hipError_t tn_reduce(int kind, const float* G, const float* Z, int64_t n, int Pm, int Pn, int out, int in, float* gW,
                       float* gb, float* gV, float* gc, float wscale) const {
    hipStream_t s = c->s;
    float *slab = c->at(c->w.slab), *bslab = c->at(c->w.bslab);
    hipError_t e;
    if (use_x2(EPI_STORE, n) && gemmx2_tn_applies(Pm, Pn)) {
      const int S2 = gemmx2_tn_splits(n, Pm, Pn, 256);
      e = hipMemsetAsync(slots(2), 0, 2 * WIRE_AMAX_SLOTS * sizeof(unsigned), s);       // G and Z
      if (e != hipSuccess) return e;
      e = launch_amax(s, G, n * Pm, slots(2));
      if (e != hipSuccess) return e;
      e = launch_amax(s, Z, n * Pn, slots(3));
      if (e != hipSuccess) return e;
      e = launch_gemmx2_tn(s, G, Pm, Z, Pn, n, Pm, Pn, S2, slab, bslab, slots(2), slots(3));
      if (e != hipSuccess) return e;
      return launch_wgrad_reduce(s, kind, slab, bslab, S2, out, in, Pm, Pn, gW, gb, gV, gc, wscale);
    }
    const int S = layer_splits(fam, n, Pm, Pn);
    if (fam == FAM_3M) {
      e = launch_gemm3m_tn(s, G, Pm, Z, Pn, n, Pm / 2, Pn / 2, S, slab, bslab);
      if (e != hipSuccess) return e;
      return launch_wgrad3m_reduce(s, slab, bslab, S, out, in, Pm / 2, Pn / 2, gW, gb);
    }
    e = fam == FAM_X3 ? launch_gemmx3_tn(s, G, Pm, Z, Pn, n, Pm, Pn, S, slab, bslab)
                      : launch_gemm_tn(s, G, Pm, Z, Pn, n, Pm, Pn, S, slab, bslab);
    if (e != hipSuccess) return e;
    return launch_wgrad_reduce(s, kind, slab, bslab, S, out, in, Pm, Pn, gW, gb, gV, gc, wscale);
  }
};

// ---------------------------------------------------------------------------
// The layer forms.  A form is everything in which the routines below differ between
//   ComplexGaborLayer    (modules/wire.py:88-93)     on complex64 rows, or fp32 coordinates when is_first
//   ComplexGaborLayer2D  (modules/wire2d.py:21-67)   the same with a second Linear (V, c): both Linears are ONE GEMM
//                                                    ([n, Pin] x [Pin -> 2 Pout], 128-column groups (lin_re | lin_im | sy_re | sy_im))
//   the real layers      SineLayer / GaussLayer / ReLULayer / Bsplines_form / Bsplines_cubic .forward (modules/siren.py:48-49,
//                        gauss.py:27-28, relu.py:28-29, bspline_form.py:38-49, bspline_cubic.py:44-52) on fp32 [n][in] rows
// The net kind of a call selects its form; the kind itself goes to the pack, the family and the activation table
// (forward epilogue = epi_fwd(kind)).  A new layer form is a new row here and its entry points' argument tests.
// ---------------------------------------------------------------------------
using RowConv = hipError_t (*)(hipStream_t, const float* src, int64_t n, int K, int P, float* dst);
using PointFn = hipError_t (*)(hipStream_t, int kind, const float* g, const float* lin, const float* out, int64_t n, int P,
                               float omega, float scale, float* g_lin);
using FirstPointFn = hipError_t (*)(hipStream_t, const float* g, const float* out, const float* coords, int D,
                                    const float* W0, const float* b0, const float* V0, const float* c0, int64_t n, int K,
                                    int P, float omega, float scale, float* g_u, int ldu);
using HparamFn = hipError_t (*)(hipStream_t, const float* g, const float* lin, const float* out, int64_t n, int K, int P,
                                int is_first, float scale, float* partial, float* out2);
struct LayerForm {
  bool two;                  // (V, c) exist: the 2-D table, a GEMM 2 Pout wide, lin | sy and g_u | g_p side by side
  int cw;                    // floats of a native element: rows are rup(cw * features, 64) wide in the workspace
  RowConv rows_in, rows_out; // native rows <-> workspace rows: complex64 <-> blocked, fp32 <-> padded
  PointFn point;             // g_act -> g_lin of a hidden layer
  FirstPointFn first_point;  // g_act -> g_u (| g_p) of a first layer on coordinates; null: the form has no is_first
  HparamFn hparam;           // {dL/d omega_0, dL/d scale_0}; null: the form has none
};
enum { FORM_GABOR, FORM_GABOR2D, FORM_REAL };
const LayerForm FORMS[] = {
  {false, 2, launch_c64_to_blocked, launch_blocked_to_c64,
   [](hipStream_t s, int, const float* g, const float* lin, const float* out, int64_t n, int P, float om, float sc,
      float* gl) { return launch_gabor_bwd_point(s, g, lin, out, n, P, om, sc, gl); },
   [](hipStream_t s, const float* g, const float* out, const float* x, int D, const float* W0, const float* b0, const float*,
      const float*, int64_t n, int K, int P, float om, float sc, float* gu, int ldu) {
     return launch_gabor_bwd_first_point(s, g, out, x, D, W0, b0, n, K, P, om, sc, gu, ldu);
   },
   launch_gabor_hparam_grad},
  {true, 2, launch_c64_to_blocked, launch_blocked_to_c64,
   [](hipStream_t s, int, const float* g, const float* lin, const float* out, int64_t n, int P, float om, float sc,
      float* gl) { return launch_gabor2d_bwd_point(s, g, lin, out, n, P, om, sc, gl); },
   launch_gabor2d_bwd_first_point, launch_gabor2d_hparam_grad},
  {false, 1, launch_pad_rows, launch_unpad_rows, launch_real_act_bwd_point, nullptr, nullptr},
};
inline int form_of(int kind) { return kind == NK_WIRE ? FORM_GABOR : kind == NK_WIRE2D ? FORM_GABOR2D : FORM_REAL; }

// One call of a layer: the form, the shape the kernels see, the arguments and the workspace.
struct Layer : LayerCall {
  const LayerForm* f;
  int kind, in, out, is_first;
  int64_t n;
  int Pin, Pout, Ng;                  // row widths of this form (a real layer's are narrower than the table's); GEMM width
  const float *x, *W, *b, *V, *c;     // V, c: null unless f->two
  float omega, scale, wscale;         // scale, wscale: kind_scale's pair (wire_kinds.h) -- s W in both images, the bias as
                                      // it is, g_W multiplied by wscale on the way out; (scale_0, 1) for the Gabor layers
  LayerGemm g;
  float *xb, *lin, *act, *gact, *glin, *gxb, *gu;

  int open(int kind_, void* stream, const void* x_, const void* W_t, const void* b_, const void* V_, const void* c_,
           float omega0, float scale0, float wscale_, int64_t n_, int in_, int out_, int first, void* ws, int64_t ws_bytes) {
    f = &FORMS[form_of(kind_)];
    if (int rc = LayerCall::open(n_, in_, out_, f->two, stream, ws, ws_bytes)) return rc;
    kind = kind_; in = in_; out = out_; is_first = first; n = n_;
    Pin = rup(f->cw * in, 64); Pout = rup(f->cw * out, 64); Ng = f->two ? 2 * Pout : Pout;
    x = (const float*)x_; W = (const float*)W_t; b = (const float*)b_; V = (const float*)V_; c = (const float*)c_;
    omega = omega0; scale = scale0; wscale = wscale_;
    // the 2 x fp16 region, or null: a cubic B-spline layer of at most 64 inputs stays on the 3 x bf16 kernels at every row
    // count.  The 2 x fp16 split drops the l l product (2^-22 of each product); the 2 to 64 products of such a row do not
    // average that out, and the layer's scale_0 sits in the operand (|s W| is 15 times the other kinds' at the class
    // default): measured 3.5 times the fp32 error on lin at 2 -> 256, s = 15, 8229 rows, where the whole-net path's first
    // layer is an fp32 FMA chain.  3 x bf16 carries 24 bits per operand.
    g = LayerGemm{wire_family_(kind), this, kind == WIRE_KIND_BSPLINE_CUBIC && Pin <= 64 ? nullptr : at(w.x2)};
    xb = at(w.xb); lin = at(w.lin); act = at(w.out); gact = at(w.gact); glin = at(w.glin); gxb = at(w.gxb); gu = at(w.gu);
    return WIRE_OK;
  }
};

// forward into the workspace (lin, act in workspace rows).  Shared by all four routines.
int layer_forward(const Layer& l, bool want_lin = false) {
  if (l.is_first) {
    if (l.in > 4) return wire_fail_(WIRE_ERR_ARG, "is_first layers support in_features <= 4");
    // u = x W0^T + b0 (| p = x V0^T + c0) is real: [n][Ng / 2] rows in lin when asked for
    LCHK(launch_first_fwd(l.s, l.kind, l.x, l.n, l.in, l.W, l.b, l.V, l.c, l.out, l.Pout, l.omega, l.scale,
                          want_lin ? l.lin : nullptr, l.act));
    return WIRE_OK;
  }
  LCHK(l.f->rows_in(l.s, l.x, l.n, l.in, l.Pin, l.xb));
  LCHK(l.g.pack(l.kind, l.W, l.b, l.V, l.c, l.out, l.in, l.Ng, l.Pin, l.wscale));
  GemmEpiParams ep;
  ep.bias = l.at(l.w.bias); ep.o0 = l.lin; ep.o1 = l.act; ep.ld0 = l.Ng; ep.ld1 = l.Pout;
  ep.omega = l.omega; ep.scale = l.scale; ep.kvalid = l.out;
  LCHK(l.g.nt(epi_fwd(l.kind), l.xb, l.n, l.Ng, l.Pin, false, ep));
  return WIRE_OK;
}

// act_out, and the pre-activation `lin` of modules/wire.py:89 when asked for (wire_gabor_fwd alone): native rows like
// act_out, or float32 [n][out] for is_first
int layer_fwd(const Layer& l, void* act_out, void* lin_out = nullptr) {
  if (int rc = layer_forward(l, lin_out != nullptr)) return rc;
  LCHK(l.f->rows_out(l.s, l.act, l.n, l.out, l.Pout, (float*)act_out));
  if (lin_out) {
    if (l.is_first) LCHK(launch_unpad_rows(l.s, l.lin, l.n, l.out, l.Pout / 2, (float*)lin_out));
    else LCHK(l.f->rows_out(l.s, l.lin, l.n, l.out, l.Pout, (float*)lin_out));
  }
  return WIRE_OK;
}

// first layer on coordinates: g_u (| g_p) = the gradient at the real pre-activations, [n][Ng / 2] rows; the parameter
// gradients are column reductions of it (g_W null: none), the coordinate gradient g_x [n][in] f32 = g_u W (+ g_p V)
// (g_x null: none)
int layer_bwd_first(const Layer& l, const void* g_act, float* g_x, float* g_W, float* g_b, float* g_V, float* g_c) {
  if (int rc = layer_forward(l)) return rc;
  LCHK(l.f->rows_in(l.s, (const float*)g_act, l.n, l.out, l.Pout, l.gact));
  const int ldu = l.Pout / 2, ldg = l.Ng / 2;
  LCHK(l.f->first_point(l.s, l.gact, l.act, l.x, l.in, l.W, l.b, l.V, l.c, l.n, l.out, l.Pout, l.omega, l.scale, l.gu, ldu));
  if (g_W) {
    LCHK(launch_colreduce(l.s, l.gu, ldg, l.out, l.x, l.in, l.n, l.at(l.w.crp), g_W, g_b));
    if (l.f->two) LCHK(launch_colreduce(l.s, l.gu + ldu, ldg, l.out, l.x, l.in, l.n, l.at(l.w.crp), g_V, g_c));
  }
  if (g_x) LCHK(launch_coordgrad_rows(l.s, l.gu, ldg, l.f->two ? l.gu + ldu : nullptr, l.W, l.V, l.out, l.in, l.n, g_x));
  return WIRE_OK;
}

// forward, g_act -> g_lin, the data-gradient GEMM when g_x is given, the weight-gradient GEMM and its reduction
int layer_bwd(const Layer& l, const void* g_act, void* g_x, void* g_W, void* g_b, void* g_V, void* g_c) {
  if (l.is_first) return layer_bwd_first(l, g_act, nullptr, (float*)g_W, (float*)g_b, (float*)g_V, (float*)g_c);
  if (int rc = layer_forward(l)) return rc;
  LCHK(l.f->rows_in(l.s, (const float*)g_act, l.n, l.out, l.Pout, l.gact));
  LCHK(l.f->point(l.s, l.kind, l.gact, l.lin, l.act, l.n, l.Pout, l.omega, l.scale, l.glin));
  if (g_x) {
    GemmEpiParams ep; ep.o0 = l.gxb; ep.ld0 = l.Pin; ep.ld1 = l.Pin;
    LCHK(l.g.nt(EPI_STORE, l.glin, l.n, l.Pin, l.Ng, true, ep));
    LCHK(l.f->rows_out(l.s, l.gxb, l.n, l.in, l.Pin, (float*)g_x));
  }
  LCHK(l.g.tn_reduce(l.kind, l.glin, l.xb, l.n, l.Ng, l.Pin, l.out, l.in, (float*)g_W, (float*)g_b, (float*)g_V,
                     (float*)g_c, l.wscale));
  return WIRE_OK;
}

// trainable omega_0 / scale_0 (ComplexGaborLayer(trainable=True), modules/wire.py:80-81; ComplexGaborLayer2D,
// modules/wire2d.py:42-43): out2 = {dL/d omega_0, dL/d scale_0} (device).  Recomputes the layer's forward from x, like
// layer_bwd.  Partial sums live in the (unused here) g_lin region: 2 * ceil(n / 32) floats <= n * Pout
int layer_hparam(const Layer& l, const void* g_act, float* out2) {
  if (int rc = layer_forward(l, true)) return rc;
  LCHK(l.f->rows_in(l.s, (const float*)g_act, l.n, l.out, l.Pout, l.gact));
  LCHK(l.f->hparam(l.s, l.gact, l.lin, l.act, l.n, l.out, l.Pout, l.is_first, l.scale, l.glin, out2));
  return WIRE_OK;
}
}  // namespace

static int64_t ws_bytes_of(int64_t n, int in, int out, bool two) {
  if (n < 0 || in < 1 || out < 1) return wire_fail_(WIRE_ERR_ARG, "bad layer shape");
  return layer_ws(n, in, out, two).total * 4 + 256;
}
extern "C" int64_t wire_layer_ws_bytes(int64_t n, int in_features, int out_features) {
  return ws_bytes_of(n, in_features, out_features, false);
}
extern "C" int64_t wire_layer2d_ws_bytes(int64_t n, int in_features, int out_features) {
  return ws_bytes_of(n, in_features, out_features, true);
}

// ---------------------------------------------------------------------------
// ComplexGaborLayer
// ---------------------------------------------------------------------------
extern "C" int wire_gabor_fwd(void* stream, const void* x, const void* W, const void* b,
                              float omega0, float scale0, int64_t n, int in_features,
                              int out_features, int is_first, void* lin_out, void* act_out,
                              void* ws, int64_t ws_bytes) {
  if (n < 0 || in_features < 1 || out_features < 1 || !x || !W || !b || !act_out || !ws)
    return wire_fail_(WIRE_ERR_ARG, "bad argument to wire_gabor_fwd");
  if (n == 0) return WIRE_OK;
  Layer l;
  if (int rc = l.open(WIRE_KIND_WIRE, stream, x, W, b, nullptr, nullptr, omega0, scale0, 1.f, n, in_features,
                      out_features, is_first, ws, ws_bytes))
    return rc;
  return layer_fwd(l, act_out, lin_out);
}

extern "C" int wire_gabor_bwd(void* stream, const void* g_act, const void* x, const void* W,
                              const void* b, float omega0, float scale0, int64_t n,
                              int in_features, int out_features, int is_first, void* g_x,
                              void* g_W, void* g_b, void* ws, int64_t ws_bytes) {
  if (n <= 0 || in_features < 1 || out_features < 1 || !g_act || !x || !W || !b || !g_W || !g_b || !ws)
    return wire_fail_(WIRE_ERR_ARG, "bad argument to wire_gabor_bwd");
  Layer l;
  if (int rc = l.open(WIRE_KIND_WIRE, stream, x, W, b, nullptr, nullptr, omega0, scale0, 1.f, n, in_features,
                      out_features, is_first, ws, ws_bytes))
    return rc;
  return layer_bwd(l, g_act, g_x, g_W, g_b, nullptr, nullptr);
}

// first layer with the coordinate gradient: g_x [n][in] f32 = g_u W (coordgrad_rows over the g_u the backward forms
// anyway); g_W / g_b NULL together = the coordinate gradient alone
extern "C" int wire_gabor_bwd_first_coords(void* stream, const void* g_act, const float* x, const float* W, const float* b,
                                           float omega0, float scale0, int64_t n, int in_features, int out_features,
                                           float* g_x, float* g_W, float* g_b, void* ws, int64_t ws_bytes) {
  if (n <= 0 || in_features < 1 || in_features > 4 || out_features < 1 || !g_act || !x || !W || !b || !g_x || !ws ||
      (!g_W) != (!g_b))
    return wire_fail_(WIRE_ERR_ARG, "bad argument to wire_gabor_bwd_first_coords");
  Layer l;
  if (int rc = l.open(WIRE_KIND_WIRE, stream, x, W, b, nullptr, nullptr, omega0, scale0, 1.f, n, in_features,
                      out_features, 1, ws, ws_bytes))
    return rc;
  return layer_bwd_first(l, g_act, g_x, g_W, g_b, nullptr, nullptr);
}

extern "C" int wire_gabor_hparam_grad(void* stream, const void* g_act, const void* x, const void* W, const void* b,
                                      float omega0, float scale0, int64_t n, int in_features, int out_features,
                                      int is_first, float* out2, void* ws, int64_t ws_bytes) {
  if (n <= 0 || in_features < 1 || out_features < 1 || !g_act || !x || !W || !b || !out2 || !ws)
    return wire_fail_(WIRE_ERR_ARG, "bad argument to wire_gabor_hparam_grad");
  Layer l;
  if (int rc = l.open(WIRE_KIND_WIRE, stream, x, W, b, nullptr, nullptr, omega0, scale0, 1.f, n, in_features,
                      out_features, is_first, ws, ws_bytes))
    return rc;
  return layer_hparam(l, g_act, out2);
}

// ---------------------------------------------------------------------------
// the final complex Linear + .real (the plain table's fpw / fpb / wf / bfr regions)
// ---------------------------------------------------------------------------
extern "C" int wire_final_fwd(void* stream, const void* z, const void* Wf, const void* bf, int64_t n,
                              int in_features, int out_features, float* y, void* ws,
                              int64_t ws_bytes) {
  if (n < 0 || in_features < 1 || out_features < 1 || out_features > 8 || !z || !Wf || !bf || !y || !ws)
    return wire_fail_(WIRE_ERR_ARG, "bad argument to wire_final_fwd");
  // final_fwd_kernel stages W_f [O][P] in the 64 KB of dynamic LDS a launch gets (make_plan refuses the same nets)
  if ((int64_t)out_features * rup64(2 * (int64_t)in_features, 64) > WIRE_FINAL_MAX_OP)
    return fail(WIRE_ERR_ARG, "out_features %d x padded row width %lld > %d (the final layer's weights in 64 KB)",
                out_features, (long long)rup64(2 * (int64_t)in_features, 64), WIRE_FINAL_MAX_OP);
  if (n == 0) return WIRE_OK;
  LayerCall c;
  if (int rc = c.open(n, in_features, out_features, false, stream, ws, ws_bytes)) return rc;
  const LayerWs& w = c.w;
  LCHK(launch_c64_to_blocked(c.s, (const float*)z, n, in_features, w.Pin, c.at(w.xb)));
  LCHK(launch_pack_final(c.s, NK_WIRE, (const float*)Wf, (const float*)bf, in_features, w.Pin,
                         out_features, c.at(w.wf), c.at(w.bfr)));
  LCHK(launch_final_fwd(c.s, c.at(w.xb), n, w.Pin, out_features, c.at(w.wf), c.at(w.bfr), y));
  return WIRE_OK;
}

extern "C" int wire_final_bwd(void* stream, const float* g_y, const void* z, const void* Wf,
                              int64_t n, int in_features, int out_features, void* g_z, void* g_Wf,
                              void* g_bf, void* ws, int64_t ws_bytes) {
  if (n <= 0 || in_features < 1 || out_features < 1 || out_features > 8 || !g_y || !z || !Wf ||
      !g_Wf || !g_bf || !ws)
    return wire_fail_(WIRE_ERR_ARG, "bad argument to wire_final_bwd");
  LayerCall c;
  if (int rc = c.open(n, in_features, out_features, false, stream, ws, ws_bytes)) return rc;
  const LayerWs& w = c.w;
  LCHK(launch_c64_to_blocked(c.s, (const float*)z, n, in_features, w.Pin, c.at(w.xb)));
  // bias pointer is irrelevant for the gradient; reuse Wf so the kernel reads valid memory
  LCHK(launch_pack_final(c.s, NK_WIRE, (const float*)Wf, (const float*)Wf, in_features, w.Pin,
                         out_features, c.at(w.wf), c.at(w.bfr)));
  LCHK(launch_final_bwd(c.s, NK_WIRE, 1, g_y, n, out_features, c.at(w.wf), nullptr, c.at(w.xb),
                        in_features, w.Pin, 0.f, 0.f, c.at(w.gxb), c.at(w.fpw), c.at(w.fpb)));
  LCHK(launch_final_reduce(c.s, NK_WIRE, c.at(w.fpw), c.at(w.fpb), final_bwd_blocks(n), out_features,
                           in_features, w.Pin, (float*)g_Wf, (float*)g_bf));
  if (g_z) LCHK(launch_blocked_to_c64(c.s, c.at(w.gxb), n, in_features, w.Pin, (float*)g_z));
  return WIRE_OK;
}

// ---------------------------------------------------------------------------
// the real layers (the plain table: its complex sizing is an upper bound of theirs)
// ---------------------------------------------------------------------------
extern "C" int wire_real_layer_fwd(void* stream, int kind, const float* x, const float* W, const float* b,
                                   float omega0, float scale0, int64_t n, int in_features, int out_features,
                                   float* act_out, void* ws, int64_t ws_bytes) {
  float kscale, wscale;
  if (!kind_is_real(kind) || n < 0 || in_features < 1 || out_features < 1 || !x ||
      !W || !b || !act_out || !ws || !kind_scale(kind, scale0, kscale, wscale))
    return wire_fail_(WIRE_ERR_ARG, "bad argument to wire_real_layer_fwd");
  if (n == 0) return WIRE_OK;
  Layer l;
  if (int rc = l.open(kind, stream, x, W, b, nullptr, nullptr, omega0, kscale, wscale, n, in_features, out_features, 0,
                      ws, ws_bytes))
    return rc;
  return layer_fwd(l, act_out);
}

extern "C" int wire_real_layer_bwd(void* stream, int kind, const float* g_act, const float* x, const float* W,
                                   const float* b, float omega0, float scale0, int64_t n, int in_features,
                                   int out_features, float* g_x, float* g_W, float* g_b, void* ws,
                                   int64_t ws_bytes) {
  float kscale, wscale;
  if (!kind_is_real(kind) || n <= 0 || in_features < 1 || out_features < 1 ||
      !g_act || !x || !W || !b || !g_W || !g_b || !ws || !kind_scale(kind, scale0, kscale, wscale))
    return wire_fail_(WIRE_ERR_ARG, "bad argument to wire_real_layer_bwd");
  Layer l;
  if (int rc = l.open(kind, stream, x, W, b, nullptr, nullptr, omega0, kscale, wscale, n, in_features, out_features, 0,
                      ws, ws_bytes))
    return rc;
  return layer_bwd(l, g_act, g_x, g_W, g_b, nullptr, nullptr);
}

// ---------------------------------------------------------------------------
// ComplexGaborLayer2D
// ---------------------------------------------------------------------------
extern "C" int wire_gabor2d_fwd(void* stream, const void* x, const void* W, const void* b, const void* V,
                                const void* c, float omega0, float scale0, int64_t n, int in_features,
                                int out_features, int is_first, void* act_out, void* ws, int64_t ws_bytes) {
  if (n < 0 || in_features < 1 || out_features < 1 || !x || !W || !b || !V || !c || !act_out || !ws)
    return wire_fail_(WIRE_ERR_ARG, "bad argument to wire_gabor2d_fwd");
  if (n == 0) return WIRE_OK;
  Layer l;
  if (int rc = l.open(WIRE_KIND_WIRE2D, stream, x, W, b, V, c, omega0, scale0, 1.f, n, in_features, out_features,
                      is_first, ws, ws_bytes))
    return rc;
  return layer_fwd(l, act_out);
}

extern "C" int wire_gabor2d_hparam_grad(void* stream, const void* g_act, const void* x, const void* W, const void* b,
                                        const void* V, const void* c, float omega0, float scale0, int64_t n,
                                        int in_features, int out_features, int is_first, float* out2, void* ws,
                                        int64_t ws_bytes) {
  if (n <= 0 || in_features < 1 || out_features < 1 || !g_act || !x || !W || !b || !V || !c || !out2 || !ws)
    return wire_fail_(WIRE_ERR_ARG, "bad argument to wire_gabor2d_hparam_grad");
  Layer l;
  if (int rc = l.open(WIRE_KIND_WIRE2D, stream, x, W, b, V, c, omega0, scale0, 1.f, n, in_features, out_features,
                      is_first, ws, ws_bytes))
    return rc;
  return layer_hparam(l, g_act, out2);
}

extern "C" int wire_gabor2d_bwd(void* stream, const void* g_act, const void* x, const void* W, const void* b,
                                const void* V, const void* c, float omega0, float scale0, int64_t n,
                                int in_features, int out_features, int is_first, void* g_x, void* g_W, void* g_b,
                                void* g_V, void* g_c, void* ws, int64_t ws_bytes) {
  if (n <= 0 || in_features < 1 || out_features < 1 || !g_act || !x || !W || !b || !V || !c || !g_W || !g_b ||
      !g_V || !g_c || !ws)
    return wire_fail_(WIRE_ERR_ARG, "bad argument to wire_gabor2d_bwd");
  Layer l;
  if (int rc = l.open(WIRE_KIND_WIRE2D, stream, x, W, b, V, c, omega0, scale0, 1.f, n, in_features, out_features,
                      is_first, ws, ws_bytes))
    return rc;
  return layer_bwd(l, g_act, g_x, g_W, g_b, g_V, g_c);
}

// wire2d first layer with the coordinate gradient: g_x [n][in] f32 = g_u W + g_p V; g_W .. g_c NULL together = the
// coordinate gradient alone
extern "C" int wire_gabor2d_bwd_first_coords(void* stream, const void* g_act, const float* x, const float* W,
                                             const float* b, const float* V, const float* c, float omega0, float scale0,
                                             int64_t n, int in_features, int out_features, float* g_x, float* g_W,
                                             float* g_b, float* g_V, float* g_c, void* ws, int64_t ws_bytes) {
  const bool pg = g_W && g_b && g_V && g_c;
  if (n <= 0 || in_features < 1 || in_features > 4 || out_features < 1 || !g_act || !x || !W || !b || !V || !c ||
      !g_x || !ws || (!pg && (g_W || g_b || g_V || g_c)))
    return wire_fail_(WIRE_ERR_ARG, "bad argument to wire_gabor2d_bwd_first_coords");
  Layer l;
  if (int rc = l.open(WIRE_KIND_WIRE2D, stream, x, W, b, V, c, omega0, scale0, 1.f, n, in_features, out_features, 1,
                      ws, ws_bytes))
    return rc;
  return layer_bwd_first(l, g_act, g_x, g_W, g_b, g_V, g_c);
}
