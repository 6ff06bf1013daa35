// wire_kinds.h -- the base net kinds, each described once: the codes its kernels are instantiated with and what the host
// decides from the kind.  constexpr only, no HIP: host and device code read the same table.
//
// Every value below is a template argument of some kernel and so part of that kernel's name (tests and profiles/ read
// those names): a new kind takes new values, an existing one keeps its own.
#pragma once
#include <cassert>
#include <cmath>

// the values of wire_kind (include/wire_hip.h) that reach a launcher: a plan's kind is handed on as it is, the composite
// kinds (multi-scale B-splines, mfn) rewritten onto one of these by make_plan
enum { NK_WIRE = 0, NK_WIRE2D = 1, NK_SIREN = 2, NK_GAUSS = 3, NK_RELU = 4, NK_BSPLINE = 5, NK_BSPLINE3 = 12 };

// the real-valued activations (wire_dev.h: real_act_fwd / real_act_bwd)
enum { ACT_SIREN = 0, ACT_GAUSS = 1, ACT_RELU = 2, ACT_BSPLINE = 3, ACT_BSPLINE3 = 4 };

// Epilogue selector of the NT GEMM  C[M][Nc] = A[M][Kd] * Bt[Nc][Kd]^T.
enum WireEpi {
  EPI_STORE = 0,            // o0 = C
  EPI_GABOR_FWD = 1,        // C = lin(re|im): o0 = lin (optional), o1 = gabor(lin + bias)
  EPI_GABOR_BWD = 2,        // C = g_out: i0 = lin, i1 = out -> o0 = g_lin
  EPI_GABOR_BWD_FIRST = 3,  // C = g_out0: i1 = out0, coords/W0/b0 -> u; o0 = g_u [M][ldu]
  EPI_SIREN_FWD = 4, EPI_GAUSS_FWD = 5, EPI_RELU_FWD = 6,   // o0 = lin, o1 = act
  EPI_SIREN_BWD = 7, EPI_GAUSS_BWD = 8, EPI_RELU_BWD = 9,   // i0 = lin, i1 = out -> o0 = g_lin
  EPI_GABOR2D_FWD = 10,     // C = (lin|sy)(re|im) 128-col groups: o0 = linsy [M][2P], o1 = out [M][P]
  EPI_GABOR2D_BWD = 11,     // C = g_out: i0 = linsy, i1 = out -> o0 = g_linsy [M][2P]
  EPI_GABOR2D_BWD_FIRST = 12, // real first layer of wire2d: o0 = g_(u|p) [M][2*ldu]
  EPI_BSPLINE_FWD = 13,     // quadratic B-spline (scale = c = 1 / |sigma0|): o0 = lin, o1 = act
  EPI_BSPLINE_BWD = 14,     // i0 = lin -> o0 = g_lin (no out read)
  // multiplicative filter network (modules/mfn.py:46-54): g = the Gabor filter of the row's coordinates (ep.coords,
  // ep.D) and the column's entry of the filter table (ep.ftab, wire_dev.h: MfnCol)
  EPI_MFN_FWD = 15,         // lin = C + bias: o0 = lin (optional), o1 = lin g
  EPI_MFN_BWD = 16,         // C = g_z: i0 = lin -> o0 = g_z g (the layer below's g_lin), o1 = g_z lin (the filter's
                            //   upstream gradient h); i0 null (filter 0): o1 = g_z alone
  EPI_BSPLINE3_FWD = 17,    // cubic B-spline of lin (scale_0 sits in the packed weights): o0 = lin, o1 = act
  EPI_BSPLINE3_BWD = 18,    // i0 = lin -> o0 = g_lin (no out read)
  // flag on the layer-1 data-gradient forms of the 16 x 16 x 32 kernels (the real BWD forms, GABOR_BWD_FIRST,
  // GABOR2D_BWD_FIRST): the instantiation that also writes ep.cg_partial.  Host code passes the plain code; the
  // launchers pick the flagged instantiation when ep.cg_partial is set
  EPI_CG = 64,
  // flags on GABOR_BWD_FIRST / GABOR2D_BWD_FIRST of the 16 x 16 x 32 kernels: the instantiations whose input width D is a
  // compile-time 2 or 3 (wire_gemmh_epi.h: h_gabor_bwd_first_dn, h_gabor2d_bwd_first_dn).  The launchers pick them when
  // ep.first_dn is set and ep.D is 2 or 3; every other D keeps the plain form
  EPI_D2 = 128, EPI_D3 = 256,
  // flag on GABOR_BWD of the 16 x 16 x 32 kernels: the edition whose epilogue loads the next row block's lin ahead of
  // the current block's arithmetic and stores (wire_gemmh_epi.h: h_gabor_bwd_la); picked when ep.lookahead is set
  EPI_LA = 512
};
constexpr int EPI_FLAGS = EPI_CG | EPI_D2 | EPI_D3 | EPI_LA;

// how scale_0 reaches the kernels (kind_scale below)
enum KindScale {
  SCALE_ASIS,      // handed on as it is
  SCALE_INV_ABS,   // a divisor of lin and the activation even: the kernels multiply by c = 1 / |sigma0|
  SCALE_WEIGHTS    // multiplies the layer's input, sign included: into the packed weights; the kernels' scale is 1
};

struct KindRow {
  int kind;             // NK_*
  const char* name;
  bool cplx;            // complex features in blocked-planar rows (2 K floats per row)
  int act;              // ACT_* of a real kind; 0 for the complex kinds, whose kernels never evaluate it
  int epi_fwd, epi_bwd; // hidden-layer epilogues of the NT GEMMs
  int z_act;            // ZMODE of gemmx2_tn16_kernel: its loader evaluates act(r) on the stored r (0: no such form)
  bool bwd_reads_out;   // real kinds: act'(lin) reads the stored out (gauss: -2 s^2 lin out; relu: [out > 0]); else lin alone
  bool rstore;          // whole-net training forward stores r = c lin and no out (z_act, the chain's branches)
  bool split_out_free;  // act' needs no out: out_l may be stored pre-split even without recompute_out
  bool lin0;            // the whole-net training forward stores lin_0 (the chain's last link reads it)
  bool presplit_a;      // the forward epilogue exists in the edition that reads a pre-split A (out bounded a priori)
  KindScale scale;
};
constexpr KindRow KINDS[] = {
  // kind         name             cplx   act           epi_fwd           epi_bwd           z_act out?   rstore split  lin0   pre-A  scale
  {NK_WIRE,     "wire",          true,  0,            EPI_GABOR_FWD,    EPI_GABOR_BWD,    0, false, false, false, false, true,  SCALE_ASIS},
  {NK_WIRE2D,   "wire2d",        true,  0,            EPI_GABOR2D_FWD,  EPI_GABOR2D_BWD,  0, false, false, false, false, true,  SCALE_ASIS},
  {NK_SIREN,    "siren",         false, ACT_SIREN,    EPI_SIREN_FWD,    EPI_SIREN_BWD,    2, false, true,  true,  true,  true,  SCALE_ASIS},
  {NK_GAUSS,    "gauss",         false, ACT_GAUSS,    EPI_GAUSS_FWD,    EPI_GAUSS_BWD,    3, true,  true,  false, true,  true,  SCALE_ASIS},
  {NK_RELU,     "relu",          false, ACT_RELU,     EPI_RELU_FWD,     EPI_RELU_BWD,     0, true,  false, false, false, false, SCALE_ASIS},
  {NK_BSPLINE,  "bspline",       false, ACT_BSPLINE,  EPI_BSPLINE_FWD,  EPI_BSPLINE_BWD,  4, false, true,  true,  true,  true,  SCALE_INV_ABS},
  {NK_BSPLINE3, "bspline_cubic", false, ACT_BSPLINE3, EPI_BSPLINE3_FWD, EPI_BSPLINE3_BWD, 5, false, true,  true,  true,  true,  SCALE_WEIGHTS},
};
constexpr int N_KINDS = sizeof(KINDS) / sizeof(KINDS[0]);

// ---- lookups (a miss is index N_KINDS / a null row: callers that take any int test it)
constexpr int kind_index(int kind) {
  for (int i = 0; i < N_KINDS; ++i) if (KINDS[i].kind == kind) return i;
  return N_KINDS;
}
constexpr const KindRow* kind_row(int kind) { return kind_index(kind) < N_KINDS ? &KINDS[kind_index(kind)] : nullptr; }
// the row of a kind its caller has validated (make_plan, kind_is_real, fused_fwd_shape): an unknown one stops here, it never
// runs another kind's kernel
inline const KindRow& known_kind(int kind) {
  const KindRow* row = kind_row(kind);
  assert(row && "kind outside wire_kinds.h");
  return *row;
}
constexpr bool kind_is_real(int kind) { return kind_row(kind) && !kind_row(kind)->cplx; }
constexpr bool kind_is_cplx(int kind) { return kind_row(kind) && kind_row(kind)->cplx; }
// the row whose forward / backward epilogue is e (real kinds only: the epilogues of wire_gemm_epi.h / wire_gemmh_epi.h
// branch on these before they look at the Gabor and mfn forms)
constexpr const KindRow* epi_real_row(int e, bool fwd) {
  for (int i = 0; i < N_KINDS; ++i)
    if (!KINDS[i].cplx && (fwd ? KINDS[i].epi_fwd : KINDS[i].epi_bwd) == e) return &KINDS[i];
  return nullptr;
}
constexpr bool epi_real_fwd(int e) { return epi_real_row(e, true) != nullptr; }
constexpr bool epi_real_bwd(int e) { return epi_real_row(e, false) != nullptr; }
constexpr int epi_real_act(int e) { return epi_real_fwd(e) ? epi_real_row(e, true)->act : epi_real_row(e, false)->act; }
constexpr int nk_real_act(int kind) { return kind_row(kind) ? kind_row(kind)->act : 0; }
// (a mask and not a walk through the table: epilogues ask this inside their loops, where it must stay a literal)
constexpr unsigned act_reads_out_mask() {
  unsigned m = 0;
  for (int i = 0; i < N_KINDS; ++i) if (!KINDS[i].cplx && KINDS[i].bwd_reads_out) m |= 1u << KINDS[i].act;
  return m;
}
constexpr unsigned ACT_READS_OUT = act_reads_out_mask();
constexpr bool act_bwd_reads_out(int act) { return (ACT_READS_OUT >> act) & 1u; }
// the loader branches of gemmx2_tn16_kernel and the ladder of launch_x2_tn_t (wire_gemmx2h.hip) run from 2 to Z_ACT_MAX
constexpr int Z_ACT_MAX = 5;
constexpr bool z_act_known(int z_act) {
  for (int i = 0; i < N_KINDS; ++i) if (z_act >= 2 && KINDS[i].z_act == z_act) return true;
  return false;
}
// forward forms that read an activation with an a-priori bound (EPI_STORE: the final linear on such an activation)
constexpr bool epi_presplit_a(int e) {
  for (int i = 0; i < N_KINDS; ++i) if (KINDS[i].epi_fwd == e) return KINDS[i].presplit_a;
  return e == EPI_STORE;
}
// the four forms of the 1-D Gabor net: all the 3M family and the 256-row tiles of wire_gemmx3.hip have
constexpr bool epi_wire_form(int e) {
  return e == EPI_STORE || e == EPI_GABOR_FWD || e == EPI_GABOR_BWD || e == EPI_GABOR_BWD_FIRST;
}

// (kind, scale_0 of the descriptor) -> the kernels' scale and the factor folded into the packed weights; false: the
// kind divides or multiplies by scale_0 and it is zero or not finite
inline bool kind_scale(int kind, float scale0, float& kscale, float& wscale) {
  const KindRow* row = kind_row(kind);
  kscale = scale0; wscale = 1.f;
  if (!row || row->scale == SCALE_ASIS) return true;
  if (!(std::isfinite(scale0) && scale0 != 0.f)) return false;
  if (row->scale == SCALE_WEIGHTS) { wscale = scale0; kscale = 1.f; }
  else kscale = (float)(1.0 / std::fabs((double)scale0));
  return true;
}

// ---- what a mistyped row would break
constexpr bool kinds_table_ok() {
  for (int i = 0; i < N_KINDS; ++i) {
    const KindRow& a = KINDS[i];
    for (int j = 0; j < i; ++j) {
      const KindRow& b = KINDS[j];
      if (a.kind == b.kind || a.epi_fwd == b.epi_fwd || a.epi_bwd == b.epi_bwd || a.epi_fwd == b.epi_bwd ||
          a.epi_bwd == b.epi_fwd)
        return false;
      if (!a.cplx && !b.cplx && a.act == b.act) return false;
      if (a.z_act && a.z_act == b.z_act) return false;
    }
    if (a.epi_fwd == a.epi_bwd || ((a.epi_fwd | a.epi_bwd) & EPI_FLAGS)) return false;
    if (a.z_act == 1 || a.z_act < 0 || a.z_act > Z_ACT_MAX) return false;                       // 0 / 1: the loader's fp32 and pre-split forms
    if (a.rstore && (a.z_act == 0 || a.cplx || !a.lin0)) return false;   // the loader and the chain evaluate on r
    if (a.split_out_free && a.bwd_reads_out) return false;
    if (!a.cplx) {                                                       // kind -> epi -> act comes back to the row
      if (!epi_real_fwd(a.epi_fwd) || !epi_real_bwd(a.epi_bwd) || epi_real_fwd(a.epi_bwd) || epi_real_bwd(a.epi_fwd))
        return false;
      if (epi_real_act(a.epi_fwd) != a.act || epi_real_act(a.epi_bwd) != a.act || nk_real_act(a.kind) != a.act) return false;
      if (act_bwd_reads_out(a.act) != a.bwd_reads_out) return false;
    } else if (epi_real_fwd(a.epi_fwd) || epi_real_bwd(a.epi_bwd)) {
      return false;
    }
    if (kind_row(a.kind) != &a) return false;
  }
  return true;
}
static_assert(kinds_table_ok(), "wire_kinds.h: a code is used twice, or a row does not round-trip kind -> epilogue -> activation");
