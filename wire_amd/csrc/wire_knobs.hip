// wire_knobs.hip -- the tuning knobs of libwire_hip.so: one row per knob, read from the environment once at load with the
// validation wire_tune_set applies (a rejected value keeps the default and is named on stderr), then read through
// knob() (wire_knobs.h) and changed through wire_tune_set (wire_api.hip).
#include <cerrno>
#include <climits>
#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <string>

#include "wire_knobs.h"

std::atomic<int> g_knob[K_COUNT];

namespace {
struct KnobDef {
  Knob id;
  const char* key;   // wire_tune_get / wire_tune_set; nullptr = environment only
  const char* env;   // nullptr = wire_tune_set only
  int dflt;
  bool flag;         // any integer, stored as value != 0; otherwise the value must be
  int lo, hi;        //   in lo .. hi (empty when lo > hi), or
  int a, b;          //   a or b (-1 = none)
};
constexpr KnobDef flag_knob(Knob id, const char* key, const char* env, int dflt) { return {id, key, env, dflt, true, 0, 1, -1, -1}; }
constexpr KnobDef range_knob(Knob id, const char* key, const char* env, int dflt, int lo, int hi, int a = -1) {
  return {id, key, env, dflt, false, lo, hi, a, -1};
}
constexpr KnobDef choice_knob(Knob id, const char* key, const char* env, int dflt, int a, int b) { return {id, key, env, dflt, false, 1, 0, a, b}; }
constexpr bool accepts(const KnobDef& d, int v) {
  return d.flag || (d.lo <= v && v <= d.hi) || (v >= 0 && (v == d.a || v == d.b));
}
#ifdef WIRE_FX_ABLATE
#define FX_ABLATE_KEY(k) k
#else
#define FX_ABLATE_KEY(k) nullptr
#endif

constexpr KnobDef kKnobs[] = {
    // ---- GEMM family
    // wire: 3-multiplication complex GEMMs on the fp32 MFMA (wire_gemm3m.hip)
    flag_knob(K_COMPLEX_3M, "complex_3m", nullptr, 1),
    // every net: split-bf16 GEMMs on the bf16 MFMA (wire_gemmx3.hip); overrides complex_3m
    flag_knob(K_SPLIT_BF16, "split_bf16", "WIRE_SPLIT_BF16", 1),
    // hidden-layer GEMMs of batches >= 4096 rows as a 2 x fp16 split on the f16 MFMA (wire_gemmx2h.hip): 3 instead of 6
    // matrix-core products per fp32 product, operand scales from device-side maxima; needs split_bf16 and the 16 x 16 x 32
    // kernels (x3_h16) for the net kind, falls back to the 3 x bf16 kernels otherwise
    flag_knob(K_SPLIT_F16, "split_f16", "WIRE_SPLIT_F16", 1),
    // ---- storage formats of the activations (make_plan snapshots these: a forward and its backward agree on them)
    // with split_f16: activations with an a-priori bound (Gabor, sine, Gaussian outputs) are stored ALREADY SPLIT into fp16
    // pairs by the epilogue that produces them (wire_dev.h: wire_store_out4), so the GEMMs that read them -- the next layer's
    // forward, the weight gradient -- spend no vector instructions on the split (wire_api.hip: make_route, out_scale)
    flag_knob(K_SPLIT_OUT, "split_out", "WIRE_SPLIT_OUT", 1),
    // wire training step on the 16 x 16 x 32 kernels: backward passes evaluate out = act(lin) again instead of reading it
    // (the data-gradient epilogues and the fused final stage), and the last hidden layer does not store out at all
    flag_knob(K_RECOMPUTE_OUT, "recompute_out", "WIRE_RECOMPUTE_OUT", 1),
    // on the 16 x 16 x 32 kernels the last data-gradient GEMM's epilogue forms the first layer's gradient sums itself
    // instead of storing g_u for a separate reduction pass
    flag_knob(K_FIRST_SUMS, "first_sums", "WIRE_FIRST_SUMS", 1),
    // wire / wire2d, that epilogue at D = 2 or 3: the edition with D a compile-time constant (no zero terms in the chains
    // over the input width), the tile's coordinates loaded once per wave and the first layer's parameters of both column
    // groups loaded ahead of the arithmetic (wire_gemmh_epi.h: h_gabor_bwd_first_dn).  0 = the plain edition; same bits.
    // Headline step, one process, alternating blocks (profiles/r05_dgrad_events_ab.txt): the four data-gradient launches
    // 1.829 -> 1.772 ms by events
    flag_knob(K_FIRST_DN, "first_dn", "WIRE_FIRST_DN", 1),
    // wire, the hidden layers' data-gradient epilogue on the 16 x 16 x 32 kernels: lin of the next 16-row block is loaded
    // ahead of the current block's arithmetic and stores (wire_gemmh_epi.h: h_gabor_bwd_la).  0 = load, compute, store per
    // block; same bits.  The four data-gradient launches 1.848 -> 1.787 ms by events; both knobs: step 5.585 -> 5.503 ms
    // (profiles/r05_dgrad_events_ab.txt, r05_knob_ab.txt)
    flag_knob(K_BWD_LOOKAHEAD, "bwd_lookahead", "WIRE_BWD_LOOKAHEAD", 1),
    // with the fused training forward + data-gradient chain of a sine / Gaussian net: store r = c lin and no out_l
    flag_knob(K_FUSED_RSTORE, "fused_rstore", "WIRE_FUSED_RSTORE", 1),
    // behind the data-gradient chain: the weight gradients of layers 2 .. L as one launch
    flag_knob(K_WGRAD_BATCH, "wgrad_batch", "WIRE_WGRAD_BATCH", 1),
    // ---- the whole-net kernels (wire_fused.hip)
    // 1 = forward-only calls of the shapes with a fused kernel (fused_fwd_shape) run it
    range_knob(K_FUSED_FWD, "fused_fwd", "WIRE_FUSED_FWD", 1, 0, 1),
    // 1 = training forwards of those nets run it too (storing lin_l / out_l); needs fused_fwd
    range_knob(K_FUSED_TRAIN, "fused_train", "WIRE_FUSED_TRAIN", 1, 0, 1),
    // 1 = also for wire at P = 384 (K = 181), whose storing edition spills (wire_api.hip: make_route)
    flag_knob(K_FUSED_TRAIN_P384, "fused_train_p384", "WIRE_FUSED_TRAIN_P384", 0),
    // 1 = wire_train_fwd_bwd of the real nets forms loss, dL/dy, g_lin_L and the final layer's gradient sums inside the
    // training forward (fx_tail_loss) instead of a pass over the stored lin_L / out_L.  Default 0: measured neutral to
    // slower (siren 2.05 / 2.03, gauss 2.02 / 1.94, relu 1.95 / 1.93 ms per step with / without,
    // profiles/r04_fused_final_ab.txt) -- the 0.18 ms pass it removes is HBM-bound and cheap, the tail it adds (3500 vector
    // instructions per wave, a third of them the 16-row sums of dL/dy^T h_L by DPP) runs with the matrix cores idle
    range_knob(K_FUSED_FINAL, "fused_final", "WIRE_FUSED_FINAL", 0, 0, 1),
    // the data-gradient chain in one kernel (real nets, P = 256); needs fused_train
    range_knob(K_FUSED_BWD, "fused_bwd", "WIRE_FUSED_BWD", 1, 0, 1),
    // its waves per workgroup.  8: one workgroup per CU, ring of three stages.  4: TWO workgroups of 64 rows per CU, each
    // with a ring of two stages (2 x 64 KB of LDS) -- they share nothing, so one's epilogue (no MFMAs: the link's
    // activation derivative, maxima, splits) runs beside the other's MFMAs, which the two waves of a SIMD inside ONE
    // workgroup cannot do (they meet at every stage barrier); price: the weight stream is fetched per 64 rows instead of
    // per 128.  (A/B on three nets, two rounds each: no difference -- profiles/r04_fused_bwd_w_ab.txt)
    choice_knob(K_FUSED_BWD_W, "fused_bwd_w", "WIRE_FUSED_BWD_W", 8, 4, 8),
    // ---- GEMM shapes and editions
    // K-slab depth of the fp32 4M NT kernel (wire_gemm.hip)
    choice_knob(K_NT_BK, "nt_bk", "WIRE_NT_BK", 16, 16, 32),
    // 2 x fp16 NT GEMM, how A is read.  A/B in one process and on one box (profiles/r03_gemm_x2_nt_tn_ab.txt, N = 262 144,
    // K = 256 complex): A through registers 0.452 / 0.539 / 0.559 ms (store / Gabor forward / data gradient) against
    // 0.470 / 0.556 / 0.563 through LDS.  Measured and dropped (profiles/r03_gemm_x2_prefetch_ablation.txt): an L2 prefetch
    // of the rows three stages ahead (+ 0.02 ms: the cost of the HBM reads is not their latency -- with every A row served
    // from cache the store form takes 0.347 ms, i.e. the 0.54 GB of A cost 0.105 ms, what they cost at 5 TB/s beside a
    // matrix pipe that shares the chip's power budget).  Round 3, late: A through the wave-private LDS region in WHOLE
    // cache lines (AMODE 2, default): 0.382 / 0.496 / 0.519 ms -- the half-line pieces of AMODE 0 and the fragment-shaped
    // register loads of AMODE 1 (16 rows x 64 bytes per instruction) put twice the line requests on the vector-memory path
    // for the same bytes (profiles/r03_gemm_x2_whole_line.txt).
    range_knob(K_X2_AMODE, "x2_amode", "WIRE_X2_AMODE", 2, 0, 2),
    // 2 x fp16 NT GEMM, A through LDS (x2_amode 2 and 0): a stage's weight pieces are issued BEFORE the wave's own rows and
    // the stage-end wait leaves the rows in flight (s_waitcnt vmcnt(2 NRB) ahead of s_barrier): the barrier publishes the
    // shared weight stage only, and a wave waits for its own rows alone, at the top of the next stage, ahead of the
    // ds_reads of its private region.  0 = rows first, vmcnt(0) ahead of the barrier: all four waves of a workgroup wait
    // for the slowest wave's rows at every stage.  Same bits.  (make_plan snapshots this and epi_early)
    flag_knob(K_NT_BFIRST, "nt_bfirst", "WIRE_NT_BFIRST", 1),
    // 2 x fp16 NT GEMM, x2_amode 2, wire's data-gradient forms: the epilogue's first loads go out under the MFMAs of the
    // last stage, into the registers the raw rows leave free -- EPI_GABOR_BWD with look-ahead: lin of row block 0; the
    // layer-1 form at D = 2: the lane's coordinates and W0 / b0 of both column groups (wire_gemmh_epi.h: h_pre_load).
    // 0 = the epilogue loads them itself.  Same bits.
    flag_knob(K_EPI_EARLY, "epi_early", "WIRE_EPI_EARLY", 1),
    // upper bound on the rows ONE 2 x fp16 weight-gradient workgroup accumulates sequentially in its fp32 accumulators
    // (0 = the fill-the-chip policy of gemmx2_tn_splits alone).  A shorter chain means more row splits, i.e. more slabs
    // for wgrad_reduce_kernel: the knob of the summation-order measurement (tools/wgrad_order_probe.py).
    range_knob(K_X2_TN_ROWS, "x2_tn_rows", "WIRE_X2_TN_ROWS", 0, 256, INT_MAX, 0),
    // waves of the 2 x fp16 weight-gradient workgroup at P = 384 (K = 181) -- 8 (default, round 4): 48 features of G per
    // wave, every SIMD carries two waves; 6: 64 features per wave (round 3)
    choice_knob(K_X2_TN_P384, "x2_tn_p384", "WIRE_X2_TN_P384", 8, 6, 8),
    // 256-row tiles (4 x 2 MFMA tiles per wave) in the split-bf16 NT kernel for the Gabor epilogues of large batches: fewer
    // weight bytes per MFMA through the 64 B/clk L1 path (tools/mfma_bf16_probe.hip), 7-9 % faster at N = 262144
    range_knob(K_X3_TALL, "x3_tall", "WIRE_X3_TALL", 1, 0, 1),
    // the same for siren / gauss / relu (A/B switch)
    range_knob(K_X3_TALL_REAL, "x3_tall_real", "WIRE_X3_TALL_REAL", 0, 0, 1),
    // 256 x 128 tiles in the split-bf16 weight-gradient kernel
    range_knob(K_X3_TN_TALL, "x3_tn_tall", "WIRE_X3_TN_TALL", 0, 0, 1),
    // 256 x 256 weight-gradient tiles on v_mfma_f32_16x16x32_bf16 when both padded widths are multiples of 256
    range_knob(K_X3_TN16, "x3_tn16", "WIRE_X3_TN16", 1, 0, 1),
    // the 16 x 16 x 32 edition of the split-bf16 NT GEMMs (wire_gemmx3h.hip) at M >= 4096 -- bit 0: forward / store
    // epilogues, bit 1: data-gradient epilogues.  In bench.py (same box, interleaved runs, profiles/r02_bench_h16_ab.txt):
    // forward launches 0.758 -> 0.700 ms, data gradient 0.749 -> 0.739 ms, step 9.93 -> 9.63 ms.  Bit 2: siren / gauss /
    // relu epilogues, bit 3: the 2-D Gabor epilogues (sweep A/B, same box: siren 72.4 -> 74.9, relu 81.9 -> 85.0,
    // wire2d 44.2 -> 47.6 M samples/s)
    range_knob(K_X3_H16, "x3_h16", "WIRE_X3_H16", 15, 0, 15),
    // late start of the 16 x 16 x 32 NT kernel's blocks 256 .. 511, in 100 MHz ticks (100 = 1 us)
    range_knob(K_X3H_STAGGER, "x3h_stagger", "WIRE_X3H_STAGGER", 0, 0, INT_MAX),
    // ---- timing probes, results wrong: the fused kernels' ablation switches (make EXTRA=-DWIRE_FX_ABLATE,
    // tools/fused_ablate.py, tools/fused_bwd_ablate.py) and the split-bf16 weight-gradient kernel's (-DWIRE_ABLATE_TN,
    // tools/build_tn_tune.sh: 1 no global loads, 2 no split / LDS stores, 4 no fragment reads, 8 no slab stores)
    range_knob(K_FX_ABLATE, FX_ABLATE_KEY("fx_ablate"), nullptr, 0, 0, 15),
    range_knob(K_FXB_ABLATE, FX_ABLATE_KEY("fxb_ablate"), nullptr, 0, 0, 127),
    range_knob(K_TN_ABL, nullptr, "WIRE_TN_ABL", 0, 0, 15),
};

constexpr bool rows_valid() {
  for (int i = 0; i < K_COUNT; ++i)
    if (kKnobs[i].id != i || !accepts(kKnobs[i], kKnobs[i].dflt)) return false;
  return true;
}
static_assert(sizeof kKnobs / sizeof kKnobs[0] == K_COUNT && rows_valid(), "one row per Knob, in enum order, default accepted");

const KnobDef* find(const char* key) {
  for (const KnobDef& d : kKnobs)
    if (d.key && !strcmp(d.key, key)) return &d;
  return nullptr;
}
std::string accepted(const KnobDef& d) {
  if (d.flag) return "any integer, 0 = off";
  std::string s;
  for (const int v : {d.a, d.b})
    if (v >= 0) s += (s.empty() ? "" : " or ") + std::to_string(v);
  if (d.lo <= d.hi) s += (s.empty() ? "" : " or ") + std::to_string(d.lo) + (d.hi == INT_MAX ? ".." : ".." + std::to_string(d.hi));
  return s;
}
int from_env(const KnobDef& d) {
  const char* s = d.env ? getenv(d.env) : nullptr;
  if (!s) return d.dflt;
  char* end = nullptr;
  errno = 0;
  const long v = strtol(s, &end, 10);
  if (end != s && *end == '\0' && errno == 0 && v >= INT_MIN && v <= INT_MAX && accepts(d, (int)v))
    return d.flag ? v != 0 : (int)v;
  fprintf(stderr, "libwire_hip: ignoring %s=%s (accepted: %s); using the default %d\n", d.env, s, accepted(d).c_str(), d.dflt);
  return d.dflt;
}
// (no other static initialiser reads a knob)
struct KnobLoader {
  KnobLoader() {
    for (const KnobDef& d : kKnobs) g_knob[d.id].store(from_env(d), std::memory_order_relaxed);
  }
} g_knob_loader;
}  // namespace

int knob_get(const char* key) {
  const KnobDef* d = find(key);
  return d ? knob(d->id) : -1;
}
int knob_set(const char* key, int value) {
  const KnobDef* d = find(key);
  if (!d || !accepts(*d, value)) return -1;
  g_knob[d->id].store(d->flag ? value != 0 : value, std::memory_order_relaxed);
  return 0;
}
