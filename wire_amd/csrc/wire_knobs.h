// wire_knobs.h -- the library's tuning knobs: ids, and the one accessor every launcher reads them through.
// The table itself (key, environment variable, default, accepted values, and why each knob exists) is wire_knobs.hip.
#pragma once
#include <atomic>

// Order = the rows of kKnobs (wire_knobs.hip).  The ablation rows exist in every build so that objects compiled with and
// without the ablation switches agree on the ids; their keys are only reachable in the builds that read them.
enum Knob {
  K_COMPLEX_3M, K_SPLIT_BF16, K_SPLIT_F16, K_SPLIT_OUT, K_RECOMPUTE_OUT, K_FIRST_SUMS, K_FIRST_DN, K_BWD_LOOKAHEAD, K_FUSED_RSTORE, K_WGRAD_BATCH,
  K_FUSED_FWD, K_FUSED_TRAIN, K_FUSED_TRAIN_P384, K_FUSED_FINAL, K_FUSED_BWD, K_FUSED_BWD_W,
  K_NT_BK, K_X2_AMODE, K_NT_BFIRST, K_EPI_EARLY, K_X2_TN_ROWS, K_X2_TN_P384, K_X3_TALL, K_X3_TALL_REAL, K_X3_TN_TALL, K_X3_TN16, K_X3_H16,
  K_X3H_STAGGER,
  K_FX_ABLATE, K_FXB_ABLATE, K_TN_ABL,
  K_COUNT
};

// relaxed atomics: wire_tune_set may run on one thread while autograd's thread reads a knob inside a launch sequence
extern std::atomic<int> g_knob[K_COUNT];
inline int knob(Knob k) { return g_knob[k].load(std::memory_order_relaxed); }

// by key (wire_tune_get / wire_tune_set; the timing harnesses under tools/ call knob_set directly):
int knob_get(const char* key);              // value, -1 = unknown key (every accepted value is >= 0)
int knob_set(const char* key, int value);   // 0, -1 = unknown key or a value the knob does not accept
