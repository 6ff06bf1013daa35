// wire_render.hip -- emission-absorption volume rendering of a 3-D net along camera rays: the sampler that turns rays
// into the net's input rows, the compositing of the net's rows into one colour per ray, its adjoint, and the loss
// kernel of FusedTrainer.step_rays.
//
// A ray r has S samples; the net's row of sample s is y[r S + s] = (c_raw[0..C), s_raw), C = O - 1.  With
//   sigma = softplus(s_raw) (density mode 0) or max(s_raw, 0) (mode 1),   c = sigmoid(c_raw),   a_s = sigma_s delta_s,
//   tau_s = sum_{j<s} a_j,   T_s = exp(-tau_s),   w_s = T_s (1 - exp(-a_s)),   T_S = exp(-tau_S):
//   rgb = sum_s w_s c_s + T_S bg,   acc = 1 - T_S,   depth = sum_s w_s t_s.
// ADJOINT: for the linear functional F = <g_rgb, rgb> + g_acc acc + g_depth depth write
//   q_s = <c_s, g_rgb> + t_s g_depth,   q_bg = <bg, g_rgb> - g_acc        (acc = 1 - T_S enters through T_S alone)
// and use dw_s/dsigma_s = delta_s T_{s+1}, dw_j/dsigma_s = -delta_s w_j (j > s), dT_S/dsigma_s = -delta_s T_S:
//   dF/dsigma_s = delta_s ( T_{s+1} q_s - sum_{j>s} w_j q_j - T_S q_bg ),   dF/dc_raw_s = w_s g_rgb (.) c (1 - c).
// (Putting g_acc into q_s as well -- acc = sum_s w_s -- would count it twice.)
//
// SHAPE: a ray's rows are S O consecutive floats.  A wave owns a ray and its lanes own consecutive samples, 64 at a
// time: a lane moves its row as 16- or 8-byte words where O allows (O = 4, 8: float4; 2, 6: float2), so a wave reads
// and writes 64 O consecutive floats.  A workgroup is four waves = RENDER_RAYS_PER_WG rays.  tau is an inclusive
// __shfl_up scan of a_s inside a chunk plus a carry across chunks; the carries of the first 64 chunks stay in a register
// of lane k (chunk k), later ones are recomputed from chunk 63's.  The adjoint walks the chunks from the last to the
// first with a __shfl_down suffix scan of w_j q_j and its own carry: a reverse sweep, never "total minus prefix",
// which cancels on opaque rays.
// PRECISION: a_s, tau, T, w, the sums over samples and the suffix sum are fp64 (each a_s = sigma delta is exact in
// fp64); softplus, sigmoid and the rows are fp32; every output is rounded to fp32 once.  exp(-tau) underflows to 0 in
// fp64 without an inf on the way (tau is capped at RENDER_TAU_CAP, beyond which exp is 0 in fp64 anyway), 1 - exp(-a)
// is -expm1(-a), and softplus takes no exponential of a positive argument: finite for every finite input.
// SUMS: a lane adds its samples chunk by chunk, the wave by the __shfl_xor tree (wire_wave_sum); the loss kernel walks
// rays r = 4 block + wave, + 4 grid, ..., a wave adding its rays' squared residuals in that order, the four waves as
// (w0 + w1) + (w2 + w3) into partial[block], launch_mse_final adds the blocks.  No atomics and no last-block counter:
// which lane adds what, in which order, depends on (R, S, O) alone.
// wire_composite_mse_grad is built from the functions of the forward / backward pair (ray_forward, ray_backward), so
// both routes give the same bits.
//
//
// HIERARCHICAL SAMPLING: wire_composite_weights writes the w_s of the forward sweep, and
// wire_ray_resample turns them into a second set of samples: a per-ray unnormalised CDF over the bins whose edges are the
// midpoints of the coarse samples, Nf inverse-CDF draws, and a merge by rank with the coarse samples.  A wave owns a
// ray there too; the CDF, the fine samples and the merged list live in LDS (layout and occupancy at the kernel).
//
// The six entry points of the C ABI (include/wire_hip.h) are at the end of this file.
#include <cfloat>
#include <cmath>

#include "wire_dev.h"
#include "wire_plan.h"

#define RENDER_RAYS_PER_WG 4            // one wave each
#define RENDER_LOSS_BLOCKS 2048         // the grid of the loss kernel is capped here: partial holds one float per block
#define RENDER_MAX_BLOCKS 2147483647ll
#define RENDER_TAU_CAP 800.0            // exp(-800) == 0 in fp64
#define RESAMPLE_MAX 1024               // the resampler's limit on S and on Nf: its CDF and lists live in LDS
#define RESAMPLE_SMALL 256              // up to here four rays share a workgroup, beyond it two

// ---------------------------------------------------------------------------
// the sampler
// ---------------------------------------------------------------------------
__global__ __launch_bounds__(256) void ray_samples_kernel(const float* __restrict__ rays,
                                                          const float* __restrict__ bounds, float near_, float far_,
                                                          const float* __restrict__ jitter, long long R, int S,
                                                          float* __restrict__ coords, float* __restrict__ ts,
                                                          float* __restrict__ deltas) {
#pragma clang fp contract(off)
  const long long e = (long long)blockIdx.x * 256 + threadIdx.x;
  if (e >= R * S) return;
  const long long r = e / S;
  const int s = (int)(e - r * S);
  const float* ray = rays + r * 6;
  const double ox = (double)ray[0], oy = (double)ray[1], oz = (double)ray[2];
  const double dx = (double)ray[3], dy = (double)ray[4], dz = (double)ray[5];
  const double nr = (double)(bounds ? bounds[2 * r] : near_), fr = (double)(bounds ? bounds[2 * r + 1] : far_);
  double t = nr, dl = 0.0;
  if (fr > nr) {
    const double u0 = jitter ? (double)jitter[e] : 0.5;
    t = nr + (((double)s + u0) * (fr - nr)) / (double)S;
    double t1 = fr;
    if (s + 1 < S) {
      const double u1 = jitter ? (double)jitter[e + 1] : 0.5;
      t1 = nr + (((double)(s + 1) + u1) * (fr - nr)) / (double)S;
    }
    dl = (t1 - t) * sqrt(dx * dx + dy * dy + dz * dz);
  }
  coords[3 * e + 0] = (float)(ox + t * dx);
  coords[3 * e + 1] = (float)(oy + t * dy);
  coords[3 * e + 2] = (float)(oz + t * dz);
  ts[e] = (float)t;
  deltas[e] = (float)dl;
}

// ---------------------------------------------------------------------------
// one lane, one row
// ---------------------------------------------------------------------------
template <int O>
WIRE_DEVINL void row_load(const float* __restrict__ p, float (&v)[O]) {
  if (O % 4 == 0) {
#pragma unroll
    for (int k = 0; k < O / 4; ++k) {
      const float4 q = ((const float4*)p)[k];
      v[4 * k] = q.x; v[4 * k + 1] = q.y; v[4 * k + 2] = q.z; v[4 * k + 3] = q.w;
    }
  } else if (O % 2 == 0) {
#pragma unroll
    for (int k = 0; k < O / 2; ++k) {
      const float2 q = ((const float2*)p)[k];
      v[2 * k] = q.x; v[2 * k + 1] = q.y;
    }
  } else {
#pragma unroll
    for (int k = 0; k < O; ++k) v[k] = p[k];
  }
}
template <int O>
WIRE_DEVINL void row_store(float* __restrict__ p, const float (&v)[O]) {
  if (O % 4 == 0) {
#pragma unroll
    for (int k = 0; k < O / 4; ++k) ((float4*)p)[k] = make_float4(v[4 * k], v[4 * k + 1], v[4 * k + 2], v[4 * k + 3]);
  } else if (O % 2 == 0) {
#pragma unroll
    for (int k = 0; k < O / 2; ++k) ((float2*)p)[k] = make_float2(v[2 * k], v[2 * k + 1]);
  } else {
#pragma unroll
    for (int k = 0; k < O; ++k) p[k] = v[k];
  }
}

// e = exp(-|x|) in (0, 1]: wire_exp takes finite arguments, and e^-128 is 0 in fp32 (the logistic loss's recipe)
WIRE_DEVINL float render_expneg(float x) { return wire_exp(-fminf(fabsf(x), 128.f)); }
WIRE_DEVINL float render_sigmoid(float x) {
  const float e = render_expneg(x);
  return x >= 0.f ? 1.f / (1.f + e) : e / (1.f + e);
}
// sigma and d sigma / d s_raw
WIRE_DEVINL void render_density(float x, int mode, float& sigma, float& dsigma) {
  if (mode == 0) {
    sigma = fmaxf(x, 0.f) + log1pf(render_expneg(x));
    dsigma = render_sigmoid(x);
  } else {
    sigma = fmaxf(x, 0.f);
    dsigma = x > 0.f ? 1.f : 0.f;
  }
}

// inclusive scans over the lanes of a wave: towards higher lanes (prefix) and towards lower lanes (suffix)
WIRE_DEVINL double wave_prefix_incl(double v, int lane) {
#pragma unroll
  for (int o = 1; o < 64; o <<= 1) {
    const double t = __shfl_up(v, o);
    if (lane >= o) v += t;
  }
  return v;
}
WIRE_DEVINL double wave_suffix_incl(double v, int lane) {
#pragma unroll
  for (int o = 1; o < 64; o <<= 1) {
    const double t = __shfl_down(v, o);
    if (lane + o < 64) v += t;
  }
  return v;
}

// One chunk of 64 samples of a ray, this lane's sample s = base + lane: the row, c = sigmoid(c_raw), t_s, delta_s,
// d sigma / d s_raw and a_s = sigma_s delta_s (lanes past the ray's end: a = 0, delta = 0, valid = false).
template <int O>
struct RayLane {
  float c[O - 1];
  float t, delta, dsigma;
  double a;
  bool valid;
};
template <int O>
WIRE_DEVINL void ray_lane_load(const float* __restrict__ y, const float* __restrict__ ts,
                               const float* __restrict__ deltas, long long row0, int S, int base, int lane, int mode,
                               RayLane<O>& L) {
#pragma clang fp contract(off)
  const int s = base + lane;
  L.valid = s < S;
  L.a = 0.0;
  L.t = 0.f; L.delta = 0.f; L.dsigma = 0.f;
#pragma unroll
  for (int k = 0; k < O - 1; ++k) L.c[k] = 0.f;
  if (L.valid) {
    float v[O];
    row_load<O>(y + (row0 + s) * O, v);
#pragma unroll
    for (int k = 0; k < O - 1; ++k) L.c[k] = render_sigmoid(v[k]);
    float sigma;
    render_density(v[O - 1], mode, sigma, L.dsigma);
    L.t = ts[row0 + s];
    L.delta = deltas[row0 + s];
    L.a = (double)sigma * (double)L.delta;
  }
}
// a_s alone (the carries past chunk 63)
template <int O>
WIRE_DEVINL double ray_lane_a(const float* __restrict__ y, const float* __restrict__ deltas, long long row0, int S,
                              int base, int lane, int mode) {
  const int s = base + lane;
  if (s >= S) return 0.0;
  float sigma, ds;
  render_density(y[(row0 + s) * O + (O - 1)], mode, sigma, ds);
  return (double)sigma * (double)deltas[row0 + s];
}

// What the forward sweep of a ray leaves in every lane of its wave.
template <int O>
struct RayOut {
  double rgb[O - 1];      // sum_s w_s c_s (the background is not in it)
  double depth, tau;      // sum_s w_s t_s, tau_S
  double carries;         // lane k: tau at the start of chunk k, k < 64
};

template <int O>
WIRE_DEVINL void ray_forward(const float* __restrict__ y, const float* __restrict__ ts,
                             const float* __restrict__ deltas, long long r, int S, int mode, int lane, RayOut<O>& F) {
#pragma clang fp contract(off)
  const long long row0 = r * S;
  double carry = 0.0;
  F.carries = 0.0;
  F.depth = 0.0;
#pragma unroll
  for (int k = 0; k < O - 1; ++k) F.rgb[k] = 0.0;
  for (int base = 0, ch = 0; base < S; base += 64, ++ch) {
    if (lane == ch) F.carries = carry;
    RayLane<O> L;
    ray_lane_load<O>(y, ts, deltas, row0, S, base, lane, mode, L);
    const double incl = wave_prefix_incl(L.a, lane);
    const double T = exp(-fmin(carry + (incl - L.a), RENDER_TAU_CAP));
    const double w = T * -expm1(-L.a);
#pragma unroll
    for (int k = 0; k < O - 1; ++k) F.rgb[k] += w * (double)L.c[k];
    F.depth += w * (double)L.t;
    carry += __shfl(incl, 63);
  }
#pragma unroll
  for (int k = 0; k < O - 1; ++k) F.rgb[k] = wire_wave_sum(F.rgb[k]);
  F.depth = wire_wave_sum(F.depth);
  F.tau = carry;
}

// tau at the start of chunk ch: the forward sweep's own sequence of additions
template <int O>
WIRE_DEVINL double ray_carry(const float* __restrict__ y, const float* __restrict__ deltas, long long row0, int S,
                             int mode, int lane, double carries, int ch) {
  if (ch < 64) return __shfl(carries, ch);
  double c = __shfl(carries, 63);
  for (int j = 63; j < ch; ++j)
    c += __shfl(wave_prefix_incl(ray_lane_a<O>(y, deltas, row0, S, j * 64, lane, mode), lane), 63);
  return c;
}

// The adjoint of a ray: every element of its S rows of g_y.  g_rgb, g_acc, g_depth and bg are the same in every lane.
template <int O>
WIRE_DEVINL void ray_backward(const float* __restrict__ y, const float* __restrict__ ts,
                              const float* __restrict__ deltas, const float* __restrict__ bg, long long r, int S,
                              int mode, int lane, const RayOut<O>& F, const float (&g_rgb)[O - 1], float g_acc,
                              float g_depth, float* __restrict__ g_y) {
#pragma clang fp contract(off)
  const long long row0 = r * S;
  double q_bg = -(double)g_acc;
  if (bg) {
#pragma unroll
    for (int k = 0; k < O - 1; ++k) q_bg += (double)bg[k] * (double)g_rgb[k];
  }
  const double tail = exp(-fmin(F.tau, RENDER_TAU_CAP)) * q_bg;         // T_S q_bg
  double after = 0.0;                                                    // sum of w_j q_j over the later chunks
  for (int ch = (S - 1) / 64; ch >= 0; --ch) {
    const int base = ch * 64;
    const double carry = ray_carry<O>(y, deltas, row0, S, mode, lane, F.carries, ch);
    RayLane<O> L;
    ray_lane_load<O>(y, ts, deltas, row0, S, base, lane, mode, L);
    const double incl = wave_prefix_incl(L.a, lane);
    const double T = exp(-fmin(carry + (incl - L.a), RENDER_TAU_CAP));
    const double T1 = exp(-fmin(carry + incl, RENDER_TAU_CAP));
    const double w = T * -expm1(-L.a);
    double q = (double)L.t * (double)g_depth;
#pragma unroll
    for (int k = 0; k < O - 1; ++k) q += (double)L.c[k] * (double)g_rgb[k];
    const double sfx = wave_suffix_incl(w * q, lane);
    double later = __shfl_down(sfx, 1);
    if (lane == 63) later = 0.0;
    later += after;
    if (L.valid) {
      float g[O];
#pragma unroll
      for (int k = 0; k < O - 1; ++k)
        g[k] = (float)((w * (double)g_rgb[k]) * ((double)L.c[k] * (1.0 - (double)L.c[k])));
      g[O - 1] = (float)(((double)L.delta * ((T1 * q - later) - tail)) * (double)L.dsigma);
      row_store<O>(g_y + (row0 + base + lane) * O, g);
    }
    after += __shfl(sfx, 0);
  }
}

// ---------------------------------------------------------------------------
// kernels: a wave per ray
// ---------------------------------------------------------------------------
template <int O>
WIRE_DEVINL void ray_rgb(const RayOut<O>& F, const float* __restrict__ bg, float (&rgb)[O - 1]) {
#pragma clang fp contract(off)
  const double TS = exp(-fmin(F.tau, RENDER_TAU_CAP));
#pragma unroll
  for (int k = 0; k < O - 1; ++k) rgb[k] = (float)(bg ? F.rgb[k] + TS * (double)bg[k] : F.rgb[k]);
}

template <int O>
__global__ __launch_bounds__(256) void composite_fwd_kernel(const float* __restrict__ y, const float* __restrict__ ts,
                                                            const float* __restrict__ deltas,
                                                            const float* __restrict__ bg, long long R, int S, int mode,
                                                            float* __restrict__ rgb, float* __restrict__ acc,
                                                            float* __restrict__ depth) {
  const int lane = threadIdx.x & 63;
  const long long r = (long long)blockIdx.x * RENDER_RAYS_PER_WG + (threadIdx.x >> 6);
  if (r >= R) return;                                      // (a whole wave leaves: no barrier below)
  RayOut<O> F;
  ray_forward<O>(y, ts, deltas, r, S, mode, lane, F);
  float c[O - 1];
  ray_rgb<O>(F, bg, c);
  if (lane < O - 1) {
    float v = c[0];
#pragma unroll
    for (int k = 1; k < O - 1; ++k) v = lane == k ? c[k] : v;
    rgb[r * (O - 1) + lane] = v;
  }
  if (lane == 0) {
    if (acc) acc[r] = (float)(-expm1(-fmin(F.tau, RENDER_TAU_CAP)));
    if (depth) depth[r] = (float)F.depth;
  }
}

// w_s alone, for the resampler: the scan, carry and expressions of ray_forward on column O - 1 of y, so w carries the
// bits of the forward sweep's summand.  O is a run-time number here: no row is moved, only its last float.
__global__ __launch_bounds__(256) void composite_weights_kernel(const float* __restrict__ y,
                                                                const float* __restrict__ deltas, long long R, int S,
                                                                int O, int mode, float* __restrict__ w) {
#pragma clang fp contract(off)
  const int lane = threadIdx.x & 63;
  const long long r = (long long)blockIdx.x * RENDER_RAYS_PER_WG + (threadIdx.x >> 6);
  if (r >= R) return;                                      // (a whole wave leaves: no barrier below)
  const long long row0 = r * S;
  double carry = 0.0;
  for (int base = 0; base < S; base += 64) {
    const int s = base + lane;
    double a = 0.0;
    if (s < S) {
      float sigma, ds;
      render_density(y[(row0 + s) * O + (O - 1)], mode, sigma, ds);
      a = (double)sigma * (double)deltas[row0 + s];
    }
    const double incl = wave_prefix_incl(a, lane);
    const double T = exp(-fmin(carry + (incl - a), RENDER_TAU_CAP));
    if (s < S) w[row0 + s] = (float)(T * -expm1(-a));
    carry += __shfl(incl, 63);
  }
}

// ---------------------------------------------------------------------------
// the resampler: inverse-CDF draws from the coarse weights, merged with the coarse samples
// ---------------------------------------------------------------------------
// A wave owns a ray.  LDS per ray, for S, Nf <= CAP:
//   tc [CAP]       float    the coarse samples (the merge's searches; the bin edges are their midpoints)
//   tf [CAP]       double   the fine samples, unrounded
//   cm [2 CAP + 2] double   first the CDF c_0 .. c_S, then -- the CDF is dead once the draws are inverted -- the merged
//                           list t_0 .. t_{S+Nf-1} with far behind it, so a lane reads its right neighbour
// = 28 CAP + 16 bytes.  Two editions: CAP = 256 with four rays per workgroup (28.1 KB: five workgroups = 20 waves per
// CU of 160 KB LDS) and CAP = 1024 with two rays (56.0 KB: two workgroups = 4 waves per CU).  A ray's arithmetic does
// not depend on the edition.  Every wave of a workgroup runs every phase (a wave past R works on ray R - 1 and stores
// nothing), so the barriers between the phases are uniform; S and Nf are the same for every ray.
// The searches return indices inside their arrays whatever the values are (NaN included), and the merged list is
// filled with near before the scatter: unsorted coarse samples give meaningless output, never an unwritten element.
template <int CAP, int RAYS>
__global__ __launch_bounds__(64 * RAYS) void ray_resample_kernel(const float* __restrict__ rays,
                                                                 const float* __restrict__ bounds, float near_,
                                                                 float far_, const float* __restrict__ ts_c,
                                                                 const float* __restrict__ w,
                                                                 const float* __restrict__ jitter, float eps,
                                                                 long long R, int S, int Nf,
                                                                 float* __restrict__ coords, float* __restrict__ ts,
                                                                 float* __restrict__ deltas) {
#pragma clang fp contract(off)
  __shared__ float s_tc[RAYS][CAP];
  __shared__ double s_tf[RAYS][CAP];
  __shared__ double s_cm[RAYS][2 * CAP + 2];
  const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
  long long r = (long long)blockIdx.x * RAYS + wave;
  const bool active = r < R;
  if (!active) r = R - 1;
  float* tc = s_tc[wave];
  double* tf = s_tf[wave];
  double* cm = s_cm[wave];
  const int M = S + Nf;
  const float* ray = rays + r * 6;
  const double ox = (double)ray[0], oy = (double)ray[1], oz = (double)ray[2];
  const double dx = (double)ray[3], dy = (double)ray[4], dz = (double)ray[5];
  const double nr = (double)(bounds ? bounds[2 * r] : near_), fr = (double)(bounds ? bounds[2 * r + 1] : far_);
  const bool hit = fr > nr;

  // the coarse samples and the unnormalised CDF: c_0 = 0, c_{s+1} = c_s + p_s
  const long long row0 = r * S;
  double carry = 0.0;
  if (lane == 0) cm[0] = 0.0;
  for (int base = 0; base < S; base += 64) {
    const int s = base + lane;
    double p = 0.0;
    if (s < S) {
      tc[s] = ts_c[row0 + s];
      double wv = (double)w[row0 + s];
      if (!(wv > 0.0)) wv = 0.0;                            // NaN and negative values count as 0
      if (wv > (double)FLT_MAX) wv = (double)FLT_MAX;       // +inf as FLT_MAX
      p = wv + (double)eps;
    }
    const double incl = wave_prefix_incl(p, lane);
    if (s < S) cm[s + 1] = carry + incl;
    carry += __shfl(incl, 63);
  }
  __syncthreads();

  // the draws: u_k = ((k + v_k) / Nf) tot, its bin s = the largest index with c_s <= u_k, the position inside the bin
  const double tot = cm[S];
  for (int base = 0; base < Nf; base += 64) {
    const int k = base + lane;
    if (k < Nf) {
      const double v = jitter ? (double)jitter[r * Nf + k] : 0.5;
      const double u = (((double)k + v) / (double)Nf) * tot;
      int lo = 0, hi = S;                                   // c_lo <= u (or lo = 0), c_hi > u (or hi = S)
      while (hi - lo > 1) {
        const int mid = (lo + hi) >> 1;
        if (cm[mid] <= u) lo = mid; else hi = mid;
      }
      const double c0 = cm[lo], den = cm[lo + 1] - c0;
      double f = den > 0.0 ? (u - c0) / den : 0.0;          // (eps can vanish beside a weight of 1e30: an empty bin)
      if (!(f > 0.0)) f = 0.0;
      if (f > 1.0) f = 1.0;
      const double e0 = lo > 0 ? ((double)tc[lo - 1] + (double)tc[lo]) / 2.0 : nr;
      const double e1 = lo + 1 < S ? ((double)tc[lo] + (double)tc[lo + 1]) / 2.0 : fr;
      double t = e0 + f * (e1 - e0);
      if (t > e1) t = e1;                                   // f = 1 may round past the edge: keep the draws sorted
      tf[k] = hit ? t : nr;
    }
  }
  __syncthreads();                                          // the CDF is dead: cm becomes the merged list
  for (int j = lane; j <= M; j += 64) cm[j] = j < M ? nr : (hit ? fr : nr);
  __syncthreads();

  // merge by rank, coarse first on a tie: pos(coarse i) = i + #{fine < tc_i}, pos(fine k) = k + #{coarse <= tf_k}
  for (int i = lane; i < S; i += 64) {
    const double cv = hit ? (double)tc[i] : nr;
    int lo = 0, hi = Nf;                                    // the first fine sample that is not < cv
    while (lo < hi) {
      const int mid = (lo + hi) >> 1;
      if (tf[mid] < cv) lo = mid + 1; else hi = mid;
    }
    cm[i + lo] = cv;
  }
  for (int k = lane; k < Nf; k += 64) {
    const double tv = tf[k];
    int lo = 0, hi = S;                                     // the first coarse sample that is not <= tv
    while (lo < hi) {
      const int mid = (lo + hi) >> 1;
      if ((hit ? (double)tc[mid] : nr) <= tv) lo = mid + 1; else hi = mid;
    }
    cm[k + lo] = tv;
  }
  __syncthreads();

  // the sampler's recipe on the merged list
  if (!active) return;
  const double norm = sqrt(dx * dx + dy * dy + dz * dz);
  for (int j = lane; j < M; j += 64) {
    const double t = cm[j];
    const double dl = hit ? (cm[j + 1] - t) * norm : 0.0;
    const long long e = r * M + j;
    coords[3 * e + 0] = (float)(ox + t * dx);
    coords[3 * e + 1] = (float)(oy + t * dy);
    coords[3 * e + 2] = (float)(oz + t * dz);
    ts[e] = (float)t;
    deltas[e] = (float)dl;
  }
}

template <int O>
__global__ __launch_bounds__(256) void composite_bwd_kernel(const float* __restrict__ y, const float* __restrict__ ts,
                                                            const float* __restrict__ deltas,
                                                            const float* __restrict__ bg,
                                                            const float* __restrict__ g_rgb,
                                                            const float* __restrict__ g_acc,
                                                            const float* __restrict__ g_depth, long long R, int S,
                                                            int mode, float* __restrict__ g_y) {
  const int lane = threadIdx.x & 63;
  const long long r = (long long)blockIdx.x * RENDER_RAYS_PER_WG + (threadIdx.x >> 6);
  if (r >= R) return;
  RayOut<O> F;
  ray_forward<O>(y, ts, deltas, r, S, mode, lane, F);
  float g[O - 1];
#pragma unroll
  for (int k = 0; k < O - 1; ++k) g[k] = g_rgb[r * (O - 1) + k];
  ray_backward<O>(y, ts, deltas, bg, r, S, mode, lane, F, g, g_acc ? g_acc[r] : 0.f, g_depth ? g_depth[r] : 0.f, g_y);
}

template <int O>
__global__ __launch_bounds__(256) void composite_mse_grad_kernel(const float* __restrict__ y,
                                                                 const float* __restrict__ ts,
                                                                 const float* __restrict__ deltas,
                                                                 const float* __restrict__ bg,
                                                                 const float* __restrict__ target, long long R, int S,
                                                                 int mode, float gscale, float* __restrict__ g_y,
                                                                 float* __restrict__ rgb,
                                                                 float* __restrict__ partial) {
#pragma clang fp contract(off)
  __shared__ float red[RENDER_RAYS_PER_WG];
  const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
  float loss = 0.f;
  for (long long r = (long long)blockIdx.x * RENDER_RAYS_PER_WG + wave; r < R;
       r += (long long)gridDim.x * RENDER_RAYS_PER_WG) {
    RayOut<O> F;
    ray_forward<O>(y, ts, deltas, r, S, mode, lane, F);
    float c[O - 1], g[O - 1];
    ray_rgb<O>(F, bg, c);
#pragma unroll
    for (int k = 0; k < O - 1; ++k) {
      const float d = c[k] - target[r * (O - 1) + k];
      loss += d * d;
      g[k] = gscale * d;
    }
    if (rgb && lane < O - 1) {
      float v = c[0];
#pragma unroll
      for (int k = 1; k < O - 1; ++k) v = lane == k ? c[k] : v;
      rgb[r * (O - 1) + lane] = v;
    }
    ray_backward<O>(y, ts, deltas, bg, r, S, mode, lane, F, g, 0.f, 0.f, g_y);
  }
  if (lane == 0) red[wave] = loss;
  __syncthreads();
  if (threadIdx.x == 0) partial[blockIdx.x] = (red[0] + red[1]) + (red[2] + red[3]);
}

// ---------------------------------------------------------------------------
// geometry and argument checks
// ---------------------------------------------------------------------------
struct RenderGeom {
  long long rows, blocks, sample_blocks;
};
static bool render_geom(int64_t R, int S, int O, RenderGeom& g) {
  if (R < 1 || S < 1 || O < 2 || O > 8) return false;
  long long rows, floats, bytes;
  if (__builtin_mul_overflow((long long)R, (long long)S, &rows) || __builtin_mul_overflow(rows, 8ll, &floats) ||
      __builtin_mul_overflow(floats, 4ll, &bytes))
    return false;                                                       // [R S][O <= 8] floats
  g.rows = rows;
  g.blocks = (R - 1) / RENDER_RAYS_PER_WG + 1;
  g.sample_blocks = (rows - 1) / 256 + 1;
  return g.blocks <= RENDER_MAX_BLOCKS && g.sample_blocks <= RENDER_MAX_BLOCKS;
}
static bool render_al4(const void* p) { return ((uintptr_t)p & 3) == 0; }
static bool render_al16(const void* p) { return ((uintptr_t)p & 15) == 0; }

#define RENDER_DISPATCH(O, LAUNCH)            \
  switch (O) {                                \
    case 2: LAUNCH(2); break;                 \
    case 3: LAUNCH(3); break;                 \
    case 4: LAUNCH(4); break;                 \
    case 5: LAUNCH(5); break;                 \
    case 6: LAUNCH(6); break;                 \
    case 7: LAUNCH(7); break;                 \
    default: LAUNCH(8); break;                \
  }

// ---------------------------------------------------------------------------
// entry points of the C ABI
// ---------------------------------------------------------------------------
extern "C" int wire_ray_samples(void* stream, const float* rays, const float* bounds, float near_, float far_,
                                const float* jitter, int64_t R, int S, float* coords, float* ts, float* deltas) {
  RenderGeom g;
  if (!render_geom(R, S, 4, g) || !rays || !coords || !ts || !deltas || !render_al4(rays) || !render_al4(bounds) ||
      !render_al4(jitter) || !render_al4(coords) || !render_al4(ts) || !render_al4(deltas) ||
      (!bounds && !(std::isfinite(near_) && std::isfinite(far_))))
    return fail(WIRE_ERR_ARG, "bad argument to wire_ray_samples");
  ProfScope ps((hipStream_t)stream, 3, 0);
  hipLaunchKernelGGL(ray_samples_kernel, dim3((unsigned)g.sample_blocks), dim3(256), 0, (hipStream_t)stream, rays,
                     bounds, near_, far_, jitter, (long long)R, S, coords, ts, deltas);
  HIPCHK(hipGetLastError());
  return WIRE_OK;
}

extern "C" int wire_composite_fwd(void* stream, const float* y, const float* ts, const float* deltas, const float* bg,
                                  int64_t R, int S, int O, int density, float* rgb, float* acc, float* depth) {
  RenderGeom g;
  if (!render_geom(R, S, O, g) || (density != 0 && density != 1) || !y || !ts || !deltas || !rgb || !render_al16(y) ||
      !render_al4(ts) || !render_al4(deltas) || !render_al4(bg) || !render_al4(rgb) || !render_al4(acc) ||
      !render_al4(depth))
    return fail(WIRE_ERR_ARG, "bad argument to wire_composite_fwd");
  ProfScope ps((hipStream_t)stream, 3, 0);
#define LAUNCH(OO)                                                                                                   \
  hipLaunchKernelGGL((composite_fwd_kernel<OO>), dim3((unsigned)g.blocks), dim3(256), 0, (hipStream_t)stream, y, ts, \
                     deltas, bg, (long long)R, S, density, rgb, acc, depth)
  RENDER_DISPATCH(O, LAUNCH)
#undef LAUNCH
  HIPCHK(hipGetLastError());
  return WIRE_OK;
}

extern "C" int wire_composite_bwd(void* stream, const float* y, const float* ts, const float* deltas, const float* bg,
                                  const float* g_rgb, const float* g_acc, const float* g_depth, int64_t R, int S, int O,
                                  int density, float* g_y) {
  RenderGeom g;
  if (!render_geom(R, S, O, g) || (density != 0 && density != 1) || !y || !ts || !deltas || !g_rgb || !g_y ||
      !render_al16(y) || !render_al16(g_y) || !render_al4(ts) || !render_al4(deltas) || !render_al4(bg) ||
      !render_al4(g_rgb) || !render_al4(g_acc) || !render_al4(g_depth))
    return fail(WIRE_ERR_ARG, "bad argument to wire_composite_bwd");
  ProfScope ps((hipStream_t)stream, 3, 0);
#define LAUNCH(OO)                                                                                                   \
  hipLaunchKernelGGL((composite_bwd_kernel<OO>), dim3((unsigned)g.blocks), dim3(256), 0, (hipStream_t)stream, y, ts, \
                     deltas, bg, g_rgb, g_acc, g_depth, (long long)R, S, density, g_y)
  RENDER_DISPATCH(O, LAUNCH)
#undef LAUNCH
  HIPCHK(hipGetLastError());
  return WIRE_OK;
}

extern "C" int wire_composite_mse_grad(void* stream, const float* y, const float* ts, const float* deltas,
                                       const float* bg, const float* target, int64_t R, int S, int O, int density,
                                       float shard, float* g_y, float* loss_out, float* rgb, float* partial) {
  RenderGeom g;
  if (!render_geom(R, S, O, g) || (density != 0 && density != 1) || !std::isfinite(shard) || !y || !ts || !deltas ||
      !target || !g_y || !loss_out || !partial || !render_al16(y) || !render_al16(g_y) || !render_al4(ts) ||
      !render_al4(deltas) || !render_al4(bg) || !render_al4(target) || !render_al4(loss_out) || !render_al4(rgb) ||
      !render_al4(partial))
    return fail(WIRE_ERR_ARG, "bad argument to wire_composite_mse_grad");
  const unsigned nb = (unsigned)(g.blocks < RENDER_LOSS_BLOCKS ? g.blocks : RENDER_LOSS_BLOCKS);
  const float scale = shard * (float)(1.0 / ((double)R * (double)(O - 1)));
  ProfScope ps((hipStream_t)stream, 3, 0);
#define LAUNCH(OO)                                                                                                  \
  hipLaunchKernelGGL((composite_mse_grad_kernel<OO>), dim3(nb), dim3(256), 0, (hipStream_t)stream, y, ts, deltas, bg, \
                     target, (long long)R, S, density, 2.f * scale, g_y, rgb, partial)
  RENDER_DISPATCH(O, LAUNCH)
#undef LAUNCH
  HIPCHK(launch_mse_final((hipStream_t)stream, partial, (int)nb, scale, loss_out));
  return WIRE_OK;
}

extern "C" int wire_composite_weights(void* stream, const float* y, const float* deltas, int64_t R, int S, int O,
                                      int density, float* w) {
  RenderGeom g;
  if (!render_geom(R, S, O, g) || (density != 0 && density != 1) || !y || !deltas || !w || !render_al16(y) ||
      !render_al4(deltas) || !render_al4(w))
    return fail(WIRE_ERR_ARG, "bad argument to wire_composite_weights");
  ProfScope ps((hipStream_t)stream, 3, 0);
  hipLaunchKernelGGL(composite_weights_kernel, dim3((unsigned)g.blocks), dim3(256), 0, (hipStream_t)stream, y, deltas,
                     (long long)R, S, O, density, w);
  HIPCHK(hipGetLastError());
  return WIRE_OK;
}

extern "C" int wire_ray_resample(void* stream, const float* rays, const float* bounds, float near_, float far_,
                                 const float* ts_c, const float* w, const float* jitter, float eps, int64_t R, int S,
                                 int Nf, float* coords, float* ts, float* deltas) {
  RenderGeom g;
  if (S < 1 || Nf < 1 || S > RESAMPLE_MAX || Nf > RESAMPLE_MAX || !render_geom(R, S + Nf, 4, g) || !rays || !ts_c ||
      !w || !coords || !ts || !deltas || !render_al4(rays) || !render_al4(bounds) || !render_al4(ts_c) ||
      !render_al4(w) || !render_al4(jitter) || !render_al4(coords) || !render_al4(ts) || !render_al4(deltas) ||
      (!bounds && !(std::isfinite(near_) && std::isfinite(far_))) || !(std::isfinite(eps) && eps > 0.f))
    return fail(WIRE_ERR_ARG, "bad argument to wire_ray_resample");
  const bool small = S <= RESAMPLE_SMALL && Nf <= RESAMPLE_SMALL;
  const long long blocks = (R - 1) / (small ? 4 : 2) + 1;
  if (blocks > RENDER_MAX_BLOCKS) return fail(WIRE_ERR_ARG, "bad argument to wire_ray_resample");
  ProfScope ps((hipStream_t)stream, 3, 0);
  if (small)
    hipLaunchKernelGGL((ray_resample_kernel<RESAMPLE_SMALL, 4>), dim3((unsigned)blocks), dim3(256), 0,
                       (hipStream_t)stream, rays, bounds, near_, far_, ts_c, w, jitter, eps, (long long)R, S, Nf, coords,
                       ts, deltas);
  else
    hipLaunchKernelGGL((ray_resample_kernel<RESAMPLE_MAX, 2>), dim3((unsigned)blocks), dim3(128), 0,
                       (hipStream_t)stream, rays, bounds, near_, far_, ts_c, w, jitter, eps, (long long)R, S, Nf, coords,
                       ts, deltas);
  HIPCHK(hipGetLastError());
  return WIRE_OK;
}
