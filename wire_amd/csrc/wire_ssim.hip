// wire_ssim.hip -- the structural similarity index of two channel-last images [H][W][O] on the device: five windowed
// moments (x, y, x^2, y^2, xy) under a separable window over the valid region, the per-pixel rational expression of them,
// and the mean over pixels and channels.  Fixed summation order, no atomics: the same bits every run.
//
// TILE: one workgroup of 256 threads owns SSIM_TR x SSIM_TC = 16 x 32 output pixels, all O channels (the tests' shapes
// are chosen around these two numbers).  It keeps in LDS
//   the halo of both images, one plane per channel          2 x O x (16 + taps - 1) x (32 + taps - 1) floats
//   the horizontal pass of a group of <= SSIM_CG channels   min(O, 4) x 5 x (16 + taps - 1) x 32 floats
// -- at 11 taps and O = 3: 2 x 3 x 26 x 42 + 3 x 5 x 26 x 32 = 19 032 floats = 76 128 B, so two workgroups share a CU's
// 160 KiB; at O = 8 (two groups of 4 channels): 34 112 floats = 136 448 B, one workgroup per CU.  The global reads follow
// the interleaved rows (a wave per row, lanes on consecutive floats); the planes make every stride of the two passes a
// compile-time constant, so a tap is an immediate offset of its LDS read, and the 32 lanes of half a wave read 32
// consecutive dwords of one row (no bank conflicts).
//
// CANCELLATION: m(x^2) - m(x)^2 loses what the mean of the image carries, so the tile subtracts a constant c (the mean of
// its two halos) from both images before the moments are formed.  Variances and covariances do not change under a shift
// when the window sums to one; the fp32 window sums to Ws = 1 + d per pass, and the unshifted expression the libraries
// evaluate is restored exactly, with Wsum = Ws^2:
//   m(x)            = m(x') + c Wsum
//   m(x^2) - m(x)^2 = m(x'^2) - m(x')^2 + (1 - Wsum) (2 c m(x') + c^2 Wsum)
//   m(xy) - m(x)m(y) = m(x'y') - m(x')m(y') + (1 - Wsum) (c (m(x') + m(y')) + c^2 Wsum)
#include "wire_dev.h"
#include "wire_point.h"

#define SSIM_TR 16
#define SSIM_TC 32
#define SSIM_CG 4            // channels of one group of the two passes

static inline int ssim_tiles_y(int H, int taps) { return (int)cdiv(H - taps + 1, SSIM_TR); }
static inline int ssim_tiles_x(int W, int taps) { return (int)cdiv(W - taps + 1, SSIM_TC); }
int64_t ssim_tiles(int H, int W, int taps) { return (int64_t)ssim_tiles_y(H, taps) * ssim_tiles_x(W, taps); }

template <int TAPS>
__global__ __launch_bounds__(256) void ssim_tile_kernel(const float* __restrict__ x, const float* __restrict__ y, int H,
                                                        int W, int O, SsimWin win, float wsum, float wdef, float cov,
                                                        float c1, float c2, int tiles_x, float* __restrict__ map,
                                                        float* __restrict__ partial) {
  extern __shared__ __attribute__((aligned(16))) float ssim_sm[];
  __shared__ float red[4];
  constexpr int HR = SSIM_TR + TAPS - 1, HC = SSIM_TC + TAPS - 1;     // rows / columns of a halo plane
  constexpr int HP = 5 * HR * SSIM_TC;                                // a channel's five planes of the horizontal pass
  float* sx = ssim_sm;                                                // [O][HR][HC]
  float* sy = sx + O * HR * HC;
  float* hb = sy + O * HR * HC;                                       // [min(O, SSIM_CG)][5][HR][SSIM_TC]
  const int tid = threadIdx.x, lane = tid & 63, wv = tid >> 6;
  const int ti = blockIdx.x / tiles_x, tj = blockIdx.x - ti * tiles_x;
  const int i0 = ti * SSIM_TR, j0 = tj * SSIM_TC;
  const int Ho = H - TAPS + 1, Wo = W - TAPS + 1;
  const int tr = Ho - i0 < SSIM_TR ? Ho - i0 : SSIM_TR;          // output rows / columns of this tile (ragged at the far edges)
  const int tc = Wo - j0 < SSIM_TC ? Wo - j0 : SSIM_TC;
  const int hrv = tr + TAPS - 1, hwv = (tc + TAPS - 1) * O;      // its halo: rows i0 .. i0 + hrv - 1 <= H - 1, hwv floats of each

  // ---- stage both halos: a wave per row (rows wv, wv + 4, ..), 256 contiguous bytes per load; the loads of all of a
  // wave's rows are issued before the first store waits for one (2 NR of them in flight per lane).  Float k of a row is
  // column k / O, channel k % O: (k + 0.5) / O in fp32 is exact to the integer for k < 2^20
  constexpr int NR = (HR + 3) / 4;
  const size_t g0 = ((size_t)(i0 + wv) * W + j0) * O, gstep = (size_t)4 * W * O;
  const float inv_o = 1.f / (float)O;
  float s = 0.f;
  for (int k = lane; k < hwv; k += 64) {
    const int col = (int)(((float)k + 0.5f) * inv_o), ch = k - col * O;
    const int d0 = (ch * HR + wv) * HC + col;
    float a[NR], b[NR];
#pragma unroll
    for (int u = 0; u < NR; ++u)
      if (wv + 4 * u < hrv) {
        a[u] = x[g0 + u * gstep + k];
        b[u] = y[g0 + u * gstep + k];
      }
#pragma unroll
    for (int u = 0; u < NR; ++u)
      if (wv + 4 * u < hrv) {
        sx[d0 + 4 * u * HC] = a[u];
        sy[d0 + 4 * u * HC] = b[u];
        s += a[u] + b[u];
      }
  }
  s = wire_wave_sum(s);
  if (lane == 0) red[wv] = s;
  __syncthreads();
  const float c = ((red[0] + red[1]) + (red[2] + red[3])) / (2.f * (float)(hrv * hwv));
  const float cw = c * wsum, ccw = c * cw;

  // both passes: half a wave per row (rows 2 wv + half, + 8, ..), a lane per column
  const int j = lane & 31, row0 = 2 * wv + (lane >> 5);
  float acc = 0.f;
  for (int ch0 = 0; ch0 < O; ch0 += SSIM_CG) {
    const int cg = O - ch0 < SSIM_CG ? O - ch0 : SSIM_CG;
    // ---- horizontal pass: every halo row, the five moments of the shifted images
    if (j < tc)
      for (int cc = 0; cc < cg; ++cc)
        for (int r = row0; r < hrv; r += 8) {
          const float* px = sx + ((ch0 + cc) * HR + r) * HC + j;
          const float* py = sy + ((ch0 + cc) * HR + r) * HC + j;
          float a0 = 0.f, a1 = 0.f, a2 = 0.f, a3 = 0.f, a4 = 0.f;
#pragma unroll
          for (int t = 0; t < TAPS; ++t) {
            const float w = win.w[t];
            const float u = px[t] - c, v = py[t] - c;
            const float wu = w * u, wq = w * v;
            a0 += wu;
            a1 += wq;
            a2 = __builtin_fmaf(wu, u, a2);
            a3 = __builtin_fmaf(wq, v, a3);
            a4 = __builtin_fmaf(wu, v, a4);
          }
          float* h = hb + cc * HP + r * SSIM_TC + j;
          h[0] = a0; h[HR * SSIM_TC] = a1; h[2 * HR * SSIM_TC] = a2; h[3 * HR * SSIM_TC] = a3; h[4 * HR * SSIM_TC] = a4;
        }
    __syncthreads();
    // ---- vertical pass, the index itself, the map and this thread's share of the sum
    if (j < tc)
      for (int cc = 0; cc < cg; ++cc)
        for (int i = row0; i < tr; i += 8) {
          const float* h = hb + cc * HP + i * SSIM_TC + j;
          float m0 = 0.f, m1 = 0.f, m2 = 0.f, m3 = 0.f, m4 = 0.f;
#pragma unroll
          for (int t = 0; t < TAPS; ++t) {
            const float w = win.w[t];
            m0 = __builtin_fmaf(w, h[t * SSIM_TC], m0);
            m1 = __builtin_fmaf(w, h[(HR + t) * SSIM_TC], m1);
            m2 = __builtin_fmaf(w, h[(2 * HR + t) * SSIM_TC], m2);
            m3 = __builtin_fmaf(w, h[(3 * HR + t) * SSIM_TC], m3);
            m4 = __builtin_fmaf(w, h[(4 * HR + t) * SSIM_TC], m4);
          }
          const float mx = m0 + cw, my = m1 + cw;
          const float vx = cov * (__builtin_fmaf(-m0, m0, m2) + wdef * __builtin_fmaf(2.f * c, m0, ccw));
          const float vy = cov * (__builtin_fmaf(-m1, m1, m3) + wdef * __builtin_fmaf(2.f * c, m1, ccw));
          const float vxy = cov * (__builtin_fmaf(-m0, m1, m4) + wdef * __builtin_fmaf(c, m0 + m1, ccw));
          const float num = __builtin_fmaf(2.f * mx, my, c1) * __builtin_fmaf(2.f, vxy, c2);
          const float den = (__builtin_fmaf(mx, mx, my * my) + c1) * ((vx + vy) + c2);
          const float S = num / den;
          if (map) map[((size_t)(i0 + i) * Wo + j0 + j) * O + ch0 + cc] = S;
          acc += S;
        }
    __syncthreads();
  }
  acc = wire_wave_sum(acc);
  if (lane == 0) red[wv] = acc;        // (the last read of red lies before the barriers above)
  __syncthreads();
  if (tid == 0) partial[blockIdx.x] = (red[0] + red[1]) + (red[2] + red[3]);
}

// the tiles' sums in a fixed order: thread t takes tiles t, t + 256, ..; then the wave, then the four waves
__global__ __launch_bounds__(256) void ssim_final_kernel(const float* __restrict__ partial, int ntiles, float count,
                                                         float* __restrict__ out) {
  __shared__ float red[4];
  float a = 0.f;
  for (int i = threadIdx.x; i < ntiles; i += 256) a += partial[i];
  a = wire_block_sum(a, red);
  if (threadIdx.x == 0) out[0] = a / count;
}

template <int TAPS>
static hipError_t launch_ssim_t(hipStream_t s, const float* x, const float* y, int H, int W, int O, const SsimWin& win,
                                float wsum, float wdef, float cov, float c1, float c2, float* map, float* partial) {
  const int tiles_x = ssim_tiles_x(W, TAPS);
  const int ntiles = (int)ssim_tiles(H, W, TAPS);
  const int cg = O < SSIM_CG ? O : SSIM_CG;
  const int lds = (SSIM_TR + TAPS - 1) * (2 * (SSIM_TC + TAPS - 1) * O + 5 * SSIM_TC * cg) * 4;
  // > 64 KB of dynamic LDS needs the opt-in, per launch: the attribute belongs to the current device's copy of the function
  if (lds > 65536) {
    const hipError_t attr = hipFuncSetAttribute(reinterpret_cast<const void*>(ssim_tile_kernel<TAPS>),
                                                hipFuncAttributeMaxDynamicSharedMemorySize, lds);
    if (attr != hipSuccess) return attr;
  }
  hipLaunchKernelGGL(ssim_tile_kernel<TAPS>, dim3((unsigned)ntiles), dim3(256), lds, s, x, y, H, W, O, win, wsum, wdef, cov,
                     c1, c2, tiles_x, map, partial);
  return hipGetLastError();
}

hipError_t launch_ssim(hipStream_t s, const float* x, const float* y, int H, int W, int O, int taps, const SsimWin& win,
                       float cov, float c1, float c2, float* out1, float* map, float* partial) {
  if (taps < 3 || taps > SSIM_MAX_TAPS || !(taps & 1) || O < 1 || O > WIRE_MAXO || H < taps || W < taps ||
      ssim_tiles(H, W, taps) > 0x7fffffff)
    return hipErrorInvalidValue;
  double ws = 0.0;                                   // the window's own sum, per pass and for both
  for (int t = 0; t < taps; ++t) ws += (double)win.w[t];
  const double w2 = ws * ws;
  const float wsum = (float)w2, wdef = (float)(1.0 - w2);
  hipError_t e;
  switch (taps) {
    case 3: e = launch_ssim_t<3>(s, x, y, H, W, O, win, wsum, wdef, cov, c1, c2, map, partial); break;
    case 5: e = launch_ssim_t<5>(s, x, y, H, W, O, win, wsum, wdef, cov, c1, c2, map, partial); break;
    case 7: e = launch_ssim_t<7>(s, x, y, H, W, O, win, wsum, wdef, cov, c1, c2, map, partial); break;
    case 9: e = launch_ssim_t<9>(s, x, y, H, W, O, win, wsum, wdef, cov, c1, c2, map, partial); break;
    default: e = launch_ssim_t<11>(s, x, y, H, W, O, win, wsum, wdef, cov, c1, c2, map, partial); break;
  }
  if (e != hipSuccess) return e;
  const double count = (double)(H - taps + 1) * (double)(W - taps + 1) * O;
  hipLaunchKernelGGL(ssim_final_kernel, dim3(1), dim3(256), 0, s, partial, (int)ssim_tiles(H, W, taps), (float)count, out1);
  return hipGetLastError();
}
