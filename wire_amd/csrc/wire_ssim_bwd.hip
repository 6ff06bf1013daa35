// wire_ssim_bwd.hip -- the gradient of the mean structural similarity (wire_ssim.hip) with respect to its second image,
// and the loss of the SSIM-regularised training step, mse + lambda (1 - ssim), fused with its backward.  Fixed
// summation order, no atomics: the same call gives the same bits.
//
// FORMULA: x = gt, y = rec, both [H][W][O]; for a pixel p of the valid region [Ho][Wo] = [H-taps+1][W-taps+1], with the
// windowed moments mx, my, vx, vy, vxy of wire_ssim.hip,
//   n1 = 2 mx my + c1,  n2 = 2 vxy + c2,  d1 = mx^2 + my^2 + c1,  d2 = vx + vy + c2,  S = n1 n2 / (d1 d2)
//   P = dS/dmy  = 2 mx n2 / (d1 d2) - 2 my S / d1  = 2 n2 (mx - my) (mx (mx + my) + c1) / (d1^2 d2)
//   B = cov dS/dvy  = -cov S / d2
//   C = cov dS/dvxy = 2 cov n1 / (d1 d2)
// (the last form of P has no difference of two nearly equal products: mx d1 - my n1 factors).  my = m(y), vy = cov (m(y^2) -
// my^2) and vxy = cov (m(xy) - mx my) depend on the input pixel q under tap w(p, q) of window p, so
//   Ho Wo O  dSSIM/dy[q] = sum_p w(p, q) ( P_p + 2 B_p (y[q] - my_p) + C_p (x[q] - mx_p) ).
// T, the sum over the windows that cover q, is a "full" correlation with the separable window; it is taken separably
// over three maps, which splits y[q] - my_p into y[q] T(B) - T(B my) -- two large numbers when the image has a mean,
// the cancellation the forward avoids.  So the workgroup subtracts a constant c (the mean of its two halos, per channel)
// from both images, x' = x - c and y' = y - c, and forms the moments m0 = m(x'), m1 = m(y') of the shifted images as
// the forward does (mx = m0 + c Wsum, and the variances restored with the terms in 1 - Wsum of wire_ssim.hip's header).
// With Wsum = Ws^2 the sum of the fp32 window over both passes,
//   y[q] - my_p = y'[q] - m1_p + c (1 - Wsum),     x[q] - mx_p = x'[q] - m0_p + c (1 - Wsum),     mx - my = m0 - m1
// exactly, whatever c is, and
//   Ho Wo O  dSSIM/dy[q] = T(A)[q] + 2 y'[q] T(B)[q] + x'[q] T(C)[q],
//   A = P - 2 B (m1 - c (1 - Wsum)) - C (m0 - c (1 - Wsum)).
//
// TILING: recompute, not a workspace.  One workgroup of 256 threads owns SSIMB_TR x SSIMB_TC = 16 x 32 INPUT pixels and
// gathers: it needs A, B, C at the (16 + taps - 1) x (32 + taps - 1) windows that cover its pixels, and recomputes them
// from a halo of 2 (taps - 1): (16 + 2 taps - 2) x (32 + 2 taps - 2) pixels of both images.  The other choice -- a first
// pass, the forward tile kernel plus three stores, and a gather from the workspace -- has every forward tile subtract its
// own constant, and the windows that cover one input tile lie in up to four forward tiles: the maps would have to be
// stored unshifted (the cancellation above) or gathered in four parts.  Recomputing costs (26 x 42) / (16 x 32) = 2.1
// times the forward's moment arithmetic at 11 taps and saves three maps written and read; one constant per workgroup
// keeps the shifted form exact.  The channels are processed one after the other, so the LDS does not grow with O:
//   both halos of one channel             2 x (16 + 2 taps - 2) x (32 + 2 taps - 2) floats
//   the horizontal pass, five moments     5 x (16 + 2 taps - 2) x (32 + taps - 1)
//   A, B, C                               3 x (16 + taps - 1) x (32 + taps - 1)
//   (the horizontal pass of A, B, C, 3 x (16 + taps - 1) x 32, reuses the moments' planes)
// -- at 11 taps 3744 + 7560 + 3276 = 14 580 floats = 58 320 B for every O, under the 64 KB that need no opt-in, two
// workgroups to a CU.  Slot (s, u) of a plane is pixel (i0 - taps + 1 + s, j0 - taps + 1 + u) whatever the image's
// edges cut off: A, B, C of a window outside the valid region are stored as zeros, so the gather has no conditions.
// Every global load and store is a plain vector access of one float; a channel's loads step by O floats.
//
// The sums of the fused loss (the index over the windows a workgroup OWNS, those whose first pixel lies in its tile,
// and the squared residuals of its selected pixels) go to per-tile partials and are added in a fixed order.
#include "wire_dev.h"
#include "wire_point.h"

#define SSIMB_TR 16
#define SSIMB_TC 32
#define SSIMB_ROWS_BLOCKS 1024       // blocks of the launch that adds the MSE term of an index list

static inline int ssimb_tiles_x(int W) { return (int)cdiv(W, SSIMB_TC); }
int64_t ssim_bwd_tiles(int H, int W) { return (int64_t)cdiv(H, SSIMB_TR) * ssimb_tiles_x(W); }
// floats of the fused loss's scratch: the tiles' index sums, then the squared residuals' (tiles or row blocks)
int64_t ssim_loss_partials(int H, int W) {
  const int64_t nt = ssim_bwd_tiles(H, W);
  return nt + (nt > SSIMB_ROWS_BLOCKS ? nt : SSIMB_ROWS_BLOCKS);
}

struct SsimLossArgs {
  long long first, n_mse;     // the rows of the MSE term inside this pass: [first, first + n_mse)
  float gscale;               // 2 / (n_mse O)
  int do_ssim;                // 0: the MSE term alone (lambda == 0), nothing of the index is evaluated
};

// g_y[q] = scale dSSIM/dy[q] (+ the MSE term of a selected row), scale = (up ? up[0] : 1) * gmul.
// partial (optional): partial[tile] = the sum of S over the windows the tile owns, partial[ntiles + tile] = its sum of
// squared residuals.
template <int TAPS>
__global__ __launch_bounds__(256) void ssim_grad_kernel(const float* __restrict__ x, const float* __restrict__ y, int H,
                                                        int W, int O, SsimWin win, float wsum, float wdef, float cov,
                                                        float c1, float c2, int tiles_x, const float* __restrict__ up,
                                                        float gmul, SsimLossArgs la, float* __restrict__ g_y,
                                                        float* __restrict__ rec, float* __restrict__ partial,
                                                        int ntiles) {
  extern __shared__ __attribute__((aligned(16))) float ssimb_sm[];
  __shared__ float red[4];
  constexpr int HR = SSIMB_TR + 2 * TAPS - 2, HC = SSIMB_TC + 2 * TAPS - 2;     // a halo plane
  constexpr int CR = SSIMB_TR + TAPS - 1, CC = SSIMB_TC + TAPS - 1;             // a plane of A, B or C
  float* sx = ssimb_sm;                    // [HR][HC]
  float* sy = sx + HR * HC;
  float* hb = sy + HR * HC;                // [5][HR][CC]: the horizontal pass of the moments
  float* cf = hb + 5 * HR * CC;            // [3][CR][CC]: A, B, C
  float* gb = hb;                          // [3][CR][SSIMB_TC]: the horizontal pass of A, B, C (the moments are spent)
  const int tid = threadIdx.x;
  const int ti = blockIdx.x / tiles_x, tj = blockIdx.x - ti * tiles_x;
  const int i0 = ti * SSIMB_TR, j0 = tj * SSIMB_TC;
  const int tr = H - i0 < SSIMB_TR ? H - i0 : SSIMB_TR;          // input rows / columns of this tile: >= 1
  const int tc = W - j0 < SSIMB_TC ? W - j0 : SSIMB_TC;
  const float scale = (up ? up[0] : 1.f) * gmul;
  float ssum = 0.f, sq = 0.f;

  if (!la.do_ssim) {
    // the MSE term alone: the tile's tr rows of tc * O consecutive floats
    const int rw = tc * O;
    for (int k = tid; k < tr * rw; k += 256) {
      const int i = k / rw, f = k - i * rw;
      const size_t pix = (size_t)(i0 + i) * W + j0 + f / O;
      const size_t e = ((size_t)(i0 + i) * W + j0) * O + f;
      float out = 0.f;
      if ((long long)pix >= la.first && (long long)pix < la.first + la.n_mse) {
        const float v = y[e], d = v - x[e];
        out = __builtin_fmaf(la.gscale, d, out);
        if (rec) rec[e] = v;
        sq = __builtin_fmaf(d, d, sq);
      }
      g_y[e] = out;
    }
  } else {
    const int Ho = H - TAPS + 1, Wo = W - TAPS + 1;
    const int r0 = i0 - (TAPS - 1), q0 = j0 - (TAPS - 1);        // the pixel of slot (0, 0)
    // the windows that cover the tile AND lie in the valid region: slots [s0, s1) x [u0, u1), never empty
    // (s1 - s0 >= 1 because H >= TAPS); their pixels: slots [s0, s1 + TAPS - 1) x [u0, u1 + TAPS - 1), rows
    // r0 + s0 >= 0 .. r0 + s1 + TAPS - 2 <= H - 1 of the image
    const int s0 = r0 < 0 ? -r0 : 0, s1 = tr + TAPS - 1 < Ho - r0 ? tr + TAPS - 1 : Ho - r0;
    const int u0 = q0 < 0 ? -q0 : 0, u1 = tc + TAPS - 1 < Wo - q0 ? tc + TAPS - 1 : Wo - q0;
    const int a1 = s1 + TAPS - 1, b1 = u1 + TAPS - 1;
    for (int ch = 0; ch < O; ++ch) {
      // ---- stage both halos of this channel; their mean is the shift
      float s = 0.f;
      for (int k = tid; k < HR * HC; k += 256) {
        const int a = k / HC, b = k - a * HC;
        if (a >= s0 && a < a1 && b >= u0 && b < b1) {
          const size_t e = ((size_t)(r0 + a) * W + (q0 + b)) * O + ch;
          const float xv = x[e], yv = y[e];
          sx[k] = xv;
          sy[k] = yv;
          s += xv + yv;
        }
      }
      const float c = wire_block_sum(s, red) / (2.f * (float)((a1 - s0) * (b1 - u0)));     // (the barriers publish sx, sy)
      const float cw = c * wsum, ccw = c * cw, cd = c * wdef;
      // ---- horizontal pass: the five moments of the shifted images, rows [s0, a1) x columns [u0, u1)
      for (int k = tid; k < HR * CC; k += 256) {
        const int a = k / CC, u = k - a * CC;
        if (a >= s0 && a < a1 && u >= u0 && u < u1) {
          const float* px = sx + a * HC + u;
          const float* py = sy + a * HC + u;
          float a0 = 0.f, a1m = 0.f, a2 = 0.f, a3 = 0.f, a4 = 0.f;
#pragma unroll
          for (int t = 0; t < TAPS; ++t) {
            const float w = win.w[t];
            const float uu = px[t] - c, vv = py[t] - c;
            const float wu = w * uu, wq = w * vv;
            a0 += wu;
            a1m += wq;
            a2 = __builtin_fmaf(wu, uu, a2);
            a3 = __builtin_fmaf(wq, vv, a3);
            a4 = __builtin_fmaf(wu, vv, a4);
          }
          float* h = hb + k;
          h[0] = a0; h[HR * CC] = a1m; h[2 * HR * CC] = a2; h[3 * HR * CC] = a3; h[4 * HR * CC] = a4;
        }
      }
      __syncthreads();
      // ---- vertical pass, the index and A, B, C of every slot the gather reads: [0, tr + TAPS - 1) x [0, tc + TAPS - 1)
      for (int k = tid; k < CR * CC; k += 256) {
        const int sr = k / CC, u = k - sr * CC;
        if (sr >= tr + TAPS - 1 || u >= tc + TAPS - 1) continue;
        float A = 0.f, B = 0.f, Cc = 0.f;
        if (sr >= s0 && sr < s1 && u >= u0 && u < u1) {
          const float* h = hb + sr * CC + u;
          float m0 = 0.f, m1 = 0.f, m2 = 0.f, m3 = 0.f, m4 = 0.f;
#pragma unroll
          for (int t = 0; t < TAPS; ++t) {
            const float w = win.w[t];
            m0 = __builtin_fmaf(w, h[t * CC], m0);
            m1 = __builtin_fmaf(w, h[(HR + t) * CC], m1);
            m2 = __builtin_fmaf(w, h[(2 * HR + t) * CC], m2);
            m3 = __builtin_fmaf(w, h[(3 * HR + t) * CC], m3);
            m4 = __builtin_fmaf(w, h[(4 * HR + t) * CC], m4);
          }
          const float mx = m0 + cw, my = m1 + cw;
          const float vx = cov * (__builtin_fmaf(-m0, m0, m2) + wdef * __builtin_fmaf(2.f * c, m0, ccw));
          const float vy = cov * (__builtin_fmaf(-m1, m1, m3) + wdef * __builtin_fmaf(2.f * c, m1, ccw));
          const float vxy = cov * (__builtin_fmaf(-m0, m1, m4) + wdef * __builtin_fmaf(c, m0 + m1, ccw));
          const float n1 = __builtin_fmaf(2.f * mx, my, c1), n2 = __builtin_fmaf(2.f, vxy, c2);
          const float d1 = __builtin_fmaf(mx, mx, my * my) + c1, d2 = (vx + vy) + c2;
          const float S = (n1 * n2) / (d1 * d2);
          const float P = 2.f * n2 * (m0 - m1) * __builtin_fmaf(mx, mx + my, c1) / (d1 * d1 * d2);
          B = -cov * S / d2;
          Cc = 2.f * cov * n1 / (d1 * d2);
          A = P - 2.f * B * (m1 - cd) - Cc * (m0 - cd);
          if (sr >= TAPS - 1 && u >= TAPS - 1) ssum += S;        // the window's first pixel lies in this tile
        }
        cf[k] = A; cf[CR * CC + k] = B; cf[2 * CR * CC + k] = Cc;
      }
      __syncthreads();
      // ---- the transpose's horizontal pass: input column j collects the windows that begin at j - t
      for (int k = tid; k < CR * SSIMB_TC; k += 256) {
        const int sr = k >> 5, j = k & 31;
        if (sr >= tr + TAPS - 1 || j >= tc) continue;
        const float* p = cf + sr * CC + j + TAPS - 1;
        float g0 = 0.f, g1 = 0.f, g2 = 0.f;
#pragma unroll
        for (int t = 0; t < TAPS; ++t) {
          const float w = win.w[t];
          g0 = __builtin_fmaf(w, p[-t], g0);
          g1 = __builtin_fmaf(w, p[CR * CC - t], g1);
          g2 = __builtin_fmaf(w, p[2 * CR * CC - t], g2);
        }
        gb[k] = g0; gb[CR * SSIMB_TC + k] = g1; gb[2 * CR * SSIMB_TC + k] = g2;
      }
      __syncthreads();
      // ---- its vertical pass and the gradient of the tile's own pixels
      for (int k = tid; k < SSIMB_TR * SSIMB_TC; k += 256) {
        const int i = k >> 5, j = k & 31;
        if (i >= tr || j >= tc) continue;
        const float* p = gb + (i + TAPS - 1) * SSIMB_TC + j;
        float g0 = 0.f, g1 = 0.f, g2 = 0.f;
#pragma unroll
        for (int t = 0; t < TAPS; ++t) {
          const float w = win.w[t];
          g0 = __builtin_fmaf(w, p[-t * SSIMB_TC], g0);
          g1 = __builtin_fmaf(w, p[CR * SSIMB_TC - t * SSIMB_TC], g1);
          g2 = __builtin_fmaf(w, p[2 * CR * SSIMB_TC - t * SSIMB_TC], g2);
        }
        const int hk = (i + TAPS - 1) * HC + j + TAPS - 1;
        const float xv = sx[hk], yv = sy[hk];
        float out = scale * __builtin_fmaf(xv - c, g2, __builtin_fmaf(2.f * (yv - c), g1, g0));
        const size_t pix = (size_t)(i0 + i) * W + j0 + j, e = pix * O + ch;
        if ((long long)pix >= la.first && (long long)pix < la.first + la.n_mse) {
          const float d = yv - xv;
          out = __builtin_fmaf(la.gscale, d, out);
          if (rec) rec[e] = yv;
          sq = __builtin_fmaf(d, d, sq);
        }
        g_y[e] = out;
      }
      __syncthreads();        // the next channel overwrites the halos and the moments' planes
    }
  }
  if (partial) {
    ssum = wire_block_sum(ssum, red);
    sq = wire_block_sum(sq, red);
    if (tid == 0) {
      partial[blockIdx.x] = ssum;
      partial[ntiles + blockIdx.x] = sq;
    }
  }
}

// The MSE term of the rows idx[0 .. n_mse) (distinct), added to the SSIM term that ssim_grad_kernel has stored: one
// thread per selected element reads and rewrites its own element of g_y.  sq_partial[b] = the block's sum of squared
// residuals.
__global__ __launch_bounds__(256) void ssim_mse_rows_kernel(const float* __restrict__ y, int O,
                                                            const float* __restrict__ target,
                                                            const int64_t* __restrict__ idx, long long n_mse,
                                                            float gscale, float* __restrict__ g_y,
                                                            float* __restrict__ rec, float* __restrict__ sq_partial) {
  __shared__ float red[4];
  const long long total = n_mse * O;
  float sq = 0.f;
  for (long long t = (long long)blockIdx.x * 256 + threadIdx.x; t < total; t += (long long)gridDim.x * 256) {
    const long long r = t / O;
    const long long e = (long long)idx[r] * O + (t - r * O);
    const float v = y[e];
    const float d = v - target[e];
    g_y[e] = __builtin_fmaf(gscale, d, g_y[e]);
    if (rec) rec[e] = v;
    sq = __builtin_fmaf(d, d, sq);
  }
  sq = wire_block_sum(sq, red);
  if (threadIdx.x == 0) sq_partial[blockIdx.x] = sq;
}

// out[0..2] = loss, mse, ssim: ssim = (sum of n_s partials) / count, mse = lscale * (sum of n_sq partials at
// partial + sq_off), loss = mse + lambda (1 - ssim), every product and sum rounded once; without the index
// (do_ssim == 0) ssim = 0 and loss = mse
__global__ __launch_bounds__(256) void ssim_loss_final_kernel(const float* __restrict__ partial, int n_s, int sq_off,
                                                              int n_sq, float count, float lscale, float lambda,
                                                              int do_ssim, float* __restrict__ out) {
  __shared__ float red[4];
  float a = 0.f, b = 0.f;
  for (int i = threadIdx.x; i < n_s; i += 256) a += partial[i];
  for (int i = threadIdx.x; i < n_sq; i += 256) b += partial[sq_off + i];
  a = wire_block_sum(a, red);
  b = wire_block_sum(b, red);
  if (threadIdx.x != 0) return;
  {
#pragma clang fp contract(off)
    const float mse = b * lscale;
    const float ssim = do_ssim ? a / count : 0.f;
    out[0] = do_ssim ? mse + lambda * (1.f - ssim) : mse;
    out[1] = mse;
    out[2] = ssim;
  }
}

template <int TAPS>
static hipError_t launch_ssim_grad_t(hipStream_t s, const float* x, const float* y, int H, int W, int O,
                                     const SsimWin& win, float wsum, float wdef, float cov, float c1, float c2,
                                     const float* up, float gmul, const SsimLossArgs& la, float* g_y, float* rec,
                                     float* partial) {
  constexpr int HR = SSIMB_TR + 2 * TAPS - 2, HC = SSIMB_TC + 2 * TAPS - 2;
  constexpr int CR = SSIMB_TR + TAPS - 1, CC = SSIMB_TC + TAPS - 1;
  constexpr int lds = (2 * HR * HC + 5 * HR * CC + 3 * CR * CC) * 4;
  static_assert(3 * CR * SSIMB_TC <= 5 * HR * CC, "the horizontal pass of A, B, C reuses the moments' planes");
  const int ntiles = (int)ssim_bwd_tiles(H, W);
  // > 64 KB of dynamic LDS needs the opt-in, per launch (as launch_ssim_t); 11 taps take 58 320 B
  if (lds > 65536) {
    const hipError_t attr = hipFuncSetAttribute(reinterpret_cast<const void*>(ssim_grad_kernel<TAPS>),
                                                hipFuncAttributeMaxDynamicSharedMemorySize, lds);
    if (attr != hipSuccess) return attr;
  }
  hipLaunchKernelGGL(ssim_grad_kernel<TAPS>, dim3((unsigned)ntiles), dim3(256), lds, s, x, y, H, W, O, win, wsum, wdef,
                     cov, c1, c2, ssimb_tiles_x(W), up, gmul, la, g_y, rec, partial, ntiles);
  return hipGetLastError();
}

static hipError_t launch_ssim_grad(hipStream_t s, const float* x, const float* y, int H, int W, int O, int taps,
                                   const SsimWin& win, float cov, float c1, float c2, const float* up, float gmul,
                                   const SsimLossArgs& la, float* g_y, float* rec, float* partial) {
  if (taps < 3 || taps > SSIM_MAX_TAPS || !(taps & 1) || O < 1 || O > WIRE_MAXO || H < taps || W < taps ||
      ssim_bwd_tiles(H, W) > 0x3fffffff)
    return hipErrorInvalidValue;
  double ws = 0.0;                                   // the window's own sum, per pass and for both (as launch_ssim)
  for (int t = 0; t < taps; ++t) ws += (double)win.w[t];
  const double w2 = ws * ws;
  const float wsum = (float)w2, wdef = (float)(1.0 - w2);
  switch (taps) {
    case 3: return launch_ssim_grad_t<3>(s, x, y, H, W, O, win, wsum, wdef, cov, c1, c2, up, gmul, la, g_y, rec, partial);
    case 5: return launch_ssim_grad_t<5>(s, x, y, H, W, O, win, wsum, wdef, cov, c1, c2, up, gmul, la, g_y, rec, partial);
    case 7: return launch_ssim_grad_t<7>(s, x, y, H, W, O, win, wsum, wdef, cov, c1, c2, up, gmul, la, g_y, rec, partial);
    case 9: return launch_ssim_grad_t<9>(s, x, y, H, W, O, win, wsum, wdef, cov, c1, c2, up, gmul, la, g_y, rec, partial);
    default: return launch_ssim_grad_t<11>(s, x, y, H, W, O, win, wsum, wdef, cov, c1, c2, up, gmul, la, g_y, rec, partial);
  }
}

hipError_t launch_ssim_bwd(hipStream_t s, const float* x, const float* y, int H, int W, int O, int taps,
                           const SsimWin& win, float cov, float c1, float c2, const float* g_ssim, float* g_y) {
  const double count = (double)(H - taps + 1) * (double)(W - taps + 1) * O;
  const SsimLossArgs la{0, 0, 0.f, 1};
  return launch_ssim_grad(s, x, y, H, W, O, taps, win, cov, c1, c2, g_ssim, (float)(1.0 / count), la, g_y, nullptr,
                          nullptr);
}

hipError_t launch_ssim_mse_grad(hipStream_t s, const float* y, int H, int W, int O, const float* target, int taps,
                                const SsimWin& win, float cov, float c1, float c2, const int64_t* idx, int64_t first,
                                int64_t n_mse, float lambda, float* g_y, float* loss_out, float* rec, float* partial) {
  const int64_t npix = (int64_t)H * W;
  if (n_mse < 0 || n_mse > npix) return hipErrorInvalidValue;
  const double count = (double)(H - taps + 1) * (double)(W - taps + 1) * O, nel = (double)n_mse * (double)O;
  const float gscale = n_mse ? (float)(2.0 / nel) : 0.f, lscale = n_mse ? (float)(1.0 / nel) : 0.f;
  const int do_ssim = lambda != 0.f;
  const int ntiles = (int)ssim_bwd_tiles(H, W);
  // a range is selected inside the one pass; rows given by idx get their MSE term in a second launch over those rows
  const SsimLossArgs la{idx ? 0ll : (long long)first, idx ? 0ll : (long long)n_mse, gscale, do_ssim};
  hipError_t e = launch_ssim_grad(s, target, y, H, W, O, taps, win, cov, c1, c2, nullptr, (float)(-(double)lambda / count),
                                  la, g_y, idx ? nullptr : rec, partial);
  if (e != hipSuccess) return e;
  int n_sq = ntiles;
  if (idx) {
    n_sq = n_mse ? (int)(n_mse * O < (int64_t)SSIMB_ROWS_BLOCKS * 256 ? cdiv(n_mse * O, 256) : SSIMB_ROWS_BLOCKS) : 0;
    if (n_mse)
      hipLaunchKernelGGL(ssim_mse_rows_kernel, dim3((unsigned)n_sq), dim3(256), 0, s, y, O, target, idx,
                         (long long)n_mse, gscale, g_y, rec, partial + ntiles);
  }
  hipLaunchKernelGGL(ssim_loss_final_kernel, dim3(1), dim3(256), 0, s, partial, ntiles, ntiles, n_sq, (float)count,
                     lscale, lambda, do_ssim, loss_out);
  return hipGetLastError();
}
