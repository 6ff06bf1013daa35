// wire_radon.hip -- the volume form of the CT operator: the parallel-beam Radon transform of wire_radon_fwd
// (wire_train.hip; formula in include/wire_hip.h) applied to every slice of a volume stored CHANNEL-LAST,
//   vol [H][W][C] -> sino [A][W][C],      sino[a][j][c] = sum_i bilinear(vol[:, :, c], x(a, j, i), y(a, j, i)),
// the layout in which a 3-D grid's network output already lies (row (i W + j) T + k: the slice index innermost), and
// its adjoint as a GATHER.  The geometry of a sample (a, j, i) -- its position, its four taps and their weights -- does
// not depend on the channel, and the C values of a tap are C consecutive floats.
//
// ARITHMETIC: exactly radon_kernel<false>'s, as the compiler contracts it, written out with explicit fmas under
// contract(off) so that it does not depend on what the optimiser fuses here:
//   x = fma(cs, xj, -(sn yi)) + cx,  y = fma(sn, xj, cs yi) + cy,  v = +0, v = fma(wy wx, value, v) over the valid taps
//   in the order (y0, x0), (y0, x0 + 1), (y0 + 1, x0), (y0 + 1, x0 + 1), acc += v over the rows in ascending i.
// Channel c of the forward therefore has the bits of wire_radon_fwd on slice c (tests/test_gpu_radon_volume.py).
//
// FORWARD: one thread per (a, j, V consecutive channels), channels fastest, rows in the loop: the lanes that share a j
// read one contiguous run of C floats per tap.  V = 4 (16-byte loads, the geometry evaluated once per four channels)
// when C % 4 == 0 and both pointers are 16-byte aligned, else V = 1.  A workgroup belongs to one angle; thread 0
// evaluates its sine and cosine into LDS.
//
// ADJOINT: g_vol[y][x][c] = sum over the samples (a, j, i) that have pixel (x, y) among their taps of
// weight * g_sino[a][j][c].  Such a sample lies within 1 of the pixel along each axis after the rotation, so within
// sqrt(2) of the pixel's inverse-rotated position (j*, i*) in the (j, i) lattice, so within sqrt(2) + 1/2 < 2 of the
// lattice point nearest to it along each axis: the 5 x 5 window around that point holds every one of them, with a whole
// lattice step to spare for the rounding of (j*, i*).  Every candidate's (x, y) is evaluated exactly as the forward
// evaluates it and the forward's own floor decides whether the pixel is one of its taps and with which weight, so the
// tap set and the weights are the forward's, tap for tap.  A workgroup of four waves owns four consecutive pixels and a
// chunk of 64 channels.  Per chunk of 64 angles: phase A, thread (pixel, angle) walks its 25 candidates and lists the
// taps -- at most nine lattice points fit into the closed 2 x 2 square -- as (weight, a W + j) in LDS; phase B, wave =
// pixel, lane = channel, applies the lists in the order angle, window row, window column.  No atomics, every element
// written exactly once by one thread in a fixed order: the same call gives the same bits and needs no memset.
//
// The two entry points of the C ABI (include/wire_hip.h) are at the end of this file.
#include <climits>

#include "wire_dev.h"
#include "wire_plan.h"

#define RV_DEG2RAD 0.017453292519943295f
#define RV_TILE 4       // pixels per workgroup of the adjoint: one wave each
#define RV_ANGLES 64    // angles per pass of the adjoint: RV_TILE * RV_ANGLES = 256 threads list taps
#define RV_MAXT 10      // taps of one (pixel, angle): <= 9 lattice points in a closed 2 x 2 square

template <int V> struct rv_vec;
template <> struct rv_vec<1> { typedef float type; };
template <> struct rv_vec<4> { typedef f32x4 type; };

template <int V>
__global__ __launch_bounds__(256) void radon_vol_fwd_kernel(const float* __restrict__ vol,
                                                            const float* __restrict__ angles, int H, int W, int C,
                                                            unsigned chunks, float* __restrict__ sino) {
#pragma clang fp contract(off)
  typedef typename rv_vec<V>::type vec;
  __shared__ float sc[2];
  const unsigned a = blockIdx.x / chunks, chunk = blockIdx.x - a * chunks;
  if (threadIdx.x == 0) wire_sincos(angles[a] * RV_DEG2RAD, sc[0], sc[1]);
  __syncthreads();
  const int CV = C / V;
  const long long e = (long long)chunk * 256 + threadIdx.x;
  if (e >= (long long)W * CV) return;
  const int j = (int)(e / CV), c = (int)(e - (long long)j * CV) * V;
  const float sn = sc[0], cs = sc[1];
  const float cx = 0.5f * (float)(W - 1), cy = 0.5f * (float)(H - 1);
  const float xj = (float)j - cx;
  const float* base = vol + c;
  vec acc = (vec)0.f;
  for (int i = 0; i < H; ++i) {
    const float yi = (float)i - cy;
    const float x = __builtin_fmaf(cs, xj, -(sn * yi)) + cx;
    const float y = __builtin_fmaf(sn, xj, cs * yi) + cy;
    const float xf = floorf(x), yf = floorf(y);
    const int x0 = (int)xf, y0 = (int)yf;
    if (x0 < -1 || x0 >= W || y0 < -1 || y0 >= H) continue;
    const float wx1 = x - xf, wy1 = y - yf, wx0 = 1.f - wx1, wy0 = 1.f - wy1;
    const bool vx0 = x0 >= 0, vx1 = x0 + 1 < W, vy0 = y0 >= 0, vy1 = y0 + 1 < H;
    vec v = (vec)0.f;
#define RV_TAP(yy, xx, wgt)                                                                    \
  {                                                                                            \
    const vec t = *(const vec*)(base + ((long long)(yy) * W + (xx)) * C);                      \
    const float m = (wgt);                                                                     \
    if constexpr (V == 1) v = __builtin_fmaf(m, t, v);                                         \
    else { _Pragma("unroll") for (int q = 0; q < V; ++q) v[q] = __builtin_fmaf(m, t[q], v[q]); } \
  }
    if (vy0) {
      if (vx0) RV_TAP(y0, x0, wy0 * wx0)
      if (vx1) RV_TAP(y0, x0 + 1, wy0 * wx1)
    }
    if (vy1) {
      if (vx0) RV_TAP(y0 + 1, x0, wy1 * wx0)
      if (vx1) RV_TAP(y0 + 1, x0 + 1, wy1 * wx1)
    }
#undef RV_TAP
    acc = acc + v;
  }
  *(vec*)(sino + ((long long)a * W + j) * C + c) = acc;
}

struct rv_tap { float w; int off; };

__global__ __launch_bounds__(256) void radon_vol_bwd_kernel(const float* __restrict__ g_sino,
                                                            const float* __restrict__ angles, int H, int W, int C,
                                                            int A, float* __restrict__ g_vol) {
#pragma clang fp contract(off)
  __shared__ float s_sn[RV_ANGLES], s_cs[RV_ANGLES];
  __shared__ int s_cnt[RV_TILE][RV_ANGLES];
  __shared__ rv_tap s_tap[RV_TILE][RV_ANGLES][RV_MAXT];
  const int t = threadIdx.x, pl = t >> 6, lane = t & 63;
  const long long npix = (long long)H * W;
  // phase A: this thread's pixel is tile pixel pl, its angle lane; phase B: pixel pl again, channel c
  const long long p = (long long)blockIdx.x * RV_TILE + pl;
  const bool pix_ok = p < npix;
  const int py = pix_ok ? (int)(p / W) : 0, px = pix_ok ? (int)(p - (long long)py * W) : 0;
  const int c = (int)blockIdx.y * 64 + lane;
  const float cx = 0.5f * (float)(W - 1), cy = 0.5f * (float)(H - 1);
  const float fx = (float)px - cx, fy = (float)py - cy;
  float acc = 0.f;
  for (int a0 = 0; a0 < A; a0 += RV_ANGLES) {
    const int na = A - a0 < RV_ANGLES ? A - a0 : RV_ANGLES;
    if (t < na) wire_sincos(angles[a0 + t] * RV_DEG2RAD, s_sn[t], s_cs[t]);
    __syncthreads();
    if (lane < na) {
      int cnt = 0;
      if (pix_ok) {
        const float sn = s_sn[lane], cs = s_cs[lane];
        // the pixel's inverse-rotated position in the (j, i) lattice, clamped so that the conversion is defined for
        // any angle (no candidate is lost: beyond the clamp the window holds no lattice point of the grid)
        const float js = fminf(fmaxf(cs * fx + sn * fy + cx, -4.f), (float)W + 4.f);
        const float is = fminf(fmaxf(cs * fy - sn * fx + cy, -4.f), (float)H + 4.f);
        const int jn = (int)rintf(js), in = (int)rintf(is);
        const int off_a = (a0 + lane) * W;
        for (int di = -2; di <= 2; ++di) {
          const int i = in + di;
          if (i < 0 || i >= H) continue;
          const float yi = (float)i - cy;
          for (int dj = -2; dj <= 2; ++dj) {
            const int j = jn + dj;
            if (j < 0 || j >= W) continue;
            const float xj = (float)j - cx;
            const float x = __builtin_fmaf(cs, xj, -(sn * yi)) + cx;
            const float y = __builtin_fmaf(sn, xj, cs * yi) + cy;
            const float xf = floorf(x), yf = floorf(y);
            const int x0 = (int)xf, y0 = (int)yf;
            if ((px != x0 && px != x0 + 1) || (py != y0 && py != y0 + 1)) continue;
            const float wx1 = x - xf, wy1 = y - yf;
            const float wx = px == x0 ? 1.f - wx1 : wx1, wy = py == y0 ? 1.f - wy1 : wy1;
            if (cnt < RV_MAXT) {
              s_tap[pl][lane][cnt].w = wy * wx;
              s_tap[pl][lane][cnt].off = off_a + j;
              ++cnt;
            }
          }
        }
      }
      s_cnt[pl][lane] = cnt;
    }
    __syncthreads();
    if (pix_ok && c < C) {
      for (int al = 0; al < na; ++al) {
        const int cnt = s_cnt[pl][al];
        for (int k = 0; k < cnt; ++k) {
          const rv_tap tp = s_tap[pl][al][k];
          acc = __builtin_fmaf(tp.w, g_sino[(long long)tp.off * C + c], acc);
        }
      }
    }
    __syncthreads();
  }
  if (pix_ok && c < C) g_vol[p * C + c] = acc;
}

// ---------------------------------------------------------------------------
// C ABI
// ---------------------------------------------------------------------------
static bool rv_bad_dims(int H, int W, int C, int A) {
  return H < 1 || W < 1 || C < 1 || A < 1 || (int64_t)H * W > INT_MAX || (int64_t)A * W > INT_MAX;
}

extern "C" int wire_radon_vol_fwd(void* stream, const float* vol, const float* angles_deg, int H, int W, int C,
                                  int nangles, float* sino) {
  if (rv_bad_dims(H, W, C, nangles) || !vol || !angles_deg || !sino)
    return fail(WIRE_ERR_ARG, "bad argument to wire_radon_vol_fwd");
  const bool v4 = C % 4 == 0 && ((uintptr_t)vol | (uintptr_t)sino) % 16 == 0;
  const int64_t chunks = ((int64_t)W * (v4 ? C / 4 : C) + 255) / 256;
  if (chunks * nangles > INT_MAX) return fail(WIRE_ERR_ARG, "wire_radon_vol_fwd: nangles * W * C is too large");
  ProfScope ps((hipStream_t)stream, 3, 0);
  dim3 grid((unsigned)(chunks * nangles));
  if (v4)
    hipLaunchKernelGGL(radon_vol_fwd_kernel<4>, grid, dim3(256), 0, (hipStream_t)stream, vol, angles_deg, H, W, C,
                       (unsigned)chunks, sino);
  else
    hipLaunchKernelGGL(radon_vol_fwd_kernel<1>, grid, dim3(256), 0, (hipStream_t)stream, vol, angles_deg, H, W, C,
                       (unsigned)chunks, sino);
  HIPCHK(hipGetLastError());
  return WIRE_OK;
}

extern "C" int wire_radon_vol_bwd(void* stream, const float* g_sino, const float* angles_deg, int H, int W, int C,
                                  int nangles, float* g_vol) {
  if (rv_bad_dims(H, W, C, nangles) || !g_sino || !angles_deg || !g_vol)
    return fail(WIRE_ERR_ARG, "bad argument to wire_radon_vol_bwd");
  const int cchunks = (C + 63) / 64;
  if (cchunks > 65535) return fail(WIRE_ERR_ARG, "wire_radon_vol_bwd: C is too large");
  ProfScope ps((hipStream_t)stream, 3, 0);
  dim3 grid((unsigned)(((int64_t)H * W + RV_TILE - 1) / RV_TILE), (unsigned)cchunks);
  hipLaunchKernelGGL(radon_vol_bwd_kernel, grid, dim3(256), 0, (hipStream_t)stream, g_sino, angles_deg, H, W, C,
                     nangles, g_vol);
  HIPCHK(hipGetLastError());
  return WIRE_OK;
}
