// wire_train.hip -- the glue of a training run around the net: the epoch's shuffle, coordinate generation (grid tables
// and per-frame rigid motion), the MSE, super-resolution and multi-image super-resolution losses with their gradients,
// flat Adam, evaluation metrics, best-so-far tracking, the sigmoid of the mesh export, and the CT forward operator
// (Radon transform) with its adjoint.
#include "wire_dev.h"
#include "wire_point.h"

// ===========================================================================
// training glue
// ===========================================================================
// Keyed bijection of [0, n): the per-epoch shuffle of wire_image_denoise.py:142 / wire_occupancy.py:137
// (torch.randperm) as a function of the POSITION, so that a rank generates exactly the slice of the epoch's
// permutation it trains on -- O(shard) work and memory per rank whatever the world size and the grid size
// (randperm sorts all n keys on every rank: 0.57 ms at n = 262 144, 1 GB of int64 at 512^3).
// b = bits of the smallest power of two >= n; four rounds of  x = (x * M_r + K_r) mod 2^b; x ^= x >> s  (each
// invertible mod 2^b), then cycle-walking: re-apply while x >= n (2^b < 2 n, so < 2 applications on average;
// it terminates because the walk stays on the cycle of a permutation of [0, 2^b) that contains the start).
// (tests/test_shuffle.py holds the bit-exact numpy twin.)
__device__ __host__ inline unsigned long long perm_splitmix(unsigned long long z) {
  z += 0x9e3779b97f4a7c15ull;
  z = (z ^ (z >> 30)) * 0xbf58476d1ce4e5b9ull;
  z = (z ^ (z >> 27)) * 0x94d049bb133111ebull;
  return z ^ (z >> 31);
}
struct PermKeys { unsigned long long m[4], k[4]; };
__device__ inline unsigned long long perm_apply(unsigned long long x, unsigned long long n, int b, int sh,
                                                const PermKeys& K) {
  const unsigned long long mask = (b >= 64) ? ~0ull : ((1ull << b) - 1ull);
  do {
#pragma unroll
    for (int r = 0; r < 4; ++r) {
      x = (x * K.m[r] + K.k[r]) & mask;
      x ^= x >> sh;
    }
  } while (x >= n);
  return x;
}
__global__ void perm_indices_kernel(PermKeys K, long long n_total, int b, int sh, long long first, long long count,
                                    int64_t* __restrict__ idx_out) {
  const long long r = (long long)blockIdx.x * blockDim.x + threadIdx.x;
  if (r >= count) return;
  idx_out[r] = (int64_t)perm_apply((unsigned long long)(first + r), (unsigned long long)n_total, b, sh, K);
}
hipError_t launch_perm_indices(hipStream_t s, uint64_t seed, int64_t n_total, int64_t first, int64_t count,
                               int64_t* idx_out) {
  if (count <= 0) return hipSuccess;
  if (n_total < 1 || first < 0 || first + count > n_total) return hipErrorInvalidValue;
  int b = 0;
  while (b < 63 && (1ull << b) < (unsigned long long)n_total) ++b;
  if (b == 0) b = 1;                       // n = 1: domain {0, 1}, cycle-walking maps 0 -> 0
  const int sh = b / 2 > 0 ? b / 2 : 1;
  PermKeys K;
  for (int r = 0; r < 4; ++r) {
    K.m[r] = perm_splitmix(seed * 8 + r) | 1ull;          // odd multiplier: a bijection mod 2^b
    K.k[r] = perm_splitmix(seed * 8 + 4 + r);
  }
  hipLaunchKernelGGL(perm_indices_kernel, dim3(cdiv(count, 256)), dim3(256), 0, s, K, (long long)n_total, b, sh,
                     (long long)first, (long long)count, idx_out);
  return hipGetLastError();
}

__global__ void coords_kernel(const int64_t* __restrict__ idx, long long first, long long n,
                              const float* __restrict__ tx, int W, const float* __restrict__ ty,
                              int H, const float* __restrict__ tz, int T,
                              float* __restrict__ coords) {
  const long long r = (long long)blockIdx.x * blockDim.x + threadIdx.x;
  if (r >= n) return;
  long long id = idx ? idx[r] : first + r;
  if (tz) {
    const long long k = id % T;
    id /= T;
    const long long j = id % W, i = id / W;
    coords[r * 3 + 0] = tx[j];
    coords[r * 3 + 1] = ty[i];
    coords[r * 3 + 2] = tz[k];
  } else {
    const long long j = id % W, i = id / W;
    coords[r * 2 + 0] = tx[j];
    coords[r * 2 + 1] = ty[i];
  }
}
hipError_t launch_coords(hipStream_t s, const int64_t* idx, int64_t first, int64_t n,
                         const float* tx, int W, const float* ty, int H, const float* tz, int T,
                         float* coords) {
  if (n <= 0) return hipSuccess;
  hipLaunchKernelGGL(coords_kernel, dim3(cdiv(n, 256)), dim3(256), 0, s, idx, (long long)first,
                     (long long)n, tx, W, ty, H, tz, T, coords);
  return hipGetLastError();
}

#define MSE_BLOCKS 1024
__global__ __launch_bounds__(256) void mse_grad_kernel(const float* __restrict__ y,
                                                       const float* __restrict__ target,
                                                       const int64_t* __restrict__ idx,
                                                       long long first, long long n, int O,
                                                       float gscale, float* __restrict__ g_y,
                                                       float* __restrict__ rec,
                                                       float* __restrict__ partial) {
  __shared__ float red[256];
  const long long total = n * O;
  float acc = 0.f;
  for (long long e = (long long)blockIdx.x * blockDim.x + threadIdx.x; e < total;
       e += (long long)gridDim.x * blockDim.x) {
    const long long r = e / O;
    const int o = (int)(e - r * O);
    const long long src = idx ? idx[r] : first + r;
    const float yy = y[e];
    const float d = yy - target[src * O + o];
    g_y[e] = gscale * d;
    if (rec) rec[src * O + o] = yy;
    acc = __builtin_fmaf(d, d, acc);
  }
  acc = wire_block_tree_sum(acc, red);
  if (threadIdx.x == 0) partial[blockIdx.x] = acc;
}
__global__ void mse_final_kernel(const float* __restrict__ partial, int nb, float lscale,
                                 float* __restrict__ loss_out) {
  __shared__ float red[256];
  float acc = 0.f;
  for (int i = threadIdx.x; i < nb; i += 256) acc += partial[i];
  acc = wire_block_tree_sum(acc, red);
  if (threadIdx.x == 0) loss_out[0] = acc * lscale;
}
// the grid of a loss kernel over n elements: it depends on the shape alone
unsigned mse_blocks(long long n) { return n < (long long)MSE_BLOCKS * 256 ? cdiv(n, 256) : MSE_BLOCKS; }
// loss_out[0] = lscale * sum of nb partial sums (one block)
hipError_t launch_mse_final(hipStream_t s, const float* partial, int nb, float lscale, float* loss_out) {
  hipLaunchKernelGGL(mse_final_kernel, dim3(1), dim3(256), 0, s, partial, nb, lscale, loss_out);
  return hipGetLastError();
}
hipError_t launch_mse_grad(hipStream_t s, const float* y, const float* target, const int64_t* idx,
                           int64_t first, int64_t n, int O, float weight, float* g_y,
                           float* loss_out, float* rec, float* partial) {
  if (n <= 0) return hipSuccess;
  const unsigned nb = mse_blocks(n * O);
  const float inv = (float)(1.0 / ((double)n * (double)O));
  hipLaunchKernelGGL(mse_grad_kernel, dim3(nb), dim3(256), 0, s, y, target, idx, (long long)first,
                     (long long)n, O, weight * 2.f * inv, g_y, rec, partial);
  return launch_mse_final(s, partial, (int)nb, weight * inv, loss_out);
}

// ===========================================================================
// super-resolution loss (wire_SISR.py:151-161): rec = AvgPool2d(scale)(rec_hr as [O][H][W]),
// loss = mean((gt_lr - rec)^2) over H2 W2 O, H2 = H / scale, W2 = W / scale (floor: AvgPool2d's default
// ceil_mode = False drops ragged borders).  One thread per pooled element; it also scatters
// dL/d rec_hr = 2 (rec - gt_lr) / (H2 W2 O scale^2) to its scale x scale window.  y, g_y: [H W][O].
// ===========================================================================
__global__ __launch_bounds__(256) void avgpool_mse_grad_kernel(const float* __restrict__ y, int H, int W, int O,
                                                               int sc, int H2, int W2,
                                                               const float* __restrict__ gt_lr, float gscale,
                                                               float* __restrict__ g_y,
                                                               float* __restrict__ rec_lr,
                                                               float* __restrict__ partial) {
  __shared__ float red[256];
  const long long total = (long long)H2 * W2 * O;
  const float inv = 1.f / (float)(sc * sc);
  float acc = 0.f;
  for (long long e = (long long)blockIdx.x * blockDim.x + threadIdx.x; e < total;
       e += (long long)gridDim.x * blockDim.x) {
    const long long pix = e / O;
    const int o = (int)(e - pix * O);
    const int pi = (int)(pix / W2), pj = (int)(pix - (long long)pi * W2);
    const float* src = y + ((size_t)(pi * sc) * W + (size_t)pj * sc) * O + o;
    float sum = 0.f;
    for (int a = 0; a < sc; ++a)
      for (int b = 0; b < sc; ++b) sum += src[((size_t)a * W + b) * O];
    const float pool = sum * inv;
    const float d = pool - gt_lr[e];
    if (rec_lr) rec_lr[e] = pool;
    const float g = gscale * d;
    float* dst = g_y + ((size_t)(pi * sc) * W + (size_t)pj * sc) * O + o;
    for (int a = 0; a < sc; ++a)
      for (int b = 0; b < sc; ++b) dst[((size_t)a * W + b) * O] = g;
    acc = __builtin_fmaf(d, d, acc);
  }
  acc = wire_block_tree_sum(acc, red);
  if (threadIdx.x == 0) partial[blockIdx.x] = acc;
}
hipError_t launch_avgpool_mse_grad(hipStream_t s, const float* y, int H, int W, int O, int scale,
                                   const float* gt_lr, float* g_y, float* rec_lr, float* loss_out,
                                   float* partial) {
  const int H2 = H / scale, W2 = W / scale;
  if (H2 < 1 || W2 < 1) return hipErrorInvalidValue;
  // ragged borders receive no gradient
  if (H2 * scale != H || W2 * scale != W) {
    hipError_t e = hipMemsetAsync(g_y, 0, (size_t)H * W * O * sizeof(float), s);
    if (e != hipSuccess) return e;
  }
  const long long total = (long long)H2 * W2 * O;
  const unsigned nb = mse_blocks(total);
  const double invn = 1.0 / (double)total;
  hipLaunchKernelGGL(avgpool_mse_grad_kernel, dim3(nb), dim3(256), 0, s, y, H, W, O, scale, H2, W2, gt_lr,
                     (float)(2.0 * invn / ((double)scale * scale)), g_y, rec_lr, partial);
  return launch_mse_final(s, partial, (int)nb, (float)invn, loss_out);
}

// ===========================================================================
// multi-image super-resolution loss (wire_multi_sr.py:190-208): B frames of [H W][O], each pooled on its own --
//   rec = AvgPool2d(scale)(frame), d = rec * m - gt * m, loss = mean(d^2) over all B H2 W2 O elements (masked ones
//   included, as MSELoss does), dL/drec = 2 d m / (B H2 W2 O), spread over the window as dL/drec / scale^2.
// A block takes one strip (frame, pooled row, tile of pooled columns): `scale` HR rows of a contiguous run of floats.
// Lanes read CONSECUTIVE floats of an HR row and add the strip's rows in a register (column sums), the column sums
// meet in LDS, one thread per pooled element adds its `scale` columns in a fixed order, and the gradient goes back
// out of LDS with lanes writing consecutive floats again.  Every element of g_y is written exactly once: the ragged
// right border by the last tile of a strip, the ragged bottom rows by the strips of the last pooled row (zeros).
// No atomics: per-block loss partials in a grid that depends on the shape alone, summed by mse_final_kernel.
// A window row wider than the LDS tile (scale * O > APF_CAP floats) takes the direct kernel below instead.
// ===========================================================================
#define APF_CAP 1024
__global__ __launch_bounds__(256) void avgpool_frames_kernel(const float* __restrict__ y, int B, int H, int W, int O,
                                                             int sc, int H2, int W2, int TP, int ntile,
                                                             const float* __restrict__ gt_lr,
                                                             const float* __restrict__ mask, float gscale,
                                                             float* __restrict__ g_y, float* __restrict__ rec_lr,
                                                             float* __restrict__ partial) {
  __shared__ float colsum[APF_CAP], gpool[APF_CAP], red[256];
  const long long rowf = (long long)W * O;                    // floats of an HR row
  const int pf = sc * O;                                       // floats of a window row (<= APF_CAP)
  const float inv = 1.f / ((float)sc * (float)sc);
  const long long njobs = (long long)B * H2 * ntile;
  const int tid = threadIdx.x;
  float acc = 0.f;
  for (long long job = blockIdx.x; job < njobs; job += gridDim.x) {
    const int t = (int)(job % ntile);
    const long long fr = job / ntile;
    const int pi = (int)(fr % H2);
    const long long f = fr / H2;
    const int p0 = t * TP;
    const int np = W2 - p0 < TP ? W2 - p0 : TP;
    const int nx = np * pf;                                    // floats of the tile in one HR row (<= APF_CAP)
    const long long x0 = (long long)p0 * pf;
    const long long hr0 = (f * H + (long long)pi * sc) * rowf + x0;
    for (int x = tid; x < nx; x += 256) {
      const float* src = y + hr0 + x;
      float s = 0.f;
      for (int a = 0; a < sc; ++a) s += src[a * rowf];
      colsum[x] = s;
    }
    __syncthreads();
    const long long pbase = ((f * H2 + pi) * W2 + p0) * O;
    for (int e = tid; e < np * O; e += 256) {
      const int pl = e / O, o = e - pl * O;
      const float* cs = colsum + pl * pf + o;
      float s = 0.f;
      for (int b = 0; b < sc; ++b) s += cs[b * O];
      const float pool = s * inv;
      const float m = mask ? mask[pbase + e] : 1.f;
      const float d = __fmul_rn(pool, m) - __fmul_rn(gt_lr[pbase + e], m);
      if (rec_lr) rec_lr[pbase + e] = pool;
      gpool[e] = gscale * (d * m);
      acc = __builtin_fmaf(d, d, acc);
    }
    __syncthreads();
    // (the next strip's colsum is written behind this barrier and its gpool behind the next one: no third barrier)
    const int nxw = t == ntile - 1 ? (int)(rowf - x0) : nx;     // the last tile also owns the ragged right border
    for (int a = 0; a < sc; ++a) {
      float* dst = g_y + hr0 + a * rowf;
      for (int x = tid; x < nxw; x += 256) {
        const int pl = x / pf;
        dst[x] = x < nx ? gpool[pl * O + (x - pl * pf) % O] : 0.f;
      }
    }
    if (pi == H2 - 1)
      for (int i = H2 * sc; i < H; ++i) {
        float* dst = g_y + (f * H + i) * rowf + x0;
        for (int x = tid; x < nxw; x += 256) dst[x] = 0.f;
      }
  }
  acc = wire_block_tree_sum(acc, red);
  if (tid == 0) partial[blockIdx.x] = acc;
}
// scale * O > APF_CAP: one thread per pooled element reads and writes its own window (g_y's ragged borders are zeroed
// by the launcher)
__global__ __launch_bounds__(256) void avgpool_frames_direct_kernel(const float* __restrict__ y, int B, int H, int W,
                                                                    int O, int sc, int H2, int W2,
                                                                    const float* __restrict__ gt_lr,
                                                                    const float* __restrict__ mask, float gscale,
                                                                    float* __restrict__ g_y,
                                                                    float* __restrict__ rec_lr,
                                                                    float* __restrict__ partial) {
  __shared__ float red[256];
  const long long total = (long long)B * H2 * W2 * O;
  const long long rowf = (long long)W * O;
  const float inv = 1.f / ((float)sc * (float)sc);
  float acc = 0.f;
  for (long long e = (long long)blockIdx.x * blockDim.x + threadIdx.x; e < total;
       e += (long long)gridDim.x * blockDim.x) {
    const long long pix = e / O;
    const int o = (int)(e - pix * O);
    const int pj = (int)(pix % W2);
    const long long fr = pix / W2;
    const int pi = (int)(fr % H2);
    const long long f = fr / H2;
    const long long off = (f * H + (long long)pi * sc) * rowf + (long long)pj * sc * O + o;
    float sum = 0.f;
    for (int a = 0; a < sc; ++a)
      for (int b = 0; b < sc; ++b) sum += y[off + a * rowf + (long long)b * O];
    const float pool = sum * inv;
    const float m = mask ? mask[e] : 1.f;
    const float d = __fmul_rn(pool, m) - __fmul_rn(gt_lr[e], m);
    if (rec_lr) rec_lr[e] = pool;
    const float g = gscale * (d * m);
    for (int a = 0; a < sc; ++a)
      for (int b = 0; b < sc; ++b) g_y[off + a * rowf + (long long)b * O] = g;
    acc = __builtin_fmaf(d, d, acc);
  }
  acc = wire_block_tree_sum(acc, red);
  if (threadIdx.x == 0) partial[blockIdx.x] = acc;
}
hipError_t launch_avgpool_mse_grad_frames(hipStream_t s, const float* y, int B, int H, int W, int O, int scale,
                                          const float* gt_lr, const float* mask, float* g_y, float* rec_lr,
                                          float* loss_out, float* partial) {
  const int H2 = H / scale, W2 = W / scale;
  if (B < 1 || O < 1 || H2 < 1 || W2 < 1) return hipErrorInvalidValue;
  const double total = (double)B * H2 * W2 * O;
  const float gscale = (float)(2.0 / total / ((double)scale * scale));
  unsigned nb;
  if ((long long)scale * O <= APF_CAP) {
    const int cap = APF_CAP / (scale * O);
    const int TP = W2 < cap ? W2 : cap;
    const int ntile = (W2 + TP - 1) / TP;
    const long long njobs = (long long)B * H2 * ntile;
    nb = njobs < MSE_BLOCKS ? (unsigned)njobs : MSE_BLOCKS;
    hipLaunchKernelGGL(avgpool_frames_kernel, dim3(nb), dim3(256), 0, s, y, B, H, W, O, scale, H2, W2, TP, ntile,
                       gt_lr, mask, gscale, g_y, rec_lr, partial);
  } else {
    if (H2 * scale != H || W2 * scale != W) {
      hipError_t e = hipMemsetAsync(g_y, 0, (size_t)B * H * W * O * sizeof(float), s);
      if (e != hipSuccess) return e;
    }
    const long long n = (long long)total;
    nb = mse_blocks(n);
    hipLaunchKernelGGL(avgpool_frames_direct_kernel, dim3(nb), dim3(256), 0, s, y, B, H, W, O, scale, H2, W2, gt_lr,
                       mask, gscale, g_y, rec_lr, partial);
  }
  return launch_mse_final(s, partial, (int)nb, (float)(1.0 / total), loss_out);
}

// ===========================================================================
// video compressive sensing (modules/lin_inverse.py:42-95, the coded exposure of Hitomi et al.): the T frames of a
// pixel are multiplied by the pixel's mask and summed in groups of `nframes` into C = ceil(T / nframes) coded frames;
// with dup_last the last group is stored a second time (frame C == frame C - 1, as the reference's trailing
// `if idx < video_ten.shape[1]` does), so an MSE over the C' = C + dup_last frames weights it twice:
//   est[c][p][o] = sum_{k in chunk c} m[p][k] y[p T + k][o],   d = est - gt,   loss = sum d^2 / (C' NP O)
//   dL/dy[p T + k][o] = m[p][k] 2 / (C' NP O) (d[c(k)][p][o] + (dup_last and c(k) == C - 1 ? d[C][p][o] : 0))
// In the row order of the 3-D grid (idx = (i W + j) T + k) a pixel's T rows are T O consecutive floats of y and its T
// mask values are consecutive too.  A block takes a tile of whole pixels, a contiguous run of y: lanes read CONSECUTIVE
// floats, the masked products meet in LDS (pixel stride padded to an odd number of floats, so that the lanes of the
// chunk sums, one pixel apart, fall into different banks), one thread per (chunk, pixel, channel) adds its frames in
// order -- for a fixed chunk consecutive threads touch consecutive floats of gt / est -- and the gradient leaves LDS
// with lanes writing consecutive floats again.  y / g_y are local to the slab of pixels [p0, p0 + n_pix); mask, gt and
// est are indexed by the global pixel.  Every element of g_y is written exactly once.  No atomics: per-block loss
// partials in a grid that depends on the shape alone, summed by mse_final_kernel.  A pixel span wider than the LDS
// tile (T O > CV_CAP floats) takes the direct kernel below instead.
// ===========================================================================
#define CV_CAP 1024
__global__ __launch_bounds__(256) void coded_mse_grad_kernel(const float* __restrict__ y, long long p0,
                                                             long long n_pix, long long NP, int T, int O, int nf,
                                                             int C, int dup, int TP, int PS,
                                                             const float* __restrict__ mask,
                                                             const float* __restrict__ gt, float gscale,
                                                             float* __restrict__ g_y, float* __restrict__ est,
                                                             float* __restrict__ partial) {
  __shared__ float ym[CV_CAP], ms[CV_CAP], gd[CV_CAP], red[256];
  const int pf = T * O;                                        // floats of a pixel (PS = pf or pf + 1, odd)
  const long long njobs = (n_pix + TP - 1) / TP;
  const long long cstride = NP * O;                            // floats of a coded frame
  const int tid = threadIdx.x;
  float acc = 0.f;
  for (long long job = blockIdx.x; job < njobs; job += gridDim.x) {
    const long long l0 = job * TP;                             // first pixel of the tile, slab-local
    const int np = n_pix - l0 < TP ? (int)(n_pix - l0) : TP;
    const int nx = np * pf;                                    // floats of the tile (np * PS <= CV_CAP)
    const long long base = l0 * pf;
    const float* mrow = mask + (p0 + l0) * T;
    for (int x = tid; x < nx; x += 256) {
      const int pl = x / pf, r = x - pl * pf;
      const float m = mrow[pl * T + r / O];
      ms[pl * PS + r] = m;
      ym[pl * PS + r] = m * y[base + x];
    }
    __syncthreads();
    const int ne = np * O;                                     // coded values of the tile in one coded frame
    const long long cbase = (p0 + l0) * O;
    for (int e = tid; e < C * ne; e += 256) {
      const int c = e / ne, r = e - c * ne;
      const int pl = r / O, o = r - pl * O;
      const int k0 = c * nf, k1 = k0 + nf < T ? k0 + nf : T;
      const float* src = ym + pl * PS + o;
      float s = 0.f;
      for (int k = k0; k < k1; ++k) s += src[k * O];
      const long long ci = c * cstride + cbase + r;
      float d = s - gt[ci];
      if (est) est[ci] = s;
      acc = __builtin_fmaf(d, d, acc);
      if (dup && c == C - 1) {
        const float d2 = s - gt[ci + cstride];
        if (est) est[ci + cstride] = s;
        acc = __builtin_fmaf(d2, d2, acc);
        d += d2;
      }
      gd[e] = gscale * d;
    }
    __syncthreads();
    for (int x = tid; x < nx; x += 256) {
      const int pl = x / pf, r = x - pl * pf;
      const int k = r / O, o = r - k * O;
      g_y[base + x] = ms[pl * PS + r] * gd[(k / nf) * ne + pl * O + o];
    }
    __syncthreads();                                           // the next tile overwrites ms
  }
  acc = wire_block_tree_sum(acc, red);
  if (tid == 0) partial[blockIdx.x] = acc;
}
// T * O > CV_CAP: one thread per (pixel, channel) walks its own frames, chunk by chunk
__global__ __launch_bounds__(256) void coded_mse_grad_direct_kernel(const float* __restrict__ y, long long p0,
                                                                    long long n_pix, long long NP, int T, int O,
                                                                    int nf, int C, int dup,
                                                                    const float* __restrict__ mask,
                                                                    const float* __restrict__ gt, float gscale,
                                                                    float* __restrict__ g_y, float* __restrict__ est,
                                                                    float* __restrict__ partial) {
  __shared__ float red[256];
  const long long total = n_pix * O;
  const long long cstride = NP * O;
  float acc = 0.f;
  for (long long e = (long long)blockIdx.x * blockDim.x + threadIdx.x; e < total;
       e += (long long)gridDim.x * blockDim.x) {
    const long long pl = e / O;
    const int o = (int)(e - pl * O);
    const float* yp = y + pl * T * O + o;
    float* gp = g_y + pl * T * O + o;
    const float* mp = mask + (p0 + pl) * T;
    for (int c = 0; c < C; ++c) {
      const int k0 = c * nf, k1 = k0 + nf < T ? k0 + nf : T;
      float s = 0.f;
      for (int k = k0; k < k1; ++k) s += mp[k] * yp[(long long)k * O];
      const long long ci = c * cstride + (p0 + pl) * O + o;
      float d = s - gt[ci];
      if (est) est[ci] = s;
      acc = __builtin_fmaf(d, d, acc);
      if (dup && c == C - 1) {
        const float d2 = s - gt[ci + cstride];
        if (est) est[ci + cstride] = s;
        acc = __builtin_fmaf(d2, d2, acc);
        d += d2;
      }
      const float g = gscale * d;
      for (int k = k0; k < k1; ++k) gp[(long long)k * O] = mp[k] * g;
    }
  }
  acc = wire_block_tree_sum(acc, red);
  if (threadIdx.x == 0) partial[blockIdx.x] = acc;
}
hipError_t launch_coded_mse_grad(hipStream_t s, const float* y, int64_t p0, int64_t n_pix, int64_t NP, int T, int O,
                                 int nframes, int dup_last, const float* mask, const float* gt, float* g_y, float* est,
                                 float* loss_out, float* partial) {
  if (T < 1 || O < 1 || nframes < 1 || n_pix < 1 || NP < 1) return hipErrorInvalidValue;
  const int C = (int)(((long long)T + nframes - 1) / nframes);
  const double count = (double)(C + dup_last) * (double)NP * O;
  const float gscale = (float)(2.0 / count);
  const long long pf = (long long)T * O;
  const long long PS = pf | 1;                                 // odd pixel stride in LDS
  unsigned nb;
  if (PS <= CV_CAP) {
    const long long cap = CV_CAP / PS;
    const int TP = (int)(n_pix < cap ? n_pix : cap);
    const long long njobs = (n_pix + TP - 1) / TP;
    nb = njobs < MSE_BLOCKS ? (unsigned)njobs : MSE_BLOCKS;
    hipLaunchKernelGGL(coded_mse_grad_kernel, dim3(nb), dim3(256), 0, s, y, (long long)p0, (long long)n_pix,
                       (long long)NP, T, O, nframes, C, dup_last, TP, (int)PS, mask, gt, gscale, g_y, est, partial);
  } else {
    const long long n = (long long)n_pix * O;
    nb = mse_blocks(n);
    hipLaunchKernelGGL(coded_mse_grad_direct_kernel, dim3(nb), dim3(256), 0, s, y, (long long)p0, (long long)n_pix,
                       (long long)NP, T, O, nframes, C, dup_last, mask, gt, gscale, g_y, est, partial);
  }
  return launch_mse_final(s, partial, (int)nb, (float)(1.0 / count), loss_out);
}

// The same operator on the reference's frame-major tensors (video, masks [T][NP], coded [C'][NP]) and its adjoint:
// one thread per coded value (forward) / per video value (backward), lanes on consecutive pixels of a frame.
__global__ __launch_bounds__(256) void coded_fwd_kernel(const float* __restrict__ video, const float* __restrict__ masks,
                                                        int T, long long NP, int nf, int C, int dup,
                                                        float* __restrict__ coded) {
  const long long e = (long long)blockIdx.x * blockDim.x + threadIdx.x;
  if (e >= C * NP) return;
  const int c = (int)(e / NP);
  const long long p = e - c * NP;
  const int k0 = c * nf, k1 = k0 + nf < T ? k0 + nf : T;
  float s = 0.f;
  for (int k = k0; k < k1; ++k) s += video[k * NP + p] * masks[k * NP + p];
  coded[e] = s;
  if (dup && c == C - 1) coded[e + NP] = s;
}
__global__ __launch_bounds__(256) void coded_bwd_kernel(const float* __restrict__ g_coded,
                                                        const float* __restrict__ masks, int T, long long NP, int nf,
                                                        int C, int dup, float* __restrict__ g_video) {
  const long long e = (long long)blockIdx.x * blockDim.x + threadIdx.x;
  if (e >= T * NP) return;
  const int k = (int)(e / NP);
  const long long p = e - k * NP;
  const int c = k / nf;
  float g = g_coded[c * NP + p];
  if (dup && c == C - 1) g += g_coded[C * NP + p];
  g_video[e] = masks[e] * g;
}
hipError_t launch_coded_fwd(hipStream_t s, const float* video, const float* masks, int T, int64_t NP, int nframes,
                            int dup_last, float* coded) {
  const int C = (int)(((long long)T + nframes - 1) / nframes);
  hipLaunchKernelGGL(coded_fwd_kernel, dim3(cdiv((long long)C * NP, 256)), dim3(256), 0, s, video, masks, T,
                     (long long)NP, nframes, C, dup_last, coded);
  return hipGetLastError();
}
hipError_t launch_coded_bwd(hipStream_t s, const float* g_coded, const float* masks, int T, int64_t NP, int nframes,
                            int dup_last, float* g_video) {
  const int C = (int)(((long long)T + nframes - 1) / nframes);
  hipLaunchKernelGGL(coded_bwd_kernel, dim3(cdiv((long long)T * NP, 256)), dim3(256), 0, s, g_coded, masks, T,
                     (long long)NP, nframes, C, dup_last, g_video);
  return hipGetLastError();
}

// The coordinate stack of motion.get_imstack at scale = 1 (modules/motion.py:284-318 as wire_multi_sr.py:74-78 calls
// it): frame f's pixel (i, j) moved by its 2 x 3 matrix, then normalised -- all in fp64, rounded to fp32 once.
__global__ void affine_coords_kernel(const double* __restrict__ mats, long long n, int H, int W,
                                     float* __restrict__ coords) {
#pragma clang fp contract(off)
  const long long r = (long long)blockIdx.x * blockDim.x + threadIdx.x;
  if (r >= n) return;
  const long long hw = (long long)H * W;
  const long long f = r / hw, p = r - f * hw;
  const double i = (double)(p / W), j = (double)(p % W);
  const double* m = mats + f * 6;
  const double xn = m[0] * j + m[1] * i + m[2];
  const double yn = m[3] * j + m[4] * i + m[5];
  coords[r * 2 + 0] = (float)(2.0 * xn / (double)W - 1.0);
  coords[r * 2 + 1] = (float)(2.0 * yn / (double)H - 1.0);
}
hipError_t launch_affine_coords(hipStream_t s, const double* mats, int B, int H, int W, float* coords) {
  const long long n = (long long)B * H * W;
  hipLaunchKernelGGL(affine_coords_kernel, dim3(cdiv(n, 256)), dim3(256), 0, s, mats, n, H, W, coords);
  return hipGetLastError();
}

// torch.optim.Adam (_single_tensor_adam): m = b1 m + (1-b1) g; v = b2 v + (1-b2) g^2;
// denom = sqrt(v)/sqrt(bc2) + eps; p -= (lr/bc1) m/denom
__global__ void adam_kernel(float* __restrict__ p, const float* __restrict__ g,
                            float* __restrict__ m, float* __restrict__ v, long long count,
                            float step_size, float beta1, float beta2, float eps,
                            float inv_sqrt_bc2) {
  const long long i = (long long)blockIdx.x * blockDim.x + threadIdx.x;
  if (i >= count) return;
  const float gg = g[i];
  const float mm = __builtin_fmaf(beta1, m[i], (1.f - beta1) * gg);
  const float vv = __builtin_fmaf(beta2, v[i], (1.f - beta2) * gg * gg);
  m[i] = mm;
  v[i] = vv;
  const float denom = __builtin_fmaf(__builtin_sqrtf(vv), inv_sqrt_bc2, eps);
  p[i] = p[i] - step_size * (mm / denom);
}
hipError_t launch_adam(hipStream_t s, float* p, const float* g, float* m, float* v, int64_t count,
                       float step_size, float beta1, float beta2, float eps, float inv_sqrt_bc2) {
  if (count <= 0) return hipSuccess;
  hipLaunchKernelGGL(adam_kernel, dim3(cdiv(count, 256)), dim3(256), 0, s, p, g, m, v,
                     (long long)count, step_size, beta1, beta2, eps, inv_sqrt_bc2);
  return hipGetLastError();
}

// ===========================================================================
// evaluation metrics on device (wire_image_denoise.py:161-178, wire_occupancy.py:160-162):
//   mode 0: out = { sum (gt - rec)^2, max gt }            -> PSNR = 10 log10(max(x) / mse)
//   mode 1: out = { |pred>=thres AND gt!=0|, |pred>=thres OR gt!=0| }   -> IoU
// two-level deterministic reduction (block partials, then one block)
// ===========================================================================
#define MET_BLOCKS 1024
__global__ __launch_bounds__(256) void metric_kernel(int mode, const float* __restrict__ rec,
                                                     const float* __restrict__ gt, long long count,
                                                     float thres, float* __restrict__ partial) {
  __shared__ float r0[256], r1[256];
  float a = 0.f, b = mode == 0 ? -3.4e38f : 0.f;
  for (long long e = (long long)blockIdx.x * 256 + threadIdx.x; e < count; e += (long long)gridDim.x * 256) {
    const float x = gt[e], y = rec[e];
    if (mode == 0) {
      const float d = x - y;
      a = __builtin_fmaf(d, d, a);
      b = x > b ? x : b;
    } else {
      const bool p = y >= thres, q = x != 0.f;
      a += (p && q) ? 1.f : 0.f;
      b += (p || q) ? 1.f : 0.f;
    }
  }
  r0[threadIdx.x] = a; r1[threadIdx.x] = b;
  __syncthreads();
  for (int sft = 128; sft >= 1; sft >>= 1) {
    if (threadIdx.x < sft) {
      r0[threadIdx.x] += r0[threadIdx.x + sft];
      r1[threadIdx.x] = mode == 0 ? (r1[threadIdx.x] > r1[threadIdx.x + sft] ? r1[threadIdx.x] : r1[threadIdx.x + sft])
                                  : r1[threadIdx.x] + r1[threadIdx.x + sft];
    }
    __syncthreads();
  }
  if (threadIdx.x == 0) { partial[2 * blockIdx.x] = r0[0]; partial[2 * blockIdx.x + 1] = r1[0]; }
}
__global__ void metric_final_kernel(int mode, const float* __restrict__ partial, int nb, float* __restrict__ out) {
  __shared__ float r0[256], r1[256];
  float a = 0.f, b = mode == 0 ? -3.4e38f : 0.f;
  for (int i = threadIdx.x; i < nb; i += 256) {
    a += partial[2 * i];
    const float v = partial[2 * i + 1];
    b = mode == 0 ? (v > b ? v : b) : b + v;
  }
  r0[threadIdx.x] = a; r1[threadIdx.x] = b;
  __syncthreads();
  for (int sft = 128; sft >= 1; sft >>= 1) {
    if (threadIdx.x < sft) {
      r0[threadIdx.x] += r0[threadIdx.x + sft];
      r1[threadIdx.x] = mode == 0 ? (r1[threadIdx.x] > r1[threadIdx.x + sft] ? r1[threadIdx.x] : r1[threadIdx.x + sft])
                                  : r1[threadIdx.x] + r1[threadIdx.x + sft];
    }
    __syncthreads();
  }
  if (threadIdx.x == 0) { out[0] = r0[0]; out[1] = r1[0]; }
}
hipError_t launch_metric(hipStream_t s, int mode, const float* rec, const float* gt, int64_t count, float thres,
                         float* out, float* partial) {
  if (count <= 0) return hipErrorInvalidValue;
  unsigned nb = cdiv(count, 256);
  if (nb > MET_BLOCKS) nb = MET_BLOCKS;
  hipLaunchKernelGGL(metric_kernel, dim3(nb), dim3(256), 0, s, mode, rec, gt, (long long)count, thres, partial);
  hipLaunchKernelGGL(metric_final_kernel, dim3(1), dim3(256), 0, s, mode, partial, (int)nb, out);
  return hipGetLastError();
}

// ===========================================================================
// best-reconstruction tracking without a host round trip (wire_image_denoise.py:176-178:
//   if (mse_array[epoch] < best_mse) or (epoch == 0): best_mse = ...; best_img = imrec
// wire_occupancy.py:170-172: if lossval < best_mse: ...; best_img = copy.deepcopy(im_estim)).
// Every thread reads the two scalars; the scalar itself is updated by a second one-thread launch.
// ===========================================================================
__global__ void best_copy_kernel(const float* __restrict__ metric, const float* __restrict__ best, int force,
                                 const float* __restrict__ src, float* __restrict__ dst, long long count) {
  if (!(force || metric[0] < best[0])) return;
  const long long i = ((long long)blockIdx.x * blockDim.x + threadIdx.x) * 4;
  if (i + 3 < count) {
    *reinterpret_cast<f32x4*>(dst + i) = *reinterpret_cast<const f32x4*>(src + i);
  } else {
    for (long long j = i; j < count; ++j) dst[j] = src[j];
  }
}
__global__ void best_scalar_kernel(const float* __restrict__ metric, float* __restrict__ best, int force,
                                   int* __restrict__ updated) {
  const bool take = force || metric[0] < best[0];
  if (take) best[0] = metric[0];
  if (updated) updated[0] = take ? 1 : 0;
}
hipError_t launch_track_best(hipStream_t s, const float* metric, float* best, int force, const float* src,
                             float* dst, int64_t count, int* updated) {
  if (count > 0)
    hipLaunchKernelGGL(best_copy_kernel, dim3(cdiv(count, 1024)), dim3(256), 0, s, metric, best, force, src, dst,
                       (long long)count);
  hipLaunchKernelGGL(best_scalar_kernel, dim3(1), dim3(1), 0, s, metric, best, force, updated);
  return hipGetLastError();
}

// torch.sigmoid of the dense occupancy query before the cube is written out (modules/volutils.py:128-131)
// wire_exp takes finite arguments below its overflow point (wire_dev.h), so it is evaluated on a = -min(|x|, 128) and
// the result is 1 / (1 + e) or e / (1 + e) by the sign of x; at a = -128 e is 0, which is also the answer for +-inf.
// Below -64 the argument is shifted by 32 (exact: both are multiples of 2^-17) and e^-32 is multiplied back, so that
// the hardware exp2, which flushes a denormal result, stays in its normal range and the product rounds into the
// denormals.  NaN keeps its bits.
__global__ void sigmoid_kernel(float* __restrict__ x, long long count) {
  const long long i = (long long)blockIdx.x * blockDim.x + threadIdx.x;
  if (i >= count) return;
  const float v = x[i];
  if (v != v) return;
  const float a = -fminf(fabsf(v), 128.f);
  const float e = a < -64.f ? wire_exp(a + 32.f) * 1.2664165549e-14f : wire_exp(a);
  x[i] = v >= 0.f ? 1.f / (1.f + e) : e / (1.f + e);
}
hipError_t launch_sigmoid(hipStream_t s, float* x, int64_t count) {
  if (count <= 0) return hipSuccess;
  hipLaunchKernelGGL(sigmoid_kernel, dim3(cdiv(count, 256)), dim3(256), 0, s, x, (long long)count);
  return hipGetLastError();
}

// ===========================================================================
// CT forward operator (modules/lin_inverse.py:19-40, wire_ct.py:128-133): the parallel-beam Radon transform the
// reference builds from kornia.geometry.rotate (kornia 0.6.5: get_rotation_matrix2d about ((W-1)/2, (H-1)/2),
// positive angle = counter-clockwise, warp_affine -> affine_grid + grid_sample, bilinear, zero padding,
// align_corners = True) followed by a sum over the rows:
//     sino[a][j] = sum_i  bilinear(img, x = c (j - cx) - s (i - cy) + cx,  y = s (j - cx) + c (i - cy) + cy)
// with c = cos(theta_a), s = sin(theta_a).  Samples within one pixel outside the image interpolate against zero.
// Pinned by the gt -> sinogram pair the reference stores (multiscale_results/ct/.../info.mat).
// Forward: one thread per (angle, column), rows in the loop -> reads of a row walk a straight line of the image.
// Backward (the adjoint, for dL/dimg): same traversal, four atomic adds per sample.
// ===========================================================================
template <bool BWD>
__global__ __launch_bounds__(256) void radon_kernel(const float* __restrict__ img, const float* __restrict__ angles,
                                                    int H, int W, int A, float* __restrict__ sino,
                                                    const float* __restrict__ g_sino, float* __restrict__ g_img) {
  const int j = blockIdx.x * blockDim.x + threadIdx.x;
  const int a = blockIdx.y;
  if (j >= W) return;
  const float th = angles[a] * 0.017453292519943295f;
  float sn, cs;
  wire_sincos(th, sn, cs);
  const float cx = 0.5f * (float)(W - 1), cy = 0.5f * (float)(H - 1);
  const float xj = (float)j - cx;
  const float g = BWD ? g_sino[(size_t)a * W + j] : 0.f;
  float acc = 0.f;
  for (int i = 0; i < H; ++i) {
    const float yi = (float)i - cy;
    const float x = __builtin_fmaf(cs, xj, -(sn * yi)) + cx;
    const float y = __builtin_fmaf(sn, xj, cs * yi) + cy;
    const float xf = floorf(x), yf = floorf(y);
    const int x0 = (int)xf, y0 = (int)yf;
    if (x0 < -1 || x0 >= W || y0 < -1 || y0 >= H) continue;
    const float wx1 = x - xf, wy1 = y - yf, wx0 = 1.f - wx1, wy0 = 1.f - wy1;
    const bool vx0 = x0 >= 0, vx1 = x0 + 1 < W, vy0 = y0 >= 0, vy1 = y0 + 1 < H;
    if (!BWD) {
      float v = 0.f;
      if (vy0) {
        const float* r = img + (size_t)y0 * W;
        if (vx0) v += wy0 * wx0 * r[x0];
        if (vx1) v += wy0 * wx1 * r[x0 + 1];
      }
      if (vy1) {
        const float* r = img + (size_t)(y0 + 1) * W;
        if (vx0) v += wy1 * wx0 * r[x0];
        if (vx1) v += wy1 * wx1 * r[x0 + 1];
      }
      acc += v;
    } else {
      if (vy0) {
        float* r = g_img + (size_t)y0 * W;
        if (vx0) atomicAdd(r + x0, g * wy0 * wx0);
        if (vx1) atomicAdd(r + x0 + 1, g * wy0 * wx1);
      }
      if (vy1) {
        float* r = g_img + (size_t)(y0 + 1) * W;
        if (vx0) atomicAdd(r + x0, g * wy1 * wx0);
        if (vx1) atomicAdd(r + x0 + 1, g * wy1 * wx1);
      }
    }
  }
  if (!BWD) sino[(size_t)a * W + j] = acc;
}
hipError_t launch_radon_fwd(hipStream_t s, const float* img, const float* angles, int H, int W, int A, float* sino) {
  dim3 grid(cdiv(W, 256), (unsigned)A);
  hipLaunchKernelGGL(radon_kernel<false>, grid, dim3(256), 0, s, img, angles, H, W, A, sino, nullptr, nullptr);
  return hipGetLastError();
}
hipError_t launch_radon_bwd(hipStream_t s, const float* g_sino, const float* angles, int H, int W, int A,
                            float* g_img) {
  hipError_t e = hipMemsetAsync(g_img, 0, (size_t)H * W * sizeof(float), s);
  if (e != hipSuccess) return e;
  dim3 grid(cdiv(W, 256), (unsigned)A);
  hipLaunchKernelGGL(radon_kernel<true>, grid, dim3(256), 0, s, nullptr, angles, H, W, A, nullptr, g_sino, g_img);
  return hipGetLastError();
}
