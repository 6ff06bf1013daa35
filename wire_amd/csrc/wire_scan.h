// wire_scan.h -- an exclusive prefix sum of 32-bit counts on the device (internal; wave64 / CDNA4 only).
//
// SHAPE: multi-pass reduce-then-scan.  A tile is WIRE_SCAN_TILE = 1024 values, four per thread of a 256-thread block.
//   1. scan_sums_kernel:  sums[b] = the sum of tile b                                   (reads the input once)
//   2. the sums are scanned by the same routine, in place (recursively: 2^28 values are 262 144 tiles, those are
//      256 tiles, those are one)
//   3. scan_apply_kernel: out[i] = sums[tile of i] + the sum of the tile's values before i   (reads the input again)
// An input of at most one tile is step 3 alone.  No workgroup waits on another: no look-back, no spin, no grid barrier,
// no cooperative launch, no atomics -- the passes are separate launches on one stream, and every sum is added in an
// order that depends on n alone, so the same call gives the same bits whatever the buffers held before.
//
// The input is a functor, so that counts can be derived from what a kernel has stored (a mask byte) instead of being
// stored themselves:  void load4(long long base, long long n, unsigned (&v)[4]) const  fills v with the values of
// elements base .. base + 3 (0 beyond n); base is a multiple of 4.  `out` may be the array the functor reads (every
// thread reads its four values before it writes them and touches no others).  Sums wrap modulo 2^32: the caller bounds
// the total.
#pragma once
#include <hip/hip_runtime.h>
#include <stdint.h>

#define WIRE_SCAN_THREADS 256
#define WIRE_SCAN_ITEMS 4
#define WIRE_SCAN_TILE (WIRE_SCAN_THREADS * WIRE_SCAN_ITEMS)

// plain 32-bit values, 16-byte aligned (a section of a workspace)
struct ScanLoadU32 {
  const unsigned* x;
  __device__ __forceinline__ void load4(long long base, long long n, unsigned (&v)[4]) const {
    if (base + 4 <= n) {
      const uint4 q = *reinterpret_cast<const uint4*>(x + base);
      v[0] = q.x; v[1] = q.y; v[2] = q.z; v[3] = q.w;
    } else {
#pragma unroll
      for (int r = 0; r < 4; ++r) v[r] = base + r < n ? x[base + r] : 0u;
    }
  }
};

// exclusive scan of one value per thread over the block: returns the sum of the values of the threads before this one,
// and the block's total in `total` (every thread).  red: 4 words of LDS; barriers separate two uses.
__device__ __forceinline__ unsigned wire_block_exscan(unsigned v, unsigned* red, unsigned& total) {
  const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
  unsigned inc = v;
#pragma unroll
  for (int o = 1; o < 64; o <<= 1) {
    const unsigned t = (unsigned)__shfl_up((int)inc, o);
    if (lane >= o) inc += t;
  }
  __syncthreads();
  if (lane == 63) red[wave] = inc;
  __syncthreads();
  const unsigned w0 = red[0], w1 = red[1], w2 = red[2], w3 = red[3];
  total = w0 + w1 + w2 + w3;
  const unsigned before = wave == 0 ? 0u : wave == 1 ? w0 : wave == 2 ? w0 + w1 : w0 + w1 + w2;
  return before + inc - v;
}

template <class Load>
__global__ __launch_bounds__(WIRE_SCAN_THREADS) void scan_sums_kernel(Load ld, long long n,
                                                                      unsigned* __restrict__ sums) {
  __shared__ unsigned red[4];
  unsigned v[4];
  ld.load4((long long)blockIdx.x * WIRE_SCAN_TILE + threadIdx.x * WIRE_SCAN_ITEMS, n, v);
  unsigned total;
  wire_block_exscan(v[0] + v[1] + v[2] + v[3], red, total);
  if (threadIdx.x == 0) sums[blockIdx.x] = total;
}

// sums: the exclusive scan of the tiles' sums, or NULL for a single tile; total_out (single tile only): the sum of
// everything, as int64
template <class Load>
__global__ __launch_bounds__(WIRE_SCAN_THREADS) void scan_apply_kernel(Load ld, long long n, const unsigned* sums,
                                                                       unsigned* out, int64_t* total_out) {
  __shared__ unsigned red[4];
  const long long base = (long long)blockIdx.x * WIRE_SCAN_TILE + threadIdx.x * WIRE_SCAN_ITEMS;
  unsigned v[4];
  ld.load4(base, n, v);
  const unsigned tile_off = sums ? sums[blockIdx.x] : 0u;
  unsigned total;
  unsigned e0 = tile_off + wire_block_exscan(v[0] + v[1] + v[2] + v[3], red, total);
  const unsigned e1 = e0 + v[0], e2 = e1 + v[1], e3 = e2 + v[2];
  if (base + 4 <= n) {
    *reinterpret_cast<uint4*>(out + base) = make_uint4(e0, e1, e2, e3);
  } else {
    if (base < n) out[base] = e0;
    if (base + 1 < n) out[base + 1] = e1;
    if (base + 2 < n) out[base + 2] = e2;
  }
  if (total_out && threadIdx.x == 0) total_out[0] = (int64_t)total;
}

// 32-bit words of scratch that wire_scan_exclusive(n) needs: every level's sums, each level 16-byte aligned
static inline long long wire_scan_scratch_words(long long n) {
  long long w = 0;
  while (n > WIRE_SCAN_TILE) {
    n = (n + WIRE_SCAN_TILE - 1) / WIRE_SCAN_TILE;
    w += (n + 3) / 4 * 4;
  }
  return w;
}

// out[i] = sum of the values before i, i < n (out: 16-byte aligned, n words); total_out[0] = the sum of all n, as
// int64 (device; NULL = not wanted).  1 <= n < 2^31 * WIRE_SCAN_TILE.  scratch: wire_scan_scratch_words(n) words,
// 16-byte aligned.
template <class Load>
static hipError_t wire_scan_exclusive(hipStream_t s, Load ld, long long n, unsigned* out, unsigned* scratch,
                                      int64_t* total_out) {
  if (n <= WIRE_SCAN_TILE) {
    hipLaunchKernelGGL(scan_apply_kernel<Load>, dim3(1), dim3(WIRE_SCAN_THREADS), 0, s, ld, n,
                       (const unsigned*)nullptr, out, total_out);
    return hipGetLastError();
  }
  const long long nb = (n + WIRE_SCAN_TILE - 1) / WIRE_SCAN_TILE;
  hipLaunchKernelGGL(scan_sums_kernel<Load>, dim3((unsigned)nb), dim3(WIRE_SCAN_THREADS), 0, s, ld, n, scratch);
  hipError_t e = hipGetLastError();
  if (e != hipSuccess) return e;
  e = wire_scan_exclusive(s, ScanLoadU32{scratch}, nb, scratch, scratch + (nb + 3) / 4 * 4, total_out);
  if (e != hipSuccess) return e;
  hipLaunchKernelGGL(scan_apply_kernel<Load>, dim3((unsigned)nb), dim3(WIRE_SCAN_THREADS), 0, s, ld, n,
                     (const unsigned*)scratch, out, (int64_t*)nullptr);
  return hipGetLastError();
}
