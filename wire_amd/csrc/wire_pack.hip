// wire_pack.hip -- weight packing: the native nn.Parameter tensors -> the padded images the GEMMs read (hidden layers,
// single and batched; the final linear; the blocked-planar complex matrices of the 3M path).  Runs once per optimizer step.
#include "wire_dev.h"
#include "wire_point.h"

// ===========================================================================
// packing
// ===========================================================================
// Hidden layer.  GEMM column j (output) and reduction index k (input) are in
// blocked-planar order.  Complex layer (modules/wire.py:89, F.linear without
// conjugation):  lin = z W^T  <=>  real image
//     [ (o,re),(i,re) ] =  W_re   [ (o,re),(i,im) ] = -W_im
//     [ (o,im),(i,re) ] =  W_im   [ (o,im),(i,im) ] =  W_re
// The data-gradient GEMM g_z = g_lin conj(W) uses exactly the transposed image.
// WS: the real kinds' W is multiplied by ws on the way in (launch_pack_hidden: wscale), the bias is not
template <bool WS>
WIRE_DEVINL void pack_hidden_body(int kind, const float* __restrict__ W, const float* __restrict__ b,
                                  const float* __restrict__ V, const float* __restrict__ c, int K,
                                  int Kin, int P, int Pin, int Nc, float* __restrict__ Bt_fwd,
                                  float* __restrict__ Bt_dgrad, float* __restrict__ bias, float ws) {
  const int k = blockIdx.x * blockDim.x + threadIdx.x;   // input (reduction) index
  const int j = blockIdx.y;                              // GEMM output column
  if (k >= Pin) return;
  float val = 0.f, bv = 0.f;
  if (kind == NK_WIRE || kind == NK_WIRE2D) {
    int o, part;
    const float* Wm = W;
    const float* bm = b;
    if (kind == NK_WIRE) {
      blk_decode(j, o, part);
    } else {
      const int sub = (j >> 5) & 3;
      o = ((j >> 7) << 5) + (j & 31);
      part = sub & 1;
      if (sub >= 2) { Wm = V; bm = c; }
    }
    int i, ipart;
    blk_decode(k, i, ipart);
    if (o < K) {
      bv = bm[2 * o + part];
      if (i < Kin) {
        const float wr = Wm[((size_t)o * Kin + i) * 2];
        const float wi = Wm[((size_t)o * Kin + i) * 2 + 1];
        val = part == 0 ? (ipart == 0 ? wr : -wi) : (ipart == 0 ? wi : wr);
      }
    }
  } else {
    if (j < K) {
      bv = b[j];
      if (k < Kin) val = WS ? ws * W[(size_t)j * Kin + k] : W[(size_t)j * Kin + k];
    }
  }
  Bt_fwd[(size_t)j * Pin + k] = val;
  Bt_dgrad[(size_t)k * Nc + j] = val;
  if (k == 0) bias[j] = bv;
}
template <bool WS>
__global__ void pack_hidden_kernel(int kind, const float* __restrict__ W, const float* __restrict__ b,
                                   const float* __restrict__ V, const float* __restrict__ c, int K,
                                   int Kin, int P, int Pin, int Nc, float* __restrict__ Bt_fwd,
                                   float* __restrict__ Bt_dgrad, float* __restrict__ bias, float ws) {
  pack_hidden_body<WS>(kind, W, b, V, c, K, Kin, P, Pin, Nc, Bt_fwd, Bt_dgrad, bias, ws);
}
// the same for up to PACK_MAXB layers of one shape in one launch (blockIdx.z = layer): wire_pack_params runs once per
// optimizer step, and a chain of ~5 us launches per layer costs more in launch gaps than in work
template <bool WS>
__global__ void pack_hidden_batch_kernel(int kind, PackBatch pb, int K, int Kin, int P, int Pin, int Nc, float ws) {
  const int z = blockIdx.z;
  pack_hidden_body<WS>(kind, pb.W[z], pb.b[z], pb.V[z], pb.c[z], K, Kin, P, Pin, Nc, pb.fwd[z], pb.dg[z], pb.bias[z], ws);
}
hipError_t launch_pack_hidden_batch(hipStream_t s, int kind, const PackBatch& pb, int nb, int K, int Kin, int P,
                                    int Pin, float wscale) {
  if (nb < 1 || nb > PACK_MAXB) return hipErrorInvalidValue;
  const int Nc = (kind == NK_WIRE2D) ? 2 * P : P;
  dim3 grid(cdiv(Pin, 128), (unsigned)Nc, (unsigned)nb);
  if (wscale != 1.f)
    hipLaunchKernelGGL(pack_hidden_batch_kernel<true>, grid, dim3(128), 0, s, kind, pb, K, Kin, P, Pin, Nc, wscale);
  else
    hipLaunchKernelGGL(pack_hidden_batch_kernel<false>, grid, dim3(128), 0, s, kind, pb, K, Kin, P, Pin, Nc, 1.f);
  return hipGetLastError();
}

hipError_t launch_pack_hidden(hipStream_t s, int kind, const float* W, const float* b,
                              const float* V, const float* c, int K, int Kin, int P, int Pin,
                              float* Bt_fwd, float* Bt_dgrad, float* bias, float wscale) {
  const int Nc = (kind == NK_WIRE2D) ? 2 * P : P;
  dim3 grid(cdiv(Pin, 128), (unsigned)Nc);
  if (wscale != 1.f)
    hipLaunchKernelGGL(pack_hidden_kernel<true>, grid, dim3(128), 0, s, kind, W, b, V, c, K, Kin, P, Pin,
                       Nc, Bt_fwd, Bt_dgrad, bias, wscale);
  else
    hipLaunchKernelGGL(pack_hidden_kernel<false>, grid, dim3(128), 0, s, kind, W, b, V, c, K, Kin, P, Pin,
                       Nc, Bt_fwd, Bt_dgrad, bias, 1.f);
  return hipGetLastError();
}

// dst = c src: the native copy of the cubic B-spline net's first-layer weights (c = its scale_0), read by the first-layer
// kernels and the coordinate gradient
__global__ void scale_copy_kernel(const float* __restrict__ src, long long n, float c, float* __restrict__ dst) {
  const long long i = (long long)blockIdx.x * blockDim.x + threadIdx.x;
  if (i < n) dst[i] = c * src[i];
}
hipError_t launch_scale_copy(hipStream_t s, const float* src, int64_t n, float c, float* dst) {
  if (n <= 0) return hipSuccess;
  hipLaunchKernelGGL(scale_copy_kernel, dim3(cdiv(n, 256)), dim3(256), 0, s, src, (long long)n, c, dst);
  return hipGetLastError();
}

// final nn.Linear(K, O, cfloat) + .real (modules/wire.py:156-157,164-165):
//   y = z_re W_re^T - z_im W_im^T + Re b
__global__ void pack_final_kernel(int kind, const float* __restrict__ Wf, const float* __restrict__ bf,
                                  int K, int P, int O, float* __restrict__ wf, float* __restrict__ bfr) {
  const int c = blockIdx.x * blockDim.x + threadIdx.x;
  const int o = blockIdx.y;
  if (c >= P) return;
  float val = 0.f;
  if (kind == NK_WIRE || kind == NK_WIRE2D) {
    int i, part;
    blk_decode(c, i, part);
    if (i < K) {
      const float w = Wf[((size_t)o * K + i) * 2 + part];
      val = part == 0 ? w : -w;
    }
    if (c == 0) bfr[o] = bf[2 * o];
  } else {
    if (c < K) val = Wf[(size_t)o * K + c];
    if (c == 0) bfr[o] = bf[o];
  }
  wf[(size_t)o * P + c] = val;
}

hipError_t launch_pack_final(hipStream_t s, int kind, const float* Wf, const float* bf, int K,
                             int P, int O, float* wf, float* bfr) {
  dim3 grid(cdiv(P, 128), (unsigned)O);
  hipLaunchKernelGGL(pack_final_kernel, grid, dim3(128), 0, s, kind, Wf, bf, K, P, O, wf, bfr);
  return hipGetLastError();
}

// ===========================================================================
// 3M complex path (wire_gemm3m.hip): weights as blocked-planar complex matrices
//   Wb_fwd[o][(i,re|im)] = W[o][i]            (lin = z W^T)
//   Wb_dg [i][(o,re|im)] = conj(W[o][i])      (g_z = g_lin conj(W))
// ===========================================================================
WIRE_DEVINL void pack3m_body(const float* __restrict__ W, const float* __restrict__ b, int K, int Kin,
                             int Kp, int Kpin, float* __restrict__ Wb_fwd, float* __restrict__ Wb_dg,
                             float* __restrict__ bias) {
  const int i = blockIdx.x * blockDim.x + threadIdx.x;   // input feature (padded)
  const int o = blockIdx.y;                              // output feature (padded)
  if (i >= Kpin) return;
  float wr = 0.f, wi = 0.f;
  if (o < K && i < Kin) {
    wr = W[((size_t)o * Kin + i) * 2];
    wi = W[((size_t)o * Kin + i) * 2 + 1];
  }
  const int ci = blk_col(i, 0), co = blk_col(o, 0);
  Wb_fwd[(size_t)o * (2 * Kpin) + ci] = wr;
  Wb_fwd[(size_t)o * (2 * Kpin) + ci + 32] = wi;
  Wb_dg[(size_t)i * (2 * Kp) + co] = wr;
  Wb_dg[(size_t)i * (2 * Kp) + co + 32] = -wi;
  if (i == 0) {
    bias[co] = o < K ? b[2 * o] : 0.f;
    bias[co + 32] = o < K ? b[2 * o + 1] : 0.f;
  }
}
__global__ void pack3m_kernel(const float* __restrict__ W, const float* __restrict__ b, int K, int Kin,
                              int Kp, int Kpin, float* __restrict__ Wb_fwd, float* __restrict__ Wb_dg,
                              float* __restrict__ bias) {
  pack3m_body(W, b, K, Kin, Kp, Kpin, Wb_fwd, Wb_dg, bias);
}
__global__ void pack3m_batch_kernel(PackBatch pb, int K, int Kin, int Kp, int Kpin) {
  const int z = blockIdx.z;
  pack3m_body(pb.W[z], pb.b[z], K, Kin, Kp, Kpin, pb.fwd[z], pb.dg[z], pb.bias[z]);
}
// up to PACK_MAXB layers per launch: pb.fwd / pb.dg / pb.bias = the 3M images and the (shared) blocked bias
hipError_t launch_pack3m_batch(hipStream_t s, const PackBatch& pb, int nb, int K, int Kin, int Kp, int Kpin) {
  if (nb < 1 || nb > PACK_MAXB) return hipErrorInvalidValue;
  dim3 grid(cdiv(Kpin, 64), (unsigned)Kp, (unsigned)nb);
  hipLaunchKernelGGL(pack3m_batch_kernel, grid, dim3(64), 0, s, pb, K, Kin, Kp, Kpin);
  return hipGetLastError();
}
hipError_t launch_pack3m(hipStream_t s, const float* W, const float* b, int K, int Kin, int Kp, int Kpin,
                         float* Wb_fwd, float* Wb_dg, float* bias) {
  dim3 grid(cdiv(Kpin, 64), (unsigned)Kp);
  hipLaunchKernelGGL(pack3m_kernel, grid, dim3(64), 0, s, W, b, K, Kin, Kp, Kpin, Wb_fwd, Wb_dg, bias);
  return hipGetLastError();
}
