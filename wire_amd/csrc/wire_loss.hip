// wire_loss.hip -- pointwise data terms with a per-sample weight: the loss of a batch of rows and its gradient,
//   loss   = shard * sum_e w_e rho(y_e - t_e) / (n O)
//   g_y[e] = shard * w_e rho'(y_e - t_e) / (n O)
// for rho = the square (WIRE_LOSS_MSE), the absolute value (WIRE_LOSS_L1), Huber's function of width delta
// (WIRE_LOSS_HUBER) and the logistic loss of a logit y against a probability t (WIRE_LOSS_LOGISTIC).  The mean runs over
// every element, those of weight 0 included: torch's MSELoss()(out * mask, gt * mask), the convention of the masked
// super-resolution loss (wire_avgpool_mse_grad_frames).
//
// SHAPE: mse_grad_kernel's (wire_train.hip).  One grid-stride pass of 256-thread blocks, at most 1024 of them
// (mse_blocks: the grid depends on n*O alone), an element per thread and step; row r of y pairs with row
// src = idx ? idx[r] : first + r of the target, weight and rec tables.  A thread adds its terms in order, the block by
// the LDS tree (wire_block_tree_sum) into partial[block], one block adds the partials in a fixed order
// (launch_mse_final).  No atomics: the same call gives the same bits.  The kind and the weight form are template
// arguments, chosen once per launch; the element loop holds no branch on either.
//
//   L1: rho'(d) = (y > t) - (y < t), by comparison and not from the rounded difference: exactly +0 at a tie, as
//     torch.nn.L1Loss, whatever the denormal mode.
//   Huber: the quadratic branch at |d| <= delta (torch.nn.HuberLoss); both branches and both gradients agree at
//     |d| = delta, so which side a rounded |d| falls on moves the value by one rounding.
//   logistic: with e = exp(-|z|) in (0, 1],  rho = max(z, 0) - t z + log1p(e)  and  sigmoid(z) = 1 / (1 + e) for
//     z >= 0, e / (1 + e) for z < 0: no exponential of a positive argument, no inf / inf.  wire_exp (wire_dev.h)
//     takes finite arguments below its overflow point, so it sees -min(|z|, 128); e^-128 is 0 in fp32 (the hardware
//     exp2 flushes a denormal result, below e^-87.3), and then rho = max(z, 0) - t z and sigmoid = 1 or 0, which
//     is what fp32 holds of them.
//
// Plain MSE without weights is not a kernel of this file: the entry point forwards it to launch_mse_grad, so that
// g_y, loss_out and rec carry wire_mse_grad's bits.
//
// The entry point of the C ABI (include/wire_hip.h) is at the end of this file.
#include <cmath>

#include "wire_dev.h"
#include "wire_plan.h"

// weight forms: none (all ones), one per row, one per element
enum { LOSS_W_NONE = 0, LOSS_W_ROW = 1, LOSS_W_ELEM = 2 };

// rho(y - t) and rho'(y - t) of one element
template <int KIND>
WIRE_DEVINL void point_rho(float y, float t, float delta, float& v, float& g) {
  if (KIND == WIRE_LOSS_MSE) {
    const float d = y - t;
    v = d * d;
    g = 2.f * d;
  } else if (KIND == WIRE_LOSS_L1) {
    v = fabsf(y - t);
    g = (float)((int)(y > t) - (int)(y < t));
  } else if (KIND == WIRE_LOSS_HUBER) {
    const float d = y - t, ad = fabsf(d);
    v = ad <= delta ? 0.5f * d * d : delta * (ad - 0.5f * delta);
    g = fminf(fmaxf(d, -delta), delta);
  } else {
    const float e = wire_exp(-fminf(fabsf(y), 128.f));
    v = (fmaxf(y, 0.f) - t * y) + log1pf(e);
    g = (y >= 0.f ? 1.f / (1.f + e) : e / (1.f + e)) - t;
  }
}

template <int KIND, int WMODE>
__global__ __launch_bounds__(256) void point_loss_grad_kernel(const float* __restrict__ y,
                                                              const float* __restrict__ target,
                                                              const float* __restrict__ weight,
                                                              const int64_t* __restrict__ idx, long long first,
                                                              long long n, int O, float delta, float gscale,
                                                              float* __restrict__ g_y, float* __restrict__ rec,
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
    float v, g;
    point_rho<KIND>(yy, target[src * O + o], delta, v, g);
    if (WMODE == LOSS_W_NONE) {
      g_y[e] = gscale * g;
      acc += v;
    } else {
      const float w = WMODE == LOSS_W_ROW ? weight[src] : weight[src * O + o];
      g_y[e] = gscale * (w * g);
      acc = __builtin_fmaf(w, v, acc);
    }
    if (rec) rec[src * O + o] = yy;
  }
  acc = wire_block_tree_sum(acc, red);
  if (threadIdx.x == 0) partial[blockIdx.x] = acc;
}

template <int KIND>
static void launch_point_kind(hipStream_t s, unsigned nb, int wmode, const float* y, const float* target,
                              const float* weight, const int64_t* idx, long long first, long long n, int O, float delta,
                              float gscale, float* g_y, float* rec, float* partial) {
#define POINT_LAUNCH(W)                                                                                            \
  hipLaunchKernelGGL((point_loss_grad_kernel<KIND, W>), dim3(nb), dim3(256), 0, s, y, target, weight, idx, first, n, O, \
                     delta, gscale, g_y, rec, partial)
  if (wmode == LOSS_W_NONE) POINT_LAUNCH(LOSS_W_NONE);
  else if (wmode == LOSS_W_ROW) POINT_LAUNCH(LOSS_W_ROW);
  else POINT_LAUNCH(LOSS_W_ELEM);
#undef POINT_LAUNCH
}

hipError_t launch_point_loss_grad(hipStream_t s, int kind, float delta, const float* y, const float* target,
                                  const float* weight, int weight_per_elem, const int64_t* idx, int64_t first,
                                  int64_t n, int O, float shard, float* g_y, float* loss_out, float* rec,
                                  float* partial) {
  if (n <= 0) return hipSuccess;
  if (kind == WIRE_LOSS_MSE && !weight)
    return launch_mse_grad(s, y, target, idx, first, n, O, shard, g_y, loss_out, rec, partial);
  const unsigned nb = mse_blocks(n * O);
  const float scale = shard * (float)(1.0 / ((double)n * (double)O));
  const int wmode = !weight ? LOSS_W_NONE : weight_per_elem ? LOSS_W_ELEM : LOSS_W_ROW;
  switch (kind) {
    case WIRE_LOSS_MSE:
      launch_point_kind<WIRE_LOSS_MSE>(s, nb, wmode, y, target, weight, idx, first, n, O, delta, scale, g_y, rec, partial);
      break;
    case WIRE_LOSS_L1:
      launch_point_kind<WIRE_LOSS_L1>(s, nb, wmode, y, target, weight, idx, first, n, O, delta, scale, g_y, rec, partial);
      break;
    case WIRE_LOSS_HUBER:
      launch_point_kind<WIRE_LOSS_HUBER>(s, nb, wmode, y, target, weight, idx, first, n, O, delta, scale, g_y, rec,
                                         partial);
      break;
    case WIRE_LOSS_LOGISTIC:
      launch_point_kind<WIRE_LOSS_LOGISTIC>(s, nb, wmode, y, target, weight, idx, first, n, O, delta, scale, g_y, rec,
                                            partial);
      break;
    default:
      return hipErrorInvalidValue;
  }
  return launch_mse_final(s, partial, (int)nb, scale, loss_out);
}

// ---------------------------------------------------------------------------
// entry point of the C ABI
// ---------------------------------------------------------------------------
extern "C" int wire_point_loss_grad(void* stream, int kind, float delta, const float* y, const float* target,
                                    const float* weight, int weight_per_elem, const int64_t* idx, int64_t first,
                                    int64_t n, int O, float shard, float* g_y, float* loss_out, float* rec,
                                    float* partial) {
  const bool kind_ok = kind == WIRE_LOSS_MSE || kind == WIRE_LOSS_L1 || kind == WIRE_LOSS_HUBER ||
                       kind == WIRE_LOSS_LOGISTIC;
  if (!kind_ok || n < 0 || O < 1 || (kind == WIRE_LOSS_HUBER && !(std::isfinite(delta) && delta > 0.f)) ||
      !std::isfinite(shard) || (weight_per_elem != 0 && weight_per_elem != 1) || !y || !target || !g_y || !loss_out ||
      !partial)
    return fail(WIRE_ERR_ARG, "bad argument to wire_point_loss_grad");
  ProfScope ps((hipStream_t)stream, 3, 0);
  HIPCHK(launch_point_loss_grad((hipStream_t)stream, kind, delta, y, target, weight, weight_per_elem, idx, first, n, O,
                                shard, g_y, loss_out, rec, partial));
  return WIRE_OK;
}
