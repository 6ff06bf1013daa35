// wire_point.h -- launchers of the bandwidth/VALU-bound kernels around the MFMA GEMMs, one group per source file.
//
// All of them move each activation byte at most once and keep 128-byte (32 lanes x 4 B) or 16-byte-per-lane accesses;
// none needs MFMA.  What several of the files must agree on (the row-block size of the final linear's partial sums, the
// output limit, the pre-reduction slack) is defined here, once.
#pragma once
#include <hip/hip_runtime.h>
#include <stdint.h>

#include "wire_gemm.h"   // with_kind, and wire_kinds.h through it

#define WIRE_MAXO 8        // outputs of the final linear (the point kernels keep one accumulator per output in registers)
// final_fwd_kernel keeps W_f [O][P] in dynamic LDS and a launch gets 64 KB of it without an opt-in: O x P floats at most.
// make_plan and wire_final_fwd refuse a wider net (WIRE_ERR_ARG) before anything is launched.
#define WIRE_FINAL_MAX_OP 16384
// rows of one block of the final linear's backward: every kernel that writes part_w / part_b for launch_final_reduce
// (final_bwd, final_fused, hier_head_bwd, mfn_final_bwd) uses this layout, final_bwd_blocks(n) blocks of it
#define WIRE_FB_ROWS 256
static inline unsigned cdiv(int64_t a, int64_t b) { return (unsigned)((a + b - 1) / b); }
// the two-stage reductions of wire_reduce.hip first sum a long list of per-block partials into at most PRE_CHUNKS chunks,
// written behind the blocks: a partial buffer of nblk blocks needs room for prereduce_room(nblk) of them
#define PRE_CHUNKS 32
static inline int prereduce_room(int nblk) { return nblk + PRE_CHUNKS; }

// ===========================================================================
// wire_pack.hip -- weight packing
// ===========================================================================
// ---- native nn.Parameter layout -> padded real-expanded image
hipError_t launch_pack_hidden(hipStream_t s, int kind, const float* W, const float* b,
                              const float* V, const float* c, int K, int Kin, int P, int Pin,
                              float* Bt_fwd, float* Bt_dgrad, float* bias, float wscale = 1.f);
// (wscale != 1, real kinds: the images hold wscale W, the bias stays as it is -- the cubic B-spline layer's scale_0, which
// multiplies the layer's input: s (x W^T) + b = x (s W)^T + b)
// several layers of one shape per launch (grid.z = layer)
#define PACK_MAXB 16
struct PackBatch {
  const float* W[PACK_MAXB]; const float* b[PACK_MAXB]; const float* V[PACK_MAXB]; const float* c[PACK_MAXB];
  float* fwd[PACK_MAXB]; float* dg[PACK_MAXB]; float* bias[PACK_MAXB];
};
hipError_t launch_pack_hidden_batch(hipStream_t s, int kind, const PackBatch& pb, int nb, int K, int Kin, int P,
                                    int Pin, float wscale = 1.f);
hipError_t launch_scale_copy(hipStream_t s, const float* src, int64_t n, float c, float* dst);   // dst = c src
hipError_t launch_pack3m_batch(hipStream_t s, const PackBatch& pb, int nb, int K, int Kin, int Kp, int Kpin);
hipError_t launch_pack_final(hipStream_t s, int kind, const float* Wf, const float* bf, int K,
                             int P, int O, float* wf, float* bfr);
// ---- 3M complex path: blocked-planar complex weight matrices
hipError_t launch_pack3m(hipStream_t s, const float* W, const float* b, int K, int Kin, int Kp, int Kpin,
                         float* Wb_fwd, float* Wb_dg, float* bias);

// ===========================================================================
// wire_first.hip -- the first stages, and the way back to the coordinates
// ===========================================================================
// ---- first layer (D <= 4 inputs): elementwise, VALU/HBM-write bound
// out [n][P] blocked; lin (optional): real nets [n][P]; wire: real u [n][P/2] (per-layer API)
hipError_t launch_first_fwd(hipStream_t s, int kind, const float* coords, int64_t n, int D,
                            const float* W0, const float* b0, const float* V0, const float* c0,
                            int K, int P, float omega, float scale, float* lin, float* out,
                            unsigned* amax_out = nullptr);   // amax_out: max |out| slots (wire_dev.h) or null

// ---- positional encoding (modules/relu.py:62-75) into a [n][Pin] padded row
hipError_t launch_posenc(hipStream_t s, const float* coords, int64_t n, int D, int F, int Pin,
                         float* dst);

// ---- the frozen first stage of the multi-scale B-spline net (modules/bspline_mscale_HL.py: Scaled_Bsplines_form)
// dst[r][j] = B(c[g(j)] (x_r . W0[j] + b0[j])) for j < SHF, 0 for SHF <= j < ld; g(j) = 0 below 256, else
// 1 + (j - 256) / split.  split_scale != 0 (ld % 4 == 0, 16-byte aligned rows): stored pre-split as wire_store_out4 does
// (B <= 0.75); else fp32, and amax (optional) receives max |value| for the 2 x fp16 GEMM that reads it.
struct MscaleC { float c[8]; };
hipError_t launch_mscale_first(hipStream_t s, const float* coords, int64_t n, int D, const float* W0, const float* b0,
                               int SHF, const MscaleC& c, int split, int ld, float split_scale, unsigned* amax,
                               float* dst);

// ---- coordinate gradients (first-order, fp32)
// g_x[r][d] = sum_k G[r][k] W[k][d] (+ sum_k G2[r][k] V[k][d]) over the K valid features of a stored first-layer gradient
// (real g_lin_0, wire g_u, wire2d g_u with G2 = g_p); W, V native [K][D].  One wave per row, fixed reduction order.
hipError_t launch_coordgrad_rows(hipStream_t s, const float* G, int ldg, const float* G2, const float* W, const float* V,
                                 int K, int D, int64_t n, float* g_x);
// g_x[r][d] = sum_t partial[t][r][d], t = 0 .. ntiles - 1 in that order (the data-gradient epilogue's per-column-tile
// partials, GemmEpiParams::cg_partial)
hipError_t launch_coordgrad_reduce(hipStream_t s, const float* partial, int ntiles, int64_t n, int D, float* g_x);
// modules/relu.py:62-75 backward: g_pe [n][ldpe] in posenc_kernel's feature order -> g_x [n][D]
hipError_t launch_posenc_bwd(hipStream_t s, const float* coords, int64_t n, int D, int F, const float* g_pe, int ldpe,
                             float* g_x);

// ===========================================================================
// wire_final.hip -- the final linear
// ===========================================================================
// ---- final linear: y[n][O] = z[n][P] . wf[O][P] + bf
hipError_t launch_final_fwd(hipStream_t s, const float* z, int64_t n, int P, int O,
                            const float* wf, const float* bfr, float* y);

// ---- final-layer backward fused with the last hidden activation gradient.
// g_out = g_y * wf; g_lin = act'(g_out; lin, out).  Also per-block partials of
// g_wf[o][c] = sum_n g_y[n][o] out[n][c] and of sum_n g_y[n][o].
// raw != 0: skip the activation gradient and write g_out itself (per-layer API).
int final_bwd_blocks(int64_t n);
hipError_t launch_final_bwd(hipStream_t s, int kind, int raw, const float* g_y, int64_t n, int O,
                            const float* wf, const float* lin, const float* out, int K, int P,
                            float omega, float scale, float* g_lin, float* part_w,
                            float* part_b, unsigned* amax_g = nullptr);   // amax_g: max |g_lin| slots or null

// ---- fused final stage of a training step (wire, O <= 4): y = Re(z Wf^T + bf), MSE loss + dL/dy,
// rec scatter, g_out = g_y conj(Wf), Gabor gradient of layer L, and the per-block partials of g_Wf /
// g_bf in the SAME layout launch_final_bwd produces (WIRE_FB_ROWS rows per block) for launch_final_reduce.
bool final_fused_supported(int P, int O);
hipError_t launch_final_fused(hipStream_t s, int kind, const float* out, const float* lin, int64_t n, int P, int O,
                              int kvalid, const float* wf, const float* bfr, const float* target, const int64_t* idx,
                              int64_t first, float weight, float omega, float scale, float* y, float* rec,
                              float* g_lin, float* part_w, float* part_b, float* loss_partial,
                              float* loss_out, unsigned* amax_g = nullptr);   // amax_g: max |g_lin| slots or null

// ===========================================================================
// wire_reduce.hip -- deterministic two-stage reductions
// ===========================================================================
// ---- the final linear's weight gradient from the per-block partials of launch_final_bwd and its kin:
// part_w / part_b must have room for prereduce_room(final_bwd_blocks(n)) blocks (pre-reduction scratch)
hipError_t launch_final_reduce(hipStream_t s, int kind, float* part_w, float* part_b,
                               int nblk, int O, int K, int P, float* gWf, float* gbf);

// ---- weight-gradient slab reduction: slab[S][Pm][Pn] (+ bslab[S][Pm]) -> native grads
hipError_t launch_wgrad_reduce(hipStream_t s, int kind, const float* slab, const float* bslab,
                               int S, int K, int Kin, int Pm, int Pn, float* gW, float* gb,
                               float* gV, float* gc, float wscale = 1.f);
// (wscale != 1, here and in the first-layer reductions below: g_W is multiplied by it on the way out, g_b is not -- the
// GEMMs ran on wscale W, so the slabs hold dL / d(wscale W))

// ---- first-layer weight gradient: g_W0[c][d] = sum_n G[n][c] x[n][d], g_b0[c] = sum_n G[n][c]
int colreduce_blocks(int64_t n);
// partial must have room for prereduce_room(colreduce_blocks(n)) * C * 5 floats
hipError_t launch_colreduce_final(hipStream_t s, int C, int D, int64_t n, float* partial, float* gW0, float* gb0,
                                  float wscale = 1.f);
hipError_t launch_colreduce_final_blocks(hipStream_t s, int C, int D, int nblk, float* partial, float* gW0, float* gb0,
                                         float wscale = 1.f);
hipError_t launch_colreduce(hipStream_t s, const float* G, int ldg, int C, const float* x, int D,
                            int64_t n, float* partial, float* gW0, float* gb0, float wscale = 1.f);

// ---- 3M complex path: slab reduction
hipError_t launch_wgrad3m_reduce(hipStream_t s, const float* slab, const float* bslab, int S, int K, int Kin,
                                 int Kp_o, int Kp_i, float* gW, float* gb);

// ===========================================================================
// wire_layer_point.hip -- what only the per-layer API uses
// ===========================================================================
// ---- layout conversion for the per-layer API
hipError_t launch_c64_to_blocked(hipStream_t s, const float* src, int64_t n, int K, int P, float* dst);
hipError_t launch_blocked_to_c64(hipStream_t s, const float* src, int64_t n, int K, int P, float* dst);
// real [n][K] <-> padded [n][P]
hipError_t launch_pad_rows(hipStream_t s, const float* src, int64_t n, int K, int P, float* dst);
hipError_t launch_unpad_rows(hipStream_t s, const float* src, int64_t n, int K, int P, float* dst);

// ---- elementwise Gabor gradient for the per-layer API
hipError_t launch_gabor_bwd_point(hipStream_t s, const float* g, const float* lin, const float* out,
                                  int64_t n, int P, float omega, float scale, float* g_lin);
hipError_t launch_gabor_bwd_first_point(hipStream_t s, const float* g, const float* out,
                                        const float* coords, int D, const float* W0, const float* b0,
                                        int64_t n, int K, int P, float omega, float scale, float* g_u,
                                        int ldu);

// 2-D Gabor (wire2d) forms: linsy / g_linsy [n][2P] in (u | v | p | q) groups; first layer g_up [n][2 ldu]
hipError_t launch_gabor2d_bwd_point(hipStream_t s, const float* g, const float* linsy, const float* out,
                                    int64_t n, int P, float omega, float scale, float* g_linsy);
hipError_t launch_gabor2d_bwd_first_point(hipStream_t s, const float* g, const float* out, const float* coords,
                                          int D, const float* W0, const float* b0, const float* V0,
                                          const float* c0, int64_t n, int K, int P, float omega, float scale,
                                          float* g_up, int ldu);

hipError_t launch_real_act_bwd_point(hipStream_t s, int kind, const float* g, const float* lin,
                                     const float* out, int64_t n, int P, float omega, float scale,
                                     float* g_lin);

// ---- trainable omega_0 / scale_0 (ComplexGaborLayer(trainable=True), modules/wire.py:80-81):
// out2 = { dL/d omega_0, dL/d scale_0 }; partial: 2 * hparam_blocks(n) floats
int hparam_blocks(int64_t n);
hipError_t launch_gabor_hparam_grad(hipStream_t s, const float* g, const float* lin, const float* out, int64_t n,
                                    int K, int P, int is_first, float scale, float* partial, float* out2);
hipError_t launch_gabor2d_hparam_grad(hipStream_t s, const float* g, const float* linsy, const float* out, int64_t n,
                                      int K, int P, int is_first, float scale, float* partial, float* out2);

// ===========================================================================
// wire_train.hip -- the glue of a training run (wire_ssim.hip and wire_tv.hip: a metric and a regulariser with kernel
// files of their own)
// ===========================================================================
// ---- training glue
// idx_out[r] = pi_seed(first + r), r < count: a keyed bijection pi_seed of [0, n_total) (the epoch's shuffle)
hipError_t launch_perm_indices(hipStream_t s, uint64_t seed, int64_t n_total, int64_t first, int64_t count,
                               int64_t* idx_out);
hipError_t launch_coords(hipStream_t s, const int64_t* idx, int64_t first, int64_t n,
                         const float* tx, int W, const float* ty, int H, const float* tz, int T,
                         float* coords);
// the grid of a loss kernel over n elements (at most 1024 blocks of 256); loss_out[0] = lscale * sum of nb partial sums
unsigned mse_blocks(long long n);
hipError_t launch_mse_final(hipStream_t s, const float* partial, int nb, float lscale, float* loss_out);
hipError_t launch_mse_grad(hipStream_t s, const float* y, const float* target, const int64_t* idx,
                           int64_t first, int64_t n, int O, float weight, float* g_y,
                           float* loss_out, float* rec, float* partial);
// pointwise data terms with a per-sample weight (wire_loss.hip): kind = WIRE_LOSS_*, weight null (ones), [*] or [*][O];
// rows, rec and partial as launch_mse_grad, whose bits plain MSE without weights gives
hipError_t launch_point_loss_grad(hipStream_t s, int kind, float delta, const float* y, const float* target,
                                  const float* weight, int weight_per_elem, const int64_t* idx, int64_t first,
                                  int64_t n, int O, float shard, float* g_y, float* loss_out, float* rec,
                                  float* partial);
// super-resolution loss: AvgPool2d(scale) of the [H W][O] reconstruction against gt_lr [H2 W2][O]
// (wire_SISR.py:151-161): loss, dL/dy (g_y [H W][O]), optionally the pooled image; partial >= 1024 floats
hipError_t launch_avgpool_mse_grad(hipStream_t s, const float* y, int H, int W, int O, int scale,
                                   const float* gt_lr, float* g_y, float* rec_lr, float* loss_out,
                                   float* partial);
// multi-image super-resolution loss (wire_multi_sr.py:190-208): y, g_y [B][H W][O], gt_lr / mask (null: ones) / rec_lr
// (optional) [B][H2 W2][O]; loss = mean((rec m - gt m)^2) over all B H2 W2 O elements; every element of g_y is written;
// partial >= 1024 floats
hipError_t launch_avgpool_mse_grad_frames(hipStream_t s, const float* y, int B, int H, int W, int O, int scale,
                                          const float* gt_lr, const float* mask, float* g_y, float* rec_lr,
                                          float* loss_out, float* partial);
// video compressive sensing loss (modules/lin_inverse.py:42-95): y, g_y [n_pix T][O], the rows of pixels p0 .. p0 + n_pix
// of NP; mask [NP][T], gt / est (optional) [C'][NP][O], C' = ceil(T / nframes) + dup_last; loss_out = this slab's
// sum d^2 / (C' NP O); every element of g_y is written; partial >= 1024 floats
hipError_t launch_coded_mse_grad(hipStream_t s, const float* y, int64_t p0, int64_t n_pix, int64_t NP, int T, int O,
                                 int nframes, int dup_last, const float* mask, const float* gt, float* g_y, float* est,
                                 float* loss_out, float* partial);
// the same operator and its adjoint on frame-major tensors: video / masks / g_video [T][NP], coded / g_coded [C'][NP]
hipError_t launch_coded_fwd(hipStream_t s, const float* video, const float* masks, int T, int64_t NP, int nframes,
                            int dup_last, float* coded);
hipError_t launch_coded_bwd(hipStream_t s, const float* g_coded, const float* masks, int T, int64_t NP, int nframes,
                            int dup_last, float* g_video);
// coords [B][H W][2] = the grid moved by frame f's 2 x 3 matrix mats[f] (device, fp64), normalised as 2 X / W - 1
// (modules/motion.py:284-318 at scale = 1)
hipError_t launch_affine_coords(hipStream_t s, const double* mats, int B, int H, int W, float* coords);
hipError_t launch_adam(hipStream_t s, float* p, const float* g, float* m, float* v, int64_t count,
                       float step_size, float beta1, float beta2, float eps, float inv_sqrt_bc2);

// ---- evaluation metrics: mode 0 -> {sum sq err, max gt}; mode 1 -> {intersection, union}
hipError_t launch_metric(hipStream_t s, int mode, const float* rec, const float* gt, int64_t count, float thres,
                         float* out, float* partial);
// ---- structural similarity (wire_ssim.hip): x, y [H][W][O] channel last, a separable window of `taps` (odd, 3 ..
// SSIM_MAX_TAPS) floats over the valid region; out1[0] = the mean of the index, map (optional) [H-taps+1][W-taps+1][O];
// partial: ssim_tiles(H, W, taps) floats
#define SSIM_MAX_TAPS 11
struct SsimWin { float w[SSIM_MAX_TAPS]; };
int64_t ssim_tiles(int H, int W, int taps);
hipError_t launch_ssim(hipStream_t s, const float* x, const float* y, int H, int W, int O, int taps, const SsimWin& win,
                       float cov, float c1, float c2, float* out1, float* map, float* partial);
// ---- its gradient and the SSIM-regularised loss (wire_ssim_bwd.hip): g_y [H][W][O] = g_ssim[0] (a device scalar) times
// d mean(S) / dy; and loss = mse + lambda (1 - ssim(target, y)) of a full-grid [H W][O] reconstruction, fused with its
// backward (the MSE over rows idx[0 .. n_mse), or first .. first + n_mse when idx is null; loss_out[0..2] = loss, mse,
// ssim; lambda == 0 leaves the index out).  partial: ssim_loss_partials(H, W) floats
int64_t ssim_bwd_tiles(int H, int W);
int64_t ssim_loss_partials(int H, int W);
hipError_t launch_ssim_bwd(hipStream_t s, const float* x, const float* y, int H, int W, int O, int taps,
                           const SsimWin& win, float cov, float c1, float c2, const float* g_ssim, float* g_y);
hipError_t launch_ssim_mse_grad(hipStream_t s, const float* y, int H, int W, int O, const float* target, int taps,
                                const SsimWin& win, float cov, float c1, float c2, const int64_t* idx, int64_t first,
                                int64_t n_mse, float lambda, float* g_y, float* loss_out, float* rec, float* partial);

// ---- total variation (wire_tv.hip): tv(x) = sum |x[i+1][j] - x[i][j]| + sum |x[i][j+1] - x[i][j]| over `planes` images
// of H x W, element (p, i, j) at x[p plane_stride + (i W + j) pix_stride]; its gradient times the device scalar g_tv[0];
// and loss = mse + lambda_tv tv of a full-grid [H W][O] reconstruction, fused with its backward (the MSE over rows
// idx[0 .. n_mse), or first .. first + n_mse when idx is null; loss_out[0..2] = loss, mse, tv).
// partial: >= 1024 floats (launch_tv_fwd), >= 2048 floats (launch_tv_mse_grad)
bool tv_shape_ok(int planes, int H, int W, int64_t pix_stride, int64_t plane_stride);
hipError_t launch_tv_fwd(hipStream_t s, const float* x, int planes, int H, int W, int64_t pix_stride,
                         int64_t plane_stride, float* tv_out, float* partial);
hipError_t launch_tv_bwd(hipStream_t s, const float* x, int planes, int H, int W, int64_t pix_stride,
                         int64_t plane_stride, const float* g_tv, float* g_x);
hipError_t launch_tv_mse_grad(hipStream_t s, const float* y, int H, int W, int O, const float* target,
                              const int64_t* idx, int64_t first, int64_t n_mse, float lambda_tv, float* g_y,
                              float* loss_out, float* rec, float* partial);
// the TV term of an (H, W, T) grid of O channels ([H W T][O] rows, T = 1: an image), its spatial and temporal sums
// weighted apart, ADDED to the g_y an operator's backward has left; loss_out[0..3] = loss, data, tv_s, tv_t.
// partial: >= 2048 floats
hipError_t launch_tv_add_grad(hipStream_t s, const float* y, int H, int W, int T, int O, float lambda_s,
                              float lambda_t, const float* data_loss, float* g_y, float* loss_out, float* partial);

// ---- best-so-far tracking on the device and the sigmoid of the mesh-export query
hipError_t launch_track_best(hipStream_t s, const float* metric, float* best, int force, const float* src,
                             float* dst, int64_t count, int* updated);
hipError_t launch_sigmoid(hipStream_t s, float* x, int64_t count);

// ---- CT forward operator: rotate-and-sum Radon transform (modules/lin_inverse.py:19-40) and its adjoint
hipError_t launch_radon_fwd(hipStream_t s, const float* img, const float* angles, int H, int W, int A, float* sino);
hipError_t launch_radon_bwd(hipStream_t s, const float* g_sino, const float* angles, int H, int W, int A,
                            float* g_img);

// ===========================================================================
// wire_m2.hip, wire_hier.hip, wire_mfn.hip -- the point kernels of the newer net kinds
// ===========================================================================
// ---- the scale combiner of the multi-pass B-spline net (wire_m2.hip): t [S][n][O] (the trunk's outputs, pass-major)
// -> y [n][O] = W2 relu(W1 [t_0 | .. | t_{S-1}] + b1) + b2, W1 [128][S O], W2 [O][128]; S <= 8, O <= 8
#define M2_MAX_SCALES 8
#define M2_H 128                 // freq_mlp's hidden width
#define M2_COMB_MAXBLK 512
struct M2Comb { const float* W1; const float* b1; const float* W2; const float* b2; };
struct M2Grads { float* W1; float* b1; float* W2; float* b2; };
// the loss of a training step inside the backward: target [.][O] at rows idx[r] (null: first + r); y, g_y (optional),
// rec (optional) written; gscale = 2 weight / (n O)
struct M2Loss {
  const float* target = nullptr; const int64_t* idx = nullptr; int64_t first = 0; float gscale = 0.f;
  float* y = nullptr; float* g_y = nullptr; float* rec = nullptr;
};
__host__ __device__ inline int m2_comb_grad_floats(int S, int O) {   // |gW1| + |gb1| + |gW2| + |gb2|
  return M2_H * S * O + M2_H + O * M2_H + O;
}
int m2_comb_blocks(int64_t n);                   // blocks of the backward: part has room for this many x grad_floats
hipError_t launch_m2_comb_fwd(hipStream_t s, const M2Comb& w, int S, int O, const float* t, int64_t n, float* y);
// g_t [S][n][O] = dL/dt; part[block][grad_floats] (null: no weight gradient); ls.target: the MSE of y against it gives
// g_y (and loss_part[block]), else g_y is read
hipError_t launch_m2_comb_bwd(hipStream_t s, const M2Comb& w, int S, int O, const float* t, int64_t n, const M2Loss& ls,
                              const float* g_y, float* g_t, float* part, float* loss_part);
hipError_t launch_m2_comb_reduce(hipStream_t s, const float* part, int64_t n, int S, int O, const M2Grads& g);
// out [n][D] = sum_k g[k][n][D]
hipError_t launch_m2_sum_passes(hipStream_t s, const float* g, int S, int64_t n, int D, float* out);

// ---- the hierarchical B-spline net (wire_hier.hip): stages coupled by a 2K -> K join, one head per stage
// first layer of a stage: lin (optional) [n][P], out rows of ldo floats (the left half of the join's [n][2P] input, or
// [n][P]); pad features 0; amax_out: max |out| slots or null
hipError_t launch_hier_first_fwd(hipStream_t s, const float* coords, int64_t n, int D, const float* W0, const float* b0,
                                 int K, int P, float c, float* lin, float* out, int ldo, unsigned* amax_out);
// y [n][O] = (acc ? y : 0) + (x Wh^T + bh), x rows of ldx floats (P of them read; pad features 0), Wh native [O][K];
// ls.target: y is complete -- its MSE terms, g_y, rec and loss_part[hier_head_blocks(n)]; O P floats of LDS (<= 64 KB)
#define HIER_HEAD_MAXBLK 1024
int hier_head_blocks(int64_t n);
hipError_t launch_hier_head_fwd(hipStream_t s, const float* x, int ldx, const float* Wh, const float* bh, int64_t n, int K,
                                int P, int O, int acc, float* y, const M2Loss& ls, float* loss_part);
// part_w / part_b (optional, launch_final_bwd's layout and room): partials of gWh = g_y^T x, gbh;  g_lin (optional)
// [n][P] = (g_y Wh) c B'(c lin) + add (add optional, [n][P]), amax_g its max-|value| slots or null
hipError_t launch_hier_head_bwd(hipStream_t s, const float* g_y, int64_t n, int O, const float* Wh, const float* x, int ldx,
                                const float* lin, const float* add, int K, int P, float c, float* g_lin, float* part_w,
                                float* part_b, unsigned* amax_g);
// W [K][2K], b [K] -> fwd [P][2P] (halves at columns 0 and P), bias [P], Wa / Wb [K][K] (the halves, contiguous)
hipError_t launch_hier_pack_join(hipStream_t s, const float* W, const float* b, int K, int P, float* fwd, float* bias,
                                 float* Wa, float* Wb);
// slab [S][P][2P], bslab [S][P] -> gW [K][2K], gb [K]
hipError_t launch_hier_join_reduce(hipStream_t s, const float* slab, const float* bslab, int S, int K, int P, float* gW,
                                   float* gb);

// ---- the multiplicative filter network (wire_mfn.hip): g(x)_j = exp(-gamma_j / 2 |x - mu_j|^2) sin(x . w_j + c_j)
// tab: a filter's table [P][MFN_TAB] in the packed image (wire_dev.h), written by launch_mfn_pack_table from the native
// mu [K][D], gamma [K], w [K][D], c [K]
hipError_t launch_mfn_pack_table(hipStream_t s, const float* mu, const float* gamma, const float* w, const float* c, int K,
                                 int D, int P, float* tab);
// out [n][P] = g(x) (pad columns 0), or mul g with mul [n][P]; amax_out: max |out| slots or null
hipError_t launch_mfn_filter_fwd(hipStream_t s, const float* tab, const float* coords, int64_t n, int D, int K, int P,
                                 const float* mul, float* out, unsigned* amax_out);
hipError_t launch_mfn_filter_fwd_native(hipStream_t s, const float* mu, const float* gamma, const float* w, const float* c,
                                        const float* coords, int64_t n, int D, int K, float* out);
// g_z = g_y wf; part_w / part_b (optional): launch_final_bwd's partials of g_y^T z, sum g_y; lin != null: g_lin = g_z g(x)
// (tab; its maximum into amax_g) and hbuf = g_z lin, else hbuf = g_z; every row of P floats
hipError_t launch_mfn_final_bwd(hipStream_t s, const float* g_y, int64_t n, int O, const float* wf, const float* z,
                                const float* lin, const float* tab, const float* coords, int D, int P, float* g_lin,
                                float* hbuf, float* part_w, float* part_b, unsigned* amax_g);
// a filter's parameter gradients from its upstream gradient hbuf [n][ldh]; part: mfn_sums_blocks(n) * 10 * K floats
int mfn_sums_blocks(int64_t n);
hipError_t launch_mfn_filter_sums(hipStream_t s, const float* tab, const float* coords, int64_t n, int D, int K,
                                  const float* hbuf, int ldh, float* part, float* g_mu, float* g_gamma, float* g_w,
                                  float* g_c);
hipError_t launch_mfn_filter_sums_native(hipStream_t s, const float* mu, const float* gamma, const float* w, const float* c,
                                         const float* coords, int64_t n, int D, int K, const float* hbuf, float* part,
                                         float* g_mu, float* g_gamma, float* g_w, float* g_c);
// a filter's share of the coordinate gradient, g_x [n][D] (acc != 0: added to what is there); fixed summation order
hipError_t launch_mfn_filter_gx(hipStream_t s, const float* tab, const float* coords, int64_t n, int D, int K,
                                const float* hbuf, int ldh, int acc, float* g_x);
hipError_t launch_mfn_filter_gx_native(hipStream_t s, const float* mu, const float* gamma, const float* w, const float* c,
                                       const float* coords, int64_t n, int D, int K, const float* hbuf, float* g_x);
