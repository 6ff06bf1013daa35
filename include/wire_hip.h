/* wire_hip.h -- C ABI of libwire_hip.so: the MI355X (gfx950) WIRE INR hot path.
 *
 * The reference (Annatk26/wire @ 2024_08_07) has no native layer and no FFI:
 * its hot path is eager PyTorch.  Each entry point
 * below names the reference code whose arithmetic it replaces; the binding a
 * maintainer adds on the reference side is a ctypes stub.
 *
 * Conventions
 *  - plain pointers and sizes only; every pointer is a DEVICE pointer unless
 *    the name ends in _host; `stream` is a hipStream_t passed as void*.
 *  - every function returns 0 on success or a negative wire_status; it never
 *    throws and never synchronises the device.  wire_last_error() returns the
 *    message of the calling thread's most recent failure.
 *  - the library owns no device memory: parameters, packed weights,
 *    activations and scratch live in caller buffers sized by the *_floats /
 *    *_bytes queries.  Re-entrant; callable from any host thread (autograd
 *    runs backward on its own thread).
 *  - "params" / "grads" are arrays (in HOST memory) of device pointers, one
 *    per trainable tensor in the reference's state_dict order and native
 *    layout (complex64 = interleaved re,im floats):
 *       wire   : W0[K][D] f32, b0[K] f32, {W_l[K][K] c64, b_l[K] c64} l=1..L,
 *                W_f[O][K] c64, b_f[O] c64        (modules/wire.py:127-157)
 *       wire2d : per layer l=0..L: W, b, V(scale_orth), c; then W_f, b_f
 *                                                  (modules/wire2d.py:98-123)
 *       siren/gauss/relu/bspline : {W_l, b_l} l=0..L, W_f, b_f, all f32
 *                (modules/siren.py:64-88, gauss.py:44-67, relu.py:99-120,
 *                 bspline_form.py:73-110; its scale_0 buffers are not
 *                 trainable and travel in wire_net_desc.scale0)
 *       bspline_cubic : the same list (modules/bspline_cubic.py:86-117; each
 *                layer's scale_0, not trainable, travels in scale0)
 *       bspline_ms : W0[SHF][D], b0[SHF] (the frozen first stage), W1[K][SHF],
 *                b1[K], {W_l[K][K], b_l[K]} l=2..max(L,1), W_f, b_f, all f32
 *                (modules/bspline_mscale_HL.py; its scales travel in
 *                 wire_net_desc_ms, see below)
 *       bspline_m2, bspline_hier : see wire_net_desc_ms below
 *       mfn    : per filter i = 0..L: mu_i[K][D], gamma_i[K], w_i[K][D], c_i[K]
 *                (gabon_filters.{i}.mu | .gamma | .linear.weight | .linear.bias);
 *                then {W_i[K][K], b_i[K]} i = 0..L-1 (linear.{i}); then W_f[O][K],
 *                b_f[O] (linear.{L}); all f32          (modules/mfn.py:29-54)
 *  - internal activation layout ("blocked planar"): a
 *    complex row of K features is stored as P = roundup(2K,64) floats; group
 *    g of 32 features occupies columns [64g,64g+32) = real parts and
 *    [64g+32,64g+64) = imaginary parts.  Pad features read as 0.
 *
 * Workspaces
 *  - `packed`, `act`, `scratch`, `partial` and every `ws` are the caller's; the library keeps nothing in them between
 *    calls except what this header says a later call reads: `packed` from wire_pack_params to the calls that take it,
 *    `act` from a forward (wire_mlp_fwd with save_for_bwd = 1, or the forward inside wire_train_fwd_bwd) to the
 *    backward that belongs to it.
 *  - no call reads a byte of `packed`, `act`, `scratch`, `partial` or `ws` that the same call -- for `act`, the forward
 *    it belongs to; for `packed`, wire_pack_params -- has not written.  The buffers need no initialisation, may be larger
 *    than the size queries ask for, and may hold anything before the call: the leftovers of a larger batch, of another
 *    net, of another GEMM family, NaN.  Results do not depend on their prior contents: where this header says that the
 *    same call gives the same bits, it gives them whatever the workspaces held (tests/test_gpu_workspace_fill.py).
 *  - the regions a call leaves unwritten (rows between n and the next multiple of 128, slabs of unused splits, partials
 *    beyond the blocks of this n) are unspecified afterwards; DESIGN.md section 3, "Padded regions", lists them.
 */
#ifndef WIRE_HIP_H
#define WIRE_HIP_H

#include <stddef.h>
#include <stdint.h>

#ifdef __cplusplus
extern "C" {
#endif

#define WIRE_ABI_VERSION 1

typedef enum wire_status {
  WIRE_OK = 0,
  WIRE_ERR_ARG = -1,     /* bad argument / unsupported shape            */
  WIRE_ERR_HIP = -2,     /* a HIP runtime call or launch failed          */
  WIRE_ERR_SIZE = -3     /* caller buffer too small                      */
} wire_status;

/* model_dict keys of modules/models.py:15-21 that are in scope */
typedef enum wire_kind {
  WIRE_KIND_WIRE = 0,    /* modules/wire.py   ComplexGaborLayer          */
  WIRE_KIND_WIRE2D = 1,  /* modules/wire2d.py ComplexGaborLayer2D        */
  WIRE_KIND_SIREN = 2,   /* modules/siren.py  SineLayer                  */
  WIRE_KIND_GAUSS = 3,   /* modules/gauss.py  GaussLayer                 */
  WIRE_KIND_RELU = 4,    /* modules/relu.py   ReLULayer (+PosEncoding)   */
  WIRE_KIND_BSPLINE = 5, /* modules/bspline_form.py Bsplines_form: the
                            quadratic B-spline of lin / scale0           */
  WIRE_KIND_BSPLINE_MS = 6, /* modules/bspline_mscale_HL.py: a frozen
                            Scaled_Bsplines_form D -> SHF, then Bsplines_form
                            SHF -> K; described by wire_net_desc_ms        */
  /* 7 and 10 stay unassigned: a plain descriptor of kind 7 or 10 is WIRE_ERR_ARG, and callers rely on that */
  WIRE_KIND_BSPLINE_M2 = 8, /* modules/bspline_mscale_2.py: the bspline_form
                            trunk run once per scale, the S outputs through
                            freq_mlp; described by wire_net_desc_ms        */
  WIRE_KIND_BSPLINE_HIER = 9, /* modules/bspline_mscale_hier.py: one stage per
                            scale, stage s > 0 joins its first layer with the
                            previous stage's output (2K -> K), one linear head
                            per stage; described by wire_net_desc_ms       */
  WIRE_KIND_MFN = 11,    /* modules/mfn.py: the multiplicative filter network
                            z_0 = g_0(x), z_{i+1} = (z_i W_i^T + b_i) g_{i+1}(x),
                            y = z_L W_f^T + b_f with hidden_layers + 1 Gabor
                            filters g_i of the COORDINATES; a plain wire_net_desc  */
  WIRE_KIND_BSPLINE_CUBIC = 12 /* modules/bspline_cubic.py Bsplines_cubic: the
                            cubic B-spline of lin = scale0 (x W^T) + b; a plain
                            wire_net_desc                                        */
} wire_kind;

/* Architecture + hyper-parameters of one INR (modules/wire.py:96-159). */
typedef struct wire_net_desc {
  int32_t kind;            /* wire_kind                                           */
  int32_t in_features;     /* D: coordinate dims, 1..4                            */
  int32_t width;           /* K: features per hidden layer AFTER the reference's
                              own rescale (int(h/sqrt2) wire, int(h/2) wire2d)   */
  int32_t hidden_layers;   /* L                                                   */
  int32_t out_features;    /* O, 1..8, and O x P <= 16384 with P the padded row
                              width (roundup(2K, 64) wire / wire2d, roundup(K, 64)
                              otherwise): the final linear's forward keeps W_f
                              [O][P] in the 64 KB of LDS a launch gets.  A wider
                              net is WIRE_ERR_ARG from every call that takes the
                              descriptor, the size queries included            */
  int32_t posenc_freqs;    /* relu only: PosEncoding.num_frequencies, 0 = off     */
  float first_omega0;      /* omega of net[0] (bspline: carried, unused)          */
  float hidden_omega0;     /* omega of net[1..L] (bspline: carried, unused)       */
  float scale0;            /* Gaussian scale s0; bspline: the divisor sigma0
                              (zero or not finite -> WIRE_ERR_ARG); bspline_cubic:
                              the multiplier s of every activation layer's INPUT,
                              lin = s (x W^T) + b -- the bias is not scaled and
                              the sign of s matters.  wire_pack_params folds it
                              into the packed weights (s W in every image, so the
                              data and coordinate gradients carry it), the
                              weight gradients come out as dL/dW = s g_lin^T x,
                              params / grads hold the unscaled W; both omegas are
                              carried and unused; zero or not finite ->
                              WIRE_ERR_ARG                                        */
} wire_net_desc;

/* The multiplicative filter network (WIRE_KIND_MFN, modules/mfn.py) is described by a plain wire_net_desc:
 *   width = K (hidden_features), hidden_layers = L >= 0 (L + 1 filters, L linears K -> K, the final linear K -> O),
 *   in_features = D <= 4, out_features = O <= 8; first_omega0, hidden_omega0, scale0 and posenc_freqs are carried and
 *   ignored (a zero scale0 is accepted).  g_i(x)_j = exp(-gamma_ij / 2 |x - mu_ij|^2) sin(x . w_ij + c_ij): every filter
 *   reads the coordinates, so every filter contributes to g_coords.  The net runs layer by layer in every mode: the
 *   knobs fused_fwd, fused_train, fused_bwd, fused_rstore and split_out leave its results unchanged.  Its backward is
 *   deterministic (the filters' column sums are per-block partials added in a fixed order).
 *   wire_act_out_offset(layer l) = the stored z_l.  The hooked call announces the final linear {W_f, b_f} first; then, for
 *   i = L-1 .. 0, the pair {W_i, b_i} followed by the four tensors of filter i + 1; filter 0 last.  Every tensor
 *   exactly once.                                                                                                     */
/* The multi-scale B-spline net (WIRE_KIND_BSPLINE_MS, modules/bspline_mscale_HL.py): a wire_net_desc followed by the
 * shape of its frozen first stage.  Callers pass &desc.base wherever a const wire_net_desc* is taken; the library reads
 * the tail only when base.kind is WIRE_KIND_BSPLINE_MS.
 *   base.width = K (hidden_features), base.hidden_layers = the reference's value (0 builds the net of 1: one SHF -> K
 *   layer, then max(L - 1, 0) K -> K layers), base.scale0 = the hidden divisor `scale`, base.posenc_freqs = 0.
 *   First stage: lin = x W0^T + b0, column j divided by scales[g(j)]: g = 0 for j < min(256, SHF), else
 *   g = 1 + (j - 256) / split with split = (SHF - 256) / (nscales - 1), which must divide SHF - 256 exactly; then B.
 *   Every scale must be finite and non-zero (the plan uses c = 1 / |s|).  No gradient reaches W0, b0 or the
 *   coordinates: the backward never writes grads[0] / grads[1] (NULL accepted there; the hooked call still announces
 *   them, holding whatever the caller put there), and a g_coords request is WIRE_ERR_ARG.                          */
/* The multi-pass B-spline net (WIRE_KIND_BSPLINE_M2, modules/bspline_mscale_2.py) uses the same struct:
 *   base.width = K, base.hidden_layers = L (trunk: D -> K, L x K -> K, then K -> O linear -- kind 5's), base.scale0 is
 *   carried and ignored (the reference's `scale`: 0 is accepted), first_width = 0, nscales = S (1..8), scales[] = the
 *   divisor of each pass: pass k computes the trunk with c_k = 1 / |scales[k]| (each finite and non-zero).
 *   The S outputs of a row, [t_0 | t_1 | ..], go through freq_mlp = Linear(S O -> 128), ReLU, Linear(128 -> O).
 *   params[] / grads[]: freq_mlp.0.weight [128][S O], freq_mlp.0.bias [128], freq_mlp.2.weight [O][128],
 *   freq_mlp.2.bias [O], then the trunk in kind 5's order (its tensors start at index 4).  combine_scales.scale_weights
 *   and combine_scales.refine.* receive no gradient in the reference's loop and are not ABI tensors.  The hooked call
 *   announces tensors 0 .. 3 first.  n is the number of coordinate rows; the library runs the trunk on S n rows.       */
/* The hierarchical B-spline net (WIRE_KIND_BSPLINE_HIER, modules/bspline_mscale_hier.py) uses the same struct:
 *   base.width = K, base.hidden_layers = L (>= 1; L = 1 only with one scale), base.scale0 carried and ignored,
 *   first_width = 0, nscales = S (1..8), scales[s] = the divisor of every layer of stage s (finite, non-zero).
 *   Stage 0: Bsplines_form D -> K, then L x K -> K, on the coordinates.  Stage s > 0: x_in = layer 0 (D -> K) of the
 *   coordinates, layer 1 (2K -> K) of [x_in | x_{s-1}], layer 2 (K -> K); layers 3.. of such a stage exist in the
 *   reference's state_dict, are never run and are not ABI tensors.  y = sum_s (x_s Wh_s^T + bh_s).
 *   params[] / grads[]: stage 0's {W, b} x (L + 1), then per stage s > 0 its three {W, b} (layer 1's W [K][2K], the
 *   x_in columns first), then the S heads {Wh_s [O][K], bh_s [O]} as one block at the end.  Every stage's first layer
 *   contributes to g_coords.  The hooked call announces the heads first, then the stages from the last to the first,
 *   each from its last layer to its first.  out_features x roundup(K, 64) <= 16384 (a head's weights in 64 KB).      */
#define WIRE_MS_MAX_SCALES 8
typedef struct wire_net_desc_ms {
  wire_net_desc base;      /* base.kind = WIRE_KIND_BSPLINE_MS                    */
  int32_t first_width;     /* SHF: scaled_hidden_features, 1..4096 (kinds 8, 9: 0) */
  int32_t nscales;         /* T: entries of scale_tensor, 2..WIRE_MS_MAX_SCALES
                              (kinds 8, 9: S, 1..WIRE_MS_MAX_SCALES)             */
  float scales[WIRE_MS_MAX_SCALES];   /* scale_tensor[0 .. T)                     */
} wire_net_desc_ms;

int wire_abi_version(void);
const char* wire_last_error(void);

/* ---- sizes ------------------------------------------------------------ */
/* number of trainable tensors (length of the params / grads arrays)       */
int wire_num_param_tensors(const wire_net_desc* d);
/* floats in tensor t in its native layout (complex counts 2 per element)  */
int64_t wire_param_tensor_floats(const wire_net_desc* d, int t);
/* floats of the packed (padded, real-expanded) weight image               */
int64_t wire_packed_floats(const wire_net_desc* d);
/* bytes of activation storage mlp_fwd writes for `n` rows (save_for_bwd=1
 * keeps what mlp_bwd needs; 0 = inference ping-pong only)                  */
int64_t wire_act_bytes(const wire_net_desc* d, int64_t n, int save_for_bwd);
/* bytes of scratch mlp_bwd needs for `n` rows                              */
int64_t wire_bwd_scratch_bytes(const wire_net_desc* d, int64_t n);

/* ---- whole-network path ------------------------------------------------ */
/* Refresh the packed weight image from the native parameters.  Call after
 * every optimizer step (replaces nothing in the reference: ATen reads the
 * nn.Parameter storage directly, modules/wire.py:89).                      */
int wire_pack_params(void* stream, const wire_net_desc* d,
                     const void* const* params_host, float* packed);

/* INR.forward (modules/wire.py:161-167; wire2d.py:122-127; siren.py:90-96;
 * gauss.py:71-74; relu.py:124-130; bspline_form.py:112-114): coords[n][D] f32 -> y[n][O] f32.
 * `act` receives the per-layer activations (wire_act_bytes).               */
int wire_mlp_fwd(void* stream, const wire_net_desc* d, const float* packed,
                 const float* coords, int64_t n, float* y,
                 void* act, int64_t act_bytes, int save_for_bwd);

/* Backward of the above (autograd graph of modules/wire.py:89-93,156-165):
 * g_y[n][O] = dL/dy.  Writes every parameter gradient in native layout
 * (PyTorch complex convention dL/dRe + j dL/dIm) through `grads_host`;
 * grads are OVERWRITTEN (= zero_grad + backward).                          */
int wire_mlp_bwd(void* stream, const wire_net_desc* d, const float* packed,
                 const float* coords, int64_t n, const float* g_y,
                 const void* act, int64_t act_bytes,
                 void* scratch, int64_t scratch_bytes,
                 void* const* grads_host);

/* One training step's compute in a single call (wire_image_denoise.py:148-156:
 * model(b_coords) -> rec[b_indices] = pix -> mse -> backward): forward, MSE against
 * target[idx[r]] (or target[first + r] when idx is NULL), loss_out[0] = weight *
 * mean((y - t)^2), optional rec scatter, and every parameter gradient of
 * weight * loss into grads_host (overwritten).  For every net kind with at least one
 * hidden layer and O <= 4 the final linear forward, the loss, its gradient, the final
 * linear backward and the last layer's activation gradient are ONE kernel (a single pass
 * over out_L / lin_L, final_fused_kernel); nets without a hidden layer or with O > 4 run
 * wire_mlp_fwd + wire_mse_grad + wire_mlp_bwd internally.
 * y [n][O] is an output; g_y [n][O] is caller scratch that receives dL/dy on the
 * unfused sequence and for the kinds whose loss is not in final_fused_kernel
 * (bspline_m2, bspline_hier, mfn) -- the fused final stage keeps dL/dy in registers
 * and leaves g_y untouched; partial >= 4096 floats.                              */
int wire_train_fwd_bwd(void* stream, const wire_net_desc* d, const float* packed,
                       const float* coords, int64_t n, const float* target,
                       const int64_t* idx, int64_t first, float weight, float* y,
                       float* g_y, float* loss_out, float* rec, float* partial,
                       void* act, int64_t act_bytes, void* scratch,
                       int64_t scratch_bytes, void* const* grads_host);

/* The same step for data-parallel callers that overlap the gradient exchange with the rest of the backward
 * (wire_occupancy.py:137-158 sharded over the GPUs of a node).  `ready(user, first_tensor, n_tensors)` is called ON THE
 * HOST, from inside this call, each time the kernels that produce the FINAL value of the parameter gradients
 * grads_host[first_tensor .. first_tensor + n_tensors) (state_dict order) have been enqueued on `stream` -- the final
 * linear layer first (loss_out is complete by then too), then the hidden layers from the last to the first, the first layer
 * last; every tensor is announced exactly once.  The callee typically records an event on `stream` and starts the
 * all-reduce of that slice on another stream; it must not wait for the device.  ready == NULL: wire_train_fwd_bwd.     */
typedef void (*wire_grad_ready_fn)(void* user, int first_tensor, int n_tensors);
int wire_train_fwd_bwd_hooked(void* stream, const wire_net_desc* d, const float* packed,
                              const float* coords, int64_t n, const float* target,
                              const int64_t* idx, int64_t first, float weight, float* y,
                              float* g_y, float* loss_out, float* rec, float* partial,
                              void* act, int64_t act_bytes, void* scratch,
                              int64_t scratch_bytes, void* const* grads_host,
                              wire_grad_ready_fn ready, void* user);

/* ---- coordinate gradients (first order, fp32) ---------------------------
 * wire_mlp_bwd_coords: wire_mlp_bwd that can also write g_coords [n][D] = dL/dcoords (f32).
 *   grads_host NULL: data gradients only (no weight-gradient GEMM, no reduction of the parameter gradients);
 *   g_coords NULL: exactly what wire_mlp_bwd produces; both NULL is an argument error.
 *   scratch: wire_bwd_coords_scratch_bytes(d, n) when g_coords is given (>= wire_bwd_scratch_bytes).
 *   The result is deterministic: every sum runs in a fixed order.
 * wire_posenc_bwd: backward of wire_posenc_fwd, g_pe [n][D + 2 D F] -> g_coords [n][D].  n < 0, D outside 1..4, F outside
 *   0..30, or (n > 0) a NULL pointer: WIRE_ERR_ARG before any HIP call; n == 0 returns WIRE_OK and touches nothing.  */
int64_t wire_bwd_coords_scratch_bytes(const wire_net_desc* d, int64_t n);
int wire_mlp_bwd_coords(void* stream, const wire_net_desc* d, const float* packed, const float* coords, int64_t n,
                        const float* g_y, const void* act, int64_t act_bytes, void* scratch, int64_t scratch_bytes,
                        void* const* grads_host, float* g_coords);
int wire_posenc_bwd(void* stream, const float* coords, int64_t n, int D, int F, const float* g_pe, float* g_coords);

/* ---- per-layer path (ComplexGaborLayer.forward, modules/wire.py:88-93) -- */
/* x: [n][in] f32 when is_first else [n][in] c64; W: [out][in] f32/c64;
 * act_out [n][out] c64 (interleaved); lin_out (optional, may be NULL) receives the pre-activation
 * `lin` of modules/wire.py:89 in the dtype of W's product: f32 [n][out] if is_first else c64.
 * The GEMM runs on the family the tuning knobs select -- the same kernels as wire_mlp_fwd.
 * ws: scratch of wire_layer_ws_bytes(n, in, out).                          */
int64_t wire_layer_ws_bytes(int64_t n, int in_features, int out_features);
int wire_gabor_fwd(void* stream, const void* x, const void* W, const void* b,
                   float omega0, float scale0, int64_t n, int in_features,
                   int out_features, int is_first, void* lin_out,
                   void* act_out, void* ws, int64_t ws_bytes);
/* backward: g_act [n][out] c64 -> g_x (NULL when is_first), g_W, g_b.      */
int wire_gabor_bwd(void* stream, const void* g_act, const void* x,
                   const void* W, const void* b, float omega0, float scale0,
                   int64_t n, int in_features, int out_features, int is_first,
                   void* g_x, void* g_W, void* g_b, void* ws, int64_t ws_bytes);
/* gradient of a TRAINABLE omega_0 / scale_0 (ComplexGaborLayer(..., trainable=True), modules/wire.py:80-81):
 * out2 (device, 2 floats) = { dL/d omega_0, dL/d scale_0 } for the upstream gradient g_act; same operands and
 * workspace as wire_gabor_bwd.  Rows are summed in blocks of 32, the blocks' sums by one block, in a fixed order: the
 * same call gives the same bits.  n, in_features or out_features < 1 or a NULL pointer: WIRE_ERR_ARG before any HIP
 * call; ws_bytes < wire_layer_ws_bytes(n, in, out): WIRE_ERR_SIZE; is_first with in_features > 4: WIRE_ERR_ARG.     */
int wire_gabor_hparam_grad(void* stream, const void* g_act, const void* x, const void* W, const void* b,
                           float omega0, float scale0, int64_t n, int in_features, int out_features,
                           int is_first, float* out2, void* ws, int64_t ws_bytes);
/* final nn.Linear(K,O,cfloat) + .real (modules/wire.py:156-157,164-165);
 * wire_final_fwd: out_features x roundup(2 in_features, 64) <= 16384, as for a
 * descriptor (WIRE_ERR_ARG before any HIP call otherwise)                   */
int wire_final_fwd(void* stream, const void* z, const void* Wf, const void* bf,
                   int64_t n, int in_features, int out_features, float* y,
                   void* ws, int64_t ws_bytes);
int wire_final_bwd(void* stream, const float* g_y, const void* z,
                   const void* Wf, int64_t n, int in_features,
                   int out_features, void* g_z, void* g_Wf, void* g_bf,
                   void* ws, int64_t ws_bytes);

/* SineLayer / GaussLayer / ReLULayer / Bsplines_form .forward (modules/siren.py:48-49,
 * gauss.py:27-28, relu.py:28-29, bspline_form.py:38-49) and their backward on native f32 tensors:
 * x [n][in], W [out][in], b [out] -> act [n][out].  kind = WIRE_KIND_SIREN /
 * _GAUSS / _RELU / _BSPLINE (scale0 = sigma0, the divisor; zero or not finite -> WIRE_ERR_ARG) /
 * _BSPLINE_CUBIC (modules/bspline_cubic.py:44-52; scale0 multiplies x: lin = scale0 (x W^T) + b, g_x and g_W carry it,
 * g_b does not; zero or not finite -> WIRE_ERR_ARG);
 * ws as for wire_gabor_fwd.                                                   */
int wire_real_layer_fwd(void* stream, int kind, const float* x, const float* W,
                        const float* b, float omega0, float scale0, int64_t n,
                        int in_features, int out_features, float* act_out,
                        void* ws, int64_t ws_bytes);
int wire_real_layer_bwd(void* stream, int kind, const float* g_act, const float* x,
                        const float* W, const float* b, float omega0, float scale0,
                        int64_t n, int in_features, int out_features, float* g_x,
                        float* g_W, float* g_b, void* ws, int64_t ws_bytes);

/* ---- training-step glue (wire_image_denoise.py:142-157,
 *      wire_occupancy.py:137-158) ---------------------------------------- */
/* coords[r] = grid point of flat index idx[r] (idx NULL -> first + r).
 * 2-D (tz NULL): idx = i*W + j -> (tx[j], ty[i])   (wire_image_denoise.py:63-66)
 * 3-D: idx = (i*W + j)*T + k -> (tx[j], ty[i], tz[k]) (modules/utils.py:171-176)
 * tx/ty/tz are the caller's linspace tables (device).  The indices are trusted.
 * n < 0, W or H < 1, T < 1 with tz given, or tx, ty or coords NULL: WIRE_ERR_ARG
 * before any HIP call; n == 0 returns WIRE_OK and touches nothing.           */
int wire_coords_from_index(void* stream, const int64_t* idx, int64_t first,
                           int64_t n, const float* tx, int W, const float* ty,
                           int H, const float* tz, int T, float* coords);
/* The per-epoch shuffle (torch.randperm(H*W) at wire_image_denoise.py:142, wire_occupancy.py:137) as a keyed
 * bijection pi_seed of [0, n_total) evaluated per position: idx_out[r] = pi_seed(first + r), r < count.  A rank
 * of a data-parallel job generates only the slice of the epoch's permutation it trains on (cost O(count),
 * independent of n_total and of the world size).  Integer arithmetic (a numpy twin in the
 * test suite reproduces it bit for bit); NOT the sequence torch.randperm draws.                                                  */
int wire_perm_indices(void* stream, uint64_t seed, int64_t n_total, int64_t first, int64_t count,
                      int64_t* idx_out);
/* loss = mean((y - target[idx])^2) over n*O elements scaled by `weight`
 * (= n/B for a shard of a global batch B; 1 for a whole batch);
 * g_y = weight * 2/(n*O) * (y - t).  loss_out[0] += is NOT used: it is
 * overwritten.  rec (optional): rec[idx[r]][:] = y[r][:]
 * (wire_image_denoise.py:150-153).  partial: scratch of >= 4096 floats.
 * Per-block sums in a grid that depends on n*O alone, added in a fixed order:
 * the same call gives the same bits.  n < 0, O < 1, or a NULL pointer other
 * than idx / rec: WIRE_ERR_ARG before any HIP call.  n == 0 returns WIRE_OK
 * and touches nothing, loss_out included.  The rows of idx are trusted.      */
int wire_mse_grad(void* stream, const float* y, const float* target,
                  const int64_t* idx, int64_t first, int64_t n, int O,
                  float weight, float* g_y, float* loss_out, float* rec,
                  float* partial);
/* Pointwise data terms with a per-sample weight: what wire_mse_grad does for the square, for four functions rho of the
 * residual.  Row r < n of y [n][O] pairs with table row src = idx ? idx[r] : first + r, exactly as in wire_mse_grad:
 * target is [*][O] and weight is NULL (all ones), [*] (weight_per_elem == 0, one per row) or [*][O]
 * (weight_per_elem == 1: a Bayer mosaic masks channels, not pixels), all read at src.  Weights may hold any finite
 * value, not only 0 and 1.  With d = y - t:
 *   loss_out[0] = shard * sum_e w_e rho(d_e) / (n O)            (overwritten)
 *   g_y[e]      = shard * w_e rho'(d_e) / (n O)                 (EVERY element is written)
 * The mean runs over every element, those of weight 0 included: MSELoss()(out * mask, gt * mask) with w = mask^2, the
 * convention of wire_avgpool_mse_grad_frames; a caller who wants the mean over the kept elements scales the weights.
 * shard is wire_mse_grad's `weight`: n/B for a shard of a global batch of B rows, 1 for a whole batch.
 *   WIRE_LOSS_MSE       rho = d^2                                           rho' = 2 d
 *   WIRE_LOSS_L1        rho = |d|                                           rho' = (y > t) - (y < t): +0 at a tie,
 *                                                                           as torch.nn.L1Loss
 *   WIRE_LOSS_HUBER     rho = d^2 / 2 if |d| <= delta,                      rho' = clamp(d, -delta, delta)
 *                             delta (|d| - delta / 2) otherwise             (torch.nn.HuberLoss)
 *   WIRE_LOSS_LOGISTIC  rho = max(z, 0) - t z + log1p(exp(-|z|))            rho' = sigmoid(z) - t
 *                       z = y a logit, t in [0, 1]                          (torch.nn.BCEWithLogitsLoss)
 * delta is read by WIRE_LOSS_HUBER alone.  The logistic form takes no exponential of a positive argument and divides by
 * 1 + e with e in [0, 1]: finite for every finite z.
 * rec (optional): rec[src][:] = y[r][:]; rows the call does not name stay untouched.  partial: >= 4096 floats of
 * scratch.  One grid-stride pass of 256-thread blocks in a grid that depends on n*O alone, per-block sums added in a
 * fixed order, no atomics: the same call gives the same bits.  WIRE_LOSS_MSE with weight == NULL writes the bits of
 * wire_mse_grad(..., weight = shard, ...) into g_y, loss_out and rec.
 * An unknown kind, n < 0, O < 1, delta not finite or <= 0 with WIRE_LOSS_HUBER, shard not finite, weight_per_elem
 * outside {0, 1}, or a NULL pointer other than weight / idx / rec: WIRE_ERR_ARG before any HIP call.  n == 0 returns
 * WIRE_OK and touches nothing, loss_out included.  The rows of idx are trusted.                                   */
typedef enum wire_loss_kind {
  WIRE_LOSS_MSE = 0,
  WIRE_LOSS_L1 = 1,
  WIRE_LOSS_HUBER = 2,
  WIRE_LOSS_LOGISTIC = 3
} wire_loss_kind;
int wire_point_loss_grad(void* stream, int kind, float delta, const float* y, const float* target, const float* weight,
                         int weight_per_elem, const int64_t* idx, int64_t first, int64_t n, int O, float shard,
                         float* g_y, float* loss_out, float* rec, float* partial);
/* Super-resolution loss of wire_SISR.py:151-161: rec = torch.nn.AvgPool2d(scale) of the full-grid
 * reconstruction y [H*W][O] (row n = i*W + j), loss = mean((gt_lr - rec)^2) over [H/scale][W/scale][O]
 * (floor: ragged borders are dropped and receive zero gradient).  Writes loss_out[0], g_y = dL/dy [H*W][O]
 * and, if rec_lr != NULL, the pooled image.  partial: >= 1024 floats of scratch.  EVERY element of g_y is written (the
 * ragged borders with +0.0).  H, W, O or scale < 1, scale > min(H, W), or a NULL pointer other than rec_lr: WIRE_ERR_ARG
 * before any HIP call.  No atomics: the same call gives the same bits.                                  */
int wire_avgpool_mse_grad(void* stream, const float* y, int H, int W, int O, int scale,
                          const float* gt_lr, float* g_y, float* rec_lr, float* loss_out,
                          float* partial);

/* Multi-image super-resolution loss of wire_multi_sr.py:190-208: B frames y [B][H*W][O] (row i*W + j inside a
 * frame), each pooled on its own by torch.nn.AvgPool2d(scale) to rec [B][H2*W2][O] (H2 = H/scale, W2 = W/scale,
 * floor), loss = MSELoss()(rec*mask, gt_lr*mask) = sum (rec m - gt m)^2 / (B H2 W2 O) -- the mean runs over every
 * element, masked ones included.  mask [B][H2*W2][O] may hold any values (dL/drec = 2 (rec m - gt m) m / count);
 * NULL = all ones.  Writes loss_out[0], EVERY element of g_y [B][H*W][O] (ragged borders exactly 0) and, if
 * rec_lr != NULL, the unmasked pooled frames.  No atomics: the same call gives the same bits.
 * partial: >= 1024 floats of scratch.  B, O or scale < 1, scale > min(H, W), or a NULL pointer other than mask /
 * rec_lr: WIRE_ERR_ARG before any HIP call.                                                             */
int wire_avgpool_mse_grad_frames(void* stream, const float* y, int B, int H, int W, int O, int scale,
                                 const float* gt_lr, const float* mask, float* g_y, float* rec_lr,
                                 float* loss_out, float* partial);
/* The frames' coordinates of that loop on the device -- motion.get_imstack's Xstack / Ystack at scale = 1
 * (modules/motion.py:284-318 as wire_multi_sr.py:74-78 calls it; ImageSRDataset stacks them, motion.py:66-69):
 * mats: DEVICE fp64 [B][2][3]; for frame f, row i, column j, in fp64
 *   Xn = m00 j + m01 i + m02,  Yn = m10 j + m11 i + m12,  coords[f][i*W + j] = (float(2 Xn / W - 1), float(2 Yn / H - 1)).
 * coords: [B][H*W][2].  B, H or W < 1 or a NULL pointer: WIRE_ERR_ARG before any HIP call.               */
int wire_affine_coords(void* stream, const double* mats, int B, int H, int W, float* coords);

/* A learnable registration of those frames: one 2 x 3 matrix theta[f] per frame, fp32, acting on the frame's NORMALISED
 * coordinates -- the convention of motion.get_transformed_coords / F.affine_grid (modules/motion.py), identity =
 * [[1,0,0],[0,1,0]], all six entries in one unit.  It composes with any base coordinates: those of wire_affine_coords,
 * a homography flow, a plain grid.  coords, out, g_out, g_in: [B][n_per][2]; theta, g_theta: [B][2][3]; all DEVICE,
 * the [..][2] arrays 8-byte aligned.
 * wire_warp_coords_fwd: for frame f and row p, (x, y) = coords[f][p], t = theta[f], in fp64, left to right, no
 *   contraction, rounded to fp32 once:
 *     out[f][p] = ( float(t00 x + t01 y + t02), float(t10 x + t11 y + t12) )
 *   The identity returns coords bit for bit.  out == coords (in place) is allowed; any other overlap is not.
 * wire_warp_coords_bwd: with v = (x, y, 1) of the INPUT coordinates,
 *     g_theta[f][a][c] = float( sum_p double(g_out[f][p][a]) * double(v_c) )        (each product exact in fp64)
 *   overwritten; pin_first = 1 writes +0.0 into the six entries of frame 0 instead (the gauge: the reference keeps its
 *   first frame unmoved), pin_first = 0 does not.  If g_in != NULL (it must not overlap another argument), in fp64,
 *   left to right:
 *     g_in[f][p] = ( float(t00 gx + t10 gy), float(t01 gx + t11 gy) ),   (gx, gy) = g_out[f][p]
 *   every element written once.  A workgroup of 256 threads adds 2048 consecutive rows of one frame in fp64 (a thread
 *   its rows in order, the wave by a fixed shuffle tree, the four waves in a fixed order) and stores six fp64 partials
 *   to ws; a second launch adds each frame's partials in a fixed order and rounds to fp32 once.  No atomics, every sum
 *   in an order that depends on (B, n_per) alone: the same call gives the same bits, whatever ws held before.
 *   ws: wire_warp_coords_bwd_ws_bytes(B, n_per) bytes of scratch, 8-byte aligned.
 * B or n_per < 1, sizes beyond 63 bits or more workgroups than a grid holds (2^31 - 1), pin_first not 0 / 1, a
 * misaligned pointer, or a NULL pointer other than g_in: WIRE_ERR_ARG before any HIP call (the size query too); a ws
 * that is too small: WIRE_ERR_SIZE.                                                                              */
int wire_warp_coords_fwd(void* stream, const float* coords, const float* theta, int B, int64_t n_per, float* out);
int64_t wire_warp_coords_bwd_ws_bytes(int B, int64_t n_per);
int wire_warp_coords_bwd(void* stream, const float* coords, const float* theta, const float* g_out, int B,
                         int64_t n_per, int pin_first, float* g_theta, float* g_in, void* ws, int64_t ws_bytes);

/* Registering those frames from their intensities (wire_register.hip): a bilinear resampler with its
 * coordinate gradient, and one Gauss-Newton iteration of a least-squares registration.  All pointers DEVICE.
 * wire_remap_bilinear_fwd: img [H][W][C] channel last, C = 1..8; xy [n][2] = (x, y), 8-byte aligned; out [n][C].
 *   normalized = 0: pixel coordinates, pixel centres at integers (cv2.remap); normalized = 1: F.grid_sample's
 *   align_corners = False, x_pix = ((x + 1) W - 1) / 2.  Taps outside the image contribute 0 (BORDER_CONSTANT 0,
 *   padding_mode = 'zeros'); a NaN or infinite coordinate gives 0.  In fp64 from the fp32 inputs, left to right, no
 *   contraction, rounded to fp32 once: x0 = floor(x), fx = x - x0, taps a b / c d,
 *     out = float( (1 - fy) ((1 - fx) a + fx b) + fy ((1 - fx) c + fx d) )
 * wire_remap_bilinear_bwd_xy: g_xy[p] = float( sum_c g_out[p][c] d out_c / d (x, y) ), c in order, the derivative of the
 *   interpolant on the cell chosen by floor (the right-hand derivative at integers):
 *     d/dx = (1 - fy) (b - a) + fy (d - c),   d/dy = ((1 - fx) c + fx d) - ((1 - fx) a + fx b)
 *   multiplied by W / 2, H / 2 for normalized = 1; 0 where the forward's coordinate is not finite or no tap is inside.
 *   g_xy [n][2], 8-byte aligned.  There is no adjoint with respect to img.  One thread per row, no atomics.
 * H, W or n < 1, C outside 1..8, normalized not 0 / 1, a NULL or misaligned pointer: WIRE_ERR_ARG before any HIP call.
 *
 * wire_register_gn_step: one iteration, for each frame b < B and each of its K start candidates, of
 *     minimise over M   E(M) = sum_(i,j) w(i,j) (R(M (j, i, 1)) - F_b(i, j))^2
 *   ref R [H][W]; frames F [B][H][W]; weight [B][H][W] or NULL (all ones); mats DEVICE fp64 [B][K][2][3] in pixel units,
 *   updated in place.  A pixel counts when u = M (j, i, 1) lies in [0, W - 1] x [0, H - 1], its weight is not 0 and
 *   F_b(i, j) is not 0 (an exact zero is the resampler's border fill).  R and its derivatives are sampled as above (a
 *   coordinate exactly on the last row / column takes the last cell inside the image).  With r = R(u) - F and
 *   J = (Rx j, Rx i, Rx, Ry j, Ry i, Ry), the first launch adds, in fp64, the 29 sums
 *     S[0..21) = sum (w J_a) J_b (a <= b, row-major),  S[21..27) = sum (w J_a) r,  S[27] = sum (w r) r,  S[28] = sum w
 *   (256 threads own 2048 consecutive pixels of one (b, k): a thread its 8 pixels in order, the wave by a fixed shuffle
 *   tree, the four waves as (w0 + w1) + (w2 + w3)); the second adds each (b, k)'s partials in a fixed order, projects
 *   onto the model -- 0 translation (tx, ty), 1 Euclidean (angle = atan2(m10, m00), tx, ty; the updated matrix is rebuilt
 *   from cos / sin of the new angle), 2 affine (six entries) -- solves (A + damping diag A) delta = -g by Cholesky and
 *   adds delta.  stats fp64 [B][K][4] = (S[27] / S[28]: the mean weighted squared residual AT THE INPUT MATRIX;
 *   S[28] / (H W): the covered weight per pixel; |delta|; valid).  On a non-positive or non-finite pivot, a non-finite
 *   result, S[28] = 0 or a covered fraction < min_cover the matrix is left as it was, |delta| = 0 and valid = 0.
 *   No atomics, no host synchronisation: the same call gives the same bits, whatever ws held before.
 *   ws: wire_register_gn_ws_bytes(B, K, H, W) bytes, 8-byte aligned; after the call its first B K 29 doubles hold the
 *   sums S of every (b, k).
 * B, K, H or W < 1, more workgroups than a grid holds, model outside 0..2, damping or min_cover negative or not finite,
 * a misaligned pointer, or a NULL pointer other than weight: WIRE_ERR_ARG before any HIP call (the size query too); a ws
 * that is too small: WIRE_ERR_SIZE.                                                                               */
int wire_remap_bilinear_fwd(void* stream, const float* img, int H, int W, int C, const float* xy, int64_t n,
                            int normalized, float* out);
int wire_remap_bilinear_bwd_xy(void* stream, const float* img, int H, int W, int C, const float* xy, const float* g_out,
                               int64_t n, int normalized, float* g_xy);
int64_t wire_register_gn_ws_bytes(int B, int K, int H, int W);
int wire_register_gn_step(void* stream, const float* ref, const float* frames, const float* weight, int B, int K, int H,
                          int W, int model, double damping, double min_cover, double* mats, double* stats, void* ws,
                          int64_t ws_bytes);

/* Image-to-image resampling in cv2.resize's modes, its adjoint and the super-resolution loss under it (wire_resize.hip,
 * DESIGN section 31).  R = R_v (x) R_h acts on a channel-last image x [H][W][C] (row n = i*W + j is the network's own
 * layout) and gives [Hl][Wl][C]; it is separable and linear, and each axis (n_in sources, n_out outputs, scale s: sy for
 * the rows, sx for the columns; cv2 uses s = n_in / n_out with an explicit size and s = 1 / f with fx / fy) is a table.
 * Output d of an axis, in fp64:
 *   NEAREST  one tap at min(floor(d s), n_in - 1)
 *   LINEAR   x = (d + 0.5) s - 0.5, i = floor(x), f = x - i; taps (i, 1 - f), (i + 1, f)
 *   CUBIC    the same x, i, f; taps i - 1 .. i + 2 with the Keys kernel at A = -0.75:
 *              w0 = ((A (f+1) - 5A)(f+1) + 8A)(f+1) - 4A,  w1 = ((A+2) f - (A+3)) f^2 + 1,  w2 = w1 at 1 - f,
 *              w3 = 1 - w0 - w1 - w2
 *   AREA     the cell [a, b) = [d s, min((d + 1) s, n_in)); every source pixel i, floor(a) <= i < ceil(b), whose overlap
 *            min(i + 1, b) - max(i, a) is positive is a tap of weight overlap / (b - a)
 * Tap indices are clamped to [0, n_in - 1] and taps that meet after clamping are added into one (in tap order), so every
 * output has a contiguous run of distinct sources start[d] .. start[d] + count[d] - 1.  s == 1 gives f = 0 and all weight
 * on tap d in every mode; that one tap (weight exactly 1) is kept and its zero-weight neighbours are not.  A linear /
 * cubic x more than four pixels outside the image puts weight 1 on the border pixel.  Weights are rounded to fp32 once,
 * at the end.  start and start + count are non-decreasing in d, so the outputs whose run contains source i form a
 * contiguous range lo[i] .. hi[i] (lo = hi + 1: none), and R^T is a GATHER over that range: no atomics.
 * These are cv2's documented formulas, by construction and NOT measured against cv2 (which also quantises its weights
 * for 8-bit images).  Two differences on purpose: cv2's non-integer INTER_AREA drops partial overlaps below 1e-3 without
 * renormalising, this operator keeps them; cv2's INTER_AREA with n_out > n_in silently becomes a linear variant, here it
 * is refused.
 *
 * tab: DEVICE, 4-byte aligned, wire_resize_tab_bytes bytes -- per axis (rows first) int32 start[n_out], count[n_out],
 *   lo[n_in], hi[n_in], then fp32 w[n_out][K], K = the axis' largest count (weights behind count[d] are 0).  The host
 *   evaluates the same run function as the kernel, so it knows K, and the layout, without reading the device.
 * wire_resize_tables: one launch writes all of tab (fp64 arithmetic, no contraction).  The forward, the adjoint and the
 *   loss read tab and nothing else about the geometry -- the adjoint uses the forward's own fp32 weights and is its
 *   exact transpose -- but every call takes the same (H, W, Hl, Wl, mode, sy, sx), which give the layout.
 * wire_resize_fwd: y [Hl][Wl][C] = R x.  wire_resize_bwd: g_x [H][W][C] = R^T g_y; EVERY element of g_x is written, the
 *   sources that no output touches with +0.0.  One thread per element of the side written, any C >= 1, the channel
 *   fastest; fp32 accumulation from +0.0, rows outer, columns inner, both ascending:
 *     acc = fma(wv[a], r_a, acc),   r_a = (... fma(wh[1], x[a][1], fma(wh[0], x[a][0], +0.0)) ...)
 *   (the adjoint: the same with the outputs lo .. hi in place of the taps).  An equal-size call copies the bits (-0.0
 *   becomes +0.0).  x / y and g_y / g_x must not overlap.
 * wire_resize_mse_grad: the super-resolution loss of wire_avgpool_mse_grad under R.  y [H*W][O], gt_lr [Hl*Wl][O]:
 *     rec = R y;   loss = sum (rec - gt_lr)^2 / (Hl Wl O);   g_y = R^T ( fl(2 / (Hl Wl O)) (rec - gt_lr) )
 *   Two launches: the forward stores the scaled residual to ws, rec to rec_lr (optional, NULL = not wanted) and a sum of
 *   squares per block of 256 threads (wire_block_sum) to partial; the gather adjoint writes EVERY element of g_y, and its
 *   block 0 adds the blocks' sums in a fixed order (wire_block_sum) and overwrites loss_out[0].  No atomics, no host
 *   synchronisation: the same call gives the same bits, whatever ws, partial and the outputs held before.
 *   ws: wire_resize_mse_grad_ws_bytes(Hl, Wl, O) bytes, 4-byte aligned; partial: >= 1024 floats of scratch.
 * H, W, Hl or Wl < 1, C / O < 1, a mode outside the enum, AREA with n_out > n_in on either axis or with a last cell that
 * begins outside the source ((n_out - 1) s >= n_in), a scale that is not finite or <= 0, sizes beyond 63 bits, ws_bytes
 * too small, or a NULL pointer other than rec_lr: WIRE_ERR_ARG before any HIP call (the size queries too).  tab is
 * trusted to be what wire_resize_tables wrote for the same geometry; the kernels hold every index they read from it
 * inside the arrays.                                                                                              */
typedef enum wire_resize_mode {   /* cv2's INTER_NEAREST, INTER_LINEAR, INTER_CUBIC, INTER_AREA */
  WIRE_RESIZE_NEAREST = 0,
  WIRE_RESIZE_LINEAR = 1,
  WIRE_RESIZE_CUBIC = 2,
  WIRE_RESIZE_AREA = 3
} wire_resize_mode;
int64_t wire_resize_tab_bytes(int H, int W, int Hl, int Wl, int mode, double sy, double sx);
int64_t wire_resize_mse_grad_ws_bytes(int Hl, int Wl, int O);
int wire_resize_tables(void* stream, int H, int W, int Hl, int Wl, int mode, double sy, double sx, void* tab);
int wire_resize_fwd(void* stream, const void* tab, int H, int W, int Hl, int Wl, int mode, double sy, double sx,
                    const float* x, int C, float* y);
int wire_resize_bwd(void* stream, const void* tab, int H, int W, int Hl, int Wl, int mode, double sy, double sx,
                    const float* g_y, int C, float* g_x);
int wire_resize_mse_grad(void* stream, const void* tab, int H, int W, int Hl, int Wl, int mode, double sy, double sx,
                         const float* y, int O, const float* gt_lr, float* g_y, float* rec_lr, float* loss_out,
                         void* ws, int64_t ws_bytes, float* partial);

/* Volume rendering of a 3-D net along camera rays (wire_render.hip): the sampler that turns rays
 * into the net's input rows, the emission-absorption compositing of the net's rows into one colour per ray, its
 * adjoint, and the loss kernel of a training step.  All pointers DEVICE fp32.  R rays, S >= 1 samples each; the net's
 * row of sample s of ray r is y[r S + s] = (c_raw[0..C), s_raw) with C = O - 1 colour channels, O in 2..8.
 * wire_ray_samples: rays [R][6] = (origin, direction); the ray's bounds are (near, far) = bounds[r] when bounds
 *   [R][2] != NULL, else the two scalars (finite).  jitter [R][S] holds u in [0, 1); NULL means midpoints, u = 0.5.  In
 *   fp64 from the fp32 inputs, left to right, no contraction, each output rounded to fp32 once:
 *     t_s = near + ((s + u_s) (far - near)) / S,   t_{s+1} likewise, and far for the last sample,
 *     coords[r S + s] = o + t_s d,   ts[r][s] = t_s,   deltas[r][s] = (t_{s+1} - t_s) sqrt(dx dx + dy dy + dz dz).
 *   A ray with far <= near (or a NaN bound) gets t_s = near and deltas = 0 for every sample: it composites to the
 *   background and receives zero gradient.  coords [R S][3], ts and deltas [R][S]; one thread per sample.
 * wire_composite_fwd: density = 0: sigma = softplus(s_raw); 1: sigma = max(s_raw, 0).  c = sigmoid(c_raw),
 *   a_s = sigma_s deltas_s,  tau_s = sum_{j<s} a_j,  T_s = exp(-tau_s),  w_s = T_s (1 - exp(-a_s)),  T_S = exp(-tau_S):
 *     rgb[r] = sum_s w_s c_s + T_S bg,   acc[r] = 1 - T_S,   depth[r] = sum_s w_s ts_s
 *   bg [C], NULL = 0; acc and depth [R] are optional outputs; rgb [R][C].
 * wire_composite_bwd: g_rgb [R][C], optional g_acc and g_depth [R] (NULL = 0); EVERY element of g_y [R S][O] is
 *   written.  With q_s = <c_s, g_rgb> + ts_s g_depth and q_bg = <bg, g_rgb> - g_acc (acc = 1 - T_S enters through T_S
 *   alone; g_acc appears nowhere else),
 *     d/dsigma_s = deltas_s ( T_{s+1} q_s - sum_{j>s} w_j q_j - T_S q_bg ),  times softplus' = sigmoid(s_raw) or the
 *     mask s_raw > 0;   d/dc_raw_s = w_s g_rgb (.) c (1 - c).
 * wire_composite_mse_grad: one launch runs the forward sweep,
 *     loss_out[0] = shard * sum (rgb - target)^2 / (R C),   g_rgb = 2 shard / (R C) * (rgb - target)
 *   (the factor a single fp32 number, the residual of the fp32-rounded rgb) and the reverse sweep with g_acc = g_depth
 *   = 0; it writes loss_out[0], every element of g_y and, if rgb != NULL, rgb.  target [R][C].  shard is
 *   wire_mse_grad's `weight`.  partial: >= 2048 floats of scratch.  g_y and rgb carry the bits of wire_composite_fwd,
 *   that residual formed in fp32, and wire_composite_bwd.
 * A wave owns a ray and its lanes consecutive samples, 64 at a time; a_s, tau, T, w, the sums over samples and the
 * suffix sum (a reverse sweep, not total minus prefix) are fp64, softplus and sigmoid fp32, every output rounded to fp32
 * once.  No exponential of a positive argument, no inf - inf: finite for every finite input.  No atomics; which lane
 * adds what, in which order, depends on (R, S, O) alone: the same call gives the same bits, whatever partial held.
 * y and g_y are 16-byte aligned, everything else 4-byte.  R or S < 1, O outside 2..8, density outside {0, 1}, R S O
 * beyond 63 bits, more workgroups than a grid holds (2^31 - 1; a workgroup takes 4 rays, the sampler's 256 samples),
 * scalar bounds or shard not finite, a misaligned pointer, or a NULL pointer other than bounds / jitter / bg / acc /
 * depth / g_acc / g_depth / rgb of the loss kernel: WIRE_ERR_ARG before any HIP call.  No workspace beyond partial.  */
int wire_ray_samples(void* stream, const float* rays, const float* bounds, float near_, float far_, const float* jitter,
                     int64_t R, int S, float* coords, float* ts, float* deltas);
int wire_composite_fwd(void* stream, const float* y, const float* ts, const float* deltas, const float* bg, int64_t R,
                       int S, int O, int density, float* rgb, float* acc, float* depth);
int wire_composite_bwd(void* stream, const float* y, const float* ts, const float* deltas, const float* bg,
                       const float* g_rgb, const float* g_acc, const float* g_depth, int64_t R, int S, int O,
                       int density, float* g_y);
int wire_composite_mse_grad(void* stream, const float* y, const float* ts, const float* deltas, const float* bg,
                            const float* target, int64_t R, int S, int O, int density, float shard, float* g_y,
                            float* loss_out, float* rgb, float* partial);

/* Hierarchical sampling along the rays (wire_render.hip): the weights of a coarse pass and the
 * second set of samples they call for.  All pointers DEVICE fp32, 4-byte aligned except y (16).
 * wire_composite_weights: w[r][s] = (float)(T_s (1 - exp(-a_s))), the summand of wire_composite_fwd's rgb and acc with
 *   its lane map, fp64 scan and carry, so the same bits; it reads column O - 1 of y [R S][O] and deltas [R][S] only and
 *   writes EVERY element of w [R][S].  density as wire_composite_fwd.
 * wire_ray_resample: rays, bounds / near_ / far_ as wire_ray_samples.  ts_c [R][S]: the coarse samples, nondecreasing
 *   inside [near, far] as wire_ray_samples makes them (NOT checked: unsorted values give finite, meaningless output);
 *   w [R][S] their weights; jitter [R][Nf] holds v in [0, 1), NULL means v = 0.5; eps > 0 (NeRF's sample_pdf: 1e-5).
 *   Per ray, in fp64 from the fp32 inputs, no contraction, each output rounded to fp32 once:
 *     edges   e_0 = near,  e_s = (ts_c[s-1] + ts_c[s]) / 2,  e_S = far        (bin s contains sample s)
 *     mass    p_s = min(max(w_s, 0), FLT_MAX) + eps  (NaN counts as 0);  c_0 = 0,  c_{s+1} = c_s + p_s,  tot = c_S
 *     draws   u_k = ((k + v_k) / Nf) tot,  k = 0 .. Nf-1
 *     inverse s = the largest index in [0, S-1] with c_s <= u_k,  f = clamp((u_k - c_s) / (c_{s+1} - c_s), 0, 1)
 *             (f = 0 where eps vanished beside a huge weight and the bin is empty),
 *             tf_k = min(e_s + f (e_{s+1} - e_s), e_{s+1})
 *     merge   the S coarse and Nf fine values by rank, coarse first on a tie, compared in fp64:
 *             pos(coarse i) = i + #{fine < ts_c[i]},  pos(fine k) = k + #{coarse <= tf_k}
 *   and on the merged t_0 <= ... <= t_{S+Nf-1} the sampler's recipe from the unrounded t, far behind the last one:
 *     coords[r (S+Nf) + k] = o + t_k d,   ts[r][k] = t_k,   deltas[r][k] = (t_{k+1} - t_k) sqrt(dx dx + dy dy + dz dz).
 *   A ray with far <= near (or a NaN bound) gets t = near and deltas = 0 everywhere.  coords [R (S+Nf)][3], ts and
 *   deltas [R][S+Nf]; EVERY element is written.  The CDF is an inclusive scan of 64 samples plus a carry, so its
 *   association differs from a running sum's.  A wave owns a ray; CDF, fine samples and merged list live in LDS, which
 *   limits S and Nf to 1024 each.  No atomics: the same call gives the same bits.
 * R, S or Nf < 1, S or Nf > 1024, O outside 2..8, density outside {0, 1}, R (S+Nf) beyond 63 bits, more workgroups than
 * a grid holds, scalar bounds not finite, eps not finite or <= 0, a misaligned pointer, or a NULL pointer other than
 * bounds / jitter: WIRE_ERR_ARG before any HIP call.                                                                 */
int wire_composite_weights(void* stream, const float* y, const float* deltas, int64_t R, int S, int O, int density,
                           float* w);
int wire_ray_resample(void* stream, const float* rays, const float* bounds, float near_, float far_, const float* ts_c,
                      const float* w, const float* jitter, float eps, int64_t R, int S, int Nf, float* coords,
                      float* ts, float* deltas);

/* Video compressive sensing (per-pixel coded exposure, modules/lin_inverse.py:42-95): the loss of a video estimate
 * against a coded video, fused with its backward.  The T frames of pixel p are multiplied by that pixel's mask and
 * summed in groups of nframes (lin_inverse.py:79-84) into C = ceil(T / nframes) coded frames; nframes > T gives one.
 * dup_last = 1 keeps a property of the reference: its trailing `if idx < video_ten.shape[1]` (lin_inverse.py:86-91) is
 * always true, so the last group is appended a second time, the coded video has C + 1 frames with frame C equal to
 * frame C - 1, and an MSE against it weights the last group twice.  dup_last = 0 is the plain operator.  With
 * C' = C + dup_last and count = C' NP O:
 *   est[c][p][o] = sum_{k in group c} mask[p][k] y[p T + k][o]          (est[C] = est[C-1] when dup_last)
 *   d = est - gt;   loss = sum d^2 / count
 *   g_y[p T + k][o] = mask[p][k] 2 / count (d[c(k)][p][o] + (dup_last and c(k) == C - 1 ? d[C][p][o] : 0))
 * Layout: the row order of the 3-D grid (row (i W + j) T + k), so a pixel's T frames are T O consecutive floats.
 * y / g_y are LOCAL to the slab of pixels [p0, p0 + n_pix): [n_pix T][O].  mask [NP][T] (any float values, shared by
 * the channels; this is the (H, W, totalframes) array of get_video_coding_frames as it lies in memory, NP = H W),
 * gt [C'][NP][O] and est [C'][NP][O] (optional, NULL = not wanted) are whole-video arrays indexed by the global pixel.
 * loss_out[0] is overwritten with THIS SLAB's sum d^2 / count (the global count): the losses of slabs that cover the
 * video add up to the loss.  Every element of g_y is written exactly once.  No atomics, every sum in a fixed order:
 * the same call gives the same bits.  partial: >= 1024 floats of scratch.
 * T, O, nframes, n_pix or NP < 1, p0 < 0, p0 + n_pix > NP, dup_last not 0 / 1, or a NULL pointer other than est:
 * WIRE_ERR_ARG before any HIP call.                                                                          */
int wire_coded_mse_grad(void* stream, const float* y, int64_t p0, int64_t n_pix, int64_t NP, int T, int O,
                        int nframes, int dup_last, const float* mask, const float* gt, float* g_y,
                        float* est, float* loss_out, float* partial);
/* The same operator in the reference's own layout, video2codedvideo of modules/lin_inverse.py:65-95 on one
 * (T, H, W) video: video [T][NP], masks [T][NP] -> coded [C'][NP], and its adjoint
 *   g_video[t][p] = masks[t][p] (g_coded[c(t)][p] + (dup_last and c(t) == C - 1 ? g_coded[C][p] : 0)).
 * T, NP or nframes < 1, dup_last not 0 / 1, a NULL pointer, or more than 2^31 - 1 blocks of 256 values:
 * WIRE_ERR_ARG before any HIP call.                                                                          */
int wire_coded_fwd(void* stream, const float* video, const float* masks, int T, int64_t NP, int nframes,
                   int dup_last, float* coded);
int wire_coded_bwd(void* stream, const float* g_coded, const float* masks, int T, int64_t NP, int nframes,
                   int dup_last, float* g_video);

/* Anisotropic total variation, utils.total_variation_loss of modules/utils.py:360-369, over `planes` images of H x W:
 *   tv(x) = sum_{p, i<H-1, j} |x[p][i+1][j] - x[p][i][j]| + sum_{p, i, j<W-1} |x[p][i][j+1] - x[p][i][j]|
 * -- a SUM, not a mean; H == 1 or W == 1 is legal and that direction contributes nothing.  Element (p, i, j) lies at
 * x[p * plane_stride + (i * W + j) * pix_stride]: planes = O, pix_stride = O, plane_stride = 1 is the network's own
 * [H*W][O] output, planes = B*C, pix_stride = 1, plane_stride = H*W a contiguous (B, C, H, W) tensor.  tv_out[0] is
 * overwritten with the sum over all planes.  One grid-stride pass, a thread per pixel adding its planes in order (a
 * block of 256 pixels loops above 262 144 pixels), the neighbours re-read through the caches; no atomics, every sum in
 * a fixed order that depends on (planes, H, W) alone: the same call gives the same bits, and so does the same image
 * under other strides.  partial: >= 1024 floats of scratch.  x, tv_out, partial: device.
 * planes, H or W < 1, a stride < 1, sizes or a largest offset beyond 63 bits, or a NULL pointer: WIRE_ERR_ARG before
 * any HIP call.                                                                                                  */
int wire_tv_fwd(void* stream, const float* x, int planes, int H, int W, int64_t pix_stride, int64_t plane_stride,
                float* tv_out, float* partial);
/* Its gradient under torch's convention d|u|/du = s(u), s in {-1, 0, +1}, s(0) = 0, times the upstream gradient g_tv[0]
 * (a DEVICE scalar: no host synchronisation):
 *   g_x[p][i][j] = g_tv[0] * (  s(x[i][j] - x[i-1][j]) - s(x[i+1][j] - x[i][j])
 *                             + s(x[i][j] - x[i][j-1]) - s(x[i][j+1] - x[i][j]) ),
 * a term whose neighbour lies outside the image being 0.  s is taken by comparison, (a > b) - (a < b), so the integer
 * factor in -4 .. 4 is exact whatever the denormal mode and every entry is one rounding of integer * g_tv[0].  g_x has
 * the layout of x (same strides); every addressed element is written exactly once, nothing between them is touched.
 * One thread per element, 256-element blocks that loop above 262 144 elements.
 * Arguments are checked as in wire_tv_fwd.                                                                        */
int wire_tv_bwd(void* stream, const float* x, int planes, int H, int W, int64_t pix_stride, int64_t plane_stride,
                const float* g_tv, float* g_x);
/* The loss of the TV-regularised image loop (bspline_image_denoise.py:160-172, there evaluated under no_grad; here the
 * term acts on the weights), fused with its backward.  y, target and g_y are full-grid [H*W][O], row i*W + j.  The MSE
 * runs over n_mse rows: idx[r] when idx != NULL (`first` is then ignored), otherwise rows first .. first + n_mse:
 *   mse  = sum_{r, o} (y[row_r][o] - target[row_r][o])^2 / (n_mse O)          (0 when n_mse == 0)
 *   loss = mse + lambda_tv tv(y)                                              (tv over the O planes of y)
 *   g_y[n][o] = [n selected] 2 (y - t)[n][o] / (n_mse O) + lambda_tv dtv/dy[n][o]
 * loss_out[0..2] = loss, mse, tv, overwritten (loss = fl(mse + fl(lambda_tv tv))).  rec (optional): rec[row_r][:] =
 * y[row_r][:], as in wire_mse_grad.  EVERY element of g_y is written, the unselected rows with the TV term alone,
 * lambda_tv * integer rounded once.  A range is handled inside the one pass over the image (one thread per element,
 * 256-element blocks that loop above 262 144 elements); with idx the pass stores
 * the TV term and a second launch over the n_mse rows adds their MSE term, each thread to its own element.  The rows of
 * idx must lie in [0, H*W) (they are trusted, as in wire_mse_grad) and be DISTINCT, as a slice of a permutation is:
 * if a row repeats, its MSE term in g_y is unspecified, and nothing outside the buffers is touched.  No atomics, every
 * sum in a fixed order: the same call gives the same bits.  partial: >= 2048 floats of scratch.
 * H, W or O < 1, O > 8, n_mse < 0 or > H*W, a range outside the grid (idx == NULL), or a NULL pointer other than idx /
 * rec: WIRE_ERR_ARG before any HIP call.                                                                          */
int wire_tv_mse_grad(void* stream, const float* y, int H, int W, int O, const float* target, const int64_t* idx,
                     int64_t first, int64_t n_mse, float lambda_tv, float* g_y, float* loss_out, float* rec,
                     float* partial);
/* The TV prior of an inverse problem, ADDED to the gradient that the operator's own backward has left in g_y (the Radon
 * adjoint, the pooled or the coded-exposure loss).  y and g_y are the network's own rows [H*W*T][O]: element
 * (i, j, k, o) lies at ((i*W + j)*T + k)*O + o; T = 1 is an image, T > 1 the (H, W, T) grid of the video step.
 *   tv_s = sum |y[i+1,j,k,o] - y[i,j,k,o]| + sum |y[i,j+1,k,o] - y[i,j,k,o]|     (utils.total_variation_loss of every
 *                                                                               frame and channel; a sum, not a mean)
 *   tv_t = sum |y[i,j,k+1,o] - y[i,j,k,o]|                                       (the same sum along the frame axis)
 *   g_y[e] = g_y[e] + (lambda_s k_s + lambda_t k_t)
 * with k_s in -4 .. 4 and k_t in -2 .. 2 the exact integer sums of s over the element's spatial and temporal pairs,
 * s by comparison and s(0) = 0 exactly as in wire_tv_bwd, a term whose neighbour lies outside the grid being 0.  Three
 * roundings, in this order: p = fl(lambda_s k_s); q = fma(lambda_t, k_t, p); g_y[e] = fl(g_y[e] + q).  Every element
 * is read and written once, by its own thread; with both lambdas 0 g_y keeps its bits up to the sign of a zero.
 * loss_out[0..3] = loss, data, tv_s, tv_t, overwritten: data = data_loss[0], a DEVICE scalar such as the slot the
 * operator wrote its loss to (no host synchronisation; NULL: 0), and
 *   loss = fl(fl(data + fl(lambda_s tv_s)) + fl(lambda_t tv_t)).
 * Both sums are reported whatever the lambdas are.  One thread per element, 256-element blocks that loop above
 * 262 144 elements, the six neighbours (O, T*O and W*T*O floats away) re-read through the caches; no atomics, every
 * sum in a fixed order: the same call gives the same bits.  partial: >= 2048 floats of scratch.
 * H, W, T or O < 1, O > 8, a lambda that is not finite, sizes beyond 63 bits, or a NULL y, g_y, loss_out or partial:
 * WIRE_ERR_ARG before any HIP call.                                                                              */
int wire_tv_add_grad(void* stream, const float* y, int H, int W, int T, int O, float lambda_s, float lambda_t,
                     const float* data_loss, float* g_y, float* loss_out, float* partial);

/* ---- iso-surface extraction (what modules/volutils.py:94-142 hands to PyMCubes) -------------------------------
 * The surface {vol >= thres} of a volume vol [H][W][T] (fp32, row-major; NaN counts as outside) as a welded, indexed
 * triangle mesh: marching tetrahedra on the six-tetrahedron Kuhn split of every cell (wire_amd/csrc/wire_iso.hip
 * states the rules).  Closed wherever the volume's boundary does not cut it, consistently wound with the normal
 * pointing from inside to outside -- by combinatorics, so also when thres equals a data value.  NOT PyMCubes' triangles.
 *   vertices: one per lattice edge (7 directions: the 3 axes, the 3 face diagonals, the body diagonal) whose ends lie
 *     on different sides, at p + t d, t = (thres - vol[p]) / (vol[p + d] - vol[p]) in fp32, in index units
 *     (i, j, k) -- the PyMCubes convention; ordered by (linear index of the lower end p, direction).
 *   faces: three vertex ids each, ordered by (linear index of the cell, tetrahedron, triangle).
 * Two passes.  wire_iso_count classifies, scans (reduce-then-scan in separate launches: no workgroup waits on another,
 * no atomics) and leaves in ws what the second pass needs; counts (DEVICE, 8-byte aligned) receives {vertices, faces}.
 * wire_iso_emit, with the same vol, sizes, thres and the ws the count left, writes verts [nverts][3] and faces
 * [nfaces][3].  It reads the two counts back from ws (16 bytes, one synchronisation of the stream) and, when
 * nverts > cap_v or nfaces > cap_f, returns WIRE_ERR_SIZE having written nothing; the kernels guard every store by the
 * capacities besides.  cap_v == 0 / cap_f == 0 allow a NULL verts / faces.  Same call, same bits, whatever ws held.
 * ws: wire_iso_ws_bytes bytes (about 9 per lattice point), device, 16-byte aligned.
 * A side < 2, more than 2^28 lattice points (so every vertex id fits an int32 and every face offset 32 bits), a NaN
 * thres, a NULL or misaligned pointer: WIRE_ERR_ARG before any HIP call (the size query too).
 * wire_iso_tet_case: host only -- the compile-time table the emit pass winds by, for tetrahedron perm (0..5, the
 * permutations of the axes in lexicographic order) and inside mask (bit n = corner v_n inside): bits 0-1 = the number
 * of triangles, then three bits per corner, triangle 0 at bits 2 / 5 / 8 and triangle 1 at bits 11 / 14 / 17, each the
 * edge 01 02 03 12 13 23 (0..5) of the tetrahedron that the corner lies on.                                          */
int64_t wire_iso_ws_bytes(int H, int W, int T);
int wire_iso_count(void* stream, const float* vol, int H, int W, int T, float thres, void* ws, int64_t* counts);
int wire_iso_emit(void* stream, const float* vol, int H, int W, int T, float thres, const void* ws, float* verts,
                  int64_t cap_v, int32_t* faces, int64_t cap_f);
int wire_iso_tet_case(int perm, int inside_mask);
/* Separable Gaussian blur of a volume [H][W][T]: 2 R + 1 taps per axis, R = floor(4 sigma + 0.5) <= 32, weights
 * exp(-x^2 / 2 sigma^2) normalised in fp64 and rounded to fp32, edge values replicated; axis T, then W, then H, per
 * axis the taps added from -R to +R, every product and sum rounded once.  in, tmp, out: three distinct device buffers
 * of H W T floats; in is not written.  A side < 1, sigma not in (0, 8], a NULL pointer or two equal ones: WIRE_ERR_ARG. */
int wire_gauss3_blur(void* stream, const float* in, int H, int W, int T, float sigma, float* tmp, float* out);

/* torch.optim.Adam single step over a flat fp32 buffer (complex tensors as
 * real pairs; wire_image_denoise.py:123-125).  step is 1-based.  param,
 * exp_avg and exp_avg_sq are updated in place; the bias corrections are taken
 * in fp64 on the host.  With lr == 0 param keeps its bits.  count < 0,
 * step < 1 or a NULL pointer: WIRE_ERR_ARG before any HIP call; count == 0
 * returns WIRE_OK and touches nothing.                                       */
int wire_adam_step_flat(void* stream, float* param, const float* grad,
                        float* exp_avg, float* exp_avg_sq, int64_t count,
                        float lr, float beta1, float beta2, float eps,
                        int64_t step);

/* Evaluation metrics without a device->host copy of the reconstruction
 * (the reference copies the whole image to the host every epoch,
 * wire_image_denoise.py:161-178, and binarises the volume on the host side,
 * modules/volutils.py:74-91).  out2 / partial: device; partial >= 2048 floats.
 *   mode 0: out2 = { sum (gt-rec)^2, max(gt) }  -> utils.psnr = 10 log10(max / (sum/count))
 *                                                   (modules/utils.py:67-82: max(x), not max^2)
 *   mode 1: out2 = { |rec>=thres & gt!=0|, |rec>=thres or gt!=0| }  -> IoU = out2[0] / out2[1]
 *           (rec is NOT binarised in place, unlike get_I_and_U).  The comparisons are the IEEE ones: a NaN in rec
 *           is below every threshold, a NaN in gt is != 0, -0.0 is == 0.
 * max(gt) is a value of gt, exact.  The two counts are sums of fp32 ones: EXACT up to 2^24 elements per call (every
 * partial sum is an integer <= 2^24), rounded to fp32 beyond -- a caller with more elements splits them into calls of
 * at most 2^24 and adds the counts itself (modules/volutils.py does).  Fixed summation order: the same call gives the
 * same bits.  mode outside {0, 1}, count < 1 or a NULL pointer: WIRE_ERR_ARG before any HIP call.  */
int wire_eval_metric(void* stream, int mode, const float* rec, const float* gt,
                     int64_t count, float thres, float* out2, float* partial);

/* Structural similarity (SSIM) of two channel-last images x, y [H][W][O] without a device->host copy or a transposed
 * copy: the windowed moments m(x), m(y), m(x^2), m(y^2), m(xy) under a separable window of `taps` weights
 * (window_host, HOST memory, applied along both axes) over the valid region [H-taps+1][W-taps+1], and per pixel and
 * channel
 *   vx = cov_norm (m(x^2) - m(x)^2),  vy = cov_norm (m(y^2) - m(y)^2),  vxy = cov_norm (m(xy) - m(x) m(y)),
 *   S  = (2 m(x) m(y) + c1) (2 vxy + c2) / ((m(x)^2 + m(y)^2 + c1) (vx + vy + c2)).
 * out1[0] = the mean of S over all pixels and channels; map (optional, NULL for none) receives S itself,
 * [H-taps+1][W-taps+1][O].  Two definitions are in use in the reference's drivers, both with c1 = (0.01 L)^2,
 * c2 = (0.03 L)^2, L = the data range:
 *   - pytorch_msssim.ssim(im_gt, im_rec, data_range=1, size_average=True), every epoch of the super-resolution loops
 *     (wire_SISR.py:169, bspline_SISR.py:192): 11 taps g[i] = exp(-(i-5)^2 / (2 1.5^2)) normalised to sum 1 in fp32,
 *     cov_norm = 1;
 *   - skimage.metrics.structural_similarity(..., multichannel=True) with its defaults, the final report of wire_ct.py,
 *     bspline_ct.py, wire_multi_sr.py, both SISR drivers and modules/volutils.py: 7 taps of 1/7 (a uniform filter,
 *     then 3 pixels cropped at each side = the valid region), cov_norm = 49/48 (sample covariance); the mean over
 *     channels of per-channel means is the same number as the mean over everything.
 * taps odd in 3..11, O in 1..8, H, W >= taps, cov_norm / c1 / c2 finite, every pointer but map non-NULL: anything else
 * is WIRE_ERR_ARG before any HIP call; ws_bytes < wire_ssim_ws_bytes(H, W, O, taps) is WIRE_ERR_SIZE.  fp32; per-tile
 * partial sums reduced in a fixed order in ws (no atomics: the same call gives the same bits).  x, y, out1, map, ws:
 * device.                                                                                                         */
int64_t wire_ssim_ws_bytes(int H, int W, int O, int taps);
int wire_ssim(void* stream, const float* x, const float* y, int H, int W, int O, int taps, const float* window_host,
              float cov_norm, float c1, float c2, float* out1, float* map, void* ws, int64_t ws_bytes);
/* The gradient of that mean with respect to the SECOND image, times the upstream gradient g_ssim[0] (a DEVICE scalar: no
 * host synchronisation): x = gt, y = rec, the window and constants as in wire_ssim,
 *   g_y[q] = g_ssim[0] / ((H-taps+1)(W-taps+1) O) * ( T(A)[q] + 2 y[q] T(B)[q] + x[q] T(C)[q] ),
 *   A = dS/dmy - 2 cov_norm my dS/dvy - cov_norm mx dS/dvxy,  B = cov_norm dS/dvy,  C = cov_norm dS/dvxy,
 *   dS/dmy = 2 mx n2 / (d1 d2) - 2 my S / d1,  dS/dvy = -S / d2,  dS/dvxy = 2 n1 / (d1 d2)
 * (n1 = 2 mx my + c1, n2 = 2 vxy + c2, d1 = mx^2 + my^2 + c1, d2 = vx + vy + c2), T the transpose of the separable valid
 * convolution: every input pixel collects the coefficient of each window that covers it under that window's tap.
 * g_y [H][W][O]: every element is written exactly once.  A workgroup owns 16 x 32 input pixels, recomputes the moments
 * of the windows that cover them from a halo of 2 (taps - 1) about a constant it subtracts from both images (the
 * forward's cancellation-safe shift, exact for a window that does not sum to one), one channel at a time: at most
 * 58 320 B of LDS, no intermediate in global memory, no atomics, every sum in a fixed order -- the same call gives the
 * same bits.  ws: wire_ssim_bwd_ws_bytes(H, W, O, taps) bytes (a small constant today: the argument is there for a
 * tiling that needs more).  Arguments are checked as in wire_ssim (g_ssim and g_y must not be NULL): WIRE_ERR_ARG before
 * any HIP call, WIRE_ERR_SIZE for a ws that is too small.  x, y, g_ssim, g_y, ws: device.                          */
int64_t wire_ssim_bwd_ws_bytes(int H, int W, int O, int taps);
int wire_ssim_bwd(void* stream, const float* x, const float* y, int H, int W, int O, int taps, const float* window_host,
                  float cov_norm, float c1, float c2, const float* g_ssim, float* g_y, void* ws, int64_t ws_bytes);
/* The loss of an SSIM-regularised image loop, fused with its backward.  y, target and g_y are full-grid [H*W][O], row
 * i*W + j.  The MSE runs over n_mse rows, given exactly as wire_tv_mse_grad takes them (idx[r] when idx != NULL, otherwise
 * rows first .. first + n_mse); the index is that of the FULL reconstruction against the full target, wire_ssim(target, y):
 *   mse  = sum_{r, o} (y[row_r][o] - target[row_r][o])^2 / (n_mse O)          (0 when n_mse == 0)
 *   loss = mse + lambda_ssim (1 - ssim)
 *   g_y[n][o] = [n selected] 2 (y - t)[n][o] / (n_mse O) - lambda_ssim dssim/dy[n][o]
 * loss_out[0..2] = loss, mse, ssim, overwritten.  rec (optional): rec[row_r][:] = y[row_r][:].  EVERY element of g_y is
 * written, the unselected rows with the SSIM term alone.  A range is handled inside the one pass of wire_ssim_bwd's
 * tiles; with idx that pass stores the SSIM term and a second launch over the n_mse rows adds their MSE term, each
 * thread to its own element.  The rows of idx are trusted and must be DISTINCT, as for wire_tv_mse_grad.  With
 * lambda_ssim == 0 the index is not evaluated: loss = mse, loss_out[2] = 0, and g_y holds the bits wire_tv_mse_grad
 * stores at lambda_tv = 0 (up to the sign of a zero).  No atomics, every sum in a fixed order, no host synchronisation.
 * ws: wire_ssim_mse_grad_ws_bytes(H, W, O, taps) bytes, device.
 * taps, O, H, W, cov_norm, c1, c2 as for wire_ssim, n_mse < 0 or > H*W, a range outside the grid (idx == NULL), a
 * lambda_ssim that is not finite, or a NULL pointer other than idx / rec: WIRE_ERR_ARG before any HIP call; a ws that
 * is too small: WIRE_ERR_SIZE.                                                                                      */
int64_t wire_ssim_mse_grad_ws_bytes(int H, int W, int O, int taps);
int wire_ssim_mse_grad(void* stream, const float* y, int H, int W, int O, const float* target, int taps,
                       const float* window_host, float cov_norm, float c1, float c2, const int64_t* idx, int64_t first,
                       int64_t n_mse, float lambda_ssim, float* g_y, float* loss_out, float* rec, void* ws,
                       int64_t ws_bytes);

/* Best-reconstruction tracking of the drivers without a device->host copy per epoch
 * (wire_image_denoise.py:176-178: `if (mse_array[epoch] < best_mse) or (epoch == 0): best_mse = ...; best_img = imrec`;
 * wire_occupancy.py:170-172 with lossval): if force != 0 or metric[0] < best_metric[0], copy src[0..count) to dst
 * and metric[0] to best_metric[0]; updated (optional, device int) receives 1 / 0.  All pointers device.  A NaN metric
 * is never taken (unless forced); any metric below +inf replaces a best of +inf.  Not taken: dst and best_metric keep
 * their bits.  The copy moves 16 bytes per thread: with count > 0, src and dst must be 16-BYTE ALIGNED (count itself may
 * be any number; the last count % 4 floats are copied one by one, and nothing behind dst[count - 1] is written).
 * count == 0 updates the scalar alone (src / dst may be NULL).  metric or best_metric NULL, count < 0, count > 0 with
 * src or dst NULL or misaligned: WIRE_ERR_ARG before any HIP call.                                              */
int wire_track_best(void* stream, const float* metric, float* best_metric, int force, const float* src,
                    float* dst, int64_t count, int* updated);
/* CT forward operator of wire_ct.py:128-133 -- lin_inverse.radon (modules/lin_inverse.py:19-40): every angle
 * rotates the image (kornia.geometry.rotate of kornia 0.6.5: about ((W-1)/2, (H-1)/2), counter-clockwise degrees,
 * bilinear, zero padding, align_corners) and sums over the rows: img [H][W] -> sino [nangles][W].  wire_radon_bwd
 * is its adjoint, g_sino [nangles][W] -> g_img [H][W] (overwritten; float atomics: summation order, hence the last
 * bits, vary from run to run; the forward has a fixed order and gives the same bits).  With c / s = cos / sin of angle a,
 * (cx, cy) = ((W-1)/2, (H-1)/2), xj = j - cx, yi = i - cy:
 *   sino[a][j] = sum_i bilinear(img, x = c xj - s yi + cx, y = s xj + c yi + cy),
 * taps outside the image reading zero (a sample up to one pixel outside still interpolates against the border).
 * A side of 1 has no reference behaviour (kornia divides by W - 1 and H - 1); here the formula as written holds there.
 * H, W or nangles < 1 or a NULL pointer: WIRE_ERR_ARG before any HIP call.                                   */
int wire_radon_fwd(void* stream, const float* img, const float* angles_deg, int H, int W, int nangles, float* sino);
int wire_radon_bwd(void* stream, const float* g_sino, const float* angles_deg, int H, int W, int nangles,
                   float* g_img);
/* The volume form of the CT operator (lin_inverse.radon(imten, angles, is_3d=True), modules/lin_inverse.py:19-40), on
 * CHANNEL-LAST data: vol [H][W][C] -> sino [nangles][W][C], the channel -- the slice of the volume -- innermost, which
 * is how the rows of a 3-D grid, (i W + j) T + k, already hold a network's output.  Channel c is wire_radon_fwd on
 * slice c, in the same arithmetic with the rows added in ascending i: wire_radon_vol_fwd gives, channel by channel,
 * the BITS of wire_radon_fwd on that slice (C = 1: of wire_radon_fwd).  wire_radon_vol_bwd is the adjoint,
 * g_sino [nangles][W][C] -> g_vol [H][W][C], as a gather: every element of g_vol is written exactly once (no memset
 * is needed, and none is made), no atomics, every sum in a fixed order -- the same call gives the same bits.  Its
 * taps and weights are the forward's, tap for tap: each candidate sample's position is evaluated as the forward
 * evaluates it, and the forward's floor decides whether the pixel is one of its taps.
 * H, W, C or nangles < 1, H W or nangles W above 2^31 - 1, more workgroups than one launch takes (forward:
 * nangles ceil(W C / 256), with C / 4 for C when C % 4 == 0 and both pointers are 16-byte aligned, above 2^31 - 1;
 * adjoint: C > 64 * 65535) or a NULL pointer: WIRE_ERR_ARG before any HIP call.  Sides of 1 are ordinary cases;
 * H W C and nangles W C may pass 2^31.                                                                          */
int wire_radon_vol_fwd(void* stream, const float* vol, const float* angles_deg, int H, int W, int C, int nangles,
                       float* sino);
int wire_radon_vol_bwd(void* stream, const float* g_sino, const float* angles_deg, int H, int W, int C, int nangles,
                       float* g_vol);
/* torch.sigmoid of the dense occupancy query before the cube is written (modules/volutils.py:128-131), in place.
 * NaN stays NaN; +inf and every x >= 17 give exactly 1, -inf exactly 0; below x = -87.33 the true value is denormal
 * and the result lies in [0, 2^-126]; elsewhere the relative error is <= 2^-21.  count < 0, or count > 0 with x NULL:
 * WIRE_ERR_ARG before any HIP call; count == 0 returns WIRE_OK.                                                  */
int wire_sigmoid_inplace(void* stream, float* x, int64_t count);

/* ---- ComplexGaborLayer2D (modules/wire2d.py:21-67) on native tensors ---------------------
 * act = exp(j w0 lin) exp(-s0^2 (|lin|^2 + |sy|^2)),  lin = x W^T + b,  sy = x V^T + c (scale_orth).
 * Same conventions as wire_gabor_fwd / wire_gabor_bwd: x, act, g_act, g_x complex64 [n][features]
 * (is_first: x real float32 [n][in <= 4], W, b, V, c real, g_x unused); W, V [out][in], b, c [out];
 * the backward recomputes the forward from x.  g_x may be NULL.                                   */
int64_t wire_layer2d_ws_bytes(int64_t n, int in_features, int out_features);
int wire_gabor2d_fwd(void* stream, const void* x, const void* W, const void* b, const void* V,
                     const void* c, float omega0, float scale0, int64_t n, int in_features,
                     int out_features, int is_first, void* act_out, void* ws, int64_t ws_bytes);
int wire_gabor2d_bwd(void* stream, const void* g_act, const void* x, const void* W, const void* b,
                     const void* V, const void* c, float omega0, float scale0, int64_t n,
                     int in_features, int out_features, int is_first, void* g_x, void* g_W, void* g_b,
                     void* g_V, void* g_c, void* ws, int64_t ws_bytes);
/* first layers (is_first) with the coordinate gradient: g_x [n][in <= 4] f32 = g_u W (+ g_p V for wire2d); the
 * parameter gradients as wire_gabor_bwd / wire_gabor2d_bwd produce them, or (all NULL) not at all.  Same workspace. */
int wire_gabor_bwd_first_coords(void* stream, const void* g_act, const float* x, const float* W, const float* b,
                                float omega0, float scale0, int64_t n, int in_features, int out_features,
                                float* g_x, float* g_W, float* g_b, void* ws, int64_t ws_bytes);
int wire_gabor2d_bwd_first_coords(void* stream, const void* g_act, const float* x, const float* W, const float* b,
                                  const float* V, const float* c, float omega0, float scale0, int64_t n,
                                  int in_features, int out_features, float* g_x, float* g_W, float* g_b,
                                  float* g_V, float* g_c, void* ws, int64_t ws_bytes);

/* trainable omega_0 / scale_0 of ComplexGaborLayer2D (modules/wire2d.py:42-43 with trainable=True):
 * out2 (device, 2 floats) = { dL/d omega_0, dL/d scale_0 }; operands and workspace as wire_gabor2d_bwd.  Summation
 * and refusals as wire_gabor_hparam_grad (V and c must not be NULL; ws: wire_layer2d_ws_bytes).              */
int wire_gabor2d_hparam_grad(void* stream, const void* g_act, const void* x, const void* W, const void* b,
                             const void* V, const void* c, float omega0, float scale0, int64_t n, int in_features,
                             int out_features, int is_first, float* out2, void* ws, int64_t ws_bytes);

/* ---- the frozen first stage of WIRE_KIND_BSPLINE_MS (Scaled_Bsplines_form.forward) on native tensors -------------
 * x [n][in] f32, W [out][in], b [out] -> out [n][out] f32: B(lin_j / scales[g(j)]) with the column groups of
 * wire_net_desc_ms: out = SHF, nscales = T, scales_host in HOST memory.  No backward: the stage is frozen.        */
int wire_mscale_first_fwd(void* stream, const float* x, const float* W, const float* b, int64_t n, int in_features,
                          int out_features, int nscales, const float* scales_host, float* out);

/* ---- the scale combiner of WIRE_KIND_BSPLINE_M2 (AdaptiveScaleCombiner 'freq_combine') on native tensors -----------
 * t [S][n][O] f32 (pass k's outputs at rows k n ..), W1 [128][S O], b1 [128], W2 [O][128], b2 [O] -> y [n][O];
 * S in 1..8, O in 1..8.  The backward writes g_t [S][n][O] and gW1, gb1, gW2, gb2 (deterministic: per-block partials
 * reduced in a fixed order in ws, wire_m2_combine_ws_bytes(nscales, out_features, n) bytes).                         */
int wire_m2_combine_fwd(void* stream, int nscales, int out_features, const float* W1, const float* b1, const float* W2,
                        const float* b2, const float* t, int64_t n, float* y);
int64_t wire_m2_combine_ws_bytes(int nscales, int out_features, int64_t n);
int wire_m2_combine_bwd(void* stream, int nscales, int out_features, const float* W1, const float* b1, const float* W2,
                        const float* b2, const float* t, int64_t n, const float* g_y, float* g_t, float* gW1,
                        float* gb1, float* gW2, float* gb2, void* ws, int64_t ws_bytes);

/* ---- GaborLayer.forward of the multiplicative filter network (modules/mfn.py:24-26) on native tensors ---------------
 * x [n][in <= 4], mu [out][in], gamma [out], w [out][in] (linear.weight), c [out] (linear.bias) -> out [n][out] =
 * exp(-gamma_j / 2 |x - mu_j|^2) sin(x . w_j + c_j).  The backward takes g_out [n][out] and writes g_mu, g_gamma, g_w,
 * g_c and, when g_x is not NULL, g_x [n][in]; deterministic (per-block partials reduced in a fixed order in ws,
 * wire_mfn_filter_ws_bytes(n, out) bytes).                                                                          */
int wire_mfn_filter_fwd(void* stream, const float* x, const float* mu, const float* gamma, const float* w, const float* c,
                        int64_t n, int in_features, int out_features, float* out);
int64_t wire_mfn_filter_ws_bytes(int64_t n, int out_features);
int wire_mfn_filter_bwd(void* stream, const float* g_out, const float* x, const float* mu, const float* gamma,
                        const float* w, const float* c, int64_t n, int in_features, int out_features, float* g_mu,
                        float* g_gamma, float* g_w, float* g_c, float* g_x, void* ws, int64_t ws_bytes);

/* ---- positional encoding (PosEncoding.forward, modules/relu.py:62-75) ----
 * out[n][D + 2 D F]: the raw coordinates, then for each frequency i < F and dimension j < D: sin(2^i pi c_j),
 * cos(2^i pi c_j) (the product 2^i pi c_j rounded to fp32 first, as the reference's python-float x tensor is).  The
 * whole-net path (wire_mlp_fwd with posenc_freqs > 0) runs the same kernel into its padded first-layer input.   */
int wire_posenc_fwd(void* stream, const float* coords, int64_t n, int D, int F, float* out);

/* ---- layout helpers ---------------------------------------------------- */
int wire_blocked_width(int K);   /* P = roundup(2K, 64) */
/* Float offset of the stored activations out_l (n rows of P floats -- blocked planar for wire / wire2d, P = roundup(K, 64)
 * plain features for siren / gauss / relu / bspline; l = 0..hidden_layers) inside an act buffer that wire_mlp_fwd / wire_train_fwd_bwd
 * filled for n rows with save_for_bwd = 1: the per-layer activations of modules/utils.py:246-252 without re-running the
 * layers.  (With recompute_out the last hidden layer of a fused training step is not stored, except for relu; with
 * fused_rstore a sine / Gaussian / B-spline net whose training step runs the fused data-gradient chain stores no out_l below the last
 * hidden layer either (r = c lin in their place); with split_out the inner hidden layers 1 .. hidden_layers - 1 hold fp16
 * pairs, see the knob -- set these knobs to 0 to read the activations.) */
int64_t wire_act_out_offset(const wire_net_desc* d, int64_t n, int layer);
/* complex64 [n][K] (interleaved) <-> the blocked-planar rows [n][wire_blocked_width(K)] described at the top of this
 * file.  wire_c64_to_blocked writes EVERY float of dst, the pad columns with +0.0; wire_blocked_to_c64 does not read the
 * pads.  Pure copies: bit-exact both ways.  n < 0, K < 1 or a NULL pointer: WIRE_ERR_ARG before any HIP call; n == 0
 * returns WIRE_OK and touches nothing.                                                                            */
int wire_c64_to_blocked(void* stream, const void* src, int64_t n, int K, float* dst);
int wire_blocked_to_c64(void* stream, const float* src, int64_t n, int K, void* dst);

/* ---- tuning knobs ---------------------------------------------------------
 * "split_f16" (default 1; environment WIRE_SPLIT_F16; needs split_bf16 = 1 and the x3_h16 bits of the net kind): the
 *     hidden-layer GEMMs of batches of >= 4096 rows run as a TWO-way fp16 split on v_mfma_f32_16x16x32_f16
 *     (wire_gemmx2h.hip): x s = h + l with s a power of two that maps the operand tensor's max |value| to [2^14, 2^15),
 *     three partial products per fp32 product (h h + h l + l h), fp32 accumulate -- fp32-accurate (measured rms error
 *     0.64 - 0.78 x the fp32 MFMA chain's, tools/f16x2_numerics.hip) at half the matrix-core work of the 3 x bf16
 *     split.  The maxima are tracked on the device by each tensor's producer kernel (64 sharded atomicMax slots inside
 *     the act / scratch / packed buffers) and read by the consumer kernel: no host round trip.  "x2_amode" (default 2):
 *     how the forward / data-gradient GEMM reads its activation operand -- 2 = through LDS in whole 128-byte lines (8 rows
 *     per LDS-DMA instruction, bank swizzle on the source address), 1 = straight into fragment registers (16 rows x 64
 *     bytes per instruction), 0 = through LDS in such half-line pieces; bit-identical results.
 *     0 = the 3 x bf16 kernels below for every batch size.
 * "split_out" (default 1; environment WIRE_SPLIT_OUT; with split_f16): the activations out_l of the INNER hidden layers
 *     (1 <= l < hidden_layers) of a wire / wire2d / siren / gauss / bspline net are stored ALREADY SPLIT by the forward epilogue --
 *     per 4 consecutive columns the 16 bytes [h h h h | l l l l] (fp16) instead of 4 floats, scale 2^(15 - e) from the
 *     activation's a-priori bound exp(w0^2 / 4 s0^2) < 2^e (sine, Gaussian, B-spline: 1) -- and read in that form by the next
 *     layer's forward GEMM and by the weight-gradient GEMM, which then spend no vector instructions on the split.  Used
 *     when the bound is <= 16 (w0 / s0 <= 3.33), recompute_out = 1 (nothing else reads out_l) and the widths have a
 *     2 x fp16 weight-gradient shape; otherwise, and always for out_0, out_L and relu, activations stay fp32 with the
 *     maximum tracked on the device.  Inside the act buffer only: every pointer of this interface still carries fp32.
 * "split_bf16" (default 1; environment WIRE_SPLIT_BF16): every GEMM of every net
 *     kind runs on the bf16 matrix cores with each fp32 operand split exactly into
 *     three bf16 terms (6 partial products, fp32 accumulate; fp32-accurate --
 *     wire_gemmx3.hip).  0 = the fp32-MFMA kernels below.
 * "complex_3m" (default 1; used when split_bf16 = 0): wire layers use the
 *     3-multiplication complex GEMMs on the fp32 MFMA (6 real flop per complex
 *     MAC); 0 = 4-multiplication real-expanded GEMMs.
 * "x3_tall" (default 1), "x3_tn_tall" (default 0): 256-row tiles in the split-bf16
 *     NT / TN kernels.   "nt_bk" (16 | 32): K-slab depth of the fp32 4M NT kernel.
 * "x3_h16" (default 15): the v_mfma_f32_16x16x32_bf16 edition (wire_gemmx3h.hip) of the NT GEMMs at M >= 4096:
 *     bit 0 wire forward, bit 1 wire data gradient, bit 2 siren / gauss / relu / bspline, bit 3 wire2d; 0 = the 32x32x16 kernels.
 * "x3_tn16" (default 1): the weight-gradient (TN) GEMM of the split-bf16 family runs its 256 x 256-tile
 *     v_mfma_f32_16x16x32_bf16 kernel when both padded widths are multiples of 256 (up to 256 row splits); 0 = the
 *     128 x 128 kernel.
 * "recompute_out" (default 1): on the 16x16x32 kernels the backward of a wire / wire2d / siren / gauss / bspline net evaluates out = act(lin) again
 *     (same lean form, same bits) instead of reading it back: data-gradient epilogues, the fused final stage of
 *     wire_train_fwd_bwd (whose last hidden layer then does not store out at all).  0 = read the stored activations.
 * "first_sums" (default 1): wire nets on the 16x16x32 kernels -- the epilogue of the last data-gradient GEMM forms the
 *     first layer's per-tile gradient sums itself instead of storing g_u for a separate reduction pass.
 * (The LDS-DMA 32x32x16 edition of round 2, "x3_glds", left the library: tools/wire_gemmx3g.hip, harness builds only.)
 * Buffer sizes (wire_packed_floats, wire_act_bytes, wire_bwd_scratch_bytes) and the layout of packed weights do not
 * depend on the knobs: wire_pack_params writes the weight image of every family, activations are 4-byte-per-element
 * blocked rows for all of them (fp32, or the fp16 pairs of split_out).  The knobs must NOT change between a forward and the backward that consumes its activation buffer: the
 * backward re-derives from them which kernel edition produced the activations (recompute_out: the lean forward form
 * whose bits it reproduces) and whether the forward filled the max-|value| slots the 2 x fp16 kernels scale by.     */
int wire_tune_set(const char* key, int value);
int wire_tune_get(const char* key);   /* any key wire_tune_set accepts (the table: wire_amd/csrc/wire_knobs.hip) -> value; < 0 = error */

/* ---- profiling hooks (bench.py roofline) -------------------------------
 * When enabled, every launch of the hot kernels is bracketed by hipEvents on
 * the launch stream; wire_prof_read synchronises those events and returns
 * per-class totals.  Classes: 0 fwd GEMM, 1 dgrad GEMM, 2 wgrad GEMM,
 * 3 everything else.                                                       */
#define WIRE_PROF_CLASSES 4
int wire_prof_enable(int on);
int wire_prof_read(double* ms_total, int64_t* launches, double* flops_total);

#ifdef __cplusplus
}
#endif
#endif /* WIRE_HIP_H */
