// wire_misc_api.hip -- the one-launch entry points of the C ABI (include/wire_hip.h): training glue, metrics, the
// Radon transform, the combiner and first stage of the scaled B-spline nets as layer calls, layout helpers.
#include <cmath>

#include "wire_plan.h"

// ---------------------------------------------------------------------------
// training glue
// ---------------------------------------------------------------------------
extern "C" int wire_coords_from_index(void* stream, const int64_t* idx, int64_t first, int64_t n,
                                      const float* tx, int W, const float* ty, int H,
                                      const float* tz, int T, float* coords) {
  if (n < 0 || !tx || !ty || !coords || W < 1 || H < 1 || (tz && T < 1))
    return fail(WIRE_ERR_ARG, "bad argument to wire_coords_from_index");
  ProfScope ps((hipStream_t)stream, 3, 0);
  HIPCHK(launch_coords((hipStream_t)stream, idx, first, n, tx, W, ty, H, tz, T, coords));
  return WIRE_OK;
}
extern "C" int wire_perm_indices(void* stream, uint64_t seed, int64_t n_total, int64_t first, int64_t count,
                                 int64_t* idx_out) {
  if (n_total < 1 || first < 0 || count < 0 || first + count > n_total || (count > 0 && !idx_out))
    return fail(WIRE_ERR_ARG, "bad argument to wire_perm_indices");
  ProfScope ps((hipStream_t)stream, 3, 0);
  HIPCHK(launch_perm_indices((hipStream_t)stream, seed, n_total, first, count, idx_out));
  return WIRE_OK;
}
extern "C" int wire_mse_grad(void* stream, const float* y, const float* target, const int64_t* idx,
                             int64_t first, int64_t n, int O, float weight, float* g_y,
                             float* loss_out, float* rec, float* partial) {
  if (n < 0 || O < 1 || !y || !target || !g_y || !loss_out || !partial)
    return fail(WIRE_ERR_ARG, "bad argument to wire_mse_grad");
  ProfScope ps((hipStream_t)stream, 3, 0);
  HIPCHK(launch_mse_grad((hipStream_t)stream, y, target, idx, first, n, O, weight, g_y, loss_out,
                         rec, partial));
  return WIRE_OK;
}
extern "C" int wire_avgpool_mse_grad(void* stream, const float* y, int H, int W, int O, int scale,
                                     const float* gt_lr, float* g_y, float* rec_lr, float* loss_out,
                                     float* partial) {
  if (H < 1 || W < 1 || O < 1 || scale < 1 || scale > H || scale > W || !y || !gt_lr || !g_y || !loss_out || !partial)
    return fail(WIRE_ERR_ARG, "bad argument to wire_avgpool_mse_grad");
  ProfScope ps((hipStream_t)stream, 3, 0);
  HIPCHK(launch_avgpool_mse_grad((hipStream_t)stream, y, H, W, O, scale, gt_lr, g_y, rec_lr, loss_out, partial));
  return WIRE_OK;
}
extern "C" int wire_avgpool_mse_grad_frames(void* stream, const float* y, int B, int H, int W, int O, int scale,
                                            const float* gt_lr, const float* mask, float* g_y, float* rec_lr,
                                            float* loss_out, float* partial) {
  if (B < 1 || H < 1 || W < 1 || O < 1 || scale < 1 || scale > H || scale > W || !y || !gt_lr || !g_y || !loss_out ||
      !partial)
    return fail(WIRE_ERR_ARG, "bad argument to wire_avgpool_mse_grad_frames");
  ProfScope ps((hipStream_t)stream, 3, 0);
  HIPCHK(launch_avgpool_mse_grad_frames((hipStream_t)stream, y, B, H, W, O, scale, gt_lr, mask, g_y, rec_lr, loss_out,
                                        partial));
  return WIRE_OK;
}
extern "C" int wire_coded_mse_grad(void* stream, const float* y, int64_t p0, int64_t n_pix, int64_t NP, int T, int O,
                                   int nframes, int dup_last, const float* mask, const float* gt, float* g_y,
                                   float* est, float* loss_out, float* partial) {
  if (T < 1 || O < 1 || nframes < 1 || n_pix < 1 || NP < 1 || p0 < 0 || n_pix > NP || p0 > NP - n_pix ||
      (dup_last != 0 && dup_last != 1) || !y || !mask || !gt || !g_y || !loss_out || !partial)
    return fail(WIRE_ERR_ARG, "bad argument to wire_coded_mse_grad");
  ProfScope ps((hipStream_t)stream, 3, 0);
  HIPCHK(launch_coded_mse_grad((hipStream_t)stream, y, p0, n_pix, NP, T, O, nframes, dup_last, mask, gt, g_y, est,
                               loss_out, partial));
  return WIRE_OK;
}
// (one thread per value in a 1-D grid of 256-thread blocks)
static bool coded_shape_ok(int T, int64_t NP, int nframes, int dup_last) {
  return T >= 1 && NP >= 1 && nframes >= 1 && (dup_last == 0 || dup_last == 1) &&
         NP <= ((int64_t)0x7fffffff * 256) / ((int64_t)T + 1);
}
extern "C" int wire_coded_fwd(void* stream, const float* video, const float* masks, int T, int64_t NP, int nframes,
                              int dup_last, float* coded) {
  if (!coded_shape_ok(T, NP, nframes, dup_last) || !video || !masks || !coded)
    return fail(WIRE_ERR_ARG, "bad argument to wire_coded_fwd");
  ProfScope ps((hipStream_t)stream, 3, 0);
  HIPCHK(launch_coded_fwd((hipStream_t)stream, video, masks, T, NP, nframes, dup_last, coded));
  return WIRE_OK;
}
extern "C" int wire_coded_bwd(void* stream, const float* g_coded, const float* masks, int T, int64_t NP, int nframes,
                              int dup_last, float* g_video) {
  if (!coded_shape_ok(T, NP, nframes, dup_last) || !g_coded || !masks || !g_video)
    return fail(WIRE_ERR_ARG, "bad argument to wire_coded_bwd");
  ProfScope ps((hipStream_t)stream, 3, 0);
  HIPCHK(launch_coded_bwd((hipStream_t)stream, g_coded, masks, T, NP, nframes, dup_last, g_video));
  return WIRE_OK;
}
extern "C" int wire_affine_coords(void* stream, const double* mats, int B, int H, int W, float* coords) {
  if (B < 1 || H < 1 || W < 1 || !mats || !coords) return fail(WIRE_ERR_ARG, "bad argument to wire_affine_coords");
  ProfScope ps((hipStream_t)stream, 3, 0);
  HIPCHK(launch_affine_coords((hipStream_t)stream, mats, B, H, W, coords));
  return WIRE_OK;
}
extern "C" int wire_adam_step_flat(void* stream, float* param, const float* grad, float* exp_avg,
                                   float* exp_avg_sq, int64_t count, float lr, float beta1,
                                   float beta2, float eps, int64_t step) {
  if (count < 0 || step < 1 || !param || !grad || !exp_avg || !exp_avg_sq)
    return fail(WIRE_ERR_ARG, "bad argument to wire_adam_step_flat");
  const double bc1 = 1.0 - std::pow((double)beta1, (double)step);
  const double bc2 = 1.0 - std::pow((double)beta2, (double)step);
  ProfScope ps((hipStream_t)stream, 3, 0);
  HIPCHK(launch_adam((hipStream_t)stream, param, grad, exp_avg, exp_avg_sq, count,
                     (float)((double)lr / bc1), beta1, beta2, eps, (float)(1.0 / std::sqrt(bc2))));
  return WIRE_OK;
}

extern "C" int wire_eval_metric(void* stream, int mode, const float* rec, const float* gt, int64_t count,
                                float thres, float* out2, float* partial) {
  if ((mode != 0 && mode != 1) || count < 1 || !rec || !gt || !out2 || !partial)
    return fail(WIRE_ERR_ARG, "bad argument to wire_eval_metric");
  ProfScope ps((hipStream_t)stream, 3, 0);
  HIPCHK(launch_metric((hipStream_t)stream, mode, rec, gt, count, thres, out2, partial));
  return WIRE_OK;
}

static bool ssim_shape_ok(int H, int W, int O, int taps) {
  return taps >= 3 && taps <= SSIM_MAX_TAPS && (taps & 1) && H >= taps && W >= taps && O >= 1 && O <= WIRE_MAXO &&
         ssim_tiles(H, W, taps) <= 0x7fffffff;
}
extern "C" int64_t wire_ssim_ws_bytes(int H, int W, int O, int taps) {
  if (!ssim_shape_ok(H, W, O, taps)) return fail(WIRE_ERR_ARG, "bad argument to wire_ssim_ws_bytes");
  return ssim_tiles(H, W, taps) * 4 + 256;
}
extern "C" int wire_ssim(void* stream, const float* x, const float* y, int H, int W, int O, int taps,
                         const float* window_host, float cov_norm, float c1, float c2, float* out1, float* map, void* ws,
                         int64_t ws_bytes) {
  if (!ssim_shape_ok(H, W, O, taps) || !x || !y || !window_host || !out1 || !ws || !std::isfinite(cov_norm) ||
      !std::isfinite(c1) || !std::isfinite(c2))
    return fail(WIRE_ERR_ARG, "bad argument to wire_ssim");
  if (ws_bytes < wire_ssim_ws_bytes(H, W, O, taps)) return fail(WIRE_ERR_SIZE, "ws too small");
  SsimWin win{};
  for (int t = 0; t < taps; ++t) win.w[t] = window_host[t];
  ProfScope ps((hipStream_t)stream, 3, 0);
  HIPCHK(launch_ssim((hipStream_t)stream, x, y, H, W, O, taps, win, cov_norm, c1, c2, out1, map, (float*)ws));
  return WIRE_OK;
}

static bool ssim_grad_shape_ok(int H, int W, int O, int taps) {
  return ssim_shape_ok(H, W, O, taps) && ssim_bwd_tiles(H, W) <= 0x3fffffff;
}
extern "C" int64_t wire_ssim_bwd_ws_bytes(int H, int W, int O, int taps) {
  if (!ssim_grad_shape_ok(H, W, O, taps)) return fail(WIRE_ERR_ARG, "bad argument to wire_ssim_bwd_ws_bytes");
  return 256;        // the tiles keep every intermediate in LDS; the argument stays for a tiling that does not
}
extern "C" int wire_ssim_bwd(void* stream, const float* x, const float* y, int H, int W, int O, int taps,
                             const float* window_host, float cov_norm, float c1, float c2, const float* g_ssim,
                             float* g_y, void* ws, int64_t ws_bytes) {
  if (!ssim_grad_shape_ok(H, W, O, taps) || !x || !y || !window_host || !g_ssim || !g_y || !ws ||
      !std::isfinite(cov_norm) || !std::isfinite(c1) || !std::isfinite(c2))
    return fail(WIRE_ERR_ARG, "bad argument to wire_ssim_bwd");
  if (ws_bytes < wire_ssim_bwd_ws_bytes(H, W, O, taps)) return fail(WIRE_ERR_SIZE, "ws too small");
  SsimWin win{};
  for (int t = 0; t < taps; ++t) win.w[t] = window_host[t];
  ProfScope ps((hipStream_t)stream, 3, 0);
  HIPCHK(launch_ssim_bwd((hipStream_t)stream, x, y, H, W, O, taps, win, cov_norm, c1, c2, g_ssim, g_y));
  return WIRE_OK;
}
extern "C" int64_t wire_ssim_mse_grad_ws_bytes(int H, int W, int O, int taps) {
  if (!ssim_grad_shape_ok(H, W, O, taps)) return fail(WIRE_ERR_ARG, "bad argument to wire_ssim_mse_grad_ws_bytes");
  return ssim_loss_partials(H, W) * 4 + 256;
}
extern "C" int wire_ssim_mse_grad(void* stream, const float* y, int H, int W, int O, const float* target, int taps,
                                  const float* window_host, float cov_norm, float c1, float c2, const int64_t* idx,
                                  int64_t first, int64_t n_mse, float lambda_ssim, float* g_y, float* loss_out,
                                  float* rec, void* ws, int64_t ws_bytes) {
  const int64_t npix = (int64_t)H * W;
  if (!ssim_grad_shape_ok(H, W, O, taps) || n_mse < 0 || n_mse > npix ||
      (!idx && (first < 0 || first > npix - n_mse)) || !y || !target || !window_host || !g_y || !loss_out || !ws ||
      !std::isfinite(cov_norm) || !std::isfinite(c1) || !std::isfinite(c2) || !std::isfinite(lambda_ssim))
    return fail(WIRE_ERR_ARG, "bad argument to wire_ssim_mse_grad");
  if (ws_bytes < wire_ssim_mse_grad_ws_bytes(H, W, O, taps)) return fail(WIRE_ERR_SIZE, "ws too small");
  SsimWin win{};
  for (int t = 0; t < taps; ++t) win.w[t] = window_host[t];
  ProfScope ps((hipStream_t)stream, 3, 0);
  HIPCHK(launch_ssim_mse_grad((hipStream_t)stream, y, H, W, O, target, taps, win, cov_norm, c1, c2, idx, first, n_mse,
                              lambda_ssim, g_y, loss_out, rec, (float*)ws));
  return WIRE_OK;
}

extern "C" int wire_track_best(void* stream, const float* metric, float* best_metric, int force, const float* src,
                               float* dst, int64_t count, int* updated) {
  if (!metric || !best_metric || count < 0 || (count > 0 && (!src || !dst)))
    return fail(WIRE_ERR_ARG, "bad argument to wire_track_best");
  if (count > 0 && (((uintptr_t)src | (uintptr_t)dst) & 15)) return fail(WIRE_ERR_ARG, "src / dst must be 16-byte aligned");
  ProfScope ps((hipStream_t)stream, 3, 0);
  HIPCHK(launch_track_best((hipStream_t)stream, metric, best_metric, force, src, dst, count, updated));
  return WIRE_OK;
}
extern "C" int wire_radon_fwd(void* stream, const float* img, const float* angles_deg, int H, int W, int nangles,
                              float* sino) {
  if (H < 1 || W < 1 || nangles < 1 || !img || !angles_deg || !sino) return fail(WIRE_ERR_ARG, "bad argument to wire_radon_fwd");
  ProfScope ps((hipStream_t)stream, 3, 0);
  HIPCHK(launch_radon_fwd((hipStream_t)stream, img, angles_deg, H, W, nangles, sino));
  return WIRE_OK;
}
extern "C" int wire_radon_bwd(void* stream, const float* g_sino, const float* angles_deg, int H, int W, int nangles,
                              float* g_img) {
  if (H < 1 || W < 1 || nangles < 1 || !g_sino || !angles_deg || !g_img) return fail(WIRE_ERR_ARG, "bad argument to wire_radon_bwd");
  ProfScope ps((hipStream_t)stream, 3, 0);
  HIPCHK(launch_radon_bwd((hipStream_t)stream, g_sino, angles_deg, H, W, nangles, g_img));
  return WIRE_OK;
}
extern "C" int wire_mscale_first_fwd(void* stream, const float* x, const float* W, const float* b, int64_t n,
                                     int in_features, int out_features, int nscales, const float* scales_host, float* out) {
  if (n < 0 || in_features < 1 || in_features > 4 || (n > 0 && (!x || !W || !b || !out)) || !scales_host)
    return fail(WIRE_ERR_ARG, "bad argument to wire_mscale_first_fwd");
  // the descriptor's checks of the first stage (make_plan), on a net around it
  wire_net_desc_ms m{};
  m.base.kind = WIRE_KIND_BSPLINE_MS; m.base.in_features = in_features; m.base.width = 1; m.base.out_features = 1;
  m.base.scale0 = 1.f; m.first_width = out_features; m.nscales = nscales;
  if (nscales >= 2 && nscales <= WIRE_MS_MAX_SCALES)
    for (int g = 0; g < nscales; ++g) m.scales[g] = scales_host[g];
  Plan p; if (int rc = make_plan(&m.base, p)) return rc;
  MscaleC c{};
  for (int g = 0; g < p.T; ++g) c.c[g] = p.sc_c[g];
  HIPCHK(launch_mscale_first((hipStream_t)stream, x, n, in_features, W, b, p.SHF, c, p.ms_split, p.SHF, 0.f, nullptr, out));
  return WIRE_OK;
}
static bool m2_shape_ok(int S, int O) { return S >= 1 && S <= WIRE_MS_MAX_SCALES && O >= 1 && O <= 8; }
extern "C" int wire_m2_combine_fwd(void* stream, int nscales, int out_features, const float* W1, const float* b1,
                                   const float* W2, const float* b2, const float* t, int64_t n, float* y) {
  if (!m2_shape_ok(nscales, out_features) || n < 0 || !W1 || !b1 || !W2 || !b2 || (n > 0 && (!t || !y)))
    return fail(WIRE_ERR_ARG, "bad argument to wire_m2_combine_fwd");
  ProfScope ps((hipStream_t)stream, 3, 0);
  HIPCHK(launch_m2_comb_fwd((hipStream_t)stream, M2Comb{W1, b1, W2, b2}, nscales, out_features, t, n, y));
  return WIRE_OK;
}
extern "C" int64_t wire_m2_combine_ws_bytes(int nscales, int out_features, int64_t n) {
  if (!m2_shape_ok(nscales, out_features) || n < 0) return fail(WIRE_ERR_ARG, "bad argument to wire_m2_combine_ws_bytes");
  return (int64_t)m2_comb_blocks(n) * m2_comb_grad_floats(nscales, out_features) * 4 + 256;
}
extern "C" int wire_m2_combine_bwd(void* stream, int nscales, int out_features, const float* W1, const float* b1,
                                   const float* W2, const float* b2, const float* t, int64_t n, const float* g_y,
                                   float* g_t, float* gW1, float* gb1, float* gW2, float* gb2, void* ws,
                                   int64_t ws_bytes) {
  if (!m2_shape_ok(nscales, out_features) || n < 1 || !W1 || !b1 || !W2 || !b2 || !t || !g_y || !g_t || !gW1 || !gb1 ||
      !gW2 || !gb2 || !ws)
    return fail(WIRE_ERR_ARG, "bad argument to wire_m2_combine_bwd");
  if (ws_bytes < wire_m2_combine_ws_bytes(nscales, out_features, n)) return fail(WIRE_ERR_SIZE, "ws too small");
  hipStream_t s = (hipStream_t)stream;
  ProfScope ps(s, 3, 0);
  const M2Comb w{W1, b1, W2, b2};
  HIPCHK(launch_m2_comb_bwd(s, w, nscales, out_features, t, n, M2Loss{}, g_y, g_t, (float*)ws, nullptr));
  HIPCHK(launch_m2_comb_reduce(s, (const float*)ws, n, nscales, out_features, M2Grads{gW1, gb1, gW2, gb2}));
  return WIRE_OK;
}
extern "C" int wire_posenc_fwd(void* stream, const float* coords, int64_t n, int D, int F, float* out) {
  if (n < 0 || D < 1 || D > 4 || F < 0 || F > 30 || (n > 0 && (!coords || !out)))
    return fail(WIRE_ERR_ARG, "bad argument to wire_posenc_fwd");
  HIPCHK(launch_posenc((hipStream_t)stream, coords, n, D, F, D + 2 * D * F, out));
  return WIRE_OK;
}
extern "C" int wire_posenc_bwd(void* stream, const float* coords, int64_t n, int D, int F, const float* g_pe,
                               float* g_coords) {
  if (n < 0 || D < 1 || D > 4 || F < 0 || F > 30 || (n > 0 && (!coords || !g_pe || !g_coords)))
    return fail(WIRE_ERR_ARG, "bad argument to wire_posenc_bwd");
  ProfScope ps((hipStream_t)stream, 3, 0);
  HIPCHK(launch_posenc_bwd((hipStream_t)stream, coords, n, D, F, g_pe, D + 2 * D * F, g_coords));
  return WIRE_OK;
}
extern "C" int wire_sigmoid_inplace(void* stream, float* x, int64_t count) {
  if (count < 0 || (count > 0 && !x)) return fail(WIRE_ERR_ARG, "bad argument to wire_sigmoid_inplace");
  HIPCHK(launch_sigmoid((hipStream_t)stream, x, count));
  return WIRE_OK;
}

// ---------------------------------------------------------------------------
// layout helpers
// ---------------------------------------------------------------------------
extern "C" int wire_c64_to_blocked(void* stream, const void* src, int64_t n, int K, float* dst) {
  if (n < 0 || K < 1 || !src || !dst) return fail(WIRE_ERR_ARG, "bad argument");
  HIPCHK(launch_c64_to_blocked((hipStream_t)stream, (const float*)src, n, K, rup(2 * K, 64), dst));
  return WIRE_OK;
}
extern "C" int wire_blocked_to_c64(void* stream, const float* src, int64_t n, int K, void* dst) {
  if (n < 0 || K < 1 || !src || !dst) return fail(WIRE_ERR_ARG, "bad argument");
  HIPCHK(launch_blocked_to_c64((hipStream_t)stream, src, n, K, rup(2 * K, 64), (float*)dst));
  return WIRE_OK;
}
