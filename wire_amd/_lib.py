"""ctypes binding of libwire_hip.so (include/wire_hip.h).

The product path has no CPU or PyTorch-op fallback: if the HIP library is not
built, ``lib()`` raises.  Build it with ``python -c "import __graft_entry__ as
g; g.build()"`` or ``make -C wire_amd/csrc``.
"""
from __future__ import annotations

import ctypes as C
import os
from typing import Optional

# torch must load ITS HIP runtime (torch/lib/libamdhip64.so) before this library
# pulls one in by SONAME: two runtimes in one process see no device.
import torch  # noqa: F401

_HERE = os.path.dirname(os.path.abspath(__file__))
LIB_PATH = os.path.join(_HERE, "lib", "libwire_hip.so")

KIND = {"wire": 0, "wire2d": 1, "siren": 2, "gauss": 3, "relu": 4, "bspline_form": 5, "bspline_mscale_HL": 6,
        "bspline_mscale_2": 8, "bspline_mscale_hier": 9, "mfn": 11, "bspline_cubic": 12}
MS_MAX_SCALES = 8   # WIRE_MS_MAX_SCALES
ABI_VERSION = 1
# enum wire_loss_kind: the data terms of wire_point_loss_grad
LOSS_KIND = {"mse": 0, "l1": 1, "huber": 2, "logistic": 3}
# the motion models of wire_register_gn_step (cv2's MOTION_TRANSLATION / MOTION_EUCLIDEAN / MOTION_AFFINE integers)
MOTION_MODEL = {"translation": 0, "euclidean": 1, "affine": 2}
# enum wire_resize_mode: cv2's INTER_NEAREST / INTER_LINEAR / INTER_CUBIC / INTER_AREA integers
RESIZE_MODE = {"nearest": 0, "linear": 1, "cubic": 2, "area": 3}
# the density modes of wire_composite_fwd / _bwd / _mse_grad / _weights
DENSITY_MODE = {"softplus": 0, "relu": 1}
REG_NSUM = 29      # the sums wire_register_gn_step leaves at the start of its workspace, per (frame, candidate)

# every symbol include/wire_hip.h declares (tests check the .so exports them)
SYMBOLS = [
    "wire_abi_version", "wire_last_error", "wire_num_param_tensors",
    "wire_param_tensor_floats", "wire_packed_floats", "wire_act_bytes",
    "wire_bwd_scratch_bytes", "wire_pack_params", "wire_mlp_fwd", "wire_mlp_bwd",
    "wire_layer_ws_bytes", "wire_gabor_fwd", "wire_gabor_bwd", "wire_final_fwd",
    "wire_final_bwd", "wire_coords_from_index", "wire_mse_grad",
    "wire_adam_step_flat", "wire_blocked_width", "wire_c64_to_blocked",
    "wire_blocked_to_c64", "wire_prof_enable", "wire_prof_read", "wire_tune_set", "wire_tune_get", "wire_avgpool_mse_grad", "wire_layer2d_ws_bytes", "wire_gabor2d_fwd", "wire_gabor2d_bwd", "wire_eval_metric", "wire_real_layer_fwd", "wire_real_layer_bwd", "wire_train_fwd_bwd", "wire_perm_indices", "wire_gabor_hparam_grad", "wire_track_best", "wire_sigmoid_inplace", "wire_radon_fwd", "wire_radon_bwd", "wire_gabor2d_hparam_grad", "wire_posenc_fwd", "wire_act_out_offset", "wire_train_fwd_bwd_hooked",
    "wire_bwd_coords_scratch_bytes", "wire_mlp_bwd_coords", "wire_posenc_bwd", "wire_gabor_bwd_first_coords",
    "wire_gabor2d_bwd_first_coords", "wire_mscale_first_fwd", "wire_m2_combine_fwd", "wire_m2_combine_ws_bytes",
    "wire_m2_combine_bwd", "wire_mfn_filter_fwd", "wire_mfn_filter_ws_bytes", "wire_mfn_filter_bwd",
    "wire_avgpool_mse_grad_frames", "wire_affine_coords", "wire_ssim_ws_bytes", "wire_ssim",
    "wire_coded_mse_grad", "wire_coded_fwd", "wire_coded_bwd", "wire_tv_fwd", "wire_tv_bwd", "wire_tv_mse_grad",
    "wire_ssim_bwd_ws_bytes", "wire_ssim_bwd", "wire_ssim_mse_grad_ws_bytes", "wire_ssim_mse_grad",
    "wire_tv_add_grad", "wire_warp_coords_fwd", "wire_warp_coords_bwd_ws_bytes", "wire_warp_coords_bwd",
    "wire_iso_ws_bytes", "wire_iso_count", "wire_iso_emit", "wire_iso_tet_case", "wire_gauss3_blur",
    "wire_radon_vol_fwd", "wire_radon_vol_bwd", "wire_point_loss_grad",
    "wire_remap_bilinear_fwd", "wire_remap_bilinear_bwd_xy", "wire_register_gn_ws_bytes", "wire_register_gn_step",
    "wire_resize_tab_bytes", "wire_resize_mse_grad_ws_bytes", "wire_resize_tables", "wire_resize_fwd", "wire_resize_bwd",
    "wire_resize_mse_grad",
    "wire_ray_samples", "wire_composite_fwd", "wire_composite_bwd", "wire_composite_mse_grad",
    "wire_composite_weights", "wire_ray_resample",
]


class NetDesc(C.Structure):
    """struct wire_net_desc"""
    _fields_ = [("kind", C.c_int32), ("in_features", C.c_int32), ("width", C.c_int32),
                ("hidden_layers", C.c_int32), ("out_features", C.c_int32),
                ("posenc_freqs", C.c_int32), ("first_omega0", C.c_float),
                ("hidden_omega0", C.c_float), ("scale0", C.c_float)]


class NetDescMS(C.Structure):
    """struct wire_net_desc_ms: the scaled B-spline nets' descriptor (kinds 6, 8, 9).  The library takes a pointer to its
    ``base`` member; ``make_desc_scaled`` returns that member, which keeps this struct alive and lies at its start."""
    _fields_ = [("base", NetDesc), ("first_width", C.c_int32), ("nscales", C.c_int32),
                ("scales", C.c_float * MS_MAX_SCALES)]


# wire_grad_ready_fn (include/wire_hip.h): void (*)(void* user, int first_tensor, int n_tensors)
GRAD_READY_FN = C.CFUNCTYPE(None, C.c_void_p, C.c_int, C.c_int)


class WireHipError(RuntimeError):
    pass


_lib: Optional[C.CDLL] = None


def _declare(l: C.CDLL) -> None:
    vp, i64, i32, f32 = C.c_void_p, C.c_int64, C.c_int, C.c_float
    dp = C.POINTER(NetDesc)
    l.wire_abi_version.restype = i32
    l.wire_last_error.restype = C.c_char_p
    l.wire_num_param_tensors.argtypes = [dp]
    l.wire_param_tensor_floats.argtypes = [dp, i32]
    l.wire_param_tensor_floats.restype = i64
    l.wire_packed_floats.argtypes = [dp]
    l.wire_packed_floats.restype = i64
    l.wire_act_bytes.argtypes = [dp, i64, i32]
    l.wire_act_bytes.restype = i64
    l.wire_bwd_scratch_bytes.argtypes = [dp, i64]
    l.wire_bwd_scratch_bytes.restype = i64
    l.wire_pack_params.argtypes = [vp, dp, C.POINTER(vp), vp]
    l.wire_mlp_fwd.argtypes = [vp, dp, vp, vp, i64, vp, vp, i64, i32]
    l.wire_mlp_bwd.argtypes = [vp, dp, vp, vp, i64, vp, vp, i64, vp, i64, C.POINTER(vp)]
    l.wire_layer_ws_bytes.argtypes = [i64, i32, i32]
    l.wire_layer_ws_bytes.restype = i64
    l.wire_gabor_fwd.argtypes = [vp, vp, vp, vp, f32, f32, i64, i32, i32, i32, vp, vp, vp, i64]
    l.wire_gabor_bwd.argtypes = [vp, vp, vp, vp, vp, f32, f32, i64, i32, i32, i32, vp, vp, vp, vp, i64]
    l.wire_gabor_hparam_grad.argtypes = [vp, vp, vp, vp, vp, f32, f32, i64, i32, i32, i32, vp, vp, i64]
    l.wire_track_best.argtypes = [vp, vp, vp, i32, vp, vp, i64, vp]
    l.wire_sigmoid_inplace.argtypes = [vp, vp, i64]
    l.wire_posenc_fwd.argtypes = [vp, vp, i64, i32, i32, vp]
    l.wire_mscale_first_fwd.argtypes = [vp, vp, vp, vp, i64, i32, i32, i32, C.POINTER(C.c_float), vp]
    l.wire_m2_combine_fwd.argtypes = [vp, i32, i32, vp, vp, vp, vp, vp, i64, vp]
    l.wire_m2_combine_ws_bytes.argtypes = [i32, i32, i64]
    l.wire_m2_combine_ws_bytes.restype = i64
    l.wire_m2_combine_bwd.argtypes = [vp, i32, i32, vp, vp, vp, vp, vp, i64, vp, vp, vp, vp, vp, vp, vp, i64]
    l.wire_mfn_filter_fwd.argtypes = [vp, vp, vp, vp, vp, vp, i64, i32, i32, vp]
    l.wire_mfn_filter_ws_bytes.argtypes = [i64, i32]
    l.wire_mfn_filter_ws_bytes.restype = i64
    l.wire_mfn_filter_bwd.argtypes = [vp, vp, vp, vp, vp, vp, vp, i64, i32, i32, vp, vp, vp, vp, vp, vp, i64]
    l.wire_bwd_coords_scratch_bytes.argtypes = [dp, i64]
    l.wire_bwd_coords_scratch_bytes.restype = i64
    l.wire_mlp_bwd_coords.argtypes = [vp, dp, vp, vp, i64, vp, vp, i64, vp, i64, C.POINTER(vp), vp]
    l.wire_posenc_bwd.argtypes = [vp, vp, i64, i32, i32, vp, vp]
    l.wire_gabor_bwd_first_coords.argtypes = [vp, vp, vp, vp, vp, f32, f32, i64, i32, i32, vp, vp, vp, vp, i64]
    l.wire_gabor2d_bwd_first_coords.argtypes = [vp, vp, vp, vp, vp, vp, vp, f32, f32, i64, i32, i32, vp, vp, vp, vp, vp,
                                                vp, i64]
    l.wire_act_out_offset.argtypes = [dp, i64, i32]
    l.wire_act_out_offset.restype = i64
    l.wire_radon_fwd.argtypes = [vp, vp, vp, i32, i32, i32, vp]
    l.wire_radon_bwd.argtypes = [vp, vp, vp, i32, i32, i32, vp]
    l.wire_radon_vol_fwd.argtypes = [vp, vp, vp, i32, i32, i32, i32, vp]
    l.wire_radon_vol_bwd.argtypes = [vp, vp, vp, i32, i32, i32, i32, vp]
    l.wire_final_fwd.argtypes = [vp, vp, vp, vp, i64, i32, i32, vp, vp, i64]
    l.wire_final_bwd.argtypes = [vp, vp, vp, vp, i64, i32, i32, vp, vp, vp, vp, i64]
    l.wire_coords_from_index.argtypes = [vp, vp, i64, i64, vp, i32, vp, i32, vp, i32, vp]
    l.wire_perm_indices.argtypes = [vp, C.c_uint64, i64, i64, i64, vp]
    l.wire_mse_grad.argtypes = [vp, vp, vp, vp, i64, i64, i32, f32, vp, vp, vp, vp]
    l.wire_point_loss_grad.argtypes = [vp, i32, f32, vp, vp, vp, i32, vp, i64, i64, i32, f32, vp, vp, vp, vp]
    l.wire_adam_step_flat.argtypes = [vp, vp, vp, vp, vp, i64, f32, f32, f32, f32, i64]
    l.wire_blocked_width.argtypes = [i32]
    l.wire_c64_to_blocked.argtypes = [vp, vp, i64, i32, vp]
    l.wire_blocked_to_c64.argtypes = [vp, vp, i64, i32, vp]
    l.wire_tune_set.argtypes = [C.c_char_p, i32]
    l.wire_tune_get.argtypes = [C.c_char_p]
    l.wire_layer2d_ws_bytes.argtypes = [i64, i32, i32]
    l.wire_layer2d_ws_bytes.restype = i64
    l.wire_gabor2d_fwd.argtypes = [vp, vp, vp, vp, vp, vp, f32, f32, i64, i32, i32, i32, vp, vp, i64]
    l.wire_gabor2d_bwd.argtypes = [vp, vp, vp, vp, vp, vp, vp, f32, f32, i64, i32, i32, i32, vp, vp, vp, vp, vp,
                                   vp, i64]
    l.wire_gabor2d_hparam_grad.argtypes = [vp, vp, vp, vp, vp, vp, vp, f32, f32, i64, i32, i32, i32, vp, vp, i64]
    l.wire_avgpool_mse_grad.argtypes = [vp, vp, i32, i32, i32, i32, vp, vp, vp, vp, vp]
    l.wire_avgpool_mse_grad_frames.argtypes = [vp, vp, i32, i32, i32, i32, i32, vp, vp, vp, vp, vp, vp]
    l.wire_affine_coords.argtypes = [vp, vp, i32, i32, i32, vp]
    l.wire_coded_mse_grad.argtypes = [vp, vp, i64, i64, i64, i32, i32, i32, i32, vp, vp, vp, vp, vp, vp]
    l.wire_coded_fwd.argtypes = [vp, vp, vp, i32, i64, i32, i32, vp]
    l.wire_coded_bwd.argtypes = [vp, vp, vp, i32, i64, i32, i32, vp]
    l.wire_tv_fwd.argtypes = [vp, vp, i32, i32, i32, i64, i64, vp, vp]
    l.wire_tv_bwd.argtypes = [vp, vp, i32, i32, i32, i64, i64, vp, vp]
    l.wire_tv_mse_grad.argtypes = [vp, vp, i32, i32, i32, vp, vp, i64, i64, f32, vp, vp, vp, vp]
    l.wire_tv_add_grad.argtypes = [vp, vp, i32, i32, i32, i32, f32, f32, vp, vp, vp, vp]
    l.wire_warp_coords_fwd.argtypes = [vp, vp, vp, i32, i64, vp]
    l.wire_warp_coords_bwd_ws_bytes.argtypes = [i32, i64]
    l.wire_warp_coords_bwd_ws_bytes.restype = i64
    l.wire_warp_coords_bwd.argtypes = [vp, vp, vp, vp, i32, i64, i32, vp, vp, vp, i64]
    l.wire_remap_bilinear_fwd.argtypes = [vp, vp, i32, i32, i32, vp, i64, i32, vp]
    l.wire_remap_bilinear_bwd_xy.argtypes = [vp, vp, i32, i32, i32, vp, vp, i64, i32, vp]
    l.wire_register_gn_ws_bytes.argtypes = [i32, i32, i32, i32]
    l.wire_register_gn_ws_bytes.restype = i64
    l.wire_register_gn_step.argtypes = [vp, vp, vp, vp, i32, i32, i32, i32, i32, C.c_double, C.c_double, vp, vp, vp, i64]
    geom = [i32, i32, i32, i32, i32, C.c_double, C.c_double]          # H, W, Hl, Wl, mode, sy, sx
    l.wire_resize_tab_bytes.argtypes = geom
    l.wire_resize_tab_bytes.restype = i64
    l.wire_resize_mse_grad_ws_bytes.argtypes = [i32, i32, i32]
    l.wire_resize_mse_grad_ws_bytes.restype = i64
    l.wire_resize_tables.argtypes = [vp] + geom + [vp]
    l.wire_resize_fwd.argtypes = [vp, vp] + geom + [vp, i32, vp]
    l.wire_resize_bwd.argtypes = [vp, vp] + geom + [vp, i32, vp]
    l.wire_resize_mse_grad.argtypes = [vp, vp] + geom + [vp, i32, vp, vp, vp, vp, vp, i64, vp]
    l.wire_ray_samples.argtypes = [vp, vp, vp, f32, f32, vp, i64, i32, vp, vp, vp]
    l.wire_composite_fwd.argtypes = [vp, vp, vp, vp, vp, i64, i32, i32, i32, vp, vp, vp]
    l.wire_composite_bwd.argtypes = [vp, vp, vp, vp, vp, vp, vp, vp, i64, i32, i32, i32, vp]
    l.wire_composite_mse_grad.argtypes = [vp, vp, vp, vp, vp, vp, i64, i32, i32, i32, f32, vp, vp, vp, vp]
    l.wire_composite_weights.argtypes = [vp, vp, vp, i64, i32, i32, i32, vp]
    l.wire_ray_resample.argtypes = [vp, vp, vp, f32, f32, vp, vp, vp, f32, i64, i32, i32, vp, vp, vp]
    l.wire_iso_ws_bytes.argtypes = [i32, i32, i32]
    l.wire_iso_ws_bytes.restype = i64
    l.wire_iso_count.argtypes = [vp, vp, i32, i32, i32, f32, vp, vp]
    l.wire_iso_emit.argtypes = [vp, vp, i32, i32, i32, f32, vp, vp, i64, vp, i64]
    l.wire_iso_tet_case.argtypes = [i32, i32]
    l.wire_gauss3_blur.argtypes = [vp, vp, i32, i32, i32, f32, vp, vp]
    l.wire_train_fwd_bwd.argtypes = [vp, dp, vp, vp, i64, vp, vp, i64, f32, vp, vp, vp, vp, vp, vp, i64, vp, i64,
                                     C.POINTER(vp)]
    l.wire_train_fwd_bwd_hooked.argtypes = [vp, dp, vp, vp, i64, vp, vp, i64, f32, vp, vp, vp, vp, vp, vp, i64, vp, i64,
                                            C.POINTER(vp), GRAD_READY_FN, vp]
    l.wire_real_layer_fwd.argtypes = [vp, i32, vp, vp, vp, f32, f32, i64, i32, i32, vp, vp, i64]
    l.wire_real_layer_bwd.argtypes = [vp, i32, vp, vp, vp, vp, f32, f32, i64, i32, i32, vp, vp, vp, vp, i64]
    l.wire_eval_metric.argtypes = [vp, i32, vp, vp, i64, f32, vp, vp]
    l.wire_ssim_ws_bytes.argtypes = [i32, i32, i32, i32]
    l.wire_ssim_ws_bytes.restype = i64
    l.wire_ssim.argtypes = [vp, vp, vp, i32, i32, i32, i32, C.POINTER(C.c_float), f32, f32, f32, vp, vp, vp, i64]
    l.wire_ssim_bwd_ws_bytes.argtypes = [i32, i32, i32, i32]
    l.wire_ssim_bwd_ws_bytes.restype = i64
    l.wire_ssim_bwd.argtypes = [vp, vp, vp, i32, i32, i32, i32, C.POINTER(C.c_float), f32, f32, f32, vp, vp, vp, i64]
    l.wire_ssim_mse_grad_ws_bytes.argtypes = [i32, i32, i32, i32]
    l.wire_ssim_mse_grad_ws_bytes.restype = i64
    l.wire_ssim_mse_grad.argtypes = [vp, vp, i32, i32, i32, vp, i32, C.POINTER(C.c_float), f32, f32, f32, vp, i64, i64,
                                     f32, vp, vp, vp, vp, i64]
    l.wire_prof_enable.argtypes = [i32]
    l.wire_prof_read.argtypes = [C.POINTER(C.c_double), C.POINTER(i64), C.POINTER(C.c_double)]


def lib() -> C.CDLL:
    """Load libwire_hip.so once; raise (never fall back) when it is missing."""
    global _lib
    if _lib is None:
        if not os.path.exists(LIB_PATH):
            raise WireHipError(
                f"{LIB_PATH} is not built: run `make -C wire_amd/csrc` (needs hipcc, "
                "--offload-arch=gfx950).  wire_amd has no CPU fallback.")
        l = C.CDLL(LIB_PATH)
        _declare(l)
        v = l.wire_abi_version()
        if v != ABI_VERSION:
            raise WireHipError(f"libwire_hip.so ABI {v} != expected {ABI_VERSION}")
        _lib = l
    return _lib


def check(rc: int, what: str = "") -> int:
    if rc < 0:
        msg = lib().wire_last_error().decode(errors="replace")
        raise WireHipError(f"{what or 'libwire_hip'} failed ({rc}): {msg}")
    return rc


def make_desc(kind: str, in_features: int, width: int, hidden_layers: int, out_features: int,
              first_omega0: float, hidden_omega0: float, scale0: float,
              posenc_freqs: int = 0) -> NetDesc:
    return NetDesc(KIND[kind], int(in_features), int(width), int(hidden_layers),
                   int(out_features), int(posenc_freqs), float(first_omega0),
                   float(hidden_omega0), float(scale0))


def make_desc_scaled(kind: str, in_features: int, width: int, hidden_layers: int, out_features: int,
                     first_omega0: float, hidden_omega0: float, scale0: float, first_width: int, scales,
                     min_scales: int) -> NetDesc:
    """Descriptor of a scaled B-spline net: the ``base`` NetDesc of a NetDescMS (pass it wherever a NetDesc goes; it
    keeps the struct alive and lies at its start), ``scales`` padded with zeros."""
    scales = [float(v) for v in scales]
    if not min_scales <= len(scales) <= MS_MAX_SCALES:
        raise ValueError(f"{len(scales)} scales: the descriptor takes {min_scales}..{MS_MAX_SCALES}")
    ms = NetDescMS(make_desc(kind, in_features, width, hidden_layers, out_features, first_omega0, hidden_omega0, scale0),
                   int(first_width), len(scales),
                   (C.c_float * MS_MAX_SCALES)(*(scales + [0.0] * (MS_MAX_SCALES - len(scales)))))
    return ms.base


def make_desc_ms(in_features: int, width: int, hidden_layers: int, out_features: int, first_omega0: float,
                 hidden_omega0: float, scale0: float, first_width: int, scales) -> NetDesc:
    """Descriptor of a bspline_mscale_HL net (kind 6): one scale per column group of its first stage."""
    return make_desc_scaled("bspline_mscale_HL", in_features, width, hidden_layers, out_features, first_omega0,
                            hidden_omega0, scale0, first_width, scales, 2)


def make_desc_m2(in_features: int, width: int, hidden_layers: int, out_features: int, first_omega0: float,
                 hidden_omega0: float, scale0: float, scales) -> NetDesc:
    """Descriptor of a bspline_mscale_2 net (kind 8): first_width = 0 and one scale per trunk pass; ``scale0`` is
    carried and ignored."""
    return make_desc_scaled("bspline_mscale_2", in_features, width, hidden_layers, out_features, first_omega0,
                            hidden_omega0, scale0, 0, scales, 1)


def make_desc_hier(in_features: int, width: int, hidden_layers: int, out_features: int, first_omega0: float,
                   hidden_omega0: float, scale0: float, scales) -> NetDesc:
    """Descriptor of a bspline_mscale_hier net (kind 9): first_width = 0 and one scale per stage; ``scale0`` is
    carried and ignored."""
    return make_desc_scaled("bspline_mscale_hier", in_features, width, hidden_layers, out_features, first_omega0,
                            hidden_omega0, scale0, 0, scales, 1)


def hier_tensor_map(hidden_layers: int, nscales: int):
    """params[] of a bspline_mscale_hier net (csrc/wire_plan.h: hier_t, hier_th) as (first, last, head0): the first
    tensor and the index of the last layer of every stage, and the first head's tensor.  Stage 0 holds hidden_layers + 1
    (W, b) pairs, a later stage three; the heads' pairs follow the stages."""
    L, S = int(hidden_layers), int(nscales)
    start = lambda s: 0 if s == 0 else 2 * (L + 1) + 6 * (s - 1)
    return [start(s) for s in range(S)], [L] + [2] * (S - 1), start(S)


def ptr_array(ptrs):
    arr = (C.c_void_p * len(ptrs))()
    for i, p in enumerate(ptrs):
        arr[i] = p
    return arr
