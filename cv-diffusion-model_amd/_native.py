"""ctypes binding of libllie_hip.so (C ABI declared in include/llie.h).

There is no Python/PyTorch fallback: if the library is missing the import of the engine fails loudly
(`LibraryNotBuilt`), and if no HIP device is present every compute entry point raises.
PyTorch is used by callers only for device memory, streams and torch.distributed.
"""
from __future__ import annotations

import ctypes as C
import os
from typing import List, Tuple

_HERE = os.path.dirname(os.path.abspath(__file__))
LIB_PATH = os.path.join(_HERE, "libllie_hip.so")

# enums of include/llie.h
LLIE_F32, LLIE_F16, LLIE_BF16 = 0, 1, 2
LLIE_UNET, LLIE_IRB, LLIE_ATTN, LLIE_DOWN, LLIE_UP, LLIE_SE, LLIE_SOFTATTN = 0, 1, 2, 3, 4, 5, 6
ERR_ARG, ERR_SHAPE, ERR_CONFIG, ERR_KEY, ERR_NOT_LOADED, ERR_WORKSPACE, ERR_NO_DEVICE = -1, -2, -3, -4, -5, -6, -7
SAMPLER_LCM, SAMPLER_DDIM = 0, 1  # llie_step_coef.sampler
PRED_EPSILON, PRED_V = 0, 1  # LLIE_PRED_*: what a network output means to llie_consistency_target_ex / llie_consistency_loss_ex
LOSS_MSE, LOSS_L1, LOSS_HUBER = 0, 1, 2  # LLIE_LOSS_*: loss_type of llie_snr_loss

EXPORTS = [
    "llie_last_error", "llie_version", "llie_create", "llie_destroy", "llie_num_params", "llie_param_info",
    "llie_load_param", "llie_params_loaded", "llie_workspace_bytes", "llie_unet_forward", "llie_module_forward",
    "llie_lcm_step", "llie_add_noise", "llie_enhance", "llie_algorithmic_bytes", "llie_flops",
    "llie_profile_begin", "llie_profile_end", "llie_enhance_workspace_bytes",
    "llie_preprocess_u8", "llie_postprocess_u8", "llie_profile_report", "llie_pw_gemm", "llie_pw_gemm_tile_rows", "llie_dwconv3x3", "llie_dwconv3x3_tiles", "llie_tune",
    "llie_grad_numel", "llie_param_grad_offset", "llie_train_workspace_bytes", "llie_unet_train_forward",
    "llie_unet_backward", "llie_module_backward", "llie_load_all", "llie_profile_dump", "llie_copy_probe", "llie_rw_probe", "llie_pw_expand", "llie_gram_stats", "llie_gram_part_floats", "llie_groupnorm_finalize", "llie_conv3x3", "llie_conv3x3_tiles", "llie_linattn", "llie_linattn_splits", "llie_se_mlp", "llie_film", "llie_refresh_params", "llie_path_bytes", "llie_time_embed", "llie_debug_irbx_stamps", "llie_debug_gemm_stamps", "llie_debug_pwx_stamps", "llie_graph_cache_entries", "llie_debug_conv_stamps", "llie_gram_finalize",
    "llie_optimizer_create", "llie_optimizer_destroy", "llie_optimizer_numel", "llie_optimizer_step",
    "llie_optimizer_step_amp", "llie_grad_accumulate",
    "llie_consistency_target", "llie_consistency_loss", "llie_consistency_target_ex", "llie_consistency_loss_ex", "llie_ema_create", "llie_ema_update", "llie_ema_destroy",
    "llie_wgrad", "llie_wgrad_msplit", "llie_wgrad_partial_floats", "llie_dw_wgrad", "llie_dw_wgrad_strips",
    "llie_groupnorm_backward", "llie_groupnorm_backward_scratch_floats", "llie_linattn_backward", "llie_linattn_dkv_floats",
    "llie_upsample2x_backward", "llie_dilate2x", "llie_linear_dx", "llie_linear_dx_scratch_floats", "llie_linear_dw",
    "llie_final_bwd_data",
    "llie_dwconv3x3_backward", "llie_groupnorm_backward_from_slab", "llie_bias_grad", "llie_bias_grad_floats", "llie_pack_planes",
    "llie_add_into", "llie_sin_embed", "llie_pointwise_backward",
    "llie_tile_count", "llie_tile_origins", "llie_tile_gather_u8", "llie_tile_gather_f32", "llie_tile_blend_u8",
    "llie_tile_sync_step",
    "llie_aug_pair_u8", "llie_aug_synth_u8",
    "llie_image_metrics_scratch_bytes", "llie_image_metrics_f32", "llie_image_metrics_u8", "llie_comparison_grid_u8",
    "llie_upconv_fold_elems", "llie_upconv_fold_weights", "llie_conv3x3_upfold", "llie_conv3x3_upfold_tiles",
    "llie_conv3x3_upmaps", "llie_conv3x3_upmaps_supported", "llie_conv3x3_upmaps_grid", "llie_conv3x3_upmaps_workgroups",
    "llie_expand_dw", "llie_expand_pool", "llie_expand_dw_project", "llie_expand_dw_project_skip", "llie_irbx_project_tiles",
    "llie_expand_dw_plan", "llie_wide_project_supported", "llie_irb_forms", "llie_dwconv3x3_pool", "llie_dwconv3x3_project",
    "llie_expand_stats", "llie_irbx_stats_rows",
    "llie_wide_gram_supported", "llie_gram_wide_floats", "llie_gram_wide_part_floats", "llie_gram_wide_block", "llie_gram_wide",
    "llie_gram_group_weights", "llie_gram_group_finalize", "llie_pw_expand_act", "llie_dwconv3x3_project_preact", "llie_irb_wide_gram",
    "llie_dwconv3x3_ex", "llie_dwconv3x3_strip_rows", "llie_last_kernel",
    "llie_init_conv", "llie_init_conv_tiles", "llie_init_conv_pack_bytes", "llie_final_conv", "llie_final_conv_pack_bytes",
    "llie_se_gate", "llie_affine_add", "llie_nchw_to_nhwc", "llie_nhwc_to_nchw", "llie_pw_gemm_dot",
    "llie_frame_shape_ok", "llie_frame_workspace_bytes", "llie_unet_forward_hw", "llie_enhance_hw",
    "llie_frame_pad", "llie_frame_load_u8", "llie_frame_store_u8",
    "llie_ssim_grad_scratch_bytes", "llie_ssim_grad_f32", "llie_x0_loss",
    "llie_train_shape_ok", "llie_unet_train_forward_hw", "llie_aug_pair_u8_hw", "llie_aug_synth_u8_hw",
    "llie_tile_gather_u8_hw", "llie_tile_gather_f32_hw", "llie_tile_blend_u8_hw", "llie_tile_sync_step_hw", "llie_frame_max_pixels",
    "llie_unet_backward_dx", "llie_init_conv_dgrad",
    "llie_softattn", "llie_softattn_backward", "llie_softattn_bwd_floats",
    "llie_pw_expand_nsplit", "llie_silu_rows",
    "llie_guide", "llie_guidance_pair", "llie_cond_dropout",
    "llie_guide_rescale_chunk", "llie_guide_rescale_scratch_bytes", "llie_guide_rescale",
    "llie_dpm_step", "llie_enhance_dpm", "llie_enhance_dpm_hw",
    "llie_snr_loss_chunk", "llie_snr_loss_scratch_bytes", "llie_snr_loss",
]
K_GEMM, K_DW, K_CONV3, K_SE, K_OTHER = 1, 2, 4, 8, 16
PW_SIGMOID_BWD, PW_RELU6_BWD, PW_SILU_BWD, PW_SCALE = 0, 1, 2, 3  # llie_pointwise_kind


class GemmSeg(C.Structure):
    _fields_ = [("ptr", C.c_void_p), ("channels", C.c_int), ("scale", C.c_void_p), ("bias", C.c_void_p),
                ("affine_ld", C.c_int), ("act", C.c_int)]


class GnBackwardArgs(C.Structure):
    """llie_gn_backward_args (include/llie.h): one GroupNorm site of the backward pass."""
    _fields_ = [("g", C.c_void_p), ("dz", C.c_void_p), ("x0", C.c_void_p), ("x1", C.c_void_p), ("c0", C.c_int), ("c1", C.c_int),
                ("scale", C.c_void_p), ("shift", C.c_void_p), ("act", C.c_int), ("mean", C.c_void_p), ("rstd", C.c_void_p),
                ("gamma", C.c_void_p), ("beta", C.c_void_p), ("film", C.c_void_p), ("film_stride", C.c_int64), ("dfilm", C.c_void_p),
                ("dfilm_stride", C.c_int64), ("dgamma", C.c_void_p), ("dbeta", C.c_void_p), ("add0", C.c_void_p), ("add1_0", C.c_void_p),
                ("add1_1", C.c_void_p), ("dx0", C.c_void_p), ("dx1", C.c_void_p), ("batch", C.c_int), ("pixels", C.c_int)]


class LibraryNotBuilt(RuntimeError):
    pass


class Config(C.Structure):
    _fields_ = [
        ("kind", C.c_int), ("compute_dtype", C.c_int), ("in_channels", C.c_int), ("out_channels", C.c_int),
        ("base_channels", C.c_int), ("channel_multipliers", C.c_int * 4), ("num_res_blocks", C.c_int),
        ("expansion_ratio", C.c_int), ("time_embed_dim", C.c_int), ("num_attention_heads", C.c_int),
        ("image_size", C.c_int), ("attention_resolutions", C.c_int * 2), ("allow_unpinned", C.c_int),
        ("softmax_attention", C.c_int),  # appended: a zero-initialised struct keeps meaning LinearAttention
    ]


class OptTensor(C.Structure):
    """llie_opt_tensor (include/llie.h): one parameter of the fused optimiser step."""
    _fields_ = [("param", C.c_void_p), ("exp_avg", C.c_void_p), ("exp_avg_sq", C.c_void_p), ("ema", C.c_void_p),
                ("grad_offset", C.c_int64), ("numel", C.c_int64)]


class OptHyper(C.Structure):
    """llie_opt_hyper (include/llie.h)."""
    _fields_ = [("lr", C.c_double), ("beta1", C.c_double), ("beta2", C.c_double), ("eps", C.c_double), ("weight_decay", C.c_double),
                ("max_grad_norm", C.c_double), ("ema_decay", C.c_double), ("grad_scale", C.c_double), ("step", C.c_int64),
                ("skip_nonfinite", C.c_int32)]


class AmpState(C.Structure):
    """llie_amp_state (include/llie.h): device pointers to the loss scale, the growth tracker and the AdamW step count."""
    _fields_ = [("scale", C.c_void_p), ("growth_tracker", C.c_void_p), ("step", C.c_void_p)]


class AmpConfig(C.Structure):
    """llie_amp_config (include/llie.h)."""
    _fields_ = [("growth_factor", C.c_double), ("backoff_factor", C.c_double), ("growth_interval", C.c_int32)]


class _StepCoefLayout(C.Structure):
    """llie_step_coef (include/llie.h), member by member."""
    _fields_ = [
        ("sqrt_alpha_t", C.c_float), ("sqrt_beta_t", C.c_float), ("sqrt_alpha_prev", C.c_float),
        ("sqrt_beta_prev", C.c_float), ("is_last", C.c_int), ("v_prediction", C.c_int), ("clamp_x0", C.c_int),
        ("sampler", C.c_int),  # 0 LCM (the default of a positional construction), 1 deterministic DDIM
    ]


class _SevenScalars(type(C.Structure)):
    """Metaclass of StepCoef: `StepCoef._fields_` names the seven scalars of the LCM step (see there); the layout is the base's."""

    @property
    def _fields_(cls):
        return _StepCoefLayout._fields_[:7]


class StepCoef(_StepCoefLayout, metaclass=_SevenScalars):
    """llie_step_coef.  The layout is _StepCoefLayout's eight members; `sampler` trails, defaults to 0 (LCM) and is set as the
    eighth positional argument or by keyword.  `StepCoef._fields_` keeps naming the seven scalars of the LCM step: callers
    enumerate it to read back the fp32 values a kernel gets and unpack them as (sa, sb, sap, sbp, is_last, vpred, clamp_x0), as
    they did before the struct grew; the sampler is read as `coef.sampler`."""


class DpmCoef(C.Structure):
    """llie_dpm_coef (include/llie.h): one step of DPM-Solver++ 2M.  The float members round a Python float (float64) once to fp32."""
    _fields_ = [
        ("sqrt_alpha_t", C.c_float), ("sqrt_beta_t", C.c_float), ("k_x", C.c_float), ("k_0", C.c_float), ("k_1", C.c_float),
        ("v_prediction", C.c_int), ("order", C.c_int), ("is_last", C.c_int),
    ]


DISTILL_LOSS_PER_WG = 1024  # kDistillLossPerWG (csrc/kernels.h): llie_consistency_loss needs one double per this many elements


def distill_scratch_bytes(n: int) -> int:
    return 8 * ((n + DISTILL_LOSS_PER_WG - 1) // DISTILL_LOSS_PER_WG)


_lib = None


def lib() -> C.CDLL:
    """Load the engine once.  torch must already be imported by the caller so that the HIP runtime the
    library binds to (SONAME libamdhip64.so.7) is the one PyTorch-ROCm loaded."""
    global _lib
    if _lib is not None:
        return _lib
    if not os.path.exists(LIB_PATH):
        raise LibraryNotBuilt(
            f"{LIB_PATH} not found: run `python -c 'import __graft_entry__ as g; g.build()'` "
            "(or `make -C cv-diffusion-model_amd/csrc`).  There is no CPU/PyTorch fallback for the hot path.")
    import torch  # noqa: F401  (loads libamdhip64 first)
    L = C.CDLL(LIB_PATH)
    vp, i64, ci = C.c_void_p, C.c_int64, C.c_int
    L.llie_last_error.restype = C.c_char_p
    L.llie_version.restype = C.c_char_p
    L.llie_create.argtypes = [C.POINTER(Config), C.POINTER(vp)]
    L.llie_destroy.argtypes = [vp]
    L.llie_destroy.restype = None
    L.llie_num_params.argtypes = [vp]
    L.llie_param_info.argtypes = [vp, ci, C.c_char_p, C.c_size_t, C.POINTER(i64), C.POINTER(ci), C.POINTER(i64)]
    L.llie_load_param.argtypes = [vp, C.c_char_p, vp, i64, vp]
    L.llie_params_loaded.argtypes = [vp]
    L.llie_load_all.argtypes = [vp, C.POINTER(vp), ci, vp]
    L.llie_refresh_params.argtypes = [vp, C.POINTER(vp), ci, vp]
    L.llie_workspace_bytes.argtypes = [vp, ci, ci, ci]
    L.llie_workspace_bytes.restype = i64
    L.llie_enhance_workspace_bytes.argtypes = [vp, ci, ci]
    L.llie_enhance_workspace_bytes.restype = i64
    L.llie_unet_forward.argtypes = [vp, vp, vp, vp, ci, vp, ci, vp, i64, vp]
    L.llie_module_forward.argtypes = [vp, vp, vp, vp, ci, ci, ci, vp, i64, vp]
    L.llie_lcm_step.argtypes = [vp, vp, vp, vp, vp, vp, i64, C.POINTER(StepCoef), vp]
    L.llie_add_noise.argtypes = [vp, vp, vp, vp, ci, vp, ci, i64, ci, vp]
    L.llie_copy_probe.argtypes = [vp, vp, i64, vp]
    L.llie_rw_probe.argtypes = [vp, vp, i64, C.c_int, C.c_int, C.c_int, vp]
    L.llie_enhance.argtypes = [vp, vp, vp, vp, C.POINTER(StepCoef), ci, vp, vp, vp, ci, vp, i64, vp]
    L.llie_algorithmic_bytes.argtypes = [vp, ci]
    L.llie_algorithmic_bytes.restype = i64
    L.llie_time_embed.argtypes = [vp, vp, ci, vp, vp, vp, vp]
    L.llie_path_bytes.argtypes = [vp, ci]
    L.llie_path_bytes.restype = i64
    L.llie_flops.argtypes = [vp, ci]
    L.llie_flops.restype = i64
    L.llie_preprocess_u8.argtypes = [vp, ci, ci, ci, vp, ci, vp]
    L.llie_postprocess_u8.argtypes = [vp, ci, ci, vp, ci, ci, vp]
    L.llie_tile_count.argtypes = [ci, ci, ci]
    L.llie_tile_origins.argtypes = [ci, ci, ci, C.POINTER(ci)]
    L.llie_tile_gather_u8.argtypes = [vp, ci, ci, ci, ci, ci, ci, vp, vp]
    L.llie_tile_gather_f32.argtypes = [vp, ci, ci, ci, ci, ci, ci, ci, vp, vp]
    L.llie_tile_blend_u8.argtypes = [vp, ci, ci, ci, ci, vp, vp]
    L.llie_tile_sync_step.argtypes = [vp, ci, ci, ci, ci, vp, vp, C.POINTER(StepCoef), vp, vp, vp]
    L.llie_tile_gather_u8_hw.argtypes = [vp, ci, ci, ci, ci, ci, ci, ci, ci, vp, vp]
    L.llie_tile_gather_f32_hw.argtypes = [vp, ci, ci, ci, ci, ci, ci, ci, ci, ci, vp, vp]
    L.llie_tile_blend_u8_hw.argtypes = [vp, ci, ci, ci, ci, ci, ci, vp, vp]
    L.llie_tile_sync_step_hw.argtypes = [vp, ci, ci, ci, ci, ci, ci, vp, vp, C.POINTER(StepCoef), vp, vp, vp]
    L.llie_frame_shape_ok.argtypes = [vp, ci, ci, ci]
    L.llie_frame_max_pixels.argtypes = [vp, ci]
    L.llie_frame_max_pixels.restype = i64
    L.llie_frame_workspace_bytes.argtypes = [vp, ci, ci, ci, ci]
    L.llie_frame_workspace_bytes.restype = i64
    L.llie_unet_forward_hw.argtypes = [vp, vp, vp, vp, ci, vp, ci, ci, ci, vp, i64, vp]
    L.llie_enhance_hw.argtypes = [vp, vp, vp, vp, C.POINTER(StepCoef), ci, vp, vp, vp, ci, ci, ci, vp, i64, vp]
    L.llie_dpm_step.argtypes = [vp, vp, vp, vp, vp, i64, C.POINTER(DpmCoef), vp]
    L.llie_enhance_dpm.argtypes = [vp, vp, vp, vp, C.POINTER(DpmCoef), ci, vp, vp, vp, ci, vp, i64, vp]
    L.llie_enhance_dpm_hw.argtypes = [vp, vp, vp, vp, C.POINTER(DpmCoef), ci, vp, vp, vp, ci, ci, ci, vp, i64, vp]
    L.llie_frame_pad.argtypes = [ci]
    L.llie_frame_load_u8.argtypes = [vp, ci, ci, vp, vp]
    L.llie_frame_store_u8.argtypes = [vp, ci, ci, vp, vp]
    L.llie_aug_pair_u8.argtypes = [vp, vp, ci, vp, ci, ci, ci, vp, vp, vp, vp, vp]
    L.llie_aug_synth_u8.argtypes = [vp, vp, ci, vp, ci, ci, ci, vp, vp, vp, vp, vp, vp]
    L.llie_aug_pair_u8_hw.argtypes = [vp, vp, ci, vp, ci, ci, ci, ci, vp, vp, vp, vp, vp]
    L.llie_aug_synth_u8_hw.argtypes = [vp, vp, ci, vp, ci, ci, ci, ci, vp, vp, vp, vp, vp, vp]
    L.llie_image_metrics_scratch_bytes.argtypes = [ci, ci, ci]
    L.llie_image_metrics_scratch_bytes.restype = i64
    L.llie_image_metrics_f32.argtypes = [vp, vp, ci, ci, ci, C.c_float, C.c_float, vp, vp, i64, vp]
    L.llie_image_metrics_u8.argtypes = [vp, vp, ci, ci, ci, vp, vp, i64, vp]
    L.llie_ssim_grad_scratch_bytes.argtypes = [ci, ci, ci]
    L.llie_ssim_grad_scratch_bytes.restype = i64
    L.llie_ssim_grad_f32.argtypes = [vp, vp, ci, ci, ci, C.c_float, C.c_float, vp, vp, vp, vp, i64, vp]
    L.llie_x0_loss.argtypes = [vp, vp, vp, vp, vp, ci, ci, C.c_float, C.c_float, vp, vp, ci, ci, ci, vp, i64, vp]
    L.llie_snr_loss_chunk.argtypes = []
    L.llie_snr_loss_chunk.restype = i64
    L.llie_snr_loss_scratch_bytes.argtypes = [ci, i64]
    L.llie_snr_loss_scratch_bytes.restype = i64
    L.llie_snr_loss.argtypes = [vp, vp, vp, vp, ci, ci, ci, C.c_float, vp, vp, vp, vp, ci, i64, vp, i64, vp]
    L.llie_comparison_grid_u8.argtypes = [vp, vp, vp, ci, ci, ci, vp, vp]
    L.llie_pw_gemm.argtypes = [ci, C.POINTER(GemmSeg), ci, vp, vp, vp, vp, vp, ci, ci, ci, vp]
    L.llie_pw_gemm_tile_rows.argtypes = [ci]
    L.llie_pw_expand.argtypes = [ci, C.POINTER(GemmSeg), ci, vp, vp, vp, vp, ci, ci, ci, vp]
    L.llie_gram_stats.argtypes = [ci, vp, ci, vp, ci, vp, vp, ci, ci, vp, vp, vp, vp]
    L.llie_gram_part_floats.argtypes = [ci, ci]
    L.llie_gram_finalize.argtypes = [ci, vp, vp, ci, ci, vp, vp, vp, i64, C.c_float, C.c_float, ci, vp, vp, vp]
    L.llie_groupnorm_finalize.argtypes = [vp, ci, ci, vp, ci, ci, ci, ci, vp, vp, vp, i64, C.c_float, C.c_float, ci, vp, vp, vp]
    L.llie_conv3x3.argtypes = [ci, ci, vp, vp, vp, vp, vp, ci, ci, ci, ci, ci, vp]
    L.llie_conv3x3_tiles.argtypes = [ci, ci]
    L.llie_upconv_fold_elems.argtypes = [ci]
    L.llie_upconv_fold_elems.restype = i64
    L.llie_upconv_fold_weights.argtypes = [ci, vp, vp, ci, vp]
    L.llie_conv3x3_upfold.argtypes = [ci, vp, vp, vp, vp, vp, ci, ci, ci, ci, vp]
    L.llie_conv3x3_upfold_tiles.argtypes = [ci, ci]
    L.llie_conv3x3_upmaps.argtypes = [ci, vp, vp, vp, vp, vp, ci, ci, ci, ci, vp]
    L.llie_conv3x3_upmaps_supported.argtypes = [ci, ci, ci, ci]
    L.llie_conv3x3_upmaps_grid.argtypes = [ci, vp, vp, vp, vp, vp, ci, ci, ci, ci, ci, vp]
    L.llie_conv3x3_upmaps_workgroups.argtypes = [ci, ci, ci, ci]
    L.llie_linattn.argtypes = [ci, vp, vp, vp, ci, ci, ci, vp]
    L.llie_linattn_splits.argtypes = [ci]
    L.llie_se_mlp.argtypes = [ci, vp, ci, vp, vp, vp, vp, vp, vp, vp, ci, ci, ci, vp]
    L.llie_film.argtypes = [vp, vp, vp, vp, ci, ci, ci, vp]
    L.llie_pw_expand_nsplit.argtypes = [ci, ci]
    L.llie_silu_rows.argtypes = [vp, vp, i64, vp]
    L.llie_gram_part_floats.restype = i64
    L.llie_dwconv3x3.argtypes = [ci, vp, vp, vp, vp, vp, vp, ci, ci, ci, ci, vp]
    L.llie_dwconv3x3_tiles.argtypes = [ci, ci]
    L.llie_dwconv3x3_ex.argtypes = [ci, vp, vp, vp, vp, vp, vp, vp, ci, ci, ci, ci, ci, vp]
    L.llie_dwconv3x3_strip_rows.argtypes = [ci, ci, ci, ci, ci]
    L.llie_init_conv_pack_bytes.argtypes = [ci, ci]
    L.llie_init_conv_pack_bytes.restype = i64
    L.llie_init_conv_tiles.argtypes = [ci, ci, ci]
    L.llie_init_conv.argtypes = [ci, vp, ci, vp, ci, vp, vp, vp, vp, ci, ci, ci, ci, ci, vp, i64, vp]
    L.llie_init_conv_dgrad.argtypes = [ci, vp, ci, vp, vp, ci, vp, ci, ci, ci, ci, vp, i64, vp]
    L.llie_final_conv_pack_bytes.argtypes = [ci]
    L.llie_final_conv_pack_bytes.restype = i64
    L.llie_final_conv.argtypes = [ci, vp, vp, vp, vp, vp, vp, ci, ci, ci, ci, ci, ci, C.POINTER(StepCoef), vp, vp, vp, vp, vp, i64, vp]
    L.llie_se_gate.argtypes = [ci, vp, ci, vp, vp, vp, vp, vp, ci, ci, ci, ci, vp, vp, vp]
    L.llie_affine_add.argtypes = [ci, vp, vp, vp, vp, vp, vp, ci, ci, ci, vp]
    L.llie_nchw_to_nhwc.argtypes = [ci, vp, vp, vp, ci, ci, ci, ci, ci, vp]
    L.llie_nhwc_to_nchw.argtypes = [ci, vp, vp, ci, ci, ci, ci, ci, vp]
    L.llie_pw_gemm_dot.argtypes = [ci, C.POINTER(GemmSeg), ci, vp, vp, vp, vp, vp, ci, ci, ci, vp]
    L.llie_last_kernel.argtypes = []
    L.llie_last_kernel.restype = C.c_char_p
    L.llie_expand_dw.argtypes = [ci, vp, ci, vp, ci, vp, vp, vp, vp, vp, vp, vp, vp, ci, ci, ci, vp]
    L.llie_expand_pool.argtypes = [ci, vp, ci, vp, ci, vp, vp, vp, vp, vp, vp, vp, ci, ci, ci, vp]
    L.llie_expand_dw_project.argtypes = [ci, vp, ci, vp, vp, vp, vp, vp, vp, vp, vp, vp, vp, ci, ci, ci, vp]
    L.llie_expand_dw_project_skip.argtypes = [ci, vp, ci, vp, ci, vp, vp, vp, vp, vp, vp, vp, vp, ci, ci, vp, vp, ci, ci, ci, vp]
    L.llie_irbx_project_tiles.argtypes = [ci, ci]
    L.llie_expand_dw_plan.argtypes = [ci, ci, ci, ci, ci, C.POINTER(ci)]
    L.llie_wide_project_supported.argtypes = [ci] * 9
    L.llie_irb_forms.argtypes = [vp, ci, ci, C.POINTER(ci), ci]
    L.llie_dwconv3x3_pool.argtypes = [ci, vp, vp, vp, vp, vp, ci, ci, ci, ci, vp]
    L.llie_dwconv3x3_project.argtypes = [ci, vp, vp, vp, vp, vp, vp, ci, vp, ci, vp, ci, ci, vp, vp, ci, ci, ci, vp]
    L.llie_expand_stats.argtypes = [ci, vp, ci, vp, ci, vp, vp, vp, vp, ci, ci, ci, vp]
    L.llie_irbx_stats_rows.argtypes = [ci]
    L.llie_wide_gram_supported.argtypes = [ci] * 5
    L.llie_gram_wide_floats.argtypes = []
    L.llie_gram_wide_floats.restype = i64
    L.llie_gram_wide_part_floats.argtypes = [ci]
    L.llie_gram_wide_part_floats.restype = i64
    L.llie_gram_wide_block.argtypes = [ci, C.POINTER(ci), C.POINTER(ci)]
    L.llie_gram_wide.argtypes = [ci, vp, ci, vp, ci, vp, vp, ci, ci, vp, vp, vp]
    L.llie_gram_group_weights.argtypes = [ci, vp, vp, ci, ci, vp]
    L.llie_gram_group_finalize.argtypes = [vp, vp, ci, ci, vp, vp, vp, i64, C.c_float, C.c_float, ci, vp, vp, vp]
    L.llie_pw_expand_act.argtypes = [ci, C.POINTER(GemmSeg), ci, vp, vp, vp, vp, vp, vp, vp, ci, ci, ci, ci, vp]
    L.llie_dwconv3x3_project_preact.argtypes = [ci, vp, vp, vp, vp, ci, vp, ci, vp, ci, ci, vp, vp, ci, ci, ci, vp]
    L.llie_irb_wide_gram.argtypes = [vp, ci, ci, C.POINTER(ci), ci]
    L.llie_tune.argtypes = [C.c_char_p, ci]
    L.llie_debug_irbx_stamps.argtypes = [C.POINTER(C.c_double)]
    L.llie_optimizer_create.argtypes = [C.POINTER(OptTensor), ci, C.POINTER(C.c_void_p)]
    L.llie_optimizer_destroy.argtypes = [C.c_void_p]
    L.llie_optimizer_destroy.restype = None
    L.llie_optimizer_numel.argtypes = [C.c_void_p]
    L.llie_optimizer_numel.restype = C.c_int64
    L.llie_optimizer_step.argtypes = [C.c_void_p, vp, C.POINTER(OptHyper), vp, vp]
    L.llie_optimizer_step_amp.argtypes = [C.c_void_p, vp, C.POINTER(OptHyper), C.POINTER(AmpState), C.POINTER(AmpConfig), vp, vp]
    L.llie_grad_accumulate.argtypes = [vp, vp, i64, C.c_float, ci, vp]
    L.llie_consistency_target.argtypes = [vp, vp, vp, vp, vp, ci, vp, ci, i64, vp]
    L.llie_consistency_loss.argtypes = [vp, vp, vp, vp, vp, vp, vp, ci, vp, vp, ci, i64, vp, i64, vp]
    L.llie_consistency_target_ex.argtypes = [vp, vp, vp, vp, vp, ci, vp, ci, i64, ci, vp]
    L.llie_consistency_loss_ex.argtypes = [vp, vp, vp, vp, vp, vp, vp, ci, vp, vp, vp, i64, ci, i64, ci, vp]
    L.llie_guide.argtypes = [vp, vp, vp, C.c_float, vp, ci, i64, vp]
    L.llie_guidance_pair.argtypes = [vp, vp, vp, vp, ci, i64, vp]
    L.llie_guide_rescale_chunk.argtypes = []
    L.llie_guide_rescale_chunk.restype = i64
    L.llie_guide_rescale_scratch_bytes.argtypes = [ci, i64]
    L.llie_guide_rescale_scratch_bytes.restype = i64
    L.llie_guide_rescale.argtypes = [vp, vp, vp, C.c_float, C.c_float, vp, vp, vp, i64, ci, i64, vp]
    L.llie_cond_dropout.argtypes = [vp, vp, C.c_float, vp, ci, i64, vp]
    L.llie_ema_create.argtypes = [C.POINTER(vp), C.POINTER(vp), C.POINTER(i64), ci, C.POINTER(vp)]
    L.llie_ema_update.argtypes = [vp, C.c_double, vp]
    L.llie_ema_destroy.argtypes = [vp]
    L.llie_ema_destroy.restype = None
    L.llie_graph_cache_entries.argtypes = [C.c_void_p]
    L.llie_graph_cache_entries.restype = C.c_int
    L.llie_debug_gemm_stamps.argtypes = [C.POINTER(C.c_double)]
    L.llie_debug_conv_stamps.argtypes = [C.POINTER(C.c_double)]
    L.llie_debug_pwx_stamps.argtypes = [C.POINTER(C.c_double)]
    L.llie_grad_numel.argtypes = [vp]
    L.llie_grad_numel.restype = i64
    L.llie_param_grad_offset.argtypes = [vp, ci]
    L.llie_param_grad_offset.restype = i64
    L.llie_train_workspace_bytes.argtypes = [vp, ci, ci, ci]
    L.llie_train_workspace_bytes.restype = i64
    L.llie_unet_train_forward.argtypes = [vp, vp, vp, vp, vp, ci, vp, i64, vp]
    L.llie_unet_train_forward_hw.argtypes = [vp, vp, vp, vp, vp, ci, ci, ci, vp, i64, vp]
    L.llie_train_shape_ok.argtypes = [vp, ci, ci, ci]
    L.llie_unet_backward.argtypes = [vp, vp, vp, ci, vp, i64, vp]
    L.llie_unet_backward_dx.argtypes = [vp, vp, vp, vp, vp, ci, vp, i64, vp]
    L.llie_module_backward.argtypes = [vp, vp, vp, vp, vp, vp, vp, ci, ci, ci, vp, i64, vp]
    L.llie_wgrad.argtypes = [ci, vp, ci, C.POINTER(GemmSeg), ci, ci, ci, ci, ci, ci, ci, ci, ci, ci, ci, ci, vp, i64, vp, i64, i64, i64, ci, vp]
    L.llie_wgrad_msplit.argtypes = [ci, ci, ci, ci, ci, ci, ci]
    L.llie_wgrad_partial_floats.argtypes = [ci, ci, ci, ci]
    L.llie_wgrad_partial_floats.restype = i64
    L.llie_dw_wgrad.argtypes = [ci, vp, vp, vp, vp, vp, vp, vp, vp, ci, ci, ci, ci, vp]
    L.llie_dw_wgrad_strips.argtypes = [ci, ci]
    L.llie_groupnorm_backward.argtypes = [ci, C.POINTER(GnBackwardArgs), vp, i64, vp]
    L.llie_groupnorm_backward_scratch_floats.argtypes = [ci, ci, ci]
    L.llie_groupnorm_backward_scratch_floats.restype = i64
    L.llie_linattn_backward.argtypes = [ci, vp, vp, vp, vp, vp, i64, ci, ci, ci, vp]
    L.llie_linattn_dkv_floats.argtypes = [ci, ci, ci]
    L.llie_linattn_dkv_floats.restype = i64
    L.llie_softattn.argtypes = [ci, vp, vp, vp, ci, ci, ci, vp]
    L.llie_softattn_backward.argtypes = [ci, vp, vp, vp, vp, vp, vp, i64, ci, ci, ci, vp]
    L.llie_softattn_bwd_floats.argtypes = [ci, ci, ci]
    L.llie_softattn_bwd_floats.restype = i64
    L.llie_upsample2x_backward.argtypes = [ci, vp, vp, ci, ci, ci, ci, vp]
    L.llie_dilate2x.argtypes = [ci, vp, vp, ci, ci, ci, ci, vp]
    L.llie_linear_dx.argtypes = [ci, vp, i64, vp, vp, ci, ci, ci, vp, i64, vp]
    L.llie_linear_dx_scratch_floats.argtypes = [ci, ci, ci]
    L.llie_linear_dx_scratch_floats.restype = i64
    L.llie_linear_dw.argtypes = [vp, i64, vp, vp, vp, ci, ci, ci, vp]
    L.llie_final_bwd_data.argtypes = [ci, vp, vp, vp, ci, ci, ci, ci, ci, vp]
    L.llie_dwconv3x3_backward.argtypes = [ci, vp, vp, vp, vp, vp, vp, vp, vp, vp, ci, ci, ci, ci, vp]
    L.llie_groupnorm_backward_from_slab.argtypes = [ci, C.POINTER(GnBackwardArgs), vp, ci, vp, i64, vp]
    L.llie_bias_grad_floats.argtypes = [ci, ci, ci, C.POINTER(i64), C.POINTER(i64)]
    L.llie_bias_grad.argtypes = [ci, vp, ci, ci, ci, ci, vp, vp, vp, vp]
    L.llie_pack_planes.argtypes = [ci, vp, ci, vp, ci, vp, ci, ci, vp]
    L.llie_add_into.argtypes = [ci, vp, vp, i64, vp]
    L.llie_sin_embed.argtypes = [vp, vp, vp, ci, ci, vp]
    L.llie_pointwise_backward.argtypes = [ci, vp, vp, vp, i64, C.c_float, vp]
    L.llie_profile_report.argtypes = [vp, C.c_char_p, C.c_size_t]
    L.llie_profile_dump.argtypes = [vp, C.c_char_p, C.c_size_t]
    L.llie_profile_begin.argtypes = [vp, ci]
    L.llie_profile_end.argtypes = [vp, ci, C.POINTER(C.c_double), C.POINTER(i64), C.POINTER(i64)]
    _lib = L
    return L


def last_error() -> str:
    return lib().llie_last_error().decode()


def check(rc: int, what: str = "") -> None:
    """Map llie_status / hipError_t to the exception types the reference raises."""
    if rc == 0:
        return
    msg = f"{what}: {last_error()}" if what else last_error()
    if rc in (ERR_CONFIG,):
        raise ValueError(msg)            # nn.GroupNorm's ValueError (efficient_unet.py:170)
    if rc in (ERR_KEY, ERR_NOT_LOADED):
        raise RuntimeError(msg)          # load_state_dict's RuntimeError
    if rc == ERR_SHAPE or rc == ERR_ARG:
        raise ValueError(msg or f"invalid argument ({rc})")
    if rc == ERR_NO_DEVICE:
        raise RuntimeError(msg or "no HIP device: the LCM hot path runs only on an MI355X-class GPU")
    raise RuntimeError(msg or f"llie error {rc}")


def dtype_code(name) -> int:
    import torch
    table = {"fp32": 0, "float32": 0, torch.float32: 0, "fp16": 1, "float16": 1, torch.float16: 1,
             "bf16": 2, "bfloat16": 2, torch.bfloat16: 2}
    if name not in table:
        raise ValueError(f"unsupported compute dtype {name!r}; choose fp32, fp16 or bf16")
    return table[name]


class Handle:
    """Owns one llie_ctx."""

    def __init__(self, cfg: Config):
        self._L = lib()
        h = C.c_void_p()
        check(self._L.llie_create(C.byref(cfg), C.byref(h)), "llie_create")
        self.h = h
        self.cfg = cfg

    def close(self):
        if getattr(self, "h", None):
            self._L.llie_destroy(self.h)
            self.h = None

    def __del__(self):
        try:
            self.close()
        except Exception:  # noqa: BLE001
            pass

    def params(self) -> List[Tuple[str, Tuple[int, ...]]]:
        out = []
        buf = C.create_string_buffer(256)
        n, nd, shp = C.c_int64(), C.c_int(), (C.c_int64 * 4)()
        for i in range(self._L.llie_num_params(self.h)):
            check(self._L.llie_param_info(self.h, i, buf, 256, C.byref(n), C.byref(nd), shp))
            out.append((buf.value.decode(), tuple(int(shp[d]) for d in range(nd.value))))
        return out

    def load_param(self, key: str, tensor, stream: int) -> None:
        check(self._L.llie_load_param(self.h, key.encode(), tensor.data_ptr(), tensor.numel(), stream), "load_state_dict")

    def load_all(self, tensors, stream: int) -> None:
        """Reload every parameter (llie_param_info order) from fp32 contiguous device tensors in one call."""
        arr = (C.c_void_p * len(tensors))(*[t.data_ptr() for t in tensors])
        check(self._L.llie_load_all(self.h, arr, len(tensors), stream), "load_state_dict")

    def refresh(self, tensors, stream: int) -> None:
        """Reload only if the parameters' content changed since the last load (decided on the device, asynchronous)."""
        arr = (C.c_void_p * len(tensors))(*[t.data_ptr() for t in tensors])
        check(self._L.llie_refresh_params(self.h, arr, len(tensors), stream), "refresh_params")

    def params_loaded(self) -> bool:
        return bool(self._L.llie_params_loaded(self.h))

    def workspace_bytes(self, batch: int, h: int = 0, w: int = 0) -> int:
        n = self._L.llie_workspace_bytes(self.h, batch, h, w)
        if n < 0:
            check(int(n), "llie_workspace_bytes")
        return int(n)

    def train_workspace_bytes(self, batch: int, h: int = 0, w: int = 0) -> int:
        n = self._L.llie_train_workspace_bytes(self.h, batch, h, w)
        if n < 0:
            check(int(n), "llie_train_workspace_bytes")
        return int(n)

    def train_plan(self, batch: int, h: int, w: int) -> int:
        """Workspace bytes of a UNet training step on [batch,3,h,w]: ValueError naming the rule for a shape llie_train_shape_ok
        refuses; image_size itself goes unasked, as it always did."""
        s = int(self.cfg.image_size)
        return self.train_workspace_bytes(batch) if (h, w) == (s, s) else self.train_workspace_bytes(batch, h, w)

    def unet_train_forward(self, lat: int, cond: int, t: int, eps: int, batch: int, h: int, w: int, ws: int, nbytes: int, stream: int) -> None:
        """llie_unet_train_forward at image_size, llie_unet_train_forward_hw elsewhere (one implementation; device pointers)."""
        s = int(self.cfg.image_size)
        if (h, w) == (s, s):
            rc = self._L.llie_unet_train_forward(self.h, lat, cond, t, eps, batch, ws, nbytes, stream)
        else:
            rc = self._L.llie_unet_train_forward_hw(self.h, lat, cond, t, eps, batch, h, w, ws, nbytes, stream)
        check(rc, "EfficientUNet.forward (training)")

    def grad_numel(self) -> int:
        return int(self._L.llie_grad_numel(self.h))

    def grad_offsets(self) -> List[int]:
        return [int(self._L.llie_param_grad_offset(self.h, i)) for i in range(self._L.llie_num_params(self.h))]

    def enhance_workspace_bytes(self, batch: int, max_steps: int) -> int:
        n = self._L.llie_enhance_workspace_bytes(self.h, batch, max_steps)
        if n < 0:
            check(int(n), "llie_enhance_workspace_bytes")
        return int(n)

    def frame_shape_ok(self, batch: int, h: int, w: int) -> None:
        """Raises ValueError naming the rule of llie_frame_shape_ok that (batch, h, w) breaks."""
        check(self._L.llie_frame_shape_ok(self.h, batch, h, w), "frame shape")

    def frame_max_pixels(self, batch: int = 1) -> int:
        """The H * W the element cap of llie_frame_shape_ok allows each frame of `batch` (host only)."""
        n = self._L.llie_frame_max_pixels(self.h, batch)
        if n < 0:
            check(int(n), "llie_frame_max_pixels")
        return int(n)

    def train_shape_ok(self, batch: int, h: int, w: int) -> None:
        """Raises ValueError naming the rule of llie_train_shape_ok that (batch, h, w) breaks."""
        check(self._L.llie_train_shape_ok(self.h, batch, h, w), "training frame shape")

    def frame_workspace_bytes(self, batch: int, h: int, w: int, max_steps: int = 0) -> int:
        n = self._L.llie_frame_workspace_bytes(self.h, batch, h, w, max_steps)
        if n < 0:
            check(int(n), "llie_frame_workspace_bytes")
        return int(n)

    def algorithmic_bytes(self, batch: int) -> int:
        return int(self._L.llie_algorithmic_bytes(self.h, batch))

    def path_bytes(self, batch: int) -> int:
        return int(self._L.llie_path_bytes(self.h, batch))

    def flops(self, batch: int) -> int:
        return int(self._L.llie_flops(self.h, batch))

    def profile_begin(self, class_mask: int) -> None:
        check(self._L.llie_profile_begin(self.h, class_mask), "profile_begin")

    def profile_report(self):
        """-> {kernel name: (total device ms, launches, algorithmic bytes)} of the recorded launches."""
        buf = C.create_string_buffer(1 << 16)
        check(self._L.llie_profile_report(self.h, buf, len(buf)), "profile_report")
        out = {}
        for line in buf.value.decode().splitlines():
            name, ms, n, b = line.split("\t")
            out[name] = (float(ms), int(n), int(b))
        return out

    def profile_dump(self):
        """-> [(class, kernel name, operator tag, device ms, algorithmic bytes)] of every recorded launch, in launch order."""
        buf = C.create_string_buffer(1 << 21)
        check(self._L.llie_profile_dump(self.h, buf, len(buf)), "profile_dump")
        out = []
        for line in buf.value.decode().splitlines():
            cls, name, tag, ms, b = line.split("\t")
            out.append((int(cls), name, tag, float(ms), int(b)))
        return out

    def profile_end(self, kernel_class: int):
        """-> (total device ms, launches, algorithmic bytes) of the recorded launches of `kernel_class`."""
        ms, n, b = C.c_double(), C.c_int64(), C.c_int64()
        check(self._L.llie_profile_end(self.h, kernel_class, C.byref(ms), C.byref(n), C.byref(b)), "profile_end")
        return ms.value, int(n.value), int(b.value)
