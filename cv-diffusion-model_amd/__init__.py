"""MI355X-native engine for the LCM denoising hot path of zamazincode/cv-diffusion-model.

Public names mirror `src/models/__init__.py:1-10` of the reference (LowLightDiffusion, EfficientUNet,
EfficientUNetConfig, LCMScheduler) plus the operator classes of efficient_unet.py.  Compute lives in
`libllie_hip.so` (hand-written HIP for gfx950, C ABI in include/llie.h); importing this package does
not need a GPU, running anything does.

The directory name contains '-', so import it as `import cv_diffusion_model_amd` (alias module at the
repository root) or `importlib.import_module("cv-diffusion-model_amd")`.
"""
from .unet import (EfficientUNet, EfficientUNetConfig, create_efficient_unet, InvertedResidualBlock,
                   LinearAttention, StandardAttention, Downsample, Upsample, SqueezeExcitation)
from .scheduler import LCMScheduler, LCMSchedulerOutput, LCMDenoisingLoop, get_lcm_timesteps
from .ddim import ddim_timesteps, ddim_step_host, ddim_enhance_host
from .dpm import dpm_timesteps, dpm_max_steps, dpm_step_coefficients, dpm_step_host, dpm_step_f32, dpm_enhance_host
from .guidance import (guide_array, cond_dropout_array, guidance_pair_array, scheduler_step_array, guided_enhance_host,
                       check_guidance_scale, check_cond_dropout, check_guidance_range, guide_device, guidance_pair_device,
                       cond_dropout_device, check_guidance_rescale, guided_keyword, guide_rescale_host, guide_rescale_array,
                       guide_rescale_device)
from .snrloss import (check_snr_gamma, snr_weight_array, snr_loss_host, snr_loss_f32, snr_loss_device, snr_loss_chunk)
from .pipeline import (LowLightDiffusion, LowLightDiffusionOutput, LowLightLCMDistillation, normalize_image,
                       denormalize_image, x0_loss, x0_loss_host, consistency_target_host, consistency_loss_host)
from .sharding import shard_range, enhance_sharded, all_gather_batch, all_reduce_gradients
from .training import (FusedAdamW, FusedGradScaler, TrainStep, DistillStep, grad_accumulate_array,
                       accumulation_windows)
from .build import build_library, library_path
from . import ops  # registers torch.ops.llie.*
from .ops import register_model
from .hostio import (load_checkpoint, extract_state_dict, preprocess_array, postprocess_array, resize_bilinear,
                     preprocess_device, postprocess_device)
from .tiling import (tile_origins, gather_tiles_array, blend_tiles_array, gather_tiles_device, gather_noise_device,
                     blend_tiles_device, enhance_tiled, frame_pad, frame_load_array, frame_store_array, frame_load_device,
                     frame_store_device, enhance_frame_u8, sync_step_array, canvas_store_array, enhance_tiled_sync_array,
                     sync_step_device, auto_tile_plan)
from .data import (DeviceFrameStore, DevicePairLoader, create_device_dataloaders, epoch_plan, augment_pairs_host, augment_synth_host,
                   augment_pairs_device, augment_synth_device)
from .metrics import (ImageMetrics, image_metrics, image_metrics_host, evaluate, evaluate_full_resolution, ssim_loss,
                      ssim_grad_host)
from .trainer import (TrainingConfig, LowLightTrainer, train_model, make_lr_scheduler, build_checkpoint, comparison_grid,
                      comparison_grid_host, distill_draw_seed)
from .distiller import LowLightDistiller, timestep_index_range, default_skip_terminal

__all__ = [
    "EfficientUNet", "EfficientUNetConfig", "create_efficient_unet", "InvertedResidualBlock", "LinearAttention", "StandardAttention", "SqueezeExcitation",
    "Downsample", "Upsample", "LCMScheduler", "LCMSchedulerOutput", "LCMDenoisingLoop", "get_lcm_timesteps", "LowLightDiffusion",
    "LowLightDiffusionOutput", "LowLightLCMDistillation", "normalize_image", "denormalize_image", "shard_range", "enhance_sharded",
    "all_gather_batch", "all_reduce_gradients", "FusedAdamW", "FusedGradScaler", "TrainStep", "DistillStep", "grad_accumulate_array", "accumulation_windows", "register_model", "build_library", "library_path", "load_checkpoint", "extract_state_dict",
    "preprocess_array", "postprocess_array", "resize_bilinear", "preprocess_device", "postprocess_device",
    "tile_origins", "gather_tiles_array", "blend_tiles_array", "gather_tiles_device", "gather_noise_device", "blend_tiles_device",
    "enhance_tiled", "frame_pad", "frame_load_array", "frame_store_array", "frame_load_device", "frame_store_device", "enhance_frame_u8",
    "sync_step_array", "canvas_store_array", "enhance_tiled_sync_array", "sync_step_device", "auto_tile_plan",
    "DeviceFrameStore", "DevicePairLoader", "create_device_dataloaders", "epoch_plan", "augment_pairs_host", "augment_synth_host",
    "augment_pairs_device", "augment_synth_device",
    "ImageMetrics", "image_metrics", "image_metrics_host", "evaluate", "evaluate_full_resolution",
    "ssim_loss", "ssim_grad_host", "x0_loss", "x0_loss_host", "consistency_target_host", "consistency_loss_host",
    "TrainingConfig", "LowLightTrainer", "train_model", "make_lr_scheduler", "build_checkpoint", "comparison_grid",
    "comparison_grid_host", "distill_draw_seed", "LowLightDistiller", "timestep_index_range", "default_skip_terminal",
    "ddim_timesteps", "ddim_step_host", "ddim_enhance_host",
    "dpm_timesteps", "dpm_max_steps", "dpm_step_coefficients", "dpm_step_host", "dpm_step_f32", "dpm_enhance_host",
    "guide_array", "cond_dropout_array", "guidance_pair_array", "scheduler_step_array", "guided_enhance_host",
    "check_guidance_scale", "check_cond_dropout", "check_guidance_range", "guide_device", "guidance_pair_device", "cond_dropout_device",
    "check_guidance_rescale", "guided_keyword", "guide_rescale_host", "guide_rescale_array", "guide_rescale_device",
    "check_snr_gamma", "snr_weight_array", "snr_loss_host", "snr_loss_f32", "snr_loss_device", "snr_loss_chunk",
]
