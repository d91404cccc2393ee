#!/usr/bin/env python3
"""Training on the MI355X engine -- the reference's scripts/train.py over LowLightTrainer and the device-resident loaders.

  python scripts/train.py --data_dir LOL/our485 --val_dir LOL/eval15 --epochs 100 --use_ema [--use_amp | --dtype bf16]

--data_dir / --val_dir are the layout DeviceFrameStore.from_folder reads (ROOT/low and ROOT/high, or lowlight / dark and
normal / bright); a --val_dir that does not exist trains without validation, as the reference's create_dataloaders does.  With
--use_synthetic the normal-light images lie in --data_dir itself and the low-light twin is made on the device.  --use_amp is
the reference's fp16 with a loss scaler; --dtype pins the engine precision instead (bf16 needs no scaler).  --seed seeds every
draw, so a run is reproducible and --resume continues it bit for bit.  Checkpoints (checkpoint_epoch_{e}.pt, best_model.pt,
final_model.pt under --checkpoint_dir) are what scripts/inference.py and scripts/evaluate.py read; the per-epoch sample sheets go
to --output_dir.  One JSON line per epoch is printed: epoch, train_loss, lr, val_loss, psnr, ssim.

  python scripts/train.py --data_dir LOL/our485 --val_dir LOL/eval15 --x0_ssim_weight 0.5 --x0_l1_weight 0.5

adds the image-space term to --loss: SSIM / L1 of the clean image each step implies against the normal-light image (train_loss
then includes it; val_loss stays the MSE).  The two weights are not stored in checkpoints: pass them again with --resume.

  python scripts/train.py --data_dir LOL/our485 --val_dir LOL/eval15 --crop_height 400 --crop_width 600

trains at a frame's own shape, the one frame mode (scripts/inference.py --mode frame) runs at: crops of 400 x 600 instead of
--image_size squares, validation and sample sheets through enhance_frame.  Both flags or neither; multiples of 8, at least 64.
The model keeps the module tree --image_size fixed.  Like the x0 weights the shape is not stored in checkpoints.

  python scripts/train.py --data_dir LOL/our485 --crop_height 1080 --crop_width 1920 --batch_size 2 --accumulate 8

takes one optimiser step per window of 8 consecutive batches (gradient accumulation): an effective batch of 16 where one call
holds 2 frames.  The last window of an epoch holds what is left; the LR schedule moves once per window.  Not stored in
checkpoints: pass it again with --resume.
"""
import argparse
import math
import importlib
import json
import os
import sys

import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

M = importlib.import_module("cv-diffusion-model_amd")


def build_parser() -> argparse.ArgumentParser:
    p = argparse.ArgumentParser(description="Train Low-Light Enhancement Model")
    # Data
    p.add_argument("--data_dir", type=str, default="src/data/our485", help="Dataset directory (default: src/data/our485)")
    p.add_argument("--val_dir", type=str, default="src/data/eval15", help="Validation directory (default: src/data/eval15)")
    # Model
    p.add_argument("--variant", type=str, default="small", choices=["tiny", "small", "base", "large"], help="Model variant")
    p.add_argument("--image_size", type=int, default=256, help="Image size")
    p.add_argument("--attention", type=str, default="linear", choices=["linear", "softmax"],
                   help="attention of the network: LinearAttention (default) or StandardAttention (use_linear_attention=False)")
    p.add_argument("--num_steps", type=int, default=4, help="LCM inference steps")
    # Training
    p.add_argument("--epochs", type=int, default=100, help="Number of epochs")
    p.add_argument("--batch_size", type=int, default=8, help="Batch size")
    p.add_argument("--lr", type=float, default=1e-4, help="Learning rate")
    p.add_argument("--loss", type=str, default="mse", choices=["mse", "huber", "l1"], help="Loss function")
    # Optimization
    p.add_argument("--use_amp", action="store_true", help="Use mixed precision (fp16 engine with a loss scaler)")
    p.add_argument("--use_ema", action="store_true", help="Use EMA")
    p.add_argument("--ema_decay", type=float, default=0.9999, help="EMA decay")
    # Logging
    p.add_argument("--output_dir", type=str, default="outputs", help="Output directory")
    p.add_argument("--use_wandb", action="store_true", help="Log to W&B")
    p.add_argument("--project", type=str, default="low-light-diffusion", help="W&B project")
    # Resume
    p.add_argument("--resume", type=str, default=None, help="Resume from checkpoint")
    # This engine's additions
    p.add_argument("--dtype", type=str, default=None, choices=["fp32", "fp16", "bf16"],
                   help="engine precision (default: fp16 with --use_amp, else fp32)")
    p.add_argument("--seed", type=int, default=0, help="seed of the weights and of every draw")
    p.add_argument("--use_synthetic", action="store_true", help="synthetic low-light twins of the images in --data_dir")
    p.add_argument("--checkpoint_dir", type=str, default="checkpoints", help="Checkpoint directory")
    p.add_argument("--save_interval", type=int, default=5, help="epochs between checkpoint_epoch_{e}.pt files")
    p.add_argument("--sample_interval", type=int, default=1, help="epochs between sample sheets")
    p.add_argument("--x0_ssim_weight", type=float, default=0.0,
                   help="weight of 1 - SSIM of the predicted clean image against the normal-light image, added to --loss")
    p.add_argument("--x0_l1_weight", type=float, default=0.0, help="weight of the L1 distance of the same two images")
    p.add_argument("--sampler", type=str, default="lcm", choices=["lcm", "ddim", "dpmpp_2m"],
                   help="how validation and the sample sheet sample: lcm = the consistency student's loop; ddim = the deterministic "
                        "DDIM loop a many-step (teacher) model wants, with --num_steps steps (anything in 1..1000) in both; "
                        "dpmpp_2m = DPM-Solver++ 2M for the same models, with --num_steps steps (at most 32 with the default table)")
    p.add_argument("--crop_height", type=int, default=None, help="train at crops of this height (with --crop_width) instead of --image_size squares")
    p.add_argument("--crop_width", type=int, default=None, help="the width that goes with --crop_height")
    p.add_argument("--accumulate", type=int, default=1,
                   help="batches per optimiser step (gradient accumulation; >= 1): the effective batch is --accumulate x --batch_size")
    p.add_argument("--cond_dropout", type=float, default=0.0,
                   help="classifier-free guidance training: probability in [0, 1] of replacing a sample's low-light condition by the "
                        "all-zero image (0 = off)")
    p.add_argument("--guidance_scale", type=float, default=None,
                   help="guidance scale w of validation and of the sample sheet: o_u + w (o_c - o_u) at every step (default: off)")
    p.add_argument("--guidance_rescale", type=float, default=None,
                   help="guidance rescale phi in [0, 1] of validation and of the sample sheet (with --guidance_scale): the guided output "
                        "is scaled by phi std(o_c) / std(o) + (1 - phi) per image and step (default: off)")
    p.add_argument("--snr_gamma", type=float, default=None,
                   help="Min-SNR-gamma weighting of the training loss: each sample's --loss is weighted by min(SNR, gamma) / SNR "
                        "at its timestep (finite, > 0; 5 is the usual choice; default: off, every timestep counts the same)")
    return p


def parse_args(argv=None):
    p = build_parser()
    args = p.parse_args(argv)
    if (args.crop_height is None) != (args.crop_width is None):
        p.error("--crop_height and --crop_width go together: both or neither")
    if args.accumulate < 1:
        p.error("--accumulate must be >= 1")
    if not 0.0 <= args.cond_dropout <= 1.0:
        p.error("--cond_dropout must be in [0, 1]")
    if args.guidance_scale is not None and not math.isfinite(args.guidance_scale):
        p.error("--guidance_scale must be finite")
    if args.guidance_rescale is not None and not 0.0 <= args.guidance_rescale <= 1.0:
        p.error("--guidance_rescale must be in [0, 1]")
    if args.snr_gamma is not None and not (math.isfinite(args.snr_gamma) and args.snr_gamma > 0):
        p.error("--snr_gamma must be finite and > 0")
    return args


def config_from_args(args) -> "M.TrainingConfig":
    return M.TrainingConfig(
        unet_variant=args.variant, image_size=args.image_size, num_inference_steps=args.num_steps,
        epochs=args.epochs, batch_size=args.batch_size, learning_rate=args.lr, loss_type=args.loss,
        use_amp=args.use_amp, use_ema=args.use_ema, ema_decay=args.ema_decay,
        save_interval=args.save_interval, sample_interval=args.sample_interval,
        output_dir=args.output_dir, checkpoint_dir=args.checkpoint_dir,
        use_wandb=args.use_wandb, wandb_project=args.project, resume_from=args.resume,
        compute_dtype=args.dtype, seed=args.seed, use_synthetic=args.use_synthetic)


def x0_weights_from_args(args) -> dict:
    """The keywords LowLightTrainer and train_model take beside the config (not TrainingConfig fields, not in checkpoints:
    a run resumed with --resume passes the same two flags again)."""
    return {"x0_ssim_weight": args.x0_ssim_weight, "x0_l1_weight": args.x0_l1_weight}


def sampler_from_args(args) -> dict:
    """LowLightTrainer's sampling keywords (like the x0 weights: not TrainingConfig fields, not in checkpoints).  The LCM default
    keeps the trainer's own step counts; --sampler ddim / dpmpp_2m runs --num_steps steps of that sampler in validation and in the sample
    sheet."""
    return {"val_sampler": args.sampler, "val_steps": args.num_steps if args.sampler != "lcm" else None}


def guidance_from_args(args) -> dict:
    """LowLightTrainer's classifier-free guidance keywords (not TrainingConfig fields, not in checkpoints): --cond_dropout trains
    with the condition dropped, --guidance_scale samples validation and the sample sheet with guidance, --guidance_rescale adds
    the rescale to them (nothing without the flag)."""
    kw = {"cond_dropout": args.cond_dropout, "val_guidance_scale": args.guidance_scale}
    if getattr(args, "guidance_rescale", None) is not None:
        kw["val_guidance_rescale"] = args.guidance_rescale
    return kw


def snr_from_args(args) -> dict:
    """LowLightTrainer's `snr_gamma` keyword (like the x0 weights: not a TrainingConfig field, not in checkpoints; a run resumed
    with --resume passes the flag again): None without --snr_gamma."""
    return {"snr_gamma": args.snr_gamma}


def crop_size_from_args(args) -> dict:
    """LowLightTrainer's `crop_size` keyword (not a TrainingConfig field, not in checkpoints): (H, W) with both flags, else None."""
    return {"crop_size": None if args.crop_height is None else (args.crop_height, args.crop_width)}


def main(argv=None) -> int:
    args = parse_args(argv)
    config = config_from_args(args)
    if not torch.cuda.is_available():
        raise SystemExit("scripts/train.py trains on a HIP device; there is no CPU fallback")
    print("=" * 60)
    print("Low-Light Enhancement Diffusion Training")
    print("=" * 60)
    print(f"\nLoading data from: {args.data_dir}")
    val_dir = args.val_dir if args.val_dir and os.path.isdir(args.val_dir) else None
    crop = crop_size_from_args(args)["crop_size"]
    train_loader, val_loader = M.create_device_dataloaders(train_root=args.data_dir, val_root=val_dir, batch_size=args.batch_size,
                                                           image_size=args.image_size if crop is None else crop,
                                                           use_synthetic=args.use_synthetic, seed=args.seed)
    print(f"  Train batches: {len(train_loader)}")
    if val_loader is not None:
        print(f"  Val batches: {len(val_loader)}")

    torch.manual_seed(args.seed)  # the initial weights
    unet = None
    if args.attention == "softmax":
        unet = M.create_efficient_unet(args.variant, args.image_size, in_channels=6, use_linear_attention=False)
    model = M.LowLightDiffusion(unet=unet, unet_variant=args.variant, image_size=args.image_size, num_inference_steps=args.num_steps)
    model = model.to(train_loader.store.device)
    size = model.get_model_size()
    print(f"  Parameters: {size['num_params']:,}")

    trainer = M.LowLightTrainer(model=model, train_loader=train_loader, val_loader=val_loader, config=config,
                                **x0_weights_from_args(args), **sampler_from_args(args), crop_size=crop, accumulate=args.accumulate,
                                **guidance_from_args(args), **snr_from_args(args))
    print(f"  Engine precision: {model.compute_dtype}, loss scaler: {trainer.scaler is not None}, EMA: {config.use_ema}")
    trainer.train(on_epoch=lambda log: print(json.dumps(log), flush=True))
    print("\nTraining complete!")
    print(f"Checkpoints saved to: {config.checkpoint_dir}")
    print(f"Samples saved to: {config.output_dir}")
    return 0


if __name__ == "__main__":
    sys.exit(main())
