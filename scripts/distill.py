#!/usr/bin/env python3
"""Consistency distillation on the MI355X engine: a trained many-step teacher -> a 4-8-step student, LowLightDistiller over the
device-resident loaders.

  python scripts/distill.py --teacher checkpoints/best_model.pt --data_dir LOL/our485 --val_dir LOL/eval15 --num_steps 4

The data / model / run flags are scripts/train.py's (--variant, --image_size and --attention describe the student; --loss,
--use_ema, --ema_decay, --x0_*_weight and --sampler have no meaning here and are not offered).  --teacher is the teacher's
checkpoint (a trainer's, or a bare state_dict), --teacher_variant / --teacher_attention its network where it differs from the
student's, --teacher_prediction / --student_prediction what each network's output means (epsilon or v_prediction; a teacher
trained with TrainStep(use_velocity_target=True) is v_prediction).  --init_student starts the student (and the EMA target) from
a checkpoint, usually the teacher's own when the variants agree; without it the student starts from --seed's random weights.
--num_ddim_timesteps is the teacher's DDIM grid (50), --num_steps the step count distilled for, --target_ema_decay the decay of
the EMA target network (0.95).  --guidance_scale_range LO HI distils the classifier-free-guided teacher (a teacher trained
with train.py --cond_dropout): each sample's scale is uniform in [LO, HI], and LO = HI is the normal use; --guidance_rescale PHI adds guidance rescale to that
teacher (0.7 is the usual value).  --crop_height / --crop_width distil at a frame's own shape; --accumulate as in train.py.

Checkpoints have the trainer's names (checkpoint_epoch_{e}.pt, best_model.pt by validation PSNR, final_model.pt); their
"model_state_dict" is the EMA student, so

  python scripts/inference.py --checkpoint checkpoints/final_model.pt --input dark.png --output out.png [--prediction v_prediction]

runs the student as it is.  One JSON line per epoch is printed: epoch, train_loss, lr, psnr, ssim.
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
hostio = importlib.import_module("cv-diffusion-model_amd.hostio")

PREDICTIONS = ["epsilon", "v_prediction"]


def build_parser() -> argparse.ArgumentParser:
    p = argparse.ArgumentParser(description="Distil a Low-Light Enhancement teacher into a few-step consistency student")
    # Data
    p.add_argument("--data_dir", type=str, default="src/data/our485", help="Dataset directory (default: src/data/our485)")
    p.add_argument("--val_dir", type=str, default="src/data/eval15", help="Validation directory (default: src/data/eval15)")
    # The student
    p.add_argument("--variant", type=str, default="small", choices=["tiny", "small", "base", "large"], help="Student variant")
    p.add_argument("--image_size", type=int, default=256, help="Image size (teacher and student)")
    p.add_argument("--attention", type=str, default="linear", choices=["linear", "softmax"], help="attention of the student's network")
    p.add_argument("--num_steps", type=int, default=4, help="inference steps the student is distilled for")
    p.add_argument("--student_prediction", type=str, default="epsilon", choices=PREDICTIONS, help="what the student predicts")
    p.add_argument("--init_student", type=str, default=None, help="checkpoint the student and the EMA target start from")
    # The teacher
    p.add_argument("--teacher", type=str, required=True, help="the teacher's checkpoint")
    p.add_argument("--teacher_variant", type=str, default=None, choices=["tiny", "small", "base", "large"],
                   help="the teacher's variant (default: --variant)")
    p.add_argument("--teacher_attention", type=str, default=None, choices=["linear", "softmax"],
                   help="attention of the teacher's network (default: --attention)")
    p.add_argument("--teacher_prediction", type=str, default="epsilon", choices=PREDICTIONS, help="what the teacher predicts")
    # Distillation
    p.add_argument("--num_ddim_timesteps", type=int, default=50, help="the teacher's DDIM grid")
    p.add_argument("--target_ema_decay", type=float, default=0.95, help="decay of the EMA target network")
    # Training
    p.add_argument("--epochs", type=int, default=100, help="Number of epochs")
    p.add_argument("--batch_size", type=int, default=8, help="Batch size")
    p.add_argument("--lr", type=float, default=1e-4, help="Learning rate")
    p.add_argument("--use_amp", action="store_true", help="Use mixed precision (fp16 engines with a loss scaler)")
    # Logging
    p.add_argument("--output_dir", type=str, default="outputs", help="Output directory")
    p.add_argument("--use_wandb", action="store_true", help="Log to W&B")
    p.add_argument("--project", type=str, default="low-light-diffusion", help="W&B project")
    # Resume
    p.add_argument("--resume", type=str, default=None, help="Resume from a distiller checkpoint")
    # This engine's additions
    p.add_argument("--dtype", type=str, default=None, choices=["fp32", "fp16", "bf16"],
                   help="engine precision of all three networks (default: fp16 with --use_amp, else fp32)")
    p.add_argument("--seed", type=int, default=0, help="seed of the student's initial weights and of every draw")
    p.add_argument("--use_synthetic", action="store_true", help="synthetic low-light twins of the images in --data_dir")
    p.add_argument("--checkpoint_dir", type=str, default="checkpoints", help="Checkpoint directory")
    p.add_argument("--save_interval", type=int, default=5, help="epochs between checkpoint_epoch_{e}.pt files")
    p.add_argument("--sample_interval", type=int, default=1, help="epochs between sample sheets")
    p.add_argument("--crop_height", type=int, default=None, help="distil at crops of this height (with --crop_width) instead of --image_size squares")
    p.add_argument("--crop_width", type=int, default=None, help="the width that goes with --crop_height")
    p.add_argument("--accumulate", type=int, default=1,
                   help="batches per optimiser step (gradient accumulation; >= 1): the effective batch is --accumulate x --batch_size")
    p.add_argument("--guidance_scale_range", type=float, nargs=2, default=None, metavar=("LO", "HI"),
                   help="distil the classifier-free-guided teacher: each sample's teacher output is o_u + w (o_c - o_u) with w "
                        "uniform in [LO, HI] (LO = HI, one scale, is the normal use); the student then needs no second forward. "
                        "Default: off")
    p.add_argument("--guidance_rescale", type=float, default=None,
                   help="with --guidance_scale_range: distil the teacher with guidance rescale phi in [0, 1] (Lin et al. 2024): its "
                        "guided output is scaled by phi std(o_c) / std(o) + (1 - phi) per sample, so the student does not inherit the "
                        "over-exposure of a large w (0.7 is the paper's value).  Default: off")
    return p


def parse_args(argv=None):
    p = build_parser()
    args = p.parse_args(argv)
    if (args.crop_height is None) != (args.crop_width is None):
        p.error("--crop_height and --crop_width go together: both or neither")
    if args.accumulate < 1:
        p.error("--accumulate must be >= 1")
    if not 0.0 <= args.target_ema_decay <= 1.0:
        p.error("--target_ema_decay must be in [0, 1]")
    if args.guidance_scale_range is not None:
        lo, hi = args.guidance_scale_range
        if not (math.isfinite(lo) and math.isfinite(hi) and lo <= hi):
            p.error("--guidance_scale_range LO HI: finite, LO <= HI")
        args.guidance_scale_range = (lo, hi)
    if args.guidance_rescale is not None:
        if not 0.0 <= args.guidance_rescale <= 1.0:
            p.error("--guidance_rescale must be in [0, 1]")
        if args.guidance_scale_range is None and args.guidance_rescale != 0:
            p.error("--guidance_rescale needs --guidance_scale_range")
    if args.teacher_variant is None:
        args.teacher_variant = args.variant
    if args.teacher_attention is None:
        args.teacher_attention = args.attention
    return args


def config_from_args(args) -> "M.TrainingConfig":
    """The TrainingConfig LowLightDistiller reads (use_ema is off: the target network is the only EMA)."""
    return M.TrainingConfig(
        unet_variant=args.variant, image_size=args.image_size, num_inference_steps=args.num_steps,
        epochs=args.epochs, batch_size=args.batch_size, learning_rate=args.lr, use_amp=args.use_amp, use_ema=False,
        save_interval=args.save_interval, sample_interval=args.sample_interval,
        output_dir=args.output_dir, checkpoint_dir=args.checkpoint_dir,
        use_wandb=args.use_wandb, wandb_project=args.project, resume_from=args.resume,
        compute_dtype=args.dtype, seed=args.seed, use_synthetic=args.use_synthetic)


def distiller_keywords(args) -> dict:
    """LowLightDistiller's keywords beside the config."""
    return {"num_inference_steps": args.num_steps, "ema_decay": args.target_ema_decay,
            "crop_size": None if args.crop_height is None else (args.crop_height, args.crop_width), "accumulate": args.accumulate}


def guidance_keywords(args) -> dict:
    """LowLightLCMDistillation's guidance keywords: nothing without --guidance_scale_range (the range stays stored and unused)."""
    r, phi = getattr(args, "guidance_scale_range", None), getattr(args, "guidance_rescale", None)
    if r is None:
        return {}
    kw = {"guidance_scale_range": tuple(r), "guidance": True}
    if phi is not None:
        kw["guidance_rescale"] = phi
    return kw


def build_network(variant: str, attention: str, prediction: str, image_size: int, num_steps: int) -> "M.LowLightDiffusion":
    unet = None
    if attention == "softmax":
        unet = M.create_efficient_unet(variant, image_size, in_channels=6, use_linear_attention=False)
    scheduler = M.LCMScheduler(num_train_timesteps=1000, beta_schedule="scaled_linear", prediction_type=prediction,
                               num_inference_steps=num_steps, rescale_betas_zero_snr=True)
    return M.LowLightDiffusion(unet=unet, scheduler=scheduler, unet_variant=variant, image_size=image_size, num_inference_steps=num_steps)


def main(argv=None) -> int:
    args = parse_args(argv)
    config = config_from_args(args)
    if not torch.cuda.is_available():
        raise SystemExit("scripts/distill.py distils on a HIP device; there is no CPU fallback")
    print("=" * 60)
    print("Low-Light Enhancement Consistency Distillation")
    print("=" * 60)
    print(f"\nLoading data from: {args.data_dir}")
    val_dir = args.val_dir if args.val_dir and os.path.isdir(args.val_dir) else None
    crop = distiller_keywords(args)["crop_size"]
    train_loader, val_loader = M.create_device_dataloaders(train_root=args.data_dir, val_root=val_dir, batch_size=args.batch_size,
                                                           image_size=args.image_size if crop is None else crop,
                                                           use_synthetic=args.use_synthetic, seed=args.seed)
    print(f"  Train batches: {len(train_loader)}")
    if val_loader is not None:
        print(f"  Val batches: {len(val_loader)}")

    teacher = build_network(args.teacher_variant, args.teacher_attention, args.teacher_prediction, args.image_size, args.num_steps)
    hostio.load_checkpoint(teacher, args.teacher)
    torch.manual_seed(args.seed)  # the student's initial weights
    student = build_network(args.variant, args.attention, args.student_prediction, args.image_size, args.num_steps)
    if args.init_student:
        hostio.load_checkpoint(student, args.init_student)
    distill = M.LowLightLCMDistillation(teacher, student, num_ddim_timesteps=args.num_ddim_timesteps,
                                        **guidance_keywords(args)).to(train_loader.store.device)
    print(f"  Teacher: {args.teacher_variant} ({args.teacher_prediction}), student: {args.variant} ({args.student_prediction}), "
          f"{student.get_model_size()['num_params']:,} parameters")

    distiller = M.LowLightDistiller(distill, train_loader, val_loader, config, **distiller_keywords(args))
    print(f"  Engine precision: {student.compute_dtype}, loss scaler: {distiller.scaler is not None}, "
          f"skip_terminal: {distiller.skip_terminal}")
    distiller.train(on_epoch=lambda log: print(json.dumps(log), flush=True))
    print("\nDistillation complete!")
    print(f"Checkpoints saved to: {config.checkpoint_dir}")
    print(f"Samples saved to: {config.output_dir}")
    return 0


if __name__ == "__main__":
    sys.exit(main())
