#!/usr/bin/env python3
"""Image / folder enhancement CLI on the MI355X engine -- flag-compatible counterpart of the reference's
scripts/inference.py (:30-62): --input --output --checkpoint --model --format --variant --image_size
--num_steps --device.  Only --format pytorch exists here (ONNX / TFLite are the reference's mobile
deployment targets, out of scope); extensions: --dtype {fp32,fp16,bf16}, --noise_seed, --sampler {lcm,ddim,dpmpp_2m} (ddim: the
deterministic sampler of a many-step model, --num_steps anything in 1..1000; dpmpp_2m: the second-order sampler of such a model,
up to 32 steps with the default table), --prediction {epsilon,v_prediction} (what the
network's output means: a v-prediction teacher, or the v student scripts/distill.py --student_prediction v_prediction writes), and --tile [--tile_overlap N]
[--tile_batch N] [--tile_sync {none,latents}] [--tile_size {auto|HxW}], which enhances the image at its own resolution as
overlapping image_size tiles instead of resizing it (--tile_sync latents: the tiles share one latent canvas, fused after every
step; --tile_size: the tiles are frames of H x W, or with auto the fewest frames the engine can run -- three for 12 MP), and
--native, which enhances it at its own resolution by one run of the network at that size (frame mode; images under the engine's
size cap, about 5.59 M pixels for `small`).  --native and the tile flags exclude each other.
"""
import argparse
import math
import importlib
import os
import sys
import time
from pathlib import Path

import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
M = importlib.import_module("cv-diffusion-model_amd")
hostio = importlib.import_module("cv-diffusion-model_amd.hostio")
tiling = importlib.import_module("cv-diffusion-model_amd.tiling")


def parse_args(argv=None):
    p = argparse.ArgumentParser(description="Low-Light Enhancement Inference (HIP engine)")
    p.add_argument("--input", type=str, required=True, help="Input image or folder")
    p.add_argument("--output", type=str, required=True, help="Output image or folder")
    p.add_argument("--checkpoint", type=str, default=None, help="PyTorch checkpoint")
    p.add_argument("--model", type=str, default=None, help="(reference flag; exported ONNX/TFLite models are not supported)")
    p.add_argument("--format", type=str, default="pytorch", choices=["pytorch", "onnx", "tflite"])
    p.add_argument("--variant", type=str, default="small")
    p.add_argument("--image_size", type=int, default=256)
    p.add_argument("--attention", type=str, default="linear", choices=["linear", "softmax"],
                   help="attention of the network the checkpoint holds: LinearAttention (default) or StandardAttention "
                        "(use_linear_attention=False)")
    p.add_argument("--num_steps", type=int, default=4)
    p.add_argument("--device", type=str, default="cuda" if torch.cuda.is_available() else "cpu")
    p.add_argument("--dtype", type=str, default="fp32", choices=["fp32", "fp16", "bf16"], help="engine precision (extension)")
    p.add_argument("--noise_seed", type=int, default=None,
                   help="(extension) draw the loop's noise on the CPU generator with this seed, in the reference's order, "
                        "instead of on the device: makes a run reproducible against the CPU reference")
    p.add_argument("--sampler", type=str, default="lcm", choices=["lcm", "ddim", "dpmpp_2m"],
                   help="(extension) lcm = the consistency student's loop (re-noise after every step); ddim = the deterministic "
                        "DDIM loop of a many-step epsilon- / v-prediction model: --num_steps may be anything in 1..1000 and "
                        "the initial latents are the only noise; dpmpp_2m = DPM-Solver++ 2M for the same models: second order, "
                        "a grid uniform in log-SNR, at most 32 steps with the default table, not with --tile_sync latents")
    p.add_argument("--prediction", type=str, default="epsilon", choices=["epsilon", "v_prediction"],
                   help="(extension) what the checkpoint's network predicts: epsilon (the default, the reference's models) or "
                        "v_prediction (a model trained or distilled as a v network)")
    p.add_argument("--tile", action="store_true",
                   help="(extension) no resize: enhance the image at its own resolution as overlapping image_size tiles, blended "
                        "on the device; --noise_seed then seeds the per-image noise canvas")
    p.add_argument("--tile_overlap", type=int, default=None, help="overlap of neighbouring tiles in pixels (default image_size // 8)")
    p.add_argument("--tile_batch", type=int, default=32, help="tiles per enhance call")
    p.add_argument("--tile_sync", type=str, default="none", choices=["none", "latents"],
                   help="with --tile: latents = keep one latent canvas per image and fuse the tiles' predictions into it after "
                        "every step, so neighbours agree where they overlap; none = each tile runs its own loop")
    p.add_argument("--tile_size", type=str, default=None, metavar="{auto|HxW}",
                   help="with --tile: tiles of H x W (multiples of 8, at least 64) run as frames instead of image_size squares; "
                        "auto = the fewest such tiles under the engine's size cap, overlapping by an eighth (--tile_overlap "
                        "is then chosen for you)")
    p.add_argument("--native", action="store_true",
                   help="(extension) no resize and no tiles: one run of the network at the image's own resolution (frame mode); "
                        "--noise_seed then seeds the noise canvas at the padded size")
    p.add_argument("--guidance_scale", type=float, default=None,
                   help="(extension) classifier-free guidance scale w: every step uses o_u + w (o_c - o_u), o_u the output on the "
                        "all-zero condition (a second forward per step; for a model trained with --cond_dropout).  Default: off")
    p.add_argument("--guidance_rescale", type=float, default=None,
                   help="(extension) guidance rescale phi in [0, 1] (Lin et al. 2024): with --guidance_scale, the guided output of each "
                        "image and step is scaled by phi std(o_c) / std(o) + (1 - phi), which removes the over-exposure of a large w "
                        "(0.7 is the paper's value).  Default: off")
    args = p.parse_args(argv)
    if args.guidance_scale is not None and not math.isfinite(args.guidance_scale):
        p.error("--guidance_scale must be finite")
    if args.guidance_rescale is not None and not 0.0 <= args.guidance_rescale <= 1.0:
        p.error("--guidance_rescale must be in [0, 1]")
    if args.guidance_scale not in (None, 1.0) and args.tile_sync == "latents":
        p.error("--guidance_scale and --tile_sync latents exclude each other")
    if args.sampler == "dpmpp_2m" and args.tile_sync == "latents":
        p.error("--sampler dpmpp_2m and --tile_sync latents exclude each other")
    if args.native and (args.tile or args.tile_overlap is not None or args.tile_batch != 32 or args.tile_sync != "none"
                        or args.tile_size is not None):
        p.error("--native and --tile / --tile_overlap / --tile_batch / --tile_sync / --tile_size exclude each other")
    if args.tile_sync != "none" and not args.tile:
        p.error("--tile_sync belongs to --tile")
    if args.tile_size is not None:
        if not args.tile:
            p.error("--tile_size belongs to --tile")
        try:
            args.tile_size = tiling.parse_tile_size(args.tile_size)
        except ValueError as e:
            p.error(str(e))
        if args.tile_size == "auto" and args.tile_overlap is not None:
            p.error("--tile_size auto chooses the overlap; drop --tile_overlap")
    return args


def load_model(args):
    if args.format != "pytorch":
        raise SystemExit(f"--format {args.format}: exported-model runtimes are outside this engine's scope; use --format pytorch")
    unet = None
    if getattr(args, "attention", "linear") == "softmax":
        unet = M.create_efficient_unet(args.variant, args.image_size, in_channels=6, use_linear_attention=False)
    scheduler = None
    if getattr(args, "prediction", "epsilon") != "epsilon":  # the default scheduler is the epsilon one, as before
        scheduler = M.LCMScheduler(num_train_timesteps=1000, beta_schedule="scaled_linear", prediction_type=args.prediction,
                                   num_inference_steps=4, rescale_betas_zero_snr=True)
    model = M.LowLightDiffusion(unet=unet, scheduler=scheduler, unet_variant=args.variant, image_size=args.image_size,
                                num_inference_steps=4, compute_dtype=args.dtype)
    if args.checkpoint:
        hostio.load_checkpoint(model, args.checkpoint)
    return model.to(args.device).eval()


def guided(args) -> dict:
    """--guidance_scale and --guidance_rescale as the `guidance_scale=` / `guidance_rescale=` keywords of the enhance calls
    (nothing without the flags)."""
    w, phi = getattr(args, "guidance_scale", None), getattr(args, "guidance_rescale", None)
    kw = {} if w is None else {"guidance_scale": w}
    if phi is not None:
        kw["guidance_rescale"] = phi
    return kw


def noise_entries(args) -> int:
    """Entries of the noise --noise_seed draws: one per step for the LCM loop, the initial latents alone for DDIM and
    DPM-Solver++."""
    return args.num_steps if args.sampler == "lcm" else 1


def enhance_tiled_image(args, model, rgb):
    """--tile: uint8 [H,W,3] -> uint8 [H,W,3] at the input's resolution."""
    noise = None
    if args.noise_seed is not None:  # the canvas every tile reads its noise from, drawn entry by entry in enhance's order
        g = torch.Generator().manual_seed(args.noise_seed)
        sh, sw, _, _ = tiling.resolve_tile_plan(model, rgb.shape[:2], args.tile_size, args.tile_overlap)
        hc, wc = max(rgb.shape[0], sh), max(rgb.shape[1], sw)
        noise = torch.stack([torch.randn(3, hc, wc, generator=g) for _ in range(noise_entries(args))])
    out = tiling.enhance_tiled(model, torch.from_numpy(rgb).to(args.device), args.num_steps, overlap=args.tile_overlap,
                               tile_batch=args.tile_batch, noise=noise, sync=args.tile_sync, sampler=args.sampler,
                               tile=args.tile_size, **guided(args))
    return out.cpu().numpy()


def enhance_native_image(args, model, rgb):
    """--native: uint8 [H,W,3] -> uint8 [H,W,3] at the input's resolution, one run of the network (frame mode)."""
    noise = None
    if args.noise_seed is not None:  # the canvas at the padded size, drawn entry by entry in enhance's order
        g = torch.Generator().manual_seed(args.noise_seed)
        hp, wp = tiling.frame_pad(rgb.shape[0]), tiling.frame_pad(rgb.shape[1])
        noise = torch.stack([torch.randn(3, hp, wp, generator=g) for _ in range(noise_entries(args))])
    out = tiling.enhance_frame_u8(model, torch.from_numpy(rgb).to(args.device), args.num_steps, noise=noise, sampler=args.sampler, **guided(args))
    return out.cpu().numpy()


def enhance_resized_image(args, model, rgb):
    """The reference's path: squash to image_size, enhance, stretch back to the input's size."""
    original = rgb.shape[:2]
    with torch.no_grad():
        # uint8 goes up, uint8 comes back: resize + normalise / denormalise run on the device
        # (bit-exact twins of hostio.preprocess_array / postprocess_array, i.e. inference.py:99-134)
        x = hostio.preprocess_device(torch.from_numpy(rgb).to(args.device), args.image_size)
        noise = None
        if args.noise_seed is not None:  # reference draw order: initial latents, then one draw per non-final step
            g = torch.Generator().manual_seed(args.noise_seed)
            noise = torch.stack([torch.randn(1, 3, args.image_size, args.image_size, generator=g) for _ in range(noise_entries(args))])
        enhanced = model.enhance(x, num_inference_steps=args.num_steps, noise=noise, sampler=args.sampler, **guided(args))
        return hostio.postprocess_device(enhanced, original)[0].cpu().numpy()


def process_single_image(args, model, input_path: str, output_path: str) -> float:
    print(f"Processing: {input_path}")
    rgb = hostio.load_image(input_path)
    start = time.perf_counter()
    if args.native:
        out = enhance_native_image(args, model, rgb)
    else:
        out = enhance_tiled_image(args, model, rgb) if args.tile else enhance_resized_image(args, model, rgb)
    elapsed = time.perf_counter() - start
    hostio.save_image(output_path, out)
    print(f"  Saved to: {output_path}")
    print(f"  Time: {elapsed * 1000:.1f} ms")
    return elapsed


def main(argv=None):
    args = parse_args(argv)
    print("=" * 60)
    print("Low-Light Enhancement Inference")
    print("=" * 60)
    print(f"\nLoading model ({args.format})...")
    model = load_model(args)
    print("Model loaded!")
    inp, out = Path(args.input), Path(args.output)
    if inp.is_file():
        out.parent.mkdir(parents=True, exist_ok=True)
        process_single_image(args, model, str(inp), str(out))
    elif inp.is_dir():
        out.mkdir(parents=True, exist_ok=True)
        images = sorted(f for f in inp.iterdir() if f.suffix.lower() in {".jpg", ".jpeg", ".png", ".bmp"})
        print(f"\nProcessing {len(images)} images...")
        total = sum(process_single_image(args, model, str(f), str(out / f.name)) for f in images)
        if images:
            avg = total / len(images) * 1000
            print(f"\nAverage time per image: {avg:.1f} ms")
            print(f"Throughput: {1000 / avg:.1f} FPS")
    else:
        print(f"Error: {inp} not found")
        return 1
    print("\nDone!")
    return 0


if __name__ == "__main__":
    sys.exit(main())
