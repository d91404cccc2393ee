#!/usr/bin/env python3
"""PSNR / SSIM of a checkpoint on a paired validation folder, on the MI355X engine -- the sibling of scripts/inference.py.

  python scripts/evaluate.py --data LOL/eval15 --checkpoint ckpt.pt [--full_resolution [frame]] [--per_image] [--output result.json]

--data is the layout DeviceFrameStore.from_folder reads (ROOT/low and ROOT/high, or lowlight / dark and normal / bright).  By
default every pair is centre-cropped to --image_size and goes through `evaluate` in batches of --batch_size (the result then
also holds the validation loss); --full_resolution scores every image at its own size through `evaluate_full_resolution`
(overlapping tiles, --tile_overlap / --tile_batch / --tile_size as in inference.py; `--full_resolution frame` runs the network once per image
at the image's own size instead, frame mode, and excludes the tile flags).  One JSON line is printed, and written to --output when
given; the per-image lists are part of it only under --per_image.  --seed seeds every draw, so a run is reproducible.
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
sys.path.insert(0, os.path.join(ROOT, "scripts"))
import inference  # noqa: E402  (model loading is shared with the enhancement CLI)

M = importlib.import_module("cv-diffusion-model_amd")


def build_parser() -> argparse.ArgumentParser:
    p = argparse.ArgumentParser(description="Low-Light Enhancement Evaluation: PSNR / SSIM on a paired folder (HIP engine)")
    p.add_argument("--data", type=str, required=True, help="paired data set root (low/ and high/ inside)")
    p.add_argument("--checkpoint", type=str, default=None, help="PyTorch checkpoint")
    p.add_argument("--variant", type=str, default="small")
    p.add_argument("--image_size", type=int, default=256)
    p.add_argument("--num_steps", type=int, default=4)
    p.add_argument("--dtype", type=str, default="fp32", choices=["fp32", "fp16", "bf16"], help="engine precision")
    p.add_argument("--device", type=str, default="cuda" if torch.cuda.is_available() else "cpu")
    p.add_argument("--batch_size", type=int, default=8, help="images per enhance call (centre-crop evaluation)")
    p.add_argument("--seed", type=int, default=0, help="seed of every noise draw")
    p.add_argument("--full_resolution", nargs="?", const="tiled", default=None, choices=["tiled", "frame"],
                   help="score every image at its own size: enhanced as overlapping tiles (the default), or `frame`: by one run of "
                        "the network at that size")
    p.add_argument("--tile_overlap", type=int, default=None, help="overlap of neighbouring tiles in pixels (default image_size // 8)")
    p.add_argument("--tile_batch", type=int, default=32, help="tiles per enhance call")
    p.add_argument("--per_image", action="store_true", help="keep the per-image lists in the result")
    p.add_argument("--output", type=str, default=None, help="also write the JSON line to this file")
    return p


def parse_args(argv=None):
    p = build_parser()
    # tests/test_metrics_host.py pins build_parser()'s flags as an exact set, so the sampler flag joins the parser here
    p.add_argument("--sampler", type=str, default="lcm", choices=["lcm", "ddim", "dpmpp_2m"],
                   help="lcm = the consistency student's loop; ddim = the deterministic DDIM loop of a many-step model "
                        "(--num_steps anything in 1..1000); dpmpp_2m = DPM-Solver++ 2M for the same models (second order, at "
                        "most 32 steps with the default table)")
    p.add_argument("--tile_size", type=str, default=None, metavar="{auto|HxW}",
                   help="with --full_resolution [tiled]: tiles of H x W run as frames instead of image_size squares; auto = the "
                        "fewest such tiles under the engine's size cap")
    p.add_argument("--attention", type=str, default="linear", choices=["linear", "softmax"],
                   help="attention of the network the checkpoint holds (softmax: use_linear_attention=False)")
    p.add_argument("--guidance_scale", type=float, default=None, help="classifier-free guidance scale w: every step uses o_u + w (o_c - o_u), o_u the output on the "
                        "all-zero condition (a second forward per step; for a model trained with --cond_dropout).  Default: off")
    p.add_argument("--guidance_rescale", type=float, default=None,
                   help="guidance rescale phi in [0, 1] (Lin et al. 2024): with --guidance_scale, the guided output of each "
                        "image and step is scaled by phi std(o_c) / std(o) + (1 - phi), which removes the over-exposure of a large w "
                        "(0.7 is the paper's value).  Default: off")
    args = p.parse_args(argv)
    if args.guidance_scale is not None and not math.isfinite(args.guidance_scale):
        p.error("--guidance_scale must be finite")
    if args.guidance_rescale is not None and not 0.0 <= args.guidance_rescale <= 1.0:
        p.error("--guidance_rescale must be in [0, 1]")
    if args.full_resolution == "frame" and (args.tile_overlap is not None or args.tile_batch != 32 or args.tile_size is not None):
        p.error("--full_resolution frame and --tile_overlap / --tile_batch / --tile_size exclude each other")
    if args.tile_size is not None:
        if args.full_resolution != "tiled":
            p.error("--tile_size belongs to --full_resolution [tiled]")
        try:
            args.tile_size = inference.tiling.parse_tile_size(args.tile_size)
        except ValueError as e:
            p.error(str(e))
        if args.tile_size == "auto" and args.tile_overlap is not None:
            p.error("--tile_size auto chooses the overlap; drop --tile_overlap")
    return args


def main(argv=None) -> int:
    args = parse_args(argv)
    model = inference.load_model(argparse.Namespace(format="pytorch", **vars(args)))
    if args.full_resolution:
        store = M.DeviceFrameStore.from_folder(args.data, device=args.device)
        res = M.evaluate_full_resolution(model, store, num_inference_steps=args.num_steps, seed=args.seed, overlap=args.tile_overlap,
                                         tile_batch=args.tile_batch, mode=args.full_resolution, sampler=args.sampler,
                                         tile=args.tile_size, **inference.guided(args))
    else:
        store = M.DeviceFrameStore.from_folder(args.data, device=args.device, image_size=args.image_size)
        loader = M.DevicePairLoader(store, args.batch_size, args.image_size, "val")
        res = M.evaluate(model, loader, num_inference_steps=args.num_steps, seed=args.seed, sampler=args.sampler, **inference.guided(args))
    if not args.per_image:
        del res["per_image"]
    line = json.dumps(res)
    print(line)
    if args.output:
        os.makedirs(os.path.dirname(os.path.abspath(args.output)), exist_ok=True)
        with open(args.output, "w") as f:
            f.write(line + "\n")
    return 0


if __name__ == "__main__":
    sys.exit(main())
