#!/usr/bin/env python3
"""Frame mode against tiles: one image enhanced at its own size by one run of the network (`enhance_frame_u8`) and by
`enhance_tiled` with its defaults, in one process.  One JSON line.

Defaults: small@256, fp16, 4 steps, synthetic weights (oracle.synth_state_dict), seeded dark images of the kind
tools/gpu_tiled_perf.py makes, at 400 x 600 and 1080 x 1920.  Per image size:

  frame_ms, tiled_ms     device-event times of the two calls end to end (noise draw, load / gathers, the loop, store / blend),
                         taken alternately after a warm-up that lets every shape capture its graph; medians of --iters
  frame_ms_per_mpix      frame_ms over the image's megapixels
  tiles, tile_mpix       what the tiles cost in pixels: count x S x S
  psnr_frame_vs_tiled    PSNR of the frame result against the tiled result on the bytes (x = byte / 255), same seed for both

and once:

  enhance_b4_ms          `enhance` at B = 4, 256 x 256 (about the pixel count of one 400 x 600 frame), same process, and its
  enhance_b4_ms_per_mpix time per megapixel
"""
import argparse
import importlib
import json
import math
import os
import statistics
import sys

R = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, R)
import numpy as np  # noqa: E402
import torch  # noqa: E402
import oracle  # noqa: E402

M = importlib.import_module("cv-diffusion-model_amd")

p = argparse.ArgumentParser()
p.add_argument("--sizes", type=str, default="400x600,1080x1920", help="comma-separated HxW list")
p.add_argument("--size", type=int, default=256, help="image_size of the module tree (and the tile side)")
p.add_argument("--dtype", default="fp16", choices=["fp32", "fp16", "bf16"])
p.add_argument("--steps", type=int, default=4)
p.add_argument("--iters", type=int, default=5)
p.add_argument("--warmup", type=int, default=3)
args = p.parse_args()
sizes = [tuple(int(v) for v in s.split("x")) for s in args.sizes.split(",")]

assert torch.cuda.is_available(), "gpu_frame_perf.py measures on a GPU; there is nothing to report without one"
dev = torch.device("cuda:0")
S = args.size

spec = oracle.make_spec("small", S)
model = M.LowLightDiffusion(unet_variant="small", image_size=S, num_inference_steps=args.steps, compute_dtype=args.dtype)
model.load_state_dict(oracle.synth_state_dict(oracle.param_shapes(spec)))
model = model.to(dev).eval()


def event_ms(fn):
    a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    a.record()
    fn()
    b.record()
    torch.cuda.synchronize()
    return a.elapsed_time(b)


def alternate(fns):
    """Warm up every function, then time them alternately: -> one list of --iters times per function."""
    for _ in range(args.warmup):  # first use of a shape runs eagerly, the second captures its graph, later ones replay
        for fn in fns:
            fn()
    torch.cuda.synchronize()
    times = [[] for _ in fns]
    for _ in range(args.iters):
        for t, fn in zip(times, fns):
            t.append(event_ms(fn))
    return times


def psnr_u8(a, b):
    d = a.double() / 255.0 - b.double() / 255.0
    mse = (d * d).mean().item()
    return math.inf if mse == 0 else -10.0 * math.log10(mse)


res = {"variant": "small", "size": S, "dtype": args.dtype, "steps": args.steps, "iters": args.iters, "images": []}
for h, w in sizes:
    img = torch.from_numpy((np.random.default_rng(h * 10000 + w).random((h, w, 3)) * 90).astype(np.uint8)).to(dev)
    torch.manual_seed(0)
    t_frame, t_tiled = alternate([lambda: M.enhance_frame_u8(model, img, args.steps), lambda: M.enhance_tiled(model, img, args.steps)])
    g = torch.Generator(device=dev)
    out_frame = M.enhance_frame_u8(model, img, args.steps, generator=g.manual_seed(1))
    out_tiled = M.enhance_tiled(model, img, args.steps, generator=g.manual_seed(1))
    tiles = len(M.tile_origins(h, S, S // 8)) * len(M.tile_origins(w, S, S // 8))
    row = {"image": [h, w], "mpix": round(h * w / 1e6, 4), "frame": [M.frame_pad(h), M.frame_pad(w)], "tiles": tiles,
           "tile_mpix": round(tiles * S * S / 1e6, 4),
           "frame_ms": round(statistics.median(t_frame), 3), "tiled_ms": round(statistics.median(t_tiled), 3),
           "frame_ms_all": [round(t, 3) for t in t_frame], "tiled_ms_all": [round(t, 3) for t in t_tiled],
           "psnr_frame_vs_tiled": round(psnr_u8(out_frame, out_tiled), 2)}
    row["frame_over_tiled"] = round(row["frame_ms"] / row["tiled_ms"], 4)
    row["frame_ms_per_mpix"] = round(row["frame_ms"] / (h * w / 1e6), 3)
    res["images"].append(row)

low = torch.rand(4, 3, S, S, device=dev) * 0.6 - 1.0
t_b4, = alternate([lambda: model.enhance(low, args.steps)])
res["enhance_b4_ms"] = round(statistics.median(t_b4), 3)
res["enhance_b4_ms_all"] = [round(t, 3) for t in t_b4]
res["enhance_b4_ms_per_mpix"] = round(res["enhance_b4_ms"] / (4 * S * S / 1e6), 3)
print(json.dumps(res))
