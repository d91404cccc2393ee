#!/usr/bin/env python3
"""What guidance rescale costs: the guided loops with `guidance_rescale` None against 0.7, and llie_guide_rescale alone against
llie_guide alone.

One process, one JSON line.  small@256, fp16, synthetic weights (oracle.synth_state_dict), w = 2.5; every figure is the median over
--repeats windows of device-event milliseconds per call, the variants of a group taken alternately, with the spread (max - min) of
the windows beside it.

  enhance   per sampler ("lcm4": the 4-step LCM loop, "ddim50": 50 DDIM steps) and batch (1 / 8 / 32):
              guided_ms     `enhance(..., guidance_scale=2.5)`: the parent's code path -- the yardstick
              rescaled_ms   the same with `guidance_rescale=0.7`: llie_guide_rescale (three launches) in llie_guide's place
              added_ms_per_step, added_share
  kernels   llie_guide and llie_guide_rescale (phi = 0.7) alone, back to back from Python, on [B, 3 * 256 * 256] fp32 for the three
            batches and on [1, 3 * 1080 * 1920]: microseconds per call and the GB/s of the bytes counted for each (guide: 2 row
            reads + 1 write; rescale: 4 row reads + 1 write)
"""
import argparse
import importlib
import json
import os
import statistics
import sys

R = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, R)
import torch  # noqa: E402
import oracle  # noqa: E402

M = importlib.import_module("cv-diffusion-model_amd")

p = argparse.ArgumentParser()
p.add_argument("--size", type=int, default=256)
p.add_argument("--batches", type=int, nargs="+", default=[1, 8, 32])
p.add_argument("--dtype", default="fp16", choices=["fp32", "fp16", "bf16"])
p.add_argument("--scale", type=float, default=2.5)
p.add_argument("--rescale", type=float, default=0.7)
p.add_argument("--repeats", type=int, default=5)
p.add_argument("--window_steps", type=int, default=100, help="denoiser steps per timed window (calls = window_steps // steps, at least 2)")
args = p.parse_args()

assert torch.cuda.is_available(), "gpu_guidance_rescale_perf.py measures on a GPU; there is nothing to report without one"
dev = torch.device("cuda:0")
S = args.size


def event_ms(fn, reps):
    a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    a.record()
    for _ in range(reps):
        fn()
    b.record()
    torch.cuda.synchronize()
    return a.elapsed_time(b) / reps


def alternate(fns, reps, digits=3):
    """({name: median ms per call}, {name: max - min}) with the variants taken in turn, --repeats times, after two warm-up
    calls each."""
    for fn in fns.values():
        fn()
        fn()
    torch.cuda.synchronize()
    times = {k: [] for k in fns}
    for _ in range(args.repeats):
        for k, fn in fns.items():
            times[k].append(event_ms(fn, reps))
    return ({k: round(statistics.median(v), digits) for k, v in times.items()},
            {k: round(max(v) - min(v), digits) for k, v in times.items()})


res = {"variant": "small", "size": S, "dtype": args.dtype, "scale": args.scale, "rescale": args.rescale, "repeats": args.repeats,
       "enhance": {}, "kernels": {}}

# ------------------------------------------------------------------ sampling
model = M.LowLightDiffusion(unet_variant="small", image_size=S, num_inference_steps=4, compute_dtype=args.dtype)
model.load_state_dict(oracle.synth_state_dict(oracle.param_shapes(oracle.make_spec("small", S)), seed=0))
model = model.to(dev).eval()
g = torch.Generator(device=dev).manual_seed(0)
for sampler, n in (("lcm", 4), ("ddim", 50)):
    group = res["enhance"][f"{sampler}{n}"] = {}
    for B in args.batches:
        low = torch.rand(B, 3, S, S, device=dev, generator=g) * 0.6 - 1.0
        noise = torch.randn(n if sampler == "lcm" else 1, B, 3, S, S, device=dev, generator=g)
        fns = {
            "guided_ms": lambda: model.enhance(low, n, noise=noise, sampler=sampler, guidance_scale=args.scale),
            "rescaled_ms": lambda: model.enhance(low, n, noise=noise, sampler=sampler, guidance_scale=args.scale, guidance_rescale=args.rescale),
        }
        med, spread = alternate(fns, max(2, args.window_steps // n))
        med["spread_ms"] = spread
        med["added_ms_per_step"] = round((med["rescaled_ms"] - med["guided_ms"]) / n, 4)
        med["added_share"] = round(med["rescaled_ms"] / med["guided_ms"] - 1.0, 4)
        group[str(B)] = med
del model

# ------------------------------------------------------------------ the kernels alone
shapes = [(str(B), B, 3 * S * S) for B in args.batches] + [("1080p", 1, 3 * 1080 * 1920)]
for name, B, per in shapes:
    x, y = torch.randn(B, per, device=dev, generator=g), torch.randn(B, per, device=dev, generator=g)
    out, factor = torch.empty_like(x), torch.empty(B, device=dev)
    med, spread = alternate({"guide": lambda: M.guide_device(x, y, args.scale, out=out),
                             "guide_rescale": lambda: M.guide_rescale_device(x, y, args.scale, args.rescale, out=out, factor=factor)},
                            200, digits=5)
    nbytes = x.numel() * 4
    res["kernels"][name] = {"batch": B, "per_sample": per,
                            "guide_us": round(med["guide"] * 1e3, 2), "guide_gbs": round(3 * nbytes / (med["guide"] * 1e-3) / 1e9, 1),
                            "guide_rescale_us": round(med["guide_rescale"] * 1e3, 2),
                            "guide_rescale_gbs": round(5 * nbytes / (med["guide_rescale"] * 1e-3) / 1e9, 1),
                            "spread_us": {k: round(v * 1e3, 2) for k, v in spread.items()}}
res["peak_mem_gib"] = round(torch.cuda.max_memory_allocated() / 2 ** 30, 2)
print(json.dumps(res))
