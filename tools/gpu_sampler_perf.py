#!/usr/bin/env python3
"""What the samplers of a many-step (teacher) model cost: DDIM against DPM-Solver++ 2M (sampler="dpmpp_2m").

One process, one JSON line.  small@256, B = 8, fp16, synthetic weights (oracle.synth_state_dict); every figure is the median over
--repeats windows of device-event milliseconds per call, the variants taken alternately (the method of gpu_guidance_perf.py), and
images / s = batch / that.

  ddim50            `enhance(sampler="ddim")`, 50 steps: what people run today
  dpmpp_2m_10 / 20  `enhance(sampler="dpmpp_2m")`, 10 and 20 steps
  ddim20            DDIM at 20 steps: the same number of network calls as dpmpp_2m_20; DDIM's step runs in the output head's
                    epilogue, the 2M step is one more elementwise launch per step, so the gap between the two is that launch
  dpmpp_2m_20_guided  20 steps with guidance_scale = --scale (the host-driven loop: a 2B-row pass per step)
  step_kernel       llie_dpm_step alone on [B,3,S,S] fp32, second order, in place: microseconds per launch and the GB/s of the
                    five passes it makes (3 reads, 2 writes)
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
native = importlib.import_module("cv-diffusion-model_amd._native")

p = argparse.ArgumentParser()
p.add_argument("--size", type=int, default=256)
p.add_argument("--batch", type=int, default=8)
p.add_argument("--dtype", default="fp16", choices=["fp32", "fp16", "bf16"])
p.add_argument("--scale", type=float, default=2.5)
p.add_argument("--repeats", type=int, default=5)
p.add_argument("--window_steps", type=int, default=100, help="denoiser steps per timed window (calls = window_steps // steps, at least 2)")
args = p.parse_args()

assert torch.cuda.is_available(), "gpu_sampler_perf.py measures on a GPU; there is nothing to report without one"
dev = torch.device("cuda:0")
S, B = args.size, args.batch


def event_ms(fn, reps):
    a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    a.record()
    for _ in range(reps):
        fn()
    b.record()
    torch.cuda.synchronize()
    return a.elapsed_time(b) / reps


def alternate(fns, reps, digits=3):
    """({name: median ms per call}, {name: max - min}) with the variants taken in turn, --repeats times, after three warm-up
    calls each (the second captures the loop's graph, the third replays it)."""
    for fn in fns.values():
        fn()
        fn()
        fn()
    torch.cuda.synchronize()
    times = {k: [] for k in fns}
    for _ in range(args.repeats):
        for k, fn in fns.items():
            times[k].append(event_ms(fn, reps[k] if isinstance(reps, dict) else reps))
    return ({k: round(statistics.median(v), digits) for k, v in times.items()},
            {k: round(max(v) - min(v), digits) for k, v in times.items()})


model = M.LowLightDiffusion(unet_variant="small", image_size=S, num_inference_steps=4, compute_dtype=args.dtype)
model.load_state_dict(oracle.synth_state_dict(oracle.param_shapes(oracle.make_spec("small", S)), seed=0))
model = model.to(dev).eval()
g = torch.Generator(device=dev).manual_seed(0)
low = torch.rand(B, 3, S, S, device=dev, generator=g) * 0.6 - 1.0
noise = torch.randn(1, B, 3, S, S, device=dev, generator=g)

rows = {"ddim50": ("ddim", 50, {}), "dpmpp_2m_10": ("dpmpp_2m", 10, {}), "dpmpp_2m_20": ("dpmpp_2m", 20, {}), "ddim20": ("ddim", 20, {}),
        "dpmpp_2m_20_guided": ("dpmpp_2m", 20, {"guidance_scale": args.scale})}
fns = {k: (lambda s=s, n=n, kw=kw: model.enhance(low, n, noise=noise, sampler=s, **kw)) for k, (s, n, kw) in rows.items()}
reps = {k: max(2, args.window_steps // n) for k, (_, n, _) in rows.items()}
med, spread = alternate(fns, reps)
res = {"variant": "small", "size": S, "batch": B, "dtype": args.dtype, "scale": args.scale, "repeats": args.repeats, "rows": {}}
for k, (s, n, _) in rows.items():
    res["rows"][k] = {"sampler": s, "steps": n, "ms": med[k], "spread_ms": spread[k], "images_per_s": round(B / (med[k] * 1e-3), 1)}
res["unfused_step_ms_per_step"] = round((med["dpmpp_2m_20"] - med["ddim20"]) / 20, 4)
res["dpmpp_2m_20_over_ddim50_images_per_s"] = round(med["ddim50"] / med["dpmpp_2m_20"], 3)

# ------------------------------------------------------------------ the step kernel alone
x, out, hist = (torch.randn(B, 3, S, S, device=dev, generator=g) for _ in range(3))
coef = model.dpm_schedule(20)[1][5]
stream = torch.cuda.current_stream(dev).cuda_stream
L = native.lib()
kmed, _ = alternate({"step": lambda: native.check(L.llie_dpm_step(out.data_ptr(), x.data_ptr(), hist.data_ptr(), x.data_ptr(), None, x.numel(),
                                                                  coef, stream), "llie_dpm_step")}, 200, digits=5)
res["step_kernel"] = {"us": round(kmed["step"] * 1e3, 2), "gbs": round(5 * x.numel() * 4 / (kmed["step"] * 1e-3) / 1e9, 1)}
res["peak_mem_gib"] = round(torch.cuda.max_memory_allocated() / 2 ** 30, 2)
print(json.dumps(res))
