#!/usr/bin/env python3
"""What classifier-free guidance costs: guided against unguided sampling, the one-pass against the two-pass form, the two
kernels alone, condition dropout in a training step, and a guided against an unguided distillation step.

One process, one JSON line.  small@256, fp16, synthetic weights (oracle.synth_state_dict); every figure is the median over
--repeats windows of device-event milliseconds per call, the variants of a group taken alternately.

  enhance      per sampler ("lcm4": the 4-step LCM loop, "ddim50": 50 DDIM steps) and batch (1 / 8 / 32):
                 unguided_ms   `enhance(...)`: the parent's code path (the captured loop) -- the yardstick
                 one_pass_ms   `enhance(..., guidance_scale=2.5)`: one 2B-row denoiser pass per step (host-driven loop)
                 two_pass_ms   the same with two B-row passes per step
               every knob is at its default: the unguided loop is the path a user runs today
  kernels      llie_guide and llie_guidance_pair alone on [B,3,256,256] fp32: microseconds per launch and the GB/s of the bytes
               they must move (guide: 2 reads + 1 write; pair: 2 reads + 4 writes, per element)
  train_step   TrainStep at B = 8 with cond_dropout 0 against 0.1
  distill_step DistillStep at B = 8, unguided against guidance=True
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
p.add_argument("--batches", type=int, nargs="+", default=[1, 8, 32])
p.add_argument("--dtype", default="fp16", choices=["fp32", "fp16", "bf16"])
p.add_argument("--scale", type=float, default=2.5)
p.add_argument("--repeats", type=int, default=5)
p.add_argument("--window_steps", type=int, default=100, help="denoiser steps per timed window (calls = window_steps // steps, at least 2)")
p.add_argument("--train_batch", type=int, default=8)
args = p.parse_args()

assert torch.cuda.is_available(), "gpu_guidance_perf.py measures on a GPU; there is nothing to report without one"
dev = torch.device("cuda:0")
S = args.size


def weights(seed=0):
    return oracle.synth_state_dict(oracle.param_shapes(oracle.make_spec("small", S)), seed=seed)


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


res = {"variant": "small", "size": S, "dtype": args.dtype, "scale": args.scale, "repeats": args.repeats, "enhance": {}}

# ------------------------------------------------------------------ sampling
model = M.LowLightDiffusion(unet_variant="small", image_size=S, num_inference_steps=4, compute_dtype=args.dtype)
model.load_state_dict(weights())
model = model.to(dev).eval()
g = torch.Generator(device=dev).manual_seed(0)
for sampler, n in (("lcm", 4), ("ddim", 50)):
    group = res["enhance"][f"{sampler}{n}"] = {}
    for B in args.batches:
        low = torch.rand(B, 3, S, S, device=dev, generator=g) * 0.6 - 1.0
        noise = torch.randn(n if sampler == "lcm" else 1, B, 3, S, S, device=dev, generator=g)
        fns = {
            "unguided_ms": lambda: model.enhance(low, n, noise=noise, sampler=sampler),
            "one_pass_ms": lambda: model.enhance(low, n, noise=noise, sampler=sampler, guidance_scale=args.scale, _passes=1),
            "two_pass_ms": lambda: model.enhance(low, n, noise=noise, sampler=sampler, guidance_scale=args.scale, _passes=2),
        }
        med, spread = alternate(fns, max(2, args.window_steps // n))
        med["spread_ms"] = spread
        med["one_pass_over_unguided"] = round(med["one_pass_ms"] / med["unguided_ms"], 3)
        med["one_pass_over_two_pass"] = round(med["one_pass_ms"] / med["two_pass_ms"], 3)
        group[str(B)] = med

# ------------------------------------------------------------------ the kernels alone
res["kernels"] = {}
for B in args.batches:
    x, y = torch.randn(B, 3, S, S, device=dev, generator=g), torch.randn(B, 3, S, S, device=dev, generator=g)
    out = torch.empty_like(x)
    x2, y2 = torch.empty(2 * B, 3, S, S, device=dev), torch.empty(2 * B, 3, S, S, device=dev)
    med, _ = alternate({"guide": lambda: M.guide_device(x, y, args.scale, out=out),
                        "guidance_pair": lambda: M.guidance_pair_device(x, y, x2, y2)}, 200, digits=5)
    nbytes = x.numel() * 4
    res["kernels"][str(B)] = {"guide_us": round(med["guide"] * 1e3, 2), "guide_gbs": round(3 * nbytes / (med["guide"] * 1e-3) / 1e9, 1),
                              "guidance_pair_us": round(med["guidance_pair"] * 1e3, 2),
                              "guidance_pair_gbs": round(6 * nbytes / (med["guidance_pair"] * 1e-3) / 1e9, 1)}
del model

# ------------------------------------------------------------------ a training step with condition dropout
B = args.train_batch
low = torch.rand(B, 3, S, S, device=dev, generator=g) * 0.6 - 1.0
normal = torch.rand(B, 3, S, S, device=dev, generator=g) * 2 - 1
steps = {}
for name, pdrop in (("cond_dropout_0_ms", 0.0), ("cond_dropout_0.1_ms", 0.1)):
    torch.manual_seed(0)
    m = M.LowLightDiffusion(unet_variant="small", image_size=S, compute_dtype=args.dtype).to(dev).train()
    opt = M.FusedAdamW(m.parameters(), lr=1e-5, weight_decay=0.01, max_grad_norm=1.0)
    scaler = M.FusedGradScaler() if args.dtype == "fp16" else None
    step = M.TrainStep(m, opt, grad_scaler=scaler, cond_dropout=pdrop)
    steps[name] = lambda step=step: step(low, normal)
med, spread = alternate(steps, 10)
res["train_step"] = {"batch": B, **med, "spread_ms": spread}
del steps

# ------------------------------------------------------------------ a distillation step, guided and not
dsteps = {}
for name, kw in (("unguided_ms", {}), ("guided_ms", {"guidance_scale_range": (args.scale, args.scale), "guidance": True})):
    t = M.LowLightDiffusion(unet_variant="small", image_size=S, num_inference_steps=4)
    t.load_state_dict(weights(1))
    s = M.LowLightDiffusion(unet_variant="small", image_size=S, num_inference_steps=4)
    s.load_state_dict(weights(2))
    d = M.LowLightLCMDistillation(t, s, **kw).to(dev)
    for net in (d.teacher, d.student, d.ema_student):
        net.compute_dtype = args.dtype
    opt = M.FusedAdamW(d.student.parameters(), lr=1e-5, weight_decay=0.01)
    scaler = M.FusedGradScaler() if args.dtype == "fp16" else None
    dstep = M.DistillStep(d, opt, grad_scaler=scaler)
    dsteps[name] = lambda dstep=dstep: dstep(low, normal)
med, spread = alternate(dsteps, 10)
res["distill_step"] = {"batch": B, **med, "spread_ms": spread}
res["peak_mem_gib"] = round(torch.cuda.max_memory_allocated() / 2 ** 30, 2)
print(json.dumps(res))
