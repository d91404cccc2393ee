#!/usr/bin/env python3
"""What the x0 term costs a training step: `TrainStep` at small@256 with weights 0 (the step without the term) against the same
step with (x0_ssim_weight, x0_l1_weight) = (0.5, 0.5), and the two kernels' calls on their own.

  python tools/gpu_x0loss_perf.py [batch] [dtype]        defaults: 32 fp16

One process, one JSON line.  Synthetic weights (oracle.synth_state_dict), seeded inputs, fixed timesteps and noise, lr = 0 so
both steps see the same weights throughout; fp16 runs with a FusedGradScaler.  Both are steps of one TrainStep object whose two
weights are switched between calls, so they share the engine, its workspace and the gradient buffer.

  step_ms / step_x0_ms   one TrainStep call by device events, the two taken alternately; medians over --iters windows of --reps calls
  added_ms               their difference
  kernels                llie_ssim_grad_f32 (ssim_loss's call, with the gradient) and llie_x0_loss (TrainStep's call) on
                         [batch,3,256,256] fp32, called through the C ABI with every buffer allocated beforehand and enqueued
                         behind a long matrix product (device time, not enqueue time): ms per call, the bytes the call must move
                         (its inputs and outputs once: 3 and 5 tensors), the achieved bytes/s against them, and the scratch
                         bytes it also writes and reads
  overhead_ms            added_ms minus the llie_x0_loss call's own time: what the step pays beyond the kernels
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
p.add_argument("batch", type=int, nargs="?", default=32)
p.add_argument("dtype", nargs="?", default="fp16", choices=["fp32", "fp16", "bf16"])
p.add_argument("--size", type=int, default=256)
p.add_argument("--iters", type=int, default=7)
p.add_argument("--reps", type=int, default=5)
p.add_argument("--warmup", type=int, default=3)
args = p.parse_args()

assert torch.cuda.is_available(), "gpu_x0loss_perf.py measures on a GPU; there is nothing to report without one"
dev = torch.device("cuda:0")
B, S = args.batch, args.size
weights = oracle.synth_state_dict(oracle.param_shapes(oracle.make_spec("small", S)))


model = M.LowLightDiffusion(unet_variant="small", image_size=S, num_inference_steps=4, compute_dtype=args.dtype)
model.load_state_dict(weights)
model = model.to(dev).train()
opt = M.FusedAdamW(model.parameters(), lr=0.0, weight_decay=0.0, max_grad_norm=1.0)
scaler = M.FusedGradScaler(init_scale=1024.0, growth_interval=1 << 30) if args.dtype == "fp16" else None
step = M.TrainStep(model, opt, grad_scaler=scaler)


def run(ws, w1):
    """One step of the one TrainStep object (same engine, workspace and gradient buffer either way) with the given weights."""
    step.x0_ssim_weight, step.x0_l1_weight = ws, w1
    return step(low, normal, timesteps=t, noise=noise)


g = torch.Generator(device=dev).manual_seed(0)
low = torch.rand(B, 3, S, S, generator=g, device=dev) * 0.6 - 1.0
normal = torch.rand(B, 3, S, S, generator=g, device=dev) * 2 - 1
noise = torch.randn(B, 3, S, S, generator=g, device=dev)
t = torch.randint(0, 999, (B,), generator=g, device=dev)


def event_ms(fn, reps):
    a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    a.record()
    for _ in range(reps):
        fn()
    b.record()
    torch.cuda.synchronize()
    return a.elapsed_time(b) / reps


run_a = lambda: run(0.0, 0.0)
run_b = lambda: run(0.5, 0.5)
for _ in range(args.warmup):
    la, lb = run_a(), run_b()
torch.cuda.synchronize()
ta, tb = [], []
for _ in range(args.iters):
    ta.append(event_ms(run_a, args.reps))
    tb.append(event_ms(run_b, args.reps))
res = {"variant": "small", "size": S, "batch": B, "dtype": args.dtype, "iters": args.iters, "reps": args.reps,
       "loss": round(la.item(), 6), "loss_x0": round(lb.item(), 6),
       "step_ms": round(statistics.median(ta), 4), "step_x0_ms": round(statistics.median(tb), 4),
       "step_ms_all": [round(v, 4) for v in ta], "step_x0_ms_all": [round(v, 4) for v in tb]}
res["added_ms"] = round(res["step_x0_ms"] - res["step_ms"], 4)

# the two entry points on their own, on tensors of the step's shapes: every buffer allocated beforehand, and each window of calls
# enqueued behind a long matrix product, so that the events bracket device time and not the host's enqueue rate
L = native.lib()
out = torch.randn(B, 3, S, S, generator=g, device=dev)
x_t = model.scheduler.add_noise(normal, noise, t)
d_out, da = torch.zeros_like(out), torch.empty_like(out)
ssim_out, loss_out = torch.empty(B, device=dev), torch.empty((), device=dev)
acp = model.scheduler._acp_on(dev)
n4 = out.numel() * 4
nbytes = int(L.llie_ssim_grad_scratch_bytes(B, S, S))
scratch = torch.empty((nbytes + 7) // 8, dtype=torch.float64, device=dev)
stream = torch.cuda.current_stream(dev).cuda_stream
blocker = torch.randn(8192, 8192, device=dev)


def call_ssim_grad():
    native.check(L.llie_ssim_grad_f32(out.data_ptr(), normal.data_ptr(), B, S, S, -1.0, 1.0, None, ssim_out.data_ptr(), da.data_ptr(),
                                      scratch.data_ptr(), nbytes, stream), "ssim_grad_f32")


def call_x0_loss():
    native.check(L.llie_x0_loss(out.data_ptr(), x_t.data_ptr(), normal.data_ptr(), t.data_ptr(), acp.data_ptr(), acp.numel(), 0, 0.5, 0.5,
                                loss_out.data_ptr(), d_out.data_ptr(), B, S, S, scratch.data_ptr(), nbytes, stream), "x0_loss")


def device_ms(fn, reps):
    a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    torch.mm(blocker, blocker)
    a.record()
    for _ in range(reps):
        fn()
    b.record()
    torch.cuda.synchronize()
    return a.elapsed_time(b) / reps


res["kernels"] = {}
for name, fn, nb in (("ssim_grad_f32", call_ssim_grad, 3 * n4), ("x0_loss", call_x0_loss, 5 * n4)):
    for _ in range(3):
        fn()
    ms = statistics.median(device_ms(fn, 20) for _ in range(5))
    res["kernels"][name] = {"ms": round(ms, 4), "bytes": nb, "gbs": round(nb / (ms * 1e-3) / 1e9, 1), "scratch_bytes": nbytes}
res["overhead_ms"] = round(res["added_ms"] - res["kernels"]["x0_loss"]["ms"], 4)
res["peak_mem_gib"] = round(torch.cuda.max_memory_allocated() / 2 ** 30, 2)
print(json.dumps(res))
