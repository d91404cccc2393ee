#!/usr/bin/env python3
"""Consistency-distillation step timing: small@256 teacher and student, B=8, bf16 engine (argv: batch, dtype, iters, size,
then optionally H W: the batches are then H x W frames through networks built at `size`, e.g. `8 bf16 20 256 400 600`).
Prints one JSON line with device-event milliseconds per
  distill_step   DistillStep (no autograd: three denoisers, distillation kernels, backward, AdamW, EMA lerp)
  autograd_step  consistency_distillation_loss -> backward -> FusedAdamW.step -> update_ema
  train_step     TrainStep (MSE, the single-denoiser step) on the same student
  forward        one per-sample-t forward of the student (no grad)
the budget DistillStep is held to (train_step + 2 x forward + 0.5 ms), and distill_ns_per_pixel = distill_step / (batch H W),
the figure that compares shapes."""
import importlib
import json
import os
import sys

R = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, R)
import torch  # noqa: E402

M = importlib.import_module("cv-diffusion-model_amd")

batch = int(sys.argv[1]) if len(sys.argv) > 1 else 8
dtype = sys.argv[2] if len(sys.argv) > 2 else "bf16"
iters = int(sys.argv[3]) if len(sys.argv) > 3 else 20
size = int(sys.argv[4]) if len(sys.argv) > 4 else 256
if len(sys.argv) not in range(1, 6) and len(sys.argv) != 7:
    raise SystemExit("usage: gpu_distill_perf.py [batch [dtype [iters [size [H W]]]]]")
height, width = (int(sys.argv[5]), int(sys.argv[6])) if len(sys.argv) == 7 else (size, size)
dev = torch.device("cuda:0")
cd = None if dtype == "fp32" else dtype


def model():
    m = M.LowLightDiffusion(unet_variant="small", image_size=size).to(dev)
    m.compute_dtype = cd
    return m


torch.manual_seed(0)
distill = M.LowLightLCMDistillation(model(), model())
opt = M.FusedAdamW(distill.student.parameters(), lr=1e-5)
step = M.DistillStep(distill, opt)
plain = model().train()
popt = M.FusedAdamW(plain.parameters(), lr=1e-5)
train = M.TrainStep(plain, popt)
low = torch.rand(batch, 3, height, width, device=dev) * 2 - 1
normal = torch.rand(batch, 3, height, width, device=dev) * 2 - 1
t = torch.randint(0, 1000, (batch,), device=dev)


def autograd_step():
    distill.student.zero_grad(set_to_none=True)
    loss = distill.consistency_distillation_loss(low, normal)
    loss.backward()
    opt.step()
    distill.update_ema(0.95)
    return loss


def forward():
    with torch.no_grad():
        return distill.student.unet.forward_split(normal, low, t, frame=True)


def time_ms(fn):
    for _ in range(3):
        fn()
    torch.cuda.synchronize()
    a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    a.record()
    for _ in range(iters):
        fn()
    b.record()
    torch.cuda.synchronize()
    return a.elapsed_time(b) / iters


res = {"batch": batch, "dtype": dtype, "size": size, "height": height, "width": width, "iters": iters}
# alternate the two distillation paths so that drift on a shared host hits both
ds, ag = [], []
for _ in range(2):
    ds.append(time_ms(lambda: step(low, normal)))
    ag.append(time_ms(autograd_step))
res["distill_step_ms"] = round(min(ds), 3)
res["autograd_step_ms"] = round(min(ag), 3)
res["train_step_ms"] = round(time_ms(lambda: train(low, normal)), 3)
res["forward_ms"] = round(time_ms(forward), 3)
res["budget_ms"] = round(res["train_step_ms"] + 2 * res["forward_ms"] + 0.5, 3)
res["within_budget"] = res["distill_step_ms"] <= res["budget_ms"]
res["faster_than_autograd"] = res["distill_step_ms"] < res["autograd_step_ms"]
res["distill_ns_per_pixel"] = round(res["distill_step_ms"] * 1e6 / (batch * height * width), 2)
res["peak_mem_gib"] = round(torch.cuda.max_memory_allocated() / 2 ** 30, 2)
print(json.dumps(res))
