#!/usr/bin/env python3
"""What sharing the latents across tiles costs: `enhance_tiled(sync="latents")` against `enhance_tiled(sync="none")`.

One process, one JSON line.  Defaults: small@256, fp16, overlap 32, 32 tiles per call, 4 steps, a seeded random 3000 x 4000 image
of the kind tools/gpu_tiled_perf.py makes (14 x 18 = 252 tiles), synthetic weights (oracle.synth_state_dict).

  sync_ms, none_ms   the two modes end to end on the same image and the same noise canvas (device events), taken alternately
                     after a warm-up that lets sync="none" capture its graphs; medians of --iters
  ratio              sync_ms / none_ms.  sync="latents" runs every step's forwards as plain launches: no graph holds the loop
  sync_step          the sync-step kernel alone over the whole canvas: ms, algorithmic bytes (T * 3 * S^2 * 4 of eps tiles, and
                     36 bytes per canvas pixel: canvas in, noise in, canvas out), GB/s, next to copy_probe_gbs
  psnr_vs_frame      at --frame_size (1080 x 1920, under frame mode's cap): PSNR on the bytes (x = byte / 255) of each mode's
                     result against `enhance_frame_u8` of the same image, the seam-free result the tiles approximate.  The tiled
                     modes share one noise canvas; the frame reads the same canvas where its padded size is the canvas's
                     (shared_noise, true at the default size) and otherwise draws its own with the same seed
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
native = importlib.import_module("cv-diffusion-model_amd._native")

p = argparse.ArgumentParser()
p.add_argument("--height", type=int, default=3000)
p.add_argument("--width", type=int, default=4000)
p.add_argument("--frame_size", type=str, default="1080x1920", help="HxW of the PSNR comparison against frame mode")
p.add_argument("--size", type=int, default=256)
p.add_argument("--dtype", default="fp16", choices=["fp32", "fp16", "bf16"])
p.add_argument("--overlap", type=int, default=32)
p.add_argument("--tile_batch", type=int, default=32)
p.add_argument("--steps", type=int, default=4)
p.add_argument("--iters", type=int, default=5)
p.add_argument("--warmup", type=int, default=3)
args = p.parse_args()

assert torch.cuda.is_available(), "gpu_tiled_sync_perf.py measures on a GPU; there is nothing to report without one"
dev = torch.device("cuda:0")
H, W, S, V, TB = args.height, args.width, args.size, args.overlap, args.tile_batch

spec = oracle.make_spec("small", S)
model = M.LowLightDiffusion(unet_variant="small", image_size=S, num_inference_steps=args.steps, compute_dtype=args.dtype)
model.load_state_dict(oracle.synth_state_dict(oracle.param_shapes(spec)))
model = model.to(dev).eval()


def dark(h, w):
    return torch.from_numpy((np.random.default_rng(h * 10000 + w).random((h, w, 3)) * 90).astype(np.uint8)).to(dev)


def event_ms(fn, reps=1):
    a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    a.record()
    for _ in range(reps):
        fn()
    b.record()
    torch.cuda.synchronize()
    return a.elapsed_time(b) / reps


def psnr_u8(a, b):
    d = a.double() / 255.0 - b.double() / 255.0
    mse = (d * d).mean().item()
    return math.inf if mse == 0 else -10.0 * math.log10(mse)


img = dark(H, W)
hc, wc = max(H, S), max(W, S)
total = len(M.tile_origins(H, S, V)) * len(M.tile_origins(W, S, V))
canvas = torch.randn(args.steps, 3, hc, wc, device=dev, generator=torch.Generator(device=dev).manual_seed(0))
modes = {"sync": lambda: M.enhance_tiled(model, img, args.steps, overlap=V, tile_batch=TB, noise=canvas, sync="latents"),
         "none": lambda: M.enhance_tiled(model, img, args.steps, overlap=V, tile_batch=TB, noise=canvas)}
for _ in range(args.warmup):  # first use of a batch size runs eagerly, the second captures its graph, later ones replay
    for fn in modes.values():
        fn()
torch.cuda.synchronize()
times = {k: [] for k in modes}
for _ in range(args.iters):
    for k, fn in modes.items():
        times[k].append(event_ms(fn))
res = {"variant": "small", "size": S, "dtype": args.dtype, "image": [H, W], "overlap": V, "tile_batch": TB, "tiles": total,
       "steps": args.steps, "iters": args.iters,
       "sync_ms": round(statistics.median(times["sync"]), 3), "none_ms": round(statistics.median(times["none"]), 3),
       "sync_ms_all": [round(t, 3) for t in times["sync"]], "none_ms_all": [round(t, 3) for t in times["none"]]}
res["ratio"] = round(res["sync_ms"] / res["none_ms"], 4)

# ---- the sync-step kernel on its own, over the whole canvas (a step that is not the last: it reads the noise too)
eps = torch.randn(total, 3, S, S, device=dev)
x = canvas[0].clone()
model.scheduler.set_timesteps(args.steps, device=dev)
coef = model.scheduler.step_coefficients(model.scheduler._timestep_list[0])
step = lambda: M.sync_step_device(eps, (H, W), V, x, canvas[1], coef, out=x)  # noqa: E731
step()
ms = event_ms(step, reps=10)
nbytes = total * 3 * S * S * 4 + 36 * hc * wc
res["sync_step"] = {"ms": round(ms, 4), "bytes": nbytes, "gbs": round(nbytes / (ms * 1e-3) / 1e9, 1)}
n = 1 << 30
src = torch.empty(n, dtype=torch.uint8, device=dev).random_(0, 255)
dst = torch.empty_like(src)
L, st = native.lib(), torch.cuda.current_stream(dev).cuda_stream
probe = lambda: native.check(L.llie_copy_probe(src.data_ptr(), dst.data_ptr(), n, st), "copy_probe")  # noqa: E731
probe()
res["copy_probe_gbs"] = round(2.0 * n / (event_ms(probe, reps=10) * 1e-3) / 1e9, 1)
del src, dst, eps, x, img, canvas

# ---- how close each mode comes to the seam-free frame
fh, fw = (int(v) for v in args.frame_size.split("x"))
fimg = dark(fh, fw)
g = torch.Generator(device=dev)
fcanvas = torch.randn(args.steps, 3, max(fh, S), max(fw, S), device=dev, generator=g.manual_seed(1))
shared = (M.frame_pad(fh), M.frame_pad(fw)) == tuple(fcanvas.shape[2:])
frame = M.enhance_frame_u8(model, fimg, args.steps, noise=fcanvas) if shared else M.enhance_frame_u8(model, fimg, args.steps, generator=g.manual_seed(1))
res["psnr_vs_frame"] = {
    "image": [fh, fw], "shared_noise": shared,
    "sync": round(psnr_u8(M.enhance_tiled(model, fimg, args.steps, overlap=V, tile_batch=TB, noise=fcanvas, sync="latents"), frame), 2),
    "none": round(psnr_u8(M.enhance_tiled(model, fimg, args.steps, overlap=V, tile_batch=TB, noise=fcanvas), frame), 2)}
res["peak_mem_gib"] = round(torch.cuda.max_memory_allocated() / 2 ** 30, 2)
print(json.dumps(res))
