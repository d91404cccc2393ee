#!/usr/bin/env python3
"""What the input gradients cost the backward pass: one autograd forward + backward of the denoiser without and with d(latents) and
d(cond), and the data-gradient kernel of the input conv on its own.

  python tools/gpu_input_grad_perf.py [dtype] [--no-dx]        default: bf16

One process, one JSON line with one entry per shape: small@256 B = 8, and a 400 x 600 frame B = 4 on the same model (frame=True).
Synthetic weights (oracle.synth_state_dict), seeded inputs, a seeded cotangent; gradients are taken with torch.autograd.grad, so
nothing is accumulated into .grad between calls.

  backward_ms / backward_dx_ms   forward_split + backward by device events, the two taken alternately on one model; medians over
                                 --iters windows of --reps calls.  --no-dx measures backward_ms alone and touches nothing the
                                 input gradients added: the figure of a tree without them, taken with the same tool
  added_ms                       their difference
  kernel                         llie_init_conv_dgrad through the C ABI at the shape, both outputs, every buffer allocated
                                 beforehand, each window enqueued behind a long matrix product (device time, not enqueue time).
                                 The entry zero-fills and repacks the weights before it launches the kernel, so the same call on
                                 one 16 x 16 tile (call_ms_tile) is taken too: ms = call_ms - call_ms_tile is the kernel at the
                                 shape, short by the few microseconds one workgroup runs.  bytes = B H W (C0 sizeof(T) + 4 Cin);
                                 gbs = bytes / ms; byte_time_ratio = ms over the time the bytes take at the copy rate DESIGN.md
                                 records for the box (5.9 TB/s, llie_copy_probe)
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
p.add_argument("dtype", nargs="?", default="bf16", choices=["fp32", "fp16", "bf16"])
p.add_argument("--no-dx", action="store_true")
p.add_argument("--iters", type=int, default=7)
p.add_argument("--reps", type=int, default=5)
p.add_argument("--warmup", type=int, default=3)
args = p.parse_args()

assert torch.cuda.is_available(), "gpu_input_grad_perf.py measures on a GPU; there is nothing to report without one"
dev = torch.device("cuda:0")
S, COPY_RATE = 256, 5.9e12
SHAPES = [(8, 256, 256), (4, 400, 600)]
weights = oracle.synth_state_dict(oracle.param_shapes(oracle.make_spec("small", S)))
model = M.LowLightDiffusion(unet_variant="small", image_size=S, num_inference_steps=4, compute_dtype=args.dtype)
model.load_state_dict(weights)
model = model.to(dev).train()
unet = model.unet
params = list(unet.parameters())
dcode = native.dtype_code(args.dtype)
esize = 4 if args.dtype == "fp32" else 2
C0, CIN = unet.config.base_channels, unet.config.in_channels
L = native.lib()
stream = torch.cuda.current_stream(dev).cuda_stream
blocker = torch.randn(8192, 8192, device=dev)


def event_ms(fn, reps, behind_blocker=False):
    a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    if behind_blocker:
        torch.mm(blocker, blocker)
    a.record()
    for _ in range(reps):
        fn()
    b.record()
    torch.cuda.synchronize()
    return a.elapsed_time(b) / reps


def kernel_call_ms(B, H, W):
    g = torch.randn(B, H, W, C0, device=dev).to({"fp32": torch.float32, "fp16": torch.float16, "bf16": torch.bfloat16}[args.dtype])
    w = unet.init_conv.weight.detach().float().contiguous()
    half = CIN // 2
    d0, d1 = torch.empty(B, half, H, W, device=dev), torch.empty(B, CIN - half, H, W, device=dev)
    nb = int(L.llie_init_conv_pack_bytes(CIN, C0))
    pack = torch.empty(nb // 4, device=dev)

    def call():
        native.check(L.llie_init_conv_dgrad(dcode, g.data_ptr(), C0, w.data_ptr(), d0.data_ptr(), half, d1.data_ptr(), CIN - half, B, H, W,
                                            pack.data_ptr(), nb, stream), "init_conv_dgrad")
    for _ in range(3):
        call()
    return statistics.median(event_ms(call, 20, True) for _ in range(5))


res = {"variant": "small", "image_size": S, "dtype": args.dtype, "iters": args.iters, "reps": args.reps, "dx": not args.no_dx, "shapes": []}
for B, H, W in SHAPES:
    gen = torch.Generator(device=dev).manual_seed(0)
    x_t = torch.randn(B, 3, H, W, generator=gen, device=dev)
    low = torch.rand(B, 3, H, W, generator=gen, device=dev) * 0.6 - 1.0
    cot = (torch.rand(B, 3, H, W, generator=gen, device=dev) * 2 - 1) / 64
    t = torch.randint(0, 999, (B,), generator=gen, device=dev)
    frame = (H, W) != (S, S)

    def run(want):
        a, b = x_t.detach().requires_grad_(want), low.detach().requires_grad_(want)
        y = unet.forward_split(a, b, t, frame=frame)
        return torch.autograd.grad(y, params + ([a, b] if want else []), cot)

    variants = [False] if args.no_dx else [False, True]
    for _ in range(args.warmup):
        for v in variants:
            run(v)
    torch.cuda.synchronize()
    ts = {v: [] for v in variants}
    for _ in range(args.iters):
        for v in variants:
            ts[v].append(event_ms(lambda: run(v), args.reps))
    e = {"batch": B, "H": H, "W": W, "backward_ms": round(statistics.median(ts[False]), 4),
         "backward_ms_all": [round(v, 4) for v in ts[False]]}
    if not args.no_dx:
        e["backward_dx_ms"] = round(statistics.median(ts[True]), 4)
        e["backward_dx_ms_all"] = [round(v, 4) for v in ts[True]]
        e["added_ms"] = round(e["backward_dx_ms"] - e["backward_ms"], 4)
        call_ms, tile_ms = kernel_call_ms(B, H, W), kernel_call_ms(1, 16, 16)
        ms, nbytes = call_ms - tile_ms, B * H * W * (C0 * esize + 4 * CIN)
        e["kernel"] = {"call_ms": round(call_ms, 4), "call_ms_tile": round(tile_ms, 4), "ms": round(ms, 4), "bytes": nbytes,
                       "gbs": round(nbytes / (ms * 1e-3) / 1e9, 1), "byte_time_ratio": round(ms * 1e-3 / (nbytes / COPY_RATE), 2)}
    res["shapes"].append(e)
res["peak_mem_gib"] = round(torch.cuda.max_memory_allocated() / 2 ** 30, 2)
print(json.dumps(res))
