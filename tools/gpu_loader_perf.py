#!/usr/bin/env python3
"""What feeding TrainStep from the device-resident loader costs: small@256, bf16 engine, B=8 and B=32, on the LOL shape (485
pairs of 600 x 400, here seeded synthetic frames).  One process, one JSON line.  Per batch size, device-event milliseconds:

  resident_ms       TrainStep fed the same two resident tensors every step (the step as it was before the loader existed)
  loader_ms         the same step fed by DevicePairLoader ("train" mode), epochs chained
  loader_only_ms    the loader alone, per batch
  synth_only_ms     the loader alone in "synthetic" mode (randn + aug_synth_u8), per batch
  *_all             every round; the two step timings alternate in this process (`--rounds` rounds of `--iters` steps each)
  loader_minus_resident_ms   the figure to judge: it should equal loader_only_ms within the spread of resident_ms
  bytes_per_batch   the byte model: reads 2 B S^2 3 (uint8 frames), writes 2 B 3 S^2 4 (fp32 planes)
  loader_only_gbs   bytes_per_batch / loader_only_ms
  store_decode_s    one-off: DeviceFrameStore.from_folder on the 970 PNGs written to a temporary folder (PIL decode + upload)

`--trace N` instead runs N loader-fed steps and nothing else, for a `rocprofv3 --kernel-trace --memory-copy-trace --stats` run
of its own: the kernel table gives the loader kernels' device time, the copy table shows that no batch copies from the host
(one plan upload per epoch)."""
import argparse
import importlib
import json
import os
import statistics
import sys
import tempfile
import time

R = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, R)
import numpy as np  # noqa: E402
import torch  # noqa: E402

M = importlib.import_module("cv-diffusion-model_amd")

p = argparse.ArgumentParser()
p.add_argument("--pairs", type=int, default=485)
p.add_argument("--height", type=int, default=400)
p.add_argument("--width", type=int, default=600)
p.add_argument("--size", type=int, default=256)
p.add_argument("--dtype", default="bf16", choices=["fp32", "fp16", "bf16"])
p.add_argument("--batches", type=int, nargs="+", default=[8, 32])
p.add_argument("--iters", type=int, default=30)
p.add_argument("--rounds", type=int, default=5)
p.add_argument("--trace", type=int, default=0)
p.add_argument("--no-decode", action="store_true", help="skip store_decode_s (the PNG round trip)")
args = p.parse_args()

assert torch.cuda.is_available(), "gpu_loader_perf.py measures on a GPU; there is nothing to report without one"
dev = torch.device("cuda:0")
S = args.size
rng = np.random.default_rng(0)
normal = [rng.integers(0, 256, size=(args.height, args.width, 3), dtype=np.uint8) for _ in range(args.pairs)]
low = [(f // 6) for f in normal]  # dark twins; the content does not change the work
store = M.DeviceFrameStore(low, normal, device=dev, image_size=S)
synth_store = M.DeviceFrameStore(normal, None, device=dev, image_size=S)


def train_step():
    torch.manual_seed(0)
    m = M.LowLightDiffusion(unet_variant="small", image_size=S, compute_dtype=args.dtype).to(dev).train()
    opt = M.FusedAdamW(m.parameters(), lr=1e-4, weight_decay=0.01, max_grad_norm=1.0, ema_decay=0.9999)
    return M.TrainStep(m, opt)


def endless(loader):
    while True:
        yield from loader


def event_ms(fn, reps):
    a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    torch.cuda.synchronize()
    a.record()
    for _ in range(reps):
        fn()
    b.record()
    torch.cuda.synchronize()
    return a.elapsed_time(b) / reps


if args.trace:
    B = args.batches[0]
    step, feed = train_step(), endless(M.DevicePairLoader(store, B, S, "train"))
    sfeed = endless(M.DevicePairLoader(synth_store, B, S, "synthetic"))
    for _ in range(args.trace):
        b = next(feed)
        step(b["low_light"], b["normal_light"])
        next(sfeed)
    torch.cuda.synchronize()
    print(json.dumps({"traced_steps": args.trace, "batch": B, "batches_per_epoch": args.pairs // B}))
    sys.exit(0)

res = {"variant": "small", "size": S, "dtype": args.dtype, "pairs": args.pairs, "frame": [args.height, args.width], "iters": args.iters,
       "rounds": args.rounds, "store_gib": round(store.pool.numel() / 2 ** 30, 3)}
for B in args.batches:
    step = train_step()
    g = torch.Generator().manual_seed(1234)
    rl = (torch.rand(B, 3, S, S, generator=g) * 2 - 1).to(dev)
    rn = (torch.rand(B, 3, S, S, generator=g) * 2 - 1).to(dev)
    feed = endless(M.DevicePairLoader(store, B, S, "train"))
    sfeed = endless(M.DevicePairLoader(synth_store, B, S, "synthetic"))

    def resident():
        step(rl, rn)

    def fed():
        b = next(feed)
        step(b["low_light"], b["normal_light"])

    for _ in range(5):  # warm-up: the engine context, its buffers, the loader kernels
        resident()
        fed()
        next(sfeed)
    t = {"resident": [], "loader": [], "loader_only": [], "synth_only": []}
    for _ in range(args.rounds):
        t["resident"].append(event_ms(resident, args.iters))
        t["loader"].append(event_ms(fed, args.iters))
        t["loader_only"].append(event_ms(lambda: next(feed), args.iters))
        t["synth_only"].append(event_ms(lambda: next(sfeed), args.iters))
    r = {f"{k}_ms": round(statistics.median(v), 4) for k, v in t.items()}
    r.update({f"{k}_ms_all": [round(x, 4) for x in v] for k, v in t.items()})
    r["resident_spread_ms"] = round(max(t["resident"]) - min(t["resident"]), 4)
    r["loader_minus_resident_ms"] = round(r["loader_ms"] - r["resident_ms"], 4)
    r["bytes_per_batch"] = 2 * B * S * S * 3 + 2 * B * 3 * S * S * 4
    r["loader_only_gbs"] = round(r["bytes_per_batch"] / (r["loader_only_ms"] * 1e-3) / 1e9, 1)
    r["pairs_per_s_loader_only"] = round(B / (r["loader_only_ms"] * 1e-3))
    res[f"b{B}"] = r
    del step, feed, sfeed
    torch.cuda.empty_cache()

if not args.no_decode:
    from PIL import Image
    with tempfile.TemporaryDirectory() as tmp:
        for sub, frames in (("low", low), ("high", normal)):
            os.makedirs(os.path.join(tmp, sub))
            for i, f in enumerate(frames):
                Image.fromarray(f).save(os.path.join(tmp, sub, f"{i:04d}.png"), compress_level=1)
        t0 = time.perf_counter()
        decoded = M.DeviceFrameStore.from_folder(tmp, device=dev, image_size=S)
        torch.cuda.synchronize()
        res["store_decode_s"] = round(time.perf_counter() - t0, 2)
        assert torch.equal(decoded.pool, store.pool)
res["peak_mem_gib"] = round(torch.cuda.max_memory_allocated() / 2 ** 30, 2)
print(json.dumps(res))
