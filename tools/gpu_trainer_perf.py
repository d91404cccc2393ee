#!/usr/bin/env python3
"""What LowLightTrainer.train_epoch costs over the bare loop it wraps: small@256, bf16 engine, B=8, on the LOL shape (485 pairs of
600 x 400, here seeded synthetic frames; 60 steps per epoch).  One process, one JSON line.  Two models with the same seed, each
with its own FusedAdamW and TrainStep, alternate for `--rounds` rounds over the same epochs of the same frame store:

  trainer   one `trainer.train_epoch()` with log_interval = 0: set_epoch, the seeded draws, the step, the LR schedule's step,
            the loss into a device buffer, one copy at the end
  bare      `loader.set_epoch(e); for batch in loader: step(batch["low_light"], batch["normal_light"])` and nothing else (the step
            draws its own timesteps and noise)

Per epoch: device-event milliseconds around it and host wall time to a final synchronise, both divided by the steps.

  *_ms_per_step                    median over the rounds (device events);  *_wall_ms_per_step  the same on the host clock
  *_all                            every round
  bare_spread_ms_per_step          max - min of the bare loop's rounds: what one loop varies by in this process
  trainer_minus_bare_ms_per_step   the figure to judge, against that spread
"""
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
p.add_argument("--batch", type=int, default=8)
p.add_argument("--dtype", default="bf16", choices=["fp32", "fp16", "bf16"])
p.add_argument("--rounds", type=int, default=5)
args = p.parse_args()

assert torch.cuda.is_available(), "gpu_trainer_perf.py measures on a GPU; there is nothing to report without one"
dev = torch.device("cuda:0")
S, B = args.size, args.batch
rng = np.random.default_rng(0)
normal = [rng.integers(0, 256, size=(args.height, args.width, 3), dtype=np.uint8) for _ in range(args.pairs)]
low = [(f // 6) for f in normal]  # dark twins; the content does not change the work
store = M.DeviceFrameStore(low, normal, device=dev, image_size=S)


def model():
    torch.manual_seed(0)
    return M.LowLightDiffusion(unet_variant="small", image_size=S).to(dev)


with tempfile.TemporaryDirectory() as tmp:
    cfg = M.TrainingConfig(image_size=S, batch_size=B, epochs=args.rounds + 1, use_amp=False, compute_dtype=args.dtype, log_interval=0,
                           progress=False, output_dir=os.path.join(tmp, "out"), checkpoint_dir=os.path.join(tmp, "ckpt"))
    trainer = M.LowLightTrainer(model(), M.DevicePairLoader(store, B, S, "train"), None, cfg)

    bare_model = model().train()
    bare_model.compute_dtype = args.dtype
    bare_opt = M.FusedAdamW(bare_model.parameters(), lr=cfg.learning_rate, weight_decay=cfg.weight_decay, max_grad_norm=cfg.gradient_clip,
                            ema_decay=cfg.ema_decay)
    bare_step = M.TrainStep(bare_model, bare_opt, loss_type=cfg.loss_type, grad_scaler=M.FusedGradScaler() if args.dtype == "fp16" else None)
    bare_loader = M.DevicePairLoader(store, B, S, "train")
    steps = len(bare_loader)

    def trainer_epoch(epoch):
        trainer.epoch = epoch
        trainer.train_epoch()

    def bare_epoch(epoch):
        bare_loader.set_epoch(epoch)
        for batch in bare_loader:
            bare_step(batch["low_light"], batch["normal_light"])

    def timed(fn, epoch):
        a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        torch.cuda.synchronize()
        t0 = time.perf_counter()
        a.record()
        fn(epoch)
        b.record()
        torch.cuda.synchronize()
        return a.elapsed_time(b) / steps, (time.perf_counter() - t0) * 1e3 / steps

    trainer_epoch(0)  # warm-up: the engine contexts, their buffers, the optimiser tables, the loader kernel
    bare_epoch(0)
    t = {"trainer": [], "bare": [], "trainer_wall": [], "bare_wall": []}
    for r in range(args.rounds):
        for name, fn in (("trainer", trainer_epoch), ("bare", bare_epoch)):
            ms, wall = timed(fn, r + 1)
            t[name].append(ms)
            t[name + "_wall"].append(wall)

res = {"variant": "small", "size": S, "dtype": args.dtype, "batch": B, "pairs": args.pairs, "frame": [args.height, args.width],
       "steps_per_epoch": steps, "rounds": args.rounds}
res.update({f"{k}_ms_per_step": round(statistics.median(v), 4) for k, v in t.items()})
res.update({f"{k}_ms_per_step_all": [round(x, 4) for x in v] for k, v in t.items()})
res["bare_spread_ms_per_step"] = round(max(t["bare"]) - min(t["bare"]), 4)
res["trainer_minus_bare_ms_per_step"] = round(res["trainer_ms_per_step"] - res["bare_ms_per_step"], 4)
res["trainer_minus_bare_wall_ms_per_step"] = round(res["trainer_wall_ms_per_step"] - res["bare_wall_ms_per_step"], 4)
res["peak_mem_gib"] = round(torch.cuda.max_memory_allocated() / 2 ** 30, 2)
print(json.dumps(res))
