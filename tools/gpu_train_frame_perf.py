"""Frame-size training: per-pixel step rate of TrainStep at 256 x 256 and at 400 x 600, `small`, bf16, B = 8, fed by the
rectangular loader from a 400 x 600 synthetic store.  The two shapes alternate in one process (one TrainStep, one workspace);
the figures are medians over the rounds.  Prints one JSON line.

  python tools/gpu_train_frame_perf.py [rounds=5] [steps per round and shape=8] [batch=8] [dtype=bf16]
  python tools/gpu_train_frame_perf.py --grad-hash      # SHA-256 of the flat gradients of small@256, B = 2, bf16, fixed inputs
"""
import hashlib
import importlib
import json
import os
import statistics
import sys
import time

R = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, R)
import numpy as np  # noqa: E402
import torch  # noqa: E402

M = importlib.import_module("cv-diffusion-model_amd")
SHAPES = [(256, 256), (400, 600)]


def grad_hash(dev) -> dict:
    """The flat gradient buffer of one TrainStep (lr = 0) of small@256, B = 2, bf16, from seeded inputs: a fingerprint of the
    square training path that two commits can compare."""
    torch.manual_seed(0)
    m = M.LowLightDiffusion(unet_variant="small", image_size=256).to(dev).train()
    m.compute_dtype = "bf16"
    g = torch.Generator().manual_seed(1)
    low = (torch.rand(2, 3, 256, 256, generator=g) * 0.6 - 1.0).to(dev)
    normal = (torch.rand(2, 3, 256, 256, generator=g) * 2 - 1).to(dev)
    noise = torch.randn(2, 3, 256, 256, generator=g).to(dev)
    t = torch.tensor([613, 88], device=dev)
    step = M.TrainStep(m, M.FusedAdamW(m.parameters(), lr=0.0, weight_decay=0.0))
    loss = step(low, normal, timesteps=t, noise=noise)
    torch.cuda.synchronize()
    flat = step._flat.cpu().numpy()
    return {"what": "sha256 of the flat fp32 gradients, small@256 B=2 bf16, fixed inputs", "loss": float(loss),
            "numel": int(flat.size), "sha256": hashlib.sha256(flat.tobytes()).hexdigest()}


def main() -> None:
    dev = torch.device("cuda:0")
    if "--grad-hash" in sys.argv:
        print(json.dumps(grad_hash(dev)))
        return
    argv = [a for a in sys.argv[1:] if not a.startswith("--")]
    rounds = int(argv[0]) if len(argv) > 0 else 5
    steps = int(argv[1]) if len(argv) > 1 else 8
    batch = int(argv[2]) if len(argv) > 2 else 8
    dtype = argv[3] if len(argv) > 3 else "bf16"
    rng = np.random.default_rng(0)
    high = [rng.integers(0, 256, size=(400, 600, 3), dtype=np.uint8) for _ in range(2 * batch)]
    store = M.DeviceFrameStore([f // 5 for f in high], high, device=dev)
    torch.manual_seed(0)
    model = M.LowLightDiffusion(unet_variant="small", image_size=256).to(dev).train()
    model.compute_dtype = None if dtype == "fp32" else dtype
    opt = M.FusedAdamW(model.parameters(), lr=1e-4, weight_decay=0.01, max_grad_norm=1.0, ema_decay=0.9999)
    step = M.TrainStep(model, opt)
    loaders = {s: M.DevicePairLoader(store, batch, s[0] if s[0] == s[1] else s, "train", seed=0) for s in SHAPES}

    def run(shape, n):
        done = 0
        loss = None
        while done < n:
            for b in loaders[shape]:
                loss = step(b["low_light"], b["normal_light"])
                done += 1
                if done == n:
                    break
        return loss

    for s in SHAPES:  # warm-up: engine context, workspace at the larger shape, optimiser tables
        run(s, 2)
    torch.cuda.synchronize()
    torch.cuda.reset_peak_memory_stats(dev)
    ms = {s: [] for s in SHAPES}
    loss = None
    for _ in range(rounds):
        for s in SHAPES:
            torch.cuda.synchronize()
            t0 = time.perf_counter()
            loss = run(s, steps)
            torch.cuda.synchronize()
            ms[s].append((time.perf_counter() - t0) / steps * 1e3)
    out = {"what": f"TrainStep small {dtype} B={batch}, loader-fed from a 400x600 store, shapes alternating in one process",
           "rounds": rounds, "steps_per_round": steps, "peak_mem_gib": round(torch.cuda.max_memory_allocated(dev) / 2 ** 30, 2),
           "last_loss": float(loss)}
    for s in SHAPES:
        med = statistics.median(ms[s])
        out[f"{s[0]}x{s[1]}"] = {"ms_per_step": round(med, 2), "img_per_s": round(batch / med * 1e3, 1),
                                 "mpix_per_s": round(batch * s[0] * s[1] / med * 1e-3, 1),
                                 "ms_min": round(min(ms[s]), 2), "ms_max": round(max(ms[s]), 2)}
    a, b = out["256x256"]["mpix_per_s"], out["400x600"]["mpix_per_s"]
    out["per_pixel_rate_400x600_over_256x256"] = round(b / a, 3)
    print(json.dumps(out))


if __name__ == "__main__":
    main()
