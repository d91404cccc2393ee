#!/usr/bin/env python3
"""Golden vectors of one training step of the reference on rectangular batches (low_light_diffusion.py:140-171,250-277 +
autograd): small built at image_size=64 with the hash-generated weights, fed 64 x 96 (levels 64x96 / 32x48 / 16x24 / 8x12)
and 72 x 104 (72x104 / 36x52 / 18x26 / 9x13), B=2 with distinct timesteps, explicit noise, MSE loss.  The network is fully
convolutional, so the reference runs these shapes as it stands; image_size only places the attention blocks.
Stores, per shape (keys prefixed "64x96:" / "72x104:"), the loss, the L2 norm of every parameter gradient and the gradient
tensors of make_golden_train_ragged.FULL (those the model built at 64 has) in full.  Runs only where the reference checkout
exists (make_golden.REF); writes tests/golden/train_small_rect.npz.
"""
import os
import sys

import numpy as np
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tools"))
import make_golden as G  # noqa: E402  (loader of the reference package + weight fill)
from make_golden_train_ragged import FULL  # noqa: E402

IMAGE_SIZE = 64
SHAPES = [(64, 96), (72, 104)]
TIMESTEPS = {(64, 96): [702, 35], (72, 104): [466, 919]}


def make(M, h: int, w: int) -> dict:
    model = M.LowLightDiffusion(unet_variant="small", image_size=IMAGE_SIZE, num_inference_steps=4).train()
    G.fill_(model)
    tag = f"train{h}x{w}"
    low = G.synth_input(tag + ".low", (2, 3, h, w), -1.0, -0.4)
    normal = G.synth_input(tag + ".normal", (2, 3, h, w), -1, 1)
    noise = G.synth_input(tag + ".noise", (2, 3, h, w), -2, 2)
    t = torch.tensor(TIMESTEPS[(h, w)])
    out = model(low, normal, timesteps=t, noise=noise)
    loss = torch.nn.functional.mse_loss(out["noise_pred"], out["noise"])
    loss.backward()
    pre = f"{h}x{w}:"
    res = {pre + "loss": np.array(loss.item()), pre + "timesteps": t.numpy()}
    keys, norms = [], []
    for k, p in model.named_parameters():
        keys.append(k)
        norms.append(p.grad.double().norm().item())
    res["keys"] = np.array(keys)
    res[pre + "grad_norms"] = np.array(norms)
    params = dict(model.named_parameters())
    for k in FULL:
        if k in params:  # at image_size = 64 the attention placement leaves encoder_blocks.3 one residual block short of the list
            res[pre + "grad:" + k] = params[k].grad.numpy().astype(np.float32)
    print(pre, "loss", loss.item(), len(keys), "params")
    return res


def main():
    torch.set_num_threads(min(16, os.cpu_count() or 1))
    M = G.load_ref_models_package()
    res = {}
    for h, w in SHAPES:
        res.update(make(M, h, w))
    path = os.path.join(ROOT, "tests", "golden", "train_small_rect.npz")
    np.savez_compressed(path, **res)
    print(path, os.path.getsize(path))


if __name__ == "__main__":
    main()
