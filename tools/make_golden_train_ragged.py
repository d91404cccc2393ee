#!/usr/bin/env python3
"""Golden vectors of one training step of the reference at image sizes that are not a multiple of 64
(low_light_diffusion.py:140-171,250-277 + autograd): small built at image_size=72 (levels 72/36/18/9) and 200
(levels 200/100/50/25) with the hash-generated weights, B=2 with distinct timesteps, explicit noise, MSE loss.
Stores the loss, the L2 norm of every parameter gradient and a few gradient tensors in full (input conv, the
bottom-level attention, a bottom-level depthwise weight, a skip weight, an upsampler bias).  Runs only where
the reference checkout exists (make_golden.REF); writes tests/golden/train_small72.npz and tests/golden/train_small200.npz.
"""
import os
import sys

import numpy as np
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tools"))
import make_golden as G  # noqa: E402  (loader of the reference package + weight fill)

# small tensors only (the wide 1x1 weights of the bottom level are covered by the gradient norms)
FULL = ["unet.init_conv.weight", "unet.init_conv.bias", "unet.mid_attn.norm.weight", "unet.mid_attn.norm.bias",
        "unet.mid_attn.to_out.1.weight", "unet.mid_attn.to_out.1.bias", "unet.mid_block1.depthwise.weight",
        "unet.encoder_blocks.3.1.depthwise.weight", "unet.decoder_blocks.3.0.skip.weight", "unet.upsamplers.0.conv.bias",
        "unet.upsamplers.2.conv.bias", "unet.downsamplers.2.down.bias", "unet.final_conv.bias"]
TIMESTEPS = {72: [613, 88], 200: [941, 250]}


def make(size: int) -> None:
    M = G.load_ref_models_package()
    model = M.LowLightDiffusion(unet_variant="small", image_size=size, num_inference_steps=4).train()
    G.fill_(model)
    tag = f"train{size}"
    low = G.synth_input(tag + ".low", (2, 3, size, size), -1.0, -0.4)
    normal = G.synth_input(tag + ".normal", (2, 3, size, size), -1, 1)
    noise = G.synth_input(tag + ".noise", (2, 3, size, size), -2, 2)
    t = torch.tensor(TIMESTEPS[size])
    out = model(low, normal, timesteps=t, noise=noise)
    loss = torch.nn.functional.mse_loss(out["noise_pred"], out["noise"])
    loss.backward()
    res = {"loss": np.array(loss.item()), "timesteps": t.numpy()}
    keys, norms = [], []
    for k, p in model.named_parameters():
        keys.append(k)
        norms.append(p.grad.double().norm().item())
    res["keys"] = np.array(keys)
    res["grad_norms"] = np.array(norms)
    params = dict(model.named_parameters())
    for k in FULL:
        res["grad:" + k] = params[k].grad.numpy().astype(np.float32)
    path = os.path.join(ROOT, "tests", "golden", f"train_small{size}.npz")
    np.savez_compressed(path, **res)
    print(path, os.path.getsize(path), "loss", loss.item(), len(keys), "params")


def main():
    torch.set_num_threads(min(16, os.cpu_count() or 1))
    for size in (72, 200):
        make(size)


if __name__ == "__main__":
    main()
