#!/usr/bin/env python3
"""Golden vectors of the reference with use_linear_attention=False (StandardAttention, efficient_unet.py:311-357): small built at
image_size=64 with the hash-generated weights -- attention at 16 x 16 (N = 256, C = 128) and 8 x 8 (N = 64, C = 256), plus mid_attn.

  layout         state_dict keys and shapes                                      -> tests/golden/softattn_keys.json
  attn9x8        a stand-alone StandardAttention(128, 4) on a 9 x 8 map, B = 2 (N = 72: no multiple of any tile)
  unet64         EfficientUNet.forward, B = 2, t = (739, 19)
  unet64x72      the same network at 64 x 72, B = 1, t = 499 (fully convolutional: N = 288 and 72)
  loop           the 4-step enhance loop, B = 2, torch.manual_seed(123) draws: enhanced in full, noise_pred / latents of every
                 step sampled [::2, ::2]
  train          one training step (B = 2, explicit timesteps and noise, MSE): loss, the L2 norm of every parameter gradient, and
                 the gradients of every attention parameter of encoder_blocks.2.1 and mid_attn (the larger matrices sampled by
                 rows, stride in grad_rows:<key>)

Inputs are synth_input(...) recipes (make_golden.py).  Runs only where the reference exists; writes tests/golden/softattn_kat.npz.
"""
import json
import os
import sys

import numpy as np
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tools"))
import make_golden as G  # noqa: E402  (loader of the reference package + weight fill)

SITES = ["unet.encoder_blocks.2.1", "unet.mid_attn"]
ROW_STRIDE = {"unet.encoder_blocks.2.1.to_qkv.weight": 2, "unet.mid_attn.to_qkv.weight": 4, "unet.mid_attn.to_out.weight": 2}


def main():
    torch.set_num_threads(8)
    M = G.load_ref_models_package()
    U = sys.modules["src.models.efficient_unet"]
    res = {}

    with torch.no_grad():
        at = U.StandardAttention(128, 4).eval()
        G.fill_(at, "softattn128.")
        res["attn9x8"] = G.np32(at(G.synth_input("softattn128.x", (2, 128, 9, 8), -2, 2)))

    def build():
        unet = U.create_efficient_unet("small", image_size=64, in_channels=6, use_linear_attention=False)
        model = M.LowLightDiffusion(unet=unet, image_size=64, num_inference_steps=4)
        G.fill_(model)  # keys already start with "unet."
        return model

    model = build().eval()
    with open(os.path.join(G.OUT, "softattn_keys.json"), "w") as f:
        json.dump({"small@64": {"num_params": sum(p.numel() for p in model.unet.parameters()),
                                "keys": [[k, list(v.shape)] for k, v in model.unet.state_dict().items()]}}, f)
    with torch.no_grad():
        t = torch.tensor([739, 19], dtype=torch.long)
        res["unet64"] = G.np32(model.unet(G.synth_input("soft64.x", (2, 6, 64, 64), -1.5, 1.5), t))
        res["unet64_t"] = t.numpy()
        t1 = torch.tensor([499], dtype=torch.long)
        res["unet64x72"] = G.np32(model.unet(G.synth_input("soft64x72.x", (1, 6, 64, 72), -1.5, 1.5), t1))
        res["unet64x72_t"] = t1.numpy()
        low = G.synth_input("softe2e64.low", (2, 3, 64, 64), -1.0, -0.4)
        preds = []
        h = model.unet.register_forward_hook(lambda mod, i, o: preds.append(o.clone()))
        torch.manual_seed(123)
        out = model.enhance(low, num_inference_steps=4, return_intermediate=True)
        h.remove()
        res["seed"] = np.array([123])
        res["enhanced"] = G.np32(out.enhanced)
        for i, (p, z) in enumerate(zip(preds, out.intermediate)):
            res[f"noise_pred_{i}"] = np.ascontiguousarray(G.np32(p)[:, :, ::2, ::2])
            res[f"latents_{i}"] = np.ascontiguousarray(G.np32(z)[:, :, ::2, ::2])

    model = build().train()
    low = G.synth_input("softtrain64.low", (2, 3, 64, 64), -1.0, -0.4)
    normal = G.synth_input("softtrain64.normal", (2, 3, 64, 64), -1, 1)
    noise = G.synth_input("softtrain64.noise", (2, 3, 64, 64), -2, 2)
    tt = torch.tensor([500, 37])
    o = model(low, normal, timesteps=tt, noise=noise)
    loss = torch.nn.functional.mse_loss(o["noise_pred"], o["noise"])
    loss.backward()
    res["train_loss"] = np.array(loss.item())
    res["train_timesteps"] = tt.numpy()
    named = dict(model.named_parameters())
    res["train_keys"] = np.array(list(named))
    res["train_grad_norms"] = np.array([p.grad.double().norm().item() for p in named.values()])
    for site in SITES:
        for leaf in ("norm.weight", "norm.bias", "to_qkv.weight", "to_out.weight"):
            k = site + "." + leaf
            g = named[k].grad.numpy().astype(np.float32)
            st = ROW_STRIDE.get(k, 1)
            res["grad:" + k] = np.ascontiguousarray(g[::st])
            res["grad_rows:" + k] = np.array([st])
    path = os.path.join(G.OUT, "softattn_kat.npz")
    np.savez_compressed(path, **res)
    print(path, os.path.getsize(path), "bytes; loss", loss.item(), len(named), "params")


if __name__ == "__main__":
    main()
