#!/usr/bin/env python3
"""Golden vectors of the reference's consistency distillation (LowLightLCMDistillation.consistency_distillation_loss,
low_light_diffusion.py:284-408) run on the CPU: small@64 teacher (hash weights, seed 1), small@64 student (seed 2) and an
ema_student overwritten with seed 3 (three distinct networks: with the EMA equal to the teacher the t_next = 999 case is
0/0 = NaN instead of inf), B=2, 4 inference steps.

Two cases:
  seeded  the reference's own draws (torch.manual_seed(SEED) before the call), recorded as they are made
  inf     idx forced to [37, 0]: t_next = 999 for sample 0, alpha-bar = 0 there, loss = +inf, gradients finite
For each: noise, idx, loss, x_next (the EMA target's input), the L2 norm of every student gradient (381), a few
gradients in full.  Also the module's state_dict key list.  Runs only where the reference exists; writes
tests/golden/distill_small64.npz.
"""
import os
import sys

import numpy as np
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tools"))
import make_golden as G  # noqa: E402  (loader of the reference package + weight fill)

SEED = 5
FULL = ["unet.final_conv.weight", "unet.final_conv.bias", "unet.init_conv.weight", "unet.time_mlp.3.bias",
        "unet.mid_attn.to_out.1.bias", "unet.encoder_blocks.0.0.depthwise.weight", "unet.decoder_blocks.3.0.skip.weight"]


def build(M):
    D = sys.modules["src.models.low_light_diffusion"]
    teacher = M.LowLightDiffusion(unet_variant="small", image_size=64, num_inference_steps=4)
    student = M.LowLightDiffusion(unet_variant="small", image_size=64, num_inference_steps=4)
    G.fill_(teacher, seed=1)
    G.fill_(student, seed=2)
    distill = D.LowLightLCMDistillation(teacher, student)
    G.fill_(distill.ema_student, seed=3)
    return distill


def run(distill, low, normal, noise=None, idx=None):
    """One call of the reference; records (or forces) its two draws and the EMA target's input."""
    rec, orig_randn, orig_randint = {}, torch.randn_like, torch.randint

    def randn_like(x, *a, **k):
        rec["noise"] = noise.clone() if noise is not None else orig_randn(x, *a, **k)
        return rec["noise"]

    def randint(*a, **k):
        rec["idx"] = idx.clone() if idx is not None else orig_randint(*a, **k)
        return rec["idx"]

    hook = distill.ema_student.unet.register_forward_pre_hook(lambda m, args: rec.__setitem__("x_next", args[0][:, :3].clone()))
    torch.randn_like, torch.randint = randn_like, randint
    try:
        distill.student.zero_grad(set_to_none=True)
        loss = distill.consistency_distillation_loss(low, normal, num_inference_steps=4)
        loss.backward()
    finally:
        torch.randn_like, torch.randint = orig_randn, orig_randint
        hook.remove()
    grads = dict(distill.student.named_parameters())
    out = {"noise": rec["noise"].numpy(), "idx": rec["idx"].numpy(), "loss": np.array(loss.item()),
           "x_next": rec["x_next"].numpy(), "grad_norms": np.array([p.grad.double().norm().item() for p in grads.values()])}
    for k in FULL:
        out["grad:" + k] = grads[k].grad.numpy().astype(np.float32)
    return out, [k for k in grads]


def main():
    M = G.load_ref_models_package()
    distill = build(M)
    low = G.synth_input("distill64.low", (2, 3, 64, 64), -1.0, -0.4)
    normal = G.synth_input("distill64.normal", (2, 3, 64, 64), -1, 1)
    res = {"state_keys": np.array(list(distill.state_dict().keys()))}
    torch.manual_seed(SEED)
    seeded, keys = run(distill, low, normal)
    inf, _ = run(distill, low, normal, noise=torch.from_numpy(seeded["noise"]), idx=torch.tensor([37, 0]))
    res["keys"] = np.array(keys)
    for tag, case in (("seeded", seeded), ("inf", inf)):
        for k, v in case.items():
            res[f"{tag}/{k}"] = v
    path = os.path.join(ROOT, "tests", "golden", "distill_small64.npz")
    np.savez_compressed(path, **res)
    print(path, os.path.getsize(path), "seeded idx", seeded["idx"].tolist(), "loss", float(seeded["loss"]),
          "| inf loss", float(inf["loss"]), "grad norm", float(np.sqrt((inf["grad_norms"] ** 2).sum())), len(keys), "params")


if __name__ == "__main__":
    main()
