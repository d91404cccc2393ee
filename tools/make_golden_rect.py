#!/usr/bin/env python3
"""Golden vectors of the reference's EfficientUNet.forward (efficient_unet.py:532-606) at rectangular sizes: the module tree
of small@64 (hash weights, as in make_golden.py), B=1, t=499, run on the CPU at H x W != 64 x 64.  The reference's network is
fully convolutional, so its own forward is the yardstick of frame mode (LowLightDiffusion.enhance_frame).

  64x96, 72x104    outputs in full
  96x64, 104x72    outputs sampled [::2, ::2] (keeps the file under 200 KB)

Inputs are synth_input("rect<H>x<W>.x", (1, 6, H, W), -1.5, 1.5).  Runs only where the reference exists; writes
tests/golden/unet_rect_kat.npz.
"""
import os
import sys

import numpy as np
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tools"))
import make_golden as G  # noqa: E402  (loader of the reference's module + weight fill)

FULL = [(64, 96), (72, 104)]
SAMPLED = [(96, 64), (104, 72)]
T = 499


@torch.no_grad()
def main():
    U = G.load_ref_unet_module()
    m = U.create_efficient_unet("small", image_size=64, in_channels=6).eval()
    G.fill_(m, "unet.")
    t = torch.tensor([T], dtype=torch.long)
    res = {"t": t.numpy()}
    for h, w in FULL + SAMPLED:
        y = G.np32(m(G.synth_input(f"rect{h}x{w}.x", (1, 6, h, w), -1.5, 1.5), t))
        assert y.shape == (1, 3, h, w), y.shape
        res[f"rect{h}x{w}"] = y if (h, w) in FULL else np.ascontiguousarray(y[:, :, ::2, ::2])
        print(f"{h}x{w}: max |y| = {np.abs(y).max():.3f}")
    path = os.path.join(ROOT, "tests", "golden", "unet_rect_kat.npz")
    np.savez_compressed(path, **res)
    print(path, os.path.getsize(path), "bytes")


if __name__ == "__main__":
    main()
