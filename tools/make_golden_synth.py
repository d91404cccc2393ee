#!/usr/bin/env python3
"""Golden bytes of the reference's synthetic low-light degradation (`SyntheticLowLightDataset._create_low_light`,
src/training/dataset.py:286-308).  Runs only where /root/reference exists; writes tests/golden/synth_lowlight_kat.npz.

dataset.py imports `albumentations` and `albumentations.pytorch` at module level; neither is needed by `_create_low_light`, so
they are replaced by empty placeholder modules (names only, no arithmetic).  The data set object is made without `__init__`
(which would build albumentations pipelines) and given the two default ranges.

For case k the reference runs after `np.random.seed(k)`; the same seed is then replayed in the reference's order of draws
(uniform gamma, uniform level, normal(0, level, shape), random(), and uniform(0.8, 1, 3) when that was below 0.5) and a float64
recomputation from the replayed draws must give the reference's bytes exactly, so the stored draws are the ones it used.

  input   uint8 [12,24,24,3]   every byte value occurs in every case
  gamma, level  float64 [12]
  noise   float64 [12,24,24,3] as drawn: normal(0, level)
  shift   bool [12]            the colour shift was drawn;  scale float64 [12,3] ((1, 1, 1) where it was not)
  output  uint8 [12,24,24,3]   the reference's low-light bytes
"""
import importlib.util
import os
import sys
import types

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
REF = "/root/reference"
OUT = os.path.join(ROOT, "tests", "golden")
CASES, SIDE = 12, 24
GAMMA_RANGE, LEVEL_RANGE = (2.0, 5.0), (0.01, 0.05)


def load_ref_dataset_module():
    for name in ("albumentations", "albumentations.pytorch"):
        if name not in sys.modules:
            sys.modules[name] = types.ModuleType(name)  # placeholder: names only
    sys.modules["albumentations"].pytorch = sys.modules["albumentations.pytorch"]
    sys.modules["albumentations"].Compose = type("Compose", (), {})  # placeholders: named in an annotation and an import, no behaviour
    sys.modules["albumentations.pytorch"].ToTensorV2 = type("ToTensorV2", (), {})
    spec = importlib.util.spec_from_file_location("_ref_dataset", os.path.join(REF, "src/training/dataset.py"))
    mod = importlib.util.module_from_spec(spec)
    sys.modules[spec.name] = mod
    spec.loader.exec_module(mod)
    return mod


def case_input(k: int) -> np.ndarray:
    """Every byte value 6.75 times over, shuffled."""
    rng = np.random.default_rng(1000 + k)
    return rng.permutation(np.arange(SIDE * SIDE * 3) % 256).astype(np.uint8).reshape(SIDE, SIDE, 3)


def main():
    D = load_ref_dataset_module()
    ds = D.SyntheticLowLightDataset.__new__(D.SyntheticLowLightDataset)
    ds.gamma_range, ds.noise_level_range = GAMMA_RANGE, LEVEL_RANGE
    out = {k: [] for k in ("input", "gamma", "level", "noise", "shift", "scale", "output")}
    for k in range(CASES):
        img = case_input(k)
        assert len(np.unique(img)) == 256
        np.random.seed(k)
        ref = ds._create_low_light(img)
        # replay of the draws
        np.random.seed(k)
        gamma = np.random.uniform(*GAMMA_RANGE)
        level = np.random.uniform(*LEVEL_RANGE)
        noise = np.random.normal(0, level, img.shape)
        shift = bool(np.random.random() < 0.5)
        scale = np.random.uniform(0.8, 1.0, size=3) if shift else np.ones(3)
        # float64 recomputation from the replayed draws
        n = np.clip(np.power(img.astype(np.float32) / 255.0, gamma).astype(np.float64) + noise, 0, 1)
        if shift:
            n = np.clip(n * scale, 0, 1)
        again = (n * 255).astype(np.uint8)
        assert ref.dtype == np.uint8 and ref.shape == img.shape
        assert np.array_equal(again, ref), f"case {k}: the replayed draws do not reproduce the reference"
        for key, val in (("input", img), ("gamma", gamma), ("level", level), ("noise", noise), ("shift", shift), ("scale", scale),
                         ("output", ref)):
            out[key].append(val)
    arrays = {k: np.stack([np.asarray(x) for x in v]) for k, v in out.items()}
    assert arrays["shift"].any() and not arrays["shift"].all(), "both colour-shift outcomes must be present"
    path = os.path.join(OUT, "synth_lowlight_kat.npz")
    np.savez_compressed(path, **arrays)
    print(f"wrote synth_lowlight_kat.npz: {CASES} cases, {int(arrays['shift'].sum())} with the colour shift, {os.path.getsize(path)} bytes")


if __name__ == "__main__":
    main()
