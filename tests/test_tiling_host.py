"""Tiled full-resolution enhancement, the parts that need no GPU: the tile plan, the NumPy twins of the gather / blend kernels
against a float64 restatement of the definition written here, argument checks and the CLI flags."""
import ctypes as C
import importlib
import os
import sys

import numpy as np
import pytest
import torch

from conftest import ROOT

M = importlib.import_module("cv-diffusion-model_amd")
T = importlib.import_module("cv-diffusion-model_amd.tiling")
native = importlib.import_module("cv-diffusion-model_amd._native")

SHAPES = [(300, 500, 64, 16), (64, 64, 64, 16), (65, 129, 64, 32), (50, 200, 64, 8), (481, 321, 128, 32), (97, 353, 64, 0),
          (1000, 777, 256, 32), (113, 64, 64, 31)]


# ------------------------------------------------------------------ restatement of the definition (float64, per output row)
def plan_ref(length, s, v):
    """Origins of one axis, from the definition, on Python ints."""
    if length <= s:
        return [0]
    n = 2
    while (n - 1) * (s - v) < length - s:  # the least n with (n - 1)(S - v) >= L - S, i.e. ceil((L - S) / (S - v)) + 1
        n += 1
    return [(i * (length - s)) // (n - 1) for i in range(n)]


def window_ref(s, v):
    return [1.0 if v == 0 else min(k + 1, s - k, v) / v for k in range(s)]


def blend_ref(tiles, h, w, v):
    """float64 [H,W,3] before denormalisation: for every output row, the covering tiles in ascending number, whole rows at once."""
    s = tiles.shape[2]
    oys, oxs = plan_ref(h, s, v), plan_ref(w, s, v)
    win = np.array(window_ref(s, v), dtype=np.float64)
    t64 = tiles.astype(np.float64)
    out = np.empty((h, w, 3), dtype=np.float64)
    for y in range(h):
        num = np.zeros((w, 3))
        den = np.zeros(w)
        for iy, oy in enumerate(oys):
            if not oy <= y < oy + s:
                continue
            for ix, ox in enumerate(oxs):
                x1 = min(ox + s, w)
                g = win[y - oy] * win[:x1 - ox]
                num[ox:x1] += t64[iy * len(oxs) + ix, :, y - oy, :x1 - ox].T * g[:, None]
                den[ox:x1] += g
        out[y] = num / den[:, None]
    return out


# ------------------------------------------------------------------ 1. the plan
@pytest.mark.parametrize("s", [16, 64])
def test_plan_sweep_and_library(s):
    """Every position covered, first origin 0, last tile ends at L, neighbouring origins 1 .. S - v apart, at most 3 tiles over a
    position (the bound on the covering tiles per axis); and the built library's host functions give the same plan."""
    lib = native.lib()
    buf = (C.c_int * 64)()
    for v in range(0, s // 2 + 1):
        for length in range(1, 6 * s + 2):
            o = T.tile_origins(length, s, v)
            assert o == plan_ref(length, s, v), (length, s, v)
            assert o[0] == 0
            if length <= s:
                assert o == [0]
            else:
                assert o[-1] + s == length
                d = np.diff(o)
                assert d.min() >= 1 and d.max() <= s - v, (length, s, v, o)
            cover = np.zeros(max(length, s), dtype=np.int64)
            for oi in o:
                cover[oi:oi + s] += 1
            assert cover[:length].min() >= 1 and cover.max() <= 3, (length, s, v, o)
            assert lib.llie_tile_count(length, s, v) == len(o)
            assert lib.llie_tile_origins(length, s, v, buf) == 0
            assert list(buf[:len(o)]) == o, (length, s, v)


def test_plan_arguments():
    lib = native.lib()
    buf = (C.c_int * 8)()
    for length, s, v in [(100, 64, -1), (100, 64, 33), (0, 64, 8), (100, 0, 0), (-5, 64, 8)]:
        assert lib.llie_tile_count(length, s, v) == native.ERR_ARG
        assert lib.llie_tile_origins(length, s, v, buf) == native.ERR_ARG
        with pytest.raises(ValueError):
            T.tile_origins(length, s, v)
    assert lib.llie_tile_origins(100, 64, 8, None) == native.ERR_ARG
    assert T.tile_origins(100, 64, 32) == [0, 18, 36] and T.tile_origins(64, 64, 32) == [0] and T.tile_origins(10, 64, 0) == [0]
    # a null pointer or a bad plan is refused before anything touches a device
    assert lib.llie_tile_gather_u8(None, 10, 10, 8, 2, 0, 1, None, None) == native.ERR_ARG
    assert lib.llie_tile_blend_u8(None, 10, 10, 8, 2, None, None) == native.ERR_ARG


# ------------------------------------------------------------------ 2. host blend against float64
@pytest.mark.parametrize("h,w,s,v", [(300, 500, 64, 16), (64, 64, 64, 16), (65, 129, 64, 32), (50, 200, 64, 8), (97, 353, 64, 0),
                                     (113, 64, 64, 31)])
def test_host_blend_vs_float64(h, w, s, v):
    """Before quantisation at most 2e-6 absolute (<= 9 products, 18 additions and a division of fp32 rounding on values up to
    1.2); after it a byte differs by at most one LSB and only where the unclipped float64 value lies within 3e-4 of an integer,
    in fewer than 0.1 % of the bytes."""
    rng = np.random.default_rng(h * 1000 + w)
    n = len(T.tile_origins(h, s, v)) * len(T.tile_origins(w, s, v))
    tiles = (rng.random((n, 3, s, s), dtype=np.float32) * np.float32(2.4) - np.float32(1.2))
    ref = blend_ref(tiles, h, w, v)
    got = T.blend_accumulate_array(tiles, (h, w), v)
    assert got.dtype == np.float32 and got.shape == (h, w, 3)
    err = np.abs(got.astype(np.float64) - ref).max()
    print(f"blend ({h},{w},{s},{v}): max abs error before quantisation {err:.3e}")
    assert err <= 2e-6
    unclipped = (ref + 1.0) * 127.5
    want = np.clip(unclipped, 0, 255).astype(np.uint8)
    assert want.min() == 0 and want.max() == 255  # the clip acts on both sides
    out = T.blend_tiles_array(tiles, (h, w), v)
    assert out.dtype == np.uint8 and out.shape == (h, w, 3)
    diff = np.abs(out.astype(np.int64) - want.astype(np.int64))
    print(f"blend ({h},{w},{s},{v}): {int((diff > 0).sum())} of {diff.size} bytes differ")
    assert diff.max() <= 1
    assert np.all(np.abs(unclipped[diff > 0] - np.rint(unclipped[diff > 0])) <= 3e-4)
    assert (diff > 0).mean() < 1e-3


def test_host_gather_definition():
    """gather_tiles_array element by element against the definition, on an image smaller than a tile along one axis and larger
    along the other (edge replication acts), and on one larger along both."""
    rng = np.random.default_rng(3)
    for h, w, s, v in [(20, 45, 32, 8), (70, 33, 32, 16)]:
        img = rng.integers(0, 256, size=(h, w, 3), dtype=np.uint8)
        tiles = T.gather_tiles_array(img, s, v)
        oys, oxs = plan_ref(h, s, v), plan_ref(w, s, v)
        assert tiles.shape == (len(oys) * len(oxs), 3, s, s) and tiles.dtype == np.float32
        for iy, oy in enumerate(oys):
            for ix, ox in enumerate(oxs):
                for y in range(s):
                    for x in range(s):
                        px = img[min(oy + y, h - 1), min(ox + x, w - 1)]
                        want = (px.astype(np.float32) / np.float32(127.5) - np.float32(1.0))
                        assert np.array_equal(tiles[iy * len(oxs) + ix, :, y, x], want)


# ------------------------------------------------------------------ 3. round trip
@pytest.mark.parametrize("h,w,s,v", SHAPES)
def test_round_trip_within_one_lsb(h, w, s, v):
    """blend(gather(img)) is within one LSB of img and never above it: the truncating denormalisation, as
    test_preprocess_postprocess_semantics states for the untiled pair."""
    rng = np.random.default_rng(h + w + s + v)
    img = rng.integers(0, 256, size=(h, w, 3), dtype=np.uint8)
    back = T.blend_tiles_array(T.gather_tiles_array(img, s, v), (h, w), v).astype(np.int64)
    assert back.shape == img.shape
    assert np.all(back <= img) and np.all(img - back <= 1)


# ------------------------------------------------------------------ 4. refusals and the CLI
def test_refusals_without_a_device():
    model = M.LowLightDiffusion(unet_variant="small", image_size=64)
    img = torch.zeros(100, 120, 3, dtype=torch.uint8)
    with pytest.raises(RuntimeError, match="HIP device"):
        M.enhance_tiled(model, img)
    with pytest.raises(RuntimeError, match="HIP device"):
        M.gather_tiles_device(img, 64, 8)
    with pytest.raises(RuntimeError, match="HIP device"):
        M.gather_noise_device(torch.zeros(4, 3, 100, 120), (100, 120), 64, 8)
    with pytest.raises(RuntimeError, match="HIP device"):
        M.blend_tiles_device(torch.zeros(4, 3, 64, 64), (100, 120), 8)
    for bad in (-1, 33, 64):
        with pytest.raises(ValueError, match="overlap"):
            M.enhance_tiled(model, img, overlap=bad)
        with pytest.raises(ValueError, match="overlap"):
            M.gather_tiles_array(img.numpy(), 64, bad)
        with pytest.raises(ValueError, match="overlap"):
            M.blend_tiles_array(np.zeros((4, 3, 64, 64), np.float32), (100, 120), bad)
    with pytest.raises(ValueError):
        M.enhance_tiled(model, img.float())           # dtype
    with pytest.raises(ValueError):
        M.enhance_tiled(model, img[None])             # rank
    with pytest.raises(ValueError):
        M.enhance_tiled(model, img[:, :, :2])         # not RGB
    with pytest.raises(ValueError):
        M.blend_tiles_array(np.zeros((5, 3, 64, 64), np.float32), (100, 120), 8)  # the plan has 4 tiles


def test_cli_parses_tile_flags():
    sys.path.insert(0, os.path.join(ROOT, "scripts"))
    try:
        inference = importlib.import_module("inference")
    finally:
        sys.path.pop(0)
    a = inference.parse_args(["--input", "a.png", "--output", "b.png", "--tile", "--tile_overlap", "16", "--tile_batch", "8"])
    assert a.tile is True and a.tile_overlap == 16 and a.tile_batch == 8
    d = inference.parse_args(["--input", "a.png", "--output", "b.png"])
    assert d.tile is False and d.tile_overlap is None and d.tile_batch == 32
