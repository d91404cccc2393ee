"""Image metrics without a GPU: the NumPy twin (the definition of PSNR / SSIM in this project) against closed forms and an
independent 2-D filter, the argument checks of the C entry points, and the evaluation CLI's flags."""
import ctypes as C
import importlib
import math
import os
import subprocess
import sys

import numpy as np
import pytest
import torch

from conftest import ROOT

M = importlib.import_module("cv-diffusion-model_amd")
MX = importlib.import_module("cv-diffusion-model_amd.metrics")
native = importlib.import_module("cv-diffusion-model_amd._native")


def window2d():
    k = np.arange(11, dtype=np.float64)
    g = np.exp(-((k - 5.0) ** 2) / (2.0 * 1.5 ** 2))
    g = g / g.sum()
    return np.outer(g, g)


def ssim_formula(mx, my, exx, eyy, exy):
    sx2, sy2, sxy = exx - mx * mx, eyy - my * my, exy - mx * my
    return ((2 * mx * my + 1e-4) * (2 * sxy + 9e-4)) / ((mx * mx + my * my + 1e-4) * (sx2 + sy2 + 9e-4))


# ------------------------------------------------------------------ closed forms
def test_public_names():
    for name in ("ImageMetrics", "image_metrics", "image_metrics_host", "evaluate", "evaluate_full_resolution"):
        assert name in M.__all__ and hasattr(M, name)
    assert hasattr(M.DeviceFrameStore, "frame")


def test_identical_images():
    a = np.random.default_rng(0).random((2, 3, 20, 33)) * 2 - 1
    mse, psnr, ssim = M.image_metrics_host(a, a.copy())
    assert mse.shape == psnr.shape == ssim.shape == (2,) and mse.dtype == np.float64
    assert (mse == 0).all() and np.isposinf(psnr).all()
    assert np.abs(ssim - 1).max() <= 1e-12


def test_constant_images():
    a = np.full((1, 3, 17, 23), 0.9)
    b = np.full((1, 3, 17, 23), 0.88)
    mse, psnr, ssim = M.image_metrics_host(a, b, data_range=(0.0, 1.0))
    assert abs(ssim[0] - (2 * 0.9 * 0.88 + 1e-4) / (0.81 + 0.7744 + 1e-4)) <= 1e-12
    assert abs(mse[0] - 4e-4) <= 1e-12
    assert abs(psnr[0] - (-10 * math.log10(4e-4))) <= 1e-12
    # the same pair in the model's range
    m2 = M.image_metrics_host(a * 2 - 1, b * 2 - 1)
    assert abs(m2.ssim[0] - ssim[0]) <= 1e-12 and abs(m2.mse[0] - 4e-4) <= 1e-12


def test_one_window_image_by_hand():
    rng = np.random.default_rng(1)
    a, b = rng.random((1, 3, 11, 11)), rng.random((1, 3, 11, 11))
    w = window2d()
    vals = []
    for c in range(3):
        x, y = a[0, c], b[0, c]
        vals.append(ssim_formula((w * x).sum(), (w * y).sum(), (w * x * x).sum(), (w * y * y).sum(), (w * x * y).sum()))
    got = M.image_metrics_host(a, b, data_range=(0.0, 1.0))
    assert abs(got.ssim[0] - np.mean(vals)) <= 1e-12
    assert abs(got.mse[0] - ((a - b) ** 2).mean()) <= 1e-15


def test_too_small_raises():
    for shape in [(1, 3, 10, 40), (1, 3, 40, 10)]:
        with pytest.raises(ValueError):
            M.image_metrics_host(np.zeros(shape), np.zeros(shape))
    with pytest.raises(ValueError):
        M.image_metrics_host(np.zeros((10, 11, 3), np.uint8), np.zeros((10, 11, 3), np.uint8))
    with pytest.raises(ValueError):
        M.image_metrics_host(np.zeros((1, 3, 12, 12)), np.zeros((1, 3, 12, 13)))
    with pytest.raises(ValueError):
        M.image_metrics_host(np.zeros((1, 3, 12, 12)), np.zeros((1, 3, 12, 12)), data_range=(1.0, 1.0))


# ------------------------------------------------------------------ an independent filter
def test_filtered_maps_against_scipy():
    signal = pytest.importorskip("scipy.signal")
    rng = np.random.default_rng(2)
    x, y = rng.random((1, 3, 24, 40)), rng.random((1, 3, 24, 40))
    maps = MX.filtered_maps(x, y)
    w = window2d()
    for got, src in zip(maps, (x, y, x * x, y * y, x * y)):
        assert got.shape == (1, 3, 14, 30)
        for c in range(3):
            want = signal.correlate2d(src[0, c], w, mode="valid")
            assert np.abs(got[0, c] - want).max() <= 1e-12


# ------------------------------------------------------------------ uint8
def test_uint8_path():
    z, f = np.zeros((13, 17, 3), np.uint8), np.full((13, 17, 3), 255, np.uint8)
    mse, psnr, _ = M.image_metrics_host(z, f)
    assert mse.shape == (1,) and mse[0] == 1.0 and psnr[0] == 0.0
    rng = np.random.default_rng(3)
    a = rng.integers(0, 256, size=(2, 19, 31, 3), dtype=np.uint8)
    b = rng.integers(0, 256, size=(2, 19, 31, 3), dtype=np.uint8)
    got = M.image_metrics_host(a, b, data_range=(5.0, 7.0))  # ignored for bytes
    fa, fb = (v.transpose(0, 3, 1, 2).astype(np.float64) / 255.0 for v in (a, b))
    want = M.image_metrics_host(fa, fb, data_range=(0.0, 1.0))
    for g, w in zip(got, want):
        assert np.array_equal(g, w)


# ------------------------------------------------------------------ the C entry points refuse bad arguments before any HIP call
def test_c_entry_points_check_arguments():
    L = native.lib()
    buf = (C.c_double * 4096)()
    p = C.cast(buf, C.c_void_p).value
    q = L.llie_image_metrics_scratch_bytes
    need = q(2, 40, 50)
    assert 0 < need <= C.sizeof(buf)
    f32 = lambda a=p, b=p, batch=2, h=40, w=50, lo=-1.0, hi=1.0, out=p, scr=p, nb=need: \
        L.llie_image_metrics_f32(a, b, batch, h, w, lo, hi, out, scr, nb, None)  # noqa: E731
    u8 = lambda a=p, b=p, batch=2, h=40, w=50, out=p, scr=p, nb=need: L.llie_image_metrics_u8(a, b, batch, h, w, out, scr, nb, None)  # noqa: E731
    for fn in (f32, u8):
        assert fn(a=None) == native.ERR_ARG and fn(b=None) == native.ERR_ARG
        assert fn(out=None) == native.ERR_ARG and fn(scr=None) == native.ERR_ARG
        assert fn(batch=0) == native.ERR_ARG and fn(batch=-3) == native.ERR_ARG
        assert fn(h=10) == native.ERR_SHAPE and fn(w=10) == native.ERR_SHAPE and fn(h=0) == native.ERR_SHAPE
        assert fn(nb=need - 1) == native.ERR_WORKSPACE and fn(nb=0) == native.ERR_WORKSPACE
    assert f32(lo=0.5, hi=0.5) == native.ERR_ARG
    assert f32(lo=0.5, hi=0.5, h=5) == native.ERR_ARG  # the argument errors come first
    assert q(0, 40, 50) == native.ERR_ARG and q(1, 10, 50) == native.ERR_SHAPE and q(1, 50, 10) == native.ERR_SHAPE


def test_scratch_bytes_positive_and_monotone():
    q = native.lib().llie_image_metrics_scratch_bytes
    th, tw = MX.TILE_H, MX.TILE_W
    for h, w in [(11, 11), (26, 42), (27, 43), (48, 80), (400, 600), (3000, 4000)]:
        tiles = -(-(h - 10) // th) * -(-(w - 10) // tw)
        assert q(1, h, w) == 16 * tiles  # one {ssim, squared error} pair of doubles per tile: TILE_H / TILE_W are the kernel's
        assert q(3, h, w) == 3 * q(1, h, w)
    prev = 0
    for b in range(1, 6):
        assert q(b, 100, 100) > prev
        prev = q(b, 100, 100)
    for axis in (0, 1):
        prev = 0
        for n in range(11, 300):
            cur = q(1, n, 64) if axis == 0 else q(1, 64, n)
            assert cur >= prev and cur > 0
            prev = cur
        assert prev > q(1, 11, 64)


def test_device_functions_refuse_cpu_tensors():
    a = torch.zeros(1, 3, 16, 16)
    with pytest.raises(RuntimeError, match="no CPU fallback"):
        M.image_metrics(a, a)
    store = M.DeviceFrameStore([np.zeros((16, 16, 3), np.uint8)], [np.zeros((16, 16, 3), np.uint8)], device="cpu")
    assert store.frame(1).shape == (16, 16, 3) and store.frame(0).dtype == torch.uint8
    with pytest.raises(IndexError):
        store.frame(2)
    with pytest.raises(RuntimeError, match="no CPU fallback"):
        M.evaluate(None, M.DevicePairLoader(store, 1, 16, "val"))
    with pytest.raises(RuntimeError, match="no CPU fallback"):
        M.evaluate_full_resolution(None, store)


# ------------------------------------------------------------------ the CLI
def test_cli_help_and_flags():
    script = os.path.join(ROOT, "scripts", "evaluate.py")
    r = subprocess.run([sys.executable, script, "--help"], capture_output=True, text=True, timeout=120)
    assert r.returncode == 0, r.stderr[-1500:]
    sys.path.insert(0, os.path.join(ROOT, "scripts"))
    try:
        ev = importlib.import_module("evaluate")
    finally:
        sys.path.pop(0)
    flags = {s for a in ev.build_parser()._actions for s in a.option_strings} - {"-h", "--help"}
    assert flags == {"--checkpoint", "--variant", "--image_size", "--num_steps", "--dtype", "--device", "--tile_overlap", "--tile_batch",
                     "--data", "--batch_size", "--seed", "--full_resolution", "--per_image", "--output"}
    args = ev.parse_args(["--data", "x"])
    assert args.batch_size == 8 and args.seed == 0 and not args.full_resolution and not args.per_image and args.output is None
