"""The x0 term without a GPU: `ssim_grad_host` against float64 autograd of the SSIM definition and against central differences,
`x0_loss_host` against float64 autograd for both prediction types and on the zero-SNR table, the argument checks of the new C
entry points, the export lists, and the training script's two flags, which reach the trainer's keywords and leave TrainingConfig as it was."""
import ctypes as C
import dataclasses
import importlib
import inspect
import os
import re
import sys

import numpy as np
import pytest
import torch
import torch.nn.functional as F

from conftest import ROOT

M = importlib.import_module("cv-diffusion-model_amd")
MX = importlib.import_module("cv-diffusion-model_amd.metrics")
P = importlib.import_module("cv-diffusion-model_amd.pipeline")
native = importlib.import_module("cv-diffusion-model_amd._native")

SHAPES = [(1, 11, 11), (2, 12, 27), (2, 37, 45), (1, 64, 64)]


def images(shape, seed):
    """A seeded uniform image in (-1, 1) and a Gaussian perturbation of it."""
    b, h, w = shape
    rng = np.random.default_rng(seed)
    y = rng.uniform(-1.0, 1.0, (b, 3, h, w))
    a = y + 0.2 * rng.standard_normal((b, 3, h, w))
    return a, y


def ssim_torch(a: torch.Tensor, b: torch.Tensor, lo=-1.0, hi=1.0) -> torch.Tensor:
    """image_metrics_host's SSIM in torch float64, written from the definition: the 2-D window g (x) g as one depthwise
    convolution over the valid positions -> [B]."""
    g = torch.from_numpy(MX.ssim_window())
    win = torch.outer(g, g)[None, None].repeat(3, 1, 1, 1)
    x, y = (a - lo) / (hi - lo), (b - lo) / (hi - lo)
    f = lambda m: F.conv2d(m, win, groups=3)
    mx, my, xx, yy, xy = f(x), f(y), f(x * x), f(y * y), f(x * y)
    sx, sy, sxy = xx - mx * mx, yy - my * my, xy - mx * my
    smap = ((2 * mx * my + 1e-4) * (2 * sxy + 9e-4)) / ((mx * mx + my * my + 1e-4) * (sx + sy + 9e-4))
    return smap.mean(dim=(1, 2, 3))


def x0_term_torch(out, x_t, normal, acp, velocity, ws, w1):
    """The term of the issue in torch float64, from its definition (samples with acp == 0 left out)."""
    batch = out.shape[0]
    total = torch.zeros((), dtype=torch.float64)
    for b in range(batch):
        if acp[b] == 0:
            continue
        alpha, sigma = np.sqrt(acp[b]), np.sqrt(1.0 - acp[b])
        p, q = (alpha, -sigma) if velocity else (1.0 / alpha, -sigma / alpha)
        xh = p * x_t[b:b + 1] + q * out[b:b + 1]
        total = total + acp[b] * (ws * (1.0 - ssim_torch(xh, normal[b:b + 1])[0]) + w1 * (xh - normal[b:b + 1]).abs().mean())
    return total / batch


# ------------------------------------------------------------------ ssim_grad_host
@pytest.mark.parametrize("shape", SHAPES)
def test_twin_against_float64_autograd(shape):
    a, y = images(shape, 11)
    ssim, grad = M.ssim_grad_host(a, y, (-1.0, 1.0))
    assert ssim.dtype == np.float64 and grad.dtype == np.float64 and ssim.shape == (shape[0],) and grad.shape == a.shape
    ta = torch.from_numpy(a).requires_grad_(True)
    ref = ssim_torch(ta, torch.from_numpy(y))
    ref.sum().backward()
    want = ta.grad.numpy()
    assert np.abs(grad - want).max() <= 1e-12 * np.abs(want).max()
    # the value is image_metrics_host's
    np.testing.assert_allclose(ssim, M.image_metrics_host(a, y, (-1.0, 1.0)).ssim, rtol=0, atol=1e-14)
    np.testing.assert_allclose(ssim, ref.detach().numpy(), rtol=0, atol=1e-13)


def test_twin_other_data_range():
    a, y = images((1, 13, 17), 5)
    a, y = (a + 1.0) * 100.0, (y + 1.0) * 100.0  # (0, 200)
    ssim, grad = M.ssim_grad_host(a, y, (0.0, 200.0))
    ta = torch.from_numpy(a).requires_grad_(True)
    ssim_torch(ta, torch.from_numpy(y), 0.0, 200.0).sum().backward()
    assert np.abs(grad - ta.grad.numpy()).max() <= 1e-12 * np.abs(ta.grad.numpy()).max()


@pytest.mark.parametrize("shape", SHAPES)
def test_twin_against_central_differences(shape):
    a, y = images(shape, 23)
    _, grad = M.ssim_grad_host(a, y, (-1.0, 1.0))
    rng = np.random.default_rng(99)
    h = 1e-6
    scale = np.abs(grad).max()
    for _ in range(20):
        idx = tuple(int(rng.integers(0, n)) for n in a.shape)
        ap, am = a.copy(), a.copy()
        ap[idx] += h
        am[idx] -= h
        fd = (M.image_metrics_host(ap, y).ssim[idx[0]] - M.image_metrics_host(am, y).ssim[idx[0]]) / (2 * h)
        assert abs(fd - grad[idx]) <= 1e-6 * scale, (idx, fd, grad[idx])


def test_twin_argument_checks():
    a, y = images((1, 11, 11), 1)
    with pytest.raises(ValueError):
        M.ssim_grad_host(a[:, :, :10], y[:, :, :10])
    with pytest.raises(ValueError):
        M.ssim_grad_host((a * 0).astype(np.uint8), (y * 0).astype(np.uint8))
    with pytest.raises(ValueError):
        M.ssim_grad_host(a, y, (1.0, 1.0))


def test_float32_evaluation_stays_close():
    """What the device tests size their tolerance with: the same formulas in float32 stay near the float64 twin."""
    a, y = images((1, 37, 45), 3)
    x, yy = (a + 1.0) / 2.0, (y + 1.0) / 2.0
    s64, g64 = MX.ssim_grad_mapped(x, yy)
    s32, g32 = MX.ssim_grad_mapped(x.astype(np.float32), yy.astype(np.float32))
    assert g32.dtype == np.float32 and s32.dtype == np.float32
    assert np.abs(g32 - g64).max() <= 1e-5 * np.abs(g64).max()
    assert abs(float(s32[0]) - float(s64[0])) <= 1e-5


# ------------------------------------------------------------------ x0_loss_host
def zero_snr_acp():
    s = M.LCMScheduler(num_train_timesteps=1000, beta_schedule="scaled_linear", prediction_type="epsilon", num_inference_steps=4,
                       rescale_betas_zero_snr=True)
    return s.alphas_cumprod.double().numpy()


def x0_inputs(shape, seed):
    b, h, w = shape
    rng = np.random.default_rng(seed)
    normal = rng.uniform(-1.0, 1.0, (b, 3, h, w))
    x_t = normal * 0.7 + 0.5 * rng.standard_normal((b, 3, h, w))
    out = rng.standard_normal((b, 3, h, w))
    return out, x_t, normal


@pytest.mark.parametrize("velocity", [False, True])
@pytest.mark.parametrize("weights", [(1.0, 0.0), (0.0, 1.0), (0.5, 0.25)])
def test_x0_host_against_float64_autograd(velocity, weights):
    out, x_t, normal = x0_inputs((3, 21, 29), 7)
    acp = np.array([0.9991, 0.31, 0.004])
    term, grad = M.x0_loss_host(out, x_t, normal, acp, velocity, *weights)
    to = torch.from_numpy(out).requires_grad_(True)
    ref = x0_term_torch(to, torch.from_numpy(x_t), torch.from_numpy(normal), acp, velocity, *weights)
    ref.backward()
    want = to.grad.numpy()
    assert abs(term - ref.item()) <= 1e-12 * max(1.0, abs(ref.item()))
    assert np.abs(grad - want).max() <= 1e-12 * np.abs(want).max()


@pytest.mark.parametrize("velocity", [False, True])
def test_x0_host_zero_snr_row(velocity):
    table = zero_snr_acp()
    assert table[999] == 0.0
    acp = table[[0, 499, 999]]
    out, x_t, normal = x0_inputs((3, 16, 19), 13)
    term, grad = M.x0_loss_host(out, x_t, normal, acp, velocity, 0.5, 0.5)
    assert np.isfinite(term) and np.isfinite(grad).all()
    assert not grad[2].any() and grad[0].any() and grad[1].any()
    # the row carries no term either: the loss is that of the two others over B = 3
    t2, _ = M.x0_loss_host(out[:2], x_t[:2], normal[:2], acp[:2], velocity, 0.5, 0.5)
    assert abs(term - t2 * 2.0 / 3.0) <= 1e-14


def test_x0_host_zero_weights_and_checks():
    out, x_t, normal = x0_inputs((2, 11, 12), 2)
    term, grad = M.x0_loss_host(out, x_t, normal, [0.5, 0.25], False, 0.0, 0.0)
    assert term == 0.0 and grad.shape == out.shape and not grad.any()
    with pytest.raises(ValueError):
        M.x0_loss_host(out, x_t, normal, [0.5, 0.25], False, -0.1, 0.0)
    with pytest.raises(ValueError):
        M.x0_loss_host(out, x_t, normal, [0.5], False, 1.0, 0.0)
    with pytest.raises(ValueError):
        M.x0_loss_host(out[:, :, :10], x_t[:, :, :10], normal[:, :, :10], [0.5, 0.25], False, 1.0, 0.0)


def test_epsilon_gradient_factor_is_bounded():
    """w q = -alpha sigma under epsilon prediction: the gradient does not blow up towards the noisy end of the table."""
    out, x_t, normal = x0_inputs((1, 12, 12), 4)
    g_small = M.x0_loss_host(out, x_t, normal, [1e-8], False, 0.0, 1.0)[1]
    assert np.abs(g_small).max() <= 1e-4 / (3 * 12 * 12) * 1.0001


# ------------------------------------------------------------------ the C entry points (checked before any HIP call)
def test_entry_points_refuse_before_any_hip_call():
    L = native.lib()
    assert L.llie_ssim_grad_scratch_bytes(1, 10, 64) == native.ERR_SHAPE
    assert L.llie_ssim_grad_scratch_bytes(0, 64, 64) == native.ERR_ARG
    vh, vw = 27, 35
    tiles = ((vh + MX.TILE_H - 1) // MX.TILE_H) * ((vw + MX.TILE_W - 1) // MX.TILE_W)
    assert L.llie_ssim_grad_scratch_bytes(2, 37, 45) == 8 * (2 * 3 * tiles * 2 + 2 * 2) + 4 * (3 * 2 * 3 * vh * vw)
    buf = (C.c_float * 16)()
    p = C.addressof(buf)
    big = 1 << 30
    assert L.llie_ssim_grad_f32(None, p, 1, 11, 11, -1.0, 1.0, None, p, None, p, big, None) == native.ERR_ARG
    assert L.llie_ssim_grad_f32(p, p, 1, 11, 11, -1.0, 1.0, None, None, None, p, big, None) == native.ERR_ARG
    assert L.llie_ssim_grad_f32(p, p, 1, 11, 11, 1.0, 1.0, None, p, None, p, big, None) == native.ERR_ARG
    assert L.llie_ssim_grad_f32(p, p, 1, 10, 11, -1.0, 1.0, None, p, None, p, big, None) == native.ERR_SHAPE
    assert L.llie_ssim_grad_f32(p, p, 1, 11, 11, -1.0, 1.0, None, p, None, p, 8, None) == native.ERR_WORKSPACE
    x0 = lambda **k: L.llie_x0_loss(k.get("out", p), p, p, k.get("t", p), p, k.get("n", 1000), 0, k.get("ws", 0.5), k.get("w1", 0.5),
                                    k.get("loss", p), None, 1, k.get("h", 11), 11, p, k.get("bytes", big), None)
    assert x0(out=None) == native.ERR_ARG
    assert x0(t=None) == native.ERR_ARG
    assert x0(loss=None) == native.ERR_ARG
    assert x0(n=0) == native.ERR_ARG
    assert x0(ws=-1.0) == native.ERR_ARG
    assert x0(w1=float("nan")) == native.ERR_ARG
    assert x0(h=10) == native.ERR_SHAPE
    assert x0(bytes=8) == native.ERR_WORKSPACE


def test_device_functions_refuse_the_cpu():
    a = torch.zeros(1, 3, 16, 16)
    with pytest.raises(RuntimeError, match="HIP device"):
        M.ssim_loss(a, a)
    s = M.LCMScheduler(num_train_timesteps=1000, beta_schedule="scaled_linear", prediction_type="epsilon", num_inference_steps=4,
                       rescale_betas_zero_snr=True)
    with pytest.raises(RuntimeError, match="HIP device"):
        M.x0_loss(s, a, a, a, torch.zeros(1, dtype=torch.long), ssim_weight=1.0, l1_weight=0.0)
    with pytest.raises(ValueError):
        M.ssim_loss(a, a.clone().requires_grad_(True))


# ------------------------------------------------------------------ names, flags, config
def test_export_lists():
    for name in ("ssim_loss", "ssim_grad_host", "x0_loss", "x0_loss_host"):
        assert name in M.__all__ and hasattr(M, name)
    header = open(os.path.join(ROOT, "include", "llie.h")).read()
    for sym in ("llie_ssim_grad_scratch_bytes", "llie_ssim_grad_f32", "llie_x0_loss"):
        assert sym in native.EXPORTS
        assert re.search(r"\b" + sym + r"\(", header)
        assert hasattr(native.lib(), sym)


def train_script():
    sys.path.insert(0, os.path.join(ROOT, "scripts"))
    try:
        return importlib.import_module("train")
    finally:
        sys.path.remove(os.path.join(ROOT, "scripts"))


def test_flags_reach_the_trainer_keywords():
    mod = train_script()
    args = mod.parse_args([])
    assert args.x0_ssim_weight == 0.0 and args.x0_l1_weight == 0.0 and type(args.x0_ssim_weight) is float
    args = mod.parse_args(["--x0_ssim_weight", "0.5", "--x0_l1_weight", "0.25"])
    kw = mod.x0_weights_from_args(args)
    assert kw == {"x0_ssim_weight": 0.5, "x0_l1_weight": 0.25}
    for fn in (M.train_model, M.LowLightTrainer.__init__, M.TrainStep.__init__):
        params = inspect.signature(fn).parameters
        for name in kw:
            assert params[name].default == 0.0, (fn, name)
    for name in kw:
        assert inspect.signature(M.LowLightDiffusion.compute_loss).parameters[name].default == 0.0
    # ... and are not TrainingConfig fields: its field list (the checkpoint's "config" entry) is unchanged
    names = [f.name for f in dataclasses.fields(M.TrainingConfig)]
    assert not [n for n in names if "x0" in n or "ssim" in n]
    assert names[-4:] == ["compute_dtype", "seed", "use_synthetic", "progress"]
