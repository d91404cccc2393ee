"""Image quality against ground truth: PSNR and SSIM on the device, and `evaluate` over a paired validation set.

One definition serves the NumPy twin here, the kernels (csrc/metrics.hip) and the tests.  All arithmetic is float64 on the
mapped values: x = (v - lo) / (hi - lo) for float images in `data_range = (lo, hi)` (the model's range is (-1, 1)), x = byte / 255
for uint8 images.

  window   g[k] = exp(-(k - 5)^2 / (2 * 1.5^2)), k = 0 .. 10, normalised to sum 1; the 2-D window is g (x) g, applied along the rows,
           then along the columns, taps in ascending order
  ssim     Wang et al. 2004 on RGB (no luma conversion): at each of the (H - 10) x (W - 10) valid positions (those whose 11 x 11
           window lies inside the image) and for each channel, the weighted means mx, my and the biased moments
           sx2 = sum w x^2 - mx^2, sy2 = sum w y^2 - my^2, sxy = sum w x y - mx my;
           map = (2 mx my + C1)(2 sxy + C2) / ((mx^2 + my^2 + C1)(sx2 + sy2 + C2)), C1 = 1e-4, C2 = 9e-4 (K1 = 0.01, K2 = 0.03, L = 1);
           ssim = mean of the map over the 3 channels and all valid positions
  mse      mean of (x - y)^2 over all 3 H W values, border included
  psnr     -10 log10(mse), +inf when mse == 0

SSIM as a loss (`ssim_loss`, `ssim_grad_host`; csrc/ssimloss.hip): the gradient of that definition with respect to the first
image.  With the five filtered maps mx, my, xx, yy, xy at a valid position and sx = xx - mx^2, sy = yy - my^2, sxy = xy - mx my,
A1 = 2 mx my + C1, A2 = 2 sxy + C2, B1 = mx^2 + my^2 + C1, B2 = sx + sy + C2, S = A1 A2 / (B1 B2):
  dmx = (2 my A2 - 2 my A1) / (B1 B2) - S (2 mx / B1 - 2 mx / B2),   dxx = -S / B2,   dxy = 2 A1 / (B1 B2)
  d ssim / d x = [W^T(dmx) + 2 x W^T(dxx) + y W^T(dxy)] / (3 (H - 10) (W - 10)),   d ssim / d a = d ssim / d x / (hi - lo)
W^T is the transposed window filter: a full correlation that is zero outside the valid region and returns H x W.  The twin is
float64; the device evaluates the same formulas in fp32 (second moments as written, xx - mx^2, not around the window mean) and
carries the sums over tiles in double.

`image_metrics_host` is that definition in code; `image_metrics` runs it on the device (no CPU fallback) and differs from the
twin only in the order of its sums.  skimage's `structural_similarity` defaults differ in two ways: it uses the sample covariance
(a factor 121 / 120 on the second moments) and, with `gaussian_weights=True`, crops a border of 5 pixels from a map computed with
reflected edges, where this definition takes the valid positions of an unpadded filter.
"""
from __future__ import annotations

from collections import namedtuple
from contextlib import contextmanager
from typing import Dict, Optional, Sequence, Tuple

import numpy as np
import torch
import torch.nn.functional as F

from . import _native as N
from .data import DeviceFrameStore, DevicePairLoader
from .ddim import check_sampler
from .guidance import guided_keyword as _guided_kw
from .tiling import enhance_tiled, enhance_frame_u8, frame_pad, resolve_tile_plan

WINDOW_TAPS, WINDOW_SIGMA = 11, 1.5
C1, C2 = 1e-4, 9e-4
TILE_H, TILE_W = 16, 32  # kMetricTileH, kMetricTileW (csrc/kernels.h): valid positions per workgroup of the device kernel

ImageMetrics = namedtuple("ImageMetrics", ["mse", "psnr", "ssim"])


def ssim_window() -> np.ndarray:
    """float64 [11]: the normalised Gaussian taps of one axis."""
    k = np.arange(WINDOW_TAPS, dtype=np.float64) - (WINDOW_TAPS // 2)
    g = np.exp(-(k * k) / (2.0 * WINDOW_SIGMA * WINDOW_SIGMA))
    return g / g.sum()


# ------------------------------------------------------------------ the host twin (float64 NumPy)
def _mapped_pair(a, b, data_range) -> Tuple[np.ndarray, np.ndarray]:
    """-> x, y float64 [B,3,H,W] in [0, 1] units."""
    a, b = np.asarray(a), np.asarray(b)
    if a.shape != b.shape or a.dtype != b.dtype:
        raise ValueError(f"the two images must have one shape and dtype, got {a.dtype} {a.shape} and {b.dtype} {b.shape}")
    if a.dtype == np.uint8:
        if a.ndim == 3:
            a, b = a[None], b[None]
        if a.ndim != 4 or a.shape[3] != 3:
            raise ValueError(f"uint8 images are HWC RGB [B,H,W,3] or [H,W,3], got {a.shape}")
        x, y = (np.ascontiguousarray(v.transpose(0, 3, 1, 2)).astype(np.float64) / 255.0 for v in (a, b))
    elif np.issubdtype(a.dtype, np.floating):
        if a.ndim != 4 or a.shape[1] != 3:
            raise ValueError(f"float images are NCHW [B,3,H,W], got {a.shape}")
        lo, hi = (float(np.float32(v)) for v in data_range)  # as the C ABI carries them
        if not lo != hi:
            raise ValueError(f"data_range must span an interval, got {tuple(data_range)}")
        x, y = ((np.ascontiguousarray(v, dtype=np.float64) - lo) / (hi - lo) for v in (a, b))
    else:
        raise ValueError(f"images must be float [B,3,H,W] or uint8 [B,H,W,3], got {a.dtype}")
    if x.shape[2] < WINDOW_TAPS or x.shape[3] < WINDOW_TAPS:
        raise ValueError(f"images must be at least {WINDOW_TAPS} x {WINDOW_TAPS} (one window), got {x.shape[2]} x {x.shape[3]}")
    return x, y


def _window_filter(m: np.ndarray) -> np.ndarray:
    """[..., H, W] -> [..., H - 10, W - 10]: the window along the rows, then along the columns."""
    g = ssim_window()
    w = m.shape[-1] - WINDOW_TAPS + 1
    rows = np.zeros(m.shape[:-1] + (w,), dtype=np.float64)
    for k in range(WINDOW_TAPS):
        rows = rows + g[k] * m[..., k:k + w]
    h = m.shape[-2] - WINDOW_TAPS + 1
    out = np.zeros(m.shape[:-2] + (h, w), dtype=np.float64)
    for k in range(WINDOW_TAPS):
        out = out + g[k] * rows[..., k:k + h, :]
    return out


def filtered_maps(x: np.ndarray, y: np.ndarray):
    """The five windowed maps of the definition: E[x], E[y], E[x^2], E[y^2], E[xy] over the valid positions."""
    return tuple(_window_filter(m) for m in (x, y, x * x, y * y, x * y))


def image_metrics_host(a, b, data_range: Tuple[float, float] = (-1.0, 1.0)) -> ImageMetrics:
    """The definition of the module docstring: float [B,3,H,W] in `data_range`, or uint8 [B,H,W,3] / [H,W,3] (x = byte / 255,
    `data_range` ignored) -> float64 arrays (mse, psnr, ssim) of shape [B].  ValueError below 11 x 11."""
    x, y = _mapped_pair(a, b, data_range)
    mx, my, xx, yy, xy = filtered_maps(x, y)
    sx2, sy2, sxy = xx - mx * mx, yy - my * my, xy - mx * my
    ssim_map = ((2.0 * mx * my + C1) * (2.0 * sxy + C2)) / ((mx * mx + my * my + C1) * (sx2 + sy2 + C2))
    d = x - y
    mse = (d * d).mean(axis=(1, 2, 3))
    with np.errstate(divide="ignore"):
        psnr = -10.0 * np.log10(mse)
    return ImageMetrics(mse, psnr, ssim_map.mean(axis=(1, 2, 3)))


# ------------------------------------------------------------------ the gradient's host twin
def _window_taps(dtype) -> np.ndarray:
    return ssim_window().astype(dtype)


def _filter_valid(m: np.ndarray) -> np.ndarray:
    """`_window_filter` in the dtype of `m`."""
    g = _window_taps(m.dtype)
    w = m.shape[-1] - WINDOW_TAPS + 1
    rows = np.zeros(m.shape[:-1] + (w,), dtype=m.dtype)
    for k in range(WINDOW_TAPS):
        rows = rows + g[k] * m[..., k:k + w]
    h = m.shape[-2] - WINDOW_TAPS + 1
    out = np.zeros(m.shape[:-2] + (h, w), dtype=m.dtype)
    for k in range(WINDOW_TAPS):
        out = out + g[k] * rows[..., k:k + h, :]
    return out


def _filter_transposed(c: np.ndarray) -> np.ndarray:
    """[..., H - 10, W - 10] -> [..., H, W]: the transpose of `_filter_valid`, along the columns, then along the rows."""
    g = _window_taps(c.dtype)
    h, w = c.shape[-2], c.shape[-1]
    cols = np.zeros(c.shape[:-2] + (h + WINDOW_TAPS - 1, w), dtype=c.dtype)
    for k in range(WINDOW_TAPS):
        cols[..., k:k + h, :] += g[k] * c
    out = np.zeros(cols.shape[:-1] + (w + WINDOW_TAPS - 1,), dtype=c.dtype)
    for k in range(WINDOW_TAPS):
        out[..., k:k + w] += g[k] * cols
    return out


def ssim_grad_mapped(x: np.ndarray, y: np.ndarray) -> Tuple[np.ndarray, np.ndarray]:
    """The formulas of the module docstring on mapped images x, y [B,3,H,W], in their dtype (float64 for the twin; the tests
    evaluate them in float32 to size the device's rounding) -> (ssim [B], d ssim / d x [B,3,H,W])."""
    t = x.dtype.type
    c1, c2 = t(C1), t(C2)
    mx, my, xx, yy, xy = (_filter_valid(m) for m in (x, y, x * x, y * y, x * y))
    sx, sy, sxy = xx - mx * mx, yy - my * my, xy - mx * my
    a1, a2 = t(2) * mx * my + c1, t(2) * sxy + c2
    b1, b2 = mx * mx + my * my + c1, sx + sy + c2
    inv = t(1) / (b1 * b2)
    s = a1 * a2 * inv
    dmx = (t(2) * my * a2 - t(2) * my * a1) * inv - s * (t(2) * mx / b1 - t(2) * mx / b2)
    dxx = -s / b2
    dxy = t(2) * a1 * inv
    n = t(3.0 * s.shape[-2] * s.shape[-1])
    grad = (_filter_transposed(dmx) + t(2) * x * _filter_transposed(dxx) + y * _filter_transposed(dxy)) / n
    return s.mean(axis=(1, 2, 3)), grad


def ssim_grad_host(a, b, data_range: Tuple[float, float] = (-1.0, 1.0)) -> Tuple[np.ndarray, np.ndarray]:
    """float [B,3,H,W] images in `data_range` -> float64 (ssim [B], d ssim / d a [B,3,H,W]): `image_metrics_host`'s SSIM and its
    gradient with respect to the first image, by the formulas of the module docstring.  ValueError below 11 x 11."""
    if np.asarray(a).dtype == np.uint8:
        raise ValueError("ssim_grad_host takes float images [B,3,H,W]")
    x, y = _mapped_pair(a, b, data_range)
    lo, hi = (float(np.float32(v)) for v in data_range)
    ssim, gx = ssim_grad_mapped(x, y)
    return ssim, gx / (hi - lo)


# ------------------------------------------------------------------ the device function
def _require_hip(t, what: str) -> None:
    if not isinstance(t, torch.Tensor) or t.device.type != "cuda":
        where = t.device if isinstance(t, torch.Tensor) else type(t).__name__
        raise RuntimeError(f"{what} runs only on a HIP device (got '{where}'); there is no CPU fallback")


def _metrics_out3(a: torch.Tensor, b: torch.Tensor, data_range) -> torch.Tensor:
    """float64 [B,3] = (mse, psnr, ssim) per image, on the inputs' device, no synchronisation."""
    _require_hip(a, "image_metrics")
    _require_hip(b, "image_metrics")
    if a.shape != b.shape or a.dtype != b.dtype or a.device != b.device:
        raise ValueError(f"the two images must have one shape, dtype and device, got {a.dtype} {tuple(a.shape)} on {a.device} and "
                         f"{b.dtype} {tuple(b.shape)} on {b.device}")
    u8 = a.dtype == torch.uint8
    if u8:
        if a.dim() == 3:
            a, b = a[None], b[None]
        if a.dim() != 4 or a.shape[3] != 3:
            raise ValueError(f"uint8 images are HWC RGB [B,H,W,3] or [H,W,3], got {tuple(a.shape)}")
        batch, h, w = a.shape[0], a.shape[1], a.shape[2]
    else:
        if a.dtype != torch.float32 or a.dim() != 4 or a.shape[1] != 3:
            raise ValueError(f"images must be fp32 NCHW [B,3,H,W] or uint8 HWC, got {a.dtype} {tuple(a.shape)}")
        batch, h, w = a.shape[0], a.shape[2], a.shape[3]
    a, b = a.detach().contiguous(), b.detach().contiguous()
    dev = a.device
    L = N.lib()
    nbytes = int(L.llie_image_metrics_scratch_bytes(batch, h, w))
    if nbytes < 0:
        N.check(nbytes, f"image_metrics: {batch} images of {h} x {w} (at least 1 image of 11 x 11)")
    scratch = torch.empty(nbytes // 8, dtype=torch.float64, device=dev)
    out = torch.empty(batch, 3, dtype=torch.float64, device=dev)
    with torch.cuda.device(dev):
        st = torch.cuda.current_stream(dev).cuda_stream
        if u8:
            rc = L.llie_image_metrics_u8(a.data_ptr(), b.data_ptr(), batch, h, w, out.data_ptr(), scratch.data_ptr(), nbytes, st)
        else:
            lo, hi = float(data_range[0]), float(data_range[1])
            rc = L.llie_image_metrics_f32(a.data_ptr(), b.data_ptr(), batch, h, w, lo, hi, out.data_ptr(), scratch.data_ptr(), nbytes, st)
    N.check(rc, "image_metrics")
    return out


def image_metrics(a: torch.Tensor, b: torch.Tensor, data_range: Tuple[float, float] = (-1.0, 1.0)) -> ImageMetrics:
    """Device twin of image_metrics_host: fp32 NCHW [B,3,H,W] in `data_range`, or uint8 HWC [B,H,W,3] / [H,W,3], on a HIP device ->
    ImageMetrics(mse, psnr, ssim), float64 device tensors [B].  Two launches on the current stream, no synchronisation; the
    results are bitwise reproducible and do not depend on the batch an image is scored in."""
    out = _metrics_out3(a, b, data_range)
    return ImageMetrics(out[:, 0], out[:, 1], out[:, 2])


def ssim_grad(a: torch.Tensor, b: torch.Tensor, data_range: Tuple[float, float] = (-1.0, 1.0), *,
              upstream: Optional[torch.Tensor] = None, need_grad: bool = True) -> Tuple[torch.Tensor, Optional[torch.Tensor]]:
    """llie_ssim_grad_f32: fp32 NCHW [B,3,H,W] on a HIP device -> (ssim fp32 [B], upstream_b * d ssim_b / d a, or None with
    `need_grad=False`).  `upstream` is a device fp32 [B] (default: ones).  No synchronisation."""
    _require_hip(a, "ssim_loss")
    _require_hip(b, "ssim_loss")
    if a.shape != b.shape or a.device != b.device or a.dtype != torch.float32 or b.dtype != torch.float32 or a.dim() != 4 or a.shape[1] != 3:
        raise ValueError(f"the two images must be fp32 NCHW [B,3,H,W] of one shape on one device, got {a.dtype} {tuple(a.shape)} and "
                         f"{b.dtype} {tuple(b.shape)}")
    batch, h, w = a.shape[0], a.shape[2], a.shape[3]
    a, b = a.detach().contiguous(), b.detach().contiguous()
    dev = a.device
    if upstream is not None:
        if upstream.dtype != torch.float32 or tuple(upstream.shape) != (batch,) or upstream.device != dev:
            raise ValueError(f"upstream must be fp32 [{batch}] on {dev}")
        upstream = upstream.detach().contiguous()
    L = N.lib()
    nbytes = int(L.llie_ssim_grad_scratch_bytes(batch, h, w))
    if nbytes < 0:
        N.check(nbytes, f"ssim_loss: {batch} images of {h} x {w} (at least 1 image of 11 x 11)")
    scratch = torch.empty((nbytes + 7) // 8, dtype=torch.float64, device=dev)
    ssim = torch.empty(batch, dtype=torch.float32, device=dev)
    da = torch.empty_like(a) if need_grad else None
    lo, hi = float(data_range[0]), float(data_range[1])
    with torch.cuda.device(dev):
        rc = L.llie_ssim_grad_f32(a.data_ptr(), b.data_ptr(), batch, h, w, lo, hi, upstream.data_ptr() if upstream is not None else None,
                                  ssim.data_ptr(), da.data_ptr() if da is not None else None, scratch.data_ptr(), nbytes,
                                  torch.cuda.current_stream(dev).cuda_stream)
    N.check(rc, "ssim_loss")
    return ssim, da


class _SsimLossFn(torch.autograd.Function):
    """1 - SSIM as an autograd node of the first image: forward = llie_ssim_grad_f32 (value and d ssim / d a in one pass over the
    images), backward = -grad_output_b times the gradient it wrote."""

    @staticmethod
    def forward(ctx, a, b, lo, hi):
        need = ctx.needs_input_grad[0]
        ssim, da = ssim_grad(a, b, (lo, hi), need_grad=need)
        if need:
            ctx.save_for_backward(da)
        return 1.0 - ssim

    @staticmethod
    def backward(ctx, grad_output):
        da, = ctx.saved_tensors
        return -grad_output.reshape(-1, 1, 1, 1) * da, None, None, None


def ssim_loss(a: torch.Tensor, b: torch.Tensor, data_range: Tuple[float, float] = (-1.0, 1.0)) -> torch.Tensor:
    """1 - SSIM(a, b) per image: fp32 [B], for fp32 NCHW [B,3,H,W] images in `data_range` on a HIP device (no CPU fallback).
    The SSIM is `image_metrics`' definition evaluated in fp32.  Differentiable with respect to `a` only (`b` is the reference
    image: one that requires grad raises ValueError).  Bitwise reproducible, and an image's value and gradient do not depend on
    the batch it is scored in."""
    if isinstance(b, torch.Tensor) and b.requires_grad:
        raise ValueError("ssim_loss differentiates with respect to `a` only; `b` must not require grad")
    return _SsimLossFn.apply(a, b, float(data_range[0]), float(data_range[1]))


# ------------------------------------------------------------------ evaluation over a validation set
@contextmanager
def _swapped_weights(model, weights: Optional[Sequence[torch.Tensor]]):
    """Copies `weights` (in model.parameters() order) into the parameters for the duration of the block and restores the
    original values afterwards, whatever happens inside (the reference's apply_shadow / restore).  The engine notices both
    writes through its content check."""
    if weights is None:
        yield
        return
    params = list(model.parameters())
    weights = list(weights)
    if len(weights) != len(params):
        raise ValueError(f"weights has {len(weights)} tensors, the model {len(params)} parameters")
    for i, (p, w) in enumerate(zip(params, weights)):
        if tuple(w.shape) != tuple(p.shape):
            raise ValueError(f"weights[{i}] is {tuple(w.shape)}, the parameter {tuple(p.shape)}")
    saved = [p.detach().clone() for p in params]
    try:
        with torch.no_grad():
            for p, w in zip(params, weights):
                p.data.copy_(w)
        yield
    finally:
        with torch.no_grad():
            for p, s in zip(params, saved):
                p.data.copy_(s)


def _steps_of(model, num_inference_steps: Optional[int], dev, sampler: str = "lcm") -> Tuple[int, int]:
    """(the argument `enhance` takes, the number of noise draws it consumes: one per step for the LCM loop, 1 for DDIM and
    DPM-Solver++)."""
    nsteps = model.num_inference_steps if num_inference_steps is None else int(num_inference_steps)
    if check_sampler(sampler) != "lcm":
        (model.ddim_schedule if sampler == "ddim" else model.dpm_schedule)(nsteps)  # the schedule's ValueErrors, before anything is drawn
        return nsteps, 1
    model.scheduler.set_timesteps(nsteps, device=dev)
    return nsteps, len(model.scheduler._timestep_list)


def _summary(names, triples: np.ndarray, loss: Optional[float]) -> Dict[str, object]:
    mse, psnr, ssim = ([float(v) for v in triples[:, j]] for j in range(3))
    n = len(names)
    res: Dict[str, object] = {"n": n, "psnr": sum(psnr) / n, "ssim": sum(ssim) / n, "mse": sum(mse) / n}
    if loss is not None:
        res["loss"] = loss
    res["per_image"] = {"filename": list(names), "psnr": psnr, "ssim": ssim, "mse": mse}
    return res


@torch.no_grad()
def evaluate(model, loader: DevicePairLoader, *, num_inference_steps: Optional[int] = None, seed: int = 0, loss: bool = True,
             weights: Optional[Sequence[torch.Tensor]] = None, sampler: str = "lcm",
             guidance_scale: Optional[float] = None, guidance_rescale: Optional[float] = None) -> Dict[str, object]:
    """PSNR / SSIM / MSE of `model.enhance` against the normal-light images of `loader` (normally a "val" DevicePairLoader:
    centre crops in file order, last partial batch kept), and the validation loss of the reference's `LowLightTrainer.validate`.

    Draw recipe (part of the contract; the global generator is neither read nor advanced):
      g = torch.Generator(device=dev).manual_seed(seed); steps = the scheduler's step count for `num_inference_steps`
      (default model.num_inference_steps); S = model.image_size; T = scheduler.config.num_train_timesteps.  Per batch of b images,
      in loader order:
        noise = torch.randn(steps, b, 3, S, S, generator=g, device=dev)
        if loss:  t = torch.randint(0, T, (b,), generator=g, device=dev);  eps = torch.randn(b, 3, S, S, generator=g, device=dev)
      `model.enhance(low_light, num_inference_steps, noise=noise)` is scored against `normal_light` by `image_metrics` in the
      model's range (-1, 1); the batch loss is F.mse_loss(model.forward(low_light, normal_light, timesteps=t, noise=eps)
      ["noise_pred"], eps) without gradients.
      sampler="ddim" scores `model.enhance(..., sampler="ddim")`, the deterministic sampler of a many-step model, at any
      `num_inference_steps` in 1..T: steps = 1 in the recipe above (the initial latents are the only noise), the rest is unchanged.
      sampler="dpmpp_2m" scores the second-order sampler of such a model (dpm.py) the same way, also with steps = 1, at any step
      count `model.dpm_schedule` accepts.
      A rectangular loader (`crop_size` = (H, W), H != W; frame-size training) is scored through `model.enhance_frame` and the
      loss runs at that shape: the same recipe with every [.., 3, S, S] draw [.., 3, H, W].  A square loader must crop
      model.image_size, as before.
      guidance_scale=w scores `model.enhance(..., guidance_scale=w)` (classifier-free guidance; None: off) and
      guidance_rescale=phi adds `guidance_rescale=phi` to that call; the draws and the loss are unchanged.
      The loss is always this flat, unweighted MSE: a trainer's `snr_gamma` (Min-SNR-gamma weighting, snrloss.py) does not reach
      it, so runs with and without that flag stay comparable.

    Returns {"n", "psnr", "ssim", "mse", ["loss",] "per_image": {"filename", "psnr", "ssim", "mse"}}: psnr / ssim / mse are the
    means over images of the per-image values (float64 sums in file order), loss = sum of batch losses / len(loader).  Everything
    stays on the device until one copy at the end.  `weights=` (e.g. FusedAdamW.ema_tensors(), in model.parameters() order) is
    copied into the parameters for the call and the original values are restored afterwards, also when the call raises."""
    check_sampler(sampler)
    guided = _guided_kw(guidance_scale, guidance_rescale)
    if not isinstance(loader, DevicePairLoader):
        raise ValueError(f"evaluate expects a DevicePairLoader, got {type(loader).__name__}")
    dev = loader.store.device
    if dev.type != "cuda":
        raise RuntimeError(f"evaluate runs only on a HIP device (the frame store is on '{dev}'); there is no CPU fallback")
    with _swapped_weights(model, weights):
        s = int(model.image_size)
        hh, ww = loader.crop_size
        frame = hh != ww
        if not frame and hh != s:
            raise ValueError(f"the loader crops {hh} x {ww}, the model takes {s} x {s}")
        enhance = model.enhance_frame if frame else model.enhance
        nsteps, steps = _steps_of(model, num_inference_steps, dev, sampler)
        t_max = int(model.scheduler.config.num_train_timesteps)
        g = torch.Generator(device=dev).manual_seed(int(seed))
        names, triples, losses = [], [], []
        for batch in loader:
            low, normal = batch["low_light"], batch["normal_light"]
            b = low.shape[0]
            noise = torch.randn(steps, b, 3, hh, ww, generator=g, device=dev)
            if loss:
                t = torch.randint(0, t_max, (b,), generator=g, device=dev)
                eps = torch.randn(b, 3, hh, ww, generator=g, device=dev)
            triples.append(_metrics_out3(enhance(low, nsteps, noise=noise, sampler=sampler, **guided), normal, (-1.0, 1.0)))
            if loss:
                pred = model.forward(low, normal, timesteps=t, noise=eps, frame=frame)["noise_pred"]
                losses.append(F.mse_loss(pred, eps).double().reshape(1))
            names += list(batch["filename"])
        if not triples:
            raise ValueError("the loader yields no batch")
        flat = torch.cat([torch.cat(triples).reshape(-1)] + losses).cpu().numpy()  # the one device-to-host copy
    n = len(names)
    total = float(sum(float(v) for v in flat[3 * n:]) / len(losses)) if loss else None
    return _summary(names, flat[:3 * n].reshape(n, 3), total)


@torch.no_grad()
def evaluate_full_resolution(model, store: DeviceFrameStore, *, num_inference_steps: Optional[int] = None, seed: int = 0,
                             overlap: Optional[int] = None, tile_batch: int = 32,
                             weights: Optional[Sequence[torch.Tensor]] = None, mode: str = "tiled",
                             sync: str = "none", sampler: str = "lcm", tile=None,
                             max_tile_pixels: Optional[int] = None, guidance_scale: Optional[float] = None,
                             guidance_rescale: Optional[float] = None) -> Dict[str, object]:
    """PSNR / SSIM / MSE at the images' own resolution: every low-light frame of the paired `store` (any sizes >= 11 x 11) goes
    through `enhance_tiled` and is scored against its normal-light frame on the bytes (x = byte / 255).

    Draw recipe: g = torch.Generator(device=dev).manual_seed(seed); per pair i, in file order, with (H, W) its size and S =
    model.image_size:  canvas = torch.randn(steps, 3, max(H, S), max(W, S), generator=g, device=dev), then
    enhance_tiled(model, store.frame(i), num_inference_steps, overlap=overlap, tile_batch=tile_batch, noise=canvas) against
    store.frame(n + i).  Returns evaluate's dictionary without "loss"; `weights=` as there.

    mode="frame": every image goes through `enhance_frame_u8` instead (one run of the network at the image's own size; images
    past the engine's size cap raise ValueError).  The same generator, one draw per pair in the same order, with Hp / Wp =
    frame_pad(H / W):  canvas = torch.randn(steps, 3, Hp, Wp, generator=g, device=dev), then enhance_frame_u8(model,
    store.frame(i), num_inference_steps, noise=canvas).  `overlap` / `tile_batch` / `sync` belong to the tiles and are refused.

    sync="latents" (mode="tiled") passes through to `enhance_tiled`: the tiles share one latent canvas at every step.
    tile= / max_tile_pixels= (mode="tiled") pass through as well: with tile=(TH, TW) the canvas of the recipe is
    [steps, 3, max(H, TH), max(W, TW)], and with tile="auto" TH x TW is the tile `auto_tile_plan` gives that image.
    sampler="ddim" passes through to `enhance_tiled` / `enhance_frame_u8` in every mode; steps = 1 in the draws above.
    sampler="dpmpp_2m" does the same, except that `enhance_tiled` refuses it with sync="latents".
    guidance_scale= passes through the same way (refused by `enhance_tiled` with sync="latents"), and guidance_rescale= with it
    (with tiles the rescale's statistic is per tile: `enhance_tiled`)."""
    if mode not in ("tiled", "frame"):
        raise ValueError(f'mode must be "tiled" or "frame", got {mode!r}')
    if mode == "frame" and (overlap is not None or tile_batch != 32 or sync != "none" or tile is not None or max_tile_pixels is not None):
        raise ValueError('overlap / tile_batch / sync / tile / max_tile_pixels belong to mode="tiled"')
    if sync not in ("none", "latents"):
        raise ValueError(f'sync must be "none" or "latents", got {sync!r}')
    check_sampler(sampler)
    if sync == "latents" and sampler == "dpmpp_2m":
        raise ValueError('evaluate_full_resolution(sync="latents", sampler="dpmpp_2m") is not provided: enhance_tiled refuses the pair')
    guided = _guided_kw(guidance_scale, guidance_rescale)
    if not isinstance(store, DeviceFrameStore) or not store.paired:
        raise ValueError("evaluate_full_resolution expects a paired DeviceFrameStore")
    dev = store.device
    if dev.type != "cuda":
        raise RuntimeError(f"evaluate_full_resolution runs only on a HIP device (the frame store is on '{dev}'); there is no CPU fallback")
    with _swapped_weights(model, weights):
        nsteps, steps = _steps_of(model, num_inference_steps, dev, sampler)
        g = torch.Generator(device=dev).manual_seed(int(seed))
        n = len(store)
        triples = []
        for i, (h, w) in enumerate(store.sizes):
            if mode == "frame":
                canvas = torch.randn(steps, 3, frame_pad(h), frame_pad(w), generator=g, device=dev)
                out = enhance_frame_u8(model, store.frame(i), nsteps, noise=canvas, sampler=sampler, **guided)
            else:
                sh, sw, vy, vx = resolve_tile_plan(model, (h, w), tile, overlap, max_tile_pixels)
                canvas = torch.randn(steps, 3, max(h, sh), max(w, sw), generator=g, device=dev)
                if tile is None:
                    plan = {"overlap": overlap}
                else:  # the plan is settled here, so "auto" is passed on as the tile it chose
                    plan = {"tile": (sh, sw), "overlap": (vy, vx)}
                out = enhance_tiled(model, store.frame(i), nsteps, tile_batch=tile_batch, noise=canvas, sync=sync, sampler=sampler,
                                    **plan, **guided)
            triples.append(_metrics_out3(out, store.frame(n + i), None))
        flat = torch.cat(triples).cpu().numpy()
    return _summary(store.names, flat, None)
