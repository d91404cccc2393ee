"""Classifier-free guidance: the definitions, as NumPy fp32 twins of csrc/guidance.hip, and the argument checks.

The denoiser is conditional: every forward reads the noised image and the low-light condition.  Guidance has three parts --
train with the condition dropped some of the time, sample with a combination of a conditional and an unconditional output,
distil the guided teacher into a student that needs one forward -- and they share three definitions:

  null condition     the all-zero image in the model's range: cond = 0.0 everywhere (positive-zero bits), fp32 [B,3,H,W].  A
                     constant; there is no learned embedding and no parameter, so `state_dict` stays the reference's.
  guided output      o = o_u + w (o_c - o_u) in fp32 for a network output of either prediction type; the difference, the product
                     and the sum are each rounded on their own (no fused multiply-add).  w is a host scalar when sampling, a
                     device fp32 [B] when distilling.  w = 1 is the conditional output up to that rounding, w = 0 the
                     unconditional one.
  condition dropout  row b of the condition becomes the null condition when u[b] < p, strictly; u is [B] uniform in [0, 1), p in
                     [0, 1], compared in fp32.  A select, not a multiply: an inf or NaN in a dropped row gives 0.  p = 0 drops
                     nothing, p = 1 everything.

  guidance rescale   (Lin et al. 2024, section 3.4) the guided output of row b times f_b = phi r_b + (1 - phi), r_b the ratio of the
                     standard deviations of o_c[b] and o[b] over the whole row, from float64 moments: `guide_rescale_host` is the
                     definition, `guide_rescale_array` the fp32 twin.  phi = 0 is the guided output, phi = 1 matches the deviations.

The device runs the same fp32 operations (llie_guide, llie_guidance_pair, llie_cond_dropout, llie_guide_rescale given its factor),
so these functions give its bits; its tests compare against them.  Nothing here needs a GPU or the engine's library.
"""
from __future__ import annotations

import math
from typing import Callable, Dict, Optional, Sequence, Tuple

import numpy as np


# ---------------------------------------------------------------------- argument checks
def check_guidance_scale(guidance_scale) -> Optional[float]:
    """`guidance_scale=` of the sampling entries: None (off) or a finite number -> None or its float.  ValueError otherwise."""
    if guidance_scale is None:
        return None
    if isinstance(guidance_scale, bool) or not isinstance(guidance_scale, (int, float, np.integer, np.floating)):
        raise ValueError(f"guidance_scale must be None or a finite number, got {guidance_scale!r}")
    w = float(guidance_scale)
    if not math.isfinite(w):
        raise ValueError(f"guidance_scale must be None or a finite number, got {guidance_scale!r}")
    return w


def guidance_is_on(guidance_scale) -> bool:
    """True when `guidance_scale` asks for the guided loop: None and 1.0 run the unguided path (o = o_c, one forward)."""
    w = check_guidance_scale(guidance_scale)
    return w is not None and w != 1.0


def check_guidance_rescale(guidance_rescale) -> float:
    """`guidance_rescale=` (phi) of the sampling and distillation entries: None (off) or a number in [0, 1] -> its float, None
    meaning 0.0.  ValueError otherwise (bool and NaN included)."""
    if guidance_rescale is None:
        return 0.0
    if isinstance(guidance_rescale, bool) or not isinstance(guidance_rescale, (int, float, np.integer, np.floating)) \
            or not 0.0 <= float(guidance_rescale) <= 1.0:
        raise ValueError(f"guidance_rescale must be None or a number in [0, 1], got {guidance_rescale!r}")
    return float(guidance_rescale)


def guided_keyword(guidance_scale, guidance_rescale=None) -> dict:
    """`guidance_scale=` (and `guidance_rescale=`) as the keywords a pass-through hands on to `enhance` / `enhance_frame`: nothing
    for a None, so the unguided call is the call it always was.  ValueError for a scale that is not finite or a rescale outside
    [0, 1]."""
    w = check_guidance_scale(guidance_scale)
    kw = {} if w is None else {"guidance_scale": w}
    if guidance_rescale is not None:
        kw["guidance_rescale"] = check_guidance_rescale(guidance_rescale)
    return kw


def check_cond_dropout(p) -> float:
    """`cond_dropout=` of the training entries: a probability in [0, 1] -> its float.  ValueError otherwise (NaN included)."""
    if isinstance(p, bool) or not isinstance(p, (int, float, np.integer, np.floating)) or not 0.0 <= float(p) <= 1.0:
        raise ValueError(f"cond_dropout must be a probability in [0, 1], got {p!r}")
    return float(p)


def check_guidance_range(guidance_scale_range) -> Tuple[float, float]:
    """`guidance_scale_range=(lo, hi)`: two finite numbers with lo <= hi -> (lo, hi) as floats.  ValueError otherwise."""
    try:
        lo, hi = guidance_scale_range
        lo, hi = check_guidance_scale(lo), check_guidance_scale(hi)
    except (TypeError, ValueError):
        raise ValueError(f"guidance_scale_range must be (lo, hi), finite with lo <= hi, got {guidance_scale_range!r}") from None
    if lo is None or hi is None or lo > hi:
        raise ValueError(f"guidance_scale_range must be (lo, hi), finite with lo <= hi, got {guidance_scale_range!r}")
    return lo, hi


# ---------------------------------------------------------------------- the twins
def _rows(x, who: str) -> np.ndarray:
    x = np.asarray(x, dtype=np.float32)
    if x.ndim < 2:
        raise ValueError(f"{who} must be [B, ...], got shape {x.shape}")
    return x


def guide_array(out_cond, out_uncond, w) -> np.ndarray:
    """o = o_u + w (o_c - o_u) in fp32, three roundings (llie_guide): out_cond / out_uncond [B, ...] of one shape, `w` a finite
    scalar or a [B] array (one scale per row, any value: the kernel reads those from the device and cannot refuse them)."""
    c, u = _rows(out_cond, "out_cond"), _rows(out_uncond, "out_uncond")
    if c.shape != u.shape:
        raise ValueError(f"out_cond and out_uncond must have one shape, got {c.shape} and {u.shape}")
    if np.ndim(w) == 0:
        wv = np.float32(check_guidance_scale(w if w is not None else float("nan")))
    else:
        wv = np.asarray(w, dtype=np.float32)
        if wv.shape != (c.shape[0],):
            raise ValueError(f"a per-row w must be [{c.shape[0]}], got {wv.shape}")
        wv = wv.reshape((-1,) + (1,) * (c.ndim - 1))
    with np.errstate(invalid="ignore", over="ignore"):
        d = (c - u).astype(np.float32)
        p = (wv * d).astype(np.float32)
        return (u + p).astype(np.float32)


def _rescale_ratio(c: np.ndarray, g: np.ndarray) -> np.ndarray:
    """r_b = sqrt(var_c / var_g) of fp32 rows in float64, from the moments S1 = sum x, S2 = sum x^2 of the widened values:
    var = max(S2 - S1^2 / n, 0), a NaN counting as 0.  1.0 where var_g is not > 0 or the fp32 rounding of r_b is not finite."""
    b = c.shape[0]
    c64, g64 = c.reshape(b, -1).astype(np.float64), g.reshape(b, -1).astype(np.float64)
    n = np.float64(c64.shape[1])
    with np.errstate(invalid="ignore", over="ignore", divide="ignore"):
        dc = (c64 * c64).sum(axis=1) - c64.sum(axis=1) ** 2 / n
        dg = (g64 * g64).sum(axis=1) - g64.sum(axis=1) ** 2 / n
        var_c, var_g = np.where(dc > 0, dc, 0.0), np.where(dg > 0, dg, 0.0)
        r = np.sqrt(var_c / np.where(var_g > 0, var_g, 1.0))
        ok = (var_g > 0) & np.isfinite(r.astype(np.float32))
    return np.where(ok, r, 1.0)


def guide_rescale_host(out_cond, out_uncond, w, phi) -> Tuple[np.ndarray, np.ndarray]:
    """Guidance rescale (Lin et al. 2024, section 3.4), the definition: (out, factor) in float64 for fp32 rows out_cond /
    out_uncond [B, ...].  g = `guide_array` (its three fp32 roundings), widened; over each whole row, in float64,
    r_b = sqrt(var_c / var_g) from the moments (`_rescale_ratio`: 1 for a constant row and for one element); phi is taken as its
    fp32 value; factor_b = phi r_b + (1 - phi); out = factor_b g.  phi = 1 gives row b the standard deviation of out_cond[b],
    phi = 0 returns g.  The usual formulation (the std over dims 1.., g std_c / std_g, then the phi-blend) agrees to 1e-10."""
    p = np.float64(np.float32(check_guidance_rescale(phi)))
    c = _rows(out_cond, "out_cond")
    g = guide_array(c, out_uncond, w)
    factor = p * _rescale_ratio(c, g) + (1.0 - p)
    return factor.reshape((-1,) + (1,) * (g.ndim - 1)) * g.astype(np.float64), factor


def guide_rescale_array(out_cond, out_uncond, w, phi, factor=None) -> np.ndarray:
    """The fp32 twin of llie_guide_rescale: out = fl(f_b g), g = `guide_array`.  With the device's `factor` [B] supplied these are
    the kernel's output bits; without it f_b = fl(fl(phi r32) + fl(1 - phi)), r32 the ratio of `guide_rescale_host` rounded once to
    fp32 -- within rounding of the device's, whose sums run in another order."""
    f = np.float32
    p = f(check_guidance_rescale(phi))
    c = _rows(out_cond, "out_cond")
    g = guide_array(c, out_uncond, w)
    if factor is None:
        r32 = _rescale_ratio(c, g).astype(f)
        fb = ((p * r32).astype(f) + f(f(1) - p)).astype(f) if p != 0 else np.ones(c.shape[0], dtype=f)
    else:
        fb = np.asarray(factor, dtype=f)
        if fb.shape != (c.shape[0],):
            raise ValueError(f"factor must be [{c.shape[0]}], got {fb.shape}")
    if p == 0 and factor is None:
        return g
    with np.errstate(invalid="ignore", over="ignore"):
        return (fb.reshape((-1,) + (1,) * (g.ndim - 1)) * g).astype(f)


def cond_dropout_array(cond, u, p) -> np.ndarray:
    """Row b of `cond` [B, ...] -> +0 where u[b] < p (fp32 comparison, strict), kept otherwise (llie_cond_dropout)."""
    x = _rows(cond, "cond")
    pv = np.float32(check_cond_dropout(p))
    uv = np.asarray(u, dtype=np.float32)
    if uv.shape != (x.shape[0],):
        raise ValueError(f"u must be [{x.shape[0]}], got {uv.shape}")
    with np.errstate(invalid="ignore"):
        drop = uv < pv
    out = x.copy()
    out[drop] = np.float32(0.0)
    return out


def guidance_pair_array(latents, cond) -> Tuple[np.ndarray, np.ndarray]:
    """(latents2, cond2) of llie_guidance_pair: the latents twice [2B, ...]; the condition followed by B null rows [2B, ...]."""
    x, c = _rows(latents, "latents"), _rows(cond, "cond")
    if x.shape != c.shape:
        raise ValueError(f"latents and cond must have one shape, got {x.shape} and {c.shape}")
    return np.concatenate([x, x]), np.concatenate([c, np.zeros_like(c)])


# ---------------------------------------------------------------------- the guided loop on the host
def _coef_fields(coef):
    if isinstance(coef, dict):
        get = coef.get
    else:
        get = lambda k, d=0: getattr(coef, k, d)  # noqa: E731
    f = np.float32
    return (f(get("sqrt_alpha_t")), f(get("sqrt_beta_t")), f(get("sqrt_alpha_prev")), f(get("sqrt_beta_prev")), bool(get("is_last", 0)),
            bool(get("v_prediction", 0)), bool(get("clamp_x0", 0)), int(get("sampler", 0)))


def scheduler_step_array(model_output, sample, noise, coef) -> np.ndarray:
    """One scheduler step of the sampling loop in fp32, each product and sum rounded on its own (llie_lcm_step): `coef` is an
    `N.StepCoef` (or any object / dict with its eight members).  LCM (sampler 0) re-noises x0 with `noise` on a non-final step;
    DDIM (sampler 1) uses the predicted noise and never reads `noise`.  -> the next latents, before the final clamp."""
    sa, sb, sap, sbp, last, vpred, clamp, sampler = _coef_fields(coef)
    e, x = np.asarray(model_output, dtype=np.float32), np.asarray(sample, dtype=np.float32)
    if e.shape != x.shape:
        raise ValueError(f"model_output and sample must have one shape, got {e.shape} and {x.shape}")
    f = np.float32
    with np.errstate(divide="ignore", invalid="ignore", over="ignore"):
        if vpred:
            x0 = ((sa * x).astype(f) - (sb * e).astype(f)).astype(f)
        else:
            x0 = ((x - (sb * e).astype(f)).astype(f) / sa).astype(f)
        if clamp:
            x0 = np.minimum(np.maximum(x0, f(-1)), f(1))
        if last:
            return x0
        if not sampler:
            if noise is None:
                raise ValueError("a non-final LCM step needs a noise draw")
            nz = np.asarray(noise, dtype=f)
        elif vpred:
            nz = ((sa * e).astype(f) + (sb * x).astype(f)).astype(f)
        else:
            nz = e
        return ((sap * x0).astype(f) + (sbp * nz).astype(f)).astype(f)


def guided_enhance_host(unet_fn: Callable, low, noise, timesteps: Sequence[int], coefs: Sequence, w, rescale=None) -> Dict[str, object]:
    """The guided loop of `enhance(..., guidance_scale=w)` on the host, the denoiser passed in, written like
    `ddim.ddim_enhance_host`: unet_fn(latents fp32 [B,3,H,W], cond fp32 [B,3,H,W], t) -> the network output [B,3,H,W].
    `low` [B,3,H,W]; `noise` [draws,B,3,H,W] in `enhance`'s order (the initial latents, then one draw per non-final LCM step; DDIM
    reads only the first); `timesteps` and `coefs` (one `N.StepCoef` each) are the schedule.  Per step: the conditional output on
    `low`, the unconditional one on the null condition, `guide_array`, `scheduler_step_array` -- all fp32, the device's operations.
    `w` None runs the unguided loop (one call per step, no combination); any finite `w`, 1.0 included, runs the guided one.
    `rescale` (phi; None or 0: off, the loop above) replaces `guide_array` by `guide_rescale_array` in the guided loop.
    -> {"enhanced" (clamped), "intermediate" (latents after each step), "noise_pred" (the guided output of each step), "timesteps"}."""
    wv = check_guidance_scale(w)
    phi = check_guidance_rescale(rescale)
    low = np.ascontiguousarray(np.asarray(low, dtype=np.float32))
    noise = np.asarray(noise, dtype=np.float32)
    ts = [int(t) for t in timesteps]
    if len(coefs) != len(ts) or not ts:
        raise ValueError(f"one coefficient per timestep, got {len(coefs)} and {len(ts)}")
    if noise.ndim != low.ndim + 1 or noise.shape[1:] != low.shape or noise.shape[0] < 1:
        raise ValueError(f"noise must be [draws, {', '.join(map(str, low.shape))}], got {noise.shape}")
    null = np.zeros_like(low)
    x = noise[0]
    inter, preds = [], []
    for i, (t, coef) in enumerate(zip(ts, coefs)):
        out = np.asarray(unet_fn(x, low, t), dtype=np.float32)
        if wv is not None and phi > 0:
            out = guide_rescale_array(out, np.asarray(unet_fn(x, null, t), dtype=np.float32), wv, phi)
        elif wv is not None:
            out = guide_array(out, np.asarray(unet_fn(x, null, t), dtype=np.float32), wv)
        draw = None
        if not _coef_fields(coef)[4] and not _coef_fields(coef)[7]:
            if i + 1 >= noise.shape[0]:
                raise ValueError(f"step {i} is a non-final LCM step and needs noise[{i + 1}]; noise has {noise.shape[0]} draws")
            draw = noise[i + 1]
        x = scheduler_step_array(out, x, draw, coef)
        preds.append(out)
        inter.append(x)
    return dict(enhanced=np.clip(x, np.float32(-1), np.float32(1)), intermediate=inter, noise_pred=preds, timesteps=ts)


# ---------------------------------------------------------------------- the kernels on device tensors
def _device_rows(tensors, who: str):
    import torch
    first = tensors[0]
    if first.device.type != "cuda":
        raise RuntimeError(f"{who} runs only on a HIP device (got '{first.device}'); there is no CPU fallback")
    for t in tensors:
        if t.dtype != torch.float32 or not t.is_contiguous() or t.device != first.device or t.dim() < 2:
            raise ValueError(f"{who}: contiguous fp32 [B, ...] tensors on one device")
    b = int(first.shape[0])
    return b, first.numel() // max(b, 1), first.device


def guide_device(out_cond, out_uncond, w, out=None):
    """llie_guide on contiguous fp32 device tensors [B, ...] of one shape: `w` a finite host scalar or a device fp32 [B] tensor;
    `out` (default: a new tensor) may be `out_cond`.  One launch, no synchronisation."""
    import torch
    from . import _native as N
    b, per, dev = _device_rows((out_cond, out_uncond), "guide")
    if out_uncond.shape != out_cond.shape:
        raise ValueError(f"out_cond and out_uncond must have one shape, got {tuple(out_cond.shape)} and {tuple(out_uncond.shape)}")
    if out is None:
        out = torch.empty_like(out_cond)
    elif out.shape != out_cond.shape or _device_rows((out,), "guide")[2] != dev:
        raise ValueError("guide: out must be shaped like out_cond, on its device")
    if isinstance(w, torch.Tensor):
        if w.dtype != torch.float32 or tuple(w.shape) != (b,) or w.device != dev or not w.is_contiguous():
            raise ValueError(f"a per-row w must be a contiguous fp32 [{b}] tensor on the outputs' device")
        w_rows, ws = w.data_ptr(), 0.0
    else:
        ws = check_guidance_scale(w)
        if ws is None:
            raise ValueError("guide: w must be a finite number or a device tensor")
        w_rows = None
    with torch.cuda.device(dev):
        N.check(N.lib().llie_guide(out_cond.data_ptr(), out_uncond.data_ptr(), w_rows, ws, out.data_ptr(), b, per,
                                   torch.cuda.current_stream(dev).cuda_stream), "guide")
    return out


_rescale_scratch: Dict[tuple, object] = {}  # (device type, index) -> the scratch tensor of guide_rescale_device, grown on demand


def guide_rescale_scratch(batch: int, per_sample: int, device):
    """A uint8 device tensor of llie_guide_rescale_scratch_bytes(batch, per_sample) bytes or more, kept and reused per device
    (launches on one stream use it in turn).  ValueError for a shape the kernel refuses."""
    import torch
    from . import _native as N
    need = int(N.lib().llie_guide_rescale_scratch_bytes(int(batch), int(per_sample)))
    if need < 0:
        raise ValueError(f"guide_rescale: batch {batch} x per_sample {per_sample} is outside the kernel's contract")
    key = (device.type, device.index)
    buf = _rescale_scratch.get(key)
    if buf is None or buf.numel() < need:
        buf = _rescale_scratch[key] = torch.empty(need, dtype=torch.uint8, device=device)
    return buf


def guide_rescale_device(out_cond, out_uncond, w, phi, out=None, factor=None):
    """llie_guide_rescale on contiguous fp32 device tensors [B, ...] of one shape: `w` as in `guide_device`, `phi` in [0, 1];
    `out` (default: a new tensor) may be `out_cond` or `out_uncond`; `factor` (optional) a contiguous fp32 [B] device tensor that
    receives f_b.  The scratch tensor is the module's, reused from call to call.  At most three launches, no synchronisation."""
    import torch
    from . import _native as N
    pv = check_guidance_rescale(phi)
    b, per, dev = _device_rows((out_cond, out_uncond), "guide_rescale")
    if out_uncond.shape != out_cond.shape:
        raise ValueError(f"out_cond and out_uncond must have one shape, got {tuple(out_cond.shape)} and {tuple(out_uncond.shape)}")
    if out is None:
        out = torch.empty_like(out_cond)
    elif out.shape != out_cond.shape or _device_rows((out,), "guide_rescale")[2] != dev:
        raise ValueError("guide_rescale: out must be shaped like out_cond, on its device")
    if factor is not None and (factor.dtype != torch.float32 or tuple(factor.shape) != (b,) or factor.device != dev
                               or not factor.is_contiguous()):
        raise ValueError(f"factor must be a contiguous fp32 [{b}] tensor on the outputs' device")
    if isinstance(w, torch.Tensor):
        if w.dtype != torch.float32 or tuple(w.shape) != (b,) or w.device != dev or not w.is_contiguous():
            raise ValueError(f"a per-row w must be a contiguous fp32 [{b}] tensor on the outputs' device")
        w_rows, ws = w.data_ptr(), 0.0
    else:
        ws = check_guidance_scale(w)
        if ws is None:
            raise ValueError("guide_rescale: w must be a finite number or a device tensor")
        w_rows = None
    scratch = guide_rescale_scratch(b, per, dev)
    with torch.cuda.device(dev):
        N.check(N.lib().llie_guide_rescale(out_cond.data_ptr(), out_uncond.data_ptr(), w_rows, ws, pv, out.data_ptr(),
                                           factor.data_ptr() if factor is not None else None, scratch.data_ptr(), scratch.numel(), b, per,
                                           torch.cuda.current_stream(dev).cuda_stream), "guide_rescale")
    return out


def guidance_pair_device(latents, cond, latents2=None, cond2=None):
    """llie_guidance_pair: (latents2, cond2) [2B, ...] of contiguous fp32 device tensors [B, ...]; the outputs (default: new
    tensors) must not overlap the inputs.  One launch, no synchronisation."""
    import torch
    from . import _native as N
    b, per, dev = _device_rows((latents, cond), "guidance_pair")
    if cond.shape != latents.shape:
        raise ValueError(f"latents and cond must have one shape, got {tuple(latents.shape)} and {tuple(cond.shape)}")
    shape2 = (2 * b,) + tuple(latents.shape[1:])
    if latents2 is None:
        latents2 = torch.empty(shape2, dtype=torch.float32, device=dev)
    if cond2 is None:
        cond2 = torch.empty(shape2, dtype=torch.float32, device=dev)
    _device_rows((latents2, cond2), "guidance_pair")
    if tuple(latents2.shape) != shape2 or tuple(cond2.shape) != shape2 or latents2.device != dev or cond2.device != dev:
        raise ValueError(f"guidance_pair: the outputs must be {list(shape2)} on the inputs' device")
    with torch.cuda.device(dev):
        N.check(N.lib().llie_guidance_pair(latents.data_ptr(), cond.data_ptr(), latents2.data_ptr(), cond2.data_ptr(), b, per,
                                           torch.cuda.current_stream(dev).cuda_stream), "guidance_pair")
    return latents2, cond2


def cond_dropout_device(cond, u, p, out=None):
    """llie_cond_dropout: rows of the contiguous fp32 device tensor `cond` [B, ...] with u[b] < p become the null condition; `u`
    a contiguous fp32 device [B]; `out` (default: a new tensor) may be `cond`.  One launch, no synchronisation."""
    import torch
    from . import _native as N
    pv = check_cond_dropout(p)
    b, per, dev = _device_rows((cond,), "cond_dropout")
    if u.dtype != torch.float32 or tuple(u.shape) != (b,) or u.device != dev or not u.is_contiguous():
        raise ValueError(f"u must be a contiguous fp32 [{b}] tensor on the condition's device")
    if out is None:
        out = torch.empty_like(cond)
    elif out.shape != cond.shape or _device_rows((out,), "cond_dropout")[2] != dev:
        raise ValueError("cond_dropout: out must be shaped like cond, on its device")
    with torch.cuda.device(dev):
        N.check(N.lib().llie_cond_dropout(cond.data_ptr(), u.data_ptr(), pv, out.data_ptr(), b, per,
                                          torch.cuda.current_stream(dev).cuda_stream), "cond_dropout")
    return out
