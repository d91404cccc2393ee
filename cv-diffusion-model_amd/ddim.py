"""The deterministic DDIM sampler (eta = 0) as a host definition: the grid, one step and the whole loop in float64 NumPy.

This is the sampler of a many-step (teacher) model -- a plain epsilon- or v-prediction denoiser -- where the LCM loop of
`enhance` (predict x0, re-noise with a fresh draw) is the sampler of a consistency student.  The step is the teacher's step of
the distillation loss (low_light_diffusion.py:365-379; `llie_consistency_target`) used as a sampler.  With abar the alpha-bar
table, alpha = sqrt(abar), sigma = sqrt(1 - abar), `out` the network output and x the current latents:

  epsilon prediction:  x0 = (x - sigma_t out) / alpha_t,   e = out
  v prediction:        x0 = alpha_t x - sigma_t out,       e = alpha_t out + sigma_t x
  non-final step:      x <- alpha_p x0 + sigma_p e         (p: the previous timestep)
  final step:          x <- x0;  enhanced = clip(x, -1, 1)

  timesteps of n steps over T = num_train_timesteps, c = T // n:  t_i = (n - 1 - i) c, i = 0 .. n-1; the previous timestep of t
  is t - c, and the step at t = 0 is the final one.  1 <= n <= T.

No noise is drawn after the initial latents.  The device runs the same operations in fp32, each multiply and add on its own
(lcm_step_kernel's DDIM branch, the fused output-head epilogue, tile_sync_step_kernel); these functions are what its tests compare
against.  Nothing here needs a GPU or the engine's library.
"""
from __future__ import annotations

from typing import Callable, Dict, List, Optional

import numpy as np

SAMPLERS = ("lcm", "ddim", "dpmpp_2m")  # "dpmpp_2m": the second-order sampler of dpm.py


def check_sampler(sampler: str) -> str:
    if sampler not in SAMPLERS:
        raise ValueError(f'sampler must be "lcm", "ddim" or "dpmpp_2m", got {sampler!r}')
    return sampler


def ddim_timesteps(n: int, num_train_timesteps: int = 1000) -> List[int]:
    """The grid of the module docstring: [(n-1) c, ..., c, 0] with c = num_train_timesteps // n."""
    if isinstance(n, bool) or int(n) != n:
        raise ValueError(f"the number of DDIM steps must be an integer, got {n!r}")
    n, t_max = int(n), int(num_train_timesteps)
    if not 1 <= n <= t_max:
        raise ValueError(f"the number of DDIM steps must lie in 1..{t_max}, got {n}")
    c = t_max // n
    return [(n - 1 - i) * c for i in range(n)]


def ddim_step_host(model_output, timestep: int, prev_timestep: int, sample, alphas_cumprod, velocity: bool = False) -> np.ndarray:
    """One step in float64: `model_output` and `sample` of one shape, `alphas_cumprod` the table (its fp32 values, widened) ->
    the next latents.  prev_timestep < 0 marks the final step (-> x0).  ValueError for a timestep outside the table, and for
    epsilon prediction at a timestep whose alpha-bar is 0 (x0 is undefined there)."""
    acp = np.asarray(alphas_cumprod, dtype=np.float64).reshape(-1)
    t, p = int(timestep), int(prev_timestep)
    if not 0 <= t < acp.shape[0] or p > t:
        raise ValueError(f"a DDIM step goes from a timestep in [0, {acp.shape[0]}) to one that is not later, got {t} -> {p}")
    out, x = np.asarray(model_output, dtype=np.float64), np.asarray(sample, dtype=np.float64)
    if out.shape != x.shape:
        raise ValueError(f"model_output and sample must have one shape, got {out.shape} and {x.shape}")
    a_t = acp[t]
    alpha_t, sigma_t = np.sqrt(a_t), np.sqrt(1.0 - a_t)
    if velocity:
        x0 = alpha_t * x - sigma_t * out
        e = alpha_t * out + sigma_t * x
    else:
        if a_t == 0:
            raise ValueError(f"alphas_cumprod[{t}] == 0: epsilon prediction defines no x0 at timestep {t}")
        x0 = (x - sigma_t * out) / alpha_t
        e = out
    if p < 0:
        return x0
    a_p = acp[p]
    return np.sqrt(a_p) * x0 + np.sqrt(1.0 - a_p) * e


def ddim_enhance_host(unet_fn: Callable, low, x_init, n: int, acp, velocity: bool = False) -> Dict[str, object]:
    """The loop of `enhance(sampler="ddim")` on the host, the denoiser passed in: unet_fn(latents fp32 [B,3,H,W], low fp32
    [B,3,H,W], t) -> the network output [B,3,H,W].  `x_init` are the initial latents, `acp` the alpha-bar table.  The network
    sees fp32 latents, as on the device; the steps between are float64.
    -> {"enhanced" (clamped), "intermediate" (the latents after each step, float64), "noise_pred" (fp32, per step), "timesteps"}."""
    acp = np.asarray(acp, dtype=np.float64).reshape(-1)
    ts = ddim_timesteps(n, acp.shape[0])
    if not velocity and acp[ts[0]] == 0:
        raise ValueError(f"alphas_cumprod[{ts[0]}] == 0: epsilon prediction cannot start at timestep {ts[0]}")
    low = np.ascontiguousarray(np.asarray(low, dtype=np.float32))
    x = np.asarray(x_init, dtype=np.float64)
    if x.shape != low.shape:
        raise ValueError(f"x_init must be shaped like low {low.shape}, got {x.shape}")
    c = acp.shape[0] // len(ts)
    inter, preds = [], []
    for t in ts:
        out = np.asarray(unet_fn(x.astype(np.float32), low, int(t)), dtype=np.float32)
        x = ddim_step_host(out, t, t - c, x, acp, velocity)
        preds.append(out)
        inter.append(x)
    return dict(enhanced=np.clip(x, -1.0, 1.0), intermediate=inter, noise_pred=preds, timesteps=ts)
