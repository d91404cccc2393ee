"""Min-SNR-gamma loss weighting (Hang et al., ICCV 2023) on the noise-space training loss: the definition in float64, the fp32
twin of csrc/snrloss.hip, the argument check and the device call.

The reference's objective is the flat mean of l(pred - target) over the batch: every timestep of U{0..999} counts the same,
although the scheduler's per-step SNR = abar / (1 - abar) runs from 0 (abar[999] = 0, the zero-terminal-SNR table) to over
1000.  With `snr_gamma` = gamma each sample's loss is weighted by

  epsilon prediction   w_b = min(SNR, gamma) / SNR        = 1 if abar == 0, otherwise min(1, (gamma (1 - abar)) / abar)
  v prediction         w_b = min(SNR, gamma) / (SNR + 1)  = min(abar, gamma (1 - abar))       (exactly 0 at abar == 0)

with abar = alphas_cumprod[t_b]; gamma = 5 is the paper's choice.  For pred / target [B, n] and d = pred - target:

  loss_type   l(d)                                       l'(d)
  mse         d^2                                        2 d
  l1          |d|                                        sign(d), sign(0) = 0 as torch.sign
  huber       0.5 d^2 where |d| < 1, else |d| - 0.5      clamp(d, -1, 1)                       (delta = 1)

  sample_loss[b] = m_b = (1 / n) sum_i l(d_bi)           unweighted, so it can be logged per timestep
  weight[b]      = w_b
  loss           = (1 / B) sum_b w_b m_b                 F.mse_loss / F.l1_loss / F.huber_loss when every w_b = 1
  d_pred[b, i]   = l'(d_bi) c_b,   c_b = (w_b / (float)B) / (float)n

The weights are not renormalised, timesteps stay uniform, and the x0 term (pipeline.py) keeps its own abar weight: it is not
multiplied by w.  `snr_loss_host` is the definition (float64 NumPy) the device is held to; `snr_loss_f32` runs the same formulas
in fp32 in the kernel's operation order -- the weight, c_b, d and l'(d) c_b one rounding each, no fused multiply-add -- so its
`weight` and `d_pred` are the device's bits, and the distance of its loss from the float64 one sizes the tests' tolerance.
llie_snr_loss (include/llie.h) is the device side: two launches, no atomics, bitwise reproducible.  Nothing here but
`snr_loss_device` needs a GPU or the engine's library.
"""
from __future__ import annotations

import math
from typing import Optional, Tuple

import numpy as np

LOSS_TYPES = ("mse", "l1", "huber")  # index = LLIE_LOSS_* (N.LOSS_MSE, N.LOSS_L1, N.LOSS_HUBER)


def check_snr_gamma(snr_gamma) -> Optional[float]:
    """`snr_gamma=` of the training entries: None (off) or a finite number > 0 -> None or its float.  ValueError otherwise."""
    if snr_gamma is None:
        return None
    if isinstance(snr_gamma, bool) or not isinstance(snr_gamma, (int, float, np.integer, np.floating)):
        raise ValueError(f"snr_gamma must be None or a finite number > 0, got {snr_gamma!r}")
    g = float(snr_gamma)
    if not math.isfinite(g) or not g > 0.0 or not math.isfinite(float(np.float32(g))) or not float(np.float32(g)) > 0.0:
        raise ValueError(f"snr_gamma must be None or a finite number > 0 (in fp32 too), got {snr_gamma!r}")
    return g


def _need_gamma(gamma) -> float:
    g = check_snr_gamma(gamma)
    if g is None:
        raise ValueError("snr_gamma must be a finite number > 0 here, got None")
    return g


def loss_code(loss_type: str) -> int:
    """"mse" / "l1" / "huber" -> LLIE_LOSS_*; ValueError for anything else (the message of compute_loss)."""
    if loss_type not in LOSS_TYPES:
        raise ValueError(f"Unknown loss type: {loss_type}")
    return LOSS_TYPES.index(loss_type)


def _weights(acp: np.ndarray, gamma, velocity: bool) -> np.ndarray:
    """w in the dtype of `acp`, each operation rounded in that dtype, in the kernel's order; NaN where acp is NaN."""
    t = acp.dtype.type
    g = (t(gamma) * (t(1) - acp)).astype(acp.dtype)
    with np.errstate(divide="ignore", invalid="ignore"):
        if velocity:
            return np.minimum(acp, g)
        r = (g / acp).astype(acp.dtype)
        return np.where(acp == 0, t(1), np.minimum(t(1), r)).astype(acp.dtype)


def snr_weight_array(acp_t, gamma, velocity: bool) -> np.ndarray:
    """The definition of w in float64 NumPy: acp_t [B] = alphas_cumprod[t_b] -> w [B] (module docstring)."""
    g = _need_gamma(gamma)
    return _weights(np.asarray(acp_t, dtype=np.float64).reshape(-1), g, bool(velocity))


def _eval(pred: np.ndarray, target: np.ndarray, acp: np.ndarray, loss_type: str, velocity: bool, gamma: float):
    """The formulas of the module docstring in the dtype of `pred`, one rounding per operation."""
    loss_code(loss_type)
    dt = pred.dtype
    t = dt.type
    b, n = pred.shape
    w = _weights(acp, gamma, velocity)
    with np.errstate(invalid="ignore", over="ignore"):
        d = (pred - target).astype(dt)
        z = np.abs(d)
        if loss_type == "mse":
            term, slope = (d * d).astype(dt), (t(2) * d).astype(dt)
        elif loss_type == "l1":
            term, slope = z, np.where(d > 0, t(1), np.where(d < 0, t(-1), d)).astype(dt)
        else:
            term = np.where(z < 1, ((t(0.5) * d).astype(dt) * d).astype(dt), (z - t(0.5)).astype(dt)).astype(dt)
            slope = np.where(d <= -1, t(-1), np.where(d >= 1, t(1), d)).astype(dt)
        m = term.mean(axis=1, dtype=dt)
        c = ((w / t(b)).astype(dt) / t(n)).astype(dt)
        grad = (slope * c[:, None]).astype(dt)
        loss = t((w * m).astype(dt).sum(dtype=dt) / t(b))
    return loss, m, w, grad


def _rows(pred, target, acp_t, dtype):
    p, y = np.asarray(pred, dtype=dtype), np.asarray(target, dtype=dtype)
    acp = np.asarray(acp_t, dtype=dtype).reshape(-1)
    if p.ndim < 2 or p.shape != y.shape or acp.shape[0] != p.shape[0] or p.size == 0:
        raise ValueError(f"pred / target must be [B, ...] of one non-empty shape and acp_t [B], got {p.shape}, {y.shape}, {acp.shape}")
    return p.reshape(p.shape[0], -1), y.reshape(p.shape[0], -1), acp, p.shape


def snr_loss_host(pred, target, acp_t, loss_type: str, velocity: bool, gamma) -> Tuple[float, np.ndarray, np.ndarray, np.ndarray]:
    """The definition in float64 NumPy: pred / target [B, ...], acp_t [B] = alphas_cumprod[t_b] ->
    (loss, sample_loss [B], weight [B], d(loss)/d(pred) shaped like pred)."""
    g = _need_gamma(gamma)
    p, y, acp, shape = _rows(pred, target, acp_t, np.float64)
    loss, m, w, grad = _eval(p, y, acp, loss_type, bool(velocity), g)
    return float(loss), m, w, grad.reshape(shape)


def snr_loss_f32(pred, target, acp_t, loss_type: str, velocity: bool, gamma) -> Tuple[np.float32, np.ndarray, np.ndarray, np.ndarray]:
    """The same formulas in NumPy float32 in the kernel's operation order: `weight` and `d_pred` are llie_snr_loss's bits; the
    loss and `sample_loss` differ from the device's in summation order only (NumPy adds pairwise in fp32, the device in fp32
    per workgroup and in double across workgroups)."""
    g = _need_gamma(gamma)
    p, y, acp, shape = _rows(pred, target, acp_t, np.float32)
    loss, m, w, grad = _eval(p, y, acp, loss_type, bool(velocity), np.float32(g))
    return np.float32(loss), m, w, grad.reshape(shape)


def snr_loss_chunk() -> int:
    """Elements of one sample that one workgroup of pass 1 covers (llie_snr_loss_chunk): a sample of n elements is
    ceil(n / chunk) partial sums."""
    from . import _native as N
    return int(N.lib().llie_snr_loss_chunk())


def snr_loss_device(scheduler, pred, target, timesteps, loss_type: str, velocity: bool, gamma, d_pred=None):
    """llie_snr_loss on device tensors: pred / target [B, ...] (fp32 contiguous is used as it is), timesteps [B] ->
    (loss 0-d, sample_loss [B], weight [B]), fp32 on the device.  `d_pred` (contiguous fp32, shaped like pred, on its device, not
    overlapping it) receives d(loss)/d(pred): stored, not accumulated.  `scheduler` supplies the alpha-bar table.  Host timesteps
    outside the table raise ValueError; device-resident ones cannot be checked without a synchronisation: the kernel turns one
    into a NaN weight, gradient and loss for that sample instead of indexing with it.  No synchronisation, no autograd."""
    import torch
    from . import _native as N
    from .pipeline import _require_hip
    _require_hip(pred, "snr_loss")
    g = _need_gamma(gamma)
    code = loss_code(loss_type)
    dev = pred.device
    if pred.dim() < 2 or pred.numel() == 0 or target.shape != pred.shape or tuple(timesteps.shape) != (pred.shape[0],):
        raise ValueError(f"pred / target must be [B, ...] of one non-empty shape and timesteps [B], got {tuple(pred.shape)}, "
                         f"{tuple(target.shape)}, {tuple(timesteps.shape)}")
    acp = scheduler._acp_on(dev)
    if timesteps.device.type == "cpu" and timesteps.numel() and (int(timesteps.min()) < 0 or int(timesteps.max()) >= acp.numel()):
        raise ValueError(f"timesteps must lie in [0, {acp.numel()})")
    pred, target = (v.detach().to(device=dev, dtype=torch.float32).contiguous() for v in (pred, target))
    t = timesteps.to(device=dev, dtype=torch.long).contiguous()
    if d_pred is not None and (d_pred.dtype != torch.float32 or not d_pred.is_contiguous() or d_pred.shape != pred.shape or d_pred.device != dev):
        raise ValueError("d_pred must be contiguous fp32, shaped like pred, on its device")
    b = int(pred.shape[0])
    per = pred.numel() // b
    L = N.lib()
    nbytes = int(L.llie_snr_loss_scratch_bytes(b, per))
    if nbytes < 0:
        N.check(nbytes, f"snr_loss: {b} samples of {per} elements")
    scratch = torch.empty((nbytes + 7) // 8, dtype=torch.float64, device=dev)
    out = torch.empty(1 + 2 * b, dtype=torch.float32, device=dev)  # loss, sample_loss, weight
    with torch.cuda.device(dev):
        N.check(L.llie_snr_loss(pred.data_ptr(), target.data_ptr(), t.data_ptr(), acp.data_ptr(), acp.numel(), code, 1 if velocity else 0,
                                g, out.data_ptr(), out.data_ptr() + 4, out.data_ptr() + 4 * (1 + b),
                                d_pred.data_ptr() if d_pred is not None else None, b, per, scratch.data_ptr(), nbytes,
                                torch.cuda.current_stream(dev).cuda_stream), "snr_loss")
    return out[0], out[1:1 + b], out[1 + b:]
