"""The optimiser side of the reference trainer's inner loop (src/training/trainer.py:281-324) on the HIP engine.

`FusedAdamW`  -- `torch.optim.AdamW` (trainer.py:163-168) whose `step()` also does what the trainer does around it:
                 `scaler.unscale_` / the 1 / world-size of the gradient average (`grad_scale`), `clip_grad_norm_(params,
                 gradient_clip)` (`max_grad_norm`, trainer.py:296-299,310-313) and `EMAModel.update` (`ema_decay`,
                 trainer.py:98-104) -- in three launches over all parameter tensors (llie_optimizer_step, csrc/optim.hip)
                 instead of ~40 launches and several milliseconds of host time on 321 tensors.  It is a
                 `torch.optim.Optimizer`: LR schedulers (`CosineAnnealingLR`, `OneCycleLR`, trainer.py:162-175) drive
                 `param_groups[0]["lr"]`, `state_dict()` has torch.optim.AdamW's layout (the trainer's checkpoint,
                 trainer.py:418-434).
`TrainStep`   -- `compute_loss -> backward -> gradient all-reduce -> clip -> AdamW -> EMA` without the autograd graph: the
                 engine's backward pass writes one flat gradient buffer and the optimiser reads it in place (no per-parameter
                 `.grad` views, no AccumulateGrad nodes).  Same numbers as the autograd path (tests/test_gpu_round4.py).
`FusedGradScaler` -- `torch.amp.GradScaler` for the fused step: its state (scale, growth tracker) lives on the device and the
                 optimiser's launches read and update it (llie_optimizer_step_amp), so `optimizer.step(grad_scaler=scaler)`
                 replaces `scaler.unscale_ -> clip_grad_norm_ -> scaler.step -> scaler.update -> ema.update` (the reference's
                 fp16 loop, trainer.py:285-322) with no host synchronisation.
`DistillStep` -- one step of consistency distillation (`LowLightLCMDistillation.consistency_distillation_loss -> backward ->
                 AdamW -> update_ema`) the same way: three denoiser passes, the distillation kernels and one flat gradient buffer.

Gradient accumulation: `TrainStep` and `DistillStep` also run as windows of micro-batches -- `accumulate` per micro-batch,
then `apply` (one optimiser step from acc = sum b_i g_i at grad_scale 1 / sum b_i) or `discard` -- see `_GradWindow`;
`grad_accumulate_array` is the NumPy definition of the kernel behind it (llie_grad_accumulate, csrc/optim.hip).

There is no CPU fallback: all three need the HIP library and parameters on a HIP device.
"""
import ctypes as C
from typing import Iterable, List, Optional

import torch
import torch.distributed as dist

from . import _native as N


class FusedGradScaler:
    """Dynamic loss scaling with torch.amp.GradScaler's semantics and checkpoint layout, for FusedAdamW / TrainStep /
    DistillStep.  The scale (fp32) and growth tracker (int32) are device scalars, created on first use on that device; the
    optimiser's step unscales, checks for inf / NaN, skips and updates them on the device (include/llie.h,
    llie_optimizer_step_amp).  `enabled=False` and several optimisers per scaler are not supported."""

    def __init__(self, init_scale: float = 2.0 ** 16, growth_factor: float = 2.0, backoff_factor: float = 0.5,
                 growth_interval: int = 2000):
        if not growth_factor > 1.0:
            raise ValueError("The growth factor must be > 1.0.")
        if not backoff_factor < 1.0:
            raise ValueError("The backoff factor must be < 1.0.")
        self._init_scale = init_scale
        self._growth_factor = growth_factor
        self._backoff_factor = backoff_factor
        self._growth_interval = growth_interval
        self._init_growth_tracker = 0
        self._scale: Optional[torch.Tensor] = None
        self._growth_tracker: Optional[torch.Tensor] = None

    def _device_scale(self, dev: torch.device) -> torch.Tensor:
        """The scale tensor on `dev`, created there on first use (as GradScaler._lazy_init_scale_growth_tracker: no sync)."""
        if self._scale is None:
            self._scale = torch.full((), self._init_scale, dtype=torch.float32, device=dev)
            self._growth_tracker = torch.full((), self._init_growth_tracker, dtype=torch.int32, device=dev)
        elif self._scale.device != dev:
            raise ValueError(f"FusedGradScaler: state lives on {self._scale.device}, used on {dev}")
        return self._scale

    def _native(self, dev: torch.device, step: torch.Tensor):
        scale = self._device_scale(dev)
        return (N.AmpState(scale.data_ptr(), self._growth_tracker.data_ptr(), step.data_ptr()),
                N.AmpConfig(float(self._growth_factor), float(self._backoff_factor), int(self._growth_interval)))

    def scale(self, outputs: torch.Tensor) -> torch.Tensor:
        """`outputs * scale` (for `scaler.scale(loss).backward()`), without a host synchronisation."""
        if not isinstance(outputs, torch.Tensor) or outputs.device.type != "cuda":
            raise ValueError("FusedGradScaler.scale: a tensor on a HIP device")
        return outputs * self._device_scale(outputs.device)

    def get_scale(self) -> float:
        """The current scale (synchronises: for logging)."""
        return self._init_scale if self._scale is None else self._scale.item()

    def get_growth_factor(self) -> float:
        return self._growth_factor

    def get_backoff_factor(self) -> float:
        return self._backoff_factor

    def get_growth_interval(self) -> int:
        return self._growth_interval

    def _get_growth_tracker(self) -> int:
        return self._init_growth_tracker if self._growth_tracker is None else int(self._growth_tracker.item())

    def state_dict(self) -> dict:
        """torch.amp.GradScaler.state_dict()'s layout (the trainer's "scaler_state_dict", trainer.py:431-432)."""
        return {"scale": self.get_scale(), "growth_factor": self._growth_factor, "backoff_factor": self._backoff_factor,
                "growth_interval": self._growth_interval, "_growth_tracker": self._get_growth_tracker()}

    def load_state_dict(self, state_dict: dict) -> None:
        if len(state_dict) == 0:
            raise RuntimeError("The source state dict is empty, possibly because it was saved from a disabled instance of GradScaler.")
        self._init_scale = float(state_dict["scale"])
        if self._scale is not None:
            self._scale.fill_(state_dict["scale"])
        self._growth_factor = float(state_dict["growth_factor"])
        self._backoff_factor = float(state_dict["backoff_factor"])
        self._growth_interval = int(state_dict["growth_interval"])
        self._init_growth_tracker = int(state_dict["_growth_tracker"])
        if self._growth_tracker is not None:
            self._growth_tracker.fill_(state_dict["_growth_tracker"])


class FusedAdamW(torch.optim.Optimizer):
    def __init__(self, params: Iterable[torch.nn.Parameter], lr: float = 1e-3, betas=(0.9, 0.999), eps: float = 1e-8,
                 weight_decay: float = 1e-2, *, max_grad_norm: Optional[float] = None, ema_decay: Optional[float] = None,
                 skip_nonfinite: bool = False):
        if lr < 0 or eps < 0 or weight_decay < 0 or not (0 <= betas[0] < 1) or not (0 <= betas[1] < 1):
            raise ValueError("FusedAdamW: lr, eps, weight_decay >= 0 and 0 <= beta < 1 (torch.optim.AdamW's checks)")
        if ema_decay is not None and not (0 <= ema_decay <= 1):
            raise ValueError("ema_decay must be in [0, 1]")
        super().__init__(params, dict(lr=lr, betas=tuple(betas), eps=eps, weight_decay=weight_decay))
        if len(self.param_groups) != 1:
            raise ValueError("FusedAdamW takes one parameter group (the reference trainer's model.parameters(), trainer.py:164)")
        ps = self.param_groups[0]["params"]
        if not ps:
            raise ValueError("no parameters")
        dev = ps[0].device
        for p in ps:
            if p.device != dev or p.dtype != torch.float32 or not p.is_contiguous():
                raise ValueError("FusedAdamW: fp32 contiguous parameters on one device (the engine's masters)")
        if dev.type != "cuda":
            raise RuntimeError("FusedAdamW runs only on a HIP device; there is no CPU fallback")
        self.max_grad_norm = max_grad_norm
        self.ema_decay = ema_decay
        self.skip_nonfinite = skip_nonfinite
        self._dev = dev
        self._numel = [p.numel() for p in ps]
        total = sum(self._numel)
        self._m = torch.zeros(total, dtype=torch.float32, device=dev)
        self._v = torch.zeros(total, dtype=torch.float32, device=dev)
        self._ema = torch.cat([p.detach().reshape(-1) for p in ps]) if ema_decay is not None else None  # EMAModel.__init__: a clone
        self._stats = torch.zeros(3, dtype=torch.float32, device=dev)
        self._step = 0
        self._dstep = None    # device int32 AdamW step count, from the first step with a grad_scaler on
        self._native = None   # llie_optimizer*
        self._layout = None   # (param pointers, gradient offsets) the native tables were built for
        o = 0
        for p, n in zip(ps, self._numel):
            self.state[p] = {"step": torch.tensor(0.0), "exp_avg": self._m[o:o + n].view_as(p), "exp_avg_sq": self._v[o:o + n].view_as(p)}
            o += n

    # ------------------------------------------------------------------ native tables
    def _bind(self, offsets: List[int]) -> None:
        ps = self.param_groups[0]["params"]
        layout = (tuple(p.data_ptr() for p in ps), tuple(offsets))
        if self._native is not None and layout == self._layout:
            return
        self._release()
        arr = (N.OptTensor * len(ps))()
        o = 0
        for i, (p, n) in enumerate(zip(ps, self._numel)):
            e = self._ema.data_ptr() + 4 * o if self._ema is not None else None
            arr[i] = N.OptTensor(p.data_ptr(), self._m.data_ptr() + 4 * o, self._v.data_ptr() + 4 * o, e, offsets[i], n)
            o += n
        out = C.c_void_p()
        with torch.cuda.device(self._dev):
            N.check(N.lib().llie_optimizer_create(arr, len(ps), C.byref(out)), "FusedAdamW")
        self._native, self._layout = out, layout

    def _release(self) -> None:
        if getattr(self, "_native", None) is not None:
            torch.cuda.synchronize(self._dev)  # a step reading the tables may still be in flight
            N.lib().llie_optimizer_destroy(self._native)
            self._native = None

    def __del__(self):
        try:
            self._release()
        except Exception:
            pass

    # ------------------------------------------------------------------ the step
    def _launch(self, grad_base: int, grad_scale: float, grad_scaler: Optional[FusedGradScaler] = None) -> None:
        g = self.param_groups[0]
        if grad_scaler is None and self._dstep is not None:
            raise ValueError("FusedAdamW: this optimiser has taken steps with a grad_scaler (its step count lives on the "
                             "device); every later step needs one too")
        if grad_scaler is not None and not isinstance(grad_scaler, FusedGradScaler):
            raise ValueError("grad_scaler must be a FusedGradScaler")
        if grad_scaler is None:
            self._step += 1
        h = N.OptHyper(float(g["lr"]), float(g["betas"][0]), float(g["betas"][1]), float(g["eps"]), float(g["weight_decay"]),
                       float(self.max_grad_norm) if self.max_grad_norm else 0.0,
                       float(self.ema_decay) if self.ema_decay is not None else -1.0, float(grad_scale), self._step,
                       1 if self.skip_nonfinite else 0)
        with torch.cuda.device(self._dev):
            stream = torch.cuda.current_stream(self._dev).cuda_stream
            if grad_scaler is None:
                N.check(N.lib().llie_optimizer_step(self._native, grad_base, C.byref(h), self._stats.data_ptr(), stream),
                        "FusedAdamW.step")
                return
            if self._dstep is None:  # seeded from the host count (torch.full: a fill kernel, no copy, no sync)
                self._dstep = torch.full((), self._step, dtype=torch.int32, device=self._dev)
            state, cfg = grad_scaler._native(self._dev, self._dstep)
            N.check(N.lib().llie_optimizer_step_amp(self._native, grad_base, C.byref(h), C.byref(state), C.byref(cfg),
                                                    self._stats.data_ptr(), stream), "FusedAdamW.step (grad_scaler)")

    @torch.no_grad()
    def step_flat(self, flat: torch.Tensor, offsets: List[int], grad_scale: float = 1.0, *,
                  grad_scaler: Optional[FusedGradScaler] = None) -> torch.Tensor:
        """One update from a flat fp32 gradient buffer (parameter i at `flat[offsets[i]:]`, e.g. what llie_unet_backward
        writes).  Returns the gradient norm before clipping as a device scalar (what clip_grad_norm_ returns).
        With `grad_scaler` the gradients are the scaled ones (backward of `grad_scaler.scale(loss)`), and this one call is
        `scaler.unscale_ -> clip_grad_norm_ -> scaler.step -> scaler.update -> EMA update`: a step with an inf / NaN gradient
        leaves parameters, moments and the step count alone (the EMA shadows still move) and backs the scale off."""
        if flat.dtype != torch.float32 or not flat.is_contiguous() or flat.device != self._dev:
            raise ValueError("flat gradients: contiguous fp32 on the parameters' device")
        if len(offsets) != len(self._numel) or any(o < 0 or o + n > flat.numel() for o, n in zip(offsets, self._numel)):
            raise ValueError("gradient offsets do not fit the flat buffer")
        self._bind(list(offsets))
        self._launch(flat.data_ptr(), grad_scale, grad_scaler)
        return self._stats[0]

    @torch.no_grad()
    def step(self, closure=None, *, grad_scale: float = 1.0, grad_scaler: Optional[FusedGradScaler] = None):
        """`clip_grad_norm_` (if max_grad_norm) + `AdamW.step` + EMA update (if ema_decay) on the `.grad` of every parameter.
        Every parameter must have a gradient (the engine's backward pass always writes all of them).  `grad_scaler`: as
        step_flat's."""
        loss = None
        if closure is not None:
            with torch.enable_grad():
                loss = closure()
        ps = self.param_groups[0]["params"]
        grads = []
        for p in ps:
            g = p.grad
            if g is None:
                raise RuntimeError("FusedAdamW.step: a parameter has no gradient")
            if g.dtype != torch.float32 or not g.is_contiguous() or g.device != self._dev:
                g = g.to(device=self._dev, dtype=torch.float32).contiguous()
            grads.append(g)
        ptrs = [g.data_ptr() for g in grads]
        base = min(ptrs)
        # offsets relative to the lowest gradient: with the engine's backward pass these are the views of one flat buffer
        # and never change; gradients from elsewhere just rebuild the tables when their relative placement moves
        self._bind([(q - base) // 4 for q in ptrs])
        self._launch(base, grad_scale, grad_scaler)
        self._keep = grads  # alive until the next step's launch is queued behind this one
        return loss

    def grad_norm(self) -> torch.Tensor:
        """Norm of the gradients of the last step times grad_scale (unscaled by the grad_scaler's scale), before clipping:
        device scalar."""
        return self._stats[0]

    def last_step_skipped(self) -> bool:
        return bool(self._stats[2].item())

    # ------------------------------------------------------------------ EMA (trainer.py:86-118)
    def ema_tensors(self) -> List[torch.Tensor]:
        """Shadow weights as views shaped like the parameters, in parameter order."""
        if self._ema is None:
            raise RuntimeError("constructed without ema_decay")
        out, o = [], 0
        for p, n in zip(self.param_groups[0]["params"], self._numel):
            out.append(self._ema[o:o + n].view_as(p))
            o += n
        return out

    # ------------------------------------------------------------------ checkpoint layout of torch.optim.AdamW
    def state_dict(self):
        if self._dstep is not None:  # updates actually taken (synchronises: checkpoints only)
            self._step = int(self._dstep.item())
        for st in self.state.values():
            st["step"] = torch.tensor(float(self._step))
        sd = super().state_dict()
        if self._ema is not None:
            sd["ema_shadow_flat"] = self._ema.clone()
        return sd

    def load_state_dict(self, state_dict) -> None:
        sd = dict(state_dict)
        ema = sd.pop("ema_shadow_flat", None)
        super().load_state_dict(sd)
        ps = self.param_groups[0]["params"]
        o, step = 0, 0
        for p, n in zip(ps, self._numel):
            st = self.state.get(p, {})
            if "exp_avg" in st:
                self._m[o:o + n].copy_(st["exp_avg"].reshape(-1))
                self._v[o:o + n].copy_(st["exp_avg_sq"].reshape(-1))
                step = max(step, int(float(st.get("step", 0))))
            self.state[p] = {"step": torch.tensor(float(step)), "exp_avg": self._m[o:o + n].view_as(p), "exp_avg_sq": self._v[o:o + n].view_as(p)}
            o += n
        self._step = step
        if self._dstep is not None:
            self._dstep.fill_(step)
        if ema is not None and self._ema is not None:
            self._ema.copy_(ema.to(self._dev))


def _engine_order(unet, optimizer: FusedAdamW, who: str) -> List[int]:
    """Engine (llie_param_info) index of each of the optimiser's parameters; they must be exactly `unet`'s."""
    index = {id(p): i for i, (_, p) in enumerate(unet._ordered_params())}
    have = optimizer.param_groups[0]["params"]
    if len(index) != len(have) or any(id(p) not in index for p in have):
        raise ValueError(f"{who}: the optimiser must hold exactly model.unet's parameters (FusedAdamW(model.parameters(), ...))")
    return [index[id(p)] for p in have]


def _train_buffers(step, h: N.Handle, batch: int, dev: torch.device, height: int = 0, width: int = 0) -> int:
    """Grow `step._ws` (train workspace; it never shrinks) and allocate `step._flat` (flat gradients) / `step._offsets` (the
    optimiser's order) for handle `h`; returns the workspace bytes the engine needs at `height` x `width` (0, 0: image_size;
    ValueError naming the rule when llie_train_shape_ok refuses the shape)."""
    nbytes = h.train_plan(batch, height, width) if height else h.train_workspace_bytes(batch)
    if step._ws is None or step._ws.numel() < nbytes or step._ws.device != dev:
        step._ws = torch.empty(nbytes, dtype=torch.uint8, device=dev)
    if step._flat is None or step._flat.numel() != h.grad_numel() or step._flat.device != dev:
        step._flat = torch.empty(h.grad_numel(), dtype=torch.float32, device=dev)
        offs = h.grad_offsets()
        step._offsets = [offs[i] for i in step._order]
    return nbytes


def grad_accumulate_array(acc, grad, weight, first):
    """NumPy definition of llie_grad_accumulate (bit-equal to the kernel): `weight * grad` when `first`, else
    `acc + weight * grad`, in fp32 with the product and the sum rounded separately.  With `first`, `acc` is not read.
    Returns a new fp32 array; inf / NaN follow IEEE arithmetic."""
    import numpy as np
    w = np.float32(weight)
    if not np.isfinite(w) or not w > 0:
        raise ValueError("grad_accumulate_array: the weight must be finite and > 0")
    g = np.asarray(grad, dtype=np.float32)
    with np.errstate(invalid="ignore", over="ignore"):
        prod = np.multiply(w, g, dtype=np.float32)
        if first:
            return prod
        a = np.asarray(acc, dtype=np.float32)
        if a.shape != g.shape:
            raise ValueError("grad_accumulate_array: acc and grad must have one shape")
        return np.add(a, prod, dtype=np.float32)


def accumulation_windows(n: int, k: int) -> List[int]:
    """Lengths of the windows that n loader batches form at `accumulate=k`: k consecutive batches each, the last one the
    remaining n mod k when that is not 0.  They sum to n; there are ceil(n / k) of them."""
    n, k = int(n), int(k)
    if n < 0 or k < 1:
        raise ValueError(f"accumulation_windows: n >= 0 and k >= 1, got n={n}, k={k}")
    return [k] * (n // k) + ([n % k] if n % k else [])


class _GradWindow:
    """Gradient accumulation shared by TrainStep and DistillStep (both provide `_flat`, `_offsets`, `opt`, `grad_scaler`).

    A window is a sequence of micro-batches i = 1..k of b_i images (their shapes may differ where the step allows it).
    `accumulate` leaves g_i, the gradient of micro-batch i's own mean loss, in the flat buffer and the window keeps
        acc = sum_i b_i * g_i          (llie_grad_accumulate: fp32, product and sum rounded separately, in micro-batch order)
    in a second flat fp32 buffer, allocated on the first `accumulate`.  `apply` takes one optimiser step,
        step_flat(acc, offsets, grad_scale = 1 / (world * sum_i b_i)),
    the gradient of the mean over the window's images of each image's own mean loss (for equal shapes: the loss of the
    concatenated batch), so nobody needs to know sum b in advance.  The window loss is formed from device scalars, without a
    host read, as
        num = float(b_1) * loss_1;  num = num + float(b_i) * loss_i (i = 2..k);  loss = num / float(sum b_i)      (fp32)
    With a FusedGradScaler the scale only moves inside `apply`, so it is constant across a window; a non-finite micro-batch
    makes `acc` non-finite, and the step is then skipped and the scale backed off exactly as for a single step.
    `__call__` raises RuntimeError while a window is open; `apply` raises RuntimeError on an empty window; `discard` closes a
    window without stepping."""

    _acc: Optional[torch.Tensor] = None
    _win_images = 0
    _win_loss: Optional[torch.Tensor] = None

    @property
    def window_images(self) -> int:
        """sum b of the open window (0: no window is open)."""
        return self._win_images

    def _no_open_window(self, who: str) -> None:
        if self._win_images:
            raise RuntimeError(f"{who}: a gradient-accumulation window is open ({self._win_images} images); apply() or discard() it first")

    def _window_add(self, b: int, loss: torch.Tensor) -> None:
        """acc (+)= b * flat; window loss numerator (+)= b * loss."""
        flat = self._flat
        first = self._win_images == 0
        if self._acc is None or self._acc.numel() != flat.numel() or self._acc.device != flat.device:
            if not first:
                raise RuntimeError("the flat gradient buffer changed inside an open window")
            self._acc = torch.empty_like(flat)
        dev = flat.device
        with torch.cuda.device(dev):
            N.check(N.lib().llie_grad_accumulate(self._acc.data_ptr(), flat.data_ptr(), flat.numel(), float(b), 1 if first else 0,
                                                 torch.cuda.current_stream(dev).cuda_stream), "accumulate")
        term = loss * float(b)
        self._win_loss = term if first else self._win_loss + term
        self._win_images += b

    @torch.no_grad()
    def _window_apply(self, group=None, reduce: bool = True) -> torch.Tensor:
        if not self._win_images:
            raise RuntimeError("apply: no micro-batch has been accumulated")
        world = 1
        if reduce and dist.is_available() and dist.is_initialized() and dist.get_world_size(group) > 1:
            dist.all_reduce(self._acc, group=group)  # the window's only collective; the average rides on grad_scale
            world = dist.get_world_size(group)
        total = self._win_images
        loss = self._win_loss / float(total)
        self._win_images, self._win_loss = 0, None
        self.opt.step_flat(self._acc, self._offsets, grad_scale=1.0 / (world * total), grad_scaler=self.grad_scaler)
        return loss

    def discard(self) -> None:
        """Close the window without stepping (the accumulator's content is dropped: the next `accumulate` overwrites it)."""
        self._win_images, self._win_loss = 0, None


class TrainStep(_GradWindow):
    """One optimisation step of the reference trainer (trainer.py:281-324) on the engine, without autograd:
    q-sample (low_light_diffusion.py:140-160) -> llie_unet_train_forward -> loss and d(loss)/d(eps) -> llie_unet_backward into a
    persistent flat buffer -> one all-reduce of that buffer over the ranks -> FusedAdamW.step_flat (clip, AdamW, EMA).
    `loss_type` / `use_velocity_target` as LowLightDiffusion.compute_loss.  With `grad_scaler` (a FusedGradScaler: fp16 engines
    need one, their unscaled gradients underflow) d(loss)/d(eps) is multiplied by the device scale before the backward pass,
    which is `scaler.scale(loss).backward()`, and the optimiser unscales, skips and updates the scale on the device.
    `x0_ssim_weight` / `x0_l1_weight` (>= 0): when either is non-zero, the x0 term of pipeline.py (SSIM / L1 of the predicted
    clean image against `normal_light`) is added to the loss, and one call of llie_x0_loss adds its gradient into d(loss)/d(eps)
    before the grad-scaler multiplication; with both 0 the step makes no such call and is unchanged bit for bit.
    `cond_grad=True`: every call also leaves `step.cond_grad`, fp32 [B,3,H,W]: the gradient of the returned (unscaled) loss with
    respect to `low_light`, from the same backward call (llie_unet_backward_dx), for a trainable module in front of the denoiser:
    `low = frontend(raw); loss = step(low.detach(), normal); low.backward(step.cond_grad)`.  With a `grad_scaler` it is divided by
    the device scale (one elementwise operation, no host read) before the optimiser updates that scale; on a step the scaler
    skips, its values may be non-finite.  Only the condition half is exposed: with the x0 term on, x_t also enters the loss
    directly.  It is this rank's gradient (never all-reduced).  With `cond_grad=False` the step is what it was, bit for bit.
    Returns the loss (device scalar, unscaled).
    Gradient accumulation: `accumulate(...)` per micro-batch, then `apply()` (or `discard()`), see _GradWindow; `__call__` is
    one step from one batch as before and raises RuntimeError while a window is open.
    `cond_dropout=p` in [0, 1] (classifier-free guidance training; guidance.py has the definitions): with p > 0, row b of the
    condition is replaced by the null condition (all zeros) where u[b] < p -- llie_cond_dropout into a persistent buffer of the
    step, before the train forward.  u is `cond_u` (fp32 [B], supplied like `timesteps=` and `noise=`) or `torch.rand(b,
    device=dev)` from the global device generator, drawn after the timestep and noise draws.  `step.cond_grad` goes through the
    same kernel: dropped rows are exactly 0.  With p == 0 no draw is made and the step is what it was, bit for bit.
    `snr_gamma=g` (finite, > 0; None = off): Min-SNR-gamma weighting of the noise-space loss (snrloss.py has the definition).
    One call of llie_snr_loss replaces the torch arithmetic between the forward and the backward pass: it returns
    (1 / B) sum_b w_b m_b, with w_b from `use_velocity_target`, and stores d(loss)/d(eps) into a buffer of the step; the x0 term
    then adds into that buffer exactly as without the flag (its own abar weight unchanged, not multiplied by w), and the
    grad-scaler multiplication, `cond_grad`, `cond_dropout` and `accumulate` / `apply` follow unchanged.  After each call
    `step.sample_loss` (the unweighted per-sample means m_b) and `step.snr_weight` (w_b), fp32 [B] on the device, hold the last
    micro-batch's values; nothing reads them on the host.  With None the step is what it was, bit for bit."""

    def __init__(self, model, optimizer: FusedAdamW, loss_type: str = "mse", use_velocity_target: bool = False, group=None,
                 grad_scaler: Optional[FusedGradScaler] = None, x0_ssim_weight: float = 0.0, x0_l1_weight: float = 0.0,
                 cond_grad: bool = False, cond_dropout: float = 0.0, snr_gamma: Optional[float] = None):
        from .guidance import check_cond_dropout
        from .snrloss import check_snr_gamma
        from .pipeline import _check_x0_weights
        if loss_type not in ("mse", "huber", "l1"):
            raise ValueError(f"Unknown loss type: {loss_type}")
        if grad_scaler is not None and not isinstance(grad_scaler, FusedGradScaler):
            raise ValueError("grad_scaler must be a FusedGradScaler")
        _check_x0_weights(x0_ssim_weight, x0_l1_weight)
        self.snr_gamma = check_snr_gamma(snr_gamma)
        self.model, self.opt, self.loss_type, self.velocity, self.group = model, optimizer, loss_type, use_velocity_target, group
        self.grad_scaler = grad_scaler
        self.x0_ssim_weight, self.x0_l1_weight = float(x0_ssim_weight), float(x0_l1_weight)
        self._order = _engine_order(model.unet, optimizer, "TrainStep")
        if use_velocity_target and getattr(model.scheduler.config, "prediction_type", "epsilon") != "v_prediction":
            raise ValueError("use_velocity_target needs a scheduler with prediction_type='v_prediction'")
        self._flat = None
        self._ws = None
        self._want_cond_grad = bool(cond_grad)
        self.cond_grad: Optional[torch.Tensor] = None
        self.cond_dropout = check_cond_dropout(cond_dropout)
        self._cond = None  # the dropped-out condition (persistent; follows the batch's shape)
        self._d_eps = None  # d(loss)/d(eps) of the weighted loss (persistent; follows the batch's shape)
        self.sample_loss: Optional[torch.Tensor] = None
        self.snr_weight: Optional[torch.Tensor] = None

    @torch.no_grad()
    def __call__(self, low_light: torch.Tensor, normal_light: torch.Tensor, timesteps: Optional[torch.Tensor] = None,
                 noise: Optional[torch.Tensor] = None, cond_u: Optional[torch.Tensor] = None) -> torch.Tensor:
        self._no_open_window("TrainStep.__call__")
        loss = self._micro(low_light, normal_light, timesteps, noise, cond_u)
        scale = 1.0
        if dist.is_available() and dist.is_initialized() and dist.get_world_size(self.group) > 1:
            dist.all_reduce(self._flat, group=self.group)  # one collective over all gradients; the average rides on grad_scale
            scale = 1.0 / dist.get_world_size(self.group)
        self.opt.step_flat(self._flat, self._offsets, grad_scale=scale, grad_scaler=self.grad_scaler)
        return loss

    @torch.no_grad()
    def accumulate(self, low_light: torch.Tensor, normal_light: torch.Tensor, timesteps: Optional[torch.Tensor] = None,
                   noise: Optional[torch.Tensor] = None, cond_u: Optional[torch.Tensor] = None) -> torch.Tensor:
        """One micro-batch of a window: everything `__call__` does up to and including the backward pass into the flat buffer
        (at the batch's own H x W, which may differ from the window's other micro-batches), then `acc (+)= b * flat`
        (llie_grad_accumulate).  Returns the micro-batch loss (device scalar, unscaled); nothing reads from the host.  A shape
        llie_train_shape_ok refuses raises before the accumulator is touched and leaves an open window as it was."""
        if self._want_cond_grad:
            raise ValueError("TrainStep.accumulate: cond_grad=True is not supported in a window (the window's weight is not known "
                             "when a micro-batch's condition gradient is produced)")
        loss = self._micro(low_light, normal_light, timesteps, noise, cond_u)
        self._window_add(int(low_light.shape[0]), loss)
        return loss

    def apply(self) -> torch.Tensor:
        """Close the window with one optimiser step from `acc` (see _GradWindow) and return the window loss.  With a process
        group of more than one rank, `acc` is all-reduced first, the window's only collective, and the divisor is world * sum b:
        every rank must have accumulated the same sum b (not checked)."""
        return self._window_apply(self.group)

    def _micro(self, low_light: torch.Tensor, normal_light: torch.Tensor, timesteps: Optional[torch.Tensor],
               noise: Optional[torch.Tensor], cond_u: Optional[torch.Tensor] = None) -> torch.Tensor:
        """q-sample -> (condition dropout) -> train forward -> loss and d(loss)/d(eps) (x0 term, grad-scaler multiplication) ->
        backward into `self._flat`; returns the loss."""
        from .unet import resolve_compute_dtype
        model, unet = self.model, self.model.unet
        b, dev = low_light.shape[0], low_light.device
        if low_light.dim() != 4 or low_light.shape[1] != 3 or tuple(normal_light.shape) != tuple(low_light.shape):
            raise ValueError("low_light / normal_light must be [B,3,H,W] of one shape")
        hh, ww = int(low_light.shape[2]), int(low_light.shape[3])
        h = unet._handle(resolve_compute_dtype(unet.compute_dtype))
        # the batch's own H x W (llie_train_shape_ok); the workspace follows the shape and only grows, so a loop may alternate shapes
        nbytes = _train_buffers(self, h, b, dev, hh, ww)
        if timesteps is None:
            timesteps = torch.randint(0, model.scheduler.config.num_train_timesteps, (b,), device=dev)
        if noise is None:
            noise = torch.randn_like(normal_light)
        noisy = model.scheduler.add_noise(normal_light, noise, timesteps).float().contiguous()
        target = model.scheduler.get_velocity(normal_light, noise, timesteps) if self.velocity else noise
        cond = low_light.detach().float().contiguous()
        u = None
        if self.cond_dropout > 0:  # the third draw, after timesteps and noise; none at p == 0
            from .guidance import cond_dropout_device
            from .pipeline import cond_uniforms
            u = cond_uniforms(cond_u, b, dev)
            if self._cond is None or self._cond.shape != cond.shape or self._cond.device != dev:
                self._cond = torch.empty_like(cond)
            cond = cond_dropout_device(cond, u, self.cond_dropout, out=self._cond)
        t = timesteps.to(device=dev, dtype=torch.long).contiguous()
        eps = torch.empty(b, unet.config.out_channels, hh, ww, dtype=torch.float32, device=dev)
        L = N.lib()
        with torch.cuda.device(dev):
            st = torch.cuda.current_stream(dev).cuda_stream
            h.unet_train_forward(noisy.data_ptr(), cond.data_ptr(), t.data_ptr(), eps.data_ptr(), b, hh, ww, self._ws.data_ptr(), nbytes, st)
            from .pipeline import base_loss_and_grad, x0_loss_device
            if self.snr_gamma is None:
                loss, d_eps = base_loss_and_grad(eps, target, self.loss_type)
            else:
                from .snrloss import snr_loss_device
                if self._d_eps is None or self._d_eps.shape != eps.shape or self._d_eps.device != dev:
                    self._d_eps = torch.empty_like(eps)
                d_eps = self._d_eps
                loss, self.sample_loss, self.snr_weight = snr_loss_device(model.scheduler, eps, target, t, self.loss_type, self.velocity,
                                                                          self.snr_gamma, d_eps)
            if self.x0_ssim_weight != 0.0 or self.x0_l1_weight != 0.0:
                d_eps = d_eps.contiguous()
                loss = loss + x0_loss_device(model.scheduler, eps, noisy, normal_light, t, self.velocity, self.x0_ssim_weight,
                                             self.x0_l1_weight, d_eps)  # adds d(term)/d(eps) into d_eps
            if self.grad_scaler is not None:
                d_eps = d_eps * self.grad_scaler._device_scale(dev)
            if self._want_cond_grad:
                dc = torch.empty_like(cond)
                N.check(L.llie_unet_backward_dx(h.h, d_eps.data_ptr(), self._flat.data_ptr(), None, dc.data_ptr(), b, self._ws.data_ptr(),
                                                nbytes, st), "EfficientUNet.backward")
                # unscaled here, before step_flat below updates the device scale
                self.cond_grad = dc / self.grad_scaler._device_scale(dev) if self.grad_scaler is not None else dc
                if u is not None:  # the gradient of the null condition's rows does not reach low_light: exactly 0
                    cond_dropout_device(self.cond_grad, u, self.cond_dropout, out=self.cond_grad)
            else:
                N.check(L.llie_unet_backward(h.h, d_eps.data_ptr(), self._flat.data_ptr(), b, self._ws.data_ptr(), nbytes, st),
                        "EfficientUNet.backward")
        return loss


class DistillStep(_GradWindow):
    """One optimisation step of consistency distillation (LowLightLCMDistillation, low_light_diffusion.py:325-393, then
    AdamW and update_ema) without autograd:
      draws (noise, idx) -> add_noise -> teacher forward at t -> llie_consistency_target (x_next) -> student
      llie_unet_train_forward at t -> EMA-target forward at t_next -> llie_consistency_loss (loss, d/d eps) ->
      llie_unet_backward into a flat buffer -> FusedAdamW.step_flat -> llie_ema_update.
    Same numbers as `loss = distill.consistency_distillation_loss(...); loss.backward(); optimizer.step();
    distill.update_ema(ema_decay)`.  The EMA student's engine weights are reloaded at its next forward (content check on the
    device).  Returns the loss (device scalar, unscaled).  fp16 students need a `grad_scaler` (FusedGradScaler: d(loss)/d(eps)
    times the device scale, unscale / skip / scale update in the optimiser's launches) and are refused without one; update_ema
    runs every step, skipped or not, as in the reference loop.  fp32 and bf16 run either way.
    Batches are [B,3,H,W] of any shape LowLightLCMDistillation accepts (its docstring has the rule); the networks' outputs are
    read with the distillation's `teacher_prediction` / `student_prediction`.
    With `LowLightLCMDistillation(guidance=True)` the teacher's output is the guided one (its docstring): the per-sample scales
    are the third draw, after `noise` and `idx`, or `w=` (fp32 [B]) of `__call__` / `accumulate`."""

    def __init__(self, distill, optimizer: FusedAdamW, ema_decay: float = 0.95, grad_scaler: Optional[FusedGradScaler] = None):
        if not (0 <= ema_decay <= 1):
            raise ValueError("ema_decay must be in [0, 1]")
        if grad_scaler is not None and not isinstance(grad_scaler, FusedGradScaler):
            raise ValueError("grad_scaler must be a FusedGradScaler")
        if grad_scaler is None and distill.student.compute_dtype in ("fp16", "float16", torch.float16):
            raise ValueError("DistillStep: fp16 students need loss scaling, which this step does not do; use the autograd "
                             "path (consistency_distillation_loss + GradScaler) or bf16")
        self.distill, self.opt, self.ema_decay, self.grad_scaler = distill, optimizer, ema_decay, grad_scaler
        self._order = _engine_order(distill.student.unet, optimizer, "DistillStep")
        self._flat = None
        self._ws = None

    @torch.no_grad()
    def __call__(self, low_light: torch.Tensor, normal_light: torch.Tensor, num_inference_steps: int = 4, *,
                 noise: Optional[torch.Tensor] = None, idx: Optional[torch.Tensor] = None,
                 w: Optional[torch.Tensor] = None) -> torch.Tensor:
        self._no_open_window("DistillStep.__call__")
        loss = self._micro(low_light, normal_light, num_inference_steps, noise, idx, w)
        self.opt.step_flat(self._flat, self._offsets, grad_scaler=self.grad_scaler)
        self.distill.update_ema(self.ema_decay)
        return loss

    @torch.no_grad()
    def accumulate(self, low_light: torch.Tensor, normal_light: torch.Tensor, num_inference_steps: int = 4, *,
                   noise: Optional[torch.Tensor] = None, idx: Optional[torch.Tensor] = None,
                   w: Optional[torch.Tensor] = None) -> torch.Tensor:
        """One micro-batch of a window (at the batch's own H x W, which may differ from the window's other micro-batches): the
        teacher, student and EMA-target forwards, the loss and the backward pass of `__call__`, then `acc (+)= b * flat`.
        Returns the micro-batch loss (device scalar).  A shape the engines refuse raises before any draw and leaves an open
        window as it was."""
        loss = self._micro(low_light, normal_light, num_inference_steps, noise, idx, w)
        self._window_add(int(low_light.shape[0]), loss)
        return loss

    def apply(self) -> torch.Tensor:
        """Close the window: one optimiser step from `acc` (see _GradWindow), then `update_ema` once.  Returns the window loss."""
        loss = self._window_apply(reduce=False)  # as __call__: this step has no gradient all-reduce
        self.distill.update_ema(self.ema_decay)
        return loss

    def _micro(self, low_light: torch.Tensor, normal_light: torch.Tensor, num_inference_steps: int, noise: Optional[torch.Tensor],
               idx: Optional[torch.Tensor], w: Optional[torch.Tensor] = None) -> torch.Tensor:
        """The three denoiser passes, the distillation kernels and the backward pass into `self._flat`; returns the loss."""
        from .pipeline import consistency_loss, consistency_target
        from .unet import resolve_compute_dtype
        d = self.distill
        d._check_inputs(low_light, normal_light)
        unet = d.student.unet
        dtype = resolve_compute_dtype(unet.compute_dtype)
        if dtype == N.LLIE_F16 and self.grad_scaler is None:
            raise ValueError("DistillStep: fp16 students need loss scaling, which this step does not do; use the autograd "
                             "path (consistency_distillation_loss + GradScaler) or bf16")
        b, dev = low_light.shape[0], low_light.device
        hh, ww = int(low_light.shape[2]), int(low_light.shape[3])
        noise, idx = d._draws(normal_light, num_inference_steps, noise, idx)
        w = d._draw_w(b, dev, w)  # None unless the distillation was built with guidance=True: then the third draw
        t, t_next = d.timestep_pairs(idx, num_inference_steps)
        sched = d.teacher.scheduler
        low = low_light.detach().float().contiguous()
        x_t = sched.add_noise(normal_light, noise, t)
        e_teacher = d.teacher_output(x_t, low, t, w)
        x_next = consistency_target(sched, x_t, e_teacher, t, t_next, prediction_type=d.teacher_prediction)
        h = unet._handle(dtype)
        # the batch's own H x W; the workspace follows the shape and only grows, so a loop or a window may alternate shapes
        nbytes = _train_buffers(self, h, b, dev, hh, ww)
        e_student = torch.empty(b, unet.config.out_channels, hh, ww, dtype=torch.float32, device=dev)
        L = N.lib()
        with torch.cuda.device(dev):
            h.unet_train_forward(x_t.data_ptr(), low.data_ptr(), t.data_ptr(), e_student.data_ptr(), b, hh, ww, self._ws.data_ptr(), nbytes,
                                 torch.cuda.current_stream(dev).cuda_stream)
        e_ema = d.ema_student.unet.forward_split(x_next, low, t_next, frame=True)
        loss, d_eps = consistency_loss(sched, x_t, x_next, e_student, e_ema, t, t_next, prediction_type=d.student_prediction)
        if self.grad_scaler is not None:
            d_eps = d_eps * self.grad_scaler._device_scale(dev)
        with torch.cuda.device(dev):
            N.check(L.llie_unet_backward(h.h, d_eps.data_ptr(), self._flat.data_ptr(), b, self._ws.data_ptr(), nbytes,
                                         torch.cuda.current_stream(dev).cuda_stream), "EfficientUNet.backward")
        return loss
