"""The loop that turns a teacher into a 4-8-step consistency student: LowLightTrainer's epochs (trainer.py: validation, checkpoints,
best model, sample sheets, accumulation windows, LR schedule -- the shared _EpochLoop) over DistillStep instead of TrainStep.

The reference has LowLightLCMDistillation (low_light_diffusion.py:284-408) and no loop around it; this is that loop, with the
trainer's file names and schedule, so the same scripts read what it writes.  `model_state_dict` of every checkpoint is the EMA
student's -- the network the loss trains towards and the one to deploy -- so `scripts/inference.py --checkpoint` runs it with no
conversion (`--prediction v_prediction` for a v student).
"""
from __future__ import annotations

from typing import Dict, Optional, Tuple

import torch

from . import _native as N
from . import hostio
from .guidance import check_guidance_range, check_guidance_scale, guided_keyword
from .metrics import evaluate
from .pipeline import LowLightDiffusion, LowLightLCMDistillation
from .trainer import TrainingConfig, _EpochLoop, distill_draw_seed, make_lr_scheduler, resolved_compute_dtype
from .training import DistillStep, FusedAdamW, FusedGradScaler, accumulation_windows

DISTILL_KEYS = ("num_ddim_timesteps", "num_inference_steps", "ema_decay", "teacher_prediction", "student_prediction", "skip_terminal")
DISTILL_CHECKPOINT_KEYS = ("epoch", "global_step", "model_state_dict", "student_state_dict", "optimizer_state_dict",
                           "scheduler_state_dict", "best_psnr", "config", "distill")


def timestep_index_range(num_ddim_timesteps: int, num_inference_steps: int, skip_terminal: bool) -> int:
    """`hi` of the distiller's `idx = randint(0, hi)`: n - k, or n - k - 1 with `skip_terminal` (k = n // num_inference_steps;
    idx = n - k - 1 is the one whose t_next is the last timestep, alpha-bar 0 on the zero-SNR table).  ValueError when no idx is
    left."""
    n, steps = int(num_ddim_timesteps), int(num_inference_steps)
    if steps < 1 or n < 1:
        raise ValueError(f"num_inference_steps and num_ddim_timesteps must be >= 1, got {steps} and {n}")
    k = n // steps
    hi = n - k - (1 if skip_terminal else 0)
    if k < 1 or hi < 1:
        raise ValueError(f"num_inference_steps={steps} leaves no timestep pair for num_ddim_timesteps={n}"
                         + (" with skip_terminal" if skip_terminal else ""))
    return hi


def default_skip_terminal(student_prediction: str) -> bool:
    """`skip_terminal=None`: True for an epsilon student, whose loss is +inf at the idx whose t_next has alpha-bar 0; False for a
    v_prediction student, whose loss is finite there."""
    from .pipeline import prediction_code
    return prediction_code(student_prediction, "student_prediction") == N.PRED_EPSILON


class LowLightDistiller(_EpochLoop):
    """LowLightTrainer's loop over DistillStep: `distill` is a LowLightLCMDistillation on a HIP device, the loaders are
    DevicePairLoaders on the same device; there is no CPU fallback.  Constructor arguments after `distill` are the trainer's
    (`config`: a TrainingConfig; `crop_size`, `accumulate`: as LowLightTrainer's, neither stored in checkpoints), plus

      num_inference_steps  the step count the student is distilled for (timestep_pairs' k); None: config.num_inference_steps.
                           Validation runs the EMA student with it, the sample sheet with 4 steps as the trainer's.
      ema_decay            of the target network (update_ema), after every optimiser step
      skip_terminal        leave out the idx whose t_next is the last timestep.  None: True for an epsilon student (alpha-bar is
                           0 there on the zero-SNR table and the epsilon form's loss is +inf), False for a v student (finite).

    Optimiser: FusedAdamW over the student with config.learning_rate / weight_decay / gradient_clip and NO optimiser EMA: the
    target network `distill.ema_student` is the only EMA, so `config.use_ema` / `config.ema_decay` are ignored.  The LR schedule
    is make_lr_scheduler over the epoch's accumulation windows; a FusedGradScaler exists only for fp16; teacher, student and EMA
    student all run in resolved_compute_dtype(config).  `config.loss_type` is not used (the loss is the Huber consistency loss).

    Draw recipe of `train_epoch` (part of the contract; the global generator is neither read nor advanced):
      train_loader.set_epoch(epoch); dev = the device; (H, W) = crop_size (config.image_size squared without one);
      hi = timestep_index_range(distill.num_ddim_timesteps, num_inference_steps, skip_terminal)
      g = torch.Generator(device=dev).manual_seed(distill_draw_seed(seed, epoch))       ((seed * 1000003 + epoch * 8191 + 76543) % (2^63 - 1))
      per batch of b pairs, in loader order, the reference's order of draws (low_light_diffusion.py:337-349: noise, then idx):
        noise = torch.randn(b, 3, H, W, generator=g, device=dev)
        idx = torch.randint(0, hi, (b,), generator=g, device=dev)
        u = torch.rand(b, generator=g, device=dev);  w = u * (w_hi - w_lo) + w_lo      only with distill.guidance: (w_lo, w_hi) =
                                                                                      distill.guidance_scale_range; two fp32 operations
        loss = step(low_light, normal_light, num_inference_steps, noise=noise, idx=idx[, w=w]);  lr_scheduler.step()
    With `accumulate=k` > 1 the draws are the same and `step(...)` becomes `step.accumulate(...)`, with `step.apply()` and
    `lr_scheduler.step()` after each window's last batch, as in the trainer.

    Checkpoints: the trainer's file names and schedule (checkpoint_epoch_{e}.pt, best_model.pt on a strictly higher validation
    PSNR, final_model.pt), read with weights_only=True.  Entries: DISTILL_CHECKPOINT_KEYS -- "model_state_dict" is the EMA
    student's state dict, "student_state_dict" the trained student's, "distill" = {num_ddim_timesteps, num_inference_steps,
    ema_decay, teacher_prediction, student_prediction, skip_terminal} -- plus "scaler_state_dict" where there is a scaler.
    The teacher is not stored.  `config.resume_from` continues bit for bit; a file whose "distill" entry disagrees with this
    constructor is a ValueError naming the field."""

    _what = "distillation"

    def __init__(self, distill: LowLightLCMDistillation, train_loader, val_loader=None, config: Optional[TrainingConfig] = None, *,
                 num_inference_steps: Optional[int] = None, ema_decay: float = 0.95, skip_terminal: Optional[bool] = None,
                 crop_size: Optional[Tuple[int, int]] = None, accumulate: int = 1, val_guidance_scale: Optional[float] = None):
        if not isinstance(distill, LowLightLCMDistillation):
            raise ValueError(f"distill is a LowLightLCMDistillation, got {type(distill).__name__}")
        self._init_shapes(config, train_loader, val_loader, crop_size, accumulate)
        cfg = self.config
        steps = cfg.num_inference_steps if num_inference_steps is None else num_inference_steps
        if isinstance(steps, bool) or int(steps) != steps or steps < 1:
            raise ValueError(f"num_inference_steps must be a positive integer or None, got {num_inference_steps!r}")
        self.num_inference_steps = int(steps)
        if not (0 <= ema_decay <= 1):
            raise ValueError(f"ema_decay must be in [0, 1], got {ema_decay!r}")
        self.ema_decay = float(ema_decay)
        self.val_guidance_scale = check_guidance_scale(val_guidance_scale)
        if skip_terminal is not None and not isinstance(skip_terminal, bool):
            raise ValueError(f"skip_terminal is True, False or None, got {skip_terminal!r}")
        self.skip_terminal = default_skip_terminal(distill.student_prediction) if skip_terminal is None else skip_terminal
        self.idx_range = timestep_index_range(distill.num_ddim_timesteps, self.num_inference_steps, self.skip_terminal)
        if int(distill.student.image_size) != int(cfg.image_size):
            raise ValueError(f"config.image_size is {cfg.image_size}, the student's {distill.student.image_size}")
        self._init_devices(distill.student, train_loader, val_loader)
        for what, m in (("the teacher", distill.teacher), ("the EMA student", distill.ema_student)):
            dev = next(m.parameters()).device
            if dev != self.device:
                raise ValueError(f"{what} is on {dev}, the student on {self.device}")
        dtype = resolved_compute_dtype(cfg)

        self.distill = distill
        for m in (distill.teacher, distill.student, distill.ema_student):
            m.compute_dtype = dtype
        if crop_size is not None:  # ValueError naming the rule, here and not at the first step
            b = max(1, int(getattr(train_loader, "batch_size", 1)))
            code = N.dtype_code(dtype)
            distill.student.unet._handle(code).train_shape_ok(b, *self.crop_size)
            for m in (distill.teacher, distill.ema_student):
                m.unet._handle(code).frame_shape_ok(b, *self.crop_size)
        self.train_loader = train_loader
        self.val_loader = val_loader

        self.optimizer = FusedAdamW(distill.student.parameters(), lr=cfg.learning_rate, weight_decay=cfg.weight_decay,
                                    max_grad_norm=cfg.gradient_clip)
        self.scheduler = make_lr_scheduler(self.optimizer, cfg, len(accumulation_windows(len(train_loader), accumulate)))
        self.scaler = FusedGradScaler() if dtype == "fp16" else None
        self.step = DistillStep(distill, self.optimizer, ema_decay=self.ema_decay, grad_scaler=self.scaler)

        self.best_psnr = float("-inf")
        self._init_run()

        if cfg.resume_from:
            self.load_checkpoint(cfg.resume_from)

    def _net(self) -> LowLightDiffusion:
        return self.distill.ema_student

    def _net_weights(self):
        return None  # the EMA student's own parameters

    # ------------------------------------------------------------------ epochs (`train`: _EpochLoop)
    def _epoch_log(self, epoch: int, train_loss: float):
        """Validate (when there is a val loader) -> (the epoch's log {"epoch", "train_loss", "lr", "psnr", "ssim"}, its progress
        line, whether it is the best so far: a strictly higher PSNR)."""
        psnr = self.validate() if self.val_loader is not None else None
        log = {"epoch": epoch, "train_loss": train_loss, "lr": self.optimizer.param_groups[0]["lr"], "psnr": psnr,
               "ssim": self.last_validation["ssim"] if psnr is not None else None}
        line = f"Epoch {epoch}: train_loss={train_loss:.4f}"
        if psnr is not None:
            line += f", psnr={psnr:.2f}, ssim={log['ssim']:.4f}"
        return log, line, psnr is not None and psnr > self.best_psnr

    def _set_best(self, log: Dict[str, object]) -> None:
        self.best_psnr = log["psnr"]

    def train_epoch(self) -> float:
        """One epoch of DistillStep over the train loader, with the draw recipe of the class docstring.  Returns the sum of the
        batch losses divided by len(train_loader), as LowLightTrainer.train_epoch."""
        cfg, dev, loader, steps, hi = self.config, self.device, self.train_loader, self.num_inference_steps, self.idx_range
        self.distill.student.train()
        loader.set_epoch(self.epoch)
        hh, ww = self.crop_size
        g = torch.Generator(device=dev).manual_seed(distill_draw_seed(cfg.seed, self.epoch))

        def micro(batch, windowed: bool) -> torch.Tensor:
            low, normal = batch["low_light"], batch["normal_light"]
            b = low.shape[0]
            noise = torch.randn(b, 3, hh, ww, generator=g, device=dev)
            idx = torch.randint(0, hi, (b,), generator=g, device=dev)
            guided = {}
            if self.distill.guidance:
                w_lo, w_hi = check_guidance_range(self.distill.guidance_scale_range)
                guided["w"] = torch.rand(b, generator=g, device=dev).mul_(w_hi - w_lo).add_(w_lo)
            return (self.step.accumulate if windowed else self.step)(low, normal, steps, noise=noise, idx=idx, **guided)

        return self._run_epoch(micro)

    @torch.no_grad()
    def validate(self) -> float:
        """`evaluate(distill.ema_student, val_loader, num_inference_steps=num_inference_steps, seed=config.seed, loss=False)`
        (through `enhance_frame` for a rectangular loader): returns the mean PSNR and keeps the whole result in
        `last_validation`; `val_guidance_scale` (the constructor's; normally None: a guided-distilled student needs no second
        forward) is passed on as `guidance_scale=`, here and in the sample sheet.  Parameters and the networks' train() / eval()
        modes are as before afterwards."""
        if self.val_loader is None:
            raise ValueError("validate needs a val_loader")
        net = self._net()
        mode = net.training
        try:
            res = evaluate(net, self.val_loader, num_inference_steps=self.num_inference_steps, seed=self.config.seed, loss=False,
                           **guided_keyword(self.val_guidance_scale))
        finally:
            net.train(mode)
        self.last_validation = res
        return res["psnr"]

    # ------------------------------------------------------------------ checkpoints
    def distill_entry(self) -> Dict[str, object]:
        """The checkpoint's "distill" entry: what a resumed run must agree on (DISTILL_KEYS)."""
        d = self.distill
        return {"num_ddim_timesteps": int(d.num_ddim_timesteps), "num_inference_steps": self.num_inference_steps,
                "ema_decay": self.ema_decay, "teacher_prediction": d.teacher_prediction, "student_prediction": d.student_prediction,
                "skip_terminal": bool(self.skip_terminal)}

    def checkpoint(self) -> dict:
        ckpt = {
            "epoch": int(self.epoch),
            "global_step": int(self.global_step),
            "model_state_dict": self.distill.ema_student.state_dict(),
            "student_state_dict": self.distill.student.state_dict(),
            "optimizer_state_dict": dict(self.optimizer.state_dict()),
            "scheduler_state_dict": self.scheduler.state_dict(),
            "best_psnr": float(self.best_psnr),
            "config": dict(self.config.__dict__),
            "distill": self.distill_entry(),
        }
        if self.scaler is not None:
            ckpt["scaler_state_dict"] = self.scaler.state_dict()
        return ckpt

    def load_checkpoint(self, path: str) -> None:
        """Continues after the saved epoch.  Read with weights_only=True (nothing from the file is executed).  A "distill" entry
        that is missing (a trainer's checkpoint) or differs from this distiller in a field is a ValueError naming it."""
        ckpt = torch.load(path, map_location=self.device, weights_only=True)
        have = ckpt.get("distill")
        if have is None or "student_state_dict" not in ckpt:
            raise ValueError(f"{path} is not a LowLightDistiller checkpoint (no 'distill' / 'student_state_dict' entry)")
        want = self.distill_entry()
        for key in DISTILL_KEYS:
            if key not in have or have[key] != want[key]:
                raise ValueError(f"{path} was written with distill[{key!r}] = {have.get(key)!r}, this distiller has {want[key]!r}")
        self.epoch = ckpt["epoch"] + 1
        self.global_step = ckpt["global_step"]
        self.best_psnr = ckpt["best_psnr"]
        for m, key in ((self.distill.ema_student, "model_state_dict"), (self.distill.student, "student_state_dict")):
            hostio.check_attention_kind(m, ckpt[key])
            m.load_state_dict(ckpt[key])
        self.optimizer.load_state_dict(ckpt["optimizer_state_dict"])
        self.scheduler.load_state_dict(ckpt["scheduler_state_dict"])
        if self.scaler is not None and "scaler_state_dict" in ckpt:
            self.scaler.load_state_dict(ckpt["scaler_state_dict"])
        self._say(f"Loaded checkpoint from epoch {self.epoch - 1}")
