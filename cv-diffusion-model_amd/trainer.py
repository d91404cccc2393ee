"""The reference's training loop (src/training/trainer.py: TrainingConfig, LowLightTrainer, train_model) on the HIP engine.

It joins what the package already has -- `TrainStep` (the step), `FusedAdamW` (clip, AdamW, EMA), `FusedGradScaler` (fp16 loss
scaling), `DevicePairLoader` (data), `evaluate` (validation) and `hostio` (checkpoints, PNG files) -- with torch's own
`CosineAnnealingLR` / `OneCycleLR`, into epochs that write the reference's checkpoints (`checkpoint_epoch_{e}.pt`,
`best_model.pt`, `final_model.pt`, read by scripts/inference.py and scripts/evaluate.py) and its per-epoch sample sheets
(`samples_epoch_{e}.png`).  The step itself is untouched; the one piece of device work added here is the sample sheet.

The sample sheet.  `comparison_grid_host` is the definition, written from torchvision's documented algorithm (torchvision is not
available to pin it against): `make_grid(cat([low, enhanced, normal]), nrow=n)` with the defaults padding = 2, pad_value = 0,
followed by `save_image`'s quantisation.  For n images of H x W per row the picture is uint8 HWC [3 (H+2) + 2][n (W+2) + 2][3]; the
image of row r (0 low-light, 1 enhanced, 2 normal-light) and column k has its top-left pixel at (r (H+2) + 2, k (W+2) + 2) and
every other byte is 0.  A pixel is, in separate fp32 operations,
    v = (x + 1) / 2;  q = v * 255 + 0.5;  q = min(max(q, 0), 255)  (NaN -> 0);  byte = trunc(q)
`comparison_grid` is the same on the device (csrc/samples.hip, one launch), bit for bit, and has no CPU fallback.
"""
from __future__ import annotations

from dataclasses import dataclass
from pathlib import Path
from typing import Dict, List, Optional, Tuple

import numpy as np
import torch
from torch.optim.lr_scheduler import CosineAnnealingLR, OneCycleLR

from . import _native as N
from . import hostio
from .data import create_device_dataloaders
from .ddim import check_sampler
from .guidance import check_cond_dropout, check_guidance_rescale, check_guidance_scale, guided_keyword
from .snrloss import check_snr_gamma
from .metrics import _require_hip, _steps_of, _swapped_weights, evaluate
from .pipeline import LowLightDiffusion
from .training import FusedAdamW, FusedGradScaler, TrainStep, accumulation_windows

try:
    import wandb
    HAS_WANDB = True
except ImportError:
    HAS_WANDB = False
    wandb = None

GRID_PADDING = 2  # kGridPad (csrc/kernels.h): make_grid's default
SAMPLE_STEPS = 4  # generate_samples enhances with 4 steps whatever the config says (trainer.py:380)


@dataclass
class TrainingConfig:
    """The reference's TrainingConfig (trainer.py:36-83), field for field, then this build's extensions."""

    # Model
    unet_variant: str = "small"
    image_size: int = 256
    num_inference_steps: int = 4

    # Training
    epochs: int = 100
    batch_size: int = 8
    learning_rate: float = 1e-4
    weight_decay: float = 0.01
    gradient_clip: float = 1.0

    # LR Scheduler
    scheduler_type: str = "cosine"  # "cosine" or "onecycle"
    warmup_epochs: int = 5
    min_lr: float = 1e-6

    # Mixed Precision: fp16 with a loss scaler, as the reference's autocast + GradScaler
    use_amp: bool = True

    # EMA
    use_ema: bool = True
    ema_decay: float = 0.9999

    # Loss
    loss_type: str = "mse"  # "mse", "huber", "l1"

    # Logging
    log_interval: int = 100  # batches; 0 = no progress line (and no host synchronisation inside an epoch)
    save_interval: int = 5  # epochs
    sample_interval: int = 1  # epochs
    num_samples: int = 4

    # Paths
    output_dir: str = "outputs"
    checkpoint_dir: str = "checkpoints"

    # Wandb
    use_wandb: bool = False
    wandb_project: str = "low-light-diffusion"
    wandb_run_name: Optional[str] = None

    # Resume
    resume_from: Optional[str] = None

    # ---- extensions
    compute_dtype: Optional[str] = None  # engine precision "fp32" | "fp16" | "bf16"; None: "fp16" with use_amp, else "fp32"
    seed: int = 0  # seeds every draw of the trainer (steps, validation, samples)
    use_synthetic: bool = False  # train_model: SyntheticLowLightDataset's degradation over the images in train_data_dir
    progress: bool = True  # print the progress and epoch lines


def resolved_compute_dtype(config: TrainingConfig) -> str:
    """The engine precision a config asks for: `compute_dtype`, or "fp16" / "fp32" by `use_amp`."""
    if config.compute_dtype is not None:
        return ("fp32", "fp16", "bf16")[N.dtype_code(config.compute_dtype)]  # ValueError for anything else
    return "fp16" if config.use_amp else "fp32"


def make_lr_scheduler(optimizer: torch.optim.Optimizer, config: TrainingConfig, steps_per_epoch: int):
    """The reference's schedule (trainer.py:158-175), its arithmetic kept as it is: total = steps_per_epoch * epochs, warmup =
    steps_per_epoch * warmup_epochs; "cosine" is CosineAnnealingLR(T_max=max(1, total - warmup), eta_min=min_lr) -- the warm-up
    only shortens the period, nothing ramps up -- and anything else OneCycleLR(max_lr=learning_rate, total_steps=total,
    pct_start=warmup / total).  It is stepped once per batch."""
    total_steps = steps_per_epoch * config.epochs
    warmup_steps = steps_per_epoch * config.warmup_epochs
    if config.scheduler_type == "cosine":
        return CosineAnnealingLR(optimizer, T_max=max(1, total_steps - warmup_steps), eta_min=config.min_lr)
    return OneCycleLR(optimizer, max_lr=config.learning_rate, total_steps=total_steps, pct_start=warmup_steps / total_steps)


def train_draw_seed(seed: int, epoch: int) -> int:
    """Seed of the device generator an epoch's (timesteps, noise) come from."""
    return (int(seed) * 1000003 + int(epoch) * 8191 + 54321) % (2 ** 63 - 1)


def distill_draw_seed(seed: int, epoch: int) -> int:
    """Seed of the device generator an epoch's distillation draws (noise, idx) come from (LowLightDistiller.train_epoch)."""
    return (int(seed) * 1000003 + int(epoch) * 8191 + 76543) % (2 ** 63 - 1)


def sample_draw_seed(seed: int, epoch: int) -> int:
    """Seed of the device generator an epoch's sample sheet draws its `enhance` noise from."""
    return (int(seed) * 1000003 + int(epoch) * 8191 + 65432) % (2 ** 63 - 1)


# ------------------------------------------------------------------ the sample sheet
def _grid_inputs(low, enhanced, normal, to_array):
    imgs = [to_array(v) for v in (low, enhanced, normal)]
    shape = tuple(imgs[0].shape)
    if len(shape) != 4 or shape[1] != 3 or shape[0] < 1 or shape[2] < 1 or shape[3] < 1:
        raise ValueError(f"images are NCHW [n,3,H,W] with n, H, W >= 1, got {shape}")
    for v in imgs[1:]:
        if tuple(v.shape) != shape:
            raise ValueError(f"the three image batches must have one shape, got {shape} and {tuple(v.shape)}")
    return imgs, shape


def comparison_grid_host(low, enhanced, normal) -> np.ndarray:
    """The definition of the module docstring: three fp32 [n,3,H,W] batches in the model's range -> uint8 [3 (H+2) + 2,
    n (W+2) + 2, 3]."""
    imgs, (n, _, h, w) = _grid_inputs(low, enhanced, normal, lambda v: np.asarray(v, dtype=np.float32))
    p = GRID_PADDING
    grid = np.zeros((3 * (h + p) + p, n * (w + p) + p, 3), dtype=np.uint8)
    one, two, half, top = np.float32(1.0), np.float32(2.0), np.float32(0.5), np.float32(255.0)
    for r, x in enumerate(imgs):
        with np.errstate(invalid="ignore", over="ignore"):
            q = ((x + one) / two) * top + half
            assert q.dtype == np.float32
            q = np.where(np.isnan(q), np.float32(0.0), np.minimum(np.maximum(q, np.float32(0.0)), top))
        byte = np.trunc(q).astype(np.uint8).transpose(0, 2, 3, 1)  # [n,H,W,3]
        for k in range(n):
            y0, x0 = r * (h + p) + p, k * (w + p) + p
            grid[y0:y0 + h, x0:x0 + w] = byte[k]
    return grid


def comparison_grid(low: torch.Tensor, enhanced: torch.Tensor, normal: torch.Tensor) -> torch.Tensor:
    """Device twin of comparison_grid_host: three fp32 [n,3,H,W] tensors on a HIP device -> uint8 [3 (H+2) + 2, n (W+2) + 2, 3] on
    that device.  One launch on the current stream, no synchronisation, bit-exact with the host twin."""
    for t in (low, enhanced, normal):
        _require_hip(t, "comparison_grid")

    def dev_array(t):
        if t.dtype != torch.float32:
            raise ValueError(f"images must be fp32 NCHW [n,3,H,W], got {t.dtype}")
        return t.detach().contiguous()

    (low, enhanced, normal), (n, _, h, w) = _grid_inputs(low, enhanced, normal, dev_array)
    dev = low.device
    if enhanced.device != dev or normal.device != dev:
        raise ValueError("the three image batches must be on one device")
    p = GRID_PADDING
    grid = torch.empty(3 * (h + p) + p, n * (w + p) + p, 3, dtype=torch.uint8, device=dev)
    with torch.cuda.device(dev):
        N.check(N.lib().llie_comparison_grid_u8(low.data_ptr(), enhanced.data_ptr(), normal.data_ptr(), n, h, w, grid.data_ptr(),
                                                torch.cuda.current_stream(dev).cuda_stream), "comparison_grid")
    return grid


# ------------------------------------------------------------------ checkpoints
CHECKPOINT_KEYS = ("epoch", "global_step", "model_state_dict", "optimizer_state_dict", "scheduler_state_dict", "best_val_loss", "config")


def build_checkpoint(*, epoch: int, global_step: int, model: torch.nn.Module, optimizer: torch.optim.Optimizer, scheduler,
                     best_val_loss: float, config: TrainingConfig, ema_shadow: Optional[Dict[str, torch.Tensor]] = None,
                     scaler=None) -> dict:
    """The reference's checkpoint dictionary (trainer.py:418-434): CHECKPOINT_KEYS, plus "ema_shadow" ({parameter name: tensor},
    EMAModel.shadow's layout) when given and "scaler_state_dict" when there is a scaler.  "optimizer_state_dict" has
    torch.optim.AdamW's layout: FusedAdamW's flat copy of the shadows is left out, they are stored once, by name.  Everything in
    it loads with torch.load(weights_only=True)."""
    opt_sd = dict(optimizer.state_dict())
    opt_sd.pop("ema_shadow_flat", None)
    ckpt = {
        "epoch": int(epoch),
        "global_step": int(global_step),
        "model_state_dict": model.state_dict(),
        "optimizer_state_dict": opt_sd,
        "scheduler_state_dict": scheduler.state_dict(),
        "best_val_loss": float(best_val_loss),
        "config": dict(config.__dict__),
    }
    if ema_shadow is not None:
        ckpt["ema_shadow"] = dict(ema_shadow)
    if scaler is not None:
        ckpt["scaler_state_dict"] = scaler.state_dict()
    return ckpt


# ------------------------------------------------------------------ the trainer
def _loader_device(loader) -> torch.device:
    store = getattr(loader, "store", None)
    dev = getattr(store, "device", None)
    if dev is None:
        raise ValueError(f"a loader is a DevicePairLoader (create_device_dataloaders), got {type(loader).__name__}")
    return torch.device(dev)


class _EpochLoop:
    """What LowLightTrainer and LowLightDistiller (distiller.py) share: the constructor's checks of `crop_size`, `accumulate` and the
    devices, the epoch schedule of `train` (validation, checkpoints, best model, sample sheets), the batch loop of an epoch with
    its accumulation windows and LR schedule, the sample sheet and `save_checkpoint`.  A subclass provides `optimizer`,
    `scheduler`, `step`, `train_epoch`, `validate`, `checkpoint`, `load_checkpoint`, the network that validation and the sample
    sheet run (`_net`, with `_net_weights` swapped in), and what an epoch logs and when it is the best one (`_epoch_log`,
    `_set_best`)."""

    _what = "training"
    val_sampler = "lcm"
    val_steps: Optional[int] = None
    val_guidance_scale: Optional[float] = None
    val_guidance_rescale: Optional[float] = None

    # ------------------------------------------------------------------ construction
    def _init_shapes(self, config: Optional[TrainingConfig], train_loader, val_loader, crop_size, accumulate) -> None:
        """`config`, `accumulate` and `crop_size` (default: config.image_size squared), checked against the loaders."""
        self.config = config or TrainingConfig()
        cfg = self.config
        if isinstance(accumulate, bool) or not isinstance(accumulate, int) or accumulate < 1:
            raise ValueError(f"accumulate must be an integer >= 1, got {accumulate!r}")
        self.accumulate = accumulate
        if crop_size is None:
            self.crop_size = (int(cfg.image_size), int(cfg.image_size))
        else:
            if len(crop_size) != 2:
                raise ValueError(f"crop_size is (H, W), got {crop_size!r}")
            self.crop_size = (int(crop_size[0]), int(crop_size[1]))
            if self.crop_size[0] == self.crop_size[1] and self.crop_size[0] != int(cfg.image_size):
                raise ValueError(f"a square crop_size is config.image_size ({cfg.image_size}), got {self.crop_size[0]}: validation "
                                 "of square crops runs `enhance`, which takes image_size only")
            for what, loader in (("train_loader", train_loader), ("val_loader", val_loader)):
                have = getattr(loader, "crop_size", None)
                if loader is not None and have is not None and tuple(have) != self.crop_size:
                    raise ValueError(f"{what} crops {have[0]} x {have[1]}, crop_size is {self.crop_size[0]} x {self.crop_size[1]}")

    def _init_devices(self, model: torch.nn.Module, train_loader, val_loader) -> None:
        """`device`: the one HIP device the model and the loaders are on; a train loader that yields a batch."""
        who = type(self).__name__
        params = list(model.parameters())
        places = [("the model", params[0].device if params else torch.device("cpu")), ("train_loader", _loader_device(train_loader))]
        if val_loader is not None:
            places.append(("val_loader", _loader_device(val_loader)))
        for what, dev in places:
            if dev.type != "cuda":
                raise RuntimeError(f"{who} runs only on a HIP device ({what} is on '{dev}'); there is no CPU fallback")
        self.device = places[0][1]
        for what, dev in places[1:]:
            if dev != self.device:
                raise ValueError(f"{what} is on {dev}, the model on {self.device}")
        if len(train_loader) < 1:
            raise ValueError("train_loader yields no batch (fewer pairs than batch_size: the last partial batch is dropped)")

    def _init_run(self) -> None:
        """Counters, the output directories, wandb."""
        cfg = self.config
        self.epoch = 0
        self.global_step = 0
        self.last_validation: Optional[Dict[str, object]] = None  # evaluate()'s result of the latest validate()
        self.output_dir = Path(cfg.output_dir)
        self.checkpoint_dir = Path(cfg.checkpoint_dir)
        self.output_dir.mkdir(parents=True, exist_ok=True)
        self.checkpoint_dir.mkdir(parents=True, exist_ok=True)
        if cfg.use_wandb:
            if not HAS_WANDB:
                print("Warning: wandb not installed. Logging disabled.")
                cfg.use_wandb = False
            else:
                wandb.init(project=cfg.wandb_project, name=cfg.wandb_run_name, config=cfg.__dict__)

    def _say(self, *a, **kw) -> None:
        if self.config.progress:
            print(*a, **kw)

    # ------------------------------------------------------------------ epochs
    def train(self, on_epoch=None) -> List[Dict[str, object]]:
        """The reference's loop (trainer.py:216-267): per epoch train, validate when there is a val loader, write
        checkpoint_epoch_{e}.pt when (e + 1) % save_interval == 0, best_model.pt when the epoch is the best so far (the trainer:
        a strictly lower validation loss; the distiller: a strictly higher PSNR) and the sample sheet when
        (e + 1) % sample_interval == 0; final_model.pt at the end.  Returns one dictionary per epoch run, the trainer's
        {"epoch", "train_loss", "lr", "val_loss", "psnr", "ssim"} (the last three None without a val loader); the distiller's
        has no "val_loss"."""
        cfg = self.config
        self._say(f"Starting {self._what} on {self.device}")
        self._say(f"Model parameters: {self._net().get_model_size()}")
        history = []
        for epoch in range(self.epoch, cfg.epochs):
            self.epoch = epoch
            train_loss = self.train_epoch()
            log, line, best = self._epoch_log(epoch, train_loss)
            history.append(log)
            if on_epoch is not None:
                on_epoch(log)
            self._say(line)
            if cfg.use_wandb:
                wandb.log({k: v for k, v in log.items() if v is not None})
            if (epoch + 1) % cfg.save_interval == 0:
                self.save_checkpoint(f"checkpoint_epoch_{epoch}.pt")
            if best:
                self._set_best(log)
                self.save_checkpoint("best_model.pt")
            if (epoch + 1) % cfg.sample_interval == 0:
                self.generate_samples(epoch)
        self.save_checkpoint("final_model.pt")
        if cfg.use_wandb:
            wandb.finish()
        return history

    def _run_epoch(self, micro) -> float:
        """The batch loop of an epoch.  `micro(batch, windowed)` makes the batch's draws and runs `step(...)` (windowed False: a
        whole optimiser step) or `step.accumulate(...)` (True), returning the batch loss; with `accumulate=k` > 1 `step.apply()`
        follows the last batch of each window (accumulation_windows(n, k)).  The LR schedule moves once per optimiser step,
        after it, also when a grad scaler skipped the step.  The losses go into a device buffer that is copied once, after the
        last batch; nothing else waits for the device, except the progress line.  Returns the Python-float sum of the fp32
        batch losses in step order, divided by the number of batches."""
        cfg, dev, loader = self.config, self.device, self.train_loader
        n = len(loader)
        losses = torch.zeros(n, dtype=torch.float32, device=dev)
        report = cfg.log_interval > 0 and (cfg.progress or cfg.use_wandb)
        ends, done = set(), 0  # 1-based index of each window's last batch
        for length in accumulation_windows(n, self.accumulate):
            done += length
            ends.add(done)
        for batch_idx, batch in enumerate(loader):
            if self.accumulate == 1:
                loss = micro(batch, False)
                stepped = True
            else:
                loss = micro(batch, True)
                stepped = batch_idx + 1 in ends
                if stepped:
                    self.step.apply()
            if stepped:
                # the steps go through step_flat, not optimizer.step(), which torch's scheduler watches to warn about a
                # schedule that moves before the optimiser: the optimiser has stepped
                self.optimizer._opt_called = True
                self.scheduler.step()
                self.global_step += 1
            losses[batch_idx].copy_(loss)
            if report and batch_idx % cfg.log_interval == 0:
                value = loss.item()
                self._say(f"Epoch {self.epoch} [{batch_idx + 1}/{n}] loss={value:.4f}")
                if cfg.use_wandb:
                    wandb.log({"train_loss_step": value, "lr": self.optimizer.param_groups[0]["lr"], "global_step": self.global_step})
        total = 0.0
        for v in losses.cpu().tolist():  # the one device-to-host copy
            total += v
        return total / n

    def _val_steps(self, default: int) -> int:
        return default if self.val_steps is None else self.val_steps

    @torch.no_grad()
    def generate_samples(self, epoch: int) -> Path:
        """The sample sheet of trainer.py:365-410: the first `num_samples` pairs of the first batch of `val_loader or
        train_loader`, enhanced with 4 steps (the trainer: on the EMA weights when EMA is on; the distiller: by the EMA student),
        as output_dir/samples_epoch_{epoch}.png (rows: low-light, enhanced, normal-light).

        Draws: g = torch.Generator(device=dev).manual_seed((seed * 1000003 + epoch * 8191 + 65432) % (2 ** 63 - 1));
        noise = torch.randn(steps, n, 3, S, S, generator=g, device=dev) with steps the scheduler's step count for 4
        (`val_steps` replaces the 4; with val_sampler="ddim" or "dpmpp_2m" steps = 1, the initial latents, and the loop is that
        sampler's).
        With a rectangular `crop_size` the images are [n, 3, H, W] and the loop is `enhance_frame`'s.  `val_guidance_scale`
        is passed on as `guidance_scale=` (classifier-free guidance) and `val_guidance_rescale` as `guidance_rescale=`; the draws
        do not depend on them.
        The loader's epoch counter, the parameters and the network's mode are as before afterwards."""
        cfg, dev = self.config, self.device
        loader = self.val_loader or self.train_loader
        loader_epoch = loader.epoch
        try:
            batch = next(iter(loader))
        finally:
            loader.set_epoch(loader_epoch)  # the peek is not an epoch
        low = batch["low_light"][:cfg.num_samples].contiguous()
        normal = batch["normal_light"][:cfg.num_samples].contiguous()
        net = self._net()
        mode = net.training
        try:
            with _swapped_weights(net, self._net_weights()):
                nsteps, steps = _steps_of(net, self._val_steps(SAMPLE_STEPS), dev, self.val_sampler)
                g = torch.Generator(device=dev).manual_seed(sample_draw_seed(cfg.seed, epoch))
                noise = torch.randn(steps, low.shape[0], 3, low.shape[2], low.shape[3], generator=g, device=dev)
                enhance = net.enhance_frame if self.crop_size[0] != self.crop_size[1] else net.enhance
                enhanced = enhance(low, nsteps, noise=noise, sampler=self.val_sampler,
                                   **guided_keyword(self.val_guidance_scale, self.val_guidance_rescale))
                grid = comparison_grid(low, enhanced, normal).cpu().numpy()  # the one device-to-host copy
        finally:
            net.train(mode)
        path = self.output_dir / f"samples_epoch_{epoch}.png"
        hostio.save_image(str(path), grid)
        if cfg.use_wandb:
            wandb.log({"samples": wandb.Image(str(path))})
        return path

    def save_checkpoint(self, filename: str) -> None:
        torch.save(self.checkpoint(), self.checkpoint_dir / filename)
        self._say(f"Saved checkpoint: {filename}")


class LowLightTrainer(_EpochLoop):
    """The reference's LowLightTrainer (trainer.py:121-456) over the engine: same constructor, methods, schedule of
    validation / checkpoints / samples and checkpoint layout.

    `model` is a LowLightDiffusion on a HIP device, the loaders are DevicePairLoaders on the same device; there is no CPU
    fallback.  The engine runs in `resolved_compute_dtype(config)`; a FusedGradScaler exists only for fp16.  Every draw comes
    from generators seeded from (config.seed, epoch): the global generator is neither read nor advanced, and a resumed run
    continues bit for bit.

    `x0_ssim_weight` / `x0_l1_weight` (extension) go to TrainStep: the training loss gains the x0 term of pipeline.py, SSIM / L1
    of the predicted clean image against the normal-light image.  They are constructor arguments, not TrainingConfig fields,
    and are not written into checkpoints: a caller that resumes a run passes them again.  The validation loss stays the
    reference's MSE.

    `snr_gamma=g` (extension; finite, > 0, None = off; a keyword like the x0 weights: neither a TrainingConfig field nor stored in
    checkpoints, a caller that resumes a run passes it again) goes to TrainStep: Min-SNR-gamma weighting of the training loss
    (snrloss.py).  The validation loss in `validate` / `evaluate` stays unweighted, so that runs with and without the flag stay
    comparable.

    `val_sampler` / `val_steps` (extension; keywords like the x0 weights, neither TrainingConfig fields nor stored in checkpoints)
    choose how validation and the sample sheet sample: val_sampler="ddim" is the deterministic sampler a many-step (teacher)
    model wants, where the default "lcm" shows the 4-step loop of a consistency student; `val_steps` replaces
    config.num_inference_steps in `validate` and the 4 steps of `generate_samples` (None keeps both; with "ddim" anything in
    1..num_train_timesteps; val_sampler="dpmpp_2m" is the second-order sampler of dpm.py for the same models, at any step count
    `model.dpm_schedule` accepts).  A schedule the model does not have is a ValueError here, not at the first validation.

    Classifier-free guidance (extension; guidance.py; keywords like the x0 weights, neither TrainingConfig fields nor stored in
    checkpoints).  `cond_dropout=p` in [0, 1] goes to TrainStep: with p > 0 each sample's condition is replaced by the null
    condition with probability p, and `train_epoch`'s draw recipe gains a third draw per batch (its docstring).
    `val_guidance_scale=w` makes `validate` and `generate_samples` sample with `guidance_scale=w` (None: unguided; the
    validation loss is not affected); `val_guidance_rescale=phi` in [0, 1] adds `guidance_rescale=phi` to those calls (None:
    nothing is handed on).

    `crop_size=(H, W)` (extension; a keyword like the x0 weights, neither a TrainingConfig field nor stored in checkpoints: a caller
    that resumes passes it again) trains at a frame's own shape instead of config.image_size x config.image_size: the loaders must
    crop (H, W) (`DevicePairLoader(..., image_size=(H, W))`), `train_epoch` draws its noise at that shape, and `validate` /
    `generate_samples` run `enhance_frame`.  The model keeps the module tree config.image_size fixed; (H, W) is any shape
    llie_train_shape_ok accepts at the batch size (checked here).

    `accumulate=k` (extension; an integer >= 1, a keyword like `crop_size`: neither a TrainingConfig field nor stored in
    checkpoints, a caller that resumes passes it again) takes one optimiser step per window of k consecutive loader batches
    (`TrainStep.accumulate` x k, then `apply`): the effective batch is k * batch_size.  The windows of an epoch of n batches are
    `accumulation_windows(n, k)`: the last one holds the remaining n mod k batches and is applied, nothing carries across an
    epoch, so a checkpoint never holds an open window.  The LR schedule is built for ceil(n / k) steps per epoch and moves once
    per `apply`; `global_step` counts optimiser steps.  k = 1 is the code path without the keyword, bit for bit."""

    def __init__(self, model: LowLightDiffusion, train_loader, val_loader=None, config: Optional[TrainingConfig] = None, *,
                 x0_ssim_weight: float = 0.0, x0_l1_weight: float = 0.0, val_sampler: str = "lcm", val_steps: Optional[int] = None,
                 crop_size: Optional[Tuple[int, int]] = None, accumulate: int = 1, cond_dropout: float = 0.0,
                 val_guidance_scale: Optional[float] = None, snr_gamma: Optional[float] = None,
                 val_guidance_rescale: Optional[float] = None):
        self.snr_gamma = check_snr_gamma(snr_gamma)
        self._init_shapes(config, train_loader, val_loader, crop_size, accumulate)
        cfg = self.config
        self.cond_dropout = check_cond_dropout(cond_dropout)
        self.val_guidance_scale = check_guidance_scale(val_guidance_scale)
        self.val_guidance_rescale = None if val_guidance_rescale is None else check_guidance_rescale(val_guidance_rescale)
        self.val_sampler = check_sampler(val_sampler)
        if val_steps is not None and (isinstance(val_steps, bool) or int(val_steps) != val_steps or val_steps < 1):
            raise ValueError(f"val_steps must be a positive integer or None, got {val_steps!r}")
        self.val_steps = None if val_steps is None else int(val_steps)
        if self.val_sampler != "lcm":
            for n in (self._val_steps(cfg.num_inference_steps), self._val_steps(SAMPLE_STEPS)):
                (model.ddim_schedule if self.val_sampler == "ddim" else model.dpm_schedule)(n)
        self._init_devices(model, train_loader, val_loader)
        dtype = resolved_compute_dtype(cfg)

        self.model = model
        self.model.compute_dtype = dtype
        if crop_size is not None:  # ValueError naming the rule, here and not at the first step
            model.unet._handle(N.dtype_code(dtype)).train_shape_ok(max(1, int(getattr(train_loader, "batch_size", 1))), *self.crop_size)
        self.train_loader = train_loader
        self.val_loader = val_loader

        self.optimizer = FusedAdamW(model.parameters(), lr=cfg.learning_rate, weight_decay=cfg.weight_decay,
                                    max_grad_norm=cfg.gradient_clip, ema_decay=cfg.ema_decay if cfg.use_ema else None)
        self.scheduler = make_lr_scheduler(self.optimizer, cfg, len(accumulation_windows(len(train_loader), accumulate)))
        self.scaler = FusedGradScaler() if dtype == "fp16" else None
        self.step = TrainStep(model, self.optimizer, loss_type=cfg.loss_type, grad_scaler=self.scaler,
                              x0_ssim_weight=x0_ssim_weight, x0_l1_weight=x0_l1_weight, cond_dropout=self.cond_dropout,
                              **({} if self.snr_gamma is None else {"snr_gamma": self.snr_gamma}))
        self._names = [name for name, _ in model.named_parameters()]

        self.best_val_loss = float("inf")
        self._init_run()

        if cfg.resume_from:
            self.load_checkpoint(cfg.resume_from)

    def _ema_weights(self) -> Optional[List[torch.Tensor]]:
        return self.optimizer.ema_tensors() if self.config.use_ema else None

    def _net(self) -> LowLightDiffusion:
        return self.model

    def _net_weights(self) -> Optional[List[torch.Tensor]]:
        return self._ema_weights()

    # ------------------------------------------------------------------ epochs (`train`: _EpochLoop)
    def _epoch_log(self, epoch: int, train_loss: float):
        """Validate (when there is a val loader) -> (the epoch's log, its progress line, whether it is the best so far: a
        strictly lower validation loss)."""
        val_loss = self.validate() if self.val_loader is not None else None
        log = {"epoch": epoch, "train_loss": train_loss, "lr": self.optimizer.param_groups[0]["lr"], "val_loss": val_loss,
               "psnr": self.last_validation["psnr"] if val_loss is not None else None,
               "ssim": self.last_validation["ssim"] if val_loss is not None else None}
        line = f"Epoch {epoch}: train_loss={train_loss:.4f}"
        if val_loss is not None:
            line += f", val_loss={val_loss:.4f}, psnr={log['psnr']:.2f}, ssim={log['ssim']:.4f}"
        return log, line, val_loss is not None and val_loss < self.best_val_loss

    def _set_best(self, log: Dict[str, object]) -> None:
        self.best_val_loss = log["val_loss"]

    def train_epoch(self) -> float:
        """One epoch (trainer.py:269-338) of TrainStep over the train loader.

        Draw recipe (part of the contract; the global generator is neither read nor advanced):
          train_loader.set_epoch(epoch); dev = the model's device; S = config.image_size (with `crop_size=(H, W)` every
          [b, 3, S, S] below is [b, 3, H, W]); T = scheduler.config.num_train_timesteps;
          g = torch.Generator(device=dev).manual_seed((seed * 1000003 + epoch * 8191 + 54321) % (2 ** 63 - 1))
          per batch of b pairs, in loader order, the reference's order of draws (low_light_diffusion.py: timesteps, then noise):
            t = torch.randint(0, T, (b,), generator=g, device=dev)
            noise = torch.randn(b, 3, S, S, generator=g, device=dev)
            u = torch.rand(b, generator=g, device=dev)                  only with cond_dropout = P > 0
            loss = step(low_light, normal_light, timesteps=t, noise=noise[, cond_u=u]);  lr_scheduler.step()
        The LR schedule moves once per batch, after the step, also when a grad scaler skipped the step.  The losses go into a
        device buffer that is copied once, after the last batch; nothing else waits for the device, except the progress line
        (every `log_interval` batches; `log_interval = 0` or `progress = False` without wandb turns it off).  Returns the
        Python-float sum of the fp32 batch losses in step order, divided by len(train_loader) (trainer.py:325,338).

        With `accumulate=k` > 1 the draws are the same, per batch and in the same order; `step(...)` becomes
        `step.accumulate(...)`, and after the last batch of each window (accumulation_windows(n, k)) come `step.apply()` and
        `lr_scheduler.step()`.  The returned value is still the sum of the batch losses divided by n."""
        cfg, dev, loader = self.config, self.device, self.train_loader
        self.model.train()
        loader.set_epoch(self.epoch)
        (hh, ww), t_max = self.crop_size, int(self.model.scheduler.config.num_train_timesteps)
        g = torch.Generator(device=dev).manual_seed(train_draw_seed(cfg.seed, self.epoch))

        def micro(batch, windowed: bool) -> torch.Tensor:
            low, normal = batch["low_light"], batch["normal_light"]
            b = low.shape[0]
            t = torch.randint(0, t_max, (b,), generator=g, device=dev)
            noise = torch.randn(b, 3, hh, ww, generator=g, device=dev)
            drop = {"cond_u": torch.rand(b, generator=g, device=dev)} if self.cond_dropout > 0 else {}
            return (self.step.accumulate if windowed else self.step)(low, normal, timesteps=t, noise=noise, **drop)

        return self._run_epoch(micro)

    @torch.no_grad()
    def validate(self) -> float:
        """`evaluate(model, val_loader, num_inference_steps=config.num_inference_steps, seed=config.seed)` (with `val_sampler` and
        `val_steps` where the constructor got them) on the EMA weights
        when EMA is on: returns its "loss" (the reference's validation loss, trainer.py:340-363, with seeded draws: the same
        weights always give the same loss) and keeps the whole result in `last_validation` (PSNR / SSIM for the epoch's log line).
        Parameters, optimiser state and the model's train() / eval() mode are as before afterwards."""
        if self.val_loader is None:
            raise ValueError("validate needs a val_loader")
        mode = self.model.training
        try:
            res = evaluate(self.model, self.val_loader, num_inference_steps=self._val_steps(self.config.num_inference_steps),
                           seed=self.config.seed, weights=self._ema_weights(), sampler=self.val_sampler,
                           **guided_keyword(self.val_guidance_scale, self.val_guidance_rescale))
        finally:
            self.model.train(mode)
        self.last_validation = res
        return res["loss"]

    # ------------------------------------------------------------------ checkpoints
    def ema_shadow(self) -> Optional[Dict[str, torch.Tensor]]:
        """{parameter name as in model.named_parameters(): shadow weight} (copies), the reference's EMAModel.shadow; None
        without EMA."""
        if not self.config.use_ema:
            return None
        return {name: t.clone() for name, t in zip(self._names, self.optimizer.ema_tensors())}

    def checkpoint(self) -> dict:
        return build_checkpoint(epoch=self.epoch, global_step=self.global_step, model=self.model, optimizer=self.optimizer,
                                scheduler=self.scheduler, best_val_loss=self.best_val_loss, config=self.config,
                                ema_shadow=self.ema_shadow(), scaler=self.scaler)

    def load_checkpoint(self, path: str) -> None:
        """trainer.py:437-456: continues after the saved epoch.  Read with weights_only=True (nothing from the file is
        executed).  The EMA shadows are copied by name; a name the model does not have, or one of its names missing from the
        file, is a ValueError."""
        ckpt = torch.load(path, map_location=self.device, weights_only=True)
        shadow = ckpt.get("ema_shadow") if self.config.use_ema else None
        if shadow is not None:
            missing = [k for k in self._names if k not in shadow]
            unexpected = [k for k in shadow if k not in set(self._names)]
            if missing or unexpected:
                raise ValueError(f"ema_shadow does not fit the model: missing {missing[:5]}, unexpected {unexpected[:5]}")
        self.epoch = ckpt["epoch"] + 1
        self.global_step = ckpt["global_step"]
        self.best_val_loss = ckpt["best_val_loss"]
        hostio.check_attention_kind(self.model, ckpt["model_state_dict"])
        self.model.load_state_dict(ckpt["model_state_dict"])
        self.optimizer.load_state_dict(ckpt["optimizer_state_dict"])
        self.scheduler.load_state_dict(ckpt["scheduler_state_dict"])
        if shadow is not None:
            with torch.no_grad():
                for name, dst in zip(self._names, self.optimizer.ema_tensors()):
                    dst.copy_(shadow[name])
        if self.scaler is not None and "scaler_state_dict" in ckpt:
            self.scaler.load_state_dict(ckpt["scaler_state_dict"])
        self._say(f"Loaded checkpoint from epoch {self.epoch - 1}")


def train_model(train_data_dir: str, val_data_dir: Optional[str] = None, config: Optional[TrainingConfig] = None,
                device="cuda", *, x0_ssim_weight: float = 0.0, x0_l1_weight: float = 0.0, val_sampler: str = "lcm",
                val_steps: Optional[int] = None, crop_size: Optional[Tuple[int, int]] = None, accumulate: int = 1,
                cond_dropout: float = 0.0, val_guidance_scale: Optional[float] = None,
                snr_gamma: Optional[float] = None, val_guidance_rescale: Optional[float] = None) -> LowLightTrainer:
    """Training entry point (trainer.py:459-496): loaders from the folders (create_device_dataloaders), a fresh model, a trainer,
    `train()`; returns the trainer.  `x0_ssim_weight` / `x0_l1_weight` / `val_sampler` / `val_steps` / `crop_size`: as
    LowLightTrainer's (with `crop_size=(H, W)` the loaders crop H x W; the model is still built at config.image_size);
    `accumulate` / `cond_dropout` / `val_guidance_scale` / `val_guidance_rescale` / `snr_gamma`: LowLightTrainer's."""
    config = config or TrainingConfig()
    train_loader, val_loader = create_device_dataloaders(train_root=train_data_dir, val_root=val_data_dir, batch_size=config.batch_size,
                                                         image_size=config.image_size if crop_size is None else tuple(crop_size),
                                                         use_synthetic=config.use_synthetic,
                                                         device=device, seed=config.seed)
    model = LowLightDiffusion(unet_variant=config.unet_variant, image_size=config.image_size,
                              num_inference_steps=config.num_inference_steps).to(train_loader.store.device)
    trainer = LowLightTrainer(model=model, train_loader=train_loader, val_loader=val_loader, config=config,
                              x0_ssim_weight=x0_ssim_weight, x0_l1_weight=x0_l1_weight, val_sampler=val_sampler, val_steps=val_steps,
                              crop_size=crop_size, accumulate=accumulate, cond_dropout=cond_dropout,
                              val_guidance_scale=val_guidance_scale, snr_gamma=snr_gamma, val_guidance_rescale=val_guidance_rescale)
    trainer.train()
    return trainer
