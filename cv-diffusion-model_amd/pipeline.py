"""Drop-in `LowLightDiffusion` (src/models/low_light_diffusion.py:31-281) on the HIP engine.

Constructor, `forward` / `enhance` / `compute_loss` / `get_model_size` signatures, attributes
(`.unet`, `.scheduler`, `.image_size`, `.condition_mode`) and the `state_dict` layout (all keys under
`unet.`) are the reference's, so scripts/inference.py and scripts/benchmark.py of the reference can
call it unchanged.  The whole denoising loop runs as one launch sequence in libllie_hip.so.

`LowLightLCMDistillation` (low_light_diffusion.py:284-408) is the teacher -> student consistency-distillation
objective on the same engine: the denoisers run through the engine's forward / backward passes, the arithmetic
around them and the EMA update through csrc/distill.hip.

The x0 term (`x0_loss`, `x0_loss_host`; csrc/ssimloss.hip, llie_x0_loss) is an image-space addition to the training loss:
SSIM and L1 of the clean image a training step implies against the normal-light image.  With `out` the network output
[B,3,H,W], `x_t` the noised input, `y` the normal-light image, abar_b = alphas_cumprod[t_b], alpha = sqrt(abar), sigma = sqrt(1 - abar):
  x^ = p_b x_t + q_b out        epsilon prediction: p = 1 / alpha, q = -sigma / alpha;  v prediction: p = alpha, q = -sigma;  not clamped
  L_x0 = (1 / B) sum_b w_b [ssim_weight (1 - SSIM_b(x^, y)) + l1_weight mean|x^_b - y_b|],   w_b = abar_b
  SSIM_b is metrics.py's definition with data_range (-1, 1); the L1 mean runs over the 3 H W values in model units (F.l1_loss)
  dL_x0/dout = (w_b / B) q_b [-ssim_weight / 2 dSSIM_b/dx + l1_weight sign(x^ - y) / (3 H W)]     (dSSIM/dx: metrics.py)
The weight w_b = abar_b keeps the gradient factor w q = -alpha sigma bounded under epsilon prediction.  A sample with abar_b == 0
(t = 999 of the zero-SNR table, where x0 is undefined) contributes exactly 0 to the loss and nothing to the gradient.
"""
from __future__ import annotations

import copy
import ctypes as C
from dataclasses import dataclass
from typing import Dict, List, Optional, Sequence, Tuple, Union

import numpy as np
import torch
import torch.nn as nn
import torch.nn.functional as F

from . import _native as N
from .ddim import check_sampler
from . import dpm as DPM
from . import guidance as G
from .scheduler import LCMScheduler
from .snrloss import check_snr_gamma
from .unet import EfficientUNet, create_efficient_unet


@dataclass
class LowLightDiffusionOutput:
    enhanced: torch.Tensor
    intermediate: Optional[list] = None


def supplied_noise(noise, draws: int, b: int, h: int, w: int, device, sampler: str = "lcm") -> torch.Tensor:
    """`noise=` of `enhance` / `enhance_frame` as the fp32 [draws,b,3,h,w] tensor the engine reads: a tensor of that shape or a
    list of `draws` tensors [b,3,h,w].  draws = the step count for the LCM loop, 1 for DDIM and DPM-Solver++ (the initial latents
    only)."""
    noise_t = noise if isinstance(noise, torch.Tensor) else torch.stack([n.to(device) for n in noise])
    noise_t = noise_t.to(device=device, dtype=torch.float32)
    if tuple(noise_t.shape) != (draws, b, 3, h, w):
        raise ValueError(f"noise must be [{draws},{b},3,{h},{w}]" + (" (DDIM draws the initial latents only)" if sampler == "ddim" else
                                                             " (DPM-Solver++ draws the initial latents only)" if sampler == "dpmpp_2m" else "")
                         + f", got {list(noise_t.shape)}")
    return noise_t


class LowLightDiffusion(nn.Module):
    def __init__(self, unet: Optional[EfficientUNet] = None, scheduler: Optional[LCMScheduler] = None,
                 unet_variant: str = "small", image_size: int = 256, num_inference_steps: int = 4,
                 condition_mode: str = "concat", compute_dtype: Optional[str] = None,
                 allow_unpinned_groupnorm: bool = False):
        """Arguments as in low_light_diffusion.py:50-58.  `compute_dtype` (extension; "fp32" | "fp16" |
        "bf16") pins the engine precision; when None the engine runs fp32, or the dtype of an active
        `torch.autocast("cuda")` region."""
        super().__init__()
        if condition_mode != "concat":
            # "add" routes low_light through a small conv encoder (:108-113,159-160); no caller of the
            # reference ever selects it, and it is outside the hot-path scope.
            raise NotImplementedError('condition_mode="add" is not provided by the HIP engine')
        self.image_size = image_size
        self.num_inference_steps = num_inference_steps
        self.condition_mode = condition_mode
        in_channels = 6
        extra = {"allow_unpinned_groupnorm": True} if allow_unpinned_groupnorm else {}  # tiny / base: see unet.py
        self.unet = unet if unet is not None else create_efficient_unet(
            variant=unet_variant, image_size=image_size, in_channels=in_channels, **extra)
        self.scheduler = scheduler if scheduler is not None else LCMScheduler(
            num_train_timesteps=1000, beta_schedule="scaled_linear", prediction_type="epsilon",
            num_inference_steps=num_inference_steps, rescale_betas_zero_snr=True)
        self.compute_dtype = compute_dtype
        object.__setattr__(self, "_t_cache", {})  # (timesteps, batch, device) -> device int64 [steps*B]

    def __getstate__(self):  # copy.deepcopy / pickling: device caches are rebuilt lazily
        st = dict(self.__dict__)
        st["_t_cache"] = {}
        return st

    @property
    def compute_dtype(self) -> Optional[str]:
        return self.unet.compute_dtype

    @compute_dtype.setter
    def compute_dtype(self, v: Optional[str]) -> None:
        self.unet.compute_dtype = v

    # ------------------------------------------------------------------ training-side forward (:115-175)
    def forward(self, low_light: torch.Tensor, normal_light: Optional[torch.Tensor] = None,
                timesteps: Optional[torch.Tensor] = None, noise: Optional[torch.Tensor] = None,
                return_dict: bool = True, *, frame: bool = False, cond_dropout: float = 0.0,
                cond_u: Optional[torch.Tensor] = None) -> Union[torch.Tensor, Dict[str, torch.Tensor]]:
        """With `normal_light`: q-sample -> denoiser, returning {noise_pred, noise, timesteps}.  When gradients
        are enabled `noise_pred` carries a grad_fn whose backward is the engine's reverse pass
        (llie_unet_backward): `loss.backward()` fills `.grad` of every parameter, so the reference trainer's
        step (trainer.py:269-338: AdamW, GradScaler, clip_grad_norm_, EMA) runs unchanged on top.
        A `low_light` that requires a gradient receives one from the same backward pass
        (llie_unet_backward_dx), so a trainable module may sit in front of the denoiser; the parameter gradients are the
        same bits either way.
        With a `prediction_type="v_prediction"` scheduler the dict also holds the velocity `target`
        (lcm_scheduler.py:282-305; the reference never wires it into `compute_loss`).  A caller that forms the x0 term needs
        the noised input too: it is `scheduler.add_noise(normal_light, noise, timesteps)` of the returned draws.
        `frame=True` (extension): the training branch runs at the batch's own H x W, any shape llie_train_shape_ok accepts
        (EfficientUNet.forward_split); without it a shape other than image_size is a ValueError, as before.
        `cond_dropout=p` (extension; classifier-free guidance training, guidance.py): with p > 0 row b of `low_light` is replaced
        by the null condition (all zeros) where u[b] < p, by llie_cond_dropout, before the denoiser; u is `cond_u` (fp32 [B]) or
        `torch.rand(B, device=device)` drawn from the global device generator after the timestep and noise draws.  The
        gradient of `low_light` is masked by the same kernel: dropped rows are exactly 0.  With p == 0 no draw is made and the
        call is what it was.
        Without `normal_light`: `enhance(low_light)`."""
        p_drop = G.check_cond_dropout(cond_dropout)
        if normal_light is None:
            return self.enhance(low_light)
        batch, device = low_light.shape[0], low_light.device
        if timesteps is None:
            timesteps = torch.randint(0, self.scheduler.config.num_train_timesteps, (batch,), device=device)
        if noise is None:
            noise = torch.randn_like(normal_light)
        if p_drop > 0:
            _require_hip(low_light, "LowLightDiffusion.forward")
            low_light = _CondDropoutFn.apply(low_light, cond_uniforms(cond_u, batch, device), p_drop)
        noisy = self.scheduler.add_noise(normal_light, noise, timesteps)
        noise_pred = self.unet.forward_split(noisy, low_light, timesteps, uniform_t=False, frame=frame)
        if return_dict:
            out = {"noise_pred": noise_pred, "noise": noise, "timesteps": timesteps}
            if getattr(self.scheduler.config, "prediction_type", "epsilon") == "v_prediction":
                out["target"] = self.scheduler.get_velocity(normal_light, noise, timesteps)
            return out
        return noise_pred

    # ------------------------------------------------------------------ inference loop (:177-248)
    @torch.no_grad()
    def enhance(self, low_light: torch.Tensor, num_inference_steps: Optional[int] = None,
                generator: Optional[torch.Generator] = None, return_intermediate: bool = False, *,
                noise: Optional[Union[torch.Tensor, Sequence[torch.Tensor]]] = None,
                return_noise_pred: bool = False, sampler: str = "lcm", guidance_scale: Optional[float] = None,
                guidance_rescale: Optional[float] = None,
                _passes: Optional[int] = None) -> Union[torch.Tensor, LowLightDiffusionOutput]:
        """low_light [B,3,S,S] in [-1,1] -> enhanced [B,3,S,S].

        sampler="lcm" (the default) is the reference's loop: predict x0, re-noise with a fresh draw -- the sampler of a
        consistency student.  sampler="ddim" (extension; ddim.py has the definition) is the deterministic DDIM loop (eta = 0)
        of a many-step epsilon- or v-prediction model: `num_inference_steps` may be anything in 1..num_train_timesteps (the
        grid t_i = (n-1-i) * (T // n)), the initial latents are the only draw -- `generator` seeds it, and with one the global
        generator is not touched -- and `noise=` is [1,B,3,S,S] or a one-element list.  Any other string is a ValueError, and so
        is DDIM with a scheduler that clamps x0 (LCMDenoisingLoop).  sampler="dpmpp_2m" (extension; dpm.py has the definition) is
        DPM-Solver++ 2M for the same models: a second-order multistep solver on a grid uniform in log-SNR, with the same number of
        network calls per step count, the same first timestep, the same single draw and the same `noise=` shape as DDIM.  The
        table's spacing in log-SNR bounds its step count (32 for the default table; `dpm_schedule` raises ValueError past it,
        naming the limit).  Its step is one more elementwise launch per step in every compute dtype (llie_dpm_step).

        Noise: by default drawn on the device in the reference's order -- the initial latents with
        `generator` (:208-211), then one draw per non-final step from the global generator
        (lcm_scheduler.py:237).  `noise=` (extension) supplies those draws, e.g. CPU-generated ones for
        a bit-comparable run against the CPU reference: a [steps,B,3,S,S] tensor or a list of `steps`
        tensors (entries after the first are the re-noising draws of steps 0..steps-2).

        Classifier-free guidance (extension; guidance.py has the definitions): `guidance_scale=w`, any finite number other than
        1.0, replaces the network output of every step by o_u + w (o_c - o_u), o_c the output on `low_light` and o_u the one on
        the null condition (the all-zero image) -- for a model trained with `cond_dropout`.  None and 1.0 run the path above
        unchanged: the captured loop, the same bits, no second forward.  The guided loop is driven from the host: per step
        llie_guidance_pair, one denoiser pass over 2B rows (rows b and b + B are the two outputs of image b), llie_guide, the
        scheduler's step kernel with the step's coefficients (llie_dpm_step and one history tensor for "dpmpp_2m"), and the final
        clamp; nothing in it allocates, waits for the device or copies from the host.  Where the engine refuses 2B rows (llie_frame_shape_ok, workspace) the two outputs come from two
        B-row passes instead, with the same bits (every kernel is bitwise batch-invariant).  Draws, `noise=` shapes,
        `generator`, `return_intermediate` and `sampler` are those of the unguided call; `return_noise_pred` returns the guided
        output of each step.  A non-finite scale is a ValueError.

        `guidance_rescale=phi` (extension; Lin et al. 2024, section 3.4; `guidance.guide_rescale_host` has the definition): guidance
        at a useful scale inflates the standard deviation of the guided output, which the zero-terminal-SNR table hands to x0 as
        over-exposure.  With phi in (0, 1] the guided output of each image and step is scaled by phi std(o_c) / std(o) + (1 - phi),
        the standard deviations taken over the image's whole C H W: llie_guide_rescale (moments, factor, apply) takes llie_guide's
        place in the loop, two more launches per step; `return_noise_pred` returns the rescaled output.  0.7 is the paper's value;
        None and 0.0 are the guided loop above, bit for bit.  With guidance off the rescale is the identity by definition (o = o_c),
        so the unguided path runs unchanged; a phi outside [0, 1] is a ValueError either way."""
        check_sampler(sampler)
        G.check_guidance_scale(guidance_scale)
        G.check_guidance_rescale(guidance_rescale)
        device = low_light.device
        if device.type != "cuda":
            raise RuntimeError("LowLightDiffusion.enhance runs only on a HIP device; there is no CPU fallback")
        s = self.image_size
        if tuple(low_light.shape[1:]) != (3, s, s):
            raise ValueError(f"low_light must be [B,3,{s},{s}] (latents are allocated at image_size, "
                             f"low_light_diffusion.py:208-210); got {tuple(low_light.shape)}")
        return self._enhance_at(low_light, None, num_inference_steps, generator, return_intermediate, noise, return_noise_pred, sampler,
                                guidance_scale, _passes, guidance_rescale)

    @torch.no_grad()
    def enhance_frame(self, low_light: torch.Tensor, num_inference_steps: Optional[int] = None,
                      generator: Optional[torch.Generator] = None, return_intermediate: bool = False, *,
                      noise: Optional[Union[torch.Tensor, Sequence[torch.Tensor]]] = None,
                      return_noise_pred: bool = False, sampler: str = "lcm", guidance_scale: Optional[float] = None,
                      guidance_rescale: Optional[float] = None,
                      _passes: Optional[int] = None) -> Union[torch.Tensor, LowLightDiffusionOutput]:
        """Frame mode (extension): low_light [B,3,H,W] in [-1,1] -> enhanced [B,3,H,W], the whole loop (`sampler`: as in
        `enhance`) at the frame's own size.  The module tree is the one `image_size` fixed (attention placement, state_dict); the
        network is fully convolutional and its attention linear in the pixel count, so it runs at any H x W the engine's frame rule
        accepts (llie_frame_shape_ok): H and W multiples of 8 and at least 64, B <= 65535, and B*H*W times the widest full-resolution
        channel count at most 2^31 - 1 (about 5.59 M pixels per call for `small`).  A frame that breaks a rule raises
        ValueError naming it; frames past the size cap go through `enhance_tiled`.

        Semantics, noise order and outputs are `enhance`'s, with [steps,B,3,H,W] noise ([1,B,3,H,W] for DDIM); on an S x S input the
        result is `enhance`'s, bit for bit.  `guidance_scale` and `guidance_rescale`: as in `enhance` (the rescale's statistic is
        over the whole frame); a frame whose 2B rows break the frame rule runs the two-pass form.  Inference only."""
        check_sampler(sampler)
        G.check_guidance_scale(guidance_scale)
        G.check_guidance_rescale(guidance_rescale)
        device = low_light.device
        if device.type != "cuda":
            raise RuntimeError("LowLightDiffusion.enhance_frame runs only on a HIP device; there is no CPU fallback")
        if low_light.dim() != 4 or low_light.shape[1] != 3:
            raise ValueError(f"low_light must be [B,3,H,W]; got {tuple(low_light.shape)}")
        return self._enhance_at(low_light, (int(low_light.shape[2]), int(low_light.shape[3])), num_inference_steps, generator,
                                return_intermediate, noise, return_noise_pred, sampler, guidance_scale, _passes, guidance_rescale)

    def ddim_schedule(self, num_inference_steps: Optional[int] = None) -> Tuple[List[int], List[N.StepCoef]]:
        """(timesteps, one N.StepCoef each) of the DDIM loop of `num_inference_steps` steps (default: self.num_inference_steps).
        ValueError for a step count outside 1..num_train_timesteps, a first timestep whose alpha-bar is 0 under epsilon
        prediction, and a scheduler without the DDIM step (LCMDenoisingLoop clamps x0, which DDIM does not define)."""
        n = self.num_inference_steps if num_inference_steps is None else num_inference_steps
        if not isinstance(self.scheduler, LCMScheduler):
            raise ValueError(f'sampler="ddim" is not defined for {type(self.scheduler).__name__} (the deployment loop clamps x0); '
                             f"use an LCMScheduler")
        ts = self.scheduler.ddim_timesteps(n)
        c = int(self.scheduler.config.num_train_timesteps) // len(ts)
        return ts, [self.scheduler.ddim_step_coefficients(t, t - c) for t in ts]

    def dpm_schedule(self, num_inference_steps: Optional[int] = None) -> Tuple[List[int], List[N.DpmCoef]]:
        """(timesteps, one N.DpmCoef each) of the DPM-Solver++ 2M loop of `num_inference_steps` steps (default:
        self.num_inference_steps): dpm.dpm_timesteps / dpm.dpm_step_coefficients on the scheduler's table, each float64 scalar
        rounded once to fp32.  ValueError for a step count the grid refuses (not an integer, < 1, more than the table's spacing in
        log-SNR allows, a first timestep whose alpha-bar is 0) and a scheduler that clamps x0 (LCMDenoisingLoop), as `ddim_schedule`."""
        n = self.num_inference_steps if num_inference_steps is None else num_inference_steps
        if not isinstance(self.scheduler, LCMScheduler):
            raise ValueError(f'sampler="dpmpp_2m" is not defined for {type(self.scheduler).__name__} (the deployment loop clamps x0); '
                             f"use an LCMScheduler")
        acp = self.scheduler.alphas_cumprod.detach().cpu().numpy()
        ts = DPM.dpm_timesteps(n, acp)
        recs = DPM.dpm_step_coefficients(ts, acp, self.scheduler._ptype() == "v_prediction")
        return ts, [N.DpmCoef(r.sqrt_alpha_t, r.sqrt_beta_t, r.k_x, r.k_0, r.k_1, r.v_prediction, r.order, r.is_last) for r in recs]

    def _enhance_at(self, low_light, frame, num_inference_steps, generator, return_intermediate, noise, return_noise_pred,
                    sampler="lcm", guidance_scale=None, passes=None, guidance_rescale=None):
        """The loop of `enhance` (frame is None: image_size, llie_enhance) and `enhance_frame` (frame = (H, W), llie_enhance_hw);
        with a `guidance_scale` other than None / 1.0, the host-driven guided loop (`_guided_loop`) after the same setup."""
        guided = G.guidance_is_on(guidance_scale)
        phi = G.check_guidance_rescale(guidance_rescale)
        if passes not in (None, 1, 2):
            raise ValueError(f"_passes must be None, 1 or 2, got {passes!r}")
        device = low_light.device
        b = low_light.shape[0]
        hh, ww = frame if frame is not None else (self.image_size, self.image_size)
        steps = self.num_inference_steps if num_inference_steps is None else num_inference_steps
        dpm = sampler == "dpmpp_2m"
        ddim = sampler == "ddim" or dpm  # one draw, no staged noise past it: what the two many-step samplers share
        if dpm:
            ts, coef_list = self.dpm_schedule(steps)
        elif ddim:
            ts, coef_list = self.ddim_schedule(steps)
        else:
            self.scheduler.set_timesteps(steps, device=device)
            ts = self.scheduler._timestep_list
        steps = len(ts)
        draws = 1 if ddim else steps  # DDIM, DPM-Solver++: the initial latents are the only noise
        # the staging area of the engine's captured loop: LCM stages one draw per step; the others stage none past the first, so only
        # the per-step outputs a caller asks for make it grow with the step count
        stage_steps = 8 if ddim and not (return_intermediate or return_noise_pred) else max(steps, 8)
        prepared = None
        if guided:
            passes = self._guided_plan(b, device, frame, passes)  # a refused frame raises here, before any draw or launch
        elif frame is not None:
            try:  # the workspace query applies the frame rule: a refused frame raises before any draw or launch
                prepared = self.unet._prepare(b, device, enhance_steps=stage_steps, frame=frame)
            except ValueError as e:
                hint = '; enhance_tiled(tile="auto") handles images of any size' if "element cap" in str(e) else ""
                raise ValueError(f"enhance_frame: {e}{hint}") from None

        if noise is None:
            # drawn straight into the [steps,B,3,S,S] buffer the engine reads (same generator streams as torch.randn)
            noise_t = torch.empty(draws, b, 3, hh, ww, dtype=torch.float32, device=device)
            noise_t[0].normal_(generator=generator)
            for i in range(1, draws):
                noise_t[i].normal_()
        else:
            noise_t = supplied_noise(noise, draws, b, hh, ww, device, sampler)
        noise_t = noise_t.contiguous()

        coefs = (N.DpmCoef * steps)(*coef_list) if dpm else \
            (N.StepCoef * steps)(*(coef_list if ddim else [self.scheduler.step_coefficients(t) for t in ts]))
        tkey = (tuple(ts), b, device.type, device.index)
        t_dev = self._t_cache.get(tkey)  # [steps*B] device timesteps: one H2D copy per (schedule, batch), not per call
        if t_dev is None:
            if len(self._t_cache) > 64:
                self._t_cache.clear()
            t_dev = self._t_cache[tkey] = torch.tensor(ts, dtype=torch.long).repeat_interleave(b).to(device)
        low = low_light.detach().float().contiguous()
        enhanced = torch.empty(b, 3, hh, ww, dtype=torch.float32, device=device)
        inter = torch.empty(steps, b, 3, hh, ww, dtype=torch.float32, device=device) if return_intermediate else None
        preds = torch.empty(steps, b, 3, hh, ww, dtype=torch.float32, device=device) if return_noise_pred else None
        if guided:
            self._guided_loop(low, noise_t, ts, coefs, float(guidance_scale), passes, frame is not None, enhanced, inter, preds, phi)
            return self._enhance_result(enhanced, inter, preds, steps, return_intermediate or return_noise_pred)
        h, ws, nbytes = prepared if prepared is not None else self.unet._prepare(b, device, enhance_steps=stage_steps)
        outs = (enhanced.data_ptr(), inter.data_ptr() if inter is not None else None, preds.data_ptr() if preds is not None else None)
        stream = torch.cuda.current_stream(device).cuda_stream
        with torch.cuda.device(device):
            if dpm and frame is None:
                N.check(N.lib().llie_enhance_dpm(h.h, low.data_ptr(), noise_t.data_ptr(), t_dev.data_ptr(), coefs, steps, *outs,
                                                 b, ws.data_ptr(), nbytes, stream), "enhance")
            elif dpm:
                N.check(N.lib().llie_enhance_dpm_hw(h.h, low.data_ptr(), noise_t.data_ptr(), t_dev.data_ptr(), coefs, steps, *outs,
                                                    b, hh, ww, ws.data_ptr(), nbytes, stream), "enhance_frame")
            elif frame is None:
                N.check(N.lib().llie_enhance(h.h, low.data_ptr(), noise_t.data_ptr(), t_dev.data_ptr(), coefs, steps, *outs,
                                             b, ws.data_ptr(), nbytes, stream), "enhance")
            else:
                N.check(N.lib().llie_enhance_hw(h.h, low.data_ptr(), noise_t.data_ptr(), t_dev.data_ptr(), coefs, steps, *outs,
                                                b, hh, ww, ws.data_ptr(), nbytes, stream), "enhance_frame")
        return self._enhance_result(enhanced, inter, preds, steps, return_intermediate or return_noise_pred)

    def _enhance_result(self, enhanced, inter, preds, steps, as_output):
        self.scheduler._step_index = steps
        if as_output:
            out = LowLightDiffusionOutput(enhanced=enhanced,
                                          intermediate=[inter[i] for i in range(steps)] if inter is not None else None)
            if preds is not None:
                out.noise_pred = [preds[i] for i in range(steps)]
            return out
        return enhanced

    def _guided_plan(self, b: int, device, frame, passes: Optional[int]) -> int:
        """The form of the guided loop: 1 (one 2B-row pass per step, the default) or 2 (two B-row passes), after the engine's
        shape and workspace queries.  B rows refused: ValueError naming the rule, as the unguided call raises.  2B rows refused
        (the frame rule or the workspace query): the two-pass form, unless `passes` forces one pass -- then that refusal."""
        from .unet import resolve_compute_dtype
        h = self.unet._handle(resolve_compute_dtype(self.unet.compute_dtype))
        try:
            h.workspace_bytes(b) if frame is None else h.frame_workspace_bytes(b, frame[0], frame[1])
        except ValueError as e:
            hint = '; enhance_tiled(tile="auto") handles images of any size' if "element cap" in str(e) else ""
            raise ValueError(f"enhance_frame: {e}{hint}" if frame is not None else str(e)) from None
        if passes == 2:
            return 2
        try:
            self.unet._prepare(2 * b, device, frame=frame)
        except (ValueError, torch.cuda.OutOfMemoryError):
            if passes == 1:
                raise
            return 2
        return 1

    def _guided_loop(self, low, noise_t, ts, coefs, w: float, passes: int, frames: bool, enhanced, inter, preds, phi: float = 0.0) -> None:
        """The guided loop after `_enhance_at`'s setup (the docstring of `enhance` has the steps).  Buffers are allocated before
        the loop; inside it there are only launches on the current stream.  `phi` > 0: llie_guide_rescale in llie_guide's place."""
        device = low.device
        b = low.shape[0]
        rows = 2 * b if passes == 1 else b
        t_dev = []
        for t in ts:  # device timesteps, kept on the model like the tiles path's
            key = ("guided", int(t), rows, device.type, device.index)
            cached = self._t_cache.get(key)
            if cached is None:
                if len(self._t_cache) > 64:
                    self._t_cache.clear()
                cached = self._t_cache[key] = torch.full((rows,), int(t), dtype=torch.long).to(device)
            t_dev.append(cached)
        out2 = torch.empty((2 * b,) + tuple(low.shape[1:]), dtype=torch.float32, device=device)  # rows b: o_c, rows b + B: o_u
        o_c, o_u = out2[:b], out2[b:]
        if passes == 1:
            lat2, cond2 = torch.empty_like(out2), torch.empty_like(out2)
        else:
            null = torch.zeros_like(low)
        guided = None if preds is not None else torch.empty_like(low)
        lat = None if inter is not None else (torch.empty_like(low), torch.empty_like(low))
        dpm = isinstance(coefs[0], N.DpmCoef)
        hist = torch.empty_like(low) if dpm else None  # DPM-Solver++: the previous step's x0
        x = noise_t[0]
        n = low.numel()
        if phi > 0:
            scratch = G.guide_rescale_scratch(b, n // b, device)
            factor = torch.empty(b, dtype=torch.float32, device=device)
        steps = len(ts)
        L = N.lib()
        with torch.cuda.device(device):
            stream = torch.cuda.current_stream(device).cuda_stream
            for i in range(steps):
                if passes == 1:
                    G.guidance_pair_device(x, low, lat2, cond2)
                    self.unet.forward_split(lat2, cond2, t_dev[i], uniform_t=True, out=out2, frame=frames)
                else:
                    self.unet.forward_split(x, low, t_dev[i], uniform_t=True, out=o_c, frame=frames)
                    self.unet.forward_split(x, null, t_dev[i], uniform_t=True, out=o_u, frame=frames)
                o = preds[i] if preds is not None else guided
                if phi > 0:
                    N.check(L.llie_guide_rescale(o_c.data_ptr(), o_u.data_ptr(), None, w, phi, o.data_ptr(), factor.data_ptr(),
                                                 scratch.data_ptr(), scratch.numel(), b, n // b, stream), "enhance (guided)")
                else:
                    N.check(L.llie_guide(o_c.data_ptr(), o_u.data_ptr(), None, w, o.data_ptr(), b, n // b, stream), "enhance (guided)")
                last = i == steps - 1
                prev = inter[i] if inter is not None else lat[i & 1]
                if dpm:
                    N.check(L.llie_dpm_step(o.data_ptr(), x.data_ptr(), hist.data_ptr(), prev.data_ptr(), enhanced.data_ptr() if last else None,
                                            n, coefs[i], stream), "enhance (guided)")
                    x = prev
                    continue
                draw = not coefs[i].is_last and not coefs[i].sampler  # a DDIM step reads no noise
                N.check(L.llie_lcm_step(o.data_ptr(), x.data_ptr(), noise_t[i + 1].data_ptr() if draw else None, prev.data_ptr(), None,
                                        enhanced.data_ptr() if last else None, n, coefs[i], stream), "enhance (guided)")
                x = prev

    # ------------------------------------------------------------------ loss (:250-277)
    def compute_loss(self, low_light: torch.Tensor, normal_light: torch.Tensor, loss_type: str = "mse", *,
                     use_velocity_target: bool = False, x0_ssim_weight: float = 0.0, x0_l1_weight: float = 0.0,
                     cond_dropout: float = 0.0, snr_gamma: Optional[float] = None) -> torch.Tensor:
        """Regresses the denoiser output against the drawn noise, as the reference does whatever the scheduler's
        prediction type (low_light_diffusion.py:262-275).  `use_velocity_target=True` (extension, needs a
        `prediction_type="v_prediction"` scheduler) regresses against `scheduler.get_velocity` instead -- the v-pred MSE of
        BASELINE config 5, which the reference defines (lcm_scheduler.py:282-305) but never wires into its loss.
        `x0_ssim_weight` / `x0_l1_weight` (extension): when either is non-zero, `x0_loss` of the predicted clean image against
        `normal_light` is added (the module docstring has the definition); with both 0 nothing changes.
        The loss and the x0 term run at the batch's own H x W: [B,3,H,W] of any shape llie_train_shape_ok accepts (frame-size
        fine-tuning; image_size is one such shape and is what it was).
        `loss.backward()` also fills the gradient of a `low_light` that requires one (forward's docstring): `compute_loss(frontend(raw),
        normal)` trains `frontend` together with, or instead of, the denoiser.
        `cond_dropout=p`: `forward`'s condition dropout (one more draw, `torch.rand(B)`, after the timestep and noise draws, only
        when p > 0) -- what TrainStep(cond_dropout=p) does without autograd.
        `snr_gamma=g` (extension; finite, > 0; None = off): Min-SNR-gamma weighting of the noise-space loss (snrloss.py has the
        definition): the loss becomes (1 / B) sum_b w_b m_b with w_b from `use_velocity_target`, computed with its gradient by
        one call of llie_snr_loss inside one autograd node, the x0 term (not multiplied by w) added into the same gradient
        buffer -- the loss and d(loss)/d(pred) bits of TrainStep(snr_gamma=g).  With None nothing changes."""
        _check_x0_weights(x0_ssim_weight, x0_l1_weight)
        snr_gamma = check_snr_gamma(snr_gamma)
        if loss_type not in ("mse", "huber", "l1") and snr_gamma is not None:
            raise ValueError(f"Unknown loss type: {loss_type}")
        out = self.forward(low_light, normal_light, frame=True, **({"cond_dropout": cond_dropout} if cond_dropout != 0 else {}))
        if use_velocity_target and "target" not in out:
            raise ValueError("use_velocity_target needs a scheduler with prediction_type='v_prediction'")
        pred, noise = out["noise_pred"], (out["target"] if use_velocity_target else out["noise"])
        if snr_gamma is not None:
            x0_on = x0_ssim_weight != 0 or x0_l1_weight != 0
            noisy = self.scheduler.add_noise(normal_light, out["noise"], out["timesteps"]) if x0_on else None  # forward's x_t
            return _SnrLossFn.apply(pred, noise, self.scheduler, noisy, normal_light, out["timesteps"], loss_type,
                                    bool(use_velocity_target), snr_gamma, float(x0_ssim_weight), float(x0_l1_weight))
        if loss_type == "mse":
            loss = F.mse_loss(pred, noise)
        elif loss_type == "huber":
            loss = F.huber_loss(pred, noise)
        elif loss_type == "l1":
            loss = F.l1_loss(pred, noise)
        else:
            raise ValueError(f"Unknown loss type: {loss_type}")
        if x0_ssim_weight != 0 or x0_l1_weight != 0:
            # one node for the base loss and the term, formed as TrainStep forms them: the same loss and d(loss)/d(pred) bits
            noisy = self.scheduler.add_noise(normal_light, out["noise"], out["timesteps"])  # forward's x_t, the same bits
            loss = _LossWithX0Fn.apply(pred, noise, self.scheduler, noisy, normal_light, out["timesteps"], loss_type,
                                       bool(use_velocity_target), float(x0_ssim_weight), float(x0_l1_weight))
        return loss

    def get_model_size(self) -> Dict[str, float]:
        return self.unet.get_memory_footprint()


# ---------------------------------------------------------------------- condition dropout (guidance.py)
def cond_uniforms(cond_u: Optional[torch.Tensor], batch: int, device) -> torch.Tensor:
    """The uniforms of a condition-dropout call as contiguous fp32 [B] on `device`: `cond_u` when supplied (ValueError for another
    shape), else `torch.rand(B, device=device)` from the global device generator."""
    if cond_u is None:
        return torch.rand(batch, device=device)
    u = torch.as_tensor(cond_u)
    if tuple(u.shape) != (batch,):
        raise ValueError(f"cond_u must be [{batch}], got {list(u.shape)}")
    return u.to(device=device, dtype=torch.float32).contiguous()


class _CondDropoutFn(torch.autograd.Function):
    """llie_cond_dropout as an autograd node of the condition: forward selects the null condition for rows with u < p, backward
    runs the same select on the gradient, so dropped rows receive exactly 0."""

    @staticmethod
    def forward(ctx, cond, u, p):
        ctx.save_for_backward(u)
        ctx.p = p
        return G.cond_dropout_device(cond.detach().float().contiguous(), u, p)

    @staticmethod
    def backward(ctx, grad_output):
        u, = ctx.saved_tensors
        return G.cond_dropout_device(grad_output.detach().float().contiguous(), u, ctx.p), None, None


# ---------------------------------------------------------------------- consistency distillation (:284-408)
def _require_hip(t: torch.Tensor, what: str) -> None:
    if t.device.type != "cuda":
        raise RuntimeError(f"{what} runs only on a HIP device (got '{t.device}'); there is no CPU fallback")


PREDICTION_TYPES = ("epsilon", "v_prediction")


def prediction_code(prediction_type: str, who: str = "prediction_type") -> int:
    """"epsilon" / "v_prediction" -> N.PRED_EPSILON / N.PRED_V; ValueError for anything else."""
    if prediction_type not in PREDICTION_TYPES:
        raise ValueError(f"{who} must be one of {PREDICTION_TYPES}, got {prediction_type!r}")
    return N.PRED_V if prediction_type == "v_prediction" else N.PRED_EPSILON


def consistency_target(scheduler: LCMScheduler, x_t: torch.Tensor, e_teacher: torch.Tensor, t: torch.Tensor,
                       t_next: torch.Tensor, *, prediction_type: str = "epsilon") -> torch.Tensor:
    """The teacher's DDIM step t -> t_next (:365-376): x_next = sqrt(a_n) x0 + sqrt(1-a_n) e^, with (x0, e^) what the teacher's
    output means at (x_t, a_t) under `prediction_type` (epsilon: x0 = (x_t - sqrt(1-a_t) o) / sqrt(a_t), e^ = o; v_prediction:
    x0 = sqrt(a_t) x_t - sqrt(1-a_t) o, e^ = sqrt(1-a_t) x_t + sqrt(a_t) o), a from `scheduler`'s alpha-bar table; t / t_next
    device int64 [B] (llie_consistency_target_ex).  Any [B, ...] shape: the kernel sees B rows of numel / B elements."""
    _require_hip(x_t, "consistency_target")
    pred = prediction_code(prediction_type)
    dev = x_t.device
    x_t, e_teacher = x_t.detach().float().contiguous(), e_teacher.detach().float().contiguous()
    acp = scheduler._acp_on(dev)
    b = x_t.shape[0]
    out = torch.empty_like(x_t)
    with torch.cuda.device(dev):
        N.check(N.lib().llie_consistency_target_ex(x_t.data_ptr(), e_teacher.data_ptr(), t.data_ptr(), t_next.data_ptr(), acp.data_ptr(),
                                                   acp.numel(), out.data_ptr(), b, x_t.numel() // b, pred,
                                                   torch.cuda.current_stream(dev).cuda_stream), "consistency_target")
    return out


def consistency_loss(scheduler: LCMScheduler, x_t: torch.Tensor, x_next: torch.Tensor, e_student: torch.Tensor, e_ema: torch.Tensor,
                     t: torch.Tensor, t_next: torch.Tensor, *, prediction_type: str = "epsilon") -> Tuple[torch.Tensor, torch.Tensor]:
    """F.huber_loss(s0, g0) of :385-393 and its gradient with respect to the student's prediction (llie_consistency_loss_ex):
    -> (loss, a 0-d device tensor; d(loss)/d(e_student), shaped like it).  `prediction_type` is how the student's and the EMA
    student's outputs are read (s0 = x0 of e_student at (x_t, a_t), g0 = x0 of e_ema at (x_next, a_n); consistency_target)."""
    _require_hip(x_t, "consistency_loss")
    pred = prediction_code(prediction_type)
    dev = x_t.device
    x_t, x_next = x_t.detach().float().contiguous(), x_next.detach().float().contiguous()
    e_student, e_ema = e_student.detach().float().contiguous(), e_ema.detach().float().contiguous()
    acp = scheduler._acp_on(dev)
    b, n = x_t.shape[0], x_t.numel()
    d = torch.empty_like(x_t)
    loss = torch.empty((), dtype=torch.float32, device=dev)
    nbytes = N.distill_scratch_bytes(n)
    scratch = torch.empty(nbytes, dtype=torch.uint8, device=dev)
    with torch.cuda.device(dev):
        N.check(N.lib().llie_consistency_loss_ex(x_t.data_ptr(), x_next.data_ptr(), e_student.data_ptr(), e_ema.data_ptr(), t.data_ptr(),
                                                 t_next.data_ptr(), acp.data_ptr(), acp.numel(), d.data_ptr(), loss.data_ptr(),
                                                 scratch.data_ptr(), nbytes, b, n // b, pred,
                                                 torch.cuda.current_stream(dev).cuda_stream), "consistency_loss")
    return loss, d


class _ConsistencyLossFn(torch.autograd.Function):
    """The Huber consistency loss as an autograd node of the student's prediction: forward = llie_consistency_loss_ex, backward =
    the gradient it wrote times grad_output (so GradScaler's scaled backward works)."""

    @staticmethod
    def forward(ctx, e_student, scheduler, x_t, x_next, e_ema, t, t_next, prediction_type="epsilon"):
        loss, d = consistency_loss(scheduler, x_t, x_next, e_student, e_ema, t, t_next, prediction_type=prediction_type)
        ctx.save_for_backward(d)
        return loss

    @staticmethod
    def backward(ctx, grad_output):
        d, = ctx.saved_tensors
        return (d * grad_output,) + (None,) * 7


def _distill_x0(x: np.ndarray, o: np.ndarray, a: np.ndarray, v: bool) -> np.ndarray:
    sa, sb = np.sqrt(a), np.sqrt(1.0 - a)
    with np.errstate(divide="ignore", invalid="ignore", over="ignore"):
        return sa * x - sb * o if v else (x - sb * o) / sa


def _distill_host_args(arrays, acps):
    arrays = [np.asarray(v, dtype=np.float64) for v in arrays]
    shape = arrays[0].shape
    if len(shape) < 2 or any(v.shape != shape for v in arrays):
        raise ValueError(f"the tensors must share one [B, ...] shape, got {[v.shape for v in arrays]}")
    acps = [np.asarray(a, dtype=np.float64).reshape(-1) for a in acps]
    if any(a.shape[0] != shape[0] for a in acps):
        raise ValueError(f"alpha-bar arrays must be [{shape[0]}], got {[a.shape for a in acps]}")
    return arrays, [a.reshape((-1,) + (1,) * (len(shape) - 1)) for a in acps]


def consistency_target_host(x_t, out_teacher, acp_t, acp_next, *, prediction_type: str = "epsilon") -> np.ndarray:
    """The definition of `consistency_target` in float64 NumPy: x_t / out_teacher [B, ...], acp_t / acp_next [B] =
    alphas_cumprod[t_b] / alphas_cumprod[t_next_b] (NaN for a timestep outside the table: that sample is NaN) -> x_next.
    At acp_t == 0 the epsilon form divides by zero (inf / NaN, as the kernel); the v form is finite."""
    v = prediction_code(prediction_type) == N.PRED_V
    (x, o), (a, an) = _distill_host_args((x_t, out_teacher), (acp_t, acp_next))
    sa, sb = np.sqrt(a), np.sqrt(1.0 - a)
    x0 = _distill_x0(x, o, a, v)
    eps = sb * x + sa * o if v else o
    with np.errstate(invalid="ignore", over="ignore"):
        return np.sqrt(an) * x0 + np.sqrt(1.0 - an) * eps


def consistency_loss_host(x_t, x_next, out_student, out_ema, acp_t, acp_next, *, prediction_type: str = "epsilon",
                          return_x0: bool = False):
    """The definition of `consistency_loss` in float64 NumPy -> (loss, d loss / d out_student): s0 = x0 of out_student at
    (x_t, acp_t), g0 = x0 of out_ema at (x_next, acp_next), both read as `prediction_type`; loss = mean huber(s0 - g0), delta 1;
    gradient = clamp(s0 - g0, -1, 1) / n * q, q = -sqrt(1 - acp_t) / sqrt(acp_t) (epsilon) or -sqrt(1 - acp_t) (v_prediction).
    `return_x0=True` appends (s0, g0).  inf / NaN follow IEEE arithmetic, as in the kernel."""
    v = prediction_code(prediction_type) == N.PRED_V
    (x, xn, os_, oe), (a, an) = _distill_host_args((x_t, x_next, out_student, out_ema), (acp_t, acp_next))
    s0, g0 = _distill_x0(x, os_, a, v), _distill_x0(xn, oe, an, v)
    with np.errstate(divide="ignore", invalid="ignore", over="ignore"):
        diff = s0 - g0
        z = np.abs(diff)
        loss = float(np.where(z < 1.0, 0.5 * z * z, z - 0.5).mean())
        c = np.where(diff <= -1.0, -1.0, np.where(diff >= 1.0, 1.0, diff))  # NaN falls through, as huber_loss_backward
        q = -np.sqrt(1.0 - a) if v else -np.sqrt(1.0 - a) / np.sqrt(a)
        grad = c / diff.size * q
    return (loss, grad, s0, g0) if return_x0 else (loss, grad)


# ---------------------------------------------------------------------- the x0 term (module docstring)
def _check_x0_weights(ssim_weight: float, l1_weight: float) -> None:
    if not (ssim_weight >= 0 and l1_weight >= 0) or ssim_weight == float("inf") or l1_weight == float("inf"):
        raise ValueError(f"x0_ssim_weight and x0_l1_weight must be finite and >= 0, got {ssim_weight} and {l1_weight}")


def x0_term_eval(out: np.ndarray, x_t: np.ndarray, y: np.ndarray, acp: np.ndarray, velocity: bool, ssim_weight: float,
                 l1_weight: float) -> Tuple[float, np.ndarray]:
    """The formulas of the module docstring in the dtype of `out` (float64 for `x0_loss_host`; the tests evaluate them in
    float32 to size the device's rounding) -> (term, d term / d out)."""
    from .metrics import ssim_grad_mapped
    t = out.dtype.type
    batch = out.shape[0]
    grad = np.zeros_like(out)
    term = t(0)
    ws, w1 = t(ssim_weight), t(l1_weight)
    for b in range(batch):
        a = t(acp[b])
        if a == 0:
            continue
        alpha, sigma = np.sqrt(a), np.sqrt(t(1) - a)
        p, q = (alpha, -sigma) if velocity else (t(1) / alpha, -sigma / alpha)
        xh, yb = p * x_t[b:b + 1] + q * out[b:b + 1], y[b:b + 1]
        ssim, dx = ssim_grad_mapped((xh + t(1)) / t(2), (yb + t(1)) / t(2))
        d = xh - yb
        term = term + a * (ws * (t(1) - ssim[0]) + w1 * np.abs(d).mean(dtype=out.dtype))
        grad[b] = (a / t(batch)) * q * (-ws * (dx[0] / t(2)) + w1 * (np.sign(d[0]) / t(d[0].size)))
    return term / t(batch), grad


def x0_loss_host(out, x_t, normal, acp_t, velocity: bool, ssim_weight: float, l1_weight: float) -> Tuple[float, np.ndarray]:
    """The definition of the x0 term in float64 NumPy: out / x_t / normal [B,3,H,W], acp_t [B] = alphas_cumprod[t_b] ->
    (term, d term / d out [B,3,H,W]).  A sample with acp_t == 0 contributes exactly 0 to both.  ValueError for negative weights,
    mismatched shapes and images below 11 x 11."""
    _check_x0_weights(ssim_weight, l1_weight)
    out, x_t, y = (np.asarray(v, dtype=np.float64) for v in (out, x_t, normal))
    acp = np.asarray(acp_t, dtype=np.float64).reshape(-1)
    if out.ndim != 4 or out.shape[1] != 3 or x_t.shape != out.shape or y.shape != out.shape or acp.shape[0] != out.shape[0]:
        raise ValueError(f"out / x_t / normal must be [B,3,H,W] and acp_t [B], got {out.shape}, {x_t.shape}, {y.shape}, {acp.shape}")
    if out.shape[2] < 11 or out.shape[3] < 11:
        raise ValueError(f"images must be at least 11 x 11 (one window), got {out.shape[2]} x {out.shape[3]}")
    if ssim_weight == 0 and l1_weight == 0:
        return 0.0, np.zeros_like(out)
    term, grad = x0_term_eval(out, x_t, y, acp, velocity, ssim_weight, l1_weight)
    return float(term), grad


def x0_loss_device(scheduler: LCMScheduler, out: torch.Tensor, x_t: torch.Tensor, normal: torch.Tensor, timesteps: torch.Tensor,
                   velocity: bool, ssim_weight: float, l1_weight: float, d_out: Optional[torch.Tensor] = None) -> torch.Tensor:
    """llie_x0_loss: the term as a 0-d fp32 device tensor; its gradient with respect to `out` is ADDED to `d_out` (fp32,
    contiguous, shaped like `out`) when one is given.  No synchronisation, no autograd."""
    _require_hip(out, "x0_loss")
    _check_x0_weights(ssim_weight, l1_weight)
    dev = out.device
    if out.dim() != 4 or out.shape[1] != 3 or x_t.shape != out.shape or normal.shape != out.shape or tuple(timesteps.shape) != (out.shape[0],):
        raise ValueError(f"out / x_t / normal must be [B,3,H,W] and timesteps [B], got {tuple(out.shape)}, {tuple(x_t.shape)}, "
                         f"{tuple(normal.shape)}, {tuple(timesteps.shape)}")
    acp = scheduler._acp_on(dev)
    if timesteps.device.type == "cpu" and timesteps.numel() and (int(timesteps.min()) < 0 or int(timesteps.max()) >= acp.numel()):
        # device-resident timesteps cannot be checked without a synchronisation: the kernels turn one outside the table into a NaN
        # loss and gradient for that sample instead of indexing with it (as LCMScheduler.add_noise does)
        raise ValueError(f"timesteps must lie in [0, {acp.numel()})")
    out, x_t, normal = (v.detach().to(device=dev, dtype=torch.float32).contiguous() for v in (out, x_t, normal))
    t = timesteps.to(device=dev, dtype=torch.long).contiguous()
    if d_out is not None and (d_out.dtype != torch.float32 or not d_out.is_contiguous() or d_out.shape != out.shape or d_out.device != dev):
        raise ValueError("d_out must be contiguous fp32, shaped like out, on its device")
    b, h, w = out.shape[0], out.shape[2], out.shape[3]
    L = N.lib()
    nbytes = int(L.llie_ssim_grad_scratch_bytes(b, h, w))
    if nbytes < 0:
        N.check(nbytes, f"x0_loss: {b} images of {h} x {w} (at least 1 image of 11 x 11)")
    scratch = torch.empty((nbytes + 7) // 8, dtype=torch.float64, device=dev)
    loss = torch.empty((), dtype=torch.float32, device=dev)
    with torch.cuda.device(dev):
        N.check(L.llie_x0_loss(out.data_ptr(), x_t.data_ptr(), normal.data_ptr(), t.data_ptr(), acp.data_ptr(), acp.numel(),
                               1 if velocity else 0, float(ssim_weight), float(l1_weight), loss.data_ptr(),
                               d_out.data_ptr() if d_out is not None else None, b, h, w, scratch.data_ptr(), nbytes,
                               torch.cuda.current_stream(dev).cuda_stream), "x0_loss")
    return loss


def base_loss_and_grad(pred: torch.Tensor, target: torch.Tensor, loss_type: str) -> Tuple[torch.Tensor, torch.Tensor]:
    """(loss, d(loss)/d(pred)) of F.mse_loss / F.l1_loss / F.huber_loss(delta=1), written out: what TrainStep hands the backward
    pass, and what compute_loss seeds the x0 term's gradient buffer with."""
    diff = pred - target
    n = diff.numel()
    if loss_type == "mse":          # mean(d^2); d/d pred = 2 d / n
        return (diff * diff).mean(), diff * (2.0 / n)
    if loss_type == "l1":           # mean|d|; sign(d) / n
        return diff.abs().mean(), torch.sign(diff) / n
    if loss_type == "huber":        # 0.5 d^2 inside, |d| - 0.5 outside; clamp(d, -1, 1) / n
        a = diff.abs()
        return torch.where(a < 1.0, 0.5 * diff * diff, a - 0.5).mean(), diff.clamp(-1.0, 1.0) / n
    raise ValueError(f"Unknown loss type: {loss_type}")


class _LossWithX0Fn(torch.autograd.Function):
    """compute_loss with the x0 term on, as one autograd node of the network output: the base loss's gradient is written first
    and llie_x0_loss adds the term's into it -- TrainStep's order of operations, so the two routes give the same loss and the
    same d(loss)/d(pred), bit for bit (two nodes summed by autograd round the term's product once more).  backward = that
    buffer times grad_output (a GradScaler's scaled backward works)."""

    @staticmethod
    def forward(ctx, pred, target, scheduler, x_t, normal, timesteps, loss_type, velocity, ssim_weight, l1_weight):
        out = pred.detach().float()
        loss, d = base_loss_and_grad(out, target, loss_type)
        d = d.contiguous()
        loss = loss + x0_loss_device(scheduler, out, x_t, normal, timesteps, velocity, ssim_weight, l1_weight, d)
        ctx.save_for_backward(d)
        return loss

    @staticmethod
    def backward(ctx, grad_output):
        d, = ctx.saved_tensors
        return (d * grad_output,) + (None,) * 9


class _SnrLossFn(torch.autograd.Function):
    """compute_loss with `snr_gamma` set, as one autograd node of the network output: llie_snr_loss stores the weighted loss's
    gradient into a buffer, then (x0 term on) llie_x0_loss adds the term's into it -- TrainStep's order of operations, so the
    two routes share the loss and d(loss)/d(pred) bits.  backward = that buffer times grad_output."""

    @staticmethod
    def forward(ctx, pred, target, scheduler, x_t, normal, timesteps, loss_type, velocity, gamma, ssim_weight, l1_weight):
        from .snrloss import snr_loss_device
        out = pred.detach().float().contiguous()
        d = torch.empty_like(out)
        loss, _, _ = snr_loss_device(scheduler, out, target, timesteps, loss_type, velocity, gamma, d)
        if ssim_weight != 0 or l1_weight != 0:
            loss = loss + x0_loss_device(scheduler, out, x_t, normal, timesteps, velocity, ssim_weight, l1_weight, d)
        else:
            loss = loss.clone()  # a view of the kernel's output block otherwise
        ctx.save_for_backward(d)
        return loss

    @staticmethod
    def backward(ctx, grad_output):
        d, = ctx.saved_tensors
        return (d * grad_output,) + (None,) * 10


class _X0LossFn(torch.autograd.Function):
    """The x0 term as an autograd node of the network output: forward = llie_x0_loss into a zeroed gradient buffer, backward =
    that buffer times grad_output (so a GradScaler's scaled backward works)."""

    @staticmethod
    def forward(ctx, out, scheduler, x_t, normal, timesteps, velocity, ssim_weight, l1_weight):
        d = torch.zeros(out.shape, dtype=torch.float32, device=out.device) if ctx.needs_input_grad[0] else None
        loss = x0_loss_device(scheduler, out, x_t, normal, timesteps, velocity, ssim_weight, l1_weight, d)
        if d is not None:
            ctx.save_for_backward(d)
        return loss

    @staticmethod
    def backward(ctx, grad_output):
        d, = ctx.saved_tensors
        return (d * grad_output,) + (None,) * 7


def x0_loss(model_or_scheduler, out: torch.Tensor, x_t: torch.Tensor, normal: torch.Tensor, timesteps: torch.Tensor, *,
            velocity: bool = False, ssim_weight: float, l1_weight: float) -> torch.Tensor:
    """The x0 term of the module docstring as a 0-d device tensor, differentiable with respect to `out` (the network output of
    `forward`; `x_t` is the noised input it was computed from, `scheduler.add_noise(normal, noise, timesteps)`).  `velocity=True`
    reads `out` as a v prediction.  `model_or_scheduler` supplies the alpha-bar table (a LowLightDiffusion or its LCMScheduler).
    HIP device only; one call of llie_x0_loss, no synchronisation."""
    scheduler = getattr(model_or_scheduler, "scheduler", model_or_scheduler)
    if not isinstance(scheduler, LCMScheduler):
        raise ValueError(f"x0_loss takes a LowLightDiffusion or an LCMScheduler, got {type(model_or_scheduler).__name__}")
    if x_t.requires_grad or normal.requires_grad:
        raise ValueError("x0_loss differentiates with respect to `out` only; x_t and normal must not require grad")
    return _X0LossFn.apply(out, scheduler, x_t, normal, timesteps, bool(velocity), float(ssim_weight), float(l1_weight))


class LowLightLCMDistillation(nn.Module):
    """Consistency distillation teacher -> student (low_light_diffusion.py:284-408).  Constructor, attributes (`teacher`,
    `student`, `ema_student`, `num_ddim_timesteps`, `guidance_scale_range`) and the `state_dict` keys (`teacher.unet.*`,
    `student.unet.*`, `ema_student.unet.*`) are the reference's.  The teacher is put in eval mode and frozen; `ema_student` is
    `copy.deepcopy(student_model)` and gets its own engine context.  `guidance_scale_range` is stored and, as in the reference,
    unused unless `guidance=True`.  Teacher and student may be different variants but must share `image_size`.

    Guided distillation (extension, `guidance=True`, keyword only; guidance.py has the definitions).  Each sample gets a scale
    w_b = lo + (hi - lo) u_b, (lo, hi) = `guidance_scale_range` (finite, lo <= hi, else ValueError), u = torch.rand(B, device=dev)
    drawn third, after `noise` and `idx` (the product and the sum are two fp32 operations); `w=` of the loss and of DistillStep
    supplies the scales instead.  The teacher's output becomes llie_guide(teacher(x_t, low), teacher(x_t, null), w) -- both from
    one 2B-row pass (llie_guidance_pair), or from two B-row passes where the teacher's engine refuses 2B rows, with the same bits
    -- and enters the unchanged `consistency_target`.  The student and the EMA student see `low`, as always, and are not told
    w: the reference network has no such input, and `state_dict` parity wins.  With lo < hi the student therefore learns the
    mixture over the range; a degenerate range (w, w) -- the scale the student is meant to reproduce -- is the normal use.  With
    `guidance=False` nothing is drawn or launched that was not before: the same bits, the same generator state.
    `guidance_rescale=phi` (keyword only, `guidance=True` only: a non-zero value without it is a ValueError) distils the teacher
    with guidance rescale, as `enhance(guidance_rescale=phi)` samples it: llie_guide_rescale with the per-row scales takes
    llie_guide's place, so a student distilled at (w, w) does not inherit the over-exposure of a large w.  0.0 (the default)
    launches nothing that was not launched before.

    Prediction types (extension).  The teacher's output is read as `teacher.scheduler.config.prediction_type`, the student's and
    the EMA student's as `student.scheduler.config.prediction_type` (`teacher_prediction` / `student_prediction`); each is
    "epsilon" or "v_prediction", in any mix, and anything else is a ValueError at construction.  The alpha-bar table is the
    teacher's scheduler's.  An output o at (x, a), sa = sqrt(a), sb = sqrt(1 - a), means
        epsilon:       x0 = (x - sb o) / sa      e^ = o
        v_prediction:  x0 = sa x - sb o          e^ = sb x + sa o
    and x_next = sa_n x0 + sb_n e^ (teacher), s0 = x0(x_t, student, a_t), g0 = x0(x_next, EMA student, a_n), loss =
    huber(s0, g0).  `consistency_target_host` / `consistency_loss_host` are the float64 definitions.

    Shapes follow the batch: [B,3,H,W] of any shape the student's engine trains at (llie_train_shape_ok) and the teacher's and
    the EMA student's engines run at (llie_frame_shape_ok) -- H and W multiples of 8 and at least 64; `image_size` is one such
    shape and runs as it always did.  A refused shape is a ValueError naming the rule, raised before any draw.

    The timestep pair of a sample is t = idx*c + c-1, t_next = (idx+k)*c + c-1 (c = T // num_ddim_timesteps, k =
    num_ddim_timesteps // num_inference_steps, idx uniform in [0, num_ddim_timesteps - k)): t_next is the noisier one, as
    written in the reference.  With the zero-SNR table alpha-bar[999] == 0, so idx = num_ddim_timesteps - k - 1 makes an
    epsilon student's target x0 +-inf and the loss +inf while every gradient stays finite (Huber's gradient saturates) --
    reproduced as is.  A v-prediction student's target is finite there (g0 = -out_ema), and so is its loss."""

    def __init__(self, teacher_model: LowLightDiffusion, student_model: LowLightDiffusion, num_ddim_timesteps: int = 50,
                 guidance_scale_range: Tuple[float, float] = (3.0, 15.0), *, guidance: bool = False,
                 guidance_rescale: float = 0.0):
        super().__init__()
        if not isinstance(guidance, bool):
            raise ValueError(f"guidance must be True or False, got {guidance!r}")
        if guidance:
            G.check_guidance_range(guidance_scale_range)
            guidance_rescale = G.check_guidance_rescale(guidance_rescale)
        elif guidance_rescale is not None and (isinstance(guidance_rescale, bool) or guidance_rescale != 0):
            raise ValueError(f"guidance_rescale={guidance_rescale!r} needs LowLightLCMDistillation(guidance=True)")
        if teacher_model.image_size != student_model.image_size:
            raise ValueError(f"teacher and student must share image_size (got {teacher_model.image_size} and "
                             f"{student_model.image_size}): both denoise the same x_t")
        for who, m in (("teacher", teacher_model), ("student", student_model)):
            prediction_code(getattr(m.scheduler.config, "prediction_type", "epsilon"), f"the {who}'s scheduler.config.prediction_type")
        self.teacher = teacher_model
        self.teacher.eval()
        self.teacher.requires_grad_(False)
        self.student = student_model
        self.num_ddim_timesteps = num_ddim_timesteps
        self.guidance_scale_range = guidance_scale_range
        self.guidance = guidance
        self.guidance_rescale = guidance_rescale if guidance else 0.0
        self.ema_student = copy.deepcopy(student_model)  # own parameters, own engine context (built lazily)
        self.ema_student.eval()
        self.ema_student.requires_grad_(False)
        object.__setattr__(self, "_ema_native", None)   # llie_ema* over (ema_student, student) parameters
        object.__setattr__(self, "_ema_layout", None)

    def __getstate__(self):
        st = dict(self.__dict__)
        st["_ema_native"], st["_ema_layout"] = None, None
        return st

    def __del__(self):
        try:
            self._release_ema()
        except Exception:  # noqa: BLE001
            pass

    @property
    def teacher_prediction(self) -> str:
        return getattr(self.teacher.scheduler.config, "prediction_type", "epsilon")

    @property
    def student_prediction(self) -> str:
        """How the student's and the EMA student's outputs are read."""
        return getattr(self.student.scheduler.config, "prediction_type", "epsilon")

    # ------------------------------------------------------------------ timestep pairs (:344-355)
    def timestep_pairs(self, idx: torch.Tensor, num_inference_steps: int = 4) -> Tuple[torch.Tensor, torch.Tensor]:
        """idx -> (t, t_next) on idx's device."""
        c = self.teacher.scheduler.config.num_train_timesteps // self.num_ddim_timesteps
        k = self.num_ddim_timesteps // num_inference_steps
        return idx * c + c - 1, (idx + k) * c + c - 1

    def _draws(self, normal_light: torch.Tensor, num_inference_steps: int, noise: Optional[torch.Tensor],
               idx: Optional[torch.Tensor]) -> Tuple[torch.Tensor, torch.Tensor]:
        b, dev = normal_light.shape[0], normal_light.device
        k = self.num_ddim_timesteps // num_inference_steps
        if k < 1 or self.num_ddim_timesteps - k < 1:
            raise ValueError(f"num_inference_steps={num_inference_steps} leaves no timestep pair for "
                             f"num_ddim_timesteps={self.num_ddim_timesteps}")
        # the reference's draw order on the device generator: noise first, then idx (:337-349)
        noise = torch.randn_like(normal_light) if noise is None else noise.to(device=dev, dtype=torch.float32)
        if idx is None:
            idx = torch.randint(0, self.num_ddim_timesteps - k, (b,), device=dev)
        else:
            idx = torch.as_tensor(idx)
            if idx.device.type == "cpu" and idx.numel() and (int(idx.min()) < 0 or int(idx.max()) >= self.num_ddim_timesteps - k):
                raise ValueError(f"idx must lie in [0, {self.num_ddim_timesteps - k})")
            idx = idx.to(device=dev, dtype=torch.long)
        if tuple(noise.shape) != tuple(normal_light.shape) or tuple(idx.shape) != (b,):
            raise ValueError(f"noise must be shaped like normal_light and idx must be [{b}]")
        return noise.contiguous(), idx.contiguous()

    def _draw_w(self, b: int, dev, w) -> Optional[torch.Tensor]:
        """The per-sample guidance scales, fp32 [B] on `dev`: None with guidance off (a supplied `w` is then a ValueError);
        the supplied `w`; else lo + (hi - lo) u with u = torch.rand(B, device=dev), the third draw."""
        if not self.guidance:
            if w is not None:
                raise ValueError("w= needs LowLightLCMDistillation(guidance=True)")
            return None
        if w is not None:
            w = torch.as_tensor(w)
            if tuple(w.shape) != (b,):
                raise ValueError(f"w must be [{b}], got {list(w.shape)}")
            return w.to(device=dev, dtype=torch.float32).contiguous()
        lo, hi = G.check_guidance_range(self.guidance_scale_range)
        return torch.rand(b, device=dev).mul_(hi - lo).add_(lo)

    def teacher_output(self, x_t: torch.Tensor, low: torch.Tensor, t: torch.Tensor, w: Optional[torch.Tensor] = None, *,
                       _passes: Optional[int] = None) -> torch.Tensor:
        """The teacher's output at (x_t, t), without gradients: its forward on `low` when `w` is None; else the guided output
        llie_guide(teacher(x_t, low), teacher(x_t, null), w), `w` device fp32 [B] -- one 2B-row pass, or two B-row passes where
        the teacher's engine refuses 2B rows (`_passes` forces either form; the bits are the same).  With `guidance_rescale` > 0
        llie_guide_rescale takes llie_guide's place."""
        with torch.no_grad():
            if w is None:
                return self.teacher.unet.forward_split(x_t, low, t, frame=True)
            b = x_t.shape[0]
            hh, ww = int(x_t.shape[2]), int(x_t.shape[3])
            s = self.teacher.image_size
            x_t, low = x_t.detach().float().contiguous(), low.detach().float().contiguous()
            if self.teacher._guided_plan(b, x_t.device, None if (hh, ww) == (s, s) else (hh, ww), _passes) == 1:
                lat2, cond2 = G.guidance_pair_device(x_t, low)
                out2 = self.teacher.unet.forward_split(lat2, cond2, torch.cat([t, t]), frame=True)
                o_c, o_u = out2[:b], out2[b:]
            else:
                o_c = self.teacher.unet.forward_split(x_t, low, t, frame=True)
                o_u = self.teacher.unet.forward_split(x_t, torch.zeros_like(low), t, frame=True)
            phi = getattr(self, "guidance_rescale", 0.0)
            if phi > 0:
                return G.guide_rescale_device(o_c, o_u, w, phi, out=o_c)
            return G.guide_device(o_c, o_u, w, out=o_c)

    def _check_inputs(self, low_light: torch.Tensor, normal_light: torch.Tensor) -> None:
        """Device, [B,3,H,W] of one shape, and the three engines' shape rules: raises before any draw."""
        from .unet import resolve_compute_dtype
        _require_hip(low_light, "LowLightLCMDistillation")
        _require_hip(normal_light, "LowLightLCMDistillation")
        if low_light.dim() != 4 or low_light.shape[1] != 3 or tuple(normal_light.shape) != tuple(low_light.shape):
            raise ValueError(f"low_light / normal_light must be [B,3,H,W] of one shape, got {tuple(low_light.shape)} and "
                             f"{tuple(normal_light.shape)}")
        b, hh, ww = int(low_light.shape[0]), int(low_light.shape[2]), int(low_light.shape[3])
        s = self.student.image_size
        if (hh, ww) == (s, s):  # image_size goes unasked, as it always did
            return
        for who, m, train in (("student", self.student, True), ("teacher", self.teacher, False), ("EMA student", self.ema_student, False)):
            h = m.unet._handle(resolve_compute_dtype(m.unet.compute_dtype))
            try:
                (h.train_shape_ok if train else h.frame_shape_ok)(b, hh, ww)
            except ValueError as e:
                raise ValueError(f"LowLightLCMDistillation ({who}): {e}") from None

    # ------------------------------------------------------------------ the loss (:325-393)
    def consistency_distillation_loss(self, low_light: torch.Tensor, normal_light: torch.Tensor, num_inference_steps: int = 4, *,
                                      noise: Optional[torch.Tensor] = None, idx: Optional[torch.Tensor] = None,
                                      w: Optional[torch.Tensor] = None, _teacher_passes: Optional[int] = None) -> torch.Tensor:
        """Huber consistency loss (0-d device tensor with a grad_fn reaching the student's parameters) at the batch's own
        H x W (the class docstring has the shape rule and the prediction types).  `noise` / `idx` (extensions) supply the two
        draws, e.g. CPU-generated ones for a run comparable with the CPU reference.  `w` (fp32 [B], `guidance=True` only)
        supplies the per-sample guidance scales, the third draw (the class docstring has the guided teacher)."""
        self._check_inputs(low_light, normal_light)
        noise, idx = self._draws(normal_light, num_inference_steps, noise, idx)
        w = self._draw_w(int(low_light.shape[0]), low_light.device, w)
        t, t_next = self.timestep_pairs(idx, num_inference_steps)
        sched = self.teacher.scheduler
        low = low_light.detach().float().contiguous()
        x_t = sched.add_noise(normal_light, noise, t)
        with torch.no_grad():
            e_teacher = self.teacher_output(x_t, low, t, w, _passes=_teacher_passes)
            x_next = consistency_target(sched, x_t, e_teacher, t, t_next, prediction_type=self.teacher_prediction)
        e_student = self.student.unet.forward_split(x_t, low, t, frame=True)
        with torch.no_grad():
            e_ema = self.ema_student.unet.forward_split(x_next, low, t_next, frame=True)
        if torch.is_grad_enabled() and e_student.requires_grad:
            return _ConsistencyLossFn.apply(e_student, sched, x_t, x_next, e_ema, t, t_next, self.student_prediction)
        return consistency_loss(sched, x_t, x_next, e_student, e_ema, t, t_next, prediction_type=self.student_prediction)[0]

    # ------------------------------------------------------------------ EMA (:316-323)
    def _ema_pairs(self):
        ema, src = list(self.ema_student.parameters()), list(self.student.parameters())
        if len(ema) != len(src) or any(a.shape != b.shape for a, b in zip(ema, src)):
            raise ValueError("ema_student and student no longer have the same parameters")
        for p in ema + src:
            _require_hip(p, "update_ema")
            if p.dtype != torch.float32 or not p.is_contiguous() or p.device != ema[0].device:
                raise ValueError("update_ema: fp32 contiguous parameters on one device")
        return ema, src

    def _release_ema(self) -> None:
        if self.__dict__.get("_ema_native") is not None:
            torch.cuda.synchronize()  # an update reading the table may still be in flight
            N.lib().llie_ema_destroy(self._ema_native)
            object.__setattr__(self, "_ema_native", None)

    def _ema_handle(self):
        ema, src = self._ema_pairs()
        layout = (tuple(p.data_ptr() for p in ema), tuple(p.data_ptr() for p in src))
        if self._ema_native is not None and layout == self._ema_layout:
            return self._ema_native, ema[0].device
        self._release_ema()
        n = len(ema)
        out = C.c_void_p()
        with torch.cuda.device(ema[0].device):
            N.check(N.lib().llie_ema_create((C.c_void_p * n)(*layout[0]), (C.c_void_p * n)(*layout[1]),
                                            (C.c_int64 * n)(*[p.numel() for p in ema]), n, C.byref(out)), "update_ema")
        object.__setattr__(self, "_ema_native", out)
        object.__setattr__(self, "_ema_layout", layout)
        return out, ema[0].device

    @torch.no_grad()
    def update_ema(self, decay: float = 0.95) -> None:
        """ema = ema * decay + (1 - decay) * student over every parameter, one launch (llie_ema_update).  The EMA student's
        engine weights follow at its next forward (the engine notices the changed content)."""
        h, dev = self._ema_handle()
        with torch.cuda.device(dev):
            N.check(N.lib().llie_ema_update(h, float(decay), torch.cuda.current_stream(dev).cuda_stream), "update_ema")


def normalize_image(x: torch.Tensor) -> torch.Tensor:
    """[0,1] -> [-1,1] (low_light_diffusion.py:412-414)."""
    return x * 2 - 1


def denormalize_image(x: torch.Tensor) -> torch.Tensor:
    """[-1,1] -> [0,1] (low_light_diffusion.py:417-419)."""
    return (x + 1) / 2
