/*
 * llie.h -- C ABI of libllie_hip.so: the MI355X (gfx950) engine for the LCM denoising hot path of
 * zamazincode/cv-diffusion-model.
 *
 * The reference has no FFI (it is pure PyTorch), so this header *defines* the native boundary that
 * replaces its hot path.  Each entry point cites the reference interface it stands in for
 * (paths relative to the reference root).  Conventions:
 *   - plain pointers and sizes only; no torch types.  All tensor pointers are DEVICE pointers.
 *   - public I/O tensors are fp32 NCHW contiguous, exactly what the reference's callers hold
 *     (scripts/inference.py:137-145, scripts/benchmark.py:61-79); NHWC / reduced precision are
 *     internal to the engine.
 *   - the caller owns every activation / IO buffer and the workspace (size from
 *     llie_workspace_bytes); the handle owns only the repacked weights.
 *   - every function returns 0 on success, a negative llie_status on bad arguments, or a positive
 *     hipError_t passed through.  Nothing throws.  llie_last_error() gives a message.
 *   - launches are asynchronous on the caller's stream; no hidden synchronisation, no host reads
 *     of device data.  A handle is not re-entrant (one stream at a time), like the reference module
 *     (lcm_scheduler.py:163-164,245 mutate scheduler state inside enhance()).
 */
#ifndef LLIE_H_
#define LLIE_H_

#include <stddef.h>
#include <stdint.h>

#ifdef __cplusplus
extern "C" {
#endif

typedef struct llie_ctx llie_ctx;
typedef void* llie_stream; /* hipStream_t */

enum llie_status {
  LLIE_OK = 0,
  LLIE_ERR_ARG = -1,       /* null pointer / bad enum / bad size */
  LLIE_ERR_SHAPE = -2,     /* shape not supported by the engine (e.g. image side not a multiple of 8, or below 64) */
  LLIE_ERR_CONFIG = -3,    /* topology the reference itself cannot construct (GroupNorm divisibility) */
  LLIE_ERR_KEY = -4,       /* unknown state_dict key or wrong element count */
  LLIE_ERR_NOT_LOADED = -5,/* forward called before every parameter was loaded */
  LLIE_ERR_WORKSPACE = -6, /* workspace too small */
  LLIE_ERR_NO_DEVICE = -7
};

enum llie_dtype { LLIE_F32 = 0, LLIE_F16 = 1, LLIE_BF16 = 2 };

/* Which module tree a handle holds.  LLIE_UNET is the product; the others expose single reference
 * operators (same parameter names as the reference classes) so that parity tests can be written
 * per operator, the way the reference's modules are organised. */
enum llie_kind {
  LLIE_UNET = 0,   /* EfficientUNet                      efficient_unet.py:387-606 */
  LLIE_IRB = 1,    /* InvertedResidualBlock              efficient_unet.py:134-236 */
  LLIE_ATTN = 2,   /* LinearAttention                    efficient_unet.py:239-308 */
  LLIE_DOWN = 3,   /* Downsample (3x3 stride-2 conv)     efficient_unet.py:360-372 */
  LLIE_UP = 4,     /* Upsample (bilinear x2 + 3x3 conv)  efficient_unet.py:375-384 */
  LLIE_SE = 5,     /* SqueezeExcitation (in_channels = C) efficient_unet.py:79-100; forward only */
  LLIE_SOFTATTN = 6 /* StandardAttention                  efficient_unet.py:311-357 */
};

/* Mirrors EfficientUNetConfig (efficient_unet.py:24-57) for LLIE_UNET; for the single-operator kinds
 * only the fields named in the comments are read. */
typedef struct llie_config {
  int kind;               /* llie_kind */
  int compute_dtype;      /* llie_dtype: storage type of activations / MFMA operand type (accumulation is fp32) */
  int in_channels;        /* UNET: 6 (concat conditioning, low_light_diffusion.py:77); IRB/ATTN/DOWN/UP: C_in */
  int out_channels;       /* UNET: 3; IRB: C_out */
  int base_channels;
  int channel_multipliers[4];
  int num_res_blocks;
  int expansion_ratio;
  int time_embed_dim;     /* UNET, IRB */
  int num_attention_heads;/* UNET, ATTN */
  int image_size;         /* UNET: decides attention placement (efficient_unet.py:426,447,509) */
  int attention_resolutions[2];
  int allow_unpinned;     /* 0: topologies whose nn.GroupNorm(min(32,C), C) the reference cannot construct (tiny, base)
                             fail with LLIE_ERR_CONFIG like the reference's ValueError.  1: build them with the
                             documented deviation groups = largest divisor of C that is <= 32 (no reference output
                             exists to pin this: parity-unpinned; inference only) */
  int softmax_attention;  /* UNET: 0 = every attention site is a LinearAttention (use_linear_attention=True, the default of the
                             reference); 1 = a StandardAttention (softmax; efficient_unet.py:311-357, keys norm / to_qkv / to_out).
                             Together with allow_unpinned: LLIE_ERR_CONFIG */
} llie_config;

/* LCM scheduler coefficients for one step (host values; computed by the host-side scheduler from the
 * fp32 alpha-bar table, lcm_scheduler.py:208-242). */
typedef struct llie_step_coef {
  float sqrt_alpha_t, sqrt_beta_t;       /* alpha_prod_t**0.5, (1-alpha_prod_t)**0.5 */
  float sqrt_alpha_prev, sqrt_beta_prev; /* for prev_t; ignored when is_last */
  int   is_last;                         /* prev_t == 0 -> prev_sample = x0 (lcm_scheduler.py:228-229) */
  int   v_prediction;                    /* 0 epsilon (:217), 1 v_prediction (:220) */
  int   clamp_x0;                        /* 1: x0 = clip(x0, -1, 1) before re-noising -- the deployment loop's
                                            semantics (src/export/android_pipeline.py:250-252); the LCMScheduler
                                            has that clamp commented out (lcm_scheduler.py:224-225) -> 0 */
  int   sampler;                         /* 0: LCM, re-noise x0 with a fresh draw (above).  1: deterministic DDIM (eta = 0): the
                                            predicted noise takes the draw's place, prev = sqrt_alpha_prev*x0 + sqrt_beta_prev*e,
                                            e = model_output (epsilon) | sqrt_alpha_t*model_output + sqrt_beta_t*sample (v); no noise
                                            is read.  Not defined together with clamp_x0 (LLIE_ERR_ARG) */
} llie_step_coef;

/* Coefficients of one step of the DPM-Solver++ 2M sampler (data-prediction form; llie_dpm_step below has the arithmetic).  Host
 * values: computed in float64 from the alpha-bar table and rounded once to fp32.  With alpha = sqrt(abar), sigma = sqrt(1 - abar),
 * lambda = log(alpha / sigma), t the step's timestep, p the next one, h = lambda_p - lambda_t and r = h_previous / h:
 *   k_x = sigma_p / sigma_t
 *   order 1 (the first step):  k_0 = -alpha_p expm1(-h),                     k_1 = 0
 *   order 2:                   k_0 = -alpha_p expm1(-h) (1 + 1 / (2 r)),     k_1 = alpha_p expm1(-h) / (2 r) */
typedef struct llie_dpm_coef {
  float sqrt_alpha_t, sqrt_beta_t;   /* x0 from the network output, as in llie_step_coef */
  float k_x, k_0, k_1;               /* ignored when is_last */
  int   v_prediction;                /* 0 epsilon, 1 v_prediction */
  int   order;                       /* 1: the history is not read.  2: it holds the previous step's x0.  Anything else: LLIE_ERR_ARG */
  int   is_last;                     /* the step at t = 0: prev = x0 */
} llie_dpm_coef;

const char* llie_last_error(void);
const char* llie_version(void);

/* create_efficient_unet / EfficientUNet.__init__ (efficient_unet.py:403-530, 631-692).  Fails with
 * LLIE_ERR_CONFIG for topologies whose GroupNorm the reference rejects (tiny, base). */
int llie_create(const llie_config* cfg, llie_ctx** out);
void llie_destroy(llie_ctx* ctx);

/* state_dict introspection: number of parameters and (key, element count, shape) of each, in the
 * reference's registration order, keys without the "unet." prefix.  `shape4` receives
 * the tensor's shape in the reference's state_dict (ndim entries valid). */
int llie_num_params(const llie_ctx* ctx);
int llie_param_info(const llie_ctx* ctx, int index, char* key_buf, size_t key_cap, int64_t* numel, int* ndim,
                    int64_t* shape4);

/* nn.Module.load_state_dict, one tensor at a time (scripts/inference.py:78-79, scripts/benchmark.py:56):
 * `src` is a DEVICE pointer to the fp32 tensor in the reference's own layout (OIHW conv weights,
 * [out,in] Linear weights); the engine repacks it on `stream`. */
int llie_load_param(llie_ctx* ctx, const char* key, const float* src, int64_t numel, llie_stream stream);
/* Reload all parameters at once -- what `optimizer.step()` implies for a module whose weights live outside PyTorch
 * (src/training/trainer.py:300-318) and what `load_state_dict` does (scripts/inference.py:78-84): srcs[i] = device fp32 tensor of parameter i in
 * llie_param_info order (host array of n = llie_num_params pointers).  One kernel for all plain / 1x1 / 3x3 /
 * depthwise tensors; equivalent to n llie_load_param calls. */
int llie_load_all(llie_ctx* ctx, const float* const* srcs, int n, llie_stream stream);
/* Same arguments; reloads only if the parameters' CONTENT differs from the last load.  The comparison (a 64-bit
 * position-weighted hash of the fp32 bits) and the decision both happen on the device, so the call stays asynchronous:
 * it catches in-place writes that bypass PyTorch's version counters -- `param.data.copy_(...)`, which is how the
 * reference's EMA swaps weights in and out (src/training/trainer.py:104-117, low_light_diffusion.py:317-323). */
int llie_refresh_params(llie_ctx* ctx, const float* const* srcs, int n, llie_stream stream);
int llie_params_loaded(const llie_ctx* ctx); /* 1 when every key has been loaded */

/* Bytes of scratch the forward needs for a batch (UNET: spatial size = image_size; single
 * operators: H x W given).  For a UNET handle the figure includes the three images the loop of llie_enhance keeps in front of the
 * forward's own plan, and llie_unet_forward / llie_unet_forward_hw ask for all of it: a workspace smaller than this query (or
 * llie_frame_workspace_bytes with max_steps = 0) answered returns LLIE_ERR_WORKSPACE before anything is launched. */
int64_t llie_workspace_bytes(llie_ctx* ctx, int batch, int height, int width);
/* Workspace for llie_enhance including the staging area its hipGraph path needs (inputs / outputs of
 * up to `max_steps` steps).  With only llie_workspace_bytes() the loop runs as plain launches. */
int64_t llie_enhance_workspace_bytes(llie_ctx* ctx, int batch, int max_steps);

/* EfficientUNet.forward(x, timestep) (efficient_unet.py:532-606) with x given as its two concat
 * halves (low_light_diffusion.py:222: cat([latents, low_light], 1)), both fp32 NCHW [B,3,S,S].
 * `timesteps`: device int64[B].  uniform_t != 0 promises all B timesteps are equal (true inside
 * enhance(), low_light_diffusion.py:218) and lets the engine evaluate the time MLPs once.
 * `eps_out`: fp32 NCHW [B,3,S,S]. */
int llie_unet_forward(llie_ctx* ctx, const float* latents, const float* cond, const int64_t* timesteps,
                      int uniform_t, float* eps_out, int batch, void* workspace, int64_t workspace_bytes,
                      llie_stream stream);

/* Frame mode: the network, with the module tree its image_size fixed (attention placement, state_dict), run at a frame's own
 * H x W.  The denoiser is fully convolutional and its attention takes any number of tokens (the linear form at a cost linear in the pixel
 * count, the softmax form of softmax_attention = 1 at a quadratic one, in flash form: no N x N matrix is stored), so nothing but
 * these rules ties it to image_size.  Inference only.  The entry points without _hw are these at H = W = image_size.
 *   llie_frame_shape_ok (host only, no GPU needed): LLIE_OK, or LLIE_ERR_SHAPE (llie_last_error names the rule) unless
 *       - height and width are multiples of 8 and at least 64 (three stride-2 levels, each restored by a x2 up-sampling);
 *       - batch <= 65535;
 *       - batch x height x width x Cmax <= 2^31 - 1, Cmax = the widest channel count the plan stores at full resolution (the
 *         hidden width of the widest level-0 block: 384 for `small`, so about 5.59 M pixels per call).  The kernels index
 *         elements of a tensor with 32-bit integers; this clause is what keeps that arithmetic safe.  Larger images go through
 *         tiles (llie_tile_*).
 *   llie_frame_workspace_bytes: scratch of llie_unet_forward_hw / llie_enhance_hw at that shape; max_steps = 0 gives the size with
 *       which the loop runs as plain launches, max_steps > 0 adds the staging area of the hipGraph path for up to that many
 *       steps (llie_enhance_workspace_bytes).  A shape llie_frame_shape_ok refuses returns its code.
 *   llie_unet_forward_hw: llie_unet_forward on fp32 NCHW [B,3,H,W] halves; eps_out [B,3,H,W].
 * A launch rule (block form, Gram statistics, folded up-sampling conv) depends on the layer, (H, W), the dtype and the knobs,
 * never on the batch: a frame's result is the same bits alone or in a batch. */
int llie_frame_shape_ok(const llie_ctx* ctx, int batch, int height, int width);
/* host only, no GPU needed: floor((2^31 - 1) / (batch x Cmax)), the pixel count height x width that the last clause above
 * allows a frame of `batch` (5 592 405 for `small` at batch 1).  What a tile plan sizes its tiles by (tiling.auto_tile_plan). */
int64_t llie_frame_max_pixels(const llie_ctx* ctx, int batch);
int64_t llie_frame_workspace_bytes(llie_ctx* ctx, int batch, int height, int width, int max_steps);
int llie_unet_forward_hw(llie_ctx* ctx, const float* latents, const float* cond, const int64_t* timesteps, int uniform_t,
                         float* eps_out, int batch, int height, int width, void* workspace, int64_t workspace_bytes,
                         llie_stream stream);

/* Single-operator forward for kinds IRB / ATTN / DOWN / UP: x fp32 NCHW [B,C,H,W] -> y fp32 NCHW.
 * `temb` (IRB only): device fp32 [B, time_embed_dim] time embedding (efficient_unet.py:203). */
int llie_module_forward(llie_ctx* ctx, const float* x, const float* temb, float* y, int batch, int height,
                        int width, void* workspace, int64_t workspace_bytes, llie_stream stream);

/* ---- Training step (callers: src/training/trainer.py:269-338 via LowLightDiffusion.compute_loss,
 * low_light_diffusion.py:140-171,250-277).  The forward pass keeps its activations in the workspace; the
 * backward pass walks them in reverse and writes every parameter's gradient, fp32 in the reference's
 * state_dict layout, into one flat buffer: parameter i (llie_param_info order) at llie_param_grad_offset(i),
 * llie_grad_numel() floats in total.  Timesteps are per sample (int64[B]).  All reductions run in a fixed
 * order, so gradients are bitwise reproducible.
 *   llie_unet_train_forward:  eps = unet(cat[lat, cond], t), activations retained in `workspace`
 *   llie_unet_backward:       given d(loss)/d(eps) (fp32 NCHW) -> grads; `workspace` must be the untouched
 *                             buffer of the preceding train_forward; lat / cond / t must still be alive
 *   llie_module_backward:     single operator (IRB / ATTN / DOWN / UP handles): forward + backward in one call;
 *                             dx fp32 NCHW like x, dtemb [B][T] (IRB only)
 * Training at a frame's own H x W (UNet handles; the module tree stays the one image_size fixed, as in frame mode):
 *   llie_train_shape_ok (host only, no GPU needed): LLIE_OK for the frames a UNet trains at.  It is llie_frame_shape_ok with the
 *       element cap taken over what the backward pass stores: batch x ceil64(height x width) x Cmax <= 2^31 - 1, where the rows
 *       of each image are padded to whole 64-row chunks (the weight-gradient GEMM walks them so) and Cmax also covers the
 *       up-sampled tensor the tape keeps at full resolution and the 32-channel packed copies of the head and the input conv.
 *       `tiny` / `base` (zero-padded channels) return LLIE_ERR_CONFIG: inference only.
 *   llie_train_workspace_bytes: for a UNet handle the plan at (height, width); 0, 0 means image_size.  A shape
 *       llie_train_shape_ok refuses returns its code.
 *   llie_unet_train_forward_hw: llie_unet_train_forward on fp32 NCHW [B,3,H,W]; llie_unet_train_forward is this entry at
 *       H = W = image_size.  The tape records (H, W): llie_unet_backward takes the shape from it (d_eps [B,3,H,W]).
 * The weight-gradient GEMM splits its rows freely when H or W is off the multiples of 64, and by the rule of the 64-grid
 * otherwise: a rule on the frame alone, never on the batch.
 *   llie_unet_backward_dx:    llie_unet_backward plus the gradients of the network input: d_latents fp32 NCHW [B][in_channels / 2][H][W]
 *       and d_cond [B][in_channels - in_channels / 2][H][W] at the tape's (H, W), the two halves llie_unet_train_forward read.  Each
 *       may be NULL and then costs nothing; with both NULL the call is llie_unet_backward, launch for launch and bit for bit
 *       (llie_unet_backward is this call with two NULLs).  They are caller buffers: the workspace plan does not grow.  Values are
 *       stored, not accumulated, by one kernel (the transpose of init_conv over d(h0), fp32 accumulation in a fixed order): bitwise
 *       reproducible, the same bits with and without the backward side stream, an image's rows the same alone or in a batch, and
 *       the parameter gradients are the bits llie_unet_backward gives.  `grads` stays required; same errors as llie_unet_backward. */
int llie_train_shape_ok(const llie_ctx* ctx, int batch, int height, int width);
int llie_unet_train_forward_hw(llie_ctx* ctx, const float* latents, const float* cond, const int64_t* timesteps, float* eps,
                               int batch, int height, int width, void* workspace, int64_t workspace_bytes, llie_stream stream);
int64_t llie_grad_numel(const llie_ctx* ctx);
int64_t llie_param_grad_offset(const llie_ctx* ctx, int index);
int64_t llie_train_workspace_bytes(llie_ctx* ctx, int batch, int height, int width);
int llie_unet_train_forward(llie_ctx* ctx, const float* latents, const float* cond, const int64_t* timesteps, float* eps,
                            int batch, void* workspace, int64_t workspace_bytes, llie_stream stream);
int llie_unet_backward(llie_ctx* ctx, const float* d_eps, float* grads, int batch, void* workspace, int64_t workspace_bytes,
                       llie_stream stream);
int llie_unet_backward_dx(llie_ctx* ctx, const float* d_eps, float* grads, float* d_latents, float* d_cond, int batch,
                          void* workspace, int64_t workspace_bytes, llie_stream stream);
int llie_module_backward(llie_ctx* ctx, const float* x, const float* temb, const float* dy, float* dx, float* dtemb,
                         float* grads, int batch, int H, int W, void* workspace, int64_t workspace_bytes, llie_stream stream);

/* ---- Optimiser step of the training loop (replaces, in the trainer's inner loop src/training/trainer.py:296-324, the eager
 * sequence  scaler.unscale_ -> torch.nn.utils.clip_grad_norm_(params, gradient_clip) -> optimizer.step() [torch.optim.AdamW,
 * trainer.py:163-168] -> EMAModel.update (trainer.py:98-104)  by three launches over every parameter tensor at once; same
 * arithmetic operation for operation: decoupled decay p *= 1 - lr wd; m = m + (g - m)(1 - b1); v = b2 v + (1 - b2) g g;
 * p -= lr / (1 - b1^t) * m / (sqrt(v) / sqrt(1 - b2^t) + eps); shadow = decay shadow + (1 - decay) p).
 * A tensor's gradient is read at grad_base + grad_offset (the flat buffer llie_unet_backward fills: grad_offset =
 * llie_param_grad_offset(i)); `ema` may be NULL.  All pointers are device fp32 and must stay valid for the optimiser's life.
 * llie_optimizer_step: every gradient is first multiplied by grad_scale (1 / loss scale, 1 / world size); the total norm of the
 * scaled gradients is clipped to max_grad_norm (<= 0: no clipping) as clip_grad_norm_ does (factor min(1, max / (norm + 1e-6)));
 * ema_decay < 0: shadows untouched; skip_nonfinite != 0: a non-finite norm leaves parameters, moments and shadows unchanged
 * (GradScaler.step).  `step` is the 1-based count of this update.  stats3 (device, 3 floats) receives {gradient norm, factor
 * applied to the gradients, 1 if the step was skipped else 0}.  The norm is a fixed-order sum: bitwise reproducible. */
typedef struct llie_opt_tensor {
  float* param;
  float* exp_avg;
  float* exp_avg_sq;
  float* ema;
  int64_t grad_offset; /* elements */
  int64_t numel;
} llie_opt_tensor;
typedef struct llie_opt_hyper {
  double lr, beta1, beta2, eps, weight_decay;
  double max_grad_norm, ema_decay, grad_scale;
  int64_t step;
  int32_t skip_nonfinite;
} llie_opt_hyper;
typedef struct llie_optimizer llie_optimizer;
int llie_optimizer_create(const llie_opt_tensor* tensors /* host array */, int count, llie_optimizer** out);
void llie_optimizer_destroy(llie_optimizer* opt);
int64_t llie_optimizer_numel(const llie_optimizer* opt);
int llie_optimizer_step(llie_optimizer* opt, const float* grad_base, const llie_opt_hyper* hyper, float* stats3, llie_stream stream);
/* llie_optimizer_step_amp: the same step with torch.amp.GradScaler around it (scaler.unscale_ -> clip_grad_norm_ ->
 * scaler.step -> scaler.update, then the EMA update), the loss scaler's state in device memory, no host synchronisation.
 * The gradients are the scaled ones (backward of loss * scale).  inv = (float)(1 / (double)*scale); the factor applied to
 * every gradient is inv * grad_scale * clip coefficient, the clip coefficient coming from the norm of the unscaled gradients.
 * found_inf = some gradient element is inf or NaN.  Then:
 *   found_inf:  parameters and moments unchanged, *step unchanged; the EMA shadows still move (shadow = decay shadow +
 *               (1 - decay) param: the reference trainer updates its EMA every iteration);
 *   otherwise:  *step += 1 and the AdamW update with the bias corrections of that count (formed on the device, in double);
 * and *scale / *growth_tracker are updated as torch's _amp_update_scale_: found_inf -> scale *= backoff_factor, tracker = 0;
 * else tracker + 1 == growth_interval -> scale *= growth_factor if the result is finite, tracker = 0; else tracker += 1.
 * hyper->step and hyper->skip_nonfinite are not used.  stats3 as llie_optimizer_step's: {norm of the unscaled gradients
 * (times grad_scale), factor applied, 1 if skipped}.  Fixed-order sums: bitwise reproducible. */
typedef struct llie_amp_state { /* device pointers */
  float* scale;            /* torch.amp.GradScaler's _scale */
  int32_t* growth_tracker; /* GradScaler's _growth_tracker */
  int32_t* step;           /* the optimiser's AdamW step count: updates taken so far */
} llie_amp_state;
typedef struct llie_amp_config {
  double growth_factor, backoff_factor;
  int32_t growth_interval;
} llie_amp_config;
int llie_optimizer_step_amp(llie_optimizer* opt, const float* grad_base, const llie_opt_hyper* hyper, const llie_amp_state* state,
                            const llie_amp_config* cfg, float* stats3, llie_stream stream);
/* Gradient accumulation over a window of micro-batches (device fp32, e.g. the flat buffer llie_unet_backward fills):
 * acc[i] = first ? weight * grad[i] : acc[i] + weight * grad[i], i < n.  The product and the sum are
 * rounded separately in fp32 (no fused multiply-add), so the NumPy twin is bit-equal.  With first != 0
 * acc is not read (stale NaNs do not survive).  n == 0: LLIE_OK, no launch.  Inf / NaN in grad propagate by ordinary
 * arithmetic, so the loss scaler of llie_optimizer_step_amp sees a bad micro-batch at the end of the window.
 * Checked before any HIP call (LLIE_ERR_ARG): a NULL pointer, a pointer that is not 4-byte aligned, n < 0 (or above 2^40), a
 * weight that is not finite or is <= 0, ranges [acc, acc + n) and [grad, grad + n) that overlap.  Pointers that are both
 * 16-byte aligned take four-float accesses with a scalar tail, others single elements; the element index is 64-bit. */
int llie_grad_accumulate(float* acc, const float* grad, int64_t n, float weight, int first, llie_stream stream);

/* ---- Consistency distillation (LowLightLCMDistillation.consistency_distillation_loss / update_ema,
 * low_light_diffusion.py:284-408).  Tensors are device fp32 [batch, per_sample] (NCHW [batch, 3, H, W]: per_sample = 3*H*W
 * elements per sample; the kernels know nothing of H x W); `t` / `t_next` are device int64 [batch]; `alphas_cumprod` is the
 * teacher scheduler's device fp32 table of `table_len` entries.  The reference's operation order is kept (no fused
 * multiply-adds).  A timestep outside [0, table_len) is never used as an index: that sample's outputs are NaN (the call is
 * asynchronous and cannot raise).
 *   llie_consistency_target:  x_next = sqrt(a_n) x0 + sqrt(1 - a_n) e_teacher,  x0 = (x_t - sqrt(1 - a_t) e_teacher) / sqrt(a_t)
 *   llie_consistency_loss:    s0 = (x_t - sqrt(1 - a_t) e_student) / sqrt(a_t),  g0 = (x_next - sqrt(1 - a_n) e_ema) / sqrt(a_n);
 *                             loss_out (device, 1 float) = F.huber_loss(s0, g0) (delta 1, mean);  d_student (like x_t) =
 *                             d(loss)/d(e_student) = clamp(s0 - g0, -1, 1) / n * (-sqrt(1 - a_t) / sqrt(a_t)).  The loss is a
 *                             fixed-order sum in double, bitwise reproducible; an inf / NaN term makes it inf / NaN (with
 *                             a zero-SNR table, t_next = T-1 has a_n = 0: g0 = +-inf, loss +inf, d_student finite).
 *                             `scratch` (device) must hold ceil(batch * per_sample / 1024) doubles.
 * a_t = alphas_cumprod[t[b]], a_n = alphas_cumprod[t_next[b]]. */
int llie_consistency_target(const float* x_t, const float* e_teacher, const int64_t* t, const int64_t* t_next,
                            const float* alphas_cumprod, int table_len, float* x_next, int batch, int64_t per_sample,
                            llie_stream stream);
int llie_consistency_loss(const float* x_t, const float* x_next, const float* e_student, const float* e_ema,
                          const int64_t* t, const int64_t* t_next, const float* alphas_cumprod, int table_len,
                          float* d_student, float* loss_out, int batch, int64_t per_sample, void* scratch,
                          int64_t scratch_bytes, llie_stream stream);
/* The same two with the prediction type of the networks as an argument (the two above are these at LLIE_PRED_EPSILON, bit for
 * bit).  A network output o of type p at (x, a), sa = sqrt(a), sb = sqrt(1 - a):
 *   LLIE_PRED_EPSILON:  x0 = (x - sb o) / sa     e^ = o              q = -sb / sa
 *   LLIE_PRED_V:        x0 = sa x - sb o         e^ = sb x + sa o     q = -sb
 *   llie_consistency_target_ex:  x_next = sa_n x0 + sb_n e^ of out_teacher at (x_t, a_t), read with teacher_pred
 *   llie_consistency_loss_ex:    s0 = x0 of out_student at (x_t, a_t), g0 = x0 of out_ema at (x_next, a_n), both read with
 *                                student_pred; loss = mean huber(s0 - g0), d_student = clamp(s0 - g0, -1, 1) / n * q(a_t).
 * Every product and difference is rounded on its own, as written.  At a = 0 the epsilon form keeps the inf / NaN behaviour
 * above; the v form is finite there (x0 = -o).  Any other prediction type: LLIE_ERR_ARG before any launch. */
#define LLIE_PRED_EPSILON 0
#define LLIE_PRED_V 1
int llie_consistency_target_ex(const float* x_t, const float* out_teacher, const int64_t* t, const int64_t* t_next,
                               const float* alphas_cumprod, int table_len, float* x_next, int batch, int64_t per_sample,
                               int teacher_pred, llie_stream stream);
int llie_consistency_loss_ex(const float* x_t, const float* x_next, const float* out_student, const float* out_ema,
                             const int64_t* t, const int64_t* t_next, const float* alphas_cumprod, int table_len,
                             float* d_student, float* loss_out, void* scratch, int64_t scratch_bytes, int batch,
                             int64_t per_sample, int student_pred, llie_stream stream);
/* Classifier-free guidance (csrc/guidance.hip), elementwise on device fp32 [batch, per_sample] tensors (the kernels know nothing
 * of H x W).  The null condition is the all-zero image in the model's range (positive-zero bits): a constant, not a parameter.
 *   llie_guide:          out = out_uncond + w (out_cond - out_uncond) for a network output of either prediction type; the
 *                        difference, the product and the sum are each rounded on their own (no fused multiply-add).  w is
 *                        w_rows[b] (device fp32 [batch]) when `w_rows` is non-NULL, the host scalar `w` otherwise.  `out` may alias
 *                        `out_cond` (or `out_uncond`).
 *   llie_guidance_pair:  latents2 [2 batch] = the latents twice; cond2 [2 batch] = `cond` followed by `batch` null rows: in one
 *                        launch, the input of one 2 batch-row denoiser pass whose rows b and b + batch are the conditional and
 *                        the unconditional output of sample b.  The outputs must not overlap the inputs.
 *   llie_cond_dropout:   out[b] = u[b] < p ? null row : in[b] (strictly; `u` device fp32 [batch], uniform in [0, 1); the
 *                        comparison is made in fp32).  A select, not a multiply: inf / NaN of a dropped row give 0.  `out` may
 *                        alias `in`.  The same call masks a gradient: dropped rows of d(cond) are zero.
 * 16-byte accesses where the pointers and per_sample allow (all pointers 16-byte aligned and per_sample % 4 == 0, or one row),
 * scalar ones for the tail and otherwise; the bits do not depend on it.  LLIE_ERR_ARG before any launch for a null pointer (`w_rows`
 * excepted), a pointer that is not 4-byte aligned, batch <= 0, per_sample <= 0, a non-finite `w` (when it is used) or `p`, and a
 * `p` outside [0, 1].
 *
 * Guidance rescale (Lin et al., "Common Diffusion Noise Schedules and Sample Steps are Flawed", section 3.4): guidance at a useful
 * scale inflates the standard deviation of the guided output, which a zero-terminal-SNR table hands straight to x0;
 * llie_guide_rescale scales the guided output of each row back towards the standard deviation of its conditional output.  For row b
 * of [batch, n] tensors, n = per_sample (the whole C H W of an image), phi an fp32 value in [0, 1]:
 *   g     = out_uncond + w (out_cond - out_uncond), llie_guide's three separately rounded fp32 operations (w: as in llie_guide)
 *   S1c = sum out_cond, S2c = sum out_cond^2, S1g = sum g, S2g = sum g^2 over the row in double, each fp32 value widened first
 *   var_c = max(S2c - S1c^2 / n, 0), var_g likewise (the ratio is the same for the biased and the unbiased estimator)
 *   r32   = (float)sqrt(var_c / var_g) (double, rounded once); 1 where var_g is not > 0 or r32 is not finite: a constant row and
 *           n = 1 are not rescaled and never give an inf
 *   f_b   = fl(fl(phi r32) + fl(1 - phi)), three fp32 operations, no fused multiply-add;   out = fl(f_b g);   factor[b] = f_b
 * phi = 1 matches the standard deviations fully; phi = 0 is llie_guide: guide_kernel alone is launched, factor = 1, the same bits.
 * Otherwise three launches, no atomics, no host synchronisation, no allocation: the moments (one workgroup per row and chunk of
 * llie_guide_rescale_chunk() elements leaves four double partials in `scratch`), the factor (one workgroup per row adds them in
 * ascending chunk order) and the apply pass (llie_guide's items, one more rounding).  The partition of a row depends on per_sample
 * alone, so a row's factor and output are the same bits alone or in a batch, from run to run, and whichever accesses carried them.
 * `out` may alias `out_cond` or `out_uncond`; `factor` (device fp32 [batch]) may be NULL; `scratch` holds at least
 * llie_guide_rescale_scratch_bytes(batch, per_sample) bytes (negative: the shape is refused) and is 8-byte aligned.  guidance.py has
 * the float64 definition (guide_rescale_host) and the fp32 twin (guide_rescale_array).
 * LLIE_ERR_ARG before any HIP call for a null pointer (`w_rows` and `factor` excepted), a pointer that is not 4-byte aligned
 * (`scratch`: 8-byte), batch < 1, per_sample < 1, a non-finite `w` when it is used, a `phi` that is not finite or outside [0, 1] and
 * more than 2^31 - 1 workgroups; LLIE_ERR_WORKSPACE for scratch_bytes below llie_guide_rescale_scratch_bytes. */
int64_t llie_guide_rescale_chunk(void);
int64_t llie_guide_rescale_scratch_bytes(int batch, int64_t per_sample);
int llie_guide_rescale(const float* out_cond, const float* out_uncond, const float* w_rows, float w, float phi, float* out,
                       float* factor, void* scratch, int64_t scratch_bytes, int batch, int64_t per_sample, llie_stream stream);
int llie_guide(const float* out_cond, const float* out_uncond, const float* w_rows, float w, float* out, int batch,
               int64_t per_sample, llie_stream stream);
int llie_guidance_pair(const float* latents, const float* cond, float* latents2, float* cond2, int batch, int64_t per_sample,
                       llie_stream stream);
int llie_cond_dropout(const float* in, const float* u, float p, float* out, int batch, int64_t per_sample, llie_stream stream);

/* EMA of a parameter set (update_ema, :316-323): ema[i] = ema[i] * decay + (1 - decay) * param[i] over `count` tensors in
 * one launch.  The table (device pointers, all fp32 and valid for the object's life) is built once by create. */
typedef struct llie_ema llie_ema;
int llie_ema_create(float* const* ema, const float* const* params, const int64_t* numel, int count, llie_ema** out);
int llie_ema_update(llie_ema* ema, double decay, llie_stream stream);
void llie_ema_destroy(llie_ema* ema);

/* LCMScheduler.step (lcm_scheduler.py:176-253), elementwise on fp32 [n]:
 *   x0 = (sample - sqrt_beta_t*model_output)/sqrt_alpha_t      (epsilon)
 *   prev = is_last ? x0 : sqrt_alpha_prev*x0 + sqrt_beta_prev*noise
 * `noise` may be null when is_last.  `x0_out` and `clamped_out` (prev.clamp(-1,1),
 * low_light_diffusion.py:240) are optional (null to skip).
 * coef->sampler == 1 is the deterministic DDIM step instead (the teacher's step of low_light_diffusion.py:365-379):
 *   e    = model_output (epsilon)  |  sqrt_alpha_t*model_output + sqrt_beta_t*sample (v_prediction)
 *   prev = is_last ? x0 : sqrt_alpha_prev*x0 + sqrt_beta_prev*e
 * `noise` is never read and may be null on every step.  Every multiply and add is a separate fp32 operation, as written. */
int llie_lcm_step(const float* model_output, const float* sample, const float* noise, float* prev_out,
                  float* x0_out, float* clamped_out, int64_t n, const llie_step_coef* coef, llie_stream stream);

/* One step of DPM-Solver++ 2M (csrc/solver.hip), the second-order multistep sampler of a many-step model, elementwise on fp32 [n]:
 *   x0   = (sample - sqrt_beta_t*model_output)/sqrt_alpha_t  (epsilon)  |  sqrt_alpha_t*sample - sqrt_beta_t*model_output  (v)
 *   a = k_x*sample;  b = k_0*x0;  s = a + b;        order 2 only:  d = k_1*hist;  s = s + d
 *   prev = is_last ? x0 : s;      hist = x0, written after hist was read;      clamped = prev.clamp(-1, 1)
 * Every multiply and add is a separate fp32 operation, in the order written.  `hist` carries the x0 of one step to the next: an
 * order-1 step only writes it, an order-2 step reads the previous x0 and replaces it.  A thread owns one element (or four), reads
 * it from every input, then writes it: `prev_out` may alias `sample`, and `hist` is updated in place; `hist` must not overlap
 * any other tensor.  `hist` may be NULL only when order == 1 && is_last; `clamped_out` is optional.  16-byte accesses where every
 * pointer is 16-byte aligned, scalar ones for the tail and otherwise; the bits do not depend on it.  No noise is read.
 * LLIE_ERR_ARG before any launch for a null pointer (the optional ones excepted), a pointer that is not 4-byte aligned, n <= 0, an
 * order other than 1 or 2, and a non-finite coefficient. */
int llie_dpm_step(const float* model_output, const float* sample, float* hist, float* prev_out, float* clamped_out, int64_t n,
                  const llie_dpm_coef* coef, llie_stream stream);

/* LCMScheduler.add_noise / get_velocity (lcm_scheduler.py:255-305): per-sample timesteps (device
 * int64[B]) index a device fp32 alpha-bar table [num_train_timesteps]; tensors fp32 [B, per_sample]. */
int llie_add_noise(const float* x0, const float* noise, const int64_t* timesteps, const float* alphas_cumprod,
                   int table_len, float* out, int batch, int64_t per_sample, int velocity, llie_stream stream);
/* A timestep outside [0, table_len) -- an IndexError in the reference -- is never used as an index: that sample's
 * output is NaN (the call is asynchronous and cannot raise; the Python layer validates host-side timesteps). */

/* Whole denoising loop of LowLightDiffusion.enhance (low_light_diffusion.py:204-240) on one stream:
 * `noise` is fp32 [steps,B,3,S,S] in the reference's draw order (initial latents first, then one draw
 * per non-final step); `timesteps_dev` device int64 [steps,B]; `coefs` host array [steps].
 * Outputs: `enhanced` [B,3,S,S] (clamped); optional `intermediates` [steps,B,3,S,S] (post-step,
 * pre-clamp latents, :236-237) and `noise_preds` [steps,B,3,S,S].
 * When the workspace has llie_enhance_workspace_bytes() the launch sequence is captured into a hipGraph
 * on its second use for a given (batch, schedule, workspace, stream) and replayed afterwards; user
 * tensors are staged through the workspace so the graph's pointers never change
 * (LLIE_NO_GRAPH=1 in the environment disables this).  The cache of captured graphs holds at most 16 entries per
 * context; the least recently used one is destroyed when a 17th key appears (llie_graph_cache_entries reads the count).
 * DDIM: when every coefficient has sampler == 1, `noise` is [1,B,3,S,S] -- the initial latents only; nothing past it is read
 * or staged, so the staging area does not grow with `steps` for noise, and a workspace sized for 8 LCM steps holds a DDIM loop
 * of any length without intermediates / noise_preds.  Loops of more than llie_tune("graph_max_steps") steps (default 20) run as
 * plain launches.  A schedule that mixes samplers, or a DDIM coefficient with clamp_x0, returns LLIE_ERR_ARG. */
int llie_enhance(llie_ctx* ctx, const float* low_light, const float* noise, const int64_t* timesteps_dev,
                 const llie_step_coef* coefs, int steps, float* enhanced, float* intermediates,
                 float* noise_preds, int batch, void* workspace, int64_t workspace_bytes, llie_stream stream);

/* llie_enhance on frames of their own size: every [..,3,S,S] above is [..,3,height,width]; the workspace comes from
 * llie_frame_workspace_bytes.  Captured graphs are keyed by the frame size as well and share the context's cache of 16.
 * A shape llie_frame_shape_ok refuses returns LLIE_ERR_SHAPE before anything is launched. */
int llie_enhance_hw(llie_ctx* ctx, const float* low_light, const float* noise, const int64_t* timesteps_dev,
                    const llie_step_coef* coefs, int steps, float* enhanced, float* intermediates, float* noise_preds,
                    int batch, int height, int width, void* workspace, int64_t workspace_bytes, llie_stream stream);

/* The same loop with the DPM-Solver++ 2M sampler: `coefs` host array [steps] of llie_dpm_coef, the first of order 1.  `noise` is
 * [1,B,3,S,S], the initial latents; nothing else is drawn.  Per step: the denoiser, then llie_dpm_step as a plain elementwise launch
 * in every compute dtype (the output head's fused step epilogue is LCM's and DDIM's only).  Outputs, workspace sizes, staging, graph
 * capture (keyed by the coefficient bytes), the branch split, LLIE_NO_GRAPH and the graph_max_steps rule are llie_enhance's; as
 * with DDIM, a workspace sized for 8 LCM steps holds a loop of any length without intermediates / noise_preds.  The loop needs no
 * image beyond the three every workspace query counts: without `intermediates` the latents are updated in place in one and the
 * history lives in the other; with `intermediates` the history takes one of the two.  LLIE_ERR_ARG for a coefficient
 * llie_dpm_step refuses and for a first step of order 2.  llie_enhance_dpm_hw: frames of their own size, as llie_enhance_hw. */
int llie_enhance_dpm(llie_ctx* ctx, const float* low_light, const float* noise, const int64_t* timesteps_dev,
                     const llie_dpm_coef* coefs, int steps, float* enhanced, float* intermediates, float* noise_preds, int batch,
                     void* workspace, int64_t workspace_bytes, llie_stream stream);
int llie_enhance_dpm_hw(llie_ctx* ctx, const float* low_light, const float* noise, const int64_t* timesteps_dev,
                        const llie_dpm_coef* coefs, int steps, float* enhanced, float* intermediates, float* noise_preds,
                        int batch, int height, int width, void* workspace, int64_t workspace_bytes, llie_stream stream);

int llie_graph_cache_entries(const llie_ctx* ctx);

/* Byte-level I/O either side of the path (scripts/inference.py:99-134), on the device:
 *   llie_preprocess_u8:  uint8 HWC RGB [B][H0][W0][3] -> resize to SxS (cv2.INTER_LINEAR geometry, round half
 *                        up to uint8) -> x/127.5 - 1 -> fp32 NCHW [B][3][S][S]
 *   llie_postprocess_u8: fp32 NCHW [B][3][S][S] -> (x+1)*127.5, clip [0,255], truncate to uint8 -> resize to
 *                        H0xW0 -> uint8 HWC RGB [B][H0][W0][3]
 * Bit-exact with the host implementation in hostio.py (fp32 arithmetic without fused multiply-adds). */
int llie_preprocess_u8(const uint8_t* img, int batch, int H0, int W0, float* out, int S, llie_stream stream);
int llie_postprocess_u8(const float* x, int batch, int S, uint8_t* img, int H0, int W0, llie_stream stream);

/* Full-resolution images as overlapping S x S tiles (S = image_size), blended back on the device.
 * The plan of one axis of length L with overlap v (0 <= 2v <= S): one tile at origin 0 when L <= S, otherwise
 * n = ceil((L - S) / (S - v)) + 1 tiles at origins floor(i * (L - S) / (n - 1)), i = 0 .. n-1 (the first starts at 0, the last
 * ends at L).  The tiles of an H x W image are numbered row-major, t = iy * nx + ix; `first` / `count` select the chunk
 * [first, first + count) of them.
 *   llie_tile_count:      n of one axis (host only, no GPU needed)
 *   llie_tile_origins:    writes the n origins of one axis to `out` (host only, no GPU needed)
 *   llie_tile_gather_u8:  uint8 HWC RGB [H][W][3] -> fp32 NCHW tiles [count][3][S][S],
 *                         tile[c][y][x] = img[min(oy + y, H-1)][min(ox + x, W-1)][c] / 127.5 - 1 (llie_preprocess_u8's normalisation;
 *                         the min replicates the edge where the image is smaller than a tile)
 *   llie_tile_gather_f32: fp32 canvas [planes][max(H,S)][max(W,S)], planes = 3 k -> out [k][count][3][S][S],
 *                         out[k][j][c][y][x] = canvas[3 k + c][oy + y][ox + x]: the noise of llie_enhance for a chunk of tiles, cut
 *                         from one canvas so that overlapping tiles see the same noise where they overlap
 *   llie_tile_blend_u8:   fp32 tiles [T][3][S][S] (all T = ny * nx tiles) -> uint8 HWC RGB [H][W][3]: per pixel the mean of the
 *                         covering tiles weighted by w[y] * w[x], w[k] = min(k + 1, S - k, v) / v (1 when v == 0), accumulated in
 *                         ascending tile number, then llie_postprocess_u8's (r + 1) * 127.5, clip [0,255], truncate.
 *   llie_tile_sync_step:  one LCM step of the latent canvas the tiles of an image share (tiling.enhance_tiled(sync="latents")).
 *                         eps_tiles fp32 [T][3][S][S] holds the denoiser's output for all T tiles, each run on its window of
 *                         canvas_in fp32 [3][max(H,S)][max(W,S)].  Per canvas pixel and channel, e = the value of the one covering
 *                         tile, or llie_tile_blend_u8's weighted mean num / den over the covering tiles when there are several;
 *                         then llie_lcm_step's arithmetic on (e, canvas_in, noise) with `coef`, written to canvas_out (which may be
 *                         canvas_in).  noise has the canvas's shape and may be NULL when coef->is_last or coef->sampler == 1 (the DDIM
 *                         step reads none).  img (or NULL; meaningful on
 *                         the last step): uint8 HWC RGB [H][W][3], llie_tile_blend_u8's bytes of canvas_out for y < H, x < W.
 * Bit-exact with the host implementation in tiling.py (fp32 arithmetic without fused multiply-adds, fixed order, no atomics).
 * v < 0, 2v > S, a non-positive size, a chunk outside the plan, planes not a positive multiple of 3 or a NULL noise on a step
 * that is not the last return LLIE_ERR_ARG. */
int llie_tile_count(int L, int S, int v);
int llie_tile_origins(int L, int S, int v, int* out);
int llie_tile_gather_u8(const uint8_t* img, int H, int W, int S, int v, int first, int count, float* tiles, llie_stream stream);
int llie_tile_gather_f32(const float* canvas, int planes, int H, int W, int S, int v, int first, int count, float* out,
                         llie_stream stream);
int llie_tile_blend_u8(const float* tiles, int H, int W, int S, int v, uint8_t* img, llie_stream stream);
int llie_tile_sync_step(const float* eps_tiles, int H, int W, int S, int v, const float* canvas_in, const float* noise,
                        const llie_step_coef* coef, float* canvas_out, uint8_t* img, llie_stream stream);

/* The same four with rectangular tiles: rows are planned with (H, SH, vy) and columns with (W, SW, vx), each axis by the rule
 * above with its own tile side and overlap (0 <= 2 vy <= SH, 0 <= 2 vx <= SW; llie_tile_count / llie_tile_origins per axis).
 * Tile tensors are [T][3][SH][SW], numbered row-major; the canvas is [..][max(H,SH)][max(W,SW)]; the window is
 * wy[y] * wx[x], wy[k] = min(k + 1, SH - k, vy) / vy (1 when vy == 0) and wx likewise.  Any positive tile sides are taken: the
 * multiple-of-8 rule belongs to the network (llie_frame_shape_ok), not to these byte kernels.  The entries above are these at
 * SH = SW = S, vy = vx = v, to the bit.  Same errors. */
int llie_tile_gather_u8_hw(const uint8_t* img, int H, int W, int SH, int SW, int vy, int vx, int first, int count, float* tiles,
                           llie_stream stream);
int llie_tile_gather_f32_hw(const float* canvas, int planes, int H, int W, int SH, int SW, int vy, int vx, int first, int count,
                            float* out, llie_stream stream);
int llie_tile_blend_u8_hw(const float* tiles, int H, int W, int SH, int SW, int vy, int vx, uint8_t* img, llie_stream stream);
int llie_tile_sync_step_hw(const float* eps_tiles, int H, int W, int SH, int SW, int vy, int vx, const float* canvas_in,
                           const float* noise, const llie_step_coef* coef, float* canvas_out, uint8_t* img, llie_stream stream);

/* Byte-level I/O of frame mode: a uint8 image of any size to the padded fp32 frame llie_enhance_hw takes, and back.
 *   llie_frame_pad:      a side L -> the next multiple of 8, at least 64 (host only)
 *   llie_frame_load_u8:  uint8 HWC RGB [H][W][3] -> fp32 [3][Hp][Wp], Hp / Wp = llie_frame_pad(H / W),
 *                        out[c][y][x] = img[min(y, H-1)][min(x, W-1)][c] / 127.5 - 1: the edge is replicated into the padding,
 *                        as llie_tile_gather_u8 does
 *   llie_frame_store_u8: fp32 [3][Hp][Wp] -> uint8 HWC RGB [H][W][3]: the crop to H x W, then llie_postprocess_u8's
 *                        (x + 1) * 127.5, clip [0,255], truncate
 * Bit-exact with the host implementation in tiling.py (fp32 arithmetic without fused multiply-adds, no atomics).  A NULL pointer
 * or a non-positive size returns LLIE_ERR_ARG. */
int llie_frame_pad(int L);
int llie_frame_load_u8(const uint8_t* img, int H, int W, float* out, llie_stream stream);
int llie_frame_store_u8(const float* x, int H, int W, uint8_t* img, llie_stream stream);

/* Device-resident paired data loader (src/training/dataset.py): the training frames stay on the device as uint8 and one launch
 * per batch crops, flips, rotates or degrades, and normalises them into the fp32 NCHW pair a training step takes.
 *   pool:   uint8, every frame HWC RGB with packed rows;  table: int64 [N][3] = (byte offset into pool, H, W) per frame; every
 *           frame is at least S x S
 *   plan:   one llie_aug_row per sample of the epoch; a call handles rows [first, first + count) and writes sample row - first
 *   low / high: fp32 [count][3][S][S] = byte / 127.5 - 1;  low_u8 / high_u8 (or NULL): uint8 [count][S][S][3], the bytes themselves
 * With crop(yy, xx) = frame[y0 + (vflip ? S-1-yy : yy)][x0 + (hflip ? S-1-xx : xx)]:
 *   aug_pair_u8, the same for frames low_frame and high_frame: without LLIE_AUG_ROTATE byte = crop(y, x); with it the crop is
 *           rotated about its centre c = (S-1)/2 by the angle whose cosine and sine are (ca, sa): xs = (ca*u + sa*v) + c,
 *           ys = (-sa*u + ca*v) + c with u = x - c, v = y - c, bilinear over the four neighbours with reflect-101 borders,
 *           byte = clip(floor(value + 0.5), 0, 255).  |angle| <= 15 degrees.
 *   aug_synth_u8 (SyntheticLowLightDataset._create_low_light), frame high_frame, hflip only: normal byte nb = crop(y, x);
 *           n = clamp(powf(nb / 255, gamma) + level * z, 0, 1); n = clamp(n * scale[c], 0, 1); low byte = trunc(n * 255);
 *           z: fp32 [count][S][S][3] standard-normal draws of the caller.
 * fp32 arithmetic without fused multiply-adds, no atomics: aug_pair_u8 is bit-exact with augment_pairs_host in data.py,
 * aug_synth_u8 with augment_synth_host up to the rounding of powf.  Frame indices and crop origins are clamped into the store,
 * so a corrupt plan row gives wrong pixels and never a read outside the pool.  A NULL pointer other than the optional two,
 * N < 1, S < 1, first < 0 or count < 0 return LLIE_ERR_ARG; count == 0 launches nothing. */
enum { LLIE_AUG_HFLIP = 1, LLIE_AUG_VFLIP = 2, LLIE_AUG_ROTATE = 4 };
typedef struct llie_aug_row {
  int32_t low_frame, high_frame; /* frame indices */
  int32_t y0, x0;                /* crop origin */
  int32_t flags;                 /* LLIE_AUG_* */
  float ca, sa;                  /* cos, sin of the rotation angle */
  float gamma, level;            /* synthetic: exponent, noise standard deviation */
  float scale[3];                /* synthetic: per-channel colour shift, (1, 1, 1) = none */
} llie_aug_row;
int llie_aug_pair_u8(const uint8_t* pool, const int64_t* table, int N, const llie_aug_row* plan, int first, int count, int S,
                     float* low, float* high, uint8_t* low_u8, uint8_t* high_u8, llie_stream stream);
int llie_aug_synth_u8(const uint8_t* pool, const int64_t* table, int N, const llie_aug_row* plan, int first, int count, int S,
                      const float* z, float* low, float* high, uint8_t* low_u8, uint8_t* high_u8, llie_stream stream);
/* The same two on rectangular crops of SH rows x SW columns (frame-size training); the entry points above are these at
 * SH = SW = S, with the same bits.  low / high: fp32 [count][3][SH][SW]; the optional bytes and z: [count][SH][SW][3].
 *   crop(yy, xx) = frame[y0 + (vflip ? SH-1-yy : yy)][x0 + (hflip ? SW-1-xx : xx)]; origins are clamped into
 *   [0, H_frame - SH] x [0, W_frame - SW]; the rotation is about (cx, cy) = ((SW-1)/2, (SH-1)/2): u = x - cx, v = y - cy,
 *   xs = (ca*u + sa*v) + cx, ys = (-sa*u + ca*v) + cy; reflect-101 and the clamp act per axis with that axis's length. */
int llie_aug_pair_u8_hw(const uint8_t* pool, const int64_t* table, int N, const llie_aug_row* plan, int first, int count, int SH,
                        int SW, float* low, float* high, uint8_t* low_u8, uint8_t* high_u8, llie_stream stream);
int llie_aug_synth_u8_hw(const uint8_t* pool, const int64_t* table, int N, const llie_aug_row* plan, int first, int count, int SH,
                         int SW, const float* z, float* low, float* high, uint8_t* low_u8, uint8_t* high_u8, llie_stream stream);

/* Image quality: per image of a against b, out3 [batch][3] doubles = {mse, psnr, ssim}.  All arithmetic is float64 on the mapped
 * values: x = (v - lo) / (hi - lo) for fp32 NCHW [batch][3][H][W] (the model's range is lo = -1, hi = 1), x = byte / 255 for uint8
 * HWC [batch][H][W][3].
 *   window   g[k] = exp(-(k - 5)^2 / (2 * 1.5^2)), k = 0 .. 10, normalised to sum 1; the 2-D window is the outer product, applied
 *            along the rows, then along the columns
 *   ssim     (Wang et al. 2004, on RGB, no luma conversion) at each of the (H - 10) x (W - 10) positions whose 11 x 11 window lies
 *            inside the image and for each channel: weighted means mx, my; biased variances sx2 = sum w x^2 - mx^2, sy2 likewise,
 *            sxy = sum w x y - mx my;  map = (2 mx my + C1)(2 sxy + C2) / ((mx^2 + my^2 + C1)(sx2 + sy2 + C2)), C1 = 1e-4, C2 = 9e-4;
 *            ssim = mean of the map over the 3 channels and all those positions
 *   mse      mean of (x - y)^2 over all 3 H W values;  psnr = -10 log10(mse), +inf when mse == 0
 * Tiles of 16 x 32 positions write partial sums into `scratch`; a second launch adds an image's partials in a fixed order.  No
 * atomics: results are bitwise reproducible and an image's triple is the same bits alone or in a batch.  The host implementation
 * in metrics.py is the definition; the two differ only in summation order.
 * Checked before any HIP call: a NULL pointer, batch < 1, lo == hi (or not finite) return LLIE_ERR_ARG; H < 11 or W < 11
 * LLIE_ERR_SHAPE; scratch_bytes below llie_image_metrics_scratch_bytes LLIE_ERR_WORKSPACE. */
int64_t llie_image_metrics_scratch_bytes(int batch, int H, int W);
int llie_image_metrics_f32(const float* a, const float* b, int batch, int H, int W, float lo, float hi, double* out3, void* scratch,
                           int64_t scratch_bytes, llie_stream stream);
int llie_image_metrics_u8(const uint8_t* a, const uint8_t* b, int batch, int H, int W, double* out3, void* scratch,
                          int64_t scratch_bytes, llie_stream stream);

/* SSIM as a training loss: the SSIM of the definition above in fp32 (sums over tiles and images in double) with its gradient
 * with respect to the first image, and the x0 term of a training step built on it.  At a valid position, with the five filtered
 * maps mx, my, xx, yy, xy and sx = xx - mx^2, sy = yy - my^2, sxy = xy - mx my, A1 = 2 mx my + C1, A2 = 2 sxy + C2,
 * B1 = mx^2 + my^2 + C1, B2 = sx + sy + C2, S = A1 A2 / (B1 B2):
 *   dmx = (2 my A2 - 2 my A1) / (B1 B2) - S (2 mx / B1 - 2 mx / B2),   dxx = -S / B2,   dxy = 2 A1 / (B1 B2)
 *   dSSIM/dx = [W^T(dmx) + 2 x W^T(dxx) + y W^T(dxy)] / (3 (H - 10) (W - 10)),   dSSIM/da = dSSIM/dx / (hi - lo)
 * with W^T the transposed window filter (a full correlation, zero outside the valid region, H x W).
 *   llie_ssim_grad_f32:  a, b fp32 NCHW [batch][3][H][W] in (lo, hi) -> ssim_out [batch] fp32 and, unless da is NULL,
 *                        da = upstream_b * dSSIM_b/da (stored); upstream is device fp32 [batch] or NULL (= 1).  ssim_out is the
 *                        same bits with and without da.
 *   llie_x0_loss:        out (the network output), x_t (the noised input), normal (the normal-light image) fp32 NCHW
 *                        [batch][3][H][W]; t device int64 [batch]; alphas_cumprod device fp32 [table_n]; abar = alphas_cumprod[t_b],
 *                        alpha = sqrt(abar), sigma = sqrt(1 - abar).  The predicted clean image is x^ = p x_t + q out, not clamped:
 *                        p = 1 / alpha, q = -sigma / alpha (velocity == 0, epsilon prediction) or p = alpha, q = -sigma
 *                        (velocity != 0, v prediction).  With w_b = abar_b and the data range (-1, 1):
 *                          *loss_out = (1 / B) sum_b w_b [lambda_s (1 - SSIM_b(x^, normal)) + lambda_1 mean|x^_b - normal_b|]
 *                          d_out    += (w_b / B) q_b [-lambda_s / 2 dSSIM_b/dx + lambda_1 sign(x^ - normal) / (3 H W)]
 *                        (d_out may be NULL: the loss alone).  A sample with abar == 0 (the last step of a zero-SNR table)
 *                        contributes exactly 0 to the loss and its rows of d_out are not written; 1 / alpha is not evaluated.
 * Four (three) launches on the stream, no atomics, no host synchronisation: every gradient element has one writer and the order
 * of every sum depends on H and W alone, so results are bitwise reproducible and an image's values are the same alone or in a
 * batch.  The host implementations are metrics.ssim_grad_host and pipeline.x0_loss_host (float64).
 * Checked before any HIP call: a NULL pointer (other than upstream, da, d_out), batch < 1, lo == hi or not finite, a negative or
 * non-finite lambda, table_n < 1 return LLIE_ERR_ARG; H < 11 or W < 11 LLIE_ERR_SHAPE; scratch_bytes below
 * llie_ssim_grad_scratch_bytes LLIE_ERR_WORKSPACE.  The timesteps live on the device and are not read by the host: one outside
 * [0, table_n) never indexes the table and makes that sample's loss and gradient NaN, as llie_add_noise does. */
int64_t llie_ssim_grad_scratch_bytes(int batch, int H, int W);
int llie_ssim_grad_f32(const float* a, const float* b, int batch, int H, int W, float lo, float hi, const float* upstream,
                       float* ssim_out, float* da, void* scratch, int64_t scratch_bytes, llie_stream stream);
int llie_x0_loss(const float* out, const float* x_t, const float* normal, const int64_t* t, const float* alphas_cumprod, int table_n,
                 int velocity, float lambda_s, float lambda_1, float* loss_out, float* d_out, int batch, int H, int W, void* scratch,
                 int64_t scratch_bytes, llie_stream stream);

/* The noise-space training loss with a per-sample Min-SNR-gamma weight (Hang et al., ICCV 2023; `gamma` is the snr_gamma of
 * TrainStep, compute_loss and scripts/train.py), its per-sample values and d(loss)/d(pred) in one read of pred and target and
 * one write of the gradient (csrc/snrloss.hip).
 *   pred, target     fp32 [batch][per_sample], any per_sample >= 1 (the network's is 3 H W);  d = pred - target
 *   t                device int64 [batch];  alphas_cumprod device fp32 [table_n];  abar = alphas_cumprod[t_b]
 *   loss_type        LLIE_LOSS_MSE    l(d) = d^2                                          l'(d) = 2 d
 *                    LLIE_LOSS_L1     l(d) = |d|                                          l'(d) = sign(d), sign(0) = 0 as torch.sign
 *                    LLIE_LOSS_HUBER  l(d) = 0.5 d^2 where |d| < 1, else |d| - 0.5        l'(d) = clamp(d, -1, 1)      (delta = 1)
 *   velocity == 0    w_b = 1 if abar == 0, otherwise min(1, (gamma (1 - abar)) / abar): min(SNR, gamma) / SNR with
 *                    SNR = abar / (1 - abar), whose limit is 1 on the zero-SNR step
 *   velocity != 0    w_b = min(abar, gamma (1 - abar)): min(SNR, gamma) / (SNR + 1) without a division, exactly 0 at abar == 0
 *   sample_loss[b]   m_b = (1 / n) sum_i l(d_bi), n = per_sample: unweighted, so it can be logged per timestep (optional)
 *   weight[b]        w_b (optional)
 *   *loss_out        (1 / B) sum_b w_b m_b; with every w_b = 1 this is F.mse_loss / F.l1_loss / F.huber_loss
 *   d_pred[b][i]     l'(d_bi) c_b, c_b = (w_b / (float)B) / (float)n; stored, not accumulated; must not overlap pred or target
 *                    (optional: without it the call returns the loss alone, the same bits)
 * The weight, c_b, d and l'(d) c_b are each separate fp32 operations in the order written, no fused multiply-add, so the host fp32
 * twin (snrloss.snr_loss_f32) gives the bits of `weight` and `d_pred`; every n the engines accept converts to float exactly (the
 * cap 3 * 5 592 405 = 2^24 - 1).  snrloss.snr_loss_host is the definition in float64.
 * Two launches on the stream, no atomics, no host synchronisation.  Pass 1: one workgroup per (sample, chunk of
 * llie_snr_loss_chunk() elements) leaves one fp32 partial in `scratch`; 16-byte accesses where pred, target, d_pred and every row
 * start are 16-byte aligned, scalar ones otherwise and for the tail, with the same bits either way.  Pass 2: one workgroup adds a
 * sample's partials in ascending chunk order, then the samples in ascending order, in double.  The order of every sum depends on
 * per_sample alone (m_b) or on batch alone (the total): m_b is the same bits for a sample alone or in a batch, and from run to run;
 * every gradient element has one writer.
 * A t_b outside [0, table_n) never indexes the table: that sample's weight, its rows of d_pred and *loss_out are NaN (its
 * sample_loss stays what it is), the convention of llie_add_noise and llie_x0_loss.
 * Checked before any HIP call: a NULL pred, target, t, alphas_cumprod, loss_out or scratch, an fp32 pointer that is not 4-byte
 * aligned (t, scratch: 8-byte), batch < 1, per_sample < 1, table_n < 1, an unknown loss_type, a gamma that is not finite or <= 0,
 * more than 2^31 - 1 workgroups return LLIE_ERR_ARG; scratch_bytes below llie_snr_loss_scratch_bytes LLIE_ERR_WORKSPACE. */
#define LLIE_LOSS_MSE 0
#define LLIE_LOSS_L1 1
#define LLIE_LOSS_HUBER 2
int64_t llie_snr_loss_chunk(void);
int64_t llie_snr_loss_scratch_bytes(int batch, int64_t per_sample);
int llie_snr_loss(const float* pred, const float* target, const int64_t* t, const float* alphas_cumprod, int table_n,
                  int loss_type, int velocity, float gamma, float* loss_out, float* sample_loss, float* weight,
                  float* d_pred, int batch, int64_t per_sample, void* scratch, int64_t scratch_bytes, llie_stream stream);

/* The trainer's per-epoch sample sheet (LowLightTrainer.generate_samples / _save_comparison, src/training/trainer.py:365-410):
 * torchvision's make_grid(cat([low, enhanced, normal]), nrow=n) with its defaults (padding 2, pad value 0) followed by
 * save_image's quantisation, in one launch.
 *   low / enhanced / normal: fp32 NCHW [n][3][H][W] in the model's range (-1, 1)
 *   grid: uint8 HWC RGB [3 (H+2) + 2][n (W+2) + 2][3].  The image of row r (0 low, 1 enhanced, 2 normal) and column k has its
 *         top-left pixel at (r (H+2) + 2, k (W+2) + 2); every other byte is 0.
 *   byte: v = (x + 1.0f) / 2.0f; q = v * 255.0f + 0.5f; q = min(max(q, 0), 255) (NaN -> 0); (uint8) trunc(q)
 * Separate fp32 operations without fused multiply-adds: bit-exact with comparison_grid_host in trainer.py, which is the definition
 * (written from torchvision's documented algorithm; torchvision itself is not available to pin it against).
 * Checked before any HIP call: a NULL pointer or n, H, W < 1 return LLIE_ERR_ARG. */
int llie_comparison_grid_u8(const float* low, const float* enhanced, const float* normal, int n, int H, int W, uint8_t* grid,
                            llie_stream stream);

/* ---- Kernel-level entry points (unit tests and tuning; SURVEY.md 8b "per-kernel entry points").
 * Activations are NHWC rows in the compute dtype T (llie_dtype); see DESIGN.md section 3.
 *
 * llie_pw_gemm: out[M][N] = sum over K-segments act(A_seg * scale + bias) . W[N][K]^T (+bias[N]) (+residual)
 *   -- the 1x1 convolutions efficient_unet.py:174,186,199,265-267 with their fused prologue/epilogue.
 *   scale/bias of a segment are fp32 [M/P][affine_ld] tables (null = identity); act: 0 none, 1 ReLU6, 3 = clamp01 with tables
 *   already divided by 6 and the accumulators times 6 (2-byte dtypes, every segment or none).  Refused with LLIE_ERR_ARG before
 *   any HIP call: any other act (the forward GEMM has no SiLU prologue), an act or a bias table without a scale table (the
 *   prologue runs only where there is one), affine_ld < channels.
 *   stats (optional): fp32 slab [M/P][P/tile_rows][2][N] of per-channel (sum, sum of squares).
 * llie_dwconv3x3: out = depthwise3x3(relu6(in*scale+bias)), weights fp32 [9][C] tap-major
 *   (efficient_unet.py:212-220); pool (optional): fp32 [B][tiles][C] partial sums for the SE average pool. */
typedef struct llie_gemm_seg {
  const void* ptr; int channels; const float* scale; const float* bias; int affine_ld; int act;
} llie_gemm_seg;
int llie_pw_gemm(int dtype, const llie_gemm_seg* segs, int nseg, const void* w, const float* bias, const void* residual,
                 void* out, float* stats, int M, int N, int P, llie_stream stream);
int llie_pw_gemm_tile_rows(int P);
/* llie_pw_expand: the expanding 1x1 conv of the wide InvertedResidualBlocks (efficient_unet.py:174 with norm1 + ReLU6
 *   :207-208 in the prologue, norm2's statistics :212 in the epilogue) in its activation-stationary form (2-byte dtypes;
 *   K in {128, 192, 256, 384, 512}, P a multiple of 128, every segment with act 3 = clamp01 tables already divided by 6):
 *   out[M][N] = sum_seg clamp01(A_seg * scale + bias) . (6 W)^T.  w32 = fp32 [N][K] as saved by the reference; wpack = N*K
 *   elements of T that receive the fragment-ordered copy the engine keeps per layer (w32 == NULL: wpack already holds it,
 *   from an earlier call with the same weights -- the GEMM alone).  stats: as llie_pw_gemm. */
int llie_pw_expand(int dtype, const llie_gemm_seg* segs, int nseg, const float* w32, void* wpack, void* out, float* stats,
                   int M, int N, int P, llie_stream stream);
/* The remaining per-kernel entry points of the hot path.  All tensors are device pointers; activations are NHWC of
 * the compute type `dtype` (0 fp32, 1 fp16, 2 bf16), tables and statistics fp32.
 *
 * llie_groupnorm_finalize: nn.GroupNorm(groups, C) statistics (efficient_unet.py:170-171,263,268,528) from per-tile
 *   (sum, sum of squares) slabs [batch][ntiles][2][ch] of up to two channel segments (a virtual concat) to the per-(image,
 *   channel) affine `scale`, `shift` [batch][C] that consumers apply on load; `film` (or NULL): [rows][2 C] FiLM (1 + scale, shift
 *   folded in, :215-217) with row stride film_stride (0 = one row for all images); post_scale 0 = none.
 * llie_conv3x3: Downsample (:367, mode 0: stride 2, pad 1) / Upsample (:383-384, mode 1: bilinear x2 then 3x3 pad 1) / the plain
 *   stride-1 pad-1 conv (mode 2: what training runs on stored up-sampled tensors, and every input-gradient conv) as implicit GEMM; w [9][Cout][Cin] of the compute type (tap-major), stats (or NULL) [batch][llie_conv3x3_tiles(Ho, Wo)][2][Cout].
 * llie_linattn: LinearAttention core (:288-302) on qkv [batch][N][3 * 32 heads] (q | k | v, head-major channels, dim_head 32):
 *   phi = elu + 1 on q and k, kv = sum_n phi(k) v^T, out = phi(q) kv / (phi(q) . sum_n phi(k) + 1e-6) -> [batch][N][32 heads];
 *   kv_scratch: llie_linattn_splits(N) * batch * heads * 32 * 33 floats.
 * llie_se_mlp: SqueezeExcitation MLP (:96-100): gate = sigmoid(W2 relu6(W1 mean + b1) + b2), mean = pool_sums / pixels;
 *   w1 [Cs][C], w2 [C][Cs] of the compute type; scratch: mean [batch][C], hidden [batch][Cs]; gate out [batch][C].
 * llie_film: all FiLM projections of a network in one launch (:189-192,215): film[r][f] = bf[f] + Wf[f][:] . silu_temb[r][:]. */
int llie_groupnorm_finalize(const float* slab0, int ntiles0, int ch0, const float* slab1, int ntiles1, int ch1, int groups, int pixels,
                            const float* gamma, const float* beta, const float* film, int64_t film_stride, float eps, float post_scale,
                            int batch, float* scale_out, float* shift_out, llie_stream stream);
int llie_conv3x3(int dtype, int mode, const void* in, const void* w, const float* bias, void* out, float* stats, int batch, int Hi, int Wi,
                 int Cin, int Cout, llie_stream stream);
int llie_conv3x3_tiles(int Ho, int Wo);
/* The Upsample conv (:383-384) with the bilinear x2 folded into per-phase 3x3 weights on the low-resolution input: the form the
 * 2-byte inference engines run (knob "upconv_fold").  llie_upconv_fold_weights: fp32 OIHW [C][C][3][3] -> `folded`,
 * llie_upconv_fold_elems(C) = 64 C^2 elements of the compute type (dtype 1 or 2; interior sets [4 phases][9 taps][C][C], then the
 * image-border corrections: 4 x 3 row-edge, 4 x 3 column-edge, 4 corner sets), rounded once.  llie_conv3x3_upfold: the conv on
 * such a blob; Hi % 8 == 0, Wi % 16 == 0, C = 64 or a multiple of 128; stats (or NULL)
 * [batch][llie_conv3x3_upfold_tiles(2 Hi, 2 Wi)][2][C]. */
int64_t llie_upconv_fold_elems(int C);
int llie_upconv_fold_weights(int dtype, const float* w_oihw, void* folded, int C, llie_stream stream);
int llie_conv3x3_upfold(int dtype, const void* in, const void* folded, const float* bias, void* out, float* stats, int batch, int Hi, int Wi,
                        int C, llie_stream stream);
int llie_conv3x3_upfold_tiles(int Ho, int Wo);
/* The same conv from nine low-resolution tap maps (knob "upconv_maps"): Z_t = W_t x for the nine taps, kept on chip, and the output is
 * bias + the sum of the bilinear x2 of Z_t at tap t's position over the taps inside the image -- a quarter of the multiply-adds.  `w` =
 * the plain [9][C][C] weights of llie_conv3x3 in the compute type (dtype 1 or 2), no folded blob; Hi % 8 == 0, Wi % 16 == 0, C a
 * multiple of 32 (llie_conv3x3_upmaps_supported: 1 where the kernel accepts the shape); stats (or NULL)
 * [batch][llie_conv3x3_tiles(2 Hi, 2 Wi)][2][C], every entry written.  The maps are rounded to the compute type once.
 * llie_tune("upconv_maps", v), default 1: of the up-sampling convs that "upconv_fold" covers, 2-byte inference engines run those of 128
 * and 256 channels this way; 0 = what "upconv_fold" alone picks, the launches and bits from before this form existed.
 * The kernel's grid is sized to the chip: a work item is (image, 8 x 16 low-resolution tile, 32 output channels), and workgroup g of n
 * works through items g, g + n, ...  llie_conv3x3_upmaps_workgroups: the n that llie_conv3x3_upmaps launches for that shape on the
 * current device = min(items, compute units), or one workgroup per item where the compute units are no multiple of 8; LLIE_ERR_ARG for
 * batch < 1 or a shape no dtype is accepted at, minus the runtime's error code where no device answers (a count is positive).
 * llie_conv3x3_upmaps_grid: the same launch on min(workgroups, items) workgroups, workgroups 0 = that rule (llie_conv3x3_upmaps is
 * this case), negative = LLIE_ERR_ARG before any launch.  Which workgroup computes an item changes no bit of the output or the
 * statistics, so every count gives the same result; the tests use it to walk the item loop at small shapes. */
int llie_conv3x3_upmaps(int dtype, const void* in, const void* w, const float* bias, void* out, float* stats, int batch, int Hi, int Wi,
                        int C, llie_stream stream);
int llie_conv3x3_upmaps_grid(int dtype, const void* in, const void* w, const float* bias, void* out, float* stats, int batch, int Hi,
                             int Wi, int C, int workgroups, llie_stream stream);
int llie_conv3x3_upmaps_workgroups(int batch, int Hi, int Wi, int C);
int llie_conv3x3_upmaps_supported(int dtype, int Hi, int Wi, int C);
int llie_linattn(int dtype, const void* qkv, float* kv_scratch, void* out, int batch, int N, int heads, llie_stream stream);
int llie_linattn_splits(int N);
int llie_se_mlp(int dtype, const float* pool_sums, int pixels, const void* w1, const float* b1, const void* w2, const float* b2, float* mean_scratch,
                float* hidden_scratch, float* gate, int batch, int C, int Cs, llie_stream stream);
int llie_film(const float* silu_temb, const float* wf, const float* bf, float* film, int rows, int T, int F, llie_stream stream);
/* llie_pw_expand_nsplit: the channel split llie_pw_expand takes for M = batch x pixels rows and N output channels (its grid is M / 128 x
 *   this many workgroups); M a multiple of 128, N of 64, else LLIE_ERR_ARG.
 * llie_silu_rows: out[i] = silu(in[i]) on n fp32 values (the time embedding before llie_film, forward and backward). */
int llie_pw_expand_nsplit(int M, int N);
int llie_silu_rows(const float* in, float* out, int64_t n, llie_stream stream);

/* The network's first and last kernels, the SE gate of the inference blocks, the attention tail, the layout converters and the
 * backward pass's GEMM epilogue.  Every contract clause below is checked before any HIP call and answered with LLIE_ERR_ARG.
 * llie_init_conv: init_conv (efficient_unet.py:420,553) on the virtual concat of two fp32 NCHW halves x0 [batch][c0][H][W] and x1
 *   [batch][c1][H][W] (x1 NULL exactly when c1 == 0; 1 <= c0, c0 + c1 <= 8) -> out NHWC [batch][H][W][Cout] of the compute type, plus
 *   (stats, optional) the statistics slab [batch][llie_init_conv_tiles(H, W, use_mfma)][2][Cout] of the stored values: tiles of 16 x
 *   16 pixels, or 8 rows x 32 columns with use_mfma, row-major, pixels past the image counting for nothing.  w_oihw fp32 [Cout][c0 +
 *   c1][3][3] and bias fp32 [Cout] as the reference holds them: the call zero-fills `pack` (llie_init_conv_pack_bytes(c0 + c1,
 *   Cout) bytes, 16-byte aligned) and repacks into it as llie_load_param does.  use_mfma 0: the VALU kernel (any dtype; fp32 operands);
 *   1: the MFMA kernel of the 2-byte engines (inputs and weights rounded to the compute type).  Refused: H or W not a multiple of 8,
 *   Cout not a multiple of 32, batch > 65535, use_mfma with LLIE_F32, a pack that is short or misaligned, NULL tensors.
 * llie_init_conv_dgrad: the data gradient of init_conv, as llie_unet_backward_dx launches it: g NHWC [batch][H][W][Cout] of the
 *   compute type (the gradient of init_conv's output) -> d_x0 fp32 NCHW [batch][c0][H][W] and d_x1 [batch][c1][H][W], the gradients
 *   of llie_init_conv's two halves: d_x[ci][y][x] = sum over ky, kx, co of g[y + 1 - ky][x + 1 - kx][co] w[co][ci][ky][kx], terms
 *   outside the map zero.  Either output may be NULL (not both; d_x1 only with c1 > 0): its channels are neither computed nor
 *   stored.  Values are stored, not accumulated; fp32 accumulation in an order that depends on Cout alone.  w_oihw fp32 [Cout][c0 +
 *   c1][3][3]: the call zero-fills `pack` (llie_init_conv_pack_bytes(c0 + c1, Cout) bytes, 16-byte aligned) and repacks the fp32
 *   table of the forward's VALU kernel into it, which is what the kernel reads.  Refused: a dtype outside 0..2, NULL g / w_oihw /
 *   pack, c0 < 1, c1 < 0, c0 + c1 > 8, H or W not a multiple of 8, batch > 65535, Cout not a positive multiple of 32, a pack that
 *   is short or misaligned.
 * llie_final_conv: the output head (:528-530,600-602): out fp32 NCHW [batch][Cout][H][W] = conv3x3(silu(in * scale + shift)) + bias,
 *   zero padding after the activation; in NHWC [batch][H][W][C] of the compute type, C a multiple of 32, scale / shift fp32
 *   [batch][C], w_oihw fp32 [Cout][C][3][3], 1 <= Cout <= 4, bias fp32 [Cout]; pack: llie_final_conv_pack_bytes(C) bytes, as above.
 *   coef non-NULL (use_mfma only) fuses llie_lcm_step into the epilogue: sample / noise / prev / clamped fp32 [batch][Cout][H][W],
 *   noise may be NULL when is_last, clamped and then also out may be NULL.  Without coef, out is required and the four must be NULL.
 * llie_se_gate: gate [batch][C] = sigmoid(W2 relu6(W1 mean + b1) + b2) from the depthwise kernels' fixed-point channel totals
 *   (int64 [batch][C], mean = total / (pixels 2^24)); w1 [Cs][C], w2 [C][Cs] of the compute type, b1 / b2 fp32.  path 0: one launch
 *   (C a multiple of 64 in fp32, 128 otherwise; (C + Cs) * 4 <= 48 KiB); path 1: the row-parallel pair, hidden_scratch fp32
 *   [batch][Cs] (C, Cs <= 4096); path 2: the MFMA pair (2-byte types, C a multiple of 256 and >= 512, Cs a multiple of 64 in [64,
 *   512]), pre_scratch int64 [batch][Cs], zero-filled by the call.  The mean is never stored on these paths.
 * llie_affine_add: y = x * scale + shift (+ res) on NHWC rows [M][C] (scale / shift fp32 [M / P][C], C a multiple of 8, <= 2048, M a
 *   multiple of P), plus (optional) y's statistics slab [M / P][ceil(P / 64)][2][C].
 * llie_nchw_to_nhwc: channels [coff, coff + C) of x fp32 [batch][Csrc][P] -> y [batch][P][C] of the compute type, plus (optional) its
 *   statistics slab [batch][P / 64][2][C]; llie_nhwc_to_nchw: x [batch][P][C] -> channels [coff, coff + C) of y fp32
 *   [batch][Cdst][P], the others untouched.  C a multiple of 32, P of 64, coff + C within Csrc / Cdst.
 * llie_pw_gemm_dot: llie_pw_gemm without a residual, with the epilogue of the backward pass: dot [M][N] of the compute type and the
 *   (mandatory) slab, which then holds (sum out * dot, sum out) per tile instead of (sum, sum of squares). */
int64_t llie_init_conv_pack_bytes(int Cin, int Cout);
int llie_init_conv_tiles(int H, int W, int mfma);
int llie_init_conv(int dtype, const float* x0, int c0, const float* x1, int c1, const float* w_oihw, const float* bias, void* out, float* stats,
                   int batch, int H, int W, int Cout, int use_mfma, void* pack, int64_t pack_bytes, llie_stream stream);
int llie_init_conv_dgrad(int dtype, const void* g, int Cout, const float* w_oihw, float* d_x0, int c0, float* d_x1, int c1, int batch,
                         int H, int W, void* pack, int64_t pack_bytes, llie_stream stream);
int64_t llie_final_conv_pack_bytes(int C);
int llie_final_conv(int dtype, const void* in, const float* scale, const float* shift, const float* w_oihw, const float* bias, float* out,
                    int batch, int H, int W, int C, int Cout, int use_mfma, const llie_step_coef* coef, const float* sample, const float* noise,
                    float* prev, float* clamped, void* pack, int64_t pack_bytes, llie_stream stream);
int llie_se_gate(int dtype, const unsigned long long* totals, int pixels, const void* w1, const float* b1, const void* w2, const float* b2,
                 float* gate, int batch, int C, int Cs, int path, float* hidden_scratch, long long* pre_scratch, llie_stream stream);
int llie_affine_add(int dtype, const void* x, const float* scale, const float* shift, const void* res, void* y, float* stats, int M, int C, int P,
                    llie_stream stream);
int llie_nchw_to_nhwc(int dtype, const float* x, void* y, float* stats, int batch, int C, int P, int Csrc, int coff, llie_stream stream);
int llie_nhwc_to_nchw(int dtype, const void* x, float* y, int batch, int C, int P, int Cdst, int coff, llie_stream stream);
int llie_pw_gemm_dot(int dtype, const llie_gemm_seg* segs, int nseg, const void* w, const float* bias, const void* dot, void* out,
                     float* stats, int M, int N, int P, llie_stream stream);

/* ---- Backward kernels of the training step (bwd.hip, wgrad.hip), one entry point each, with the conventions above: dtype 0 / 1 / 2,
 * NHWC activations and activation gradients of the compute type, fp32 tables and parameter gradients, device pointers.  Every
 * entry point returns LLIE_ERR_ARG for a bad argument before it makes any HIP call.
 *
 * llie_wgrad: weight gradient of a 1x1 conv, or of a 3x3 conv (ntap 9: all taps; ntap 1: the single tap (dy, dx) in -1..1) --
 *   out[n*ldn + k*ldk + off (+ tap)] = sum_m g[m][n] * A'[src(m)][k] for n < nstore, k < kstore (0 = all), A' = act(A_seg * scale +
 *   bias) rounded to the compute type (up to 3 K-segments as llie_pw_gemm; act 0 none, 1 ReLU6, 2 SiLU), m = (b, y, x) over
 *   Ho x Wo, src(m) = input pixel (y*stride + dy, x*stride + dx) of an Hi x Wi map (zero outside).  g: [batch*Ho*Wo][N];
 *   N and every segment's channels multiples of 32.  The pixel rows are split msplit ways (0: llie_wgrad_msplit with
 *   ragged_rule = (Ho*Wo % 64 != 0)) into partial [msplit][ntap][N][K] fp32 (llie_wgrad_partial_floats), summed in split order.
 * llie_wgrad_msplit: the split the engine takes for these sizes: ragged_rule 0 = the rule at image sizes that are multiples of
 *   64, 1 = the rule of every other image size.
 * llie_dw_wgrad: depthwise 3x3 weight gradient out[c][tap] (reference layout [C][1][3][3]) = sum over (b, y, x) of
 *   (g*gs + gb) * relu6(h*scale + shift) at the tap's input pixel; gs / gb (or NULL) and scale / shift are [batch][C];
 *   C a multiple of 32 (fp32) or 64 (2-byte); partial: batch * llie_dw_wgrad_strips(H, W) * 9 * C floats.
 * llie_groupnorm_backward: one GroupNorm(32, C) site of the backward pass as the engine runs it, for
 *   y = act((xhat * gamma + beta) * (1 + s) + f) with the forward record (scale / shift = the affine x*scale + shift of
 *   llie_groupnorm_finalize, mean / rstd [batch][32]): dz = g * act' (stored over dz, which may alias g; act 0 none, 1 ReLU6,
 *   2 SiLU), dgamma / dbeta [C], with FiLM rows (film[b][c] = s, film[b][C + c] = f, row stride film_stride) also dfilm
 *   (same layout; NULL = not wanted), and dx = d/dx (+ add0, dense [M][C]) (+ add1, split like x), written to dx0 / dx1.  x0 / x1:
 *   a virtual concat of c0 + c1 channels (c1 = 0: no x1).  scratch: llie_groupnorm_backward_scratch_floats floats.
 * llie_linattn_backward: gradient dqkv [batch][N][3 * 32 heads] of llie_linattn w.r.t. its qkv, given d(out); kv_scratch: what
 *   llie_linattn left there for the same qkv; dkv_scratch: llie_linattn_dkv_floats floats (the per-64-position partials
 *   [batch][heads][ceil(N/64)][32][33], then their sum).
 * llie_softattn: StandardAttention core (:349-353), out = softmax(q k^T / sqrt(32)) v per head, on the qkv layout of llie_linattn
 *   ([batch][N][3 * 32 heads], q | k | v head-major) -> out [batch][N][32 heads]; fused (flash form) on MFMA, any N >= 1; lse_or_NULL:
 *   [batch][heads][N] fp32 log-sum-exp of the scaled logits, which llie_softattn_backward needs.  Bitwise reproducible, and an
 *   image's result does not depend on the batch it is in.
 * llie_softattn_backward: dqkv [batch][N][3 * 32 heads] given d(out), with out and lse as llie_softattn left them; scratch:
 *   llie_softattn_bwd_floats floats (delta = rowsum(dout * out) per query).  No atomics: bitwise reproducible, batch-invariant.
 * llie_upsample2x_backward: adjoint of bilinear x2 (align_corners=False): [batch][2Hi][2Wi][C] -> [batch][Hi][Wi][C];
 *   llie_dilate2x: out[2y][2x] = in[y][x], zero elsewhere.  C a multiple of 4 (fp32) or 8.
 * llie_linear_dx: dx[b][k] = sum_r dy[b * dy_stride + r] * w[r][k] (w [R][Kc] of the type wdtype, dx fp32); scratch (or NULL):
 *   llie_linear_dx_scratch_floats floats, lets a long R run in parallel chunks.  llie_linear_dw: dw[r][k] = sum_b dy[b][r] x[b][k],
 *   db[r] = sum_b dy[b][r] (db may be NULL).
 * llie_final_bwd_data: input gradient of the output head's 3x3 conv (pad 1): da[b][y][x][c] (NHWC, compute type) =
 *   sum_{o,tap} deps[b][o][y - ky + 1][x - kx + 1] * w[tap][c][o], deps fp32 NCHW [batch][Cout][H][W], w fp32 [9][C][4], Cout <= 4. */
int llie_wgrad(int dtype, const void* g, int N, const llie_gemm_seg* segs, int nseg, int batch, int Ho, int Wo, int Hi, int Wi, int stride,
               int dy, int dx, int ntap, int nstore, int kstore, float* partial, int64_t partial_floats, float* out, int64_t ldn, int64_t ldk,
               int64_t off, int msplit, llie_stream stream);
int llie_wgrad_msplit(int dtype, int batch, int pixels, int N, int K, int ntap, int ragged_rule);
int64_t llie_wgrad_partial_floats(int msplit, int N, int K, int ntap);
int llie_dw_wgrad(int dtype, const void* g, const float* gs, const float* gb, const void* h, const float* scale, const float* shift,
                  float* partial, float* out, int batch, int H, int W, int C, llie_stream stream);
int llie_dw_wgrad_strips(int H, int W);
typedef struct llie_gn_backward_args {
  const void* g; void* dz;
  const void* x0; const void* x1; int c0, c1;
  const float* scale; const float* shift; int act;
  const float* mean; const float* rstd; const float* gamma; const float* beta;
  const float* film; int64_t film_stride; float* dfilm; int64_t dfilm_stride;
  float* dgamma; float* dbeta;
  const void* add0; const void* add1_0; const void* add1_1;
  void* dx0; void* dx1;
  int batch, pixels;
} llie_gn_backward_args;
int llie_groupnorm_backward(int dtype, const llie_gn_backward_args* args, float* scratch, int64_t scratch_floats, llie_stream stream);
int64_t llie_groupnorm_backward_scratch_floats(int batch, int C, int pixels);
int llie_linattn_backward(int dtype, const void* qkv, const float* kv_scratch, const void* dout, void* dqkv, float* dkv_scratch,
                          int64_t dkv_floats, int batch, int N, int heads, llie_stream stream);
int64_t llie_linattn_dkv_floats(int batch, int N, int heads);
int llie_softattn(int dtype, const void* qkv, void* out, float* lse_or_NULL, int batch, int N, int heads, llie_stream stream);
int llie_softattn_backward(int dtype, const void* qkv, const void* out, const void* dout, const float* lse, void* dqkv, float* scratch,
                           int64_t scratch_floats, int batch, int N, int heads, llie_stream stream);
int64_t llie_softattn_bwd_floats(int batch, int N, int heads);
int llie_upsample2x_backward(int dtype, const void* dout, void* din, int batch, int Hi, int Wi, int C, llie_stream stream);
int llie_dilate2x(int dtype, const void* in, void* out, int batch, int Hi, int Wi, int C, llie_stream stream);
int llie_linear_dx(int wdtype, const float* dy, int64_t dy_stride, const void* w, float* dx, int batch, int R, int Kc, float* scratch,
                   int64_t scratch_floats, llie_stream stream);
int64_t llie_linear_dx_scratch_floats(int batch, int R, int Kc);
int llie_linear_dw(const float* dy, int64_t dy_stride, const float* x, float* dw, float* db, int batch, int R, int Kc, llie_stream stream);
int llie_final_bwd_data(int dtype, const float* deps, const float* w, void* da, int batch, int H, int W, int C, int Cout, llie_stream stream);

/* The parts of the training backward pass that run between those kernels, each as the engine launches it.
 * llie_dwconv3x3_backward: input gradient of the depthwise conv of one inverted-residual block, on the forward kernel's body.  g
 *   [B][H][W][C] (the gradient of the conv's output before the SE gate); the prologue forms dh2 = g * gs + gb (gs / gb fp32 [B][C]: the
 *   SE gate and d(mean) / pixels) rounded to the compute type; w9c_flipped fp32 [9][C]: the forward weights with the taps in reverse
 *   order; the epilogue multiplies by the ReLU6 derivative [0 < bx * bas + bab < 6] of the forward pre-activation (bx [B][H][W][C]: the
 *   tensor the forward conv read, bas / bab [B][C]: its norm affine) and stores dz_out in the compute type, plus slab fp32
 *   [B][tiles][2][C] with tiles = the forward's llie_dwconv3x3_tiles: per (8-row segment, strip) the sums of dz and of dz * bx over
 *   the pixels inside the map.  The strip height is the forward's llie_dwconv3x3_strip_rows.  Refused: NULL tensors, sizes < 1, C not a
 *   multiple of 32 (fp32) / 64 (2-byte).
 * llie_groupnorm_backward_from_slab: llie_groupnorm_backward for a site whose producer (llie_dwconv3x3_backward) already applied the
 *   activation's derivative and wrote the tile partials: slab [batch][ntiles][2][C] with tiles of any pixel count.  Needs act != 0
 *   and args->dz == args->g (dz is read, not written); scratch: 7 * batch * C floats.
 * llie_bias_grad: out[0 .. Cstore) = column sums of g [M][C] (compute type, P pixels per image, C a multiple of 32, Cstore <= C)
 *   through the scratch slab and S, whose sizes in floats llie_bias_grad_floats returns.
 * llie_pack_planes: fp32 NCHW planes x0 [batch][c0][pixels] and x1 [batch][c1][pixels] (NULL with c1 = 0; c0 + c1 <= 8) -> out
 *   [batch * pixels][32] of the compute type, channels beyond c0 + c1 zero.  llie_add_into: dst += src over n elements of the compute
 *   type (n a multiple of 4 in fp32, 8 otherwise), the sum formed in fp32.
 * llie_sin_embed: emb [rows][dim] = [cos | sin] of float(t[r]) * freqs[i], freqs fp32 [dim / 2], t device int64.
 * llie_pointwise_backward: the fp32 elementwise kernels of the SE and time MLPs' backward over n elements: out = a * b * (1 - b)
 *   (LLIE_PW_SIGMOID_BWD: b the sigmoid's output), 0 < b < 6 ? a : 0 (LLIE_PW_RELU6_BWD: b the ReLU6's output), a * silu'(b)
 *   (LLIE_PW_SILU_BWD: b the SiLU's input), a * scale (LLIE_PW_SCALE: b unused).  out may alias a. */
enum llie_pointwise_kind { LLIE_PW_SIGMOID_BWD = 0, LLIE_PW_RELU6_BWD = 1, LLIE_PW_SILU_BWD = 2, LLIE_PW_SCALE = 3 };
int llie_dwconv3x3_backward(int dtype, const void* g, const float* gs, const float* gb, const float* w9c_flipped, const void* bx,
                            const float* bas, const float* bab, void* dz_out, float* slab, int B, int H, int W, int C, llie_stream stream);
int llie_groupnorm_backward_from_slab(int dtype, const llie_gn_backward_args* args, float* slab, int ntiles, float* scratch,
                                      int64_t scratch_floats, llie_stream stream);
int llie_bias_grad_floats(int batch, int C, int pixels, int64_t* slab_floats, int64_t* s_floats);
int llie_bias_grad(int dtype, const void* g, int M, int C, int P, int Cstore, float* slab, float* S, float* out, llie_stream stream);
int llie_pack_planes(int dtype, const float* x0, int c0, const float* x1, int c1, void* out, int batch, int pixels, llie_stream stream);
int llie_add_into(int dtype, void* dst, const void* src, int64_t n, llie_stream stream);
int llie_sin_embed(const int64_t* t, const float* freqs, float* emb, int rows, int dim, llie_stream stream);
int llie_pointwise_backward(int kind, const float* a, const float* b, float* out, int64_t n, float scale, llie_stream stream);

/* Statistics pass of the recompute form of InvertedResidualBlock (efficient_unet.py:207-212) on its own: Gram matrix
 * G = sum_px a' a'^T and column sums m = sum_px a' of a' = clamp01(x * scale + bias) rounded to the compute type, per image
 * (gram.hip).  x0 / x1: NHWC [batch][pixels][c0 / c1] of the compute type (x1 may be NULL with c1 = 0), c0 + c1 in {32, 64, 96},
 * c0 % 8 == 0, pixels % 512 == 0; scale / bias [batch][c0 + c1] fp32; part: scratch of batch * llie_gram_part_floats floats;
 * gtot out: [batch][K * K + K] fp32 (G row-major, then m); tickets: [batch] uint32, zero on entry (left zero). */
int llie_gram_stats(int dtype, const void* x0, int c0, const void* x1, int c1, const float* scale, const float* bias, int batch,
                    int pixels, float* part, float* gtot, unsigned int* tickets, llie_stream stream);
int64_t llie_gram_part_floats(int K, int pixels);
/* The finalize behind it (gram.hip: gram_finalize_kernel; replaces nn.GroupNorm(32, 4K) statistics of h1 = W1 . relu6(norm1(x)),
 * efficient_unet.py:174,212, + the FiLM fold :215-217): sum h1[c] = 6 w_c . m, sum h1[c]^2 = 36 w_c^T G w_c (row products and sums
 * in fp64), then scale[b][c] = rstd gamma[c] (1 + fs), shift[b][c] = (beta[c] - mean rstd gamma[c]) (1 + fs) + fh like
 * llie_groupnorm_finalize.  gram_totals: llie_gram_stats' gtot; w_expand: [4K][K] of the compute type; K in {32, 64, 96}. */
int llie_gram_finalize(int dtype, const float* gram_totals, const void* w_expand, int K, int pixels, const float* gamma, const float* beta,
                       const float* film, int64_t film_stride, float eps, float post_scale, int batch, float* scale_out, float* shift_out,
                       llie_stream stream);
int llie_dwconv3x3(int dtype, const void* in, void* out, const float* scale, const float* bias, const float* w9c,
                   float* pool, int B, int H, int W, int C, llie_stream stream);
int llie_dwconv3x3_tiles(int H, int W);
/* llie_dwconv3x3_ex: llie_dwconv3x3 in every form the engines launch.  pool_totals (or NULL; exclusive with pool): uint64 [B][C],
 *   += round(2^24 x partial sums of the stored output per channel) (integer adds; the caller sets the starting value).
 *   flags bit 0 (s6, 2-byte dtypes): scale / bias hold norm2's affine divided by 6, the prologue is clamp01(in*scale+bias) rounded to
 *   the compute type and the weights are taken as T(6 w) -- relu6(z) w = clamp01(z / 6) (6 w); bit 1 (no_act): the prologue is the
 *   affine alone.  Checked before any HIP call (LLIE_ERR_ARG): NULL tensors, pool and pool_totals together, s6 with no_act or in
 *   fp32, C not a multiple of 32 (fp32) / 64 (2-byte), sizes < 1.
 * llie_dwconv3x3_strip_rows: the strip height (8, 16, 32 or 64 rows per workgroup) the launcher takes for these sizes.
 * llie_last_kernel: the name the last kernel launcher called on this thread recorded (kernel and template arguments, as
 *   llie_profile_report aggregates them); "" before the first launch.  Not every launcher records one. */
int llie_dwconv3x3_ex(int dtype, const void* in, void* out, const float* scale, const float* bias, const float* w9c, float* pool,
                      unsigned long long* pool_totals, int flags, int B, int H, int W, int C, llie_stream stream);
int llie_dwconv3x3_strip_rows(int dtype, int B, int H, int W, int C);
const char* llie_last_kernel(void);
/* The recompute form of InvertedResidualBlock (efficient_unet.py:203-236; irbx.hip), kernel by kernel.  x0 / x1: the block input,
 * NHWC [batch][H][W][c0 / c1] of a 2-byte compute type (x1 NULL with c1 = 0), Cin = c0 + c1 in {32, 64, 96}, c0 % 16 == 0,
 * H % 8 == 0, W % 16 == 0, Chid = 4 Cin.  scale1 / shift1 [batch][Cin]: norm1's affine DIVIDED BY 6 (a' = clamp01(x scale1 + shift1)
 * = relu6(norm1 x) / 6, rounded to the compute type); w_expand [Chid][Cin] of the compute type; scale2 / shift2 [batch][Chid]:
 * norm2 + FiLM, undivided: a = relu6(scale2 h1 + shift2) with h1 = 6 w_expand a'; w_dw fp32 [9][Chid] tap-major.
 * expand_dw: h2 = depthwise3x3(a) [batch][H][W][Chid]; pool_totals (or NULL): uint64 [batch][Chid], += round(2^24 partial sums
 *   of h2 per channel) (integer adds: independent of order); the caller zeroes it.
 * expand_pool: the same totals without h2: the conv is linear and zero-padded, so a channel's sum of h2 follows from nine sums of a
 *   (all pixels, first / last row, first / last column, four corners) -- one pass that only rebuilds h1.
 * expand_dw_project (identity-residual blocks, Cout = Cin = C in {32, 64}, one input segment): y = w_project (gate * h2) + x with the
 *   SE gate [batch][Chid] given, w_project [C][Chid] of the compute type; h2 never leaves the workgroup.  stats: fp32 slab
 *   [batch][irbx_project_tiles(H, W)][2][C] of y's per-channel (sum, sum of squares), one entry per 8 x 16 tile.
 * expand_dw_project_skip (the 96 -> 32 block: a skip conv for a shortcut, c0 + c1 = 96 in one or two segments, cout = 32):
 *   y = w_project (gate * h2) + w_skip x, x the raw concatenated input; w_project_skip [cout][ld] of the compute type holds w_project
 *   in columns [0, Chid) and w_skip in [Chid, Chid + Cin) (ld >= Chid + Cin, ld % 8 == 0).  stats as above.
 * The engine takes expand_pool and the matching project kernel for the blocks these two cover while the knob "irbx_project" is
 * 1 [the default]; 2 keeps only the identity-residual blocks, 0 none (then expand_dw and the project GEMM, as for every other
 * recompute block; tests and A/B measurements). */
int llie_expand_dw(int dtype, const void* x0, int c0, const void* x1, int c1, const float* scale1, const float* shift1, const void* w_expand,
                   const float* scale2, const float* shift2, const float* w_dw, void* h2, unsigned long long* pool_totals, int batch, int H, int W,
                   llie_stream stream);
int llie_expand_pool(int dtype, const void* x0, int c0, const void* x1, int c1, const float* scale1, const float* shift1, const void* w_expand,
                     const float* scale2, const float* shift2, const float* w_dw, unsigned long long* pool_totals, int batch, int H, int W,
                     llie_stream stream);
int llie_expand_dw_project(int dtype, const void* x, int C, const float* scale1, const float* shift1, const void* w_expand, const float* scale2,
                           const float* shift2, const float* w_dw, const float* gate, const void* w_project, void* y, float* stats, int batch,
                           int H, int W, llie_stream stream);
int llie_expand_dw_project_skip(int dtype, const void* x0, int c0, const void* x1, int c1, const float* scale1, const float* shift1,
                                const void* w_expand, const float* scale2, const float* shift2, const float* w_dw, const float* gate,
                                const void* w_project_skip, int ld, int cout, void* y, float* stats, int batch, int H, int W, llie_stream stream);
int llie_irbx_project_tiles(int H, int W);
/* The wide decoder blocks (192 -> 64 at Chid 768, 384 -> 128 at Chid 1536; skip conv, one or two input segments) without h2, from the
 * STORED h1 [batch][H][W][Chid] of a 2-byte compute type.  scale2 / shift2 [batch][Chid]: norm2 + FiLM DIVIDED BY 6, as the unfused
 * depthwise takes them in its s6 form: a = clamp01(h1 scale2 + shift2) rounded to the compute type, weights T(6 w_dw).
 * dwconv3x3_pool: pool_totals uint64 [batch][Chid] += round(2^24 x per-channel sums of depthwise3x3(a) (6 w_dw)), from nine sums of a
 *   (expand_pool's restatement), one streaming read of h1; the caller zeroes it.  Needs Chid in {768, 1536}, H % 8 == 0, W % 16 == 0.
 * dwconv3x3_project: y = w_project (gate * depthwise3x3(a)) + w_skip x [batch][H][W][cout], x the raw concatenated block input
 *   (x1 NULL with c1 = 0; Chid = 4 (c0 + c1)); w_project_skip [cout][ld] of the compute type holds w_project in columns [0, Chid) and
 *   w_skip in [Chid, Chid + Cin) (ld % 8 == 0); stats: fp32 slab [batch][llie_irbx_project_tiles(H, W)][2][cout] of y's per-channel
 *   (sum, sum of squares), one entry per 8 x 16 tile.  The depthwise result never leaves the workgroup.
 * llie_wide_project_supported: 1 where the engine takes this pair (knob "wide_project" = 1 [the default]; 0 = dwconv3x3 + project
 *   GEMM): 2-byte dtype, a skip conv, no zero-padded channels, (cin, chid, cout) one of the two triples, c0 % 16 == 0, H % 8 == 0,
 *   W % 16 == 0; else 0.  Outside it the launchers return LLIE_ERR_SHAPE and launch nothing. */
int llie_wide_project_supported(int dtype, int cin, int c0, int chid, int cout, int skip, int padded, int H, int W);
/* llie_irb_forms: the launch sequence the inference engine picks for every inverted-residual block of a UNet context whose
 *   full-resolution map is H x W, under the knobs of the moment, in forward order (encoder, middle, decoder): six ints per block --
 *   cin, hid, cout, the block's map H and W, and the form: 0 unfused, 1 recompute (expand_dw), 2 project (expand_pool +
 *   expand_dw_project), 3 wide (dwconv3x3_pool + dwconv3x3_project).  At most cap_blocks entries are written; returns the number
 *   of blocks.  Needs no GPU. */
int llie_irb_forms(llie_ctx* c, int H, int W, int* out6, int cap_blocks);
int llie_dwconv3x3_pool(int dtype, const void* h1, const float* scale2, const float* shift2, const float* w_dw, unsigned long long* pool_totals,
                        int batch, int H, int W, int chid, llie_stream stream);
int llie_dwconv3x3_project(int dtype, const void* h1, const float* scale2, const float* shift2, const float* w_dw, const float* gate, const void* x0,
                           int c0, const void* x1, int c1, const void* w_project_skip, int ld, int cout, void* y, float* stats, int batch, int H,
                           int W, llie_stream stream);
/* The wide Gram form of the 192 -> 64 block (knob "wide_gram", default 1 = maps of at least 4096 pixels, 2 = every map; 0 = the pool pass
 * from the stored h1, bit for bit what the engine computed before the form existed):
 * norm2's tables are known BEFORE the expand GEMM, from the Gram matrix G = sum_px a' a'^T and m = sum_px a' of the activated input
 * a' = clamp01(x scale1 + shift1), so the expand GEMM stores the activated h1 and adds the SE pool totals itself.
 * llie_wide_gram_supported: 2-byte dtype, cin = 192, chid = 768, c0 % 8 == 0, pixels % 128 == 0.
 * llie_gram_wide: gblk [batch][llie_gram_wide_floats()] fp32 = the 21 upper 32 x 32 blocks of G (block q = rows 32 bi, columns 32 bj
 *   of llie_gram_wide_block), then m[192]; part: scratch of batch x llie_gram_wide_part_floats(pixels) floats.  Batch-invariant bits.
 * llie_gram_group_weights: mg fp64 [32][llie_gram_wide_floats()] from the packed expand weights (wpack as llie_pw_expand fills or
 *   takes it: the weight times 6 rounded to the compute type, what the GEMM multiplies with): per GroupNorm group M_g = sum_c w_c w_c^T
 *   in the same block layout (off-diagonal blocks doubled) and u_g = sum_c w_c.
 * llie_gram_group_finalize: norm2 + FiLM tables [batch][768] from <G, M_g> and <m, u_g> in fp64 (times post_scale unless 0).
 * llie_pw_expand_act: out [M][768] = T(clamp01((w a') scale2 + shift2)), one rounding; pool_totals uint64 [batch][768] += what
 *   llie_dwconv3x3_pool adds from such a tensor (the caller zeroes it).  w32 / wpack as llie_pw_expand; M = batch x H x W.
 * llie_dwconv3x3_project_preact: llie_dwconv3x3_project on an h1 that already holds the activated values (cout = 64).
 * llie_irb_wide_gram: one int per block in llie_irb_forms' order: 1 where the engine takes this form. */
int llie_wide_gram_supported(int dtype, int cin, int c0, int chid, int pixels);
int64_t llie_gram_wide_floats(void);
int64_t llie_gram_wide_part_floats(int pixels);
int llie_gram_wide_block(int q, int* bi, int* bj);
int llie_gram_wide(int dtype, const void* x0, int c0, const void* x1, int c1, const float* scale, const float* bias, int batch, int pixels,
                   float* part, float* gblk, llie_stream stream);
int llie_gram_group_weights(int dtype, const void* wpack, double* mg, int chid, int K, llie_stream stream);
int llie_gram_group_finalize(const float* gblk, const double* mg, int K, int pixels, const float* gamma, const float* beta, const float* film,
                             int64_t film_stride, float eps, float post_scale, int batch, float* scale_out, float* shift_out, llie_stream stream);
int llie_pw_expand_act(int dtype, const llie_gemm_seg* segs, int nseg, const float* w32, void* wpack, const float* scale2, const float* shift2,
                       const float* w_dw, void* out, unsigned long long* pool_totals, int M, int N, int H, int W, llie_stream stream);
int llie_dwconv3x3_project_preact(int dtype, const void* h1a, const float* w_dw, const float* gate, const void* x0, int c0, const void* x1, int c1,
                                  const void* w_project_skip, int ld, int cout, void* y, float* stats, int batch, int H, int W, llie_stream stream);
int llie_irb_wide_gram(llie_ctx* c, int H, int W, int* out1, int cap_blocks);
/* llie_expand_dw_plan: the launch plan expand_dw (project = 0) or expand_dw_project (project = 1) takes for cin input channels at
 *   these sizes, the "irbx_grid*" knobs included (they act on expand_dw only; the dtype and the segment split do not enter).
 *   plan4[0] = tiles per workgroup, a run along x (4, 2 or 1: the largest that divides W / 16 and keeps 2048 workgroups; 0 = the
 *   image's tiles split evenly over grid.x workgroups, "irbx_grid*"), plan4[1] = 64-channel chunks per workgroup (all cin / 16 of
 *   them, halved while the launch has fewer than 1024 workgroups and the count is even; project: always all), plan4[2] = grid.x,
 *   plan4[3] = grid.y; grid.z is the batch.  LLIE_ERR_ARG: plan4 NULL, a size < 1, project not 0 or 1; LLIE_ERR_SHAPE: outside
 *   the shapes above (cin in {32, 64, 96}, H % 8 == 0, W % 16 == 0). */
int llie_expand_dw_plan(int cin, int batch, int H, int W, int project, int* plan4);
/* expand_stats: the statistics pass of the same blocks on its own (knob "gram" = 0, and every recompute block below 32 768 pixels):
 * stats [batch][H W / llie_irbx_stats_rows(H W)][2][Chid] fp32 = (sum, sum of squares) of h1 = w_expand relu6(norm1(x)) per channel
 * over each run of llie_irbx_stats_rows(H W) consecutive pixels; every entry is written.  Leading arguments as expand_pool. */
int llie_expand_stats(int dtype, const void* x0, int c0, const void* x1, int c1, const float* scale1, const float* shift1, const void* w_expand,
                      float* stats, int batch, int H, int W, llie_stream stream);
int llie_irbx_stats_rows(int P);
/* dst[0:bytes] = src[0:bytes] with 16-byte lane accesses: the on-box HBM copy-bandwidth probe behind bench.py's
 * `peak_measured` ("a copy-kernel bandwidth probe"; 2 x bytes move per call). */
int llie_copy_probe(const void* src, void* dst, int64_t bytes, llie_stream stream);
/* Streaming probe with a chosen read : write mix: `units` steps, each reading `reads` and writing `writes` 16 KB blocks
 * ((reads, writes) in {(1,0),(0,1),(1,1),(1,2),(1,4),(2,1),(4,1)}; src holds units*reads, dst units*writes blocks).
 * nontemporal: 0 plain, 1 non-temporal loads and stores, 2 write-through (sc1) stores, 3 sc0 sc1 stores.  reads == -1: a
 * trivial dependent launch (boundary cost studies).
 * The ceiling the write-dominated 4x expansions (efficient_unet.py:174) are compared with. */
int llie_rw_probe(const void* src, void* dst, int64_t units, int reads, int writes, int nontemporal, llie_stream stream);
/* Engine knobs (process-wide; every call starts a new epoch of the hipGraph cache).  Production defaults in brackets.
 *   "enhance_split" [2] concurrent batch branches of the captured enhance graph (1 = one chain; env LLIE_ENHANCE_SPLIT)
 *   "irbx" [1] recompute form of the inverted-residual front half (0 = expand GEMM + depthwise kernel), "irbx_dbuf" [0] its double-buffered
 *   32-channel variant, "irbx_grid" [0], "irbx_grid2" [0], "irbx_grid4" [0], "irbx_grid6" [0] workgroups per expand_dw launch (all / 32- / 64- /
 *   96-channel inputs; 0 = heuristics), "gram" [1] (norm2 statistics of the recompute form from the Gram matrix of the block input, gram.hip;
 *   0 = expand_stats), "pwx" [1] (activation-stationary expand GEMM, pwx.hip; 0 = tile kernel), "se_mfma" [1] (SE MLP of the wide blocks on the
 *   MFMA pipe), "gemm_bk" [0] (0 = auto, 32 = 32-wide K chunks), "nt_mask" [1], "nt_min_mb" [100] (which producers store tensors of at least so
 *   many MiB non-temporally: tune.cpp), "bwd_async" [1] (weight gradients on a side stream; 0 = single stream).
 *   "irbx_project" [1] the recompute blocks expand_dw_project and expand_dw_project_skip cover run without h2 (expand_pool + the project
 *   kernel above); 2 = the identity-residual blocks only, 0 = expand_dw and the project GEMM; any other value is taken as 1.
 *   "wide_project" [1] the two wide decoder blocks of llie_wide_project_supported run without h2 (dwconv3x3_pool + dwconv3x3_project
 *   above); 0 = dwconv3x3 and the project GEMM.  Independent of irbx_project.
 *   "wide_gram" [1] the 192 -> 64 wide block takes norm2's tables from the Gram of its input (llie_gram_wide above) on maps of at least 4096
 *   pixels, llie_pw_expand_act stores the activated h1 and adds the pool totals; 2 = on every map, 0 = the pool pass over the stored h1;
 *   any other value is taken as 1.
 *   "upconv_fold" [1] the up-sampling convs of 2-byte inference engines run from folded weights (llie_conv3x3_upfold above) on maps of
 *   whole 8 x 16 low-resolution tiles; 0 = the kernel that blends the patch itself, everywhere.
 *   "graph_max_steps" [20] loops of llie_enhance with more steps run as plain launches and are never captured (measured: replaying the
 *   graph of a 50-step loop is slower than launching it); a value <= 0 restores the default.  It changes no bit.
 * Diagnostics, slow (cycle-stamped kernel builds read back by llie_debug_*_stamps): "gemm_stamp" [0], "pwx_stamp" [0], "conv_stamp" [0],
 * "irbx_stamp" [0] (1 expand_dw, 2 expand_pool, 3 expand_dw_project).
 * Threading: the knobs are plain process-wide variables read by every forward; call llie_tune only while no other
 * thread is inside an llie_* compute call (same rule as the handle itself: SURVEY.md 8b, one stream at a time). */
int llie_tune(const char* knob, int value);
int llie_debug_irbx_stamps(double* out10); /* diagnostic builds: 9 per-wave cycle sums of expand_dw ("irbx_stamp" = 1) or of expand_pool's LDS-tile scan ("irbx_stamp" = 2, 5 slots used) or of expand_dw_project ("irbx_stamp" = 3, slots of its own) (irbx.hip: STAMP) + waves averaged */
int llie_debug_conv_stamps(double* out8); /* diagnostic builds: 7 per-wave cycle sums of the up-sampling conv (conv.hip: STAMP) + waves averaged */
int llie_debug_gemm_stamps(double* out3); /* diagnostic builds: see gemm.hip (STAMP) */
int llie_debug_pwx_stamps(double* out4);  /* diagnostic builds: see pwx.hip (STAMP): {A phase, channel loop, of which waiting for the weight DMA} cycles per wave, waves */

/* Per-kernel-class timing with HIP events recorded on the launch stream (what bench.py's `roofline`
 * object is computed from).  llie_profile_begin arms recording for the classes in `class_mask`;
 * every subsequent launch of those kernels is bracketed by an event pair (at most 8192 pairs).
 * llie_profile_end disarms, synchronises on the recorded events and returns, for `kernel_class`, the
 * summed device time, the launch count and the summed ALGORITHMIC bytes of those launches
 * (activation elements the kernel must read and write once, plus its weights). */
enum llie_kernel_class {
  LLIE_K_GEMM = 1,  /* pw_gemm_kernel: 1x1 convs with fused prologue / epilogue */
  LLIE_K_DW = 2,    /* dwconv3x3_kernel */
  LLIE_K_CONV3 = 4, /* conv3x3_kernel, conv3x3_upfold_kernel, conv3x3_upmaps_kernel (down / up sampling convs) */
  LLIE_K_SE = 8,    /* squeeze-excitation MLP launches */
  LLIE_K_OTHER = 16 /* everything else on the forward path (norm finalize, attention core, input / output convs, time MLPs) */
};
int llie_profile_begin(llie_ctx* ctx, int class_mask);
int llie_profile_end(llie_ctx* ctx, int kernel_class, double* total_ms, int64_t* launches, int64_t* algorithmic_bytes);
/* Same data aggregated per kernel NAME (template arguments included, the granularity of
 * `rocprofv3 --kernel-trace --stats`): writes lines "name\tms\tlaunches\talgorithmic_bytes\n" into buf. */
int llie_profile_report(llie_ctx* ctx, char* buf, size_t cap);
/* Every recorded launch in launch order: lines "class\tkernel\toperator tag\tms\talgorithmic_bytes\n". */
int llie_profile_dump(llie_ctx* ctx, char* buf, size_t cap);

/* SinusoidalPosEmb + time_mlp of a LLIE_UNET handle on their own (efficient_unet.py:60-76, 412-417, and the SiLU
 * that opens every block's FiLM projection, :189-192): emb [rows][base_channels] ([cos | sin]), temb [rows][T],
 * silu_temb [rows][T]; timesteps device int64 [rows].  emb may be null. */
int llie_time_embed(llie_ctx* ctx, const int64_t* timesteps, int rows, float* emb, float* temb, float* silu_temb,
                    llie_stream stream);

/* llie_algorithmic_bytes returns the roofline numerator of SURVEY.md 8d for one
 * UNet forward of `batch` images at the handle's dtype (activation traffic + weights once). */
int64_t llie_algorithmic_bytes(llie_ctx* ctx, int batch);
int64_t llie_flops(llie_ctx* ctx, int batch);
/* Same model with the blocks the engine runs in the recompute form (irbx.hip: h1 is never stored) counted as
 * (3Cin + 2Chid + Cout) P -- the bytes the engine's own kernel selection has to move. */
int64_t llie_path_bytes(llie_ctx* ctx, int batch);

#ifdef __cplusplus
}
#endif
#endif /* LLIE_H_ */
