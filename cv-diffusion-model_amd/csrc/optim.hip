// Optimiser step of the training loop in two launches + one single-workgroup launch between them, over every parameter
// tensor at once.
//
// Replaces, for the trainer's inner loop (reference src/training/trainer.py:300-324), the eager sequence
//   scaler.unscale_ -> torch.nn.utils.clip_grad_norm_(params, max_norm) -> optimizer.step() [torch.optim.AdamW]
//   -> EMAModel.update (trainer.py:98-104: shadow = decay * shadow + (1 - decay) * param)
// which on 321 parameter tensors is ~40 launches and several milliseconds of host time per step; here the host cost is
// three launches, whatever the number of tensors.  The arithmetic is torch's, operation for operation (torch/optim/adamw.py,
// _single_tensor_adamw: decoupled decay p *= 1 - lr wd; m = lerp(m, g, 1 - b1); v = b2 v + (1 - b2) g g;
// p -= lr / (1 - b1^t) * m / (sqrt(v) / sqrt(1 - b2^t) + eps)), the clip coefficient is clip_grad_norm_'s
// min(1, max_norm / (||g|| + 1e-6)).
//
// Layout: `tensors[i]` = one parameter (fp32 master, first / second moment, optional EMA shadow, offset of its gradient
// in the flat gradient buffer the backward pass writes); `chunks[c]` = (tensor, first element) of a run of at most kOptChunk
// elements.  HBM-bound: 4 (g) bytes per element in the norm pass, 4 x 5 read + 4 x 4 written in the update.
// The gradient norm is a fixed-order sum (per-thread, per-workgroup, then one workgroup over the chunk partials, in double):
// deterministic run to run.
#include "common.h"
#include "kernels.h"

namespace llie {

constexpr int kOptThreads = 256;

__device__ __forceinline__ bool opt_aligned16(const void* a) { return (reinterpret_cast<uintptr_t>(a) & 15) == 0; }

// sum of squares of the gradients per chunk -> partial[chunk].  Per-thread sums in Acc: float for the plain step; double for
// the AMP step, where a squared fp32 cannot overflow, so the sum is non-finite exactly when some gradient element is inf / NaN
template <typename Acc>
__device__ __forceinline__ void opt_sumsq(const OptTensor* __restrict__ tensors, const OptChunk* __restrict__ chunks,
                                          const float* __restrict__ gbase, double* __restrict__ partial) {
  const OptChunk ch = chunks[blockIdx.x];
  const OptTensor t = tensors[ch.tensor];
  const float* g = gbase + t.goff + ch.first;
  const long long left = t.n - ch.first;
  const int n = left < kOptChunk ? (int)left : kOptChunk;
  Acc acc = 0;
  if (opt_aligned16(g)) {
    const int nv = n >> 2;
    for (int i = threadIdx.x; i < nv; i += kOptThreads) {
      const f32x4 v = reinterpret_cast<const f32x4*>(g)[i];
      acc += (Acc)v[0] * (Acc)v[0];
      acc += (Acc)v[1] * (Acc)v[1];
      acc += (Acc)v[2] * (Acc)v[2];
      acc += (Acc)v[3] * (Acc)v[3];
    }
    for (int i = (nv << 2) + threadIdx.x; i < n; i += kOptThreads) acc += (Acc)g[i] * (Acc)g[i];
  } else {
    for (int i = threadIdx.x; i < n; i += kOptThreads) acc += (Acc)g[i] * (Acc)g[i];
  }
  __shared__ double red[kOptThreads];
  red[threadIdx.x] = (double)acc;
  wg_barrier();
  for (int o = kOptThreads / 2; o > 0; o >>= 1) {
    if ((int)threadIdx.x < o) red[threadIdx.x] += red[threadIdx.x + o];
    wg_barrier();
  }
  if (threadIdx.x == 0) partial[blockIdx.x] = red[0];
}

__global__ void __launch_bounds__(kOptThreads) opt_sumsq_kernel(const OptTensor* __restrict__ tensors, const OptChunk* __restrict__ chunks,
                                                               const float* __restrict__ gbase, double* __restrict__ partial) {
  opt_sumsq<float>(tensors, chunks, gbase, partial);
}

__global__ void __launch_bounds__(kOptThreads) opt_sumsq_amp_kernel(const OptTensor* __restrict__ tensors, const OptChunk* __restrict__ chunks,
                                                                   const float* __restrict__ gbase, double* __restrict__ partial) {
  opt_sumsq<double>(tensors, chunks, gbase, partial);
}

// fixed-order sum of the chunk partials by one workgroup -> red[0] (opt_clip_kernel keeps its own inline copy: unchanged code)
__device__ __forceinline__ void opt_sum_partials(const double* __restrict__ partial, int nchunks, double* red) {
  double acc = 0.0;
  for (int i = threadIdx.x; i < nchunks; i += kOptThreads) acc += partial[i];
  red[threadIdx.x] = acc;
  wg_barrier();
  for (int o = kOptThreads / 2; o > 0; o >>= 1) {
    if ((int)threadIdx.x < o) red[threadIdx.x] += red[threadIdx.x + o];
    wg_barrier();
  }
}

// stats[0] = ||gscale * g||, stats[1] = factor applied to every gradient = gscale * clip coefficient, stats[2] = 1 if the step
// is skipped (non-finite norm and skip_nonfinite: GradScaler.step's behaviour, torch/amp/grad_scaler.py)
__global__ void __launch_bounds__(kOptThreads) opt_clip_kernel(const double* __restrict__ partial, int nchunks, float gscale, float max_norm,
                                                              int skip_nonfinite, float* __restrict__ stats) {
  __shared__ double red[kOptThreads];
  double acc = 0.0;
  for (int i = threadIdx.x; i < nchunks; i += kOptThreads) acc += partial[i];
  red[threadIdx.x] = acc;
  wg_barrier();
  for (int o = kOptThreads / 2; o > 0; o >>= 1) {
    if ((int)threadIdx.x < o) red[threadIdx.x] += red[threadIdx.x + o];
    wg_barrier();
  }
  if (threadIdx.x == 0) {
    const float norm = (float)sqrt(red[0]) * fabsf(gscale);
    float coef = 1.f;
    if (max_norm > 0.f) {
      coef = max_norm / (norm + 1e-6f);
      coef = coef > 1.f ? 1.f : coef;  // NaN stays NaN, as torch.clamp(max=1.0) leaves it
    }
    const bool bad = !(norm <= 3.4028234664e38f);  // inf or NaN
    stats[0] = norm;
    stats[1] = gscale * coef;
    stats[2] = (bad && skip_nonfinite) ? 1.f : 0.f;
  }
}

// The AMP form (torch.amp.GradScaler around the step, with the loss scaler's state in device memory):
//   inv = 1 / scale as scale.double().reciprocal().float(); found_inf = some gradient element is inf / NaN (the double sum
//   of squares is non-finite); norm = ||inv * gscale * g|| formed in double before rounding; factor = inv * gscale * clip
//   coefficient; a taken step advances the AdamW step count and forms its bias corrections in double from it; then
//   _amp_update_scale_ (aten/src/ATen/native/cuda/AmpKernels.cu).
// stats / coef[0..2] as opt_clip_kernel's stats; coef[3] = lr / (1 - beta1^t), coef[4] = sqrt(1 - beta2^t) for the update kernel.
__global__ void __launch_bounds__(kOptThreads) opt_clip_amp_kernel(const double* __restrict__ partial, int nchunks, float gscale, float max_norm,
                                                                  OptAmpArgs amp, double lr, double beta1, double beta2,
                                                                  float* __restrict__ stats, float* __restrict__ coef) {
  __shared__ double red[kOptThreads];
  opt_sum_partials(partial, nchunks, red);
  if (threadIdx.x == 0) {
    const double sum = red[0];
    const float scale = *amp.scale;
    const float inv = (float)(1.0 / (double)scale);
    const bool found_inf = !(sum <= 1.7976931348623157e308);  // inf or NaN
    const float norm = (float)(sqrt(sum) * (double)inv * fabs((double)gscale));
    float clip = 1.f;
    if (max_norm > 0.f) {
      clip = max_norm / (norm + 1e-6f);
      clip = clip > 1.f ? 1.f : clip;
    }
    const float gf = (inv * gscale) * clip;
    const float skip = found_inf ? 1.f : 0.f;
    stats[0] = coef[0] = norm;
    stats[1] = coef[1] = gf;
    stats[2] = coef[2] = skip;
    if (!found_inf) {
      const int t = *amp.step + 1;
      *amp.step = t;
      coef[3] = (float)(lr / (1.0 - pow(beta1, (double)t)));
      coef[4] = (float)sqrt(1.0 - pow(beta2, (double)t));
    }
    if (found_inf) {
      *amp.scale = (float)((double)scale * amp.backoff_factor);
      *amp.growth_tracker = 0;
    } else {
      const int successful = *amp.growth_tracker + 1;
      if (successful == amp.growth_interval) {
        const float grown = (float)((double)scale * amp.growth_factor);
        if (isfinite(grown)) *amp.scale = grown;
        *amp.growth_tracker = 0;
      } else {
        *amp.growth_tracker = successful;
      }
    }
  }
}

struct OptHyper {
  float decay_mul;   // 1 - lr * weight_decay (formed in double, as Python does for torch)
  float one_m_b1;    // 1 - beta1
  float beta2;
  float one_m_b2;    // 1 - beta2
  float step_size;   // lr / (1 - beta1^t)
  float bc2_sqrt;    // sqrt(1 - beta2^t)
  float eps;
  float ema_decay;   // < 0: no EMA
  float one_m_ema;
};

__device__ __forceinline__ void opt_update(float g, float& p, float& m, float& v, float& e, const OptHyper& h, float step_size, float bc2_sqrt,
                                           float gf, bool has_ema) {
  g *= gf;
  p *= h.decay_mul;
  m = m + (g - m) * h.one_m_b1;
  v = v * h.beta2 + (h.one_m_b2 * g) * g;
  const float denom = __fsqrt_rn(v) / bc2_sqrt + h.eps;
  p = p + (m / denom) * (-step_size);
  if (has_ema) e = e * h.ema_decay + p * h.one_m_ema;
}

// shadow = decay * shadow + (1 - decay) * param over one chunk: the EMA update of an AMP step the loss scaler skipped
__device__ __forceinline__ void opt_ema_only(const OptTensor* __restrict__ tensors, const OptChunk* __restrict__ chunks, const OptHyper& h) {
  const OptChunk ch = chunks[blockIdx.x];
  const OptTensor t = tensors[ch.tensor];
  if (t.ema == nullptr || h.ema_decay < 0.f) return;
  const float* p = t.p + ch.first;
  float* e = t.ema + ch.first;
  const long long left = t.n - ch.first;
  const int n = left < kOptChunk ? (int)left : kOptChunk;
  int done = 0;
  if (opt_aligned16(p) && opt_aligned16(e)) {
    const int nv = n >> 2;
    for (int i = threadIdx.x; i < nv; i += kOptThreads) {
      const f32x4 pv = reinterpret_cast<const f32x4*>(p)[i];
      f32x4 ev = reinterpret_cast<f32x4*>(e)[i];
#pragma unroll
      for (int k = 0; k < 4; ++k) ev[k] = ev[k] * h.ema_decay + pv[k] * h.one_m_ema;
      reinterpret_cast<f32x4*>(e)[i] = ev;
    }
    done = nv << 2;
  }
  for (int i = done + threadIdx.x; i < n; i += kOptThreads) e[i] = e[i] * h.ema_decay + p[i] * h.one_m_ema;
}

// kAmp: `stats` is the optimiser's coefficient slot written by opt_clip_amp_kernel (the bias corrections come from it too),
// and a skipped step still moves the EMA shadows (the reference trainer calls ema.update whether or not GradScaler stepped)
template <bool kAmp>
__global__ void __launch_bounds__(kOptThreads) opt_adamw_kernel(const OptTensor* __restrict__ tensors, const OptChunk* __restrict__ chunks,
                                                               const float* __restrict__ gbase, const float* __restrict__ stats, const OptHyper h) {
  if (stats[2] != 0.f) {  // skipped step: nothing moves
    if constexpr (kAmp) opt_ema_only(tensors, chunks, h);
    return;
  }
  const float step_size = kAmp ? stats[3] : h.step_size, bc2_sqrt = kAmp ? stats[4] : h.bc2_sqrt;
  const float gf = stats[1];
  const OptChunk ch = chunks[blockIdx.x];
  const OptTensor t = tensors[ch.tensor];
  const float* g = gbase + t.goff + ch.first;
  float* p = t.p + ch.first;
  float* m = t.m + ch.first;
  float* v = t.v + ch.first;
  const bool has_ema = t.ema != nullptr && h.ema_decay >= 0.f;
  float* e = has_ema ? t.ema + ch.first : nullptr;
  const long long left = t.n - ch.first;
  const int n = left < kOptChunk ? (int)left : kOptChunk;
  int done = 0;
  if (opt_aligned16(g) && opt_aligned16(p) && opt_aligned16(m) && opt_aligned16(v) && (!has_ema || opt_aligned16(e))) {
    const int nv = n >> 2;
    for (int i = threadIdx.x; i < nv; i += kOptThreads) {
      const f32x4 gv = __builtin_nontemporal_load(reinterpret_cast<const f32x4*>(g) + i);
      f32x4 pv = reinterpret_cast<f32x4*>(p)[i], mv = reinterpret_cast<f32x4*>(m)[i], vv = reinterpret_cast<f32x4*>(v)[i], ev = {0.f, 0.f, 0.f, 0.f};
      if (has_ema) ev = reinterpret_cast<f32x4*>(e)[i];
#pragma unroll
      for (int k = 0; k < 4; ++k) {
        float pk = pv[k], mk = mv[k], vk = vv[k], ek = ev[k];
        opt_update(gv[k], pk, mk, vk, ek, h, step_size, bc2_sqrt, gf, has_ema);
        pv[k] = pk; mv[k] = mk; vv[k] = vk; ev[k] = ek;
      }
      reinterpret_cast<f32x4*>(p)[i] = pv;
      reinterpret_cast<f32x4*>(m)[i] = mv;
      reinterpret_cast<f32x4*>(v)[i] = vv;
      if (has_ema) reinterpret_cast<f32x4*>(e)[i] = ev;
    }
    done = nv << 2;
  }
  for (int i = done + threadIdx.x; i < n; i += kOptThreads) {
    float pk = p[i], mk = m[i], vk = v[i], ek = has_ema ? e[i] : 0.f;
    opt_update(g[i], pk, mk, vk, ek, h, step_size, bc2_sqrt, gf, has_ema);
    p[i] = pk; m[i] = mk; v[i] = vk;
    if (has_ema) e[i] = ek;
  }
}

static bool opt_hyper_ok(const OptStepArgs& a) {
  return a.tensors && a.chunks && a.gbase && a.partial && a.stats && a.nchunks > 0 && a.lr >= 0.0 && a.beta1 >= 0.0 && a.beta1 < 1.0 &&
         a.beta2 >= 0.0 && a.beta2 < 1.0 && a.eps >= 0.0 && a.weight_decay >= 0.0 && a.ema_decay <= 1.0;
}

static OptHyper opt_hyper(const OptStepArgs& a, double step) {
  OptHyper h;
  const double bc1 = 1.0 - pow(a.beta1, step), bc2 = 1.0 - pow(a.beta2, step);
  h.decay_mul = (float)(1.0 - a.lr * a.weight_decay);
  h.one_m_b1 = (float)(1.0 - a.beta1);
  h.beta2 = (float)a.beta2;
  h.one_m_b2 = (float)(1.0 - a.beta2);
  h.step_size = (float)(a.lr / bc1);
  h.bc2_sqrt = (float)sqrt(bc2);
  h.eps = (float)a.eps;
  h.ema_decay = (float)a.ema_decay;
  h.one_m_ema = (float)(1.0 - a.ema_decay);
  return h;
}

hipError_t launch_optimizer_step(const OptStepArgs& a, hipStream_t s) {
  if (!opt_hyper_ok(a) || a.step < 1) return hipErrorInvalidValue;
  note_kernel("opt_sumsq_kernel");
  hipLaunchKernelGGL(opt_sumsq_kernel, dim3(a.nchunks), dim3(kOptThreads), 0, s, a.tensors, a.chunks, a.gbase, a.partial);
  if (hipError_t e = hipGetLastError(); e != hipSuccess) return e;
  note_kernel("opt_clip_kernel");
  hipLaunchKernelGGL(opt_clip_kernel, dim3(1), dim3(kOptThreads), 0, s, a.partial, a.nchunks, (float)a.grad_scale, (float)a.max_grad_norm, a.skip_nonfinite, a.stats);
  if (hipError_t e = hipGetLastError(); e != hipSuccess) return e;
  const OptHyper h = opt_hyper(a, (double)a.step);
  note_kernel("opt_adamw_kernel");
  hipLaunchKernelGGL(opt_adamw_kernel<false>, dim3(a.nchunks), dim3(kOptThreads), 0, s, a.tensors, a.chunks, a.gbase, a.stats, h);
  return hipGetLastError();
}

hipError_t launch_optimizer_step_amp(const OptStepArgs& a, const OptAmpArgs& amp, float* coef, hipStream_t s) {
  if (!opt_hyper_ok(a) || !amp.scale || !amp.growth_tracker || !amp.step || !coef) return hipErrorInvalidValue;
  note_kernel("opt_sumsq_amp_kernel");
  hipLaunchKernelGGL(opt_sumsq_amp_kernel, dim3(a.nchunks), dim3(kOptThreads), 0, s, a.tensors, a.chunks, a.gbase, a.partial);
  if (hipError_t e = hipGetLastError(); e != hipSuccess) return e;
  note_kernel("opt_clip_amp_kernel");
  hipLaunchKernelGGL(opt_clip_amp_kernel, dim3(1), dim3(kOptThreads), 0, s, a.partial, a.nchunks, (float)a.grad_scale, (float)a.max_grad_norm,
                     amp, a.lr, a.beta1, a.beta2, a.stats, coef);
  if (hipError_t e = hipGetLastError(); e != hipSuccess) return e;
  const OptHyper h = opt_hyper(a, 1.0);  // step_size / bc2_sqrt are replaced by the device's coef[3], coef[4]
  note_kernel("opt_adamw_kernel<amp>");
  hipLaunchKernelGGL(opt_adamw_kernel<true>, dim3(a.nchunks), dim3(kOptThreads), 0, s, a.tensors, a.chunks, a.gbase, coef, h);
  return hipGetLastError();
}

// Gradient accumulation over a window of micro-batches: acc = weight * g (kFirst: acc is not read, so what it held, NaNs
// included, is gone) or acc + weight * g.  The product and the sum are two separately rounded fp32 operations (fp contraction
// is off in the kernel: no fused multiply-add), so a NumPy twin is bit-equal; inf / NaN follow IEEE arithmetic.
// One workgroup per run of kOptChunk elements, as the optimiser's kernels; 64-bit element index for the run's base.  A run's
// base is a multiple of 16 KB, so the alignment of the two pointers decides the path for every run alike.
// HBM-bound: 8 bytes per element (kFirst) or 12.  No LDS, no atomics.
template <bool kFirst>
__global__ void __launch_bounds__(kOptThreads) grad_accumulate_kernel(float* __restrict__ acc, const float* __restrict__ grad, long long total, float w) {
#pragma clang fp contract(off)
  const long long base = (long long)blockIdx.x * kOptChunk;
  const long long left = total - base;
  const int n = left < kOptChunk ? (int)left : kOptChunk;
  float* a = acc + base;
  const float* g = grad + base;
  int done = 0;
  if (opt_aligned16(a) && opt_aligned16(g)) {
    const int nv = n >> 2;
    for (int i = threadIdx.x; i < nv; i += kOptThreads) {
      const f32x4 gv = __builtin_nontemporal_load(reinterpret_cast<const f32x4*>(g) + i);
      f32x4 av = {0.f, 0.f, 0.f, 0.f};
      if (!kFirst) av = reinterpret_cast<const f32x4*>(a)[i];
#pragma unroll
      for (int k = 0; k < 4; ++k) {
        const float prod = w * gv[k];
        av[k] = kFirst ? prod : av[k] + prod;
      }
      reinterpret_cast<f32x4*>(a)[i] = av;
    }
    done = nv << 2;
  }
  for (int i = done + threadIdx.x; i < n; i += kOptThreads) {
    const float prod = w * g[i];
    a[i] = kFirst ? prod : a[i] + prod;
  }
}

hipError_t launch_grad_accumulate(float* acc, const float* grad, long long n, float weight, bool first, hipStream_t s) {
  const long long blocks = (n + kOptChunk - 1) / kOptChunk;
  if (!acc || !grad || n < 0 || blocks > 2147483647LL) return hipErrorInvalidValue;
  if (n == 0) return hipSuccess;
  note_kernel(first ? "grad_accumulate_kernel<first>" : "grad_accumulate_kernel");
  if (first) hipLaunchKernelGGL(grad_accumulate_kernel<true>, dim3((unsigned)blocks), dim3(kOptThreads), 0, s, acc, grad, n, weight);
  else hipLaunchKernelGGL(grad_accumulate_kernel<false>, dim3((unsigned)blocks), dim3(kOptThreads), 0, s, acc, grad, n, weight);
  return hipGetLastError();
}

}  // namespace llie
