// Consistency distillation (reference LowLightLCMDistillation, src/models/low_light_diffusion.py:284-408): the elementwise
// arithmetic around the three denoiser calls of one distillation step, and the EMA update of the target network.
//
//   consistency_target:  x_next = sqrt(a_n) * (x_t - sqrt(1 - a_t) e_T) / sqrt(a_t) + sqrt(1 - a_n) e_T      (:365-376)
//   consistency_loss:    s0 = (x_t - sqrt(1 - a_t) e_S) / sqrt(a_t),  g0 = (x_next - sqrt(1 - a_n) e_E) / sqrt(a_n),
//                        loss = huber(s0, g0) (delta 1, mean), d(loss)/d(e_S) = clamp(s0 - g0, -1, 1) / n * (-sqrt(1 - a_t) / sqrt(a_t))
// The prediction type of a network output o at (x, a), sa = sqrt(a), sb = sqrt(1 - a), is a template parameter (kPredEpsilon /
// kPredV), so the epsilon instantiation is the code above, unchanged, and no element branches on it:
//   epsilon:  x0 = (x - sb o) / sa     e^ = o              d x0 / d o = -sb / sa
//   v:        x0 = sa x - sb o         e^ = sb x + sa o     d x0 / d o = -sb          (finite at a = 0: x0 = -o)
// The target reads the teacher's output with the teacher's type; s0 and g0 read the student's and the EMA student's outputs
// with the student's type.
//   ema_lerp:            ema = ema * decay + (1 - decay) * p over every parameter tensor in one launch (:316-323)
//
// a_t / a_n are per sample: alphas_cumprod[t[b]] / alphas_cumprod[t_next[b]] read from the device table.  The reference's
// operation order is kept with fp contraction off (as lcm_step_kernel / add_noise_kernel do).  A timestep outside the table
// never indexes it: that sample's outputs are NaN.  The loss is a fixed-order sum (per-workgroup partials in double, then one
// workgroup over the partials in double, as optim.hip does): bitwise reproducible, and inf / NaN propagate as a plain sum does
// (Huber terms are >= 0, so an inf term gives +inf, a NaN term gives NaN).
#include "common.h"
#include "kernels.h"

namespace llie {

constexpr int kDistillThreads = 256;

__device__ __forceinline__ float distill_acp(const int64_t* t, int b, const float* acp, int table_len) {
  const int64_t tb = t[b];
  return (tb >= 0 && tb < table_len) ? acp[tb] : __builtin_nanf("");
}

// x0 and e^ of a network output `o` of type PRED at (x, sa, sb); every product and difference is rounded as written
template <int PRED>
__device__ __forceinline__ float distill_x0(float x, float o, float sa, float sb) {
#pragma clang fp contract(off)
  if constexpr (PRED == kPredV) return sa * x - sb * o;
  else return (x - sb * o) / sa;
}

template <int PRED>
__device__ __forceinline__ float distill_eps(float x, float o, float sa, float sb) {
#pragma clang fp contract(off)
  if constexpr (PRED == kPredV) return sb * x + sa * o;
  else return o;
}

template <int PRED>
__global__ void __launch_bounds__(kDistillThreads) consistency_target_kernel(const float* __restrict__ x_t, const float* __restrict__ e_t,
                                                                            const int64_t* __restrict__ t, const int64_t* __restrict__ t_next,
                                                                            const float* __restrict__ acp, int table_len, int64_t per,
                                                                            float* __restrict__ x_next) {
#pragma clang fp contract(off)
  const int b = blockIdx.y;
  const int64_t i = (int64_t)blockIdx.x * kDistillThreads + threadIdx.x;
  if (i >= per) return;
  const float a = distill_acp(t, b, acp, table_len), an = distill_acp(t_next, b, acp, table_len);
  const float sa = sqrtf(a), sb = sqrtf(1.f - a), san = sqrtf(an), sbn = sqrtf(1.f - an);
  const size_t o = (size_t)b * per + i;
  const float e = e_t[o];
  const float x = x_t[o];
  const float x0 = distill_x0<PRED>(x, e, sa, sb);
  x_next[o] = san * x0 + sbn * distill_eps<PRED>(x, e, sa, sb);
}

// Each workgroup covers kDistillLossPerWG consecutive elements of the flattened [B, per] tensors (thread k: elements
// k, k + 256, ...), so the partial count depends on n only.
template <int PRED>
__global__ void __launch_bounds__(kDistillThreads) consistency_loss_kernel(const float* __restrict__ x_t, const float* __restrict__ x_next,
                                                                          const float* __restrict__ e_s, const float* __restrict__ e_e,
                                                                          const int64_t* __restrict__ t, const int64_t* __restrict__ t_next,
                                                                          const float* __restrict__ acp, int table_len, int64_t per, int64_t n,
                                                                          float inv_n, float* __restrict__ d_es, double* __restrict__ partial) {
#pragma clang fp contract(off)
  const int64_t base = (int64_t)blockIdx.x * kDistillLossPerWG;
  double acc = 0.0;
  for (int k = 0; k < kDistillLossPerWG / kDistillThreads; ++k) {
    const int64_t i = base + k * kDistillThreads + threadIdx.x;
    if (i >= n) break;
    const int b = (int)(i / per);
    const float a = distill_acp(t, b, acp, table_len), an = distill_acp(t_next, b, acp, table_len);
    const float sa = sqrtf(a), sb = sqrtf(1.f - a), san = sqrtf(an), sbn = sqrtf(1.f - an);
    const float s0 = distill_x0<PRED>(x_t[i], e_s[i], sa, sb);
    const float g0 = distill_x0<PRED>(x_next[i], e_e[i], san, sbn);
    const float x = s0 - g0;
    const float z = fabsf(x);
    const float l = z < 1.f ? 0.5f * z * z : z - 0.5f;  // F.huber_loss, delta = 1 (NaN takes the second branch and stays NaN)
    acc += (double)l;
    // huber_loss_backward: x <= -1 -> -1, x >= 1 -> 1, else x (NaN falls through), times 1/n; then the autograd chain of s0
    const float c = x <= -1.f ? -1.f : (x >= 1.f ? 1.f : x);
    const float gs0 = inv_n * c;
    if constexpr (PRED == kPredV) d_es[i] = -(gs0 * sb);
    else d_es[i] = -(gs0 / sa) * sb;
  }
  __shared__ double red[kDistillThreads];
  red[threadIdx.x] = acc;
  wg_barrier();
  for (int o = kDistillThreads / 2; o > 0; o >>= 1) {
    if ((int)threadIdx.x < o) red[threadIdx.x] += red[threadIdx.x + o];
    wg_barrier();
  }
  if (threadIdx.x == 0) partial[blockIdx.x] = red[0];
}

__global__ void __launch_bounds__(kDistillThreads) consistency_loss_final_kernel(const double* __restrict__ partial, int nparts, double n,
                                                                                float* __restrict__ loss) {
  __shared__ double red[kDistillThreads];
  double acc = 0.0;
  for (int i = threadIdx.x; i < nparts; i += kDistillThreads) acc += partial[i];
  red[threadIdx.x] = acc;
  wg_barrier();
  for (int o = kDistillThreads / 2; o > 0; o >>= 1) {
    if ((int)threadIdx.x < o) red[threadIdx.x] += red[threadIdx.x + o];
    wg_barrier();
  }
  if (threadIdx.x == 0) *loss = (float)(red[0] / n);
}

// ema.mul_(decay) then ema.add_(p, alpha=1 - decay): the product is rounded on its own (separate op in the reference), the
// add-with-alpha is one fused multiply-add like torch's device kernel (self + alpha * other).
__global__ void __launch_bounds__(kDistillThreads) ema_lerp_kernel(const OptTensor* __restrict__ tensors, const OptChunk* __restrict__ chunks,
                                                                  float decay, float one_m) {
  const OptChunk ch = chunks[blockIdx.x];
  const OptTensor t = tensors[ch.tensor];
  const float* p = t.p + ch.first;
  float* e = t.ema + ch.first;
  const long long left = t.n - ch.first;
  const int n = left < kOptChunk ? (int)left : kOptChunk;
  for (int i = threadIdx.x; i < n; i += kDistillThreads) {
    float v = e[i];
    v = __fmul_rn(v, decay);
    e[i] = __fmaf_rn(one_m, p[i], v);
  }
}

hipError_t launch_consistency_target(const DistillArgs& a, hipStream_t s) {
  if (!a.x_t || !a.e_a || !a.t || !a.t_next || !a.acp || !a.out || a.batch <= 0 || a.per <= 0 || a.table_len <= 0) return hipErrorInvalidValue;
  if (a.pred != kPredEpsilon && a.pred != kPredV) return hipErrorInvalidValue;
  note_kernel("consistency_target_kernel");
  dim3 grid((unsigned)((a.per + kDistillThreads - 1) / kDistillThreads), (unsigned)a.batch);
  auto* kern = a.pred == kPredV ? consistency_target_kernel<kPredV> : consistency_target_kernel<kPredEpsilon>;
  hipLaunchKernelGGL(kern, grid, dim3(kDistillThreads), 0, s, a.x_t, a.e_a, a.t, a.t_next, a.acp, a.table_len, a.per, a.out);
  return hipGetLastError();
}

hipError_t launch_consistency_loss(const DistillArgs& a, double* partial, float* loss, hipStream_t s) {
  if (!a.x_t || !a.x_next || !a.e_a || !a.e_b || !a.t || !a.t_next || !a.acp || !a.out || !partial || !loss || a.batch <= 0 || a.per <= 0 ||
      a.table_len <= 0)
    return hipErrorInvalidValue;
  if (a.pred != kPredEpsilon && a.pred != kPredV) return hipErrorInvalidValue;
  const int64_t n = (int64_t)a.batch * a.per;
  const int64_t nparts = distill_loss_partials(n);
  if (nparts > (int64_t)INT32_MAX) return hipErrorInvalidValue;
  note_kernel("consistency_loss_kernel");
  auto* kern = a.pred == kPredV ? consistency_loss_kernel<kPredV> : consistency_loss_kernel<kPredEpsilon>;
  hipLaunchKernelGGL(kern, dim3((unsigned)nparts), dim3(kDistillThreads), 0, s, a.x_t, a.x_next, a.e_a, a.e_b, a.t, a.t_next,
                     a.acp, a.table_len, a.per, n, (float)(1.0 / (double)n), a.out, partial);
  if (hipError_t e = hipGetLastError(); e != hipSuccess) return e;
  note_kernel("consistency_loss_final_kernel");
  hipLaunchKernelGGL(consistency_loss_final_kernel, dim3(1), dim3(kDistillThreads), 0, s, partial, (int)nparts, (double)n, loss);
  return hipGetLastError();
}

hipError_t launch_ema_lerp(const OptTensor* tensors, const OptChunk* chunks, int nchunks, double decay, hipStream_t s) {
  if (!tensors || !chunks || nchunks <= 0 || !(decay >= 0.0 && decay <= 1.0)) return hipErrorInvalidValue;
  note_kernel("ema_lerp_kernel");
  hipLaunchKernelGGL(ema_lerp_kernel, dim3(nchunks), dim3(kDistillThreads), 0, s, tensors, chunks, (float)decay, (float)(1.0 - decay));
  return hipGetLastError();
}

}  // namespace llie
