// The noise-space training loss with a per-sample Min-SNR-gamma weight (Hang et al., ICCV 2023), its per-sample values and
// d(loss)/d(pred), in one read of pred and target and one write of the gradient (kernels.h (16) and include/llie.h have the
// definition; snrloss.py the float64 definition and the fp32 twin).  snr_gamma is the gamma of
//   epsilon prediction  w_b = min(SNR, gamma) / SNR        = min(1, gamma (1 - abar) / abar),  1 at abar == 0
//   v prediction        w_b = min(SNR, gamma) / (SNR + 1)  = min(abar, gamma (1 - abar))
// with abar = alphas_cumprod[t_b] and SNR = abar / (1 - abar).
//
//   snr_loss_chunk (pass 1):    one workgroup of 256 threads per (sample, chunk of kSnrChunk elements); the chunk count of a
//                               sample depends on per_sample alone.  Thread k owns the groups of 4 consecutive elements
//                               k, k + 256, ... of its chunk (kSnrGroups of them) and adds l(d) of its elements in ascending
//                               order into one fp32 partial; a group is one 16-byte access per tensor where the row start and
//                               the three pointers are 16-byte aligned and the group lies inside the row, else up to 4 scalar
//                               accesses -- the same elements in the same order, so the bits do not depend on the path.  The
//                               partials meet by wave shuffles, then through LDS: one store per workgroup into scratch.  Every
//                               workgroup reads t_b and its table entry once and forms w_b and c_b itself.
//   snr_loss_finalize (pass 2): one workgroup of 16 waves.  Wave k takes samples k, k + 16, ...: it adds the sample's partials in
//                               ascending chunk order in double (coalesced loads, then lane reads in order), writes
//                               sample_loss and weight; then wave 0 adds w_b m_b over b in ascending order the same way.
//
// The gradient's arithmetic is fp32, one rounding per operation written in the definition, no fused multiply-add (contraction
// is off, as in guidance.hip and solver.hip), so snrloss.snr_loss_f32 gives its bits.  No atomics: every gradient element has
// one writer, the order of every sum depends on per_sample alone (m_b) or on the batch alone (the total).
// A timestep outside the table never indexes it: abar is NaN, and so are w_b, the sample's gradient rows and the total.
#include "common.h"
#include "kernels.h"

#include <cmath>

namespace llie {

constexpr int kSnrThreads = 256;
constexpr int kSnrFinalThreads = 1024;  // pass 2: 16 waves, one sample each at a time
constexpr int kSnrGroups = (int)(kSnrChunk / (4 * kSnrThreads));  // groups of 4 elements per thread and chunk
static_assert(kSnrChunk == (int64_t)kSnrGroups * 4 * kSnrThreads, "a chunk is a whole number of float4 rounds of the workgroup");

struct SnrArgs {
  const float* pred; const float* target;
  const int64_t* t; const float* acp; int table_len;
  int velocity; float gamma;
  float* d_pred;       // stored (GRAD instantiations only)
  float* partial;      // [batch][chunks]
  int batch; int64_t per; int64_t chunks;
  int vec;             // 16-byte accesses are allowed: the three pointers and every row start are 16-byte aligned
};

// w_b; NaN for a timestep outside the table (it never indexes the table).  Each operation is rounded on its own.
__device__ __forceinline__ float snr_weight(const int64_t* __restrict__ t, const float* __restrict__ acp, int table_len, int b, int velocity,
                                            float gamma) {
#pragma clang fp contract(off)
  const int64_t tb = t[b];
  if (tb < 0 || tb >= table_len) return __builtin_nanf("");
  const float a = acp[tb];
  const float om = 1.f - a;
  const float g = gamma * om;
  if (a != a) return a;
  if (velocity) return a < g ? a : g;
  if (a == 0.f) return 1.f;
  const float r = g / a;
  return r < 1.f ? r : 1.f;
}

template <int LOSS>
__device__ __forceinline__ float snr_term(float d) {
#pragma clang fp contract(off)
  if constexpr (LOSS == kLossMse) return d * d;
  else if constexpr (LOSS == kLossL1) return fabsf(d);
  else {
    const float z = fabsf(d);
    const float h = 0.5f * d;
    return z < 1.f ? h * d : z - 0.5f;  // F.huber_loss, delta = 1 (NaN takes the second branch and stays NaN)
  }
}
template <int LOSS>
__device__ __forceinline__ float snr_slope(float d) {
  if constexpr (LOSS == kLossMse) return 2.f * d;
  else if constexpr (LOSS == kLossL1) return d > 0.f ? 1.f : (d < 0.f ? -1.f : d);  // torch.sign: 0 at 0, NaN stays NaN
  else return d <= -1.f ? -1.f : (d >= 1.f ? 1.f : d);                               // huber_loss_backward; NaN falls through
}

// one element: adds l(d) into acc, returns l'(d) c
template <int LOSS>
__device__ __forceinline__ float snr_one(float p, float y, float c, float& acc) {
#pragma clang fp contract(off)
  const float d = p - y;
  const float l = snr_term<LOSS>(d);
  acc = acc + l;
  const float s = snr_slope<LOSS>(d);
  return s * c;
}

template <int LOSS, bool GRAD>
__global__ void __launch_bounds__(kSnrThreads, 8) snr_loss_chunk_kernel(SnrArgs p) {
#pragma clang fp contract(off)
  __shared__ float red[kSnrThreads / 64];
  const int tid = threadIdx.x;
  const int b = (int)(blockIdx.x / p.chunks);
  const int64_t chunk = blockIdx.x - (int64_t)b * p.chunks;
  const int64_t per = p.per;
  float c = 0.f;
  if constexpr (GRAD) {
    const float w = snr_weight(p.t, p.acp, p.table_len, b, p.velocity, p.gamma);
    const float wb = w / (float)p.batch;
    c = wb / (float)per;
  }
  const int64_t first = chunk * kSnrChunk;
  const float* __restrict__ pr = p.pred + (size_t)b * per;
  const float* __restrict__ tg = p.target + (size_t)b * per;
  float* __restrict__ dp = GRAD ? p.d_pred + (size_t)b * per : nullptr;
  float acc = 0.f;
  if (p.vec && first + kSnrChunk <= per) {
    // a whole chunk of aligned groups: every load of the chunk may be in flight before the first use
    float4 a[kSnrGroups], y[kSnrGroups];
#pragma unroll
    for (int k = 0; k < kSnrGroups; ++k) {
      const int64_t e = first + (int64_t)(k * kSnrThreads + tid) * 4;
      a[k] = *reinterpret_cast<const float4*>(pr + e);
      y[k] = *reinterpret_cast<const float4*>(tg + e);
    }
#pragma unroll
    for (int k = 0; k < kSnrGroups; ++k) {
      const int64_t e = first + (int64_t)(k * kSnrThreads + tid) * 4;
      float4 g;
      g.x = snr_one<LOSS>(a[k].x, y[k].x, c, acc);
      g.y = snr_one<LOSS>(a[k].y, y[k].y, c, acc);
      g.z = snr_one<LOSS>(a[k].z, y[k].z, c, acc);
      g.w = snr_one<LOSS>(a[k].w, y[k].w, c, acc);
      if constexpr (GRAD) *reinterpret_cast<float4*>(dp + e) = g;
    }
  } else {
    for (int k = 0; k < kSnrGroups; ++k) {
      const int64_t e = first + (int64_t)(k * kSnrThreads + tid) * 4;
      if (e >= per) break;
      if (p.vec && e + 4 <= per) {
        const float4 a = *reinterpret_cast<const float4*>(pr + e);
        const float4 y = *reinterpret_cast<const float4*>(tg + e);
        float4 g;
        g.x = snr_one<LOSS>(a.x, y.x, c, acc);
        g.y = snr_one<LOSS>(a.y, y.y, c, acc);
        g.z = snr_one<LOSS>(a.z, y.z, c, acc);
        g.w = snr_one<LOSS>(a.w, y.w, c, acc);
        if constexpr (GRAD) *reinterpret_cast<float4*>(dp + e) = g;
      } else {
        const int m = per - e < 4 ? (int)(per - e) : 4;
        for (int j = 0; j < m; ++j) {
          const float g = snr_one<LOSS>(pr[e + j], tg[e + j], c, acc);
          if constexpr (GRAD) dp[e + j] = g;
        }
      }
    }
  }
  acc = wave_sum(acc);
  if ((tid & 63) == 0) red[tid >> 6] = acc;
  wg_barrier();
  if (tid == 0) {
    float s = red[0];
#pragma unroll
    for (int k = 1; k < kSnrThreads / 64; ++k) s = s + red[k];
    p.partial[blockIdx.x] = s;
  }
}

// v[0] + v[1] + ... + v[n - 1] in that order, in double: every lane of the wave returns the sum.  load(i) is called with
// i < n only.  Four coalesced loads are in flight before the first lane read, so a long row pays a load's latency once per 256
// values.
template <typename F>
__device__ __forceinline__ double snr_ordered_sum(int64_t n, int lane, F&& load) {
  double acc = 0.0;
  for (int64_t base = 0; base < n; base += 256) {
    double v[4];
#pragma unroll
    for (int k = 0; k < 4; ++k) {
      const int64_t i = base + k * 64 + lane;
      v[k] = i < n ? load(i) : 0.0;  // acc + 0.0 leaves acc as it is
    }
#pragma unroll
    for (int k = 0; k < 4; ++k) {
      if (base + k * 64 >= n) break;  // uniform over the wave
#pragma unroll
      for (int j = 0; j < 64; ++j) acc = acc + __shfl(v[k], j, 64);
    }
  }
  return acc;
}

__global__ void __launch_bounds__(kSnrFinalThreads) snr_loss_finalize_kernel(SnrArgs p, double* mean, float* __restrict__ loss,
                                                                        float* __restrict__ sample_loss, float* __restrict__ weight) {
  const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
  for (int b = wave; b < p.batch; b += kSnrFinalThreads / 64) {
    const float* src = p.partial + (size_t)b * p.chunks;
    const double sum = snr_ordered_sum(p.chunks, lane, [&](int64_t i) { return (double)src[i]; });
    if (lane == 0) {
      const double m = sum / (double)p.per;
      mean[b] = m;
      if (sample_loss) sample_loss[b] = (float)m;
      if (weight) weight[b] = snr_weight(p.t, p.acp, p.table_len, b, p.velocity, p.gamma);
    }
  }
  __threadfence_block();
  wg_barrier();
  if (wave != 0) return;
  const double tot = snr_ordered_sum(p.batch, lane, [&](int64_t b) {
    return (double)snr_weight(p.t, p.acp, p.table_len, (int)b, p.velocity, p.gamma) * mean[b];
  });
  if (lane == 0) *loss = (float)(tot / (double)p.batch);
}

hipError_t launch_snr_loss(const SnrLossArgs& x, void* scratch, hipStream_t s) {
  if (!x.pred || !x.target || !x.t || !x.acp || !x.loss || !scratch || x.table_len < 1 || !(x.gamma > 0.f) || !std::isfinite(x.gamma))
    return hipErrorInvalidValue;
  const int64_t chunks = snr_loss_chunks(x.per);
  if (x.batch < 1 || chunks < 1 || (int64_t)x.batch * chunks > (int64_t)INT32_MAX) return hipErrorInvalidValue;
  if (x.loss_type != kLossMse && x.loss_type != kLossL1 && x.loss_type != kLossHuber) return hipErrorInvalidValue;
  SnrArgs p{};
  p.pred = x.pred; p.target = x.target; p.t = x.t; p.acp = x.acp; p.table_len = x.table_len; p.velocity = x.velocity != 0;
  p.gamma = x.gamma; p.d_pred = x.d_pred; p.batch = x.batch; p.per = x.per; p.chunks = chunks;
  // scratch: the per-sample means (doubles) first, then the per-workgroup partials
  double* mean = reinterpret_cast<double*>(scratch);
  p.partial = reinterpret_cast<float*>(mean + x.batch);
  const uintptr_t bits = reinterpret_cast<uintptr_t>(x.pred) | reinterpret_cast<uintptr_t>(x.target) | reinterpret_cast<uintptr_t>(x.d_pred);
  p.vec = (bits & 15) == 0 && (x.per % 4 == 0 || x.batch == 1);
  const dim3 grid((unsigned)(x.batch * chunks)), block(kSnrThreads);
  const bool grad = x.d_pred != nullptr;
  note_kernel("snr_loss_chunk_kernel");
  const hipError_t e = with_value<kLossMse, kLossL1, kLossHuber>(x.loss_type, [&](auto L) {
    constexpr int LOSS = decltype(L)::value;
    if (grad) hipLaunchKernelGGL((snr_loss_chunk_kernel<LOSS, true>), grid, block, 0, s, p);
    else hipLaunchKernelGGL((snr_loss_chunk_kernel<LOSS, false>), grid, block, 0, s, p);
    return hipGetLastError();
  });
  if (e != hipSuccess) return e;
  note_kernel("snr_loss_finalize_kernel");
  hipLaunchKernelGGL(snr_loss_finalize_kernel, dim3(1), dim3(kSnrFinalThreads), 0, s, p, mean, x.loss, x.sample_loss, x.weight);
  return hipGetLastError();
}

}  // namespace llie
