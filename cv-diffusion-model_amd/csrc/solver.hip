// DPM-Solver++ 2M, data-prediction form: one step of the second-order multistep sampler of a many-step (teacher) model.
//
//   x0   = (x - sb out) / sa  |  sa x - sb out          epsilon | v prediction: the DDIM branch of lcm_step_kernel, unchanged
//   a = k_x x;  b = k_0 x0;  s = a + b;                 order 2 only:  d = k_1 h;  s = s + d        h: the previous step's x0
//   prev = is_last ? x0 : s;   hist <- x0;   clamped = clip(prev, -1, 1)
//
// The scalars come from the host (dpm.py: float64, rounded once to fp32).  Every multiply and add is rounded on its own (no fused
// multiply-add), like lcm_step_kernel and guide_kernel, so dpm.dpm_step_f32 gives the same bits.
//
// Tensors are fp32 [n]; the kernel knows nothing of B x 3 x H x W.  The indexing is guidance.hip's for a single row: `nvec` float4
// items followed by n - 4 nvec scalar items (the tail).  A thread owns one item, reads it from every input, then writes it, so
// `prev` may alias `x` and `hist` is updated in place.  nvec = n / 4 when every pointer is 16-byte aligned, otherwise 0 and every
// element is a tail item.  The value of an element does not depend on which kind of item carried it.
#include <cmath>

#include "common.h"
#include "kernels.h"

namespace llie {

constexpr int kDpmThreads = 256;

struct DpmPair { float prev, x0; };

__device__ __forceinline__ DpmPair dpm_one(float e, float xv, float h, const DpmCoef& c) {
#pragma clang fp contract(off)
  float x0;
  if (c.vpred) x0 = c.sa * xv - c.sb * e;
  else x0 = (xv - c.sb * e) / c.sa;
  const float a = c.kx * xv;
  const float b = c.k0 * x0;
  float s = a + b;
  if (c.order == 2) {
    const float d = c.k1 * h;
    s = s + d;
  }
  return DpmPair{c.is_last ? x0 : s, x0};
}

__device__ __forceinline__ float clamp1(float v) { return fminf(fmaxf(v, -1.f), 1.f); }

__global__ void __launch_bounds__(kDpmThreads) dpm_step_kernel(const float* out, const float* x, float* hist, float* prev, float* clamped,
                                                               int64_t n, int64_t nvec, DpmCoef c) {
#pragma clang fp contract(off)
  const int64_t item = (int64_t)blockIdx.x * kDpmThreads + threadIdx.x;
  const bool second = c.order == 2;
  if (item < nvec) {
    const size_t o = (size_t)item * 4;
    const float4 e = *reinterpret_cast<const float4*>(out + o);
    const float4 xv = *reinterpret_cast<const float4*>(x + o);
    const float4 h = second ? *reinterpret_cast<const float4*>(hist + o) : make_float4(0.f, 0.f, 0.f, 0.f);
    const DpmPair r0 = dpm_one(e.x, xv.x, h.x, c), r1 = dpm_one(e.y, xv.y, h.y, c), r2 = dpm_one(e.z, xv.z, h.z, c),
                  r3 = dpm_one(e.w, xv.w, h.w, c);
    *reinterpret_cast<float4*>(prev + o) = make_float4(r0.prev, r1.prev, r2.prev, r3.prev);
    if (hist) *reinterpret_cast<float4*>(hist + o) = make_float4(r0.x0, r1.x0, r2.x0, r3.x0);
    if (clamped) *reinterpret_cast<float4*>(clamped + o) = make_float4(clamp1(r0.prev), clamp1(r1.prev), clamp1(r2.prev), clamp1(r3.prev));
    return;
  }
  const int64_t i = nvec * 4 + (item - nvec);
  if (i >= n) return;
  const DpmPair r = dpm_one(out[i], x[i], second ? hist[i] : 0.f, c);
  prev[i] = r.prev;
  if (hist) hist[i] = r.x0;
  if (clamped) clamped[i] = clamp1(r.prev);
}

bool dpm_coef_ok(const DpmCoef& c) {
  return (c.order == 1 || c.order == 2) && std::isfinite(c.sa) && std::isfinite(c.sb) && std::isfinite(c.kx) && std::isfinite(c.k0) &&
         std::isfinite(c.k1);
}

hipError_t launch_dpm_step(const float* out, const float* x, float* hist, float* prev, float* clamped, int64_t n, const DpmCoef& c,
                           hipStream_t s) {
  if (!out || !x || !prev || n <= 0 || !dpm_coef_ok(c)) return hipErrorInvalidValue;
  if (!hist && !(c.order == 1 && c.is_last)) return hipErrorInvalidValue;  // every other step leaves its x0 for the next one
  const uintptr_t bits = reinterpret_cast<uintptr_t>(out) | reinterpret_cast<uintptr_t>(x) | reinterpret_cast<uintptr_t>(hist) |
                         reinterpret_cast<uintptr_t>(prev) | reinterpret_cast<uintptr_t>(clamped);
  if (bits & 3) return hipErrorInvalidValue;
  const int64_t nvec = (bits & 15) == 0 ? n / 4 : 0;
  const int64_t items = nvec + (n - 4 * nvec);
  const int64_t blocks = (items + kDpmThreads - 1) / kDpmThreads;
  if (blocks > (int64_t)INT32_MAX) return hipErrorInvalidValue;
  note_kernel("dpm_step_kernel");
  hipLaunchKernelGGL(dpm_step_kernel, dim3((unsigned)blocks), dim3(kDpmThreads), 0, s, out, x, hist, prev, clamped, n, nvec, c);
  return hipGetLastError();
}

}  // namespace llie
