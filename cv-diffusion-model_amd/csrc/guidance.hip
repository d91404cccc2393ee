// Classifier-free guidance: the elementwise arithmetic around a conditional and an unconditional denoiser call.
//
//   guide:          out = o_u + w (o_c - o_u)                 w: one host scalar, or a device fp32 value per row
//   guidance_pair:  latents2 = [latents; latents],  cond2 = [cond; 0]   the 2B-row input of one pass that runs both calls
//   cond_dropout:   out[b] = u[b] < p ? 0 : in[b]             a select: inf / NaN of a dropped row give +0, not NaN
//
// Tensors are fp32 [batch, per]; the kernels know nothing of H x W.  The difference, the product and the sum of `guide` are each
// rounded on their own (no fused multiply-add), like lcm_step_kernel and the distillation kernels, so the NumPy fp32 twins of
// guidance.py give the same bits.  The null condition is the all-zero image, positive-zero bits.
//
// One indexing serves the three kernels.  A row is `nvec` float4 items followed by per - 4 nvec scalar items (the tail); a thread
// owns one item, reads it, then writes it, so an output may alias the input it replaces.  nvec = per / 4 when every pointer is
// 16-byte aligned and every row starts 16-byte aligned (per % 4 == 0, or a single row); otherwise 0, and the whole row is tail.
// The value of an element does not depend on which kind of item carried it.
#include <cmath>
#include <initializer_list>

#include "common.h"
#include "kernels.h"

namespace llie {

constexpr int kGuideThreads = 256;

// item -> (is a float4, first element within the row); false past the row's end
__device__ __forceinline__ bool guide_item(int64_t item, int64_t nvec, int64_t per, bool& vec, int64_t& e) {
  vec = item < nvec;
  e = vec ? item * 4 : nvec * 4 + (item - nvec);
  return e < per;
}

// three operations, three roundings: contraction is off, as in lcm_step_kernel (w * d + u must not become one fma)
__device__ __forceinline__ float guide_one(float c, float u, float w) {
#pragma clang fp contract(off)
  const float d = c - u;
  const float p = w * d;
  return u + p;
}

__global__ void __launch_bounds__(kGuideThreads) guide_kernel(const float* oc, const float* ou, const float* __restrict__ w_rows, float w,
                                                              float* out, int batch, int64_t per, int64_t nvec) {
#pragma clang fp contract(off)
  const int64_t item = (int64_t)blockIdx.x * kGuideThreads + threadIdx.x;
  bool vec;
  int64_t e;
  if (!guide_item(item, nvec, per, vec, e)) return;
  for (int b = blockIdx.y; b < batch; b += gridDim.y) {
    const float wb = w_rows ? w_rows[b] : w;
    const size_t o = (size_t)b * per + e;
    if (vec) {
      const float4 c = *reinterpret_cast<const float4*>(oc + o);
      const float4 u = *reinterpret_cast<const float4*>(ou + o);
      *reinterpret_cast<float4*>(out + o) = make_float4(guide_one(c.x, u.x, wb), guide_one(c.y, u.y, wb), guide_one(c.z, u.z, wb),
                                                        guide_one(c.w, u.w, wb));
    } else {
      out[o] = guide_one(oc[o], ou[o], wb);
    }
  }
}

__global__ void __launch_bounds__(kGuideThreads) guidance_pair_kernel(const float* __restrict__ lat, const float* __restrict__ cond,
                                                                      float* __restrict__ lat2, float* __restrict__ cond2, int batch,
                                                                      int64_t per, int64_t nvec) {
  const int64_t item = (int64_t)blockIdx.x * kGuideThreads + threadIdx.x;
  bool vec;
  int64_t e;
  if (!guide_item(item, nvec, per, vec, e)) return;
  for (int b = blockIdx.y; b < batch; b += gridDim.y) {
    const size_t o = (size_t)b * per + e, o2 = (size_t)(b + batch) * per + e;
    if (vec) {
      const float4 x = *reinterpret_cast<const float4*>(lat + o);
      *reinterpret_cast<float4*>(lat2 + o) = x;
      *reinterpret_cast<float4*>(lat2 + o2) = x;
      *reinterpret_cast<float4*>(cond2 + o) = *reinterpret_cast<const float4*>(cond + o);
      *reinterpret_cast<float4*>(cond2 + o2) = make_float4(0.f, 0.f, 0.f, 0.f);
    } else {
      const float x = lat[o];
      lat2[o] = x;
      lat2[o2] = x;
      cond2[o] = cond[o];
      cond2[o2] = 0.f;
    }
  }
}

__global__ void __launch_bounds__(kGuideThreads) cond_dropout_kernel(const float* in, const float* __restrict__ u, float p, float* out,
                                                                     int batch, int64_t per, int64_t nvec) {
  const int64_t item = (int64_t)blockIdx.x * kGuideThreads + threadIdx.x;
  bool vec;
  int64_t e;
  if (!guide_item(item, nvec, per, vec, e)) return;
  for (int b = blockIdx.y; b < batch; b += gridDim.y) {
    const bool drop = u[b] < p;  // strict; a NaN uniform keeps the row
    const size_t o = (size_t)b * per + e;
    if (vec) *reinterpret_cast<float4*>(out + o) = drop ? make_float4(0.f, 0.f, 0.f, 0.f) : *reinterpret_cast<const float4*>(in + o);
    else out[o] = drop ? 0.f : in[o];
  }
}

// float4 items per row (0: every element is a tail item) and the grid that covers nvec + tail items of `batch` rows; `rows` is
// the row count of the tallest tensor (guidance_pair writes 2 * batch rows)
static bool guide_plan(std::initializer_list<const void*> ptrs, int rows, int batch, int64_t per, int64_t& nvec, dim3& grid) {
  uintptr_t bits = 0;
  for (const void* p : ptrs) bits |= reinterpret_cast<uintptr_t>(p);
  nvec = ((bits & 15) == 0 && (per % 4 == 0 || rows == 1)) ? per / 4 : 0;
  const int64_t items = nvec + (per - 4 * nvec);
  const int64_t blocks = (items + kGuideThreads - 1) / kGuideThreads;
  if (blocks > (int64_t)INT32_MAX) return false;
  grid = dim3((unsigned)blocks, (unsigned)(batch < 65535 ? batch : 65535));
  return true;
}

hipError_t launch_guide(const float* out_cond, const float* out_uncond, const float* w_rows, float w, float* out, int batch, int64_t per,
                        hipStream_t s) {
  if (!out_cond || !out_uncond || !out || batch <= 0 || per <= 0) return hipErrorInvalidValue;
  if (!w_rows && !std::isfinite(w)) return hipErrorInvalidValue;
  if ((reinterpret_cast<uintptr_t>(out_cond) | reinterpret_cast<uintptr_t>(out_uncond) | reinterpret_cast<uintptr_t>(out) |
       reinterpret_cast<uintptr_t>(w_rows)) & 3)
    return hipErrorInvalidValue;
  int64_t nvec;
  dim3 grid;
  if (!guide_plan({out_cond, out_uncond, out}, batch, batch, per, nvec, grid)) return hipErrorInvalidValue;
  note_kernel("guide_kernel");
  hipLaunchKernelGGL(guide_kernel, grid, dim3(kGuideThreads), 0, s, out_cond, out_uncond, w_rows, w, out, batch, per, nvec);
  return hipGetLastError();
}

hipError_t launch_guidance_pair(const float* latents, const float* cond, float* latents2, float* cond2, int batch, int64_t per, hipStream_t s) {
  if (!latents || !cond || !latents2 || !cond2 || batch <= 0 || per <= 0 || batch > INT32_MAX / 2) return hipErrorInvalidValue;
  if ((reinterpret_cast<uintptr_t>(latents) | reinterpret_cast<uintptr_t>(cond) | reinterpret_cast<uintptr_t>(latents2) |
       reinterpret_cast<uintptr_t>(cond2)) & 3)
    return hipErrorInvalidValue;
  int64_t nvec;
  dim3 grid;
  if (!guide_plan({latents, cond, latents2, cond2}, 2 * batch, batch, per, nvec, grid)) return hipErrorInvalidValue;
  note_kernel("guidance_pair_kernel");
  hipLaunchKernelGGL(guidance_pair_kernel, grid, dim3(kGuideThreads), 0, s, latents, cond, latents2, cond2, batch, per, nvec);
  return hipGetLastError();
}

hipError_t launch_cond_dropout(const float* in, const float* u, float p, float* out, int batch, int64_t per, hipStream_t s) {
  if (!in || !u || !out || batch <= 0 || per <= 0) return hipErrorInvalidValue;
  if (!std::isfinite(p) || p < 0.f || p > 1.f) return hipErrorInvalidValue;
  if ((reinterpret_cast<uintptr_t>(in) | reinterpret_cast<uintptr_t>(u) | reinterpret_cast<uintptr_t>(out)) & 3) return hipErrorInvalidValue;
  int64_t nvec;
  dim3 grid;
  if (!guide_plan({in, out}, batch, batch, per, nvec, grid)) return hipErrorInvalidValue;
  note_kernel("cond_dropout_kernel");
  hipLaunchKernelGGL(cond_dropout_kernel, grid, dim3(kGuideThreads), 0, s, in, u, p, out, batch, per, nvec);
  return hipGetLastError();
}

}  // namespace llie
