// Classifier-free guidance: the elementwise arithmetic around a conditional and an unconditional denoiser call.
//
//   guide:          out = o_u + w (o_c - o_u)                 w: one host scalar, or a device fp32 value per row
//   guidance_pair:  latents2 = [latents; latents],  cond2 = [cond; 0]   the 2B-row input of one pass that runs both calls
//   cond_dropout:   out[b] = u[b] < p ? 0 : in[b]             a select: inf / NaN of a dropped row give +0, not NaN
//   guide_rescale:  out = f_b g,  g the guided output above   f_b = phi r_b + (1 - phi), r_b = std(o_c[b]) / std(g[b]) (see below)
//
// Tensors are fp32 [batch, per]; the kernels know nothing of H x W.  The difference, the product and the sum of `guide` are each
// rounded on their own (no fused multiply-add), like lcm_step_kernel and the distillation kernels, so the NumPy fp32 twins of
// guidance.py give the same bits.  The null condition is the all-zero image, positive-zero bits.
//
// One indexing serves the three kernels.  A row is `nvec` float4 items followed by per - 4 nvec scalar items (the tail); a thread
// owns one item, reads it, then writes it, so an output may alias the input it replaces.  nvec = per / 4 when every pointer is
// 16-byte aligned and every row starts 16-byte aligned (per % 4 == 0, or a single row); otherwise 0, and the whole row is tail.
// The value of an element does not depend on which kind of item carried it.
//
// Guidance rescale (Lin et al. 2024, section 3.4; kernels.h (10b) and include/llie.h have the definition) is three launches:
//   guide_moments_kernel   one workgroup per (row, chunk of kGuideRescaleChunk elements); thread k owns the groups of 4 consecutive
//                          elements k, k + 256, ... of its chunk -- group j of a row is float4 item j where j < nvec, scalar items
//                          otherwise, the same elements in the same order -- recomputes g and adds o_c, o_c^2, g, g^2 in double in
//                          ascending order.  The four sums meet by wave shuffles, then through LDS in wave order: four doubles per
//                          workgroup into scratch, laid out [row][quantity][chunk].
//   guide_factor_kernel    one workgroup of four waves per row: wave q adds quantity q over the chunks in ascending order
//                          (coalesced loads, then lane reads in order); thread 0 forms f_b.
//   guide_kernel<true>     guide_kernel's items, each value multiplied by f_b.
// The partition of a row depends on per alone, so a row's factor and output are the same bits alone or in a batch.
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

// RESCALE: every value is multiplied by factor[b] (one more rounding); otherwise a non-null `factor` is set to 1
template <bool RESCALE>
__global__ void __launch_bounds__(kGuideThreads) guide_kernel(const float* oc, const float* ou, const float* __restrict__ w_rows, float w,
                                                              float* out, float* factor, int batch, int64_t per, int64_t nvec) {
#pragma clang fp contract(off)
  const int64_t item = (int64_t)blockIdx.x * kGuideThreads + threadIdx.x;
  bool vec;
  int64_t e;
  if (!guide_item(item, nvec, per, vec, e)) return;
  for (int b = blockIdx.y; b < batch; b += gridDim.y) {
    const float wb = w_rows ? w_rows[b] : w;
    const size_t o = (size_t)b * per + e;
    if constexpr (RESCALE) {
      const float f = factor[b];
      if (vec) {
        const float4 c = *reinterpret_cast<const float4*>(oc + o);
        const float4 u = *reinterpret_cast<const float4*>(ou + o);
        *reinterpret_cast<float4*>(out + o) = make_float4(f * guide_one(c.x, u.x, wb), f * guide_one(c.y, u.y, wb),
                                                          f * guide_one(c.z, u.z, wb), f * guide_one(c.w, u.w, wb));
      } else {
        out[o] = f * guide_one(oc[o], ou[o], wb);
      }
    } else {
      if (factor && item == 0) factor[b] = 1.f;
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
}

// ---- guidance rescale: the moments of a row and its factor
constexpr int kGuideGroups = (int)(kGuideRescaleChunk / (4 * kGuideThreads));  // groups of 4 elements per thread and chunk
static_assert(kGuideRescaleChunk == (int64_t)kGuideGroups * 4 * kGuideThreads, "a chunk is a whole number of float4 rounds of the workgroup");

struct GuideMoments { double s1c, s2c, s1g, s2g; };
// one element: widened first, so each square is exact
__device__ __forceinline__ void guide_moment_one(float c, float u, float w, GuideMoments& m) {
#pragma clang fp contract(off)
  const double dc = (double)c, dg = (double)guide_one(c, u, w);
  m.s1c = m.s1c + dc;
  m.s2c = m.s2c + dc * dc;
  m.s1g = m.s1g + dg;
  m.s2g = m.s2g + dg * dg;
}

__global__ void __launch_bounds__(kGuideThreads, 8) guide_moments_kernel(const float* __restrict__ oc_all, const float* __restrict__ ou_all,
                                                                         const float* __restrict__ w_rows, float w, double* __restrict__ partial,
                                                                         int64_t per, int64_t nvec, int64_t chunks) {
#pragma clang fp contract(off)
  __shared__ double red[kGuideThreads / 64][4];
  const int tid = threadIdx.x;
  const int b = (int)(blockIdx.x / chunks);
  const int64_t chunk = blockIdx.x - (int64_t)b * chunks;
  const float wb = w_rows ? w_rows[b] : w;
  const float* __restrict__ oc = oc_all + (size_t)b * per;
  const float* __restrict__ ou = ou_all + (size_t)b * per;
  const int64_t first = chunk * kGuideRescaleChunk;
  GuideMoments m{0.0, 0.0, 0.0, 0.0};
  if (first + kGuideRescaleChunk <= 4 * nvec) {
    // a whole chunk of float4 items: every load of the chunk may be in flight before the first use
    float4 c[kGuideGroups], u[kGuideGroups];
#pragma unroll
    for (int k = 0; k < kGuideGroups; ++k) {
      const int64_t e = first + (int64_t)(k * kGuideThreads + tid) * 4;
      c[k] = *reinterpret_cast<const float4*>(oc + e);
      u[k] = *reinterpret_cast<const float4*>(ou + e);
    }
#pragma unroll
    for (int k = 0; k < kGuideGroups; ++k) {
      guide_moment_one(c[k].x, u[k].x, wb, m);
      guide_moment_one(c[k].y, u[k].y, wb, m);
      guide_moment_one(c[k].z, u[k].z, wb, m);
      guide_moment_one(c[k].w, u[k].w, wb, m);
    }
  } else {
    for (int k = 0; k < kGuideGroups; ++k) {
      const int64_t e = first + (int64_t)(k * kGuideThreads + tid) * 4;
      if (e >= per) break;
      if (e + 4 <= 4 * nvec) {
        const float4 c = *reinterpret_cast<const float4*>(oc + e);
        const float4 u = *reinterpret_cast<const float4*>(ou + e);
        guide_moment_one(c.x, u.x, wb, m);
        guide_moment_one(c.y, u.y, wb, m);
        guide_moment_one(c.z, u.z, wb, m);
        guide_moment_one(c.w, u.w, wb, m);
      } else {
        const int cnt = per - e < 4 ? (int)(per - e) : 4;
        for (int j = 0; j < cnt; ++j) guide_moment_one(oc[e + j], ou[e + j], wb, m);
      }
    }
  }
  m.s1c = wave_sum(m.s1c);
  m.s2c = wave_sum(m.s2c);
  m.s1g = wave_sum(m.s1g);
  m.s2g = wave_sum(m.s2g);
  if ((tid & 63) == 0) {
    double* r = red[tid >> 6];
    r[0] = m.s1c; r[1] = m.s2c; r[2] = m.s1g; r[3] = m.s2g;
  }
  wg_barrier();
  if (tid < 4) {
    double s = red[0][tid];
#pragma unroll
    for (int k = 1; k < kGuideThreads / 64; ++k) s = s + red[k][tid];
    partial[((size_t)b * 4 + tid) * chunks + chunk] = s;
  }
}

// v[0] + v[1] + ... + v[n - 1] in that order: every lane of the wave returns the sum.  Four coalesced loads are in flight before
// the first lane read.
__device__ __forceinline__ double guide_ordered_sum(const double* __restrict__ v, int64_t n, int lane) {
#pragma clang fp contract(off)
  double acc = 0.0;
  for (int64_t base = 0; base < n; base += 256) {
    double x[4];
#pragma unroll
    for (int k = 0; k < 4; ++k) {
      const int64_t i = base + k * 64 + lane;
      x[k] = i < n ? v[i] : 0.0;
    }
#pragma unroll
    for (int k = 0; k < 4; ++k) {
      if (base + k * 64 >= n) break;  // uniform over the wave
      const int64_t left = n - (base + k * 64);
      if (left >= 64) {
#pragma unroll
        for (int j = 0; j < 64; ++j) acc = acc + __shfl(x[k], j, 64);
      } else {
        for (int j = 0; j < (int)left; ++j) acc = acc + __shfl(x[k], j, 64);  // no "+ 0.0": a sum of -0.0 keeps its sign
      }
    }
  }
  return acc;
}

__global__ void __launch_bounds__(256) guide_factor_kernel(const double* __restrict__ partial, float phi, float* __restrict__ f_scratch,
                                                           float* __restrict__ factor, int64_t per, int64_t chunks) {
#pragma clang fp contract(off)
  __shared__ double tot[4];
  const int tid = threadIdx.x, lane = tid & 63, q = tid >> 6;
  const int b = blockIdx.x;
  const double s = guide_ordered_sum(partial + ((size_t)b * 4 + q) * chunks, chunks, lane);
  if (lane == 0) tot[q] = s;
  wg_barrier();
  if (tid != 0) return;
  const double n = (double)per;
  const double mc = tot[0] * tot[0], mg = tot[2] * tot[2];
  const double dc = tot[1] - mc / n, dg = tot[3] - mg / n;
  const double var_c = dc > 0.0 ? dc : 0.0, var_g = dg > 0.0 ? dg : 0.0;  // a NaN becomes 0
  float r32 = 1.f;
  if (var_g > 0.0) {
    r32 = (float)sqrt(var_c / var_g);
    if (!(fabsf(r32) <= 3.4028234663852886e38f)) r32 = 1.f;
  }
  const float a = phi * r32;
  const float c = 1.f - phi;
  const float f = a + c;
  f_scratch[b] = f;
  if (factor) factor[b] = f;
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

// the checks llie_guide and llie_guide_rescale share
static bool guide_args_ok(const float* out_cond, const float* out_uncond, const float* w_rows, float w, const float* out, const float* factor,
                          int batch, int64_t per) {
  if (!out_cond || !out_uncond || !out || batch <= 0 || per <= 0) return false;
  if (!w_rows && !std::isfinite(w)) return false;
  return ((reinterpret_cast<uintptr_t>(out_cond) | reinterpret_cast<uintptr_t>(out_uncond) | reinterpret_cast<uintptr_t>(out) |
           reinterpret_cast<uintptr_t>(w_rows) | reinterpret_cast<uintptr_t>(factor)) & 3) == 0;
}

static hipError_t launch_guide_ones(const float* out_cond, const float* out_uncond, const float* w_rows, float w, float* out, float* factor,
                                    int batch, int64_t per, hipStream_t s) {
  if (!guide_args_ok(out_cond, out_uncond, w_rows, w, out, factor, batch, per)) return hipErrorInvalidValue;
  int64_t nvec;
  dim3 grid;
  if (!guide_plan({out_cond, out_uncond, out}, batch, batch, per, nvec, grid)) return hipErrorInvalidValue;
  note_kernel("guide_kernel");
  hipLaunchKernelGGL(guide_kernel<false>, grid, dim3(kGuideThreads), 0, s, out_cond, out_uncond, w_rows, w, out, factor, batch, per, nvec);
  return hipGetLastError();
}

hipError_t launch_guide(const float* out_cond, const float* out_uncond, const float* w_rows, float w, float* out, int batch, int64_t per,
                        hipStream_t s) {
  return launch_guide_ones(out_cond, out_uncond, w_rows, w, out, nullptr, batch, per, s);
}

hipError_t launch_guide_rescale(const float* out_cond, const float* out_uncond, const float* w_rows, float w, float phi, float* out,
                                float* factor, void* scratch, int batch, int64_t per, hipStream_t s) {
  if (!guide_args_ok(out_cond, out_uncond, w_rows, w, out, factor, batch, per)) return hipErrorInvalidValue;
  if (!scratch || (reinterpret_cast<uintptr_t>(scratch) & 7) || !std::isfinite(phi) || phi < 0.f || phi > 1.f) return hipErrorInvalidValue;
  const int64_t chunks = guide_rescale_chunks(per);
  if (guide_rescale_scratch_bytes(batch, per) < 0) return hipErrorInvalidValue;
  if (phi == 0.f) return launch_guide_ones(out_cond, out_uncond, w_rows, w, out, factor, batch, per, s);
  int64_t nvec;
  dim3 grid;
  if (!guide_plan({out_cond, out_uncond, out}, batch, batch, per, nvec, grid)) return hipErrorInvalidValue;
  // scratch: the partials [batch][4][chunks] (doubles) first, then the factors [batch]
  double* partial = reinterpret_cast<double*>(scratch);
  float* f_scratch = reinterpret_cast<float*>(partial + (size_t)batch * 4 * chunks);
  // the moments read the inputs alone: their float4 items do not depend on how `out` is aligned, and neither do the bits
  int64_t nvec_in;
  dim3 unused;
  guide_plan({out_cond, out_uncond}, batch, batch, per, nvec_in, unused);
  note_kernel("guide_moments_kernel");
  hipLaunchKernelGGL(guide_moments_kernel, dim3((unsigned)((int64_t)batch * chunks)), dim3(kGuideThreads), 0, s, out_cond, out_uncond, w_rows, w,
                     partial, per, nvec_in, chunks);
  hipError_t e = hipGetLastError();
  if (e != hipSuccess) return e;
  note_kernel("guide_factor_kernel");
  hipLaunchKernelGGL(guide_factor_kernel, dim3((unsigned)batch), dim3(256), 0, s, partial, phi, f_scratch, factor, per, chunks);
  e = hipGetLastError();
  if (e != hipSuccess) return e;
  note_kernel("guide_rescale_apply_kernel");
  hipLaunchKernelGGL(guide_kernel<true>, grid, dim3(kGuideThreads), 0, s, out_cond, out_uncond, w_rows, w, out, f_scratch, batch, per, nvec);
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
