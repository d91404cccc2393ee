// Device-resident paired data loader: one launch turns rows [first, first + count) of an epoch plan into the two fp32 NCHW
// batches TrainStep takes, reading uint8 frames that stay in HBM (kernels.h (12) has the layouts).  aug_pair_u8 is bit-exact
// with augment_pairs_host in data.py; aug_synth_u8 differs from augment_synth_host only through powf.
//
// The crop is SH rows by SW columns (the square entry points: SH = SW = S).
//   crop(yy, xx) = frame[y0 + (vflip ? SH-1-yy : yy)][x0 + (hflip ? SW-1-xx : xx)]
//   aug_pair_u8, per output pixel (y, x), the same for the low and the high frame:
//     no rotate:  byte = crop(y, x)
//     rotate:     cx = (SW-1) * 0.5f, cy = (SH-1) * 0.5f, u = x - cx, v = y - cy;  xs = (ca*u + sa*v) + cx;  ys = ((-sa)*u + ca*v) + cy
//                 x0i = floor(xs), fx = xs - x0i (y likewise); taps at r(x0i), r(x0i+1) (reflect-101 in SW), r(y0i), r(y0i+1) (in SH)
//                 top = p00*(1-fx) + p01*fx;  bot = p10*(1-fx) + p11*fx;  out = top*(1-fy) + bot*fy
//                 byte = clip(floor(out + 0.5f), 0, 255)                            (every multiply and add on its own)
//   aug_synth_u8 (SyntheticLowLightDataset._create_low_light): nb = crop(y, x) with hflip only;
//                 d = lut[nb], lut[k] = powf(k / 255f, gamma);  n = clamp(d + level * z, 0, 1);  n = clamp(n * scale[c], 0, 1)
//                 low byte = (uint8) trunc(n * 255f);  normal byte = nb
//   both:         value = float(byte) / 127.5f - 1.0f
//
// A workgroup belongs to one sample, so the plan row, the rotate branch and the gamma table are uniform in it.  A thread owns
// four consecutive x of one output row: 12 pixel bytes (three dwords when aligned) and 16 bytes of each fp32 plane.  The frame
// index and the crop origin are clamped into the store, and rows and columns into the frame: a corrupt plan row gives wrong
// pixels, never a read outside the pool.  No atomics, fixed order.
#include "common.h"
#include "kernels.h"

namespace llie {

constexpr int kAugThreads = 256;

struct AugFrame {
  const uint8_t* base;
  int H, W, y0, x0;
};

__device__ __forceinline__ AugFrame aug_frame(const AugArgs& a, int index, int y0, int x0) {
  const int64_t* t = a.table + (size_t)min(max(index, 0), a.N - 1) * 3;
  AugFrame f;
  f.base = a.pool + t[0];
  f.H = (int)t[1];
  f.W = (int)t[2];
  f.y0 = max(min(y0, f.H - a.SH), 0);
  f.x0 = max(min(x0, f.W - a.SW), 0);
  return f;
}
__device__ __forceinline__ const uint8_t* aug_row(const AugFrame& f, int yy, int SH, int flags) {
  const int r = f.y0 + ((flags & kAugVflip) ? SH - 1 - yy : yy);
  return f.base + (size_t)min(r, f.H - 1) * f.W * 3;
}
__device__ __forceinline__ int aug_col(const AugFrame& f, int xx, int SW, int flags) {
  return min(f.x0 + ((flags & kAugHflip) ? SW - 1 - xx : xx), f.W - 1);
}

// the bytes of crop(y, x0 .. x0+3): one 12-byte run of the frame, reversed pixel by pixel under hflip
__device__ __forceinline__ void aug_crop_quad(const AugFrame& f, int y, int x0, int SH, int SW, int flags, uint32_t (&b)[12]) {
  const uint8_t* row = aug_row(f, y, SH, flags);
  const bool flip = flags & kAugHflip;
  const int X = f.x0 + (flip ? SW - 1 - (x0 + 3) : x0);  // the leftmost frame column of the run
  if (x0 + 3 < SW && X + 3 < f.W) {
    uint32_t t[12];
    load12(row + (size_t)X * 3, t);
#pragma unroll
    for (int k = 0; k < 4; ++k)
#pragma unroll
      for (int c = 0; c < 3; ++c) b[k * 3 + c] = flip ? t[(3 - k) * 3 + c] : t[k * 3 + c];
  } else {  // the row ends inside this quad (SW % 4 != 0), or the table names a frame narrower than the crop
#pragma unroll
    for (int k = 0; k < 4; ++k) {
      const uint8_t* px = row + (size_t)aug_col(f, min(x0 + k, SW - 1), SW, flags) * 3;
#pragma unroll
      for (int c = 0; c < 3; ++c) b[k * 3 + c] = px[c];
    }
  }
}

__device__ __forceinline__ int aug_reflect(int i, int S) {
  i = i < 0 ? -i : (i >= S ? 2 * (S - 1) - i : i);
  return min(max(i, 0), S - 1);  // acts only on a corrupt (ca, sa)
}

// the rotated bytes of output pixels (y, x0 .. x0+3)
__device__ __forceinline__ void aug_rotate_quad(const AugFrame& f, int y, int x0, int SH, int SW, int flags, float ca, float sa,
                                                uint32_t (&b)[12]) {
#pragma clang fp contract(off)
  const float cx = (float)(SW - 1) * 0.5f, cy = (float)(SH - 1) * 0.5f;
  const float v = (float)y - cy;
#pragma unroll
  for (int k = 0; k < 4; ++k) {
    const float u = (float)(x0 + k) - cx;
    const float xs = (ca * u + sa * v) + cx;
    const float ys = ((-sa) * u + ca * v) + cy;
    const float xf = floorf(xs), yf = floorf(ys);
    const float fx = xs - xf, fy = ys - yf;
    const float gx = 1.0f - fx, gy = 1.0f - fy;
    const int xi = (int)xf, yi = (int)yf;
    const uint8_t* r0 = aug_row(f, aug_reflect(yi, SH), SH, flags);
    const uint8_t* r1 = aug_row(f, aug_reflect(yi + 1, SH), SH, flags);
    const int c0 = aug_col(f, aug_reflect(xi, SW), SW, flags) * 3;
    const int c1 = aug_col(f, aug_reflect(xi + 1, SW), SW, flags) * 3;
#pragma unroll
    for (int ch = 0; ch < 3; ++ch) {
      const float p00 = (float)r0[c0 + ch], p01 = (float)r0[c1 + ch], p10 = (float)r1[c0 + ch], p11 = (float)r1[c1 + ch];
      const float top = p00 * gx + p01 * fx;
      const float bot = p10 * gx + p11 * fx;
      const float out = top * gy + bot * fy;
      b[k * 3 + ch] = (uint32_t)fminf(fmaxf(floorf(out + 0.5f), 0.f), 255.f);
    }
  }
}

// sample j, row y, columns x0 .. x0+3: normalised values into the three fp32 planes, the bytes themselves into `u8` (or null)
__device__ __forceinline__ void aug_store_quad(const uint32_t (&b)[12], int j, int y, int x0, int SH, int SW, float* __restrict__ out,
                                               uint8_t* __restrict__ u8) {
#pragma clang fp contract(off)
  float* dst = out + (((size_t)j * 3) * SH + y) * SW + x0;
#pragma unroll
  for (int c = 0; c < 3; ++c, dst += (size_t)SH * SW) {
    f32x4 val;
#pragma unroll
    for (int k = 0; k < 4; ++k) val[k] = (float)b[k * 3 + c] / 127.5f - 1.0f;
    if (x0 + 3 < SW) {
      *reinterpret_cast<f32x4u*>(dst) = val;
    } else {
#pragma unroll
      for (int k = 0; k < 4; ++k)
        if (x0 + k < SW) dst[k] = val[k];
    }
  }
  if (u8) {
    uint8_t* d = u8 + (((size_t)j * SH + y) * SW + x0) * 3;
    if (x0 + 3 < SW) {
      store12(d, b);
    } else {
      for (int i = 0; i < (SW - x0) * 3; ++i) d[i] = (uint8_t)b[i];
    }
  }
}

// grid.x = count * bps (bps workgroups cover the SH * ceil(SW/4) quads of a sample)
__global__ void __launch_bounds__(kAugThreads) aug_pair_u8_kernel(AugArgs a, int bps) {
  const int SH = a.SH, SW = a.SW, qpr = (SW + 3) >> 2;
  const int j = blockIdx.x / bps;
  const int q = (blockIdx.x - j * bps) * kAugThreads + threadIdx.x;
  if (q >= qpr * SH) return;
  const int y = q / qpr, x0 = (q - y * qpr) * 4;
  const AugRow row = a.plan[a.first + j];
  const AugFrame lo = aug_frame(a, row.low_frame, row.y0, row.x0), hi = aug_frame(a, row.high_frame, row.y0, row.x0);
  uint32_t bl[12], bh[12];
  if (row.flags & kAugRotate) {
    aug_rotate_quad(lo, y, x0, SH, SW, row.flags, row.ca, row.sa, bl);
    aug_rotate_quad(hi, y, x0, SH, SW, row.flags, row.ca, row.sa, bh);
  } else {
    aug_crop_quad(lo, y, x0, SH, SW, row.flags, bl);
    aug_crop_quad(hi, y, x0, SH, SW, row.flags, bh);
  }
  aug_store_quad(bl, j, y, x0, SH, SW, a.low, a.low_u8);
  aug_store_quad(bh, j, y, x0, SH, SW, a.high, a.high_u8);
}

__global__ void __launch_bounds__(kAugThreads) aug_synth_u8_kernel(AugArgs a, int bps) {
#pragma clang fp contract(off)
  __shared__ float lut[256];
  const int SH = a.SH, SW = a.SW, qpr = (SW + 3) >> 2;
  const int j = blockIdx.x / bps;
  const AugRow row = a.plan[a.first + j];
  lut[threadIdx.x] = powf((float)threadIdx.x / 255.0f, row.gamma);  // kAugThreads == 256 entries
  __syncthreads();
  const int q = (blockIdx.x - j * bps) * kAugThreads + threadIdx.x;
  if (q >= qpr * SH) return;
  const int y = q / qpr, x0 = (q - y * qpr) * 4;
  const AugFrame f = aug_frame(a, row.high_frame, row.y0, row.x0);
  uint32_t nb[12], lb[12];
  aug_crop_quad(f, y, x0, SH, SW, row.flags & kAugHflip, nb);
  const float* zp = a.z + (((size_t)j * SH + y) * SW + x0) * 3;
  float z[12];
  if (x0 + 3 < SW) {
#pragma unroll
    for (int i = 0; i < 3; ++i) {
      const f32x4 t = *reinterpret_cast<const f32x4u*>(zp + i * 4);
#pragma unroll
      for (int k = 0; k < 4; ++k) z[i * 4 + k] = t[k];
    }
  } else {
#pragma unroll
    for (int i = 0; i < 12; ++i) z[i] = i < (SW - x0) * 3 ? zp[i] : 0.f;
  }
#pragma unroll
  for (int k = 0; k < 4; ++k)
#pragma unroll
    for (int c = 0; c < 3; ++c) {
      const float t = row.level * z[k * 3 + c];
      float n = fminf(fmaxf(lut[nb[k * 3 + c]] + t, 0.f), 1.f);
      n = fminf(fmaxf(n * row.scale[c], 0.f), 1.f);
      lb[k * 3 + c] = (uint32_t)truncf(n * 255.0f);
    }
  aug_store_quad(lb, j, y, x0, SH, SW, a.low, a.low_u8);
  aug_store_quad(nb, j, y, x0, SH, SW, a.high, a.high_u8);
}

static_assert(kAugThreads == 256, "aug_synth_u8_kernel fills its 256-entry gamma table with one thread per entry");

// workgroups per sample, or 0 when the launch is outside the contract
static int aug_blocks_per_sample(const AugArgs& a, bool synth) {
  if (!a.pool || !a.table || !a.plan || !a.low || !a.high || (synth && !a.z) || a.N < 1 || a.SH < 1 || a.SW < 1 || a.first < 0 || a.count < 0 ||
      (long long)a.first + a.count >= (1ll << 31))
    return 0;
  const long long quads = (long long)((a.SW + 3) / 4) * a.SH;  // a thread's quad index is an int
  if (quads >= (1ll << 31) - kAugThreads) return 0;
  const long long bps = (quads + kAugThreads - 1) / kAugThreads;
  return bps * std::max(a.count, 1) < (1ll << 31) ? (int)bps : 0;
}

hipError_t launch_aug_pair_u8(const AugArgs& a, hipStream_t s) {
  const int bps = aug_blocks_per_sample(a, false);
  if (!bps) return hipErrorInvalidValue;
  if (a.count == 0) return hipSuccess;
  hipLaunchKernelGGL(aug_pair_u8_kernel, dim3((unsigned)(a.count * bps)), dim3(kAugThreads), 0, s, a, bps);
  return hipGetLastError();
}

hipError_t launch_aug_synth_u8(const AugArgs& a, hipStream_t s) {
  const int bps = aug_blocks_per_sample(a, true);
  if (!bps) return hipErrorInvalidValue;
  if (a.count == 0) return hipSuccess;
  hipLaunchKernelGGL(aug_synth_u8_kernel, dim3((unsigned)(a.count * bps)), dim3(kAugThreads), 0, s, a, bps);
  return hipGetLastError();
}

}  // namespace llie
