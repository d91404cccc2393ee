// Image quality of one batch of images against another: per image {mse, psnr, ssim} (kernels.h (13) has the definition).
// All arithmetic is float64 on the mapped values x = (v - lo) / (hi - lo) (bytes: x = byte / 255); metrics.py holds the NumPy twin.
//
//   image_metrics_tile:      one workgroup per (image, tile of kMetricTileH x kMetricTileW valid positions).  Per channel it
//                            stages the tile and its 10-pixel halo of both images in LDS as doubles, filters the five maps x, y,
//                            x^2, y^2, xy with the 11 taps along the rows, then along the columns, evaluates the SSIM formula per
//                            valid position and, after the three channels, adds the workgroup's values in a fixed tree.  Each
//                            input pixel is counted in the squared-error sum of the tile that owns it: the tile whose first
//                            kMetricTileH x kMetricTileW staged pixels hold it, the last tile of an axis owning its halo as well.
//                            It writes partial[image][tile] = {sum of ssim_map, sum of (x - y)^2}.
//   image_metrics_finalize:  one workgroup per image adds that image's partials (thread i takes tiles i, i + 256, ... in
//                            ascending order, then the same fixed tree) and writes {mse, psnr, ssim}.
//
// No atomics; the order of every sum depends on H and W alone, so an image's triple is the same bits alone or in a batch.
// LDS: 2 x 26 x 42 + 5 x 26 x 32 doubles = 50 752 bytes.
#include "common.h"
#include "kernels.h"

#include <cmath>

namespace llie {

constexpr int kMetricThreads = 256;
constexpr int kMetricHalo = kMetricTaps - 1;                 // 10
constexpr int kMetricInH = kMetricTileH + kMetricHalo;       // 26 staged rows
constexpr int kMetricInW = kMetricTileW + kMetricHalo;       // 42 staged columns
static_assert(kMetricThreads * 2 <= 5 * kMetricInH * kMetricTileW, "the reduction reuses the filtered maps' LDS");

struct MetricWindow { double g[kMetricTaps]; };

struct MetricArgs {
  const void* a; const void* b;
  int H, W, tiles_y, tiles_x;
  double lo, den;  // fp32 input: x = (v - lo) / den; bytes: x = byte / 255
  double* partial;
};

template <bool U8>
__device__ __forceinline__ double metric_value(const void* base, size_t img, int c, int y, int x, int H, int W, double lo, double den) {
  if constexpr (U8) {
    const uint8_t* p = static_cast<const uint8_t*>(base);
    return (double)p[((img * H + y) * W + x) * 3 + c] / 255.0;
  } else {
    const float* p = static_cast<const float*>(base);
    return ((double)p[((img * 3 + c) * H + y) * W + x] - lo) / den;
  }
}

// adds v over the workgroup in a fixed tree; the result is valid in thread 0.  `red` holds kMetricThreads doubles.
__device__ __forceinline__ double metric_block_sum(double v, double* red) {
  const int tid = threadIdx.x;
  red[tid] = v;
  __syncthreads();
#pragma unroll
  for (int s = kMetricThreads / 2; s > 0; s >>= 1) {
    if (tid < s) red[tid] = red[tid] + red[tid + s];
    __syncthreads();
  }
  return red[0];
}

template <bool U8>
__global__ void __launch_bounds__(kMetricThreads) image_metrics_tile_kernel(MetricArgs p, MetricWindow win) {
#pragma clang fp contract(off)
  __shared__ double sx[kMetricInH][kMetricInW];
  __shared__ double sy[kMetricInH][kMetricInW];
  __shared__ double hm[5][kMetricInH][kMetricTileW];

  const int tid = threadIdx.x;
  const int ntiles = p.tiles_y * p.tiles_x;
  const size_t img = blockIdx.x / ntiles;
  const int tile = blockIdx.x - (int)img * ntiles;
  const int tyi = tile / p.tiles_x, txi = tile - tyi * p.tiles_x;
  const int y0 = tyi * kMetricTileH, x0 = txi * kMetricTileW;
  const int H = p.H, W = p.W;
  const int vh = min(kMetricTileH, H - kMetricHalo - y0);  // valid positions of this tile (>= 1)
  const int vw = min(kMetricTileW, W - kMetricHalo - x0);
  const bool last_y = tyi == p.tiles_y - 1, last_x = txi == p.tiles_x - 1;

  double err = 0.0, ssim = 0.0;
  for (int c = 0; c < 3; ++c) {
    // stage rows [y0, y0 + vh + 10) x columns [x0, x0 + vw + 10): all inside the image; the rest of the arrays is zero
    for (int i = tid; i < kMetricInH * kMetricInW; i += kMetricThreads) {
      const int r = i / kMetricInW, q = i - r * kMetricInW;
      double x = 0.0, y = 0.0;
      if (r < vh + kMetricHalo && q < vw + kMetricHalo) {
        x = metric_value<U8>(p.a, img, c, y0 + r, x0 + q, H, W, p.lo, p.den);
        y = metric_value<U8>(p.b, img, c, y0 + r, x0 + q, H, W, p.lo, p.den);
        if ((r < kMetricTileH || last_y) && (q < kMetricTileW || last_x)) {
          const double d = x - y;
          err = err + d * d;
        }
      }
      sx[r][q] = x;
      sy[r][q] = y;
    }
    __syncthreads();
    // along the rows: taps in ascending order
    for (int i = tid; i < kMetricInH * kMetricTileW; i += kMetricThreads) {
      const int r = i / kMetricTileW, q = i - r * kMetricTileW;
      double mx = 0.0, my = 0.0, xx = 0.0, yy = 0.0, xy = 0.0;
#pragma unroll
      for (int k = 0; k < kMetricTaps; ++k) {
        const double g = win.g[k], x = sx[r][q + k], y = sy[r][q + k];
        mx = mx + g * x;
        my = my + g * y;
        xx = xx + g * (x * x);
        yy = yy + g * (y * y);
        xy = xy + g * (x * y);
      }
      hm[0][r][q] = mx; hm[1][r][q] = my; hm[2][r][q] = xx; hm[3][r][q] = yy; hm[4][r][q] = xy;
    }
    __syncthreads();
    // along the columns, then the SSIM formula
    for (int i = tid; i < kMetricTileH * kMetricTileW; i += kMetricThreads) {
      const int r = i / kMetricTileW, q = i - r * kMetricTileW;
      if (r >= vh || q >= vw) continue;
      double m[5];
#pragma unroll
      for (int j = 0; j < 5; ++j) {
        double s = 0.0;
#pragma unroll
        for (int k = 0; k < kMetricTaps; ++k) s = s + win.g[k] * hm[j][r + k][q];
        m[j] = s;
      }
      const double mx = m[0], my = m[1];
      const double vx = m[2] - mx * mx, vy = m[3] - my * my, cxy = m[4] - mx * my;
      const double num = (2.0 * mx * my + kMetricC1) * (2.0 * cxy + kMetricC2);
      const double den = (mx * mx + my * my + kMetricC1) * (vx + vy + kMetricC2);
      ssim = ssim + num / den;
    }
    __syncthreads();  // the next channel overwrites sx / sy / hm
  }
  double* red = &hm[0][0][0];
  const double ssim_tot = metric_block_sum(ssim, red);
  __syncthreads();
  const double err_tot = metric_block_sum(err, red);
  if (tid == 0) {
    double* dst = p.partial + ((size_t)img * ntiles + tile) * 2;
    dst[0] = ssim_tot;
    dst[1] = err_tot;
  }
}

__global__ void __launch_bounds__(kMetricThreads) image_metrics_finalize_kernel(const double* __restrict__ partial, int ntiles, int H, int W,
                                                                                double* __restrict__ out3) {
#pragma clang fp contract(off)
  __shared__ double red[kMetricThreads];
  const int tid = threadIdx.x;
  const size_t img = blockIdx.x;
  const double* src = partial + img * (size_t)ntiles * 2;
  double ssim = 0.0, err = 0.0;
  for (int t = tid; t < ntiles; t += kMetricThreads) {
    ssim = ssim + src[(size_t)t * 2];
    err = err + src[(size_t)t * 2 + 1];
  }
  const double ssim_tot = metric_block_sum(ssim, red);
  __syncthreads();
  const double err_tot = metric_block_sum(err, red);
  if (tid == 0) {
    const double mse = err_tot / (3.0 * (double)H * (double)W);
    double* dst = out3 + img * 3;
    dst[0] = mse;
    dst[1] = mse == 0.0 ? (double)INFINITY : -10.0 * log10(mse);
    dst[2] = ssim_tot / (3.0 * (double)(H - kMetricHalo) * (double)(W - kMetricHalo));
  }
}

static MetricWindow metric_window() {
  MetricWindow w;
  double sum = 0.0;
  for (int k = 0; k < kMetricTaps; ++k) {
    const double d = (double)(k - kMetricTaps / 2);
    w.g[k] = std::exp(-(d * d) / (2.0 * 1.5 * 1.5));
    sum += w.g[k];
  }
  for (int k = 0; k < kMetricTaps; ++k) w.g[k] /= sum;
  return w;
}

static hipError_t launch_image_metrics(bool u8, const void* a, const void* b, int batch, int H, int W, double lo, double hi, double* out3,
                                       double* partial, hipStream_t s) {
  if (!a || !b || !out3 || !partial || batch < 1 || H < kMetricTaps || W < kMetricTaps || !(lo != hi)) return hipErrorInvalidValue;
  const long long ntiles = image_metrics_tiles(H, W);
  if (ntiles * batch >= (1ll << 31)) return hipErrorInvalidValue;
  MetricArgs p{};
  p.a = a; p.b = b; p.H = H; p.W = W;
  p.tiles_y = (H - kMetricHalo + kMetricTileH - 1) / kMetricTileH;
  p.tiles_x = (W - kMetricHalo + kMetricTileW - 1) / kMetricTileW;
  p.lo = lo; p.den = hi - lo; p.partial = partial;
  const MetricWindow win = metric_window();
  const dim3 grid((unsigned)(ntiles * batch));
  if (u8) hipLaunchKernelGGL(image_metrics_tile_kernel<true>, grid, dim3(kMetricThreads), 0, s, p, win);
  else hipLaunchKernelGGL(image_metrics_tile_kernel<false>, grid, dim3(kMetricThreads), 0, s, p, win);
  hipError_t e = hipGetLastError();
  if (e != hipSuccess) return e;
  hipLaunchKernelGGL(image_metrics_finalize_kernel, dim3((unsigned)batch), dim3(kMetricThreads), 0, s, partial, (int)ntiles, H, W, out3);
  return hipGetLastError();
}

hipError_t launch_image_metrics_f32(const float* a, const float* b, int batch, int H, int W, float lo, float hi, double* out3, double* partial,
                                    hipStream_t s) {
  return launch_image_metrics(false, a, b, batch, H, W, (double)lo, (double)hi, out3, partial, s);
}

hipError_t launch_image_metrics_u8(const uint8_t* a, const uint8_t* b, int batch, int H, int W, double* out3, double* partial, hipStream_t s) {
  return launch_image_metrics(true, a, b, batch, H, W, 0.0, 255.0, out3, partial, s);
}

}  // namespace llie
