// The trainer's per-epoch sample sheet (LowLightTrainer.generate_samples / _save_comparison, trainer.py:365-410): three rows of n
// images -- low-light, enhanced, normal-light -- as one uint8 picture.  It is torchvision's make_grid(cat([low, enhanced, normal]),
// nrow=n) with its defaults (padding 2, pad value 0) followed by save_image's quantisation, in one launch.  Bit-exact with
// comparison_grid_host in trainer.py, which is the definition (kernels.h (14) has the layout).
//
//   grid[r (H+2) + 2 + y][k (W+2) + 2 + x][c] = byte(src_r[k][c][y][x]),  src = (low, enhanced, normal);  every other byte is 0
//   byte(x):  v = (x + 1.0f) / 2.0f;  q = v * 255.0f + 0.5f;  q = min(max(q, 0), 255)  (NaN -> 0);  (uint8) trunc(q)
//
// A thread owns four consecutive x of one output row, so a wave writes 768 contiguous bytes.  Output rows are 3 (n (W+2) + 2)
// bytes long and start at arbitrary byte offsets: the 12 bytes go as three dwords when their address allows it and as bytes
// otherwise (store12, as tiles.hip).  A quad that lies inside one image reads each plane with one four-float access.
#include "common.h"
#include "kernels.h"

namespace llie {

constexpr int kGridThreads = 256;

__device__ __forceinline__ uint32_t grid_byte(float x) {
#pragma clang fp contract(off)
  const float v = (x + 1.0f) / 2.0f;
  const float q = v * 255.0f + 0.5f;
  return (uint32_t)truncf(fminf(fmaxf(q, 0.f), 255.f));  // fmaxf(NaN, 0) == 0
}

__global__ void __launch_bounds__(kGridThreads) comparison_grid_u8_kernel(const float* __restrict__ low, const float* __restrict__ enhanced,
                                                                          const float* __restrict__ normal, int n, int H, int W,
                                                                          uint8_t* __restrict__ grid) {
#pragma clang fp contract(off)
  const int GH = comparison_grid_rows(H), GW = comparison_grid_cols(n, W);
  const int qpr = (GW + 3) >> 2;
  const int64_t q = (int64_t)blockIdx.x * kGridThreads + threadIdx.x;
  if (q >= (int64_t)qpr * GH) return;
  const int Y = (int)(q / qpr), X0 = (int)(q - (int64_t)Y * qpr) * 4;
  uint32_t b[12];
#pragma unroll
  for (int i = 0; i < 12; ++i) b[i] = 0;
  const int yy = Y - kGridPad;
  const int r = yy >= 0 ? yy / (H + kGridPad) : 0;  // r <= 2 because GH = 3 (H + 2) + 2
  const int y = yy - r * (H + kGridPad);
  if (yy >= 0 && y < H) {  // not a padding line
    const float* src = r == 0 ? low : (r == 1 ? enhanced : normal);
    const size_t plane = (size_t)H * W;
    const int xx0 = X0 - kGridPad;
    const int k0 = xx0 >= 0 ? xx0 / (W + kGridPad) : 0;
    const int x0 = xx0 - k0 * (W + kGridPad);
    if (xx0 >= 0 && x0 + 3 < W) {  // the whole quad lies in image k0 (k0 < n because X0 + 3 < GW follows)
      const float* p = src + ((size_t)k0 * 3 * H + y) * W + x0;
#pragma unroll
      for (int c = 0; c < 3; ++c) {
        const f32x4 v = *reinterpret_cast<const f32x4u*>(p + c * plane);
#pragma unroll
        for (int i = 0; i < 4; ++i) b[i * 3 + c] = grid_byte(v[i]);
      }
    } else {
#pragma unroll
      for (int i = 0; i < 4; ++i) {
        const int xx = xx0 + i;
        if (xx < 0 || X0 + i >= GW) continue;
        const int k = xx / (W + kGridPad), x = xx - k * (W + kGridPad);
        if (x >= W || k >= n) continue;  // a padding column
        const float* p = src + ((size_t)k * 3 * H + y) * W + x;
#pragma unroll
        for (int c = 0; c < 3; ++c) b[i * 3 + c] = grid_byte(p[c * plane]);
      }
    }
  }
  uint8_t* dst = grid + ((size_t)Y * GW + X0) * 3;
  if (X0 + 3 < GW) {
    store12(dst, b);
  } else {
    for (int i = 0; i < (GW - X0) * 3; ++i) dst[i] = (uint8_t)b[i];
  }
}

hipError_t launch_comparison_grid_u8(const float* low, const float* enhanced, const float* normal, int n, int H, int W, uint8_t* grid,
                                     hipStream_t s) {
  if (!low || !enhanced || !normal || !grid || !comparison_grid_ok(n, H, W)) return hipErrorInvalidValue;
  const long long blocks = ((long long)((comparison_grid_cols(n, W) + 3) / 4) * comparison_grid_rows(H) + kGridThreads - 1) / kGridThreads;
  if (blocks >= (1ll << 31)) return hipErrorInvalidValue;
  hipLaunchKernelGGL(comparison_grid_u8_kernel, dim3((unsigned)blocks), dim3(kGridThreads), 0, s, low, enhanced, normal, n, H, W, grid);
  return hipGetLastError();
}

}  // namespace llie
