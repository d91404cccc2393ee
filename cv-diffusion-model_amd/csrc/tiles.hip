// Full-resolution images through a fixed-size denoiser: the byte work either side of `enhance` when an image is cut into
// overlapping SH x SW tiles (kernels.h (11) has the plan; each axis has its own tile side and overlap).  Bit-exact with the NumPy twins in tiling.py.
//
//   tile_gather_u8:   tile[t][c][y][x] = float(img[min(oy + y, H-1)][min(ox + x, W-1)][c]) / 127.5f - 1.0f
//   tile_gather_f32:  out[k][j][c][y][x] = canvas[k][c][oy + y][ox + x]           (the noise every tile of an image shares)
//   tile_blend_u8:    per pixel and channel, over the covering tiles in ascending tile number:
//                       g = wy[Y - oy] * wx[X - ox];  num = num + val * g;  den = den + g     (separate fp32 operations)
//                     out = (uint8) trunc(min(max((num / den + 1.0f) * 127.5f, 0), 255)),  wy[k] = min(k + 1, SH - k, vy) / vy  (1 if vy == 0), wx likewise
//   tile_sync_step:   one LCM step of the latent canvas [3][Hc][Wc] (Hc / Wc = max(H / W, SH / SW)) every tile of an image shares: per
//                     canvas pixel and channel, e = the eps of the one covering tile, or num / den of tile_blend_u8's sums over
//                     eps when several cover it; then lcm_step_kernel's arithmetic (small.hip; LCM or DDIM) on (e, canvas, noise), written
//                     back to the canvas, and on request tile_blend_u8's bytes of the result for y < H, x < W
//
//
// Whole frames at their own size (llie_enhance_hw), Hp / Wp = frame_pad(H) / frame_pad(W):
//   frame_load_u8:    out[c][y][x] = float(img[min(y, H-1)][min(x, W-1)][c]) / 127.5f - 1.0f,  0 <= y < Hp, 0 <= x < Wp
//   frame_store_u8:   img[y][x][c] = (uint8) trunc(min(max((in[c][y][x] + 1.0f) * 127.5f, 0), 255)),  0 <= y < H, 0 <= x < W
//
// Origins are computed in the kernels from each axis's (L, S, v): nothing is uploaded per call.  A thread owns four consecutive x, so a
// wave moves contiguous runs: 768 bytes of pixels and 1 KB of each fp32 plane.  The fp32 rows start at arbitrary origins, so
// their four-float accesses are only 4-byte aligned (global_load/store_dwordx4 need no more than that); the 12 pixel bytes go
// as three dwords when their address allows it and as bytes otherwise.  The blend is a gather: no atomics, fixed order.
#include "common.h"
#include "kernels.h"

namespace llie {

constexpr int kTileThreads = 256;

__device__ __forceinline__ void tile_origin_of(const TilePlan& p, int t, int ny, int nx, int& oy, int& ox) {
  const int iy = t / nx, ix = t - iy * nx;
  oy = tile_axis_origin(iy, p.H, p.SH, ny);
  ox = tile_axis_origin(ix, p.W, p.SW, nx);
}

// grid.x = count * bpt (bpt workgroups cover the SH * ceil(SW/4) quads of a tile)
__global__ void __launch_bounds__(kTileThreads) tile_gather_u8_kernel(const uint8_t* __restrict__ img, TilePlan p, int ny, int nx, int bpt,
                                                                      float* __restrict__ tiles) {
#pragma clang fp contract(off)
  const int SH = p.SH, SW = p.SW, qpr = (SW + 3) >> 2;
  const int j = blockIdx.x / bpt;
  const int q = (blockIdx.x - j * bpt) * kTileThreads + threadIdx.x;
  if (q >= qpr * SH) return;
  const int y = q / qpr, x0 = (q - y * qpr) * 4;
  int oy, ox;
  tile_origin_of(p, p.first + j, ny, nx, oy, ox);
  const uint8_t* src = img + (size_t)min(oy + y, p.H - 1) * p.W * 3;
  const int X = ox + x0;
  uint32_t b[12];
  if (X + 3 < p.W) {
    load12(src + (size_t)X * 3, b);
  } else {  // the image ends inside this quad (only where it is narrower than a tile): replicate its last column
#pragma unroll
    for (int k = 0; k < 4; ++k) {
      const uint8_t* px = src + (size_t)min(X + k, p.W - 1) * 3;
#pragma unroll
      for (int c = 0; c < 3; ++c) b[k * 3 + c] = px[c];
    }
  }
  float* dst = tiles + (((size_t)j * 3) * SH + y) * SW + x0;
#pragma unroll
  for (int c = 0; c < 3; ++c, dst += (size_t)SH * SW) {
    f32x4 u;
#pragma unroll
    for (int k = 0; k < 4; ++k) u[k] = (float)b[k * 3 + c] / 127.5f - 1.0f;
    if (x0 + 3 < SW) {
      *reinterpret_cast<f32x4u*>(dst) = u;
    } else {
#pragma unroll
      for (int k = 0; k < 4; ++k)
        if (x0 + k < SW) dst[k] = u[k];
    }
  }
}

// grid.x as above, grid.y = plane of the canvas (k * 3 + c)
__global__ void __launch_bounds__(kTileThreads) tile_gather_f32_kernel(const float* __restrict__ canvas, TilePlan p, int ny, int nx, int bpt,
                                                                       float* __restrict__ out) {
  const int SH = p.SH, SW = p.SW, qpr = (SW + 3) >> 2;
  const int j = blockIdx.x / bpt;
  const int q = (blockIdx.x - j * bpt) * kTileThreads + threadIdx.x;
  if (q >= qpr * SH) return;
  const int y = q / qpr, x0 = (q - y * qpr) * 4;
  int oy, ox;
  tile_origin_of(p, p.first + j, ny, nx, oy, ox);
  const int Hc = max(p.H, SH), Wc = max(p.W, SW);  // oy + SH <= Hc and ox + SW <= Wc by construction of the plan
  const int plane = blockIdx.y, k = plane / 3, c = plane - k * 3;
  const float* src = canvas + ((size_t)plane * Hc + oy + y) * Wc + ox + x0;
  float* dst = out + ((((size_t)k * p.count + j) * 3 + c) * SH + y) * SW + x0;
  if (x0 + 3 < SW) {
    *reinterpret_cast<f32x4u*>(dst) = *reinterpret_cast<const f32x4u*>(src);
  } else {
    for (int i = 0; x0 + i < SW; ++i) dst[i] = src[i];
  }
}

__device__ __forceinline__ float tile_window(int k, int S, int v) {
  return v == 0 ? 1.0f : (float)min(min(k + 1, S - k), v) / (float)v;
}
// the tiles of one axis that cover position P: [lo, hi]
__device__ __forceinline__ void tile_cover(int P, int L, int S, int n, int& lo, int& hi) {
  if (n <= 1) { lo = hi = 0; return; }
  const int D = L - S, m = n - 1;
  hi = min(m, ((P + 1) * m - 1) / D);  // the last i with floor(i D / m) <= P
  lo = hi;
  while (lo > 0 && tile_axis_origin(lo - 1, L, S, n) + S > P) --lo;
}

// one thread per four consecutive output pixels of a row
__global__ void __launch_bounds__(kTileThreads) tile_blend_u8_kernel(const float* __restrict__ tiles, TilePlan p, int ny, int nx,
                                                                     uint8_t* __restrict__ img) {
#pragma clang fp contract(off)
  const int SH = p.SH, SW = p.SW, vy = p.vy, vx = p.vx, H = p.H, W = p.W;
  const int qpr = (W + 3) >> 2;
  const int64_t q = (int64_t)blockIdx.x * kTileThreads + threadIdx.x;
  if (q >= (int64_t)qpr * H) return;
  const int Y = (int)(q / qpr), X0 = (int)(q - (int64_t)Y * qpr) * 4;
  const int Xl = min(X0 + 3, W - 1);
  int ylo, yhi, xlo, xhi, unused;
  tile_cover(Y, H, SH, ny, ylo, yhi);
  tile_cover(X0, W, SW, nx, xlo, unused);
  tile_cover(Xl, W, SW, nx, unused, xhi);
  float num[4][3], den[4];
#pragma unroll
  for (int k = 0; k < 4; ++k) den[k] = num[k][0] = num[k][1] = num[k][2] = 0.0f;
  for (int iy = ylo; iy <= yhi; ++iy) {
    const int ty = Y - tile_axis_origin(iy, H, SH, ny);
    const float wy = tile_window(ty, SH, vy);
    for (int ix = xlo; ix <= xhi; ++ix) {  // ascending tile number iy * nx + ix
      const int tx = X0 - tile_axis_origin(ix, W, SW, nx);
      const float* src = tiles + (((size_t)(iy * nx + ix) * 3) * SH + ty) * SW;
      src += tx;  // dereferenced only where 0 <= tx + k < SW
      if (tx >= 0 && tx + 3 < SW && X0 + 3 < W) {
        f32x4 val[3];
#pragma unroll
        for (int c = 0; c < 3; ++c) val[c] = *reinterpret_cast<const f32x4u*>(src + (size_t)c * SH * SW);
#pragma unroll
        for (int k = 0; k < 4; ++k) {
          const float g = wy * tile_window(tx + k, SW, vx);
#pragma unroll
          for (int c = 0; c < 3; ++c) num[k][c] = num[k][c] + val[c][k] * g;
          den[k] = den[k] + g;
        }
      } else {
#pragma unroll
        for (int k = 0; k < 4; ++k) {
          if (tx + k < 0 || tx + k >= SW || X0 + k >= W) continue;
          const float g = wy * tile_window(tx + k, SW, vx);
#pragma unroll
          for (int c = 0; c < 3; ++c) num[k][c] = num[k][c] + src[(size_t)c * SH * SW + k] * g;
          den[k] = den[k] + g;
        }
      }
    }
  }
  uint32_t b[12];
#pragma unroll
  for (int k = 0; k < 4; ++k)
#pragma unroll
    for (int c = 0; c < 3; ++c) {
      const float r = num[k][c] / den[k];  // pixels past W have den == 0 and are not stored
      b[k * 3 + c] = (uint32_t)truncf(fminf(fmaxf((r + 1.0f) * 127.5f, 0.f), 255.f));
    }
  uint8_t* dst = img + ((size_t)Y * W + X0) * 3;
  if (X0 + 3 < W) {
    store12(dst, b);
  } else {
    for (int i = 0; i < (W - X0) * 3; ++i) dst[i] = (uint8_t)b[i];
  }
}

// One thread per four consecutive x of a canvas row, all three channels.  The plan of (Hc, Wc) is the plan of (H, W) and its
// tiles cover the canvas, so every pixel has at least one tile.  A thread reads its own four canvas values of a plane before it
// writes them and no other thread touches them: canvas_out may be canvas_in.  img (or NULL) takes the bytes of the new canvas.
__global__ void __launch_bounds__(kTileThreads) tile_sync_step_kernel(const float* __restrict__ eps, TilePlan p, int ny, int nx,
                                                                      const float* canvas_in, const float* __restrict__ noise, StepCoef sc,
                                                                      float* canvas_out, uint8_t* __restrict__ img) {
#pragma clang fp contract(off)
  const int SH = p.SH, SW = p.SW, vy = p.vy, vx = p.vx;
  const int Hc = max(p.H, SH), Wc = max(p.W, SW);
  const int qpr = (Wc + 3) >> 2;
  const int64_t q = (int64_t)blockIdx.x * kTileThreads + threadIdx.x;
  if (q >= (int64_t)qpr * Hc) return;
  const int Y = (int)(q / qpr), X0 = (int)(q - (int64_t)Y * qpr) * 4;
  const int Xl = min(X0 + 3, Wc - 1);
  int ylo, yhi, xlo, xhi, unused;
  tile_cover(Y, Hc, SH, ny, ylo, yhi);
  tile_cover(X0, Wc, SW, nx, xlo, unused);
  tile_cover(Xl, Wc, SW, nx, unused, xhi);
  float num[4][3], den[4], one[4][3];  // one: the eps of the covering tile seen last, used where it is the only one
  int cover[4];
#pragma unroll
  for (int k = 0; k < 4; ++k) {
    den[k] = num[k][0] = num[k][1] = num[k][2] = one[k][0] = one[k][1] = one[k][2] = 0.0f;
    cover[k] = 0;
  }
  for (int iy = ylo; iy <= yhi; ++iy) {
    const int ty = Y - tile_axis_origin(iy, Hc, SH, ny);
    const float wy = tile_window(ty, SH, vy);
    for (int ix = xlo; ix <= xhi; ++ix) {  // ascending tile number iy * nx + ix
      const int tx = X0 - tile_axis_origin(ix, Wc, SW, nx);
      const float* src = eps + (((size_t)(iy * nx + ix) * 3) * SH + ty) * SW;
      src += tx;  // dereferenced only where 0 <= tx + k < SW
      if (tx >= 0 && tx + 3 < SW) {  // X0 + 3 <= ox + SW - 1 < Wc
        f32x4 val[3];
#pragma unroll
        for (int c = 0; c < 3; ++c) val[c] = *reinterpret_cast<const f32x4u*>(src + (size_t)c * SH * SW);
#pragma unroll
        for (int k = 0; k < 4; ++k) {
          const float g = wy * tile_window(tx + k, SW, vx);
#pragma unroll
          for (int c = 0; c < 3; ++c) {
            num[k][c] = num[k][c] + val[c][k] * g;
            one[k][c] = val[c][k];
          }
          den[k] = den[k] + g;
          ++cover[k];
        }
      } else {
#pragma unroll
        for (int k = 0; k < 4; ++k) {
          if (tx + k < 0 || tx + k >= SW) continue;  // tx + k < SW keeps X0 + k < Wc
          const float g = wy * tile_window(tx + k, SW, vx);
#pragma unroll
          for (int c = 0; c < 3; ++c) {
            const float e = src[(size_t)c * SH * SW + k];
            num[k][c] = num[k][c] + e * g;
            one[k][c] = e;
          }
          den[k] = den[k] + g;
          ++cover[k];
        }
      }
    }
  }
  const bool whole = X0 + 3 < Wc;
  const size_t plane = (size_t)Hc * Wc, at = (size_t)Y * Wc + X0;
  uint32_t b[12];
#pragma unroll
  for (int c = 0; c < 3; ++c) {
    const float* xs = canvas_in + c * plane + at;
    const bool draw = !sc.is_last && !sc.sampler;  // the DDIM step (sampler 1) re-noises with the predicted noise: nothing to read
    const float* ns = draw ? noise + c * plane + at : xs;
    f32x4 xv = {0.f, 0.f, 0.f, 0.f}, nz = {0.f, 0.f, 0.f, 0.f}, pv;
    if (whole) {
      xv = *reinterpret_cast<const f32x4u*>(xs);
      if (draw) nz = *reinterpret_cast<const f32x4u*>(ns);
    } else {
      for (int k = 0; X0 + k < Wc; ++k) {
        xv[k] = xs[k];
        if (draw) nz[k] = ns[k];
      }
    }
#pragma unroll
    for (int k = 0; k < 4; ++k) {  // pixels past Wc have den == 0 and are not stored
      const float e = cover[k] == 1 ? one[k][c] : num[k][c] / den[k];
      float x0;
      if (sc.vpred) x0 = sc.sa * xv[k] - sc.sb * e;
      else x0 = (xv[k] - sc.sb * e) / sc.sa;
      if (sc.clamp_x0) x0 = fminf(fmaxf(x0, -1.f), 1.f);
      float pr = x0;
      if (!sc.is_last) {
        float z = nz[k];
        if (sc.sampler) z = sc.vpred ? sc.sa * e + sc.sb * xv[k] : e;
        pr = sc.sap * x0 + sc.sbp * z;
      }
      pv[k] = pr;
      b[k * 3 + c] = (uint32_t)truncf(fminf(fmaxf((pr + 1.0f) * 127.5f, 0.f), 255.f));
    }
    float* dst = canvas_out + c * plane + at;
    if (whole) {
      *reinterpret_cast<f32x4u*>(dst) = pv;
    } else {
      for (int k = 0; X0 + k < Wc; ++k) dst[k] = pv[k];
    }
  }
  if (img && Y < p.H && X0 < p.W) {
    uint8_t* dst = img + ((size_t)Y * p.W + X0) * 3;
    if (X0 + 3 < p.W) {
      store12(dst, b);
    } else {
      for (int i = 0; i < (p.W - X0) * 3; ++i) dst[i] = (uint8_t)b[i];
    }
  }
}

// one thread per four consecutive x of a padded row (Wp is a multiple of 8, so every quad is whole and 16-byte aligned in its plane)
__global__ void __launch_bounds__(kTileThreads) frame_load_u8_kernel(const uint8_t* __restrict__ img, int H, int W, int Hp, int Wp,
                                                                     float* __restrict__ out) {
#pragma clang fp contract(off)
  const int qpr = Wp >> 2;
  const int64_t q = (int64_t)blockIdx.x * kTileThreads + threadIdx.x;
  if (q >= (int64_t)qpr * Hp) return;
  const int y = (int)(q / qpr), x0 = (int)(q - (int64_t)y * qpr) * 4;
  const uint8_t* src = img + (size_t)min(y, H - 1) * W * 3;
  uint32_t b[12];
  if (x0 + 3 < W) {
    load12(src + (size_t)x0 * 3, b);
  } else {  // the frame ends inside or before this quad: replicate its last column
#pragma unroll
    for (int k = 0; k < 4; ++k) {
      const uint8_t* px = src + (size_t)min(x0 + k, W - 1) * 3;
#pragma unroll
      for (int c = 0; c < 3; ++c) b[k * 3 + c] = px[c];
    }
  }
  float* dst = out + (size_t)y * Wp + x0;
#pragma unroll
  for (int c = 0; c < 3; ++c, dst += (size_t)Hp * Wp) {
    f32x4 u;
#pragma unroll
    for (int k = 0; k < 4; ++k) u[k] = (float)b[k * 3 + c] / 127.5f - 1.0f;
    *reinterpret_cast<f32x4u*>(dst) = u;
  }
}

// one thread per four consecutive output pixels of a row; the four floats it reads lie inside the padded row (x0 + 3 < Wp)
__global__ void __launch_bounds__(kTileThreads) frame_store_u8_kernel(const float* __restrict__ in, int H, int W, int Hp, int Wp,
                                                                      uint8_t* __restrict__ img) {
#pragma clang fp contract(off)
  const int qpr = (W + 3) >> 2;
  const int64_t q = (int64_t)blockIdx.x * kTileThreads + threadIdx.x;
  if (q >= (int64_t)qpr * H) return;
  const int y = (int)(q / qpr), x0 = (int)(q - (int64_t)y * qpr) * 4;
  const float* src = in + (size_t)y * Wp + x0;
  uint32_t b[12];
#pragma unroll
  for (int c = 0; c < 3; ++c, src += (size_t)Hp * Wp) {
    const f32x4 val = *reinterpret_cast<const f32x4u*>(src);
#pragma unroll
    for (int k = 0; k < 4; ++k) b[k * 3 + c] = (uint32_t)truncf(fminf(fmaxf((val[k] + 1.0f) * 127.5f, 0.f), 255.f));
  }
  uint8_t* dst = img + ((size_t)y * W + x0) * 3;
  if (x0 + 3 < W) {
    store12(dst, b);
  } else {
    for (int i = 0; i < (W - x0) * 3; ++i) dst[i] = (uint8_t)b[i];
  }
}

// workgroups per tile; 0 when the quads of one tile do not fit the kernels' 32-bit quad index
static int tile_blocks(const TilePlan& p) {
  const long long n = ((long long)((p.SW + 3) / 4) * p.SH + kTileThreads - 1) / kTileThreads;
  return n * kTileThreads < (1ll << 31) ? (int)n : 0;
}
static bool chunk_ok(const TilePlan& p, int ny, int nx, int bpt) {
  return bpt > 0 && p.first >= 0 && p.count > 0 && (long long)p.first + p.count <= (long long)ny * nx &&
         (long long)p.count * bpt < (1ll << 31);
}

hipError_t launch_tile_gather_u8(const uint8_t* img, const TilePlan& p, float* tiles, hipStream_t s) {
  if (!tile_plan_ok(p.H, p.W, p.SH, p.SW, p.vy, p.vx)) return hipErrorInvalidValue;
  const int ny = tile_axis_count(p.H, p.SH, p.vy), nx = tile_axis_count(p.W, p.SW, p.vx);
  const int bpt = tile_blocks(p);
  if (!chunk_ok(p, ny, nx, bpt)) return hipErrorInvalidValue;
  hipLaunchKernelGGL(tile_gather_u8_kernel, dim3((unsigned)(p.count * bpt)), dim3(kTileThreads), 0, s, img, p, ny, nx, bpt, tiles);
  return hipGetLastError();
}

hipError_t launch_tile_gather_f32(const float* canvas, int planes, const TilePlan& p, float* out, hipStream_t s) {
  if (!tile_plan_ok(p.H, p.W, p.SH, p.SW, p.vy, p.vx) || planes <= 0 || planes % 3 || planes > 65535) return hipErrorInvalidValue;
  const int ny = tile_axis_count(p.H, p.SH, p.vy), nx = tile_axis_count(p.W, p.SW, p.vx);
  const int bpt = tile_blocks(p);
  if (!chunk_ok(p, ny, nx, bpt)) return hipErrorInvalidValue;
  hipLaunchKernelGGL(tile_gather_f32_kernel, dim3((unsigned)(p.count * bpt), (unsigned)planes), dim3(kTileThreads), 0, s, canvas, p, ny, nx,
                     bpt, out);
  return hipGetLastError();
}

hipError_t launch_tile_blend_u8(const float* tiles, const TilePlan& p, uint8_t* img, hipStream_t s) {
  if (!tile_plan_ok(p.H, p.W, p.SH, p.SW, p.vy, p.vx)) return hipErrorInvalidValue;
  const int ny = tile_axis_count(p.H, p.SH, p.vy), nx = tile_axis_count(p.W, p.SW, p.vx);
  const long long blocks = ((long long)((p.W + 3) / 4) * p.H + kTileThreads - 1) / kTileThreads;
  if (blocks >= (1ll << 31)) return hipErrorInvalidValue;
  hipLaunchKernelGGL(tile_blend_u8_kernel, dim3((unsigned)blocks), dim3(kTileThreads), 0, s, tiles, p, ny, nx, img);
  return hipGetLastError();
}

hipError_t launch_tile_sync_step(const float* eps, const TilePlan& p, const float* canvas_in, const float* noise, const StepCoef& c,
                                 float* canvas_out, uint8_t* img, hipStream_t s) {
  if (!tile_plan_ok(p.H, p.W, p.SH, p.SW, p.vy, p.vx) || (!c.is_last && !c.sampler && !noise) || (c.sampler && c.clamp_x0)) return hipErrorInvalidValue;
  const int Hc = p.H > p.SH ? p.H : p.SH, Wc = p.W > p.SW ? p.W : p.SW;
  if (!tile_plan_ok(Hc, Wc, p.SH, p.SW, p.vy, p.vx)) return hipErrorInvalidValue;
  const int ny = tile_axis_count(p.H, p.SH, p.vy), nx = tile_axis_count(p.W, p.SW, p.vx);
  const long long blocks = ((long long)((Wc + 3) / 4) * Hc + kTileThreads - 1) / kTileThreads;
  if (blocks >= (1ll << 31)) return hipErrorInvalidValue;
  hipLaunchKernelGGL(tile_sync_step_kernel, dim3((unsigned)blocks), dim3(kTileThreads), 0, s, eps, p, ny, nx, canvas_in, noise, c, canvas_out,
                     img);
  return hipGetLastError();
}

// rows x quads of 256 threads; false when the frame is empty or the grid would not fit
static bool frame_blocks(int H, int W, long long rows, long long quads, unsigned& blocks) {
  if (H <= 0 || W <= 0 || H > (1 << 24) || W > (1 << 24)) return false;
  const long long n = (rows * quads + kTileThreads - 1) / kTileThreads;
  if (n >= (1ll << 31)) return false;
  blocks = (unsigned)n;
  return true;
}

hipError_t launch_frame_load_u8(const uint8_t* img, int H, int W, float* out, hipStream_t s) {
  unsigned blocks;
  if (!frame_blocks(H, W, frame_pad(H), frame_pad(W) / 4, blocks)) return hipErrorInvalidValue;
  hipLaunchKernelGGL(frame_load_u8_kernel, dim3(blocks), dim3(kTileThreads), 0, s, img, H, W, frame_pad(H), frame_pad(W), out);
  return hipGetLastError();
}

hipError_t launch_frame_store_u8(const float* in, int H, int W, uint8_t* img, hipStream_t s) {
  unsigned blocks;
  if (!frame_blocks(H, W, H, (W + 3) / 4, blocks)) return hipErrorInvalidValue;
  hipLaunchKernelGGL(frame_store_u8_kernel, dim3(blocks), dim3(kTileThreads), 0, s, in, H, W, frame_pad(H), frame_pad(W), img);
  return hipGetLastError();
}

}  // namespace llie
