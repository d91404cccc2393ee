// The 3 -> C0 head and C0 -> 3 tail convolutions of the denoiser (gfx950); the other 3x3 convs are in conv.hip and upconv.hip.
//   init_conv   (efficient_unet.py:420,553)  Cin=6 -> C0, reads the two fp32 NCHW halves of
//               torch.cat([latents, low_light], 1) (low_light_diffusion.py:222) directly: the concat is virtual.
//   final head  (efficient_unet.py:528-530,600-602)  GroupNorm affine + SiLU fused into the tile load,
//               C0 -> 3, writes the fp32 NCHW noise prediction.
#include <type_traits>

#include "common.h"
#include "kernels.h"

namespace llie {

// =============================================================================================
// init_conv: one thread = one output pixel x 32 output channels (K = 54 is too small for MFMA tiles
// to pay; weights are wave-uniform and come through the scalar cache).
// Weight layout here: [k = ci*9 + tap][Cout] fp32 (repacked at load).
template <typename T>
__global__ void __launch_bounds__(256) init_conv_kernel(const InitConvArgs a) {
  constexpr int VEC = Elem<T>::VEC;
  constexpr int MAXC = 8;
  __shared__ float patch[MAXC][18][19];
  __shared__ float red[4][2][32];
  const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
  const int tiles_x = (a.W + 15) / 16;  // edge tiles may be partly empty (image sizes that are not a multiple of 16)
  const int tx = blockIdx.x % tiles_x, ty = blockIdx.x / tiles_x, b = blockIdx.y;
  const int x0 = tx * 16, y0 = ty * 16;
  const int Cin = a.c0 + a.c1;
  const size_t plane = (size_t)a.H * a.W;
  for (int i = tid; i < Cin * 18 * 18; i += 256) {
    const int ci = i / 324, r = i % 324;
    const int py = r / 18, px = r % 18;
    const int gy = y0 + py - 1, gx = x0 + px - 1;
    float v = 0.f;
    if (gy >= 0 && gy < a.H && gx >= 0 && gx < a.W) {
      const float* src = ci < a.c0 ? a.x0 + ((size_t)b * a.c0 + ci) * plane : a.x1 + ((size_t)b * a.c1 + (ci - a.c0)) * plane;
      v = src[(size_t)gy * a.W + gx];
    }
    patch[ci][py][px] = v;
  }
  wg_barrier();
  const int py = tid >> 4, px = tid & 15;
  const bool ok = y0 + py < a.H && x0 + px < a.W;
  const float* __restrict__ w = a.w;
  T* out = reinterpret_cast<T*>(a.out) + (((size_t)b * a.H + y0 + py) * a.W + x0 + px) * a.Cout;
  const int ntiles = tiles_x * ((a.H + 15) / 16);
  for (int oc0 = 0; oc0 < a.Cout; oc0 += 32) {
    float acc[32];
#pragma unroll
    for (int o = 0; o < 32; ++o) acc[o] = a.bias[oc0 + o];
    for (int ci = 0; ci < Cin; ++ci) {
#pragma unroll
      for (int tap = 0; tap < 9; ++tap) {
        const float v = patch[ci][py + tap / 3][px + tap % 3];
        const float* wr = w + (size_t)(ci * 9 + tap) * a.Cout + oc0;
#pragma unroll
        for (int o = 0; o < 32; ++o) acc[o] += wr[o] * v;
      }
    }
    float q[32];
#pragma unroll
    for (int o = 0; o < 32; o += VEC) {
      typename Elem<T>::vec_t ov = f32_to_vec<T>(acc + o);
      if (ok) st_vec<T>(out + oc0 + o, ov);
#pragma unroll
      for (int e = 0; e < VEC; ++e) q[o + e] = ok ? (float)ov[e] : 0.f;
    }
    if (a.stats) {
#pragma unroll
      for (int o = 0; o < 32; ++o) {
        const float s1 = wave_sum(q[o]), s2 = wave_sum(q[o] * q[o]);
        if (lane == 0) {
          red[wave][0][o] = s1;
          red[wave][1][o] = s2;
        }
      }
      wg_barrier();
      if (tid < 64) {
        const int which = tid >> 5, o = tid & 31;
        const float t = red[0][which][o] + red[1][which][o] + red[2][which][o] + red[3][which][o];
        a.stats[((size_t)(b * ntiles + blockIdx.x) * 2 + which) * a.Cout + oc0 + o] = t;
      }
      wg_barrier();
    }
  }
}
// ---------------------------------------------------------------------------------------------
// init_conv on MFMA (2-byte T): im2col without a gather.  The 18x18 halo patch is staged in LDS as
// [y][x][8 channels] (16 B per pixel; channels >= Cin are zero), and K is ordered (tap, channel8), so
// one ds_read_b128 per k-step IS the lane's A fragment: k-step s covers taps 2s (lane half 0) and 2s+1
// (lane half 1); tap 9 does not exist and is fed zeros.  5 k-steps (K = 80 >= 72).  Weights come
// pre-packed as [s][half][Cout][8] T.  One wave computes two 32-pixel x 32-channel tiles per 32 output
// channels; its fp32 tile goes through a wave-private LDS patch so stores are full 64-byte pixel rows.
template <typename T>
__global__ void __launch_bounds__(256) init_conv_mfma_kernel(const InitConvArgs a) {
  typedef typename Elem<T>::vec_t vec_t;
  constexpr int TH = 8, TW = 32, PH = TH + 2, PWD = TW + 3;  // 8 x 32 output tile: 136-byte runs of the fp32 input planes
  __shared__ vec_t patch[PH * PWD + 1];   // +1: an all-zero slot for the missing 10th tap
  __shared__ float ctile[4][32 * 33];
  __shared__ float red[4][2][32];
  const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
  const int tiles_x = (a.W + TW - 1) / TW;  // the last tile of a row may be partly empty (W % 32 != 0)
  // XCD-aware tile order (workgroups are dealt round-robin to the 8 XCDs, one L2 each): an XCD gets a run of consecutive tiles,
  // so horizontal neighbours share the lines their halo columns straddle in ONE L2.  With neighbours on different XCDs every
  // 136-byte patch row cost three 128-byte lines per XCD: 275 MB of HBM traffic per launch against 184.5 MB algorithmic.
  const int tile_id = xcd_tile_order(blockIdx.x, gridDim.x);
  const int tx = tile_id % tiles_x, ty = tile_id / tiles_x, b = blockIdx.y;
  const int x0 = tx * TW, y0 = ty * TH;
  const int Cin = a.c0 + a.c1;
  const size_t plane = (size_t)a.H * a.W;
  // first block's weight fragments and bias up front: their (L2) latency runs under the patch staging
  vec_t wf0[5];
  {
    const T* wp0 = reinterpret_cast<const T*>(a.wp);
#pragma unroll
    for (int s = 0; s < 5; ++s) wf0[s] = ld_vec<T>(wp0 + ((size_t)(s * 2 + (lane >> 5)) * a.Cout + (lane & 31)) * 8);
  }
  const float bias0 = a.bias[lane & 31];
  for (int i = tid; i < PH * PWD + 1; i += 256) {
    const int py = i / PWD, px = i % PWD;
    const int gy = y0 + py - 1, gx = x0 + px - 1;
    vec_t v;
#pragma unroll
    for (int e = 0; e < 8; ++e) v[e] = (T)0.f;
    if (i < PH * PWD && px < TW + 2 && gy >= 0 && gy < a.H && gx >= 0 && gx < a.W) {
      for (int ci = 0; ci < Cin; ++ci) {
        const float* src = ci < a.c0 ? a.x0 + ((size_t)b * a.c0 + ci) * plane : a.x1 + ((size_t)b * a.c1 + (ci - a.c0)) * plane;
        v[ci] = (T)src[(size_t)gy * a.W + gx];
      }
    }
    patch[i] = v;
  }
  wg_barrier();
  const int r = lane & 31, h = lane >> 5;
  const T* wp = reinterpret_cast<const T*>(a.wp);
  T* out = reinterpret_cast<T*>(a.out) + (size_t)b * a.H * a.W * a.Cout;
  const int ntiles = tiles_x * (a.H / TH);
  float* ct = ctile[wave];
  for (int oc0 = 0; oc0 < a.Cout; oc0 += 32) {
    vec_t wf[5];
#pragma unroll
    for (int s = 0; s < 5; ++s) wf[s] = oc0 ? ld_vec<T>(wp + ((size_t)(s * 2 + h) * a.Cout + oc0 + r) * 8) : wf0[s];
    const float bias = oc0 ? a.bias[oc0 + r] : bias0;
    float s1 = 0.f, s2 = 0.f;
#pragma unroll
    for (int t = 0; t < 2; ++t) {
      const int g = wave * 2 + t;                 // 32-pixel group: row g of the 8 x 32 tile
      const int py = g, px = r;
      f32x16 acc;
#pragma unroll
      for (int q = 0; q < 16; ++q) acc[q] = 0.f;
#pragma unroll
      for (int s = 0; s < 5; ++s) {
        const int tap = 2 * s + h;
        const int idx = tap < 9 ? (py + tap / 3) * PWD + px + tap % 3 : PH * PWD;
        const vec_t av = patch[idx];
        if constexpr (std::is_same<T, half_t>::value) acc = __builtin_amdgcn_mfma_f32_32x32x16_f16(av, wf[s], acc, 0, 0, 0);
        else acc = __builtin_amdgcn_mfma_f32_32x32x16_bf16(av, wf[s], acc, 0, 0, 0);
      }
      // D[pixel (rows in registers)][channel = r]: + bias, round, stats, then transpose through LDS
#pragma unroll
      for (int q = 0; q < 16; ++q) {
        float v = (float)(T)(acc[q] + bias);
        if (x0 + mfma_row(q, lane) >= a.W) v = 0.f;  // pixel past the image (never stored either)
        s1 += v;
        s2 += v * v;
        ct[mfma_row(q, lane) * 33 + r] = v;
      }
      // wave-private tile: no block barrier needed, only LDS ordering within the wave
      __builtin_amdgcn_s_waitcnt(0xc07f);  // lgkmcnt(0)
      __builtin_amdgcn_wave_barrier();
      {
        const int p = lane >> 1, half = lane & 1;        // pixel in group, 16-channel half
        float f[16];
#pragma unroll
        for (int e = 0; e < 16; ++e) f[e] = ct[p * 33 + half * 16 + e];
        const int oy = y0 + g, ox = x0 + p;
        T* dst = out + ((size_t)oy * a.W + ox) * a.Cout + oc0 + half * 16;
        if (ox < a.W) {
          st_vec<T>(dst, f32_to_vec<T>(f));
          st_vec<T>(dst + 8, f32_to_vec<T>(f + 8));
        }
      }
      __builtin_amdgcn_wave_barrier();
    }
    if (a.stats) {
      s1 += __shfl_xor(s1, 32, 64);
      s2 += __shfl_xor(s2, 32, 64);
      if (lane < 32) {
        red[wave][0][lane] = s1;
        red[wave][1][lane] = s2;
      }
      wg_barrier();
      if (tid < 64) {
        const int which = tid >> 5, o = tid & 31;
        const float tt = red[0][which][o] + red[1][which][o] + red[2][which][o] + red[3][which][o];
        a.stats[((size_t)(b * ntiles + tile_id) * 2 + which) * a.Cout + oc0 + o] = tt;
      }
      wg_barrier();
    }
  }
}
// statistics partials per image: the 2-byte engines' MFMA kernel works on 8 x 32 tiles, the fp32 kernel on 16 x 16
int init_conv_ntiles(int H, int W, bool mfma) { return mfma ? (H / 8) * ((W + 31) / 32) : ((H + 15) / 16) * ((W + 15) / 16); }
hipError_t launch_init_conv(int dtype, const InitConvArgs& a, hipStream_t s) {
  if (a.H % 8 || a.W % 8 || a.Cout % 32 || a.c0 + a.c1 > 8) return hipErrorInvalidValue;
  const bool mfma = a.wp && dtype != 0;
  dim3 grid(init_conv_ntiles(a.H, a.W, mfma), a.B);  // 256-pixel tiles: 16 x 16 (VALU kernel) or 8 x 32 (MFMA kernel)
  return with_dtype(dtype, [&](auto t) {
    using T = decltype(t);
    if constexpr (sizeof(T) == 2) {  // the MFMA kernel exists for the 2-byte types only
      if (a.wp) {
        static const char* const name = kernel_name<T>("init_conv_mfma_kernel");
        note_kernel(name);
        hipLaunchKernelGGL(init_conv_mfma_kernel<T>, grid, dim3(256), 0, s, a);
        return hipGetLastError();
      }
    }
    static const char* const name = kernel_name<T>("init_conv_kernel");
    note_kernel(name);
    hipLaunchKernelGGL(init_conv_kernel<T>, grid, dim3(256), 0, s, a);
    return hipGetLastError();
  });
}

// =============================================================================================
// final head: affine (GroupNorm) + SiLU applied once per element while staging a 18x18 halo tile of
// 32 channels into LDS (channel-major, so a wave's pixel-consecutive reads are conflict free), then
// one thread = one pixel x Cout(<=4) outputs.  Weight layout: [tap][C][4] fp32, zero padded (repacked at load).
template <typename T>
__global__ void __launch_bounds__(256) final_conv_kernel(const FinalConvArgs a) {
  constexpr int VEC = Elem<T>::VEC;
  constexpr int VPP = 32 / VEC;  // vectors per pixel per 32-channel chunk
  __shared__ float patch[32][18][19];
  const int tid = threadIdx.x;
  const int tiles_x = (a.W + 15) / 16;  // edge tiles may be partly empty
  const int tx = blockIdx.x % tiles_x, ty = blockIdx.x / tiles_x, b = blockIdx.y;
  const int x0 = tx * 16, y0 = ty * 16;
  const int py = tid >> 4, px = tid & 15;
  const T* in = reinterpret_cast<const T*>(a.in) + (size_t)b * a.H * a.W * a.C;
  const float* __restrict__ w = a.w;
  float acc[4] = {0.f, 0.f, 0.f, 0.f};
  for (int cc = 0; cc < a.C; cc += 32) {
    if (cc) wg_barrier();
    for (int i = tid; i < 18 * 18 * VPP; i += 256) {
      const int pix = i / VPP, cv = (i % VPP) * VEC;
      const int ppy = pix / 18, ppx = pix % 18;
      const int gy = y0 + ppy - 1, gx = x0 + ppx - 1;
      float f[VEC];
      if (gy >= 0 && gy < a.H && gx >= 0 && gx < a.W) {
        ld_f32<T>(in + ((size_t)gy * a.W + gx) * a.C + cc + cv, f);
#pragma unroll
        for (int e = 0; e < VEC; ++e) {
          const int c = cc + cv + e;
          f[e] = siluf(f[e] * a.as[(size_t)b * a.C + c] + a.ab[(size_t)b * a.C + c]);
        }
      } else {
#pragma unroll
        for (int e = 0; e < VEC; ++e) f[e] = 0.f;
      }
#pragma unroll
      for (int e = 0; e < VEC; ++e) patch[cv + e][ppy][ppx] = f[e];
    }
    wg_barrier();
    for (int ci = 0; ci < 32; ++ci) {
#pragma unroll
      for (int tap = 0; tap < 9; ++tap) {
        const float v = patch[ci][py + tap / 3][px + tap % 3];
        const float* wr = w + ((size_t)tap * a.C + cc + ci) * 4;
#pragma unroll
        for (int o = 0; o < 4; ++o) acc[o] += wr[o] * v;
      }
    }
  }
#pragma unroll
  for (int o = 0; o < 4; ++o)
    if (o < a.Cout && y0 + py < a.H && x0 + px < a.W) a.out[(((size_t)b * a.Cout + o) * a.H + y0 + py) * a.W + x0 + px] = acc[o] + a.bias[o];
}
// ---------------------------------------------------------------------------------------------
// final head on MFMA (2-byte T) with the LCM scheduler step fused into the epilogue.
// Roles are swapped relative to a usual conv-GEMM: the (zero-padded) weights are the A operand
// (rows = output channel, only rows 0..2 are non-zero) and the activated halo patch is the B operand
// (columns = pixels), so after the K loop lane p of lane-half 0 holds the 3 outputs of ITS pixel in
// acc[0..2]: the epilogue (bias, LCMScheduler.step lcm_scheduler.py:204-242 or the DDIM step of lcm_step_kernel, clamp
// low_light_diffusion.py:240) is per-lane and its fp32 NCHW accesses are 64-byte row segments.
// K order per 32-channel chunk: k-step = (tap, 16-channel half); lane half h takes 8 channels.
// Weights pre-packed as [chunk][18][2][4][8] T (output channel padded to 4).
template <typename T, int TW>
__global__ void __launch_bounds__(256, 4) final_conv_mfma_kernel(const FinalConvArgs a) {
  typedef typename Elem<T>::vec_t vec_t;
  // output tile (256 / TW) x TW pixels.  TW = 16 is used: 8 x 32 tiles (128-byte instead of 64-byte runs on the fp32 planes
  // of the scheduler step) measured 210 us against 163 us at B = 32 -- this kernel is not bound by its coalescing
  constexpr int TH = 256 / TW, PH = TH + 2, PWD = TW + 3, PIX = 40;  // pixel pitch 80 B: conflict-free ds_read_b128 (cf. TilePitch)
  __shared__ __align__(16) T patch[(PH * PWD + 1) * PIX];
  const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
  const int tiles_x = (a.W + TW - 1) / TW;  // edge tiles may be partly empty
  const int tile_id = xcd_tile_order(blockIdx.x, gridDim.x);  // horizontal neighbours on one XCD (see init_conv_mfma_kernel)
  const int tx = tile_id % tiles_x, ty = tile_id / tiles_x, b = blockIdx.y;
  const int x0 = tx * TW, y0 = ty * TH;
  const T* in = reinterpret_cast<const T*>(a.in) + (size_t)b * a.H * a.W * a.C;
  const T* wp = reinterpret_cast<const T*>(a.wp);
  const int r = lane & 31, h = lane >> 5;
  f32x16 acc[2];
#pragma unroll
  for (int t = 0; t < 2; ++t)
#pragma unroll
    for (int q = 0; q < 16; ++q) acc[t][q] = 0.f;
  vec_t zero;
#pragma unroll
  for (int e = 0; e < 8; ++e) zero[e] = (T)0.f;

  // The scheduler step's operands (this lane's pixel of the fp32 planes) and the first chunk's weight fragments are
  // fetched before anything else: their latency then runs under the patch staging instead of after the MFMAs.
  const size_t plane = (size_t)a.H * a.W;
  float pre_x[2][4], pre_n[2][4];
  if (a.fuse_step && !h) {
#pragma unroll
    for (int t = 0; t < 2; ++t) {
      const int g = wave * 2 + t;
      const int y = y0 + g * (32 / TW) + r / TW, x = x0 + r % TW;
#pragma unroll
      for (int o = 0; o < 4; ++o) {
        pre_x[t][o] = pre_n[t][o] = 0.f;
        if (o < a.Cout && y < a.H && x < a.W) {
          const size_t idx = ((size_t)b * a.Cout + o) * plane + (size_t)y * a.W + x;
          pre_x[t][o] = a.sample[idx];
          if (!a.coef.is_last && !a.coef.sampler) pre_n[t][o] = a.noise[idx];
        }
      }
    }
  }
  // A operand = the weights: rows r < 4 of every fragment, zero elsewhere.  They used to live in 72 registers per lane
  // (18 k-steps x 16 bytes), which held the kernel at two waves per SIMD -- a streaming kernel that waits on its patch loads;
  // now the 2.3 KB of real rows per 32-channel chunk sit in LDS ([ks][h][4 rows][8 T], then one zero row) and each MFMA
  // reads its fragment right before use (lanes with r >= 4 all read the zero row: a broadcast).
  __shared__ __align__(16) T wsh[(18 * 2 * 4 + 1) * 8];
  auto stage_wf = [&](int chunk) {
    if (tid < 18 * 2 * 4) *reinterpret_cast<vec_t*>(wsh + tid * 8) = ld_vec<T>(wp + ((size_t)chunk * 18 * 2 * 4 + tid) * 8);
    if (tid == 18 * 2 * 4) *reinterpret_cast<vec_t*>(wsh + tid * 8) = zero;
  };
  stage_wf(0);
  const T* wrow = wsh + (r < 4 ? h * 4 + r : 18 * 2 * 4) * 8;  // + ks * 64 for rows r < 4
  const int wstep = r < 4 ? 64 : 0;

  for (int cc = 0; cc < a.C; cc += 32) {
    if (cc) {
      wg_barrier();  // everyone done with the previous chunk's patch and weights
      stage_wf(cc >> 5);
    }
    // stage the activated 10x34x32 patch (GroupNorm affine + SiLU applied once per element); a thread's
    // 8-channel slice is loop invariant (256 % 4 == 0), so its affine pairs live in registers
    const int cv = (tid & 3) * 8;
    float sc[8], sh[8];
#pragma unroll
    for (int e = 0; e < 8; ++e) {
      sc[e] = a.as[(size_t)b * a.C + cc + cv + e];
      sh[e] = a.ab[(size_t)b * a.C + cc + cv + e];
    }
    for (int i = tid; i < (PH * PWD + 1) * 4; i += 256) {
      const int pix = i >> 2;
      const int ppy = pix / PWD, ppx = pix % PWD;
      const int gy = y0 + ppy - 1, gx = x0 + ppx - 1;
      vec_t v = zero;
      if (pix < PH * PWD && ppx < TW + 2 && gy >= 0 && gy < a.H && gx >= 0 && gx < a.W) {
        float f[8];
        ld_f32<T>(in + ((size_t)gy * a.W + gx) * a.C + cc + cv, f);
#pragma unroll
        for (int e = 0; e < 8; ++e) f[e] = siluf_fast(f[e] * sc[e] + sh[e]);
        v = f32_to_vec<T>(f);
      }
      *reinterpret_cast<vec_t*>(patch + pix * PIX + cv) = v;
    }
    wg_barrier();
#pragma unroll
    for (int t = 0; t < 2; ++t) {
      const int g = wave * 2 + t;
      const int py = g * (32 / TW) + r / TW, px = r % TW;
#pragma unroll
      for (int ks = 0; ks < 18; ++ks) {
        const int tap = ks >> 1, q = ks & 1;
        // one tap row (6 k-steps, 12 fragment reads) at a time: left alone, hipcc hoists all 36 reads of a block (144 registers)
        if (ks % 6 == 0) __builtin_amdgcn_sched_barrier(0);
        const vec_t bv = *reinterpret_cast<const vec_t*>(patch + ((py + tap / 3) * PWD + px + tap % 3) * PIX + q * 16 + h * 8);
        const vec_t wv = *reinterpret_cast<const vec_t*>(wrow + ks * wstep);
        if constexpr (std::is_same<T, half_t>::value) acc[t] = __builtin_amdgcn_mfma_f32_32x32x16_f16(wv, bv, acc[t], 0, 0, 0);
        else acc[t] = __builtin_amdgcn_mfma_f32_32x32x16_bf16(wv, bv, acc[t], 0, 0, 0);
      }
    }
  }
  if (h) return;  // rows 4..7 of D (lane half 1) are padding
  {
#pragma clang fp contract(off)  // scheduler step: keep the reference's operation order (no fused multiply-adds)
#pragma unroll
  for (int t = 0; t < 2; ++t) {
    const int g = wave * 2 + t;
    const int y = y0 + g * (32 / TW) + r / TW, x = x0 + r % TW;
    if (y >= a.H || x >= a.W) continue;
#pragma unroll
    for (int o = 0; o < 4; ++o) {
      if (o >= a.Cout) break;
      const size_t idx = ((size_t)b * a.Cout + o) * plane + (size_t)y * a.W + x;
      const float e = acc[t][o] + a.bias[o];
      if (a.out) a.out[idx] = e;
      if (a.fuse_step) {
        const float xv = pre_x[t][o];
        float x0v;
        if (a.coef.vpred) x0v = a.coef.sa * xv - a.coef.sb * e;
        else x0v = (xv - a.coef.sb * e) / a.coef.sa;
        if (a.coef.clamp_x0) x0v = fminf(fmaxf(x0v, -1.f), 1.f);
        float pv = x0v;
        if (!a.coef.is_last) {
          float nz = pre_n[t][o];
          if (a.coef.sampler) nz = a.coef.vpred ? a.coef.sa * e + a.coef.sb * xv : e;  // DDIM: the predicted noise, no draw
          pv = a.coef.sap * x0v + a.coef.sbp * nz;
        }
        a.prev[idx] = pv;
        if (a.clamped) a.clamped[idx] = fminf(fmaxf(pv, -1.f), 1.f);
      }
    }
  }
  }
}
hipError_t launch_final_conv(int dtype, const FinalConvArgs& a, hipStream_t s) {
  if (a.H % 8 || a.W % 8 || a.C % 32 || a.Cout > 4) return hipErrorInvalidValue;
  if (a.fuse_step && (!a.wp || dtype == 0 || !a.sample || !a.prev || (!a.coef.is_last && !a.coef.sampler && !a.noise) ||
                      (a.coef.sampler && a.coef.clamp_x0))) return hipErrorInvalidValue;
  if (!a.fuse_step && !a.out) return hipErrorInvalidValue;
  dim3 grid(((a.H + 15) / 16) * ((a.W + 15) / 16), a.B);
  return with_dtype(dtype, [&](auto t) {
    using T = decltype(t);
    if constexpr (sizeof(T) == 2) {  // the MFMA kernel exists for the 2-byte types only
      if (a.wp) {
        static const char* const name = kernel_name<T>("final_conv_mfma_kernel", 16);
        note_kernel(name);
        hipLaunchKernelGGL((final_conv_mfma_kernel<T, 16>), grid, dim3(256), 0, s, a);
        return hipGetLastError();
      }
    }
    static const char* const name = kernel_name<T>("final_conv_kernel");
    note_kernel(name);
    hipLaunchKernelGGL(final_conv_kernel<T>, grid, dim3(256), 0, s, a);
    return hipGetLastError();
  });
}

}  // namespace llie
