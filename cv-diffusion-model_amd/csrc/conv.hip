// Dense 3x3 convolutions of the denoiser (gfx950).
//   Downsample  (efficient_unet.py:367)  3x3 stride 2       } implicit GEMM on MFMA: M = 8 x TW output pixels,
//   Upsample    (efficient_unet.py:383-384) bilinear x2 + 3x3 } N = Cout tile, K = 9 taps x Cin; the upsampled
//               halo patch is interpolated on the fly into LDS, so the 4x tensor never reaches HBM.
// (The 3 -> C0 head and C0 -> 3 tail convs: conv_edge.hip; the up-sampling convs from folded weights / tap maps: upconv.hip.)
#include <type_traits>

#include "common.h"
#include "kernels.h"
#include "mfma_tile.h"

namespace llie {

// =============================================================================================
// Implicit-GEMM 3x3 conv on MFMA.  MODE 0: stride 2, pad 1.  MODE 1: bilinear x2 (align_corners=False:
// src = (dst+0.5)/2 - 0.5 clamped at 0, upper neighbour clamped at n-1) then stride 1, pad 1.
// STAMP: diagnostic build (llie_tune("conv_stamp", 1)): s_memtime sums per wave into a.stamps[wave][kConvStamps] = {0 patch
// commit (bounds / bilinear blend + ds_write), 1 first W tile staged + barrier, 2 operand ds_reads of a tap, 3 its MFMAs,
// 4 next W tile staged + prefetch issued, 5 the tap's barrier, 6 epilogue}; never used in production.
constexpr int kConvStamps = 7;
template <typename T, int MODE, int TW, int BN, int WM, int WN, bool RAGGED = false, bool STAMP = false>
__global__ void __launch_bounds__(WM* WN * 64) conv3x3_kernel(const Conv3Args a) {
  constexpr int NT = WM * WN * 64;
  unsigned long long tk[kConvStamps] = {}, t_prev = 0;
  auto stamp = [&](int slot) {
    if constexpr (STAMP) {
      __builtin_amdgcn_sched_barrier(0);
      const unsigned long long now = __builtin_amdgcn_s_memtime();
      __builtin_amdgcn_sched_barrier(0);
      if (slot >= 0) tk[slot] += now - t_prev;
      t_prev = now;
    }
  };
  constexpr int TH = 8, BM = TH * TW;
  constexpr int VEC = Elem<T>::VEC, VPR = 32 / VEC, PITCH = TilePitch<T>::value;
  constexpr int MI = BM / (WM * 32), NI = BN / (WN * 32);
  constexpr int PH = MODE == 0 ? 2 * TH + 1 : TH + 2;
  constexpr int PW = MODE == 0 ? 2 * TW + 1 : TW + 2;
  constexpr int B_VECS = BN * VPR, B_PER = (B_VECS + NT - 1) / NT;
  constexpr int CP = BN + 4;
  typedef typename Elem<T>::vec_t vec_t;
  static_assert(NT % VPR == 0, "mapping");

  extern __shared__ __align__(16) unsigned char smem[];
  T* sP = reinterpret_cast<T*>(smem);
  T* sB = sP + PH * PW * PITCH;  // [2][BN][PITCH]
  float* sC = reinterpret_cast<float*>(smem);

  const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
  const int wm = wave / WN, wn = wave % WN;
  const int Ho = MODE == 0 ? a.Hi / 2 : (MODE == 1 ? a.Hi * 2 : a.Hi), Wo = MODE == 0 ? a.Wi / 2 : (MODE == 1 ? a.Wi * 2 : a.Wi);
  // ragged outputs (Ho % 8 or Wo % TW != 0: image sizes that are not a multiple of 64): edge tiles are partly empty -- pixels past
  // the image are neither stored nor counted (the patch loader already reads everything outside as zero)
  const int nb = a.Cout / BN, tiles_x = RAGGED ? (Wo + TW - 1) / TW : Wo / TW, tiles = tiles_x * (RAGGED ? (Ho + TH - 1) / TH : Ho / TH);
  int bid = blockIdx.x;
  const int ntile = bid % nb; bid /= nb;
  const int tile = bid % tiles, b = bid / tiles;
  const int oy0 = (tile / tiles_x) * TH, ox0 = (tile % tiles_x) * TW;
  const int n0 = ntile * BN;
  const int kv = (tid % VPR) * VEC;
  const T* in = reinterpret_cast<const T*>(a.in) + (size_t)b * a.Hi * a.Wi * a.Cin;
  const T* wbase = reinterpret_cast<const T*>(a.w);

  f32x16 acc[MI][NI];
#pragma unroll
  for (int i = 0; i < MI; ++i)
#pragma unroll
    for (int j = 0; j < NI; ++j)
#pragma unroll
      for (int r = 0; r < 16; ++r) acc[i][j][r] = 0.f;

  // per-lane patch offsets of this lane's A rows (tap (0,0)); tap (dy,dx) adds (dy*PW+dx)*PITCH
  // MODE 1, TW = 16: odd tile rows are rotated by two pixels in the GEMM row order (mfma_tile.h: tile_px, conflict-free A reads)
  constexpr bool ROT = MODE == 1 && TW == 16;
  int arow[MI];
#pragma unroll
  for (int i = 0; i < MI; ++i) {
    const int m = (wm * MI + i) * 32 + (lane & 31);
    int py, px;
    tile_px<TW, ROT>(m, py, px);
    arow[i] = (MODE == 0 ? (2 * py * PW + 2 * px) : (py * PW + px)) * PITCH + (lane >> 5) * 16;
  }

  vec_t rb[B_PER];
  auto prefetch_w = [&](int tap, int c0) {
#pragma unroll
    for (int i = 0; i < B_PER; ++i) {
      const int idx = tid + i * NT;
      if (B_VECS % NT == 0 || idx < B_VECS) {
        const int n = idx / VPR;
        rb[i] = ld_vec<T>(wbase + ((size_t)tap * a.Cout + n0 + n) * a.Cin + c0 + kv);
      }
    }
  };
  auto stage_w = [&](int buf) {  // two W tiles in LDS: tap t computes from buffer t & 1 while t + 1 is being written
#pragma unroll
    for (int i = 0; i < B_PER; ++i) {
      const int idx = tid + i * NT;
      if (B_VECS % NT == 0 || idx < B_VECS) st_vec<T>(sB + buf * (BN * PITCH) + (idx / VPR) * PITCH + kv, rb[i]);
    }
  };

  // Input patch of one 32-channel chunk: the global loads are issued one chunk ahead (issue_patch keeps the raw
  // vectors in registers while the nine taps of the current chunk run) and turned into the LDS patch afterwards
  // (commit_patch: bounds -> zeros, MODE 1 interpolates its four neighbours).
  constexpr int P_ITEMS = (PH * PW * VPR + NT - 1) / NT, P_LOADS = MODE == 1 ? 4 : 1;
  vec_t praw[P_ITEMS][P_LOADS];
  struct Src { bool ok; int o00, o01, o10, o11; float ly1, lx1; };
  auto patch_src = [&](int i) {
    Src r{false, 0, 0, 0, 0, 0.f, 0.f};
    if (i >= PH * PW * VPR) return r;
    const int pix = i / VPR;
    const int ppy = pix / PW, ppx = pix % PW;
    if (MODE == 0 || MODE == 2) {
      const int gy = (MODE == 0 ? 2 * oy0 : oy0) - 1 + ppy, gx = (MODE == 0 ? 2 * ox0 : ox0) - 1 + ppx;
      r.ok = gy >= 0 && gy < a.Hi && gx >= 0 && gx < a.Wi;
      r.o00 = (gy * a.Wi + gx) * a.Cin;
    } else {
      const int uy = oy0 - 1 + ppy, ux = ox0 - 1 + ppx;  // coordinates in the upsampled image
      r.ok = uy >= 0 && uy < Ho && ux >= 0 && ux < Wo;
      float sy = ((float)uy + 0.5f) * 0.5f - 0.5f, sx = ((float)ux + 0.5f) * 0.5f - 0.5f;
      sy = sy < 0.f ? 0.f : sy;
      sx = sx < 0.f ? 0.f : sx;
      const int iy0 = (int)sy, ix0 = (int)sx;
      const int iy1 = min(iy0 + 1, a.Hi - 1), ix1 = min(ix0 + 1, a.Wi - 1);
      r.ly1 = sy - (float)iy0; r.lx1 = sx - (float)ix0;
      r.o00 = (iy0 * a.Wi + ix0) * a.Cin; r.o01 = (iy0 * a.Wi + ix1) * a.Cin;
      r.o10 = (iy1 * a.Wi + ix0) * a.Cin; r.o11 = (iy1 * a.Wi + ix1) * a.Cin;
    }
    return r;
  };
  auto issue_item = [&](int it, int c0) {
    {
      const Src r = patch_src(tid + it * NT);
      if (r.ok) {
        const T* base = in + c0 + kv;
        praw[it][0] = ld_vec<T>(base + r.o00);
        if (MODE == 1) {
          praw[it][P_LOADS > 1 ? 1 : 0] = ld_vec<T>(base + r.o01);
          praw[it][P_LOADS > 2 ? 2 : 0] = ld_vec<T>(base + r.o10);
          praw[it][P_LOADS > 3 ? 3 : 0] = ld_vec<T>(base + r.o11);
        }
      }
    }
  };
  auto commit_item = [&](int it) {
    {
      const int i = tid + it * NT;
      if (i >= PH * PW * VPR) return;
      const Src r = patch_src(i);
      vec_t v;
      if (!r.ok) {
#pragma unroll
        for (int e = 0; e < VEC; ++e) v[e] = (T)0.f;
      } else if (MODE == 1) {
        const float ly0 = 1.f - r.ly1, lx0 = 1.f - r.lx1;
        float f00[VEC], f01[VEC], f10[VEC], f11[VEC], f[VEC];
        vec_to_f32<T>(praw[it][0], f00);
        vec_to_f32<T>(praw[it][P_LOADS > 1 ? 1 : 0], f01);
        vec_to_f32<T>(praw[it][P_LOADS > 2 ? 2 : 0], f10);
        vec_to_f32<T>(praw[it][P_LOADS > 3 ? 3 : 0], f11);
#pragma unroll
        for (int e = 0; e < VEC; ++e)
          f[e] = ly0 * (lx0 * f00[e] + r.lx1 * f01[e]) + r.ly1 * (lx0 * f10[e] + r.lx1 * f11[e]);
        v = f32_to_vec<T>(f);
      } else {
        v = praw[it][0];
      }
      st_vec<T>(sP + (i / VPR) * PITCH + kv, v);
    }
  };

  // measured: the look-ahead pays everywhere except the 64-channel upsampling conv (4 x 3 raw vectors per thread
  // cost it an occupancy step: 294 -> 365 us), which keeps load-then-use
  constexpr bool PREF = !(MODE == 1 && BN == 64);
  auto issue_patch = [&](int c0) {
#pragma unroll
    for (int it = 0; it < P_ITEMS; ++it) issue_item(it, c0);
  };
  if (PREF) issue_patch(0);
  stamp(-1);
  for (int c0 = 0; c0 < a.Cin; c0 += 32) {
    prefetch_w(0, c0);
    if constexpr (PREF) {  // this chunk's patch: its loads were issued during the previous chunk's taps
#pragma unroll
      for (int it = 0; it < P_ITEMS; ++it) commit_item(it);
    } else {  // load-then-use, one item at a time (lowest register footprint); MODE 1 only
      for (int i = tid; i < PH * PW * VPR; i += NT) {
        const int pix = i / VPR;
        const int ppy = pix / PW, ppx = pix % PW;
        vec_t v;
        const int uy = oy0 - 1 + ppy, ux = ox0 - 1 + ppx;  // coordinates in the upsampled image
        if (uy >= 0 && uy < Ho && ux >= 0 && ux < Wo) {
          float sy = ((float)uy + 0.5f) * 0.5f - 0.5f, sx = ((float)ux + 0.5f) * 0.5f - 0.5f;
          sy = sy < 0.f ? 0.f : sy;
          sx = sx < 0.f ? 0.f : sx;
          const int iy0 = (int)sy, ix0 = (int)sx;
          const int iy1 = min(iy0 + 1, a.Hi - 1), ix1 = min(ix0 + 1, a.Wi - 1);
          const float ly1 = sy - (float)iy0, lx1 = sx - (float)ix0;
          const float ly0 = 1.f - ly1, lx0 = 1.f - lx1;
          float f00[VEC], f01[VEC], f10[VEC], f11[VEC], f[VEC];
          ld_f32<T>(in + ((size_t)iy0 * a.Wi + ix0) * a.Cin + c0 + kv, f00);
          ld_f32<T>(in + ((size_t)iy0 * a.Wi + ix1) * a.Cin + c0 + kv, f01);
          ld_f32<T>(in + ((size_t)iy1 * a.Wi + ix0) * a.Cin + c0 + kv, f10);
          ld_f32<T>(in + ((size_t)iy1 * a.Wi + ix1) * a.Cin + c0 + kv, f11);
#pragma unroll
          for (int e = 0; e < VEC; ++e)
            f[e] = ly0 * (lx0 * f00[e] + lx1 * f01[e]) + ly1 * (lx0 * f10[e] + lx1 * f11[e]);
          v = f32_to_vec<T>(f);
        } else {
#pragma unroll
          for (int e = 0; e < VEC; ++e) v[e] = (T)0.f;
        }
        st_vec<T>(sP + pix * PITCH + kv, v);
      }
    }
    stamp(0);
    stage_w(0);
    prefetch_w(1, c0);
    wg_barrier();  // patch and W tile of tap 0 visible
    if (PREF && c0 + 32 < a.Cin) issue_patch(c0 + 32);
    stamp(1);
    for (int tap = 0; tap < 9; ++tap) {
      const int toff = ((tap / 3) * PW + (tap % 3)) * PITCH;
      T fa[MI][16], fb[NI][16];
#pragma unroll
      for (int i = 0; i < MI; ++i) {
        const T* p = sP + arow[i] + toff;
#pragma unroll
        for (int q = 0; q < 16 / VEC; ++q) *reinterpret_cast<vec_t*>(&fa[i][q * VEC]) = *reinterpret_cast<const vec_t*>(p + q * VEC);
      }
#pragma unroll
      for (int j = 0; j < NI; ++j) {
        const T* p = sB + (tap & 1) * (BN * PITCH) + ((wn * NI + j) * 32 + (lane & 31)) * PITCH + (lane >> 5) * 16;
#pragma unroll
        for (int q = 0; q < 16 / VEC; ++q) *reinterpret_cast<vec_t*>(&fb[j][q * VEC]) = *reinterpret_cast<const vec_t*>(p + q * VEC);
      }
      if constexpr (STAMP) asm volatile("s_waitcnt lgkmcnt(0)" ::: "memory");
      stamp(2);
#pragma unroll
      for (int i = 0; i < MI; ++i)
#pragma unroll
        for (int j = 0; j < NI; ++j) Mfma<T>::chunk(fa[i], fb[j], acc[i][j]);
      stamp(3);
      if (tap + 1 < 9) {
        stage_w((tap + 1) & 1);  // its last readers finished before the previous barrier
        if (tap + 2 < 9) prefetch_w(tap + 2, c0);
      }
      stamp(4);
      wg_barrier();  // next W tile visible; everyone done with this one (and, after tap 8, with the patch)
      stamp(5);
      // (Tried in round 4 and removed: issuing the next tap's operand ds_reads right behind this tap's MFMAs, into the same
      // registers, with a third W buffer -- MFMAs issue in order at the pipe's pace, so the reads start when the last MFMA
      // has issued, and the in-place overwrite of MFMA source registers stalls: 313 vs 244 us at C = 256.  A second
      // register set costs 32 VGPRs = one of the two waves per SIMD.  The loop is co-bound by LDS traffic: per tap and
      // workgroup 32 KB of fragment reads (128 cycles) + 8 KB of W tile writes (~104) against 256 cycles of MFMA.)
    }
  }

  // ---- epilogue (same scheme as the pointwise GEMM): one pass per 32-row MFMA block index, so the
  // fp32 staging tile holds only WM*32 rows and the kernel fits 4 workgroups per CU
  constexpr int VR = BN / VEC, RPP = NT / VR, SROWS = WM * 32;
  static_assert(NT % VR == 0 && VR <= 64, "epilogue mapping");
  const int cv = tid % VR, r0 = tid / VR;
  float bias[VEC], s1[VEC], s2[VEC];
#pragma unroll
  for (int e = 0; e < VEC; ++e) {
    bias[e] = a.bias ? a.bias[n0 + cv * VEC + e] : 0.f;
    s1[e] = 0.f;
    s2[e] = 0.f;
  }
  T* outp = reinterpret_cast<T*>(a.out) + (size_t)b * Ho * Wo * a.Cout;
#pragma unroll
  for (int pi = 0; pi < MI; ++pi) {
    if (pi) wg_barrier();
    stage_acc_tile<CP>(sC, acc[pi], wm, wn, lane);
    wg_barrier();
    for (int srow = r0; srow < SROWS; srow += RPP) {
      const int row = ((srow >> 5) * MI + pi) * 32 + (srow & 31);  // pixel index inside the BM tile
      float v[VEC];
      const float* pc = sC + srow * CP + cv * VEC;
#pragma unroll
      for (int e = 0; e < VEC; ++e) v[e] = pc[e] + bias[e];
      int py, px;
      tile_px<TW, ROT>(row, py, px);
      const int oy = oy0 + py, ox = ox0 + px;
      if (RAGGED && (oy >= Ho || ox >= Wo)) continue;
      vec_t ov = f32_to_vec<T>(v);
      st_vec_pol<T>(outp + ((size_t)oy * Wo + ox) * a.Cout + n0 + cv * VEC, ov, a.nt != 0);
#pragma unroll
      for (int e = 0; e < VEC; ++e) {
        const float q = (float)ov[e];
        s1[e] += q;
        s2[e] += q * q;
      }
    }
  }
  if (a.stats) {
#pragma unroll
    for (int o = VR; o < 64; o <<= 1)
#pragma unroll
      for (int e = 0; e < VEC; ++e) {
        s1[e] += __shfl_xor(s1[e], o, 64);
        s2[e] += __shfl_xor(s2[e], o, 64);
      }
    float* red = sC + SROWS * CP;
    constexpr int NW = NT / 64;
    if (lane < VR) {
#pragma unroll
      for (int e = 0; e < VEC; ++e) {
        red[(wave * 2 + 0) * BN + cv * VEC + e] = s1[e];
        red[(wave * 2 + 1) * BN + cv * VEC + e] = s2[e];
      }
    }
    wg_barrier();
    for (int i = tid; i < 2 * BN; i += NT) {
      const int which = i / BN, c = i % BN;
      float t = 0.f;
#pragma unroll
      for (int w = 0; w < NW; ++w) t += red[(w * 2 + which) * BN + c];
      a.stats[((size_t)(b * tiles + tile) * 2 + which) * a.Cout + n0 + c] = t;
    }
  }
  stamp(6);
  if constexpr (STAMP) {
    if (a.stamps && lane == 0) {
#pragma unroll
      for (int i = 0; i < kConvStamps; ++i) a.stamps[((size_t)blockIdx.x * (NT / 64) + wave) * kConvStamps + i] = tk[i];
    }
  }
}

StampSink g_conv_stamps{kConvStamps, 0};  // cycles per wave, the slots listed at STAMP

static int conv_tw(int Wo) { return (Wo % 16 == 0) ? 16 : 8; }
// the tile width launch_conv_t takes: ragged maps (Ho % 8 or Wo % 8) run 8-wide tiles whatever Wo is -- a 9 x 16 map is four tiles
static int conv_tw(int Ho, int Wo) { return (Ho % 8 || Wo % 8) ? 8 : conv_tw(Wo); }
int conv3x3_ntiles(int Ho, int Wo) { return ((Ho + 7) / 8) * ((Wo + conv_tw(Ho, Wo) - 1) / conv_tw(Ho, Wo)); }

template <typename T, int MODE, int TW, int BN, int WM, int WN, bool RAGGED = false>
static hipError_t launch_conv_cfg(const Conv3Args& a, hipStream_t s) {
  constexpr int NT = WM * WN * 64, BM = 8 * TW, PITCH = TilePitch<T>::value;
  constexpr int PH = MODE == 0 ? 17 : 10, PW = MODE == 0 ? 2 * TW + 1 : TW + 2;
  constexpr size_t tiles = (size_t)(PH * PW + 2 * BN) * PITCH * sizeof(T);
  constexpr size_t ctile = (size_t)(WM * 32) * (BN + 4) * 4 + (size_t)(NT / 64) * 2 * BN * 4;
  constexpr size_t lds = tiles > ctile ? tiles : ctile;
  static std::atomic<uint64_t> attr_done{0};
  if (lds > 48 * 1024) {
    if (hipError_t e = ensure_max_lds(reinterpret_cast<const void*>(&conv3x3_kernel<T, MODE, TW, BN, WM, WN, RAGGED>), (int)lds, attr_done);
        e != hipSuccess)
      return e;
  }
  const int Ho = MODE == 0 ? a.Hi / 2 : (MODE == 1 ? a.Hi * 2 : a.Hi), Wo = MODE == 0 ? a.Wi / 2 : (MODE == 1 ? a.Wi * 2 : a.Wi);
  const unsigned grid = (unsigned)(a.B * ((Ho + 7) / 8) * ((Wo + TW - 1) / TW) * (a.Cout / BN));
  static const char* const name = kernel_name<T>("conv3x3_kernel", MODE, TW, BN, WM, WN);
  note_kernel(name);
  if constexpr (MODE == 1 && TW == 16 && !RAGGED && std::is_same<T, half_t>::value) {
    if (g_knobs.conv_stamp) {  // diagnostic build with in-kernel cycle stamps
      Conv3Args b = a;
      if (hipError_t e = g_conv_stamps.arm((size_t)grid * (NT / 64), &b.stamps); e != hipSuccess) return e;
      static std::atomic<uint64_t> stamp_attr_done{0};
      if (lds > 48 * 1024) {
        if (hipError_t e = ensure_max_lds(reinterpret_cast<const void*>(&conv3x3_kernel<T, MODE, TW, BN, WM, WN, RAGGED, true>), (int)lds, stamp_attr_done);
            e != hipSuccess)
          return e;
      }
      hipLaunchKernelGGL((conv3x3_kernel<T, MODE, TW, BN, WM, WN, RAGGED, true>), dim3(grid), dim3(NT), lds, s, b);
      return hipGetLastError();
    }
  }
  hipLaunchKernelGGL((conv3x3_kernel<T, MODE, TW, BN, WM, WN, RAGGED>), dim3(grid), dim3(NT), lds, s, a);
  return hipGetLastError();
}

template <typename T, int MODE>
static hipError_t launch_conv_t(const Conv3Args& a, hipStream_t s) {
  const int Ho = MODE == 0 ? a.Hi / 2 : (MODE == 1 ? a.Hi * 2 : a.Hi), Wo = MODE == 0 ? a.Wi / 2 : (MODE == 1 ? a.Wi * 2 : a.Wi);
  if (Ho < 1 || Wo < 1 || a.Cin % 32 || a.Cout % 32 || (MODE == 0 && (a.Hi % 2 || a.Wi % 2))) return hipErrorInvalidValue;
  // partly empty edge tiles: maps that are not a multiple of 8 (image sizes % 64 != 0); MODE 2 = training
  const bool ragged = Ho % 8 || Wo % 8;
  return with_value<128, 64, 32>((a.Cout % 128 == 0) ? 128 : ((a.Cout % 64 == 0) ? 64 : 32), [&](auto bn) {
    constexpr int BN = decltype(bn)::value, WN = BN == 32 ? 1 : 2;  // 32-column tiles: one wave wide, 16-wide ones four waves tall
    if (ragged) return launch_conv_cfg<T, MODE, 8, BN, 2, WN, true>(a, s);
    if (conv_tw(Wo) == 16) return launch_conv_cfg<T, MODE, 16, BN, BN == 32 ? 4 : 2, WN>(a, s);
    return launch_conv_cfg<T, MODE, 8, BN, 2, WN>(a, s);
  });
}

hipError_t launch_conv3x3(int dtype, const Conv3Args& a, hipStream_t s) {
  return with_value<0, 1, 2>(a.mode, [&](auto mode) {
    return with_dtype(dtype, [&](auto t) { return launch_conv_t<decltype(t), decltype(mode)::value>(a, s); });
  });
}

}  // namespace llie
