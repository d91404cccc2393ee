// Front half of an InvertedResidualBlock in its "recompute" form for gfx950 (2-byte compute types):
//
//   h2 = dw3x3( relu6( aff2( W1 . relu6( aff1(x) ) ) ) )      aff1 = GroupNorm-1, aff2 = GroupNorm-2 + FiLM
//   (efficient_unet.py:207-220: norm1, ReLU6, expand, norm2, FiLM, ReLU6, depthwise)
//
// The 4x-expanded tensor h1 = W1 . a is the largest object of the network.  The unfused path writes it (pw_gemm)
// and reads it back (dwconv3x3); here it never reaches HBM (SURVEY.md 8d "recompute variant", 3Cin + 2Chid + Cout
// elements per pixel instead of 2Cin + 4Chid + Cout):
//
//   expand_stats_kernel  reads x once and produces only h1's per-channel (sum, sum of squares) slab for GroupNorm-2:
//                        lanes load their MFMA operand slices of x straight from HBM (16 B per lane), the 32x32
//                        accumulators are squared / summed in registers and never stored;
//   expand_dw_kernel     a workgroup owns an 8 x 16 pixel tile: it rebuilds h1 on the 10 x 18 halo tile with MFMA
//                        (weights = A operand, pixels = B operand, so a lane ends up with runs of channels of ONE
//                        pixel), applies aff2 + ReLU6 (+ zero padding) to the accumulators, parks the tile in LDS as
//                        [pixel][64 channels] and runs the depthwise 3x3 from there, 64 hidden channels at a time;
//                        the x tile is loaded once per tile (next tile prefetched) and reused by every channel chunk.
//
// The GroupNorm partial sums are fixed per-tile slab entries; the SE pool sums go into per-image 64-bit fixed-point
// totals with integer atomics (integer adds commute).  No float atomics, so results stay bitwise independent of the
// batch and of the schedule.
#include <type_traits>
#include <vector>

#include "common.h"
#include "kernels.h"

namespace llie {

typedef uint32_t u32x2 __attribute__((ext_vector_type(2)));

typedef __bf16 bf16x2_t __attribute__((ext_vector_type(2)));
__device__ __forceinline__ float dot2_bf16(uint32_t a, uint32_t b, float c) {
  return __builtin_amdgcn_fdot2_f32_bf16(*reinterpret_cast<const bf16x2_t*>(&a), *reinterpret_cast<const bf16x2_t*>(&b), c, false);
}

// ---------------------------------------------------------------------------------------------
// Both kernels run out of VALU issue slots first (a wave64 instruction holds its SIMD for 4 cycles), so the two
// activations are written for instruction count.  ReLU6 is carried as clamp01(z / 6): the clamp is the FMA's free output
// modifier, and the factor 6 is pushed through the linear operators that follow -- the expand GEMM (h1 = 6 W1 a', so
// GroupNorm-2 sees sums scaled by 6 / 36 and its affine is applied to acc' = acc / 6 with shift / 6) and the depthwise
// conv (weights staged as 6 w).  In real arithmetic nothing changes; in T the rounding points move by one operation.
// a' = clamp01(a * s + b) = relu6(norm1(a)) / 6 on one 16-byte operand slice (8 channels); sc / sh point at the slice's
// 8 scale / shift values (already divided by 6) in an LDS table (16-byte aligned), read at use
template <typename T>
__device__ __forceinline__ typename Elem<T>::vec_t activate8(typename Elem<T>::vec_t v, const float* sc, const float* sh) {
  const u32x4 x = reinterpret_cast<const u32x4&>(v);
  const f32x4 s0 = *reinterpret_cast<const f32x4*>(sc), s1 = *reinterpret_cast<const f32x4*>(sc + 4);
  const f32x4 b0 = *reinterpret_cast<const f32x4*>(sh), b1 = *reinterpret_cast<const f32x4*>(sh + 4);
  u32x4 o;
  o[0] = act_clamp01_pack<T>(x[0], s0[0], s0[1], b0[0], b0[1]);
  o[1] = act_clamp01_pack<T>(x[1], s0[2], s0[3], b0[2], b0[3]);
  o[2] = act_clamp01_pack<T>(x[2], s1[0], s1[1], b1[0], b1[1]);
  o[3] = act_clamp01_pack<T>(x[3], s1[2], s1[3], b1[2], b1[3]);
  return reinterpret_cast<const typename Elem<T>::vec_t&>(o);
}

// ---------------------------------------------------------------------------------------------
// (1) statistics of h1 = W1 . relu6(aff1(x)) without storing it.
//   grid (P / RP, 1, B): a workgroup walks RP pixels of one image in steps of 128.  Each step's x rows are activated
//   ONCE, cooperatively, into a double-buffered LDS tile (one barrier per step); wave w owns the NBW = Chid / 128
//   32-channel blocks [w * NBW, (w + 1) * NBW) -- their weight slices stay in registers -- and multiplies them with all
//   four 32-pixel blocks of the tile.  MFMA roles: A = pixels (rows), B = weights (columns): a lane holds 16 pixels of
//   ONE channel, so the per-channel sums are plain register adds and no accumulator is ever stored.
//
// POOL: the same walk produces the SE pool totals of the block instead (expand_pool_kernel).  The depthwise conv is linear and
// zero-padded, so sum_p dw(a)_c[p] = sum_tap w_c[tap] * S_tap with S_tap = the sum of a_c over the pixels the tap can reach:
// the whole image minus one border row and / or column (plus the corner they share).  Nine sums of a = relu6(aff2(h1)) / 6
// per channel -- everything, first / last row, first / last column, four corners -- replace h2: a is rounded to T where
// expand_dw_kernel rounds the tile it parks in LDS, the weights are the 6 w in T it stages, so the two routes add the same numbers.
// Two accumulator registers pack into one dword of T and one v_dot2 adds both to an fp32 sum.  Every 16-pixel group adds its sum
// to the total; W % 16 == 0, so a group lies in one image row and starts at a multiple of 16, and only a group of the first / last
// image row or the first / last group of a row can touch a border class (one in eight at W = 256, one in four at W = 128).  Those
// groups alone enter ONE wave-uniform branch that holds all border work: the one-hot operands (this lane's first- / last-column
// pixel), the column sums (v_dot2 against them on the two registers that can hold such a pixel), the row sums and the four
// corners.  Whether a group is an edge group follows from blockIdx and loop counters, i.e. from scalar registers.  Written as
// plain `if`s hipcc turned all of it into selects that every group executed (88 VALU instructions per 32 x 32 block at <2, 1>,
// 37 with the branch); the skipped instructions only ever added exact zeros, so the totals did not change by a bit.
constexpr int kXStamps = 9;  // cycle-stamp slots of a diagnostic build (STAMP, below)
template <typename T> struct PackedOne;
template <> struct PackedOne<half_t> { static constexpr uint32_t lo = 0x00003C00u, hi = 0x3C000000u; };
template <> struct PackedOne<bf16_t> { static constexpr uint32_t lo = 0x00003F80u, hi = 0x3F800000u; };
// c + a.lo * b.lo + a.hi * b.hi on packed dwords of T
template <typename T> __device__ __forceinline__ float dot2_pk(uint32_t a, uint32_t b, float c) {
  if constexpr (std::is_same<T, half_t>::value)
    return __builtin_amdgcn_fdot2(*reinterpret_cast<const f16x2*>(&a), *reinterpret_cast<const f16x2*>(&b), c, false);
  else return dot2_bf16(a, b, c);
}

// STAMP = diagnostic build (llie_tune("irbx_stamp", 2), expand_pool in fp16): s_memtime around the phases of a step, summed per
// wave into a.dbg ([workgroup][wave][kXStamps] cycles: 0 wait for the step's loads (vmcnt), 1 activation + ds_write + next step's
// loads issued, 2 barrier, 3 fragment reads + MFMAs until the accumulator can be read, 4 epilogue; 5.. unused)
template <typename T, int KS, int NBW, bool POOL, bool STAMP = false>
__device__ __forceinline__ void expand_scan(const IrbxArgs& a, const int RP) {
  constexpr int K = 16 * KS, XP = (K + 8) * 2;  // LDS pixel pitch in bytes: conflict-free ds_read_b128
  typedef typename Elem<T>::vec_t vec_t;
  __shared__ __align__(16) unsigned char sA[2][128 * XP];
  __shared__ __align__(16) float aff1[2][K];
  const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
  const int n = lane & 31, h = lane >> 5;
  const int b = blockIdx.z, tile = blockIdx.x;
  const int P = a.H * a.W;
  const T* x0 = reinterpret_cast<const T*>(a.x0) + (size_t)b * P * a.c0;
  const T* x1 = a.x1 ? reinterpret_cast<const T*>(a.x1) + (size_t)b * P * a.c1 : nullptr;
  const T* w1 = reinterpret_cast<const T*>(a.w1);

  vec_t wf[NBW][KS];
#pragma unroll
  for (int j = 0; j < NBW; ++j)
#pragma unroll
    for (int s = 0; s < KS; ++s) wf[j][s] = ld_vec<T>(w1 + (size_t)((wave * NBW + j) * 32 + n) * K + 16 * s + 8 * h);
  for (int i = tid; i < K; i += 256) {
    aff1[0][i] = a.as1[(size_t)b * K + i];   // already / 6 (GnFinalizeArgs::post_scale)
    aff1[1][i] = a.ab1[(size_t)b * K + i];
  }
  float s1[NBW], s2[NBW];
#pragma unroll
  for (int j = 0; j < NBW; ++j) s1[j] = s2[j] = 0.f;
  // POOL: aff2 of this lane's channels (applied to acc = h1 / 6: shift / 6, clamp01), the border sums, and the position of the
  // next 16-pixel group: (index inside the image, index inside its row)
  constexpr int NP = POOL ? NBW : 1;
  float sc2[NP], sh2[NP], c0s[NP], cws[NP], r0s[NP], rhs[NP], kk[NP][4];
  const int w16 = a.W / 16, gbot = (a.H - 1) * w16;  // groups per image row; first group of the last row
  int gidx = 0, gcol = 0;
  if constexpr (POOL) {
#pragma unroll
    for (int j = 0; j < NBW; ++j) {
      const int c = (wave * NBW + j) * 32 + n;
      sc2[j] = a.as2[(size_t)b * a.Chid + c];
      sh2[j] = a.ab2[(size_t)b * a.Chid + c] * kSixth;
      c0s[j] = cws[j] = r0s[j] = rhs[j] = kk[j][0] = kk[j][1] = kk[j][2] = kk[j][3] = 0.f;
    }
    gidx = tile * (RP / 16);
    gcol = gidx % w16;
  }

  // cooperative load: vector v = tid + j*256 of a step -> pixel v / (2 KS), channel vector v % (2 KS)
  const int nsteps = RP / 128;
  const size_t p_first = (size_t)tile * RP;
  vec_t raw[KS];
  auto load = [&](int step) {
#pragma unroll
    for (int j = 0; j < KS; ++j) {
      const int v = tid + j * 256;
      const size_t pix = p_first + (size_t)step * 128 + v / (2 * KS);
      const int k = (v % (2 * KS)) * 8;
      raw[j] = k < a.c0 ? ld_vec<T>(x0 + pix * a.c0 + k) : ld_vec<T>(x1 + pix * a.c1 + (k - a.c0));
    }
  };
  load(0);
  wg_barrier();  // aff1 staged
  unsigned long long tk[5] = {}, t_prev = 0;
  auto stamp = [&](int slot) {
    if constexpr (STAMP) {
      __builtin_amdgcn_sched_barrier(0);
      const unsigned long long now = __builtin_amdgcn_s_memtime();
      __builtin_amdgcn_sched_barrier(0);
      if (slot >= 0) tk[slot] += now - t_prev;
      t_prev = now;
    }
  };
  stamp(-1);
  for (int step = 0; step < nsteps; ++step) {
    unsigned char* buf = sA[step & 1];
    if constexpr (STAMP) asm volatile("s_waitcnt vmcnt(0)" ::: "memory");
    stamp(0);
#pragma unroll
    for (int j = 0; j < KS; ++j) {
      const int v = tid + j * 256;
      const int k = (v % (2 * KS)) * 8;
      *reinterpret_cast<vec_t*>(buf + (v / (2 * KS)) * XP + k * 2) = activate8<T>(raw[j], &aff1[0][k], &aff1[1][k]);
    }
    if (step + 1 < nsteps) load(step + 1);
    stamp(1);
    wg_barrier();  // tile `step` complete; the other buffer (read during step - 1) is free for step + 1
    stamp(2);
#pragma unroll 1
    for (int pb = 0; pb < 4; ++pb) {
      vec_t af[KS];
#pragma unroll
      for (int s = 0; s < KS; ++s) af[s] = *reinterpret_cast<const vec_t*>(buf + (pb * 32 + n) * XP + (16 * s + 8 * h) * 2);
      // POOL: the block's two 16-pixel groups (accumulator registers 0..7 and 8..15): which border classes they touch.  All of it
      // follows from blockIdx and the loop counters, so it stays in scalar registers; nothing per lane is built out here
      bool left[2] = {false, false}, right[2] = {false, false}, top[2] = {false, false}, bot[2] = {false, false};
      bool edge[2] = {false, false};
      if constexpr (POOL) {
#pragma unroll
        for (int gi = 0; gi < 2; ++gi) {
          left[gi] = gcol == 0; right[gi] = gcol == w16 - 1;
          top[gi] = gidx < w16; bot[gi] = gidx >= gbot;
          edge[gi] = left[gi] || right[gi] || top[gi] || bot[gi];
          // no row counter: `row += wrapped` compiles to a VALU select and a v_readfirstlane in the middle of the epilogue
          ++gidx;
          gcol = gcol + 1 == w16 ? 0 : gcol + 1;
        }
      }
#pragma unroll
      for (int j = 0; j < NBW; ++j) {
        f32x16 acc;
#pragma unroll
        for (int r = 0; r < 16; ++r) acc[r] = 0.f;
#pragma unroll
        for (int s = 0; s < KS; ++s) acc = mfma16<T>(af[s], wf[j][s], acc);
        if constexpr (STAMP) {  // a read of the last accumulator register: the compiler waits for the MFMAs here
          asm volatile("" ::"s"(__builtin_amdgcn_readfirstlane(__float_as_int(acc[15]))));
          stamp(3);
        }
        if constexpr (POOL) {
          constexpr uint32_t ones = PackedOne<T>::lo | PackedOne<T>::hi;
          uint32_t pk[8];  // registers (2 i, 2 i + 1) = two neighbouring pixels
#pragma unroll
          for (int i = 0; i < 8; ++i) pk[i] = affine_clamp01_pack<T>(acc[2 * i], acc[2 * i + 1], sc2[j], sc2[j], sh2[j], sh2[j]);
          float gs[2];
#pragma unroll
          for (int gi = 0; gi < 2; ++gi) {
            gs[gi] = dot2_pk<T>(pk[4 * gi], ones, 0.f);
#pragma unroll
            for (int i = 1; i < 4; ++i) gs[gi] = dot2_pk<T>(pk[4 * gi + i], ones, gs[gi]);
            if (edge[gi]) {
              // Wave-uniform, and taken by one group in eight at W = 256.  The empty asm keeps it a branch: without it hipcc
              // if-converts these few accumulating instructions into selects that every group of every block then executes.
              asm volatile("" ::: "memory");
              // one-hot operands: this lane's first-column pixel of the group (offset 0: register 8 gi, lower half) and its
              // last-column pixel (offset 15: register 8 gi + 7, upper half)
              const uint32_t mc0 = (left[gi] && h == 0) ? PackedOne<T>::lo : 0u;
              const uint32_t mcw = (right[gi] && h == 1) ? PackedOne<T>::hi : 0u;
              c0s[j] = dot2_pk<T>(pk[4 * gi], mc0, c0s[j]);
              cws[j] = dot2_pk<T>(pk[4 * gi + 3], mcw, cws[j]);
              if (top[gi]) {
                r0s[j] += gs[gi];
                kk[j][0] = dot2_pk<T>(pk[4 * gi], mc0, kk[j][0]);
                kk[j][1] = dot2_pk<T>(pk[4 * gi + 3], mcw, kk[j][1]);
              }
              if (bot[gi]) {
                rhs[j] += gs[gi];
                kk[j][2] = dot2_pk<T>(pk[4 * gi], mc0, kk[j][2]);
                kk[j][3] = dot2_pk<T>(pk[4 * gi + 3], mcw, kk[j][3]);
              }
            }
          }
          s1[j] += gs[0] + gs[1];
          stamp(4);
          continue;
        }
        // packed fp32 (v_pk_add_f32 / v_pk_fma_f32: two values per instruction) -- this reduction, not the MFMAs, is what
        // the wave spends its issue slots on
        f32x2 t1 = {0.f, 0.f}, t2 = {0.f, 0.f};
#pragma unroll
        for (int r = 0; r < 16; r += 2) {
          const f32x2 v = {acc[r], acc[r + 1]};
          t1 += v;
          t2 = __builtin_elementwise_fma(v, v, t2);
        }
        s1[j] += t1[0] + t1[1];
        s2[j] += t2[0] + t2[1];
      }
    }
  }
  if constexpr (STAMP) {
    if (a.dbg && lane == 0) {
      const size_t wg = (size_t)blockIdx.z * gridDim.x + blockIdx.x;
      for (int i = 0; i < kXStamps; ++i) a.dbg[(wg * 4 + wave) * kXStamps + i] = i < 5 ? tk[i] : 0ull;
    }
  }
  // lane halves hold different pixel rows of the same channel; every wave owns its channels outright
  const int ntiles = P / RP;
  if constexpr (POOL) {
#pragma unroll
    for (int j = 0; j < NBW; ++j) {
      float v[9] = {s1[j], r0s[j], rhs[j], c0s[j], cws[j], kk[j][0], kk[j][1], kk[j][2], kk[j][3]};
#pragma unroll
      for (int i = 0; i < 9; ++i) v[i] += __shfl_xor(v[i], 32, 64);
      if (h == 0) {
        const int c = (wave * NBW + j) * 32 + n;
        float t = 0.f;
#pragma unroll
        for (int tap = 0; tap < 9; ++tap) {  // tap (ky, kx) reads pixel p + (ky - 1, kx - 1): p itself must leave the far border out
          const int ky = tap / 3, kx = tap % 3;
          float st = v[0];
          if (ky == 2) st -= v[1];
          if (ky == 0) st -= v[2];
          if (kx == 2) st -= v[3];
          if (kx == 0) st -= v[4];
          if (ky == 2 && kx == 2) st += v[5];
          if (ky == 2 && kx == 0) st += v[6];
          if (ky == 0 && kx == 2) st += v[7];
          if (ky == 0 && kx == 0) st += v[8];
          t = __builtin_fmaf((float)(T)(6.f * a.wd[tap * a.Chid + c]), st, t);
        }
        fixed_add(a.pool_tot + (size_t)b * a.Chid + c, t, kPoolFixScale);
      }
    }
    return;
  }
#pragma unroll
  for (int j = 0; j < NBW; ++j) {
    s1[j] += __shfl_xor(s1[j], 32, 64);
    s2[j] += __shfl_xor(s2[j], 32, 64);
    if (h == 0) {
      const int c = (wave * NBW + j) * 32 + n;
      a.stats[((size_t)(b * ntiles + tile) * 2 + 0) * a.Chid + c] = 6.f * s1[j];   // h1 = 6 W1 a'
      a.stats[((size_t)(b * ntiles + tile) * 2 + 1) * a.Chid + c] = 36.f * s2[j];
    }
  }
}
template <int KS, int NBW>
__global__ void __launch_bounds__(256, 2) expand_pool_stamp_kernel(const IrbxArgs a, const int RP) {
  expand_scan<half_t, KS, NBW, true, true>(a, RP);
}
template <typename T, int KS, int NBW>
__global__ void __launch_bounds__(256, 2) expand_stats_kernel(const IrbxArgs a, const int RP) {
  expand_scan<T, KS, NBW, false>(a, RP);
}
template <typename T, int KS, int NBW>
__global__ void __launch_bounds__(256, 2) expand_pool_kernel(const IrbxArgs a, const int RP) {
  expand_scan<T, KS, NBW, true>(a, RP);
}

// ---------------------------------------------------------------------------------------------
// (2) fused expand + norm2 / FiLM / ReLU6 + depthwise 3x3, as two kernels built from the same phases:
//   expand_dw_kernel          stores h2 and leaves the SE pool partials;
//   expand_dw_project_kernel  keeps h2 in the workgroup and runs the project GEMM (+ shortcut) as its tail.
constexpr int kXT_H = 8, kXT_W = 16;                 // output tile
constexpr int kXH_W = kXT_W + 2, kXH_H = kXT_H + 2;  // halo tile 10 x 18 = 180 pixels -> 6 blocks of 32
constexpr int kXNPX = kXH_W * kXH_H;
constexpr int kXNPB = 6;

// LDS image of the activated h1 tile: [pixel q][64 channels + 16 B pad].  Both users address it with lane = pixel and a
// fixed 16-byte channel slot (the expand epilogue's ds_write_b128, the depthwise MFMAs' ds_read_b128): the 144-byte
// pitch (36 dwords) spreads consecutive pixels over distinct bank groups for either instruction's lane grouping.
constexpr int SHP = 144;

// Dynamic LDS of both kernels, as byte offsets from its start (sH = 0), for the kernels and for the launchers:
//   [sH: (DBUF ? 2 : 1) x 192 x 144 B][sX: 192 x XP][wds: 10 x Chid T][aff2: 2 x Chid fp32][aff1: 2 x K fp32][red][tail]
//   expand_dw (PCO = 0):          red = 2 x 4 x 64 fp32, tail = the pool totals, KS x 64 int64, where they live in LDS (KS <= 4)
//   expand_dw_project (PCO > 0):  red = 4 x 2 x PCO fp32, tail = the gate table (Chid fp32) at 64 channels only: elsewhere the
//                                 gate is in the depthwise weights
struct IrbxLds { int sX, wds, aff2, aff1, red, tail, total; };
constexpr IrbxLds irbx_lds(int KS, int Chid, bool dbuf, int PCO) {
  IrbxLds l{};
  l.sX = (dbuf ? 2 : 1) * kXNPB * 32 * SHP;
  l.wds = l.sX + kXNPB * 32 * (16 * KS + 8) * 2;
  l.aff2 = l.wds + 10 * Chid * 2;
  l.aff1 = l.aff2 + 2 * Chid * 4;
  l.red = l.aff1 + 2 * 16 * KS * 4;
  l.tail = l.red + (PCO != 0 ? 8 * PCO : 2 * 256) * 4;
  l.total = l.tail + (PCO != 0 ? (KS == 4 ? Chid * 4 : 0) : (KS <= 4 ? KS * 64 * 8 : 0));
  return l;
}
constexpr size_t irbx_lds_bytes(int KS, int Chid, bool dbuf, int PCO) { return (size_t)irbx_lds(KS, Chid, dbuf, PCO).total; }
// 96 -> 32: 1 792 B short of what two workgroups per CU allow (256 B while the gate table was in LDS, profiles/r08/README.md)
static_assert(irbx_lds_bytes(6, 384, false, 32) == 80128 && irbx_lds_bytes(6, 384, false, 32) <= 80 * 1024, "expand_dw_project<6, 32>: two workgroups per CU");

// a thread's places: (n, h) in the 32x32 MFMAs of the expand phase, where wave (chb, pxg) owns channel half chb of the chunk
// and pixel blocks 3 pxg .. 3 pxg + 2; (li, g) in the 16x16 MFMAs of the depthwise phase and the project tail
struct IrbxLane { int tid, lane, wave, n, h, chb, pxg, li, g; };
__device__ __forceinline__ IrbxLane irbx_lane() {
  IrbxLane t;
  t.tid = threadIdx.x; t.lane = t.tid & 63; t.wave = t.tid >> 6;
  t.n = t.lane & 31; t.h = t.lane >> 5;
  t.chb = t.wave & 1; t.pxg = t.wave >> 1;
  t.li = t.lane & 15; t.g = t.lane >> 4;
  return t;
}

// STAMP = diagnostic build (llie_tune("irbx_stamp", 1) expand_dw, 3 expand_dw_project; fp16): s_memtime around the phases, summed
// per wave into a.dbg ([workgroup][wave][kXStamps] cycles; each body lists its slots); never used in production.
template <bool STAMP>
struct IrbxStamps {
  unsigned long long tk[kXStamps] = {}, t_prev = 0;
  __device__ __forceinline__ void operator()(int slot) {
    if constexpr (STAMP) {
      __builtin_amdgcn_sched_barrier(0);
      const unsigned long long now = __builtin_amdgcn_s_memtime();
      __builtin_amdgcn_sched_barrier(0);
      if (slot >= 0) tk[slot] += now - t_prev;
      t_prev = now;
    }
  }
  __device__ __forceinline__ void store(const IrbxArgs& a, const IrbxLane& t) {
    if constexpr (STAMP) {
      if (a.dbg && t.lane == 0) {
        const size_t wg = ((size_t)blockIdx.z * gridDim.y + blockIdx.y) * gridDim.x + blockIdx.x;
#pragma unroll
        for (int i = 0; i < kXStamps; ++i) a.dbg[(wg * 4 + t.wave) * kXStamps + i] = tk[i];
      }
    }
  }
};

// ---- per-workgroup constants: depthwise weights (packed T), affine tables of this image, in ONE memory round trip.  A workgroup
// with a short run of tiles (one tile at B = 16 on the 128 x 128 maps) does not amortise its prologue, and 2048 - 4096 workgroups
// per launch repeat it: as a loop over the 10 Chid weight slots -- a division by Chid, one or two loads, a wait, one 16-bit LDS
// write per iteration -- the staging alone was 5 / 10 / 15 dependent round trips per workgroup (profiles/r28/README.md).
// Chid = 64 KS (irbx_supported), so every trip count is known here and a thread owns fixed channels: tid & 127 and a share of the
// tap pairs at 128 channels (threads 0..127 pairs 0..2, threads 128..255 pairs 3..4), tid at 256, tid and tid + 256 at 384.  All
// loads of a thread go out before the first value is used -- its weights, ONE gate per channel, its table entries -- and none
// is predicated: a thread without a second channel, or past tap 8, loads from a clamped address and writes nothing (hipcc counts
// unpredicated loads exactly; the callers' x halo and W1 loads, issued before these, complete under the same wait).
// GATEW: the image's SE gate is part of the staged depthwise weights; GTAB: it is staged as a table [Chid] at gate_s
template <typename T, int KS, bool GATEW, bool GTAB>
__device__ __forceinline__ void irbx_stage_constants(const IrbxArgs& a, const int b, const int tid, T* wds, float* aff2, float* aff1,
                                                     float* gate_s, unsigned char* sX) {
  constexpr int K = 16 * KS, XP = (K + 8) * 2, Chid = 64 * KS;
  constexpr bool SPLIT = Chid < 256;                // two threads per channel
  constexpr int NCH = SPLIT ? 1 : (Chid + 255) / 256;  // channels per thread
  constexpr int NPR = SPLIT ? 3 : 5;                // tap pairs per thread
  const int part = SPLIT ? tid >> 7 : 0;            // wave-uniform
  const int p0 = NPR * part;
  float wv[NCH][NPR][2], gv[NCH], s2v[NCH], b2v[NCH];
#pragma unroll
  for (int k = 0; k < NCH; ++k) {
    const int c = (SPLIT ? tid & 127 : tid) + 256 * k, cl = c < Chid ? c : c - 256;
#pragma unroll
    for (int j = 0; j < NPR; ++j)
#pragma unroll
      for (int t = 0; t < 2; ++t) {
        const int tap = 2 * (p0 + j) + t;
        if (SPLIT || tap < 9) wv[k][j][t] = a.wd[(tap < 9 ? tap : 8) * Chid + cl];
        else wv[k][j][t] = 0.f;
      }
  }
#pragma unroll
  for (int k = 0; k < NCH; ++k) {
    const int c = (SPLIT ? tid & 127 : tid) + 256 * k, cl = c < Chid ? c : c - 256;
    gv[k] = (GATEW || GTAB) ? a.gate[(size_t)b * Chid + cl] : 1.f;
    s2v[k] = a.as2[(size_t)b * Chid + cl];
    b2v[k] = a.ab2[(size_t)b * Chid + cl];
  }
  // aff1 [2][K]: scale, then shift.  Every thread takes an entry (the threads past 2 K one that another thread has too) and writes
  // it: a load that only a predicated block uses is sunk into that block by hipcc, behind the waits -- a round trip of its own
  const int i1 = tid % (2 * K);
  float v1 = i1 < K ? a.as1[(size_t)b * K + i1] : a.ab1[(size_t)b * K + i1 - K];
  // Everything is in flight; every value is named here, outside any predicated block, so that hipcc neither sinks a load into the
  // block that uses it (behind the waits of the blocks before) nor starts converting between two loads
  __builtin_amdgcn_sched_barrier(0);
#pragma unroll
  for (int k = 0; k < NCH; ++k) {
#pragma unroll
    for (int j = 0; j < NPR; ++j) asm volatile("" : "+v"(wv[k][j][0]), "+v"(wv[k][j][1]));
    asm volatile("" : "+v"(gv[k]), "+v"(s2v[k]), "+v"(b2v[k]));
  }
  asm volatile("" : "+v"(v1));

  // [tap pair][channel][2]: one dword = this channel's weights of taps 2 p and 2 p + 1 (tap 9 = 0); the tile in LDS holds relu6(.) / 6
  uint32_t* wpair = reinterpret_cast<uint32_t*>(wds);
#pragma unroll
  for (int k = 0; k < NCH; ++k) {
    const int c = (SPLIT ? tid & 127 : tid) + 256 * k;
    if (k > 0 && c >= Chid) continue;  // 384 channels: threads 128..255 have no second channel
#pragma unroll
    for (int j = 0; j < NPR; ++j) {
      const int p = p0 + j;
      if (p >= 5) continue;  // (128 channels: the sixth pair of the upper threads)
      // GATEW: times the image's SE gate -- a constant per (image, channel) like the weight itself: the fp32 product is rounded to
      // T once, where 6 w alone was rounded, and the chunk tail has no gate to apply
      T o[2];
#pragma unroll
      for (int t = 0; t < 2; ++t) {
        if constexpr (GATEW) o[t] = (T)(6.f * wv[k][j][t] * gv[k]);
        else o[t] = (T)(6.f * wv[k][j][t]);
        // One conversion per value, each with its multiply (in fp16 a v_fma_mixlo_f16), as when the slots were written one by
        // one: left to itself hipcc converts the pair with one v_cvt_pk_f16_f32 behind separate multiplies, and the staged
        // weights then differ from the one-by-one form in a few last bits per launch (profiles/r28/README.md, section 4)
        asm volatile("" : "+v"(o[t]));
      }
      if (p == 4) o[1] = (T)0.f;
      static_assert(sizeof(T) == 2, "two values per dword");
      const uint32_t lo = *reinterpret_cast<const unsigned short*>(&o[0]), hi = *reinterpret_cast<const unsigned short*>(&o[1]);
      wpair[p * Chid + c] = lo | (hi << 16);
    }
    if (!SPLIT || part == 0) {
      aff2[c] = s2v[k];                   // applied to acc' = acc / 6: scale unchanged,
      if constexpr (GTAB) gate_s[c] = gv[k];
    }
    if (!SPLIT || part == 1) aff2[Chid + c] = b2v[k] * kSixth;  // shift / 6, result clamped to [0, 1]
  }
  aff1[i1] = v1;                          // already / 6 (GnFinalizeArgs::post_scale)
  // pixels 180..191 of the last MFMA block do not exist: their operand rows stay zero
  for (int i = tid; i < (kXNPB * 32 - kXNPX) * (XP / 16); i += 256)
    *reinterpret_cast<u32x4*>(sX + kXNPX * XP + i * 16) = u32x4{0u, 0u, 0u, 0u};
}

// the workgroup's run of tiles [first, last) out of the image's `per_image`.  tiles_per_wg > 0: fixed runs; <= 0: the image's
// tiles split evenly over the gridDim.x workgroups (knob "irbx_grid")
struct IrbxTiles { int first, last, per_image; };
__device__ __forceinline__ IrbxTiles irbx_tiles(const IrbxArgs& a, const int tiles_per_wg) {
  IrbxTiles r;
  r.per_image = (a.W / kXT_W) * (a.H / kXT_H);
  r.first = tiles_per_wg > 0 ? blockIdx.x * tiles_per_wg : (int)(blockIdx.x * (unsigned)r.per_image / gridDim.x);
  const int end = tiles_per_wg > 0 ? r.first + tiles_per_wg : (int)((blockIdx.x + 1) * (unsigned)r.per_image / gridDim.x);
  r.last = end < r.per_image ? end : r.per_image;
  return r;
}
// tile (ty, tx) touches the image border: its halo needs bounds checks and zero padding; interior tiles need neither
__device__ __forceinline__ bool irbx_border(const IrbxArgs& a, int ty, int tx, int tiles_x) {
  return ty == 0 || tx == 0 || ty == a.H / kXT_H - 1 || tx == tiles_x - 1;
}

// ---- the x halo tile: raw x of the 10 x 18 pixels in registers (`raw`), then norm1 + ReLU6 into sX as [pixel][K + 8 channels].
// thread -> (pixel xq0, 16-byte channel vector xkv); pass j covers pixel xq0 + j * QSTEP.  The channel vector -- hence the K
// segment, its base pointer and the norm1 table slice -- is the same in every pass and every tile.
template <typename T, int KS>
struct IrbxHalo {
  static constexpr int K = 16 * KS;
  static constexpr int XP = (K + 8) * 2;                        // sX pixel pitch in bytes (80 / 144 / 208 / 272: conflict-free ds_read_b128)
  static constexpr int QSTEP = 256 / (2 * KS);                  // 64 / 32 / 21 pixels per pass
  static constexpr int XTHR = QSTEP * 2 * KS;                   // threads that take part (252 of 256 at KS = 6)
  static constexpr int XPT = (kXNPX + QSTEP - 1) / QSTEP;       // passes: 3 / 6 / 9
  // next tile's x prefetched into registers at the top of the tile.  32 channels only: at 64 and 96 the registers are there (233 / 243
  // of 256, nothing spilled, still two workgroups per CU) but no launch got faster for it (profiles/r28/README.md, section 3)
  static constexpr bool PREF = KS <= 2;
  typedef typename Elem<T>::vec_t vec_t;
  // per-thread constants of the staging -- nothing in the tile loop divides
  int xq0, xk8, xc;
  bool xthr, xlast;
  const T* xb;       // + pixel * xc
  int xrel[XPT];     // pixel offset of pass j relative to the tile's first output pixel
  unsigned char* sxw;
  vec_t raw[XPT];

  __device__ __forceinline__ void init(const IrbxArgs& a, const T* x0, const T* x1, unsigned char* sX, const int tid) {
    const int xkv = tid % (2 * KS);
    xq0 = tid / (2 * KS); xk8 = xkv * 8;
    xthr = XTHR == 256 || tid < XTHR;
    const bool xseg1 = xk8 >= a.c0;
    xb = xseg1 ? x1 + (xk8 - a.c0) : x0 + xk8;
    xc = xseg1 ? a.c1 : a.c0;
    xlast = xthr && (XPT - 1) * QSTEP + xq0 < kXNPX;   // the last pass is partial
#pragma unroll
    for (int j = 0; j < XPT; ++j) {
      const int q = xq0 + j * QSTEP;
      xrel[j] = (q / kXH_W - 1) * a.W + (q % kXH_W - 1);
    }
    sxw = sX + xq0 * XP + xk8 * 2;
  }
  // (ty, tx) = tile coordinates; interior tiles need no bounds checks
  __device__ __forceinline__ void load(const IrbxArgs& a, int ty, int tx, int tiles_x) {
    const int pix0 = ty * kXT_H * a.W + tx * kXT_W;
    if (!irbx_border(a, ty, tx, tiles_x)) {
#pragma unroll
      for (int j = 0; j < XPT; ++j) {
        if (j < XPT - 1 ? xthr : xlast) raw[j] = ld_vec<T>(xb + (size_t)(pix0 + xrel[j]) * xc);
        else raw[j] = vec_t{};
      }
    } else {
#pragma unroll
      for (int j = 0; j < XPT; ++j) {
        const int q = xq0 + j * QSTEP;
        const int gy = ty * kXT_H - 1 + q / kXH_W, gx = tx * kXT_W - 1 + q % kXH_W;
        // outside the image: h1 is forced to zero there (irbx_halo_ok), the value is irrelevant
        if ((j < XPT - 1 ? xthr : xlast) && gy >= 0 && gy < a.H && gx >= 0 && gx < a.W) raw[j] = ld_vec<T>(xb + (size_t)(pix0 + xrel[j]) * xc);
        else raw[j] = vec_t{};
      }
    }
  }
  __device__ __forceinline__ void clear() {
#pragma unroll
    for (int j = 0; j < XPT; ++j) raw[j] = vec_t{};
  }
  // a' = relu6(norm1(raw)) / 6 into sX; aff1 = the image's norm1 table [2][K]
  __device__ __forceinline__ void activate(const float* aff1) {
#pragma unroll
    for (int j = 0; j < XPT; ++j) {
      if (j < XPT - 1 ? xthr : xlast)
        *reinterpret_cast<vec_t*>(sxw + j * QSTEP * XP) = activate8<T>(raw[j], aff1 + xk8, aff1 + K + xk8);
    }
  }
};
// validity of this lane's three halo pixels (zero padding of the depthwise input): border tiles only
__device__ __forceinline__ void irbx_halo_ok(const IrbxArgs& a, const IrbxLane& t, const bool border, const int y0, const int x0p, bool (&ok)[3]) {
  ok[0] = ok[1] = ok[2] = true;
  if (border) {
#pragma unroll
    for (int i = 0; i < 3; ++i) {
      const int q = (t.pxg * 3 + i) * 32 + t.n;
      const int gy = y0 - 1 + q / kXH_W, gx = x0p - 1 + q % kXH_W;
      ok[i] = q < kXNPX && gy >= 0 && gy < a.H && gx >= 0 && gx < a.W;
    }
  }
}

// ---- the expand phase of one 64-channel chunk: h1^T block (32 channels x 32 pixels) x 3 pixel blocks per wave, from sX into the
// h1 tile.  Weight slices (A operand) of a chunk.  They are always fetched one depthwise phase ahead and BEFORE that phase's stores: the
// wait in front of the MFMAs then leaves the (younger) stores in flight instead of draining them.
template <typename T, int KS>
__device__ __forceinline__ void irbx_load_wf(typename Elem<T>::vec_t (&wf)[KS], const T* w1, const int chunk, const IrbxLane& t) {
  constexpr int K = 16 * KS;
#pragma unroll
  for (int s = 0; s < KS; ++s) wf[s] = ld_vec<T>(w1 + (size_t)(chunk * 64 + t.chb * 32 + t.n) * K + 16 * s + 8 * t.h);
}
// epilogue of one 32-channel x 32-pixel accumulator block of the expand phase: aff2 + ReLU6, zero outside the image (the conv's
// padding), pack, exchange lane halves so that each lane owns 8 consecutive channels, two ds_write_b128 at dst (+ 16).
// (The MFMAs in front of it are written out in both kernel bodies: as one function with this epilogue they cost
// expand_dw_project_kernel<T, 2, 32>, which sits at its 168 registers, two spilled registers (8 bytes of scratch).)
template <typename T>
__device__ __forceinline__ void irbx_expand_store(const f32x16& acc, const f32x4 (&sc2)[4], const f32x4 (&sh2)[4], const bool border, const bool ok,
                                                  unsigned char* dst) {
  uint32_t pk[4][2];
#pragma unroll
  for (int g = 0; g < 4; ++g)
#pragma unroll
    for (int j = 0; j < 2; ++j)
      pk[g][j] = affine_clamp01_pack<T>(acc[4 * g + 2 * j], acc[4 * g + 2 * j + 1], sc2[g][2 * j], sc2[g][2 * j + 1],
                                        sh2[g][2 * j], sh2[g][2 * j + 1]);
  if (border) {  // tiles on the image border: zero padding of the depthwise input (uniform branch, most tiles skip it)
#pragma unroll
    for (int g = 0; g < 4; ++g)
#pragma unroll
      for (int j = 0; j < 2; ++j) pk[g][j] = ok ? pk[g][j] : 0u;
  }
  u32x4 lo, hi2;
#pragma unroll
  for (int j = 0; j < 2; ++j) {
    const u32x2 r02 = __builtin_amdgcn_permlane32_swap(pk[0][j], pk[2][j], false, false);
    const u32x2 r13 = __builtin_amdgcn_permlane32_swap(pk[1][j], pk[3][j], false, false);
    lo[j] = r02[0]; lo[2 + j] = r02[1];    // h=0: channels 0..7 of the block; h=1: channels 16..23
    hi2[j] = r13[0]; hi2[2 + j] = r13[1];  // h=0: channels 8..15;             h=1: channels 24..31
  }
  *reinterpret_cast<u32x4*>(dst) = lo;
  *reinterpret_cast<u32x4*>(dst + 16) = hi2;
}

// ---- depthwise 3x3 on the MFMA pipe.  The VALU is what these kernels run out of (a wave64 instruction costs a SIMD
// 4 cycles; 72 FMAs per 16 output bytes), the matrix pipe idles.  A depthwise tap is a diagonal matrix:
//   out[ch][px] += sum_k diag(w_tap)[ch][k] * in[k][px + tap]      (k over the block's channels, 16 per tap)
// the data operand is one ds_read_b128 per MFMA (lane = pixel, 8 channels), the weight operand this lane's weight
// masked into its diagonal position (4 v_and per step).  A few per cent of the MACs are useful, which still equals
// the VALU's rate -- on a pipe that was idle, for a quarter of the VALU instructions.
// Two taps per 16x16x32 MFMA: D[16 ch][16 px] += A[16 ch][k] B[k][16 px], k = 16 t + c (tap slot t, channel c of the
// 16-channel tile), in this order of k: lane (li = lane & 15, g = lane >> 4) holds k-slice g = tap slot g & 1, channels 8 (g >> 1) + j.
//   B: lane = output pixel li of one tile row; its 8 channels of the halo pixel under tap slot g & 1: ONE ds_read_b128,
//      address = row base + this lane's tap offset (odd and even lane quarters read different taps)
//   A: lane = channel li of the tile; its weight of tap slot g & 1 at element li & 7 if (g >> 1) == li >> 3, else 0
// (k = 16 t + c in MFMA order would put the channel half in g & 1: the 16-lane groups of a ds_read_b128 -- {0-3, 12-15,
// 20-27}, ... -- would then mix 8 pixels at channel slot s with 8 at slot s + 1 and collide two-way on the 144-byte
// pitch.  With the tap in g & 1 a group reads 16 pixels of ONE slot, 8 of them shifted by the tap distance (1 or 16
// pixels; equal addresses broadcast): conflict-free, 4 instead of 8 LDS cycles for each of the reads.)
// One data operand per MFMA, 640 matrix-pipe cycles per 64-channel chunk and wave (one tap per 32x32x16 MFMA, round 2's form,
// took 1 152).
// A wave owns ROWS output rows (ROWS pixel tiles) x CT 16-channel tiles, ROWS x CT = 8 accumulator tiles of 4 registers:
// 5 tap pairs (the last one half empty) x CT steps of ROWS MFMAs = 40 MFMAs of 16 cycles.  expand_dw: (4, 2), a channel half of
// the chunk (its body holds that instance written out, see there); the project tail: (2, 4), all 64 channels.
// The caller names its share: row group rg = rows ROWS rg .. of the tile, channel half = tiles CT half .. of the chunk; buf is the
// h1 tile in LDS, wds the staged weight pairs.
//   bbase = the lane's pixel li of the wave's first halo row in the h1 tile, at its 16-byte slot (g >> 1) of the first channel tile
//   wpair = the lane's channel li of the first tile in the staged weight pairs
// dacc[c][r]: lane (pixel li of row r, g): channels 16 c + 4 g + e.
template <typename T, int ROWS, int CT>
__device__ __forceinline__ void irbx_dw_two_tap(f32x4 (&dacc)[CT][ROWS], const unsigned char* buf, const int rg, const int half, const T* wds,
                                                const int chunk, const int Chid, const IrbxLane& t) {
  typedef typename Elem<T>::vec_t vec_t;
  const int li = t.li, g = t.g;
  uint32_t amask[4];
#pragma unroll
  for (int d = 0; d < 4; ++d)
    amask[d] = (((li & 7) >> 1) == d && (g >> 1) == (li >> 3)) ? ((li & 1) ? 0xFFFF0000u : 0x0000FFFFu) : 0u;
  const uint32_t* wpair = reinterpret_cast<const uint32_t*>(wds) + chunk * 64 + half * (16 * CT) + li;  // + (pair * Chid + 16 c)
  const uint32_t wsel = (g & 1) ? 0x03020302u : 0x01000100u;  // v_perm_b32 selector: this lane quarter's tap, duplicated
#pragma unroll
  for (int c = 0; c < CT; ++c)
#pragma unroll
    for (int r = 0; r < ROWS; ++r) dacc[c][r] = f32x4{0.f, 0.f, 0.f, 0.f};
  const unsigned char* bbase = buf + ((ROWS * rg) * kXH_W + li) * SHP + (half * (2 * CT) + (g >> 1)) * 16;
  const bool upper = (g & 1) != 0;
  vec_t bf[2][ROWS];
  uint32_t wq[2];
  auto ld_step = [&](int step, vec_t (&bb)[ROWS], uint32_t& w2) {  // step = CT * pair + c
    const int pr = step / CT, c = step % CT;
    const int ta = 2 * pr, tb = 2 * pr + 1 < 9 ? 2 * pr + 1 : 8;
    const int offa = (ta / 3) * kXH_W + ta % 3, offb = (tb / 3) * kXH_W + tb % 3;
    const unsigned char* p0 = bbase + (upper ? offb : offa) * SHP + c * 32;
#pragma unroll
    for (int r = 0; r < ROWS; ++r) bb[r] = *reinterpret_cast<const vec_t*>(p0 + r * kXH_W * SHP);
    w2 = wpair[pr * Chid + 16 * c];
  };
  ld_step(0, bf[0], wq[0]);
#pragma unroll
  for (int step = 0; step < 5 * CT; ++step) {
    if (step + 1 < 5 * CT) ld_step(step + 1, bf[(step + 1) & 1], wq[(step + 1) & 1]);
    __builtin_amdgcn_sched_barrier(0);  // keep the look-ahead reads above this step's MFMAs
    const int c = step % CT;
    const uint32_t wdup = __builtin_amdgcn_perm(wq[step & 1], wq[step & 1], wsel);
    u32x4 m;
#pragma unroll
    for (int d = 0; d < 4; ++d) m[d] = wdup & amask[d];
    const vec_t af = reinterpret_cast<const vec_t&>(m);
#pragma unroll
    for (int r = 0; r < ROWS; ++r) dacc[c][r] = mfma16x16<T>(af, bf[step & 1][r], dacc[c][r]);
  }
}

// Two accumulator quads of one pixel -- lane (li, g): channels 4 g + e of 16-channel tiles c0 and c0 + 1 -- rounded to T and
// packed (p0, p1: two dwords each), then v_permlane16_swap between the two tiles gives every lane 8 consecutive channels of its
// pixel: even g: 4 g .. 4 g + 7, odd g: 16 + 4 (g - 1) .. 16 + 4 g + 3, i.e. channels irbx_choff(g) .. + 7 of the 32
__device__ __forceinline__ u32x4 irbx_swap8(const uint32_t (&p0)[2], const uint32_t (&p1)[2]) {
  const u32x2 s0 = __builtin_amdgcn_permlane16_swap(p0[0], p1[0], false, false);
  const u32x2 s1 = __builtin_amdgcn_permlane16_swap(p0[1], p1[1], false, false);
  return u32x4{s0[0], s1[0], s0[1], s1[1]};
}
template <typename T>
__device__ __forceinline__ u32x4 irbx_pack8_swap(const f32x4& q0, const f32x4& q1) {
  uint32_t p0[2], p1[2];
#pragma unroll
  for (int j = 0; j < 2; ++j) {
    typedef T t2 __attribute__((ext_vector_type(2)));
    t2 o0, o1;
    o0[0] = (T)q0[2 * j]; o0[1] = (T)q0[2 * j + 1];
    o1[0] = (T)q1[2 * j]; o1[1] = (T)q1[2 * j + 1];
    p0[j] = *reinterpret_cast<uint32_t*>(&o0);
    p1[j] = *reinterpret_cast<uint32_t*>(&o1);
  }
  return irbx_swap8(p0, p1);
}
__device__ __forceinline__ int irbx_choff(int g) { return 8 * (g >> 1) + 16 * (g & 1); }

// SE pool partial of expand_dw: channel sums over the wave's 64 pixels -- the 4 rows in registers, then the 16 pixel lanes of a row
// by DPP -- left by lane li = 0 of every row at red4 (its channels 4 g + e of the wave's two tiles)
__device__ __forceinline__ void irbx_pool_partial(const f32x4 (&dacc)[2][4], const int li, float* red4) {
  float v[8];
#pragma unroll
  for (int c2 = 0; c2 < 2; ++c2)
#pragma unroll
    for (int e = 0; e < 4; ++e) v[4 * c2 + e] = (dacc[c2][0][e] + dacc[c2][1][e]) + (dacc[c2][2][e] + dacc[c2][3][e]);
  // v += rotate(v) inside each 16-lane row, as ONE v_add_f32 with a DPP source per step (through
  // __builtin_amdgcn_update_dpp hipcc emits v_mov 0 + v_mov_dpp + add: 92 instructions for this reduction instead
  // of 32).  The eight values are stepped together, so a register written by one statement is read again eight
  // statements later: the VALU-write -> DPP-read hazard (2 wait states) needs no s_nop inside the strings.
#define LLIE_DPP_STEP(ROR)                                                                                               \
  _Pragma("unroll") for (int i = 0; i < 8; ++i)                                                                          \
      asm volatile("v_add_f32_dpp %0, %0, %0 row_ror:" #ROR " row_mask:0xf bank_mask:0xf" : "+v"(v[i]));
  // the sums just written by ordinary VALU adds: 2 wait states before the first DPP read.  The eight values are operands of
  // the statement, so every add that produces them is scheduled ABOVE the nop (a bare volatile asm orders only against
  // other side effects, and hipcc's hazard recognizer does not look inside inline asm for the DPP read).
  asm volatile("s_nop 1" : "+v"(v[0]), "+v"(v[1]), "+v"(v[2]), "+v"(v[3]), "+v"(v[4]), "+v"(v[5]), "+v"(v[6]), "+v"(v[7]));
  LLIE_DPP_STEP(8)
  LLIE_DPP_STEP(4)
  LLIE_DPP_STEP(2)
  LLIE_DPP_STEP(1)
#undef LLIE_DPP_STEP
  if (li == 0) {  // channels 16 c2 + 4 g + e of the wave's block
    float* rp = red4;
    *reinterpret_cast<f32x4*>(rp) = f32x4{v[0], v[1], v[2], v[3]};
    *reinterpret_cast<f32x4*>(rp + 16) = f32x4{v[4], v[5], v[6], v[7]};
  }
}

// ---- expand_dw: h2 to HBM + SE pool partials.  DBUF: the h1 tile and `red` are double-buffered (one barrier per chunk);
// NTST = h2 leaves with non-temporal stores (IrbxArgs::nt).
// STAMP slots: 0 waiting for memory before a tile can start: prologue + x wait (the clock starts at kernel entry: entry -> "constants
// staged" barrier, then every tile's wait for its prefetched / loaded x tile, vmcnt), 1 activate + ds_write of the x tile, 2 next tile's loads issued
// + halo validity, 3 tile-top barrier, 4 pool flush behind it, 5 chunk-top barrier + flush (chunks after the first), 6 expand
// MFMAs + epilogue + ds_write, 7 barrier behind them, 8 depthwise phase incl. the h2 stores and the pool partial.
template <typename T, int KS, bool DBUF, bool STAMP, bool NTST>
__device__ __forceinline__ void expand_dw_body(const IrbxArgs& a, const int tiles_per_wg, const int chunks_per_wg) {
  constexpr int SH_BYTES = kXNPB * 32 * SHP;
  typedef typename Elem<T>::vec_t vec_t;
  typedef IrbxHalo<T, KS> Halo;
  extern __shared__ __align__(16) unsigned char smem[];
  const IrbxLds lds = irbx_lds(KS, a.Chid, DBUF, 0);
  unsigned char* sH = smem;
  unsigned char* sX = smem + lds.sX;
  T* wds = reinterpret_cast<T*>(smem + lds.wds);
  float* aff2 = reinterpret_cast<float*>(smem + lds.aff2);
  float* aff1 = reinterpret_cast<float*>(smem + lds.aff1);
  float* red = reinterpret_cast<float*>(smem + lds.red);
  // fixed-point pool totals of this workgroup's tiles, [chunk][channel 64]: in LDS rather than in 2 KS registers of every
  // thread -- this kernel sits exactly at an occupancy step, and a spilled register costs more than its scratch access:
  // every reload is a vector-memory operation whose wait (vmcnt is in order) also waits for the h2 stores in flight
  // (KS = 6 keeps them in registers: its 79 KB of LDS are two workgroups per CU only as long as nothing is added)
  constexpr bool PACC_LDS = KS <= 4;
  long long* pacc_lds = reinterpret_cast<long long*>(smem + lds.tail);
  long long pacc_reg[PACC_LDS ? 1 : KS];

  const IrbxLane t = irbx_lane();
  const int tid = t.tid, n = t.n, h = t.h, chb = t.chb, pxg = t.pxg, li = t.li, g = t.g;
  const int b = blockIdx.z;
  const int tiles_x = a.W / kXT_W;
  const int P = a.H * a.W;
  const T* x0 = reinterpret_cast<const T*>(a.x0) + (size_t)b * P * a.c0;
  const T* x1 = a.x1 ? reinterpret_cast<const T*>(a.x1) + (size_t)b * P * a.c1 : nullptr;
  const T* w1 = reinterpret_cast<const T*>(a.w1);
  T* out = reinterpret_cast<T*>(a.out) + (size_t)b * P * a.Chid;
  const int chunk0 = blockIdx.y * chunks_per_wg;
  const int nchunks_all = a.Chid / 64;
  const int chunk1 = chunk0 + chunks_per_wg < nchunks_all ? chunk0 + chunks_per_wg : nchunks_all;

  IrbxStamps<STAMP> stamp;
  stamp(-1);  // the clock starts at kernel entry: slot 0 takes the prologue
  // The prologue is one memory round trip: what the first tile needs goes out first -- its x halo (at every width: raw[] is live
  // through the prologue only, where nothing else is), the expand weights of the first chunk -- then the constants, and the first
  // wait is the one in front of the constants' LDS writes.
  const IrbxTiles run = irbx_tiles(a, tiles_per_wg);
  Halo halo;
  halo.init(a, x0, x1, sX, tid);
  int ty = run.first / tiles_x, tx = run.first % tiles_x;   // the only division: once per workgroup
  if (run.first < run.last) halo.load(a, ty, tx, tiles_x);
  vec_t wf[KS];
  irbx_load_wf<T, KS>(wf, w1, chunk0, t);
  irbx_stage_constants<T, KS, false, false>(a, b, tid, wds, aff2, aff1, nullptr, sX);
  wg_barrier();  // constants staged
  stamp(0);
  const bool has_pool = a.pool != nullptr || a.pool_tot != nullptr;
  int par = 0;  // sH / red buffer parity (DBUF)
  int pend_tile = -1, pend_chunk = 0, pend_par = 0;  // pool partial waiting for its cross-wave sum
  if constexpr (PACC_LDS) {
    if (tid < 64) {  // threads 0..63 own channel tid of every chunk (Chid / 64 = KS chunks at most); only they touch it
#pragma unroll
      for (int q = 0; q < KS; ++q) pacc_lds[q * 64 + tid] = 0;
    }
  } else {
#pragma unroll
    for (int q = 0; q < KS; ++q) pacc_reg[q] = 0;
  }
  auto flush_pool = [&]() {  // after a barrier that follows the depthwise phase which wrote red[pend_par]
    if (pend_tile >= 0 && tid < 64) {
      const float* r = red + pend_par * 256;  // wave (chb, pxg) = chb + 2 pxg left its 32 channel sums at [wave * 64 + channel]
      const int cbb = tid >> 5, ci = tid & 31;
      const float s = r[cbb * 64 + ci] + r[(cbb + 2) * 64 + ci];
      if (a.pool_tot) {  // fixed-point, summed over this workgroup's tiles in registers: one global atomic per chunk at the end
        const long long v = __float2ll_rn(s * kPoolFixScale);
        if constexpr (PACC_LDS) {
          pacc_lds[(pend_chunk - chunk0) * 64 + tid] += v;
        } else {
#pragma unroll
          for (int q = 0; q < KS; ++q) pacc_reg[q] += (pend_chunk - chunk0 == q) ? v : 0ll;
        }
      } else {
        a.pool[((size_t)b * run.per_image + pend_tile) * a.Chid + pend_chunk * 64 + tid] = s;
      }
    }
    pend_tile = -1;
  };

  for (int tile = run.first; tile < run.last; ++tile) {
    const int y0 = ty * kXT_H, x0p = tx * kXT_W;
    int tyn = ty, txn = tx + 1;  // the next tile of the run
    if (txn == tiles_x) { txn = 0; ++tyn; }
    // ---- activate this tile's x (norm1 + ReLU6) into sX, prefetch the next tile.  Every wave is past the last
    // MFMA phase of the previous tile here (the barrier that follows it), so sX is free.
    // Every vector-memory operation so far has to be complete here anyway (raw[] below is older than all of them), but the
    // compiler's wait sits inside the predicated block below; said unconditionally, the chunk loop is entered with nothing
    // pending, and the wait for the prefetched weight slices at its head becomes vmcnt(4 + ...) -- the depthwise phase's four
    // h2 stores stay in flight -- instead of the vmcnt(0) that the merge with this path forced.
    __builtin_amdgcn_s_waitcnt(0x0F70);  // vmcnt(0)
    stamp(0);
    halo.activate(aff1);
    stamp(1);
    if (Halo::PREF && tile + 1 < run.last) halo.load(a, tyn, txn, tiles_x);
    const bool border = irbx_border(a, ty, tx, tiles_x);
    bool ok[3];
    irbx_halo_ok(a, t, border, y0, x0p, ok);
    stamp(2);
    wg_barrier();
    stamp(3);
    if (!DBUF) flush_pool();
    stamp(4);
    // (Unrolling this loop lets hipcc count the memory operations between a prefetch and its use -- vmcnt(5) instead of
    // vmcnt(2) for the weight slices -- but costs 11 spilled registers, and every spill reload waits vmcnt(0), i.e. for the
    // h2 stores in flight: 35.7 vs 34.7 ms per step.  The run-time loop stays.)
#pragma unroll 1
    for (int chunk = chunk0; chunk < chunk1; ++chunk) {
      unsigned char* buf = sH + (DBUF ? par * SH_BYTES : 0);
      if (!DBUF && chunk > chunk0) {
        wg_barrier();  // previous depthwise phase done with sH
        flush_pool();
        stamp(5);
      }
      // ---- MFMA: h1^T block (32 channels x 32 pixels) x 3 pixel blocks
      const int ch0 = chunk * 64 + chb * 32;
      // aff2 of this lane's 16 accumulator channels: ch0 + 8g + 4h + e
      f32x4 sc2[4], sh2[4];
#pragma unroll
      for (int g = 0; g < 4; ++g) {
        sc2[g] = *reinterpret_cast<const f32x4*>(aff2 + ch0 + 8 * g + 4 * h);
        sh2[g] = *reinterpret_cast<const f32x4*>(aff2 + a.Chid + ch0 + 8 * g + 4 * h);
      }
      // accumulators in flight: all three pixel blocks, or one at a time (registers)
      constexpr int NACC = KS <= 2 ? 3 : 1;
      f32x16 accs[NACC];
      if constexpr (NACC == 3) {
#pragma unroll
        for (int i = 0; i < 3; ++i) {
          const int q = (pxg * 3 + i) * 32 + n;
#pragma unroll
          for (int r = 0; r < 16; ++r) accs[i][r] = 0.f;
#pragma unroll
          for (int s = 0; s < KS; ++s)
            accs[i] = mfma16<T>(wf[s], *reinterpret_cast<const vec_t*>(sX + q * Halo::XP + (16 * s + 8 * h) * 2), accs[i]);
        }
        irbx_load_wf<T, KS>(wf, w1, chunk + 1 < chunk1 ? chunk + 1 : chunk0, t);  // next chunk (or the next tile's first): see irbx_load_wf
      }
#pragma unroll
      for (int i = 0; i < 3; ++i) {
        const int q = (pxg * 3 + i) * 32 + n;
        if constexpr (NACC == 1) {
#pragma unroll
          for (int r = 0; r < 16; ++r) accs[0][r] = 0.f;
#pragma unroll
          for (int s = 0; s < KS; ++s)
            accs[0] = mfma16<T>(wf[s], *reinterpret_cast<const vec_t*>(sX + q * Halo::XP + (16 * s + 8 * h) * 2), accs[0]);
          if (i == 2) irbx_load_wf<T, KS>(wf, w1, chunk + 1 < chunk1 ? chunk + 1 : chunk0, t);
        }
        const f32x16 acc = accs[NACC == 3 ? i : 0];
        irbx_expand_store<T>(acc, sc2, sh2, border, ok[i], buf + q * SHP + (chb * 4 + 2 * h) * 16);
      }
      stamp(6);
      wg_barrier();
      if (DBUF) flush_pool();
      stamp(7);
      // ---- depthwise (irbx_dw_two_tap explains it): the wave's 32 channels (2 tiles) x its 4 output rows.  Written out here:
      // irbx_dw_two_tap<T, 4, 2> is the same IR in another order, and hipcc's schedule of this kernel then takes 168 registers
      // instead of 165 at 32 channels -- all that three workgroups per CU allow -- and 207 instead of 198 at 96.
      uint32_t amask[4];
#pragma unroll
      for (int d = 0; d < 4; ++d)
        amask[d] = (((li & 7) >> 1) == d && (g >> 1) == (li >> 3)) ? ((li & 1) ? 0xFFFF0000u : 0x0000FFFFu) : 0u;
      const uint32_t* wpair = reinterpret_cast<const uint32_t*>(wds) + chunk * 64 + chb * 32 + li;  // + (pair * Chid + 16 c2)
      const uint32_t wsel = (g & 1) ? 0x03020302u : 0x01000100u;  // v_perm_b32 selector: this lane quarter's tap, duplicated
      f32x4 dacc[2][4];
#pragma unroll
      for (int c2 = 0; c2 < 2; ++c2)
#pragma unroll
        for (int r = 0; r < 4; ++r) dacc[c2][r] = f32x4{0.f, 0.f, 0.f, 0.f};
      const unsigned char* bbase = buf + ((4 * pxg) * kXH_W + li) * SHP + (chb * 4 + (g >> 1)) * 16;
      const bool upper = (g & 1) != 0;
      vec_t bf[2][4];
      uint32_t wq[2];
      auto ld_step = [&](int step, vec_t (&bb)[4], uint32_t& w2) {  // step = 2 * pair + c2
        const int pr = step >> 1, c2 = step & 1;
        const int ta = 2 * pr, tb = 2 * pr + 1 < 9 ? 2 * pr + 1 : 8;
        const int offa = (ta / 3) * kXH_W + ta % 3, offb = (tb / 3) * kXH_W + tb % 3;
        const unsigned char* p0 = bbase + (upper ? offb : offa) * SHP + c2 * 32;
#pragma unroll
        for (int r = 0; r < 4; ++r) bb[r] = *reinterpret_cast<const vec_t*>(p0 + r * kXH_W * SHP);
        w2 = wpair[pr * a.Chid + 16 * c2];
      };
      ld_step(0, bf[0], wq[0]);
#pragma unroll
      for (int step = 0; step < 10; ++step) {
        if (step + 1 < 10) ld_step(step + 1, bf[(step + 1) & 1], wq[(step + 1) & 1]);
        __builtin_amdgcn_sched_barrier(0);  // keep the look-ahead reads above this step's MFMAs
        const int c2 = step & 1;
        const uint32_t wdup = __builtin_amdgcn_perm(wq[step & 1], wq[step & 1], wsel);
        u32x4 m;
#pragma unroll
        for (int d = 0; d < 4; ++d) m[d] = wdup & amask[d];
        const vec_t af = reinterpret_cast<const vec_t&>(m);
#pragma unroll
        for (int r = 0; r < 4; ++r) dacc[c2][r] = mfma16x16<T>(af, bf[step & 1][r], dacc[c2][r]);
      }
      const int choff = irbx_choff(g);
#pragma unroll
      for (int r = 0; r < 4; ++r) {
        const u32x4 v = irbx_pack8_swap<T>(dacc[0][r], dacc[1][r]);
        const int orow = 4 * t.pxg + r;
        T* op = out + ((size_t)(y0 + orow) * a.W + x0p + li) * a.Chid + chunk * 64 + t.chb * 32 + choff;
        if constexpr (NTST) __builtin_nontemporal_store(v, reinterpret_cast<u32x4*>(op));
        else *reinterpret_cast<u32x4*>(op) = v;
      }
      if (has_pool) {
        irbx_pool_partial(dacc, li, red + (DBUF ? par : 0) * 256 + t.wave * 64 + 4 * g);
        pend_tile = tile; pend_chunk = chunk; pend_par = DBUF ? par : 0;
      }
      if (DBUF) par ^= 1;
      stamp(8);
    }
    if constexpr (!Halo::PREF) {  // no registers to hold it under the tile: waited for at once
      if (tile + 1 < run.last) halo.load(a, tyn, txn, tiles_x);
      else halo.clear();  // (so that raw[] is not live around the loop)
    }
    ty = tyn; tx = txn;
  }
  stamp.store(a, t);
  if (has_pool) {
    wg_barrier();
    flush_pool();
    if (a.pool_tot && tid < 64) {
#pragma unroll
      for (int q = 0; q < KS; ++q)
        if (chunk0 + q < chunk1) atomicAdd(a.pool_tot + (size_t)b * a.Chid + (chunk0 + q) * 64 + tid, (unsigned long long)(PACC_LDS ? pacc_lds[q * 64 + tid] : pacc_reg[PACC_LDS ? 0 : q]));
    }
  }
}

// ---- the tile epilogue of expand_dw_project: y = round(yacc) stored, y's GroupNorm partials of the wave into red[wave][2][PCO]
template <typename T, int PCO>
__device__ __forceinline__ void irbx_project_store_y(const IrbxArgs& a, const IrbxLane& t, const f32x4 (&yacc)[2][PCO / 16], const int b, const int y0,
                                                     const int x0p, float* red) {
  constexpr int NCB = PCO / 16;
  const int wave = t.wave, li = t.li, g = t.g;
  const int P = a.H * a.W;
  // ---- y = round(acc) for the wave's 2 rows x 16 pixels (the shortcut is in acc since the top of the tile): lane (pixel li, g)
  // holds rows 16 cb + 4 g + e of every block cb
  const int choff = irbx_choff(g);
  T* yout = reinterpret_cast<T*>(a.y) + (size_t)b * P * PCO;
  float st[2][NCB * 4];  // (sum, sum of squares) of the rounded outputs, this lane's 2 pixels
#pragma unroll
  for (int i = 0; i < NCB * 4; ++i) st[0][i] = st[1][i] = 0.f;
#pragma unroll
  for (int r = 0; r < 2; ++r) {
    const size_t pix = (size_t)(y0 + 2 * wave + r) * a.W + x0p + li;
    uint32_t pk[NCB][2];  // rounded here, not in irbx_pack8_swap: the statistics are those of the rounded values
#pragma unroll
    for (int cb = 0; cb < NCB; ++cb) {
      typedef T t2 __attribute__((ext_vector_type(2)));
#pragma unroll
      for (int j = 0; j < 2; ++j) {
        t2 o;
#pragma unroll
        for (int e = 0; e < 2; ++e) {
          o[e] = (T)yacc[r][cb][2 * j + e];
          const float q = (float)o[e];
          st[0][4 * cb + 2 * j + e] += q;
          st[1][4 * cb + 2 * j + e] = __builtin_fmaf(q, q, st[1][4 * cb + 2 * j + e]);
        }
        pk[cb][j] = *reinterpret_cast<uint32_t*>(&o);
      }
    }
#pragma unroll
    for (int pp = 0; pp < NCB / 2; ++pp)
      *reinterpret_cast<u32x4*>(yout + pix * PCO + 32 * pp + choff) = irbx_swap8(pk[2 * pp], pk[2 * pp + 1]);
  }
  // Sums over the 16 pixel lanes of a row, sixteen values at a time, as a transposing reduction: a step halves the values a
  // lane carries -- the lane keeps one half and adds its partner's copy of that half, the partner keeps the other -- so the
  // steps cost 16 + 8 adds and leave lane quad k = li >> 2 with the sums of values 4 k .. 4 k + 3 over four lanes each; two
  // butterfly steps inside the quad (4 + 4 adds) finish them: 32 adds instead of 4 x 16.  The partner is the mirrored lane
  // (li ^ 15, then li ^ 7), and which half a lane writes is the DPP bank mask (banks = lane quads of a row): the first add of a
  // pair completes the half kept in place, the second builds the other half from the upper registers into the lower ones.
  // As in the pool partial of expand_dw the adds are single v_add_f32 with a DPP source, written out because the
  // builtin costs three instructions each, and a register written by one statement is read by DPP four or more statements
  // later (2 wait states needed); s_nop 1 covers the ordinary VALU writes in front.  The order is fixed: the slab stays
  // bitwise independent of the batch and the schedule.
#pragma unroll
  for (int grp = 0; grp < NCB / 2; ++grp) {
    // PCO = 32: (which, cb, e) = (j >> 3, (j >> 2) & 1, j & 3); PCO = 64, 128: which = grp / (NCB / 4), blocks cb = cb0 + (j >> 2), e = j & 3
    constexpr int GPW = NCB >= 4 ? NCB / 4 : 1;  // groups per `which`
    const int cb0 = 4 * (grp % GPW);
    float v[16];
#pragma unroll
    for (int j = 0; j < 16; ++j) {
      if constexpr (NCB == 2) v[j] = st[j >> 3][j & 7];
      else v[j] = st[grp / GPW][4 * cb0 + j];
    }
    asm volatile("s_nop 1" : "+v"(v[0]), "+v"(v[1]), "+v"(v[2]), "+v"(v[3]), "+v"(v[4]), "+v"(v[5]), "+v"(v[6]), "+v"(v[7]),
                             "+v"(v[8]), "+v"(v[9]), "+v"(v[10]), "+v"(v[11]), "+v"(v[12]), "+v"(v[13]), "+v"(v[14]), "+v"(v[15]));
#define LLIE_DPP_HALVE(N, CTRL, KEEP, TAKE)                                                                                  \
  _Pragma("unroll") for (int i = 0; i < N; ++i)                                                                              \
      asm volatile("v_add_f32_dpp %0, %0, %0 " CTRL " row_mask:0xf bank_mask:" KEEP : "+v"(v[i]));                           \
  _Pragma("unroll") for (int i = 0; i < N; ++i)                                                                              \
      asm volatile("v_add_f32_dpp %0, %1, %1 " CTRL " row_mask:0xf bank_mask:" TAKE : "+v"(v[i]) : "v"(v[i + N]));
#define LLIE_DPP_STEP(CTRL)                                                                                                  \
  _Pragma("unroll") for (int i = 0; i < 4; ++i)                                                                              \
      asm volatile("v_add_f32_dpp %0, %0, %0 " CTRL " row_mask:0xf bank_mask:0xf" : "+v"(v[i]));
    LLIE_DPP_HALVE(8, "row_mirror", "0x3", "0xc")        // lanes 0..7 keep values 0..7, lanes 8..15 take 8..15
    LLIE_DPP_HALVE(4, "row_half_mirror", "0x5", "0xa")   // quads 0 and 2 keep values 0..3 of theirs, quads 1 and 3 take 4..7
    LLIE_DPP_STEP("quad_perm:[2,3,0,1]")
    LLIE_DPP_STEP("quad_perm:[1,0,3,2]")
#undef LLIE_DPP_HALVE
#undef LLIE_DPP_STEP
    if ((li & 3) == 0) {  // red[wave][which][channel 16 cb + 4 g + e]: quad k of the row holds (which, cb) = (k >> 1, k & 1) or (grp, k)
      const int k = li >> 2;
      const int which = NCB == 2 ? k >> 1 : grp / GPW, cb = NCB == 2 ? k & 1 : cb0 + k;
      *reinterpret_cast<f32x4*>(red + (wave * 2 + which) * PCO + 16 * cb + 4 * g) = f32x4{v[0], v[1], v[2], v[3]};
    }
  }
}

// ---- expand_dw_project: the project GEMM of the block as the tail, PCO = Cout.  h2 never leaves the workgroup: a wave owns two
// output rows and ALL 64 channels of the chunk in the depthwise phase (instead of four rows and 32 channels), so after the same
// permlane16 swap that feeds expand_dw's h2 stores a lane holds 8 consecutive channels of one pixel -- a B fragment of a 16x16x32
// MFMA whose A fragment is 16 rows of Wp.  No pool work here: the SE gate is already known (expand_pool_kernel), a constant per
// (image, channel), and a workgroup serves one image, so the gate is part of the depthwise weights it stages, T(6 w gate): the
// accumulators of the depthwise phase are gate * h2 and the chunk tail has nothing to multiply (expand_pool keeps T(6 w): its
// totals are what the gate is computed from; and so does the 64-channel form here, which keeps the gate as a table in LDS and
// multiplies the fp32 accumulators: GATEW below).  y[32 pixels][PCO] accumulates in fp32 over the chunks (PCO / 2 registers) and
// STARTS as the shortcut -- the raw x of the centre pixels, loaded before the tile-top barrier together with the next tile's
// prefetch -- so the tile's epilogue only rounds to T, stores y and leaves y's GroupNorm partials as the tile's slab entry.
// PCO != K (96 -> 32): the block has a skip conv instead of the identity shortcut, and its input may be a virtual concat.  Wp is
// then the engine's K-concatenated matrix [PCO][Chid + K] (row stride IrbxArgs::ldp), project columns first: the chunk tail reads
// the project columns as before, and y starts as Wskip . x on the raw centre pixels: K / 32 k-steps at the top of the tile (no
// norm, no activation: the skip segments of pw_gemm), their operands loaded before the tile-top barrier.
// STAMP slots: 0 waiting for memory before a tile can start: prologue + x wait (the clock starts at kernel entry: entry -> "constants
// staged" barrier, then every tile's wait for its x tile, vmcnt), 1 activate + ds_write + the next tile's and the shortcut's loads issued + halo
// validity, 2 tile-top barrier + flush of y's statistics + the shortcut into the y accumulators, 3 chunk-top barrier (chunks after
// the first), 4 expand MFMAs + epilogue + ds_write, 5 barrier behind them, 6 depthwise steps until the last accumulator can be
// read, 7 pack + swap + project MFMAs issued (they complete under whatever follows), 8 the tile's epilogue: rounding, y's
// statistics, stores issued.
template <typename T, int KS, bool STAMP, int PCO>
__device__ __forceinline__ void expand_dw_project_body(const IrbxArgs& a, const int tiles_per_wg) {
  constexpr int K = 16 * KS;
  typedef typename Elem<T>::vec_t vec_t;
  typedef IrbxHalo<T, KS> Halo;
  constexpr bool PSKIP = PCO != K;  // skip conv in place of the identity shortcut
  // The image's SE gate is part of the staged depthwise weights (GATEW) -- except at 64 channels, where that measured no faster
  // than the gate table [Chid] in LDS behind `red`, applied to the accumulators in the chunk tail (profiles/r20/README.md), and
  // the table stays
  constexpr bool GATEW = KS != 4;
  static_assert(PCO > 0 && (PCO == K ? KS <= 4 : PCO % 32 == 0 && PCO <= 64),
                "project tail: single-buffered kernel; identity form at 32 and 64 channels, skip form to 32 or 64");
  constexpr int NCB = PCO / 16;  // 16-row blocks of Wp
  constexpr int NKS = PSKIP ? K / 32 : 1;
  extern __shared__ __align__(16) unsigned char smem[];
  const IrbxLds lds = irbx_lds(KS, a.Chid, false, PCO);
  unsigned char* buf = smem;  // sH, single-buffered
  unsigned char* sX = smem + lds.sX;
  T* wds = reinterpret_cast<T*>(smem + lds.wds);
  float* aff2 = reinterpret_cast<float*>(smem + lds.aff2);
  float* aff1 = reinterpret_cast<float*>(smem + lds.aff1);
  float* red = reinterpret_cast<float*>(smem + lds.red);  // the four waves' (sum, sum of squares) of y, 4 x 2 x PCO floats
  float* gate_s = reinterpret_cast<float*>(smem + lds.tail);

  const IrbxLane t = irbx_lane();
  const int tid = t.tid, wave = t.wave, n = t.n, h = t.h, chb = t.chb, pxg = t.pxg, li = t.li, g = t.g;
  const int b = blockIdx.z;
  const int tiles_x = a.W / kXT_W;
  const int P = a.H * a.W;
  const T* x0 = reinterpret_cast<const T*>(a.x0) + (size_t)b * P * a.c0;
  const T* x1 = a.x1 ? reinterpret_cast<const T*>(a.x1) + (size_t)b * P * a.c1 : nullptr;
  const T* w1 = reinterpret_cast<const T*>(a.w1);
  // every workgroup takes all KS = Chid / 64 channel chunks: y accumulates over them (the launch has gridDim.y = 1)
  const int chunk0 = blockIdx.y * KS;
  const int nchunks_all = a.Chid / 64;
  const int chunk1 = chunk0 + KS < nchunks_all ? chunk0 + KS : nchunks_all;

  IrbxStamps<STAMP> stamp;
  stamp(-1);  // the clock starts at kernel entry: slot 0 takes the prologue
  // one memory round trip: the first tile's x halo, the first chunk's expand weights, the constants (see expand_dw_body)
  const IrbxTiles run = irbx_tiles(a, tiles_per_wg);
  Halo halo;
  halo.init(a, x0, x1, sX, tid);
  int ty = run.first / tiles_x, tx = run.first % tiles_x;   // the only division: once per workgroup
  if (run.first < run.last) halo.load(a, ty, tx, tiles_x);
  vec_t wf[KS];
  irbx_load_wf<T, KS>(wf, w1, chunk0, t);
  irbx_stage_constants<T, KS, GATEW, !GATEW>(a, b, tid, wds, aff2, aff1, gate_s, sX);
  wg_barrier();  // constants staged
  stamp(0);
  int pend_tile = -1;  // tile whose y statistics wait in `red` for their cross-wave sum
  auto flush_ystats = [&]() {  // after a barrier that follows the tile epilogue which wrote `red`
    // y's statistics of the tile before: the four waves' (sum, sum of squares) [wave][2][PCO], added in wave order
    if (pend_tile >= 0 && tid < 2 * PCO) {
      const float s = (red[tid] + red[2 * PCO + tid]) + (red[4 * PCO + tid] + red[6 * PCO + tid]);
      a.ystats[((size_t)b * run.per_image + pend_tile) * 2 * PCO + tid] = s;
    }
    pend_tile = -1;
  };

  for (int tile = run.first; tile < run.last; ++tile) {
    const int y0 = ty * kXT_H, x0p = tx * kXT_W;
    int tyn = ty, txn = tx + 1;  // the next tile of the run
    if (txn == tiles_x) { txn = 0; ++tyn; }
    // ---- activate this tile's x (norm1 + ReLU6) into sX, prefetch the next tile.  Every wave is past the last
    // MFMA phase of the previous tile here (the barrier that follows it), so sX is free.
    // Every vector-memory operation so far has to be complete here anyway (raw[] below is older than all of them), but the
    // compiler's wait sits inside the predicated block below; said unconditionally, the chunk loop is entered with nothing
    // pending (see expand_dw_body).
    __builtin_amdgcn_s_waitcnt(0x0F70);  // vmcnt(0)
    stamp(0);
    halo.activate(aff1);
    // The shortcut's operands, for the wave's 2 rows x 16 pixels (lane = pixel li, quarter g): the raw x of the centre pixels,
    // rows 16 cb + 4 g + e of every block cb (identity form), or the K / 32 k-steps of the skip conv -- k-step ks covers input
    // channels 32 ks .. 32 ks + 31, lane (li, g) holds channels 32 ks + 8 g .. + 7 of row 16 cb + li of Wskip (A) and of pixel li
    // of the row (B); a 16-byte vector never straddles the segments (c0 % 16 == 0).  The tile's own loads have left x in L2.  They
    // go out here, ahead of the next tile's prefetch, and become the start of the y accumulators behind the tile-top barrier; the
    // staging registers (raw) are free by now.  (vmcnt counts in order, so the wait for them could leave the prefetch in flight;
    // hipcc's does not -- the prefetch loads are lane-predicated, it assumes none was issued and waits vmcnt(0) for the last
    // shortcut register: profiles/r20/README.md, section 1.)
    typedef T t4 __attribute__((ext_vector_type(4)));
    t4 res[2][NCB];
    vec_t wsf[NKS][NCB], xsv[NKS][2];
#pragma unroll
    for (int r = 0; r < 2; ++r) {
      const size_t pix = (size_t)(y0 + 2 * wave + r) * a.W + x0p + li;
      if constexpr (!PSKIP) {
#pragma unroll
        for (int cb = 0; cb < NCB; ++cb) res[r][cb] = *reinterpret_cast<const t4*>(x0 + pix * PCO + 16 * cb + 4 * g);
      } else {
#pragma unroll
        for (int ks = 0; ks < NKS; ++ks) {
          const int ch = 32 * ks + 8 * g;
          xsv[ks][r] = ch < a.c0 ? ld_vec<T>(x0 + pix * a.c0 + ch) : ld_vec<T>(x1 + pix * a.c1 + (ch - a.c0));
        }
      }
    }
    if constexpr (PSKIP) {
      const T* wsk = reinterpret_cast<const T*>(a.wp) + (size_t)li * a.ldp + a.Chid + 8 * g;
#pragma unroll
      for (int ks = 0; ks < NKS; ++ks)
#pragma unroll
        for (int cb = 0; cb < NCB; ++cb) wsf[ks][cb] = ld_vec<T>(wsk + (size_t)cb * 16 * a.ldp + 32 * ks);
    }
    if (Halo::PREF && tile + 1 < run.last) halo.load(a, tyn, txn, tiles_x);
    const bool border = irbx_border(a, ty, tx, tiles_x);
    bool ok[3];
    irbx_halo_ok(a, t, border, y0, x0p, ok);
    stamp(1);
    wg_barrier();
    flush_ystats();

    // y[32 pixels][PCO] of the wave starts as its shortcut: raw x (identity form), Wskip . x (skip form)
    f32x4 yacc[2][NCB];
#pragma unroll
    for (int r = 0; r < 2; ++r)
#pragma unroll
      for (int cb = 0; cb < NCB; ++cb) {
        if constexpr (!PSKIP) yacc[r][cb] = f32x4{(float)res[r][cb][0], (float)res[r][cb][1], (float)res[r][cb][2], (float)res[r][cb][3]};
        else yacc[r][cb] = f32x4{0.f, 0.f, 0.f, 0.f};
      }
    if constexpr (PSKIP) {
#pragma unroll
      for (int ks = 0; ks < NKS; ++ks)
#pragma unroll
        for (int r = 0; r < 2; ++r)
#pragma unroll
          for (int cb = 0; cb < NCB; ++cb) yacc[r][cb] = mfma16x16<T>(wsf[ks][cb], xsv[ks][r], yacc[r][cb]);
    }
    stamp(2);
    // (A run-time loop: see expand_dw_body.  Said with a pragma: chunk1 - chunk0 <= KS is visible here, and with the depthwise
    // steps in a function hipcc unrolls the loop fully -- 540 more instructions at KS = 2, 56 bytes of scratch.)
#pragma unroll 1
    for (int chunk = chunk0; chunk < chunk1; ++chunk) {
      if (chunk > chunk0) {
        wg_barrier();  // previous depthwise phase done with sH
        flush_ystats();
        stamp(3);
      }
      // ---- MFMA: h1^T block (32 channels x 32 pixels) x 3 pixel blocks, one accumulator at a time (registers: the identity tail
      // at 32 channels fits three workgroups per CU that way)
      const int ch0 = chunk * 64 + chb * 32;
      // aff2 of this lane's 16 accumulator channels: ch0 + 8g + 4h + e
      f32x4 sc2[4], sh2[4];
#pragma unroll
      for (int g = 0; g < 4; ++g) {
        sc2[g] = *reinterpret_cast<const f32x4*>(aff2 + ch0 + 8 * g + 4 * h);
        sh2[g] = *reinterpret_cast<const f32x4*>(aff2 + a.Chid + ch0 + 8 * g + 4 * h);
      }
#pragma unroll
      for (int i = 0; i < 3; ++i) {
        const int q = (pxg * 3 + i) * 32 + n;
        f32x16 acc;
#pragma unroll
        for (int r = 0; r < 16; ++r) acc[r] = 0.f;
#pragma unroll
        for (int s = 0; s < KS; ++s)
          acc = mfma16<T>(wf[s], *reinterpret_cast<const vec_t*>(sX + q * Halo::XP + (16 * s + 8 * h) * 2), acc);
        if (i == 2) irbx_load_wf<T, KS>(wf, w1, chunk + 1 < chunk1 ? chunk + 1 : chunk0, t);  // next chunk (or the next tile's first)
        irbx_expand_store<T>(acc, sc2, sh2, border, ok[i], buf + q * SHP + (chb * 4 + 2 * h) * 16);
      }
      stamp(4);
      wg_barrier();
      stamp(5);
      // ---- depthwise with the wave's share turned: rows 2 wave, 2 wave + 1 of the tile x the chunk's four 16-channel tiles
      const int choff = irbx_choff(g);  // the lane's 8 channels of a 32-channel half after the swap below
      // Wp fragments of this chunk: rows 16 cb + li, k = the lane's 8 channels of half kb -- in flight under the depthwise steps
      vec_t wpf[NCB][2];
      const T* wp = reinterpret_cast<const T*>(a.wp) + (size_t)li * a.ldp + chunk * 64 + choff;
#pragma unroll
      for (int cb = 0; cb < NCB; ++cb)
#pragma unroll
        for (int kb = 0; kb < 2; ++kb) wpf[cb][kb] = ld_vec<T>(wp + (size_t)cb * 16 * a.ldp + 32 * kb);
      f32x4 dacc[4][2];
      irbx_dw_two_tap<T, 2, 4>(dacc, buf, wave, 0, wds, chunk, a.Chid, t);
      if constexpr (STAMP) {  // a read of the last accumulator: the compiler waits for the depthwise MFMAs here
        asm volatile("" ::"s"(__builtin_amdgcn_readfirstlane(__float_as_int(dacc[3][1][3]))));
        stamp(6);
      }
      // GATEW: the accumulators hold gate * h2 (the gate is in the staged weights); else the SE gate on the fp32 accumulators
      // (lane: channels 16 c + 4 g + e).  One rounding to T, then y += Wp . (gate * h2)
      if constexpr (!GATEW) {
#pragma unroll
        for (int c = 0; c < 4; ++c) {
          const f32x4 gt = *reinterpret_cast<const f32x4*>(gate_s + chunk * 64 + 16 * c + 4 * g);
#pragma unroll
          for (int r = 0; r < 2; ++r)
#pragma unroll
            for (int e = 0; e < 4; ++e) dacc[c][r][e] *= gt[e];
        }
      }
#pragma unroll
      for (int r = 0; r < 2; ++r)
#pragma unroll
        for (int kb = 0; kb < 2; ++kb) {
          const u32x4 v = irbx_pack8_swap<T>(dacc[2 * kb][r], dacc[2 * kb + 1][r]);  // channels 32 kb + choff .. + 7 of pixel li
#pragma unroll
          for (int cb = 0; cb < NCB; ++cb) yacc[r][cb] = mfma16x16<T>(wpf[cb][kb], reinterpret_cast<const vec_t&>(v), yacc[r][cb]);
        }
      stamp(7);
    }
    irbx_project_store_y<T, PCO>(a, t, yacc, b, y0, x0p, red);
    pend_tile = tile;
    stamp(8);
    if constexpr (!Halo::PREF) {  // no registers to hold it under the tile: waited for at once
      if (tile + 1 < run.last) halo.load(a, tyn, txn, tiles_x);
      else halo.clear();  // (so that raw[] is not live around the loop)
    }
    ty = tyn; tx = txn;
  }
  stamp.store(a, t);
  wg_barrier();
  flush_ystats();
}

template <typename T, int KS, bool DBUF, bool STAMP = false, bool NTST = false>
__global__ void __launch_bounds__(256, (KS == 2 && !DBUF) ? 3 : 2) expand_dw_kernel(const IrbxArgs a, const int tiles_per_wg, const int chunks_per_wg) {
  expand_dw_body<T, KS, DBUF, STAMP, NTST>(a, tiles_per_wg, chunks_per_wg);
}
// two workgroups per CU at 64 and 96 channels: the y accumulators and the Wp fragments do not fit the 168 registers of three; at 32
// they do (168, none spilled) once the expand phase keeps one accumulator at a time
template <typename T, int KS, int PCO>
__global__ void __launch_bounds__(256, KS == 2 ? 3 : 2) expand_dw_project_kernel(const IrbxArgs a, const int tiles_per_wg) {
  expand_dw_project_body<T, KS, false, PCO>(a, tiles_per_wg);
}
template <int KS, int PCO>
__global__ void __launch_bounds__(256, KS == 2 ? 3 : 2) expand_dw_project_stamp_kernel(const IrbxArgs a, const int tiles_per_wg) {
  expand_dw_project_body<half_t, KS, true, PCO>(a, tiles_per_wg);
}

// ---------------------------------------------------------------------------------------------
bool irbx_supported(int dtype, int Cin, int c0, int Chid, int H, int W) {
  if (dtype != 1 && dtype != 2) return false;
  if (Cin != 32 && Cin != 64 && Cin != 96) return false;  // Cin = 128: 92 KB of LDS = one workgroup per CU, not worth it
  if (c0 % 16 || Chid != 4 * Cin) return false;
  return W % kXT_W == 0 && H % kXT_H == 0 && (H * W) % irbx_stats_rows(H * W) == 0;
}
int irbx_pool_tiles(int H, int W) { return (H / kXT_H) * (W / kXT_W); }
// the project tail (a rule on the layer alone, never on the batch): kIrbxProjectIdentity for the identity-residual blocks of the
// 32- and 64-channel levels (one input segment), kIrbxProjectSkip for the 96 -> 32 block with a skip conv (one or two segments),
// 0 for every other block
int irbx_project_supported(int dtype, int Cin, int c0, int Chid, int Cout, bool skip, int H, int W) {
  if (!irbx_supported(dtype, Cin, c0, Chid, H, W)) return 0;
  if (!skip) return (Cin == 32 || Cin == 64) && Cout == Cin && c0 == Cin ? kIrbxProjectIdentity : 0;
  return Cin == 96 && Cout == 32 ? kIrbxProjectSkip : 0;
}
int irbx_project_tiles(int H, int W) { return irbx_pool_tiles(H, W); }  // slab entries of y per image: one per 8 x 16 tile
// pixels per statistics partial: fixed per image size (never a function of the batch: bitwise batch invariance)
int irbx_stats_rows(int P) {
  int rp = 128;  // a power of two in [128, 1024], about P / 64
  while (rp < 1024 && rp * 2 * 64 <= P) rp *= 2;
  return rp;
}

StampSink g_irbx_stamps{kXStamps, 0};  // cycles per wave, the slots listed at STAMP; shared by the three stamped kernels

// expand_stats (POOL = false) and expand_pool: the same scan of x, one workgroup per irbx_stats_rows(P) pixels of an image
template <typename T, int KS, int NBW, bool POOL>
static hipError_t launch_scan_cfg(const IrbxArgs& a, hipStream_t s) {
  const int P = a.H * a.W, RP = irbx_stats_rows(P);
  static const char* const name = kernel_name<T>(POOL ? "expand_pool_kernel" : "expand_stats_kernel", KS, NBW);
  note_kernel(name);
  if constexpr (POOL && std::is_same<T, half_t>::value) {
    if (g_knobs.irbx_stamp == 2) {  // diagnostic build: in-kernel cycle stamps
      IrbxArgs b = a;
      if (hipError_t e = g_irbx_stamps.arm((size_t)(P / RP) * a.B * 4, &b.dbg); e != hipSuccess) return e;
      hipLaunchKernelGGL((expand_pool_stamp_kernel<KS, NBW>), dim3(P / RP, 1, a.B), dim3(256), 0, s, b, RP);
      return hipGetLastError();
    }
  }
  constexpr auto kernel = POOL ? &expand_pool_kernel<T, KS, NBW> : &expand_stats_kernel<T, KS, NBW>;
  hipLaunchKernelGGL(kernel, dim3(P / RP, 1, a.B), dim3(256), 0, s, a, RP);
  return hipGetLastError();
}
template <bool POOL>
static hipError_t launch_scan(int dtype, const IrbxArgs& a, hipStream_t s) {
  return with_dtype2(dtype, [&](auto t) {
    return with_value<32, 64, 96>(a.c0 + a.c1, [&](auto cin) {  // Chid = 4 Cin: irbx_supported
      constexpr int NBW = decltype(cin)::value / 32;
      return launch_scan_cfg<decltype(t), 2 * NBW, NBW, POOL>(a, s);
    });
  });
}
hipError_t launch_expand_stats(int dtype, const IrbxArgs& a, hipStream_t s) {
  if (!irbx_supported(dtype, a.c0 + a.c1, a.c0, a.Chid, a.H, a.W) || (a.c1 && !a.x1) || !a.stats) return hipErrorInvalidValue;
  return launch_scan<false>(dtype, a, s);
}
// pool_tot += the image's SE pool totals (fixed point, kPoolFixScale); the caller zeroes it
hipError_t launch_expand_pool(int dtype, const IrbxArgs& a, hipStream_t s) {
  if (!irbx_supported(dtype, a.c0 + a.c1, a.c0, a.Chid, a.H, a.W) || (a.c1 && !a.x1) || !a.pool_tot || !a.as2 || !a.ab2 || !a.wd)
    return hipErrorInvalidValue;
  return launch_scan<true>(dtype, a, s);
}

constexpr int kXTilesPerWg = 4;  // longest run of tiles along x one workgroup takes
// The launch plan of expand_dw (project = false) and expand_dw_project (true) for Cin input channels (Chid = 4 Cin); both
// launchers take it from here and llie_expand_dw_plan reports it.
//   tpw: tiles per workgroup, a run along x (neighbouring halo columns hit L1), as long as the launch keeps >= 2048 workgroups
//   cpw: 64-channel chunks per workgroup: all of them (x tile loaded once) unless the launch would be too small; expand_dw_project
//        always takes all (y accumulates over them)
//   knobs "irbx_grid", "irbx_grid2/4/6" (expand_dw only): about this many workgroups per launch, each image's tiles split evenly
//        over its share (tpw = 0)
IrbxPlan irbx_plan(int Cin, int B, int H, int W, bool project) {
  const int ntiles = irbx_pool_tiles(H, W), nchunks = 4 * Cin / 64;
  IrbxPlan p;
  p.tpw = kXTilesPerWg;
  while (p.tpw > 1 && ((W / kXT_W) % p.tpw || (long)(ntiles / p.tpw) * B < 2048)) p.tpw >>= 1;
  p.cpw = nchunks;
  if (!project)
    while (p.cpw > 1 && (long)(ntiles / p.tpw) * B * (nchunks / p.cpw) < 1024 && p.cpw % 2 == 0) p.cpw >>= 1;
  p.gx = ntiles / p.tpw;
  p.gy = nchunks / p.cpw;
  const int want = project ? 0 : g_knobs.irbx_grid[Cin / 32 - 1];
  if (want > 0) {
    const int gx = want / (B * p.gy);
    p.gx = gx < 1 ? 1 : (gx > ntiles ? ntiles : gx);
    p.tpw = 0;
  }
  return p;
}

template <typename T, int KS, bool DBUF, bool STAMP, bool NTST>
static hipError_t launch_dw_one(const IrbxArgs& a, dim3 grid, size_t lds, int tpw, int cpw, hipStream_t s) {
  static std::atomic<uint64_t> attr_done{0};
  if (hipError_t e = ensure_max_lds(reinterpret_cast<const void*>(&expand_dw_kernel<T, KS, DBUF, STAMP, NTST>), 128 * 1024, attr_done); e != hipSuccess)
    return e;
  hipLaunchKernelGGL((expand_dw_kernel<T, KS, DBUF, STAMP, NTST>), grid, dim3(256), lds, s, a, tpw, cpw);
  return hipGetLastError();
}
template <typename T, int KS, bool DBUF>
static hipError_t launch_dw_cfg(const IrbxArgs& a, hipStream_t s) {
  const size_t lds = irbx_lds_bytes(KS, a.Chid, DBUF, 0);
  const IrbxPlan plan = irbx_plan(16 * KS, a.B, a.H, a.W, false);
  const int tpw = plan.tpw, cpw = plan.cpw;
  static const char* const name = kernel_name<T>("expand_dw_kernel", KS, (int)DBUF);
  note_kernel(name);
  const dim3 grid(plan.gx, plan.gy, a.B);
  if constexpr (std::is_same<T, half_t>::value && !DBUF) {
    if (g_knobs.irbx_stamp == 1) {  // diagnostic build: in-kernel cycle stamps (fp16 only)
      IrbxArgs b = a;
      if (hipError_t e = g_irbx_stamps.arm((size_t)grid.x * grid.y * grid.z * 4, &b.dbg); e != hipSuccess) return e;
      return launch_dw_one<T, KS, DBUF, true, false>(b, grid, lds, tpw, cpw, s);
    }
  }
  if constexpr (!DBUF) {
    if (a.nt) return launch_dw_one<T, KS, DBUF, false, true>(a, grid, lds, tpw, cpw, s);
  }
  return launch_dw_one<T, KS, DBUF, false, false>(a, grid, lds, tpw, cpw, s);
}
template <typename T, int KS, int PCO>
static hipError_t launch_project_cfg(const IrbxArgs& a, hipStream_t s) {
  const size_t lds = irbx_lds_bytes(KS, a.Chid, false, PCO);
  const IrbxPlan plan = irbx_plan(16 * KS, a.B, a.H, a.W, true);
  const int tpw = plan.tpw;
  // PCO = 16 KS is the kernel's default argument, which the profiler's name leaves out
  static const char* const name = PCO == 16 * KS ? kernel_name<T>("expand_dw_project_kernel", KS) : kernel_name<T>("expand_dw_project_kernel", KS, PCO);
  note_kernel(name);
  if constexpr (std::is_same<T, half_t>::value) {
    if (g_knobs.irbx_stamp == 3) {  // diagnostic build: in-kernel cycle stamps (fp16 only)
      IrbxArgs b = a;
      if (hipError_t e = g_irbx_stamps.arm((size_t)plan.gx * plan.gy * a.B * 4, &b.dbg); e != hipSuccess) return e;
      static std::atomic<uint64_t> stamp_attr_done{0};
      if (hipError_t e = ensure_max_lds(reinterpret_cast<const void*>(&expand_dw_project_stamp_kernel<KS, PCO>), 128 * 1024, stamp_attr_done); e != hipSuccess)
        return e;
      hipLaunchKernelGGL((expand_dw_project_stamp_kernel<KS, PCO>), dim3(plan.gx, plan.gy, a.B), dim3(256), lds, s, b, tpw);
      return hipGetLastError();
    }
  }
  static std::atomic<uint64_t> attr_done{0};
  if (hipError_t e = ensure_max_lds(reinterpret_cast<const void*>(&expand_dw_project_kernel<T, KS, PCO>), 128 * 1024, attr_done); e != hipSuccess) return e;
  hipLaunchKernelGGL((expand_dw_project_kernel<T, KS, PCO>), dim3(plan.gx, plan.gy, a.B), dim3(256), lds, s, a, tpw);
  return hipGetLastError();
}
// y = Wp . (gate * dw3x3(relu6(aff2(W1 . relu6(aff1(x)))))) + shortcut with y's statistics slab [B][irbx_project_tiles][2][Cout].
// !skip: the identity form (shortcut x, one segment, wp [cout][Chid], cout = Cin = c0; a.ldp is set here); skip: the skip form
// (shortcut Wskip . x, wp [cout][a.ldp] = project columns, then skip columns, a.ldp >= Chid + Cin)
hipError_t launch_expand_dw_project(int dtype, const IrbxArgs& a0, int cout, bool skip, hipStream_t s) {
  IrbxArgs a = a0;
  const int Cin = a.c0 + a.c1;
  if (!skip) a.ldp = a.Chid;
  const int form = irbx_project_supported(dtype, Cin, a.c0, a.Chid, cout, skip, a.H, a.W);
  if (!form || (a.c1 != 0) != (a.x1 != nullptr) || a.ldp < a.Chid + (skip ? Cin : 0) || a.ldp % 8 || !a.gate || !a.wp || !a.y || !a.ystats ||
      !a.as2 || !a.ab2 || !a.wd)
    return hipErrorInvalidValue;
  return with_dtype2(dtype, [&](auto t) {
    using T = decltype(t);
    if (form == kIrbxProjectSkip) return launch_project_cfg<T, 6, 32>(a, s);
    return a.c0 == 32 ? launch_project_cfg<T, 2, 32>(a, s) : launch_project_cfg<T, 4, 64>(a, s);
  });
}
hipError_t launch_expand_dw(int dtype, const IrbxArgs& a, hipStream_t s) {
  if (!irbx_supported(dtype, a.c0 + a.c1, a.c0, a.Chid, a.H, a.W) || (a.c1 && !a.x1) || !a.out) return hipErrorInvalidValue;
  return with_dtype2(dtype, [&](auto t) {
    using T = decltype(t);
    return with_value<32, 64, 96>(a.c0 + a.c1, [&](auto cin) {
      constexpr int KS = decltype(cin)::value / 16;
      // llie_tune("irbx_dbuf", 1): double-buffered h1 tile for the 32-channel inputs (one barrier per chunk, 76 KB of LDS = two
      // workgroups per CU).  The single-buffered kernel (49 KB, three workgroups per CU) is the default: 1 % faster end to end
      if constexpr (KS == 2) {
        if (g_knobs.irbx_dbuf) return launch_dw_cfg<T, KS, true>(a, s);
      }
      return launch_dw_cfg<T, KS, false>(a, s);
    });
  });
}

// ---------------------------------------------------------------------------------------------
// (3) The wide decoder blocks (192 -> 64 at hid 768, 384 -> 128 at hid 1536) without h2, from the STORED h1.  Recomputing h1 is
// too dear there (155 GFLOP per pass), so pw_expand still writes it; what goes is the depthwise output: written once and read
// once only because SE needs its pooled mean before the projection may start.
//   dwconv3x3_pool_kernel     one streaming read of h1 leaves the SE pool totals: the nine-sum restatement of expand_scan<POOL>
//                             with a = clamp01(h1 s + b) rounded to T exactly where the project kernel rounds the tile it parks
//                             in LDS, and the weights T(6 w);
//   dwconv3x3_project_kernel  a workgroup owns one 8 x 16 tile: per 64-channel chunk it loads the 10 x 18 halo tile of h1,
//                             activates it into the LDS tile of the recompute kernels (that replaces their expand phase) and
//                             runs their depthwise steps, pack-and-swap and project MFMAs; y accumulates in registers over the
//                             chunks, starts as the skip conv of the raw input and leaves through irbx_project_store_y.
// as2 / ab2 are norm2's tables divided by 6 (IrbxArgs::h1).

// The pool pass.  grid (H / 8, Chid / 128, B): a workgroup reads 8 image rows of 128 channels; thread (cv = tid & 15, pg = tid >> 4)
// owns 8 channels of the pixels pg, pg + 16, ... of those rows, eight loads in flight.  Sums per thread: everything, the first and
// the last image row (a row's sum is added where the row ends: a uniform branch); the first / last column and the corners come
// from one more load per thread (pg < 8: column 0 of row pg, else column W - 1 of row pg - 8; the lines are in L2).  The 16 pixel
// slots are added in slot order through LDS, the nine sums combined with the weights and one fixed-point atomic per channel
// leaves the workgroup: the float order depends on (H, W, Chid) alone, the integer adds commute.
constexpr int kWpRows = 8;
template <typename T>
__global__ void __launch_bounds__(256) dwconv3x3_pool_kernel(const IrbxArgs a) {
  typedef typename Elem<T>::vec_t vec_t;
  __shared__ __align__(16) float red[4][16][128];  // everything, first row, last row, column pixels
  const int tid = threadIdx.x, cv = tid & 15, pg = tid >> 4;
  const int b = blockIdx.z, cbase = blockIdx.y * 128, y0 = blockIdx.x * kWpRows;
  const int c8 = cbase + cv * 8;
  const T* h1 = reinterpret_cast<const T*>(a.h1) + (size_t)b * a.H * a.W * a.Chid + c8;
  float sc[8], sh[8];
#pragma unroll
  for (int e = 0; e < 8; ++e) {
    sc[e] = a.as2[(size_t)b * a.Chid + c8 + e];
    sh[e] = a.ab2[(size_t)b * a.Chid + c8 + e];
  }
  auto act = [&](vec_t v, float (&f)[8]) {  // a in T, as fp32
    const u32x4 x = reinterpret_cast<const u32x4&>(v);
    u32x4 o;
#pragma unroll
    for (int q = 0; q < 4; ++q) o[q] = act_clamp01_pack<T>(x[q], sc[2 * q], sc[2 * q + 1], sh[2 * q], sh[2 * q + 1]);
    vec_to_f32<T>(reinterpret_cast<const vec_t&>(o), f);
  };
  float all[8], r0[8], rh[8], row[8];
#pragma unroll
  for (int e = 0; e < 8; ++e) all[e] = r0[e] = rh[e] = row[e] = 0.f;
  const int n = kWpRows * a.W / 16;  // a multiple of 8 (W % 16 == 0)
  const size_t step = (size_t)16 * a.Chid;
  const T* p = h1 + ((size_t)y0 * a.W + pg) * a.Chid;
  int col = 0, gy = y0;
  for (int i0 = 0; i0 < n; i0 += 8) {
    vec_t v[8];
#pragma unroll
    for (int u = 0; u < 8; ++u) v[u] = ld_vec<T>(p + (size_t)(i0 + u) * step);
#pragma unroll
    for (int u = 0; u < 8; ++u) {
      float f[8];
      act(v[u], f);
#pragma unroll
      for (int e = 0; e < 8; ++e) row[e] += f[e];
      col += 16;
      if (col == a.W) {  // uniform: an image row ends
#pragma unroll
        for (int e = 0; e < 8; ++e) {
          all[e] += row[e];
          if (gy == 0) r0[e] += row[e];
          if (gy == a.H - 1) rh[e] += row[e];
          row[e] = 0.f;
        }
        col = 0; ++gy;
      }
    }
  }
  float cf[8];
  act(ld_vec<T>(h1 + ((size_t)(y0 + (pg & 7)) * a.W + (pg >= 8 ? a.W - 1 : 0)) * a.Chid), cf);
#pragma unroll
  for (int e = 0; e < 8; ++e) {
    red[0][pg][cv * 8 + e] = all[e];
    red[1][pg][cv * 8 + e] = r0[e];
    red[2][pg][cv * 8 + e] = rh[e];
    red[3][pg][cv * 8 + e] = cf[e];
  }
  wg_barrier();
  if (tid < 128) {
    const int c = tid;
    float v[9] = {0.f, 0.f, 0.f, 0.f, 0.f, 0.f, 0.f, 0.f, 0.f};  // as in expand_scan: all, first / last row, first / last column, corners
#pragma unroll
    for (int s = 0; s < 16; ++s) {
      v[0] += red[0][s][c]; v[1] += red[1][s][c]; v[2] += red[2][s][c];
    }
#pragma unroll
    for (int s = 0; s < 8; ++s) {
      v[3] += red[3][s][c]; v[4] += red[3][8 + s][c];
    }
    if (y0 == 0) { v[5] = red[3][0][c]; v[6] = red[3][8][c]; }
    if (y0 + kWpRows == a.H) { v[7] = red[3][7][c]; v[8] = red[3][15][c]; }
    float t = 0.f;
#pragma unroll
    for (int tap = 0; tap < 9; ++tap) {  // tap (ky, kx) reads pixel p + (ky - 1, kx - 1): p itself must leave the far border out
      const int ky = tap / 3, kx = tap % 3;
      float st = v[0];
      if (ky == 2) st -= v[1];
      if (ky == 0) st -= v[2];
      if (kx == 2) st -= v[3];
      if (kx == 0) st -= v[4];
      if (ky == 2 && kx == 2) st += v[5];
      if (ky == 2 && kx == 0) st += v[6];
      if (ky == 0 && kx == 2) st += v[7];
      if (ky == 0 && kx == 0) st += v[8];
      t = __builtin_fmaf((float)(T)(6.f * a.wd[tap * a.Chid + cbase + c]), st, t);
    }
    fixed_add(a.pool_tot + (size_t)b * a.Chid + cbase + c, t, kPoolFixScale);
  }
}

// The depthwise-project pass.  grid (tiles, 1, B), four waves.  Dynamic LDS: [sH: 192 x 144 B][wds: 10 x Chid T][wpl: PCO x 144 B]
// [red: 4 x 2 x PCO fp32].  The SE gate is part of the staged depthwise weights, T(6 w gate), as in expand_dw_project<2, 32> and
// <6, 32>.  The depthwise phase is the MFMA form (irbx_dw_two_tap): the project MFMAs want its accumulator layout, and the VALU
// has the activation of the halo tile to do.  Thread (kv = tid & 7, q0 = tid >> 3) stages the 16-byte channel vector kv of the
// halo pixels q0 + 32 j of every chunk: the six loads of a later chunk go out before this chunk's depthwise phase.
// The chunk's project columns of Wp go through LDS too ([PCO rows][64 channels + 16 B pad], the pitch of the h1 tile): loaded once
// per workgroup with whole 128-byte rows, read as MFMA A fragments by all four waves.  Fetched by every wave as fragments straight
// from memory -- 16 rows x 64 bytes per load instruction -- they cost more than everything else in the chunk (profiles/r21/README.md).
constexpr size_t wide_lds_bytes(int Chid, int PCO) { return (size_t)kXNPB * 32 * SHP + 10 * Chid * 2 + PCO * SHP + 8 * PCO * 4; }
static_assert(2 * wide_lds_bytes(768, 64) <= 160 * 1024 && 2 * wide_lds_bytes(1536, 128) <= 160 * 1024, "two workgroups per CU");
// PREACT: a.h1 already holds a = T(clamp01(h1 as2 + ab2)) (pw_expand_act_kernel stored it): the halo tile goes to LDS as loaded
// and norm2's tables are neither fetched nor kept in registers.
template <typename T, int PCO, bool PREACT = false>
__global__ void __launch_bounds__(256, 2) dwconv3x3_project_kernel(const IrbxArgs a) {
  constexpr int NCB = PCO / 16, NPASS = kXNPB * 32 / 32;
  // chunks the halo tile is fetched ahead: two at 64 output channels; at 128 the y accumulators and the skip conv's operands leave
  // room for one set of staging registers only (two sets spill 80 registers)
  constexpr int DEPTH = PCO == 64 ? 2 : 1;
  typedef typename Elem<T>::vec_t vec_t;
  extern __shared__ __align__(16) unsigned char smem[];
  unsigned char* buf = smem;
  T* wds = reinterpret_cast<T*>(smem + kXNPB * 32 * SHP);
  unsigned char* wpl = smem + kXNPB * 32 * SHP + 10 * a.Chid * 2;
  float* red = reinterpret_cast<float*>(wpl + PCO * SHP);

  const IrbxLane t = irbx_lane();
  const int tid = t.tid, wave = t.wave, li = t.li, g = t.g;
  const int b = blockIdx.z;
  const int tiles_x = a.W / kXT_W;
  const int ty = blockIdx.x / tiles_x, tx = blockIdx.x % tiles_x;
  const int y0 = ty * kXT_H, x0p = tx * kXT_W;
  const int P = a.H * a.W, Cin = a.c0 + a.c1;
  const T* x0 = reinterpret_cast<const T*>(a.x0) + (size_t)b * P * a.c0;
  const T* x1 = a.x1 ? reinterpret_cast<const T*>(a.x1) + (size_t)b * P * a.c1 : nullptr;
  const T* h1 = reinterpret_cast<const T*>(a.h1) + (size_t)b * P * a.Chid;
  const int nchunks = a.Chid / 64;

  // the thread's six halo pixels: offset inside the image's h1 (its channel vector included), and whether the pixel exists --
  // outside the image the depthwise input is zero (the conv's padding), and pixels 180..191 of the last MFMA block do not exist
  const int kv = tid & 7, q0 = tid >> 3;
  // Every thread loads all six, from a pixel clamped into the image where its own does not exist: unpredicated loads are
  // counted exactly by hipcc's vmcnt bookkeeping, so the wait for one chunk's operands leaves the younger prefetch in flight
  // (a lane-predicated load makes it wait for everything: profiles/r20/README.md, section 1).  The tile is fetched DEPTH chunks
  // ahead: two workgroups per CU have to keep enough bytes in flight for the memory latency (profiles/r21/README.md).
  int hoff[NPASS];
  bool hok[NPASS];
#pragma unroll
  for (int j = 0; j < NPASS; ++j) {
    const int q = q0 + 32 * j;
    const int gy = y0 - 1 + q / kXH_W, gx = x0p - 1 + q % kXH_W;
    hok[j] = q < kXNPX && gy >= 0 && gy < a.H && gx >= 0 && gx < a.W;
    const int cy = gy < 0 ? 0 : (gy < a.H ? gy : a.H - 1), cx = gx < 0 ? 0 : (gx < a.W ? gx : a.W - 1);
    hoff[j] = (cy * a.W + cx) * a.Chid + kv * 8;
  }
  // with the tile come norm2's tables of the thread's 8 channels of that chunk: scale (2 x 4), then shift
  vec_t raw[DEPTH][NPASS];
  f32x4 aff[DEPTH][PREACT ? 1 : 4];
  const float* as2 = PREACT ? nullptr : a.as2 + (size_t)b * a.Chid + kv * 8;
  const float* ab2 = PREACT ? nullptr : a.ab2 + (size_t)b * a.Chid + kv * 8;
  auto load = [&](int chunk, vec_t (&dst)[NPASS], f32x4 (&af)[PREACT ? 1 : 4]) {
#pragma unroll
    for (int j = 0; j < NPASS; ++j) dst[j] = ld_vec<T>(h1 + hoff[j] + chunk * 64);
    if constexpr (PREACT) return;
    af[0] = *reinterpret_cast<const f32x4*>(as2 + chunk * 64); af[1] = *reinterpret_cast<const f32x4*>(as2 + chunk * 64 + 4);
    af[2 % (PREACT ? 1 : 4)] = *reinterpret_cast<const f32x4*>(ab2 + chunk * 64);
    af[3 % (PREACT ? 1 : 4)] = *reinterpret_cast<const f32x4*>(ab2 + chunk * 64 + 4);
  };
  // the chunk's Wp block: vector v = tid + 256 j -> row v / 8, 16-byte channel vector v % 8; one chunk ahead
  constexpr int NWV = PCO * 8 / 256;
  vec_t wreg[NWV];
  auto load_wp = [&](int chunk) {
#pragma unroll
    for (int j = 0; j < NWV; ++j) wreg[j] = ld_vec<T>(reinterpret_cast<const T*>(a.wp) + (size_t)(q0 + 32 * j) * a.ldp + chunk * 64 + kv * 8);
  };
  load_wp(0);
#pragma unroll
  for (int d = 0; d < DEPTH; ++d) load(d, raw[d], aff[d]);
  // The constants of irbx_stage_constants, [tap pair][channel][2] weights and the two tables.  A workgroup serves ONE tile, so
  // their staging is not amortised over a run of tiles: a thread owns channels tid + 256 k and all its loads (nine weights, the
  // gate, two table entries per channel) go out together -- as a loop over the 10 Chid weight slots, one dependent pair of loads
  // per iteration, the staging alone took 30 (60) memory round trips per workgroup, most of the kernel (profiles/r21/README.md)
  {
    constexpr int KC = 12 * PCO / 256;  // Chid / 256: 3 or 6 channels per thread
    float wv[KC][9], gv[KC];
#pragma unroll
    for (int k = 0; k < KC; ++k) {
      const int c = tid + 256 * k;
#pragma unroll
      for (int tap = 0; tap < 9; ++tap) wv[k][tap] = a.wd[tap * a.Chid + c];
      gv[k] = a.gate[(size_t)b * a.Chid + c];
    }
#pragma unroll
    for (int k = 0; k < KC; ++k) {
      const int c = tid + 256 * k;
#pragma unroll
      for (int p = 0; p < 5; ++p) {
        wds[2 * (p * a.Chid + c)] = (T)(6.f * wv[k][2 * p] * gv[k]);
        wds[2 * (p * a.Chid + c) + 1] = p < 4 ? (T)(6.f * wv[k][2 * p + 1] * gv[k]) : (T)0.f;
      }
    }
  }

  // y[32 pixels][PCO] of the wave starts as Wskip . x on the raw centre pixels: Cin / 32 k-steps (expand_dw_project_body's skip
  // form).  The x operands of six k-steps go out together (they come from HBM), the weight rows two k-steps at a time (L2)
  f32x4 yacc[2][NCB];
#pragma unroll
  for (int r = 0; r < 2; ++r)
#pragma unroll
    for (int cb = 0; cb < NCB; ++cb) yacc[r][cb] = f32x4{0.f, 0.f, 0.f, 0.f};
  {
    const T* wsk = reinterpret_cast<const T*>(a.wp) + (size_t)li * a.ldp + a.Chid + 8 * g;
    const size_t pix0 = (size_t)(y0 + 2 * wave) * a.W + x0p + li;
#pragma unroll 1
    for (int ks0 = 0; ks0 < Cin / 32; ks0 += 6) {  // Cin / 32 is 6 or 12
      vec_t xsv[6][2];
#pragma unroll
      for (int u = 0; u < 6; ++u) {
        const int ch = 32 * (ks0 + u) + 8 * g;
#pragma unroll
        for (int r = 0; r < 2; ++r) {
          const size_t pix = pix0 + (size_t)r * a.W;
          xsv[u][r] = ch < a.c0 ? ld_vec<T>(x0 + pix * a.c0 + ch) : ld_vec<T>(x1 + pix * a.c1 + (ch - a.c0));
        }
      }
#pragma unroll
      for (int u0 = 0; u0 < 6; u0 += 2) {
        vec_t wsf[2][NCB];
#pragma unroll
        for (int u = 0; u < 2; ++u)
#pragma unroll
          for (int cb = 0; cb < NCB; ++cb) wsf[u][cb] = ld_vec<T>(wsk + (size_t)cb * 16 * a.ldp + 32 * (ks0 + u0 + u));
#pragma unroll
        for (int u = 0; u < 2; ++u)
#pragma unroll
          for (int r = 0; r < 2; ++r)
#pragma unroll
            for (int cb = 0; cb < NCB; ++cb) yacc[r][cb] = mfma16x16<T>(wsf[u][cb], xsv[u0 + u][r], yacc[r][cb]);
      }
    }
  }

  const int choff = irbx_choff(g);  // the lane's 8 channels of a 32-channel half after the swap below
  // one chunk: `cur` holds its halo tile and is refilled with the tile of chunk + 2 once it has been activated into sH
  auto chunk_step = [&](const int chunk, vec_t (&cur)[NPASS], f32x4 (&af)[PREACT ? 1 : 4]) {
    wg_barrier();  // weights staged (first chunk); previous depthwise phase done with sH, previous project phase with wpl
#pragma unroll
    for (int j = 0; j < NPASS; ++j) {  // activate8 on tables held in registers
      const u32x4 x = reinterpret_cast<const u32x4&>(cur[j]);
      u32x4 o = x;
      if constexpr (!PREACT) {
        constexpr int A1 = PREACT ? 0 : 1, A2 = PREACT ? 0 : 2, A3 = PREACT ? 0 : 3;
        o[0] = act_clamp01_pack<T>(x[0], af[0][0], af[0][1], af[A2][0], af[A2][1]);
        o[1] = act_clamp01_pack<T>(x[1], af[0][2], af[0][3], af[A2][2], af[A2][3]);
        o[2] = act_clamp01_pack<T>(x[2], af[A1][0], af[A1][1], af[A3][0], af[A3][1]);
        o[3] = act_clamp01_pack<T>(x[3], af[A1][2], af[A1][3], af[A3][2], af[A3][3]);
      }
      *reinterpret_cast<u32x4*>(buf + (q0 + 32 * j) * SHP + kv * 16) = hok[j] ? o : u32x4{0u, 0u, 0u, 0u};
    }
#pragma unroll
    for (int j = 0; j < NWV; ++j) *reinterpret_cast<vec_t*>(wpl + (q0 + 32 * j) * SHP + kv * 16) = wreg[j];
    // the next chunk's Wp block goes out BEFORE the halo prefetch: the wait for it at the top of the next chunk (vmcnt counts in
    // order) then leaves the younger prefetch in flight
    load_wp(chunk + 1 < nchunks ? chunk + 1 : chunk);
    __builtin_amdgcn_sched_barrier(0);
    load(chunk + DEPTH < nchunks ? chunk + DEPTH : chunk, cur, af);  // (the last DEPTH refills are never used)
    wg_barrier();
    // depthwise: rows 2 wave, 2 wave + 1 of the tile x the chunk's four 16-channel tiles; the accumulators hold gate * h2
    f32x4 dacc[4][2];
    irbx_dw_two_tap<T, 2, 4>(dacc, buf, wave, 0, wds, chunk, a.Chid, t);
#pragma unroll
    for (int r = 0; r < 2; ++r)
#pragma unroll
      for (int kb = 0; kb < 2; ++kb) {
        const u32x4 v = irbx_pack8_swap<T>(dacc[2 * kb][r], dacc[2 * kb + 1][r]);  // channels 32 kb + choff .. + 7 of pixel li
#pragma unroll
        for (int cb = 0; cb < NCB; ++cb)  // A fragment: rows 16 cb + li of Wp, k = the lane's 8 channels of half kb
          yacc[r][cb] = mfma16x16<T>(*reinterpret_cast<const vec_t*>(wpl + (16 * cb + li) * SHP + (32 * kb + choff) * 2),
                                     reinterpret_cast<const vec_t&>(v), yacc[r][cb]);
      }
  };
#pragma unroll 1
  for (int chunk = 0; chunk < nchunks; chunk += DEPTH) {  // Chid / 64 is 12 or 24
#pragma unroll
    for (int d = 0; d < DEPTH; ++d) chunk_step(chunk + d, raw[d], aff[d]);
  }
  irbx_project_store_y<T, PCO>(a, t, yacc, b, y0, x0p, red);
  wg_barrier();
  if (tid < 2 * PCO)  // the four waves' (sum, sum of squares) [wave][2][PCO], added in wave order
    a.ystats[((size_t)b * gridDim.x + blockIdx.x) * 2 * PCO + tid] = (red[tid] + red[2 * PCO + tid]) + (red[4 * PCO + tid] + red[6 * PCO + tid]);
}

bool wide_project_supported(int dtype, int Cin, int c0, int Chid, int Cout, bool skip, bool padded, int H, int W) {
  if ((dtype != 1 && dtype != 2) || padded || !skip) return false;
  if (!((Cin == 192 && Chid == 768 && Cout == 64) || (Cin == 384 && Chid == 1536 && Cout == 128))) return false;
  if (c0 <= 0 || c0 > Cin || c0 % 16) return false;
  if (H <= 0 || W <= 0 || (long long)H * W * Chid >= (1ll << 31)) return false;  // the project kernel's halo offsets are 32-bit
  return H % kXT_H == 0 && W % kXT_W == 0;
}
// pool_tot += the image's SE pool totals (fixed point, kPoolFixScale); the caller zeroes it
hipError_t launch_dwconv3x3_pool(int dtype, const IrbxArgs& a, hipStream_t s) {
  if ((dtype != 1 && dtype != 2) || (a.Chid != 768 && a.Chid != 1536) || a.B <= 0 || a.H <= 0 || a.W <= 0 || a.H % kWpRows || a.W % 16 || !a.h1 ||
      !a.pool_tot || !a.as2 || !a.ab2 || !a.wd)
    return hipErrorInvalidValue;
  const dim3 grid(a.H / kWpRows, a.Chid / 128, a.B);
  return with_dtype2(dtype, [&](auto t) {
    using T = decltype(t);
    static const char* const name = kernel_name<T>("dwconv3x3_pool_kernel");
    note_kernel(name);
    hipLaunchKernelGGL((dwconv3x3_pool_kernel<T>), grid, dim3(256), 0, s, a);
    return hipGetLastError();
  });
}
template <typename T, int PCO, bool PREACT = false>
static hipError_t launch_wide_project_cfg(const IrbxArgs& a, hipStream_t s) {
  static const char* const name = PREACT ? kernel_name<T>("dwconv3x3_project_kernel", PCO, true) : kernel_name<T>("dwconv3x3_project_kernel", PCO);
  note_kernel(name);
  static std::atomic<uint64_t> attr_done{0};
  if (hipError_t e = ensure_max_lds(reinterpret_cast<const void*>(&dwconv3x3_project_kernel<T, PCO, PREACT>), 128 * 1024, attr_done); e != hipSuccess) return e;
  hipLaunchKernelGGL((dwconv3x3_project_kernel<T, PCO, PREACT>), dim3(irbx_project_tiles(a.H, a.W), 1, a.B), dim3(256), wide_lds_bytes(a.Chid, PCO), s, a);
  return hipGetLastError();
}
// y = Wp . (gate * dw3x3(clamp01(h1 as2 + ab2) x 6 w)) + Wskip . [x0 | x1] with y's statistics slab [B][irbx_project_tiles][2][cout];
// wp [cout][a.ldp] = project columns, then skip columns (a.ldp >= Chid + Cin, a.ldp % 8 == 0)
hipError_t launch_dwconv3x3_project(int dtype, const IrbxArgs& a, int cout, hipStream_t s) {
  const int Cin = a.c0 + a.c1;
  if (!wide_project_supported(dtype, Cin, a.c0, a.Chid, cout, true, false, a.H, a.W) || a.B <= 0 || (a.c1 != 0) != (a.x1 != nullptr) || !a.x0 ||
      a.ldp < a.Chid + Cin || a.ldp % 8 || !a.h1 || !a.gate || !a.wp || !a.y || !a.ystats || (!a.h1_act && (!a.as2 || !a.ab2)) || !a.wd)
    return hipErrorInvalidValue;
  if (a.h1_act && cout != 64) return hipErrorInvalidValue;  // the activated h1 of pw_expand_act: 192 -> 64 only
  return with_dtype2(dtype, [&](auto t) {
    using T = decltype(t);
    if (a.h1_act) return launch_wide_project_cfg<T, 64, true>(a, s);
    return cout == 64 ? launch_wide_project_cfg<T, 64>(a, s) : launch_wide_project_cfg<T, 128>(a, s);
  });
}

}  // namespace llie
