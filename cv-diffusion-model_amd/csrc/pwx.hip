// Expanding pointwise GEMM (1x1 conv, N = 4 K) in activation-stationary form for gfx950, 2-byte compute types.
//
// Replaces the reference's `expand` conv of the wide InvertedResidualBlocks (efficient_unet.py:174 with norm1 + ReLU6
// :207-208 in the operand prologue and the statistics of norm2 :212 in the epilogue; virtual torch.cat :588 as K segments).
//
// These launches write four times what they read (K <= 512 in, N = 4 K out): the tile-per-workgroup kernel of gemm.hip
// spends them waiting -- every output tile re-reads and re-activates its A rows, pays two barriers per K chunk and
// pushes its C tile through LDS in bursts that all workgroups issue at the same moment (profiles/r03/
// gemm_stamp_baseline.txt: 27 k cycles per wave and tile for 1.5 k cycles of MFMA).  Here
//
//   * a workgroup (4 waves) owns 128 pixels and ALL its output channels (or 1 / nsplit of them on small grids); each
//     wave loads its 32 pixel rows once, coalesced, applies norm1 + ReLU6 (clamp01(z / 6), kernels.h: ACT_RELU6_S6)
//     once and keeps them as MFMA A-operand fragments IN REGISTERS for the whole launch (K / 4 VGPRs);
//   * the weights stream past: they are stored pre-packed in MFMA B-fragment order (and pre-multiplied by the 6 of the
//     ReLU6 carry), so a 32-channel block is K / 16 KB of contiguous memory that the LDS-DMA engine
//     (global_load_lds_dwordx4) drops into a double-buffered LDS ring with no staging registers and no bank conflicts
//     on the ds_read_b128 side; one barrier per buffer;
//   * the epilogue never touches LDS with the tile: accumulators (lane = channel, registers = pixels) are rounded to T,
//     the GroupNorm partial sums come from v_dot2 on the packed words (a lane's 16 pixels, one half-swap, one LDS word
//     per wave and channel), the tile is transposed ON THE MATRIX PIPE (two MFMAs against a 0/1 selection matrix: exact)
//     into lane = pixel, registers = channels; after v_permlane32_swap a lane owns 16-byte runs of one pixel's channels,
//     which go through a wave-private 4.5 KB LDS tile (no barrier) and leave, every second block, as four stores of
//     8 rows x 128 bytes -- whole cache lines (32-byte pieces straight from registers cost 30 % of the launch:
//     profiles/r03/pwx_store_shape.txt), a steady trickle under the next block's MFMAs instead of a burst per tile.
//
// Statistics are fixed per-(128-pixel tile, channel) slab entries summed in a fixed order: bitwise independent of the batch.
#include <type_traits>
#include <vector>

#include "common.h"
#include "kernels.h"

namespace llie {

namespace {

typedef _Float16 f16x2_t __attribute__((ext_vector_type(2)));
typedef __bf16 bf16x2_v __attribute__((ext_vector_type(2)));

template <typename T> __device__ __forceinline__ uint32_t pack2(float a, float b) {
  typedef T t2 __attribute__((ext_vector_type(2)));
  t2 o;
  o[0] = (T)a;
  o[1] = (T)b;
  return *reinterpret_cast<uint32_t*>(&o);
}
// c + x.lo * y.lo + x.hi * y.hi on packed 2-byte pairs, fp32 accumulate (v_dot2_f32_f16 / v_dot2_f32_bf16)
template <typename T> __device__ __forceinline__ float dot2(uint32_t x, uint32_t y, float c) {
  if constexpr (std::is_same<T, half_t>::value)
    return __builtin_amdgcn_fdot2(*reinterpret_cast<f16x2_t*>(&x), *reinterpret_cast<f16x2_t*>(&y), c, false);
  else
    return __builtin_amdgcn_fdot2_f32_bf16(*reinterpret_cast<bf16x2_v*>(&x), *reinterpret_cast<bf16x2_v*>(&y), c, false);
}
template <typename T> __device__ __forceinline__ f32x16 mfma_u(const u32x4& a, const u32x4& b, f32x16 c) {
  typedef typename Elem<T>::vec_t vec_t;
  return mfma16<T>(reinterpret_cast<const vec_t&>(a), reinterpret_cast<const vec_t&>(b), c);
}
template <typename T> constexpr uint32_t one_bits() { return std::is_same<T, half_t>::value ? 0x3C00u : 0x3F80u; }

constexpr int kStagePitch = 144;  // bytes per staged 64-channel row: 128 + one 16-byte pad (conflict-free ds_read_b128)
constexpr bool pwx_has_tile(int KS, int NBW, bool REGSTORE) { return !REGSTORE || NBW * KS * 1024 < 4 * 32 * kStagePitch; }
constexpr int pwx_lds_bytes(int KS, int NBW, bool REGSTORE) {
  return 2 * NBW * KS * 1024 + 2 * 4 * NBW * 64 * 4 + (pwx_has_tile(KS, NBW, REGSTORE) ? 4 * 32 * kStagePitch : 0);
}
constexpr int kPwxActMaxN = 768;  // ACT: three fp32 per output channel behind the tiles (norm2's scale and shift, the sum of the nine depthwise weights)

}  // namespace

// KS = K / 16 MFMA steps; NBW = 32-channel blocks per LDS buffer (1 everywhere, see kPwxNbw).
// REGSTORE = output stores straight from registers (32 rows x 32 bytes per instruction) instead of through the LDS tile.
// STAMP (llie_tune "pwx_stamp") = s_memtime per wave after the A phase and at the end.  Template parameters, not run-time
// flags: a flag inside the MFMA loop changes the code it measures.
//
// ACT (pw_expand_act_kernel): norm2's tables are known before the launch (gram.hip: the wide Gram), so the epilogue stores the
// ACTIVATED h1, a = T(clamp01(acc s + b)) with one rounding, and adds the SE pool totals dwconv3x3_pool would have added from it:
// no statistics slab.  The depthwise conv is linear and zero-padded, so the totals are nine border-aware sums of a per channel
// (irbx.hip: expand_scan<POOL>).  This kernel adds the first of them, the sum over all pixels times the sum of the nine weights:
// lane = channel here, so it is eight v_dot2 per block and one fixed-point add per channel and 128-pixel tile.  The other eight
// (first / last row and column, four corners) touch 4 (H + W) pixels of the image and are taken back out by
// pool_border_kernel from the stored tensor.  Nothing is loaded from global memory inside the channel loop: vmcnt counts in
// order, so a load's wait would also wait for the output stores issued before it (with norm2's tables and the border weights
// fetched per block the launch took 325 us instead of 245); the tables and the weight sums are staged in LDS before the loop.
template <typename T, int KS, int NBW, bool REGSTORE, bool STAMP, bool ACT>
__device__ __forceinline__ void pw_expand_body(const ExpandArgs& g) {
  unsigned long long t_start = 0, t_a = 0, t_wait = 0;
  if constexpr (STAMP) t_start = __builtin_amdgcn_s_memtime();
  static_assert(sizeof(T) == 2 && KS % 4 == 0, "");
  constexpr int BUF = NBW * KS * 1024;  // bytes per weight buffer
  constexpr bool LDSOUT = !REGSTORE;  // full 128-byte lines through a wave-private LDS tile
  constexpr bool HAS_TILE = pwx_has_tile(KS, NBW, REGSTORE);  // wave-private [32 pixels][64 channels + pad] tiles behind the statistics
  extern __shared__ __align__(16) unsigned char smem[];
  float* red = reinterpret_cast<float*>(smem + 2 * BUF);  // [2][4 waves][NBW][2][32]
  unsigned char* tbuf = smem + 2 * BUF + 2 * 4 * NBW * 64 * 4 + (threadIdx.x >> 6) * (32 * kStagePitch);
  float* swall = reinterpret_cast<float*>(smem + pwx_lds_bytes(KS, NBW, REGSTORE));  // ACT only

  const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
  const int lr = lane & 31, lh = lane >> 5;
  // tile order: the nsplit channel parts of a pixel tile, and runs of pixel tiles, stay on one XCD (round-robin dispatch)
  const int mtiles = g.M >> 7;
  int mt = blockIdx.x / g.nsplit, part = blockIdx.x % g.nsplit;
  if ((mtiles & 7) == 0) {
    const int xcd = blockIdx.x & 7, slot = blockIdx.x >> 3;
    mt = (slot / g.nsplit) * 8 + xcd;
    part = slot % g.nsplit;
  }
  const int tpi = g.P >> 7;
  const int img = mt / tpi, tile = mt - img * tpi;
  const size_t m0 = (size_t)mt * 128;
  const int nper = g.N / g.nsplit, nbase = part * nper, nit = nper / (32 * NBW);
  const unsigned char* wsrc = reinterpret_cast<const unsigned char*>(g.wf) + (size_t)(nbase >> 5) * KS * 1024;

  auto dma = [&](int it) {  // weight buffer `it` -> LDS ring slot it & 1: NBW * KS contiguous KB, 16 bytes per lane
    const unsigned char* src = wsrc + (size_t)it * BUF + lane * 16;
    unsigned char* dst = smem + (it & 1) * BUF;
#pragma unroll
    for (int c = 0; c < NBW * KS / 4; ++c) {
      const int chunk = wave + 4 * c;
      __builtin_amdgcn_global_load_lds((const __attribute__((address_space(1))) void*)(src + chunk * 1024),
                                       (__attribute__((address_space(3))) void*)(dst + chunk * 1024), 16, 0, 0);
    }
  };
  dma(0);
  if constexpr (ACT) {  // [scale2][shift2][sum of the nine T(6 w)] of this workgroup's channels
    for (int c = tid; c < nper; c += 256) {
      float t = 0.f;
#pragma unroll
      for (int tap = 0; tap < 9; ++tap) t += (float)(T)(6.f * g.wd[tap * g.N + nbase + c]);
      swall[c] = g.as2[(size_t)img * g.N + nbase + c];
      swall[kPwxActMaxN + c] = g.ab2[(size_t)img * g.N + nbase + c];
      swall[2 * kPwxActMaxN + c] = t;
    }
  }

  // ---- A phase: this wave's 32 pixel rows -> activated MFMA fragments in registers --------------------------------
  u32x4 afr[KS];
  {
    // staging rows: the output tile if this variant has one, else weight buffer 1 (free until the loop starts)
    unsigned char* stg = HAS_TILE ? tbuf : smem + BUF + wave * (32 * kStagePitch);
    const int srow = lane >> 3, kv = (lane & 7) * 8;  // load mapping: 8 lanes cover one row's 128 bytes
    const int koff1 = g.seg[0].ch, koff2 = g.seg[0].ch + g.seg[1].ch;
    constexpr int NCH = KS / 4;  // 64-channel chunks
    constexpr int PF = NCH < 3 ? NCH : 3;
    u32x4 raw[PF][4];
    f32x4 sc[PF][2], bi[PF][2];
    auto issue = [&](int c, int slot) {
      const int k0 = c * 64;
      const int s = (g.nseg > 1 && k0 >= koff1) + (g.nseg > 2 && k0 >= koff2);
      const GemmSeg sg = g.seg[s];
      const int cl = k0 - (s == 0 ? 0 : (s == 1 ? koff1 : koff2)) + kv;
      const T* base = reinterpret_cast<const T*>(sg.ptr) + (m0 + wave * 32 + srow) * sg.ch + cl;
#pragma unroll
      for (int j = 0; j < 4; ++j) raw[slot][j] = *reinterpret_cast<const u32x4*>(base + (size_t)(8 * j) * sg.ch);
      const float* ps = sg.as + (size_t)img * sg.aff_ld + cl;
      const float* pb = sg.ab + (size_t)img * sg.aff_ld + cl;
      sc[slot][0] = *reinterpret_cast<const f32x4*>(ps);
      sc[slot][1] = *reinterpret_cast<const f32x4*>(ps + 4);
      bi[slot][0] = *reinterpret_cast<const f32x4*>(pb);
      bi[slot][1] = *reinterpret_cast<const f32x4*>(pb + 4);
    };
#pragma unroll
    for (int c = 0; c < PF; ++c) issue(c, c);
#pragma unroll
    for (int c = 0; c < NCH; ++c) {
      const int slot = c % PF;
#pragma unroll
      for (int j = 0; j < 4; ++j) {
        u32x4 o;
#pragma unroll
        for (int q = 0; q < 4; ++q)
          o[q] = act_clamp01_pack<T, true>(raw[slot][j][q], sc[slot][q >> 1][(2 * q) & 3], sc[slot][q >> 1][(2 * q + 1) & 3],
                                           bi[slot][q >> 1][(2 * q) & 3], bi[slot][q >> 1][(2 * q + 1) & 3]);
        *reinterpret_cast<u32x4*>(stg + (srow + 8 * j) * kStagePitch + kv * 2) = o;
      }
      if (c + PF < NCH) issue(c + PF, slot);
      asm volatile("s_waitcnt lgkmcnt(0)" ::: "memory");  // wave-private staging: this wave's own writes, then its reads
#pragma unroll
      for (int q = 0; q < 4; ++q) afr[4 * c + q] = *reinterpret_cast<const u32x4*>(stg + lr * kStagePitch + (16 * q + 8 * lh) * 2);
      asm volatile("s_waitcnt lgkmcnt(0)" ::: "memory");  // fragments read before the next chunk overwrites the rows
    }
  }

  // 0/1 selection matrices of the register transpose: B[k][j] = 1 iff pixel(k) == j, with the pixel order of the packed
  // accumulator words (k = 8 * half + e  <->  accumulator register e (+ 8 for the second MFMA) of that lane half)
  u32x4 id1, id2;
#pragma unroll
  for (int q = 0; q < 4; ++q) {
    uint32_t w1 = 0, w2 = 0;
#pragma unroll
    for (int t = 0; t < 2; ++t) {
      const int e = 2 * q + t;
      const int px = (e & 3) + 8 * (e >> 2) + 4 * lh;
      if (px == lr) w1 |= one_bits<T>() << (16 * t);
      if (px + 16 == lr) w2 |= one_bits<T>() << (16 * t);
    }
    id1[q] = w1;
    id2[q] = w2;
  }
  const uint32_t ones2 = one_bits<T>() | (one_bits<T>() << 16);

  T* outp = reinterpret_cast<T*>(g.out) + (m0 + wave * 32 + lr) * g.N + nbase + lh * 8;
  const int ntiles = tpi;
  auto flush_stats = [&](int it) {  // after a barrier: combine the four waves' partial sums of buffer `it` in wave order
    if constexpr (ACT) {
      // the tile's sum of the channel, times the sum of its weights, parked in the weight sum's own LDS slot (this thread alone
      // touches it): the fixed-point adds leave together at the end.  Issued here they sat in front of every vmcnt wait of wave 0,
      // and the other three waves waited for it at the barrier
      if (tid < NBW * 64 && (tid & 32) == 0) {
        const float* r = red + (size_t)(it & 1) * 4 * NBW * 64 + tid;  // [wave][lane half][channel]
        const float t = (((r[0] + r[32]) + (r[NBW * 64] + r[NBW * 64 + 32])) + (r[2 * NBW * 64] + r[2 * NBW * 64 + 32])) + (r[3 * NBW * 64] + r[3 * NBW * 64 + 32]);
        const int c = (it * NBW + (tid >> 6)) * 32 + (tid & 31);
        swall[2 * kPwxActMaxN + c] *= t;
      }
    } else if (tid < NBW * 64) {
      const float* r = red + (size_t)(it & 1) * 4 * NBW * 64 + tid;
      const float t = ((r[0] + r[NBW * 64]) + r[2 * NBW * 64]) + r[3 * NBW * 64];
      const int j = tid >> 6, which = (tid >> 5) & 1, c = tid & 31;
      g.stats[((size_t)(img * ntiles + tile) * 2 + which) * g.N + nbase + (it * NBW + j) * 32 + c] = t;
    }
  };

  if constexpr (STAMP) t_a = __builtin_amdgcn_s_memtime();
  // buffer 0 has been in flight since the start; buffer 1's slot held the staging rows until here
  asm volatile("s_waitcnt vmcnt(0) lgkmcnt(0)" ::: "memory");
  __builtin_amdgcn_s_barrier();
  if (nit > 1) dma(1);

  for (int it = 0; it < nit; ++it) {
    const unsigned char* wb = smem + (it & 1) * BUF + lane * 16;
    float* redw = red + (size_t)((it & 1) * 4 + wave) * NBW * 64 + lane;
#pragma unroll
    for (int j = 0; j < NBW; ++j) {
      f32x16 acc;
#pragma unroll
      for (int r = 0; r < 16; ++r) acc[r] = 0.f;
      float sc2 = 0.f, sh2 = 0.f;  // ACT: norm2's tables of the lane's channel (LDS), requested ahead of the MFMAs
      if constexpr (ACT) {
        sc2 = swall[(it * NBW + j) * 32 + lr];
        sh2 = swall[kPwxActMaxN + (it * NBW + j) * 32 + lr];
      }
      {
        // the weight fragments run PD reads ahead of their MFMAs (left alone, hipcc issues two reads, waits for both and
        // multiplies twice: at two waves per SIMD the matrix pipe then waits on LDS latency in every pair)
        constexpr int PD = KS >= 32 ? 4 : 6;
        u32x4 wfrag[KS];
#pragma unroll
        for (int s = 0; s < KS; ++s) wfrag[s] = *reinterpret_cast<const u32x4*>(wb + (j * KS + s) * 1024);
#pragma unroll
        for (int s = 0; s < KS; ++s) acc = mfma_u<T>(afr[s], wfrag[s], acc);
        __builtin_amdgcn_sched_group_barrier(0x100, PD, 0);
#pragma unroll
        for (int s = 0; s < KS - PD; ++s) {
          __builtin_amdgcn_sched_group_barrier(0x008, 1, 0);
          __builtin_amdgcn_sched_group_barrier(0x100, 1, 0);
        }
        __builtin_amdgcn_sched_group_barrier(0x008, PD, 0);
      }
      // ---- epilogue of one 32 pixel x 32 channel block (lane = channel lr, registers = 16 pixels) ----
      u32x4 h0, h1;
      if constexpr (ACT) {
#pragma unroll
        for (int q = 0; q < 4; ++q) {
          h0[q] = affine_clamp01_pack<T>(acc[2 * q], acc[2 * q + 1], sc2, sc2, sh2, sh2);
          h1[q] = affine_clamp01_pack<T>(acc[8 + 2 * q], acc[8 + 2 * q + 1], sc2, sc2, sh2, sh2);
        }
        float gs = 0.f;  // the lane's 16 pixels of the channel, as stored
#pragma unroll
        for (int q = 0; q < 4; ++q) {
          gs = dot2<T>(h0[q], ones2, gs);
          gs = dot2<T>(h1[q], ones2, gs);
        }
        redw[j * 64] = gs;
      } else {
#pragma unroll
        for (int q = 0; q < 4; ++q) {
          h0[q] = pack2<T>(acc[2 * q], acc[2 * q + 1]);
          h1[q] = pack2<T>(acc[8 + 2 * q], acc[8 + 2 * q + 1]);
        }
        float s1 = 0.f, s2 = 0.f;
#pragma unroll
        for (int q = 0; q < 4; ++q) {
          s1 = dot2<T>(h0[q], ones2, s1);
          s2 = dot2<T>(h0[q], h0[q], s2);
        }
#pragma unroll
        for (int q = 0; q < 4; ++q) {
          s1 = dot2<T>(h1[q], ones2, s1);
          s2 = dot2<T>(h1[q], h1[q], s2);
        }
        {  // lanes 0-31 end up with the channel's sum, lanes 32-63 with its sum of squares (one half swap)
          const auto r = __builtin_amdgcn_permlane32_swap(__float_as_uint(s1), __float_as_uint(s2), false, false);
          redw[j * 64] = __uint_as_float(r[0]) + __uint_as_float(r[1]);
        }
      }
      f32x16 d2;
#pragma unroll
      for (int r = 0; r < 16; ++r) d2[r] = 0.f;
      d2 = mfma_u<T>(h0, id1, d2);
      d2 = mfma_u<T>(h1, id2, d2);  // lane = pixel lr, register r = channel (r & 3) + 8 (r >> 2) + 4 lh, values exact
      uint32_t o[8];
#pragma unroll
      for (int q = 0; q < 8; ++q) o[q] = pack2<T>(d2[2 * q], d2[2 * q + 1]);
#pragma unroll
      for (int q = 0; q < 8; q += 4) {  // (o[q], o[q+1] | o[q+2], o[q+3]): channels 0-3 | 8-11 (+ 4 lh) of a 16-channel half
        const auto a = __builtin_amdgcn_permlane32_swap(o[q], o[q + 2], false, false);
        const auto b = __builtin_amdgcn_permlane32_swap(o[q + 1], o[q + 3], false, false);
        u32x4 v = {a[0], b[0], a[1], b[1]};  // lower lanes: channels 0-7, upper lanes: channels 8-15 of that half
        if constexpr (LDSOUT) {
          *reinterpret_cast<u32x4*>(tbuf + lr * kStagePitch + (((it * NBW + j) & 1) * 32 + lh * 8 + q * 4) * 2) = v;
        } else {  // straight from registers: 32 rows x 32 bytes per instruction
          *reinterpret_cast<u32x4*>(outp + (it * NBW + j) * 32 + q * 4) = v;
        }
      }
      if constexpr (LDSOUT) {
        if (((it * NBW + j) & 1) == 1) {  // 64 channels of the wave's 32 pixels are in the tile: 4 stores of 8 rows x 128 bytes
          asm volatile("s_waitcnt lgkmcnt(0)" ::: "memory");  // this wave's own writes (the tile is wave-private)
          u32x4 rowv[4];
#pragma unroll
          for (int i = 0; i < 4; ++i) rowv[i] = *reinterpret_cast<const u32x4*>(tbuf + (8 * i + (lane >> 3)) * kStagePitch + (lane & 7) * 16);
          // the reads must have returned before another lane's next write lands on their rows: the compiler orders
          // memory operations per thread only, so pin the order here
          asm volatile("s_waitcnt lgkmcnt(0)" ::: "memory");
          T* orow = reinterpret_cast<T*>(g.out) + (m0 + wave * 32 + (lane >> 3)) * g.N + nbase + ((it * NBW + j) >> 1) * 64 + (lane & 7) * 8;
          if (g.nt) {  // uniform
#pragma unroll
            for (int i = 0; i < 4; ++i) __builtin_nontemporal_store(rowv[i], reinterpret_cast<u32x4*>(orow + (size_t)(8 * i) * g.N));
          } else {
#pragma unroll
            for (int i = 0; i < 4; ++i) *reinterpret_cast<u32x4*>(orow + (size_t)(8 * i) * g.N) = rowv[i];
          }
        }
      }
    }
    if (it + 1 < nit) {  // hand over to the next buffer (kept at the END of the body: a uniform loop, nothing peeled)
      unsigned long long t0 = 0;
      if constexpr (STAMP) t0 = __builtin_amdgcn_s_memtime();
      // the DMA of the next buffer was issued before this buffer's output stores: leave those in flight.
      // (LDSOUT stores 4 instructions per pair of blocks, the direct path 2 per block: 2 * NBW either way, except that
      // with one block per buffer the LDS path stores only behind every second buffer.)
      if constexpr (LDSOUT && NBW == 1) {
        if (it & 1) asm volatile("s_waitcnt vmcnt(4) lgkmcnt(0)" ::: "memory");
        else asm volatile("s_waitcnt vmcnt(0) lgkmcnt(0)" ::: "memory");
      } else {
        asm volatile("s_waitcnt vmcnt(%0) lgkmcnt(0)" ::"n"(2 * NBW) : "memory");
      }
      if constexpr (STAMP) t_wait += __builtin_amdgcn_s_memtime() - t0;
      __builtin_amdgcn_s_barrier();
      flush_stats(it);
      if (it + 2 < nit) dma(it + 2);
    }
  }
  asm volatile("s_waitcnt lgkmcnt(0)" ::: "memory");
  __builtin_amdgcn_s_barrier();
  flush_stats(nit - 1);
  if constexpr (ACT) {  // one fixed-point add per channel and 128-pixel tile: the float order is fixed, the integer adds commute
    wg_barrier();
    for (int c = tid; c < nper; c += 256) fixed_add(g.pool_tot + (size_t)img * g.N + nbase + c, swall[2 * kPwxActMaxN + c], kPoolFixScale);
  }
  if constexpr (STAMP) {
    if (g.stamps && lane == 0) {
      const unsigned long long t_end = __builtin_amdgcn_s_memtime();
      const size_t wv = (size_t)blockIdx.x * 4 + wave;
      g.stamps[3 * wv] = t_a - t_start;
      g.stamps[3 * wv + 1] = t_end - t_a;
      g.stamps[3 * wv + 2] = t_wait;
    }
  }
}
template <typename T, int KS, int NBW, bool REGSTORE = false, bool STAMP = false>
__global__ void __launch_bounds__(256, 2) pw_expand_kernel(const ExpandArgs g) {
  pw_expand_body<T, KS, NBW, REGSTORE, STAMP, false>(g);
}
template <typename T, int KS, int NBW>
__global__ void __launch_bounds__(256, 2) pw_expand_act_kernel(const ExpandArgs g) {
  pw_expand_body<T, KS, NBW, false, false, true>(g);
}

// Weight pack: fp32 [N][K] (OIHW of a 1x1 conv) -> T in MFMA B-fragment order, times `scale`:
//   dst[((nblk * KS + s) * 64 + lane) * 8 + e] = scale * W[32 nblk + (lane & 31)][16 s + 8 (lane >> 5) + e]
template <typename T>
__global__ void pack_expand_kernel(const float* __restrict__ src, T* __restrict__ dst, int N, int K, float scale) {
  const long long i = (long long)blockIdx.x * blockDim.x + threadIdx.x;
  if (i >= (long long)N * K) return;
  dst[pw_expand_pack_index((int)(i / K), (int)(i % K), K)] = (T)(src[i] * scale);
}
hipError_t launch_pack_expand(int dtype, const float* src, void* dst, int N, int K, float scale, hipStream_t s) {
  if (N % 32 || K % 16) return hipErrorInvalidValue;
  const dim3 grid((unsigned)(((long long)N * K + 255) / 256));
  return with_dtype2(dtype, [&](auto t) {
    using T = decltype(t);
    hipLaunchKernelGGL(pack_expand_kernel<T>, grid, dim3(256), 0, s, src, reinterpret_cast<T*>(dst), N, K, scale);
    return hipGetLastError();
  });
}

// 32-channel blocks per LDS buffer.  One everywhere: the smaller LDS footprint (three workgroups per CU up to K = 256) is
// worth more than the saved barriers (measured in round 3: profiles/r03)
constexpr int kPwxNbw = 1;
static int nsplit_for(int M, int N, int nbw) {
  // small grids: split the channels of a pixel tile over workgroups until the chip's 512 slots (2 per CU) are filled
  int ns = 1;
  while ((long)(M / 128) * ns < 512 && (N / (32 * nbw)) % (2 * ns) == 0 && N / (32 * nbw * 2 * ns) >= 2 && (N / (2 * ns)) % 64 == 0) ns *= 2;
  return ns;
}
int pw_expand_nsplit(int M, int N) { return nsplit_for(M, N, kPwxNbw); }
bool pw_expand_serves_k(int K) { return K == 128 || K == 192 || K == 256 || K == 384 || K == 512; }
bool pw_expand_supported(int dtype, const GemmSeg* seg, int nseg, int M, int N, int K, int P) {
  if (!g_knobs.pwx || (dtype != 1 && dtype != 2) || nseg < 1 || nseg > 3 || P % 128 || M % P) return false;
  if (!pw_expand_serves_k(K) || N % (32 * kPwxNbw) || N % 64) return false;  // pairs of 32-channel blocks leave as 128-byte lines
  int k = 0;
  for (int i = 0; i < nseg; ++i) {
    if (!seg[i].ptr || seg[i].ch <= 0 || seg[i].ch % 64 || seg[i].act != ACT_RELU6_S6 || !seg[i].as || !seg[i].ab || seg[i].aff_ld < seg[i].ch) return false;
    k += seg[i].ch;
  }
  return k == K;
}

StampSink g_pwx_stamps{3, 1u << 18};  // s_memtime ticks per wave: {A phase, channel loop, of which in the vmcnt wait at the top of a buffer}

template <typename T, int KS, int NBW, bool REGSTORE = false, bool STAMP = false>
static hipError_t launch_one(ExpandArgs a, hipStream_t s) {
  constexpr int lds = pwx_lds_bytes(KS, NBW, REGSTORE);
  static std::atomic<uint64_t> attr_done{0};
  if (hipError_t e = ensure_max_lds(reinterpret_cast<const void*>(&pw_expand_kernel<T, KS, NBW, REGSTORE, STAMP>), lds, attr_done); e != hipSuccess) return e;
  hipLaunchKernelGGL((pw_expand_kernel<T, KS, NBW, REGSTORE, STAMP>), dim3((unsigned)((a.M / 128) * a.nsplit)), dim3(256), lds, s, a);
  return hipGetLastError();
}
template <typename T, int KS, int NBW = kPwxNbw>
static hipError_t launch_cfg(ExpandArgs a, hipStream_t s) {
  a.nsplit = nsplit_for(a.M, a.N, NBW);
  static const char* const name = kernel_name<T>("pw_expand_kernel", KS, NBW);
  note_kernel(name);
  if constexpr (std::is_same<T, half_t>::value && (KS == 12 || KS == 24)) {  // diagnostics for two representative shapes only
    if (g_knobs.pwx_stamp) {
      if (hipError_t e = g_pwx_stamps.arm((size_t)(a.M / 128) * a.nsplit * 4, &a.stamps); e != hipSuccess) return e;
      return launch_one<T, KS, NBW, false, true>(a, s);
    }
  }
  // K = 512: the LDS tile would leave room for one workgroup per CU only (64 KB of weight buffers): registers -> HBM there
  return launch_one<T, KS, NBW, KS == 32>(a, s);
}
// The border part of the SE pool totals of an ACTIVATED h1 [B][H][W][N]: a tap (ky, kx) of the zero-padded depthwise conv reads pixel
// p + (ky - 1, kx - 1), so summed over the image it misses the far border row and / or column (dwconv3x3_pool_kernel's table).
// pw_expand_act_kernel has added (sum over all pixels) x (sum of the nine weights); this takes the border sums back out.
// grid (4 sides, N / 64, B): side 0 / 1 = first / last row with its two corners, 2 / 3 = first / last column.  Thread (cv = tid & 7,
// pl = tid >> 3) adds the pixels pl, pl + 32, ... of the side for 8 channels; the 32 slots are added in slot order through LDS and
// one fixed-point add per channel leaves: the float order depends on (H, W) alone, the integer adds commute.
template <typename T>
__global__ void __launch_bounds__(256) pool_border_kernel(const T* h1a, const float* wd, unsigned long long* pool_tot, int H, int W, int N) {
  __shared__ float red[32][64];
  const int side = blockIdx.x, cbase = blockIdx.y * 64, b = blockIdx.z, tid = threadIdx.x, cv = tid & 7, pl = tid >> 3;
  const T* img = h1a + (size_t)b * H * W * N + cbase + cv * 8;
  const int n = side < 2 ? W : H;
  const size_t first = side == 0 ? 0 : (side == 1 ? (size_t)(H - 1) * W : (side == 2 ? 0 : (size_t)W - 1));
  const size_t stride = side < 2 ? 1 : (size_t)W;
  float acc[8];
#pragma unroll
  for (int e = 0; e < 8; ++e) acc[e] = 0.f;
  for (int i = pl; i < n; i += 32) {
    float f[8];
    vec_to_f32<T>(ld_vec<T>(img + (first + (size_t)i * stride) * N), f);
#pragma unroll
    for (int e = 0; e < 8; ++e) acc[e] += f[e];
  }
#pragma unroll
  for (int e = 0; e < 8; ++e) red[pl][cv * 8 + e] = acc[e];
  wg_barrier();
  if (tid >= 64) return;
  const int c = cbase + tid;
  float sum = 0.f;
#pragma unroll
  for (int p = 0; p < 32; ++p) sum += red[p][tid];
  float w[9];
#pragma unroll
  for (int tap = 0; tap < 9; ++tap) w[tap] = (float)(T)(6.f * wd[tap * N + c]);
  float t;
  if (side < 2) {  // a row: its taps, and its two corners back in (the column sides take them out a second time)
    const T* row = h1a + ((size_t)b * H * W + first) * N + c;
    const float k0 = (float)row[0], k1 = (float)row[(size_t)(W - 1) * N];
    t = side == 0 ? -sum * ((w[6] + w[7]) + w[8]) : -sum * ((w[0] + w[1]) + w[2]);
    t = __builtin_fmaf(k0, side == 0 ? w[8] : w[2], t);
    t = __builtin_fmaf(k1, side == 0 ? w[6] : w[0], t);
  } else {
    t = side == 2 ? -sum * ((w[2] + w[5]) + w[8]) : -sum * ((w[0] + w[3]) + w[6]);
  }
  fixed_add(pool_tot + (size_t)b * N + c, t, kPoolFixScale);
}

// The activating form: 192 -> 768 only (the block the engine's rule can select)
bool pw_expand_act_supported(int dtype, const GemmSeg* seg, int nseg, int M, int N, int K, int P, int H, int W) {
  return K == 192 && N == 768 && N <= kPwxActMaxN && H > 0 && W > 0 && W % 16 == 0 && H * W == P && pw_expand_supported(dtype, seg, nseg, M, N, K, P);
}
template <typename T>
static hipError_t launch_act_t(ExpandArgs a, hipStream_t s) {
  constexpr int KS = 12, NBW = kPwxNbw, lds = pwx_lds_bytes(KS, NBW, false) + 3 * kPwxActMaxN * 4;
  static_assert(3 * lds <= 160 * 1024, "three workgroups per CU, as pw_expand_kernel<T, 12, 1>");
  a.nsplit = nsplit_for(a.M, a.N, NBW);
  static const char* const name = kernel_name<T>("pw_expand_act_kernel", KS, NBW);
  note_kernel(name);
  static std::atomic<uint64_t> attr_done{0};
  if (hipError_t e = ensure_max_lds(reinterpret_cast<const void*>(&pw_expand_act_kernel<T, KS, NBW>), lds, attr_done); e != hipSuccess) return e;
  hipLaunchKernelGGL((pw_expand_act_kernel<T, KS, NBW>), dim3((unsigned)((a.M / 128) * a.nsplit)), dim3(256), lds, s, a);
  if (hipError_t e = hipGetLastError(); e != hipSuccess) return e;
  hipLaunchKernelGGL((pool_border_kernel<T>), dim3(4, a.N / 64, a.M / a.P), dim3(256), 0, s, reinterpret_cast<const T*>(a.out), a.wd, a.pool_tot, a.H, a.W, a.N);
  return hipGetLastError();
}
// out = T(clamp01((6 W a') as2 + ab2)) and pool_tot += its SE pool totals (fixed point, kPoolFixScale; the caller zeroes it)
hipError_t launch_pw_expand_act(int dtype, const ExpandArgs& a, hipStream_t s) {
  if (!a.wf || !a.out || !a.as2 || !a.ab2 || !a.wd || !a.pool_tot || !pw_expand_act_supported(dtype, a.seg, a.nseg, a.M, a.N, a.K, a.P, a.H, a.W))
    return hipErrorInvalidValue;
  return with_dtype2(dtype, [&](auto t) { return launch_act_t<decltype(t)>(a, s); });
}
hipError_t launch_pw_expand(int dtype, const ExpandArgs& a, hipStream_t s) {
  // host-side shape contract (an out-of-contract shape would index out of bounds on the device)
  if (!a.wf || !a.out || !a.stats || !pw_expand_supported(dtype, a.seg, a.nseg, a.M, a.N, a.K, a.P)) return hipErrorInvalidValue;
  return with_dtype2(dtype, [&](auto t) {
    return with_value<128, 192, 256, 384, 512>(a.K, [&](auto k) { return launch_cfg<decltype(t), decltype(k)::value / 16>(a, s); });
  });
}

}  // namespace llie
