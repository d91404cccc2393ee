// Small / elementwise kernels of the LCM hot path (gfx950): GroupNorm statistics finalisation, SE MLP,
// time embedding + FiLM projections, linear-attention core, layout conversion, weight repack and the
// LCM scheduler's elementwise step.  All reductions use fixed orders (bitwise reproducible).
#include "common.h"
#include "kernels.h"

namespace llie {

static thread_local const char* g_last_kernel = "";
void note_kernel(const char* name) { g_last_kernel = name; }
const char* last_kernel() { return g_last_kernel; }

// =============================================================================================
// GroupNorm finalize: slabs of per-channel (sum, sumsq) -> per-(image, channel) affine.
// nn.GroupNorm(min(32,C), C) call sites: efficient_unet.py:170-171,263,268,528 (biased variance,
// eps 1e-5); FiLM fold: efficient_unet.py:215-217  h*(1+scale)+shift after norm2's own affine.
// One 4-wave block per (image, group); tile partials are fp32, the cross-tile combination is fp64
// in a fixed order.
__global__ void __launch_bounds__(256) gn_finalize_kernel(const GnFinalizeArgs a) {
  __shared__ double part[2][4];
  const int g = blockIdx.x, b = blockIdx.y, tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
  // groups partition the REAL channels [0, Creal); channels beyond (zero padding of the unpinned variants, always
  // at the end of the tensor / of the second concat segment) get a zero affine so they stay zero
  const int Creal = a.Creal > 0 ? a.Creal : a.C;
  const int cg = Creal / a.groups;
  const int c_lo = g * cg;
  if (g == 0)
    for (int c = Creal + tid; c < a.C; c += 256) {
      a.as[(size_t)b * a.C + c] = 0.f;
      a.ab[(size_t)b * a.C + c] = 0.f;
    }
  // This kernel sits between two big launches 188 times per 4-step call and is pure latency: everything that does not
  // depend on the statistics (norm affine, FiLM row) is fetched up front, and the slab is read with eight independent
  // loads in flight per thread instead of one dependent load per tile (one memory round trip instead of up to 13).
  float p_ga = 0.f, p_be = 0.f, p_fs = 0.f, p_fh = 0.f;
  if (tid < cg) {  // cg <= 64 in every network of this engine (2048 / 32); wider groups take the loop at the end
    p_ga = a.gamma[c_lo + tid];
    p_be = a.beta[c_lo + tid];
    if (a.film) {
      const float* f = a.film + (size_t)b * a.film_stride;
      p_fs = f[c_lo + tid];
      p_fh = f[Creal + c_lo + tid];
    }
  }
  double s1 = 0.0, s2 = 0.0;
  int coff = 0;
  for (int s = 0; s < 2; ++s) {
    const StatSrc src = a.src[s];
    if (!src.slab) continue;
    // channels of this group that live in this source: [lo, hi) in source-local numbering
    const int lo = max(c_lo - coff, 0), hi = min(c_lo + cg - coff, src.ch);
    if (hi > lo) {
      // thread -> (tile lane tl, channel c): consecutive threads read consecutive channels of one
      // tile row (coalesced), then stride over tiles; no division inside the loop
      const int w = hi - lo;
      const int per = w <= 256 ? 256 / w : 1;       // tiles covered per sweep of the block
      const int tl = w <= 256 ? tid / w : 0, cc = w <= 256 ? tid % w : tid;
      const float* base = src.slab + (size_t)b * src.ntiles * 2 * src.ch + lo;
      if (w <= 256) {
        if (tl < per) {
          // four tiles (eight loads) per trip; the partial sums are combined in tile order, so the result does not
          // depend on the unrolling
          int t = tl;
          for (; t + 3 * per < src.ntiles; t += 4 * per) {
            float v[8];
#pragma unroll
            for (int u = 0; u < 4; ++u) {
              v[2 * u] = base[(size_t)((t + u * per) * 2 + 0) * src.ch + cc];
              v[2 * u + 1] = base[(size_t)((t + u * per) * 2 + 1) * src.ch + cc];
            }
#pragma unroll
            for (int u = 0; u < 4; ++u) {
              s1 += (double)v[2 * u];
              s2 += (double)v[2 * u + 1];
            }
          }
          for (; t < src.ntiles; t += per) {
            s1 += (double)base[(size_t)(t * 2 + 0) * src.ch + cc];
            s2 += (double)base[(size_t)(t * 2 + 1) * src.ch + cc];
          }
        }
      } else {
        for (int t = 0; t < src.ntiles; ++t)
          for (int c = tid; c < w; c += 256) {
            s1 += (double)base[(size_t)(t * 2 + 0) * src.ch + c];
            s2 += (double)base[(size_t)(t * 2 + 1) * src.ch + c];
          }
      }
    }
    coff += src.ch;
  }
  s1 = wave_sum(s1);
  s2 = wave_sum(s2);
  if (lane == 0) {
    part[0][wave] = s1;
    part[1][wave] = s2;
  }
  wg_barrier();
  s1 = (part[0][0] + part[0][1]) + (part[0][2] + part[0][3]);
  s2 = (part[1][0] + part[1][1]) + (part[1][2] + part[1][3]);
  const double n = (double)cg * (double)a.P;
  const double mean = s1 / n;
  double var = s2 / n - mean * mean;
  if (var < 0.0) var = 0.0;
  const float rstd = (float)(1.0 / sqrt(var + (double)a.eps));
  const float fmean = (float)mean;
  if (a.mean_out && tid == 0) {
    a.mean_out[(size_t)b * a.groups + g] = fmean;
    a.rstd_out[(size_t)b * a.groups + g] = rstd;
  }
  for (int i = tid; i < cg; i += 256) {
    const int c = c_lo + i;
    float gam = p_ga, bet = p_be, ffs = p_fs, ffh = p_fh;
    if (i >= 256) {  // groups wider than the block (not reached by the reference's variants)
      gam = a.gamma[c]; bet = a.beta[c];
      if (a.film) {
        const float* f = a.film + (size_t)b * a.film_stride;
        ffs = f[c]; ffh = f[Creal + c];
      }
    }
    const float ga = gam * rstd;
    float sc = ga, sh = bet - fmean * ga;
    if (a.film) {
      const float fs = 1.f + ffs, fh = ffh;
      sc *= fs;
      sh = sh * fs + fh;
    }
    if (a.post_scale != 0.f) {
      sc *= a.post_scale;
      sh *= a.post_scale;
    }
    a.as[(size_t)b * a.C + c] = sc;
    a.ab[(size_t)b * a.C + c] = sh;
  }
}

hipError_t launch_gn_finalize(const GnFinalizeArgs& a, hipStream_t s) {
  if (a.groups <= 0 || a.P <= 0 || a.B <= 0 || a.Creal > a.C || (a.Creal > 0 ? a.Creal : a.C) % a.groups) return hipErrorInvalidValue;
  for (int i = 0; i < 2; ++i)
    if (a.src[i].slab && (a.src[i].ntiles <= 0 || a.src[i].ch <= 0)) return hipErrorInvalidValue;
  int c = 0;
  for (int i = 0; i < 2; ++i)
    if (a.src[i].slab) c += a.src[i].ch;
  if (c != a.C) return hipErrorInvalidValue;
  hipLaunchKernelGGL(gn_finalize_kernel, dim3(a.groups, a.B), dim3(256), 0, s, a);
  return hipGetLastError();
}

// =============================================================================================
// Squeeze-and-Excitation MLP (efficient_unet.py:96-100); fc1/fc2 are 1x1 convs on a 1x1 map,
// i.e. two skinny GEMMs over the batch.  One wave per output row, all images looped inside so each
// weight row is read once per launch.
constexpr int kSeMaxB = 4;  // images per pass held in registers / LDS

// pool partials [B][ntiles][C] -> mean[B][C]: one block per (64 channels, image).  Thread t owns a
// float4 of channels (t & 15) and a tile group (t >> 4): 16 groups stride over the tiles with 16-byte
// loads; the 16 partial sums per channel are combined through LDS in a fixed order.
__global__ void __launch_bounds__(256) se_pool_kernel(const SeArgs a) {
  __shared__ float part[16][64];
  const int tid = threadIdx.x, c4 = tid & 15, tg = tid >> 4;
  const int c = blockIdx.x * 64 + c4 * 4, b = blockIdx.y;
  f32x4 s = {0.f, 0.f, 0.f, 0.f};
  if (c < a.C) {
    const int ps = a.pool_stride ? a.pool_stride : a.C;
    const float* p = a.pool + (size_t)b * a.ntiles * ps + c;
    for (int t = tg; t < a.ntiles; t += 16) s += *reinterpret_cast<const f32x4*>(p + (size_t)t * ps);
  }
#pragma unroll
  for (int e = 0; e < 4; ++e) part[tg][c4 * 4 + e] = s[e];
  wg_barrier();
  if (tid < 64 && blockIdx.x * 64 + tid < a.C) {
    float t = 0.f;
#pragma unroll
    for (int g = 0; g < 16; ++g) t += part[g][tid];
    a.mean[(size_t)b * a.C + blockIdx.x * 64 + tid] = t * (1.f / (float)a.P);
  }
}

constexpr int kSeRows = 4;  // output rows per block = waves per block

// dot products of one weight row (K contiguous T elements, 16-byte vector loads) with kSeMaxB fp32
// vectors held in LDS; wave-wide, every lane gets the totals.  These kernels are pure latency (a few KB of weights per wave
// between two big launches, 24 times per forward): the row's vectors -- at most kSeRowVecs per lane, K <= 64 VEC kSeRowVecs =
// 2 048 for 2-byte T, every network of this engine -- are all requested before the first is used (one memory round trip per
// row instead of one per 512 channels); the summation order is the loop's.
constexpr int kSeRowVecs = 4;
template <typename T>
struct SeRow {  // the vectors of one weight row held by this lane
  typename Elem<T>::vec_t wv[kSeRowVecs];
  bool pre;
};
template <typename T>
__device__ __forceinline__ void se_row_fetch(SeRow<T>& r, const T* wrow, int K, int lane) {
  constexpr int VEC = Elem<T>::VEC;
  const int kvec = K / VEC * VEC;
  r.pre = kvec <= 64 * VEC * kSeRowVecs;
  if (r.pre) {
#pragma unroll
    for (int u = 0; u < kSeRowVecs; ++u)
      if ((lane + 64 * u) * VEC < kvec) r.wv[u] = ld_vec<T>(wrow + (lane + 64 * u) * VEC);
  }
}
template <typename T>
__device__ __forceinline__ void se_row_dots(const SeRow<T>& r, const T* wrow, const float* vecs, int K, int nb, int lane, float* out) {
  constexpr int VEC = Elem<T>::VEC;
  typedef typename Elem<T>::vec_t vec_t;
  float acc[kSeMaxB];
#pragma unroll
  for (int q = 0; q < kSeMaxB; ++q) acc[q] = 0.f;
  const int kvec = K / VEC * VEC;
  auto use = [&](const vec_t& wv, int k) {
    float w[VEC];
    vec_to_f32<T>(wv, w);
#pragma unroll
    for (int q = 0; q < kSeMaxB; ++q)
      if (q < nb) {
#pragma unroll
        for (int e = 0; e < VEC; ++e) acc[q] += w[e] * vecs[q * K + k + e];
      }
  };
  if (r.pre) {
#pragma unroll
    for (int u = 0; u < kSeRowVecs; ++u)
      if ((lane + 64 * u) * VEC < kvec) use(r.wv[u], (lane + 64 * u) * VEC);
  } else {
    for (int k = lane * VEC; k < kvec; k += 64 * VEC) use(ld_vec<T>(wrow + k), k);
  }
  for (int k = kvec + lane; k < K; k += 64) {  // tail (K not a multiple of the vector width)
    const float w = (float)wrow[k];
#pragma unroll
    for (int q = 0; q < kSeMaxB; ++q)
      if (q < nb) acc[q] += w * vecs[q * K + k];
  }
#pragma unroll
  for (int q = 0; q < kSeMaxB; ++q) out[q] = wave_sum(acc[q]);
}

// One output row per wave; the row's weights are requested first, so they travel while the block stages its operand.
template <typename T>
__global__ void __launch_bounds__(256) se_fc1_kernel(const SeArgs a) {
  extern __shared__ float smean[];  // [nb][C] means of this block's image chunk
  const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
  const int b0 = blockIdx.y * kSeMaxB, nb = min(kSeMaxB, a.B - b0);
  const T* w1 = reinterpret_cast<const T*>(a.w1);
  const int j = blockIdx.x * kSeRows + wave;
  SeRow<T> row;
  float bj = 0.f;
  if (j < a.Cs) {
    se_row_fetch<T>(row, w1 + (size_t)j * a.C, a.C, lane);
    bj = a.b1[j];
  }
  if (a.tot) {  // fixed-point channel totals straight from the depthwise kernel: no pool pass
    const double inv = 1.0 / ((double)a.P * (double)kPoolFixScale);
    for (int i = tid; i < nb * a.C; i += 256) smean[i] = (float)((double)(long long)a.tot[(size_t)b0 * a.C + i] * inv);
  } else {
    for (int i = tid; i < nb * a.C; i += 256) smean[i] = a.mean[(size_t)b0 * a.C + i];
  }
  wg_barrier();
  if (j >= a.Cs) return;
  float v[kSeMaxB];
  se_row_dots<T>(row, w1 + (size_t)j * a.C, smean, a.C, nb, lane, v);
#pragma unroll
  for (int q = 0; q < kSeMaxB; ++q)
    if (q < nb && lane == 0) a.hid[(size_t)(b0 + q) * a.Cs + j] = relu6f(v[q] + bj);
}

template <typename T>
__global__ void __launch_bounds__(256) se_fc2_kernel(const SeArgs a) {
  extern __shared__ float shid[];  // [nb][Cs]
  const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
  const int b0 = blockIdx.y * kSeMaxB, nb = min(kSeMaxB, a.B - b0);
  const T* w2 = reinterpret_cast<const T*>(a.w2);
  const int c = blockIdx.x * kSeRows + wave;
  SeRow<T> row;
  float bc = 0.f;
  if (c < a.C) {
    se_row_fetch<T>(row, w2 + (size_t)c * a.Cs, a.Cs, lane);
    bc = a.b2[c];
  }
  for (int i = tid; i < nb * a.Cs; i += 256) shid[i] = a.hid[(size_t)b0 * a.Cs + i];
  wg_barrier();
  if (c >= a.C) return;
  float v[kSeMaxB];
  se_row_dots<T>(row, w2 + (size_t)c * a.Cs, shid, a.Cs, nb, lane, v);
#pragma unroll
  for (int q = 0; q < kSeMaxB; ++q)
    if (q < nb && lane == 0) a.gate[(size_t)(b0 + q) * a.C + c] = sigmoidf(v[q] + bc);
}

// Inference form of the whole SE branch in one launch.  The depthwise kernels leave fixed-point channel totals
// (DwArgs::pool_tot) instead of a slab of tile partials, so the mean is one conversion per channel.  Grid (G, B): every
// workgroup of an image redoes fc1 + ReLU6 (weights come from L2; a 16-lane group per hidden row, eight 16-byte loads in
// flight per lane -- with one workgroup per image and dependent loads the big layers took 60-200 us of pure latency) and
// then owns C / G channels of fc2 + sigmoid (a thread per channel).  Sums run in an order fixed by (C, Cs) alone.
// Used up to 384 channels (7-14 us against 20-38 for the three launches below); beyond that one workgroup per image is
// slower than the row-parallel pair se_fc1 / se_fc2 (which then read the totals too, without the pool pass).
template <typename T>
__global__ void __launch_bounds__(1024) se_gate_kernel(const SeArgs a) {
  extern __shared__ float sm[];  // [C] means, [Cs] hidden
  float* mean = sm;
  float* hid = sm + a.C;
  constexpr int VEC = Elem<T>::VEC;
  typedef typename Elem<T>::vec_t vec_t;
  const int b = blockIdx.y, tid = threadIdx.x;
  const double inv = 1.0 / ((double)a.P * (double)kPoolFixScale);
  for (int c = tid; c < a.C; c += 1024) mean[c] = (float)((double)(long long)a.tot[(size_t)b * a.C + c] * inv);
  wg_barrier();
  {  // fc1: row j by lane group (tid >> 4); lane gl takes vectors gl, gl + 16, ... of the row
    const T* w1 = reinterpret_cast<const T*>(a.w1);
    const int gi = tid >> 4, gl = tid & 15;
    const int its = a.C / (16 * VEC);  // launcher: C % (16 VEC) == 0
    for (int j = gi; j < a.Cs; j += 64) {
      const T* wr = w1 + (size_t)j * a.C + gl * VEC;
      float acc = 0.f;
      for (int i0 = 0; i0 < its; i0 += 8) {
        vec_t w[8];
#pragma unroll
        for (int u = 0; u < 8; ++u)
          if (i0 + u < its) w[u] = ld_vec<T>(wr + (size_t)(i0 + u) * 16 * VEC);
#pragma unroll
        for (int u = 0; u < 8; ++u)
          if (i0 + u < its) {
            float f[VEC];
            vec_to_f32<T>(w[u], f);
            const float* mv = mean + (i0 + u) * 16 * VEC + gl * VEC;
#pragma unroll
            for (int e = 0; e < VEC; ++e) acc += f[e] * mv[e];
          }
      }
#pragma unroll
      for (int o = 8; o > 0; o >>= 1) acc += __shfl_xor(acc, o, 64);
      if (gl == 0) hid[j] = relu6f(acc + a.b1[j]);
    }
  }
  wg_barrier();
  const T* w2 = reinterpret_cast<const T*>(a.w2);
  const int cs = a.C / gridDim.x;
  for (int cc = tid; cc < cs; cc += 1024) {
    const int c = blockIdx.x * cs + cc;
    const T* wr = w2 + (size_t)c * a.Cs;
    float acc = 0.f;
    if (a.Cs % VEC == 0) {
      const int nv = a.Cs / VEC;
      for (int i0 = 0; i0 < nv; i0 += 8) {
        vec_t w[8];
#pragma unroll
        for (int u = 0; u < 8; ++u)
          if (i0 + u < nv) w[u] = ld_vec<T>(wr + (i0 + u) * VEC);
#pragma unroll
        for (int u = 0; u < 8; ++u)
          if (i0 + u < nv) {
            float f[VEC];
            vec_to_f32<T>(w[u], f);
#pragma unroll
            for (int e = 0; e < VEC; ++e) acc += f[e] * hid[(i0 + u) * VEC + e];
          }
      }
    } else {
      for (int k = 0; k < a.Cs; ++k) acc += (float)wr[k] * hid[k];
    }
    a.gate[(size_t)b * a.C + c] = sigmoidf(acc + a.b2[c]);
  }
}
// SE MLP of the wide blocks (more than 384 hidden channels) on the matrix pipe, 2-byte T: the batch is the 32 rows of one
// 32x32x16 tile.  The row-parallel pair above re-stages the means in every one of its 500+ workgroups and spends two
// dependent launches of 10-25 us on ~1 MFLOP per image; here
//   fc1: grid (Cs / 32 column blocks, K slices): a wave turns its slice of the fixed-point pool totals into fp16 means in
//        registers (its A fragments), loads its W1 fragments straight from HBM / L2 (the [Cs][C] rows ARE B fragments), runs
//        4 MFMAs and adds its 32 x 32 partial products as 2^-32 fixed-point 64-bit integers into pre[B][Cs] (zero at launch;
//        integer adds commute: bitwise reproducible, and a row = an image, so batch-invariant);
//   fc2: grid (C / 32): A = relu6(pre + b1) rebuilt per wave slice of Cs, B = W2 rows, the four waves' partial tiles summed in
//        wave order through LDS, sigmoid, gate.
// Every global operand of a wave is requested before the first is used: one memory round trip per launch.
constexpr float kSePreScale = 4294967296.f;  // 2^32
template <typename T>
__global__ void __launch_bounds__(256) se_fc1_mfma_kernel(const SeArgs a, const int kw /* K per wave */) {
  static_assert(sizeof(T) == 2, "");
  typedef typename Elem<T>::vec_t vec_t;
  constexpr int MAXS = 4;  // k-steps per wave (launcher: kw <= 64)
  const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6, lr = lane & 31, lh = lane >> 5;
  const int n0 = blockIdx.x * 32, b0 = blockIdx.z * 32;
  const int nb = a.B - b0 < 32 ? a.B - b0 : 32;
  const int k0 = (blockIdx.y * 4 + wave) * kw + 8 * lh;
  const int steps = kw >> 4;
  const T* wrow = reinterpret_cast<const T*>(a.w1) + (size_t)(n0 + lr) * a.C + k0;
  const unsigned long long* trow = a.tot + (size_t)(b0 + lr) * a.C + k0;
  const bool live = lr < nb;
  vec_t wf[MAXS];
  u32x4 tq[MAXS][4];  // 8 totals of 8 bytes per step
#pragma unroll
  for (int s = 0; s < MAXS; ++s)
    if (s < steps) {
      wf[s] = ld_vec<T>(wrow + 16 * s);
#pragma unroll
      for (int q = 0; q < 4; ++q) tq[s][q] = live ? *reinterpret_cast<const u32x4*>(trow + 16 * s + 2 * q) : u32x4{0u, 0u, 0u, 0u};
    }
  const float inv = 1.f / ((float)a.P * kPoolFixScale);
  f32x16 acc;
#pragma unroll
  for (int r = 0; r < 16; ++r) acc[r] = 0.f;
#pragma unroll
  for (int s = 0; s < MAXS; ++s)
    if (s < steps) {
      vec_t av;
#pragma unroll
      for (int q = 0; q < 4; ++q) {
        const long long t0 = (long long)(((unsigned long long)tq[s][q][1] << 32) | tq[s][q][0]);
        const long long t1 = (long long)(((unsigned long long)tq[s][q][3] << 32) | tq[s][q][2]);
        av[2 * q] = (T)((float)t0 * inv);
        av[2 * q + 1] = (T)((float)t1 * inv);
      }
      acc = mfma16<T>(av, wf[s], acc);
    }
#pragma unroll
  for (int r = 0; r < 16; ++r) {
    const int b = mfma_row(r, lane);  // image of this accumulator register; column = lr
    if (b < nb) atomicAdd(reinterpret_cast<unsigned long long*>(a.pre) + (size_t)(b0 + b) * a.Cs + n0 + lr, (unsigned long long)__float2ll_rn(acc[r] * kSePreScale));
  }
}
template <typename T>
__global__ void __launch_bounds__(256) se_fc2_mfma_kernel(const SeArgs a) {
  static_assert(sizeof(T) == 2, "");
  typedef typename Elem<T>::vec_t vec_t;
  constexpr int MAXS = 8;  // k-steps per wave (launcher: Cs <= 512)
  __shared__ float part[4][32 * 33];
  const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6, lr = lane & 31, lh = lane >> 5;
  const int n0 = blockIdx.x * 32, b0 = blockIdx.y * 32;
  const int nb = a.B - b0 < 32 ? a.B - b0 : 32;
  const int kw = a.Cs >> 2, steps = kw >> 4;
  const int k0 = wave * kw + 8 * lh;
  const T* wrow = reinterpret_cast<const T*>(a.w2) + (size_t)(n0 + lr) * a.Cs + k0;
  const long long* prow = a.pre + (size_t)(b0 + lr) * a.Cs + k0;
  const bool live = lr < nb;
  vec_t wf[MAXS];
  u32x4 pq[MAXS][4];
  f32x4 bq[MAXS][2];
#pragma unroll
  for (int s = 0; s < MAXS; ++s)
    if (s < steps) {
      wf[s] = ld_vec<T>(wrow + 16 * s);
#pragma unroll
      for (int q = 0; q < 4; ++q) pq[s][q] = live ? *reinterpret_cast<const u32x4*>(prow + 16 * s + 2 * q) : u32x4{0u, 0u, 0u, 0u};
      bq[s][0] = *reinterpret_cast<const f32x4*>(a.b1 + k0 + 16 * s);
      bq[s][1] = *reinterpret_cast<const f32x4*>(a.b1 + k0 + 16 * s + 4);
    }
  const float bc = a.b2[n0 + lr];
  f32x16 acc;
#pragma unroll
  for (int r = 0; r < 16; ++r) acc[r] = 0.f;
  constexpr float unscale = 1.f / kSePreScale;
#pragma unroll
  for (int s = 0; s < MAXS; ++s)
    if (s < steps) {
      vec_t av;
#pragma unroll
      for (int q = 0; q < 4; ++q) {
        const long long t0 = (long long)(((unsigned long long)pq[s][q][1] << 32) | pq[s][q][0]);
        const long long t1 = (long long)(((unsigned long long)pq[s][q][3] << 32) | pq[s][q][2]);
        const float h0 = live ? relu6f((float)t0 * unscale + bq[s][q >> 1][(2 * q) & 3]) : 0.f;
        const float h1 = live ? relu6f((float)t1 * unscale + bq[s][q >> 1][(2 * q + 1) & 3]) : 0.f;
        av[2 * q] = (T)h0;
        av[2 * q + 1] = (T)h1;
      }
      acc = mfma16<T>(av, wf[s], acc);
    }
#pragma unroll
  for (int r = 0; r < 16; ++r) part[wave][mfma_row(r, lane) * 33 + lr] = acc[r];
  wg_barrier();
  for (int i = tid; i < 32 * 32; i += 256) {
    const int b = i >> 5, n = i & 31;
    if (b < nb) {
      const float v = ((part[0][b * 33 + n] + part[1][b * 33 + n]) + part[2][b * 33 + n]) + part[3][b * 33 + n];
      a.gate[(size_t)(b0 + b) * a.C + n0 + n] = sigmoidf(v + a.b2[n0 + n]);
    }
  }
  (void)bc;
}
bool se_mlp_mfma_supported(int dtype, const SeArgs& a) {
  if ((dtype != 1 && dtype != 2) || !a.tot || !a.pre || !a.gate || a.B <= 0 || a.P <= 0) return false;
  return a.C % 256 == 0 && a.C >= 512 && a.Cs % 64 == 0 && a.Cs >= 64 && a.Cs <= 512;
}
hipError_t launch_se_mlp_mfma(int dtype, const SeArgs& a, hipStream_t s) {
  if (!se_mlp_mfma_supported(dtype, a)) return hipErrorInvalidValue;
  note_kernel("se_fc1_mfma_kernel+se_fc2_mfma_kernel");
  const int ksl = a.C / 256, kw = 64;  // 256 channels of K per workgroup, 64 per wave (4 k-steps)
  const dim3 g1(a.Cs / 32, ksl, (a.B + 31) / 32), g2(a.C / 32, (a.B + 31) / 32);
  return with_dtype2(dtype, [&](auto t) {
    using T = decltype(t);
    hipLaunchKernelGGL(se_fc1_mfma_kernel<T>, g1, dim3(256), 0, s, a, kw);
    hipLaunchKernelGGL(se_fc2_mfma_kernel<T>, g2, dim3(256), 0, s, a);
    return hipGetLastError();
  });
}

hipError_t launch_se_gate(int dtype, const SeArgs& a, hipStream_t s) {
  if (!a.tot || !a.gate || a.C <= 0 || a.Cs <= 0 || a.P <= 0) return hipErrorInvalidValue;
  const int vec = dtype == 0 ? 4 : 8;
  const size_t lds = (size_t)(a.C + a.Cs) * 4;
  if (lds > 48 * 1024 || a.C % (16 * vec)) return hipErrorInvalidValue;
  int G = a.C / 256;  // fc2 channels per workgroup
  if (G < 1) G = 1;
  while (a.C % G) --G;
  note_kernel("se_gate_kernel");
  return with_dtype(dtype, [&](auto t) {
    hipLaunchKernelGGL(se_gate_kernel<decltype(t)>, dim3(G, a.B), dim3(1024), lds, s, a);
    return hipGetLastError();
  });
}

hipError_t launch_se_fc1(int dtype, const SeArgs& a, hipStream_t s) {
  note_kernel(a.tot ? "se_fc1_kernel+se_fc2_kernel" : "se_pool_kernel+se_fc1_kernel+se_fc2_kernel");
  if (!a.tot) hipLaunchKernelGGL(se_pool_kernel, dim3((a.C + 63) / 64, a.B), dim3(256), 0, s, a);
  dim3 grid((a.Cs + kSeRows - 1) / kSeRows, (a.B + kSeMaxB - 1) / kSeMaxB);
  const size_t lds = (size_t)kSeMaxB * a.C * 4;
  return with_dtype(dtype, [&](auto t) {
    hipLaunchKernelGGL(se_fc1_kernel<decltype(t)>, grid, dim3(256), lds, s, a);
    return hipGetLastError();
  });
}
hipError_t launch_se_fc2(int dtype, const SeArgs& a, hipStream_t s) {
  dim3 grid((a.C + kSeRows - 1) / kSeRows, (a.B + kSeMaxB - 1) / kSeMaxB);
  const size_t lds = (size_t)kSeMaxB * a.Cs * 4;
  return with_dtype(dtype, [&](auto t) {
    hipLaunchKernelGGL(se_fc2_kernel<decltype(t)>, grid, dim3(256), lds, s, a);
    return hipGetLastError();
  });
}

// =============================================================================================
// Time embedding: SinusoidalPosEmb (efficient_unet.py:68-76: [cos|sin], freqs exp(-ln(1e4)*i/half),
// fp32 always) -> Linear -> SiLU -> Linear (:412-417).  One block per row.
__global__ void __launch_bounds__(256) time_embed_kernel(const TimeArgs a) {
  extern __shared__ float sm[];  // [dim] emb, [T] hidden
  float* emb = sm;
  float* hid = sm + a.dim;
  const int r = blockIdx.x, tid = threadIdx.x;
  const float t = (float)a.t[r];
  const int half = a.dim / 2;
  for (int i = tid; i < half; i += 256) {
    const float arg = t * a.freqs[i];  // fp32 product like t[:, None].float() * freqs[None] (:74)
    emb[i] = cosf(arg);
    emb[half + i] = sinf(arg);
    if (a.emb_out) {
      a.emb_out[(size_t)r * a.dim + i] = emb[i];
      a.emb_out[(size_t)r * a.dim + half + i] = emb[half + i];
    }
  }
  wg_barrier();
  for (int j = tid; j < a.T; j += 256) {
    float acc = a.b1[j];
    for (int k = 0; k < a.dim; ++k) acc += a.w1[(size_t)j * a.dim + k] * emb[k];
    hid[j] = siluf(acc);
  }
  wg_barrier();
  for (int j = tid; j < a.T; j += 256) {
    float acc = a.b3[j];
    for (int k = 0; k < a.T; ++k) acc += a.w3[(size_t)j * a.T + k] * hid[k];
    a.temb[(size_t)r * a.T + j] = acc;
    a.silu_temb[(size_t)r * a.T + j] = siluf(acc);
  }
}
hipError_t launch_time_embed(const TimeArgs& a, hipStream_t s) {
  hipLaunchKernelGGL(time_embed_kernel, dim3(a.rows), dim3(256), (size_t)(a.dim + a.T) * 4, s, a);
  return hipGetLastError();
}

// All per-block FiLM Linears (efficient_unet.py:189-192,215) concatenated along the output dim:
// film[r][f] = bf[f] + Wf[f][:] . silu(temb[r]).  16 lanes per output row, 4 rows per wave step.
__global__ void __launch_bounds__(256) film_kernel(const FilmArgs a) {
  extern __shared__ float st[];  // [rows_chunk][T]
  const int tid = threadIdx.x;
  const int r0 = blockIdx.y * kSeMaxB, nr = min(kSeMaxB, a.rows - r0);
  for (int i = tid; i < nr * a.T; i += 256) st[i] = a.silu_temb[(size_t)r0 * a.T + i];
  wg_barrier();
  const int sub = tid & 15;
  const int f = blockIdx.x * 16 + (tid >> 4);
  if (f >= a.F) return;  // whole 16-lane group exits together; no block-level sync follows
  float acc[kSeMaxB];
#pragma unroll
  for (int q = 0; q < kSeMaxB; ++q) acc[q] = 0.f;
  for (int k = sub; k < a.T; k += 16) {
    const float w = a.wf[(size_t)f * a.T + k];
#pragma unroll
    for (int q = 0; q < kSeMaxB; ++q)
      if (q < nr) acc[q] += w * st[q * a.T + k];
  }
#pragma unroll
  for (int q = 0; q < kSeMaxB; ++q) {
    float v = acc[q];
#pragma unroll
    for (int o = 8; o > 0; o >>= 1) v += __shfl_xor(v, o, 64);
    if (q < nr && sub == 0) a.film[(size_t)(r0 + q) * a.F + f] = v + a.bf[f];
  }
}
hipError_t launch_film(const FilmArgs& a, hipStream_t s) {
  dim3 grid((a.F + 15) / 16, (a.rows + kSeMaxB - 1) / kSeMaxB);
  hipLaunchKernelGGL(film_kernel, grid, dim3(256), (size_t)kSeMaxB * a.T * 4, s, a);
  return hipGetLastError();
}

__global__ void silu_rows_kernel(const float* in, float* out, int64_t n) {
  const int64_t i = (int64_t)blockIdx.x * blockDim.x + threadIdx.x;
  if (i < n) out[i] = siluf(in[i]);
}
hipError_t launch_silu_rows(const float* in, float* out, int64_t n, hipStream_t s) {
  hipLaunchKernelGGL(silu_rows_kernel, dim3((unsigned)((n + 255) / 256)), dim3(256), 0, s, in, out, n);
  return hipGetLastError();
}

// =============================================================================================
// Linear attention core (efficient_unet.py:288-302).  qkv rows are [q | k | v], each head-major
// (heads d) (:284-286).  phi(x) = elu(x)+1 on q and k only.
__device__ __forceinline__ float phi(float x) { return x > 0.f ? x + 1.f : __expf(x); }

// pass 1: kv[d][e] = sum_n phi(k[n][d]) v[n][e], ksum[d] = sum_n phi(k[n][d]); one block per
// (head, image, position split): the splits keep small batches from running on a handful of CUs.
template <typename T>
__global__ void __launch_bounds__(256) linattn_kv_kernel(const AttnArgs a) {
  constexpr int CH = 64;  // positions per staged chunk
  __shared__ float sk[CH][33], sv[CH][33];
  const int h = blockIdx.x, b = blockIdx.y, sp = blockIdx.z, tid = threadIdx.x;
  const int inner = a.heads * 32, ld = 3 * inner;
  const T* base = reinterpret_cast<const T*>(a.qkv) + (size_t)b * a.N * ld;
  const int d = tid >> 3, e0 = (tid & 7) * 4;
  float acc[4] = {0.f, 0.f, 0.f, 0.f}, ks = 0.f;
  const int span = a.N / a.nsplit;
  for (int n0 = sp * span; n0 < (sp + 1) * span; n0 += CH) {
    for (int i = tid; i < CH * 32; i += 256) {
      const int n = i >> 5, c = i & 31;
      const bool ok = n0 + n < (sp + 1) * span;  // last chunk of a span that is not a multiple of 64 positions: zero contribution
      const T* row = base + (size_t)(ok ? n0 + n : 0) * ld;
      sk[n][c] = ok ? phi((float)row[inner + h * 32 + c]) : 0.f;
      sv[n][c] = ok ? (float)row[2 * inner + h * 32 + c] : 0.f;
    }
    wg_barrier();
#pragma unroll 8
    for (int n = 0; n < CH; ++n) {
      const float kd = sk[n][d];
      ks += kd;
#pragma unroll
      for (int q = 0; q < 4; ++q) acc[q] += kd * sv[n][e0 + q];
    }
    wg_barrier();
  }
  float* out = a.kv + ((size_t)(sp * a.B + b) * a.heads + h) * 32 * 33;
#pragma unroll
  for (int q = 0; q < 4; ++q) out[d * 33 + e0 + q] = acc[q];
  if ((tid & 7) == 0) out[d * 33 + 32] = ks;
}

// pass 2: out[n][e] = sum_d phi(q[n][d]) kv[d][e] / (sum_d phi(q[n][d]) ksum[d] + 1e-6)
template <typename T>
__global__ void __launch_bounds__(256) linattn_out_kernel(const AttnArgs a) {
  __shared__ float skv[32 * 33];
  __shared__ float sq[64][33];
  const int h = blockIdx.y, b = blockIdx.z, tid = threadIdx.x;
  const int n0 = blockIdx.x * 64;
  const int inner = a.heads * 32, ld = 3 * inner;
  const float* kvp = a.kv + (size_t)(b * a.heads + h) * 32 * 33;
  const size_t sps = (size_t)a.B * a.heads * 32 * 33;
  for (int i = tid; i < 32 * 33; i += 256) {
    float v = kvp[i];
    for (int sp = 1; sp < a.nsplit; ++sp) v += kvp[sp * sps + i];
    skv[i] = v;
  }
  const T* base = reinterpret_cast<const T*>(a.qkv) + (size_t)b * a.N * ld;
  for (int i = tid; i < 64 * 32; i += 256) {
    const int n = i >> 5, c = i & 31;
    sq[n][c] = (n0 + n < a.N) ? phi((float)base[(size_t)(n0 + n) * ld + h * 32 + c]) : 0.f;
  }
  wg_barrier();
  const int n = tid >> 2, e0 = (tid & 3) * 8;
  if (n0 + n >= a.N) return;
  float acc[8], den = 0.f;
#pragma unroll
  for (int q = 0; q < 8; ++q) acc[q] = 0.f;
#pragma unroll 8
  for (int d = 0; d < 32; ++d) {
    const float qd = sq[n][d];
    den += qd * skv[d * 33 + 32];
#pragma unroll
    for (int q = 0; q < 8; ++q) acc[q] += qd * skv[d * 33 + e0 + q];
  }
  const float inv = 1.f / (den + 1e-6f);
  T* o = reinterpret_cast<T*>(a.out) + ((size_t)b * a.N + n0 + n) * inner + h * 32 + e0;
#pragma unroll
  for (int q = 0; q < 8; ++q) o[q] = (T)(acc[q] * inv);
}

// Position splits of pass 1: 128 positions per partial, at most 8 -- a function of N only, so the
// summation order (and the result bits) do not depend on the batch size.
int linattn_nsplit(int N) {
  int ns = 1;
  while (ns < 8 && N % (ns * 2 * 128) == 0) ns *= 2;
  return ns;
}
hipError_t launch_linattn_kv(int dtype, const AttnArgs& a, hipStream_t s) {
  if (a.nsplit < 1 || a.N % a.nsplit || (a.nsplit > 1 && a.N % (64 * a.nsplit))) return hipErrorInvalidValue;
  dim3 grid(a.heads, a.B, a.nsplit);
  return with_dtype(dtype, [&](auto t) {
    hipLaunchKernelGGL(linattn_kv_kernel<decltype(t)>, grid, dim3(256), 0, s, a);
    return hipGetLastError();
  });
}
hipError_t launch_linattn_out(int dtype, const AttnArgs& a, hipStream_t s) {
  dim3 grid((a.N + 63) / 64, a.heads, a.B);
  return with_dtype(dtype, [&](auto t) {
    hipLaunchKernelGGL(linattn_out_kernel<decltype(t)>, grid, dim3(256), 0, s, a);
    return hipGetLastError();
  });
}

// =============================================================================================
// y = x*as + ab (+res): the GroupNorm after to_out plus the attention residual
// (efficient_unet.py:266-269,306-308).  Block = 64 rows x all channels, stats slab tile = block.
template <typename T>
__global__ void __launch_bounds__(256) affine_add_kernel(const AffineAddArgs a) {
  constexpr int VEC = Elem<T>::VEC;
  extern __shared__ float red[];  // [4 waves][2][C]
  const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
  // tiles never straddle images: ceil(P / 64) tiles per image, the last one partial when P is not a multiple of 64
  const int tpi = (a.P + kAffineTileRows - 1) / kAffineTileRows;
  const int img = blockIdx.x / tpi, r0 = (blockIdx.x - img * tpi) * kAffineTileRows;
  const int m0 = img * a.P + r0;
  const int vrows = a.P - r0 < kAffineTileRows ? a.P - r0 : kAffineTileRows;
  const int vpr = a.C / VEC;  // vectors per row
  const T* x = reinterpret_cast<const T*>(a.x);
  const T* res = reinterpret_cast<const T*>(a.res);
  T* y = reinterpret_cast<T*>(a.y);
  // thread owns column vectors cv = tid % 64 + k*64 ... handled by looping rows per wave:
  // wave w processes rows w, w+4, ...; lanes stride over the row's vectors.
  for (int i = tid; i < 2 * 4 * a.C; i += 256) red[i] = 0.f;
  wg_barrier();
  for (int v0 = lane; v0 < vpr; v0 += 64) {
    float sc[VEC], sh[VEC], s1[VEC], s2[VEC];
#pragma unroll
    for (int e = 0; e < VEC; ++e) {
      sc[e] = a.as[(size_t)img * a.C + v0 * VEC + e];
      sh[e] = a.ab[(size_t)img * a.C + v0 * VEC + e];
      s1[e] = 0.f;
      s2[e] = 0.f;
    }
    for (int r = wave; r < vrows; r += 4) {
      const size_t o = (size_t)(m0 + r) * a.C + v0 * VEC;
      float f[VEC];
      ld_f32<T>(x + o, f);
#pragma unroll
      for (int e = 0; e < VEC; ++e) f[e] = f[e] * sc[e] + sh[e];
      if (res) {
        float rr[VEC];
        ld_f32<T>(res + o, rr);
#pragma unroll
        for (int e = 0; e < VEC; ++e) f[e] += rr[e];
      }
      typename Elem<T>::vec_t ov = f32_to_vec<T>(f);
      st_vec<T>(y + o, ov);
#pragma unroll
      for (int e = 0; e < VEC; ++e) {
        const float q = (float)ov[e];
        s1[e] += q;
        s2[e] += q * q;
      }
    }
    if (a.stats) {
#pragma unroll
      for (int e = 0; e < VEC; ++e) {
        red[(wave * 2 + 0) * a.C + v0 * VEC + e] = s1[e];
        red[(wave * 2 + 1) * a.C + v0 * VEC + e] = s2[e];
      }
    }
  }
  if (a.stats) {
    wg_barrier();
    const int ntiles = tpi, tile = r0 / kAffineTileRows;
    for (int i = tid; i < 2 * a.C; i += 256) {
      const int which = i / a.C, c = i % a.C;
      const float t = red[(0 * 2 + which) * a.C + c] + red[(1 * 2 + which) * a.C + c] + red[(2 * 2 + which) * a.C + c] +
                      red[(3 * 2 + which) * a.C + c];
      a.stats[((size_t)(img * ntiles + tile) * 2 + which) * a.C + c] = t;
    }
  }
}
hipError_t launch_affine_add(int dtype, const AffineAddArgs& a, hipStream_t s) {
  if (a.P < 1 || a.M % a.P || a.C % 8) return hipErrorInvalidValue;
  dim3 grid((a.M / a.P) * ((a.P + kAffineTileRows - 1) / kAffineTileRows));
  const size_t lds = (size_t)8 * a.C * 4;
  return with_dtype(dtype, [&](auto t) {
    hipLaunchKernelGGL(affine_add_kernel<decltype(t)>, grid, dim3(256), lds, s, a);
    return hipGetLastError();
  });
}

// =============================================================================================
// fp32 NCHW <-> NHWC T at the single-operator boundary.  Block = 64 pixels x 32 channels through LDS; pixels past P (the last
// block of a map whose pixel count is no multiple of 64) are read as zeros, counted as zeros in the statistics and not stored.
template <typename T>
__global__ void __launch_bounds__(256) nchw_to_nhwc_kernel(const float* x, T* y, float* stats, int C, int P, int Csrc,
                                                           int coff) {
  __shared__ float sm[32 * 65];
  const int tid = threadIdx.x;
  const int b = blockIdx.y, p0 = blockIdx.x * 64, c0 = blockIdx.z * 32;
  for (int i = tid; i < 32 * 64; i += 256) {
    const int c = i >> 6, p = i & 63;
    sm[c * 65 + p] = p0 + p < P ? x[((size_t)b * Csrc + coff + c0 + c) * P + p0 + p] : 0.f;
  }
  wg_barrier();
  for (int i = tid; i < 32 * 64; i += 256) {
    const int p = i >> 5, c = i & 31;
    const T v = (T)sm[c * 65 + p];
    if (p0 + p < P) y[((size_t)b * P + p0 + p) * C + c0 + c] = v;
    sm[c * 65 + p] = (float)v;  // element owned by this thread in this phase: no race
  }
  if (stats) {
    wg_barrier();
    const int ntiles = (P + 63) / 64, tile = blockIdx.x;
    if (tid < 32) {
      float s1 = 0.f, s2 = 0.f;
      for (int p = 0; p < 64; ++p) {
        const float q = sm[tid * 65 + p];
        s1 += q;
        s2 += q * q;
      }
      stats[((size_t)(b * ntiles + tile) * 2 + 0) * C + c0 + tid] = s1;
      stats[((size_t)(b * ntiles + tile) * 2 + 1) * C + c0 + tid] = s2;
    }
  }
}
template <typename T>
__global__ void __launch_bounds__(256) nhwc_to_nchw_kernel(const T* x, float* y, int C, int P, int Cdst, int coff) {
  __shared__ float sm[32 * 65];
  const int tid = threadIdx.x;
  const int b = blockIdx.y, p0 = blockIdx.x * 64, c0 = blockIdx.z * 32;
  for (int i = tid; i < 32 * 64; i += 256) {
    const int p = i >> 5, c = i & 31;
    sm[c * 65 + p] = p0 + p < P ? (float)x[((size_t)b * P + p0 + p) * C + c0 + c] : 0.f;
  }
  wg_barrier();
  for (int i = tid; i < 32 * 64; i += 256) {
    const int c = i >> 6, p = i & 63;
    if (p0 + p < P) y[((size_t)b * Cdst + coff + c0 + c) * P + p0 + p] = sm[c * 65 + p];
  }
}
hipError_t launch_nchw_to_nhwc(int dtype, const float* x, void* y, float* stats, int B, int C, int P, int Csrc, int coff,
                               hipStream_t s) {
  if (P < 1 || C % 32) return hipErrorInvalidValue;
  dim3 grid((P + 63) / 64, B, C / 32);
  return with_dtype(dtype, [&](auto t) {
    using T = decltype(t);
    hipLaunchKernelGGL(nchw_to_nhwc_kernel<T>, grid, dim3(256), 0, s, x, (T*)y, stats, C, P, Csrc, coff);
    return hipGetLastError();
  });
}
hipError_t launch_nhwc_to_nchw(int dtype, const void* x, float* y, int B, int C, int P, hipStream_t s, int Cdst, int coff) {
  if (Cdst <= 0) Cdst = C;
  if (P < 1 || C % 32) return hipErrorInvalidValue;
  dim3 grid((P + 63) / 64, B, C / 32);
  return with_dtype(dtype, [&](auto t) {
    using T = decltype(t);
    hipLaunchKernelGGL(nhwc_to_nchw_kernel<T>, grid, dim3(256), 0, s, (const T*)x, y, C, P, Cdst, coff);
    return hipGetLastError();
  });
}

// =============================================================================================
// Weight repack (load time only).
// Up-sampling conv, 2-byte engines: the bilinear x2 (align_corners = False) folded into per-phase 3x3 weights on the replicate-padded
// low-resolution input (layout: kernels.h, launch_conv3x3_upfold).  Output pixel (2i + a, 2j + b) of conv3x3(up2(x), w) is
//   sum_{r,s} Wf[a][b][r][s] xr[i + r - 1, j + s - 1],  Wf[a][b][r][s] = sum_{u,v} R[a][r][u] R[b][s][v] w[u][v]
// with R[a][r][u] the weight of low-resolution row i + r - 1 in up-sampled row 2i + a + u - 1.  On the output's outermost ring the
// conv's zero padding replaces kernel row ue = 0 (a = 0, i = 0) / 2 (a = 1, i = H - 1) -- for which the replicate padding has put
// x[ie] -- and likewise column ve: the correction sets hold -sum_v R[b][s][v] w[ue][v] (row edge), -sum_u R[a][r][u] w[u][ve]
// (column edge) and +w[ue][ve] (corner, subtracted twice by the other two).  Every coefficient is a multiple of 1/16: fp64 sums
// are exact, and the single rounding to T goes through a float rounded to odd.
__constant__ double kUpR[2][3][3] = {{{.75, .25, 0.}, {.25, .75, .75}, {0., 0., .25}}, {{.25, 0., 0.}, {.75, .75, .25}, {0., .25, .75}}};
template <typename T>
__global__ void __launch_bounds__(256) upconv_fold_kernel(const float* src, T* dst, int C, const unsigned long long* state) {
  if (state && state[1] == 0) return;  // parameters unchanged since the last load
  const long long idx = (long long)blockIdx.x * 256 + threadIdx.x, cc = (long long)C * C;
  if (idx >= 64 * cc) return;
  const int set = (int)(idx / cc), co = (int)(idx % cc) / C, ci = (int)(idx % cc) % C;
  const float* w = src + ((size_t)co * C + ci) * 9;
  const int p = set < 36 ? set / 9 : (set < 60 ? ((set - 36) % 12) / 3 : set - 60), a = p >> 1, b = p & 1;
  const int ue = a ? 2 : 0, ve = b ? 2 : 0;
  double v = 0.0;
  if (set < 36) {
    const int r = (set % 9) / 3, s = set % 3;
    for (int u = 0; u < 3; ++u)
      for (int x = 0; x < 3; ++x) v += kUpR[a][r][u] * kUpR[b][s][x] * (double)w[u * 3 + x];
  } else if (set < 48) {
    const int s = (set - 36) % 3;
    for (int x = 0; x < 3; ++x) v -= kUpR[b][s][x] * (double)w[ue * 3 + x];
  } else if (set < 60) {
    const int r = (set - 48) % 3;
    for (int u = 0; u < 3; ++u) v -= kUpR[a][r][u] * (double)w[u * 3 + ve];
  } else {
    v = (double)w[ue * 3 + ve];
  }
  float f = (float)v;
  if ((double)f != v) {  // round to odd, so that the rounding to T below is the only one that counts
    uint32_t bits = __float_as_uint(f);
    if (!(bits & 1u)) bits += (((double)f < v) == !(bits >> 31)) ? 1u : 0xFFFFFFFFu;
    f = __uint_as_float(bits);
  }
  dst[idx] = (T)f;
}
hipError_t launch_upconv_fold(int dtype, const float* src, void* dst, int C, hipStream_t s, const unsigned long long* state) {
  if (C < 1) return hipErrorInvalidValue;
  dim3 grid((unsigned)((64LL * C * C + 255) / 256));
  return with_dtype2(dtype, [&](auto t) {
    using T = decltype(t);
    hipLaunchKernelGGL(upconv_fold_kernel<T>, grid, dim3(256), 0, s, src, (T*)dst, C, state);
    return hipGetLastError();
  });
}

// Content hash of every parameter (fp32 bits, position-weighted, summed mod 2^64: the order of the partial sums does
// not matter), so that writes PyTorch's version counters cannot see (`p.data.copy_()`, the reference's EMA
// apply_shadow / restore, trainer.py:104-117) are noticed without a host round trip: hash_finalize compares with
// the hash of the last load and raises state[1]; load_all_kernel does nothing when state[1] == 0.
__global__ void __launch_bounds__(256) params_hash_kernel(const LoadDesc* descs, unsigned long long* partial) {
  const LoadDesc d = descs[blockIdx.y];
  const uint32_t* src = reinterpret_cast<const uint32_t*>(d.src);
  unsigned long long acc = 0;
  const unsigned long long wy = 0x9E3779B97F4A7C15ull * (unsigned long long)(blockIdx.y + 1);
  for (long long i = (long long)blockIdx.x * 256 + threadIdx.x; i < d.numel; i += (long long)gridDim.x * 256)
    acc += (unsigned long long)src[i] * ((wy + 0xD1B54A32D192ED03ull * (unsigned long long)(i + 1)) | 1ull);
#pragma unroll
  for (int o = 32; o > 0; o >>= 1) acc += __shfl_xor(acc, o, 64);
  __shared__ unsigned long long red[4];
  if ((threadIdx.x & 63) == 0) red[threadIdx.x >> 6] = acc;
  wg_barrier();
  if (threadIdx.x == 0) partial[(size_t)blockIdx.y * gridDim.x + blockIdx.x] = red[0] + red[1] + red[2] + red[3];
}
__global__ void __launch_bounds__(256) hash_finalize_kernel(const unsigned long long* partial, int count, unsigned long long* state,
                                                            int force) {
  unsigned long long acc = 0;
  for (int i = threadIdx.x; i < count; i += 256) acc += partial[i];
#pragma unroll
  for (int o = 32; o > 0; o >>= 1) acc += __shfl_xor(acc, o, 64);
  __shared__ unsigned long long red[4];
  if ((threadIdx.x & 63) == 0) red[threadIdx.x >> 6] = acc;
  wg_barrier();
  if (threadIdx.x == 0) {
    const unsigned long long h = red[0] + red[1] + red[2] + red[3];
    state[1] = (force || h != state[0]) ? 1ull : 0ull;
    state[0] = h;
  }
}
hipError_t launch_params_hash(const LoadDesc* descs_dev, int n, unsigned long long* partial, unsigned long long* state, int force,
                              hipStream_t s) {
  hipLaunchKernelGGL(params_hash_kernel, dim3(32, n), dim3(256), 0, s, descs_dev, partial);
  hipLaunchKernelGGL(hash_finalize_kernel, dim3(1), dim3(256), 0, s, partial, 32 * n, state, force);
  return hipGetLastError();
}

// Every engine layout of a parameter (kernels.h: LoadDesc), stated once: one source element per iteration, scattered to the main
// destination and to whichever secondary copies the descriptor names.
template <typename T>
__device__ __forceinline__ void load_one(const LoadDesc& d, char* blob) {
  const float* src = d.src;
  for (long long i = (long long)blockIdx.x * 256 + threadIdx.x; i < d.numel; i += (long long)gridDim.x * 256) {
    const float v = src[i];
    if (d.kind == PK_F32) {
      reinterpret_cast<float*>(blob + d.dst)[i] = v;
    } else if (d.kind == PK_MAT) {
      const int r = (int)(i / d.cols), c = (int)(i % d.cols);
      const size_t o = (size_t)r * d.ld + d.col0 + c;
      if (d.as_t) reinterpret_cast<T*>(blob + d.dst)[o] = (T)v;
      else reinterpret_cast<float*>(blob + d.dst)[o] = v;
      if (d.dst_t >= 0) reinterpret_cast<T*>(blob + d.dst_t)[(size_t)c * d.rows + r] = (T)v;
      if (d.dst_f >= 0) reinterpret_cast<T*>(blob + d.dst_f)[pw_expand_pack_index(r, c, d.cols)] = (T)(v * d.fscale);
    } else if (d.kind == PK_CONV3) {
      const int tap = (int)(i % 9);
      const int ci = (int)((i / 9) % d.I), co = (int)(i / (9 * (long long)d.I));
      reinterpret_cast<T*>(blob + d.dst)[((size_t)tap * d.Op + co) * d.Ip + ci] = (T)v;
      if (d.dst_t >= 0) reinterpret_cast<T*>(blob + d.dst_t)[((size_t)(8 - tap) * d.Ip + ci) * d.Op + co] = (T)v;
    } else if (d.kind == PK_DW) {  // flipped taps: the input-gradient of a depthwise conv is the same conv with w'[t] = w[8 - t]
      const int tap = (int)(i % 9), c = (int)(i / 9);
      reinterpret_cast<float*>(blob + d.dst)[(size_t)tap * d.Op + c] = v;
      if (d.dst_t >= 0) reinterpret_cast<float*>(blob + d.dst_t)[(size_t)(8 - tap) * d.Op + c] = v;
    } else if (d.kind == PK_INIT) {  // input conv OIHW: fp32 [I*9][Op], and (2-byte T) the MFMA pack [tap][Op][8]: tap 9, channels
                                     // >= I and outputs >= O keep the zeros of llie_create's memset of the blob, like all padding
      const int k = (int)(i % (d.I * 9)), o = (int)(i / (d.I * 9));
      reinterpret_cast<float*>(blob + d.dst)[(size_t)k * d.Op + o] = v;
      if (d.dst_t >= 0) {
        const int tap = k % 9, ci = k / 9;
        reinterpret_cast<T*>(blob + d.dst_t)[((size_t)tap * d.Op + o) * 8 + ci] = (T)v;
      }
    } else {  // PK_FINAL: output conv OIHW (O <= 4): fp32 [9][Ip][4], and the MFMA pack
              // dst[(((chunk*18 + ks)*2 + h)*4 + o)*8 + j] = W[o][chunk*32 + (ks&1)*16 + h*8 + j][tap = ks>>1]
      const int tap = (int)(i % 9), ci = (int)((i / 9) % d.I), o = (int)(i / (9 * (long long)d.I));
      reinterpret_cast<float*>(blob + d.dst)[((size_t)tap * d.Ip + ci) * 4 + o] = v;
      if (d.dst_t >= 0) {
        const int chunk = ci >> 5, r = ci & 31, ks = tap * 2 + (r >> 4), hh = (r >> 3) & 1, j = r & 7;
        reinterpret_cast<T*>(blob + d.dst_t)[((((size_t)chunk * 18 + ks) * 2 + hh) * 4 + o) * 8 + j] = (T)v;
      }
    }
  }
}
template <typename T>
__global__ void __launch_bounds__(256) load_all_kernel(const LoadDesc* descs, char* blob, const unsigned long long* state) {
  if (state && state[1] == 0) return;  // parameters unchanged since the last load
  const LoadDesc d = descs[blockIdx.y];
  load_one<T>(d, blob);
}
template <typename T>
__global__ void __launch_bounds__(256) load_one_kernel(const LoadDesc d, char* blob) { load_one<T>(d, blob); }
hipError_t launch_load_all(int dtype, const LoadDesc* descs_dev, int n, char* blob, hipStream_t s, const unsigned long long* state) {
  dim3 grid(32, n);
  return with_dtype(dtype, [&](auto t) {
    hipLaunchKernelGGL(load_all_kernel<decltype(t)>, grid, dim3(256), 0, s, descs_dev, blob, state);
    return hipGetLastError();
  });
}
hipError_t launch_load_one(int dtype, const LoadDesc& d, char* blob, hipStream_t s) {
  dim3 grid((unsigned)((d.numel + 255) / 256));
  return with_dtype(dtype, [&](auto t) {
    hipLaunchKernelGGL(load_one_kernel<decltype(t)>, grid, dim3(256), 0, s, d, blob);
    return hipGetLastError();
  });
}

// =============================================================================================
// uint8 image I/O either side of the path (scripts/inference.py:99-134), bit-exact with the host
// implementation (hostio.py): bilinear resize with cv2.INTER_LINEAR's half-pixel geometry evaluated in
// fp32 WITHOUT fused multiply-adds (NumPy evaluates a*(1-f) + b*f as two products and a sum), rounding
// half up to uint8; then x/127.5 - 1 on the way in, (x+1)*127.5 clipped and truncated on the way out.
struct ResizeAxis { int i0, i1; float f; };
// NB: HIP's __fmul_rn / __fadd_rn are ordinary operators, so clang's default -ffp-contract=fast would
// still fuse them; contraction is switched off per function where the operation order is part of the contract.
__device__ __forceinline__ ResizeAxis resize_axis(int o, int n_in, float scale) {
#pragma clang fp contract(off)
  const float pos = ((float)o + 0.5f) * scale - 0.5f;
  const float fl = floorf(pos);
  ResizeAxis r;
  const int lo = (int)fl;
  r.f = pos - fl;
  r.i0 = min(max(lo, 0), n_in - 1);
  r.i1 = min(max(lo + 1, 0), n_in - 1);
  return r;
}
__device__ __forceinline__ float lerp2_nofma(float v00, float v01, float v10, float v11, float fx, float fy) {
#pragma clang fp contract(off)
  const float gx = 1.f - fx, gy = 1.f - fy;
  const float top = v00 * gx + v01 * fx;
  const float bot = v10 * gx + v11 * fx;
  return top * gy + bot * fy;
}
__device__ __forceinline__ float round_u8(float v) {
#pragma clang fp contract(off)
  return fminf(fmaxf(floorf(v + 0.5f), 0.f), 255.f);
}

// img u8 [B][H0][W0][3] -> out fp32 [B][3][S][S]
__global__ void preprocess_u8_kernel(const uint8_t* img, int H0, int W0, float* out, int S, float sy, float sx) {
#pragma clang fp contract(off)
  const int x = blockIdx.x * blockDim.x + threadIdx.x, y = blockIdx.y, b = blockIdx.z;
  if (x >= S) return;
  const uint8_t* src = img + (size_t)b * H0 * W0 * 3;
  float u[3];
  if (H0 == S && W0 == S) {
#pragma unroll
    for (int c = 0; c < 3; ++c) u[c] = (float)src[((size_t)y * W0 + x) * 3 + c];
  } else {
    const ResizeAxis ay = resize_axis(y, H0, sy), ax = resize_axis(x, W0, sx);
#pragma unroll
    for (int c = 0; c < 3; ++c) {
      const float v = lerp2_nofma((float)src[((size_t)ay.i0 * W0 + ax.i0) * 3 + c], (float)src[((size_t)ay.i0 * W0 + ax.i1) * 3 + c],
                                  (float)src[((size_t)ay.i1 * W0 + ax.i0) * 3 + c], (float)src[((size_t)ay.i1 * W0 + ax.i1) * 3 + c], ax.f, ay.f);
      u[c] = round_u8(v);
    }
  }
#pragma unroll
  for (int c = 0; c < 3; ++c) out[(((size_t)b * 3 + c) * S + y) * S + x] = u[c] / 127.5f - 1.0f;
}
// x fp32 [B][3][S][S] -> img u8 [B][H0][W0][3]
__global__ void postprocess_u8_kernel(const float* xin, int S, uint8_t* img, int H0, int W0, float sy, float sx) {
#pragma clang fp contract(off)
  const int x = blockIdx.x * blockDim.x + threadIdx.x, y = blockIdx.y, b = blockIdx.z;
  if (x >= W0) return;
  const float* src = xin + (size_t)b * 3 * S * S;
  auto den = [&](int c, int yy, int xx) {  // (x+1)*127.5, clip, truncate -> the uint8 the host would have stored
    const float v = (src[((size_t)c * S + yy) * S + xx] + 1.0f) * 127.5f;
    return truncf(fminf(fmaxf(v, 0.f), 255.f));
  };
  uint8_t* dst = img + (((size_t)b * H0 + y) * W0 + x) * 3;
  if (H0 == S && W0 == S) {
#pragma unroll
    for (int c = 0; c < 3; ++c) dst[c] = (uint8_t)den(c, y, x);
  } else {
    const ResizeAxis ay = resize_axis(y, S, sy), ax = resize_axis(x, S, sx);
#pragma unroll
    for (int c = 0; c < 3; ++c)
      dst[c] = (uint8_t)round_u8(lerp2_nofma(den(c, ay.i0, ax.i0), den(c, ay.i0, ax.i1), den(c, ay.i1, ax.i0), den(c, ay.i1, ax.i1), ax.f, ay.f));
  }
}
hipError_t launch_preprocess_u8(const uint8_t* img, int B, int H0, int W0, float* out, int S, hipStream_t s) {
  if (B <= 0 || H0 <= 0 || W0 <= 0 || S <= 0) return hipErrorInvalidValue;
  const float sy = (float)((double)H0 / (double)S), sx = (float)((double)W0 / (double)S);
  hipLaunchKernelGGL(preprocess_u8_kernel, dim3((S + 127) / 128, S, B), dim3(128), 0, s, img, H0, W0, out, S, sy, sx);
  return hipGetLastError();
}
hipError_t launch_postprocess_u8(const float* x, int B, int S, uint8_t* img, int H0, int W0, hipStream_t s) {
  if (B <= 0 || H0 <= 0 || W0 <= 0 || S <= 0) return hipErrorInvalidValue;
  const float sy = (float)((double)S / (double)H0), sx = (float)((double)S / (double)W0);
  hipLaunchKernelGGL(postprocess_u8_kernel, dim3((W0 + 127) / 128, H0, B), dim3(128), 0, s, x, S, img, H0, W0, sy, sx);
  return hipGetLastError();
}

// =============================================================================================
// LCMScheduler.step (lcm_scheduler.py:204-242), same operation order as the reference:
//   x0 = (x - sb*eps)/sa  |  x0 = sa*x - sb*v ;  prev = last ? x0 : sap*x0 + sbp*noise
// sampler == 1, the deterministic DDIM step (low_light_diffusion.py:365-379): the predicted noise takes the draw's place,
//   eh = eps  |  sa*v + sb*x ;  prev = last ? x0 : sap*x0 + sbp*eh          (noise is not read)
__global__ void lcm_step_kernel(const float* eps, const float* x, const float* noise, float* prev, float* x0o,
                                float* clamped, int64_t n, StepCoef c) {
#pragma clang fp contract(off)
  const int64_t i = (int64_t)blockIdx.x * blockDim.x + threadIdx.x;
  if (i >= n) return;
  const float e = eps[i], xv = x[i];
  float x0;
  if (c.vpred) x0 = c.sa * xv - c.sb * e;
  else x0 = (xv - c.sb * e) / c.sa;
  if (c.clamp_x0) x0 = fminf(fmaxf(x0, -1.f), 1.f);
  float p = x0;
  if (!c.is_last) {
    float nz;
    if (!c.sampler) nz = noise[i];
    else if (c.vpred) nz = c.sa * e + c.sb * xv;
    else nz = e;
    p = c.sap * x0 + c.sbp * nz;
  }
  prev[i] = p;
  if (x0o) x0o[i] = x0;
  if (clamped) clamped[i] = fminf(fmaxf(p, -1.f), 1.f);
}
hipError_t launch_lcm_step(const float* eps, const float* x, const float* noise, float* prev, float* x0,
                           float* clamped, int64_t n, StepCoef c, hipStream_t s) {
  if ((!c.is_last && !c.sampler && !noise) || (c.sampler && c.clamp_x0)) return hipErrorInvalidValue;
  hipLaunchKernelGGL(lcm_step_kernel, dim3((unsigned)((n + 255) / 256)), dim3(256), 0, s, eps, x, noise, prev, x0,
                     clamped, n, c);
  return hipGetLastError();
}
// add_noise / get_velocity (lcm_scheduler.py:255-305)
// A timestep outside [0, table_len) (an IndexError in the reference) never indexes the table: the sample comes out NaN.
__global__ void add_noise_kernel(const float* x0, const float* noise, const int64_t* t, const float* acp, float* out,
                                 int64_t per, int velocity, int table_len) {
#pragma clang fp contract(off)
  const int b = blockIdx.y;
  const int64_t i = (int64_t)blockIdx.x * blockDim.x + threadIdx.x;
  if (i >= per) return;
  const int64_t tb = t[b];
  const float a = (tb >= 0 && tb < table_len) ? acp[tb] : __builtin_nanf("");
  const float sa = sqrtf(a), sb = sqrtf(1.f - a);
  const size_t o = (size_t)b * per + i;
  out[o] = velocity ? sa * noise[o] - sb * x0[o] : sa * x0[o] + sb * noise[o];
}
hipError_t launch_add_noise(const float* x0, const float* noise, const int64_t* t, const float* acp, float* out, int B,
                            int64_t per, int velocity, int table_len, hipStream_t s) {
  dim3 grid((unsigned)((per + 255) / 256), B);
  hipLaunchKernelGGL(add_noise_kernel, grid, dim3(256), 0, s, x0, noise, t, acp, out, per, velocity, table_len);
  return hipGetLastError();
}

// HBM copy-bandwidth probe (bench.py `peak_measured`): 16 bytes per lane, grid-stride.
// zero fill as a kernel of this library (16 bytes per lane): the totals region of a forward (Run::zbegin)
__global__ void __launch_bounds__(256) zero_fill_kernel(u32x4* __restrict__ dst, int64_t n16) {
  const u32x4 z = {0u, 0u, 0u, 0u};
  for (int64_t i = (int64_t)blockIdx.x * 256 + threadIdx.x; i < n16; i += (int64_t)gridDim.x * 256) dst[i] = z;
}
hipError_t launch_zero_fill(void* dst, int64_t bytes, hipStream_t s) {
  if (bytes % 16 || (reinterpret_cast<uintptr_t>(dst) & 15)) return hipErrorInvalidValue;
  const int64_t n16 = bytes / 16;
  int grid = (int)((n16 + 255) / 256);
  if (grid > 1024) grid = 1024;
  if (grid < 1) grid = 1;
  hipLaunchKernelGGL(zero_fill_kernel, dim3(grid), dim3(256), 0, s, reinterpret_cast<u32x4*>(dst), n16);
  return hipGetLastError();
}

// four 16-byte loads in flight per lane before the (non-temporal) stores: a workgroup streams 16 KB per iteration
__global__ void __launch_bounds__(256) copy_probe_kernel(const u32x4* __restrict__ src, u32x4* __restrict__ dst, int64_t n) {
  const int64_t stride = (int64_t)gridDim.x * 1024;
  int64_t i = (int64_t)blockIdx.x * 1024 + threadIdx.x;
  for (; i + 768 < n; i += stride) {
    u32x4 v[4];
#pragma unroll
    for (int j = 0; j < 4; ++j) v[j] = __builtin_nontemporal_load(src + i + j * 256);
#pragma unroll
    for (int j = 0; j < 4; ++j) __builtin_nontemporal_store(v[j], dst + i + j * 256);
  }
  for (int j = 0; j < 4; ++j)  // ragged end
    if (i + j * 256 < n) dst[i + j * 256] = src[i + j * 256];
}
hipError_t launch_copy_probe(const void* src, void* dst, int64_t bytes, hipStream_t s) {
  if (bytes % 16) return hipErrorInvalidValue;
  hipLaunchKernelGGL(copy_probe_kernel, dim3(256 * 8), dim3(256), 0, s, reinterpret_cast<const u32x4*>(src),
                     reinterpret_cast<u32x4*>(dst), bytes / 16);
  return hipGetLastError();
}

// Mixed read / write streaming probe: per step a workgroup reads R and writes W 16 KB blocks (16 bytes per lane).  The
// write-dominated launches of this engine (the 4x expansions) are judged against what HBM sustains at THEIR read : write
// mix, which is not the copy rate (bench.py `peak_measured`).
// MODE: 0 plain loads / stores, 1 non-temporal, 2 plain loads + write-through (sc1) stores, 3 plain loads + sc0 sc1 stores
template <int R, int W, int MODE>
__global__ void __launch_bounds__(256) rw_probe_kernel(const u32x4* __restrict__ src, u32x4* __restrict__ dst, int64_t units) {
  u32x4 acc = {0u, 0u, 0u, 0u};
  for (int64_t u = blockIdx.x; u < units; u += gridDim.x) {
    u32x4 v[R > 0 ? R * 4 : 1];
#pragma unroll
    for (int j = 0; j < R * 4; ++j) {
      const u32x4* p = src + (u * R * 4 + j) * 256 + threadIdx.x;
      v[j] = MODE == 1 ? __builtin_nontemporal_load(p) : *p;
    }
#pragma unroll
    for (int j = 0; j < R * 4; ++j) acc ^= v[j];
#pragma unroll
    for (int j = 0; j < W * 4; ++j) {
      u32x4* p = dst + (u * W * 4 + j) * 256 + threadIdx.x;
      u32x4 o = acc;
      o[0] += (uint32_t)j;
      if constexpr (MODE == 1) __builtin_nontemporal_store(o, p);
      else if constexpr (MODE == 2) asm volatile("global_store_dwordx4 %0, %1, off sc1\n\ts_nop 1" ::"v"(p), "v"(o) : "memory");
      else if constexpr (MODE == 3) asm volatile("global_store_dwordx4 %0, %1, off sc0 sc1\n\ts_nop 1" ::"v"(p), "v"(o) : "memory");
      else *p = o;
    }
  }
  if (W == 0 && acc[0] == 0x9E3779B9u && acc[1] == 0x7F4A7C15u) dst[threadIdx.x] = acc;  // keeps the loads alive
}
__global__ void tiny_probe_kernel(unsigned* p) {
  if (threadIdx.x == 0 && blockIdx.x == 0) p[0] += 1u;
}
hipError_t launch_rw_probe(const void* src, void* dst, int64_t units, int r, int w, int nt, hipStream_t s) {
  const u32x4* a = reinterpret_cast<const u32x4*>(src);
  u32x4* b = reinterpret_cast<u32x4*>(dst);
  const dim3 grid(256 * 8), block(256);
  if (r == -1) {  // a trivial dependent launch: what a kernel boundary costs behind a write-heavy kernel (tools/gpu_rw_probe.py)
    hipLaunchKernelGGL(tiny_probe_kernel, dim3(1), dim3(64), 0, s, reinterpret_cast<unsigned*>(dst));
    return hipGetLastError();
  }
  if (r < 0 || r > 4 || w < 0 || w > 4) return hipErrorInvalidValue;
  return with_value<10, 1, 11, 12, 14, 21, 41>(10 * r + w, [&](auto rw) {  // the read : write mixes that exist, as 10 R + W
    constexpr int R = decltype(rw)::value / 10, W = decltype(rw)::value % 10;
    return with_value<1, 2, 3, 0>(nt >= 1 && nt <= 3 ? nt : 0, [&](auto mode) {
      hipLaunchKernelGGL((rw_probe_kernel<R, W, decltype(mode)::value>), grid, block, 0, s, a, b, units);
      return hipGetLastError();
    });
  });
}

}  // namespace llie
