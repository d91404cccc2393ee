// Softmax attention core of StandardAttention (efficient_unet.py:349-353) in flash form on the matrix cores, forward and backward.
//
// Layout: qkv [B][N][3 * inner] T (q | k | v, each head-major), inner = 32 heads, dim_head 32; out / dout [B][N][inner] T;
// lse [B][heads][N] fp32 = log sum_j exp(scale q_i . k_j); dqkv like qkv.  The N x N matrix never exists in memory.
//
// All three kernels share one shape.  A workgroup of four waves owns a tile of 128 rows of one (image, head) -- queries in the
// forward and the dQ kernel, keys in the dK / dV kernel -- 32 rows per wave, whose operands stay in registers.  The other side
// streams through LDS in blocks of 64 rows, ascending, and every wave walks a block as two 32-row halves:
//   1. S^T = X . R^T on MFMA with the streamed rows X as the A operand and the wave's own rows R as B, so a lane holds 16 streamed
//      rows of ONE own row (accumulator layout: column = lane & 31, rows = mfma_row(r, lane)): the row maximum and the row sum
//      are 16 in-lane steps and one exchange with lane ^ 32.
//   2. the second product (P . V, dS . K, P^T . dO, dS^T . Q) takes that accumulator, rounded once to T, as its B operand in the
//      accumulator's own row order, and reads the A operand from a transposed LDS copy of the streamed block in the same
//      permuted order: the permutation of the summation index cancels, no shuffle is needed.
// Rows past N are staged as zeros and masked (-inf logits, +inf lse), so they contribute exactly zero; own rows past N are
// computed on zeros and never stored.  Tile and block sizes are constants: the summation order of an image depends on N alone,
// never on the batch.  No atomics; wg_barrier() is the only barrier.
#include "common.h"

namespace llie {

namespace {

constexpr int kSaTile = 128;   // own rows per workgroup (32 per wave)
constexpr int kSaBlock = 64;   // streamed rows per LDS block
constexpr float kLog2e = 1.4426950408889634f, kLn2 = 0.6931471805599453f;
constexpr float kSaScale = 0.17677669529663687f;  // 32^-0.5

template <typename T> struct Sa {
  static constexpr int VEC = Elem<T>::VEC;
  static constexpr int VPR = 32 / VEC;                  // 16-byte vectors per 32-channel row
  static constexpr int NV = kSaBlock * VPR / 256;       // vectors of one staged block per thread
  static constexpr int RP = TilePitch<T>::value;        // pitch of a row-major [64][32] tile
  static constexpr int TP = kSaBlock + 4;               // pitch of a transposed [32][64] tile: 8- / 16-byte aligned 4-element reads
  typedef typename Elem<T>::vec_t vec_t;
  struct alignas(16) Slice { T v[16]; };                // a lane's 16 channels [16 h, 16 h + 16) of its own row
};

template <typename T> __device__ __forceinline__ typename Sa<T>::vec_t zero_vec() {
  typename Sa<T>::vec_t z;
#pragma unroll
  for (int i = 0; i < Sa<T>::VEC; ++i) z[i] = (T)0.f;
  return z;
}

// this lane's slice of row `row` (of N) of a [N][ld] matrix whose 32 channels start at `base`; zeros past N
template <typename T> __device__ __forceinline__ typename Sa<T>::Slice load_slice(const T* base, int64_t ld, int row, int N, int h) {
  typename Sa<T>::Slice s;
#pragma unroll
  for (int i = 0; i < 16 / Sa<T>::VEC; ++i) {
    const typename Sa<T>::vec_t v = row < N ? ld_vec<T>(base + (int64_t)row * ld + 16 * h + i * Sa<T>::VEC) : zero_vec<T>();
    *reinterpret_cast<typename Sa<T>::vec_t*>(&s.v[i * Sa<T>::VEC]) = v;
  }
  return s;
}

// the thread's vectors of the 64-row block starting at row0: global -> registers (zeros past N)
template <typename T>
__device__ __forceinline__ void block_load(const T* base, int64_t ld, int row0, int N, int tid, typename Sa<T>::vec_t (&v)[Sa<T>::NV]) {
#pragma unroll
  for (int i = 0; i < Sa<T>::NV; ++i) {
    const int idx = tid + 256 * i, row = row0 + idx / Sa<T>::VPR, c0 = (idx % Sa<T>::VPR) * Sa<T>::VEC;
    v[i] = row < N ? ld_vec<T>(base + (int64_t)row * ld + c0) : zero_vec<T>();
  }
}
// registers -> LDS, row-major (rows != null) and / or transposed (tr != null)
template <typename T>
__device__ __forceinline__ void block_store(T* rows, T* tr, int tid, const typename Sa<T>::vec_t (&v)[Sa<T>::NV]) {
#pragma unroll
  for (int i = 0; i < Sa<T>::NV; ++i) {
    const int idx = tid + 256 * i, row = idx / Sa<T>::VPR, c0 = (idx % Sa<T>::VPR) * Sa<T>::VEC;
    if (rows) st_vec<T>(rows + row * Sa<T>::RP + c0, v[i]);
    if (tr) {
#pragma unroll
      for (int e = 0; e < Sa<T>::VEC; ++e) tr[(c0 + e) * Sa<T>::TP + row] = v[i][e];
    }
  }
}

// acc[streamed row][own row] = X . R^T over the 32 channels: X = rows of the row-major tile (half `sub`), R = the lane's slice
template <typename T>
__device__ __forceinline__ f32x16 mm_rows(const T* rows, int sub, int lane, const typename Sa<T>::Slice& r) {
  f32x16 acc;
#pragma unroll
  for (int i = 0; i < 16; ++i) acc[i] = 0.f;
  Mfma<T>::chunk(rows + (sub * 32 + (lane & 31)) * Sa<T>::RP + 16 * (lane >> 5), r.v, acc);
  return acc;
}

// acc[channel][own row] += sum over the 32 streamed rows of half `sub`: Xt[channel][row] p[row][own row], p in accumulator order
// (p[r] belongs to streamed row mfma_row(r, lane)), rounded once to T
template <typename T>
__device__ __forceinline__ void mm_t(f32x16& acc, const T* tr, int sub, int lane, const float (&p)[16]) {
  const T* trow = tr + (lane & 31) * Sa<T>::TP + sub * 32 + 4 * (lane >> 5);
  if constexpr (std::is_same<T, float>::value) {
#pragma unroll
    for (int g = 0; g < 4; ++g) {
      const f32x4 a = *reinterpret_cast<const f32x4*>(trow + 8 * g);
#pragma unroll
      for (int i = 0; i < 4; ++i) acc = __builtin_amdgcn_mfma_f32_32x32x2f32(a[i], p[4 * g + i], acc, 0, 0, 0);
    }
  } else {
    typedef T t4 __attribute__((ext_vector_type(4)));
#pragma unroll
    for (int half = 0; half < 2; ++half) {
      const t4 lo = *reinterpret_cast<const t4*>(trow + 16 * half), hi = *reinterpret_cast<const t4*>(trow + 16 * half + 8);
      typename Sa<T>::vec_t a, b;
#pragma unroll
      for (int j = 0; j < 4; ++j) { a[j] = lo[j]; a[4 + j] = hi[j]; }
#pragma unroll
      for (int j = 0; j < 8; ++j) b[j] = (T)p[8 * half + j];
      acc = mfma16<T>(a, b, acc);
    }
  }
}

// acc[channel mfma_row(r)][own row lane & 31] * mul -> dst[32 channels] of the lane's own row
template <typename T> __device__ __forceinline__ void store_own(T* dst, const f32x16& acc, float mul, int lane) {
  typedef T t4 __attribute__((ext_vector_type(4)));
#pragma unroll
  for (int g = 0; g < 4; ++g) {
    t4 o;
#pragma unroll
    for (int i = 0; i < 4; ++i) o[i] = (T)(acc[4 * g + i] * mul);
    *reinterpret_cast<t4*>(dst + 8 * g + 4 * (lane >> 5)) = o;
  }
}

}  // namespace

// ---------------------------------------------------------------------------------------------------------------------------
// out_i = sum_j softmax_j(scale q_i . k_j) v_j with a running maximum and sum (fp32); lse written when non-null
template <typename T>
__global__ void __launch_bounds__(256) softattn_fwd_kernel(const SoftAttnArgs a) {
  typedef Sa<T> S;
  __shared__ __attribute__((aligned(16))) T Ks[kSaBlock * S::RP];
  __shared__ __attribute__((aligned(16))) T Vt[32 * S::TP];
  const int tid = threadIdx.x, lane = tid & 63, h = lane >> 5;
  const int head = blockIdx.y, b = blockIdx.z, q0 = blockIdx.x * kSaTile + (tid >> 6) * 32, qi = q0 + (lane & 31);
  const int N = a.N, inner = a.heads * 32;
  const int64_t ld = 3 * inner;
  const T* qb = reinterpret_cast<const T*>(a.qkv) + (int64_t)b * N * ld + head * 32;
  const typename S::Slice q = load_slice<T>(qb, ld, qi, N, h);
  f32x16 o;
#pragma unroll
  for (int i = 0; i < 16; ++i) o[i] = 0.f;
  float m = -INFINITY, l = 0.f;  // running maximum (in log2 units) and sum of this lane's query
  constexpr float cs = kSaScale * kLog2e;
  const int nkb = (N + kSaBlock - 1) / kSaBlock;
  typename S::vec_t kr[S::NV], vr[S::NV];
  block_load<T>(qb + inner, ld, 0, N, tid, kr);
  block_load<T>(qb + 2 * inner, ld, 0, N, tid, vr);
  for (int kb = 0; kb < nkb; ++kb) {
    wg_barrier();  // every wave is done with the previous block
    block_store<T>(Ks, nullptr, tid, kr);
    block_store<T>(nullptr, Vt, tid, vr);
    wg_barrier();
    if (kb + 1 < nkb) {  // in flight while this block is computed
      block_load<T>(qb + inner, ld, (kb + 1) * kSaBlock, N, tid, kr);
      block_load<T>(qb + 2 * inner, ld, (kb + 1) * kSaBlock, N, tid, vr);
    }
    if (q0 >= N) continue;  // wave-uniform: a wave without queries only stages
#pragma unroll
    for (int sub = 0; sub < 2; ++sub) {
      const int k0 = kb * kSaBlock + sub * 32;
      if (k0 >= N) break;  // a half that is walked holds at least one key: the maximum stays finite
      const f32x16 s = mm_rows<T>(Ks, sub, lane, q);
      float t[16], mx = -INFINITY;
#pragma unroll
      for (int r = 0; r < 16; ++r) {
        t[r] = k0 + mfma_row(r, lane) < N ? s[r] * cs : -INFINITY;
        mx = fmaxf(mx, t[r]);
      }
      mx = fmaxf(mx, __shfl_xor(mx, 32, 64));
      const float mn = fmaxf(m, mx), alpha = __builtin_amdgcn_exp2f(m - mn);
      float rs = 0.f;
#pragma unroll
      for (int r = 0; r < 16; ++r) {
        t[r] = __builtin_amdgcn_exp2f(t[r] - mn);
        rs += t[r];
      }
      rs += __shfl_xor(rs, 32, 64);
      l = l * alpha + rs;
      m = mn;
#pragma unroll
      for (int r = 0; r < 16; ++r) o[r] *= alpha;
      mm_t<T>(o, Vt, sub, lane, t);
    }
  }
  if (qi >= N) return;
  store_own<T>(reinterpret_cast<T*>(a.out) + ((int64_t)b * N + qi) * inner + head * 32, o, 1.f / l, lane);
  if (a.lse && h == 0) a.lse[((int64_t)b * a.heads + head) * N + qi] = (m + log2f(l)) * kLn2;
}

// ---------------------------------------------------------------------------------------------------------------------------
// dQ: a query tile walks the key blocks.  dS_ij = P_ij (dO_i . v_j - delta_i), dq_i = scale sum_j dS_ij k_j; delta_i =
// sum_d dO_id out_id (fp32) is left in `delta` [B][heads][N] for the dK / dV kernel.
template <typename T>
__global__ void __launch_bounds__(256) softattn_bwd_q_kernel(const SoftAttnBwdArgs a) {
  typedef Sa<T> S;
  __shared__ __attribute__((aligned(16))) T Ks[kSaBlock * S::RP];
  __shared__ __attribute__((aligned(16))) T Vs[kSaBlock * S::RP];
  __shared__ __attribute__((aligned(16))) T Kt[32 * S::TP];
  const int tid = threadIdx.x, lane = tid & 63, h = lane >> 5;
  const int head = blockIdx.y, b = blockIdx.z, q0 = blockIdx.x * kSaTile + (tid >> 6) * 32, qi = q0 + (lane & 31);
  const int N = a.N, inner = a.heads * 32;
  const int64_t ld = 3 * inner;
  const T* qb = reinterpret_cast<const T*>(a.qkv) + (int64_t)b * N * ld + head * 32;
  const int64_t ob = (int64_t)b * N * inner + head * 32;
  const typename S::Slice q = load_slice<T>(qb, ld, qi, N, h);
  const typename S::Slice dO = load_slice<T>(reinterpret_cast<const T*>(a.dout) + ob, inner, qi, N, h);
  float delta = 0.f;
  {
    const typename S::Slice oo = load_slice<T>(reinterpret_cast<const T*>(a.out) + ob, inner, qi, N, h);
#pragma unroll
    for (int i = 0; i < 16; ++i) delta = __builtin_fmaf((float)dO.v[i], (float)oo.v[i], delta);
    delta += __shfl_xor(delta, 32, 64);
  }
  const int64_t li = ((int64_t)b * a.heads + head) * N + qi;
  const float lse2 = qi < N ? a.lse[li] * kLog2e : 0.f;
  constexpr float cs = kSaScale * kLog2e;
  f32x16 dq;
#pragma unroll
  for (int i = 0; i < 16; ++i) dq[i] = 0.f;
  const int nkb = (N + kSaBlock - 1) / kSaBlock;
  typename S::vec_t kr[S::NV], vr[S::NV];
  block_load<T>(qb + inner, ld, 0, N, tid, kr);
  block_load<T>(qb + 2 * inner, ld, 0, N, tid, vr);
  for (int kb = 0; kb < nkb; ++kb) {
    wg_barrier();
    block_store<T>(Ks, Kt, tid, kr);
    block_store<T>(Vs, nullptr, tid, vr);
    wg_barrier();
    if (kb + 1 < nkb) {
      block_load<T>(qb + inner, ld, (kb + 1) * kSaBlock, N, tid, kr);
      block_load<T>(qb + 2 * inner, ld, (kb + 1) * kSaBlock, N, tid, vr);
    }
    if (q0 >= N) continue;
#pragma unroll
    for (int sub = 0; sub < 2; ++sub) {
      const int k0 = kb * kSaBlock + sub * 32;
      if (k0 >= N) break;
      const f32x16 s = mm_rows<T>(Ks, sub, lane, q);
      const f32x16 dp = mm_rows<T>(Vs, sub, lane, dO);
      float ds[16];
#pragma unroll
      for (int r = 0; r < 16; ++r) {
        const float p = k0 + mfma_row(r, lane) < N ? __builtin_amdgcn_exp2f(__builtin_fmaf(s[r], cs, -lse2)) : 0.f;
        ds[r] = p * (dp[r] - delta);
      }
      mm_t<T>(dq, Kt, sub, lane, ds);
    }
  }
  if (qi >= N) return;
  store_own<T>(reinterpret_cast<T*>(a.dqkv) + ((int64_t)b * N + qi) * ld + head * 32, dq, kSaScale, lane);
  if (h == 0) a.delta[li] = delta;
}

// dK / dV: a key tile walks the query blocks.  dv_j = sum_i P_ij dO_i, dk_j = scale sum_i dS_ij q_i, P recomputed from lse.
template <typename T>
__global__ void __launch_bounds__(256) softattn_bwd_kv_kernel(const SoftAttnBwdArgs a) {
  typedef Sa<T> S;
  __shared__ __attribute__((aligned(16))) T Qs[kSaBlock * S::RP];
  __shared__ __attribute__((aligned(16))) T Os[kSaBlock * S::RP];
  __shared__ __attribute__((aligned(16))) T Qt[32 * S::TP];
  __shared__ __attribute__((aligned(16))) T Ot[32 * S::TP];
  __shared__ float lse_s[kSaBlock], del_s[kSaBlock];
  const int tid = threadIdx.x, lane = tid & 63, h = lane >> 5;
  const int head = blockIdx.y, b = blockIdx.z, k0w = blockIdx.x * kSaTile + (tid >> 6) * 32, ki = k0w + (lane & 31);
  const int N = a.N, inner = a.heads * 32;
  const int64_t ld = 3 * inner;
  const T* qb = reinterpret_cast<const T*>(a.qkv) + (int64_t)b * N * ld + head * 32;
  const T* dob = reinterpret_cast<const T*>(a.dout) + (int64_t)b * N * inner + head * 32;
  const int64_t lb = ((int64_t)b * a.heads + head) * N;
  const typename S::Slice kk = load_slice<T>(qb + inner, ld, ki, N, h);
  const typename S::Slice vv = load_slice<T>(qb + 2 * inner, ld, ki, N, h);
  constexpr float cs = kSaScale * kLog2e;
  f32x16 dk, dv;
#pragma unroll
  for (int i = 0; i < 16; ++i) dk[i] = dv[i] = 0.f;
  const int nqb = (N + kSaBlock - 1) / kSaBlock;
  typename S::vec_t qr[S::NV], gr[S::NV];
  float lr = 0.f, dr = 0.f;  // threads 0..63: lse (log2 units; +inf past N, so P = 0) and delta of one query of the block
  auto load_stats = [&](int i0) {
    if (tid < kSaBlock) {
      const bool ok = i0 + tid < N;
      lr = ok ? a.lse[lb + i0 + tid] * kLog2e : INFINITY;
      dr = ok ? a.delta[lb + i0 + tid] : 0.f;
    }
  };
  block_load<T>(qb, ld, 0, N, tid, qr);
  block_load<T>(dob, inner, 0, N, tid, gr);
  load_stats(0);
  for (int ib = 0; ib < nqb; ++ib) {
    wg_barrier();
    block_store<T>(Qs, Qt, tid, qr);
    block_store<T>(Os, Ot, tid, gr);
    if (tid < kSaBlock) { lse_s[tid] = lr; del_s[tid] = dr; }
    wg_barrier();
    if (ib + 1 < nqb) {
      block_load<T>(qb, ld, (ib + 1) * kSaBlock, N, tid, qr);
      block_load<T>(dob, inner, (ib + 1) * kSaBlock, N, tid, gr);
      load_stats((ib + 1) * kSaBlock);
    }
    if (k0w >= N) continue;
#pragma unroll
    for (int sub = 0; sub < 2; ++sub) {
      if (ib * kSaBlock + sub * 32 >= N) break;
      const f32x16 s = mm_rows<T>(Qs, sub, lane, kk);
      const f32x16 dp = mm_rows<T>(Os, sub, lane, vv);
      float p[16], ds[16];
#pragma unroll
      for (int r = 0; r < 16; ++r) {
        const int qq = sub * 32 + mfma_row(r, lane);
        p[r] = __builtin_amdgcn_exp2f(__builtin_fmaf(s[r], cs, -lse_s[qq]));
        ds[r] = p[r] * (dp[r] - del_s[qq]);
      }
      mm_t<T>(dv, Ot, sub, lane, p);
      mm_t<T>(dk, Qt, sub, lane, ds);
    }
  }
  if (ki >= N) return;
  T* dst = reinterpret_cast<T*>(a.dqkv) + ((int64_t)b * N + ki) * ld + head * 32;
  store_own<T>(dst + inner, dk, kSaScale, lane);
  store_own<T>(dst + 2 * inner, dv, 1.f, lane);
}

// ---------------------------------------------------------------------------------------------------------------------------
static bool sa_ok(int B, int N, int heads) {
  return B >= 1 && N >= 1 && heads >= 1 && heads <= 65535 && B <= 65535;
}
hipError_t launch_softattn_fwd(int dtype, const SoftAttnArgs& a, hipStream_t s) {
  if (!sa_ok(a.B, a.N, a.heads) || !a.qkv || !a.out) return hipErrorInvalidValue;
  const dim3 grid((a.N + kSaTile - 1) / kSaTile, a.heads, a.B);
  return with_dtype(dtype, [&](auto t) {
    using T = decltype(t);
    static const char* const name = kernel_name<T>("softattn_fwd_kernel");
    note_kernel(name);
    hipLaunchKernelGGL(softattn_fwd_kernel<T>, grid, dim3(256), 0, s, a);
    return hipGetLastError();
  });
}
hipError_t launch_softattn_bwd(int dtype, const SoftAttnBwdArgs& a, hipStream_t s) {
  if (!sa_ok(a.B, a.N, a.heads) || !a.qkv || !a.out || !a.dout || !a.lse || !a.dqkv || !a.delta) return hipErrorInvalidValue;
  const dim3 grid((a.N + kSaTile - 1) / kSaTile, a.heads, a.B);
  return with_dtype(dtype, [&](auto t) {
    using T = decltype(t);
    static const char* const name = kernel_name<T>("softattn_bwd_kv_kernel");
    hipLaunchKernelGGL(softattn_bwd_q_kernel<T>, grid, dim3(256), 0, s, a);
    note_kernel(name);
    hipLaunchKernelGGL(softattn_bwd_kv_kernel<T>, grid, dim3(256), 0, s, a);
    return hipGetLastError();
  });
}

}  // namespace llie
