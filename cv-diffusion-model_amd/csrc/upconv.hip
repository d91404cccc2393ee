// The up-sampling 3x3 convs that never form the bilinear x2 image (gfx950): from per-phase folded weights (conv3x3_upfold_kernel) and
// from nine low-resolution tap maps blended on chip (conv3x3_upmaps_kernel).  The general kernel (conv.hip: conv3x3_kernel, MODE 1)
// interpolates the halo patch instead and takes every shape these two refuse.
#include <algorithm>

#include "common.h"
#include "kernels.h"
#include "mfma_tile.h"

namespace llie {

// =============================================================================================
// Up-sampling conv with the bilinear x2 folded into the weights (small.hip: upconv_fold_kernel, kernels.h: the blob's layout).
// Output pixel (2i + a, 2j + b) is a 3x3 conv, with the weights of phase (a, b), of the LOW-resolution input replicate-padded by
// one pixel: a stride-1 implicit GEMM with M = 8 x 16 low-resolution pixels, N = 128 (phase, cout) pairs, K = 9 taps x Cin.
// The 10 x 18 patch of a 32-channel chunk is a plain clamped copy -- no blend, a sixteenth of the loads per output of
// conv3x3_kernel's MODE 1.  An N tile never mixes row phases: one phase x 128 outputs, or (C64: Cout = 64) one row phase x both
// column phases x 64 outputs, where a wave column (wn) is one column phase.  Either way a low-resolution pixel's 128 columns
// are 256 contiguous bytes of the output.
// The outermost ring of the output, where the conv's zero padding must win over the replicate clamp, takes correction terms as
// extra k-steps ("taps" 9..15) into the same accumulators: three on the centre patch row for pixels of the image's first
// (a = 0) / last (a = 1) row, three on the centre column for its first / last column, one for the corner.  A lane whose pixel
// is not on that edge reads an all-zero patch pixel instead; workgroups that touch no edge run nine steps, and a wave skips
// the MFMAs of 32-row blocks without such a pixel.  Skipped and zero terms add exactly 0, so every pixel sees one fixed
// summation order: bitwise reproducible and batch invariant like the kernel above.
// Statistics: one slab entry per (low-resolution tile, phase): entry tile * 4 + phase.
// Workgroup order: edge workgroups run up to 16 steps per chunk where the others run 9, and a launch is only a few rounds of
// workgroups deep, so the heaviest go first (both edges, then one edge, then none) and the light ones fill the tail.
struct UpfoldStep { int kind, toff, sbase, cnt, k; };  // kind 0 interior tap, 1 row edge, 2 column edge, 3 corner
template <typename T, bool C64>
__global__ void __launch_bounds__(256) conv3x3_upfold_kernel(const Conv3Args a) {
  constexpr int NT = 256, WN = 2, TH = 8, TW = 16, BN = 128, MI = 2, NI = 2;
  constexpr int VEC = Elem<T>::VEC, VPR = 32 / VEC, PITCH = TilePitch<T>::value;
  constexpr int PH = TH + 2, PW = TW + 2, ZP = PH * PW;  // patch pixel ZP is all zero
  constexpr int B_PER = BN * VPR / NT;
  constexpr int CP = BN + 4;
  typedef typename Elem<T>::vec_t vec_t;
  static_assert(VEC == 8 && B_PER * NT == BN * VPR, "2-byte types only");

  extern __shared__ __align__(16) unsigned char smem[];
  T* sP = reinterpret_cast<T*>(smem);   // [PH * PW + 1][PITCH]
  T* sB = sP + (ZP + 1) * PITCH;        // [2][BN][PITCH]
  float* sC = reinterpret_cast<float*>(smem);

  const int tid = threadIdx.x, lane = tid & 63, wave = __builtin_amdgcn_readfirstlane(tid >> 6);
  const int wm = wave / WN, wn = wave % WN;
  const int H = a.Hi, W = a.Wi, Ho = 2 * H, Wo = 2 * W, C = a.Cin;
  const int tiles_x = W / TW, tiles = tiles_x * (H / TH);
  const int nb = C / BN;
  // blockIdx = (t * B + image) * cout blocks + cout block; t enumerates (row combination r, column combination c), heaviest first.
  // r: (row phase, tile row) -- 0 = (0, first) and 1 = (1, last) are the two that touch an image row edge; c likewise for
  // (column phase, tile column), or (C64: both column phases in one workgroup) the tile column alone, first and last touching.
  const int TY = H / TH, TX = tiles_x;
  const int NR = 2 * TY, NC = C64 ? TX : 2 * TX, HC = C64 && TX == 1 ? 1 : 2, nbk = C64 ? 1 : nb;
  int bid = blockIdx.x;
  const int nblk = bid % nbk; bid /= nbk;
  const int b = bid % a.B, t = bid / a.B;
  int r, c;
  {
    const int n_rc = 2 * HC, n_r = 2 * (NC - HC), n_c = (NR - 2) * HC;
    if (t < n_rc) { r = t / HC; c = t % HC; }
    else if (t < n_rc + n_r) { r = (t - n_rc) & 1; c = HC + ((t - n_rc) >> 1); }
    else if (t < n_rc + n_r + n_c) { r = 2 + (t - n_rc - n_r) / HC; c = (t - n_rc - n_r) % HC; }
    else { r = 2 + (t - n_rc - n_r - n_c) / (NC - HC); c = HC + (t - n_rc - n_r - n_c) % (NC - HC); }
  }
  const int pa = r < 2 ? r : (r - 2 < TY - 1 ? 0 : 1);                                   // row phase
  const int ty = r < 2 ? r * (TY - 1) : (r - 2 < TY - 1 ? r - 1 : r - 2 - (TY - 1));
  const int pb = C64 ? 0 : (c < 2 ? c : (c - 2 < TX - 1 ? 0 : 1));                       // column phase (of column 0)
  const int tx = C64 ? (c == 0 ? 0 : (c == 1 ? TX - 1 : c - 1)) : (c < 2 ? c * (TX - 1) : (c - 2 < TX - 1 ? c - 1 : c - 2 - (TX - 1)));
  const int tile = ty * TX + tx;
  const int iy0 = ty * TH, ix0 = tx * TW;
  const int phase0 = pa * 2 + pb;   // phase a * 2 + b of column 0 (C64: columns 64.. are phase0 + 1)
  const int n0 = nblk * BN;
  const int pbw = C64 ? wn : pb;  // column phase of this wave
  const int kv = (tid % VPR) * VEC;
  const T* in = reinterpret_cast<const T*>(a.in) + (size_t)b * H * W * C;
  const T* wbase = reinterpret_cast<const T*>(a.w);

  // which edges this workgroup / this wave touches
  const bool row_touch = pa == 0 ? iy0 == 0 : iy0 + TH == H;
  const bool col0 = ix0 == 0, col1 = ix0 + TW == W;
  const bool wg_col = C64 ? (col0 || col1) : ((phase0 & 1) ? col1 : col0);
  const bool wave_col = pbw ? col1 : col0;
  const int ie = pa ? TH - 1 : 0, je = pbw ? TW - 1 : 0;  // the edge pixels' tile coordinates
  const int nsteps = 9 + (row_touch ? 3 : 0) + (wg_col ? 3 : 0) + (row_touch && wg_col ? 1 : 0);
  auto decode = [&](int st) {
    if (st < 9) return UpfoldStep{0, ((st / 3) * PW + st % 3) * PITCH, 0, 9, st};
    st -= 9;
    if (row_touch) {
      if (st < 3) return UpfoldStep{1, (PW + st) * PITCH, 36, 3, st};
      st -= 3;
    }
    if (st < 3) return UpfoldStep{2, (st * PW + 1) * PITCH, 48, 3, st};
    return UpfoldStep{3, (PW + 1) * PITCH, 60, 1, 0};
  };

  f32x16 acc[MI][NI];
#pragma unroll
  for (int i = 0; i < MI; ++i)
#pragma unroll
    for (int j = 0; j < NI; ++j)
#pragma unroll
      for (int r = 0; r < 16; ++r) acc[i][j][r] = 0.f;

  // odd tile rows are rotated by two pixels in the GEMM row order (mfma_tile.h: tile_px, conflict-free A reads on the 18-pixel rows)
  const int zoff = ZP * PITCH + (lane >> 5) * 16;
  int arow[MI], amask[MI], bmask[MI];  // amask: bit k = this lane's pixel takes part in steps of kind k; bmask: some pixel of the block does
#pragma unroll
  for (int i = 0; i < MI; ++i) {
    const int blk = wm * MI + i;
    int py, px;
    tile_px<TW, true>(blk * 32 + (lane & 31), py, px);
    arow[i] = (py * PW + px) * PITCH + (lane >> 5) * 16;
    const bool lr = row_touch && py == ie, lc = wave_col && px == je;
    amask[i] = 1 | (lr ? 2 : 0) | (lc ? 4 : 0) | (lr && lc ? 8 : 0);
    const bool br = row_touch && (ie >> 1) == blk;  // a block is two tile rows; every block holds a pixel of each column
    bmask[i] = 1 | (br ? 2 : 0) | (wave_col ? 4 : 0) | (br && wave_col ? 8 : 0);
  }

  vec_t rb[B_PER];
  auto prefetch_w = [&](const UpfoldStep& st, int c0) {
#pragma unroll
    for (int i = 0; i < B_PER; ++i) {
      const int n = (tid + i * NT) / VPR;
      const int phase = C64 ? phase0 + (n >> 6) : phase0, co = C64 ? (n & 63) : n0 + n;
      rb[i] = ld_vec<T>(wbase + ((size_t)(st.sbase + phase * st.cnt + st.k) * C + co) * C + c0 + kv);
    }
  };
  auto stage_w = [&](int buf) {
#pragma unroll
    for (int i = 0; i < B_PER; ++i) st_vec<T>(sB + buf * (BN * PITCH) + ((tid + i * NT) / VPR) * PITCH + kv, rb[i]);
  };

  // the patch of one chunk: loads issued one chunk ahead, kept raw in registers during the current chunk's steps
  constexpr int P_ITEMS = (PH * PW * VPR + NT - 1) / NT;
  vec_t praw[P_ITEMS];
  auto issue_patch = [&](int c0) {
#pragma unroll
    for (int it = 0; it < P_ITEMS; ++it) {
      const int i = tid + it * NT;
      if (i < PH * PW * VPR) {
        const int pix = i / VPR;
        const int gy = min(max(iy0 - 1 + pix / PW, 0), H - 1), gx = min(max(ix0 - 1 + pix % PW, 0), W - 1);  // replicate padding
        praw[it] = ld_vec<T>(in + ((size_t)gy * W + gx) * C + c0 + kv);
      }
    }
  };
  auto commit_patch = [&]() {
#pragma unroll
    for (int it = 0; it < P_ITEMS; ++it) {
      const int i = tid + it * NT;
      if (i < PH * PW * VPR) st_vec<T>(sP + (i / VPR) * PITCH + kv, praw[it]);
    }
  };
  if (tid < VPR) {
    vec_t z;
#pragma unroll
    for (int e = 0; e < VEC; ++e) z[e] = (T)0.f;
    st_vec<T>(sP + ZP * PITCH + kv, z);
  }

  const int anyb = bmask[0] | bmask[1];  // bit k: this wave has MFMAs in steps of kind k
  auto run_step = [&](int st, const UpfoldStep& cur, int c0) {
    if ((anyb >> cur.kind) & 1) {
      T fa[MI][16], fb[NI][16];
#pragma unroll
      for (int i = 0; i < MI; ++i) {
        if (!((bmask[i] >> cur.kind) & 1)) continue;
        const T* p = sP + (((amask[i] >> cur.kind) & 1) ? arow[i] + cur.toff : zoff);
#pragma unroll
        for (int q = 0; q < 16 / VEC; ++q) *reinterpret_cast<vec_t*>(&fa[i][q * VEC]) = *reinterpret_cast<const vec_t*>(p + q * VEC);
      }
#pragma unroll
      for (int j = 0; j < NI; ++j) {
        const T* p = sB + (st & 1) * (BN * PITCH) + ((wn * NI + j) * 32 + (lane & 31)) * PITCH + (lane >> 5) * 16;
#pragma unroll
        for (int q = 0; q < 16 / VEC; ++q) *reinterpret_cast<vec_t*>(&fb[j][q * VEC]) = *reinterpret_cast<const vec_t*>(p + q * VEC);
      }
#pragma unroll
      for (int i = 0; i < MI; ++i) {
        if (!((bmask[i] >> cur.kind) & 1)) continue;
#pragma unroll
        for (int j = 0; j < NI; ++j) Mfma<T>::chunk(fa[i], fb[j], acc[i][j]);
      }
    }
    if (st + 1 < nsteps) {
      stage_w((st + 1) & 1);  // its last readers finished before the previous barrier
      if (st + 2 < nsteps) prefetch_w(decode(st + 2), c0);
    }
    wg_barrier();  // next W tile visible; everyone done with this one (and, after the last step, with the patch)
  };

  issue_patch(0);
  for (int c0 = 0; c0 < C; c0 += 32) {
    prefetch_w(decode(0), c0);
    commit_patch();
    stage_w(0);
    prefetch_w(decode(1), c0);
    wg_barrier();  // patch and W tile of step 0 visible
    if (c0 + 32 < C) issue_patch(c0 + 32);
#pragma unroll
    for (int st = 0; st < 9; ++st) run_step(st, decode(st), c0);
    for (int st = 9; st < nsteps; ++st) run_step(st, decode(st), c0);
  }

  // ---- epilogue: conv3x3_kernel's, with the phase in the output address and in the slab entry
  constexpr int VR = BN / VEC, RPP = NT / VR, SROWS = 2 * 32;
  const int cv = tid % VR, r0 = tid / VR;
  const int ephase = C64 ? phase0 + (cv * VEC >> 6) : phase0, ech = C64 ? (cv * VEC & 63) : n0 + cv * VEC;  // of this thread's columns
  float bias[VEC], s1[VEC], s2[VEC];
#pragma unroll
  for (int e = 0; e < VEC; ++e) {
    bias[e] = a.bias ? a.bias[ech + e] : 0.f;
    s1[e] = 0.f;
    s2[e] = 0.f;
  }
  T* outp = reinterpret_cast<T*>(a.out) + (size_t)b * Ho * Wo * C;
#pragma unroll
  for (int pi = 0; pi < MI; ++pi) {
    if (pi) wg_barrier();
    stage_acc_tile<CP>(sC, acc[pi], wm, wn, lane);
    wg_barrier();
    for (int srow = r0; srow < SROWS; srow += RPP) {
      const int row = ((srow >> 5) * MI + pi) * 32 + (srow & 31);  // pixel index inside the tile
      float v[VEC];
      const float* pc = sC + srow * CP + cv * VEC;
#pragma unroll
      for (int e = 0; e < VEC; ++e) v[e] = pc[e] + bias[e];
      int py, px;
      tile_px<TW, true>(row, py, px);
      const int oy = 2 * (iy0 + py) + pa, ox = 2 * (ix0 + px) + (ephase & 1);
      vec_t ov = f32_to_vec<T>(v);
      st_vec_pol<T>(outp + ((size_t)oy * Wo + ox) * C + ech, ov, a.nt != 0);
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
      const int phase = C64 ? phase0 + (c >> 6) : phase0, ch = C64 ? (c & 63) : n0 + c;
      a.stats[((size_t)((b * tiles + tile) * 4 + phase) * 2 + which) * C + ch] = t;
    }
  }
}

bool conv3x3_upfold_ok(int dtype, int Hi, int Wi, int C) {
  return (dtype == 1 || dtype == 2) && Hi > 0 && Wi > 0 && Hi % 8 == 0 && Wi % 16 == 0 && (C == 64 || (C > 0 && C % 128 == 0));
}
int conv3x3_upfold_ntiles(int Ho, int Wo) { return 4 * (Ho / 16) * (Wo / 32); }  // (low-resolution 8 x 16 tile, phase) pairs

template <typename T, bool C64>
static hipError_t launch_upfold_cfg(const Conv3Args& a, hipStream_t s) {
  constexpr int PITCH = TilePitch<T>::value;
  constexpr size_t tiles = (size_t)(10 * 18 + 1 + 2 * 128) * PITCH * sizeof(T);
  constexpr size_t ctile = (size_t)64 * (128 + 4) * 4 + (size_t)4 * 2 * 128 * 4;
  constexpr size_t lds = tiles > ctile ? tiles : ctile;
  static_assert(lds <= 48 * 1024, "static LDS limit");
  const unsigned grid = (unsigned)(a.B * (a.Hi / 8) * (a.Wi / 16) * (C64 ? 2 : 4 * (a.Cin / 128)));
  static const char* const name = kernel_name<T>("conv3x3_upfold_kernel", C64 ? 64 : 128);
  note_kernel(name);
  hipLaunchKernelGGL((conv3x3_upfold_kernel<T, C64>), dim3(grid), dim3(256), lds, s, a);
  return hipGetLastError();
}
// a.w = the folded blob (upconv_fold_elems(C) elements of the compute type); a.mode is ignored
hipError_t launch_conv3x3_upfold(int dtype, const Conv3Args& a, hipStream_t s) {
  if (a.Cin != a.Cout || a.B < 1 || !conv3x3_upfold_ok(dtype, a.Hi, a.Wi, a.Cin)) return hipErrorInvalidValue;
  return with_dtype2(dtype, [&](auto t) { return a.Cin == 64 ? launch_upfold_cfg<decltype(t), true>(a, s) : launch_upfold_cfg<decltype(t), false>(a, s); });
}

// =============================================================================================
// Up-sampling conv from nine low-resolution tap maps.  conv3x3(up2(x)) is linear in x and up2 is fixed, so with Z_t = W_t x (nine
// 1x1 maps of the LOW-resolution input, one per tap t = (dy, dx)) the output is bias + the sum over the taps that fall inside
// the 2H x 2W image of up2(Z_t) at the tap's position: 9/4 C^2 multiply-adds per output pixel instead of 9 C^2.  up2 = bilinear
// x2, align_corners=False = weights 3/4, 1/4 on the replicate-clamped low-resolution neighbours, so the conv's zero padding is a
// dropped term, never a correction: every workgroup does the same work.
// Work item = one image, one 8 x 16 low-resolution tile, 32 output channels.  One 8-wave workgroup per compute unit (the maps take
// 104 KB of LDS) works through items blockIdx.x, + gridDim.x, ...; the first operand loads of the next item are issued before
// the blend of this one, and this one's stores drain under the next one's MFMAs (6-10 us per launch against one workgroup per
// item, profiles/r24).
//   1. Maps: a plain GEMM, no shifted reads.  288 (tap, cout) rows of the [9][Cout][Cin] weights x the replicate-clamped 10 x 18
//      patch (180 pixels, padded to 192 columns) over K = Cin, on the 16x16x32 MFMA with the weights as its A operand: a lane then
//      holds four consecutive channels of one tap of one pixel.  Wave (wn, wp) = 9 row blocks x 3 pixel blocks.  Both operands of
//      a 32-channel chunk are staged in LDS as unpadded 64-byte rows, 16-byte slot s of row r at slot s ^ 2 (r >> 3 & 1): with it
//      every ds_read_b128 lane group of a fragment read covers 64 different banks.  Two buffers, the global loads of the next two
//      chunks in registers under this chunk's MFMAs, one barrier per chunk.
//   2. The maps, rounded to T, replace the operand buffers: [180 pixels][9 taps][32 channels], the eight channel quads of a
//      (pixel, tap) rotated by pixel >> 1 so that the 16 pixels of a block's ds_write_b64 fall into 32 different banks; the pixel
//      pitch (144 dwords) keeps the blend's reads conflict-free.
//   3. Blend, separable: a thread owns two channels of one tile column and four tile rows.  Per patch row it forms H[dy][b], the
//      three column taps of row tap dy blended for column phase b (7 map reads per dy), and an output pixel (2i + a, 2j + b) is
//      the same combination of H over rows i - 1, i, i + 1.  One fixed order of fp32 operations for every pixel, border terms
//      multiplied by an exact 0: bitwise reproducible and batch invariant like the two kernels above.
//   4. + bias, round to T, store; GroupNorm partials from the rounded values go to slab entry 4 tile of the tile's four entries,
//      the other three are written as zeros.
// Item order: the channel blocks of one tile run on ONE XCD (workgroups are dealt round-robin to the eight XCDs and the item
// stride is a multiple of 8), so a patch comes from HBM once and is re-read from that XCD's L2.  Which workgroup computes an
// item changes no bit of it.
template <typename T>
__global__ void __launch_bounds__(512) conv3x3_upmaps_kernel(const Conv3Args a, const int nitems) {
  constexpr int NT = 512, TH = 8, TW = 16, PW = TW + 2, NPIX = (TH + 2) * PW, BN = 32, NROW = 9 * BN;
  constexpr int PROWS = 192, SROWS = PROWS + NROW;  // rows of one operand buffer: patch pixels (180, padded), then weight rows
  constexpr int P_ITEMS = (NPIX * 4 + NT - 1) / NT, W_ITEMS = (NROW * 4 + NT - 1) / NT;
  typedef typename Elem<T>::vec_t vec_t;
  typedef T t2 __attribute__((ext_vector_type(2)));
  typedef T t4 __attribute__((ext_vector_type(4)));
  static_assert(Elem<T>::VEC == 8, "2-byte types only");

  extern __shared__ __align__(16) unsigned char smem[];
  T* sS = reinterpret_cast<T*>(smem);                                            // [2][SROWS][32]
  T* sM = reinterpret_cast<T*>(smem);                                            // [NPIX][NROW], after the K loop
  float* red = reinterpret_cast<float*>(smem + (size_t)NPIX * NROW * sizeof(T));  // [8 waves][2][BN]

  const int tid = threadIdx.x, lane = tid & 63, wave = __builtin_amdgcn_readfirstlane(tid >> 6);
  const int H = a.Hi, W = a.Wi, Ho = 2 * H, Wo = 2 * W, C = a.Cin;
  const int tiles_x = W / TW, tiles = tiles_x * (H / TH), nb = C / BN, ntot = a.B * tiles;
  const T* wbase = reinterpret_cast<const T*>(a.w);

  struct Item { int b, tile, iy0, ix0, n0; };
  auto decode = [&](int id) {
    int t, nblk;
    if (ntot & 7) {
      t = id / nb; nblk = id % nb;
    } else {
      const int slot = id >> 3;
      t = (slot / nb) * 8 + (id & 7); nblk = slot % nb;
    }
    Item it;
    it.b = t / tiles; it.tile = t % tiles;
    it.iy0 = (it.tile / tiles_x) * TH; it.ix0 = (it.tile % tiles_x) * TW; it.n0 = nblk * BN;
    return it;
  };

  // ---- operand loads of one work item: its patch and its 288 weight rows, one 32-channel chunk at a time
  const int ks = tid & 3, kv = ks * 8;
  const T* in = nullptr;
  int poff[P_ITEMS], woff[W_ITEMS];
  float nbias[2];
  auto setup = [&](const Item& it) {
    in = reinterpret_cast<const T*>(a.in) + (size_t)it.b * H * W * C;
#pragma unroll
    for (int q = 0; q < P_ITEMS; ++q) {
      const int pix = min((tid + q * NT) >> 2, NPIX - 1);
      const int gy = min(max(it.iy0 - 1 + pix / PW, 0), H - 1), gx = min(max(it.ix0 - 1 + pix % PW, 0), W - 1);  // replicate padding
      poff[q] = (gy * W + gx) * C + kv;
    }
#pragma unroll
    for (int q = 0; q < W_ITEMS; ++q) {
      const int row = min((tid + q * NT) >> 2, NROW - 1);
      woff[q] = ((row >> 5) * C + it.n0 + (row & 31)) * C + kv;
    }
    nbias[0] = a.bias ? a.bias[it.n0 + 2 * (tid & 15)] : 0.f;
    nbias[1] = a.bias ? a.bias[it.n0 + 2 * (tid & 15) + 1] : 0.f;
  };
  auto srow = [](int r, int s) { return r * 32 + ((s ^ (((r >> 3) & 1) << 1)) << 3); };  // element offset of slot s of row r
  // two register sets: the loads of chunk k + 2 are issued when chunk k starts and written to LDS when chunk k + 1 ends
  vec_t rp[2][P_ITEMS], rw[2][W_ITEMS];
  auto issue = [&](int set, int c0) {
#pragma unroll
    for (int q = 0; q < P_ITEMS; ++q)
      if (tid + q * NT < NPIX * 4) rp[set][q] = ld_vec<T>(in + poff[q] + c0);
#pragma unroll
    for (int q = 0; q < W_ITEMS; ++q)
      if (tid + q * NT < NROW * 4) rw[set][q] = ld_vec<T>(wbase + woff[q] + c0);
  };
  auto commit = [&](int set, int buf) {
    T* sp = sS + buf * (SROWS * 32);
#pragma unroll
    for (int q = 0; q < P_ITEMS; ++q)
      if (tid + q * NT < NPIX * 4) st_vec<T>(sp + srow((tid + q * NT) >> 2, ks), rp[set][q]);
#pragma unroll
    for (int q = 0; q < W_ITEMS; ++q)
      if (tid + q * NT < NROW * 4) st_vec<T>(sp + PROWS * 32 + srow((tid + q * NT) >> 2, ks), rw[set][q]);
  };

  const int wn = wave & 1, wp = wave >> 1;
  int prd[3];
#pragma unroll
  for (int i = 0; i < 3; ++i) prd[i] = srow(min((wp * 3 + i) * 16 + (lane & 15), NPIX - 1), lane >> 4);  // rows 180..191: a copy of 179, never kept
  const int wrd = PROWS * 32 + srow(wn * 9 * 16 + (lane & 15), lane >> 4);  // + 16 rows per block: the slot does not change

  int item = blockIdx.x;
  Item cur = decode(item);
  setup(cur);
  issue(0, 0);
  if (C > 32) issue(1, 32);
  while (true) {
    const float bias[2] = {nbias[0], nbias[1]};
    // ---- 1. maps
    f32x4acc acc[9][3];
#pragma unroll
    for (int jj = 0; jj < 9; ++jj)
#pragma unroll
      for (int i = 0; i < 3; ++i)
#pragma unroll
        for (int r = 0; r < 4; ++r) acc[jj][i][r] = 0.f;
    commit(0, 0);  // (the previous item's maps are done with: the barrier that ends the loop body)
    wg_barrier();
    auto chunk = [&](int c0, int buf) {  // buf = (c0 / 32) & 1, a constant at both call sites: the register sets stay registers
      if (c0 + 64 < C) issue(buf, c0 + 64);
      const T* sp = sS + buf * (SROWS * 32);
      vec_t pf[3];
#pragma unroll
      for (int i = 0; i < 3; ++i) pf[i] = *reinterpret_cast<const vec_t*>(sp + prd[i]);
#pragma unroll
      for (int jj = 0; jj < 9; ++jj) {
        const vec_t wf = *reinterpret_cast<const vec_t*>(sp + wrd + jj * (16 * 32));
#pragma unroll
        for (int i = 0; i < 3; ++i) acc[jj][i] = mfma16x16<T>(wf, pf[i], acc[jj][i]);
      }
      if (c0 + 32 < C) commit(buf ^ 1, buf ^ 1);  // its last readers finished before the previous barrier
      wg_barrier();                               // next chunk visible; after the last chunk: everyone done with the operand buffers
    };
    for (int c0 = 0; c0 < C; c0 += 64) {
      chunk(c0, 0);
      if (c0 + 32 < C) chunk(c0 + 32, 1);
    }

    // ---- 2. maps to LDS, rounded to T
    // (lv, tv: the lane and thread number again, opaque to the compiler -- it would otherwise compute the ~60 LDS and output
    // addresses of steps 2 to 4 once, in front of the item loop, and keep them in registers through the K loop: 35 spilled)
    int lv = lane, tv = tid;
    asm volatile("" : "+v"(lv), "+v"(tv));
#pragma unroll
    for (int i = 0; i < 3; ++i) {
      const int p = (wp * 3 + i) * 16 + (lv & 15);
      if (p < NPIX) {
#pragma unroll
        for (int jj = 0; jj < 9; ++jj) {
          const int n = (wn * 9 + jj) * 16 + 4 * (lv >> 4);  // rows n .. n + 3 of D: four channels of tap n >> 5
          t4 v;
#pragma unroll
          for (int r = 0; r < 4; ++r) v[r] = (T)acc[jj][i][r];
          *reinterpret_cast<t4*>(sM + p * NROW + (n >> 5) * 32 + (((((n & 31) >> 2) + (p >> 1)) & 7) << 2)) = v;
        }
      }
    }
    wg_barrier();

    // the next item's first two chunks: their latency runs under this item's blend
    const int next = item + (int)gridDim.x;
    const bool has_next = next < nitems;
    Item nx = cur;
    if (has_next) {
      nx = decode(next);
      setup(nx);
      issue(0, 0);
      if (C > 32) issue(1, 32);
    }

    // ---- 3. blend + 4. epilogue
    const int cp = tv & 15, j = (wave & 3) * 4 + ((tv >> 4) & 3), i0 = (wave >> 2) * 4;  // two channels, tile column, first tile row
    const float kl = cur.ix0 + j == 0 ? 0.f : 1.f, kr = cur.ix0 + j == W - 1 ? 0.f : 1.f;
    auto ldz = [&](int pix, int tap, float (&z)[2]) {
      const t2 v = *reinterpret_cast<const t2*>(sM + pix * NROW + tap * 32 + ((((cp >> 1) + (pix >> 1)) & 7) << 2) + (cp & 1) * 2);
      z[0] = (float)v[0];
      z[1] = (float)v[1];
    };
    // H[dy][b] of patch row pr at this thread's column: up-sampled columns 2j + b + dx - 1 of map (dy, dx), summed over dx
    auto hrow = [&](int pr, float (&h)[3][2][2]) {
      const int pix = pr * PW + j;  // patch column j = tile column j - 1
#pragma unroll
      for (int dy = 0; dy < 3; ++dy) {
        float l0[2], m0[2], l1[2], m1[2], r1[2], m2[2], r2[2];
        ldz(pix, dy * 3, l0); ldz(pix + 1, dy * 3, m0);
        ldz(pix, dy * 3 + 1, l1); ldz(pix + 1, dy * 3 + 1, m1); ldz(pix + 2, dy * 3 + 1, r1);
        ldz(pix + 1, dy * 3 + 2, m2); ldz(pix + 2, dy * 3 + 2, r2);
#pragma unroll
        for (int e = 0; e < 2; ++e) {
          h[dy][0][e] = 0.75f * ((kl * l0[e] + m1[e]) + m2[e]) + 0.25f * ((kl * m0[e] + l1[e]) + r2[e]);
          h[dy][1][e] = 0.75f * ((kr * r2[e] + m1[e]) + m0[e]) + 0.25f * ((kr * m2[e] + r1[e]) + l0[e]);
        }
      }
    };
    float s1[2] = {0.f, 0.f}, s2[2] = {0.f, 0.f};
    T* outp = reinterpret_cast<T*>(a.out) + (size_t)cur.b * Ho * Wo * C + cur.n0 + 2 * cp;
    float h[3][3][2][2];
    hrow(i0, h[0]);
    hrow(i0 + 1, h[1]);
#pragma unroll
    for (int r = 0; r < 4; ++r) {
      hrow(i0 + r + 2, h[(r + 2) % 3]);
      const auto& hm = h[r % 3];
      const auto& hc = h[(r + 1) % 3];
      const auto& hp = h[(r + 2) % 3];
      const int iy = cur.iy0 + i0 + r;
      const float kt = iy == 0 ? 0.f : 1.f, kb = iy == H - 1 ? 0.f : 1.f;
#pragma unroll
      for (int pb = 0; pb < 2; ++pb) {
        t2 o0, o1;
#pragma unroll
        for (int e = 0; e < 2; ++e) {
          const float v0 = 0.75f * ((kt * hm[0][pb][e] + hc[1][pb][e]) + hc[2][pb][e]) + 0.25f * ((kt * hc[0][pb][e] + hm[1][pb][e]) + hp[2][pb][e]);
          const float v1 = 0.75f * ((kb * hp[2][pb][e] + hc[1][pb][e]) + hc[0][pb][e]) + 0.25f * ((kb * hc[2][pb][e] + hp[1][pb][e]) + hm[0][pb][e]);
          o0[e] = (T)(v0 + bias[e]);
          o1[e] = (T)(v1 + bias[e]);
          const float q0 = (float)o0[e], q1 = (float)o1[e];
          s1[e] += q0; s2[e] += q0 * q0;
          s1[e] += q1; s2[e] += q1 * q1;
        }
        t2* d0 = reinterpret_cast<t2*>(outp + ((size_t)(2 * iy) * Wo + 2 * (cur.ix0 + j) + pb) * C);
        t2* d1 = reinterpret_cast<t2*>(outp + ((size_t)(2 * iy + 1) * Wo + 2 * (cur.ix0 + j) + pb) * C);
        if (a.nt) {
          __builtin_nontemporal_store(o0, d0);
          __builtin_nontemporal_store(o1, d1);
        } else {
          *d0 = o0;
          *d1 = o1;
        }
      }
    }
    if (a.stats) {
#pragma unroll
      for (int e = 0; e < 2; ++e) {
        s1[e] += __shfl_xor(s1[e], 16, 64); s1[e] += __shfl_xor(s1[e], 32, 64);
        s2[e] += __shfl_xor(s2[e], 16, 64); s2[e] += __shfl_xor(s2[e], 32, 64);
      }
      if (lane < 16) {
#pragma unroll
        for (int e = 0; e < 2; ++e) {
          red[(wave * 2 + 0) * BN + 2 * cp + e] = s1[e];
          red[(wave * 2 + 1) * BN + 2 * cp + e] = s2[e];
        }
      }
      wg_barrier();
      if (tid < 8 * BN) {  // entry k of the tile's four, sum / sum of squares, channel
        const int k = tid >> 6, which = (tid >> 5) & 1, c = tid & 31;
        float tt = 0.f;
        if (k == 0) {
#pragma unroll
          for (int w = 0; w < NT / 64; ++w) tt += red[(w * 2 + which) * BN + c];
        }
        a.stats[((size_t)((cur.b * tiles + cur.tile) * 4 + k) * 2 + which) * C + cur.n0 + c] = tt;
      }
    }
    if (!has_next) break;
    wg_barrier();  // everyone done with the maps and the statistics scratch
    cur = nx;
    item = next;
  }
}

bool conv3x3_upmaps_ok(int dtype, int Hi, int Wi, int C) {
  return (dtype == 1 || dtype == 2) && Hi > 0 && Wi > 0 && Hi % 8 == 0 && Wi % 16 == 0 && C > 0 && C % 32 == 0;
}

// compute units of the current device (one workgroup fits on each), asked once per device
static int upmaps_cus() {
  static std::atomic<int> cached[64];
  int dev = 0;
  if (hipGetDevice(&dev) != hipSuccess) return 0;
  int n = cached[dev & 63].load(std::memory_order_acquire);
  if (n == 0) {
    if (hipDeviceGetAttribute(&n, hipDeviceAttributeMultiprocessorCount, dev) != hipSuccess) return 0;
    cached[dev & 63].store(n, std::memory_order_release);
  }
  return n;
}

static int upmaps_nitems(int B, int Hi, int Wi, int C) { return B * (Hi / 8) * (Wi / 16) * (C / 32); }
// the rule: one workgroup per compute unit, or per item where there are fewer items
static hipError_t upmaps_rule(int nitems, int* wgs) {
  int cus = upmaps_cus();
  if (cus < 1) return hipErrorInvalidDevice;
  if (cus & 7) cus = 1 << 30;  // the XCD order of the items counts on a stride that is a multiple of 8: else one item per workgroup
  *wgs = std::min(nitems, cus);
  return hipSuccess;
}
int conv3x3_upmaps_workgroups(int B, int Hi, int Wi, int C, hipError_t* err) {
  int wgs = 0;
  *err = B < 1 || !conv3x3_upmaps_ok(1, Hi, Wi, C) ? hipErrorInvalidValue : upmaps_rule(upmaps_nitems(B, Hi, Wi, C), &wgs);
  return wgs;
}

template <typename T>
static hipError_t launch_upmaps_t(const Conv3Args& a, hipStream_t s, int workgroups) {
  constexpr size_t lds = (size_t)180 * 288 * sizeof(T) + (size_t)8 * 2 * 32 * 4;  // the maps (> the operand buffers) + the statistics
  static_assert(lds >= (size_t)2 * (192 + 288) * 32 * sizeof(T) && lds <= 160 * 1024, "LDS");
  static std::atomic<uint64_t> attr_done{0};
  if (hipError_t e = ensure_max_lds(reinterpret_cast<const void*>(&conv3x3_upmaps_kernel<T>), (int)lds, attr_done); e != hipSuccess) return e;
  const int nitems = upmaps_nitems(a.B, a.Hi, a.Wi, a.Cin);
  int wgs = std::min(nitems, workgroups);
  if (workgroups == 0)
    if (hipError_t e = upmaps_rule(nitems, &wgs); e != hipSuccess) return e;
  static const char* const name = kernel_name<T>("conv3x3_upmaps_kernel");
  note_kernel(name);
  hipLaunchKernelGGL((conv3x3_upmaps_kernel<T>), dim3((unsigned)wgs), dim3(512), lds, s, a, nitems);
  return hipGetLastError();
}
// a.w = the plain [9][Cout][Cin] weights of launch_conv3x3; a.mode is ignored.  workgroups 0: the rule; n >= 1: min(n, items),
// any of which computes the same bits (the kernel's decode is a bijection on the items whatever the stride)
hipError_t launch_conv3x3_upmaps(int dtype, const Conv3Args& a, hipStream_t s, int workgroups) {
  if (a.Cin != a.Cout || a.B < 1 || workgroups < 0 || !conv3x3_upmaps_ok(dtype, a.Hi, a.Wi, a.Cin)) return hipErrorInvalidValue;
  return with_dtype2(dtype, [&](auto t) { return launch_upmaps_t<decltype(t)>(a, s, workgroups); });
}

}  // namespace llie
