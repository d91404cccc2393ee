// Pieces shared by the kernels that compute a [BM][BN] fp32 tile on the 32x32 MFMA and hand it on through an fp32 LDS tile: the
// pointwise GEMM (gemm.hip), the implicit-GEMM 3x3 conv (conv.hip) and the folded up-sampling conv (upconv.hip).  Inlined into
// their callers: no kernels, no launches.  Waves are laid out WM x WN over the tile (wm = wave / WN, wn = wave % WN).
// Only what left every kernel's register and LDS budget untouched lives here; profiles/r26 lists what did not.
#pragma once
#include "common.h"

namespace llie {

// Pixel (py, px) of GEMM row m of an 8 x TW conv tile.  ROT (TW = 16, stride-1 reads of an 18-pixel-wide patch): row m is pixel
// (m / 16, (m % 16 + 14 (m / 16 & 1)) % 16) -- odd tile rows rotated by two pixels.  A ds_read_b128 is served in the 16-lane groups
// {0-3, 12-15, 20-27}, {4-11, 16-19, 28-31} (and + 32), and with the 80-byte pixel pitch a group is conflict-free iff its 16 patch
// pixels differ mod 16; lanes 16..31 sit one patch row (18 pixels) below lanes 0..15, so without the rotation pixels 12, 13 (4, 5)
// of a group collide with 22 + 6, 7: every A read two-way conflicted.  (Stride 2 reads every second pixel: two-way whatever the
// order.)
template <int TW, bool ROT>
__device__ __forceinline__ void tile_px(int m, int& py, int& px) {
  static_assert(!ROT || TW == 16, "the rotation is worked out for 16-pixel tile rows");
  py = m / TW;
  px = m % TW;
  if (ROT) px = (px + 14 * (py & 1)) & 15;
}

// Epilogue, first half: the accumulators of one 32-row MFMA block index -> the fp32 staging tile sC[WM * 32][CP], CP = BN + 4
// (row = wm * 32 + row in the block, column = (wn * NI + j) * 32 + column in the block).
template <int CP, int NI>
__device__ __forceinline__ void stage_acc_tile(float* sC, const f32x16 (&acc)[NI], int wm, int wn, int lane) {
#pragma unroll
  for (int j = 0; j < NI; ++j)
#pragma unroll
    for (int r = 0; r < 16; ++r) {
      const int row = wm * 32 + mfma_row(r, lane);
      const int col = (wn * NI + j) * 32 + (lane & 31);
      sC[row * CP + col] = acc[j][r];
    }
}

}  // namespace llie
