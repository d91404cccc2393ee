// Host-side launch API of the gfx950 kernels (implemented in the *.hip files of this directory).
// Everything is asynchronous on the given stream; dtype is an llie_dtype value.
#pragma once
#include <hip/hip_runtime.h>
#include <stdint.h>

namespace llie {

// ACT_RELU6_S6 (pointwise GEMM prologue, 2-byte T): a' = clamp01(a * as + ab) with tables that ALREADY hold scale / 6 and
// shift / 6 (GnFinalizeArgs::post_scale), i.e. relu6(.) / 6 for one FMA with a free clamp; the GEMM multiplies its
// accumulators by 6 in the epilogue.  Every K-segment of such a GEMM must use it.
enum Act : int { ACT_NONE = 0, ACT_RELU6 = 1, ACT_SILU = 2, ACT_RELU6_S6 = 3 };

// Launchers of the profiled kernel classes record the name of the kernel they dispatched (template
// arguments included, as rocprofv3 prints them) so that llie_profile_report can aggregate per kernel.
void note_kernel(const char* name);
const char* last_kernel();

// ---------------------------------------------------------------------------------------------
// Tuning knobs (tune.cpp: the table of names, defaults, environment variables and value rules behind llie_tune).  Process-global;
// the engine and the launchers read the fields directly.  The reasons behind each default are in tune.cpp, next to its row.
struct Knobs {
  int use_irbx;       // "irbx": recompute form of the inverted-residual block (irbx.hip) wherever irbx_supported()
  int irbx_project;   // "irbx_project": recompute blocks without h2 (expand_pool + expand_dw_project): 1 = every shape irbx_project_supported
                      // names, 2 = its identity-residual shapes only, 0 = none (expand_dw + project GEMM)
  int wide_project;   // "wide_project": the wide decoder blocks wide_project_supported names without h2 (dwconv3x3_pool + dwconv3x3_project)
  int wide_gram;      // "wide_gram" (1 = maps of at least kWideGramMinPixels pixels, 2 = every map): the 192 -> 64 wide block takes norm2's tables from the Gram of its input (gram.hip), pw_expand stores the
                      // activated h1 and adds the SE pool totals: no pool pass (0 = dwconv3x3_pool from the stored h1)
  int gram;           // "gram": norm2 statistics of the recompute form from the Gram matrix (gram.hip); 0 = expand_stats; 2 = at every size
  int nt_min_mb;      // "nt_min_mb": tensors of at least this many MiB are stored non-temporally by the producers in nt_mask
  int nt_mask;        // "nt_mask": 1 expand_dw, 2 pw_expand, 4 dwconv3x3, 8 project / attention GEMMs, 16 dense 3x3 convs
  int se_mfma;        // "se_mfma": SE MLP of the wide blocks as two MFMA launches; 0 = the row-parallel pair
  int bwd_async;      // "bwd_async": weight-gradient kernels of the backward pass on a side stream
  int upconv_fold;    // "upconv_fold": up-sampling convs from folded weights wherever upconv_fold_supported(); 0 = blend in the kernel
  int upconv_maps;    // "upconv_maps": up-sampling convs from nine low-resolution tap maps wherever upconv_maps_supported(); 0 = the rule of upconv_fold alone
  int enhance_split;  // "enhance_split": concurrent branches of the captured enhance graph (< 2: a single chain)
  int graph_max_steps;  // "graph_max_steps": loops of more steps than this run as plain launches, never captured
  // read by the launchers
  int pwx;            // "pwx": the activation-stationary expand GEMM (pwx.hip) where pw_expand_supported(); 0 = the tile kernel
  int gemm_bk;        // "gemm_bk": K chunk of pw_gemm (0 = automatic, 32 = 32-wide chunks)
  int irbx_dbuf;      // "irbx_dbuf": expand_dw's double-buffered variant for 32-channel inputs
  int irbx_grid[3];   // "irbx_grid" (all), "irbx_grid2/4/6": workgroups per expand_dw launch, per input width 32 / 64 / 96 (0 = heuristics)
  // 1 = launch the cycle-stamped diagnostic build of the family; "irbx_stamp": 1 expand_dw, 2 expand_pool, 3 expand_dw_project
  int gemm_stamp, pwx_stamp, conv_stamp, irbx_stamp;
  int epoch;          // llie_tune calls so far: keys the graph cache and the zero-region sizes, which bake kernel choices in
};
extern Knobs g_knobs;

// Where a kernel family's cycle-stamped diagnostic builds write (host side, tune.cpp): `slots` counters per wave, wave after wave.
// One instance per family, defined next to its launchers; llie_debug_*_stamps reads it back.
struct StampSink {
  int slots;
  size_t max_waves;  // launches of more waves are refused; 0 = unbounded
  unsigned long long* buf = nullptr;
  size_t cap = 0, waves = 0;  // waves the buffer holds, waves of the last stamped launch
  // the buffer a stamped launch of `waves` waves writes (grown on demand); hipErrorInvalidValue above max_waves
  hipError_t arm(size_t launch_waves, unsigned long long** stamps);
  // out[i] = mean over the waves of the last stamped launch of entry wave * slots + i, out[slots] = the number of waves;
  // hipErrorInvalidValue when nothing was stamped
  hipError_t fetch(double* out) const;
};
extern StampSink g_gemm_stamps, g_pwx_stamps, g_conv_stamps, g_irbx_stamps;

// Per-channel statistics slab written by producers for the next GroupNorm:
//   slab[((b * ntiles + tile) * 2 + {0: sum, 1: sum of squares}) * C + c]   (fp32)
// `tile` enumerates the producer's row tiles inside one image.  gn_finalize reduces slabs in a fixed
// order, so results are bitwise reproducible (no float atomics anywhere in the engine).
struct StatSrc {
  const float* slab;  // null = absent
  int ntiles;
  int ch;
};

// One K-segment of a pointwise GEMM's A operand: NHWC rows [M][ch] with an optional per-(image,
// channel) affine + activation applied on load:  a' = act(a * as[b][c] + ab[b][c]).
struct GemmSeg {
  const void* ptr;
  int ch;
  const float* as;   // [B][aff_ld] (pre-offset to this segment's first channel) or null (identity)
  const float* ab;   // same layout, or null (treated as 0 when as != null)
  int aff_ld;        // row stride of as/ab in floats
  int act;           // Act
};

// out[M][N] = sum_seg act(A_seg) * W[N][Ktot]^T (+bias[N]) (+res[M][N]);  optional stats slab of `out`.
struct GemmArgs {
  GemmSeg seg[3];
  int nseg;
  const void* w;      // [N][Ktot] T, K order = segments concatenated
  const float* bias;  // [N] or null
  const void* res;    // [M][N] T or null
  void* out;          // [M][N] T
  float* stats;       // slab of out or null
  int M, N, K;        // K = sum of seg ch
  int P;              // rows (pixels) per image; M = B * P
  int nostore;        // 1: compute and write only the statistics slab (out may be null)
  const void* dot;    // optional [M][N] T: the slab then holds (sum out*dot, sum out) instead of (sum, sum of squares)
  int nt;             // 1: `out` is stored non-temporally (set by the engine for tensors beyond the Infinity Cache, common.h: st_vec_pol)
  unsigned long long* stamps;  // diagnostic builds only (knob "gemm_stamp")
};
hipError_t launch_pw_gemm(int dtype, const GemmArgs& a, hipStream_t s);
int pw_gemm_tile_rows(int P);  // BM used for a given P
int pw_gemm_ntiles(int P);     // stats slab tiles per image = ceil(P / BM)

// Expanding pointwise GEMM in activation-stationary form (pwx.hip; 2-byte T, every segment ACT_RELU6_S6):
//   out[M][N] = sum_seg clamp01(A_seg * as + ab) . Wf^T,  Wf = the [N][K] weights times 6, pre-packed in MFMA fragment order
//   (launch_pack_expand), plus the statistics slab of `out` at 128-row granularity (== pw_gemm_tile_rows for P % 128 == 0).
struct ExpandArgs {
  GemmSeg seg[3];
  int nseg;
  const void* wf;
  void* out;
  float* stats;
  int M, N, K, P;
  int nsplit;  // set by the launcher
  int nt;      // 1: non-temporal output stores (see GemmArgs::nt)
  unsigned long long* stamps;  // diagnostic builds only (knob "pwx_stamp")
  // launch_pw_expand_act: norm2's tables [B][N] DIVIDED BY 6 (DwArgs::s6), the depthwise weights [9][N] fp32, the image size
  // (H * W == P) and the fixed-point SE pool totals [B][N] it adds to; `stats` is not used
  const float* as2; const float* ab2; const float* wd;
  unsigned long long* pool_tot;
  int H, W;
};
__host__ __device__ inline long long pw_expand_pack_index(int n, int k, int K) {
  const int lane = (n & 31) + 32 * ((k >> 3) & 1);
  return ((((long long)(n >> 5) * (K >> 4) + (k >> 4)) * 64 + lane) << 3) + (k & 7);
}
bool pw_expand_supported(int dtype, const GemmSeg* seg, int nseg, int M, int N, int K, int P);
int pw_expand_nsplit(int M, int N);  // the channel split launch_pw_expand takes: workgroups = M / 128 x this
bool pw_expand_serves_k(int K);  // the kernel exists for this input width (the builder packs the fragment-ordered weight copy only then)
hipError_t launch_pw_expand(int dtype, const ExpandArgs& a, hipStream_t s);
// The activating form (wide block 192 -> 768 with norm2's tables from the wide Gram): stores a = T(clamp01(h1 as2 + ab2)) instead
// of h1 and adds the SE pool totals of dwconv3x3(a, T(6 wd)) to pool_tot, as dwconv3x3_pool would from the stored h1
bool pw_expand_act_supported(int dtype, const GemmSeg* seg, int nseg, int M, int N, int K, int P, int H, int W);
hipError_t launch_pw_expand_act(int dtype, const ExpandArgs& a, hipStream_t s);
hipError_t launch_pack_expand(int dtype, const float* src, void* dst, int N, int K, float scale, hipStream_t s);

// GroupNorm statistics -> per-(image, channel) affine tables.
//   mean/var over groups of cg = C/32 channels x P pixels from up to two slabs (virtual concat),
//   as[b][c] = rstd*gamma[c]*(1+fs),  ab[b][c] = (beta[c] - mean*rstd*gamma[c])*(1+fs) + fh
//   with (fs, fh) = FiLM (scale, shift) = film[b*film_stride + {c, C + c}] or (0,0) when film == null.
struct GnFinalizeArgs {
  StatSrc src[2];
  int C;             // total channels (sum of src ch)
  int groups;        // 32
  int P;             // pixels per image
  const float* gamma;
  const float* beta;
  const float* film; // null or [rows][2C] fp32
  int64_t film_stride;  // row stride in floats (0 = same row for every image)
  float eps;
  float* as;         // [B][C]
  float* ab;         // [B][C]
  int B;
  int Creal;         // 0 = C; otherwise the groups partition channels [0, Creal) and the rest (zero padding) gets a zero affine
  float* mean_out;   // optional [B][groups] (training: kept for the backward pass)
  float* rstd_out;
  float post_scale;  // 0 = 1: as and ab are multiplied by it (1/6 for consumers that carry ReLU6 as clamp01(z / 6))
};
hipError_t launch_gn_finalize(const GnFinalizeArgs& a, hipStream_t s);

// Depthwise 3x3 (pad 1, stride 1) with fused input affine + ReLU6 and SE average-pool partials.
//   in/out NHWC [B][H][W][C] T; w [9][C] fp32 (tap-major); pool slab [B][ntiles][C] fp32.
struct DwArgs {
  const void* in; void* out;
  const float* as; const float* ab;  // [B][C]
  const float* w;
  float* pool;
  unsigned long long* pool_tot;  // inference: [B][C] fixed-point (x 2^24) channel totals, added with integer atomics (no pool slab)
  int B, H, W, C;
  int no_act;        // 1: prologue is the affine alone (backward: dh2 = da3*gate + dmean/P), 0: affine + ReLU6
  int s6;            // 1 (2-byte T, forward): as / ab hold scale / 6 and shift / 6 (GnFinalizeArgs::post_scale); the
                     // prologue is clamp01(x * as + ab) = relu6(.) / 6 (one FMA, free clamp) and the weights are taken x 6
  // backward epilogue (all four set, pool null): out = conv * [0 < bx*bas + bab < 6], and
  // bslab[b][tile][0][c] = sum out, [1][c] = sum out*bx over 8-row segments (tile = dwconv_ntiles numbering)
  const void* bx; const float* bas; const float* bab; float* bslab;
  int nt;            // 1: non-temporal output stores (see GemmArgs::nt)
};
hipError_t launch_dwconv3x3(int dtype, const DwArgs& a, hipStream_t s);

// GroupNorm-2 statistics of the recompute form from the Gram matrix of the activated block input (gram.hip, 2-byte T).
struct GramArgs {
  const void* x0; const void* x1; int c0, c1;   // block input (virtual concat), K = c0 + c1 in {32, 64, 96}, c0 % 8 == 0
  const float* as1; const float* ab1;            // [B][K] GroupNorm-1 affine DIVIDED BY 6 (a' = clamp01(.) = relu6 / 6)
  float* part;                                    // [B][P / gram_rows][upper 32 x 32 blocks x 1024 + K] workgroup partials
  float* gtot;                                    // [B][K * K + K]: G = sum_px a' a'^T in full, then m = sum_px a'
  unsigned int* tickets;                          // [B], zero at launch (the kernel leaves them zero)
  int B, P, RP;                                   // RP is set by the launcher (gram_rows)
};
struct GramFinalizeArgs {
  const float* gtot;   // as written by gram_stats_kernel
  const void* w1;      // [Chid][K] T: the expand weights the main pass multiplies with
  int K, Chid, groups, P, B;
  const float* gamma; const float* beta;   // norm2
  const float* film; int64_t film_stride;  // null or [rows][2 Chid]
  float eps;
  float* as; float* ab;                    // [B][Chid]
  float post_scale;
};
int gram_rows(int K, int P);
size_t gram_part_floats(int K, int P);
bool gram_supported(int dtype, int K, int c0, int P);
hipError_t launch_gram_stats(int dtype, const GramArgs& a, hipStream_t s);
hipError_t launch_gram_finalize(int dtype, const GramFinalizeArgs& a, hipStream_t s);

// The same statistics for the wide decoder block 192 -> 64 (hid 768), known BEFORE the expand GEMM runs, so that pw_expand can
// store the activated h1 and add the SE pool totals itself (gram.hip).  G is kept as its 21 upper 32 x 32 blocks in the order of
// gram_wide_block, then m: kGramWideFloats floats per image.  M_g / u_g (launch_gram_group_weights, load time) use the same layout
// in fp64, one set per GroupNorm group, off-diagonal blocks doubled.
constexpr int kGramWideK = 192, kGramWideBlocks = 21, kGramWideFloats = kGramWideBlocks * 1024 + kGramWideK;
__host__ __device__ inline void gram_wide_block(int q, int* bi, int* bj) {  // block q of the layout = G[32 bi ..][32 bj ..]
  const int w = q / 7, t = q % 7, x = 2 * w, y = 2 * ((w + 1) % 3);
  *bi = t == 2 || t >= 5 ? x + 1 : x;
  *bj = t == 0 ? x : (t <= 2 ? x + 1 : (t == 3 || t == 5 ? y : y + 1));
}
struct GramWideArgs {
  const void* x0; const void* x1; int c0, c1;   // block input (virtual concat), c0 + c1 == 192, c0 % 8 == 0
  const float* as1; const float* ab1;            // [B][192] GroupNorm-1 affine DIVIDED BY 6
  float* part;                                    // [B][P / gram_wide_rows(P)][kGramWideFloats] workgroup partials
  float* gblk;                                    // [B][kGramWideFloats]
  int B, P, RP;                                   // RP is set by the launcher (gram_wide_rows)
};
struct GramGroupFinalizeArgs {
  const float* gblk;   // as written by launch_gram_wide
  const double* mg;    // [groups][kGramWideFloats] of the layer (launch_gram_group_weights)
  int K, Chid, groups, P, B;
  const float* gamma; const float* beta;   // norm2
  const float* film; int64_t film_stride;  // null or [rows][2 Chid]
  float eps;
  float* as; float* ab;                    // [B][Chid]
  float post_scale;
};
int gram_wide_rows(int P);
size_t gram_wide_part_floats(int P);
bool gram_wide_supported(int dtype, int K, int c0, int Chid, int P);
hipError_t launch_gram_wide(int dtype, const GramWideArgs& a, hipStream_t s);  // the Gram pass and the sum of its partials
hipError_t launch_gram_group_finalize(const GramGroupFinalizeArgs& a, hipStream_t s);
// wpack: the layer's packed expand weights T(6 W) (launch_pack_expand / LoadDesc::dst_f), already written on this stream; `state` as in launch_load_all
hipError_t launch_gram_group_weights(int dtype, const void* wpack, double* mg, int Chid, int K, hipStream_t s, const unsigned long long* state = nullptr);

// Recompute form of the block's front half (irbx.hip, 2-byte T): expand_stats writes only h1's statistics slab
// ([B][P / irbx_stats_rows(P)][2][Chid]), expand_dw produces h2 and the SE pool slab ([B][irbx_pool_tiles][Chid]).
// The blocks irbx_project_supported names (identity-residual 32 -> 32 and 64 -> 64; 96 -> 32 with a skip conv) go without h2 as
// well: expand_pool adds the SE pool totals from a pass that only rebuilds h1, and expand_dw_project, given the gate, multiplies
// the depthwise result by Wp itself, adds the shortcut and writes y.
struct IrbxArgs {
  const void* x0; const void* x1; int c0, c1;   // block input (virtual concat), Cin = c0 + c1 in {32, 64, 96, 128}
  const float* as1; const float* ab1;            // [B][Cin]   GroupNorm-1 affine DIVIDED BY 6 (post_scale): a' = clamp01(.) = relu6 / 6
  const void* w1;                                // [Chid][Cin] T
  const float* as2; const float* ab2;            // [B][Chid]  GroupNorm-2 + FiLM affine (ReLU6 follows), undivided
  const float* wd;                               // [9][Chid] fp32 depthwise weights, tap-major
  void* out; float* pool;                        // expand_dw outputs
  unsigned long long* pool_tot;                  // or: [B][Chid] fixed-point channel totals (see DwArgs::pool_tot)
  float* stats;                                  // expand_stats output
  int B, H, W, Chid;
  unsigned long long* dbg;                       // diagnostic builds only (knob "irbx_stamp")
  int nt;                                        // 1: h2 is stored non-temporally (see GemmArgs::nt)
  // expand_dw_project: SE gate [B][Chid], project weights [Cout][ldp] T, y [B][H][W][Cout] T and y's statistics slab
  // [B][irbx_project_tiles][2][Cout].  Identity form: Cout = Cin = c0, x1 absent, ldp = Chid (set by the launcher); skip form:
  // columns [Chid, Chid + Cin) of wp are the skip conv's weights (the engine's K-concatenated matrix)
  const float* gate; const void* wp; void* y; float* ystats;
  int ldp;
  // wide decoder blocks (dwconv3x3_pool / dwconv3x3_project, below): the stored h1 [B][H][W][Chid] T; as2 / ab2 are then norm2's
  // tables DIVIDED BY 6 (the s6 form of DwArgs), since h1 is the real tensor and not an accumulator / 6
  const void* h1;
  int h1_act;  // dwconv3x3_project: 1 = h1 holds the activated values a = T(clamp01(h1 as2 + ab2)) (launch_pw_expand_act); as2 / ab2 unused
};
// Wide decoder blocks without h2 (irbx.hip), from the stored h1: dwconv3x3_pool adds the SE pool totals from nine sums of
// a = clamp01(h1 as2 + ab2) (the restatement of expand_pool), and dwconv3x3_project, given the gate, runs depthwise, gate, project
// GEMM and skip conv per 8 x 16 tile and writes y with its statistics slab [B][irbx_project_tiles][2][Cout].  The layers of
// wide_project_supported only: 2-byte T, unpadded, skip conv, (Cin, Chid, Cout) in {(192, 768, 64), (384, 1536, 128)},
// c0 % 16 == 0, H % 8 == 0, W % 16 == 0.  The pool pass itself needs no more than Chid in {768, 1536} and the map rule.
bool wide_project_supported(int dtype, int Cin, int c0, int Chid, int Cout, bool skip, bool padded, int H, int W);
hipError_t launch_dwconv3x3_pool(int dtype, const IrbxArgs& a, hipStream_t s);     // needs h1, as2 / ab2, wd; adds into pool_tot
hipError_t launch_dwconv3x3_project(int dtype, const IrbxArgs& a, int cout, hipStream_t s);
bool irbx_supported(int dtype, int Cin, int c0, int Chid, int H, int W);
int irbx_pool_tiles(int H, int W);
constexpr int kIrbxProjectIdentity = 1, kIrbxProjectSkip = 2;  // forms of the project tail
int irbx_project_supported(int dtype, int Cin, int c0, int Chid, int Cout, bool skip, int H, int W);  // 0 or the form
int irbx_project_tiles(int H, int W);
int irbx_stats_rows(int P);
// launch plan of expand_dw / expand_dw_project (irbx.hip: irbx_plan): tiles per workgroup (0 = the image's tiles split evenly over
// grid.x workgroups, knobs "irbx_grid*"), 64-channel chunks per workgroup, grid.x, grid.y (grid.z = B).  Shapes of irbx_supported only
struct IrbxPlan { int tpw, cpw, gx, gy; };
IrbxPlan irbx_plan(int Cin, int B, int H, int W, bool project);
hipError_t launch_expand_stats(int dtype, const IrbxArgs& a, hipStream_t s);
hipError_t launch_expand_dw(int dtype, const IrbxArgs& a, hipStream_t s);
hipError_t launch_expand_pool(int dtype, const IrbxArgs& a, hipStream_t s);        // needs as2 / ab2 / wd; adds into pool_tot
hipError_t launch_expand_dw_project(int dtype, const IrbxArgs& a, int cout, bool skip, hipStream_t s);
int dwconv_ntiles(int H, int W);  // pool slab entries per image: (H/8 row segments) x (W / strip width)
int dw_pick_tyl(int B, int H, int W, int chunks);

// Squeeze-and-Excitation MLP (efficient_unet.py:96-100) in two launches.
//   fc1: mean[b][c] = sum_tiles pool / P (own launch);  hid[b][j] = relu6(b1[j] + sum_c W1[j][c] * mean[b][c])
//   fc2: gate[b][c] = sigmoid(b2[c] + sum_j W2[c][j] * hid[b][j])
struct SeArgs {
  const float* pool; int ntiles; int P;
  int pool_stride;                  // floats between consecutive tile entries of one image (0 = C)
  const void* w1; const float* b1;  // [Cs][C] T
  const void* w2; const float* b2;  // [C][Cs] T
  float* mean;                      // [B][C] scratch
  float* hid;                       // [B][Cs]
  float* gate;                      // [B][C]
  int B, C, Cs;
  const unsigned long long* tot;    // launch_se_gate: [B][C] fixed-point pool totals (kPoolFixScale)
  long long* pre;                   // launch_se_mlp_mfma: [B][Cs] 2^-32 fixed-point fc1 pre-activations, zero at launch
};
// wide blocks, 2-byte T: fc1 and fc2 as two MFMA launches with the batch as the rows of a 32 x 32 tile (small.hip)
bool se_mlp_mfma_supported(int dtype, const SeArgs& a);
hipError_t launch_se_mlp_mfma(int dtype, const SeArgs& a, hipStream_t s);
constexpr float kPoolFixScale = 16777216.f;  // 2^24: per-tile pool partials are rounded to 2^-24 before the integer add
hipError_t launch_se_gate(int dtype, const SeArgs& a, hipStream_t s);  // mean -> fc1 -> ReLU6 -> fc2 -> sigmoid, one launch
hipError_t launch_se_fc1(int dtype, const SeArgs& a, hipStream_t s);
hipError_t launch_se_fc2(int dtype, const SeArgs& a, hipStream_t s);

// Time embedding (efficient_unet.py:60-76, 412-417) and all FiLM projections in one go.
//   temb[r] = W3 * silu(W1 * sinemb(t[r]) + b1) + b3;  film[r][f] = bf[f] + sum_k Wf[f][k]*silu(temb[r][k])
//   rows = 1 (uniform t) or B.
struct TimeArgs {
  const int64_t* t; int rows;
  int dim;  // sinusoidal dim = base_channels
  const float* freqs;  // [dim/2] exp(-ln(1e4)*i/half), tabulated on the host at create time
  int T;    // time_embed_dim
  const float* w1; const float* b1; const float* w3; const float* b3;
  float* temb;        // [rows][T]
  float* silu_temb;   // [rows][T]
  float* emb_out;     // optional [rows][dim]: the sinusoidal embedding itself
};
hipError_t launch_time_embed(const TimeArgs& a, hipStream_t s);
struct FilmArgs {
  const float* silu_temb; int rows; int T;
  const float* wf; const float* bf;  // [F][T], [F]
  float* film;                       // [rows][F]
  int F;
};
hipError_t launch_film(const FilmArgs& a, hipStream_t s);
hipError_t launch_silu_rows(const float* in, float* out, int64_t n, hipStream_t s);

// Dense 3x3 convolutions.
//   init: fp32 NCHW planes (two 3-channel halves = virtual concat) -> NHWC T, + stats slab.
struct InitConvArgs {
  const float* x0; const float* x1; int c0, c1;  // c0 + c1 = Cin
  const float* w; const float* bias;             // [Cin*9][Cout] (repacked), [Cout] fp32
  const void* wp;                                // 2-byte T only: MFMA-packed [5][2][Cout][8] T, or null (VALU kernel)
  void* out; float* stats;
  int B, H, W, Cout;
};
hipError_t launch_init_conv(int dtype, const InitConvArgs& a, hipStream_t s);
int init_conv_ntiles(int H, int W, bool mfma);  // mfma: the 2-byte engines' kernel (8 x 32 tiles); else 16 x 16
//   final: NHWC T -> affine + SiLU -> 3x3 conv C->Cout(3) -> fp32 NCHW; the MFMA variant (2-byte T)
//   can apply LCMScheduler.step to its own output in the epilogue (fuse_step).
struct StepCoef { float sa, sb, sap, sbp; int is_last; int vpred; int clamp_x0; int sampler; };  // llie_step_coef; sampler 1 = DDIM
struct FinalConvArgs {
  const void* in; const float* as; const float* ab;
  const float* w; const float* bias;             // [9][C][4] (repacked, zero padded), [Cout]
  const void* wp;                                // 2-byte T only: MFMA-packed [C/32][18][2][4][8] T, or null (VALU kernel)
  float* out;                                    // noise prediction (may be null when fuse_step)
  int B, H, W, C, Cout;
  int fuse_step;                                 // 1: also prev = step(eps, sample, noise) (and clamp)
  StepCoef coef;
  const float* sample; const float* noise; float* prev; float* clamped;
};
hipError_t launch_final_conv(int dtype, const FinalConvArgs& a, hipStream_t s);
//   implicit-GEMM MFMA conv: mode 0 = stride-2 downsample, 1 = bilinear x2 upsample then conv (pad 1),
//   2 = plain stride-1 conv (training: conv on the stored upsampled tensor, and every input-gradient conv).
struct Conv3Args {
  const void* in;      // NHWC [B][Hi][Wi][C]
  const void* w;       // [9][Cout][Cin] T
  const float* bias;
  void* out;           // NHWC [B][Ho][Wo][Cout]
  float* stats;        // slab of out or null
  int B, Hi, Wi, Cin, Cout;
  int mode;
  int nt;              // 1: non-temporal output stores (see GemmArgs::nt)
  unsigned long long* stamps;  // diagnostic builds only (knob "conv_stamp")
};
hipError_t launch_conv3x3(int dtype, const Conv3Args& a, hipStream_t s);
int conv3x3_ntiles(int Ho, int Wo);
//   the up-sampling conv (mode 1) from folded weights: the fixed bilinear x2 lives in per-phase 3x3 weights on the low-resolution
//   input, so the kernel blends nothing (upconv.hip: conv3x3_upfold_kernel).  Cin == Cout == C; `w` = the folded blob of
//   launch_upconv_fold: 64 sets of [Cout][Cin] T, phase p = 2 a + b for output pixels (2i + a, 2j + b):
//     set p * 9 + r * 3 + s   interior tap (r, s) on the replicate-padded input
//     set 36 + p * 3 + s      row-edge correction (already negated), first (a = 0) / last (a = 1) image row
//     set 48 + p * 3 + r      column-edge correction (already negated), first (b = 0) / last (b = 1) image column
//     set 60 + p              corner correction
//   stats: [B][conv3x3_upfold_ntiles(Ho, Wo)][2][C]
bool conv3x3_upfold_ok(int dtype, int Hi, int Wi, int C);  // the kernel's contract: 2-byte dtype, Hi % 8 == 0, Wi % 16 == 0, C = 64 or a multiple of 128
hipError_t launch_conv3x3_upfold(int dtype, const Conv3Args& a, hipStream_t s);
int conv3x3_upfold_ntiles(int Ho, int Wo);
//   the up-sampling conv (mode 1) from nine low-resolution tap maps, blended on chip (upconv.hip: conv3x3_upmaps_kernel): a quarter of
//   the multiply-adds.  Cin == Cout == C; `w` = the plain [9][C][C] T weights of launch_conv3x3 (no folded blob).
//   stats: [B][conv3x3_ntiles(Ho, Wo)][2][C], four entries per low-resolution 8 x 16 tile: the first carries the sums, three are zero
bool conv3x3_upmaps_ok(int dtype, int Hi, int Wi, int C);  // the kernel's contract: 2-byte dtype, Hi % 8 == 0, Wi % 16 == 0, C a multiple of 32
//   The grid is sized to the chip: workgroup g of n works through items g, g + n, ... (item = image, tile, 32 output channels).
//   workgroups 0 = the rule, conv3x3_upmaps_workgroups (min(items, compute units); one per item where the compute units are no
//   multiple of 8; *err says why it has no answer); n >= 1 = min(n, items) workgroups, the same bits on any n (what the tests use)
hipError_t launch_conv3x3_upmaps(int dtype, const Conv3Args& a, hipStream_t s, int workgroups = 0);
int conv3x3_upmaps_workgroups(int B, int Hi, int Wi, int C, hipError_t* err);
constexpr int kUpconvFoldSets = 64;
inline size_t upconv_fold_elems(int C) { return (size_t)kUpconvFoldSets * C * C; }

// Linear attention core (efficient_unet.py:288-302) on qkv NHWC [B][N][3*inner].
struct AttnArgs {
  const void* qkv; int B, N, heads;  // dim_head = 32
  float* kv;      // [nsplit][B][heads][32][33]: rows 0..31 = kv[d][e], column 32 = ksum[d]; partial sums over
                  // position ranges, added in split order by the second pass (deterministic)
  void* out;      // [B][N][inner] T
  int nsplit;     // linattn_nsplit(N)
};
int linattn_nsplit(int N);
hipError_t launch_linattn_kv(int dtype, const AttnArgs& a, hipStream_t s);
hipError_t launch_linattn_out(int dtype, const AttnArgs& a, hipStream_t s);

// Softmax attention core (efficient_unet.py:349-353) in flash form on MFMA (softattn.hip), same qkv / out layout as AttnArgs.
struct SoftAttnArgs {
  const void* qkv; void* out;  // [B][N][3 * inner], [B][N][inner] T; dim_head = 32, scale = 32^-0.5
  float* lse;                  // [B][heads][N] log-sum-exp of the scaled logits, or null (inference)
  int B, N, heads;
};
hipError_t launch_softattn_fwd(int dtype, const SoftAttnArgs& a, hipStream_t s);
// dqkv of the core given d(out): a dQ kernel per query tile (it leaves delta = rowsum(dout * out) for the second), then a
// dK / dV kernel per key tile; P is recomputed from lse.  No atomics.
struct SoftAttnBwdArgs {
  const void* qkv; const void* out; const void* dout; const float* lse; void* dqkv;
  float* delta;                // [B][heads][N] scratch
  int B, N, heads;
};
hipError_t launch_softattn_bwd(int dtype, const SoftAttnBwdArgs& a, hipStream_t s);

// y = x*as + ab (+ res), NHWC rows [M][C]; optional stats slab of y (tiles of 64 rows).
struct AffineAddArgs {
  const void* x; const float* as; const float* ab; const void* res; void* y; float* stats;
  int M, C, P;
};
hipError_t launch_affine_add(int dtype, const AffineAddArgs& a, hipStream_t s);
constexpr int kAffineTileRows = 64;

// Layout conversion at the operator boundary: fp32 NCHW <-> NHWC T (+ stats slab, tiles of 64 pixels).
//   x is [B][Csrc][P]; channels [coff, coff+C) are converted.
hipError_t launch_nchw_to_nhwc(int dtype, const float* x, void* y, float* stats, int B, int C, int P, int Csrc,
                               int coff, hipStream_t s);
hipError_t launch_nhwc_to_nchw(int dtype, const void* x, float* y, int B, int C, int P, hipStream_t s, int Cdst = 0,
                               int coff = 0);  // y is [B][Cdst][P]; the C channels land at [coff, coff+C)

// Weight repack at load time (fp32 reference layout -> engine layout).  One device function (small.hip: load_one) states every
// layout once, driven by a LoadDesc; it runs either over a device table of descriptors, one per parameter (launch_load_all: an
// optimiser step changes every parameter, and 300+ small repack launches would cost more than the repack itself), or over a single
// descriptor passed by value (launch_load_one: llie_load_param).  Offsets are bytes into the weight blob; -1 = no such copy.
//   PK_F32    fp32 copy
//   PK_MAT    [rows][cols] -> dst[r * ld + col0 + c], T or (as_t == 0) fp32;  dst_t: transposed [cols][rows] T;
//             dst_f: times fscale in MFMA fragment order (pw_expand_pack_index), T
//   PK_CONV3  OIHW 3x3 -> [tap][Op][Ip] T;  dst_t: [8 - tap][Ip][Op] T, the weights of the input-gradient conv
//   PK_DW     [C][1][3][3] -> [tap][Op] fp32;  dst_t: taps flipped, [8 - tap][Op] fp32
//   PK_INIT   input conv OIHW -> fp32 [I * 9][Op];  dst_t: the MFMA pack [tap][Op][8] T
//   PK_FINAL  output conv OIHW (O <= 4) -> fp32 [9][Ip][4];  dst_t: the MFMA pack [Ip / 32][18][2][4][8] T
// Padding entries (Op / Ip beyond O / I, taps and channels the packs round up to) are never written: they keep the zeros of
// llie_create's memset of the blob.
enum PKind : int { PK_F32, PK_MAT, PK_CONV3, PK_DW, PK_INIT, PK_FINAL };
struct LoadDesc {
  const float* src;
  PKind kind;
  int as_t;            // PK_MAT: destination in the compute dtype (1) or fp32 (0)
  int rows, cols, ld, col0, O, I, Op, Ip;  // Op / Ip: padded destination dims of the conv / depthwise layouts
  long long numel, dst, dst_t, dst_f;
  float fscale;
};
// state (optional, device): [0] = content hash of the last load, [1] = 1 when the parameters changed (set by launch_params_hash);
// with a state the kernel is a no-op when [1] == 0
hipError_t launch_load_all(int dtype, const LoadDesc* descs_dev, int n, char* blob, hipStream_t s, const unsigned long long* state = nullptr);
hipError_t launch_load_one(int dtype, const LoadDesc& d, char* blob, hipStream_t s);
hipError_t launch_params_hash(const LoadDesc* descs_dev, int n, unsigned long long* partial, unsigned long long* state, int force,
                              hipStream_t s);
// OIHW [C][C][3][3] fp32 -> the 64 folded sets of the up-sampling conv (layout above): fp64 arithmetic, one rounding to the compute
// dtype (1 or 2).  `state` as in launch_load_all: with one, a no-op when the parameters did not change.
hipError_t launch_upconv_fold(int dtype, const float* src, void* dst, int C, hipStream_t s, const unsigned long long* state = nullptr);

// uint8 HWC RGB <-> normalised fp32 NCHW with bilinear resize (scripts/inference.py:99-134), bit-exact with hostio.py.
hipError_t launch_preprocess_u8(const uint8_t* img, int B, int H0, int W0, float* out, int S, hipStream_t s);
hipError_t launch_postprocess_u8(const float* x, int B, int S, uint8_t* img, int H0, int W0, hipStream_t s);

// LCM scheduler elementwise ops (fp32).
hipError_t launch_lcm_step(const float* eps, const float* x, const float* noise, float* prev, float* x0,
                           float* clamped, int64_t n, StepCoef c, hipStream_t s);
hipError_t launch_add_noise(const float* x0, const float* noise, const int64_t* t, const float* acp, float* out,
                            int B, int64_t per, int velocity, int table_len, hipStream_t s);
hipError_t launch_copy_probe(const void* src, void* dst, int64_t bytes, hipStream_t s);
hipError_t launch_rw_probe(const void* src, void* dst, int64_t units, int r, int w, int nt, hipStream_t s);


// =============================================================================================
// Training: backward kernels (bwd.hip, wgrad.hip).  Gradients of activations are NHWC T like the
// activations; parameter gradients are fp32 in the reference's state_dict layout.  Every reduction
// runs in a fixed order (tile partials, then a sequential combine), so gradients are reproducible.

// (1) activation backward + per-channel partial sums for the GroupNorm backward:
//   dz = g * act'(x*as + ab)   (ReLU6 / SiLU / none);   slab[b][tile][0][c] = sum dz, [1] = sum dz * x  (tiles of 64 rows)
// x is the (virtually concatenated) input of the norm.  dz may alias g; null = do not store (act none).
struct BwdMaskArgs {
  const void* g;
  const void* x0; const void* x1; int c0, c1;
  const float* as; const float* ab;
  int act;
  void* dz;
  float* slab;
  int M, C, P;
};
hipError_t launch_bwd_mask_reduce(int dtype, const BwdMaskArgs& a, hipStream_t s);

// sum a slab over its tiles: out[b][j][c] = sum_t slab[b][t][j][c] for j < nj_out (slab rows have nj entries; pre-offset
// the pointer by j0*C to pick a single component).  Fixed order.
hipError_t launch_slab_reduce(const float* slab, float* out, int B, int ntiles, int nj, int nj_out, int C, hipStream_t s);
// out[c] = sum_b in[b*stride + c]
hipError_t launch_batch_sum(const float* in, float* out, int B, int64_t stride, int C, hipStream_t s);
// bias gradient: out[0..Cstore) = column sums of g [M][C] of T (P pixels per image; C a multiple of 32, Cstore <= C) -- bwd_mask_reduce
// without activation or x, slab_reduce of its first plane, batch_sum.  Scratch: slab [M / P][bias_grad_tiles(P)][2][C], S [M / P][C].
inline int bias_grad_tiles(int P) { return (P + 63) / 64; }
hipError_t launch_bias_grad(int dtype, const void* g, int M, int C, int P, int Cstore, float* slab, float* S, float* out, hipStream_t s);

// (2) GroupNorm backward coefficients from the reduced sums S[b][2][C] and the forward mean / rstd:
//   dx = dz*A + x*Bq + Cq;  dG[b][c] = sum dz*xhat,  dBc[b][c] = sum dz  (before the FiLM / batch reductions)
struct GnBwdArgs {
  const float* S; const float* mean; const float* rstd;   // [B][2][C], [B][groups], [B][groups]
  const float* slab; int ntiles;                          // or (S null): the tile partials [B][ntiles][2][C], summed inside the kernel
  const float* gamma; const float* film; int64_t film_stride;  // FiLM rows of the forward (scale at c, shift at C+c) or null
  int C, groups, P, B;
  float* A; float* Bq; float* Cq; float* dG; float* dBc;   // [B][C] each
};
hipError_t launch_gn_bwd_coef(const GnBwdArgs& a, hipStream_t s);
//   parameter gradients: dgamma[c] = sum_b dG*(1+s), dbeta[c] = sum_b dBc*(1+s);  FiLM: ds = dG*gamma + dBc*beta, df = dBc
struct GnParamGradArgs {
  const float* dG; const float* dBc; const float* gamma; const float* beta;
  const float* film; int64_t film_stride;
  float* dgamma; float* dbeta;
  float* dfilm; int64_t dfilm_stride;   // row b: [c] <- ds, [C + c] <- df  (pre-offset to this block's rows) or null
  int B, C;
};
hipError_t launch_gn_param_grad(const GnParamGradArgs& a, hipStream_t s);
// (3) dx = dz*A + x*Bq + Cq (+ add0) (+ add1): x / dx / add1 follow the virtual-concat split, add0 is dense [M][C]
struct GnApplyArgs {
  const void* dz; const void* x0; const void* x1; int c0, c1;
  const float* A; const float* Bq; const float* Cq;
  const void* add0; const void* add1_0; const void* add1_1;
  void* dx0; void* dx1;
  int M, P;
};
hipError_t launch_gn_bwd_apply(int dtype, const GnApplyArgs& a, hipStream_t s);
// One norm site of the training backward, in the engine's order: (1) bwd_mask_reduce (skipped when the producer already wrote dz
// and the tile partials: slab_ready), the tile partials summed inside gn_bwd_coef (C / 32 <= 64) or by slab_reduce into S,
// (2) gn_bwd_coef, gn_param_grad, (3) gn_bwd_apply.  32 groups.  Scratch: slab [B][ntiles][2][C], S [B][2][C] (used only when
// C / 32 > 64), A / Bq / Cq / dG / dBc [B][C].
struct GnSiteArgs {
  const void* g; void* dz;            // incoming gradient of act(norm(x)); dz = g * act' (may alias g; null: act none, g is dz)
  const void* x0; const void* x1; int c0, c1;
  const float* as; const float* ab; int act;                    // forward record: the norm's affine, the activation
  const float* mean; const float* rstd;                         // forward record [B][32]
  const float* gamma; const float* beta;
  const float* film; int64_t film_stride; float* dfilm; int64_t dfilm_stride;
  float* dgamma; float* dbeta;
  float* slab; int ntiles; int slab_ready;
  float* S; float* A; float* Bq; float* Cq; float* dG; float* dBc;
  const void* add0; const void* add1_0; const void* add1_1;     // as GnApplyArgs
  void* dx0; void* dx1;
  int B, P;
};
hipError_t launch_gn_site_bwd(int dtype, const GnSiteArgs& a, hipStream_t s);
hipError_t launch_add_into(int dtype, void* dst, const void* src, int64_t n, hipStream_t s);   // dst += src
hipError_t launch_fill_zero(void* dst, int64_t bytes, hipStream_t s);
hipError_t launch_zero_fill(void* dst, int64_t bytes, hipStream_t s);  // kernel, not a memset node

// (4) weight gradient of a 1x1 / one tap of a 3x3 convolution (TN GEMM on MFMA, split over the rows):
//   out[n*ldn + k*ldk + off] = sum_m g[m][n] * A'[src(m)][k],   A' = act(a*as + ab) per K-segment as in GemmArgs;
//   src(m) = pixel (y*stride + dy, x*stride + dx) of the input image (zero outside), m = (b, y, x) over Ho x Wo.
struct WgradArgs {
  const void* g; int N;
  GemmSeg seg[3]; int nseg; int K;
  int B, Ho, Wo, Hi, Wi, stride, dy, dx;
  int ntap;            // 1, or 9: all taps of a 3x3 weight in one launch (dy, dx ignored; tap t lands at off + t)
  int nstore, kstore;  // only rows n < nstore / columns k < kstore are stored (0 = all): operands padded to 32 channels
  float* partial;      // [msplit][ntap][N][K] scratch
  float* out; int64_t ldn, ldk, off;
  int msplit;
};
int wgrad_msplit(int dtype, int M, int N, int K, int ntap);
int wgrad_msplit_ragged(int dtype, int M, int N, int K, int ntap);  // image sizes off the multiples of 64
int wgrad_rows(int B, int P);  // rows the weight-gradient GEMM walks: B * P, padded per image to 64-row chunks when P % 64 != 0
hipError_t launch_wgrad(int dtype, const WgradArgs& a, hipStream_t s);

// (5) depthwise 3x3 weight gradient: dw[c][tap] (reference layout [C][1][3][3]) =
//   sum_{b,y,x} (g*gs[b][c] + gb[b][c]) * relu6(h*as[b][c] + ab[b][c]) at (y+ky-1, x+kx-1)
struct DwWgradArgs {
  const void* g; const float* gs; const float* gb;     // incoming gradient and its affine
  const void* h; const float* as; const float* ab;     // forward input of the depthwise conv and its affine (+ReLU6)
  float* partial;      // [B*strips][9][C] scratch
  float* out;          // [C][9]
  int B, H, W, C;
};
int dw_wgrad_strips(int H, int W);
hipError_t launch_dw_wgrad(int dtype, const DwWgradArgs& a, hipStream_t s);

// (6) small dense pieces over the batch (SE MLP, FiLM / time-embedding Linears): fp32 activations
//   linear_dx:  dx[b][k] (=|+=) sum_r dy[b][r] * W[r][k]      (W is [R][Kc], T or fp32)
//   linear_dw:  dW[r][k] = sum_b dy[b][r] * x[b][k],  db[r] = sum_b dy[b][r]      (fp32 outputs)
//   dy rows have stride dy_stride (>= R) so that a slice of a wider table can be used in place
//   scratch (optional, linear_dx_chunks(R)*B*Kc floats): lets a long R be cut into chunks that run in parallel
int linear_dx_chunks(int R);
hipError_t launch_linear_dx(int wdtype, const float* dy, int64_t dy_stride, const void* W, float* dx, int B, int R, int Kc,
                            hipStream_t s, float* scratch = nullptr);
hipError_t launch_linear_dw(const float* dy, int64_t dy_stride, const float* x, float* dW, float* db, int B, int R, int Kc,
                            hipStream_t s);
//   SE gate: dpre2 = dgate * g*(1-g);  ReLU6 hidden: dpre1 = dr * [0 < r < 6];  SiLU: dx = dy * silu'(x)
hipError_t launch_sigmoid_bwd(const float* dgate, const float* gate, float* out, int64_t n, hipStream_t s);
hipError_t launch_relu6_bwd(const float* dy, const float* y, float* out, int64_t n, hipStream_t s);
hipError_t launch_silu_bwd(const float* dy, const float* x, float* out, int64_t n, hipStream_t s);
hipError_t launch_scale_rows(const float* x, float* out, int64_t n, float scale, hipStream_t s);
//   sinusoidal embedding rows (SinusoidalPosEmb, efficient_unet.py:68-76) for the time-MLP weight gradient
hipError_t launch_sin_embed(const int64_t* t, const float* freqs, float* emb, int rows, int dim, hipStream_t s);

// (7) dense 3x3 pieces
hipError_t launch_upsample2x(int dtype, const void* in, void* out, int B, int Hi, int Wi, int C, hipStream_t s);       // bilinear, align_corners=False
hipError_t launch_upsample2x_bwd(int dtype, const void* dout, void* din, int B, int Hi, int Wi, int C, hipStream_t s); // adjoint
hipError_t launch_dilate2x(int dtype, const void* in, void* out, int B, int Hi, int Wi, int C, hipStream_t s);          // out[2y][2x] = in[y][x], zeros elsewhere
//   output head: d(eps) fp32 NCHW [B][Cout][H][W] -> da NHWC [M][C] T (gradient of the SiLU output), and its weight gradient
struct FinalBwdArgs {
  const float* deps; const float* w;       // w: the forward kernel's repacked fp32 weights [9][C][4]
  void* da;                                 // [M][C] T
  int B, H, W, C, Cout;
};
hipError_t launch_final_bwd_data(int dtype, const FinalBwdArgs& a, hipStream_t s);
//   fp32 NCHW planes ([B][c0][P] and optionally [B][c1][P]) -> NHWC T [B*P][32], zero beyond the real channels: the
//   operand layout launch_wgrad wants (weight gradients of the output head and of the input conv)
hipError_t launch_pack_planes(int dtype, const float* x0, const float* x1, int c0, int c1, void* out, int B, int P, hipStream_t s);
//   input conv, data gradient: g = d(h0) NHWC [B][H][W][C0] T -> fp32 NCHW planes dx0 [B][c0][H][W] and dx1 [B][c1][H][W], the
//   forward's two input halves; either may be null (not both; dx1 needs c1 > 0) and then costs neither stores nor arithmetic.
//   Values are stored, one writer per element; C0 a multiple of 32, c0 + c1 <= 8, H and W multiples of 8, B <= 65535.
struct InitDgradArgs {
  const void* g; const float* w;  // w: the forward VALU kernel's fp32 table [(c0 + c1) * 9][C0]
  float* dx0; float* dx1; int c0, c1;
  int B, H, W, C0;
};
hipError_t launch_init_conv_dgrad(int dtype, const InitDgradArgs& a, hipStream_t s);

// (8) linear attention backward.  qkv / dqkv NHWC [B][N][3*inner]; kv = forward partials [nsplit][B][heads][32][33].
struct AttnBwdArgs {
  const void* qkv; const void* dout; void* dqkv;
  const float* kv; int nsplit;
  float* dkv;          // [B][heads][N/64][32][33] partials written by pass A, read by pass B
  int B, N, heads;
};
hipError_t launch_linattn_bwd_q(int dtype, const AttnBwdArgs& a, hipStream_t s);
hipError_t launch_linattn_bwd_kv(int dtype, const AttnBwdArgs& a, hipStream_t s);
// both passes: a.dkv = the tile partials [B][heads][ceil(N/64)][32][33], reduced in tile order into tot [B][heads][32][33]
hipError_t launch_linattn_bwd(int dtype, const AttnBwdArgs& a, float* tot, hipStream_t s);

// (9) optimiser step over all parameter tensors (optim.hip): gradient norm -> clip coefficient -> AdamW (+ EMA shadow)
constexpr int kOptChunk = 4096;  // elements per workgroup
struct OptTensor { float* p; float* m; float* v; float* ema; long long goff; long long n; };  // goff: element offset of the gradient in the flat buffer
struct OptChunk { int tensor; int first; };                                                    // first element of the run inside the tensor
struct OptStepArgs {
  const OptTensor* tensors; const OptChunk* chunks; int nchunks;  // device tables
  const float* gbase;                                              // flat fp32 gradients
  double* partial;                                                 // [nchunks] scratch
  float* stats;                                                    // [3]: ||g||, factor applied to g, 1 = step skipped
  double lr, beta1, beta2, eps, weight_decay;
  double max_grad_norm;  // <= 0: no clipping
  double ema_decay;      // < 0: no EMA update
  double grad_scale;     // multiplies every gradient first (1 / loss scale, 1 / world size)
  long long step;        // 1-based step count (bias correction)
  int skip_nonfinite;    // leave everything untouched when the norm is inf / NaN (GradScaler.step)
};
hipError_t launch_optimizer_step(const OptStepArgs& a, hipStream_t s);
// AMP form (loss-scaler state in device memory, torch.amp.GradScaler's semantics): a.step and a.skip_nonfinite are unused,
// the step count is *step (updates taken so far), a step is skipped exactly when some gradient is inf / NaN
struct OptAmpArgs {
  float* scale;            // device: loss scale, read for the unscale, then updated (_amp_update_scale_)
  int* growth_tracker;     // device: steps since the last backoff / growth
  int* step;               // device: AdamW step count, incremented by a taken step
  double growth_factor, backoff_factor;
  int growth_interval;
};
hipError_t launch_optimizer_step_amp(const OptStepArgs& a, const OptAmpArgs& amp, float* coef /* device [5] */, hipStream_t s);
// gradient accumulation: acc[i] = first ? weight * grad[i] : acc[i] + weight * grad[i], i < n (two fp32 roundings, no FMA);
// n == 0 launches nothing.  The caller has checked weight and that the ranges do not overlap.
hipError_t launch_grad_accumulate(float* acc, const float* grad, long long n, float weight, bool first, hipStream_t s);

// (10) consistency distillation (distill.hip): per-sample alpha-bar from a device table, fp32 [batch, per] tensors
constexpr int kDistillLossPerWG = 1024;  // elements per workgroup of the loss pass (one double partial each)
inline long long distill_loss_partials(long long n) { return (n + kDistillLossPerWG - 1) / kDistillLossPerWG; }
constexpr int kPredEpsilon = 0, kPredV = 1;  // what a network output means (LLIE_PRED_EPSILON / LLIE_PRED_V)
struct DistillArgs {
  const float* x_t; const float* x_next;     // x_next: loss only
  const float* e_a; const float* e_b;        // target: e_a = teacher eps; loss: e_a = student eps, e_b = EMA-target eps
  const int64_t* t; const int64_t* t_next;   // device int64 [batch]
  const float* acp; int table_len;           // device alphas_cumprod
  int batch; long long per;                  // elements per sample
  float* out;                                // target: x_next; loss: d(loss)/d(e_a)
  int pred;                                  // target: the teacher's type; loss: the student's and the EMA target's
};
hipError_t launch_consistency_target(const DistillArgs& a, hipStream_t s);
hipError_t launch_consistency_loss(const DistillArgs& a, double* partial, float* loss, hipStream_t s);
// ema = ema * decay + (1 - decay) * p over the tables' tensors (OptTensor.p = source, OptTensor.ema = destination)
hipError_t launch_ema_lerp(const OptTensor* tensors, const OptChunk* chunks, int nchunks, double decay, hipStream_t s);

// (10b) classifier-free guidance (guidance.hip): fp32 [batch, per] tensors; hipErrorInvalidValue before any launch for a null or
// unaligned pointer, an empty shape, a non-finite w (when w_rows is null) or a p outside [0, 1]
hipError_t launch_guide(const float* out_cond, const float* out_uncond, const float* w_rows, float w, float* out, int batch, int64_t per,
                        hipStream_t s);
hipError_t launch_guidance_pair(const float* latents, const float* cond, float* latents2, float* cond2, int batch, int64_t per, hipStream_t s);
hipError_t launch_cond_dropout(const float* in, const float* u, float p, float* out, int batch, int64_t per, hipStream_t s);
// Guidance rescale (Lin et al. 2024, section 3.4): the guided output of a row scaled towards the standard deviation of its
// conditional output.  For row b, n = per, g = o_u + w (o_c - o_u) as launch_guide rounds it:
//   S1c = sum o_c, S2c = sum o_c^2, S1g = sum g, S2g = sum g^2 in double (each value widened first, every square exact)
//   var_c = max(S2c - S1c^2 / n, 0), var_g likewise;  r32 = (float)sqrt(var_c / var_g), 1 where var_g is not > 0 or r32 not finite
//   f_b = fl(fl(phi r32) + fl(1 - phi));  out = fl(f_b g);  factor[b] = f_b (optional)
// A row is kGuideRescaleChunk-element chunks, one workgroup each; no atomics; the order of every sum depends on n alone.
// phi == 0 launches guide_kernel alone (factor = 1): launch_guide's bits.
constexpr int64_t kGuideRescaleChunk = 4096;
inline int64_t guide_rescale_chunks(int64_t per) { return per < 1 ? 0 : (per + kGuideRescaleChunk - 1) / kGuideRescaleChunk; }
// batch * 4 * chunks doubles (the per-workgroup partials) + batch floats (the factors), rounded up to 8 bytes; -1 for batch < 1,
// per < 1 or more than 2^31 - 1 workgroups in a launch
inline long long guide_rescale_scratch_bytes(int batch, int64_t per) {
  const int64_t chunks = guide_rescale_chunks(per);
  if (batch < 1 || chunks < 1 || (int64_t)batch * chunks > (int64_t)INT32_MAX || (per + 255) / 256 > (int64_t)INT32_MAX) return -1;
  return (long long)batch * chunks * 32 + (((long long)batch * 4 + 7) & ~7LL);
}
// as launch_guide, and hipErrorInvalidValue for a null or not 8-byte aligned scratch, a misaligned factor, a phi that is not finite
// or outside [0, 1], and a shape guide_rescale_scratch_bytes refuses
hipError_t launch_guide_rescale(const float* out_cond, const float* out_uncond, const float* w_rows, float w, float phi, float* out,
                                float* factor, void* scratch, int batch, int64_t per, hipStream_t s);

// (10c) the DPM-Solver++ 2M step (solver.hip): fp32 [n] tensors.  llie_dpm_coef as the kernel takes it.
struct DpmCoef { float sa, sb, kx, k0, k1; int vpred, order, is_last; };
bool dpm_coef_ok(const DpmCoef& c);  // order 1 or 2, every scalar finite
// prev may alias x; hist (the previous step's x0, read when order == 2, then overwritten with this step's) may be null only when
// order == 1 && is_last; clamped may be null.  hipErrorInvalidValue before any launch for a null or unaligned pointer, n <= 0 or a
// coefficient dpm_coef_ok refuses
hipError_t launch_dpm_step(const float* out, const float* x, float* hist, float* prev, float* clamped, int64_t n, const DpmCoef& c,
                           hipStream_t s);

// (11) full-resolution images as overlapping SH x SW tiles (tiles.hip).  The plan of one axis of length L, tile side S, overlap
// v (0 <= 2v <= S): one tile at 0 when L <= S, else n = ceil((L - S) / (S - v)) + 1 tiles at o_i = floor(i (L - S) / (n - 1)).
// The same two functions serve the host (llie_tile_count / llie_tile_origins) and the kernels, which compute origins themselves.
__host__ __device__ inline int tile_axis_count(int L, int S, int v) { return L <= S ? 1 : (L - S + (S - v) - 1) / (S - v) + 1; }
__host__ __device__ inline int tile_axis_origin(int i, int L, int S, int n) { return n <= 1 ? 0 : i * (L - S) / (n - 1); }  // n * L < 2^31 (tile_plan_ok)
inline bool tile_plan_ok(int H, int W, int SH, int SW, int vy, int vx) {
  if (H <= 0 || W <= 0 || SH <= 0 || SW <= 0 || vy < 0 || vx < 0 || 2 * vy > SH || 2 * vx > SW) return false;
  const long long ny = tile_axis_count(H, SH, vy), nx = tile_axis_count(W, SW, vx);
  return ny * H < (1ll << 31) && nx * W < (1ll << 31) && ny * nx < (1ll << 31);
}
// image size, tile sides (rows use (H, SH, vy), columns (W, SW, vx)), overlaps, chunk [first, first + count) of the row-major tiles
struct TilePlan { int H, W, SH, SW, vy, vx, first, count; };
// img u8 [H][W][3] -> tiles fp32 [count][3][SH][SW] = img / 127.5 - 1 (edge replication where the image is smaller than a tile)
hipError_t launch_tile_gather_u8(const uint8_t* img, const TilePlan& p, float* tiles, hipStream_t s);
// canvas fp32 [planes][max(H,SH)][max(W,SW)], planes = 3 k -> out fp32 [k][count][3][SH][SW]: a copy
hipError_t launch_tile_gather_f32(const float* canvas, int planes, const TilePlan& p, float* out, hipStream_t s);
// tiles fp32 [T][3][SH][SW] (every tile of the plan) -> img u8 [H][W][3]: feathered weighted mean in ascending tile order, then
// (r + 1) * 127.5 clipped and truncated; one thread per 4 output pixels, no atomics
hipError_t launch_tile_blend_u8(const float* tiles, const TilePlan& p, uint8_t* img, hipStream_t s);
// One LCM step of the latent canvas fp32 [3][max(H,SH)][max(W,SW)] the tiles of an image share: eps fp32 [T][3][SH][SW] (every tile
// of the plan) is fused per canvas pixel -- the one covering tile's value, or the blend's weighted mean in ascending tile order --
// and goes through lcm_step_kernel's arithmetic with the canvas and `noise` (same shape; may be NULL when c.is_last).  canvas_out
// may be canvas_in.  img (or NULL): u8 [H][W][3], the blend's bytes of the new canvas.  One thread per 4 canvas pixels, no atomics
hipError_t launch_tile_sync_step(const float* eps, const TilePlan& p, const float* canvas_in, const float* noise, const StepCoef& c,
                                 float* canvas_out, uint8_t* img, hipStream_t s);

// Whole frames at their own size (tiles.hip): a side L is padded to frame_pad(L), the next multiple of 8 and at least 64 -- the
// sizes llie_frame_shape_ok accepts -- by replicating the edge.
inline int frame_pad(int L) { return L < 64 ? 64 : (L + 7) / 8 * 8; }
// img u8 [H][W][3] -> out fp32 [3][Hp][Wp] = img[min(y,H-1)][min(x,W-1)] / 127.5 - 1
hipError_t launch_frame_load_u8(const uint8_t* img, int H, int W, float* out, hipStream_t s);
// in fp32 [3][Hp][Wp] -> img u8 [H][W][3]: the crop, then (x + 1) * 127.5 clipped and truncated
hipError_t launch_frame_store_u8(const float* in, int H, int W, uint8_t* img, hipStream_t s);

// (12) device-resident paired data loader (augment.hip).  Frame store: one uint8 pool of HWC RGB frames with packed rows, and a
// table int64 [N][3] = (byte offset into the pool, H, W) per frame.  Epoch plan: one AugRow per sample (== llie_aug_row); a launch
// handles rows [first, first + count) and writes sample j = row - first.
constexpr int kAugHflip = 1, kAugVflip = 2, kAugRotate = 4;
struct AugRow {
  int low_frame, high_frame;  // frame indices (aug_synth_u8 reads high_frame only: the normal-light frame)
  int y0, x0;                 // crop origin, the same in both frames
  int flags;                  // kAugHflip | kAugVflip | kAugRotate
  float ca, sa;               // cos and sin of the rotation angle, rounded once from float64 on the host
  float gamma, level;         // synthetic degradation: darkening exponent, noise standard deviation
  float scale[3];             // per-channel colour shift ((1, 1, 1) = none)
};
struct AugArgs {
  const uint8_t* pool; const int64_t* table; int N;
  const AugRow* plan; int first, count;
  int SH, SW;                 // crop height and width; every frame must be at least SH x SW
  const float* z;             // aug_synth_u8 only: standard-normal noise fp32 [count][SH][SW][3]
  float* low; float* high;    // fp32 [count][3][SH][SW] in [-1, 1]
  uint8_t* low_u8; uint8_t* high_u8;  // optional uint8 [count][SH][SW][3]: the bytes before normalisation
};
// null pointers (other than the optional two), N < 1, SH < 1, SW < 1, first < 0 or count < 0: hipErrorInvalidValue; count == 0 launches nothing
hipError_t launch_aug_pair_u8(const AugArgs& a, hipStream_t s);
hipError_t launch_aug_synth_u8(const AugArgs& a, hipStream_t s);

// (13) image quality (metrics.hip): per image {mse, psnr, ssim} of a against b, float64 arithmetic on x = (v - lo) / (hi - lo)
// (bytes: x = byte / 255).  SSIM is Wang et al. 2004 on RGB: 11-tap Gaussian window (sigma 1.5, normalised) applied along rows,
// then columns, over the (H - 10) x (W - 10) positions whose window lies inside the image; biased variances E[x^2] - mu^2;
// ssim_map = (2 mx my + C1)(2 sxy + C2) / ((mx^2 + my^2 + C1)(sx^2 + sy^2 + C2)); ssim = mean over channels and positions;
// mse = mean of (x - y)^2 over all 3 H W values; psnr = -10 log10(mse), +inf at mse == 0.
// One workgroup per tile of kMetricTileH x kMetricTileW valid positions writes partial[image][tile][2] = {sum ssim_map,
// sum (x - y)^2}; a second launch adds an image's partials in a fixed order.  No atomics: bitwise reproducible, and the same bits
// for an image alone or in a batch.
constexpr int kMetricTaps = 11, kMetricTileH = 16, kMetricTileW = 32;
constexpr double kMetricC1 = 1e-4, kMetricC2 = 9e-4;  // (0.01 L)^2, (0.03 L)^2 with L = 1
inline long long image_metrics_tiles(int H, int W) {  // per image; H, W >= kMetricTaps
  return (long long)((H - kMetricTaps + kMetricTileH) / kMetricTileH) * ((W - kMetricTaps + kMetricTileW) / kMetricTileW);
}
// a / b: fp32 NCHW [batch][3][H][W] or uint8 HWC [batch][H][W][3]; out3 [batch][3] doubles; partial: image_metrics_tiles * batch * 2
// doubles.  A null pointer, batch < 1, H or W < 11, lo == hi: hipErrorInvalidValue
hipError_t launch_image_metrics_f32(const float* a, const float* b, int batch, int H, int W, float lo, float hi, double* out3, double* partial,
                                    hipStream_t s);
hipError_t launch_image_metrics_u8(const uint8_t* a, const uint8_t* b, int batch, int H, int W, double* out3, double* partial, hipStream_t s);

// (14) the trainer's sample sheet (samples.hip): low / enhanced / normal fp32 NCHW [n][3][H][W] in the model's range -> one uint8
// HWC picture [3 (H+2) + 2][n (W+2) + 2][3], torchvision's make_grid(cat([low, enhanced, normal]), nrow=n) with padding 2 and pad
// value 0, then save_image's bytes: image (row r, column k) has its top-left pixel at (r (H+2) + 2, k (W+2) + 2), every other byte
// is 0, byte = trunc(min(max(((x + 1) / 2) * 255 + 0.5, 0), 255)) in separate fp32 operations, NaN -> 0.
constexpr int kGridPad = 2;
__host__ __device__ inline int comparison_grid_rows(int H) { return 3 * (H + kGridPad) + kGridPad; }
__host__ __device__ inline int comparison_grid_cols(int n, int W) { return n * (W + kGridPad) + kGridPad; }
inline bool comparison_grid_ok(int n, int H, int W) {  // sizes whose picture and inputs index within int / size_t arithmetic
  if (n < 1 || H < 1 || W < 1) return false;
  return 3ll * (H + kGridPad) + kGridPad < (1ll << 31) && (long long)n * (W + kGridPad) + kGridPad < (1ll << 31);
}
// a null pointer or n, H, W < 1: hipErrorInvalidValue
hipError_t launch_comparison_grid_u8(const float* low, const float* enhanced, const float* normal, int n, int H, int W, uint8_t* grid,
                                     hipStream_t s);

// (15) SSIM / L1 with a gradient (ssimloss.hip): definition (13)'s SSIM in fp32, differentiated with respect to the first image.
// With the filtered maps mx, my, xx, yy, xy at a valid position and sx = xx - mx^2, sy = yy - my^2, sxy = xy - mx my,
// A1 = 2 mx my + C1, A2 = 2 sxy + C2, B1 = mx^2 + my^2 + C1, B2 = sx + sy + C2, S = A1 A2 / (B1 B2):
//   dmx = (2 my A2 - 2 my A1) / (B1 B2) - S (2 mx / B1 - 2 mx / B2),   dxx = -S / B2,   dxy = 2 A1 / (B1 B2)
//   dSSIM/dx = [W^T(dmx) + 2 x W^T(dxx) + y W^T(dxy)] / (3 (H - 10) (W - 10)),   dSSIM/da = dSSIM/dx / (hi - lo)
// W^T is the transposed window filter: a full correlation that is zero outside the valid region and returns H x W.  The second
// moments are formed as written (xx - mx^2), not around the window mean.
// The x0 term of a training step (out = the network output [B,3,H,W], x_t the noised input, y the normal-light image,
// abar_b = alphas_cumprod[t_b], alpha = sqrt(abar), sigma = sqrt(1 - abar)):
//   x^ = p_b x_t + q_b out          epsilon prediction p = 1 / alpha, q = -sigma / alpha;  v prediction p = alpha, q = -sigma;  not clamped
//   L_x0 = (1 / B) sum_b w_b [lambda_s (1 - SSIM_b(x^, y)) + lambda_1 mean|x^_b - y_b|],   w_b = abar_b,  data range (-1, 1),
//          the L1 mean over the 3 H W values in model units
//   dL_x0/dout = (w_b / B) q_b [-lambda_s/2 dSSIM_b/dx + lambda_1 sign(x^ - y) / (3 H W)]
// A sample with abar_b == 0 contributes exactly 0 to the loss and nothing to the gradient (1 / alpha is never evaluated).
// Tiles as (13); no atomics; every sum's order depends on H and W alone.
long long ssim_grad_scratch_bytes(int batch, int H, int W);  // -1 for batch < 1 or an image below 11 x 11
// ssim_out [batch] fp32; da (or null: forward only) = upstream_b dSSIM_b/da, stored; upstream [batch] or null (= 1).
// A null pointer (other than the optional two), batch < 1, H or W < 11, lo == hi: hipErrorInvalidValue
hipError_t launch_ssim_grad_f32(const float* a, const float* b, int batch, int H, int W, float lo, float hi, const float* upstream,
                                float* ssim_out, float* da, void* scratch, hipStream_t s);
struct X0LossArgs {
  const float* out; const float* x_t; const float* normal;  // fp32 NCHW [batch][3][H][W]
  const int64_t* t; const float* acp; int table_len;        // device int64 [batch], device alphas_cumprod
  int velocity;                                             // 0 epsilon prediction, 1 v prediction
  float lambda_s, lambda_1;                                 // >= 0
  float* loss;                                              // one device fp32: the term alone
  float* d_out;                                             // accumulated into (or null: loss only)
  int batch, H, W;
};
hipError_t launch_x0_loss(const X0LossArgs& a, void* scratch, hipStream_t s);

// (16) the noise-space loss with a Min-SNR-gamma weight (snrloss.hip).  pred / target fp32 [B][n], d = pred - target:
//   l(d), l'(d):  mse d^2, 2 d;   l1 |d|, sign(d) (0 at 0);   huber (delta 1) 0.5 d^2 where |d| < 1 else |d| - 0.5, clamp(d, -1, 1)
//   abar = acp[t_b];  w_b = (abar == 0 ? 1 : min(1, (gamma (1 - abar)) / abar))  (epsilon)  or  min(abar, gamma (1 - abar))  (v)
//   m_b = (1 / n) sum_i l(d_bi)  (unweighted);   loss = (1 / B) sum_b w_b m_b;   d_pred[b][i] = l'(d_bi) c_b,
//   c_b = (w_b / (float)B) / (float)n -- fp32, one rounding per operation, no fused multiply-add.
// A timestep outside [0, table_len) never indexes the table: w_b, the sample's gradient rows and the loss are NaN.
// A sample is kSnrChunk-element chunks, one workgroup each; no atomics; the order of every sum depends on n (m_b) or B (loss) alone.
constexpr int kLossMse = 0, kLossL1 = 1, kLossHuber = 2;  // LLIE_LOSS_*
constexpr int64_t kSnrChunk = 4096;
inline int64_t snr_loss_chunks(int64_t per) { return per < 1 ? 0 : (per + kSnrChunk - 1) / kSnrChunk; }
// B doubles (the means) + B * chunks floats (the per-workgroup partials); -1 for batch < 1, per < 1 or more than 2^31 - 1 workgroups
inline long long snr_loss_scratch_bytes(int batch, int64_t per) {
  const int64_t chunks = snr_loss_chunks(per);
  if (batch < 1 || chunks < 1 || (int64_t)batch * chunks > (int64_t)INT32_MAX) return -1;
  return (long long)batch * 8 + (long long)batch * chunks * 4;
}
struct SnrLossArgs {
  const float* pred; const float* target;             // fp32 [batch][per]
  const int64_t* t; const float* acp; int table_len;  // device int64 [batch], device alphas_cumprod
  int loss_type, velocity; float gamma;               // kLoss*; 0 epsilon prediction, 1 v prediction; finite, > 0
  float* loss;                                        // one device fp32
  float* sample_loss; float* weight;                  // [batch] each, or null
  float* d_pred;                                      // stored (or null: the loss alone, the same bits)
  int batch; int64_t per;
};
// A null required pointer, batch or per < 1, table_len < 1, an unknown loss_type, gamma not finite or <= 0: hipErrorInvalidValue
hipError_t launch_snr_loss(const SnrLossArgs& a, void* scratch, hipStream_t s);

}  // namespace llie
