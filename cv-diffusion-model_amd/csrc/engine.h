// libllie_hip.so: context, state_dict repack, workspace arena and the launch sequence of the
// denoiser behind the C ABI of include/llie.h.  Host-only code; kernels live in the *.hip files.
//
// Execution model: one UNet forward is a fixed sequence of kernel launches on the caller's stream.
// All temporaries come from a caller-provided workspace through a deterministic first-fit arena, so
// the same (batch, H, W) always produces the same offsets: llie_workspace_bytes() replays the
// sequence with launches disabled to obtain the high-water mark.
//
// Internal header of the host sources: model.cpp (parameter table, topology, loading, byte / flop model), forward.cpp,
// backward.cpp, enhance.cpp (scheduler loop, hipGraph cache), kernel_api.cpp (kernel-level entry points, optimiser, EMA,
// distillation) and tune.cpp (knobs, profiler).
#pragma once
#include <hip/hip_runtime.h>

#include <algorithm>
#include <cmath>
#include <cstdarg>
#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <map>
#include <tuple>
#include <string>
#include <vector>

#include "../../include/llie.h"
#include "kernels.h"

namespace llie {

void set_err(const char* fmt, ...);  // text of llie_last_error() (model.cpp)
inline hipStream_t hs(llie_stream stream) { return reinterpret_cast<hipStream_t>(stream); }

inline size_t elem_size(int dt) { return dt == LLIE_F32 ? 4 : 2; }
inline size_t align_up(size_t x, size_t a) { return (x + a - 1) / a * a; }

// ---------------------------------------------------------------------------------------------
// Parameter table (PKind and the layouts behind it: kernels.h, LoadDesc; model.cpp: make_desc turns a Param into one)
struct Param {
  std::string key;
  int64_t numel = 0;
  PKind kind = PK_F32;
  size_t off = 0;                      // byte offset of the destination in the weight blob
  int rows = 0, cols = 0, ld = 0, col0 = 0;  // PK_MAT: [rows][cols] -> dst[r*ld + col0 + c]
  int O = 0, I = 0;
  int Op = 0, Ip = 0;                  // padded destination dims of conv / depthwise layouts (0 = O / I)
  bool as_t = true;                    // PK_MAT: store as compute dtype (true) or fp32
  bool loaded = false;
  int ndim = 1;
  int64_t shape[4] = {0, 0, 0, 0};     // shape in the reference's state_dict
  // training: second copy in the layout the input-gradient kernels read (PK_MAT: transposed [cols][rows];
  // PK_DW: taps flipped; PK_CONV3: [8-tap][I][O]); 0 = none.  goff = offset (floats) in the flat gradient buffer.
  bool has_t = false;
  size_t t_off = 0;
  int64_t goff = 0;
  // PK_MAT, 2-byte engines: third copy = the matrix times f_scale in MFMA fragment order (kernels.h: pw_expand_pack_index)
  bool has_f = false;
  size_t f_off = 0;
  float f_scale = 1.f;
  // PK_CONV3 of an up-sampling conv, 2-byte engines: third copy = the 64 folded sets of conv3x3_upfold_kernel (small.hip: launch_upconv_fold)
  bool has_fold = false;
  size_t fold_off = 0;
  // PK_MAT, expand weight of a block the wide Gram rule can select: fp64 M_g / u_g per GroupNorm group (kernels.h: launch_gram_group_weights)
  bool has_mg = false;
  size_t mg_off = 0;
};

// cin / cout / hid are the PHYSICAL channel counts of the tensors (multiples of 32; hid of 64 for 2-byte types);
// *_r the reference's.  They differ only for the unpinned variants (tiny / base), whose odd channel counts are
// zero-padded at the end of each tensor: zero weights and a zero norm affine keep the padding at exactly zero.
struct IrbW {
  int cin, cout, hid, sq;
  int cin_r, cout_r, hid_r;
  bool skip;
  size_t n1g, n1b, n2g, n2b, w_expand, w_dw, se_w1, se_b1, se_w2, se_b2, w_proj;
  int film_off;  // first row of this block inside the concatenated FiLM projection
  size_t w_expand_t, w_proj_t, w_dw_flip;  // training copies: [cin][hid], [hid (+cin)][cout], flipped taps
  bool has_wf = false;  // expand weights x 6 in MFMA fragment order for the activation-stationary kernel (pwx.hip)
  size_t w_expand_f = 0;
  bool has_mg = false;  // norm2's group matrices M_g / u_g of the wide Gram form (gram.hip), fp64
  size_t w_mg = 0;
  // index of each parameter in llie_ctx::params, recorded where the builder registers it (the backward pass writes the
  // parameter's gradient through it); i_film_*: this block's time_mlp.1; i_skip = -1 without a skip conv
  int i_n1g, i_n1b, i_n2g, i_n2b, i_expand, i_dw, i_se_w1, i_se_b1, i_se_w2, i_se_b2, i_proj, i_film_w, i_film_b, i_skip;
};
struct AttnW {
  int c, heads, inner;
  bool soft;  // StandardAttention (softmax; no second norm: n2g / n2b unused, i_n2g = i_n2b = -1), else LinearAttention
  size_t ng, nb, w_qkv, w_out, n2g, n2b;
  size_t w_qkv_t, w_out_t;
  int i_ng, i_nb, i_qkv, i_out, i_n2g, i_n2b;  // parameter indices, as in IrbW
};
struct ConvW {
  int c, c_r;
  size_t w, bias;
  size_t w_t;
  int i_w, i_bias;  // parameter indices, as in IrbW
  bool has_fold = false;  // up-sampling convs of the 2-byte engines: bilinear x2 folded into per-phase weights (kernels.h)
  size_t w_fold = 0;
};
struct Block {
  int kind;  // 0 irb, 1 attn
  int idx;
};

// ---------------------------------------------------------------------------------------------
// Deterministic first-fit arena over the caller's workspace.
struct Arena {
  struct Blk { size_t off, size; };
  std::vector<Blk> freelist;   // sorted by offset, coalesced
  std::map<size_t, size_t> live;  // off -> size
  size_t cap = 0, high = 0;
  bool failed = false;
  static constexpr size_t kUnbounded = (size_t)1 << 46;  // capacity of a planning (dry) run: `high` is then the plan's size
  explicit Arena(size_t capacity = kUnbounded) : cap(capacity) { freelist.push_back({0, capacity}); }
  size_t alloc(size_t bytes) {
    bytes = align_up(bytes ? bytes : 1, 256);
    for (size_t i = 0; i < freelist.size(); ++i) {
      if (freelist[i].size >= bytes) {
        const size_t off = freelist[i].off;
        freelist[i].off += bytes;
        freelist[i].size -= bytes;
        if (!freelist[i].size) freelist.erase(freelist.begin() + i);
        live[off] = bytes;
        if (off + bytes > high) high = off + bytes;
        return off;
      }
    }
    failed = true;
    return 0;
  }
  void free(size_t off) {
    auto it = live.find(off);
    if (it == live.end()) return;
    Blk b{off, it->second};
    live.erase(it);
    size_t i = 0;
    while (i < freelist.size() && freelist[i].off < b.off) ++i;
    freelist.insert(freelist.begin() + i, b);
    if (i + 1 < freelist.size() && freelist[i].off + freelist[i].size == freelist[i + 1].off) {
      freelist[i].size += freelist[i + 1].size;
      freelist.erase(freelist.begin() + i + 1);
    }
    if (i > 0 && freelist[i - 1].off + freelist[i - 1].size == freelist[i].off) {
      freelist[i - 1].size += freelist[i].size;
      freelist.erase(freelist.begin() + i);
    }
  }
};

// NHWC activation living in the workspace, with the stats slab its producer wrote.
struct Tens {
  size_t off = 0, slab = 0;
  int C = 0, H = 0, W = 0, ntiles = 0;
  bool valid = false;
  int Cr = 0;  // real channels (<= C; the rest is zero padding)
};

// GroupNorm(min(32, C), C) of the reference; for channel counts it cannot construct (tiny / base: 48, 144 ...) the
// documented deviation: the largest divisor of C that is <= 32.  Identical whenever C is a multiple of 32 or C < 32 | 32.
inline int gn_groups(int c) {
  for (int g = std::min(32, c); g >= 1; --g)
    if (c % g == 0) return g;
  return 1;
}
inline int pad32(int c) { return (c + 31) / 32 * 32; }

// ---------------------------------------------------------------------------------------------
// Training tape: what the forward pass leaves in the workspace for the backward pass (offsets).
struct GnRec { size_t as = 0, ab = 0, mean = 0, rstd = 0; };
struct IrbRec { int w; Tens x0, x1; bool cat; GnRec n1, n2; Tens h1; size_t h2, gate, sehid, semean; Tens y; };
// linear form: kv / nsplit, tmp (to_out's result before the second norm) and n2; softmax form: lse instead
struct AttnRec { int w; Tens x; GnRec n1, n2; size_t qkv, kv, ao, lse; int nsplit; Tens tmp, y; };
struct ConvRec { int w; bool up; Tens x, u, y; };
struct TapeOp { int kind, idx; };  // kind: 0 irb, 1 attn, 2 conv; idx into the vectors below
struct Tape {
  std::vector<IrbRec> irbs;
  std::vector<AttnRec> attns;
  std::vector<ConvRec> convs;
  std::vector<TapeOp> ops;  // forward order
  // UNet level
  size_t temb = 0, stemb = 0, film = 0;
  Tens h0, hlast;
  Tens x1;  // bare IRB with a virtual-concat input: the second input segment (h0 is the first)
  GnRec fin;
  const float* lat = nullptr; const float* cond = nullptr; const int64_t* t = nullptr;
  int B = 0;
  int H = 0, W = 0;  // the frame of a UNet training forward: the backward pass takes its shape from here (0 for a single operator)
  const void* ws = nullptr;
  bool valid = false;
  void clear() { irbs.clear(); attns.clear(); convs.clear(); ops.clear(); valid = false; }
};

constexpr int kMaxBranches = 8;

}  // namespace llie

struct llie_ctx {
  llie_config cfg{};
  int dt = 0;
  std::vector<llie::Param> params;
  std::map<std::string, int> index;
  size_t blob_bytes = 0;
  char* blob = nullptr;
  // topology
  std::vector<llie::IrbW> irbs;
  std::vector<llie::AttnW> attns;
  std::vector<llie::ConvW> downs, ups;
  std::vector<std::vector<llie::Block>> enc, dec;
  std::vector<llie::Block> mid;
  std::vector<int> channels;    // physical (padded) channels per level
  std::vector<int> channels_r;  // the reference's
  bool padded = false;          // some tensor carries zero padding (unpinned variant): inference only
  // UNet-level tensors
  size_t t_w1 = 0, t_b1 = 0, t_w3 = 0, t_b3 = 0, freqs = 0, film_w = 0, film_b = 0;
  // their parameter indices (UNet only), recorded by the builder like IrbW's
  int i_t_w1 = -1, i_t_b1 = -1, i_t_w3 = -1, i_t_b3 = -1, i_init_w = -1, i_init_b = -1, i_fin_g = -1, i_fin_b = -1, i_fin_w = -1, i_fin_bias = -1;
  int film_rows = 0;
  int64_t grad_numel = 0;
  // batched reload (llie_load_all): device descriptor table + the host pointers it was built for
  llie::LoadDesc* load_descs = nullptr;
  std::vector<const float*> load_srcs;
  unsigned long long* hash_partial = nullptr;  // [n][32] partial content hashes (llie_refresh_params)
  unsigned long long* hash_state = nullptr;    // [0] hash of the last load, [1] "changed" flag read by load_all_kernel
  llie::Tape tape;           // last training forward (llie_unet_train_forward), read by llie_unet_backward
  llie::Arena* train_arena = nullptr;  // arena state after that forward; the backward pass continues in it
  size_t init_wp = 0, fin_wp = 0;  // MFMA-packed init / final conv weights (2-byte compute dtypes)
  size_t init_w = 0, init_b = 0, fin_g = 0, fin_b = 0, fin_w = 0, fin_bias = 0;
  // hipGraph cache of llie_enhance launch sequences (key -> executable graph)
  // bounded: least-recently-used entries beyond kMaxGraphs are destroyed (a server sweeping batch sizes or schedules would
  // otherwise grow it without limit; an evicted key is simply captured again on its second next use)
  struct GraphEntry { bool seen = false; hipGraphExec_t exec = nullptr; hipGraph_t graph = nullptr; uint64_t used = 0; };
  static constexpr size_t kMaxGraphs = 16;
  uint64_t graph_clock = 0;
  std::map<std::string, GraphEntry> graphs;
  std::map<std::tuple<int, int, int, int>, size_t> zneed;  // (batch, height, width, knob epoch) -> bytes of zero-initialised totals one forward takes (Run::zbegin)
  std::map<std::tuple<int, int, int, int>, size_t> qplan;  // same key -> the forward's plan with per-sample timesteps, which every workspace query of a UNet handle is built on (forward.cpp: query_plan)
  hipStream_t cap_stream = nullptr;  // side stream used only to record captures (the legacy null stream cannot capture)
  // backward pass: weight-gradient kernels run on this stream next to the activation-gradient chain (Back::fork/join)
  hipStream_t side_stream = nullptr;
  hipEvent_t ev_fork = nullptr, ev_join = nullptr;
  // concurrent branches of the captured enhance graph (branch 0 is cap_stream)
  hipStream_t branch_stream[llie::kMaxBranches] = {};
  hipEvent_t branch_join[llie::kMaxBranches] = {};
  // per-kernel-class HIP-event profiling (llie_profile_begin / llie_profile_end)
  int prof_mask = 0;
  struct ProfRec { int cls; int64_t bytes; hipEvent_t e0, e1; const char* name; char tag[56]; };
  std::vector<ProfRec> prof;
  std::vector<hipEvent_t> event_pool;
  hipEvent_t get_event() {
    if (!event_pool.empty()) { hipEvent_t e = event_pool.back(); event_pool.pop_back(); return e; }
    hipEvent_t e = nullptr;
    if (hipEventCreate(&e) != hipSuccess) return nullptr;
    return e;
  }
};

namespace llie {

// ---------------------------------------------------------------------------------------------
// (the tuning knobs the rules below read: kernels.h, Knobs)
constexpr int kGraphMaxSteps = 20;  // default of Knobs::graph_max_steps: capture pays at 20 steps and loses at 50

// The launch sequence of an inverted-residual block (forward.cpp: Run::irb; the byte model, llie_path_bytes, asks too):
//   unfused    expand GEMM, dwconv3x3, SE, project GEMM: fp32 engines, training, wide or padded blocks
//   recompute  2-byte inference, narrow inputs: a statistics-only expand pass, then expand_dw rebuilds h1 on the fly (irbx.hip)
//   project    identity-residual recompute blocks and the 96 -> 32 skip-conv block go without h2 too: the SE pool totals come from a
//              pass that only rebuilds h1 (expand_pool); given the gate, expand_dw_project applies Wp itself and adds the shortcut
//   wide       the 192 -> 64 and 384 -> 128 decoder blocks (2-byte inference): unfused up to norm2 -- h1 is stored, recomputing it is
//              too dear -- then the SE pool totals from one read of h1 (dwconv3x3_pool) and, given the gate, depthwise + project +
//              skip conv in one kernel (dwconv3x3_project): h2 is never allocated
enum IrbForm { kIrbUnfused, kIrbRecompute, kIrbProject, kIrbWide };
struct IrbPath {
  IrbForm form;
  // 2-byte inference engines carry norm1's ReLU6 as clamp01(z / 6): the tables come out divided by 6 and the expand GEMM (or the
  // recompute kernels) puts the 6 back (kernels.h: ACT_RELU6_S6); the unfused depthwise treats norm2's alike (DwArgs::s6), the
  // recompute kernels take norm2's plain tables (their accumulators are already / 6).  Training keeps the plain tables.
  bool s6;
  // SE pool: inference adds fixed-point channel totals into the zeroed region (one gate kernel follows); training keeps the
  // slab of tile partials (the backward pass and the 3-launch SE path read it)
  bool fixtot;
  // recompute forms: norm2's statistics from the Gram matrix of the activated input (gram.hip) -- the statistics pass is then a
  // plain read of x -- or, knob "gram" = 0, from a second run of the expand GEMM (expand_stats).  From 32 768 pixels per image
  // on: below, the workgroup epilogue and the last-ticket sum outweigh the saved MFMAs (measured at B = 1 and B = 32; the rule
  // must not depend on the batch, it fixes the statistics' summation order)
  bool gram;
  // wide form, the layer gram_wide_supported names (192 -> 64 at hid 768; knob "wide_gram"): gn(norm1), the wide Gram and its group
  // finalize give norm2's tables before the expand GEMM, pw_expand_act stores the activated h1 and adds the pool totals,
  // dwconv3x3_project reads it pre-activated.  No statistics slab of h1, no second gn launch, no dwconv3x3_pool.  The 384 -> 128
  // block keeps the pool pass: its Gram (78 blocks) was not built.  From kWideGramMinPixels pixels per image on (knob 2: at every
  // size): the form trades two launches (norm2's gn, the pool pass) for three (Gram, its partial sum, the group finalize), and on a
  // small map every launch of the block is latency; only the 128 x 128 map of a 256 x 256 frame has been measured.
  bool wgram;
};
constexpr int kWideGramMinPixels = 4096;
// c0 = channels of the block's first input segment (= w.cin without a virtual concat).  A rule on the layer, the image size, the
// dtype and the knobs alone -- never on the batch or the grid, which would break batch invariance.
inline IrbPath irb_path(int dt, const IrbW& w, int c0, int H, int W, bool training) {
  IrbPath p{kIrbUnfused, !training && dt != LLIE_F32, !training && w.hid % 128 == 0, false, false};
  if (p.fixtot && p.s6 && g_knobs.wide_project &&
      wide_project_supported(dt, w.cin, c0, w.hid, w.cout, w.skip, w.hid != w.hid_r || w.cin != w.cin_r || w.cout != w.cout_r, H, W)) {
    p.form = kIrbWide;
    // (the activating expand is pw_expand's: knob "pwx" on, input segments of whole 64-channel chunks)
    p.wgram = g_knobs.wide_gram && (H * W >= kWideGramMinPixels || g_knobs.wide_gram > 1) && w.has_mg && g_knobs.pwx && c0 % 64 == 0 &&
              (w.cin - c0) % 64 == 0 && gram_wide_supported(dt, w.cin, c0, w.hid, H * W);
    return p;
  }
  // (!fixtot: the recompute kernels only know the fixed-point totals; every hid irbx_supported accepts is a multiple of 128)
  if (!p.fixtot || !g_knobs.use_irbx || w.hid != w.hid_r || w.cin != w.cin_r || !irbx_supported(dt, w.cin, c0, w.hid, H, W)) return p;
  p.gram = g_knobs.gram && (H * W >= 32768 || g_knobs.gram > 1) && gram_supported(dt, w.cin, c0, H * W);
  const int tail = g_knobs.irbx_project && w.cout == w.cout_r ? irbx_project_supported(dt, w.cin, c0, w.hid, w.cout, w.skip, H, W) : 0;
  // knob "irbx_project" = 2 keeps the identity-residual shapes only
  p.form = tail && !(tail == kIrbxProjectSkip && g_knobs.irbx_project == 2) ? kIrbProject : kIrbRecompute;
  return p;
}

// The up-sampling conv of an inference forward (forward.cpp: Run::conv3) runs from the folded weights (conv3x3_upfold_kernel: no
// bilinear blend in the kernel) on 2-byte engines, for maps of whole 8 x 16 low-resolution tiles, at C = 64 and C = 128: the
// channel counts measured faster than conv3x3_kernel's mode 1 in every pair (profiles/r10; C = 256 at 32 x 32 was 5 % slower --
// there a quarter more k-steps go to the border corrections -- and keeps the blending kernel).  So do the fp32 engine, ragged
// maps, the training forward (it keeps the up-sampled tensor) and llie_conv3x3.  A rule on the layer, the map and the knobs
// alone, never on the batch.
inline bool upconv_fold_supported(int dt, int Hi, int Wi, int C) {
  return g_knobs.upconv_fold && (C == 64 || C == 128) && conv3x3_upfold_ok(dt, Hi, Wi, C);
}
// Asked before it: the same conv from nine low-resolution tap maps blended on chip (conv3x3_upmaps_kernel: a quarter of the
// multiply-adds, plain weights), under the same conditions, at the channel counts where it measured faster than what it
// replaces in every pair (profiles/r24).  C = 64 stays with the folded weights: there the blend alone costs what that kernel
// takes in all.
inline bool upconv_maps_supported(int dt, int Hi, int Wi, int C) {
  return g_knobs.upconv_maps && (C == 128 || C == 256) && conv3x3_upmaps_ok(dt, Hi, Wi, C);
}

// ---------------------------------------------------------------------------------------------
// What the forward (forward.cpp: Run) and the backward pass (backward.cpp: Back) share: context, arena, stream, workspace.
// In a dry run nothing is launched and nothing dereferenced; only the arena is exercised.
struct Exec {
  llie_ctx* c;
  Arena* ar;
  hipStream_t s;
  char* ws;
  bool dry;
  int B;
  int dt;
  hipError_t err = hipSuccess;
  static Exec planning(llie_ctx* c, Arena* ar, int B) { return Exec{c, ar, nullptr, nullptr, true, B, c->dt}; }
  static Exec live(llie_ctx* c, Arena* ar, llie_stream stream, void* ws, int B) {
    return Exec{c, ar, hs(stream), reinterpret_cast<char*>(ws), false, B, c->dt};
  }
  template <typename T = void> T* wptr(size_t off) const { return reinterpret_cast<T*>(c->blob + off); }
  // null in a dry run (there is no workspace).  Callers may add an offset to that null while planning, since a dry run never
  // dereferences or launches, but nothing may compare the value or let it decide an allocation
  template <typename T = void> T* p(size_t off) const {
    if (dry) return nullptr;
    return reinterpret_cast<T*>(ws + off);
  }
  void chk(hipError_t e) { if (e != hipSuccess && err == hipSuccess) err = e; }
  size_t es() const { return elem_size(dt); }
  // film[rows][F] = wf[F][T] silu_temb[rows][T] + bf (small.hip: film_kernel); wf / bf in the weight blob, the rest in the workspace
  FilmArgs film_args(size_t silu_temb, int rows, int T, size_t wf, size_t bf, size_t film, int F) const {
    FilmArgs fa{};
    fa.silu_temb = p<float>(silu_temb); fa.rows = rows; fa.T = T; fa.wf = wptr<float>(wf); fa.bf = wptr<float>(bf);
    fa.film = p<float>(film); fa.F = F;
    return fa;
  }
  // return code of a finished pass, with the text of llie_last_error(); backward: the backward pass's wording
  int rc(bool backward = false) const;  // model.cpp
};

// ---------------------------------------------------------------------------------------------
// Functions that cross files
int check_loaded(const llie_ctx* c);          // model.cpp
int check_ready(const llie_ctx* c);           // model.cpp: a device and every parameter loaded
int shape_ok(const llie_ctx* c, int H, int W);  // model.cpp
// capacity check before the first launch, so that no kernel ever sees an offset past the workspace
int fits(size_t need, int64_t ws_bytes);  // model.cpp
// forward.cpp: the forward pass of `x`; tape != null: training forward -- nothing is released, every operator is recorded
int run_unet(Exec x, Tape* tape, const float* lat, const float* cond, const int64_t* t, float* eps, int H, int W);
int run_module(Exec x, Tape* tape, const float* in, const float* temb, float* y, int H, int W);
// scheduler step fused into the final conv's epilogue (2-byte compute dtypes only)
struct FusedStep { StepCoef coef; const float* noise; float* prev; float* clamped; };
// llie_step_coef as the kernels take it; a sampler other than 0 / 1, or DDIM together with clamp_x0, is not a step (LLIE_ERR_ARG)
inline StepCoef step_coef(const llie_step_coef& k) {
  return StepCoef{k.sqrt_alpha_t, k.sqrt_beta_t, k.sqrt_alpha_prev, k.sqrt_beta_prev, k.is_last, k.v_prediction, k.clamp_x0, k.sampler};
}
inline bool step_coef_ok(const llie_step_coef& k) { return k.sampler == 0 || (k.sampler == 1 && !k.clamp_x0); }
// llie_dpm_coef as solver.hip takes it (dpm_coef_ok: an order other than 1 / 2 or a non-finite scalar is not a step)
inline DpmCoef dpm_coef(const llie_dpm_coef& k) {
  return DpmCoef{k.sqrt_alpha_t, k.sqrt_beta_t, k.k_x, k.k_0, k.k_1, k.v_prediction, k.order, k.is_last};
}
// `reserve`: bytes the caller's workspace query counts beyond the forward's plan, added to the plan in the capacity check.  The
// loop keeps its images in front of the slice it passes and gives 0; the public forward gives loop_image_bytes, so that it refuses
// exactly what is smaller than llie_workspace_bytes / llie_frame_workspace_bytes answered
int unet_forward_impl(llie_ctx* c, const float* lat, const float* cond, const int64_t* t, int uniform_t, float* eps,
                      const FusedStep* fs, int batch, int H, int W, void* ws, int64_t ws_bytes, llie_stream stream, size_t reserve = 0);
// the latents ping-pong and eps images of the loop, which every workspace query of a UNet handle counts in front of the plan
inline size_t loop_image_bytes(int batch, int H, int W) { return 3 * align_up((size_t)batch * 3 * H * W * 4, 256); }
// forward.cpp: the frame rule of llie_frame_shape_ok, and the workspace of `max_steps` steps of the loop at H x W without that
// check (0: plain launches, no staging area) -- the entry points at image_size go through it unchecked, as they always did
int frame_shape_ok(const llie_ctx* c, int batch, int H, int W);
int widest_full_res_channels(const llie_ctx* c);  // what the element cap of frame_shape_ok multiplies
int64_t frame_workspace(llie_ctx* c, int batch, int H, int W, int max_steps);
// HIP status of a kernel-level entry point -> return code and llie_last_error() text.  hipErrorInvalidValue is how a launcher
// refuses its arguments: `refuse_rc` with "<what>: <refuse_msg>" (no text when refuse_msg is null)
int kerr(const char* what, hipError_t e, int refuse_rc = LLIE_ERR_SHAPE, const char* refuse_msg = "shape outside the kernel contract");

}  // namespace llie
