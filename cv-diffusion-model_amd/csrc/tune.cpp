// Tuning knobs, the kernels' cycle-stamp readers and the per-launch HIP-event profiler.
#include "engine.h"

using namespace llie;

// The engine's own knobs, with the defaults and the environment variables that are read once, when the library is loaded
// (no other file's initialiser depends on this one).  llie_tune below sets them; the other names of its table go to
// the kernels' launchers (kernels.h).
static Knobs knob_defaults() {
  Knobs k{};
  // Recompute form (irbx.hip: statistics-only expand + tile-fused expand/depthwise): default for the
  // inference path of 2-byte engines wherever irbx_supported(); llie_tune("irbx", 0) restores the unfused pair.
  k.use_irbx = getenv("LLIE_NO_IRBX") ? 0 : 1;
  // Recompute blocks irbx_project_supported names: the SE pool from a pass that only rebuilds h1 (expand_pool), the project GEMM
  // as expand_dw's tail (expand_dw_project) -- h2 never reaches HBM either; llie_tune("irbx_project", 0) restores expand_dw +
  // pw_gemm, 2 keeps only the identity-residual shapes (A/B of the 96 -> 32 skip-conv block alone).
  k.irbx_project = 1;
  // The two wide decoder blocks wide_project_supported names keep the expand GEMM and its stored h1, but go without h2: the SE
  // pool from one read of h1 (dwconv3x3_pool), then depthwise + gate + project + skip conv in one kernel (dwconv3x3_project);
  // llie_tune("wide_project", 0) restores dwconv3x3 + pw_gemm.
  k.wide_project = 1;
  // Of those, the 192 -> 64 block knows norm2's tables before its expand GEMM runs (the Gram of the activated input, gram.hip):
  // pw_expand stores the activated h1 and adds the pool totals itself, the pool pass goes.  llie_tune("wide_gram", 0) restores it,
  // 2 takes the form at every map size (1: from 4096 pixels per image).
  k.wide_gram = 1;
  k.gram = 1;  // norm2 statistics of the recompute form from the Gram matrix of the block input (gram.hip); 0 = expand_stats
  // Cache policy of the big activation tensors (inference): a tensor of at least nt_min_mb MiB (this run's batch) is stored
  // non-temporally by its producer (common.h: st_vec_pol).  nt_mask picks the producers: 1 expand_dw (h2), 2 pw_expand (h1),
  // 4 dwconv3x3 (h2), 8 project / attention GEMM outputs, 16 dense 3x3 conv outputs.  Values never change, only where lines live.
  k.nt_min_mb = 100; k.nt_mask = 1;
  // Up-sampling convs from folded weights (conv.hip: conv3x3_upfold_kernel) wherever upconv_fold_supported();
  // llie_tune("upconv_fold", 0) restores conv3x3_kernel's mode 1, which blends the patch itself.
  k.upconv_fold = 1;
  k.se_mfma = 1;  // SE MLP of the wide blocks as two MFMA launches (small.hip: se_fc1_mfma / se_fc2_mfma); 0 = the row-parallel pair
  // Backward pass: run the weight-gradient kernels on a side stream next to the activation-gradient chain
  // (llie_tune("bwd_async", 0) puts everything back on the caller's stream).
  k.bwd_async = 1;
  // hipGraph path of llie_enhance: batches of 16 and more are captured as two concurrent half-batch branches (no operator
  // mixes samples and every kernel is bitwise batch-invariant, so the bits do not change): the launch-bound tail of one
  // half (norm finalisation, SE MLP) overlaps the streaming kernels of the other, +4 % at B = 32.  Overlapping kernels
  // stretch each other, so per-kernel durations are only meaningful from a single chain: llie_profile_* already forces
  // the eager single chain, and LLIE_ENHANCE_SPLIT=0 (or llie_tune("enhance_split", 0)) gives rocprofv3 the same.
  k.enhance_split = getenv("LLIE_ENHANCE_SPLIT") ? atoi(getenv("LLIE_ENHANCE_SPLIT")) : 2;
  // Loops longer than this are not captured (llie_tune("graph_max_steps", n); n <= 0 restores the default): DESIGN.md 7 has the
  // measurement behind the number.
  k.graph_max_steps = kGraphMaxSteps;
  // Captured graphs bake in the kernel choices of the moment: every llie_tune call starts a new epoch of the graph cache.
  k.epoch = 0;
  return k;
}
Knobs llie::g_knobs = knob_defaults();

// one profiled launch's duration, once it has finished
static hipError_t elapsed_ms(const llie_ctx::ProfRec& r, float* ms) {
  hipError_t e = hipEventSynchronize(r.e1);
  if (e == hipSuccess) e = hipEventElapsedTime(ms, r.e0, r.e1);
  if (e != hipSuccess) set_err("profile: %s", hipGetErrorString(e));
  return e;
}

// diagnostics: mean per-wave cycles of the last stamped launch of one kernel family (llie_tune("*_stamp", 1)); synchronises
static int read_stamps(double* out, hipError_t (*fetch)(double*)) {
  if (!out) return LLIE_ERR_ARG;
  hipError_t e = hipDeviceSynchronize();
  if (e == hipSuccess) e = fetch(out);
  return e == hipSuccess ? LLIE_OK : LLIE_ERR_ARG;
}

extern "C" {

int llie_tune(const char* knob, int value) {
  if (!knob) return LLIE_ERR_ARG;
  ++g_knobs.epoch;
  if (!strcmp(knob, "gemm_bk")) { pw_gemm_force_bk(value); return LLIE_OK; }
  if (!strcmp(knob, "se_mfma")) { g_knobs.se_mfma = value; return LLIE_OK; }
  if (!strcmp(knob, "nt_min_mb")) { g_knobs.nt_min_mb = value; return LLIE_OK; }
  if (!strcmp(knob, "nt_mask")) { g_knobs.nt_mask = value; return LLIE_OK; }
  if (!strcmp(knob, "upconv_fold")) { g_knobs.upconv_fold = value != 0; return LLIE_OK; }
  if (!strcmp(knob, "gram")) { g_knobs.gram = value; return LLIE_OK; }
  if (!strcmp(knob, "irbx")) { g_knobs.use_irbx = value != 0; return LLIE_OK; }
  if (!strcmp(knob, "irbx_project")) { g_knobs.irbx_project = value < 0 || value > 2 ? 1 : value; return LLIE_OK; }
  if (!strcmp(knob, "wide_project")) { g_knobs.wide_project = value != 0; return LLIE_OK; }
  if (!strcmp(knob, "wide_gram")) { g_knobs.wide_gram = value < 0 || value > 2 ? 1 : value; return LLIE_OK; }
  if (!strcmp(knob, "irbx_dbuf")) { irbx_tune(value); return LLIE_OK; }
  if (!strcmp(knob, "irbx_stamp")) { irbx_stamp(value); return LLIE_OK; }
  if (!strcmp(knob, "irbx_grid")) { irbx_grid(0, value); return LLIE_OK; }
  if (!strcmp(knob, "irbx_grid2")) { irbx_grid(2, value); return LLIE_OK; }
  if (!strcmp(knob, "irbx_grid4")) { irbx_grid(4, value); return LLIE_OK; }
  if (!strcmp(knob, "irbx_grid6")) { irbx_grid(6, value); return LLIE_OK; }
  if (!strcmp(knob, "conv_stamp")) { conv3x3_stamp(value); return LLIE_OK; }
  if (!strcmp(knob, "gemm_stamp")) { pw_gemm_stamp(value); return LLIE_OK; }
  if (!strcmp(knob, "pwx")) { pw_expand_enable(value); return LLIE_OK; }
  if (!strcmp(knob, "pwx_stamp")) { pw_expand_debug(value); return LLIE_OK; }
  if (!strcmp(knob, "bwd_async")) { g_knobs.bwd_async = value; return LLIE_OK; }
  if (!strcmp(knob, "enhance_split")) { g_knobs.enhance_split = value; return LLIE_OK; }
  if (!strcmp(knob, "graph_max_steps")) { g_knobs.graph_max_steps = value > 0 ? value : kGraphMaxSteps; return LLIE_OK; }
  return LLIE_ERR_ARG;
}

int llie_debug_gemm_stamps(double* out3) { return read_stamps(out3, pw_gemm_stamp_fetch); }
int llie_debug_pwx_stamps(double* out4) { return read_stamps(out4, pw_expand_stamp_fetch); }
int llie_debug_conv_stamps(double* out8) { return read_stamps(out8, conv3x3_stamp_fetch); }   // the up-sampling conv
int llie_debug_irbx_stamps(double* out10) { return read_stamps(out10, irbx_stamp_fetch); }  // expand_dw

int llie_profile_begin(llie_ctx* c, int class_mask) {
  if (!c) return LLIE_ERR_ARG;
  for (auto& r : c->prof) { c->event_pool.push_back(r.e0); c->event_pool.push_back(r.e1); }
  c->prof.clear();
  c->prof_mask = class_mask;
  return LLIE_OK;
}

int llie_profile_end(llie_ctx* c, int kernel_class, double* total_ms, int64_t* launches, int64_t* alg_bytes) {
  if (!c) return LLIE_ERR_ARG;
  c->prof_mask = 0;
  double ms = 0.0;
  int64_t n = 0, bytes = 0;
  for (auto& r : c->prof) {
    if (!(r.cls & kernel_class)) continue;
    float t = 0.f;
    if (hipError_t e = elapsed_ms(r, &t)) return (int)e;
    ms += t; ++n; bytes += r.bytes;
  }
  if (total_ms) *total_ms = ms;
  if (launches) *launches = n;
  if (alg_bytes) *alg_bytes = bytes;
  return LLIE_OK;
}

int llie_profile_report(llie_ctx* c, char* buf, size_t cap) {
  if (!c || !buf || cap < 2) return LLIE_ERR_ARG;
  c->prof_mask = 0;
  struct Agg { double ms = 0; int64_t n = 0, bytes = 0; };
  std::map<std::string, Agg> agg;
  for (auto& r : c->prof) {
    float t = 0.f;
    if (hipError_t e = elapsed_ms(r, &t)) return (int)e;
    Agg& a = agg[r.name ? r.name : "?"];
    a.ms += t; a.n += 1; a.bytes += r.bytes;
  }
  std::string out;
  char line[512];
  for (auto& kv : agg) {
    snprintf(line, sizeof line, "%s\t%.6f\t%lld\t%lld\n", kv.first.c_str(), kv.second.ms, (long long)kv.second.n, (long long)kv.second.bytes);
    out += line;
  }
  if (out.size() + 1 > cap) { set_err("profile report buffer too small"); return LLIE_ERR_ARG; }
  memcpy(buf, out.c_str(), out.size() + 1);
  return LLIE_OK;
}

// Every recorded launch, in launch order: "class\tkernel\ttag\tms\talgorithmic_bytes\n" (tools/gpu_layers.py).
int llie_profile_dump(llie_ctx* c, char* buf, size_t cap) {
  if (!c || !buf || cap < 2) return LLIE_ERR_ARG;
  c->prof_mask = 0;
  std::string out;
  char line[640];
  for (auto& r : c->prof) {
    float t = 0.f;
    if (hipError_t e = elapsed_ms(r, &t)) return (int)e;
    snprintf(line, sizeof line, "%d\t%s\t%s\t%.6f\t%lld\n", r.cls, r.name ? r.name : "?", r.tag, t, (long long)r.bytes);
    out += line;
  }
  if (out.size() + 1 > cap) { set_err("profile dump buffer too small"); return LLIE_ERR_ARG; }
  memcpy(buf, out.c_str(), out.size() + 1);
  return LLIE_OK;
}

}  // extern "C"
