// Tuning knobs, the kernels' cycle-stamp readers and the per-launch HIP-event profiler.
#include "engine.h"

using namespace llie;

// Every knob: its name for llie_tune, its slot in g_knobs (`n` consecutive ints), its default and how llie_tune turns a caller's
// value into the stored one.  g_knobs is initialised from this table when the library is loaded, together with the two environment
// variables, which are read once, there (no other file's initialiser depends on this one).
enum KnobRule {
  kAsGiven,      // the value
  kOnOff,        // value != 0
  kZeroToTwo,    // the value if it is in 0..2, else 1
  kPositive,     // the value if it is > 0, else the default
  kNotNegative,  // a negative value is ignored
};
struct KnobRow { const char* name; size_t slot; int n; int def; KnobRule rule; };
#define SLOT(field) offsetof(Knobs, field)
static const KnobRow kKnobTable[] = {
  // Recompute form (irbx.hip: statistics-only expand + tile-fused expand/depthwise): default for the
  // inference path of 2-byte engines wherever irbx_supported(); llie_tune("irbx", 0) restores the unfused pair.
  {"irbx", SLOT(use_irbx), 1, 1, kOnOff},  // (0 when LLIE_NO_IRBX is set)
  // Recompute blocks irbx_project_supported names: the SE pool from a pass that only rebuilds h1 (expand_pool), the project GEMM
  // as expand_dw's tail (expand_dw_project) -- h2 never reaches HBM either; llie_tune("irbx_project", 0) restores expand_dw +
  // pw_gemm, 2 keeps only the identity-residual shapes (A/B of the 96 -> 32 skip-conv block alone).
  {"irbx_project", SLOT(irbx_project), 1, 1, kZeroToTwo},
  // The two wide decoder blocks wide_project_supported names keep the expand GEMM and its stored h1, but go without h2: the SE
  // pool from one read of h1 (dwconv3x3_pool), then depthwise + gate + project + skip conv in one kernel (dwconv3x3_project);
  // llie_tune("wide_project", 0) restores dwconv3x3 + pw_gemm.
  {"wide_project", SLOT(wide_project), 1, 1, kOnOff},
  // Of those, the 192 -> 64 block knows norm2's tables before its expand GEMM runs (the Gram of the activated input, gram.hip):
  // pw_expand stores the activated h1 and adds the pool totals itself, the pool pass goes.  llie_tune("wide_gram", 0) restores it,
  // 2 takes the form at every map size (1: from 4096 pixels per image).
  {"wide_gram", SLOT(wide_gram), 1, 1, kZeroToTwo},
  {"gram", SLOT(gram), 1, 1, kAsGiven},  // norm2 statistics of the recompute form from the Gram matrix of the block input (gram.hip); 0 = expand_stats
  // Cache policy of the big activation tensors (inference): a tensor of at least nt_min_mb MiB (this run's batch) is stored
  // non-temporally by its producer (common.h: st_vec_pol).  nt_mask picks the producers: 1 expand_dw (h2), 2 pw_expand (h1),
  // 4 dwconv3x3 (h2), 8 project / attention GEMM outputs, 16 dense 3x3 conv outputs.  Values never change, only where lines live.
  {"nt_min_mb", SLOT(nt_min_mb), 1, 100, kAsGiven},
  {"nt_mask", SLOT(nt_mask), 1, 1, kAsGiven},
  // Up-sampling convs from folded weights (upconv.hip: conv3x3_upfold_kernel) wherever upconv_fold_supported();
  // llie_tune("upconv_fold", 0) restores conv3x3_kernel's mode 1, which blends the patch itself.
  {"upconv_fold", SLOT(upconv_fold), 1, 1, kOnOff},
  // Up-sampling convs from nine low-resolution tap maps blended on chip (upconv.hip: conv3x3_upmaps_kernel) wherever
  // upconv_maps_supported(), which is asked first; llie_tune("upconv_maps", 0) leaves the choice to upconv_fold alone.
  {"upconv_maps", SLOT(upconv_maps), 1, 1, kOnOff},
  {"se_mfma", SLOT(se_mfma), 1, 1, kAsGiven},  // SE MLP of the wide blocks as two MFMA launches (small.hip: se_fc1_mfma / se_fc2_mfma); 0 = the row-parallel pair
  // Backward pass: run the weight-gradient kernels on a side stream next to the activation-gradient chain
  // (llie_tune("bwd_async", 0) puts everything back on the caller's stream).
  {"bwd_async", SLOT(bwd_async), 1, 1, kAsGiven},
  // hipGraph path of llie_enhance: batches of 16 and more are captured as two concurrent half-batch branches (no operator
  // mixes samples and every kernel is bitwise batch-invariant, so the bits do not change): the launch-bound tail of one
  // half (norm finalisation, SE MLP) overlaps the streaming kernels of the other, +4 % at B = 32.  Overlapping kernels
  // stretch each other, so per-kernel durations are only meaningful from a single chain: llie_profile_* already forces
  // the eager single chain, and LLIE_ENHANCE_SPLIT=0 (or llie_tune("enhance_split", 0)) gives rocprofv3 the same.
  {"enhance_split", SLOT(enhance_split), 1, 2, kAsGiven},  // (LLIE_ENHANCE_SPLIT's value when it is set)
  // Loops longer than this are not captured (llie_tune("graph_max_steps", n); n <= 0 restores the default): DESIGN.md 7 has the
  // measurement behind the number.
  {"graph_max_steps", SLOT(graph_max_steps), 1, kGraphMaxSteps, kPositive},
  // The launchers' own (kernels.h, Knobs)
  {"pwx", SLOT(pwx), 1, 1, kAsGiven},
  {"gemm_bk", SLOT(gemm_bk), 1, 0, kAsGiven},
  {"irbx_dbuf", SLOT(irbx_dbuf), 1, 0, kNotNegative},
  {"irbx_grid", SLOT(irbx_grid), 3, 0, kAsGiven},  // all three input widths
  {"irbx_grid2", SLOT(irbx_grid[0]), 1, 0, kAsGiven},
  {"irbx_grid4", SLOT(irbx_grid[1]), 1, 0, kAsGiven},
  {"irbx_grid6", SLOT(irbx_grid[2]), 1, 0, kAsGiven},
  // Diagnostics: the cycle-stamped builds, read back by llie_debug_*_stamps below
  {"gemm_stamp", SLOT(gemm_stamp), 1, 0, kAsGiven},
  {"pwx_stamp", SLOT(pwx_stamp), 1, 0, kAsGiven},
  {"conv_stamp", SLOT(conv_stamp), 1, 0, kAsGiven},
  {"irbx_stamp", SLOT(irbx_stamp), 1, 0, kAsGiven},
};
#undef SLOT
static int* knob_slot(Knobs& k, const KnobRow& r) { return reinterpret_cast<int*>(reinterpret_cast<char*>(&k) + r.slot); }
static void knob_store(Knobs& k, const KnobRow& r, int value) {
  for (int i = 0; i < r.n; ++i) knob_slot(k, r)[i] = value;
}
static Knobs knob_defaults() {
  Knobs k{};
  for (const KnobRow& r : kKnobTable) knob_store(k, r, r.def);
  if (getenv("LLIE_NO_IRBX")) k.use_irbx = 0;
  if (getenv("LLIE_ENHANCE_SPLIT")) k.enhance_split = atoi(getenv("LLIE_ENHANCE_SPLIT"));
  // Captured graphs bake in the kernel choices of the moment: every llie_tune call starts a new epoch of the graph cache.
  k.epoch = 0;
  return k;
}
Knobs llie::g_knobs = knob_defaults();

// StampSink (kernels.h): the buffer of a stamped launch, and the means llie_debug_*_stamps report
hipError_t StampSink::arm(size_t launch_waves, unsigned long long** stamps) {
  if (max_waves && launch_waves > max_waves) return hipErrorInvalidValue;
  if (launch_waves > cap || !buf) {
    if (buf) (void)hipFree(buf);
    buf = nullptr; cap = 0;
    if (hipError_t e = hipMalloc(reinterpret_cast<void**>(&buf), launch_waves * slots * sizeof(unsigned long long)); e != hipSuccess) return e;
    cap = launch_waves;
  }
  waves = launch_waves;
  *stamps = buf;
  return hipSuccess;
}
hipError_t StampSink::fetch(double* out) const {
  if (!buf || !waves) return hipErrorInvalidValue;
  std::vector<unsigned long long> h(waves * slots);
  if (hipError_t e = hipMemcpy(h.data(), buf, h.size() * sizeof(unsigned long long), hipMemcpyDeviceToHost); e != hipSuccess) return e;
  for (int i = 0; i < slots; ++i) out[i] = 0.0;
  for (size_t i = 0; i < h.size(); ++i) out[i % slots] += (double)h[i];
  for (int i = 0; i < slots; ++i) out[i] /= (double)waves;
  out[slots] = (double)waves;
  return hipSuccess;
}

// one profiled launch's duration, once it has finished
static hipError_t elapsed_ms(const llie_ctx::ProfRec& r, float* ms) {
  hipError_t e = hipEventSynchronize(r.e1);
  if (e == hipSuccess) e = hipEventElapsedTime(ms, r.e0, r.e1);
  if (e != hipSuccess) set_err("profile: %s", hipGetErrorString(e));
  return e;
}

// diagnostics: mean per-wave cycles of the last stamped launch of one kernel family (llie_tune("*_stamp", 1)); synchronises
static int read_stamps(double* out, const StampSink& sink) {
  if (!out) return LLIE_ERR_ARG;
  hipError_t e = hipDeviceSynchronize();
  if (e == hipSuccess) e = sink.fetch(out);
  return e == hipSuccess ? LLIE_OK : LLIE_ERR_ARG;
}

extern "C" {

int llie_tune(const char* knob, int value) {
  if (!knob) return LLIE_ERR_ARG;
  ++g_knobs.epoch;
  for (const KnobRow& r : kKnobTable) {
    if (strcmp(knob, r.name)) continue;
    switch (r.rule) {
      case kAsGiven: break;
      case kOnOff: value = value != 0; break;
      case kZeroToTwo: value = value < 0 || value > 2 ? 1 : value; break;
      case kPositive: value = value > 0 ? value : r.def; break;
      case kNotNegative: if (value < 0) return LLIE_OK; break;
    }
    knob_store(g_knobs, r, value);
    return LLIE_OK;
  }
  return LLIE_ERR_ARG;
}

int llie_debug_gemm_stamps(double* out3) { return read_stamps(out3, g_gemm_stamps); }
int llie_debug_pwx_stamps(double* out4) { return read_stamps(out4, g_pwx_stamps); }
int llie_debug_conv_stamps(double* out8) { return read_stamps(out8, g_conv_stamps); }   // the up-sampling conv
int llie_debug_irbx_stamps(double* out10) { return read_stamps(out10, g_irbx_stamps); }  // expand_dw, expand_pool, expand_dw_project

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
