// The scheduler loop of LowLightDiffusion.enhance: launch sequence, hipGraph cache and the concurrent half-batch branches.
#include "engine.h"

using namespace llie;

extern "C" {

int llie_lcm_step(const float* mo, const float* sample, const float* noise, float* prev, float* x0, float* clamped,
                  int64_t n, const llie_step_coef* k, llie_stream stream) {
  if (!mo || !sample || !prev || !k || n <= 0) return LLIE_ERR_ARG;
  if (!step_coef_ok(*k) || (!k->is_last && !k->sampler && !noise)) return LLIE_ERR_ARG;
  return kerr("lcm_step", launch_lcm_step(mo, sample, noise, prev, x0, clamped, n, step_coef(*k), hs(stream)), 0);
}

int llie_dpm_step(const float* mo, const float* sample, float* hist, float* prev, float* clamped, int64_t n, const llie_dpm_coef* k,
                  llie_stream stream) {
  if (!k) return LLIE_ERR_ARG;
  return kerr("dpm_step", launch_dpm_step(mo, sample, hist, prev, clamped, n, dpm_coef(*k), hs(stream)), LLIE_ERR_ARG,
              "null or unaligned pointer, n <= 0, an order other than 1 or 2, or a non-finite coefficient");
}

int llie_add_noise(const float* x0, const float* noise, const int64_t* t, const float* acp, int table_len, float* out, int batch,
                   int64_t per, int velocity, llie_stream stream) {
  if (!x0 || !noise || !t || !acp || !out || batch <= 0 || per <= 0 || table_len <= 0) return LLIE_ERR_ARG;
  return kerr("add_noise", launch_add_noise(x0, noise, t, acp, out, batch, per, velocity, table_len, hs(stream)), 0);
}

// The coefficients of a loop, [steps]: `k` for the LCM and DDIM samplers (llie_enhance), `d` for DPM-Solver++ 2M (llie_enhance_dpm);
// exactly one is set.
struct Schedule {
  const llie_step_coef* k;
  const llie_dpm_coef* d;
  bool one_draw() const { return d || k[0].sampler; }  // the initial latents are the only noise
  const void* bytes() const { return d ? static_cast<const void*>(d) : static_cast<const void*>(k); }
  size_t step_bytes() const { return d ? sizeof(llie_dpm_coef) : sizeof(llie_step_coef); }
};

// The launch sequence of LowLightDiffusion.enhance (low_light_diffusion.py:204-240): `steps` x
// (UNet forward, scheduler step).  `base` holds two latent ping-pong images and one eps image,
// followed by the UNet workspace.
// `step_batch`: images per step in the noise / inter / preds / timestep arrays (>= batch when this call handles a
// slice of a larger batch; 0 = batch).  Every image is H x W.
static int enhance_sequence(llie_ctx* c, const float* low, const float* noise, const int64_t* t_dev,
                            const Schedule& sc, int steps, float* enhanced, float* inter, float* preds,
                            int batch, int H, int W, char* base, int64_t ws_bytes, llie_stream stream, int step_batch = 0) {
  const int64_t n = (int64_t)batch * 3 * H * W;
  if (step_batch <= 0) step_batch = batch;
  const int64_t sn = (int64_t)step_batch * 3 * H * W;  // elements between consecutive steps
  const size_t img = align_up((size_t)n * 4, 256);
  float* lat[2] = {reinterpret_cast<float*>(base), reinterpret_cast<float*>(base + img)};
  float* eps_ws = reinterpret_cast<float*>(base + 2 * img);
  void* uws = base + 3 * img;
  const int64_t uws_bytes = ws_bytes - (int64_t)(3 * img);
  const float* cur = noise;  // initial latents = first draw (low_light_diffusion.py:208-211)
  if (sc.d) {
    // DPM-Solver++ 2M: the denoiser, then the step as a plain launch in every dtype.  Without `inter` the latents are updated in
    // place in lat[0] (the first step reads the staged initial latents) and the history lives in lat[1]; with it both are free
    float* hist = inter ? lat[0] : lat[1];
    for (int i = 0; i < steps; ++i) {
      float* prev = inter ? inter + (size_t)i * sn : lat[0];
      float* eps = preds ? preds + (size_t)i * sn : eps_ws;
      int rc = unet_forward_impl(c, cur, low, t_dev + (size_t)i * step_batch, 1, eps, nullptr, batch, H, W, uws, uws_bytes, stream);
      if (rc) return rc;
      rc = llie_dpm_step(eps, cur, hist, prev, i == steps - 1 ? enhanced : nullptr, n, &sc.d[i], stream);
      if (rc) return rc;
      cur = prev;
    }
    return LLIE_OK;
  }
  const llie_step_coef* coefs = sc.k;
  const bool fuse = c->dt != LLIE_F32;  // the MFMA output head applies the scheduler step in its epilogue
  for (int i = 0; i < steps; ++i) {
    const bool last = i == steps - 1;
    float* prev = inter ? inter + (size_t)i * sn : lat[i & 1];
    const bool draw = !coefs[i].is_last && !coefs[i].sampler;  // a DDIM step reads no noise: `noise` ends after the initial latents
    const float* nz = draw ? noise + (size_t)(i + 1) * sn : nullptr;
    if (draw && i + 1 >= steps) return LLIE_ERR_ARG;  // a non-final LCM step needs a noise draw
    int rc;
    if (fuse) {
      FusedStep fs{step_coef(coefs[i]), nz, prev, last ? enhanced : nullptr};
      rc = unet_forward_impl(c, cur, low, t_dev + (size_t)i * step_batch, 1, preds ? preds + (size_t)i * sn : nullptr, &fs, batch,
                             H, W, uws, uws_bytes, stream);
      if (rc) return rc;
    } else {
      float* eps = preds ? preds + (size_t)i * sn : eps_ws;
      rc = unet_forward_impl(c, cur, low, t_dev + (size_t)i * step_batch, 1, eps, nullptr, batch, H, W, uws, uws_bytes, stream);
      if (rc) return rc;
      rc = llie_lcm_step(eps, cur, nz, prev, nullptr, last ? enhanced : nullptr, n, &coefs[i], stream);
      if (rc) return rc;
    }
    cur = prev;
  }
  return LLIE_OK;
}

// llie_enhance / llie_enhance_dpm (H = W = image_size) and llie_enhance_hw / llie_enhance_dpm_hw
static int enhance_impl(llie_ctx* c, const float* low, const float* noise, const int64_t* t_dev, const Schedule& sc,
                        int steps, float* enhanced, float* inter, float* preds, int batch, int H, int W, void* ws, int64_t ws_bytes,
                        llie_stream stream) {
  if (!c || !low || !noise || !t_dev || (!sc.k && !sc.d) || !enhanced || !ws || steps <= 0 || batch <= 0 || c->cfg.kind != LLIE_UNET)
    return LLIE_ERR_ARG;
  for (int i = 0; i < steps; ++i) {
    if (sc.d) {  // the first step has no history to read
      if (dpm_coef_ok(dpm_coef(sc.d[i])) && (i > 0 || sc.d[i].order == 1)) continue;
      set_err("enhance: step %d: a DPM coefficient has order 1 or 2 (the first: 1) and finite scalars", i);
    } else {
      if (step_coef_ok(sc.k[i]) && sc.k[i].sampler == sc.k[0].sampler) continue;
      set_err("enhance: step %d: a schedule is all LCM or all DDIM steps, and DDIM has no clamp_x0", i);
    }
    return LLIE_ERR_ARG;
  }
  const int64_t n = (int64_t)batch * 3 * H * W;
  const size_t img = align_up((size_t)n * 4, 256);
  if ((int64_t)(3 * img) > ws_bytes) { set_err("workspace too small"); return LLIE_ERR_WORKSPACE; }
  char* base = reinterpret_cast<char*>(ws);
  hipStream_t us = hs(stream);  // the caller's stream

  // ---- hipGraph path: the ~800 launches of a 4-step loop are launch-bound in their runs of tiny
  // kernels (GroupNorm finalize, SE MLP).  The sequence is captured once per (shape, schedule,
  // workspace) with every pointer inside the workspace: user tensors are staged in/out by plain
  // async copies around the graph launch.  First use of a key runs eagerly (it also performs the
  // one-time hipFuncSetAttribute calls, which must not happen during capture).
  static const bool no_graph = getenv("LLIE_NO_GRAPH") != nullptr;
  const size_t n_noise = sc.one_draw() ? 1 : (size_t)steps;    // DDIM, DPM: the initial latents are the only draw, whatever `steps`
  const size_t n_in = 1 + n_noise;                             // low + noise draws
  const size_t n_out = 1 + (inter ? steps : 0) + (preds ? steps : 0);
  const size_t tbytes = align_up((size_t)steps * batch * 8, 256);
  const size_t stage = (n_in + n_out) * img + tbytes;
  const int64_t seq_bytes = ws_bytes - (int64_t)stage;
  // a loop of more than graph_max_steps steps is not worth capturing (several thousand nodes: DESIGN.md 7): plain launches
  bool use_graph = !no_graph && c->prof_mask == 0 && steps <= g_knobs.graph_max_steps && seq_bytes >= frame_workspace(c, batch, H, W, 0);
  if (!use_graph) return enhance_sequence(c, low, noise, t_dev, sc, steps, enhanced, inter, preds, batch, H, W, base, ws_bytes, stream);

  std::string key(reinterpret_cast<const char*>(sc.bytes()), sc.step_bytes() * steps);
  char tail[128];
  snprintf(tail, sizeof tail, "|%s%d|%dx%d|%d|%d|%d|%p|%lld|%d|%d", sc.d ? "dpm" : "", batch, H, W, steps, inter ? 1 : 0, preds ? 1 : 0, ws, (long long)ws_bytes,
           g_knobs.enhance_split, g_knobs.epoch);
  key += tail;
  if (c->graphs.find(key) == c->graphs.end() && c->graphs.size() >= llie_ctx::kMaxGraphs) {  // evict the least recently used entry
    auto lru = c->graphs.begin();
    for (auto it = c->graphs.begin(); it != c->graphs.end(); ++it)
      if (it->second.used < lru->second.used) lru = it;
    if (lru->second.exec || lru->second.graph) (void)hipDeviceSynchronize();  // a replay of it may still be in flight (on any stream); evictions are rare
    if (lru->second.exec) (void)hipGraphExecDestroy(lru->second.exec);
    if (lru->second.graph) (void)hipGraphDestroy(lru->second.graph);
    c->graphs.erase(lru);
  }
  llie_ctx::GraphEntry& ge = c->graphs[key];
  ge.used = ++c->graph_clock;
  if (!ge.seen) {
    ge.seen = true;
    return enhance_sequence(c, low, noise, t_dev, sc, steps, enhanced, inter, preds, batch, H, W, base, ws_bytes, stream);
  }
  // staging area at the tail of the workspace
  char* st = base + seq_bytes;
  float* s_low = reinterpret_cast<float*>(st);
  float* s_noise = reinterpret_cast<float*>(st + img);
  float* s_enh = reinterpret_cast<float*>(st + n_in * img);
  float* s_inter = inter ? reinterpret_cast<float*>(st + (n_in + 1) * img) : nullptr;
  float* s_preds = preds ? reinterpret_cast<float*>(st + (n_in + 1 + (inter ? steps : 0)) * img) : nullptr;
  int64_t* s_t = reinterpret_cast<int64_t*>(st + (n_in + n_out) * img);
  // NB: staged noise / inter / preds are step-major with stride `img` >= n*4; keep them dense (img == n*4 when n*4 % 256 == 0)
  if (img != (size_t)n * 4) return enhance_sequence(c, low, noise, t_dev, sc, steps, enhanced, inter, preds, batch, H, W, base, ws_bytes, stream);
  hipError_t e = hipMemcpyAsync(s_low, low, (size_t)n * 4, hipMemcpyDeviceToDevice, us);
  if (e == hipSuccess) e = hipMemcpyAsync(s_noise, noise, (size_t)n * 4 * n_noise, hipMemcpyDeviceToDevice, us);
  if (e == hipSuccess) e = hipMemcpyAsync(s_t, t_dev, (size_t)steps * batch * 8, hipMemcpyDeviceToDevice, us);
  if (e != hipSuccess) { set_err("enhance staging: %s", hipGetErrorString(e)); return (int)e; }
  if (!ge.exec) {
    if (!c->cap_stream) {
      e = hipStreamCreateWithFlags(&c->cap_stream, hipStreamNonBlocking);
      if (e != hipSuccess) { set_err("hipStreamCreate: %s", hipGetErrorString(e)); return (int)e; }
    }
    e = hipStreamBeginCapture(c->cap_stream, hipStreamCaptureModeThreadLocal);
    if (e != hipSuccess) { set_err("hipStreamBeginCapture: %s", hipGetErrorString(e)); return (int)e; }
    int rc = LLIE_OK;
    // The batch as Knobs::enhance_split (default 2) concurrent branches of the graph: no operator mixes samples and every kernel
    // is bitwise batch-invariant, so the result is unchanged; memory-bound kernels of one branch overlap with the
    // latency / MFMA-bound ones and the launch boundaries of the others (llie_tune("enhance_split", 0 or 1): a single chain).
    int nbr = g_knobs.enhance_split < 2 ? 1 : (g_knobs.enhance_split > kMaxBranches ? kMaxBranches : g_knobs.enhance_split);
    while (nbr > 1 && batch / nbr < 8) --nbr;  // branches of fewer than 8 images lose more in kernel efficiency than they hide
    int hb[kMaxBranches];
    size_t woff[kMaxBranches];
    int64_t wsz[kMaxBranches];
    size_t wtot = 0;
    for (int i = 0; i < nbr; ++i) {
      hb[i] = batch / nbr + (i < batch % nbr ? 1 : 0);
      wsz[i] = frame_workspace(c, hb[i], H, W, 0);
      if (wsz[i] <= 0) { nbr = 1; break; }
      woff[i] = wtot;
      wtot += align_up((size_t)wsz[i], 256);
    }
    if (nbr > 1 && (int64_t)wtot > seq_bytes) nbr = 1;
    if (nbr > 1) {
      hipError_t e2 = hipSuccess;
      if (!c->ev_fork) e2 = hipEventCreateWithFlags(&c->ev_fork, hipEventDisableTiming);
      for (int i = 1; i < nbr && e2 == hipSuccess; ++i) {
        if (!c->branch_stream[i]) e2 = hipStreamCreateWithFlags(&c->branch_stream[i], hipStreamNonBlocking);
        if (e2 == hipSuccess && !c->branch_join[i]) e2 = hipEventCreateWithFlags(&c->branch_join[i], hipEventDisableTiming);
      }
      if (e2 == hipSuccess) e2 = hipEventRecord(c->ev_fork, c->cap_stream);
      for (int i = 1; i < nbr && e2 == hipSuccess; ++i) e2 = hipStreamWaitEvent(c->branch_stream[i], c->ev_fork, 0);  // joins the capture
      if (e2 != hipSuccess) { hipGraph_t gd = nullptr; (void)hipStreamEndCapture(c->cap_stream, &gd); if (gd) (void)hipGraphDestroy(gd);
                              set_err("enhance split: %s", hipGetErrorString(e2)); return (int)e2; }
      size_t img0 = 0;  // first image of the branch
      for (int i = 0; i < nbr; ++i) {
        const size_t off = img0 * 3 * H * W;
        hipStream_t bs = i == 0 ? c->cap_stream : c->branch_stream[i];
        const int rci = enhance_sequence(c, s_low + off, s_noise + off, s_t + img0, sc, steps, s_enh + off, s_inter ? s_inter + off : nullptr,
                                         s_preds ? s_preds + off : nullptr, hb[i], H, W, base + woff[i], wsz[i], reinterpret_cast<llie_stream>(bs), batch);
        if (rc == LLIE_OK) rc = rci;
        img0 += hb[i];
      }
      for (int i = 1; i < nbr; ++i) {
        e2 = hipEventRecord(c->branch_join[i], c->branch_stream[i]);
        if (e2 == hipSuccess) e2 = hipStreamWaitEvent(c->cap_stream, c->branch_join[i], 0);
        if (e2 != hipSuccess && rc == LLIE_OK) { set_err("enhance split join: %s", hipGetErrorString(e2)); rc = (int)e2; }
      }
    } else {
      rc = enhance_sequence(c, s_low, s_noise, s_t, sc, steps, s_enh, s_inter, s_preds, batch, H, W, base, seq_bytes,
                            reinterpret_cast<llie_stream>(c->cap_stream));
    }
    hipGraph_t g = nullptr;
    e = hipStreamEndCapture(c->cap_stream, &g);
    if (rc != LLIE_OK) { if (g) (void)hipGraphDestroy(g); return rc; }
    if (e != hipSuccess || !g) { set_err("hipStreamEndCapture: %s", hipGetErrorString(e)); return (int)(e ? e : hipErrorUnknown); }
    e = hipGraphInstantiate(&ge.exec, g, nullptr, nullptr, 0);
    if (e != hipSuccess) { (void)hipGraphDestroy(g); ge.exec = nullptr; set_err("hipGraphInstantiate: %s", hipGetErrorString(e)); return (int)e; }
    ge.graph = g;
  }
  e = hipGraphLaunch(ge.exec, us);
  if (e == hipSuccess) e = hipMemcpyAsync(enhanced, s_enh, (size_t)n * 4, hipMemcpyDeviceToDevice, us);
  if (e == hipSuccess && inter) e = hipMemcpyAsync(inter, s_inter, (size_t)n * 4 * steps, hipMemcpyDeviceToDevice, us);
  if (e == hipSuccess && preds) e = hipMemcpyAsync(preds, s_preds, (size_t)n * 4 * steps, hipMemcpyDeviceToDevice, us);
  if (e != hipSuccess) { set_err("enhance graph launch: %s", hipGetErrorString(e)); return (int)e; }
  return LLIE_OK;
}

int llie_enhance(llie_ctx* c, const float* low, const float* noise, const int64_t* t_dev, const llie_step_coef* coefs,
                 int steps, float* enhanced, float* inter, float* preds, int batch, void* ws, int64_t ws_bytes,
                 llie_stream stream) {
  if (!c) return LLIE_ERR_ARG;
  return enhance_impl(c, low, noise, t_dev, Schedule{coefs, nullptr}, steps, enhanced, inter, preds, batch, c->cfg.image_size,
                      c->cfg.image_size, ws, ws_bytes, stream);
}

int llie_enhance_hw(llie_ctx* c, const float* low, const float* noise, const int64_t* t_dev, const llie_step_coef* coefs,
                    int steps, float* enhanced, float* inter, float* preds, int batch, int height, int width, void* ws,
                    int64_t ws_bytes, llie_stream stream) {
  if (!c || !low || !noise || !t_dev || !coefs || !enhanced || !ws || steps <= 0 || batch <= 0 || c->cfg.kind != LLIE_UNET)
    return LLIE_ERR_ARG;
  const int rc = frame_shape_ok(c, batch, height, width);
  return rc ? rc : enhance_impl(c, low, noise, t_dev, Schedule{coefs, nullptr}, steps, enhanced, inter, preds, batch, height, width, ws,
                                ws_bytes, stream);
}

int llie_enhance_dpm(llie_ctx* c, const float* low, const float* noise, const int64_t* t_dev, const llie_dpm_coef* coefs, int steps,
                     float* enhanced, float* inter, float* preds, int batch, void* ws, int64_t ws_bytes, llie_stream stream) {
  if (!c) return LLIE_ERR_ARG;
  return enhance_impl(c, low, noise, t_dev, Schedule{nullptr, coefs}, steps, enhanced, inter, preds, batch, c->cfg.image_size,
                      c->cfg.image_size, ws, ws_bytes, stream);
}

int llie_enhance_dpm_hw(llie_ctx* c, const float* low, const float* noise, const int64_t* t_dev, const llie_dpm_coef* coefs, int steps,
                        float* enhanced, float* inter, float* preds, int batch, int height, int width, void* ws, int64_t ws_bytes,
                        llie_stream stream) {
  if (!c || !low || !noise || !t_dev || !coefs || !enhanced || !ws || steps <= 0 || batch <= 0 || c->cfg.kind != LLIE_UNET)
    return LLIE_ERR_ARG;
  const int rc = frame_shape_ok(c, batch, height, width);
  return rc ? rc : enhance_impl(c, low, noise, t_dev, Schedule{nullptr, coefs}, steps, enhanced, inter, preds, batch, height, width, ws,
                                ws_bytes, stream);
}

// number of entries in the context's hipGraph cache (bounded by kMaxGraphs, least recently used evicted)
int llie_graph_cache_entries(const llie_ctx* c) { return c ? (int)c->graphs.size() : LLIE_ERR_ARG; }

}  // extern "C"
