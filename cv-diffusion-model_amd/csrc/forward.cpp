// The inference launch sequence (and the training forward, which records a tape) and its workspace plan.
#include "engine.h"

using namespace llie;

namespace {

struct Run : Exec {
  Tape* tape = nullptr;  // non-null: training forward -- nothing is released, every operator is recorded
  char tag[56] = "";     // label of the operator being launched (llie_profile_dump)
  void rel(size_t off) { if (!tape) ar->free(off); }
  // Zero-initialised totals (inference): fixed-point accumulators that kernels add to with integer atomics (SE pool sums).
  // One block of the arena per forward, cleared by a single memset node at its start and handed out by ztake() in
  // launch order; its size comes from a counting dry run of the same forward (cached per batch, height and width).
  size_t zoff = 0, zcur = 0, zcap = 0;
  bool zcount = false;
  template <typename F> void zbegin(int H, int W, F&& forward_again) {
    if (tape || zcount) return;
    const auto key = std::make_tuple(B, H, W, g_knobs.epoch);
    auto it = c->zneed.find(key);
    if (it == c->zneed.end()) {
      size_t zbytes = 0;
      plan(c, B, forward_again, &zbytes);
      it = c->zneed.emplace(key, zbytes).first;
    }
    zcap = it->second;
    if (!zcap) return;
    zoff = ar->alloc(zcap);
    // a kernel of ours, not hipMemsetAsync: as a memset node of the captured graph it stopped clearing the region once another
    // engine context had run between two replays (ROCm 7.2; tests/test_gpu_round2.py::test_inplace_data_writes_are_noticed)
    if (!dry) chk(launch_zero_fill(ws + zoff, (int64_t)zcap, s));
  }
  size_t ztake(size_t bytes) {
    bytes = align_up(bytes, 256);
    const size_t off = zoff + zcur;
    zcur += bytes;
    if (!zcount && zcur > zcap) chk(hipErrorOutOfMemory);
    return off;
  }

  // Dry run of `forward` in an unbounded arena: returns its high-water mark, the workspace plan (zbytes: a counting run
  // for zbegin, which also reports the zero-initialised bytes the forward takes)
  template <typename F> static size_t plan(llie_ctx* c, int B, F&& forward, size_t* zbytes = nullptr) {
    Arena probe;
    Run d{Exec::planning(c, &probe, B)};
    d.zcount = zbytes != nullptr;
    forward(d);
    if (zbytes) *zbytes = d.zcur;
    return probe.high;
  }
  int nt_store(int site, int64_t elems) const {  // see Knobs::nt_min_mb
    return !tape && (g_knobs.nt_mask & site) && g_knobs.nt_min_mb > 0 && elems * (int64_t)elem_size(dt) >= ((int64_t)g_knobs.nt_min_mb << 20) ? 1 : 0;
  }
  // launch `f` bracketed by HIP events on the launch stream when its class is being profiled
  template <typename F> void timed(int cls, int64_t bytes, F&& f, const char* nm = nullptr) {
    if (!(c->prof_mask & cls) || c->prof.size() >= 8192) { chk(f()); return; }
    llie_ctx::ProfRec r{cls, bytes, c->get_event(), c->get_event(), "", {0}};
    snprintf(r.tag, sizeof r.tag, "%s", tag);
    if (!r.e0 || !r.e1) { chk(f()); return; }
    chk(hipEventRecord(r.e0, s));
    chk(f());
    chk(hipEventRecord(r.e1, s));
    r.name = nm ? nm : last_kernel();  // static storage: launchers pass string literals / function-local statics
    c->prof.push_back(r);
  }

  Tens new_tens(int C, int H, int W, int ntiles, int Cr = 0) {
    Tens t;
    t.C = C; t.H = H; t.W = W; t.ntiles = ntiles; t.valid = true;
    t.Cr = Cr > 0 ? Cr : C;
    t.off = ar->alloc((size_t)B * H * W * C * es());
    t.slab = ar->alloc((size_t)B * ntiles * 2 * C * 4);
    return t;
  }
  void free_tens(Tens& t) {
    if (!t.valid || tape) return;
    ar->free(t.off);
    ar->free(t.slab);
    t.valid = false;
  }
  StatSrc src(const Tens& t) const { return StatSrc{p<float>(t.slab), t.ntiles, t.C}; }

  // GroupNorm affine of (x0 [+ x1]) -> freshly allocated as/ab [B][C]; returns offsets
  void gn(const Tens& x0, const Tens* x1, size_t gamma, size_t beta, const float* film, int64_t film_stride,
          size_t& as, size_t& ab, GnRec* rec = nullptr, float post_scale = 0.f) {
    const int C = x0.C + (x1 ? x1->C : 0);
    const int Creal = x0.Cr + (x1 ? x1->Cr : 0);  // x0 is unpadded whenever x1 exists (checked at build time)
    as = ar->alloc((size_t)B * C * 4);
    ab = ar->alloc((size_t)B * C * 4);
    size_t mo = 0, ro = 0;
    if (tape && rec) {
      mo = ar->alloc((size_t)B * 32 * 4);
      ro = ar->alloc((size_t)B * 32 * 4);
      rec->as = as; rec->ab = ab; rec->mean = mo; rec->rstd = ro;
    }
    if (dry) return;
    GnFinalizeArgs a{};
    a.src[0] = src(x0);
    if (x1) a.src[1] = src(*x1);
    a.C = C; a.Creal = Creal; a.groups = gn_groups(Creal); a.P = x0.H * x0.W;
    a.gamma = wptr<float>(gamma); a.beta = wptr<float>(beta);
    a.film = film; a.film_stride = film_stride; a.eps = 1e-5f;
    a.as = p<float>(as); a.ab = p<float>(ab); a.B = B; a.post_scale = post_scale;
    if (tape && rec) { a.mean_out = p<float>(mo); a.rstd_out = p<float>(ro); }
    timed(LLIE_K_OTHER, (int64_t)B * C * 8, [&] { return launch_gn_finalize(a, s); }, "gn_finalize_kernel");
  }

  // one-segment GEMM out[M][N] = act(seg) W[N][K]^T; callers add further segments, a residual or the store policy
  static GemmArgs gemm1(GemmSeg seg, const void* w, void* out, float* stats, int M, int N, int K, int P) {
    GemmArgs g{};
    g.seg[0] = seg; g.nseg = 1; g.w = w; g.out = out; g.stats = stats; g.M = M; g.N = N; g.K = K; g.P = P;
    return g;
  }
  // the block's SE MLP over pool partials or totals the caller adds (small.hip)
  SeArgs se_args(const IrbW& w, int P, size_t semean, size_t sehid, size_t gate) const {
    SeArgs e{};
    e.P = P; e.w1 = wptr(w.se_w1); e.b1 = wptr<float>(w.se_b1); e.w2 = wptr(w.se_w2); e.b2 = wptr<float>(w.se_b2);
    e.mean = p<float>(semean); e.hid = p<float>(sehid); e.gate = p<float>(gate); e.B = B; e.C = w.hid; e.Cs = w.sq;
    return e;
  }

  // What the stages of one inverted-residual block hand on (workspace offsets)
  struct IrbTmp {
    size_t as1 = 0, ab1 = 0, as2 = 0, ab2 = 0;  // norm1 / norm2 + FiLM tables
    Tens h1;                                    // unfused form only
    size_t h2 = 0, pool = 0, ptot = 0;          // depthwise output (none in the project form); SE pool: tile partials or fixed-point totals
    int dnt = 0;                                // tiles per image of the kernel that pooled
    size_t sehid = 0, semean = 0, gate = 0;
    IrbxArgs xa{};                              // recompute forms: the kernels' inputs (irbx.hip); each launch adds its outputs to a copy
  };

  // Wide Gram form (IrbPath::wgram): norm2's tables from the Gram of the activated input, then the expand GEMM stores the activated
  // h1 and adds the SE pool totals.  No statistics slab of h1, no second gn launch, no pool pass.
  void front_wide_gram(const IrbW& w, const Tens& x0, const Tens* x1, const float* film, int64_t film_stride, IrbTmp& t) {
    const int H = x0.H, W = x0.W, P = H * W, M = B * P;
    Tens& h1 = t.h1;
    h1.C = w.hid; h1.Cr = w.hid_r; h1.H = H; h1.W = W; h1.ntiles = 0; h1.valid = true;
    t.as2 = ar->alloc((size_t)B * w.hid * 4); t.ab2 = ar->alloc((size_t)B * w.hid * 4);
    const size_t gpart = ar->alloc((size_t)B * gram_wide_part_floats(P) * 4);
    const size_t gblk = ar->alloc((size_t)B * kGramWideFloats * 4);
    t.dnt = irbx_project_tiles(H, W);
    t.ptot = ztake((size_t)B * w.hid * 8);
    if (!dry) {
      GramWideArgs ga{};
      ga.x0 = p(x0.off); ga.c0 = x0.C; ga.x1 = x1 ? p(x1->off) : nullptr; ga.c1 = x1 ? x1->C : 0; ga.as1 = p<float>(t.as1); ga.ab1 = p<float>(t.ab1);
      ga.part = p<float>(gpart); ga.gblk = p<float>(gblk); ga.B = B; ga.P = P;
      timed(LLIE_K_GEMM, (int64_t)M * w.cin * (int64_t)es(), [&] { return launch_gram_wide(dt, ga, s); });
      GramGroupFinalizeArgs fa{};
      fa.gblk = p<float>(gblk); fa.mg = wptr<double>(w.w_mg); fa.K = w.cin; fa.Chid = w.hid; fa.groups = gn_groups(w.hid); fa.P = P; fa.B = B;
      fa.gamma = wptr<float>(w.n2g); fa.beta = wptr<float>(w.n2b); fa.film = film; fa.film_stride = film_stride; fa.eps = 1e-5f;
      fa.as = p<float>(t.as2); fa.ab = p<float>(t.ab2); fa.post_scale = 1.f / 6.f;
      timed(LLIE_K_OTHER, (int64_t)B * w.hid * 8, [&] { return launch_gram_group_finalize(fa, s); }, "gram_group_finalize_kernel");
    }
    // the Gram's partials are gone before h1 exists: the block's high-water mark stays h1 + its input
    rel(gpart); rel(gblk);
    h1.off = ar->alloc((size_t)M * w.hid * es());
    if (!dry) {
      ExpandArgs x{};
      x.seg[0] = GemmSeg{p(x0.off), x0.C, p<float>(t.as1), p<float>(t.ab1), w.cin, ACT_RELU6_S6};
      x.nseg = 1;
      if (x1) x.seg[x.nseg++] = GemmSeg{p(x1->off), x1->C, p<float>(t.as1) + x0.C, p<float>(t.ab1) + x0.C, w.cin, ACT_RELU6_S6};
      x.wf = wptr(w.w_expand_f); x.out = p(h1.off); x.M = M; x.N = w.hid; x.K = w.cin; x.P = P; x.H = H; x.W = W;
      x.as2 = p<float>(t.as2); x.ab2 = p<float>(t.ab2); x.wd = wptr<float>(w.w_dw); x.pool_tot = p<unsigned long long>(t.ptot);
      x.nt = nt_store(2, (int64_t)M * w.hid);
      const int64_t kbytes = ((int64_t)M * (w.cin + w.hid) + (int64_t)w.hid * w.cin) * (int64_t)es();
      timed(LLIE_K_GEMM, kbytes, [&] { return launch_pw_expand_act(dt, x, s); });
      t.xa = IrbxArgs{};
      t.xa.h1 = p(h1.off); t.xa.h1_act = 1; t.xa.wd = wptr<float>(w.w_dw);
      t.xa.B = B; t.xa.H = H; t.xa.W = W; t.xa.Chid = w.hid;
    }
    rel(t.as1); rel(t.ab1);
  }

  // K1: expand with norm1 + ReLU6 prologue; norm2 + FiLM folded into one affine; K2: depthwise with affine + ReLU6 prologue and SE pool
  void front_unfused(const IrbPath& path, const IrbW& w, const Tens& x0, const Tens* x1, const float* film, int64_t film_stride, IrbRec& rec, IrbTmp& t) {
    const int H = x0.H, W = x0.W, P = H * W, M = B * P;
    Tens& h1 = t.h1;
    h1.C = w.hid; h1.Cr = w.hid_r; h1.H = H; h1.W = W; h1.ntiles = pw_gemm_ntiles(P); h1.valid = true;
    h1.off = ar->alloc((size_t)B * P * w.hid * es());
    h1.slab = ar->alloc((size_t)B * h1.ntiles * 2 * w.hid * 4);
    if (!dry) {
      const int act1 = path.s6 ? ACT_RELU6_S6 : ACT_RELU6;
      GemmArgs g = gemm1(GemmSeg{p(x0.off), x0.C, p<float>(t.as1), p<float>(t.ab1), w.cin, act1}, wptr(w.w_expand), p(h1.off), p<float>(h1.slab), M, w.hid, w.cin, P);
      if (x1) g.seg[g.nseg++] = GemmSeg{p(x1->off), x1->C, p<float>(t.as1) + x0.C, p<float>(t.ab1) + x0.C, w.cin, act1};
      const int64_t kbytes = ((int64_t)M * (w.cin + w.hid) + (int64_t)w.hid * w.cin) * (int64_t)es();
      if (path.s6 && w.has_wf && pw_expand_supported(dt, g.seg, g.nseg, M, w.hid, w.cin, P)) {
        // activation-stationary form: pixels activated once and held in registers, packed weights streamed (pwx.hip)
        ExpandArgs x{};
        for (int i = 0; i < g.nseg; ++i) x.seg[i] = g.seg[i];
        x.nseg = g.nseg; x.wf = wptr(w.w_expand_f); x.out = g.out; x.stats = g.stats; x.M = M; x.N = w.hid; x.K = w.cin; x.P = P;
        x.nt = nt_store(2, (int64_t)M * w.hid);
        timed(LLIE_K_GEMM, kbytes, [&] { return launch_pw_expand(dt, x, s); });
      } else {
        if (path.s6) g.nt = nt_store(2, (int64_t)M * w.hid);
        timed(LLIE_K_GEMM, kbytes, [&] { return launch_pw_gemm(dt, g, s); });
      }
    }
    gn(h1, nullptr, w.n2g, w.n2b, film, film_stride, t.as2, t.ab2, &rec.n2, path.s6 ? 1.f / 6.f : 0.f);
    if (path.form == kIrbWide) {
      // wide form: no h2.  The pool totals from one read of h1 (nine sums); h1 and norm2's tables stay for dwconv3x3_project
      t.dnt = irbx_project_tiles(H, W);
      t.ptot = ztake((size_t)B * w.hid * 8);
      if (!dry) {
        t.xa = IrbxArgs{};
        t.xa.h1 = p(h1.off); t.xa.as2 = p<float>(t.as2); t.xa.ab2 = p<float>(t.ab2); t.xa.wd = wptr<float>(w.w_dw);
        t.xa.B = B; t.xa.H = H; t.xa.W = W; t.xa.Chid = w.hid;
        IrbxArgs a = t.xa;
        a.pool_tot = p<unsigned long long>(t.ptot);
        timed(LLIE_K_DW, (int64_t)M * w.hid * (int64_t)es(), [&] { return launch_dwconv3x3_pool(dt, a, s); });
      }
      rel(t.as1); rel(t.ab1); rel(h1.slab);
      return;
    }
    t.dnt = dwconv_ntiles(H, W);
    t.h2 = ar->alloc((size_t)M * w.hid * es());
    t.pool = path.fixtot ? 0 : ar->alloc((size_t)B * t.dnt * w.hid * 4);
    t.ptot = path.fixtot ? ztake((size_t)B * w.hid * 8) : 0;
    if (!dry) {
      DwArgs d{};
      d.in = p(h1.off); d.out = p(t.h2); d.as = p<float>(t.as2); d.ab = p<float>(t.ab2); d.w = wptr<float>(w.w_dw);
      if (path.fixtot) d.pool_tot = p<unsigned long long>(t.ptot); else d.pool = p<float>(t.pool);
      d.B = B; d.H = H; d.W = W; d.C = w.hid; d.s6 = path.s6 ? 1 : 0; d.nt = nt_store(4, (int64_t)M * w.hid);
      timed(LLIE_K_DW, 2LL * M * w.hid * (int64_t)es(), [&] { return launch_dwconv3x3(dt, d, s); });
    }
    rel(t.as1); rel(t.ab1); rel(h1.off); rel(h1.slab); rel(t.as2); rel(t.ab2);
  }

  IrbxArgs irbx_args(const IrbW& w, const Tens& x0, const Tens* x1, size_t as1, size_t ab1) const {
    IrbxArgs a{};
    a.x0 = p(x0.off); a.c0 = x0.C; a.x1 = x1 ? p(x1->off) : nullptr; a.c1 = x1 ? x1->C : 0; a.as1 = p<float>(as1); a.ab1 = p<float>(ab1);
    a.w1 = wptr(w.w_expand); a.wd = wptr<float>(w.w_dw); a.B = B; a.H = x0.H; a.W = x0.W; a.Chid = w.hid;
    return a;
  }
  // Recompute and project forms (inference, fixed-point pool totals): norm2's statistics without h1, its affine, then expand_dw
  // (h2 and the pool totals) or, project form, expand_pool (the totals alone; the norm tables stay for expand_dw_project)
  void front_recompute(const IrbPath& path, const IrbW& w, const Tens& x0, const Tens* x1, const float* film, int64_t film_stride, IrbTmp& t) {
    const int H = x0.H, W = x0.W, P = H * W, M = B * P;
    const bool pool_only = path.form == kIrbProject;
    Tens st;  // h1 as norm2 sees it: the statistics slab of expand_stats alone
    st.C = w.hid; st.Cr = w.hid_r; st.H = H; st.W = W; st.ntiles = P / irbx_stats_rows(P); st.valid = true;
    st.slab = path.gram ? 0 : ar->alloc((size_t)B * st.ntiles * 2 * w.hid * 4);
    const size_t gpart = path.gram ? ar->alloc((size_t)B * gram_part_floats(w.cin, P) * 4) : 0;
    const size_t gtot = path.gram ? ar->alloc((size_t)B * (w.cin * w.cin + w.cin) * 4) : 0;
    const size_t gtick = path.gram ? ztake((size_t)B * 4) : 0;
    if (!dry) {
      t.xa = irbx_args(w, x0, x1, t.as1, t.ab1);
      if (path.gram) {
        GramArgs ga{};
        ga.x0 = t.xa.x0; ga.x1 = t.xa.x1; ga.c0 = t.xa.c0; ga.c1 = t.xa.c1; ga.as1 = t.xa.as1; ga.ab1 = t.xa.ab1;
        ga.part = p<float>(gpart); ga.gtot = p<float>(gtot); ga.tickets = p<unsigned int>(gtick); ga.B = B; ga.P = P;
        timed(LLIE_K_GEMM, (int64_t)M * w.cin * (int64_t)es(), [&] { return launch_gram_stats(dt, ga, s); });
      } else {
        IrbxArgs a = t.xa;
        a.stats = p<float>(st.slab);
        timed(LLIE_K_GEMM, ((int64_t)M * w.cin + (int64_t)w.hid * w.cin) * (int64_t)es(), [&] { return launch_expand_stats(dt, a, s); });
      }
    }
    if (path.gram) {
      t.as2 = ar->alloc((size_t)B * w.hid * 4); t.ab2 = ar->alloc((size_t)B * w.hid * 4);
      if (!dry) {
        GramFinalizeArgs fa{};
        fa.gtot = p<float>(gtot); fa.w1 = wptr(w.w_expand); fa.K = w.cin; fa.Chid = w.hid; fa.groups = gn_groups(w.hid); fa.P = P; fa.B = B;
        fa.gamma = wptr<float>(w.n2g); fa.beta = wptr<float>(w.n2b); fa.film = film; fa.film_stride = film_stride; fa.eps = 1e-5f;
        fa.as = p<float>(t.as2); fa.ab = p<float>(t.ab2); fa.post_scale = 0.f;
        timed(LLIE_K_OTHER, (int64_t)B * w.hid * 8, [&] { return launch_gram_finalize(dt, fa, s); }, "gram_finalize_kernel");
      }
      rel(gpart);
    } else {
      gn(st, nullptr, w.n2g, w.n2b, film, film_stride, t.as2, t.ab2);
    }
    t.dnt = irbx_pool_tiles(H, W);
    t.h2 = pool_only ? 0 : ar->alloc((size_t)M * w.hid * es());
    t.ptot = ztake((size_t)B * w.hid * 8);
    if (!dry) {
      t.xa.as2 = p<float>(t.as2); t.xa.ab2 = p<float>(t.ab2);
      IrbxArgs a = t.xa;
      a.pool_tot = p<unsigned long long>(t.ptot);
      if (pool_only) {
        timed(LLIE_K_DW, ((int64_t)M * w.cin + (int64_t)w.hid * w.cin) * (int64_t)es(), [&] { return launch_expand_pool(dt, a, s); });
      } else {
        a.out = p(t.h2);
        a.nt = w.cin <= 64 ? nt_store(1, (int64_t)M * w.hid) : 0;  // 96 -> 384: the kernel itself loses more than its consumer gains
        timed(LLIE_K_DW, (int64_t)M * (w.cin + w.hid) * (int64_t)es(), [&] { return launch_expand_dw(dt, a, s); });
      }
    }
    if (!pool_only) { rel(t.as1); rel(t.ab1); }
    rel(path.gram ? gtot : st.slab);
    if (!pool_only) { rel(t.as2); rel(t.ab2); }
  }

  // SE MLP: pool partials or totals -> gate
  // (wide blocks of the 2-byte inference engines: fc1's pre-activations accumulate as integers in the zero-initialised region)
  void se_gate(const IrbPath& path, const IrbW& w, int P, IrbTmp& t) {
    const bool fixtot = path.fixtot;
    const bool sepre_ok = fixtot && dt != LLIE_F32 && g_knobs.se_mfma && w.hid >= 768 && w.hid % 256 == 0 && w.sq % 64 == 0 && w.sq <= 512;
    const size_t sepre = sepre_ok ? ztake((size_t)B * w.sq * 8) : 0;
    t.sehid = ar->alloc((size_t)B * w.sq * 4); t.gate = ar->alloc((size_t)B * w.hid * 4); t.semean = ar->alloc((size_t)B * w.hid * 4);
    if (!dry) {
      SeArgs e = se_args(w, P, t.semean, t.sehid, t.gate);
      e.ntiles = t.dnt;
      if (fixtot) e.tot = p<unsigned long long>(t.ptot); else e.pool = p<float>(t.pool);
      if (sepre_ok) e.pre = p<long long>(sepre);
      if (sepre_ok && se_mlp_mfma_supported(dt, e)) {
        timed(LLIE_K_SE, (int64_t)B * w.hid * 12 + 2LL * w.hid * w.sq * (int64_t)es(), [&] { return launch_se_mlp_mfma(dt, e, s); });
      } else if (fixtot && w.hid <= 384) {
        timed(LLIE_K_SE, (int64_t)B * w.hid * 12 + 2LL * w.hid * w.sq * (int64_t)es(), [&] { return launch_se_gate(dt, e, s); });
      } else timed(LLIE_K_SE, ((int64_t)B * t.dnt * w.hid * 4) + 2LL * w.hid * w.sq * (int64_t)es(), [&] {
        hipError_t r1 = launch_se_fc1(dt, e, s);
        return r1 != hipSuccess ? r1 : launch_se_fc2(dt, e, s);
      });
    }
    if (!fixtot) rel(t.pool);
    rel(t.sehid); rel(t.semean);
  }

  // K3: project with SE gate prologue (+ skip conv as extra K segments, or identity residual)
  Tens project_gemm(const IrbW& w, const Tens& x0, const Tens* x1, IrbTmp& t) {
    const int P = x0.H * x0.W, M = B * P;
    Tens y = new_tens(w.cout, x0.H, x0.W, pw_gemm_ntiles(P), w.cout_r);
    if (!dry) {
      GemmArgs g = gemm1(GemmSeg{p(t.h2), w.hid, p<float>(t.gate), nullptr, w.hid, ACT_NONE}, wptr(w.w_proj), p(y.off), p<float>(y.slab), M, w.cout, w.hid, P);
      if (w.skip) {
        g.seg[g.nseg++] = GemmSeg{p(x0.off), x0.C, nullptr, nullptr, 0, ACT_NONE};
        if (x1) g.seg[g.nseg++] = GemmSeg{p(x1->off), x1->C, nullptr, nullptr, 0, ACT_NONE};
        g.K += w.cin;
      } else {
        g.res = p(x0.off);
      }
      g.nt = nt_store(8, (int64_t)M * w.cout);
      timed(LLIE_K_GEMM, ((int64_t)M * (g.K + w.cout + (w.skip ? 0 : w.cout)) + (int64_t)w.cout * g.K) * (int64_t)es(),
            [&] { return launch_pw_gemm(dt, g, s); });
    }
    rel(t.h2); rel(t.gate);
    return y;
  }
  // project form: expand_dw_project rebuilds h1 and the depthwise result (both norms again), gates, projects, adds the shortcut
  Tens project_fused(const IrbW& w, const Tens& x0, IrbTmp& t) {
    const int H = x0.H, W = x0.W, M = B * H * W;
    Tens y = new_tens(w.cout, H, W, irbx_project_tiles(H, W), w.cout_r);
    if (!dry) {
      IrbxArgs a = t.xa;
      a.gate = p<float>(t.gate); a.wp = wptr(w.w_proj); a.y = p(y.off); a.ystats = p<float>(y.slab);
      a.ldp = w.hid + (w.skip ? w.cin : 0);  // project and skip share one K-concatenated matrix (model.cpp)
      timed(LLIE_K_DW, ((int64_t)M * (w.cin + w.cout) + (int64_t)w.hid * (w.cin + w.cout)) * (int64_t)es(),
            [&] { return launch_expand_dw_project(dt, a, w.cout, w.skip, s); });
    }
    rel(t.as1); rel(t.ab1); rel(t.as2); rel(t.ab2); rel(t.gate);
    return y;
  }

  // wide form: dwconv3x3_project reads the stored h1 with its halo (180 pixels per 128), the raw input for the skip conv, and writes y
  Tens project_wide(const IrbW& w, const Tens& x0, const Tens* x1, IrbTmp& t) {
    const int H = x0.H, W = x0.W, M = B * H * W;
    Tens y = new_tens(w.cout, H, W, irbx_project_tiles(H, W), w.cout_r);
    if (!dry) {
      IrbxArgs a = t.xa;
      a.x0 = p(x0.off); a.c0 = x0.C; a.x1 = x1 ? p(x1->off) : nullptr; a.c1 = x1 ? x1->C : 0;
      a.gate = p<float>(t.gate); a.wp = wptr(w.w_proj); a.y = p(y.off); a.ystats = p<float>(y.slab);
      a.ldp = w.hid + w.cin;  // project and skip share one K-concatenated matrix (model.cpp)
      timed(LLIE_K_DW, ((int64_t)M * w.hid * 45 / 32 +(int64_t)M * (w.cin + w.cout) + (int64_t)w.cout * (w.hid + w.cin)) * (int64_t)es(),
            [&] { return launch_dwconv3x3_project(dt, a, w.cout, s); });
    }
    rel(t.h1.off); rel(t.as2); rel(t.ab2); rel(t.gate);
    return y;
  }

  // InvertedResidualBlock.forward (efficient_unet.py:203-236) in the form irb_path picks (engine.h): 7 launches unfused
  Tens irb(const IrbW& w, const Tens& x0, const Tens* x1, const float* film, int64_t film_stride) {
    const int P = x0.H * x0.W;
    const IrbPath path = irb_path(dt, w, x0.C, x0.H, x0.W, tape != nullptr);
    IrbRec rec{};
    IrbTmp t;  // what the stages hand on
    snprintf(tag, sizeof tag, "irb P=%d %d->%d hid=%d", P, w.cin, w.cout, w.hid);
    gn(x0, x1, w.n1g, w.n1b, nullptr, 0, t.as1, t.ab1, &rec.n1, path.s6 ? 1.f / 6.f : 0.f);
    const float* film2 = film ? film + w.film_off : nullptr;  // this block's rows of the FiLM projection
    if (path.form == kIrbWide && path.wgram) front_wide_gram(w, x0, x1, film2, film_stride, t);
    else if (path.form == kIrbUnfused || path.form == kIrbWide) front_unfused(path, w, x0, x1, film2, film_stride, rec, t);
    else front_recompute(path, w, x0, x1, film2, film_stride, t);
    se_gate(path, w, P, t);
    Tens y = path.form == kIrbProject ? project_fused(w, x0, t) : path.form == kIrbWide ? project_wide(w, x0, x1, t) : project_gemm(w, x0, x1, t);
    if (tape) {
      rec.w = (int)(&w - c->irbs.data());
      rec.x0 = x0; rec.cat = x1 != nullptr;
      if (x1) rec.x1 = *x1;
      rec.h1 = t.h1; rec.h2 = t.h2; rec.gate = t.gate; rec.sehid = t.sehid; rec.semean = t.semean; rec.y = y;
      tape->ops.push_back({0, (int)tape->irbs.size()});
      tape->irbs.push_back(rec);
    }
    return y;
  }

  // StandardAttention.forward after the qkv projection (efficient_unet.py:345-357): the fused softmax core, then to_out with the
  // residual and the statistics slab of y in the GEMM's epilogue (the identity-residual epilogue of a block's project GEMM)
  Tens softattn_tail(const AttnW& w, const Tens& x, size_t qkv, AttnRec& rec) {
    const int H = x.H, W = x.W, N = H * W, M = B * N;
    const size_t ao = ar->alloc((size_t)M * w.inner * es());
    const size_t lse = tape ? ar->alloc((size_t)B * w.heads * N * 4) : 0;  // only the backward pass reads it
    if (!dry) {
      SoftAttnArgs a{};
      a.qkv = p(qkv); a.out = p(ao); a.lse = tape ? p<float>(lse) : nullptr; a.B = B; a.N = N; a.heads = w.heads;
      timed(LLIE_K_OTHER, (int64_t)M * 4 * w.inner * (int64_t)es(), [&] { return launch_softattn_fwd(dt, a, s); });
    }
    rel(qkv);
    Tens y = new_tens(x.C, H, W, pw_gemm_ntiles(N));
    if (!dry) {
      GemmArgs g = gemm1(GemmSeg{p(ao), w.inner, nullptr, nullptr, 0, ACT_NONE}, wptr(w.w_out), p(y.off), p<float>(y.slab), M, x.C, w.inner, N);
      g.res = p(x.off);
      timed(LLIE_K_GEMM, ((int64_t)M * (2 * x.C + w.inner) + (int64_t)w.inner * x.C) * (int64_t)es(), [&] { return launch_pw_gemm(dt, g, s); });
    }
    rel(ao);
    if (tape) {
      rec.w = (int)(&w - c->attns.data());
      rec.x = x; rec.qkv = qkv; rec.ao = ao; rec.lse = lse; rec.y = y;
      tape->ops.push_back({1, (int)tape->attns.size()});
      tape->attns.push_back(rec);
    }
    return y;
  }

  // LinearAttention.forward (efficient_unet.py:273-308); StandardAttention (:336-357) shares the norm and the qkv projection
  Tens attn(const AttnW& w, const Tens& x) {
    const int H = x.H, W = x.W, N = H * W, M = B * N;
    size_t as, ab;
    AttnRec rec{};
    snprintf(tag, sizeof tag, "attn N=%d C=%d", N, x.C);
    gn(x, nullptr, w.ng, w.nb, nullptr, 0, as, ab, &rec.n1);
    const size_t qkv = ar->alloc((size_t)M * 3 * w.inner * es());
    if (!dry) {
      const GemmArgs g = gemm1(GemmSeg{p(x.off), x.C, p<float>(as), p<float>(ab), x.C, ACT_NONE}, wptr(w.w_qkv), p(qkv), nullptr, M, 3 * w.inner, x.C, N);
      timed(LLIE_K_GEMM, ((int64_t)M * (x.C + 3 * w.inner) + 3LL * w.inner * x.C) * (int64_t)es(), [&] { return launch_pw_gemm(dt, g, s); });
    }
    rel(as); rel(ab);
    if (w.soft) return softattn_tail(w, x, qkv, rec);
    const int nsplit = linattn_nsplit(N);
    const size_t kv = ar->alloc((size_t)nsplit * B * w.heads * 32 * 33 * 4);
    const size_t ao = ar->alloc((size_t)M * w.inner * es());
    if (!dry) {
      AttnArgs a{};
      a.qkv = p(qkv); a.B = B; a.N = N; a.heads = w.heads; a.kv = p<float>(kv); a.out = p(ao); a.nsplit = nsplit;
      timed(LLIE_K_OTHER, (int64_t)M * 2 * w.inner * (int64_t)es(), [&] { return launch_linattn_kv(dt, a, s); }, "linattn_kv_kernel");
      timed(LLIE_K_OTHER, (int64_t)M * 2 * w.inner * (int64_t)es(), [&] { return launch_linattn_out(dt, a, s); }, "linattn_out_kernel");
    }
    rel(qkv); rel(kv);
    Tens tmp = new_tens(x.C, H, W, pw_gemm_ntiles(N));
    if (!dry) {
      const GemmArgs g = gemm1(GemmSeg{p(ao), w.inner, nullptr, nullptr, 0, ACT_NONE}, wptr(w.w_out), p(tmp.off), p<float>(tmp.slab), M, x.C, w.inner, N);
      timed(LLIE_K_GEMM, ((int64_t)M * (x.C + w.inner) + (int64_t)w.inner * x.C) * (int64_t)es(), [&] { return launch_pw_gemm(dt, g, s); });
    }
    rel(ao);
    size_t as2, ab2;
    gn(tmp, nullptr, w.n2g, w.n2b, nullptr, 0, as2, ab2, &rec.n2);
    Tens y = new_tens(x.C, H, W, (N + kAffineTileRows - 1) / kAffineTileRows);
    if (!dry) {
      AffineAddArgs a{};
      a.x = p(tmp.off); a.as = p<float>(as2); a.ab = p<float>(ab2); a.res = p(x.off); a.y = p(y.off);
      a.stats = p<float>(y.slab); a.M = M; a.C = x.C; a.P = N;
      timed(LLIE_K_OTHER, 3LL * M * x.C * (int64_t)es(), [&] { return launch_affine_add(dt, a, s); }, "affine_add_kernel");
    }
    free_tens(tmp);
    rel(as2); rel(ab2);
    if (tape) {
      rec.w = (int)(&w - c->attns.data());
      rec.x = x; rec.qkv = qkv; rec.kv = kv; rec.ao = ao; rec.nsplit = nsplit; rec.tmp = tmp; rec.y = y;
      tape->ops.push_back({1, (int)tape->attns.size()});
      tape->attns.push_back(rec);
    }
    return y;
  }

  Tens conv3(const ConvW& w, const Tens& x, int mode) {
    const int Ho = mode == 0 ? x.H / 2 : x.H * 2, Wo = mode == 0 ? x.W / 2 : x.W * 2;
    // up-sampling convs of an inference forward run from the folded weights wherever the rule of engine.h says so
    // (nine tap maps first, then the folded weights)
    const bool maps = mode == 1 && !tape && w.c == w.c_r && upconv_maps_supported(dt, x.H, x.W, w.c);
    const bool fold = !maps && mode == 1 && !tape && w.has_fold && upconv_fold_supported(dt, x.H, x.W, w.c);
    Tens y = new_tens(w.c, Ho, Wo, fold ? conv3x3_upfold_ntiles(Ho, Wo) : conv3x3_ntiles(Ho, Wo), w.c_r);
    Tens u;
    snprintf(tag, sizeof tag, "conv3 mode=%d C=%d %dx%d", mode, w.c, x.H, x.W);
    if (tape && mode == 1) {
      // training: keep the upsampled tensor (the weight gradient reads it) and run the plain stride-1 conv on it
      u.C = w.c; u.H = Ho; u.W = Wo; u.valid = true;
      u.off = ar->alloc((size_t)B * Ho * Wo * w.c * es());
    }
    if (!dry) {
      const Tens& in = u.valid ? u : x;
      Conv3Args a{};
      a.in = p(in.off); a.w = wptr(w.w); a.bias = wptr<float>(w.bias); a.out = p(y.off); a.stats = p<float>(y.slab);
      a.B = B; a.Hi = in.H; a.Wi = in.W; a.Cin = w.c; a.Cout = w.c; a.mode = u.valid ? 2 : mode;
      if (u.valid) {
        chk(launch_upsample2x(dt, p(x.off), p(u.off), B, x.H, x.W, w.c, s));
        timed(LLIE_K_CONV3, (2LL * B * w.c * Ho * Wo + 9LL * w.c * w.c) * (int64_t)es(), [&] { return launch_conv3x3(dt, a, s); });
      } else {
        a.nt = nt_store(16, (int64_t)B * Ho * Wo * w.c);
        if (fold) a.w = wptr(w.w_fold);
        // the algorithmic bytes charge the 9 C^2 source weights in either form (the folded blob is 64 C^2)
        timed(LLIE_K_CONV3, ((int64_t)B * w.c * ((int64_t)x.H * x.W + (int64_t)Ho * Wo) + 9LL * w.c * w.c) * (int64_t)es(),
              [&] { return maps ? launch_conv3x3_upmaps(dt, a, s) : (fold ? launch_conv3x3_upfold(dt, a, s) : launch_conv3x3(dt, a, s)); });
      }
    }
    if (tape) {
      ConvRec rec{};
      rec.w = mode == 0 ? (int)(&w - c->downs.data()) : (int)(&w - c->ups.data());
      rec.up = mode != 0; rec.x = x; rec.u = u; rec.y = y;
      tape->ops.push_back({2, (int)tape->convs.size()});
      tape->convs.push_back(rec);
    }
    return y;
  }

  Tens run_blocks(const std::vector<Block>& blocks, Tens h, const Tens* cat, const float* film, int64_t fstride,
                  bool keep_input) {
    bool first = true;
    for (const Block& b : blocks) {
      Tens y = b.kind == 0 ? irb(c->irbs[b.idx], h, first ? cat : nullptr, film, fstride) : attn(c->attns[b.idx], h);
      if (!(first && keep_input)) free_tens(h);
      h = y;
      first = false;
    }
    return h;
  }

  // EfficientUNet.forward (efficient_unet.py:532-606) on H x W maps: the network is fully convolutional, so the module tree that
  // image_size fixed (attention placement) runs at any frame frame_shape_ok accepts; H = W = image_size is the reference's call
  // `fs` (optional): scheduler step fused into the final conv's epilogue (2-byte compute dtypes only)
  void unet(const float* lat, const float* cond, const int64_t* t, int uniform_t, float* eps, int H, int W, const FusedStep* fs = nullptr) {
    const llie_config& g = c->cfg;
    const int T = g.time_embed_dim, F = c->film_rows;
    const int rows = uniform_t ? 1 : B;
    zbegin(H, W, [&](Run& d) { d.unet(nullptr, nullptr, nullptr, uniform_t, nullptr, H, W); });
    const size_t temb = ar->alloc((size_t)rows * T * 4), stemb = ar->alloc((size_t)rows * T * 4);
    const size_t film = ar->alloc((size_t)rows * F * 4);
    if (!dry) {
      TimeArgs ta{};
      ta.t = t; ta.rows = rows; ta.dim = g.base_channels; ta.freqs = wptr<float>(c->freqs); ta.T = T;
      ta.w1 = wptr<float>(c->t_w1); ta.b1 = wptr<float>(c->t_b1); ta.w3 = wptr<float>(c->t_w3); ta.b3 = wptr<float>(c->t_b3);
      ta.temb = p<float>(temb); ta.silu_temb = p<float>(stemb);
      snprintf(tag, sizeof tag, "time");
      timed(LLIE_K_OTHER, 0, [&] { return launch_time_embed(ta, s); }, "time_embed_kernel");
      const FilmArgs fa = film_args(stemb, rows, T, c->film_w, c->film_b, film, F);
      timed(LLIE_K_OTHER, (int64_t)F * T * 4, [&] { return launch_film(fa, s); }, "film_kernel");
    }
    const float* filmp = p<float>(film);
    const int64_t fstride = uniform_t ? 0 : F;

    Tens h = new_tens(c->channels[0], H, W, init_conv_ntiles(H, W, dt != LLIE_F32), c->channels_r[0]);
    if (!dry) {
      InitConvArgs a{};
      const int half = g.in_channels / 2;
      a.x0 = lat; a.x1 = cond; a.c0 = half; a.c1 = g.in_channels - half;
      a.w = wptr<float>(c->init_w); a.bias = wptr<float>(c->init_b); a.out = p(h.off); a.stats = p<float>(h.slab);
      a.wp = dt != LLIE_F32 ? wptr(c->init_wp) : nullptr;
      a.B = B; a.H = H; a.W = W; a.Cout = c->channels[0];
      snprintf(tag, sizeof tag, "init_conv");
      timed(LLIE_K_OTHER, (int64_t)B * H * W * (g.in_channels * 4 + c->channels[0] * (int64_t)es()), [&] { return launch_init_conv(dt, a, s); }, "init_conv_kernel");
    }
    if (tape) {
      tape->temb = temb; tape->stemb = stemb; tape->film = film; tape->h0 = h;
      tape->lat = lat; tape->cond = cond; tape->t = t; tape->B = B; tape->H = H; tape->W = W;
    }
    Tens skips[4];
    for (int l = 0; l < 4; ++l) {
      h = run_blocks(c->enc[l], h, nullptr, filmp, fstride, false);
      skips[l] = h;  // one skip per level, taken before the downsample (:567)
      if (l < 3) h = conv3(c->downs[l], h, 0);  // the skip stays alive
    }
    // level 3: h aliases skips[3]; mid_block1 must not free it
    h = run_blocks(c->mid, h, nullptr, filmp, fstride, true);
    for (int l = 0; l < 4; ++l) {
      if (l > 0) {
        Tens u = conv3(c->ups[l - 1], h, 1);
        free_tens(h);
        h = u;
      }
      Tens y = run_blocks(c->dec[l], h, &skips[3 - l], filmp, fstride, false);  // cat([h, skip]) (:588)
      free_tens(skips[3 - l]);
      h = y;
    }
    size_t as, ab;
    GnRec finrec{};
    snprintf(tag, sizeof tag, "final_norm");
    gn(h, nullptr, c->fin_g, c->fin_b, nullptr, 0, as, ab, &finrec);
    if (tape) { tape->fin = finrec; tape->hlast = h; }
    if (!dry) {
      FinalConvArgs a{};
      a.in = p(h.off); a.as = p<float>(as); a.ab = p<float>(ab); a.w = wptr<float>(c->fin_w); a.bias = wptr<float>(c->fin_bias);
      a.out = eps; a.B = B; a.H = H; a.W = W; a.C = c->channels[0]; a.Cout = g.out_channels;
      a.wp = dt != LLIE_F32 ? wptr(c->fin_wp) : nullptr;
      if (fs) {
        a.fuse_step = 1; a.coef = fs->coef; a.sample = lat; a.noise = fs->noise; a.prev = fs->prev; a.clamped = fs->clamped;
      }
      snprintf(tag, sizeof tag, "final_conv");
      timed(LLIE_K_OTHER, (int64_t)B * H * W * (c->channels[0] * (int64_t)es() + 3 * 4 * (fs ? 4 : 1)), [&] { return launch_final_conv(dt, a, s); }, "final_conv_kernel");
    }
    free_tens(h);
    rel(as); rel(ab);
    rel(temb); rel(stemb); rel(film);
  }

  // single-operator forward: fp32 NCHW in/out
  void module(const float* x, const float* temb, float* y, int H, int W) {
    const llie_config& g = c->cfg;
    const int P = H * W;
    const int split = (g.kind == LLIE_IRB) ? g.base_channels : 0;  // IRB: optional virtual-concat split point
    zbegin(H, W, [&](Run& d) { d.module(nullptr, nullptr, nullptr, H, W); });
    const int xt = (P + 63) / 64;  // tiles of the conversion's statistics slab (P is a multiple of 64 for every kind but LLIE_SOFTATTN)
    Tens x0 = new_tens(split ? split : g.in_channels, H, W, xt);
    Tens x1;
    if (split) x1 = new_tens(g.in_channels - split, H, W, xt);
    if (!dry) {
      chk(launch_nchw_to_nhwc(dt, x, p(x0.off), p<float>(x0.slab), B, x0.C, P, g.in_channels, 0, s));
      if (split) chk(launch_nchw_to_nhwc(dt, x, p(x1.off), p<float>(x1.slab), B, x1.C, P, g.in_channels, split, s));
    }
    Tens out;
    if (g.kind == LLIE_IRB) {
      const int T = g.time_embed_dim, F = c->film_rows;
      const size_t st = ar->alloc((size_t)B * T * 4), film = ar->alloc((size_t)B * F * 4);
      if (!dry) {
        chk(launch_silu_rows(temb, p<float>(st), (int64_t)B * T, s));
        chk(launch_film(film_args(st, B, T, c->film_w, c->film_b, film, F), s));
      }
      out = irb(c->irbs[0], x0, split ? &x1 : nullptr, p<float>(film), F);
      rel(st); rel(film);
      if (tape) { tape->stemb = st; tape->film = film; }
    } else if (g.kind == LLIE_ATTN || g.kind == LLIE_SOFTATTN) {
      out = attn(c->attns[0], x0);
    } else if (g.kind == LLIE_SE) {
      // SqueezeExcitation.forward (efficient_unet.py:96-100): the 64-pixel (sum, sum of squares) slab of the layout
      // conversion doubles as the pool partials (every second entry), then the block's own SE kernels and x * gate
      const IrbW& w = c->irbs[0];
      const int C = w.hid;
      const size_t sehid = ar->alloc((size_t)B * w.sq * 4), gate = ar->alloc((size_t)B * C * 4);
      const size_t semean = ar->alloc((size_t)B * C * 4), zero = ar->alloc((size_t)B * C * 4);
      out = new_tens(C, H, W, P / kAffineTileRows);
      if (!dry) {
        SeArgs e = se_args(w, P, semean, sehid, gate);
        e.pool = p<float>(x0.slab); e.ntiles = P / 64; e.pool_stride = 2 * C;
        chk(launch_se_fc1(dt, e, s));
        chk(launch_se_fc2(dt, e, s));
        chk(launch_fill_zero(p(zero), (int64_t)B * C * 4, s));
        AffineAddArgs a{};
        a.x = p(x0.off); a.as = p<float>(gate); a.ab = p<float>(zero); a.res = nullptr; a.y = p(out.off);
        a.stats = p<float>(out.slab); a.M = B * P; a.C = C; a.P = P;
        chk(launch_affine_add(dt, a, s));
      }
      rel(sehid); rel(gate); rel(semean); rel(zero);
    } else if (g.kind == LLIE_DOWN) {
      out = conv3(c->downs[0], x0, 0);
    } else {
      out = conv3(c->ups[0], x0, 1);
    }
    if (!dry && y) chk(launch_nhwc_to_nchw(dt, p(out.off), y, B, out.C, out.H * out.W, s));
    if (tape) { tape->h0 = x0; tape->x1 = x1; tape->hlast = out; tape->B = B; }
    free_tens(out);
    free_tens(x0);
    free_tens(x1);
  }
};


}  // namespace

int llie::run_unet(Exec x, Tape* tape, const float* lat, const float* cond, const int64_t* t, float* eps, int H, int W) {
  Run r{x};
  r.tape = tape;
  r.unet(lat, cond, t, 0, eps, H, W);
  return r.rc();
}
int llie::run_module(Exec x, Tape* tape, const float* in, const float* temb, float* y, int H, int W) {
  Run r{x};
  r.tape = tape;
  r.module(in, temb, y, H, W);
  return r.rc();
}

// The forward's plan as every workspace query of a UNet handle counts it: per-sample timesteps.  One dry run per batch, frame
// and knob epoch (the key of llie_ctx::zneed, for the same reason: the knobs bake kernel choices into the plan)
static size_t query_plan(llie_ctx* c, int batch, int H, int W) {
  const auto key = std::make_tuple(batch, H, W, g_knobs.epoch);
  auto it = c->qplan.find(key);
  if (it == c->qplan.end())
    it = c->qplan.emplace(key, Run::plan(c, batch, [&](Run& d) { d.unet(nullptr, nullptr, nullptr, 0, nullptr, H, W); })).first;
  return it->second;
}

int llie::unet_forward_impl(llie_ctx* c, const float* lat, const float* cond, const int64_t* t, int uniform_t, float* eps,
                            const FusedStep* fs, int batch, int H, int W, void* ws, int64_t ws_bytes, llie_stream stream, size_t reserve) {
  if (!c || !lat || !cond || !t || (!eps && !fs) || !ws || batch <= 0 || c->cfg.kind != LLIE_UNET) return LLIE_ERR_ARG;
  int rc = check_ready(c);
  if (rc) return rc;
  // Too small is what is smaller than the queries answered, and they plan per-sample timesteps: a forward with equal timesteps
  // (one row of time tables) would run in a few bytes less, but no query says how many, so it is held to the same figure
  size_t need = query_plan(c, batch, H, W);
  if (uniform_t) need = std::max(need, Run::plan(c, batch, [&](Run& d) { d.unet(nullptr, nullptr, nullptr, uniform_t, nullptr, H, W); }));
  rc = fits(need + reserve, ws_bytes);
  if (rc) return rc;
  Arena ar((size_t)ws_bytes);
  Run r{Exec::live(c, &ar, stream, ws, batch)};
  r.unet(lat, cond, t, uniform_t, eps, H, W, fs);
  return r.rc();
}

// The widest tensor one forward stores at full resolution, in channels: what the element cap of frame_shape_ok multiplies
int llie::widest_full_res_channels(const llie_ctx* c) {
  int m = std::max(c->channels[0], c->cfg.in_channels);
  for (const std::vector<Block>* blocks : {&c->enc[0], &c->dec[3]})
    for (const Block& b : *blocks) {
      if (b.kind == 0) m = std::max({m, c->irbs[b.idx].cin, c->irbs[b.idx].hid, c->irbs[b.idx].cout});
      else m = std::max({m, c->attns[b.idx].c, 3 * c->attns[b.idx].inner});
    }
  return m;
}

int llie::frame_shape_ok(const llie_ctx* c, int batch, int H, int W) {
  if (!c || c->cfg.kind != LLIE_UNET || batch <= 0) return LLIE_ERR_ARG;
  if (H % 8 || W % 8 || H < 64 || W < 64) {
    set_err("frame %dx%d: height and width must be multiples of 8 and at least 64", H, W);
    return LLIE_ERR_SHAPE;
  }
  if (batch > 65535) {
    set_err("batch %d: at most 65535 frames per call", batch);
    return LLIE_ERR_SHAPE;
  }
  const int cw = widest_full_res_channels(c);
  if ((long long)batch * H * W * cw > 2147483647ll) {
    set_err("frame too large: batch %d x %dx%d x %d channels exceeds the element cap 2^31 - 1; use tiles", batch, H, W, cw);
    return LLIE_ERR_SHAPE;
  }
  return LLIE_OK;
}

// one forward's plan + the latents ping-pong and eps buffers of the loop; max_steps > 0: + the staging area of its hipGraph path
// (inputs / outputs of up to `max_steps` steps with intermediates and noise predictions)
int64_t llie::frame_workspace(llie_ctx* c, int batch, int H, int W, int max_steps) {
  const size_t core = query_plan(c, batch, H, W);
  const size_t img = align_up((size_t)batch * 3 * H * W * 4, 256);
  size_t n = core + loop_image_bytes(batch, H, W);
  if (max_steps > 0) n += (2 + 3 * (size_t)max_steps) * img + align_up((size_t)max_steps * batch * 8, 256);
  return (int64_t)n;
}

extern "C" {

int64_t llie_workspace_bytes(llie_ctx* c, int batch, int height, int width) {
  if (!c || batch <= 0) return LLIE_ERR_ARG;
  if (c->cfg.kind == LLIE_UNET) return frame_workspace(c, batch, c->cfg.image_size, c->cfg.image_size, 0);
  if (shape_ok(c, height, width) != LLIE_OK) return LLIE_ERR_SHAPE;
  return (int64_t)Run::plan(c, batch, [&](Run& d) { d.module(nullptr, nullptr, nullptr, height, width); });
}

// Workspace for llie_enhance with room for the hipGraph staging area
int64_t llie_enhance_workspace_bytes(llie_ctx* c, int batch, int max_steps) {
  if (!c || batch <= 0 || max_steps <= 0 || c->cfg.kind != LLIE_UNET) return LLIE_ERR_ARG;
  return frame_workspace(c, batch, c->cfg.image_size, c->cfg.image_size, max_steps);
}

int llie_frame_shape_ok(const llie_ctx* c, int batch, int height, int width) { return frame_shape_ok(c, batch, height, width); }

// the pixel count the element cap of frame_shape_ok leaves a frame of a batch: floor((2^31 - 1) / (batch * Cmax))
int64_t llie_frame_max_pixels(const llie_ctx* c, int batch) {
  if (!c || c->cfg.kind != LLIE_UNET || batch <= 0) return LLIE_ERR_ARG;
  return 2147483647ll / ((long long)batch * widest_full_res_channels(c));
}

int64_t llie_frame_workspace_bytes(llie_ctx* c, int batch, int height, int width, int max_steps) {
  if (max_steps < 0) return LLIE_ERR_ARG;
  const int rc = frame_shape_ok(c, batch, height, width);
  return rc ? rc : frame_workspace(c, batch, height, width, max_steps);
}

int llie_unet_forward(llie_ctx* c, const float* lat, const float* cond, const int64_t* t, int uniform_t, float* eps,
                      int batch, void* ws, int64_t ws_bytes, llie_stream stream) {
  if (!eps || !c) return LLIE_ERR_ARG;
  const int S = c->cfg.image_size;
  return unet_forward_impl(c, lat, cond, t, uniform_t, eps, nullptr, batch, S, S, ws, ws_bytes, stream, loop_image_bytes(batch, S, S));
}

int llie_unet_forward_hw(llie_ctx* c, const float* lat, const float* cond, const int64_t* t, int uniform_t, float* eps,
                         int batch, int height, int width, void* ws, int64_t ws_bytes, llie_stream stream) {
  if (!eps) return LLIE_ERR_ARG;
  const int rc = frame_shape_ok(c, batch, height, width);
  return rc ? rc : unet_forward_impl(c, lat, cond, t, uniform_t, eps, nullptr, batch, height, width, ws, ws_bytes, stream,
                                     loop_image_bytes(batch, height, width));
}

int llie_module_forward(llie_ctx* c, const float* x, const float* temb, float* y, int batch, int H, int W, void* ws,
                        int64_t ws_bytes, llie_stream stream) {
  if (!c || !x || !y || !ws || batch <= 0 || c->cfg.kind == LLIE_UNET) return LLIE_ERR_ARG;
  if (c->cfg.kind == LLIE_IRB && !temb) return LLIE_ERR_ARG;
  int rc = check_ready(c);
  if (rc) return rc;
  rc = shape_ok(c, H, W);
  if (rc) return rc;
  rc = fits(Run::plan(c, batch, [&](Run& d) { d.module(nullptr, nullptr, nullptr, H, W); }), ws_bytes);
  if (rc) return rc;
  Arena ar((size_t)ws_bytes);
  return run_module(Exec::live(c, &ar, stream, ws, batch), nullptr, x, temb, y, H, W);
}

}  // extern "C"
