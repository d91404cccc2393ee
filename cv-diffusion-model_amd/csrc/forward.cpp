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
  // launch order; its size comes from a counting dry run of the same forward (cached per batch and image size).
  size_t zoff = 0, zcur = 0, zcap = 0;
  bool zcount = false;
  template <typename F> void zbegin(int64_t pixels, F&& forward_again) {
    if (tape || zcount) return;
    const auto key = std::make_tuple(B, pixels, g_knobs.epoch);
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

  // InvertedResidualBlock.forward (efficient_unet.py:203-236) as 7 launches.
  Tens irb(const IrbW& w, const Tens& x0, const Tens* x1, const float* film, int64_t film_stride) {
    const int H = x0.H, W = x0.W, P = H * W, M = B * P;
    size_t as1, ab1;
    IrbRec rec{};
    snprintf(tag, sizeof tag, "irb P=%d %d->%d hid=%d", P, w.cin, w.cout, w.hid);
    // 2-byte inference engines carry norm1's ReLU6 as clamp01(z / 6): the tables come out divided by 6 and the expand
    // GEMM (or the recompute kernels) puts the 6 back (kernels.h: ACT_RELU6_S6).  Training keeps the plain tables.
    const bool s6 = !tape && dt != LLIE_F32;
    gn(x0, x1, w.n1g, w.n1b, nullptr, 0, as1, ab1, &rec.n1, s6 ? 1.f / 6.f : 0.f);
    // Recompute form (2-byte T, narrow inputs): a statistics-only expand pass, then the fused expand + depthwise kernel
    // rebuilds h1 on the fly, so the 4x-expanded tensor never touches HBM (irbx.hip).
    const bool fusedx = !tape && g_knobs.use_irbx && w.hid == w.hid_r && w.cin == w.cin_r &&
                        irbx_supported(dt, w.cin, x0.C, w.hid, H, W);
    // K1: expand with norm1 + ReLU6 prologue
    Tens h1;
    h1.C = w.hid; h1.Cr = w.hid_r; h1.H = H; h1.W = W; h1.ntiles = fusedx ? P / irbx_stats_rows(P) : pw_gemm_ntiles(P); h1.valid = true;
    h1.off = fusedx ? 0 : ar->alloc((size_t)B * P * w.hid * es());
    // norm2's statistics of the recompute form: from the Gram matrix of the activated input (gram.hip) -- the statistics
    // pass is then a plain read of x -- or, knob "gram" = 0, from a second run of the expand GEMM (expand_stats)
    // (from 32 768 pixels per image on: below, the workgroup epilogue and the last-ticket sum outweigh the saved MFMAs --
    // measured at B = 1 and B = 32; the rule must not depend on the batch, it fixes the statistics' summation order)
    const bool gram = fusedx && g_knobs.gram && (P >= 32768 || g_knobs.gram > 1) && gram_supported(dt, w.cin, x0.C, P);
    h1.slab = gram ? 0 : ar->alloc((size_t)B * h1.ntiles * 2 * w.hid * 4);
    const size_t gpart = gram ? ar->alloc((size_t)B * gram_part_floats(w.cin, P) * 4) : 0;
    const size_t gtot = gram ? ar->alloc((size_t)B * (w.cin * w.cin + w.cin) * 4) : 0;
    const size_t gtick = gram ? ztake((size_t)B * 4) : 0;
    IrbxArgs xa{};
    if (fusedx && !dry) {
      xa.x0 = p(x0.off); xa.c0 = x0.C; xa.x1 = x1 ? p(x1->off) : nullptr; xa.c1 = x1 ? x1->C : 0;
      xa.as1 = p<float>(as1); xa.ab1 = p<float>(ab1); xa.w1 = wptr(w.w_expand); xa.wd = wptr<float>(w.w_dw);
      xa.stats = gram ? nullptr : p<float>(h1.slab); xa.B = B; xa.H = H; xa.W = W; xa.Chid = w.hid;
      if (gram) {
        GramArgs ga{};
        ga.x0 = xa.x0; ga.x1 = xa.x1; ga.c0 = xa.c0; ga.c1 = xa.c1; ga.as1 = xa.as1; ga.ab1 = xa.ab1;
        ga.part = p<float>(gpart); ga.gtot = p<float>(gtot); ga.tickets = p<unsigned int>(gtick); ga.B = B; ga.P = P;
        timed(LLIE_K_GEMM, (int64_t)M * w.cin * (int64_t)es(), [&] { return launch_gram_stats(dt, ga, s); });
      } else {
        timed(LLIE_K_GEMM, ((int64_t)M * w.cin + (int64_t)w.hid * w.cin) * (int64_t)es(), [&] { return launch_expand_stats(dt, xa, s); });
      }
    } else if (!dry) {
      GemmArgs g{};
      const int act1 = s6 ? ACT_RELU6_S6 : ACT_RELU6;
      g.seg[0] = GemmSeg{p(x0.off), x0.C, p<float>(as1), p<float>(ab1), w.cin, act1};
      g.nseg = 1;
      if (x1) {
        g.seg[1] = GemmSeg{p(x1->off), x1->C, p<float>(as1) + x0.C, p<float>(ab1) + x0.C, w.cin, act1};
        g.nseg = 2;
      }
      g.w = wptr(w.w_expand); g.out = p(h1.off); g.stats = p<float>(h1.slab);
      g.M = M; g.N = w.hid; g.K = w.cin; g.P = P;
      const int64_t kbytes = ((int64_t)M * (w.cin + w.hid) + (int64_t)w.hid * w.cin) * (int64_t)es();
      if (s6 && w.has_wf && pw_expand_supported(dt, g.seg, g.nseg, M, w.hid, w.cin, P)) {
        // activation-stationary form: pixels activated once and held in registers, packed weights streamed (pwx.hip)
        ExpandArgs x{};
        for (int i = 0; i < g.nseg; ++i) x.seg[i] = g.seg[i];
        x.nseg = g.nseg; x.wf = wptr(w.w_expand_f); x.out = g.out; x.stats = g.stats;
        x.M = M; x.N = w.hid; x.K = w.cin; x.P = P;
        x.nt = nt_store(2, (int64_t)M * w.hid);
        timed(LLIE_K_GEMM, kbytes, [&] { return launch_pw_expand(dt, x, s); });
      } else {
        if (s6) g.nt = nt_store(2, (int64_t)M * w.hid);
        timed(LLIE_K_GEMM, kbytes, [&] { return launch_pw_gemm(dt, g, s); });
      }
    }
    // norm2 + FiLM folded into one affine
    size_t as2, ab2;
    // unfused depthwise of a 2-byte inference engine: tables / 6 and clamp01 in its prologue too (DwArgs::s6); the
    // recompute kernel takes the plain tables (it rescales the shift itself: its accumulators are already / 6)
    const bool s6dw = s6 && !fusedx;
    if (gram) {
      as2 = ar->alloc((size_t)B * w.hid * 4);
      ab2 = ar->alloc((size_t)B * w.hid * 4);
      if (!dry) {
        GramFinalizeArgs fa{};
        fa.gtot = p<float>(gtot); fa.w1 = wptr(w.w_expand); fa.K = w.cin; fa.Chid = w.hid; fa.groups = gn_groups(w.hid); fa.P = P; fa.B = B;
        fa.gamma = wptr<float>(w.n2g); fa.beta = wptr<float>(w.n2b);
        fa.film = film ? film + w.film_off : nullptr; fa.film_stride = film_stride; fa.eps = 1e-5f;
        fa.as = p<float>(as2); fa.ab = p<float>(ab2); fa.post_scale = 0.f;
        timed(LLIE_K_OTHER, (int64_t)B * w.hid * 8, [&] { return launch_gram_finalize(dt, fa, s); }, "gram_finalize_kernel");
      }
      rel(gpart);
    } else {
      gn(h1, nullptr, w.n2g, w.n2b, film ? film + w.film_off : nullptr, film_stride, as2, ab2, &rec.n2, s6dw ? 1.f / 6.f : 0.f);
    }
    // K2: depthwise with affine + ReLU6 prologue and SE pool partials
    const int dnt = fusedx ? irbx_pool_tiles(H, W) : dwconv_ntiles(H, W);
    // Identity-residual recompute blocks and the 96 -> 32 skip-conv block go without h2 too: the SE pool totals come from a pass
    // that only rebuilds h1 (expand_pool), and once the gate is known expand_dw_project multiplies the depthwise result by Wp
    // itself and adds the shortcut.  A rule on the layer alone (irb_project_form) -- never on the batch or the grid, which would
    // break batch invariance.
    const bool fusedp = fusedx && irb_project_form(dt, w, x0.C, H, W) != 0;
    const size_t h2 = fusedp ? 0 : ar->alloc((size_t)M * w.hid * es());
    // SE pool: inference adds fixed-point channel totals into the zeroed region (one gate kernel follows); training keeps
    // the slab of tile partials (the backward pass and the 3-launch SE path read it)
    const bool fixtot = !tape && w.hid % 128 == 0;
    const size_t pool = fixtot ? 0 : ar->alloc((size_t)B * dnt * w.hid * 4);
    const size_t ptot = fixtot ? ztake((size_t)B * w.hid * 8) : 0;
    if (!dry) {
      if (fusedp) {
        xa.as2 = p<float>(as2); xa.ab2 = p<float>(ab2); xa.pool_tot = p<unsigned long long>(ptot);
        timed(LLIE_K_DW, ((int64_t)M * w.cin + (int64_t)w.hid * w.cin) * (int64_t)es(), [&] { return launch_expand_pool(dt, xa, s); });
      } else if (fusedx) {
        xa.as2 = p<float>(as2); xa.ab2 = p<float>(ab2); xa.out = p(h2);
        xa.pool = fixtot ? nullptr : p<float>(pool);
        xa.pool_tot = fixtot ? p<unsigned long long>(ptot) : nullptr;
        xa.nt = w.cin <= 64 ? nt_store(1, (int64_t)M * w.hid) : 0;  // 96 -> 384: the kernel itself loses more than its consumer gains
        timed(LLIE_K_DW, (int64_t)M * (w.cin + w.hid) * (int64_t)es(), [&] { return launch_expand_dw(dt, xa, s); });
      } else {
        DwArgs d{};
        d.in = p(h1.off); d.out = p(h2); d.as = p<float>(as2); d.ab = p<float>(ab2);
        d.w = wptr<float>(w.w_dw); d.pool = fixtot ? nullptr : p<float>(pool);
        d.pool_tot = fixtot ? p<unsigned long long>(ptot) : nullptr; d.B = B; d.H = H; d.W = W; d.C = w.hid; d.s6 = s6dw ? 1 : 0;
        d.nt = nt_store(4, (int64_t)M * w.hid);
        timed(LLIE_K_DW, 2LL * M * w.hid * (int64_t)es(), [&] { return launch_dwconv3x3(dt, d, s); });
      }
    }
    if (!fusedp) { rel(as1); rel(ab1); }  // expand_dw_project applies both norms again
    if (!fusedx) rel(h1.off);
    if (gram) rel(gtot); else rel(h1.slab);
    if (!fusedp) { rel(as2); rel(ab2); }
    // SE MLP
    // (wide blocks of the 2-byte inference engines: fc1's pre-activations accumulate as integers in the zero-initialised region)
    const bool sepre_ok = fixtot && dt != LLIE_F32 && g_knobs.se_mfma && w.hid >= 768 && w.hid % 256 == 0 && w.sq % 64 == 0 && w.sq <= 512;
    const size_t sepre = sepre_ok ? ztake((size_t)B * w.sq * 8) : 0;
    const size_t sehid = ar->alloc((size_t)B * w.sq * 4), gate = ar->alloc((size_t)B * w.hid * 4);
    const size_t semean = ar->alloc((size_t)B * w.hid * 4);
    if (!dry) {
      SeArgs e{};
      e.pool = fixtot ? nullptr : p<float>(pool); e.ntiles = dnt; e.P = P;
      e.w1 = wptr(w.se_w1); e.b1 = wptr<float>(w.se_b1); e.w2 = wptr(w.se_w2); e.b2 = wptr<float>(w.se_b2);
      e.mean = p<float>(semean); e.hid = p<float>(sehid); e.gate = p<float>(gate); e.B = B; e.C = w.hid; e.Cs = w.sq;
      if (fixtot) e.tot = p<unsigned long long>(ptot);
      if (sepre_ok) e.pre = p<long long>(sepre);
      if (sepre_ok && g_knobs.se_mfma && se_mlp_mfma_supported(dt, e)) {
        timed(LLIE_K_SE, (int64_t)B * w.hid * 12 + 2LL * w.hid * w.sq * (int64_t)es(), [&] { return launch_se_mlp_mfma(dt, e, s); });
      } else if (fixtot && w.hid <= 384) {
        timed(LLIE_K_SE, (int64_t)B * w.hid * 12 + 2LL * w.hid * w.sq * (int64_t)es(), [&] { return launch_se_gate(dt, e, s); });
      } else timed(LLIE_K_SE, ((int64_t)B * dnt * w.hid * 4) + 2LL * w.hid * w.sq * (int64_t)es(), [&] {
        hipError_t r1 = launch_se_fc1(dt, e, s);
        return r1 != hipSuccess ? r1 : launch_se_fc2(dt, e, s);
      });
    }
    if (!fixtot) rel(pool);
    rel(sehid); rel(semean);
    // K3: project with SE gate prologue (+ skip conv as extra K segments, or identity residual)
    Tens y = new_tens(w.cout, H, W, fusedp ? irbx_project_tiles(H, W) : pw_gemm_ntiles(P), w.cout_r);
    if (fusedp) {
      if (!dry) {
        xa.pool_tot = nullptr; xa.gate = p<float>(gate); xa.wp = wptr(w.w_proj); xa.y = p(y.off); xa.ystats = p<float>(y.slab);
        xa.ldp = w.hid + (w.skip ? w.cin : 0);  // project and skip share one K-concatenated matrix (model.cpp)
        timed(LLIE_K_DW, ((int64_t)M * (w.cin + w.cout) + (int64_t)w.hid * (w.cin + w.cout)) * (int64_t)es(),
              [&] { return launch_expand_dw_project(dt, xa, w.cout, w.skip, s); });
      }
      rel(as1); rel(ab1); rel(as2); rel(ab2);
    } else if (!dry) {
      GemmArgs g{};
      g.seg[0] = GemmSeg{p(h2), w.hid, p<float>(gate), nullptr, w.hid, ACT_NONE};
      g.nseg = 1;
      g.K = w.hid;
      if (w.skip) {
        g.seg[g.nseg++] = GemmSeg{p(x0.off), x0.C, nullptr, nullptr, 0, ACT_NONE};
        if (x1) g.seg[g.nseg++] = GemmSeg{p(x1->off), x1->C, nullptr, nullptr, 0, ACT_NONE};
        g.K += w.cin;
      } else {
        g.res = p(x0.off);
      }
      g.w = wptr(w.w_proj); g.out = p(y.off); g.stats = p<float>(y.slab);
      g.M = M; g.N = w.cout; g.P = P;
      g.nt = nt_store(8, (int64_t)M * w.cout);
      timed(LLIE_K_GEMM, ((int64_t)M * (g.K + w.cout + (w.skip ? 0 : w.cout)) + (int64_t)w.cout * g.K) * (int64_t)es(),
            [&] { return launch_pw_gemm(dt, g, s); });
    }
    if (!fusedp) rel(h2);
    rel(gate);
    if (tape) {
      rec.w = (int)(&w - c->irbs.data());
      rec.x0 = x0; rec.cat = x1 != nullptr;
      if (x1) rec.x1 = *x1;
      rec.h1 = h1; rec.h2 = h2; rec.gate = gate; rec.sehid = sehid; rec.semean = semean; rec.y = y;
      tape->ops.push_back({0, (int)tape->irbs.size()});
      tape->irbs.push_back(rec);
    }
    return y;
  }

  // LinearAttention.forward (efficient_unet.py:273-308)
  Tens attn(const AttnW& w, const Tens& x) {
    const int H = x.H, W = x.W, N = H * W, M = B * N;
    size_t as, ab;
    AttnRec rec{};
    snprintf(tag, sizeof tag, "attn N=%d C=%d", N, x.C);
    gn(x, nullptr, w.ng, w.nb, nullptr, 0, as, ab, &rec.n1);
    const size_t qkv = ar->alloc((size_t)M * 3 * w.inner * es());
    if (!dry) {
      GemmArgs g{};
      g.seg[0] = GemmSeg{p(x.off), x.C, p<float>(as), p<float>(ab), x.C, ACT_NONE};
      g.nseg = 1; g.w = wptr(w.w_qkv); g.out = p(qkv);
      g.M = M; g.N = 3 * w.inner; g.K = x.C; g.P = N;
      timed(LLIE_K_GEMM, ((int64_t)M * (x.C + 3 * w.inner) + 3LL * w.inner * x.C) * (int64_t)es(), [&] { return launch_pw_gemm(dt, g, s); });
    }
    rel(as); rel(ab);
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
      GemmArgs g{};
      g.seg[0] = GemmSeg{p(ao), w.inner, nullptr, nullptr, 0, ACT_NONE};
      g.nseg = 1; g.w = wptr(w.w_out); g.out = p(tmp.off); g.stats = p<float>(tmp.slab);
      g.M = M; g.N = x.C; g.K = w.inner; g.P = N;
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
    Tens y = new_tens(w.c, Ho, Wo, conv3x3_ntiles(Ho, Wo), w.c_r);
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
        chk(launch_conv3x3(dt, a, s));
      } else {
        a.nt = nt_store(16, (int64_t)B * Ho * Wo * w.c);
        timed(LLIE_K_CONV3, ((int64_t)B * w.c * ((int64_t)x.H * x.W + (int64_t)Ho * Wo) + 9LL * w.c * w.c) * (int64_t)es(),
              [&] { return launch_conv3x3(dt, a, s); });
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

  // EfficientUNet.forward (efficient_unet.py:532-606)
  // `fs` (optional): scheduler step fused into the final conv's epilogue (2-byte compute dtypes only)
  void unet(const float* lat, const float* cond, const int64_t* t, int uniform_t, float* eps, const FusedStep* fs = nullptr) {
    const llie_config& g = c->cfg;
    const int S = g.image_size, T = g.time_embed_dim, F = c->film_rows;
    const int rows = uniform_t ? 1 : B;
    zbegin((int64_t)S * S, [&](Run& d) { d.unet(nullptr, nullptr, nullptr, uniform_t, nullptr); });
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

    Tens h = new_tens(c->channels[0], S, S, init_conv_ntiles(S, S, dt != LLIE_F32), c->channels_r[0]);
    if (!dry) {
      InitConvArgs a{};
      const int half = g.in_channels / 2;
      a.x0 = lat; a.x1 = cond; a.c0 = half; a.c1 = g.in_channels - half;
      a.w = wptr<float>(c->init_w); a.bias = wptr<float>(c->init_b); a.out = p(h.off); a.stats = p<float>(h.slab);
      a.wp = dt != LLIE_F32 ? wptr(c->init_wp) : nullptr;
      a.B = B; a.H = S; a.W = S; a.Cout = c->channels[0];
      snprintf(tag, sizeof tag, "init_conv");
      timed(LLIE_K_OTHER, (int64_t)B * S * S * (g.in_channels * 4 + c->channels[0] * (int64_t)es()), [&] { return launch_init_conv(dt, a, s); }, "init_conv_kernel");
    }
    if (tape) {
      tape->temb = temb; tape->stemb = stemb; tape->film = film; tape->h0 = h;
      tape->lat = lat; tape->cond = cond; tape->t = t; tape->B = B;
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
      a.out = eps; a.B = B; a.H = S; a.W = S; a.C = c->channels[0]; a.Cout = g.out_channels;
      a.wp = dt != LLIE_F32 ? wptr(c->fin_wp) : nullptr;
      if (fs) {
        a.fuse_step = 1; a.coef = fs->coef; a.sample = lat; a.noise = fs->noise; a.prev = fs->prev; a.clamped = fs->clamped;
      }
      snprintf(tag, sizeof tag, "final_conv");
      timed(LLIE_K_OTHER, (int64_t)B * S * S * (c->channels[0] * (int64_t)es() + 3 * 4 * (fs ? 4 : 1)), [&] { return launch_final_conv(dt, a, s); }, "final_conv_kernel");
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
    zbegin((int64_t)P, [&](Run& d) { d.module(nullptr, nullptr, nullptr, H, W); });
    Tens x0 = new_tens(split ? split : g.in_channels, H, W, P / 64);
    Tens x1;
    if (split) x1 = new_tens(g.in_channels - split, H, W, P / 64);
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
    } else if (g.kind == LLIE_ATTN) {
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
        SeArgs e{};
        e.pool = p<float>(x0.slab); e.ntiles = P / 64; e.pool_stride = 2 * C; e.P = P;
        e.w1 = wptr(w.se_w1); e.b1 = wptr<float>(w.se_b1); e.w2 = wptr(w.se_w2); e.b2 = wptr<float>(w.se_b2);
        e.mean = p<float>(semean); e.hid = p<float>(sehid); e.gate = p<float>(gate); e.B = B; e.C = C; e.Cs = w.sq;
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

int llie::run_unet(Exec x, Tape* tape, const float* lat, const float* cond, const int64_t* t, float* eps) {
  Run r{x};
  r.tape = tape;
  r.unet(lat, cond, t, 0, eps);
  return r.rc();
}
int llie::run_module(Exec x, Tape* tape, const float* in, const float* temb, float* y, int H, int W) {
  Run r{x};
  r.tape = tape;
  r.module(in, temb, y, H, W);
  return r.rc();
}

int llie::unet_forward_impl(llie_ctx* c, const float* lat, const float* cond, const int64_t* t, int uniform_t, float* eps,
                            const FusedStep* fs, int batch, void* ws, int64_t ws_bytes, llie_stream stream) {
  if (!c || !lat || !cond || !t || (!eps && !fs) || !ws || batch <= 0 || c->cfg.kind != LLIE_UNET) return LLIE_ERR_ARG;
  int rc = check_ready(c);
  if (rc) return rc;
  rc = fits(Run::plan(c, batch, [&](Run& d) { d.unet(nullptr, nullptr, nullptr, uniform_t, nullptr); }), ws_bytes);
  if (rc) return rc;
  Arena ar((size_t)ws_bytes);
  Run r{Exec::live(c, &ar, stream, ws, batch)};
  r.unet(lat, cond, t, uniform_t, eps, fs);
  return r.rc();
}

extern "C" {

int64_t llie_workspace_bytes(llie_ctx* c, int batch, int height, int width) {
  if (!c || batch <= 0) return LLIE_ERR_ARG;
  if (c->cfg.kind == LLIE_UNET) {
    const size_t core = Run::plan(c, batch, [](Run& d) { d.unet(nullptr, nullptr, nullptr, 0, nullptr); });
    // + latents ping-pong and eps buffers for llie_enhance
    const size_t img = align_up((size_t)batch * 3 * c->cfg.image_size * c->cfg.image_size * 4, 256);
    return (int64_t)(core + 3 * img);
  }
  if (shape_ok(c, height, width) != LLIE_OK) return LLIE_ERR_SHAPE;
  return (int64_t)Run::plan(c, batch, [&](Run& d) { d.module(nullptr, nullptr, nullptr, height, width); });
}

// Workspace for llie_enhance with room for the hipGraph staging area (inputs/outputs of up to
// `max_steps` steps with intermediates and noise predictions).
int64_t llie_enhance_workspace_bytes(llie_ctx* c, int batch, int max_steps) {
  if (!c || batch <= 0 || max_steps <= 0 || c->cfg.kind != LLIE_UNET) return LLIE_ERR_ARG;
  const int64_t core = llie_workspace_bytes(c, batch, 0, 0);
  if (core < 0) return core;
  const size_t img = align_up((size_t)batch * 3 * c->cfg.image_size * c->cfg.image_size * 4, 256);
  return core + (int64_t)((2 + 3 * (size_t)max_steps) * img + align_up((size_t)max_steps * batch * 8, 256));
}

int llie_unet_forward(llie_ctx* c, const float* lat, const float* cond, const int64_t* t, int uniform_t, float* eps,
                      int batch, void* ws, int64_t ws_bytes, llie_stream stream) {
  if (!eps) return LLIE_ERR_ARG;
  return unet_forward_impl(c, lat, cond, t, uniform_t, eps, nullptr, batch, ws, ws_bytes, stream);
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
