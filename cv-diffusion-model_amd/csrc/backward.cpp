// Training: the backward pass over the tape that the training forward (forward.cpp) leaves, and its entry points.
#include "engine.h"

using namespace llie;

namespace {

// ---------------------------------------------------------------------------------------------
// Backward pass over the tape.  Reverse-mode over the recorded operators: every forward
// tensor's gradient lives in the same workspace (NHWC T), keyed by the tensor's offset; an operator takes
// the gradient of its output, writes / accumulates the gradients of its inputs and the fp32 parameter
// gradients (reference state_dict layout, flat buffer `grads` at Param::goff).
struct Back : Exec {
  Tape* tp;
  float* grads;
  std::map<size_t, size_t> gmap;  // forward tensor offset -> gradient offset
  // Weight gradients do not feed the activation-gradient chain, so they run on a side stream (`async`): fork() makes
  // the side stream wait for what the main stream has enqueued so far, defer() keeps a buffer the side stream may still
  // read until join(), where the main stream waits for the side stream and the deferred buffers are released.  The dry
  // run follows the same release order, so the workspace plan accounts for the longer lifetimes.
  bool async = false;
  hipStream_t s2 = nullptr;
  std::vector<size_t> deferred;
  hipStream_t side() const { return (async && s2) ? s2 : s; }
  void fork() {
    if (!async || dry || !s2) return;
    chk(hipEventRecord(c->ev_fork, s));
    chk(hipStreamWaitEvent(s2, c->ev_fork, 0));
  }
  void defer(size_t off) {
    if (async) deferred.push_back(off);
    else ar->free(off);
  }
  void join() {
    if (async && !dry && s2) {
      chk(hipEventRecord(c->ev_join, s2));
      chk(hipStreamWaitEvent(s, c->ev_join, 0));
    }
    for (size_t off : deferred) ar->free(off);
    deferred.clear();
  }

  size_t alloc(size_t bytes) { return ar->alloc(bytes); }
  // gradient of parameter `param` (an i_* index of IrbW / AttnW / ConvW / llie_ctx); null in a dry run, which has no buffer
  float* gp(int param) const { return grads ? grads + c->params[param].goff : nullptr; }

  size_t take_grad(const Tens& t) {
    auto it = gmap.find(t.off);
    if (it == gmap.end()) { if (err == hipSuccess) err = hipErrorInvalidValue; return 0; }
    const size_t g = it->second;
    gmap.erase(it);
    return g;
  }
  // gradient buffer of a forward tensor: the existing one (existed = true) or a fresh allocation
  size_t grad_of(const Tens& t, bool& existed) {
    auto it = gmap.find(t.off);
    existed = it != gmap.end();
    if (existed) return it->second;
    const size_t g = alloc((size_t)B * t.H * t.W * t.C * es());
    gmap[t.off] = g;
    return g;
  }
  void add_grad(const Tens& t, size_t g) {  // hand over `g` as (part of) t's gradient
    auto it = gmap.find(t.off);
    if (it == gmap.end()) { gmap[t.off] = g; return; }
    if (!dry) chk(launch_add_into(dt, p(it->second), p(g), (int64_t)B * t.H * t.W * t.C, s));
    ar->free(g);
  }

  // out[M][N] = in[M][K] * W[N][K]^T on the forward GEMM kernel (W = a transposed weight copy)
  void gemm(size_t in, int K, const void* w, size_t out, int N, int M, int P, size_t slab = 0, size_t dot = 0, bool with_dot = false) {
    if (dry) return;
    GemmArgs g{};
    g.seg[0] = GemmSeg{p(in), K, nullptr, nullptr, 0, ACT_NONE};
    g.nseg = 1; g.w = w; g.out = p(out); g.M = M; g.N = N; g.K = K; g.P = P;
    if (with_dot) { g.stats = p<float>(slab); g.dot = p(dot); }  // slab[b][tile][0][n] = sum over the tile's rows of out*dot
    chk(launch_pw_gemm(dt, g, s));
  }
  struct Geo { int Ho, Wo, Hi, Wi, stride, dy, dx; };
  void wgrad(size_t g, int N, const GemmSeg* segs, int nseg, int K, Geo geo, float* out, int64_t ldn, int64_t ldk, int64_t off,
             int ntap = 1, int nstore = 0, int kstore = 0) {
    const int M = wgrad_rows(B, geo.Ho * geo.Wo);  // ragged maps: padded per image to whole 64-row chunks
    // frames off the multiples of 64 in either axis split their rows freely (every level); the launch decisions at multiples of 64 stay
    const bool off64 = c->cfg.kind == LLIE_UNET && (tp->H % 64 || tp->W % 64);
    const int ms = off64 ? wgrad_msplit_ragged(dt, M, N, K, ntap) : wgrad_msplit(dt, M, N, K, ntap);
    const size_t part = alloc((size_t)ms * ntap * N * K * 4);
    if (!dry) {
      WgradArgs a{};
      a.g = p(g); a.N = N; a.nseg = nseg; a.K = K;
      for (int i = 0; i < nseg; ++i) a.seg[i] = segs[i];
      a.B = B; a.Ho = geo.Ho; a.Wo = geo.Wo; a.Hi = geo.Hi; a.Wi = geo.Wi; a.stride = geo.stride; a.dy = geo.dy; a.dx = geo.dx;
      a.partial = p<float>(part); a.out = out; a.ldn = ldn; a.ldk = ldk; a.off = off; a.msplit = ms; a.ntap = ntap; a.nstore = nstore; a.kstore = kstore;
      chk(launch_wgrad(dt, a, side()));
    }
    defer(part);
  }

  // bias gradient: out[0..Cstore) = column sums of g [M][C] (P pixels per image) through the caller's scratch slab
  // [B][bias_grad_tiles(P)][2][C] and S [B][C], on stream `st`
  void bias_grad(size_t g, int M, int C, int P, size_t slab, size_t S, float* out, int Cstore, hipStream_t st) {
    if (dry) return;
    chk(launch_bias_grad(dt, p(g), M, C, P, Cstore, p<float>(slab), p<float>(S), out, st));
  }

  // activation backward + GroupNorm backward (coefficients, norm parameter gradients, input gradient) at one norm site, on
  // launch_gn_site_bwd.  gn_plan takes the site's scratch from the arena and releases what only the coefficient pass reads;
  // the caller may then allocate the input gradient it writes into, and gn_bwd enqueues the whole site and releases the rest.
  //   g: gradient w.r.t. the activation output act(norm(x)) [M][C]; dz is written over g when act != none.
  //   pre_slab / pre_tiles: the producer already applied the activation derivative and wrote the partial sums
  //   (depthwise backward epilogue); then only the reduction and the coefficient kernels run before the apply.
  struct Coef { size_t slab, S, A, Bq, Cq, dG, dBc; int nt; bool pre; };
  Coef gn_plan(const Tens& x0, const Tens* x1, size_t pre_slab = 0, int pre_tiles = 0) {
    const int C = x0.C + (x1 ? x1->C : 0), P = x0.H * x0.W, nt = pre_tiles ? pre_tiles : (P + 63) / 64;
    Coef k{};
    k.nt = nt; k.pre = pre_tiles != 0;
    k.slab = pre_tiles ? pre_slab : alloc((size_t)B * nt * 2 * C * 4);
    k.S = alloc((size_t)B * 2 * C * 4);
    k.A = alloc((size_t)B * C * 4); k.Bq = alloc((size_t)B * C * 4); k.Cq = alloc((size_t)B * C * 4);
    k.dG = alloc((size_t)B * C * 4); k.dBc = alloc((size_t)B * C * 4);
    // released here, as the workspace plan always has: the input gradient a caller allocates before gn_bwd may land on them; it is
    // written only by the site's last kernel, after they have been read
    if (!pre_tiles) ar->free(k.slab);
    ar->free(k.S); ar->free(k.dG); ar->free(k.dBc);
    return k;
  }
  void gn_bwd(const Coef& k, size_t g, const Tens& x0, const Tens* x1, const GnRec& rec, int act, size_t gamma, size_t beta,
              float* dgamma, float* dbeta, const float* film, int64_t fstride, float* dfilm, int64_t dfstride,
              size_t add0, bool has_add0, size_t a10, bool has10, size_t a11, bool has11, size_t dx0, size_t dx1) {
    if (!dry) {
      GnSiteArgs a{};
      a.g = p(g); a.dz = act == ACT_NONE ? nullptr : p(g);
      a.x0 = p(x0.off); a.c0 = x0.C; a.x1 = x1 ? p(x1->off) : nullptr; a.c1 = x1 ? x1->C : 0;
      a.as = p<float>(rec.as); a.ab = p<float>(rec.ab); a.act = act; a.mean = p<float>(rec.mean); a.rstd = p<float>(rec.rstd);
      a.gamma = wptr<float>(gamma); a.beta = wptr<float>(beta);
      a.film = film; a.film_stride = fstride; a.dfilm = dfilm; a.dfilm_stride = dfstride; a.dgamma = dgamma; a.dbeta = dbeta;
      a.slab = p<float>(k.slab); a.ntiles = k.nt; a.slab_ready = k.pre;
      a.S = p<float>(k.S); a.A = p<float>(k.A); a.Bq = p<float>(k.Bq); a.Cq = p<float>(k.Cq); a.dG = p<float>(k.dG); a.dBc = p<float>(k.dBc);
      a.add0 = has_add0 ? p(add0) : nullptr; a.add1_0 = has10 ? p(a10) : nullptr; a.add1_1 = has11 ? p(a11) : nullptr;
      a.dx0 = p(dx0); a.dx1 = x1 ? p(dx1) : nullptr; a.B = B; a.P = x0.H * x0.W;
      chk(launch_gn_site_bwd(dt, a, s));
    }
    ar->free(k.A); ar->free(k.Bq); ar->free(k.Cq);
  }

  // ---- InvertedResidualBlock
  void irb_bwd(const IrbRec& r, size_t dfilm, int F) {
    const IrbW& w = c->irbs[r.w];
    const int H = r.x0.H, W = r.x0.W, P = H * W, M = B * P, hid = w.hid, cin = w.cin, cout = w.cout;
    const Tens* x1 = r.cat ? &r.x1 : nullptr;
    const size_t dY = take_grad(r.y);
    const Geo g11{H, W, H, W, 1, 0, 0};
    // project (+ skip) input gradients
    const size_t da3 = alloc((size_t)M * hid * es());
    const int gtiles = pw_gemm_ntiles(P);
    const size_t gslab = alloc((size_t)B * gtiles * 2 * hid * 4);  // d(gate) partials from the GEMM's epilogue: sum_px da3*h2
    gemm(dY, cout, wptr(w.w_proj_t), da3, hid, M, P, gslab, r.h2, true);
    size_t dxs = 0;
    if (w.skip) {
      dxs = alloc((size_t)M * cin * es());
      gemm(dY, cout, wptr<char>(w.w_proj_t) + (size_t)hid * cout * es(), dxs, cin, M, P);
    }
    {  // project / skip weight gradients (side stream: they only need dY, which the previous operator produced)
      fork();
      GemmSeg sg[2];
      sg[0] = GemmSeg{p(r.h2), hid, p<float>(r.gate), nullptr, hid, ACT_NONE};
      wgrad(dY, cout, sg, 1, hid, g11, gp(w.i_proj), hid, 1, 0);
      if (w.skip) {
        sg[0] = GemmSeg{p(r.x0.off), r.x0.C, nullptr, nullptr, 0, ACT_NONE};
        if (x1) sg[1] = GemmSeg{p(x1->off), x1->C, nullptr, nullptr, 0, ACT_NONE};
        wgrad(dY, cout, sg, x1 ? 2 : 1, cin, g11, gp(w.i_skip), cin, 1, 0);
      }
    }
    // SE: dgate = sum_px da3*h2, then the two-layer MLP backwards to d(mean)
    const size_t dgate = alloc((size_t)B * hid * 4), dpre2 = alloc((size_t)B * hid * 4), dr = alloc((size_t)B * w.sq * 4);
    const size_t dmean = alloc((size_t)B * hid * 4);
    {
      const size_t sescr = alloc((size_t)std::max(linear_dx_chunks(hid) * w.sq, linear_dx_chunks(w.sq) * hid) * B * 4);
      if (!dry) {
        chk(launch_slab_reduce(p<float>(gslab), p<float>(dgate), B, gtiles, 2, 1, hid, s));
        chk(launch_sigmoid_bwd(p<float>(dgate), p<float>(r.gate), p<float>(dpre2), (int64_t)B * hid, s));
        chk(launch_linear_dw(p<float>(dpre2), hid, p<float>(r.sehid), gp(w.i_se_w2), gp(w.i_se_b2), B, hid, w.sq, s));
        chk(launch_linear_dx(dt, p<float>(dpre2), hid, wptr(w.se_w2), p<float>(dr), B, hid, w.sq, s, p<float>(sescr)));
        chk(launch_relu6_bwd(p<float>(dr), p<float>(r.sehid), p<float>(dr), (int64_t)B * w.sq, s));
        chk(launch_linear_dw(p<float>(dr), w.sq, p<float>(r.semean), gp(w.i_se_w1), gp(w.i_se_b1), B, w.sq, hid, s));
        chk(launch_linear_dx(dt, p<float>(dr), w.sq, wptr(w.se_w1), p<float>(dmean), B, w.sq, hid, s, p<float>(sescr)));
        chk(launch_scale_rows(p<float>(dmean), p<float>(dmean), (int64_t)B * hid, 1.f / (float)P, s));
      }
      ar->free(gslab); ar->free(sescr);
    }
    // depthwise: input gradient (same kernel, flipped taps, prologue dh2 = da3*gate + dmean/P) and weight gradient
    const size_t da2 = alloc((size_t)M * hid * es());
    const int dztiles = dwconv_ntiles(H, W);
    const size_t dzslab = alloc((size_t)B * dztiles * 2 * hid * 4);
    {
      const size_t part = alloc((size_t)B * dw_wgrad_strips(H, W) * 9 * hid * 4);
      if (!dry) {
        DwArgs d{};  // writes dz2 = da2 * relu6'(norm2(h1)) and the (sum dz, sum dz*h1) partials in its epilogue
        d.in = p(da3); d.out = p(da2); d.as = p<float>(r.gate); d.ab = p<float>(dmean); d.w = wptr<float>(w.w_dw_flip);
        d.pool = nullptr; d.B = B; d.H = H; d.W = W; d.C = hid; d.no_act = 1;
        d.bx = p(r.h1.off); d.bas = p<float>(r.n2.as); d.bab = p<float>(r.n2.ab); d.bslab = p<float>(dzslab);
        chk(launch_dwconv3x3(dt, d, s));
        fork();  // da3 and d(mean) are enqueued: the depthwise weight gradient may run beside the rest of the chain
        DwWgradArgs q{};
        q.g = p(da3); q.gs = p<float>(r.gate); q.gb = p<float>(dmean); q.h = p(r.h1.off); q.as = p<float>(r.n2.as);
        q.ab = p<float>(r.n2.ab); q.partial = p<float>(part); q.out = gp(w.i_dw); q.B = B; q.H = H; q.W = W; q.C = hid;
        chk(launch_dw_wgrad(dt, q, side()));
      }
      defer(part);
    }
    defer(da3); ar->free(dgate); ar->free(dpre2); ar->free(dr); defer(dmean);
    // norm2 + FiLM + ReLU6
    const float* film = p<float>(tp->film) + w.film_off;
    float* dfl = p<float>(dfilm) + w.film_off;
    const Coef k2 = gn_plan(r.h1, nullptr, dzslab, dztiles);
    ar->free(dzslab);
    gn_bwd(k2, da2, r.h1, nullptr, r.n2, ACT_RELU6, w.n2g, w.n2b, gp(w.i_n2g), gp(w.i_n2b), film, F, dfl, F,
           0, false, 0, false, 0, false, da2, 0);  // dh1, in place
    // expand
    const size_t da1 = alloc((size_t)M * cin * es());
    gemm(da2, hid, wptr(w.w_expand_t), da1, cin, M, P);
    {
      GemmSeg sg[2];
      sg[0] = GemmSeg{p(r.x0.off), r.x0.C, p<float>(r.n1.as), p<float>(r.n1.ab), cin, ACT_RELU6};
      if (x1) sg[1] = GemmSeg{p(x1->off), x1->C, p<float>(r.n1.as) + r.x0.C,
                              p<float>(r.n1.ab) + r.x0.C, cin, ACT_RELU6};
      fork();  // dh1 (in da2) is complete
      wgrad(da2, hid, sg, x1 ? 2 : 1, cin, g11, gp(w.i_expand), cin, 1, 0);
    }
    defer(da2);
    // norm1 + ReLU6, then the block input (residual / skip-conv gradient added, existing gradients accumulated)
    const Coef k1 = gn_plan(r.x0, x1);
    bool e0 = false, e1 = false;
    const size_t g0 = grad_of(r.x0, e0);
    const size_t g1 = x1 ? grad_of(*x1, e1) : 0;
    gn_bwd(k1, da1, r.x0, x1, r.n1, ACT_RELU6, w.n1g, w.n1b, gp(w.i_n1g), gp(w.i_n1b), nullptr, 0, nullptr, 0,
           w.skip ? dxs : dY, true, g0, e0, g1, e1, g0, g1);
    ar->free(da1);
    if (w.skip) ar->free(dxs);
    defer(dY);
    join();
  }

  // ---- StandardAttention: y = to_out(core(to_qkv(norm(x)))) + x
  void softattn_bwd(const AttnRec& r) {
    const AttnW& w = c->attns[r.w];
    const int H = r.x.H, W = r.x.W, N = H * W, M = B * N, C = w.c, inner = w.inner;
    const size_t dY = take_grad(r.y);  // fans out to to_out and, through the last gn_bwd's add0, to the residual
    const Geo g11{H, W, H, W, 1, 0, 0};
    // to_out
    const size_t dao = alloc((size_t)M * inner * es());
    gemm(dY, C, wptr(w.w_out_t), dao, inner, M, N);
    {
      GemmSeg sg{p(r.ao), inner, nullptr, nullptr, 0, ACT_NONE};
      fork();
      wgrad(dY, C, &sg, 1, inner, g11, gp(w.i_out), inner, 1, 0);
    }
    // attention core
    const size_t dqkv = alloc((size_t)M * 3 * inner * es());
    {
      const size_t delta = alloc((size_t)B * w.heads * N * 4);
      if (!dry) {
        SoftAttnBwdArgs a{};
        a.qkv = p(r.qkv); a.out = p(r.ao); a.dout = p(dao); a.lse = p<float>(r.lse); a.dqkv = p(dqkv); a.delta = p<float>(delta);
        a.B = B; a.N = N; a.heads = w.heads;
        chk(launch_softattn_bwd(dt, a, s));
      }
      ar->free(delta);
    }
    ar->free(dao);
    // to_qkv
    const size_t dxn = alloc((size_t)M * C * es());
    gemm(dqkv, 3 * inner, wptr(w.w_qkv_t), dxn, C, M, N);
    {
      GemmSeg sg{p(r.x.off), C, p<float>(r.n1.as), p<float>(r.n1.ab), C, ACT_NONE};
      fork();
      wgrad(dqkv, 3 * inner, &sg, 1, C, g11, gp(w.i_qkv), C, 1, 0);
    }
    defer(dqkv);
    // norm (no activation) + residual
    const Coef k1 = gn_plan(r.x, nullptr);
    bool e0 = false;
    const size_t g0 = grad_of(r.x, e0);
    gn_bwd(k1, dxn, r.x, nullptr, r.n1, ACT_NONE, w.ng, w.nb, gp(w.i_ng), gp(w.i_nb), nullptr, 0, nullptr, 0,
           dY, true, g0, e0, 0, false, g0, 0);
    ar->free(dxn);
    defer(dY);  // to_out's weight gradient on the side stream reads it
    join();
  }

  // ---- LinearAttention
  void attn_bwd(const AttnRec& r) {
    const AttnW& w = c->attns[r.w];
    if (w.soft) return softattn_bwd(r);
    const int H = r.x.H, W = r.x.W, N = H * W, M = B * N, C = w.c, inner = w.inner;
    const size_t dY = take_grad(r.y);
    const Geo g11{H, W, H, W, 1, 0, 0};
    // y = norm2(tmp) + x
    const Coef k2 = gn_plan(r.tmp, nullptr);
    const size_t dtmp = alloc((size_t)M * C * es());
    gn_bwd(k2, dY, r.tmp, nullptr, r.n2, ACT_NONE, w.n2g, w.n2b, gp(w.i_n2g), gp(w.i_n2b), nullptr, 0, nullptr, 0,
           0, false, 0, false, 0, false, dtmp, 0);
    // to_out
    const size_t dao = alloc((size_t)M * inner * es());
    gemm(dtmp, C, wptr(w.w_out_t), dao, inner, M, N);
    {
      GemmSeg sg{p(r.ao), inner, nullptr, nullptr, 0, ACT_NONE};
      fork();
      wgrad(dtmp, C, &sg, 1, inner, g11, gp(w.i_out), inner, 1, 0);
    }
    defer(dtmp);
    // attention core
    const size_t dqkv = alloc((size_t)M * 3 * inner * es());
    {
      const int nt = (N + 63) / 64;
      const size_t part = alloc((size_t)B * w.heads * nt * 32 * 33 * 4), tot = alloc((size_t)B * w.heads * 32 * 33 * 4);
      if (!dry) {
        AttnBwdArgs a{};
        a.qkv = p(r.qkv); a.dout = p(dao); a.dqkv = p(dqkv); a.kv = p<float>(r.kv); a.nsplit = r.nsplit;
        a.dkv = p<float>(part); a.B = B; a.N = N; a.heads = w.heads;
        chk(launch_linattn_bwd(dt, a, p<float>(tot), s));
      }
      ar->free(part); ar->free(tot);
    }
    ar->free(dao);
    // to_qkv
    const size_t dxn = alloc((size_t)M * C * es());
    gemm(dqkv, 3 * inner, wptr(w.w_qkv_t), dxn, C, M, N);
    {
      GemmSeg sg{p(r.x.off), C, p<float>(r.n1.as), p<float>(r.n1.ab), C, ACT_NONE};
      fork();
      wgrad(dqkv, 3 * inner, &sg, 1, C, g11, gp(w.i_qkv), C, 1, 0);
    }
    defer(dqkv);
    // norm (no activation) + residual
    const Coef k1 = gn_plan(r.x, nullptr);
    bool e0 = false;
    const size_t g0 = grad_of(r.x, e0);
    gn_bwd(k1, dxn, r.x, nullptr, r.n1, ACT_NONE, w.ng, w.nb, gp(w.i_ng), gp(w.i_nb), nullptr, 0, nullptr, 0,
           dY, true, g0, e0, 0, false, g0, 0);
    ar->free(dxn);
    ar->free(dY);
    join();
  }

  // ---- Downsample / Upsample convolutions
  void conv_bwd(const ConvRec& r) {
    const ConvW& w = r.up ? c->ups[r.w] : c->downs[r.w];
    const int C = w.c, Ho = r.y.H, Wo = r.y.W, Mo = B * Ho * Wo;
    const size_t dY = take_grad(r.y);
    {  // bias gradient: column sums of dY
      const int nt = bias_grad_tiles(Ho * Wo);
      const size_t slab = alloc((size_t)B * nt * 2 * C * 4), S = alloc((size_t)B * C * 4);
      bias_grad(dY, Mo, C, Ho * Wo, slab, S, gp(w.i_bias), C, s);
      ar->free(slab); ar->free(S);
    }
    const Tens& src = r.up ? r.u : r.x;  // what the conv itself read
    {
      GemmSeg sg{p(src.off), C, nullptr, nullptr, 0, ACT_NONE};
      const Geo geo{Ho, Wo, src.H, src.W, r.up ? 1 : 2, 0, 0};
      fork();
      wgrad(dY, C, &sg, 1, C, geo, gp(w.i_w), (int64_t)C * 9, 9, 0, 9);
    }
    // input gradient: stride-1 conv with flipped / transposed weights over dY (zero-dilated for the stride-2 conv)
    size_t din = dY;
    if (!r.up) {
      din = alloc((size_t)B * r.x.H * r.x.W * C * es());
      if (!dry) chk(launch_dilate2x(dt, p(dY), p(din), B, Ho, Wo, C, s));
    }
    const size_t dsrc = alloc((size_t)B * src.H * src.W * C * es());
    if (!dry) {
      Conv3Args a{};
      a.in = p(din); a.w = wptr(w.w_t); a.bias = nullptr; a.out = p(dsrc); a.stats = nullptr;
      a.B = B; a.Hi = src.H; a.Wi = src.W; a.Cin = C; a.Cout = C; a.mode = 2;
      chk(launch_conv3x3(dt, a, s));
    }
    if (!r.up) ar->free(din);
    defer(dY);
    if (r.up) {
      const size_t dx = alloc((size_t)B * r.x.H * r.x.W * C * es());
      if (!dry) chk(launch_upsample2x_bwd(dt, p(dsrc), p(dx), B, r.x.H, r.x.W, C, s));
      ar->free(dsrc);
      add_grad(r.x, dx);
    } else {
      add_grad(r.x, dsrc);
    }
    join();
  }

  void run_ops(size_t dfilm, int F) {
    for (int i = (int)tp->ops.size() - 1; i >= 0; --i) {
      const TapeOp& op = tp->ops[i];
      if (op.kind == 0) irb_bwd(tp->irbs[op.idx], dfilm, F);
      else if (op.kind == 1) attn_bwd(tp->attns[op.idx]);
      else conv_bwd(tp->convs[op.idx]);
    }
  }
  // FiLM Linear of every block: weight / bias gradients, and d(silu(temb)) summed over all FiLM rows
  void film_bwd(size_t dfilm, int F, int T, size_t dstemb) {
    const size_t scratch = alloc((size_t)linear_dx_chunks(F) * B * T * 4);
    if (!dry) {
      for (const IrbW& w : c->irbs)
        chk(launch_linear_dw(p<float>(dfilm) + w.film_off, F, p<float>(tp->stemb), gp(w.i_film_w), gp(w.i_film_b), B,
                             2 * w.hid, T, s));
      chk(launch_linear_dx(0, p<float>(dfilm), F, wptr(c->film_w), p<float>(dstemb), B, F, T, s, p<float>(scratch)));
    }
    ar->free(scratch);
  }

  // ---- whole UNet; dlat / dcond (optional): fp32 NCHW gradients of the two input halves, caller buffers
  void unet(const float* deps, float* dlat = nullptr, float* dcond = nullptr) {
    const llie_config& g = c->cfg;
    const int H = tp->H, W = tp->W, C0 = c->channels[0], P = H * W, M = B * P, T = g.time_embed_dim, F = c->film_rows;
    const size_t dfilm = alloc((size_t)B * F * 4);
    // output head
    const size_t da = alloc((size_t)M * C0 * es());
    {
      // weight gradient of the head on the MFMA weight-gradient GEMM: d(eps) packed to [M][32] NHWC is the "g"
      // operand (3 real rows), silu(norm(h)) recomputed in the prologue the other; bias = plane sums of d(eps).
      // It only needs d(eps) and forward tensors: side stream, joined with the first operator.
      const size_t g32 = alloc((size_t)M * 32 * es());
      const int nt = bias_grad_tiles(P);
      const size_t bslab = alloc((size_t)B * nt * 2 * 32 * 4), bS = alloc((size_t)B * 32 * 4);
      if (!dry) {
        FinalBwdArgs a{};
        a.deps = deps; a.w = wptr<float>(c->fin_w); a.da = p(da);
        a.B = B; a.H = H; a.W = W; a.C = C0; a.Cout = g.out_channels;
        chk(launch_final_bwd_data(dt, a, s));
        fork();
        chk(launch_pack_planes(dt, deps, nullptr, g.out_channels, 0, p(g32), B, P, side()));
        bias_grad(g32, M, 32, P, bslab, bS, gp(c->i_fin_bias), g.out_channels, side());  // of the packed d(eps)
      }
      defer(bslab); defer(bS);
      GemmSeg sg{p(tp->hlast.off), C0, p<float>(tp->fin.as), p<float>(tp->fin.ab), C0, ACT_SILU};
      const Geo geo{H, W, H, W, 1, 0, 0};
      wgrad(g32, 32, &sg, 1, C0, geo, gp(c->i_fin_w), (int64_t)C0 * 9, 9, 0, 9, g.out_channels, 0);
      defer(g32);  // released at the first operator's join
    }
    const Coef kf = gn_plan(tp->hlast, nullptr);
    gn_bwd(kf, da, tp->hlast, nullptr, tp->fin, ACT_SILU, c->fin_g, c->fin_b, gp(c->i_fin_g),
           gp(c->i_fin_b), nullptr, 0, nullptr, 0, 0, false, 0, false, 0, false, da, 0);
    gmap[tp->hlast.off] = da;
    run_ops(dfilm, F);
    // input conv
    {
      // dW[co][ci][tap] on the same GEMM: g = d(h0) [M][C0], the other operand the two fp32 input planes packed to
      // [M][32] NHWC (6 real channels); bias = column sums of d(h0)
      const size_t g0 = take_grad(tp->h0);
      const int half = g.in_channels / 2, nt = bias_grad_tiles(P);
      const size_t x32 = alloc((size_t)M * 32 * es());
      const size_t slab = alloc((size_t)B * nt * 2 * C0 * 4), S1 = alloc((size_t)B * C0 * 4);
      if (!dry) {
        chk(launch_pack_planes(dt, tp->lat, tp->cond, half, g.in_channels - half, p(x32), B, P, s));
        bias_grad(g0, M, C0, P, slab, S1, gp(c->i_init_b), c->channels_r[0], s);
      }
      GemmSeg sg{p(x32), 32, nullptr, nullptr, 0, ACT_NONE};
      const Geo geo{H, W, H, W, 1, 0, 0};
      fork();
      wgrad(g0, C0, &sg, 1, 32, geo, gp(c->i_init_w), (int64_t)g.in_channels * 9, 9, 0, 9, c->channels_r[0], g.in_channels);
      ar->free(slab); ar->free(S1);
      // data gradient of the input conv, on the main stream beside the weight-gradient GEMM: both only read g0
      if (!dry && (dlat || dcond)) {
        InitDgradArgs a{};
        a.g = p(g0); a.w = wptr<float>(c->init_w); a.dx0 = dlat; a.dx1 = dcond; a.c0 = half; a.c1 = g.in_channels - half;
        a.B = B; a.H = H; a.W = W; a.C0 = C0;
        chk(launch_init_conv_dgrad(dt, a, s));
      }
      defer(x32); defer(g0);
      join();
    }
    // time embedding MLP (efficient_unet.py:412-417): temb = W3 silu(W1 emb + b1) + b3, FiLM reads silu(temb)
    const int dim = g.base_channels;
    const size_t dtemb = alloc((size_t)B * T * 4), emb = alloc((size_t)B * dim * 4), z1 = alloc((size_t)B * T * 4);
    const size_t a1 = alloc((size_t)B * T * 4), dh = alloc((size_t)B * T * 4);
    film_bwd(dfilm, F, T, dtemb);
    if (!dry) {
      chk(launch_silu_bwd(p<float>(dtemb), p<float>(tp->temb), p<float>(dtemb), (int64_t)B * T, s));
      chk(launch_sin_embed(tp->t, wptr<float>(c->freqs), p<float>(emb), B, dim, s));
      chk(launch_film(film_args(emb, B, dim, c->t_w1, c->t_b1, z1, T), s));
      chk(launch_silu_rows(p<float>(z1), p<float>(a1), (int64_t)B * T, s));
      chk(launch_linear_dw(p<float>(dtemb), T, p<float>(a1), gp(c->i_t_w3), gp(c->i_t_b3), B, T, T, s));
      chk(launch_linear_dx(0, p<float>(dtemb), T, wptr(c->t_w3), p<float>(dh), B, T, T, s));
      chk(launch_silu_bwd(p<float>(dh), p<float>(z1), p<float>(dh), (int64_t)B * T, s));
      chk(launch_linear_dw(p<float>(dh), T, p<float>(emb), gp(c->i_t_w1), gp(c->i_t_b1), B, T, dim, s));
    }
    ar->free(dtemb); ar->free(emb); ar->free(z1); ar->free(a1); ar->free(dh); ar->free(dfilm);
  }

  // ---- single operator: dy / dx fp32 NCHW, dtemb [B][T] (IRB only)
  void module(const float* temb, const float* dy, float* dx, float* dtemb) {
    const llie_config& g = c->cfg;
    const Tens& out = tp->hlast;
    const Tens& x0 = tp->h0;
    const Tens& x1 = tp->x1;
    const int T = g.time_embed_dim, F = c->film_rows;
    const size_t gy = alloc((size_t)B * out.H * out.W * out.C * es());
    if (!dry) chk(launch_nchw_to_nhwc(dt, dy, p(gy), nullptr, B, out.C, out.H * out.W, out.C, 0, s));
    gmap[out.off] = gy;
    const size_t dfilm = g.kind == LLIE_IRB ? alloc((size_t)B * F * 4) : 0;
    run_ops(dfilm, F);
    if (g.kind == LLIE_IRB) {
      const size_t ds = alloc((size_t)B * T * 4);
      film_bwd(dfilm, F, T, ds);
      if (!dry) chk(launch_silu_bwd(p<float>(ds), temb, dtemb, (int64_t)B * T, s));
      ar->free(ds); ar->free(dfilm);
    }
    const size_t g0 = take_grad(x0);
    if (!dry) chk(launch_nhwc_to_nchw(dt, p(g0), dx, B, x0.C, x0.H * x0.W, s, g.in_channels, 0));
    ar->free(g0);
    if (x1.valid) {
      const size_t g1 = take_grad(x1);
      if (!dry) chk(launch_nhwc_to_nchw(dt, p(g1), dx, B, x1.C, x1.H * x1.W, s, g.in_channels, x0.C));
      ar->free(g1);
    }
  }
};

}  // namespace

// side stream + events of the backward pass (created on first use); dry runs only copy the flag
static int setup_async(llie_ctx* c, Back& b) {
  b.async = g_knobs.bwd_async != 0;
  if (!b.async || b.dry) return LLIE_OK;
  hipError_t e = hipSuccess;
  if (!c->side_stream) e = hipStreamCreateWithFlags(&c->side_stream, hipStreamNonBlocking);
  if (e == hipSuccess && !c->ev_fork) e = hipEventCreateWithFlags(&c->ev_fork, hipEventDisableTiming);
  if (e == hipSuccess && !c->ev_join) e = hipEventCreateWithFlags(&c->ev_join, hipEventDisableTiming);
  if (e != hipSuccess) { set_err("backward side stream: %s", hipGetErrorString(e)); return (int)e; }
  b.s2 = c->side_stream;
  return LLIE_OK;
}

// The frames a UNet handle trains at: the frame rule of the forward, tightened by what only the backward pass stores.  Every
// gradient has the shape of its forward tensor, the zero-dilated gradient of a stride-2 conv has the shape of that conv's input and
// the tape's up-sampled tensor at full resolution carries channels[1]; the packed [M][32] operands of the head and the input conv
// carry 32.  The weight-gradient GEMM walks wgrad_rows(B, P) rows -- each image padded to whole 64-row chunks -- and forms
// row * channels in 32 bits, so the cap is taken over the padded rows.  Lower levels hold a quarter of the pixels at twice the
// channels per step down, and at least 64 pixels each (H, W >= 64), so padding at most doubles them: full resolution is the bound.
static int train_shape_ok(const llie_ctx* c, int batch, int H, int W) {
  if (!c || c->cfg.kind != LLIE_UNET || batch <= 0) return LLIE_ERR_ARG;
  if (c->padded) { set_err("the unpinned variants (tiny / base, zero-padded channels) are inference-only"); return LLIE_ERR_CONFIG; }
  const int rc = frame_shape_ok(c, batch, H, W);
  if (rc) return rc;
  const int cw = std::max({widest_full_res_channels(c), c->channels[1], 32});
  const long long rows = (long long)batch * (((long long)H * W + 63) / 64 * 64);
  if (rows * cw > 2147483647ll) {
    set_err("training frame too large: batch %d x %dx%d (rows padded to 64 per image) x %d channels exceeds the element cap 2^31 - 1",
            batch, H, W, cw);
    return LLIE_ERR_SHAPE;
  }
  return LLIE_OK;
}

// what the training entry points check before they touch the device: loaded weights and a workspace that holds the plan
// (a UNet handle: H = W = 0 is image_size)
static int train_ready(llie_ctx* c, int batch, int H, int W, int64_t ws_bytes) {
  int rc = check_ready(c);
  if (rc) return rc;
  if (c->cfg.kind != LLIE_UNET && (rc = shape_ok(c, H, W))) return rc;
  const int64_t need = llie_train_workspace_bytes(c, batch, H, W);
  return need < 0 ? (int)need : fits((size_t)need, ws_bytes);
}

extern "C" {

// ---------------------------------------------------------------------------------------------
// Training: forward that keeps its activations + reverse pass over the tape.
int64_t llie_grad_numel(const llie_ctx* c) { return c ? c->grad_numel : LLIE_ERR_ARG; }
int64_t llie_param_grad_offset(const llie_ctx* c, int i) {
  if (!c || i < 0 || i >= (int)c->params.size()) return LLIE_ERR_ARG;
  return c->params[i].goff;
}

int64_t llie_train_workspace_bytes(llie_ctx* c, int batch, int height, int width) {
  if (!c || batch <= 0) return LLIE_ERR_ARG;
  if (c->padded) { set_err("the unpinned variants (tiny / base, zero-padded channels) are inference-only"); return LLIE_ERR_CONFIG; }
  Arena ar;
  Tape tape;
  const Exec x = Exec::planning(c, &ar, batch);
  Back b{x, &tape, nullptr};
  setup_async(c, b);
  if (c->cfg.kind == LLIE_UNET) {
    if ((height == 0) != (width == 0) || height < 0 || width < 0) return LLIE_ERR_ARG;
    if (height == 0) height = width = c->cfg.image_size;  // unchecked, as the entry points at image_size always were
    else if (const int rc = train_shape_ok(c, batch, height, width)) return rc;
    run_unet(x, &tape, nullptr, nullptr, nullptr, nullptr, height, width);
    b.unet(nullptr);
  } else {
    if (shape_ok(c, height, width) != LLIE_OK) return LLIE_ERR_SHAPE;
    run_module(x, &tape, nullptr, nullptr, nullptr, height, width);
    b.module(nullptr, nullptr, nullptr, nullptr);
  }
  if (b.err != hipSuccess) { set_err("training plan is inconsistent"); return LLIE_ERR_ARG; }
  return (int64_t)ar.high;
}

int llie_train_shape_ok(const llie_ctx* c, int batch, int height, int width) { return train_shape_ok(c, batch, height, width); }

// llie_unet_train_forward (H = W = 0: image_size, unchecked as always) and llie_unet_train_forward_hw
static int train_forward_impl(llie_ctx* c, const float* lat, const float* cond, const int64_t* t, float* eps, int batch, int H, int W,
                              void* ws, int64_t ws_bytes, llie_stream stream) {
  if (!c || !lat || !cond || !t || !eps || !ws || batch <= 0 || c->cfg.kind != LLIE_UNET) return LLIE_ERR_ARG;
  if (c->padded) { set_err("the unpinned variants (tiny / base, zero-padded channels) are inference-only"); return LLIE_ERR_CONFIG; }
  int rc = train_ready(c, batch, H, W, ws_bytes);
  if (rc) return rc;
  if (!H) H = W = c->cfg.image_size;
  delete c->train_arena;
  c->train_arena = new Arena((size_t)ws_bytes);
  c->tape.clear();
  rc = run_unet(Exec::live(c, c->train_arena, stream, ws, batch), &c->tape, lat, cond, t, eps, H, W);
  if (rc) return rc;
  c->tape.valid = true;
  c->tape.ws = ws;
  return LLIE_OK;
}

int llie_unet_train_forward(llie_ctx* c, const float* lat, const float* cond, const int64_t* t, float* eps, int batch,
                            void* ws, int64_t ws_bytes, llie_stream stream) {
  return train_forward_impl(c, lat, cond, t, eps, batch, 0, 0, ws, ws_bytes, stream);
}

int llie_unet_train_forward_hw(llie_ctx* c, const float* lat, const float* cond, const int64_t* t, float* eps, int batch,
                               int height, int width, void* ws, int64_t ws_bytes, llie_stream stream) {
  if (height <= 0 || width <= 0) return LLIE_ERR_ARG;
  return train_forward_impl(c, lat, cond, t, eps, batch, height, width, ws, ws_bytes, stream);
}

int llie_unet_backward_dx(llie_ctx* c, const float* d_eps, float* grads, float* d_latents, float* d_cond, int batch, void* ws,
                          int64_t ws_bytes, llie_stream stream) {
  if (!c || !d_eps || !grads || !ws || c->cfg.kind != LLIE_UNET) return LLIE_ERR_ARG;
  if (!c->tape.valid || c->tape.ws != ws || c->tape.B != batch || !c->train_arena || (int64_t)c->train_arena->cap != ws_bytes) {
    set_err("llie_unet_backward needs the workspace of the preceding llie_unet_train_forward (same batch)");
    return LLIE_ERR_ARG;
  }
  Back b{Exec::live(c, c->train_arena, stream, ws, batch), &c->tape, grads};
  if (const int rc = setup_async(c, b)) return rc;
  b.unet(d_eps, d_latents, d_cond);
  return b.rc(true);
}
int llie_unet_backward(llie_ctx* c, const float* d_eps, float* grads, int batch, void* ws, int64_t ws_bytes, llie_stream stream) {
  return llie_unet_backward_dx(c, d_eps, grads, nullptr, nullptr, batch, ws, ws_bytes, stream);
}

int llie_module_backward(llie_ctx* c, const float* x, const float* temb, const float* dy, float* dx, float* dtemb, float* grads,
                         int batch, int H, int W, void* ws, int64_t ws_bytes, llie_stream stream) {
  if (!c || !x || !dy || !dx || !grads || !ws || batch <= 0 || c->cfg.kind == LLIE_UNET || c->cfg.kind == LLIE_SE) return LLIE_ERR_ARG;
  if (c->cfg.kind == LLIE_IRB && (!temb || !dtemb)) return LLIE_ERR_ARG;
  int rc = train_ready(c, batch, H, W, ws_bytes);
  if (rc) return rc;
  Arena ar((size_t)ws_bytes);
  Tape tape;
  const Exec live = Exec::live(c, &ar, stream, ws, batch);
  rc = run_module(live, &tape, x, temb, nullptr, H, W);
  if (rc) return rc;
  Back b{live, &tape, grads};
  if ((rc = setup_async(c, b))) return rc;
  b.module(temb, dy, dx, dtemb);
  return b.rc(true);
}

}  // extern "C"
