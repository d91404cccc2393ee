// Kernel-level entry points (unit tests, tuning), pre / post-processing, optimiser, EMA, distillation and the memory probes:
// thin wrappers over the launch API of kernels.h.
#include "engine.h"

using namespace llie;

static bool dtype_ok(int dtype) { return dtype >= 0 && dtype <= 2; }

int llie::kerr(const char* what, hipError_t e, int refuse_rc, const char* refuse_msg) {
  if (e == hipSuccess) return LLIE_OK;
  if (e == hipErrorInvalidValue && refuse_rc) {
    if (refuse_msg) set_err("%s: %s", what, refuse_msg);
    return refuse_rc;
  }
  set_err("%s: %s", what, hipGetErrorString(e));
  return (int)e;
}

// the C ABI's K segments as the launch API's; returns their total channel count
static int to_segs(const llie_gemm_seg* segs, int nseg, GemmSeg* out) {
  int K = 0;
  for (int i = 0; i < nseg; ++i) {
    out[i] = GemmSeg{segs[i].ptr, segs[i].channels, segs[i].scale, segs[i].bias, segs[i].affine_ld, segs[i].act};
    K += segs[i].channels;
  }
  return K;
}

extern "C" {

int llie_gram_stats(int dtype, const void* x0, int c0, const void* x1, int c1, const float* scale, const float* bias, int batch, int pixels,
                    float* part, float* gtot, unsigned int* tickets, llie_stream stream) {
  GramArgs a{};
  a.x0 = x0; a.x1 = x1; a.c0 = c0; a.c1 = c1; a.as1 = scale; a.ab1 = bias; a.part = part; a.gtot = gtot; a.tickets = tickets; a.B = batch; a.P = pixels;
  if (!gram_supported(dtype, c0 + c1, c0, pixels)) { set_err("gram_stats: K in {32, 64, 96}, 2-byte dtype, pixels a multiple of 512"); return LLIE_ERR_SHAPE; }
  // a refusal keeps the runtime's own text for hipErrorInvalidValue, mapped to LLIE_ERR_ARG
  return kerr("gram_stats", launch_gram_stats(dtype, a, hs(stream)), LLIE_ERR_ARG, hipGetErrorString(hipErrorInvalidValue));
}
int64_t llie_gram_part_floats(int K, int pixels) { return (K == 32 || K == 64 || K == 96) && pixels > 0 && pixels % 512 == 0 ? (int64_t)gram_part_floats(K, pixels) : LLIE_ERR_ARG; }

// ---- kernel-level entry points (unit tests, tuning): thin wrappers over the launch API
}  // extern "C"
static int pw_gemm_call(const char* what, int dtype, const llie_gemm_seg* segs, int nseg, const void* w, const float* bias, const void* residual,
                        const void* dot, void* out, float* stats, int M, int N, int P, llie_stream stream) {
  if (!segs || nseg < 1 || nseg > 3 || !w || !out || dtype < 0 || dtype > 2) return LLIE_ERR_ARG;
  // the kernel's prologue is affine (+ ReLU6 / clamp01) and runs only where a segment has a table: an activation it does not
  // have (SiLU), an activation or a shift without a scale table, or a table row shorter than the segment would be computed as
  // something else without a word
  for (int i = 0; i < nseg; ++i) {
    const llie_gemm_seg& sg = segs[i];
    if ((sg.act != ACT_NONE && sg.act != ACT_RELU6 && sg.act != ACT_RELU6_S6) || (!sg.scale && (sg.act != ACT_NONE || sg.bias)) ||
        (sg.scale && sg.affine_ld < sg.channels)) {
      set_err("%s: segment %d: act 0, 1 or 3; an activation or a shift needs a scale table; affine_ld >= channels", what, i);
      return LLIE_ERR_ARG;
    }
  }
  GemmArgs g{};
  g.nseg = nseg;
  g.K = to_segs(segs, nseg, g.seg);
  g.w = w; g.bias = bias; g.res = residual; g.dot = dot; g.out = out; g.stats = stats; g.M = M; g.N = N; g.P = P;
  return kerr(what, launch_pw_gemm(dtype, g, hs(stream)));
}
extern "C" {
int llie_pw_gemm(int dtype, const llie_gemm_seg* segs, int nseg, const void* w, const float* bias, const void* residual,
                 void* out, float* stats, int M, int N, int P, llie_stream stream) {
  return pw_gemm_call("pw_gemm", dtype, segs, nseg, w, bias, residual, nullptr, out, stats, M, N, P, stream);
}
// the backward pass's epilogue (backward.cpp: gemm(.., with_dot)): the slab holds (sum out * dot, sum out) per tile
int llie_pw_gemm_dot(int dtype, const llie_gemm_seg* segs, int nseg, const void* w, const float* bias, const void* dot, void* out,
                     float* stats, int M, int N, int P, llie_stream stream) {
  if (!dot || !stats) return LLIE_ERR_ARG;
  return pw_gemm_call("pw_gemm_dot", dtype, segs, nseg, w, bias, nullptr, dot, out, stats, M, N, P, stream);
}

int llie_pw_expand(int dtype, const llie_gemm_seg* segs, int nseg, const float* w32, void* wpack, void* out, float* stats,
                   int M, int N, int P, llie_stream stream) {
  if (!segs || nseg < 1 || nseg > 3 || !wpack || !out || !stats || dtype < 1 || dtype > 2) return LLIE_ERR_ARG;
  ExpandArgs x{};
  x.nseg = nseg;
  x.K = to_segs(segs, nseg, x.seg);
  x.wf = wpack; x.out = out; x.stats = stats; x.M = M; x.N = N; x.P = P;
  hipStream_t s = hs(stream);
  hipError_t e = !pw_expand_supported(dtype, x.seg, nseg, M, N, x.K, P) ? hipErrorInvalidValue
                 : (w32 ? launch_pack_expand(dtype, w32, wpack, N, x.K, 6.f, s) : hipSuccess);
  if (e == hipSuccess) e = launch_pw_expand(dtype, x, s);
  return kerr("pw_expand", e);
}

int llie_dwconv3x3(int dtype, const void* in, void* out, const float* scale, const float* bias, const float* w9c,
                   float* pool, int B, int H, int W, int C, llie_stream stream) {
  if (!in || !out || !scale || !bias || !w9c || dtype < 0 || dtype > 2) return LLIE_ERR_ARG;
  DwArgs d{};
  d.in = in; d.out = out; d.as = scale; d.ab = bias; d.w = w9c; d.pool = pool; d.B = B; d.H = H; d.W = W; d.C = C;
  return kerr("dwconv3x3", launch_dwconv3x3(dtype, d, hs(stream)));
}
// the forms the engines run beyond llie_dwconv3x3: fixed-point pool totals, the clamp01 prologue with weights x 6 (s6), no activation
int llie_dwconv3x3_ex(int dtype, const void* in, void* out, const float* scale, const float* bias, const float* w9c, float* pool,
                      unsigned long long* pool_totals, int flags, int B, int H, int W, int C, llie_stream stream) {
  const int s6 = flags & 1, no_act = (flags >> 1) & 1;
  if (!in || !out || !scale || !bias || !w9c || dtype < 0 || dtype > 2 || (pool && pool_totals) || flags < 0 || flags > 3 ||
      (s6 && (no_act || dtype == 0)) || B <= 0 || H <= 0 || W <= 0 || C <= 0 || C % (dtype == 0 ? 32 : 64))
    return LLIE_ERR_ARG;
  DwArgs d{};
  d.in = in; d.out = out; d.as = scale; d.ab = bias; d.w = w9c; d.pool = pool; d.pool_tot = pool_totals; d.s6 = s6; d.no_act = no_act;
  d.B = B; d.H = H; d.W = W; d.C = C;
  return kerr("dwconv3x3_ex", launch_dwconv3x3(dtype, d, hs(stream)));
}
int llie_dwconv3x3_strip_rows(int dtype, int B, int H, int W, int C) {
  const int cc = dtype == 0 ? 32 : 64;
  if (dtype < 0 || dtype > 2 || B <= 0 || H <= 0 || W <= 0 || C <= 0 || C % cc) return LLIE_ERR_ARG;
  return dw_pick_tyl(B, H, W, C / cc);
}
const char* llie_last_kernel(void) { return last_kernel(); }

// ---- the remaining kernel-level entry points of SURVEY.md 8b (GroupNorm finalize, dense 3x3, linear attention, SE MLP, FiLM)
int llie_groupnorm_finalize(const float* slab0, int ntiles0, int ch0, const float* slab1, int ntiles1, int ch1, int groups, int pixels,
                            const float* gamma, const float* beta, const float* film, int64_t film_stride, float eps, float post_scale,
                            int batch, float* scale_out, float* shift_out, llie_stream stream) {
  if (!slab0 || !gamma || !beta || !scale_out || !shift_out || batch <= 0 || ch0 <= 0 || (slab1 && ch1 <= 0) || groups <= 0 || pixels <= 0 ||
      ntiles0 <= 0 || (slab1 && ntiles1 <= 0) || (ch0 + (slab1 ? ch1 : 0)) % groups)
    return LLIE_ERR_ARG;
  GnFinalizeArgs a{};
  a.src[0] = StatSrc{slab0, ntiles0, ch0};
  if (slab1) a.src[1] = StatSrc{slab1, ntiles1, ch1};
  a.C = ch0 + (slab1 ? ch1 : 0); a.groups = groups; a.P = pixels; a.gamma = gamma; a.beta = beta; a.film = film; a.film_stride = film_stride;
  a.eps = eps; a.as = scale_out; a.ab = shift_out; a.B = batch; a.post_scale = post_scale;
  return kerr("groupnorm_finalize", launch_gn_finalize(a, hs(stream)));
}
// GroupNorm-2 + FiLM affine of the recompute form from the Gram totals llie_gram_stats leaves (gram.hip: gram_finalize_kernel)
int llie_gram_finalize(int dtype, const float* gram_totals, const void* w_expand, int K, int pixels, const float* gamma, const float* beta,
                       const float* film, int64_t film_stride, float eps, float post_scale, int batch, float* scale_out, float* shift_out,
                       llie_stream stream) {
  if (!gram_totals || !w_expand || !gamma || !beta || !scale_out || !shift_out || batch <= 0 || pixels <= 0 || (K != 32 && K != 64 && K != 96) ||
      (dtype != 1 && dtype != 2))
    return LLIE_ERR_ARG;
  GramFinalizeArgs a{};
  a.gtot = gram_totals; a.w1 = w_expand; a.K = K; a.Chid = 4 * K; a.groups = 32; a.P = pixels; a.B = batch; a.gamma = gamma; a.beta = beta;
  a.film = film; a.film_stride = film_stride; a.eps = eps; a.as = scale_out; a.ab = shift_out; a.post_scale = post_scale;
  return kerr("gram_finalize", launch_gram_finalize(dtype, a, hs(stream)));
}
int llie_conv3x3(int dtype, int mode, const void* in, const void* w, const float* bias, void* out, float* stats, int batch, int Hi, int Wi,
                 int Cin, int Cout, llie_stream stream) {
  if (!in || !w || !out || dtype < 0 || dtype > 2 || mode < 0 || mode > 2) return LLIE_ERR_ARG;
  Conv3Args a{};
  a.in = in; a.w = w; a.bias = bias; a.out = out; a.stats = stats; a.B = batch; a.Hi = Hi; a.Wi = Wi; a.Cin = Cin; a.Cout = Cout; a.mode = mode;
  return kerr("conv3x3", launch_conv3x3(dtype, a, hs(stream)));
}
int llie_conv3x3_tiles(int Ho, int Wo) { return conv3x3_ntiles(Ho, Wo); }
int64_t llie_upconv_fold_elems(int C) { return C > 0 ? (int64_t)upconv_fold_elems(C) : LLIE_ERR_ARG; }
int llie_upconv_fold_weights(int dtype, const float* w_oihw, void* folded, int C, llie_stream stream) {
  if (!w_oihw || !folded || C < 1 || (dtype != 1 && dtype != 2)) return LLIE_ERR_ARG;
  return kerr("upconv_fold_weights", launch_upconv_fold(dtype, w_oihw, folded, C, hs(stream)));
}
int llie_conv3x3_upfold(int dtype, const void* in, const void* folded, const float* bias, void* out, float* stats, int batch, int Hi, int Wi,
                        int C, llie_stream stream) {
  if (!in || !folded || !out || (dtype != 1 && dtype != 2)) return LLIE_ERR_ARG;
  Conv3Args a{};
  a.in = in; a.w = folded; a.bias = bias; a.out = out; a.stats = stats; a.B = batch; a.Hi = Hi; a.Wi = Wi; a.Cin = C; a.Cout = C; a.mode = 1;
  return kerr("conv3x3_upfold", launch_conv3x3_upfold(dtype, a, hs(stream)));
}
int llie_conv3x3_upfold_tiles(int Ho, int Wo) { return conv3x3_upfold_ntiles(Ho, Wo); }
int llie_conv3x3_upmaps_grid(int dtype, const void* in, const void* w, const float* bias, void* out, float* stats, int batch, int Hi, int Wi,
                             int C, int workgroups, llie_stream stream) {
  if (!in || !w || !out || (dtype != 1 && dtype != 2) || workgroups < 0) return LLIE_ERR_ARG;
  Conv3Args a{};
  a.in = in; a.w = w; a.bias = bias; a.out = out; a.stats = stats; a.B = batch; a.Hi = Hi; a.Wi = Wi; a.Cin = C; a.Cout = C; a.mode = 1;
  return kerr("conv3x3_upmaps", launch_conv3x3_upmaps(dtype, a, hs(stream), workgroups));
}
int llie_conv3x3_upmaps(int dtype, const void* in, const void* w, const float* bias, void* out, float* stats, int batch, int Hi, int Wi, int C,
                        llie_stream stream) {
  return llie_conv3x3_upmaps_grid(dtype, in, w, bias, out, stats, batch, Hi, Wi, C, 0, stream);
}
int llie_conv3x3_upmaps_workgroups(int batch, int Hi, int Wi, int C) {
  hipError_t e = hipSuccess;
  const int n = conv3x3_upmaps_workgroups(batch, Hi, Wi, C, &e);
  if (e == hipSuccess) return n;
  // a count is positive, so the runtime's own codes (> 0) come back negated; a refused shape is LLIE_ERR_ARG
  const int rc = kerr("conv3x3_upmaps_workgroups", e, LLIE_ERR_ARG, "batch >= 1, Hi % 8 == 0, Wi % 16 == 0, C % 32 == 0");
  return rc < 0 ? rc : -rc;
}
int llie_conv3x3_upmaps_supported(int dtype, int Hi, int Wi, int C) { return conv3x3_upmaps_ok(dtype, Hi, Wi, C) ? 1 : 0; }
int llie_linattn_splits(int N) { return linattn_nsplit(N); }
int llie_pw_expand_nsplit(int M, int N) { return M > 0 && M % 128 == 0 && N > 0 && N % 64 == 0 ? pw_expand_nsplit(M, N) : LLIE_ERR_ARG; }
int llie_linattn(int dtype, const void* qkv, float* kv_scratch, void* out, int batch, int N, int heads, llie_stream stream) {
  if (!qkv || !kv_scratch || !out || dtype < 0 || dtype > 2 || batch <= 0 || N <= 0 || heads <= 0) return LLIE_ERR_ARG;
  AttnArgs a{};
  a.qkv = qkv; a.B = batch; a.N = N; a.heads = heads; a.kv = kv_scratch; a.out = out; a.nsplit = linattn_nsplit(N);
  hipError_t e = launch_linattn_kv(dtype, a, hs(stream));
  if (e == hipSuccess) e = launch_linattn_out(dtype, a, hs(stream));
  return kerr("linattn", e);
}
int llie_se_mlp(int dtype, const float* pool_sums, int pixels, const void* w1, const float* b1, const void* w2, const float* b2, float* mean_scratch,
                float* hidden_scratch, float* gate, int batch, int C, int Cs, llie_stream stream) {
  if (!pool_sums || !w1 || !b1 || !w2 || !b2 || !mean_scratch || !hidden_scratch || !gate || dtype < 0 || dtype > 2 || batch <= 0 || C <= 0 || Cs <= 0)
    return LLIE_ERR_ARG;
  SeArgs a{};
  a.pool = pool_sums; a.ntiles = 1; a.P = pixels; a.w1 = w1; a.b1 = b1; a.w2 = w2; a.b2 = b2; a.mean = mean_scratch; a.hid = hidden_scratch; a.gate = gate;
  a.B = batch; a.C = C; a.Cs = Cs;
  hipError_t e = launch_se_fc1(dtype, a, hs(stream));
  if (e == hipSuccess) e = launch_se_fc2(dtype, a, hs(stream));
  return kerr("se_mlp", e);
}

// ---- the network's first and last kernels, the SE gate of the inference blocks, the attention tail and the layout converters.
// Every contract check runs here, before any HIP call.  The two convs take the reference's OIHW weights: the wrapper zero-fills the
// caller's pack scratch and runs the engine's own repack (launch_load_one with a PK_INIT / PK_FINAL descriptor) before the launch.
static int64_t align16(int64_t n) { return (n + 15) & ~(int64_t)15; }
static bool conv_sizes_ok(int B, int H, int W) { return B > 0 && B <= 65535 && H > 0 && W > 0 && H % 8 == 0 && W % 8 == 0; }
int64_t llie_init_conv_pack_bytes(int Cin, int Cout) {
  if (Cin < 1 || Cin > 8 || Cout <= 0 || Cout % 32) return LLIE_ERR_ARG;
  return align16((int64_t)Cin * 9 * Cout * 4) + (int64_t)10 * Cout * 8 * 2;  // fp32 [Cin * 9][Cout], then the MFMA pack [10][Cout][8] T
}
int64_t llie_final_conv_pack_bytes(int C) {
  if (C <= 0 || C % 32) return LLIE_ERR_ARG;
  return (int64_t)9 * C * 4 * 4 + (int64_t)(C / 32) * 18 * 2 * 4 * 8 * 2;  // fp32 [9][C][4], then the MFMA pack [C / 32][18][2][4][8] T
}
int llie_init_conv_tiles(int H, int W, int mfma) { return H > 0 && W > 0 && H % 8 == 0 && W % 8 == 0 ? init_conv_ntiles(H, W, mfma != 0) : LLIE_ERR_ARG; }
int llie_init_conv(int dtype, const float* x0, int c0, const float* x1, int c1, const float* w_oihw, const float* bias, void* out, float* stats,
                   int batch, int H, int W, int Cout, int use_mfma, void* pack, int64_t pack_bytes, llie_stream stream) {
  if (!dtype_ok(dtype) || !x0 || !w_oihw || !bias || !out || !pack || ((uintptr_t)pack & 15) || c0 < 1 || c1 < 0 || c0 + c1 > 8 ||
      (c1 > 0) != (x1 != nullptr) || !conv_sizes_ok(batch, H, W) || Cout <= 0 || Cout % 32 || use_mfma < 0 || use_mfma > 1 ||
      (use_mfma && dtype == 0) || pack_bytes < llie_init_conv_pack_bytes(c0 + c1, Cout))
    return LLIE_ERR_ARG;
  const int Cin = c0 + c1;
  const int64_t need = llie_init_conv_pack_bytes(Cin, Cout), off = align16((int64_t)Cin * 9 * Cout * 4);
  char* blob = reinterpret_cast<char*>(pack);
  LoadDesc d{};
  d.src = w_oihw; d.kind = PK_INIT; d.O = Cout; d.I = Cin; d.Op = Cout; d.Ip = Cin; d.numel = (long long)Cout * Cin * 9;
  d.dst = 0; d.dst_t = use_mfma ? off : -1; d.dst_f = -1;
  InitConvArgs a{};
  a.x0 = x0; a.x1 = x1; a.c0 = c0; a.c1 = c1; a.w = reinterpret_cast<const float*>(blob); a.bias = bias; a.wp = use_mfma ? blob + off : nullptr;
  a.out = out; a.stats = stats; a.B = batch; a.H = H; a.W = W; a.Cout = Cout;
  hipStream_t s = hs(stream);
  hipError_t e = launch_fill_zero(blob, need, s);
  if (e == hipSuccess) e = launch_load_one(dtype, d, blob, s);
  if (e == hipSuccess) e = launch_init_conv(dtype, a, s);
  return kerr("init_conv", e);
}
// the data gradient of init_conv on the forward VALU kernel's fp32 table, repacked from OIHW as above (the MFMA pack is not built)
int llie_init_conv_dgrad(int dtype, const void* g, int Cout, const float* w_oihw, float* d_x0, int c0, float* d_x1, int c1, int batch,
                         int H, int W, void* pack, int64_t pack_bytes, llie_stream stream) {
  if (!dtype_ok(dtype) || !g || !w_oihw || !pack || ((uintptr_t)pack & 15) || c0 < 1 || c1 < 0 || c0 + c1 > 8 || (!d_x0 && !d_x1) ||
      (d_x1 && c1 == 0) || !conv_sizes_ok(batch, H, W) || Cout <= 0 || Cout % 32 || pack_bytes < llie_init_conv_pack_bytes(c0 + c1, Cout))
    return LLIE_ERR_ARG;
  const int Cin = c0 + c1;
  char* blob = reinterpret_cast<char*>(pack);
  LoadDesc d{};
  d.src = w_oihw; d.kind = PK_INIT; d.O = Cout; d.I = Cin; d.Op = Cout; d.Ip = Cin; d.numel = (long long)Cout * Cin * 9;
  d.dst = 0; d.dst_t = -1; d.dst_f = -1;
  InitDgradArgs a{};
  a.g = g; a.w = reinterpret_cast<const float*>(blob); a.dx0 = d_x0; a.dx1 = d_x1; a.c0 = c0; a.c1 = c1;
  a.B = batch; a.H = H; a.W = W; a.C0 = Cout;
  hipStream_t s = hs(stream);
  hipError_t e = launch_fill_zero(blob, llie_init_conv_pack_bytes(Cin, Cout), s);
  if (e == hipSuccess) e = launch_load_one(dtype, d, blob, s);
  if (e == hipSuccess) e = launch_init_conv_dgrad(dtype, a, s);
  return kerr("init_conv_dgrad", e);
}
int llie_final_conv(int dtype, const void* in, const float* scale, const float* shift, const float* w_oihw, const float* bias, float* out,
                    int batch, int H, int W, int C, int Cout, int use_mfma, const llie_step_coef* coef, const float* sample, const float* noise,
                    float* prev, float* clamped, void* pack, int64_t pack_bytes, llie_stream stream) {
  if (!dtype_ok(dtype) || !in || !scale || !shift || !w_oihw || !bias || !pack || ((uintptr_t)pack & 15) || !conv_sizes_ok(batch, H, W) ||
      C <= 0 || C % 32 || Cout < 1 || Cout > 4 || use_mfma < 0 || use_mfma > 1 || (use_mfma && dtype == 0) ||
      pack_bytes < llie_final_conv_pack_bytes(C))
    return LLIE_ERR_ARG;
  // the scheduler step lives in the MFMA kernel's epilogue alone; without it the noise prediction is the only output
  if (coef ? (!use_mfma || !sample || !prev || !step_coef_ok(*coef) || (!coef->is_last && !coef->sampler && !noise)) : (!out || sample || noise || prev || clamped)) return LLIE_ERR_ARG;
  const int64_t need = llie_final_conv_pack_bytes(C), off = (int64_t)9 * C * 4 * 4;
  char* blob = reinterpret_cast<char*>(pack);
  LoadDesc d{};
  d.src = w_oihw; d.kind = PK_FINAL; d.O = Cout; d.I = C; d.Op = Cout; d.Ip = C; d.numel = (long long)Cout * C * 9;
  d.dst = 0; d.dst_t = use_mfma ? off : -1; d.dst_f = -1;
  FinalConvArgs a{};
  a.in = in; a.as = scale; a.ab = shift; a.w = reinterpret_cast<const float*>(blob); a.bias = bias; a.wp = use_mfma ? blob + off : nullptr;
  a.out = out; a.B = batch; a.H = H; a.W = W; a.C = C; a.Cout = Cout;
  if (coef) {
    a.fuse_step = 1;
    a.coef = step_coef(*coef);
    a.sample = sample; a.noise = noise; a.prev = prev; a.clamped = clamped;
  }
  hipStream_t s = hs(stream);
  hipError_t e = launch_fill_zero(blob, need, s);
  if (e == hipSuccess) e = launch_load_one(dtype, d, blob, s);
  if (e == hipSuccess) e = launch_final_conv(dtype, a, s);
  return kerr("final_conv", e);
}
// the SE gate from the depthwise kernels' fixed-point totals, by each path Run::se_gate can take: 0 se_gate_kernel, 1 se_fc1 + se_fc2
// reading the totals, 2 the MFMA pair (2-byte types)
int llie_se_gate(int dtype, const unsigned long long* totals, int pixels, const void* w1, const float* b1, const void* w2, const float* b2,
                 float* gate, int batch, int C, int Cs, int path, float* hidden_scratch, long long* pre_scratch, llie_stream stream) {
  if (!dtype_ok(dtype) || !totals || !w1 || !b1 || !w2 || !b2 || !gate || pixels <= 0 || batch <= 0 || C <= 0 || Cs <= 0 || path < 0 || path > 2)
    return LLIE_ERR_ARG;
  SeArgs a{};
  a.tot = totals; a.ntiles = 1; a.P = pixels; a.w1 = w1; a.b1 = b1; a.w2 = w2; a.b2 = b2; a.hid = hidden_scratch; a.pre = pre_scratch; a.gate = gate;
  a.B = batch; a.C = C; a.Cs = Cs;
  hipStream_t s = hs(stream);
  if (path == 0) {
    if (C % (dtype == 0 ? 64 : 128) || (int64_t)(C + Cs) * 4 > 48 * 1024) return LLIE_ERR_ARG;
    return kerr("se_gate", launch_se_gate(dtype, a, s));
  }
  if (path == 1) {
    if (!hidden_scratch || C > 4096 || Cs > 4096) return LLIE_ERR_ARG;  // four images' rows in 64 KB of LDS
    hipError_t e = launch_se_fc1(dtype, a, s);
    if (e == hipSuccess) e = launch_se_fc2(dtype, a, s);
    return kerr("se_gate", e);
  }
  if (!pre_scratch || !se_mlp_mfma_supported(dtype, a)) return LLIE_ERR_ARG;
  hipError_t e = launch_fill_zero(pre_scratch, (int64_t)batch * Cs * 8, s);  // the kernel's contract: zero at launch
  if (e == hipSuccess) e = launch_se_mlp_mfma(dtype, a, s);
  return kerr("se_gate", e);
}
int llie_affine_add(int dtype, const void* x, const float* scale, const float* shift, const void* res, void* y, float* stats, int M, int C, int P,
                    llie_stream stream) {
  if (!dtype_ok(dtype) || !x || !scale || !shift || !y || M <= 0 || P <= 0 || M % P || C <= 0 || C % 8 || C > 2048) return LLIE_ERR_ARG;
  AffineAddArgs a{};
  a.x = x; a.as = scale; a.ab = shift; a.res = res; a.y = y; a.stats = stats; a.M = M; a.C = C; a.P = P;
  return kerr("affine_add", launch_affine_add(dtype, a, hs(stream)));
}
int llie_nchw_to_nhwc(int dtype, const float* x, void* y, float* stats, int batch, int C, int P, int Csrc, int coff, llie_stream stream) {
  if (!dtype_ok(dtype) || !x || !y || batch <= 0 || C <= 0 || C % 32 || P <= 0 || P % 64 || coff < 0 || Csrc < coff + C || batch > 65535 || C / 32 > 65535)
    return LLIE_ERR_ARG;
  return kerr("nchw_to_nhwc", launch_nchw_to_nhwc(dtype, x, y, stats, batch, C, P, Csrc, coff, hs(stream)));
}
int llie_nhwc_to_nchw(int dtype, const void* x, float* y, int batch, int C, int P, int Cdst, int coff, llie_stream stream) {
  if (!dtype_ok(dtype) || !x || !y || batch <= 0 || C <= 0 || C % 32 || P <= 0 || P % 64 || coff < 0 || Cdst < coff + C || batch > 65535 || C / 32 > 65535)
    return LLIE_ERR_ARG;
  return kerr("nhwc_to_nchw", launch_nhwc_to_nchw(dtype, x, y, batch, C, P, hs(stream), Cdst, coff));
}
int llie_film(const float* silu_temb, const float* wf, const float* bf, float* film, int rows, int T, int F, llie_stream stream) {
  if (!silu_temb || !wf || !bf || !film || rows <= 0 || T <= 0 || F <= 0) return LLIE_ERR_ARG;
  FilmArgs a{};
  a.silu_temb = silu_temb; a.rows = rows; a.T = T; a.wf = wf; a.bf = bf; a.film = film; a.F = F;
  return kerr("film", launch_film(a, hs(stream)));
}
int llie_silu_rows(const float* in, float* out, int64_t n, llie_stream stream) {
  if (!in || !out || n <= 0 || n > (int64_t)0x7fffffff * 256) return LLIE_ERR_ARG;
  return kerr("silu_rows", launch_silu_rows(in, out, n, hs(stream)));
}

// ---- backward kernels (training): thin wrappers over the launch API; every contract check runs here, before any HIP call
static int wgrad_rule(int dtype, int batch, int pixels, int N, int K, int ntap, int ragged_rule) {
  const int M = wgrad_rows(batch, pixels);
  return ragged_rule ? wgrad_msplit_ragged(dtype, M, N, K, ntap) : wgrad_msplit(dtype, M, N, K, ntap);
}
int llie_wgrad_msplit(int dtype, int batch, int pixels, int N, int K, int ntap, int ragged_rule) {
  if (!dtype_ok(dtype) || batch <= 0 || pixels <= 0 || N <= 0 || K <= 0 || (ntap != 1 && ntap != 9)) return LLIE_ERR_ARG;
  return wgrad_rule(dtype, batch, pixels, N, K, ntap, ragged_rule);
}
int64_t llie_wgrad_partial_floats(int msplit, int N, int K, int ntap) {
  if (msplit <= 0 || N <= 0 || K <= 0 || (ntap != 1 && ntap != 9)) return LLIE_ERR_ARG;
  return (int64_t)msplit * ntap * N * K;
}
int llie_wgrad(int dtype, const void* g, int N, const llie_gemm_seg* segs, int nseg, int batch, int Ho, int Wo, int Hi, int Wi, int stride,
               int dy, int dx, int ntap, int nstore, int kstore, float* partial, int64_t partial_floats, float* out, int64_t ldn, int64_t ldk,
               int64_t off, int msplit, llie_stream stream) {
  if (!dtype_ok(dtype) || !g || !segs || !partial || !out || nseg < 1 || nseg > 3 || N <= 0 || N % 32 || batch <= 0 || Ho <= 0 ||
      Wo <= 0 || Hi <= 0 || Wi <= 0 || (stride != 1 && stride != 2) || (ntap != 1 && ntap != 9) || dy < -1 || dy > 1 || dx < -1 ||
      dx > 1 || msplit < 0 || ldn < 0 || ldk < 0 || off < 0)
    return LLIE_ERR_ARG;
  WgradArgs a{};
  a.nseg = nseg;
  for (int i = 0; i < nseg; ++i) {
    const llie_gemm_seg& sg = segs[i];
    if (!sg.ptr || sg.channels <= 0 || sg.channels % 32 || sg.act < ACT_NONE || sg.act > ACT_SILU || (sg.bias && !sg.scale) ||
        (sg.scale && sg.affine_ld < sg.channels))
      return LLIE_ERR_ARG;
  }
  a.K = to_segs(segs, nseg, a.seg);
  // the output pixel grid must lie inside the input's (stride-s conv with pad 1 or a 1x1 tap)
  if (nstore < 0 || nstore > N || kstore < 0 || kstore > a.K || (Ho - 1) * stride >= Hi || (Wo - 1) * stride >= Wi) return LLIE_ERR_ARG;
  const int P = Ho * Wo, M = wgrad_rows(batch, P);
  const int ms = msplit ? msplit : wgrad_rule(dtype, batch, P, N, a.K, ntap, P % 64 != 0);
  if (ms > M / 64 || partial_floats < (int64_t)ms * ntap * N * a.K) return LLIE_ERR_ARG;
  a.g = g; a.N = N; a.B = batch; a.Ho = Ho; a.Wo = Wo; a.Hi = Hi; a.Wi = Wi; a.stride = stride; a.dy = dy; a.dx = dx;
  a.ntap = ntap; a.nstore = nstore; a.kstore = kstore; a.partial = partial; a.out = out; a.ldn = ldn; a.ldk = ldk; a.off = off; a.msplit = ms;
  return kerr("wgrad", launch_wgrad(dtype, a, hs(stream)));
}
int llie_dw_wgrad_strips(int H, int W) { return H > 0 && W > 0 ? dw_wgrad_strips(H, W) : LLIE_ERR_ARG; }
int llie_dw_wgrad(int dtype, const void* g, const float* gs, const float* gb, const void* h, const float* as, const float* ab, float* partial,
                  float* out, int batch, int H, int W, int C, llie_stream stream) {
  if (!dtype_ok(dtype) || !g || !h || !as || !ab || !partial || !out || batch <= 0 || H <= 0 || W <= 0 || C <= 0 || C % (dtype == 0 ? 32 : 64))
    return LLIE_ERR_ARG;
  DwWgradArgs a{};
  a.g = g; a.gs = gs; a.gb = gb; a.h = h; a.as = as; a.ab = ab; a.partial = partial; a.out = out; a.B = batch; a.H = H; a.W = W; a.C = C;
  return kerr("dw_wgrad", launch_dw_wgrad(dtype, a, hs(stream)));
}
int64_t llie_groupnorm_backward_scratch_floats(int batch, int C, int pixels) {
  if (batch <= 0 || C <= 0 || pixels <= 0) return LLIE_ERR_ARG;
  return (int64_t)batch * C * (2 * ((pixels + 63) / 64) + 7);  // slab, S, A, Bq, Cq, dG, dBc
}
}  // extern "C"
// one norm site on launch_gn_site_bwd: slab NULL = the site's own mask-and-reduce pass writes dz and the tile partials into the head
// of `scratch`; otherwise the producer's slab of `ntiles` tiles per image is summed as it stands (slab_ready)
static int gn_site_call(const char* what, int dtype, const llie_gn_backward_args* a, float* slab, int ntiles, float* scratch,
                        int64_t scratch_floats, llie_stream stream) {
  if (!dtype_ok(dtype) || !a || !scratch) return LLIE_ERR_ARG;
  const int C = a->c0 + a->c1;
  if (!a->g || !a->x0 || !a->dx0 || !a->scale || !a->shift || !a->mean || !a->rstd || !a->gamma || !a->beta || !a->dgamma || !a->dbeta ||
      a->act < ACT_NONE || a->act > ACT_SILU || (a->act != ACT_NONE && !a->dz) || a->batch <= 0 || a->pixels <= 0 || a->c0 <= 0 ||
      a->c0 % 32 || a->c1 < 0 || a->c1 % 32 || (a->c1 && (!a->x1 || !a->dx1)) || (!a->c1 && (a->x1 || a->dx1 || a->add1_1)) ||
      (a->dfilm && !a->film) || (a->film && a->film_stride < 0) || (a->dfilm && a->dfilm_stride < 2 * C) ||
      (int64_t)a->batch * a->pixels * C / (dtype == 0 ? 4 : 8) >= (1ll << 31))
    return LLIE_ERR_ARG;
  // a producer's slab: the mask is already applied, so g is dz
  if (slab && (ntiles <= 0 || a->act == ACT_NONE || a->dz != a->g)) return LLIE_ERR_ARG;
  const int nt = slab ? ntiles : (a->pixels + 63) / 64;
  const size_t bc = (size_t)a->batch * C;
  if (scratch_floats < (int64_t)(bc * (slab ? 7 : 2 * (size_t)nt + 7))) return LLIE_ERR_ARG;
  GnSiteArgs s{};
  s.g = a->g; s.dz = a->act == ACT_NONE ? nullptr : a->dz; s.x0 = a->x0; s.x1 = a->x1; s.c0 = a->c0; s.c1 = a->c1;
  s.as = a->scale; s.ab = a->shift; s.act = a->act; s.mean = a->mean; s.rstd = a->rstd; s.gamma = a->gamma; s.beta = a->beta;
  s.film = a->film; s.film_stride = a->film_stride; s.dfilm = a->dfilm; s.dfilm_stride = a->dfilm_stride; s.dgamma = a->dgamma; s.dbeta = a->dbeta;
  s.slab = slab ? slab : scratch; s.ntiles = nt; s.slab_ready = slab ? 1 : 0;
  s.S = slab ? scratch : scratch + bc * 2 * nt; s.A = s.S + 2 * bc; s.Bq = s.A + bc; s.Cq = s.Bq + bc; s.dG = s.Cq + bc; s.dBc = s.dG + bc;
  s.add0 = a->add0; s.add1_0 = a->add1_0; s.add1_1 = a->add1_1; s.dx0 = a->dx0; s.dx1 = a->dx1; s.B = a->batch; s.P = a->pixels;
  return kerr(what, launch_gn_site_bwd(dtype, s, hs(stream)));
}
extern "C" {
int llie_groupnorm_backward(int dtype, const llie_gn_backward_args* a, float* scratch, int64_t scratch_floats, llie_stream stream) {
  return gn_site_call("groupnorm_backward", dtype, a, nullptr, 0, scratch, scratch_floats, stream);
}
int llie_groupnorm_backward_from_slab(int dtype, const llie_gn_backward_args* a, float* slab, int ntiles, float* scratch,
                                      int64_t scratch_floats, llie_stream stream) {
  if (!slab) return LLIE_ERR_ARG;
  return gn_site_call("groupnorm_backward_from_slab", dtype, a, slab, ntiles, scratch, scratch_floats, stream);
}
int64_t llie_linattn_dkv_floats(int batch, int N, int heads) {
  if (batch <= 0 || N <= 0 || heads <= 0) return LLIE_ERR_ARG;
  return (int64_t)batch * heads * ((N + 63) / 64 + 1) * 32 * 33;  // tile partials, then their sum
}
int llie_linattn_backward(int dtype, const void* qkv, const float* kv_scratch, const void* dout, void* dqkv, float* dkv_scratch,
                          int64_t dkv_floats, int batch, int N, int heads, llie_stream stream) {
  if (!dtype_ok(dtype) || !qkv || !kv_scratch || !dout || !dqkv || !dkv_scratch || batch <= 0 || N <= 0 || heads <= 0 ||
      dkv_floats < llie_linattn_dkv_floats(batch, N, heads))
    return LLIE_ERR_ARG;
  AttnBwdArgs a{};
  a.qkv = qkv; a.dout = dout; a.dqkv = dqkv; a.kv = kv_scratch; a.nsplit = linattn_nsplit(N); a.dkv = dkv_scratch;
  a.B = batch; a.N = N; a.heads = heads;
  float* tot = dkv_scratch + (size_t)batch * heads * ((N + 63) / 64) * 32 * 33;
  return kerr("linattn_backward", launch_linattn_bwd(dtype, a, tot, hs(stream)));
}
int llie_softattn(int dtype, const void* qkv, void* out, float* lse_or_NULL, int batch, int N, int heads, llie_stream stream) {
  if (!dtype_ok(dtype) || !qkv || !out || batch <= 0 || N <= 0 || heads <= 0) return LLIE_ERR_ARG;
  SoftAttnArgs a{};
  a.qkv = qkv; a.out = out; a.lse = lse_or_NULL; a.B = batch; a.N = N; a.heads = heads;
  return kerr("softattn", launch_softattn_fwd(dtype, a, hs(stream)));
}
int64_t llie_softattn_bwd_floats(int batch, int N, int heads) {
  if (batch <= 0 || N <= 0 || heads <= 0) return LLIE_ERR_ARG;
  return (int64_t)batch * heads * N;  // delta per query
}
int llie_softattn_backward(int dtype, const void* qkv, const void* out, const void* dout, const float* lse, void* dqkv, float* scratch,
                           int64_t scratch_floats, int batch, int N, int heads, llie_stream stream) {
  if (!dtype_ok(dtype) || !qkv || !out || !dout || !lse || !dqkv || !scratch || batch <= 0 || N <= 0 || heads <= 0 ||
      scratch_floats < llie_softattn_bwd_floats(batch, N, heads))
    return LLIE_ERR_ARG;
  SoftAttnBwdArgs a{};
  a.qkv = qkv; a.out = out; a.dout = dout; a.lse = lse; a.dqkv = dqkv; a.delta = scratch; a.B = batch; a.N = N; a.heads = heads;
  return kerr("softattn_backward", launch_softattn_bwd(dtype, a, hs(stream)));
}
int llie_upsample2x_backward(int dtype, const void* dout, void* din, int batch, int Hi, int Wi, int C, llie_stream stream) {
  if (!dtype_ok(dtype) || !dout || !din || batch <= 0 || Hi <= 0 || Wi <= 0 || C <= 0 || C % (dtype == 0 ? 4 : 8)) return LLIE_ERR_ARG;
  return kerr("upsample2x_backward", launch_upsample2x_bwd(dtype, dout, din, batch, Hi, Wi, C, hs(stream)));
}
int llie_dilate2x(int dtype, const void* in, void* out, int batch, int Hi, int Wi, int C, llie_stream stream) {
  if (!dtype_ok(dtype) || !in || !out || batch <= 0 || Hi <= 0 || Wi <= 0 || C <= 0 || C % (dtype == 0 ? 4 : 8)) return LLIE_ERR_ARG;
  return kerr("dilate2x", launch_dilate2x(dtype, in, out, batch, Hi, Wi, C, hs(stream)));
}
int64_t llie_linear_dx_scratch_floats(int batch, int R, int Kc) {
  if (batch <= 0 || R <= 0 || Kc <= 0) return LLIE_ERR_ARG;
  return (int64_t)linear_dx_chunks(R) * batch * Kc;
}
int llie_linear_dx(int wdtype, const float* dy, int64_t dy_stride, const void* w, float* dx, int batch, int R, int Kc, float* scratch,
                   int64_t scratch_floats, llie_stream stream) {
  if (!dtype_ok(wdtype) || !dy || !w || !dx || batch <= 0 || R <= 0 || Kc <= 0 || dy_stride < R ||
      (scratch && scratch_floats < llie_linear_dx_scratch_floats(batch, R, Kc)))
    return LLIE_ERR_ARG;
  return kerr("linear_dx", launch_linear_dx(wdtype, dy, dy_stride, w, dx, batch, R, Kc, hs(stream), scratch));
}
int llie_linear_dw(const float* dy, int64_t dy_stride, const float* x, float* dw, float* db, int batch, int R, int Kc, llie_stream stream) {
  if (!dy || !x || !dw || batch <= 0 || R <= 0 || Kc <= 0 || dy_stride < R) return LLIE_ERR_ARG;
  return kerr("linear_dw", launch_linear_dw(dy, dy_stride, x, dw, db, batch, R, Kc, hs(stream)));
}
int llie_final_bwd_data(int dtype, const float* deps, const float* w, void* da, int batch, int H, int W, int C, int Cout, llie_stream stream) {
  if (!dtype_ok(dtype) || !deps || !w || !da || batch <= 0 || H <= 0 || W <= 0 || C <= 0 || C % 8 || Cout < 1 || Cout > 4) return LLIE_ERR_ARG;
  FinalBwdArgs a{};
  a.deps = deps; a.w = w; a.da = da; a.B = batch; a.H = H; a.W = W; a.C = C; a.Cout = Cout;
  return kerr("final_bwd_data", launch_final_bwd_data(dtype, a, hs(stream)));
}
// the depthwise input gradient as Back::irb_bwd launches it: the forward kernel's body with flipped taps, the affine-only prologue,
// the ReLU6 mask of the forward pre-activation and the norm-2 partial sums in the epilogue
int llie_dwconv3x3_backward(int dtype, const void* g, const float* gs, const float* gb, const float* w9c_flipped, const void* bx,
                            const float* bas, const float* bab, void* dz_out, float* slab, int B, int H, int W, int C, llie_stream stream) {
  if (!dtype_ok(dtype) || !g || !gs || !gb || !w9c_flipped || !bx || !bas || !bab || !dz_out || !slab || B <= 0 || H <= 0 || W <= 0 ||
      C <= 0 || C % (dtype == 0 ? 32 : 64))
    return LLIE_ERR_ARG;
  DwArgs d{};
  d.in = g; d.out = dz_out; d.as = gs; d.ab = gb; d.w = w9c_flipped; d.pool = nullptr; d.B = B; d.H = H; d.W = W; d.C = C; d.no_act = 1;
  d.bx = bx; d.bas = bas; d.bab = bab; d.bslab = slab;
  return kerr("dwconv3x3_backward", launch_dwconv3x3(dtype, d, hs(stream)));
}
int llie_bias_grad_floats(int batch, int C, int pixels, int64_t* slab_floats, int64_t* s_floats) {
  if (batch <= 0 || C <= 0 || pixels <= 0 || !slab_floats || !s_floats) return LLIE_ERR_ARG;
  *slab_floats = (int64_t)batch * bias_grad_tiles(pixels) * 2 * C;
  *s_floats = (int64_t)batch * C;
  return LLIE_OK;
}
int llie_bias_grad(int dtype, const void* g, int M, int C, int P, int Cstore, float* slab, float* S, float* out, llie_stream stream) {
  if (!dtype_ok(dtype) || !g || !slab || !S || !out || P <= 0 || M < P || M % P || C <= 0 || C % 32 || Cstore < 1 || Cstore > C) return LLIE_ERR_ARG;
  return kerr("bias_grad", launch_bias_grad(dtype, g, M, C, P, Cstore, slab, S, out, hs(stream)));
}
int llie_pack_planes(int dtype, const float* x0, int c0, const float* x1, int c1, void* out, int batch, int pixels, llie_stream stream) {
  if (!dtype_ok(dtype) || !x0 || !out || c0 < 1 || c1 < 0 || c0 + c1 > 8 || (c1 > 0) != (x1 != nullptr) || batch <= 0 || pixels <= 0) return LLIE_ERR_ARG;
  return kerr("pack_planes", launch_pack_planes(dtype, x0, x1, c0, c1, out, batch, pixels, hs(stream)));
}
int llie_add_into(int dtype, void* dst, const void* src, int64_t n, llie_stream stream) {
  if (!dtype_ok(dtype) || !dst || !src || n <= 0 || n % (dtype == 0 ? 4 : 8)) return LLIE_ERR_ARG;
  return kerr("add_into", launch_add_into(dtype, dst, src, n, hs(stream)));
}
int llie_sin_embed(const int64_t* t, const float* freqs, float* emb, int rows, int dim, llie_stream stream) {
  if (!t || !freqs || !emb || rows <= 0 || dim < 2 || dim % 2) return LLIE_ERR_ARG;
  return kerr("sin_embed", launch_sin_embed(t, freqs, emb, rows, dim, hs(stream)));
}
int llie_pointwise_backward(int kind, const float* a, const float* b, float* out, int64_t n, float scale, llie_stream stream) {
  if (kind < LLIE_PW_SIGMOID_BWD || kind > LLIE_PW_SCALE || !a || !out || n <= 0 || (kind != LLIE_PW_SCALE && !b)) return LLIE_ERR_ARG;
  hipStream_t s = hs(stream);
  switch (kind) {
    case LLIE_PW_SIGMOID_BWD: return kerr("pointwise_backward", launch_sigmoid_bwd(a, b, out, n, s));
    case LLIE_PW_RELU6_BWD: return kerr("pointwise_backward", launch_relu6_bwd(a, b, out, n, s));
    case LLIE_PW_SILU_BWD: return kerr("pointwise_backward", launch_silu_bwd(a, b, out, n, s));
  }
  return kerr("pointwise_backward", launch_scale_rows(a, out, n, scale, s));
}

int llie_preprocess_u8(const uint8_t* img, int batch, int H0, int W0, float* out, int S, llie_stream stream) {
  if (!img || !out) return LLIE_ERR_ARG;
  return kerr("preprocess_u8", launch_preprocess_u8(img, batch, H0, W0, out, S, hs(stream)), LLIE_ERR_ARG, nullptr);
}
int llie_postprocess_u8(const float* x, int batch, int S, uint8_t* img, int H0, int W0, llie_stream stream) {
  if (!img || !x) return LLIE_ERR_ARG;
  return kerr("postprocess_u8", launch_postprocess_u8(x, batch, S, img, H0, W0, hs(stream)), LLIE_ERR_ARG, nullptr);
}

int llie_tile_count(int L, int S, int v) {
  if (!tile_plan_ok(L, L, S, S, v, v)) return LLIE_ERR_ARG;
  return tile_axis_count(L, S, v);
}
int llie_tile_origins(int L, int S, int v, int* out) {
  if (!out || !tile_plan_ok(L, L, S, S, v, v)) return LLIE_ERR_ARG;
  const int n = tile_axis_count(L, S, v);
  for (int i = 0; i < n; ++i) out[i] = tile_axis_origin(i, L, S, n);
  return LLIE_OK;
}
int llie_tile_gather_u8_hw(const uint8_t* img, int H, int W, int SH, int SW, int vy, int vx, int first, int count, float* tiles,
                           llie_stream stream) {
  if (!img || !tiles) return LLIE_ERR_ARG;
  return kerr("tile_gather_u8", launch_tile_gather_u8(img, TilePlan{H, W, SH, SW, vy, vx, first, count}, tiles, hs(stream)), LLIE_ERR_ARG,
              nullptr);
}
int llie_tile_gather_f32_hw(const float* canvas, int planes, int H, int W, int SH, int SW, int vy, int vx, int first, int count, float* out,
                            llie_stream stream) {
  if (!canvas || !out) return LLIE_ERR_ARG;
  return kerr("tile_gather_f32", launch_tile_gather_f32(canvas, planes, TilePlan{H, W, SH, SW, vy, vx, first, count}, out, hs(stream)),
              LLIE_ERR_ARG, nullptr);
}
int llie_tile_blend_u8_hw(const float* tiles, int H, int W, int SH, int SW, int vy, int vx, uint8_t* img, llie_stream stream) {
  if (!tiles || !img) return LLIE_ERR_ARG;
  return kerr("tile_blend_u8", launch_tile_blend_u8(tiles, TilePlan{H, W, SH, SW, vy, vx, 0, 1}, img, hs(stream)), LLIE_ERR_ARG, nullptr);
}
int llie_tile_sync_step_hw(const float* eps_tiles, int H, int W, int SH, int SW, int vy, int vx, const float* canvas_in, const float* noise,
                           const llie_step_coef* k, float* canvas_out, uint8_t* img, llie_stream stream) {
  if (!eps_tiles || !canvas_in || !k || !canvas_out || !step_coef_ok(*k)) return LLIE_ERR_ARG;
  const StepCoef c = step_coef(*k);
  return kerr("tile_sync_step",
              launch_tile_sync_step(eps_tiles, TilePlan{H, W, SH, SW, vy, vx, 0, 1}, canvas_in, noise, c, canvas_out, img, hs(stream)),
              LLIE_ERR_ARG, nullptr);
}
// the square entries: the same launchers at SH = SW = S, vy = vx = v
int llie_tile_gather_u8(const uint8_t* img, int H, int W, int S, int v, int first, int count, float* tiles, llie_stream stream) {
  return llie_tile_gather_u8_hw(img, H, W, S, S, v, v, first, count, tiles, stream);
}
int llie_tile_gather_f32(const float* canvas, int planes, int H, int W, int S, int v, int first, int count, float* out, llie_stream stream) {
  return llie_tile_gather_f32_hw(canvas, planes, H, W, S, S, v, v, first, count, out, stream);
}
int llie_tile_blend_u8(const float* tiles, int H, int W, int S, int v, uint8_t* img, llie_stream stream) {
  return llie_tile_blend_u8_hw(tiles, H, W, S, S, v, v, img, stream);
}
int llie_tile_sync_step(const float* eps_tiles, int H, int W, int S, int v, const float* canvas_in, const float* noise,
                        const llie_step_coef* k, float* canvas_out, uint8_t* img, llie_stream stream) {
  return llie_tile_sync_step_hw(eps_tiles, H, W, S, S, v, v, canvas_in, noise, k, canvas_out, img, stream);
}

int llie_frame_pad(int L) { return L > 0 && L <= (1 << 24) ? frame_pad(L) : LLIE_ERR_ARG; }
int llie_frame_load_u8(const uint8_t* img, int H, int W, float* out, llie_stream stream) {
  if (!img || !out) return LLIE_ERR_ARG;
  return kerr("frame_load_u8", launch_frame_load_u8(img, H, W, out, hs(stream)), LLIE_ERR_ARG, nullptr);
}
int llie_frame_store_u8(const float* x, int H, int W, uint8_t* img, llie_stream stream) {
  if (!x || !img) return LLIE_ERR_ARG;
  return kerr("frame_store_u8", launch_frame_store_u8(x, H, W, img, hs(stream)), LLIE_ERR_ARG, nullptr);
}

static_assert(sizeof(llie_aug_row) == sizeof(AugRow) && sizeof(AugRow) == 48, "llie_aug_row and AugRow are one layout");
static AugArgs aug_args(const uint8_t* pool, const int64_t* table, int N, const llie_aug_row* plan, int first, int count, int SH, int SW,
                        const float* z, float* low, float* high, uint8_t* low_u8, uint8_t* high_u8) {
  AugArgs a{};
  a.pool = pool; a.table = table; a.N = N; a.plan = reinterpret_cast<const AugRow*>(plan); a.first = first; a.count = count;
  a.SH = SH; a.SW = SW;
  a.z = z; a.low = low; a.high = high; a.low_u8 = low_u8; a.high_u8 = high_u8;
  return a;
}
int llie_aug_pair_u8_hw(const uint8_t* pool, const int64_t* table, int N, const llie_aug_row* plan, int first, int count, int SH, int SW,
                        float* low, float* high, uint8_t* low_u8, uint8_t* high_u8, llie_stream stream) {
  return kerr("aug_pair_u8", launch_aug_pair_u8(aug_args(pool, table, N, plan, first, count, SH, SW, nullptr, low, high, low_u8, high_u8), hs(stream)),
              LLIE_ERR_ARG, nullptr);
}
int llie_aug_synth_u8_hw(const uint8_t* pool, const int64_t* table, int N, const llie_aug_row* plan, int first, int count, int SH, int SW,
                         const float* z, float* low, float* high, uint8_t* low_u8, uint8_t* high_u8, llie_stream stream) {
  return kerr("aug_synth_u8", launch_aug_synth_u8(aug_args(pool, table, N, plan, first, count, SH, SW, z, low, high, low_u8, high_u8), hs(stream)),
              LLIE_ERR_ARG, nullptr);
}
int llie_aug_pair_u8(const uint8_t* pool, const int64_t* table, int N, const llie_aug_row* plan, int first, int count, int S,
                     float* low, float* high, uint8_t* low_u8, uint8_t* high_u8, llie_stream stream) {
  return llie_aug_pair_u8_hw(pool, table, N, plan, first, count, S, S, low, high, low_u8, high_u8, stream);
}
int llie_aug_synth_u8(const uint8_t* pool, const int64_t* table, int N, const llie_aug_row* plan, int first, int count, int S,
                      const float* z, float* low, float* high, uint8_t* low_u8, uint8_t* high_u8, llie_stream stream) {
  return llie_aug_synth_u8_hw(pool, table, N, plan, first, count, S, S, z, low, high, low_u8, high_u8, stream);
}

// ---- image quality (metrics.hip): every contract check runs here, before any HIP call
static int metrics_check(const void* a, const void* b, int batch, int H, int W, const double* out3, const void* scratch, int64_t scratch_bytes) {
  if (!a || !b || !out3 || !scratch || batch < 1) return LLIE_ERR_ARG;
  if (H < kMetricTaps || W < kMetricTaps) {
    set_err("image_metrics: images of at least %d x %d, got %d x %d", kMetricTaps, kMetricTaps, H, W);
    return LLIE_ERR_SHAPE;
  }
  const int64_t need = llie_image_metrics_scratch_bytes(batch, H, W);
  if (need < 0) return LLIE_ERR_ARG;
  if (scratch_bytes < need) {
    set_err("image_metrics: scratch of %lld bytes needed, %lld given", (long long)need, (long long)scratch_bytes);
    return LLIE_ERR_WORKSPACE;
  }
  return LLIE_OK;
}
int64_t llie_image_metrics_scratch_bytes(int batch, int H, int W) {
  if (batch < 1) return LLIE_ERR_ARG;
  if (H < kMetricTaps || W < kMetricTaps) return LLIE_ERR_SHAPE;
  const long long tiles = image_metrics_tiles(H, W) * batch;
  return tiles < (1ll << 31) ? (int64_t)(tiles * 2 * (long long)sizeof(double)) : (int64_t)LLIE_ERR_ARG;
}
int llie_image_metrics_f32(const float* a, const float* b, int batch, int H, int W, float lo, float hi, double* out3, void* scratch,
                           int64_t scratch_bytes, llie_stream stream) {
  if (!a || !b || !out3 || !scratch || batch < 1 || !(lo != hi) || !std::isfinite(lo) || !std::isfinite(hi)) return LLIE_ERR_ARG;
  if (int rc = metrics_check(a, b, batch, H, W, out3, scratch, scratch_bytes)) return rc;
  return kerr("image_metrics_f32", launch_image_metrics_f32(a, b, batch, H, W, lo, hi, out3, reinterpret_cast<double*>(scratch), hs(stream)));
}
int llie_image_metrics_u8(const uint8_t* a, const uint8_t* b, int batch, int H, int W, double* out3, void* scratch, int64_t scratch_bytes,
                          llie_stream stream) {
  if (int rc = metrics_check(a, b, batch, H, W, out3, scratch, scratch_bytes)) return rc;
  return kerr("image_metrics_u8", launch_image_metrics_u8(a, b, batch, H, W, out3, reinterpret_cast<double*>(scratch), hs(stream)));
}

// ---- SSIM / L1 with a gradient (ssimloss.hip): every contract check runs here, before any HIP call
static int ssim_grad_check(const char* what, int batch, int H, int W, const void* scratch, int64_t scratch_bytes) {
  if (!scratch || batch < 1) return LLIE_ERR_ARG;
  if (H < kMetricTaps || W < kMetricTaps) {
    set_err("%s: images of at least %d x %d, got %d x %d", what, kMetricTaps, kMetricTaps, H, W);
    return LLIE_ERR_SHAPE;
  }
  const int64_t need = llie_ssim_grad_scratch_bytes(batch, H, W);
  if (need < 0) return LLIE_ERR_ARG;
  if (scratch_bytes < need) {
    set_err("%s: scratch of %lld bytes needed, %lld given", what, (long long)need, (long long)scratch_bytes);
    return LLIE_ERR_WORKSPACE;
  }
  return LLIE_OK;
}
int64_t llie_ssim_grad_scratch_bytes(int batch, int H, int W) {
  if (batch < 1) return LLIE_ERR_ARG;
  if (H < kMetricTaps || W < kMetricTaps) return LLIE_ERR_SHAPE;
  if (3ll * batch * ((H + kMetricTileH - 1) / kMetricTileH) * ((W + kMetricTileW - 1) / kMetricTileW) >= (1ll << 31)) return LLIE_ERR_ARG;
  return (int64_t)ssim_grad_scratch_bytes(batch, H, W);
}
int llie_ssim_grad_f32(const float* a, const float* b, int batch, int H, int W, float lo, float hi, const float* upstream,
                       float* ssim_out, float* da, void* scratch, int64_t scratch_bytes, llie_stream stream) {
  if (!a || !b || !ssim_out || !(lo != hi) || !std::isfinite(lo) || !std::isfinite(hi)) return LLIE_ERR_ARG;
  if (int rc = ssim_grad_check("ssim_grad_f32", batch, H, W, scratch, scratch_bytes)) return rc;
  return kerr("ssim_grad_f32", launch_ssim_grad_f32(a, b, batch, H, W, lo, hi, upstream, ssim_out, da, scratch, hs(stream)), LLIE_ERR_ARG,
              nullptr);
}
int llie_x0_loss(const float* out, const float* x_t, const float* normal, const int64_t* t, const float* alphas_cumprod, int table_n,
                 int velocity, float lambda_s, float lambda_1, float* loss_out, float* d_out, int batch, int H, int W, void* scratch,
                 int64_t scratch_bytes, llie_stream stream) {
  if (!out || !x_t || !normal || !t || !alphas_cumprod || table_n < 1 || !loss_out) return LLIE_ERR_ARG;
  if (!(lambda_s >= 0.f) || !(lambda_1 >= 0.f) || !std::isfinite(lambda_s) || !std::isfinite(lambda_1)) {
    set_err("x0_loss: the weights must be finite and >= 0");
    return LLIE_ERR_ARG;
  }
  if (int rc = ssim_grad_check("x0_loss", batch, H, W, scratch, scratch_bytes)) return rc;
  X0LossArgs x{};
  x.out = out; x.x_t = x_t; x.normal = normal; x.t = t; x.acp = alphas_cumprod; x.table_len = table_n; x.velocity = velocity != 0;
  x.lambda_s = lambda_s; x.lambda_1 = lambda_1; x.loss = loss_out; x.d_out = d_out; x.batch = batch; x.H = H; x.W = W;
  return kerr("x0_loss", launch_x0_loss(x, scratch, hs(stream)), LLIE_ERR_ARG, nullptr);
}

// ---- the noise-space loss with a Min-SNR-gamma weight (snrloss.hip): every contract check runs here, before any HIP call
static_assert(LLIE_LOSS_MSE == kLossMse && LLIE_LOSS_L1 == kLossL1 && LLIE_LOSS_HUBER == kLossHuber, "LLIE_LOSS_* are the kernels' codes");
int64_t llie_snr_loss_chunk(void) { return kSnrChunk; }
int64_t llie_snr_loss_scratch_bytes(int batch, int64_t per_sample) {
  const long long n = snr_loss_scratch_bytes(batch, per_sample);
  return n < 0 ? (int64_t)LLIE_ERR_ARG : (int64_t)n;
}
int llie_snr_loss(const float* pred, const float* target, const int64_t* t, const float* alphas_cumprod, int table_n, int loss_type,
                  int velocity, float gamma, float* loss_out, float* sample_loss, float* weight, float* d_pred, int batch,
                  int64_t per_sample, void* scratch, int64_t scratch_bytes, llie_stream stream) {
  if (!pred || !target || !t || !alphas_cumprod || !loss_out || !scratch || batch < 1 || per_sample < 1 || table_n < 1) return LLIE_ERR_ARG;
  for (const void* p : {(const void*)pred, (const void*)target, (const void*)alphas_cumprod, (const void*)loss_out, (const void*)sample_loss,
                        (const void*)weight, (const void*)d_pred})
    if (reinterpret_cast<uintptr_t>(p) & 3) {
      set_err("snr_loss: fp32 pointers must be 4-byte aligned");
      return LLIE_ERR_ARG;
    }
  if ((reinterpret_cast<uintptr_t>(t) | reinterpret_cast<uintptr_t>(scratch)) & 7) {
    set_err("snr_loss: t and scratch must be 8-byte aligned");
    return LLIE_ERR_ARG;
  }
  if (loss_type != LLIE_LOSS_MSE && loss_type != LLIE_LOSS_L1 && loss_type != LLIE_LOSS_HUBER) {
    set_err("snr_loss: unknown loss_type %d", loss_type);
    return LLIE_ERR_ARG;
  }
  if (!std::isfinite(gamma) || !(gamma > 0.f)) {
    set_err("snr_loss: snr_gamma must be finite and > 0");
    return LLIE_ERR_ARG;
  }
  const int64_t need = llie_snr_loss_scratch_bytes(batch, per_sample);
  if (need < 0) return LLIE_ERR_ARG;
  if (scratch_bytes < need) {
    set_err("snr_loss: scratch of %lld bytes needed, %lld given", (long long)need, (long long)scratch_bytes);
    return LLIE_ERR_WORKSPACE;
  }
  SnrLossArgs x{};
  x.pred = pred; x.target = target; x.t = t; x.acp = alphas_cumprod; x.table_len = table_n; x.loss_type = loss_type;
  x.velocity = velocity != 0; x.gamma = gamma; x.loss = loss_out; x.sample_loss = sample_loss; x.weight = weight; x.d_pred = d_pred;
  x.batch = batch; x.per = per_sample;
  return kerr("snr_loss", launch_snr_loss(x, scratch, hs(stream)), LLIE_ERR_ARG, nullptr);
}

// ---- the trainer's sample sheet (samples.hip): arguments are checked here, before any HIP call
int llie_comparison_grid_u8(const float* low, const float* enhanced, const float* normal, int n, int H, int W, uint8_t* grid,
                            llie_stream stream) {
  if (!low || !enhanced || !normal || !grid || !comparison_grid_ok(n, H, W)) return LLIE_ERR_ARG;
  return kerr("comparison_grid_u8", launch_comparison_grid_u8(low, enhanced, normal, n, H, W, grid, hs(stream)), LLIE_ERR_ARG, nullptr);
}

int llie_time_embed(llie_ctx* c, const int64_t* t, int rows, float* emb, float* temb, float* silu_temb, llie_stream stream) {
  if (!c || !t || !temb || !silu_temb || rows <= 0 || c->cfg.kind != LLIE_UNET) return LLIE_ERR_ARG;
  if (int rc = check_loaded(c)) return rc;
  const llie_config& g = c->cfg;
  TimeArgs ta{};
  ta.t = t; ta.rows = rows; ta.dim = g.base_channels; ta.T = g.time_embed_dim;
  ta.freqs = reinterpret_cast<const float*>(c->blob + c->freqs);
  ta.w1 = reinterpret_cast<const float*>(c->blob + c->t_w1); ta.b1 = reinterpret_cast<const float*>(c->blob + c->t_b1);
  ta.w3 = reinterpret_cast<const float*>(c->blob + c->t_w3); ta.b3 = reinterpret_cast<const float*>(c->blob + c->t_b3);
  ta.temb = temb; ta.silu_temb = silu_temb; ta.emb_out = emb;
  return kerr("time_embed", launch_time_embed(ta, hs(stream)), 0);
}

// ---- optimiser step (training): one object per parameter set, tables resident on the device
struct llie_optimizer {
  int device = 0;
  OptTensor* tensors = nullptr;
  OptChunk* chunks = nullptr;
  double* partial = nullptr;
  float* amp_coef = nullptr;  // [5]: the AMP step's stats and bias corrections, from its clip kernel to its update kernel
  int count = 0, nchunks = 0;
  int64_t numel = 0;
};

}  // extern "C"

// what both optimiser steps take
static OptStepArgs opt_args(const llie_optimizer* o, const float* grad_base, const llie_opt_hyper* h, float* stats3) {
  OptStepArgs a{};
  a.tensors = o->tensors; a.chunks = o->chunks; a.nchunks = o->nchunks;
  a.gbase = grad_base; a.partial = o->partial; a.stats = stats3;
  a.lr = h->lr; a.beta1 = h->beta1; a.beta2 = h->beta2; a.eps = h->eps; a.weight_decay = h->weight_decay;
  a.max_grad_norm = h->max_grad_norm; a.ema_decay = h->ema_decay; a.grad_scale = h->grad_scale;
  return a;
}

extern "C" {

int llie_optimizer_create(const llie_opt_tensor* tensors, int count, llie_optimizer** out) {
  if (!tensors || count <= 0 || !out) return LLIE_ERR_ARG;
  std::vector<OptTensor> tt((size_t)count);
  std::vector<OptChunk> cc;
  int64_t total = 0;
  for (int i = 0; i < count; ++i) {
    const llie_opt_tensor& t = tensors[i];
    if (!t.param || !t.exp_avg || !t.exp_avg_sq || t.numel <= 0 || t.grad_offset < 0 || t.numel > (int64_t)INT32_MAX) {
      set_err("optimizer_create: tensor %d: null pointer, empty tensor or negative gradient offset", i);
      return LLIE_ERR_ARG;
    }
    tt[(size_t)i] = OptTensor{t.param, t.exp_avg, t.exp_avg_sq, t.ema, (long long)t.grad_offset, (long long)t.numel};
    for (int64_t o = 0; o < t.numel; o += kOptChunk) cc.push_back(OptChunk{i, (int)o});
    total += t.numel;
  }
  if (cc.size() > (size_t)INT32_MAX) return LLIE_ERR_ARG;
  auto* o = new llie_optimizer();
  o->count = count;
  o->nchunks = (int)cc.size();
  o->numel = total;
  hipError_t e = hipGetDevice(&o->device);
  if (e == hipSuccess) e = hipMalloc(reinterpret_cast<void**>(&o->tensors), tt.size() * sizeof(OptTensor));
  if (e == hipSuccess) e = hipMalloc(reinterpret_cast<void**>(&o->chunks), cc.size() * sizeof(OptChunk));
  if (e == hipSuccess) e = hipMalloc(reinterpret_cast<void**>(&o->partial), cc.size() * sizeof(double));
  if (e == hipSuccess) e = hipMalloc(reinterpret_cast<void**>(&o->amp_coef), 5 * sizeof(float));
  if (e == hipSuccess) e = hipMemcpy(o->tensors, tt.data(), tt.size() * sizeof(OptTensor), hipMemcpyHostToDevice);
  if (e == hipSuccess) e = hipMemcpy(o->chunks, cc.data(), cc.size() * sizeof(OptChunk), hipMemcpyHostToDevice);
  if (e != hipSuccess) {
    set_err("optimizer_create: %s", hipGetErrorString(e));
    llie_optimizer_destroy(o);
    return e == hipErrorNoDevice ? LLIE_ERR_NO_DEVICE : (int)e;
  }
  *out = o;
  return LLIE_OK;
}

void llie_optimizer_destroy(llie_optimizer* o) {
  if (!o) return;
  if (o->tensors) (void)hipFree(o->tensors);
  if (o->chunks) (void)hipFree(o->chunks);
  if (o->partial) (void)hipFree(o->partial);
  if (o->amp_coef) (void)hipFree(o->amp_coef);
  delete o;
}

int64_t llie_optimizer_numel(const llie_optimizer* o) { return o ? o->numel : (int64_t)LLIE_ERR_ARG; }

int llie_optimizer_step(llie_optimizer* o, const float* grad_base, const llie_opt_hyper* h, float* stats3, llie_stream stream) {
  if (!o || !grad_base || !h || !stats3) return LLIE_ERR_ARG;
  OptStepArgs a = opt_args(o, grad_base, h, stats3);
  a.step = h->step; a.skip_nonfinite = h->skip_nonfinite;
  return kerr("optimizer_step", launch_optimizer_step(a, hs(stream)), LLIE_ERR_ARG, "hyper-parameters outside their ranges (lr, eps, weight_decay >= 0; 0 <= beta < 1; ema_decay <= 1; step >= 1)");
}

int llie_optimizer_step_amp(llie_optimizer* o, const float* grad_base, const llie_opt_hyper* h, const llie_amp_state* state,
                            const llie_amp_config* cfg, float* stats3, llie_stream stream) {
  if (!o || !grad_base || !h || !state || !cfg || !stats3 || !state->scale || !state->growth_tracker || !state->step) return LLIE_ERR_ARG;
  const OptStepArgs a = opt_args(o, grad_base, h, stats3);
  OptAmpArgs amp{};
  amp.scale = state->scale; amp.growth_tracker = state->growth_tracker; amp.step = state->step;
  amp.growth_factor = cfg->growth_factor; amp.backoff_factor = cfg->backoff_factor; amp.growth_interval = cfg->growth_interval;
  return kerr("optimizer_step_amp", launch_optimizer_step_amp(a, amp, o->amp_coef, hs(stream)), LLIE_ERR_ARG, "hyper-parameters outside their ranges (lr, eps, weight_decay >= 0; 0 <= beta < 1; ema_decay <= 1)");
}

int llie_grad_accumulate(float* acc, const float* grad, int64_t n, float weight, int first, llie_stream stream) {
  if (!acc || !grad || n < 0) { set_err("grad_accumulate: null pointer or n < 0"); return LLIE_ERR_ARG; }
  if (!std::isfinite(weight) || !(weight > 0.f)) { set_err("grad_accumulate: the weight must be finite and > 0"); return LLIE_ERR_ARG; }
  const uintptr_t a = reinterpret_cast<uintptr_t>(acc), g = reinterpret_cast<uintptr_t>(grad);
  if ((a | g) & 3) { set_err("grad_accumulate: pointers must be 4-byte aligned"); return LLIE_ERR_ARG; }
  // keeps the byte count and the grid inside their types; no real buffer comes near it
  if (n > (int64_t)1 << 40) { set_err("grad_accumulate: n above 2^40"); return LLIE_ERR_ARG; }
  const uintptr_t bytes = (uintptr_t)n * 4;
  if (a < g + bytes && g < a + bytes) { set_err("grad_accumulate: acc and grad overlap"); return LLIE_ERR_ARG; }
  if (n == 0) return LLIE_OK;
  return kerr("grad_accumulate", launch_grad_accumulate(acc, grad, (long long)n, weight, first != 0, hs(stream)), LLIE_ERR_ARG, "null pointer or n out of range");
}

// ---- consistency distillation
static int distill_pred_ok(const char* who, int pred) {
  if (pred == LLIE_PRED_EPSILON || pred == LLIE_PRED_V) return LLIE_OK;
  set_err("%s: prediction type %d (LLIE_PRED_EPSILON = 0 or LLIE_PRED_V = 1)", who, pred);
  return LLIE_ERR_ARG;
}

int llie_consistency_target_ex(const float* x_t, const float* out_teacher, const int64_t* t, const int64_t* t_next, const float* acp,
                               int table_len, float* x_next, int batch, int64_t per, int teacher_pred, llie_stream stream) {
  if (int e = distill_pred_ok("consistency_target", teacher_pred); e != LLIE_OK) return e;
  DistillArgs a{};
  a.x_t = x_t; a.e_a = out_teacher; a.t = t; a.t_next = t_next; a.acp = acp; a.table_len = table_len; a.batch = batch; a.per = per; a.out = x_next;
  a.pred = teacher_pred;
  return kerr("consistency_target", launch_consistency_target(a, hs(stream)), LLIE_ERR_ARG, "null pointer or empty shape");
}

int llie_consistency_loss_ex(const float* x_t, const float* x_next, const float* out_student, const float* out_ema, const int64_t* t,
                             const int64_t* t_next, const float* acp, int table_len, float* d_student, float* loss_out, void* scratch,
                             int64_t scratch_bytes, int batch, int64_t per, int student_pred, llie_stream stream) {
  if (int e = distill_pred_ok("consistency_loss", student_pred); e != LLIE_OK) return e;
  if (batch <= 0 || per <= 0) return LLIE_ERR_ARG;
  const int64_t need = distill_loss_partials((int64_t)batch * per) * (int64_t)sizeof(double);
  if (!scratch || scratch_bytes < need) {
    set_err("consistency_loss: scratch of %lld bytes needed, %lld given", (long long)need, (long long)scratch_bytes);
    return LLIE_ERR_WORKSPACE;
  }
  DistillArgs a{};
  a.x_t = x_t; a.x_next = x_next; a.e_a = out_student; a.e_b = out_ema; a.t = t; a.t_next = t_next; a.acp = acp; a.table_len = table_len;
  a.batch = batch; a.per = per; a.out = d_student; a.pred = student_pred;
  return kerr("consistency_loss", launch_consistency_loss(a, reinterpret_cast<double*>(scratch), loss_out, hs(stream)), LLIE_ERR_ARG, "null pointer or empty shape");
}

// the epsilon-only entries: the epsilon instantiation of the same kernels
int llie_consistency_target(const float* x_t, const float* e_teacher, const int64_t* t, const int64_t* t_next, const float* acp, int table_len,
                            float* x_next, int batch, int64_t per, llie_stream stream) {
  return llie_consistency_target_ex(x_t, e_teacher, t, t_next, acp, table_len, x_next, batch, per, LLIE_PRED_EPSILON, stream);
}

int llie_consistency_loss(const float* x_t, const float* x_next, const float* e_student, const float* e_ema, const int64_t* t,
                          const int64_t* t_next, const float* acp, int table_len, float* d_student, float* loss_out, int batch, int64_t per,
                          void* scratch, int64_t scratch_bytes, llie_stream stream) {
  return llie_consistency_loss_ex(x_t, x_next, e_student, e_ema, t, t_next, acp, table_len, d_student, loss_out, scratch, scratch_bytes, batch, per,
                                  LLIE_PRED_EPSILON, stream);
}

// ---- classifier-free guidance
int llie_guide(const float* out_cond, const float* out_uncond, const float* w_rows, float w, float* out, int batch, int64_t per_sample,
               llie_stream stream) {
  return kerr("guide", launch_guide(out_cond, out_uncond, w_rows, w, out, batch, per_sample, hs(stream)), LLIE_ERR_ARG,
              "null or unaligned pointer, empty shape, or a non-finite guidance scale");
}

// guidance rescale: every contract check runs here, before any HIP call
int64_t llie_guide_rescale_chunk(void) { return kGuideRescaleChunk; }
int64_t llie_guide_rescale_scratch_bytes(int batch, int64_t per_sample) {
  const long long n = guide_rescale_scratch_bytes(batch, per_sample);
  return n < 0 ? (int64_t)LLIE_ERR_ARG : (int64_t)n;
}
int llie_guide_rescale(const float* out_cond, const float* out_uncond, const float* w_rows, float w, float phi, float* out, float* factor,
                       void* scratch, int64_t scratch_bytes, int batch, int64_t per_sample, llie_stream stream) {
  if (!out_cond || !out_uncond || !out || !scratch || batch < 1 || per_sample < 1) {
    set_err("guide_rescale: null pointer or empty shape");
    return LLIE_ERR_ARG;
  }
  for (const void* p : {(const void*)out_cond, (const void*)out_uncond, (const void*)w_rows, (const void*)out, (const void*)factor})
    if (reinterpret_cast<uintptr_t>(p) & 3) {
      set_err("guide_rescale: fp32 pointers must be 4-byte aligned");
      return LLIE_ERR_ARG;
    }
  if (reinterpret_cast<uintptr_t>(scratch) & 7) {
    set_err("guide_rescale: scratch must be 8-byte aligned");
    return LLIE_ERR_ARG;
  }
  if (!w_rows && !std::isfinite(w)) {
    set_err("guide_rescale: the guidance scale must be finite");
    return LLIE_ERR_ARG;
  }
  if (!std::isfinite(phi) || phi < 0.f || phi > 1.f) {
    set_err("guide_rescale: phi must be in [0, 1]");
    return LLIE_ERR_ARG;
  }
  const int64_t need = llie_guide_rescale_scratch_bytes(batch, per_sample);
  if (need < 0) {
    set_err("guide_rescale: more than 2^31 - 1 workgroups");
    return LLIE_ERR_ARG;
  }
  if (scratch_bytes < need) {
    set_err("guide_rescale: scratch of %lld bytes needed, %lld given", (long long)need, (long long)scratch_bytes);
    return LLIE_ERR_WORKSPACE;
  }
  return kerr("guide_rescale", launch_guide_rescale(out_cond, out_uncond, w_rows, w, phi, out, factor, scratch, batch, per_sample, hs(stream)),
              LLIE_ERR_ARG, nullptr);
}

int llie_guidance_pair(const float* latents, const float* cond, float* latents2, float* cond2, int batch, int64_t per_sample,
                       llie_stream stream) {
  return kerr("guidance_pair", launch_guidance_pair(latents, cond, latents2, cond2, batch, per_sample, hs(stream)), LLIE_ERR_ARG,
              "null or unaligned pointer, or empty shape");
}

int llie_cond_dropout(const float* in, const float* u, float p, float* out, int batch, int64_t per_sample, llie_stream stream) {
  return kerr("cond_dropout", launch_cond_dropout(in, u, p, out, batch, per_sample, hs(stream)), LLIE_ERR_ARG,
              "null or unaligned pointer, empty shape, or p outside [0, 1]");
}

// the optimiser's table types: OptTensor.p = source parameter, OptTensor.ema = shadow written in place (m, v unused)
struct llie_ema {
  OptTensor* tensors = nullptr;
  OptChunk* chunks = nullptr;
  int nchunks = 0;
};

int llie_ema_create(float* const* ema, const float* const* params, const int64_t* numel, int count, llie_ema** out) {
  if (!ema || !params || !numel || count <= 0 || !out) return LLIE_ERR_ARG;
  std::vector<OptTensor> tt((size_t)count);
  std::vector<OptChunk> cc;
  for (int i = 0; i < count; ++i) {
    if (!ema[i] || !params[i] || numel[i] <= 0 || numel[i] > (int64_t)INT32_MAX) {
      set_err("ema_create: tensor %d: null pointer or empty tensor", i);
      return LLIE_ERR_ARG;
    }
    tt[(size_t)i] = OptTensor{const_cast<float*>(params[i]), nullptr, nullptr, ema[i], 0, (long long)numel[i]};
    for (int64_t o = 0; o < numel[i]; o += kOptChunk) cc.push_back(OptChunk{i, (int)o});
  }
  if (cc.size() > (size_t)INT32_MAX) return LLIE_ERR_ARG;
  auto* o = new llie_ema();
  o->nchunks = (int)cc.size();
  hipError_t e = hipMalloc(reinterpret_cast<void**>(&o->tensors), tt.size() * sizeof(OptTensor));
  if (e == hipSuccess) e = hipMalloc(reinterpret_cast<void**>(&o->chunks), cc.size() * sizeof(OptChunk));
  if (e == hipSuccess) e = hipMemcpy(o->tensors, tt.data(), tt.size() * sizeof(OptTensor), hipMemcpyHostToDevice);
  if (e == hipSuccess) e = hipMemcpy(o->chunks, cc.data(), cc.size() * sizeof(OptChunk), hipMemcpyHostToDevice);
  if (e != hipSuccess) {
    set_err("ema_create: %s", hipGetErrorString(e));
    llie_ema_destroy(o);
    return e == hipErrorNoDevice ? LLIE_ERR_NO_DEVICE : (int)e;
  }
  *out = o;
  return LLIE_OK;
}

int llie_ema_update(llie_ema* o, double decay, llie_stream stream) {
  if (!o) return LLIE_ERR_ARG;
  return kerr("ema_update", launch_ema_lerp(o->tensors, o->chunks, o->nchunks, decay, hs(stream)), LLIE_ERR_ARG, "decay must be in [0, 1]");
}

void llie_ema_destroy(llie_ema* o) {
  if (!o) return;
  if (o->tensors) (void)hipFree(o->tensors);
  if (o->chunks) (void)hipFree(o->chunks);
  delete o;
}

int llie_copy_probe(const void* src, void* dst, int64_t bytes, llie_stream stream) {
  if (!src || !dst || bytes <= 0) return LLIE_ERR_ARG;
  return kerr("copy_probe", launch_copy_probe(src, dst, bytes, hs(stream)), LLIE_ERR_ARG, nullptr);
}

int llie_rw_probe(const void* src, void* dst, int64_t units, int reads, int writes, int nontemporal, llie_stream stream) {
  if (!src || !dst || units <= 0) return LLIE_ERR_ARG;
  return kerr("rw_probe", launch_rw_probe(src, dst, units, reads, writes, nontemporal, hs(stream)), LLIE_ERR_ARG, nullptr);
}

// ---- recompute form of the inverted-residual block (irbx.hip), kernel by kernel
static IrbxArgs irbx_args(const void* x0, int c0, const void* x1, int c1, const float* scale1, const float* shift1, const void* w_expand,
                          const float* scale2, const float* shift2, const float* w_dw, int batch, int H, int W) {
  IrbxArgs a{};
  a.x0 = x0; a.c0 = c0; a.x1 = x1; a.c1 = c1; a.as1 = scale1; a.ab1 = shift1; a.w1 = w_expand; a.as2 = scale2; a.ab2 = shift2; a.wd = w_dw;
  a.B = batch; a.H = H; a.W = W; a.Chid = 4 * (c0 + c1);
  return a;
}
static const char* kIrbxShapes = "2-byte dtype, c0 + c1 in {32, 64, 96}, c0 % 16 == 0, H % 8 == 0, W % 16 == 0";
int llie_expand_dw(int dtype, const void* x0, int c0, const void* x1, int c1, const float* scale1, const float* shift1, const void* w_expand,
                   const float* scale2, const float* shift2, const float* w_dw, void* h2, unsigned long long* pool_totals, int batch, int H, int W,
                   llie_stream stream) {
  if (!x0 || !scale1 || !shift1 || !w_expand || !scale2 || !shift2 || !w_dw || !h2 || batch <= 0 || c0 <= 0 || c1 < 0 || (c1 > 0) != (x1 != nullptr))
    return LLIE_ERR_ARG;
  IrbxArgs a = irbx_args(x0, c0, x1, c1, scale1, shift1, w_expand, scale2, shift2, w_dw, batch, H, W);
  a.out = h2; a.pool_tot = pool_totals;
  return kerr("expand_dw", launch_expand_dw(dtype, a, hs(stream)), LLIE_ERR_SHAPE, kIrbxShapes);
}
int llie_expand_pool(int dtype, const void* x0, int c0, const void* x1, int c1, const float* scale1, const float* shift1, const void* w_expand,
                     const float* scale2, const float* shift2, const float* w_dw, unsigned long long* pool_totals, int batch, int H, int W,
                     llie_stream stream) {
  if (!x0 || !scale1 || !shift1 || !w_expand || !scale2 || !shift2 || !w_dw || !pool_totals || batch <= 0 || c0 <= 0 || c1 < 0 ||
      (c1 > 0) != (x1 != nullptr))
    return LLIE_ERR_ARG;
  IrbxArgs a = irbx_args(x0, c0, x1, c1, scale1, shift1, w_expand, scale2, shift2, w_dw, batch, H, W);
  a.pool_tot = pool_totals;
  return kerr("expand_pool", launch_expand_pool(dtype, a, hs(stream)), LLIE_ERR_SHAPE, kIrbxShapes);
}
int llie_expand_stats(int dtype, const void* x0, int c0, const void* x1, int c1, const float* scale1, const float* shift1, const void* w_expand,
                      float* stats, int batch, int H, int W, llie_stream stream) {
  if (!x0 || !scale1 || !shift1 || !w_expand || !stats || batch <= 0 || c0 <= 0 || c1 < 0 || (c1 > 0) != (x1 != nullptr)) return LLIE_ERR_ARG;
  IrbxArgs a = irbx_args(x0, c0, x1, c1, scale1, shift1, w_expand, nullptr, nullptr, nullptr, batch, H, W);
  a.stats = stats;
  return kerr("expand_stats", launch_expand_stats(dtype, a, hs(stream)), LLIE_ERR_SHAPE, kIrbxShapes);
}
int llie_irbx_stats_rows(int P) { return P > 0 ? irbx_stats_rows(P) : LLIE_ERR_ARG; }
int llie_expand_dw_project(int dtype, const void* x, int C, const float* scale1, const float* shift1, const void* w_expand, const float* scale2,
                           const float* shift2, const float* w_dw, const float* gate, const void* w_project, void* y, float* stats, int batch,
                           int H, int W, llie_stream stream) {
  if (!x || !scale1 || !shift1 || !w_expand || !scale2 || !shift2 || !w_dw || !gate || !w_project || !y || !stats || batch <= 0 || C <= 0)
    return LLIE_ERR_ARG;
  IrbxArgs a = irbx_args(x, C, nullptr, 0, scale1, shift1, w_expand, scale2, shift2, w_dw, batch, H, W);
  a.gate = gate; a.wp = w_project; a.y = y; a.ystats = stats;
  return kerr("expand_dw_project", launch_expand_dw_project(dtype, a, C, false, hs(stream)), LLIE_ERR_SHAPE,
              "2-byte dtype, C in {32, 64}, H % 8 == 0, W % 16 == 0");
}
int llie_expand_dw_project_skip(int dtype, const void* x0, int c0, const void* x1, int c1, const float* scale1, const float* shift1,
                                const void* w_expand, const float* scale2, const float* shift2, const float* w_dw, const float* gate,
                                const void* w_project_skip, int ld, int cout, void* y, float* stats, int batch, int H, int W, llie_stream stream) {
  if (!x0 || !scale1 || !shift1 || !w_expand || !scale2 || !shift2 || !w_dw || !gate || !w_project_skip || !y || !stats || batch <= 0 || c0 <= 0 ||
      c1 < 0 || (c1 > 0) != (x1 != nullptr) || cout <= 0 || ld < 5 * (c0 + c1))
    return LLIE_ERR_ARG;
  IrbxArgs a = irbx_args(x0, c0, x1, c1, scale1, shift1, w_expand, scale2, shift2, w_dw, batch, H, W);
  a.gate = gate; a.wp = w_project_skip; a.ldp = ld; a.y = y; a.ystats = stats;
  return kerr("expand_dw_project_skip", launch_expand_dw_project(dtype, a, cout, true, hs(stream)), LLIE_ERR_SHAPE,
              "2-byte dtype, c0 + c1 == 96, c0 % 16 == 0, cout == 32, ld % 8 == 0, H % 8 == 0, W % 16 == 0");
}
int llie_expand_dw_plan(int cin, int batch, int H, int W, int project, int* plan4) {
  if (!plan4 || cin <= 0 || batch <= 0 || H <= 0 || W <= 0 || project < 0 || project > 1) return LLIE_ERR_ARG;
  if (!irbx_supported(1, cin, cin, 4 * cin, H, W)) return LLIE_ERR_SHAPE;
  const IrbxPlan p = irbx_plan(cin, batch, H, W, project != 0);
  plan4[0] = p.tpw; plan4[1] = p.cpw; plan4[2] = p.gx; plan4[3] = p.gy;
  return LLIE_OK;
}
// ---- wide decoder blocks without h2, from the stored h1 (irbx.hip, section 3)
int llie_wide_project_supported(int dtype, int cin, int c0, int chid, int cout, int skip, int padded, int H, int W) {
  return wide_project_supported(dtype, cin, c0, chid, cout, skip != 0, padded != 0, H, W) ? 1 : 0;
}
static const char* kWideShapes = "2-byte dtype, skip conv, (c0 + c1, Chid, cout) in {(192, 768, 64), (384, 1536, 128)}, c0 % 16 == 0, H % 8 == 0, W % 16 == 0";
int llie_dwconv3x3_pool(int dtype, const void* h1, const float* scale2, const float* shift2, const float* w_dw, unsigned long long* pool_totals,
                        int batch, int H, int W, int chid, llie_stream stream) {
  if (!h1 || !scale2 || !shift2 || !w_dw || !pool_totals || batch <= 0) return LLIE_ERR_ARG;
  IrbxArgs a{};
  a.h1 = h1; a.as2 = scale2; a.ab2 = shift2; a.wd = w_dw; a.pool_tot = pool_totals; a.B = batch; a.H = H; a.W = W; a.Chid = chid;
  return kerr("dwconv3x3_pool", launch_dwconv3x3_pool(dtype, a, hs(stream)), LLIE_ERR_SHAPE, "2-byte dtype, Chid in {768, 1536}, H % 8 == 0, W % 16 == 0");
}
int llie_dwconv3x3_project(int dtype, const void* h1, const float* scale2, const float* shift2, const float* w_dw, const float* gate, const void* x0,
                           int c0, const void* x1, int c1, const void* w_project_skip, int ld, int cout, void* y, float* stats, int batch, int H,
                           int W, llie_stream stream) {
  if (!h1 || !scale2 || !shift2 || !w_dw || !gate || !x0 || !w_project_skip || !y || !stats || batch <= 0 || c0 <= 0 || c1 < 0 ||
      (c1 > 0) != (x1 != nullptr) || cout <= 0 || ld < 5 * (c0 + c1))
    return LLIE_ERR_ARG;
  IrbxArgs a{};
  a.h1 = h1; a.as2 = scale2; a.ab2 = shift2; a.wd = w_dw; a.gate = gate; a.x0 = x0; a.c0 = c0; a.x1 = x1; a.c1 = c1; a.wp = w_project_skip;
  a.ldp = ld; a.y = y; a.ystats = stats; a.B = batch; a.H = H; a.W = W; a.Chid = 4 * (c0 + c1);
  return kerr("dwconv3x3_project", launch_dwconv3x3_project(dtype, a, cout, hs(stream)), LLIE_ERR_SHAPE, kWideShapes);
}
// ---- the wide Gram form of the 192 -> 64 block (gram.hip, pwx.hip, irbx.hip)
int llie_wide_gram_supported(int dtype, int cin, int c0, int chid, int pixels) { return gram_wide_supported(dtype, cin, c0, chid, pixels) ? 1 : 0; }
int64_t llie_gram_wide_floats(void) { return kGramWideFloats; }
int64_t llie_gram_wide_part_floats(int pixels) { return pixels > 0 && pixels % 128 == 0 ? (int64_t)gram_wide_part_floats(pixels) : LLIE_ERR_ARG; }
int llie_gram_wide_block(int q, int* bi, int* bj) {
  if (q < 0 || q >= kGramWideBlocks || !bi || !bj) return LLIE_ERR_ARG;
  gram_wide_block(q, bi, bj);
  return LLIE_OK;
}
int llie_gram_wide(int dtype, const void* x0, int c0, const void* x1, int c1, const float* scale, const float* bias, int batch, int pixels,
                   float* part, float* gblk, llie_stream stream) {
  GramWideArgs a{};
  a.x0 = x0; a.x1 = x1; a.c0 = c0; a.c1 = c1; a.as1 = scale; a.ab1 = bias; a.part = part; a.gblk = gblk; a.B = batch; a.P = pixels;
  if (!gram_wide_supported(dtype, c0 + c1, c0, 4 * (c0 + c1), pixels)) { set_err("gram_wide: K = 192, 2-byte dtype, pixels a multiple of 128"); return LLIE_ERR_SHAPE; }
  return kerr("gram_wide", launch_gram_wide(dtype, a, hs(stream)), LLIE_ERR_ARG, hipGetErrorString(hipErrorInvalidValue));
}
int llie_gram_group_weights(int dtype, const void* wpack, double* mg, int chid, int K, llie_stream stream) {
  if (!wpack || !mg) return LLIE_ERR_ARG;
  return kerr("gram_group_weights", launch_gram_group_weights(dtype, wpack, mg, chid, K, hs(stream)), LLIE_ERR_SHAPE, "2-byte dtype, K = 192, Chid = 768");
}
int llie_gram_group_finalize(const float* gblk, const double* mg, int K, int pixels, const float* gamma, const float* beta, const float* film,
                             int64_t film_stride, float eps, float post_scale, int batch, float* scale_out, float* shift_out, llie_stream stream) {
  if (!gblk || !mg || !gamma || !beta || !scale_out || !shift_out || batch <= 0 || pixels <= 0 || K != kGramWideK) return LLIE_ERR_ARG;
  GramGroupFinalizeArgs a{};
  a.gblk = gblk; a.mg = mg; a.K = K; a.Chid = 4 * K; a.groups = 32; a.P = pixels; a.B = batch; a.gamma = gamma; a.beta = beta;
  a.film = film; a.film_stride = film_stride; a.eps = eps; a.as = scale_out; a.ab = shift_out; a.post_scale = post_scale;
  return kerr("gram_group_finalize", launch_gram_group_finalize(a, hs(stream)));
}
int llie_pw_expand_act(int dtype, const llie_gemm_seg* segs, int nseg, const float* w32, void* wpack, const float* scale2, const float* shift2,
                       const float* w_dw, void* out, unsigned long long* pool_totals, int M, int N, int H, int W, llie_stream stream) {
  if (!segs || nseg < 1 || nseg > 3 || !wpack || !out || !scale2 || !shift2 || !w_dw || !pool_totals || dtype < 1 || dtype > 2 || H <= 0 || W <= 0)
    return LLIE_ERR_ARG;
  ExpandArgs x{};
  x.nseg = nseg;
  x.K = to_segs(segs, nseg, x.seg);
  x.wf = wpack; x.out = out; x.M = M; x.N = N; x.P = H * W; x.H = H; x.W = W;
  x.as2 = scale2; x.ab2 = shift2; x.wd = w_dw; x.pool_tot = pool_totals;
  hipStream_t s = hs(stream);
  hipError_t e = !pw_expand_act_supported(dtype, x.seg, nseg, M, N, x.K, x.P, H, W) ? hipErrorInvalidValue
                 : (w32 ? launch_pack_expand(dtype, w32, wpack, N, x.K, 6.f, s) : hipSuccess);
  if (e == hipSuccess) e = launch_pw_expand_act(dtype, x, s);
  return kerr("pw_expand_act", e);
}
int llie_dwconv3x3_project_preact(int dtype, const void* h1a, const float* w_dw, const float* gate, const void* x0, int c0, const void* x1, int c1,
                                  const void* w_project_skip, int ld, int cout, void* y, float* stats, int batch, int H, int W, llie_stream stream) {
  if (!h1a || !w_dw || !gate || !x0 || !w_project_skip || !y || !stats || batch <= 0 || c0 <= 0 || c1 < 0 || (c1 > 0) != (x1 != nullptr) || cout <= 0 ||
      ld < 5 * (c0 + c1))
    return LLIE_ERR_ARG;
  IrbxArgs a{};
  a.h1 = h1a; a.h1_act = 1; a.wd = w_dw; a.gate = gate; a.x0 = x0; a.c0 = c0; a.x1 = x1; a.c1 = c1; a.wp = w_project_skip;
  a.ldp = ld; a.y = y; a.ystats = stats; a.B = batch; a.H = H; a.W = W; a.Chid = 4 * (c0 + c1);
  return kerr("dwconv3x3_project_preact", launch_dwconv3x3_project(dtype, a, cout, hs(stream)), LLIE_ERR_SHAPE, kWideShapes);
}
int llie_irbx_project_tiles(int H, int W) { return H > 0 && W > 0 && H % 8 == 0 && W % 16 == 0 ? irbx_project_tiles(H, W) : LLIE_ERR_ARG; }

int llie_dwconv3x3_tiles(int H, int W) { return dwconv_ntiles(H, W); }
int llie_pw_gemm_tile_rows(int P) { return pw_gemm_tile_rows(P); }
}  // extern "C"
