// Parameter table and topology of the denoiser, context life cycle, state_dict (re)loading, byte / flop model.
#include "engine.h"

using namespace llie;

namespace {
thread_local char g_err[512] = "";
}
void llie::set_err(const char* fmt, ...) {
  va_list ap;
  va_start(ap, fmt);
  vsnprintf(g_err, sizeof(g_err), fmt, ap);
  va_end(ap);
}

namespace {

// ---------------------------------------------------------------------------------------------
// Topology builder (efficient_unet.py:403-530).  Adds parameters in the reference's registration
// order and lays the weight blob out.
struct Builder {
  llie_ctx* c;
  size_t cursor = 0;
  size_t reserve(size_t bytes) {
    const size_t o = cursor;
    cursor += align_up(bytes, 256);
    return o;
  }
  // idx (here and below): where to record the new parameter's index
  Param& add(const std::string& key, int64_t numel, PKind kind, size_t off, int* idx = nullptr) {
    Param p;
    p.key = key;
    p.numel = numel;
    p.kind = kind;
    p.off = off;
    p.ndim = 1;
    p.shape[0] = numel;
    c->index[key] = (int)c->params.size();
    if (idx) *idx = (int)c->params.size();
    c->params.push_back(p);
    return c->params.back();
  }
  size_t f32(const std::string& key, int64_t n, int64_t n_phys = 0, int* idx = nullptr) {  // n_phys: zero-padded length of the destination
    const size_t o = reserve((size_t)std::max(n, n_phys) * 4);
    add(key, n, PK_F32, o, idx);
    return o;
  }
  int padh(int hid) const { return c->dt == LLIE_F32 ? pad32(hid) : (hid + 63) / 64 * 64; }  // depthwise: 64 channels per workgroup
  size_t es() const { return elem_size(c->dt); }
  // matrix [rows][cols] stored in compute dtype at an existing destination
  void mat_into(const std::string& key, int rows, int cols, size_t off, int ld, int col0, int* idx = nullptr) {
    Param& p = add(key, (int64_t)rows * cols, PK_MAT, off, idx);
    p.rows = rows; p.cols = cols; p.ld = ld; p.col0 = col0;
    p.ndim = 4; p.shape[0] = rows; p.shape[1] = cols; p.shape[2] = 1; p.shape[3] = 1;  // 1x1 conv weight
  }
  static void set_shape(Param& p, std::initializer_list<int64_t> dims) {
    p.ndim = (int)dims.size();
    int i = 0;
    for (int64_t d : dims) p.shape[i++] = d;
  }
  size_t mat(const std::string& key, int rows, int cols, int* idx, size_t* t_off = nullptr, int rows_p = 0, int cols_p = 0) {
    rows_p = std::max(rows, rows_p); cols_p = std::max(cols, cols_p);
    const size_t o = reserve((size_t)rows_p * cols_p * es());
    mat_into(key, rows, cols, o, cols_p, 0, idx);
    if (t_off) {
      *t_off = reserve((size_t)rows_p * cols_p * es());
      c->params.back().has_t = true;
      c->params.back().t_off = *t_off;
    }
    return o;
  }
  // cin_r / cout_r: the reference's channel counts; x0_r: real channels of the first input segment (== cin_r unless
  // the block reads a virtual concat, whose first segment must be unpadded so that real channels stay contiguous)
  int add_irb(const std::string& p, int cin_r, int cout_r, int T, int e, int x0_r = 0) {
    if (x0_r <= 0) x0_r = cin_r;
    if (x0_r != cin_r && x0_r % 32) bad = true;  // a padded first concat segment would break the real-channel numbering
    IrbW w{};
    w.cin_r = cin_r; w.cout_r = cout_r; w.hid_r = cin_r * e; w.sq = std::max(1, (int)(w.hid_r * 0.25));
    w.cin = x0_r == cin_r ? pad32(cin_r) : x0_r + pad32(cin_r - x0_r);
    w.cout = pad32(cout_r); w.hid = padh(w.hid_r);
    if (w.cin != cin_r || w.cout != cout_r || w.hid != w.hid_r) c->padded = true;
    w.skip = cin_r != cout_r;
    w.n1g = f32(p + ".norm1.weight", cin_r, w.cin, &w.i_n1g); w.n1b = f32(p + ".norm1.bias", cin_r, w.cin, &w.i_n1b);
    w.n2g = f32(p + ".norm2.weight", w.hid_r, w.hid, &w.i_n2g); w.n2b = f32(p + ".norm2.bias", w.hid_r, w.hid, &w.i_n2b);
    w.w_expand = mat(p + ".expand.weight", w.hid_r, cin_r, &w.i_expand, &w.w_expand_t, w.hid, w.cin);
    if (c->dt != LLIE_F32 && w.hid == w.hid_r && w.cin == cin_r && pw_expand_serves_k(w.cin) && w.hid % 64 == 0) {
      // wide blocks of the 2-byte engines: the expand GEMM runs activation-stationary (pwx.hip) from this packed copy
      w.has_wf = true;
      w.w_expand_f = reserve((size_t)w.hid * w.cin * es());
      Param& q = c->params.back();
      q.has_f = true; q.f_off = w.w_expand_f; q.f_scale = 6.f;  // the 6 of ReLU6 carried as clamp01(z / 6), kernels.h
      if (w.cin == kGramWideK && w.hid == 4 * w.cin && w.skip) {
        // the layer irb_path's wide Gram rule can select: norm2's group matrices, rebuilt with the weight (engine.h: IrbPath::wgram)
        w.has_mg = true;
        w.w_mg = reserve((size_t)32 * kGramWideFloats * 8);
        q.has_mg = true; q.mg_off = w.w_mg;
      }
    }
    w.w_dw = reserve((size_t)9 * w.hid * 4);
    w.w_dw_flip = reserve((size_t)9 * w.hid * 4);
    { Param& q = add(p + ".depthwise.weight", (int64_t)w.hid_r * 9, PK_DW, w.w_dw, &w.i_dw); q.O = w.hid_r; q.Op = w.hid; set_shape(q, {w.hid_r, 1, 3, 3});
      q.has_t = true; q.t_off = w.w_dw_flip; }
    w.se_w1 = mat(p + ".se.fc1.weight", w.sq, w.hid_r, &w.i_se_w1, nullptr, w.sq, w.hid); w.se_b1 = f32(p + ".se.fc1.bias", w.sq, 0, &w.i_se_b1);
    w.se_w2 = mat(p + ".se.fc2.weight", w.hid_r, w.sq, &w.i_se_w2, nullptr, w.hid, w.sq); w.se_b2 = f32(p + ".se.fc2.bias", w.hid_r, w.hid, &w.i_se_b2);
    const int kp = w.hid + (w.skip ? w.cin : 0);  // project and skip share one K-concatenated matrix
    w.w_proj = reserve((size_t)w.cout * kp * es());
    w.w_proj_t = reserve((size_t)w.cout * kp * es());  // [kp][cout]: project rows first, then the skip rows
    mat_into(p + ".project.weight", cout_r, w.hid_r, w.w_proj, kp, 0, &w.i_proj);
    c->params.back().has_t = true; c->params.back().t_off = w.w_proj_t;
    // FiLM Linear: rows appended to the global [F][T] fp32 table (filled in finish())
    w.film_off = c->film_rows;
    c->film_rows += 2 * w.hid_r;
    film_keys.push_back({p + ".time_mlp.1", 2 * w.hid_r, w.film_off});
    if (w.skip) pending_skip.push_back({p + ".skip.weight", cout_r, cin_r, w.w_proj, kp, w.hid, w.w_proj_t + (size_t)w.hid * w.cout * es()});
    flush_pending(w);  // registration order: ... project, time_mlp, skip
    c->irbs.push_back(w);
    return (int)c->irbs.size() - 1;
  }
  bool bad = false;
  struct FilmKey { std::string p; int rows, off; };
  struct SkipKey { std::string key; int rows, cols; size_t off; int ld, col0; size_t t_off; };
  std::vector<FilmKey> film_keys;
  std::vector<SkipKey> pending_skip;
  void flush_pending(IrbW& w) {
    // time_mlp.1.{weight,bias} params are created now (to keep registration order) with offsets
    // patched in finish() once the total FiLM row count is known.
    const FilmKey& fk = film_keys.back();
    Param& pw = add(fk.p + ".weight", (int64_t)fk.rows * c->cfg.time_embed_dim, PK_MAT, 0, &w.i_film_w);
    pw.rows = fk.rows; pw.cols = c->cfg.time_embed_dim; pw.ld = pw.cols; pw.col0 = 0; pw.as_t = false;
    set_shape(pw, {fk.rows, c->cfg.time_embed_dim});  // nn.Linear weight
    add(fk.p + ".bias", fk.rows, PK_F32, 0, &w.i_film_b);
    w.i_skip = -1;
    for (auto& s : pending_skip) {
      mat_into(s.key, s.rows, s.cols, s.off, s.ld, s.col0, &w.i_skip);
      c->params.back().has_t = true; c->params.back().t_off = s.t_off;
    }
    pending_skip.clear();
  }
  // soft: StandardAttention (efficient_unet.py:329-332: to_out is a bare conv, no second norm), else LinearAttention (:263-269)
  int add_attn(const std::string& p, int ch, int heads, bool soft) {
    if (ch % 32) bad = true;
    AttnW w{};
    w.c = ch; w.heads = heads; w.inner = heads * 32; w.soft = soft;
    w.ng = f32(p + ".norm.weight", ch, 0, &w.i_ng); w.nb = f32(p + ".norm.bias", ch, 0, &w.i_nb);
    w.w_qkv = mat(p + ".to_qkv.weight", 3 * w.inner, ch, &w.i_qkv, &w.w_qkv_t);
    w.i_n2g = w.i_n2b = -1;
    if (soft) {
      w.w_out = mat(p + ".to_out.weight", ch, w.inner, &w.i_out, &w.w_out_t);
    } else {
      w.w_out = mat(p + ".to_out.0.weight", ch, w.inner, &w.i_out, &w.w_out_t);
      w.n2g = f32(p + ".to_out.1.weight", ch, 0, &w.i_n2g); w.n2b = f32(p + ".to_out.1.bias", ch, 0, &w.i_n2b);
    }
    c->attns.push_back(w);
    return (int)c->attns.size() - 1;
  }
  ConvW add_conv3(const std::string& p, int ch_r, bool up = false) {
    ConvW w{};
    const int ch = pad32(ch_r);
    if (ch != ch_r) c->padded = true;
    w.c = ch; w.c_r = ch_r;
    w.w = reserve((size_t)9 * ch * ch * es());
    w.w_t = reserve((size_t)9 * ch * ch * es());
    { Param& q = add(p + ".weight", (int64_t)ch_r * ch_r * 9, PK_CONV3, w.w, &w.i_w); q.O = ch_r; q.I = ch_r; q.Op = ch; q.Ip = ch;
      set_shape(q, {ch_r, ch_r, 3, 3}); q.has_t = true; q.t_off = w.w_t;
      if (up && c->dt != LLIE_F32 && ch == ch_r) {  // the folded sets of conv3x3_upfold_kernel (engine.h: upconv_fold_supported)
        w.has_fold = true;
        w.w_fold = reserve(upconv_fold_elems(ch) * es());
        q.has_fold = true; q.fold_off = w.w_fold;
      } }
    w.bias = f32(p + ".bias", ch_r, ch, &w.i_bias);
    return w;
  }
  void finish_film() {
    const int T = c->cfg.time_embed_dim;
    c->film_w = reserve((size_t)c->film_rows * T * 4);
    c->film_b = reserve((size_t)c->film_rows * 4);
    for (auto& fk : film_keys) {
      Param& pw = c->params[c->index[fk.p + ".weight"]];
      pw.off = c->film_w + (size_t)fk.off * T * 4;
      Param& pb = c->params[c->index[fk.p + ".bias"]];
      pb.off = c->film_b + (size_t)fk.off * 4;
    }
  }
};

void assign_grad_offsets(llie_ctx* c) {
  int64_t o = 0;
  for (Param& p : c->params) { p.goff = o; o += p.numel; }
  c->grad_numel = o;
}

int build_unet(llie_ctx* c) {
  const llie_config& g = c->cfg;
  Builder b{c};
  c->channels.clear();
  c->channels_r.clear();
  for (int i = 0; i < 4; ++i) {
    c->channels_r.push_back(g.base_channels * g.channel_multipliers[i]);
    c->channels.push_back(pad32(c->channels_r.back()));
  }
  const std::vector<int>& ch = c->channels_r;  // the builder registers parameters with the reference's shapes
  const int T = g.time_embed_dim, e = g.expansion_ratio;
  // GroupNorm(min(32,C), C) must be constructible for every site (efficient_unet.py:170-171,263,528) -- unless the
  // caller opted into the unpinned variants (allow_unpinned: groups = largest divisor <= 32, channels zero-padded)
  auto gn_ok = [](int x) { return x >= 32 && x % 32 == 0; };
  if (g.softmax_attention != 0 && g.softmax_attention != 1) return LLIE_ERR_ARG;
  const bool soft = g.softmax_attention != 0;
  if (g.allow_unpinned) {
    // what the padding scheme needs: the first segment of every virtual concat and every attention input unpadded
    for (int l = 1; l < 4; ++l)
      if (ch[l] % 32) return LLIE_ERR_CONFIG;
    if (g.base_channels < 8 || g.base_channels % 8) return LLIE_ERR_CONFIG;
  } else {
    int in_ch = ch[0];
    for (int l = 0; l < 4; ++l) {
      for (int k = 0; k < g.num_res_blocks; ++k) {
        const int cin = k == 0 ? in_ch : ch[l];
        if (!gn_ok(cin) || !gn_ok(cin * e)) return LLIE_ERR_CONFIG;
      }
      in_ch = ch[l];
    }
    for (int l = 0; l < 4; ++l) {
      const int out = ch[3 - l];
      if (!gn_ok(in_ch + out) || !gn_ok((in_ch + out) * e) || !gn_ok(out) || !gn_ok(out * e)) return LLIE_ERR_CONFIG;
      in_ch = out;
    }
  }
  // three stride-2 levels, each followed by a x2 upsample that must restore the size: any multiple of 8, like the reference
  // (edge tiles of the kernels may be partly empty).  Training needs multiples of 64 (checked in the training entry points).
  if (g.base_channels % 2 || g.image_size % 8 || g.image_size < 64) return LLIE_ERR_SHAPE;
  if (g.in_channels < 2 || g.in_channels > 8 || g.out_channels > 4) return LLIE_ERR_SHAPE;

  c->t_w1 = b.reserve((size_t)T * g.base_channels * 4);
  { Param& p = b.add("time_mlp.1.weight", (int64_t)T * g.base_channels, PK_F32, c->t_w1, &c->i_t_w1); Builder::set_shape(p, {T, g.base_channels}); }
  c->t_b1 = b.f32("time_mlp.1.bias", T, 0, &c->i_t_b1);
  c->t_w3 = b.f32("time_mlp.3.weight", (int64_t)T * T, 0, &c->i_t_w3);
  Builder::set_shape(c->params.back(), {T, T});
  c->t_b3 = b.f32("time_mlp.3.bias", T, 0, &c->i_t_b3);
  const int c0p = c->channels[0];
  if (c0p != ch[0]) c->padded = true;
  c->init_w = b.reserve((size_t)c0p * g.in_channels * 9 * 4);
  { Param& p = b.add("init_conv.weight", (int64_t)ch[0] * g.in_channels * 9, PK_INIT, c->init_w, &c->i_init_w); p.O = ch[0]; p.I = g.in_channels; p.Op = c0p; Builder::set_shape(p, {ch[0], g.in_channels, 3, 3}); }
  c->init_b = b.f32("init_conv.bias", ch[0], c0p, &c->i_init_b);
  c->init_wp = b.reserve((size_t)10 * c0p * 8 * 2);

  int res = g.image_size;
  auto is_attn_res = [&](int r) { return r == g.attention_resolutions[0] || r == g.attention_resolutions[1]; };
  int in_ch = ch[0];
  c->enc.assign(4, {});
  for (int l = 0; l < 4; ++l) {
    int k = 0;
    for (int r = 0; r < g.num_res_blocks; ++r) {
      const std::string p = "encoder_blocks." + std::to_string(l) + "." + std::to_string(k++);
      c->enc[l].push_back({0, b.add_irb(p, r == 0 ? in_ch : ch[l], ch[l], T, e)});
      if (is_attn_res(res)) {
        const std::string pa = "encoder_blocks." + std::to_string(l) + "." + std::to_string(k++);
        c->enc[l].push_back({1, b.add_attn(pa, ch[l], g.num_attention_heads, soft)});
      }
    }
    in_ch = ch[l];
    if (l < 3) res /= 2;
  }
  for (int l = 0; l < 3; ++l) c->downs.push_back(b.add_conv3("downsamplers." + std::to_string(l) + ".down", ch[l]));
  c->mid.push_back({0, b.add_irb("mid_block1", ch[3], ch[3], T, e)});
  c->mid.push_back({1, b.add_attn("mid_attn", ch[3], g.num_attention_heads, soft)});
  c->mid.push_back({0, b.add_irb("mid_block2", ch[3], ch[3], T, e)});
  c->dec.assign(4, {});
  for (int l = 0; l < 4; ++l) {
    const int out = ch[3 - l];
    int k = 0;
    for (int r = 0; r < g.num_res_blocks + 1; ++r) {
      const std::string p = "decoder_blocks." + std::to_string(l) + "." + std::to_string(k++);
      c->dec[l].push_back({0, b.add_irb(p, r == 0 ? in_ch + out : out, out, T, e, r == 0 ? in_ch : 0)});
      if (is_attn_res(res)) {
        const std::string pa = "decoder_blocks." + std::to_string(l) + "." + std::to_string(k++);
        c->dec[l].push_back({1, b.add_attn(pa, out, g.num_attention_heads, soft)});
      }
    }
    in_ch = out;
    if (l < 3) res *= 2;
  }
  for (int l = 0; l < 3; ++l) c->ups.push_back(b.add_conv3("upsamplers." + std::to_string(l) + ".conv", ch[3 - l], true));
  c->fin_g = b.f32("final_norm.weight", ch[0], c0p, &c->i_fin_g);
  c->fin_b = b.f32("final_norm.bias", ch[0], c0p, &c->i_fin_b);
  c->fin_w = b.reserve((size_t)9 * c0p * 4 * 4);
  { Param& p = b.add("final_conv.weight", (int64_t)g.out_channels * ch[0] * 9, PK_FINAL, c->fin_w, &c->i_fin_w); p.O = g.out_channels; p.I = ch[0]; p.Ip = c0p; Builder::set_shape(p, {g.out_channels, ch[0], 3, 3}); }
  c->fin_bias = b.f32("final_conv.bias", g.out_channels, 0, &c->i_fin_bias);
  c->fin_wp = b.reserve((size_t)(c0p / 32) * 18 * 2 * 4 * 8 * 2);
  c->freqs = b.reserve((size_t)(g.base_channels / 2) * 4);
  b.finish_film();
  c->blob_bytes = b.cursor;
  assign_grad_offsets(c);
  if (b.bad) return LLIE_ERR_CONFIG;
  return LLIE_OK;
}

int build_module(llie_ctx* c) {
  const llie_config& g = c->cfg;
  Builder b{c};
  auto gn_ok = [](int x) { return x >= 32 && x % 32 == 0; };
  switch (g.kind) {
    case LLIE_IRB:
      if (!gn_ok(g.in_channels) || !gn_ok(g.in_channels * g.expansion_ratio) || g.out_channels % 32) return LLIE_ERR_CONFIG;
      // a two-tensor (virtual concat) input has no single tensor to add as the identity residual: like every
      // concat-fed block of the network (efficient_unet.py:588), such a block needs Cin != Cout (skip conv)
      if (g.base_channels > 0 && (g.in_channels == g.out_channels || g.base_channels % 32 || g.base_channels >= g.in_channels))
        return LLIE_ERR_SHAPE;
      b.add_irb("", g.in_channels, g.out_channels, g.time_embed_dim, g.expansion_ratio, g.base_channels);
      // keys of a bare block have no leading dot
      break;
    case LLIE_ATTN:
      if (!gn_ok(g.in_channels)) return LLIE_ERR_CONFIG;
      b.add_attn("", g.in_channels, g.num_attention_heads, false);
      break;
    case LLIE_SOFTATTN:
      if (!gn_ok(g.in_channels) || g.num_attention_heads < 1) return LLIE_ERR_CONFIG;
      b.add_attn("", g.in_channels, g.num_attention_heads, true);
      break;
    case LLIE_SE: {  // efficient_unet.py:85-94: squeezed = max(1, int(C * 0.25)), both 1x1 convs with bias
      if (g.in_channels % 32) return LLIE_ERR_CONFIG;
      IrbW w{};
      w.hid = w.hid_r = g.in_channels; w.sq = std::max(1, (int)(g.in_channels * 0.25));
      w.se_w1 = b.mat("fc1.weight", w.sq, w.hid, &w.i_se_w1); w.se_b1 = b.f32("fc1.bias", w.sq, 0, &w.i_se_b1);
      w.se_w2 = b.mat("fc2.weight", w.hid, w.sq, &w.i_se_w2); w.se_b2 = b.f32("fc2.bias", w.hid, 0, &w.i_se_b2);
      c->irbs.push_back(w);
      break;
    }
    case LLIE_DOWN: c->downs.push_back(b.add_conv3("down", g.in_channels)); break;
    case LLIE_UP: c->ups.push_back(b.add_conv3("conv", g.in_channels, true)); break;
    default: return LLIE_ERR_ARG;
  }
  b.finish_film();
  // strip the leading '.' that an empty prefix leaves on block keys
  c->index.clear();
  for (size_t i = 0; i < c->params.size(); ++i) {
    std::string& k = c->params[i].key;
    if (!k.empty() && k[0] == '.') k = k.substr(1);
    c->index[k] = (int)i;
  }
  c->blob_bytes = b.cursor;
  assign_grad_offsets(c);
  return LLIE_OK;
}

}  // namespace

int llie::check_loaded(const llie_ctx* c) {
  for (const Param& p : c->params)
    if (!p.loaded) {
      set_err("parameter '%s' was never loaded", p.key.c_str());
      return LLIE_ERR_NOT_LOADED;
    }
  return LLIE_OK;
}

// a handle created without a device describes the state_dict and the plans, but holds no weights and cannot run
static int need_device(const llie_ctx* c) {
  if (c->blob) return LLIE_OK;
  set_err("no HIP device");
  return LLIE_ERR_NO_DEVICE;
}
int llie::check_ready(const llie_ctx* c) {
  const int rc = need_device(c);
  return rc ? rc : check_loaded(c);
}

int llie::shape_ok(const llie_ctx* c, int H, int W) {
  const int k = c->cfg.kind;
  if (k == LLIE_SOFTATTN) {  // any map of at least 64 pixels, the smallest the network itself runs its GEMMs and norms on
    if (H >= 1 && W >= 1 && (long long)H * W >= 64 && (long long)H * W <= (1 << 24)) return LLIE_OK;
    set_err("unsupported spatial size %dx%d", H, W);
    return LLIE_ERR_SHAPE;
  }
  int minside = 8;
  if (k == LLIE_DOWN) minside = 16;
  if (H % 8 || W % 8 || H < minside || W < minside || (H * W) % 64) {
    set_err("unsupported spatial size %dx%d", H, W);
    return LLIE_ERR_SHAPE;
  }
  return LLIE_OK;
}

int llie::fits(size_t need, int64_t ws_bytes) {
  if ((int64_t)need <= ws_bytes) return LLIE_OK;
  set_err("workspace too small: need %zu, have %lld", need, (long long)ws_bytes);
  return LLIE_ERR_WORKSPACE;
}

int Exec::rc(bool backward) const {
  if (ar->failed) {
    if (backward) set_err("workspace too small for the backward pass");
    else set_err("workspace too small: have %lld bytes", (long long)ar->cap);
    return LLIE_ERR_WORKSPACE;
  }
  if (err != hipSuccess) {
    set_err("HIP error %d: %s", (int)err, hipGetErrorString(err));
    return (int)err;
  }
  return LLIE_OK;
}

extern "C" {

const char* llie_last_error(void) { return g_err; }
const char* llie_version(void) { return "llie-hip 0.1 (gfx950)"; }

int llie_create(const llie_config* cfg, llie_ctx** out) {
  if (!cfg || !out) return LLIE_ERR_ARG;
  if (cfg->compute_dtype < 0 || cfg->compute_dtype > 2) { set_err("bad compute_dtype"); return LLIE_ERR_ARG; }
  if (cfg->kind == LLIE_UNET && cfg->softmax_attention && cfg->allow_unpinned) {
    set_err("softmax_attention together with allow_unpinned (the zero-padded tiny / base variants) is not supported");
    return LLIE_ERR_CONFIG;
  }
  llie_ctx* c = new llie_ctx();
  c->cfg = *cfg;
  c->dt = cfg->compute_dtype;
  const int rc = cfg->kind == LLIE_UNET ? build_unet(c) : build_module(c);
  if (rc != LLIE_OK) {
    if (rc == LLIE_ERR_CONFIG) set_err("num_channels must be divisible by num_groups");  // nn.GroupNorm's ValueError
    else set_err("unsupported configuration");
    delete c;
    return rc;
  }
  int ndev = 0;
  if (hipGetDeviceCount(&ndev) != hipSuccess || ndev == 0) {
    // No device (CPU-only build container): the handle still describes the state_dict, but cannot
    // hold weights or run.  Loading / forward report LLIE_ERR_NO_DEVICE.
    c->blob = nullptr;
    *out = c;
    return LLIE_OK;
  }
  hipError_t e = hipMalloc(reinterpret_cast<void**>(&c->blob), c->blob_bytes ? c->blob_bytes : 256);
  if (e != hipSuccess) { set_err("hipMalloc(%zu) failed: %s", c->blob_bytes, hipGetErrorString(e)); delete c; return (int)e; }
  e = hipMemset(c->blob, 0, c->blob_bytes);
  if (e != hipSuccess) { set_err("hipMemset failed"); (void)hipFree(c->blob); delete c; return (int)e; }
  if (cfg->kind == LLIE_UNET) {
    // SinusoidalPosEmb frequencies (efficient_unet.py:70-73), tabulated once
    const int half = cfg->base_channels / 2;
    std::vector<float> f(half);
    // same fp32 operation chain as torch.exp(-math.log(10000) * torch.arange(half) / half)
    const float neg_ln = (float)(-std::log(10000.0));
    for (int i = 0; i < half; ++i) {
      const float q = (neg_ln * (float)i) / (float)half;
      f[i] = (float)std::exp((double)q);
    }
    e = hipMemcpy(c->blob + c->freqs, f.data(), half * 4, hipMemcpyHostToDevice);
    if (e != hipSuccess) { set_err("hipMemcpy failed"); (void)hipFree(c->blob); delete c; return (int)e; }
  }
  *out = c;
  return LLIE_OK;
}

void llie_destroy(llie_ctx* c) {
  if (!c) return;
  for (auto& kv : c->graphs) {
    if (kv.second.exec) (void)hipGraphExecDestroy(kv.second.exec);
    if (kv.second.graph) (void)hipGraphDestroy(kv.second.graph);
  }
  if (c->cap_stream) (void)hipStreamDestroy(c->cap_stream);
  if (c->side_stream) (void)hipStreamDestroy(c->side_stream);
  for (int i = 0; i < kMaxBranches; ++i) {
    if (c->branch_stream[i]) (void)hipStreamDestroy(c->branch_stream[i]);
    if (c->branch_join[i]) (void)hipEventDestroy(c->branch_join[i]);
  }
  if (c->ev_fork) (void)hipEventDestroy(c->ev_fork);
  if (c->ev_join) (void)hipEventDestroy(c->ev_join);
  for (auto& r : c->prof) { (void)hipEventDestroy(r.e0); (void)hipEventDestroy(r.e1); }
  for (hipEvent_t e : c->event_pool) (void)hipEventDestroy(e);
  if (c->blob) (void)hipFree(c->blob);
  delete c->train_arena;
  if (c->load_descs) (void)hipFree(c->load_descs);
  if (c->hash_partial) (void)hipFree(c->hash_partial);
  if (c->hash_state) (void)hipFree(c->hash_state);
  delete c;
}

int llie_num_params(const llie_ctx* c) { return c ? (int)c->params.size() : LLIE_ERR_ARG; }

int llie_param_info(const llie_ctx* c, int i, char* key, size_t cap, int64_t* numel, int* ndim, int64_t* shape4) {
  if (!c || i < 0 || i >= (int)c->params.size()) return LLIE_ERR_ARG;
  if (key && cap) {
    strncpy(key, c->params[i].key.c_str(), cap - 1);
    key[cap - 1] = 0;
  }
  if (numel) *numel = c->params[i].numel;
  if (ndim) *ndim = c->params[i].ndim;
  if (shape4)
    for (int d = 0; d < 4; ++d) shape4[d] = c->params[i].shape[d];
  return LLIE_OK;
}

// The one statement of what is loaded where for a parameter: the main destination, which secondary copies exist, and the padded
// destination dims.  The refusals of the engine layouts need no check here, because no handle with such a parameter exists:
// build_unet rejects in_channels > 8 (the input conv's MFMA pack holds 8) and out_channels > 4 (the output conv's layouts hold 4),
// the output conv's Ip is channels[0] = pad32(.), a multiple of 32 by construction, and build_module never registers either conv;
// the fragment-order copy (has_f) is reserved only for rows % 64 == 0 and pw_expand_serves_k(cols), all multiples of 16.
static LoadDesc make_desc(const llie_ctx* c, const Param& p, const float* src) {
  LoadDesc d{};
  d.src = src; d.kind = p.kind; d.numel = p.numel; d.dst = (long long)p.off;
  d.as_t = p.as_t ? 1 : 0; d.rows = p.rows; d.cols = p.cols; d.ld = p.ld; d.col0 = p.col0;
  d.O = p.O; d.I = p.I; d.Op = p.Op > 0 ? p.Op : p.O; d.Ip = p.Ip > 0 ? p.Ip : p.I;
  // the transposed copies feed the backward pass, which the padded (unpinned) variants do not have; the flipped depthwise
  // taps are written all the same (their blob space is reserved and padded like the main copy)
  d.dst_t = p.has_t && (!c->padded || p.kind == PK_DW) ? (long long)p.t_off : -1;
  d.dst_f = p.has_f ? (long long)p.f_off : -1; d.fscale = p.f_scale;
  // the 2-byte engines' input / output convs run on MFMA from a pack of their own
  if (p.kind == PK_INIT) d.dst_t = c->dt != LLIE_F32 ? (long long)c->init_wp : -1;
  if (p.kind == PK_FINAL) d.dst_t = c->dt != LLIE_F32 ? (long long)c->fin_wp : -1;
  return d;
}

int llie_load_param(llie_ctx* c, const char* key, const float* src, int64_t numel, llie_stream stream) {
  if (!c || !key || !src) return LLIE_ERR_ARG;
  if (const int rc = need_device(c)) return rc;
  auto it = c->index.find(key);
  if (it == c->index.end()) { set_err("unexpected key '%s'", key); return LLIE_ERR_KEY; }
  Param& p = c->params[it->second];
  if (p.numel != numel) { set_err("size mismatch for '%s': expected %lld elements, got %lld", key, (long long)p.numel, (long long)numel); return LLIE_ERR_KEY; }
  hipStream_t s = hs(stream);
  hipError_t e = launch_load_one(c->dt, make_desc(c, p, src), c->blob, s);
  if (e == hipSuccess && p.has_fold) e = launch_upconv_fold(c->dt, src, c->blob + p.fold_off, p.O, s);
  if (e == hipSuccess && p.has_mg) e = launch_gram_group_weights(c->dt, c->blob + p.f_off, reinterpret_cast<double*>(c->blob + p.mg_off), p.rows, p.cols, s);
  if (e != hipSuccess) { set_err("repack of '%s' failed: %s", key, hipGetErrorString(e)); return (int)e; }
  p.loaded = true;
  // the blob no longer holds what the last llie_load_all wrote, whose content hash a llie_refresh_params of the same tensors
  // would find unchanged: forget its sources, so that the next batched call rebuilds its table and loads unconditionally
  c->load_srcs.clear();
  return LLIE_OK;
}

// Reload every parameter from `srcs[i]` (device fp32, llie_param_info order) -- what an optimiser step needs.  Everything
// goes through one kernel driven by a descriptor table that is rebuilt only when a source pointer changes.
// conditional != 0 (llie_refresh_params): the reload happens on the device only if the parameters' content hash differs
// from the one of the last load -- no host round trip, ~3 small launches when nothing changed.
static int load_all_impl(llie_ctx* c, const float* const* srcs, int n, llie_stream stream, int conditional) {
  if (!c || !srcs || n != (int)c->params.size()) return LLIE_ERR_ARG;
  if (const int rc = need_device(c)) return rc;
  hipStream_t s = hs(stream);
  for (int i = 0; i < n; ++i)
    if (!srcs[i]) return LLIE_ERR_ARG;
  bool rebuild = !c->load_descs || (int)c->load_srcs.size() != n;
  for (int i = 0; !rebuild && i < n; ++i) rebuild = c->load_srcs[i] != srcs[i];
  if (rebuild) {
    std::vector<LoadDesc> d;
    for (int i = 0; i < n; ++i) d.push_back(make_desc(c, c->params[i], srcs[i]));
    hipError_t e = hipSuccess;
    if (!c->load_descs) e = hipMalloc(reinterpret_cast<void**>(&c->load_descs), sizeof(LoadDesc) * c->params.size());
    if (e == hipSuccess && !c->hash_partial) e = hipMalloc(reinterpret_cast<void**>(&c->hash_partial), sizeof(unsigned long long) * 32 * c->params.size());
    if (e == hipSuccess && !c->hash_state) {
      e = hipMalloc(reinterpret_cast<void**>(&c->hash_state), 2 * sizeof(unsigned long long));
      if (e == hipSuccess) e = hipMemsetAsync(c->hash_state, 0, 2 * sizeof(unsigned long long), s);
    }
    // pageable host memory: the copy is staged before the call returns, so the vector may go out of scope
    if (e == hipSuccess) e = hipMemcpyAsync(c->load_descs, d.data(), sizeof(LoadDesc) * d.size(), hipMemcpyHostToDevice, s);
    if (e == hipSuccess) e = hipStreamSynchronize(s);
    if (e != hipSuccess) { set_err("llie_load_all: %s", hipGetErrorString(e)); return (int)e; }
    c->load_srcs.assign(srcs, srcs + n);
    conditional = 0;
  }
  hipError_t e = launch_params_hash(c->load_descs, n, c->hash_partial, c->hash_state, conditional ? 0 : 1, s);
  if (e == hipSuccess) e = launch_load_all(c->dt, c->load_descs, n, c->blob, s, c->hash_state);
  // the up-sampling convs' folded sets gather nine source values per element: a launch of their own, under the same "changed" flag
  for (int i = 0; e == hipSuccess && i < n; ++i)
    if (c->params[i].has_fold) e = launch_upconv_fold(c->dt, srcs[i], c->blob + c->params[i].fold_off, c->params[i].O, s, c->hash_state);
  // and norm2's group matrices of the wide Gram form, from the packed weights the kernel above has just written: under the same flag
  for (int i = 0; e == hipSuccess && i < n; ++i)
    if (c->params[i].has_mg)
      e = launch_gram_group_weights(c->dt, c->blob + c->params[i].f_off, reinterpret_cast<double*>(c->blob + c->params[i].mg_off), c->params[i].rows,
                                    c->params[i].cols, s, c->hash_state);
  if (e != hipSuccess) { set_err("llie_load_all: %s", hipGetErrorString(e)); return (int)e; }
  for (int i = 0; i < n; ++i) c->params[i].loaded = true;
  return LLIE_OK;
}
int llie_load_all(llie_ctx* c, const float* const* srcs, int n, llie_stream stream) { return load_all_impl(c, srcs, n, stream, 0); }
int llie_refresh_params(llie_ctx* c, const float* const* srcs, int n, llie_stream stream) { return load_all_impl(c, srcs, n, stream, 1); }

int llie_params_loaded(const llie_ctx* c) {
  if (!c) return 0;
  for (const Param& p : c->params)
    if (!p.loaded) return 0;
  return 1;
}

// SURVEY.md 8d byte model: IRB (2Cin + 4Chid + Cout)P, attention 6CP, dense 3x3 Cin*Pin + Cout*Pout,
// final C0*P + 3P, LCM step 12P fp32; activations at the compute dtype; weights once.
// engine != 0: what the engine's own kernel selection has to move -- blocks that run in the recompute form (irbx.hip)
// read x three times and never store h1: (3Cin + 2Chid + Cout) P (SURVEY.md 8d "recompute variant").  x0c = channels of
// the first input segment of the first block (virtual concat), 0 = none.  Blocks that also take the project form
// (irb_path: h2 stays on chip) move (4Cin + Cout) P: x is read by the statistics pass, the pool pass, the main pass and
// the shortcut, y is written.  The wide form (irb_path: the two decoder blocks without h2) is charged exactly as unfused, so
// llie_path_bytes keeps its integers at every knob setting: it over-charges those two blocks by about 0.6 Chid P from now on
// (they move 2Cin + 3.4 Chid + Cout: h1 written, read by the pool pass, read with its halo by dwconv3x3_project).
static void count_blocks(const llie_ctx* c, const std::vector<Block>& bl, int64_t P, int64_t& elems, int64_t& flops, int engine = 0,
                         int x0c = 0) {
  bool first = true;
  for (const Block& b : bl) {
    if (b.kind == 0) {
      const IrbW& w = c->irbs[b.idx];
      const int S = (int)std::lround(std::sqrt((double)P));
      const IrbForm form = engine ? irb_path(c->dt, w, (first && x0c) ? x0c : w.cin, S, S, false).form : kIrbUnfused;
      first = false;
      if (form == kIrbProject) elems += (4LL * w.cin + w.cout) * P;
      else if (form == kIrbRecompute) elems += (3LL * w.cin + 2LL * w.hid + w.cout) * P;
      else elems += (2LL * w.cin + 4LL * w.hid + w.cout) * P;
      flops += 2LL * P * ((int64_t)w.cin * w.hid + 9LL * w.hid + (int64_t)w.hid * w.cout + (w.skip ? (int64_t)w.cin * w.cout : 0));
    } else {
      const AttnW& w = c->attns[b.idx];
      if (w.soft) {
        // x read by the qkv GEMM and as the residual, y written; the core reads qkv and writes out, which the GEMMs wrote / read:
        // 3C + 8 inner elements per pixel; the core's two products are 4 N^2 inner flops per image
        elems += (3LL * w.c + 8LL * w.inner) * P;
        flops += 2LL * P * ((int64_t)w.c * 3 * w.inner + (int64_t)w.inner * w.c) + 4LL * P * P * w.inner;
        continue;
      }
      elems += 6LL * w.c * P;
      flops += 2LL * P * ((int64_t)w.c * 3 * w.inner + (int64_t)w.inner * w.c + 2LL * w.inner * 32);
    }
  }
}
static void model_counts(const llie_ctx* c, int64_t& elems, int64_t& flops, int engine = 0) {
  elems = flops = 0;
  if (c->cfg.kind != LLIE_UNET) return;
  const int S = c->cfg.image_size;
  int64_t P = (int64_t)S * S;
  const std::vector<int>& ch = c->channels;
  elems += (int64_t)c->cfg.in_channels * P + ch[0] * P;
  flops += 2LL * P * 9 * c->cfg.in_channels * ch[0];
  for (int l = 0; l < 4; ++l) {
    count_blocks(c, c->enc[l], P, elems, flops, engine);
    if (l < 3) {
      elems += ch[l] * P + ch[l] * (P / 4);
      flops += 2LL * (P / 4) * 9 * ch[l] * ch[l];
      P /= 4;
    }
  }
  count_blocks(c, c->mid, P, elems, flops, engine);
  for (int l = 0; l < 4; ++l) {
    if (l > 0) {
      const int cc = ch[4 - l];
      elems += (int64_t)cc * P + (int64_t)cc * P * 4;
      flops += 2LL * (P * 4) * 9 * cc * cc;
      P *= 4;
    }
    count_blocks(c, c->dec[l], P, elems, flops, engine, l == 0 ? ch[3] : ch[4 - l]);
  }
  elems += (int64_t)ch[0] * P + 3 * P;
  flops += 2LL * P * 9 * ch[0] * c->cfg.out_channels;
}

static int64_t model_bytes(llie_ctx* c, int batch, int engine) {
  if (!c) return LLIE_ERR_ARG;
  int64_t elems, flops;
  model_counts(c, elems, flops, engine);
  int64_t wbytes = 0;
  for (const Param& p : c->params) wbytes += p.numel * (p.kind == PK_F32 || !p.as_t ? 4 : (int64_t)elem_size(c->dt));
  return elems * batch * (int64_t)elem_size(c->dt) + wbytes;
}
int64_t llie_algorithmic_bytes(llie_ctx* c, int batch) { return model_bytes(c, batch, 0); }
int64_t llie_path_bytes(llie_ctx* c, int batch) { return model_bytes(c, batch, 1); }
// The form irb_path picks for every inverted-residual block of a UNet whose full-resolution map is H x W (inference), in forward
// order: six ints per block (cin, hid, cout, block H, block W, IrbForm).  Returns the number of blocks, or LLIE_ERR_ARG.
int llie_irb_forms(llie_ctx* c, int H, int W, int* out6, int cap_blocks) {
  if (!c || c->cfg.kind != LLIE_UNET || H <= 0 || W <= 0 || (cap_blocks > 0 && !out6)) return LLIE_ERR_ARG;
  int n = 0;
  auto walk = [&](const std::vector<Block>& bl, int h, int w, int x0c) {
    bool first = true;
    for (const Block& b : bl) {
      if (b.kind != 0) { first = false; continue; }
      const IrbW& iw = c->irbs[b.idx];
      const IrbForm form = irb_path(c->dt, iw, (first && x0c) ? x0c : iw.cin, h, w, false).form;
      first = false;
      if (n < cap_blocks) {
        int* o = out6 + 6 * n;
        o[0] = iw.cin; o[1] = iw.hid; o[2] = iw.cout; o[3] = h; o[4] = w; o[5] = (int)form;
      }
      ++n;
    }
  };
  const std::vector<int>& ch = c->channels;
  int h = H, w = W;
  for (int l = 0; l < 4; ++l) {
    walk(c->enc[l], h, w, 0);
    if (l < 3) { h /= 2; w /= 2; }
  }
  walk(c->mid, h, w, 0);
  for (int l = 0; l < 4; ++l) {
    if (l > 0) { h *= 2; w *= 2; }
    walk(c->dec[l], h, w, l == 0 ? ch[3] : ch[4 - l]);
  }
  return n;
}
// Which of those blocks take the wide Gram form (IrbPath::wgram), same walk and order: one int per block.  Returns the number of blocks.
int llie_irb_wide_gram(llie_ctx* c, int H, int W, int* out1, int cap_blocks) {
  if (!c || c->cfg.kind != LLIE_UNET || H <= 0 || W <= 0 || (cap_blocks > 0 && !out1)) return LLIE_ERR_ARG;
  int n = 0;
  auto walk = [&](const std::vector<Block>& bl, int h, int w, int x0c) {
    bool first = true;
    for (const Block& b : bl) {
      if (b.kind != 0) { first = false; continue; }
      const IrbW& iw = c->irbs[b.idx];
      if (n < cap_blocks) out1[n] = irb_path(c->dt, iw, (first && x0c) ? x0c : iw.cin, h, w, false).wgram ? 1 : 0;
      first = false;
      ++n;
    }
  };
  const std::vector<int>& ch = c->channels;
  int h = H, w = W;
  for (int l = 0; l < 4; ++l) {
    walk(c->enc[l], h, w, 0);
    if (l < 3) { h /= 2; w /= 2; }
  }
  walk(c->mid, h, w, 0);
  for (int l = 0; l < 4; ++l) {
    if (l > 0) { h *= 2; w *= 2; }
    walk(c->dec[l], h, w, l == 0 ? ch[3] : ch[4 - l]);
  }
  return n;
}
int64_t llie_flops(llie_ctx* c, int batch) {
  if (!c) return LLIE_ERR_ARG;
  int64_t elems, flops;
  model_counts(c, elems, flops);
  return flops * batch;
}

}  // extern "C"
