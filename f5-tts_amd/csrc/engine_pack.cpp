// f5h engine: weight packing and engine creation / release (see engine_internal.h for the map of the engine's files).
#include "engine_internal.h"

static constexpr size_t kProbeBytes = (64 + 2 * (size_t)kProbeEnd) * sizeof(unsigned long long);

// ---------------------------------------------------------------- weight packing
// Weights arrive as typed views (f5h_tensor_view: fp32/bf16/fp16, host or device memory, the
// reference's parameter dtype and placement, utils_infer.py:190-232). Host views are staged to the
// device once in their own dtype; every panel is then packed on the device by pack_strided
// (reorder, zero padding, rounding to the operand dtype), so no host fp32 copy of the model exists.
struct WView {
  const void* p;      // device pointer (staged when the caller's view was in host memory)
  int dt;             // f5h_dtype
  int64_t numel;
};
struct WMap {
  std::unordered_map<std::string, WView> m;
  const WView* get(const std::string& n, int64_t numel, std::string* err) const {
    auto it = m.find(n);
    if (it == m.end()) {
      *err = "missing weight " + n;
      return nullptr;
    }
    if (it->second.numel != numel) {
      *err = "weight " + n + " has " + std::to_string(it->second.numel) + " elements, expected " +
             std::to_string(numel);
      return nullptr;
    }
    return &it->second;
  }
};

// device buffer owned by the engine (stream-ordered pool, reaper.h: its release never syncs the device)
static int ealloc(f5h_engine* e, size_t bytes, void** out) {
  void* p = dev_alloc(e->dev, bytes, e->mstream);
  if (!p) return fail(F5H_EHIP, "device allocation of " + std::to_string(bytes) + " bytes");
  e->allocs.push_back(p);
  *out = p;
  return 0;
}

template <typename T>
static int upload(f5h_engine* e, const std::vector<T>& h, T** out) {
  void* p = nullptr;
  RC(ealloc(e, h.size() * sizeof(T) + 16, &p));
  HIPCK(hipMemcpyAsync(p, h.data(), h.size() * sizeof(T), hipMemcpyHostToDevice, e->mstream));
  HIPCK(hipStreamSynchronize(e->mstream));  // the host vector may go away after the return
  *out = reinterpret_cast<T*>(p);
  return 0;
}

// zeroed device buffer owned by the engine
static int dalloc(f5h_engine* e, size_t bytes, void** out) {
  void* p = nullptr;
  RC(ealloc(e, bytes + 16, &p));
  HIPCK(hipMemsetAsync(p, 0, bytes + 16, e->mstream));
  *out = p;
  return 0;
}

// op element type of the engine (f5h_dtype numbering: 0 fp32, 1 bf16, 2 fp16 == f5h_compute)
static int op_dt(const f5h_engine* e) { return e->bf; }

// dst[r][dst_col + c] (row stride ld_dst, element type ddt) = src[r][col0 + c] (row stride ld_src)
static int pack_rows(const WView& v, int rows, int64_t ld_src, int col0, int ncols, void* dst, int ddt,
                     int64_t ld_dst, int dst_row0, int dst_col, hipStream_t st) {
  PackArgs pa{};
  pa.src = v.p;
  pa.src_dt = v.dt;
  pa.src_st[0] = 0;
  pa.src_st[1] = 0;
  pa.src_st[2] = ld_src;
  pa.src_st[3] = 1;
  const size_t esz = ddt ? 2 : 4;
  pa.dst = (char*)dst + ((size_t)dst_row0 * ld_dst + dst_col) * esz;
  // the source column offset goes into the base pointer
  pa.src = (const char*)v.p + (size_t)col0 * (v.dt ? 2 : 4);
  pa.dst_dt = ddt;
  pa.dst_st[0] = 0;
  pa.dst_st[1] = 0;
  pa.dst_st[2] = ld_dst;
  pa.n[0] = 1;
  pa.n[1] = 1;
  pa.n[2] = rows;
  pa.n[3] = ncols;
  HIPCK(pack_strided(pa, st));
  return 0;
}

// Build a GEMM panel [Npad][K] (operand dtype, zero padded) from column blocks of several source
// matrices stacked along N, plus an fp32 bias [Npad] from per-block bias vectors (null: zeros).
struct Block {
  const WView* src;   // [rows][ld]
  int rows, ld, col0, ncols, dst_col;
};
static int make_lin(f5h_engine* e, const std::vector<Block>& blocks, int K, const std::vector<const WView*>& biases,
                    Lin* L) {
  int N = 0;
  for (const Block& b : blocks) N += b.rows;
  L->N = N;
  L->K = K;
  L->Npad = (N + 127) / 128 * 128;
  RC(dalloc(e, (size_t)L->Npad * K * e->esz, &L->w));
  int r0 = 0;
  for (const Block& b : blocks) {
    RC(pack_rows(*b.src, b.rows, b.ld, b.col0, b.ncols, L->w, op_dt(e), K, r0, b.dst_col, e->mstream));
    r0 += b.rows;
  }
  if (!biases.empty()) {
    void* bp;
    RC(dalloc(e, (size_t)L->Npad * sizeof(float), &bp));
    L->b = reinterpret_cast<float*>(bp);
    r0 = 0;
    for (size_t i = 0; i < blocks.size(); ++i) {
      if (i < biases.size() && biases[i])
        RC(pack_rows(*biases[i], 1, 0, 0, blocks[i].rows, L->b, 0, 0, 0, r0, e->mstream));
      r0 += blocks[i].rows;
    }
  }
  return 0;
}
// Simple linear: weight [N][K] (K padded to 64), bias [N] or none.
static int lin_simple(f5h_engine* e, const WMap& W, const std::string& wn, const std::string& bn, int N, int K,
                      Lin* L, std::string* err) {
  const WView* w = W.get(wn, (int64_t)N * K, err);
  if (!w) return fail(F5H_ENOWEIGHT, *err);
  const WView* b = nullptr;
  if (!bn.empty()) {
    b = W.get(bn, N, err);
    if (!b) return fail(F5H_ENOWEIGHT, *err);
  }
  const int Kp = (K + 63) / 64 * 64;
  return make_lin(e, {Block{w, N, K, 0, K, 0}}, Kp, b ? std::vector<const WView*>{b} : std::vector<const WView*>{},
                  L);
}
// fp32 device copy of a vector parameter
static int vec_upload(f5h_engine* e, const WMap& W, const std::string& n, int64_t numel, float** out, std::string* err) {
  const WView* v = W.get(n, numel, err);
  if (!v) return fail(F5H_ENOWEIGHT, *err);
  void* p;
  RC(dalloc(e, (size_t)numel * sizeof(float), &p));
  RC(pack_rows(*v, 1, 0, 0, (int)numel, p, 0, 0, 0, 0, e->mstream));
  *out = reinterpret_cast<float*>(p);
  return 0;
}

// ConvPositionEmbedding weight [d, d/16, 31] (element type src_dt) -> the conv kernels' panel [16][31][64 out][64 in]
// (element type dst_dt): dst (g, t, o, i) <- src ((g*cg + o)*cg + i)*31 + t, cg = d / 16. dst holds kConvPackElems
// elements and is zero on entry (groups narrower than 64 channels keep zero padding). Engine creation and
// f5h_op_conv_pos both pack through here.
int pack_conv_weight(const void* src, int src_dt, int d, void* dst, int dst_dt, hipStream_t st) {
  const int cg = d / 16;
  PackArgs pa{};
  pa.src = src;
  pa.src_dt = src_dt;
  pa.src_st[0] = (int64_t)cg * cg * 31;  // g
  pa.src_st[1] = 1;                      // t
  pa.src_st[2] = (int64_t)cg * 31;       // o
  pa.src_st[3] = 31;                     // i
  pa.dst = dst;
  pa.dst_dt = dst_dt;
  pa.dst_st[0] = 31 * 64 * 64;
  pa.dst_st[1] = 64 * 64;
  pa.dst_st[2] = 64;
  pa.n[0] = 16;
  pa.n[1] = 31;
  pa.n[2] = cg;
  pa.n[3] = cg;
  HIPCK(pack_strided(pa, st));
  return 0;
}

// ConvPositionEmbedding under `prefix` (conv1d.0 and conv1d.2): the weights as the conv kernels' panels, the biases
static int pack_conv_pos(f5h_engine* e, const WMap& W, const std::string& prefix, std::string* err) {
  const int d = e->a.dim;
  for (int j = 0; j < 2; ++j) {
    const std::string p = prefix + std::to_string(j * 2) + ".";
    const WView* w = W.get(p + "weight", (int64_t)d * (d / 16) * 31, err);
    if (!w) return fail(F5H_ENOWEIGHT, *err);
    RC(dalloc(e, kConvPackElems * e->esz, &e->conv_w[j]));
    RC(pack_conv_weight(w->p, w->dt, d, e->conv_w[j], op_dt(e), e->mstream));
    RC(vec_upload(e, W, p + "bias", d, &e->conv_b[j], err));
  }
  return 0;
}

// precompute_freqs_cis(dim, rows) (modules.py:207-218): [rows][cos(p f_i) for i < dim/2 | sin(p f_i)]
static std::vector<float> freqs_cis(int dim, int rows) {
  std::vector<float> fc((size_t)rows * dim);
  const int half = dim / 2;
  for (int p = 0; p < rows; ++p)
    for (int i = 0; i < half; ++i) {
      float f = 1.0f / std::pow(10000.0f, (float)(2 * i) / (float)dim);
      float ang = (float)p * f;
      fc[(size_t)p * dim + i] = std::cos(ang);
      fc[(size_t)p * dim + half + i] = std::sin(ang);
    }
  return fc;
}

// [q | k | v] panel of three [inner][d] linears with their biases
static int pack_qkv(f5h_engine* e, const WMap& W, const std::string& pa, const char* sfx, int inner, int d, Lin* L,
                    std::string* err) {
  const WView *w[3], *b[3];
  const char* n[3] = {"to_q", "to_k", "to_v"};
  for (int j = 0; j < 3; ++j) {
    w[j] = W.get(pa + n[j] + sfx + ".weight", (int64_t)inner * d, err);
    if (!w[j]) return fail(F5H_ENOWEIGHT, *err);
    b[j] = W.get(pa + n[j] + sfx + ".bias", inner, err);
    if (!b[j]) return fail(F5H_ENOWEIGHT, *err);
  }
  return make_lin(e, {Block{w[0], inner, d, 0, d, 0}, Block{w[1], inner, d, 0, d, 0}, Block{w[2], inner, d, 0, d, 0}},
                  d, {b[0], b[1], b[2]}, L);
}

// MMDiT (mmdit.py:87-133) under the reference's names
static int pack_mmdit(f5h_engine* e, const WMap& W) {
  const f5h_arch& a = e->a;
  const int d = a.dim, inner = a.heads * a.dim_head, F = a.ff_dim, mel = a.mel_dim;
  const int V = a.text_num_embeds + 1;
  std::string err;
  RC(lin_simple(e, W, "time_embed.time_mlp.0.weight", "time_embed.time_mlp.0.bias", d, 256, &e->t1, &err));
  RC(lin_simple(e, W, "time_embed.time_mlp.2.weight", "time_embed.time_mlp.2.bias", d, d, &e->t2, &err));
  RC(vec_upload(e, W, "text_embed.text_embed.weight", (int64_t)V * d, &e->text_table, &err));
  RC(upload(e, freqs_cis(d, kMMTextPos), &e->freqs));
  // audio_embed.linear over cat(x, cond) (mmdit.py:78-79): the x columns per evaluation, the cond columns and the bias
  // hoisted (the DiT input projection without its text columns)
  {
    const WView* w = W.get("audio_embed.linear.weight", (int64_t)d * 2 * mel, &err);
    const WView* b = w ? W.get("audio_embed.linear.bias", d, &err) : nullptr;
    if (!w || !b) return fail(F5H_ENOWEIGHT, err);
    RC(make_lin(e, {Block{w, d, 2 * mel, 0, mel, 0}}, 128, {}, &e->in_x));
    RC(make_lin(e, {Block{w, d, 2 * mel, mel, mel, 0}}, 128, {b}, &e->in_ct));
  }
  RC(pack_conv_pos(e, W, "audio_embed.conv_pos_embed.conv1d.", &err));
  e->layers.resize(a.depth);
  std::vector<Block> ada_blocks;
  std::vector<const WView*> ada_bias;
  auto ada_push = [&](const std::string& n, int rows) -> int {
    const WView* aw = W.get(n + ".linear.weight", (int64_t)rows * d, &err);
    const WView* ab = aw ? W.get(n + ".linear.bias", rows, &err) : nullptr;
    if (!aw || !ab) return fail(F5H_ENOWEIGHT, err);
    ada_blocks.push_back(Block{aw, rows, d, 0, d, 0});
    ada_bias.push_back(ab);
    return 0;
  };
  for (int l = 0; l < a.depth; ++l) {
    Layer& L = e->layers[l];
    const bool last = l == a.depth - 1;  // context_pre_only (mmdit.py:124)
    const std::string p = "transformer_blocks." + std::to_string(l) + ".";
    const std::string pa = p + "attn.";
    RC(ada_push(p + "attn_norm_x", 6 * d));
    RC(ada_push(p + "attn_norm_c", last ? 2 * d : 6 * d));
    RC(pack_qkv(e, W, pa, "", inner, d, &L.qkv, &err));
    RC(pack_qkv(e, W, pa, "_c", inner, d, &L.qkv_c, &err));
    if (a.qk_norm) {
      const char* nn[4] = {"q_norm.weight", "k_norm.weight", "c_q_norm.weight", "c_k_norm.weight"};
      float** dst[4] = {&L.q_norm_w, &L.k_norm_w, &L.cq_norm_w, &L.ck_norm_w};
      for (int j = 0; j < 4; ++j) {
        if (!W.get(pa + nn[j], a.dim_head, &err)) return fail(F5H_ENOWEIGHT, "qk_norm: " + err);
        RC(vec_upload(e, W, pa + nn[j], a.dim_head, dst[j], &err));
      }
    }
    RC(lin_simple(e, W, pa + "to_out.0.weight", pa + "to_out.0.bias", d, inner, &L.out, &err));
    RC(lin_simple(e, W, p + "ff_x.ff.0.0.weight", p + "ff_x.ff.0.0.bias", F, d, &L.ff1, &err));
    RC(lin_simple(e, W, p + "ff_x.ff.2.weight", p + "ff_x.ff.2.bias", d, F, &L.ff2, &err));
    if (!last) {
      RC(lin_simple(e, W, pa + "to_out_c.weight", pa + "to_out_c.bias", d, inner, &L.out_c, &err));
      RC(lin_simple(e, W, p + "ff_c.ff.0.0.weight", p + "ff_c.ff.0.0.bias", F, d, &L.ff1_c, &err));
      RC(lin_simple(e, W, p + "ff_c.ff.2.weight", p + "ff_c.ff.2.bias", d, F, &L.ff2_c, &err));
    }
  }
  RC(ada_push("norm_out", 2 * d));
  RC(make_lin(e, ada_blocks, d, ada_bias, &e->ada));
  RC(lin_simple(e, W, "proj_out.weight", "proj_out.bias", mel, d, &e->proj_out, &err));
  return 0;
}

static int pack_all(f5h_engine* e, const WMap& W) {
  const f5h_arch& a = e->a;
  if (a.backbone == F5H_MMDIT) return pack_mmdit(e, W);
  const int d = a.dim, inner = a.heads * a.dim_head, F = a.ff_dim, td = a.text_dim, mel = a.mel_dim;
  const int V = a.text_num_embeds + 1;
  std::string err;
  // time MLP (modules.py:852-862)
  RC(lin_simple(e, W, "time_embed.time_mlp.0.weight", "time_embed.time_mlp.0.bias", d, 256, &e->t1, &err));
  RC(lin_simple(e, W, "time_embed.time_mlp.2.weight", "time_embed.time_mlp.2.bias", d, d, &e->t2, &err));
  // text table
  RC(vec_upload(e, W, "text_embed.text_embed.weight", (int64_t)V * td, &e->text_table, &err));
  if (a.conv_layers > 0) RC(upload(e, freqs_cis(td, 8192), &e->freqs));
  e->cnx.resize(a.conv_layers);
  for (int i = 0; i < a.conv_layers; ++i) {
    const std::string p = "text_embed.text_blocks." + std::to_string(i) + ".";
    CNX& c = e->cnx[i];
    RC(vec_upload(e, W, p + "dwconv.weight", (int64_t)td * 7, &c.dw_w, &err));
    RC(vec_upload(e, W, p + "dwconv.bias", td, &c.dw_b, &err));
    RC(vec_upload(e, W, p + "norm.weight", td, &c.ln_w, &err));
    RC(vec_upload(e, W, p + "norm.bias", td, &c.ln_b, &err));
    RC(vec_upload(e, W, p + "grn.gamma", 2 * td, &c.gamma, &err));
    RC(vec_upload(e, W, p + "grn.beta", 2 * td, &c.beta, &err));
    RC(lin_simple(e, W, p + "pwconv1.weight", p + "pwconv1.bias", 2 * td, td, &c.pw1, &err));
    RC(lin_simple(e, W, p + "pwconv2.weight", p + "pwconv2.bias", td, 2 * td, &c.pw2, &err));
  }
  // input projection split (dit.py:162): [x | cond | text] -> x part per step, cond|text hoisted
  {
    const int Kin = 2 * mel + td;
    const WView* w = W.get("input_embed.proj.weight", (int64_t)d * Kin, &err);
    const WView* b = w ? W.get("input_embed.proj.bias", d, &err) : nullptr;
    if (!w || !b) return fail(F5H_ENOWEIGHT, err);
    RC(make_lin(e, {Block{w, d, Kin, 0, mel, 0}}, 128, {}, &e->in_x));
    // cond columns -> [0,128), text columns -> [128, 128+tdp): two column blocks of the same rows
    const int Kct = 128 + e->tdp;
    Lin& L = e->in_ct;
    L.N = d;
    L.K = Kct;
    L.Npad = (d + 127) / 128 * 128;
    RC(dalloc(e, (size_t)L.Npad * Kct * e->esz, &L.w));
    RC(pack_rows(*w, d, Kin, mel, mel, L.w, op_dt(e), Kct, 0, 0, e->mstream));
    RC(pack_rows(*w, d, Kin, 2 * mel, td, L.w, op_dt(e), Kct, 0, 128, e->mstream));
    void* bp;
    RC(dalloc(e, (size_t)L.Npad * sizeof(float), &bp));
    L.b = reinterpret_cast<float*>(bp);
    RC(pack_rows(*b, 1, 0, 0, d, L.b, 0, 0, 0, 0, e->mstream));
  }
  RC(pack_conv_pos(e, W, "input_embed.conv_pos_embed.conv1d.", &err));
  // blocks
  e->layers.resize(a.depth);
  std::vector<Block> ada_blocks;
  std::vector<const WView*> ada_bias;
  for (int l = 0; l < a.depth; ++l) {
    Layer& L = e->layers[l];
    const bool dit = a.backbone == F5H_DIT;
    const std::string p = dit ? "transformer_blocks." + std::to_string(l) + "." : "layers." + std::to_string(l) + ".";
    const std::string pa = dit ? p + "attn." : p + "2.";
    const std::string pf = dit ? p + "ff.ff." : p + "4.ff.";
    const WView* wq = W.get(pa + "to_q.weight", (int64_t)inner * d, &err);
    const WView* wk = wq ? W.get(pa + "to_k.weight", (int64_t)inner * d, &err) : nullptr;
    const WView* wv = wk ? W.get(pa + "to_v.weight", (int64_t)inner * d, &err) : nullptr;
    const WView* bq = wv ? W.get(pa + "to_q.bias", inner, &err) : nullptr;
    const WView* bk = bq ? W.get(pa + "to_k.bias", inner, &err) : nullptr;
    const WView* bv = bk ? W.get(pa + "to_v.bias", inner, &err) : nullptr;
    if (!wq || !wk || !wv || !bq || !bk || !bv) return fail(F5H_ENOWEIGHT, err);
    RC(make_lin(e, {Block{wq, inner, d, 0, d, 0}, Block{wk, inner, d, 0, d, 0}, Block{wv, inner, d, 0, d, 0}}, d,
                {bq, bk, bv}, &L.qkv));
    if (a.qk_norm) {  // RMSNorm(dim_head) gains, shared by the layer's heads (modules.py:402-407)
      for (int j = 0; j < 2; ++j) {
        const std::string n = pa + (j ? "k_norm.weight" : "q_norm.weight");
        if (!W.get(n, a.dim_head, &err)) return fail(F5H_EINVAL, "qk_norm: " + err);
        RC(vec_upload(e, W, n, a.dim_head, j ? &L.k_norm_w : &L.q_norm_w, &err));
      }
    }
    RC(lin_simple(e, W, pa + "to_out.0.weight", pa + "to_out.0.bias", d, inner, &L.out, &err));
    RC(lin_simple(e, W, pf + "0.0.weight", pf + "0.0.bias", F, d, &L.ff1, &err));
    RC(lin_simple(e, W, pf + "2.weight", pf + "2.bias", d, F, &L.ff2, &err));
    if (dit) {
      const WView* aw = W.get(p + "attn_norm.linear.weight", (int64_t)6 * d * d, &err);
      const WView* ab = aw ? W.get(p + "attn_norm.linear.bias", 6 * d, &err) : nullptr;
      if (!aw || !ab) return fail(F5H_ENOWEIGHT, err);
      ada_blocks.push_back(Block{aw, 6 * d, d, 0, d, 0});
      ada_bias.push_back(ab);
    } else {
      RC(vec_upload(e, W, p + "1.g", d, &L.g_attn, &err));
      RC(vec_upload(e, W, p + "3.g", d, &L.g_ff, &err));
      if (l >= a.depth / 2) {
        const WView* sw = W.get(p + "0.weight", (int64_t)d * 2 * d, &err);
        if (!sw) return fail(F5H_ENOWEIGHT, err);
        RC(make_lin(e, {Block{sw, d, 2 * d, 0, 2 * d, 0}}, 2 * d, {}, &L.skip));
      }
    }
  }
  if (a.backbone == F5H_DIT) {
    const WView* nw = W.get("norm_out.linear.weight", (int64_t)2 * d * d, &err);
    const WView* nb = nw ? W.get("norm_out.linear.bias", 2 * d, &err) : nullptr;
    if (!nw || !nb) return fail(F5H_ENOWEIGHT, err);
    ada_blocks.push_back(Block{nw, 2 * d, d, 0, d, 0});
    ada_bias.push_back(nb);
    RC(make_lin(e, ada_blocks, d, ada_bias, &e->ada));
    if (a.long_skip_connection) {
      const WView* sw = W.get("long_skip_connection.weight", (int64_t)d * 2 * d, &err);
      if (!sw) return fail(F5H_EINVAL, "long_skip_connection: " + err);
      RC(make_lin(e, {Block{sw, d, 2 * d, 0, 2 * d, 0}}, 2 * d, {}, &e->long_skip));
    }
  } else {
    RC(vec_upload(e, W, "norm_out.g", d, &e->norm_out_g, &err));
  }
  RC(lin_simple(e, W, "proj_out.weight", "proj_out.bias", mel, d, &e->proj_out, &err));
  return 0;
}

static int check_arch(const f5h_arch* a) {
  if (!a) return fail(F5H_EINVAL, "null arch");
  if (a->backbone != F5H_DIT && a->backbone != F5H_UNETT && a->backbone != F5H_MMDIT)
    return fail(F5H_EINVAL, "backbone must be DiT, UNetT or MMDiT");
  if (a->backbone == F5H_MMDIT) {  // mmdit.py:87-133: one width for both streams, no ConvNeXt text blocks, RoPE on all heads
    if (a->text_dim != a->dim) return fail(F5H_EINVAL, "MMDiT: text_dim must equal dim");
    if (a->conv_layers != 0) return fail(F5H_EINVAL, "MMDiT: conv_layers must be 0");
    if (a->pe_attn_head != 0) return fail(F5H_EINVAL, "MMDiT: pe_attn_head must be 0");
    if (a->long_skip_connection != 0) return fail(F5H_EINVAL, "MMDiT: long_skip_connection must be 0");
    if (a->text_average_upsampling != 0) return fail(F5H_EINVAL, "MMDiT: text_average_upsampling must be 0");
    if (a->depth < 1) return fail(F5H_EINVAL, "MMDiT: depth must be >= 1");
  }
  if (a->dim_head != 64) return fail(F5H_EINVAL, "dim_head must be 64");
  if (a->dim % 128 || a->dim <= 0 || a->dim > 1024) return fail(F5H_EINVAL, "dim must be a multiple of 128, <= 1024");
  if (a->heads * 64 != a->dim) return fail(F5H_EINVAL, "heads*dim_head must equal dim");
  if (a->ff_dim % 64 || a->ff_dim <= 0) return fail(F5H_EINVAL, "ff_dim must be a positive multiple of 64");
  if (a->mel_dim != 100) return fail(F5H_EINVAL, "mel_dim must be 100");
  if (a->backbone != F5H_MMDIT && (a->text_dim <= 0 || a->text_dim % 4 || a->text_dim > 512))
    return fail(F5H_EINVAL, "text_dim must be <= 512, % 4");
  if (a->depth <= 0 || (a->backbone == F5H_UNETT && a->depth % 2)) return fail(F5H_EINVAL, "bad depth");
  if (a->backbone == F5H_UNETT && a->conv_layers != 0) return fail(F5H_EINVAL, "UNetT with conv_layers unsupported");
  if (a->compute != F5H_FP32 && a->compute != F5H_BF16 && a->compute != F5H_FP16 && a->compute != F5H_MXFP8)
    return fail(F5H_EINVAL, "compute must be FP32, BF16, FP16 or MXFP8");
  if (a->compute == F5H_MXFP8) {  // the MX8 GEMM's K-step is 128 elements (dim and heads * 64: checked above)
    if (a->backbone != F5H_DIT) return fail(F5H_EINVAL, "compute MXFP8: the backbone must be DiT");
    if (a->ff_dim % 128) return fail(F5H_EINVAL, "compute MXFP8: ff_dim must be a multiple of 128");
  }
  if (a->qk_norm != 0 && a->qk_norm != 1) return fail(F5H_EINVAL, "qk_norm must be 0 (none) or 1 (rms_norm)");
  if ((a->long_skip_connection != 0 && a->long_skip_connection != 1) ||
      (a->text_average_upsampling != 0 && a->text_average_upsampling != 1))
    return fail(F5H_EINVAL, "long_skip_connection and text_average_upsampling must be 0 or 1");
  if (a->backbone != F5H_DIT && (a->long_skip_connection || a->text_average_upsampling))
    return fail(F5H_EINVAL, "long_skip_connection and text_average_upsampling are DiT options");
  if (a->text_average_upsampling && !a->text_mask_padding)
    return fail(F5H_EINVAL, "text_embedding_average_upsampling requires text_mask_padding to be True");
  return 0;
}

// ============================================================================ C ABI
extern "C" {

int f5h_engine_create_views(const f5h_arch* arch, const f5h_tensor_view* weights, int32_t n_weights, int32_t device,
                            f5h_engine** out) {
  if (!out) return fail(F5H_EINVAL, "null out");
  *out = nullptr;
  RC(check_arch(arch));
  if (n_weights < 0 || (n_weights > 0 && !weights)) return fail(F5H_EINVAL, "null weights");
  for (int i = 0; i < n_weights; ++i) {
    const f5h_tensor_view& v = weights[i];
    if (!v.name || (!v.data && v.numel > 0) || v.numel < 0) return fail(F5H_EINVAL, "bad weight view");
    if (v.dtype != F5H_DT_F32 && v.dtype != F5H_DT_BF16 && v.dtype != F5H_DT_F16)
      return fail(F5H_EINVAL, std::string("weight ") + v.name + ": dtype must be F5H_DT_F32, _BF16 or _F16");
    if (v.on_device != 0 && v.on_device != 1)
      return fail(F5H_EINVAL, std::string("weight ") + v.name + ": on_device must be 0 or 1");
  }
  HIPCK(hipSetDevice(device));
  f5h_engine* e = new f5h_engine();
  if (hipStreamCreateWithFlags(&e->mstream, hipStreamNonBlocking) != hipSuccess) {
    delete e;
    return fail(F5H_EHIP, "engine stream");
  }
  e->a = *arch;
  e->dev = device;
  // MXFP8 is the bf16 mode with MX8 operands in the per-layer GEMM classes of mx8_mask (default: all four)
  e->mx8 = arch->compute == F5H_MXFP8 ? 1 : 0;
  e->bf = e->mx8 ? F5H_BF16 : arch->compute;
  e->esz = e->bf ? 2 : 4;
  if (e->mx8) {
    e->mx8_mask = 1 | 4 | 8 | 16;
    if (const char* mv = getenv("F5H_MX8_CLASSES")) e->mx8_mask = atoi(mv) & (1 | 4 | 8 | 16);
  }
  // text columns of the hoisted input projection (none for MMDiT: its text is a stream of its own)
  e->tdp = arch->backbone == F5H_MMDIT ? 0 : (arch->text_dim + 63) / 64 * 64;
  if (const char* gv = getenv("F5H_GRAPH")) e->graph_mode = atoi(gv) ? 1 : 0;
  if (const char* sv = getenv("F5H_SPLIT_CFG")) e->split_cfg = std::min(2, std::max(0, atoi(sv)));
  if (const char* pv = getenv("F5H_NO_PAD_SKIP")) e->pad_skip = (*pv == '1') ? 0 : 1;
  if (const char* cv = getenv("F5H_CHAIN")) e->chain = (*cv == '1') ? 1 : 0;
  // device views are read on the engine's non-blocking stream: order it behind the null stream (so behind
  // every blocking stream's queued work, the ordering the packing had when it ran on the null stream); work
  // on other non-blocking streams must be complete (f5h.h)
  {
    hipEvent_t ev = nullptr;
    if (hipEventCreateWithFlags(&ev, hipEventDisableTiming) == hipSuccess) {
      if (hipEventRecord(ev, nullptr) != hipSuccess || hipStreamWaitEvent(e->mstream, ev, 0) != hipSuccess)
        (void)hipGetLastError();
      (void)hipEventDestroy(ev);
    } else {
      (void)hipGetLastError();
    }
  }
  // host views: staged once, in their own dtype, into temporaries freed after packing
  WMap W;
  std::vector<void*> staged;
  int rc = 0;
  for (int i = 0; i < n_weights && !rc; ++i) {
    const f5h_tensor_view& v = weights[i];
    const size_t bytes = (size_t)v.numel * (v.dtype == F5H_DT_F32 ? 4 : 2);
    const void* dp = v.data;
    if (!v.on_device && bytes) {
      void* t = dev_alloc(device, bytes, e->mstream);
      if (!t) {
        rc = fail(F5H_EHIP, "weight staging allocation");
        break;
      }
      staged.push_back(t);
      if (hipMemcpyAsync(t, v.data, bytes, hipMemcpyHostToDevice, e->mstream) != hipSuccess) {
        rc = fail(F5H_EHIP, std::string("weight staging copy: ") + v.name);
        break;
      }
      dp = t;
    } else if (v.on_device && bytes) {
      hipPointerAttribute_t at{};
      if (hipPointerGetAttributes(&at, v.data) != hipSuccess || at.device != device) {
        (void)hipGetLastError();
        rc = fail(F5H_EINVAL, std::string("weight ") + v.name + ": on_device view is not memory of device " +
                                  std::to_string(device));
        break;
      }
    }
    W.m[v.name] = WView{dp, v.dtype, v.numel};
  }
  if (!rc) rc = pack_all(e, W);
  // LayerNorm fold support and the AdaLN table row length (DiT: the modulation rows, then the fold's u/v per layer)
  if (!rc && arch->backbone == F5H_DIT) {
    e->lnf_ok = e->bf != 0 && arch->dim % 64 == 0 && arch->dim <= 1024 && arch->ff_dim % 64 == 0;
    e->ada_row = e->ada.Npad + (e->lnf_ok ? (int64_t)arch->depth * (2 * (int64_t)arch->ff_dim + 6 * (int64_t)arch->dim) : 0);
    if (e->lnf_ok) {
      std::vector<const void*> wp;
      for (const Layer& L : e->layers) wp.push_back(L.ff1.w);
      for (const Layer& L : e->layers) wp.push_back(L.qkv.w);
      if (upload(e, wp, &e->lnf_w)) e->lnf_ok = false;
    }
  }
  // MXFP8: every layer's four GEMM weights quantised on the device from the packed bf16 copy, which stays (a class
  // outside the mask runs on it), and the device word the MX8 launches count themselves in
  if (!rc && e->mx8) {
    for (Layer& L : e->layers) {
      for (Lin* W : {&L.qkv, &L.out, &L.ff1, &L.ff2}) {
        void *q8 = nullptr, *s8 = nullptr;
        if (W->K % 128 || dalloc(e, (size_t)W->N * W->K, &q8) || dalloc(e, (size_t)W->N * (W->K / 32), &s8) ||
            quant_rows_mx8(W->w, W->N, W->K, (uint8_t*)q8, (uint8_t*)s8, e->mstream) != hipSuccess) {
          rc = fail(F5H_EHIP, "MXFP8 weight quantisation");
          break;
        }
        W->w8 = (uint8_t*)q8;
        W->ws = (uint8_t*)s8;
      }
      if (rc) break;
    }
    void* cw = nullptr;
    if (!rc && dalloc(e, 64, &cw)) rc = fail(F5H_EHIP, "MXFP8 launch counter");  // (zeroed)
    e->mx8_count = reinterpret_cast<unsigned long long*>(cw);
  }
  if (!rc && arch->backbone == F5H_MMDIT) e->ada_row = e->ada.Npad;  // no fold: the modulation rows only
  // RMSNorm fold support (UNetT, 16-bit): every layer's QKV and FFN1 weights with their norm's gain folded in
  if (!rc && arch->backbone == F5H_UNETT && e->bf != 0 && arch->dim % 64 == 0 && arch->dim <= 1024) {
    e->rmsf_ok = true;
    for (Layer& L : e->layers) {
      L.qkv_g = L.qkv;
      L.ff1_g = L.ff1;
      if (dalloc(e, (size_t)L.qkv.Npad * L.qkv.K * e->esz, &L.qkv_g.w) ||
          dalloc(e, (size_t)L.ff1.Npad * L.ff1.K * e->esz, &L.ff1_g.w) ||
          scale_cols(e->bf, L.qkv.w, L.qkv.Npad, L.qkv.K, L.g_attn, L.qkv_g.w, e->mstream) != hipSuccess ||
          scale_cols(e->bf, L.ff1.w, L.ff1.Npad, L.ff1.K, L.g_ff, L.ff1_g.w, e->mstream) != hipSuccess) {
        e->rmsf_ok = false;
        break;
      }
    }
  }
  // default: on for DiT (C2 -2 %, profiles/r06_ab_fold_c2.txt), off for UNetT (its RMSNorm fold measured within noise
  // at C5, profiles/r06_ab_rmsfold_c5.txt); F5H_LNFOLD=0/1 or f5h_set_ln_fold overrides
  e->lnfold = arch->backbone == F5H_DIT ? 1 : 0;
  if (const char* lv = getenv("F5H_LNFOLD")) e->lnfold = (*lv == '0') ? 0 : 1;
  // packing ran on the engine's stream (no device-wide synchronisation)
  if (!rc && hipStreamSynchronize(e->mstream) != hipSuccess) rc = fail(F5H_EHIP, "weight packing");
  for (void* t : staged) dev_free(t, e->mstream);
  if (rc) {
    f5h_engine_destroy(e);
    return rc;
  }
  {
    void* p = nullptr;
    int khz = 0;
    void* tl = nullptr;
    if (dalloc(e, kProbeBytes, &p) || dalloc(e, (size_t)kTimelineWG * 4 * sizeof(unsigned long long), &tl) ||
        hipStreamSynchronize(e->mstream) != hipSuccess) {
      f5h_engine_destroy(e);
      return fail(F5H_EHIP, "probe buffers");
    }
    void* fw = nullptr;
    if (dalloc(e, 64, &fw) || hipStreamSynchronize(e->mstream) != hipSuccess) {
      f5h_engine_destroy(e);
      return fail(F5H_EHIP, "chain fault word");
    }
    e->chain_fault = reinterpret_cast<unsigned*>(fw);
    e->fault_slot = fault_slot_take(&e->fault_host);
    if (e->fault_slot < 0) {  // no pinned word: the chain stays off (its give-ups could not be reported)
      (void)hipGetLastError();
      e->chain_fault = nullptr;
    }
    e->pstamp = reinterpret_cast<unsigned long long*>(p);
    e->pslots = e->pstamp + 64;
    e->ptick = reinterpret_cast<int*>(e->pstamp);
    e->ptl = reinterpret_cast<unsigned long long*>(tl);
    if (hipDeviceGetAttribute(&khz, hipDeviceAttributeWallClockRate, device) == hipSuccess) e->wall_khz = khz;
  }
  *out = e;
  return 0;
}

int f5h_engine_create(const f5h_arch* arch, const f5h_weight* weights, int32_t n_weights, int32_t device,
                      f5h_engine** out) {
  if (n_weights < 0 || (n_weights > 0 && !weights)) return fail(F5H_EINVAL, "null weights");
  std::vector<f5h_tensor_view> v((size_t)n_weights);
  for (int i = 0; i < n_weights; ++i)
    v[i] = f5h_tensor_view{weights[i].name, weights[i].data, F5H_DT_F32, 0, weights[i].numel};
  return f5h_engine_create_views(arch, v.data(), n_weights, device, out);
}

// Returns at once: the release runs on the reaper thread (reaper.h), which waits only for this engine's
// own work -- the last-use event of every stream its calls ran on and the events recorded after its graph
// replays -- and then destroys the graphs and frees the device memory. No device-wide synchronisation, so
// dropping an engine never waits for unrelated streams (the reference's ThreadPoolExecutor may be
// sampling with other models meanwhile).
void f5h_engine_destroy(f5h_engine* e) {
  if (!e) return;
  retire(e->dev, [e] {
    for (hipEvent_t ev : e->uses.take()) {
      (void)hipEventSynchronize(ev);
      (void)hipEventDestroy(ev);
    }
    {
      std::lock_guard<std::mutex> g(e->gm);
      for (auto* v : {&e->graphs, &e->graveyard})
        for (auto& x : *v)
          for (hipEvent_t ev : x->inflight) (void)hipEventSynchronize(ev);
    }
    e->graphs.clear();
    e->graveyard.clear();
    for (hipEvent_t ev : e->ev_pool) (void)hipEventDestroy(ev);
    e->ev_pool.clear();
    if (e->cap) (void)hipStreamDestroy(e->cap);
    if (e->cap2) (void)hipStreamDestroy(e->cap2);
    if (e->ev_fork) (void)hipEventDestroy(e->ev_fork);
    if (e->ev_join) (void)hipEventDestroy(e->ev_join);
    // stream-ordered releases into the pool: no device-wide wait (hipFree would wait for every stream)
    for (void* p : e->allocs) dev_free(p, e->mstream);
    if (e->mstream) (void)hipStreamDestroy(e->mstream);
    fault_slot_give(e->fault_slot);  // after the use events: the last fault copy has landed
    delete e;
  });
}

}  // extern "C"
