// f5h engine: weight packing, workspace layout and the CFM.sample orchestration behind the
// C ABI declared in include/f5h.h. Host code; every kernel is enqueued on the caller's stream.
//
// Hot-path map (reference file:line -> what runs here):
//   cfm.py:211-216  t grid            -> host (caller), passed as t_grid
//   modules.py:852-862, 321-323, 342-344  time MLP + every AdaLN row for every step
//                                     -> three GEMMs before the loop (one table [nfe, depth*6d+2d])
//   dit.py:86-139 text embed (cached) -> text_embed + ConvNeXt kernels once per call (both branches)
//   dit.py:159-162 InputEmbedding.proj -> split: cond/text part hoisted (P), x part per step
//   modules.py:175-201 ConvPositionEmbedding -> conv_pos x2 (implicit-GEMM MFMA)
//   modules.py:743-757 DiTBlock x depth -> ln_modulate, QKV+RoPE GEMM, attention, out GEMM+gate,
//                                     ln_modulate, FFN1+GELU GEMM, FFN2 GEMM+gate
//   dit.py:367-368, cfm.py:190-191, torchdiffeq euler -> ln_modulate, proj_out GEMM, cfg_euler
//   cfm.py:223 final where            -> final_where
#include "engine_internal.h"

// AdaLN backbones (a per-step modulation table, L = N rows per sequence): DiT and MMDiT
static bool adaln_bb(const f5h_arch& a) { return a.backbone != F5H_UNETT; }
// MMDiT AdaLN table row: per block the audio stream's 6d (attn_norm_x) then the text stream's 6d (attn_norm_c; 2d
// (scale, shift) in the last block, AdaLayerNorm_Final), then norm_out's 2d
static size_t mm_ada_x(const f5h_arch& a, int l) { return (size_t)l * 12 * a.dim; }
static size_t mm_ada_c(const f5h_arch& a, int l) { return mm_ada_x(a, l) + (size_t)6 * a.dim; }
static size_t mm_ada_fin(const f5h_arch& a) { return mm_ada_c(a, a.depth - 1) + (size_t)2 * a.dim; }

// ---------------------------------------------------------------- workspace layout
// nfe: table rows. method / steps: the multi-stage solvers' extra buffers (none for Euler, whose layout is unchanged)
// nt: text tokens (MMDiT only: its text stream's buffers; the other backbones' layouts do not depend on it)
// rgB / rgL (ragged sampling: utterances and the longest one; the call then passes B = 1 and N = R, the packed rows of
// one CFG branch): every [S*N, .] buffer holds the 2R packed rows; q / k / v are padded panels [2 rgB, heads, rgL, 64]
static void layout(const f5h_engine* e, WS& ws, Bufs& b, int B, int N, int nfe, int use_cfg, int method = 0,
                   int steps = 0, int nt = 0, int rgB = 0, int rgL = 0) {
  const f5h_arch& a = e->a;
  const int d = a.dim, td = a.text_dim, S = use_cfg ? 2 * B : B;
  const bool mm = a.backbone == F5H_MMDIT;
  const int L = adaln_bb(a) ? N : N + 1;
  const size_t rows = (size_t)S * L, es = e->esz;
  const size_t jrows = mm ? (size_t)S * (N + nt) : rows;  // rows of the q / k / v buffers (MMDiT: the joint sequence)
  const int inner = a.heads * 64;
  b.tsin = ws.take<float>((size_t)nfe * 256);
  b.th = ws.take<float>((size_t)nfe * d);
  b.temb = ws.take<float>((size_t)nfe * d);
  b.tin_op = ws.take<char>((size_t)nfe * std::max(256, d) * es);
  b.ada = adaln_bb(a) ? ws.take<float>((size_t)nfe * e->ada_row) : nullptr;
  b.te = ws.take<float>((size_t)2 * B * (mm ? nt : N) * td);  // (MMDiT: [2][B][nt][d], not padded to the audio length)
  b.keepfill = ws.take<uint8_t>((size_t)2 * B * N);
  if (a.conv_layers > 0) {
    b.dwln = ws.take<char>((size_t)2 * B * N * td * es);
    b.pw1o = ws.take<float>((size_t)2 * B * N * 2 * td);
    b.grno = ws.take<char>((size_t)2 * B * N * 2 * td * es);
    b.grn_scr = rgB ? ws.take<float>((size_t)((rgL + 63) / 64 + 1) * 2 * rgB * 2 * td)
                    : ws.take<float>((size_t)((N + 63) / 64 + 1) * 2 * B * 2 * td);
  } else {
    b.dwln = b.grno = nullptr;
    b.pw1o = b.grn_scr = nullptr;
  }
  b.act = ws.take<char>((size_t)S * N * (128 + e->tdp) * es);
  b.P = ws.take<float>((size_t)S * N * d);
  b.ypad = ws.take<char>((size_t)B * N * 128 * es);
  b.h0 = ws.take<float>((size_t)S * N * d);
  b.c1 = ws.take<char>((size_t)S * N * d * es);
  b.h = adaln_bb(a) ? ws.take<float>(rows * d) : nullptr;  // DiT / MMDiT (audio) residual stream
  b.aop = ws.take<char>(rows * d * es);
  const size_t qrows = rgB ? (size_t)(use_cfg ? 2 : 1) * rgB * rgL : jrows;
  b.q = ws.take<char>(qrows * inner * es);
  b.k = ws.take<char>(qrows * inner * es);
  b.v = ws.take<char>(qrows * inner * es);
  b.o = ws.take<char>(rows * inner * es);
  b.f = ws.take<char>(rows * a.ff_dim * es);
  b.p = ws.take<float>(rows * e->proj_out.Npad);  // proj_out rows padded to the GEMM tile width
  b.rope = ws.take<float2>((size_t)(mm ? std::max(N, nt) : L) * 32);  // (MMDiT: both streams count from 0)
  b.rowkeep = ws.take<uint8_t>(rows);
  b.kvlen = ws.take<int32_t>(S);
  b.chain_g4 = ((int)((rows + kChainRows - 1) / kChainRows) + 3) / 4 * 4;
  b.chain = a.backbone == F5H_DIT ? ws.take<unsigned>((size_t)a.depth * 5 * b.chain_g4) : nullptr;
  b.ada_cur = adaln_bb(a) ? ws.take<float>((size_t)e->ada_row) : nullptr;
  // LayerNorm fold: per row and 64-column strip of the residual stream, (mean, M2) (float2)
  b.lnp = (e->lnf_ok || e->rmsf_ok) ? ws.take<float>(rows * (size_t)(d / 64) * 2) : nullptr;
  b.temb_cur = ws.take<float>((size_t)d);
  b.tgrid = ws.take<float>((size_t)nfe);
  b.kstep = ws.take<int>(64);
  b.y = ws.take<float>((size_t)B * N * e->a.mel_dim);
  b.trajp = ws.take<float*>(8);
  b.in_cond = ws.take<float>((size_t)B * N * a.mel_dim);
  b.in_mask = ws.take<uint8_t>((size_t)B * N);
  b.in_text = ws.take<int64_t>((size_t)B * (mm ? std::max(N, nt) : N));
  b.in_dur = ws.take<int32_t>((size_t)B);
  b.xs.clear();
  b.pp[0] = b.pp[1] = nullptr;
  if (a.backbone == F5H_UNETT) {
    for (int i = 0; i <= a.depth / 2; ++i) b.xs.push_back(ws.take<char>(rows * d * es));
    b.pp[0] = ws.take<char>(rows * d * es);
    b.pp[1] = ws.take<char>(rows * d * es);
  }
  b.sgrid = method ? ws.take<float>((size_t)steps + 1) : nullptr;
  const int kept = ode_kept_slopes(method);
  b.kbuf = kept ? ws.take<float>((size_t)kept * B * N * a.mel_dim) : nullptr;
  // the options' buffers come last, so every other buffer sits where it does without them
  b.hkeep = a.long_skip_connection ? ws.take<char>(rows * d * es) : nullptr;
  b.te_up = a.text_average_upsampling ? ws.take<float>((size_t)2 * B * N * td) : nullptr;
  // MMDiT text stream [S, nt, .]: the call-constant embedding c0 in the residual dtype (both branches; the fp32 mode
  // reads b.te itself), the stream, its norm / attention / FFN operands and the c_mask bytes
  const size_t crows = (size_t)S * nt, hsz = e->bf ? es : sizeof(float);
  b.c0 = (mm && e->bf) ? ws.take<char>((size_t)2 * B * nt * d * es) : nullptr;
  b.ch = mm ? ws.take<char>(crows * d * hsz) : nullptr;
  b.caop = mm ? ws.take<char>(crows * d * es) : nullptr;
  b.co = mm ? ws.take<char>(crows * inner * es) : nullptr;
  b.cf = mm ? ws.take<char>(crows * a.ff_dim * es) : nullptr;
  b.ckeep = mm ? ws.take<uint8_t>(crows) : nullptr;
  b.tlen = mm ? ws.take<int32_t>(S) : nullptr;
  b.rowkeep_n = a.backbone != F5H_UNETT ? nullptr : a.conv_layers > 0 ? ws.take<uint8_t>((size_t)S * N) : b.keepfill;
  b.rg_off = rgB ? ws.take<int32_t>((size_t)2 * rgB + 1) : nullptr;
  b.rg_len = rgB ? ws.take<int32_t>((size_t)2 * rgB) : nullptr;
  b.rg_tab = rgB ? ws.take<int2>((size_t)2 * N) : nullptr;
  // F5H_MXFP8 only, and last, so that every other buffer sits where the bf16 mode has it: the MX8 launches' activation
  // operand (elements, then scales), a row of max K = max(dim, ff_dim) bytes per stream row (heads * 64 == dim)
  const size_t kmax = (size_t)std::max(d, a.ff_dim);
  b.a8 = e->mx8 ? ws.take<uint8_t>(rows * kmax) : nullptr;
  b.a8s = e->mx8 ? ws.take<uint8_t>(rows * (kmax / 32)) : nullptr;
}

// ---------------------------------------------------------------- probe
// Store policy: the class bits of f5h_set_store_policy's per-class form, and the classes the auto rule stores
// write-through (what the per-class A/B at C2 kept, profiles/r07_ab_store_policy_c2.txt)
static constexpr int kStoreBit(int kclass) {
  return kclass == KC_QKV ? 1 : kclass == KC_ATTN ? 2 : kclass == KC_OUT ? 4 : kclass == KC_FFN1 ? 8 : kclass == KC_FFN2 ? 16 : 0;
}
static constexpr int kStoreAutoMask = 1 | 2 | 4 | 8 | 16;
// what a class asks of gemm_store_wt / attention_store_wt under an engine policy
static int store_want(int policy, int kclass) {
  if (policy == 0 || policy == 1) return policy;
  if (policy >= 0x100) return (policy & kStoreBit(kclass)) ? 1 : 0;
  return (kStoreAutoMask & kStoreBit(kclass)) ? -1 : 0;
}
// store policy of a hot launch (its final arguments): write-through or plain stores, counted
static void count_store(f5h_engine* e, int wt) {
  (wt ? e->n_store_wt : e->n_store_plain).fetch_add(1, std::memory_order_relaxed);
}
static void gemm_policy(const Ctx& c, GemmArgs& g, int epi, int kclass) {
  g.store_wt = gemm_store_wt(c.e->bf, epi, g, store_want(c.store, kclass));
  count_store(c.e, g.store_wt);
}
// Times one launch site when its kernel class is probed (kc < 0: a site that is never timed). With `kp` the kernel
// stamps itself (GemmArgs/AttnArgs::probe); without, stamp kernels bracket the launch.
struct ProbeScope {
  f5h_engine* e;
  hipStream_t st;
  bool on;
  bool self = false;
  unsigned long long* slots = nullptr;
  ProbeScope(Ctx& c, int kc, hipStream_t s, DevProbe* kp = nullptr)
      : e(c.e), st(s), on(kc >= 0 && c.m.probe_class == kc && c.e->pslots && c.site < kProbeSites) {
    if (!on) return;
    const int s0 = c.site++;
    slots = e->pslots + (size_t)s0 * kProbeRow;
    if (kp) {
      self = true;
      kp->slots = slots;
      kp->tick = e->ptick;
      kp->tl = s0 == 0 ? e->ptl : nullptr;  // the class's first launch site of a step, tick 0
    } else {
      (void)stamp_begin(slots, e->ptick, st);
    }
  }
  ~ProbeScope() {
    if (on && !self) (void)stamp_end(slots, e->ptick, st);
  }
};

// ---------------------------------------------------------------- forward pieces
static GemmArgs gargs(const void* A, int64_t lda, const Lin& W, int M, void* C, int64_t ldc) {
  GemmArgs g{};
  g.A = A;
  g.lda = (int)lda;
  g.W = W.w;
  g.ldw = W.K;
  g.M = M;
  g.N = W.N;
  g.K = W.K;
  g.bias = W.b;
  g.C = C;
  g.ldc = ldc;
  return g;
}

// Everything that depends only on the call's inputs (not on y): time/AdaLN tables, text
// embedding, hoisted input projection, masks, rope table.
static int prologue(Ctx& c, const float* t_host, int nt_vals, const float* cond, const uint8_t* cond_mask,
                    const int64_t* text, const int32_t* duration, bool text_cached = false) {
  f5h_engine* e = c.e;
  const f5h_arch& a = e->a;
  const int d = a.dim, td = a.text_dim, bf = e->bf;
  Bufs& b = c.b;
  hipStream_t st = c.st;
  const bool mm = a.backbone == F5H_MMDIT;
  KCK(rope_table(c.rag_B ? c.rag_L : mm ? std::max(c.N, c.nt) : c.L, b.rope, st));
  if (c.rag_B) KCK(build_rowtab(b.rg_off, 2 * c.rag_B, 2 * c.N, b.rg_tab, b.rg_len, st));
  if (mm) KCK(build_textkeep(text, c.B, c.S, c.nt, b.ckeep, st));  // c_mask (mmdit.py:232), both branches
  const int off = adaln_bb(a) ? 0 : 1;
  if (c.batch_mask) {
    KCK(build_rowkeep(duration, c.B, c.S, c.L, off, b.rowkeep, st));
    KCK(build_kvlen(duration, c.B, c.S, off, b.kvlen, st));
    // MMDiT isolated: the text keys' range, from the text as given (before drop_text, as c_mask)
    if (mm && c.isolate) KCK(build_textlen(text, c.B, c.S, c.nt, b.tlen, st));
  }
  // ---- time embedding for every grid point used, then the AdaLN table
  {
    if (t_host)
      KCK(time_sinus(t_host, nt_vals, b.tsin, st));
    else
      KCK(time_sinus_dev(b.tgrid, nt_vals, b.tsin, st));  // prologue graph: grid uploaded beforehand
    KCK(f32_to_op(bf, b.tsin, (int64_t)nt_vals * 256, b.tin_op, st));
    GemmArgs g = gargs(b.tin_op, 256, e->t1, nt_vals, b.th, d);
    KCK(gemm(bf, EPI_SILU, g, st));
    KCK(f32_to_op(bf, b.th, (int64_t)nt_vals * d, b.tin_op, st));
    g = gargs(b.tin_op, d, e->t2, nt_vals, b.temb, d);
    KCK(gemm(bf, EPI_STORE, g, st));
    if (adaln_bb(a)) {
      KCK(silu_to_op(bf, b.temb, b.tin_op, (int64_t)nt_vals * d, st));
      g = gargs(b.tin_op, d, e->ada, nt_vals, b.ada, e->ada_row);
      KCK(gemm(bf, EPI_STORE, g, st));
      if (c.m.lnfold) {  // every step's u / v of the folded LayerNorms (kernels.h LnFoldArgs)
        LnFoldArgs la{};
        la.table = b.ada;
        la.stride = e->ada_row;
        la.out_off = e->ada.Npad;
        la.nfe = nt_vals;
        la.depth = a.depth;
        la.d = d;
        la.F = a.ff_dim;
        la.w1 = e->lnf_w;
        la.wqkv = e->lnf_w + a.depth;
        KCK(lnfold_uv(bf, la, st));
      }
    }
  }
  // ---- text embedding, both branches (cached once per call in the reference, dit.py:294-310);
  // text_cached: the plugin's kept embedding is already in the workspace (f5h_forward text_cache 2)
  if (!text_cached && mm) {
    // mmdit.py:32-63: Embedding(text + 1) [nt, dim] + freqs_cis[min(j, 1023)], filler rows (taken before drop_text)
    // zeroed; no ConvNeXt blocks, not padded to the audio length. Both branches, then once into the residual dtype
    TextEmbArgs t{};
    t.text = text;
    t.B = c.B;
    t.nt = c.nt;
    t.N = c.nt;
    t.td = d;
    t.table = e->text_table;
    t.freqs = e->freqs;
    t.freq_rows = kMMTextPos;
    t.mask_padding = a.text_mask_padding;
    t.out_c = b.te;
    t.out_u = b.te + (size_t)c.B * c.nt * d;
    KCK(text_embed(t, st));
    if (bf) KCK(f32_to_op(bf, b.te, (int64_t)2 * c.B * c.nt * d, b.c0, st));
  } else if (!text_cached) {
    TextEmbArgs t{};
    t.text = text;
    t.B = c.rag_B ? c.rag_B : c.B;
    t.nt = c.nt;
    t.N = c.N;
    t.td = td;
    t.seg_off = b.rg_off;  // ragged: utterance b's tokens, then filler, on its own packed rows (null otherwise)
    t.seq_len = (a.backbone == F5H_DIT && c.batch_mask) ? duration : nullptr;
    t.table = e->text_table;
    t.freqs = a.conv_layers > 0 ? e->freqs : nullptr;
    t.mask_padding = a.text_mask_padding;
    t.out_c = b.te;
    t.out_u = b.te + (size_t)c.B * c.N * td;
    t.keep = b.keepfill;
    KCK(text_embed(t, st));
    const int S2 = 2 * c.B, R2 = S2 * c.N;
    // isolation: the depthwise conv's taps and GRN's norm over time stop at the sequence's own length (the reference
    // runs both over the padded axis, modules.py:236-245, 260-264)
    const int32_t* tl = c.isolate ? duration : nullptr;
    for (int i = 0; i < a.conv_layers; ++i) {
      CNX& x = e->cnx[i];
      if (c.rag_B)  // the 2 rag_B sequences of both branches on the 2R packed rows
        KCK(dwconv_ln_ragged(bf, b.te, b.rg_off, 2 * c.rag_B, R2, td, x.dw_w, x.dw_b, x.ln_w, x.ln_b, b.dwln, st));
      else
        KCK(dwconv_ln(bf, b.te, S2, c.N, td, x.dw_w, x.dw_b, x.ln_w, x.ln_b, b.dwln, st, tl, c.B));
      GemmArgs g = gargs(b.dwln, td, x.pw1, R2, b.pw1o, 2 * td);
      KCK(gemm(bf, EPI_GELU_ERF, g, st));
      if (c.rag_B)
        KCK(grn_ragged(bf, b.pw1o, b.rg_off, 2 * c.rag_B, R2, c.rag_L, 2 * td, x.gamma, x.beta, b.grn_scr, b.grno, st));
      else
        KCK(grn(bf, b.pw1o, S2, c.N, 2 * td, x.gamma, x.beta, b.grn_scr, b.grno, st, tl, c.B));
      g = gargs(b.grno, 2 * td, x.pw2, R2, b.te, td);
      g.rowkeep = a.text_mask_padding ? b.keepfill : nullptr;
      KCK(gemm(bf, EPI_RESID_FILL, g, st));
    }
    // text_embedding_average_upsampling (dit.py:55-84, 131-137): both branches, by the mask taken before drop_text
    if (a.text_average_upsampling) {
      TextUpArgs u{};
      u.text = text;
      u.B = c.B;
      u.nt = c.nt;
      u.N = c.N;
      u.td = td;
      u.seq_len = t.seq_len;
      u.in_c = t.out_c;
      u.in_u = t.out_u;
      u.out_c = b.te_up;
      u.out_u = b.te_up + (size_t)c.B * c.N * td;
      KCK(text_upsample(u, st));
    }
  }
  // UNetT isolated: the audio rows' mask (after the text embedding, whose keepfill bytes it may take over)
  if (c.isolate && b.rowkeep_n) KCK(build_rowkeep(duration, c.B, c.S, c.N, 0, b.rowkeep_n, st));
  // ---- hoisted input projection: P = [step_cond | text] . W_ct^T + b
  const float* te = a.text_average_upsampling ? b.te_up : b.te;
  // (MMDiT: no text columns, the audio embedding sees cat(x, cond) only)
  KCK(build_ct(bf, cond, cond_mask, te, te + (size_t)c.B * c.N * td, c.B, c.N, mm ? 0 : td, c.S, c.drop_audio,
               c.drop_text, b.act, st));
  GemmArgs g = gargs(b.act, 128 + e->tdp, e->in_ct, c.S * c.N, b.P, d);
  KCK(gemm(bf, EPI_STORE, g, st));
  return 0;
}

// kstep buffer (64 ints): [0] the step index, [kArrive] the Euler launch's arrival counter
constexpr int kArrive = 16;

// Copy the step's table row (k = *kstep) to the fixed per-step buffer the layers read.
static int step_prep(Ctx& c) {
  f5h_engine* e = c.e;
  if (adaln_bb(e->a))
    KCK(step_begin(c.b.kstep, c.b.ada, e->ada_row, e->ada_row, c.b.ada_cur, c.st));
  else
    KCK(step_begin(c.b.kstep, c.b.temb, e->a.dim, e->a.dim, c.b.temb_cur, c.st));
  return 0;
}

// ---------------------------------------------------------------- layer-op launchers
// Each is the one place for its launch; the backbones differ in the arguments they hand in.

// A part's MX8 activation operand (F5H_MXFP8 engines: elements and scales; null otherwise)
struct Mx8Act {
  uint8_t *a8 = nullptr, *a8s = nullptr;
};

// A per-layer GEMM of class kclass (QKV, out-projection, FFN1, FFN2). With the class's bit in mx it runs on MX8
// operands: A from act (quantised here from g.A when quant_a: the out-projection and FFN2, whose A no norm launch
// writes), W's MX8 copy, plain stores only. Otherwise the 16-bit / fp32 launch under the call's store policy.
static int layer_gemm(Ctx& c, hipStream_t st, int kclass, int epi, GemmArgs& g, const Lin& W, int mx = 0,
                      const Mx8Act& act = {}, bool quant_a = false) {
  f5h_engine* e = c.e;
  if (mx & kStoreBit(kclass)) {
    // (rows of A the attention's pad-row skip left unwritten quantise to whatever they hold: they feed pad rows of the
    // product only, which keep their residual)
    if (quant_a) KCK(quant_rows_mx8(g.A, g.M, g.K, act.a8, act.a8s, st));
    count_store(e, 0);
    ProbeScope ps(c, kclass, st, &g.probe);
    KCK(gemm_mx8(epi, g, Mx8Ops{act.a8, act.a8s, W.w8, W.ws, e->mx8_count}, st));
  } else {
    gemm_policy(c, g, epi, kclass);
    ProbeScope ps(c, kclass, st, &g.probe);
    KCK(gemm(e->bf, epi, g, st));
  }
  return 0;
}

// The QKV + RoPE GEMM's arguments: A [M, d] into the q / k / v panels, sequences of seq_len rows
static GemmArgs qkv_gargs(const Ctx& c, const void* A, const Lin& W, int M, int seq_len, void* q, void* k, void* v,
                          const float* q_norm_w, const float* k_norm_w) {
  const f5h_arch& a = c.e->a;
  GemmArgs g = gargs(A, a.dim, W, M, nullptr, 0);
  g.rope = c.b.rope;
  g.seq_len = seq_len;
  g.heads = a.heads;
  g.rope_heads = a.heads;
  g.q = q;
  g.k = k;
  g.v = v;
  g.q_scale = 0.125f * 1.4426950408889634f;  // softmax scale 1/sqrt(64) in log2 units, folded into q
  g.q_norm_w = q_norm_w;  // qk_norm (null without it): RMSNorm of every q / k head ahead of RoPE
  g.k_norm_w = k_norm_w;
  g.qk_norm_eps = 1e-6f;  // modules.py:406-407
  return g;
}

// Attention over S sequences of L rows. The caller has set what differs between the backbones (kv_len / q_len, the
// ragged fields, o_split / o2, the second key range).
static int launch_attention(Ctx& c, hipStream_t st, AttnArgs& at, void* q, void* k, void* v, void* o, int S, int L) {
  at.q = q;
  at.k = k;
  at.v = v;
  at.o = o;
  at.S = S;
  at.H = c.e->a.heads;
  at.L = L;
  at.prescaled = 1;
  at.store_wt = attention_store_wt(c.e->bf, at, store_want(c.store, KC_ATTN));
  count_store(c.e, at.store_wt);
  ProbeScope ps(c, KC_ATTN, st, &at.probe);
  KCK(attention(c.e->bf, at, st));
  return 0;
}

// Input embedding of ns sequences from row `no` of the N-row buffers: h0 = y.Wx^T + P, then conv_pos_embed(h0) + h0
// (two conv_pos launches; rowkeep: their row mask or null) into dst, sequence s at row s * dst_seq_stride + dst_row_off.
// Sequence s reads y[s % B]; a part holding both branches computes y.Wx^T once and adds both branches' hoisted P rows.
static int input_embed(Ctx& c, hipStream_t st, int ns, size_t no, const uint8_t* rowkeep, void* dst, int dst_seq_stride,
                       int dst_row_off) {
  f5h_engine* e = c.e;
  Bufs& b = c.b;
  const int d = e->a.dim, bf = e->bf, BN = c.B * c.N;
  void* c1 = (char*)b.c1 + no * d * e->esz;
  GemmArgs g = gargs(b.ypad, 128, e->in_x, BN, b.h0 + no * d, d);
  g.bias = nullptr;
  g.add = b.P + no * d;
  g.ld_add = d;
  g.dual_rows = ns == 2 * c.B ? BN : 0;
  KCK(gemm(bf, EPI_INPROJ, g, st));
  ConvArgs cv{};
  cv.S = ns;
  cv.L = c.N;
  cv.d = d;
  cv.rowkeep = rowkeep;
  cv.x = b.h0 + no * d;
  cv.x_f32 = 1;
  cv.w = e->conv_w[0];
  cv.bias = e->conv_b[0];
  cv.mode = 0;
  cv.y = c1;
  if (c.rag_B) {  // packed rows: the part's sequences by the segment table (always the whole packed batch, no == 0)
    cv.ragged = 1;
    cv.S = ns * c.rag_B;
    cv.L = c.rag_L;
    cv.rowkeep = reinterpret_cast<const uint8_t*>(b.rg_off);
  }
  {
    ProbeScope ps(c, KC_CONV, st);
    KCK(conv_pos(bf, cv, st));
  }
  cv.x = c1;
  cv.x_f32 = bf ? 0 : 1;
  cv.w = e->conv_w[1];
  cv.bias = e->conv_b[1];
  cv.mode = c.m.r16 ? 2 : 1;
  cv.y = dst;
  cv.y_seq_stride = dst_seq_stride;
  cv.y_row_off = dst_row_off;
  cv.resid = b.h0 + no * d;
  KCK(conv_pos(bf, cv, st));
  return 0;
}

// LayerNorm + AdaLN modulation in front of a consumer, into the operand that consumer reads: aop, or the MX8 operand
// when act is given. probed: timed as KC_NORM (the FFN-norm sites; the attention-norm sites never were)
static int adaln_norm(Ctx& c, hipStream_t st, bool probed, const void* h, int rows, const float* shift,
                      const float* scale, void* aop, const Mx8Act* act = nullptr) {
  const int d = c.e->a.dim;
  ProbeScope ps(c, probed ? KC_NORM : -1, st);
  KCK(act ? ln_modulate_mx8(h, c.m.r16, rows, d, shift, scale, act->a8, act->a8s, st)
          : ln_modulate(c.e->bf, h, c.m.r16, rows, d, shift, scale, aop, st));
  return 0;
}
// UNetT's RMSNorm with gain in front of a consumer, probed as adaln_norm
static int rms_norm(Ctx& c, hipStream_t st, bool probed, const void* h, int rows, const float* gain, void* aop) {
  ProbeScope ps(c, probed ? KC_NORM : -1, st);
  KCK(rms_norm_g(c.e->bf, h, c.m.r16, rows, c.e->a.dim, gain, aop, st));
  return 0;
}

// The tail: proj_out over the normed rows of aop into b.p from row ro. All Npad (128) columns: the padded weight rows
// and bias are zero, and whole-column tiles take the fast epilogue; readers use the first mel_dim columns of each row
static int proj_out_tail(Ctx& c, hipStream_t st, const void* aop, int rows, size_t ro) {
  f5h_engine* e = c.e;
  const int pld = e->proj_out.Npad;
  GemmArgs g = gargs(aop, e->a.dim, e->proj_out, rows, c.b.p + ro * pld, pld);
  g.N = pld;
  KCK(gemm(e->bf, EPI_STORE, g, st));
  return 0;
}

// ---------------------------------------------------------------- DiT / UNetT
// One part of a step: sequences [s0, s0 + ns) of the packed batch on stream st, with the part's rows of the buffers
// the layers share, and the call's modes narrowed to the part
struct Part {
  Ctx& c;
  hipStream_t st;
  int s0, ns, rows;
  size_t ro;   // first row of the part (L rows per sequence)
  size_t hsz;  // element size of the residual stream
  void *aop, *q, *k, *v, *o, *f;
  const uint8_t* keep;  // the part's rows of the batch mask, or null
  Mx8Act act;           // F5H_MXFP8: the activation operand of this part's MX8 launches
  float* lnp;           // the folds' statistics of the part's rows
  const float* ada_k;   // DiT: the step's AdaLN table row
  // chain_on: StepModes::chain_eligible on the whole packed batch. (s0 == 0 only: two chain launches on the two CFG
  // streams run 72 instead of 49 ms at C2, their waiting workgroups holding the slots the other stream's producers
  // need, profiles/r05_ab_c2_prio_split.txt; for the same reason the call does not chain while another stream's chained
  // call is in flight, chain_admit)
  bool chain_on, fold_on, rms_on;
  void* res(void* base) const { return (char*)base + ro * c.e->a.dim * hsz; }
};

static GemmArgs part_qkv_args(const Part& p, const Layer& Lq) {
  const Ctx& c = p.c;
  const f5h_arch& a = c.e->a;
  GemmArgs g = qkv_gargs(c, p.aop, Lq.qkv, p.rows, c.L, p.q, p.k, p.v, Lq.q_norm_w, Lq.k_norm_w);
  if (a.pe_attn_head > 0) g.rope_heads = a.pe_attn_head;
  if (c.rag_B) {  // packed rows into padded panels [sequences, H, rag_L, 64] (kernels.h qkv_rowtab)
    g.add = reinterpret_cast<const float*>(c.b.rg_tab);
    g.seq_len = c.rag_L;
    g.qkv_dst_len = c.rag_L;
  }
  return g;
}
static int part_attention(Part& p) {
  Ctx& c = p.c;
  const f5h_arch& a = c.e->a;
  Bufs& b = c.b;
  AttnArgs at{};
  at.kv_len = ((a.attn_mask_enabled || c.isolate) && c.batch_mask) ? b.kvlen + p.s0 : nullptr;
  // pad query rows' outputs are zeroed after to_out (modules.py:551-553): their blocks are skipped
  at.q_len = (c.batch_mask && c.m.pad_skip) ? b.kvlen + p.s0 : nullptr;
  if (!c.rag_B) return launch_attention(c, p.st, at, p.q, p.k, p.v, p.o, p.ns, c.L);
  // ragged: the sequences' own lengths as key and query lengths; O back to the packed rows
  at.kv_len = at.q_len = b.rg_len;
  at.o_split = kAttnRagged;
  at.o2 = b.rg_off;
  return launch_attention(c, p.st, at, p.q, p.k, p.v, p.o, p.ns * c.rag_B, c.rag_L);
}
// the out-projection's pad-row skip: row tiles of padding only do no work at all (in place only)
static void live_rows(const Part& p, GemmArgs& g) {
  g.live_len = p.c.b.kvlen + p.s0;
  g.live_seq = p.c.L;
}
// The folds (DESIGN.md §3 'LayerNorm fold'): a producer GEMM writes its output rows' statistics per 64-column strip,
// the consumer GEMM applies the norm as algebra. LayerNorm form: the producer also stores hs = h (1 + scale), the
// consumer takes the step's u / v. RMSNorm form: x / max(|x|, 1e-12) sqrt(d) = x / sqrt(ss / d) (the epsilon only
// keeps an all-zero row finite), the consumer reads the residual stream itself with W diag(g).
static void fold_producer(const Part& p, GemmArgs& g, const float* scale) {
  g.hs = p.aop;
  g.hs_scale = scale;
  g.ln_part = p.lnp;
  g.ln_nparts = p.c.e->a.dim / 64;
}
static void fold_consumer(const Part& p, GemmArgs& g, const float* u, const float* v) {
  g.ln_part_in = p.lnp;
  g.ln_nparts = p.c.e->a.dim / 64;
  g.ln_u = u;
  g.ln_v = v;
  g.ln_eps = 1e-6f;  // LayerNorm eps (modules.py:316,336)
}
static void rms_producer(const Part& p, GemmArgs& g) {
  g.ln_part = p.lnp;
  g.ln_nparts = p.c.e->a.dim / 64;
  g.ln_rms = 1;
}
static void rms_consumer(const Part& p, GemmArgs& g, const void* A, const Lin& Wg) {
  g.A = A;
  g.W = Wg.w;
  g.ln_part_in = p.lnp;
  g.ln_nparts = p.c.e->a.dim / 64;
  g.ln_rms = 1;
  g.ln_eps = 1e-30f;
}

// DiT block l on the stream h, in place (modules.py:743-757). qkv_done: this layer's LayerNorm + QKV came with the
// previous layer's chain; final_done: the final LayerNorm came with this (the last) layer's chain.
// In-launch phase chain (chain.hip, Part::chain_on): the out-projection .. FFN2 plus the next layer's LayerNorm + QKV
// (or the final LayerNorm) as one launch. LayerNorm fold (Part::fold_on): the attention-norm of layers 1.. and every
// FFN-norm run inside the GEMMs around them; the first layer's attention-norm and the final norm stay launches.
static int dit_layer(Part& p, int l, void* h, bool& qkv_done, bool& final_done) {
  Ctx& c = p.c;
  f5h_engine* e = c.e;
  const f5h_arch& a = e->a;
  const StepModes& m = c.m;
  const int d = a.dim, F = a.ff_dim, inner = a.heads * 64, rows = p.rows;
  hipStream_t st = p.st;
  Layer& Ly = e->layers[l];
  const float* ad = p.ada_k + (size_t)l * 6 * d;  // (shift_msa, scale_msa, gate_msa, shift_mlp, scale_mlp, gate_mlp)
  const int epi_resid = m.r16 ? EPI_RESID16 : EPI_RESID;
  // lnf: layer l's u/v block of the current step's table row (kernels.h LnFoldArgs layout)
  const float* lnf = p.ada_k + e->ada.Npad + (int64_t)l * (2 * (int64_t)F + 6 * (int64_t)d);
  auto mx_act = [&](int kclass) { return (m.mx & kStoreBit(kclass)) ? &p.act : nullptr; };
  if (!qkv_done) {
    const bool folded = p.fold_on && l > 0;  // the previous layer's FFN2 produced this attention-norm
    if (m.do_ln && !folded) RC(adaln_norm(c, st, false, h, rows, ad /*shift_msa*/, ad + d /*scale_msa*/, p.aop, mx_act(KC_QKV)));
    GemmArgs g = part_qkv_args(p, Ly);
    if (folded) fold_consumer(p, g, lnf + 2 * F, lnf + 2 * F + 3 * d);
    RC(layer_gemm(c, st, KC_QKV, EPI_QKV, g, Ly.qkv, m.mx, p.act));
  }
  qkv_done = false;
  RC(part_attention(p));
  if (p.chain_on) {
    ChainArgs ca{};
    ca.out = gargs(p.o, inner, Ly.out, rows, h, d);
    ca.out.gate = ad + 2 * d;  // gate_msa
    ca.ln1 = LnArgs{h, p.aop, ad + 3 * d /*shift_mlp*/, ad + 4 * d /*scale_mlp*/};
    ca.ff1 = gargs(p.aop, d, Ly.ff1, rows, p.f, F);
    ca.ff2 = gargs(p.f, F, Ly.ff2, rows, h, d);
    ca.ff2.gate = ad + 5 * d;  // gate_mlp
    if (l + 1 < a.depth) {
      const float* an = ad + 6 * d;
      ca.ln2 = LnArgs{h, p.aop, an /*shift_msa*/, an + d /*scale_msa*/};
      ca.qkv = part_qkv_args(p, e->layers[l + 1]);
    } else {
      const float* fin = ad + 6 * d;  // AdaLayerNorm_Final: (scale, shift)
      ca.ln2 = LnArgs{h, p.aop, fin + d, fin};
    }
    ca.cnt = c.b.chain + (size_t)l * 5 * c.b.chain_g4;
    ca.groups = (rows + kChainRows - 1) / kChainRows;
    ca.fault = e->chain_fault;
    ProbeScope ps(c, KC_CHAIN, st, &ca.probe);
    const hipError_t ce = chain_launch(e->bf, ca, st);
    if (ce == hipSuccess) {
      e->n_chain.fetch_add(1, std::memory_order_relaxed);
      qkv_done = l + 1 < a.depth;
      final_done = l + 1 == a.depth;
      return 0;
    }
    if (ce != hipErrorInvalidValue) KCK(ce);  // shapes outside the chain: the separate launches below
  }
  {
    GemmArgs g = gargs(p.o, inner, Ly.out, rows, h, d);
    g.gate = ad + 2 * d;  // gate_msa
    g.rowkeep = p.keep;   // masked_fill of pad rows (modules.py:552-554)
    if (m.out_live_skip) live_rows(p, g);
    if (p.fold_on) fold_producer(p, g, ad + 4 * d /*scale_mlp: hs = h (1 + scale_mlp) for FFN1*/);
    RC(layer_gemm(c, st, KC_OUT, epi_resid, g, Ly.out, m.mx, p.act, true));
  }
  if (!p.fold_on) {
    if (m.do_ln) {
      RC(adaln_norm(c, st, true, h, rows, ad + 3 * d /*shift_mlp*/, ad + 4 * d /*scale_mlp*/, p.aop, mx_act(KC_FFN1)));
    } else {
      ProbeScope ps(c, KC_NORM, st);  // F5H_DIAG_SKIP_LN: the site keeps its stamps around the skipped launch
    }
  }
  {
    GemmArgs g = gargs(p.aop, d, Ly.ff1, rows, p.f, F);
    if (p.fold_on) fold_consumer(p, g, lnf, lnf + F);
    RC(layer_gemm(c, st, KC_FFN1, EPI_GELU_TANH, g, Ly.ff1, m.mx, p.act));
  }
  {
    GemmArgs g = gargs(p.f, F, Ly.ff2, rows, h, d);
    g.gate = ad + 5 * d;  // gate_mlp
    // the next layer's attention-norm: hs = h (1 + scale_msa of layer l + 1) for its QKV
    if (p.fold_on && l + 1 < a.depth) fold_producer(p, g, ad + 6 * d + d);
    RC(layer_gemm(c, st, KC_FFN2, epi_resid, g, Ly.ff2, m.mx, p.act, true));
  }
  return 0;
}
// After the last DiT block: the long skip connection, then the final AdaLN norm of h (or h's projection) into aop
static int dit_tail(Part& p, void* h, void* hkeep, size_t no, bool final_done) {
  Ctx& c = p.c;
  f5h_engine* e = c.e;
  const f5h_arch& a = e->a;
  const int d = a.dim;
  const float* fin = p.ada_k + (size_t)a.depth * 6 * d;  // AdaLayerNorm_Final: (scale, shift)
  if (hkeep) {
    // x = long_skip_connection(cat(x, kept)) (dit.py:364-365): ONE GEMM over K = 2d whose A columns [d, 2d) come
    // from the kept buffer (as the UNetT skip projection), into the free first conv buffer
    void* hl = (char*)c.b.c1 + no * d * p.hsz;
    GemmArgs g = gargs(h, d, e->long_skip, p.rows, hl, d);
    g.A2 = hkeep;
    g.k_split = d;
    KCK(gemm(e->bf, c.m.r16 ? EPI_STORE16 : EPI_STORE, g, p.st));
    h = hl;
  }
  if (!final_done) RC(adaln_norm(c, p.st, false, h, p.rows, fin + d, fin, p.aop));
  return 0;
}

// UNetT block l (unett.py:280-300); h: the previous layer's output on entry, this layer's on return. RMSNorm fold
// (Part::rms_on): the FFN-norm of every layer and the attention-norm of layers 1 .. depth/2 - 1 (whose input FFN2 of
// the previous layer writes) run inside the GEMMs around them. Masked batches too (the producers keep masked rows as
// they are), but never with the pad-row skip on a producer (StepModes::out_live_skip).
static int unett_layer(Part& p, int l, void*& h) {
  Ctx& c = p.c;
  f5h_engine* e = c.e;
  const f5h_arch& a = e->a;
  Bufs& b = c.b;
  const int d = a.dim, bf = e->bf, inner = a.heads * 64, rows = p.rows, half = a.depth / 2;
  const bool r16 = c.m.r16;
  hipStream_t st = p.st;
  Layer& Ly = e->layers[l];
  const int epi_resid = r16 ? EPI_RESID16 : EPI_RESID;
  const void* h_in = nullptr;  // first half: the layer input, kept as its skip connection
  if (l < half) {
    // skips.append(x) (unett.py:283-284): layer l reads xs[l] and writes xs[l+1], so xs[l] stays the skip connection
    // without a copy
    h_in = p.res(b.xs[l]);
    h = p.res(b.xs[l + 1]);
    if (!(p.rms_on && l > 0)) RC(rms_norm(c, st, false, h_in, rows, Ly.g_attn, p.aop));
  } else {
    // x = skip_proj(cat(x, skips.pop())) (unett.py:288-297): ONE GEMM over K = 2d whose A columns [d, 2d) come from
    // the skip buffer; then attention / FFN update the result in place
    void* x_prev = h;
    h = p.res(b.pp[(l - half) & 1]);
    GemmArgs g = gargs(x_prev, d, Ly.skip, rows, h, d);
    g.A2 = p.res(b.xs[a.depth - 1 - l]);
    g.k_split = d;
    KCK(gemm(bf, r16 ? EPI_STORE16 : EPI_STORE, g, st));
    RC(rms_norm(c, st, false, h, rows, Ly.g_attn, p.aop));
  }
  {
    GemmArgs g = part_qkv_args(p, Ly);
    if (p.rms_on && l > 0 && l < half) rms_consumer(p, g, h_in, Ly.qkv_g);  // A = the layer input xs[l] itself
    RC(layer_gemm(c, st, KC_QKV, EPI_QKV, g, Ly.qkv));
  }
  RC(part_attention(p));
  {
    GemmArgs g = gargs(p.o, inner, Ly.out, rows, h, d);
    g.resid = h_in;       // first half: x_in + attn(.) -> the next buffer
    g.rowkeep = p.keep;   // masked_fill of pad rows (modules.py:552-554)
    // only in place: a first-half layer writes x_in + attn into the next buffer, so its pad rows must still be copied
    if (c.m.out_live_skip && !h_in) live_rows(p, g);
    if (p.rms_on) rms_producer(p, g);  // the FFN-norm's statistics of h
    RC(layer_gemm(c, st, KC_OUT, epi_resid, g, Ly.out));
  }
  if (!p.rms_on) RC(rms_norm(c, st, true, h, rows, Ly.g_ff, p.aop));
  {
    GemmArgs g = gargs(p.aop, d, Ly.ff1, rows, p.f, a.ff_dim);
    if (p.rms_on) rms_consumer(p, g, h, Ly.ff1_g);  // A = h itself
    RC(layer_gemm(c, st, KC_FFN1, EPI_GELU_TANH, g, Ly.ff1));
  }
  {
    GemmArgs g = gargs(p.f, a.ff_dim, Ly.ff2, rows, h, d);
    if (p.rms_on && l + 1 < half) rms_producer(p, g);  // the next layer's attention-norm (its input is this h)
    RC(layer_gemm(c, st, KC_FFN2, epi_resid, g, Ly.ff2));
  }
  return 0;
}

// Sequences [s0, s0+ns) of the packed cond/uncond DiT / UNetT forward for the current step, enqueued
// on `st`; result in b.p rows of those sequences. Every buffer is sequence-major, so a part works on
// pointer offsets of the packed buffers; sequences never interact, so a part computes exactly what
// the packed forward computes for its rows (bitwise: GEMM tile configurations agree bit for bit).
static int backbone_part(Ctx& c, int s0, int ns, hipStream_t st) {
  f5h_engine* e = c.e;
  const f5h_arch& a = e->a;
  const StepModes& m = c.m;
  const int d = a.dim, inner = a.heads * 64;
  const bool dit = a.backbone == F5H_DIT;
  const size_t es = e->esz;
  Bufs& b = c.b;
  const size_t ro = (size_t)s0 * c.L;  // first row of the part (L rows per sequence)
  const size_t no = (size_t)s0 * c.N;  // first row in the N-row input-embedding buffers
  auto op = [&](void* base, size_t width) -> void* { return (char*)base + ro * width * es; };
  const size_t mx_kmax = (size_t)std::max(d, a.ff_dim);
  Part p{c, st, s0, ns, ns * c.L, ro, m.r16 ? es : sizeof(float)};
  p.aop = op(b.aop, d);
  p.q = op(b.q, inner);
  p.k = op(b.k, inner);
  p.v = op(b.v, inner);
  p.o = op(b.o, inner);
  p.f = op(b.f, a.ff_dim);
  p.keep = c.batch_mask ? b.rowkeep + ro : nullptr;
  if (m.mx) p.act = Mx8Act{b.a8 + ro * mx_kmax, b.a8s + ro * (mx_kmax / 32)};
  p.lnp = b.lnp ? b.lnp + ro * (size_t)(d / 64) * 2 : nullptr;
  p.ada_k = dit ? b.ada_cur : nullptr;
  p.chain_on = m.chain_eligible && b.chain && s0 == 0 && ns == c.S;
  p.fold_on = m.fold_on && b.lnp;
  p.rms_on = m.rms_on && b.lnp;
  void* h = dit ? p.res(b.h) : p.res(b.xs[0]);  // the layer's output (residual updates land here)
  // ---- input embedding. UNetT's InputEmbedding passes no mask (unett.py:100); isolated, its N audio rows are masked
  // as DiT's are
  RC(input_embed(c, st, ns, no, dit ? p.keep : (c.isolate ? b.rowkeep_n + no : nullptr), h, c.L, dit ? 0 : 1));
  if (!dit) KCK(write_time_token(e->bf, m.r16, b.temb_cur, ns, c.L, d, h, st));
  // long_skip_connection (dit.py:354-355): the stream as it stands after the input embedding, kept for the whole
  // evaluation (a copy: the layers update the stream in place)
  void* hkeep = a.long_skip_connection ? (char*)b.hkeep + ro * d * p.hsz : nullptr;
  if (hkeep) {
    if (e->bf != 0 && !m.r16)
      return fail(F5H_EINVAL, "long_skip_connection: F5H_RES32 (fp32 residual under 16-bit operands) is not supported");
    KCK(hipMemcpyAsync(hkeep, h, (size_t)p.rows * d * p.hsz, hipMemcpyDeviceToDevice, st));
  }
  if (p.chain_on) {  // the chain's arrival counters start every step at zero
    const int64_t words = (int64_t)a.depth * 5 * b.chain_g4;
    if (proc_switches().chain_zero_memset)
      KCK(hipMemsetAsync(b.chain, 0, (size_t)words * sizeof(unsigned), st));
    else
      KCK(zero_words(b.chain, words, st));
  }
  if (p.fold_on || p.rms_on) e->n_lnfold.fetch_add(1, std::memory_order_relaxed);
  // ---- the layers, then the final norm into aop
  if (dit) {
    bool qkv_done = false, final_done = false;
    for (int l = 0; l < a.depth; ++l) RC(dit_layer(p, l, h, qkv_done, final_done));
    RC(dit_tail(p, h, hkeep, no, final_done));
  } else {
    for (int l = 0; l < a.depth; ++l) RC(unett_layer(p, l, h));
    RC(rms_norm(c, st, false, h, p.rows, e->norm_out_g, p.aop));
  }
  return proj_out_tail(c, st, p.aop, p.rows, ro);
}

// The MMDiT backbone (mmdit.py:214-262, modules.py:563-705, 763-846) for all S sequences of the current step; result in
// b.p. Two residual streams, audio h [S,N,d] and text ch [S,nt,d] (it restarts from the call-constant embedding c0 at
// every evaluation: block 0's text-side residual GEMM reads c0 and writes ch, so c0 is never copied). Per block: both
// streams' LN-modulate, two QKV launches into the joint q / k / v [S,H,N+nt,64] (audio rows [0,N), text rows [N,N+nt)
// of every panel, each stream rotated from position 0, GemmArgs::qkv_dst_len), one attention over N + nt rows with the
// output split back (AttnArgs::o_split), then per stream the out-projection, LN-modulate, FFN1 and FFN2 with the
// kernels the DiT block uses. The last block (context_pre_only) only pre-normalises the text stream, with
// AdaLayerNorm_Final's (scale, shift) order. No key is masked (pad audio and pad text keys are attended, as in the
// reference without attn_mask_enabled) unless the call is isolated (Ctx::isolate): then the keys are the two ranges
// [0, dur) and [N, N + text length); audio rows are zeroed where ~mask on batch calls, text rows where text == -1
// always (modules.py:700-703). No phase chain, LayerNorm fold or pad-row skip: the joint layout's live rows are not
// a prefix, and the fold's producers / consumers would need the text stream's statistics buffers.
static int backbone_mmdit(Ctx& c, hipStream_t st) {
  f5h_engine* e = c.e;
  const f5h_arch& a = e->a;
  const int d = a.dim, H = a.heads, inner = H * 64, F = a.ff_dim;
  const size_t es = e->esz;
  Bufs& b = c.b;
  const int rows = c.S * c.N, crows = c.S * c.nt, Lj = c.N + c.nt;
  const bool r16 = c.m.r16;  // residual streams in the operand dtype (16-bit modes), fp32 in the fp32 mode
  const int epi_resid = r16 ? EPI_RESID16 : EPI_RESID;
  const uint8_t* keep = c.batch_mask ? b.rowkeep : nullptr;
  // ---- audio embedding (mmdit.py:75-81): conv_pos_embed(h0) + h0 (the reference passes no mask there: pad rows bleed
  // 15 frames per conv; isolated calls mask them)
  RC(input_embed(c, st, c.S, 0, c.isolate ? keep : nullptr, b.h, c.N, 0));
  // the text stream's start: the conditional rows then the unconditional ones (packed), or the branch asked for
  const char* te0 = r16 ? (const char*)b.c0 : (const char*)b.te;
  const size_t hsz = r16 ? es : sizeof(float);
  const void* c0 = te0 + ((c.S == c.B && c.drop_text) ? (size_t)c.B * c.nt * d * hsz : 0);
  const float* ada_k = b.ada_cur;
  // one stream's QKV into its rows [row0, row0 + seq) of every joint panel
  auto qkv = [&](const void* A, const Lin& W, int M, int seq, size_t row0, const float* qn, const float* kn) -> int {
    GemmArgs g = qkv_gargs(c, A, W, M, seq, (char*)b.q + row0 * 64 * es, (char*)b.k + row0 * 64 * es,
                           (char*)b.v + row0 * 64 * es, qn, kn);
    g.qkv_dst_len = Lj;
    return layer_gemm(c, st, KC_QKV, EPI_QKV, g, W);
  };
  // out-projection or FFN2 of one stream: C += gate (acc + bias) on kept rows, the residual read from `resid` when set
  auto resid_gemm = [&](const void* A, int K, const Lin& W, int M, void* C, const void* resid, const float* gate,
                        const uint8_t* rk, int kclass) -> int {
    GemmArgs g = gargs(A, K, W, M, C, d);
    g.resid = resid;
    g.gate = gate;
    g.rowkeep = rk;
    return layer_gemm(c, st, kclass, epi_resid, g, W);
  };
  auto ffn1 = [&](const void* A, const Lin& W, int M, void* out) -> int {
    GemmArgs g = gargs(A, d, W, M, out, F);
    return layer_gemm(c, st, KC_FFN1, EPI_GELU_TANH, g, W);
  };
  for (int l = 0; l < a.depth; ++l) {
    Layer& Ly = e->layers[l];
    const bool last = l == a.depth - 1;
    const float* ax = ada_k + mm_ada_x(a, l);  // (shift_msa, scale_msa, gate_msa, shift_mlp, scale_mlp, gate_mlp)
    const float* ac = ada_k + mm_ada_c(a, l);  // the same, or (scale, shift) in the last block
    const void* c_in = l == 0 ? c0 : b.ch;
    RC(adaln_norm(c, st, false, b.h, rows, ax, ax + d, b.aop));
    RC(adaln_norm(c, st, false, c_in, crows, last ? ac + d : ac, last ? ac : ac + d, b.caop));
    RC(qkv(b.aop, Ly.qkv, rows, c.N, 0, Ly.q_norm_w, Ly.k_norm_w));
    RC(qkv(b.caop, Ly.qkv_c, crows, c.nt, (size_t)c.N, Ly.cq_norm_w, Ly.ck_norm_w));
    {
      AttnArgs at{};
      at.o2 = b.co;
      at.o_split = c.N;
      // isolated: the audio keys [0, dur) and the text keys [N, N + text length) of the joint sequence
      if (c.isolate) {
        at.kv_len = b.kvlen;
        at.kv_start2 = c.N;
        at.kv_len2 = b.tlen;
      }
      RC(launch_attention(c, st, at, b.q, b.k, b.v, b.o, c.S, Lj));
    }
    RC(resid_gemm(b.o, inner, Ly.out, rows, b.h, nullptr, ax + 2 * d, keep, KC_OUT));
    if (!last) RC(resid_gemm(b.co, inner, Ly.out_c, crows, b.ch, l == 0 ? c0 : nullptr, ac + 2 * d, b.ckeep, KC_OUT));
    RC(adaln_norm(c, st, true, b.h, rows, ax + 3 * d, ax + 4 * d, b.aop));
    RC(ffn1(b.aop, Ly.ff1, rows, b.f));
    RC(resid_gemm(b.f, F, Ly.ff2, rows, b.h, nullptr, ax + 5 * d, nullptr, KC_FFN2));
    if (!last) {
      RC(adaln_norm(c, st, true, b.ch, crows, ac + 3 * d, ac + 4 * d, b.caop));
      RC(ffn1(b.caop, Ly.ff1_c, crows, b.cf));
      RC(resid_gemm(b.cf, F, Ly.ff2_c, crows, b.ch, nullptr, ac + 5 * d, nullptr, KC_FFN2));
    }
  }
  const float* fin = ada_k + mm_ada_fin(a);  // AdaLayerNorm_Final: (scale, shift)
  RC(adaln_norm(c, st, false, b.h, rows, fin + d, fin, b.aop));
  return proj_out_tail(c, st, b.aop, rows, 0);
}

// One packed cond/uncond backbone forward for the current step; result in b.p [S, L, mel]. With a
// second stream (c.st2, graph capture only) the conditional and unconditional branches run as two
// independent launch chains (fork/join by events), so one chain's kernel heads and tails overlap
// the other's bodies instead of leaving CUs idle at every kernel boundary.
static int backbone_step(Ctx& c) {
  if (c.e->a.backbone == F5H_MMDIT) return backbone_mmdit(c, c.st);  // always one chain (f5h_set_cfg_streams: no effect)
  if (!c.st2 || !c.use_cfg) return backbone_part(c, 0, c.S, c.st);
  f5h_engine* e = c.e;
  KCK(hipEventRecord(e->ev_fork, c.st));
  KCK(hipStreamWaitEvent(c.st2, e->ev_fork, 0));
  RC(backbone_part(c, 0, c.B, c.st));
  RC(backbone_part(c, c.B, c.B, c.st2));
  KCK(hipEventRecord(e->ev_join, c.st2));
  KCK(hipStreamWaitEvent(c.st, e->ev_join, 0));
  return 0;
}

// The evaluation times of the multi-stage solvers, as torchdiffeq forms them from a grid held in the parameter
// dtype: dt = t1 - t0, then t0 + 0.5 dt (midpoint) or t0 + dt/3, t0 + dt 2/3 and t1 itself (rk4), every operation
// on fp32 values of 16-bit operands and rounded back to the dtype (the Python scalar 1/3 enters as its fp32 value).
// The grid arrives as fp32 values; it was built in the engine's 16-bit operand dtype (compute, f5h_compute: a model
// run in its own precision) exactly when every value is one of that dtype's, and in fp32 otherwise (fp32
// parameters under a 16-bit compute override), whose stage times then keep fp32 precision. out[steps * stages].
static float round_to(int compute, float x) {
  if (compute == F5H_FP16) return (float)(_Float16)x;
  if (compute != F5H_BF16 || x != x) return x;
  uint32_t u;
  std::memcpy(&u, &x, 4);
  u = (u + 0x7fffu + ((u >> 16) & 1u)) & 0xffff0000u;  // round to nearest even
  std::memcpy(&x, &u, 4);
  return x;
}
void ode_eval_times(int method, int compute, const float* t, int steps, float* out) {
#pragma clang fp contract(off)
  const OdeTableau T = ode_tableau(method);
  for (int i = 0; i <= steps; ++i)
    if (round_to(compute, t[i]) != t[i]) compute = F5H_FP32;
  for (int k = 0; k < steps; ++k) {
    const float t0 = t[k], t1 = t[k + 1];
    const float dt = round_to(compute, t1 - t0);
    for (int s = 0; s < T.stages; ++s) {
      float v = t0;
      if (s > 0) v = T.c[s] == 1.f ? t1 : round_to(compute, t0 + round_to(compute, dt * T.c[s]));
      out[k * T.stages + s] = v;
    }
  }
}

// ============================================================================ C ABI
extern "C" {

size_t f5h_workspace_size_ode(const f5h_engine* e, int32_t B, int32_t N, int32_t nt, int32_t steps, int32_t use_cfg,
                             int32_t method) {
  if (!e || B <= 0 || N <= 0 || steps <= 0 || method < 0 || method >= kOdeMethods) return 0;
  if (e->a.backbone == F5H_MMDIT && nt < 0) return 0;
  WS ws;
  Bufs b;
  layout(e, ws, b, B, N, steps * ode_tableau(method).stages + 1, use_cfg, method, steps,
         e->a.backbone == F5H_MMDIT ? nt : 0);
  return ws.off;
}
size_t f5h_workspace_size(const f5h_engine* e, int32_t B, int32_t N, int32_t nt, int32_t nfe, int32_t use_cfg) {
  return f5h_workspace_size_ode(e, B, N, nt, nfe, use_cfg, F5H_EULER);
}

// The call's buffers (c.b) in the caller's workspace, by the call's shape (c.nfe evaluations = table rows)
static int check_ws(Ctx& c, void* w, size_t bytes) {
  WS ws;
  layout(c.e, ws, c.b, c.B, c.N, c.nfe + 1, c.use_cfg, c.method, c.steps, c.nt, c.rag_B, c.rag_L);
  if (bytes < ws.off)
    return fail(F5H_ENOMEM, "workspace too small: need " + std::to_string(ws.off) + " have " + std::to_string(bytes));
  ws.off = 0;
  ws.base = reinterpret_cast<char*>(w);
  layout(c.e, ws, c.b, c.B, c.N, c.nfe + 1, c.use_cfg, c.method, c.steps, c.nt, c.rag_B, c.rag_L);
  return 0;
}
// MMDiT calls (f5h_sample / f5h_forward): what the joint attention cannot serve
// (use_batch_mask == 2 masks both key ranges itself, whatever attn_mask_enabled says, and is served)
static int check_mmdit_call(const f5h_engine* e, int nt, int batch_mask, int isolate) {
  if (e->a.backbone != F5H_MMDIT) return 0;
  if (nt <= 0) return fail(F5H_EINVAL, "MMDiT needs nt >= 1 text tokens");
  if (e->a.attn_mask_enabled && batch_mask && !isolate)
    return fail(F5H_EINVAL,
                "MMDiT: attn_mask_enabled with a batch mask is not supported: the valid keys [0, dur) and [N, N + "
                "text length) are not a prefix of the joint sequence, and the reference's masked mode is not wired to "
                "the two-range attention (use_batch_mask 2 masks both ranges and isolates the batch)");
  return 0;
}

// The fields every kind of cached graph distinguishes (GraphKey::kind: 0 step, 1 prologue, 2 f5h_forward's step). The
// graphs touch only workspace buffers (the ODE state, the trajectory base and the step index live in the workspace),
// so they are keyed by the workspace and the launch shape. Each site adds what its kind alone depends on; a field it
// leaves at zero does not make that kind capture afresh (the prologue: probe, split, pad_skip, chain, cfg_bits).
static GraphKey graph_key(const Ctx& c, const void* ws, int kind) {
  GraphKey key{};
  key.ws = ws;
  key.kind = kind;
  key.B = c.B;
  key.N = c.N;
  key.nt = c.nt;
  key.nfe = c.nfe;
  key.use_cfg = c.use_cfg;
  key.batch_mask = c.batch_mask + c.isolate;
  key.lnfold = c.m.lnfold;
  key.store = c.store;
  key.mx8 = c.m.mx;
  key.method = c.method;
  key.rag_B = c.rag_B;
  key.rag_L = c.rag_L;
  key.kernel_epoch = g_kernel_epoch.load();
  return key;
}

// The prologue as one captured graph per (workspace, shape): its ~56 launches otherwise cost more
// host time than device time (profiles/r02_call_gaps_c2.txt). The inputs it reads are staged into
// fixed workspace slots first, the grid is read from the device copy. F5H_PROLOGUE_GRAPH=0: eager.
static int prologue_graph(Ctx& c, const f5h_sample_args* a, const GraphKey& key) {
  f5h_engine* e = c.e;
  const size_t bn = (size_t)c.B * c.N;
  HIPCK(hipMemcpyAsync(c.b.in_cond, a->cond, bn * e->a.mel_dim * sizeof(float), hipMemcpyDeviceToDevice, c.st));
  HIPCK(hipMemcpyAsync(c.b.in_mask, a->cond_mask, bn, hipMemcpyDeviceToDevice, c.st));
  if (c.nt > 0)
    HIPCK(hipMemcpyAsync(c.b.in_text, a->text, (size_t)c.B * c.nt * sizeof(int64_t), hipMemcpyDeviceToDevice, c.st));
  HIPCK(hipMemcpyAsync(c.b.in_dur, a->duration, (size_t)c.B * sizeof(int32_t), hipMemcpyDeviceToDevice, c.st));
  const Bufs& b = c.b;
  std::shared_ptr<GraphEntry> hold;
  RC(graph_get(c, key, false,
               [&](Ctx& cc) { return prologue(cc, nullptr, cc.nfe, b.in_cond, b.in_mask, b.in_text, b.in_dur); },
               hold, 1));
  HIPCK(hipGraphLaunch(hold->exec, c.st));
  return note_replays(e, hold.get(), c.st);
}

// One NFE step, eager or as the graph's capture source: backbone -> CFG + Euler (dt and trajectory
// slot from the device step index), which also copies the next step's table row into the fixed
// per-step buffer and bumps the step index (folded: no step_begin / step_advance launches).
static int enqueue_step(Ctx& c, const f5h_sample_args* a) {
  f5h_engine* e = c.e;
  c.site = 0;
  RC(backbone_step(c));
  const bool dit = adaln_bb(e->a);  // an AdaLN table row per evaluation, predictions from row 0 (DiT, MMDiT)
  // what cfg_euler and cfg_rk both take (EulerArgs / RkArgs, kernels.h): state, predictions, CFG, the next table row
  auto common = [&](auto& u) {
    u.y = c.b.y;
    u.B = c.B;
    u.N = c.N;
    u.mel = e->a.mel_dim;
    u.p = c.b.p;
    u.p_seq_stride = (int64_t)c.L * e->proj_out.Npad;
    u.p_row_off = dit ? 0 : 1;
    u.p_ld = e->proj_out.Npad;
    u.use_cfg = c.use_cfg;
    u.cfg = a->cfg_strength;
    u.ypad = c.b.ypad;
    u.compute = e->bf;
    u.trajp = c.b.trajp;
    u.next_src = dit ? c.b.ada : c.b.temb;
    u.next_stride = dit ? e->ada_row : e->a.dim;
    u.next_n = dit ? (int)e->ada_row : e->a.dim;
    u.next_dst = dit ? c.b.ada_cur : c.b.temb_cur;
    u.arrive = reinterpret_cast<unsigned*>(c.b.kstep + kArrive);
    u.tick = e->ptick;
  };
  if (c.method != F5H_EULER) {  // one evaluation of a midpoint / rk4 step: same launches, cfg_rk for cfg_euler
    RkArgs r{};
    common(r);
    r.method = c.method;
    r.kbuf = c.b.kbuf;
    r.keval = c.b.kstep;
    r.sgrid = c.b.sgrid;
    r.neval = c.nfe;
    KCK(cfg_rk(r, c.st));
    return 0;
  }
  EulerArgs u{};
  common(u);
  u.dt = 0.f;
  u.kstep = c.b.kstep;
  u.tgrid = c.b.tgrid;
  u.traj = nullptr;
  u.nfe = c.nfe;
  KCK(cfg_euler(u, c.st));
  return 0;
}

// The NFE loop: eager launches, or one captured step graph replayed nfe times.
static int run_steps(Ctx& c, const f5h_sample_args* a, const void* ws) {
  f5h_engine* e = c.e;
  if (!e->graph_mode) {
    for (int k = 0; k < c.nfe; ++k) RC(enqueue_step(c, a));
    return 0;
  }
  GraphKey key = graph_key(c, ws, 0);
  // MMDiT: the step's launches and the text stream's buffers depend on nt (the other backbones' steps do not)
  if (e->a.backbone != F5H_MMDIT) key.nt = 0;
  const bool split = c.m.split != 0;
  key.probe = c.m.probe_class;
  key.split = split;
  key.pad_skip = c.m.pad_skip;
  key.chain = c.m.chain_call;
  std::memcpy(&key.cfg_bits, &a->cfg_strength, 4);
  std::shared_ptr<GraphEntry> hold;  // keeps the replayed graph alive through the launch loop
  RC(graph_get(c, key, split, [&](Ctx& cc) { return enqueue_step(cc, a); }, hold, c.nfe));
  // the replays-done event is recorded whenever any replay was enqueued, also when a later launch fails:
  // an evicted entry is destroyed only after it (reap_graphs)
  int rc = 0, k = 0;
  for (; k < c.nfe; ++k) {
    const hipError_t le = hipGraphLaunch(hold->exec, c.st);
    if (le != hipSuccess) {
      rc = fail(F5H_EHIP, std::string("hipGraphLaunch: ") + hipGetErrorString(le));
      break;
    }
  }
  if (k > 0) {
    const int r2 = note_replays(e, hold.get(), c.st);
    if (!rc) rc = r2;
  }
  return rc;
}

// A ragged call (f5h_sample_ragged): B utterances of `dur` (host) frames, at most Lmax, as the packed rows of `a`
// (a->B = 1, a->N = R)
struct RagCall {
  int B, Lmax;
  const int32_t* dur;
};
// What an entry point states about its call; call_begin derives the rest of the Ctx from it
struct CallShape {
  int B, N, nt;
  int nfe;  // backbone evaluations (time-table rows)
  int use_cfg, use_batch_mask;
  int method, steps;  // f5h_sample_ode (Ctx::method, Ctx::steps); 0 for f5h_forward
};
// The setup f5h_sample* and f5h_forward share, after their own argument checks: the Ctx of the call with its buffers
// laid out in the workspace, the engine's pending chain fault reported, and the call's chain / fold / store decisions.
// `ticket` lives in the entry point, declared after its UseNote: the ticket's event is recorded first, both after
// every launch of the call.
static int call_begin(f5h_engine* e, hipStream_t st, const CallShape& sh, void* ws, size_t bytes, const RagCall* rg,
                      Ctx& c, ChainTicket& ticket) {
  c.e = e;
  c.st = st;
  c.B = sh.B;
  c.N = sh.N;
  c.nt = sh.nt;
  c.method = sh.method;
  c.steps = sh.steps;
  c.nfe = sh.nfe;
  c.use_cfg = sh.use_cfg;
  c.S = c.use_cfg ? 2 * c.B : c.B;
  c.L = adaln_bb(e->a) ? c.N : c.N + 1;
  if (sh.use_batch_mask < 0 || sh.use_batch_mask > 2) return fail(F5H_EINVAL, "use_batch_mask must be 0, 1 or 2");
  c.batch_mask = sh.use_batch_mask ? 1 : 0;
  c.isolate = sh.use_batch_mask == 2 ? 1 : 0;
  c.rag_B = rg ? rg->B : 0;
  c.rag_L = rg ? rg->Lmax : 0;
  RC(check_mmdit_call(e, c.nt, c.batch_mask, c.isolate));
  RC(check_ws(c, ws, bytes));
  RC(chain_fault_check(e, c.st));
  // the call's modes, from the engine's switches as they stand now; a chain the per-device gate does not admit
  // (chain_admit: a runtime answer, so not step_modes' business) is a chain switched off
  const ProcSwitches& ps = proc_switches();
  ModeIn in{e->a.backbone, e->a.dim, e->a.qk_norm, e->a.long_skip_connection, e->bf,
            e->lnf_ok, e->rmsf_ok, e->chain_fault != nullptr, e->mx8,
            e->chain, e->lnfold, e->pad_skip, e->graph_mode, e->split_cfg, e->mx8_mask, e->probe_class,
            ps.res32, ps.skip_ln, c.use_cfg, c.batch_mask, rg != nullptr};
  c.m = step_modes(in);
  if (c.m.chain_call && !chain_for_call(e, c, ticket)) {
    in.chain = 0;
    c.m = step_modes(in);
  }
  c.store = e->store_policy;
  return 0;
}
// method F5H_EULER: the Euler path exactly as before the other solvers existed (same launches, same layout).
static int sample_impl(f5h_engine* e, void* stream, const f5h_sample_args* a, int method, void* workspace,
                       size_t workspace_bytes, const RagCall* rg = nullptr) {
  if (!e || !a) return fail(F5H_EINVAL, "null engine/args");
  if (a->B <= 0 || a->N <= 0 || a->nt < 0 || a->nfe <= 0 || a->nfe > 512)
    return fail(F5H_EINVAL, "bad B/N/nt/nfe");
  const int stages = ode_tableau(method).stages;
  if (a->nfe * stages > 512)
    return fail(F5H_EINVAL, std::to_string(a->nfe) + " steps x " + std::to_string(stages) + " stages = " +
                                std::to_string(a->nfe * stages) +
                                " backbone evaluations exceed the 512 rows of the per-call time tables");
  if (!a->cond || !a->cond_mask || (!a->duration && !rg) || !a->y0 || !a->t_grid || !a->out || (a->nt > 0 && !a->text))
    return fail(F5H_EINVAL, "null tensor argument");
  if (e->a.backbone == F5H_DIT && (rg ? rg->Lmax : a->N) > 8192)
    return fail(F5H_EINVAL, "N exceeds the text position table (8192)");
  HIPCK(hipSetDevice(e->dev));
  UseNote used{e->uses, reinterpret_cast<hipStream_t>(stream)};  // on every return: the engine's release waits for it
  ChainTicket ticket;  // (declared after `used`: its event is recorded first, both after every launch of the call)
  Ctx c{};
  // evaluations: the time tables hold one row each, the step graph is replayed for each
  const CallShape sh{a->B, a->N, a->nt, a->nfe * stages, a->cfg_strength >= 1e-5f, a->use_batch_mask, method, a->nfe};
  RC(call_begin(e, reinterpret_cast<hipStream_t>(stream), sh, workspace, workspace_bytes, rg, c, ticket));
  if (rg) {
    // the segment table of both branches' sequences, from the host lengths (by kernel argument, stream-ordered); the
    // prologue derives the lengths and the per-row table from it on the device
    std::vector<int32_t> off((size_t)2 * rg->B + 1);
    off[0] = 0;
    for (int s = 0; s < 2 * rg->B; ++s) off[s + 1] = off[s] + rg->dur[s % rg->B];
    HIPCK(seg_upload(off.data(), (int64_t)off.size(), c.b.rg_off, c.st));
  }
  double hp[kHostPhases] = {};
  c.hp = hp;
  const double h0 = host_ms();
  static const bool pro_graph = [] {
    const char* v = getenv("F5H_PROLOGUE_GRAPH");
    return !(v && *v == '0');
  }();
  // the table times: Euler evaluates fn at t_0 .. t_{nfe-1}; the multi-stage solvers at their stage times, derived
  // here in the dtype the grid was built in (ode_eval_times), with the step grid kept beside them for dt
  std::vector<float> evt;
  const float* t_rows = a->t_grid;
  if (method == F5H_EULER) {
    HIPCK(grid_upload(a->t_grid, c.nfe + 1, c.b.tgrid, c.st));
  } else {
    evt.resize(c.nfe);
    ode_eval_times(method, e->bf, a->t_grid, c.steps, evt.data());
    t_rows = evt.data();
    HIPCK(grid_upload(t_rows, c.nfe, c.b.tgrid, c.st));
    HIPCK(grid_upload(a->t_grid, c.steps + 1, c.b.sgrid, c.st));
  }
  const GraphKey pkey = graph_key(c, workspace, 1);
  // (a ragged call's prologue runs eagerly: its text is [B, nt], which the staging slots of a B = 1 layout do not hold)
  if (pro_graph && e->graph_mode && !rg && c.nt <= c.N && prologue_repeats(e, pkey))
    RC(prologue_graph(c, a, pkey));
  else
    RC(prologue(c, t_rows, c.nfe, a->cond, a->cond_mask, a->text, a->duration));
  const double h1 = host_ms();
  const size_t ysz = (size_t)c.B * c.N * e->a.mel_dim;
  HIPCK(hipMemcpyAsync(c.b.y, a->y0, ysz * sizeof(float), hipMemcpyDeviceToDevice, c.st));
  if (a->trajectory)
    HIPCK(hipMemcpyAsync(a->trajectory, a->y0, ysz * sizeof(float), hipMemcpyDeviceToDevice, c.st));
  HIPCK(pack_y(e->bf, c.b.y, c.B * c.N, e->a.mel_dim, c.b.ypad, c.st));
  HIPCK(ptr_upload(a->trajectory, c.b.trajp, c.st));
  // step index and the Euler launch's arrival counter (kstep[kArrive]) start at 0; step 0's table row
  // is copied here, every later one by the previous step's Euler launch
  HIPCK(hipMemsetAsync(c.b.kstep, 0, 64 * sizeof(int), c.st));
  RC(step_prep(c));
  const double h2 = host_ms();
  const double g2 = hp[HP_LOCK] + hp[HP_REAP] + hp[HP_CAPTURE] + hp[HP_INSTANTIATE];
  RC(run_steps(c, a, workspace));
  const double h3 = host_ms();
  HIPCK(final_where_out(a->cond, a->cond_mask, c.b.y, a->out, c.B, c.N, e->a.mel_dim,
                        c.m.chain_call ? e->chain_fault : nullptr, c.st));
  if (c.m.chain_call) RC(chain_fault_note(e, c.st));
  const double h4 = host_ms();
  hp[HP_TOTAL] = h4 - h0;
  hp[HP_PROLOGUE] = h1 - h0;
  hp[HP_LAUNCH] = (h3 - h2) - (hp[HP_LOCK] + hp[HP_REAP] + hp[HP_CAPTURE] + hp[HP_INSTANTIATE] - g2);
  hp[HP_FINAL] = h4 - h3;
  {
    std::lock_guard<std::mutex> g(e->hm);
    std::memcpy(e->last_host, hp, sizeof(hp));
  }
  return 0;
}

int f5h_sample(f5h_engine* e, void* stream, const f5h_sample_args* a, void* workspace, size_t workspace_bytes) {
  return sample_impl(e, stream, a, F5H_EULER, workspace, workspace_bytes);
}
int f5h_sample_ode(f5h_engine* e, void* stream, const f5h_sample_args* a, int32_t method, void* workspace,
                   size_t workspace_bytes) {
  if (method < 0 || method >= kOdeMethods) return fail(F5H_EINVAL, "ode method must be 0 (euler), 1 (midpoint) or 2 (rk4)");
  return sample_impl(e, stream, a, method, workspace, workspace_bytes);
}

static int check_ragged_call(const f5h_engine* e, int B, int64_t R, int Lmax, const int32_t* dur) {
  if (!e) return fail(F5H_EINVAL, "null engine");
  if (e->a.backbone != F5H_DIT)
    return fail(F5H_EINVAL, "ragged sampling serves the DiT backbone only (UNetT's time-token row and MMDiT's joint "
                            "sequence are not packed)");
  if (e->a.text_average_upsampling)
    return fail(F5H_EINVAL, "ragged sampling does not serve text_embedding_average_upsampling");
  if (B <= 0 || R <= 0 || Lmax <= 0) return fail(F5H_EINVAL, "ragged sampling: bad B / R / Lmax");
  // 2R rows index 32-bit buffer descriptors and the division-free row arithmetic of the GEMM epilogues (2^24 rows)
  if (2 * R >= (int64_t)1 << 24) return fail(F5H_EINVAL, "ragged sampling: 2 R must stay below 2^24 rows");
  if (dur) {
    int64_t sum = 0;
    for (int b = 0; b < B; ++b) {
      if (dur[b] < 1) return fail(F5H_EINVAL, "ragged sampling: duration[" + std::to_string(b) + "] is below 1");
      if (dur[b] > Lmax)
        return fail(F5H_EINVAL, "ragged sampling: duration[" + std::to_string(b) + "] exceeds Lmax");
      sum += dur[b];
    }
    if (sum != R) return fail(F5H_EINVAL, "ragged sampling: the durations add up to " + std::to_string(sum) + ", not R");
  }
  return 0;
}
size_t f5h_workspace_size_ragged(const f5h_engine* e, int32_t B, int64_t R, int32_t Lmax, int32_t nt, int32_t steps,
                                 int32_t use_cfg, int32_t method) {
  (void)nt;
  if (!e || steps <= 0 || method < 0 || method >= kOdeMethods || R > INT32_MAX) return 0;
  if (check_ragged_call(e, B, R, Lmax, nullptr)) return 0;
  WS ws;
  Bufs b;
  layout(e, ws, b, 1, (int)R, steps * ode_tableau(method).stages + 1, use_cfg, method, steps, 0, B, Lmax);
  return ws.off;
}
int f5h_sample_ragged(f5h_engine* e, void* stream, const f5h_ragged_args* r, int32_t method, void* workspace,
                      size_t workspace_bytes) {
  if (!e || !r) return fail(F5H_EINVAL, "null engine/args");
  if (method < 0 || method >= kOdeMethods) return fail(F5H_EINVAL, "ode method must be 0 (euler), 1 (midpoint) or 2 (rk4)");
  if (!r->duration) return fail(F5H_EINVAL, "null tensor argument");
  if (r->R > INT32_MAX) return fail(F5H_EINVAL, "ragged sampling: R too large");
  RC(check_ragged_call(e, r->B, r->R, r->Lmax, r->duration));
  f5h_sample_args a{};
  a.B = 1;
  a.N = (int32_t)r->R;
  a.nt = r->nt;
  a.nfe = r->nfe;
  a.cond = r->cond;
  a.cond_mask = r->cond_mask;
  a.text = r->text;
  a.duration = nullptr;
  a.y0 = r->y0;
  a.t_grid = r->t_grid;
  a.cfg_strength = r->cfg_strength;
  a.use_batch_mask = 0;
  a.out = r->out;
  a.trajectory = r->trajectory;
  const RagCall rg{r->B, r->Lmax, r->duration};
  return sample_impl(e, stream, &a, method, workspace, workspace_bytes, &rg);
}

int f5h_forward(f5h_engine* e, void* stream, const f5h_forward_args* a, void* workspace, size_t workspace_bytes) {
  if (!e || !a) return fail(F5H_EINVAL, "null engine/args");
  if (a->B <= 0 || a->N <= 0 || a->nt < 0) return fail(F5H_EINVAL, "bad B/N/nt");
  if (!a->x || !a->cond || !a->cond_mask || !a->duration || !a->pred || (a->nt > 0 && !a->text))
    return fail(F5H_EINVAL, "null tensor argument");
  HIPCK(hipSetDevice(e->dev));
  UseNote used{e->uses, reinterpret_cast<hipStream_t>(stream)};
  ChainTicket ticket;
  Ctx c{};
  const CallShape sh{a->B, a->N, a->nt, 1, a->cfg_infer ? 1 : 0, a->use_batch_mask, 0, 0};
  // these two have always come after the use_batch_mask range check, which call_begin reports first
  const bool mask_ok = sh.use_batch_mask >= 0 && sh.use_batch_mask <= 2;
  if (mask_ok && e->a.backbone == F5H_DIT && a->N > 8192)
    return fail(F5H_EINVAL, "N exceeds the text position table (8192)");
  if (mask_ok && (a->text_cache < 0 || a->text_cache > 2)) return fail(F5H_EINVAL, "text_cache must be 0, 1 or 2");
  RC(call_begin(e, reinterpret_cast<hipStream_t>(stream), sh, workspace, workspace_bytes, nullptr, c, ticket));
  c.drop_audio = (!c.use_cfg && a->drop_audio_cond) ? 1 : 0;
  c.drop_text = (!c.use_cfg && a->drop_text) ? 1 : 0;
  const bool cached = a->text_cache == 2;
  if (a->t_dev) {  // time read on the stream: no host round trip (dit.py:332-333 takes a tensor)
    HIPCK(hipMemcpyAsync(c.b.tgrid, a->t_dev, sizeof(float), hipMemcpyDeviceToDevice, c.st));
    RC(prologue(c, nullptr, 1, a->cond, a->cond_mask, a->text, a->duration, cached));
  } else {
    float tg[2] = {a->t, a->t};
    RC(prologue(c, tg, 1, a->cond, a->cond_mask, a->text, a->duration, cached));
  }
  HIPCK(pack_y(e->bf, a->x, c.B * c.N, e->a.mel_dim, c.b.ypad, c.st));
  HIPCK(hipMemsetAsync(c.b.kstep, 0, sizeof(int), c.st));
  auto body = [](Ctx& cc) -> int {
    cc.site = 0;
    RC(step_prep(cc));
    RC(backbone_step(cc));
    KCK(step_advance(cc.b.kstep, cc.e->ptick, cc.st));
    return 0;
  };
  if (e->graph_mode && a->text_cache != 0) {
    // a kept workspace is reused call after call (the reference's ODE loop over the plugin): the
    // backbone step (workspace buffers only) replays as one graph per (workspace, shape)
    GraphKey key = graph_key(c, workspace, 2);
    key.probe = c.m.probe_class;
    key.pad_skip = c.m.pad_skip;
    key.chain = c.m.chain_call;
    key.drop_text = e->a.backbone == F5H_MMDIT ? c.drop_text : 0;
    std::shared_ptr<GraphEntry> hold;
    RC(graph_get(c, key, false, body, hold, 1));
    HIPCK(hipGraphLaunch(hold->exec, c.st));
    RC(note_replays(e, hold.get(), c.st));
  } else {
    RC(body(c));
  }
  HIPCK(copy_pred(c.b.p, c.S, c.L, adaln_bb(e->a) ? 0 : 1, e->a.mel_dim, e->proj_out.Npad, a->pred,
                  c.m.chain_call ? e->chain_fault : nullptr, c.st));
  if (c.m.chain_call) RC(chain_fault_note(e, c.st));
  return 0;
}

}  // extern "C"
