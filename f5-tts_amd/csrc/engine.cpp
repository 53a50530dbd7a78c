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
#include <hip/hip_runtime.h>

#include <cmath>
#include <cstring>
#include <algorithm>
#include <atomic>
#include <chrono>
#include <cstdio>
#include <memory>
#include <functional>
#include <mutex>
#include <string>
#include <unordered_map>
#include <vector>

#include "../../include/f5h.h"
#include "kernels.h"
#include "reaper.h"

using namespace f5h;

static thread_local std::string g_err;
static int fail(int code, const std::string& msg) {
  g_err = msg;
  return code;
}
int f5h_internal_fail(int code, const std::string& msg) { return fail(code, msg); }
#define HIPCK(x)                                                                               \
  do {                                                                                         \
    hipError_t _e = (x);                                                                       \
    if (_e != hipSuccess) return fail(F5H_EHIP, std::string(#x) + ": " + hipGetErrorString(_e)); \
  } while (0)

#define RC(x)              \
  do {                     \
    int _r = (x);          \
    if (_r) return _r;     \
  } while (0)

struct Lin {
  void* w = nullptr;      // [Npad][K] operand dtype
  float* b = nullptr;     // [Npad] fp32 (may be null)
  int N = 0, K = 0, Npad = 0;
};

struct CNX {
  float *dw_w = nullptr, *dw_b = nullptr, *ln_w = nullptr, *ln_b = nullptr, *gamma = nullptr, *beta = nullptr;
  Lin pw1, pw2;
};

struct Layer {
  Lin qkv, out, ff1, ff2, skip;  // skip: UNetT skip_proj [d][2d] over cat(x, skip) (later half)
  float *g_attn = nullptr, *g_ff = nullptr;  // UNetT RMSNorm gains
  Lin qkv_g, ff1_g;  // UNetT RMSNorm fold: qkv / ff1 with the norm's gain folded in, W diag(g) (same bias)
  float *q_norm_w = nullptr, *k_norm_w = nullptr;  // qk_norm = "rms_norm": the [64] gains of q_norm / k_norm (fp32)
  // MMDiT text stream (modules.py:411-427, 807-812): to_{q,k,v}_c, to_out_c, ff_c and the c_q_norm / c_k_norm gains;
  // the last block (context_pre_only) has qkv_c only
  Lin qkv_c, out_c, ff1_c, ff2_c;
  float *cq_norm_w = nullptr, *ck_norm_w = nullptr;
};
// AdaLN backbones (a per-step modulation table, L = N rows per sequence): DiT and MMDiT
static bool adaln_bb(const f5h_arch& a) { return a.backbone != F5H_UNETT; }
// MMDiT AdaLN table row: per block the audio stream's 6d (attn_norm_x) then the text stream's 6d (attn_norm_c; 2d
// (scale, shift) in the last block, AdaLayerNorm_Final), then norm_out's 2d
static size_t mm_ada_x(const f5h_arch& a, int l) { return (size_t)l * 12 * a.dim; }
static size_t mm_ada_c(const f5h_arch& a, int l) { return mm_ada_x(a, l) + (size_t)6 * a.dim; }
static size_t mm_ada_fin(const f5h_arch& a) { return mm_ada_c(a, a.depth - 1) + (size_t)2 * a.dim; }
constexpr int kMMTextPos = 1024;  // TextEmbedding.precompute_max_pos (mmdit.py:39)

struct GraphKey {
  const void* ws;
  int kind;  // 0: one NFE step, 1: the call prologue (inputs staged into the workspace)
  int B, N, nt, nfe, use_cfg, batch_mask, probe, split, pad_skip, chain, lnfold, store;
  int method;  // f5h_ode_method (nfe counts evaluations = table rows: steps x stages)
  // MMDiT single-branch forward (kind 2): the captured step reads the text stream's start from the conditional or the
  // dropped-text embedding, so drop_text is part of the key (DiT / UNetT: the drop flags act in the prologue only)
  int drop_text;
  // ragged sampling (f5h_sample_ragged; 0 otherwise): utterances and longest utterance. With N = the packed rows R these
  // fix the launch geometry; the lengths themselves live in the workspace's segment tables, not in the key
  int rag_B, rag_L;
  uint64_t kernel_epoch;  // bumped whenever a forced GEMM config changes
  uint32_t cfg_bits;
  bool operator==(const GraphKey& o) const {
    return ws == o.ws && kind == o.kind && B == o.B && N == o.N && nt == o.nt && nfe == o.nfe && kernel_epoch == o.kernel_epoch &&
           use_cfg == o.use_cfg && batch_mask == o.batch_mask && probe == o.probe && cfg_bits == o.cfg_bits &&
           split == o.split && pad_skip == o.pad_skip && chain == o.chain && lnfold == o.lnfold && store == o.store &&
           method == o.method && drop_text == o.drop_text && rag_B == o.rag_B && rag_L == o.rag_L;
  }
};

struct f5h_engine {
  f5h_arch a{};
  int dev = 0;
  int bf = 0;          // compute mode (f5h_compute == ComputeMode): 0 fp32, 1 bf16, 2 fp16 operands
  size_t esz = 4;      // operand element size
  int tdp = 0;         // text_dim padded to 64
  std::vector<void*> allocs;  // device memory from the stream-ordered pool (dev_alloc), freed by the reaper
  hipStream_t mstream = nullptr;  // the engine's own stream: creation-time uploads/packing, frees at release
  Lin t1, t2, ada, in_x, in_ct, proj_out;
  Lin long_skip;  // DiT long_skip_connection [d][2d] over cat(x, kept input embedding) (dit.py:228, 364-365)
  float* text_table = nullptr;
  float* freqs = nullptr;
  std::vector<CNX> cnx;
  void* conv_w[2] = {nullptr, nullptr};
  float* conv_b[2] = {nullptr, nullptr};
  std::vector<Layer> layers;
  float* norm_out_g = nullptr;
  // hipGraph cache of one NFE step (keyed by the call's buffers and shape)
  std::mutex gm;
  std::vector<std::shared_ptr<struct GraphEntry>> graphs;
  // evicted entries whose replays may still be in flight: destroyed by a later graph_get once every
  // event recorded after their replays has completed and no caller holds them (no host wait)
  std::vector<std::shared_ptr<struct GraphEntry>> graveyard;
  std::vector<hipEvent_t> ev_pool;  // completed "replays done" events, reused
  // prologue keys seen once: the prologue is captured only when its shape repeats (a call with a
  // new shape runs it eagerly instead of paying capture + instantiate for one replay)
  std::vector<struct GraphKey> pro_seen;
  int64_t n_evicted = 0, n_reaped = 0;
  std::mutex hm;
  double last_host[8] = {};  // f5h_last_call_host_ms: the newest f5h_sample call's host phases
  hipStream_t cap = nullptr;  // private capture stream (the caller's may be the null stream)
  hipStream_t cap2 = nullptr; // second capture stream: the unconditional CFG branch
  hipEvent_t ev_fork = nullptr, ev_join = nullptr;
  int graph_mode = 1;
  // CFG branches as parallel captured chains: 1 = always, 0 = never, 2 = auto, which is one packed chain:
  // with the round-3 kernels the split measured C2 +2.3 %, C3 +1.0 %, C5 +1.0 % per call and C4 -0.7 %
  // (profiles/r03_ab_cfg_chains.txt; in round 1 it won C5 by 4 %). Env F5H_SPLIT_CFG, f5h_set_cfg_streams.
  int split_cfg = 2;
  // skip the dead pad-row work of the batch path (attention query blocks and out-proj row tiles of padding
  // only): f5h_set_pad_skip, env F5H_NO_PAD_SKIP=1 at creation turns it off. Bitwise identical results.
  int pad_skip = 1;
  // In-launch phase chain of the DiT block-step's row-local seams (chain.hip): f5h_set_chain, env F5H_CHAIN=1 at
  // creation turns it on. Bitwise identical results. OFF by default since round 6: with its counters correctly
  // re-zeroed on every graph replay it measured C2 58.4 vs 51.1 ms unchained (profiles/r06_ab_chain_c2.txt); the
  // round-5 gain came from a captured memset node that later replays did not apply (waits skipped, wrong results).
  int chain = 0;
  // LayerNorm fold (DESIGN.md §3 'LayerNorm fold'): on the 16-bit DiT path without row masks the AdaLN LayerNorms
  // between the residual GEMMs and their consumers run as algebra in those GEMMs (gemm_impl.h LNF) instead of as
  // launches of their own. f5h_set_ln_fold, env F5H_LNFOLD=0 at creation turns it off. lnf_ok: the engine supports
  // it (DiT, 16-bit, dim and ff a multiple of 64, dim <= 1024); lnf_w: device array [W1 of every layer, Wqkv of every
  // layer] for lnfold_uv; ada_row: floats per AdaLN table row (the modulation rows, then per layer the fold's u/v).
  // The same switch covers the UNetT RMSNorm fold (rmsf_ok: 16-bit UNetT, dim a multiple of 64, dim <= 1024; the
  // consumers read the residual stream with W diag(g), Layer::qkv_g / ff1_g).
  int lnfold = 1;
  bool lnf_ok = false, rmsf_ok = false;
  const void** lnf_w = nullptr;
  int64_t ada_row = 0;
  std::atomic<int64_t> n_lnfold{0};  // backbone passes enqueued with the fold
  // Store policy of the layer's five hot launches (kernels.h gemm_store_wt; DESIGN.md §3 'Launch boundaries'):
  // -1 = auto (write-through for the classes of kStoreAutoMask when the launch is a single wave of workgroups: C1 / C2;
  // the batch configurations keep plain stores), 0 = plain, 1 = write-through wherever a variant exists,
  // 0x100 | mask = write-through for the classes in mask (kStoreBit; per-class A/Bs). f5h_set_store_policy.
  int store_policy = -1;
  std::atomic<int64_t> n_store_wt{0}, n_store_plain{0};  // hot launches enqueued with write-through / plain stores
  // The chain's give-up word (chain.h): device memory of the engine, set by a chain wait that expired. The call's final
  // kernel then writes NaN results; a copy of it lands in a pinned host word (fault_host) at the end of every chained
  // call, and the engine's next call reads that word, fails with F5H_EHIP and switches the chain off.
  unsigned* chain_fault = nullptr;
  volatile unsigned* fault_host = nullptr;
  int fault_slot = -1;
  std::atomic<int64_t> n_chain{0};  // chain launches enqueued (eager launches and captures)
  uint64_t use_ctr = 0;
  int64_t n_captures = 0, n_replays = 0;
  // probe
  // Probed launches are timed on the device wall clock (s_memrealtime): GEMM and attention
  // kernels stamp themselves (DevProbe), the others get a stamp kernel on each side. Slots are
  // indexed by (launch site within a step, device step tick), so eager launches and graph
  // replays are timed alike. pstamp[0] (as int) = tick, bumped by every step; pslots =
  // pstamp + 64: kProbeSites x kProbeTicks start stamps, then as many end stamps.
  std::mutex pm;
  int probe_class = -1;
  unsigned long long* pstamp = nullptr;
  unsigned long long* pslots = nullptr;
  unsigned long long* ptl = nullptr;  // per-workgroup timeline of the first probed launch (kTimelineWG x 4)
  int* ptick = nullptr;
  double wall_khz = 0.0;
  // per stream, an event recorded after the last call's launches: what f5h_engine_destroy waits for
  UseLog uses;
};
static constexpr size_t kGraphCache = 16;  // cached graphs (prologue and step graphs together)
static constexpr size_t kProbeBytes = (64 + 2 * (size_t)kProbeEnd) * sizeof(unsigned long long);

// The step graph touches only workspace buffers (the ODE state, the trajectory base and the step
// index live in the workspace), so it is keyed by the workspace and the launch shape alone.
// Captured step graphs bake in the kernel choice: forcing a GEMM config or an attention variant
// (tuning/tests) moves the epoch so that later calls capture afresh.
static std::atomic<uint64_t> g_kernel_epoch{0};

// Shared by the cache and by every call replaying it: an entry evicted while another thread is
// still in its launch loop is destroyed by the last holder, after the device has drained (an
// already-submitted replay may still be executing).
struct GraphEntry {
  GraphKey key{};
  hipGraphExec_t exec = nullptr;
  uint64_t stamp = 0;
  std::vector<hipEvent_t> inflight;  // recorded after this entry's replays (guarded by f5h_engine::gm)
  // Destroyed only when nothing replays it any more: from the graveyard once `inflight` has
  // completed and no caller holds it, or by f5h_engine_destroy after a device synchronisation.
  ~GraphEntry() {
    if (exec) (void)hipGraphExecDestroy(exec);
    for (hipEvent_t ev : inflight) (void)hipEventDestroy(ev);
  }
};

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
static constexpr size_t kConvPackElems = (size_t)16 * 31 * 64 * 64;
static int pack_conv_weight(const void* src, int src_dt, int d, void* dst, int dst_dt, hipStream_t st) {
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
  for (int j = 0; j < 2; ++j) {
    const std::string p = "audio_embed.conv_pos_embed.conv1d." + std::to_string(j * 2) + ".";
    const WView* w = W.get(p + "weight", (int64_t)d * (d / 16) * 31, &err);
    if (!w) return fail(F5H_ENOWEIGHT, err);
    RC(dalloc(e, kConvPackElems * e->esz, &e->conv_w[j]));
    RC(pack_conv_weight(w->p, w->dt, d, e->conv_w[j], op_dt(e), e->mstream));
    RC(vec_upload(e, W, p + "bias", d, &e->conv_b[j], &err));
  }
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
  if (a.conv_layers > 0) {
    // precompute_freqs_cis(text_dim, 8192) (modules.py:207-218)
    std::vector<float> fc((size_t)8192 * td);
    const int half = td / 2;
    for (int p = 0; p < 8192; ++p)
      for (int i = 0; i < half; ++i) {
        float f = 1.0f / std::pow(10000.0f, (float)(2 * i) / (float)td);
        float ang = (float)p * f;
        fc[(size_t)p * td + i] = std::cos(ang);
        fc[(size_t)p * td + half + i] = std::sin(ang);
      }
    RC(upload(e, fc, &e->freqs));
  }
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
  // ConvPositionEmbedding: [d, d/16, 31] -> [16][31][64 out][64 in] (zero-padded to 64 channels):
  // dst (g, t, o, i) <- src ((g*cg + o)*cg + i)*31 + t
  for (int j = 0; j < 2; ++j) {
    const std::string p = "input_embed.conv_pos_embed.conv1d." + std::to_string(j * 2) + ".";
    const int cg = d / 16;
    const WView* w = W.get(p + "weight", (int64_t)d * cg * 31, &err);
    if (!w) return fail(F5H_ENOWEIGHT, err);
    RC(dalloc(e, kConvPackElems * e->esz, &e->conv_w[j]));
    RC(pack_conv_weight(w->p, w->dt, d, e->conv_w[j], op_dt(e), e->mstream));
    RC(vec_upload(e, W, p + "bias", d, &e->conv_b[j], &err));
  }
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

// ---------------------------------------------------------------- workspace layout
struct WS {
  size_t off = 0;
  char* base = nullptr;
  template <typename T>
  T* take(size_t n) {
    size_t o = off;
    off = (off + n * sizeof(T) + 255) / 256 * 256;
    return base ? reinterpret_cast<T*>(base + o) : nullptr;
  }
};

struct Bufs {
  float *tsin, *th, *temb, *ada;
  void* tin_op;
  float *te, *pw1o, *grn_scr;
  void *dwln, *grno;
  uint8_t* keepfill;
  void* act;
  float* P;
  void* ypad;
  float *h0, *h, *p;
  void *c1, *aop, *q, *k, *v, *o, *f;
  float2* rope;
  uint8_t* rowkeep;
  int32_t* kvlen;
  float* lnp;          // LayerNorm fold partial statistics [rows][d / 64][2]
  unsigned* chain;     // phase-chain arrival counters: [depth][5][chain_g4] (the chain runs on the packed batch only)
  int chain_g4;        // row groups per counter row, rounded up to 4 (16-B rows)
  float *ada_cur, *temb_cur, *tgrid;  // the current step's table rows; device copy of the grid
  int* kstep;                         // device-side NFE step index
  float* y;                           // ODE state [B][N][mel] fp32
  float** trajp;                      // device slot: trajectory base pointer (or null)
  // midpoint / rk4 only: the step grid [steps + 1] (tgrid then holds the evaluation times) and the kept slopes
  float *sgrid, *kbuf;
  // DiT options (null without them): the residual stream as it stood after the input embedding, kept for the
  // long skip connection (residual dtype); the text embedding after average upsampling [2][B][N][td]
  void* hkeep;
  float* te_up;
  // MMDiT text stream (null otherwise), see layout
  void *c0, *ch, *caop, *co, *cf;
  uint8_t* ckeep;
  // isolation (use_batch_mask == 2): the text key range's length per sequence (MMDiT, AttnArgs::kv_len2); UNetT's row
  // mask over the N audio rows of a sequence (b.rowkeep counts the time token's row). The latter lives in keepfill,
  // which only the ConvNeXt text blocks read and UNetT has none of (written after the text embedding; a UNetT with
  // text blocks would get a buffer of its own), so UNetT's workspace keeps its size
  int32_t* tlen;
  uint8_t* rowkeep_n;
  // UNetT residual stream (operand dtype): xs[0..depth/2] -- layer l < depth/2 reads xs[l] (its
  // skip connection, kept) and writes xs[l+1]; later layers ping-pong between pp[0] and pp[1]
  std::vector<void*> xs;
  void* pp[2];
  // the call's inputs staged into the workspace (prologue graph): cond [B][N][mel] fp32,
  // cond_mask [B][N], text [B][<= N] (int64), duration [B]
  float* in_cond;
  uint8_t* in_mask;
  int64_t* in_text;
  int32_t* in_dur;
  // ragged sampling (null otherwise): the segment table of the 2B sequences, off[2B + 1] (the conditional branch's B
  // utterances, then the unconditional branch's; off[B] = R, off[2B] = 2R), their lengths [2B] and the per-row
  // (sequence, position) table [2R] of the QKV epilogue
  int32_t *rg_off, *rg_len;
  int2* rg_tab;
};

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
}

// ---------------------------------------------------------------- probe
enum { KC_FFN1 = 0, KC_ATTN = 1, KC_QKV = 2, KC_FFN2 = 3, KC_CONV = 4, KC_OUT = 5, KC_NORM = 6, KC_CHAIN = 7 };
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
// Times one launch site when its kernel class is probed. With `kp` the kernel stamps itself
// (GemmArgs/AttnArgs::probe); without, stamp kernels bracket the launch.
struct ProbeScope {
  f5h_engine* e;
  hipStream_t st;
  bool on;
  bool self = false;
  unsigned long long* slots = nullptr;
  ProbeScope(f5h_engine* e_, int kc, hipStream_t s, int* site, DevProbe* kp = nullptr)
      : e(e_), st(s), on(e_->probe_class == kc && e_->pslots && *site < kProbeSites) {
    if (!on) return;
    const int s0 = (*site)++;
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
struct Ctx {
  f5h_engine* e;
  hipStream_t st;
  Bufs b;
  int B, N, nt, S, L, nfe, use_cfg, batch_mask;
  // use_batch_mask == 2 (batch_mask is 1 as well): every sequence is computed as if it were alone -- pad rows and
  // pad keys of the batch reach no valid row (conv_pos row masks on every backbone, key lengths on every attention,
  // the text embedding's GRN and depthwise conv bounded by the sequence's own length)
  int isolate;
  int method, steps;  // f5h_ode_method and grid steps of an f5h_sample_ode call; nfe = steps x stages evaluations
  int drop_audio, drop_text;  // single-branch forward only (f5h_forward with cfg_infer = 0)
  hipStream_t st2;            // second stream for the unconditional branch (step-graph capture), or null
  int site;  // probe launch-site counter, reset at the start of every step's enqueue
  int chain;  // this call may run the phase chain (engine switch, shape, and chain_admit's per-device check)
  int lnfold;  // this call runs the LayerNorm fold (engine switch, shape; never beside the chain)
  int store;   // the engine's store policy at the start of the call
  double* hp;  // host milliseconds of the call by phase (kHostPhases, f5h_last_call_host_ms), or null
  // ragged sampling (f5h_sample_ragged; rag_B = 0 otherwise): rag_B utterances of at most rag_L frames as packed rows.
  // The row-local launches see B = 1, N = L = R (one "sequence" per CFG branch); the four kernels that reach across
  // rows take the segment tables (Bufs rg_*), which the call uploads before the prologue
  int rag_B, rag_L;
};
// Host time of an f5h_sample call by phase (f5h_last_call_host_ms): a call that blocks the host shows where.
enum { HP_TOTAL = 0, HP_PROLOGUE, HP_LOCK, HP_REAP, HP_CAPTURE, HP_INSTANTIATE, HP_LAUNCH, HP_FINAL, kHostPhases };
static double host_ms() {
  return std::chrono::duration<double, std::milli>(std::chrono::steady_clock::now().time_since_epoch()).count();
}

static GemmArgs gargs(const void* A, int64_t lda, const Lin& W, int M, void* C, int64_t ldc) {
  GemmArgs g{};
  g.A = A;
  g.lda = lda;
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

#define KCK(x)                                                                                  \
  do {                                                                                          \
    hipError_t _e = (x);                                                                        \
    if (_e != hipSuccess) return fail(F5H_EHIP, std::string(#x) + ": " + hipGetErrorString(_e)); \
  } while (0)

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
      if (c.lnfold) {  // every step's u / v of the folded LayerNorms (kernels.h LnFoldArgs)
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

// Sequences [s0, s0+ns) of the packed cond/uncond backbone forward for the current step, enqueued
// on `st`; result in b.p rows of those sequences. Every buffer is sequence-major, so a part works on
// pointer offsets of the packed buffers; sequences never interact, so a part computes exactly what
// the packed forward computes for its rows (bitwise: GEMM tile configurations agree bit for bit).
static int backbone_part(Ctx& c, int s0, int ns, hipStream_t st) {
  f5h_engine* e = c.e;
  const f5h_arch& a = e->a;
  const int d = a.dim, bf = e->bf, H = a.heads, inner = H * 64;
  const bool dit = a.backbone == F5H_DIT;
  const size_t es = e->esz;
  Bufs& b = c.b;
  const int BN = c.B * c.N;
  const int rows = ns * c.L;
  const size_t ro = (size_t)s0 * c.L;  // first row of the part (L rows per sequence)
  const size_t no = (size_t)s0 * c.N;  // first row in the N-row input-embedding buffers
  auto op = [&](void* base, size_t row, size_t width) -> void* { return (char*)base + row * width * es; };
  const uint8_t* keep = c.batch_mask ? b.rowkeep + ro : nullptr;
  // residual stream: the operand dtype (as the reference keeps it in the parameter dtype), i.e. 16 bit
  // in the bf16/fp16 modes for DiT and UNetT alike, fp32 in the fp32 parity mode
  static const bool res32 = [] {  // F5H_RES32=1: fp32 residual on the 16-bit DiT path (A/B)
    const char* v = getenv("F5H_RES32");
    return v && *v == '1';
  }();
  const bool r16 = bf != 0 && (!dit || !res32);
  // F5H_DIAG_SKIP_LN=1: timing-only diagnostic, the 16-bit DiT path skips its LayerNorm launches
  // (wrong results; bounds what removing those launches can save). Never set in tests or benches.
  static const bool skip_ln = [] {
    const char* v = getenv("F5H_DIAG_SKIP_LN");
    const bool on = v && *v == '1';
    if (on) std::fprintf(stderr, "[f5h] F5H_DIAG_SKIP_LN=1: LayerNorm launches skipped, results are WRONG (timing only)\n");
    return on;
  }();
  const bool do_ln = !(skip_ln && r16);
  const size_t hsz = r16 ? es : sizeof(float);
  auto res = [&](void* base) -> void* { return (char*)base + ro * d * hsz; };
  void* bh = dit ? res(b.h) : res(b.xs[0]);
  void* aop = op(b.aop, ro, d);
  void* q = op(b.q, ro, inner);
  void* k = op(b.k, ro, inner);
  void* v = op(b.v, ro, inner);
  void* o = op(b.o, ro, inner);
  void* f = op(b.f, ro, a.ff_dim);
  // ---- input embedding: h0 = y.Wx^T + P, conv position embedding. Sequence s reads y[s % B]; a
  // part holding both branches computes y.Wx^T once and adds both branches' hoisted P rows.
  {
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
    // UNetT's InputEmbedding passes no mask (unett.py:100); isolated, its N audio rows are masked as DiT's are
    cv.rowkeep = dit ? keep : (c.isolate ? b.rowkeep_n + no : nullptr);
    cv.x = b.h0 + no * d;
    cv.x_f32 = 1;
    cv.w = e->conv_w[0];
    cv.bias = e->conv_b[0];
    cv.mode = 0;
    cv.y = op(b.c1, no, d);
    if (c.rag_B) {  // packed rows: the part's sequences by the segment table (always the whole packed batch, s0 == 0)
      cv.ragged = 1;
      cv.S = ns * c.rag_B;
      cv.L = c.rag_L;
      cv.rowkeep = reinterpret_cast<const uint8_t*>(b.rg_off);
    }
    {
      ProbeScope ps(e, KC_CONV, st, &c.site);
      KCK(conv_pos(bf, cv, st));
    }
    cv.x = op(b.c1, no, d);
    cv.x_f32 = bf ? 0 : 1;
    cv.w = e->conv_w[1];
    cv.bias = e->conv_b[1];
    cv.mode = r16 ? 2 : 1;
    cv.y = bh;
    cv.y_seq_stride = c.L;
    cv.y_row_off = dit ? 0 : 1;
    cv.resid = b.h0 + no * d;
    KCK(conv_pos(bf, cv, st));
  }
  if (!dit) KCK(write_time_token(bf, r16, b.temb_cur, ns, c.L, d, bh, st));
  // long_skip_connection (dit.py:354-355): the stream as it stands after the input embedding, kept for the whole
  // evaluation (a copy: the layers update the stream in place)
  void* hkeep = a.long_skip_connection ? (char*)b.hkeep + ro * d * hsz : nullptr;
  if (hkeep) {
    if (bf != 0 && !r16)
      return fail(F5H_EINVAL, "long_skip_connection: F5H_RES32 (fp32 residual under 16-bit operands) is not supported");
    KCK(hipMemcpyAsync(hkeep, bh, (size_t)rows * d * hsz, hipMemcpyDeviceToDevice, st));
  }

  const float* ada_k = dit ? b.ada_cur : nullptr;
  const int epi_resid = r16 ? EPI_RESID16 : EPI_RESID;
  void* h = bh;             // the layer's output (residual updates land here)
  const void* h_in = nullptr;  // UNetT first half: the layer input, kept as its skip connection
  auto qkv_args = [&](const Layer& Lq) {
    GemmArgs g = gargs(aop, d, Lq.qkv, rows, nullptr, 0);
    g.rope = b.rope;
    g.seq_len = c.L;
    g.heads = H;
    g.rope_heads = a.pe_attn_head > 0 ? a.pe_attn_head : H;
    g.q = q;
    g.k = k;
    g.v = v;
    g.q_scale = 0.125f * 1.4426950408889634f;  // softmax scale 1/sqrt(64) in log2 units, folded into q
    g.q_norm_w = Lq.q_norm_w;  // qk_norm (null without it): RMSNorm of every q / k head ahead of RoPE
    g.k_norm_w = Lq.k_norm_w;
    g.qk_norm_eps = 1e-6f;     // modules.py:406-407
    if (c.rag_B) {  // packed rows into padded panels [sequences, H, rag_L, 64] (kernels.h qkv_rowtab)
      g.add = reinterpret_cast<const float*>(b.rg_tab);
      g.seq_len = c.rag_L;
      g.qkv_dst_len = c.rag_L;
    }
    return g;
  };
  // In-launch phase chain (chain.hip): a layer's out-proj .. FFN2 plus the next layer's LayerNorm + QKV (or
  // the final LayerNorm) as one launch. The 16-bit DiT path without row masks (single-utterance calls); not
  // while a chained class is probed (its launches are timed one by one).
  // (the packed batch only, s0 == 0: two chain launches on the two CFG streams run 72 instead of 49 ms at C2, their
  // waiting workgroups holding the slots the other stream's producers need, profiles/r05_ab_c2_prio_split.txt; for
  // the same reason c.chain is off while another stream's chained call is in flight, chain_admit)
  const bool chain_on = c.chain && dit && r16 && do_ln && !keep && d == 1024 && b.chain && s0 == 0 && ns == c.S &&
                        (e->probe_class < 0 || e->probe_class == KC_ATTN || e->probe_class == KC_CONV ||
                         e->probe_class == KC_CHAIN);
  static const bool zero_memset = [] {  // F5H_CHAIN_ZERO=memset: the counters zeroed by a memset node (A/B)
    const char* v = getenv("F5H_CHAIN_ZERO");
    return v && !strcmp(v, "memset");
  }();
  if (chain_on) {
    if (zero_memset)
      KCK(hipMemsetAsync(b.chain, 0, (size_t)a.depth * 5 * b.chain_g4 * sizeof(unsigned), st));
    else
      KCK(zero_words(b.chain, (int64_t)a.depth * 5 * b.chain_g4, st));
  }
  bool qkv_done = false;    // this layer's LayerNorm + QKV came with the previous layer's chain
  bool final_done = false;  // the final LayerNorm came with the last layer's chain
  // LayerNorm fold (engine.lnfold): the attention-norm of layers 1.. and every FFN-norm run inside the GEMMs around
  // them; the first layer's attention-norm and the final norm stay launches. lnf(l): layer l's u/v block of the
  // current step's table row (kernels.h LnFoldArgs layout)
  const bool fold_on = c.lnfold && dit && r16 && do_ln && !keep && !chain_on && b.lnp && e->lnf_ok;
  // UNetT RMSNorm fold (engine.rmsf_ok): the FFN-norm of every layer and the attention-norm of layers 1 .. depth/2 - 1
  // (whose input FFN2 of the previous layer writes) run inside the GEMMs around them; the consumers read the residual
  // stream as A with W diag(g). Masked batches too (the producers keep masked rows as they are), but never with the
  // pad-row skip on a producer (a skipped tile would leave its rows' statistics unwritten)
  const bool rms_on = c.lnfold && !dit && r16 && b.lnp && e->rmsf_ok;
  const int64_t lnf_lw = 2 * (int64_t)a.ff_dim + 6 * (int64_t)d;
  auto lnf = [&](int l) { return ada_k + e->ada.Npad + (int64_t)l * lnf_lw; };
  auto fold_consumer = [&](GemmArgs& g, const float* u, const float* v) {
    g.ln_part_in = b.lnp + ro * (size_t)(d / 64) * 2;
    g.ln_nparts = d / 64;
    g.ln_u = u;
    g.ln_v = v;
    g.ln_eps = 1e-6f;  // LayerNorm eps (modules.py:316,336)
  };
  // RMSNorm form: x / max(|x|, 1e-12) sqrt(d) = x / sqrt(ss / d) (the epsilon only keeps an all-zero row finite)
  auto rms_consumer = [&](GemmArgs& g) {
    g.ln_part_in = b.lnp + ro * (size_t)(d / 64) * 2;
    g.ln_nparts = d / 64;
    g.ln_rms = 1;
    g.ln_eps = 1e-30f;
  };
  auto rms_producer = [&](GemmArgs& g) {
    g.ln_part = b.lnp + ro * (size_t)(d / 64) * 2;
    g.ln_nparts = d / 64;
    g.ln_rms = 1;
  };
  auto fold_producer = [&](GemmArgs& g, const float* scale) {
    g.hs = aop;
    g.hs_scale = scale;
    g.ln_part = b.lnp + ro * (size_t)(d / 64) * 2;
    g.ln_nparts = d / 64;
  };
  if (fold_on || rms_on) e->n_lnfold.fetch_add(1, std::memory_order_relaxed);
  // store policy of a hot launch (its final arguments): write-through or plain stores
  auto count_store = [&](int wt) { (wt ? e->n_store_wt : e->n_store_plain).fetch_add(1, std::memory_order_relaxed); };
  auto gemm_policy = [&](GemmArgs& g, int epi, int kclass) {
    g.store_wt = gemm_store_wt(bf, epi, g, store_want(c.store, kclass));
    count_store(g.store_wt);
  };
  for (int l = 0; l < a.depth; ++l) {
    Layer& Ly = e->layers[l];
    const float* ad = ada_k ? ada_k + (size_t)l * 6 * d : nullptr;
    if (!dit) {
      const int half = a.depth / 2;
      if (l < half) {
        // skips.append(x) (unett.py:283-284): layer l reads xs[l] and writes xs[l+1], so xs[l] stays
        // the skip connection without a copy
        h_in = res(b.xs[l]);
        h = res(b.xs[l + 1]);
        if (!(rms_on && l > 0)) KCK(rms_norm_g(bf, h_in, r16, rows, d, Ly.g_attn, aop, st));
      } else {
        // x = skip_proj(cat(x, skips.pop())) (unett.py:288-297): ONE GEMM over K = 2d whose A columns
        // [d, 2d) come from the skip buffer; then attention/FFN update the result in place
        void* x_prev = h;
        h = res(b.pp[(l - half) & 1]);
        h_in = nullptr;
        GemmArgs g = gargs(x_prev, d, Ly.skip, rows, h, d);
        g.A2 = res(b.xs[a.depth - 1 - l]);
        g.k_split = d;
        KCK(gemm(bf, r16 ? EPI_STORE16 : EPI_STORE, g, st));
        KCK(rms_norm_g(bf, h, r16, rows, d, Ly.g_attn, aop, st));
      }
    } else {
      if (do_ln && !qkv_done && !(fold_on && l > 0))
        KCK(ln_modulate(bf, h, r16, rows, d, ad /*shift_msa*/, ad + d /*scale_msa*/, aop, st));
    }
    if (!qkv_done) {
      GemmArgs g = qkv_args(Ly);
      if (fold_on && l > 0) fold_consumer(g, lnf(l) + 2 * a.ff_dim, lnf(l) + 2 * a.ff_dim + 3 * d);
      if (rms_on && l > 0 && l < a.depth / 2) {  // A = the layer input xs[l] itself, W diag(g_attn)
        g.A = h_in;
        g.W = Ly.qkv_g.w;
        rms_consumer(g);
      }
      gemm_policy(g, EPI_QKV, KC_QKV);
      ProbeScope ps(e, KC_QKV, st, &c.site, &g.probe);
      KCK(gemm(bf, EPI_QKV, g, st));
    }
    qkv_done = false;
    {
      AttnArgs at{};
      at.q = q;
      at.k = k;
      at.v = v;
      at.o = o;
      at.S = ns;
      at.H = H;
      at.L = c.L;
      at.kv_len = ((a.attn_mask_enabled || c.isolate) && c.batch_mask) ? b.kvlen + s0 : nullptr;
      // pad query rows' outputs are zeroed after to_out (modules.py:551-553): their blocks are skipped
      at.q_len = (c.batch_mask && e->pad_skip) ? b.kvlen + s0 : nullptr;
      at.prescaled = 1;
      if (c.rag_B) {  // the sequences' own lengths as key and query lengths; O back to the packed rows
        at.S = ns * c.rag_B;
        at.L = c.rag_L;
        at.kv_len = at.q_len = b.rg_len;
        at.o_split = kAttnRagged;
        at.o2 = b.rg_off;
      }
      at.store_wt = attention_store_wt(bf, at, store_want(c.store, KC_ATTN));
      count_store(at.store_wt);
      ProbeScope ps(e, KC_ATTN, st, &c.site, &at.probe);
      KCK(attention(bf, at, st));
    }
    if (chain_on) {
      ChainArgs ca{};
      ca.out = gargs(o, inner, Ly.out, rows, h, d);
      ca.out.gate = ad + 2 * d;  // gate_msa
      ca.ln1 = LnArgs{h, aop, ad + 3 * d /*shift_mlp*/, ad + 4 * d /*scale_mlp*/};
      ca.ff1 = gargs(aop, d, Ly.ff1, rows, f, a.ff_dim);
      ca.ff2 = gargs(f, a.ff_dim, Ly.ff2, rows, h, d);
      ca.ff2.gate = ad + 5 * d;  // gate_mlp
      if (l + 1 < a.depth) {
        const float* an = ada_k + (size_t)(l + 1) * 6 * d;
        ca.ln2 = LnArgs{h, aop, an /*shift_msa*/, an + d /*scale_msa*/};
        ca.qkv = qkv_args(e->layers[l + 1]);
      } else {
        const float* fin = ada_k + (size_t)a.depth * 6 * d;  // AdaLayerNorm_Final: (scale, shift)
        ca.ln2 = LnArgs{h, aop, fin + d, fin};
      }
      ca.cnt = b.chain + (size_t)l * 5 * b.chain_g4;
      ca.groups = (rows + kChainRows - 1) / kChainRows;
      ca.fault = e->chain_fault;
      ProbeScope ps(e, KC_CHAIN, st, &c.site, &ca.probe);
      const hipError_t ce = chain_launch(bf, ca, st);
      if (ce == hipSuccess) {
        e->n_chain.fetch_add(1, std::memory_order_relaxed);
        qkv_done = l + 1 < a.depth;
        final_done = l + 1 == a.depth;
        continue;
      }
      if (ce != hipErrorInvalidValue) KCK(ce);  // shapes outside the chain: the separate launches below
    }
    {
      GemmArgs g = gargs(o, inner, Ly.out, rows, h, d);
      g.resid = h_in;                      // UNetT first half: x_in + attn(.) -> the next buffer
      g.gate = ad ? ad + 2 * d : nullptr;  // gate_msa
      g.rowkeep = keep;                    // masked_fill of pad rows (modules.py:552-554)
      // row tiles of padding only: no work at all. Only in place (h_in null): a UNetT first-half layer
      // writes x_in + attn into the next buffer, so its pad rows must still be copied there
      if (keep && !h_in && e->pad_skip && !rms_on) {
        g.live_len = b.kvlen + s0;
        g.live_seq = c.L;
      }
      if (fold_on) fold_producer(g, ad + 4 * d /*scale_mlp: hs = h (1 + scale_mlp) for FFN1*/);
      if (rms_on) rms_producer(g);  // the FFN-norm's statistics of h
      gemm_policy(g, epi_resid, KC_OUT);
      ProbeScope ps(e, KC_OUT, st, &c.site, &g.probe);
      KCK(gemm(bf, epi_resid, g, st));
    }
    if (!fold_on && !rms_on) {
      ProbeScope ps(e, KC_NORM, st, &c.site);
      if (dit) {
        if (do_ln) KCK(ln_modulate(bf, h, r16, rows, d, ad + 3 * d /*shift_mlp*/, ad + 4 * d /*scale_mlp*/, aop, st));
      }
      else
        KCK(rms_norm_g(bf, h, r16, rows, d, Ly.g_ff, aop, st));
    }
    {
      GemmArgs g = gargs(aop, d, Ly.ff1, rows, f, a.ff_dim);
      if (fold_on) fold_consumer(g, lnf(l), lnf(l) + a.ff_dim);
      if (rms_on) {  // A = h itself, W diag(g_ff)
        g.A = h;
        g.W = Ly.ff1_g.w;
        rms_consumer(g);
      }
      gemm_policy(g, EPI_GELU_TANH, KC_FFN1);
      ProbeScope ps(e, KC_FFN1, st, &c.site, &g.probe);
      KCK(gemm(bf, EPI_GELU_TANH, g, st));
    }
    {
      GemmArgs g = gargs(f, a.ff_dim, Ly.ff2, rows, h, d);
      g.gate = ad ? ad + 5 * d : nullptr;  // gate_mlp
      // the next layer's attention-norm: hs = h (1 + scale_msa of layer l + 1) for its QKV
      if (fold_on && l + 1 < a.depth) fold_producer(g, ada_k + (size_t)(l + 1) * 6 * d + d);
      if (rms_on && l + 1 < a.depth / 2) rms_producer(g);  // the next layer's attention-norm (its input is this h)
      gemm_policy(g, epi_resid, KC_FFN2);
      ProbeScope ps(e, KC_FFN2, st, &c.site, &g.probe);
      KCK(gemm(bf, epi_resid, g, st));
    }
  }
  if (dit) {
    const float* fin = ada_k + (size_t)a.depth * 6 * d;  // AdaLayerNorm_Final: (scale, shift)
    if (hkeep) {
      // x = long_skip_connection(cat(x, kept)) (dit.py:364-365): ONE GEMM over K = 2d whose A columns [d, 2d) come
      // from the kept buffer (as the UNetT skip projection above), into the free first conv buffer
      void* hl = (char*)b.c1 + no * d * hsz;
      GemmArgs g = gargs(h, d, e->long_skip, rows, hl, d);
      g.A2 = hkeep;
      g.k_split = d;
      KCK(gemm(bf, r16 ? EPI_STORE16 : EPI_STORE, g, st));
      h = hl;
    }
    if (!final_done) KCK(ln_modulate(bf, h, r16, rows, d, fin + d, fin, aop, st));
  } else {
    KCK(rms_norm_g(bf, h, r16, rows, d, e->norm_out_g, aop, st));
  }
  // all Npad (128) columns: the padded weight rows and bias are zero, and whole-column tiles take the
  // fast epilogue; readers use the first mel_dim columns of each 128-float row
  const int pld = e->proj_out.Npad;
  GemmArgs g = gargs(aop, d, e->proj_out, rows, b.p + ro * pld, pld);
  g.N = pld;
  KCK(gemm(bf, EPI_STORE, g, st));
  return 0;
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
  const int d = a.dim, bf = e->bf, H = a.heads, inner = H * 64, F = a.ff_dim;
  const size_t es = e->esz;
  Bufs& b = c.b;
  const int BN = c.B * c.N, rows = c.S * c.N, crows = c.S * c.nt, Lj = c.N + c.nt;
  const bool r16 = bf != 0;  // residual streams in the operand dtype (16-bit modes), fp32 in the fp32 mode
  const int epi_resid = r16 ? EPI_RESID16 : EPI_RESID;
  const uint8_t* keep = c.batch_mask ? b.rowkeep : nullptr;
  // ---- audio embedding (mmdit.py:75-81): h0 = y.Wx^T + P, then conv_pos_embed(h0) + h0 (no mask there)
  {
    GemmArgs g = gargs(b.ypad, 128, e->in_x, BN, b.h0, d);
    g.bias = nullptr;
    g.add = b.P;
    g.ld_add = d;
    g.dual_rows = c.S == 2 * c.B ? BN : 0;
    KCK(gemm(bf, EPI_INPROJ, g, st));
    ConvArgs cv{};
    cv.S = c.S;
    cv.L = c.N;
    cv.d = d;
    cv.x = b.h0;
    cv.x_f32 = 1;
    cv.w = e->conv_w[0];
    cv.bias = e->conv_b[0];
    cv.mode = 0;
    cv.y = b.c1;
    cv.rowkeep = c.isolate ? keep : nullptr;  // (the reference passes no mask: pad rows bleed 15 frames per conv)
    {
      ProbeScope ps(e, KC_CONV, st, &c.site);
      KCK(conv_pos(bf, cv, st));
    }
    cv.x = b.c1;
    cv.x_f32 = bf ? 0 : 1;
    cv.w = e->conv_w[1];
    cv.bias = e->conv_b[1];
    cv.mode = r16 ? 2 : 1;
    cv.y = b.h;
    cv.y_seq_stride = c.N;
    cv.y_row_off = 0;
    cv.resid = b.h0;
    KCK(conv_pos(bf, cv, st));
  }
  // the text stream's start: the conditional rows then the unconditional ones (packed), or the branch asked for
  const char* te0 = r16 ? (const char*)b.c0 : (const char*)b.te;
  const size_t hsz = r16 ? es : sizeof(float);
  const void* c0 = te0 + ((c.S == c.B && c.drop_text) ? (size_t)c.B * c.nt * d * hsz : 0);
  const float* ada_k = b.ada_cur;
  auto count_store = [&](int wt) { (wt ? e->n_store_wt : e->n_store_plain).fetch_add(1, std::memory_order_relaxed); };
  auto gemm_policy = [&](GemmArgs& g, int epi, int kclass) {
    g.store_wt = gemm_store_wt(bf, epi, g, store_want(c.store, kclass));
    count_store(g.store_wt);
  };
  auto qkv = [&](const void* A, const Lin& W, int M, int seq, size_t row0, const float* qn, const float* kn) -> int {
    GemmArgs g = gargs(A, d, W, M, nullptr, 0);
    g.rope = b.rope;
    g.seq_len = seq;
    g.qkv_dst_len = Lj;
    g.heads = H;
    g.rope_heads = H;
    g.q = (char*)b.q + row0 * 64 * es;
    g.k = (char*)b.k + row0 * 64 * es;
    g.v = (char*)b.v + row0 * 64 * es;
    g.q_scale = 0.125f * 1.4426950408889634f;  // softmax scale 1/sqrt(64) in log2 units, folded into q
    g.q_norm_w = qn;
    g.k_norm_w = kn;
    g.qk_norm_eps = 1e-6f;
    gemm_policy(g, EPI_QKV, KC_QKV);
    ProbeScope ps(e, KC_QKV, st, &c.site, &g.probe);
    KCK(gemm(bf, EPI_QKV, g, st));
    return 0;
  };
  // out-projection or FFN2 of one stream: C += gate (acc + bias) on kept rows, the residual read from `resid` when set
  auto resid_gemm = [&](const void* A, int K, const Lin& W, int M, void* C, const void* resid, const float* gate,
                        const uint8_t* rk, int kclass) -> int {
    GemmArgs g = gargs(A, K, W, M, C, d);
    g.resid = resid;
    g.gate = gate;
    g.rowkeep = rk;
    gemm_policy(g, epi_resid, kclass);
    ProbeScope ps(e, kclass, st, &c.site, &g.probe);
    KCK(gemm(bf, epi_resid, g, st));
    return 0;
  };
  auto ffn1 = [&](const void* A, const Lin& W, int M, void* out) -> int {
    GemmArgs g = gargs(A, d, W, M, out, F);
    gemm_policy(g, EPI_GELU_TANH, KC_FFN1);
    ProbeScope ps(e, KC_FFN1, st, &c.site, &g.probe);
    KCK(gemm(bf, EPI_GELU_TANH, g, st));
    return 0;
  };
  for (int l = 0; l < a.depth; ++l) {
    Layer& Ly = e->layers[l];
    const bool last = l == a.depth - 1;
    const float* ax = ada_k + mm_ada_x(a, l);  // (shift_msa, scale_msa, gate_msa, shift_mlp, scale_mlp, gate_mlp)
    const float* ac = ada_k + mm_ada_c(a, l);  // the same, or (scale, shift) in the last block
    const void* c_in = l == 0 ? c0 : b.ch;
    KCK(ln_modulate(bf, b.h, r16, rows, d, ax, ax + d, b.aop, st));
    KCK(ln_modulate(bf, c_in, r16, crows, d, last ? ac + d : ac, last ? ac : ac + d, b.caop, st));
    RC(qkv(b.aop, Ly.qkv, rows, c.N, 0, Ly.q_norm_w, Ly.k_norm_w));
    RC(qkv(b.caop, Ly.qkv_c, crows, c.nt, (size_t)c.N, Ly.cq_norm_w, Ly.ck_norm_w));
    {
      AttnArgs at{};
      at.q = b.q;
      at.k = b.k;
      at.v = b.v;
      at.o = b.o;
      at.o2 = b.co;
      at.o_split = c.N;
      at.S = c.S;
      at.H = H;
      at.L = Lj;
      // isolated: the audio keys [0, dur) and the text keys [N, N + text length) of the joint sequence
      if (c.isolate) {
        at.kv_len = b.kvlen;
        at.kv_start2 = c.N;
        at.kv_len2 = b.tlen;
      }
      at.prescaled = 1;
      at.store_wt = attention_store_wt(bf, at, store_want(c.store, KC_ATTN));
      count_store(at.store_wt);
      ProbeScope ps(e, KC_ATTN, st, &c.site, &at.probe);
      KCK(attention(bf, at, st));
    }
    RC(resid_gemm(b.o, inner, Ly.out, rows, b.h, nullptr, ax + 2 * d, keep, KC_OUT));
    if (!last) RC(resid_gemm(b.co, inner, Ly.out_c, crows, b.ch, l == 0 ? c0 : nullptr, ac + 2 * d, b.ckeep, KC_OUT));
    {
      ProbeScope ps(e, KC_NORM, st, &c.site);
      KCK(ln_modulate(bf, b.h, r16, rows, d, ax + 3 * d, ax + 4 * d, b.aop, st));
    }
    RC(ffn1(b.aop, Ly.ff1, rows, b.f));
    RC(resid_gemm(b.f, F, Ly.ff2, rows, b.h, nullptr, ax + 5 * d, nullptr, KC_FFN2));
    if (!last) {
      {
        ProbeScope ps(e, KC_NORM, st, &c.site);
        KCK(ln_modulate(bf, b.ch, r16, crows, d, ac + 3 * d, ac + 4 * d, b.caop, st));
      }
      RC(ffn1(b.caop, Ly.ff1_c, crows, b.cf));
      RC(resid_gemm(b.cf, F, Ly.ff2_c, crows, b.ch, nullptr, ac + 5 * d, nullptr, KC_FFN2));
    }
  }
  const float* fin = ada_k + mm_ada_fin(a);  // AdaLayerNorm_Final: (scale, shift)
  KCK(ln_modulate(bf, b.h, r16, rows, d, fin + d, fin, b.aop, st));
  const int pld = e->proj_out.Npad;
  GemmArgs g = gargs(b.aop, d, e->proj_out, rows, b.p, pld);
  g.N = pld;
  KCK(gemm(bf, EPI_STORE, g, st));
  return 0;
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

// ---------------------------------------------------------------- phase-chain admission and fault word
// Pinned host words the engines' fault copies land in: one slab per process (allocated once; a hipHostFree per engine
// could wait for the device), slots handed out and returned by index.
static std::mutex g_slot_m;
static unsigned* g_slots = nullptr;
static std::vector<int> g_free_slots;
static constexpr int kFaultSlots = 4096;
static int fault_slot_take(volatile unsigned** host) {
  std::lock_guard<std::mutex> lk(g_slot_m);
  if (!g_slots) {
    void* p = nullptr;
    if (hipHostMalloc(&p, kFaultSlots * 64, hipHostMallocDefault) != hipSuccess) return -1;
    g_slots = static_cast<unsigned*>(p);
    for (int i = kFaultSlots - 1; i >= 0; --i) g_free_slots.push_back(i);
  }
  if (g_free_slots.empty()) return -1;
  const int i = g_free_slots.back();
  g_free_slots.pop_back();
  *host = g_slots + (size_t)i * 16;  // one 64-B line per slot
  **host = 0u;
  return i;
}
static void fault_slot_give(int i) {
  if (i < 0) return;
  std::lock_guard<std::mutex> lk(g_slot_m);
  g_free_slots.push_back(i);
}

// Per-device admission of chained calls. Two phase-chain launches in flight at once starve each
// other: each one's waiting workgroups hold CU slots the other's producers need (C2 72 instead of 49 ms with the two
// CFG branches on their own streams, profiles/r05_ab_c2_prio_split.txt). A call that would chain while a chained
// call from ANOTHER stream is still being enqueued or still runs on the device (its "done" event not complete) takes
// the separate launches instead (bitwise identical results). Calls on one stream are ordered by the stream itself.
// Non-blocking: one hipEventQuery, no wait.
struct ChainGate {
  std::mutex m;
  hipStream_t owner = nullptr;
  bool owned = false;
  int enqueuing = 0;          // chained calls of the owner stream being enqueued
  hipEvent_t done = nullptr;  // recorded on the owner stream after its last chained call
  bool pending = false;
};
static ChainGate g_gate[64];
static std::atomic<int64_t> g_gate_refused{0};

static bool chain_admit(int dev, hipStream_t st) {
  ChainGate& g = g_gate[dev & 63];
  std::lock_guard<std::mutex> lk(g.m);
  if (g.owned && g.owner != st) {
    bool busy = g.enqueuing > 0;
    if (!busy && g.pending) {
      busy = hipEventQuery(g.done) == hipErrorNotReady;
      (void)hipGetLastError();  // hipErrorNotReady is the expected answer for a pending event
      if (!busy) g.pending = false;
    }
    if (busy) {
      g_gate_refused.fetch_add(1, std::memory_order_relaxed);
      return false;
    }
  }
  g.owner = st;
  g.owned = true;
  ++g.enqueuing;
  return true;
}
static void chain_leave(int dev, hipStream_t st) {
  ChainGate& g = g_gate[dev & 63];
  std::lock_guard<std::mutex> lk(g.m);
  --g.enqueuing;
  if (!g.done && hipEventCreateWithFlags(&g.done, hipEventDisableTiming) != hipSuccess) {
    (void)hipGetLastError();
    g.done = nullptr;
    return;
  }
  if (hipEventRecord(g.done, st) == hipSuccess)
    g.pending = true;
  else
    (void)hipGetLastError();
}
// Held for one call: admits the call's chain (or not) and, on every return path, records the gate's "done" event
// after the call's launches.
struct ChainTicket {
  int dev = 0;
  hipStream_t st = nullptr;
  bool held = false;
  ~ChainTicket() {
    if (held) chain_leave(dev, st);
  }
};
// Could this call's step run the chain? (the engine switch and the shapes backbone_part checks per part); if so,
// ask the gate.
static int chain_for_call(f5h_engine* e, const Ctx& c, ChainTicket& t) {
  static const bool res32 = [] {
    const char* v = getenv("F5H_RES32");
    return v && *v == '1';
  }();
  const bool split = e->graph_mode && e->split_cfg == 1 && c.use_cfg;  // the two CFG parts: no chain
  // qk_norm / long_skip_connection: the chain's own QKV phase has no norm and its last launch carries the final
  // LayerNorm, which the long skip projection must precede: such engines always take the separate launches
  if (!e->chain || e->a.backbone != F5H_DIT || e->bf == 0 || res32 || e->a.dim != 1024 || c.batch_mask || split ||
      !e->chain_fault || e->a.qk_norm || e->a.long_skip_connection)
    return 0;
  if (!chain_admit(e->dev, c.st)) return 0;
  t.dev = e->dev;
  t.st = c.st;
  t.held = true;
  return 1;
}
// Start of every sample/forward call: a give-up recorded by an earlier chained call of this engine (its copy in the
// pinned word, landed once that call completed) fails this call and switches the chain off for the engine.
static int chain_fault_check(f5h_engine* e, hipStream_t st) {
  if (!e->fault_host || *e->fault_host == 0u) return 0;
  *e->fault_host = 0u;
  {
    std::lock_guard<std::mutex> g(e->gm);
    e->chain = 0;
  }
  (void)hipMemsetAsync(e->chain_fault, 0, sizeof(unsigned), st);
  return fail(F5H_EHIP,
              "phase chain: a wait for a producer row group gave up in an earlier call of this engine (its output was "
              "set to NaN); the chain is now off for this engine (f5h_set_chain re-enables it)");
}
// End of a chained call: the fault word's copy to the pinned host word, stream-ordered behind the call
static int chain_fault_note(f5h_engine* e, hipStream_t st) {
  if (!e->fault_host) return 0;
  HIPCK(hipMemcpyAsync(const_cast<unsigned*>(e->fault_host), e->chain_fault, sizeof(unsigned), hipMemcpyDeviceToHost,
                       st));
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
  if (a->compute != F5H_FP32 && a->compute != F5H_BF16 && a->compute != F5H_FP16)
    return fail(F5H_EINVAL, "compute must be FP32, BF16 or FP16");
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

const char* f5h_last_error(void) { return g_err.c_str(); }
const char* f5h_version(void) { return "f5h 0.1 gfx950"; }

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
  e->bf = arch->compute;
  e->esz = e->bf ? 2 : 4;
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

// nfe: evaluations (table rows); method / steps: as layout
static int check_ws(f5h_engine* e, int B, int N, int nfe, int use_cfg, void* w, size_t bytes, Ctx& c, int method = 0,
                    int steps = 0) {
  WS ws;
  layout(e, ws, c.b, B, N, nfe + 1, use_cfg, method, steps, c.nt, c.rag_B, c.rag_L);
  if (bytes < ws.off)
    return fail(F5H_ENOMEM, "workspace too small: need " + std::to_string(ws.off) + " have " + std::to_string(bytes));
  ws.off = 0;
  ws.base = reinterpret_cast<char*>(w);
  layout(e, ws, c.b, B, N, nfe + 1, use_cfg, method, steps, c.nt, c.rag_B, c.rag_L);
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

static int run_steps(Ctx& c, const f5h_sample_args* a, const void* ws);
static int graph_get(Ctx& c, const GraphKey& key, bool split, const std::function<int(Ctx&)>& body,
                     std::shared_ptr<GraphEntry>& hold, int64_t replays);
static int note_replays(f5h_engine* e, GraphEntry* g, hipStream_t st);
static bool prologue_repeats(f5h_engine* e, const GraphKey& key);

// The prologue as one captured graph per (workspace, shape): its ~56 launches otherwise cost more
// host time than device time (profiles/r02_call_gaps_c2.txt). The inputs it reads are staged into
// fixed workspace slots first, the grid is read from the device copy. F5H_PROLOGUE_GRAPH=0: eager.
static GraphKey prologue_key(const Ctx& c, const void* ws) {
  GraphKey key{};
  key.ws = ws;
  key.kind = 1;
  key.B = c.B;
  key.N = c.N;
  key.nt = c.nt;
  key.nfe = c.nfe;
  key.use_cfg = c.use_cfg;
  key.batch_mask = c.batch_mask + c.isolate;
  key.lnfold = c.lnfold;
  key.store = c.store;
  key.method = c.method;
  key.rag_B = c.rag_B;
  key.rag_L = c.rag_L;
  key.kernel_epoch = g_kernel_epoch.load();
  return key;
}
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
static void ode_eval_times(int method, int compute, const float* t, int steps, float* out) {
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

int f5h_debug_ode_tableau(int32_t method, int32_t* stages, float* c, float* a, float* b) {
  if (method < 0 || method >= kOdeMethods) return fail(F5H_EINVAL, "ode method must be 0 (euler), 1 (midpoint) or 2 (rk4)");
  const OdeTableau T = ode_tableau(method);
  if (stages) *stages = T.stages;
  if (c) std::memcpy(c, T.c, sizeof(T.c));
  if (a) std::memcpy(a, T.a, sizeof(T.a));
  if (b) std::memcpy(b, T.b, sizeof(T.b));
  return 0;
}
int f5h_debug_ode_eval_times(int32_t method, int32_t compute, const float* t_grid, int32_t steps, float* out) {
  if (method < 0 || method >= kOdeMethods || compute < F5H_FP32 || compute > F5H_FP16 || !t_grid || steps <= 0 || !out)
    return fail(F5H_EINVAL, "bad ode_eval_times argument");
  ode_eval_times(method, compute, t_grid, steps, out);
  return 0;
}

// A ragged call (f5h_sample_ragged): B utterances of `dur` (host) frames, at most Lmax, as the packed rows of `a`
// (a->B = 1, a->N = R)
struct RagCall {
  int B, Lmax;
  const int32_t* dur;
};
static int sample_impl(f5h_engine* e, void* stream, const f5h_sample_args* a, int method, void* workspace,
                       size_t workspace_bytes, const RagCall* rg = nullptr);
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

// method F5H_EULER: the Euler path exactly as before the other solvers existed (same launches, same layout).
static int sample_impl(f5h_engine* e, void* stream, const f5h_sample_args* a, int method, void* workspace,
                       size_t workspace_bytes, const RagCall* rg) {
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
  Ctx c{};
  c.e = e;
  c.st = reinterpret_cast<hipStream_t>(stream);
  c.B = a->B;
  c.N = a->N;
  c.nt = a->nt;
  c.method = method;
  c.steps = a->nfe;
  c.nfe = a->nfe * stages;  // evaluations: the time tables hold one row each, the step graph is replayed for each
  c.use_cfg = a->cfg_strength >= 1e-5f;
  c.S = c.use_cfg ? 2 * c.B : c.B;
  c.L = adaln_bb(e->a) ? c.N : c.N + 1;
  if (a->use_batch_mask < 0 || a->use_batch_mask > 2) return fail(F5H_EINVAL, "use_batch_mask must be 0, 1 or 2");
  c.batch_mask = a->use_batch_mask ? 1 : 0;
  c.isolate = a->use_batch_mask == 2 ? 1 : 0;
  c.rag_B = rg ? rg->B : 0;
  c.rag_L = rg ? rg->Lmax : 0;
  RC(check_mmdit_call(e, c.nt, c.batch_mask, c.isolate));
  RC(check_ws(e, c.B, c.N, c.nfe, c.use_cfg, workspace, workspace_bytes, c, method, c.steps));
  RC(chain_fault_check(e, c.st));
  ChainTicket ticket;  // (declared after `used`: its event is recorded first, both after every launch of the call)
  // ragged: no chain and no fold, as for every masked batch (each utterance then has the bits of its own unfolded call)
  c.chain = rg ? 0 : chain_for_call(e, c, ticket);
  c.lnfold = !rg && e->lnfold && !c.chain && ((e->lnf_ok && !c.batch_mask) || e->rmsf_ok);
  if (rg) {
    // the segment table of both branches' sequences, from the host lengths (by kernel argument, stream-ordered); the
    // prologue derives the lengths and the per-row table from it on the device
    std::vector<int32_t> off((size_t)2 * rg->B + 1);
    off[0] = 0;
    for (int s = 0; s < 2 * rg->B; ++s) off[s + 1] = off[s] + rg->dur[s % rg->B];
    HIPCK(seg_upload(off.data(), (int64_t)off.size(), c.b.rg_off, c.st));
  }
  c.store = e->store_policy;
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
  const GraphKey pkey = prologue_key(c, workspace);
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
                        c.chain ? e->chain_fault : nullptr, c.st));
  if (c.chain) RC(chain_fault_note(e, c.st));
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

// One NFE step, eager or as the graph's capture source: backbone -> CFG + Euler (dt and trajectory
// slot from the device step index), which also copies the next step's table row into the fixed
// per-step buffer and bumps the step index (folded: no step_begin / step_advance launches).
static int enqueue_step(Ctx& c, const f5h_sample_args* a) {
  f5h_engine* e = c.e;
  {
    c.site = 0;
    RC(backbone_step(c));
    const bool dit = adaln_bb(e->a);  // an AdaLN table row per evaluation, predictions from row 0 (DiT, MMDiT)
    if (c.method != F5H_EULER) {  // one evaluation of a midpoint / rk4 step: same launches, cfg_rk for cfg_euler
      RkArgs r{};
      r.y = c.b.y;
      r.B = c.B;
      r.N = c.N;
      r.mel = e->a.mel_dim;
      r.p = c.b.p;
      r.p_seq_stride = (int64_t)c.L * e->proj_out.Npad;
      r.p_row_off = dit ? 0 : 1;
      r.p_ld = e->proj_out.Npad;
      r.use_cfg = c.use_cfg;
      r.cfg = a->cfg_strength;
      r.ypad = c.b.ypad;
      r.compute = e->bf;
      r.method = c.method;
      r.kbuf = c.b.kbuf;
      r.keval = c.b.kstep;
      r.sgrid = c.b.sgrid;
      r.trajp = c.b.trajp;
      r.next_src = dit ? c.b.ada : c.b.temb;
      r.next_stride = dit ? e->ada_row : e->a.dim;
      r.next_n = dit ? (int)e->ada_row : e->a.dim;
      r.next_dst = dit ? c.b.ada_cur : c.b.temb_cur;
      r.neval = c.nfe;
      r.arrive = reinterpret_cast<unsigned*>(c.b.kstep + kArrive);
      r.tick = e->ptick;
      KCK(cfg_rk(r, c.st));
      return 0;
    }
    EulerArgs u{};
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
    u.dt = 0.f;
    u.kstep = c.b.kstep;
    u.tgrid = c.b.tgrid;
    u.ypad = c.b.ypad;
    u.compute = e->bf;
    u.traj = nullptr;
    u.trajp = c.b.trajp;
    u.next_src = dit ? c.b.ada : c.b.temb;
    u.next_stride = dit ? e->ada_row : e->a.dim;
    u.next_n = dit ? (int)e->ada_row : e->a.dim;
    u.next_dst = dit ? c.b.ada_cur : c.b.temb_cur;
    u.nfe = c.nfe;
    u.arrive = reinterpret_cast<unsigned*>(c.b.kstep + kArrive);
    u.tick = e->ptick;
    KCK(cfg_euler(u, c.st));
  }
  return 0;
}

// The NFE loop: eager launches, or one captured step graph replayed nfe times.
static int run_steps(Ctx& c, const f5h_sample_args* a, const void* ws) {
  f5h_engine* e = c.e;
  if (!e->graph_mode) {
    for (int k = 0; k < c.nfe; ++k) RC(enqueue_step(c, a));
    return 0;
  }
  GraphKey key{};
  key.ws = ws;
  key.B = c.B;
  key.N = c.N;
  // MMDiT: the step's launches and the text stream's buffers depend on nt (the other backbones' steps do not)
  key.nt = e->a.backbone == F5H_MMDIT ? c.nt : 0;
  key.nfe = c.nfe;
  key.use_cfg = c.use_cfg;
  key.batch_mask = c.batch_mask + c.isolate;
  key.probe = e->probe_class;
  // auto (2): one packed chain. Ragged: always one chain (the segment tables address the packed batch as a whole)
  const bool split = e->split_cfg == 1 && !c.rag_B;
  key.rag_B = c.rag_B;
  key.rag_L = c.rag_L;
  key.split = split;
  key.pad_skip = e->pad_skip;
  key.chain = c.chain;
  key.lnfold = c.lnfold;
  key.store = c.store;
  key.method = c.method;
  key.kernel_epoch = g_kernel_epoch.load();
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

// F5H_HOST_TRACE=1: host time of the graph-cache phases on stderr (diagnostic)
static bool host_trace() {
  static const bool on = [] {
    const char* v = getenv("F5H_HOST_TRACE");
    return v && *v == '1';
  }();
  return on;
}
// Destroy graveyard entries that nothing replays any more: every event recorded after their
// replays has completed and no caller holds them. Non-blocking (hipEventQuery); caller holds e->gm.
static void reap_graphs(f5h_engine* e) {
  auto done = [e](GraphEntry& g) {
    size_t k = 0;
    for (hipEvent_t ev : g.inflight) {
      if (hipEventQuery(ev) == hipSuccess)
        e->ev_pool.push_back(ev);
      else
        g.inflight[k++] = ev;
    }
    (void)hipGetLastError();  // hipErrorNotReady is the expected answer for a pending event
    g.inflight.resize(k);
    return k == 0;
  };
  for (auto& g : e->graphs)
    if (g->inflight.size() > 4) done(*g);  // keep live entries' lists short
  size_t k = 0;
  for (size_t i = 0; i < e->graveyard.size(); ++i) {
    auto& g = e->graveyard[i];
    if (done(*g) && g.use_count() == 1) {
      ++e->n_reaped;
      continue;  // last reference: destroyed when the slot is overwritten or the vector shrinks
    }
    if (k != i) std::swap(e->graveyard[k], e->graveyard[i]);
    ++k;
  }
  e->graveyard.resize(k);
}

// Record, on `st`, an event after the launches just enqueued from `g` (the entry stays in the
// graveyard until it completes).
static int note_replays(f5h_engine* e, GraphEntry* g, hipStream_t st) {
  hipEvent_t ev = nullptr;
  {
    std::lock_guard<std::mutex> lk(e->gm);
    if (!e->ev_pool.empty()) {
      ev = e->ev_pool.back();
      e->ev_pool.pop_back();
    }
  }
  if (!ev) HIPCK(hipEventCreateWithFlags(&ev, hipEventDisableTiming));
  HIPCK(hipEventRecord(ev, st));
  std::lock_guard<std::mutex> lk(e->gm);
  g->inflight.push_back(ev);
  return 0;
}

// The cached graph for `key`, captured from `body` on the private capture stream(s) when absent.
// An evicted entry moves to the graveyard (no device synchronisation, no wait under the mutex).
static int graph_get(Ctx& c, const GraphKey& key, bool split, const std::function<int(Ctx&)>& body,
                     std::shared_ptr<GraphEntry>& hold, int64_t replays) {
  f5h_engine* e = c.e;
  const double t0 = host_ms();
  std::lock_guard<std::mutex> g(e->gm);
  const double t1 = host_ms();
  const int64_t reaped0 = e->n_reaped;
  reap_graphs(e);
  const double t2 = host_ms();
  if (c.hp) {
    c.hp[HP_LOCK] += t1 - t0;
    c.hp[HP_REAP] += t2 - t1;
  }
  if (host_trace())
    std::fprintf(stderr, "[f5h host] graph_get kind %d: lock %.3f ms, reap %.3f ms (%lld destroyed)\n", key.kind,
                 t1 - t0, t2 - t1, (long long)(e->n_reaped - reaped0));
  for (const auto& x : e->graphs)
    if (x->key == key) hold = x;
  if (!hold) {
    if (!e->cap) HIPCK(hipStreamCreateWithFlags(&e->cap, hipStreamNonBlocking));
    if (split && !e->cap2) {
      HIPCK(hipStreamCreateWithFlags(&e->cap2, hipStreamNonBlocking));
      HIPCK(hipEventCreateWithFlags(&e->ev_fork, hipEventDisableTiming));
      HIPCK(hipEventCreateWithFlags(&e->ev_join, hipEventDisableTiming));
    }
    auto ne = std::make_shared<GraphEntry>();
    ne->key = key;
    Ctx cc = c;
    cc.st = e->cap;
    cc.st2 = split ? e->cap2 : nullptr;
    const double c0 = host_ms();
    hipError_t be = hipStreamBeginCapture(e->cap, hipStreamCaptureModeThreadLocal);
    if (be != hipSuccess) return fail(F5H_EHIP, std::string("hipStreamBeginCapture: ") + hipGetErrorString(be));
    const int rc = body(cc);
    hipGraph_t graph = nullptr;
    const hipError_t ce = hipStreamEndCapture(e->cap, &graph);
    if (rc || ce != hipSuccess) {
      if (graph) (void)hipGraphDestroy(graph);
      if (rc) return rc;
      return fail(F5H_EHIP, std::string("hipStreamEndCapture: ") + hipGetErrorString(ce));
    }
    const double c1 = host_ms();
    const hipError_t ie = hipGraphInstantiate(&ne->exec, graph, nullptr, nullptr, 0);
    (void)hipGraphDestroy(graph);
    if (c.hp) {
      c.hp[HP_CAPTURE] += c1 - c0;
      c.hp[HP_INSTANTIATE] += host_ms() - c1;
    }
    if (host_trace())
      std::fprintf(stderr, "[f5h host] capture %.3f ms, instantiate %.3f ms\n", c1 - c0, host_ms() - c1);
    if (ie != hipSuccess) {
      ne->exec = nullptr;
      return fail(F5H_EHIP, std::string("hipGraphInstantiate: ") + hipGetErrorString(ie));
    }
    if (e->graphs.size() >= kGraphCache) {  // evict the least recently used graph to the graveyard
      size_t lru = 0;
      for (size_t i = 1; i < e->graphs.size(); ++i)
        if (e->graphs[i]->stamp < e->graphs[lru]->stamp) lru = i;
      e->graveyard.push_back(std::move(e->graphs[lru]));
      e->graphs.erase(e->graphs.begin() + lru);
      ++e->n_evicted;
    }
    e->graphs.push_back(ne);
    e->n_captures++;
    hold = ne;
  }
  hold->stamp = ++e->use_ctr;
  e->n_replays += replays;
  return 0;
}

// Prologue graphs pay off only when a shape repeats: true when the prologue graph for `key` is
// cached or the key was seen before (remembered in a short FIFO); a first sighting is recorded.
static bool prologue_repeats(f5h_engine* e, const GraphKey& key) {
  std::lock_guard<std::mutex> g(e->gm);
  for (const auto& x : e->graphs)
    if (x->key == key) return true;
  for (const auto& k : e->pro_seen)
    if (k == key) return true;
  if (e->pro_seen.size() >= 64) e->pro_seen.erase(e->pro_seen.begin());
  e->pro_seen.push_back(key);
  return false;
}

int f5h_forward(f5h_engine* e, void* stream, const f5h_forward_args* a, void* workspace, size_t workspace_bytes) {
  if (!e || !a) return fail(F5H_EINVAL, "null engine/args");
  if (a->B <= 0 || a->N <= 0 || a->nt < 0) return fail(F5H_EINVAL, "bad B/N/nt");
  if (!a->x || !a->cond || !a->cond_mask || !a->duration || !a->pred || (a->nt > 0 && !a->text))
    return fail(F5H_EINVAL, "null tensor argument");
  HIPCK(hipSetDevice(e->dev));
  UseNote used{e->uses, reinterpret_cast<hipStream_t>(stream)};
  Ctx c{};
  c.e = e;
  c.st = reinterpret_cast<hipStream_t>(stream);
  c.B = a->B;
  c.N = a->N;
  c.nt = a->nt;
  c.nfe = 1;
  c.use_cfg = a->cfg_infer ? 1 : 0;
  c.S = c.use_cfg ? 2 * c.B : c.B;
  c.drop_audio = (!c.use_cfg && a->drop_audio_cond) ? 1 : 0;
  c.drop_text = (!c.use_cfg && a->drop_text) ? 1 : 0;
  c.L = adaln_bb(e->a) ? c.N : c.N + 1;
  if (a->use_batch_mask < 0 || a->use_batch_mask > 2) return fail(F5H_EINVAL, "use_batch_mask must be 0, 1 or 2");
  c.batch_mask = a->use_batch_mask ? 1 : 0;
  c.isolate = a->use_batch_mask == 2 ? 1 : 0;
  if (e->a.backbone == F5H_DIT && a->N > 8192) return fail(F5H_EINVAL, "N exceeds the text position table (8192)");
  if (a->text_cache < 0 || a->text_cache > 2) return fail(F5H_EINVAL, "text_cache must be 0, 1 or 2");
  RC(check_mmdit_call(e, c.nt, c.batch_mask, c.isolate));
  RC(check_ws(e, c.B, c.N, 1, c.use_cfg, workspace, workspace_bytes, c));
  RC(chain_fault_check(e, c.st));
  ChainTicket ticket;
  c.chain = chain_for_call(e, c, ticket);
  c.lnfold = e->lnfold && !c.chain && ((e->lnf_ok && !c.batch_mask) || e->rmsf_ok);
  c.store = e->store_policy;
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
    GraphKey key{};
    key.ws = workspace;
    key.kind = 2;
    key.B = c.B;
    key.N = c.N;
    key.nt = c.nt;
    key.nfe = 1;
    key.use_cfg = c.use_cfg;
    key.batch_mask = c.batch_mask + c.isolate;
    key.probe = e->probe_class;
    key.pad_skip = e->pad_skip;
    key.chain = c.chain;
    key.lnfold = c.lnfold;
    key.store = c.store;
    key.drop_text = e->a.backbone == F5H_MMDIT ? c.drop_text : 0;
    key.kernel_epoch = g_kernel_epoch.load();
    std::shared_ptr<GraphEntry> hold;
    RC(graph_get(c, key, false, body, hold, 1));
    HIPCK(hipGraphLaunch(hold->exec, c.st));
    RC(note_replays(e, hold.get(), c.st));
  } else {
    RC(body(c));
  }
  HIPCK(copy_pred(c.b.p, c.S, c.L, adaln_bb(e->a) ? 0 : 1, e->a.mel_dim, e->proj_out.Npad, a->pred,
                  c.chain ? e->chain_fault : nullptr, c.st));
  if (c.chain) RC(chain_fault_note(e, c.st));
  return 0;
}

int f5h_probe_enable(f5h_engine* e, int32_t kclass, int32_t enable) {
  if (!e) return fail(F5H_EINVAL, "null engine");
  std::lock_guard<std::mutex> g(e->pm);
  e->probe_class = enable ? kclass : -1;
  if (e->pstamp) {  // tick = 0, start stamps = max, end stamps = 0
    HIPCK(hipSetDevice(e->dev));
    HIPCK(hipDeviceSynchronize());
    HIPCK(hipMemset(e->pstamp, 0, 64 * sizeof(unsigned long long)));
    HIPCK(hipMemset(e->pslots, 0xff, (size_t)kProbeEnd * sizeof(unsigned long long)));
    HIPCK(hipMemset(e->pslots + kProbeEnd, 0, (size_t)kProbeEnd * sizeof(unsigned long long)));
    HIPCK(hipMemset(e->ptl, 0, (size_t)kTimelineWG * 4 * sizeof(unsigned long long)));
    HIPCK(hipDeviceSynchronize());
  }
  return 0;
}

int f5h_probe_timeline(f5h_engine* e, uint64_t* stamps, int32_t max_wg, int32_t* n_wg, double* tick_khz) {
  if (!e || !stamps || max_wg <= 0) return fail(F5H_EINVAL, "null engine / buffer");
  std::lock_guard<std::mutex> g(e->pm);
  HIPCK(hipSetDevice(e->dev));
  HIPCK(hipDeviceSynchronize());
  const int n = std::min<int>(max_wg, kTimelineWG);
  HIPCK(hipMemcpy(stamps, e->ptl, (size_t)n * 4 * sizeof(unsigned long long), hipMemcpyDeviceToHost));
  int last = 0;
  for (int i = 0; i < n; ++i)
    if (stamps[4 * i]) last = i + 1;
  if (n_wg) *n_wg = last;
  if (tick_khz) *tick_khz = e->wall_khz;
  return 0;
}

int f5h_probe_read(f5h_engine* e, int64_t* launches, double* total_ms) {
  if (!e) return fail(F5H_EINVAL, "null engine");
  std::lock_guard<std::mutex> g(e->pm);
  double ms = 0.0;
  int64_t n = 0;
  if (e->pstamp && e->wall_khz > 0.0) {
    HIPCK(hipSetDevice(e->dev));
    HIPCK(hipDeviceSynchronize());
    std::vector<unsigned long long> h(2 * (size_t)kProbeEnd);
    HIPCK(hipMemcpy(h.data(), e->pslots, h.size() * sizeof(unsigned long long), hipMemcpyDeviceToHost));
    unsigned long long ticks = 0;
    for (int64_t i = 0; i < kProbeEnd; i += (int64_t)kProbeLanes * kProbeStride) {  // one (site, tick)
      unsigned long long t0 = ~0ull, t1 = 0;
      for (int l = 0; l < kProbeLanes; ++l) {
        t0 = std::min(t0, h[i + l * kProbeStride]);
        t1 = std::max(t1, h[kProbeEnd + i + l * kProbeStride]);
      }
      if (t1 == 0 || t0 == ~0ull || t1 < t0) continue;  // no finished launch at this site and tick
      ticks += t1 - t0;
      ++n;
    }
    ms = (double)ticks / e->wall_khz;
  }
  if (launches) *launches = n;
  if (total_ms) *total_ms = ms;
  return 0;
}

int f5h_set_graph_mode(f5h_engine* e, int32_t mode) {
  if (!e) return fail(F5H_EINVAL, "null engine");
  if (mode != 0 && mode != 1) return fail(F5H_EINVAL, "graph mode must be 0 (eager) or 1 (step graph)");
  std::lock_guard<std::mutex> g(e->gm);
  e->graph_mode = mode;
  return 0;
}

int f5h_set_cfg_streams(f5h_engine* e, int32_t n) {
  if (!e) return fail(F5H_EINVAL, "null engine");
  if (n < 0 || n > 2) return fail(F5H_EINVAL, "cfg streams must be 0 (auto), 1 or 2");
  std::lock_guard<std::mutex> g(e->gm);
  e->split_cfg = n == 0 ? 2 : (n == 2 ? 1 : 0);
  return 0;
}

int f5h_set_pad_skip(f5h_engine* e, int32_t enable) {
  if (!e) return fail(F5H_EINVAL, "null engine");
  if (enable != 0 && enable != 1) return fail(F5H_EINVAL, "pad skip must be 0 or 1");
  std::lock_guard<std::mutex> g(e->gm);
  e->pad_skip = enable;
  return 0;
}

int f5h_set_chain(f5h_engine* e, int32_t enable) {
  if (!e) return fail(F5H_EINVAL, "null engine");
  if (enable != 0 && enable != 1) return fail(F5H_EINVAL, "chain must be 0 or 1");
  std::lock_guard<std::mutex> g(e->gm);
  e->chain = enable;
  return 0;
}

int f5h_chain_stats(f5h_engine* e, int64_t* launches, int32_t* fault, int64_t* refused) {
  if (!e) return fail(F5H_EINVAL, "null engine");
  if (launches) *launches = e->n_chain.load(std::memory_order_relaxed);
  if (refused) *refused = g_gate_refused.load(std::memory_order_relaxed);
  if (fault) {
    *fault = 0;
    if (e->chain_fault) {  // the caller has synchronised with the engine's calls (the device word is final)
      unsigned v = 0;
      HIPCK(hipSetDevice(e->dev));
      HIPCK(hipMemcpyAsync(&v, e->chain_fault, sizeof(v), hipMemcpyDeviceToHost, e->mstream));
      HIPCK(hipStreamSynchronize(e->mstream));
      *fault = v ? 1 : 0;
    }
  }
  return 0;
}

int f5h_set_ln_fold(f5h_engine* e, int32_t enable) {
  if (!e) return fail(F5H_EINVAL, "null engine");
  if (enable != 0 && enable != 1) return fail(F5H_EINVAL, "ln fold must be 0 or 1");
  std::lock_guard<std::mutex> g(e->gm);
  e->lnfold = enable;
  return 0;
}

int f5h_ln_fold_stats(f5h_engine* e, int32_t* supported, int64_t* passes) {
  if (!e) return fail(F5H_EINVAL, "null engine");
  if (supported) *supported = (e->lnf_ok || e->rmsf_ok) ? 1 : 0;
  if (passes) *passes = e->n_lnfold.load(std::memory_order_relaxed);
  return 0;
}

int f5h_set_store_policy(f5h_engine* e, int32_t mode) {
  if (!e) return fail(F5H_EINVAL, "null engine");
  if (mode != -1 && mode != 0 && mode != 1 && (mode < 0x100 || mode > 0x11F))
    return fail(F5H_EINVAL, "store policy must be -1 (auto), 0 (plain), 1 (write-through) or 0x100 | class mask");
  std::lock_guard<std::mutex> g(e->gm);
  e->store_policy = mode;  // part of the step graph's key: a cached graph of another policy is not replayed
  return 0;
}

int f5h_store_policy_stats(f5h_engine* e, int64_t* write_through, int64_t* plain) {
  if (!e) return fail(F5H_EINVAL, "null engine");
  if (write_through) *write_through = e->n_store_wt.load(std::memory_order_relaxed);
  if (plain) *plain = e->n_store_plain.load(std::memory_order_relaxed);
  return 0;
}

int f5h_store_policy_force(int32_t mode) {
  if (mode < -1 || mode > 1) return fail(F5H_EINVAL, "forced store policy must be -1 (off), 0 (plain) or 1 (write-through)");
  store_policy_force(mode);
  g_kernel_epoch.fetch_add(1);  // captured graphs hold the old kernel choice
  return 0;
}

int f5h_last_call_host_ms(f5h_engine* e, double* ms, int32_t n) {
  if (!e || !ms || n <= 0) return fail(F5H_EINVAL, "null engine / buffer");
  std::lock_guard<std::mutex> g(e->hm);
  for (int i = 0; i < n; ++i) ms[i] = i < kHostPhases ? e->last_host[i] : 0.0;
  return 0;
}

int f5h_chain_debug_spin_limit(int64_t limit) {
  chain_set_spin_limit(limit);
  g_kernel_epoch.fetch_add(1);  // captured graphs hold the old kernel arguments
  return 0;
}

int f5h_graph_stats(f5h_engine* e, int64_t* captures, int64_t* replays, int32_t* cached) {
  if (!e) return fail(F5H_EINVAL, "null engine");
  std::lock_guard<std::mutex> g(e->gm);
  if (captures) *captures = e->n_captures;
  if (replays) *replays = e->n_replays;
  if (cached) *cached = (int32_t)e->graphs.size();
  return 0;
}

// ---------------------------------------------------------------- op-level entry points
int f5h_op_linear(void* stream, int32_t compute, int32_t M, int32_t N, int32_t K, const float* A, const float* W,
                  const float* bias, float* C, void* workspace, size_t workspace_bytes) {
  if (M <= 0 || N <= 0 || K <= 0 || K % 64) return fail(F5H_EINVAL, "op_linear needs K % 64 == 0");
  if (compute < F5H_FP32 || compute > F5H_FP16) return fail(F5H_EINVAL, "bad compute mode");
  const int Npad = (N + 127) / 128 * 128;
  const size_t es = compute ? 2 : 4;
  const size_t need = (size_t)Npad * K * es;
  if (workspace_bytes < (need + 255) / 256 * 256 + (size_t)M * K * es)
    return fail(F5H_ENOMEM, "workspace too small for op_linear");
  hipStream_t st = reinterpret_cast<hipStream_t>(stream);
  HIPCK(hipMemsetAsync(workspace, 0, need, st));
  HIPCK(f32_to_op(compute, W, (int64_t)N * K, workspace, st));
  const void* Aop = A;
  if (compute) {
    char* ab = reinterpret_cast<char*>(workspace) + (need + 255) / 256 * 256;
    HIPCK(f32_to_op(compute, A, (int64_t)M * K, ab, st));
    Aop = ab;
  }
  GemmArgs g{};
  g.A = Aop;
  g.lda = K;
  g.W = workspace;
  g.ldw = K;
  g.M = M;
  g.N = N;
  g.K = K;
  g.bias = bias;
  g.C = C;
  g.ldc = N;
  HIPCK(gemm(compute, EPI_STORE, g, st));
  return 0;
}

int f5h_gemm_force_config(int32_t cfg) {
  if (cfg != -1 && cfg != 0 && cfg != 1 && cfg != 5 && cfg != 11 && cfg != 12 && cfg != 13)
    return fail(F5H_EINVAL, "gemm config must be -1, 0, 1, 5, 11, 12 or 13");
  gemm_force_config(cfg);
  g_kernel_epoch.fetch_add(1);
  return 0;
}

int f5h_attn_force_safe(int32_t on) {
  attention_force_safe(on);
  g_kernel_epoch.fetch_add(1);  // captured graphs hold the old kernel arguments
  return 0;
}

int f5h_debug_tile_live(const int32_t* live_len, int32_t live_seq, int32_t M, int32_t m0, int32_t BM) {
  if (live_seq <= 0 || M <= 0 || BM <= 0 || m0 < 0 || m0 >= M) return fail(F5H_EINVAL, "bad tile");
  return tile_live_rows(live_len, live_seq, M, m0, BM) ? 1 : 0;
}

static int op_attention_impl(void* stream, int32_t compute, int32_t S, int32_t H, int32_t N, const float* Q,
                             const float* K, const float* V, const int32_t* kv_len, const int32_t* q_len,
                             int32_t q_prescaled, float* O, void* workspace, size_t workspace_bytes,
                             int32_t o_split = 0, float* O2 = nullptr, int32_t kv_start2 = 0,
                             const int32_t* kv_len2 = nullptr) {
  if (S <= 0 || H <= 0 || N <= 0) return fail(F5H_EINVAL, "bad attention shape");
  if (kv_len2 && (kv_start2 < 0 || kv_start2 > N))
    return fail(F5H_EINVAL, "op_attention_ranges: kv_start2 must lie in [0, N]");
  if (o_split < 0 || o_split >= N || (o_split > 0 && !O2))
    return fail(F5H_EINVAL, "op_attention_split: o_split must lie in [0, N) and needs O2");
  if (compute < F5H_FP32 || compute > F5H_FP16) return fail(F5H_EINVAL, "bad compute mode");
  hipStream_t st = reinterpret_cast<hipStream_t>(stream);
  const int64_t n = (int64_t)S * H * N * 64;
  AttnArgs at{};
  at.S = S;
  at.H = H;
  at.L = N;
  at.kv_len = kv_len;
  at.q_len = q_len;
  at.prescaled = q_prescaled ? 1 : 0;
  at.o_split = o_split;
  at.kv_start2 = kv_start2;
  at.kv_len2 = kv_len2;
  const int64_t n1 = o_split ? (int64_t)S * o_split * H * 64 : n;  // elements of the first output
  if (compute) {
    const size_t need = (size_t)n * 2 * 4 + 4 * 256;
    if (workspace_bytes < need) return fail(F5H_ENOMEM, "workspace too small for op_attention");
    char* w = reinterpret_cast<char*>(workspace);
    void *q = w, *k = w + n * 2, *v = w + n * 4, *o = w + n * 6;
    HIPCK(f32_to_op(compute, Q, n, q, st));
    HIPCK(f32_to_op(compute, K, n, k, st));
    HIPCK(f32_to_op(compute, V, n, v, st));
    at.q = q;
    at.k = k;
    at.v = v;
    at.o = o;
    at.o2 = (char*)o + n1 * 2;  // the two 16-bit outputs back to back: n elements in all
    HIPCK(attention(compute, at, st));
    HIPCK(op_to_f32(compute, o, n1, O, st));
    if (o_split) HIPCK(op_to_f32(compute, at.o2, n - n1, O2, st));
  } else {
    at.q = Q;
    at.k = K;
    at.v = V;
    at.o = O;
    at.o2 = O2;
    HIPCK(attention(0, at, st));
  }
  return 0;
}

int f5h_op_attention(void* stream, int32_t compute, int32_t S, int32_t H, int32_t N, const float* Q, const float* K,
                     const float* V, const int32_t* kv_len, int32_t q_prescaled, float* O, void* workspace,
                     size_t workspace_bytes) {
  return op_attention_impl(stream, compute, S, H, N, Q, K, V, kv_len, nullptr, q_prescaled, O, workspace,
                           workspace_bytes);
}

int f5h_op_attention_qlen(void* stream, int32_t compute, int32_t S, int32_t H, int32_t N, const float* Q,
                          const float* K, const float* V, const int32_t* kv_len, const int32_t* q_len,
                          int32_t q_prescaled, float* O, void* workspace, size_t workspace_bytes) {
  return op_attention_impl(stream, compute, S, H, N, Q, K, V, kv_len, q_len, q_prescaled, O, workspace,
                           workspace_bytes);
}

int f5h_op_attention_split(void* stream, int32_t compute, int32_t S, int32_t H, int32_t N, const float* Q,
                           const float* K, const float* V, const int32_t* kv_len, const int32_t* q_len,
                           int32_t q_prescaled, int32_t o_split, float* O, float* O2, void* workspace,
                           size_t workspace_bytes) {
  return op_attention_impl(stream, compute, S, H, N, Q, K, V, kv_len, q_len, q_prescaled, O, workspace,
                           workspace_bytes, o_split, O2);
}

int f5h_op_attention_ranges(void* stream, int32_t compute, int32_t S, int32_t H, int32_t N, const float* Q,
                            const float* K, const float* V, const int32_t* kv_len, int32_t kv_start2,
                            const int32_t* kv_len2, const int32_t* q_len, int32_t q_prescaled, float* O,
                            void* workspace, size_t workspace_bytes) {
  return op_attention_impl(stream, compute, S, H, N, Q, K, V, kv_len, q_len, q_prescaled, O, workspace,
                           workspace_bytes, 0, nullptr, kv_start2, kv_len2);
}

static bool op_compute_ok(int32_t compute) { return compute >= F5H_FP32 && compute <= F5H_FP16; }
// caller workspace as a bump allocator: null when it does not fit (fits() then fails the call)
struct OpWs {
  WS ws;
  size_t bytes;
  OpWs(void* base, size_t n) : bytes(n) { ws.base = reinterpret_cast<char*>(base); }
  void* take(size_t n) { return ws.take<char>(n); }
  bool fits() const { return ws.off == 0 || (ws.base && ws.off <= bytes); }
};
#define OPWS_CHECK(w, what)                                                                       \
  do {                                                                                            \
    if (!(w).fits()) return fail(F5H_ENOMEM, std::string("workspace too small for ") + (what));  \
  } while (0)

// A host segment table off[S + 1] of an op hook: off[0] = 0, every length in [1, Lmax], off[S] = R
static int op_seg_check(const char* what, const int32_t* off, int S, int64_t R, int Lmax) {
  if (!off || S <= 0 || R <= 0 || Lmax <= 0) return fail(F5H_EINVAL, std::string(what) + ": bad segment table");
  if (off[0] != 0 || off[S] != R) return fail(F5H_EINVAL, std::string(what) + ": seg_off must run from 0 to R");
  for (int s = 0; s < S; ++s)
    if (off[s + 1] - off[s] < 1 || off[s + 1] - off[s] > Lmax)
      return fail(F5H_EINVAL, std::string(what) + ": segment " + std::to_string(s) + " is empty or longer than Lmax");
  return 0;
}

int f5h_op_attention_ragged(void* stream, int32_t compute, int32_t S, int32_t H, int32_t Lmax, int32_t R,
                            const int32_t* seg_off, const float* Q, const float* K, const float* V,
                            int32_t q_prescaled, float* O, void* workspace, size_t workspace_bytes) {
  if (!op_compute_ok(compute)) return fail(F5H_EINVAL, "bad compute mode");
  if (S <= 0 || H <= 0 || !Q || !K || !V || !O) return fail(F5H_EINVAL, "op_attention_ragged: bad shape or null tensor");
  RC(op_seg_check("op_attention_ragged", seg_off, S, R, Lmax));
  hipStream_t st = reinterpret_cast<hipStream_t>(stream);
  const int64_t n = (int64_t)S * H * Lmax * 64, no = (int64_t)R * H * 64;
  const size_t es = compute ? 2 : 4;
  OpWs ws(workspace, workspace_bytes);
  int32_t* off = reinterpret_cast<int32_t*>(ws.take((size_t)(S + 1) * 4));
  int32_t* len = reinterpret_cast<int32_t*>(ws.take((size_t)S * 4));
  int2* tab = reinterpret_cast<int2*>(ws.take((size_t)R * 8));
  void* q = compute ? ws.take((size_t)n * es) : nullptr;
  void* k = compute ? ws.take((size_t)n * es) : nullptr;
  void* v = compute ? ws.take((size_t)n * es) : nullptr;
  void* o = compute ? ws.take((size_t)no * es) : nullptr;
  OPWS_CHECK(ws, "op_attention_ragged");
  HIPCK(seg_upload(seg_off, S + 1, off, st));
  HIPCK(build_rowtab(off, S, R, tab, len, st));
  AttnArgs at{};
  at.S = S;
  at.H = H;
  at.L = Lmax;
  at.kv_len = at.q_len = len;
  at.prescaled = q_prescaled ? 1 : 0;
  at.o_split = kAttnRagged;
  at.o2 = off;
  at.q = Q;
  at.k = K;
  at.v = V;
  at.o = O;
  if (compute) {
    HIPCK(f32_to_op(compute, Q, n, q, st));
    HIPCK(f32_to_op(compute, K, n, k, st));
    HIPCK(f32_to_op(compute, V, n, v, st));
    HIPCK(f32_to_op(compute, O, no, o, st));
    at.q = q;
    at.k = k;
    at.v = v;
    at.o = o;
  }
  HIPCK(attention(compute, at, st));
  if (compute) HIPCK(op_to_f32(compute, o, no, O, st));
  return 0;
}

int f5h_op_conv_pos_ragged(void* stream, int32_t compute, int32_t S, int32_t Lmax, int32_t R, int32_t d,
                           const int32_t* seg_off, const float* x, const float* w, const float* bias, int32_t mode,
                           const float* resid, int32_t x_as_f32, float* y, void* workspace, size_t workspace_bytes) {
  if (!op_compute_ok(compute)) return fail(F5H_EINVAL, "bad compute mode");
  if (d <= 0 || d % 128 || d > 1024) return fail(F5H_EINVAL, "op_conv_pos_ragged needs d % 128 == 0 and d <= 1024");
  if (mode < 0 || mode > 2 || (mode == 2 && !compute)) return fail(F5H_EINVAL, "op_conv_pos_ragged: bad mode");
  if (!x || !w || !bias || !y || (mode != 0 && !resid)) return fail(F5H_EINVAL, "op_conv_pos_ragged: null tensor");
  RC(op_seg_check("op_conv_pos_ragged", seg_off, S, R, Lmax));
  if ((int64_t)R * d >= (int64_t)1 << 31) return fail(F5H_EINVAL, "op_conv_pos_ragged: R * d must stay below 2^31");
  hipStream_t st = reinterpret_cast<hipStream_t>(stream);
  const size_t es = compute ? 2 : 4;
  const int64_t nx = (int64_t)R * d;
  OpWs ws(workspace, workspace_bytes);
  void* wp = ws.take(kConvPackElems * es);
  int32_t* off = reinterpret_cast<int32_t*>(ws.take((size_t)(S + 1) * 4));
  void* xop = (compute && !x_as_f32) ? ws.take((size_t)nx * es) : nullptr;
  const bool y16 = compute && mode != 1;
  void* yop = y16 ? ws.take((size_t)nx * es) : nullptr;
  OPWS_CHECK(ws, "op_conv_pos_ragged");
  HIPCK(hipMemsetAsync(wp, 0, kConvPackElems * es, st));
  RC(pack_conv_weight(w, F5H_DT_F32, d, wp, compute, st));
  HIPCK(seg_upload(seg_off, S + 1, off, st));
  ConvArgs cv{};
  cv.S = S;
  cv.L = Lmax;
  cv.d = d;
  cv.ragged = 1;
  cv.rowkeep = reinterpret_cast<const uint8_t*>(off);
  cv.x = x;
  cv.x_f32 = 1;
  if (xop) {
    HIPCK(f32_to_op(compute, x, nx, xop, st));
    cv.x = xop;
    cv.x_f32 = 0;
  }
  cv.w = wp;
  cv.bias = bias;
  cv.mode = mode;
  cv.y = y;
  if (yop) {
    HIPCK(f32_to_op(compute, y, nx, yop, st));
    cv.y = yop;
  }
  cv.resid = resid;
  HIPCK(conv_pos(compute, cv, st));
  if (yop) HIPCK(op_to_f32(compute, yop, nx, y, st));
  return 0;
}

int f5h_op_grn_ragged(void* stream, int32_t compute, int32_t S, int32_t Lmax, int32_t R, int32_t C,
                      const int32_t* seg_off, const float* x, const float* gamma, const float* beta, float* out,
                      void* workspace, size_t workspace_bytes) {
  if (!op_compute_ok(compute)) return fail(F5H_EINVAL, "bad compute mode");
  if (C <= 0 || !x || !gamma || !beta || !out) return fail(F5H_EINVAL, "op_grn_ragged: bad shape or null tensor");
  RC(op_seg_check("op_grn_ragged", seg_off, S, R, Lmax));
  if (S > 65535 || (Lmax + 63) / 64 > 65535) return fail(F5H_EINVAL, "op_grn_ragged: S and Lmax / 64 are grid dimensions");
  hipStream_t st = reinterpret_cast<hipStream_t>(stream);
  const int64_t n = (int64_t)R * C;
  OpWs ws(workspace, workspace_bytes);
  int32_t* off = reinterpret_cast<int32_t*>(ws.take((size_t)(S + 1) * 4));
  float* scratch = reinterpret_cast<float*>(ws.take(((size_t)(Lmax + 63) / 64 + 1) * S * C * sizeof(float)));
  void* oop = compute ? ws.take((size_t)n * 2) : nullptr;
  OPWS_CHECK(ws, "op_grn_ragged");
  HIPCK(seg_upload(seg_off, S + 1, off, st));
  HIPCK(grn_ragged(compute, x, off, S, R, Lmax, C, gamma, beta, scratch, oop ? oop : (void*)out, st));
  if (oop) HIPCK(op_to_f32(compute, oop, n, out, st));
  return 0;
}

// ---- op-level entry points of the conv / norm / GEMM-epilogue kernels (tests/test_gpu_ops.py). Each validates
// its shapes on the host (F5H_EINVAL, nothing enqueued), stages the operand-dtype buffers the kernel's contract
// asks for in the caller's workspace (f32_to_op / op_to_f32), calls the production launcher unchanged and
// returns fp32. A buffer the kernel writes in the operand dtype starts as the rounded copy of the caller's
// fp32 buffer, so elements the kernel leaves alone come back as they went in.

int f5h_op_conv_pos(void* stream, int32_t compute, int32_t S, int32_t L, int32_t d, const float* x, const float* w,
                    const float* bias, const uint8_t* rowkeep, int32_t mode, const float* resid, int32_t x_as_f32,
                    int64_t y_seq_stride, int64_t y_row_off, float* y, void* workspace, size_t workspace_bytes) {
  if (!op_compute_ok(compute)) return fail(F5H_EINVAL, "bad compute mode");
  if (S <= 0 || L <= 0 || d <= 0) return fail(F5H_EINVAL, "op_conv_pos: bad shape");
  if (d % 128 || d > 1024) return fail(F5H_EINVAL, "op_conv_pos needs d % 128 == 0 and d <= 1024");
  if ((int64_t)S * L * d >= (int64_t)1 << 31) return fail(F5H_EINVAL, "op_conv_pos: S * L * d must stay below 2^31");
  if (mode < 0 || mode > 2) return fail(F5H_EINVAL, "op_conv_pos: mode must be 0, 1 or 2");
  if (mode == 2 && !compute) return fail(F5H_EINVAL, "op_conv_pos: mode 2 writes the 16-bit residual stream");
  if (!x || !w || !bias || !y) return fail(F5H_EINVAL, "op_conv_pos: null tensor");
  if (mode != 0 && !resid) return fail(F5H_EINVAL, "op_conv_pos: modes 1 and 2 add a residual");
  // mode 0 writes a dense [S, L, d] (the kernel ignores the row placement there)
  if (mode == 0 && (y_row_off != 0 || y_seq_stride != L))
    return fail(F5H_EINVAL, "op_conv_pos: mode 0 takes y_row_off 0 and y_seq_stride L");
  if (y_row_off < 0 || y_seq_stride < y_row_off + L) return fail(F5H_EINVAL, "op_conv_pos: rows outside y");
  hipStream_t st = reinterpret_cast<hipStream_t>(stream);
  const size_t es = compute ? 2 : 4;
  const int64_t nx = (int64_t)S * L * d, ny = (int64_t)S * y_seq_stride * d;
  OpWs ws(workspace, workspace_bytes);
  void* wp = ws.take(kConvPackElems * es);
  void* xop = (compute && !x_as_f32) ? ws.take((size_t)nx * es) : nullptr;
  const bool y16 = compute && mode != 1;
  void* yop = y16 ? ws.take((size_t)ny * es) : nullptr;
  OPWS_CHECK(ws, "op_conv_pos");
  HIPCK(hipMemsetAsync(wp, 0, kConvPackElems * es, st));
  RC(pack_conv_weight(w, F5H_DT_F32, d, wp, compute, st));
  ConvArgs cv{};
  cv.S = S;
  cv.L = L;
  cv.d = d;
  cv.x = x;
  cv.x_f32 = 1;
  if (xop) {
    HIPCK(f32_to_op(compute, x, nx, xop, st));
    cv.x = xop;
    cv.x_f32 = 0;
  }
  cv.w = wp;
  cv.bias = bias;
  cv.rowkeep = rowkeep;
  cv.mode = mode;
  cv.y = y;
  if (yop) {
    HIPCK(f32_to_op(compute, y, ny, yop, st));
    cv.y = yop;
  }
  cv.y_seq_stride = y_seq_stride;
  cv.y_row_off = y_row_off;
  cv.resid = resid;
  HIPCK(conv_pos(compute, cv, st));
  if (yop) HIPCK(op_to_f32(compute, yop, ny, y, st));
  return 0;
}

int f5h_op_norm(void* stream, int32_t compute, int32_t kind, int32_t h16, int32_t M, int32_t d, const float* h,
                const float* shift_or_g, const float* scale, float* out, void* workspace, size_t workspace_bytes) {
  if (!op_compute_ok(compute)) return fail(F5H_EINVAL, "bad compute mode");
  if (kind != 0 && kind != 1) return fail(F5H_EINVAL, "op_norm: kind must be 0 (LayerNorm-modulate) or 1 (RMSNorm)");
  if (M <= 0 || d <= 0) return fail(F5H_EINVAL, "op_norm: bad shape");
  if (d % 4 || d > 2048) return fail(F5H_EINVAL, "op_norm needs d % 4 == 0 and d <= 2048");
  if (h16 && !compute) return fail(F5H_EINVAL, "op_norm: a 16-bit h needs a 16-bit compute mode");
  if (!h || !shift_or_g || !out || (kind == 0 && !scale)) return fail(F5H_EINVAL, "op_norm: null tensor");
  hipStream_t st = reinterpret_cast<hipStream_t>(stream);
  const int64_t n = (int64_t)M * d;
  OpWs ws(workspace, workspace_bytes);
  void* hop = h16 ? ws.take((size_t)n * 2) : nullptr;
  void* oop = compute ? ws.take((size_t)n * 2) : nullptr;
  OPWS_CHECK(ws, "op_norm");
  const void* hin = h;
  if (hop) {
    HIPCK(f32_to_op(compute, h, n, hop, st));
    hin = hop;
  }
  void* o = oop ? oop : (void*)out;
  if (kind == 0)
    HIPCK(ln_modulate(compute, hin, h16 ? 1 : 0, M, d, shift_or_g, scale, o, st));
  else
    HIPCK(rms_norm_g(compute, hin, h16 ? 1 : 0, M, d, shift_or_g, o, st));
  if (oop) HIPCK(op_to_f32(compute, oop, n, out, st));
  return 0;
}

static int op_dwconv_ln_impl(void* stream, int32_t compute, int32_t S, int32_t L, int32_t C, const float* x,
                             const float* dw_w, const float* dw_b, const float* ln_w, const float* ln_b,
                             const int32_t* len, float* out, void* workspace, size_t workspace_bytes) {
  if (!op_compute_ok(compute)) return fail(F5H_EINVAL, "bad compute mode");
  if (S <= 0 || L <= 0 || C <= 0) return fail(F5H_EINVAL, "op_dwconv_ln: bad shape");
  if (C > 1024) return fail(F5H_EINVAL, "op_dwconv_ln needs C <= 1024");
  if ((int64_t)S * L >= (int64_t)1 << 30) return fail(F5H_EINVAL, "op_dwconv_ln: too many rows");
  if (!x || !dw_w || !dw_b || !ln_w || !ln_b || !out) return fail(F5H_EINVAL, "op_dwconv_ln: null tensor");
  hipStream_t st = reinterpret_cast<hipStream_t>(stream);
  const int64_t n = (int64_t)S * L * C;
  OpWs ws(workspace, workspace_bytes);
  void* oop = compute ? ws.take((size_t)n * 2) : nullptr;
  OPWS_CHECK(ws, "op_dwconv_ln");
  HIPCK(dwconv_ln(compute, x, S, L, C, dw_w, dw_b, ln_w, ln_b, oop ? oop : (void*)out, st, len, S));
  if (oop) HIPCK(op_to_f32(compute, oop, n, out, st));
  return 0;
}
int f5h_op_dwconv_ln(void* stream, int32_t compute, int32_t S, int32_t L, int32_t C, const float* x,
                     const float* dw_w, const float* dw_b, const float* ln_w, const float* ln_b, float* out,
                     void* workspace, size_t workspace_bytes) {
  return op_dwconv_ln_impl(stream, compute, S, L, C, x, dw_w, dw_b, ln_w, ln_b, nullptr, out, workspace,
                           workspace_bytes);
}
int f5h_op_dwconv_ln_len(void* stream, int32_t compute, int32_t S, int32_t L, int32_t C, const float* x,
                         const float* dw_w, const float* dw_b, const float* ln_w, const float* ln_b,
                         const int32_t* len, float* out, void* workspace, size_t workspace_bytes) {
  return op_dwconv_ln_impl(stream, compute, S, L, C, x, dw_w, dw_b, ln_w, ln_b, len, out, workspace,
                           workspace_bytes);
}

static int op_grn_impl(void* stream, int32_t compute, int32_t S, int32_t L, int32_t C, const float* x,
                       const float* gamma, const float* beta, const int32_t* len, float* out, void* workspace,
                       size_t workspace_bytes) {
  if (!op_compute_ok(compute)) return fail(F5H_EINVAL, "bad compute mode");
  if (S <= 0 || L <= 0 || C <= 0) return fail(F5H_EINVAL, "op_grn: bad shape");
  if (S > 65535 || (L + 63) / 64 > 65535) return fail(F5H_EINVAL, "op_grn: S and L / 64 are grid dimensions");
  if (!x || !gamma || !beta || !out) return fail(F5H_EINVAL, "op_grn: null tensor");
  hipStream_t st = reinterpret_cast<hipStream_t>(stream);
  const int64_t n = (int64_t)S * L * C;
  OpWs ws(workspace, workspace_bytes);
  float* scratch = reinterpret_cast<float*>(ws.take(((size_t)(L + 63) / 64 + 1) * S * C * sizeof(float)));
  void* oop = compute ? ws.take((size_t)n * 2) : nullptr;
  OPWS_CHECK(ws, "op_grn");
  HIPCK(grn(compute, x, S, L, C, gamma, beta, scratch, oop ? oop : (void*)out, st, len, S));
  if (oop) HIPCK(op_to_f32(compute, oop, n, out, st));
  return 0;
}
int f5h_op_grn(void* stream, int32_t compute, int32_t S, int32_t L, int32_t C, const float* x, const float* gamma,
               const float* beta, float* out, void* workspace, size_t workspace_bytes) {
  return op_grn_impl(stream, compute, S, L, C, x, gamma, beta, nullptr, out, workspace, workspace_bytes);
}
int f5h_op_grn_len(void* stream, int32_t compute, int32_t S, int32_t L, int32_t C, const float* x, const float* gamma,
                   const float* beta, const int32_t* len, float* out, void* workspace, size_t workspace_bytes) {
  return op_grn_impl(stream, compute, S, L, C, x, gamma, beta, len, out, workspace, workspace_bytes);
}

int f5h_op_gemm_epi(void* stream, const f5h_op_gemm_args* a, void* workspace, size_t workspace_bytes) {
  if (!a) return fail(F5H_EINVAL, "op_gemm_epi: null args");
  const int compute = a->compute, epi = a->epi, M = a->M, N = a->N, K = a->K;
  if (!op_compute_ok(compute)) return fail(F5H_EINVAL, "bad compute mode");
  if (epi < EPI_STORE || epi > EPI_STORE16) return fail(F5H_EINVAL, "op_gemm_epi: unknown epilogue");
  if (M <= 0 || N <= 0 || K <= 0) return fail(F5H_EINVAL, "op_gemm_epi: bad shape");
  if (K % 64) return fail(F5H_EINVAL, "op_gemm_epi needs K % 64 == 0");
  if (!a->A || !a->W) return fail(F5H_EINVAL, "op_gemm_epi: null operand");
  if (a->A2 && (a->k_split <= 0 || a->k_split % 64 || a->k_split >= K))
    return fail(F5H_EINVAL, "op_gemm_epi: k_split must be a multiple of 64 inside (0, K)");
  const bool resid_epi = epi == EPI_RESID || epi == EPI_RESID16;
  const bool inout = resid_epi || epi == EPI_RESID_FILL;
  if (a->resid && !resid_epi) return fail(F5H_EINVAL, "op_gemm_epi: resid goes with EPI_RESID / EPI_RESID16");
  if (a->gate && !resid_epi) return fail(F5H_EINVAL, "op_gemm_epi: gate goes with EPI_RESID / EPI_RESID16");
  if (a->rowkeep && !inout) return fail(F5H_EINVAL, "op_gemm_epi: rowkeep goes with the in/out epilogues");
  if (a->live_len) {
    // the pad-row skip: in place only (a skipped tile leaves C as it was), rows described by rowkeep as well
    if (!resid_epi || a->resid || !a->rowkeep || a->live_seq <= 0 || M % a->live_seq)
      return fail(F5H_EINVAL, "op_gemm_epi: live_len needs an in-place EPI_RESID(16) with rowkeep and M % live_seq == 0");
  }
  int64_t dual = 0;
  if (epi == EPI_INPROJ) {
    if (N % 8 || !a->add || a->ld_add < N || a->ld_add % 8 || a->dual_rows < 0 || a->bias)
      return fail(F5H_EINVAL, "op_gemm_epi: EPI_INPROJ needs N % 8 == 0, an addend with ld_add % 8 == 0 and no bias");
    dual = a->dual_rows;
    if (dual != 0 && dual < M) return fail(F5H_EINVAL, "op_gemm_epi: dual_rows must be 0 or >= M");
  } else if (a->add || a->dual_rows) {
    return fail(F5H_EINVAL, "op_gemm_epi: add / dual_rows go with EPI_INPROJ");
  }
  int inner = 0;
  const bool rq = a->seg_off != nullptr;  // ragged QKV rows (packed sequences into padded panels)
  if (rq) {
    if (epi != EPI_QKV) return fail(F5H_EINVAL, "op_gemm_epi: seg_off goes with EPI_QKV");
    if (a->qkv_dst_len <= 0 || a->seq_len != a->qkv_dst_len || a->ln_part_in)
      return fail(F5H_EINVAL, "op_gemm_epi: ragged EPI_QKV needs seq_len == qkv_dst_len > 0 and no fold consumer");
    RC(op_seg_check("op_gemm_epi", a->seg_off, a->n_seq, M, a->qkv_dst_len));
  }
  if (epi == EPI_QKV) {
    inner = a->heads * 64;
    if (a->heads <= 0 || N != 3 * inner || a->seq_len <= 0 || (!rq && M % a->seq_len) || a->rope_heads < 0 ||
        a->rope_heads > a->heads || !a->q || !a->k || !a->v)
      return fail(F5H_EINVAL, "op_gemm_epi: EPI_QKV needs N == 3 * heads * 64, M % seq_len == 0 and q, k, v");
    if (a->qkv_dst_len != 0 && (a->qkv_dst_len < a->seq_len || a->ln_part_in))
      return fail(F5H_EINVAL, "op_gemm_epi: qkv_dst_len must be 0 or >= seq_len, and takes no fold consumer");
  } else if (a->qkv_dst_len) {
    return fail(F5H_EINVAL, "op_gemm_epi: qkv_dst_len goes with EPI_QKV");
  } else if (!a->C) {
    return fail(F5H_EINVAL, "op_gemm_epi: null C");
  }
  if (a->q_norm_w || a->k_norm_w) {
    if (epi != EPI_QKV) return fail(F5H_EINVAL, "op_gemm_epi: q_norm_w / k_norm_w go with EPI_QKV");
    if (!a->q_norm_w || !a->k_norm_w) return fail(F5H_EINVAL, "op_gemm_epi: qk_norm needs q_norm_w and k_norm_w");
    if (!(a->qk_norm_eps >= 0.f)) return fail(F5H_EINVAL, "op_gemm_epi: qk_norm_eps must be >= 0");
  }
  // LayerNorm / RMSNorm fold forms: launch_t's contract (gemm_impl.h), refused here with a message
  const bool fold_prod = a->ln_part_out != nullptr, fold_cons = a->ln_part_in != nullptr;
  const bool fold = fold_prod || fold_cons || a->hs_scale || a->hs_out || a->ln_u || a->ln_v || a->ln_rms || a->ln_nparts;
  if (fold) {
    if (!compute) return fail(F5H_EINVAL, "op_gemm_epi: the fold forms need a 16-bit compute mode");
    if (fold_prod && fold_cons)
      return fail(F5H_EINVAL, "op_gemm_epi: fold producer (ln_part_out) and consumer (ln_part_in) fields together");
    if (!fold_prod && !fold_cons)
      return fail(F5H_EINVAL, "op_gemm_epi: fold fields without ln_part_out or ln_part_in");
    if (a->ln_rms != 0 && a->ln_rms != 1) return fail(F5H_EINVAL, "op_gemm_epi: ln_rms must be 0 or 1");
    if (a->ln_nparts < 1 || a->ln_nparts > 16)
      return fail(F5H_EINVAL, "op_gemm_epi: ln_nparts must be 1..16");
    if (N % 128) return fail(F5H_EINVAL, "op_gemm_epi: the fold forms need N % 128 == 0");
    if (a->live_len) return fail(F5H_EINVAL, "op_gemm_epi: the fold forms take no live_len");
    if (a->rowkeep && !a->ln_rms) return fail(F5H_EINVAL, "op_gemm_epi: rowkeep only with the ln_rms fold form");
    if (a->A2) return fail(F5H_EINVAL, "op_gemm_epi: the fold forms take no A2");
    if (fold_prod) {
      if (epi != EPI_RESID16) return fail(F5H_EINVAL, "op_gemm_epi: the fold producer is EPI_RESID16");
      if (a->ln_nparts != N / 64) return fail(F5H_EINVAL, "op_gemm_epi: producer ln_nparts must be N / 64");
      if (a->ln_u || a->ln_v) return fail(F5H_EINVAL, "op_gemm_epi: ln_u / ln_v go with the fold consumer");
      if (a->ln_rms ? (a->hs_scale || a->hs_out) : (!a->hs_scale || !a->hs_out))
        return fail(F5H_EINVAL, "op_gemm_epi: the LayerNorm producer needs hs_scale and hs_out, the ln_rms form neither");
    } else {
      if (epi != EPI_GELU_TANH && epi != EPI_QKV)
        return fail(F5H_EINVAL, "op_gemm_epi: the fold consumer is EPI_GELU_TANH or EPI_QKV");
      if (a->ln_nparts != K / 64) return fail(F5H_EINVAL, "op_gemm_epi: consumer ln_nparts must be K / 64");
      if (a->hs_scale || a->hs_out) return fail(F5H_EINVAL, "op_gemm_epi: hs_scale / hs_out go with the fold producer");
      if (a->ln_rms ? (a->ln_u || a->ln_v) : (!a->ln_u || !a->ln_v))
        return fail(F5H_EINVAL, "op_gemm_epi: the LayerNorm consumer needs ln_u and ln_v, the ln_rms form neither");
    }
  }
  hipStream_t st = reinterpret_cast<hipStream_t>(stream);
  const size_t es = compute ? 2 : 4;
  const int Npad = (N + 127) / 128 * 128;
  // output element type: the operand dtype for these, fp32 otherwise
  const bool out_op = epi == EPI_GELU_TANH || epi == EPI_GELU_ERF_OP || epi == EPI_RESID16 || epi == EPI_STORE16;
  const int64_t nC = (int64_t)(M + dual) * N, nA = (int64_t)M * K;
  // q / k / v elements the launch may address: M * inner, or with qkv_dst_len up to the end of its last panel's rows
  int64_t nqkv = (int64_t)M * inner;
  if (epi == EPI_QKV && a->qkv_dst_len) {
    GemmArgs t{};
    t.M = M;
    t.heads = a->heads;
    t.seq_len = a->seq_len;
    t.qkv_dst_len = a->qkv_dst_len;
    nqkv = (int64_t)qkv_dst_elems(t, M / a->seq_len);
  }
  if (rq) nqkv = (int64_t)a->n_seq * a->heads * a->qkv_dst_len * 64;
  OpWs ws(workspace, workspace_bytes);
  void* wop = ws.take((size_t)Npad * K * es);
  void* aop = compute ? ws.take((size_t)nA * es) : nullptr;
  void* a2op = (compute && a->A2) ? ws.take((size_t)nA * es) : nullptr;
  void* cop = (compute && out_op) ? ws.take((size_t)nC * es) : nullptr;
  void* rop = (compute && epi == EPI_RESID16 && a->resid) ? ws.take((size_t)nC * es) : nullptr;
  // fold producer outputs, each with F5H_OP_GUARD_ROWS rows past M that the launch must leave alone
  const size_t hs_live = (size_t)M * N * 2, hs_all = (size_t)(M + F5H_OP_GUARD_ROWS) * N * 2;
  const size_t lp_live = (size_t)M * a->ln_nparts * 8, lp_all = (size_t)(M + F5H_OP_GUARD_ROWS) * a->ln_nparts * 8;
  void* hsop = a->hs_out ? ws.take(hs_all) : nullptr;
  void *qop = nullptr, *kop = nullptr, *vop = nullptr;
  float2* rope = nullptr;
  if (epi == EPI_QKV) {
    rope = reinterpret_cast<float2*>(ws.take((size_t)a->seq_len * 32 * sizeof(float2)));
    if (compute) {
      qop = ws.take((size_t)nqkv * es);
      kop = ws.take((size_t)nqkv * es);
      vop = ws.take((size_t)nqkv * es);
    }
  }
  int32_t* rq_off = rq ? reinterpret_cast<int32_t*>(ws.take((size_t)(a->n_seq + 1) * 4)) : nullptr;
  int2* rq_tab = rq ? reinterpret_cast<int2*>(ws.take((size_t)M * 8)) : nullptr;
  OPWS_CHECK(ws, "op_gemm_epi");
  HIPCK(hipMemsetAsync(wop, 0, (size_t)Npad * K * es, st));
  HIPCK(f32_to_op(compute, a->W, (int64_t)N * K, wop, st));
  GemmArgs g{};
  g.A = a->A;
  g.A2 = a->A2;
  if (aop) {
    HIPCK(f32_to_op(compute, a->A, nA, aop, st));
    g.A = aop;
  }
  if (a2op) {
    HIPCK(f32_to_op(compute, a->A2, nA, a2op, st));
    g.A2 = a2op;
  }
  g.k_split = a->A2 ? a->k_split : 0;
  g.lda = K;
  g.W = wop;
  g.ldw = K;
  g.M = M;
  g.N = N;
  g.K = K;
  g.bias = a->bias;
  g.C = a->C;
  g.ldc = N;
  g.gate = a->gate;
  g.rowkeep = a->rowkeep;
  g.resid = a->resid;
  g.live_len = a->live_len;
  g.live_seq = a->live_len ? a->live_seq : 0;
  g.add = a->add;
  g.ld_add = a->ld_add;
  g.dual_rows = dual;
  if (rq) {
    HIPCK(seg_upload(a->seg_off, a->n_seq + 1, rq_off, st));
    HIPCK(build_rowtab(rq_off, a->n_seq, M, rq_tab, nullptr, st));
    g.add = reinterpret_cast<const float*>(rq_tab);
  }
  if (cop) {
    // in/out (EPI_RESID16): the rounded C goes in; write-only epilogues overwrite every element
    if (inout) HIPCK(f32_to_op(compute, a->C, nC, cop, st));
    g.C = cop;
  }
  if (rop) {
    HIPCK(f32_to_op(compute, a->resid, nC, rop, st));
    g.resid = rop;
  }
  if (epi == EPI_QKV) {
    HIPCK(rope_table(a->seq_len, rope, st));
    if (a->rope_out)
      HIPCK(hipMemcpyAsync(a->rope_out, rope, (size_t)a->seq_len * 32 * sizeof(float2), hipMemcpyDeviceToDevice, st));
    g.rope = rope;
    g.seq_len = a->seq_len;
    g.heads = a->heads;
    g.rope_heads = a->rope_heads > 0 ? a->rope_heads : a->heads;
    g.q_scale = a->q_scale;
    g.q = compute ? qop : (void*)a->q;
    g.k = compute ? kop : (void*)a->k;
    g.v = compute ? vop : (void*)a->v;
    g.C = nullptr;
    g.ldc = 0;
    g.q_norm_w = a->q_norm_w;
    g.k_norm_w = a->k_norm_w;
    g.qk_norm_eps = a->qk_norm_eps;
    g.qkv_dst_len = a->qkv_dst_len;
    if (a->qkv_dst_len && compute) {  // rows the launch does not own come back as the caller's buffers hold them
      HIPCK(f32_to_op(compute, a->q, nqkv, qop, st));
      HIPCK(f32_to_op(compute, a->k, nqkv, kop, st));
      HIPCK(f32_to_op(compute, a->v, nqkv, vop, st));
    }
  }
  if (fold_prod) {
    // 0xFF bytes: NaN in fp32 and in both 16-bit types. Live rows: NaN with poison, else 0; guard rows: NaN
    const int live_fill = a->poison ? 0xFF : 0;
    HIPCK(hipMemsetAsync(a->ln_part_out, live_fill, lp_live, st));
    HIPCK(hipMemsetAsync(reinterpret_cast<char*>(a->ln_part_out) + lp_live, 0xFF, lp_all - lp_live, st));
    g.ln_part = a->ln_part_out;
    if (hsop) {
      HIPCK(hipMemsetAsync(hsop, live_fill, hs_live, st));
      HIPCK(hipMemsetAsync(reinterpret_cast<char*>(hsop) + hs_live, 0xFF, hs_all - hs_live, st));
      g.hs = hsop;
      g.hs_scale = a->hs_scale;
    }
  }
  if (fold_cons) {
    g.ln_part_in = a->ln_part_in;
    g.ln_u = a->ln_u;
    g.ln_v = a->ln_v;
  }
  if (fold) {
    g.ln_nparts = a->ln_nparts;
    g.ln_rms = a->ln_rms;
    g.ln_eps = a->ln_eps;
  }
  HIPCK(gemm(compute, epi, g, st));
  if (hsop) HIPCK(op_to_f32(compute, hsop, (int64_t)(M + F5H_OP_GUARD_ROWS) * N, a->hs_out, st));
  if (cop) HIPCK(op_to_f32(compute, cop, nC, a->C, st));
  if (epi == EPI_QKV && compute) {
    HIPCK(op_to_f32(compute, qop, nqkv, a->q, st));
    HIPCK(op_to_f32(compute, kop, nqkv, a->k, st));
    HIPCK(op_to_f32(compute, vop, nqkv, a->v, st));
  }
  return 0;
}

int f5h_op_text_upsample(void* stream, int32_t B, int32_t nt, int32_t N, int32_t td, const int64_t* text,
                         const int32_t* seq_len, const float* in, float* out) {
  if (B <= 0 || nt < 0 || N <= 0 || N > 8192 || td <= 0 || td % 4)
    return fail(F5H_EINVAL, "op_text_upsample needs B > 0, nt >= 0, 0 < N <= 8192 and td % 4 == 0");
  if ((nt > 0 && !text) || !in || !out || in == out) return fail(F5H_EINVAL, "op_text_upsample: null or aliased tensor");
  TextUpArgs u{};
  u.text = text;
  u.B = B;
  u.nt = nt;
  u.N = N;
  u.td = td;
  u.seq_len = seq_len;
  u.in_c = in;
  u.out_c = out;
  HIPCK(text_upsample(u, reinterpret_cast<hipStream_t>(stream)));
  return 0;
}

int f5h_op_lnfold_uv(void* stream, int32_t compute, int32_t nfe, int32_t depth, int32_t d, int32_t F, float* table,
                     int64_t stride, int64_t out_off, const float* W1, const float* Wqkv, void* workspace,
                     size_t workspace_bytes) {
  if (compute != F5H_BF16 && compute != F5H_FP16) return fail(F5H_EINVAL, "op_lnfold_uv needs a 16-bit compute mode");
  if (nfe <= 0 || depth <= 0 || d <= 0 || F <= 0 || d % 64 || F % 64)
    return fail(F5H_EINVAL, "op_lnfold_uv needs nfe, depth > 0 and d % 64 == 0, F % 64 == 0");
  const int64_t LW = 2 * (int64_t)F + 6 * (int64_t)d;
  if (stride % 4 || out_off < 6 * (int64_t)d * depth || stride < out_off + depth * LW)
    return fail(F5H_EINVAL, "op_lnfold_uv: stride % 4 == 0, u / v blocks past the modulation rows and inside the row");
  if (!table || !W1 || !Wqkv) return fail(F5H_EINVAL, "op_lnfold_uv: null tensor");
  hipStream_t st = reinterpret_cast<hipStream_t>(stream);
  const int64_t n1 = (int64_t)F * d, nq = 3 * (int64_t)d * d;
  OpWs ws(workspace, workspace_bytes);
  void* w1op = ws.take((size_t)depth * n1 * 2);
  void* wqop = ws.take((size_t)depth * nq * 2);
  const void** ptrs = reinterpret_cast<const void**>(ws.take(2 * (size_t)depth * sizeof(void*)));
  OPWS_CHECK(ws, "op_lnfold_uv");
  HIPCK(f32_to_op(compute, W1, depth * n1, w1op, st));
  HIPCK(f32_to_op(compute, Wqkv, depth * nq, wqop, st));
  std::vector<const void*> host(2 * (size_t)depth);
  for (int l = 0; l < depth; ++l) {
    host[l] = reinterpret_cast<const char*>(w1op) + (size_t)l * n1 * 2;
    host[depth + l] = reinterpret_cast<const char*>(wqop) + (size_t)l * nq * 2;
  }
  HIPCK(hipMemcpyAsync(ptrs, host.data(), host.size() * sizeof(void*), hipMemcpyHostToDevice, st));
  HIPCK(hipStreamSynchronize(st));  // `host` leaves scope
  LnFoldArgs la{};
  la.table = table;
  la.stride = stride;
  la.out_off = out_off;
  la.nfe = nfe;
  la.depth = depth;
  la.d = d;
  la.F = F;
  la.w1 = ptrs;
  la.wqkv = ptrs + depth;
  HIPCK(lnfold_uv(compute, la, st));
  return 0;
}

int f5h_op_scale_cols(void* stream, int32_t compute, int64_t rows, int32_t K, const float* W, const float* g,
                      float* out, void* workspace, size_t workspace_bytes) {
  if (compute != F5H_BF16 && compute != F5H_FP16) return fail(F5H_EINVAL, "op_scale_cols needs a 16-bit compute mode");
  if (rows <= 0 || K <= 0 || K % 8) return fail(F5H_EINVAL, "op_scale_cols needs rows > 0 and K % 8 == 0");
  if (!W || !g || !out) return fail(F5H_EINVAL, "op_scale_cols: null tensor");
  hipStream_t st = reinterpret_cast<hipStream_t>(stream);
  const int64_t n = rows * K;
  OpWs ws(workspace, workspace_bytes);
  void* wop = ws.take((size_t)n * 2);
  void* oop = ws.take((size_t)n * 2);
  OPWS_CHECK(ws, "op_scale_cols");
  HIPCK(f32_to_op(compute, W, n, wop, st));
  HIPCK(scale_cols(compute, wop, rows, K, g, oop, st));
  HIPCK(op_to_f32(compute, oop, n, out, st));
  return 0;
}

}  // extern "C"
