// Internal header of the engine's translation units (not installed, not part of include/f5h.h).
//
// Where things live:
//   engine.cpp        workspace layout, prologue, the layer-op launchers (layer_gemm, launch_attention, input_embed,
//                     adaln_norm / rms_norm, proj_out_tail), the backbones (dit_layer / unett_layer under backbone_part,
//                     backbone_mmdit), the NFE step and loop, call setup (call_begin), graph keys, f5h_sample*,
//                     f5h_workspace_size*, f5h_forward, store_want, ProbeScope
//   engine_modes.cpp  which modes a call runs in: step_modes (pure, the one place a mode is switched on or off),
//                     proc_switches (the process-wide environment diagnostics), f5h_debug_step_modes
//   engine_pack.cpp   weight views and packing (pack_all, pack_mmdit, pack_conv_weight), check_arch,
//                     f5h_engine_create*, f5h_engine_destroy
//   engine_graph.cpp  the hipGraph cache: graph_get, reap_graphs, note_replays, prologue_repeats, g_kernel_epoch
//   engine_chain.cpp  phase-chain bookkeeping: fault slots, ChainGate admission, ChainTicket, chain_fault_*,
//                     f5h_set_chain, f5h_chain_stats, f5h_chain_debug_spin_limit
//   engine_ctl.cpp    the error string (g_err, fail), switches, statistics, probes, f5h_*_force_*
//   engine_ops.cpp    op-level test hooks (f5h_op_*, f5h_debug_*), OpWs, op_seg_check: never on the product path
//   engine_ops_glue.cpp  op-level test hooks of the audio glue, prologue and ODE step kernels (no staging)
// Everything declared here has hidden visibility: libf5h.so exports the C API only.
#pragma once
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
#include <type_traits>
#include <unordered_map>
#include <vector>

#include "../../include/f5h.h"
#include "kernels.h"
#include "reaper.h"

using namespace f5h;

#pragma GCC visibility push(hidden)

// the thread's last error message (f5h_last_error); fail sets it and returns `code`
extern thread_local std::string g_err;
int fail(int code, const std::string& msg);
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

#define KCK(x) HIPCK(x)

struct Lin {
  void* w = nullptr;      // [Npad][K] operand dtype
  float* b = nullptr;     // [Npad] fp32 (may be null)
  int N = 0, K = 0, Npad = 0;
  // F5H_MXFP8 engines, the four per-layer GEMMs' weights: e4m3fn elements [N][K] and E8M0 scales [N][K / 32]
  // (kernels.h 'MXFP8 operands'), quantised from w on the device at creation; w stays
  uint8_t* w8 = nullptr;
  uint8_t* ws = nullptr;
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
constexpr int kMMTextPos = 1024;  // TextEmbedding.precompute_max_pos (mmdit.py:39)

// Key of a cached graph. Fixed-width members ordered so that the struct has no padding: keys are value-initialised
// (GraphKey key{}) and compared as bytes, so a member added here takes part in the comparison by construction.
struct GraphKey {
  const void* ws;
  uint64_t kernel_epoch;  // bumped whenever a forced GEMM config changes
  int32_t kind;  // 0: one NFE step, 1: the call prologue (inputs staged into the workspace), 2: f5h_forward's step
  int32_t B, N, nt, nfe, use_cfg, batch_mask, probe, split, pad_skip, chain, lnfold, store;
  int32_t method;  // f5h_ode_method (nfe counts evaluations = table rows: steps x stages)
  // MMDiT single-branch forward (kind 2): the captured step reads the text stream's start from the conditional or the
  // dropped-text embedding, so drop_text is part of the key (DiT / UNetT: the drop flags act in the prologue only)
  int32_t drop_text;
  // ragged sampling (f5h_sample_ragged; 0 otherwise): utterances and longest utterance. With N = the packed rows R these
  // fix the launch geometry; the lengths themselves live in the workspace's segment tables, not in the key
  int32_t rag_B, rag_L;
  uint32_t cfg_bits;
  // F5H_MXFP8 engines: the classes that run on MXFP8 operands (f5h_set_mx8_classes; 0 otherwise). spare: always 0,
  // keeps the struct free of padding
  int32_t mx8, spare;
};
static_assert(std::has_unique_object_representations_v<GraphKey>, "GraphKey is compared as bytes: no padding");
inline bool operator==(const GraphKey& a, const GraphKey& b) { return std::memcmp(&a, &b, sizeof(GraphKey)) == 0; }

struct f5h_engine {
  f5h_arch a{};
  int dev = 0;
  int bf = 0;          // compute mode (f5h_compute == ComputeMode): 0 fp32, 1 bf16, 2 fp16 operands
  // F5H_MXFP8 (DESIGN.md §3 'MXFP8 GEMMs'): bf = 1 throughout, and the per-layer GEMM classes of mx8_mask (kStoreBit:
  // QKV 1, out-proj 4, FFN1 8, FFN2 16) take MXFP8 operands. mx8_count: device word the MX8 GEMM launches bump
  int mx8 = 0, mx8_mask = 0;
  unsigned long long* mx8_count = nullptr;
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

// ---------------------------------------------------------------- workspace
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
  // F5H_MXFP8 engines (null otherwise): the activation operand of the MX8 launches, elements [rows][max K] and
  // scales [rows][max K / 32] (max K = max(dim, ff_dim); a launch uses the leading rows x K bytes of its part)
  uint8_t *a8, *a8s;
};

// kernel classes of the launch probes (f5h_probe_enable) and, by kStoreBit, of the store policy and the MX8 mask
enum { KC_FFN1 = 0, KC_ATTN = 1, KC_QKV = 2, KC_FFN2 = 3, KC_CONV = 4, KC_OUT = 5, KC_NORM = 6, KC_CHAIN = 7 };

// ---------------------------------------------------------------- the modes of one call
// What step_modes decides from: all int32 (f5h_debug_step_modes takes them as a flat array in this order).
struct ModeIn {
  int32_t backbone, dim, qk_norm, long_skip;  // architecture (f5h_arch)
  int32_t bf;                                 // compute mode (f5h_engine::bf)
  // engine capabilities: the LayerNorm / RMSNorm fold is supported, the chain's fault word exists, F5H_MXFP8 engine
  int32_t lnf_ok, rmsf_ok, chain_slot, mx8_engine;
  // engine switches at the start of the call
  int32_t chain, lnfold, pad_skip, graph_mode, split_cfg, mx8_mask, probe_class;
  int32_t res32, skip_ln;              // process-wide diagnostics (proc_switches)
  int32_t use_cfg, batch_mask, ragged;  // call shape
};
// The modes of one call: decided once (call_begin), read by the graph key, the prologue and the backbone. A new mode is
// a member here and a line in step_modes, where it is also switched off beside the modes it cannot run with. All int32
// (f5h_debug_step_modes returns them as a flat array in this order).
struct StepModes {
  int32_t mx;     // the GEMM classes on MX8 operands (kStoreBit mask; 0: the 16-bit launches exactly)
  int32_t r16;    // 16-bit residual stream (fp32 in the fp32 mode and, on DiT without MX8 classes, under F5H_RES32=1)
  int32_t do_ln;  // 0: F5H_DIAG_SKIP_LN=1 skips the 16-bit DiT path's LayerNorm launches (wrong results, timing only)
  int32_t split;  // the two CFG branches as parallel captured chains (f5h_sample's step graph)
  // this call may run the phase chain: engine switch, architecture and shape; call_begin then asks chain_admit, whose
  // refusal acts as the switch being off. Part of the graph key; the fold yields to it
  int32_t chain_call;
  // ... and the step's launches do chain (not under F5H_DIAG_SKIP_LN, not while a chained class is probed): what
  // backbone_part needs beside its part being the whole packed batch
  int32_t chain_eligible;
  int32_t lnfold;   // the call runs a norm fold (engine switch and shape; never beside the chain): prologue, graph key
  int32_t fold_on;  // DiT: the LayerNorm fold's producers and consumers run
  int32_t rms_on;   // UNetT: the RMSNorm fold's producers and consumers run
  int32_t out_live_skip;  // an out-projection that updates in place skips its row tiles of padding only (live_len)
  int32_t pad_skip, probe_class;  // the engine's switches as they stood at the start of the call
};
StepModes step_modes(const ModeIn& in);
// The process-wide switches of the environment, read once: F5H_RES32=1 (fp32 residual on the 16-bit DiT path, A/B),
// F5H_DIAG_SKIP_LN=1 (StepModes::do_ln), F5H_CHAIN_ZERO=memset (the chain's counters zeroed by a memset node, A/B)
struct ProcSwitches {
  bool res32, skip_ln, chain_zero_memset;
};
const ProcSwitches& proc_switches();

// ---------------------------------------------------------------- one call
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
  StepModes m;  // the call's modes (step_modes, with chain_admit's answer applied): chain, folds, MX8 classes, ...
  int store;    // the engine's store policy at the start of the call
  double* hp;  // host milliseconds of the call by phase (kHostPhases, f5h_last_call_host_ms), or null
  // ragged sampling (f5h_sample_ragged; rag_B = 0 otherwise): rag_B utterances of at most rag_L frames as packed rows.
  // The row-local launches see B = 1, N = L = R (one "sequence" per CFG branch); the four kernels that reach across
  // rows take the segment tables (Bufs rg_*), which the call uploads before the prologue
  int rag_B, rag_L;
};
// Host time of an f5h_sample call by phase (f5h_last_call_host_ms): a call that blocks the host shows where.
enum { HP_TOTAL = 0, HP_PROLOGUE, HP_LOCK, HP_REAP, HP_CAPTURE, HP_INSTANTIATE, HP_LAUNCH, HP_FINAL, kHostPhases };
inline double host_ms() {
  return std::chrono::duration<double, std::milli>(std::chrono::steady_clock::now().time_since_epoch()).count();
}

// ---------------------------------------------------------------- functions that cross files
// engine_pack.cpp
constexpr size_t kConvPackElems = (size_t)16 * 31 * 64 * 64;
int pack_conv_weight(const void* src, int src_dt, int d, void* dst, int dst_dt, hipStream_t st);
// engine_graph.cpp
extern std::atomic<uint64_t> g_kernel_epoch;
int graph_get(Ctx& c, const GraphKey& key, bool split, const std::function<int(Ctx&)>& body,
              std::shared_ptr<GraphEntry>& hold, int64_t replays);
int note_replays(f5h_engine* e, GraphEntry* g, hipStream_t st);
bool prologue_repeats(f5h_engine* e, const GraphKey& key);
// engine_chain.cpp
int fault_slot_take(volatile unsigned** host);
void fault_slot_give(int i);
// Held for one call: admits the call's chain (or not) and, on every return path, records the gate's "done" event
// after the call's launches.
struct ChainTicket {
  int dev = 0;
  hipStream_t st = nullptr;
  bool held = false;
  ~ChainTicket();
};
bool chain_for_call(f5h_engine* e, const Ctx& c, ChainTicket& t);
int chain_fault_check(f5h_engine* e, hipStream_t st);
int chain_fault_note(f5h_engine* e, hipStream_t st);
// engine.cpp
void ode_eval_times(int method, int compute, const float* t, int steps, float* out);

#pragma GCC visibility pop
