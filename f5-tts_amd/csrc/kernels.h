// Launcher declarations for the engine's HIP kernels (gfx950).
#pragma once
#include <hip/hip_runtime.h>
#include <stddef.h>
#include <stdint.h>

namespace f5h {

// Operand dtype of a compute mode (f5h_compute in include/f5h.h): GEMM/attention/conv operands are
// fp32 (parity mode), bf16 or fp16; accumulation, residual stream, norms and the ODE state stay fp32.
enum ComputeMode { F5H_C_FP32 = 0, F5H_C_BF16 = 1, F5H_C_FP16 = 2 };

enum Epi {
  EPI_STORE = 0,      // C = acc + bias                                  (fp32 out)
  EPI_SILU = 1,       // C = silu(acc + bias)                            (fp32 out)
  EPI_GELU_TANH = 2,  // C = gelu_tanh(acc + bias)                       (operand out)
  EPI_GELU_ERF = 3,   // C = gelu_erf(acc + bias)                        (fp32 out)
  EPI_RESID = 4,      // C += gate[n] * (acc + bias) * rowkeep[m]        (fp32 in/out)
  EPI_RESID_FILL = 5, // C = rowkeep[m] ? C + acc + bias : 0             (fp32 in/out)
  EPI_INPROJ = 6,     // C[m] = acc + add[m]; C[m+dual] = acc + add[m+dual]  (fp32)
  EPI_QKV = 7,        // RoPE + scatter to q/k/v [S,H,L,64]              (operand out)
  EPI_GELU_ERF_OP = 8,  // C = gelu_erf(acc + bias)                      (operand out; Vocos pwconv1)
  EPI_RESID16 = 9,   // C += gate[n] * (acc + bias) * rowkeep[m]        (operand dtype in/out: 16-bit residual)
  EPI_STORE16 = 10,  // C = acc + bias                                   (operand out: UNetT skip_proj)
};
// EPI_RESID / EPI_RESID16 read the residual from `resid` when set (else from C) and write C, so a
// layer can keep its input (UNetT skip connections) without a copy.

// In-kernel launch probe (see probe_enter/probe_exit in common.h). Per launch site a row of
// kProbeTicks x kProbeLanes entries, each on its own 128-B line (kProbeStride words): workgroup b
// stamps lane b % kProbeLanes, so same-line atomics stay few; the start rows (atomicMin) come
// first, the end rows (atomicMax) kProbeEnd words further on. Host: min/max over lanes.
// Only every kProbeEvery-th step tick is stamped (the rest run unperturbed apart from one load).
constexpr int kProbeTicks = 512, kProbeSites = 64, kProbeLanes = 16, kProbeStride = 16, kProbeEvery = 4;
constexpr int64_t kProbeRow = (int64_t)kProbeTicks * kProbeLanes * kProbeStride;
constexpr int64_t kProbeEnd = kProbeRow * kProbeSites;
struct DevProbe {
  unsigned long long* slots;  // null: not probed
  const int* tick;            // device step tick
  // per-workgroup timeline of the tick-0 launch of the first probed site (diagnostic, or null):
  // tl[wg*4 + {0: entry, 1: main loop entered (first stage landed), 2: main loop done, 3: exit}]
  unsigned long long* tl;
};
constexpr int kTimelineWG = 8192;  // workgroups recorded per timeline

// Layout: a kernel argument of every GEMM launch, 304 bytes: 24 bytes more moved the hidden grid-size argument onto
// another cache line of the kernarg segment and measured C2 -0.4 % with unchanged kernel code.
// The first 64 bytes are the hot line: everything gemm_kernel reads on its way to the first operand DMA, fetched as one
// batch of scalar loads at entry (gemm_impl.h gemm_body; DESIGN.md §3 'Launch head'). The head_* fields are filled by
// the launchers from the others (gemm_head_fill below); callers leave them alone. lda / ldw / ld_add / dual_rows are
// 32-bit to make room for them; the 4-byte fields store_wt and qk_norm_eps sit where alignment padding would
// otherwise be, away from the fields they go with.
struct GemmArgs {
  const void* A;                   // [M,K] row-major, TA elements, row stride lda
  const void* W;                   // [Npad,K] row-major, operand elements (rows padded to 128), row stride ldw
  const void* A2;                  // A columns [k_split, K) come from A2 (same lda), e.g. cat(x, skip)
  int lda, ldw;
  int M, N, K;                     // K: multiple of 64 (bf16) / 32 (fp32)
  int k_split;                     // with A2
  unsigned head_flags;             // kHeadProbe | kHeadLive (probe.slots / live_len non-null) | div shift << 8
  int head_nwg, head_ntn;          // the launch's workgroups and column tiles
  unsigned head_ntn_mul;           // bid / head_ntn as a multiply and shift (MagicDiv below)
  const float* bias;               // [N] or null
  void* C; int64_t ldc;            // output
  const float* gate;               // EPI_RESID: [N] or null (=1)
  const uint8_t* rowkeep;          // [M] or null (=1)
  const float* add; int ld_add;    // EPI_INPROJ addend
  int dual_rows;                   // EPI_INPROJ: second output at row m + dual_rows (0 = none)
  // EPI_QKV
  const float2* rope;              // [L][32] (cos, sin)
  int seq_len;                     // L: rows per sequence
  int heads, rope_heads;
  int store_wt;                    // store policy (below)
  void* q; void* k; void* v;
  float q_scale;                   // EPI_QKV: q is stored pre-multiplied by this (0 -> 1)
  float qk_norm_eps;               // qk_norm (below)
  DevProbe probe;                  // in-kernel launch timing (null slots: off)
  const void* resid;               // EPI_RESID / EPI_RESID16 residual input (null: C)
  const float* q_norm_w;           // qk_norm (below)
  // EPI_RESID / EPI_RESID16 with rowkeep: the live rows of sequence s are [s*live_seq, s*live_seq +
  // live_len[s]); a tile with no live row skips its K loop and epilogue (its rows keep the residual, as
  // the masked rows of a computed tile do). Null: every tile is computed.
  const int32_t* live_len; int live_seq;
  int group_m;                     // persistent kernel (cfg 13): tile order in groups of this many row tiles (<= 1: n-fastest)
  // LayerNorm fold (DiT 16-bit path without row masks; DESIGN.md §3 'LayerNorm fold'). The AdaLN LayerNorm between a
  // residual GEMM and its consumer, aop = LN(h) (1 + sc) + sh (modules.py:325,753), runs as algebra in the two GEMMs:
  // producer (EPI_RESID16, hs != null): besides h, writes hs = round(h' (1 + hs_scale[n])) (h' = the stored, rounded
  //   h; operand dtype, row stride ldc) and, per row and 64-column strip p, the strip's (mean, M2) of h' into
  //   ln_part[row * ln_nparts + p] (float2; ln_nparts = N / 64);
  // consumer (EPI_GELU_TANH / EPI_QKV, ln_part_in != null; A = hs): combines the row's ln_nparts partials into
  //   (mean_m, rstd_m) and applies x = rstd_m (acc - mean_m ln_u[n]) + ln_v[n] before the bias, where
  //   ln_u[n] = sum_k (1 + sc_k) W[n,k] and ln_v[n] = sum_k sh_k W[n,k] (lnfold_uv, per ODE step).
  void* hs; const float* hs_scale; float* ln_part;
  const float* ln_part_in; int ln_nparts;
  // EPI_QKV: rows of a (sequence, head) panel in the destination, q / k / v [S, heads, qkv_dst_len, 64]; 0 = seq_len
  // (the panels hold exactly the launch's rows). Larger: the launch fills rows [0, seq_len) of every panel and leaves
  // the rest alone, so two launches (the second with q / k / v advanced by the first one's seq_len * 64 elements)
  // fill one joint buffer without a copy (MMDiT: audio rows, then text rows). Not with a fold consumer. It sits in
  // the alignment padding behind ln_nparts (see the layout note).
  int qkv_dst_len;
  const float* ln_u; const float* ln_v;
  // RMSNorm form (UNetT, x_transformers RMSNorm: x / max(|x|, 1e-12) sqrt(d) g): ln_rms = 1. The producer writes
  // (0, sum of squares) per strip and no hs (hs, hs_scale null); the consumer reads the residual stream itself as A,
  // its W already carries the gain (W' = W diag(g), built once), ln_u / ln_v are null (0) and rstd = 1 / sqrt(ss / d +
  // ln_eps). ln_eps: the consumer's variance epsilon (LayerNorm: 1e-6, modules.py:316,336).
  int ln_rms; float ln_eps;
  // Store policy: 1 = the epilogue's stores are write-through (sc1) where the launch has such a variant
  // (EPI_QKV / EPI_RESID16 / EPI_GELU_TANH in the 16-bit 64x128, 128x128 and 192x128 kernels), 0 = plain stores.
  // Same values either way. Set from gemm_store_wt (DESIGN.md §3 'Launch boundaries'). (store_wt: above)
  // EPI_QKV with qk_norm = "rms_norm" (modules.py:286-305, 493-496): both set, or both null (no norm). Per row and
  // head, q <- q rsqrt(mean(q^2) + qk_norm_eps) q_norm_w and k likewise with k_norm_w (each [64] fp32, shared by the
  // heads; the mean over the head's 64 channels), in fp32 on the accumulators after the bias and the fold consumer's
  // correction, before RoPE and q_scale, on every head (also those rope_heads leaves unrotated); v is untouched.
  // Kernels with the norm are instantiations of their own (gemm_impl.h QKN): launches without it run the same code
  // as before. Tile configurations 12 and 13 have no such kernel and run as 11 (or 1), with the same bits.
  // (q_norm_w, qk_norm_eps: above)
  const float* k_norm_w;
  // Ragged EPI_QKV (ragged sampling: packed rows of unequal sequences): `add` (EPI_INPROJ's field, unused by EPI_QKV)
  // then points to a per-row table int2 (sequence, position) [M] (qkv_rowtab below): row m is rotated by rope[position]
  // and stored at row `position` of the (sequence, head) panel, q / k / v [S, heads, qkv_dst_len, 64] (qkv_dst_len set:
  // the longest sequence; seq_len unused). These launches run the general 8-column epilogue (epi8) of the 64x128 (fp32)
  // or 128x128 (16-bit) tile, in instantiations of their own (gemm_impl.h RQ, gemm_rq.hip); every tile configuration
  // gives the same bits, so each sequence has those of its own launch. Not with a fold consumer.
};
__host__ __device__ inline const int2* qkv_rowtab(const GemmArgs& g) { return reinterpret_cast<const int2*>(g.add); }
static_assert(sizeof(GemmArgs) == 304, "GemmArgs: keep the kernel argument's size (see the layout note)");
static_assert(offsetof(GemmArgs, qkv_dst_len) == offsetof(GemmArgs, ln_nparts) + 4 &&
                  offsetof(GemmArgs, ln_u) == offsetof(GemmArgs, ln_nparts) + 8,
              "GemmArgs: qkv_dst_len fills the padding behind ln_nparts");
static_assert(offsetof(GemmArgs, bias) == 64, "GemmArgs: the hot line is the first 64 bytes");

// n / d without a division (the launch heads' tile indices): q = (mulhi(n, mul) + n) >> shift with shift =
// ceil(log2 d) and mul = floor(2^(32 + shift) / d) + 1 - 2^32, the round-up method, exact for every 32-bit n; the
// sum must not carry, so n < 2^31. The launchers use it for n < kMagicMaxN and 1 <= d <= kMagicMaxD and refuse
// larger grids (tests/test_launch_head_div.py walks that whole range against / and %).
constexpr unsigned kMagicMaxN = 1u << 20, kMagicMaxD = 1u << 11;
struct MagicDiv {
  unsigned mul, shift;
};
__host__ __device__ inline MagicDiv magic_div_make(unsigned d) {
  unsigned s = 0;
  while ((1ull << s) < d) ++s;
  return MagicDiv{(unsigned)(((1ull << (32 + s)) / d) + 1ull - (1ull << 32)), s};
}
__host__ __device__ inline unsigned magic_div(unsigned n, unsigned mul, unsigned shift) {
  return ((unsigned)(((unsigned long long)n * mul) >> 32) + n) >> shift;
}

// GemmArgs::head_flags: what the launch head must look at besides the hot line
constexpr unsigned kHeadProbe = 1u, kHeadLive = 2u, kHeadShift = 8;
// Fill the head_* fields for a launch of nwg workgroups over BN-column tiles (the launchers; chain.hip per phase).
// False: the grid is outside the multiply-shift division's range.
inline bool gemm_head_fill(GemmArgs& g, int nwg, int BN) {
  const int ntn = (g.N + BN - 1) / BN;
  if (nwg <= 0 || ntn <= 0 || (unsigned)nwg > kMagicMaxN || (unsigned)ntn > kMagicMaxD) return false;
  const MagicDiv md = magic_div_make((unsigned)ntn);
  g.head_flags = (g.probe.slots ? kHeadProbe : 0u) | (g.live_len ? kHeadLive : 0u) | (md.shift << kHeadShift);
  g.head_nwg = nwg;
  g.head_ntn = ntn;
  g.head_ntn_mul = md.mul;
  return true;
}

// EPI_QKV destination panels (GemmArgs::qkv_dst_len): rows per panel, and the elements from q / k / v to the end of
// the launch's last panel, which holds seq_len rows (the extent of the stores' buffer descriptors; rows >= M start a
// panel past it and are dropped). qkv_dst_len == 0: M * heads * 64, as before.
__host__ __device__ inline int qkv_panel_rows(const GemmArgs& g) { return g.qkv_dst_len ? g.qkv_dst_len : g.seq_len; }
// (S = M / seq_len, the launch's sequences: the kernels pass their division-free quotient)
__host__ __device__ inline uint64_t qkv_dst_elems(const GemmArgs& g, int S) {
  if (!g.qkv_dst_len) return (uint64_t)g.M * g.heads * 64;
  return ((uint64_t)(S * g.heads - 1) * g.qkv_dst_len + g.seq_len) * 64;
}

// Does the row tile [m0, m0 + BM) of an M-row GEMM hold a live row? Sequence s (rows [s*live_seq, (s+1)*live_seq))
// contributes the tile's rows [max(m0, r0), min(last + 1, r0 + live_seq)); its live rows are [r0, r0 +
// live_len[s]): the tile is live iff one of those overlaps is non-empty. Null live_len: always live. Host and
// device (the GEMM kernels' pad-row skip; f5h_debug_tile_live checks it from the CPU tests).
__host__ __device__ inline bool tile_live_rows(const int32_t* live_len, int live_seq, int M, int m0, int BM) {
  if (!live_len) return true;
  const int last = (m0 + BM < M ? m0 + BM : M) - 1;
  for (int s = m0 / live_seq; s <= last / live_seq; ++s) {
    const int r0 = s * live_seq;
    const int lo = m0 > r0 ? m0 : r0;
    const int hi_tile = last + 1, hi_live = r0 + live_len[s];
    if (lo < (hi_tile < hi_live ? hi_tile : hi_live)) return true;
  }
  return false;
}

// compute: ComputeMode (fp32 / bf16 / fp16 operands). A and W both in the operand dtype.
hipError_t gemm(int compute, int epi, const GemmArgs& a, hipStream_t st);
// pin the 16-bit GEMM tile configuration (0, 1, 5, 11, 12, 13; -1 = automatic choice); tuning and test hook
void gemm_force_config(int cfg);


// Store policy of the hot-path producers (DESIGN.md §3 'Launch boundaries'). A launch that is a single wave of
// workgroups (grid <= the resident block slots of its configuration) writes nothing back until its end-of-kernel
// release, which then flushes every dirty byte of the XCD L2s in one burst with all CUs idle; with write-through
// stores the write-back runs under the epilogue and the kernel boundary stays the only synchronisation.
// want: 0 = plain, 1 = write-through wherever a variant exists, -1 = write-through when a variant exists and the
// launch is a single wave. Returns the store_wt to put into the launch's arguments. store_policy_force (test / A/B
// hook, f5h_store_policy_force): mode >= 0 replaces every `want`, also for launches whose arguments were built
// without asking (the op entry points); -1 = as asked.
int gemm_store_wt(int compute, int epi, const GemmArgs& a, int want);
void store_policy_force(int mode);
int store_policy_forced();

// attention: Q,K,V [S,H,L,64] operand dtype; O [S,L,H*64] operand dtype. The softmax scale is 1/sqrt(64) (kAttnScale).
// Layout: a kernel argument of every attention launch, held at 120 bytes (the size it had before kv_start2 / kv_len2:
// kv_start2 sits in the padding behind L, the scale became a constant, and the three 0 / 1 switches share one word
// with the launch head's flags) -- 8 bytes more move the hidden kernel arguments, which measured C2 +0.4 % with the
// default kernels' code unchanged (as GemmArgs' layout note; DESIGN.md §5 'Isolated batches').
// The first 64 bytes are the hot line: everything attn16_kernel reads on its way to the first K/V DMA, fetched as one
// batch of scalar loads at entry (DESIGN.md §3 'Launch head'). The grid's extents follow from it (query blocks of
// 256 rows of L, S * H (sequence, head) pairs). The head_* fields are filled by `attention` (attn_head_fill below);
// callers leave them alone.
constexpr float kAttnScale = 0.125f;
struct AttnArgs {
  const void* q; const void* k; const void* v; void* o;
  int S, H, L;
  int kv_start2;          // first row of the second key range (with kv_len2, below)
  unsigned prescaled : 1;   // q already carries kAttnScale*log2(e): scores are in log2 units
  unsigned force_safe : 1;  // test hook: every workgroup reruns its key loop in the lazy-max form (attention.hip)
  unsigned store_wt : 1;    // store policy: 1 = O is stored write-through (16-bit kernel), 0 = plain; attention_store_wt
  // kAttnHead* (kv_len / q_len / kv_len2 / probe.slots non-null) | shift of id / nqb << 4 | shift of bh / H << 9
  unsigned head_flags : 29;
  unsigned head_nqb_mul, head_h_mul;  // id / nqb and bh / H as multiplies and shifts (MagicDiv above)
  int o_split;            // split output (below)
  const int32_t* kv_len;  // [S] or null: keys [kv_len[s], L) masked
  // [S] or null: query rows [q_len[s], L) are dead (their output is masked to 0 after to_out,
  // modules.py:551-553): query blocks wholly past q_len[s] exit at entry and leave O unwritten
  const int32_t* q_len;
  DevProbe probe;         // in-kernel launch timing (null slots: off)
  // Split output (MMDiT joint attention; 0 = none): with 0 < o_split < L, row r < o_split of sequence s goes to
  // o [S, o_split, H*64] and row r >= o_split to o2 [S, L - o_split, H*64] row r - o_split. Only the output
  // addressing changes (the Q load, the K/V ring and the softmax see one sequence of L rows). (o_split: above)
  void* o2;
  // Second key range (MMDiT joint attention with masked keys; null = none): with kv_len2 [S] the valid keys of
  // sequence s are [0, kv_len[s]) and [kv_start2, kv_start2 + kv_len2[s]) (kv_len null: the first range is
  // [0, kv_start2)). The kernels clamp the first range to kv_start2 and the second to L, so no length reads outside
  // the (sequence, head)'s rows. The key loop walks the first range's 64-key tiles from row 0, then the second
  // range's from row kv_start2 (any row: the tile descriptor's base moves); a tile's DMA extent and key mask end at
  // its own range's end, so rows outside the ranges are never read. Both ranges empty: the output rows are 0.
  // Queries are unchanged (every row of [0, L), q_len, o_split). A separately compiled instantiation: launches
  // without kv_len2 run the kernels they always ran.
  const int32_t* kv_len2;
  // Ragged output (o_split == kAttnRagged; ragged sampling): q / k / v stay padded panels [S, H, L, 64],
  // but sequence s holds only kv_len[s] rows of its panels and its output row n goes to the packed row seg_off[s] + n of
  // o [R, H*64], with seg_off = reinterpret_cast<const int32_t*>(o2) ([S], device). kv_len[s] is key length and live
  // query length at once (q_len == kv_len, both set) and stands where L stands in the plain kernel, so panel rows past it
  // are never read and each (sequence, head) has the bits of the plain kernel on that sequence alone at L = kv_len[s].
  // Not with kv_len2. Separately compiled instantiations (attention.hip RO), as the two-range form's.
};
constexpr int kAttnRagged = -1;
static_assert(sizeof(AttnArgs) == 120, "AttnArgs: keep the kernel argument's size (see the layout note)");
static_assert(offsetof(AttnArgs, kv_len) == 64, "AttnArgs: the hot line is the first 64 bytes");
constexpr unsigned kAttnHeadKv = 1u, kAttnHeadQ = 2u, kAttnHeadKv2 = 4u, kAttnHeadProbe = 8u;
constexpr unsigned kAttnHeadShiftQb = 4, kAttnHeadShiftH = 9;
// Fill the head_* fields of a 16-bit attention launch (query blocks of qrows rows). False: the grid is outside the
// multiply-shift division's range.
inline bool attn_head_fill(AttnArgs& a, int qrows) {
  const int64_t nqb = ((int64_t)a.L + qrows - 1) / qrows, nwg = nqb * a.S * a.H;
  if (nqb <= 0 || nwg <= 0 || nwg > (int64_t)kMagicMaxN || nqb > (int64_t)kMagicMaxD || a.H > (int)kMagicMaxD)
    return false;
  const MagicDiv dq = magic_div_make((unsigned)nqb), dh = magic_div_make((unsigned)a.H);
  a.head_flags = (a.kv_len ? kAttnHeadKv : 0u) | (a.q_len ? kAttnHeadQ : 0u) | (a.kv_len2 ? kAttnHeadKv2 : 0u) |
                 (a.probe.slots ? kAttnHeadProbe : 0u) | (dq.shift << kAttnHeadShiftQb) | (dh.shift << kAttnHeadShiftH);
  a.head_nqb_mul = dq.mul;
  a.head_h_mul = dh.mul;
  return true;
}
hipError_t attention(int compute, const AttnArgs& a, hipStream_t st);
int attention_store_wt(int compute, const AttnArgs& a, int want);  // as gemm_store_wt
// test hook (f5h_attn_force_safe): 1 = every later 16-bit attention launch takes the SAFE rerun
void attention_force_safe(int on);

// grouped conv1d k=31, 16 groups, pad 15 (ConvPositionEmbedding, modules.py:175-201)
struct ConvArgs {
  const void* x; int x_f32;        // [S, L, d] input (fp32 or operand dtype)
  // ragged (in the padding behind x_f32): x, resid and y are packed rows [R, d]; `rowkeep` is then the device segment
  // table int32 off[S + 1] (reinterpreted), sequence s owns rows [off[s], off[s+1]) and taps outside them read zero;
  // L = the longest sequence (the grid's extent), y_seq_stride / y_row_off are unused. Kernels of their own (conv.hip
  // RAG): each sequence has the bits of the plain launch on that sequence alone
  int ragged;
  const void* w;                   // packed [16][31][64 out][64 in] operand dtype
  const float* bias;               // [d]
  const uint8_t* rowkeep;          // [S*L] or null: input rows masked, output rows masked
  int S, L, d;
  // output: mode 0 -> y (operand dtype) = mish(mask(conv)); mode 1 -> y fp32 = mish(mask(conv)) + resid;
  // mode 2 (16-bit operands) -> y operand dtype = mish(mask(conv)) + resid (the 16-bit residual stream)
  int mode;
  void* y; int64_t y_seq_stride; int64_t y_row_off;  // in rows
  const float* resid;              // [S, L, d] fp32 (mode 1)
};
hipError_t conv_pos(int compute, const ConvArgs& a, hipStream_t st);

// ---- elementwise / small kernels (elementwise.hip)
hipError_t time_sinus(const float* t_host, int n, float* out, hipStream_t st);  // host t[n<=512] -> [n,256]
hipError_t time_sinus_dev(const float* tg, int n, float* out, hipStream_t st);  // device t[n]
hipError_t silu_to_op(int compute, const float* x, void* y, int64_t n, hipStream_t st);
// LayerNorm(no affine, eps) * (1 + scale) + shift -> operand dtype; h: [M, d] fp32, or the operand
// dtype when h16 (the 16-bit residual stream of the bf16/fp16 DiT path)
hipError_t ln_modulate(int compute, const void* h, int h16, int M, int d, const float* shift, const float* scale,
                       void* out, hipStream_t st);
// x_transformers RMSNorm: x / max(||x||, 1e-12) * sqrt(d) * g -> operand dtype
// h: fp32, or the operand dtype when h16 (16-bit residual stream)
hipError_t rms_norm_g(int compute, const void* h, int h16, int M, int d, const float* g, void* out, hipStream_t st);
// out[n][k] = round(W[n][k] g[k]) for rows x K 16-bit W (the RMSNorm fold's W' = W diag(g), built once per engine)
hipError_t scale_cols(int compute, const void* W, int64_t rows, int K, const float* g, void* out, hipStream_t st);
hipError_t rope_table(int L, float2* out, hipStream_t st);
// text tokens -> embeddings (dit.py:86-120 / unett.py:53-64), both branches
struct TextEmbArgs {
  const int64_t* text; int B, nt, N, td;  // (ragged: N = the packed rows R)
  const int32_t* seq_len;       // [B] per-sample valid length or null (= N for all)
  const float* table;           // [V, td]
  const float* freqs;           // [8192, td] or null (no sinus pos); [freq_rows, td] when freq_rows > 0
  int freq_rows;                // > 0: position n reads row min(n, freq_rows - 1) (MMDiT: 1024, mmdit.py:39-56)
  int mask_padding;
  float* out_c; float* out_u;   // [B, N, td] each
  uint8_t* keep;                // [2B*N] !fill (for masked_fill after each block) or null
  // ragged (or null): device segment table off[B + 1]; packed row off[b] + n is position n of utterance b, every row
  // valid (seq_len unused); out_c / out_u are [R, td], keep [2R]
  const int32_t* seg_off;
};
hipError_t text_embed(const TextEmbArgs& a, hipStream_t st);
// text_embedding_average_upsampling (TextEmbedding.average_upsample_text_by_mask, dit.py:55-84): per sequence, the T
// valid tokens (not filler after the +1 shift and the per-sample valid range; the mask precedes drop_text, so both
// branches share it; not necessarily a prefix) are spread over the first audio_len = seq_len[b] (N when null) frames:
// with base = audio_len / T and rem = audio_len % T the first T - rem tokens repeat base times, the last rem tokens
// base + 1 times; frames past audio_len, and every frame when T == 0, are zero. A gather (bitwise). in / out:
// [B, N, td] fp32 each, distinct buffers; the _u pair (the unconditional branch) may be null. N <= 8192, td % 4 == 0.
struct TextUpArgs {
  const int64_t* text; int B, nt, N, td;
  const int32_t* seq_len;
  const float* in_c; const float* in_u;
  float* out_c; float* out_u;
};
hipError_t text_upsample(const TextUpArgs& a, hipStream_t st);
// depthwise conv k7 pad3 + bias then LayerNorm(affine, eps 1e-6) -> operand dtype. x: [S, L, C] fp32
// len (device, or null): sequence s ends at row min(L, len[s % len_mod]) -- taps past it are zero, as taps past L
// are; rows below it then have the bits of the sequence alone at that length (rows past it hold anything)
hipError_t dwconv_ln(int compute, const float* x, int S, int L, int C, const float* dw_w, const float* dw_b,
                     const float* ln_w, const float* ln_b, void* out, hipStream_t st, const int32_t* len = nullptr,
                     int len_mod = 1);
// GRN: sumsq[s,c] = sum_n x^2 ; then out = gamma*(x*Nx)+beta+x -> operand dtype
// len (device, or null): the sum runs over rows below min(L, len[s % len_mod]) only (as dwconv_ln's)
hipError_t grn(int compute, const float* x, int S, int L, int C, const float* gamma, const float* beta,
               float* scratch /*[(ceil(L/64)+1)*S*C]*/, void* out, hipStream_t st, const int32_t* len = nullptr,
               int len_mod = 1);
// A_ct [S*N, 128 + td] operand dtype: [where(cond_mask,cond,0) (zeros for uncond) pad 128 | text];
// drop_audio / drop_text apply to the first (conditional) B sequences (single-branch forward)
hipError_t build_ct(int compute, const float* cond, const uint8_t* cond_mask, const float* text_c,
                    const float* text_u, int B, int N, int td, int S, int drop_audio, int drop_text, void* out,
                    hipStream_t st);
// y (fp32 [B,N,mel]) -> ypad operand [B*N, 128]
hipError_t pack_y(int compute, const float* y, int rows, int mel, void* ypad, hipStream_t st);
// CFG + Euler: y += dt * (pc + (pc - pu) * cfg); pred rows from p with row offset/stride.
struct EulerArgs {
  float* y; int B, N, mel;
  const float* p; int64_t p_seq_stride; int p_row_off; int64_t p_ld;  // p[s, row_off + n, c]
  int use_cfg; float cfg; float dt;
  void* ypad; int compute;      // refreshed operand copy (or null)
  float* traj;                  // [B,N,mel] slot to copy y into (or null)
  // device-indexed form (graph replay): when kstep is set, dt = tgrid[k+1] - tgrid[k] and the
  // trajectory slot is traj + (k+1)*B*N*mel, k = *kstep (dt above is ignored)
  // trajectory base (or null) read from *trajp in the device-indexed form
  const int* kstep; const float* tgrid; float* const* trajp;
  // the step bookkeeping folded into this launch (device-indexed form): next_dst[0..next_n) =
  // next_src[(k+1) * next_stride ..] for k + 1 < nfe (the next step's AdaLN / time-token row), and
  // the workgroup that arrives last on *arrive (zeroed per call) bumps *kstep and *tick once every
  // workgroup has read k. next_dst null: no copy; arrive null: no bump.
  const float* next_src; int64_t next_stride; int next_n; float* next_dst; int nfe;
  unsigned* arrive; int* tick;
};
hipError_t cfg_euler(const EulerArgs& a, hipStream_t st);
// Fixed-grid multi-stage solvers (torchdiffeq "midpoint" and "rk4" = the 3/8 rule; f5h_ode_method numbering).
// Butcher tableau of a method: stage times c, stage matrix a (row-major [4][4], strictly lower), weights b.
// cfg_rk_kernel is instantiated with these values; f5h_debug_ode_tableau returns them to the CPU tests.
constexpr int kOdeMethods = 3;
struct OdeTableau {
  int stages;
  float c[4], a[16], b[4];
};
constexpr float kOneThird = (float)(1.0 / 3.0), kTwoThirds = (float)(2.0 / 3.0);
constexpr OdeTableau ode_tableau(int method) {
  return method == 1   ? OdeTableau{2, {0.f, 0.5f}, {0.f, 0.f, 0.f, 0.f, 0.5f}, {0.f, 1.f}}
         : method == 2 ? OdeTableau{4,
                                    {0.f, kOneThird, kTwoThirds, 1.f},
                                    {0.f, 0.f, 0.f, 0.f, kOneThird, 0.f, 0.f, 0.f, -kOneThird, 1.f, 0.f, 0.f, 1.f, -1.f, 1.f, 0.f},
                                    {0.125f, 0.375f, 0.375f, 0.125f}}
                       : OdeTableau{1, {0.f}, {0.f}, {1.f}};
}
// Slopes a method keeps across launches: rk4's k1..k3 (read by its later stages); midpoint's k1 is used up by the
// launch that forms it.
constexpr int ode_kept_slopes(int method) { return method == 2 ? 3 : 0; }
// CFG + one evaluation of a multi-stage step. The device counter *keval counts evaluations e: step k = e / stages,
// stage s = e % stages, dt = sgrid[k+1] - sgrid[k]. A non-final stage keeps its slope in kbuf[s] (rk4) and writes
// the next stage's input to ypad only; the final stage updates y, refreshes ypad and writes trajectory slot k+1.
// Every evaluation copies table row e+1 (e + 1 < neval) to next_dst and the last workgroup bumps the counter, as
// cfg_euler does. p / ypad / next_* / arrive / tick: as EulerArgs.
struct RkArgs {
  float* y; int B, N, mel;
  const float* p; int64_t p_seq_stride; int p_row_off; int64_t p_ld;
  int use_cfg; float cfg;
  void* ypad; int compute;
  int method;                   // 1 midpoint, 2 rk4
  float* kbuf;                  // [ode_kept_slopes(method)][B*N*mel] fp32 (or null when none is kept)
  int* keval; const float* sgrid; float* const* trajp;
  const float* next_src; int64_t next_stride; int next_n; float* next_dst; int neval;
  unsigned* arrive; int* tick;
};
hipError_t cfg_rk(const RkArgs& a, hipStream_t st);
// host grid t[n <= 512] -> device (by kernel argument)
hipError_t grid_upload(const float* t_host, int n, float* out, hipStream_t st);
// dst[0..n) = src[k*stride ..], k = *kstep (n, stride multiples of 4)
hipError_t step_begin(const int* kstep, const float* src, int64_t stride, int n, float* dst, hipStream_t st);
// probe stamps around a launch (DevProbe slot layout), indexed by *tick
hipError_t stamp_begin(unsigned long long* slots, const int* tick, hipStream_t st);
hipError_t stamp_end(unsigned long long* slots, const int* tick, hipStream_t st);
// *kstep += 1 and *tick += 1 (probe step tick)
hipError_t step_advance(int* kstep, int* tick, hipStream_t st);
// p[0..n) = 0 (n a multiple of 4, p 16-B aligned): a kernel, not a memset node
hipError_t zero_words(unsigned* p, int64_t n, hipStream_t st);
hipError_t final_where(const float* cond, const uint8_t* cond_mask, float* y, int B, int N, int mel,
                       hipStream_t st);
// fault: the phase-chain give-up word (or null); when set, out is filled with NaN (the results are wrong)
hipError_t final_where_out(const float* cond, const uint8_t* cond_mask, const float* y, float* out, int B, int N,
                           int mel, const unsigned* fault, hipStream_t st);
// *slot = p (stream-ordered)
hipError_t ptr_upload(float* p, float** slot, hipStream_t st);
// rowkeep[s*L + pos] = (pos - off < dur[s % B]) || pos < off ; for S sequences
hipError_t build_rowkeep(const int32_t* dur, int B, int S, int L, int off, uint8_t* keep, hipStream_t st);
// keep[s*nt + j] = text[(s % B)*nt + j] != -1 for S sequences (MMDiT c_mask, mmdit.py:232)
hipError_t build_textkeep(const int64_t* text, int B, int S, int nt, uint8_t* keep, hipStream_t st);
// kv_len[s] = dur[s % B] + off
hipError_t build_kvlen(const int32_t* dur, int B, int S, int off, int32_t* kv, hipStream_t st);
// len[s] = 1 + the last position j with text[(s % B)*nt + j] != -1 (0 when all are filler), for S sequences: the
// text key range of the MMDiT joint attention (AttnArgs::kv_len2). list_str_to_idx pads with fillers at the end
// only, so this range is the reference's elementwise c_mask; a filler in the interior would stay attended.
hipError_t build_textlen(const int64_t* text, int B, int S, int nt, int32_t* len, hipStream_t st);
// h[s, 0, :] = temb (UNetT time token)
hipError_t write_time_token(int compute, int h16, const float* temb, int S, int L, int d, void* h, hipStream_t st);
// extract rows [s, 1..L-1] of pred -> dst [S, L-1, mel]; NaN when *fault (as final_where_out)
hipError_t copy_pred(const float* p, int S, int L, int row_off, int mel, int64_t p_ld, float* dst,
                     const unsigned* fault, hipStream_t st);
// Vocos decoder glue (vocos.hip)
hipError_t vocos_im2col(int compute, const float* mel, int B, int T, int C, int Kp, void* out, hipStream_t st);
hipError_t vocos_spec(float* x, int64_t rows, int bins, int ld, hipStream_t st);
hipError_t vocos_ola(const float* frames, const float* win, int B, int T, int n_fft, int hop, float* y,
                     hipStream_t st);
// log-mel front end glue (melspec.hip)
hipError_t mel_frames(const float* wav, int B, int L, int T, int n_fft, int hop, float* frames, hipStream_t st);
hipError_t mel_mag(const float* spec, int64_t rows, int bins, int ld_spec, int ld_mag, float* mag, hipStream_t st);
hipError_t mel_log(const float* mel, int B, int T, int n_mels, float* out, hipStream_t st);
// ---- Ragged batches: B utterances of unequal length as packed rows, no padding rows. A device segment table
// int32 off[B + 1] (off[0] = 0, utterance s owns rows [off[s], off[s+1]), every length >= 1) tells the four kernels
// with a reach across rows where each utterance begins and ends; the row-local kernels run on M = off[B] rows.
// Each result equals the per-utterance kernel's bit for bit (same operations in the same order per element).
// host int32 values -> device (by kernel argument, stream-ordered: the host array is free on return)
hipError_t seg_upload(const int32_t* host, int64_t n, int32_t* out, hipStream_t st);
// dwconv_ln over packed rows x [R, C]: taps outside the row's own segment are zero
hipError_t dwconv_ln_ragged(int compute, const float* x, const int32_t* off, int B, int R, int C, const float* dw_w,
                            const float* dw_b, const float* ln_w, const float* ln_b, void* out, hipStream_t st);
// vocos_im2col from a strided source: packed row off[s] + t reads src[s*row_st + (start[s] + t + j - 3)*frame_st +
// c*chan_st] (element strides), zero for taps outside [0, off[s+1] - off[s])
hipError_t vocos_im2col_ragged(int compute, const float* src, int64_t row_st, int64_t frame_st, int64_t chan_st,
                               const int32_t* off, const int32_t* start, int B, int R, int C, int Kp, void* out,
                               hipStream_t st);
// vocos_ola per segment: y packed, utterance s at (off[s] - s)*hop, (len_s - 1)*hop samples
hipError_t vocos_ola_ragged(const float* frames, const float* win, const int32_t* off, int B, int R, int n_fft,
                            int hop, float* y, hipStream_t st);
// mel_frames with one length per wave: off = frame offsets (T_s = 1 + len[s]/hop), wav row s at s*wav_st,
// reflection at len[s] (every len[s] > n_fft/2, checked by the caller)
hipError_t mel_frames_ragged(const float* wav, int64_t wav_st, const int32_t* off, const int32_t* len, int B, int R,
                             int n_fft, int hop, float* frames, hipStream_t st);
// out[s][t][m] = log(max(mel[off[s] + t][m], 1e-5)) for t < T_s, exact 0 for T_s <= t < T_out ([B, T_out, n_mels])
hipError_t mel_log_ragged(const float* mel, const int32_t* off, int B, int T_out, int n_mels, float* out,
                          hipStream_t st);
// GRN over packed rows x [R, C] of S sequences (off[S + 1]): the norm of sequence s runs over its own rows, in 64-row
// partial sums that start at the segment's first row and are added in the fixed order of `grn`, so each sequence has
// grn's bits on that sequence alone. Lmax: the longest sequence. scratch: [(ceil(Lmax/64) + 1) * S * C] floats
hipError_t grn_ragged(int compute, const float* x, const int32_t* off, int S, int R, int Lmax, int C,
                      const float* gamma, const float* beta, float* scratch, void* out, hipStream_t st);
// rowtab[m] = (sequence, position) of packed row m < R = off[S] (GemmArgs ragged EPI_QKV); len[s] = off[s+1] - off[s]
hipError_t build_rowtab(const int32_t* off, int S, int R, int2* rowtab, int32_t* len, hipStream_t st);
hipError_t f32_to_op(int compute, const float* x, int64_t n, void* out, hipStream_t st);
hipError_t op_to_f32(int compute, const void* x, int64_t n, float* out, hipStream_t st);
// Weight packing (engine creation): dst[i0*dst_st[0] + i1*dst_st[1] + i2*dst_st[2] + i3] =
// cvt(src[i0*src_st[0] + i1*src_st[1] + i2*src_st[2] + i3*src_st[3]]) for i < n; element types
// 0 = fp32, 1 = bf16, 2 = fp16 (f5h_dtype); conversions round to nearest even.
struct PackArgs {
  const void* src; int src_dt; int64_t src_st[4];
  void* dst; int dst_dt; int64_t dst_st[3];
  int n[4];
};
hipError_t pack_strided(const PackArgs& a, hipStream_t st);

// ---- MXFP8 operands (OCP MX; compute mode F5H_MXFP8: quant_mx8.hip, gemm_mx8.hip; DESIGN.md §3 'MXFP8 GEMMs').
// A [rows, K] panel is e4m3fn bytes [rows, K] plus one E8M0 scale byte per 32 consecutive K elements [rows, K / 32];
// element value = e4m3(byte) * 2^(scale - 127). The quantisation rule is written in integers, the same code on host
// (f5h_debug_mx8_quant_block, the CPU tests) and device, for weights and activations alike:
//   amax  = the largest |v| of the block as fp32 bits (an integer maximum: NaN > inf > every finite value)
//   scale = clamp(E - 8 + (m > 0x600000), 0, 254) with E / m the exponent / mantissa fields of amax,
//           i.e. 2^ceil(log2(amax / 448)): no element exceeds 448 (the largest e4m3fn value), nothing saturates
//   elem  = RNE e4m3fn of v * 2^(127 - scale) (an exact multiply); a non-finite v gives the e4m3fn NaN 0x7F
__host__ __device__ inline uint8_t mx8_scale_byte(uint32_t amax_bits) {
  const int E = (int)((amax_bits >> 23) & 0xFFu), b = E - 8 + ((amax_bits & 0x7FFFFFu) > 0x600000u ? 1 : 0);
  return (uint8_t)(b < 0 ? 0 : (b > 254 ? 254 : b));
}
// fp32 bits of the scaled value (|x| <= 448 when finite) -> e4m3fn byte, round to nearest even
__host__ __device__ inline uint8_t mx8_e4m3(uint32_t u) {
  const uint32_t sign = (u >> 24) & 0x80u;
  uint32_t a = u & 0x7FFFFFFFu, code;
  if (a >= 0x7F800000u) return 0x7Fu;
  if (a >= 0x3C800000u) {  // >= 2^-6: a normal e4m3 value; the rounding carry runs into the exponent field
    a += 0x7FFFFu + ((a >> 20) & 1u);
    code = (a >> 20) - (120u << 3);
    if (code > 0x7Eu) code = 0x7Eu;
  } else if (a < 0x3A000000u) {  // < 2^-11: below half of the smallest subnormal 2^-9
    code = 0;
  } else {  // subnormal target: RNE(|x| 2^9) in 0 .. 8 (8 = the smallest normal's code)
    const int sh = 14 - ((int)(a >> 23) - 127);  // 21 .. 25
    const uint32_t m = (a & 0x7FFFFFu) | 0x800000u, q = m >> sh, rem = m & ((1u << sh) - 1u), half = 1u << (sh - 1);
    code = q + ((rem > half || (rem == half && (q & 1u))) ? 1u : 0u);
  }
  return (uint8_t)(sign | code);
}
// 2^(127 - scale) as fp32 bits (scale <= 248 for every fp32 amax, so the factor is a normal number)
__host__ __device__ inline uint32_t mx8_unscale_bits(uint8_t scale) { return (uint32_t)(254 - (int)scale) << 23; }

// The fp8 operands of a gemm_mx8 launch, its second kernel argument (GemmArgs keeps its size; its A / W / lda / ldw
// are unused there). count (or null): device word, bumped once per launch (f5h_mx8_stats; exact under graph replay).
struct Mx8Ops {
  const uint8_t* a8; const uint8_t* as;  // A [M, K] elements, [M, K / 32] scales
  const uint8_t* w8; const uint8_t* ws;  // W [N, K] elements, [N, K / 32] scales
  unsigned long long* count;
};
// x: bf16 [M, K], K % 32 == 0 -> q [M, K], s [M, K / 32]
hipError_t quant_rows_mx8(const void* x, int64_t M, int K, uint8_t* q, uint8_t* s, hipStream_t st);
// ln_modulate (bf16 output) written as MX8: bit for bit quant_rows_mx8(ln_modulate(h)), it quantises the
// bf16-rounded value. h: fp32, or bf16 when h16. d % 32 == 0
hipError_t ln_modulate_mx8(const void* h, int h16, int M, int d, const float* shift, const float* scale, uint8_t* q,
                           uint8_t* s, hipStream_t st);
// C = A8 . W8^T on v_mfma_scale_f32_16x16x128_f8f6f4, fp32 accumulation in ascending K, bf16 epilogues EPI_QKV
// (qk_norm, ragged row table, qkv_dst_len as the bf16 launches), EPI_RESID16 and EPI_GELU_TANH through epi8
// (gemm_impl.h). K % 128 == 0. One tile configuration (128 x 128, 4 waves), so an output row's bits depend on its own
// A row only, whatever M and wherever the row sits.
hipError_t gemm_mx8(int epi, const GemmArgs& a, const Mx8Ops& o, hipStream_t st);

// ---- In-launch phase chain (chain.hip): the row-local seams of a DiT block-step (out-proj -> LayerNorm ->
// FFN1 -> FFN2 -> LayerNorm -> next QKV) as ONE launch whose phases hand row groups (kChainRows rows) to the
// next phase through per-group arrival counters (cdna_hip_programming.md §6 Guideline 16, R1: write-through
// payload, drained, one counter add per workgroup; the consumer polls relaxed and acquires once).
constexpr int kChainRows = 64;
struct ChainDep {
  const unsigned* wait;  // the producer phase's row-group counters (null: no in-launch producer)
  int wait_mult, wait_unit;  // a complete group holds wait_mult * ceil(rows of the group / wait_unit) arrivals
  unsigned* pub;         // this phase's row-group counters (null: last phase)
  unsigned* err;         // the engine's fault word: set to 1 when a wait gives up (bounded spin); results then wrong
  unsigned spin_limit;   // polls before a wait gives up
  unsigned long long* tl;  // (set per workgroup in the kernel) its timeline row when the launch is probed, or null
};
struct LnArgs {
  const void* h;  // [M, 1024] residual stream (operand dtype)
  void* out;      // [M, 1024] LN(h) * (1 + scale) + shift
  const float* shift;
  const float* scale;
};
struct ChainArgs {
  GemmArgs out, ff1, ff2, qkv;  // qkv.M == 0: no QKV phase (the model's last layer)
  LnArgs ln1, ln2;
  unsigned* cnt;   // [5][groups] arrival counters, zero before the launch
  int groups;      // ceil(M / kChainRows) (stride of cnt)
  unsigned* fault; // the engine's give-up word (device): a wait that gives up sets it to 1 (f5h_sample then
                   // returns NaN in `out`, and the engine's next call fails with F5H_EHIP)
  DevProbe probe;  // launch timing (f5h_probe_enable "chain"); timeline row per workgroup: entry, rows acquired,
                   // results stored, exit
};
// bytes of cnt a chain launch over M rows uses (the caller zeroes them before the first layer's launch of a step:
// every layer's launch has its own [5][groups] block)
inline size_t chain_counter_bytes(int M) {
  return (size_t)5 * ((M + kChainRows - 1) / kChainRows) * sizeof(unsigned);
}
// LayerNorm fold: out[s][l*LW + {0: u1, F: v1, 2F: u2, 2F+3d: v2} + n] (LW = 2F + 6d, rows of `stride` floats,
// first column out_off) for every ODE step s < nfe and layer l < depth, with sc/sh the step's AdaLN rows of the
// layer in table[s] (modulation layout of modules.py:321-323): FFN1 (W1 [F][d], mlp scale/shift) and QKV
// (Wqkv [3d][d], msa scale/shift). u = sum_k (1 + sc_k) W[n,k], v = sum_k sh_k W[n,k], fp32.
struct LnFoldArgs {
  float* table; int64_t stride; int64_t out_off;
  int nfe, depth, d, F;
  const void* const* w1;    // [depth] device pointers (operand dtype [F][d])
  const void* const* wqkv;  // [depth] device pointers (operand dtype [3d][d])
};
hipError_t lnfold_uv(int compute, const LnFoldArgs& a, hipStream_t st);

// Launch the chain (16-bit operands, dim 1024, whole-column tiles); hipErrorInvalidValue when the shapes do not
// fit it (the caller then issues the separate launches).
hipError_t chain_launch(int compute, const ChainArgs& a, hipStream_t st);
// polls before a chain wait gives up: kChainSpinLimit by default; test hook (f5h_chain_debug_spin_limit) to force
// give-ups, -1 restores the default. Read at launch (graphs captured earlier keep their value)
void chain_set_spin_limit(long long limit);

}  // namespace f5h
