/*
 * f5h.h — C ABI of the MI355X (gfx950) CFM sampling engine.
 *
 * The engine replaces the hot path of the reference:
 *   CFM.sample()            /root/reference/src/f5_tts/model/cfm.py:83-229   (Euler ODE + CFG loop)
 *   DiT.forward()           /root/reference/src/f5_tts/model/backbones/dit.py:319-370
 *   UNetT.forward()         /root/reference/src/f5_tts/model/backbones/unett.py:244-307
 * behind the reference's own Python surface (`model_obj.sample(...)`, called from
 * infer/utils_infer.py:497-504, eval/eval_infer_batch.py:190-200, runtime/.../benchmark.py:415-423).
 *
 * Plain C types only: pointers, sizes, ints. No torch types cross this boundary.
 * Every entry point returns 0 on success, a negative f5h_status otherwise; the
 * message is available from f5h_last_error() (thread-local).
 *
 * Ownership: the engine owns its packed device weights and is immutable after
 * f5h_engine_create (shareable between host threads). The caller owns every I/O
 * buffer and the workspace, so concurrent calls on different workspaces are
 * re-entrant (this replaces the reference's thread-local text cache, dit.py:237-262).
 * All work is enqueued on the caller's hipStream_t (passed as void*).
 */
#ifndef F5H_H
#define F5H_H

#include <stddef.h>
#include <stdint.h>

#ifdef __cplusplus
extern "C" {
#endif

enum f5h_status {
  F5H_OK = 0,
  F5H_EINVAL = -1,   /* bad argument / shape */
  F5H_EHIP = -2,     /* HIP runtime error */
  F5H_ENOWEIGHT = -3,/* missing or mis-shaped weight */
  F5H_ENOMEM = -4,   /* workspace too small */
};

/* F5H_MMDIT (mmdit.py:87-262; a library that exports f5h_op_attention_split has it): joint text-audio attention.
 * Audio tokens [S,N,d] and text tokens [S,nt,d] are two residual streams with their own AdaLN, QKV, out-projection and
 * FFN weights; per block both are projected, rotated by RoPE independently (positions 0..N-1 and 0..nt-1), attended as
 * one sequence of N + nt rows and split again. The last block only pre-normalises the text stream (context_pre_only).
 * The arch must have text_dim == dim, conv_layers == 0, pe_attn_head == 0, long_skip_connection == 0,
 * text_average_upsampling == 0 and depth >= 1 (F5H_EINVAL names the field); qk_norm adds c_q_norm / c_k_norm.
 * nt >= 1. attn_mask_enabled together with use_batch_mask == 1 is refused by f5h_sample / f5h_forward (F5H_EINVAL): the
 * valid keys [0, dur) and [N, N + tlen) are not a prefix of the joint sequence; without a batch mask
 * the flag has no effect, as in the reference. use_batch_mask == 2 (below) masks both ranges itself, whatever the
 * flag says, and is served: tlen = 1 + the last non-filler text position (fillers stand at the end of a text,
 * list_str_to_idx, where this is the reference's elementwise c_mask; a filler in the interior stays attended).
 * Accepted without effect on such an engine: f5h_set_chain, f5h_set_ln_fold, f5h_set_pad_skip and
 * f5h_set_cfg_streams (the joint layout has no live-row prefix, and the block step always runs as one chain of
 * separate launches). */
enum f5h_backbone { F5H_DIT = 0, F5H_UNETT = 1, F5H_MMDIT = 2 };
/* Operand dtype of the GEMM / attention / conv MFMAs. Accumulation, norm and softmax statistics and
 * the ODE state are fp32 in every mode; the residual stream is fp32 in the fp32 mode and, in the 16-bit
 * modes, kept in the operand dtype on both backbones (DiT and UNetT), as the reference keeps it in the
 * parameter dtype.
 *   F5H_FP32: parity mode (exact-f32 MFMA, VALU attention), the <=1e-3 contract;
 *   F5H_BF16: bf16 operands (the BASELINE configs' dtype);
 *   F5H_FP16: fp16 operands = the reference's default GPU dtype (load_checkpoint casts to fp16 on
 *             any GPU with compute capability >= 7, utils_infer.py:190-199); same MFMA rate as bf16. */
enum f5h_compute { F5H_FP32 = 0, F5H_BF16 = 1, F5H_FP16 = 2, F5H_MXFP8 = 3 };
/*   F5H_MXFP8 (opt-in, DiT only; DESIGN.md §3 'MXFP8 GEMMs'): the bf16 mode in every respect but the operands of the
 *             four per-layer GEMMs (QKV, out-projection, FFN1, FFN2), which are OCP MXFP8: e4m3fn elements, one E8M0
 *             scale byte per 32 consecutive K elements, fp32 accumulation on the block-scaled MFMA. The weights are
 *             quantised once at creation (beside the bf16 copy), the activations by the LayerNorm launches and by
 *             quantiser launches ahead of the out-projection and FFN2. f5h_set_mx8_classes chooses the classes.
 *             Engine creation returns F5H_EINVAL for UNetT, MMDiT and an ff_dim that is not a multiple of 128. The
 *             LayerNorm fold, the phase chain, the pad-row live_len skip and F5H_RES32 are off in this mode. */

/* Architecture: mirrors DiT.__init__ (dit.py:171-192) / UNetT.__init__ (unett.py:108-129)
 * and the Hydra arch block (configs/F5TTS_v1_Base.yaml:24-37). */
typedef struct f5h_arch {
  int32_t backbone;          /* f5h_backbone */
  int32_t dim;               /* model width d (multiple of 64) */
  int32_t depth;             /* blocks */
  int32_t heads;             /* attention heads */
  int32_t dim_head;          /* must be 64 */
  int32_t ff_dim;            /* int(dim * ff_mult) */
  int32_t text_dim;          /* text embedding width (DiT: 512; UNetT: mel_dim) */
  int32_t text_num_embeds;   /* vocab size (embedding has text_num_embeds+1 rows) */
  int32_t mel_dim;           /* 100 */
  int32_t conv_layers;       /* ConvNeXtV2 text blocks */
  int32_t text_mask_padding; /* 0/1 */
  int32_t pe_attn_head;      /* 0 = rope on all heads, k>0 = first k heads (modules.py:503-506) */
  int32_t attn_mask_enabled; /* 0/1: key-padding mask in attention (modules.py:512-516) */
  int32_t compute;           /* f5h_compute: FP32 parity mode, BF16 or FP16 MFMA mode */
  /* Appended options (all 0: none; a library that exports f5h_op_text_upsample reads them):
   * qk_norm: 0 none, 1 "rms_norm" (modules.py:402-407, 493-496): RMSNorm(dim_head, eps 1e-6) of every q and k head
   *   ahead of RoPE, fused into the QKV GEMM's epilogue in fp32 on the accumulators (the 16-bit modes round once, at
   *   the store); parameters {attn}.q_norm.weight / {attn}.k_norm.weight [64], DiT and UNetT.
   * long_skip_connection (DiT, dit.py:228, 354-365): x = W . cat(x, input embedding) after the last block, ahead of
   *   the final AdaLN; parameter long_skip_connection.weight [d, 2d].
   * text_average_upsampling (DiT, needs text_mask_padding; dit.py:55-84, 131-137): the valid text tokens' embeddings
   *   spread evenly over each sequence's frames at the end of the text embedding. */
  int32_t qk_norm;
  int32_t long_skip_connection;
  int32_t text_average_upsampling;
} f5h_arch;

/* One named parameter, host memory, float32, C-contiguous, with the reference's
 * state-dict name minus the `transformer.` prefix (e.g. "transformer_blocks.3.attn.to_q.weight"). */
typedef struct f5h_weight {
  const char* name;
  const float* data;
  int64_t numel;
} f5h_weight;

/* Element type of a weight view. */
enum f5h_dtype { F5H_DT_F32 = 0, F5H_DT_BF16 = 1, F5H_DT_F16 = 2 };

/* One named parameter in its own dtype and placement: host memory, or device memory
 * of the engine's device (e.g. a torch parameter's data_ptr() after model.to(dtype).to(device), as
 * load_checkpoint leaves it, utils_infer.py:190-232). C-contiguous, state-dict name as f5h_weight. */
typedef struct f5h_tensor_view {
  const char* name;
  const void* data;
  int32_t dtype;             /* f5h_dtype */
  int32_t on_device;         /* 0: host memory; 1: device memory of `device` */
  int64_t numel;
} f5h_tensor_view;

typedef struct f5h_engine f5h_engine;

/* Replaces: model construction + load_checkpoint (utils_infer.py:190-276): packs the
 * weights into the engine's device layout (bf16/fp16/fp32 GEMM panels, conv taps, the
 * concatenated AdaLN matrix). Host views are staged to the device in their own dtype; every
 * panel is packed on the device (no host fp32 copy of the model). Blocks until packing is complete;
 * the views may be released afterwards. Device views are read on the engine's own non-blocking stream,
 * ordered behind the null stream (hence behind work queued on blocking streams): the caller must have
 * completed any write to them still queued on a non-blocking stream (e.g. a torch side stream). */
int f5h_engine_create_views(const f5h_arch* arch, const f5h_tensor_view* weights, int32_t n_weights,
                            int32_t device, f5h_engine** out);
/* The same from fp32 host arrays (f5h_weight). */
int f5h_engine_create(const f5h_arch* arch, const f5h_weight* weights, int32_t n_weights,
                      int32_t device, f5h_engine** out);
/* Returns at once. The engine's device resources are released on a background thread once the
 * engine's own work has completed (per stream, an event recorded after each call; the events after its
 * graph replays): no device-wide synchronisation, so dropping an engine never waits for other streams.
 * The same holds for f5h_vocos_destroy and f5h_mel_destroy. */
void f5h_engine_destroy(f5h_engine* eng);
/* Releases still queued or running (engines, Vocos and log-mel objects destroyed above); wait != 0
 * first blocks until every one of them has completed (also run at process exit). The objects' device
 * memory comes from a stream-ordered pool per device that keeps released memory for reuse (so neither
 * creation nor release synchronises the device); wait == 2 then also returns the pool's unused memory
 * to the system, which waits for the device. */
int f5h_release_pending(int32_t wait);

/* Arguments of one CFM.sample call after the host preamble of cfm.py:105-158 and
 * the noise/time-grid recipe of cfm.py:196-216. All pointers are DEVICE pointers
 * except t_grid (host). Shapes: B utterances, N = max duration (padded frames),
 * nt text tokens. */
typedef struct f5h_sample_args {
  int32_t B, N, nt, nfe;
  const float* cond;         /* [B,N,mel] padded cond mel (cfm.py:148) */
  const uint8_t* cond_mask;  /* [B,N] 1 = keep cond (lens_to_mask(lens) & edit_mask, cfm.py:128-130) */
  const int64_t* text;       /* [B,nt] token ids, -1 = pad (utils.py:99-106) */
  const int32_t* duration;   /* [B] per-utterance total frames (cfm.py:135-139) */
  const float* y0;           /* [B,N,mel] initial noise, zero-padded (cfm.py:196-201) */
  const float* t_grid;       /* HOST [nfe+1] time grid, EPSS/linspace + sway (cfm.py:211-216) */
  float cfg_strength;        /* < 1e-5 disables the packed uncond branch (cfm.py:167) */
  /* 1 when B>1 (cfm.py:155-158). 2 = the batch mask plus isolation (a library that exports f5h_op_attention_ranges):
   * every utterance is computed as if it were sampled alone, so its rows below duration[b] do not depend on what else
   * is in the batch (the reference's padded batch does: pad keys are attended without attn_mask_enabled, GRN norms over
   * the padded time axis, UNetT / MMDiT run conv_pos_embed unmasked, MMDiT attends filler text keys). Isolated, the
   * row mask goes on both conv_pos launches of every backbone, the key lengths on every attention whatever
   * attn_mask_enabled says (MMDiT: the two ranges [0, dur) and [N, N + tlen)), and the DiT text embedding's depthwise
   * conv and GRN stop at duration[b]. DiT and UNetT rows then equal the utterance's own B = 1 call bit for bit (with
   * the LayerNorm fold off there, as masked batches never fold); MMDiT to rounding (the text keys' tile partition
   * differs). Other values: F5H_EINVAL. The same holds for f5h_forward_args.use_batch_mask. */
  int32_t use_batch_mask;
  float* out;                /* [B,N,mel] result: where(cond_mask, cond, y_final) (cfm.py:223) */
  float* trajectory;         /* [nfe+1,B,N,mel] or NULL (odeint output, cfm.py:218) */
} f5h_sample_args;

/* Bytes of workspace f5h_sample needs for a call of this shape. */
size_t f5h_workspace_size(const f5h_engine* eng, int32_t B, int32_t N, int32_t nt, int32_t nfe,
                          int32_t use_cfg);

/* Replaces CFM.sample's ODE loop (cfm.py:160-223): text embedding once, then nfe Euler
 * steps each running one packed cond/uncond backbone forward, CFG combine and the update,
 * then the final cond overwrite. Everything enqueued on `stream` (a hipStream_t). */
int f5h_sample(f5h_engine* eng, void* stream, const f5h_sample_args* args, void* workspace,
               size_t workspace_bytes);

/* Fixed-grid ODE solvers of the sampler (cfm.py:218 hands odeint_kwargs["method"] to torchdiffeq; the reference's
 * E2-TTS evaluation runs "midpoint"). Per grid interval [t0, t1], dt = t1 - t0, f = the CFG-combined flow:
 *   F5H_EULER:    y1 = y0 + dt f(t0, y0)
 *   F5H_MIDPOINT: h = 0.5 dt; y1 = y0 + dt f(t0 + h, y0 + k1 h), k1 = f(t0, y0)
 *   F5H_RK4:      torchdiffeq's "rk4", the 3/8 rule, c = 1/3: k1 = f(t0, y0), k2 = f(t0 + dt c, y0 + dt k1 c),
 *                 k3 = f(t0 + dt 2/3, y0 + dt (k2 - k1 c)), k4 = f(t1, y0 + dt (k1 - k2 + k3)),
 *                 y1 = y0 + (k1 + 3 (k2 + k3) + k4) dt 0.125
 * 1, 2 and 4 backbone evaluations per step. */
enum f5h_ode_method { F5H_EULER = 0, F5H_MIDPOINT = 1, F5H_RK4 = 2 };

/* f5h_workspace_size / f5h_sample with the solver chosen (F5H_EULER: the same bytes, and bitwise f5h_sample).
 * args->nfe counts grid STEPS and args->t_grid is the step grid [nfe+1]; the trajectory keeps torchdiffeq's
 * meaning, grid points only: [nfe+1,B,N,mel]. The engine derives the stage times from the grid on the host, in
 * the dtype the grid was built in, as the reference does with its parameter-dtype grid: the engine's 16-bit
 * operand dtype (f5h_arch.compute) when every grid value is one of that dtype's (dt and the stage times are then
 * rounded to it), fp32 otherwise. It runs nfe x stages evaluations: one table row and one replay of the captured
 * evaluation graph each, the graph keyed by the method as well. nfe x stages may not exceed 512 (F5H_EINVAL). */
size_t f5h_workspace_size_ode(const f5h_engine* eng, int32_t B, int32_t N, int32_t nt, int32_t steps,
                              int32_t use_cfg, int32_t method);
int f5h_sample_ode(f5h_engine* eng, void* stream, const f5h_sample_args* args, int32_t method, void* workspace,
                   size_t workspace_bytes);
/* Ragged sampling (DiT; DESIGN.md §3 'Ragged sampling'): the B utterances of a call as packed rows, no pad frames.
 * R = sum of duration[b]; utterance b owns rows [off[b], off[b] + duration[b]) of every packed tensor, off the running
 * sum. The engine runs the 2R rows of both CFG branches (the conditional half first); the kernels that reach across
 * rows (QKV epilogue, attention, conv position embedding, the text embedding's ConvNeXt blocks) work per segment, so
 * every utterance's rows equal its own B = 1 call bit for bit (with the LayerNorm fold off there; ragged calls never
 * fold or chain), hence also the use_batch_mask == 2 batch over the rows below duration[b].
 * duration is a HOST array, consumed before the call returns (the segment tables are uploaded by kernel argument); every
 * other pointer is a device pointer except t_grid. Lmax >= every duration (the geometry of the per-segment launches
 * and the q / k / v panels): the step graph is keyed by (B, R, Lmax), not by the lengths, so calls with the same three
 * numbers replay one graph. F5H_EINVAL: a backbone other than DiT, text_average_upsampling, a duration below 1 or above
 * Lmax, durations that do not add up to R, Lmax above 8192, 2 R at or above 2^24. The solver argument is
 * f5h_sample_ode's. Their presence tells a caller that the library samples ragged batches. */
typedef struct f5h_ragged_args {
  int32_t B, Lmax, nt, nfe;
  int64_t R;
  const float* cond;         /* [R,mel] packed cond mel */
  const uint8_t* cond_mask;  /* [R] */
  const int64_t* text;       /* [B,nt] token ids, -1 = pad */
  const int32_t* duration;   /* HOST [B] frames per utterance, each in [1, Lmax] */
  const float* y0;           /* [R,mel] initial noise */
  const float* t_grid;       /* HOST [nfe+1] */
  float cfg_strength;
  float* out;                /* [R,mel] */
  float* trajectory;         /* [nfe+1,R,mel] or NULL */
} f5h_ragged_args;
size_t f5h_workspace_size_ragged(const f5h_engine* eng, int32_t B, int64_t R, int32_t Lmax, int32_t nt, int32_t steps,
                                 int32_t use_cfg, int32_t method);
int f5h_sample_ragged(f5h_engine* eng, void* stream, const f5h_ragged_args* args, int32_t method, void* workspace,
                      size_t workspace_bytes);

/* Test hooks (host only, no device needed). f5h_debug_ode_tableau: the Butcher tableau the solver kernel is
 * instantiated with: *stages, stage times c[4], stage matrix a[16] (row-major 4x4, strictly lower), weights b[4];
 * entries past the method's stages are 0. f5h_debug_ode_eval_times: the steps x stages evaluation times the engine
 * derives from the step grid t_grid[steps+1] for an engine of operand dtype `compute` (f5h_compute). */
int f5h_debug_ode_tableau(int32_t method, int32_t* stages, float* c, float* a, float* b);
int f5h_debug_ode_eval_times(int32_t method, int32_t compute, const float* t_grid, int32_t steps, float* out);

/* One backbone forward: the backbone plugin contract DiT.forward / UNetT.forward
 * (dit.py:319-370, unett.py:244-307) with a scalar time t.
 *   cfg_infer = 1: the packed cond/uncond forward CFM.sample uses (cfm.py:181-191): pred [2B,N,mel],
 *                  conditional rows then unconditional rows (drop flags ignored);
 *   cfg_infer = 0: one branch (cfm.py:167-178), pred [B,N,mel], honouring drop_audio_cond (cond -> 0,
 *                  InputEmbedding, dit.py:155-156) and drop_text (all-filler text ids, dit.py:106-107).
 * x [B,N,mel]; step_cond = where(cond_mask, cond, 0) is formed from cond/cond_mask. Per-sample time
 * values are served by the caller in groups of equal t (sequences are independent at equal N). */
typedef struct f5h_forward_args {
  int32_t B, N, nt;
  const float* x;
  const float* cond;
  const uint8_t* cond_mask;
  const int64_t* text;
  const int32_t* duration;
  float t;
  int32_t use_batch_mask;
  float* pred;               /* [2B,N,mel] (cfg_infer) or [B,N,mel] */
  int32_t cfg_infer;
  int32_t drop_audio_cond;
  int32_t drop_text;
  const float* t_dev;        /* DEVICE fp32 scalar time (read on the stream, no host sync), or NULL: use t */
  /* The reference's text cache (dit.py:294-317: with cache=True the first forward of a sample()
   * computes text_cond/text_uncond, later forwards reuse them until clear_cache()):
   *   0: compute the text embedding (both branches) for this call only;
   *   1: compute it and keep it in `workspace` for later calls;
   *   2: reuse the one kept in `workspace` (same B, N, nt; the text and durations of the keeping call).
   * With 1 or 2 the backbone step runs as a captured graph keyed by the workspace (graph mode). */
  int32_t text_cache;
} f5h_forward_args;
int f5h_forward(f5h_engine* eng, void* stream, const f5h_forward_args* args, void* workspace,
                size_t workspace_bytes);

/* Kernel probe: when enabled, every launch of kernel class `kclass` is timed on the device wall
 * clock (s_memrealtime): GEMM and attention kernels stamp their own entry/exit, the other classes
 * get a stamp kernel on each side (no HIP events, so it also times graph replays; every 4th NFE
 * step is sampled). f5h_probe_read returns (sampled launches, total ms). Enabling resets the slots
 * and synchronises the device. Classes: 0 = FFN1 GEMM, 1 = attention, 2 = QKV GEMM, 3 = FFN2 GEMM,
 * 4 = conv, 5 = attention output-projection GEMM, 6 = pre-FFN norm (LayerNorm+modulate / RMSNorm), 7 = the phase
 * chain launch (f5h_set_chain; its timeline row per workgroup: entry, rows acquired, results stored, exit). While
 * one of the classes 0, 2, 3, 5, 6 is probed the chain is off (those launches are timed one by one). */
int f5h_probe_enable(f5h_engine* eng, int32_t kclass, int32_t enable);
int f5h_probe_read(f5h_engine* eng, int64_t* launches, double* total_ms);
/* Per-workgroup timeline of the probed class's first launch in the first probed step (GEMM and
 * attention kernels): stamps[4*w + {0 entry, 1 main loop entered, 2 main loop done, 3 exit}] in ticks of
 * the device wall clock (tick_khz); n_wg = workgroups recorded (at most max_wg, at most 8192). */
int f5h_probe_timeline(f5h_engine* eng, uint64_t* stamps, int32_t max_wg, int32_t* n_wg, double* tick_khz);

/* NFE-step graph (the CFM.sample ODE loop, cfm.py:218 -> torchdiffeq Euler): with mode 1 (default;
 * env F5H_GRAPH=0 selects 0 at engine creation) f5h_sample captures one NFE step -- table-row
 * copy, backbone forward, CFG combine + Euler update, device step counter -- into a hipGraph on
 * first use and replays it nfe times; mode 0 launches the same sequence eagerly. The step touches
 * only workspace buffers, so the graph is keyed by (workspace, B, N, nfe, cfg, mask, probe,
 * kernel epoch); the caller's out/trajectory pointers are staged into the workspace per call.
 * The call prologue (time/AdaLN tables, text embedding, hoisted input projection) is captured as
 * a graph of its own only when its shape repeats (the first call of a shape runs it eagerly; env
 * F5H_PROLOGUE_GRAPH=0: always eager). Results are bitwise identical in every mode.
 * f5h_graph_stats: captures so far and graph replays so far (prologue and step graphs together),
 * graphs cached (LRU of 16 over both kinds). An evicted graph is destroyed later, without any host
 * wait, once the events recorded after its replays have completed and no caller holds it. */
int f5h_set_graph_mode(f5h_engine* eng, int32_t mode);
/* Launch chains of the captured step: 2 captures the conditional and the unconditional CFG branch as
 * two parallel chains (fork/join by events), so kernel boundaries of one branch overlap work of the
 * other; 1 = one chain over the packed batch; 0 = automatic (the default: currently one chain, measured
 * faster at C2, C3 and C5 and 0.7 % slower at C4; env F5H_SPLIT_CFG=0/1/2 = never/always/auto at engine
 * creation). Results are bitwise identical. */
int f5h_set_cfg_streams(f5h_engine* eng, int32_t n);
int f5h_graph_stats(f5h_engine* eng, int64_t* captures, int64_t* replays, int32_t* cached);
/* Host milliseconds the engine's newest f5h_sample call spent, by phase (a call that blocks its host thread
 * shows where): ms[0] whole call, [1] prologue (enqueue, or graph stage + launch), [2] waiting for the graph
 * cache lock, [3] destroying evicted graphs, [4] capturing, [5] instantiating, [6] launching the step graphs /
 * steps, [7] final kernel + fault-word copy. Writes min(n, 8) values, zeros past 8. */
int f5h_last_call_host_ms(f5h_engine* eng, double* ms, int32_t n);
/* Batch path (use_batch_mask): pad query rows' attention output is zeroed after to_out
 * (modules.py:551-553), so attention query blocks past a sequence's length exit at entry and out-proj row
 * tiles of padding only skip their work (the rows keep their residual, as masked rows of a computed tile
 * do). 1 (default; env F5H_NO_PAD_SKIP=1 at creation: 0) or 0 to compute every block. Bitwise identical. */
int f5h_set_pad_skip(f5h_engine* eng, int32_t enable);
/* 16-bit DiT path without row masks: run each layer's out-proj, LayerNorm, FFN1, FFN2 and the next layer's
 * LayerNorm + QKV (modules.py:743-757) as ONE launch whose phases hand 64-row groups to each other through
 * arrival counters (chain.hip, DESIGN.md §3 'Phase chain'), instead of six launches. 0 (default) or 1 (env
 * F5H_CHAIN=1 at creation: 1). Bitwise identical results; slower than the separate launches at C2 (58.4 vs
 * 51.1 ms), hence off. */
int f5h_set_chain(f5h_engine* eng, int32_t enable);
/* LayerNorm fold (DESIGN.md §3 'LayerNorm fold'): on the 16-bit DiT path without row masks, the AdaLN LayerNorm +
 * modulate between a residual GEMM and its consumer (modules.py:325,753: out-proj -> FFN1, FFN2 -> the next QKV)
 * runs inside those two GEMMs instead of as a launch of its own: the producer also writes h (1 + scale) and per-row
 * (mean, M2) partials of h, the consumer normalises its accumulators, rstd (acc - mean u) + v with per-step vectors
 * u = (1 + scale) W^T, v = shift W^T computed once per call. Not bitwise the separate launches (the statistics and
 * the rounding point move): within the reduced-precision envelopes (tests/test_gpu_envelope.py). 1 (default) or 0
 * (env F5H_LNFOLD=0 at creation: 0). The same switch covers the UNetT RMSNorm fold (default 0 on UNetT engines,
 * F5H_LNFOLD=1: on; unett.py:300-301, x_transformers
 * RMSNorm): every FFN-norm and the attention-norms of the first half's layers 1.., on masked batches too; the
 * producers write per-row sums of squares, the consumers read the residual stream with W diag(g) built once per
 * engine. f5h_ln_fold_stats: *supported = 1 when the engine can fold (16-bit DiT with dim and ff_dim multiples of
 * 64, or 16-bit UNetT with dim a multiple of 64; dim <= 1024), *passes = backbone passes enqueued with a fold. */
int f5h_set_ln_fold(f5h_engine* eng, int32_t enable);
int f5h_ln_fold_stats(f5h_engine* eng, int32_t* supported, int64_t* passes);
/* Store policy of a layer's five hot launches (QKV, attention, out-proj, FFN1, FFN2; 16-bit modes). A launch that is
 * a single wave of workgroups writes nothing back until its end-of-kernel release flushes every dirty byte at once,
 * with all compute units idle; the write-through variants of those kernels store with the sc1 cache policy, so the
 * write-back runs under the epilogue. Values are bitwise identical under every policy.
 * mode: -1 = auto (default): write-through when the launch is a single wave (grid <= resident workgroup slots of
 * its configuration: single-utterance calls; batches keep plain stores), 0 = plain stores, 1 = write-through wherever
 * a variant exists, 0x100 | mask = write-through for the classes in mask (1 QKV, 2 attention, 4 out-proj, 8 FFN1,
 * 16 FFN2; for A/B runs). The policy is part of the step graph's key. f5h_store_policy_stats: hot launches enqueued
 * (eager launches and graph captures, not replays) with write-through and with plain stores.
 * f5h_store_policy_force: process-wide test hook beside f5h_gemm_force_config; mode 0 / 1 overrides every engine's
 * policy and also applies to the op entry points (f5h_op_gemm_epi, f5h_op_attention*), -1 = off. */
int f5h_set_store_policy(f5h_engine* eng, int32_t mode);
int f5h_store_policy_stats(f5h_engine* eng, int64_t* write_through, int64_t* plain);
int f5h_store_policy_force(int32_t mode);
/* F5H_MXFP8 engines: the GEMM classes that run on MXFP8 operands, mask of the store policy's class bits (1 QKV,
 * 4 out-proj, 8 FFN1, 16 FFN2; other bits: F5H_EINVAL). A class outside the mask runs the bf16 launch of the bf16
 * mode, so mask 0 is that mode bit for bit. Default: all four (29), or F5H_MX8_CLASSES at creation. The mask is part
 * of the step graph's key. F5H_EINVAL on an engine of another compute mode.
 * f5h_mx8_stats: *mask = the current mask (0 on other engines), *launches = MX8 GEMM launches the device has run for
 * this engine (counted on the device, so graph replays count). Synchronous: call after the engine's work completed. */
int f5h_set_mx8_classes(f5h_engine* eng, int32_t mask);
int f5h_mx8_stats(f5h_engine* eng, int32_t* mask, int64_t* launches);
/* Failure of the chain (never expected): a chain wait that gives up (a bounded spin of ~0.3 s) sets the
 * ENGINE's fault word; that call's `out` (f5h_sample) / `pred` (f5h_forward) is then all NaN, and the engine's
 * next f5h_sample / f5h_forward fails with F5H_EHIP (message in f5h_last_error), clears the word and turns the
 * chain off for the engine. Concurrency: a call that would chain while a chained call from another stream of
 * the same device is still enqueued or running takes the separate launches (two chain launches in flight starve
 * each other, DESIGN.md §3 'Phase chain'); results are bitwise the same either way.
 * Test hook: *launches = chain launches this engine has enqueued (eager launches and graph captures);
 * *fault = the engine's fault word (1: a wait gave up since it was last cleared; NOT cleared here: the next call
 * reports it); *refused = chained calls of this process sent to the separate launches by the concurrency rule.
 * Synchronous; call after the engine's work has completed. Any pointer may be NULL. */
int f5h_chain_stats(f5h_engine* eng, int64_t* launches, int32_t* fault, int64_t* refused);
/* Test hook: polls before a chain wait gives up (limit >= 0; 0 = at the first poll that finds its rows not yet
 * produced), -1 restores the default (~0.3 s). Applies to launches and graph captures made afterwards. */
int f5h_chain_debug_spin_limit(int64_t limit);

/* Op-level entry points (parity tests / microbenchmarks). Device pointers, row-major. */
/* C[M,N] = A[M,K] . W[N,K]^T + bias  (fp32 in/out; compute = F5H_FP32 or F5H_BF16 operands) */
int f5h_op_linear(void* stream, int32_t compute, int32_t M, int32_t N, int32_t K, const float* A,
                  const float* W, const float* bias, float* C, void* workspace, size_t workspace_bytes);
/* O[S,N,H*64] = softmax(Q K^T / 8 [+key mask]) V with Q,K,V [S,H,N,64] fp32;
 * kv_len: [S] valid keys per sequence or NULL. q_prescaled != 0: Q already carries
 * scale * log2(e) (the engine's layout: scores in log2 units). */
int f5h_op_attention(void* stream, int32_t compute, int32_t S, int32_t H, int32_t N, const float* Q,
                     const float* K, const float* V, const int32_t* kv_len, int32_t q_prescaled, float* O,
                     void* workspace, size_t workspace_bytes);
/* The same with q_len: [S] live query rows per sequence or NULL. Rows [q_len[s], N) are dead: a skip unit (a
 * 64-row block in the fp32 mode, a 32-row wave in the 16-bit modes) wholly past q_len[s] leaves its rows of O
 * unwritten, one that straddles it writes all of its rows. In the 16-bit modes the kernel writes the 16-bit O at
 * workspace byte 6 * S*H*N*64, which is then converted to `O` whole: unwritten rows show what the caller left
 * there. */
int f5h_op_attention_qlen(void* stream, int32_t compute, int32_t S, int32_t H, int32_t N, const float* Q,
                          const float* K, const float* V, const int32_t* kv_len, const int32_t* q_len,
                          int32_t q_prescaled, float* O, void* workspace, size_t workspace_bytes);

/* f5h_op_attention_qlen with a second key range: with kv_len2 [S] (device) the valid keys of sequence s are
 * [0, kv_len[s]) and [kv_start2, kv_start2 + kv_len2[s]) (kv_len NULL: [0, kv_start2)); 0 <= kv_start2 <= N, any row.
 * The first range is clamped to kv_start2 and the second to N. K / V rows outside the ranges are never read (they may
 * hold NaN); a sequence with both ranges empty gets 0. kv_len2 NULL is f5h_op_attention_qlen itself, the same
 * kernels. Its presence tells a caller that the library serves use_batch_mask == 2. */
int f5h_op_attention_ranges(void* stream, int32_t compute, int32_t S, int32_t H, int32_t N, const float* Q,
                            const float* K, const float* V, const int32_t* kv_len, int32_t kv_start2,
                            const int32_t* kv_len2, const int32_t* q_len, int32_t q_prescaled, float* O,
                            void* workspace, size_t workspace_bytes);

/* f5h_op_attention_qlen with a split output (MMDiT joint attention): with 0 < o_split < N, row r < o_split of
 * sequence s goes to O [S, o_split, H*64] and row r >= o_split to O2 [S, N - o_split, H*64] row r - o_split; o_split
 * == 0 is f5h_op_attention_qlen (O2 unused). In the 16-bit modes the 16-bit O and O2 sit back to back at workspace
 * byte 6 * S*H*N*64 (S*H*N*64 elements together) and are then converted whole, as f5h_op_attention_qlen's. Its
 * presence tells a caller that the library runs F5H_MMDIT engines and reads f5h_op_gemm_args.qkv_dst_len. */
int f5h_op_attention_split(void* stream, int32_t compute, int32_t S, int32_t H, int32_t N, const float* Q,
                           const float* K, const float* V, const int32_t* kv_len, const int32_t* q_len,
                           int32_t q_prescaled, int32_t o_split, float* O, float* O2, void* workspace,
                           size_t workspace_bytes);

/* Op-level entry points of the conv, norm and GEMM-epilogue kernels (tests/test_gpu_ops.py). fp32 device tensors
 * in and out; buffers a kernel reads or writes in the operand dtype are staged in `workspace` (rounded to nearest
 * even); the production launcher runs unchanged. A buffer the kernel writes in the operand dtype starts as the
 * rounded copy of the caller's fp32 buffer, so elements the kernel leaves alone come back as they went in. Shapes
 * outside a launcher's contract return F5H_EINVAL before any device work, a short workspace F5H_ENOMEM.
 *
 * ConvPositionEmbedding layer (modules.py:175-201): y = mish(where(keep, conv(where(keep, x, 0)) + bias, 0))
 * [+ resid], Conv1d(d, d, k 31, 16 groups, pad 15) per sequence. x [S,L,d]; w [d, d/16, 31] (torch layout, packed
 * as engine creation packs it); bias [d]; rowkeep [S*L] bytes or NULL. mode 0: y [S,L,d] in the operand dtype
 * (y_seq_stride = L, y_row_off = 0); mode 1: y fp32 = .. + resid; mode 2 (16-bit modes): y operand dtype = .. +
 * resid; modes 1, 2 write row y_row_off + n of sequence s in y [S, y_seq_stride, d]; resid [S,L,d] fp32.
 * x_as_f32 (16-bit modes): the kernel reads the fp32 x and rounds it itself; 0: it reads x rounded beforehand.
 * d % 128 == 0, d <= 1024. */
int f5h_op_conv_pos(void* stream, int32_t compute, int32_t S, int32_t L, int32_t d, const float* x, const float* w,
                    const float* bias, const uint8_t* rowkeep, int32_t mode, const float* resid, int32_t x_as_f32,
                    int64_t y_seq_stride, int64_t y_row_off, float* y, void* workspace, size_t workspace_bytes);
/* Row norms, h [M,d] -> out [M,d] (operand dtype). kind 0: LayerNorm(eps 1e-6, no affine) * (1 + scale) + shift
 * with shift_or_g = shift [d], scale [d] (modules.py:325, 346); kind 1: x_transformers RMSNorm
 * h / max(|h|, 1e-12) * sqrt(d) * g with shift_or_g = g [d] (scale ignored). h16 (16-bit modes): the kernel reads
 * h in the operand dtype (the 16-bit residual stream). d % 4 == 0, d <= 2048. */
int f5h_op_norm(void* stream, int32_t compute, int32_t kind, int32_t h16, int32_t M, int32_t d, const float* h,
                const float* shift_or_g, const float* scale, float* out, void* workspace, size_t workspace_bytes);
/* ConvNeXtV2Block front half (modules.py:260-264, 273-275): depthwise Conv1d(k 7, pad 3) + bias, then
 * LayerNorm(affine, eps 1e-6). x [S,L,C]; dw_w [C,7]; dw_b, ln_w, ln_b [C]; out [S,L,C] (operand dtype). C <= 1024. */
int f5h_op_dwconv_ln(void* stream, int32_t compute, int32_t S, int32_t L, int32_t C, const float* x,
                     const float* dw_w, const float* dw_b, const float* ln_w, const float* ln_b, float* out,
                     void* workspace, size_t workspace_bytes);
/* GRN (modules.py:236-245): Gx = |x|_2 over time, Nx = Gx / (mean_c Gx + 1e-6), out = gamma (x Nx) + beta + x.
 * x [S,L,C]; gamma, beta [C]; out [S,L,C] (operand dtype). */
int f5h_op_grn(void* stream, int32_t compute, int32_t S, int32_t L, int32_t C, const float* x, const float* gamma,
               const float* beta, float* out, void* workspace, size_t workspace_bytes);
/* The two with a length per sequence, len [S] (device; NULL: the plain ops): sequence s ends at row min(L, len[s]).
 * The depthwise conv's taps past it are zero and GRN's norm sums rows below it only, so rows below len[s] equal, bit
 * for bit, the plain op on that sequence alone at L = len[s]. Rows past it are written from whatever x holds there. */
int f5h_op_dwconv_ln_len(void* stream, int32_t compute, int32_t S, int32_t L, int32_t C, const float* x,
                         const float* dw_w, const float* dw_b, const float* ln_w, const float* ln_b,
                         const int32_t* len, float* out, void* workspace, size_t workspace_bytes);
int f5h_op_grn_len(void* stream, int32_t compute, int32_t S, int32_t L, int32_t C, const float* x, const float* gamma,
                   const float* beta, const int32_t* len, float* out, void* workspace, size_t workspace_bytes);

/* f5h_op_linear with any GEMM epilogue (the LayerNorm / RMSNorm fold forms: the struct's trailing fields). epi:
 *   0 STORE       C = acc + bias                          1 SILU          C = silu(acc + bias)
 *   2 GELU_TANH   C = gelu_tanh(acc + bias)  (operand)    3 GELU_ERF      C = gelu_erf(acc + bias)
 *   4 RESID       C = keep[m] ? R + gate[n] (acc + bias) : R, R = resid or C
 *   5 RESID_FILL  C = keep[m] ? C + acc + bias : 0
 *   6 INPROJ      C[m] = acc + add[m]; with dual_rows, C[m + dual_rows] = acc + add[m + dual_rows]
 *   7 QKV         columns [q | k | v] of heads x 64: interleaved-pair RoPE on the first rope_heads heads of q and
 *                 k (0 = all) at position m % seq_len, q times q_scale (0 = 1), to q, k, v [M/seq_len, heads,
 *                 seq_len, 64] (operand)
 *   8 GELU_ERF_OP as 3 (operand)    9 RESID16 as 4 with C and resid in the operand dtype    10 STORE16 as 0 (operand)
 * acc = [A[:, :k_split] | A2[:, :K - k_split]] . W^T when A2 is set (both [M,K], row stride K), else A . W^T.
 * "(operand)": the kernel stores the operand dtype. C is [M + dual_rows, N]. live_len [M / live_seq] with live_seq:
 * the pad-row skip of an in-place RESID / RESID16 with rowkeep (row tiles without a live row are not computed).
 * rope_out [seq_len, 32, 2] or NULL: receives the (cos, sin) table the kernel read. K % 64 == 0. */
typedef struct f5h_op_gemm_args {
  int32_t compute, epi, M, N, K, k_split;
  const float* A;
  const float* A2;
  const float* W;        /* [N,K] */
  const float* bias;     /* [N] or NULL */
  float* C;
  const float* resid;    /* [M,N] or NULL */
  const float* gate;     /* [N] or NULL (= 1) */
  const uint8_t* rowkeep;/* [M] or NULL (= 1) */
  const int32_t* live_len;
  int32_t live_seq;
  int32_t seq_len, heads, rope_heads;
  float q_scale;
  const float* add;      /* [M + dual_rows, ld_add] */
  int64_t ld_add;
  int64_t dual_rows;
  float* q;
  float* k;
  float* v;
  float* rope_out;
  /* LayerNorm / RMSNorm fold forms (16-bit modes; all zero: none). ln_nparts = the row's 64-column strips.
   * Producer (epi 9, ln_part_out set; ln_nparts = N / 64, N % 128 == 0): besides C, the kernel writes per row and
   * strip the (mean, M2) of the stored C into ln_part_out [M + F5H_OP_GUARD_ROWS, ln_nparts, 2] and, in the
   * LayerNorm form (hs_scale [N] and hs_out both set), hs = round(C (1 + hs_scale)) into hs_out
   * [M + F5H_OP_GUARD_ROWS, N] (fp32 view of the 16-bit buffer). ln_rms = 1: the RMSNorm form, strips hold
   * (0, sum of squares), no hs (hs_scale, hs_out NULL); rowkeep is allowed in this form only. Both outputs come
   * back with their guard rows, which the hook fills with NaN before the launch (the kernel's descriptors end at
   * row M); with poison != 0 the live rows start as NaN too (else 0), so an unwritten strip shows.
   * Consumer (epi 2 or 7, ln_part_in [M, ln_nparts, 2] set; ln_nparts = K / 64): x = rstd (acc - mean ln_u[n]) +
   * ln_v[n] + bias ahead of the activation, (mean, rstd) combined from the row's partials with variance epsilon
   * ln_eps; A is hs. LayerNorm form: ln_u, ln_v [N] both set; RMSNorm form (ln_rms = 1): both NULL. live_len and
   * fp32 compute are refused with either form. */
  const float* hs_scale;
  float* hs_out;
  float* ln_part_out;
  const float* ln_part_in;
  const float* ln_u;
  const float* ln_v;
  int32_t ln_nparts, ln_rms;
  float ln_eps;
  int32_t poison;
  /* qk_norm (epi 7; both NULL: none): q <- q rsqrt(mean_64(q^2) + qk_norm_eps) q_norm_w per row and head, k likewise
   * with k_norm_w ([64] each), after the bias (and the fold consumer's correction), before RoPE and q_scale, on every
   * head; v is untouched. Every tile configuration gives the same bits (12 and 13 run as 11 or 1). */
  const float* q_norm_w;
  const float* k_norm_w;
  float qk_norm_eps;
  /* epi 7 (read by a library that exports f5h_op_attention_split): rows of a destination (sequence, head) panel, 0 =
   * seq_len. Larger: q, k, v are [M/seq_len, heads, qkv_dst_len, 64], the launch writes rows [0, seq_len) of every panel
   * and leaves the others as the caller's buffers hold them (the hook pre-fills its 16-bit staging from them). Refused
   * below seq_len and with a fold consumer. */
  int32_t qkv_dst_len;
  /* epi 7 over packed rows of unequal sequences (read by a library that exports f5h_sample_ragged; NULL: none): seg_off
   * is a HOST table [n_seq + 1], 0 = seg_off[0] < ... < seg_off[n_seq] = M, every length <= qkv_dst_len; row m of
   * sequence s at position n = m - seg_off[s] is rotated by rope[n] and stored at row n of panel (s, head) of q, k, v
   * [n_seq, heads, qkv_dst_len, 64]; seq_len must equal qkv_dst_len (the rope table's rows). Panel rows past a
   * sequence's length come back as the caller's buffers hold them. No fold consumer. */
  const int32_t* seg_off;
  int32_t n_seq;
} f5h_op_gemm_args;
#define F5H_OP_GUARD_ROWS 4
int f5h_op_gemm_epi(void* stream, const f5h_op_gemm_args* args, void* workspace, size_t workspace_bytes);
/* MXFP8 op hooks (compute mode F5H_MXFP8). fp32 device tensors in; the hooks round them to bf16 and the DEVICE
 * quantises: e4m3fn element bytes q [rows, K] and E8M0 scale bytes s [rows, K / 32] come back (device, uint8), value =
 * e4m3(q) * 2^(s - 127). The rule (integers only): amax = the largest |v| of a 32-block as fp32 bits; s = clamp(E - 8 +
 * (m > 0x600000), 0, 254) with E, m its exponent and mantissa fields; q = RNE e4m3fn of v * 2^(127 - s); a non-finite v
 * gives 0x7F. f5h_debug_mx8_quant_block runs the same code on the host for one block of 32 fp32 values.
 *   f5h_op_quant_mx8: x [M, K], K % 32 == 0.
 *   f5h_op_ln_modulate_mx8: f5h_op_norm's kind 0 written as MX8 (h16: the kernel reads the bf16-rounded h); bit for bit
 *     f5h_op_quant_mx8 of f5h_op_norm's output. d % 32 == 0, d <= 2048.
 *   f5h_op_gemm_mx8: C = A8 . W8^T with epilogue epi 2 (GELU_TANH), 7 (QKV: qk_norm, qkv_dst_len, seg_off as
 *     f5h_op_gemm_epi) or 9 (RESID16: gate, rowkeep, resid); args->compute is ignored (bf16 epilogues); A2, add,
 *     live_len and the fold fields are refused. K % 128 == 0. a8 / as / w8 / ws_ (each may be NULL) receive the
 *     quantised operands [M, K], [M, K / 32], [N, K], [N, K / 32]. */
int f5h_debug_mx8_quant_block(const float* v32, uint8_t* q32, uint8_t* scale);
int f5h_op_quant_mx8(void* stream, int64_t M, int32_t K, const float* x, uint8_t* q, uint8_t* s, void* workspace,
                     size_t workspace_bytes);
int f5h_op_ln_modulate_mx8(void* stream, int32_t h16, int32_t M, int32_t d, const float* h, const float* shift,
                           const float* scale, uint8_t* q, uint8_t* s, void* workspace, size_t workspace_bytes);
int f5h_op_gemm_mx8(void* stream, const f5h_op_gemm_args* args, uint8_t* a8, uint8_t* as, uint8_t* w8, uint8_t* ws_,
                    void* workspace, size_t workspace_bytes);
/* The text average upsampling kernel alone (text_average_upsampling): text [B, nt] token ids (-1 = padding),
 * seq_len [B] or NULL (= N): each sequence's frames; in, out [B, N, td] fp32, distinct. Valid tokens are those with
 * id != -1 at positions below min(nt, seq_len[b]); with T of them, base = seq_len / T and rem = seq_len % T, the first
 * T - rem repeat base times and the last rem repeat base + 1 times over frames [0, seq_len); later frames, and all of
 * them when T == 0, are zero. N <= 8192, td % 4 == 0. */
int f5h_op_text_upsample(void* stream, int32_t B, int32_t nt, int32_t N, int32_t td, const int64_t* text,
                         const int32_t* seq_len, const float* in, float* out);
/* lnfold_uv alone (16-bit modes): table [rows, stride] fp32 holds, per ODE step s < nfe, the AdaLN modulation rows
 * of `depth` layers ([depth][6][d]: shift_msa, scale_msa, gate_msa, shift_mlp, scale_mlp, gate_mlp) in its first
 * 6 d depth floats; the kernel writes, per step and layer l, at column out_off + l (2F + 6d): u1 [F], v1 [F] (FFN1,
 * mlp rows), u2 [3d], v2 [3d] (QKV, msa rows), u = sum_k (1 + sc_k) W[n,k], v = sum_k sh_k W[n,k]. W1 [depth,F,d]
 * and Wqkv [depth,3d,d] fp32, rounded to the operand dtype on the device. The table is updated in place (rows >=
 * nfe are the caller's guard). d % 64 == 0, F % 64 == 0, out_off >= 6 d depth, stride % 4 == 0,
 * stride >= out_off + depth (2F + 6d). */
int f5h_op_lnfold_uv(void* stream, int32_t compute, int32_t nfe, int32_t depth, int32_t d, int32_t F, float* table,
                     int64_t stride, int64_t out_off, const float* W1, const float* Wqkv, void* workspace,
                     size_t workspace_bytes);
/* scale_cols alone (16-bit modes): out[n][k] = round(round(W[n][k]) g[k]); W, out [rows, K] fp32 views of the 16-bit
 * buffers, g [K]. K % 8 == 0. */
int f5h_op_scale_cols(void* stream, int32_t compute, int64_t rows, int32_t K, const float* W, const float* g,
                      float* out, void* workspace, size_t workspace_bytes);

/* The ragged forms of the three ops that reach across rows, over S sequences as packed rows: seg_off is a HOST table
 * [S + 1] from 0 to R with every length in [1, Lmax]. Each sequence's rows equal, bit for bit, the plain op on that
 * sequence alone (f5h_op_attention at N = its length, f5h_op_conv_pos at S = 1, L = its length, f5h_op_grn likewise).
 * Attention: Q, K, V are padded panels [S, H, Lmax, 64] of which sequence s holds seg_len[s] rows (the rest is never
 * read and may hold NaN); O [R, H*64] packed. Conv: x, resid, y [R, d] packed, taps outside a row's own segment read
 * zero; mode and x_as_f32 as f5h_op_conv_pos. GRN: x, out [R, C] packed. */
int f5h_op_attention_ragged(void* stream, int32_t compute, int32_t S, int32_t H, int32_t Lmax, int32_t R,
                            const int32_t* seg_off, const float* Q, const float* K, const float* V,
                            int32_t q_prescaled, float* O, void* workspace, size_t workspace_bytes);
int f5h_op_conv_pos_ragged(void* stream, int32_t compute, int32_t S, int32_t Lmax, int32_t R, int32_t d,
                           const int32_t* seg_off, const float* x, const float* w, const float* bias, int32_t mode,
                           const float* resid, int32_t x_as_f32, float* y, void* workspace, size_t workspace_bytes);
int f5h_op_grn_ragged(void* stream, int32_t compute, int32_t S, int32_t Lmax, int32_t R, int32_t C,
                      const int32_t* seg_off, const float* x, const float* gamma, const float* beta, float* out,
                      void* workspace, size_t workspace_bytes);

/* Op-level entry points of the audio glue, prologue and ODE step kernels (tests/test_gpu_glue_ops.py). Unlike the
 * hooks above these stage nothing: every pointer is a device pointer in the type the kernel reads or writes (a buffer
 * in the operand dtype is bf16 / fp16 memory, "(operand)" below), each hook makes one launcher call on `stream`, and
 * shapes outside the launcher's contract return F5H_EINVAL before any device work. Tables the kernel reads from
 * device memory (segment offsets, lengths, counters) cannot be checked here: the caller guarantees them.
 *
 * Log-mel front end. mel_frames: wav [B, L] -> frames [B * T, n_fft], T = 1 + L / hop, frame t of wave b =
 * wav[b][reflect(t hop + j - n_fft/2)] (torch.stft center=True, pad_mode "reflect"); L > n_fft / 2. The ragged form:
 * wave s is wav[s * wav_stride .. + len[s]), its frames are rows [frame_off[s], frame_off[s+1]) of frames [R, n_fft]
 * (frame_off [B+1], len [B]: device int32; every len[s] > n_fft / 2, frame_off[s+1] - frame_off[s] = 1 + len[s] / hop).
 * mel_mag: spec [rows, ld_spec] of interleaved (re, im) -> mag [rows, ld_mag] = |.| for columns < bins, 0 beyond.
 * mel_log: mel [B * T, n_mels] -> out [B, n_mels, T] = log(max(mel, 1e-5)) (NaN stays NaN). The ragged form: out
 * [B, T_out, n_mels], row t of wave s = log(max(mel[frame_off[s] + t], 1e-5)) for t < T_s, exact 0 up to T_out. */
int f5h_op_mel_frames(void* stream, int32_t B, int32_t L, int32_t n_fft, int32_t hop, const float* wav,
                      float* frames);
int f5h_op_mel_frames_ragged(void* stream, int32_t B, int32_t R, int32_t n_fft, int32_t hop, const float* wav,
                             int64_t wav_stride, const int32_t* frame_off, const int32_t* len, float* frames);
int f5h_op_mel_mag(void* stream, int64_t rows, int32_t bins, int32_t ld_spec, int32_t ld_mag, const float* spec,
                   float* mag);
int f5h_op_mel_log(void* stream, int32_t B, int32_t T, int32_t n_mels, const float* mel, float* out);
int f5h_op_mel_log_ragged(void* stream, int32_t B, int32_t T_out, int32_t n_mels, const float* mel,
                          const int32_t* frame_off, float* out);
/* Vocos decoder glue (compute: F5H_FP32 or F5H_BF16). imcol: the embed conv's im2col, mel [B, C, T] -> out
 * [B * T, Kp] (operand), out[b T + t][7 c + j] = mel[b][c][t + j - 3] (0 outside [0, T)), columns [7 C, Kp) zero;
 * Kp >= 7 C, Kp % 64 == 0. The ragged form gathers from src[s row_stride + (start[s] + q) frame_stride + c chan_stride]
 * into packed rows [seg_off[s], seg_off[s+1]) of out [R, Kp], taps outside the utterance's own frames zero (seg_off
 * [B+1], start [B]: device int32). spec: rows of ld floats in place, columns (2k, 2k+1) = (log-magnitude m, phase p)
 * of bin k < bins become min(exp(m), 100) (cos p, sin p) (NaN in m or p stays NaN), columns [2 bins, ld) zero.
 * ola: frames [B * T, n_fft] (already windowed), win [n_fft] -> y [B, (T - 1) hop], torch.istft(center=True)'s
 * overlap-add over the squared-window envelope; T = 1 launches nothing; n_fft % hop == 0. The ragged form: packed
 * frames [R, n_fft], utterance s at sample (seg_off[s] - s) hop of y, (len_s - 1) hop samples. */
int f5h_op_vocos_imcol(void* stream, int32_t compute, int32_t B, int32_t T, int32_t C, int32_t Kp, const float* mel,
                       void* out);
int f5h_op_vocos_imcol_ragged(void* stream, int32_t compute, int32_t B, int32_t R, int32_t C, int32_t Kp,
                              const float* src, int64_t row_stride, int64_t frame_stride, int64_t chan_stride,
                              const int32_t* seg_off, const int32_t* start, void* out);
int f5h_op_vocos_spec(void* stream, int64_t rows, int32_t bins, int32_t ld, float* x);
int f5h_op_vocos_ola(void* stream, int32_t B, int32_t T, int32_t n_fft, int32_t hop, const float* frames,
                     const float* win, float* y);
int f5h_op_vocos_ola_ragged(void* stream, int32_t B, int32_t R, int32_t n_fft, int32_t hop, const float* frames,
                            const float* win, const int32_t* seg_off, float* y);
/* Sampler prologue. time_sinus: t [n] (a HOST array, or device memory when t_on_device) -> out [n, 256] =
 * [sin | cos](1000 t exp(-j ln 1e4 / 127)), 1 <= n <= 512. rope_table: out [L, 32, 2] (cos, sin)(n 10000^(-2j/64)).
 * text_embed (TextEmbedding.forward, both CFG branches): text [B, nt] int64 (-1 = filler), seq_len [B] or NULL, table
 * [V, td], freqs [rows, td] or NULL (freq_rows > 0: position n reads row min(n, freq_rows - 1)) -> out_c, out_u
 * [B, N, td], keep [2 B N] bytes or NULL; with seg_off [B+1] (device) N counts packed rows and the outputs are
 * [N, td], keep [2 N]. build_ct: the input projection's operand [S N, 128 + roundup(td, 64)] (operand) from cond
 * [B, N, 100], cond_mask [B N] bytes and the text embeddings [B, N, td]; S = B or 2 B. pack_y: y [rows, mel] ->
 * ypad [rows, 128] (operand), columns >= mel zero. masks, by kind: 0 rowkeep: src = dur [B] int32 -> out [S L] bytes
 * (pos < off or pos - off < dur[s % B]); 1 kvlen: out [S] int32 = dur[s % B] + off (L unused); 2 textkeep: src = text
 * [B, L] int64 -> out [S L] bytes (!= -1); 3 textlen: out [S] int32 = 1 + the last position != -1 (0: none). S % B
 * == 0. final_where_out: out = where(cond_mask, cond, y) over [B, N, mel], all NaN when *fault != 0 (fault NULL:
 * never). copy_pred: dst [S, L - row_off, mel] = p[(s L + row_off + n) p_ld + c], all NaN when *fault != 0. */
int f5h_op_time_sinus(void* stream, int32_t t_on_device, int32_t n, const float* t, float* out);
int f5h_op_rope_table(void* stream, int32_t L, float* out);
int f5h_op_text_embed(void* stream, int32_t B, int32_t nt, int32_t N, int32_t td, const int64_t* text,
                      const int32_t* seq_len, const float* table, const float* freqs, int32_t freq_rows,
                      int32_t mask_padding, float* out_c, float* out_u, uint8_t* keep, const int32_t* seg_off);
int f5h_op_build_ct(void* stream, int32_t compute, int32_t B, int32_t N, int32_t td, int32_t S, int32_t drop_audio,
                    int32_t drop_text, const float* cond, const uint8_t* cond_mask, const float* text_c,
                    const float* text_u, void* out);
int f5h_op_pack_y(void* stream, int32_t compute, int32_t rows, int32_t mel, const float* y, void* ypad);
int f5h_op_masks(void* stream, int32_t kind, int32_t B, int32_t S, int32_t L, int32_t off, const void* src,
                 void* out);
int f5h_op_final_where_out(void* stream, int32_t B, int32_t N, int32_t mel, const float* cond,
                           const uint8_t* cond_mask, const float* y, float* out, const uint32_t* fault);
int f5h_op_copy_pred(void* stream, int32_t S, int32_t L, int32_t row_off, int32_t mel, int64_t p_ld, const float* p,
                     float* dst, const uint32_t* fault);
/* CFG + one ODE update launch. v = pc + (pc - pu) cfg (pc alone when !use_cfg) with pc = p[b p_seq_stride +
 * (p_row_off + n) p_ld + c] and pu the same of sequence B + b. f5h_op_cfg_euler (method 0): y += dt v, the new y also
 * to ypad [B N, 128] (operand, or NULL) and to the trajectory slot. Host form (kstep NULL): dt and traj (a slot, or
 * NULL) as given. Device-indexed form: k = *kstep, dt = tgrid[k+1] - tgrid[k], slot (*trajp) + (k + 1) B N mel
 * (trajp NULL or *trajp NULL: none); next_dst[0, next_n) = next_src[(k + 1) next_stride ..] while k + 1 < nfe; with
 * arrive (zero before the launch) the last workgroup sets *kstep = k + 1, *arrive = 0 and bumps *tick (or NULL).
 * f5h_op_cfg_rk (method 1 midpoint, 2 rk4): one evaluation e = *kstep of neval = nfe, step k = e / stages, stage
 * e % stages; a non-final stage writes the next stage point to ypad only (rk4 keeps its slope in kbuf [3][B N mel]),
 * the final stage updates y, ypad and trajectory slot k + 1; table row e + 1 and the counter as above. mel <= 128. */
typedef struct f5h_op_step_args {
  int32_t compute, method;
  int32_t B, N, mel, use_cfg;
  float cfg, dt;
  float* y;
  const float* p;
  int64_t p_seq_stride, p_ld;
  int32_t p_row_off, nfe;
  void* ypad;
  float* traj;
  float* kbuf;
  int32_t* kstep;
  const float* tgrid;
  float* const* trajp;
  const float* next_src;
  int64_t next_stride;
  int32_t next_n;
  float* next_dst;
  uint32_t* arrive;
  int32_t* tick;
} f5h_op_step_args;
int f5h_op_cfg_euler(void* stream, const f5h_op_step_args* args);
int f5h_op_cfg_rk(void* stream, const f5h_op_step_args* args);

/* Tuning/test hook: pin the 16-bit GEMM tile configuration for all later launches in this
 * process (0, 1, 5, 11, 12, 13), or -1 to restore the automatic per-shape choice. */
int f5h_gemm_force_config(int32_t cfg);
/* Test hook: on != 0 makes every later 16-bit attention launch of this process rerun each workgroup's key
 * loop in its lazy-running-max form (the path a row takes when a score runs far above its first tile's max;
 * attention.hip), 0 restores the default. Results agree to rounding (tests/test_gpu_parity.py). */
int f5h_attn_force_safe(int32_t on);
/* Test hook (host only, no device needed): the batch path's pad-row skip test of a GEMM row tile
 * (modules.py:551-553): 1 if rows [m0, m0 + BM) of an M-row operand hold a live row, where sequence s owns
 * rows [s*live_seq, (s+1)*live_seq) and its first live_len[s] rows are live; 0 if every row is padding.
 * The device kernels run the same function (kernels.h tile_live_rows). */
int f5h_debug_tile_live(const int32_t* live_len, int32_t live_seq, int32_t M, int32_t m0, int32_t BM);
/* Test hook (host only, no device needed): the multiply-shift division of the kernels' launch heads (kernels.h
 * magic_div_make / magic_div, which turn a workgroup id into tile indices) against `/` and `%`: for every divisor d
 * in [d_lo, d_hi] and every numerator n in [0, n_end), counts the (n, d) whose quotient or remainder differs and
 * returns the count (0: exact over the whole range), or -1 for a bad range. limits (or null): receives the ranges
 * the launchers allow, {largest numerator + 1, largest divisor}. */
int64_t f5h_debug_magic_div_sweep(uint32_t n_end, uint32_t d_lo, uint32_t d_hi, uint32_t* limits);
/* Test hook (host only, no device, no engine, and the environment is not read): the engine's decision which modes a
 * call runs in (the phase chain, the norm folds, the MXFP8 classes, the residual dtype, the pad-row skip, the two CFG
 * chains), as every sample / forward call takes it once at its start. in[21]: backbone, dim, qk_norm,
 * long_skip_connection, compute (f5h_compute; MXFP8 engines pass BF16), LayerNorm fold supported, RMSNorm fold
 * supported, chain fault word present, MXFP8 engine, then the switches chain, ln_fold, pad_skip, graph_mode,
 * cfg_streams (0 / 1 / 2), mx8 class mask, probed class (-1: none), then F5H_RES32, F5H_DIAG_SKIP_LN, then the call's
 * use_cfg, batch mask, ragged. out[12]: mx8 classes in use, 16-bit residual, LayerNorms run, two CFG chains, the call
 * may chain (before the per-device admission), its launches chain, a norm fold runs (call level), LayerNorm fold on,
 * RMSNorm fold on, the in-place out-projection skips pad-row tiles, and pad_skip and the probed class as given.
 * Returns F5H_EINVAL unless n_in == 21 and n_out == 12. */
int f5h_debug_step_modes(const int32_t* in, int32_t n_in, int32_t* out, int32_t n_out);

/* ---------------------------------------------------------------------------------------
 * Vocos decoder (mel -> waveform), SURVEY §8(f1): the step after the CFM path, replacing
 * `vocoder.decode(mel)` (infer/utils_infer.py:510-511; runtime/triton_trtllm/benchmark.py:435)
 * of the vocos package's mel-24khz model (Vocos.decode = backbone + ISTFTHead). Weights by the
 * vocos state-dict names ("backbone.embed.weight", "backbone.convnext.{i}.pwconv1.weight",
 * "head.out.weight", ...), fp32 host arrays. compute: F5H_BF16 runs the backbone GEMMs on bf16
 * MFMA; the head and the inverse STFT always run in fp32. */
typedef struct f5h_vocos_arch {
  int32_t input_channels;    /* 100 mel bins */
  int32_t dim;               /* 512 */
  int32_t intermediate_dim;  /* 1536 */
  int32_t num_layers;        /* 8 */
  int32_t n_fft;             /* 1024 (win_length = n_fft, hann, center padding) */
  int32_t hop_length;        /* 256 */
  int32_t compute;           /* f5h_compute */
} f5h_vocos_arch;
typedef struct f5h_vocos f5h_vocos;

int f5h_vocos_create(const f5h_vocos_arch* arch, const f5h_weight* weights, int32_t n_weights, int32_t device,
                     f5h_vocos** out);
void f5h_vocos_destroy(f5h_vocos* v);
size_t f5h_vocos_workspace_size(const f5h_vocos* v, int32_t B, int32_t T);
/* mel [B][input_channels][T] fp32 (vocos' channel-first layout) -> audio [B][(T-1)*hop] fp32
 * (torch.istft center=True length). Device pointers; work enqueued on `stream`. */
int f5h_vocos_decode(f5h_vocos* v, void* stream, int32_t B, int32_t T, const float* mel, float* audio,
                     void* workspace, size_t workspace_bytes);
/* A batch of B utterances of unequal length in one pass (the eval driver's per-utterance
 * `gen[ref_len:total_len]` -> `vocoder.decode`, eval/eval_infer_batch.py:202-212). Utterance i is frames
 * [starts[i], starts[i] + lens[i]) of row i of `feats`, read in place through element strides:
 * feats[i*row_stride + t*frame_stride + c*chan_stride], so both the sampler's [B][N][C] output and vocos'
 * [B][C][T] layout are sources without a slice, permute or copy. The utterances run as packed rows with no padding
 * rows; the convolutions and the overlap-add stop at each utterance's own ends, so every wave equals
 * f5h_vocos_decode of that utterance alone bit for bit (zero-padding to one length does not: the convolutions
 * reach 27 frames across a boundary). audio_packed: utterance i at sum_{j<i} (lens[j] - 1)*hop, (lens[i] - 1)*hop
 * samples (none for lens[i] = 1). starts / lens are HOST arrays, consumed before the call returns (the caller may
 * free or overwrite them at once); the call does not synchronise the device or the stream. F5H_EINVAL names the
 * offending row for lens[i] < 1, starts[i] < 0 and a total above 2^24 frames. */
size_t f5h_vocos_ragged_workspace_size(const f5h_vocos* v, int32_t B, int64_t total_frames);
int f5h_vocos_decode_ragged(f5h_vocos* v, void* stream, int32_t B, const float* feats, int64_t row_stride,
                            int64_t frame_stride, int64_t chan_stride, const int32_t* starts, const int32_t* lens,
                            float* audio_packed, void* workspace, size_t workspace_bytes);

/* ---------------------------------------------------------------------------------------
 * Log-mel front end (wav -> mel), SURVEY §8(f2): replaces get_vocos_mel_spectrogram
 * (model/modules.py:80-109; torchaudio MelSpectrogram power 1, center/reflect, periodic Hann,
 * htk filterbank without norm, f_max = sr/2; then clamp(1e-5).log()), which CFM.sample applies
 * to raw-audio conditioning (cfm.py:106-108). fp32 throughout (DFT and filterbank on fp32 MFMA). */
typedef struct f5h_mel_arch {
  int32_t n_fft;        /* 1024 (= win_length) */
  int32_t hop_length;   /* 256 */
  int32_t n_mels;       /* 100 */
  int32_t sample_rate;  /* 24000 */
} f5h_mel_arch;
typedef struct f5h_mel f5h_mel;

int f5h_mel_create(const f5h_mel_arch* arch, int32_t device, f5h_mel** out);
void f5h_mel_destroy(f5h_mel* m);
/* frames T = 1 + L / hop (torch.stft center=True); L must exceed n_fft/2 (reflect padding) */
size_t f5h_mel_workspace_size(const f5h_mel* m, int32_t B, int32_t L);
/* wav [B][L] fp32 -> mel [B][n_mels][T] fp32 (device pointers, enqueued on `stream`) */
int f5h_mel_forward(f5h_mel* m, void* stream, int32_t B, int32_t L, const float* wav, float* mel, void* workspace,
                    size_t workspace_bytes);
/* B waves of unequal length in one pass (the eval driver computes each prompt's log-mel separately and pads
 * the mels, eval/utils_eval.py:58-66,130). Wave i is wav[i*wav_stride .. + lens[i]) and gives T_i = 1 + lens[i]/hop
 * frames, reflected at its own end; cond [B][T_out][n_mels] (frame-major, the layout CFM.sample takes) holds them
 * with exact zeros for frames >= T_i, i.e. the zero-padded batch of the per-wave log-mels, bit for bit.
 * total_frames = sum T_i. lens is a HOST array, consumed before the call returns; no synchronisation.
 * F5H_EINVAL names the offending wave for lens[i] <= n_fft/2, T_i > T_out and a total above 2^24 frames. */
size_t f5h_mel_ragged_workspace_size(const f5h_mel* m, int32_t B, int64_t total_frames);
int f5h_mel_forward_ragged(f5h_mel* m, void* stream, int32_t B, const float* wav, int64_t wav_stride,
                           const int32_t* lens, int32_t T_out, float* cond, void* workspace, size_t workspace_bytes);

const char* f5h_last_error(void);
const char* f5h_version(void);

#ifdef __cplusplus
}
#endif
#endif /* F5H_H */
