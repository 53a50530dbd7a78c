// f5h engine: op-level entry points of the audio glue (melspec.hip, vocos.hip), prologue and ODE step kernels
// (elementwise.hip), called by the test suite only (tests/test_gpu_glue_ops.py), never by the product path. Each hook
// checks its arguments against the launcher's contract (F5H_EINVAL before any device work), then makes one launcher
// call on the caller's stream with the caller's device pointers, in the types the kernel reads and writes: no
// staging, no workspace. Tables a kernel reads from device memory (segment offsets, lengths, step counters) are the
// caller's to get right; the Python wrappers build them from host values and check them there.
#include "engine_internal.h"

extern "C" {

#define GLUE_REQ(cond, msg)                        \
  do {                                             \
    if (!(cond)) return fail(F5H_EINVAL, (msg));   \
  } while (0)

static hipStream_t glue_stream(void* s) { return reinterpret_cast<hipStream_t>(s); }
static bool glue_compute_ok(int32_t compute) { return compute >= F5H_FP32 && compute <= F5H_FP16; }
// element counts the kernels index with 32-bit products stay below this
static constexpr int64_t kGlueMaxElems = (int64_t)1 << 30;

// ---------------------------------------------------------------- log-mel front end (melspec.hip)
int f5h_op_mel_frames(void* stream, int32_t B, int32_t L, int32_t n_fft, int32_t hop, const float* wav,
                      float* frames) {
  GLUE_REQ(B > 0 && L > 0 && n_fft > 0 && n_fft % 2 == 0 && hop > 0 && wav && frames,
           "op_mel_frames: bad shape or null tensor");
  GLUE_REQ(L > n_fft / 2, "op_mel_frames: reflect padding needs L > n_fft / 2");
  const int T = 1 + L / hop;
  GLUE_REQ((int64_t)B * T * n_fft < kGlueMaxElems, "op_mel_frames: too large");
  HIPCK(mel_frames(wav, B, L, T, n_fft, hop, frames, glue_stream(stream)));
  return 0;
}

int f5h_op_mel_frames_ragged(void* stream, int32_t B, int32_t R, int32_t n_fft, int32_t hop, const float* wav,
                             int64_t wav_stride, const int32_t* frame_off, const int32_t* len, float* frames) {
  GLUE_REQ(B > 0 && R >= B && n_fft > 0 && n_fft % 2 == 0 && hop > 0 && wav_stride > 0 && wav && frame_off && len &&
               frames,
           "op_mel_frames_ragged: bad shape or null tensor");
  GLUE_REQ((int64_t)R * n_fft < kGlueMaxElems, "op_mel_frames_ragged: too large");
  HIPCK(mel_frames_ragged(wav, wav_stride, frame_off, len, B, R, n_fft, hop, frames, glue_stream(stream)));
  return 0;
}

int f5h_op_mel_mag(void* stream, int64_t rows, int32_t bins, int32_t ld_spec, int32_t ld_mag, const float* spec,
                   float* mag) {
  GLUE_REQ(rows > 0 && bins > 0 && spec && mag, "op_mel_mag: bad shape or null tensor");
  GLUE_REQ(ld_spec % 2 == 0 && ld_spec >= 2 * bins && ld_mag >= bins,
           "op_mel_mag: needs an even ld_spec >= 2 bins and ld_mag >= bins");
  GLUE_REQ(rows * ld_mag < kGlueMaxElems && rows * ld_spec < kGlueMaxElems, "op_mel_mag: too large");
  HIPCK(mel_mag(spec, rows, bins, ld_spec, ld_mag, mag, glue_stream(stream)));
  return 0;
}

int f5h_op_mel_log(void* stream, int32_t B, int32_t T, int32_t n_mels, const float* mel, float* out) {
  GLUE_REQ(B > 0 && T > 0 && n_mels > 0 && mel && out, "op_mel_log: bad shape or null tensor");
  GLUE_REQ((int64_t)B * T * n_mels < kGlueMaxElems, "op_mel_log: too large");
  HIPCK(mel_log(mel, B, T, n_mels, out, glue_stream(stream)));
  return 0;
}

int f5h_op_mel_log_ragged(void* stream, int32_t B, int32_t T_out, int32_t n_mels, const float* mel,
                          const int32_t* frame_off, float* out) {
  GLUE_REQ(B > 0 && T_out > 0 && n_mels > 0 && mel && frame_off && out,
           "op_mel_log_ragged: bad shape or null tensor");
  GLUE_REQ((int64_t)B * T_out * n_mels < kGlueMaxElems, "op_mel_log_ragged: too large");
  HIPCK(mel_log_ragged(mel, frame_off, B, T_out, n_mels, out, glue_stream(stream)));
  return 0;
}

// ---------------------------------------------------------------- Vocos decoder glue (vocos.hip)
// (the Vocos engine runs fp32 or bf16 operands; its launchers know no fp16 form)
static bool vocos_compute_ok(int32_t compute) { return compute == F5H_FP32 || compute == F5H_BF16; }

int f5h_op_vocos_imcol(void* stream, int32_t compute, int32_t B, int32_t T, int32_t C, int32_t Kp, const float* mel,
                       void* out) {
  GLUE_REQ(vocos_compute_ok(compute), "op_vocos_imcol: compute must be fp32 or bf16");
  GLUE_REQ(B > 0 && T > 0 && C > 0 && mel && out, "op_vocos_imcol: bad shape or null tensor");
  GLUE_REQ(Kp >= C * 7 && Kp % 64 == 0, "op_vocos_imcol: needs Kp >= 7 C and Kp % 64 == 0");
  GLUE_REQ((int64_t)B * T * Kp < kGlueMaxElems, "op_vocos_imcol: too large");
  HIPCK(vocos_im2col(compute, mel, B, T, C, Kp, out, glue_stream(stream)));
  return 0;
}

int f5h_op_vocos_imcol_ragged(void* stream, int32_t compute, int32_t B, int32_t R, int32_t C, int32_t Kp,
                              const float* src, int64_t row_stride, int64_t frame_stride, int64_t chan_stride,
                              const int32_t* seg_off, const int32_t* start, void* out) {
  GLUE_REQ(vocos_compute_ok(compute), "op_vocos_imcol_ragged: compute must be fp32 or bf16");
  GLUE_REQ(B > 0 && R >= B && C > 0 && src && seg_off && start && out,
           "op_vocos_imcol_ragged: bad shape or null tensor");
  GLUE_REQ(Kp >= C * 7 && Kp % 64 == 0, "op_vocos_imcol_ragged: needs Kp >= 7 C and Kp % 64 == 0");
  GLUE_REQ(row_stride > 0 && frame_stride > 0 && chan_stride > 0, "op_vocos_imcol_ragged: strides must be positive");
  GLUE_REQ((int64_t)R * Kp < kGlueMaxElems, "op_vocos_imcol_ragged: too large");
  HIPCK(vocos_im2col_ragged(compute, src, row_stride, frame_stride, chan_stride, seg_off, start, B, R, C, Kp, out,
                            glue_stream(stream)));
  return 0;
}

int f5h_op_vocos_spec(void* stream, int64_t rows, int32_t bins, int32_t ld, float* x) {
  GLUE_REQ(rows > 0 && bins > 0 && x, "op_vocos_spec: bad shape or null tensor");
  GLUE_REQ(ld % 2 == 0 && ld >= 2 * bins, "op_vocos_spec: needs an even ld >= 2 bins");
  GLUE_REQ(rows * ld < kGlueMaxElems, "op_vocos_spec: too large");
  HIPCK(vocos_spec(x, rows, bins, ld, glue_stream(stream)));
  return 0;
}

int f5h_op_vocos_ola(void* stream, int32_t B, int32_t T, int32_t n_fft, int32_t hop, const float* frames,
                     const float* win, float* y) {
  GLUE_REQ(B > 0 && T >= 1 && n_fft > 0 && n_fft % 2 == 0 && hop > 0 && frames && win && y,
           "op_vocos_ola: bad shape or null tensor");
  GLUE_REQ(n_fft % hop == 0, "op_vocos_ola: needs n_fft % hop == 0");
  GLUE_REQ((int64_t)B * T * n_fft < kGlueMaxElems, "op_vocos_ola: too large");
  HIPCK(vocos_ola(frames, win, B, T, n_fft, hop, y, glue_stream(stream)));
  return 0;
}

int f5h_op_vocos_ola_ragged(void* stream, int32_t B, int32_t R, int32_t n_fft, int32_t hop, const float* frames,
                            const float* win, const int32_t* seg_off, float* y) {
  GLUE_REQ(B > 0 && R >= B && n_fft > 0 && n_fft % 2 == 0 && hop > 0 && frames && win && seg_off && y,
           "op_vocos_ola_ragged: bad shape or null tensor");
  GLUE_REQ(n_fft % hop == 0, "op_vocos_ola_ragged: needs n_fft % hop == 0");
  GLUE_REQ((int64_t)R * n_fft < kGlueMaxElems, "op_vocos_ola_ragged: too large");
  HIPCK(vocos_ola_ragged(frames, win, seg_off, B, R, n_fft, hop, y, glue_stream(stream)));
  return 0;
}

// ---------------------------------------------------------------- prologue (elementwise.hip)
int f5h_op_time_sinus(void* stream, int32_t t_on_device, int32_t n, const float* t, float* out) {
  GLUE_REQ(t && out, "op_time_sinus: null tensor");
  GLUE_REQ(n >= 1 && n <= 512, "op_time_sinus: needs 1 <= n <= 512");
  if (t_on_device)
    HIPCK(time_sinus_dev(t, n, out, glue_stream(stream)));
  else
    HIPCK(time_sinus(t, n, out, glue_stream(stream)));
  return 0;
}

int f5h_op_rope_table(void* stream, int32_t L, float* out) {
  GLUE_REQ(out, "op_rope_table: null tensor");
  GLUE_REQ(L >= 1 && L <= (1 << 20), "op_rope_table: needs 1 <= L <= 2^20");
  HIPCK(rope_table(L, reinterpret_cast<float2*>(out), glue_stream(stream)));
  return 0;
}

int f5h_op_text_embed(void* stream, int32_t B, int32_t nt, int32_t N, int32_t td, const int64_t* text,
                      const int32_t* seq_len, const float* table, const float* freqs, int32_t freq_rows,
                      int32_t mask_padding, float* out_c, float* out_u, uint8_t* keep, const int32_t* seg_off) {
  GLUE_REQ(B > 0 && nt > 0 && N > 0 && td > 0 && text && table && out_c && out_u,
           "op_text_embed: bad shape or null tensor");
  GLUE_REQ(freq_rows >= 0 && (freq_rows == 0 || freqs), "op_text_embed: freq_rows needs freqs");
  GLUE_REQ(!(seg_off && seq_len), "op_text_embed: seq_len is not read with seg_off");
  GLUE_REQ(!seg_off || N >= B, "op_text_embed: with seg_off, N counts the packed rows (>= B)");
  GLUE_REQ((int64_t)(seg_off ? 1 : B) * N * td < kGlueMaxElems, "op_text_embed: too large");
  TextEmbArgs a{};
  a.text = text;
  a.B = B;
  a.nt = nt;
  a.N = N;
  a.td = td;
  a.seq_len = seq_len;
  a.table = table;
  a.freqs = freqs;
  a.freq_rows = freq_rows;
  a.mask_padding = mask_padding ? 1 : 0;
  a.out_c = out_c;
  a.out_u = out_u;
  a.keep = keep;
  a.seg_off = seg_off;
  HIPCK(text_embed(a, glue_stream(stream)));
  return 0;
}

int f5h_op_build_ct(void* stream, int32_t compute, int32_t B, int32_t N, int32_t td, int32_t S, int32_t drop_audio,
                    int32_t drop_text, const float* cond, const uint8_t* cond_mask, const float* text_c,
                    const float* text_u, void* out) {
  GLUE_REQ(glue_compute_ok(compute), "op_build_ct: bad compute mode");
  GLUE_REQ(B > 0 && N > 0 && td > 0 && cond && cond_mask && text_c && text_u && out,
           "op_build_ct: bad shape or null tensor");
  GLUE_REQ(S == B || S == 2 * B, "op_build_ct: S must be B (one branch) or 2 B (both)");
  GLUE_REQ((int64_t)S * N * (128 + (td + 63) / 64 * 64) < kGlueMaxElems, "op_build_ct: too large");
  HIPCK(build_ct(compute, cond, cond_mask, text_c, text_u, B, N, td, S, drop_audio ? 1 : 0, drop_text ? 1 : 0, out,
                 glue_stream(stream)));
  return 0;
}

int f5h_op_pack_y(void* stream, int32_t compute, int32_t rows, int32_t mel, const float* y, void* ypad) {
  GLUE_REQ(glue_compute_ok(compute), "op_pack_y: bad compute mode");
  GLUE_REQ(rows > 0 && y && ypad, "op_pack_y: bad shape or null tensor");
  GLUE_REQ(mel >= 1 && mel <= 128, "op_pack_y: needs 1 <= mel <= 128");
  GLUE_REQ((int64_t)rows * 128 < kGlueMaxElems, "op_pack_y: too large");
  HIPCK(pack_y(compute, y, rows, mel, ypad, glue_stream(stream)));
  return 0;
}

int f5h_op_masks(void* stream, int32_t kind, int32_t B, int32_t S, int32_t L, int32_t off, const void* src,
                 void* out) {
  GLUE_REQ(kind >= 0 && kind <= 3, "op_masks: kind must be 0 (rowkeep), 1 (kvlen), 2 (textkeep) or 3 (textlen)");
  GLUE_REQ(B > 0 && S >= B && S % B == 0 && src && out, "op_masks: bad shape or null tensor");
  GLUE_REQ(kind == 1 || (L > 0 && (int64_t)S * L < kGlueMaxElems), "op_masks: bad row length");
  GLUE_REQ(off >= 0 && (kind < 2 || off == 0), "op_masks: off is a non-negative row offset (rowkeep, kvlen only)");
  hipStream_t st = glue_stream(stream);
  switch (kind) {
    case 0: HIPCK(build_rowkeep(static_cast<const int32_t*>(src), B, S, L, off, static_cast<uint8_t*>(out), st)); break;
    case 1: HIPCK(build_kvlen(static_cast<const int32_t*>(src), B, S, off, static_cast<int32_t*>(out), st)); break;
    case 2: HIPCK(build_textkeep(static_cast<const int64_t*>(src), B, S, L, static_cast<uint8_t*>(out), st)); break;
    default: HIPCK(build_textlen(static_cast<const int64_t*>(src), B, S, L, static_cast<int32_t*>(out), st));
  }
  return 0;
}

int f5h_op_final_where_out(void* stream, int32_t B, int32_t N, int32_t mel, const float* cond,
                           const uint8_t* cond_mask, const float* y, float* out, const uint32_t* fault) {
  GLUE_REQ(B > 0 && N > 0 && mel > 0 && cond && cond_mask && y && out, "op_final_where_out: bad shape or null tensor");
  GLUE_REQ((int64_t)B * N * mel < kGlueMaxElems, "op_final_where_out: too large");
  HIPCK(final_where_out(cond, cond_mask, y, out, B, N, mel, fault, glue_stream(stream)));
  return 0;
}

int f5h_op_copy_pred(void* stream, int32_t S, int32_t L, int32_t row_off, int32_t mel, int64_t p_ld, const float* p,
                     float* dst, const uint32_t* fault) {
  GLUE_REQ(S > 0 && L > 0 && mel > 0 && p && dst, "op_copy_pred: bad shape or null tensor");
  GLUE_REQ(row_off >= 0 && row_off < L, "op_copy_pred: row_off must lie in [0, L)");
  GLUE_REQ(p_ld >= mel, "op_copy_pred: needs p_ld >= mel");
  GLUE_REQ((int64_t)S * L * p_ld < kGlueMaxElems, "op_copy_pred: too large");
  HIPCK(copy_pred(p, S, L, row_off, mel, p_ld, dst, fault, glue_stream(stream)));
  return 0;
}

// ---------------------------------------------------------------- ODE step (elementwise.hip)
static int step_common_check(const char* what, const f5h_op_step_args* a) {
  const std::string w(what);
  if (!a) return fail(F5H_EINVAL, w + ": null arguments");
  if (!glue_compute_ok(a->compute)) return fail(F5H_EINVAL, w + ": bad compute mode");
  if (a->B <= 0 || a->N <= 0 || !a->y || !a->p) return fail(F5H_EINVAL, w + ": bad shape or null tensor");
  if (a->mel < 1 || a->mel > 128) return fail(F5H_EINVAL, w + ": needs 1 <= mel <= 128 (ypad rows hold 128)");
  if (a->p_ld < a->mel || a->p_row_off < 0 || a->p_seq_stride < (int64_t)(a->p_row_off + a->N) * a->p_ld)
    return fail(F5H_EINVAL, w + ": p needs p_ld >= mel and p_seq_stride >= (p_row_off + N) p_ld");
  if ((int64_t)a->B * a->N * 128 >= kGlueMaxElems) return fail(F5H_EINVAL, w + ": too large");
  if (a->next_dst && (!a->next_src || a->next_n <= 0 || a->next_n % 4 || a->next_stride % 4 || a->next_stride < a->next_n))
    return fail(F5H_EINVAL, w + ": next_dst needs next_src and next_n, next_stride multiples of 4");
  return 0;
}

int f5h_op_cfg_euler(void* stream, const f5h_op_step_args* a) {
  RC(step_common_check("op_cfg_euler", a));
  GLUE_REQ(a->method == F5H_EULER, "op_cfg_euler: method must be 0");
  if (a->kstep) {
    GLUE_REQ(a->tgrid && a->nfe > 0, "op_cfg_euler: the device-indexed form needs tgrid and nfe");
    GLUE_REQ(!a->traj, "op_cfg_euler: the device-indexed form takes its trajectory from trajp");
  } else {
    GLUE_REQ(!a->tgrid && !a->trajp && !a->next_dst && !a->arrive && !a->tick,
             "op_cfg_euler: tgrid, trajp, next_dst, arrive and tick belong to the device-indexed form (kstep)");
  }
  GLUE_REQ(!a->tick || a->arrive, "op_cfg_euler: tick is bumped with arrive");
  EulerArgs e{};
  e.y = a->y;
  e.B = a->B;
  e.N = a->N;
  e.mel = a->mel;
  e.p = a->p;
  e.p_seq_stride = a->p_seq_stride;
  e.p_row_off = a->p_row_off;
  e.p_ld = a->p_ld;
  e.use_cfg = a->use_cfg ? 1 : 0;
  e.cfg = a->cfg;
  e.dt = a->dt;
  e.ypad = a->ypad;
  e.compute = a->compute;
  e.traj = a->traj;
  e.kstep = a->kstep;
  e.tgrid = a->tgrid;
  e.trajp = a->trajp;
  e.next_src = a->next_src;
  e.next_stride = a->next_stride;
  e.next_n = a->next_n;
  e.next_dst = a->next_dst;
  e.nfe = a->nfe;
  e.arrive = a->arrive;
  e.tick = a->tick;
  HIPCK(cfg_euler(e, glue_stream(stream)));
  return 0;
}

int f5h_op_cfg_rk(void* stream, const f5h_op_step_args* a) {
  RC(step_common_check("op_cfg_rk", a));
  GLUE_REQ(a->method == F5H_MIDPOINT || a->method == F5H_RK4, "op_cfg_rk: method must be 1 (midpoint) or 2 (rk4)");
  GLUE_REQ(a->kstep && a->tgrid && a->ypad && a->nfe > 0, "op_cfg_rk: needs kstep (the evaluation counter), tgrid, ypad and nfe");
  GLUE_REQ(a->method != F5H_RK4 || a->kbuf, "op_cfg_rk: rk4 needs kbuf");
  GLUE_REQ(!a->traj, "op_cfg_rk: the trajectory comes from trajp");
  GLUE_REQ(!a->tick || a->arrive, "op_cfg_rk: tick is bumped with arrive");
  RkArgs r{};
  r.y = a->y;
  r.B = a->B;
  r.N = a->N;
  r.mel = a->mel;
  r.p = a->p;
  r.p_seq_stride = a->p_seq_stride;
  r.p_row_off = a->p_row_off;
  r.p_ld = a->p_ld;
  r.use_cfg = a->use_cfg ? 1 : 0;
  r.cfg = a->cfg;
  r.ypad = a->ypad;
  r.compute = a->compute;
  r.method = a->method;
  r.kbuf = a->kbuf;
  r.keval = a->kstep;
  r.sgrid = a->tgrid;
  r.trajp = a->trajp;
  r.next_src = a->next_src;
  r.next_stride = a->next_stride;
  r.next_n = a->next_n;
  r.next_dst = a->next_dst;
  r.neval = a->nfe;
  r.arrive = a->arrive;
  r.tick = a->tick;
  HIPCK(cfg_rk(r, glue_stream(stream)));
  return 0;
}

}  // extern "C"
