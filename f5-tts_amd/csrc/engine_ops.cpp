// f5h engine: op-level entry points and debug hooks, called by the test suite only, never by the product path (see
// engine_internal.h for the map of the engine's files).
#include "engine_internal.h"

extern "C" {

static bool op_compute_ok(int32_t compute) { return compute >= F5H_FP32 && compute <= F5H_FP16; }
// caller workspace as a bump allocator: null when it does not fit (fits() then fails the call)
struct OpWs {
  WS ws;
  size_t bytes;
  size_t end = 0;  // where the last buffer taken ends (ws.off pads it to the next 256 bytes)
  OpWs(void* base, size_t n) : bytes(n) { ws.base = reinterpret_cast<char*>(base); }
  void* take(size_t n) {
    end = ws.off + n;
    return ws.take<char>(n);
  }
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
  if (method < 0 || method >= kOdeMethods || !op_compute_ok(compute) || !t_grid || steps <= 0 || !out)
    return fail(F5H_EINVAL, "bad ode_eval_times argument");
  ode_eval_times(method, compute, t_grid, steps, out);
  return 0;
}

// ---------------------------------------------------------------- op-level entry points
int f5h_op_linear(void* stream, int32_t compute, int32_t M, int32_t N, int32_t K, const float* A, const float* W,
                  const float* bias, float* C, void* workspace, size_t workspace_bytes) {
  if (M <= 0 || N <= 0 || K <= 0 || K % 64) return fail(F5H_EINVAL, "op_linear needs K % 64 == 0");
  if (!op_compute_ok(compute)) return fail(F5H_EINVAL, "bad compute mode");
  const int Npad = (N + 127) / 128 * 128;
  const size_t es = compute ? 2 : 4;
  const size_t need = (size_t)Npad * K * es;
  OpWs ws(workspace, workspace_bytes);
  void* wop = ws.take(need);
  void* aop = ws.take((size_t)M * K * es);  // (asked for in the fp32 mode too, which reads A in place)
  // the bytes this hook has always asked for: the last buffer without its padding
  if (ws.end > workspace_bytes) return fail(F5H_ENOMEM, "workspace too small for op_linear");
  hipStream_t st = reinterpret_cast<hipStream_t>(stream);
  HIPCK(hipMemsetAsync(wop, 0, need, st));
  HIPCK(f32_to_op(compute, W, (int64_t)N * K, wop, st));
  if (compute) HIPCK(f32_to_op(compute, A, (int64_t)M * K, aop, st));
  GemmArgs g{};
  g.A = compute ? aop : A;
  g.lda = K;
  g.W = wop;
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

int f5h_debug_tile_live(const int32_t* live_len, int32_t live_seq, int32_t M, int32_t m0, int32_t BM) {
  if (live_seq <= 0 || M <= 0 || BM <= 0 || m0 < 0 || m0 >= M) return fail(F5H_EINVAL, "bad tile");
  return tile_live_rows(live_len, live_seq, M, m0, BM) ? 1 : 0;
}

int64_t f5h_debug_magic_div_sweep(uint32_t n_end, uint32_t d_lo, uint32_t d_hi, uint32_t* limits) {
  if (limits) {
    limits[0] = kMagicMaxN;
    limits[1] = kMagicMaxD;
  }
  if (d_lo == 0 || d_hi < d_lo || n_end > 0x7fffffffu) return -1;
  int64_t bad = 0;
  for (uint32_t d = d_lo; d <= d_hi; ++d) {
    const MagicDiv m = magic_div_make(d);
    for (uint32_t n = 0; n < n_end; ++n) {
      const uint32_t q = magic_div(n, m.mul, m.shift);
      bad += (q != n / d) | (n - q * d != n % d);
    }
  }
  return bad;
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
  if (!op_compute_ok(compute)) return fail(F5H_EINVAL, "bad compute mode");
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

// Both conv_pos hooks, after their own validation. x holds nx elements and y ny. seg_off (host, [S + 1]): the ragged
// form over packed rows, L = the longest segment; otherwise rowkeep and the y placement apply.
static int op_conv_pos_impl(const char* what, void* stream, int32_t compute, int32_t S, int32_t L, int32_t d,
                            int64_t nx, int64_t ny, const int32_t* seg_off, const float* x, const float* w,
                            const float* bias, const uint8_t* rowkeep, int32_t mode, const float* resid,
                            int32_t x_as_f32, int64_t y_seq_stride, int64_t y_row_off, float* y, void* workspace,
                            size_t workspace_bytes) {
  hipStream_t st = reinterpret_cast<hipStream_t>(stream);
  const size_t es = compute ? 2 : 4;
  OpWs ws(workspace, workspace_bytes);
  void* wp = ws.take(kConvPackElems * es);
  int32_t* off = seg_off ? reinterpret_cast<int32_t*>(ws.take((size_t)(S + 1) * 4)) : nullptr;
  void* xop = (compute && !x_as_f32) ? ws.take((size_t)nx * es) : nullptr;
  const bool y16 = compute && mode != 1;
  void* yop = y16 ? ws.take((size_t)ny * es) : nullptr;
  OPWS_CHECK(ws, what);
  HIPCK(hipMemsetAsync(wp, 0, kConvPackElems * es, st));
  RC(pack_conv_weight(w, F5H_DT_F32, d, wp, compute, st));
  ConvArgs cv{};
  cv.S = S;
  cv.L = L;
  cv.d = d;
  cv.rowkeep = rowkeep;
  if (seg_off) {
    HIPCK(seg_upload(seg_off, S + 1, off, st));
    cv.ragged = 1;
    cv.rowkeep = reinterpret_cast<const uint8_t*>(off);
  }
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

int f5h_op_conv_pos_ragged(void* stream, int32_t compute, int32_t S, int32_t Lmax, int32_t R, int32_t d,
                           const int32_t* seg_off, const float* x, const float* w, const float* bias, int32_t mode,
                           const float* resid, int32_t x_as_f32, float* y, void* workspace, size_t workspace_bytes) {
  if (!op_compute_ok(compute)) return fail(F5H_EINVAL, "bad compute mode");
  if (d <= 0 || d % 128 || d > 1024) return fail(F5H_EINVAL, "op_conv_pos_ragged needs d % 128 == 0 and d <= 1024");
  if (mode < 0 || mode > 2 || (mode == 2 && !compute)) return fail(F5H_EINVAL, "op_conv_pos_ragged: bad mode");
  if (!x || !w || !bias || !y || (mode != 0 && !resid)) return fail(F5H_EINVAL, "op_conv_pos_ragged: null tensor");
  RC(op_seg_check("op_conv_pos_ragged", seg_off, S, R, Lmax));
  if ((int64_t)R * d >= (int64_t)1 << 31) return fail(F5H_EINVAL, "op_conv_pos_ragged: R * d must stay below 2^31");
  const int64_t nx = (int64_t)R * d;
  return op_conv_pos_impl("op_conv_pos_ragged", stream, compute, S, Lmax, d, nx, nx, seg_off, x, w, bias, nullptr, mode,
                          resid, x_as_f32, 0, 0, y, workspace, workspace_bytes);
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
  return op_conv_pos_impl("op_conv_pos", stream, compute, S, L, d, (int64_t)S * L * d, (int64_t)S * y_seq_stride * d,
                          nullptr, x, w, bias, rowkeep, mode, resid, x_as_f32, y_seq_stride, y_row_off, y, workspace,
                          workspace_bytes);
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
    if (a->ld_add > 0x7fffffff || dual > 0x7fffffff)
      return fail(F5H_EINVAL, "op_gemm_epi: ld_add and dual_rows are 32-bit in the launch arguments");
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
  g.ld_add = (int)a->ld_add;
  g.dual_rows = (int)dual;
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

// ---------------------------------------------------------------- MXFP8 hooks (kernels.h 'MXFP8 operands')
int f5h_debug_mx8_quant_block(const float* v32, uint8_t* q32, uint8_t* scale) {
  if (!v32 || !q32 || !scale) return fail(F5H_EINVAL, "mx8_quant_block: null argument");
  uint32_t bits[32], amax = 0;
  std::memcpy(bits, v32, sizeof(bits));
  for (uint32_t b : bits) amax = std::max(amax, b & 0x7FFFFFFFu);
  const uint8_t sb = mx8_scale_byte(amax);
  float mult;
  const uint32_t mb = mx8_unscale_bits(sb);
  std::memcpy(&mult, &mb, 4);
  for (int i = 0; i < 32; ++i) {
    uint32_t u = bits[i];
    if ((u & 0x7FFFFFFFu) < 0x7F800000u) {
      float v;
      std::memcpy(&v, &u, 4);
      const volatile float p = v * mult;  // one fp32 multiply by a power of two, as the device's
      const float pv = p;
      std::memcpy(&u, &pv, 4);
    }
    q32[i] = mx8_e4m3(u);
  }
  *scale = sb;
  return 0;
}

int f5h_op_quant_mx8(void* stream, int64_t M, int32_t K, const float* x, uint8_t* q, uint8_t* s, void* workspace,
                     size_t workspace_bytes) {
  if (M <= 0 || K <= 0 || K % 32 || M * (int64_t)K >= (1ll << 40)) return fail(F5H_EINVAL, "op_quant_mx8 needs M > 0 and K % 32 == 0");
  if (!x || !q || !s) return fail(F5H_EINVAL, "op_quant_mx8: null tensor");
  hipStream_t st = reinterpret_cast<hipStream_t>(stream);
  OpWs ws(workspace, workspace_bytes);
  void* xop = ws.take((size_t)M * K * 2);
  OPWS_CHECK(ws, "op_quant_mx8");
  HIPCK(f32_to_op(F5H_C_BF16, x, M * K, xop, st));
  HIPCK(quant_rows_mx8(xop, M, K, q, s, st));
  return 0;
}

int f5h_op_ln_modulate_mx8(void* stream, int32_t h16, int32_t M, int32_t d, const float* h, const float* shift,
                           const float* scale, uint8_t* q, uint8_t* s, void* workspace, size_t workspace_bytes) {
  if (M <= 0 || d <= 0 || d % 32 || d > 2048) return fail(F5H_EINVAL, "op_ln_modulate_mx8 needs d % 32 == 0 and d <= 2048");
  if (!h || !shift || !scale || !q || !s) return fail(F5H_EINVAL, "op_ln_modulate_mx8: null tensor");
  hipStream_t st = reinterpret_cast<hipStream_t>(stream);
  OpWs ws(workspace, workspace_bytes);
  void* hop = h16 ? ws.take((size_t)M * d * 2) : nullptr;
  OPWS_CHECK(ws, "op_ln_modulate_mx8");
  if (hop) HIPCK(f32_to_op(F5H_C_BF16, h, (int64_t)M * d, hop, st));
  HIPCK(ln_modulate_mx8(hop ? hop : (const void*)h, h16 ? 1 : 0, M, d, shift, scale, q, s, st));
  return 0;
}

int f5h_op_gemm_mx8(void* stream, const f5h_op_gemm_args* a, uint8_t* a8_out, uint8_t* as_out, uint8_t* w8_out,
                    uint8_t* ws_out, void* workspace, size_t workspace_bytes) {
  if (!a) return fail(F5H_EINVAL, "op_gemm_mx8: null args");
  const int epi = a->epi, M = a->M, N = a->N, K = a->K;
  if (epi != EPI_QKV && epi != EPI_RESID16 && epi != EPI_GELU_TANH)
    return fail(F5H_EINVAL, "op_gemm_mx8: the epilogue must be 2 (GELU_TANH), 7 (QKV) or 9 (RESID16)");
  if (M <= 0 || N <= 0 || K <= 0 || K % 128) return fail(F5H_EINVAL, "op_gemm_mx8 needs K % 128 == 0");
  if (!a->A || !a->W) return fail(F5H_EINVAL, "op_gemm_mx8: null operand");
  if (a->A2 || a->add || a->dual_rows || a->live_len || a->ln_part_in || a->ln_part_out || a->hs_scale || a->hs_out ||
      a->ln_u || a->ln_v || a->ln_rms || a->ln_nparts)
    return fail(F5H_EINVAL, "op_gemm_mx8: A2, add, live_len and the fold fields have no MX8 form");
  const bool resid_epi = epi == EPI_RESID16;
  if ((a->resid || a->gate || a->rowkeep) && !resid_epi)
    return fail(F5H_EINVAL, "op_gemm_mx8: resid, gate and rowkeep go with EPI_RESID16");
  const bool rq = a->seg_off != nullptr;
  int inner = 0;
  if (rq) {
    if (epi != EPI_QKV) return fail(F5H_EINVAL, "op_gemm_mx8: seg_off goes with EPI_QKV");
    if (a->qkv_dst_len <= 0 || a->seq_len != a->qkv_dst_len)
      return fail(F5H_EINVAL, "op_gemm_mx8: ragged EPI_QKV needs seq_len == qkv_dst_len > 0");
    RC(op_seg_check("op_gemm_mx8", a->seg_off, a->n_seq, M, a->qkv_dst_len));
  }
  if (epi == EPI_QKV) {
    inner = a->heads * 64;
    if (a->heads <= 0 || N != 3 * inner || a->seq_len <= 0 || (!rq && M % a->seq_len) || a->rope_heads < 0 ||
        a->rope_heads > a->heads || !a->q || !a->k || !a->v)
      return fail(F5H_EINVAL, "op_gemm_mx8: EPI_QKV needs N == 3 * heads * 64, M % seq_len == 0 and q, k, v");
    if (a->qkv_dst_len != 0 && a->qkv_dst_len < a->seq_len)
      return fail(F5H_EINVAL, "op_gemm_mx8: qkv_dst_len must be 0 or >= seq_len");
    if ((a->q_norm_w != nullptr) != (a->k_norm_w != nullptr) || (a->q_norm_w && !(a->qk_norm_eps >= 0.f)))
      return fail(F5H_EINVAL, "op_gemm_mx8: qk_norm needs q_norm_w, k_norm_w and qk_norm_eps >= 0");
  } else if (a->qkv_dst_len || a->q_norm_w || a->k_norm_w) {
    return fail(F5H_EINVAL, "op_gemm_mx8: qkv_dst_len and qk_norm go with EPI_QKV");
  } else if (!a->C) {
    return fail(F5H_EINVAL, "op_gemm_mx8: null C");
  }
  hipStream_t st = reinterpret_cast<hipStream_t>(stream);
  const int64_t nC = (int64_t)M * N, nA = (int64_t)M * K, nW = (int64_t)N * K;
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
  void* wop = ws.take((size_t)nW * 2);
  void* aop = ws.take((size_t)nA * 2);
  uint8_t* w8 = reinterpret_cast<uint8_t*>(ws.take((size_t)nW));
  uint8_t* wsc = reinterpret_cast<uint8_t*>(ws.take((size_t)nW / 32));
  uint8_t* a8 = reinterpret_cast<uint8_t*>(ws.take((size_t)nA));
  uint8_t* asc = reinterpret_cast<uint8_t*>(ws.take((size_t)nA / 32));
  void* cop = epi != EPI_QKV ? ws.take((size_t)nC * 2) : nullptr;
  void* rop = (resid_epi && a->resid) ? ws.take((size_t)nC * 2) : nullptr;
  void *qop = nullptr, *kop = nullptr, *vop = nullptr;
  float2* rope = nullptr;
  if (epi == EPI_QKV) {
    rope = reinterpret_cast<float2*>(ws.take((size_t)a->seq_len * 32 * sizeof(float2)));
    qop = ws.take((size_t)nqkv * 2);
    kop = ws.take((size_t)nqkv * 2);
    vop = ws.take((size_t)nqkv * 2);
  }
  int32_t* rq_off = rq ? reinterpret_cast<int32_t*>(ws.take((size_t)(a->n_seq + 1) * 4)) : nullptr;
  int2* rq_tab = rq ? reinterpret_cast<int2*>(ws.take((size_t)M * 8)) : nullptr;
  OPWS_CHECK(ws, "op_gemm_mx8");
  HIPCK(f32_to_op(F5H_C_BF16, a->W, nW, wop, st));
  HIPCK(f32_to_op(F5H_C_BF16, a->A, nA, aop, st));
  HIPCK(quant_rows_mx8(wop, N, K, w8, wsc, st));
  HIPCK(quant_rows_mx8(aop, M, K, a8, asc, st));
  GemmArgs g{};
  g.M = M;
  g.N = N;
  g.K = K;
  g.bias = a->bias;
  g.ldc = N;
  g.gate = a->gate;
  g.rowkeep = a->rowkeep;
  if (rq) {
    HIPCK(seg_upload(a->seg_off, a->n_seq + 1, rq_off, st));
    HIPCK(build_rowtab(rq_off, a->n_seq, M, rq_tab, nullptr, st));
    g.add = reinterpret_cast<const float*>(rq_tab);
  }
  if (cop) {
    if (resid_epi) HIPCK(f32_to_op(F5H_C_BF16, a->C, nC, cop, st));
    g.C = cop;
  }
  if (rop) {
    HIPCK(f32_to_op(F5H_C_BF16, a->resid, nC, rop, st));
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
    g.q = qop;
    g.k = kop;
    g.v = vop;
    g.q_norm_w = a->q_norm_w;
    g.k_norm_w = a->k_norm_w;
    g.qk_norm_eps = a->qk_norm_eps;
    g.qkv_dst_len = a->qkv_dst_len;
    // rows the launch does not own (and panel rows past a ragged sequence) come back as the caller's buffers hold them
    HIPCK(f32_to_op(F5H_C_BF16, a->q, nqkv, qop, st));
    HIPCK(f32_to_op(F5H_C_BF16, a->k, nqkv, kop, st));
    HIPCK(f32_to_op(F5H_C_BF16, a->v, nqkv, vop, st));
  }
  HIPCK(gemm_mx8(epi, g, Mx8Ops{a8, asc, w8, wsc, nullptr}, st));
  if (cop) HIPCK(op_to_f32(F5H_C_BF16, cop, nC, a->C, st));
  if (epi == EPI_QKV) {
    HIPCK(op_to_f32(F5H_C_BF16, qop, nqkv, a->q, st));
    HIPCK(op_to_f32(F5H_C_BF16, kop, nqkv, a->k, st));
    HIPCK(op_to_f32(F5H_C_BF16, vop, nqkv, a->v, st));
  }
  if (a8_out) HIPCK(hipMemcpyAsync(a8_out, a8, (size_t)nA, hipMemcpyDeviceToDevice, st));
  if (as_out) HIPCK(hipMemcpyAsync(as_out, asc, (size_t)nA / 32, hipMemcpyDeviceToDevice, st));
  if (w8_out) HIPCK(hipMemcpyAsync(w8_out, w8, (size_t)nW, hipMemcpyDeviceToDevice, st));
  if (ws_out) HIPCK(hipMemcpyAsync(ws_out, wsc, (size_t)nW / 32, hipMemcpyDeviceToDevice, st));
  return 0;
}

}  // extern "C"
