// Vocos decoder kernels (mel -> waveform), gfx950. SURVEY §8(f1).
//
// The network is vocos' mel-24khz decoder (vocos package, unpinned in the reference's
// pyproject.toml:42; called at utils_infer.py:510-511 and runtime/triton_trtllm/benchmark.py:435):
//   backbone: Conv1d(100, 512, k7, pad 3) -> LayerNorm(eps 1e-6) -> 8 x ConvNeXtBlock
//             (dwconv k7 -> LayerNorm -> Linear 512->1536 -> GELU(erf) -> Linear 1536->512 ->
//              gamma * . -> + residual) -> final LayerNorm
//   head:     Linear(512, n_fft + 2) -> mag = clip(exp(.), max 100), phase -> S = mag e^{i phase}
//             -> iSTFT(n_fft 1024, hop 256, hann 1024, center) (restated in-tree by
//             runtime/triton_trtllm/scripts/export_vocoder_to_onnx.py:45-60 + conv_stft.py:201-234)
// The GEMMs run on gemm(); this file holds the glue kernels around them: the embed im2col,
// the magnitude/phase -> (re, im) map and the overlap-add with window-envelope division.
#include "common.h"
#include "kernels.h"

namespace f5h {

static inline unsigned vblk(int64_t n, int t) { return (unsigned)((n + t - 1) / t); }

// out[(b*T + t)][c*7 + j] = mel[b][c][t + j - 3] (0 outside [0, T)); columns [C*7, Kp) zeroed.
// mel is vocos' channel-first [B][C][T] layout (the permute at utils_infer.py:508).
template <typename TO>
__global__ void vocos_im2col_kernel(const float* mel, int B, int T, int C, int Kp, TO* out) {
  const int64_t i = (int64_t)blockIdx.x * blockDim.x + threadIdx.x;
  if (i >= (int64_t)B * T * Kp) return;
  const int col = (int)(i % Kp);
  const int64_t row = i / Kp;
  const int b = (int)(row / T), t = (int)(row - (int64_t)b * T);
  float v = 0.f;
  if (col < C * 7) {
    const int c = col / 7, j = col - c * 7, q = t + j - 3;
    if (q >= 0 && q < T) v = mel[((int64_t)b * C + c) * T + q];
  }
  out[i] = from_f32<TO>(v);
}
hipError_t vocos_im2col(int compute, const float* mel, int B, int T, int C, int Kp, void* out, hipStream_t st) {
  if (Kp < C * 7 || Kp % 64) return hipErrorInvalidValue;
  const int64_t n = (int64_t)B * T * Kp;
  if (compute)
    hipLaunchKernelGGL(vocos_im2col_kernel<bf16>, dim3(vblk(n, 256)), dim3(256), 0, st, mel, B, T, C, Kp, (bf16*)out);
  else
    hipLaunchKernelGGL(vocos_im2col_kernel<float>, dim3(vblk(n, 256)), dim3(256), 0, st, mel, B, T, C, Kp,
                       (float*)out);
  return hipGetLastError();
}

// ISTFTHead.forward's pointwise part, in place on rows of ld floats: the head weight is packed
// so that columns (2k, 2k+1) = (log-magnitude, phase) of bin k; they become (re, im) =
// clip(exp(m), 100) * (cos p, sin p). Columns [2*bins, ld) are zeroed (K padding of the iDFT GEMM).
__global__ void vocos_spec_kernel(float* x, int64_t rows, int bins, int ld) {
  const int64_t i = (int64_t)blockIdx.x * blockDim.x + threadIdx.x;
  const int half = ld / 2;
  if (i >= rows * half) return;
  const int64_t r = i / half;
  const int k = (int)(i - r * half);
  float2* p = reinterpret_cast<float2*>(x + r * ld) + k;
  if (k >= bins) {
    *p = make_float2(0.f, 0.f);
    return;
  }
  const float2 mp = *p;
  // torch.clip(exp, max=1e2). A comparison, not fminf: C fminf returns the non-NaN operand and would turn a NaN
  // log-magnitude into magnitude 100; this way NaN propagates as in torch, and every other value has fminf's bits
  const float e = expf(mp.x);
  const float mag = e > 100.f ? 100.f : e;
  float s, c;
  sincosf(mp.y, &s, &c);
  *p = make_float2(mag * c, mag * s);
}
hipError_t vocos_spec(float* x, int64_t rows, int bins, int ld, hipStream_t st) {
  if (ld % 2 || ld < 2 * bins) return hipErrorInvalidValue;
  const int64_t n = rows * (ld / 2);
  hipLaunchKernelGGL(vocos_spec_kernel, dim3(vblk(n, 256)), dim3(256), 0, st, x, rows, bins, ld);
  return hipGetLastError();
}

// torch.istft(center=True) tail: the iDFT GEMM already produced windowed frames
// fr[b*T + t][j] = win[j] * irfft(S[b, :, t])[j]; here y[b][n] = sum_t fr[t][p - t*hop] /
// sum_t win^2[p - t*hop], p = n + n_fft/2, over the frames covering p (output length (T-1)*hop).
// Every sample sums its <= n_fft/hop frames in a fixed order (deterministic, no atomics).
__global__ void vocos_ola_kernel(const float* fr, const float* win, int B, int T, int n_fft, int hop, float* y) {
  const int Lout = (T - 1) * hop;
  const int64_t i = (int64_t)blockIdx.x * blockDim.x + threadIdx.x;
  if (i >= (int64_t)B * Lout) return;
  const int b = (int)(i / Lout), n = (int)(i - (int64_t)b * Lout);
  const int p = n + n_fft / 2;
  int t0 = p - n_fft + 1 > 0 ? (p - n_fft + 1 + hop - 1) / hop : 0;
  int t1 = min(p / hop, T - 1);
  float acc = 0.f, env = 0.f;
  for (int t = t0; t <= t1; ++t) {
    const int j = p - t * hop;
    const float w = win[j];
    acc += fr[((int64_t)b * T + t) * n_fft + j];
    env += w * w;
  }
  y[i] = acc / env;
}
hipError_t vocos_ola(const float* frames, const float* win, int B, int T, int n_fft, int hop, float* y,
                     hipStream_t st) {
  if (T < 1 || n_fft % hop) return hipErrorInvalidValue;
  const int64_t n = (int64_t)B * (T - 1) * hop;
  if (n == 0) return hipSuccess;
  hipLaunchKernelGGL(vocos_ola_kernel, dim3(vblk(n, 256)), dim3(256), 0, st, frames, win, B, T, n_fft, hop, y);
  return hipGetLastError();
}

// ---- Ragged batch (kernels.h): utterance s owns packed rows [off[s], off[s+1]). Padding a batch to equal
// length is not equivalent: the embed conv and the k7 depthwise convs reach 27 frames across a boundary and
// LayerNorm of a zero row is not zero, so the kernels below stop every tap at the utterance's own ends.

// vocos_im2col gathering in place from a strided source (the sampler's [B][N][C] output or vocos' [B][C][T]):
// out[off[s] + t][c*7 + j] = src[s*row_st + (start[s] + t + j - 3)*frame_st + c*chan_st], zero when t + j - 3
// is outside [0, len_s): the utterance's own zero padding, never a neighbouring frame of the source.
template <typename TO>
__global__ void vocos_im2col_ragged_kernel(const float* src, int64_t row_st, int64_t frame_st, int64_t chan_st,
                                           const int* off, const int* start, int B, int R, int C, int Kp, TO* out) {
  const int64_t i = (int64_t)blockIdx.x * blockDim.x + threadIdx.x;
  if (i >= (int64_t)R * Kp) return;
  const int col = (int)(i % Kp), row = (int)(i / Kp);
  float v = 0.f;
  if (col < C * 7) {
    const int s = seg_find(off, B, row), base = off[s];
    const int c = col / 7, j = col - c * 7, q = row - base + j - 3;
    if (q >= 0 && q < off[s + 1] - base) v = src[s * row_st + (int64_t)(start[s] + q) * frame_st + c * chan_st];
  }
  out[i] = from_f32<TO>(v);
}
hipError_t vocos_im2col_ragged(int compute, const float* src, int64_t row_st, int64_t frame_st, int64_t chan_st,
                               const int32_t* off, const int32_t* start, int B, int R, int C, int Kp, void* out,
                               hipStream_t st) {
  if (Kp < C * 7 || Kp % 64 || B <= 0 || R <= 0) return hipErrorInvalidValue;
  const int64_t n = (int64_t)R * Kp;
  if (compute)
    hipLaunchKernelGGL(vocos_im2col_ragged_kernel<bf16>, dim3(vblk(n, 256)), dim3(256), 0, st, src, row_st, frame_st,
                       chan_st, off, start, B, R, C, Kp, (bf16*)out);
  else
    hipLaunchKernelGGL(vocos_im2col_ragged_kernel<float>, dim3(vblk(n, 256)), dim3(256), 0, st, src, row_st, frame_st,
                       chan_st, off, start, B, R, C, Kp, (float*)out);
  return hipGetLastError();
}

// vocos_ola per utterance: a thread per (packed row, offset in the hop). Row off[s] + t, t < len_s - 1, gives
// samples [t*hop, (t+1)*hop) of utterance s, summed over that utterance's frames only, in vocos_ola_kernel's
// order; the last row of every utterance gives none, so a one-frame utterance contributes nothing. Utterance s
// starts at sum_{j<s} (len_j - 1)*hop = (off[s] - s)*hop of y.
__global__ void vocos_ola_ragged_kernel(const float* fr, const float* win, const int* off, int B, int R, int n_fft,
                                        int hop, float* y) {
  const int64_t i = (int64_t)blockIdx.x * blockDim.x + threadIdx.x;
  if (i >= (int64_t)R * hop) return;
  const int row = (int)(i / hop), h = (int)(i - (int64_t)row * hop);
  const int s = seg_find(off, B, row), base = off[s], T = off[s + 1] - base;
  if (row - base >= T - 1) return;
  const int n = (row - base) * hop + h;
  const int p = n + n_fft / 2;
  int t0 = p - n_fft + 1 > 0 ? (p - n_fft + 1 + hop - 1) / hop : 0;
  int t1 = min(p / hop, T - 1);
  float acc = 0.f, env = 0.f;
  for (int t = t0; t <= t1; ++t) {
    const int j = p - t * hop;
    const float w = win[j];
    acc += fr[((int64_t)base + t) * n_fft + j];
    env += w * w;
  }
  y[(int64_t)(row - s) * hop + h] = acc / env;
}
hipError_t vocos_ola_ragged(const float* frames, const float* win, const int32_t* off, int B, int R, int n_fft,
                            int hop, float* y, hipStream_t st) {
  if (B <= 0 || R < B || n_fft % hop) return hipErrorInvalidValue;
  if (R == B) return hipSuccess;  // every utterance is one frame: no samples
  const int64_t n = (int64_t)R * hop;
  hipLaunchKernelGGL(vocos_ola_ragged_kernel, dim3(vblk(n, 256)), dim3(256), 0, st, frames, win, off, B, R, n_fft,
                     hop, y);
  return hipGetLastError();
}

}  // namespace f5h
