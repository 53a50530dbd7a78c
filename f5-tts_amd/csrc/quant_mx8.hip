// MXFP8 quantisers (compute mode F5H_MXFP8; the rule and the layouts: kernels.h 'MXFP8 operands').
//   quant_rows_mx8   bf16 [M, K] -> e4m3fn elements + E8M0 scale bytes: the weights once at engine creation, the
//                    attention output ahead of the out-projection and the GELU output ahead of FFN2
//   ln_modulate_mx8  ln_modulate (lnrow.h: the same row functions, so the same bits) whose bf16 row goes to LDS and
//                    from there through the same block quantiser: feeds QKV and FFN1
#include "common.h"
#include "kernels.h"
#include "lnrow.h"

namespace f5h {

static inline unsigned nblk(int64_t n, int per) { return (unsigned)((n + per - 1) / per); }

// One 32-element block held as bf16 in four 16-byte chunks (any address space the caller loaded them from):
// integer amax, scale byte, 32 e4m3 bytes as two 16-byte stores.
F5H_DEV void mx8_quant_block(const uint4 (&raw)[4], uint8_t* q, uint8_t* s) {
  uint32_t bits[32];
#pragma unroll
  for (int c = 0; c < 4; ++c) {
    const uint32_t w[4] = {raw[c].x, raw[c].y, raw[c].z, raw[c].w};
#pragma unroll
    for (int e = 0; e < 4; ++e) {  // bf16 -> fp32 is a 16-bit shift
      bits[c * 8 + 2 * e] = w[e] << 16;
      bits[c * 8 + 2 * e + 1] = w[e] & 0xFFFF0000u;
    }
  }
  uint32_t amax = 0;
#pragma unroll
  for (int e = 0; e < 32; ++e) amax = max(amax, bits[e] & 0x7FFFFFFFu);
  const uint8_t sb = mx8_scale_byte(amax);
  const float mult = __uint_as_float(mx8_unscale_bits(sb));
  uint32_t out[8];
#pragma unroll
  for (int w = 0; w < 8; ++w) {
    uint32_t p = 0;
#pragma unroll
    for (int e = 0; e < 4; ++e) {
      const uint32_t b = bits[4 * w + e], a = b & 0x7FFFFFFFu;
      // a non-finite element stays non-finite (inf * mult = inf, NaN stays NaN): 0x7F from mx8_e4m3
      const uint32_t scaled = a >= 0x7F800000u ? b : __float_as_uint(mul_nc(__uint_as_float(b), mult));
      p |= (uint32_t)mx8_e4m3(scaled) << (8 * e);
    }
    out[w] = p;
  }
  uint4* qo = reinterpret_cast<uint4*>(q);
  qo[0] = uint4{out[0], out[1], out[2], out[3]};
  qo[1] = uint4{out[4], out[5], out[6], out[7]};
  *s = sb;
}

// one thread per 32-element block
__global__ __launch_bounds__(256) void quant_rows_mx8_kernel(const bf16* x, int64_t nblocks, uint8_t* q, uint8_t* s) {
  const int64_t i = (int64_t)blockIdx.x * 256 + threadIdx.x;
  if (i >= nblocks) return;
  const uint4* src = reinterpret_cast<const uint4*>(x + i * 32);
  const uint4 raw[4] = {src[0], src[1], src[2], src[3]};
  mx8_quant_block(raw, q + i * 32, s + i);
}

hipError_t quant_rows_mx8(const void* x, int64_t M, int K, uint8_t* q, uint8_t* s, hipStream_t st) {
  if (!x || !q || !s || M <= 0 || K <= 0 || K % 32 || ((uintptr_t)x & 15) || ((uintptr_t)q & 15))
    return hipErrorInvalidValue;
  const int64_t nb = M * (K / 32);  // rows are contiguous: the blocks of the whole panel in one index
  if (nblk(nb, 256) > 0x7FFFFFFFu) return hipErrorInvalidValue;
  hipLaunchKernelGGL(quant_rows_mx8_kernel, dim3(nblk(nb, 256)), dim3(256), 0, st, (const bf16*)x, nb, q, s);
  return hipGetLastError();
}

// A wave per row as ln_mod_kernel / ln_mod16_kernel (elementwise.hip), with the same loads and the same row
// functions; the bf16 row lands in the wave's LDS row instead of global memory, then lane b quantises block b.
constexpr int kMx8MaxD = 2048;  // ln_modulate's limit (8 float4 per lane)
template <int NV, typename TI, bool V16>
__global__ __launch_bounds__(256) void ln_mod_mx8_kernel(const TI* h, int M, int d, const float* shift,
                                                         const float* scale, uint8_t* q, uint8_t* s) {
  __shared__ __attribute__((aligned(16))) bf16 rows[4][kMx8MaxD];
  const int wv = threadIdx.x >> 6, row = blockIdx.x * 4 + wv, lane = threadIdx.x & 63;
  if (row >= M) return;  // whole waves leave: the rest of the kernel has wave-level synchronisation only
  const float4* sh = reinterpret_cast<const float4*>(shift);
  const float4* sc = reinterpret_cast<const float4*>(scale);
  bf16* orow = rows[wv];
  if constexpr (V16) {  // d == 1024, bf16 residual stream: ln_mod16_kernel's form
    const uint4* x = reinterpret_cast<const uint4*>(h + (int64_t)row * 1024);
    uint4 xv[2], o[2];
    float4 a[2][2], b[2][2];
#pragma unroll
    for (int k = 0; k < 2; ++k) {
      const int c = lane + 64 * k;
      xv[k] = x[c];
      a[k][0] = sc[2 * c];
      a[k][1] = sc[2 * c + 1];
      b[k][0] = sh[2 * c];
      b[k][1] = sh[2 * c + 1];
    }
    ln16_row<bf16>(xv, a, b, o);
    uint4* op = reinterpret_cast<uint4*>(orow);
#pragma unroll
    for (int k = 0; k < 2; ++k) op[lane + 64 * k] = o[k];
  } else {
    constexpr bool FIXED = NV > 0;
    constexpr int V = FIXED ? NV : 8;
    const TI* x = h + (int64_t)row * d;
    const int n4 = FIXED ? 64 * NV : d >> 2;
    float4 v[V], a[V], b[V];
#pragma unroll
    for (int k = 0; k < V; ++k) {
      const int i = lane + 64 * k;
      const bool ok = FIXED || i < n4;
      v[k] = ok ? load4f<TI>(x + 4 * i) : make_float4(0, 0, 0, 0);
      a[k] = ok ? sc[i] : make_float4(0, 0, 0, 0);
      b[k] = ok ? sh[i] : make_float4(0, 0, 0, 0);
    }
    ln_mod_row<bf16, V, FIXED>(v, a, b, lane, n4, d, orow);
  }
  __builtin_amdgcn_fence(__ATOMIC_RELEASE, "wavefront");
  __builtin_amdgcn_wave_barrier();
  __builtin_amdgcn_fence(__ATOMIC_ACQUIRE, "wavefront");
  const int nb = d >> 5;  // <= 64
  if (lane < nb) {
    const uint4* src = reinterpret_cast<const uint4*>(orow + lane * 32);
    const uint4 raw[4] = {src[0], src[1], src[2], src[3]};
    mx8_quant_block(raw, q + (int64_t)row * d + lane * 32, s + (int64_t)row * nb + lane);
  }
}

hipError_t ln_modulate_mx8(const void* hv, int h16, int M, int d, const float* shift, const float* scale, uint8_t* q,
                           uint8_t* s, hipStream_t st) {
  if (!hv || !q || !s || !shift || !scale || M <= 0 || d <= 0 || d % 32 || d > kMx8MaxD || ((uintptr_t)q & 15))
    return hipErrorInvalidValue;
  const dim3 g(nblk(M, 4)), b(256);
  // the kernel per width mirrors ln_modulate's choice (elementwise.hip), so each width runs the row function it runs there
  if (h16) {
    const bf16* x = (const bf16*)hv;
    switch (d) {
      case 1024: hipLaunchKernelGGL((ln_mod_mx8_kernel<0, bf16, true>), g, b, 0, st, x, M, d, shift, scale, q, s); break;
      case 768: hipLaunchKernelGGL((ln_mod_mx8_kernel<3, bf16, false>), g, b, 0, st, x, M, d, shift, scale, q, s); break;
      case 512: hipLaunchKernelGGL((ln_mod_mx8_kernel<2, bf16, false>), g, b, 0, st, x, M, d, shift, scale, q, s); break;
      default: hipLaunchKernelGGL((ln_mod_mx8_kernel<0, bf16, false>), g, b, 0, st, x, M, d, shift, scale, q, s);
    }
  } else {
    const float* x = (const float*)hv;
    switch (d) {
      case 1024: hipLaunchKernelGGL((ln_mod_mx8_kernel<4, float, false>), g, b, 0, st, x, M, d, shift, scale, q, s); break;
      case 768: hipLaunchKernelGGL((ln_mod_mx8_kernel<3, float, false>), g, b, 0, st, x, M, d, shift, scale, q, s); break;
      case 512: hipLaunchKernelGGL((ln_mod_mx8_kernel<2, float, false>), g, b, 0, st, x, M, d, shift, scale, q, s); break;
      default: hipLaunchKernelGGL((ln_mod_mx8_kernel<0, float, false>), g, b, 0, st, x, M, d, shift, scale, q, s);
    }
  }
  return hipGetLastError();
}

}  // namespace f5h
