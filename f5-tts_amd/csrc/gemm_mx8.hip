// MXFP8 GEMM (compute mode F5H_MXFP8): C[M,N] = A8[M,K] . W8[N,K]^T with per-32-K E8M0 scales on
// v_mfma_scale_f32_16x16x128_f8f6f4 (e4m3 operands: twice the bf16 MFMA rate), fp32 accumulation, bf16 epilogues.
//
// One tile configuration: 128 x 128 block tile, 256 threads = 4 waves as 2 x 2, each wave a 64 x 64 sub-tile of
// 4 x 4 MFMA tiles. A K-step is 128 elements = 128 bytes per row = one MFMA: the stage image is the bf16 kernel's
// (gemm_impl.h: 128-byte rows of 8 chunks, XOR-swizzled through the DMA's source address, filled by 16-byte LDS-DMA),
// plus one dword of scales per row (the K-step's four blocks) filled by a 4-byte LDS-DMA. Two stages, two blocks
// per CU.
// Operand lane map of the scaled MFMA with 8-bit operands, established on the hardware with one-hot operands and
// distinct scales per lane (and held by tests/test_gpu_mx8_ops.py::test_gemm_exact_integers, exact integer data with
// asymmetric operands and scales): lane l = 16 q + r holds row (column) r; its registers 0-3 hold K bytes
// 16 q .. 16 q + 15 and its registers 4-7 K bytes 64 + 16 q .. 64 + 16 q + 15, i.e. the 16-byte chunks q and 4 + q of
// the 128-byte row (the bf16 kernel's two k-slabs); bytes ascend inside a register. The scale of the 32-K block b
// (K bytes 32 b .. 32 b + 31) of row r is taken from lane 16 b + r: lane l supplies the scale of block q of its own
// row, though that block's bytes sit in two other lanes' registers. op_sel is an immediate, so every lane shifts
// byte q of its row's scale dword into byte 0.
// The operands are passed swapped (W as the first operand), so a lane holds output row l & 15 and four consecutive
// columns: the accumulator is staged through the wave's LDS strip exactly as gemm_impl.h's general epilogue stages the
// bf16 form of the same M x N, and epi8 runs unchanged.
// K order: ascending K-steps into one accumulator, whatever M: a row's bits depend on its own A row only.
#include "gemm_impl.h"

namespace f5h {

typedef int i32x8 __attribute__((ext_vector_type(8)));

namespace mx {
constexpr int BM = 128, BN = 128, NS = 2, THREADS = 256, NW = 4;
constexpr int WM = 64, WN = 64, MT = 4, NT = 4;
constexpr int KB = 128;                           // K elements = bytes per row per stage
constexpr int stage_bytes = (BM + BN) * KB;       // A rows, then W rows
constexpr int scale_bytes = (BM + BN) * 4;        // one dword per row
constexpr int scale_base = NS * stage_bytes;
constexpr int main_bytes = NS * (stage_bytes + scale_bytes);
constexpr int EPAD = WN + 4;
constexpr int epi_bytes = NW * 16 * EPAD * 4;
constexpr int bytes = main_bytes > epi_bytes ? main_bytes : epi_bytes;
constexpr int RPR = THREADS / 8;                  // rows per DMA round
constexpr int AR = BM / RPR, BR = BN / RPR;       // DMA rounds per stage
static_assert(RPR % 16 == 0, "the swizzled chunk of a lane is the same in every DMA round");
static_assert(BM + BN == NW * 64, "one scale dword per lane: one 4-byte DMA per wave covers the stage's rows");
}  // namespace mx

template <int OFF>
F5H_DEV uint32_t lds_read_b32(uint32_t addr) {
  uint32_t r;
  asm volatile("ds_read_b32 %0, %1 offset:%2" : "=v"(r) : "v"(addr), "i"(OFF));
  return r;
}
F5H_DEV void dma4(__amdgpu_buffer_rsrc_t r, LDS_PTR(void) dst, uint32_t voff, uint32_t soff) {
  __builtin_amdgcn_raw_ptr_buffer_load_lds(r, dst, 4, voff, soff, 0, 0);
}

template <int EPI, bool QKN, bool RQ>
__global__ __launch_bounds__(mx::THREADS, 2) void gemm_mx8_kernel(GemmArgs g, Mx8Ops o) {
  using namespace mx;
  __shared__ __attribute__((aligned(16))) uint4 lds[bytes / 16];
  const ProbeT probe_t = probe_enter(g.probe);
  const int tid = threadIdx.x, lane = tid & 63, wid = tid >> 6;
  const int wid_s = __builtin_amdgcn_readfirstlane(wid);
  const int wm = wid >> 1, wn = wid & 1;
  const int ntn = (g.N + BN - 1) / BN;
  const int mrow = (int)blockIdx.x / ntn;
  const int m0 = mrow * BM, n0 = ((int)blockIdx.x - mrow * ntn) * BN;
  const int K = g.K, KS = K >> 5;  // scale bytes per row
  if (o.count && blockIdx.x == 0 && tid == 0) atomicAdd(o.count, 1ull);

  // Rows past M (N) are outside the block's buffers and read as zero (elements and scales): they feed unstored
  // outputs only.
  const int arows = min(BM, g.M - m0), wrows = min(BN, g.N - n0);
  const __amdgpu_buffer_rsrc_t ars = rsrc_of(o.a8 + (int64_t)m0 * K, (uint64_t)arows * K);
  const __amdgpu_buffer_rsrc_t wrs = rsrc_of(o.w8 + (int64_t)n0 * K, (uint64_t)wrows * K);
  // scales: waves 0, 1 bring the A rows' dwords (rows 64 wid + lane), waves 2, 3 the W rows'
  const bool sw = wid_s >= 2;
  const uint8_t* const sp = sw ? o.ws + (int64_t)n0 * KS : o.as + (int64_t)m0 * KS;
  const __amdgpu_buffer_rsrc_t srs = rsrc_of(sp, (uint64_t)(sw ? wrows : arows) * KS);
  const uint32_t soff_lane = (uint32_t)(((wid_s & 1) * 64 + lane) * KS);

  const int row0 = tid >> 3, chunk0 = swz128g(row0, tid & 7) * 16;
  uint32_t aoff[AR], boff[BR];
  static_for<0, AR>([&](auto I) {
    constexpr int i = decltype(I)::value;
    aoff[i] = (uint32_t)((row0 + i * RPR) * K + chunk0);
  });
  static_for<0, BR>([&](auto I) {
    constexpr int i = decltype(I)::value;
    boff[i] = (uint32_t)((row0 + i * RPR) * K + chunk0);
  });
  auto stage = [&](int buf, int kt) {
    uint4* As = lds + buf * (stage_bytes / 16);
    uint4* Bs = As + BM * 8;
    static_for<0, AR>([&](auto I) {
      constexpr int i = decltype(I)::value;
      dma16(ars, (LDS_PTR(void))(As + (i * NW + wid_s) * 64), aoff[i], (uint32_t)(kt * KB));
    });
    static_for<0, BR>([&](auto I) {
      constexpr int i = decltype(I)::value;
      dma16(wrs, (LDS_PTR(void))(Bs + (i * NW + wid_s) * 64), boff[i], (uint32_t)(kt * KB));
    });
    dma4(srs, (LDS_PTR(void))(lds + (scale_base + buf * scale_bytes) / 16 + wid_s * 16), soff_lane, (uint32_t)(kt * 4));
  };

  const int nk = K / KB;
  stage(0, 0);

  // fragment addresses: lane l reads row l & 15 of a 16-row tile at the logical chunks q and 4 + q (q = l >> 4),
  // and its row's scale dword
  const uint32_t lds0 = (uint32_t)(uintptr_t)(LDS_PTR(void))lds;
  const int fr = lane & 15, q = lane >> 4;
  uint32_t abase[2], bbase[2];
#pragma unroll
  for (int c = 0; c < 2; ++c) {
    abase[c] = lds0 + (wm * WM + fr) * KB + swz128g(fr, 4 * c + q) * 16;
    bbase[c] = lds0 + BM * KB + (wn * WN + fr) * KB + swz128g(fr, 4 * c + q) * 16;
  }
  const uint32_t sabase = lds0 + scale_base + (wm * WM + fr) * 4;
  const uint32_t sbbase = lds0 + scale_base + (BM + wn * WN + fr) * 4;

  f32x4 acc[MT][NT];
#pragma unroll
  for (int i = 0; i < MT; ++i)
#pragma unroll
    for (int j = 0; j < NT; ++j) acc[i][j] = f32x4{0.f, 0.f, 0.f, 0.f};

  for (int kt = 0; kt < nk; ++kt) {
    // stage kt is this wave's only DMA in flight: wait for it, then the barrier publishes every wave's part
    asm volatile("s_waitcnt vmcnt(0)" ::: "memory");
    __builtin_amdgcn_s_barrier();
    const uint32_t eoff = (uint32_t)((kt & 1) * stage_bytes), soff = (uint32_t)((kt & 1) * scale_bytes);
    u32x4 ar[MT][2], br[NT][2];
    uint32_t sa[MT], sb[NT];
    static_for<0, MT>([&](auto I) {
      constexpr int i = decltype(I)::value;
      ar[i][0] = lds_read_b128<i * 16 * KB>(abase[0] + eoff);
      ar[i][1] = lds_read_b128<i * 16 * KB>(abase[1] + eoff);
      sa[i] = lds_read_b32<i * 64>(sabase + soff);
    });
    static_for<0, NT>([&](auto J) {
      constexpr int j = decltype(J)::value;
      br[j][0] = lds_read_b128<j * 16 * KB>(bbase[0] + eoff);
      br[j][1] = lds_read_b128<j * 16 * KB>(bbase[1] + eoff);
      sb[j] = lds_read_b32<j * 64>(sbbase + soff);
    });
    // WAR: the other slot was last read in iteration kt - 1, whose reads all completed before that iteration's
    // MFMAs, i.e. before every wave reached this barrier
    if (kt + 1 < nk) stage((kt + 1) & 1, kt + 1);
    asm volatile("s_waitcnt lgkmcnt(0)" ::: "memory");
#pragma unroll
    for (int i = 0; i < MT; ++i) asm volatile("" : "+v"(ar[i][0]), "+v"(ar[i][1]), "+v"(sa[i]));
#pragma unroll
    for (int j = 0; j < NT; ++j) asm volatile("" : "+v"(br[j][0]), "+v"(br[j][1]), "+v"(sb[j]));
    __builtin_amdgcn_sched_barrier(0);
    i32x8 av[MT], bv[NT];
#pragma unroll
    for (int i = 0; i < MT; ++i) {
      av[i] = i32x8{(int)ar[i][0].x, (int)ar[i][0].y, (int)ar[i][0].z, (int)ar[i][0].w,
                    (int)ar[i][1].x, (int)ar[i][1].y, (int)ar[i][1].z, (int)ar[i][1].w};
      sa[i] >>= 8 * q;
    }
#pragma unroll
    for (int j = 0; j < NT; ++j) {
      bv[j] = i32x8{(int)br[j][0].x, (int)br[j][0].y, (int)br[j][0].z, (int)br[j][0].w,
                    (int)br[j][1].x, (int)br[j][1].y, (int)br[j][1].z, (int)br[j][1].w};
      sb[j] >>= 8 * q;
    }
#pragma unroll
    for (int i = 0; i < MT; ++i)
#pragma unroll
      for (int j = 0; j < NT; ++j)
        acc[i][j] = __builtin_amdgcn_mfma_scale_f32_16x16x128_f8f6f4(bv[j], av[i], acc[i][j], 0, 0, 0, (int)sb[j], 0,
                                                                     (int)sa[i]);
  }
  __syncthreads();  // every wave is done with the stages: the epilogue strips reuse their LDS

  // ---- epilogue: gemm_impl.h's general form, per wave and 16-row strip
  float* Cs = reinterpret_cast<float*>(lds) + wid * 16 * EPAD;
  constexpr int CH = WN / 8, TPC = 16 * CH / 64;
#pragma unroll
  for (int i = 0; i < MT; ++i) {
#pragma unroll
    for (int j = 0; j < NT; ++j) *reinterpret_cast<f32x4*>(Cs + fr * EPAD + j * 16 + 4 * q) = acc[i][j];
    __builtin_amdgcn_fence(__ATOMIC_RELEASE, "wavefront");
    __builtin_amdgcn_wave_barrier();
    __builtin_amdgcn_fence(__ATOMIC_ACQUIRE, "wavefront");
#pragma unroll
    for (int t = 0; t < TPC; ++t) {
      const int idx = t * 64 + lane, rr = idx / CH, cc = idx % CH;
      const int row = m0 + wm * WM + i * 16 + rr, col = n0 + wn * WN + cc * 8;
      const float* src = Cs + rr * EPAD + cc * 8;
      const float4 a = *reinterpret_cast<const float4*>(src), b = *reinterpret_cast<const float4*>(src + 4);
      if (row < g.M && col < g.N)
        epi8<bf16, EPI, QKN, RQ>(g, row, col, V8{{a.x, a.y, a.z, a.w, b.x, b.y, b.z, b.w}}, nullptr);
    }
    __builtin_amdgcn_fence(__ATOMIC_RELEASE, "wavefront");
    __builtin_amdgcn_wave_barrier();
    __builtin_amdgcn_fence(__ATOMIC_ACQUIRE, "wavefront");
  }
  probe_exit(g.probe, probe_t);
}

template <int EPI, bool QKN, bool RQ>
static hipError_t launch_mx8(const GemmArgs& a, const Mx8Ops& o, hipStream_t st) {
  const int64_t nwg = (int64_t)((a.M + mx::BM - 1) / mx::BM) * ((a.N + mx::BN - 1) / mx::BN);
  if (nwg <= 0 || nwg > (1 << 20)) return hipErrorInvalidValue;
  hipLaunchKernelGGL((gemm_mx8_kernel<EPI, QKN, RQ>), dim3((unsigned)nwg), dim3(mx::THREADS), 0, st, a, o);
  return hipGetLastError();
}

hipError_t gemm_mx8(int epi, const GemmArgs& a, const Mx8Ops& o, hipStream_t st) {
  if (!o.a8 || !o.as || !o.w8 || !o.ws || a.M <= 0 || a.N <= 0 || a.K <= 0 || a.K % 128) return hipErrorInvalidValue;
  if (((uintptr_t)o.a8 & 15) || ((uintptr_t)o.w8 & 15) || ((uintptr_t)o.as & 3) || ((uintptr_t)o.ws & 3))
    return hipErrorInvalidValue;
  // the buffer descriptors' extents and the lanes' offsets are 32-bit
  if ((int64_t)mx::BM * a.K >= (1ll << 31)) return hipErrorInvalidValue;
  if (a.A2 || a.ln_part_in || a.hs || a.ln_part || a.live_len) return hipErrorInvalidValue;  // no fold, no pad-row skip
  switch (epi) {
    case EPI_QKV: {
      if (!a.q || !a.k || !a.v || a.heads <= 0 || a.N != 3 * a.heads * 64) return hipErrorInvalidValue;
      const bool qkn = a.q_norm_w != nullptr, rq = a.add != nullptr;
      if (qkn != (a.k_norm_w != nullptr)) return hipErrorInvalidValue;
      if (!rq && a.seq_len <= 0) return hipErrorInvalidValue;
      if (rq && a.qkv_dst_len <= 0) return hipErrorInvalidValue;
      if (qkn) return rq ? launch_mx8<EPI_QKV, true, true>(a, o, st) : launch_mx8<EPI_QKV, true, false>(a, o, st);
      return rq ? launch_mx8<EPI_QKV, false, true>(a, o, st) : launch_mx8<EPI_QKV, false, false>(a, o, st);
    }
    case EPI_RESID16:
      if (!a.C) return hipErrorInvalidValue;
      return launch_mx8<EPI_RESID16, false, false>(a, o, st);
    case EPI_GELU_TANH:
      if (!a.C) return hipErrorInvalidValue;
      return launch_mx8<EPI_GELU_TANH, false, false>(a, o, st);
    default: return hipErrorInvalidValue;
  }
}

}  // namespace f5h
