// QKV GEMM launchers over packed rows of unequal sequences (gemm_impl.h RQ; see launch_t and kernels.h qkv_rowtab)
#include "gemm_impl.h"

namespace f5h {
hipError_t gemm_launch_rq_bf16(const GemmArgs& a, hipStream_t st) { return launch_rq<bf16>(a, st); }
hipError_t gemm_launch_rq_f16(const GemmArgs& a, hipStream_t st) { return launch_rq<f16>(a, st); }
hipError_t gemm_launch_rq_f32(const GemmArgs& a, hipStream_t st) { return launch_rq<float>(a, st); }
}  // namespace f5h
