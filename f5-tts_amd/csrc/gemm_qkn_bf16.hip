// bf16 QKV GEMM launchers with qk_norm in the epilogue (gemm_impl.h QKN; see launch_t)
#include "gemm_impl.h"

namespace f5h {
hipError_t gemm_launch_qkn_bf16(const GemmArgs& a, int cfg, hipStream_t st) { return launch_qkn<bf16>(a, cfg, st); }
}  // namespace f5h
