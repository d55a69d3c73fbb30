// ALiBi instantiations of the two-waves-per-SIMD backward kernels (C ABI: usp_flash_bwd_alibi, include/usp_hip.h).
// The bodies are the ones usp_flash_bwd.hip compiles (usp_flash_bwd_dq_body.inc, usp_flash_bwd_dkdv_body.inc) with AL = true: the
// bias -slope * log2(e) * |row + al_diag - key| goes into the exponent of P = exp2(S c + bias - lse2) -- in the dQ kernel and in
// role A of the dK/dV kernel, where one work item streams `gsub` query heads and reads the slope again for each.  dS, dQ, dK, dV
// are formed as without it: the bias is additive and has no gradient path to q, k or v; the slopes get no gradient.
// A translation unit of its own: the build parallelises and the objects of the other kernels do not change.
#include "usp_bwd_params.hpp"
#include "usp_host.hpp"

namespace usp {

template <int D, int DT, bool CAUSAL>
__global__ __launch_bounds__(512, 2) void flash_bwd_alibi_kernel(const BwdArgsAL p_in) {
#include "usp_flash_bwd_dq_body.inc"
}

template <int D, int DT, bool CAUSAL>
__global__ __launch_bounds__(512, 2) void flash_bwd_dkdv_alibi_kernel(const BwdArgsAL p_in) {
#include "usp_flash_bwd_dkdv_body.inc"
}

int launch_dkdv_alibi(const BwdArgsAL& p, int D, int dtype, bool causal, int grid, size_t lds, hipStream_t st) {
  return with_head_dim_dtype(D, dtype, [&](auto d, auto dt) -> int {
    with_causal(causal, [&](auto c) {
      hipLaunchKernelGGL((flash_bwd_dkdv_alibi_kernel<decltype(d)::value, decltype(dt)::value, decltype(c)::value>), dim3(grid),
                         dim3(512), lds, st, p);
    });
    return launched();
  });
}

int launch_dq_alibi(const BwdArgsAL& p, int D, int dtype, bool causal, int grid, size_t lds, hipStream_t st) {
  return with_head_dim_dtype(D, dtype, [&](auto d, auto dt) -> int {
    with_causal(causal, [&](auto c) {
      hipLaunchKernelGGL((flash_bwd_alibi_kernel<decltype(d)::value, decltype(dt)::value, decltype(c)::value>), dim3(grid),
                         dim3(512), lds, st, p);
    });
    return launched();
  });
}

}  // namespace usp
