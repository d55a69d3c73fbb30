// Dropout instantiations of the two-waves-per-SIMD backward kernels (C ABI: usp_flash_bwd_dropout, include/usp_hip.h).
// The bodies are the ones usp_flash_bwd.hip compiles (usp_flash_bwd_dq_body.inc, usp_flash_bwd_dkdv_body.inc) with DR = true.
// Both regenerate the forward's mask from global (batch, query head, row, key) (usp_dropout_rng.h); P = exp2(S c - lse2) is the
// un-dropped probability, delta = rowsum(dout * out) is that of the dropped `out`, and with rs = 256 / t
//     dV = rs (P o keep)^T dO,    dS = P (rs keep dP - delta),    dQ = scale dS K,    dK = scale dS^T Q.
// dQ forms dS per element.  In dK/dV role A uses P o keep for dV and hands role B the un-dropped P with the keep decision in the
// sign bit; role B starts its dP chain from -delta / rs, forms |P| (kept ? chain : -delta / rs), and rs goes into the epilogue's
// factor of both outputs.  One work item streams `gsub` query heads, so the head of the mask's counter follows the streamed head.
// A translation unit of its own: the build parallelises and the objects of the other kernels do not change.
#include "usp_bwd_params.hpp"
#include "usp_host.hpp"

namespace usp {

template <int D, int DT, bool CAUSAL>
__global__ __launch_bounds__(512, 2) void flash_bwd_dropout_kernel(const BwdArgsDR p_in) {
#include "usp_flash_bwd_dq_body.inc"
}

template <int D, int DT, bool CAUSAL>
__global__ __launch_bounds__(512, 2) void flash_bwd_dkdv_dropout_kernel(const BwdArgsDR p_in) {
#include "usp_flash_bwd_dkdv_body.inc"
}

int launch_dkdv_dropout(const BwdArgsDR& p, int D, int dtype, bool causal, int grid, size_t lds, hipStream_t st) {
  return with_head_dim_dtype(D, dtype, [&](auto d, auto dt) -> int {
    with_causal(causal, [&](auto c) {
      hipLaunchKernelGGL((flash_bwd_dkdv_dropout_kernel<decltype(d)::value, decltype(dt)::value, decltype(c)::value>), dim3(grid),
                         dim3(512), lds, st, p);
    });
    return launched();
  });
}

int launch_dq_dropout(const BwdArgsDR& p, int D, int dtype, bool causal, int grid, size_t lds, hipStream_t st) {
  return with_head_dim_dtype(D, dtype, [&](auto d, auto dt) -> int {
    with_causal(causal, [&](auto c) {
      hipLaunchKernelGGL((flash_bwd_dropout_kernel<decltype(d)::value, decltype(dt)::value, decltype(c)::value>), dim3(grid),
                         dim3(512), lds, st, p);
    });
    return launched();
  });
}

}  // namespace usp
