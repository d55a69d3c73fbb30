// Span instantiations of the two-waves-per-SIMD backward kernels (C ABI: usp_flash_bwd_span, include/usp_hip.h).
// The bodies are the ones usp_flash_bwd.hip compiles (usp_flash_bwd_dq_body.inc, usp_flash_bwd_dkdv_body.inc) with DOC = true and
// SPAN = true: row i sees key j only if row_lo[i] <= j < row_hi[i].  The dQ kernel owns rows and reads (row_lo, row_hi); the dK/dV
// kernel owns keys and reads the transpose (key_lo, key_hi): only if key_lo[j] <= i < key_hi[j].  All four arrays are monotone
// (usp_tile_range.h), so an item's streamed range and a wave's live and masked tiles are two reads per bound.  The planner folds
// the causal diagonal into the arrays: these kernels are never causal.  Only role A of the dK/dV kernel masks.
// 3 head dims x 2 types x 2 launches = 12 kernels.
// A translation unit of its own: the build parallelises and the objects of the other kernels do not change.
#include "usp_bwd_params.hpp"
#include "usp_host.hpp"

namespace usp {

template <int D, int DT>
__global__ __launch_bounds__(512, 2) void flash_bwd_span_kernel(const BwdArgsSPAN p_in) {
  constexpr bool CAUSAL = false;
#include "usp_flash_bwd_dq_body.inc"
}

template <int D, int DT>
__global__ __launch_bounds__(512, 2) void flash_bwd_dkdv_span_kernel(const BwdArgsSPAN p_in) {
  constexpr bool CAUSAL = false;
#include "usp_flash_bwd_dkdv_body.inc"
}

int launch_dkdv_span(const BwdArgsSPAN& p, int D, int dtype, int grid, size_t lds, hipStream_t st) {
  return with_head_dim_dtype(D, dtype, [&](auto d, auto dt) -> int {
    hipLaunchKernelGGL((flash_bwd_dkdv_span_kernel<decltype(d)::value, decltype(dt)::value>), dim3(grid), dim3(512), lds, st, p);
    return launched();
  });
}

int launch_dq_span(const BwdArgsSPAN& p, int D, int dtype, int grid, size_t lds, hipStream_t st) {
  return with_head_dim_dtype(D, dtype, [&](auto d, auto dt) -> int {
    hipLaunchKernelGGL((flash_bwd_span_kernel<decltype(d)::value, decltype(dt)::value>), dim3(grid), dim3(512), lds, st, p);
    return launched();
  });
}

}  // namespace usp
