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

#define USP_BWD_SPAN_ONLY                           \
  constexpr bool SC = false, AL = false, DR = false, DOC = true, SPAN = true, CAUSAL = false; \
  constexpr float sc_cl2 = 0.f, sc_k2 = 0.f;        \
  constexpr const float* al_slopes = nullptr;       \
  constexpr int64_t al_sb = 0;                      \
  constexpr int al_diag = 0;                        \
  constexpr Dropout dr{};                           \
  [[maybe_unused]] const int* const doc_row_lo = p_in.row_lo;   \
  [[maybe_unused]] const int* const doc_key_hi = p_in.key_hi;   \
  [[maybe_unused]] const int64_t doc_rl_sb = p_in.row_lo_sb, doc_kh_sb = p_in.key_hi_sb;   \
  [[maybe_unused]] const int* const span_row_hi = p_in.row_hi;  \
  [[maybe_unused]] const int* const span_key_lo = p_in.key_lo;  \
  [[maybe_unused]] const int64_t span_rh_sb = p_in.row_hi_sb, span_kl_sb = p_in.key_lo_sb; \
  USP_BWD_NO_BSP

template <int D, int DT>
__global__ __launch_bounds__(512, 2) void flash_bwd_span_kernel(const BwdArgsSPAN p_in) {
  USP_BWD_SPAN_ONLY
#include "usp_flash_bwd_dq_body.inc"
}

template <int D, int DT>
__global__ __launch_bounds__(512, 2) void flash_bwd_dkdv_span_kernel(const BwdArgsSPAN p_in) {
  USP_BWD_SPAN_ONLY
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
