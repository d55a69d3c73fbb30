// Block-sparse instantiations of the two-waves-per-SIMD backward kernels (C ABI: usp_flash_bwd_bsp, include/usp_hip.h).
// The bodies are the ones usp_flash_bwd.hip compiles (usp_flash_bwd_dq_body.inc, usp_flash_bwd_dkdv_body.inc) with BSP = true: the
// streamed tiles of a work item are a list built by usp_block_lists.hip from the 128 x 128 block mask, not a range.
//   dQ:     the 256-row block holds two mask row blocks and streams the union of their lists of 64-key tiles; an entry carries
//           one "live" bit per half, and the four waves of a half skip the compute of an entry that is dead for them.
//   dK/dV:  the 128-key block is one mask column and streams, for each query head of its loop, the 64-row tiles of that head's
//           transposed list; only the staging cursor reads the lists.
// The diagonal blocks are masked by the bodies' causal steps, unchanged.  Entries are read with ordinary loads and clamped as read.
// 3 head dims x 2 types x causal / full x 2 launches = 24 kernels.
// A translation unit of its own: the build parallelises and the objects of the other kernels do not change.
#include "usp_bwd_params.hpp"
#include "usp_host.hpp"

namespace usp {

#define USP_BWD_BSP_ONLY                            \
  constexpr bool SC = false, AL = false, DR = false, DOC = false, BSP = true; \
  constexpr float sc_cl2 = 0.f, sc_k2 = 0.f;        \
  constexpr const float* al_slopes = nullptr;       \
  constexpr int64_t al_sb = 0;                      \
  constexpr int al_diag = 0;                        \
  constexpr Dropout dr{};                           \
  [[maybe_unused]] constexpr const int* doc_row_lo = nullptr;   \
  [[maybe_unused]] constexpr const int* doc_key_hi = nullptr;   \
  [[maybe_unused]] constexpr int64_t doc_rl_sb = 0, doc_kh_sb = 0;   \
  [[maybe_unused]] constexpr bool SPAN = false;                  \
  [[maybe_unused]] constexpr const int* span_row_hi = nullptr;   \
  [[maybe_unused]] constexpr const int* span_key_lo = nullptr;   \
  [[maybe_unused]] constexpr int64_t span_rh_sb = 0, span_kl_sb = 0; \
  const int* const bsp_lists = p_in.bsp_lists;      \
  const int bsp_stride = p_in.bsp_stride;

template <int D, int DT, bool CAUSAL>
__global__ __launch_bounds__(512, 2) void flash_bwd_bsp_kernel(const BwdArgsBSP p_in) {
  USP_BWD_BSP_ONLY
#include "usp_flash_bwd_dq_body.inc"
}

template <int D, int DT, bool CAUSAL>
__global__ __launch_bounds__(512, 2) void flash_bwd_dkdv_bsp_kernel(const BwdArgsBSP p_in) {
  USP_BWD_BSP_ONLY
#include "usp_flash_bwd_dkdv_body.inc"
}

int launch_dkdv_bsp(const BwdArgsBSP& p, int D, int dtype, bool causal, int grid, size_t lds, hipStream_t st) {
  return with_head_dim_dtype(D, dtype, [&](auto d, auto dt) -> int {
    with_causal(causal, [&](auto c) {
      hipLaunchKernelGGL((flash_bwd_dkdv_bsp_kernel<decltype(d)::value, decltype(dt)::value, decltype(c)::value>), dim3(grid), dim3(512),
                         lds, st, p);
    });
    return launched();
  });
}

int launch_dq_bsp(const BwdArgsBSP& p, int D, int dtype, bool causal, int grid, size_t lds, hipStream_t st) {
  return with_head_dim_dtype(D, dtype, [&](auto d, auto dt) -> int {
    with_causal(causal, [&](auto c) {
      hipLaunchKernelGGL((flash_bwd_bsp_kernel<decltype(d)::value, decltype(dt)::value, decltype(c)::value>), dim3(grid), dim3(512), lds,
                         st, p);
    });
    return launched();
  });
}

}  // namespace usp
