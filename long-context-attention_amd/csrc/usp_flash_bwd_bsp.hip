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

template <int D, int DT, bool CAUSAL>
__global__ __launch_bounds__(512, 2) void flash_bwd_bsp_kernel(const BwdArgsBSP p_in) {
#include "usp_flash_bwd_dq_body.inc"
}

template <int D, int DT, bool CAUSAL>
__global__ __launch_bounds__(512, 2) void flash_bwd_dkdv_bsp_kernel(const BwdArgsBSP p_in) {
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
