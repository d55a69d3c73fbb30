// Block-sparse instantiations of the two-waves-per-SIMD forward (C ABI: usp_flash_fwd_bsp, include/usp_hip.h).
// The body is the one usp_flash_fwd.hip compiles (usp_flash_fwd_body.inc), on the plain (unsplit) argument block, with BSP = true:
// a work item -- always 4 waves, 128 query rows, ONE row block of the 128 x 128 block mask -- walks the ascending list of 64-key
// tiles that usp_block_lists.hip built for it instead of the tiles [0, nt).  Buffers and barriers of the body are per walk index,
// the online softmax does not care about gaps: the listed tiles below a wave's diagonal / ragged limit are a prefix of the list
// and keep the pipelined main loop, the diagonal and ragged ones come last and take the masked tail, as in the plain kernel.
// List entries are read with ordinary (scalar) loads, one iteration ahead in the pipelined loop, and clamped as read.
// 3 head dims x 2 types x causal / full = 12 kernels.
// A translation unit of its own: the build parallelises and the objects of the other kernels do not change.
#include "usp_fwd_params.hpp"
#include "usp_host.hpp"

namespace usp {

// (PA: the argument block as a template parameter, so that the body's discarded K-split steps, which name fields this block does
// not have, are not looked up; it is part of the kernels' symbol names)
template <int D, int DT, bool CAUSAL, class PA = FwdArgsBSP>
__global__ __launch_bounds__(256, 2) void flash_fwd_bsp_kernel(const PA p_in) {
  constexpr int NWAVES = 4;
  constexpr bool WIN = false;
#include "usp_flash_fwd_body.inc"
}

int launch_fwd_bsp(const FwdArgsBSP& p, int D, int dtype, bool causal, int grid, size_t lds, hipStream_t st) {
  return with_head_dim_dtype(D, dtype, [&](auto d, auto dt) -> int {
    constexpr int Dc = decltype(d)::value, DT = decltype(dt)::value;
    with_causal(causal, [&](auto c) {
      hipLaunchKernelGGL((flash_fwd_bsp_kernel<Dc, DT, decltype(c)::value>), dim3(grid), dim3(256), lds, st, p);
    });
    return launched();
  });
}

}  // namespace usp
