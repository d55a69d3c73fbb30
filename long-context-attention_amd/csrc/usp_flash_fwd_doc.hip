// Document-mask instantiations of the two-waves-per-SIMD forward (C ABI: usp_flash_fwd_doc, include/usp_hip.h).
// The body is the one usp_flash_fwd.hip compiles (usp_flash_fwd_body.inc), on the plain (unsplit) argument block, with DOC = true:
// a left key bound read per row, row i sees key j only if j >= row_lo[i], for a monotone row_lo (usp_tile_range.h).  It keeps the
// window kernel's rotated walk: the key tiles in front of the item's first visible key are not streamed at all, the tiles the
// bound cuts for no row of the item go first through the pipelined main loop, and the cut ones follow through the masked loop.
// A one-document launch (row_lo = 0) and every item inside a long document walk exactly as flash_fwd_kernel does.
// The lane's own bound lies in LDS (32 * NWAVES ints per workgroup) and is read in masked tiles only: the plain kernels sit on
// the register cliff, and a bound held across the pipelined loop would cost them a register there.
// 3 head dims x 2 types x causal / full x 8 / 4 waves = 24 kernels.
// A translation unit of its own: the build parallelises and the objects of the other kernels do not change.
#include "usp_fwd_params.hpp"
#include "usp_host.hpp"

namespace usp {

// (PA: the argument block as a template parameter, so that the body's discarded K-split steps, which name fields this block does
// not have, are not looked up; it is part of the kernels' symbol names)
template <int D, int DT, bool CAUSAL, int NWAVES, class PA = FwdArgsDOC>
__global__ __launch_bounds__(64 * NWAVES, 2) void flash_fwd_doc_kernel(const PA p_in) {
  constexpr bool WIN = false;
#include "usp_flash_fwd_body.inc"
}

int launch_fwd_doc(const FwdArgsDOC& p, int D, int dtype, bool causal, int waves, int grid, size_t lds, hipStream_t st) {
  return with_head_dim_dtype(D, dtype, [&](auto d, auto dt) -> int {
    with_causal(causal, [&](auto c) {
      constexpr int Dc = decltype(d)::value, DT = decltype(dt)::value;
      constexpr bool C = decltype(c)::value;
      // behind the K/V buffers: the queue's two slots (unused: no packed batch), then the item's row bounds
      if (waves == 4) hipLaunchKernelGGL((flash_fwd_doc_kernel<Dc, DT, C, 4>), dim3(grid), dim3(256), lds + 16 + 128 * 4, st, p);
      else hipLaunchKernelGGL((flash_fwd_doc_kernel<Dc, DT, C, 8>), dim3(grid), dim3(512), lds + 16 + 256 * 4, st, p);
    });
    return launched();
  });
}

}  // namespace usp
