// Span instantiations of the two-waves-per-SIMD forward (C ABI: usp_flash_fwd_span, include/usp_hip.h).
// The body is the one usp_flash_fwd.hip compiles (usp_flash_fwd_body.inc), on the plain (unsplit) argument block, with DOC = true and
// SPAN = true: row i sees key j only if row_lo[i] <= j < row_hi[i], for monotone row_lo and row_hi (usp_tile_range.h).  The
// right bound stands where the causal diagonal stands in the other kernels -- the planner folds the diagonal into row_hi, so
// these kernels are never causal: the item streams no tile at or past the end of its last valid row, a wave's pipelined tiles
// end at its first row's bound, and the tiles between go through the masked loop.  The left bound keeps the document kernel's
// rebasing and rotated walk.  Both bounds of a lane's row lie in LDS (2 x 32 * NWAVES ints per workgroup) and are read in masked
// tiles only; the wave-uniform ones stay in scalar registers.
// 3 head dims x 2 types x 8 / 4 waves = 12 kernels.
// A translation unit of its own: the build parallelises and the objects of the other kernels do not change.
#include "usp_fwd_params.hpp"
#include "usp_host.hpp"

namespace usp {

// (PA: the argument block as a template parameter, so that the body's discarded K-split steps, which name fields this block does
// not have, are not looked up; it is part of the kernels' symbol names)
template <int D, int DT, int NWAVES, class PA = FwdArgsSPAN>
__global__ __launch_bounds__(64 * NWAVES, 2) void flash_fwd_span_kernel(const PA p_in) {
  constexpr bool WIN = false, CAUSAL = false;
#include "usp_flash_fwd_body.inc"
}

int launch_fwd_span(const FwdArgsSPAN& p, int D, int dtype, int waves, int grid, size_t lds, hipStream_t st) {
  return with_head_dim_dtype(D, dtype, [&](auto d, auto dt) -> int {
    constexpr int Dc = decltype(d)::value, DT = decltype(dt)::value;
    // behind the K/V buffers: the queue's two slots (unused: no packed batch), then the item's left and right row bounds
    if (waves == 4) hipLaunchKernelGGL((flash_fwd_span_kernel<Dc, DT, 4>), dim3(grid), dim3(256), lds + 16 + 2 * 128 * 4, st, p);
    else hipLaunchKernelGGL((flash_fwd_span_kernel<Dc, DT, 8>), dim3(grid), dim3(512), lds + 16 + 2 * 256 * 4, st, p);
    return launched();
  });
}

}  // namespace usp
