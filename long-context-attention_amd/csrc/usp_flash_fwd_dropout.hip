// Dropout instantiations of the two-waves-per-SIMD forward (C ABI: usp_flash_fwd_dropout, include/usp_hip.h).
// The body is the one usp_flash_fwd.hip compiles (usp_flash_fwd_body.inc), on the K-split instantiation -- which carries the
// left window bound and the generic tile loop -- with DR = true: every tile takes the generic loop, whose softmax adds the
// un-dropped P to the row sum (the LSE is that of the un-dropped scores: the ring and the K-split merge by it, unchanged), zeroes
// the dropped P in front of the PV MFMAs and leaves 256 / t to the epilogue's fp32 weight.  The mask is a function of global
// (batch, query head, row, key) alone (usp_dropout_rng.h): a K cut rebases the keys, so the key offset is carried with it.
// A translation unit of its own: the build parallelises and the objects of the other kernels do not change.
#include "usp_fwd_params.hpp"
#include "usp_host.hpp"

namespace usp {

template <int D, int DT, bool CAUSAL, int NWAVES>
__global__ __launch_bounds__(64 * NWAVES, 2) void flash_fwd_dropout_kernel(const FwdArgsDR p_in) {
  constexpr bool WIN = false;
#include "usp_flash_fwd_body.inc"
}

int launch_fwd_dropout(const FwdArgsDR& p, int D, int dtype, bool causal, int waves, int grid, size_t lds, hipStream_t st) {
  return with_head_dim_dtype(D, dtype, [&](auto d, auto dt) -> int {
    with_causal(causal, [&](auto c) {
      constexpr int Dc = decltype(d)::value, DT = decltype(dt)::value;
      constexpr bool C = decltype(c)::value;
      if (waves == 4) hipLaunchKernelGGL((flash_fwd_dropout_kernel<Dc, DT, C, 4>), dim3(grid), dim3(256), lds, st, p);
      else hipLaunchKernelGGL((flash_fwd_dropout_kernel<Dc, DT, C, 8>), dim3(grid), dim3(512), lds, st, p);
    });
    return launched();
  });
}

}  // namespace usp
