// ALiBi instantiations of the two-waves-per-SIMD forward (C ABI: usp_flash_fwd_alibi, include/usp_hip.h).
// The body is the one usp_flash_fwd.hip compiles (usp_flash_fwd_body.inc), on the K-split instantiation -- which carries the
// left window bound and the generic tile loop -- with AL = true: every tile takes the generic loop, where the raw score becomes
//     s2 = raw * scale_log2 - slope * log2(e) * |row + al_diag - key|
// before the mask, and the online softmax runs with c = 1 (as for softcap).  The LSE is the true logsumexp of the biased scores:
// the ring merges by it.  A translation unit of its own: the build parallelises and the objects of the other kernels do not change.
#include "usp_fwd_params.hpp"
#include "usp_host.hpp"

namespace usp {

template <int D, int DT, bool CAUSAL, int NWAVES>
__global__ __launch_bounds__(64 * NWAVES, 2) void flash_fwd_alibi_kernel(const FwdArgsAL p_in) {
  constexpr bool WIN = false;
#include "usp_flash_fwd_body.inc"
}

int launch_fwd_alibi(const FwdArgsAL& p, int D, int dtype, bool causal, int waves, int grid, size_t lds, hipStream_t st) {
  return with_head_dim_dtype(D, dtype, [&](auto d, auto dt) -> int {
    with_causal(causal, [&](auto c) {
      constexpr int Dc = decltype(d)::value, DT = decltype(dt)::value;
      constexpr bool C = decltype(c)::value;
      if (waves == 4) hipLaunchKernelGGL((flash_fwd_alibi_kernel<Dc, DT, C, 4>), dim3(grid), dim3(256), lds, st, p);
      else hipLaunchKernelGGL((flash_fwd_alibi_kernel<Dc, DT, C, 8>), dim3(grid), dim3(512), lds, st, p);
    });
    return launched();
  });
}

}  // namespace usp
