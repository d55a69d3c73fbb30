// Max-logit instantiations of the two-waves-per-SIMD forward (C ABI: usp_flash_fwd_maxlogit, include/usp_hip.h).
// The body is the one usp_flash_fwd.hip compiles (usp_flash_fwd_body.inc) with MAXL = true: every lane keeps the TRUE running
// maximum of the raw scores of its row beside the lazily raised reference m_run, and the epilogue writes it, times softmax_scale,
// to row_max[b, h, row] (a merging launch takes the maximum with the value there).  The tile loops are those of the plain family,
// pipelined interior tiles included: the pipelined loop folds the per-lane tile maximum its phase B forms anyway (one v_max a tile,
// never for the still unmasked tile that opens the generic tail), the generic softmax its masked tile maximum.  Two forms:
//   FORM 0  flash_fwd_kernel<.., KSPLIT = false>'s walk on the plain argument block: launches without a left bound;
//   FORM 2  flash_fwd_window_kernel's rotated walk, which keeps the main loop under a left window bound.
// (The numbering is the sink kernels'.  Their FORM 1, the K-split walk, has no instantiation here: k_splits is ignored under the
// switch and the launch served uncut, so nothing would ever launch it.)
// 3 head dims x 2 types x causal / full x 8 / 4 waves x 2 forms = 48 kernels.
// A translation unit of its own: the build parallelises and the objects of the other kernels do not change.
#include "usp_fwd_params.hpp"
#include "usp_host.hpp"

namespace usp {

template <int D, int DT, bool CAUSAL, int NWAVES, int FORM>
__global__ __launch_bounds__(64 * NWAVES, 2) void flash_fwd_maxl_kernel(const std::conditional_t<FORM == 0, FwdArgsMXP, FwdArgsMX> p_in) {
  constexpr bool WIN = FORM == 2;
#include "usp_flash_fwd_body.inc"
}

int launch_fwd_maxl(const FwdArgsMX& p, int D, int dtype, bool causal, int waves, int grid, size_t lds, hipStream_t st) {
  FwdArgsMXP plain;                                          // the argument block of form 0: FwdParams and the row maxima alone
  static_cast<FwdParams&>(plain) = p;
  static_cast<FwdMaxl&>(plain) = p;
  return with_head_dim_dtype(D, dtype, [&](auto d, auto dt) -> int {
    with_causal(causal, [&](auto c) {
      constexpr int Dc = decltype(d)::value, DT = decltype(dt)::value;
      constexpr bool C = decltype(c)::value;
      auto go = [&](auto nw) {
        constexpr int NW = decltype(nw)::value;
        if (p.win_on) hipLaunchKernelGGL((flash_fwd_maxl_kernel<Dc, DT, C, NW, 2>), dim3(grid), dim3(64 * NW), lds, st, p);
        else hipLaunchKernelGGL((flash_fwd_maxl_kernel<Dc, DT, C, NW, 0>), dim3(grid), dim3(64 * NW), lds, st, plain);
      };
      if (waves == 4) go(Int<4>{});
      else go(Int<8>{});
    });
    return launched();
  });
}

}  // namespace usp
