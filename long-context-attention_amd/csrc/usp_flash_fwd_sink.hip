// Attention-sink instantiations of the two-waves-per-SIMD forward (C ABI: usp_flash_fwd_sink, include/usp_hip.h).
// The body is the one usp_flash_fwd.hip compiles (usp_flash_fwd_body.inc) with SINK = true, which changes the epilogue alone: the
// block result is merged with the constant block (o = 0, lse = sinks[h]) on the item that opens the rows' state.  The tile
// loops are those of the plain family, pipelined interior tiles included -- unlike softcap, ALiBi and dropout nothing is done
// per score, so nothing falls to the generic loop.  Three forms, the three the plain dispatch of usp_flash_fwd.hip has:
//   FORM 0  flash_fwd_kernel<.., KSPLIT = false>'s walk on the plain argument block: launches without cuts and without a left bound
//           (at D = 128 the split form spills 8 VGPRs where this one spills 4: 2.2 % of the forward rate, profiles/sink_rates.txt);
//   FORM 1  flash_fwd_kernel<.., KSPLIT = true>'s: K-split launches -- cut 0 carries the sink;
//   FORM 2  flash_fwd_window_kernel's rotated walk, which keeps the main loop under a left window bound (cut or not) -- the
//           GPT-OSS layers alternate window 128 and full causal, so both are hot.
// 3 head dims x 2 types x causal / full x 8 / 4 waves x 3 forms = 72 kernels.
// A translation unit of its own: the build parallelises and the objects of the other kernels do not change.
#include "usp_fwd_params.hpp"
#include "usp_host.hpp"

namespace usp {

template <int D, int DT, bool CAUSAL, int NWAVES, int FORM>
__global__ __launch_bounds__(64 * NWAVES, 2) void flash_fwd_sink_kernel(const std::conditional_t<FORM == 0, FwdArgsSKP, FwdArgsSK> p_in) {
  constexpr bool WIN = FORM == 2;
#include "usp_flash_fwd_body.inc"
}

int launch_fwd_sink(const FwdArgsSK& p, int D, int dtype, bool causal, int waves, int grid, size_t lds, hipStream_t st) {
  FwdArgsSKP plain;                                          // the argument block of form 0: FwdParams and the sinks alone
  static_cast<FwdParams&>(plain) = p;
  plain.sinks = p.sinks;
  return with_head_dim_dtype(D, dtype, [&](auto d, auto dt) -> int {
    with_causal(causal, [&](auto c) {
      constexpr int Dc = decltype(d)::value, DT = decltype(dt)::value;
      constexpr bool C = decltype(c)::value;
      auto go = [&](auto nw) {
        constexpr int NW = decltype(nw)::value;
        if (p.win_on) hipLaunchKernelGGL((flash_fwd_sink_kernel<Dc, DT, C, NW, 2>), dim3(grid), dim3(64 * NW), lds, st, p);
        else if (p.ksplit > 1) hipLaunchKernelGGL((flash_fwd_sink_kernel<Dc, DT, C, NW, 1>), dim3(grid), dim3(64 * NW), lds, st, p);
        else hipLaunchKernelGGL((flash_fwd_sink_kernel<Dc, DT, C, NW, 0>), dim3(grid), dim3(64 * NW), lds, st, plain);
      };
      if (waves == 4) go(Int<4>{});
      else go(Int<8>{});
    });
    return launched();
  });
}

}  // namespace usp
