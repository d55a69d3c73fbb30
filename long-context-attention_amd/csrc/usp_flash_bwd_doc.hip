// Document-mask instantiations of the two-waves-per-SIMD backward kernels (C ABI: usp_flash_bwd_doc, include/usp_hip.h).
// The bodies are the ones usp_flash_bwd.hip compiles (usp_flash_bwd_dq_body.inc, usp_flash_bwd_dkdv_body.inc) with DOC = true: a left
// key bound read per row.  The dQ kernel owns rows and takes it as row_lo (row i sees key j only if j >= row_lo[i]); the dK/dV
// kernel owns keys and takes its transpose key_hi (only if i < key_hi[j]).  Both arrays are monotone (usp_tile_range.h), so an
// item's streamed range and a wave's live and masked tiles are two reads each: the dQ item starts at the first key its first
// row sees, the dK/dV item ends behind the last row that sees its last key.  Only role A of the dK/dV kernel masks: role B
// receives P = 0 for a hidden pair.  The lane's own bound is one register (both kernels have room for it: no scratch).
// 3 head dims x 2 types x causal / full x 2 launches = 24 kernels.
// A translation unit of its own: the build parallelises and the objects of the other kernels do not change.
#include "usp_bwd_params.hpp"
#include "usp_host.hpp"

namespace usp {

template <int D, int DT, bool CAUSAL>
__global__ __launch_bounds__(512, 2) void flash_bwd_doc_kernel(const BwdArgsDOC p_in) {
#include "usp_flash_bwd_dq_body.inc"
}

template <int D, int DT, bool CAUSAL>
__global__ __launch_bounds__(512, 2) void flash_bwd_dkdv_doc_kernel(const BwdArgsDOC p_in) {
#include "usp_flash_bwd_dkdv_body.inc"
}

int launch_dkdv_doc(const BwdArgsDOC& p, int D, int dtype, bool causal, int grid, size_t lds, hipStream_t st) {
  return with_head_dim_dtype(D, dtype, [&](auto d, auto dt) -> int {
    with_causal(causal, [&](auto c) {
      hipLaunchKernelGGL((flash_bwd_dkdv_doc_kernel<decltype(d)::value, decltype(dt)::value, decltype(c)::value>), dim3(grid),
                         dim3(512), lds, st, p);
    });
    return launched();
  });
}

int launch_dq_doc(const BwdArgsDOC& p, int D, int dtype, bool causal, int grid, size_t lds, hipStream_t st) {
  return with_head_dim_dtype(D, dtype, [&](auto d, auto dt) -> int {
    with_causal(causal, [&](auto c) {
      hipLaunchKernelGGL((flash_bwd_doc_kernel<decltype(d)::value, decltype(dt)::value, decltype(c)::value>), dim3(grid),
                         dim3(512), lds, st, p);
    });
    return launched();
  });
}

}  // namespace usp
