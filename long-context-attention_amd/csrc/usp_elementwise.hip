// HBM-bound helper kernels of libusp_hip.so: backward delta, stand-alone LSE merge, the row-gather
// copy behind the Ulysses all-to-all pack/unpack, its r-term summing form (KV heads shared by r ranks),
// fp32 -> 16-bit cast, fp32 add and the gradient of the attention sinks.
// All are pure streaming kernels: 16-byte accesses per lane, grid-stride loops capped at
// 256 CUs x 8 blocks (cdna_hip_programming.md Guideline 11/13).
#include "usp_host.hpp"

namespace usp {

constexpr int kEwThreads = 256;
static inline int ew_grid(int64_t work_items) {
  int64_t g = (work_items + kEwThreads - 1) / kEwThreads;
  if (g < 1) g = 1;
  if (g > 2048) g = 2048;
  return (int)g;
}

template <int DT> USP_DEV void unpack8(const u32x4& w, float (&f)[8]) {
#pragma unroll
  for (int i = 0; i < 4; ++i) {
    f[2 * i] = Elem<DT>::lo(w[i]);
    f[2 * i + 1] = Elem<DT>::hi(w[i]);
  }
}

// ---- delta[b,h,s] = sum_d dout * out --------------------------------------------------------------
// One (b,s,h) row per group of D/8 lanes (each lane 8 elements = 16 B), reduced with shuffles.
template <int D, int DT>
__global__ __launch_bounds__(kEwThreads) void delta_kernel(
    const char* dout, int64_t do_sb, int64_t do_ss, int64_t do_sh, const char* out, int64_t o_sb,
    int64_t o_ss, int64_t o_sh, float* delta, int64_t d_sb, int64_t d_sh, int B, int S, int H) {
  constexpr int LPR = D / 8;                       // lanes per row
  constexpr int RPB = kEwThreads / LPR;            // rows per block per iteration
  const int sub = threadIdx.x % LPR;
  const int64_t nrows = (int64_t)B * S * H;
  for (int64_t r = (int64_t)blockIdx.x * RPB + threadIdx.x / LPR; r < nrows;
       r += (int64_t)gridDim.x * RPB) {
    const int h = (int)(r % H);
    const int64_t bs = r / H;
    const int s = (int)(bs % S);
    const int b = (int)(bs / S);
    const u32x4 a = *(const u32x4*)(dout + 2 * (b * do_sb + (int64_t)s * do_ss + h * do_sh) + 16 * sub);
    const u32x4 c = *(const u32x4*)(out + 2 * (b * o_sb + (int64_t)s * o_ss + h * o_sh) + 16 * sub);
    float fa[8], fc[8];
    unpack8<DT>(a, fa);
    unpack8<DT>(c, fc);
    float acc = 0.f;
#pragma unroll
    for (int i = 0; i < 8; ++i) acc += fa[i] * fc[i];
#pragma unroll
    for (int m = LPR / 2; m >= 1; m >>= 1) acc += __shfl_xor(acc, m, 64);
    if (sub == 0) delta[b * d_sb + h * d_sh + s] = acc;
  }
}

// ---- stand-alone LSE merge ------------------------------------------------------------------------
template <int D, int DT>
__global__ __launch_bounds__(kEwThreads) void merge_kernel(
    float* acc, int64_t a_sb, int64_t a_ss, int64_t a_sh, float* lse, int64_t l_sb, int64_t l_sh,
    const char* bo, int64_t bo_sb, int64_t bo_ss, int64_t bo_sh, const float* bl, int64_t bl_sb,
    int64_t bl_sh, int B, int S, int H, int first) {
  constexpr int LPR = D / 8;
  constexpr int RPB = kEwThreads / LPR;
  const int sub = threadIdx.x % LPR;
  const int64_t nrows = (int64_t)B * S * H;
  for (int64_t r = (int64_t)blockIdx.x * RPB + threadIdx.x / LPR; r < nrows;
       r += (int64_t)gridDim.x * RPB) {
    const int h = (int)(r % H);
    const int64_t bs = r / H;
    const int s = (int)(bs % S);
    const int b = (int)(bs / S);
    const u32x4 w = *(const u32x4*)(bo + 2 * (b * bo_sb + (int64_t)s * bo_ss + h * bo_sh) + 16 * sub);
    float fb[8];
    unpack8<DT>(w, fb);
    const float blk = bl[b * bl_sb + h * bl_sh + s];
    float* ap = acc + b * a_sb + (int64_t)s * a_ss + h * a_sh + 8 * sub;
    float* lp = lse + b * l_sb + h * l_sh + s;
    float w_old = 0.f, w_blk = 1.f, nl = blk;
    if (!first) {
      const float old = *lp;
      const float mx = fmaxf(old, blk);
      if (mx == USP_NEG_INF) {
        w_old = 0.f; w_blk = 0.f; nl = USP_NEG_INF;
      } else {
        const float eo = exp2f((old - mx) * kLog2e), eb = exp2f((blk - mx) * kLog2e);
        const float sum = eo + eb;
        nl = mx + log2f(sum) * kLn2;
        w_old = eo / sum;
        w_blk = eb / sum;
      }
    }
    f32x4 v0 = {fb[0] * w_blk, fb[1] * w_blk, fb[2] * w_blk, fb[3] * w_blk};
    f32x4 v1 = {fb[4] * w_blk, fb[5] * w_blk, fb[6] * w_blk, fb[7] * w_blk};
    if (!first) {
      v0 += *(const f32x4*)ap * w_old;
      v1 += *(const f32x4*)(ap + 4) * w_old;
    }
    *(f32x4*)ap = v0;
    *(f32x4*)(ap + 4) = v1;
    // every lane of the row group read `old` above; the row's lanes sit in one wave
    if (sub == 0) *lp = nl;
  }
}

// ---- row-gather copy -------------------------------------------------------------------------------
__global__ __launch_bounds__(kEwThreads) void copy_rows_kernel(
    char* dst, const char* src, int64_t chunks_per_row, int64_t n1, int64_t n2, int64_t n3,
    int64_t total_chunks, int64_t ds0, int64_t ds1, int64_t ds2, int64_t ds3, int64_t ss0,
    int64_t ss1, int64_t ss2, int64_t ss3) {
  for (int64_t i = (int64_t)blockIdx.x * kEwThreads + threadIdx.x; i < total_chunks;
       i += (int64_t)gridDim.x * kEwThreads) {
    const int64_t cc = i % chunks_per_row;
    int64_t r = i / chunks_per_row;
    const int64_t i3 = r % n3; r /= n3;
    const int64_t i2 = r % n2; r /= n2;
    const int64_t i1 = r % n1;
    const int64_t i0 = r / n1;
    const u32x4 v = *(const u32x4*)(src + i0 * ss0 + i1 * ss1 + i2 * ss2 + i3 * ss3 + 16 * cc);
    *(u32x4*)(dst + i0 * ds0 + i1 * ds1 + i2 * ds2 + i3 * ds3 + 16 * cc) = v;
  }
}

// ---- row-gather with an r-term sum -----------------------------------------------------------------
// dst row = round(sum_t src row of term t), fp32 accumulation in ascending t: the dK/dV partials of the r Ulysses ranks
// that share one KV head (comm/all_to_all.py:unpack_kv_sum).  Terms are loaded four at a time so that up to four 16-byte
// reads per lane are in flight before the first add; the adds keep the ascending order.
template <int DT>
__global__ __launch_bounds__(kEwThreads) void sum_rows_kernel(
    char* dst, const char* src, int64_t chunks_per_row, int64_t n1, int64_t n2, int64_t total_chunks, int r,
    int64_t term_stride, int64_t ds0, int64_t ds1, int64_t ds2, int64_t ss0, int64_t ss1, int64_t ss2) {
  for (int64_t i = (int64_t)blockIdx.x * kEwThreads + threadIdx.x; i < total_chunks;
       i += (int64_t)gridDim.x * kEwThreads) {
    const int64_t cc = i % chunks_per_row;
    int64_t row = i / chunks_per_row;
    const int64_t i2 = row % n2; row /= n2;
    const int64_t i1 = row % n1;
    const int64_t i0 = row / n1;
    const char* sp = src + i0 * ss0 + i1 * ss1 + i2 * ss2 + 16 * cc;
    float acc[8];
#pragma unroll
    for (int e = 0; e < 8; ++e) acc[e] = 0.f;
    int t = 0;
    for (; t + 4 <= r; t += 4) {
      u32x4 w[4];
#pragma unroll
      for (int j = 0; j < 4; ++j) w[j] = *(const u32x4*)(sp + (t + j) * term_stride);
#pragma unroll
      for (int j = 0; j < 4; ++j) {
        float f[8];
        unpack8<DT>(w[j], f);
#pragma unroll
        for (int e = 0; e < 8; ++e) acc[e] += f[e];
      }
    }
    for (; t < r; ++t) {
      float f[8];
      unpack8<DT>(*(const u32x4*)(sp + t * term_stride), f);
#pragma unroll
      for (int e = 0; e < 8; ++e) acc[e] += f[e];
    }
    const u32x4 o = {Elem<DT>::pack2(acc[0], acc[1]), Elem<DT>::pack2(acc[2], acc[3]),
                     Elem<DT>::pack2(acc[4], acc[5]), Elem<DT>::pack2(acc[6], acc[7])};
    *(u32x4*)(dst + i0 * ds0 + i1 * ds1 + i2 * ds2 + 16 * cc) = o;
  }
}

// ---- fp32 -> 16-bit cast ---------------------------------------------------------------------------
template <int DT>
__global__ __launch_bounds__(kEwThreads) void cast_kernel(char* dst, int64_t d_rs, const float* src,
                                                          int64_t s_rs, int64_t rows, int64_t n8) {
  const int64_t total = rows * n8;
  for (int64_t i = (int64_t)blockIdx.x * kEwThreads + threadIdx.x; i < total;
       i += (int64_t)gridDim.x * kEwThreads) {
    const int64_t r = i / n8, c = i % n8;
    const float* sp = src + r * s_rs + 8 * c;
    const f32x4 a = *(const f32x4*)sp, b = *(const f32x4*)(sp + 4);
    u32x4 w = {Elem<DT>::pack2(a[0], a[1]), Elem<DT>::pack2(a[2], a[3]),
               Elem<DT>::pack2(b[0], b[1]), Elem<DT>::pack2(b[2], b[3])};
    *(u32x4*)(dst + 2 * (r * d_rs + 8 * c)) = w;
  }
}

// ---- fp32 add --------------------------------------------------------------------------------------
__global__ __launch_bounds__(kEwThreads) void add_kernel(float* dst, int64_t d_rs, const float* a,
                                                         int64_t a_rs, const float* b, int64_t b_rs,
                                                         int64_t rows, int64_t n4) {
  const int64_t total = rows * n4;
  for (int64_t i = (int64_t)blockIdx.x * kEwThreads + threadIdx.x; i < total;
       i += (int64_t)gridDim.x * kEwThreads) {
    const int64_t r = i / n4, c = i % n4;
    const f32x4 x = *(const f32x4*)(a + r * a_rs + 4 * c);
    const f32x4 y = *(const f32x4*)(b + r * b_rs + 4 * c);
    *(f32x4*)(dst + r * d_rs + 4 * c) = x + y;
  }
}

// ---- dsinks[h] (+)= -sum_{b,i} exp(sinks[h] - lse[b,h,i]) * delta[b,h,i] -----------------------------------------------
// One workgroup per head (B * S * 8 bytes to read): thread t sums the terms t, t + 1024, ... of every batch in that order
// with a compensated (Kahan) sum, then a fixed LDS tree: deterministic, no atomics.  A term whose lse is -inf counts as 0.
constexpr int kSinkThreads = 1024;
__global__ __launch_bounds__(kSinkThreads) void sink_bwd_kernel(const float* sinks, const float* lse, int64_t l_sb, int64_t l_sh,
                                                                const float* delta, int64_t d_sb, int64_t d_sh, float* dsinks,
                                                                int B, int S, int accum) {
  __shared__ float part[kSinkThreads];
  const int h = blockIdx.x, tid = threadIdx.x;
  const float s = sinks[h];
  float sum = 0.f, comp = 0.f;
  for (int b = 0; b < B; ++b) {
    const float* lp = lse + b * l_sb + h * l_sh;
    const float* dp = delta + b * d_sb + h * d_sh;
    for (int i = tid; i < S; i += kSinkThreads) {
      const float l = lp[i];
      const float term = l == USP_NEG_INF ? 0.f : expf(s - l) * dp[i];
      const float y = term - comp;
      const float t = sum + y;
      comp = (t - sum) - y;
      sum = t;
    }
  }
  part[tid] = sum;
  for (int st = kSinkThreads / 2; st > 0; st >>= 1) {
    __syncthreads();
    if (tid < st) part[tid] += part[tid + st];
  }
  if (tid == 0) dsinks[h] = accum ? dsinks[h] - part[0] : -part[0];
}

// ---- out[h] = max_{b,i} row_max[b,h,i]  (accum: ... and of out[h]) -----------------------------------------------------------
// One workgroup per head, as above (B * S * 4 bytes to read): thread t takes the maximum of the entries t, t + 1024, ... of every
// batch, then a fixed LDS tree.  A maximum does not depend on the order, so the result is exact; no atomics.
__global__ __launch_bounds__(kSinkThreads) void row_max_reduce_kernel(const float* row_max, int64_t r_sb, int64_t r_sh, float* out,
                                                                      int B, int S, int accum) {
  __shared__ float part[kSinkThreads];
  const int h = blockIdx.x, tid = threadIdx.x;
  float mx = USP_NEG_INF;
  for (int b = 0; b < B; ++b) {
    const float* rp = row_max + b * r_sb + h * r_sh;
    for (int i = tid; i < S; i += kSinkThreads) mx = fmaxf(mx, rp[i]);
  }
  part[tid] = mx;
  for (int st = kSinkThreads / 2; st > 0; st >>= 1) {
    __syncthreads();
    if (tid < st) part[tid] = fmaxf(part[tid], part[tid + st]);
  }
  if (tid == 0) out[h] = accum ? fmaxf(out[h], part[0]) : part[0];
}

}  // namespace usp

using namespace usp;

extern "C" int usp_row_max_reduce(int32_t B, int32_t S, int32_t H, const float* row_max, int64_t r_sb, int64_t r_sh, float* out,
                                  int32_t accum, void* stream) {
  if (!row_max || !out || B <= 0 || S <= 0 || H <= 0 || r_sb < 0 || r_sh < 0) return USP_EINVAL;
  hipLaunchKernelGGL(row_max_reduce_kernel, dim3(H), dim3(kSinkThreads), 0, (hipStream_t)stream, row_max, r_sb, r_sh, out, (int)B,
                     (int)S, accum ? 1 : 0);
  return launched();
}

extern "C" int usp_sink_bwd(int32_t B, int32_t S, int32_t H, const float* sinks, const float* lse, int64_t l_sb, int64_t l_sh,
                            const float* delta, int64_t d_sb, int64_t d_sh, float* dsinks, int32_t accum, void* stream) {
  if (!sinks || !lse || !delta || !dsinks || B <= 0 || S <= 0 || H <= 0) return USP_EINVAL;
  hipLaunchKernelGGL(sink_bwd_kernel, dim3(H), dim3(kSinkThreads), 0, (hipStream_t)stream, sinks, lse, l_sb, l_sh, delta, d_sb,
                     d_sh, dsinks, (int)B, (int)S, accum ? 1 : 0);
  return launched();
}

extern "C" int usp_bwd_delta(int32_t dtype, int32_t B, int32_t S, int32_t H, int32_t D,
                             const usp_tensor* dout, const usp_tensor* out, float* delta,
                             int64_t d_sb, int64_t d_sh, void* stream) {
  if (!dout || !out || !delta || B <= 0 || S <= 0 || H <= 0) return USP_EINVAL;
  if (dtype != USP_BF16 && dtype != USP_FP16) return USP_EINVAL;
  if (D != 32 && D != 64 && D != 128) return USP_EUNSUPPORTED;
  if (!tensor_aligned(*dout, 16, 8) || !tensor_aligned(*out, 16, 8)) return USP_EUNSUPPORTED;
  hipStream_t st = (hipStream_t)stream;
  const int64_t rows = (int64_t)B * S * H;
  const int grid = ew_grid(rows * (D / 8));
  return with_head_dim_dtype(D, dtype, [&](auto d, auto dt) {
    hipLaunchKernelGGL((delta_kernel<decltype(d)::value, decltype(dt)::value>), dim3(grid), dim3(kEwThreads), 0, st,
                       (const char*)dout->ptr, dout->stride_b, dout->stride_s, dout->stride_h,
                       (const char*)out->ptr, out->stride_b, out->stride_s, out->stride_h, delta, d_sb, d_sh, B, S, H);
    return launched();
  });
}

extern "C" int usp_lse_merge(int32_t dtype, int32_t B, int32_t S, int32_t H, int32_t D,
                             const usp_tensor* acc, float* lse, int64_t l_sb, int64_t l_sh,
                             const usp_tensor* bo, const float* bl, int64_t bl_sb, int64_t bl_sh,
                             int32_t first, void* stream) {
  if (!acc || !lse || !bo || !bl || B <= 0 || S <= 0 || H <= 0) return USP_EINVAL;
  if (dtype != USP_BF16 && dtype != USP_FP16) return USP_EINVAL;
  if (D != 32 && D != 64 && D != 128) return USP_EUNSUPPORTED;
  if (!tensor_aligned(*acc, 16, 4) || !tensor_aligned(*bo, 16, 8)) return USP_EUNSUPPORTED;
  hipStream_t st = (hipStream_t)stream;
  const int64_t rows = (int64_t)B * S * H;
  const int grid = ew_grid(rows * (D / 8));
  return with_head_dim_dtype(D, dtype, [&](auto d, auto dt) {
    hipLaunchKernelGGL((merge_kernel<decltype(d)::value, decltype(dt)::value>), dim3(grid), dim3(kEwThreads), 0, st,
                       (float*)acc->ptr, acc->stride_b, acc->stride_s, acc->stride_h, lse, l_sb, l_sh,
                       (const char*)bo->ptr, bo->stride_b, bo->stride_s, bo->stride_h, bl, bl_sb, bl_sh, B, S, H, first ? 1 : 0);
    return launched();
  });
}

extern "C" int usp_copy_rows(void* dst, const void* src, int64_t row_bytes, int64_t n0, int64_t n1,
                             int64_t n2, int64_t n3, int64_t ds0, int64_t ds1, int64_t ds2,
                             int64_t ds3, int64_t ss0, int64_t ss1, int64_t ss2, int64_t ss3,
                             void* stream) {
  if (!dst || !src || row_bytes <= 0 || n0 <= 0 || n1 <= 0 || n2 <= 0 || n3 <= 0) return USP_EINVAL;
  const int64_t all = row_bytes | ds0 | ds1 | ds2 | ds3 | ss0 | ss1 | ss2 | ss3;
  if ((all & 15) || !aligned(dst, 16) || !aligned(src, 16)) return USP_EUNSUPPORTED;
  const int64_t cpr = row_bytes / 16;
  const int64_t total = cpr * n0 * n1 * n2 * n3;
  hipLaunchKernelGGL(copy_rows_kernel, dim3(ew_grid(total)), dim3(kEwThreads), 0,
                     (hipStream_t)stream, (char*)dst, (const char*)src, cpr, n1, n2, n3, total, ds0,
                     ds1, ds2, ds3, ss0, ss1, ss2, ss3);
  return launched();
}

extern "C" int usp_sum_rows(int32_t dtype, void* dst, const void* src, int64_t row_bytes, int32_t r,
                            int64_t term_stride, int64_t n0, int64_t n1, int64_t n2, int64_t ds0, int64_t ds1,
                            int64_t ds2, int64_t ss0, int64_t ss1, int64_t ss2, void* stream) {
  if (!dst || !src || row_bytes <= 0 || r <= 0 || n0 <= 0 || n1 <= 0 || n2 <= 0) return USP_EINVAL;
  if (dtype != USP_BF16 && dtype != USP_FP16) return USP_EINVAL;
  const int64_t all = row_bytes | term_stride | ds0 | ds1 | ds2 | ss0 | ss1 | ss2;
  if ((all & 15) || !aligned(dst, 16) || !aligned(src, 16)) return USP_EUNSUPPORTED;
  const int64_t cpr = row_bytes / 16;
  const int64_t total = cpr * n0 * n1 * n2;
  const int grid = ew_grid(total);
  with_dtype(dtype, [&](auto dt) {
    hipLaunchKernelGGL(sum_rows_kernel<decltype(dt)::value>, dim3(grid), dim3(kEwThreads), 0, (hipStream_t)stream, (char*)dst,
                       (const char*)src, cpr, n1, n2, total, (int)r, term_stride, ds0, ds1, ds2, ss0, ss1, ss2);
  });
  return launched();
}

extern "C" int usp_cast_from_f32(int32_t dtype, void* dst, int64_t d_rs, const float* src,
                                 int64_t s_rs, int64_t rows, int64_t n, void* stream) {
  if (!dst || !src || rows <= 0 || n <= 0) return USP_EINVAL;
  if (dtype != USP_BF16 && dtype != USP_FP16) return USP_EINVAL;
  if ((n & 7) || (d_rs & 7) || (s_rs & 3) || !aligned(dst, 16) || !aligned(src, 16)) return USP_EUNSUPPORTED;
  const int64_t n8 = n / 8;
  const int grid = ew_grid(rows * n8);
  with_dtype(dtype, [&](auto dt) {
    hipLaunchKernelGGL(cast_kernel<decltype(dt)::value>, dim3(grid), dim3(kEwThreads), 0, (hipStream_t)stream,
                       (char*)dst, d_rs, src, s_rs, rows, n8);
  });
  return launched();
}

extern "C" int usp_add_f32(float* dst, int64_t d_rs, const float* a, int64_t a_rs, const float* b,
                           int64_t b_rs, int64_t rows, int64_t n, void* stream) {
  if (!dst || !a || !b || rows <= 0 || n <= 0) return USP_EINVAL;
  if ((n & 3) || (d_rs & 3) || (a_rs & 3) || (b_rs & 3) || !aligned(dst, 16) || !aligned(a, 16) || !aligned(b, 16))
    return USP_EUNSUPPORTED;
  const int64_t n4 = n / 4;
  hipLaunchKernelGGL(add_kernel, dim3(ew_grid(rows * n4)), dim3(kEwThreads), 0, (hipStream_t)stream,
                     dst, d_rs, a, a_rs, b, b_rs, rows, n4);
  return launched();
}

// ---- diagnostic: what the matrix pipe sustains on THIS part, on THESE operands -----------------------------------------
// An MFMA-only loop of the flash kernels' instruction (v_mfma_f32_32x32x16_{bf16}) on operands the caller provides
// (N(0,1) bf16 as the bench's inputs, or zeros): no LDS, no VALU, no memory traffic in the loop, eight independent
// accumulators, eight A and eight B fragments in rotation (64 distinct products per pass).  One or two waves per SIMD.
// The part clocks by power, and MFMA power depends on the operands' bit patterns: the rate this loop sustains on random
// operands is the ceiling a flash kernel can approach on the same box in the same run.
// Lane 0 of every wave records s_memtime (shader clock) and s_memrealtime (100 MHz) around the loop: sustained clock.
namespace usp {
__global__ __launch_bounds__(512, 1) void mfma_probe_kernel(const u32x4* ops, int n_frag, int iters, float* sink,
                                                            unsigned long long* clocks) {
  const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
  u32x4 a[8], b[8];
#pragma unroll
  for (int i = 0; i < 8; ++i) {            // every wave of the launch draws its own fragments from the operand buffer
    const unsigned w = (blockIdx.x * (blockDim.x >> 6) + wave) * 16 + i;
    a[i] = ops[((w * 64 + lane) * 2) % n_frag];
    b[i] = ops[((w * 64 + lane) * 2 + 1 + 128 * i) % n_frag];
  }
  f32x16 acc[8];
#pragma unroll
  for (int i = 0; i < 8; ++i)
#pragma unroll
    for (int r = 0; r < 16; ++r) acc[i][r] = 0.f;
  const unsigned long long t0 = __builtin_amdgcn_s_memtime(), r0 = __builtin_amdgcn_s_memrealtime();
  for (int it = 0; it < iters; ++it) {
#pragma unroll
    for (int m = 0; m < 64; ++m)
      acc[m & 7] = Elem<0>::mfma(a[m & 7], b[(m >> 3) & 7], acc[m & 7]);
  }
  const unsigned long long t1 = __builtin_amdgcn_s_memtime(), r1 = __builtin_amdgcn_s_memrealtime();
  float s = 0.f;
#pragma unroll
  for (int i = 0; i < 8; ++i)
#pragma unroll
    for (int r = 0; r < 16; ++r) s += acc[i][r];
  if (s == 123.456f) sink[threadIdx.x] = s;            // keeps the loop alive; practically never true
  if (clocks && lane == 0 && wave == 0 && blockIdx.x == 0) { clocks[0] = t1 - t0; clocks[1] = r1 - r0; }
}
}  // namespace usp

extern "C" int usp_mfma_probe(const void* operands, int64_t operand_bytes, int32_t iters, int32_t waves_per_simd,
                              float* sink, uint64_t* clocks, void* stream) {
  using namespace usp;
  if (!operands || operand_bytes < 16 * 4096 || iters <= 0 || !sink || (waves_per_simd != 1 && waves_per_simd != 2)) return USP_EINVAL;
  if (!aligned(operands, 16)) return USP_EUNSUPPORTED;
  hipLaunchKernelGGL(mfma_probe_kernel, dim3(device_cus()), dim3(256 * waves_per_simd), 0, (hipStream_t)stream,
                     (const u32x4*)operands, (int)(operand_bytes / 16), (int)iters, sink, (unsigned long long*)clocks);
  return launched();
}

extern "C" int usp_abi_version(void) { return USP_ABI_VERSION; }
extern "C" int usp_attn_features(void) { return USP_ATTN_WINDOW | USP_ATTN_SOFTCAP | USP_ATTN_SHIFT | USP_ATTN_ALIBI | USP_ATTN_DROPOUT | USP_ATTN_SINK | USP_ATTN_DOC | USP_ATTN_SPAN | USP_ATTN_BLOCK_MASK | USP_ATTN_MAX_LOGIT | USP_ATTN_BLOCK_SELECT | USP_ATTN_BLOCK_SELECT_TOP_P | USP_ATTN_BLOCK_MASS; }

// What the calling thread's last flash call launched (include/usp_hip.h: usp_last_launch_kinds).  Thread-local: the entry
// points share no mutable state.
namespace usp {
static thread_local int t_last_kinds = 0;
void launch_kinds_reset() { t_last_kinds = 0; }
void launch_kinds_note(int kind) { t_last_kinds |= kind; }
}  // namespace usp
extern "C" int usp_last_launch_kinds(void) { return usp::t_last_kinds; }

extern "C" const char* usp_strerror(int code) {
  switch (code) {
    case USP_OK: return "ok";
    case USP_EINVAL: return "invalid argument (null pointer, non-positive size or bad dtype)";
    case USP_EUNSUPPORTED:
      return "unsupported shape/layout (head_dim must be 32/64/128, Hq % Hkv == 0, 16-byte aligned "
             "pointers and strides; or a forced kernel family that does not serve the call)";
    case USP_ELAUNCH: return "HIP kernel launch failed";
  }
  return "unknown error";
}
