// Per-head e4m3 quantizer for the fp8 forward (usp_flash_fwd_fp8.hip).  C ABI: usp_quantize_fp8 (include/usp_hip.h).
//   descale[b, h] = amax over (s, d) of |x[b, s, h, d]| / 448   (1 for an all-zero head)
//   x8[b, s, h, d] = e4m3(x[b, s, h, d] / descale[b, h])          round to nearest even
// Two launches on one grid of (row chunk, head, batch) workgroups, no atomics, the same bits every run:
//   1. quantize_amax_kernel   a workgroup takes the maximum of its USP_QUANT_FP8_ROWS rows of one head -> partial[b, h, chunk]
//   2. quantize_cast_kernel   a workgroup reduces ITS head's partials (a few floats, L2-resident), takes the one fp32 division, and
//                             casts its rows; chunk 0 writes the descale
// Any strides.  Where both tensors have a unit last stride, 16-byte (x) / 8-byte (x8) aligned rows and D % 8 == 0, a thread moves 8
// elements (one dwordx4 load, one dwordx2 store); else one.  HBM-bound: x is read twice (the second time mostly from L2 / MALL for
// the sizes of one attention call), x8 written once.
#include "usp_host.hpp"
#include "usp_fp8.hpp"

namespace usp {

struct QuantArgs {
  const char* x; char* y; float* descale; float* partial;
  int64_t x_sb, x_ss, x_sh, x_sd, y_sb, y_ss, y_sh, y_sd;
  int S, H, D, nchunk;
};

// maximum over the workgroup's 256 threads, returned to all of them
USP_DEV float block_max(float v, USP_LDS float* red) {
#pragma unroll
  for (int o = 32; o > 0; o >>= 1) v = fmaxf(v, __shfl_xor(v, o));
  __syncthreads();                                         // (red may still be read from the previous call)
  if ((threadIdx.x & 63) == 0) red[threadIdx.x >> 6] = v;
  __syncthreads();
  return fmaxf(fmaxf(red[0], red[1]), fmaxf(red[2], red[3]));
}

template <int DT, bool VEC>
__global__ __launch_bounds__(256) void quantize_amax_kernel(const QuantArgs p) {
  using E = Elem<DT>;
  __shared__ float red[4];
  const int chunk = blockIdx.x, h = blockIdx.y, b = blockIdx.z;
  const int r0 = chunk * USP_QUANT_FP8_ROWS;
  const int rows = p.S - r0 < USP_QUANT_FP8_ROWS ? p.S - r0 : USP_QUANT_FP8_ROWS;
  const char* base = p.x + 2 * (b * p.x_sb + (int64_t)r0 * p.x_ss + h * p.x_sh);
  float m = 0.f;
  if (VEC) {
    const int d8 = p.D >> 3;
    for (int i = threadIdx.x; i < rows * d8; i += 256) {
      const int r = i / d8, c8 = i - r * d8;
      const u32x4 w = *(const u32x4*)(base + 2 * ((int64_t)r * p.x_ss + 8 * c8));
#pragma unroll
      for (int e = 0; e < 4; ++e) m = fmaxf(m, fmaxf(fabsf(E::lo(w[e])), fabsf(E::hi(w[e]))));
    }
  } else {
    for (int i = threadIdx.x; i < rows * p.D; i += 256) {
      const int r = i / p.D, d = i - r * p.D;
      m = fmaxf(m, fabsf(E::lo(*(const uint16_t*)(base + 2 * ((int64_t)r * p.x_ss + d * p.x_sd)))));
    }
  }
  m = block_max(m, (USP_LDS float*)red);
  if (threadIdx.x == 0) p.partial[((int64_t)b * p.H + h) * p.nchunk + chunk] = m;
}

USP_DEV float quantize_one(float x, float d) {
  const float q = x / d;                                   // |q| <= 448 (1 + 2^-22): clamped, never left to the conversion
  return fminf(fmaxf(q, -448.f), 448.f);
}

template <int DT, bool VEC>
__global__ __launch_bounds__(256) void quantize_cast_kernel(const QuantArgs p) {
  using E = Elem<DT>;
  __shared__ float red[4];
  const int chunk = blockIdx.x, h = blockIdx.y, b = blockIdx.z;
  const float* part = p.partial + ((int64_t)b * p.H + h) * p.nchunk;
  float m = 0.f;
  for (int i = threadIdx.x; i < p.nchunk; i += 256) m = fmaxf(m, part[i]);
  m = block_max(m, (USP_LDS float*)red);
  const float d = m > 0.f ? m / 448.f : 1.f;
  if (chunk == 0 && threadIdx.x == 0) p.descale[(int64_t)b * p.H + h] = d;
  const int r0 = chunk * USP_QUANT_FP8_ROWS;
  const int rows = p.S - r0 < USP_QUANT_FP8_ROWS ? p.S - r0 : USP_QUANT_FP8_ROWS;
  const char* src = p.x + 2 * (b * p.x_sb + (int64_t)r0 * p.x_ss + h * p.x_sh);
  char* dst = p.y + (b * p.y_sb + (int64_t)r0 * p.y_ss + h * p.y_sh);
  if (VEC) {
    const int d8 = p.D >> 3;
    for (int i = threadIdx.x; i < rows * d8; i += 256) {
      const int r = i / d8, c8 = i - r * d8;
      const u32x4 w = *(const u32x4*)(src + 2 * ((int64_t)r * p.x_ss + 8 * c8));
      u32x2 o;
#pragma unroll
      for (int e = 0; e < 2; ++e)
        o[e] = (uint32_t)fp8::pack4(quantize_one(E::lo(w[2 * e]), d), quantize_one(E::hi(w[2 * e]), d),
                                    quantize_one(E::lo(w[2 * e + 1]), d), quantize_one(E::hi(w[2 * e + 1]), d));
      *(u32x2*)(dst + (int64_t)r * p.y_ss + 8 * c8) = o;
    }
  } else {
    for (int i = threadIdx.x; i < rows * p.D; i += 256) {
      const int r = i / p.D, e = i - r * p.D;
      const float v = quantize_one(E::lo(*(const uint16_t*)(src + 2 * ((int64_t)r * p.x_ss + e * p.x_sd))), d);
      dst[(int64_t)r * p.y_ss + e * p.y_sd] = (char)(fp8::pack4(v, 0.f, 0.f, 0.f) & 0xff);
    }
  }
}

}  // namespace usp

extern "C" int usp_quantize_fp8(int32_t dtype, const usp_tensor* x, int64_t x_stride_d, const usp_tensor* x8, int64_t x8_stride_d,
                                float* descale, float* partial, int32_t B, int32_t S, int32_t H, int32_t D, void* stream) {
  using namespace usp;
  if (!x || !x8 || !x->ptr || !x8->ptr || !descale || !partial) return USP_EINVAL;
  if (dtype != USP_BF16 && dtype != USP_FP16) return USP_EINVAL;
  if (B <= 0 || S <= 0 || H <= 0 || D <= 0) return USP_EINVAL;
  if (!aligned(x->ptr, 2) || !aligned(descale, 4) || !aligned(partial, 4)) return USP_EUNSUPPORTED;
  if (H > 65535 || B > 65535 || (int64_t)USP_QUANT_FP8_ROWS * D >= (1LL << 24)) return USP_EUNSUPPORTED;   // grid y / z, 32-bit loop index
  QuantArgs p;
  p.x = (const char*)x->ptr; p.y = (char*)x8->ptr; p.descale = descale; p.partial = partial;
  p.x_sb = x->stride_b; p.x_ss = x->stride_s; p.x_sh = x->stride_h; p.x_sd = x_stride_d;
  p.y_sb = x8->stride_b; p.y_ss = x8->stride_s; p.y_sh = x8->stride_h; p.y_sd = x8_stride_d;
  p.S = S; p.H = H; p.D = D;
  p.nchunk = (S + USP_QUANT_FP8_ROWS - 1) / USP_QUANT_FP8_ROWS;
  const bool vec = D % 8 == 0 && x_stride_d == 1 && x8_stride_d == 1 && tensor_aligned(*x, 16, 8) && tensor_aligned(*x8, 8, 8);
  const dim3 grid(p.nchunk, H, B);
  hipStream_t st = (hipStream_t)stream;
  return with_dtype(dtype, [&](auto dt) -> int {
    constexpr int DT = decltype(dt)::value;
    if (vec) hipLaunchKernelGGL((quantize_amax_kernel<DT, true>), grid, dim3(256), 0, st, p);
    else hipLaunchKernelGGL((quantize_amax_kernel<DT, false>), grid, dim3(256), 0, st, p);
    if (launched() != USP_OK) return USP_ELAUNCH;
    if (vec) hipLaunchKernelGGL((quantize_cast_kernel<DT, true>), grid, dim3(256), 0, st, p);
    else hipLaunchKernelGGL((quantize_cast_kernel<DT, false>), grid, dim3(256), 0, st, p);
    return launched();
  });
}
