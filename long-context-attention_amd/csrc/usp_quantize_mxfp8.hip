// MXFP8 quantizer for the MX forward (usp_flash_fwd_mxfp8.hip).  C ABI: usp_quantize_mxfp8 (include/usp_hip.h).  OCP Microscaling v1.0:
//   amax  = the block's largest magnitude, e = floor(log2(amax)) - 8 clamped to [-127, 127] (8 = e4m3's largest exponent),
//   scale byte (E8M0) = e + 127; an all-zero block gets 127
//   x8    = e4m3(x * 2^-e), round to nearest even, SATURATING at +-448: the quotient's largest magnitude lies in [256, 512), and
//           what lies above 448 clamps.  That is the format's conversion rule, not a shortcut taken here.
// floor(log2) is the exponent field of the fp32 value (an fp16 subnormal is an fp32 normal; an fp32 subnormal lands on the clamp
// either way) and the scaling is a multiplication by an exact power of two, so the result is defined bit for bit.
// A block is 32 elements along the head dim of one token (USP_MX_AXIS_D: q and k) or along the sequence of one (b, h, d)
// (USP_MX_AXIS_S: v; a ragged last block has the rows that exist).  ONE launch per call, x read once, no atomics, no scratch:
//   axis d   a thread takes 8 consecutive dims, the 4 lanes of a block share their maximum by two lane exchanges
//   axis s   a thread takes 4 consecutive dims of the block's 32 rows and keeps them in 64 registers between the maximum and the cast
// Any strides.  With unit last strides and aligned rows a thread moves its dims of a row in one load and one store; else by elements.
#include "usp_host.hpp"
#include "usp_mxfp8.hpp"

namespace usp {

struct QuantMXArgs {
  const char* x; char* y; char* sc;
  int64_t x_sb, x_ss, x_sh, x_sd, y_sb, y_ss, y_sh, y_sd, sc_sb, sc_ss, sc_sh;
  int64_t total;                             // threads with work
  int S, H, D, nblk;
};

// E8M0 byte of a block of largest magnitude `amax` (>= 0, finite), and the exact factor 2^-e its elements are multiplied by
USP_DEV int mx_scale_byte(float amax, float* factor) {
  const int field = (int)((__builtin_bit_cast(uint32_t, amax) >> 23) & 0xffu);     // floor(log2) + 127 of a normal value
  int byte = field - 8;                                                            // e + 127
  byte = byte < 0 ? 0 : byte;                                                      // (the field stops at 254: e <= 119)
  if (!(amax > 0.f)) byte = mx::kOne;
  *factor = __builtin_bit_cast(float, (uint32_t)(254 - byte) << 23);               // 2^(127 - byte), normal: 254 - byte >= 8
  return byte;
}
USP_DEV float mx_quotient(float x, float factor) { return fminf(fmaxf(x * factor, -448.f), 448.f); }

template <int DT, bool VEC>
__global__ __launch_bounds__(256) void quantize_mx_d_kernel(const QuantMXArgs p) {
  using E = Elem<DT>;
  const int64_t i = (int64_t)blockIdx.x * 256 + threadIdx.x;
  const bool valid = i < p.total;            // (whole groups of 4 lanes: D / 8 is a multiple of 4)
  const int d8 = p.D >> 3;
  const int c8 = (int)(i % d8);
  int64_t rest = i / d8;
  const int h = (int)(rest % p.H); rest /= p.H;
  const int s = (int)(rest % p.S);
  const int64_t b = rest / p.S;
  u32x4 w = {0u, 0u, 0u, 0u};
  if (valid) {
    const char* src = p.x + 2 * (b * p.x_sb + (int64_t)s * p.x_ss + h * p.x_sh);
    if (VEC) {
      w = *(const u32x4*)(src + 16 * c8);
    } else {
#pragma unroll
      for (int e = 0; e < 4; ++e)
        w[e] = (uint32_t)*(const uint16_t*)(src + 2 * (8 * c8 + 2 * e) * p.x_sd) |
               ((uint32_t)*(const uint16_t*)(src + 2 * (8 * c8 + 2 * e + 1) * p.x_sd) << 16);
    }
  }
  float m = 0.f;
#pragma unroll
  for (int e = 0; e < 4; ++e) m = fmaxf(m, fmaxf(fabsf(E::lo(w[e])), fabsf(E::hi(w[e]))));
  m = fmaxf(m, __shfl_xor(m, 1));
  m = fmaxf(m, __shfl_xor(m, 2));
  if (!valid) return;
  float f;
  const int byte = mx_scale_byte(m, &f);
  u32x2 o;
#pragma unroll
  for (int e = 0; e < 2; ++e)
    o[e] = (uint32_t)fp8::pack4(mx_quotient(E::lo(w[2 * e]), f), mx_quotient(E::hi(w[2 * e]), f), mx_quotient(E::lo(w[2 * e + 1]), f),
                                mx_quotient(E::hi(w[2 * e + 1]), f));
  char* dst = p.y + (b * p.y_sb + (int64_t)s * p.y_ss + h * p.y_sh);
  if (VEC) {
    *(u32x2*)(dst + 8 * c8) = o;
  } else {
#pragma unroll
    for (int e = 0; e < 8; ++e) dst[(8 * c8 + e) * p.y_sd] = (char)((o[e >> 2] >> (8 * (e & 3))) & 0xffu);
  }
  if ((c8 & 3) == 0) p.sc[b * p.sc_sb + (int64_t)s * p.sc_ss + h * p.sc_sh + (c8 >> 2)] = (char)byte;
}

template <int DT, bool VEC>
__global__ __launch_bounds__(256) void quantize_mx_s_kernel(const QuantMXArgs p) {
  using E = Elem<DT>;
  const int64_t i = (int64_t)blockIdx.x * 256 + threadIdx.x;
  if (i >= p.total) return;
  const int d4 = p.D >> 2;
  const int c4 = (int)(i % d4);
  int64_t rest = i / d4;
  const int h = (int)(rest % p.H); rest /= p.H;
  const int blk = (int)(rest % p.nblk);
  const int64_t b = rest / p.nblk;
  const int r0 = blk * mx::kBlock;
  const int rows = p.S - r0 < mx::kBlock ? p.S - r0 : mx::kBlock;
  const char* src = p.x + 2 * (b * p.x_sb + (int64_t)r0 * p.x_ss + h * p.x_sh);
  u32x2 w[mx::kBlock];
#pragma unroll
  for (int r = 0; r < mx::kBlock; ++r) {
    w[r] = u32x2{0u, 0u};
    if (r < rows) {
      const char* row = src + 2 * (int64_t)r * p.x_ss;
      if (VEC) {
        w[r] = *(const u32x2*)(row + 8 * c4);
      } else {
#pragma unroll
        for (int e = 0; e < 2; ++e)
          w[r][e] = (uint32_t)*(const uint16_t*)(row + 2 * (4 * c4 + 2 * e) * p.x_sd) |
                    ((uint32_t)*(const uint16_t*)(row + 2 * (4 * c4 + 2 * e + 1) * p.x_sd) << 16);
      }
    }
  }
  float m[4] = {0.f, 0.f, 0.f, 0.f};
#pragma unroll
  for (int r = 0; r < mx::kBlock; ++r) {
    m[0] = fmaxf(m[0], fabsf(E::lo(w[r][0]))); m[1] = fmaxf(m[1], fabsf(E::hi(w[r][0])));
    m[2] = fmaxf(m[2], fabsf(E::lo(w[r][1]))); m[3] = fmaxf(m[3], fabsf(E::hi(w[r][1])));
  }
  float f[4];
  uint32_t bytes = 0u;
#pragma unroll
  for (int e = 0; e < 4; ++e) bytes |= (uint32_t)mx_scale_byte(m[e], &f[e]) << (8 * e);
  *(uint32_t*)(p.sc + (b * p.sc_sb + (int64_t)blk * p.sc_ss + h * p.sc_sh + 4 * c4)) = bytes;
  char* dst = p.y + (b * p.y_sb + (int64_t)r0 * p.y_ss + h * p.y_sh);
#pragma unroll
  for (int r = 0; r < mx::kBlock; ++r) {
    if (r < rows) {
      const uint32_t o = (uint32_t)fp8::pack4(mx_quotient(E::lo(w[r][0]), f[0]), mx_quotient(E::hi(w[r][0]), f[1]),
                                              mx_quotient(E::lo(w[r][1]), f[2]), mx_quotient(E::hi(w[r][1]), f[3]));
      char* row = dst + (int64_t)r * p.y_ss;
      if (VEC) {
        *(uint32_t*)(row + 4 * c4) = o;
      } else {
#pragma unroll
        for (int e = 0; e < 4; ++e) row[(4 * c4 + e) * p.y_sd] = (char)((o >> (8 * e)) & 0xffu);
      }
    }
  }
}

}  // namespace usp

extern "C" int usp_quantize_mxfp8(int32_t dtype, int32_t axis, const usp_tensor* x, int64_t x_stride_d, const usp_tensor* x8,
                                  int64_t x8_stride_d, const usp_tensor* scale, int32_t B, int32_t S, int32_t H, int32_t D, void* stream) {
  using namespace usp;
  if (!x || !x8 || !scale || !x->ptr || !x8->ptr || !scale->ptr) return USP_EINVAL;
  if (dtype != USP_BF16 && dtype != USP_FP16) return USP_EINVAL;
  if (axis != USP_MX_AXIS_D && axis != USP_MX_AXIS_S) return USP_EINVAL;
  if (B <= 0 || S <= 0 || H <= 0 || D <= 0) return USP_EINVAL;
  if (D % mx::kBlock != 0 || !aligned(x->ptr, 2)) return USP_EUNSUPPORTED;
  const bool by_s = axis == USP_MX_AXIS_S;
  if (by_s && !tensor_aligned(*scale, 4, 4)) return USP_EUNSUPPORTED;               // four dims' bytes are one store
  QuantMXArgs p;
  p.x = (const char*)x->ptr; p.y = (char*)x8->ptr; p.sc = (char*)scale->ptr;
  p.x_sb = x->stride_b; p.x_ss = x->stride_s; p.x_sh = x->stride_h; p.x_sd = x_stride_d;
  p.y_sb = x8->stride_b; p.y_ss = x8->stride_s; p.y_sh = x8->stride_h; p.y_sd = x8_stride_d;
  p.sc_sb = scale->stride_b; p.sc_ss = scale->stride_s; p.sc_sh = scale->stride_h;
  p.S = S; p.H = H; p.D = D;
  p.nblk = (S + mx::kBlock - 1) / mx::kBlock;
  p.total = by_s ? (int64_t)B * p.nblk * H * (D / 4) : (int64_t)B * S * H * (D / 8);
  const int64_t grid = (p.total + 255) / 256;
  if (grid >= (1LL << 31)) return USP_EUNSUPPORTED;
  const bool unit = x_stride_d == 1 && x8_stride_d == 1;
  const bool vec = unit && (by_s ? tensor_aligned(*x, 8, 4) && tensor_aligned(*x8, 4, 4) : tensor_aligned(*x, 16, 8) && tensor_aligned(*x8, 8, 8));
  hipStream_t st = (hipStream_t)stream;
  return with_dtype(dtype, [&](auto dt) -> int {
    constexpr int DT = decltype(dt)::value;
    if (by_s && vec) hipLaunchKernelGGL((quantize_mx_s_kernel<DT, true>), dim3((unsigned)grid), dim3(256), 0, st, p);
    else if (by_s) hipLaunchKernelGGL((quantize_mx_s_kernel<DT, false>), dim3((unsigned)grid), dim3(256), 0, st, p);
    else if (vec) hipLaunchKernelGGL((quantize_mx_d_kernel<DT, true>), dim3((unsigned)grid), dim3(256), 0, st, p);
    else hipLaunchKernelGGL((quantize_mx_d_kernel<DT, false>), dim3((unsigned)grid), dim3(256), 0, st, p);
    return launched();
  });
}
