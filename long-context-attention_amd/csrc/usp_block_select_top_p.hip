// Top-p block selection: a second producer of the 128 x 128 block mask that usp_flash_fwd_bsp / usp_flash_bwd_bsp consume (C ABI:
// usp_block_select_top_p; include/usp_hip.h states the function, the order of every sum and the tie expression).  The pooled
// means come from usp_block_means (usp_block_select.hip), unchanged.  One kernel, no atomics, nothing read on the host, no inline
// assembly:
//   block_select_top_p_kernel  one workgroup per (b, h, row block) -- with share_group per (b, KV head, row block), looping over
//                        the group's query heads in ascending order.  Per head: the scores of the visible blocks in fp32 (one
//                        chain of fused multiply-adds over ascending d), the row maximum, one expf per block, Z, and the
//                        weights e / Z added into LDS.  Then the cut: the largest order-preserving key T with
//                        mass(forced or key >= T) >= top_p * total, found bit by bit (32 mass reductions); ties at the cut go
//                        to the lower J by a ballot prefix over ascending chunks of 256 blocks, as many as the tie expression
//                        asks for.  Every byte of the mask row(s) is written.
// Every reduction (block_sum) has one order, a function of J alone: thread t adds its blocks J = t, t + 256, ... ascending from
// 0.f; the 64 lanes of a wave are added by the butterfly x += x[lane ^ 32], ^ 16, ^ 8, ^ 4, ^ 2, ^ 1 (every lane holds the same
// bits afterwards: fp32 addition commutes); the four waves are added ((w0 + w1) + w2) + w3.  Terms left out of a sum enter it
// as 0.f, so a sum over a subset is the sum over all blocks with zeros: non-negative terms make it monotone in the subset.
#include "usp_host.hpp"

namespace usp {

constexpr int kTopPThreads = 256;

struct BlockSelectTopPArgs {
  const float* qbar;           // (B, nbq, Hq, D) contiguous
  const float* kbar;           // (B, nbk, Hkv, D) contiguous
  unsigned char* mask;
  int64_t sb, sh, sr;          // byte strides of batch, head, row block
  int Hq, Hkv, D, nbq, nbk, row_block0;
  float scale, top_p;
  int causal, keep_first, keep_local, share;
};

// ascending key <=> ascending float (usp_block_select.hip: order_key); a weight >= +0 has a key >= 0x80000000
USP_DEV uint32_t weight_key(float w) {
  if (w == 0.f) w = 0.f;
  const uint32_t u = __builtin_bit_cast(uint32_t, w);
  return (u & 0x80000000u) ? ~u : (u | 0x80000000u);
}

USP_DEV float wave_sum(float x) {
#pragma unroll
  for (int m = 32; m >= 1; m >>= 1) x += __shfl_xor(x, m, 64);
  return x;
}

USP_DEV float wave_max(float x) {
#pragma unroll
  for (int m = 32; m >= 1; m >>= 1) x = fmaxf(x, __shfl_xor(x, m, 64));
  return x;
}

// The sum / maximum over the workgroup, the same bits in every thread.  Two sets of four wave slots alternate (`phase`), so one
// barrier a reduction is enough: a set is written again only behind the barrier of the reduction between, which every thread
// reaches after it has read the set.
USP_DEV float block_sum(float x, float* slots, int& phase, int lane, int wave) {
  x = wave_sum(x);
  float* const w = slots + 4 * (phase++ & 1);
  if (lane == 0) w[wave] = x;
  __syncthreads();
  return ((w[0] + w[1]) + w[2]) + w[3];
}

USP_DEV float block_max(float x, float* slots, int& phase, int lane, int wave) {
  x = wave_max(x);
  float* const w = slots + 4 * (phase++ & 1);
  if (lane == 0) w[wave] = x;
  __syncthreads();
  return fmaxf(fmaxf(w[0], w[1]), fmaxf(w[2], w[3]));
}

__global__ __launch_bounds__(kTopPThreads) void block_select_top_p_kernel(const BlockSelectTopPArgs a) {
  extern __shared__ __attribute__((aligned(16))) uint32_t top_p_lds[];   // [nbk weights, padded to 4][nbk scratch][D floats of q][2 x 4 wave slots]
  const int nbk4 = (a.nbk + 3) & ~3;
  float* const wts = (float*)top_p_lds;
  float* const tmp = wts + nbk4;                   // a head's scores, then its exponentials
  float* const qs = tmp + nbk4;
  float* const slots = qs + a.D;
  const int t = threadIdx.x, lane = t & 63, wave = t >> 6;
  const int G = a.Hq / a.Hkv;
  const int heads = a.share ? a.Hkv : a.Hq;        // rows of the grid per (b, I)
  const int64_t id = blockIdx.x;                   // (b, head or KV head, I), I fastest: neighbours share the keys of one KV head
  const int I = (int)(id % a.nbq);
  const int64_t bh = id / a.nbq;
  const int hh = (int)(bh % heads), b = (int)(bh / heads);
  const int h0 = a.share ? hh * G : hh, nh = a.share ? G : 1, hkv = a.share ? hh : hh / G;
  const int Ig = a.row_block0 + I;
  const int nbk = a.nbk, D = a.D;
  // visible: [0, nv); forced: [0, kf) and [lo, hi] inside it
  const int nv = a.causal ? (Ig + 1 < nbk ? Ig + 1 : nbk) : nbk;
  const int kf = a.keep_first < nv ? a.keep_first : nv;
  const int lo = Ig - a.keep_local + 1 > 0 ? Ig - a.keep_local + 1 : 0;
  const int hi = Ig < nv - 1 ? Ig : nv - 1;
  const int n_local = hi >= lo ? hi - lo + 1 : 0;
  const int both = n_local > 0 && kf > lo ? (kf < hi + 1 ? kf : hi + 1) - lo : 0;
  const int n_cand = nv - (kf + n_local - both);
  const bool search = n_cand > 0;                  // (otherwise every visible block is forced: no weight decides anything)
  int phase = 0;

  if (search) {
    const float* const kb = a.kbar + ((int64_t)b * nbk * a.Hkv + hkv) * D;
    for (int g = 0; g < nh; ++g) {
      // (the last reads of the previous head's q lie in front of two barriers: block_max, block_sum)
      const float* const q = a.qbar + (((int64_t)b * a.nbq + I) * a.Hq + h0 + g) * D;
      for (int d = t; d < D; d += kTopPThreads) qs[d] = q[d];
      __syncthreads();
      float mx = -__builtin_inff();
      for (int J = t; J < nv; J += kTopPThreads) {
        const f32x4* const kr = (const f32x4*)(kb + (int64_t)J * a.Hkv * D);
        float s = 0.f;
        for (int d4 = 0; d4 < (D >> 2); ++d4) {
          const f32x4 kv = kr[d4];
          const f32x4 qv = *(const f32x4*)(qs + 4 * d4);
          s = __builtin_fmaf(qv[0], kv[0], s);
          s = __builtin_fmaf(qv[1], kv[1], s);
          s = __builtin_fmaf(qv[2], kv[2], s);
          s = __builtin_fmaf(qv[3], kv[3], s);
        }
        s *= a.scale;
        tmp[J] = s;
        mx = fmaxf(mx, s);
      }
      mx = block_max(mx, slots, phase, lane, wave);
      float z = 0.f;
      for (int J = t; J < nv; J += kTopPThreads) {   // (a thread reads what it wrote: tmp and wts need no barrier)
        const float e = expf(tmp[J] - mx);
        tmp[J] = e;
        z += e;
      }
      z = block_sum(z, slots, phase, lane, wave);
      for (int J = t; J < nbk; J += kTopPThreads) {
        const float w = J < nv ? tmp[J] / z : 0.f;
        wts[J] = g == 0 ? w : wts[J] + w;            // the group's heads in ascending order, each over its own Z
      }
    }
  }
  const auto is_forced = [&](int J) { return J < nv && (J < kf || (J >= lo && J <= hi)); };
  // key of block J: of its weight where it is a candidate, 0 (below every candidate's) elsewhere
  const auto key_of = [&](int J, float w) { return (J < nv && !is_forced(J)) ? weight_key(w) : 0u; };
  // mass(c) = sum of the weights of the forced blocks and of the candidates with key >= c
  const auto mass = [&](uint32_t c) {
    float acc = 0.f;
    for (int J = t; J < nbk; J += kTopPThreads) {
      const float w = wts[J];
      acc += (is_forced(J) || key_of(J, w) >= c) ? w : 0.f;
    }
    return block_sum(acc, slots, phase, lane, wave);
  };
  // the cut T, bit by bit: the largest T with mass(T) >= target (mass(0) = total >= target: top_p <= 1)
  uint32_t T = 0xFFFFFFFFu;
  float target = 0.f, m_gt = 0.f, wt = 0.f;
  int n_eq = 0, need = 0;
  if (search) {
    target = a.top_p * mass(0u);
    T = 0u;
    for (int bit = 31; bit >= 0; --bit) {
      const uint32_t c = T | (1u << bit);
      if (mass(c) >= target) T = c;
    }
    if (T != 0xFFFFFFFFu) {                        // (all ones: the forced blocks alone reach the target)
      m_gt = mass(T + 1u);
      float cnt = 0.f;
      for (int J = t; J < nbk; J += kTopPThreads) cnt += key_of(J, wts[J]) == T ? 1.f : 0.f;
      n_eq = (int)block_sum(cnt, slots, phase, lane, wave);       // (at most 8192: exact)
      wt = __builtin_bit_cast(float, T & 0x7FFFFFFFu);            // the weight every block of key T has
      // ties taken: the smallest c in [1, n_eq] with fmaf(c, wt, m_gt) >= target, n_eq where none has
      need = n_eq;
      if (n_eq > 0 && __builtin_fmaf((float)n_eq, wt, m_gt) >= target) {
        int c_lo = 1, c_hi = n_eq;
        while (c_lo < c_hi) {
          const int mid = (c_lo + c_hi) >> 1;
          if (__builtin_fmaf((float)mid, wt, m_gt) >= target) c_hi = mid; else c_lo = mid + 1;
        }
        need = c_lo;
      }
    }
  }
  int taken = 0;                                   // ties met in the chunks before this one
  unsigned char* const out = a.mask + b * a.sb + h0 * a.sh + I * a.sr;
  for (int J0 = 0; J0 < nbk; J0 += kTopPThreads) {
    const int J = J0 + t;
    const bool in = J < nbk;
    bool sel = in && is_forced(J);
    if (search) {
      const uint32_t key = in ? key_of(J, wts[J]) : 0u;
      const bool eq = in && key == T && key != 0u;
      const unsigned long long bal = __ballot(eq);
      float* const w = slots + 4 * (phase++ & 1);
      if (lane == 0) w[wave] = (float)__builtin_popcountll(bal);
      __syncthreads();
      int before = taken;
      for (int i = 0; i < wave; ++i) before += (int)w[i];
      taken += (int)(w[0] + w[1] + w[2] + w[3]);
      const int rank = before + __builtin_popcountll(bal & ((1ull << lane) - 1ull));
      sel = sel || (key > T) || (eq && rank < need);
    }
    if (in)
      for (int g = 0; g < nh; ++g) out[g * a.sh + J] = sel ? 1 : 0;
  }
}

}  // namespace usp

extern "C" int usp_block_select_top_p(const float* qbar, const float* kbar, int32_t B, int32_t Hq, int32_t Hkv, int32_t D,
                                      int32_t nbq, int32_t nbk, int32_t row_block0, float scale, int32_t causal, float top_p,
                                      int32_t keep_first, int32_t keep_local, int32_t share_group, void* mask,
                                      int64_t mask_stride_b, int64_t mask_stride_h, int64_t mask_stride_row, void* stream) {
  using namespace usp;
  if (!qbar || !kbar || !mask || B <= 0 || Hq <= 0 || Hkv <= 0 || D <= 0 || nbq <= 0 || nbk <= 0) return USP_EINVAL;
  if (row_block0 < 0 || keep_first < 0 || keep_local < 0 || (causal && keep_local < 1)) return USP_EINVAL;
  if (!(top_p > 0.f) || !(top_p <= 1.f)) return USP_EINVAL;          // NaN, <= 0, > 1
  if (mask_stride_b < 0 || mask_stride_h < 0 || mask_stride_row < 0 || !(scale == scale)) return USP_EINVAL;
  if (D % 8 || D > 128 || Hq % Hkv) return USP_EUNSUPPORTED;
  if (nbk > USP_BLOCK_SELECT_MAX_BLOCKS || (int64_t)row_block0 + nbq > (1 << 30)) return USP_EUNSUPPORTED;
  if (!aligned(qbar, 16) || !aligned(kbar, 16)) return USP_EUNSUPPORTED;
  const int64_t grid = (int64_t)B * (share_group ? Hkv : Hq) * nbq;
  if (grid >= (1LL << 31)) return USP_EUNSUPPORTED;
  BlockSelectTopPArgs a;
  a.qbar = qbar; a.kbar = kbar; a.mask = (unsigned char*)mask;
  a.sb = mask_stride_b; a.sh = mask_stride_h; a.sr = mask_stride_row;
  a.Hq = Hq; a.Hkv = Hkv; a.D = D; a.nbq = nbq; a.nbk = nbk; a.row_block0 = row_block0;
  a.scale = scale; a.top_p = top_p; a.causal = causal ? 1 : 0; a.keep_first = keep_first; a.keep_local = keep_local;
  a.share = share_group ? 1 : 0;
  const size_t lds = (2 * (size_t)((nbk + 3) & ~3) + D + 8) * 4;     // <= 2 * 8192 * 4 + 544 bytes of the 160 KiB
  if (lds > 64 * 1024 &&
      hipFuncSetAttribute((const void*)block_select_top_p_kernel, hipFuncAttributeMaxDynamicSharedMemorySize, (int)lds) != hipSuccess)
    return USP_ELAUNCH;
  hipLaunchKernelGGL(block_select_top_p_kernel, dim3((unsigned)grid), dim3(kTopPThreads), lds, (hipStream_t)stream, a);
  return launched();
}
