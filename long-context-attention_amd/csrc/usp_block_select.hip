// Top-k block selection: the producer of the 128 x 128 block mask that usp_flash_fwd_bsp / usp_flash_bwd_bsp consume (C ABI:
// usp_block_means, usp_block_select; include/usp_hip.h).  The MoBA gate at the kernels' block size: mean-pooled 128-row blocks
// of q against mean-pooled 128-key blocks of k, top-k per (batch, query head, row block).  Two kernels, no atomics, nothing
// read on the host, no inline assembly:
//   block_means_kernel   HBM-bound.  16-bit (B, S, H, D) -> fp32 (B, nb, H, D).  One (b, block, h) per group of D threads: the
//                        thread of (8 dims, run of 16 rows) adds its 16 rows in ascending order from 16-byte loads, and the
//                        8 runs of a dim are added in ascending order through LDS.  The order of every sum is a function of
//                        (row, d) alone: the result does not depend on B, H, the grid or which workgroup holds the block.
//                        (One lane per (b, block, h, 8 dims) walking all 128 rows, with no LDS, measured slower: 0.145 against
//                        0.062 ms at 16K tokens, profiles/block_select_rates.txt.)
//   block_select_kernel  one workgroup per (b, h, row block): the nbk scores in fp32 (one chain of fused multiply-adds over
//                        ascending d) become order-preserving 32-bit keys in LDS; the k-th largest key is found bit by bit (32
//                        counting passes, wave ballots + one LDS word per wave); ties at the cut go to the lower J by a
//                        ballot prefix over ascending chunks of 256 blocks.  Every byte of the mask row is written.
#include "usp_host.hpp"

namespace usp {

constexpr int kSelThreads = 256;
constexpr int kMeanRuns = 8, kMeanRunRows = USP_BLOCK_MASK_SIZE / kMeanRuns;     // 8 runs of 16 rows per block

struct BlockMeansArgs {
  const uint16_t* x;
  int64_t sb, ss, sh;          // element strides of batch, row, head
  float* out;                  // (B, nb, H, D) contiguous
  int64_t items;               // B * nb * H
  int S, H, D, nb;
};

template <int DT>
__global__ __launch_bounds__(256) void block_means_kernel(const BlockMeansArgs a) {
  __shared__ float part[256 * 8];                  // [item of the workgroup][run][d], D floats per run
  const int D = a.D, per = 256 / D;                // items per workgroup (D <= 128: at least 2)
  const int t = threadIdx.x, il = t / D, slot = t - il * D;
  const int64_t item = (int64_t)blockIdx.x * per + il;
  const bool on = il < per && item < a.items;
  const int c8 = D >> 3;                           // 16-byte chunks of a row
  const int run = slot / c8, d0 = (slot - run * c8) * 8;
  int count = 0;
  int64_t bb = 0;
  int h = 0;
  if (on) {
    h = (int)(item % a.H);
    bb = item / a.H;                               // b * nb + blk
    const int blk = (int)(bb % a.nb);
    const int b = (int)(bb / a.nb);
    const int row0 = blk * USP_BLOCK_MASK_SIZE;
    count = a.S - row0 < USP_BLOCK_MASK_SIZE ? a.S - row0 : USP_BLOCK_MASK_SIZE;
    const uint16_t* const p = a.x + b * a.sb + h * a.sh + d0;
    float acc[8] = {0.f, 0.f, 0.f, 0.f, 0.f, 0.f, 0.f, 0.f};
    const int r_begin = run * kMeanRunRows;
#pragma unroll
    for (int i = 0; i < kMeanRunRows; ++i) {       // (16 independent 16-byte loads in flight per lane)
      const int r = r_begin + i;
      if (r < count) {
        const u32x4 w = *(const u32x4*)(p + (int64_t)(row0 + r) * a.ss);
#pragma unroll
        for (int j = 0; j < 4; ++j) {
          acc[2 * j] += Elem<DT>::lo(w[j]);
          acc[2 * j + 1] += Elem<DT>::hi(w[j]);
        }
      }
    }
    float* const dst = part + (il * kMeanRuns + run) * D + d0;
#pragma unroll
    for (int j = 0; j < 8; ++j) dst[j] = acc[j];
  }
  __syncthreads();
  if (on) {                                        // thread `slot` finishes dim d = slot
    const float* const src = part + il * kMeanRuns * D + slot;
    float s = src[0];
#pragma unroll
    for (int g = 1; g < kMeanRuns; ++g) s += src[g * D];
    a.out[(bb * a.H + h) * D + slot] = s / (float)count;
  }
}

struct BlockSelectArgs {
  const float* qbar;           // (B, nbq, Hq, D) contiguous
  const float* kbar;           // (B, nbk, Hkv, D) contiguous
  unsigned char* mask;
  int64_t sb, sh, sr;          // byte strides of batch, head, row block
  int Hq, Hkv, D, nbq, nbk, row_block0;
  float scale;
  int causal, top_k, keep_first, keep_local;
};

// ascending key <=> ascending float; every number (the infinities included) gets a key >= 1
USP_DEV uint32_t order_key(float s) {
  if (s == 0.f) s = 0.f;                           // -0 ties with +0
  const uint32_t u = __builtin_bit_cast(uint32_t, s);
  return (u & 0x80000000u) ? ~u : (u | 0x80000000u);
}

__global__ __launch_bounds__(kSelThreads) void block_select_kernel(const BlockSelectArgs a) {
  extern __shared__ __attribute__((aligned(16))) uint32_t sel_lds[];   // [nbk keys, padded to 4][D floats of q][2 x 4 wave counts]
  const int nbk4 = (a.nbk + 3) & ~3;
  uint32_t* const keys = sel_lds;
  float* const qs = (float*)(sel_lds + nbk4);
  uint32_t* const wcnt = sel_lds + nbk4 + a.D;
  const int t = threadIdx.x, lane = t & 63, wave = t >> 6;
  const int64_t id = blockIdx.x;                   // (b, h, I), I fastest: neighbours share the keys of one KV head
  const int I = (int)(id % a.nbq);
  const int64_t bh = id / a.nbq;
  const int h = (int)(bh % a.Hq), b = (int)(bh / a.Hq);
  const int Ig = a.row_block0 + I;
  const int nbk = a.nbk, D = a.D;
  // visible: [0, nv); forced: [0, kf) and [lo, hi] inside it
  const int nv = a.causal ? (Ig + 1 < nbk ? Ig + 1 : nbk) : nbk;
  const int kf = a.keep_first < nv ? a.keep_first : nv;
  const int lo = Ig - a.keep_local + 1 > 0 ? Ig - a.keep_local + 1 : 0;
  const int hi = Ig < nv - 1 ? Ig : nv - 1;
  const int n_local = hi >= lo ? hi - lo + 1 : 0;
  const int both = n_local > 0 && kf > lo ? (kf < hi + 1 ? kf : hi + 1) - lo : 0;
  const int n_forced = kf + n_local - both;
  const int n_cand = nv - n_forced;
  const int k_rem = a.top_k > n_forced ? a.top_k - n_forced : 0;

  const float* const q = a.qbar + (((int64_t)b * a.nbq + I) * a.Hq + h) * D;
  for (int d = t; d < D; d += kSelThreads) qs[d] = q[d];
  __syncthreads();
  const bool search = k_rem > 0 && k_rem < n_cand;
  if (search) {                                    // (otherwise no score decides anything)
    const float* const kb = a.kbar + ((int64_t)b * nbk * a.Hkv + h / (a.Hq / a.Hkv)) * D;
    for (int J = t; J < nbk; J += kSelThreads) {
      const bool cand = J < nv && J >= kf && !(J >= lo && J <= hi);
      uint32_t key = 0;
      if (cand) {
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
        key = order_key(a.scale * s);
      }
      keys[J] = key;
    }
    __syncthreads();
  }
  // the k_rem-th largest key T, bit by bit: the largest T with count(key >= T) >= k_rem
  uint32_t T = 0;
  int n_ge = 0;                                    // count(key >= T) of the final T
  if (search) {
    for (int bit = 31; bit >= 0; --bit) {
      const uint32_t c = T | (1u << bit);
      int cnt = 0;
      for (int J0 = 0; J0 < nbk; J0 += kSelThreads) {
        const int J = J0 + t;
        cnt += __builtin_popcountll(__ballot(J < nbk && keys[J] >= c));
      }
      uint32_t* const w = wcnt + 4 * (bit & 1);
      if (lane == 0) w[wave] = (uint32_t)cnt;
      __syncthreads();
      const int total = (int)(w[0] + w[1] + w[2] + w[3]);
      if (total >= k_rem) { T = c; n_ge = total; }
    }
  }
  // (T >= 1 for numbers: at least k_rem candidates have a key >= 1.)  Ties at the cut: the first `need` of the keys == T.
  const bool scan = search && n_ge > k_rem;
  int n_gt = 0;
  if (scan) {
    int cnt = 0;
    for (int J0 = 0; J0 < nbk; J0 += kSelThreads) {
      const int J = J0 + t;
      cnt += __builtin_popcountll(__ballot(J < nbk && keys[J] > T));
    }
    __syncthreads();                               // (the last counting pass has been read by every wave)
    if (lane == 0) wcnt[wave] = (uint32_t)cnt;
    __syncthreads();
    n_gt = (int)(wcnt[0] + wcnt[1] + wcnt[2] + wcnt[3]);
    __syncthreads();
  }
  const int need = k_rem - n_gt;
  int taken = 0;                                   // ties taken in the chunks before this one
  unsigned char* const out = a.mask + b * a.sb + h * a.sh + I * a.sr;
  for (int J0 = 0, it = 0; J0 < nbk; J0 += kSelThreads, ++it) {
    const int J = J0 + t;
    const bool in = J < nbk;
    const bool forced = in && J < nv && (J < kf || (J >= lo && J <= hi));
    const bool cand = in && J < nv && !forced;
    bool sel = forced || (cand && k_rem >= n_cand);
    if (search) {
      const uint32_t key = in ? keys[J] : 0u;
      if (!scan) {
        sel = sel || (cand && key >= T);
      } else {
        const bool eq = cand && key == T;
        const unsigned long long bal = __ballot(eq);
        uint32_t* const w = wcnt + 4 * (it & 1);
        if (lane == 0) w[wave] = (uint32_t)__builtin_popcountll(bal);
        __syncthreads();
        int before = taken;
        for (int i = 0; i < wave; ++i) before += (int)w[i];
        taken += (int)(w[0] + w[1] + w[2] + w[3]);
        const int rank = before + __builtin_popcountll(bal & ((1ull << lane) - 1ull));
        sel = sel || (cand && key > T) || (eq && rank < need);
      }
    }
    if (in) out[J] = sel ? 1 : 0;
  }
}

}  // namespace usp

extern "C" int usp_block_means(const void* x, int32_t dtype, int32_t B, int32_t S, int32_t H, int32_t D, int64_t stride_b,
                               int64_t stride_s, int64_t stride_h, float* out, void* stream) {
  using namespace usp;
  if (!x || !out || B <= 0 || S <= 0 || H <= 0 || D <= 0 || (dtype != USP_BF16 && dtype != USP_FP16)) return USP_EINVAL;
  if (stride_b < 0 || stride_s < 0 || stride_h < 0) return USP_EINVAL;
  if (D % 8 || D > 128) return USP_EUNSUPPORTED;
  if (!tensor_aligned(x, stride_b, stride_s, stride_h, 16, 8) || !aligned(out, 4)) return USP_EUNSUPPORTED;
  BlockMeansArgs a;
  a.x = (const uint16_t*)x; a.sb = stride_b; a.ss = stride_s; a.sh = stride_h; a.out = out;
  a.S = S; a.H = H; a.D = D; a.nb = (S + USP_BLOCK_MASK_SIZE - 1) / USP_BLOCK_MASK_SIZE;
  a.items = (int64_t)B * a.nb * H;
  const int per = 256 / D;
  const int64_t grid = (a.items + per - 1) / per;
  if (grid >= (1LL << 31)) return USP_EUNSUPPORTED;
  with_dtype(dtype, [&](auto dt) {
    hipLaunchKernelGGL(block_means_kernel<decltype(dt)::value>, dim3((unsigned)grid), dim3(256), 0, (hipStream_t)stream, a);
    return 0;
  });
  return launched();
}

extern "C" int usp_block_select(const float* qbar, const float* kbar, int32_t B, int32_t Hq, int32_t Hkv, int32_t D, int32_t nbq,
                                int32_t nbk, int32_t row_block0, float scale, int32_t causal, int32_t top_k, int32_t keep_first,
                                int32_t keep_local, void* mask, int64_t mask_stride_b, int64_t mask_stride_h, int64_t mask_stride_row,
                                void* stream) {
  using namespace usp;
  if (!qbar || !kbar || !mask || B <= 0 || Hq <= 0 || Hkv <= 0 || D <= 0 || nbq <= 0 || nbk <= 0) return USP_EINVAL;
  if (row_block0 < 0 || top_k < 0 || keep_first < 0 || keep_local < 0 || (causal && keep_local < 1)) return USP_EINVAL;
  if (mask_stride_b < 0 || mask_stride_h < 0 || mask_stride_row < 0 || !(scale == scale)) return USP_EINVAL;
  if (D % 8 || D > 128 || Hq % Hkv) return USP_EUNSUPPORTED;
  if (nbk > USP_BLOCK_SELECT_MAX_BLOCKS || (int64_t)row_block0 + nbq > (1 << 30)) return USP_EUNSUPPORTED;
  if (!aligned(qbar, 16) || !aligned(kbar, 16)) return USP_EUNSUPPORTED;
  const int64_t grid = (int64_t)B * Hq * nbq;
  if (grid >= (1LL << 31)) return USP_EUNSUPPORTED;
  BlockSelectArgs a;
  a.qbar = qbar; a.kbar = kbar; a.mask = (unsigned char*)mask;
  a.sb = mask_stride_b; a.sh = mask_stride_h; a.sr = mask_stride_row;
  a.Hq = Hq; a.Hkv = Hkv; a.D = D; a.nbq = nbq; a.nbk = nbk; a.row_block0 = row_block0;
  a.scale = scale; a.causal = causal ? 1 : 0; a.top_k = top_k; a.keep_first = keep_first; a.keep_local = keep_local;
  const size_t lds = ((size_t)((nbk + 3) & ~3) + D + 8) * 4;      // <= 8192 * 4 + 544 bytes
  hipLaunchKernelGGL(block_select_kernel, dim3((unsigned)grid), dim3(kSelThreads), lds, (hipStream_t)stream, a);
  return launched();
}
