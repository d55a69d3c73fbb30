// Antidiagonal block weights: the XAttention gate at the kernels' block size (C ABI: usp_block_antidiag_weights; include/usp_hip.h
// states the function and the order of every sum).  With s = stride, sub-row r / sub-column c the s x s patch of rows r s .. and
// keys c s .., the sub-score a[r][c] = (scale / s) * sum_t q[r s + s-1-t] . k[c s + t] is the sum over ONE antidiagonal of the
// patch; p = softmax of a over the visible sub-columns, and w[I][J] is the mean over the sub-rows of block I of the p that falls
// on the sub-columns of block J.  For a fixed t the sum is an ordinary Q K^T between every s-th row of q and every s-th row of k:
//   block_antidiag_kernel  4 waves; a wave owns one UNIT = 32 sub-rows of one query head, and the four units of an item share one
//                      KV head: min(G, 4) query heads of the group side by side (G = 3: one wave idles), and where G < 4 the
//                      next 4 / G sub-row tiles beside them -- every K stage in LDS is read by four units whatever G is.  K goes
//                      through a two-deep LDS ring of STAGES filled by LDS-DMA straight from the strided rows: a stage is 32
//                      sub-columns x 4 antidiagonals = the 128 rows (c0 + c) s + t0 + tt of k (512 D bytes for both buffers,
//                      the forward's slot swizzle on the source side), one barrier a stage.  Q is the B operand, fetched by
//                      strided row addressing into registers: for s = 4 / 8 the whole chain's fragments stay resident for the
//                      item (D or 2 D VGPRs), for s = 16 the fragments of the next four antidiagonals are fetched a stage
//                      ahead into the set the previous stage has left.  One v_mfma_f32_32x32x16 chain of depth s D per 32 x 32
//                      tile of sub-scores: t ascending, d ascending inside.
// TWO SWEEPS over the item's stages: the first keeps a running (max, sum) per lane and ends in the row's
// log2-sum-exp, the second forms p against it and the block sums; the matrix work is 2 / s of Q K^T.  A wave owns whole 128-row
// blocks, so no sum crosses waves and LDS holds K alone.  No atomics, ordinary vector stores, nothing read on the host.  Rows and
// keys past S enter as 0 (q by a select on a clamped address, k by the buffer descriptor's range check).
// ORDER (y = sub-score in log2 units, one fma each; lane = (sub-row l = lane & 31, half hf = lane >> 5); register r of a tile
// holds sub-column 32 tile + 4 hf + (r & 3) + 8 (r >> 2)):
//   lse   per lane over the tiles ascending: m' = max(m, y_0 .. y_15); l = l * exp2(m - m'); l += exp2(y_r - m') for r = 0 .. 15;
//         then the halves: M = max(m(0), m(1)), L = l(0) exp2(m(0) - M) + l(1) exp2(m(1) - M), lse2 = M + log2(L);
//   w     per lane the p = exp2(y_r - lse2) of one block J ascending in r from 0.f (16 / (s / 4) registers), the halves
//         x(hf = 0) + x(hf = 1), the n = 128 / s sub-rows of block I by the butterfly x += x[l ^ n/2], .. , x[l ^ 1], one division
//         by rows'(I).  Hidden sub-columns and sub-rows past S enter as +0.
// A function of the position inside the block alone: the result repeats from call to call and does not depend on B, H or the grid.
#include "usp_host.hpp"
#include "usp_fwd_params.hpp"

namespace usp {

constexpr int kAdWaves = 4;
constexpr int kAdTile = 32;                      // sub-rows of a unit, sub-columns of a tile
constexpr int kAdStageT = 4;                     // antidiagonals per LDS stage
constexpr int kAdStageRows = kAdTile * kAdStageT;

struct BlockAntidiagArgs {
  const char* q; const char* k;
  float* out;
  int64_t q_sb, q_ss, q_sh;                      // element strides of batch, row, head
  int64_t k_sb, k_ss, k_sh;
  int64_t o_sb, o_sh, o_sr;                      // element strides of batch, head, row block
  int S, Hkv, G, nb, n_items;
  int hw;                                        // query heads side by side in an item: 1, 2 or 4
  int n_rg, n_hc;                                // items along the sequence, head chunks per KV group
  int causal;
  float c;                                       // (scale / stride) * log2(e)
};

template <int D, int DT, int STRIDE>
__global__ __launch_bounds__(64 * kAdWaves) void block_antidiag_kernel(const BlockAntidiagArgs a) {
  using E = Elem<DT>;
  constexpr int NW = kAdWaves;
  constexpr int ROWB = D * 2;                    // bytes per K row
  constexpr int SBYTES = kAdStageRows * ROWB;    // one stage
  constexpr int NKT = D / 16;                    // k-steps per antidiagonal
  constexpr int NF = kAdStageT * NKT;            // Q fragments per stage
  constexpr int CPW = SBYTES / 1024 / NW;        // 1 KiB pieces per wave per stage (D / 16)
  constexpr int SPT = STRIDE / kAdStageT;        // stages per tile = key blocks per tile = row blocks per unit
  constexpr int NQ = SPT < 2 ? 1 : 2;            // Q fragment sets in registers
  constexpr int NSUB = 128 / STRIDE;             // sub-rows per 128-block
  constexpr int RPJ = 16 / SPT;                  // registers of a lane per key block
  extern __shared__ __attribute__((aligned(16))) char smem_raw[];
  USP_LDS char* smem = (USP_LDS char*)smem_raw;

  const int tid = threadIdx.x;
  const int lane = tid & 63;
  const int wave = __builtin_amdgcn_readfirstlane(tid >> 6);
  const int l31 = lane & 31;
  const int hi = lane >> 5;
  const int n_sub = (a.S + STRIDE - 1) / STRIDE;             // sub-rows = sub-columns with a position < S
  const int n_ct = (n_sub + kAdTile - 1) / kAdTile;
  const int rtw = NW / a.hw;                                 // sub-row tiles side by side in an item

  const ItemWalk walk(a.n_items);
  for (int pass = 0;; ++pass) {
    int w = walk.at(pass);
    if (w < 0) break;
    const int rg_r = w % a.n_rg;
    int rest = w / a.n_rg;
    const int rg = a.causal ? (a.n_rg - 1 - rg_r) : rg_r;    // heavy (late) rows first
    const int hc = rest % a.n_hc;
    rest /= a.n_hc;
    const int hkv = rest % a.Hkv;
    const int b = rest / a.Hkv;
    const int g = hc * a.hw + wave % a.hw;
    const int rt = rg * rtw + wave / a.hw;                   // this wave's sub-row tile
    const int r0 = rt * kAdTile;
    const bool active = g < a.G && r0 < n_sub;               // (wave-uniform)
    const int h = hkv * a.G + (g < a.G ? g : a.G - 1);
    const int rr = r0 + l31;                                 // this lane's sub-row

    // ---- tiles of sub-columns the item and this wave reach ----
    int nct_item = n_ct, nct_wave = active ? n_ct : 0;
    if (a.causal) {
      nct_item = rg * rtw + rtw < n_ct ? rg * rtw + rtw : n_ct;
      nct_wave = active ? rt + 1 : 0;                        // (rt < n_ct)
    }
    const int n_st = nct_item * SPT;

    // ---- Q fragments (B operand: lane holds q[row][16 kt + 8 hi .. + 7]) of the antidiagonals 4 tg .. 4 tg + 3 ----
    const char* const qbase = a.q + 2 * (b * a.q_sb + h * a.q_sh) + 16 * hi;
    auto load_q = [&](int tg, u32x4* qf) {
#pragma unroll
      for (int tt = 0; tt < kAdStageT; ++tt) {
        const int64_t row = (int64_t)rr * STRIDE + (STRIDE - 1 - (tg * kAdStageT + tt));
        const bool in = row < a.S;
        const char* const qp = qbase + 2 * ((in ? row : (int64_t)a.S - 1) * a.q_ss);
#pragma unroll
        for (int kt = 0; kt < NKT; ++kt) {
          const u32x4 v = *(const u32x4*)(qp + 32 * kt);
          qf[tt * NKT + kt] = in ? v : u32x4{0u, 0u, 0u, 0u};
        }
      }
    };
    u32x4 qf[NQ][NF];

    // ---- K staging: LDS row R = 32 tt + c of a stage is the k row (c0 + c) s + t0 + tt; 16-byte slots swizzled at the source ----
    const char* const kbase = a.k + 2 * (b * a.k_sb + hkv * a.k_sh);
    int k_voff[CPW];
#pragma unroll
    for (int i = 0; i < CPW; ++i) {
      const int R = (wave + NW * i) * (1024 / ROWB) + lane / (D / 8);
      const int c8 = (lane % (D / 8)) ^ KSwz<D>::of(R);
      k_voff[i] = ((R & 31) * STRIDE + (R >> 5)) * (int)a.k_ss * 2 + c8 * 16;
    }
    auto dma_k = [&](int st) {
      const int64_t row0 = (int64_t)(st / SPT) * kAdTile * STRIDE + (st % SPT) * kAdStageT;
      // num_records makes every row >= S read as 0
      int64_t rem = ((a.S - 1 - row0) * a.k_ss + D) * 2;
      rem = rem < 0 ? 0 : (rem > 0xffffffffLL ? 0xffffffffLL : rem);
      const auto rs_ = __builtin_amdgcn_make_buffer_rsrc((void*)(kbase + row0 * a.k_ss * 2), 0, (int)(uint32_t)rem, 0x00020000);
#pragma unroll
      for (int i = 0; i < CPW; ++i) lds_dma16(rs_, smem + (st & 1) * SBYTES + (wave + NW * i) * 1024, k_voff[i]);
    };
    const int k_rd_row = l31 * ROWB;
    const int k_rd_x = hi ^ KSwz<D>::of(l31);                // (the swizzle of row 32 tt + l is that of row l)

    const int rows_left = n_sub - r0;                        // sub-rows of this unit with a position < S, if <= 32
    float nl = 0.f;                                          // -(log2-sum-exp) of this lane's sub-row
    for (int sweep = 0; sweep < 2; ++sweep) {
      if (active) {
        load_q(0, qf[0]);
        if constexpr (SPT == 2) load_q(1, qf[1]);
      }
      if (n_st > 0) dma_k(0);
      dma_drain();
      __syncthreads();
      float m_run = -3.0e38f, l_run = 0.f;
      for (int ct = 0; ct < nct_item; ++ct) {
        const bool mine = ct < nct_wave;
        f32x16 acc;
#pragma unroll
        for (int r = 0; r < 16; ++r) acc[r] = 0.f;
#pragma unroll
        for (int tg = 0; tg < SPT; ++tg) {
          const int st = ct * SPT + tg;
          if (st + 1 < n_st) dma_k(st + 1);                  // its buffer held stage st - 1: last read in front of the previous barrier
          if constexpr (SPT > 2) {
            if (active) load_q((tg + 1) % SPT, qf[(tg + 1) & 1]);
          }
          if (mine) {
            USP_LDS const char* const kb = smem + (st & 1) * SBYTES + k_rd_row;
#pragma unroll
            for (int tt = 0; tt < kAdStageT; ++tt)
#pragma unroll
              for (int kt = 0; kt < NKT; ++kt) {
                const u32x4 ka = *(USP_LDS const u32x4*)(kb + tt * kAdTile * ROWB + ((2 * kt) ^ k_rd_x) * 16);
                acc = E::mfma(ka, qf[tg & (NQ - 1)][tt * NKT + kt], acc);
              }
          }
          dma_drain();
          __syncthreads();
        }
        if (!mine) continue;
        // ---- the tile's 32 x 32 sub-scores: register r is sub-column cc0 + (r & 3) + 8 (r >> 2) of sub-row rr ----
        const int cc0 = ct * kAdTile + 4 * hi;
        int clim = n_sub - 1;                                // last visible sub-column
        if (a.causal) clim = rr < clim ? rr : clim;
        if (sweep == 0) {
          float tmax = m_run;
#pragma unroll
          for (int r = 0; r < 16; ++r) {
            const bool vis = cc0 + (r & 3) + 8 * (r >> 2) <= clim;
            tmax = fmaxf(tmax, vis ? acc[r] * a.c : USP_NEG_INF);
          }
          l_run *= fast_exp2(m_run - tmax);
#pragma unroll
          for (int r = 0; r < 16; ++r) {
            const bool vis = cc0 + (r & 3) + 8 * (r >> 2) <= clim;
            l_run += vis ? fast_exp2(__builtin_fmaf(acc[r], a.c, -tmax)) : 0.f;
          }
          m_run = tmax;
        } else {
          float x[SPT];
#pragma unroll
          for (int jj = 0; jj < SPT; ++jj) {
            float sum = 0.f;
#pragma unroll
            for (int r = jj * RPJ; r < (jj + 1) * RPJ; ++r) {
              const bool vis = cc0 + (r & 3) + 8 * (r >> 2) <= clim;
              sum += vis ? fast_exp2(__builtin_fmaf(acc[r], a.c, nl)) : 0.f;
            }
            x[jj] = sum;
          }
#pragma unroll
          for (int jj = 0; jj < SPT; ++jj) {
            float v = xhalf_sum(x[jj]);
#pragma unroll
            for (int m = NSUB / 2; m >= 1; m >>= 1) v += __shfl_xor(v, m, 64);
            const int I = rr / NSUB, J = ct * SPT + jj;
            if (hi == 0 && (l31 % NSUB) == 0 && I < a.nb && J < a.nb) {
              const int left = n_sub - I * NSUB;
              a.out[b * a.o_sb + h * a.o_sh + I * a.o_sr + J] = v / (float)(left < NSUB ? left : NSUB);
            }
          }
        }
      }
      if (sweep == 0) {
        float m0, m1, l0, l1;
        xhalf_pair(m_run, m0, m1);
        xhalf_pair(l_run, l0, l1);
        const float M = fmaxf(m0, m1);
        const float L = l0 * fast_exp2(m0 - M) + l1 * fast_exp2(m1 - M);
        // a sub-row past S gets -inf: fma(s, c, -inf) = -inf and exp2 gives +0
        nl = (l31 < rows_left) ? -(M + __builtin_log2f(L)) : USP_NEG_INF;
      }
    }
    // key blocks this unit's row blocks do not reach (above the diagonal): written as 0
    if (active) {
#pragma unroll
      for (int ii = 0; ii < SPT; ++ii) {
        const int I = r0 / NSUB + ii;
        if (I < a.nb) {
          float* const orow = a.out + b * a.o_sb + h * a.o_sh + I * a.o_sr;
          for (int J = nct_wave * SPT + lane; J < a.nb; J += 64) orow[J] = 0.f;
        }
      }
    }
  }  // next item
}

template <int D, int DT, int STRIDE> int launch_block_antidiag(const BlockAntidiagArgs& a, hipStream_t st) {
  // persistent launch: two workgroups per CU where the registers of the Q fragments leave room for two, else one
  const size_t lds = 2 * kAdStageRows * D * 2;               // 16 / 32 / 64 KiB
  static std::atomic<int> per_cu{0};                         // 0 = not asked yet (the answer is the same on every device of a kind)
  int n = per_cu.load(std::memory_order_relaxed);
  if (n == 0) {
    if (hipOccupancyMaxActiveBlocksPerMultiprocessor(&n, block_antidiag_kernel<D, DT, STRIDE>, 64 * kAdWaves, lds) != hipSuccess || n < 1) n = 1;
    n = n > 2 ? 2 : n;
    per_cu.store(n, std::memory_order_relaxed);
  }
  const int grid = persistent_grid(a.n_items, device_cus() * n, 0);
  hipLaunchKernelGGL((block_antidiag_kernel<D, DT, STRIDE>), dim3(grid), dim3(64 * kAdWaves), lds, st, a);
  launch_kinds_note(USP_KIND_BLOCK_ANTIDIAG);
  return launched();
}

}  // namespace usp

extern "C" int usp_block_antidiag_weights(const void* q, const void* k, int32_t dtype, int32_t B, int32_t S, int32_t Hq, int32_t Hkv,
                                          int32_t D, int64_t q_stride_b, int64_t q_stride_s, int64_t q_stride_h, int64_t k_stride_b,
                                          int64_t k_stride_s, int64_t k_stride_h, float scale, int32_t causal, int32_t stride,
                                          float* out, int64_t out_stride_b, int64_t out_stride_h, int64_t out_stride_row,
                                          void* stream) {
  using namespace usp;
  launch_kinds_reset();
  if (!q || !k || !out || B <= 0 || S <= 0 || Hq <= 0 || Hkv <= 0 || D <= 0) return USP_EINVAL;
  if (dtype != USP_BF16 && dtype != USP_FP16) return USP_EINVAL;
  if (stride != 4 && stride != 8 && stride != 16) return USP_EINVAL;
  if (q_stride_b < 0 || q_stride_s < 0 || q_stride_h < 0 || k_stride_b < 0 || k_stride_s < 0 || k_stride_h < 0) return USP_EINVAL;
  if (out_stride_b < 0 || out_stride_h < 0 || out_stride_row < 0) return USP_EINVAL;
  if (!(scale == scale)) return USP_EINVAL;
  if (D != 32 && D != 64 && D != 128) return USP_EUNSUPPORTED;
  if (Hq % Hkv != 0) return USP_EUNSUPPORTED;
  if (!tensor_aligned(q, q_stride_b, q_stride_s, q_stride_h, 16, 8) || !tensor_aligned(k, k_stride_b, k_stride_s, k_stride_h, 16, 8))
    return USP_EUNSUPPORTED;
  if (!aligned(out, 4)) return USP_EUNSUPPORTED;
  // 32-bit arithmetic of the kernel: sub-row indices, a stage's per-lane byte offsets (512 rows of k), the item count
  // ... and the range check that zeroes the k rows past S counts bytes from the stage's first row: rows must not overlap
  if (S >= (1 << 29) || k_stride_s >= (1 << 21) || (S > 1 && k_stride_s < D)) return USP_EUNSUPPORTED;
  BlockAntidiagArgs a;
  a.q = (const char*)q; a.k = (const char*)k; a.out = out;
  a.q_sb = q_stride_b; a.q_ss = q_stride_s; a.q_sh = q_stride_h;
  a.k_sb = k_stride_b; a.k_ss = k_stride_s; a.k_sh = k_stride_h;
  a.o_sb = out_stride_b; a.o_sh = out_stride_h; a.o_sr = out_stride_row;
  a.S = S; a.Hkv = Hkv; a.G = Hq / Hkv; a.nb = (S + USP_BLOCK_MASK_SIZE - 1) / USP_BLOCK_MASK_SIZE;
  a.hw = a.G >= 3 ? 4 : a.G;
  a.n_hc = (a.G + a.hw - 1) / a.hw;
  const int n_sub = (S + stride - 1) / stride, n_ct = (n_sub + kAdTile - 1) / kAdTile, rtw = kAdWaves / a.hw;
  a.n_rg = (n_ct + rtw - 1) / rtw;
  const int64_t items = (int64_t)B * Hkv * a.n_hc * a.n_rg;
  if (items >= (1LL << 31)) return USP_EUNSUPPORTED;
  a.n_items = (int)items;
  a.causal = causal ? 1 : 0;
  a.c = (scale / (float)stride) * kLog2e;
  hipStream_t st = (hipStream_t)stream;
  return with_head_dim_dtype(D, dtype, [&](auto d, auto dt) -> int {
    constexpr int Dv = decltype(d)::value, DTv = decltype(dt)::value;
    return stride == 4 ? launch_block_antidiag<Dv, DTv, 4>(a, st)
         : stride == 8 ? launch_block_antidiag<Dv, DTv, 8>(a, st)
                       : launch_block_antidiag<Dv, DTv, 16>(a, st);
  });
}
