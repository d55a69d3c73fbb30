// Block attention mass: the block-pooled attention map of a call (C ABI: usp_block_attn_mass; include/usp_hip.h states the
// function and the order of every sum).  For every (b, query head h, 128-row block I, 128-key block J) the attention probability
// that the rows of I give to the keys of J, from q, k and the call's own lse -- the quantity every block gate of this package
// approximates.  The forward's K Q^T tile walk with no V, no O accumulator and no running maximum: the lse is known.
//   block_mass_kernel  one work item per (b, h, I): 4 waves x 32 rows, the block-sparse forward's item.  Q lives in registers (B
//                      operand of S^T = K Q^T on v_mfma_f32_32x32x16), K goes through a double-buffered LDS ring of 64-key tiles
//                      filled by LDS-DMA with the forward's slot swizzle, one barrier a tile.  Per score
//                      p = exp2(fma(s, scale * log2e, -lse_i * log2e)); only tiles cut by the diagonal or the ragged end take the
//                      masked path, where a hidden key's p is set to 0.  Persistent workgroups walk the items, under causal the
//                      heavy (late) row blocks first (ItemWalk).  No atomics, ordinary vector stores, nothing read on the host.
// ORDER of the sum of one (I, J) -- a function of the position inside the 128 x 128 block alone:
//   1. lane (row i = 32 wave + (lane & 31), half hf = lane >> 5) adds, ascending from 0.f, the p of its keys: tile 2J then tile
//      2J + 1, in a tile the keys kt0 + 4 hf + (r & 3) + 8 (r >> 2) for r = 0 .. 15, then the same + 32 for r = 0 .. 15 (64 terms;
//      a hidden key, a row past Sq, a row with lse = -inf and a tile the item does not reach enter as +0, which changes no bit);
//   2. the row's two halves: x(hf = 0) + x(hf = 1);
//   3. the 32 rows of a wave by the butterfly x += x[lane ^ 16], ^ 8, ^ 4, ^ 2, ^ 1 (fp32 addition commutes: every lane holds the
//      same bits afterwards);
//   4. the four waves ((w0 + w1) + w2) + w3;
//   5. one division by rows(I).
// So the result repeats from call to call and does not depend on the grid, B or H, and a launch on a slice of rows against a
// slice of keys with the matching `diag` gives the bits of the whole call's sub-matrix.
#include "usp_host.hpp"
#include "usp_fwd_params.hpp"

namespace usp {

constexpr int kMassWaves = 4;
constexpr int kMassRows = 32 * kMassWaves;       // = USP_BLOCK_MASK_SIZE

struct BlockMassArgs {
  const char* q; const char* k;
  const float* lse;
  float* out;
  int64_t q_sb, q_ss, q_sh;                      // element strides of batch, row, head
  int64_t k_sb, k_ss, k_sh;
  int64_t lse_sb, lse_sh;
  int64_t o_sb, o_sh, o_sr;                      // element strides of batch, head, row block
  int Sq, Sk, Hkv, G, nbq, nbk, n_items;
  int diag;                                      // causal: row i sees key j iff j <= i + diag
  float scale_log2;                              // scale * log2(e), one fp32 product
};

template <int D, int DT, bool CAUSAL>
__global__ __launch_bounds__(64 * kMassWaves) void block_mass_kernel(const BlockMassArgs a) {
  using E = Elem<DT>;
  constexpr int NW = kMassWaves;
  constexpr int ROWB = D * 2;                    // bytes per K row
  constexpr int KBYTES = kBN * ROWB;             // one K tile
  constexpr int NKT = D / 16;                    // k-steps of K Q^T
  constexpr int CHUNKS = KBYTES / 1024;          // 1 KiB pieces per tile
  constexpr int CPW = (CHUNKS + NW - 1) / NW;    // pieces per wave per tile
  // LDS: Kbuf[0], Kbuf[1], then 2 x 4 wave sums
  extern __shared__ __attribute__((aligned(16))) char smem_raw[];
  USP_LDS char* smem = (USP_LDS char*)smem_raw;
  USP_LDS float* const slots = (USP_LDS float*)(smem + 2 * KBYTES);

  const int tid = threadIdx.x;
  const int lane = tid & 63;
  const int wave = __builtin_amdgcn_readfirstlane(tid >> 6);
  const int l31 = lane & 31;
  const int hi = lane >> 5;

  const ItemWalk walk(a.n_items);
  for (int pass = 0;; ++pass) {
    int w = walk.at(pass);
    if (w < 0) break;
    w = walk.dealt(w, a.nbq);
    const int I_r = w % a.nbq;
    int rest = w / a.nbq;
    const int I = CAUSAL ? (a.nbq - 1 - I_r) : I_r;          // heavy (late) row blocks first
    const int g = rest % a.G;
    rest /= a.G;
    const int hkv = rest % a.Hkv;
    const int b = rest / a.Hkv;
    const int h = hkv * a.G + g;

    const int q0 = I * kMassRows;
    const int qw = q0 + wave * 32;
    const int row = qw + l31;
    const int row_c = row < a.Sq ? row : a.Sq - 1;
    const int off = a.diag;
    const int n_rows = a.Sq - q0 < kMassRows ? a.Sq - q0 : kMassRows;   // rows(I) >= 1

    // ---- key range of the item and of this wave (usp_tile_range.h) ----
    const int blk_kv_end = usp_rows_key_end(q0, kMassRows, a.Sq, a.Sk, CAUSAL ? 1 : 0, off);
    const int wave_kv_end = qw < a.Sq ? usp_rows_key_end(qw, 32, a.Sq, a.Sk, CAUSAL ? 1 : 0, off) : 0;
    const int nt = usp_tiles_holding(blk_kv_end, kBN);
    const int nblk = (nt + 1) >> 1;                           // key blocks the item reaches; the others are written as 0

    // ---- Q fragments (B operand: lane holds Q[row][16t + 8hi .. +7]) and the row's exponent offset ----
    u32x4 qf[NKT];
    {
      const char* qp = a.q + 2 * (b * a.q_sb + (int64_t)row_c * a.q_ss + h * a.q_sh) + 16 * hi;
#pragma unroll
      for (int t = 0; t < NKT; ++t) qf[t] = *(const u32x4*)(qp + 32 * t);
    }
    // -lse * log2(e); a row past Sq or with lse = -inf gets -inf: fma(s, c, -inf) = -inf and exp2 gives +0
    float nl;
    {
      const float l = a.lse[b * a.lse_sb + h * a.lse_sh + row_c];
      nl = (row < a.Sq && l != USP_NEG_INF) ? -(l * kLog2e) : USP_NEG_INF;
    }
    const float c = a.scale_log2;

    // ---- K staging: LDS-DMA, the forward's layout (row-major tile, 16-byte slots swizzled on the source side) ----
    const char* kbase = a.k + 2 * (b * a.k_sb + hkv * a.k_sh);
    int k_voff[CPW];
#pragma unroll
    for (int i = 0; i < CPW; ++i) {
      const int cidx = wave + NW * i;
      const int r = cidx * (1024 / ROWB) + lane / (D / 8);
      const int c8 = (lane % (D / 8)) ^ KSwz<D>::of(r);
      k_voff[i] = r * (int)a.k_ss * 2 + c8 * 16;
    }
    auto dma_k = [&](int tile, int buf) {
      // the tile offset lives in the 64-bit descriptor base; num_records makes rows >= Sk read as 0 (they are masked)
      const int64_t toff = (int64_t)tile * kBN * a.k_ss * 2;
      int64_t rem = ((int64_t)(a.Sk - 1 - tile * kBN) * a.k_ss + D) * 2;
      rem = rem < 0 ? 0 : (rem > 0xffffffffLL ? 0xffffffffLL : rem);
      const auto rs_ = __builtin_amdgcn_make_buffer_rsrc((void*)(kbase + toff), 0, (int)(uint32_t)rem, 0x00020000);
#pragma unroll
      for (int i = 0; i < CPW; ++i)
        if (CHUNKS % NW == 0 || wave + NW * i < CHUNKS)
          lds_dma16(rs_, smem + buf * KBYTES + (wave + NW * i) * 1024, k_voff[i]);
    };
    const int k_rd_row = l31 * ROWB;
    const int k_rd_x = hi ^ KSwz<D>::of(l31);
    // S^T = K Q^T of the tile in Kbuf[kbuf]: one MFMA chain over D per score
    auto qk = [&](int kbuf, f32x16& s0, f32x16& s1) {
      USP_LDS const char* kb = smem + kbuf * KBYTES;
#pragma unroll
      for (int r = 0; r < 16; ++r) { s0[r] = 0.f; s1[r] = 0.f; }
#pragma unroll
      for (int kt = 0; kt < NKT; ++kt) {
        const int slot = ((2 * kt) ^ k_rd_x) * 16;
        const u32x4 ka = *(USP_LDS const u32x4*)(kb + k_rd_row + slot);
        const u32x4 kc = *(USP_LDS const u32x4*)(kb + 32 * ROWB + k_rd_row + slot);
        s0 = E::mfma(ka, qf[kt], s0);
        s1 = E::mfma(kc, qf[kt], s1);
      }
    };

    // blocks the item does not reach (above the diagonal): written as 0
    {
      float* const orow = a.out + b * a.o_sb + h * a.o_sh + I * a.o_sr;
      for (int J = nblk + tid; J < a.nbk; J += 64 * NW) orow[J] = 0.f;
    }

    if (nt > 0) dma_k(0, 0);
    dma_drain();
    __syncthreads();

    float acc = 0.f;                                          // step 1 of the order: this lane's keys of block J
    for (int t = 0; t < nt; ++t) {
      const int kt0 = t * kBN;
      if (t + 1 < nt) dma_k(t + 1, (t + 1) & 1);              // Kbuf[(t+1)&1] held K(t-1): last read in front of the previous barrier
      if (kt0 < wave_kv_end) {                                // (otherwise every p of this wave is +0)
        f32x16 s0, s1;
        qk(t & 1, s0, s1);
#pragma unroll
        for (int r = 0; r < 16; ++r) {
          s0[r] = fast_exp2(__builtin_fmaf(s0[r], c, nl));
          s1[r] = fast_exp2(__builtin_fmaf(s1[r], c, nl));
        }
        if (usp_key_tile_masked(kt0, kBN, qw, 32, a.Sk, CAUSAL ? 1 : 0, off, 0, 0)) {
          int klim = a.Sk - 1;
          if (CAUSAL) klim = row + off < klim ? row + off : klim;
          const int kb0 = kt0 + 4 * hi;
#pragma unroll
          for (int r = 0; r < 16; ++r) {
            const int key = kb0 + (r & 3) + 8 * (r >> 2);
            if (key > klim) s0[r] = 0.f;
            if (key + 32 > klim) s1[r] = 0.f;
          }
        }
#pragma unroll
        for (int r = 0; r < 16; ++r) acc += s0[r];
#pragma unroll
        for (int r = 0; r < 16; ++r) acc += s1[r];
      }
      const bool block_done = (t & 1) || t + 1 == nt;
      const int J = t >> 1;
      if (block_done) {
        float x = xhalf_sum(acc);                             // step 2
#pragma unroll
        for (int m = 16; m >= 1; m >>= 1) x += __shfl_xor(x, m, 64);    // step 3
        if (lane == 0) slots[4 * (J & 1) + wave] = x;
        acc = 0.f;
      }
      dma_drain();                 // this wave's pieces of K(t+1) have landed ...
      __syncthreads();             // ... and so have everybody else's; the wave sums of block J are visible
      // The set J & 1 is written again at the end of block J + 2, behind a later barrier than the one this thread meets next.
      if (block_done && tid == 0) {
        USP_LDS const float* const ws = slots + 4 * (J & 1);
        const float sum = ((ws[0] + ws[1]) + ws[2]) + ws[3];  // step 4
        a.out[b * a.o_sb + h * a.o_sh + I * a.o_sr + J] = sum / (float)n_rows;   // step 5
      }
    }
  }  // next item
}

template <int D, int DT, bool CAUSAL> int launch_block_mass(const BlockMassArgs& a, hipStream_t st) {
  // persistent launch, the block-sparse forward's shape: 4 waves, two workgroups per CU
  const int grid = persistent_grid(a.n_items, device_cus() * 2, 0);
  const size_t lds = 2 * kBN * D * 2 + 32;
  hipLaunchKernelGGL((block_mass_kernel<D, DT, CAUSAL>), dim3(grid), dim3(64 * kMassWaves), lds, st, a);
  return launched();
}

}  // namespace usp

extern "C" int usp_block_attn_mass(const void* q, const void* k, const float* lse, int32_t dtype, int32_t B, int32_t Sq, int32_t Sk,
                                   int32_t Hq, int32_t Hkv, int32_t D, int64_t q_stride_b, int64_t q_stride_s, int64_t q_stride_h,
                                   int64_t k_stride_b, int64_t k_stride_s, int64_t k_stride_h, int64_t lse_stride_b,
                                   int64_t lse_stride_h, float scale, int32_t causal, int32_t diag, float* out, int64_t out_stride_b,
                                   int64_t out_stride_h, int64_t out_stride_row, void* stream) {
  using namespace usp;
  if (!q || !k || !lse || !out || B <= 0 || Sq <= 0 || Sk <= 0 || Hq <= 0 || Hkv <= 0 || D <= 0) return USP_EINVAL;
  if (dtype != USP_BF16 && dtype != USP_FP16) return USP_EINVAL;
  if (q_stride_b < 0 || q_stride_s < 0 || q_stride_h < 0 || k_stride_b < 0 || k_stride_s < 0 || k_stride_h < 0) return USP_EINVAL;
  if (lse_stride_b < 0 || lse_stride_h < 0 || out_stride_b < 0 || out_stride_h < 0 || out_stride_row < 0) return USP_EINVAL;
  if (!(scale == scale)) return USP_EINVAL;
  if (D != 32 && D != 64 && D != 128) return USP_EUNSUPPORTED;
  if (Hq % Hkv != 0) return USP_EUNSUPPORTED;
  if (!tensor_aligned(q, q_stride_b, q_stride_s, q_stride_h, 16, 8) || !tensor_aligned(k, k_stride_b, k_stride_s, k_stride_h, 16, 8))
    return USP_EUNSUPPORTED;
  if (!aligned(lse, 4) || !aligned(out, 4)) return USP_EUNSUPPORTED;
  // 32-bit arithmetic of the kernel: row + diag, a tile's per-lane byte offsets, the item count
  if (Sq >= (1 << 29) || Sk >= (1 << 29) || diag >= (1 << 29) || diag <= -(1 << 29)) return USP_EUNSUPPORTED;
  if (!dma_rows_ok(k_stride_s, false)) return USP_EUNSUPPORTED;
  const int nbq = (Sq + kMassRows - 1) / kMassRows, nbk = (Sk + kMassRows - 1) / kMassRows;
  const int64_t items = (int64_t)B * Hq * nbq;
  if (items >= (1LL << 31)) return USP_EUNSUPPORTED;
  BlockMassArgs a;
  a.q = (const char*)q; a.k = (const char*)k; a.lse = lse; a.out = out;
  a.q_sb = q_stride_b; a.q_ss = q_stride_s; a.q_sh = q_stride_h;
  a.k_sb = k_stride_b; a.k_ss = k_stride_s; a.k_sh = k_stride_h;
  a.lse_sb = lse_stride_b; a.lse_sh = lse_stride_h;
  a.o_sb = out_stride_b; a.o_sh = out_stride_h; a.o_sr = out_stride_row;
  a.Sq = Sq; a.Sk = Sk; a.Hkv = Hkv; a.G = Hq / Hkv; a.nbq = nbq; a.nbk = nbk; a.n_items = (int)items;
  a.diag = diag;
  a.scale_log2 = scale * kLog2e;
  hipStream_t st = (hipStream_t)stream;
  return with_head_dim_dtype(D, dtype, [&](auto d, auto dt) -> int {
    return causal ? launch_block_mass<decltype(d)::value, decltype(dt)::value, true>(a, st)
                  : launch_block_mass<decltype(d)::value, decltype(dt)::value, false>(a, st);
  });
}
