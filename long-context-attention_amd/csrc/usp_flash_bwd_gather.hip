// Gathered-key sparse backward for gfx950 (include/usp_hip.h: USP_ATTN_KEY_INDEX_BWD): dQ, dK and dV of the forward of
// usp_flash_fwd_gather.hip.  A row's visible keys are two disjoint sets.  The BAND (window_left below the diagonal) is the existing
// windowed causal backward on the forward's lse and delta, launched first through usp_flash_bwd into fp32 tensors; the LISTED part
// -- entry e of the list of (b, h) with e < d_i - left, without a window e <= d_i: the forward's "gathered" compare -- is the three
// kernels below, which ADD to what the band left (order of every sum: band first, then the listed part).
//   flash_bwd_gather_dq_kernel    row-stationary.  The forward's item and walk: (batch, head, 128-row tile), 4 waves x 32 rows, late tiles
//                                 first, persistent; phase G of the forward alone (index ring, LDS-DMA gather of K and V tiles with a
//                                 per-lane offset, double-buffered).  Per tile S^T = K Q^T, p from the row's lse, dP^T = V dO^T (V by
//                                 rows: the same image), dS^T, dQ^T += K^T dS^T (K by the transposed read).  Q and dO fragments and
//                                 dQ^T are register resident: 64 + 32 + 32 registers at D = 128, one wave per SIMD.
//   flash_bwd_gather_dkdv_kernel  key-stationary, per QUERY head: an item is (batch, query head, 64-entry tile of its list); wave w owns
//                                 entries 32 (w & 1) .. + 31 and rows 32 (w >> 1) .. + 31 of every streamed 64-row tile.  The K and V
//                                 rows of a wave's entries are gathered ONCE, from memory into B-operand fragments (range-checked,
//                                 absent: zeros).  Q / dO tiles with lse and delta stream through double-buffered LDS from the first
//                                 row that sees the tile's smallest in-range entry to Sq:  S = Q K^T, dP = dO V^T, p, dS, then
//                                 dV^T += dO^T P and dK^T += Q^T dS with the transposed read.  The two row halves are summed through
//                                 LDS in a fixed order (rows 0-31 of every tile, then rows 32-63) and leave as fp32 partials
//                                 dk_list / dv_list (B, Hq, n_pad, D) with vector stores.  One workgroup per item, low tiles (most
//                                 rows) first.  No atomics; the sums do not depend on the grid.
//   gather_scatter_kernel         per (batch, KV head, key j): band value (or 0), then for the group's query heads in ascending order a
//                                 binary search of the head's list for j and, on a hit, that head's partial row.  Writes EVERY row of
//                                 dk / dv, fp32 or 16 bits rounded once.
// Every entry is range-checked where it is read and every search position lies in [0, n_idx): a list that breaks the contract gives
// wrong numbers, never an access outside the operands or the workspace.
#include "usp_host.hpp"
#include "usp_mfma64.hpp"
#include "usp_gather_bwd.hpp"

namespace usp {

// rows a lane's accumulator registers 4 g4 .. + 3 hold: gather::acc_m(4 g4 + x, hi) = 8 g4 + 4 hi + x
constexpr int kAbsent = 0x7fffffff;

template <int D, int DT>
__global__ __launch_bounds__(256, 1) void flash_bwd_gather_dq_kernel(const BwdArgsGather p) {
  using E = Elem<DT>;
  using namespace gather;
  using I = Img<D>;
  constexpr int kBM = 128;
  extern __shared__ __attribute__((aligned(16))) char smem_raw[];
  USP_LDS char* smem = (USP_LDS char*)smem_raw;            // Kbuf[0], Kbuf[1], Vbuf[0], Vbuf[1], index ring
  USP_LDS int* ring = (USP_LDS int*)(smem + 4 * I::kTileB);

  const int tid = threadIdx.x;
  const int lane = tid & 63;
  const int wave = __builtin_amdgcn_readfirstlane(tid >> 6);
  const int l31 = lane & 31, hi = lane >> 5;
  LaneBase<D> lb(lane);
  const float c = p.scale_log2;
  const int off = p.causal_off;
  const int k_rowb = (int)p.k_ss * 2, v_rowb = (int)p.v_ss * 2;
  const int n_lt = (p.n_idx + kRows - 1) / kRows;

  const ItemWalk walk(p.n_items);
  for (int pass = 0;; ++pass) {
    int w = walk.at(pass);
    if (w < 0) break;
    w = walk.grouped(walk.dealt(w, p.nq), p.nq, p.walk_g);
    const int qt = p.nq - 1 - w % p.nq;
    int rest = w / p.nq;
    const int g = rest % p.G;
    rest /= p.G;
    const int hkv = rest % p.Hkv;
    const int b = rest / p.Hkv;
    const int h = hkv * p.G + g;
    const int q0 = qt * kBM, qw = q0 + 32 * wave;
    const int* list = p.kidx + b * p.kidx_sb + h * p.kidx_sh;

    // the list tiles whose first entry lies at or below the item's last diagonal position (the forward's phase G)
    const int d_hi = (q0 + kBM < p.Sq ? q0 + kBM : p.Sq) - 1 + off;
    int nt = 0;
    for (int t0 = 0; t0 < n_lt; t0 += 256) {               // (every thread: the count is a barrier)
      const int t = t0 + tid;
      nt += __syncthreads_count(d_hi >= 0 && t < n_lt && list[t * kRows] <= d_hi);
    }
    const int wd_hi = (qw + 32 < p.Sq ? qw + 32 : p.Sq) - 1 + off;
    const bool wave_on = qw < p.Sq && wd_hi >= 0;

    auto entry_of = [&](int t) -> int {
      const int pos = t * kRows + lane;
      return pos < p.n_idx ? list[pos] : kAbsent;
    };
    const auto k_rs = __builtin_amdgcn_make_buffer_rsrc((void*)(p.k + 2 * (b * p.k_sb + hkv * p.k_sh)), 0, p.k_bytes, 0x00020000);
    const auto v_rs = __builtin_amdgcn_make_buffer_rsrc((void*)(p.v + 2 * (b * p.v_sb + hkv * p.v_sh)), 0, p.v_bytes, 0x00020000);
    auto stage = [&](int t, int buf) {
      USP_LDS const int* ent = ring + (t & (kRing - 1)) * kRows;
#pragma unroll
      for (int i = 0; i < I::kNP; ++i) {
        const int rr = I::piece_row(wave, lane, i);
        const int e = ent[rr];
        const bool ok = (unsigned)e < (unsigned)p.Sk;      // checked as it is read: nothing else forms an address from it
        const int col = I::piece_col(lane, rr);
        const int dst = (16 * wave + I::kRPP * i) * I::kRowB;
        lds_dma16(k_rs, smem + buf * I::kTileB + dst, ok ? e * k_rowb + col : p.k_bytes);
        lds_dma16(v_rs, smem + (2 + buf) * I::kTileB + dst, ok ? e * v_rowb + col : p.v_bytes);
      }
    };

    // ---- Q and dO fragments (B operands: lane holds X[row][16 t + 8 hi .. + 7]), the row's lse and delta ----
    const int row = qw + l31;
    const bool valid = row < p.Sq;
    const int row_c = valid ? row : p.Sq - 1;
    u32x4 qf[I::kNT], dof[I::kNT];
    {
      const char* qp = p.q + 2 * (b * p.q_sb + (int64_t)row_c * p.q_ss + h * p.q_sh) + 16 * hi;
      const char* dp = p.dout + 2 * (b * p.do_sb + (int64_t)row_c * p.do_ss + h * p.do_sh) + 16 * hi;
#pragma unroll
      for (int t = 0; t < I::kNT; ++t) {
        qf[t] = *(const u32x4*)(qp + 32 * t);
        dof[t] = *(const u32x4*)(dp + 32 * t);
      }
    }
    const float lse = p.lse[b * p.lse_sb + h * p.lse_sh + row_c];
    const float nl = lse == USP_NEG_INF ? USP_NEG_INF : -lse * kLog2e;     // a row that saw nothing: p = exp2(-inf) = 0
    const float dl = p.delta[b * p.dl_sb + h * p.dl_sh + row_c];
    // the row takes entry e iff (unsigned)e < cnt
    const int d_i = row + off;
    const int edge = p.win_on ? d_i - p.left : d_i + 1;
    const unsigned cnt = valid && edge > 0 ? (unsigned)edge : 0u;

    f32x16 dq[I::kNDJ];
#pragma unroll
    for (int dj = 0; dj < I::kNDJ; ++dj)
#pragma unroll
      for (int r = 0; r < 16; ++r) dq[dj][r] = 0.f;

    if (nt > 0) {                              // (the previous item's last barrier stands behind its last LDS read)
      if (wave == 0) {
        ring[lane] = entry_of(0);
        if (nt > 1) ring[kRows + lane] = entry_of(1);
      }
      __syncthreads();
      stage(0, 0);
      dma_drain();
      __syncthreads();
    }
    for (int j = 0; j < nt; ++j) {
      if (j + 1 < nt) stage(j + 1, (j + 1) & 1);
      int e_ahead = 0;
      if (wave == 0 && j + 2 < nt) e_ahead = entry_of(j + 2);
      USP_LDS const int* ent = ring + (j & (kRing - 1)) * kRows;
      const int e_first = __builtin_amdgcn_readfirstlane(ent[0]);
      if (wave_on && e_first <= wd_hi) {
        lb.keep_opaque();
        USP_LDS const char* kt = smem + (j & 1) * I::kTileB;
        USP_LDS const char* vt = smem + (2 + (j & 1)) * I::kTileB;
        f32x16 s[2], dp[2];
#pragma unroll
        for (int kb = 0; kb < 2; ++kb)
#pragma unroll
          for (int r = 0; r < 16; ++r) { s[kb][r] = 0.f; dp[kb][r] = 0.f; }
#pragma unroll
        for (int t = 0; t < I::kNT; ++t)
#pragma unroll
          for (int kb = 0; kb < 2; ++kb) s[kb] = E::mfma(lb.read_rows(kt, kb, t), qf[t], s[kb]);       // S^T = K Q^T
#pragma unroll
        for (int t = 0; t < I::kNT; ++t)
#pragma unroll
          for (int kb = 0; kb < 2; ++kb) dp[kb] = E::mfma(lb.read_rows(vt, kb, t), dof[t], dp[kb]);    // dP^T = V dO^T
        u32x4 dsf[2][2];                                    // packed dS^T [key block][k-step]: the B operand as it stands
#pragma unroll
        for (int kb = 0; kb < 2; ++kb)
#pragma unroll
          for (int g4 = 0; g4 < 4; ++g4) {
            const u32x4 e4 = *(USP_LDS const u32x4*)(ent + 32 * kb + 8 * g4 + 4 * hi);      // columns acc_m(4 g4 .. + 3, hi)
            float ds[4];
#pragma unroll
            for (int x = 0; x < 4; ++x) {
              const int r = 4 * g4 + x;
              const float pr = fast_exp2(__builtin_fmaf(s[kb][r], c, nl));
              ds[x] = e4[x] < cnt ? pr * (dp[kb][r] - dl) : 0.f;
            }
            dsf[kb][g4 >> 1][2 * (g4 & 1)] = E::pack2(ds[0], ds[1]);
            dsf[kb][g4 >> 1][2 * (g4 & 1) + 1] = E::pack2(ds[2], ds[3]);
          }
        // dQ^T += K^T dS^T: 4 k-steps x D / 32 dim blocks
#pragma unroll
        for (int kb = 0; kb < 2; ++kb)
#pragma unroll
          for (int ks = 0; ks < 2; ++ks)
#pragma unroll
            for (int dj = 0; dj < I::kNDJ; ++dj) dq[dj] = E::mfma(lb.read_tr(kt, 32 * kb + 16 * ks, dj), dsf[kb][ks], dq[dj]);
      }
      if (wave == 0 && j + 2 < nt) ring[((j + 2) & (kRing - 1)) * kRows + lane] = e_ahead;
      dma_drain();
      __syncthreads();
    }

    if (valid) {
      const GatherGrad& o = p.gq;
      float* f = o.f32 ? o.f32 + b * o.f_sb + (int64_t)row * o.f_ss + h * o.f_sh : nullptr;
      char* h16 = o.h16 ? o.h16 + 2 * (b * o.h_sb + (int64_t)row * o.h_ss + h * o.h_sh) : nullptr;
      store_row32_acc<E, I::kNDJ>(f, h16, dq, p.scale, hi, o.add);
    }
  }  // next item
}

template <int D, int DT>
__global__ __launch_bounds__(256, 1) void flash_bwd_gather_dkdv_kernel(const BwdArgsGather p) {
  using E = Elem<DT>;
  using namespace gather;
  using I = Img<D>;
  extern __shared__ __attribute__((aligned(16))) char smem_raw[];
  USP_LDS char* smem = (USP_LDS char*)smem_raw;            // Qbuf[0], Qbuf[1], dObuf[0], dObuf[1], row statistics [2][2][64]
  USP_LDS float* stat = (USP_LDS float*)(smem + 4 * I::kTileB);

  const int tid = threadIdx.x;
  const int lane = tid & 63;
  const int wave = __builtin_amdgcn_readfirstlane(tid >> 6);
  const int l31 = lane & 31, hi = lane >> 5;
  const int kb = wave & 1, rb = wave >> 1;
  LaneBase<D> lb(lane);
  const float c = p.scale_log2;
  const int off = p.causal_off;

  // item: tile-major, so that the low tiles of every list (the most rows) are dispatched first
  const int bh_n = p.B * p.Hq;
  const int t = blockIdx.x / bh_n, bh = blockIdx.x % bh_n;
  const int b = bh / p.Hq, h = bh % p.Hq, hkv = h / p.G;
  const int* list = p.kidx + b * p.kidx_sb + h * p.kidx_sh;

  // ---- this lane's entry (column l31 of the wave's 32), its K and V fragments: gathered once ----
  int e;
  {
    const int pos = t * kRows + 32 * kb + l31;
    e = pos < p.n_idx ? list[pos] : kAbsent;
    if (!((unsigned)e < (unsigned)p.Sk)) e = kAbsent;       // checked as it is read; kAbsent is below no row's count
  }
  u32x4 kf[I::kNT], vf[I::kNT];
  {
    const int e_c = e == kAbsent ? 0 : e;
    const char* kp = p.k + 2 * (b * p.k_sb + (int64_t)e_c * p.k_ss + hkv * p.k_sh) + 16 * hi;
    const char* vp = p.v + 2 * (b * p.v_sb + (int64_t)e_c * p.v_ss + hkv * p.v_sh) + 16 * hi;
#pragma unroll
    for (int x = 0; x < I::kNT; ++x) {
      kf[x] = e == kAbsent ? u32x4{0, 0, 0, 0} : *(const u32x4*)(kp + 32 * x);
      vf[x] = e == kAbsent ? u32x4{0, 0, 0, 0} : *(const u32x4*)(vp + 32 * x);
    }
  }
  // ---- the rows to stream: from the first row that takes the tile's smallest in-range entry ----
  int e_min;
  {
    const int pos = t * kRows + lane;
    e_min = pos < p.n_idx ? list[pos] : kAbsent;
    if (!((unsigned)e_min < (unsigned)p.Sk)) e_min = kAbsent;
#pragma unroll
    for (int m = 32; m >= 1; m >>= 1) {
      const int o = __shfl_xor(e_min, m);
      e_min = o < e_min ? o : e_min;
    }
    e_min = __builtin_amdgcn_readfirstlane(e_min);
  }
  int jt0 = 0, nt = 0;
  if (e_min != kAbsent) {
    int first = (p.win_on ? e_min + p.left + 1 : e_min) - off;      // e < d_i - left  |  e <= d_i
    first = first > 0 ? first : 0;
    if (first < p.Sq) {
      jt0 = first / kRows;
      nt = (p.Sq + kRows - 1) / kRows - jt0;
    }
  }

  const int q_rowb = (int)p.q_ss * 2, do_rowb = (int)p.do_ss * 2;
  const auto q_rs = __builtin_amdgcn_make_buffer_rsrc((void*)(p.q + 2 * (b * p.q_sb + h * p.q_sh)), 0, p.q_bytes, 0x00020000);
  const auto do_rs = __builtin_amdgcn_make_buffer_rsrc((void*)(p.dout + 2 * (b * p.do_sb + h * p.do_sh)), 0, p.do_bytes, 0x00020000);
  const float* lse_h = p.lse + b * p.lse_sb + h * p.lse_sh;
  const float* dl_h = p.delta + b * p.dl_sb + h * p.dl_sh;
  auto stage = [&](int j, int buf) {
    const int r0 = (jt0 + j) * kRows;
#pragma unroll
    for (int i = 0; i < I::kNP; ++i) {
      const int rr = I::piece_row(wave, lane, i);
      const bool ok = r0 + rr < p.Sq;                      // rows behind the end fetch zeros through the byte count
      const int col = I::piece_col(lane, rr);
      const int dst = (16 * wave + I::kRPP * i) * I::kRowB;
      lds_dma16(q_rs, smem + buf * I::kTileB + dst, ok ? (r0 + rr) * q_rowb + col : p.q_bytes);
      lds_dma16(do_rs, smem + (2 + buf) * I::kTileB + dst, ok ? (r0 + rr) * do_rowb + col : p.do_bytes);
    }
    if (tid < 128) {                                       // -lse log2(e) (-inf: a row that takes nothing) and delta of the tile's rows
      const int r = r0 + (tid & 63);
      float x;
      if (tid < 64) {
        const float l = r < p.Sq ? lse_h[r] : USP_NEG_INF;
        x = l == USP_NEG_INF ? USP_NEG_INF : -l * kLog2e;
      } else {
        x = r < p.Sq ? dl_h[r] : 0.f;
      }
      stat[buf * 128 + tid] = x;
    }
  };

  f32x16 dk[I::kNDJ], dv[I::kNDJ];
#pragma unroll
  for (int dj = 0; dj < I::kNDJ; ++dj)
#pragma unroll
    for (int r = 0; r < 16; ++r) { dk[dj][r] = 0.f; dv[dj][r] = 0.f; }

  if (nt > 0) {
    stage(0, 0);
    dma_drain();
    __syncthreads();
  }
  for (int j = 0; j < nt; ++j) {
    if (j + 1 < nt) stage(j + 1, (j + 1) & 1);             // buffers last read in iteration j - 1
    {
      lb.keep_opaque();
      USP_LDS const char* qt = smem + (j & 1) * I::kTileB;
      USP_LDS const char* dot = smem + (2 + (j & 1)) * I::kTileB;
      USP_LDS const float* st = stat + (j & 1) * 128;
      const int r0 = (jt0 + j) * kRows + 32 * rb;
      f32x16 s, dp;
#pragma unroll
      for (int r = 0; r < 16; ++r) { s[r] = 0.f; dp[r] = 0.f; }
#pragma unroll
      for (int x = 0; x < I::kNT; ++x) s = E::mfma(lb.read_rows(qt, rb, x), kf[x], s);         // S = Q K^T: rows x entries
#pragma unroll
      for (int x = 0; x < I::kNT; ++x) dp = E::mfma(lb.read_rows(dot, rb, x), vf[x], dp);      // dP = dO V^T
      u32x4 pf[2], dsf[2];                                  // packed P / dS [k-step over the rows]: B operands as they stand
#pragma unroll
      for (int g4 = 0; g4 < 4; ++g4) {
        const f32x4 nl4 = *(USP_LDS const f32x4*)(st + 32 * rb + 8 * g4 + 4 * hi);             // rows acc_m(4 g4 .. + 3, hi)
        const f32x4 dl4 = *(USP_LDS const f32x4*)(st + 64 + 32 * rb + 8 * g4 + 4 * hi);
        float pr[4], ds[4];
#pragma unroll
        for (int x = 0; x < 4; ++x) {
          const int r = 4 * g4 + x;
          const int row = r0 + 8 * g4 + 4 * hi + x;
          const int edge = p.win_on ? row + off - p.left : row + off + 1;
          const unsigned cnt = row < p.Sq && edge > 0 ? (unsigned)edge : 0u;
          const bool vis = (unsigned)e < cnt;
          const float pe = fast_exp2(__builtin_fmaf(s[r], c, nl4[x]));
          pr[x] = vis ? pe : 0.f;
          ds[x] = vis ? pe * (dp[r] - dl4[x]) : 0.f;
        }
        pf[g4 >> 1][2 * (g4 & 1)] = E::pack2(pr[0], pr[1]);
        pf[g4 >> 1][2 * (g4 & 1) + 1] = E::pack2(pr[2], pr[3]);
        dsf[g4 >> 1][2 * (g4 & 1)] = E::pack2(ds[0], ds[1]);
        dsf[g4 >> 1][2 * (g4 & 1) + 1] = E::pack2(ds[2], ds[3]);
      }
#pragma unroll
      for (int ks = 0; ks < 2; ++ks)
#pragma unroll
        for (int dj = 0; dj < I::kNDJ; ++dj) {
          dv[dj] = E::mfma(lb.read_tr(dot, 32 * rb + 16 * ks, dj), pf[ks], dv[dj]);            // dV^T += dO^T P
          dk[dj] = E::mfma(lb.read_tr(qt, 32 * rb + 16 * ks, dj), dsf[ks], dk[dj]);            // dK^T += Q^T dS
        }
    }
    dma_drain();
    __syncthreads();
  }

  // ---- the two row halves of an entry block, summed in a fixed order through LDS (the tile buffers are free: D / 32 x 16 KiB) ----
  USP_LDS float* xch = (USP_LDS float*)smem;
  if (rb == 1) {
#pragma unroll
    for (int dj = 0; dj < I::kNDJ; ++dj)
#pragma unroll
      for (int r = 0; r < 16; ++r) {
        xch[(((kb * 2 + 0) * I::kNDJ + dj) * 16 + r) * 64 + lane] = dk[dj][r];
        xch[(((kb * 2 + 1) * I::kNDJ + dj) * 16 + r) * 64 + lane] = dv[dj][r];
      }
  }
  __syncthreads();
  if (rb == 0) {
#pragma unroll
    for (int dj = 0; dj < I::kNDJ; ++dj)
#pragma unroll
      for (int r = 0; r < 16; ++r) {
        dk[dj][r] += xch[(((kb * 2 + 0) * I::kNDJ + dj) * 16 + r) * 64 + lane];
        dv[dj][r] += xch[(((kb * 2 + 1) * I::kNDJ + dj) * 16 + r) * 64 + lane];
      }
    const int64_t prow = ((int64_t)bh * p.n_pad + t * kRows + 32 * kb + l31) * D;      // < B Hq n_pad D: inside the partials
    store_row32_acc<E, I::kNDJ>(p.dk_list + prow, nullptr, dk, p.scale, hi, 0);
    store_row32_acc<E, I::kNDJ>(p.dv_list + prow, nullptr, dv, 1.f, hi, 0);
  }
}

// position of j in the sorted list, or -1; every probe lies in [0, n)
USP_DEV int list_find(const int* list, int n, int j) {
  int lo = 0, hi = n;
  while (lo < hi) {
    const int mid = (lo + hi) >> 1;
    if (list[mid] < j) lo = mid + 1; else hi = mid;
  }
  return lo < n && list[lo] == j ? lo : -1;
}

template <int DT>
__global__ __launch_bounds__(256) void gather_scatter_kernel(const BwdArgsGather p) {
  using E = Elem<DT>;
  const int d4n = p.D / 4;
  const int64_t total = (int64_t)p.B * p.Hkv * p.Sk * d4n;
  for (int64_t i = (int64_t)blockIdx.x * 256 + threadIdx.x; i < total; i += (int64_t)gridDim.x * 256) {
    const int d0 = 4 * (int)(i % d4n);
    int64_t rest = i / d4n;
    const int j = (int)(rest % p.Sk);
    rest /= p.Sk;
    const int hkv = (int)(rest % p.Hkv);
    const int b = (int)(rest / p.Hkv);
    f32x4 sk = {0.f, 0.f, 0.f, 0.f}, sv = {0.f, 0.f, 0.f, 0.f};
    if (p.gk.add) sk = *(const f32x4*)(p.gk.f32 + b * p.gk.f_sb + (int64_t)j * p.gk.f_ss + hkv * p.gk.f_sh + d0);
    if (p.gv.add) sv = *(const f32x4*)(p.gv.f32 + b * p.gv.f_sb + (int64_t)j * p.gv.f_ss + hkv * p.gv.f_sh + d0);
    for (int g = 0; g < p.G; ++g) {                        // ascending query heads: the order of the sum
      const int h = hkv * p.G + g;
      const int pos = list_find(p.kidx + b * p.kidx_sb + h * p.kidx_sh, p.n_idx, j);
      if (pos < 0) continue;
      const int64_t prow = (((int64_t)b * p.Hq + h) * p.n_pad + pos) * p.D + d0;
      sk += *(const f32x4*)(p.dk_list + prow);
      sv += *(const f32x4*)(p.dv_list + prow);
    }
    auto put = [&](const GatherGrad& o, const f32x4& v) {
      if (o.h16) *(u32x2*)(o.h16 + 2 * (b * o.h_sb + (int64_t)j * o.h_ss + hkv * o.h_sh + d0)) = u32x2{E::pack2(v[0], v[1]), E::pack2(v[2], v[3])};
      else *(f32x4*)(o.f32 + b * o.f_sb + (int64_t)j * o.f_ss + hkv * o.f_sh + d0) = v;
    };
    put(p.gk, sk);
    put(p.gv, sv);
  }
}

int launch_bwd_gather(const BwdArgsGather& p_in, int D, int dtype, int which, hipStream_t st) {
  BwdArgsGather p = p_in;
  p.nq = (p.Sq + 127) / 128;
  p.n_items = p.B * p.Hq * p.nq;
  const int n_lt = p.n_pad / gather::kRows;
  return with_dtype(dtype, [&](auto dt) -> int {
    constexpr int kDT = decltype(dt)::value;
    auto go = [&](auto d) -> int {
      constexpr int kD = decltype(d)::value;
      if (which & 2) {
        constexpr size_t lds = 4 * gather::Img<kD>::kTileB + 2 * 128 * 4;
        auto* kern = flash_bwd_gather_dkdv_kernel<kD, kDT>;
        if (hipFuncSetAttribute((const void*)kern, hipFuncAttributeMaxDynamicSharedMemorySize, (int)lds) != hipSuccess) {
          (void)hipGetLastError();
          return USP_ELAUNCH;
        }
        hipLaunchKernelGGL(kern, dim3(p.B * p.Hq * n_lt), dim3(256), lds, st, p);
        if (launched() != USP_OK) return USP_ELAUNCH;
        launch_kinds_note(USP_KIND_DKDV_GATHER);
        const int64_t groups = ((int64_t)p.B * p.Hkv * p.Sk * (kD / 4) + 255) / 256;
        hipLaunchKernelGGL((gather_scatter_kernel<kDT>), dim3((int)(groups > 4096 ? 4096 : groups)), dim3(256), 0, st, p);
        if (launched() != USP_OK) return USP_ELAUNCH;
      }
      if (which & 1) {
        constexpr size_t lds = 4 * gather::Img<kD>::kTileB + gather::kRing * gather::kRows * 4;
        auto* kern = flash_bwd_gather_dq_kernel<kD, kDT>;
        if (hipFuncSetAttribute((const void*)kern, hipFuncAttributeMaxDynamicSharedMemorySize, (int)lds) != hipSuccess) {
          (void)hipGetLastError();
          return USP_ELAUNCH;
        }
        const int grid = persistent_grid(p.n_items, device_cus(), p.interleave);        // one workgroup per CU
        hipLaunchKernelGGL(kern, dim3(grid), dim3(256), lds, st, p);
        if (launched() != USP_OK) return USP_ELAUNCH;
        launch_kinds_note(USP_KIND_DQ_GATHER);
      }
      return USP_OK;
    };
    return D == 128 ? go(Int<128>{}) : go(Int<64>{});
  });
}

// The caller's workspace: [dk_list | dv_list | band dq | band dk | band dv]; the lists only when the dK/dV launch runs, a band tensor
// only under a window where the caller takes that gradient in 16 bits (the band's fp32 result then has no other home).
struct GatherWs {
  int64_t list, dq, dk, dv;                       // bytes of one list tensor, of the three band tensors (0: not there)
  int64_t total() const { return 2 * list + dq + dk + dv; }
};
static GatherWs gather_ws(const usp_bwd_args& a, int32_t n_index) {
  GatherWs w{0, 0, 0, 0};
  const bool want_dq = !(a.flags & USP_BWD_SKIP_DQ), want_dkdv = !(a.flags & USP_BWD_SKIP_DKDV);
  const bool win = (a.flags & USP_ATTN_WINDOW) != 0;
  const int64_t n_pad = ((int64_t)n_index + 63) / 64 * 64;
  if (want_dkdv) w.list = (int64_t)a.B * a.Hq * n_pad * a.D * 4;
  if (win && want_dq && a.dq16.ptr) w.dq = (int64_t)a.B * a.Sq * a.Hq * a.D * 4;
  if (win && want_dkdv && a.dk16.ptr) w.dk = (int64_t)a.B * a.Sk * a.Hkv * a.D * 4;
  if (win && want_dkdv && a.dv16.ptr) w.dv = (int64_t)a.B * a.Sk * a.Hkv * a.D * 4;
  return w;
}

}  // namespace usp

extern "C" int64_t usp_flash_bwd_gather_workspace_bytes(const usp_bwd_args* a, int32_t n_index) {
  if (!a || n_index < 1 || a->B <= 0 || a->Sq <= 0 || a->Sk <= 0 || a->Hq <= 0 || a->Hkv <= 0 || a->D <= 0) return 0;
  return usp::gather_ws(*a, n_index).total();
}

// usp_flash_bwd_gather (include/usp_hip.h: USP_ATTN_KEY_INDEX_BWD): checked in the order of the header's table, nothing launched or
// written by a call that is declined.
extern "C" int usp_flash_bwd_gather(const usp_bwd_args* args, const int32_t* key_index, int64_t index_stride_b, int64_t index_stride_h,
                                    int32_t n_index, void* stream) {
  using namespace usp;
  launch_kinds_reset();
  if (!args || !args->lse || !args->delta) return USP_EINVAL;
  const usp_bwd_args& a = *args;
  if (!key_index || n_index < 1 || !aligned(key_index, 4) || index_stride_b < 0 || index_stride_h < 0) return USP_EINVAL;
  const int skip = a.flags & (USP_BWD_SKIP_DQ | USP_BWD_SKIP_DKDV);
  if (skip == (USP_BWD_SKIP_DQ | USP_BWD_SKIP_DKDV)) return USP_EINVAL;
  if (int rc = check_problem(a)) return rc;
  if (!a.causal || (a.D != 64 && a.D != 128)) return USP_EUNSUPPORTED;
  const bool has_win = (a.flags & USP_ATTN_WINDOW) != 0;
  if (has_win && a.window_right != 0) return USP_EUNSUPPORTED;
  if (a.flags & (USP_ATTN_SOFTCAP | USP_ATTN_SHIFT | USP_FORCE_ROW64 | USP_FORCE_WAVE32 | USP_DKDV_KEYS128 | USP_DKDV_KEYS256)) return USP_EUNSUPPORTED;
  if (a.seq_q || a.seq_k) return USP_EUNSUPPORTED;
  if (!a.dout.ptr || !a.q.ptr || !a.k.ptr || !a.v.ptr) return USP_EINVAL;
  const bool want_dq = !(skip & USP_BWD_SKIP_DQ), want_dkdv = !(skip & USP_BWD_SKIP_DKDV);
  if ((want_dq && !a.dq.ptr && !a.dq16.ptr) || (want_dkdv && ((!a.dk.ptr && !a.dk16.ptr) || (!a.dv.ptr && !a.dv16.ptr)))) return USP_EINVAL;
  // a 16-bit final output that is also accumulated from is the rings' case: not served here
  if ((want_dq && a.dq16.ptr && a.accum_dq) || (want_dkdv && ((a.dk16.ptr && a.accum_dk) || (a.dv16.ptr && a.accum_dv)))) return USP_EUNSUPPORTED;
  auto ok32 = [](const usp_tensor& t) { return !t.ptr || tensor_aligned(t, 16, 4); };
  auto ok16 = [](const usp_tensor& t) { return !t.ptr || tensor_aligned(t, 8, 4); };
  if (!tensor_aligned(a.dout, 16, 8) || !tensor_aligned(a.q, 16, 8) || !tensor_aligned(a.k, 16, 8) || !tensor_aligned(a.v, 16, 8) ||
      !ok32(a.dq) || !ok32(a.dk) || !ok32(a.dv) || !ok16(a.dq16) || !ok16(a.dk16) || !ok16(a.dv16))
    return USP_EUNSUPPORTED;
  // a lane's offset into a (batch, head) plane is 32-bit and an absent row's lies behind the plane: planes end below 2^31 bytes
  auto plane = [&](const usp_tensor& t, int S) { return t.stride_s < 0 ? (int64_t)-1 : ((int64_t)(S - 1) * t.stride_s + a.D) * 2; };
  const int64_t k_bytes = plane(a.k, a.Sk), v_bytes = plane(a.v, a.Sk), q_bytes = plane(a.q, a.Sq), do_bytes = plane(a.dout, a.Sq);
  for (int64_t n : {k_bytes, v_bytes, q_bytes, do_bytes})
    if (n < 0 || n >= (1LL << 31) - 16) return USP_EUNSUPPORTED;
  const GatherWs ws = gather_ws(a, n_index);
  if (ws.total() > 0 && (!a.workspace || !aligned(a.workspace, 16) || a.workspace_bytes < ws.total())) return USP_EINVAL;

  char* wsp = (char*)a.workspace;
  float* dk_list = (float*)wsp;
  float* dv_list = (float*)(wsp + ws.list);
  float* band[3] = {ws.dq ? (float*)(wsp + 2 * ws.list) : nullptr, ws.dk ? (float*)(wsp + 2 * ws.list + ws.dq) : nullptr,
                    ws.dv ? (float*)(wsp + 2 * ws.list + ws.dq + ws.dk) : nullptr};
  // one gradient: where the band writes its fp32 share (x32 / accum), and how the listed part finishes it
  auto plan = [&](const usp_tensor& t32, const usp_tensor& t16, int accum, float* ws32, int S, int H, usp_tensor* x32, int* x_accum) {
    GatherGrad o{};
    if (t16.ptr) {
      *x32 = usp_tensor{ws32, (int64_t)S * H * a.D, (int64_t)H * a.D, (int64_t)a.D};
      *x_accum = 0;
      o.f32 = ws32; o.f_sb = x32->stride_b; o.f_ss = x32->stride_s; o.f_sh = x32->stride_h;
      o.h16 = (char*)t16.ptr; o.h_sb = t16.stride_b; o.h_ss = t16.stride_s; o.h_sh = t16.stride_h;
      o.add = has_win ? 1 : 0;
    } else {
      *x32 = t32;
      *x_accum = accum ? 1 : 0;
      o.f32 = (float*)t32.ptr; o.f_sb = t32.stride_b; o.f_ss = t32.stride_s; o.f_sh = t32.stride_h;
      o.add = (has_win || accum) ? 1 : 0;
    }
    return o;
  };
  usp_bwd_args bd = a;                             // the band: the windowed causal backward on the same lse and delta, fp32, uncut
  bd.dq16 = bd.dk16 = bd.dv16 = usp_tensor{nullptr, 0, 0, 0};
  BwdArgsGather p{};
  p.gq = plan(a.dq, a.dq16, a.accum_dq, band[0], a.Sq, a.Hq, &bd.dq, &bd.accum_dq);
  p.gk = plan(a.dk, a.dk16, a.accum_dk, band[1], a.Sk, a.Hkv, &bd.dk, &bd.accum_dk);
  p.gv = plan(a.dv, a.dv16, a.accum_dv, band[2], a.Sk, a.Hkv, &bd.dv, &bd.accum_dv);
  if (has_win) {                                   // first: the listed part adds to what it leaves
    bd.flags = (a.flags & (USP_LAUNCH_INTERLEAVE | USP_BWD_SKIP_DQ | USP_BWD_SKIP_DKDV)) | USP_ATTN_WINDOW;
    bd.window_right = 0;
    bd.dq_splits = bd.dkdv_splits = 0; bd.dkdv_heads = 0;
    bd.workspace = nullptr; bd.workspace_bytes = 0;
    if (int rc = usp_flash_bwd(&bd, stream)) return rc;          // (notes its own kinds)
  }
  p.dout = (const char*)a.dout.ptr; p.q = (const char*)a.q.ptr; p.k = (const char*)a.k.ptr; p.v = (const char*)a.v.ptr;
  p.lse = a.lse; p.delta = a.delta;
  p.do_sb = a.dout.stride_b; p.do_ss = a.dout.stride_s; p.do_sh = a.dout.stride_h;
  p.q_sb = a.q.stride_b; p.q_ss = a.q.stride_s; p.q_sh = a.q.stride_h;
  p.k_sb = a.k.stride_b; p.k_ss = a.k.stride_s; p.k_sh = a.k.stride_h;
  p.v_sb = a.v.stride_b; p.v_ss = a.v.stride_s; p.v_sh = a.v.stride_h;
  p.lse_sb = a.lse_stride_b; p.lse_sh = a.lse_stride_h; p.dl_sb = a.delta_stride_b; p.dl_sh = a.delta_stride_h;
  p.dk_list = dk_list; p.dv_list = dv_list;
  p.n_pad = (n_index + 63) / 64 * 64;
  p.kidx = key_index; p.kidx_sb = index_stride_b; p.kidx_sh = index_stride_h; p.n_idx = n_index;
  p.B = a.B; p.Sq = a.Sq; p.Sk = a.Sk; p.Hq = a.Hq; p.Hkv = a.Hkv; p.G = a.Hq / a.Hkv; p.D = a.D;
  p.causal_off = a.Sk - a.Sq;
  p.scale = a.softmax_scale;
  p.scale_log2 = a.softmax_scale * kLog2e;
  p.win_on = has_win ? 1 : 0;
  p.left = !has_win ? 0 : (a.window_left < 0 || a.window_left > a.Sk ? a.Sk : a.window_left);    // (negative: no left bound)
  p.k_bytes = (int)k_bytes; p.v_bytes = (int)v_bytes; p.q_bytes = (int)q_bytes; p.do_bytes = (int)do_bytes;
  p.interleave = (a.flags & USP_LAUNCH_INTERLEAVE) ? 1 : 0;
  p.walk_g = p.G;
  return launch_bwd_gather(p, a.D, a.dtype, (want_dq ? 1 : 0) | (want_dkdv ? 2 : 0), (hipStream_t)stream);
}
