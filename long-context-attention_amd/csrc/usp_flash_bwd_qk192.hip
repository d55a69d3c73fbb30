// Flash-attention backward for gfx950 at HEAD DIMS (192, 128) -- q, k, dq, dk of 192 dims, v, dout, dv of 128 --, one wave per SIMD,
// 4 waves per workgroup: the dQ kernel (a wave owns 32 query rows, K and V stream through LDS) and the dK/dV kernel (a wave owns 32
// keys, Q and dO stream through LDS).  Entry usp_flash_bwd_vdim; numerics as the equal-dim kernels: P is rebuilt from the forward's
// LSE, dS = P (dP - delta), the scale is applied once in the epilogue.  Tile image and fill: usp_qk192.hpp; 64-row tiles of 24 KiB
// (K, Q) and 16 KiB (V, dO), double-buffered = 80 KiB, one barrier per tile.
//
// dQ, per wave:     dQ^T 192 x 32 fp32 = 96 registers; Q and dO fragments (B operands of S^T = K Q^T and dP^T = V dO^T) 48 + 32;
//                   S^T and dP^T of a 64-key tile 32 + 32; dS packed to 16 bits (16) is the B operand of dQ^T += K^T dS^T as it
//                   stands.  A tile: 24 + 16 + 24 = 64 MFMAs.
// dK/dV, per wave:  dK^T and dV^T 96 + 64 registers; K and V fragments (B operands of S = Q K^T and dP = dO V^T) 48 + 32: 240 of 512
//                   where D = 256 needs 384.  S and dP of one 32-row block 16 + 16 (a 64-row tile is two blocks in turn).  One wave
//                   does all four products for its keys, so P never crosses LDS.  A tile: 2 x (12 + 8 + 8 + 12) = 80 MFMAs.  An item
//                   is 128 keys of one KV head and loops over the WHOLE group of query heads: no per-head partials, no reduce
//                   launch, no workspace, no atomics -- deterministic.  The rows' -lse log2(e) and delta of a tile are staged
//                   beside it (two waves, one value per lane) since a lane's 16 score registers belong to 16 different rows.
// The MFMAs are the builtins: hipcc pads their hazards (tools/mfma_hazards.py).
#include "usp_bwd_params.hpp"
#include "usp_host.hpp"
#include "usp_mfma64.hpp"
#include "usp_qk192.hpp"

namespace usp {

// -lse log2(e) of a row, -inf for a row that saw no key (lse = -inf) or lies behind the last one: P = exp2(S c - inf) = 0
USP_DEV float neg_lse_log2_qk192(float lse, bool valid) { return (valid && lse != USP_NEG_INF) ? -lse * kLog2e : USP_NEG_INF; }

template <int DT, bool CAUSAL>
__global__ __launch_bounds__(256, 1) void flash_bwd_dq_qk192_kernel(const BwdParams p) {
  using E = Elem<DT>;
  using namespace qk192;
  constexpr int kBM = 128;
  constexpr int kVbuf = 2 * kQkTileB;         // LDS: Kbuf[0], Kbuf[1], Vbuf[0], Vbuf[1]
  extern __shared__ __attribute__((aligned(16))) char smem_raw[];
  USP_LDS char* smem = (USP_LDS char*)smem_raw;

  const int tid = threadIdx.x;
  const int lane = tid & 63;
  const int wave = __builtin_amdgcn_readfirstlane(tid >> 6);
  const int l31 = lane & 31, hi = lane >> 5;
  LaneBase lb(lane);
  const float c = p.scale_log2;
  int k_voff[6], v_voff[4];
  stage_offsets<3>(k_voff, wave, lane, (int)p.k_ss * 2);
  stage_offsets<2>(v_voff, wave, lane, (int)p.v_ss * 2);

  const ItemWalk walk(p.n_items);
  for (int pass = 0;; ++pass) {
    int w = walk.at(pass);
    if (w < 0) break;
    w = walk.grouped(walk.dealt(w, p.nblk), p.nblk, p.walk_g);
    const int qt_r = w % p.nblk;
    int rest = w / p.nblk;
    const int qt = CAUSAL ? (p.nblk - 1 - qt_r) : qt_r;     // heavy (late) tiles first
    const int g = rest % p.G;
    rest /= p.G;
    const int hkv = rest % p.Hkv;
    const int b = rest / p.Hkv;
    const int h = hkv * p.G + g;
    const int q0 = qt * kBM, qw = q0 + 32 * wave;
    const int off = p.causal_off;

    const usp_query_tiles tr = usp_query_tiles_of(q0, kBM, qw, 32, p.Sq, p.Sk, CAUSAL, off, kRows);
    const int nt = tr.nt, n_w = tr.n_w, n_full = tr.n_full;

    // ---- the wave's rows: Q and dO fragments (B operands), -lse log2(e) and delta of the lane's row ----
    const int row = qw + l31;
    const bool valid = row < p.Sq;
    const int row_c = valid ? row : p.Sq - 1;
    u32x4 qf[kNTqk], dof[kNTv];
    {
      const char* qp = p.q + 2 * (b * p.q_sb + (int64_t)row_c * p.q_ss + h * p.q_sh) + 16 * hi;
      const char* dp_ = p.dout + 2 * (b * p.do_sb + (int64_t)row_c * p.do_ss + h * p.do_sh) + 16 * hi;
#pragma unroll
      for (int t = 0; t < kNTqk; ++t) qf[t] = *(const u32x4*)(qp + 32 * t);
#pragma unroll
      for (int t = 0; t < kNTv; ++t) dof[t] = *(const u32x4*)(dp_ + 32 * t);
    }
    const float nl = neg_lse_log2_qk192(p.lse[b * p.lse_sb + h * p.lse_sh + row_c], valid);
    const float delta = p.delta[b * p.dl_sb + h * p.dl_sh + row_c];

    const char* kbase = p.k + 2 * (b * p.k_sb + hkv * p.k_sh);
    const char* vbase = p.v + 2 * (b * p.v_sb + hkv * p.v_sh);
    auto stage = [&](int tile, int buf) {
      stage_tile<3>(tile_rsrc<kDqk>(kbase, p.k_ss, tile * kRows, p.Sk), smem + buf * kQkTileB, wave, k_voff);
      stage_tile<2>(tile_rsrc<kDv>(vbase, p.v_ss, tile * kRows, p.Sk), smem + kVbuf + buf * kVTileB, wave, v_voff);
    };

    f32x16 dq[kNDJqk];
#pragma unroll
    for (int dj = 0; dj < kNDJqk; ++dj)
#pragma unroll
      for (int r = 0; r < 16; ++r) dq[dj][r] = 0.f;

    if (nt > 0) {
      stage(0, 0);
      dma_drain();
      __syncthreads();
    }
    for (int j = 0; j < nt; ++j) {
      if (j + 1 < nt) stage(j + 1, (j + 1) & 1);
      if (j < n_w) {
        lb.keep_opaque();
        USP_LDS const char* kt = smem + (j & 1) * kQkTileB;
        USP_LDS const char* vt = smem + kVbuf + (j & 1) * kVTileB;
        f32x16 s[2], dp[2];
#pragma unroll
        for (int kb = 0; kb < 2; ++kb)
#pragma unroll
          for (int r = 0; r < 16; ++r) { s[kb][r] = 0.f; dp[kb][r] = 0.f; }
#pragma unroll
        for (int t = 0; t < kNTqk; ++t)
#pragma unroll
          for (int kb = 0; kb < 2; ++kb) {
            s[kb] = E::mfma(read_rows(kt, lb, kb, t), qf[t], s[kb]);
            if (t < kNTv) dp[kb] = E::mfma(read_rows(vt, lb, kb, t), dof[t], dp[kb]);
          }
        if (j >= n_full) {
          int klim = p.Sk - 1;
          if (CAUSAL) klim = row + off < klim ? row + off : klim;
#pragma unroll
          for (int kb = 0; kb < 2; ++kb)
#pragma unroll
            for (int r = 0; r < 16; ++r)
              if (j * kRows + 32 * kb + acc_m(r, hi) > klim) s[kb][r] = USP_NEG_INF;
        }
        u32x4 dsf[2][2];                                    // packed dS^T [key block][k-step]
#pragma unroll
        for (int kb = 0; kb < 2; ++kb)
#pragma unroll
          for (int r = 0; r < 16; r += 2) {
            const float p0 = fast_exp2(__builtin_fmaf(s[kb][r], c, nl)), p1 = fast_exp2(__builtin_fmaf(s[kb][r + 1], c, nl));
            dsf[kb][r >> 3][(r & 7) >> 1] = E::pack2(p0 * (dp[kb][r] - delta), p1 * (dp[kb][r + 1] - delta));
          }
#pragma unroll
        for (int kb = 0; kb < 2; ++kb)
#pragma unroll
          for (int ks = 0; ks < 2; ++ks)
#pragma unroll
            for (int dj = 0; dj < kNDJqk; ++dj) dq[dj] = E::mfma(read_tr(kt, lb, 32 * kb + 16 * ks, dj), dsf[kb][ks], dq[dj]);
      }
      dma_drain();
      __syncthreads();
    }

    // ---- epilogue: dQ = scale * dQ^T, fp32 store / accumulate or the final 16-bit store ----
    if (valid) {
      float* o1 = p.dq + b * p.dq_sb + (int64_t)row * p.dq_ss + h * p.dq_sh;
      char* h1 = p.dq16 ? p.dq16 + 2 * (b * p.dq16_sb + (int64_t)row * p.dq16_ss + h * p.dq16_sh) : nullptr;
      store_row32_acc<E, kNDJqk>(o1, h1, dq, p.scale, hi, p.accum_dq);
    }
  }  // next item
}

template <int DT, bool CAUSAL>
__global__ __launch_bounds__(256, 1) void flash_bwd_dkdv_qk192_kernel(const BwdParams p) {
  using E = Elem<DT>;
  using namespace qk192;
  constexpr int kBK = 128;                                  // keys per work item
  constexpr int kDObuf = 2 * kQkTileB;                      // LDS: Qbuf[0], Qbuf[1], dObuf[0], dObuf[1], stat[2][2][64] floats
  constexpr int kStat = kLdsB;
  extern __shared__ __attribute__((aligned(16))) char smem_raw[];
  USP_LDS char* smem = (USP_LDS char*)smem_raw;

  const int tid = threadIdx.x;
  const int lane = tid & 63;
  const int wave = __builtin_amdgcn_readfirstlane(tid >> 6);
  const int l31 = lane & 31, hi = lane >> 5;
  LaneBase lb(lane);
  const float c = p.scale_log2;
  int q_voff[6], do_voff[4];
  stage_offsets<3>(q_voff, wave, lane, (int)p.q_ss * 2);
  stage_offsets<2>(do_voff, wave, lane, (int)p.do_ss * 2);

  // ---- persistent workgroups over (batch, KV head, 128-key block) items; causal: early (heavy) key blocks first ----
  const ItemWalk walk(p.n_items);
  for (int pass = 0;; ++pass) {
    int w = walk.at(pass);
    if (w < 0) break;
    w = walk.dealt(w, p.nblk);
    const int kblk = w % p.nblk;
    int rest = w / p.nblk;
    const int hkv = rest % p.Hkv;
    const int b = rest / p.Hkv;
    const int k0 = kblk * kBK, kw = k0 + 32 * wave;
    const int off = p.causal_off;

    // ---- row tiles (usp_tile_range.h): [tb, te) hold a row that sees a key of the block; the item walks them once per head ----
    const int te = usp_tiles_holding(p.Sq, kRows);
    const int tb = usp_first_row_tile(k0, CAUSAL, off, te, kRows);
    const int ntl = te - tb;
    const int n_it = ntl * p.G;

    // ---- K and V fragments of the wave's keys (B operands: lane holds K[key][16 t + 8 hi .. + 7]) ----
    const int key = kw + l31;
    const int key_c = key < p.Sk ? key : p.Sk - 1;
    u32x4 kf[kNTqk], vf[kNTv];
    {
      const char* kp = p.k + 2 * (b * p.k_sb + (int64_t)key_c * p.k_ss + hkv * p.k_sh) + 16 * hi;
      const char* vp = p.v + 2 * (b * p.v_sb + (int64_t)key_c * p.v_ss + hkv * p.v_sh) + 16 * hi;
#pragma unroll
      for (int t = 0; t < kNTqk; ++t) kf[t] = *(const u32x4*)(kp + 32 * t);
#pragma unroll
      for (int t = 0; t < kNTv; ++t) vf[t] = *(const u32x4*)(vp + 32 * t);
    }
    f32x16 dv[kNDJv], dk[kNDJqk];
#pragma unroll
    for (int r = 0; r < 16; ++r) {
#pragma unroll
      for (int dj = 0; dj < kNDJv; ++dj) dv[dj][r] = 0.f;
#pragma unroll
      for (int dj = 0; dj < kNDJqk; ++dj) dk[dj][r] = 0.f;
    }

    // iteration `it` = (query head it / ntl of the group, row tile tb + it % ntl)
    auto stage = [&](int it, int buf) {
      const int h = hkv * p.G + it / ntl, s0 = (tb + it % ntl) * kRows;
      stage_tile<3>(tile_rsrc<kDqk>(p.q + 2 * (b * p.q_sb + h * p.q_sh), p.q_ss, s0, p.Sq), smem + buf * kQkTileB, wave, q_voff);
      stage_tile<2>(tile_rsrc<kDv>(p.dout + 2 * (b * p.do_sb + h * p.do_sh), p.do_ss, s0, p.Sq), smem + kDObuf + buf * kVTileB, wave,
                    do_voff);
    };
    // the tile's row statistics: waves 0 / 1 fetch -lse log2(e) / delta of row s0 + lane, and put it beside the tile later
    auto stat_fetch = [&](int it) -> float {
      const int h = hkv * p.G + it / ntl, r = (tb + it % ntl) * kRows + lane;
      const int r_c = r < p.Sq ? r : p.Sq - 1;
      if (wave == 0) return neg_lse_log2_qk192(p.lse[b * p.lse_sb + h * p.lse_sh + r_c], r < p.Sq);
      if (wave == 1) return r < p.Sq ? p.delta[b * p.dl_sb + h * p.dl_sh + r_c] : 0.f;
      return 0.f;
    };
    auto stat_put = [&](float x, int buf) {
      if (wave < 2) *(USP_LDS float*)(smem + kStat + ((buf * 2 + wave) * 64 + lane) * 4) = x;
    };

    if (n_it > 0) {
      stage(0, 0);
      stat_put(stat_fetch(0), 0);
      dma_drain();
      __syncthreads();
    }
    for (int it = 0; it < n_it; ++it) {
      float st_next = 0.f;
      if (it + 1 < n_it) { stage(it + 1, (it + 1) & 1); st_next = stat_fetch(it + 1); }
      const int s0 = (tb + it % ntl) * kRows;
      if (usp_row_tile_live(s0, kRows, kw, 32, p.Sk, CAUSAL, off, 0, 0)) {
        lb.keep_opaque();
        USP_LDS const char* qt = smem + (it & 1) * kQkTileB;
        USP_LDS const char* dot = smem + kDObuf + (it & 1) * kVTileB;
        USP_LDS const char* stat = smem + kStat + (it & 1) * 512;
        const bool masked = CAUSAL && s0 + off < kw + 31;       // some (row, key) of the tile lies above the diagonal
#pragma unroll
        for (int rb = 0; rb < 2; ++rb) {
          f32x16 s, dp;
#pragma unroll
          for (int r = 0; r < 16; ++r) { s[r] = 0.f; dp[r] = 0.f; }
#pragma unroll
          for (int t = 0; t < kNTqk; ++t) {
            s = E::mfma(read_rows(qt, lb, rb, t), kf[t], s);
            if (t < kNTv) dp = E::mfma(read_rows(dot, lb, rb, t), vf[t], dp);
          }
          if (masked) {
#pragma unroll
            for (int r = 0; r < 16; ++r)
              if (key > s0 + 32 * rb + acc_m(r, hi) + off) s[r] = USP_NEG_INF;
          }
          u32x4 pf[2], dsf[2];                              // packed P and dS [k-step]: B operands as they stand
#pragma unroll
          for (int q4 = 0; q4 < 4; ++q4) {                  // registers 4 q4 .. + 3 hold rows 32 rb + 8 q4 + 4 hi + 0 .. 3
            const f32x4 nl = *(USP_LDS const f32x4*)(stat + (32 * rb + 8 * q4 + 4 * hi) * 4);
            const f32x4 dl = *(USP_LDS const f32x4*)(stat + 256 + (32 * rb + 8 * q4 + 4 * hi) * 4);
            float pv[4], ds[4];
#pragma unroll
            for (int x = 0; x < 4; ++x) {
              pv[x] = fast_exp2(__builtin_fmaf(s[4 * q4 + x], c, nl[x]));
              ds[x] = pv[x] * (dp[4 * q4 + x] - dl[x]);
            }
            pf[q4 >> 1][2 * (q4 & 1)] = E::pack2(pv[0], pv[1]);
            pf[q4 >> 1][2 * (q4 & 1) + 1] = E::pack2(pv[2], pv[3]);
            dsf[q4 >> 1][2 * (q4 & 1)] = E::pack2(ds[0], ds[1]);
            dsf[q4 >> 1][2 * (q4 & 1) + 1] = E::pack2(ds[2], ds[3]);
          }
#pragma unroll
          for (int ks = 0; ks < 2; ++ks)
#pragma unroll
            for (int dj = 0; dj < kNDJqk; ++dj) {
              if (dj < kNDJv) dv[dj] = E::mfma(read_tr(dot, lb, 32 * rb + 16 * ks, dj), pf[ks], dv[dj]);
              dk[dj] = E::mfma(read_tr(qt, lb, 32 * rb + 16 * ks, dj), dsf[ks], dk[dj]);
            }
        }
      }
      stat_put(st_next, (it + 1) & 1);         // (the other buffer: last read in iteration it - 1)
      dma_drain();
      __syncthreads();
    }

    // ---- epilogue: dV = dV^T, dK = scale * dK^T, fp32 store / accumulate or the final 16-bit store ----
    if (key < p.Sk) {
      float* v1 = p.dv + b * p.dv_sb + (int64_t)key * p.dv_ss + hkv * p.dv_sh;
      char* v16 = p.dv16 ? p.dv16 + 2 * (b * p.dv16_sb + (int64_t)key * p.dv16_ss + hkv * p.dv16_sh) : nullptr;
      store_row32_acc<E, kNDJv>(v1, v16, dv, 1.f, hi, p.accum_dv);
      float* k1 = p.dk + b * p.dk_sb + (int64_t)key * p.dk_ss + hkv * p.dk_sh;
      char* k16 = p.dk16 ? p.dk16 + 2 * (b * p.dk16_sb + (int64_t)key * p.dk16_ss + hkv * p.dk16_sh) : nullptr;
      store_row32_acc<E, kNDJqk>(k1, k16, dk, p.scale, hi, p.accum_dk);
    }
  }  // next item
}

// the 80 KiB (+ 1 KiB of row statistics) of dynamic LDS are above the 64 KiB a launch gets unasked
template <class K> static int launch_big_lds_qk192(K* kern, int grid, size_t lds, hipStream_t st, const BwdParams& p) {
  if (hipFuncSetAttribute((const void*)kern, hipFuncAttributeMaxDynamicSharedMemorySize, (int)lds) != hipSuccess) {
    (void)hipGetLastError();
    return USP_ELAUNCH;
  }
  hipLaunchKernelGGL(kern, dim3(grid), dim3(256), lds, st, p);
  return launched();
}

int launch_dq_qk192(const BwdParams& p_in, int dtype, bool causal, hipStream_t st) {
  if (!dma_rows_ok(p_in.k_ss, false) || !dma_rows_ok(p_in.v_ss, false)) return USP_EUNSUPPORTED;   // 32-bit offsets into a tile
  BwdParams p = p_in;
  p.nblk = (p.Sq + 127) / 128;
  p.n_items = p.B * p.Hq * p.nblk;
  const int grid = persistent_grid(p.n_items, device_cus(), p.interleave);
  return with_dtype_causal(dtype, causal, [&](auto dt, auto c) -> int {
    return launch_big_lds_qk192(flash_bwd_dq_qk192_kernel<decltype(dt)::value, decltype(c)::value>, grid, qk192::kLdsB, st, p);
  });
}

int launch_dkdv_qk192(const BwdParams& p_in, int dtype, bool causal, hipStream_t st) {
  if (!dma_rows_ok(p_in.q_ss, false) || !dma_rows_ok(p_in.do_ss, false)) return USP_EUNSUPPORTED;
  BwdParams p = p_in;
  p.nblk = (p.Sk + 127) / 128;
  p.n_items = p.B * p.Hkv * p.nblk;
  const int grid = persistent_grid(p.n_items, device_cus(), p.interleave);
  return with_dtype_causal(dtype, causal, [&](auto dt, auto c) -> int {
    return launch_big_lds_qk192(flash_bwd_dkdv_qk192_kernel<decltype(dt)::value, decltype(c)::value>, grid, qk192::kLdsB + 1024, st, p);
  });
}

}  // namespace usp
