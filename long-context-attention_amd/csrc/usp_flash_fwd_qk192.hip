// Blockwise flash-attention forward for gfx950 at HEAD DIMS (192, 128) -- q and k of 192 dims, v and out of 128 (multi-head latent
// attention) --, one wave per SIMD: a workgroup is 4 waves x 64 query rows (256 rows of one (batch, head)), KV tile = 64 keys.  Entry
// usp_flash_fwd_vdim; same numerics and the same epilogue (fused ring LSE merge, final ranges) as the equal-dim kernels.
//
// Budget of a wave (512 registers: launch bounds of one wave per SIMD):
//   O^T          128 dims x 64 rows fp32 = 2 row blocks x 4 dim blocks of 32x32 = 128 registers
//   Q fragments  64 rows x 192 dims, B operand of S^T = K Q^T: 2 row blocks x 12 k-steps x 4 = 96 registers, loaded once per item
//   S^T          64 keys x 64 rows = 4 blocks = 64 registers, packed P 32
// Every K and V fragment read from LDS feeds TWO MFMAs, one per row block (the point of 64 rows per wave).  A tile is
// 48 MFMAs for S^T (2 key blocks x 12 k-steps x 2 row blocks) and 32 for O^T += V^T P^T (4 dim blocks x 4 k-steps x 2 row blocks).
// LDS: K tiles of 24 KiB and V tiles of 16 KiB in the family's panel image (usp_qk192.hpp), double-buffered = 80 KiB, filled by
// LDS-DMA one tile ahead; one barrier per tile.  The MFMAs are the builtins: hipcc pads their hazards (tools/mfma_hazards.py).
// The online softmax rescales a row block's O only when one of its rows' maximum moved (wave-uniform test).
#include "usp_fwd_params.hpp"
#include "usp_host.hpp"
#include "usp_mfma64.hpp"
#include "usp_qk192.hpp"

namespace usp {

template <int DT, bool CAUSAL>
__global__ __launch_bounds__(256, 1) void flash_fwd_qk192_kernel(const FwdArgsT<false> p) {
  using E = Elem<DT>;
  using namespace qk192;
  constexpr int kBM = 256;                    // query rows per workgroup
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

  // ---- persistent workgroups: each walks a static list of (batch, head, 256-row query tile) items, heavy causal tiles first, a
  // KV group's query heads side by side (ItemWalk) ----
  const ItemWalk walk(p.n_items);
  for (int pass = 0;; ++pass) {
    int w = walk.at(pass);
    if (w < 0) break;
    w = walk.grouped(walk.dealt(w, p.nq), p.nq, p.walk_g);
    const int qt_r = w % p.nq;
    int rest = w / p.nq;
    const int qt = CAUSAL ? (p.nq - 1 - qt_r) : qt_r;
    const int g = rest % p.G;
    rest /= p.G;
    const int hkv = rest % p.Hkv;
    const int b = rest / p.Hkv;
    const int h = hkv * p.G + g;
    const int q0 = qt * kBM, qw = q0 + 64 * wave;
    const int off = p.causal_off;

    // ---- tile ranges (usp_tile_range.h): nt tiles hold a key some row of the workgroup sees, n_w a key this wave sees, the
    // first n_full of them need no mask for this wave ----
    const usp_query_tiles tr = usp_query_tiles_of(q0, kBM, qw, 64, p.Sq, p.Sk, CAUSAL, off, kRows);
    const int nt = tr.nt, n_w = tr.n_w, n_full = tr.n_full;

    // ---- Q fragments (B operand: lane holds Q[row][16 t + 8 hi .. + 7]) of the wave's two row blocks ----
    u32x4 qf[2][kNTqk];
#pragma unroll
    for (int rq = 0; rq < 2; ++rq) {
      const int row = qw + 32 * rq + l31;
      const int row_c = row < p.Sq ? row : p.Sq - 1;
      const char* qp = p.q + 2 * (b * p.q_sb + (int64_t)row_c * p.q_ss + h * p.q_sh) + 16 * hi;
#pragma unroll
      for (int t = 0; t < kNTqk; ++t) qf[rq][t] = *(const u32x4*)(qp + 32 * t);
    }
    const char* kbase = p.k + 2 * (b * p.k_sb + hkv * p.k_sh);
    const char* vbase = p.v + 2 * (b * p.v_sb + hkv * p.v_sh);
    auto stage = [&](int tile, int buf) {
      stage_tile<3>(tile_rsrc<kDqk>(kbase, p.k_ss, tile * kRows, p.Sk), smem + buf * kQkTileB, wave, k_voff);
      stage_tile<2>(tile_rsrc<kDv>(vbase, p.v_ss, tile * kRows, p.Sk), smem + kVbuf + buf * kVTileB, wave, v_voff);
    };

    f32x16 o[2][kNDJv];
#pragma unroll
    for (int rq = 0; rq < 2; ++rq)
#pragma unroll
      for (int dj = 0; dj < kNDJv; ++dj)
#pragma unroll
        for (int r = 0; r < 16; ++r) o[rq][dj][r] = 0.f;
    float m_run[2] = {USP_NEG_INF, USP_NEG_INF};   // running row max, raw score units
    float l_run[2] = {0.f, 0.f};                   // this lane's share of the row sum

    if (nt > 0) {                              // (the previous item's last barrier stands behind its last LDS read)
      stage(0, 0);
      dma_drain();
      __syncthreads();
    }
    for (int j = 0; j < nt; ++j) {
      if (j + 1 < nt) stage(j + 1, (j + 1) & 1);           // buffers last read in iteration j - 1
      if (j < n_w) {
        lb.keep_opaque();
        USP_LDS const char* kt = smem + (j & 1) * kQkTileB;
        USP_LDS const char* vt = smem + kVbuf + (j & 1) * kVTileB;
        // S^T = K Q^T: [key block][row block], k-step major; one K fragment, two products
        f32x16 s[2][2];
#pragma unroll
        for (int kb = 0; kb < 2; ++kb)
#pragma unroll
          for (int rq = 0; rq < 2; ++rq)
#pragma unroll
            for (int r = 0; r < 16; ++r) s[kb][rq][r] = 0.f;
#pragma unroll
        for (int t = 0; t < kNTqk; ++t)
#pragma unroll
          for (int kb = 0; kb < 2; ++kb) {
            const u32x4 kf = read_rows(kt, lb, kb, t);
            s[kb][0] = E::mfma(kf, qf[0][t], s[kb][0]);
            s[kb][1] = E::mfma(kf, qf[1][t], s[kb][1]);
          }
        u32x4 pf[2][2][2];                                  // packed P^T [row block][key block][k-step]: B operands as they stand
#pragma unroll
        for (int rq = 0; rq < 2; ++rq) {
          if (j >= n_full) {                                // the diagonal / the ragged last tile
            int klim = p.Sk - 1;
            if (CAUSAL) klim = qw + 32 * rq + l31 + off < klim ? qw + 32 * rq + l31 + off : klim;
#pragma unroll
            for (int kb = 0; kb < 2; ++kb)
#pragma unroll
              for (int r = 0; r < 16; ++r)
                if (j * kRows + 32 * kb + acc_m(r, hi) > klim) s[kb][rq][r] = USP_NEG_INF;
          }
          // online softmax: the row of lane l31 is split over the two half-waves
          float mt = s[0][rq][0];
#pragma unroll
          for (int r = 1; r < 16; ++r) mt = fmaxf(mt, s[0][rq][r]);
#pragma unroll
          for (int r = 0; r < 16; ++r) mt = fmaxf(mt, s[1][rq][r]);
          const float m_new = fmaxf(m_run[rq], xhalf_max(mt));
          const float m_use = (m_new == USP_NEG_INF) ? 0.f : m_new;
          if (!__all(m_new == m_run[rq])) {
            const float alpha = fast_exp2(m_run[rq] * c - m_use * c);   // m_run = -inf: 0, and O and l are 0 anyway
            l_run[rq] *= alpha;
#pragma unroll
            for (int dj = 0; dj < kNDJv; ++dj)
#pragma unroll
              for (int r = 0; r < 16; ++r) o[rq][dj][r] *= alpha;
            m_run[rq] = m_new;
          }
          const float nmc = -(m_use * c);
          float rs = 0.f;
#pragma unroll
          for (int kb = 0; kb < 2; ++kb)
#pragma unroll
            for (int r = 0; r < 16; r += 2) {
              const float e0 = fast_exp2(__builtin_fmaf(s[kb][rq][r], c, nmc)), e1 = fast_exp2(__builtin_fmaf(s[kb][rq][r + 1], c, nmc));
              rs += e0 + e1;
              pf[rq][kb][r >> 3][(r & 7) >> 1] = E::pack2(e0, e1);
            }
          l_run[rq] += rs;
        }
        // O^T += V^T P^T: 4 k-steps x 4 dim blocks; one V fragment, two products
#pragma unroll
        for (int kb = 0; kb < 2; ++kb)
#pragma unroll
          for (int ks = 0; ks < 2; ++ks)
#pragma unroll
            for (int dj = 0; dj < kNDJv; ++dj) {
              const u32x4 vf = read_tr(vt, lb, 32 * kb + 16 * ks, dj);
              o[0][dj] = E::mfma(vf, pf[0][kb][ks], o[0][dj]);
              o[1][dj] = E::mfma(vf, pf[1][kb][ks], o[1][dj]);
            }
      }
      dma_drain();                 // this wave's pieces of the next tiles have landed ...
      __syncthreads();             // ... and so have everybody else's; every wave is done with this iteration's buffers
    }

    // ---- epilogue: normalise, merge with the running result, store (as usp_flash_fwd_d256.hip, one row block after the other) ----
#pragma unroll
    for (int rq = 0; rq < 2; ++rq) {
      const int row = qw + 32 * rq + l31;
      const float l_tot = xhalf_sum(l_run[rq]);
      const bool empty = !(l_tot > 0.f);
      const float inv = empty ? 0.f : 1.f / l_tot;
      const float blk_lse = empty ? USP_NEG_INF : (m_run[rq] * c + log2f(l_tot)) * kLn2;
      float w_blk = inv, w_old = 0.f, new_lse = blk_lse;
      const bool valid = row < p.Sq;
      const int row_c = valid ? row : p.Sq - 1;
      float* lse_p = p.lse + b * p.lse_sb + h * p.lse_sh + row_c;
      const bool fin = row >= p.final_begin && row < p.final_end;
      // single-pass call whose 32 rows are all final and 16-byte aligned: whole-row-piece stores
      const bool wide = !p.merge_in && p.out_wide && __all(!valid || fin);
      if (valid && p.merge_in) {
        const float old = *lse_p;
        const float mx = fmaxf(old, blk_lse);
        if (mx == USP_NEG_INF) {
          new_lse = USP_NEG_INF; w_old = 0.f; w_blk = 0.f;
        } else {
          const float e_old = exp2f((old - mx) * kLog2e);
          const float e_blk = exp2f((blk_lse - mx) * kLog2e);
          const float sum = e_old + e_blk;
          new_lse = mx + log2f(sum) * kLn2;
          w_old = e_old / sum;
          w_blk = e_blk / sum * inv;
        }
      }
      const int64_t arow = b * p.a_sb + (int64_t)row_c * p.a_ss + h * p.a_sh;
      const int64_t orow = b * p.o_sb + (int64_t)row_c * p.o_ss + h * p.o_sh;
      if (wide) {
        store_row16_wide<E, kNDJv>(p.out + 2 * orow, o[rq], w_blk, hi, valid);
        if (valid && hi == 0) *lse_p = new_lse;
      } else if (valid) {
#pragma unroll
        for (int dj = 0; dj < kNDJv; ++dj)
#pragma unroll
          for (int g4 = 0; g4 < 4; ++g4) {
            const int d0 = 32 * dj + 8 * g4 + 4 * hi;
            f32x4 val = {o[rq][dj][4 * g4] * w_blk, o[rq][dj][4 * g4 + 1] * w_blk, o[rq][dj][4 * g4 + 2] * w_blk,
                         o[rq][dj][4 * g4 + 3] * w_blk};
            if (p.merge_in) val += *(const f32x4*)(p.acc + arow + d0) * w_old;
            if (fin) *(u32x2*)(p.out + 2 * (orow + d0)) = u32x2{E::pack2(val[0], val[1]), E::pack2(val[2], val[3])};
            else *(f32x4*)(p.acc + arow + d0) = val;
          }
        // both half-waves have read the running LSE above: the wave runs in lockstep, the store follows the loads
        if (hi == 0) *lse_p = new_lse;
      }
    }
  }  // next item
}

int launch_fwd_qk192(const FwdParams& p_in, int dtype, bool causal, hipStream_t st) {
  // per-lane offsets into a 64-row tile are 32-bit
  if (!dma_rows_ok(p_in.k_ss, false) || !dma_rows_ok(p_in.v_ss, false)) return USP_EUNSUPPORTED;
  FwdArgsT<false> p;
  static_cast<FwdParams&>(p) = p_in;
  p.nq = (p.Sq + 255) / 256;
  p.n_items = p.B * p.Hq * p.nq;
  const int grid = persistent_grid(p.n_items, device_cus(), p.interleave);      // persistent: one workgroup per CU
  constexpr size_t lds = qk192::kLdsB;                                            // 80 KiB: above the 64 KiB a launch gets unasked
  return with_dtype_causal(dtype, causal, [&](auto dt, auto c) -> int {
    auto* kern = flash_fwd_qk192_kernel<decltype(dt)::value, decltype(c)::value>;
    if (hipFuncSetAttribute((const void*)kern, hipFuncAttributeMaxDynamicSharedMemorySize, (int)lds) != hipSuccess) {
      (void)hipGetLastError();
      return USP_ELAUNCH;
    }
    hipLaunchKernelGGL(kern, dim3(grid), dim3(256), lds, st, p);
    return launched();
  });
}

}  // namespace usp
