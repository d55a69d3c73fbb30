// Blockwise flash-attention forward for gfx950 on E4M3 q, k, v (one byte per element, OCP e4m3fn), head dim 128, one wave per SIMD:
// a workgroup is 4 waves x 64 query rows (256 rows of one (batch, head)), KV tile = 64 keys.  Entry usp_flash_fwd_fp8; 16-bit out
// (bf16 or fp16, chosen by the launch), fp32 acc and lse, and the epilogue of the other families (fused ring LSE merge, final ranges).
//
// Both products run on v_mfma_f32_32x32x64_f8f6f4 with e4m3 operands -- 64 k indices an instruction, twice the 16-bit rate:
//   S^T = K Q^T      2 key blocks x 2 k-steps x 2 row blocks = 8 MFMAs a tile; a K fragment (two ds_read_b128) feeds two of them
//   O^T += V^T P^T   4 dim blocks x 1 k-step (the tile's 64 keys) x 2 row blocks = 8 MFMAs; a V^T fragment (four ds_read_b64_tr_b8)
//                    feeds two of them
// 16 MFMAs of 16 passes for 64 x 64 scores, against 32 + 32 of 8 passes at 16 bits.  Operand orders and the LDS image: usp_fp8.hpp.
//
// Numbers (include/usp_hip.h, USP_ATTN_FP8): the two score descales are folded into the item's exponent scale c = softmax_scale *
// log2(e) * dq[b, h] * dk[b, hkv] -- nothing in the loop knows of them.  p = exp2(s c - m c + 8) in fp32 against the TRUE running
// maximum m (taken before the exponentials, so p <= 2^8 by construction and nothing above 448 reaches the conversion); the row sum
// adds these fp32 values, the value product takes them rounded to e4m3.  Both carry the 2^8, so O / l needs no compensation, dv[b,
// hkv] rides the epilogue factor and lse subtracts 8 in log2 units.
//
// Budget of a wave (512 registers: launch bounds of one wave per SIMD):
//   O^T          128 dims x 64 rows fp32 = 2 row blocks x 4 dim blocks of 32x32 = 128 registers
//   Q fragments  64 rows x 128 bytes, B operand of S^T: 2 row blocks x 2 k-steps x 8 = 32 registers, loaded once per item
//   S^T          64 keys x 64 rows = 4 blocks = 64 registers, packed P^T 16
// LDS: K and V tiles of 8 KiB each, double-buffered = 32 KiB, filled by LDS-DMA one tile ahead; one barrier per tile.  The MFMAs are
// the builtins: hipcc pads their hazards (tools/mfma_hazards.py).
#include "usp_fwd_params.hpp"
#include "usp_host.hpp"
#include "usp_mfma64.hpp"
#include "usp_fp8.hpp"

namespace usp {

struct FwdArgsFP8 : FwdParams {
  const float* dq; const float* dk; const float* dv;     // fp32 (B, Hq) / (B, Hkv) / (B, Hkv), contiguous; NULL = 1
};

template <int DT, bool CAUSAL>
__global__ __launch_bounds__(256, 1) void flash_fwd_fp8_kernel(const FwdArgsFP8 p) {
  using E = Elem<DT>;                         // the OUTPUT type
  using namespace fp8;
  constexpr int kBM = 256;                    // query rows per workgroup
  extern __shared__ __attribute__((aligned(16))) char smem_raw[];
  USP_LDS char* smem = (USP_LDS char*)smem_raw;            // Kbuf[0], Kbuf[1], Vbuf[0], Vbuf[1]

  const int tid = threadIdx.x;
  const int lane = tid & 63;
  const int wave = __builtin_amdgcn_readfirstlane(tid >> 6);
  const int l31 = lane & 31, hi = lane >> 5;
  LaneBase lb(lane);
  int k_voff[2], v_voff[2];
  stage_offsets(k_voff, wave, lane, (int)p.k_ss);
  stage_offsets(v_voff, wave, lane, (int)p.v_ss);

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
    // the item's exponent scale and epilogue factor carry the descales
    const float c = p.scale_log2 * (p.dq ? p.dq[b * p.Hq + h] : 1.f) * (p.dk ? p.dk[b * p.Hkv + hkv] : 1.f);
    const float dv = p.dv ? p.dv[b * p.Hkv + hkv] : 1.f;

    // ---- tile ranges (usp_tile_range.h): nt tiles hold a key some row of the workgroup sees, n_w a key this wave sees, the
    // first n_full of them need no mask for this wave ----
    const usp_query_tiles tr = usp_query_tiles_of(q0, kBM, qw, 64, p.Sq, p.Sk, CAUSAL, off, kRows);
    const int nt = tr.nt, n_w = tr.n_w, n_full = tr.n_full;

    // ---- Q fragments (B operand, the S^T byte order of usp_fp8.hpp) of the wave's two row blocks ----
    i32x8 qf[2][kNT];
#pragma unroll
    for (int rq = 0; rq < 2; ++rq) {
      const int row = qw + 32 * rq + l31;
      const int row_c = row < p.Sq ? row : p.Sq - 1;
      const char* qp = p.q + (b * p.q_sb + (int64_t)row_c * p.q_ss + h * p.q_sh) + 16 * hi;
#pragma unroll
      for (int t = 0; t < kNT; ++t) {
        const u32x4 a = *(const u32x4*)(qp + 64 * t), b2 = *(const u32x4*)(qp + 64 * t + 32);
        qf[rq][t] = i32x8{(int)a[0], (int)a[1], (int)a[2], (int)a[3], (int)b2[0], (int)b2[1], (int)b2[2], (int)b2[3]};
      }
    }
    const char* kbase = p.k + (b * p.k_sb + hkv * p.k_sh);
    const char* vbase = p.v + (b * p.v_sb + hkv * p.v_sh);
    auto stage = [&](int tile, int buf) {
      stage_tile(tile_rsrc(kbase, p.k_ss, tile * kRows, p.Sk), smem + buf * kTileB, wave, k_voff);
      stage_tile(tile_rsrc(vbase, p.v_ss, tile * kRows, p.Sk), smem + (2 + buf) * kTileB, wave, v_voff);
    };

    f32x16 o[2][kNDJ];
#pragma unroll
    for (int rq = 0; rq < 2; ++rq)
#pragma unroll
      for (int dj = 0; dj < kNDJ; ++dj)
#pragma unroll
        for (int r = 0; r < 16; ++r) o[rq][dj][r] = 0.f;
    float m_run[2] = {USP_NEG_INF, USP_NEG_INF};   // running row max, raw score units
    float l_run[2] = {0.f, 0.f};                   // this lane's share of the row sum, times 2^kPShift

    if (nt > 0) {                              // (the previous item's last barrier stands behind its last LDS read)
      stage(0, 0);
      dma_drain();
      __syncthreads();
    }
    for (int j = 0; j < nt; ++j) {
      if (j + 1 < nt) stage(j + 1, (j + 1) & 1);           // buffers last read in iteration j - 1
      if (j < n_w) {
        lb.keep_opaque();
        USP_LDS const char* kt = smem + (j & 1) * kTileB;
        USP_LDS const char* vt = smem + (2 + (j & 1)) * kTileB;
        // S^T = K Q^T: [key block][row block]; one K fragment, two products
        f32x16 s[2][2];
#pragma unroll
        for (int kb = 0; kb < 2; ++kb)
#pragma unroll
          for (int rq = 0; rq < 2; ++rq)
#pragma unroll
            for (int r = 0; r < 16; ++r) s[kb][rq][r] = 0.f;
#pragma unroll
        for (int t = 0; t < kNT; ++t)
#pragma unroll
          for (int kb = 0; kb < 2; ++kb) {
            const i32x8 kf = read_rows(kt, lb, kb, t);
            s[kb][0] = mfma(kf, qf[0][t], s[kb][0]);
            s[kb][1] = mfma(kf, qf[1][t], s[kb][1]);
          }
        i32x8 pf[2];                                        // packed e4m3 P^T [row block]: the B operand as it stands
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
            for (int dj = 0; dj < kNDJ; ++dj)
#pragma unroll
              for (int r = 0; r < 16; ++r) o[rq][dj][r] *= alpha;
            m_run[rq] = m_new;
          }
          const float nmc = (float)kPShift - m_use * c;     // s <= m_use: the exponent is at most kPShift (+ one fp32 rounding)
          float rs = 0.f;
#pragma unroll
          for (int kb = 0; kb < 2; ++kb)
#pragma unroll
            for (int r = 0; r < 16; r += 4) {
              const float e0 = fast_exp2(__builtin_fmaf(s[kb][rq][r], c, nmc)), e1 = fast_exp2(__builtin_fmaf(s[kb][rq][r + 1], c, nmc));
              const float e2 = fast_exp2(__builtin_fmaf(s[kb][rq][r + 2], c, nmc)), e3 = fast_exp2(__builtin_fmaf(s[kb][rq][r + 3], c, nmc));
              rs += (e0 + e1) + (e2 + e3);                  // the fp32 values: the row sum never sees the rounded ones
              pf[rq][4 * kb + (r >> 2)] = pack4(e0, e1, e2, e3);
            }
          l_run[rq] += rs;
        }
        // O^T += V^T P^T: the tile's 64 keys are ONE k-step; one V^T fragment, two products
#pragma unroll
        for (int dj = 0; dj < kNDJ; ++dj) {
          const i32x8 vf = read_tr(vt, lb, dj);
          o[0][dj] = mfma(vf, pf[0], o[0][dj]);
          o[1][dj] = mfma(vf, pf[1], o[1][dj]);
        }
      }
      dma_drain();                 // this wave's pieces of the next tiles have landed ...
      __syncthreads();             // ... and so have everybody else's; every wave is done with this iteration's buffers
    }

    // ---- epilogue: normalise, merge with the running result, store (as usp_flash_fwd_qk192.hip; dv rides the block's weight) ----
#pragma unroll
    for (int rq = 0; rq < 2; ++rq) {
      const int row = qw + 32 * rq + l31;
      const float l_tot = xhalf_sum(l_run[rq]);
      const bool empty = !(l_tot > 0.f);
      const float inv = empty ? 0.f : dv / l_tot;
      const float blk_lse = empty ? USP_NEG_INF : (m_run[rq] * c + (log2f(l_tot) - (float)kPShift)) * kLn2;
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
        store_row16_wide<E, kNDJ>(p.out + 2 * orow, o[rq], w_blk, hi, valid);
        if (valid && hi == 0) *lse_p = new_lse;
      } else if (valid) {
#pragma unroll
        for (int dj = 0; dj < kNDJ; ++dj)
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

int launch_fwd_fp8(const FwdParams& p_in, const float* q_descale, const float* k_descale, const float* v_descale, int out_dtype,
                   bool causal, hipStream_t st) {
  // per-lane offsets into a 64-row tile are 32-bit (row pitches are in bytes here)
  if (p_in.k_ss * 64 >= (1LL << 31) || p_in.v_ss * 64 >= (1LL << 31)) return USP_EUNSUPPORTED;
  FwdArgsFP8 p;
  static_cast<FwdParams&>(p) = p_in;
  p.dq = q_descale; p.dk = k_descale; p.dv = v_descale;
  p.nq = (p.Sq + 255) / 256;
  p.n_items = p.B * p.Hq * p.nq;
  const int grid = persistent_grid(p.n_items, device_cus(), p.interleave);      // persistent: one workgroup per CU
  return with_dtype_causal(out_dtype, causal, [&](auto dt, auto c) -> int {
    hipLaunchKernelGGL((flash_fwd_fp8_kernel<decltype(dt)::value, decltype(c)::value>), dim3(grid), dim3(256), fp8::kLdsB, st, p);
    return launched();
  });
}

}  // namespace usp
