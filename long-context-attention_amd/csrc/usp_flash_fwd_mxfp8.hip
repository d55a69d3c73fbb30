// Blockwise flash-attention forward for gfx950 on MXFP8 q, k, v (OCP Microscaling v1.0: e4m3 elements, one E8M0 power-of-two scale
// per block of 32), head dim 128, one wave per SIMD: a workgroup is 4 waves x 64 query rows, KV tile = 64 keys.  Entry
// usp_flash_fwd_mxfp8; 16-bit out (bf16 or fp16, chosen by the launch), fp32 acc and lse, the epilogue of the other families.
//
// Work split, tile image, LDS-DMA fill and operand byte orders are those of the per-head e4m3 forward (usp_flash_fwd_fp8.hip,
// usp_fp8.hpp).  What is new is that the block scales are applied INSIDE the matrix pipe: both products run on
// v_mfma_scale_f32_32x32x64_f8f6f4 with a scale register and an op_sel per operand (usp_mxfp8.hpp: the lane map, measured):
//   S^T = K Q^T      q and k carry 4 scales per token along the head dim.  A k-step of 64 dims is two MX blocks = the instruction's
//                    two k-blocks: A takes k_scale[key][2 t + hi], B takes q_scale[row][2 t + hi], op_sel = t on both
//   O^T += V^T P^T   v carries one scale per (32-key block, dim) along the sequence -- the reduction axis.  A tile of 64 keys is two
//                    blocks = the two k-blocks: A takes v_scale[2 tile + hi][32 dj + l31], op_sel = dj; B (P) takes the byte 127
// No fp32 multiply by a scale exists anywhere: the item's exponent scale is softmax_scale * log2(e) alone and the epilogue factor 1 / l.
// The loop costs, beside the fp8 one, per tile and lane: 2 dword loads (k scales of the wave's 2 x 32 keys) and 4 byte loads (v scales),
// issued a tile ahead into registers, and 7 VALU to permute / pack them.  The Q scales are one dword per row block, once per item.
//
// Numbers (include/usp_hip.h, USP_ATTN_MXFP8): p = exp2(s c - m c + 8) in fp32 against the TRUE running maximum m, the row sum adds
// these fp32 values, the value product takes them rounded to e4m3; lse subtracts the 8 in log2 units.
//
// Budget of a wave (512 registers): O^T 128, Q fragments 32, S^T 64, packed P^T 16 as usp_flash_fwd_fp8.hip; scales 2 (Q) + 2 + 4
// (K, V of the next tile) + 3 (packed, this tile).  LDS: K and V tiles of 8 KiB, double-buffered = 32 KiB; one barrier per tile.
// The MFMAs are the builtins: hipcc pads their hazards (tools/mfma_hazards.py).
#include "usp_fwd_params.hpp"
#include "usp_host.hpp"
#include "usp_mfma64.hpp"
#include "usp_mxfp8.hpp"

namespace usp {

struct FwdArgsMXFP8 : FwdParams {
  // E8M0 bytes, strides in bytes, unit last stride: (B, Sq, Hq, 4), (B, Sk, Hkv, 4), (B, ceil(Sk / 32), Hkv, 128)
  const char* qs; const char* ks; const char* vs;
  int64_t qs_sb, qs_ss, qs_sh, ks_sb, ks_ss, ks_sh, vs_sb, vs_ss, vs_sh;
};

template <int DT, bool CAUSAL>
__global__ __launch_bounds__(256, 1) void flash_fwd_mxfp8_kernel(const FwdArgsMXFP8 p) {
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
    const float c = p.scale_log2;              // no descale: every scale rides an MFMA

    // ---- tile ranges (usp_tile_range.h): nt tiles hold a key some row of the workgroup sees, n_w a key this wave sees, the
    // first n_full of them need no mask for this wave ----
    const usp_query_tiles tr = usp_query_tiles_of(q0, kBM, qw, 64, p.Sq, p.Sk, CAUSAL, off, kRows);
    const int nt = tr.nt, n_w = tr.n_w, n_full = tr.n_full;

    // ---- Q fragments (B operand, the S^T byte order of usp_fp8.hpp) of the wave's two row blocks ----
    i32x8 qf[2][kNT];
    int qsc[2];                                // ... and their scale registers: byte t = block 2 t + hi of the row
#pragma unroll
    for (int rq = 0; rq < 2; ++rq) {
      const int row = qw + 32 * rq + l31;
      const int row_c = row < p.Sq ? row : p.Sq - 1;
      qsc[rq] = mx::scale_pair(*(const uint32_t*)(p.qs + (b * p.qs_sb + (int64_t)row_c * p.qs_ss + h * p.qs_sh)), hi);
      const char* qp = p.q + (b * p.q_sb + (int64_t)row_c * p.q_ss + h * p.q_sh) + 16 * hi;
#pragma unroll
      for (int t = 0; t < kNT; ++t) {
        const u32x4 a = *(const u32x4*)(qp + 64 * t), b2 = *(const u32x4*)(qp + 64 * t + 32);
        qf[rq][t] = i32x8{(int)a[0], (int)a[1], (int)a[2], (int)a[3], (int)b2[0], (int)b2[1], (int)b2[2], (int)b2[3]};
      }
    }
    const char* kbase = p.k + (b * p.k_sb + hkv * p.k_sh);
    const char* vbase = p.v + (b * p.v_sb + hkv * p.v_sh);
    // the scale bytes of tile `tile`, raw: the four of key 32 kb + l31, and v_scale[2 tile + hi][32 dj + l31]
    const char* ksbase = p.ks + (b * p.ks_sb + hkv * p.ks_sh);
    const char* vsbase = p.vs + (b * p.vs_sb + hkv * p.vs_sh) + l31;
    const int last_blk = (p.Sk - 1) / mx::kBlock;
    auto fetch_scales = [&](int tile, uint32_t (&kraw)[2], int (&vraw)[kNDJ]) {
#pragma unroll
      for (int kb = 0; kb < 2; ++kb) {
        const int key = tile * kRows + 32 * kb + l31;
        kraw[kb] = *(const uint32_t*)(ksbase + (int64_t)(key < p.Sk ? key : p.Sk - 1) * p.ks_ss);
      }
      const int blk = 2 * tile + hi;
      const char* vrow = vsbase + (int64_t)(blk < last_blk ? blk : last_blk) * p.vs_ss;
#pragma unroll
      for (int dj = 0; dj < kNDJ; ++dj) vraw[dj] = *(const uint8_t*)(vrow + 32 * dj);
    };
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

    uint32_t kraw[2] = {0u, 0u};
    int vraw[kNDJ] = {0, 0, 0, 0};
    if (nt > 0) {                              // (the previous item's last barrier stands behind its last LDS read)
      fetch_scales(0, kraw, vraw);
      stage(0, 0);
      dma_drain();
      __syncthreads();
    }
    for (int j = 0; j < nt; ++j) {
      const int ksc[2] = {mx::scale_pair(kraw[0], hi), mx::scale_pair(kraw[1], hi)};
      const int vsc = mx::scale_quad(vraw);
      if (j + 1 < nt) {
        fetch_scales(j + 1, kraw, vraw);                   // into registers, ahead of the DMA: its wait does not hold them back
        stage(j + 1, (j + 1) & 1);                         // buffers last read in iteration j - 1
      }
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
        for (int kb = 0; kb < 2; ++kb) {
          const i32x8 k0 = read_rows(kt, lb, kb, 0), k1 = read_rows(kt, lb, kb, 1);
#pragma unroll
          for (int rq = 0; rq < 2; ++rq) {
            s[kb][rq] = mx::mfma<0, 0>(k0, qf[rq][0], s[kb][rq], ksc[kb], qsc[rq]);
            s[kb][rq] = mx::mfma<1, 1>(k1, qf[rq][1], s[kb][rq], ksc[kb], qsc[rq]);
          }
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
        // (op_sel is an immediate: the four dim blocks are written out)
#define USP_MX_PV(DJ)                                                              \
        {                                                                          \
          const i32x8 vf = read_tr(vt, lb, DJ);                                    \
          o[0][DJ] = mx::mfma<DJ, 0>(vf, pf[0], o[0][DJ], vsc, mx::kOne);          \
          o[1][DJ] = mx::mfma<DJ, 0>(vf, pf[1], o[1][DJ], vsc, mx::kOne);          \
        }
        USP_MX_PV(0) USP_MX_PV(1) USP_MX_PV(2) USP_MX_PV(3)
#undef USP_MX_PV
      }
      dma_drain();                 // this wave's pieces of the next tiles have landed ...
      __syncthreads();             // ... and so have everybody else's; every wave is done with this iteration's buffers
    }

    // ---- epilogue: normalise, merge with the running result, store (as usp_flash_fwd_fp8.hip, without a descale) ----
#pragma unroll
    for (int rq = 0; rq < 2; ++rq) {
      const int row = qw + 32 * rq + l31;
      const float l_tot = xhalf_sum(l_run[rq]);
      const bool empty = !(l_tot > 0.f);
      const float inv = empty ? 0.f : 1.f / l_tot;
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

int launch_fwd_mxfp8(const FwdParams& p_in, const usp_tensor& q_scale, const usp_tensor& k_scale, const usp_tensor& v_scale,
                     int out_dtype, bool causal, hipStream_t st) {
  // per-lane offsets into a 64-row tile are 32-bit (row pitches are in bytes here)
  if (p_in.k_ss * 64 >= (1LL << 31) || p_in.v_ss * 64 >= (1LL << 31)) return USP_EUNSUPPORTED;
  FwdArgsMXFP8 p;
  static_cast<FwdParams&>(p) = p_in;
  p.qs = (const char*)q_scale.ptr; p.qs_sb = q_scale.stride_b; p.qs_ss = q_scale.stride_s; p.qs_sh = q_scale.stride_h;
  p.ks = (const char*)k_scale.ptr; p.ks_sb = k_scale.stride_b; p.ks_ss = k_scale.stride_s; p.ks_sh = k_scale.stride_h;
  p.vs = (const char*)v_scale.ptr; p.vs_sb = v_scale.stride_b; p.vs_ss = v_scale.stride_s; p.vs_sh = v_scale.stride_h;
  p.nq = (p.Sq + 255) / 256;
  p.n_items = p.B * p.Hq * p.nq;
  const int grid = persistent_grid(p.n_items, device_cus(), p.interleave);      // persistent: one workgroup per CU
  return with_dtype_causal(out_dtype, causal, [&](auto dt, auto c) -> int {
    hipLaunchKernelGGL((flash_fwd_mxfp8_kernel<decltype(dt)::value, decltype(c)::value>), dim3(grid), dim3(256), fp8::kLdsB, st, p);
    return launched();
  });
}

}  // namespace usp
