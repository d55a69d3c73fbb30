// Gathered-key sparse forward for gfx950 (include/usp_hip.h: USP_ATTN_KEY_INDEX): causal attention in which row i sees a band below
// its diagonal plus a short sorted per-(batch, head) list of individual keys.  Head dims 64 and 128, bf16 and fp16.
//
// Work item: (batch, head, 128-row tile), 4 waves x 32 rows; persistent workgroups, late (heavy) row tiles first.  An item walks
//   phase G   the list in tiles of 64 entries: tile row r is key entry[64 t + r], wherever it lies.  The list is sorted, so the tiles
//             whose first entry lies at or below the item's last diagonal position are a prefix; it is counted once per item.
//   phase B   the contiguous 64-key tiles that cover [d_lo - left, d_hi] of the item (none without a window),
// as ONE sequence of tiles through one pipeline: a band tile is a gathered tile whose entries are key0 + r.  The entries of tile t
// stand in a ring of 256-byte index tiles in LDS, written two tiles ahead by wave 0 (the list is read from memory a tile before that);
// the staging lanes turn them into LDS-DMA offsets (usp_gather.hpp), the masking lanes compare them with the row's bounds:
//   gathered  entry in [0, d_i - left)   (no window: [0, d_i])      -- in the band: the band tile counts it, not this one
//   band      entry in [max(0, d_i - left), d_i]
// both as one unsigned compare (entry - lo) < cnt.  Every entry is range-checked where it is read: an absent one (outside [0, Sk))
// fetches zeros through the descriptor's byte count and is masked.  K and V tiles are double-buffered, one barrier per tile; the
// S^T = K Q^T and O^T += V^T P^T chains, the transposed V reads and the lazy online softmax are those of the head-dim-256 forward.
// Registers (D = 128): O^T 64, Q fragments 32, S^T 32, packed P 16: two waves per SIMD; LDS 65 KiB per workgroup.
#include "usp_host.hpp"
#include "usp_mfma64.hpp"
#include "usp_gather.hpp"

namespace usp {

template <int D, int DT>
__global__ __launch_bounds__(256, 2) void flash_fwd_gather_kernel(const FwdArgsGather p) {
  using E = Elem<DT>;
  using namespace gather;
  using I = Img<D>;
  constexpr int kBM = 128;                    // query rows per workgroup
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
  const int n_lt = (p.n_idx + kRows - 1) / kRows;          // tiles of the whole list

  const ItemWalk walk(p.n_items);
  for (int pass = 0;; ++pass) {
    int w = walk.at(pass);
    if (w < 0) break;
    w = walk.grouped(walk.dealt(w, p.nq), p.nq, p.walk_g);
    const int qt = p.nq - 1 - w % p.nq;                    // late row tiles see more of the list: first
    int rest = w / p.nq;
    const int g = rest % p.G;
    rest /= p.G;
    const int hkv = rest % p.Hkv;
    const int b = rest / p.Hkv;
    const int h = hkv * p.G + g;
    const int q0 = qt * kBM, qw = q0 + 32 * wave;
    const int* list = p.kidx + b * p.kidx_sb + h * p.kidx_sh;

    // ---- the item's tiles: nG gathered, then nB band tiles from key tile kt0 on ----
    const int d_lo = q0 + off;
    const int d_hi = (q0 + kBM < p.Sq ? q0 + kBM : p.Sq) - 1 + off;        // <= Sk - 1
    int nG = 0;
    for (int t0 = 0; t0 < n_lt; t0 += 256) {               // (every thread: the count is a barrier)
      const int t = t0 + tid;
      nG += __syncthreads_count(d_hi >= 0 && t < n_lt && list[t * kRows] <= d_hi);
    }
    int kt0 = 0, nB = 0;
    if (p.win_on && d_hi >= 0) {
      const int lo = d_lo - p.left;
      kt0 = (lo > 0 ? lo : 0) / kRows;
      nB = d_hi / kRows - kt0 + 1;
    }
    const int nt = nG + nB;
    // what this wave's 32 rows reach
    const int wd_lo = qw + off;
    const int wd_hi = (qw + 32 < p.Sq ? qw + 32 : p.Sq) - 1 + off;
    const bool wave_on = qw < p.Sq && wd_hi >= 0;

    // entry of tile t for this lane (wave 0): absent behind the list's end
    auto entry_of = [&](int t) -> int {
      if (t >= nG) return (kt0 + t - nG) * kRows + lane;
      const int pos = t * kRows + lane;
      return pos < p.n_idx ? list[pos] : 0x7fffffff;
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

    // ---- Q fragments (B operand: lane holds Q[row][16 t + 8 hi .. + 7]) ----
    const int row = qw + l31;
    u32x4 qf[I::kNT];
    {
      const int row_c = row < p.Sq ? row : p.Sq - 1;
      const char* qp = p.q + 2 * (b * p.q_sb + (int64_t)row_c * p.q_ss + h * p.q_sh) + 16 * hi;
#pragma unroll
      for (int t = 0; t < I::kNT; ++t) qf[t] = *(const u32x4*)(qp + 32 * t);
    }
    // the row's bounds: a column with entry e counts iff (unsigned)(e - lo) < cnt
    const int d_i = row + off;
    const int below = d_i - p.left > 0 ? d_i - p.left : 0;
    const int cnt_g = p.win_on ? below : (d_i + 1 > 0 ? d_i + 1 : 0);
    const int cnt_b = d_i + 1 - below > 0 ? d_i + 1 - below : 0;

    f32x16 o[I::kNDJ];
#pragma unroll
    for (int dj = 0; dj < I::kNDJ; ++dj)
#pragma unroll
      for (int r = 0; r < 16; ++r) o[dj][r] = 0.f;
    float m_run = USP_NEG_INF;                 // running row max, raw score units
    float l_run = 0.f;                         // this lane's share of the row sum

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
      if (j + 1 < nt) stage(j + 1, (j + 1) & 1);           // buffers last read in iteration j - 1
      int e_ahead = 0;
      if (wave == 0 && j + 2 < nt) e_ahead = entry_of(j + 2);                   // in flight across the tile's arithmetic
      USP_LDS const int* ent = ring + (j & (kRing - 1)) * kRows;
      const bool band = j >= nG;
      const int e_first = __builtin_amdgcn_readfirstlane(ent[0]);
      // does the tile hold a key some row of this wave sees; does every row see every key of it (band tiles only)
      bool need = wave_on && e_first <= wd_hi, full = false;
      if (band) {
        need = need && e_first + kRows - 1 >= wd_lo - p.left;
        full = e_first + kRows - 1 <= wd_lo && wd_hi - e_first <= p.left;
      }
      if (need) {
        lb.keep_opaque();
        USP_LDS const char* kt = smem + (j & 1) * I::kTileB;
        USP_LDS const char* vt = smem + (2 + (j & 1)) * I::kTileB;
        // S^T = K Q^T: two key blocks, k-step major (no dependent neighbours)
        f32x16 s[2];
#pragma unroll
        for (int kb = 0; kb < 2; ++kb)
#pragma unroll
          for (int r = 0; r < 16; ++r) s[kb][r] = 0.f;
#pragma unroll
        for (int t = 0; t < I::kNT; ++t)
#pragma unroll
          for (int kb = 0; kb < 2; ++kb) s[kb] = E::mfma(lb.read_rows(kt, kb, t), qf[t], s[kb]);
        if (!full) {
          const int lo = band ? below : 0;
          const unsigned cnt = (unsigned)(band ? cnt_b : cnt_g);
#pragma unroll
          for (int kb = 0; kb < 2; ++kb)
#pragma unroll
            for (int g4 = 0; g4 < 4; ++g4) {
              const u32x4 e4 = *(USP_LDS const u32x4*)(ent + 32 * kb + 8 * g4 + 4 * hi);      // columns acc_m(4 g4 .. + 3, hi)
#pragma unroll
              for (int x = 0; x < 4; ++x)
                if (!(e4[x] - (unsigned)lo < cnt)) s[kb][4 * g4 + x] = USP_NEG_INF;
            }
        }
        // online softmax: the row of lane l31 is split over the two half-waves; an all-masked tile leaves m_run at -inf
        float mt = s[0][0];
#pragma unroll
        for (int r = 1; r < 16; ++r) mt = fmaxf(mt, s[0][r]);
#pragma unroll
        for (int r = 0; r < 16; ++r) mt = fmaxf(mt, s[1][r]);
        const float m_new = fmaxf(m_run, xhalf_max(mt));
        const float m_use = (m_new == USP_NEG_INF) ? 0.f : m_new;
        if (!__all(m_new == m_run)) {
          const float alpha = fast_exp2(m_run * c - m_use * c);     // m_run = -inf: 0, and O and l are 0 anyway
          l_run *= alpha;
#pragma unroll
          for (int dj = 0; dj < I::kNDJ; ++dj)
#pragma unroll
            for (int r = 0; r < 16; ++r) o[dj][r] *= alpha;
          m_run = m_new;
        }
        const float nmc = -(m_use * c);
        float rs = 0.f;
        u32x4 pf[2][2];                                     // packed P^T [key block][k-step]: the B operand as it stands
#pragma unroll
        for (int kb = 0; kb < 2; ++kb)
#pragma unroll
          for (int r = 0; r < 16; r += 2) {
            const float e0 = fast_exp2(__builtin_fmaf(s[kb][r], c, nmc)), e1 = fast_exp2(__builtin_fmaf(s[kb][r + 1], c, nmc));
            rs += e0 + e1;
            pf[kb][r >> 3][(r & 7) >> 1] = E::pack2(e0, e1);
          }
        l_run += rs;
        // O^T += V^T P^T: 4 k-steps x D / 32 dim blocks
#pragma unroll
        for (int kb = 0; kb < 2; ++kb)
#pragma unroll
          for (int ks = 0; ks < 2; ++ks)
#pragma unroll
            for (int dj = 0; dj < I::kNDJ; ++dj) o[dj] = E::mfma(lb.read_tr(vt, 32 * kb + 16 * ks, dj), pf[kb][ks], o[dj]);
      }
      if (wave == 0 && j + 2 < nt) ring[((j + 2) & (kRing - 1)) * kRows + lane] = e_ahead;   // slot of tile j - 2
      dma_drain();                 // this wave's pieces of the next tiles have landed ...
      __syncthreads();             // ... and so have everybody else's; every wave is done with this iteration's buffers
    }

    // ---- epilogue: normalise and store (a row that saw nothing: out = 0, lse = -inf) ----
    {
      const float l_tot = xhalf_sum(l_run);
      const bool empty = !(l_tot > 0.f);
      const float inv = empty ? 0.f : 1.f / l_tot;
      const float lse = empty ? USP_NEG_INF : (m_run * c + log2f(l_tot)) * kLn2;
      const bool valid = row < p.Sq;
      const int row_c = valid ? row : p.Sq - 1;
      char* orow = p.out + 2 * (b * p.o_sb + (int64_t)row_c * p.o_ss + h * p.o_sh);
      if (p.out_wide) {
        store_row16_wide<E, I::kNDJ>(orow, o, inv, hi, valid);
      } else if (valid) {
        store_row32_acc<E, I::kNDJ>(nullptr, orow, o, inv, hi, 0);
      }
      if (valid && hi == 0) p.lse[b * p.lse_sb + h * p.lse_sh + row_c] = lse;
    }
  }  // next item
}

int launch_fwd_gather(const FwdArgsGather& p_in, int D, int dtype, hipStream_t st) {
  FwdArgsGather p = p_in;
  p.nq = (p.Sq + 127) / 128;
  p.n_items = p.B * p.Hq * p.nq;
  const int grid = persistent_grid(p.n_items, 2 * device_cus(), p.interleave);      // two workgroups per CU
  return with_dtype(dtype, [&](auto dt) -> int {
    auto go = [&](auto d) -> int {
      constexpr int kD = decltype(d)::value;
      constexpr size_t lds = 4 * gather::Img<kD>::kTileB + gather::kRing * gather::kRows * 4;
      auto* kern = flash_fwd_gather_kernel<kD, decltype(dt)::value>;
      if (hipFuncSetAttribute((const void*)kern, hipFuncAttributeMaxDynamicSharedMemorySize, (int)lds) != hipSuccess) {
        (void)hipGetLastError();
        return USP_ELAUNCH;
      }
      hipLaunchKernelGGL(kern, dim3(grid), dim3(256), lds, st, p);
      return launched();
    };
    return D == 128 ? go(Int<128>{}) : go(Int<64>{});
  });
}

}  // namespace usp

// usp_flash_fwd_gather (include/usp_hip.h: USP_ATTN_KEY_INDEX): checked in the order of the header's table, nothing launched or
// written by a call that is declined.
extern "C" int usp_flash_fwd_gather(const usp_fwd_args* args, const int32_t* key_index, int64_t index_stride_b, int64_t index_stride_h,
                                    int32_t n_index, void* stream) {
  using namespace usp;
  launch_kinds_reset();
  if (!args || !args->lse) return USP_EINVAL;
  const usp_fwd_args& a = *args;
  if (!key_index || n_index < 1 || !aligned(key_index, 4) || index_stride_b < 0 || index_stride_h < 0) return USP_EINVAL;
  if (int rc = check_problem(a)) return rc;
  if (!a.causal || (a.D != 64 && a.D != 128)) return USP_EUNSUPPORTED;
  const bool has_win = (a.flags & USP_ATTN_WINDOW) != 0;
  if (has_win && a.window_right != 0) return USP_EUNSUPPORTED;
  if (a.flags & (USP_ATTN_SOFTCAP | USP_ATTN_SHIFT | USP_FORCE_ROW64 | USP_FORCE_WAVE32)) return USP_EUNSUPPORTED;
  if (a.seq_q || a.seq_k || a.merge_in || a.acc.ptr) return USP_EUNSUPPORTED;
  if (a.final_begin > 0 || a.final_end < a.Sq) return USP_EUNSUPPORTED;        // rows that would stay in acc
  if (!tensor_aligned(a.q, 16, 8) || !tensor_aligned(a.k, 16, 8) || !tensor_aligned(a.v, 16, 8)) return USP_EUNSUPPORTED;
  if (!tensor_aligned(a.out, 8, 4)) return a.out.ptr ? USP_EUNSUPPORTED : USP_EINVAL;
  // a lane's offset into a (batch, kv head) plane is 32-bit and an absent entry's lies behind the plane: planes end below 2^31 bytes
  const int64_t k_bytes = ((int64_t)(a.Sk - 1) * a.k.stride_s + a.D) * 2, v_bytes = ((int64_t)(a.Sk - 1) * a.v.stride_s + a.D) * 2;
  if (a.k.stride_s < 0 || a.v.stride_s < 0 || k_bytes >= (1LL << 31) - 16 || v_bytes >= (1LL << 31) - 16) return USP_EUNSUPPORTED;

  FwdArgsGather p;
  p.q = (const char*)a.q.ptr; p.k = (const char*)a.k.ptr; p.v = (const char*)a.v.ptr;
  p.out = (char*)a.out.ptr; p.acc = nullptr; p.lse = a.lse;
  p.q_sb = a.q.stride_b; p.q_ss = a.q.stride_s; p.q_sh = a.q.stride_h;
  p.k_sb = a.k.stride_b; p.k_ss = a.k.stride_s; p.k_sh = a.k.stride_h;
  p.v_sb = a.v.stride_b; p.v_ss = a.v.stride_s; p.v_sh = a.v.stride_h;
  p.o_sb = a.out.stride_b; p.o_ss = a.out.stride_s; p.o_sh = a.out.stride_h;
  p.a_sb = p.a_ss = p.a_sh = 0;
  p.lse_sb = a.lse_stride_b; p.lse_sh = a.lse_stride_h;
  p.B = a.B; p.Sq = a.Sq; p.Sk = a.Sk; p.Hq = a.Hq; p.Hkv = a.Hkv;
  p.G = a.Hq / a.Hkv;
  p.nq = 0; p.n_items = 0;                         // set in launch_fwd_gather
  p.causal_off = a.Sk - a.Sq;
  p.scale = a.softmax_scale;
  p.scale_log2 = a.softmax_scale * kLog2e;
  p.merge_in = 0; p.final_begin = 0; p.final_end = a.Sq;
  p.out_wide = tensor_aligned(a.out, 16, 8) ? 1 : 0;
  p.seq_q = nullptr; p.seq_k = nullptr; p.sched = nullptr;
  p.interleave = (a.flags & USP_LAUNCH_INTERLEAVE) ? 1 : 0;
  p.walk_g = p.G;                                  // a KV group's heads side by side in the item walk
  p.kidx = key_index; p.kidx_sb = index_stride_b; p.kidx_sh = index_stride_h; p.n_idx = n_index;
  p.win_on = has_win ? 1 : 0;
  p.left = !has_win ? 0 : (a.window_left < 0 || a.window_left > a.Sk ? a.Sk : a.window_left);    // (negative: no left bound)
  p.k_bytes = (int)k_bytes; p.v_bytes = (int)v_bytes;
  const int rc = launch_fwd_gather(p, a.D, a.dtype, (hipStream_t)stream);
  if (rc == USP_OK) launch_kinds_note(USP_KIND_FWD_GATHER);
  return rc;
}
