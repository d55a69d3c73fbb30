// Body of the two-waves-per-SIMD backward kernels (usp_flash_bwd*.hip): the dQ launch, 8 waves x 32 query rows.
// Contract: the including __global__ template has D / DT in scope and defines `p_in` (its argument block, by value) and CAUSAL;
// everything else -- SC AL DR DOC SPAN BSP and their values -- is derived from p_in's type by usp_flash_bwd_prelude.inc.  A switch
// that is off compiles none of its `if constexpr` steps.  DESIGN.md, "How a kernel variant is declared".
// (Not a header: no include guard, no declarations of its own outside the function body.)
#include "usp_flash_bwd_prelude.inc"
  using E = Elem<DT>;
  constexpr int NT = 512;     // threads
  constexpr int OWN = (NT / 64) * 32;           // query rows of the workgroup
  constexpr int ROWB = D * 2;
  constexpr int TILEB = kTile * ROWB;           // one K (or V) tile
  constexpr int BUFB = 2 * TILEB;
  constexpr int NKT = D / 16;
  constexpr int NDJ = D / 32;

  extern __shared__ __attribute__((aligned(16))) char smem_raw[];
  USP_LDS char* smem = (USP_LDS char*)smem_raw;

  const int tid = threadIdx.x;
  const int lane = tid & 63;
  const int wave = __builtin_amdgcn_readfirstlane(tid >> 6);
  const int l31 = lane & 31;
  const int hi = lane >> 5;

  // ---- work items (persistent workgroups, usp_common.hpp ItemWalk) ------------------------------------
  const ItemWalk walk(p_in.n_items);
  ItemQueue queue{p_in.sched, p_in.seq_q, p_in.n_items / p_in.nblk, p_in.nblk,
                  p_in.Hq, OWN, CAUSAL ? 1 : 0};
  int qstate = 0;
  USP_LDS int* qslots = (USP_LDS int*)(smem + p_in.sched_lds);
  for (int pass = 0;; ++pass) {
  int w = p_in.sched ? item_queue_next(queue, qstate, qslots, pass) : walk.at(pass);
  if (w < 0) break;
  BwdParams p = p_in;
  if (!p_in.sched) w = walk.dealt(w, p.nblk);
  const int blk_r = w % p.nblk;
  int rest = w / p.nblk;
  const int blk = CAUSAL ? (p.nblk - 1 - blk_r) : blk_r;   // late query blocks see most keys
  int cut = 0;
  if (p.ksplit > 1) { cut = rest % p.ksplit; rest /= p.ksplit; }
  const int g = rest % p.G; rest /= p.G;
  const int hkv = rest % p.Hkv, b = rest / p.Hkv;
  const int h0 = hkv * p.G + g;
  int64_t ws_row0;
  if (!bind_sequence(p, b, &ws_row0)) continue;
  const int own0 = blk * OWN;                  // first query row of the block
  if (p.seq_q != nullptr && own0 >= (p.Sq)) continue;   // past the end of its sequence
  const int off = p.causal_off;
  const int ow = own0 + wave * 32;             // first row of this wave
  const int orow = ow + l31;                   // this lane's row
  const int orow_c = orow < p.Sq ? orow : p.Sq - 1;

  // ---- register-resident Q and dO fragments (B operands: lane holds row[16t + 8hi .. +7]) ----------
  u32x4 qf[NKT], dof[NKT];
  {
    const char* qp = p.q + 2 * (b * p.q_sb + (int64_t)orow_c * p.q_ss + h0 * p.q_sh);
    const char* dop = p.dout + 2 * (b * p.do_sb + (int64_t)orow_c * p.do_ss + h0 * p.do_sh);
#pragma unroll
    for (int t = 0; t < NKT; ++t) {
      qf[t] = *(const u32x4*)(qp + 32 * t + 16 * hi);
      dof[t] = *(const u32x4*)(dop + 32 * t + 16 * hi);
    }
  }
  // lane-local row statistics
  const float l_ = p.lse[b * p.lse_sb + h0 * p.lse_sh + orow_c];
  const float lse2_l = (l_ == USP_NEG_INF) ? __builtin_inff() : l_ * kLog2e;
  const float delta_l = p.delta[b * p.dl_sb + h0 * p.dl_sh + orow_c];

  // ---- streamed range: key tiles [t_begin, t_end) (usp_tile_range.h) ---------------------------------
  int t_end = (p.Sk + kTile - 1) / kTile;
  if (CAUSAL) t_end = usp_tiles_holding(usp_rows_key_end(own0, OWN, p.Sq, p.Sk, 1, off), kTile);
  // key tiles left of the window of the block's first row: not streamed
  int t_begin = usp_first_key_tile(own0, p.win_on, p.win_lo, t_end, kTile);
  if (p.ksplit > 1) {             // this item's cut of the key tiles [t_begin, t_end): equal runs
    const int per = (t_end - t_begin + p.ksplit - 1) / p.ksplit;   // = usp_run_length: called, every stream changes
    t_begin = usp_run_begin(t_begin, t_end, per, cut);
    t_end = usp_run_end(t_begin, t_end, per);
  }
  // DOC: row i sees key j only if j >= row_lo[i] (monotone, usp_tile_range.h): the key tiles in front of the first key of the
  // block's first row are not streamed; the lane keeps its own row's bound, the wave the bounds of its first and last valid row
  [[maybe_unused]] int doc_lo = 0, doc_lo_w0 = 0, doc_lo_w1 = 0;
  if constexpr (DOC) {
    const int* const rl = doc_row_lo + b * doc_rl_sb;
    t_begin = usp_doc_first_key_tile(usp_doc_row_lo(rl, own0, p.Sq, p.Sk), t_end, kTile);
    doc_lo = usp_doc_row_lo(rl, orow, p.Sq, p.Sk);
    doc_lo_w0 = usp_doc_row_lo(rl, ow, p.Sq, p.Sk);
    doc_lo_w1 = usp_doc_row_lo(rl, ow + 31, p.Sq, p.Sk);
  }
  // SPAN (usp_flash_bwd_span.hip, DOC with a right bound, never CAUSAL): ... and only if j < row_hi[i] (monotone): the key tiles
  // behind the last key of the block's last valid row are not streamed; lane and wave keep their bounds like the left ones
  [[maybe_unused]] int span_hi = 0, span_hi_w0 = 0, span_hi_w1 = 0;
  if constexpr (SPAN) {
    const int* const rh = span_row_hi + b * span_rh_sb;
    t_end = usp_span_key_tiles_end(usp_span_row_hi(rh, own0 + OWN - 1, p.Sq, p.Sk), t_end, kTile);
    if (t_begin > t_end) t_begin = t_end;
    span_hi = usp_span_row_hi(rh, orow, p.Sq, p.Sk);
    span_hi_w0 = usp_span_row_hi(rh, ow, p.Sq, p.Sk);
    span_hi_w1 = usp_span_row_hi(rh, ow + 31, p.Sq, p.Sk);
  }
  // BSP (usp_flash_bwd_bsp.hip): the 256-row block holds TWO row blocks of the 128 x 128 block mask; it streams the ascending union
  // of their lists (usp_block_lists.hip), entry = 4 * key tile + (bit 0: live for rows [0, 128), bit 1: for [128, 256)) -- under
  // CAUSAL without the blocks above the diagonal.  A wave skips the compute of an entry dead for its half, and still stages and
  // meets the barrier.  Count and entries are clamped as read; the entry of an iteration was read when its tile was staged.
  // The entries come 64 at a time, one per lane (one vector load every 64 tiles), and the cursor picks its own with
  // v_readlane: no memory latency in front of a stage's descriptors.  (It measured like a scalar load per tile: the 1.8 x of
  // this kernel on an all-set mask against the plain one lies elsewhere -- profiles/block_mask_rates.txt.)
  [[maybe_unused]] const int* bsp_l = nullptr;
  [[maybe_unused]] int bsp_cnt = 0, bsp_i = 0, bsp_ent = 0, bsp_vec = 0;
  if constexpr (BSP) {
    bsp_l = bsp_lists + ((int64_t)(b * p.Hq + h0) * p.nblk + blk) * bsp_stride;
    const int c0 = bsp_l[0], cap = bsp_stride - 2;
    bsp_cnt = (c0 < 0 || t_end <= 0) ? 0 : (c0 > cap ? cap : c0);
    t_begin = 0;
  }
  const int n_iter = BSP ? bsp_cnt : t_end - t_begin;

  // ---- staging: LDS-DMA (buffer_load ... lds), no staging registers, no ds_write ---------------------
  // One wave-instruction fills 1 KiB of LDS linearly (wave-uniform base + lane*16), i.e. 1024/ROWB
  // whole tile rows.  The slot swizzle is therefore applied on the SOURCE: the lane that lands on
  // physical slot p of row r fetches logical slot p ^ swz(r) of that row (same 16-byte chunks of the
  // same row: coalescing is unaffected).  Rows past the end of the tensor read as 0 (descriptor
  // bounds); hipcc drains the DMA (vmcnt(0)) in front of the s_barrier that ends the iteration.
  constexpr int NW = NT / 64;                     // waves
  constexpr int CHUNKS = TILEB / 1024;            // 1 KiB pieces per K (or V) tile
  constexpr int CPW = (CHUNKS + NW - 1) / NW;     // pieces per wave per tile
  constexpr int RPC = 1024 / ROWB;                // tile rows per piece
  int k_voff[CPW], v_voff[CPW];
#pragma unroll
  for (int i = 0; i < CPW; ++i) {
    const int cidx = wave + NW * i;
    const int r = cidx * RPC + lane / (D / 8);
    const int c8 = (lane % (D / 8)) ^ tile_swz<D>(r);
    k_voff[i] = r * (int)p.k_ss * 2 + c8 * 16;
    v_voff[i] = r * (int)p.v_ss * 2 + c8 * 16;
  }
  // Prefetch cursor: running 64-bit tile pointers / remaining-bytes counters, advanced by additions only.
  decltype(__builtin_amdgcn_make_buffer_rsrc((void*)nullptr, 0, 0, 0)) k_rs, v_rs;
  int dma_buf = 0;
  const int64_t k_step = (int64_t)kTile * p.k_ss * 2, v_step = (int64_t)kTile * p.v_ss * 2;   // bytes per tile step
  // the cursor starts at tile t_begin of the K / V rows of (b, hkv)
  const char* k_next = p.k + 2 * (b * p.k_sb + hkv * p.k_sh) + t_begin * k_step;
  const char* v_next = p.v + 2 * (b * p.v_sb + hkv * p.v_sh) + t_begin * v_step;
  int64_t k_rem = ((int64_t)(p.Sk - 1 - t_begin * kTile) * p.k_ss + D) * 2;
  int64_t v_rem = ((int64_t)(p.Sk - 1 - t_begin * kTile) * p.v_ss + D) * 2;
  // build the descriptors for the cursor's tile, then advance the cursor
  auto stage_setup = [&](int buf) {
    auto clampu = [](int64_t r) { return (int)(uint32_t)(r < 0 ? 0 : (r > 0xffffffffLL ? 0xffffffffLL : r)); };
    if constexpr (BSP) {                       // the cursor jumps to the next listed tile
      if ((bsp_i & 63) == 0) bsp_vec = bsp_i + lane < bsp_cnt ? bsp_l[1 + bsp_i + lane] : 0;
      const int e = __builtin_amdgcn_readlane(bsp_vec, bsp_i & 63);
      ++bsp_i;
      const int t = e < 0 ? 0 : ((e >> 2) >= t_end ? t_end - 1 : (e >> 2));
      bsp_ent = 4 * t + (e & 3);
      k_next = p.k + 2 * (b * p.k_sb + hkv * p.k_sh) + t * k_step;
      v_next = p.v + 2 * (b * p.v_sb + hkv * p.v_sh) + t * v_step;
      k_rem = ((int64_t)(p.Sk - 1 - t * kTile) * p.k_ss + D) * 2;
      v_rem = ((int64_t)(p.Sk - 1 - t * kTile) * p.v_ss + D) * 2;
    }
    k_rs = __builtin_amdgcn_make_buffer_rsrc((void*)k_next, 0, clampu(k_rem), 0x00020000);
    v_rs = __builtin_amdgcn_make_buffer_rsrc((void*)v_next, 0, clampu(v_rem), 0x00020000);
    dma_buf = buf;
    k_next += k_step; v_next += v_step; k_rem -= k_step; v_rem -= v_step;
  };
  // piece pi in [0, 2*CPW): K (pi even) or V (pi odd), chunk wave + NW * (pi >> 1)
  auto stage_piece = [&](int pi) {
    const int i = pi >> 1;
    const int cidx = wave + NW * i;
    if (CHUNKS % NW == 0 || cidx < CHUNKS) {
      USP_LDS char* dst = smem + dma_buf * BUFB + cidx * 1024;
      if ((pi & 1) == 0) lds_dma16(k_rs, dst, k_voff[i]);
      else lds_dma16(v_rs, dst + TILEB, v_voff[i]);
    }
  };
  auto stage_all = [&]() {
#pragma unroll
    for (int pi = 0; pi < 2 * CPW; ++pi) stage_piece(pi);
  };

  // ---- per-lane LDS read addresses ----------------------------------------------------------------
  // row read (A operand of S / T): tile row 32*n32 + l31, logical slot 2kt + hi
  const int rd_row = l31 * ROWB;
  const int rd_x = hi ^ tile_swz<D>(l31);
  // transpose read (A operand of the gradient MFMAs) for dim tile dj, element half e, k-step ks:
  // the 16-lane group reads the [4 rows][16 dims] block rows 16ks + 8e + 4hi + (0..3),
  // dims 32dj + 16*grp + (0..15); lane i supplies row i>>2, dims 4*(i&3)..+3.
  int tr_addr[NDJ][2];
  {
    const int i = lane & 15, grp = (lane >> 4) & 1;
#pragma unroll
    for (int dj = 0; dj < NDJ; ++dj)
#pragma unroll
      for (int e = 0; e < 2; ++e) {
        const int rr = 8 * e + 4 * hi + (i >> 2);
        const int slot = 4 * dj + 2 * grp + ((i & 3) >> 1);
        tr_addr[dj][e] = rr * ROWB + ((slot ^ tile_swz<D>(rr)) * 16) + (i & 1) * 8;
      }
  }

  // ---- accumulators -----------------------------------------------------------------------------
  f32x16 dq_acc[NDJ];                    // dQ^T
#pragma unroll
  for (int dj = 0; dj < NDJ; ++dj)
#pragma unroll
    for (int r = 0; r < 16; ++r) dq_acc[dj][r] = 0.f;
  const float c = p.scale_log2;
  // ALiBi: -slope * log2(e) of this item's (batch, head), read per item
  float al_ns2 = 0.f;
  if constexpr (AL) al_ns2 = -kLog2e * al_slopes[b * al_sb + h0];

  if (n_iter > 0) { stage_setup(0); stage_all(); }
  dma_drain();            // this wave's DMA pieces of the staged tile have landed (usp_common.hpp)
  __syncthreads();

  const f32x16 zero16 = {0.f, 0.f, 0.f, 0.f, 0.f, 0.f, 0.f, 0.f, 0.f, 0.f, 0.f, 0.f, 0.f, 0.f, 0.f, 0.f};
  constexpr int NST = 2 * NKT;                          // MFMAs of one S/T phase
  constexpr int NGR = 2 * NDJ;                          // MFMAs of one gradient phase

  int cur_tile = t_begin;                              // streamed tile of the current iteration
  for (int it = 0; it < n_iter; ++it) {
    const int buf = it & 1;
    const int tile = BSP ? (bsp_ent >> 2) : cur_tile;    // (BSP: read here, in front of the stage_setup that replaces it)
    [[maybe_unused]] const int bsp_halves = bsp_ent & 3;
    cur_tile = (cur_tile + 1 == t_end) ? t_begin : cur_tile + 1;
    const int s0 = tile * kTile;                       // first key of this tile
    const bool prefetch = it + 1 < n_iter;
    if (prefetch) stage_setup(buf ^ 1);

    int wave_kv_end = p.Sk;
    if (CAUSAL) wave_kv_end = usp_rows_key_end(ow, 32, p.Sq, p.Sk, 1, off);
    // active = usp_key_tile_live with wave_end = 0 for a wave past Sq, need_mask = usp_key_tile_masked (usp_tile_range.h):
    // called, either changes every stream
    bool active = ow < p.Sq && s0 < wave_kv_end && (!p.win_on || s0 + kTile - 1 >= ow + p.win_lo);
    bool need_mask = (s0 + kTile > p.Sk) || (CAUSAL && s0 + kTile - 1 > ow + off) || (p.win_on && s0 < ow + 31 + p.win_lo);
    if constexpr (DOC) {
      active = active && s0 + kTile > doc_lo_w0;                 // (usp_doc_key_tile_live's left-bound term)
      need_mask = need_mask || usp_doc_key_tile_masked(s0, doc_lo_w1);
    }
    if constexpr (SPAN) {
      active = active && s0 < span_hi_w1;                        // (usp_span_key_tile_live's right-bound term)
      need_mask = need_mask || usp_span_key_tile_masked(s0, kTile, span_hi_w0);
    }
    if constexpr (BSP) active = active && ((bsp_halves >> (wave >> 2)) & 1) != 0;     // waves 0-3: the first mask row block

    if (active) {
      // Hand-pinned pipeline over the two 32-row halves h0, h1 of the tile (sched_barrier(0) fences;
      // hipcc otherwise emits MFMA clusters and VALU clusters):
      //   ST(h0) | ST(h1) || P,dS(h0) | GRAD(h0) || P,dS(h1) | GRAD(h1)
      // LDS operands are prefetched two MFMAs ahead; the first MFMA of a chain takes C = 0.
      USP_LDS const char* k_lds = smem + buf * BUFB;  // K tile
      USP_LDS const char* v_lds = k_lds + TILEB;      // V tile
      f32x16 sS[2], sT[2];
      u32x4 pk_ds[2][2];
      // ALiBi: row + diag - key of register 0 of half 0 (key of register r of half h: s0 + 32 h + 4 hi + (r & 3) + 8 (r >> 2))
      [[maybe_unused]] const int al_d0 = orow + al_diag - s0 - 4 * hi;
      // dropout: the keep words of this lane's row against the tile's 64 keys (usp_dropout_rng.h); `active` is wave-uniform
      [[maybe_unused]] uint32_t kw[8];
      if constexpr (DR)
        usp_dropout_tile_words<true>(dr.k0, dr.k1, (uint32_t)b, dr.head0 + (uint32_t)h0, (dr.row0 + (uint32_t)orow) >> 2,
                                     ((dr.key0 + (uint32_t)s0) >> 2) + (uint32_t)hi, lane, kw);

      auto apply_mask = [&](int h) {
        const int k0 = s0 + 32 * h + 4 * hi;            // key of register r: k0 + 8(r>>2) + (r&3)
        int klim = p.Sk - 1;
        if (CAUSAL) klim = orow + off < klim ? orow + off : klim;
        int klo = p.win_on ? orow + p.win_lo : -0x40000000;
        if constexpr (DOC) klo = doc_lo;
        if constexpr (SPAN) klim = span_hi - 1 < klim ? span_hi - 1 : klim;
#pragma unroll
        for (int r = 0; r < 16; ++r) {
          const int key = k0 + (r & 3) + 8 * (r >> 2);
          if (key > klim || key < klo) sS[h][r] = USP_NEG_INF;
        }
      };
      // P and dS of element r of half h (+ pack when a pair completes)
      auto elem = [&](int h, int r) {
        float pr, ds;
        if constexpr (SC) {
          const float x = sS[h][r];                   // raw score, -inf where masked
          const float t = softcap_tanh(x, sc_k2);
          pr = fast_exp2(__builtin_fmaf(t, sc_cl2, -lse2_l));
          pr = x == USP_NEG_INF ? 0.f : pr;
          ds = pr * (sT[h][r] - delta_l) * __builtin_fmaf(-t, t, 1.f);
        } else if constexpr (AL) {                    // the bias goes into the exponent: P = exp2(S c + bias - lse2)
          const int d = al_d0 - (32 * h + (r & 3) + 8 * (r >> 2));
          pr = fast_exp2(__builtin_fmaf(sS[h][r], c, __builtin_fmaf(al_ns2, (float)(d < 0 ? -d : d), -lse2_l)));
          ds = pr * (sT[h][r] - delta_l);
        } else if constexpr (DR) {                    // dS = P (256/t keep dP - delta): delta is that of the dropped `out`
          pr = fast_exp2(__builtin_fmaf(sS[h][r], c, -lse2_l));
          const float nd = -delta_l;
          ds = pr * (usp_dropout_keep(kw[4 * h + (r >> 2)], r & 3, dr.t) ? __builtin_fmaf(dr.rs, sT[h][r], nd) : nd);
        } else {
          pr = fast_exp2(__builtin_fmaf(sS[h][r], c, -lse2_l));
          ds = pr * (sT[h][r] - delta_l);
        }
        sS[h][r] = pr;
        sT[h][r] = ds;
        if (r & 1) {
          // pin_here: hipcc otherwise SINKS the whole element block of half 0 out of the S/T phase it is meant to
          // hide behind, into the block of its first use (the gradient phase) -- ~110 VALU in front of the
          // first gradient MFMA (seen in the .s; sched_barrier only pins the machine scheduler inside a block)
          uint32_t w = E::pack2(sT[h][r - 1], sT[h][r]);
          pin_here(w);
          pk_ds[h][r >> 3][(r & 7) >> 1] = w;
        }
      };
      // S/T phase of half h; `vh` >= 0: interleave the element work of half vh
      auto st_phase = [&](int h, int vh) {
        u32x4 kf[NKT], vf[NKT];
        auto rd = [&](int kt) {
          const int a = h * 32 * ROWB + rd_row + (((2 * kt) ^ rd_x) * 16);
          kf[kt] = *(USP_LDS const u32x4*)(k_lds + a);
          vf[kt] = *(USP_LDS const u32x4*)(v_lds + a);
        };
        rd(0);
        if (NKT > 1) rd(1);
        __builtin_amdgcn_sched_barrier(0);
#pragma unroll
        for (int sl = 0; sl < NST; ++sl) {
          const int kt = sl >> 1;
          if ((sl & 1) == 0) {
            if (kt + 2 < NKT) rd(kt + 2);
            sS[h] = E::mfma(kf[kt], qf[kt], kt == 0 ? zero16 : sS[h]);
          } else {
            sT[h] = E::mfma(vf[kt], dof[kt], kt == 0 ? zero16 : sT[h]);
          }
          if (vh >= 0) {
#pragma unroll
            for (int e = sl * 16 / NST; e < (sl + 1) * 16 / NST; ++e) elem(vh, e);
          }
          __builtin_amdgcn_sched_barrier(0);
        }
      };
      // gradient phase of half h; `vh` >= 0: interleave the element work of half vh
      auto grad_phase = [&](int h, int vh) {
        u32x4 xa[NGR];
        auto rd = [&](int i) {                           // i -> (k2, dj): K^T fragments of the tile
          const int k2 = i / NDJ, dj = i % NDJ;
          USP_LDS const char* xb = k_lds + (2 * h + k2) * 16 * ROWB;
          const u32x2 a0 = lds_read_tr16(xb + tr_addr[dj][0]);
          const u32x2 a1 = lds_read_tr16(xb + tr_addr[dj][1]);
          xa[i] = u32x4{a0[0], a0[1], a1[0], a1[1]};
        };
        rd(0);
        if (NGR > 1) rd(1);
        __builtin_amdgcn_sched_barrier(0);
#pragma unroll
        for (int i = 0; i < NGR; ++i) {
          if (i + 2 < NGR) rd(i + 2);
          const int k2 = i / NDJ, dj = i % NDJ;
          dq_acc[dj] = E::mfma(xa[i], pk_ds[h][k2], dq_acc[dj]);
          if (vh >= 0) {
#pragma unroll
            for (int e = i * 16 / NGR; e < (i + 1) * 16 / NGR; ++e) elem(vh, e);
          }
          __builtin_amdgcn_sched_barrier(0);
        }
      };

      // the next tile's LDS-DMA pieces go out back to back in front of the first chain (spread over its MFMA slots they
      // measured +0.4 % here at two waves per SIMD, and +6 % in the dK/dV kernel)
      if (prefetch) stage_all();
      st_phase(0, -1);
      if (need_mask) apply_mask(0);
      st_phase(1, 0);
      if (need_mask) apply_mask(1);
      grad_phase(0, 1);
      grad_phase(1, -1);
    } else if (prefetch) {
      stage_all();
    }

    dma_drain();            // this wave's DMA pieces of the staged tile have landed (usp_common.hpp)
    __syncthreads();
  }

  // ---- epilogue: fp32 store / accumulate, or final 16-bit store ---------------------------------------
  if (orow < p.Sq) {
    float* o32;
    char* o16 = nullptr;                         // 16-bit final destination (row base), if any
    int accf;
    if (p.ksplit > 1) {   // partial of this cut, combined (deterministically) by reduce_cuts_kernel
      o32 = p.ws_dq + ((((int64_t)cut * p.B + b) * p.Sq + orow) * p.Hq + h0) * D; accf = 0;
    } else {
      o32 = p.dq + b * p.dq_sb + (int64_t)orow * p.dq_ss + h0 * p.dq_sh; accf = p.accum_dq;
      if (p.dq16) o16 = p.dq16 + 2 * (b * p.dq16_sb + (int64_t)orow * p.dq16_ss + h0 * p.dq16_sh);
    }
#pragma unroll
    for (int dj = 0; dj < NDJ; ++dj)
#pragma unroll
      for (int g4 = 0; g4 < 4; ++g4) {
        const int d0 = 32 * dj + 8 * g4 + 4 * hi;
        f32x4 v = {dq_acc[dj][4 * g4] * p.scale, dq_acc[dj][4 * g4 + 1] * p.scale,
                   dq_acc[dj][4 * g4 + 2] * p.scale, dq_acc[dj][4 * g4 + 3] * p.scale};
        if (accf) v += *(const f32x4*)(o32 + d0);
        if (o16) *(u32x2*)(o16 + 2 * d0) = u32x2{E::pack2(v[0], v[1]), E::pack2(v[2], v[3])};
        else *(f32x4*)(o32 + d0) = v;
      }
  }
  if (p_in.sched && p_in.interleave) break;   // one item per workgroup: leave room for other streams' kernels
  }  // next item
  if (p_in.sched && threadIdx.x == 0) item_queue_release(queue);
