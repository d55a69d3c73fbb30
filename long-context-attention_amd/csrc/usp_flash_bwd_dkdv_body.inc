// Body of the two-waves-per-SIMD backward kernels (usp_flash_bwd*.hip): the dK/dV launch, role-specialised waves.
// Contract: the including __global__ template has D / DT in scope and defines `p_in` (its argument block, by value) and CAUSAL;
// everything else -- SC AL DR DOC SPAN BSP and their values -- is derived from p_in's type by usp_flash_bwd_prelude.inc.  A switch
// that is off compiles none of its `if constexpr` steps.  DESIGN.md, "How a kernel variant is declared".
// Dropout: role A forms the un-dropped P, uses P o keep for its dV MFMAs and hands B the un-dropped P with the keep decision in
// the sign bit (P >= 0: set = dropped; no extra LDS); role B starts its dP chain from -delta t/256 and forms
// |P| (kept ? chain : -delta t/256); 256/t goes into the epilogue's factor of both outputs.
// (Not a header: no include guard, no declarations of its own outside the function body.)
#include "usp_flash_bwd_prelude.inc"
  using E = Elem<DT>;
  constexpr int NW = 8, OWN = 128;
  constexpr int ROWB = D * 2;
  constexpr int TILEB = kTile * ROWB;
  constexpr int STATB = 2 * kTile * 4;
  constexpr int BUFB = 2 * TILEB + STATB;
  constexpr int NBUF = 3;
  constexpr int PSLOT = 4096;                    // P of one 64 x 32 block, 16-bit
  constexpr int POFF = NBUF * BUFB;              // P exchange: [4 slices][2 slots][PSLOT]
  constexpr int NKT = D / 16;
  constexpr int NDJ = D / 32;
  constexpr int CHUNKS = TILEB / 1024;
  constexpr int CPW = (CHUNKS + NW - 1) / NW;
  constexpr int RPC = 1024 / ROWB;
  constexpr int NGR = 2 * NDJ;                   // gradient MFMAs per half
  constexpr int PF = 2;                          // LDS operands are fetched this many MFMAs ahead

  extern __shared__ __attribute__((aligned(16))) char smem_raw[];
  USP_LDS char* smem = (USP_LDS char*)smem_raw;

  const int tid = threadIdx.x;
  const int lane = tid & 63;
  const int wave = __builtin_amdgcn_readfirstlane(tid >> 6);
  const int role = wave >> 2;                    // 0: A (S, P, dV)   1: B (dP, dS, dK)
  const int slice = wave & 3;
  const int l31 = lane & 31;
  const int hi = lane >> 5;

  const ItemWalk walk(p_in.n_items);             // persistent workgroups (usp_common.hpp)
  ItemQueue queue{p_in.sched, p_in.seq_k, p_in.n_items / p_in.nblk, p_in.nblk,
                  p_in.Hkv * p_in.ngrp, OWN, 0};
  int qstate = 0;
  USP_LDS int* qslots = (USP_LDS int*)(smem + p_in.sched_lds);
  for (int pass = 0;; ++pass) {
  int w = p_in.sched ? item_queue_next(queue, qstate, qslots, pass) : walk.at(pass);
  if (w < 0) break;
  BwdParams p = p_in;
  if (!p_in.sched) w = walk.dealt(w, p.nblk);
  const int blk = w % p.nblk;                    // early key blocks are seen by most rows: first
  int rest = w / p.nblk;
  int g = 0, cut = 0;
  if (p.qsplit > 1) { cut = rest % p.qsplit; rest /= p.qsplit; }
  if (p.ngrp > 1) { g = rest % p.ngrp; rest /= p.ngrp; }
  const int hkv = rest % p.Hkv, b = rest / p.Hkv;
  const int h0 = hkv * p.G + g * p.gsub;
  int64_t ws_row0;
  if (!bind_sequence(p, b, &ws_row0)) continue;
  const int own0 = blk * OWN;
  if (p.seq_q != nullptr && own0 >= p.Sk) continue;          // past the end of its sequence
  const int off = p.causal_off;
  const int ow = own0 + slice * 32;
  const int orow = ow + l31;
  const int orow_c = orow < p.Sk ? orow : p.Sk - 1;

  // K (role A) or V (role B) fragments of this wave's 32 keys
  u32x4 rf[NKT];
  {
    const char* pr = role == 0 ? p.k + 2 * (b * p.k_sb + (int64_t)orow_c * p.k_ss + hkv * p.k_sh)
                               : p.v + 2 * (b * p.v_sb + (int64_t)orow_c * p.v_ss + hkv * p.v_sh);
#pragma unroll
    for (int t = 0; t < NKT; ++t) rf[t] = *(const u32x4*)(pr + 32 * t + 16 * hi);
  }

  // ---- streamed range: query tiles [t_begin, t_end) of each of the item's gsub heads (usp_tile_range.h) ---------------
  int t_end = (p.Sq + kTile - 1) / kTile;
  int t_begin = usp_first_row_tile(own0, CAUSAL, off, t_end, kTile);
  if (p.win_on) {                                // query rows beyond the window of the block's last key: not streamed
    t_end = usp_last_row_tile(own0, OWN, 1, p.win_lo, t_end, kTile);
    if (t_begin > t_end) t_begin = t_end;
  }
  if (p.qsplit > 1) {                            // this item's cut of the query tiles [t_begin, t_end): equal runs
    const usp_tile_run run = usp_equal_run(t_begin, t_end, p.qsplit, cut);
    t_begin = run.begin; t_end = run.end;
  }
  // DOC: row i sees key j only if i < key_hi[j] (monotone, usp_tile_range.h): the row tiles behind the last row that sees the
  // block's last key are not streamed; the lane keeps its own key's bound, the wave the bounds of its first and last valid key
  [[maybe_unused]] int doc_hi = 0, doc_hi_w0 = 0, doc_hi_w1 = 0;
  if constexpr (DOC) {
    const int* const kh = doc_key_hi + b * doc_kh_sb;
    t_end = usp_doc_last_row_tile(usp_doc_key_hi(kh, own0 + OWN - 1, p.Sq, p.Sk), t_end, kTile);
    if (t_begin > t_end) t_begin = t_end;
    doc_hi = usp_doc_key_hi(kh, orow, p.Sq, p.Sk);
    doc_hi_w0 = usp_doc_key_hi(kh, ow, p.Sq, p.Sk);
    doc_hi_w1 = usp_doc_key_hi(kh, ow + 31, p.Sq, p.Sk);
  }
  // SPAN (usp_flash_bwd_span.hip, DOC with the transpose of a right key bound, never CAUSAL): ... and only if i >= key_lo[j]
  // (monotone): the row tiles in front of the first row that sees the block's first key are not streamed
  [[maybe_unused]] int span_lo = 0, span_lo_w0 = 0, span_lo_w1 = 0;
  if constexpr (SPAN) {
    const int* const kl = span_key_lo + b * span_kl_sb;
    const int tb = usp_span_first_row_tile(usp_span_key_lo(kl, own0, p.Sq, p.Sk), t_end, kTile);
    t_begin = tb > t_begin ? tb : t_begin;
    span_lo = usp_span_key_lo(kl, orow, p.Sq, p.Sk);
    span_lo_w0 = usp_span_key_lo(kl, ow, p.Sq, p.Sk);
    span_lo_w1 = usp_span_key_lo(kl, ow + 31, p.Sq, p.Sk);
  }
  // BSP (usp_flash_bwd_bsp.hip): the 128-key block is ONE column of the 128 x 128 block mask; for each of its gsub query heads it
  // streams the ascending list of 64-row tiles of that head's transposed list (usp_block_lists.hip) -- under CAUSAL without the
  // blocks above the diagonal.  Only the staging cursor reads the lists (count and entries clamped as read); the two roles take the
  // tile of their iteration from what was staged one and two iterations ago.
  [[maybe_unused]] const int* bsp_l = nullptr;
  [[maybe_unused]] int bsp_cnt = 0, bsp_i = 0, bsp_total = 0, bsp_tn = 0, bsp_ta = 0, bsp_tb = 0;
  [[maybe_unused]] auto bsp_list_of = [&](int hh) { return bsp_lists + ((int64_t)(b * p.Hq + h0 + hh) * p.nblk + blk) * bsp_stride; };
  [[maybe_unused]] auto bsp_count_of = [&](const int* l) {
    const int c0 = l[0], cap = bsp_stride - 2;
    return (c0 < 0 || t_end <= 0) ? 0 : (c0 > cap ? cap : c0);
  };
  if constexpr (BSP) {
    t_begin = 0;
    for (int hh = 0; hh < p.gsub; ++hh) bsp_total += bsp_count_of(bsp_list_of(hh));
  }
  const int n_iter = BSP ? bsp_total : (t_end - t_begin) * p.gsub;

  // ---- LDS-DMA staging of the Q / dO tiles -----------------------------------------------------------------
  // ONE buffer descriptor pair per (item, query head), based on row 0 of that head; a tile is addressed by a scalar byte
  // offset (the instruction's soffset operand).  Per tile that is two s_add and the loads.  (Round 2 kept 64-bit tile
  // pointers / remaining-bytes counters and rebuilt both descriptors -- clamps included -- for every tile, and every
  // tile recomputed the 64-bit addresses of its row statistics: ~170 scalar instructions and 40-50 SGPR-spill reloads
  // (v_readlane) at the head of EVERY iteration of EVERY wave, 40 % of a wave's instruction stream -- the kernel was
  // bound by instruction issue, not by the MFMA pipe: with every element operation removed it still ran at 973 of
  // 1071 us, profiles/r03_bwd_ablations.txt.)  The host guarantees that a head's rows span less than 2^31 bytes.
  int q_voff[CPW], do_voff[CPW];
#pragma unroll
  for (int i = 0; i < CPW; ++i) {
    const int cidx = wave + NW * i;
    const int r = cidx * RPC + lane / (D / 8);
    const int c8 = (lane % (D / 8)) ^ tile_swz<D>(r);
    q_voff[i] = r * (int)p.q_ss * 2 + c8 * 16;
    do_voff[i] = r * (int)p.do_ss * 2 + c8 * 16;
  }
  float st_lse = 0.f, st_delta = 0.f;
  bool st_in = false;
  decltype(__builtin_amdgcn_make_buffer_rsrc((void*)nullptr, 0, 0, 0)) q_rs, do_rs;
  const int q_step = kTile * (int)p.q_ss * 2, do_step = kTile * (int)p.do_ss * 2;   // bytes per tile step
  int pf_tile = t_begin, pf_hh = 0, q_soff = 0, do_soff = 0;
  const float *lse_h = nullptr, *dl_h = nullptr;                             // row statistics of the cursor's head
  const bool stat_wave = wave == 4;              // a role-B wave fetches the tile's statistics: role A is the longer stream
  auto pf_head = [&]() {                         // (re)base the cursor on head h0 + pf_hh, tile t_begin
    auto clampu = [](int64_t r) { return (int)(uint32_t)(r < 0 ? 0 : (r > 0xffffffffLL ? 0xffffffffLL : r)); };
    const int h = h0 + pf_hh;
    q_rs = __builtin_amdgcn_make_buffer_rsrc((void*)(p.q + 2 * (b * p.q_sb + h * p.q_sh)), 0,
                                             clampu(((int64_t)(p.Sq - 1) * p.q_ss + D) * 2), 0x00020000);
    do_rs = __builtin_amdgcn_make_buffer_rsrc((void*)(p.dout + 2 * (b * p.do_sb + h * p.do_sh)), 0,
                                              clampu(((int64_t)(p.Sq - 1) * p.do_ss + D) * 2), 0x00020000);
    lse_h = p.lse + b * p.lse_sb + h * p.lse_sh;
    dl_h = p.delta + b * p.dl_sb + h * p.dl_sh;
    pf_tile = t_begin;
    q_soff = t_begin * q_step;
    do_soff = t_begin * do_step;
  };
  pf_head();
  // BSP: base the cursor on the first head from pf_hh on whose list is not empty (stage_next is called n_iter times: there is one)
  [[maybe_unused]] auto bsp_head = [&]() {
    for (; pf_hh < p.gsub; ++pf_hh) {
      bsp_l = bsp_list_of(pf_hh);
      bsp_cnt = bsp_count_of(bsp_l);
      if (bsp_cnt > 0) break;
    }
    bsp_i = 0;
    if (pf_hh < p.gsub) pf_head();
  };
  if constexpr (BSP) bsp_head();
  // issue the cursor's tile into LDS buffer `buf`, fetch its row statistics, advance the cursor
  auto stage_next = [&](int buf) {
    if constexpr (BSP) {                         // the cursor jumps to the next listed tile of its head
      const int e = bsp_l[1 + bsp_i];
      pf_tile = e < 0 ? 0 : (e >= t_end ? t_end - 1 : e);
      bsp_tn = pf_tile;
      q_soff = pf_tile * q_step;
      do_soff = pf_tile * do_step;
    }
    if (stat_wave) {                             // raw loads only: the values are consumed by stage_stats, a tile later
      const int r = pf_tile * kTile + lane;
      st_in = r < p.Sq;                          // rows past the end: P = 0 (their Q / dO rows read as zero)
      const int rc = st_in ? r : p.Sq - 1;
      st_lse = lse_h[rc];
      st_delta = dl_h[rc];
    }
#pragma unroll
    for (int i = 0; i < CPW; ++i) {
      const int cidx = wave + NW * i;
      if (CHUNKS % NW == 0 || cidx < CHUNKS) {
        USP_LDS char* dst = smem + buf * BUFB + cidx * 1024;
        lds_dma16(q_rs, dst, q_voff[i], q_soff);
        lds_dma16(do_rs, dst + TILEB, do_voff[i], do_soff);
      }
    }
    if constexpr (BSP) {
      if (++bsp_i == bsp_cnt) { ++pf_hh; bsp_head(); }
    } else {
    ++pf_tile;
    q_soff += q_step;
    do_soff += do_step;
    if (p.gsub > 1 && pf_tile == t_end) { ++pf_hh; pf_head(); }
    }
  };
  auto stage_stats = [&](int buf) {
    if (stat_wave) {
      const float l2 = (st_in && st_lse != USP_NEG_INF) ? st_lse * kLog2e : __builtin_inff();
      *(USP_LDS float*)(smem + buf * BUFB + 2 * TILEB + 4 * lane) = l2;
      *(USP_LDS float*)(smem + buf * BUFB + 2 * TILEB + 4 * kTile + 4 * lane) = st_in ? -st_delta : 0.f;   // NEGATED:
    }                                                                          // role B folds it into the dP chain
  };

  // ---- per-lane LDS addresses ------------------------------------------------------------------------
  const int rd_row = l31 * ROWB;
  const int rd_x = hi ^ tile_swz<D>(l31);
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
  USP_LDS char* pex = smem + POFF + slice * 2 * PSLOT + lane * 16;   // + slot*PSLOT + (2h+k2)*1024

  f32x16 acc[NDJ];                               // dV^T (role A) / dK^T (role B)
#pragma unroll
  for (int dj = 0; dj < NDJ; ++dj)
#pragma unroll
    for (int r = 0; r < 16; ++r) acc[dj][r] = 0.f;
  const float c = p.scale_log2;
  const f32x16 zero16 = {0.f, 0.f, 0.f, 0.f, 0.f, 0.f, 0.f, 0.f, 0.f, 0.f, 0.f, 0.f, 0.f, 0.f, 0.f, 0.f};

  if (n_iter > 0) { stage_next(0); stage_stats(0); }
  dma_drain();            // this wave's DMA pieces of the staged tile have landed (usp_common.hpp)
  __syncthreads();

  // The streaming loop is instantiated once per role, with ROLE a compile-time constant, and the role
  // is chosen by ONE branch around the whole loop: both roles execute the same barrier sequence.  (With
  // run-time role tests inside the per-element code every MFMA slot was split into several basic
  // blocks: 5.9 SALU per MFMA and 51 % of wave cycles parked; with one loop holding both roles' tile
  // bodies their loop invariants added up and the kernel spilled.)
  auto stream = [&](auto role_c) {
    constexpr int ROLE = decltype(role_c)::value;
    int tile_a = t_begin;                          // streamed tile role A works on in iteration `it`
    int tile_b = t_begin;                          // ... and role B (the previous tile of A)
    int buf_a = 0, buf_b = NBUF - 1;               // LDS buffers of those tiles (it % 3, (it - 1) % 3)
    // ALiBi, role A: -slope * log2(e) of the query head being streamed; an item streams `gsub` heads one after the other,
    // so it is read again at the first tile of each
    [[maybe_unused]] float al_ns2 = 0.f;
    [[maybe_unused]] int al_hh = 0;
    // dropout, role A: the query head being streamed (the mask's counter holds the QUERY head), counted like al_hh
    [[maybe_unused]] uint32_t dr_h = 0;
    [[maybe_unused]] int dr_hh = 0;
    for (int it = 0; it <= n_iter; ++it) {
      const bool prefetch = it + 1 < n_iter;
      const int buf_n = buf_a + 1 == NBUF ? 0 : buf_a + 1;      // (it + 1) % NBUF
      if constexpr (BSP) { bsp_tb = bsp_ta; bsp_ta = bsp_tn; }  // (in front of the stage_next that replaces bsp_tn)
      if (prefetch) stage_next(buf_n);

      const int my_it = it - ROLE;
      const int tile = BSP ? (ROLE == 0 ? bsp_ta : bsp_tb) : (ROLE == 0 ? tile_a : tile_b);
      tile_b = tile_a;
      tile_a = (tile_a + 1 == t_end) ? t_begin : tile_a + 1;
      const int s0 = tile * kTile;
      const bool valid = my_it >= 0 && my_it < n_iter;
      if constexpr (AL) {
        if (ROLE == 0 && valid && tile == t_begin) al_ns2 = -kLog2e * al_slopes[b * al_sb + h0 + al_hh++];
      }
      // = usp_row_tile_live, usp_row_tile_masked (usp_tile_range.h): called, either changes every stream
      if constexpr (DR) {
        if (ROLE == 0 && valid && tile == t_begin) dr_h = dr.head0 + (uint32_t)(h0 + dr_hh++);
      }
      bool active = valid && ow < p.Sk && (!CAUSAL || (s0 + kTile - 1 + off >= ow)) &&
                    (!p.win_on || s0 <= ow + 31 - p.win_lo);
      bool need_mask = (CAUSAL && (s0 + off < ow + 31)) || (p.win_on && s0 + kTile - 1 > ow - p.win_lo);
      if constexpr (DOC) {
        active = active && usp_doc_row_tile_live(s0, doc_hi_w1);
        need_mask = need_mask || usp_doc_row_tile_masked(s0, kTile, doc_hi_w0);
      }
      if constexpr (SPAN) {
        active = active && usp_span_row_tile_live(s0, kTile, span_lo_w0);
        need_mask = need_mask || usp_span_row_tile_masked(s0, span_lo_w1);
      }

      if (active) {
        USP_LDS const char* q_lds = smem + (ROLE == 0 ? buf_a : buf_b) * BUFB;   // Q tile
        USP_LDS const char* do_lds = q_lds + TILEB;            // dO tile
        USP_LDS const char* xs = ROLE == 0 ? q_lds : do_lds;   // row-read operand of the S / dP chain
        USP_LDS const char* xg = ROLE == 0 ? do_lds : q_lds;   // transpose-read operand of the gradient
        USP_LDS const char* stat = q_lds + 2 * TILEB + (ROLE == 0 ? 0 : 4 * kTile);
        USP_LDS char* pslot = pex + (my_it & 1) * PSLOT;
        f32x16 sc[2];                                          // S (role A) / dP (role B) of the two halves
        u32x4 pk[2][2];                                        // packed P (A) / dS (B): B operand of the gradient
        u32x4 pin[2][2];                                       // role B: P received from A
        f32x4 st4;
        f32x4 stq[4];                                          // row statistics of one half, fetched ahead of use
        float pg_prev = 0.f;                                   // softcap, role A: P (1 - t^2) of the previous element
        u32x4 pkg;                                             // ... packed: the k-step handed to B
        // ALiBi: row + diag - key of register 0 of half 0 (query row of register r of half h: s0 + 32 h + 4 hi + (r & 3) + 8 (r >> 2))
        [[maybe_unused]] const int al_d0 = s0 + 4 * hi + al_diag - orow;
        // dropout, role A: the keep words of this lane's key against the tile's 64 rows (usp_dropout_rng.h); `active` is
        // wave-uniform
        [[maybe_unused]] uint32_t kw[8];
        if constexpr (DR) {
          if (ROLE == 0)
            usp_dropout_tile_words<false>(dr.k0, dr.k1, (uint32_t)b, dr_h, (dr.key0 + (uint32_t)orow) >> 2,
                                          ((dr.row0 + (uint32_t)s0) >> 2) + (uint32_t)hi, lane, kw);
        }
        auto load_stat = [&](int h, int j) {
          stq[j] = *(USP_LDS const f32x4*)(stat + (32 * h + 4 * hi) * 4 + 32 * j);
        };
        auto load_stats = [&](int h) {
#pragma unroll
          for (int j = 0; j < 4; ++j) load_stat(h, j);
        };

        // element r of half h: role A: P = exp2(S*c - lse2); role B: dS = P * (dP - delta), where the dP chain
        // STARTS from -delta (the MFMA's C operand = the row statistics tuple: one VALU per score less in the role
        // that has the most of them)
        auto elem = [&](int h, int r) {
          if (ROLE == 0 && (r & 3) == 0) st4 = stq[r >> 2];
          float val;
          if (ROLE == 0) {
            if constexpr (SC) {
              const float x = sc[h][r];                         // raw score, -inf where masked
              const float t = softcap_tanh(x, sc_k2);
              val = fast_exp2(__builtin_fmaf(t, sc_cl2, -st4[r & 3]));
              val = x == USP_NEG_INF ? 0.f : val;
              const float pg = val * __builtin_fmaf(-t, t, 1.f);
              if (r & 1) pkg[(r & 7) >> 1] = E::pack2(pg_prev, pg);
              else pg_prev = pg;
            } else if constexpr (AL) {                        // the bias goes into the exponent: P = exp2(S c + bias - lse2)
              const int d = al_d0 + (32 * h + (r & 3) + 8 * (r >> 2));
              val = fast_exp2(__builtin_fmaf(sc[h][r], c, __builtin_fmaf(al_ns2, (float)(d < 0 ? -d : d), -st4[r & 3])));
            } else if constexpr (DR) {
              const float pu = fast_exp2(__builtin_fmaf(sc[h][r], c, -st4[r & 3]));   // the un-dropped P
              const bool kept = usp_dropout_keep(kw[4 * h + (r >> 2)], r & 3, dr.t);
              val = kept ? pu : 0.f;                             // dV takes P o keep
              const float ph = kept ? pu : -pu;                  // B takes P, sign bit = dropped
              if (r & 1) pkg[(r & 7) >> 1] = E::pack2(pg_prev, ph);
              else pg_prev = ph;
            } else {
              val = fast_exp2(__builtin_fmaf(sc[h][r], c, -st4[r & 3]));
            }
          } else {
            const uint32_t wd = pin[h][r >> 3][(r & 7) >> 1];
            const float pr = (r & 1) ? E::hi(wd) : E::lo(wd);
            if constexpr (DR) {
              // -delta t/256 of the element's row again (the chain's start; the tuple of four rows is re-read from the
              // statistics in LDS rather than held in 32 registers across the phases)
              if ((r & 3) == 0) st4 = *(USP_LDS const f32x4*)(stat + (32 * h + 4 * hi) * 4 + 32 * (r >> 2)) * dr.irs;
              val = __builtin_fabsf(pr) * (__builtin_signbit(pr) ? st4[r & 3] : sc[h][r]);
            } else {
              val = pr * sc[h][r];
            }
          }
          sc[h][r] = val;
          if (r & 1) pk[h][r >> 3][(r & 7) >> 1] = E::pack2(sc[h][r - 1], sc[h][r]);
          if (ROLE == 0 && (r & 7) == 7)                        // 8 elements done: hand one k-step of P to B
            *(USP_LDS u32x4*)(pslot + (2 * h + (r >> 3)) * 1024) = (SC || DR) ? pkg : pk[h][r >> 3];
        };
        auto chain_phase = [&](int h, int vh) {
          u32x4 f[NKT];
          auto rd = [&](int kt) {
            f[kt] = *(USP_LDS const u32x4*)(xs + h * 32 * ROWB + rd_row + (((2 * kt) ^ rd_x) * 16));
          };
          f32x16 c0 = zero16;
          if (ROLE == 1) {                                     // -delta of this half's 16 rows: the chain's C operand
            load_stats(h);
#pragma unroll
            for (int r = 0; r < 16; ++r) c0[r] = DR ? stq[r >> 2][r & 3] * dr.irs : stq[r >> 2][r & 3];
          }
#pragma unroll
          for (int kt = 0; kt < PF && kt < NKT; ++kt) rd(kt);
          if (ROLE == 1) {                                     // fetch A's P of this half early
            pin[h][0] = *(USP_LDS const u32x4*)(pslot + (2 * h) * 1024);
            pin[h][1] = *(USP_LDS const u32x4*)(pslot + (2 * h + 1) * 1024);
          }
          if (ROLE == 0 && vh >= 0) load_stats(vh);
          __builtin_amdgcn_sched_barrier(0);
#pragma unroll
          for (int kt = 0; kt < NKT; ++kt) {
            if (kt + PF < NKT) rd(kt + PF);
            sc[h] = E::mfma(f[kt], rf[kt], kt == 0 ? c0 : sc[h]);
            if (vh >= 0) {
#pragma unroll
              for (int e = kt * 16 / NKT; e < (kt + 1) * 16 / NKT; ++e) elem(vh, e);
            }
            __builtin_amdgcn_sched_barrier(0);
          }
        };
        auto grad_phase = [&](int h, int vh) {
          u32x4 xa[NGR];
          auto rd = [&](int i) {
            const int k2 = i / NDJ, dj = i % NDJ;
            USP_LDS const char* xb = xg + (2 * h + k2) * 16 * ROWB;
            const u32x2 a0 = lds_read_tr16(xb + tr_addr[dj][0]);
            const u32x2 a1 = lds_read_tr16(xb + tr_addr[dj][1]);
            xa[i] = u32x4{a0[0], a0[1], a1[0], a1[1]};
          };
#pragma unroll
          for (int i = 0; i < PF && i < NGR; ++i) rd(i);
          if (ROLE == 0 && vh >= 0) load_stats(vh);
          __builtin_amdgcn_sched_barrier(0);
#pragma unroll
          for (int i = 0; i < NGR; ++i) {
            if (i + PF < NGR) rd(i + PF);
            acc[i % NDJ] = E::mfma(xa[i], pk[h][i / NDJ], acc[i % NDJ]);
            if (vh >= 0) {
#pragma unroll
              for (int e = i * 16 / NGR; e < (i + 1) * 16 / NGR; ++e) elem(vh, e);
            }
            __builtin_amdgcn_sched_barrier(0);
          }
        };
        auto apply_mask = [&](int h) {                         // role A only: query row i sees key j iff j <= i + off
          if (CAUSAL) {
            const int d = orow - off - s0 - 4 * hi;            // one VGPR; thresholds are inline constants
#pragma unroll
            for (int r = 0; r < 16; ++r)
              if (d > 32 * h + (r & 3) + 8 * (r >> 2)) sc[h][r] = USP_NEG_INF;
          }
          if (p.win_on) {                                      // ... and only if j >= i + win_lo
            const int dl = orow - p.win_lo - s0 - 4 * hi;
#pragma unroll
            for (int r = 0; r < 16; ++r)
              if (dl < 32 * h + (r & 3) + 8 * (r >> 2)) sc[h][r] = USP_NEG_INF;
          }
          if constexpr (DOC) {                                 // ... and only if i < key_hi[j]
            const int dh = doc_hi - s0 - 4 * hi;
#pragma unroll
            for (int r = 0; r < 16; ++r)
              if (dh <= 32 * h + (r & 3) + 8 * (r >> 2)) sc[h][r] = USP_NEG_INF;
          }
          if constexpr (SPAN) {                                // ... and only if i >= key_lo[j]
            const int dlo = span_lo - s0 - 4 * hi;
#pragma unroll
            for (int r = 0; r < 16; ++r)
              if (dlo > 32 * h + (r & 3) + 8 * (r >> 2)) sc[h][r] = USP_NEG_INF;
          }
        };

        chain_phase(0, -1);
        if (ROLE == 0 && need_mask) apply_mask(0);
        chain_phase(1, 0);
        if (ROLE == 0 && need_mask) apply_mask(1);
        grad_phase(0, 1);
        grad_phase(1, -1);
      }

      if (prefetch) stage_stats(buf_n);
      buf_b = buf_a;
      buf_a = buf_n;
      dma_drain();            // this wave's DMA pieces of the staged tile have landed (usp_common.hpp)
      __syncthreads();
    }
  };
  if (role == 0) stream(std::integral_constant<int, 0>{});
  else stream(std::integral_constant<int, 1>{});

  // ---- epilogue ------------------------------------------------------------------------------------------
  if (orow < p.Sk) {
    float* o32;
    char* o16 = nullptr;
    int accf;
    const float mul_plain = role == 0 ? 1.f : p.scale;
    const float mul = DR ? mul_plain * dr.rs : mul_plain;   // dropout: 256 / t of both outputs, in fp32
    if (p.split) {
      const int64_t wo = (((int64_t)(g * p.qsplit + cut) * p.ws_rows + ws_row0 + orow) * p.Hkv + hkv) * D;
      o32 = (role == 0 ? p.ws_dv : p.ws_dk) + wo; accf = 0;
    } else if (role == 0) {
      o32 = p.dv + b * p.dv_sb + (int64_t)orow * p.dv_ss + hkv * p.dv_sh; accf = p.accum_dv;
      if (p.dv16) o16 = p.dv16 + 2 * (b * p.dv16_sb + (int64_t)orow * p.dv16_ss + hkv * p.dv16_sh);
    } else {
      o32 = p.dk + b * p.dk_sb + (int64_t)orow * p.dk_ss + hkv * p.dk_sh; accf = p.accum_dk;
      if (p.dk16) o16 = p.dk16 + 2 * (b * p.dk16_sb + (int64_t)orow * p.dk16_ss + hkv * p.dk16_sh);
    }
#pragma unroll
    for (int dj = 0; dj < NDJ; ++dj)
#pragma unroll
      for (int g4 = 0; g4 < 4; ++g4) {
        const int d0 = 32 * dj + 8 * g4 + 4 * hi;
        f32x4 v = {acc[dj][4 * g4] * mul, acc[dj][4 * g4 + 1] * mul, acc[dj][4 * g4 + 2] * mul,
                   acc[dj][4 * g4 + 3] * mul};
        if (accf) v += *(const f32x4*)(o32 + d0);
        if (o16) *(u32x2*)(o16 + 2 * d0) = u32x2{E::pack2(v[0], v[1]), E::pack2(v[2], v[3])};
        else *(f32x4*)(o32 + d0) = v;
      }
  }
  if (p_in.sched && p_in.interleave) break;   // one item per workgroup: leave room for other streams' kernels
  }  // next item
  if (p_in.sched && threadIdx.x == 0) item_queue_release(queue);
