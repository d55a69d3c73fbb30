// Body of flash_fwd_kernel / flash_fwd_softcap_kernel (usp_flash_fwd.hip): one workgroup = NWAVES x 32 query rows.
// Included as the body of the kernel templates in usp_flash_fwd.hip: the kernels without softcap (SC = false) compile exactly
// the source they were profiled with, so they keep their symbol names and machine code; the softcap kernels add
// the `if constexpr (SC)` steps, the window kernel the `if constexpr (WIN)` ones, the ALiBi kernel (usp_flash_fwd_alibi.hip) the
// `if constexpr (AL)` ones, the dropout kernel (usp_flash_fwd_dropout.hip) the `if constexpr (DR)` ones, the sink kernel
// (usp_flash_fwd_sink.hip) the `if constexpr (SINK)` one in the epilogue.  The including kernel
// defines `p_in`, KSPLIT / SC / WIN / AL / DR / SINK, sc_cl2 / sc_k2, al_slopes / al_sb / al_diag, `dr` (usp_dropout_rng.h: Dropout)
// and sink_s (fp32 (Hq,) sink logits).
// (Not a header: no include guard, no declarations of its own outside the function body.)
  using E = Elem<DT>;
  constexpr int kThreads = 64 * NWAVES;
  constexpr int kBM = 32 * NWAVES;
  constexpr int ROWB = D * 2;                 // bytes per K row
  constexpr int KBYTES = kBN * ROWB;          // one K (or V) tile
  constexpr int NKT = D / 16;                 // k-steps of K Q^T
  constexpr int NDJ = D / 32;                 // 32-wide dim tiles of O^T
  // LDS: Kbuf[0], Kbuf[1], Vbuf[0], Vbuf[1]
  constexpr int VOFF = 2 * KBYTES;

  extern __shared__ __attribute__((aligned(16))) char smem_raw[];
  USP_LDS char* smem = (USP_LDS char*)smem_raw;

  const int tid = threadIdx.x;
  const int lane = tid & 63;
  const int wave = __builtin_amdgcn_readfirstlane(tid >> 6);
  const int l31 = lane & 31;
  const int hi = lane >> 5;

  // ---- persistent workgroups: each walks a static list of (batch, head, query tile) items (ItemWalk) --
  const ItemWalk walk(p_in.n_items);
  ItemQueue queue{p_in.sched, p_in.seq_q, p_in.B * p_in.Hq, p_in.nq, p_in.Hq, kBM, CAUSAL ? 1 : 0};
  int qstate = 0;
  USP_LDS int* qslots = (USP_LDS int*)(smem + 4 * KBYTES);          // 2 ints behind the K/V buffers
  for (int pass = 0;; ++pass) {
  int w = p_in.sched ? item_queue_next(queue, qstate, qslots, pass) : walk.at(pass);
  if (w < 0) break;
  FwdParams p = p_in;
  int ks = 0;
  if constexpr (KSPLIT) {
    // the K cuts of a tile are dealt like tiles; a packed softcap launch (the only packed one of this instantiation) takes
    // its items from the queue as they come, like the plain kernel
    if (!SC || !p_in.sched) w = walk.dealt(w, p.nq * p_in.ksplit);
    ks = w % p_in.ksplit; w /= p_in.ksplit;
  } else {
    if (!p_in.sched) w = walk.dealt(w, p.nq);
  }
  const int qt_r = w % p.nq;
  int rest = w / p.nq;
  const int qt = CAUSAL ? (p.nq - 1 - qt_r) : qt_r;      // heavy (late) tiles first
  const int g = rest % p.G;
  rest /= p.G;
  const int hkv = rest % p.Hkv;
  const int b = rest / p.Hkv;
  const int h = hkv * p.G + g;

  // ---- packed variable-length batch: bind this workgroup to the rows of sequence b -------------------
  // (the host passes batch strides of 0 in this mode, so every `b * stride_b` below vanishes)
  if (p.seq_q != nullptr) {
    const int q_first = p.seq_q[2 * b], q_len = p.seq_q[2 * b + 1];
    const int k_first = p.seq_k[2 * b], k_len = p.seq_k[2 * b + 1];
    if (qt * kBM >= q_len) continue;                        // whole workgroup past the end of its sequence
    p.q += 2 * q_first * p.q_ss;
    p.k += 2 * k_first * p.k_ss;
    p.v += 2 * k_first * p.v_ss;
    if (p.out) p.out += 2 * q_first * p.o_ss;
    if (p.acc) p.acc += q_first * p.a_ss;
    p.lse += q_first;
    p.Sq = q_len;
    p.Sk = k_len > 0 ? k_len : 0;
    p.causal_off = p.Sk - q_len;
    const int half = q_len >> 1;                            // final_begin/_end count half sequences here
    p.final_begin = p.final_begin >= 2 ? q_len : p.final_begin * half;
    p.final_end = p.final_end >= 2 ? q_len : p.final_end * half;
  }

  // ---- K split: bind this workgroup to cut `ks` of the keys its query tile sees ------------------------
  // Few (batch, head, tile) items cannot fill the part, and a causal launch lasts as long as its heaviest item: the
  // tiles [0, nt) of the item are cut into ksplit equal runs, one workgroup each, by rebasing the K/V pointers, Sk
  // and the causal offset (the tile loops are untouched, as in packed mode).  Each cut writes its own normalised
  // partial (fp32) and its LSE to the workspace through the ordinary not-final epilogue; split_merge_kernel combines
  // them (and the running result, and the 16-bit emission) afterwards.
  int al_dg = 0;          // ALiBi: the bias diagonal in this item's key numbering (rebased with the K cut below)
  [[maybe_unused]] uint32_t dr_kg = 0;   // dropout: global position of this item's key 0 (rebased with the K cut below)
  bool win = false;       // left window bound active (split instantiation only)
  int win_lo = 0;         // row i sees key j only if j >= i + win_lo (in the rebased key numbering)
  if constexpr (KSPLIT) {
    win = p_in.win_on != 0;
    win_lo = p_in.win_lo;
    const int q0s = qt * kBM;
    int e = p.Sk;
    if (CAUSAL) e = usp_rows_key_end(q0s, kBM, p.Sq, e, 1, p.causal_off);
    const int nt_all = usp_tiles_holding(e, kBN);
    // = usp_first_key_tile(q0s, win, win_lo, nt_all, kBN) (usp_tile_range.h): called, every split stream changes
    int t0 = 0;           // first tile any row of this query tile sees (its first row has the smallest left bound)
    if (win) {
      const int first = q0s + win_lo;
      t0 = first > 0 ? first / kBN : 0;
      t0 = t0 < nt_all ? t0 : nt_all;
    }
    // kb, ke and the rebasing below = usp_prop_cut_keys_from and usp_cut_problem, which as struct-returning calls change the streams
    const int ntw = nt_all - t0;
    const int kb = (t0 + usp_prop_cut_tile(ntw, p_in.ksplit, ks)) * kBN;
    int ke = (ks == p_in.ksplit - 1) ? p.Sk : (t0 + usp_prop_cut_tile(ntw, p_in.ksplit, ks + 1)) * kBN;
    ke = ke < p.Sk ? ke : p.Sk;
    p.k += 2 * (int64_t)kb * p.k_ss;
    p.v += 2 * (int64_t)kb * p.v_ss;
    p.Sk = ke > kb ? ke - kb : 0;
    p.causal_off -= kb;
    win_lo -= kb;
    if constexpr (AL) al_dg = al_diag - kb;
    if constexpr (DR) dr_kg = dr.key0 + (uint32_t)kb;
    if (p_in.ksplit > 1) {
      p.acc = p_in.ws_o + (int64_t)ks * p.B * p.Sq * p.Hq * D;
      p.a_sb = (int64_t)p.Sq * p.Hq * D; p.a_ss = (int64_t)p.Hq * D; p.a_sh = D;
      p.lse = p_in.ws_lse + (int64_t)ks * p.B * p.Hq * p.Sq;
      p.lse_sb = (int64_t)p.Hq * p.Sq; p.lse_sh = p.Sq;
      p.merge_in = 0; p.final_begin = 0; p.final_end = 0; p.out_wide = 0;
    }
  }

  const int q0 = qt * kBM;
  const int qw = q0 + wave * 32;
  const int row = qw + l31;
  const int row_c = row < p.Sq ? row : p.Sq - 1;
  const int off = p.causal_off;

  // ---- KV range -----------------------------------------------------------------------------
  int blk_kv_end = p.Sk, wave_kv_end = p.Sk;
  if (CAUSAL) {
    // (wave_kv_end mirrors usp_rows_key_end: called here, the causal kernels' streams change)
    const int wav_last = (qw + 32 < p.Sq ? qw + 32 : p.Sq) - 1;
    blk_kv_end = usp_rows_key_end(q0, kBM, p.Sq, p.Sk, 1, off);
    wave_kv_end = wav_last + off + 1 < p.Sk ? wav_last + off + 1 : p.Sk;
  }
  if (qw >= p.Sq) wave_kv_end = 0;
  const int nt = blk_kv_end > 0 ? (blk_kv_end + kBN - 1) / kBN : 0;     // = usp_tiles_holding: called, the softcap streams change
  // leading tiles that need neither a causal nor a ragged mask for this wave (= usp_unmasked_tiles: called, the causal split
  // streams change)
  int n_full = p.Sk / kBN;
  if (CAUSAL) {
    const int lim = qw + off + 1;                         // keys < lim are visible to EVERY row of the wave
    const int nf = lim > 0 ? lim / kBN : 0;
    n_full = nf < n_full ? nf : n_full;
  }
  if (qw + 32 > p.Sq) n_full = 0;                         // ragged / inactive waves take the generic loop
  if constexpr (KSPLIT && !WIN) { if (win) n_full = 0; }  // a left window bound outside the window kernel: every tile through the masked loop
  if constexpr (SC) n_full = 0;                           // softcap: every tile through the generic loop
  if constexpr (AL) n_full = 0;                           // ALiBi: likewise (the bias step lives there)
  if constexpr (DR) n_full = 0;                           // dropout: likewise (the keep step lives in the generic softmax)
  if (n_full > nt) n_full = nt;
  // WIN (flash_fwd_window_kernel: every launch has a left bound): the tiles are walked in the ROTATED order [rot, nt) then
  // [0, rot) -- online softmax does not care -- where rot is the workgroup-uniform number of leading tiles the left bound
  // cuts for ANY wave of the workgroup (kt0 < last row + win_lo).  Walk index j holds tile tmap(j); the tiles [rot, n_full) of
  // the unrotated count are then cut by no bound for this wave and take the pipelined main loop as walk indices
  // [0, n_full - rot); the generic tail takes the diagonal tiles and then the `rot` leading ones.  Every wave walks the same
  // order (the barriers and the K/V buffers are per walk index), only n_full differs per wave, as ever.
  // (rot and the n_full behind it = usp_window_rotation, which as one call changes every window stream.)
  int rot = 0;
  if constexpr (WIN) {
    rot = usp_tiles_holding(q0 + kBM - 1 + win_lo, kBN);
    if (rot >= nt) { rot = 0; n_full = 0; }               // the left bound cuts every tile
    else n_full = n_full > rot ? n_full - rot : 0;
  }
  auto tmap = [&](int j) {
    if constexpr (WIN) { const int t = j + rot; return t < nt ? t : t - nt; }
    else return j;
  };
  // does this wave have a visible key in the tile that starts at key kt0?  (WIN only: also skips tiles wholly left of the wave's window)
  // = usp_key_tile_live (kt0 + kBN - 1 >= qw + win_lo), which changes the window streams when called
  auto tile_live = [&](int kt0) { return kt0 < wave_kv_end && kt0 + kBN > qw + win_lo; };

  // ---- Q fragments (B operand: lane holds Q[row][16t + 8hi .. +7]) ---------------------------
  u32x4 qf[NKT];
  {
    const char* qp = p.q + 2 * (b * p.q_sb + (int64_t)row_c * p.q_ss + h * p.q_sh) + 16 * hi;
#pragma unroll
    for (int t = 0; t < NKT; ++t) qf[t] = *(const u32x4*)(qp + 32 * t);
  }

  // ---- staging: LDS-DMA (buffer_load ... lds): no staging registers, no ds_write ---------------------
  // One wave-instruction fills 1 KiB of LDS linearly (wave-uniform base + lane*16):
  //   K tile (row-major, slot swizzle): 1024/ROWB whole rows; the lane landing on physical slot p of row
  //     r fetches logical slot p ^ swz(r) of that row (swizzle applied on the SOURCE side);
  //   V tile ([4 keys][32 dims] blocks of 256 B): 4 blocks; lane l fetches key 4*kb + (l%16)/4,
  //     dims 32*dj + 8*(l%4) .. +7 of block (kb, dj) = (4*piece + l/16) / NDJ, % NDJ.
  // The tile offset is folded into the 64-bit descriptor base (no 32-bit overflow at any sequence
  // length); num_records makes rows >= Sk read as 0 (they are masked).  hipcc drains the DMA
  // (vmcnt(0)) in front of the s_barrier that ends the iteration.
  const char* kbase = p.k + 2 * (b * p.k_sb + hkv * p.k_sh);
  const char* vbase = p.v + 2 * (b * p.v_sb + hkv * p.v_sh);
  constexpr int NW = kThreads / 64;
  constexpr int CHUNKS = KBYTES / 1024;           // 1 KiB pieces per tile
  constexpr int CPW = (CHUNKS + NW - 1) / NW;     // pieces per wave per tile
  int k_voff[CPW], v_voff[CPW];
#pragma unroll
  for (int i = 0; i < CPW; ++i) {
    const int cidx = wave + NW * i;
    {
      const int r = cidx * (1024 / ROWB) + lane / (D / 8);
      const int c8 = (lane % (D / 8)) ^ KSwz<D>::of(r);
      k_voff[i] = r * (int)p.k_ss * 2 + c8 * 16;
    }
    {
      const int blk = 4 * cidx + (lane >> 4);
      const int kb = blk / NDJ, dj = blk % NDJ;
      const int key = 4 * kb + ((lane & 15) >> 2), d = 32 * dj + 8 * (lane & 3);
      v_voff[i] = key * (int)p.v_ss * 2 + d * 2;
    }
  }
  auto tile_rsrc = [&](const char* base, int64_t ss, int tile) {
    const int64_t toff = (int64_t)tile * kBN * ss * 2;
    int64_t rem = ((int64_t)(p.Sk - 1 - tile * kBN) * ss + D) * 2;
    rem = rem < 0 ? 0 : (rem > 0xffffffffLL ? 0xffffffffLL : rem);
    return __builtin_amdgcn_make_buffer_rsrc((void*)(base + toff), 0, (int)(uint32_t)rem, 0x00020000);
  };
  // piece i (of CPW) of K tile `tile` -> Kbuf[buf]; likewise V -> Vbuf[buf]
  auto dma_k = [&](int tile, int buf) {
    const auto rs_ = tile_rsrc(kbase, p.k_ss, tile);
#pragma unroll
    for (int i = 0; i < CPW; ++i)
      if (CHUNKS % NW == 0 || wave + NW * i < CHUNKS)
        lds_dma16(rs_, smem + buf * KBYTES + (wave + NW * i) * 1024, k_voff[i]);
  };
  auto dma_v = [&](int tile, int buf) {
    const auto rs_ = tile_rsrc(vbase, p.v_ss, tile);
#pragma unroll
    for (int i = 0; i < CPW; ++i)
      if (CHUNKS % NW == 0 || wave + NW * i < CHUNKS)
        lds_dma16(rs_, smem + VOFF + buf * KBYTES + (wave + NW * i) * 1024, v_voff[i]);
  };

  // ---- per-lane LDS read bases -----------------------------------------------------------------
  const int k_rd_row = l31 * ROWB;
  const int k_rd_x = hi ^ KSwz<D>::of(l31);          // (2t + hi) ^ s == (2t) ^ (hi ^ s)
  const int v_rd = VOFF + hi * NDJ * 256 + ((lane & 15) >> 2) * 64 + ((lane >> 4) & 1) * 32 +
                   (lane & 3) * 8;

  // ---- accumulators ----------------------------------------------------------------------------
  f32x16 o[NDJ];
#pragma unroll
  for (int dj = 0; dj < NDJ; ++dj)
#pragma unroll
    for (int r = 0; r < 16; ++r) o[dj][r] = 0.f;
  float m_run = USP_NEG_INF;   // running row max, raw score units
  float l_run = 0.f;           // this lane's share of the row sum
  const float c = (SC || AL) ? 1.f : p.scale_log2;   // softcap, ALiBi: the scores arrive capped / biased and in exp2 units
  // ALiBi: -slope * log2(e) of this item's (batch, head), read per item: the persistent walk and the K cuts of a tile change it
  float al_ns2 = 0.f;
  if constexpr (AL) al_ns2 = -kLog2e * al_slopes[b * al_sb + h];
  [[maybe_unused]] int dr_kt0 = 0;   // dropout: first key of the tile the generic softmax works on

  // S^T = K Q^T for the K tile in Kbuf[kbuf]
  auto qk = [&](int kbuf, f32x16& s0, f32x16& s1) {
    USP_LDS const char* kb = smem + kbuf * KBYTES;
#pragma unroll
    for (int r = 0; r < 16; ++r) { s0[r] = 0.f; s1[r] = 0.f; }
#pragma unroll
    for (int kt = 0; kt < NKT; ++kt) {
      const int slot = ((2 * kt) ^ k_rd_x) * 16;
      u32x4 ka = *(USP_LDS const u32x4*)(kb + k_rd_row + slot);
      u32x4 kc = *(USP_LDS const u32x4*)(kb + 32 * ROWB + k_rd_row + slot);
      s0 = E::mfma(ka, qf[kt], s0);
      s1 = E::mfma(kc, qf[kt], s1);
    }
  };
  // online softmax of one 64-key tile held in (s0, s1); rescales o, returns P packed for the PV MFMAs
  auto softmax = [&](f32x16& s0, f32x16& s1, u32x4 (&pf)[4]) {
    float mt = s0[0];
#pragma unroll
    for (int r = 1; r < 16; ++r) mt = fmaxf(mt, s0[r]);
#pragma unroll
    for (int r = 0; r < 16; ++r) mt = fmaxf(mt, s1[r]);
    mt = xhalf_max(mt);
    const float m_new = fmaxf(m_run, mt);
    const float m_use = (m_new == USP_NEG_INF) ? 0.f : m_new;
    const float mc = m_use * c;
    const float alpha = fast_exp2(m_run * c - mc);
    m_run = m_new;
    float rs = 0.f;
#pragma unroll
    for (int r = 0; r < 16; ++r) {
      s0[r] = fast_exp2(__builtin_fmaf(s0[r], c, -mc));
      s1[r] = fast_exp2(__builtin_fmaf(s1[r], c, -mc));
      rs += s0[r] + s1[r];
    }
    l_run = l_run * alpha + rs;
#pragma unroll
    for (int dj = 0; dj < NDJ; ++dj)
#pragma unroll
      for (int r = 0; r < 16; ++r) o[dj][r] *= alpha;
    if constexpr (DR) {
      // dropout: the row sum above took the un-dropped P (the LSE is that of the un-dropped scores); the P packed for the PV
      // MFMAs is zeroed where dropped, and 256 / t goes into the epilogue's weight in fp32.  The lane's row is fixed, its keys
      // are the register dimension (usp_dropout_rng.h).
      uint32_t kw[8];
      usp_dropout_tile_words<true>(dr.k0, dr.k1, (uint32_t)b, dr.head0 + (uint32_t)h, (dr.row0 + (uint32_t)row) >> 2,
                                   ((dr_kg + (uint32_t)dr_kt0) >> 2) + (uint32_t)hi, lane, kw);
#pragma unroll
      for (int r = 0; r < 16; ++r) {
        if (!usp_dropout_keep(kw[r >> 2], r & 3, dr.t)) s0[r] = 0.f;
        if (!usp_dropout_keep(kw[4 + (r >> 2)], r & 3, dr.t)) s1[r] = 0.f;
      }
    }
    // P (B operand of V^T P^T): k-step ks = 2*n32 + (r>>3), element e = r & 7
#pragma unroll
    for (int j = 0; j < 4; ++j) {
      pf[0][j] = E::pack2(s0[2 * j], s0[2 * j + 1]);
      pf[1][j] = E::pack2(s0[8 + 2 * j], s0[8 + 2 * j + 1]);
      pf[2][j] = E::pack2(s1[2 * j], s1[2 * j + 1]);
      pf[3][j] = E::pack2(s1[8 + 2 * j], s1[8 + 2 * j + 1]);
    }
  };
  // O^T += V^T P^T for the V tile in Vbuf[vbuf]
  auto pv = [&](int vbuf, const u32x4 (&pf)[4]) {
    USP_LDS const char* vb = smem + vbuf * KBYTES + v_rd;
#pragma unroll
    for (int ks = 0; ks < 4; ++ks) {
#pragma unroll
      for (int dj = 0; dj < NDJ; ++dj) {
        USP_LDS const char* vp = vb + (4 * ks * NDJ + dj) * 256;
        u32x2 v0 = lds_read_tr16(vp);
        u32x2 v1 = lds_read_tr16(vp + 2 * NDJ * 256);
        u32x4 va = {v0[0], v0[1], v1[0], v1[1]};
        o[dj] = E::mfma(va, pf[ks], o[dj]);
      }
    }
  };
  auto mask = [&](int kt0, f32x16& s0, f32x16& s1) {
    int klim = p.Sk - 1;
    if (CAUSAL) klim = row + off < klim ? row + off : klim;
    const int kb0 = kt0 + 4 * hi;
#pragma unroll
    for (int r = 0; r < 16; ++r) {
      const int key = kb0 + (r & 3) + 8 * (r >> 2);
      if (key > klim) s0[r] = USP_NEG_INF;
      if (key + 32 > klim) s1[r] = USP_NEG_INF;
    }
    if constexpr (KSPLIT) {
      if (win) {
        const int klo = row + win_lo;
#pragma unroll
        for (int r = 0; r < 16; ++r) {
          const int key = kb0 + (r & 3) + 8 * (r >> 2);
          if (key < klo) s0[r] = USP_NEG_INF;
          if (key + 32 < klo) s1[r] = USP_NEG_INF;
        }
      }
    }
  };

  // ---- prologue: K(0), V(0), K(1) resident; S(0) computed ------------------------------------------
  f32x16 sa, sb;          // S^T of the tile the softmax works on next
#pragma unroll
  for (int r = 0; r < 16; ++r) { sa[r] = 0.f; sb[r] = 0.f; }
  if (nt > 0) {
    dma_k(tmap(0), 0); dma_v(tmap(0), 0);
    if (nt > 1) dma_k(tmap(1), 1);
  }
  dma_drain();
  __syncthreads();
  if constexpr (WIN) { if (nt > 0 && tile_live(tmap(0) * kBN)) qk(0, sa, sb); }
  else { if (nt > 0 && wave_kv_end > 0) qk(0, sa, sb); }
  // K(0) must have been read by EVERY wave before the first loop iteration refills Kbuf[0] with K(2): a
  // wave that skips qk(0) (no valid rows) reaches that DMA at once, and a mostly out-of-range K(2) tile
  // (short sequences) lands immediately -- observed as rare small errors on ragged shapes.
  __syncthreads();

  // ---- main loop over unmasked tiles, hand-pinned software pipeline --------------------------------
  // Per iteration j (reference max m_run already decided for tile j):
  //   phase A: 2*NKT MFMAs of S(j+1) = K(j+1) Q^T, each followed by a slice of the exp2 / row-sum /
  //            pack work of tile j (24 of its 32 elements), K fragments prefetched two k-steps ahead;
  //   phase B: 4*NDJ MFMAs of O^T += V(j)^T P(j)^T, the first half each followed by one of the 8
  //            remaining exp2 elements, all of them by a slice of the row-max chain of S(j+1),
  //            V fragments prefetched two MFMAs ahead;
  //   decision: defer-max -- O and l are rescaled only when some row's max grew by more than 2^kThr
  //            (wave-uniform, rare); otherwise the old reference max is kept (P <= 2^kThr).
  // sched_barrier(0) pins the order: hipcc otherwise emits all MFMAs, then all VALU (measured).
  // The two S register sets ping-pong (no copies); the first MFMA of each chain takes C = 0.
  // K/V tiles are fetched with buffer loads: per-thread offsets are loop invariant, the tile offset
  // is a scalar (no 64-bit VALU address math in the loop).
  constexpr float kThr = 8.f;
  constexpr int NA = 2 * NKT, NB = 4 * NDJ;
  int j = 0;
  const int n_main = n_full < nt - 1 ? n_full : nt - 1;    // j + 1 < nt holds inside: no branches
  // m_thr = m_run + kThr / c: a tile whose scores all stay below it keeps the reference max.  Every lane tests the
  // maximum of ITS 32 scores of the row (the other half-wave's lane tests the other 32), so the common path needs no
  // exchange between the half-waves; the (rare, wave-uniform) rescale does it.
  const float thr_raw = kThr / c;
  float m_thr = USP_NEG_INF;
  float nmc = 0.f;             // -(reference max * c) of the pipelined loop, 0 while the reference is still -inf
  auto rescale = [&](float mt_lane) {
    asm volatile("; rescale (rare)" ::: "memory");          // keeps hipcc from if-converting the branch
    const float m_new = fmaxf(m_run, xhalf_max(mt_lane));
    const float m_use = (m_new == USP_NEG_INF) ? 0.f : m_new;
    const float alpha = fast_exp2(m_run * c - m_use * c);
    m_run = m_new;
    m_thr = m_new + thr_raw;
    nmc = -(m_use * c);
    l_run *= alpha;
#pragma unroll
    for (int dj = 0; dj < NDJ; ++dj)
#pragma unroll
      for (int r = 0; r < 16; ++r) o[dj][r] *= alpha;
  };
  // one pipelined iteration: softmax + PV of tile jj (scores in ca/cb), scores of tile jj+1 into na/nb
  auto iter = [&](int jj, f32x16& ca, f32x16& cb, f32x16& na, f32x16& nb) {
    const int jk = jj + 2 < nt ? jj + 2 : nt - 1;           // clamped prefetch (redundant load at the end)
    dma_k(tmap(jk), jj & 1);            // Kbuf[jj&1] held K(jj): last read in the previous iteration
    dma_v(tmap(jj + 1), (jj + 1) & 1);  // Vbuf[(jj+1)&1] held V(jj-1): last read in the previous iteration
    // ---------------- phase A ----------------
    USP_LDS const char* kb = smem + ((jj + 1) & 1) * KBYTES + k_rd_row;
    u32x4 ka[NKT], kc[NKT];
    auto rd_k = [&](int kt) {
      const int slot = ((2 * kt) ^ k_rd_x) * 16;
      ka[kt] = *(USP_LDS const u32x4*)(kb + slot);
      kc[kt] = *(USP_LDS const u32x4*)(kb + 32 * ROWB + slot);
    };
    constexpr int PF = 2;                                       // LDS fragment prefetch distance (k-steps / MFMAs)
#pragma unroll
    for (int t = 0; t < PF && t < NKT; ++t) rd_k(t);
    float rs = 0.f;
    u32x4 pf[4];
    // element e of the tile's 32 scores: e < 16 -> ca[e], else cb[e - 16]
    auto exp_elem = [&](int e) {
      // The consumers of an exp2 result run ONE ELEMENT LATE (the row-sum add of element e-1 and the pack of the pair
      // (e-2, e-1) are issued with element e): nothing waits for the transcendental it was just issued behind.
      auto P = [&](int i) -> float { return i < 16 ? ca[i] : cb[i - 16]; };
      if (e < 16) ca[e] = fast_exp2(__builtin_fmaf(ca[e], c, nmc));
      else cb[e - 16] = fast_exp2(__builtin_fmaf(cb[e - 16], c, nmc));
      if (e == 1) rs = P(0);
      else if (e > 1) rs += P(e - 1);
      if (e >= 2 && (e & 1) == 0) {                         // pair (e-2, e-1) complete -> pack
        const int r = (e - 2) & 15;
        if (e - 2 < 16) pf[r >> 3][(r & 7) >> 1] = E::pack2(ca[r], ca[r + 1]);
        else pf[2 + (r >> 3)][(r & 7) >> 1] = E::pack2(cb[r], cb[r + 1]);
      }
      if (e == 31) {
        rs += cb[15];
        pf[3][3] = E::pack2(cb[14], cb[15]);
      }
    };
    const f32x16 zero = {0.f, 0.f, 0.f, 0.f, 0.f, 0.f, 0.f, 0.f, 0.f, 0.f, 0.f, 0.f, 0.f, 0.f, 0.f, 0.f};
    USP_LDS const char* vb = smem + (jj & 1) * KBYTES + v_rd;
    u32x4 va[NB];
    auto rd_v = [&](int i) {                                  // i = ks * NDJ + dj
      const int ks = i / NDJ, dj = i % NDJ;
      USP_LDS const char* vp = vb + (4 * ks * NDJ + dj) * 256;
      const u32x2 v0 = lds_read_tr16(vp);
      const u32x2 v1 = lds_read_tr16(vp + 2 * NDJ * 256);
      va[i] = u32x4{v0[0], v0[1], v1[0], v1[1]};
    };
    // The first MFMA of the phase waits for the K fragments read just above (K(jj+1) is only guaranteed behind the
    // barrier): the first slice of exp work goes IN FRONT of it, every later slice behind the MFMA before it; the V
    // fragments of phase B's first MFMAs are read behind phase A's last ones (V(jj) has been resident since the
    // previous barrier), so phase B starts without an LDS round trip.
    constexpr int LEAD = 24 / NA;        // exp elements issued in front of the first MFMA of phase A
#pragma unroll
    for (int e = 0; e < LEAD; ++e) exp_elem(e);
    __builtin_amdgcn_sched_barrier(0);
#pragma unroll
    for (int sl = 0; sl < NA; ++sl) {
      const int kt = sl >> 1;
      if ((sl & 1) == 0) {
        if (kt + PF < NKT) rd_k(kt + PF);
        na = E::mfma(ka[kt], qf[kt], kt == 0 ? zero : na);
      } else {
        nb = E::mfma(kc[kt], qf[kt], kt == 0 ? zero : nb);
      }
      if (sl + 1 < NA) {
#pragma unroll
        for (int e = LEAD + sl * (24 - LEAD) / (NA - 1); e < LEAD + (sl + 1) * (24 - LEAD) / (NA - 1); ++e) exp_elem(e);
      }
      if (sl >= NA - PF && sl - (NA - PF) < NB) rd_v(sl - (NA - PF));
      __builtin_amdgcn_sched_barrier(0);
    }
    // ---------------- phase B ----------------
    float mt = USP_NEG_INF;
    bool keep = true;
#pragma unroll
    for (int i = 0; i < NB; ++i) {
      if (i + PF < NB) rd_v(i + PF);
      o[i % NDJ] = E::mfma(va[i], pf[i / NDJ], o[i % NDJ]);
      if (i < NB / 2) {
#pragma unroll
        for (int e = 24 + i * 16 / NB; e < 24 + (i + 1) * 16 / NB; ++e) exp_elem(e);
        if (i == NB / 2 - 1) l_run += rs;
      } else {                                                // row-max chain of S(jj+1), second half of the phase
#pragma unroll
        for (int e = (i - NB / 2) * 64 / NB; e < (i - NB / 2 + 1) * 64 / NB; ++e)
          mt = fmaxf(mt, e < 16 ? na[e] : nb[e - 16]);
        if (i == NB - 1) keep = __all(mt <= m_thr);           // decided behind the last MFMA, not after it
      }
      __builtin_amdgcn_sched_barrier(0);
    }
    // S(n_main) is the first tile of the generic tail: its scores are still UNMASKED here, and the tail's softmax takes its
    // row max itself, behind the mask.  Raising the reference to the score of a key the row must not see costs no
    // correctness but, in fp16, the precision of every visible P (a masked score 20 above the visible ones leaves them
    // subnormal: `out` off by 5e-3 with lse exact; tests/test_gpu_needle.py, wave4-d64-fp16) -- so that tile decides nothing.
    if (!keep && jj + 1 < n_main) rescale(mt);
    dma_drain();                 // this wave's pieces of K(jj+2), V(jj+1) have landed ...
    __syncthreads();             // ... and so have everybody else's
  };

  if (!SC && !AL && !DR && n_main > 0) {
    float mt = sa[0];
#pragma unroll
    for (int r = 1; r < 16; ++r) mt = fmaxf(mt, sa[r]);
#pragma unroll
    for (int r = 0; r < 16; ++r) mt = fmaxf(mt, sb[r]);
    if (!__all(mt <= m_thr)) rescale(mt);
    f32x16 ta, tb;
    for (; j + 1 < n_main; j += 2) {
      iter(j, sa, sb, ta, tb);
      iter(j + 1, ta, tb, sa, sb);
    }
    if (j < n_main) {
      iter(j, sa, sb, ta, tb);
      sa = ta; sb = tb;
      ++j;
    }
  }
  // ---- generic tail: masked and/or inactive tiles ---------------------------------------------------
  for (; j < nt; ++j) {
    const int kt0 = tmap(j) * kBN;
    if (j + 2 < nt) dma_k(tmap(j + 2), j & 1);
    if (j + 1 < nt) dma_v(tmap(j + 1), (j + 1) & 1);
    f32x16 na, nb;
#pragma unroll
    for (int r = 0; r < 16; ++r) { na[r] = 0.f; nb[r] = 0.f; }
    bool live;
    if constexpr (WIN) {
      if (j + 1 < nt && tile_live(tmap(j + 1) * kBN)) qk((j + 1) & 1, na, nb);
      live = tile_live(kt0);
    } else {
      if (j + 1 < nt && kt0 + kBN < wave_kv_end) qk((j + 1) & 1, na, nb);
      live = kt0 < wave_kv_end;
    }
    if (live) {
      // = usp_key_tile_masked (usp_tile_range.h): called, the streams change
      bool need_mask = (kt0 + kBN > p.Sk) || (CAUSAL && kt0 + kBN - 1 > qw + off);
      if constexpr (KSPLIT) need_mask = need_mask || (win && kt0 < qw + 31 + win_lo);
      if constexpr (SC) {
#pragma unroll
        for (int r = 0; r < 16; ++r) {
          sa[r] = sc_cl2 * softcap_tanh(sa[r], sc_k2);
          sb[r] = sc_cl2 * softcap_tanh(sb[r], sc_k2);
        }
      }
      if constexpr (AL) {
        // S2 = raw * scale_log2 - slope_log2 * |row + diag - key|: the distance is an integer, converted once; before the
        // mask (a masked score stays -inf).  Register r holds key kt0 + 4 hi + (r & 3) + 8 (r >> 2), sb the key 32 further.
        const int d0 = row + al_dg - kt0 - 4 * hi;
#pragma unroll
        for (int r = 0; r < 16; ++r) {
          const int da = d0 - ((r & 3) + 8 * (r >> 2)), db = da - 32;
          sa[r] = __builtin_fmaf(sa[r], p.scale_log2, al_ns2 * (float)(da < 0 ? -da : da));
          sb[r] = __builtin_fmaf(sb[r], p.scale_log2, al_ns2 * (float)(db < 0 ? -db : db));
        }
      }
      if (need_mask) mask(kt0, sa, sb);
      if constexpr (DR) dr_kt0 = kt0;
      u32x4 pf[4];
      softmax(sa, sb, pf);
      pv(j & 1, pf);
    }
    sa = na; sb = nb;
    dma_drain();
    __syncthreads();
  }

  // ---- epilogue: normalise, merge with the running result, store -------------------------------
  const float l_tot = xhalf_sum(l_run);
  const bool empty = !(l_tot > 0.f);
  float inv = empty ? 0.f : 1.f / l_tot;
  if constexpr (DR) inv *= dr.rs;     // dropout: the kept terms are rescaled by 256 / t, in fp32
  const float blk_lse = empty ? USP_NEG_INF : (m_run * c + log2f(l_tot)) * kLn2;
  float w_blk = inv, w_old = 0.f, new_lse = blk_lse;
  float* lse_p = p.lse + b * p.lse_sb + h * p.lse_sh + row;
  const bool valid = row < p.Sq;
  const bool fin = row >= p.final_begin && row < p.final_end;
  // single-pass call whose 32 rows are all final and 16-byte aligned: straight-line widened stores
  const bool wide = !p.merge_in && p.out_wide && __all(!valid || fin);
  if (valid) {
    if (p.merge_in) {
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
    if constexpr (SINK) {
      // The sink of head h joins the row's denominator and carries no value: the block result merged with (o = 0, lse = s_h),
      // the arithmetic of the merge above with old = s_h and no acc to read.  Once per row: on the launch that opens the rows'
      // state, and of a K-split launch on cut 0 alone (p.merge_in is 0 for EVERY cut, so both are read from p_in and ks) --
      // split_merge_kernel then combines partials of which one holds it.  An empty row, or an empty cut 0, gives (0, s_h):
      // mx = s_h, e_old = 1, e_blk = 0, log2f(1) = 0.
      bool carries = !p_in.merge_in;
      if constexpr (KSPLIT) carries = carries && (p_in.ksplit <= 1 || ks == 0);
      if (carries) {
        const float old = sink_s[h];
        const float mx = fmaxf(old, blk_lse);
        if (mx == USP_NEG_INF) {
          new_lse = USP_NEG_INF; w_blk = 0.f;
        } else {
          const float e_old = exp2f((old - mx) * kLog2e);
          const float e_blk = exp2f((blk_lse - mx) * kLog2e);
          const float sum = e_old + e_blk;
          new_lse = mx + log2f(sum) * kLn2;
          w_blk = e_blk / sum * inv;
        }
      }
    }
    if (hi == 0) *lse_p = new_lse;
    const int64_t arow = b * p.a_sb + (int64_t)row * p.a_ss + h * p.a_sh;
    const int64_t orow = b * p.o_sb + (int64_t)row * p.o_ss + h * p.o_sh;
    if (wide) {
      // Each row is split across the two half-waves in 8-byte pieces; one v_permlane32_swap per dword
      // regroups two adjacent pieces into 16 contiguous bytes per lane: 2*NDJ dwordx4 stores instead of
      // 4*NDJ dwordx2 (the store tail is issue-bound; the fp32 path already stores 16 bytes per lane).
      char* op = p.out + 2 * orow;
#pragma unroll
      for (int dj = 0; dj < NDJ; ++dj)
#pragma unroll
        for (int g2 = 0; g2 < 2; ++g2) {
          const int r0 = 8 * g2;                 // regs r0..r0+3: column group 2*g2, r0+4..r0+7: group 2*g2+1
          uint32_t ax = E::pack2(o[dj][r0] * w_blk, o[dj][r0 + 1] * w_blk);
          uint32_t ay = E::pack2(o[dj][r0 + 2] * w_blk, o[dj][r0 + 3] * w_blk);
          uint32_t bx = E::pack2(o[dj][r0 + 4] * w_blk, o[dj][r0 + 5] * w_blk);
          uint32_t by = E::pack2(o[dj][r0 + 6] * w_blk, o[dj][r0 + 7] * w_blk);
          const auto sx = __builtin_amdgcn_permlane32_swap(ax, bx, false, false);
          const auto sy = __builtin_amdgcn_permlane32_swap(ay, by, false, false);
          *(u32x4*)(op + 2 * (32 * dj + 16 * g2 + 8 * hi)) = u32x4{sx[0], sy[0], sx[1], sy[1]};
        }
    } else {
#pragma unroll
      for (int dj = 0; dj < NDJ; ++dj) {
#pragma unroll
        for (int g4 = 0; g4 < 4; ++g4) {
          const int d0 = 32 * dj + 8 * g4 + 4 * hi;
          f32x4 val = {o[dj][4 * g4] * w_blk, o[dj][4 * g4 + 1] * w_blk, o[dj][4 * g4 + 2] * w_blk,
                       o[dj][4 * g4 + 3] * w_blk};
          if (p.merge_in) {
            const f32x4 a = *(const f32x4*)(p.acc + arow + d0);
            val += a * w_old;
          }
          if (fin) {
            u32x2 pk = {E::pack2(val[0], val[1]), E::pack2(val[2], val[3])};
            *(u32x2*)(p.out + 2 * (orow + d0)) = pk;
          } else {
            *(f32x4*)(p.acc + arow + d0) = val;
          }
        }
      }
    }
  }
  if (p_in.sched && p_in.interleave) break;   // one item per workgroup: leave room for other streams' kernels
  }  // next item
  if (p_in.sched && threadIdx.x == 0) item_queue_release(queue);
