// Blockwise flash-attention backward for gfx950, dQ launch, ONE WAVE PER SIMD.  C ABI: usp_flash_bwd (include/usp_hip.h);
// replaces -- together with the dK/dV launch of usp_flash_bwd64.hip -- the reference's `bwd-only` block kernel
// (yunchang/kernels/attention.py:205-250).
//
// workgroup = 4 waves = 256 query rows of one (batch, head); a wave owns 64 rows (two 32-row query blocks) and its SIMD's
// whole register file:
//   a[0:127]   dQ^T accumulators, 2 query blocks x 4 dim tiles                       (asm MFMAs, "+a")
//   a[128:191] Q fragments, a[192:255] dO fragments of the wave's rows: B operands of the S^T / dP^T chains, never copied
//   v[...]     S^T -> P^T and dP^T -> dS^T of the streamed 64-key tile (2 x 64), packed dS^T (32), LDS fragments
// K / V tiles stream through LDS (LDS-DMA, two buffers each).  Everything is computed TRANSPOSED (keys down the rows of an
// accumulator tile, queries across the lanes), so that the row statistics lse / delta are ONE value per lane and query block
// and P, dS leave the accumulator layout as MFMA B operands without any cross-lane move (usp_flash_fwd64.hip).
// A tile is 96 MFMA slots per wave, in six blocks of 16, query block major, so that a block's elements can start while the
// other query block's MFMAs run:
//   B1  S^T[0] = K Q0^T    | B2  S^T[1] = K Q1^T    | B3  dP^T[0] = V dO0^T  | B4  dP^T[1] = V dO1^T
//   B5  dQ^T[0] += K^T dS^T[0]                      | B6  dQ^T[1] += K^T dS^T[1]
// Every LDS fragment is read once and serves two MFMAs (the second block of a pair takes it from the registers): 16 + 16
// row reads (ds_read_b128) and 32 transposed reads (ds_read_b64_tr_b16) per tile = 0.67 per MFMA.  The dP^T chains START FROM
// -delta (an accumulator tuple per query block, built once per item, the C operand of a chain's first MFMA), so the element
// streams are
//   X[qb]: P = exp2(S c - lse)        Y[qb]: dS = P * chain, packed to 16 bits
// 1.9 VALU + 0.67 transcendental issues per MFMA.  Where they ride is a table by GAP of the tile (q64_gap_x / q64_gap_y,
// checked at compile time against the chains they read and the k-step of dQ that takes them), levelled so that no block
// carries more than its MFMAs cover: X[0] over B2 and the head of B3, X[1] over B3 and B4, Y[0] over B4 and the head of B5,
// Y[1] from the middle of B5 into B6.  The next tile's staging: the descriptors (dma_open, scalar work) under the LDS round
// trip of B1's first fragments, the 8 LDS-DMA pieces in every other gap of B1 -- back to back they cost 0.8 % of the launch,
// in B4 / B5 (a block before the drain) 0.8 % more on short key ranges (profiles/dq64_levelled.txt).
// MFMAs are inline asm (usp_mfma64.hpp); tools/mfma_hazards.py checks the emitted stream.
#ifdef USP_Q64_TIMING
#define USP_TIMING
#endif
#include "usp_bwd_params.hpp"
#include "usp_host.hpp"
#include "usp_mfma64.hpp"

namespace usp {

#ifdef USP_TIMING
USP_DEV uint32_t tm_stamp() {           // low half of the clock, fenced against the instruction scheduler
  __builtin_amdgcn_sched_barrier(0);
  const uint32_t t = (uint32_t)__builtin_amdgcn_s_memtime();
  __builtin_amdgcn_sched_barrier(0);
  return t;
}
#endif

#ifndef USP_Q64_PF
#define USP_Q64_PF 3
#endif
constexpr int kQ64_PF = USP_Q64_PF;     // LDS fragments are read this many fragments ahead of the first MFMA that takes them
// Where the next tile's staging rides, in gaps of the tile (0 .. 95; block b is gaps 16 b .. 16 b + 15): dma_open in gap
// OPEN, piece n (K 0-3, V 4-7) in gap P0 + n * PS.
#ifndef USP_Q64_DMA_OPEN
#define USP_Q64_DMA_OPEN -1
#endif
#ifndef USP_Q64_DMA_P0
#define USP_Q64_DMA_P0 1
#endif
#ifndef USP_Q64_DMA_PS
#define USP_Q64_DMA_PS 2
#endif
// The element streams by gap of the tile.  e = 32 qb + n counts a stream's 64 elements in the order the dQ k-steps take them.
// X (12 issue cycles an element): XB2 elements ride in B2, XB4 in B4, the rest in B3, evenly over the block's 16 gaps.
// Y (6): the first YB4 elements of Y[0] in B4, then two a gap from B5 on, Y[1] behind Y[0].
#ifndef USP_Q64_XB2
#define USP_Q64_XB2 28
#endif
#ifndef USP_Q64_XB4
#define USP_Q64_XB4 20
#endif
#ifndef USP_Q64_YB4
#define USP_Q64_YB4 16
#endif
constexpr int kQ64_XB2 = USP_Q64_XB2, kQ64_XB4 = USP_Q64_XB4, kQ64_XB3 = 64 - kQ64_XB2 - kQ64_XB4, kQ64_YB4 = USP_Q64_YB4;
static_assert(kQ64_XB2 >= 1 && kQ64_XB3 >= 1 && kQ64_XB4 >= 0 && kQ64_YB4 >= 1 && kQ64_YB4 <= 32 && kQ64_YB4 % 2 == 0, "element streams");
constexpr int q64_gap_x(int e) {
  if (e < kQ64_XB2) return 16 + e * 16 / kQ64_XB2;
  if (e < kQ64_XB2 + kQ64_XB3) return 32 + (e - kQ64_XB2) * 16 / kQ64_XB3;
  return 48 + (e - kQ64_XB2 - kQ64_XB3) * 16 / (kQ64_XB4 > 0 ? kQ64_XB4 : 1);
}
constexpr int q64_gap_y(int e) {
  if (e < kQ64_YB4) return 48 + e * 16 / kQ64_YB4;
  return 64 + (e - kQ64_YB4) / 2;
}
constexpr bool q64_streams_ok() {
  for (int e = 0; e < 64; ++e) {
    const int qb = e >> 5, ks = (e & 31) >> 3;
    if (q64_gap_x(e) < 16 + 16 * qb) return false;                        // S^T[qb] is complete behind block qb + 1
    if (q64_gap_y(e) < 48 + 16 * qb || q64_gap_y(e) < q64_gap_x(e)) return false;      // dP^T[qb] complete, P there
    if (q64_gap_y(e) >= 64 + 16 * qb + 4 * ks) return false;              // packed before the k-step's first MFMA
    if (e && (q64_gap_x(e) < q64_gap_x(e - 1) || q64_gap_y(e) < q64_gap_y(e - 1))) return false;
  }
  return true;
}
static_assert(q64_streams_ok(), "dS of k-step ks must be packed before gap 16 + 4 ks of its dQ block, from complete chains");
constexpr int kQ64_DmaOpen = USP_Q64_DMA_OPEN, kQ64_DmaP0 = USP_Q64_DMA_P0, kQ64_DmaPS = USP_Q64_DMA_PS;
static_assert(kQ64_DmaOpen >= -1 && kQ64_DmaOpen < kQ64_DmaP0 && kQ64_DmaPS >= 1, "the descriptors are made before the first piece");
static_assert(kQ64_DmaP0 + 7 * kQ64_DmaPS < 80, "every piece is issued a block (16 gaps) or more before the dma_drain");

template <int DT, bool CAUSAL>
__global__ __launch_bounds__(256, 1) void flash_bwd_dq64_kernel(const BwdParams /* read through the kernarg segment */) {
  using E = Elem<DT>;
  using M = M64<DT>;
  constexpr int D = 128, kBM = 256;
  constexpr int ROWB = D * 2;
  constexpr int TILEB = kTile * ROWB;            // one K (or V) tile: 64 keys
  constexpr int VOFF = 2 * TILEB;                // LDS: Kbuf[0], Kbuf[1], Vbuf[0], Vbuf[1]
  constexpr int NKT = D / 16, NDJ = D / 32;
  constexpr int PF = kQ64_PF;

  extern __shared__ __attribute__((aligned(16))) char smem_raw[];
  USP_LDS char* smem = lds_block_at_zero(smem_raw);

  const int tid = threadIdx.x;
  const int lane = tid & 63;
  const int wave = __builtin_amdgcn_readfirstlane(tid >> 6);
  const int l31 = lane & 31;
  const int hi = lane >> 5;
  // the argument block stays in the kernarg segment (usp_flash_fwd64.hip: held in SGPRs it fills the scalar file)
  typedef const __attribute__((address_space(4))) BwdParams* KArgs;
  KArgs p = (KArgs)__builtin_amdgcn_kernarg_segment_ptr();
  asm volatile("" : "+s"(p));

  // ---- lane-constant addresses (tile layout, LDS-DMA pieces, row and transposed reads: usp_mfma64.hpp) -----------------
  // a tile is 4 groups of 16 rows; wave w stages group w of the K tile and of the V tile
  const int dma_row = lane >> 4, dma_c8 = dma_lane_col(lane & 15, dma_row);
  const int k_voff = dma_row * (int)p->k_ss * 2 + dma_c8, v_voff = dma_row * (int)p->v_ss * 2 + dma_c8;
  const int rd_base = l31 * ROWB + ((hi ^ tile_swz<D>(l31)) * 16);            // ^ (32 kt), + 32 kb rows
  int tr_addr[NDJ][2];
  {
    const int i = lane & 15, grp = (lane >> 4) & 1;
#pragma unroll
    for (int dj = 0; dj < NDJ; ++dj)
#pragma unroll
      for (int e = 0; e < 2; ++e) tr_addr[dj][e] = tr_read_offset<D>(i, grp, hi, dj, e);
  }
  const float c = p->scale_log2;

  const ItemWalk walk(p->n_items);               // persistent workgroups (usp_common.hpp)
  for (int pass = 0;; ++pass) {
  int w = walk.at(pass);
  if (w < 0) break;
  asm volatile("" : "+s"(p));
  USP_TM(const uint64_t tm_item = __builtin_amdgcn_s_memtime();)
  w = walk.dealt(w, p->nblk);
  if (p->ksplit <= 1) w = walk.grouped(w, p->nblk, p->walk_g);
  const int qt_r = w % p->nblk;
  int rest = w / p->nblk;
  const int qt = CAUSAL ? (p->nblk - 1 - qt_r) : qt_r;    // heavy (late) tiles first
  int cut = 0;                                            // key cut of a few-item launch (ABI v5 dq_splits): this item's run of
  if (p->ksplit > 1) { cut = rest % p->ksplit; rest /= p->ksplit; }     // the key tiles, partial to the workspace
  const int h = rest % p->Hq, b = rest / p->Hq;
  const int hkv = h / p->G;
  const int q0 = qt * kBM;
  const int qw = q0 + wave * 64;                          // first row of this wave
  const int off = p->causal_off;

  // ---- key range (usp_tile_range.h): the workgroup streams nt tiles, this wave works on n_w, the first n_full need no mask
  const usp_query_tiles kr = usp_query_tiles_of(q0, kBM, qw, 64, p->Sq, p->Sk, CAUSAL, off, kTile);
  const int nt = kr.nt, n_w = kr.n_w, n_full = kr.n_full;
  // key cut: the workgroup streams tiles [tb, te) of its [0, nt) -- equal runs, as the 8-wave kernel cuts them
  usp_tile_run run = {0, nt};
  if (p->ksplit > 1) run = usp_equal_run(0, nt, p->ksplit, cut);
  const int tb = run.begin, te = run.end;
  const int e_full = usp_clamp_to_run(n_full, tb, te);                      // [tb, e_full) plain, [e_full, e_own) masked,
  const int e_own = usp_clamp_to_run(n_w, tb, te);                          // [e_own, te) other waves' tiles

  // ---- resident B operands: Q and dO fragments of the wave's 64 rows, loaded straight into the accumulator file ------------
  u32x4 qf[2][NKT], df[2][NKT];
  float nl[2], dl[2];                            // -lse * log2(e) (-inf: the row sees no key -> P = 0) and delta per lane
#pragma unroll
  for (int qb = 0; qb < 2; ++qb) {
    const int row = qw + 32 * qb + l31;
    const int row_c = row < p->Sq ? row : p->Sq - 1;
    const char* qp = p->q + 2 * (b * p->q_sb + (int64_t)row_c * p->q_ss + h * p->q_sh) + 16 * hi;
    const char* dp = p->dout + 2 * (b * p->do_sb + (int64_t)row_c * p->do_ss + h * p->do_sh) + 16 * hi;
    load_resident16(qf[qb], df[qb], qp, dp);     // (per query block: the four groups of an item cost two round trips, not four)
    const float lse = p->lse[b * p->lse_sb + h * p->lse_sh + row_c];
    const float dlt = p->delta[b * p->dl_sb + h * p->dl_sh + row_c];
    const bool live = row < p->Sq && lse != USP_NEG_INF;
    nl[qb] = live ? -lse * kLog2e : USP_NEG_INF;
    dl[qb] = live ? dlt : 0.f;
  }

  // ---- LDS-DMA staging of the K / V tiles: running cursors at this wave's group (16 rows) of the tile ------------------
  const int k_rowb = (int)p->k_ss * 2, v_rowb = (int)p->v_ss * 2;
  const int64_t k_tb = (int64_t)kTile * k_rowb, v_tb = (int64_t)kTile * v_rowb;         // bytes per tile step
  int k_step = 4 * k_rowb - 1024, v_step = 4 * v_rowb - 1024;
  int lds_w = wave * 4096;
  const char* k_cur = p->k + 2 * (b * p->k_sb + hkv * p->k_sh) + (int64_t)wave * 16 * k_rowb + tb * k_tb;
  const char* v_cur = p->v + 2 * (b * p->v_sb + hkv * p->v_sh) + (int64_t)wave * 16 * v_rowb + tb * v_tb;
  int rows_kv = p->Sk - 16 * wave - tb * kTile;  // valid rows from the cursors on (<= 0: nothing left, lanes read 0)
  u32x4 k_rs, v_rs;
  int dma_buf = 0;
  auto dma_open = [&](int buf) {                 // scalar work only, no branch: it runs inside the MFMA stream
    k_rs = make_rsrc_rows(k_cur, rows_kv, 16, k_rowb, 2 * D);
    v_rs = make_rsrc_rows(v_cur, rows_kv, 16, v_rowb, 2 * D);
    dma_buf = buf;
    k_cur += k_tb;
    v_cur += v_tb;
    rows_kv -= kTile;
  };
  auto dma_piece = [&](int n) {                  // n < 4: K piece n, else V piece n - 4
    asm volatile("" : "+s"(lds_w), "+s"(k_step), "+s"(v_step));
    const int i = n & 3;
    if (n < 4) lds_dma16_asm(k_rs, lds_w + dma_buf * TILEB, k_voff ^ (16 * i), i * k_step, i);
    else lds_dma16_asm(v_rs, lds_w + VOFF + dma_buf * TILEB, v_voff ^ (16 * i), i * v_step, i);
  };

  // the dP^T chains start from -delta (one accumulator tuple per query block, all 16 values the lane's own row's), so the
  // element stream is left with dS = P * chain.  Opaque: hipcc otherwise re-materialises 16 v_mov per chain and tile.
  f32x16 cd[2];
#pragma unroll
  for (int qb = 0; qb < 2; ++qb) {
#pragma unroll
    for (int r = 0; r < 16; ++r) cd[qb][r] = -dl[qb];
    asm volatile("" : "+v"(cd[qb]));
  }

  f32x16 dq[2][NDJ];                             // dQ^T: [query block][dim tile]
#pragma unroll
  for (int qb = 0; qb < 2; ++qb)
#pragma unroll
    for (int dj = 0; dj < NDJ; ++dj) zero_pin_agpr(dq[qb][dj]);

  dma_open(tb & 1);                              // (iteration t reads buffer t & 1)
#pragma unroll
  for (int n = 0; n < 8; ++n) dma_piece(n);
  dma_drain();
  __syncthreads();

  USP_TM(uint32_t tm_blk[8] = {0, 0, 0, 0, 0, 0, 0, 0};)     // plain tiles: cycles of B1 .. B6, of drain + barrier, and their number
  // one iteration = one key tile: [stage the next tile] [the six blocks] [publish].  The tile body is STRAIGHT-LINE code
  // (usp_flash_bwd64.hip: anything conditional around the asm MFMAs makes hipcc copy accumulators); a tile that needs the
  // causal / ragged mask runs in a loop instance of its own (MASK) with the mask applied to S^T behind B1 and B2.
  auto iter = [&](auto mask_c, int t, bool work) __attribute__((always_inline)) {
    constexpr bool MASK = decltype(mask_c)::value;
    const int par = t & 1;
    USP_TM(uint32_t tm_s[8] = {0, 0, 0, 0, 0, 0, 0, 0};)
    if (work) {
      USP_TM(tm_s[0] = tm_stamp();)
#pragma unroll
      for (int qb = 0; qb < 2; ++qb)
#pragma unroll
        for (int kt = 0; kt < NKT; ++kt) { pin_agpr4(qf[qb][kt]); pin_agpr4(df[qb][kt]); }
      // buffer bases go INTO the swizzled offsets before the XOR (multiples of 256; the XOR touches bits 5-7)
      int kr = rd_base + par * TILEB, vr = rd_base + VOFF + par * TILEB;
      asm volatile("" : "+v"(kr), "+v"(vr));     // opaque per tile: hipcc otherwise hoists the XORed addresses and spills them
      USP_LDS const char* kt_base = smem + par * TILEB;
      f32x16 bs[2][2], bd[2][2];                 // S^T -> P^T, dP^T -> dS^T: [query block][key block]
      u32x4 pk[2][4];                            // packed dS^T: [query block][k-step of 16 keys]
      u32x4 ka[2 * NKT], va[2 * NKT], xa[4 * NDJ];
      auto rd_k = [&](int f) { ka[f] = *(USP_LDS const u32x4*)(smem + (f & 1) * 32 * ROWB + (kr ^ (32 * (f >> 1)))); };
      auto rd_v = [&](int f) { va[f] = *(USP_LDS const u32x4*)(smem + (f & 1) * 32 * ROWB + (vr ^ (32 * (f >> 1)))); };
      auto rd_x = [&](int f) {                   // fragment f = NDJ * ks + dj of K^T
        USP_LDS const char* xb = kt_base + (f / NDJ) * 16 * ROWB;
        const u32x2 a0 = lds_read_tr16(xb + tr_addr[f % NDJ][0]);
        const u32x2 a1 = lds_read_tr16(xb + tr_addr[f % NDJ][1]);
        xa[f] = u32x4{a0[0], a0[1], a1[0], a1[1]};
      };
      // element n (0 .. 31) of query block qb, in the order the dQ k-steps need them: n = 8 ks + r8 ->
      // [qb][ks >> 1][8 (ks & 1) + r8]
      auto X = [&](int qb, int n) {
        const int ks = n >> 3, kb = ks >> 1, r = 8 * (ks & 1) + (n & 7);
        bs[qb][kb][r] = fast_exp2(__builtin_fmaf(bs[qb][kb][r], c, nl[qb]));
      };
      auto Y = [&](int qb, int n) {
        const int ks = n >> 3, kb = ks >> 1, r = 8 * (ks & 1) + (n & 7);
        bd[qb][kb][r] = bd[qb][kb][r] * bs[qb][kb][r];
        if (r & 1) pk[qb][ks][(n & 7) >> 1] = E::pack2(bd[qb][kb][r - 1], bd[qb][kb][r]);
      };
      auto elems = [&](int g) {                  // the element work of gap g
#pragma unroll
        for (int e = 0; e < 64; ++e)
          if (q64_gap_x(e) == g) X(e >> 5, e & 31);
#pragma unroll
        for (int e = 0; e < 64; ++e)
          if (q64_gap_y(e) == g) Y(e >> 5, e & 31);
      };
      auto stage = [&](int g) {                  // the next tile's staging, by gap of the tile
        if (g == kQ64_DmaOpen) dma_open(par ^ 1);
#pragma unroll
        for (int n = 0; n < 8; ++n)
          if (g == kQ64_DmaP0 + n * kQ64_DmaPS) dma_piece(n);
      };
      auto mask = [&](int qb) {                  // key j is visible to query row i iff j <= min(i + off, Sk - 1)
        const int row = qw + 32 * qb + l31;
        int klim = p->Sk - 1;
        if (CAUSAL) klim = row + off < klim ? row + off : klim;
        const int kb0 = t * kTile + 4 * hi;
#pragma unroll
        for (int r = 0; r < 16; ++r) {
          const int key = kb0 + (r & 3) + 8 * (r >> 2);
          if (key > klim) bs[qb][0][r] = USP_NEG_INF;
          if (key + 32 > klim) bs[qb][1][r] = USP_NEG_INF;
        }
      };
      // ---------------- B1: S^T[0], the K row fragments arrive; the next tile's staging ----------------
#pragma unroll
      for (int f = 0; f < PF; ++f) rd_k(f);
      if (kQ64_DmaOpen < 0) dma_open(par ^ 1);   // scalar work under the fragments' LDS round trip
      __builtin_amdgcn_sched_barrier(0);
#pragma unroll
      for (int i = 0; i < 16; ++i) {
        const int kt = i >> 1, kb = i & 1;
        if (kt == 0) M::template s_first<MASK>(bs[0][kb], ka[i], qf[0][0]);
        else M::template s_next<MASK>(bs[0][kb], ka[i], qf[0][kt]);
        if (i == 0) __builtin_amdgcn_sched_barrier(0);
        if (i + PF < 16) rd_k(i + PF);
        stage(i);
        __builtin_amdgcn_sched_barrier(0);
      }
      USP_TM(tm_s[1] = tm_stamp();)
      if (MASK) { mfma_settle(bs[0]); mask(0); }
      // ---------------- B2: S^T[1] (fragments from the registers) | elements by the table; the first V fragments ----------------
#pragma unroll
      for (int i = 0; i < 16; ++i) {
        const int kt = i >> 1, kb = i & 1;
        if (kt == 0) M::template s_first<MASK>(bs[1][kb], ka[i], qf[1][0]);
        else M::template s_next<MASK>(bs[1][kb], ka[i], qf[1][kt]);
        if (i == 0) __builtin_amdgcn_sched_barrier(0);     // the elements read B1's results: not in front of this MFMA
        elems(16 + i);
        if (i >= 16 - PF) rd_v(i - (16 - PF));
        stage(16 + i);
        __builtin_amdgcn_sched_barrier(0);
      }
      USP_TM(tm_s[2] = tm_stamp();)
      if (MASK) { mfma_settle(bs[1]); mask(1); }
      // ---------------- B3: dP^T[0] from -delta, the V row fragments arrive | elements ----------------
#pragma unroll
      for (int i = 0; i < 16; ++i) {
        const int kt = i >> 1, kb = i & 1;
        if (kt == 0) M::template s_first_c<MASK>(bd[0][kb], va[i], df[0][0], cd[0]);
        else M::template s_next<MASK>(bd[0][kb], va[i], df[0][kt]);
        if (i == 0) __builtin_amdgcn_sched_barrier(0);
        if (i + PF < 16) rd_v(i + PF);
        elems(32 + i);
        stage(32 + i);
        __builtin_amdgcn_sched_barrier(0);
      }
      USP_TM(tm_s[3] = tm_stamp();)
      // ---------------- B4: dP^T[1] from -delta | elements; the first K^T fragments ----------------
#pragma unroll
      for (int i = 0; i < 16; ++i) {
        const int kt = i >> 1, kb = i & 1;
        if (kt == 0) M::template s_first_c<MASK>(bd[1][kb], va[i], df[1][0], cd[1]);
        else M::template s_next<MASK>(bd[1][kb], va[i], df[1][kt]);
        if (i == 0) __builtin_amdgcn_sched_barrier(0);
        elems(48 + i);
        if (i >= 16 - PF) rd_x(i - (16 - PF));
        stage(48 + i);
        __builtin_amdgcn_sched_barrier(0);
      }
      USP_TM(tm_s[4] = tm_stamp();)
      // ---------------- B5: dQ^T[0], the K^T fragments arrive | B6: dQ^T[1] | the tail of Y[0], Y[1] ----------------
#pragma unroll
      for (int i = 0; i < 16; ++i) {
        M::template o_acc<MASK>(dq[0][i % NDJ], xa[i], pk[0][i / NDJ]);
        if (i == 0) __builtin_amdgcn_sched_barrier(0);
        if (i + PF < 16) rd_x(i + PF);
        elems(64 + i);
        stage(64 + i);
        __builtin_amdgcn_sched_barrier(0);
      }
      USP_TM(tm_s[5] = tm_stamp();)
#pragma unroll
      for (int i = 0; i < 16; ++i) {
        M::template o_acc<MASK>(dq[1][i % NDJ], xa[i], pk[1][i / NDJ]);
        elems(80 + i);
        __builtin_amdgcn_sched_barrier(0);
      }
      USP_TM(tm_s[6] = tm_stamp();)
    } else {
      dma_open(par ^ 1);
#pragma unroll
      for (int n = 0; n < 8; ++n) dma_piece(n);
    }
    dma_drain();            // this wave's pieces of the next tile have landed ...
    __syncthreads();        // ... and so have everybody else's; every wave is done with this tile's buffers
    USP_TM(if (work && !MASK) {
      tm_s[7] = tm_stamp();
      _Pragma("unroll") for (int j = 0; j < 7; ++j) tm_blk[j] += tm_s[j + 1] - tm_s[j];
      ++tm_blk[7];
    })
  };
  const std::integral_constant<bool, false> plain;
  const std::integral_constant<bool, true> masked;
  int t = tb;
  USP_TM(const uint64_t tm_loop = __builtin_amdgcn_s_memtime();)
  __builtin_amdgcn_s_waitcnt(0x0f70);            // (usp_flash_bwd64.hip: nothing may still count as pending at a loop header)
  for (; t < e_full; ++t) iter(plain, t, true);
  __builtin_amdgcn_s_waitcnt(0x0f70);
  for (; t < e_own; ++t) iter(masked, t, true);
  mfma_settle(dq);
  USP_TM(const uint64_t tm_own = __builtin_amdgcn_s_memtime(); const uint64_t tm_plain_n = n_full;)
  for (; t < te; ++t) iter(plain, t, false);     // tiles other waves of the workgroup still work on: keep the cadence
  USP_TM(const uint64_t tm_epi = __builtin_amdgcn_s_memtime();)

  // ---- epilogue: fp32 store / accumulate, or final 16-bit store (dQ^T: a lane holds 4-dim pieces of ONE query row) --------
  mfma_settle(dq);
  asm volatile("" : "+s"(p));
  const bool wide = (p->wide16 & 1) != 0;         // 16-bit final output, rows 16-byte aligned, nothing accumulated (never with a cut)
#pragma unroll
  for (int qb = 0; qb < 2; ++qb) {
    const int row = qw + 32 * qb + l31;
    if (wide) {
      const int row_c = row < p->Sq ? row : 0;
      store_row16_wide<E, NDJ>(p->dq16 + 2 * (b * p->dq16_sb + (int64_t)row_c * p->dq16_ss + h * p->dq16_sh), dq[qb], p->scale, hi,
                               row < p->Sq);
    } else if (row < p->Sq) {
      float* o1 = p->dq + b * p->dq_sb + (int64_t)row * p->dq_ss + h * p->dq_sh;
      char* h1 = p->dq16 ? p->dq16 + 2 * (b * p->dq16_sb + (int64_t)row * p->dq16_ss + h * p->dq16_sh) : nullptr;
      int acc_f = p->accum_dq;
      if (p->ksplit > 1) {       // the partial of this cut, combined (deterministically) with the others and with an accumulated
        o1 = p->ws_dq + ((((int64_t)cut * p->B + b) * p->Sq + row) * p->Hq + h) * D;      // dq by reduce_cuts_kernel
        h1 = nullptr;
        acc_f = 0;
      }
      store_row32_acc<E, NDJ>(o1, h1, dq[qb], p->scale, hi, acc_f);
    }
  }
  __syncthreads();          // the next item's prologue refills the tile buffers
USP_TM(
  const uint32_t tm_n = tm_blk[7] ? tm_blk[7] : 1;
  if (pass < 3 && lane == 0 && (blockIdx.x % 61) == 0)
    printf("TQ wg %3d pass %d wave %d qt %2d tiles own %3d (plain %3d) wg %3d : prologue %6llu own tiles %8llu (%5llu / tile) idle %6llu epilogue %6llu | plain tile B1-B6, drain + barrier: %u %u %u %u %u %u %u\n",
           (int)blockIdx.x, pass, wave, qt, n_w, (int)tm_plain_n, nt, (unsigned long long)(tm_loop - tm_item),
           (unsigned long long)(tm_own - tm_loop), (unsigned long long)((tm_own - tm_loop) / (n_w > 0 ? n_w : 1)),
           (unsigned long long)(tm_epi - tm_own), (unsigned long long)(__builtin_amdgcn_s_memtime() - tm_epi),
           tm_blk[0] / tm_n, tm_blk[1] / tm_n, tm_blk[2] / tm_n, tm_blk[3] / tm_n, tm_blk[4] / tm_n, tm_blk[5] / tm_n, tm_blk[6] / tm_n);
)
  }  // next item
}

bool dq64_serves(const BwdParams& p_in) {
  // dense launches (bf16 / fp16) without a window or the dynamic item queue; the pieces' swizzle is XORed into the per-lane byte
  // offset (rows a multiple of 256 bytes apart), 64 rows of K / V span less than 2^31 bytes
  if (p_in.seq_q || p_in.seq_k || p_in.sched || p_in.win_on) return false;
  return dma_rows_ok(p_in.k_ss, true) && dma_rows_ok(p_in.v_ss, true);
}

bool launch_dq64(const BwdParams& p_in, int dtype, bool causal, hipStream_t st, int* rc) {
  if (!dq64_serves(p_in)) return false;
  BwdParams p = p_in;
  p.nblk = (p.Sq + 255) / 256;
  p.n_items = p.B * p.Hq * p.nblk * p.ksplit;
  p.wide16 = (p.ksplit <= 1 && p.dq16 && !p.accum_dq && tensor_aligned(p.dq16, p.dq16_sb, p.dq16_ss, p.dq16_sh, 16, 8)) ? 1 : 0;
  const int grid = persistent_grid(p.n_items, device_cus(), p.interleave);      // persistent: one workgroup per CU
  const size_t lds = 4 * kTile * 128 * 2;
  with_dtype_causal(dtype, causal, [&](auto dt, auto c) {
    hipLaunchKernelGGL((flash_bwd_dq64_kernel<decltype(dt)::value, decltype(c)::value>), dim3(grid), dim3(256), lds, st, p);
  });
  *rc = launched();
  return true;
}

}  // namespace usp
