// The top-p rule from "total = SUM(W)" on (include/usp_hip.h: usp_block_select_top_p), included as TEXT by both producers of the
// weights -- block_select_top_p_kernel (usp_block_select_top_p.hip) and block_select_weights_kernel (usp_block_select_weights.hip) -- so that each compiles the
// very statements the other does.  USP_TOP_P_HELPERS: the workgroup reductions and the order-preserving key, at namespace scope.
// USP_TOP_P_ROW: what the row block sees and must keep; the includer has Ig, nbk, a.causal,
// a.keep_first, a.keep_local.  USP_TOP_P_CUT: the cut over the nbk weights `wts` in LDS and the mask row(s); the includer has
// besides t, lane, wave, slots, phase, a.top_p, a.mask with a.sb / a.sh / a.sr, b, h0, nh, I.
#if defined(USP_TOP_P_HELPERS)
constexpr int kTopPThreads = 256;

// ascending key <=> ascending float (usp_block_select.hip: order_key); a weight >= +0 has a key >= 0x80000000
USP_DEV uint32_t weight_key(float w) {
  if (w == 0.f) w = 0.f;
  const uint32_t u = __builtin_bit_cast(uint32_t, w);
  return (u & 0x80000000u) ? ~u : (u | 0x80000000u);
}

USP_DEV float wave_sum(float x) {
#pragma unroll
  for (int m = 32; m >= 1; m >>= 1) x += __shfl_xor(x, m, 64);
  return x;
}

USP_DEV float wave_max(float x) {
#pragma unroll
  for (int m = 32; m >= 1; m >>= 1) x = fmaxf(x, __shfl_xor(x, m, 64));
  return x;
}

// The sum / maximum over the workgroup, the same bits in every thread.  Two sets of four wave slots alternate (`phase`), so one
// barrier a reduction is enough: a set is written again only behind the barrier of the reduction between, which every thread
// reaches after it has read the set.
USP_DEV float block_sum(float x, float* slots, int& phase, int lane, int wave) {
  x = wave_sum(x);
  float* const w = slots + 4 * (phase++ & 1);
  if (lane == 0) w[wave] = x;
  __syncthreads();
  return ((w[0] + w[1]) + w[2]) + w[3];
}

USP_DEV float block_max(float x, float* slots, int& phase, int lane, int wave) {
  x = wave_max(x);
  float* const w = slots + 4 * (phase++ & 1);
  if (lane == 0) w[wave] = x;
  __syncthreads();
  return fmaxf(fmaxf(w[0], w[1]), fmaxf(w[2], w[3]));
}
#elif defined(USP_TOP_P_ROW)
  // visible: [0, nv); forced: [0, kf) and [lo, hi] inside it
  const int nv = a.causal ? (Ig + 1 < nbk ? Ig + 1 : nbk) : nbk;
  const int kf = a.keep_first < nv ? a.keep_first : nv;
  const int lo = Ig - a.keep_local + 1 > 0 ? Ig - a.keep_local + 1 : 0;
  const int hi = Ig < nv - 1 ? Ig : nv - 1;
  const int n_local = hi >= lo ? hi - lo + 1 : 0;
  const int both = n_local > 0 && kf > lo ? (kf < hi + 1 ? kf : hi + 1) - lo : 0;
  const int n_cand = nv - (kf + n_local - both);
  const bool search = n_cand > 0;                  // (otherwise every visible block is forced: no weight decides anything)
  int phase = 0;
#elif defined(USP_TOP_P_CUT)
  const auto is_forced = [&](int J) { return J < nv && (J < kf || (J >= lo && J <= hi)); };
  // key of block J: of its weight where it is a candidate, 0 (below every candidate's) elsewhere
  const auto key_of = [&](int J, float w) { return (J < nv && !is_forced(J)) ? weight_key(w) : 0u; };
  // mass(c) = sum of the weights of the forced blocks and of the candidates with key >= c
  const auto mass = [&](uint32_t c) {
    float acc = 0.f;
    for (int J = t; J < nbk; J += kTopPThreads) {
      const float w = wts[J];
      acc += (is_forced(J) || key_of(J, w) >= c) ? w : 0.f;
    }
    return block_sum(acc, slots, phase, lane, wave);
  };
  // the cut T, bit by bit: the largest T with mass(T) >= target (mass(0) = total >= target: top_p <= 1)
  uint32_t T = 0xFFFFFFFFu;
  float target = 0.f, m_gt = 0.f, wt = 0.f;
  int n_eq = 0, need = 0;
  if (search) {
    target = a.top_p * mass(0u);
    T = 0u;
    for (int bit = 31; bit >= 0; --bit) {
      const uint32_t c = T | (1u << bit);
      if (mass(c) >= target) T = c;
    }
    if (T != 0xFFFFFFFFu) {                        // (all ones: the forced blocks alone reach the target)
      m_gt = mass(T + 1u);
      float cnt = 0.f;
      for (int J = t; J < nbk; J += kTopPThreads) cnt += key_of(J, wts[J]) == T ? 1.f : 0.f;
      n_eq = (int)block_sum(cnt, slots, phase, lane, wave);       // (at most 8192: exact)
      wt = __builtin_bit_cast(float, T & 0x7FFFFFFFu);            // the weight every block of key T has
      // ties taken: the smallest c in [1, n_eq] with fmaf(c, wt, m_gt) >= target, n_eq where none has
      need = n_eq;
      if (n_eq > 0 && __builtin_fmaf((float)n_eq, wt, m_gt) >= target) {
        int c_lo = 1, c_hi = n_eq;
        while (c_lo < c_hi) {
          const int mid = (c_lo + c_hi) >> 1;
          if (__builtin_fmaf((float)mid, wt, m_gt) >= target) c_hi = mid; else c_lo = mid + 1;
        }
        need = c_lo;
      }
    }
  }
  int taken = 0;                                   // ties met in the chunks before this one
  unsigned char* const out = a.mask + b * a.sb + h0 * a.sh + I * a.sr;
  for (int J0 = 0; J0 < nbk; J0 += kTopPThreads) {
    const int J = J0 + t;
    const bool in = J < nbk;
    bool sel = in && is_forced(J);
    if (search) {
      const uint32_t key = in ? key_of(J, wts[J]) : 0u;
      const bool eq = in && key == T && key != 0u;
      const unsigned long long bal = __ballot(eq);
      float* const w = slots + 4 * (phase++ & 1);
      if (lane == 0) w[wave] = (float)__builtin_popcountll(bal);
      __syncthreads();
      int before = taken;
      for (int i = 0; i < wave; ++i) before += (int)w[i];
      taken += (int)(w[0] + w[1] + w[2] + w[3]);
      const int rank = before + __builtin_popcountll(bal & ((1ull << lane) - 1ull));
      sel = sel || (key > T) || (eq && rank < need);
    }
    if (in)
      for (int g = 0; g < nh; ++g) out[g * a.sh + J] = sel ? 1 : 0;
  }
#endif
