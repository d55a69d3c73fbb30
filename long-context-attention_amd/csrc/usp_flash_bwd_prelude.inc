// Prelude of usp_flash_bwd_dq_body.inc and usp_flash_bwd_dkdv_body.inc: what the argument block `p_in` says about the kernel.  A
// feature is ON when the block derives from the feature's struct (usp_bwd_params.hpp); its values are then the block's own fields,
// and zero / null otherwise.  A new feature adds its struct, one switch and its values HERE, and its steps to the bodies: no other
// kernel's wrapper changes.  The dQ body reads the row bounds, the dK/dV body their transposes, the key bounds.
// The form is what keeps every kernel's machine code (profiles/variant_prelude_isa.txt): fields are read straight from the block,
// never through a function or a lambda that takes it; the names the bodies read are `const` (their lambdas capture them by
// reference, and a name left assignable changed the causal block-sparse dK/dV kernels); `dr` is a reference to the block's Dropout
// part, not a copy of it (a copy changed all three dropout kernels).
  using PA_ = std::conditional_t<(D > 0), std::remove_cv_t<decltype(p_in)>, void>;   // dependent: a discarded branch below is not looked up
  const PA_& px = p_in;
  [[maybe_unused]] constexpr bool SC = std::is_base_of_v<BwdSoftcap, PA_>, AL = std::is_base_of_v<BwdAlibi, PA_>,
                                  DR = std::is_base_of_v<Dropout, PA_>, DOC = std::is_base_of_v<BwdDoc, PA_>,
                                  SPAN = std::is_base_of_v<BwdSpan, PA_>, BSP = std::is_base_of_v<BwdBsp, PA_>;
  static_assert(!SPAN || (DOC && !CAUSAL), "a span is a document bound with a right bound in the diagonal's place");
  static_assert(!BSP || !DOC, "a listed walk starts at its list's first entry, not at a document's first key");
  struct {                                                   // the values of a kernel with every feature off
    float sc_cl2 = 0.f, sc_k2 = 0.f;                         // softcap: cap * log2(e), 2 * scale * log2(e) / cap
    const float* al_slopes = nullptr;                        // ALiBi: fp32 slopes, their batch stride, the bias diagonal
    int64_t al_sb = 0;
    int al_diag = 0;
    const int* doc_row_lo = nullptr;                         // document mask: int32 left bounds by row (dQ) ...
    const int* doc_key_hi = nullptr;                         // ... and by key (dK/dV), their batch strides
    int64_t doc_rl_sb = 0, doc_kh_sb = 0;
    const int* span_row_hi = nullptr;                        // span: int32 right bounds by row (dQ) ...
    const int* span_key_lo = nullptr;                        // ... and by key (dK/dV), their batch strides
    int64_t span_rh_sb = 0, span_kl_sb = 0;
    const int* bsp_lists = nullptr;                          // block-sparse mask: the items' tile lists, ints per list
    int bsp_stride = 0;
  } v_;
  [[maybe_unused]] constexpr Dropout dr_off{};               // dropout: the block of usp_dropout_rng.h
  const Dropout* dr_ = &dr_off;
  if constexpr (SC) { v_.sc_cl2 = px.cap_log2; v_.sc_k2 = px.tanh_k2; }
  if constexpr (AL) { v_.al_slopes = px.al_slopes; v_.al_sb = px.al_sb; v_.al_diag = px.al_diag; }
  if constexpr (DR) dr_ = &px;
  if constexpr (DOC) { v_.doc_row_lo = px.row_lo; v_.doc_key_hi = px.key_hi; v_.doc_rl_sb = px.row_lo_sb; v_.doc_kh_sb = px.key_hi_sb; }
  if constexpr (SPAN) { v_.span_row_hi = px.row_hi; v_.span_key_lo = px.key_lo; v_.span_rh_sb = px.row_hi_sb; v_.span_kl_sb = px.key_lo_sb; }
  if constexpr (BSP) { v_.bsp_lists = px.bsp_lists; v_.bsp_stride = px.bsp_stride; }
  [[maybe_unused]] const float sc_cl2 = v_.sc_cl2, sc_k2 = v_.sc_k2;
  [[maybe_unused]] const float* const al_slopes = v_.al_slopes;
  [[maybe_unused]] const int64_t al_sb = v_.al_sb;
  [[maybe_unused]] const int al_diag = v_.al_diag;
  [[maybe_unused]] const Dropout& dr = *dr_;
  [[maybe_unused]] const int* const doc_row_lo = v_.doc_row_lo;
  [[maybe_unused]] const int* const doc_key_hi = v_.doc_key_hi;
  [[maybe_unused]] const int64_t doc_rl_sb = v_.doc_rl_sb, doc_kh_sb = v_.doc_kh_sb;
  [[maybe_unused]] const int* const span_row_hi = v_.span_row_hi;
  [[maybe_unused]] const int* const span_key_lo = v_.span_key_lo;
  [[maybe_unused]] const int64_t span_rh_sb = v_.span_rh_sb, span_kl_sb = v_.span_kl_sb;
  [[maybe_unused]] const int* const bsp_lists = v_.bsp_lists;
  [[maybe_unused]] const int bsp_stride = v_.bsp_stride;
