// Prelude of usp_flash_fwd_body.inc: what the argument block `p_in` says about the kernel.  A feature is ON when the block derives
// from the feature's struct (usp_fwd_params.hpp); its values are then the block's own fields, and zero / null otherwise.  A new
// feature adds its struct, one switch and its values HERE, and its steps to the body: no other kernel's wrapper changes.
// The form is what keeps every kernel's machine code (profiles/variant_prelude_isa.txt): fields are read straight from the block,
// never through a function or a lambda that takes it; the names the body reads are `const` (its lambdas capture them by reference,
// and a name left assignable changed the span kernels); `dr` is a reference to the block's Dropout part, not a copy of it.
  using PA_ = std::conditional_t<(D > 0), std::remove_cv_t<decltype(p_in)>, void>;   // dependent: a discarded branch below is not looked up
  const PA_& px = p_in;
  [[maybe_unused]] constexpr bool KSPLIT = std::is_base_of_v<FwdSplit, PA_>, SC = std::is_base_of_v<FwdSoftcap, PA_>,
                                  AL = std::is_base_of_v<FwdAlibi, PA_>, DR = std::is_base_of_v<Dropout, PA_>,
                                  SINK = std::is_base_of_v<FwdSink, PA_>, DOC = std::is_base_of_v<FwdDoc, PA_>,
                                  SPAN = std::is_base_of_v<FwdSpan, PA_>, BSP = std::is_base_of_v<FwdBsp, PA_>,
                                  MAXL = std::is_base_of_v<FwdMaxl, PA_>;
  static_assert(!WIN || KSPLIT, "the window walk reads the left bound of the split block");
  static_assert(!(AL || DR) || KSPLIT, "the bias diagonal and the dropout key offset are rebased with the K cut");
  static_assert(!SPAN || (DOC && !CAUSAL), "a span is a document bound with a right bound in the diagonal's place");
  static_assert(!BSP || !(WIN || DOC), "a listed walk has no rotation");
  static_assert(!MAXL || !(SC || AL || DR || SINK || DOC || BSP), "the true row maximum is kept for raw, unbiased scores of a plain walk");
  struct {                                                   // the values of a kernel with every feature off
    float sc_cl2 = 0.f, sc_k2 = 0.f;                         // softcap: cap * log2(e), 2 * scale * log2(e) / cap
    const float* al_slopes = nullptr;                        // ALiBi: fp32 slopes, their batch stride, the bias diagonal
    int64_t al_sb = 0;
    int al_diag = 0;
    const float* sink_s = nullptr;                           // sinks: fp32 (Hq,) sink logits
    const int* doc_row_lo = nullptr;                         // document mask: int32 left row bounds, their batch stride
    int64_t doc_sb = 0;
    const int* span_row_hi = nullptr;                        // span: int32 right row bounds, their batch stride
    int64_t span_sb = 0;
    const int* bsp_lists = nullptr;                          // block-sparse mask: the items' tile lists, ints per list
    int bsp_stride = 0;
    float* maxl_row = nullptr;                               // max logits: fp32 (B, Hq, Sq) row maxima, batch / head strides
    int64_t maxl_sb = 0, maxl_sh = 0;
  } v_;
  [[maybe_unused]] constexpr Dropout dr_off{};               // dropout: the block of usp_dropout_rng.h
  const Dropout* dr_ = &dr_off;
  if constexpr (SC) { v_.sc_cl2 = px.cap_log2; v_.sc_k2 = px.tanh_k2; }
  if constexpr (AL) { v_.al_slopes = px.al_slopes; v_.al_sb = px.al_sb; v_.al_diag = px.al_diag; }
  if constexpr (DR) dr_ = &px;
  if constexpr (SINK) v_.sink_s = px.sinks;
  if constexpr (DOC) { v_.doc_row_lo = px.row_lo; v_.doc_sb = px.row_lo_sb; }
  if constexpr (SPAN) { v_.span_row_hi = px.row_hi; v_.span_sb = px.row_hi_sb; }
  if constexpr (BSP) { v_.bsp_lists = px.bsp_lists; v_.bsp_stride = px.bsp_stride; }
  if constexpr (MAXL) { v_.maxl_row = px.row_max; v_.maxl_sb = px.row_max_sb; v_.maxl_sh = px.row_max_sh; }
  [[maybe_unused]] const float sc_cl2 = v_.sc_cl2, sc_k2 = v_.sc_k2;
  [[maybe_unused]] const float* const al_slopes = v_.al_slopes;
  [[maybe_unused]] const int64_t al_sb = v_.al_sb;
  [[maybe_unused]] const int al_diag = v_.al_diag;
  [[maybe_unused]] const Dropout& dr = *dr_;
  [[maybe_unused]] const float* const sink_s = v_.sink_s;
  [[maybe_unused]] const int* const doc_row_lo = v_.doc_row_lo;
  [[maybe_unused]] const int64_t doc_sb = v_.doc_sb;
  [[maybe_unused]] const int* const span_row_hi = v_.span_row_hi;
  [[maybe_unused]] const int64_t span_sb = v_.span_sb;
  [[maybe_unused]] const int* const bsp_lists = v_.bsp_lists;
  [[maybe_unused]] const int bsp_stride = v_.bsp_stride;
  [[maybe_unused]] float* const maxl_row = v_.maxl_row;
  [[maybe_unused]] const int64_t maxl_sb = v_.maxl_sb, maxl_sh = v_.maxl_sh;
