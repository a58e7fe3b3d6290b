// What the pattern stages (ingest.hip, correct.hip, resample.hip) share about their source: raw
// patterns arrive as `const void* src` with the public header's src_dtype code (0 float64,
// 1 float32, 2 uint8), and a non-finite source value counts as 0.
#pragma once
#include <type_traits>

#include "common.h"

namespace ev {
EV_DEVINL float finite_or_zero(float v) { return fabsf(v) <= 3.4028235e38f ? v : 0.f; }   // NaN, +-inf
}  // namespace ev

namespace evh {
// f(the typed source pointer) for a src_dtype the entry point has already checked
template <typename F>
inline void with_src(const void* src, int src_dtype, F&& f) {
  if (src_dtype == 0) f((const double*)src);
  else if (src_dtype == 1) f((const float*)src);
  else f((const unsigned char*)src);
}
// the element type behind the pointer with_src hands to f
template <typename P>
using elem_t = std::remove_const_t<std::remove_pointer_t<P>>;
}  // namespace evh
