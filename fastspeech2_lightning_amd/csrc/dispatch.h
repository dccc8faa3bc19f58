// Host side of the non-GEMM launchers (norm.hip, bn.hip, conv.hip, attention*.hip, gemm_ws.hip): a run-time bool or int
// becomes a compile-time constant handed to a generic lambda, which names the kernel instance and returns an int
// (0, a launch error, FS2HIP_EINVAL).  Two or three picks nest by hand.  A pick over independent values instantiates
// their whole product: a combination that has no kernel instance is refused in ONE visible place -- a check before the
// picks, or `if constexpr (...) return FS2HIP_EINVAL;` at the top of the lambda.  Host-only.
#pragma once
#include <type_traits>

#include "common.h"

// what a launcher returns behind its <<<>>>: the launch error, if any
inline int fs2_launched() {
  FS2_LAUNCH_CHECK();
  return 0;
}

// f(std::bool_constant<b>)
template <class F>
inline int fs2_pick_bool(bool b, F&& f) {
  return b ? f(std::true_type{}) : f(std::false_type{});
}

// f(std::integral_constant<int, v>) for the v of Vs... that equals `v`, else f(std::integral_constant<int, FALLBACK>)
template <int FALLBACK, int... Vs, class F>
inline int fs2_pick_int(int v, F&& f) {
  int rc = 0;
  const bool hit = ((v == Vs ? (rc = f(std::integral_constant<int, Vs>{}), true) : false) || ...);
  return hit ? rc : f(std::integral_constant<int, FALLBACK>{});
}
