// dispatch.h -- host side: run-time shape and model to the kernel instance built for it. A launcher
// names its kernel once, inside nested with_* calls; each hands the functor one compile-time value.
#pragma once
#include <type_traits>

#include "mmre_common.h"

namespace mmre {

// 64-float chunks per lane (the kernels' NC: 1, 2, 4, ... max_nc) for rows of `dim` floats; 0: no
// instance.
inline int nc_for_dim(int dim, int max_nc) {
  for (int nc = 1; nc <= max_nc; nc *= 2)
    if (dim <= nc * kWave) return nc;
  return 0;
}

// The launches f(std::integral_constant<int, NC>) makes for nc == NC in 1, 2, 4, ... MAX_NC (no
// wider instance is built) and their error; anything else is no shape of the family.
template <int MAX_NC, int NC = 1, class F>
int with_nc(int nc, F&& f) {
  if constexpr (NC > MAX_NC) {
    return MMRE_ERR_SHAPE;
  } else {
    if (nc != NC) return with_nc<MAX_NC, 2 * NC>(nc, f);
    f(std::integral_constant<int, NC>{});
    MMRE_CHECK_LAUNCH();
    return MMRE_OK;
  }
}

template <class F>
int with_bool(bool b, F&& f) {
  return b ? f(std::true_type{}) : f(std::false_type{});
}
template <class F>  // f(a_, b_, c_)
int with_bools(bool a, bool b, bool c, F&& f) {
  return with_bool(a, [&](auto a_) {
    return with_bool(b, [&](auto b_) { return with_bool(c, [&](auto c_) { return f(a_, b_, c_); }); });
  });
}

// f(std::integral_constant<int, OP>) for the link sweeps' score operator op = op_of_model(model), 0 .. 4
template <int OP = 0, class F>
int with_op(int op, F&& f) {
  if constexpr (OP < 4) {
    if (op != OP) return with_op<OP + 1>(op, f);
  }
  return f(std::integral_constant<int, OP>{});
}

// the five models
template <class F>
int with_model(int model, F&& f) {
  switch (model) {
    case MMRE_TRANSE_L1: return f(std::integral_constant<int, MMRE_TRANSE_L1>{});
    case MMRE_TRANSE_L2: return f(std::integral_constant<int, MMRE_TRANSE_L2>{});
    case MMRE_DISTMULT: return f(std::integral_constant<int, MMRE_DISTMULT>{});
    case MMRE_COMPLEX: return f(std::integral_constant<int, MMRE_COMPLEX>{});
    case MMRE_ROTATE: return f(std::integral_constant<int, MMRE_ROTATE>{});
    default: return MMRE_ERR_MODEL;
  }
}

}  // namespace mmre
