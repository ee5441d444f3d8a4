// features_f64_strict.hip — rttnw_render_features in the IEEE-strict build of the f64 arithmetic (rt_core.hpp RT_STRICT_F64, namespace
// rt::ieee_strict; precision RTTNW_F64_STRICT), under render_f64_strict.hip's flags: nothing contracted, every quotient an IEEE division.
#define RT_STRICT_F64 1
#if defined(__FAST_MATH__)
#error "features_f64_strict.hip must not be built with fast-math flags: its results are the CPU reference's bit for bit"
#endif
#pragma clang fp contract(off)
#include "feature_kernels.hpp"

namespace rt {
inline namespace RT_ARITH_NS {
RT_FEATURE_ENTRY_POINTS(RT_INSTANTIATE_T, double)
} // namespace RT_ARITH_NS
} // namespace rt
