// features_f64.hip — the F64 (contracted) instantiation of rttnw_render_features' kernels and launch code (feature_kernels.hpp), under
// render_f64.hip's flags.
#include "feature_kernels.hpp"

namespace rt {
inline namespace RT_ARITH_NS {
RT_FEATURE_ENTRY_POINTS(RT_INSTANTIATE_T, double)
} // namespace RT_ARITH_NS
} // namespace rt
