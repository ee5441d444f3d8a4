// features_f32.hip — the F32 instantiation of rttnw_render_features' kernels and launch code (feature_kernels.hpp), under render_f32.hip's flags.
#include "feature_kernels.hpp"

namespace rt {
inline namespace RT_ARITH_NS {
RT_FEATURE_ENTRY_POINTS(RT_INSTANTIATE_T, float)
} // namespace RT_ARITH_NS
} // namespace rt
