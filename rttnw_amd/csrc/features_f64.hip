// features_f64.hip — the F64 (contracted) instantiation of rttnw_render_features' kernels and launch code (feature_kernels.hpp), under
// render_f64.hip's flags.
#include "feature_kernels.hpp"

namespace rt {
inline namespace RT_ARITH_NS {
template int render_features_t<double>(::rttnw_scene*, const rttnw_camera_desc*, const rttnw_params*, double*, double*, double*, double*, rttnw_stats*);
} // namespace RT_ARITH_NS
} // namespace rt
