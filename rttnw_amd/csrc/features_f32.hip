// features_f32.hip — the F32 instantiation of rttnw_render_features' kernels and launch code (feature_kernels.hpp), under render_f32.hip's flags.
#include "feature_kernels.hpp"

namespace rt {
inline namespace RT_ARITH_NS {
template int render_features_t<float>(::rttnw_scene*, const rttnw_camera_desc*, const rttnw_params*, double*, double*, double*, double*, rttnw_stats*);
} // namespace RT_ARITH_NS
} // namespace rt
