// guided.hip — the device half of the filtering adaptive forms' own steps (guided.hpp): the launch code of guided_kernels.hpp.  One
// translation unit for every precision: its kernels only widen the packed means, so they need no copy per arithmetic build.
#include "guided.hpp"
#include "guided_kernels.hpp"

namespace rt {

static dim3 guided_grid(uint32_t width, uint32_t height) { return dim3((width + 31) / 32, (height + 7) / 8); }

int guided_lattice_launch(uint8_t* d_alive, uint32_t pixels_per_rank, uint32_t width, uint32_t height, uint32_t level, hipStream_t stream) {
    rttnw_tile_layout L;
    fill_layout(width, height, 1, L);
    HIP_TRY(hipMemsetAsync(d_alive, 0, pixels_per_rank, stream));
    hipLaunchKernelGGL(guided_lattice_kernel, guided_grid(width, height), dim3(32, 8), 0, stream, d_alive, width, height, L.tiles_x, level);
    HIP_TRY(hipGetLastError());
    return RTTNW_OK;
}

int guided_raw_launch(uint32_t precision, const void* d_means, const double* d_aux, double* d_mean, double* d_variance, double* d_raw_stderr, uint32_t* d_spp,
                      uint8_t* d_valid, uint32_t width, uint32_t height, hipStream_t stream) {
    rttnw_tile_layout L;
    fill_layout(width, height, 1, L);
    if (precision == RTTNW_F32)
        hipLaunchKernelGGL(guided_raw_kernel<float>, guided_grid(width, height), dim3(32, 8), 0, stream, (const float*)d_means, d_aux, d_mean, d_variance,
                           d_raw_stderr, d_spp, d_valid, width, height, L.tiles_x);
    else
        hipLaunchKernelGGL(guided_raw_kernel<double>, guided_grid(width, height), dim3(32, 8), 0, stream, (const double*)d_means, d_aux, d_mean, d_variance,
                           d_raw_stderr, d_spp, d_valid, width, height, L.tiles_x);
    HIP_TRY(hipGetLastError());
    return RTTNW_OK;
}

int guided_stop_launch(const double* d_den, const double* d_var_f, const double* d_raw_stderr, double rel_error, double abs_error, uint8_t* d_alive,
                       double* d_stderr_f, uint32_t width, uint32_t height, hipStream_t stream) {
    rttnw_tile_layout L;
    fill_layout(width, height, 1, L);
    hipLaunchKernelGGL(guided_stop_kernel, guided_grid(width, height), dim3(32, 8), 0, stream, d_den, d_var_f, d_raw_stderr, rel_error, abs_error, d_alive,
                       d_stderr_f, width, height, L.tiles_x);
    HIP_TRY(hipGetLastError());
    return RTTNW_OK;
}

} // namespace rt
