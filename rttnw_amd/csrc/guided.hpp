// guided.hpp — what rttnw_render_adaptive_denoised (render_adaptive_api.cpp; include/rttnw_hip.h has the contract, DESIGN.md §10a "filter-guided form" the
// why) launches between a round's trace and its filter, and behind the filter: guided.hip holds the launch code, guided_kernels.hpp the kernels.
// Everything is enqueued on `stream` — no allocation, no copy, no wait — over buffers of the caller's on one device; the frame lives on ONE rank
// (packed order: tile * 64 + y * 8 + x, tiles in the permuted order of a single rank).
#pragma once
#include "render_common.hpp"

namespace rt {

// Before round 0: the alive byte of every packed pixel — 1 for the pixels of the image, 0 for the rest of an edge tile.
int guided_begin_launch(uint8_t* d_alive, uint32_t pixels_per_rank, uint32_t width, uint32_t height, hipStream_t stream);
// Behind a round's trace: the packed means (adaptive_finish_packed_kernel's, reals of `precision`) and auxiliary records (standard error r, g, b
// and n) to what the denoiser reads and the call reports — row-major doubles: mean w*h*3, variance = stderr * stderr w*h*3, the standard errors
// themselves w*h*3, and the sample counts w*h.
int guided_raw_launch(uint32_t precision, const void* d_means, const double* d_aux, double* d_mean, double* d_variance, double* d_raw_stderr, uint32_t* d_spp,
                      uint32_t width, uint32_t height, hipStream_t stream);
// Behind a round's filter: sqrt of the filtered variance for every pixel (w*h*3), and the alive byte of every alive pixel under the stopping rule.
int guided_stop_launch(const double* d_den, const double* d_var_f, const double* d_raw_stderr, double rel_error, double abs_error, uint8_t* d_alive,
                       double* d_stderr_f, uint32_t width, uint32_t height, hipStream_t stream);

} // namespace rt
