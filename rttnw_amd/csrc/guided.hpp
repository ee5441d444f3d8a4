// guided.hpp — what the filtering adaptive forms (render_adaptive_api.cpp: rttnw_render_adaptive_denoised, rttnw_render_preview,
// rttnw_render_adaptive_budget_denoised; include/rttnw_hip.h has the contracts, DESIGN.md §10a "filter-guided form" the why) launch before their rounds,
// between a round's trace and its filter, and behind the filter: guided.hip holds the launch code, guided_kernels.hpp the kernels.
// Everything is enqueued on `stream` — no allocation, no copy, no wait — over buffers of the caller's on one device; the frame lives on ONE rank
// (packed order: tile * 64 + y * 8 + x, tiles in the permuted order of a single rank).
#pragma once
#include "render_common.hpp"

namespace rt {

// Before round 0: the alive byte of every packed pixel — 1 for the pixels of the image on the lattice x % 2^level == 0 && y % 2^level == 0
// (level 0: all of them), 0 for the others and for the rest of an edge tile.
int guided_lattice_launch(uint8_t* d_alive, uint32_t pixels_per_rank, uint32_t width, uint32_t height, uint32_t level, hipStream_t stream);
// Behind a round's trace: the packed means (adaptive_finish_packed_kernel's, reals of `precision`) and auxiliary records (standard error r, g, b
// and n) to what the filter reads and the call reports — row-major doubles: mean w*h*3, variance = stderr * stderr w*h*3, the standard errors
// themselves w*h*3, the sample counts w*h and, where d_valid is not nullptr, the valid byte (count > 0) of every pixel, w*h bytes.
int guided_raw_launch(uint32_t precision, const void* d_means, const double* d_aux, double* d_mean, double* d_variance, double* d_raw_stderr, uint32_t* d_spp,
                      uint8_t* d_valid, uint32_t width, uint32_t height, hipStream_t stream);
// Behind a round's filter: sqrt of the filtered variance for every pixel (w*h*3), and the alive byte of every alive pixel under the stopping rule.
int guided_stop_launch(const double* d_den, const double* d_var_f, const double* d_raw_stderr, double rel_error, double abs_error, uint8_t* d_alive,
                       double* d_stderr_f, uint32_t width, uint32_t height, hipStream_t stream);

} // namespace rt
