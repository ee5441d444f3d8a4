// pixel_lists.hpp — the steps of the adaptive and region renders that compute nothing in a render's arithmetic type: bytes per packed pixel (who is
// selected, marked, active), the list of 2x2 blocks over such bytes, and the auxiliary records' way to their maps.  Byte, integer and double code:
// ONE build for every precision (pixel_lists.hip has the kernels, and says what each writes).  Everything is enqueued on `stream`, nothing else:
// no allocation, no copy, no wait.
#pragma once
#include "render_common.hpp"

namespace rt {
// The list of the 2x2 blocks, of n_blocks > 0, that hold a marked pixel (`marks`: a byte per packed pixel), built on the device in `quads`
// (n_blocks words): per wave of blocks the counts, their scan, then the compaction (`scan`, quad_scan_words(n_blocks) words, holds the waves'
// counts of blocks and of pixels, the waves' bases and, at quad_list_totals, the two totals).
int enqueue_quad_list(const uint8_t* marks, uint32_t n_blocks, uint32_t* scan, uint32_t* quads, hipStream_t stream);
// The marks of one level of a resumed render: the active pixels that hold exactly level_n samples (d_state: the rank's AdaptivePixel records)
int adaptive_level_select_launch(const uint8_t* d_active, const void* d_state, uint8_t* d_marks, uint32_t n_pixels, uint32_t level_n, hipStream_t stream);
// On the root: the gathered auxiliary records (standard error r, g, b and the sample count) to the frame's samples and standard-error maps
int untile_aux_launch(uint32_t width, uint32_t height, uint32_t world, const double* d_gathered_aux, uint32_t* d_spp, double* d_stderr, hipStream_t stream);
// The selection bytes of rank tile_rank of tile_world over a width x height frame: the pixels of the window [x0, x1) x [y0, y1) whose mask byte is
// set (d_mask: window-sized, on this device; nullptr = the whole window) ...
int region_select_launch(uint32_t width, uint32_t height, uint32_t tile_rank, uint32_t tile_world, const uint8_t* d_mask, uint8_t* d_select, uint32_t x0,
                         uint32_t y0, uint32_t x1, uint32_t y1, hipStream_t stream);
// ... and, behind them and the state's import, the active bytes rttnw_render_adaptive_region starts from
int adaptive_region_activate_launch(uint32_t width, uint32_t height, uint32_t tile_rank, uint32_t tile_world, const uint8_t* d_mask, uint8_t* d_select,
                                    const void* d_state, uint8_t* d_active, uint32_t x0, uint32_t y0, uint32_t x1, uint32_t y1, hipStream_t stream);
} // namespace rt
