// adaptive_launch.hpp — launch code of one precision for the adaptive and region renders: what they launch around render_tiles_t's passes
// (render_tiles.hpp) from adaptive_kernels.hpp, and rttnw_render_region's body.  The steps that compute nothing in the arithmetic type are
// pixel_lists.hpp's plain functions.  Included by the render units only.
#pragma once
#include "render_tiles.hpp"
#include "pixel_lists.hpp"

namespace rt {
inline namespace RT_ARITH_NS {

// The blocking form of enqueue_quad_list (pixel_lists.hpp) that the single-device entry points use, in d->list_quads / d->list_scan (grown here): one 8-byte
// copy gives the host the list's length and the number of marked pixels.
inline int build_quad_list(DeviceState* d, const uint8_t* marks, uint32_t n_blocks, hipStream_t stream, uint32_t& n_listed, uint32_t& n_marked) {
    HIP_TRY(d->list_quads.grow(size_t(n_blocks) * sizeof(uint32_t)));
    HIP_TRY(d->list_scan.grow(quad_scan_words(n_blocks) * sizeof(uint32_t)));
    if (int rc = enqueue_quad_list(marks, n_blocks, (uint32_t*)d->list_scan.p, (uint32_t*)d->list_quads.p, stream)) return rc;
    uint32_t count[2] = {0, 0}; // listed blocks, marked pixels
    HIP_TRY(hipMemcpy(count, quad_list_totals((uint32_t*)d->list_scan.p, n_blocks), sizeof(count), hipMemcpyDeviceToHost));
    n_listed = count[0];
    n_marked = count[1];
    return 0;
}

// rttnw_render_adaptive (include/rttnw_hip.h has the contract, DESIGN.md "Adaptive sampling" the why).  Pass k traces samples
// [sample_begin + kB, sample_begin + (k+1)B) of every active pixel with render_tiles_t's own kernel choice, chunk schedule and launch split:
// pass 0 over every pixel, in the plain render's job numbering; pass k > 0 over the list of 2x2 blocks that hold an active pixel, built on the
// device after each pass (one 8-byte copy to the host per pass: the list's length sizes the next pass).  Arguments were checked by the caller.
template <typename R>
int render_adaptive_t(::rttnw_scene* s, const rttnw_camera_desc* cam, const rttnw_params* p, const rttnw_adaptive* a, rttnw_stats* stats) {
    DeviceState* d = s->device;
    HIP_TRY(hipSetDevice(d->device));
    rttnw_tile_layout L;
    fill_layout(p->width, p->height, 1, L);
    const size_t npx = size_t(p->width) * p->height;
    const uint32_t n_blocks = L.n_tiles * 16u;
    HIP_TRY(d->packed.grow(size_t(L.pixels_per_rank) * 4 * sizeof(R)));
    HIP_TRY(d->linear.grow(npx * 3 * sizeof(R)));
    HIP_TRY(d->rgba.grow(npx * 4));
    HIP_TRY(d->ad_state.grow(size_t(L.pixels_per_rank) * sizeof(AdaptivePixel)));
    HIP_TRY(d->ad_active.grow(L.pixels_per_rank));
    HIP_TRY(d->ad_spp.grow(npx * sizeof(uint32_t)));
    HIP_TRY(d->ad_stderr.grow(npx * 3 * sizeof(double)));

    ListPass ad;
    ad.state = (AdaptivePixel*)d->ad_state.p;
    ad.active = d->ad_active.p;
    ad.cap = p->spp;
    ad.rel_error = a->rel_error;
    ad.abs_error = a->abs_error;
    rttnw_params pass = *p;
    pass.spp = a->pass_spp;
    const hipStream_t stream = nullptr;
    const uint32_t n_passes = p->spp / a->pass_spp;
    uint64_t samples = uint64_t(npx) * a->pass_spp;
    for (uint32_t k = 0; k < n_passes; ++k) {
        pass.sample_begin = p->sample_begin + k * a->pass_spp;
        if (k > 0) {
            uint32_t n_active = 0;
            if (int rc = build_quad_list(d, ad.active, n_blocks, stream, ad.n_quads, n_active)) return rc;
            if (ad.n_quads == 0) break; // every pixel is done
            ad.quads = (const uint32_t*)d->list_quads.p;
            ad.first = false;
            samples += uint64_t(n_active) * a->pass_spp;
        }
        // (pass 0 fills `stats` as a plain render does — kernel form, scene sizes — and starts its clock)
        if (int rc = render_tiles_t<R>(s, d, cam, &pass, d->packed.p, stream, k == 0 ? stats : nullptr, false, false, &ad)) return rc;
    }
    dim3 block(32, 8), grid((p->width + 31) / 32, (p->height + 7) / 8);
    hipLaunchKernelGGL(adaptive_output_kernel<R>, grid, block, 0, stream, (R*)d->packed.p, (const AdaptivePixel*)ad.state, (uint32_t*)d->ad_spp.p,
                       (double*)d->ad_stderr.p, p->width, p->height, L.tiles_x);
    HIP_TRY(hipGetLastError());
    if (stats) HIP_TRY(hipEventRecord(d->ev1.get(), stream));
    if (int rc = untile_launch<R>(p->width, p->height, 1, d->packed.p, d->linear.p, d->rgba.p, stream)) return rc;
    HIP_TRY(hipDeviceSynchronize());
    if (stats) {
        float ms = 0;
        HIP_TRY(hipEventElapsedTime(&ms, d->ev0.get(), d->ev1.get()));
        stats->kernel_ms = ms;
        stats->samples = samples;
    }
    return RTTNW_OK;
}

// What rttnw_render_adaptive_multi and its kin launch behind a rank's passes (render_adaptive_api.cpp has the loops; the passes themselves are
// render_tiles_t's): the rank's packed sums and noise state to means and auxiliary records ...
template <typename R>
int adaptive_finish_launch(void* d_packed, const void* d_state, double* d_aux, uint32_t pixels_per_rank, uint32_t rank_pixels, hipStream_t stream) {
    hipLaunchKernelGGL(adaptive_finish_packed_kernel<R>, dim3((pixels_per_rank + 255u) / 256u), dim3(256), 0, stream, (R*)d_packed,
                       (const AdaptivePixel*)d_state, d_aux, pixels_per_rank, rank_pixels);
    HIP_TRY(hipGetLastError());
    return RTTNW_OK;
}

// ... and, where a state comes in or goes out (rttnw_render_adaptive_resume): a rank's packed state records to its running sums, noise state and
// active bytes; the same back, before adaptive_finish_launch turns the sums into means.
template <typename R>
int adaptive_state_import_launch(const double* d_records, void* d_packed, void* d_state, uint8_t* d_active, uint32_t pixels_per_rank, uint32_t cap,
                                 double rel_error, double abs_error, hipStream_t stream) {
    hipLaunchKernelGGL(adaptive_state_import_kernel<R>, dim3((pixels_per_rank + 255u) / 256u), dim3(256), 0, stream, d_records, (R*)d_packed,
                       (AdaptivePixel*)d_state, d_active, pixels_per_rank, cap, rel_error, abs_error);
    HIP_TRY(hipGetLastError());
    return RTTNW_OK;
}
template <typename R>
int adaptive_state_export_launch(const void* d_packed, const void* d_state, double* d_records, uint32_t pixels_per_rank, uint32_t rank_pixels,
                                 hipStream_t stream) {
    hipLaunchKernelGGL(adaptive_state_export_kernel<R>, dim3((pixels_per_rank + 255u) / 256u), dim3(256), 0, stream, (const R*)d_packed,
                       (const AdaptivePixel*)d_state, d_records, pixels_per_rank, rank_pixels);
    HIP_TRY(hipGetLastError());
    return RTTNW_OK;
}
// The stats record of a rank that starts from a state: what pass 0 of a fresh render reports of the scene and the kernel form (its
// plan: render_tiles_t's for a pass that is not listed), with no samples yet — a resumed render has no pass 0 to fill it.
template <typename R>
int adaptive_rank_stats_t(::rttnw_scene* s, DeviceState* d, const rttnw_params* p, rttnw_stats* stats) {
    const FlatScene* flat = nullptr;
    DeviceScene<R>* ds = nullptr;
    if (int rc = bind_scene<R>(s, d, flat, ds)) return rc;
    rttnw_tile_layout L;
    fill_layout(p->width, p->height, p->tile_world, L);
    const RenderConsts rc = base_consts(p, *flat, L);
    if (int g = fill_stats<R>(d, *ds, *flat, plan_for<R>(*flat, false, false), rc, false, nullptr, stats)) return g;
    stats->samples = 0;
    return RTTNW_OK;
}

// rttnw_render_adaptive_region, on the root: the window's four outputs from the gathered means and auxiliary records.
template <typename R>
int adaptive_region_window_launch(uint32_t width, uint32_t height, uint32_t world, const void* d_gathered, const double* d_gathered_aux, void* d_linear_rgb,
                                  uint8_t* d_rgba8, uint32_t* d_spp, double* d_stderr, uint32_t x0, uint32_t y0, uint32_t x1, uint32_t y1,
                                  hipStream_t stream) {
    rttnw_tile_layout L;
    fill_layout(width, height, world, L);
    dim3 block(32, 8), grid((x1 - x0 + 31) / 32, (y1 - y0 + 7) / 8);
    hipLaunchKernelGGL(adaptive_region_window_kernel<R>, grid, block, 0, stream, (const R*)d_gathered, d_gathered_aux, (R*)d_linear_rgb, d_rgba8, d_spp,
                       d_stderr, L.tiles_x, world, L.pixels_per_rank, x0, y0, x1, y1);
    HIP_TRY(hipGetLastError());
    return RTTNW_OK;
}

// rttnw_render_region (include/rttnw_hip.h has the contract, DESIGN.md §10c the why).  The selected pixels of the window become the list of 2x2
// blocks that hold one (pixel_lists.hpp: region_select_launch, then the list build; one 8-byte copy gives the host the list's length), and
// render_tiles_t traces that list with its own kernel choice, chunk schedule and launch split — the jobs rttnw_render runs for those pixels.
// The running sums are kept by list slot (d->rg_sums): beyond the selection byte nothing here scales with the frame.
// Arguments were checked by the caller.
template <typename R>
int render_region_t(::rttnw_scene* s, const rttnw_camera_desc* cam, const rttnw_params* p, uint32_t x0, uint32_t y0, uint32_t x1, uint32_t y1,
                    const uint8_t* mask, rttnw_stats* stats) {
    DeviceState* d = s->device;
    const FlatScene* flat = nullptr;
    DeviceScene<R>* ds = nullptr;
    if (int rc = bind_scene<R>(s, d, flat, ds)) return rc;
    rttnw_tile_layout L;
    fill_layout(p->width, p->height, 1, L);
    const RenderConsts rc = base_consts(p, *flat, L);
    const size_t wpx = size_t(x1 - x0) * (y1 - y0);
    HIP_TRY(d->rg_select.grow(L.pixels_per_rank));
    HIP_TRY(d->rg_linear.grow(wpx * 3 * sizeof(R)));
    HIP_TRY(d->rg_rgba.grow(wpx * 4));
    if (mask) HIP_TRY(d->rg_mask.grow(wpx));
    const hipStream_t stream = nullptr;
    if (stats) HIP_TRY(hipEventRecord(d->ev0.get(), stream));
    if (mask) HIP_TRY(hipMemcpy(d->rg_mask.p, mask, wpx, hipMemcpyHostToDevice)); // uploaded once, window-sized
    HIP_TRY(hipMemsetAsync(d->rg_linear.p, 0, wpx * 3 * sizeof(R), stream)); // what an unselected pixel of the window keeps
    HIP_TRY(hipMemsetAsync(d->rg_rgba.p, 0, wpx * 4, stream));
    if (int g = region_select_launch(p->width, p->height, p->tile_rank, p->tile_world, mask ? (const uint8_t*)d->rg_mask.p : nullptr, d->rg_select.p, x0, y0,
                                     x1, y1, stream)) return g;
    ListPass list;
    uint32_t n_selected = 0;
    if (int g = build_quad_list(d, d->rg_select.p, L.n_tiles * 16u, stream, list.n_quads, n_selected)) return g;
    if (list.n_quads != 0) {
        HIP_TRY(d->rg_sums.grow(size_t(list.n_quads) * 4 * 4 * sizeof(R)));
        list.quads = (const uint32_t*)d->list_quads.p;
        list.clock_started = true;
        // (fills `stats` as a plain render does: kernel form, scene sizes)
        if (int g = render_tiles_t<R>(s, d, cam, p, d->rg_sums.p, stream, stats, false, false, &list)) return g;
        hipLaunchKernelGGL(region_output_kernel<R>, dim3((list.n_quads * 4u + 255u) / 256u), dim3(256), 0, stream, (const R*)d->rg_sums.p, list.quads, rc,
                           list.n_quads * 4u, x0, y0, x1, y1, (R*)d->rg_linear.p, d->rg_rgba.p);
        HIP_TRY(hipGetLastError());
    } else if (stats) {
        // nothing selected: no trace launch; the stats say what a render of this scene would have run
        if (int g = fill_stats<R>(d, *ds, *flat, plan_for<R>(*flat, false, true), rc, false, stream, stats)) return g;
    }
    if (stats) HIP_TRY(hipEventRecord(d->ev1.get(), stream));
    HIP_TRY(hipDeviceSynchronize());
    if (stats) {
        float ms = 0;
        HIP_TRY(hipEventElapsedTime(&ms, d->ev0.get(), d->ev1.get()));
        stats->kernel_ms = ms;
        stats->samples = uint64_t(n_selected) * p->spp;
    }
    return RTTNW_OK;
}

} // namespace RT_ARITH_NS
} // namespace rt
