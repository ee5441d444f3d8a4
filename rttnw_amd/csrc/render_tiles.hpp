// render_tiles.hpp — launch code of one precision: rttnw_render_tiles_device's body (passes, kernel selection, workspace),
// the per-bounce probe and the un-tile launch, as templates over the arithmetic type.  (adaptive_launch.hpp: what the adaptive and region renders
// launch around render_tiles_t's passes.)
#pragma once
#include "trace_kernels.hpp"
#include "adaptive_kernels.hpp" // resolve_pass launches a list pass's resolve step

namespace rt {
inline namespace RT_ARITH_NS {

// The lane-owns-path kernel of a plan: its instantiation by what the scene holds (launch_plan.hpp plan_launch says why each exists).
template <typename R, bool LDSN, int SHAPES, bool LIST> const void* plain_kernel(const LaunchPlan& pl) {
    constexpr int BLOCK = !LDSN ? TRACE_BLOCK : sizeof(R) == 4 ? 1024 : RT_F64_BLOCK;
    if constexpr (!LIST && (SHAPES == SHAPES_FAST || SHAPES == SHAPES_GENERAL)) // (the only shapes that tally)
        if (pl.count) return (const void*)trace_kernel_plain<R, true, BLOCK, LDSN, SHAPES>;
    if constexpr (LDSN && SHAPES != SHAPES_FAST && SHAPES != SHAPES_GENERAL) // (run-ahead: the walks that never change frames, launch_plan.hpp)
        if (pl.run_ahead) return (const void*)trace_kernel_plain<R, false, BLOCK, true, SHAPES, RUN_AHEAD_STEPS, LIST, true>;
    if constexpr (LDSN)
        if (pl.steps == RT_TINY_TREE_STEPS) return (const void*)trace_kernel_plain<R, false, BLOCK, true, SHAPES, RT_TINY_TREE_STEPS, LIST>;
    return (const void*)trace_kernel_plain<R, false, BLOCK, LDSN, SHAPES, RT_NODE_STEPS, LIST>;
}
template <typename R, bool LIST> const void* plain_kernel_of(const LaunchPlan& pl) {
    if (!pl.lds) return pl.shapes == SHAPES_GENERAL ? plain_kernel<R, false, SHAPES_GENERAL, LIST>(pl) : plain_kernel<R, false, SHAPES_FAST, LIST>(pl);
    switch (pl.shapes) {
    case SHAPES_NONE: return plain_kernel<R, true, SHAPES_NONE, LIST>(pl);
    case SHAPES_SINGLE: return plain_kernel<R, true, SHAPES_SINGLE, LIST>(pl);
    case SHAPES_NONE_NT: return plain_kernel<R, true, SHAPES_NONE_NT, LIST>(pl);
    case SHAPES_SINGLE_NT: return plain_kernel<R, true, SHAPES_SINGLE_NT, LIST>(pl);
    default: return pl.shapes == SHAPES_GENERAL ? plain_kernel<R, true, SHAPES_GENERAL, LIST>(pl) : plain_kernel<R, true, SHAPES_FAST, LIST>(pl);
    }
}
// ... and the decoupled kernel's
template <typename R, bool LIST> const void* wave_kernel_of(const LaunchPlan& pl) {
    if constexpr (!LIST)
        if (pl.count) return pl.shapes == SHAPES_GENERAL ? (const void*)trace_kernel<R, true, SHAPES_GENERAL> : (const void*)trace_kernel<R, true, SHAPES_FAST>;
    switch (pl.shapes) {
    case SHAPES_GENERAL: return (const void*)trace_kernel<R, false, SHAPES_GENERAL, LIST>;
    case SHAPES_NONE: return (const void*)trace_kernel<R, false, SHAPES_NONE, LIST>;
    case SHAPES_NONE_NT: return (const void*)trace_kernel<R, false, SHAPES_NONE_NT, LIST>;
    default: return (const void*)trace_kernel<R, false, SHAPES_FAST, LIST>;
    }
}
// The active-list instantiations take their list of 2x2 blocks in the kernels' `counters` argument, which they never read as counters
// (trace_kernels.hpp TraceArgsList): every other launch passes the counters behind the job counter.
inline DeviceCounters* counters_argument(DeviceState* d, const LaunchPlan& pl, const uint32_t* quads) {
    return pl.list ? (DeviceCounters*)quads : reinterpret_cast<DeviceCounters*>(d->job_counter.p + 1);
}

// The chunk-sum workspace of a render and how many of its chunks one launch traces (rt_types.hpp launch_chunks: the chunk sums of a
// launch stay within the device's budget; the resolve step continues every pixel's chain, so the image does not depend on the split).
// (if the device cannot give the workspace — other tenants of its memory — the budget is halved, down to 1 GiB: more launches, same image)
// The budget that worked is REMEMBERED (d->chunk_budget): a later render does not retry the allocation that failed, and the
// buffer in hand is released only once a larger one has been obtained — or, if none can be, simply used: the launch split
// then follows ITS size.
template <typename R>
int size_chunk_sums(DeviceState* d, uint64_t sum_pixels, uint32_t total_chunks, uint32_t& per_launch) {
    const bool pinned = getenv("RTTNW_CHUNK_SUM_BUDGET") != nullptr; // (launch_chunks() then follows the environment, so no other budget is tried or remembered)
    for (uint64_t budget = d->chunk_budget;; budget /= 2) {
        per_launch = launch_chunks(sum_pixels, 3 * sizeof(R), total_chunks, budget);
        const size_t want = std::max<size_t>(size_t(sum_pixels) * std::min(per_launch, total_chunks), 1) * 3 * sizeof(R);
        if (d->partial.n >= want && d->partial.p) break;
        DevBuf<uint8_t> bigger;
        const hipError_t e = bigger.grow(want);
        if (e == hipSuccess) {
            d->partial = bigger;
            if (!pinned) d->chunk_budget = budget;
            break;
        }
        (void)hipGetLastError(); // clear the sticky out-of-memory
        const size_t one_group = size_t(sum_pixels) * std::min<uint32_t>(16u, total_chunks) * 3 * sizeof(R);
        // (not when pinned: launch_chunks() would size the launches by the environment's budget again, not by the buffer in hand)
        if (d->partial.p && d->partial.n >= one_group && !pinned) { // no larger buffer to be had: split the render by the one in hand
            per_launch = launch_chunks(sum_pixels, 3 * sizeof(R), total_chunks, d->partial.n);
            d->chunk_budget = std::max<uint64_t>(d->partial.n, 1ull << 30);
            break;
        }
        if (budget <= (1ull << 30) || pinned) { set_last_error(std::string("render: no memory for the chunk sums: ") + hipGetErrorString(e)); return RTTNW_ERR_HIP; }
    }
    return 0;
}

// The launch plan of a render of `flat` in this precision (launch_plan.hpp plan_launch, which reads no environment itself) under the experiment
// overrides: RTTNW_KERNEL=plain|plainglobal|wave names the form, RTTNW_WAVE_BLOCK=<threads> the decoupled LEAN flavour's block, RTTNW_RUN_AHEAD=0|1
// run-ahead in the lane-owns-path kernel's trips (launch_plan.hpp plan_launch).
template <typename R> LaunchPlan plan_for(const FlatScene& flat, bool count, bool listed) {
    const char* wave_block = getenv("RTTNW_WAVE_BLOCK");
    const char* ahead = getenv("RTTNW_RUN_AHEAD"); // 0 | 1: run-ahead off / on wherever an instantiation has it
    return plan_launch(flat, sizeof(R), count, listed, kernel_form_named(getenv("RTTNW_KERNEL")), wave_block ? atoi(wave_block) : 0,
                       ahead && (ahead[0] == '0' || ahead[0] == '1') && !ahead[1] ? ahead[0] - '0' : -1);
}

// One trace launch over the rc.n_jobs jobs of a pass: the workspace its grid needs, then the plan's kernel (prepare_only: the workspace alone).
template <typename R>
int launch_pass(DeviceState* d, DeviceScene<R>& ds, const FlatScene& flat, const LaunchPlan& pl, RenderConsts rc, CameraRec<R> cam, const rttnw_params* p,
                const uint32_t* quads, hipStream_t stream, bool prepare_only) {
    if (int q4 = pl.quantised ? ds.ensure_quant4(flat) : 0) return q4; // this kernel walks the quantised records: made here, on the device, once
    const void* kernel = pl.decoupled ? (pl.list ? wave_kernel_of<R, true>(pl) : wave_kernel_of<R, false>(pl))
                                      : (pl.list ? plain_kernel_of<R, true>(pl) : plain_kernel_of<R, false>(pl));
    if (pl.lds_bytes > LDS_BYTES_PER_CU) { set_last_error(pl.decoupled ? "render: queues + traversal stacks do not fit in LDS" : "render: traversal stacks do not fit in LDS"); return RTTNW_ERR_UNSUPPORTED; }
    HIP_TRY(hipFuncSetAttribute(kernel, hipFuncAttributeMaxDynamicSharedMemorySize, int(pl.lds_bytes)));
    int blocks_per_cu = 0;
    HIP_TRY(hipOccupancyMaxActiveBlocksPerMultiprocessor(&blocks_per_cu, kernel, pl.block, pl.lds_bytes));
    // (the decoupled kernel's also by LDS granules: the runtime's answer counts LDS in finer units than the hardware allocates it in, lds_blocks_per_cu)
    blocks_per_cu = std::max(1, std::min(blocks_per_cu, pl.decoupled ? std::min(8, int(lds_blocks_per_cu(pl.lds_bytes))) : 8));
    // what the chip holds at once (no inter-workgroup dependency, so a little over-subscription is harmless), but never more waves than there is work
    // for: a wave of the decoupled kernel feeds SLOTS_PER_WAVE jobs at a time, a wave of the lane-owns-path kernel 64
    const size_t n_jobs = rc.n_jobs, waves_needed = (n_jobs + (pl.decoupled ? SLOTS_PER_WAVE : 64u) - 1) / (pl.decoupled ? SLOTS_PER_WAVE : 64u);
    const size_t waves_per_block = size_t(pl.block) / 64, blocks_needed = (waves_needed + waves_per_block - 1) / waves_per_block;
    const size_t grid = std::max<size_t>(1, std::min<size_t>(size_t(d->num_cus) * blocks_per_cu, blocks_needed));
    uint32_t n_slots = 0;
    if (pl.decoupled) {
        n_slots = uint32_t(grid * size_t(pl.block / 64) * SLOTS_PER_WAVE);
        HIP_TRY(d->pool_r.grow(size_t(n_slots) * PR_COUNT * sizeof(R)));
        HIP_TRY(d->pool_u.grow(size_t(n_slots) * PU_COUNT * sizeof(uint32_t)));
    }
    // stack entries beyond the LDS-resident ones, for every thread of the launch
    const uint32_t lds_entries = pl.decoupled ? wave_stack_entries<R>() : LDS_STACK_ENTRIES;
    const size_t extra = rc.stack_depth > lds_entries ? rc.stack_depth - lds_entries : 0;
    HIP_TRY(d->spill.grow(std::max<size_t>(grid * size_t(pl.block) * extra, 1) * sizeof(int32_t)));
    if (n_jobs == 0 || prepare_only) return 0;
    SceneView<R> view = pl.decoupled ? ds.decoupled_view() : ds.view;
    R bg0 = R(p->background[0]), bg1 = R(p->background[1]), bg2 = R(p->background[2]), tmin = R(p->t_min);
    R *part = (R*)d->partial.p, *pool_r = (R*)d->pool_r.p;
    unsigned long long* jc = d->job_counter.p;
    DeviceCounters* dc = counters_argument(d, pl, quads);
    uint32_t* pool_u = (uint32_t*)d->pool_u.p;
    int32_t* sp = (int32_t*)d->spill.p;
    void* plain_args[] = {&view, &cam, &rc, &bg0, &bg1, &bg2, &tmin, &part, &jc, &dc, &sp};
    void* wave_args[] = {&view, &cam, &rc, &bg0, &bg1, &bg2, &tmin, &part, &jc, &dc, &pool_r, &pool_u, &n_slots, &sp};
    HIP_TRY(hipLaunchKernel(kernel, dim3(uint32_t(grid)), dim3(uint32_t(pl.block)), pl.decoupled ? wave_args : plain_args, pl.lds_bytes, stream));
    return 0;
}

// ... and the step behind it: the pass's chunk sums continue every pixel's chain in d_packed (an adaptive pass: and its noise state; a
// region render: in the running sums by list slot)
template <typename R>
int resolve_pass(DeviceState* d, const RenderConsts& rc, const rttnw_tile_layout& L, const ListPass* ad, void* d_packed, bool first, bool last, hipStream_t stream) {
    if (ad && !ad->state)
        hipLaunchKernelGGL(region_resolve_kernel<R>, dim3((rc.jobs_per_chunk + 255) / 256), dim3(256), 0, stream, (const R*)d->partial.p, (R*)d_packed,
                           ad->quads, rc.n_chunks, rc.jobs_per_chunk, uint32_t(first), uint32_t(last), rc.spp);
    else if (ad)
        hipLaunchKernelGGL(adaptive_resolve_kernel<R>, dim3((rc.jobs_per_chunk + 255) / 256), dim3(256), 0, stream, (const R*)d->partial.p, (R*)d_packed,
                           ad->state, ad->active, ad->quads, rc, rc.jobs_per_chunk, uint32_t(first && ad->first), uint32_t(last), ad->cap, ad->rel_error,
                           ad->abs_error);
    else
        hipLaunchKernelGGL(resolve_kernel<R>, dim3((L.pixels_per_rank + 255) / 256), dim3(256), 0, stream, (const R*)d->partial.p, (R*)d_packed, rc,
                           L.pixels_per_rank, uint32_t(first), uint32_t(last), rc.spp);
    HIP_TRY(hipGetLastError());
    return 0;
}

// rttnw_stats of a render (kernel_ms and the counters only where the caller lets this call wait for the stream)
template <typename R>
int fill_stats(DeviceState* d, const DeviceScene<R>& ds, const FlatScene& flat, const LaunchPlan& pl, const RenderConsts& rc, bool sync_for_stats,
               hipStream_t stream, rttnw_stats* stats) {
    std::memset(stats, 0, sizeof(*stats));
    if (sync_for_stats) {
        HIP_TRY(hipStreamSynchronize(stream));
        float ms = 0;
        HIP_TRY(hipEventElapsedTime(&ms, d->ev0.get(), d->ev1.get()));
        stats->kernel_ms = ms;
    }
    // samples traced by this rank: pixels of its tiles that lie inside the image
    uint64_t px_count = 0;
    for (uint32_t t = 0; t < rc.my_tiles; ++t) {
        uint32_t tx, ty;
        tile_unpermute(rc.tile_rank + t * rc.tile_world, rc.tiles_x, tx, ty);
        uint32_t w = std::min(8u, rc.width - tx * 8), h = std::min(8u, rc.height - ty * 8);
        px_count += uint64_t(w) * h;
    }
    stats->samples = px_count * rc.spp;
    if (pl.count && sync_for_stats) {
        DeviceCounters hc;
        HIP_TRY(hipMemcpy(&hc, d->job_counter.p + 1, sizeof(hc), hipMemcpyDeviceToHost));
        stats->rays = hc.rays; stats->nodes_visited = hc.nodes; stats->prims_tested = hc.prims; stats->texel_fetches = hc.texels;
        if (getenv("RTTNW_DEBUG_SCHED")) debug_print_sched(hc, !pl.decoupled, rc.profile, stats->samples); // (debug_sched.cpp)
    }
    stats->n_nodes = flat.total_nodes4();
    stats->n_prims = flat.n_prims_in_bvh;
    stats->scene_bytes = uint32_t(std::min<size_t>(ds.bytes, 0xFFFFFFFFu));
    stats->reserved = pl.form_bits | (pl.decoupled && ds.interleaved ? FORM_INTERLEAVED : 0u) | (pl.run_ahead ? FORM_RUN_AHEAD : 0u); // which kernel form ran (launch_plan.hpp FORM_*)
    return 0;
}

// A render's steps: bind the scene, fill the constants, size the chunk-sum workspace, plan the launch (ONCE: launch_plan.hpp), then per launch
// of the split the trace pass and its resolve step; the stats at the end.
// prepare_only: upload the scene on first use and grow every workspace buffer this render will need (blocking
// allocations, copies and frees), launch nothing — rttnw_render_multi does that for ALL its ranks before the first launch, so
// that no allocation (a device-wide synchronisation) sits between two ranks' kernels.
template <typename R>
int render_tiles_t(::rttnw_scene* s, DeviceState* d, const rttnw_camera_desc* cam, const rttnw_params* p, void* d_packed, hipStream_t stream,
                   rttnw_stats* stats, bool sync_for_stats, bool prepare_only, const ListPass* ad) {
    const FlatScene* flat = nullptr;
    DeviceScene<R>* ds = nullptr;
    if (int rc = bind_scene<R>(s, d, flat, ds)) return rc;
    rttnw_tile_layout L;
    fill_layout(p->width, p->height, p->tile_world, L);
    RenderConsts rc = base_consts(p, *flat, L);
    // The render's chunk schedule (a function of spp alone)
    plan_chunks(rc, p->spp, p->spp_chunk);
    const uint32_t total_chunks = rc.n_chunks;
    // (an adaptive refinement pass and a region render keep the sums of their listed blocks only: 4 per block and chunk)
    const bool listed = ad && ad->quads, count = p->collect_counters != 0;
    if (listed && count) { set_last_error("render: an active-list pass cannot collect counters"); return RTTNW_ERR_UNSUPPORTED; }
    uint32_t per_launch = 0;
    if (int g = size_chunk_sums<R>(d, listed ? uint64_t(ad->n_quads) * 4 : uint64_t(rc.my_tiles) * 64, total_chunks, per_launch)) return g;
    const CameraRec<R> camr = camera_of<R>(cam);
    const LaunchPlan pl = plan_for<R>(*flat, count, listed);
    rc.lds_nodes = pl.lds_nodes;
    // (a counting render at level >= 2 tallies the trips its timed twin takes: trace_tally.hpp; levels 0 and 1 keep the canonical walk and its counts)
    if (count && rc.profile >= 2u && plan_for<R>(*flat, false, listed).run_ahead) rc.scene_flags |= SCENE_TALLY_AHEAD;
    for (int k = 0; k < 6; ++k) rc.lds_recs[k] = pl.lds_recs[k];
    if (!prepare_only) HIP_TRY(hipMemsetAsync(d->job_counter.p, 0, sizeof(unsigned long long) + sizeof(DeviceCounters), stream));
    if (stats && !prepare_only && !(ad && ad->clock_started)) HIP_TRY(hipEventRecord(d->ev0.get(), stream));
    for (uint32_t c0 = 0; c0 < total_chunks; c0 += per_launch) {
        rc.chunk_base = c0;
        rc.n_chunks = std::min(per_launch, total_chunks - c0);
        const bool first = c0 == 0, last = c0 + per_launch >= total_chunks;
        if (!(listed ? plan_jobs_list(rc, ad->n_quads) : plan_jobs(rc))) { set_last_error("render: more than 2^32 jobs in a launch"); return RTTNW_ERR_UNSUPPORTED; }
        HIP_TRY(d->partial.grow(std::max<size_t>(size_t(rc.jobs_per_chunk) * rc.n_chunks, 1) * 3 * sizeof(R)));
        if (!first && !prepare_only) HIP_TRY(hipMemsetAsync(d->job_counter.p, 0, sizeof(unsigned long long), stream)); // the job counter only: statistics add up
        if (int g = launch_pass<R>(d, *ds, *flat, pl, rc, camr, p, listed ? ad->quads : nullptr, stream, prepare_only)) return g;
        if (prepare_only) continue;
        if (stats && last) HIP_TRY(hipEventRecord(d->ev1.get(), stream));
        if (int g = resolve_pass<R>(d, rc, L, ad, d_packed, first, last, stream)) return g;
    }
    if (prepare_only || !stats) return RTTNW_OK;
    return fill_stats<R>(d, *ds, *flat, pl, rc, sync_for_stats, stream, stats);
}

template <typename R>
int probe_path_t(::rttnw_scene* s, const rttnw_camera_desc* cam, const rttnw_params* p, uint32_t px, uint32_t row, uint32_t sample,
                 double* out, uint32_t max_out) {
    const FlatScene* flat = nullptr;
    DeviceScene<R>* ds = nullptr;
    if (int rc = bind_scene<R>(s, s->device, flat, ds)) return rc;
    rttnw_tile_layout L;
    fill_layout(p->width, p->height, p->tile_world, L);
    RenderConsts rc = base_consts(p, *flat, L);
    rc.sample_begin = 0; // the probe names its sample itself ...
    rc.scene_flags = 0;  // ... and reports the shutter draw of its ray whether or not the scene reads it
    DevBuf<double> d_out;
    DevBuf<int32_t> d_n, d_spill;
    HIP_TRY(d_out.upload(std::vector<double>(size_t(max_out) * PROBE_STRIDE + 4, 0.0)));
    HIP_TRY(d_n.upload(std::vector<int32_t>(1, 0)));
    HIP_TRY(d_spill.upload(std::vector<int32_t>(std::max<size_t>(rc.stack_depth, 1), 0)));
    const size_t lds = size_t(LDS_STACK_ENTRIES + 1) * 64 * sizeof(int32_t);
    hipLaunchKernelGGL(probe_path_kernel<R>, dim3(1), dim3(64), lds, 0, ds->view, camera_of<R>(cam), rc, R(p->t_min), px, row,
                       sample, d_out.p, max_out, d_n.p, d_spill.p);
    HIP_TRY(hipGetLastError());
    int32_t n = 0;
    HIP_TRY(hipMemcpy(&n, d_n.p, sizeof(n), hipMemcpyDeviceToHost));
    HIP_TRY(hipMemcpy(out, d_out.p, size_t(n) * PROBE_STRIDE * sizeof(double), hipMemcpyDeviceToHost));
    // radiance of the sample (path_step loop) is returned after the last possible bounce record
    HIP_TRY(hipMemcpy(out + size_t(max_out) * PROBE_STRIDE, d_out.p + size_t(max_out) * PROBE_STRIDE, 4 * sizeof(double), hipMemcpyDeviceToHost));
    return n;
}

template <typename R>
int untile_launch(uint32_t width, uint32_t height, uint32_t world, const void* d_gathered, void* d_linear_rgb, uint8_t* d_rgba8, hipStream_t stream) {
    rttnw_tile_layout L;
    fill_layout(width, height, world, L);
    dim3 block(32, 8), grid((width + 31) / 32, (height + 7) / 8);
    hipLaunchKernelGGL(untile_kernel<R>, grid, block, 0, stream, (const R*)d_gathered, (R*)d_linear_rgb, d_rgba8, width, height, L.tiles_x, world,
                       L.pixels_per_rank);
    HIP_TRY(hipGetLastError());
    return RTTNW_OK;
}

} // namespace RT_ARITH_NS
} // namespace rt
