// render_adaptive_api.cpp — the adaptive family beyond rttnw_render_adaptive: the forms over the ranks of a node (multi, resume, region), the round driver
// of the forms that run one rank on the scene's device (RankRounds) and those forms (denoised, preview, budget, budget_denoised), and rttnw_budget_select.  Host code
// only; the kernels live in render_f32.hip / render_f64.hip, pixel_lists.hip (selection, marks and lists: one build for every precision), denoise.hip
// (the filter, with and without flags), guided.hip (the filtering forms' own steps) and budget.hip (the selection).
#include "render_multi.hpp"
#include "pixel_lists.hpp"
#include "adaptive_state.hpp"
#include "feature_api.hpp"
#include "guided.hpp"
#include "budget.hpp"

// ---------------------------------------------------------------------------------------------
// rttnw_render_adaptive_multi: rttnw_render_adaptive over the ranks of rttnw_render_multi (include/rttnw_hip.h has the contract, DESIGN.md §10a the
// why).  Rank r runs render_adaptive_t's passes over ITS tiles — render_tiles_t with tile_rank = r — but the loop is pass-major, rank-minor: a pass
// is enqueued on every live rank's stream before the host waits for any of them, so the devices of a node work side by side.
// rttnw_render_adaptive_resume is the same render begun from, and left as, a state (adaptive_node_render runs both): its passes go by LEVEL, the
// number of passes a pixel has behind it.  rttnw_render_adaptive_region is the resumed render over a SELECTION — a window of the frame, or a mask
// inside it —, where a pixel may hold no samples yet: only selected pixels are ever active, and the outputs are the window's.
// ---------------------------------------------------------------------------------------------
namespace rt {
// ---- refusals more than one entry point of this unit makes, each under the call's name
// Where rttnw_render_adaptive_multi (ngpu >= 1), rttnw_render_adaptive_resume and rttnw_render_adaptive_region (`allow_zero`: ngpu == 0 is the scene's
// own device) run: no device needed
static int refuse_ranks_misuse(const char* caller, bool allow_zero, uint32_t ngpu, const int32_t* device_ids) {
    const std::string call = std::string(caller) + ": ";
    if (ngpu > 64 || (!ngpu && !allow_zero)) { set_last_error(call + (allow_zero ? "ngpu must be 0 .. 64" : "ngpu must be 1 .. 64")); return RTTNW_ERR_INVALID; }
    if (ngpu && !device_ids) { set_last_error(call + (allow_zero ? "device_ids is NULL with ngpu >= 1" : "device_ids is NULL")); return RTTNW_ERR_INVALID; }
    if (!ngpu && device_ids) { set_last_error(call + "device_ids must be NULL with ngpu == 0 (the current device)"); return RTTNW_ERR_INVALID; }
    return 0;
}
// ... and, behind validate(), a device id nobody has
static int refuse_unknown_devices(const char* caller, uint32_t ngpu, const int32_t* device_ids) {
    const int n_dev = rttnw_device_count();
    for (uint32_t r = 0; r < ngpu; ++r)
        if (device_ids[r] < 0 || device_ids[r] >= n_dev) { set_last_error(std::string(caller) + ": no such device in device_ids"); return RTTNW_ERR_INVALID; }
    return 0;
}

// Where a call's level loop starts, and up to which level each rank must look even when a list comes back empty (a fresh render: level 0 only)
struct LevelPlan {
    bool resumed = false;
    uint32_t first = 0;         // the lowest level n / B a pixel of the state stands at
    std::vector<uint32_t> last; // per rank: the highest
};
// Where rank r keeps what lives across its passes: slots of its device's buffers, like MultiPlan::packed
struct AdaptiveSlots {
    rttnw_tile_layout L;
    size_t state_chunk = 0, active_chunk = 0, list_chunk = 0; // bytes of a rank's noise state, active bytes, list + scan
    size_t records_chunk = 0;                                 // rttnw_render_adaptive_resume: bytes of a rank's packed state records
    uint32_t tiles(uint32_t r, uint32_t world) const { return L.n_tiles > r ? (L.n_tiles - r + world - 1) / world : 0; } // the tiles rank r owns (base_consts' my_tiles)
    AdaptivePixel* state(const MultiPlan& m, uint32_t r) const { return (AdaptivePixel*)(m.ranks[r].d->multi_ad_state.p + state_chunk * m.ranks[r].slot); }
    uint8_t* active(const MultiPlan& m, uint32_t r) const { return m.ranks[r].d->multi_ad_active.p + active_chunk * m.ranks[r].slot; }
    uint32_t* quads(const MultiPlan& m, uint32_t r) const { return (uint32_t*)(m.ranks[r].d->multi_list.p + list_chunk * m.ranks[r].slot); }
    uint32_t* scan(const MultiPlan& m, uint32_t r) const { return quads(m, r) + size_t(L.tiles_per_rank) * 16; }
    double* records(const MultiPlan& m, uint32_t r) const { return (double*)(m.ranks[r].d->multi_ad_records.p + records_chunk * m.ranks[r].slot); }
    uint8_t* marks(const MultiPlan& m, uint32_t r) const { return m.ranks[r].d->multi_ad_marks.p + active_chunk * m.ranks[r].slot; }
    uint8_t* select(const MultiPlan& m, uint32_t r) const { return m.ranks[r].d->multi_ad_select.p + active_chunk * m.ranks[r].slot; }
};
// The selection of rttnw_render_adaptive_region: the window [x0, x1) x [y0, y1) of the frame and, optionally, the mask inside it (the caller's array)
struct RegionSelection {
    uint32_t x0, y0, x1, y1;
    const uint8_t* mask;
    size_t pixels() const { return size_t(x1 - x0) * (y1 - y0); }
    bool has(uint32_t x, uint32_t y) const { return x >= x0 && x < x1 && y >= y0 && y < y1 && (!mask || mask[size_t(y - y0) * (x1 - x0) + (x - x0)] != 0); }
    // is (x, y), a selected pixel, the first selected pixel of its 2x2 block in row-major order?  (counts the blocks a list can hold)
    bool opens_block(uint32_t x, uint32_t y) const {
        if ((x & 1u) && has(x - 1u, y)) return false;
        return !((y & 1u) && (has(x & ~1u, y - 1u) || has(x | 1u, y - 1u)));
    }
};
static ListPass adaptive_rank_pass(const MultiPlan& m, const AdaptiveSlots& sl, uint32_t r, const rttnw_params& p, const rttnw_adaptive& a) {
    ListPass ad;
    ad.state = sl.state(m, r);
    ad.active = sl.active(m, r);
    ad.cap = p.spp;
    ad.rel_error = a.rel_error;
    ad.abs_error = a.abs_error;
    return ad;
}

// multi_prepare for the adaptive passes: every buffer of every rank, and what a first use brings for pass 0 AND for a refinement pass over all of
// the rank's blocks — a list never holds more, so no later pass allocates (a hipMalloc between two ranks' launches would synchronise the device)
// (`resumed`: the render starts from a state, so it has no pass 0; `records`: a state comes in or goes out; `sel`, with `sel_blocks`: the region form —
// a rank's lists hold at most sel_blocks[r] blocks, those with a selected pixel, which sizes its chunk sums; the mask goes to every device once, the
// ranks get their selection bytes and the root the window's outputs in place of the frame's)
static int adaptive_multi_prepare(::rttnw_scene* s, const rttnw_camera_desc* cam, const rttnw_params& p, const rttnw_adaptive& a, const MultiPlan& m,
                                  const AdaptiveSlots& sl, bool resumed = false, bool records = false, const RegionSelection* sel = nullptr,
                                  const std::vector<uint32_t>* sel_blocks = nullptr) {
    if (int rc = multi_prepare_buffers(m, sel == nullptr)) return rc;
    for (size_t k = 0; k < m.devices.size(); ++k) {
        DeviceState* d = m.dev_state[k];
        HIP_TRY(hipSetDevice(d->device));
        HIP_TRY(d->multi_ad_state.grow(sl.state_chunk * m.dev_ranks[k]));
        HIP_TRY(d->multi_ad_active.grow(sl.active_chunk * m.dev_ranks[k]));
        HIP_TRY(d->multi_list.grow(sl.list_chunk * m.dev_ranks[k]));
        HIP_TRY(d->multi_aux.grow(m.aux_chunk * m.dev_ranks[k]));
        if (records) HIP_TRY(d->multi_ad_records.grow(sl.records_chunk * m.dev_ranks[k]));
        if (resumed) HIP_TRY(d->multi_ad_marks.grow(sl.active_chunk * m.dev_ranks[k]));
        if (!sel) continue;
        HIP_TRY(d->multi_ad_select.grow(sl.active_chunk * m.dev_ranks[k]));
        if (!sel->mask) continue;
        HIP_TRY(d->rg_mask.grow(sel->pixels()));
        HIP_TRY(hipMemcpy(d->rg_mask.p, sel->mask, sel->pixels(), hipMemcpyHostToDevice));
    }
    DeviceState* root = m.root;
    HIP_TRY(hipSetDevice(root->device));
    HIP_TRY(root->gathered_aux.grow(m.aux_chunk * m.ranks.size()));
    if (sel) {
        HIP_TRY(root->rg_linear.grow(sel->pixels() * 3 * m.rsz));
        HIP_TRY(root->rg_rgba.grow(sel->pixels() * 4));
        HIP_TRY(root->rg_spp.grow(sel->pixels() * sizeof(uint32_t)));
        HIP_TRY(root->rg_stderr.grow(sel->pixels() * 3 * sizeof(double)));
    } else {
        HIP_TRY(root->ad_spp.grow(m.npx * sizeof(uint32_t)));
        HIP_TRY(root->ad_stderr.grow(m.npx * 3 * sizeof(double)));
    }
    rttnw_params pr = p;
    pr.spp = a.pass_spp;
    for (uint32_t r = 0; r < m.ranks.size(); ++r) {
        pr.tile_rank = r;
        DeviceState* d = m.ranks[r].d;
        ListPass ad = adaptive_rank_pass(m, sl, r, p, a);
        if (!resumed)
            if (int rc = render_tiles_any(s, d, cam, &pr, m.packed(r), d->stream.get(), nullptr, false, true, &ad)) return rc;
        ad.quads = sl.quads(m, r);
        ad.n_quads = sel_blocks ? (*sel_blocks)[r] : sl.tiles(r, p.tile_world) * 16u;
        ad.first = false;
        if (ad.n_quads)
            if (int rc = render_tiles_any(s, d, cam, &pr, m.packed(r), d->stream.get(), nullptr, false, true, &ad)) return rc;
    }
    return 0;
}

struct HostFree { void operator()(void* q) const { (void)hipHostFree(q); } };

// The passes.  Per pass and live rank, on its device's stream between its two events: the trace launches and the adaptive resolve (render_tiles_t),
// the list of its blocks that still hold an active pixel — what its NEXT pass traces, in its own slot — and a copy of the list's two totals into
// the rank's pinned words.  Only then does the host wait, once per device, and read the totals: a rank whose list is empty takes no further part.
// A render begun from a state (lv.resumed) has pixels at several LEVELS (passes behind them), and level k traces the active pixels that stand at it:
// the step before the loop brings every rank's records in (`upload`: per rank, in its packed order) and lists level lv.first; each list is then
// made of the level's marks (adaptive_level_select_kernel) instead of the active bytes, a rank with an empty list stays in the loop while its
// state holds pixels at a higher level, and a rank with nothing to trace at a level launches no trace kernel.  A fresh render is the case of one
// level: the launches it always had.  With a selection (`sel`: rttnw_render_adaptive_region) the same step leaves only selected pixels active, those
// without samples among them, and lv.first / lv.last are the selected pixels' — level 0 is then a list pass like every other.
// `ms`: the ranks' device time so far; `refined`: samples they traced beyond a fresh render's pass 0.
static int adaptive_multi_passes(::rttnw_scene* s, const rttnw_camera_desc* cam, const rttnw_params& p, const rttnw_adaptive& a, const MultiPlan& m,
                                 const AdaptiveSlots& sl, const LevelPlan& lv, const RegionSelection* sel, const std::vector<std::vector<double>>& upload,
                                 std::vector<Event>& ev, uint32_t* counts, rttnw_stats* stats, std::vector<double>& ms, std::vector<uint64_t>& refined) {
    const uint32_t ngpu = uint32_t(m.ranks.size()), n_passes = p.spp / a.pass_spp;
    std::vector<uint32_t> n_quads(ngpu, 0);
    std::vector<char> live(ngpu);
    for (uint32_t r = 0; r < ngpu; ++r) live[r] = sl.tiles(r, ngpu) != 0;
    rttnw_params pr = p;
    pr.spp = a.pass_spp;
    // on rank r's stream: the list of what it traces at `level`, and the copy of the list's totals
    const auto enqueue_list = [&](uint32_t r, uint32_t level, hipStream_t stream) -> int {
        uint32_t* scan = sl.scan(m, r);
        const uint32_t n_blocks = sl.tiles(r, ngpu) * 16u; // (its own tiles only: no pass writes the active bytes of a pad tile)
        const uint8_t* marks = sl.active(m, r);
        if (lv.resumed) {
            if (int rc = adaptive_level_select_launch(marks, sl.state(m, r), sl.marks(m, r), n_blocks * 4u, level * a.pass_spp, stream)) return rc;
            marks = sl.marks(m, r);
        }
        if (int rc = enqueue_quad_list(marks, n_blocks, scan, sl.quads(m, r), stream)) return rc;
        HIP_TRY(hipMemcpyAsync(counts + 2 * r, quad_list_totals(scan, n_blocks), 2 * sizeof(uint32_t), hipMemcpyDeviceToHost, stream));
        return 0;
    };
    // the host waits for the step just enqueued, once per device with a live rank, and reads what it left: device time and — `listed`: the step
    // built the lists of `level` — the lists' totals.  Whether any rank goes on.
    const auto wait_for_step = [&](bool listed, uint32_t level, bool& any) -> int {
        std::vector<char> dev_live(m.devices.size(), 0);
        for (uint32_t r = 0; r < ngpu; ++r)
            if (live[r]) dev_live[m.ranks[r].dev] = 1;
        for (size_t dk = 0; dk < m.devices.size(); ++dk) {
            if (!dev_live[dk]) continue;
            HIP_TRY(hipSetDevice(m.devices[dk]));
            HIP_TRY(hipStreamSynchronize(m.dev_state[dk]->stream.get()));
        }
        any = false;
        for (uint32_t r = 0; r < ngpu; ++r) {
            if (!live[r]) continue;
            float t = 0;
            HIP_TRY(hipSetDevice(m.ranks[r].d->device));
            HIP_TRY(hipEventElapsedTime(&t, ev[2 * r].get(), ev[2 * r + 1].get()));
            ms[r] += t;
            if (listed) {
                n_quads[r] = counts[2 * r];
                refined[r] += uint64_t(counts[2 * r + 1]) * a.pass_spp; // the pixels it lists: what its pass at `level` traces
            }
            live[r] = listed && (n_quads[r] != 0 || level < lv.last[r]);
            any = any || live[r];
        }
        return 0;
    };
    uint32_t k = lv.first;
    bool any = true;
    if (lv.resumed) { // the state comes in: records, conversion, and the list of the lowest level
        for (uint32_t r = 0; r < ngpu; ++r) {
            if (!live[r]) continue;
            DeviceState* d = m.ranks[r].d;
            const hipStream_t stream = d->stream.get();
            HIP_TRY(hipSetDevice(d->device));
            HIP_TRY(hipEventRecord(ev[2 * r].get(), stream));
            HIP_TRY(hipMemcpyAsync(sl.records(m, r), upload[r].data(), upload[r].size() * sizeof(double), hipMemcpyHostToDevice, stream));
            if (int rc = RT_BY_PRECISION(p.precision, adaptive_state_import_launch, sl.records(m, r), m.packed(r), sl.state(m, r), sl.active(m, r),
                                         sl.L.pixels_per_rank, p.spp, a.rel_error, a.abs_error, stream)) return rc;
            if (sel)
                if (int rc = adaptive_region_activate_launch(p.width, p.height, r, ngpu, sel->mask ? (const uint8_t*)d->rg_mask.p : nullptr, sl.select(m, r),
                                                             sl.state(m, r), sl.active(m, r), sel->x0, sel->y0, sel->x1, sel->y1, stream)) return rc;
            if (k < n_passes)
                if (int rc = enqueue_list(r, k, stream)) return rc;
            HIP_TRY(hipEventRecord(ev[2 * r + 1].get(), stream));
        }
        if (int rc = wait_for_step(k < n_passes, k, any)) return rc;
    }
    for (; k < n_passes && any; ++k) {
        const bool more = k + 1 < n_passes; // the cap ends the loop: no list behind the last pass
        pr.sample_begin = p.sample_begin + k * a.pass_spp;
        for (uint32_t r = 0; r < ngpu; ++r) {
            if (!live[r]) continue;
            DeviceState* d = m.ranks[r].d;
            const hipStream_t stream = d->stream.get();
            HIP_TRY(hipSetDevice(d->device));
            pr.tile_rank = r;
            ListPass ad = adaptive_rank_pass(m, sl, r, p, a);
            const bool pass0 = !lv.resumed && k == 0;
            if (!pass0) { ad.quads = sl.quads(m, r); ad.n_quads = n_quads[r]; ad.first = false; }
            HIP_TRY(hipEventRecord(ev[2 * r].get(), stream));
            // (pass 0 fills stats[r] as a plain render of the rank does: kernel form, scene sizes, the samples of its pixels)
            if (pass0 || ad.n_quads != 0)
                if (int rc = render_tiles_any(s, d, cam, &pr, m.packed(r), stream, pass0 && stats ? &stats[r] : nullptr, false, false, &ad)) return rc;
            if (more)
                if (int rc = enqueue_list(r, k + 1, stream)) return rc;
            HIP_TRY(hipEventRecord(ev[2 * r + 1].get(), stream));
        }
        if (int rc = wait_for_step(more, k + 1, any)) return rc; // (no rank goes on: every pixel of every rank is done)
    }
    return 0;
}

// The render behind rttnw_render_adaptive_multi and rttnw_render_adaptive_resume, its arguments checked by them (`p`: tile_world = the number of
// ranks; `single`: rttnw_render_adaptive_resume's ngpu == 0, one rank on the scene's own device).  state_in / state_out (each optional): the
// render starts from, and leaves, a state (include/rttnw_hip.h); without a state_in it is the fresh render, launch for launch.
// `sel` (rttnw_render_adaptive_region): only its pixels are ever active, a missing state_in stands for zero records, the levels are those of the
// selected pixels, and the four outputs are the window's.
static int adaptive_node_render(const char* call, ::rttnw_scene* s, const rttnw_camera_desc* cam, const rttnw_params& p, const rttnw_adaptive* a,
                                uint32_t ngpu, const int32_t* device_ids, bool single, const double* state_in, uint32_t first_level, double* state_out,
                                double* out_linear_rgb, uint8_t* out_rgba8, uint32_t* out_spp, double* out_stderr_rgb, rttnw_stats* stats,
                                const RegionSelection* sel = nullptr) {
    DeviceGuard restore; // (the caller's device is current again after EVERY return below, the error paths included)
    MultiPlan m;
    m.single = single;
    if (int rc = multi_plan(s, p, ngpu, device_ids, m, call)) return rc;
    if (m.env.gather_invalid && !single) { set_last_error(std::string(call) + ": RTTNW_MULTI_GATHER must be rccl or peer"); return RTTNW_ERR_INVALID; }
    AdaptiveSlots sl;
    fill_layout(p.width, p.height, ngpu, sl.L);
    const auto padded = [](size_t bytes) { return (bytes + 255) / 256 * 256; };
    sl.state_chunk = padded(size_t(sl.L.pixels_per_rank) * sizeof(AdaptivePixel));
    sl.active_chunk = padded(sl.L.pixels_per_rank);
    sl.list_chunk = padded((size_t(sl.L.tiles_per_rank) * 16 + quad_scan_words(sl.L.tiles_per_rank * 16u)) * sizeof(uint32_t));
    sl.records_chunk = padded(size_t(sl.L.pixels_per_rank) * STATE_RECORD_DOUBLES * sizeof(double));
    m.aux_chunk = size_t(sl.L.pixels_per_rank) * 4 * sizeof(double);
    // a state_in: its row-major records to every rank's packed order, on the host (pixels outside the image and pad tiles keep zero records)
    LevelPlan lv;
    lv.resumed = state_in != nullptr || sel != nullptr;
    lv.first = first_level;
    lv.last.assign(ngpu, 0);
    const size_t rank_doubles = size_t(sl.L.pixels_per_rank) * STATE_RECORD_DOUBLES;
    RankRecords host_records;
    if (lv.resumed || state_out) state_scatter(state_in, p.width, p.height, sl.L, ngpu, host_records);
    if (state_in && !sel) // the highest level on each rank (the zero records of its padding stand at level 0)
        for (uint32_t r = 0; r < ngpu; ++r)
            for (size_t i = 3; i < rank_doubles; i += STATE_RECORD_DOUBLES) lv.last[r] = std::max(lv.last[r], uint32_t(host_records[r][i]) / a->pass_spp);
    // a selection: the levels its pixels stand at (an unselected pixel is never active), and per rank the blocks that hold a selected pixel
    std::vector<uint32_t> sel_blocks(sel ? ngpu : 0, 0);
    if (sel) {
        lv.first = p.spp / a->pass_spp; // (nothing selected: no level to run)
        for (uint32_t y = sel->y0; y < sel->y1; ++y)
            for (uint32_t x = sel->x0; x < sel->x1; ++x) {
                if (!sel->has(x, y)) continue;
                uint32_t owner;
                const uint32_t level = uint32_t(state_record_at(host_records, x, y, sl.L, owner)[3]) / a->pass_spp;
                lv.first = std::min(lv.first, level);
                lv.last[owner] = std::max(lv.last[owner], level);
                if (sel->opens_block(x, y)) ++sel_blocks[owner];
            }
    }
    // everything that allocates, before the first launch: buffers and workspaces, the ranks' events, their pinned words for the lists' totals
    if (int rc = adaptive_multi_prepare(s, cam, p, *a, m, sl, lv.resumed, lv.resumed || state_out, sel, sel ? &sel_blocks : nullptr)) return rc;
    std::vector<Event> ev(size_t(ngpu) * 2);
    for (uint32_t r = 0; r < ngpu; ++r) {
        HIP_TRY(hipSetDevice(m.ranks[r].d->device));
        HIP_TRY(create_event(ev[2 * r]));
        HIP_TRY(create_event(ev[2 * r + 1]));
    }
    void* pinned = nullptr;
    HIP_TRY(hipHostMalloc(&pinned, size_t(ngpu) * 2 * sizeof(uint32_t), hipHostMallocPortable));
    std::unique_ptr<void, HostFree> counts(pinned);
    std::memset(pinned, 0, size_t(ngpu) * 2 * sizeof(uint32_t));
    if (stats) std::memset(stats, 0, size_t(ngpu) * sizeof(*stats)); // (a rank without a tile runs nothing and keeps zeros)
    if (stats && lv.resumed) // no pass 0 fills them: the scene's sizes and the kernel form, no samples yet
        for (uint32_t r = 0; r < ngpu; ++r) {
            if (!sl.tiles(r, ngpu)) continue;
            rttnw_params pr = p;
            pr.tile_rank = r;
            if (int rc = RT_BY_PRECISION(p.precision, adaptive_rank_stats_t, s, m.ranks[r].d, &pr, &stats[r])) return rc;
        }
    std::vector<double> ms(ngpu, 0.0);
    std::vector<uint64_t> refined(ngpu, 0);
    if (int rc = adaptive_multi_passes(s, cam, p, *a, m, sl, lv, sel, host_records, ev, (uint32_t*)pinned, stats, ms, refined)) return rc;
    // every rank's sums to means and auxiliary records (a rank without a tile: zeros), in its device time like adaptive_output_kernel in the single
    // call's — and, before that, sums and noise state to its state records where the caller wants the state
    for (uint32_t r = 0; r < ngpu; ++r) {
        DeviceState* d = m.ranks[r].d;
        HIP_TRY(hipSetDevice(d->device));
        HIP_TRY(hipEventRecord(ev[2 * r].get(), d->stream.get()));
        if (state_out)
            if (int rc = RT_BY_PRECISION(p.precision, adaptive_state_export_launch, m.packed(r), sl.state(m, r), sl.records(m, r), sl.L.pixels_per_rank,
                                         sl.tiles(r, ngpu) * 64u, d->stream.get())) return rc;
        if (int rc = RT_BY_PRECISION(p.precision, adaptive_finish_launch, m.packed(r), sl.state(m, r), (double*)m.aux(r), sl.L.pixels_per_rank,
                                     sl.tiles(r, ngpu) * 64u, d->stream.get())) return rc;
        HIP_TRY(hipEventRecord(ev[2 * r + 1].get(), d->stream.get()));
    }
    bool use_peer = false, fell_back = false;
    if (int rc = multi_gather(m, use_peer, fell_back)) return rc;
    if (sel) { // the window's outputs in place of the frame's
        DeviceState* root = m.root;
        if (int rc = multi_join_local(m)) return rc;
        if (int rc = RT_BY_PRECISION(p.precision, adaptive_region_window_launch, p.width, p.height, p.tile_world, root->gathered.p, (const double*)root->gathered_aux.p,
                                     root->rg_linear.p, root->rg_rgba.p, (uint32_t*)root->rg_spp.p, (double*)root->rg_stderr.p, sel->x0, sel->y0, sel->x1,
                                     sel->y1, root->stream.get())) return rc;
        if (int rc = multi_finish_streams(m)) return rc;
    } else if (int rc = multi_untile(p, m)) return rc;
    for (uint32_t r = 0; r < ngpu && stats; ++r) {
        float t = 0;
        HIP_TRY(hipSetDevice(m.ranks[r].d->device));
        HIP_TRY(hipEventElapsedTime(&t, ev[2 * r].get(), ev[2 * r + 1].get()));
        stats[r].kernel_ms = ms[r] + t;
        stats[r].samples += refined[r];
    }
    if (stats && use_peer) stats[0].reserved |= 0x100u | (fell_back ? 0x200u : 0u);
    if (state_out) { // every stream has finished (multi_untile): the ranks' records come back and go to their row-major places behind the header
        for (uint32_t r = 0; r < ngpu; ++r) {
            HIP_TRY(hipSetDevice(m.ranks[r].d->device));
            HIP_TRY(hipMemcpy(host_records[r].data(), sl.records(m, r), rank_doubles * sizeof(double), hipMemcpyDeviceToHost));
        }
        state_header(p, *a, cam, state_out);
        state_gather(host_records, p.width, p.height, sl.L, state_out);
    }
    DeviceState* root = m.root;
    HIP_TRY(hipSetDevice(root->device));
    hipError_t e = hipSuccess;
    const size_t out_px = sel ? sel->pixels() : m.npx;
    if (out_spp) e = hipMemcpy(out_spp, (sel ? root->rg_spp : root->ad_spp).p, out_px * sizeof(uint32_t), hipMemcpyDeviceToHost);
    if (e == hipSuccess && out_stderr_rgb) e = hipMemcpy(out_stderr_rgb, (sel ? root->rg_stderr : root->ad_stderr).p, out_px * 3 * sizeof(double), hipMemcpyDeviceToHost);
    return copy_image_out(call, sel ? root->rg_rgba : root->rgba, sel ? root->rg_linear : root->linear, p.precision, out_px, out_rgba8, out_linear_rgb, e);
}
// What the three entry points over ranks make of their arguments: the refusals in the header's order — none of them needs a device — and the render.
// `allow_zero`: ngpu == 0 stands for the scene's own device (resume, region); `sel`: the region form, whose state may hold empty records.
static int adaptive_ranks_entry(const char* call, bool allow_zero, const RegionSelection* sel, ::rttnw_scene* s, const rttnw_camera_desc* cam,
                                const rttnw_params* p_in, const rttnw_adaptive* a, uint32_t ngpu, const int32_t* device_ids, const double* state_in,
                                double* state_out, double* out_linear_rgb, uint8_t* out_rgba8, uint32_t* out_spp, double* out_stderr_rgb, rttnw_stats* stats) {
    if (!p_in || !a) { set_last_error(std::string(call) + ": NULL argument (p or a)"); return RTTNW_ERR_INVALID; }
    if (sel && (sel->x0 >= sel->x1 || sel->y0 >= sel->y1 || sel->x1 > p_in->width || sel->y1 > p_in->height)) {
        set_last_error(std::string(call) + ": the window [x0, x1) x [y0, y1) must be non-empty and lie inside the width x height frame");
        return RTTNW_ERR_INVALID;
    }
    if (int rc = refuse_ranks_misuse(call, allow_zero, ngpu, device_ids)) return rc;
    if (int rc = refuse_adaptive_misuse(call, p_in, a)) return rc;
    rttnw_params p = *p_in;
    if (ngpu) { p.tile_rank = 0; p.tile_world = 1; } // (ngpu >= 1: the caller's are ignored, so the tile_world rule of the single call has nothing to refuse; ngpu == 0: tile_world must be 1)
    if (int rc = refuse_host_output_misuse(call, a->reserved0, &p)) return rc;
    uint32_t first_level = 0; // (the region form does not use it: its levels are the selected pixels', adaptive_node_render)
    std::string err;
    if (state_in)
        if (int rc = refuse_state_misuse(call, sel != nullptr, *p_in, *a, cam, state_in, first_level, err)) { set_last_error(err); return rc; }
    p.tile_rank = 0; p.tile_world = std::max(ngpu, 1u);
    if (int rc = validate(s, cam, &p)) return rc;
    if (int rc = refuse_unknown_devices(call, ngpu, device_ids)) return rc;
    const int32_t own = s->device->device; // ngpu == 0: one rank where rttnw_render_adaptive runs
    return adaptive_node_render(call, s, cam, p, a, std::max(ngpu, 1u), ngpu ? device_ids : &own, ngpu == 0, state_in, first_level, state_out, out_linear_rgb,
                                out_rgba8, out_spp, out_stderr_rgb, stats, sel);
}
} // namespace rt

extern "C" int rttnw_render_adaptive_multi(rttnw_scene* s, const rttnw_camera_desc* cam, const rttnw_params* p, const rttnw_adaptive* a, uint32_t ngpu,
                                           const int32_t* device_ids, double* out_linear_rgb, uint8_t* out_rgba8, uint32_t* out_spp, double* out_stderr_rgb,
                                           rttnw_stats* stats) {
    return rt::adaptive_ranks_entry("render_adaptive_multi", false, nullptr, s, cam, p, a, ngpu, device_ids, nullptr, nullptr, out_linear_rgb, out_rgba8, out_spp,
                                    out_stderr_rgb, stats);
}

extern "C" uint64_t rttnw_adaptive_state_doubles(uint32_t width, uint32_t height) { return rt::state_doubles(width, height); }

// rttnw_render_adaptive_resume (include/rttnw_hip.h has the contract and the state's layout, DESIGN.md §10a "resumable form" the why)
extern "C" int rttnw_render_adaptive_resume(rttnw_scene* s, const rttnw_camera_desc* cam, const rttnw_params* p, const rttnw_adaptive* a, uint32_t ngpu,
                                            const int32_t* device_ids, const double* state_in, double* state_out, double* out_linear_rgb,
                                            uint8_t* out_rgba8, uint32_t* out_spp, double* out_stderr_rgb, rttnw_stats* stats) {
    return rt::adaptive_ranks_entry("render_adaptive_resume", true, nullptr, s, cam, p, a, ngpu, device_ids, state_in, state_out, out_linear_rgb, out_rgba8,
                                    out_spp, out_stderr_rgb, stats);
}

// rttnw_render_adaptive_region (include/rttnw_hip.h has the contract, DESIGN.md §10a "windowed form" the why): the resumed render over a selection
extern "C" int rttnw_render_adaptive_region(rttnw_scene* s, const rttnw_camera_desc* cam, const rttnw_params* p, const rttnw_adaptive* a, uint32_t x0,
                                            uint32_t y0, uint32_t x1, uint32_t y1, const uint8_t* mask, uint32_t ngpu, const int32_t* device_ids,
                                            const double* state_in, double* state_out, double* out_linear_rgb, uint8_t* out_rgba8, uint32_t* out_spp,
                                            double* out_stderr_rgb, rttnw_stats* stats) {
    const rt::RegionSelection sel{x0, y0, x1, y1, mask};
    return rt::adaptive_ranks_entry("render_adaptive_region", true, &sel, s, cam, p, a, ngpu, device_ids, state_in, state_out, out_linear_rgb, out_rgba8, out_spp,
                                    out_stderr_rgb, stats);
}

// ---------------------------------------------------------------------------------------------
// The adaptive forms that run ONE rank on the scene's device, on the default stream: rttnw_render_adaptive_denoised, rttnw_render_preview,
// rttnw_render_adaptive_budget and rttnw_render_adaptive_budget_denoised.  RankRounds owns what they share — the rank's sums and noise state in the scene's workspaces, the list pass, the raw
// values, the state going in and out — as steps that each form calls in its own order; what differs between the forms (who is alive, what a round
// runs besides its trace, the clocks, the outputs) stays in the form.
// ---------------------------------------------------------------------------------------------
namespace rt {
struct RankRounds {
    DeviceGuard restore; // (the caller's device is current again after EVERY return of the form, the error paths included)
    ::rttnw_scene* const s; const rttnw_camera_desc* const cam; const rttnw_params& p; const rttnw_adaptive& a; // the call's arguments
    DeviceState* const d;
    rttnw_tile_layout L;
    size_t npx, ppr, rsz;         // pixels of the frame, of the rank's packed order; bytes of a real
    uint32_t n_blocks, B;         // 2x2 blocks of the rank's tiles; samples of a pass
    const hipStream_t stream = nullptr;
    rttnw_params pass;            // p with spp = B: what a list pass traces
    ListPass ad;
    DevBuf<uint8_t> means;        // raw(): a copy of the sums, divided
    DevBuf<double> aux, records;  // raw(): the auxiliary records; the packed state records, going in or out
    RankRecords host_records;     // ... and their host copy
    bool resumed = false;
    Event ev0, ev1;               // the form's clock: recorded by the form
    uint64_t samples = 0;         // traced so far (list() counts; a form that does not read the totals adds its own)

    RankRounds(::rttnw_scene* s, const rttnw_camera_desc* cam, const rttnw_params& p, const rttnw_adaptive& a) : s(s), cam(cam), p(p), a(a), d(s->device), pass(p) {
        fill_layout(p.width, p.height, 1, L);
        npx = size_t(p.width) * p.height, ppr = L.pixels_per_rank, rsz = p.precision == RTTNW_F32 ? sizeof(float) : sizeof(double);
        n_blocks = L.n_tiles * 16u, B = a.pass_spp;
        pass.spp = B;
    }
    // Everything of the shared part that allocates, before the first launch: the adaptive passes' buffers, the driver's own, what a list pass over
    // `n_quads` blocks needs, and the scene's sizes in `stats`.  `active`: the bytes the pass's resolve step writes (d->ad_active, or the form's own).
    // `state_in` (optional): its records go to packed order here, on the host; `state_out`: the form will export_state().
    int open(DevBuf<uint8_t>& active, uint32_t n_quads, const double* state_in, bool state_out, rttnw_stats* stats) {
        HIP_TRY(hipSetDevice(d->device));
        HIP_TRY(d->packed.grow(ppr * 4 * rsz));
        HIP_TRY(d->ad_state.grow(ppr * sizeof(AdaptivePixel)));
        HIP_TRY(active.grow(ppr));
        HIP_TRY(d->list_quads.grow(size_t(n_blocks) * sizeof(uint32_t)));
        HIP_TRY(d->list_scan.grow(quad_scan_words(n_blocks) * sizeof(uint32_t)));
        HIP_TRY(means.alloc(ppr * 4 * rsz));
        HIP_TRY(aux.alloc(ppr * 4));
        resumed = state_in != nullptr;
        if (resumed || state_out) HIP_TRY(records.alloc(ppr * STATE_RECORD_DOUBLES));
        if (resumed) state_scatter(state_in, p.width, p.height, L, 1, host_records);
        HIP_TRY(create_event(ev0)); HIP_TRY(create_event(ev1));
        ad.state = (AdaptivePixel*)d->ad_state.p; ad.active = active.p;
        ad.quads = (const uint32_t*)d->list_quads.p; ad.n_quads = n_quads;
        ad.first = false; // (level 0 too is a list pass on zero sums: 0 + c0 is the chain's first addition, as in the windowed form)
        if (int rc = render_tiles_any(s, d, cam, &pass, d->packed.p, stream, nullptr, false, true, &ad)) return rc;
        return stats ? RT_BY_PRECISION(p.precision, adaptive_rank_stats_t, s, d, &p, stats) : 0;
    }
    // Before round 0: zero sums and zero noise state everywhere, or the state that came in (`import_active`: where the import leaves its active
    // bytes, under the caller's rule)
    int start(uint8_t* import_active) {
        if (resumed) {
            HIP_TRY(hipMemcpyAsync(records.p, host_records[0].data(), host_records[0].size() * sizeof(double), hipMemcpyHostToDevice, stream));
            return RT_BY_PRECISION(p.precision, adaptive_state_import_launch, records.p, d->packed.p, d->ad_state.p, import_active, L.pixels_per_rank, p.spp,
                                   a.rel_error, a.abs_error, stream);
        }
        HIP_TRY(hipMemsetAsync(d->packed.p, 0, ppr * 4 * rsz, stream));
        HIP_TRY(hipMemsetAsync(d->ad_state.p, 0, ppr * sizeof(AdaptivePixel), stream));
        return 0;
    }
    // The list of the 2x2 blocks that hold a marked pixel ...
    int enqueue_list(const uint8_t* marks) {
        return enqueue_quad_list(marks, n_blocks, (uint32_t*)d->list_scan.p, (uint32_t*)d->list_quads.p, stream);
    }
    // ... and, in one 8-byte copy the host waits for, its totals: listed blocks, marked pixels — the pixels the pass over it traces
    int list(const uint8_t* marks, uint32_t count[2]) {
        if (int rc = enqueue_list(marks)) return rc;
        HIP_TRY(hipMemcpy(count, quad_list_totals((uint32_t*)d->list_scan.p, n_blocks), 2 * sizeof(uint32_t), hipMemcpyDeviceToHost));
        samples += uint64_t(count[1]) * B;
        return 0;
    }
    // The list pass over the first n_quads blocks of the list, all of whose marked pixels stand at `level` (hold level * B samples)
    int trace(uint32_t level, uint32_t n_quads, uint32_t cap, double rel_error, double abs_error) {
        pass.sample_begin = p.sample_begin + level * B;
        ad.n_quads = n_quads; ad.cap = cap; ad.rel_error = rel_error; ad.abs_error = abs_error;
        return render_tiles_any(s, d, cam, &pass, d->packed.p, stream, nullptr, false, false, &ad);
    }
    // The raw values of every pixel of the frame, by the adaptive render's own division on a COPY of the sums (the sums themselves stay for the next
    // round): `means` and `aux`
    int raw() {
        HIP_TRY(hipMemcpyAsync(means.p, d->packed.p, ppr * 4 * rsz, hipMemcpyDeviceToDevice, stream));
        return RT_BY_PRECISION(p.precision, adaptive_finish_launch, means.p, d->ad_state.p, aux.p, L.pixels_per_rank, L.n_tiles * 64u, stream);
    }
    // Sums and noise state to the packed state records, on the stream; and, once the host has waited for it, the records to their row-major places
    // behind the header
    int export_state() {
        return RT_BY_PRECISION(p.precision, adaptive_state_export_launch, d->packed.p, d->ad_state.p, records.p, L.pixels_per_rank, L.n_tiles * 64u, stream);
    }
    int state_out(double* out) {
        if (!resumed) state_scatter(nullptr, p.width, p.height, L, 1, host_records); // (the host copy is made where it is first needed)
        HIP_TRY(hipMemcpy(host_records[0].data(), records.p, host_records[0].size() * sizeof(double), hipMemcpyDeviceToHost));
        state_header(p, a, cam, out);
        state_gather(host_records, p.width, p.height, L, out);
        return RTTNW_OK;
    }
};

// The filter half of the forms that filter (denoised, preview, budget_denoised), beside a RankRounds: the workspace of the à-trous passes, the
// feature pass that guides them, the raw maps they read, the passes themselves and the copies of what they leave to the host.  Row-major buffers
// of the frame on the scene's device; when a form runs each step — per round, or once behind its rounds — stays in the form.
struct FilterStage {
    RankRounds& r;
    const size_t npx;
    const bool flags, with_variance; // a pixel may hold no value yet (rttnw_reconstruct's passes); a variance goes through the filter
    DevBuf<double> maps, mean, variance, raw_stderr, stderr_f, d_c[2], d_v[2]; // stderr_f: the form's own step behind the filter writes it
    DevBuf<uint32_t> spp;
    DevBuf<uint8_t> rgba, valid, valid_out, holds[2];
    float feature_ms = 0;
    int out = 0; // filter(): the image is left in d_c[out], its variance in d_v[out]

    FilterStage(RankRounds& r, bool flags, bool with_variance) : r(r), npx(r.npx), flags(flags), with_variance(with_variance) {}
    // Everything of the stage that allocates, before the first launch: a form without flags or without a variance has no buffers for them
    int open() {
        HIP_TRY(maps.alloc(npx * 8)); HIP_TRY(mean.alloc(npx * 3)); HIP_TRY(variance.alloc(npx * 3)); HIP_TRY(raw_stderr.alloc(npx * 3));
        HIP_TRY(spp.alloc(npx)); HIP_TRY(rgba.alloc(npx * 4));
        if (with_variance) HIP_TRY(stderr_f.alloc(npx * 3));
        if (flags) { HIP_TRY(valid.alloc(npx)); HIP_TRY(valid_out.alloc(npx)); }
        for (int k = 0; k < 2; ++k) {
            HIP_TRY(d_c[k].alloc(npx * 3));
            if (with_variance) HIP_TRY(d_v[k].alloc(npx * 3));
            if (flags) HIP_TRY(holds[k].alloc(npx));
        }
        return 0;
    }
    // The feature maps, which stay on the device (the pass times itself between d->ev0 and d->ev1 and waits for the stream)
    int features(uint32_t feature_spp) {
        rttnw_params pf = r.p;
        pf.spp = feature_spp ? feature_spp : r.B;
        if (int rc = RT_BY_PRECISION(r.p.precision, render_features_device_t, r.s, r.cam, &pf, maps.p, r.stream)) return rc;
        HIP_TRY(hipEventElapsedTime(&feature_ms, r.d->ev0.get(), r.d->ev1.get()));
        return 0;
    }
    const double* albedo() const { return maps.p; }
    const double* normal() const { return maps.p + npx * 3; }
    const double* depth() const { return maps.p + npx * 6; }
    const double* alpha() const { return maps.p + npx * 7; }
    // The raw maps of every pixel of the frame (with flags: and the valid byte of those that hold samples)
    int raw() {
        if (int rc = r.raw()) return rc;
        return guided_raw_launch(r.p.precision, r.means.p, r.aux.p, mean.p, variance.p, raw_stderr.p, spp.p, flags ? valid.p : nullptr, r.p.width, r.p.height,
                                 r.stream);
    }
    // The passes over the raw maps
    int filter(const rttnw_denoise_params& dn) {
        const DenoiseParams prm = denoise_params(dn.sigma_luminance, dn.sigma_normal, dn.sigma_depth, with_variance);
        double* const c[2] = {d_c[0].p, d_c[1].p};
        double* const v[2] = {d_v[0].p, d_v[1].p};
        uint8_t* const h[2] = {holds[0].p, holds[1].p};
        return atrous_passes_device(r.p.width, r.p.height, mean.p, with_variance ? variance.p : nullptr, flags ? valid.p : nullptr, albedo(), normal(), depth(),
                                    alpha(), dn.iterations, prm, c, v, h, rgba.p, valid_out.p, r.stream, out);
    }
    const double* filtered() const { return d_c[out].p; }
    const double* filtered_variance() const { return d_v[out].p; }
    // What the last filter() and raw() left, to the host arrays the caller gave (the device is idle: the form has waited)
    int copy_out(double* out_linear_rgb, uint8_t* out_rgba8, uint8_t* out_valid, uint32_t* out_spp, double* out_stderr_rgb, double* out_raw_linear_rgb,
                 double* out_raw_stderr_rgb) {
        const size_t rgb_bytes = npx * 3 * sizeof(double);
        if (out_linear_rgb) HIP_TRY(hipMemcpy(out_linear_rgb, filtered(), rgb_bytes, hipMemcpyDeviceToHost));
        if (out_rgba8) HIP_TRY(hipMemcpy(out_rgba8, rgba.p, npx * 4, hipMemcpyDeviceToHost));
        if (out_valid) HIP_TRY(hipMemcpy(out_valid, valid_out.p, npx, hipMemcpyDeviceToHost));
        if (out_spp) HIP_TRY(hipMemcpy(out_spp, spp.p, npx * sizeof(uint32_t), hipMemcpyDeviceToHost));
        if (out_stderr_rgb) HIP_TRY(hipMemcpy(out_stderr_rgb, stderr_f.p, rgb_bytes, hipMemcpyDeviceToHost));
        if (out_raw_linear_rgb) HIP_TRY(hipMemcpy(out_raw_linear_rgb, mean.p, rgb_bytes, hipMemcpyDeviceToHost));
        if (out_raw_stderr_rgb) HIP_TRY(hipMemcpy(out_raw_stderr_rgb, raw_stderr.p, rgb_bytes, hipMemcpyDeviceToHost));
        return 0;
    }
};

// rttnw_render_adaptive_denoised (include/rttnw_hip.h has the contract, DESIGN.md §10a "filter-guided form" the why): adaptive rounds whose stopping
// rule reads the FILTERED image.  A round is one level of the windowed form's loop — the list of the 2x2 blocks that hold an alive pixel, the list pass
// over it with the windowed form's arguments (a cap of (k+1)B and zero tolerances), the raw values — and then the denoiser's passes and the stop kernel
// (guided.hpp), all on buffers that never leave the device: per round the host reads the list's two totals, which are also the count of alive pixels.
static int adaptive_denoised_render(::rttnw_scene* s, const rttnw_camera_desc* cam, const rttnw_params& p, const rttnw_adaptive& a, const rttnw_guided& g,
                                    double* out_linear_rgb, uint8_t* out_rgba8, uint32_t* out_spp, double* out_stderr_rgb, double* out_raw_linear_rgb,
                                    double* out_raw_stderr_rgb, double* state_out, rttnw_stats* stats) {
    RankRounds r(s, cam, p, a);
    FilterStage f(r, false, true);
    DeviceState* d = r.d;
    const hipStream_t stream = r.stream;
    // everything that allocates, before the first launch (d->ad_active: the resolve step's active bytes under the pass's own cap — not read here, the
    // alive bytes decide)
    if (int rc = r.open(d->ad_active, r.n_blocks, nullptr, state_out != nullptr, stats)) return rc;
    if (int rc = f.open()) return rc;
    DevBuf<uint8_t> alive;
    HIP_TRY(alive.alloc(r.ppr));

    // before round 0: the feature maps, and every pixel of the image alive on zero sums and zero noise state
    if (int rc = f.features(g.feature_spp)) return rc;
    HIP_TRY(hipEventRecord(r.ev0.get(), stream));
    if (int rc = r.start(nullptr)) return rc;
    if (int rc = guided_lattice_launch(alive.p, r.L.pixels_per_rank, p.width, p.height, 0u, stream)) return rc;
    for (uint32_t k = 0; k < p.spp / r.B; ++k) {
        // the list of this round: the alive bytes are its active AND its selection bytes
        uint32_t count[2] = {0, 0}; // listed blocks, alive pixels
        if (int rc = r.list(alive.p, count)) return rc;
        if (count[0] == 0) break; // every pixel has stopped
        // 1. trace: the alive pixels, all of which hold exactly kB samples — one level
        if (int rc = r.trace(k, count[0], (k + 1u) * r.B, 0.0, 0.0)) return rc;
        // 2. raw values of every pixel of the frame, 3. filter
        if (int rc = f.raw()) return rc;
        if (int rc = f.filter(g.denoise)) return rc;
        // 4. stop
        if (int rc = guided_stop_launch(f.filtered(), f.filtered_variance(), f.raw_stderr.p, a.rel_error, a.abs_error, alive.p, f.stderr_f.p, p.width, p.height,
                                        stream)) return rc;
    }
    if (state_out)
        if (int rc = r.export_state()) return rc;
    HIP_TRY(hipEventRecord(r.ev1.get(), stream));
    HIP_TRY(hipDeviceSynchronize());
    if (stats) {
        float ms = 0;
        HIP_TRY(hipEventElapsedTime(&ms, r.ev0.get(), r.ev1.get()));
        stats->kernel_ms = double(f.feature_ms) + double(ms);
        stats->samples = r.samples;
    }
    // the outputs of the last round that ran
    if (int rc = f.copy_out(out_linear_rgb, out_rgba8, nullptr, out_spp, out_stderr_rgb, out_raw_linear_rgb, out_raw_stderr_rgb)) return rc;
    return state_out ? r.state_out(state_out) : RTTNW_OK;
}
} // namespace rt

extern "C" int rttnw_render_adaptive_denoised(rttnw_scene* s, const rttnw_camera_desc* cam, const rttnw_params* p, const rttnw_adaptive* a, const rttnw_guided* g,
                                              double* out_linear_rgb, uint8_t* out_rgba8, uint32_t* out_spp, double* out_stderr_rgb,
                                              double* out_raw_linear_rgb, double* out_raw_stderr_rgb, double* state_out, rttnw_stats* stats) {
    using namespace rt;
    // the refusals, in the header's order: none of them needs a device
    if (!p || !a || !g) { set_last_error("render_adaptive_denoised: NULL argument (p, a or g)"); return RTTNW_ERR_INVALID; }
    if (int rc = refuse_adaptive_misuse("render_adaptive_denoised", p, a)) return rc;
    if (int rc = refuse_host_output_misuse("render_adaptive_denoised", a->reserved0, p)) return rc;
    if (g->reserved0 != 0) { set_last_error("render_adaptive_denoised: g->reserved0 must be 0"); return RTTNW_ERR_INVALID; }
    if (int rc = denoise_refuse_params("render_adaptive_denoised", "g->denoise.", g->denoise)) return rc;
    if (int rc = validate(s, cam, p)) return rc;
    return adaptive_denoised_render(s, cam, *p, *a, *g, out_linear_rgb, out_rgba8, out_spp, out_stderr_rgb, out_raw_linear_rgb, out_raw_stderr_rgb, state_out,
                                    stats);
}

// ---------------------------------------------------------------------------------------------
// rttnw_render_preview (include/rttnw_hip.h has the contract, DESIGN.md §10b "a frame from a fraction of its pixels" the why): the adaptive rounds of
// the windowed form over a LATTICE of the frame, then the feature pass and rttnw_reconstruct's passes, all on buffers that never leave the device.
// One rank on the scene's device, default stream.  The rounds are adaptive_denoised_render's, with two differences: the bytes that start alive are the
// lattice's (guided_lattice_launch at the caller's level), and a round's list pass runs under the caller's cap and tolerances, so the resolve step's own stopping rule
// writes the next round's bytes — the alive bytes ARE the pass's active bytes.  Every alive pixel holds exactly kB samples in round k, which is one
// level of the windowed form's loop: list for list what rttnw_render_adaptive_region traces under mask = the lattice.
// ---------------------------------------------------------------------------------------------
namespace rt {
static int preview_render(::rttnw_scene* s, const rttnw_camera_desc* cam, const rttnw_params& p, const rttnw_adaptive& a, const rttnw_preview& pv,
                          double* out_linear_rgb, uint8_t* out_rgba8, uint8_t* out_valid, uint32_t* out_spp, double* out_raw_linear_rgb,
                          double* out_raw_stderr_rgb, double* state_out, rttnw_stats* stats) {
    RankRounds r(s, cam, p, a);
    FilterStage f(r, true, false); // no variance goes into the filter
    DeviceState* d = r.d;
    const hipStream_t stream = r.stream;
    // the blocks that hold a lattice pixel: every block at level 0 and 1, one in 4^(level-1) above
    const uint32_t step = 1u << pv.level, block_step = std::max(step, 2u);
    const uint32_t lattice_blocks = ((p.width + block_step - 1) / block_step) * ((p.height + block_step - 1) / block_step);
    // everything that allocates, before the first launch: the shared part with what a list pass over the lattice's blocks needs, and this call's own
    if (int rc = r.open(d->ad_active, std::min(lattice_blocks, r.n_blocks), nullptr, state_out != nullptr, stats)) return rc;
    if (int rc = f.open()) return rc;
    Event ev2, ev3; // the reconstruction's clock
    HIP_TRY(create_event(ev2)); HIP_TRY(create_event(ev3));

    // before round 0: zero sums and zero noise state everywhere, and the lattice alive
    HIP_TRY(hipEventRecord(r.ev0.get(), stream));
    if (int rc = r.start(nullptr)) return rc;
    if (int rc = guided_lattice_launch(d->ad_active.p, r.L.pixels_per_rank, p.width, p.height, pv.level, stream)) return rc;
    for (uint32_t k = 0; k < p.spp / r.B; ++k) {
        uint32_t count[2] = {0, 0}; // listed blocks, alive pixels
        if (int rc = r.list(d->ad_active.p, count)) return rc;
        if (count[0] == 0) break; // every lattice pixel has stopped
        // trace the alive pixels, all of which hold exactly kB samples; the resolve step decides, under the caller's rule, who is alive in round k + 1
        if (int rc = r.trace(k, count[0], p.spp, a.rel_error, a.abs_error)) return rc;
    }
    // the raw values of every pixel of the frame; a pixel holds a value where it holds samples
    if (state_out)
        if (int rc = r.export_state()) return rc;
    if (int rc = f.raw()) return rc;
    HIP_TRY(hipEventRecord(r.ev1.get(), stream));
    // the features, and the reconstruction on its own clock
    if (int rc = f.features(pv.feature_spp)) return rc;
    HIP_TRY(hipEventRecord(ev2.get(), stream));
    if (int rc = f.filter(pv.denoise)) return rc;
    HIP_TRY(hipEventRecord(ev3.get(), stream));
    HIP_TRY(hipDeviceSynchronize());
    if (stats) {
        float ms = 0, ms_r = 0;
        HIP_TRY(hipEventElapsedTime(&ms, r.ev0.get(), r.ev1.get()));
        HIP_TRY(hipEventElapsedTime(&ms_r, ev2.get(), ev3.get()));
        stats->kernel_ms = double(ms) + double(f.feature_ms) + double(ms_r);
        stats->samples = r.samples;
    }
    if (int rc = f.copy_out(out_linear_rgb, out_rgba8, out_valid, out_spp, nullptr, out_raw_linear_rgb, out_raw_stderr_rgb)) return rc;
    return state_out ? r.state_out(state_out) : RTTNW_OK;
}
} // namespace rt

extern "C" int rttnw_render_preview(rttnw_scene* s, const rttnw_camera_desc* cam, const rttnw_params* p, const rttnw_adaptive* a, const rttnw_preview* v,
                                    double* out_linear_rgb, uint8_t* out_rgba8, uint8_t* out_valid, uint32_t* out_spp, double* out_raw_linear_rgb,
                                    double* out_raw_stderr_rgb, double* state_out, rttnw_stats* stats) {
    using namespace rt;
    // the refusals, in the header's order: none of them needs a device
    if (!p || !a || !v) { set_last_error("render_preview: NULL argument (p, a or v)"); return RTTNW_ERR_INVALID; }
    if (int rc = refuse_adaptive_misuse("render_preview", p, a)) return rc;
    if (int rc = refuse_host_output_misuse("render_preview", a->reserved0, p)) return rc;
    if (v->level > 6) { set_last_error("render_preview: v->level must be 0 .. 6"); return RTTNW_ERR_INVALID; }
    if (int rc = denoise_refuse_params("render_preview", "v->denoise.", v->denoise)) return rc;
    if (int rc = validate(s, cam, p)) return rc;
    return preview_render(s, cam, *p, *a, *v, out_linear_rgb, out_rgba8, out_valid, out_spp, out_raw_linear_rgb, out_raw_stderr_rgb, state_out, stats);
}

// ---------------------------------------------------------------------------------------------
// rttnw_budget_select and rttnw_render_adaptive_budget (include/rttnw_hip.h has the contracts, DESIGN.md §10a "budgeted form" the why): adaptive rounds
// under a budget of samples.  One rank on the scene's device, default stream.  A round: the running sums COPIED and turned into means and auxiliary
// records by adaptive_finish_launch (as in adaptive_denoised_render), the selection of the worst pixels the budget still pays for (budget.hpp) — which
// leaves their bytes on the device and a small record for the host: how many, and per level the blocks that hold one — and then, per occupied level
// in ascending order, the windowed form's list pass: adaptive_level_select_launch over the selection bytes, the list, render_tiles_t under a cap of
// (k+1)B and zero tolerances.  The selection bytes are that pass's ACTIVE bytes: its resolve step clears the byte of every pixel it traced (n == its
// cap), so a pixel that moved from level k to k + 1 is not listed a second time in the same round.
// ---------------------------------------------------------------------------------------------
extern "C" int rttnw_budget_select(uint32_t width, uint32_t height, const double* linear_rgb, const double* stderr_rgb, const uint32_t* spp, uint32_t cap,
                                   double rel_error, double abs_error, uint64_t max_pixels, uint8_t* out_mask, double* out_priority,
                                   uint64_t* out_selected, double* kernel_ms) {
    using namespace rt;
    if (!linear_rgb) { set_last_error("budget_select: linear_rgb is NULL"); return RTTNW_ERR_INVALID; }
    if (!stderr_rgb) { set_last_error("budget_select: stderr_rgb is NULL"); return RTTNW_ERR_INVALID; }
    if (!spp) { set_last_error("budget_select: spp is NULL"); return RTTNW_ERR_INVALID; }
    if (!width || !height) { set_last_error("budget_select: width * height is 0"); return RTTNW_ERR_INVALID; }
    if (cap == 0) { set_last_error("budget_select: cap is 0"); return RTTNW_ERR_INVALID; }
    if (!(rel_error >= 0.0) || !(abs_error >= 0.0)) { set_last_error("budget_select: rel_error and abs_error must be >= 0 (and not NaN)"); return RTTNW_ERR_INVALID; }
    if (rel_error == 0.0 && abs_error == 0.0) {
        set_last_error("budget_select: rel_error and abs_error are both 0 (a priority relative to a tolerance of nothing ranks every noisy pixel +inf)");
        return RTTNW_ERR_INVALID;
    }
    // (the key holds the row-major index in 32 bits)
    if (uint64_t(width) * height > 0xFFFFFFFFull) { set_last_error("budget_select: width * height is limited to 2^32 - 1 pixels"); return RTTNW_ERR_UNSUPPORTED; }
    return budget_select_device(width, height, linear_rgb, stderr_rgb, spp, cap, rel_error, abs_error, max_pixels, out_mask, out_priority, out_selected,
                                kernel_ms);
}

namespace rt {
// What a round of either budgeted form traces once its census is on the host (census[0] pixels selected, census[1 + k] blocks listed at level k):
// per occupied level, ascending, the level's marks out of the selection bytes, the list, and the pass over it.  Counts the round's samples.
static int budget_round_trace(RankRounds& r, const std::vector<uint32_t>& census, uint8_t* select, uint8_t* marks) {
    const uint32_t B = r.B, n_levels = r.p.spp / B;
    r.samples += uint64_t(census[0]) * B;
    for (uint32_t k = 0; k < n_levels; ++k) { // (a level's list length comes with the census: the list's own totals are not read)
        if (census[1u + k] == 0) continue;
        if (int rc = adaptive_level_select_launch(select, r.d->ad_state.p, marks, r.n_blocks * 4u, k * B, r.stream)) return rc;
        if (int rc = r.enqueue_list(marks)) return rc;
        if (int rc = r.trace(k, census[1u + k], (k + 1u) * B, 0.0, 0.0)) return rc;
    }
    return 0;
}

static int adaptive_budget_render(::rttnw_scene* s, const rttnw_camera_desc* cam, const rttnw_params& p, const rttnw_adaptive& a, const rttnw_budget& bg,
                                  const double* state_in, double* state_out, double* out_linear_rgb, uint8_t* out_rgba8, uint32_t* out_spp,
                                  double* out_stderr_rgb, rttnw_stats* stats) {
    RankRounds r(s, cam, p, a);
    DeviceState* d = r.d;
    const size_t npx = r.npx;
    const uint32_t B = r.B, n_levels = p.spp / B;
    const uint64_t round_pixels = bg.round_pixels ? bg.round_pixels : (uint64_t(npx) + 1u) / 2u; // (half the frame: DESIGN.md §10a has the measurement)
    const hipStream_t stream = r.stream;
    // everything that allocates, before the first launch: the shared part with what a list pass over every block needs (the selection bytes are that
    // pass's active bytes), and this call's own
    DevBuf<uint8_t> select, marks;
    DevBuf<uint32_t> record;
    BudgetWorkspace work;
    if (int rc = r.open(select, r.n_blocks, state_in, state_out != nullptr, stats)) return rc;
    HIP_TRY(d->rg_linear.grow(npx * 3 * r.rsz)); HIP_TRY(d->rg_rgba.grow(npx * 4));
    HIP_TRY(d->rg_spp.grow(npx * sizeof(uint32_t))); HIP_TRY(d->rg_stderr.grow(npx * 3 * sizeof(double)));
    HIP_TRY(marks.alloc(r.ppr)); HIP_TRY(record.alloc(1u + size_t(n_levels))); HIP_TRY(work.alloc(npx));

    // before round 0: the state comes in (or zero sums and zero noise state), and nothing is selected
    // (the import's active bytes, under the caller's rule, go to `marks` and are not read: the selection decides who is traced)
    HIP_TRY(hipEventRecord(r.ev0.get(), stream));
    if (int rc = r.start(marks.p)) return rc;
    HIP_TRY(hipMemsetAsync(select.p, 0, r.ppr, stream)); // (the rest of an edge tile is never selected: a round writes the bytes of the image's pixels only)
    uint64_t remaining = bg.samples, rounds = 0;
    std::vector<uint32_t> census(1u + size_t(n_levels));
    for (;;) {
        // the values every pixel is ranked by — and the call's outputs, if this round selects nothing
        if (int rc = r.raw()) return rc;
        const uint64_t max_pixels = std::min<uint64_t>(round_pixels, remaining / B);
        if (max_pixels == 0) break; // the budget pays for no further pass
        // the selection, and in one copy its record: the pixels selected and, per level, the length of the list over them
        if (int rc = budget_round_launch(work, p.precision, r.means.p, r.aux.p, d->ad_state.p, p.width, p.height, p.spp, B, a.rel_error, a.abs_error, max_pixels,
                                         select.p, record.p, stream)) return rc;
        HIP_TRY(hipMemcpy(census.data(), record.p, census.size() * sizeof(uint32_t), hipMemcpyDeviceToHost));
        if (census[0] == 0) break; // no candidate is left
        ++rounds;
        remaining -= uint64_t(census[0]) * B;
        if (int rc = budget_round_trace(r, census, select.p, marks.p)) return rc;
    }
    // the state the call ends in, and the whole frame as the windowed form reports a window (`means` and `aux` are those of that state)
    if (state_out)
        if (int rc = r.export_state()) return rc;
    if (int rc = RT_BY_PRECISION(p.precision, adaptive_region_window_launch, p.width, p.height, 1u, r.means.p, r.aux.p, d->rg_linear.p, d->rg_rgba.p,
                                 (uint32_t*)d->rg_spp.p, (double*)d->rg_stderr.p, 0u, 0u, p.width, p.height, stream)) return rc;
    HIP_TRY(hipEventRecord(r.ev1.get(), stream));
    HIP_TRY(hipDeviceSynchronize());
    if (stats) {
        float ms = 0;
        HIP_TRY(hipEventElapsedTime(&ms, r.ev0.get(), r.ev1.get()));
        stats->kernel_ms = ms;
        stats->samples = r.samples;
        stats->reserved |= uint32_t(std::min<uint64_t>(rounds, 0xFFFFu)) << 16;
    }
    if (out_spp) HIP_TRY(hipMemcpy(out_spp, d->rg_spp.p, npx * sizeof(uint32_t), hipMemcpyDeviceToHost));
    if (out_stderr_rgb) HIP_TRY(hipMemcpy(out_stderr_rgb, d->rg_stderr.p, npx * 3 * sizeof(double), hipMemcpyDeviceToHost));
    if (state_out)
        if (int rc = r.state_out(state_out)) return rc;
    return copy_image_out("render_adaptive_budget", d->rg_rgba, d->rg_linear, p.precision, npx, out_rgba8, out_linear_rgb);
}
} // namespace rt

extern "C" int rttnw_render_adaptive_budget(rttnw_scene* s, const rttnw_camera_desc* cam, const rttnw_params* p, const rttnw_adaptive* a, const rttnw_budget* b,
                                            const double* state_in, double* state_out, double* out_linear_rgb, uint8_t* out_rgba8, uint32_t* out_spp,
                                            double* out_stderr_rgb, rttnw_stats* stats) {
    using namespace rt;
    // the refusals, in the header's order: none of them needs a device
    if (!p || !a || !b) { set_last_error("render_adaptive_budget: NULL argument (p, a or b)"); return RTTNW_ERR_INVALID; }
    if (int rc = refuse_adaptive_misuse("render_adaptive_budget", p, a)) return rc;
    if (int rc = refuse_host_output_misuse("render_adaptive_budget", a->reserved0, p)) return rc;
    if (b->reserved0 != 0) { set_last_error("render_adaptive_budget: b->reserved0 must be 0"); return RTTNW_ERR_INVALID; }
    if (a->rel_error == 0.0 && a->abs_error == 0.0) {
        set_last_error("render_adaptive_budget: rel_error and abs_error are both 0 (a priority relative to a tolerance of nothing ranks every noisy pixel +inf)");
        return RTTNW_ERR_INVALID;
    }
    uint32_t first_level = 0; // (not used: every round finds the levels of its own pixels)
    std::string err;
    if (state_in)
        if (int rc = refuse_state_misuse("render_adaptive_budget", true, *p, *a, cam, state_in, first_level, err)) { set_last_error(err); return rc; }
    if (int rc = validate(s, cam, p)) return rc;
    return adaptive_budget_render(s, cam, *p, *a, *b, state_in, state_out, out_linear_rgb, out_rgba8, out_spp, out_stderr_rgb, stats);
}

// ---------------------------------------------------------------------------------------------
// rttnw_render_adaptive_budget_denoised (include/rttnw_hip.h has the contract, DESIGN.md §10a "filter-guided budgeted form" the why): the budgeted
// form's rounds, ranked by the noise of the FILTERED image.  One rank on the scene's device, default stream.  Before round 0 the feature maps, which
// stay on the device.  A round: the raw maps of every pixel with their valid bytes (FilterStage::raw), rttnw_reconstruct's passes over
// them — a pixel may hold nothing yet —, the rank (sqrt of the filtered variance, and the selection's keys on the filtered maps), and from the keys on
// the budgeted form's own round: the select, the selection bytes, the census, one list pass per occupied level (budget_round_trace).  No byte
// survives a round — candidates are recomputed from the maps —, which is why a state can come in.  The filter that selects nothing is the call's
// output: it runs once more than the rounds, and once when there is no work.
// ---------------------------------------------------------------------------------------------
namespace rt {
static int adaptive_budget_denoised_render(::rttnw_scene* s, const rttnw_camera_desc* cam, const rttnw_params& p, const rttnw_adaptive& a,
                                           const rttnw_budget& bg, const rttnw_guided& g, const double* state_in, double* state_out, double* out_linear_rgb,
                                           uint8_t* out_rgba8, uint8_t* out_valid, uint32_t* out_spp, double* out_stderr_rgb, double* out_raw_linear_rgb,
                                           double* out_raw_stderr_rgb, rttnw_stats* stats) {
    RankRounds r(s, cam, p, a);
    DeviceState* d = r.d;
    const size_t npx = r.npx;
    const uint32_t B = r.B, n_levels = p.spp / B;
    const uint64_t round_pixels = bg.round_pixels ? bg.round_pixels : (uint64_t(npx) + 1u) / 2u;
    const hipStream_t stream = r.stream;
    // everything that allocates, before the first launch: the shared part with what a list pass over every block needs (the selection bytes are that
    // pass's active bytes), the filter's, and this call's own
    FilterStage f(r, true, true);
    DevBuf<uint8_t> select, marks;
    DevBuf<uint32_t> record;
    BudgetWorkspace work;
    if (int rc = r.open(select, r.n_blocks, state_in, state_out != nullptr, stats)) return rc;
    if (int rc = f.open()) return rc;
    HIP_TRY(marks.alloc(r.ppr)); HIP_TRY(record.alloc(1u + size_t(n_levels))); HIP_TRY(work.alloc(npx));

    // before round 0: the feature maps, the state that came in (or zero sums and zero noise state; the import's active bytes go to `marks` and are
    // not read), and nothing selected
    if (int rc = f.features(g.feature_spp)) return rc;
    HIP_TRY(hipEventRecord(r.ev0.get(), stream));
    if (int rc = r.start(marks.p)) return rc;
    HIP_TRY(hipMemsetAsync(select.p, 0, r.ppr, stream)); // (the rest of an edge tile is never selected: a round writes the bytes of the image's pixels only)
    uint64_t remaining = bg.samples, rounds = 0;
    std::vector<uint32_t> census(1u + size_t(n_levels));
    for (;;) {
        // 1. the raw maps of every pixel, 2. the filter, 3. the rank — the call's outputs, if this round selects nothing
        if (int rc = f.raw()) return rc;
        if (int rc = f.filter(g.denoise)) return rc;
        if (int rc = guided_budget_rank_launch(work, f.filtered(), f.filtered_variance(), f.raw_stderr.p, f.spp.p, p.spp, a.rel_error, a.abs_error, f.stderr_f.p,
                                               stream)) return rc;
        const uint64_t max_pixels = std::min<uint64_t>(round_pixels, remaining / B);
        if (max_pixels == 0) break; // the budget pays for no further pass
        // the selection on the rank's keys, and in one copy its record: the pixels selected and, per level, the length of the list over them
        if (int rc = budget_keys_round_launch(work, d->ad_state.p, p.width, p.height, p.spp, B, max_pixels, select.p, record.p, stream)) return rc;
        HIP_TRY(hipMemcpy(census.data(), record.p, census.size() * sizeof(uint32_t), hipMemcpyDeviceToHost));
        if (census[0] == 0) break; // no candidate is left
        ++rounds;
        remaining -= uint64_t(census[0]) * B;
        // 4. trace
        if (int rc = budget_round_trace(r, census, select.p, marks.p)) return rc;
    }
    if (state_out)
        if (int rc = r.export_state()) return rc;
    HIP_TRY(hipEventRecord(r.ev1.get(), stream));
    HIP_TRY(hipDeviceSynchronize());
    if (stats) {
        float ms = 0;
        HIP_TRY(hipEventElapsedTime(&ms, r.ev0.get(), r.ev1.get()));
        stats->kernel_ms = double(f.feature_ms) + double(ms);
        stats->samples = r.samples;
        stats->reserved |= uint32_t(std::min<uint64_t>(rounds, 0xFFFFu)) << 16;
    }
    // the outputs of the last filter that ran
    if (int rc = f.copy_out(out_linear_rgb, out_rgba8, out_valid, out_spp, out_stderr_rgb, out_raw_linear_rgb, out_raw_stderr_rgb)) return rc;
    return state_out ? r.state_out(state_out) : RTTNW_OK;
}
} // namespace rt

extern "C" int rttnw_render_adaptive_budget_denoised(rttnw_scene* s, const rttnw_camera_desc* cam, const rttnw_params* p, const rttnw_adaptive* a,
                                                     const rttnw_budget* b, const rttnw_guided* g, const double* state_in, double* state_out,
                                                     double* out_linear_rgb, uint8_t* out_rgba8, uint8_t* out_valid, uint32_t* out_spp, double* out_stderr_rgb,
                                                     double* out_raw_linear_rgb, double* out_raw_stderr_rgb, rttnw_stats* stats) {
    using namespace rt;
    const char* const call = "render_adaptive_budget_denoised";
    // the refusals, in the header's order: none of them needs a device
    if (!p || !a || !b || !g) { set_last_error(std::string(call) + ": NULL argument (p, a, b or g)"); return RTTNW_ERR_INVALID; }
    if (int rc = refuse_adaptive_misuse(call, p, a)) return rc;
    if (int rc = refuse_host_output_misuse(call, a->reserved0, p)) return rc;
    if (b->reserved0 != 0) { set_last_error(std::string(call) + ": b->reserved0 must be 0"); return RTTNW_ERR_INVALID; }
    if (a->rel_error == 0.0 && a->abs_error == 0.0) {
        set_last_error(std::string(call) + ": rel_error and abs_error are both 0 (a priority relative to a tolerance of nothing ranks every noisy pixel +inf)");
        return RTTNW_ERR_INVALID;
    }
    if (g->reserved0 != 0) { set_last_error(std::string(call) + ": g->reserved0 must be 0"); return RTTNW_ERR_INVALID; }
    if (int rc = denoise_refuse_params(call, "g->denoise.", g->denoise)) return rc;
    uint32_t first_level = 0; // (not used: every round finds the levels of its own pixels)
    std::string err;
    if (state_in)
        if (int rc = refuse_state_misuse(call, true, *p, *a, cam, state_in, first_level, err)) { set_last_error(err); return rc; }
    if (int rc = validate(s, cam, p)) return rc;
    return adaptive_budget_denoised_render(s, cam, *p, *a, *b, *g, state_in, state_out, out_linear_rgb, out_rgba8, out_valid, out_spp, out_stderr_rgb,
                                           out_raw_linear_rgb, out_raw_stderr_rgb, stats);
}
