// TEST INFRASTRUCTURE — host drivers of RUN-AHEAD (rttnw_amd/csrc/rt_core.hpp trav_trip_ahead, the trips of trace_kernel_plain's RUN_AHEAD instantiations):
// the host build of the tracing core (tests/hostsim/hostsim.cpp, compiled into this unit as it stands: its scenes, stacks, set-up and every one of
// its exports) plus
//   hostsim_render_run_ahead   a render whose walks take the kernel's trips, each held against the canonical walk of its ray
//   hostsim_wave_model_ahead   hostsim_wave_model's policy 4 (asynchronous shade phases) with run-ahead in its trips: what a form costs in step executions
//   hostsim_plan_run_ahead     the launch plan's run-ahead choice and trip length
// Never loaded by the rttnw_amd package.
#include "../hostsim/hostsim.cpp"

namespace {
// RUN-AHEAD (rt_core.hpp trav_trip_ahead: the trips of trace_kernel_plain's RUN_AHEAD instantiations).  A lane's walk does not depend on the other lanes of
// its wave — every walk starts at a trip's start, is suspended and taken up between trips, and a trip is the same steps whoever else takes it — so ONE
// lane driven through the kernel's trips until the kernel's finish rule says it is over is the kernel's walk.  render_ahead_t renders with those walks
// and holds each against the canonical walk of the same ray (closest_solid's steps), which it runs beside it.
// out: [0] walks, [1] / [2] node steps canonical / run-ahead, [3] / [4] record tests canonical / run-ahead, [5] records put aside, [6] walks whose canonical
// tests are NOT a subsequence, in order, of the run-ahead ones, [7] walks whose result differs (closest, primitive, instance, face, found), [8] walks
// that ended with a record still put aside, [9] walks in which a pop found the stack empty while a record was put aside, [10] walks with FEWER
// run-ahead node steps than canonical ones, [11] trips, [12] trips after which the walk driven by trav_trip_ahead — the function the kernel calls, whose walk
// makes the image — and its LOGGED TWIN (the same trip spelt out step by step, so that its record tests can be written down) stand at different cursors.
struct AheadTotals { uint64_t v[13] = {0, 0, 0, 0, 0, 0, 0, 0, 0, 0, 0, 0, 0}; };
// the record the next leaf step of (node, leaf_k, stash) tests: leaf code and index in the leaf, or 0 for an empty slot
static uint64_t next_test_of(int32_t node, uint32_t leaf_k, int32_t stash) {
    if (stash != 0) return uint64_t(uint32_t(stash)) << 8;
    if (node == CHILD_EMPTY) return 0;
    return uint64_t(uint32_t(node)) << 8 | (leaf_kind(node) == PRIM_INSTANCE ? 0u : leaf_k);
}
template <int NSTEPS, typename R>
static bool walk_ahead_checked(const SceneView<R>& sc, const Ray<R>& wray, R t_min, R& closest, HitRef& best, HostStack& stack, HostStack& stack2,
                               HostStack& stack3, LaneCounters& cnt, AheadTotals& tot, std::vector<uint64_t>& seq_a, std::vector<uint64_t>& seq_c) {
    seq_a.clear(); seq_c.clear();
    LaneCounters ca, cc, cl; // this walk's own counts
    Trav<R> tr, tl;
    trav_begin(tr, sc, wray, stack);
    trav_begin(tl, sc, wray, stack3);
    bool done_while_stashed = false;
    while (tr.node != TRAV_DONE) { // the kernel's loop: `unfinished` is taken between trips, where nothing is put aside
        tot.v[11]++;
        int32_t stash = 0, stash_l = 0; // (as in the kernel: the register lives inside the trip)
        trav_trip_ahead<NSTEPS>(tr, stash, sc, wray, t_min, stack, ca); // the kernel's trip
        // the logged twin: the same trip spelt out, so that the tests can be written down
        for (int k = 0; k < NSTEPS; ++k) {
            if (trav_stash_point_before(k) && trav_stash_point<false, false>(tl, stash_l, wray, stack3)) { tot.v[5]++; done_while_stashed = done_while_stashed || tl.node == TRAV_DONE; }
            if (tl.node >= 0) trav_node_step(tl, sc, wray, t_min, stack3, cl);
        }
        if (trav_wants_leaf_step(tl.node, stash_l)) {
            if (const uint64_t t = next_test_of(tl.node, tl.leaf_k, stash_l)) seq_a.push_back(t);
            trav_leaf_step_t<true>(tl, stash_l, sc, wray, t_min, stack3, cl);
        }
        if (stash != 0 || stash_l != 0 || trav_unfinished(tr.node, stash) != (tr.node != TRAV_DONE)) tot.v[8]++; // (a trip never ends with the register full)
        tot.v[12] += tr.node != tl.node || tr.sp != tl.sp || tr.leaf_k != tl.leaf_k || tr.found != tl.found || std::memcmp(&tr.closest, &tl.closest, sizeof(R)) != 0 ||
                     ca.nodes != cl.nodes || ca.prims != cl.prims;
    }
    Trav<R> tc;
    trav_begin(tc, sc, wray, stack2);
    while (tc.node != TRAV_DONE) {
        for (int k = 0; k < RT_NODE_STEPS; ++k)
            if (tc.node >= 0) trav_node_step(tc, sc, wray, t_min, stack2, cc);
        if (tc.node < 0 && tc.node != TRAV_DONE) {
            if (const uint64_t t = next_test_of(tc.node, tc.leaf_k, 0)) seq_c.push_back(t);
            trav_leaf_step(tc, sc, wray, t_min, stack2, cc);
        }
    }
    size_t j = 0;
    for (size_t i = 0; i < seq_a.size() && j < seq_c.size(); ++i) j += seq_a[i] == seq_c[j];
    tot.v[0]++; tot.v[1] += cc.nodes; tot.v[2] += ca.nodes; tot.v[3] += cc.prims; tot.v[4] += ca.prims;
    tot.v[6] += j != seq_c.size();
    const bool same = tr.found == tc.found && std::memcmp(&tr.closest, &tc.closest, sizeof(R)) == 0 &&
                      (!tr.found || (tr.best.prim == tc.best.prim && tr.best.inst == tc.best.inst && tr.best.aux == tc.best.aux));
    tot.v[7] += !same;
    tot.v[9] += done_while_stashed;
    tot.v[10] += ca.nodes < cc.nodes;
    cnt.nodes += ca.nodes; cnt.prims += ca.prims;
    closest = tr.closest; best = tr.best;
    return tr.found;
}
template <typename R>
static int render_ahead_t(rttnw_scene* s, const rttnw_camera_desc* cam, const rttnw_params* p, int node_steps, double* out_linear, uint64_t* out_totals,
                          int n_threads) {
    if (s->flat.walk_changes_frames) return RTTNW_ERR_UNSUPPORTED; // a record put aside is tested with the walk's one ray (launch_plan.hpp: such scenes never get it)
    if (node_steps < 1 || node_steps > 4) return RTTNW_ERR_INVALID;
    HostSetup<R> su(s, cam, p);
    HostScene<R>& hs = su.hs;
    RenderConsts& rc = su.rc;
    rc.sample_begin = p->sample_begin;
    plan_chunks(rc, p->spp, p->spp_chunk);
    rc.stack_depth = s->flat.stack_depth;
    const V3<R> background(R(p->background[0]), R(p->background[1]), R(p->background[2]));
    const R t_min = R(p->t_min);
    if (n_threads <= 0) n_threads = int(std::thread::hardware_concurrency());
    std::atomic<uint32_t> next_row{0};
    std::vector<AheadTotals> totals(n_threads);
    auto worker = [&](int tid) {
        HostStack stack, stack2, stack3;
        LaneCounters cnt;
        std::vector<uint64_t> seq_a, seq_c;
        AheadTotals& tot = totals[tid];
        for (;;) {
            const uint32_t row = next_row.fetch_add(1);
            if (row >= rc.height) break;
            for (uint32_t px = 0; px < rc.width; ++px) {
                V3<R> total; // (render_t's chains: chunk sums added in chunk order)
                for (uint32_t c = 0; c < rc.n_chunks; ++c) {
                    V3<R> acc;
                    uint32_t s0, s1;
                    chunk_samples(rc, c, s0, s1);
                    for (uint32_t si = s0; si < s1; ++si) {
                        PathState<R> ps;
                        path_begin(ps, su.camr, rc, px, row, si);
                        for (;;) { // path_step with the walk replaced
                            cnt.ray();
                            R closest;
                            HitRef best;
                            const bool found = node_steps == 1 ? walk_ahead_checked<1>(hs.view, ps.ray, t_min, closest, best, stack, stack2, stack3, cnt, tot, seq_a, seq_c)
                                               : node_steps == 2 ? walk_ahead_checked<2>(hs.view, ps.ray, t_min, closest, best, stack, stack2, stack3, cnt, tot, seq_a, seq_c)
                                               : node_steps == 3 ? walk_ahead_checked<3>(hs.view, ps.ray, t_min, closest, best, stack, stack2, stack3, cnt, tot, seq_a, seq_c)
                                                                 : walk_ahead_checked<4>(hs.view, ps.ray, t_min, closest, best, stack, stack2, stack3, cnt, tot, seq_a, seq_c);
                            if (!path_shade(ps, hs.view, rc, background, t_min, found, closest, best, cnt)) break;
                        }
                        acc = acc + ps.radiance;
                    }
                    total = total + acc;
                }
                const V3<R> mean = total / R(rc.spp);
                const size_t o = (size_t(row) * rc.width + px) * 3;
                out_linear[o] = double(mean.x); out_linear[o + 1] = double(mean.y); out_linear[o + 2] = double(mean.z);
            }
        }
    };
    std::vector<std::thread> th;
    for (int t = 1; t < n_threads; ++t) th.emplace_back(worker, t);
    worker(0);
    for (auto& t : th) t.join();
    for (int k = 0; k < 13; ++k) { out_totals[k] = 0; for (auto& t : totals) out_totals[k] += t.v[k]; }
    return RTTNW_OK;
}

// hostsim_wave_model's policy 4 — a lane whose walk is finished WAITS, the wave runs a shade phase once `b` lanes wait or none walks, trips of node steps + a
// leaf step in between — with RUN-AHEAD in the trips.  steps: node steps per trip.  form 0: the trip without run-ahead.  Form 1: a STASH POINT before the node
// steps k with bit k of `mask` set (mask 0: the kernel's own, rt_core.hpp trav_stash_point_before): a lane at a one-record leaf that is no instance, its
// register empty, puts the leaf aside and takes its next pending subtree (trav_stash_point, the kernel's own); the leaf step tests the record put aside,
// else the leaf the lane stands at (trav_leaf_step_t<true>).  Form 2: the leaf is put aside INSIDE the node step's descend — only where the nearest hit
// child is such a leaf and a second child is hit, which the walk then descends into instead of pushing it (a push and a pop saved, not a pop moved; the
// same walk as a stash point right behind a node step that pushed).
// out: [0] shade phases, [1] node-step executions, [2] node lane-steps, [3] leaf-step executions, [4] leaf lane-steps, [5] samples, [32] walks, [33] lanes the
// shade phases served, [36] records put aside, [37] stash points at which a lane did (the pop's code runs), [39] stash points a walking lane passed (the
// test's code runs), [60 + k] records put aside at the stash point before node step k, [38] lanes that came to a trip's end with the register full (must stay 0).
template <typename R>
void wave_model_ahead(rttnw_scene* s, const rttnw_camera_desc* cam, const rttnw_params* p, int steps, int form, int mask, int b, uint32_t n_waves,
                      uint32_t jobs_per_wave, uint64_t* out) {
    HostSetup<R> su(s, cam, p);
    su.plan_whole_frame(p);
    const HostScene<R>& hs = su.hs;
    const RenderConsts& rc = su.rc;
    const V3<R> background(R(p->background[0]), R(p->background[1]), R(p->background[2]));
    const R t_min = R(p->t_min);
    struct Lane {
        HostStack stack; Trav<R> tr; PathState<R> ps;
        bool alive = false, done = false, walking = false;
        int32_t stash = 0;
        uint32_t px = 0, row = 0, s = 0, s_end = 0;
    };
    NoCounters cnt;
    std::vector<Lane> L(64);
    const int points = mask ? mask : 1; // (the kernel's: the stash point at the trip's start, rt_core.hpp trav_stash_point_before)
    for (uint32_t w = 0; w < n_waves; ++w) {
        uint64_t next = uint64_t(w) * (rc.n_jobs / n_waves) / 64 * 64;
        const uint64_t end = next + jobs_per_wave;
        for (auto& l : L) { l.alive = l.done = l.walking = false; l.s = l.s_end = 0; l.stash = 0; }
        for (;;) {
            uint32_t n_walk = 0, n_wait = 0;
            for (auto& l : L) {
                if (l.done) continue;
                if (l.stash != 0) out[38]++;
                if (l.walking && !trav_unfinished(l.tr.node, l.stash)) l.walking = false; // its walk is over: waits for the shade phase
                if (l.walking) ++n_walk; else ++n_wait;
            }
            if (n_walk + n_wait == 0) break;
            if (n_walk == 0 || n_wait >= uint32_t(b)) { // the shade phase: shade, job hand-out, path begin, walk begin for the waiting lanes
                uint32_t served = 0;
                for (auto& l : L) {
                    if (l.done || l.walking) continue;
                    ++served;
                    if (l.alive) {
                        l.alive = path_shade(l.ps, hs.view, rc, background, t_min, l.tr.found, l.tr.closest, l.tr.best, cnt);
                        if (!l.alive) { ++l.s; out[5]++; }
                    }
                    while (!l.alive && l.s >= l.s_end) {
                        if (next >= end || next >= rc.n_jobs) { l.done = true; break; }
                        const JobInfo ji = job_decode(rc, uint32_t(next++));
                        l.px = ji.px; l.row = ji.row; l.s = ji.s; l.s_end = ji.s_end;
                    }
                    if (l.done) continue;
                    if (!l.alive) { path_begin(l.ps, su.camr, rc, l.px, l.row, l.s); l.alive = true; }
                    trav_begin(l.tr, hs.view, l.ps.ray, l.stack);
                    l.walking = true;
                    out[32]++;
                }
                out[0]++; out[33] += served;
                continue;
            }
            for (int k = 0; k < steps; ++k) { // the trip
                if (form == 1 && ((points >> k) & 1)) {
                    uint32_t passed = 0, put = 0;
                    for (auto& l : L) if (!l.done && l.walking) { ++passed; put += trav_stash_point<false, false>(l.tr, l.stash, l.ps.ray, l.stack); }
                    out[36] += put; out[37] += put != 0; out[39] += passed != 0;
                    if (k < 4) out[60 + k] += put;
                }
                uint32_t n = 0;
                for (auto& l : L) if (!l.done && l.walking && l.tr.node >= 0) {
                    const int32_t sp_before = l.tr.sp;
                    trav_node_step(l.tr, hs.view, l.ps.ray, t_min, l.stack, cnt); ++n;
                    if (form == 2 && l.tr.sp > sp_before && trav_stash_point<false, false>(l.tr, l.stash, l.ps.ray, l.stack)) out[36]++;
                }
                if (n) { out[1]++; out[2] += n; }
            }
            uint32_t n = 0;
            for (auto& l : L) if (!l.done && l.walking && trav_wants_leaf_step(l.tr.node, l.stash)) {
                if (form) trav_leaf_step_t<true>(l.tr, l.stash, hs.view, l.ps.ray, t_min, l.stack, cnt);
                else trav_leaf_step(l.tr, hs.view, l.ps.ray, t_min, l.stack, cnt);
                ++n;
            }
            if (n) { out[3]++; out[4] += n; }
        }
    }
}
} // namespace

extern "C" {
// A render whose walks take the kernel's run-ahead trips of `node_steps` node steps, each held against the canonical walk of its ray (render_ahead_t above has
// the thirteen totals).  RTTNW_ERR_UNSUPPORTED for a scene whose walk changes frames.
int hostsim_render_run_ahead(rttnw_scene* s, const rttnw_camera_desc* cam, const rttnw_params* p, int node_steps, double* out_linear, uint64_t* out_totals,
                             int n_threads) {
    if (!s || !s->committed || !cam || !p || !out_linear || !out_totals) return RTTNW_ERR_INVALID;
    return p->precision == RTTNW_F32 ? render_ahead_t<float>(s, cam, p, node_steps, out_linear, out_totals, n_threads)
                                     : render_ahead_t<double>(s, cam, p, node_steps, out_linear, out_totals, n_threads);
}
int hostsim_wave_model_ahead(rttnw_scene* s, const rttnw_camera_desc* cam, const rttnw_params* p, int steps, int form, int mask, int b, uint32_t n_waves,
                             uint32_t jobs_per_wave, uint64_t* out) {
    if (!s || !s->committed || !cam || !p || !out || steps < 1 || steps > 8 || form < 0 || form > 2 || s->flat.walk_changes_frames) return RTTNW_ERR_INVALID;
    if (p->precision == RTTNW_F32) wave_model_ahead<float>(s, cam, p, steps, form, mask, b, n_waves, jobs_per_wave, out);
    else wave_model_ahead<double>(s, cam, p, steps, form, mask, b, n_waves, jobs_per_wave, out);
    return RTTNW_OK;
}
// The plan's run-ahead choice (LaunchPlan::run_ahead, bit 7 of rttnw_stats.reserved) and its trip length: run_ahead | steps << 1, or -1.
// override: RTTNW_RUN_AHEAD as plan_launch takes it (-1 unset, 0 off, 1 on).
int hostsim_plan_run_ahead(rttnw_scene* s, uint32_t real_bytes, int count, int listed, int forced, int override) {
    if (!s || !s->committed || (real_bytes != 4 && real_bytes != 8) || forced < 0 || forced > 3) return -1;
    const LaunchPlan pl = plan_launch(s->flat, real_bytes, count != 0, listed != 0, KernelForm(forced), 0, override);
    return (pl.run_ahead ? 1 : 0) | ((pl.run_ahead ? RUN_AHEAD_STEPS : pl.steps) << 1);
}
}
