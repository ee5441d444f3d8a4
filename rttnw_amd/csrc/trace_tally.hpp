// trace_tally.hpp — DEBUG / MEASUREMENT ONLY: one phase of the lane-owns-path kernel (trace_kernels.hpp trace_kernel_plain) with the
// wave clock read between its parts and the trips of its walk loop tallied.  Compiled into the COUNT = true instantiations only
// (rttnw_params.collect_counters != 0: the untimed counting pass of bench.py, RTTNW_DEBUG_SCHED); the product kernels never contain it.
// One PHASE = start the walks of the lanes that have none, trips until at most RT_ASYNC_SLACK walks are unfinished, shade the finished ones:
// the steps of the kernel's own phase, in the same order.  The trips are the CANONICAL ones (NSTEPS node steps + a leaf step: the counts the tests pin)
// unless rc.scene_flags has SCENE_TALLY_AHEAD — collect_counters >= 2 on a scene whose timed kernel runs RUN-AHEAD (render_tiles.hpp) —: then they are
// that kernel's (rt_core.hpp trav_trip_ahead: a stash point, RUN_AHEAD_STEPS node steps, the leaf step that tests a record put aside), so that lanes per
// step, visits and record tests are the timed kernel's.
//   prof[0..3]  wave clock: job hand-out / path begin / BVH walk / shade;  [15] media + hit record part of shade
//   prof[4]     trips of the walk loop ([7] with a node lane, [8] with a leaf lane), [5] / [6] lane steps served (node / leaf)
//   prof[9]     phases, [10] lanes a phase shaded, [11] phases that began paths, [12] paths begun
//   prof[13,14] clock of the node steps / the leaf steps
//   counters->dbg[16..], [80..], [144..] (collect_counters 2, 3): leaf clock by the set of record kinds served (2: dbg[16 + set], count dbg[80 + set]; bit k =
//               record kind k, bit 5 = empty slot); histograms (3) of trips per walk [16..], of the trips of a phase [80..], and trips by what the walk found
//               [144 + class] / walks [152 + class]: class 0 miss, 1 + kind (sphere, moving, rect, box), 6 anything inside an instance
#pragma once

namespace rt {
inline namespace RT_ARITH_NS {

template <int NSTEPS, typename R, typename Stack, typename Cnt>
__device__ __forceinline__ void plain_phase_tallied(bool done, bool& alive, bool& walking, Trav<R>& tr, uint32_t& my_trips, uint32_t px, uint32_t row, uint32_t& s, uint32_t s_end,
                                                    V3<R>& acc, PathState<R>& ps, const CameraRec<R>& cam, const RenderConsts& rc, const SceneView<R>& sc, V3<R> background,
                                                    R t_min, Stack& stack, Cnt& cnt, unsigned long long* prof, DeviceCounters* __restrict__ counters, uint32_t lane,
                                                    long long tk0) {
    const long long tk1 = clock64();
    const bool fresh_path = !done && !walking && !alive && s < s_end;
    const unsigned long long bm = __ballot(fresh_path);
    if (fresh_path) {
        path_begin(ps, cam, rc, px, row, s);
        alive = true;
    }
    const long long tk2 = clock64();
    const bool fresh_walk = !done && !walking && alive;
    if (fresh_walk) { cnt.ray(); trav_init(tr, sc); walking = true; my_trips = 0; }
    if constexpr (Cnt::NO_INST) trav_set_ray(tr, ps.ray, stack);
    else if (fresh_walk) trav_set_ray(tr, ps.ray, stack);
    if (fresh_walk) trav_reject_unwalkable(tr, ps.ray);
    uint32_t phase_trips = 0;
    const bool ahead = (rc.scene_flags & SCENE_TALLY_AHEAD) != 0u; // (wave-uniform)
    for (;;) {
        const bool unfinished = walking && tr.node != TRAV_DONE;
        const unsigned long long act = __ballot(unfinished);
        if (act != 0ull) {
            ++phase_trips;
            unsigned long long n_node = 0, n_leaf = 0;
            bool any_node = false;
            const long long q0 = clock64();
            int32_t stash = 0; // (run-ahead: lives inside the trip, trav_trip_ahead)
            if (unfinished) {
                ++my_trips;
                if (ahead) {
#pragma unroll
                    for (int k = 0; k < RUN_AHEAD_STEPS; ++k) {
                        if (trav_stash_point_before(k)) trav_stash_point<Cnt::NO_INST, Cnt::NO_INST_LEAF>(tr, stash, ps.ray, stack);
                        if (tr.node >= 0) { ++n_node; trav_node_step(tr, sc, ps.ray, t_min, stack, cnt); }
                    }
                } else {
#pragma unroll
                    for (int k = 0; k < NSTEPS; ++k)
                        if (tr.node >= 0) { ++n_node; trav_node_step(tr, sc, ps.ray, t_min, stack, cnt); }
                }
            }
            any_node = __ballot(n_node != 0ull) != 0ull;
            const long long q1 = clock64();
            const bool is_leaf = unfinished && trav_wants_leaf_step(tr.node, stash); // (nothing put aside: the lanes at a leaf)
            const unsigned long long lm = __ballot(is_leaf);
            uint32_t kmask = 0;
            if (rc.profile == 2u) {
                const int32_t lf = stash != 0 ? stash : tr.node;
                const uint32_t kd = lf == CHILD_EMPTY ? 5u : leaf_kind(lf);
#pragma unroll
                for (uint32_t k = 0; k < 6; ++k) kmask |= __ballot(is_leaf && kd == k) != 0ull ? (1u << k) : 0u;
            }
            const long long q1b = clock64();
            if (is_leaf) { ++n_leaf; trav_leaf_step_t<true>(tr, stash, sc, ps.ray, t_min, stack, cnt); } // (with nothing put aside: trav_leaf_step)
            const long long q2 = clock64();
            prof[5] += n_node;
            prof[6] += n_leaf;
            if (lane == uint32_t(__ffsll((long long)act) - 1)) {
                prof[4] += 1;
                prof[7] += any_node;
                prof[8] += lm != 0ull;
                prof[13] += (unsigned long long)(q1 - q0);
                prof[14] += (unsigned long long)(q2 - q1b);
                if (kmask && rc.profile == 2u) {
                    atomicAdd(&counters->dbg[16 + kmask], (unsigned long long)(q2 - q1b));
                    atomicAdd(&counters->dbg[80 + kmask], 1ull);
                }
            }
        }
        const unsigned long long um = __ballot(walking && tr.node != TRAV_DONE);
        if (um == 0ull) break;
        if (uint32_t(__popcll(um)) <= uint32_t(RT_ASYNC_SLACK) && __ballot(walking && tr.node == TRAV_DONE) != 0ull) break;
    }
    const long long tk3 = clock64();
    long long tk3b = tk3;
    const bool shade_now = walking && tr.node == TRAV_DONE;
    const unsigned long long sm = __ballot(shade_now);
    if (shade_now) {
        walking = false;
        if (rc.profile == 3u) {
            atomicAdd(&counters->dbg[16 + min(my_trips, 63u)], 1ull); // histogram of trips per walk
            const uint32_t cls = !tr.found ? 0u : (tr.best.inst >= 0 ? 6u : 1u + ref_kind(tr.best.prim));
            atomicAdd(&counters->dbg[144 + cls], (unsigned long long)my_trips);
            atomicAdd(&counters->dbg[152 + cls], 1ull);
        }
        HitRecord<R> rec;
        const bool hit = world_hit_finish(sc, ps.ray, t_min, ps.key, ps.bounce, rc.quirks, tr.found, tr.closest, tr.best, rec, cnt);
        tk3b = clock64();
        if (!hit) {
            ps.radiance = ps.throughput * background;
            if (tr.closest != tr.closest) ps.radiance = V3<R>(tr.closest, tr.closest, tr.closest); // (as path_shade: a ray that was not walked)
            keep_rounded(ps.radiance);
            alive = false;
        } else {
            V3<R> att, emitted;
            const bool cont = shade(sc, rec, ps.key, ps.bounce, ps.ray, att, emitted, cnt);
            ps.radiance = ps.throughput * emitted;
            keep_rounded(ps.radiance);
            if (cont) { ps.throughput = ps.throughput * att; ps.bounce += 1; }
            alive = cont && ps.bounce < rc.max_depth;
        }
        if (!alive) {
            acc = acc + ps.radiance;
            ++s;
        }
    }
    if (rc.profile == 3u && lane == 0) atomicAdd(&counters->dbg[80 + min(phase_trips, 63u)], 1ull); // trips of a phase
    const long long tk4 = clock64();
    if (lane == 0) {
        prof[0] += (unsigned long long)(tk1 - tk0);
        prof[1] += (unsigned long long)(tk2 - tk1);
        prof[2] += (unsigned long long)(tk3 - tk2);
        prof[3] += (unsigned long long)(tk4 - tk3);
        prof[15] += (unsigned long long)(tk3b - tk3);
        prof[9] += 1;
        prof[10] += (unsigned long long)__popcll(sm);
        prof[11] += bm != 0ull;
        prof[12] += (unsigned long long)__popcll(bm);
    }
}

} // namespace RT_ARITH_NS
} // namespace rt
