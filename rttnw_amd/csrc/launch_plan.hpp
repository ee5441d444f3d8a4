// launch_plan.hpp — which kernel instantiation a scene runs and how its launch is shaped: decided ONCE, by a pure host function over the lowered scene
// (plan_launch), and read by the kernel lookup, the launch and rttnw_stats.reserved alike (render_tiles.hpp).  No __global__ function, no device call: of
// rt_core.hpp (host-and-device code the host compiler builds too) it needs SHAPES_*, RT_NODE_STEPS and the arithmetic namespace (tests/hostsim builds it).
#pragma once
#include "rt_core.hpp"
#include "scene_lower.hpp"
#include <algorithm>
#include <cstring>

#ifndef RT_TINY_TREE_STEPS
#define RT_TINY_TREE_STEPS 3 // node steps per walk trip of the lane-owns-path kernel for top trees of <= 16 nodes (RT_NODE_STEPS otherwise)
#endif
// Every decoupled kernel walks the QUANTISED records (rt_types.hpp Bvh4QNode; LaunchPlan::quantised).  (Mid-round-4: f64 +4 / +7 %, f32 -2 % against the
// f32 records.  At the round's end — no slot tests, no instance code, 13-real path slots — the f32 kernel moves 6.2 TB/s and little else, and half the
// node bytes are worth +10 %: spheres_1m f32 433 -> 476 Msamples/s on these records.)
#ifndef RT_F64_BLOCK
#define RT_F64_BLOCK 1024 // threads per block of the LDS-resident f64 kernel (4 waves/SIMD at 128 VGPRs; see the Makefile's f64 flags and profiles/r03/README.md)
#endif
#ifndef RT_SLOTS
#define RT_SLOTS 128
#endif
// LDS stack entries of the decoupled kernel: 16 for f32; 13 for f64, whose queues are twice as wide: THREE 256-thread blocks must fit a CU's 160 KB,
// or the kernel runs at 2 waves per SIMD however few registers it is held to.  gfx950 hands LDS out in granules of 1280 BYTES (128 to a CU): a block
// of 42 granules (53 760 B) fits three times, one of 54 016 B does not — measured in round 5 (profiles/r05/README.md: 445 against 344 Msamples/s
// on spheres_1m; hipOccupancyMaxActiveBlocksPerMultiprocessor says 3 for both).  Rounds 1-4 asked for 54 272 B with 12 entries — the runtime's
// answer was 3, SQ_WAVE_CYCLES said 2 of 3 waves were ever resident — so the f64 decoupled kernels ran a third short of their waves: the ray slot
// queue as bytes (slots are < 128) and 13 entries make it 53 760 B exactly (the spill strip in global memory takes the rare deeper entries).
#ifndef RT_F64_WAVE_STACK
#define RT_F64_WAVE_STACK 13
#endif

namespace rt {
inline namespace RT_ARITH_NS {

constexpr int TRACE_BLOCK = 256;
constexpr int RUN_AHEAD_STEPS = 3; // node steps per trip with run-ahead (final_scene f64: two 1645, three 1704 against 1664 Msamples/s without; profiles/LEDGER.md)
constexpr uint32_t SLOTS_PER_WAVE = RT_SLOTS; // paths owned by one wave64: 64 being traversed + up to 64 queued
constexpr uint32_t QCAP = RT_SLOTS;           // capacity of a wave's ray queue and hit queue (entries)
static_assert(QCAP == SLOTS_PER_WAVE, "a slot has at most one ray or hit in flight: the queues never hold more entries than the wave has slots");
static_assert(SLOTS_PER_WAVE <= 256u, "slot numbers travel as bytes");

// bytes of LDS one wave of the decoupled kernel needs: ray queue (7 reals + slot), hit queue (t + prim + inst + meta), traversal stacks
template <typename R> constexpr uint32_t wave_stack_entries() { return sizeof(R) == 8 ? uint32_t(RT_F64_WAVE_STACK) : LDS_STACK_ENTRIES; }
template <typename R> constexpr uint32_t wave_lds_bytes(uint32_t stack_depth, bool no_time = false) {
    // ray queue (7 reals) + hit t | hit prim, inst, meta (words) | ray slot (bytes) | stack: + the spare slot
    return (no_time ? 7u : 8u) * QCAP * uint32_t(sizeof(R)) + 3u * QCAP * 4u + QCAP + (wave_stack_entries<R>() + 1u) * 64u * 4u;
}
constexpr uint32_t LDS_GRANULE_BYTES = 1280u, LDS_BYTES_PER_CU = 160u * 1024u; // gfx950: 128 granules per CU
constexpr uint32_t lds_blocks_per_cu(uint32_t block_bytes) {
    return block_bytes == 0u ? 1024u : LDS_BYTES_PER_CU / ((block_bytes + LDS_GRANULE_BYTES - 1u) / LDS_GRANULE_BYTES * LDS_GRANULE_BYTES);
}
// waves of ONE block that fills a CU (the LEAN flavour of the decoupled kernel): as many as the CU's LDS granules hold, at most 16 (4 per SIMD)
constexpr uint32_t wave_block_waves(uint32_t wave_bytes) {
    uint32_t n = 16u;
    while (n > 4u && (n * wave_bytes + LDS_GRANULE_BYTES - 1u) / LDS_GRANULE_BYTES > LDS_BYTES_PER_CU / LDS_GRANULE_BYTES) --n;
    return n;
}
static_assert(lds_blocks_per_cu(wave_lds_bytes<double>(0) * 4u) >= 3u, "the f64 decoupled kernel's block must fit a CU's LDS three times");
static_assert(lds_blocks_per_cu(wave_lds_bytes<float>(0) * 4u) >= 3u, "the f32 decoupled kernel's block must fit a CU's LDS three times");

// RTTNW_KERNEL (experiments and tests): the caller reads the environment, plan_launch does not
enum class KernelForm : int { AUTO = 0, PLAIN = 1, PLAINGLOBAL = 2, WAVE = 3 };
inline KernelForm kernel_form_named(const char* v) {
    return !v ? KernelForm::AUTO : !std::strcmp(v, "plain") ? KernelForm::PLAIN : !std::strcmp(v, "plainglobal") ? KernelForm::PLAINGLOBAL : !std::strcmp(v, "wave") ? KernelForm::WAVE : KernelForm::AUTO;
}

// Bits 0-7 of rttnw_stats.reserved: which kernel form a render ran (the tests and bench.py's roofline read them).  Bits 0-5 are LaunchPlan::form_bits,
// bit 6 is known only once the scene's records are on the device, bit 7 is LaunchPlan::run_ahead; bits 8 / 9 belong to rttnw_render_multi's gather.
//   0 the decoupled kernel (else lane-owns-path)   1 node records resident in LDS (the form bench.py's roofline calls issue-bound)   2 three node steps per
//   trip WITHOUT run-ahead (tiny top trees; with bit 7 a trip has RUN_AHEAD_STEPS = three node steps whatever this bit says)   3 a walk that never changes frames (rt_core.hpp SHAPES_NONE / SHAPES_SINGLE)   4 ... the one that tests single wrapped records in
//   place (SHAPES_SINGLE)   5 ... in the LEAN flavour (SHAPES_*_NT)   6 the decoupled kernel walked the interleaved node + sphere buffer (render_common.hpp)
//   7 the lane-owns-path kernel's trips ran with run-ahead (rt_core.hpp trav_trip_ahead) — the launch's own instantiation: never set by a counting render
// Bits 3-5 say what the SCENE is eligible for: a counting render (collect_counters) runs the SHAPES_FAST / SHAPES_GENERAL instantiation — the only ones
// that tally — and still reports them as its timed twin would.
enum : uint32_t { FORM_DECOUPLED = 1u, FORM_LDS_NODES = 2u, FORM_THREE_STEPS = 4u, FORM_NO_FRAMES = 8u, FORM_SINGLE = 16u, FORM_LEAN = 32u, FORM_INTERLEAVED = 64u, FORM_RUN_AHEAD = 128u };

// Everything a render decides about its trace launches before it touches the device, which adds the occupancy answer and its CUs (the grid) and bit 6.
struct LaunchPlan {
    bool decoupled; // the form: paths decoupled from lanes (trace_kernel), else a lane owns a path (trace_kernel_plain)
    bool lds;       // lane-owns-path: node records (and what else fits) staged in LDS, in one large block per CU
    bool count;     // the tallying instantiation
    bool list;      // the active-list instantiation (rttnw_render_adaptive's refinement passes; non-counting forms only)
    bool quantised; // the kernel walks the quantised node records (DeviceScene::ensure_quant4)
    int shapes;     // rt_core.hpp SHAPES_*
    int steps;      // node steps per walk trip of the lane-owns-path kernel (its trips without run-ahead)
    bool run_ahead; // ... whose trips put one-record leaves aside and walk on, and are then RUN_AHEAD_STEPS node steps long (trace_kernel_plain RUN_AHEAD;
                    // bit 7 of rttnw_stats.reserved)
    int block;      // threads per block
    uint32_t lds_nodes, lds_recs[6]; // RenderConsts::lds_nodes / lds_recs
    uint32_t staged_bytes;           // LDS bytes of the arrays staged behind the stacks (Perlin tables, record arrays)
    uint32_t lds_bytes;              // dynamic LDS of a block
    uint32_t form_bits;              // FORM_* bits 0-5
};

// Two forms of the same loop (DESIGN.md "Kernels"): measured on MI355X the lane-owns-a-path form wins on shallow scenes (cornell_box,
// final_scene: <= ~1k nodes), the decoupled form on deep BVHs where traversal lengths vary most (1M spheres).
// (crossover measured on spheres_1m-like scenes of 4e3 - 1e5 spheres, 512x512 spp 256, lane-owns-path against decoupled, Msamples/s.  Round 3: f32 at
// ~24 k 4-wide nodes, f64 at ~50 k.  After round 4 — quantised records, no instance code, 13-real path slots, the f64 unit split — the decoupled kernel
// takes over much earlier: f32 5.7 k nodes 7158 / 6646, 9.9 k 5272 / 5403, 15.4 k 3917 / 4460, 28.3 k 2273 / 3184; f64 9.9 k 4776 / 4039, 15.4 k
// 3559 / 3340, 19.6 k 2818 / 2898, 28.3 k 1979 / 2332, 50.9 k 1223 / 1722)
// (round 5 — asynchronous shade phases in the lane-owns-path kernel, the f64 decoupled kernel at three blocks per CU: f32 9.9 k nodes 5441 / 5350,
// 15.4 k 4180 / 4483, 19.6 k 3400 / 3911; f64 9.9 k 5168 / 4898, 15.4 k 3960 / 4153, 19.6 k 3166 / 3667; RTTNW_F64_STRICT 15.4 k 4015 / 4110 —
// profiles/r05/README.md: both cross at ~13 k records)
// (later in round 5 — the decoupled kernel keeps a slot's ray in LDS, +5 .. 9 %: f32 5.7 k nodes 7216 / 7620, 7.6 k 6101 / 6840, 9.9 k 5410 / 6371; f64
// 5.7 k 6974 / 6577, 7.6 k 5919 / 5817, 9.9 k 5150 / 5318, 15.4 k 3941 / 4450; RTTNW_F64_STRICT 7.6 k 5945 / 5783, 9.9 k 5195 / 5224: f32 crosses
// at ~5 k records, f64 at ~9 k)
// real_bytes: sizeof the arithmetic type; wave_block: RTTNW_WAVE_BLOCK=<threads> (experiments), 0 = unset; run_ahead: RTTNW_RUN_AHEAD (experiments and
// tests) 0 = off, 1 = on wherever an instantiation has it, -1 = unset: the plan's own choice.
inline LaunchPlan plan_launch(const FlatScene& flat, size_t real_bytes, bool count, bool listed, KernelForm forced, int wave_block, int run_ahead = -1) {
    LaunchPlan pl{};
    pl.count = count; pl.list = listed && !count; pl.steps = RT_NODE_STEPS;
    const uint32_t n4 = flat.total_nodes4();
    const bool f32 = real_bytes == 4, gen = flat.needs_general, lean = flat.lean();
    pl.decoupled = forced == KernelForm::AUTO ? n4 >= (f32 ? 5000u : 9000u) : forced == KernelForm::WAVE;
    if (!pl.decoupled) {
        // Small scenes: node array in LDS, in ONE large block per CU so that nodes + all the lanes' stacks fit in 160 KB:
        // 1024 threads in both precisions (4 waves/SIMD at <= 128 VGPRs; RT_F64_BLOCK: the f64 code spills ~26 registers to get there)
        const uint32_t lds_block = f32 ? 1024u : uint32_t(RT_F64_BLOCK);
        const size_t resident = lds_form_bytes(n4, flat.stack_depth, lds_block);
        pl.lds = forced != KernelForm::PLAINGLOBAL && resident <= LDS_BYTES_PER_CU;
        pl.block = pl.lds ? int(lds_block) : TRACE_BLOCK;
        size_t staged = 0;
        if (pl.lds) {
            pl.lds_nodes = n4;
            // the scene's Perlin tables ride along in LDS when they fit behind the stacks (trace_kernel_plain)
            const size_t n_perlin = flat.perlin_vec.size() / 768u, perlin_bytes = lds_perlin_bytes(n_perlin, real_bytes);
            if (n_perlin > 0 && n_perlin < 256 && n4 <= LDS_NODES_MASK && resident + perlin_bytes <= LDS_BYTES_PER_CU) {
                pl.lds_nodes |= uint32_t(n_perlin) << LDS_PERLIN_SHIFT;
                staged = lds_pad32(perlin_bytes);
            }
            // ... and so do the record arrays of the leaf steps, each if it still fits (chains, rectangles, moving spheres, cubes; the spheres' material slots)
            const size_t counts[5] = {flat.insts.size(), flat.rects.size(), flat.moving.size(), flat.boxes.size(), flat.sphere_mat_is_index ? 0 : flat.sphere_mat.size()};
            const size_t sizes[5] = {f32 ? sizeof(InstanceRec<float>) : sizeof(InstanceRec<double>), f32 ? sizeof(RectRec<float>) : sizeof(RectRec<double>),
                                     f32 ? sizeof(MovingSphereRec<float>) : sizeof(MovingSphereRec<double>), f32 ? sizeof(BoxRec<float>) : sizeof(BoxRec<double>), 4};
            for (int k = 0; k < 5; ++k) {
                const size_t bytes = lds_pad32(counts[k] * sizes[k]);
                if (counts[k] == 0 || resident + staged + bytes > LDS_BYTES_PER_CU) continue;
                pl.lds_recs[k] = uint32_t(counts[k]);
                staged += bytes;
            }
        }
        pl.staged_bytes = uint32_t(staged);
        pl.lds_bytes = uint32_t(lds_form_bytes(pl.lds ? n4 : 0u, flat.stack_depth, uint32_t(pl.block)) + staged);
        // a top tree of one or two levels (cornell_box: 6 nodes; its walks are mostly entered instances) takes three node steps per trip
        // (the counting variant's tallied loop is written for two: same steps per lane, same counters)
        const bool three_steps = pl.lds && n4 <= 16u && RT_NODE_STEPS == 2;
        if (three_steps && !count) pl.steps = RT_TINY_TREE_STEPS;
        // ... and a scene whose walk never changes frames the instantiation without instance code (rt_core.hpp SHAPES_NONE: final_scene — its one
        // instance record is the bare chain of the cluster's world-space copies), or the one that keeps the test of single wrapped records
        // (SHAPES_SINGLE); of those two, the LEAN flavour where the scene holds no moving sphere, no medium and only solid colours (SHAPES_*_NT)
        const bool no_frames = pl.lds && !gen && !flat.walk_changes_frames;
        pl.shapes = gen                    ? SHAPES_GENERAL // rare graph shapes: the instantiation that carries their code
                    : !no_frames || count  ? SHAPES_FAST
                    : flat.has_instance_leaves ? (lean ? SHAPES_SINGLE_NT : SHAPES_SINGLE)
                                               : (lean ? SHAPES_NONE_NT : SHAPES_NONE);
        // RUN-AHEAD: only the timed instantiations of a walk that never changes frames have it (a record put aside is tested with the walk's one ray); the
        // counting ones keep the canonical sequence of steps, whose counts the tests pin.  Left to itself the plan gives it to the scenes that meet no
        // instance leaf at all (SHAPES_NONE / SHAPES_NONE_NT: final_scene); the override turns it on for the SINGLE family too, or off.
        const bool can_run_ahead = no_frames && !count && !gen;
        pl.run_ahead = can_run_ahead && (run_ahead < 0 ? !flat.has_instance_leaves : run_ahead != 0);
        const bool in_lds = pl.lds_nodes != 0u, eligible = no_frames && in_lds;
        pl.form_bits = (in_lds ? FORM_LDS_NODES : 0u) | (three_steps ? FORM_THREE_STEPS : 0u) | (eligible ? FORM_NO_FRAMES : 0u) |
                       (eligible && flat.has_instance_leaves ? FORM_SINGLE : 0u) | (eligible && lean ? FORM_LEAN : 0u);
    } else {
        pl.quantised = true;
        // (a scene without any instance record takes the instantiation whose walk never changes frames, rt_core.hpp SHAPES_NONE)
        const bool no_inst = !gen && !flat.has_instance_leaves;
        pl.shapes = gen ? SHAPES_GENERAL : !no_inst || count ? SHAPES_FAST : lean ? SHAPES_NONE_NT : SHAPES_NONE;
        // (the LEAN flavour: ONE block per CU of as many waves as its LDS holds — 13 in f64, where three 4-wave blocks make 12)
        const bool lean_kernel = pl.shapes == SHAPES_NONE_NT;
        const uint32_t wave_bytes = f32 ? wave_lds_bytes<float>(flat.stack_depth, lean_kernel) : wave_lds_bytes<double>(flat.stack_depth, lean_kernel);
        pl.block = lean_kernel ? int(wave_block_waves(wave_bytes)) * 64 : TRACE_BLOCK;
        // (clamped to what a CU's LDS holds: 16 f64 waves would ask for 198 KB and fail the whole render instead of running with 13)
        if (wave_block >= 64 && wave_block % 64 == 0 && wave_block <= (lean_kernel ? 1024 : TRACE_BLOCK)) pl.block = lean_kernel ? std::min(wave_block, pl.block) : wave_block;
        pl.lds_bytes = wave_bytes * uint32_t(pl.block / 64);
        pl.form_bits = FORM_DECOUPLED | (no_inst ? FORM_NO_FRAMES : 0u) | (no_inst && lean ? FORM_LEAN : 0u);
    }
    return pl;
}

} // namespace RT_ARITH_NS
} // namespace rt
