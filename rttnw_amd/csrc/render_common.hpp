// render_common.hpp — host-side state of the device half of include/rttnw_hip.h, shared by its translation units:
//   render_api.cpp   device state, validation and the single-GPU extern "C" entry points (host code only, like the next two)
//   render_multi.cpp rttnw_render_multi + RCCL; render_multi.hpp: its plan and steps, which the adaptive forms over ranks walk too
//   render_adaptive_api.cpp  the adaptive family beyond rttnw_render_adaptive: multi, resume, region, denoised, preview, budget
//                    (adaptive_state.hpp: the state's host side, plain C++)
//   render_f32.hip   the F32 instantiation of the kernels (trace_kernels.hpp, adaptive_kernels.hpp) and of their launch code (render_tiles.hpp,
//                    adaptive_launch.hpp)
//   render_f64.hip   the F64 instantiation — a translation unit of its own because its code wants other compiler settings
//                    than the f32 code (Makefile: machine LICM off, 1024-thread blocks) and because the two halves build in
//                    parallel.
#pragma once
#include "../../include/rttnw_hip.h"
#include "rt_core.hpp"
#include "adaptive.hpp"
#include "scene_handle.hpp"
#include "scene_narrow.hpp"
#include "device_mem.hpp"

#include <hip/hip_runtime.h>

#include <algorithm>
#include <memory>
#include <chrono>
#include <mutex>
#include <type_traits>
#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <string>
#include <vector>

namespace rt {

// A HIP call that must succeed: on failure the last error becomes "<text><hip's words>" and the function returns RTTNW_ERR_HIP.  HIP_TRY's text
// is the call as written, HIP_TRY_AS's the same behind a prefix such as "denoise: " (a string, known at run time or not).  (Both stringify
// their own argument: handed from one macro to the other it would be macro-expanded first.)
#define HIP_TRY_TEXT(text, expr)                                                           \
    do {                                                                                   \
        hipError_t e_ = (expr);                                                            \
        if (e_ != hipSuccess) {                                                            \
            ::rt::set_last_error(text + hipGetErrorString(e_));                                  \
            return RTTNW_ERR_HIP;                                                          \
        }                                                                                  \
    } while (0)
#define HIP_TRY(expr) HIP_TRY_TEXT(std::string(#expr) + ": ", expr)
#define HIP_TRY_AS(prefix, expr) HIP_TRY_TEXT(std::string(prefix) + #expr ": ", expr)

// What the image filters' device halves start with (`call`: "denoise", ...): they take host arrays, not a scene that already found its device
inline int require_device(const char* call) {
    int count = 0;
    if (hipGetDeviceCount(&count) == hipSuccess && count > 0) return 0;
    set_last_error(std::string(call) + ": no HIP device available (this library has no CPU fallback)");
    return RTTNW_ERR_HIP;
}

// A scene's arrays on one device.  A scene is uploaded whole or not at all (upload), and the decoupled kernels' records are added whole or not at
// all (ensure_quant4): every step builds into local owners, which the members take over only once all of them have succeeded.  An empty
// DeviceScene{} is a scene not yet uploaded; assigning one drops the arrays.
template <typename R> struct DeviceScene {
    bool ready = false;
    DevBuf<Bvh4Node> nodes;
    DevBuf<Bvh4QNode> nodes4q;   // the same records with quantised boxes (made on first use by the decoupled kernels, ensure_quant4)
    DevBuf<SphereRec<R>> spheres;
    DevBuf<int32_t> sphere_mat, sphere_seq;
    DevBuf<MovingSphereRec<R>> moving;
    DevBuf<RectRec<R>> rects;
    DevBuf<BoxRec<R>> boxes;
    DevBuf<InstanceRec<R>> insts;
    DevBuf<MediumRec<R>> media;
    DevBuf<int32_t> medium_refs;
    DevBuf<MaterialRec<R>> mats;
    DevBuf<TextureRec<R>> texs;
    DevBuf<ImageRec> images;
    DevBuf<uint32_t> texels;
    DevBuf<R> perlin_vec;
    DevBuf<uint8_t> perlin_perm;
    SceneView<R> view{};
    size_t bytes = 0;
    // The decoupled kernels' own view of a big cloud (round 6, ensure_quant4): node records and the sphere records of their leaves INTERLEAVED in one
    // buffer (bvh_build.hpp interleave_build_device), the spheres' sequence numbers and materials at the same, sparse, indices; the few other records'
    // material references moved behind them.  Layout only: what `view` describes, elsewhere.
    bool interleaved = false;
    SceneView<R> view_q{};
    DevBuf<int32_t> seq_q;
    DevBuf<MaterialRec<R>> mats_q;
    DevBuf<RectRec<R>> rects_q;
    DevBuf<BoxRec<R>> boxes_q;
    const SceneView<R>& decoupled_view() const { return interleaved ? view_q : view; }

    // The scene's node array on the current device: the host-built records followed by the device-built trees.  A scene whose
    // nodes are ONE device-built tree on this very device (spheres_1m: 57 MB) simply adopts the builder's buffer; otherwise the
    // pieces are put together — device-to-device for trees built here, through the host copy (materialize_host_nodes) for
    // trees built on another device.
    static int upload_nodes(const FlatScene& f, DevBuf<Bvh4Node>& nodes) {
        int dev = -1;
        HIP_TRY(hipGetDevice(&dev));
        if (f.device_trees.empty()) { HIP_TRY(nodes.upload(f.nodes4)); return 0; }
        if (f.n_host4 == 0 && f.device_trees.size() == 1 && f.device_trees[0].device == dev) {
            nodes.adopt(f.device_trees[0].nodes4, f.device_trees[0].count4);
            return 0;
        }
        HIP_TRY(nodes.alloc(f.total_nodes4()));
        if (f.n_host4) HIP_TRY(hipMemcpy(nodes.p, f.nodes4.data(), size_t(f.n_host4) * sizeof(Bvh4Node), hipMemcpyHostToDevice));
        for (const DeviceTree& t : f.device_trees) {
            if (t.device == dev) {
                HIP_TRY(hipMemcpy(nodes.p + t.base4, t.nodes4.get(), size_t(t.count4) * sizeof(Bvh4Node), hipMemcpyDeviceToDevice));
            } else {
                std::string err;
                if (int mrc = materialize_host_nodes(const_cast<FlatScene&>(f), err)) { set_last_error(err); return mrc; }
                HIP_TRY(hipMemcpy(nodes.p + t.base4, f.nodes4.data() + t.base4, size_t(t.count4) * sizeof(Bvh4Node), hipMemcpyHostToDevice));
            }
        }
        return 0;
    }

    // The decoupled kernels' node records, made on this device from the f32 ones the first time such a kernel is chosen.
    int ensure_quant4(const FlatScene& f) {
        if (nodes4q.p) return 0;
        const char* e = getenv("RTTNW_INTERLEAVE"); // (0: the separate arrays of rounds 1-5, for A/B runs and tests)
        if (f.sphere_mat_is_index && f.insts.empty() && f.moving.empty() && f.media.empty() && !(e && e[0] == '0')) return build_interleaved(f);
        return build_quant4(f);
    }
    int build_quant4(const FlatScene& f) {
        const uint32_t n = f.total_nodes4();
        DevBuf<Bvh4QNode> q;
        HIP_TRY(q.alloc(n));
        std::string err;
        if (int rc = quant4_build_device(nodes.p, n, q.p, err)) { set_last_error(err); return rc; }
        nodes4q = q;
        view.nodes4q = nodes4q.p;
        return 0;
    }

    // A big cloud (FlatScene::sphere_mat_is_index: >= 65 536 spheres, slot i holds i, no instance, medium or moving sphere): the quantised node
    // records and the spheres of their leaves in ONE buffer.  Per-record sphere counts come from the device (the tree may live only there), the
    // layout is a sequential pass on the host (a record with sphere leaves starts on a 128-byte line, any other on a 64-byte boundary), the
    // records are written by one kernel.  tests/hostsim/cache_model.hpp priced it: nodes + spheres 73.9 -> 64.7 read-miss lines per sample in
    // f32 (all four 16-byte spheres of a record share its line), 80.1 -> 73.7 in f64.
    int build_interleaved(const FlatScene& f) {
        const uint32_t n4 = f.total_nodes4();
        std::string err;
        DevBuf<uint8_t> d_cnt;
        HIP_TRY(d_cnt.alloc(n4));
        if (int rc = interleave_count_device(nodes.p, n4, d_cnt.p, err)) { set_last_error(err); return rc; }
        std::vector<uint8_t> cnt(n4);
        if (n4) HIP_TRY(hipMemcpy(cnt.data(), d_cnt.p, n4, hipMemcpyDeviceToHost));
        constexpr uint32_t su = uint32_t(sizeof(SphereRec<R>) / 16);
        std::vector<uint32_t> off(n4);
        uint64_t at = 0;
        for (uint32_t i = 0; i < n4; ++i) {
            const uint32_t align = cnt[i] ? 8u : 4u;
            at = (at + align - 1) / align * align;
            off[i] = uint32_t(at);
            at += 4u + uint32_t(cnt[i]) * su;
        }
        at = (at + 7) / 8 * 8;
        const uint64_t n_sparse = at / su;               // sphere indices of the buffer run up to here
        if (at >= (1ull << 32) || n_sparse >= (1ull << 26)) return build_quant4(f); // (beyond the leaf bits' 26-bit record index: the separate arrays)
        DevBuf<uint32_t> d_off;
        HIP_TRY(d_off.alloc(n4));
        if (n4) HIP_TRY(hipMemcpy(d_off.p, off.data(), size_t(n4) * 4, hipMemcpyHostToDevice));
        DevBuf<Bvh4QNode> buf;
        HIP_TRY(buf.alloc(size_t(at) / 4));
        HIP_TRY(hipMemset(buf.p, 0, size_t(at) * 16));
        DevBuf<int32_t> seq;
        HIP_TRY(seq.alloc(size_t(n_sparse)));
        HIP_TRY(hipMemset(seq.p, 0, size_t(n_sparse) * 4));
        const size_t nm = f.mats.size();
        DevBuf<MaterialRec<R>> mq;
        HIP_TRY(mq.alloc(size_t(n_sparse) + nm));
        HIP_TRY(hipMemset(mq.p, 0, size_t(n_sparse) * sizeof(MaterialRec<R>)));
        if (nm) HIP_TRY(hipMemcpy(mq.p + n_sparse, mats.p, nm * sizeof(MaterialRec<R>), hipMemcpyDeviceToDevice)); // the scene's materials, behind the spheres'
        static_assert(sizeof(SphereRec<R>) % 16 == 0 && sizeof(MaterialRec<R>) % 16 == 0, "interleave_scatter_kernel copies 16-byte units");
        InterleaveArgs a{};
        a.nodes4 = nodes.p; a.n4 = n4; a.noff = d_off.p; a.spheres = spheres.p; a.sphere_bytes = uint32_t(sizeof(SphereRec<R>)); a.sphere_seq = sphere_seq.p;
        a.mats = mats.p; a.mat_bytes = uint32_t(sizeof(MaterialRec<R>)); a.buffer = buf.p; a.seq_out = seq.p; a.mats_out = mq.p;
        if (int rc = interleave_build_device(a, err)) { set_last_error(err); return rc; }
        // the other kinds' records keep their places; their material references move behind the sparse block
        std::vector<RectRec<R>> rq;
        for (auto& r : f.rects) { rq.push_back(narrow<R>(r)); rq.back().mat += int32_t(n_sparse); }
        std::vector<BoxRec<R>> bq;
        for (auto& b : f.boxes) { bq.push_back(narrow<R>(b)); bq.back().mat += int32_t(n_sparse); }
        DevBuf<RectRec<R>> rects_buf;
        DevBuf<BoxRec<R>> boxes_buf;
        HIP_TRY(rects_buf.upload(rq));
        HIP_TRY(boxes_buf.upload(bq));
        // every step has succeeded: the scene takes the new arrays
        nodes4q = buf; seq_q = seq; mats_q = mq; rects_q = rects_buf; boxes_q = boxes_buf;
        view_q = view;
        view_q.nodes4q = nodes4q.p;
        view_q.spheres = reinterpret_cast<const SphereRec<R>*>(nodes4q.p);
        view_q.sphere_mat = nullptr;
        view_q.sphere_seq = seq_q.p;
        view_q.mats = mats_q.p;
        view_q.rects = rects_q.p;
        view_q.boxes = boxes_q.p;
        view_q.top_root = int32_t(off[size_t(f.top_root)] >> 2);
        view.nodes4q = nodes4q.p; // (never walked through `view`: the records' child slots are the interleaved buffer's)
        interleaved = true;
        return 0;
    }

    int upload(const FlatScene& f) {
        const NarrowScene<R> n(f); // the records in this precision (scene_narrow.hpp)
        DeviceScene s; // taken over whole once every upload has succeeded
        if (int rc = upload_nodes(f, s.nodes)) return rc;
        HIP_TRY(s.spheres.upload(n.spheres));
        if (!f.sphere_mat_is_index) HIP_TRY(s.sphere_mat.upload(f.sphere_mat));
        HIP_TRY(s.sphere_seq.upload(f.sphere_seq)); HIP_TRY(s.moving.upload(n.moving)); HIP_TRY(s.rects.upload(n.rects)); HIP_TRY(s.boxes.upload(n.boxes));
        HIP_TRY(s.insts.upload(n.insts)); HIP_TRY(s.media.upload(n.media)); HIP_TRY(s.medium_refs.upload(f.medium_refs)); HIP_TRY(s.mats.upload(n.mats));
        HIP_TRY(s.texs.upload(n.texs)); HIP_TRY(s.images.upload(f.images)); HIP_TRY(s.texels.upload(f.texels));
        HIP_TRY(s.perlin_vec.upload(n.perlin_vec)); HIP_TRY(s.perlin_perm.upload(f.perlin_perm));
        SceneView<R>& v = s.view;
        v.nodes = s.nodes.p; v.spheres = s.spheres.p; v.sphere_mat = f.sphere_mat_is_index ? nullptr : s.sphere_mat.p; v.sphere_seq = s.sphere_seq.p;
        v.moving = s.moving.p; v.rects = s.rects.p; v.boxes = s.boxes.p; v.insts = s.insts.p; v.media = s.media.p; v.medium_refs = s.medium_refs.p;
        v.mats = s.mats.p; v.texs = s.texs.p; v.images = s.images.p; v.texels = s.texels.p;
        v.perlin_vec = s.perlin_vec.p; v.perlin_perm = s.perlin_perm.p;
        v.top_root = f.top_root;
        v.n_media = int32_t(f.media.size());
        s.bytes = size_t(f.total_nodes4()) * sizeof(Bvh4Node) + n.spheres.size() * sizeof(SphereRec<R>) + n.moving.size() * sizeof(MovingSphereRec<R>) +
                  n.rects.size() * sizeof(RectRec<R>) + n.boxes.size() * sizeof(BoxRec<R>) + n.insts.size() * sizeof(InstanceRec<R>);
        s.ready = true;
        *this = s;
        return 0;
    }
};

struct DeviceState {
    int device = -1;
    int num_cus = 0;
    uint64_t chunk_budget = 0; // bytes of chunk sums a launch may hold on this device (rt_types.hpp launch_chunks): total HBM / 12, 4 .. 24 GiB
    DeviceScene<float> s32;
    DeviceScene<double> s64;
    DeviceScene<double> s64_ref; // rttnw_scene::flat_ref on this device (RTTNW_F64_STRICT renders of scenes with world-space copies)
    // workspace, grown on demand and kept (DevBuf::grow: n = bytes)
    DevBuf<uint8_t> partial;
    DevBuf<uint8_t> pool_r, pool_u; // path-slot state (reals / words), SoA over all slots
    DevBuf<uint8_t> spill;          // traversal-stack entries beyond LDS_STACK_ENTRIES, per thread of the launch
    DevBuf<unsigned long long> job_counter; // [0] job counter, then DeviceCounters
    Event ev0, ev1;
    Stream stream;                  // rttnw_render_multi: this device's launch stream
    DevBuf<uint8_t> multi_packed;   // packed tiles of the logical ranks living on this device
    DevBuf<uint8_t> gathered;       // root device: every rank's packed tiles
    // scratch for the blocking host-output render()
    DevBuf<uint8_t> packed, linear, rgba;
    // rttnw_render_adaptive: per packed pixel the noise state (adaptive.hpp) and the active bit, the maps
    DevBuf<uint8_t> ad_state, ad_active, ad_spp, ad_stderr;
    // rttnw_render_region: the caller's mask (window-sized), the selection byte per packed pixel, the running sums per list slot and the
    // window-sized outputs
    DevBuf<uint8_t> rg_mask, rg_select, rg_sums, rg_linear, rg_rgba;
    // both: the list of 2x2 blocks that hold a marked pixel and its scan (adaptive_launch.hpp build_quad_list), built anew before every use
    DevBuf<uint8_t> list_quads, list_scan;
    // rttnw_render_adaptive_multi: what lives across passes, per logical rank of this device (slotted like multi_packed) — the noise state, the
    // active bytes, each rank's list and scan (a rank's list is built behind one pass and read by its next, with other ranks' work between) —
    // and the ranks' auxiliary records (standard errors and samples, 4 doubles per packed pixel); on the root device, every rank's records
    DevBuf<uint8_t> multi_ad_state, multi_ad_active, multi_list, multi_aux, gathered_aux;
    // rttnw_render_adaptive_resume, slotted the same way: the ranks' packed state records (12 doubles per packed pixel, copied from and to the host)
    // and the marks of the level being listed (a byte per packed pixel)
    DevBuf<uint8_t> multi_ad_records, multi_ad_marks;
    // rttnw_render_adaptive_region: the ranks' selection bytes (a byte per packed pixel, slotted like the active bytes; the mask is rg_mask, once per
    // device) and, on the root, the window-sized samples and standard-error maps beside rg_linear / rg_rgba
    DevBuf<uint8_t> multi_ad_select, rg_spp, rg_stderr;
};
// Words of build_quad_list's scan workspace over n_blocks blocks, and where its two totals (listed blocks, marked pixels) stand in it
inline size_t quad_scan_words(uint32_t n_blocks) { return size_t((n_blocks + 63u) / 64u) * 3 + 2; }
inline uint32_t* quad_list_totals(uint32_t* scan, uint32_t n_blocks) { return scan + size_t((n_blocks + 63u) / 64u) * 3; }
// What render_tiles_t needs to run a pass that is not a plain render's (render_tiles.hpp): a resolve step of the pass's own in place of
// resolve_kernel and, with `quads`, the active-list instantiation of the scene's kernel over that list of 2x2 blocks.
//   state != nullptr  a pass of rttnw_render_adaptive (render_adaptive_t): adaptive_resolve_kernel, which keeps the noise state
//   state == nullptr  rttnw_render_region (render_region_t): region_resolve_kernel; d_packed holds the running sums BY LIST SLOT
struct ListPass {
    const uint32_t* quads = nullptr; // nullptr: pass 0 of an adaptive render, every pixel of the rank in the render's own job numbering
    uint32_t n_quads = 0;
    bool first = true;               // pass 0: the running sums and the noise state start here
    bool clock_started = false;      // the caller recorded d->ev0 itself, before it built the list
    AdaptivePixel* state = nullptr;
    uint8_t* active = nullptr;
    uint32_t cap = 0;
    double rel_error = 0, abs_error = 0;
};
void debug_print_sched(const DeviceCounters& hc, bool plain, uint32_t profile, uint64_t samples); // RTTNW_DEBUG_SCHED=1 only (debug_sched.cpp)
int device_state_create(DeviceState*& out, std::string& err);
// The lowering an RTTNW_F64_STRICT render walks: s->flat, or — when that holds world-space copies of transformed groups' spheres — the same
// graph lowered without them (made once, under the scene's mutex).  render_api.cpp.
int reference_frame_scene(::rttnw_scene* s, const FlatScene*& flat);

void fill_layout(uint32_t w, uint32_t h, uint32_t world, rttnw_tile_layout& L);
int validate(::rttnw_scene* s, const rttnw_camera_desc* cam, const rttnw_params* p);
// What the host-output entry points beyond rttnw_render refuse among their own arguments, before validate() (`reserved0`: the call's own reserved
// field; `counters_why`: appended to the collect_counters refusal).
inline int refuse_host_output_misuse(const char* prefix, uint32_t reserved0, const rttnw_params* p, const char* counters_why = "") {
    const std::string call = std::string(prefix) + ": ";
    if (reserved0 != 0) { set_last_error(call + "reserved0 must be 0"); return RTTNW_ERR_INVALID; }
    if (p->tile_world != 1) { set_last_error(call + "host-output form needs tile_world == 1"); return RTTNW_ERR_INVALID; }
    if (p->collect_counters != 0) { set_last_error(call + "collect_counters is not supported" + counters_why); return RTTNW_ERR_UNSUPPORTED; }
    return 0;
}

// The launch code of one precision (render_tiles.hpp, adaptive_launch.hpp), instantiated in render_f32.hip / render_f64.hip — and, for double, a second
// time in render_f64_strict.hip in the namespace rt::ieee_strict (rt_core.hpp: the two builds of the f64 arithmetic).
inline namespace RT_ARITH_NS {
// What every entry point that launches over a scene starts with: the device made current, the lowering this build walks and its arrays on the
// device, uploaded on first use.
template <typename R> int bind_scene(::rttnw_scene* s, DeviceState* d, const FlatScene*& flat, DeviceScene<R>*& ds) {
    HIP_TRY(hipSetDevice(d->device));
    flat = &s->flat;
    if constexpr (sizeof(R) == 4) ds = &d->s32; else ds = &d->s64;
#if defined(RT_STRICT_F64)
    // the IEEE-strict build walks the lowering that tests every object in the reference's frame (render_api.cpp reference_frame_scene)
    if (int rc = reference_frame_scene(s, flat)) return rc;
    if (flat != &s->flat) ds = &d->s64_ref;
#endif
    return ds->ready ? 0 : ds->upload(*flat);
}
// The constants of a render of `p` over tile layout L (fill_layout); the chunk schedule, the jobs and the LDS staging follow where they are planned.
// (probe_path_t sets sample_begin and scene_flags back to 0: a field added here that path_begin reads needs a look there)
inline RenderConsts base_consts(const rttnw_params* p, const FlatScene& flat, const rttnw_tile_layout& L) {
    RenderConsts rc{};
    rc.width = p->width; rc.height = p->height; rc.spp = p->spp; rc.max_depth = p->max_depth;
    rc.tiles_x = L.tiles_x; rc.tiles_y = L.tiles_y; rc.n_tiles = L.n_tiles;
    rc.tile_rank = p->tile_rank; rc.tile_world = p->tile_world;
    rc.my_tiles = L.n_tiles > p->tile_rank ? (L.n_tiles - p->tile_rank + p->tile_world - 1) / p->tile_world : 0;
    rc.quirks = p->quirks; rc.seed = p->seed; rc.stack_depth = flat.stack_depth;
    rc.profile = p->collect_counters;
    rc.sample_begin = p->sample_begin;
    rc.scene_flags = flat.moving.empty() ? SCENE_NO_TIME : 0u;
    rc.inv_width = 1.0 / double(p->width); rc.inv_height = 1.0 / double(p->height);
    rc.div_tiles_x = make_fastdiv(std::max<uint32_t>(1u, rc.tiles_x));
    return rc;
}
} // namespace RT_ARITH_NS

// The per-precision entry points of render_tiles.hpp and adaptive_launch.hpp, ONE list: X(R, name, parameters).  It makes the declarations, the
// `extern template` lines of both builds and what a precision's translation unit instantiates (RT_INSTANTIATE_PRECISION): a new entry point is one
// line here.  (What computes nothing in R is no entry point of a precision: pixel_lists.hpp.)
//   render_adaptive_t  rttnw_render_adaptive's device half: every pass, then the image (d->linear, d->rgba) and the maps (d->ad_spp, d->ad_stderr) on the device
//   render_region_t    rttnw_render_region's device half: selection, list, trace, resolve; the window's image on the device (d->rg_linear, d->rg_rgba)
//   adaptive_finish_launch   what rttnw_render_adaptive_multi (render_adaptive_api.cpp) enqueues behind render_tiles_t's passes
//   adaptive_state_import_launch, adaptive_state_export_launch, adaptive_rank_stats_t   what rttnw_render_adaptive_resume adds to it
//   adaptive_region_window_launch   ... and rttnw_render_adaptive_region to those: the window's outputs
#define RT_PRECISION_ENTRY_POINTS(X, R)                                                                                                              \
    X(R, render_tiles_t, (::rttnw_scene* s, DeviceState* d, const rttnw_camera_desc* cam, const rttnw_params* p, void* d_packed, hipStream_t stream, \
                          rttnw_stats* stats, bool sync_for_stats, bool prepare_only, const ListPass* ad))                                          \
    X(R, probe_path_t, (::rttnw_scene* s, const rttnw_camera_desc* cam, const rttnw_params* p, uint32_t px, uint32_t row, uint32_t sample,           \
                        double* out, uint32_t max_out))                                                                                              \
    X(R, untile_launch, (uint32_t width, uint32_t height, uint32_t world, const void* d_gathered, void* d_linear_rgb, uint8_t* d_rgba8,              \
                         hipStream_t stream))                                                                                                        \
    X(R, render_adaptive_t, (::rttnw_scene* s, const rttnw_camera_desc* cam, const rttnw_params* p, const rttnw_adaptive* a, rttnw_stats* stats))    \
    X(R, render_region_t, (::rttnw_scene* s, const rttnw_camera_desc* cam, const rttnw_params* p, uint32_t x0, uint32_t y0, uint32_t x1,             \
                           uint32_t y1, const uint8_t* mask, rttnw_stats* stats))                                                                    \
    X(R, adaptive_finish_launch, (void* d_packed, const void* d_state, double* d_aux, uint32_t pixels_per_rank, uint32_t rank_pixels,                \
                                  hipStream_t stream))                                                                                               \
    X(R, adaptive_state_import_launch, (const double* d_records, void* d_packed, void* d_state, uint8_t* d_active, uint32_t pixels_per_rank,         \
                                        uint32_t cap, double rel_error, double abs_error, hipStream_t stream))                                       \
    X(R, adaptive_state_export_launch, (const void* d_packed, const void* d_state, double* d_records, uint32_t pixels_per_rank,                      \
                                        uint32_t rank_pixels, hipStream_t stream))                                                                   \
    X(R, adaptive_rank_stats_t, (::rttnw_scene* s, DeviceState* d, const rttnw_params* p, rttnw_stats* stats))                                      \
    X(R, adaptive_region_window_launch, (uint32_t width, uint32_t height, uint32_t world, const void* d_gathered, const double* d_gathered_aux,     \
                                         void* d_linear_rgb, uint8_t* d_rgba8, uint32_t* d_spp, double* d_stderr, uint32_t x0, uint32_t y0,         \
                                         uint32_t x1, uint32_t y1, hipStream_t stream))
#define RT_DECLARE_T(R, name, params) template <typename> int name params;
#define RT_EXTERN_T(R, name, params) extern template int name<R> params;
#define RT_INSTANTIATE_T(R, name, params) template int name<R> params;
#define RT_INSTANTIATE_PRECISION(R) RT_PRECISION_ENTRY_POINTS(RT_INSTANTIATE_T, R)
// ... declared in this unit's build for float and double, and (for the host code) in the IEEE-strict build for double (render_f64_strict.hip)
#define RT_DECLARE_BUILDS(LIST)                                                                              \
    inline namespace RT_ARITH_NS { LIST(RT_DECLARE_T, ) LIST(RT_EXTERN_T, float) LIST(RT_EXTERN_T, double) } \
    RT_DECLARE_STRICT_BUILD(LIST)
#if !defined(RT_STRICT_F64)
#define RT_DECLARE_STRICT_BUILD(LIST) namespace ieee_strict { LIST(RT_DECLARE_T, ) LIST(RT_EXTERN_T, double) }
#else
#define RT_DECLARE_STRICT_BUILD(LIST)
#endif
RT_DECLARE_BUILDS(RT_PRECISION_ENTRY_POINTS)

// One precision's launch code, by rttnw_params::precision (RTTNW_F64_STRICT: the ieee_strict build of the f64 arithmetic, rt_core.hpp).
#define RT_BY_PRECISION(precision, fn, ...)                                       \
    ((precision) == RTTNW_F32          ? rt::fn<float>(__VA_ARGS__)               \
     : (precision) == RTTNW_F64_STRICT ? rt::ieee_strict::fn<double>(__VA_ARGS__) \
                                       : rt::fn<double>(__VA_ARGS__))

} // namespace rt
