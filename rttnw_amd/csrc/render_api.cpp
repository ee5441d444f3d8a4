// render_api.cpp — the extern "C" half of the device side of include/rttnw_hip.h: device state, render entry points,
// rttnw_render_multi and rttnw_render_adaptive_multi (per-device streams, RCCL gather), rttnw_render_adaptive_denoised (the rounds that alternate the
// adaptive passes with the denoiser's), rttnw_render_adaptive_budget (the rounds that alternate a selection with the passes it chose).  Host code only; the kernels and their launch code live in render_f32.hip / render_f64.hip (render_common.hpp
// says why there are two), denoise.hip, guided.hip and budget.hip.
// No CPU fallback: every entry point needs a HIP device.
#include "render_common.hpp"
#include "bvh_build.hpp"
#include "feature_api.hpp"
#include "guided.hpp"
#include "budget.hpp"

#include <rccl/rccl.h>
#include <dlfcn.h>
#include <mutex>

namespace rt {

// A plain render's launch code in the precision of `p`
static int render_tiles_any(::rttnw_scene* s, DeviceState* d, const rttnw_camera_desc* cam, const rttnw_params* p, void* d_packed, hipStream_t stream,
                            rttnw_stats* stats, bool sync_for_stats = true, bool prepare_only = false, const ListPass* ad = nullptr) {
    return RT_BY_PRECISION(p->precision, render_tiles_t, s, d, cam, p, d_packed, stream, stats, sync_for_stats, prepare_only, ad);
}
// What rttnw_render_adaptive and rttnw_render_adaptive_multi refuse among the adaptive arguments themselves (both non-NULL): no device needed
static int refuse_adaptive_misuse(const char* prefix, const rttnw_params* p, const rttnw_adaptive* a) {
    const std::string call = std::string(prefix) + ": ";
    if (a->pass_spp == 0) { set_last_error(call + "pass_spp is 0"); return RTTNW_ERR_INVALID; }
    if (p->spp == 0 || p->spp % a->pass_spp != 0) { set_last_error(call + "spp (the cap) must be a positive multiple of pass_spp"); return RTTNW_ERR_INVALID; }
    if (!(a->rel_error >= 0.0) || !(a->abs_error >= 0.0)) { set_last_error(call + "rel_error and abs_error must be >= 0 (and not NaN)"); return RTTNW_ERR_INVALID; }
    return 0;
}

// The linear image of a blocking render (`linear`: d->linear or d->rg_linear, in the render's precision) to the caller's doubles: an f32 image is
// widened through a temporary.
static hipError_t copy_linear_out(const DevBuf<uint8_t>& linear, uint32_t precision, size_t npx, double* out) {
    if (precision != RTTNW_F32) return hipMemcpy(out, linear.p, npx * 3 * sizeof(double), hipMemcpyDeviceToHost);
    std::vector<float> tmp(npx * 3);
    const hipError_t e = hipMemcpy(tmp.data(), linear.p, npx * 3 * sizeof(float), hipMemcpyDeviceToHost);
    for (size_t i = 0; i < npx * 3; ++i) out[i] = double(tmp[i]);
    return e;
}
// What every host-output entry point ends with: the npx pixels of the image on the device to the caller's arrays (each optional), and a HIP error —
// `e`: of the call's own steps before this one — as RTTNW_ERR_HIP under the call's name.
static int copy_image_out(const char* what, const DevBuf<uint8_t>& rgba, const DevBuf<uint8_t>& linear, uint32_t precision, size_t npx, uint8_t* out_rgba8,
                          double* out_linear, hipError_t e = hipSuccess) {
    if (e == hipSuccess && out_rgba8) e = hipMemcpy(out_rgba8, rgba.p, npx * 4, hipMemcpyDeviceToHost);
    if (e == hipSuccess && out_linear) e = copy_linear_out(linear, precision, npx, out_linear);
    if (e != hipSuccess) { set_last_error(std::string(what) + ": " + hipGetErrorString(e)); return RTTNW_ERR_HIP; }
    return RTTNW_OK;
}

void device_release(DeviceState* d) {
    if (!d) return;
    DeviceGuard restore;
    if (d->device >= 0) (void)hipSetDevice(d->device);
    delete d;
}

int device_bvh_builder(::rttnw_scene* s, DeviceBvhApi& out, std::string& err) {
    int count = 0;
    if (hipGetDeviceCount(&count) != hipSuccess || count <= 0) {
        err = "no HIP device available (the device BVH builder has no CPU fallback)";
        return RTTNW_ERR_HIP;
    }
    out.build = [s](const BuildPrim* prims, size_t n, const float* centroid_bounds, DeviceTree& tree, std::string& e) {
        return lbvh_build_device_tree(prims, n, centroid_bounds, s->bvh_builder != RTTNW_BVH_DEVICE_LBVH, tree, &s->build_kernel_ms, e);
    };
    out.rebase = [](DeviceTree& tree, uint32_t base4, uint32_t base2, std::string& e) { return device_tree_rebase(tree, base4, base2, e); };
    out.min_leaves = s->bvh_builder == RTTNW_BVH_AUTO ? RTTNW_BVH_AUTO_DEVICE_LEAVES : 2u;
    return 0;
}

int materialize_host_nodes(FlatScene& f, std::string& err) {
    if (f.device_trees.empty() || f.nodes4.size() == f.total_nodes4()) return 0;
    f.nodes4.resize(f.total_nodes4());
    f.nodes.resize(f.total_nodes2());
    for (const DeviceTree& t : f.device_trees)
        if (device_tree_download(t, f.nodes4.data() + t.base4, f.nodes.data() + t.base2, err)) {
            f.nodes4.resize(f.n_host4);
            f.nodes.resize(f.n_host2);
            return RTTNW_ERR_HIP;
        }
    return 0;
}

// State on the CURRENT device (job counter, events; the scene arrays follow on first use).
int device_state_create(DeviceState*& out, std::string& err) {
    DeviceState* d = new DeviceState();
    hipError_t e = hipGetDevice(&d->device);
    hipDeviceProp_t prop;
    if (e == hipSuccess) e = hipGetDeviceProperties(&prop, d->device);
    if (e != hipSuccess) { err = std::string("hipGetDeviceProperties: ") + hipGetErrorString(e); device_release(d); return RTTNW_ERR_HIP; }
    d->num_cus = prop.multiProcessorCount;
    d->chunk_budget = std::min<uint64_t>(24ull << 30, std::max<uint64_t>(4ull << 30, uint64_t(prop.totalGlobalMem) / 12));
    e = d->job_counter.alloc(1 + sizeof(DeviceCounters) / sizeof(unsigned long long));
    if (e == hipSuccess) e = create_event(d->ev0);
    if (e == hipSuccess) e = create_event(d->ev1);
    if (e != hipSuccess) { err = std::string("device state: ") + hipGetErrorString(e); device_release(d); return RTTNW_ERR_HIP; }
    out = d;
    return 0;
}

int device_commit(::rttnw_scene* s, std::string& err) {
    int count = 0;
    if (hipGetDeviceCount(&count) != hipSuccess || count <= 0) {
        err = "no HIP device available (this library has no CPU fallback)";
        return RTTNW_ERR_HIP;
    }
    if (s->device) { device_release(s->device); s->device = nullptr; } // a commit that failed half-way and is retried
    // The scene arrays are uploaded per precision on first use (render), see bind_scene.
    return device_state_create(s->device, err);
}


// RTTNW_F64_STRICT promises the reference's operations in the reference's order.  The default lowering breaks that promise in one place: a
// sphere under Translate / YRotate wrappers is tested as a world-space copy in the top tree (scene_lower.cpp: the same quadratic written in
// another frame — t differs in the last place, which a few bounces off small spheres amplify: final_scene 800x800 spp 1000, 9 of 1536 pixels of
// the cluster crop beyond 1e-9).  So the strict build walks a second lowering of the same graph that leaves those spheres in their groups'
// trees (the ray goes through the wrappers as in hittable.rs:599-606,686-699): on that crop every pixel is within 1.5e-13 of the CPU
// restatement, at 7 % of the strict build's speed on that scene (more node steps, a second tree).  Made at the first strict render of a scene
// that has such copies, with the scene's own builder and shutter interval; scenes without them render `flat` itself.
int reference_frame_scene(::rttnw_scene* s, const FlatScene*& flat) {
    flat = &s->flat;
    if (s->flat.n_world_copies == 0) return 0;
    std::lock_guard<std::mutex> lock(s->rebuild_mutex);
    if (!s->flat_ref) {
        std::string err;
        DeviceBvhApi device_builder;
        bool on_device = s->bvh_builder != RTTNW_BVH_HOST_SAH;
        if (on_device)
            if (int brc = device_bvh_builder(s, device_builder, err)) {
                // (as rttnw_scene_commit, capi_builder.cpp: RTTNW_BVH_AUTO falls back to the host builder; an explicitly requested device builder fails)
                if (s->bvh_builder != RTTNW_BVH_AUTO) { set_last_error(err); return brc; }
                on_device = false;
            }
        std::unique_ptr<FlatScene> ref(new FlatScene());
        // RTTNW_STRICT_GROUP_TREES=1 (experiments / tests): the round-4 form — the copies stay in their groups' trees and the walk enters them
        const char* gt = getenv("RTTNW_STRICT_GROUP_TREES");
        const int ref_mode = gt && gt[0] == '1' ? 0 : 2;
        if (int rc = lower_scene(s->graph, *ref, err, on_device ? &device_builder : nullptr, s->flat.time0, s->flat.time1, ref_mode)) { set_last_error(err); return rc; }
        s->flat_ref = std::move(ref);
    }
    flat = s->flat_ref.get();
    return 0;
}

void fill_layout(uint32_t w, uint32_t h, uint32_t world, rttnw_tile_layout& L) {
    L.tiles_x = (w + 7) / 8; L.tiles_y = (h + 7) / 8;
    L.n_tiles = L.tiles_x * L.tiles_y;
    L.tiles_per_rank = (L.n_tiles + world - 1) / world;
    L.pixels_per_rank = L.tiles_per_rank * 64;
}

int validate(::rttnw_scene* s, const rttnw_camera_desc* cam, const rttnw_params* p) {
    if (!s || !cam || !p) { set_last_error("render: NULL argument"); return RTTNW_ERR_INVALID; }
    if (!s->committed || !s->device) { set_last_error("render: scene is not committed"); return RTTNW_ERR_STATE; }
    if (!p->width || !p->height || !p->spp || !p->max_depth) { set_last_error("render: empty image, spp or depth"); return RTTNW_ERR_INVALID; }
    if (p->precision != RTTNW_F32 && p->precision != RTTNW_F64 && p->precision != RTTNW_F64_STRICT) { set_last_error("render: bad precision"); return RTTNW_ERR_INVALID; }
    // (the f32 lane-owns-path kernel's folded slab test, rt_core.hpp SLAB_FMA_FOLDED, is conservative for t_min >= 0 only; a
    // negative or NaN t_min has no meaning in main.rs:33 either)
    if (!(p->t_min >= 0.0) || !(p->t_min < 1e300)) { set_last_error("render: t_min must be finite and >= 0"); return RTTNW_ERR_INVALID; }
    if (p->tile_world == 0 || p->tile_rank >= p->tile_world) { set_last_error("render: bad tile_rank / tile_world"); return RTTNW_ERR_INVALID; }
    // the decoupled kernel packs a pixel as px | row << 16, and the free-flight draw of medium m uses RNG slot m < 16
    if (p->width > 65535u || p->height > 65535u) { set_last_error("render: width and height are limited to 65535"); return RTTNW_ERR_UNSUPPORTED; }
    if (s->flat.media.size() > SLOT_DIELECTRIC) { set_last_error("render: more than 16 constant media"); return RTTNW_ERR_UNSUPPORTED; }
    if (!(cam->open_time <= cam->close_time)) { set_last_error("render: open_time > close_time"); return RTTNW_ERR_INVALID; }
    // The boxes of moving spheres are built for the shutter interval [0, 1] (what BvhTree::from uses, hittable.rs:256).  A
    // camera whose shutter reaches outside it (BvhTree::from_time, hittable.rs:261) makes the library rebuild the trees
    // for the wider interval, once, and drop the device copies (they are uploaded again on use).  This is the ONE change a
    // committed scene can undergo (include/rttnw_hip.h says so): it happens under the scene's mutex, before anything of this
    // call is enqueued, and rttnw_scene_build_info reports the rebuilt trees afterwards.  "One render in flight per scene"
    // (the header's rule) is what keeps a concurrent render from seeing the swap.
    {
        std::lock_guard<std::mutex> lock(s->rebuild_mutex);
        if (!s->flat.moving.empty() && (cam->open_time < s->flat.time0 || cam->close_time > s->flat.time1)) {
            const double t0 = std::min(s->flat.time0, cam->open_time), t1 = std::max(s->flat.time1, cam->close_time);
            std::string err;
            DeviceBvhApi device_builder;
            const bool on_device = s->bvh_builder != RTTNW_BVH_HOST_SAH;
            if (on_device)
                if (int brc = device_bvh_builder(s, device_builder, err)) { set_last_error(err); return brc; }
            FlatScene wider;
            const auto tb = std::chrono::steady_clock::now();
            s->build_kernel_ms = 0;
            if (int rc = lower_scene(s->graph, wider, err, on_device ? &device_builder : nullptr, t0, t1)) { set_last_error(err); return rc; }
            s->lower_ms = std::chrono::duration<double, std::milli>(std::chrono::steady_clock::now() - tb).count();
            std::vector<DeviceState*> all = s->more_devices;
            all.push_back(s->device);
            {
                DeviceGuard restore;
                for (DeviceState* d : all) { // nothing of an earlier render may still read the arrays that are about to go
                    (void)hipSetDevice(d->device);
                    (void)hipDeviceSynchronize();
                    d->s32 = {}; d->s64 = {}; d->s64_ref = {};
                }
            }
            s->flat = std::move(wider);
            s->flat_ref.reset(); // (made again, for the wider interval, by the next RTTNW_F64_STRICT render)
        }
    }
    return 0;
}

} // namespace rt

// =============================================================================================
extern "C" {

int rttnw_debug_probe_path(rttnw_scene* s, const rttnw_camera_desc* cam, const rttnw_params* p, uint32_t px, uint32_t row,
                           uint32_t sample, double* out, uint32_t max_out) {
    if (int rc = rt::validate(s, cam, p)) return rc;
    if (!out || px >= p->width || row >= p->height) { rt::set_last_error("debug_probe_path: bad arguments"); return RTTNW_ERR_INVALID; }
    return RT_BY_PRECISION(p->precision, probe_path_t, s, cam, p, px, row, sample, out, max_out);
}


int rttnw_device_count(void) {
    int n = 0;
    if (hipGetDeviceCount(&n) != hipSuccess) return 0;
    return n;
}

int rttnw_tile_layout_get(uint32_t width, uint32_t height, uint32_t world, rttnw_tile_layout* out) {
    if (!out || !width || !height || !world) { rt::set_last_error("tile_layout_get: bad arguments"); return RTTNW_ERR_INVALID; }
    rt::fill_layout(width, height, world, *out);
    return RTTNW_OK;
}

int rttnw_scene_info(rttnw_scene* s, rttnw_stats* out) {
    if (!s || !out || !s->committed) { rt::set_last_error("scene_info: scene not committed"); return RTTNW_ERR_STATE; }
    std::memset(out, 0, sizeof(*out));
    out->n_nodes = s->flat.total_nodes4();
    out->n_prims = s->flat.n_prims_in_bvh;
    const auto& f = s->flat;
    size_t b32 = size_t(f.total_nodes4()) * sizeof(rt::Bvh4Node) + f.spheres.size() * sizeof(rt::SphereRec<float>) +
                 f.moving.size() * sizeof(rt::MovingSphereRec<float>) + f.rects.size() * sizeof(rt::RectRec<float>) +
                 f.boxes.size() * sizeof(rt::BoxRec<float>) + f.insts.size() * sizeof(rt::InstanceRec<float>);
    out->scene_bytes = uint32_t(std::min<size_t>(b32, 0xFFFFFFFFu));
    out->reserved = f.stack_depth;
    return RTTNW_OK;
}

int rttnw_render_tiles_device(rttnw_scene* s, const rttnw_camera_desc* cam, const rttnw_params* p, void* d_packed, void* hip_stream,
                              rttnw_stats* stats) {
    if (int rc = rt::validate(s, cam, p)) return rc;
    if (!d_packed) { rt::set_last_error("render_tiles_device: d_packed is NULL"); return RTTNW_ERR_INVALID; }
    hipStream_t stream = (hipStream_t)hip_stream;
    return rt::render_tiles_any(s, s->device, cam, p, d_packed, stream, stats);
}

int rttnw_untile_device(uint32_t width, uint32_t height, uint32_t world, uint32_t precision, const void* d_gathered,
                        void* d_linear_rgb, uint8_t* d_rgba8, void* hip_stream) {
    if (!width || !height || !world || !d_gathered || (precision != RTTNW_F32 && precision != RTTNW_F64 && precision != RTTNW_F64_STRICT)) {
        rt::set_last_error("untile_device: bad arguments");
        return RTTNW_ERR_INVALID;
    }
    hipStream_t stream = (hipStream_t)hip_stream;
    return precision == RTTNW_F32 ? rt::untile_launch<float>(width, height, world, d_gathered, d_linear_rgb, d_rgba8, stream)
                                  : rt::untile_launch<double>(width, height, world, d_gathered, d_linear_rgb, d_rgba8, stream);
}

int rttnw_render(rttnw_scene* s, const rttnw_camera_desc* cam, const rttnw_params* p, double* out_linear_rgb, uint8_t* out_rgba8,
                 rttnw_stats* stats) {
    if (int rc = rt::validate(s, cam, p)) return rc;
    if (p->tile_world != 1) { rt::set_last_error("render: host-output form needs tile_world == 1"); return RTTNW_ERR_INVALID; }
    rt::DeviceState* d = s->device;
    rttnw_tile_layout L;
    rt::fill_layout(p->width, p->height, 1, L);
    const size_t rsz = p->precision == RTTNW_F32 ? sizeof(float) : sizeof(double);
    const size_t npx = size_t(p->width) * p->height;
    hipError_t e = d->packed.grow(size_t(L.pixels_per_rank) * 4 * rsz);
    if (e == hipSuccess) e = d->linear.grow(npx * 3 * rsz);
    if (e == hipSuccess) e = d->rgba.grow(npx * 4);
    if (e != hipSuccess) { rt::set_last_error(std::string("render: ") + hipGetErrorString(e)); return RTTNW_ERR_HIP; }
    if (int rc = rttnw_render_tiles_device(s, cam, p, d->packed.p, nullptr, stats)) return rc;
    if (int rc = rttnw_untile_device(p->width, p->height, 1, p->precision, d->packed.p, d->linear.p, d->rgba.p, nullptr)) return rc;
    return rt::copy_image_out("render", d->rgba, d->linear, p->precision, npx, out_rgba8, out_linear_rgb, hipDeviceSynchronize());
}

int rttnw_render_adaptive(rttnw_scene* s, const rttnw_camera_desc* cam, const rttnw_params* p, const rttnw_adaptive* a, double* out_linear_rgb,
                          uint8_t* out_rgba8, uint32_t* out_spp, double* out_stderr_rgb, rttnw_stats* stats) {
    // the adaptive arguments first: their refusals need no device (nor a committed scene)
    if (!p || !a) { rt::set_last_error("render_adaptive: NULL argument"); return RTTNW_ERR_INVALID; }
    if (int rc = rt::refuse_adaptive_misuse("render_adaptive", p, a)) return rc;
    if (int rc = rt::refuse_host_output_misuse("render_adaptive", a->reserved0, p)) return rc;
    if (int rc = rt::validate(s, cam, p)) return rc;
    rt::DeviceState* d = s->device;
    if (int rc = RT_BY_PRECISION(p->precision, render_adaptive_t, s, cam, p, a, stats)) return rc;
    const size_t npx = size_t(p->width) * p->height;
    hipError_t e = hipSuccess;
    if (out_spp) e = hipMemcpy(out_spp, d->ad_spp.p, npx * sizeof(uint32_t), hipMemcpyDeviceToHost);
    if (e == hipSuccess && out_stderr_rgb) e = hipMemcpy(out_stderr_rgb, d->ad_stderr.p, npx * 3 * sizeof(double), hipMemcpyDeviceToHost);
    return rt::copy_image_out("render_adaptive", d->rgba, d->linear, p->precision, npx, out_rgba8, out_linear_rgb, e);
}

int rttnw_render_region(rttnw_scene* s, const rttnw_camera_desc* cam, const rttnw_params* p, uint32_t x0, uint32_t y0, uint32_t x1, uint32_t y1,
                        const uint8_t* mask, double* out_linear_rgb, uint8_t* out_rgba8, rttnw_stats* stats) {
    // the region's own arguments first, in the header's order: their refusals need no device (nor a committed scene)
    if (!p) { rt::set_last_error("render_region: NULL argument"); return RTTNW_ERR_INVALID; }
    if (x0 >= x1 || y0 >= y1 || x1 > p->width || y1 > p->height) {
        rt::set_last_error("render_region: the window [x0, x1) x [y0, y1) must be non-empty and lie inside the width x height frame");
        return RTTNW_ERR_INVALID;
    }
    if (int rc = rt::refuse_host_output_misuse("render_region", p->reserved0, p, " (the active-list kernels do not tally)")) return rc;
    if (int rc = rt::validate(s, cam, p)) return rc;
    if (int rc = RT_BY_PRECISION(p->precision, render_region_t, s, cam, p, x0, y0, x1, y1, mask, stats)) return rc;
    const rt::DeviceState* d = s->device;
    return rt::copy_image_out("render_region", d->rg_rgba, d->rg_linear, p->precision, size_t(x1 - x0) * (y1 - y0), out_rgba8, out_linear_rgb);
}

} // extern "C"

// ---------------------------------------------------------------------------------------------
// rttnw_render_multi: the whole of main.rs:202-229 on the GPUs of one node, in one call.
// ---------------------------------------------------------------------------------------------
namespace rt {
// RCCL, bound at first use (a single device, or logical ranks that share one device, never touch it).
struct Rccl {
    void* lib = nullptr;
    ncclResult_t (*CommInitAll)(ncclComm_t*, int, const int*) = nullptr;
    ncclResult_t (*CommDestroy)(ncclComm_t) = nullptr;
    ncclResult_t (*GroupStart)() = nullptr;
    ncclResult_t (*GroupEnd)() = nullptr;
    ncclResult_t (*Send)(const void*, size_t, ncclDataType_t, int, ncclComm_t, hipStream_t) = nullptr;
    ncclResult_t (*Recv)(void*, size_t, ncclDataType_t, int, ncclComm_t, hipStream_t) = nullptr;
    const char* (*GetErrorString)(ncclResult_t) = nullptr;
    bool load(std::string& err) {
        if (lib) return true;
        lib = dlopen("librccl.so.1", RTLD_NOW | RTLD_GLOBAL);
        if (!lib) lib = dlopen("librccl.so", RTLD_NOW | RTLD_GLOBAL);
        if (!lib) { err = std::string("cannot load RCCL: ") + dlerror(); return false; }
        CommInitAll = (decltype(CommInitAll))dlsym(lib, "ncclCommInitAll");
        CommDestroy = (decltype(CommDestroy))dlsym(lib, "ncclCommDestroy");
        GroupStart = (decltype(GroupStart))dlsym(lib, "ncclGroupStart");
        GroupEnd = (decltype(GroupEnd))dlsym(lib, "ncclGroupEnd");
        Send = (decltype(Send))dlsym(lib, "ncclSend");
        Recv = (decltype(Recv))dlsym(lib, "ncclRecv");
        GetErrorString = (decltype(GetErrorString))dlsym(lib, "ncclGetErrorString");
        if (!CommInitAll || !CommDestroy || !GroupStart || !GroupEnd || !Send || !Recv || !GetErrorString) { err = "RCCL lacks an expected entry point"; return false; }
        return true;
    }
};
static Rccl g_rccl;
struct MultiComms { // one communicator set per distinct list of devices, kept until rttnw_shutdown() / process exit
    std::vector<int> devices;
    std::vector<ncclComm_t> comms; // (empty: the set-up over these devices failed, comms_over)
    std::mutex in_use; // RCCL allows ONE thread at a time to issue operations on a communicator: held from GroupStart to GroupEnd
};
static std::vector<MultiComms*> g_comms;
static std::mutex g_comms_mutex; // the list itself (rttnw_render_multi may be called from several host threads, each with its own scene)
static bool g_comms_atexit = false;

// Destroy the cached communicator sets (rttnw_shutdown; registered with atexit at the first set-up, so that a process that
// never calls it still leaves RCCL in order — before the HIP runtime's own teardown, which atexit runs later: LIFO).
static void destroy_comms() {
    std::lock_guard<std::mutex> lock(g_comms_mutex);
    // (at exit, under a host that tears its own HIP context down first — Python with torch —, the runtime may already be finalising: then
    // only the host structures are released; RCCL's own teardown has nothing left to talk to)
    int n_dev = 0;
    const bool runtime_alive = hipGetDeviceCount(&n_dev) == hipSuccess && n_dev > 0;
    for (MultiComms* c : g_comms) {
        std::lock_guard<std::mutex> use(c->in_use);
        for (ncclComm_t comm : c->comms)
            if (comm && g_rccl.CommDestroy && runtime_alive) (void)g_rccl.CommDestroy(comm);
        c->comms.clear();
    }
    for (MultiComms* c : g_comms) delete c;
    g_comms.clear();
}

static DeviceState* state_on(::rttnw_scene* s, int device, std::string& err) {
    if (s->device && s->device->device == device) return s->device;
    for (DeviceState* d : s->more_devices)
        if (d->device == device) return d;
    if (hipSetDevice(device) != hipSuccess) { err = "hipSetDevice failed"; return nullptr; }
    DeviceState* d = nullptr;
    if (device_state_create(d, err)) return nullptr;
    s->more_devices.push_back(d);
    return d;
}

// The environment of a call, read once (a MultiPlan holds it).  The gather to the root is a device-to-device copy for ranks on the root's device; for the others one of
// TWO transports over xGMI (RTTNW_MULTI_GATHER=rccl|peer, default rccl):
//   rccl  a grouped ncclSend / ncclRecv per rank buffer (north_star's "RCCL gather over xGMI"; communicators cached per device list);
//   peer  hipMemcpyPeerAsync of each rank's packed tiles into the root's gather buffer on the RANK's stream, an event behind it that the
//         root's stream waits for — 5 MB per rank, no library, no communicator.  Also what the call FALLS THROUGH to when RCCL cannot be
//         loaded or ncclCommInitAll fails (one stderr line; rttnw_stats.reserved bit 9 of rank 0), so that a node whose RCCL is broken
//         still renders.  Bit 8 of stats[0].reserved: the gather went through peer copies.
// RTTNW_MULTI_FORCE_TRANSPORT=1 (tests; RTTNW_MULTI_FORCE_RCCL=1 is the older name): the ranks on the root's device travel through the
// transport too — the root sending to itself — so that the dlopen'ed entry points, the communicator set-up, the peer copies, the stream
// ordering and the error paths run on a box with ONE GPU as well.  RTTNW_MULTI_FAIL_RCCL=1 (tests): the RCCL set-up reports failure.
// RTTNW_DEBUG_MULTI: one stderr line per communicator set-up and per gather.
struct MultiEnv {
    bool force_transport = false, gather_peer = false, gather_invalid = false, fail_rccl = false, debug = false;
    MultiEnv() {
        const auto is_1 = [](const char* e) { return e && e[0] == '1'; };
        force_transport = is_1(getenv("RTTNW_MULTI_FORCE_RCCL")) || is_1(getenv("RTTNW_MULTI_FORCE_TRANSPORT"));
        const char* gather = getenv("RTTNW_MULTI_GATHER");
        gather_peer = gather && std::string(gather) == "peer";
        gather_invalid = gather && !gather_peer && std::string(gather) != "rccl";
        fail_rccl = is_1(getenv("RTTNW_MULTI_FAIL_RCCL"));
        debug = getenv("RTTNW_DEBUG_MULTI") != nullptr;
    }
};

// Who traces what, and where: made once per call (multi_plan), read by every step.
struct MultiPlan {
    const MultiEnv env;
    struct Rank { DeviceState* d; uint32_t dev, slot; }; // its device's state, index in `devices`, and its place among the ranks of that device
    std::vector<Rank> ranks;
    std::vector<int> devices;             // in order of first appearance; devices[0] = the root's (rank 0's) device
    std::vector<DeviceState*> dev_state;  // per distinct device
    std::vector<uint32_t> dev_ranks;      // ... and how many ranks live on it
    DeviceState* root = nullptr;
    size_t rsz = 0, chunk = 0, npx = 0;   // bytes of a real, of a rank's packed tiles; pixels of the image
    size_t aux_chunk = 0;                 // rttnw_render_adaptive_multi: bytes of a rank's auxiliary records, which travel with its tiles (0: a plain render)
    bool single = false;                  // rttnw_render_adaptive_resume with ngpu == 0: one rank on the scene's own device, which reads no gather environment
    bool transport() const { return !single && (devices.size() > 1 || env.force_transport); } // some rank's tiles travel
    bool local(uint32_t r) const { return single || (!env.force_transport && ranks[r].dev == 0); } // rank r's do not: a copy on the root's device
    uint8_t* packed(uint32_t r) const { return ranks[r].d->multi_packed.p + chunk * ranks[r].slot; } // rank r's packed tiles, on its device
    uint8_t* gathered(uint32_t r) const { return root->gathered.p + chunk * r; }                      // ... and their place on the root's
    uint8_t* aux(uint32_t r) const { return ranks[r].d->multi_aux.p + aux_chunk * ranks[r].slot; }    // the same for its auxiliary records
    uint8_t* gathered_aux(uint32_t r) const { return root->gathered_aux.p + aux_chunk * r; }
};

static int multi_plan(::rttnw_scene* s, const rttnw_params& p, uint32_t ngpu, const int32_t* device_ids, MultiPlan& m, const char* call = "render_multi") {
    std::string err;
    m.ranks.resize(ngpu);
    for (uint32_t r = 0; r < ngpu; ++r) {
        DeviceState* d = state_on(s, device_ids[r], err);
        if (!d) { set_last_error(std::string(call) + ": " + err); return RTTNW_ERR_HIP; }
        uint32_t k = 0;
        while (k < m.devices.size() && m.devices[k] != device_ids[r]) ++k;
        if (k == m.devices.size()) { m.devices.push_back(device_ids[r]); m.dev_state.push_back(d); m.dev_ranks.push_back(0); }
        m.ranks[r] = {d, k, m.dev_ranks[k]++};
    }
    rttnw_tile_layout L;
    fill_layout(p.width, p.height, ngpu, L);
    m.root = m.ranks[0].d;
    m.rsz = p.precision == RTTNW_F32 ? sizeof(float) : sizeof(double);
    m.chunk = size_t(L.pixels_per_rank) * 4 * m.rsz;
    m.npx = size_t(p.width) * p.height;
    return 0;
}

// Everything that allocates, before anything is launched (an allocation or a free between two ranks' launches would synchronise its whole
// device): the streams, this layer's buffers, then per rank what a first use brings — scene uploads and workspace growth
// (`frame_image`: the root un-tiles a frame-sized image; rttnw_render_adaptive_region writes a window-sized one instead)
static int multi_prepare_buffers(const MultiPlan& m, bool frame_image = true) {
    for (size_t k = 0; k < m.devices.size(); ++k) {
        DeviceState* d = m.dev_state[k];
        HIP_TRY(hipSetDevice(d->device));
        if (!d->stream) HIP_TRY(create_stream(d->stream, hipStreamNonBlocking));
        HIP_TRY(d->multi_packed.grow(m.chunk * m.dev_ranks[k]));
    }
    DeviceState* root = m.root;
    HIP_TRY(hipSetDevice(root->device));
    HIP_TRY(root->gathered.grow(m.chunk * m.ranks.size()));
    if (!frame_image) return 0;
    HIP_TRY(root->linear.grow(m.npx * 3 * m.rsz));
    HIP_TRY(root->rgba.grow(m.npx * 4));
    return 0;
}
static int multi_prepare(::rttnw_scene* s, const rttnw_camera_desc* cam, const rttnw_params& p, const MultiPlan& m) {
    if (int rc = multi_prepare_buffers(m)) return rc;
    for (uint32_t r = 0; r < m.ranks.size(); ++r) {
        rttnw_params pr = p;
        pr.tile_rank = r;
        DeviceState* d = m.ranks[r].d;
        if (int rc = render_tiles_any(s, d, cam, &pr, m.packed(r), d->stream.get(), nullptr, false, true)) return rc;
    }
    return 0;
}

// Every rank traces its tiles, on its device's stream, between its two events of `ev`; ranks that share a device run one after the other
static int multi_trace(::rttnw_scene* s, const rttnw_camera_desc* cam, const rttnw_params& p, const MultiPlan& m, std::vector<Event>& ev, rttnw_stats* stats) {
    for (uint32_t r = 0; r < m.ranks.size(); ++r) {
        DeviceState* d = m.ranks[r].d;
        HIP_TRY(hipSetDevice(d->device));
        rttnw_params pr = p;
        pr.tile_rank = r;
        HIP_TRY(create_event(ev[2 * r]));
        HIP_TRY(create_event(ev[2 * r + 1]));
        HIP_TRY(hipEventRecord(ev[2 * r].get(), d->stream.get()));
        if (int rc = render_tiles_any(s, d, cam, &pr, m.packed(r), d->stream.get(), stats ? &stats[r] : nullptr, false)) return rc;
        HIP_TRY(hipEventRecord(ev[2 * r + 1].get(), d->stream.get()));
    }
    return 0;
}

// The communicator set over `devices`: found, or made at the first call over that list and kept (set-up costs ~100 ms; destroyed by
// rttnw_shutdown() or at exit).  nullptr when there is none: a failed set-up says why on stderr, once, and is kept as well — an entry without
// communicators —, so that later calls over that list go straight to the peer copies.  Called with g_comms_mutex held.
static MultiComms* comms_over(const std::vector<int>& devices, const MultiEnv& env) {
    for (MultiComms* c : g_comms)
        if (c->devices == devices) return c->comms.empty() ? nullptr : c;
    MultiComms* mc = new MultiComms();
    mc->devices = devices;
    g_comms.push_back(mc);
    std::string why;
    if (env.fail_rccl) why = "RTTNW_MULTI_FAIL_RCCL=1";
    else if (g_rccl.load(why)) {
        mc->comms.resize(devices.size());
        const ncclResult_t nr = g_rccl.CommInitAll(mc->comms.data(), int(devices.size()), devices.data());
        if (nr != ncclSuccess) { why = std::string("ncclCommInitAll: ") + g_rccl.GetErrorString(nr); mc->comms.clear(); }
    }
    if (mc->comms.empty()) {
        fprintf(stderr, "[render_multi] RCCL gather unavailable (%s): gathering through peer copies\n", why.c_str());
        return nullptr;
    }
    if (!g_comms_atexit) { g_comms_atexit = true; std::atexit(destroy_comms); }
    if (env.debug) fprintf(stderr, "[render_multi] RCCL communicators over %zu device(s)\n", devices.size());
    return mc;
}

// The two transports of the ranks' tiles to the root's gather buffer (MultiEnv has what they are).
constexpr int GATHER_UNAVAILABLE = 1; // gather_rccl: there is no communicator set; nothing has been sent yet, so gather_peer can do the same job
static int gather_rccl(const MultiPlan& m) {
    std::unique_lock<std::mutex> comms_lock(g_comms_mutex);
    MultiComms* mc = comms_over(m.devices, m.env);
    if (!mc) return GATHER_UNAVAILABLE;
    // (the list's lock is released, the set's own is taken: two host threads rendering over the SAME devices take turns on
    // its communicators; threads over different device lists do not wait for each other)
    std::unique_lock<std::mutex> use(mc->in_use);
    comms_lock.unlock();
    ncclResult_t nr = g_rccl.GroupStart();
    uint32_t n_sent = 0;
    for (uint32_t r = 0; r < m.ranks.size() && nr == ncclSuccess; ++r) {
        if (m.local(r)) continue; // on the root's device: copied by multi_untile
        const uint32_t k = m.ranks[r].dev;
        nr = g_rccl.Send(m.packed(r), m.chunk, ncclChar, 0, mc->comms[k], m.ranks[r].d->stream.get());
        if (nr == ncclSuccess) nr = g_rccl.Recv(m.gathered(r), m.chunk, ncclChar, int(k), mc->comms[0], m.root->stream.get());
        ++n_sent;
        if (!m.aux_chunk) continue; // the rank's auxiliary records: a second send inside the one group
        if (nr == ncclSuccess) nr = g_rccl.Send(m.aux(r), m.aux_chunk, ncclChar, 0, mc->comms[k], m.ranks[r].d->stream.get());
        if (nr == ncclSuccess) nr = g_rccl.Recv(m.gathered_aux(r), m.aux_chunk, ncclChar, int(k), mc->comms[0], m.root->stream.get());
        ++n_sent;
    }
    ncclResult_t ne = g_rccl.GroupEnd();
    if (nr == ncclSuccess) nr = ne;
    if (nr != ncclSuccess) { set_last_error(std::string("RCCL gather: ") + g_rccl.GetErrorString(nr)); return RTTNW_ERR_HIP; }
    if (m.env.debug) fprintf(stderr, "[render_multi] %u rank buffer(s) of %zu bytes through ncclSend / ncclRecv\n", n_sent, m.chunk);
    return 0;
}
static int gather_peer(const MultiPlan& m) {
    DeviceState* root = m.root;
    // direct access root <- rank device where the fabric allows it (xGMI: every pair of a node); without it the copy is staged by the runtime
    for (size_t k = 1; k < m.devices.size(); ++k) {
        int can = 0;
        if (hipDeviceCanAccessPeer(&can, m.devices[k], root->device) == hipSuccess && can) {
            HIP_TRY(hipSetDevice(m.devices[k]));
            const hipError_t e = hipDeviceEnablePeerAccess(root->device, 0);
            if (e != hipSuccess && e != hipErrorPeerAccessAlreadyEnabled) HIP_TRY(e);
            (void)hipGetLastError();
        }
    }
    std::vector<Event> sent(m.ranks.size());
    uint32_t n_sent = 0;
    for (uint32_t r = 0; r < m.ranks.size(); ++r) {
        if (m.local(r)) continue; // on the root's device: copied by multi_untile
        DeviceState* d = m.ranks[r].d;
        HIP_TRY(hipSetDevice(d->device));
        HIP_TRY(hipMemcpyPeerAsync(m.gathered(r), root->device, m.packed(r), d->device, m.chunk, d->stream.get()));
        if (m.aux_chunk) { HIP_TRY(hipMemcpyPeerAsync(m.gathered_aux(r), root->device, m.aux(r), d->device, m.aux_chunk, d->stream.get())); ++n_sent; }
        HIP_TRY(create_event(sent[r], hipEventDisableTiming));
        HIP_TRY(hipEventRecord(sent[r].get(), d->stream.get()));
        ++n_sent;
    }
    HIP_TRY(hipSetDevice(root->device));
    for (uint32_t r = 0; r < m.ranks.size(); ++r)
        if (sent[r]) HIP_TRY(hipStreamWaitEvent(root->stream.get(), sent[r].get(), 0)); // the un-tile reads what the ranks' streams have written
    if (m.env.debug) fprintf(stderr, "[render_multi] %u rank buffer(s) of %zu bytes through hipMemcpyPeerAsync\n", n_sent, m.chunk);
    // (the events are destroyed when this function ends: a recorded event may be destroyed while work waits on it — the wait was enqueued)
    return 0;
}

// On the root's stream: the tiles of the ranks that live on its device (unless they went through the transport) join the gathered ones ...
static int multi_join_local(const MultiPlan& m) {
    DeviceState* root = m.root;
    HIP_TRY(hipSetDevice(root->device));
    for (uint32_t r = 0; r < m.ranks.size(); ++r) {
        if (!m.local(r)) continue;
        HIP_TRY(hipMemcpyAsync(m.gathered(r), m.packed(r), m.chunk, hipMemcpyDeviceToDevice, root->stream.get()));
        if (m.aux_chunk) HIP_TRY(hipMemcpyAsync(m.gathered_aux(r), m.aux(r), m.aux_chunk, hipMemcpyDeviceToDevice, root->stream.get()));
    }
    return 0;
}
// ... and, once the image is enqueued behind them, every device's stream has finished
static int multi_finish_streams(const MultiPlan& m) {
    for (DeviceState* d : m.dev_state) {
        HIP_TRY(hipSetDevice(d->device));
        HIP_TRY(hipStreamSynchronize(d->stream.get()));
    }
    HIP_TRY(hipSetDevice(m.root->device));
    return 0;
}
// The frame's image (and, of auxiliary records, its samples and standard-error maps) made of the gathered tiles on the root
static int multi_untile(const rttnw_params& p, const MultiPlan& m) {
    DeviceState* root = m.root;
    if (int rc = multi_join_local(m)) return rc;
    if (int rc = rttnw_untile_device(p.width, p.height, p.tile_world, p.precision, root->gathered.p, root->linear.p, root->rgba.p, root->stream.get())) return rc;
    if (m.aux_chunk) // ... and the samples and standard-error maps of the auxiliary records
        if (int rc = RT_BY_PRECISION(p.precision, untile_aux_launch, p.width, p.height, p.tile_world, (const double*)root->gathered_aux.p, (uint32_t*)root->ad_spp.p,
                                     (double*)root->ad_stderr.p, root->stream.get())) return rc;
    return multi_finish_streams(m);
}
// The ranks' buffers to the root's gather buffers, by the transport the call uses (MultiEnv), falling through from RCCL to the peer copies
static int multi_gather(const MultiPlan& m, bool& use_peer, bool& fell_back) {
    use_peer = m.transport() && m.env.gather_peer;
    fell_back = false;
    if (m.transport() && !use_peer) {
        const int rc = gather_rccl(m);
        if (rc == GATHER_UNAVAILABLE) use_peer = fell_back = true;
        else if (rc) return rc;
    }
    return use_peer ? gather_peer(m) : 0;
}
} // namespace rt

extern "C" int rttnw_render_multi(rttnw_scene* s, const rttnw_camera_desc* cam, const rttnw_params* p_in, uint32_t ngpu, const int32_t* device_ids,
                                  double* out_linear_rgb, uint8_t* out_rgba8, rttnw_stats* stats) {
    using namespace rt;
    if (!p_in || !ngpu || ngpu > 64 || !device_ids) { set_last_error("render_multi: bad arguments"); return RTTNW_ERR_INVALID; }
    rttnw_params p = *p_in;
    p.tile_rank = 0; p.tile_world = ngpu;
    if (int rc = validate(s, cam, &p)) return rc;
    const int n_dev = rttnw_device_count();
    for (uint32_t r = 0; r < ngpu; ++r)
        if (device_ids[r] < 0 || device_ids[r] >= n_dev) { set_last_error("render_multi: no such device"); return RTTNW_ERR_INVALID; }
    DeviceGuard restore; // (the caller's device is current again after EVERY return below, the error paths included)
    MultiPlan m;
    if (int rc = multi_plan(s, p, ngpu, device_ids, m)) return rc;
    if (int rc = multi_prepare(s, cam, p, m)) return rc;
    std::vector<Event> ev(size_t(ngpu) * 2); // per rank: before and behind its trace
    if (int rc = multi_trace(s, cam, p, m, ev, stats)) return rc;
    // (refused here, after the trace, as it always was)
    if (m.env.gather_invalid) { set_last_error("render_multi: RTTNW_MULTI_GATHER must be rccl or peer"); return RTTNW_ERR_INVALID; }
    bool use_peer = false, fell_back = false;
    if (int rc = multi_gather(m, use_peer, fell_back)) return rc;
    if (int rc = multi_untile(p, m)) return rc;
    for (uint32_t r = 0; r < ngpu && stats; ++r) {
        float ms = 0;
        HIP_TRY(hipSetDevice(m.ranks[r].d->device));
        HIP_TRY(hipEventElapsedTime(&ms, ev[2 * r].get(), ev[2 * r + 1].get()));
        stats[r].kernel_ms = ms; // trace + resolve of this rank (the other fields are render_tiles_t's)
    }
    if (stats && use_peer) stats[0].reserved |= 0x100u | (fell_back ? 0x200u : 0u);
    HIP_TRY(hipSetDevice(m.root->device));
    return copy_image_out("render_multi", m.root->rgba, m.root->linear, p.precision, m.npx, out_rgba8, out_linear_rgb);
}

// ---------------------------------------------------------------------------------------------
// rttnw_render_adaptive_multi: rttnw_render_adaptive over the ranks of rttnw_render_multi (include/rttnw_hip.h has the contract, DESIGN.md §10a the
// why).  Rank r runs render_adaptive_t's passes over ITS tiles — render_tiles_t with tile_rank = r — but the loop is pass-major, rank-minor: a pass
// is enqueued on every live rank's stream before the host waits for any of them, so the devices of a node work side by side.
// rttnw_render_adaptive_resume is the same render begun from, and left as, a state (adaptive_node_render runs both): its passes go by LEVEL, the
// number of passes a pixel has behind it.  rttnw_render_adaptive_region is the resumed render over a SELECTION — a window of the frame, or a mask
// inside it —, where a pixel may hold no samples yet: only selected pixels are ever active, and the outputs are the window's.
// ---------------------------------------------------------------------------------------------
namespace rt {
// ---- the state of rttnw_render_adaptive_resume on the host (include/rttnw_hip.h has the layout): its header, its checks, and the permutation between
// its row-major records and the ranks' packed order
constexpr uint32_t STATE_HEADER_DOUBLES = RTTNW_ADAPTIVE_STATE_HEADER, STATE_HEADER_FIELDS = 31;
static_assert(STATE_RECORD_DOUBLES == RTTNW_ADAPTIVE_STATE_RECORD, "the kernels' record is the header's");
static const char* const STATE_FIELD_NAMES[STATE_HEADER_FIELDS] = {
    "magic", "version", "width", "height", "pass_spp", "spp_chunk", "sample_begin", "precision", "max_depth", "quirks", "seed", "seed", "t_min",
    "background", "background", "background", "camera lookfrom", "camera lookfrom", "camera lookfrom", "camera lookat", "camera lookat", "camera lookat",
    "camera view_up", "camera view_up", "camera view_up", "camera vertical_fov", "camera aspect_ratio", "camera aperture", "camera focus_distance",
    "camera open_time", "camera close_time"};
// The header this call's arguments make (cam == nullptr: validate() refuses the call next; its camera fields are then not compared)
static void state_header(const rttnw_params& p, const rttnw_adaptive& a, const rttnw_camera_desc* cam, double h[STATE_HEADER_DOUBLES]) {
    std::fill(h, h + STATE_HEADER_DOUBLES, 0.0);
    h[0] = double(RTTNW_ADAPTIVE_STATE_MAGIC); h[1] = double(RTTNW_ADAPTIVE_STATE_VERSION);
    h[2] = p.width; h[3] = p.height; h[4] = a.pass_spp; h[5] = p.spp_chunk; h[6] = p.sample_begin; h[7] = p.precision; h[8] = p.max_depth; h[9] = p.quirks;
    h[10] = double(uint32_t(p.seed)); h[11] = double(uint32_t(p.seed >> 32));
    h[12] = p.t_min;
    for (int k = 0; k < 3; ++k) h[13 + k] = p.background[k];
    static_assert(sizeof(rttnw_camera_desc) == 15 * sizeof(double), "the state's header holds the camera as 15 doubles");
    if (cam) std::memcpy(h + 16, cam, sizeof(*cam));
}
// Where a call's level loop starts, and up to which level each rank must look even when a list comes back empty (a fresh render: level 0 only)
struct LevelPlan {
    bool resumed = false;
    uint32_t first = 0;         // the lowest level n / B a pixel of the state stands at
    std::vector<uint32_t> last; // per rank: the highest
};
// What `caller` (rttnw_render_adaptive_resume, rttnw_render_adaptive_region) refuses of a state_in (p and a have passed refuse_adaptive_misuse);
// `first`: the lowest level in it.  `allow_empty` (the region form): a record of twelve zeros — a pixel that holds no samples yet — is accepted.
static int refuse_state_misuse(const char* caller, bool allow_empty, const rttnw_params& p, const rttnw_adaptive& a, const rttnw_camera_desc* cam,
                               const double* st, uint32_t& first) {
    const std::string call = std::string(caller) + ": state_in: ";
    double want[STATE_HEADER_DOUBLES];
    state_header(p, a, cam, want);
    for (uint32_t i = 0; i < (cam ? STATE_HEADER_FIELDS : 16u); ++i) {
        if (std::memcmp(&st[i], &want[i], sizeof(double)) == 0) continue;
        set_last_error(call + (i == 0 ? "wrong magic number: not a state of this library" : i == 1 ? "unknown format version"
                                      : std::string(STATE_FIELD_NAMES[i]) + " differs from this call's"));
        return RTTNW_ERR_INVALID;
    }
    first = 0;
    if (!p.width || !p.height) return 0; // (validate() refuses the call next)
    RenderConsts rc{};
    plan_chunks(rc, a.pass_spp, p.spp_chunk);
    const double B = a.pass_spp, cap = p.spp, chunks = rc.n_chunks;
    const auto whole = [](double v) { return v >= 0.0 && v <= 4294967295.0 && v == std::floor(v); }; // (false for NaN and the infinities)
    double lowest = cap;
    const size_t npx = size_t(p.width) * p.height;
    for (size_t q = 0; q < npx; ++q) {
        const double* rec = st + STATE_HEADER_DOUBLES + q * STATE_RECORD_DOUBLES;
        const double n = rec[3], k = rec[7];
        if (allow_empty && n == 0.0) {
            if (std::all_of(rec, rec + STATE_RECORD_DOUBLES, [](double v) { return v == 0.0; })) { lowest = 0.0; continue; }
            set_last_error(call + "a record's n is 0 but the record is not empty (a pixel without samples is twelve zeros) (pixel " + std::to_string(q) + ")");
            return RTTNW_ERR_INVALID;
        }
        const char* why = !whole(n) ? "a record's n is not a finite integer" : !whole(k) ? "a record's k is not a finite integer"
                        : n < B ? "a record's n is below pass_spp" : std::fmod(n, B) != 0.0 ? "a record's n is not a multiple of pass_spp"
                        : n > cap ? "the state holds more samples than the cap (a record's n exceeds spp)"
                        : k != n / B * chunks ? "a record's k is not its passes times the chunks of a pass" : nullptr;
        if (why) { set_last_error(call + why + " (pixel " + std::to_string(q) + ")"); return RTTNW_ERR_INVALID; }
        lowest = std::min(lowest, n);
    }
    first = uint32_t(lowest / B);
    return 0;
}
// Packed index of framebuffer pixel (x, y) on its owner among `world` ranks (rt_core.hpp tile_permuted; rttnw_amd/tiles.py packed_index)
static inline void packed_place(uint32_t x, uint32_t y, const rttnw_tile_layout& L, uint32_t world, uint32_t& owner, size_t& idx) {
    const uint32_t permuted = tile_permuted(x >> 3, y >> 3, L.tiles_x);
    owner = permuted % world;
    idx = size_t(permuted / world) * 64 + ((y & 7u) << 3) + (x & 7u);
}
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
            if (int rc = RT_BY_PRECISION(p.precision, adaptive_level_select_launch, marks, sl.state(m, r), sl.marks(m, r), n_blocks * 4u,
                                         level * a.pass_spp, stream)) return rc;
            marks = sl.marks(m, r);
        }
        if (int rc = RT_BY_PRECISION(p.precision, enqueue_quad_list, marks, n_blocks, scan, sl.quads(m, r), stream)) return rc;
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
            if (sel) {
                pr.tile_rank = r;
                if (int rc = RT_BY_PRECISION(p.precision, adaptive_region_activate_launch, s, d, &pr, sel->mask ? (const uint8_t*)d->rg_mask.p : nullptr,
                                             sl.select(m, r), sl.state(m, r), sl.active(m, r), sel->x0, sel->y0, sel->x1, sel->y1, stream)) return rc;
            }
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
    std::vector<std::vector<double>> host_records(lv.resumed || state_out ? ngpu : 0);
    for (std::vector<double>& v : host_records) v.assign(rank_doubles, 0.0);
    if (state_in)
        for (uint32_t y = 0; y < p.height; ++y)
            for (uint32_t x = 0; x < p.width; ++x) {
                uint32_t owner;
                size_t idx;
                packed_place(x, y, sl.L, ngpu, owner, idx);
                const double* rec = state_in + STATE_HEADER_DOUBLES + (size_t(y) * p.width + x) * STATE_RECORD_DOUBLES;
                std::copy(rec, rec + STATE_RECORD_DOUBLES, host_records[owner].begin() + idx * STATE_RECORD_DOUBLES);
                if (!sel) lv.last[owner] = std::max(lv.last[owner], uint32_t(rec[3]) / a->pass_spp);
            }
    // a selection: the levels its pixels stand at (an unselected pixel is never active), and per rank the blocks that hold a selected pixel
    std::vector<uint32_t> sel_blocks(sel ? ngpu : 0, 0);
    if (sel) {
        lv.first = p.spp / a->pass_spp; // (nothing selected: no level to run)
        for (uint32_t y = sel->y0; y < sel->y1; ++y)
            for (uint32_t x = sel->x0; x < sel->x1; ++x) {
                if (!sel->has(x, y)) continue;
                uint32_t owner;
                size_t idx;
                packed_place(x, y, sl.L, ngpu, owner, idx);
                const uint32_t level = uint32_t(host_records[owner][idx * STATE_RECORD_DOUBLES + 3]) / a->pass_spp;
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
        for (uint32_t y = 0; y < p.height; ++y)
            for (uint32_t x = 0; x < p.width; ++x) {
                uint32_t owner;
                size_t idx;
                packed_place(x, y, sl.L, ngpu, owner, idx);
                const double* rec = host_records[owner].data() + idx * STATE_RECORD_DOUBLES;
                std::copy(rec, rec + STATE_RECORD_DOUBLES, state_out + STATE_HEADER_DOUBLES + (size_t(y) * p.width + x) * STATE_RECORD_DOUBLES);
            }
    }
    DeviceState* root = m.root;
    HIP_TRY(hipSetDevice(root->device));
    hipError_t e = hipSuccess;
    const size_t out_px = sel ? sel->pixels() : m.npx;
    if (out_spp) e = hipMemcpy(out_spp, (sel ? root->rg_spp : root->ad_spp).p, out_px * sizeof(uint32_t), hipMemcpyDeviceToHost);
    if (e == hipSuccess && out_stderr_rgb) e = hipMemcpy(out_stderr_rgb, (sel ? root->rg_stderr : root->ad_stderr).p, out_px * 3 * sizeof(double), hipMemcpyDeviceToHost);
    return copy_image_out(call, sel ? root->rg_rgba : root->rgba, sel ? root->rg_linear : root->linear, p.precision, out_px, out_rgba8, out_linear_rgb, e);
}
} // namespace rt

extern "C" int rttnw_render_adaptive_multi(rttnw_scene* s, const rttnw_camera_desc* cam, const rttnw_params* p_in, const rttnw_adaptive* a, uint32_t ngpu,
                                           const int32_t* device_ids, double* out_linear_rgb, uint8_t* out_rgba8, uint32_t* out_spp, double* out_stderr_rgb,
                                           rttnw_stats* stats) {
    using namespace rt;
    // the refusals, in the header's order: none of them needs a device
    if (!p_in || !a) { set_last_error("render_adaptive_multi: NULL argument (p or a)"); return RTTNW_ERR_INVALID; }
    if (!ngpu || ngpu > 64) { set_last_error("render_adaptive_multi: ngpu must be 1 .. 64"); return RTTNW_ERR_INVALID; }
    if (!device_ids) { set_last_error("render_adaptive_multi: device_ids is NULL"); return RTTNW_ERR_INVALID; }
    if (int rc = refuse_adaptive_misuse("render_adaptive_multi", p_in, a)) return rc;
    rttnw_params p = *p_in;
    p.tile_rank = 0; p.tile_world = 1; // (the caller's are ignored, so the tile_world rule of the single call has nothing to refuse)
    if (int rc = refuse_host_output_misuse("render_adaptive_multi", a->reserved0, &p)) return rc;
    p.tile_world = ngpu;
    if (int rc = validate(s, cam, &p)) return rc;
    const int n_dev = rttnw_device_count();
    for (uint32_t r = 0; r < ngpu; ++r)
        if (device_ids[r] < 0 || device_ids[r] >= n_dev) { set_last_error("render_adaptive_multi: no such device in device_ids"); return RTTNW_ERR_INVALID; }
    return adaptive_node_render("render_adaptive_multi", s, cam, p, a, ngpu, device_ids, false, nullptr, 0, nullptr, out_linear_rgb, out_rgba8, out_spp,
                                out_stderr_rgb, stats);
}

extern "C" uint64_t rttnw_adaptive_state_doubles(uint32_t width, uint32_t height) {
    return uint64_t(RTTNW_ADAPTIVE_STATE_HEADER) + uint64_t(RTTNW_ADAPTIVE_STATE_RECORD) * width * height;
}

// rttnw_render_adaptive_resume (include/rttnw_hip.h has the contract and the state's layout, DESIGN.md §10a "resumable form" the why)
extern "C" int rttnw_render_adaptive_resume(rttnw_scene* s, const rttnw_camera_desc* cam, const rttnw_params* p_in, const rttnw_adaptive* a, uint32_t ngpu,
                                            const int32_t* device_ids, const double* state_in, double* state_out, double* out_linear_rgb,
                                            uint8_t* out_rgba8, uint32_t* out_spp, double* out_stderr_rgb, rttnw_stats* stats) {
    using namespace rt;
    // the refusals, in the header's order: none of them needs a device
    if (!p_in || !a) { set_last_error("render_adaptive_resume: NULL argument (p or a)"); return RTTNW_ERR_INVALID; }
    if (ngpu > 64) { set_last_error("render_adaptive_resume: ngpu must be 0 .. 64"); return RTTNW_ERR_INVALID; }
    if (ngpu && !device_ids) { set_last_error("render_adaptive_resume: device_ids is NULL with ngpu >= 1"); return RTTNW_ERR_INVALID; }
    if (!ngpu && device_ids) { set_last_error("render_adaptive_resume: device_ids must be NULL with ngpu == 0 (the current device)"); return RTTNW_ERR_INVALID; }
    if (int rc = refuse_adaptive_misuse("render_adaptive_resume", p_in, a)) return rc;
    rttnw_params p = *p_in;
    if (ngpu) { p.tile_rank = 0; p.tile_world = 1; } // (ngpu >= 1: the caller's are ignored, as in rttnw_render_adaptive_multi; ngpu == 0: tile_world must be 1)
    if (int rc = refuse_host_output_misuse("render_adaptive_resume", a->reserved0, &p)) return rc;
    uint32_t first_level = 0;
    if (state_in)
        if (int rc = refuse_state_misuse("render_adaptive_resume", false, *p_in, *a, cam, state_in, first_level)) return rc;
    p.tile_rank = 0; p.tile_world = std::max(ngpu, 1u);
    if (int rc = validate(s, cam, &p)) return rc;
    const int n_dev = rttnw_device_count();
    for (uint32_t r = 0; r < ngpu; ++r)
        if (device_ids[r] < 0 || device_ids[r] >= n_dev) { set_last_error("render_adaptive_resume: no such device in device_ids"); return RTTNW_ERR_INVALID; }
    const int32_t own = s->device->device; // ngpu == 0: one rank where rttnw_render_adaptive runs
    return adaptive_node_render("render_adaptive_resume", s, cam, p, a, std::max(ngpu, 1u), ngpu ? device_ids : &own, ngpu == 0, state_in, first_level,
                                state_out, out_linear_rgb, out_rgba8, out_spp, out_stderr_rgb, stats);
}

// rttnw_render_adaptive_region (include/rttnw_hip.h has the contract, DESIGN.md §10a "windowed form" the why): the resumed render over a selection
extern "C" int rttnw_render_adaptive_region(rttnw_scene* s, const rttnw_camera_desc* cam, const rttnw_params* p_in, const rttnw_adaptive* a, uint32_t x0,
                                            uint32_t y0, uint32_t x1, uint32_t y1, const uint8_t* mask, uint32_t ngpu, const int32_t* device_ids,
                                            const double* state_in, double* state_out, double* out_linear_rgb, uint8_t* out_rgba8, uint32_t* out_spp,
                                            double* out_stderr_rgb, rttnw_stats* stats) {
    using namespace rt;
    // the refusals, in the header's order: none of them needs a device
    if (!p_in || !a) { set_last_error("render_adaptive_region: NULL argument (p or a)"); return RTTNW_ERR_INVALID; }
    if (x0 >= x1 || y0 >= y1 || x1 > p_in->width || y1 > p_in->height) {
        set_last_error("render_adaptive_region: the window [x0, x1) x [y0, y1) must be non-empty and lie inside the width x height frame");
        return RTTNW_ERR_INVALID;
    }
    if (ngpu > 64) { set_last_error("render_adaptive_region: ngpu must be 0 .. 64"); return RTTNW_ERR_INVALID; }
    if (ngpu && !device_ids) { set_last_error("render_adaptive_region: device_ids is NULL with ngpu >= 1"); return RTTNW_ERR_INVALID; }
    if (!ngpu && device_ids) { set_last_error("render_adaptive_region: device_ids must be NULL with ngpu == 0 (the current device)"); return RTTNW_ERR_INVALID; }
    if (int rc = refuse_adaptive_misuse("render_adaptive_region", p_in, a)) return rc;
    rttnw_params p = *p_in;
    if (ngpu) { p.tile_rank = 0; p.tile_world = 1; } // (ngpu >= 1: the caller's are ignored; ngpu == 0: tile_world must be 1)
    if (int rc = refuse_host_output_misuse("render_adaptive_region", a->reserved0, &p)) return rc;
    uint32_t first_level = 0; // (not used: the levels are the selected pixels', adaptive_node_render)
    if (state_in)
        if (int rc = refuse_state_misuse("render_adaptive_region", true, *p_in, *a, cam, state_in, first_level)) return rc;
    p.tile_rank = 0; p.tile_world = std::max(ngpu, 1u);
    if (int rc = validate(s, cam, &p)) return rc;
    const int n_dev = rttnw_device_count();
    for (uint32_t r = 0; r < ngpu; ++r)
        if (device_ids[r] < 0 || device_ids[r] >= n_dev) { set_last_error("render_adaptive_region: no such device in device_ids"); return RTTNW_ERR_INVALID; }
    const int32_t own = s->device->device; // ngpu == 0: one rank where rttnw_render_adaptive runs
    const RegionSelection sel{x0, y0, x1, y1, mask};
    return adaptive_node_render("render_adaptive_region", s, cam, p, a, std::max(ngpu, 1u), ngpu ? device_ids : &own, ngpu == 0, state_in, 0, state_out,
                                out_linear_rgb, out_rgba8, out_spp, out_stderr_rgb, stats, &sel);
}

// ---------------------------------------------------------------------------------------------
// rttnw_render_adaptive_denoised (include/rttnw_hip.h has the contract, DESIGN.md §10a "filter-guided form" the why): adaptive rounds whose stopping
// rule reads the FILTERED image.  One rank on the scene's device, default stream.  A round is one level of the windowed form's loop — the list of the
// 2x2 blocks that hold an alive pixel, render_tiles_t's list pass over it with the windowed form's arguments (a cap of (k+1)B and zero tolerances), the
// running sums COPIED and turned into means and auxiliary records by adaptive_finish_launch (the sums themselves stay for the next round) — and then the
// denoiser's passes and the stop kernel (guided.hpp), all on buffers that never leave the device: per round the host reads the list's two totals, 8
// bytes, which are also the count of alive pixels.
// ---------------------------------------------------------------------------------------------
namespace rt {
// A frame that lives on ONE rank: its packed state records (adaptive_state_export_launch) come back from the device and go to their row-major places
// behind the header (rttnw_render_adaptive_denoised, rttnw_render_preview)
static int single_rank_state_out(const rttnw_params& p, const rttnw_adaptive& a, const rttnw_camera_desc* cam, const rttnw_tile_layout& L,
                                 const double* d_records, double* state_out) {
    std::vector<double> host_records(size_t(L.pixels_per_rank) * STATE_RECORD_DOUBLES);
    HIP_TRY(hipMemcpy(host_records.data(), d_records, host_records.size() * sizeof(double), hipMemcpyDeviceToHost));
    state_header(p, a, cam, state_out);
    for (uint32_t y = 0; y < p.height; ++y)
        for (uint32_t x = 0; x < p.width; ++x) {
            uint32_t owner;
            size_t idx;
            packed_place(x, y, L, 1, owner, idx);
            const double* rec = host_records.data() + idx * STATE_RECORD_DOUBLES;
            std::copy(rec, rec + STATE_RECORD_DOUBLES, state_out + STATE_HEADER_DOUBLES + (size_t(y) * p.width + x) * STATE_RECORD_DOUBLES);
        }
    return RTTNW_OK;
}
static int adaptive_denoised_render(::rttnw_scene* s, const rttnw_camera_desc* cam, const rttnw_params& p, const rttnw_adaptive& a, const rttnw_guided& g,
                                    double* out_linear_rgb, uint8_t* out_rgba8, uint32_t* out_spp, double* out_stderr_rgb, double* out_raw_linear_rgb,
                                    double* out_raw_stderr_rgb, double* state_out, rttnw_stats* stats) {
    DeviceGuard restore; // (the caller's device is current again after EVERY return below, the error paths included)
    DeviceState* d = s->device;
    HIP_TRY(hipSetDevice(d->device));
    rttnw_tile_layout L;
    fill_layout(p.width, p.height, 1, L);
    const size_t npx = size_t(p.width) * p.height, ppr = L.pixels_per_rank, rsz = p.precision == RTTNW_F32 ? sizeof(float) : sizeof(double);
    const uint32_t n_blocks = L.n_tiles * 16u, B = a.pass_spp, n_rounds = p.spp / B;
    const hipStream_t stream = nullptr;
    // everything that allocates, before the first launch: the adaptive passes' buffers, this call's own, and what a list pass over every block needs
    HIP_TRY(d->packed.grow(ppr * 4 * rsz));
    HIP_TRY(d->ad_state.grow(ppr * sizeof(AdaptivePixel)));
    HIP_TRY(d->ad_active.grow(ppr)); // (the resolve step's active bytes under the pass's own cap: not read here, the alive bytes decide)
    HIP_TRY(d->list_quads.grow(size_t(n_blocks) * sizeof(uint32_t)));
    HIP_TRY(d->list_scan.grow(quad_scan_words(n_blocks) * sizeof(uint32_t)));
    DevBuf<uint8_t> alive, means, rgba;
    DevBuf<uint32_t> spp;
    DevBuf<double> aux, maps, mean, variance, raw_stderr, stderr_f, d_c[2], d_v[2], records;
    HIP_TRY(alive.alloc(ppr));
    HIP_TRY(means.alloc(ppr * 4 * rsz));
    HIP_TRY(rgba.alloc(npx * 4));
    HIP_TRY(spp.alloc(npx));
    HIP_TRY(aux.alloc(ppr * 4));
    HIP_TRY(maps.alloc(npx * 8));
    HIP_TRY(mean.alloc(npx * 3));
    HIP_TRY(variance.alloc(npx * 3));
    HIP_TRY(raw_stderr.alloc(npx * 3));
    HIP_TRY(stderr_f.alloc(npx * 3));
    for (int k = 0; k < 2; ++k) {
        HIP_TRY(d_c[k].alloc(npx * 3));
        HIP_TRY(d_v[k].alloc(npx * 3));
    }
    if (state_out) HIP_TRY(records.alloc(ppr * STATE_RECORD_DOUBLES));
    Event ev0, ev1;
    HIP_TRY(create_event(ev0));
    HIP_TRY(create_event(ev1));
    rttnw_params pass = p;
    pass.spp = B;
    ListPass ad;
    ad.state = (AdaptivePixel*)d->ad_state.p;
    ad.active = d->ad_active.p;
    ad.quads = (const uint32_t*)d->list_quads.p;
    ad.n_quads = n_blocks;
    ad.first = false; // (round 0 too is a list pass on zero sums: 0 + c0 is the chain's first addition, as in the windowed form)
    if (int rc = render_tiles_any(s, d, cam, &pass, d->packed.p, stream, nullptr, false, true, &ad)) return rc;
    if (stats)
        if (int rc = RT_BY_PRECISION(p.precision, adaptive_rank_stats_t, s, d, &p, stats)) return rc;

    // before round 0: the feature maps, which stay on the device, and every pixel of the image alive on zero sums and zero noise state
    rttnw_params pf = p;
    pf.spp = g.feature_spp ? g.feature_spp : B;
    if (int rc = RT_BY_PRECISION(p.precision, render_features_device_t, s, cam, &pf, maps.p, stream)) return rc;
    float feature_ms = 0;
    HIP_TRY(hipEventElapsedTime(&feature_ms, d->ev0.get(), d->ev1.get()));
    const double *m_albedo = maps.p, *m_normal = maps.p + npx * 3, *m_depth = maps.p + npx * 6, *m_alpha = maps.p + npx * 7;
    const DenoiseParams prm = denoise_params(g.denoise.sigma_luminance, g.denoise.sigma_normal, g.denoise.sigma_depth, true);
    double* const c[2] = {d_c[0].p, d_c[1].p};
    double* const v[2] = {d_v[0].p, d_v[1].p};
    HIP_TRY(hipEventRecord(ev0.get(), stream));
    HIP_TRY(hipMemsetAsync(d->packed.p, 0, ppr * 4 * rsz, stream));
    HIP_TRY(hipMemsetAsync(d->ad_state.p, 0, ppr * sizeof(AdaptivePixel), stream));
    if (int rc = guided_begin_launch(alive.p, L.pixels_per_rank, p.width, p.height, stream)) return rc;
    uint64_t samples = 0;
    int out = 0;
    for (uint32_t k = 0; k < n_rounds; ++k) {
        // the list of this round — the alive bytes are its active AND its selection bytes — and, in one 8-byte copy, its length and the alive pixels
        if (int rc = RT_BY_PRECISION(p.precision, enqueue_quad_list, alive.p, n_blocks, (uint32_t*)d->list_scan.p, (uint32_t*)d->list_quads.p, stream)) return rc;
        uint32_t count[2] = {0, 0}; // listed blocks, alive pixels
        HIP_TRY(hipMemcpy(count, quad_list_totals((uint32_t*)d->list_scan.p, n_blocks), sizeof(count), hipMemcpyDeviceToHost));
        if (count[0] == 0) break; // every pixel has stopped
        samples += uint64_t(count[1]) * B;
        // 1. trace: the alive pixels, all of which hold exactly kB samples — one level
        pass.sample_begin = p.sample_begin + k * B;
        ad.n_quads = count[0];
        ad.cap = (k + 1u) * B;
        if (int rc = render_tiles_any(s, d, cam, &pass, d->packed.p, stream, nullptr, false, false, &ad)) return rc;
        // 2. raw values of every pixel of the frame, by the adaptive render's own division on a copy of the sums
        HIP_TRY(hipMemcpyAsync(means.p, d->packed.p, ppr * 4 * rsz, hipMemcpyDeviceToDevice, stream));
        if (int rc = RT_BY_PRECISION(p.precision, adaptive_finish_launch, means.p, d->ad_state.p, aux.p, L.pixels_per_rank, L.n_tiles * 64u, stream)) return rc;
        if (int rc = guided_raw_launch(p.precision, means.p, aux.p, mean.p, variance.p, raw_stderr.p, spp.p, p.width, p.height, stream)) return rc;
        // 3. filter
        if (int rc = denoise_passes_device(p.width, p.height, mean.p, variance.p, m_albedo, m_normal, m_depth, m_alpha, g.denoise.iterations, prm, c, v,
                                           rgba.p, stream, out)) return rc;
        // 4. stop
        if (int rc = guided_stop_launch(c[out], v[out], raw_stderr.p, a.rel_error, a.abs_error, alive.p, stderr_f.p, p.width, p.height, stream)) return rc;
    }
    if (state_out)
        if (int rc = RT_BY_PRECISION(p.precision, adaptive_state_export_launch, d->packed.p, d->ad_state.p, records.p, L.pixels_per_rank, L.n_tiles * 64u, stream)) return rc;
    HIP_TRY(hipEventRecord(ev1.get(), stream));
    HIP_TRY(hipDeviceSynchronize());
    if (stats) {
        float ms = 0;
        HIP_TRY(hipEventElapsedTime(&ms, ev0.get(), ev1.get()));
        stats->kernel_ms = double(feature_ms) + double(ms);
        stats->samples = samples;
    }
    // the outputs of the last round that ran
    if (out_linear_rgb) HIP_TRY(hipMemcpy(out_linear_rgb, c[out], npx * 3 * sizeof(double), hipMemcpyDeviceToHost));
    if (out_rgba8) HIP_TRY(hipMemcpy(out_rgba8, rgba.p, npx * 4, hipMemcpyDeviceToHost));
    if (out_spp) HIP_TRY(hipMemcpy(out_spp, spp.p, npx * sizeof(uint32_t), hipMemcpyDeviceToHost));
    if (out_stderr_rgb) HIP_TRY(hipMemcpy(out_stderr_rgb, stderr_f.p, npx * 3 * sizeof(double), hipMemcpyDeviceToHost));
    if (out_raw_linear_rgb) HIP_TRY(hipMemcpy(out_raw_linear_rgb, mean.p, npx * 3 * sizeof(double), hipMemcpyDeviceToHost));
    if (out_raw_stderr_rgb) HIP_TRY(hipMemcpy(out_raw_stderr_rgb, raw_stderr.p, npx * 3 * sizeof(double), hipMemcpyDeviceToHost));
    if (state_out)
        if (int rc = single_rank_state_out(p, a, cam, L, records.p, state_out)) return rc;
    return RTTNW_OK;
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
    if (g->denoise.iterations > DENOISE_MAX_ITERATIONS) { set_last_error("render_adaptive_denoised: g->denoise.iterations: more than 8 iterations"); return RTTNW_ERR_INVALID; }
    if (g->denoise.reserved0 != 0) { set_last_error("render_adaptive_denoised: g->denoise.reserved0 must be 0"); return RTTNW_ERR_INVALID; }
    if (!(g->denoise.sigma_luminance >= 0.0) || !(g->denoise.sigma_normal >= 0.0) || !(g->denoise.sigma_depth >= 0.0)) {
        set_last_error("render_adaptive_denoised: g->denoise: the sigmas (sigma_luminance, sigma_normal, sigma_depth) must be >= 0 (and not NaN)");
        return RTTNW_ERR_INVALID;
    }
    if (int rc = validate(s, cam, p)) return rc;
    return adaptive_denoised_render(s, cam, *p, *a, *g, out_linear_rgb, out_rgba8, out_spp, out_stderr_rgb, out_raw_linear_rgb, out_raw_stderr_rgb, state_out,
                                    stats);
}

// ---------------------------------------------------------------------------------------------
// rttnw_render_preview (include/rttnw_hip.h has the contract, DESIGN.md §10b "a frame from a fraction of its pixels" the why): the adaptive rounds of
// the windowed form over a LATTICE of the frame, then the feature pass and rttnw_reconstruct's passes, all on buffers that never leave the device.
// One rank on the scene's device, default stream.  The rounds are adaptive_denoised_render's, with two differences: the bytes that start alive are the
// lattice's (preview_lattice_launch), and a round's list pass runs under the caller's cap and tolerances, so the resolve step's own stopping rule
// writes the next round's bytes — the alive bytes ARE the pass's active bytes.  Every alive pixel holds exactly kB samples in round k, which is one
// level of the windowed form's loop: list for list what rttnw_render_adaptive_region traces under mask = the lattice.
// ---------------------------------------------------------------------------------------------
namespace rt {
static int preview_render(::rttnw_scene* s, const rttnw_camera_desc* cam, const rttnw_params& p, const rttnw_adaptive& a, const rttnw_preview& pv,
                          double* out_linear_rgb, uint8_t* out_rgba8, uint8_t* out_valid, uint32_t* out_spp, double* out_raw_linear_rgb,
                          double* out_raw_stderr_rgb, double* state_out, rttnw_stats* stats) {
    DeviceGuard restore; // (the caller's device is current again after EVERY return below, the error paths included)
    DeviceState* d = s->device;
    HIP_TRY(hipSetDevice(d->device));
    rttnw_tile_layout L;
    fill_layout(p.width, p.height, 1, L);
    const size_t npx = size_t(p.width) * p.height, ppr = L.pixels_per_rank, rsz = p.precision == RTTNW_F32 ? sizeof(float) : sizeof(double);
    const uint32_t n_blocks = L.n_tiles * 16u, B = a.pass_spp, n_rounds = p.spp / B;
    const hipStream_t stream = nullptr;
    // everything that allocates, before the first launch: the adaptive passes' buffers, this call's own, and what a list pass over the lattice's blocks needs
    HIP_TRY(d->packed.grow(ppr * 4 * rsz));
    HIP_TRY(d->ad_state.grow(ppr * sizeof(AdaptivePixel)));
    HIP_TRY(d->ad_active.grow(ppr));
    HIP_TRY(d->list_quads.grow(size_t(n_blocks) * sizeof(uint32_t)));
    HIP_TRY(d->list_scan.grow(quad_scan_words(n_blocks) * sizeof(uint32_t)));
    DevBuf<uint8_t> means, rgba, valid, holds[2], valid_out;
    DevBuf<uint32_t> spp;
    DevBuf<double> aux, maps, mean, variance, raw_stderr, d_c[2], records;
    HIP_TRY(means.alloc(ppr * 4 * rsz));
    HIP_TRY(rgba.alloc(npx * 4));
    HIP_TRY(valid.alloc(npx));
    HIP_TRY(valid_out.alloc(npx));
    HIP_TRY(spp.alloc(npx));
    HIP_TRY(aux.alloc(ppr * 4));
    HIP_TRY(maps.alloc(npx * 8));
    HIP_TRY(mean.alloc(npx * 3));
    HIP_TRY(variance.alloc(npx * 3));
    HIP_TRY(raw_stderr.alloc(npx * 3));
    for (int k = 0; k < 2; ++k) {
        HIP_TRY(d_c[k].alloc(npx * 3));
        HIP_TRY(holds[k].alloc(npx));
    }
    if (state_out) HIP_TRY(records.alloc(ppr * STATE_RECORD_DOUBLES));
    Event ev0, ev1, ev2, ev3;
    HIP_TRY(create_event(ev0));
    HIP_TRY(create_event(ev1));
    HIP_TRY(create_event(ev2));
    HIP_TRY(create_event(ev3));
    // the blocks that hold a lattice pixel: every block at level 0 and 1, one in 4^(level-1) above
    const uint32_t step = 1u << pv.level, block_step = std::max(step, 2u);
    const uint32_t lattice_blocks = ((p.width + block_step - 1) / block_step) * ((p.height + block_step - 1) / block_step);
    rttnw_params pass = p;
    pass.spp = B;
    ListPass ad;
    ad.state = (AdaptivePixel*)d->ad_state.p;
    ad.active = d->ad_active.p;
    ad.quads = (const uint32_t*)d->list_quads.p;
    ad.n_quads = std::min(lattice_blocks, n_blocks);
    ad.first = false; // (round 0 too is a list pass on zero sums: 0 + c0 is the chain's first addition, as in the windowed form)
    ad.cap = p.spp;
    ad.rel_error = a.rel_error;
    ad.abs_error = a.abs_error;
    if (int rc = render_tiles_any(s, d, cam, &pass, d->packed.p, stream, nullptr, false, true, &ad)) return rc;
    if (stats)
        if (int rc = RT_BY_PRECISION(p.precision, adaptive_rank_stats_t, s, d, &p, stats)) return rc;

    // before round 0: zero sums and zero noise state everywhere, and the lattice alive
    HIP_TRY(hipEventRecord(ev0.get(), stream));
    HIP_TRY(hipMemsetAsync(d->packed.p, 0, ppr * 4 * rsz, stream));
    HIP_TRY(hipMemsetAsync(d->ad_state.p, 0, ppr * sizeof(AdaptivePixel), stream));
    if (int rc = preview_lattice_launch(d->ad_active.p, L.pixels_per_rank, p.width, p.height, pv.level, stream)) return rc;
    uint64_t samples = 0;
    for (uint32_t k = 0; k < n_rounds; ++k) {
        // the list of this round and, in one 8-byte copy, its length and the alive pixels
        if (int rc = RT_BY_PRECISION(p.precision, enqueue_quad_list, d->ad_active.p, n_blocks, (uint32_t*)d->list_scan.p, (uint32_t*)d->list_quads.p, stream)) return rc;
        uint32_t count[2] = {0, 0}; // listed blocks, alive pixels
        HIP_TRY(hipMemcpy(count, quad_list_totals((uint32_t*)d->list_scan.p, n_blocks), sizeof(count), hipMemcpyDeviceToHost));
        if (count[0] == 0) break; // every lattice pixel has stopped
        samples += uint64_t(count[1]) * B;
        // trace the alive pixels, all of which hold exactly kB samples; the resolve step decides, under the caller's rule, who is alive in round k + 1
        pass.sample_begin = p.sample_begin + k * B;
        ad.n_quads = count[0];
        if (int rc = render_tiles_any(s, d, cam, &pass, d->packed.p, stream, nullptr, false, false, &ad)) return rc;
    }
    // the raw values of every pixel of the frame, by the adaptive render's own division on a copy of the sums; a pixel holds a value where it holds samples
    if (state_out)
        if (int rc = RT_BY_PRECISION(p.precision, adaptive_state_export_launch, d->packed.p, d->ad_state.p, records.p, L.pixels_per_rank, L.n_tiles * 64u, stream)) return rc;
    HIP_TRY(hipMemcpyAsync(means.p, d->packed.p, ppr * 4 * rsz, hipMemcpyDeviceToDevice, stream));
    if (int rc = RT_BY_PRECISION(p.precision, adaptive_finish_launch, means.p, d->ad_state.p, aux.p, L.pixels_per_rank, L.n_tiles * 64u, stream)) return rc;
    if (int rc = guided_raw_launch(p.precision, means.p, aux.p, mean.p, variance.p, raw_stderr.p, spp.p, p.width, p.height, stream)) return rc;
    if (int rc = preview_valid_launch(spp.p, valid.p, p.width, p.height, stream)) return rc;
    HIP_TRY(hipEventRecord(ev1.get(), stream));
    // the features, which stay on the device (the pass times itself between d->ev0 and d->ev1 and waits for the stream) ...
    rttnw_params pf = p;
    pf.spp = pv.feature_spp ? pv.feature_spp : B;
    if (int rc = RT_BY_PRECISION(p.precision, render_features_device_t, s, cam, &pf, maps.p, stream)) return rc;
    float feature_ms = 0;
    HIP_TRY(hipEventElapsedTime(&feature_ms, d->ev0.get(), d->ev1.get()));
    // ... and the reconstruction: no variance goes into the filter
    const double *m_albedo = maps.p, *m_normal = maps.p + npx * 3, *m_depth = maps.p + npx * 6, *m_alpha = maps.p + npx * 7;
    const DenoiseParams prm = denoise_params(pv.denoise.sigma_luminance, pv.denoise.sigma_normal, pv.denoise.sigma_depth, false);
    double* const c[2] = {d_c[0].p, d_c[1].p};
    double* const v[2] = {nullptr, nullptr};
    uint8_t* const h[2] = {holds[0].p, holds[1].p};
    int out = 0;
    HIP_TRY(hipEventRecord(ev2.get(), stream));
    if (int rc = reconstruct_passes_device(p.width, p.height, mean.p, nullptr, valid.p, m_albedo, m_normal, m_depth, m_alpha, pv.denoise.iterations, prm, c, v,
                                           h, rgba.p, valid_out.p, stream, out)) return rc;
    HIP_TRY(hipEventRecord(ev3.get(), stream));
    HIP_TRY(hipDeviceSynchronize());
    if (stats) {
        float ms = 0, ms_r = 0;
        HIP_TRY(hipEventElapsedTime(&ms, ev0.get(), ev1.get()));
        HIP_TRY(hipEventElapsedTime(&ms_r, ev2.get(), ev3.get()));
        stats->kernel_ms = double(ms) + double(feature_ms) + double(ms_r);
        stats->samples = samples;
    }
    if (out_linear_rgb) HIP_TRY(hipMemcpy(out_linear_rgb, c[out], npx * 3 * sizeof(double), hipMemcpyDeviceToHost));
    if (out_rgba8) HIP_TRY(hipMemcpy(out_rgba8, rgba.p, npx * 4, hipMemcpyDeviceToHost));
    if (out_valid) HIP_TRY(hipMemcpy(out_valid, valid_out.p, npx, hipMemcpyDeviceToHost));
    if (out_spp) HIP_TRY(hipMemcpy(out_spp, spp.p, npx * sizeof(uint32_t), hipMemcpyDeviceToHost));
    if (out_raw_linear_rgb) HIP_TRY(hipMemcpy(out_raw_linear_rgb, mean.p, npx * 3 * sizeof(double), hipMemcpyDeviceToHost));
    if (out_raw_stderr_rgb) HIP_TRY(hipMemcpy(out_raw_stderr_rgb, raw_stderr.p, npx * 3 * sizeof(double), hipMemcpyDeviceToHost));
    if (state_out)
        if (int rc = single_rank_state_out(p, a, cam, L, records.p, state_out)) return rc;
    return RTTNW_OK;
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
    if (v->denoise.iterations > DENOISE_MAX_ITERATIONS) { set_last_error("render_preview: v->denoise.iterations: more than 8 iterations"); return RTTNW_ERR_INVALID; }
    if (v->denoise.reserved0 != 0) { set_last_error("render_preview: v->denoise.reserved0 must be 0"); return RTTNW_ERR_INVALID; }
    if (!(v->denoise.sigma_luminance >= 0.0) || !(v->denoise.sigma_normal >= 0.0) || !(v->denoise.sigma_depth >= 0.0)) {
        set_last_error("render_preview: v->denoise: the sigmas (sigma_luminance, sigma_normal, sigma_depth) must be >= 0 (and not NaN)");
        return RTTNW_ERR_INVALID;
    }
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
static int adaptive_budget_render(::rttnw_scene* s, const rttnw_camera_desc* cam, const rttnw_params& p, const rttnw_adaptive& a, const rttnw_budget& bg,
                                  const double* state_in, double* state_out, double* out_linear_rgb, uint8_t* out_rgba8, uint32_t* out_spp,
                                  double* out_stderr_rgb, rttnw_stats* stats) {
    DeviceGuard restore; // (the caller's device is current again after EVERY return below, the error paths included)
    DeviceState* d = s->device;
    HIP_TRY(hipSetDevice(d->device));
    rttnw_tile_layout L;
    fill_layout(p.width, p.height, 1, L);
    const size_t npx = size_t(p.width) * p.height, ppr = L.pixels_per_rank, rsz = p.precision == RTTNW_F32 ? sizeof(float) : sizeof(double);
    const uint32_t n_blocks = L.n_tiles * 16u, B = a.pass_spp, n_levels = p.spp / B;
    const uint64_t round_pixels = bg.round_pixels ? bg.round_pixels : (uint64_t(npx) + 1u) / 2u; // (half the frame: DESIGN.md §10a has the measurement)
    const hipStream_t stream = nullptr;
    // everything that allocates, before the first launch: the adaptive passes' buffers, this call's own, and what a list pass over every block needs
    HIP_TRY(d->packed.grow(ppr * 4 * rsz));
    HIP_TRY(d->ad_state.grow(ppr * sizeof(AdaptivePixel)));
    HIP_TRY(d->list_quads.grow(size_t(n_blocks) * sizeof(uint32_t)));
    HIP_TRY(d->list_scan.grow(quad_scan_words(n_blocks) * sizeof(uint32_t)));
    HIP_TRY(d->rg_linear.grow(npx * 3 * rsz));
    HIP_TRY(d->rg_rgba.grow(npx * 4));
    HIP_TRY(d->rg_spp.grow(npx * sizeof(uint32_t)));
    HIP_TRY(d->rg_stderr.grow(npx * 3 * sizeof(double)));
    DevBuf<uint8_t> select, marks, means;
    DevBuf<uint32_t> record;
    DevBuf<double> aux, records;
    BudgetWorkspace work;
    HIP_TRY(select.alloc(ppr));
    HIP_TRY(marks.alloc(ppr));
    HIP_TRY(means.alloc(ppr * 4 * rsz));
    HIP_TRY(record.alloc(1u + size_t(n_levels)));
    HIP_TRY(aux.alloc(ppr * 4));
    if (state_in || state_out) HIP_TRY(records.alloc(ppr * STATE_RECORD_DOUBLES));
    HIP_TRY(work.alloc(npx));
    Event ev0, ev1;
    HIP_TRY(create_event(ev0));
    HIP_TRY(create_event(ev1));
    rttnw_params pass = p;
    pass.spp = B;
    ListPass ad;
    ad.state = (AdaptivePixel*)d->ad_state.p;
    ad.active = select.p;
    ad.quads = (const uint32_t*)d->list_quads.p;
    ad.n_quads = n_blocks;
    ad.first = false; // (level 0 too is a list pass on zero sums: 0 + c0 is the chain's first addition, as in the windowed form)
    if (int rc = render_tiles_any(s, d, cam, &pass, d->packed.p, stream, nullptr, false, true, &ad)) return rc;
    if (stats)
        if (int rc = RT_BY_PRECISION(p.precision, adaptive_rank_stats_t, s, d, &p, stats)) return rc;
    // a state_in: its row-major records in the rank's packed order (pixels outside the image keep zero records)
    std::vector<double> host_records;
    if (state_in) {
        host_records.assign(ppr * STATE_RECORD_DOUBLES, 0.0);
        for (uint32_t y = 0; y < p.height; ++y)
            for (uint32_t x = 0; x < p.width; ++x) {
                uint32_t owner;
                size_t idx;
                packed_place(x, y, L, 1, owner, idx);
                const double* rec = state_in + STATE_HEADER_DOUBLES + (size_t(y) * p.width + x) * STATE_RECORD_DOUBLES;
                std::copy(rec, rec + STATE_RECORD_DOUBLES, host_records.begin() + idx * STATE_RECORD_DOUBLES);
            }
    }

    // before round 0: the state comes in (or zero sums and zero noise state), and nothing is selected
    HIP_TRY(hipEventRecord(ev0.get(), stream));
    if (state_in) {
        HIP_TRY(hipMemcpyAsync(records.p, host_records.data(), host_records.size() * sizeof(double), hipMemcpyHostToDevice, stream));
        // (the import's active bytes, under the caller's rule, go to `marks` and are not read: the selection decides who is traced)
        if (int rc = RT_BY_PRECISION(p.precision, adaptive_state_import_launch, records.p, d->packed.p, d->ad_state.p, marks.p, L.pixels_per_rank, p.spp,
                                     a.rel_error, a.abs_error, stream)) return rc;
    } else {
        HIP_TRY(hipMemsetAsync(d->packed.p, 0, ppr * 4 * rsz, stream));
        HIP_TRY(hipMemsetAsync(d->ad_state.p, 0, ppr * sizeof(AdaptivePixel), stream));
    }
    HIP_TRY(hipMemsetAsync(select.p, 0, ppr, stream)); // (the rest of an edge tile is never selected: a round writes the bytes of the image's pixels only)
    uint64_t remaining = bg.samples, samples = 0, rounds = 0;
    std::vector<uint32_t> census(1u + size_t(n_levels));
    ad.rel_error = 0.0;
    ad.abs_error = 0.0;
    for (;;) {
        // the values every pixel is ranked by — and the call's outputs, if this round selects nothing: the adaptive render's own division on a copy of the sums
        HIP_TRY(hipMemcpyAsync(means.p, d->packed.p, ppr * 4 * rsz, hipMemcpyDeviceToDevice, stream));
        if (int rc = RT_BY_PRECISION(p.precision, adaptive_finish_launch, means.p, d->ad_state.p, aux.p, L.pixels_per_rank, L.n_tiles * 64u, stream)) return rc;
        const uint64_t max_pixels = std::min<uint64_t>(round_pixels, remaining / B);
        if (max_pixels == 0) break; // the budget pays for no further pass
        // the selection, and in one copy its record: the pixels selected and, per level, the length of the list over them
        if (int rc = budget_round_launch(work, p.precision, means.p, aux.p, d->ad_state.p, p.width, p.height, p.spp, B, a.rel_error, a.abs_error, max_pixels,
                                         select.p, record.p, stream)) return rc;
        HIP_TRY(hipMemcpy(census.data(), record.p, census.size() * sizeof(uint32_t), hipMemcpyDeviceToHost));
        if (census[0] == 0) break; // no candidate is left
        ++rounds;
        remaining -= uint64_t(census[0]) * B;
        samples += uint64_t(census[0]) * B;
        for (uint32_t k = 0; k < n_levels; ++k) {
            if (census[1u + k] == 0) continue;
            if (int rc = RT_BY_PRECISION(p.precision, adaptive_level_select_launch, select.p, d->ad_state.p, marks.p, n_blocks * 4u, k * B, stream)) return rc;
            if (int rc = RT_BY_PRECISION(p.precision, enqueue_quad_list, marks.p, n_blocks, (uint32_t*)d->list_scan.p, (uint32_t*)d->list_quads.p, stream)) return rc;
            pass.sample_begin = p.sample_begin + k * B;
            ad.n_quads = census[1u + k];
            ad.cap = (k + 1u) * B;
            if (int rc = render_tiles_any(s, d, cam, &pass, d->packed.p, stream, nullptr, false, false, &ad)) return rc;
        }
    }
    // the state the call ends in, and the whole frame as the windowed form reports a window (`means` and `aux` are those of that state)
    if (state_out)
        if (int rc = RT_BY_PRECISION(p.precision, adaptive_state_export_launch, d->packed.p, d->ad_state.p, records.p, L.pixels_per_rank, L.n_tiles * 64u, stream)) return rc;
    if (int rc = RT_BY_PRECISION(p.precision, adaptive_region_window_launch, p.width, p.height, 1u, means.p, aux.p, d->rg_linear.p, d->rg_rgba.p,
                                 (uint32_t*)d->rg_spp.p, (double*)d->rg_stderr.p, 0u, 0u, p.width, p.height, stream)) return rc;
    HIP_TRY(hipEventRecord(ev1.get(), stream));
    HIP_TRY(hipDeviceSynchronize());
    if (stats) {
        float ms = 0;
        HIP_TRY(hipEventElapsedTime(&ms, ev0.get(), ev1.get()));
        stats->kernel_ms = ms;
        stats->samples = samples;
        stats->reserved |= uint32_t(std::min<uint64_t>(rounds, 0xFFFFu)) << 16;
    }
    if (out_spp) HIP_TRY(hipMemcpy(out_spp, d->rg_spp.p, npx * sizeof(uint32_t), hipMemcpyDeviceToHost));
    if (out_stderr_rgb) HIP_TRY(hipMemcpy(out_stderr_rgb, d->rg_stderr.p, npx * 3 * sizeof(double), hipMemcpyDeviceToHost));
    if (state_out)
        if (int rc = single_rank_state_out(p, a, cam, L, records.p, state_out)) return rc;
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
    if (state_in)
        if (int rc = refuse_state_misuse("render_adaptive_budget", true, *p, *a, cam, state_in, first_level)) return rc;
    if (int rc = validate(s, cam, p)) return rc;
    return adaptive_budget_render(s, cam, *p, *a, *b, state_in, state_out, out_linear_rgb, out_rgba8, out_spp, out_stderr_rgb, stats);
}

// Release what the library keeps for the life of the process (today: the RCCL communicator sets of rttnw_render_multi).  Scenes
// are the caller's (rttnw_scene_destroy).  Safe to call more than once and with renders finished; also runs at exit.
extern "C" void rttnw_shutdown(void) { rt::destroy_comms(); }
