// render_api.cpp — the extern "C" half of the device side of include/rttnw_hip.h: device state, validation and the single-GPU render entry points
// (render_multi.cpp has the node-wide renderer, render_adaptive_api.cpp the adaptive family beyond rttnw_render_adaptive).  Host code only; the kernels
// and their launch code live in render_f32.hip / render_f64.hip (render_common.hpp says why there are two).
// No CPU fallback: every entry point needs a HIP device.
#include "render_multi.hpp"
#include "bvh_build.hpp"

namespace rt {
int refuse_adaptive_misuse(const char* prefix, const rttnw_params* p, const rttnw_adaptive* a) {
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
int copy_image_out(const char* what, const DevBuf<uint8_t>& rgba, const DevBuf<uint8_t>& linear, uint32_t precision, size_t npx, uint8_t* out_rgba8,
                   double* out_linear, hipError_t e) {
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
