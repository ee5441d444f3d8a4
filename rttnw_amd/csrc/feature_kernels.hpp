// feature_kernels.hpp — rttnw_render_features (include/rttnw_hip.h has the contract): the first hit of every camera ray as feature
// buffers — albedo, normal, depth, coverage — for a denoiser or a compositor.  A template over the arithmetic type like the trace kernels,
// instantiated once per arithmetic build in translation units of its own (features_f32.hip, features_f64.hip, features_f64_strict.hip,
// each under the flags of the render unit of that build).
//
// The plain form: one lane owns one PIXEL and loops over its samples — bounce 0 of the render's own path (path_begin, world_hit with the
// keyed draws of bounce 0, shade), nothing else.  Lanes are laid out in the render's 8x8 tile order, so a wave is one tile and its
// primary rays are coherent; the traversal stack is the trace kernels' (LdsStack: 16 entries in LDS, the rest in a global strip).
// 256-thread blocks: 17 KB of LDS each, so LDS never limits occupancy; the kernel is a few milliseconds next to a render of hundreds.
#pragma once
#include "trace_kernels.hpp"
#include "feature_api.hpp"

namespace rt {
inline namespace RT_ARITH_NS {

constexpr int FEATURE_BLOCK = 256;
constexpr uint32_t FEATURE_CHANNELS = 8; // albedo r g b, normal x y z, depth, alpha

// a product kept as a value of its own: the contracted builds would otherwise fuse it into the sum it is added to (rt_core.hpp keep_rounded)
template <typename R> __device__ __forceinline__ R feature_rounded(R v) {
    asm volatile("" : "+v"(v));
    return v;
}

// Packed pixel p = tile * 64 + y * 8 + x (tile in the permuted order of a single rank) -> FEATURE_CHANNELS sample means.
template <typename R>
__global__ __launch_bounds__(FEATURE_BLOCK) void feature_kernel(SceneView<R> sc, CameraRec<R> cam, RenderConsts rc, R bg_r, R bg_g, R bg_b, R t_min,
                                                                R* __restrict__ packed, uint32_t n_pixels, int32_t* __restrict__ spill) {
    extern __shared__ int32_t lds_stack[];
    const uint32_t p = blockIdx.x * blockDim.x + threadIdx.x;
    if (p >= n_pixels) return;
    LdsStack<FEATURE_BLOCK> stack{(LdsIntPtr)(lds_stack + threadIdx.x), (GlobalIntPtr)(spill + p), gridDim.x * blockDim.x};
    uint32_t tx, ty;
    tile_unpermute(p >> 6, rc.div_tiles_x, tx, ty);
    const uint32_t px = tx * 8u + (p & 7u), row = ty * 8u + ((p >> 3) & 7u);
    R sum[FEATURE_CHANNELS] = {0, 0, 0, 0, 0, 0, 0, 0};
    if (px < rc.width && row < rc.height) {
        NoCounters cnt;
        for (uint32_t s = 0; s < rc.spp; ++s) { // ONE chain per channel, in sample order
            PathState<R> ps;
            path_begin(ps, cam, rc, px, row, s);
            HitRecord<R> rec;
            if (world_hit(sc, ps.ray, t_min, ps.key, 0u, rc.quirks, rec, stack, cnt)) {
                const R depth = feature_rounded(rec.t * magnitude(ps.ray.d));
                V3<R> att, emitted;
                const bool scattered = shade(sc, rec, ps.key, 0u, ps.ray, att, emitted, cnt);
                const V3<R> albedo = scattered ? att : emitted;
                sum[0] = sum[0] + albedo.x; sum[1] = sum[1] + albedo.y; sum[2] = sum[2] + albedo.z;
                sum[3] = sum[3] + rec.normal.x; sum[4] = sum[4] + rec.normal.y; sum[5] = sum[5] + rec.normal.z;
                sum[6] = sum[6] + depth;
                sum[7] = sum[7] + R(1);
            } else {
                sum[0] = sum[0] + bg_r; sum[1] = sum[1] + bg_g; sum[2] = sum[2] + bg_b;
            }
        }
        const R n = R(rc.spp);
        for (uint32_t c = 0; c < FEATURE_CHANNELS; ++c) sum[c] = sum[c] / n;
    }
    R* dst = packed + size_t(p) * FEATURE_CHANNELS;
    for (uint32_t c = 0; c < FEATURE_CHANNELS; ++c) dst[c] = sum[c];
}

// Packed feature records -> the four row-major, top-first maps, as doubles (untile_kernel's addressing for one rank).
template <typename R>
__global__ void feature_untile_kernel(const R* __restrict__ packed, double* __restrict__ albedo, double* __restrict__ normal, double* __restrict__ depth,
                                      double* __restrict__ alpha, uint32_t width, uint32_t height, uint32_t tiles_x) {
    const uint32_t x = blockIdx.x * blockDim.x + threadIdx.x, y = blockIdx.y * blockDim.y + threadIdx.y;
    if (x >= width || y >= height) return;
    const R* src = packed + (tile_permuted(x >> 3, y >> 3, tiles_x) * 64ull + ((y & 7u) << 3) + (x & 7u)) * FEATURE_CHANNELS;
    const unsigned long long o = (unsigned long long)y * width + x;
    for (uint32_t c = 0; c < 3u; ++c) {
        albedo[o * 3 + c] = double(src[c]);
        normal[o * 3 + c] = double(src[3u + c]);
    }
    depth[o] = double(src[6]);
    alpha[o] = double(src[7]);
}

// The feature pass with its maps left ON THE DEVICE (rttnw_render_features behind it copies them out; rttnw_render_adaptive_denoised filters with
// them round after round): `d_maps`, 8 * w * h doubles of the caller's on the scene's device — albedo w*h*3, normal w*h*3, depth w*h, alpha w*h,
// row-major, top row first.  The two launches run between d->ev0 and d->ev1 on `stream`, and the stream has finished on return (the packed records
// and the stack strip are this call's own).  Arguments were checked by the caller.
template <typename R>
int render_features_device_t(::rttnw_scene* s, const rttnw_camera_desc* cam, const rttnw_params* p, double* d_maps, hipStream_t stream) {
    DeviceState* d = s->device;
    const FlatScene* flat = nullptr;
    DeviceScene<R>* ds = nullptr;
    if (int rc = bind_scene<R>(s, d, flat, ds)) return rc;
    rttnw_tile_layout L;
    fill_layout(p->width, p->height, 1, L);
    const RenderConsts rc = base_consts(p, *flat, L); // (the caller has checked: one rank, no counters)

    const size_t npx = size_t(p->width) * p->height;
    const uint32_t n_pixels = L.pixels_per_rank;
    const uint32_t grid = (n_pixels + FEATURE_BLOCK - 1) / FEATURE_BLOCK;
    const size_t threads = size_t(grid) * FEATURE_BLOCK;
    const size_t extra = rc.stack_depth > LDS_STACK_ENTRIES ? rc.stack_depth - LDS_STACK_ENTRIES : 0;
    DevBuf<R> packed;
    DevBuf<int32_t> spill;
    HIP_TRY(packed.alloc(size_t(n_pixels) * FEATURE_CHANNELS));
    HIP_TRY(spill.alloc(threads * extra + threads)); // (+ threads: `spill + p` is a valid address for every lane even without extra entries)
    double *m_albedo = d_maps, *m_normal = d_maps + npx * 3, *m_depth = d_maps + npx * 6, *m_alpha = d_maps + npx * 7;

    const size_t lds = size_t(LDS_STACK_ENTRIES + 1) * FEATURE_BLOCK * sizeof(int32_t);
    HIP_TRY(hipEventRecord(d->ev0.get(), stream));
    hipLaunchKernelGGL(feature_kernel<R>, dim3(grid), dim3(FEATURE_BLOCK), lds, stream, ds->view, camera_of<R>(cam), rc, R(p->background[0]),
                       R(p->background[1]), R(p->background[2]), R(p->t_min), packed.p, n_pixels, spill.p);
    HIP_TRY(hipGetLastError());
    dim3 ublock(32, 8), ugrid((p->width + 31) / 32, (p->height + 7) / 8);
    hipLaunchKernelGGL(feature_untile_kernel<R>, ugrid, ublock, 0, stream, (const R*)packed.p, m_albedo, m_normal, m_depth, m_alpha, p->width, p->height,
                       L.tiles_x);
    HIP_TRY(hipGetLastError());
    HIP_TRY(hipEventRecord(d->ev1.get(), stream));
    HIP_TRY(hipStreamSynchronize(stream));
    return RTTNW_OK;
}

// rttnw_render_features: the pass above, then its maps to the caller's arrays and the stats
template <typename R>
int render_features_t(::rttnw_scene* s, const rttnw_camera_desc* cam, const rttnw_params* p, double* out_albedo, double* out_normal, double* out_depth,
                      double* out_alpha, rttnw_stats* stats) {
    DeviceState* d = s->device;
    HIP_TRY(hipSetDevice(d->device));
    const size_t npx = size_t(p->width) * p->height;
    DevBuf<double> maps; // albedo, normal, depth, alpha: 8 doubles per pixel
    HIP_TRY(maps.alloc(npx * 8));
    if (int rc = render_features_device_t<R>(s, cam, p, maps.p, nullptr)) return rc;
    HIP_TRY(hipDeviceSynchronize());
    const double *m_albedo = maps.p, *m_normal = maps.p + npx * 3, *m_depth = maps.p + npx * 6, *m_alpha = maps.p + npx * 7;
    if (out_albedo) HIP_TRY(hipMemcpy(out_albedo, m_albedo, npx * 3 * sizeof(double), hipMemcpyDeviceToHost));
    if (out_normal) HIP_TRY(hipMemcpy(out_normal, m_normal, npx * 3 * sizeof(double), hipMemcpyDeviceToHost));
    if (out_depth) HIP_TRY(hipMemcpy(out_depth, m_depth, npx * sizeof(double), hipMemcpyDeviceToHost));
    if (out_alpha) HIP_TRY(hipMemcpy(out_alpha, m_alpha, npx * sizeof(double), hipMemcpyDeviceToHost));
    if (stats) {
        const FlatScene* flat = nullptr;
        DeviceScene<R>* ds = nullptr;
        if (int rc = bind_scene<R>(s, d, flat, ds)) return rc; // (uploaded by the pass: this only names the lowering and its arrays)
        std::memset(stats, 0, sizeof(*stats));
        float ms = 0;
        HIP_TRY(hipEventElapsedTime(&ms, d->ev0.get(), d->ev1.get()));
        stats->kernel_ms = ms;
        stats->samples = uint64_t(npx) * p->spp;
        stats->rays = stats->samples;
        stats->n_nodes = flat->total_nodes4();
        stats->n_prims = flat->n_prims_in_bvh;
        stats->scene_bytes = uint32_t(std::min<size_t>(ds->bytes, 0xFFFFFFFFu));
    }
    return RTTNW_OK;
}

} // namespace RT_ARITH_NS
} // namespace rt
