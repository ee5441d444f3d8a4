// svgf.hip — rttnw_svgf_create / _destroy / _reset / _set_clamp / _clipped / _set_sampling / _samples / _push / _frame (include/rttnw_hip.h): the SVGF loop over a history that stays on the device,
// around the arithmetic of svgf.hpp, double throughout.  The handle owns every buffer from rttnw_svgf_create on; a frame call enqueues, on one
// stream and without allocating,
//   svgf_ingest_kernel      one thread per pixel, blocks of 32 x 8: the frame's colour — the trace's packed tiles (reals of the render's precision,
//                           tile * 64 + y * 8 + x, four reals a pixel: guided_raw_kernel's order) or the doubles rttnw_svgf_push uploaded — to
//                           row-major doubles, divided by the albedo with `demodulate`, and the per-channel "was divided" bytes
//   svgf_accumulate_kernel  one thread per pixel, blocks of 64 x 4 like variance_accumulate_kernel: the reprojection and the four taps once,
//                           M1, M2 and — with feedback — the colour over H on them; plain global loads, no LDS
//   variance_estimate_kernel (variance.hip) and the à-trous passes (denoise.hip) as they are, the feedback a tap of the pass loop
//   (with rttnw_svgf_set_clamp: clamp.hip's clamp_accumulate_kernel in svgf_accumulate_kernel's place, M1 and H clipped to the frame's interval)
//   svgf_emit_kernel        one thread per pixel: the result and the accumulation multiplied back, and the RGBA8
//   (with rttnw_svgf_set_sampling, in front of all that: probe.hip's probe_kernel over the frame's features and the state's, and per level of the
//   boost a list of 2x2 blocks — pixel_lists.hip — traced by render_tiles_t and written over the plain trace's pixels; one 8-byte copy per level)
//   (with rttnw_svgf_set_regress, and rttnw_svgf_push_halves / rttnw_svgf_halves beside it: svgf_ingest_halves_kernel over two halves — two traces
//   of p->spp / 2, or two uploaded images —, svgf_accumulate_halves_kernel with the half histories Ha and Hb on the taps in H's place, the estimate
//   as it is, regress.hip's kernels — regress_passes_device — in the à-trous passes' place over the two accumulated halves, and
//   svgf_emit_halves_kernel, which shows the mean of those halves as the accumulation)
// then waits once and copies out what the caller asked for.  No atomics.
#include "feature_api.hpp"
#include "render_multi.hpp"
#include "pixel_lists.hpp"
#include "svgf.hpp"

struct rttnw_svgf {
    int device = -1;
    uint32_t width = 0, height = 0;
    rttnw_svgf_params q = {};
    rt::VarianceParams vprm = {};
    rt::DenoiseParams dprm = {};
    bool has_state = false;
    int cur = 0; // maps[cur], m1[cur], m2[cur], len[cur] are the state; the other halves are written by the next call
    rttnw_camera_desc cam = {};
    rt::DevBuf<uint8_t> packed, flags, rgba, scratch_rgba;
    rt::DevBuf<double> raw, c, maps[2], m1[2], m2[2], len[2], hist, acc, xy, var, ones, fc[2], fv[2], out_lin, out_acc;
    rt::Event ev0, ev1;
    // rttnw_svgf_set_clamp: off by default.  `clipped` is allocated by the first set call; clipped_live: the last frame call ran with a clamp and wrote it
    bool clamp = false, clipped_live = false;
    rt::ClampParams kprm = {};
    rt::DevBuf<uint8_t> clipped;
    // rttnw_svgf_set_sampling: off by default.  The buffers are allocated by the first set call: the probe's length and multiplier maps, the level
    // mask and selection bytes, the list of 2x2 blocks with its scan, and the list passes' running sums (as large as the packed frame: every block
    // listed).  samples_live: the last frame call ran with sampling and wrote the maps; last_spp: the last frame call's p->spp (0 before any).
    bool sampling = false, samples_live = false;
    uint32_t last_spp = 0;
    rt::SamplingParams sprm = {};
    rt::DevBuf<double> s_len;
    rt::DevBuf<uint8_t> s_mult, s_mask, s_select, s_sums;
    rt::DevBuf<uint32_t> s_quads, s_scan;
    rt::Event ev2, ev3;
    // rttnw_svgf_set_regress: off by default.  The buffers are allocated by the set calls, each when a setting first needs it: the second half's
    // packed trace, the ingested halves ca / cb (rttnw_svgf_push_halves uploads into them), the accumulated halves ha / hb as ping-pong pairs beside
    // m1 / m2 (ha[cur], hb[cur] are the state), the doubled variance, and rttnw_denoise_regress's workspace.  halves_live: the last frame call ran
    // with the stage and wrote what rttnw_svgf_halves copies out.
    bool regress = false, halves_live = false;
    uint32_t variance_source = 0;
    rt::RegressParams gprm = {};
    rt::RegressPlan gplan = {};
    rt::DevBuf<uint8_t> packed_b, g_rgba, g_fit_a, g_fit_b;
    rt::DevBuf<double> ca, cb, ha[2], hb[2], var2, g_pair, g_fa, g_fb, g_out, g_err, g_fit;
    rt::DevBuf<rt::RegressRecord> g_rec;
};

namespace rt {
namespace {

// T: the reals the colour comes in; PACKED: the trace's tiles (four reals a pixel) or a row-major image (three)
template <typename T, bool PACKED>
__global__ void svgf_ingest_kernel(uint32_t width, uint32_t height, uint32_t tiles_x, uint32_t demodulate, const T* __restrict__ colour,
                                   const double* __restrict__ albedo, const double* __restrict__ alpha, double* __restrict__ out_raw,
                                   double* __restrict__ out_c, uint8_t* __restrict__ out_flags) {
    const uint32_t x = blockIdx.x * blockDim.x + threadIdx.x, y = blockIdx.y * blockDim.y + threadIdx.y;
    if (x >= width || y >= height) return;
    const size_t p = size_t(y) * width + x;
    const T* src = PACKED ? colour + (tile_permuted(x >> 3, y >> 3, tiles_x) * 64ull + ((y & 7u) << 3) + (x & 7u)) * 4ull : colour + p * 3;
    const double a = alpha[p];
    for (int ch = 0; ch < 3; ++ch) {
        const double v = double(src[ch]);
        uint8_t divided;
        if (PACKED) out_raw[p * 3 + ch] = v;
        out_c[p * 3 + ch] = svgf_ingest_value(demodulate != 0u, v, albedo[p * 3 + ch], a, divided);
        out_flags[p * 3 + ch] = divided;
    }
}

__global__ __launch_bounds__(int(SVGF_BLOCK_X* SVGF_BLOCK_Y)) void svgf_accumulate_kernel(
    uint32_t width, uint32_t height, TemporalParams prm, uint32_t feedback, const double* __restrict__ linear, const double* __restrict__ normal,
    const double* __restrict__ depth, const double* __restrict__ alpha, const double* __restrict__ prev_moment1, const double* __restrict__ prev_moment2,
    const double* __restrict__ prev_history, const double* __restrict__ prev_length, const double* __restrict__ prev_normal,
    const double* __restrict__ prev_depth, const double* __restrict__ prev_alpha, double* __restrict__ out_moment1, double* __restrict__ out_moment2,
    double* __restrict__ out_acc, double* __restrict__ out_length, double* __restrict__ out_prev_xy) {
    const uint32_t x = blockIdx.x * SVGF_BLOCK_X + threadIdx.x, y = blockIdx.y * SVGF_BLOCK_Y + threadIdx.y;
    if (x >= width || y >= height) return;
    const SvgfAccumulated px = svgf_accumulate_pixel(width, height, x, y, prm, feedback != 0u, linear, normal, depth, alpha, prev_moment1, prev_moment2,
                                                     prev_history, prev_length, prev_normal, prev_depth, prev_alpha);
    const size_t p = size_t(y) * width + x;
    for (int ch = 0; ch < 3; ++ch) {
        out_moment1[p * 3 + ch] = px.m1[ch];
        out_moment2[p * 3 + ch] = px.m2[ch];
        out_acc[p * 3 + ch] = px.a[ch];
    }
    out_length[p] = px.length;
    out_prev_xy[p * 2] = px.xy[0];
    out_prev_xy[p * 2 + 1] = px.xy[1];
}

__global__ void svgf_emit_kernel(uint32_t n, const double* __restrict__ filtered, const double* __restrict__ accumulated, const double* __restrict__ albedo,
                                 const uint8_t* __restrict__ flags, double* __restrict__ out_linear, double* __restrict__ out_accumulated,
                                 uint8_t* __restrict__ out_rgba8) {
    const uint32_t i = blockIdx.x * blockDim.x + threadIdx.x; // one thread per pixel
    if (i >= n) return;
    const size_t o = size_t(i) * 3;
    for (int ch = 0; ch < 3; ++ch) {
        const double lin = svgf_emit_value(filtered[o + ch], albedo[o + ch], flags[o + ch]);
        out_linear[o + ch] = lin;
        out_accumulated[o + ch] = svgf_emit_value(accumulated[o + ch], albedo[o + ch], flags[o + ch]);
        out_rgba8[size_t(i) * 4 + ch] = denoise_quantise(lin);
    }
    out_rgba8[size_t(i) * 4 + 3] = 255;
}

// rttnw_svgf_set_regress's ingest: the two halves — two packed tile buffers of the trace, or the two row-major images rttnw_svgf_push_halves
// uploaded into out_ca / out_cb (each thread reads its pixel's values before it writes them: the arrays are not `__restrict__`) — to their mean
// C (out_raw), and C and both halves divided under the one rule: c, ca, cb.  The flags are C's, which are the halves' too: the rule reads the
// albedo and alpha only.
template <typename T, bool PACKED>
__global__ void svgf_ingest_halves_kernel(uint32_t width, uint32_t height, uint32_t tiles_x, uint32_t demodulate, const T* half_a, const T* half_b,
                                          const double* __restrict__ albedo, const double* __restrict__ alpha, double* __restrict__ out_raw,
                                          double* __restrict__ out_c, double* out_ca, double* out_cb, uint8_t* __restrict__ out_flags) {
    const uint32_t x = blockIdx.x * blockDim.x + threadIdx.x, y = blockIdx.y * blockDim.y + threadIdx.y;
    if (x >= width || y >= height) return;
    const size_t p = size_t(y) * width + x;
    const size_t s = PACKED ? (tile_permuted(x >> 3, y >> 3, tiles_x) * 64ull + ((y & 7u) << 3) + (x & 7u)) * 4ull : p * 3;
    const double a = alpha[p];
    double va[3], vb[3];
    for (int ch = 0; ch < 3; ++ch) {
        va[ch] = double(half_a[s + ch]);
        vb[ch] = double(half_b[s + ch]);
    }
    for (int ch = 0; ch < 3; ++ch) {
        const double mean = svgf_halves_mean(va[ch], vb[ch]), alb = albedo[p * 3 + ch];
        uint8_t divided, same;
        out_raw[p * 3 + ch] = mean;
        out_c[p * 3 + ch] = svgf_ingest_value(demodulate != 0u, mean, alb, a, divided);
        out_ca[p * 3 + ch] = svgf_ingest_value(demodulate != 0u, va[ch], alb, a, same);
        out_cb[p * 3 + ch] = svgf_ingest_value(demodulate != 0u, vb[ch], alb, a, same);
        out_flags[p * 3 + ch] = divided;
    }
}

// svgf_accumulate_kernel with the two half histories on the taps: five RGB planes gathered per tap (M1, M2, Ha, Hb and the state's normal), plain
// global loads, no LDS
__global__ __launch_bounds__(int(SVGF_BLOCK_X* SVGF_BLOCK_Y)) void svgf_accumulate_halves_kernel(
    uint32_t width, uint32_t height, TemporalParams prm, const double* __restrict__ linear, const double* __restrict__ half_a,
    const double* __restrict__ half_b, const double* __restrict__ normal, const double* __restrict__ depth, const double* __restrict__ alpha,
    const double* __restrict__ prev_moment1, const double* __restrict__ prev_moment2, const double* __restrict__ prev_half_a,
    const double* __restrict__ prev_half_b, const double* __restrict__ prev_length, const double* __restrict__ prev_normal,
    const double* __restrict__ prev_depth, const double* __restrict__ prev_alpha, double* __restrict__ out_moment1, double* __restrict__ out_moment2,
    double* __restrict__ out_half_a, double* __restrict__ out_half_b, double* __restrict__ out_length, double* __restrict__ out_prev_xy) {
    const uint32_t x = blockIdx.x * SVGF_BLOCK_X + threadIdx.x, y = blockIdx.y * SVGF_BLOCK_Y + threadIdx.y;
    if (x >= width || y >= height) return;
    const SvgfAccumulatedHalves px = svgf_accumulate_halves_pixel(width, height, x, y, prm, linear, half_a, half_b, normal, depth, alpha, prev_moment1,
                                                                  prev_moment2, prev_half_a, prev_half_b, prev_length, prev_normal, prev_depth, prev_alpha);
    const size_t p = size_t(y) * width + x;
    for (int ch = 0; ch < 3; ++ch) {
        out_moment1[p * 3 + ch] = px.m1[ch];
        out_moment2[p * 3 + ch] = px.m2[ch];
        out_half_a[p * 3 + ch] = px.a[ch];
        out_half_b[p * 3 + ch] = px.b[ch];
    }
    out_length[p] = px.length;
    out_prev_xy[p * 2] = px.xy[0];
    out_prev_xy[p * 2 + 1] = px.xy[1];
}

// svgf_emit_kernel behind the regression stage: the accumulation shown is the mean of the two accumulated halves
__global__ void svgf_emit_halves_kernel(uint32_t n, const double* __restrict__ filtered, const double* __restrict__ acc_a, const double* __restrict__ acc_b,
                                        const double* __restrict__ albedo, const uint8_t* __restrict__ flags, double* __restrict__ out_linear,
                                        double* __restrict__ out_accumulated, uint8_t* __restrict__ out_rgba8) {
    const uint32_t i = blockIdx.x * blockDim.x + threadIdx.x; // one thread per pixel
    if (i >= n) return;
    const size_t o = size_t(i) * 3;
    for (int ch = 0; ch < 3; ++ch) {
        const double lin = svgf_emit_value(filtered[o + ch], albedo[o + ch], flags[o + ch]);
        out_linear[o + ch] = lin;
        out_accumulated[o + ch] = svgf_emit_value(svgf_halves_mean(acc_a[o + ch], acc_b[o + ch]), albedo[o + ch], flags[o + ch]);
        out_rgba8[size_t(i) * 4 + ch] = denoise_quantise(lin);
    }
    out_rgba8[size_t(i) * 4 + 3] = 255;
}

// var + var, one sum: the variance of a half, which is a mean over half the samples of M1 (rttnw_svgf_set_regress, variance_source 0)
__global__ void svgf_half_variance_kernel(size_t n, const double* __restrict__ var, double* __restrict__ out) {
    const size_t i = size_t(blockIdx.x) * blockDim.x + threadIdx.x;
    if (i < n) out[i] = svgf_half_variance(var[i]);
}

__global__ void svgf_fill_kernel(size_t n, double value, double* __restrict__ out) {
    const size_t i = size_t(blockIdx.x) * blockDim.x + threadIdx.x;
    if (i < n) out[i] = value;
}

// What rttnw_temporal_variance, rttnw_temporal_accumulate and rttnw_denoise refuse for their parameter blocks, then the loop's own
int refuse_params(const char* call, const rttnw_svgf_params* q) {
    if (int rc = temporal_refuse_params(call, "q->t.", q->t)) return rc;
    if (int rc = variance_refuse_params(call, "q->v.", q->v)) return rc;
    if (int rc = denoise_refuse_params(call, "q->d.", q->d)) return rc;
    if (q->feedback_iterations > q->d.iterations) return refuse(call, "q->feedback_iterations is more than q->d.iterations");
    if (q->demodulate > 1) return refuse(call, "q->demodulate must be 0 or 1");
    if (q->reserved0 != 0) return refuse(call, "q->reserved0 must be 0");
    return 0;
}

// The reprojection of a frame seen through `cam` into the handle's state (none: a first frame)
TemporalParams svgf_temporal_params(const ::rttnw_svgf* g, const rttnw_camera_desc* cam) {
    return history_temporal_params(cam, g->has_state ? &g->cam : nullptr, g->q.t, false);
}

// A call on an existing handle: the handle's device made current until the caller returns, and the prefix of a HIP failure's message
struct OnHandleDevice {
    DeviceGuard restore;
    std::string at;
    int rc = RTTNW_OK; // RTTNW_ERR_HIP, the message set, where the device could not be made current
    OnHandleDevice(const char* call, const ::rttnw_svgf* g) : at(std::string(call) + ": ") {
        const hipError_t e = hipSetDevice(g->device);
        if (e == hipSuccess) return;
        set_last_error(at + "hipSetDevice(q->device): " + hipGetErrorString(e));
        rc = RTTNW_ERR_HIP;
    }
};

// An optional output of a call: nothing where the caller passed no array
hipError_t copy_out(void* dst, const void* src, size_t bytes) { return dst ? hipMemcpy(dst, src, bytes, hipMemcpyDeviceToHost) : hipSuccess; }

// The four feature planes of a pushed frame, host to maps[cur ^ 1] in rttnw_render_features' layout: albedo, normal, depth, alpha
int svgf_upload_features(const std::string& at, ::rttnw_svgf* g, const double* albedo, const double* normal, const double* depth, const double* alpha) {
    const size_t npx = size_t(g->width) * g->height, b3 = npx * 3 * sizeof(double), b1 = npx * sizeof(double);
    double* maps = g->maps[g->cur ^ 1].p;
    HIP_TRY_AS(at, hipMemcpy(maps, albedo, b3, hipMemcpyHostToDevice));
    HIP_TRY_AS(at, hipMemcpy(maps + npx * 3, normal, b3, hipMemcpyHostToDevice));
    HIP_TRY_AS(at, hipMemcpy(maps + npx * 6, depth, b1, hipMemcpyHostToDevice));
    HIP_TRY_AS(at, hipMemcpy(maps + npx * 7, alpha, b1, hipMemcpyHostToDevice));
    return RTTNW_OK;
}

// rttnw_svgf_set_sampling's steps 2 and 3 behind the plain trace of the frame (g->packed holds every pixel at p->spp) and the feature pass
// (maps[cur ^ 1]): the probe over the frame's features and the state's, then per level 2, 4, 8 up to the boost the mask {m == level}, its selection
// bytes, the list of 2x2 blocks over them — one 8-byte copy gives the host its length —, render_tiles_t over that list at level * p->spp and the
// selected pixels' records written over the plain trace's in g->packed.  A level nobody holds traces nothing.  `traced`: the samples of the list
// passes.  Everything on the null stream, between g->ev2 and g->ev3.
int svgf_boost_levels(const char* call, ::rttnw_svgf* g, ::rttnw_scene* s, const rttnw_camera_desc* cam, const rttnw_params* p, uint64_t& traced) {
    const std::string at = std::string(call) + ": ";
    const uint32_t w = g->width, h = g->height;
    const size_t npx = size_t(w) * h;
    const hipStream_t stream = nullptr;
    const double* maps = g->maps[g->cur ^ 1].p;
    const double* pmaps = g->maps[g->cur].p;
    rttnw_tile_layout L;
    fill_layout(w, h, 1, L);
    const uint32_t n_blocks = L.n_tiles * 16u;
    traced = 0;
    HIP_TRY_AS(at, hipSetDevice(g->device));
    HIP_TRY_AS(at, hipEventRecord(g->ev2.get(), stream));
    if (int rc = probe_enqueue_device(at.c_str(), w, h, svgf_temporal_params(g, cam), g->sprm, maps + npx * 3, maps + npx * 6, maps + npx * 7, g->len[g->cur].p,
                                      pmaps + npx * 3, pmaps + npx * 6, pmaps + npx * 7, g->s_len.p, nullptr, g->s_mult.p, stream)) return rc;
    for (uint32_t level = 2; level <= g->sprm.boost; level *= 2) {
        if (int rc = probe_level_mask_device(at.c_str(), uint32_t(npx), g->s_mult.p, level, g->s_mask.p, stream)) return rc;
        if (int rc = region_select_launch(w, h, 0, 1, g->s_mask.p, g->s_select.p, 0, 0, w, h, stream)) return rc;
        if (int rc = enqueue_quad_list(g->s_select.p, n_blocks, g->s_scan.p, g->s_quads.p, stream)) return rc;
        uint32_t count[2] = {0, 0}; // listed blocks, selected pixels
        HIP_TRY_AS(at, hipMemcpy(count, quad_list_totals(g->s_scan.p, n_blocks), sizeof(count), hipMemcpyDeviceToHost));
        if (count[0] == 0) continue;
        ListPass list;
        list.quads = g->s_quads.p;
        list.n_quads = count[0];
        rttnw_params pl = *p;
        pl.spp = level * p->spp;
        if (int rc = render_tiles_any(s, s->device, cam, &pl, g->s_sums.p, stream, nullptr, false, false, &list)) return rc;
        if (int rc = probe_scatter_device(at.c_str(), p->precision, g->s_sums.p, g->s_quads.p, list.n_quads, g->packed.p, stream)) return rc;
        traced += uint64_t(count[1]) * pl.spp;
    }
    HIP_TRY_AS(at, hipEventRecord(g->ev3.get(), stream));
    return RTTNW_OK;
}

// Steps 0 - 5 of the contract behind a frame whose features are in maps[cur ^ 1]: ingest (`packed`: the trace's tiles of `precision`, or the
// uploaded doubles), accumulate, estimate, filter with the tap, emit — enqueued between the handle's events —, the one wait, the outputs.
int svgf_run(const char* call, ::rttnw_svgf* g, const rttnw_camera_desc* cam, bool packed, uint32_t precision, const rttnw_svgf_out* out) {
    const std::string at = std::string(call) + ": ";
    const uint32_t w = g->width, h = g->height;
    const size_t npx = size_t(w) * h;
    const int nxt = g->cur ^ 1, old = g->cur;
    const hipStream_t stream = nullptr;
    double* maps = g->maps[nxt].p;
    const double *albedo = maps, *normal = maps + npx * 3, *depth = maps + npx * 6, *alpha = maps + npx * 7;
    const double* pmaps = g->maps[old].p;
    const bool feedback = g->q.feedback_iterations > 0 && g->has_state;

    const TemporalParams prm = svgf_temporal_params(g, cam);
    rttnw_tile_layout L;
    fill_layout(w, h, 1, L);

    HIP_TRY_AS(at, hipEventRecord(g->ev0.get(), stream));
    const dim3 block(32, 8), grid((w + 31) / 32, (h + 7) / 8);
    if (g->regress) { // the two halves: rttnw_svgf_push_halves uploaded them into ca / cb, rttnw_svgf_frame traced them into packed / packed_b
        if (!packed)
            hipLaunchKernelGGL((svgf_ingest_halves_kernel<double, false>), grid, block, 0, stream, w, h, L.tiles_x, g->q.demodulate, (const double*)g->ca.p,
                               (const double*)g->cb.p, albedo, alpha, g->raw.p, g->c.p, g->ca.p, g->cb.p, g->flags.p);
        else if (precision == RTTNW_F32)
            hipLaunchKernelGGL((svgf_ingest_halves_kernel<float, true>), grid, block, 0, stream, w, h, L.tiles_x, g->q.demodulate, (const float*)g->packed.p,
                               (const float*)g->packed_b.p, albedo, alpha, g->raw.p, g->c.p, g->ca.p, g->cb.p, g->flags.p);
        else
            hipLaunchKernelGGL((svgf_ingest_halves_kernel<double, true>), grid, block, 0, stream, w, h, L.tiles_x, g->q.demodulate, (const double*)g->packed.p,
                               (const double*)g->packed_b.p, albedo, alpha, g->raw.p, g->c.p, g->ca.p, g->cb.p, g->flags.p);
    } else if (!packed)
        hipLaunchKernelGGL((svgf_ingest_kernel<double, false>), grid, block, 0, stream, w, h, L.tiles_x, g->q.demodulate, (const double*)g->raw.p, albedo, alpha,
                           g->raw.p, g->c.p, g->flags.p);
    else if (precision == RTTNW_F32)
        hipLaunchKernelGGL((svgf_ingest_kernel<float, true>), grid, block, 0, stream, w, h, L.tiles_x, g->q.demodulate, (const float*)g->packed.p, albedo, alpha,
                           g->raw.p, g->c.p, g->flags.p);
    else
        hipLaunchKernelGGL((svgf_ingest_kernel<double, true>), grid, block, 0, stream, w, h, L.tiles_x, g->q.demodulate, (const double*)g->packed.p, albedo,
                           alpha, g->raw.p, g->c.p, g->flags.p);
    HIP_TRY_AS(at, hipGetLastError());

    const dim3 ablock(SVGF_BLOCK_X, SVGF_BLOCK_Y), agrid((w + SVGF_BLOCK_X - 1) / SVGF_BLOCK_X, (h + SVGF_BLOCK_Y - 1) / SVGF_BLOCK_Y);
    if (g->regress) { // steps 1 and 2 with Ha and Hb on the taps (the stage is exclusive with the clamp and with feedback)
        hipLaunchKernelGGL(svgf_accumulate_halves_kernel, agrid, ablock, 0, stream, w, h, prm, (const double*)g->c.p, (const double*)g->ca.p,
                           (const double*)g->cb.p, normal, depth, alpha, (const double*)g->m1[old].p, (const double*)g->m2[old].p, (const double*)g->ha[old].p,
                           (const double*)g->hb[old].p, (const double*)g->len[old].p, pmaps + npx * 3, pmaps + npx * 6, pmaps + npx * 7, g->m1[nxt].p,
                           g->m2[nxt].p, g->ha[nxt].p, g->hb[nxt].p, g->len[nxt].p, g->xy.p);
        HIP_TRY_AS(at, hipGetLastError());
    } else if (g->clamp) { // steps 1 and 2 through rttnw_temporal_clamp's kernel (clamp.hip): M1 and H clipped into the frame's interval on the same taps
        if (int rc = clamp_accumulate_device(at.c_str(), w, h, prm, g->kprm, feedback, g->c.p, normal, depth, alpha, g->m1[old].p, g->m2[old].p, g->hist.p,
                                             g->len[old].p, pmaps + npx * 3, pmaps + npx * 6, pmaps + npx * 7, g->m1[nxt].p, nullptr, g->m2[nxt].p, g->acc.p,
                                             g->len[nxt].p, g->xy.p, nullptr, nullptr, g->clipped.p, stream)) return rc;
    } else {
        hipLaunchKernelGGL(svgf_accumulate_kernel, agrid, ablock, 0, stream, w, h, prm, feedback ? 1u : 0u, (const double*)g->c.p, normal, depth, alpha,
                           (const double*)g->m1[old].p, (const double*)g->m2[old].p, (const double*)g->hist.p, (const double*)g->len[old].p, pmaps + npx * 3,
                           pmaps + npx * 6, pmaps + npx * 7, g->m1[nxt].p, g->m2[nxt].p, g->acc.p, g->len[nxt].p, g->xy.p);
        HIP_TRY_AS(at, hipGetLastError());
    }
    g->clipped_live = g->clamp;
    g->halves_live = g->regress;

    if (int rc = variance_passes_device(at.c_str(), w, h, nullptr, g->vprm, nullptr, normal, depth, alpha, nullptr, nullptr, nullptr, nullptr, nullptr, nullptr,
                                        g->m1[nxt].p, nullptr, g->m2[nxt].p, g->len[nxt].p, nullptr, g->var.p, stream)) return rc;

    const double* filter_albedo = g->q.demodulate ? g->ones.p : albedo;
    double* const fc[2] = {g->fc[0].p, g->fc[1].p};
    double* const fv[2] = {g->fv[0].p, g->fv[1].p};
    int fo = 0;
    const double* filtered_variance = nullptr;
    if (g->regress) { // step 3 is rttnw_denoise_regress over the accumulated halves, F.albedo a regressor; step 5 shows the mean of the halves
        const size_t n3 = npx * 3;
        double* half_var = nullptr; // variance_source 1: the filter's own pair variance
        if (g->variance_source == 0u) {
            half_var = g->var2.p;
            hipLaunchKernelGGL(svgf_half_variance_kernel, dim3(uint32_t((n3 + 255) / 256)), dim3(256), 0, stream, n3, (const double*)g->var.p, half_var);
        }
        const RegressWork work{nullptr, nullptr, nullptr, nullptr, g->g_pair.p, g->g_rec.p, g->g_fa.p, g->g_fb.p, g->g_fit_a.p, g->g_fit_b.p, g->g_out.p,
                               g->g_rgba.p, g->g_err.p, g->g_fit.p};
        if (int rc = regress_passes_device(at.c_str(), w, h, g->ha[nxt].p, g->hb[nxt].p, half_var, half_var, albedo, normal, depth, alpha, g->gprm, g->gplan,
                                           work, stream)) return rc;
        hipLaunchKernelGGL(svgf_emit_halves_kernel, dim3((uint32_t(npx) + 255u) / 256u), dim3(256), 0, stream, uint32_t(npx), (const double*)g->g_out.p,
                           (const double*)g->ha[nxt].p, (const double*)g->hb[nxt].p, albedo, (const uint8_t*)g->flags.p, g->out_lin.p, g->out_acc.p, g->rgba.p);
        filtered_variance = g->g_err.p;
    } else {
        if (int rc = atrous_passes_tap_device(w, h, g->acc.p, g->var.p, filter_albedo, normal, depth, alpha, g->q.d.iterations, g->dprm, fc, fv, g->scratch_rgba.p,
                                              g->q.feedback_iterations, g->q.feedback_iterations ? g->hist.p : nullptr, stream, fo)) return rc;

        hipLaunchKernelGGL(svgf_emit_kernel, dim3((uint32_t(npx) + 255u) / 256u), dim3(256), 0, stream, uint32_t(npx), (const double*)fc[fo], (const double*)g->acc.p,
                           albedo, (const uint8_t*)g->flags.p, g->out_lin.p, g->out_acc.p, g->rgba.p);
        filtered_variance = fv[fo];
    }
    HIP_TRY_AS(at, hipGetLastError());
    HIP_TRY_AS(at, hipEventRecord(g->ev1.get(), stream));
    HIP_TRY_AS(at, hipStreamSynchronize(stream));

    // the state is the frame's from here on
    g->cur = nxt;
    g->has_state = true;
    g->cam = *cam;
    if (!out) return RTTNW_OK;
    const size_t b3 = npx * 3 * sizeof(double), b1 = npx * sizeof(double);
    HIP_TRY_AS(at, copy_out(out->linear_rgb, g->out_lin.p, b3));
    HIP_TRY_AS(at, copy_out(out->rgba8, g->rgba.p, npx * 4));
    HIP_TRY_AS(at, copy_out(out->accumulated_rgb, g->out_acc.p, b3));
    HIP_TRY_AS(at, copy_out(out->variance_rgb, g->var.p, b3));
    HIP_TRY_AS(at, copy_out(out->filtered_variance_rgb, filtered_variance, b3));
    HIP_TRY_AS(at, copy_out(out->length, g->len[nxt].p, b1));
    HIP_TRY_AS(at, copy_out(out->prev_xy, g->xy.p, b1 * 2));
    HIP_TRY_AS(at, copy_out(out->moment1_rgb, g->m1[nxt].p, b3));
    HIP_TRY_AS(at, copy_out(out->moment2_rgb, g->m2[nxt].p, b3));
    HIP_TRY_AS(at, copy_out(out->history_rgb, g->q.feedback_iterations ? g->hist.p : g->m1[nxt].p, b3));
    HIP_TRY_AS(at, copy_out(out->raw_rgb, g->raw.p, b3));
    HIP_TRY_AS(at, copy_out(out->albedo, albedo, b3));
    HIP_TRY_AS(at, copy_out(out->normal, normal, b3));
    HIP_TRY_AS(at, copy_out(out->depth, depth, b1));
    HIP_TRY_AS(at, copy_out(out->alpha, alpha, b1));
    if (out->image_ms) {
        float ms = 0;
        HIP_TRY_AS(at, hipEventElapsedTime(&ms, g->ev0.get(), g->ev1.get()));
        *out->image_ms = ms;
    }
    return RTTNW_OK;
}

int svgf_allocate(::rttnw_svgf* g) {
    const char* const at = "svgf_create: ";
    const size_t npx = size_t(g->width) * g->height;
    rttnw_tile_layout L;
    fill_layout(g->width, g->height, 1, L);
    HIP_TRY_AS(at, hipGetDevice(&g->device));
    HIP_TRY_AS(at, g->packed.alloc(size_t(L.pixels_per_rank) * 4 * sizeof(double)));
    HIP_TRY_AS(at, g->flags.alloc(npx * 3));
    HIP_TRY_AS(at, g->rgba.alloc(npx * 4));
    HIP_TRY_AS(at, g->scratch_rgba.alloc(npx * 4));
    for (DevBuf<double>* b : {&g->raw, &g->c, &g->m1[0], &g->m1[1], &g->m2[0], &g->m2[1], &g->hist, &g->acc, &g->var, &g->ones, &g->fc[0], &g->fc[1], &g->fv[0],
                              &g->fv[1], &g->out_lin, &g->out_acc})
        HIP_TRY_AS(at, b->alloc(npx * 3));
    for (int k = 0; k < 2; ++k) {
        HIP_TRY_AS(at, g->maps[k].alloc(npx * 8));
        HIP_TRY_AS(at, g->len[k].alloc(npx));
    }
    HIP_TRY_AS(at, g->xy.alloc(npx * 2));
    HIP_TRY_AS(at, create_event(g->ev0));
    HIP_TRY_AS(at, create_event(g->ev1));
    hipLaunchKernelGGL(svgf_fill_kernel, dim3(uint32_t((npx * 3 + 255) / 256)), dim3(256), 0, nullptr, npx * 3, 1.0, g->ones.p);
    HIP_TRY_AS(at, hipGetLastError());
    if (int rc = variance_admit_lds(at, g->vprm.radius)) return rc;
    HIP_TRY_AS(at, hipDeviceSynchronize());
    return RTTNW_OK;
}

} // namespace
} // namespace rt

extern "C" {

int rttnw_svgf_create(uint32_t width, uint32_t height, const rttnw_svgf_params* q, rttnw_svgf** out) {
    const char* const call = "svgf_create";
    if (!q) return rt::refuse(call, "q is NULL");
    if (!out) return rt::refuse(call, "out is NULL");
    *out = nullptr;
    if (int rc = rt::image_size_refused(call, width, height)) return rc;
    if (int rc = rt::refuse_params(call, q)) return rc;
    if (int rc = rt::require_device(call)) return rc;
    std::unique_ptr<rttnw_svgf> g(new rttnw_svgf());
    g->width = width;
    g->height = height;
    g->q = *q;
    g->vprm = rt::variance_params(q->v.min_temporal, q->v.radius, q->v.sigma_normal, q->v.sigma_depth);
    g->dprm = rt::denoise_params(q->d.sigma_luminance, q->d.sigma_normal, q->d.sigma_depth, true);
    if (int rc = rt::svgf_allocate(g.get())) return rc;
    *out = g.release();
    return RTTNW_OK;
}

void rttnw_svgf_destroy(rttnw_svgf* q) {
    if (!q) return;
    rt::DeviceGuard restore;
    (void)hipSetDevice(q->device);
    (void)hipDeviceSynchronize();
    delete q;
}

int rttnw_svgf_reset(rttnw_svgf* q) {
    if (!q) return rt::refuse("svgf_reset", "q is NULL");
    q->has_state = false;
    return RTTNW_OK;
}

int rttnw_svgf_set_clamp(rttnw_svgf* q, const rttnw_clamp_params* k) {
    const char* const call = "svgf_set_clamp";
    if (k)
        if (int rc = rt::clamp_refuse_params(call, k)) return rc;
    if (!q) return rt::refuse(call, "q is NULL");
    if (!k) {
        q->clamp = false;
        return RTTNW_OK;
    }
    if (q->regress) return rt::refuse(call, "q: the handle has a regression stage (rttnw_svgf_set_regress), which is exclusive with a clamp");
    if (!q->clipped.p) { // the one byte map, once: frame calls still allocate nothing
        const rt::OnHandleDevice on(call, q);
        if (on.rc) return on.rc;
        HIP_TRY_AS(on.at, q->clipped.alloc(size_t(q->width) * q->height));
    }
    q->kprm = rt::clamp_params(k->radius, k->gamma, k->sigma_normal, k->sigma_depth);
    q->clamp = true;
    return RTTNW_OK;
}

int rttnw_svgf_clipped(rttnw_svgf* q, uint8_t* out_clipped) {
    const char* const call = "svgf_clipped";
    if (!out_clipped) return rt::refuse(call, "out_clipped is NULL");
    if (!q) return rt::refuse(call, "q is NULL");
    const size_t npx = size_t(q->width) * q->height;
    if (!q->clipped_live) { // before any frame call, or after one without a clamp
        std::memset(out_clipped, 0, npx);
        return RTTNW_OK;
    }
    const rt::OnHandleDevice on(call, q);
    if (on.rc) return on.rc;
    HIP_TRY_AS(on.at, hipMemcpy(out_clipped, q->clipped.p, npx, hipMemcpyDeviceToHost));
    return RTTNW_OK;
}

int rttnw_svgf_set_sampling(rttnw_svgf* q, const rttnw_sampling_params* a) {
    const char* const call = "svgf_set_sampling";
    if (a)
        if (int rc = rt::sampling_refuse_params(call, a)) return rc;
    if (!q) return rt::refuse(call, "q is NULL");
    if (!a) {
        q->sampling = false;
        return RTTNW_OK;
    }
    if (q->regress) return rt::refuse(call, "q: the handle has a regression stage (rttnw_svgf_set_regress), which is exclusive with sampling");
    if (!q->s_mult.p) { // the maps, the list and the list passes' sums, once: frame calls still allocate none of the handle's buffers
        const size_t npx = size_t(q->width) * q->height;
        rttnw_tile_layout L;
        rt::fill_layout(q->width, q->height, 1, L);
        const uint32_t n_blocks = L.n_tiles * 16u;
        const rt::OnHandleDevice on(call, q);
        if (on.rc) return on.rc;
        const std::string& at = on.at;
        HIP_TRY_AS(at, q->s_len.alloc(npx));
        HIP_TRY_AS(at, q->s_mask.alloc(npx));
        HIP_TRY_AS(at, q->s_select.alloc(L.pixels_per_rank));
        HIP_TRY_AS(at, q->s_quads.alloc(n_blocks));
        HIP_TRY_AS(at, q->s_scan.alloc(rt::quad_scan_words(n_blocks)));
        HIP_TRY_AS(at, q->s_sums.alloc(size_t(L.pixels_per_rank) * 4 * sizeof(double)));
        HIP_TRY_AS(at, rt::create_event(q->ev2));
        HIP_TRY_AS(at, rt::create_event(q->ev3));
        HIP_TRY_AS(at, q->s_mult.alloc(npx)); // (last: its presence says that all of them are there)
    }
    q->sprm = rt::sampling_params(a->boost, a->fill);
    q->sampling = true;
    return RTTNW_OK;
}

int rttnw_svgf_samples(rttnw_svgf* q, uint32_t* out_spp, double* out_length) {
    const char* const call = "svgf_samples";
    if (!q) return rt::refuse(call, "q is NULL");
    const size_t npx = size_t(q->width) * q->height;
    if (!q->samples_live) { // before any frame call (last_spp is 0), or after one without sampling: every pixel got p->spp, no length was probed
        if (out_spp) std::fill(out_spp, out_spp + npx, q->last_spp);
        if (out_length) std::fill(out_length, out_length + npx, 0.0);
        return RTTNW_OK;
    }
    const rt::OnHandleDevice on(call, q);
    if (on.rc) return on.rc;
    const std::string& at = on.at;
    if (out_spp) {
        std::vector<uint8_t> m(npx);
        HIP_TRY_AS(at, hipMemcpy(m.data(), q->s_mult.p, npx, hipMemcpyDeviceToHost));
        for (size_t i = 0; i < npx; ++i) out_spp[i] = uint32_t(m[i]) * q->last_spp;
    }
    if (out_length) HIP_TRY_AS(at, hipMemcpy(out_length, q->s_len.p, npx * sizeof(double), hipMemcpyDeviceToHost));
    return RTTNW_OK;
}

int rttnw_svgf_push(rttnw_svgf* q, const rttnw_camera_desc* cam, const double* linear_rgb, const double* albedo, const double* normal, const double* depth,
                    const double* alpha, const rttnw_svgf_out* out) {
    const char* const call = "svgf_push";
    // (the handle last: a handle exists only on a machine with a device, and the other refusals need none)
    if (!cam) return rt::refuse(call, "cam is NULL");
    if (!linear_rgb) return rt::refuse(call, "linear_rgb is NULL");
    if (!albedo || !normal || !depth || !alpha) return rt::refuse(call, "NULL argument (albedo, normal, depth or alpha)");
    if (!q) return rt::refuse(call, "q is NULL");
    if (q->regress) return rt::refuse(call, "q: the handle has a regression stage (rttnw_svgf_set_regress): it takes rttnw_svgf_push_halves");
    const rt::OnHandleDevice on(call, q);
    if (on.rc) return on.rc;
    const std::string& at = on.at;
    const size_t b3 = size_t(q->width) * q->height * 3 * sizeof(double);
    HIP_TRY_AS(at, hipMemcpy(q->raw.p, linear_rgb, b3, hipMemcpyHostToDevice));
    if (int rc = rt::svgf_upload_features(at, q, albedo, normal, depth, alpha)) return rc;
    return rt::svgf_run(call, q, cam, false, RTTNW_F64, out);
}

int rttnw_svgf_set_regress(rttnw_svgf* q, const rttnw_regress_params* g, uint32_t variance_source) {
    const char* const call = "svgf_set_regress";
    if (g) {
        if (int rc = rt::regress_refuse_params(call, g)) return rc;
        if (g->demodulate != 0) return rt::refuse(call, "g->demodulate must be 0: the handle's own demodulate does that job");
        if (variance_source > 1) return rt::refuse(call, "variance_source must be 0 (the temporal estimate) or 1 (the filter's pair variance)");
    }
    if (!q) return rt::refuse(call, "q is NULL");
    if (!g) {
        if (!q->regress) return RTTNW_OK; // nothing to clear: the history stays
        q->regress = q->halves_live = false;
        q->has_state = false;
        return RTTNW_OK;
    }
    if (q->q.feedback_iterations != 0 || q->clamp || q->sampling)
        return rt::refuse(call, "q: the regression stage is exclusive with feedback_iterations != 0, a clamp (rttnw_svgf_set_clamp) and sampling (rttnw_svgf_set_sampling)");
    const rt::RegressParams prm = rt::regress_params(g->search_radius, g->patch_radius, g->k, g->ridge, g->features, 0);
    const rt::OnHandleDevice on(call, q);
    if (on.rc) return on.rc;
    const std::string& at = on.at;
    const size_t npx = size_t(q->width) * q->height;
    rttnw_tile_layout L;
    rt::fill_layout(q->width, q->height, 1, L);
    // every buffer the stage needs under these settings, each once: frame calls still allocate nothing
    if (!q->packed_b.p) HIP_TRY_AS(at, q->packed_b.alloc(size_t(L.pixels_per_rank) * 4 * sizeof(double)));
    for (rt::DevBuf<double>* b : {&q->ca, &q->cb, &q->ha[0], &q->ha[1], &q->hb[0], &q->hb[1], &q->g_fa, &q->g_fb, &q->g_out, &q->g_err})
        if (!b->p) HIP_TRY_AS(at, b->alloc(npx * 3));
    rt::DevBuf<double>& half_var = variance_source == 0u ? q->var2 : q->g_pair;
    if (!half_var.p) HIP_TRY_AS(at, half_var.alloc(npx * 3));
    if (!q->g_fit.p) HIP_TRY_AS(at, q->g_fit.alloc(npx));
    if (!q->g_rgba.p) HIP_TRY_AS(at, q->g_rgba.alloc(npx * 4));
    if (!q->g_fit_a.p) HIP_TRY_AS(at, q->g_fit_a.alloc(npx));
    if (!q->g_fit_b.p) HIP_TRY_AS(at, q->g_fit_b.alloc(npx));
    if (prm.features != 0u && !q->g_rec.p) HIP_TRY_AS(at, q->g_rec.alloc(npx));
    rt::RegressPlan plan;
    if (int rc = rt::regress_plan_device(at.c_str(), prm, plan)) return rc; // the filter kernel's dynamic LDS, admitted here
    q->gprm = prm;
    q->gplan = plan;
    q->variance_source = variance_source;
    q->regress = true;
    q->halves_live = false;
    q->has_state = false; // as rttnw_svgf_reset: a history without Ha and Hb is none
    return RTTNW_OK;
}

int rttnw_svgf_push_halves(rttnw_svgf* q, const rttnw_camera_desc* cam, const double* half_a, const double* half_b, const double* albedo,
                           const double* normal, const double* depth, const double* alpha, const rttnw_svgf_out* out) {
    const char* const call = "svgf_push_halves";
    // rttnw_svgf_push's checks, half_a and half_b where linear_rgb stood
    if (!cam) return rt::refuse(call, "cam is NULL");
    if (!half_a || !half_b) return rt::refuse(call, "NULL argument (half_a or half_b)");
    if (!albedo || !normal || !depth || !alpha) return rt::refuse(call, "NULL argument (albedo, normal, depth or alpha)");
    if (!q) return rt::refuse(call, "q is NULL");
    if (!q->regress) return rt::refuse(call, "q: the handle has no regression stage (rttnw_svgf_set_regress): it takes rttnw_svgf_push");
    const rt::OnHandleDevice on(call, q);
    if (on.rc) return on.rc;
    const std::string& at = on.at;
    const size_t b3 = size_t(q->width) * q->height * 3 * sizeof(double);
    HIP_TRY_AS(at, hipMemcpy(q->ca.p, half_a, b3, hipMemcpyHostToDevice));
    HIP_TRY_AS(at, hipMemcpy(q->cb.p, half_b, b3, hipMemcpyHostToDevice));
    if (int rc = rt::svgf_upload_features(at, q, albedo, normal, depth, alpha)) return rc;
    return rt::svgf_run(call, q, cam, false, RTTNW_F64, out);
}

int rttnw_svgf_halves(rttnw_svgf* q, double* out_acc_a, double* out_acc_b, double* out_filtered_a, double* out_filtered_b, double* out_fit) {
    const char* const call = "svgf_halves";
    if (!q) return rt::refuse(call, "q is NULL");
    const size_t npx = size_t(q->width) * q->height;
    if (!q->halves_live) { // before any frame call with the stage, or after the stage was set anew or cleared
        for (double* o : {out_acc_a, out_acc_b, out_filtered_a, out_filtered_b})
            if (o) std::fill(o, o + npx * 3, 0.0);
        if (out_fit) std::fill(out_fit, out_fit + npx, 0.0);
        return RTTNW_OK;
    }
    const rt::OnHandleDevice on(call, q);
    if (on.rc) return on.rc;
    const std::string& at = on.at;
    const size_t b3 = npx * 3 * sizeof(double);
    HIP_TRY_AS(at, rt::copy_out(out_acc_a, q->ha[q->cur].p, b3)); // (the last frame call's Aa and Ab are the state's Ha and Hb)
    HIP_TRY_AS(at, rt::copy_out(out_acc_b, q->hb[q->cur].p, b3));
    HIP_TRY_AS(at, rt::copy_out(out_filtered_a, q->g_fa.p, b3));
    HIP_TRY_AS(at, rt::copy_out(out_filtered_b, q->g_fb.p, b3));
    HIP_TRY_AS(at, rt::copy_out(out_fit, q->g_fit.p, npx * sizeof(double)));
    return RTTNW_OK;
}

int rttnw_svgf_frame(rttnw_svgf* q, rttnw_scene* s, const rttnw_camera_desc* cam, const rttnw_params* p, const rttnw_svgf_out* out, rttnw_stats* stats) {
    const char* const call = "svgf_frame";
    if (!cam) return rt::refuse(call, "cam is NULL");
    if (!p) return rt::refuse(call, "p is NULL");
    if (int rc = rt::refuse_host_output_misuse(call, p->reserved0, p)) return rc; // tile_world != 1 among them
    if (!q) return rt::refuse(call, "q is NULL");
    if (!s) return rt::refuse(call, "s is NULL");
    if (p->width != q->width || p->height != q->height) return rt::refuse(call, "p->width and p->height must equal the handle's");
    // with sampling a pixel may get boost * p->spp samples: that product must be a spp rttnw_render takes
    const bool boosted = q->sampling; // (a boost of 1 still probes: rttnw_svgf_samples returns the lengths)
    if (boosted && uint64_t(q->sprm.boost) * p->spp > 0xFFFFFFFFull) return rt::refuse(call, "p->spp times the handle's boost (rttnw_svgf_set_sampling) is more than a render's spp can be");
    // with a regression stage the frame is traced as two halves of p->spp / 2 samples
    if (q->regress && (p->spp < 2u || p->spp % 2u != 0u)) return rt::refuse(call, "p->spp must be even and at least 2 on a handle with a regression stage (rttnw_svgf_set_regress): two halves of p->spp / 2");
    if (int rc = rt::validate(s, cam, p)) return rc;
    if (s->device->device != q->device) return rt::refuse(call, "s: the scene was committed on another device than the handle's");
    rttnw_params pf = *p;
    pf.spp = q->q.feature_spp ? q->q.feature_spp : (p->spp < 16u ? p->spp : 16u);
    rt::DeviceGuard restore;
    uint64_t boost_samples = 0;
    if (q->regress) { // the two halves, disjoint sample ranges, then the feature pass as without the stage; `stats` sums the two traces
        rttnw_params pa = *p, pb = *p;
        pa.spp = pb.spp = p->spp / 2u;
        pb.sample_begin = p->sample_begin + p->spp / 2u;
        rttnw_stats sb = {};
        if (int rc = rt::render_tiles_any(s, s->device, cam, &pa, q->packed.p, nullptr, stats)) return rc;
        if (int rc = rt::render_tiles_any(s, s->device, cam, &pb, q->packed_b.p, nullptr, stats ? &sb : nullptr)) return rc;
        if (stats) {
            stats->samples += sb.samples;
            stats->rays += sb.rays;
            stats->nodes_visited += sb.nodes_visited;
            stats->prims_tested += sb.prims_tested;
            stats->texel_fetches += sb.texel_fetches;
            stats->kernel_ms += sb.kernel_ms;
        }
        if (int rc = RT_BY_PRECISION(p->precision, render_features_device_t, s, cam, &pf, q->maps[q->cur ^ 1].p, nullptr)) return rc;
    } else if (!boosted) {
        if (int rc = rt::render_tiles_any(s, s->device, cam, p, q->packed.p, nullptr, stats)) return rc;
        if (int rc = RT_BY_PRECISION(p->precision, render_features_device_t, s, cam, &pf, q->maps[q->cur ^ 1].p, nullptr)) return rc;
    } else {
        // the feature pass first — it does not depend on the trace —, then the plain trace of every pixel, then the boosted levels over it
        if (int rc = RT_BY_PRECISION(p->precision, render_features_device_t, s, cam, &pf, q->maps[q->cur ^ 1].p, nullptr)) return rc;
        if (int rc = rt::render_tiles_any(s, s->device, cam, p, q->packed.p, nullptr, stats)) return rc;
        if (int rc = rt::svgf_boost_levels(call, q, s, cam, p, boost_samples)) return rc;
    }
    q->samples_live = boosted;
    q->last_spp = p->spp;
    if (stats) {
        const uint64_t feature_rays = uint64_t(p->width) * p->height * pf.spp;
        stats->samples += feature_rays + boost_samples;
        stats->rays += feature_rays;
    }
    const int rc = rt::svgf_run(call, q, cam, true, p->precision, out);
    if (rc == RTTNW_OK && boosted && stats) { // (svgf_run waited for the stream: both events are reached)
        float ms = 0;
        if (hipEventElapsedTime(&ms, q->ev2.get(), q->ev3.get()) == hipSuccess) stats->kernel_ms += ms;
    }
    return rc;
}

} // extern "C"
