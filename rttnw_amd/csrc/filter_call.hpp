// filter_call.hpp — the scaffold of a blocking image-filter call, "host arrays in, host arrays out": what the *_device wrappers of denoise.hip,
// nlm.hip, regress.hip, select.hip, temporal.hip, variance.hip, clamp.hip and probe.hip have in common around their kernels.  A wrapper reads
//     FilterCall fc;
//     if (int rc = fc.open("denoise_nlm", width, height)) return rc;
//     fc.upload(d_a, half_a, 3);  fc.alloc(d_out, 3);  ...             counts are ELEMENTS PER PIXEL
//     (kernel attributes, dynamic LDS: still in front of the clock)
//     if (int rc = fc.start()) return rc;
//     (the kernels, on fc.stream)
//     if (int rc = fc.finish(kernel_ms)) return rc;
//     fc.copy_out(out_linear_rgb, d_out, 3);  ...                       a NULL host pointer is skipped
//     return fc.rc;
// The first HIP failure is kept in `rc` behind the message "<call>: <step>: <hip's words>", and every later step does nothing: start() hands it
// back before any kernel is launched, the last line after the copies.  Host code of the HIP translation units only.
#pragma once
#include "render_common.hpp"

namespace rt {

struct FilterCall {
    static constexpr hipStream_t stream = nullptr; // the null stream: the kernels, the two events and the copies are ordered on it
    std::string at;                                // "<call>: "
    size_t npx = 0;                                // width * height
    Event ev0, ev1;                                // around the kernels: kernel_ms
    int rc = RTTNW_OK;

    int open(const char* call, uint32_t width, uint32_t height) {
        if (int no_device = require_device(call)) return rc = no_device;
        at = std::string(call) + ": ";
        npx = size_t(width) * height;
        note(create_event(ev0), "create_event");
        note(create_event(ev1), "create_event");
        return rc;
    }
    template <typename T> void upload(DevBuf<T>& b, const T* src, size_t per_pixel) {
        if (!rc) note(rt::upload(b, src, npx * per_pixel), "upload");
    }
    template <typename T> void alloc(DevBuf<T>& b, size_t per_pixel) {
        if (!rc) note(b.alloc(npx * per_pixel), "alloc");
    }
    int start() {
        if (!rc) note(hipEventRecord(ev0.get(), stream), "hipEventRecord");
        return rc;
    }
    // Behind the last kernel: the second event, the wait, and the time between the two events where the caller asked for it
    int finish(double* kernel_ms) {
        if (!rc) note(hipEventRecord(ev1.get(), stream), "hipEventRecord");
        if (!rc) note(hipDeviceSynchronize(), "hipDeviceSynchronize");
        float ms = 0;
        if (!rc && kernel_ms && !note(hipEventElapsedTime(&ms, ev0.get(), ev1.get()), "hipEventElapsedTime")) *kernel_ms = ms;
        return rc;
    }
    template <typename T> void copy_out(T* dst, const T* d_src, size_t per_pixel) {
        if (!rc && dst) note(hipMemcpy(dst, d_src, npx * per_pixel * sizeof(T), hipMemcpyDeviceToHost), "copy_out");
    }
    template <typename T> void copy_out(T* dst, const DevBuf<T>& b, size_t per_pixel) { copy_out(dst, static_cast<const T*>(b.p), per_pixel); }

    int note(hipError_t e, const char* step) {
        if (e != hipSuccess) {
            set_last_error(at + step + ": " + hipGetErrorString(e));
            rc = RTTNW_ERR_HIP;
        }
        return rc;
    }
};

// What rttnw_temporal_variance and rttnw_temporal_clamp stage alike: the frame, the history (uploaded only with one) and the six outputs of the
// accumulation and the estimate.
struct MomentBuffers {
    DevBuf<double> lin, normal, depth, alpha, plin, pm2, plen, pnormal, pdepth, palpha, out, m2, len, xy, var;
    DevBuf<uint8_t> rgba;

    void stage(FilterCall& fc, bool has_history, const double* linear_rgb, const double* normal_, const double* depth_, const double* alpha_,
               const double* prev_linear_rgb, const double* prev_moment2_rgb, const double* prev_length, const double* prev_normal, const double* prev_depth,
               const double* prev_alpha) {
        fc.upload(lin, linear_rgb, 3);
        fc.upload(normal, normal_, 3);
        fc.upload(depth, depth_, 1);
        fc.upload(alpha, alpha_, 1);
        if (has_history) {
            fc.upload(plin, prev_linear_rgb, 3);
            fc.upload(pm2, prev_moment2_rgb, 3);
            fc.upload(plen, prev_length, 1);
            fc.upload(pnormal, prev_normal, 3);
            fc.upload(pdepth, prev_depth, 1);
            fc.upload(palpha, prev_alpha, 1);
        }
        fc.alloc(out, 3);
        fc.alloc(m2, 3);
        fc.alloc(len, 1);
        fc.alloc(xy, 2);
        fc.alloc(var, 3);
        fc.alloc(rgba, 4);
    }
    void copy_out(FilterCall& fc, double* out_linear_rgb, uint8_t* out_rgba8, double* out_moment2_rgb, double* out_length, double* out_prev_xy,
                  double* out_variance_rgb) {
        fc.copy_out(out_linear_rgb, out, 3);
        fc.copy_out(out_rgba8, rgba, 4);
        fc.copy_out(out_moment2_rgb, m2, 3);
        fc.copy_out(out_length, len, 1);
        fc.copy_out(out_prev_xy, xy, 2);
        fc.copy_out(out_variance_rgb, var, 3);
    }
};

} // namespace rt
