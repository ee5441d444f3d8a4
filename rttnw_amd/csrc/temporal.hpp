// temporal.hpp — the arithmetic of rttnw_temporal_accumulate (include/rttnw_hip.h has the contract, DESIGN.md §10b the why), shared by the device
// kernel (temporal.hip) and the host test harness (tests/temporal_host): the temporal stage of SVGF (Schied et al. 2017) over a static scene.  The
// surface point behind a pixel is rebuilt from the camera record and the first-hit depth, projected into the previous frame's camera record, the
// previous frame's accumulated colour is gathered there through four bilinear taps, each kept only where depth and normal say "same surface", and
// blended with this frame as a running mean of at most max_history frames.
//
// Everything is double.  + - * /, sqrt, floor and comparisons only, every product through unfused_mul() (adaptive.hpp), the order of every sum
// fixed here, so the device code, a g++ host build and a numpy restatement produce the same bits (tests/test_temporal_cpu.py,
// tests/test_gpu_temporal.py):
//   dot(a, b) = (a0 b0 + a1 b1) + a2 b2
//   s = (x + 0.5) / w;  t = ((h - 1 - y) + 0.5) / h;  d = ((llc + s H) + t V) - o;  z = depth / alpha;  P = o + d * (z / sqrt(dot(d, d)))
//   q = P - o_p;  lambda = dot(e, n) / dot(q, n), n = H_p x V_p, e = llc_p - o_p;  r = lambda q - e
//   fx = (dot(r, H_p) / dot(H_p, H_p)) * w - 0.5;  fy = (h - (dot(r, V_p) / dot(V_p, V_p)) * h) - 0.5;  zq = sqrt(dot(q, q))
//   taps (floor(fx) + i, floor(fy) + j), i then j, weights (i ? ax : 1 - ax) * (j ? ay : 1 - ay); sums from 0.0 over the accepted taps in that order
//   temporal_taps:     tap k = 00, 10, 01, 11 kept where it is inside the image and temporal_accepts it;  W = sum wt;  SL = sum wt * length';
//                      blend = W > 0 — each sum a chain of its own over the kept taps, a tap not kept skipped
//   temporal_tap_sum:  S[ch] = sum wt * q'[ch] of one RGB quantity q of the previous frame, likewise;  its mean is S / W
//   temporal_blend:    L = SL / W;  N = min(L + 1, max_history);  a = 1 / N;  (1 - a)
//   out = (1 - a) * hist + a * cur;  out_var = ((1 - a)(1 - a)) * vh + (a a) * var
// The three functions are the one statement of the reprojected gather: variance.hpp, clamp.hpp, probe.hpp and svgf.hpp hang their quantities on them.
#pragma once
#include "denoise.hpp"

namespace rt {

constexpr uint32_t TEMPORAL_HISTORY_LIMIT = 65535;
// The library defaults (a 0 in rttnw_temporal_params)
constexpr uint32_t TEMPORAL_MAX_HISTORY = 32;
constexpr double TEMPORAL_DEPTH_TOLERANCE = 0.05, TEMPORAL_NORMAL_MIN = 0.9;

// The call's parameters with the defaults resolved, and what the geometry reads of the two camera records (Camera::new, camera.rs:32-61; the lens
// at its centre, no shutter time).  n, e and the three dot products are the same for every pixel: formed once, on the host, by the functions the
// pixels would have used.
struct TemporalParams {
    double o[3], llc[3], H[3], V[3];      // this frame's record
    double po[3], pH[3], pV[3];           // the previous frame's
    double n[3], e[3], en, hh, vv;        // H_p x V_p, llc_p - o_p, dot(e, n), dot(H_p, H_p), dot(V_p, V_p)
    double max_history, depth_tolerance, normal_min;
    uint32_t has_history, same_camera;    // same_camera: the two descriptors' 15 doubles are bitwise equal — the geometry is skipped
    uint32_t normal_test, has_variance;   // normal_test == 0: normal_min was -1
};

RT_HD double temporal_dot(const double* a, const double* b) { return (unfused_mul(a[0], b[0]) + unfused_mul(a[1], b[1])) + unfused_mul(a[2], b[2]); }
// false for an infinity and for a NaN
RT_HD bool temporal_finite(double v) { return v - v == 0.0; }

inline TemporalParams temporal_params(const CameraRec<double>& cur, const CameraRec<double>* prev, bool same_camera, uint32_t max_history, double depth_tolerance,
                                      double normal_min, bool has_variance) {
    TemporalParams q = {};
    for (int k = 0; k < 3; ++k) {
        q.o[k] = cur.origin[k];
        q.llc[k] = cur.lower_left_corner[k];
        q.H[k] = cur.horizontal[k];
        q.V[k] = cur.vertical[k];
    }
    q.has_history = prev != nullptr;
    q.same_camera = prev != nullptr && same_camera;
    if (prev) {
        for (int k = 0; k < 3; ++k) {
            q.po[k] = prev->origin[k];
            q.pH[k] = prev->horizontal[k];
            q.pV[k] = prev->vertical[k];
            q.e[k] = prev->lower_left_corner[k] - prev->origin[k];
        }
        q.n[0] = unfused_mul(q.pH[1], q.pV[2]) - unfused_mul(q.pH[2], q.pV[1]);
        q.n[1] = unfused_mul(q.pH[2], q.pV[0]) - unfused_mul(q.pH[0], q.pV[2]);
        q.n[2] = unfused_mul(q.pH[0], q.pV[1]) - unfused_mul(q.pH[1], q.pV[0]);
        q.en = temporal_dot(q.e, q.n);
        q.hh = temporal_dot(q.pH, q.pH);
        q.vv = temporal_dot(q.pV, q.pV);
    }
    q.max_history = double(max_history == 0 ? TEMPORAL_MAX_HISTORY : max_history);
    q.depth_tolerance = depth_tolerance == 0.0 ? TEMPORAL_DEPTH_TOLERANCE : depth_tolerance;
    q.normal_test = normal_min != -1.0;
    q.normal_min = normal_min == 0.0 ? TEMPORAL_NORMAL_MIN : normal_min;
    q.has_variance = has_variance;
    return q;
}

// Where pixel (x, y), whose samples hit at the mean distance z, was in the previous frame: (fx, fy) in that frame's pixel coordinates and zq, its
// distance from that frame's origin.  false: it was behind that camera or outside its image — no history.
RT_HD bool temporal_where(uint32_t w, uint32_t h, uint32_t x, uint32_t y, const TemporalParams& q, double z, double& fx, double& fy, double& zq) {
    if (q.same_camera) {
        fx = double(x);
        fy = double(y);
        zq = z;
        return true;
    }
    const double s = (double(x) + 0.5) / double(w), t = (double(h - 1u - y) + 0.5) / double(h);
    double d[3], v[3], r[3];
    for (int k = 0; k < 3; ++k) d[k] = ((q.llc[k] + unfused_mul(s, q.H[k])) + unfused_mul(t, q.V[k])) - q.o[k];
    const double scale = z / sqrt(temporal_dot(d, d));
    for (int k = 0; k < 3; ++k) v[k] = (q.o[k] + unfused_mul(d[k], scale)) - q.po[k]; // q of the contract: P - o_p
    const double lambda = q.en / temporal_dot(v, q.n);
    if (!(lambda > 0.0)) return false;
    for (int k = 0; k < 3; ++k) r[k] = unfused_mul(lambda, v[k]) - q.e[k];
    const double sp = temporal_dot(r, q.pH) / q.hh, tp = temporal_dot(r, q.pV) / q.vv;
    fx = unfused_mul(sp, double(w)) - 0.5;
    fy = (double(h) - unfused_mul(tp, double(h))) - 0.5;
    if (!temporal_finite(fx) || !temporal_finite(fy)) return false;
    if (!(fx > -1.0 && fx < double(w)) || !(fy > -1.0 && fy < double(h))) return false;
    zq = sqrt(temporal_dot(v, v));
    return true;
}

// Whether the previous frame's pixel `p` shows the surface this pixel shows: a hit, with a history, at the reprojected distance, facing the same way
RT_HD bool temporal_accepts(const TemporalParams& q, size_t p, const double* normal, double nn, double zq, const double* prev_length, const double* prev_normal,
                            const double* prev_depth, const double* prev_alpha) {
    const double pa = prev_alpha[p];
    if (pa == 0.0) return false;
    if (!(prev_length[p] > 0.0)) return false;
    if (!(fabs(prev_depth[p] / pa - zq) <= unfused_mul(q.depth_tolerance, zq))) return false;
    if (q.normal_test) {
        const double* pn = prev_normal + p * 3;
        if (!(temporal_dot(normal, pn) >= unfused_mul(q.normal_min, sqrt(unfused_mul(nn, temporal_dot(pn, pn)))))) return false;
    }
    return true;
}

// The reprojection and the four bilinear taps of one pixel, once for every stage that reads a history (temporal_pixel here; variance.hpp, clamp.hpp,
// probe.hpp and svgf.hpp): which taps are kept, their weights and places, and the two sums every stage needs.  Fixed slots in the order 00, 10, 01,
// 11 with a flag each: a tap outside the image or refused by temporal_accepts is SKIPPED, never weighted 0 — histories carry NaN and inf.  No tap
// is kept (blend == false, sw == sl == 0.0) without a history, where alpha == 0, where the pixel has no place in the previous frame (xy stays NaN)
// and where the kept weights do not sum above 0 (a reset).  The `prev_*` arrays are not read without a history.
struct TemporalTaps {
    double xy[2];  // (fx, fy); NaN, NaN where the pixel has no place in the previous frame
    double sw, sl; // sum wt and sum wt * prev_length over the kept taps, from 0.0, in tap order
    double wt[4];
    size_t at[4];  // pixel index of tap k in the previous frame
    bool ok[4];    // tap k is kept
    bool blend;    // sw > 0
};
RT_HD TemporalTaps temporal_taps(uint32_t w, uint32_t h, uint32_t x, uint32_t y, const TemporalParams& q, const double* normal, const double* depth,
                                 const double* alpha, const double* prev_length, const double* prev_normal, const double* prev_depth,
                                 const double* prev_alpha) {
    const size_t p = size_t(y) * w + x, o = p * 3;
    TemporalTaps t;
    t.xy[0] = t.xy[1] = NAN;
    t.sw = t.sl = 0.0;
    t.blend = false;
    for (int k = 0; k < 4; ++k) {
        t.ok[k] = false;
        t.wt[k] = 0.0;
        t.at[k] = 0;
    }
    const double a = alpha[p];
    if (!q.has_history || a == 0.0) return t;
    double fx, fy, zq;
    if (!temporal_where(w, h, x, y, q, depth[p] / a, fx, fy, zq)) return t;
    t.xy[0] = fx;
    t.xy[1] = fy;
    const double x0 = floor(fx), y0 = floor(fy);
    const double ax = fx - x0, ay = fy - y0;
    const int ix = int(x0), iy = int(y0); // -1 .. w - 1, -1 .. h - 1
    const double nn = temporal_dot(normal + o, normal + o);
#pragma unroll
    for (int k = 0; k < 4; ++k) { // 00, 10, 01, 11; unrolled, so that every slot is a register on the device
        const int i = k & 1, j = k >> 1;
        const int tx = ix + i, ty = iy + j;
        if (tx < 0 || tx >= int(w) || ty < 0 || ty >= int(h)) continue;
        const size_t tp = size_t(ty) * w + size_t(tx);
        if (!temporal_accepts(q, tp, normal + o, nn, zq, prev_length, prev_normal, prev_depth, prev_alpha)) continue;
        const double wt = unfused_mul(i ? ax : 1.0 - ax, j ? ay : 1.0 - ay);
        t.ok[k] = true;
        t.wt[k] = wt;
        t.at[k] = tp;
        t.sw = t.sw + wt;
        t.sl = t.sl + unfused_mul(wt, prev_length[tp]);
    }
    t.blend = t.sw > 0.0;
    return t;
}

// One RGB quantity of the previous frame over the kept taps: a chain of its own per channel, from 0.0, in tap order
RT_HD void temporal_tap_sum(const TemporalTaps& t, const double* prev_rgb, double* s) {
    s[0] = s[1] = s[2] = 0.0;
#pragma unroll
    for (int k = 0; k < 4; ++k)
        if (t.ok[k])
            for (int ch = 0; ch < 3; ++ch) s[ch] = s[ch] + unfused_mul(t.wt[k], prev_rgb[t.at[k] * 3 + ch]);
}

// The running mean's weights where t.blend: the history's length grown by this frame, capped; wa for this frame, wb for the history
struct TemporalBlend {
    double n, wa, wb;
};
RT_HD TemporalBlend temporal_blend(const TemporalTaps& t, const TemporalParams& q) {
    const double grown = t.sl / t.sw + 1.0;
    TemporalBlend b;
    b.n = grown < q.max_history ? grown : q.max_history;
    b.wa = 1.0 / b.n;
    b.wb = 1.0 - b.wa;
    return b;
}

struct TemporalPixel {
    double c[3], v[3], length, xy[2]; // v is meaningful with variances only
};

// One pixel of the call.  The current frame's arrays and the previous frame's are whole images; `prev_*` are not read without a history.
RT_HD TemporalPixel temporal_pixel(uint32_t w, uint32_t h, uint32_t x, uint32_t y, const TemporalParams& q, const double* linear, const double* variance,
                                   const double* normal, const double* depth, const double* alpha, const double* prev_linear, const double* prev_variance,
                                   const double* prev_length, const double* prev_normal, const double* prev_depth, const double* prev_alpha) {
    const size_t o = (size_t(y) * w + x) * 3;
    TemporalPixel out;
    for (int ch = 0; ch < 3; ++ch) { // this frame alone: no history, a miss, a reset
        out.c[ch] = linear[o + ch];
        out.v[ch] = q.has_variance ? variance[o + ch] : 0.0;
    }
    out.length = 1.0;
    const TemporalTaps t = temporal_taps(w, h, x, y, q, normal, depth, alpha, prev_length, prev_normal, prev_depth, prev_alpha);
    out.xy[0] = t.xy[0];
    out.xy[1] = t.xy[1];
    if (!t.blend) return out;
    double sc[3], sv[3];
    temporal_tap_sum(t, prev_linear, sc);
    if (q.has_variance) temporal_tap_sum(t, prev_variance, sv);
    const TemporalBlend b = temporal_blend(t, q);
    for (int ch = 0; ch < 3; ++ch) {
        out.c[ch] = unfused_mul(b.wb, sc[ch] / t.sw) + unfused_mul(b.wa, linear[o + ch]);
        if (q.has_variance) out.v[ch] = unfused_mul(unfused_mul(b.wb, b.wb), sv[ch] / t.sw) + unfused_mul(unfused_mul(b.wa, b.wa), variance[o + ch]);
    }
    out.length = b.n;
    return out;
}

// The device's block (temporal.hip): 64 pixels of a row by 4 rows, so a wave's loads of this frame's planes are consecutive doubles
constexpr uint32_t TEMPORAL_BLOCK_X = 64, TEMPORAL_BLOCK_Y = 4;

} // namespace rt
