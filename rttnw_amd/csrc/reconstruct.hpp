// reconstruct.hpp — the arithmetic of rttnw_reconstruct (include/rttnw_hip.h has the contract, DESIGN.md §10b the why), shared by the device
// kernels (denoise.hip) and the host test harness (tests/reconstruct_host): rttnw_denoise's à-trous filter over an image of which only
// some pixels hold a value.  Every pixel carries a flag H, "holds a value", through the passes beside its colour: a tap without H is dropped
// like a tap outside the image, and a centre without H is FILLED from the taps that remain — weighted by the features alone, it has no colour
// to compare — and holds a value from then on.  Pass i reaches 2 * 2^i pixels to either side, so a lattice of spacing 2^L is filled after
// L passes at the latest where the features let neighbours through.
//
// The arithmetic is denoise.hpp's atrous_*<FLAGS> templates with the flags on — rttnw_denoise is the same templates with them off, so with
// every flag set the two agree bit for bit (tests/test_reconstruct_cpu.py).  This header only names the instantiations.
#pragma once
#include "denoise.hpp"

namespace rt {

// One pass's input: denoise.hpp's view and the flags, a byte per pixel, row-major.
struct ReconstructView {
    DenoiseView img;
    const uint8_t* holds; // w*h, nonzero = the pixel holds a value
};

RT_HD uint8_t reconstruct_prepare_pixel(bool holds, const double* colour, const double* variance, const double* albedo, double alpha,
                                        double* out_colour, double* out_variance) {
    uint8_t h = 0u;
    for (int ch = 0; ch < 3; ++ch)
        h = atrous_prepare_value<true>(holds, colour + ch, variance ? variance + ch : nullptr, albedo[ch], alpha, out_colour + ch,
                                       variance ? out_variance + ch : nullptr);
    return h;
}
RT_HD uint8_t reconstruct_filter_pixel(const ReconstructView& rv, const DenoiseParams& prm, uint32_t x, uint32_t y, uint32_t stride,
                                       double* out_colour, double* out_variance) {
    return atrous_filter_pixel<true>(rv.img, rv.holds, prm, x, y, stride, out_colour, out_variance);
}
RT_HD uint8_t reconstruct_finish_pixel(bool holds, bool remodulate, const double* colour, const double* variance, const double* albedo, double alpha,
                                       double* out_colour, uint8_t* out_rgba, double* out_variance) {
    return atrous_finish_pixel<true>(holds, remodulate, colour, variance, albedo, alpha, out_colour, out_rgba, out_variance);
}

} // namespace rt
