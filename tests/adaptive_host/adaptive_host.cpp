// Host harness of rttnw_amd/csrc/adaptive.hpp: the functions the adaptive resolve kernel folds a pixel's chunks with, behind a C
// interface for tests/test_adaptive_cpu.py.
#include "../../rttnw_amd/csrc/adaptive.hpp"

extern "C" {
// Fold chunks [c0, c1) of a sequence (means m[3 * c], sample counts n[c]) into `state`.
void ah_fold(rt::AdaptivePixel* state, const double* m, const uint32_t* n, uint32_t c0, uint32_t c1) {
    for (uint32_t c = c0; c < c1; ++c) rt::adaptive_fold(*state, m + 3 * size_t(c), n[c]);
}
double ah_stderr(const rt::AdaptivePixel* state, int ch) { return rt::adaptive_stderr(*state, ch); }
int ah_active(const rt::AdaptivePixel* state, const double* value, double rel_error, double abs_error, uint32_t cap) {
    return rt::adaptive_active(*state, value, rel_error, abs_error, cap) ? 1 : 0;
}
}
