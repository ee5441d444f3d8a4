// budget_select.hpp — the arithmetic of rttnw_budget_select (include/rttnw_hip.h has the contract, DESIGN.md §10a "budgeted form" the why): who is a
// candidate for the next pass, the priority a candidate is ranked by, and the 96-bit key whose order IS the selection's order.  Shared by the
// device kernels (budget_kernels.hpp) and by a host build with a plain sort as its select (tests/budget_host), which is the CPU yardstick.
// Everything is double and integer; the one product goes through unfused_mul(), so no build fuses it into the sum that follows.
#pragma once
#include "adaptive.hpp"
#include <string.h>

namespace rt {

// The priority of a pixel read off the maps an adaptive entry point returns (value: its mean, se: its standard errors, spp: its samples):
//   0            not a candidate: spp >= cap, or spp > 0 and se_c <= abs_error + rel_error * value_c in every channel (adaptive_active's rule)
//   +inf         spp == 0 (value and se are never read: they may be NaN)
//   max_c e_c    otherwise, e_c = 0 where se_c <= t_c = abs_error + rel_error * value_c, else se_c / t_c — and +inf where that quotient is not a
//                finite positive number (t_c == 0, a NaN or infinite se_c, a negative t_c).
// A candidate's priority lies in (1, +inf]: se > t > 0 makes the correctly rounded quotient at least 1 + 2^-52.
RT_HD double budget_priority(const double* value, const double* se, uint32_t spp, uint32_t cap, double rel_error, double abs_error) {
    if (spp == 0u) return INFINITY;
    if (spp >= cap) return 0.0;
    double rho = 0.0;
    for (int ch = 0; ch < 3; ++ch) {
        const double t = abs_error + unfused_mul(rel_error, value[ch]);
        if (se[ch] <= t) continue;
        double e = se[ch] / t;
        if (!(e > 0.0 && e < INFINITY)) e = INFINITY;
        if (e > rho) rho = e;
    }
    return rho;
}

// The key of pixel `index` (row-major, y * width + x): 96 bits, the high 64 the bit pattern of its priority — positive doubles and +inf order as
// their bits —, the low 32 bits 0xFFFFFFFF - index, so that of two equal priorities the smaller index is the larger key.  A non-candidate's key is
// 0; a candidate's high word is above the bits of 1.0, so the keys of candidates are unique and never 0.
struct BudgetKey {
    uint64_t hi;
    uint32_t lo;
};
RT_HD uint64_t budget_priority_bits(double rho) {
    uint64_t u;
    memcpy(&u, &rho, sizeof(u));
    return u;
}
RT_HD BudgetKey budget_key(double rho, uint32_t index) {
    BudgetKey k;
    k.hi = rho > 0.0 ? budget_priority_bits(rho) : 0ull;
    k.lo = k.hi ? 0xFFFFFFFFu - index : 0u;
    return k;
}
RT_HD bool budget_key_ge(const BudgetKey& a, const BudgetKey& b) { return a.hi > b.hi || (a.hi == b.hi && a.lo >= b.lo); }

// The radix select reads a key as BUDGET_DIGITS digits of BUDGET_DIGIT_BITS bits, most significant first.
constexpr uint32_t BUDGET_DIGIT_BITS = 12u, BUDGET_DIGITS = 8u, BUDGET_BINS = 1u << BUDGET_DIGIT_BITS;
static_assert(BUDGET_DIGIT_BITS * BUDGET_DIGITS == 96u, "the digits cover the key");
// Digit d of a key.  Digits 0 .. 4 lie in the high word, digit 5 straddles the two words, digits 6 and 7 lie in the low word.
RT_HD uint32_t budget_digit(const BudgetKey& k, uint32_t d) {
    const uint32_t shift = 96u - BUDGET_DIGIT_BITS * (d + 1u); // of the digit's lowest bit in the 96-bit key
    if (shift >= 32u) return uint32_t(k.hi >> (shift - 32u)) & (BUDGET_BINS - 1u);
    if (shift + BUDGET_DIGIT_BITS > 32u) return (uint32_t(k.hi << (32u - shift)) | (k.lo >> shift)) & (BUDGET_BINS - 1u);
    return (k.lo >> shift) & (BUDGET_BINS - 1u);
}
// The key that holds digit `value` at place d and zeros elsewhere
RT_HD BudgetKey budget_digit_key(uint32_t d, uint32_t value) {
    const uint32_t shift = 96u - BUDGET_DIGIT_BITS * (d + 1u);
    BudgetKey k;
    k.hi = shift >= 32u ? uint64_t(value) << (shift - 32u) : uint64_t(value) >> (32u - shift);
    k.lo = shift >= 32u ? 0u : value << shift;
    return k;
}
// Do the first d digits of k equal those of `prefix` (whose digits from d on are 0)?
RT_HD bool budget_prefix_matches(const BudgetKey& k, const BudgetKey& prefix, uint32_t d) {
    const uint32_t bits = BUDGET_DIGIT_BITS * d;
    if (bits == 0u) return true;
    const uint64_t mask_hi = bits >= 64u ? ~0ull : ~0ull << (64u - bits);
    const uint32_t mask_lo = bits <= 64u ? 0u : ~0u << (96u - bits);
    return (k.hi & mask_hi) == prefix.hi && (k.lo & mask_lo) == prefix.lo;
}

} // namespace rt
