// Host harness of rttnw_amd/csrc/budget_select.hpp: rttnw_budget_select with the functions the device kernels (budget_kernels.hpp) call, pixel by
// pixel, and a plain sort of the keys in place of the radix select, behind a C interface for tests/test_budget_cpu.py.
#include "../../rttnw_amd/csrc/budget_select.hpp"
#include <algorithm>
#include <vector>

extern "C" int bh_select(uint32_t w, uint32_t h, const double* value, const double* se, const uint32_t* spp, uint32_t cap, double rel_error,
                         double abs_error, uint64_t max_pixels, uint8_t* out_mask, double* out_priority, uint64_t* out_selected) {
    const size_t n = size_t(w) * h;
    std::vector<rt::BudgetKey> keys(n);
    std::vector<uint32_t> order;
    for (size_t q = 0; q < n; ++q) {
        const double zero[3] = {0.0, 0.0, 0.0};
        const bool read = spp[q] != 0u; // (the colour and the error of a pixel without samples are never read)
        const double rho = rt::budget_priority(read ? value + q * 3 : zero, read ? se + q * 3 : zero, spp[q], cap, rel_error, abs_error);
        keys[q] = rt::budget_key(rho, uint32_t(q));
        if (keys[q].hi != 0) order.push_back(uint32_t(q));
        if (out_priority) out_priority[q] = rho;
        if (out_mask) out_mask[q] = 0;
    }
    std::sort(order.begin(), order.end(), [&](uint32_t a, uint32_t b) { return !rt::budget_key_ge(keys[b], keys[a]); }); // descending, no ties
    const uint64_t m = std::min<uint64_t>(order.size(), max_pixels);
    for (uint64_t i = 0; i < m && out_mask; ++i) out_mask[order[i]] = 1;
    if (out_selected) *out_selected = m;
    return 0;
}

// The radix select's view of a key: its digits put together again give the key, and a key matches every prefix of itself.  Returns 0 when that holds.
extern "C" int bh_digits_roundtrip(uint64_t hi, uint32_t lo) {
    const rt::BudgetKey k{hi, lo};
    rt::BudgetKey again{0, 0};
    for (uint32_t d = 0; d < rt::BUDGET_DIGITS; ++d) {
        if (!rt::budget_prefix_matches(k, again, d)) return 1 + int(d);
        const rt::BudgetKey part = rt::budget_digit_key(d, rt::budget_digit(k, d));
        again.hi |= part.hi;
        again.lo |= part.lo;
    }
    if (again.hi != k.hi || again.lo != k.lo) return 100;
    // a key that differs in one bit stops matching at the digit that holds it
    for (uint32_t bit = 0; bit < 96; ++bit) {
        rt::BudgetKey other = k;
        if (bit < 32) other.lo ^= 1u << bit; else other.hi ^= 1ull << (bit - 32);
        const uint32_t first_diff = (95 - bit) / rt::BUDGET_DIGIT_BITS;
        for (uint32_t d = 0; d <= rt::BUDGET_DIGITS; ++d) {
            rt::BudgetKey prefix{0, 0};
            for (uint32_t e = 0; e < d; ++e) { const rt::BudgetKey part = rt::budget_digit_key(e, rt::budget_digit(k, e)); prefix.hi |= part.hi; prefix.lo |= part.lo; }
            if (rt::budget_prefix_matches(other, prefix, d) != (d <= first_diff)) return 200 + int(bit);
        }
    }
    return 0;
}
