// adaptive_state.hpp — the state of rttnw_render_adaptive_resume and its kin on the host (include/rttnw_hip.h has the layout): its header, its checks,
// and the permutation between its row-major records and the ranks' packed order.  No HIP: plain C++, which tests/state_host builds with the host
// compiler for tests/test_adaptive_state_cpu.py.  render_adaptive_api.cpp is the caller.
#pragma once
#include "../../include/rttnw_hip.h"
#include "rt_core.hpp"
#include "adaptive.hpp"

#include <algorithm>
#include <cmath>
#include <cstring>
#include <string>
#include <vector>

namespace rt {
constexpr uint32_t STATE_HEADER_DOUBLES = RTTNW_ADAPTIVE_STATE_HEADER, STATE_HEADER_FIELDS = 31;
static_assert(STATE_RECORD_DOUBLES == RTTNW_ADAPTIVE_STATE_RECORD, "the kernels' record is the header's");
static const char* const STATE_FIELD_NAMES[STATE_HEADER_FIELDS] = {
    "magic", "version", "width", "height", "pass_spp", "spp_chunk", "sample_begin", "precision", "max_depth", "quirks", "seed", "seed", "t_min",
    "background", "background", "background", "camera lookfrom", "camera lookfrom", "camera lookfrom", "camera lookat", "camera lookat", "camera lookat",
    "camera view_up", "camera view_up", "camera view_up", "camera vertical_fov", "camera aspect_ratio", "camera aperture", "camera focus_distance",
    "camera open_time", "camera close_time"};
inline uint64_t state_doubles(uint32_t width, uint32_t height) { return uint64_t(STATE_HEADER_DOUBLES) + uint64_t(STATE_RECORD_DOUBLES) * width * height; }
// The header this call's arguments make (cam == nullptr: validate() refuses the call next; its camera fields are then not compared)
inline void state_header(const rttnw_params& p, const rttnw_adaptive& a, const rttnw_camera_desc* cam, double h[STATE_HEADER_DOUBLES]) {
    std::fill(h, h + STATE_HEADER_DOUBLES, 0.0);
    h[0] = double(RTTNW_ADAPTIVE_STATE_MAGIC); h[1] = double(RTTNW_ADAPTIVE_STATE_VERSION);
    h[2] = p.width; h[3] = p.height; h[4] = a.pass_spp; h[5] = p.spp_chunk; h[6] = p.sample_begin; h[7] = p.precision; h[8] = p.max_depth; h[9] = p.quirks;
    h[10] = double(uint32_t(p.seed)); h[11] = double(uint32_t(p.seed >> 32));
    h[12] = p.t_min;
    for (int k = 0; k < 3; ++k) h[13 + k] = p.background[k];
    static_assert(sizeof(rttnw_camera_desc) == 15 * sizeof(double), "the state's header holds the camera as 15 doubles");
    if (cam) std::memcpy(h + 16, cam, sizeof(*cam));
}
// What `caller` (rttnw_render_adaptive_resume, rttnw_render_adaptive_region, rttnw_render_adaptive_budget) refuses of a state_in (p and a have passed
// refuse_adaptive_misuse), with the message in `err`; `first`: the lowest level in it.  `allow_empty` (the region and budget forms): a record of
// twelve zeros — a pixel that holds no samples yet — is accepted.
inline int refuse_state_misuse(const char* caller, bool allow_empty, const rttnw_params& p, const rttnw_adaptive& a, const rttnw_camera_desc* cam,
                               const double* st, uint32_t& first, std::string& err) {
    const std::string call = std::string(caller) + ": state_in: ";
    double want[STATE_HEADER_DOUBLES];
    state_header(p, a, cam, want);
    for (uint32_t i = 0; i < (cam ? STATE_HEADER_FIELDS : 16u); ++i) {
        if (std::memcmp(&st[i], &want[i], sizeof(double)) == 0) continue;
        err = call + (i == 0 ? "wrong magic number: not a state of this library" : i == 1 ? "unknown format version"
                             : std::string(STATE_FIELD_NAMES[i]) + " differs from this call's");
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
            err = call + "a record's n is 0 but the record is not empty (a pixel without samples is twelve zeros) (pixel " + std::to_string(q) + ")";
            return RTTNW_ERR_INVALID;
        }
        const char* why = !whole(n) ? "a record's n is not a finite integer" : !whole(k) ? "a record's k is not a finite integer"
                        : n < B ? "a record's n is below pass_spp" : std::fmod(n, B) != 0.0 ? "a record's n is not a multiple of pass_spp"
                        : n > cap ? "the state holds more samples than the cap (a record's n exceeds spp)"
                        : k != n / B * chunks ? "a record's k is not its passes times the chunks of a pass" : nullptr;
        if (why) { err = call + why + " (pixel " + std::to_string(q) + ")"; return RTTNW_ERR_INVALID; }
        lowest = std::min(lowest, n);
    }
    first = uint32_t(lowest / B);
    return 0;
}

// ---- the permutation.  A frame of `world` ranks (tile layout L: rttnw_tile_layout_get) keeps a pixel's record on the rank that owns its tile, in
// that rank's packed order; `ranks` holds one buffer of L.pixels_per_rank records per rank (one rank: the whole frame in packed order).
using RankRecords = std::vector<std::vector<double>>;
// Packed index of framebuffer pixel (x, y) on its owner among `world` ranks (rt_core.hpp tile_permuted; rttnw_amd/tiles.py packed_index)
inline void packed_place(uint32_t x, uint32_t y, const rttnw_tile_layout& L, uint32_t world, uint32_t& owner, size_t& idx) {
    const uint32_t permuted = tile_permuted(x >> 3, y >> 3, L.tiles_x);
    owner = permuted % world;
    idx = size_t(permuted / world) * 64 + ((y & 7u) << 3) + (x & 7u);
}
// The record of pixel (x, y) where the ranks keep it, and who owns it
inline const double* state_record_at(const RankRecords& ranks, uint32_t x, uint32_t y, const rttnw_tile_layout& L, uint32_t& owner) {
    size_t idx;
    packed_place(x, y, L, uint32_t(ranks.size()), owner, idx);
    return ranks[owner].data() + idx * STATE_RECORD_DOUBLES;
}
// f(q, owner, idx, n) for every run of n <= 8 pixels that is contiguous in BOTH orders — a tile's row inside the image: q its first pixel's row-major
// index, idx its packed index on `owner`
template <typename F> inline void for_each_tile_row(uint32_t width, uint32_t height, const rttnw_tile_layout& L, uint32_t world, F f) {
    for (uint32_t y = 0; y < height; ++y)
        for (uint32_t x = 0; x < width; x += 8) {
            uint32_t owner;
            size_t idx;
            packed_place(x, y, L, world, owner, idx);
            f(size_t(y) * width + x, owner, idx, std::min(8u, width - x));
        }
}
// A state's row-major records (`state`: header included; nullptr: no record anywhere) to every rank's packed order.  The rest of an edge tile and
// pad tiles keep zero records.
inline void state_scatter(const double* state, uint32_t width, uint32_t height, const rttnw_tile_layout& L, uint32_t world, RankRecords& ranks) {
    ranks.resize(world);
    for (std::vector<double>& v : ranks) v.assign(size_t(L.pixels_per_rank) * STATE_RECORD_DOUBLES, 0.0); // (each buffer made once: 25 MB for 512x512)
    if (!state) return;
    const double* rec = state + STATE_HEADER_DOUBLES;
    for_each_tile_row(width, height, L, world, [&](size_t q, uint32_t owner, size_t idx, uint32_t n) {
        std::copy(rec + q * STATE_RECORD_DOUBLES, rec + (q + n) * STATE_RECORD_DOUBLES, ranks[owner].begin() + idx * STATE_RECORD_DOUBLES);
    });
}
// ... and back: the ranks' records to their row-major places behind the header of `state` (which state_header writes)
inline void state_gather(const RankRecords& ranks, uint32_t width, uint32_t height, const rttnw_tile_layout& L, double* state) {
    for_each_tile_row(width, height, L, uint32_t(ranks.size()), [&](size_t q, uint32_t owner, size_t idx, uint32_t n) {
        const double* rec = ranks[owner].data() + idx * STATE_RECORD_DOUBLES;
        std::copy(rec, rec + size_t(n) * STATE_RECORD_DOUBLES, state + STATE_HEADER_DOUBLES + q * STATE_RECORD_DOUBLES);
    });
}
} // namespace rt
