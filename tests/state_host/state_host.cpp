// Host harness of rttnw_amd/csrc/adaptive_state.hpp: the state's header, its checks and the permutation between its row-major records and the ranks'
// packed order, behind a C interface for tests/test_adaptive_state_cpu.py.  With -DSTATE_HOST_MAIN a stand-alone program (the Makefile's
// `sanitize` target builds it with ASan + UBSan): the round trip of a 45x37 frame over 3 ranks.
#include "../../rttnw_amd/csrc/adaptive_state.hpp"
#include <cstdio>

static rttnw_tile_layout layout_of(uint32_t w, uint32_t h, uint32_t world) { // (rttnw_tile_layout_get, which lives behind the HIP runtime)
    rttnw_tile_layout L;
    L.tiles_x = (w + 7) / 8; L.tiles_y = (h + 7) / 8;
    L.n_tiles = L.tiles_x * L.tiles_y;
    L.tiles_per_rank = (L.n_tiles + world - 1) / world;
    L.pixels_per_rank = L.tiles_per_rank * 64;
    return L;
}

// owner and packed index of every pixel, row-major; returns pixels_per_rank
extern "C" uint32_t sh_place(uint32_t w, uint32_t h, uint32_t world, uint32_t* owner, uint64_t* idx) {
    const rttnw_tile_layout L = layout_of(w, h, world);
    for (uint32_t y = 0; y < h; ++y)
        for (uint32_t x = 0; x < w; ++x) {
            size_t i;
            rt::packed_place(x, y, L, world, owner[size_t(y) * w + x], i);
            idx[size_t(y) * w + x] = i;
        }
    return L.pixels_per_rank;
}
// state_in scattered to `world` ranks (`packed`: world x pixels_per_rank records, as the ranks hold them) and gathered into state_out's records
extern "C" void sh_round_trip(uint32_t w, uint32_t h, uint32_t world, const double* state_in, double* packed, double* state_out) {
    const rttnw_tile_layout L = layout_of(w, h, world);
    rt::RankRecords ranks;
    rt::state_scatter(state_in, w, h, L, world, ranks);
    for (uint32_t r = 0; r < world; ++r) std::copy(ranks[r].begin(), ranks[r].end(), packed + r * ranks[r].size());
    rt::state_gather(ranks, w, h, L, state_out);
}
extern "C" void sh_header(const rttnw_params* p, const rttnw_adaptive* a, const rttnw_camera_desc* cam, double* h) { rt::state_header(*p, *a, cam, h); }
extern "C" uint64_t sh_state_doubles(uint32_t w, uint32_t h) { return rt::state_doubles(w, h); }
extern "C" int sh_refuse(const char* caller, int allow_empty, const rttnw_params* p, const rttnw_adaptive* a, const rttnw_camera_desc* cam, const double* st,
                         uint32_t* first, char* msg, uint32_t msg_bytes) {
    std::string err;
    const int rc = rt::refuse_state_misuse(caller, allow_empty != 0, *p, *a, cam, st, *first, err);
    std::snprintf(msg, msg_bytes, "%s", err.c_str());
    return rc;
}

#if defined(STATE_HOST_MAIN)
int main() {
    const uint32_t w = 45, h = 37, world = 3;
    const rttnw_tile_layout L = layout_of(w, h, world);
    std::vector<double> in(rt::state_doubles(w, h)), out(in.size(), -1.0), packed(size_t(world) * L.pixels_per_rank * rt::STATE_RECORD_DOUBLES);
    for (size_t i = 0; i < in.size(); ++i) in[i] = double(i) + 0.5;
    sh_round_trip(w, h, world, in.data(), packed.data(), out.data());
    if (!std::equal(in.begin() + rt::STATE_HEADER_DOUBLES, in.end(), out.begin() + rt::STATE_HEADER_DOUBLES)) { std::puts("round trip differs"); return 1; }
    std::puts("state_host: 45x37 over 3 ranks round trip ok");
    return 0;
}
#endif
