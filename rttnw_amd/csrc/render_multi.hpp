// render_multi.hpp — what the host units of the render entry points share beyond render_common.hpp: the plan and the steps of a render over the ranks of
// a node (render_multi.cpp), which rttnw_render_adaptive_multi and its kin (render_adaptive_api.cpp) walk too, and three helpers of render_api.cpp.
#pragma once
#include "render_common.hpp"

namespace rt {
// A plain render's launch code in the precision of `p`
inline int render_tiles_any(::rttnw_scene* s, DeviceState* d, const rttnw_camera_desc* cam, const rttnw_params* p, void* d_packed, hipStream_t stream,
                            rttnw_stats* stats, bool sync_for_stats = true, bool prepare_only = false, const ListPass* ad = nullptr) {
    return RT_BY_PRECISION(p->precision, render_tiles_t, s, d, cam, p, d_packed, stream, stats, sync_for_stats, prepare_only, ad);
}
// What rttnw_render_adaptive and the entry points of render_adaptive_api.cpp refuse among the adaptive arguments themselves (both non-NULL): no device needed
int refuse_adaptive_misuse(const char* prefix, const rttnw_params* p, const rttnw_adaptive* a);
// What every host-output entry point ends with: the npx pixels of the image on the device to the caller's arrays (each optional), and a HIP error —
// `e`: of the call's own steps before this one — as RTTNW_ERR_HIP under the call's name.
int copy_image_out(const char* what, const DevBuf<uint8_t>& rgba, const DevBuf<uint8_t>& linear, uint32_t precision, size_t npx, uint8_t* out_rgba8,
                   double* out_linear, hipError_t e = hipSuccess);

// The environment of a call, read once (a MultiPlan holds it).  The gather to the root is a device-to-device copy for ranks on the root's device; for the others one of
// TWO transports over xGMI (RTTNW_MULTI_GATHER=rccl|peer, default rccl):
//   rccl  a grouped ncclSend / ncclRecv per rank buffer (north_star's "RCCL gather over xGMI"; communicators cached per device list);
//   peer  hipMemcpyPeerAsync of each rank's packed tiles into the root's gather buffer on the RANK's stream, an event behind it that the
//         root's stream waits for — 5 MB per rank, no library, no communicator.  Also what the call FALLS THROUGH to when RCCL cannot be
//         loaded or ncclCommInitAll fails (one stderr line; rttnw_stats.reserved bit 9 of rank 0), so that a node whose RCCL is broken
//         still renders.  Bit 8 of stats[0].reserved: the gather went through peer copies.
// RTTNW_MULTI_FORCE_TRANSPORT=1 (tests; RTTNW_MULTI_FORCE_RCCL=1 is the older name): the ranks on the root's device travel through the
// transport too — the root sending to itself — so that the dlopen'ed entry points, the communicator set-up, the peer copies, the stream
// ordering and the error paths run on a box with ONE GPU as well.  RTTNW_MULTI_FAIL_RCCL=1 (tests): the RCCL set-up reports failure.
// RTTNW_DEBUG_MULTI: one stderr line per communicator set-up and per gather.
struct MultiEnv {
    bool force_transport = false, gather_peer = false, gather_invalid = false, fail_rccl = false, debug = false;
    MultiEnv() {
        const auto is_1 = [](const char* e) { return e && e[0] == '1'; };
        force_transport = is_1(getenv("RTTNW_MULTI_FORCE_RCCL")) || is_1(getenv("RTTNW_MULTI_FORCE_TRANSPORT"));
        const char* gather = getenv("RTTNW_MULTI_GATHER");
        gather_peer = gather && std::string(gather) == "peer";
        gather_invalid = gather && !gather_peer && std::string(gather) != "rccl";
        fail_rccl = is_1(getenv("RTTNW_MULTI_FAIL_RCCL"));
        debug = getenv("RTTNW_DEBUG_MULTI") != nullptr;
    }
};

// Who traces what, and where: made once per call (multi_plan), read by every step.
struct MultiPlan {
    const MultiEnv env;
    struct Rank { DeviceState* d; uint32_t dev, slot; }; // its device's state, index in `devices`, and its place among the ranks of that device
    std::vector<Rank> ranks;
    std::vector<int> devices;             // in order of first appearance; devices[0] = the root's (rank 0's) device
    std::vector<DeviceState*> dev_state;  // per distinct device
    std::vector<uint32_t> dev_ranks;      // ... and how many ranks live on it
    DeviceState* root = nullptr;
    size_t rsz = 0, chunk = 0, npx = 0;   // bytes of a real, of a rank's packed tiles; pixels of the image
    size_t aux_chunk = 0;                 // rttnw_render_adaptive_multi: bytes of a rank's auxiliary records, which travel with its tiles (0: a plain render)
    bool single = false;                  // rttnw_render_adaptive_resume with ngpu == 0: one rank on the scene's own device, which reads no gather environment
    bool transport() const { return !single && (devices.size() > 1 || env.force_transport); } // some rank's tiles travel
    bool local(uint32_t r) const { return single || (!env.force_transport && ranks[r].dev == 0); } // rank r's do not: a copy on the root's device
    uint8_t* packed(uint32_t r) const { return ranks[r].d->multi_packed.p + chunk * ranks[r].slot; } // rank r's packed tiles, on its device
    uint8_t* gathered(uint32_t r) const { return root->gathered.p + chunk * r; }                      // ... and their place on the root's
    uint8_t* aux(uint32_t r) const { return ranks[r].d->multi_aux.p + aux_chunk * ranks[r].slot; }    // the same for its auxiliary records
    uint8_t* gathered_aux(uint32_t r) const { return root->gathered_aux.p + aux_chunk * r; }
};

// The steps (render_multi.cpp says what each does)
int multi_plan(::rttnw_scene* s, const rttnw_params& p, uint32_t ngpu, const int32_t* device_ids, MultiPlan& m, const char* call = "render_multi");
int multi_prepare_buffers(const MultiPlan& m, bool frame_image = true);
int multi_gather(const MultiPlan& m, bool& use_peer, bool& fell_back);
int multi_join_local(const MultiPlan& m);
int multi_finish_streams(const MultiPlan& m);
int multi_untile(const rttnw_params& p, const MultiPlan& m);
} // namespace rt
