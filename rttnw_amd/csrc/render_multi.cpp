// render_multi.cpp — rttnw_render_multi: the whole of main.rs:202-229 on the GPUs of one node, in one call (per-device streams, RCCL gather), as named
// steps over a MultiPlan (render_multi.hpp) that the adaptive forms over ranks (render_adaptive_api.cpp) walk too; and rttnw_shutdown.  Host code only.
#include "render_multi.hpp"
#include "pixel_lists.hpp"

#include <rccl/rccl.h>
#include <dlfcn.h>

namespace rt {
// RCCL, bound at first use (a single device, or logical ranks that share one device, never touch it).
struct Rccl {
    void* lib = nullptr;
    ncclResult_t (*CommInitAll)(ncclComm_t*, int, const int*) = nullptr;
    ncclResult_t (*CommDestroy)(ncclComm_t) = nullptr;
    ncclResult_t (*GroupStart)() = nullptr;
    ncclResult_t (*GroupEnd)() = nullptr;
    ncclResult_t (*Send)(const void*, size_t, ncclDataType_t, int, ncclComm_t, hipStream_t) = nullptr;
    ncclResult_t (*Recv)(void*, size_t, ncclDataType_t, int, ncclComm_t, hipStream_t) = nullptr;
    const char* (*GetErrorString)(ncclResult_t) = nullptr;
    bool load(std::string& err) {
        if (lib) return true;
        lib = dlopen("librccl.so.1", RTLD_NOW | RTLD_GLOBAL);
        if (!lib) lib = dlopen("librccl.so", RTLD_NOW | RTLD_GLOBAL);
        if (!lib) { err = std::string("cannot load RCCL: ") + dlerror(); return false; }
        CommInitAll = (decltype(CommInitAll))dlsym(lib, "ncclCommInitAll");
        CommDestroy = (decltype(CommDestroy))dlsym(lib, "ncclCommDestroy");
        GroupStart = (decltype(GroupStart))dlsym(lib, "ncclGroupStart");
        GroupEnd = (decltype(GroupEnd))dlsym(lib, "ncclGroupEnd");
        Send = (decltype(Send))dlsym(lib, "ncclSend");
        Recv = (decltype(Recv))dlsym(lib, "ncclRecv");
        GetErrorString = (decltype(GetErrorString))dlsym(lib, "ncclGetErrorString");
        if (!CommInitAll || !CommDestroy || !GroupStart || !GroupEnd || !Send || !Recv || !GetErrorString) { err = "RCCL lacks an expected entry point"; return false; }
        return true;
    }
};
static Rccl g_rccl;
struct MultiComms { // one communicator set per distinct list of devices, kept until rttnw_shutdown() / process exit
    std::vector<int> devices;
    std::vector<ncclComm_t> comms; // (empty: the set-up over these devices failed, comms_over)
    std::mutex in_use; // RCCL allows ONE thread at a time to issue operations on a communicator: held from GroupStart to GroupEnd
};
static std::vector<MultiComms*> g_comms;
static std::mutex g_comms_mutex; // the list itself (rttnw_render_multi may be called from several host threads, each with its own scene)
static bool g_comms_atexit = false;

// Destroy the cached communicator sets (rttnw_shutdown; registered with atexit at the first set-up, so that a process that
// never calls it still leaves RCCL in order — before the HIP runtime's own teardown, which atexit runs later: LIFO).
static void destroy_comms() {
    std::lock_guard<std::mutex> lock(g_comms_mutex);
    // (at exit, under a host that tears its own HIP context down first — Python with torch —, the runtime may already be finalising: then
    // only the host structures are released; RCCL's own teardown has nothing left to talk to)
    int n_dev = 0;
    const bool runtime_alive = hipGetDeviceCount(&n_dev) == hipSuccess && n_dev > 0;
    for (MultiComms* c : g_comms) {
        std::lock_guard<std::mutex> use(c->in_use);
        for (ncclComm_t comm : c->comms)
            if (comm && g_rccl.CommDestroy && runtime_alive) (void)g_rccl.CommDestroy(comm);
        c->comms.clear();
    }
    for (MultiComms* c : g_comms) delete c;
    g_comms.clear();
}

static DeviceState* state_on(::rttnw_scene* s, int device, std::string& err) {
    if (s->device && s->device->device == device) return s->device;
    for (DeviceState* d : s->more_devices)
        if (d->device == device) return d;
    if (hipSetDevice(device) != hipSuccess) { err = "hipSetDevice failed"; return nullptr; }
    DeviceState* d = nullptr;
    if (device_state_create(d, err)) return nullptr;
    s->more_devices.push_back(d);
    return d;
}

// Who traces what, and where
int multi_plan(::rttnw_scene* s, const rttnw_params& p, uint32_t ngpu, const int32_t* device_ids, MultiPlan& m, const char* call) {
    std::string err;
    m.ranks.resize(ngpu);
    for (uint32_t r = 0; r < ngpu; ++r) {
        DeviceState* d = state_on(s, device_ids[r], err);
        if (!d) { set_last_error(std::string(call) + ": " + err); return RTTNW_ERR_HIP; }
        uint32_t k = 0;
        while (k < m.devices.size() && m.devices[k] != device_ids[r]) ++k;
        if (k == m.devices.size()) { m.devices.push_back(device_ids[r]); m.dev_state.push_back(d); m.dev_ranks.push_back(0); }
        m.ranks[r] = {d, k, m.dev_ranks[k]++};
    }
    rttnw_tile_layout L;
    fill_layout(p.width, p.height, ngpu, L);
    m.root = m.ranks[0].d;
    m.rsz = p.precision == RTTNW_F32 ? sizeof(float) : sizeof(double);
    m.chunk = size_t(L.pixels_per_rank) * 4 * m.rsz;
    m.npx = size_t(p.width) * p.height;
    return 0;
}

// Everything that allocates, before anything is launched (an allocation or a free between two ranks' launches would synchronise its whole
// device): the streams, this layer's buffers, then per rank what a first use brings — scene uploads and workspace growth
// (`frame_image`: the root un-tiles a frame-sized image; rttnw_render_adaptive_region writes a window-sized one instead)
int multi_prepare_buffers(const MultiPlan& m, bool frame_image) {
    for (size_t k = 0; k < m.devices.size(); ++k) {
        DeviceState* d = m.dev_state[k];
        HIP_TRY(hipSetDevice(d->device));
        if (!d->stream) HIP_TRY(create_stream(d->stream, hipStreamNonBlocking));
        HIP_TRY(d->multi_packed.grow(m.chunk * m.dev_ranks[k]));
    }
    DeviceState* root = m.root;
    HIP_TRY(hipSetDevice(root->device));
    HIP_TRY(root->gathered.grow(m.chunk * m.ranks.size()));
    if (!frame_image) return 0;
    HIP_TRY(root->linear.grow(m.npx * 3 * m.rsz));
    HIP_TRY(root->rgba.grow(m.npx * 4));
    return 0;
}
static int multi_prepare(::rttnw_scene* s, const rttnw_camera_desc* cam, const rttnw_params& p, const MultiPlan& m) {
    if (int rc = multi_prepare_buffers(m)) return rc;
    for (uint32_t r = 0; r < m.ranks.size(); ++r) {
        rttnw_params pr = p;
        pr.tile_rank = r;
        DeviceState* d = m.ranks[r].d;
        if (int rc = render_tiles_any(s, d, cam, &pr, m.packed(r), d->stream.get(), nullptr, false, true)) return rc;
    }
    return 0;
}

// Every rank traces its tiles, on its device's stream, between its two events of `ev`; ranks that share a device run one after the other
static int multi_trace(::rttnw_scene* s, const rttnw_camera_desc* cam, const rttnw_params& p, const MultiPlan& m, std::vector<Event>& ev, rttnw_stats* stats) {
    for (uint32_t r = 0; r < m.ranks.size(); ++r) {
        DeviceState* d = m.ranks[r].d;
        HIP_TRY(hipSetDevice(d->device));
        rttnw_params pr = p;
        pr.tile_rank = r;
        HIP_TRY(create_event(ev[2 * r]));
        HIP_TRY(create_event(ev[2 * r + 1]));
        HIP_TRY(hipEventRecord(ev[2 * r].get(), d->stream.get()));
        if (int rc = render_tiles_any(s, d, cam, &pr, m.packed(r), d->stream.get(), stats ? &stats[r] : nullptr, false)) return rc;
        HIP_TRY(hipEventRecord(ev[2 * r + 1].get(), d->stream.get()));
    }
    return 0;
}

// The communicator set over `devices`: found, or made at the first call over that list and kept (set-up costs ~100 ms; destroyed by
// rttnw_shutdown() or at exit).  nullptr when there is none: a failed set-up says why on stderr, once, and is kept as well — an entry without
// communicators —, so that later calls over that list go straight to the peer copies.  Called with g_comms_mutex held.
static MultiComms* comms_over(const std::vector<int>& devices, const MultiEnv& env) {
    for (MultiComms* c : g_comms)
        if (c->devices == devices) return c->comms.empty() ? nullptr : c;
    MultiComms* mc = new MultiComms();
    mc->devices = devices;
    g_comms.push_back(mc);
    std::string why;
    if (env.fail_rccl) why = "RTTNW_MULTI_FAIL_RCCL=1";
    else if (g_rccl.load(why)) {
        mc->comms.resize(devices.size());
        const ncclResult_t nr = g_rccl.CommInitAll(mc->comms.data(), int(devices.size()), devices.data());
        if (nr != ncclSuccess) { why = std::string("ncclCommInitAll: ") + g_rccl.GetErrorString(nr); mc->comms.clear(); }
    }
    if (mc->comms.empty()) {
        fprintf(stderr, "[render_multi] RCCL gather unavailable (%s): gathering through peer copies\n", why.c_str());
        return nullptr;
    }
    if (!g_comms_atexit) { g_comms_atexit = true; std::atexit(destroy_comms); }
    if (env.debug) fprintf(stderr, "[render_multi] RCCL communicators over %zu device(s)\n", devices.size());
    return mc;
}

// The two transports of the ranks' tiles to the root's gather buffer (MultiEnv has what they are).
constexpr int GATHER_UNAVAILABLE = 1; // gather_rccl: there is no communicator set; nothing has been sent yet, so gather_peer can do the same job
static int gather_rccl(const MultiPlan& m) {
    std::unique_lock<std::mutex> comms_lock(g_comms_mutex);
    MultiComms* mc = comms_over(m.devices, m.env);
    if (!mc) return GATHER_UNAVAILABLE;
    // (the list's lock is released, the set's own is taken: two host threads rendering over the SAME devices take turns on
    // its communicators; threads over different device lists do not wait for each other)
    std::unique_lock<std::mutex> use(mc->in_use);
    comms_lock.unlock();
    ncclResult_t nr = g_rccl.GroupStart();
    uint32_t n_sent = 0;
    for (uint32_t r = 0; r < m.ranks.size() && nr == ncclSuccess; ++r) {
        if (m.local(r)) continue; // on the root's device: copied by multi_untile
        const uint32_t k = m.ranks[r].dev;
        nr = g_rccl.Send(m.packed(r), m.chunk, ncclChar, 0, mc->comms[k], m.ranks[r].d->stream.get());
        if (nr == ncclSuccess) nr = g_rccl.Recv(m.gathered(r), m.chunk, ncclChar, int(k), mc->comms[0], m.root->stream.get());
        ++n_sent;
        if (!m.aux_chunk) continue; // the rank's auxiliary records: a second send inside the one group
        if (nr == ncclSuccess) nr = g_rccl.Send(m.aux(r), m.aux_chunk, ncclChar, 0, mc->comms[k], m.ranks[r].d->stream.get());
        if (nr == ncclSuccess) nr = g_rccl.Recv(m.gathered_aux(r), m.aux_chunk, ncclChar, int(k), mc->comms[0], m.root->stream.get());
        ++n_sent;
    }
    ncclResult_t ne = g_rccl.GroupEnd();
    if (nr == ncclSuccess) nr = ne;
    if (nr != ncclSuccess) { set_last_error(std::string("RCCL gather: ") + g_rccl.GetErrorString(nr)); return RTTNW_ERR_HIP; }
    if (m.env.debug) fprintf(stderr, "[render_multi] %u rank buffer(s) of %zu bytes through ncclSend / ncclRecv\n", n_sent, m.chunk);
    return 0;
}
static int gather_peer(const MultiPlan& m) {
    DeviceState* root = m.root;
    // direct access root <- rank device where the fabric allows it (xGMI: every pair of a node); without it the copy is staged by the runtime
    for (size_t k = 1; k < m.devices.size(); ++k) {
        int can = 0;
        if (hipDeviceCanAccessPeer(&can, m.devices[k], root->device) == hipSuccess && can) {
            HIP_TRY(hipSetDevice(m.devices[k]));
            const hipError_t e = hipDeviceEnablePeerAccess(root->device, 0);
            if (e != hipSuccess && e != hipErrorPeerAccessAlreadyEnabled) HIP_TRY(e);
            (void)hipGetLastError();
        }
    }
    std::vector<Event> sent(m.ranks.size());
    uint32_t n_sent = 0;
    for (uint32_t r = 0; r < m.ranks.size(); ++r) {
        if (m.local(r)) continue; // on the root's device: copied by multi_untile
        DeviceState* d = m.ranks[r].d;
        HIP_TRY(hipSetDevice(d->device));
        HIP_TRY(hipMemcpyPeerAsync(m.gathered(r), root->device, m.packed(r), d->device, m.chunk, d->stream.get()));
        if (m.aux_chunk) { HIP_TRY(hipMemcpyPeerAsync(m.gathered_aux(r), root->device, m.aux(r), d->device, m.aux_chunk, d->stream.get())); ++n_sent; }
        HIP_TRY(create_event(sent[r], hipEventDisableTiming));
        HIP_TRY(hipEventRecord(sent[r].get(), d->stream.get()));
        ++n_sent;
    }
    HIP_TRY(hipSetDevice(root->device));
    for (uint32_t r = 0; r < m.ranks.size(); ++r)
        if (sent[r]) HIP_TRY(hipStreamWaitEvent(root->stream.get(), sent[r].get(), 0)); // the un-tile reads what the ranks' streams have written
    if (m.env.debug) fprintf(stderr, "[render_multi] %u rank buffer(s) of %zu bytes through hipMemcpyPeerAsync\n", n_sent, m.chunk);
    // (the events are destroyed when this function ends: a recorded event may be destroyed while work waits on it — the wait was enqueued)
    return 0;
}

// On the root's stream: the tiles of the ranks that live on its device (unless they went through the transport) join the gathered ones ...
int multi_join_local(const MultiPlan& m) {
    DeviceState* root = m.root;
    HIP_TRY(hipSetDevice(root->device));
    for (uint32_t r = 0; r < m.ranks.size(); ++r) {
        if (!m.local(r)) continue;
        HIP_TRY(hipMemcpyAsync(m.gathered(r), m.packed(r), m.chunk, hipMemcpyDeviceToDevice, root->stream.get()));
        if (m.aux_chunk) HIP_TRY(hipMemcpyAsync(m.gathered_aux(r), m.aux(r), m.aux_chunk, hipMemcpyDeviceToDevice, root->stream.get()));
    }
    return 0;
}
// ... and, once the image is enqueued behind them, every device's stream has finished
int multi_finish_streams(const MultiPlan& m) {
    for (DeviceState* d : m.dev_state) {
        HIP_TRY(hipSetDevice(d->device));
        HIP_TRY(hipStreamSynchronize(d->stream.get()));
    }
    HIP_TRY(hipSetDevice(m.root->device));
    return 0;
}
// The frame's image (and, of auxiliary records, its samples and standard-error maps) made of the gathered tiles on the root
int multi_untile(const rttnw_params& p, const MultiPlan& m) {
    DeviceState* root = m.root;
    if (int rc = multi_join_local(m)) return rc;
    if (int rc = rttnw_untile_device(p.width, p.height, p.tile_world, p.precision, root->gathered.p, root->linear.p, root->rgba.p, root->stream.get())) return rc;
    if (m.aux_chunk) // ... and the samples and standard-error maps of the auxiliary records
        if (int rc = untile_aux_launch(p.width, p.height, p.tile_world, (const double*)root->gathered_aux.p, (uint32_t*)root->ad_spp.p, (double*)root->ad_stderr.p,
                                       root->stream.get())) return rc;
    return multi_finish_streams(m);
}
// The ranks' buffers to the root's gather buffers, by the transport the call uses (MultiEnv), falling through from RCCL to the peer copies
int multi_gather(const MultiPlan& m, bool& use_peer, bool& fell_back) {
    use_peer = m.transport() && m.env.gather_peer;
    fell_back = false;
    if (m.transport() && !use_peer) {
        const int rc = gather_rccl(m);
        if (rc == GATHER_UNAVAILABLE) use_peer = fell_back = true;
        else if (rc) return rc;
    }
    return use_peer ? gather_peer(m) : 0;
}
} // namespace rt

extern "C" int rttnw_render_multi(rttnw_scene* s, const rttnw_camera_desc* cam, const rttnw_params* p_in, uint32_t ngpu, const int32_t* device_ids,
                                  double* out_linear_rgb, uint8_t* out_rgba8, rttnw_stats* stats) {
    using namespace rt;
    if (!p_in || !ngpu || ngpu > 64 || !device_ids) { set_last_error("render_multi: bad arguments"); return RTTNW_ERR_INVALID; }
    rttnw_params p = *p_in;
    p.tile_rank = 0; p.tile_world = ngpu;
    if (int rc = validate(s, cam, &p)) return rc;
    const int n_dev = rttnw_device_count();
    for (uint32_t r = 0; r < ngpu; ++r)
        if (device_ids[r] < 0 || device_ids[r] >= n_dev) { set_last_error("render_multi: no such device"); return RTTNW_ERR_INVALID; }
    DeviceGuard restore; // (the caller's device is current again after EVERY return below, the error paths included)
    MultiPlan m;
    if (int rc = multi_plan(s, p, ngpu, device_ids, m)) return rc;
    if (int rc = multi_prepare(s, cam, p, m)) return rc;
    std::vector<Event> ev(size_t(ngpu) * 2); // per rank: before and behind its trace
    if (int rc = multi_trace(s, cam, p, m, ev, stats)) return rc;
    // (refused here, after the trace, as it always was)
    if (m.env.gather_invalid) { set_last_error("render_multi: RTTNW_MULTI_GATHER must be rccl or peer"); return RTTNW_ERR_INVALID; }
    bool use_peer = false, fell_back = false;
    if (int rc = multi_gather(m, use_peer, fell_back)) return rc;
    if (int rc = multi_untile(p, m)) return rc;
    for (uint32_t r = 0; r < ngpu && stats; ++r) {
        float ms = 0;
        HIP_TRY(hipSetDevice(m.ranks[r].d->device));
        HIP_TRY(hipEventElapsedTime(&ms, ev[2 * r].get(), ev[2 * r + 1].get()));
        stats[r].kernel_ms = ms; // trace + resolve of this rank (the other fields are render_tiles_t's)
    }
    if (stats && use_peer) stats[0].reserved |= 0x100u | (fell_back ? 0x200u : 0u);
    HIP_TRY(hipSetDevice(m.root->device));
    return copy_image_out("render_multi", m.root->rgba, m.root->linear, p.precision, m.npx, out_rgba8, out_linear_rgb);
}

// Release what the library keeps for the life of the process (today: the RCCL communicator sets of rttnw_render_multi).  Scenes
// are the caller's (rttnw_scene_destroy).  Safe to call more than once and with renders finished; also runs at exit.
extern "C" void rttnw_shutdown(void) { rt::destroy_comms(); }
