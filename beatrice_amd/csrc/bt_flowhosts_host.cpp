// bt_flowhosts_host.cpp — bt_flow_track_hosts_device: the endpoint table of a device-resident
// tracker state (bt_flowhosts.hip) on a stream, behind the updates it is to see;
// bt_flow_track_hosts_host, the same on the calling thread over a state in host memory; the
// scratch size.
#include <mutex>

#include "bt_ctx.h"
#include "bt_flowhosts.h"
#include "bt_hip_util.h"

using namespace bt;

namespace bt {

// e0 / e1: timing events recorded by the first / last kernel's own dispatch (bt_time_flow_hosts).
int run_flow_track_hosts(bt_ctx* c, const void* state, const bt_flow_hosts_opts* opts, const bt_flow_tcp_rec* tcp, void* scratch,
                         uint64_t scratch_bytes, const bt_flow_hosts_out* out, hipStream_t st, hipEvent_t e0, hipEvent_t e1) {
    FlowhostsArgs a;
    FkShadow sh{};
    char why[160];
    // before the context and any HIP call: every refusal is the same with and without a GPU
    const bool known = state && fk_known_state(state, &sh);
    if (!flowhosts_args(known ? &sh : nullptr, state, opts, tcp, scratch, scratch_bytes, out, &a, why, sizeof(why)))
        return set_error(BT_E_INVALID_ARGUMENT, "bt_flow_track_hosts_device: %s", why);
    if (!c) return set_error(BT_E_INVALID_ARGUMENT, "bt_flow_track_hosts_device: null context");
    HIP_TRY(hipSetDevice(c->device));
    if (!st) st = c->stream;
    const int rc = launch_flowhosts(a, st, e0, e1);
    if (rc) return set_error(rc, "flow hosts kernel launch failed: %s", hipGetErrorString(hipGetLastError()));
    return BT_OK;
}

}  // namespace bt

extern "C" int bt_flow_track_hosts_scratch_bytes(uint32_t flow_cap, uint32_t slots, uint64_t* bytes) {
    if (!bytes) return set_error(BT_E_INVALID_ARGUMENT, "bt_flow_track_hosts_scratch_bytes: null bytes");
    char why[128];
    uint32_t s = 0;
    if (!flowhosts_slots(slots, why, sizeof(why)) || !flowhosts_geometry(flow_cap, slots, &s, why, sizeof(why)))
        return set_error(BT_E_INVALID_ARGUMENT, "bt_flow_track_hosts_scratch_bytes: %s", why);
    *bytes = fh_scratch(flow_cap, s).total;
    return BT_OK;
}

extern "C" int bt_flow_track_hosts_device(bt_ctx* c, const void* state, const bt_flow_hosts_opts* opts, const bt_flow_tcp_rec* tcp,
                                          void* scratch, uint64_t scratch_bytes, const bt_flow_hosts_out* out, void* stream) {
    if (!c) return run_flow_track_hosts(nullptr, state, opts, tcp, scratch, scratch_bytes, out, nullptr, nullptr, nullptr);
    const bt::DeviceRestore keep_device;   // the caller's current device, restored on return
    std::lock_guard<std::mutex> lk(c->mu);
    return run_flow_track_hosts(c, state, opts, tcp, scratch, scratch_bytes, out, reinterpret_cast<hipStream_t>(stream), nullptr, nullptr);
}

extern "C" int bt_flow_track_hosts_host(const void* state, uint64_t state_bytes, const bt_flow_hosts_opts* opts, const bt_flow_tcp_rec* tcp,
                                        const bt_flow_hosts_out* out) {
    char why[160];
    FkHostState hs{};
    uint32_t slots = 0;
    if (!flowhosts_host_args(state, state_bytes, opts, tcp, out, &hs, &slots, why, sizeof(why)))
        return set_error(BT_E_INVALID_ARGUMENT, "bt_flow_track_hosts_host: %s", why);
    flowhosts_host(hs, slots, *opts, tcp, *out);
    return BT_OK;
}
