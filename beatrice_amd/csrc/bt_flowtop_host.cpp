// bt_flowtop_host.cpp — bt_flow_track_top_device: the top-K query over a device-resident tracker
// state (bt_flowtop.hip) on a stream, behind the updates it is to see; bt_flow_track_top_host, the
// same on the calling thread over a state in host memory; the scratch size.
#include <mutex>

#include "bt_ctx.h"
#include "bt_flowtop.h"
#include "bt_hip_util.h"

using namespace bt;

namespace bt {

// e0 / e1: timing events recorded by the first / last kernel's own dispatch (bt_time_flow_top).
int run_flow_track_top(bt_ctx* c, const void* state, const bt_flow_top_opts* opts, const bt_flow_tcp_rec* tcp, void* scratch,
                       uint64_t scratch_bytes, const bt_flow_top_out* out, hipStream_t st, hipEvent_t e0, hipEvent_t e1) {
    FlowtopArgs a;
    FkShadow sh{};
    char why[160];
    // before the context and any HIP call: every refusal is the same with and without a GPU
    const bool known = state && fk_known_state(state, &sh);
    if (!flowtop_args(known ? &sh : nullptr, state, opts, tcp, scratch, scratch_bytes, out, &a, why, sizeof(why)))
        return set_error(BT_E_INVALID_ARGUMENT, "bt_flow_track_top_device: %s", why);
    if (!c) return set_error(BT_E_INVALID_ARGUMENT, "bt_flow_track_top_device: null context");
    HIP_TRY(hipSetDevice(c->device));
    if (!st) st = c->stream;
    const int rc = launch_flowtop(a, st, e0, e1);
    if (rc) return set_error(rc, "flow top kernel launch failed: %s", hipGetErrorString(hipGetLastError()));
    return BT_OK;
}

}  // namespace bt

extern "C" int bt_flow_track_top_scratch_bytes(uint32_t flow_cap, uint32_t k, uint64_t* bytes) {
    if (!bytes) return set_error(BT_E_INVALID_ARGUMENT, "bt_flow_track_top_scratch_bytes: null bytes");
    if (k > BT_FLOW_TOP_MAX_K) return set_error(BT_E_INVALID_ARGUMENT, "bt_flow_track_top_scratch_bytes: k above BT_FLOW_TOP_MAX_K");
    char why[128];
    bt_flow_track_sizes l{};
    if (!fk_layout(flow_cap, flow_cap > (1u << 30) ? 1u << 31 : 0u, &l, why, sizeof(why)))
        return set_error(BT_E_INVALID_ARGUMENT, "bt_flow_track_top_scratch_bytes: %s", why);
    *bytes = ftop_scratch(flow_cap, k).total;
    return BT_OK;
}

extern "C" int bt_flow_track_top_device(bt_ctx* c, const void* state, const bt_flow_top_opts* opts, const bt_flow_tcp_rec* tcp,
                                        void* scratch, uint64_t scratch_bytes, const bt_flow_top_out* out, void* stream) {
    if (!c) return run_flow_track_top(nullptr, state, opts, tcp, scratch, scratch_bytes, out, nullptr, nullptr, nullptr);
    const bt::DeviceRestore keep_device;   // the caller's current device, restored on return
    std::lock_guard<std::mutex> lk(c->mu);
    return run_flow_track_top(c, state, opts, tcp, scratch, scratch_bytes, out, reinterpret_cast<hipStream_t>(stream), nullptr, nullptr);
}

extern "C" int bt_flow_track_top_host(const void* state, uint64_t state_bytes, const bt_flow_top_opts* opts, const bt_flow_tcp_rec* tcp,
                                      const bt_flow_top_out* out) {
    char why[160];
    FkHostState hs{};
    if (!flowtop_host_args(state, state_bytes, opts, tcp, out, &hs, why, sizeof(why)))
        return set_error(BT_E_INVALID_ARGUMENT, "bt_flow_track_top_host: %s", why);
    flowtop_host(hs, *opts, tcp, *out);
    return BT_OK;
}
