// bt_flowtcp_host.cpp — bt_flow_tcp_update_device: the per-flow TCP side table of a device-resident
// batch (bt_flowtcp.hip) on a stream, behind the flow table or tracker call that numbered the
// packets; bt_flow_tcp_update_host, the same on the calling thread; bt_flow_tcp_state.
#include <mutex>

#include "bt_ctx.h"
#include "bt_flowtcp.h"
#include "bt_hip_util.h"

using namespace bt;

namespace bt {

// e0 / e1: timing events recorded by the kernel's own dispatch (bt_time_flow_tcp).
int run_flow_tcp(bt_ctx* c, const bt_batch* frames, const uint32_t* flow_id, uint32_t table_flags, bt_flow_tcp_rec* tcp,
                 uint32_t flow_cap, bt_flow_tcp_result* result, hipStream_t st, hipEvent_t e0, hipEvent_t e1) {
    FlowtcpArgs a;
    char why[128];
    // before the context and any HIP call: every refusal is the same with and without a GPU
    if (!flowtcp_args(frames, flow_id, table_flags, tcp, flow_cap, result, &a, why, sizeof(why)))
        return set_error(BT_E_INVALID_ARGUMENT, "bt_flow_tcp_update_device: %s", why);
    if (!c) return set_error(BT_E_INVALID_ARGUMENT, "bt_flow_tcp_update_device: null context");
    HIP_TRY(hipSetDevice(c->device));
    if (!st) st = c->stream;
    // *result in stream order: zeros, then every block adds its sums (nothing more for n == 0)
    HIP_TRY(hipMemsetAsync(result, 0, sizeof(bt_flow_tcp_result), st));
    const int rc = launch_flowtcp(a, st, e0, e1);
    if (rc) return set_error(rc, "flow TCP kernel launch failed: %s", hipGetErrorString(hipGetLastError()));
    return BT_OK;
}

}  // namespace bt

extern "C" int bt_flow_tcp_update_device(bt_ctx* c, const bt_batch* frames, const uint32_t* flow_id, uint32_t table_flags,
                                         bt_flow_tcp_rec* tcp, uint32_t flow_cap, bt_flow_tcp_result* result, void* stream) {
    if (!c) return run_flow_tcp(nullptr, frames, flow_id, table_flags, tcp, flow_cap, result, nullptr, nullptr, nullptr);
    const bt::DeviceRestore keep_device;   // the caller's current device, restored on return
    std::lock_guard<std::mutex> lk(c->mu);
    return run_flow_tcp(c, frames, flow_id, table_flags, tcp, flow_cap, result, reinterpret_cast<hipStream_t>(stream), nullptr, nullptr);
}

extern "C" int bt_flow_tcp_update_host(const uint8_t* base, uint64_t bytes, const bt_pkt_desc* desc, uint32_t n, const uint32_t* flow_id,
                                       uint32_t table_flags, bt_flow_tcp_rec* tcp, uint32_t flow_cap, bt_flow_tcp_result* result) {
    char why[96];
    if (!flowtcp_host_args(base, desc, n, flow_id, table_flags, tcp, flow_cap, result, why, sizeof(why)))
        return set_error(BT_E_INVALID_ARGUMENT, "bt_flow_tcp_update_host: %s", why);
    flowtcp_host(base, bytes, desc, n, flow_id, table_flags, tcp, flow_cap, result);
    return BT_OK;
}

extern "C" int bt_flow_tcp_state(uint32_t flags_fwd, uint32_t flags_rev, uint32_t table_flags) {
    return flowtcp_state(flags_fwd, flags_rev, table_flags);
}
