// bt_flowstat_host.cpp — bt_flow_stat_update_device: the per-flow statistics side table of a
// device-resident batch (bt_flowstat.hip) on a stream, behind the flow table or tracker call that
// numbered the packets; bt_flow_stat_update_host, the same on the calling thread; bt_flow_stat_rtt;
// bt_flow_track_side_move_device / _host: any side table through an expire by the expire's remap.
#include <mutex>

#include "bt_ctx.h"
#include "bt_flowstat.h"
#include "bt_hip_util.h"

using namespace bt;

namespace bt {

// e0 / e1: timing events recorded by the kernel's own dispatch (bt_time_flow_stat).
int run_flow_stat(bt_ctx* c, const bt_batch* frames, const uint32_t* flow_id, uint32_t table_flags, const bt_flow_track_update* upd,
                  bt_flow_stat_rec* stat, uint32_t flow_cap, bt_flow_stat_result* result, hipStream_t st, hipEvent_t e0, hipEvent_t e1) {
    FlowstatArgs a;
    char why[128];
    // before the context and any HIP call: every refusal is the same with and without a GPU
    if (!flowstat_args(frames, flow_id, table_flags, upd, stat, flow_cap, result, &a, why, sizeof(why)))
        return set_error(BT_E_INVALID_ARGUMENT, "bt_flow_stat_update_device: %s", why);
    if (!c) return set_error(BT_E_INVALID_ARGUMENT, "bt_flow_stat_update_device: null context");
    HIP_TRY(hipSetDevice(c->device));
    if (!st) st = c->stream;
    // *result in stream order: zeros, then every block adds its sums (nothing more for n == 0)
    HIP_TRY(hipMemsetAsync(result, 0, sizeof(bt_flow_stat_result), st));
    const int rc = launch_flowstat(a, st, e0, e1);
    if (rc) return set_error(rc, "flow statistics kernel launch failed: %s", hipGetErrorString(hipGetLastError()));
    return BT_OK;
}

}  // namespace bt

extern "C" int bt_flow_stat_update_device(bt_ctx* c, const bt_batch* frames, const uint32_t* flow_id, uint32_t table_flags,
                                          const bt_flow_track_update* upd, bt_flow_stat_rec* stat, uint32_t flow_cap,
                                          bt_flow_stat_result* result, void* stream) {
    if (!c) return run_flow_stat(nullptr, frames, flow_id, table_flags, upd, stat, flow_cap, result, nullptr, nullptr, nullptr);
    const bt::DeviceRestore keep_device;   // the caller's current device, restored on return
    std::lock_guard<std::mutex> lk(c->mu);
    return run_flow_stat(c, frames, flow_id, table_flags, upd, stat, flow_cap, result, reinterpret_cast<hipStream_t>(stream), nullptr,
                         nullptr);
}

extern "C" int bt_flow_stat_update_host(const uint8_t* base, uint64_t bytes, const bt_pkt_desc* desc, uint32_t n, const uint32_t* flow_id,
                                        uint32_t table_flags, const bt_flow_track_update* upd, bt_flow_stat_rec* stat, uint32_t flow_cap,
                                        bt_flow_stat_result* result) {
    char why[96];
    if (!flowstat_host_args(base, desc, n, flow_id, table_flags, upd, stat, flow_cap, result, why, sizeof(why)))
        return set_error(BT_E_INVALID_ARGUMENT, "bt_flow_stat_update_host: %s", why);
    flowstat_host(base, bytes, desc, n, flow_id, table_flags, upd, stat, flow_cap, result);
    return BT_OK;
}

extern "C" int bt_flow_stat_rtt(const bt_flow_stat_rec* rec, bt_flow_stat_rtt_out* out) {
    if (!rec || !out) return set_error(BT_E_INVALID_ARGUMENT, "bt_flow_stat_rtt: null argument");
    flowstat_rtt(*rec, out);
    return BT_OK;
}

extern "C" int bt_flow_track_side_move_scratch_bytes(uint32_t flow_cap, uint32_t rec_bytes, uint64_t* bytes) {
    if (!bytes) return set_error(BT_E_INVALID_ARGUMENT, "bt_flow_track_side_move_scratch_bytes: null bytes");
    if (!flowside_rec_bytes_ok(rec_bytes))
        return set_error(BT_E_INVALID_ARGUMENT, "bt_flow_track_side_move_scratch_bytes: rec_bytes is not a multiple of 4 in 4 .. 256");
    *bytes = fs_scratch(flow_cap, rec_bytes).total;
    return BT_OK;
}

extern "C" int bt_flow_track_side_move_device(bt_ctx* c, const bt_flow_side_move* m, void* scratch, uint64_t scratch_bytes, void* stream) {
    FlowsideArgs a;
    char why[128];
    if (!flowside_args(m, scratch, scratch_bytes, &a, why, sizeof(why)))
        return set_error(BT_E_INVALID_ARGUMENT, "bt_flow_track_side_move_device: %s", why);
    if (!c) return set_error(BT_E_INVALID_ARGUMENT, "bt_flow_track_side_move_device: null context");
    const bt::DeviceRestore keep_device;   // the caller's current device, restored on return
    std::lock_guard<std::mutex> lk(c->mu);
    HIP_TRY(hipSetDevice(c->device));
    hipStream_t st = stream ? reinterpret_cast<hipStream_t>(stream) : c->stream;
    const int rc = launch_flowside(a, st);
    if (rc) return set_error(rc, "side move kernel launch failed: %s", hipGetErrorString(hipGetLastError()));
    return BT_OK;
}

extern "C" int bt_flow_track_side_move_host(const bt_flow_side_move* m) {
    char why[96];
    if (!flowside_common_args(m, why, sizeof(why))) return set_error(BT_E_INVALID_ARGUMENT, "bt_flow_track_side_move_host: %s", why);
    flowside_host(m);
    return BT_OK;
}
