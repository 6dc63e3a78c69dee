// bt_flowmark_host.cpp — bt_flow_mark_update_device: the per-flow mark side table (bt_flowmark.hip)
// raised by a verdict on a stream, behind the flow table or tracker call that numbered the packets;
// bt_flow_mark_select_device: the selection of every packet whose flow carries a mark;
// bt_flow_mark_update_host / bt_flow_mark_select_host, the same on the calling thread.
#include <mutex>

#include "bt_ctx.h"
#include "bt_flowmark.h"
#include "bt_hip_util.h"

using namespace bt;

namespace bt {

// e0 / e1: timing events recorded by the kernel's own dispatch (bt_time_flow_mark).
int run_flow_mark(bt_ctx* c, const bt_batch* frames, const uint32_t* flow_id, const uint64_t* hit, const bt_flow_mark_update* upd,
                  bt_flow_mark_rec* table, uint32_t flow_cap, bt_flow_mark_result* result, hipStream_t st, hipEvent_t e0, hipEvent_t e1) {
    FlowmarkArgs a;
    char why[128];
    // before the context and any HIP call: every refusal is the same with and without a GPU
    if (!flowmark_args(frames, flow_id, hit, upd, table, flow_cap, result, &a, why, sizeof(why)))
        return set_error(BT_E_INVALID_ARGUMENT, "bt_flow_mark_update_device: %s", why);
    if (!c) return set_error(BT_E_INVALID_ARGUMENT, "bt_flow_mark_update_device: null context");
    HIP_TRY(hipSetDevice(c->device));
    if (!st) st = c->stream;
    // *result in stream order: zeros, then every block adds its sums (nothing more for n == 0)
    HIP_TRY(hipMemsetAsync(result, 0, sizeof(bt_flow_mark_result), st));
    const int rc = launch_flowmark(a, st, e0, e1);
    if (rc) return set_error(rc, "flow mark kernel launch failed: %s", hipGetErrorString(hipGetLastError()));
    return BT_OK;
}

int run_flow_mark_select(bt_ctx* c, const uint32_t* flow_id, uint32_t n, const bt_flow_mark_rec* table, uint32_t flow_cap,
                         const bt_flow_mark_select_opts* opts, const uint64_t* base, uint64_t* out, bt_flow_mark_select_result* result,
                         hipStream_t st, hipEvent_t e0, hipEvent_t e1) {
    FlowmarkSelArgs a;
    char why[128];
    if (!flowmark_sel_args(flow_id, n, table, flow_cap, opts, base, out, result, &a, why, sizeof(why)))
        return set_error(BT_E_INVALID_ARGUMENT, "bt_flow_mark_select_device: %s", why);
    if (!c) return set_error(BT_E_INVALID_ARGUMENT, "bt_flow_mark_select_device: null context");
    HIP_TRY(hipSetDevice(c->device));
    if (!st) st = c->stream;
    HIP_TRY(hipMemsetAsync(result, 0, sizeof(bt_flow_mark_select_result), st));
    const int rc = launch_flowmark_select(a, st, e0, e1);
    if (rc) return set_error(rc, "flow mark select kernel launch failed: %s", hipGetErrorString(hipGetLastError()));
    return BT_OK;
}

}  // namespace bt

extern "C" int bt_flow_mark_update_device(bt_ctx* c, const bt_batch* frames, const uint32_t* flow_id, const uint64_t* hit,
                                          const bt_flow_mark_update* upd, bt_flow_mark_rec* table, uint32_t flow_cap,
                                          bt_flow_mark_result* result, void* stream) {
    if (!c) return run_flow_mark(nullptr, frames, flow_id, hit, upd, table, flow_cap, result, nullptr, nullptr, nullptr);
    const bt::DeviceRestore keep_device;   // the caller's current device, restored on return
    std::lock_guard<std::mutex> lk(c->mu);
    return run_flow_mark(c, frames, flow_id, hit, upd, table, flow_cap, result, reinterpret_cast<hipStream_t>(stream), nullptr, nullptr);
}

extern "C" int bt_flow_mark_select_device(bt_ctx* c, const uint32_t* flow_id, uint32_t n, const bt_flow_mark_rec* table, uint32_t flow_cap,
                                          const bt_flow_mark_select_opts* opts, const uint64_t* base, uint64_t* out,
                                          bt_flow_mark_select_result* result, void* stream) {
    if (!c) return run_flow_mark_select(nullptr, flow_id, n, table, flow_cap, opts, base, out, result, nullptr, nullptr, nullptr);
    const bt::DeviceRestore keep_device;   // the caller's current device, restored on return
    std::lock_guard<std::mutex> lk(c->mu);
    return run_flow_mark_select(c, flow_id, n, table, flow_cap, opts, base, out, result, reinterpret_cast<hipStream_t>(stream), nullptr,
                                nullptr);
}

extern "C" int bt_flow_mark_update_host(const bt_pkt_desc* desc, uint32_t n, const uint32_t* flow_id, const uint64_t* hit,
                                        const bt_flow_mark_update* upd, bt_flow_mark_rec* table, uint32_t flow_cap,
                                        bt_flow_mark_result* result) {
    char why[96];
    if (!flowmark_host_args(desc, n, flow_id, hit, upd, table, flow_cap, result, why, sizeof(why)))
        return set_error(BT_E_INVALID_ARGUMENT, "bt_flow_mark_update_host: %s", why);
    flowmark_host(desc, n, flow_id, hit, upd, table, flow_cap, result);
    return BT_OK;
}

extern "C" int bt_flow_mark_select_host(const uint32_t* flow_id, uint32_t n, const bt_flow_mark_rec* table, uint32_t flow_cap,
                                        const bt_flow_mark_select_opts* opts, const uint64_t* base, uint64_t* out,
                                        bt_flow_mark_select_result* result) {
    FlowmarkSelArgs a;
    char why[96];
    if (!flowmark_sel_args(flow_id, n, table, flow_cap, opts, base, out, result, &a, why, sizeof(why)))
        return set_error(BT_E_INVALID_ARGUMENT, "bt_flow_mark_select_host: %s", why);
    flowmark_sel_host(a);
    return BT_OK;
}
