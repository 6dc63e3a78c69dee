// bt_flowtab_host.cpp — bt_flow_table_device: the flow table of a device-resident batch
// (bt_flowtab.hip) over the caller's scratch on a stream, right behind the parse+filter pass that
// wrote the selection; bt_flow_table_scratch_bytes; and bt_flow_table_host, the same group-by on
// the calling thread.
#include <mutex>

#include "bt_ctx.h"
#include "bt_hip_util.h"

using namespace bt;

namespace bt {

// e0 / e1: timing events recorded by the first / last kernel's own dispatch (bt_time_flow_table).
int run_flow_table(bt_ctx* c, const bt_batch* frames, const uint64_t* select, const bt_flow_table_opts* opts, void* scratch,
                   uint64_t scratch_bytes, const bt_flow_table_out* out, hipStream_t st, hipEvent_t e0, hipEvent_t e1) {
    FlowtabArgs a;
    char why[128];
    // before the context and any HIP call: every refusal is the same with and without a GPU
    if (!flowtab_args(frames, select, opts, scratch, scratch_bytes, out, &a, why, sizeof(why)))
        return set_error(BT_E_INVALID_ARGUMENT, "bt_flow_table_device: %s", why);
    if (!c) return set_error(BT_E_INVALID_ARGUMENT, "bt_flow_table_device: null context");
    HIP_TRY(hipSetDevice(c->device));
    if (!st) st = c->stream;
    if (a.n == 0) {   // nothing to launch: *result is still written in stream order
        HIP_TRY(hipMemsetAsync(out->result, 0, sizeof(bt_flow_table_result), st));
        HIP_TRY(hipMemsetD32Async(reinterpret_cast<hipDeviceptr_t>(&out->result->slots), (int)a.slots, 1, st));
        return BT_OK;
    }
    const int rc = launch_flowtab(a, st, e0, e1);
    if (rc) return set_error(rc, "flow table kernel launch failed: %s", hipGetErrorString(hipGetLastError()));
    return BT_OK;
}

}  // namespace bt

extern "C" int bt_flow_table_scratch_bytes(uint32_t n, uint32_t slots, uint64_t* bytes) {
    if (!bytes) return set_error(BT_E_INVALID_ARGUMENT, "bt_flow_table_scratch_bytes: null bytes");
    const bt_flow_table_opts o{0u, slots, 0u, 0u};
    char why[96];
    uint32_t s = 0;
    if (!flowtab_opts(&o, n, &s, why, sizeof(why))) return set_error(BT_E_INVALID_ARGUMENT, "bt_flow_table_scratch_bytes: %s", why);
    *bytes = ft_layout(n, s).total;
    return BT_OK;
}

extern "C" int bt_flow_table_device(bt_ctx* c, const bt_batch* frames, const uint64_t* select, const bt_flow_table_opts* opts,
                                    void* scratch, uint64_t scratch_bytes, const bt_flow_table_out* out, void* stream) {
    if (!c) return run_flow_table(nullptr, frames, select, opts, scratch, scratch_bytes, out, nullptr, nullptr, nullptr);
    const bt::DeviceRestore keep_device;   // the caller's current device, restored on return
    std::lock_guard<std::mutex> lk(c->mu);
    return run_flow_table(c, frames, select, opts, scratch, scratch_bytes, out, reinterpret_cast<hipStream_t>(stream), nullptr,
                          nullptr);
}

extern "C" int bt_flow_table_host(const uint8_t* base, uint64_t bytes, const bt_pkt_desc* desc, uint32_t n,
                                  const uint64_t* select, const bt_flow_table_opts* opts, uint32_t* flow_id, bt_flow_rec* flows,
                                  bt_flow_table_result* result) {
    char why[96];
    uint32_t slots = 0;
    if (!flowtab_opts(opts, n, &slots, why, sizeof(why))) return set_error(BT_E_INVALID_ARGUMENT, "bt_flow_table_host: %s", why);
    if (!result) return set_error(BT_E_INVALID_ARGUMENT, "bt_flow_table_host: null result");
    if (n && (!base || !desc)) return set_error(BT_E_INVALID_ARGUMENT, "bt_flow_table_host: null base / desc");
    if (!flows && opts->flow_cap) return set_error(BT_E_INVALID_ARGUMENT, "bt_flow_table_host: null flows with flow_cap != 0");
    flowtab_host(base, bytes, desc, n, select, opts->flags, slots, opts->flow_cap, flow_id, flows, result);
    return BT_OK;
}
