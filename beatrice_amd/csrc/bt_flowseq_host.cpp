// bt_flowseq_host.cpp — bt_flow_seq_device: every selected packet's position inside its flow and
// the per-flow cut-off (bt_flowseq.hip) on a stream, behind the flow table or tracker call that
// numbered the packets; bt_flow_seq_host, the same on the calling thread; bt_flow_seq_scratch_bytes.
#include <mutex>

#include "bt_ctx.h"
#include "bt_flowseq.h"
#include "bt_hip_util.h"

using namespace bt;

namespace bt {

// ev: nullptr, or launch_flowseq's five timing events (bt_time_flow_seq).
int run_flow_seq(bt_ctx* c, const bt_batch* frames, const uint32_t* flow_id, const uint64_t* select, const bt_flow_seq_opts* opts,
                 bt_flow_seq_rec* table, uint32_t flow_cap, const bt_flow_seq_out* out, void* scratch, uint64_t scratch_bytes,
                 bt_flow_seq_result* result, hipStream_t st, void* const* ev) {
    FlowseqArgs a;
    char why[128];
    // before the context and any HIP call: every refusal is the same with and without a GPU
    if (!flowseq_args(frames, flow_id, select, opts, table, flow_cap, out, scratch, scratch_bytes, result, &a, why, sizeof(why)))
        return set_error(BT_E_INVALID_ARGUMENT, "bt_flow_seq_device: %s", why);
    if (!c) return set_error(BT_E_INVALID_ARGUMENT, "bt_flow_seq_device: null context");
    HIP_TRY(hipSetDevice(c->device));
    if (!st) st = c->stream;
    // *result in stream order: zeros, then every wave adds its sums (nothing more for n == 0)
    HIP_TRY(hipMemsetAsync(result, 0, sizeof(bt_flow_seq_result), st));
    const int rc = launch_flowseq(a, st, ev);
    if (rc) return set_error(rc, "flow seq kernel launch failed: %s", hipGetErrorString(hipGetLastError()));
    return BT_OK;
}

}  // namespace bt

extern "C" int bt_flow_seq_scratch_bytes(uint32_t n, uint32_t flow_cap, uint64_t* bytes) {
    if (!bytes) return set_error(BT_E_INVALID_ARGUMENT, "bt_flow_seq_scratch_bytes: null bytes");
    *bytes = fs_layout(n, flow_cap).total;
    return BT_OK;
}

extern "C" int bt_flow_seq_device(bt_ctx* c, const bt_batch* frames, const uint32_t* flow_id, const uint64_t* select,
                                  const bt_flow_seq_opts* opts, bt_flow_seq_rec* table, uint32_t flow_cap, const bt_flow_seq_out* out,
                                  void* scratch, uint64_t scratch_bytes, bt_flow_seq_result* result, void* stream) {
    if (!c) return run_flow_seq(nullptr, frames, flow_id, select, opts, table, flow_cap, out, scratch, scratch_bytes, result, nullptr, nullptr);
    const bt::DeviceRestore keep_device;   // the caller's current device, restored on return
    std::lock_guard<std::mutex> lk(c->mu);
    return run_flow_seq(c, frames, flow_id, select, opts, table, flow_cap, out, scratch, scratch_bytes, result,
                        reinterpret_cast<hipStream_t>(stream), nullptr);
}

extern "C" int bt_flow_seq_host(const bt_pkt_desc* desc, uint32_t n, const uint32_t* flow_id, const uint64_t* select,
                                const bt_flow_seq_opts* opts, bt_flow_seq_rec* table, uint32_t flow_cap, const bt_flow_seq_out* out,
                                bt_flow_seq_result* result) {
    char why[96];
    if (!flowseq_host_args(desc, n, flow_id, select, opts, table, flow_cap, out, result, why, sizeof(why)))
        return set_error(BT_E_INVALID_ARGUMENT, "bt_flow_seq_host: %s", why);
    flowseq_host(desc, n, flow_id, select, opts, table, flow_cap, out, result);
    return BT_OK;
}
