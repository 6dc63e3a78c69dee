// bt_flowtcpseq_host.cpp — bt_flow_tcpseq_device: TCP segments classified per flow and direction
// against the sequence space (bt_flowtcpseq.hip) on a stream, behind the flow table or tracker call
// that numbered the packets; bt_flow_tcpseq_host, the same on the calling thread;
// bt_flow_tcpseq_scratch_bytes.
#include <mutex>

#include "beatrice_gpu_bench.h"
#include "bt_ctx.h"
#include "bt_flowtcpseq.h"
#include "bt_hip_util.h"

using namespace bt;

namespace bt {

// ev: nullptr, or launch_flowtcpseq's five timing events (bt_time_flow_tcpseq).
int run_flow_tcpseq(bt_ctx* c, const bt_batch* frames, const uint32_t* flow_id, const uint64_t* select, uint32_t table_flags,
                    bt_flow_tcpseq_rec* table, uint32_t flow_cap, void* scratch, uint64_t scratch_bytes, const bt_flow_tcpseq_out* out,
                    hipStream_t st, void* const* ev) {
    FlowtcpseqArgs a;
    char why[160];
    // before the context and any HIP call: every refusal is the same with and without a GPU
    if (!flowtcpseq_args(frames, flow_id, select, table_flags, table, flow_cap, scratch, scratch_bytes, out, &a, why, sizeof(why)))
        return set_error(BT_E_INVALID_ARGUMENT, "bt_flow_tcpseq_device: %s", why);
    if (!c) return set_error(BT_E_INVALID_ARGUMENT, "bt_flow_tcpseq_device: null context");
    HIP_TRY(hipSetDevice(c->device));
    if (!st) st = c->stream;
    // in stream order: zeros into *result, then the kernels (nothing more for n == 0)
    HIP_TRY(hipMemsetAsync(out->result, 0, sizeof(bt_flow_tcpseq_result), st));
    const int rc = launch_flowtcpseq(a, st, ev);
    if (rc) return set_error(rc, "flow tcpseq kernel launch failed: %s", hipGetErrorString(hipGetLastError()));
    return BT_OK;
}

}  // namespace bt

extern "C" int bt_flow_tcpseq_scratch_bytes(uint32_t n, uint32_t flow_cap, uint64_t* bytes) {
    (void)flow_cap;   // the scratch follows n alone; the argument keeps the family's shape
    if (!bytes) return set_error(BT_E_INVALID_ARGUMENT, "bt_flow_tcpseq_scratch_bytes: null bytes");
    *bytes = fts_layout(n).total;
    return BT_OK;
}

extern "C" int bt_flow_tcpseq_device(bt_ctx* c, const bt_batch* frames, const uint32_t* flow_id, const uint64_t* select,
                                     uint32_t table_flags, bt_flow_tcpseq_rec* table, uint32_t flow_cap, void* scratch,
                                     uint64_t scratch_bytes, const bt_flow_tcpseq_out* out, void* stream) {
    if (!c) return run_flow_tcpseq(nullptr, frames, flow_id, select, table_flags, table, flow_cap, scratch, scratch_bytes, out, nullptr, nullptr);
    const bt::DeviceRestore keep_device;   // the caller's current device, restored on return
    std::lock_guard<std::mutex> lk(c->mu);
    return run_flow_tcpseq(c, frames, flow_id, select, table_flags, table, flow_cap, scratch, scratch_bytes, out,
                           reinterpret_cast<hipStream_t>(stream), nullptr);
}

extern "C" int bt_flow_tcpseq_host(const uint8_t* base, uint64_t bytes, const bt_pkt_desc* desc, uint32_t n, const uint32_t* flow_id,
                                   const uint64_t* select, uint32_t table_flags, bt_flow_tcpseq_rec* table, uint32_t flow_cap,
                                   const bt_flow_tcpseq_out* out) {
    char why[160];
    if (!flowtcpseq_host_args(base, desc, n, flow_id, select, table_flags, table, flow_cap, out, why, sizeof(why)))
        return set_error(BT_E_INVALID_ARGUMENT, "bt_flow_tcpseq_host: %s", why);
    flowtcpseq_host(base, bytes, desc, n, flow_id, select, table_flags, table, flow_cap, out);
    return BT_OK;
}
