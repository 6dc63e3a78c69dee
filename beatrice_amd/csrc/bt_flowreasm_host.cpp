// bt_flowreasm_host.cpp — bt_flow_reasm_device: a payload pattern matched per flow and direction
// over the TCP segments in sequence order (bt_flowreasm.hip) on a stream, behind the
// bt_flow_tcpseq_device call that placed them; bt_flow_reasm_host, the same on the calling thread;
// bt_flow_reasm_scratch_bytes.
#include <mutex>

#include "beatrice_gpu_bench.h"
#include "bt_ctx.h"
#include "bt_flowreasm.h"
#include "bt_hip_util.h"

using namespace bt;

namespace bt {

// ev: nullptr, or launch_flowreasm's seven timing events (bt_time_flow_reasm).
int run_flow_reasm(bt_ctx* c, const bt_batch* frames, const uint32_t* flow_id, const uint64_t* select, const int64_t* off,
                   uint32_t table_flags, const void* pattern, const void* pattern_device, uint32_t pattern_bytes,
                   bt_flow_reasm_rec* table, uint32_t flow_cap, void* scratch, uint64_t scratch_bytes, const bt_flow_reasm_out* out,
                   hipStream_t st, void* const* ev) {
    FlowreasmArgs a;
    char why[160];
    // before the context and any HIP call: every refusal is the same with and without a GPU
    if (const int rc = flowreasm_args(frames, flow_id, select, off, table_flags, pattern, pattern_device, pattern_bytes, table, flow_cap,
                                      scratch, scratch_bytes, out, &a, why, sizeof(why)))
        return set_error(rc, "bt_flow_reasm_device: %s", why);
    if (!c) return set_error(BT_E_INVALID_ARGUMENT, "bt_flow_reasm_device: null context");
    HIP_TRY(hipSetDevice(c->device));
    if (!st) st = c->stream;
    // in stream order: zeros into *result and the flows' bits, then the kernels (nothing more for n == 0)
    HIP_TRY(hipMemsetAsync(out->result, 0, sizeof(bt_flow_reasm_result), st));
    if (a.n && a.bits_bytes) HIP_TRY(hipMemsetAsync(a.bits, 0, a.bits_bytes, st));
    const int rc = launch_flowreasm(a, st, ev);
    if (rc) return set_error(rc, "flow reasm kernel launch failed: %s", hipGetErrorString(hipGetLastError()));
    return BT_OK;
}

}  // namespace bt

extern "C" int bt_flow_reasm_scratch_bytes(uint32_t n, uint32_t flow_cap, uint64_t* bytes) {
    if (!bytes) return set_error(BT_E_INVALID_ARGUMENT, "bt_flow_reasm_scratch_bytes: null bytes");
    *bytes = fr_layout(n, flow_cap).total;
    return BT_OK;
}

extern "C" int bt_flow_reasm_device(bt_ctx* c, const bt_batch* frames, const uint32_t* flow_id, const uint64_t* select,
                                    const int64_t* off, uint32_t table_flags, const void* pattern, const void* pattern_device,
                                    uint32_t pattern_bytes, bt_flow_reasm_rec* table, uint32_t flow_cap, void* scratch,
                                    uint64_t scratch_bytes, const bt_flow_reasm_out* out, void* stream) {
    if (!c)
        return run_flow_reasm(nullptr, frames, flow_id, select, off, table_flags, pattern, pattern_device, pattern_bytes, table,
                              flow_cap, scratch, scratch_bytes, out, nullptr, nullptr);
    const bt::DeviceRestore keep_device;   // the caller's current device, restored on return
    std::lock_guard<std::mutex> lk(c->mu);
    return run_flow_reasm(c, frames, flow_id, select, off, table_flags, pattern, pattern_device, pattern_bytes, table, flow_cap,
                          scratch, scratch_bytes, out, reinterpret_cast<hipStream_t>(stream), nullptr);
}

extern "C" int bt_flow_reasm_host(const uint8_t* base, uint64_t bytes, const bt_pkt_desc* desc, uint32_t n, const uint32_t* flow_id,
                                  const uint64_t* select, const int64_t* off, uint32_t table_flags, const void* pattern,
                                  uint32_t pattern_bytes, bt_flow_reasm_rec* table, uint32_t flow_cap, const bt_flow_reasm_out* out) {
    char why[160];
    FstPattern p;
    if (const int rc = flowreasm_host_args(base, desc, n, flow_id, select, off, table_flags, pattern, pattern_bytes, table, flow_cap,
                                           out, &p, why, sizeof(why)))
        return set_error(rc, "bt_flow_reasm_host: %s", why);
    flowreasm_host(base, bytes, desc, n, flow_id, select, off, table_flags, pattern, p, table, flow_cap, out);
    return BT_OK;
}
