// bt_flowfollow_host.cpp — bt_flow_follow_device: bt_flow_reasm_device's work with the delivered
// bytes, the runs between holes and each packet's place exported (bt_flowfollow.hip between the
// stages of bt_flowreasm.hip) on a stream; bt_flow_follow_host, the same on the calling thread;
// bt_flow_follow_scratch_bytes.
#include <mutex>

#include "beatrice_gpu_bench.h"
#include "bt_ctx.h"
#include "bt_flowfollow.h"
#include "bt_hip_util.h"

using namespace bt;

namespace bt {

// ev: nullptr, or nine timing events (bt_time_flow_follow): launch_flowreasm's first five, the start
// of the follow's sums, of its copy and of the commit, and the end of the last kernel.
int run_flow_follow(bt_ctx* c, const bt_batch* frames, const uint32_t* flow_id, const uint64_t* select, const int64_t* off,
                    uint32_t table_flags, const void* pattern, const void* pattern_device, uint32_t pattern_bytes,
                    bt_flow_reasm_rec* table, uint32_t flow_cap, void* scratch, uint64_t scratch_bytes, const bt_flow_reasm_out* out,
                    const bt_flow_follow_out* fo, hipStream_t st, void* const* ev) {
    FlowreasmArgs a;
    FlowfollowArgs f;
    char why[160];
    // before the context and any HIP call: every refusal is the same with and without a GPU
    if (const int rc = flowfollow_args(frames, flow_id, select, off, table_flags, pattern, pattern_device, pattern_bytes, table, flow_cap,
                                       scratch, scratch_bytes, out, fo, &a, &f, why, sizeof(why)))
        return set_error(rc, "bt_flow_follow_device: %s", why);
    if (!c) return set_error(BT_E_INVALID_ARGUMENT, "bt_flow_follow_device: null context");
    HIP_TRY(hipSetDevice(c->device));
    if (!st) st = c->stream;
    const bool with = pattern != nullptr;
    // in stream order: zeros into *result and the flows' bits, then the kernels (for n == 0 the two results and nothing more)
    HIP_TRY(hipMemsetAsync(out->result, 0, sizeof(bt_flow_reasm_result), st));
    if (a.n == 0 || a.nchunks == 0) {
        HIP_TRY(hipMemsetAsync(fo->result, 0, sizeof(bt_flow_follow_result), st));
        return BT_OK;
    }
    if (with && a.bits_bytes) HIP_TRY(hipMemsetAsync(a.bits, 0, a.bits_bytes, st));
    if (fo->place) HIP_TRY(hipMemsetAsync(fo->place, 0xFF, (uint64_t)a.n * 8u, st));
    const FsPair* sorted = nullptr;
    int rc = launch_flowreasm_front(a, st, ev, &sorted);
    if (!rc && with) rc = launch_flowreasm_match(a, st, ev ? ev[4] : nullptr);
    if (rc) return set_error(rc, "flow follow kernel launch failed: %s", hipGetErrorString(hipGetLastError()));
    if (!with) {   // what only the match writes and Commit reads; the hit words behind the classification's read of select
        if (ev) HIP_TRY(hipEventRecord(reinterpret_cast<hipEvent_t>(ev[4]), st));
        HIP_TRY(hipMemsetAsync(a.hitw, 0, (uint64_t)a.ntiles * 8u, st));
        HIP_TRY(hipMemsetAsync(a.dfin, 0, (uint64_t)a.n * 8u, st));
        if (a.hit) HIP_TRY(hipMemsetAsync(a.hit, 0, (uint64_t)a.ntiles * 8u, st));
    }
    f.s = sorted;
    rc = launch_flowfollow(f, st, ev ? ev[5] : nullptr, ev ? ev[6] : nullptr);
    if (!rc) rc = launch_flowreasm_commit(a, sorted, st, ev ? ev[7] : nullptr, ev ? ev[8] : nullptr);
    if (rc) return set_error(rc, "flow follow kernel launch failed: %s", hipGetErrorString(hipGetLastError()));
    return BT_OK;
}

}  // namespace bt

extern "C" int bt_flow_follow_scratch_bytes(uint32_t n, uint32_t flow_cap, uint64_t* bytes) {
    if (!bytes) return set_error(BT_E_INVALID_ARGUMENT, "bt_flow_follow_scratch_bytes: null bytes");
    *bytes = ff_layout(n, flow_cap).total;
    return BT_OK;
}

extern "C" int bt_flow_follow_device(bt_ctx* c, const bt_batch* frames, const uint32_t* flow_id, const uint64_t* select,
                                     const int64_t* off, uint32_t table_flags, const void* pattern, const void* pattern_device,
                                     uint32_t pattern_bytes, bt_flow_reasm_rec* table, uint32_t flow_cap, void* scratch,
                                     uint64_t scratch_bytes, const bt_flow_reasm_out* out, const bt_flow_follow_out* fo, void* stream) {
    if (!c)
        return run_flow_follow(nullptr, frames, flow_id, select, off, table_flags, pattern, pattern_device, pattern_bytes, table,
                               flow_cap, scratch, scratch_bytes, out, fo, nullptr, nullptr);
    const bt::DeviceRestore keep_device;   // the caller's current device, restored on return
    std::lock_guard<std::mutex> lk(c->mu);
    return run_flow_follow(c, frames, flow_id, select, off, table_flags, pattern, pattern_device, pattern_bytes, table, flow_cap,
                           scratch, scratch_bytes, out, fo, reinterpret_cast<hipStream_t>(stream), nullptr);
}

extern "C" int bt_flow_follow_host(const uint8_t* base, uint64_t bytes, const bt_pkt_desc* desc, uint32_t n, const uint32_t* flow_id,
                                   const uint64_t* select, const int64_t* off, uint32_t table_flags, const void* pattern,
                                   uint32_t pattern_bytes, bt_flow_reasm_rec* table, uint32_t flow_cap, const bt_flow_reasm_out* out,
                                   const bt_flow_follow_out* fo) {
    char why[160];
    FstPattern p;
    bool with = false;
    if (const int rc = flowfollow_host_args(base, bytes, desc, n, flow_id, select, off, table_flags, pattern, pattern_bytes, table,
                                            flow_cap, out, fo, &p, &with, why, sizeof(why)))
        return set_error(rc, "bt_flow_follow_host: %s", why);
    flowfollow_host(base, bytes, desc, n, flow_id, select, off, table_flags, with ? pattern : nullptr, p, table, flow_cap, out, fo);
    return BT_OK;
}
