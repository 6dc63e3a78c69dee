// bt_fanout_host.cpp — bt_flow_fanout_device: the selected packets of a device-resident batch
// fanned out to K queues by RSS flow hash (bt_fanout.hip) on a stream, right behind the
// parse+filter pass that wrote the selection; and bt_flow_hash_host, the same key and hash of
// one frame on the host.
#include <cstdlib>
#include <mutex>

#include "bt_ctx.h"
#include "bt_hip_util.h"

using namespace bt;

namespace bt {

// e0 / e1: timing events recorded by the first / last kernel's own dispatch (bt_time_fanout).
int run_fanout(bt_ctx* c, const bt_batch* frames, const uint64_t* select, const bt_fanout_opts* opts, const bt_fanout_out* out,
               hipStream_t st, hipEvent_t e0, hipEvent_t e1) {
    FanoutArgs a;
    char why[128];
    // before the context and any HIP call: every refusal is the same with and without a GPU
    if (!fanout_args(frames, select, opts, out, &a, why, sizeof(why)))
        return set_error(BT_E_INVALID_ARGUMENT, "bt_flow_fanout_device: %s", why);
    if (!c) return set_error(BT_E_INVALID_ARGUMENT, "bt_flow_fanout_device: null context");
    HIP_TRY(hipSetDevice(c->device));
    if (a.n == 0) {   // nothing to launch: *result is still written in stream order
        HIP_TRY(hipMemsetAsync(out->result, 0, sizeof(bt_fanout_result), st ? st : c->stream));
        return BT_OK;
    }
    if (!st) st = c->stream;
    bt_ctx::Ws* w = nullptr;
    int rc = take_ws(c, a.n, &w);
    if (rc) return rc;
    if ((rc = ws_touch(c, w, st))) return rc;
    a.parts = reinterpret_cast<FanoutPartial*>(w->fan_parts);
    a.rel = reinterpret_cast<uint32_t*>(w->fan_parts + (size_t)a.nchunks * sizeof(FanoutPartial));
    if (!a.queue) a.queue = w->fan_queue;
    // Toeplitz from nibble tables in LDS or bit-serial with the key in SGPRs (profiles/fanout).
    // A/B knob (tools/fanout_rate.py): BT_FANOUT_TABLE=0 selects the bit-serial form.
    static const bool table = [] {
        const char* e = getenv("BT_FANOUT_TABLE");
        return !e || atoi(e) != 0;
    }();
    a.table = table ? 1u : 0u;
    rc = launch_fanout(a, st, e0, e1);
    if (rc) return set_error(rc, "fan-out kernel launch failed: %s", hipGetErrorString(hipGetLastError()));
    return ws_done(c, w, st);
}

}  // namespace bt

extern "C" int bt_flow_fanout_device(bt_ctx* c, const bt_batch* frames, const uint64_t* select, const bt_fanout_opts* opts,
                                     const bt_fanout_out* out, void* stream) {
    if (!c) return run_fanout(nullptr, frames, select, opts, out, nullptr, nullptr, nullptr);   // refused without a GPU
    const bt::DeviceRestore keep_device;   // the caller's current device, restored on return
    std::lock_guard<std::mutex> lk(c->mu);
    return run_fanout(c, frames, select, opts, out, reinterpret_cast<hipStream_t>(stream), nullptr, nullptr);
}

extern "C" int bt_flow_hash_host(const uint8_t* frame, uint32_t len, const bt_fanout_opts* opts, uint32_t* hash,
                                 uint32_t* klass, uint32_t* queue) {
    uint8_t key[kFanKeyBytes], reta[kFanReta], in[kFanInputMax];
    char why[128];
    if (!fanout_opts(opts, key, reta, why, sizeof(why))) return set_error(BT_E_INVALID_ARGUMENT, "bt_flow_hash_host: %s", why);
    if (!frame && len) return set_error(BT_E_INVALID_ARGUMENT, "bt_flow_hash_host: null frame");
    uint32_t k = BT_FLOW_NONE;
    const uint32_t nb = flow_key_host(frame, len, (opts->flags & BT_FANOUT_L3_ONLY) != 0, in, &k);
    const uint32_t h = toeplitz_host(key, in, nb);
    if (hash) *hash = h;
    if (klass) *klass = k;
    if (queue) *queue = reta[h & 127u];
    return BT_OK;
}
