// bt_tally_host.cpp — bt_tally_device: the counts of a device-resident batch (bt_tally.hip)
// on a stream, right behind the parse+filter pass that wrote what it counts.
#include <cstddef>
#include <cstdlib>
#include <mutex>

#include "bt_ctx.h"
#include "bt_hip_util.h"

using namespace bt;

namespace bt {

// e0 / e1: timing events recorded by the first / second kernel's own dispatch (bt_time_tally).
int run_tally(bt_ctx* c, const uint8_t* decide, uint32_t n, const bt_batch* frames, const void* records, uint32_t n_cap,
              uint32_t flags, bt_tally* out, hipStream_t st, hipEvent_t e0, hipEvent_t e1) {
    TallyArgs a;
    char why[128];
    if (!tally_args(decide, n, frames, records, n_cap, flags, out, c->opts.flags, &a, why, sizeof(why)))
        return set_error(BT_E_INVALID_ARGUMENT, "bt_tally_device: %s", why);
    HIP_TRY(hipSetDevice(c->device));
    if (n == 0) {   // nothing to launch: *out is still written in stream order
        if (!(flags & BT_TALLY_ACCUMULATE)) {
            HIP_TRY(hipMemsetAsync(out, 0, sizeof(bt_tally), st));
        } else {    // the first_* fields describe this call alone
            constexpr size_t lo = offsetof(bt_tally, first_throw), hi = offsetof(bt_tally, code);
            HIP_TRY(hipMemsetAsync(reinterpret_cast<uint8_t*>(out) + lo, 0, hi - lo, st));
        }
        return BT_OK;
    }
    bt_ctx::Ws* w = nullptr;
    int rc = take_ws(c, n, &w);
    if (rc) return rc;
    if ((rc = ws_touch(c, w, st))) return rc;
    a.parts = w->tally_parts;
    // The histogram by ballot peeling: 0.113 against 0.124 ms with LDS adds on C3's 16.8 M decisions
    // (profiles/tally). A/B knob (tools/tally_rate.py): BT_TALLY_PEEL=0 selects the LDS adds.
    static const bool peel = [] {
        const char* e = getenv("BT_TALLY_PEEL");
        return !e || atoi(e) != 0;
    }();
    a.peel = peel ? 1u : 0u;
    rc = launch_tally(a, st, e0, e1);
    if (rc) return set_error(rc, "tally kernel launch failed: %s", hipGetErrorString(hipGetLastError()));
    return ws_done(c, w, st);
}

}  // namespace bt

extern "C" int bt_tally_device(bt_ctx* c, const uint8_t* decide, uint32_t n, const bt_batch* frames, const void* records,
                               uint32_t n_cap, uint32_t flags, bt_tally* out, void* stream) {
    if (!c) return set_error(BT_E_INVALID_ARGUMENT, "null context");   // before any HIP call: refused without a GPU
    const bt::DeviceRestore keep_device;   // the caller's current device, restored on return
    std::lock_guard<std::mutex> lk(c->mu);
    hipStream_t st = stream ? reinterpret_cast<hipStream_t>(stream) : c->stream;
    return run_tally(c, decide, n, frames, records, n_cap, flags, out, st, nullptr, nullptr);
}
