// bt_flowtrack_host.cpp — bt_flow_track_*: the flow tracker's entry points. The device forms
// enqueue bt_flowtab.hip's and bt_flowtrack.hip's kernels on a stream over a state in the caller's
// device memory; the host forms run bt_flowtrack.h's tracker over a state in host memory; the
// layout and scratch sizes. The device calls never read the device, so what they must know of a
// state on the host (flags, flow_cap, slots) is remembered here when it is initialised.
#include <mutex>

#include "bt_ctx.h"
#include "bt_flowtrack.h"
#include "bt_hip_util.h"

using namespace bt;

namespace {

// The states bt_flow_track_init_device has initialised in this process, by address. A fixed table:
// no allocation; initialising an address again replaces its entry, bt_flow_track_forget frees one,
// and a full table refuses the next address (no live tracker is ever dropped behind its caller's back).
constexpr uint32_t kStates = 256;
struct Known { const void* state; FkShadow sh; };
Known g_known[kStates];
uint32_t g_n_known = 0;
std::mutex g_known_mu;

bool known_state(const void* state, FkShadow* sh) {
    std::lock_guard<std::mutex> lk(g_known_mu);
    for (uint32_t k = 0; k < g_n_known; ++k)
        if (g_known[k].state == state) { *sh = g_known[k].sh; return true; }
    return false;
}

bool room_for_state(const void* state) {   // the address is known already, or an entry is free
    std::lock_guard<std::mutex> lk(g_known_mu);
    for (uint32_t k = 0; k < g_n_known; ++k)
        if (g_known[k].state == state) return true;
    return g_n_known < kStates;
}

bool remember_state(const void* state, const FkShadow& sh) {
    std::lock_guard<std::mutex> lk(g_known_mu);
    for (uint32_t k = 0; k < g_n_known; ++k)
        if (g_known[k].state == state) { g_known[k].sh = sh; return true; }
    if (g_n_known == kStates) return false;
    g_known[g_n_known++] = Known{state, sh};
    return true;
}

bool forget_state(const void* state) {
    std::lock_guard<std::mutex> lk(g_known_mu);
    for (uint32_t k = 0; k < g_n_known; ++k)
        if (g_known[k].state == state) { g_known[k] = g_known[--g_n_known]; return true; }
    return false;
}

}  // namespace

namespace bt {

bool fk_known_state(const void* state, FkShadow* sh) { return known_state(state, sh); }   // for bt_flowtop_host.cpp, bt_flowhosts_host.cpp

// e0 / e1: timing events recorded by the first / last kernel's own dispatch (bt_time_flow_track).
int run_flow_track_update(bt_ctx* c, void* state, const bt_batch* frames, const uint64_t* select, const bt_flow_track_update* upd,
                          void* scratch, uint64_t scratch_bytes, const bt_flow_track_out* out, hipStream_t st, hipEvent_t e0,
                          hipEvent_t e1) {
    FlowtabArgs fa;
    FlowtrackArgs ka;
    FkShadow sh{};
    char why[160];
    // before the context and any HIP call: every refusal is the same with and without a GPU
    const bool known = state && known_state(state, &sh);
    if (!flowtrack_update_args(known ? &sh : nullptr, state, frames, select, upd, scratch, scratch_bytes, out, &fa, &ka, why, sizeof(why)))
        return set_error(BT_E_INVALID_ARGUMENT, "bt_flow_track_update_device: %s", why);
    if (!c) return set_error(BT_E_INVALID_ARGUMENT, "bt_flow_track_update_device: null context");
    HIP_TRY(hipSetDevice(c->device));
    if (!st) st = c->stream;
    int rc = launch_flowtab(fa, st, e0, nullptr);   // nothing for n == 0
    if (!rc) rc = launch_flowtrack(ka, st, e1);
    if (rc) return set_error(rc, "flow tracker kernel launch failed: %s", hipGetErrorString(hipGetLastError()));
    return BT_OK;
}

}  // namespace bt

extern "C" int bt_flow_track_layout(uint32_t flow_cap, uint32_t slots, bt_flow_track_sizes* layout) {
    if (!layout) return set_error(BT_E_INVALID_ARGUMENT, "bt_flow_track_layout: null layout");
    char why[128];
    bt_flow_track_sizes l{};
    if (!fk_layout(flow_cap, slots, &l, why, sizeof(why))) return set_error(BT_E_INVALID_ARGUMENT, "bt_flow_track_layout: %s", why);
    *layout = l;
    return BT_OK;
}

extern "C" int bt_flow_track_scratch_bytes(uint32_t n, uint64_t* bytes) {
    if (!bytes) return set_error(BT_E_INVALID_ARGUMENT, "bt_flow_track_scratch_bytes: null bytes");
    if (n > kFkMaxBatch) return set_error(BT_E_INVALID_ARGUMENT, "bt_flow_track_scratch_bytes: n above 2^30");
    *bytes = fk_scratch(n).total;
    return BT_OK;
}

extern "C" int bt_flow_track_expire_scratch_bytes(uint32_t flow_cap, uint64_t* bytes) {
    if (!bytes) return set_error(BT_E_INVALID_ARGUMENT, "bt_flow_track_expire_scratch_bytes: null bytes");
    char why[128];
    bt_flow_track_sizes l{};
    if (!fk_layout(flow_cap, flow_cap > (1u << 30) ? 1u << 31 : 0u, &l, why, sizeof(why)))
        return set_error(BT_E_INVALID_ARGUMENT, "bt_flow_track_expire_scratch_bytes: %s", why);
    *bytes = fx_scratch(flow_cap).total;
    return BT_OK;
}

extern "C" int bt_flow_track_init_device(bt_ctx* c, void* state, uint64_t state_bytes, const bt_flow_track_opts* opts, void* stream) {
    char why[160];
    bt_flow_track_sizes l{};
    if (!flowtrack_init_args(state, state_bytes, opts, &l, why, sizeof(why)))
        return set_error(BT_E_INVALID_ARGUMENT, "bt_flow_track_init_device: %s", why);
    if (!c) return set_error(BT_E_INVALID_ARGUMENT, "bt_flow_track_init_device: null context");
    const FkShadow sh{opts->flags, opts->flow_cap, l.slots};
    const char* const full = "bt_flow_track_init_device: 256 tracker states are known to this process (bt_flow_track_forget frees one)";
    if (!room_for_state(state)) return set_error(BT_E_RESOURCE, "%s", full);
    const bt::DeviceRestore keep_device;   // the caller's current device, restored on return
    std::lock_guard<std::mutex> lk(c->mu);
    HIP_TRY(hipSetDevice(c->device));
    uint8_t* const s = static_cast<uint8_t*>(state);
    FlowexpArgs a{};
    a.hdr = reinterpret_cast<bt_flow_track_hdr*>(s + l.header);
    a.recs = reinterpret_cast<bt_flow_track_rec*>(s + l.records);
    a.slot = reinterpret_cast<uint32_t*>(s + l.slot_words);
    a.flags = sh.flags; a.flow_cap = sh.flow_cap; a.slots = sh.slots;
    const int rc = launch_flowtrack_init(a, stream ? stream : c->stream);
    if (rc) return set_error(rc, "flow tracker kernel launch failed: %s", hipGetErrorString(hipGetLastError()));
    if (!remember_state(state, sh)) return set_error(BT_E_RESOURCE, "%s", full);   // known only once the launch is enqueued
    return BT_OK;
}

extern "C" int bt_flow_track_forget(void* state) {
    if (!state) return set_error(BT_E_INVALID_ARGUMENT, "bt_flow_track_forget: null state");
    if (!forget_state(state)) return set_error(BT_E_INVALID_ARGUMENT, "bt_flow_track_forget: state is not an initialised tracker (bt_flow_track_init_device)");
    return BT_OK;
}

extern "C" int bt_flow_track_update_device(bt_ctx* c, void* state, const bt_batch* frames, const uint64_t* select,
                                           const bt_flow_track_update* upd, void* scratch, uint64_t scratch_bytes,
                                           const bt_flow_track_out* out, void* stream) {
    if (!c) return run_flow_track_update(nullptr, state, frames, select, upd, scratch, scratch_bytes, out, nullptr, nullptr, nullptr);
    const bt::DeviceRestore keep_device;   // the caller's current device, restored on return
    std::lock_guard<std::mutex> lk(c->mu);
    return run_flow_track_update(c, state, frames, select, upd, scratch, scratch_bytes, out, reinterpret_cast<hipStream_t>(stream),
                                 nullptr, nullptr);
}

extern "C" int bt_flow_track_expire_device(bt_ctx* c, void* state, uint64_t now, uint64_t idle, void* scratch, uint64_t scratch_bytes,
                                           const bt_flow_track_expire_out* out, void* stream) {
    FlowexpArgs xa;
    FkShadow sh{};
    char why[160];
    const bool known = state && known_state(state, &sh);
    if (!flowtrack_expire_args(known ? &sh : nullptr, state, now, idle, scratch, scratch_bytes, out, &xa, why, sizeof(why)))
        return set_error(BT_E_INVALID_ARGUMENT, "bt_flow_track_expire_device: %s", why);
    if (!c) return set_error(BT_E_INVALID_ARGUMENT, "bt_flow_track_expire_device: null context");
    const bt::DeviceRestore keep_device;   // the caller's current device, restored on return
    std::lock_guard<std::mutex> lk(c->mu);
    HIP_TRY(hipSetDevice(c->device));
    const int rc = launch_flowexpire(xa, stream ? stream : c->stream);
    if (rc) return set_error(rc, "flow tracker kernel launch failed: %s", hipGetErrorString(hipGetLastError()));
    return BT_OK;
}

extern "C" int bt_flow_track_expire_tcp_scratch_bytes(uint32_t flow_cap, uint64_t* bytes) {
    if (!bytes) return set_error(BT_E_INVALID_ARGUMENT, "bt_flow_track_expire_tcp_scratch_bytes: null bytes");
    char why[128];
    bt_flow_track_sizes l{};
    if (!fk_layout(flow_cap, flow_cap > (1u << 30) ? 1u << 31 : 0u, &l, why, sizeof(why)))
        return set_error(BT_E_INVALID_ARGUMENT, "bt_flow_track_expire_tcp_scratch_bytes: %s", why);
    *bytes = fx_tcp_scratch(flow_cap).total;
    return BT_OK;
}

extern "C" int bt_flow_track_expire_tcp_device(bt_ctx* c, void* state, uint64_t now, uint64_t idle, const bt_flow_track_expire_tcp* x,
                                               void* scratch, uint64_t scratch_bytes, const bt_flow_track_expire_out* out, void* stream) {
    FlowexpTcpArgs xa;
    FkShadow sh{};
    char why[160];
    const bool known = state && known_state(state, &sh);
    if (!flowtrack_expire_tcp_args(known ? &sh : nullptr, state, now, idle, x, scratch, scratch_bytes, out, &xa, why, sizeof(why)))
        return set_error(BT_E_INVALID_ARGUMENT, "bt_flow_track_expire_tcp_device: %s", why);
    if (!c) return set_error(BT_E_INVALID_ARGUMENT, "bt_flow_track_expire_tcp_device: null context");
    const bt::DeviceRestore keep_device;   // the caller's current device, restored on return
    std::lock_guard<std::mutex> lk(c->mu);
    HIP_TRY(hipSetDevice(c->device));
    const int rc = launch_flowexpire_tcp(xa, stream ? stream : c->stream);
    if (rc) return set_error(rc, "flow tracker kernel launch failed: %s", hipGetErrorString(hipGetLastError()));
    return BT_OK;
}

extern "C" int bt_flow_track_init_host(void* state, uint64_t state_bytes, const bt_flow_track_opts* opts) {
    char why[160];
    bt_flow_track_sizes l{};
    if (!flowtrack_init_args(state, state_bytes, opts, &l, why, sizeof(why)))
        return set_error(BT_E_INVALID_ARGUMENT, "bt_flow_track_init_host: %s", why);
    fk_init_host(state, *opts, l);
    return BT_OK;
}

extern "C" int bt_flow_track_update_host(void* state, uint64_t state_bytes, const uint8_t* base, uint64_t bytes, const bt_pkt_desc* desc,
                                         uint32_t n, const uint64_t* select, const bt_flow_track_update* upd, uint32_t* flow_id,
                                         bt_flow_track_result* result) {
    char why[160];
    FkHostState hs{};
    if (!fk_host_state(state, state_bytes, &hs, why, sizeof(why))) return set_error(BT_E_INVALID_ARGUMENT, "bt_flow_track_update_host: %s", why);
    if (!upd) return set_error(BT_E_INVALID_ARGUMENT, "bt_flow_track_update_host: null upd");
    if (!result) return set_error(BT_E_INVALID_ARGUMENT, "bt_flow_track_update_host: null result");
    if (n && (!base || !desc)) return set_error(BT_E_INVALID_ARGUMENT, "bt_flow_track_update_host: null base / desc");
    if (n > kFkMaxBatch) return set_error(BT_E_INVALID_ARGUMENT, "bt_flow_track_update_host: n above 2^30");
    fk_update_host(hs, base, bytes, desc, n, select, upd->ts, upd->batch_ts, flow_id, result);
    return BT_OK;
}

extern "C" int bt_flow_track_expire_host(void* state, uint64_t state_bytes, uint64_t now, uint64_t idle,
                                         const bt_flow_track_expire_out* out) {
    char why[160];
    FkHostState hs{};
    if (!fk_host_state(state, state_bytes, &hs, why, sizeof(why))) return set_error(BT_E_INVALID_ARGUMENT, "bt_flow_track_expire_host: %s", why);
    if (!out) return set_error(BT_E_INVALID_ARGUMENT, "bt_flow_track_expire_host: null out");
    if (!out->result) return set_error(BT_E_INVALID_ARGUMENT, "bt_flow_track_expire_host: null result");
    if (!out->expired && out->expired_cap) return set_error(BT_E_INVALID_ARGUMENT, "bt_flow_track_expire_host: null expired with expired_cap != 0");
    fk_expire_host(hs, now, idle, out);
    return BT_OK;
}

extern "C" int bt_flow_track_expire_tcp_host(void* state, uint64_t state_bytes, uint64_t now, uint64_t idle,
                                             const bt_flow_track_expire_tcp* x, const bt_flow_track_expire_out* out) {
    char why[160];
    FkHostState hs{};
    if (!flowtrack_expire_tcp_x(x, out, why, sizeof(why))) return set_error(BT_E_INVALID_ARGUMENT, "bt_flow_track_expire_tcp_host: %s", why);
    if (!fk_host_state(state, state_bytes, &hs, why, sizeof(why))) return set_error(BT_E_INVALID_ARGUMENT, "bt_flow_track_expire_tcp_host: %s", why);
    if (!out) return set_error(BT_E_INVALID_ARGUMENT, "bt_flow_track_expire_tcp_host: null out");
    if (!out->result) return set_error(BT_E_INVALID_ARGUMENT, "bt_flow_track_expire_tcp_host: null result");
    if (!out->expired && out->expired_cap) return set_error(BT_E_INVALID_ARGUMENT, "bt_flow_track_expire_tcp_host: null expired with expired_cap != 0");
    fk_expire_tcp_host(hs, now, idle, x, out);
    return BT_OK;
}
