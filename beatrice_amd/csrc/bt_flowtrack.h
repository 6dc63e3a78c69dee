// bt_flowtrack.h — the flow tracker (bt_flowtrack.hip), shared with the host runtime
// (bt_flow_track_* in bt_flowtrack_host.cpp): the layout of the state and of the caller's scratch,
// the argument checks, the slot hash, and the tracker on the host (init, update, expire over a
// state in host memory). The host part is plain C++ with no device and no runtime state:
// tools/flowtrack_host_check.cpp runs it under the host sanitizers.
#pragma once

#include <stdint.h>
#include <cstddef>
#include <cstring>
#include <vector>

#include "beatrice_gpu.h"
#include "bt_flowtab.h"
#include "bt_flowtcp.h"

#ifdef __HIPCC__
#define BT_FK_HD __host__ __device__
#else
#define BT_FK_HD
#endif

namespace bt {

// Update: one thread per flow of the batch, blocks of 4 waves. Expire: one thread per flow of the state.
constexpr uint32_t kFkThreads = 256;
constexpr uint32_t kFkWaves = kFkThreads / 64u;
constexpr uint32_t kFkJoinThreads = 1024;
constexpr uint32_t kFkEmpty = 0xFFFFFFFFu;        // a slot word that holds no flow
constexpr uint32_t kFkNew = kFtPending;           // map[j] between find and apply: the batch's flow j is not in the table
constexpr uint32_t kFkMaxFlows = BT_FLOW_ID_EXPIRED;   // flow numbers stay below every sentinel
constexpr uint32_t kFkMaxBatch = 1u << 30;        // the per-batch table's limit at auto slots
static_assert(BT_FLOW_ID_EXPIRED < kFtPending, "BT_FLOW_ID_EXPIRED below the other sentinels");
static_assert(sizeof(bt_flow_track_rec) == 104 && alignof(bt_flow_track_rec) == 8, "bt_flow_track_rec layout");
static_assert(sizeof(bt_flow_track_hdr) == 128 && sizeof(bt_flow_track_result) == 64 &&
              sizeof(bt_flow_track_expire_result) == 32 && sizeof(bt_flow_track_opts) == 16, "flow tracker ABI layout");
// a bt_flow_rec and a bt_flow_track_rec begin alike: the 36 key bytes, the class, three zero bytes
static_assert(offsetof(bt_flow_rec, klass) == 36 && offsetof(bt_flow_track_rec, klass) == 36 &&
              offsetof(bt_flow_rec, first) == 40 && offsetof(bt_flow_track_rec, first_batch) == 40, "the records' common head");

struct FkPart {                   // update scratch, one per block of batch flows (bt_flowtrack_find)
    uint32_t nnew, rel;           // new flows of the block; of the blocks before it (bt_flowtrack_join)
    uint32_t wnew[kFkWaves];      // new flows of wave w
    uint64_t new_packets, new_bytes;   // the new flows' packets and bytes: what overflows when none of them fits
};
static_assert(sizeof(FkPart) == 40, "FkPart layout");
struct FkCtl { uint32_t ok, base, seq, room; };   // bt_flowtrack_join for the kernels behind it: n_flows before the call, ...

struct FxPart { uint32_t nidle, rel; uint32_t widle[kFkWaves]; };   // expire scratch, one per block of flows
struct FxCtl { uint32_t ok, n_before, n_live, limit; };             // limit: the first `limit` idle flows leave

struct FkShadow { uint32_t flags, flow_cap, slots; };   // what the host knows of a device state (bt_flowtrack_host.cpp)

// The slot hash of a flow: the first ten little-endian words of its record (36 key bytes, class, zeros).
BT_FK_HD inline uint32_t fk_hash(const uint32_t (&w)[10]) {
    uint32_t h = 0x165667B1u;
    for (int d = 0; d < 10; ++d) {
        h += w[d] * 0xC2B2AE3Du;
        h = ((h << 17) | (h >> 15)) * 0x27D4EB2Fu;
    }
    h ^= h >> 15; h *= 0x85EBCA77u;
    h ^= h >> 13; h *= 0xC2B2AE3Du;
    return h ^ (h >> 16);
}

// bt_flow_track_layout's work: false with the reason in why[0 .. cap).
inline bool fk_layout(uint32_t flow_cap, uint32_t slots, bt_flow_track_sizes* l, char* why, size_t cap) {
    const auto no = [&](const char* s) { snprintf(why, cap, "%s", s); return false; };
    if (!flow_cap) return no("flow_cap == 0");
    if (flow_cap > kFkMaxFlows) return no("flow_cap above 0xFFFFFFFB: flow numbers would meet the flow id sentinels");
    uint32_t s = slots;
    if (!s && !(s = ft_auto_slots(flow_cap))) return no("slots == 0 (auto) needs flow_cap <= 2^30");
    if (s & (s - 1u)) return no("slots is not a power of two");
    if (s < kFtMinSlots) return no("slots below 128");
    if (s < flow_cap) return no("slots below flow_cap");
    *l = bt_flow_track_sizes{};
    l->header = 0;
    l->records = ft_round(sizeof(bt_flow_track_hdr));
    l->slot_words = l->records + ft_round((uint64_t)flow_cap * sizeof(bt_flow_track_rec));
    l->total = l->slot_words + ft_round((uint64_t)s * 4u);
    l->slots = s;
    return true;
}

struct FkLayout { uint64_t ft, flows, ftres, map, parts, ctl, total; };   // byte offsets into an update's scratch

inline FkLayout fk_scratch(uint32_t n) {   // n <= kFkMaxBatch
    FkLayout l{};
    l.ft = 0;
    l.flows = l.ft + ft_layout(n, ft_auto_slots(n)).total;
    l.ftres = l.flows + ft_round((uint64_t)n * sizeof(bt_flow_rec));
    l.map = l.ftres + ft_round(sizeof(bt_flow_table_result));
    l.parts = l.map + ft_round((uint64_t)n * 4u);
    l.ctl = l.parts + ft_round(((uint64_t)n + kFkThreads - 1u) / kFkThreads * sizeof(FkPart));
    l.total = l.ctl + ft_round(sizeof(FkCtl));
    return l;
}

struct FxLayout { uint64_t ctl, parts, tmp, total; };   // ... an expire's scratch

inline FxLayout fx_scratch(uint32_t flow_cap) {
    FxLayout l{};
    l.ctl = 0;
    l.parts = l.ctl + ft_round(sizeof(FxCtl));
    l.tmp = l.parts + ft_round(((uint64_t)flow_cap + kFkThreads - 1u) / kFkThreads * sizeof(FxPart));
    l.total = l.tmp + ft_round((uint64_t)flow_cap * sizeof(bt_flow_track_rec));
    return l;
}

struct FlowtrackArgs {            // the update kernels'
    bt_flow_track_hdr* hdr;
    bt_flow_track_rec* recs;
    uint32_t* slot;
    uint32_t flags, flow_cap, slots;   // as the state was initialised: compared with *hdr on the device
    uint32_t n, empty;            // empty: n == 0, the per-batch kernels did not run
    const bt_flow_rec* flows;     // the per-batch table's outputs, in the scratch
    const bt_flow_table_result* ftres;
    uint32_t* map;                // batch flow -> flow number, kFkNew or BT_FLOW_ID_OVERFLOW
    FkPart* parts;
    FkCtl* ctl;
    const uint64_t* ts;
    uint64_t batch_ts;
    uint32_t* flow_id;
    bt_flow_track_result* result;
};

struct FlowexpArgs {              // the expire kernels'
    bt_flow_track_hdr* hdr;
    bt_flow_track_rec* recs;
    uint32_t* slot;
    uint32_t flags, flow_cap, slots;
    uint32_t expired_cap, all;    // all: expired == NULL, every idle flow leaves
    uint64_t now, idle;
    bt_flow_track_rec* tmp;       // scratch, flow_cap records
    FxPart* parts;
    FxCtl* ctl;
    bt_flow_track_rec* expired;
    uint32_t* remap;
    bt_flow_track_expire_result* result;
};

BT_FK_HD inline bool fk_is_idle(uint64_t last_ts, uint64_t now, uint64_t idle) { return last_ts <= now && now - last_ts > idle; }

// The TCP-aware expire (bt_flow_track_expire_tcp_*): the plain expire's arguments and the side table.
struct FlowexpTcpArgs : FlowexpArgs {
    bt_flow_tcp_rec* tcp;          // the state's side table, flow_cap records
    bt_flow_tcp_rec* tmp_tcp;      // scratch, flow_cap records
    bt_flow_tcp_rec* expired_tcp;  // optional, beside expired[]
    uint64_t closed_idle;
};

// Does a flow leave under the TCP-aware expire? Idle, or closed / reset and idle by closed_idle.
BT_FK_HD inline bool fk_tcp_leaves(uint64_t last_ts, const bt_flow_tcp_rec& t, uint32_t flags, uint64_t now, uint64_t idle,
                                   uint64_t closed_idle) {
    if (fk_is_idle(last_ts, now, idle)) return true;
    const int s = flowtcp_state(t.flags[0], t.flags[1], flags);
    return (s == BT_TCP_CLOSED || s == BT_TCP_RESET) && fk_is_idle(last_ts, now, closed_idle);
}

struct FxTcpLayout { uint64_t tmp_tcp, total; };   // the plain expire's scratch, then flow_cap side records

inline FxTcpLayout fx_tcp_scratch(uint32_t flow_cap) {
    FxTcpLayout l{};
    l.tmp_tcp = fx_scratch(flow_cap).total;
    l.total = l.tmp_tcp + ft_round((uint64_t)flow_cap * sizeof(bt_flow_tcp_rec));
    return l;
}

// The checks of bt_flow_track_init_device / _init_host on everything but the context.
inline bool flowtrack_init_args(const void* state, uint64_t state_bytes, const bt_flow_track_opts* opts, bt_flow_track_sizes* l,
                                char* why, size_t cap) {
    const auto no = [&](const char* s) { snprintf(why, cap, "%s", s); return false; };
    if (!state) return no("null state");
    if (reinterpret_cast<uintptr_t>(state) & 255u) return no("state is not 256-byte aligned");
    if (!opts) return no("null opts");
    if (opts->flags & ~(BT_FLOWTAB_L3_ONLY | BT_FLOWTAB_BIDIRECTIONAL)) return no("unknown flag bits");
    if (!fk_layout(opts->flow_cap, opts->slots, l, why, cap)) return false;
    if (state_bytes < l->total) {
        snprintf(why, cap, "state_bytes %llu below the layout's %llu", (unsigned long long)state_bytes, (unsigned long long)l->total);
        return false;
    }
    return true;
}

// The checks of bt_flow_track_update_device on everything but the context, the per-batch table's
// launch arguments (*fa) and the merge kernels' (*ka). `sh`: the state's entry, nullptr = unknown.
inline bool flowtrack_update_args(const FkShadow* sh, void* state, const bt_batch* frames, const uint64_t* select,
                                  const bt_flow_track_update* upd, void* scratch, uint64_t scratch_bytes,
                                  const bt_flow_track_out* out, FlowtabArgs* fa, FlowtrackArgs* ka, char* why, size_t cap) {
    const auto no = [&](const char* s) { snprintf(why, cap, "%s", s); return false; };
    if (!state) return no("null state");
    if (reinterpret_cast<uintptr_t>(state) & 255u) return no("state is not 256-byte aligned");
    if (!frames) return no("null frames");
    if (!upd) return no("null upd");
    if (!out) return no("null out");
    if (!out->result) return no("null result");
    if (reinterpret_cast<uintptr_t>(out->result) & 7u) return no("result is not 8-byte aligned");
    if (reinterpret_cast<uintptr_t>(out->flow_id) & 3u) return no("flow_id is not 4-byte aligned");
    if (reinterpret_cast<uintptr_t>(upd->ts) & 7u) return no("ts is not 8-byte aligned");
    if (reinterpret_cast<uintptr_t>(scratch) & 255u) return no("scratch is not 256-byte aligned");
    if (frames->flags & (BT_BATCH_PREFIXES | BT_BATCH_LEAN))
        return no("a BT_BATCH_PREFIXES / BT_BATCH_LEAN batch holds no whole frames to key");
    const uint32_t n = frames->n;
    if (n > kFkMaxBatch) return no("n above 2^30: the per-batch flow table's limit at auto slots");
    const FkLayout l = fk_scratch(n);
    if (n && !scratch) return no("null scratch");
    if (n && scratch_bytes < l.total) {
        snprintf(why, cap, "scratch_bytes %llu below the need %llu", (unsigned long long)scratch_bytes, (unsigned long long)l.total);
        return false;
    }
    uint8_t* const s = static_cast<uint8_t*>(scratch);
    const auto at = [&](uint64_t off) -> uint8_t* { return n ? s + off : nullptr; };   // an empty batch uses no scratch
    const bt_flow_table_opts o{sh ? sh->flags : 0u, 0u, n, 0u};
    // (flowtab_args wants a result pointer; with n == 0 nothing is launched and none is written)
    const bt_flow_table_out fo{out->flow_id, reinterpret_cast<bt_flow_rec*>(at(l.flows)),
                               n ? reinterpret_cast<bt_flow_table_result*>(at(l.ftres)) : reinterpret_cast<bt_flow_table_result*>(out->result)};
    if (!flowtab_args(frames, select, &o, at(l.ft), l.flows - l.ft, &fo, fa, why, cap)) return false;
    // last of the checks, so that every other refusal is the same for any state
    if (!sh) return no("state is not an initialised tracker (bt_flow_track_init_device)");
    bt_flow_track_sizes sl{};
    if (!fk_layout(sh->flow_cap, sh->slots, &sl, why, cap)) return false;
    uint8_t* const st = static_cast<uint8_t*>(state);
    *ka = FlowtrackArgs{};
    ka->hdr = reinterpret_cast<bt_flow_track_hdr*>(st + sl.header);
    ka->recs = reinterpret_cast<bt_flow_track_rec*>(st + sl.records);
    ka->slot = reinterpret_cast<uint32_t*>(st + sl.slot_words);
    ka->flags = sh->flags; ka->flow_cap = sh->flow_cap; ka->slots = sl.slots;
    ka->n = n; ka->empty = n ? 0u : 1u;
    ka->flows = fo.flows;
    ka->ftres = n ? fo.result : nullptr;
    ka->map = reinterpret_cast<uint32_t*>(at(l.map));
    ka->parts = reinterpret_cast<FkPart*>(at(l.parts));
    ka->ctl = reinterpret_cast<FkCtl*>(at(l.ctl));
    ka->ts = upd->ts; ka->batch_ts = upd->batch_ts;
    ka->flow_id = out->flow_id;
    ka->result = out->result;
    return true;
}

// The checks of bt_flow_track_expire_device on everything but the context.
inline bool flowtrack_expire_args(const FkShadow* sh, void* state, uint64_t now, uint64_t idle, void* scratch, uint64_t scratch_bytes,
                                  const bt_flow_track_expire_out* out, FlowexpArgs* xa, char* why, size_t cap) {
    const auto no = [&](const char* s) { snprintf(why, cap, "%s", s); return false; };
    if (!state) return no("null state");
    if (reinterpret_cast<uintptr_t>(state) & 255u) return no("state is not 256-byte aligned");
    if (!out) return no("null out");
    if (!out->result) return no("null result");
    if (reinterpret_cast<uintptr_t>(out->result) & 7u) return no("result is not 8-byte aligned");
    if (reinterpret_cast<uintptr_t>(out->expired) & 7u) return no("expired is not 8-byte aligned");
    if (reinterpret_cast<uintptr_t>(out->remap) & 3u) return no("remap is not 4-byte aligned");
    if (!out->expired && out->expired_cap) return no("null expired with expired_cap != 0");
    if (!scratch) return no("null scratch");
    if (reinterpret_cast<uintptr_t>(scratch) & 255u) return no("scratch is not 256-byte aligned");
    if (!sh) return no("state is not an initialised tracker (bt_flow_track_init_device)");
    bt_flow_track_sizes sl{};
    if (!fk_layout(sh->flow_cap, sh->slots, &sl, why, cap)) return false;
    const FxLayout l = fx_scratch(sh->flow_cap);
    if (scratch_bytes < l.total) {
        snprintf(why, cap, "scratch_bytes %llu below the need %llu", (unsigned long long)scratch_bytes, (unsigned long long)l.total);
        return false;
    }
    uint8_t* const st = static_cast<uint8_t*>(state);
    uint8_t* const s = static_cast<uint8_t*>(scratch);
    *xa = FlowexpArgs{};
    xa->hdr = reinterpret_cast<bt_flow_track_hdr*>(st + sl.header);
    xa->recs = reinterpret_cast<bt_flow_track_rec*>(st + sl.records);
    xa->slot = reinterpret_cast<uint32_t*>(st + sl.slot_words);
    xa->flags = sh->flags; xa->flow_cap = sh->flow_cap; xa->slots = sl.slots;
    xa->expired_cap = out->expired_cap; xa->all = out->expired ? 0u : 1u;
    xa->now = now; xa->idle = idle;
    xa->tmp = reinterpret_cast<bt_flow_track_rec*>(s + l.tmp);
    xa->parts = reinterpret_cast<FxPart*>(s + l.parts);
    xa->ctl = reinterpret_cast<FxCtl*>(s + l.ctl);
    xa->expired = out->expired; xa->remap = out->remap; xa->result = out->result;
    return true;
}

// The checks on a bt_flow_track_expire_tcp, for the device and the host form.
inline bool flowtrack_expire_tcp_x(const bt_flow_track_expire_tcp* x, const bt_flow_track_expire_out* out, char* why, size_t cap) {
    const auto no = [&](const char* s) { snprintf(why, cap, "%s", s); return false; };
    if (!x) return no("null x");
    if (!x->tcp) return no("null tcp");
    if (reinterpret_cast<uintptr_t>(x->tcp) & 3u) return no("tcp is not 4-byte aligned");
    if (reinterpret_cast<uintptr_t>(x->expired_tcp) & 3u) return no("expired_tcp is not 4-byte aligned");
    if (out && x->expired_tcp && !out->expired) return no("expired_tcp without expired");
    return true;
}

// The checks of bt_flow_track_expire_tcp_device on everything but the context.
inline bool flowtrack_expire_tcp_args(const FkShadow* sh, void* state, uint64_t now, uint64_t idle, const bt_flow_track_expire_tcp* x,
                                      void* scratch, uint64_t scratch_bytes, const bt_flow_track_expire_out* out, FlowexpTcpArgs* xa,
                                      char* why, size_t cap) {
    if (!flowtrack_expire_tcp_x(x, out, why, cap)) return false;
    FlowexpArgs plain;
    if (!flowtrack_expire_args(sh, state, now, idle, scratch, scratch_bytes, out, &plain, why, cap)) return false;
    const FxTcpLayout l = fx_tcp_scratch(sh->flow_cap);
    if (scratch_bytes < l.total) {
        snprintf(why, cap, "scratch_bytes %llu below the need %llu", (unsigned long long)scratch_bytes, (unsigned long long)l.total);
        return false;
    }
    *xa = FlowexpTcpArgs{};
    static_cast<FlowexpArgs&>(*xa) = plain;
    xa->tcp = x->tcp;
    xa->tmp_tcp = reinterpret_cast<bt_flow_tcp_rec*>(static_cast<uint8_t*>(scratch) + l.tmp_tcp);
    xa->expired_tcp = x->expired_tcp;
    xa->closed_idle = x->closed_idle;
    return true;
}

// ---- the tracker on the host: the same state layout in host memory --------------------------

struct FkHostState { bt_flow_track_hdr* hdr; bt_flow_track_rec* recs; uint32_t* slot; };

// A state the host forms accept: an initialised header whose layout fits state_bytes.
inline bool fk_host_state(void* state, uint64_t state_bytes, FkHostState* hs, char* why, size_t cap) {
    const auto no = [&](const char* s) { snprintf(why, cap, "%s", s); return false; };
    if (!state) return no("null state");
    if (reinterpret_cast<uintptr_t>(state) & 255u) return no("state is not 256-byte aligned");
    if (state_bytes < sizeof(bt_flow_track_hdr)) return no("state is not an initialised tracker: state_bytes below the header");
    bt_flow_track_hdr* const h = static_cast<bt_flow_track_hdr*>(state);
    bt_flow_track_sizes l{};
    char inner[96];
    if (h->magic != BT_FLOW_TRACK_MAGIC || (h->flags & ~(BT_FLOWTAB_L3_ONLY | BT_FLOWTAB_BIDIRECTIONAL)) ||
        !fk_layout(h->flow_cap, h->slots, &l, inner, sizeof(inner)) || !h->slots || h->n_flows > h->flow_cap)
        return no("state is not an initialised tracker: the header does not hold one");
    if (state_bytes < l.total) return no("state is not an initialised tracker: state_bytes below the header's layout");
    uint8_t* const st = static_cast<uint8_t*>(state);
    *hs = {h, reinterpret_cast<bt_flow_track_rec*>(st + l.records), reinterpret_cast<uint32_t*>(st + l.slot_words)};
    return true;
}

inline void fk_init_host(void* state, const bt_flow_track_opts& o, const bt_flow_track_sizes& l) {
    uint8_t* const st = static_cast<uint8_t*>(state);
    bt_flow_track_hdr h{};
    h.magic = BT_FLOW_TRACK_MAGIC; h.flags = o.flags; h.flow_cap = o.flow_cap; h.slots = l.slots;
    memcpy(st + l.header, &h, sizeof(h));
    memset(st + l.records, 0, (size_t)o.flow_cap * sizeof(bt_flow_track_rec));
    memset(st + l.slot_words, 0xFF, (size_t)l.slots * 4u);
}

inline uint32_t fk_host_hash(const void* rec_head) {   // of the first 40 bytes of either record type
    uint32_t w[10];
    memcpy(w, rec_head, sizeof(w));
    return fk_hash(w);
}

// The first empty slot on the probe sequence of flow f's key takes f. n_flows <= flow_cap <= slots: there is one.
inline void fk_host_claim(const FkHostState& s, uint32_t f) {
    const uint32_t mask = s.hdr->slots - 1u;
    uint32_t at = fk_host_hash(&s.recs[f]) & mask;
    for (uint32_t probe = 0; probe < s.hdr->slots; ++probe, at = (at + 1u) & mask)
        if (s.slot[at] == kFkEmpty) { s.slot[at] = f; return; }
}

// One batch's flows (a per-batch table's records and result, n packets) merged into a checked
// state, in batch order; map[j] (n_flows entries, optional) = flow j's number or BT_FLOW_ID_OVERFLOW.
inline void fk_merge_host(const FkHostState& s, const bt_flow_rec* flows, const bt_flow_table_result& fr, uint32_t n,
                          const uint64_t* ts, uint64_t batch_ts, uint32_t* map, bt_flow_track_result* result) {
    bt_flow_track_hdr& h = *s.hdr;
    bt_flow_track_result r{};
    r.n = n; r.n_selected = fr.n_selected; r.none_packets = fr.none_packets; r.batch_flows = fr.n_flows;
    r.seq = h.seq; r.keyed_bytes = fr.keyed_bytes; r.none_bytes = fr.none_bytes;
    const uint32_t mask = h.slots - 1u;
    const auto stamp = [&](uint32_t i) { return ts ? ts[i] : batch_ts; };
    uint32_t unused = 0;
    for (uint32_t j = 0; j < fr.n_flows; ++j) {
        uint32_t& to = map ? map[j] : unused;
        const bt_flow_rec& f = flows[j];
        uint32_t at = fk_host_hash(&f) & mask, found = kFkNew;
        for (uint32_t probe = 0; probe < h.slots; ++probe, at = (at + 1u) & mask) {
            const uint32_t id = s.slot[at];
            if (id == kFkEmpty) break;
            if (id < h.flow_cap && memcmp(&s.recs[id], &f, 40) == 0) { found = id; break; }
        }
        if (found != kFkNew) {
            bt_flow_track_rec& t = s.recs[found];
            t.packets[0] += f.packets[0]; t.packets[1] += f.packets[1];
            t.bytes[0] += f.bytes[0]; t.bytes[1] += f.bytes[1];
            t.last_batch = h.seq; t.last = f.last; t.last_ts = stamp(f.last);
            to = found;
        } else if (h.n_flows < h.flow_cap) {
            const uint32_t g = h.n_flows++;
            bt_flow_track_rec t{};
            memcpy(&t, &f, 40);
            t.first_batch = t.last_batch = h.seq;
            t.first = f.first; t.last = f.last;
            t.packets[0] = f.packets[0]; t.packets[1] = f.packets[1];
            t.bytes[0] = f.bytes[0]; t.bytes[1] = f.bytes[1];
            t.first_ts = stamp(f.first); t.last_ts = stamp(f.last);
            s.recs[g] = t;
            fk_host_claim(s, g);
            to = g;
            ++r.new_flows;
        } else {
            to = BT_FLOW_ID_OVERFLOW;
            ++r.overflow_flows;
            r.overflow_packets += f.packets[0] + f.packets[1];
            r.overflow_bytes += f.bytes[0] + f.bytes[1];
        }
    }
    r.n_flows = h.n_flows;
    ++h.seq;
    h.selected_packets += r.n_selected; h.keyed_packets += r.n_selected - r.none_packets; h.none_packets += r.none_packets;
    h.overflow_packets += r.overflow_packets;
    h.selected_bytes += r.keyed_bytes + r.none_bytes; h.keyed_bytes += r.keyed_bytes; h.none_bytes += r.none_bytes;
    h.overflow_bytes += r.overflow_bytes;
    *result = r;
}

// bt_flow_track_update_host's work on a checked state: the per-batch group-by, then the merge.
inline void fk_update_host(const FkHostState& s, const uint8_t* base, uint64_t bytes, const bt_pkt_desc* desc, uint32_t n,
                           const uint64_t* select, const uint64_t* ts, uint64_t batch_ts, uint32_t* flow_id,
                           bt_flow_track_result* result) {
    std::vector<uint32_t> local(n);
    std::vector<bt_flow_rec> flows(n);
    bt_flow_table_result fr{};
    flowtab_host(base, bytes, desc, n, select, s.hdr->flags, ft_auto_slots(n), n, n ? local.data() : nullptr,
                 n ? flows.data() : nullptr, &fr);
    std::vector<uint32_t> map(fr.n_flows);
    fk_merge_host(s, flows.data(), fr, n, ts, batch_ts, map.data(), result);
    if (flow_id)
        for (uint32_t i = 0; i < n; ++i) flow_id[i] = local[i] < kFtPending ? map[local[i]] : local[i];
}

// bt_flow_track_expire_host's work on a checked state and checked outputs.
inline void fk_expire_host(const FkHostState& s, uint64_t now, uint64_t idle, const bt_flow_track_expire_out* out) {
    bt_flow_track_hdr& h = *s.hdr;
    bt_flow_track_expire_result r{};
    r.n_flows_before = h.n_flows;
    uint32_t live = 0;
    for (uint32_t f = 0; f < h.n_flows; ++f) {
        const bool is_idle = fk_is_idle(s.recs[f].last_ts, now, idle);
        r.n_idle += is_idle ? 1u : 0u;
        if (is_idle && (!out->expired || r.n_expired < out->expired_cap)) {
            if (out->expired) out->expired[r.n_expired] = s.recs[f];
            if (out->remap) out->remap[f] = BT_FLOW_ID_EXPIRED;
            ++r.n_expired;
            continue;
        }
        if (out->remap) out->remap[f] = live;
        if (live != f) s.recs[live] = s.recs[f];
        ++live;
    }
    if (r.n_expired) {
        memset(static_cast<void*>(s.recs + live), 0, (size_t)(h.n_flows - live) * sizeof(bt_flow_track_rec));
        memset(s.slot, 0xFF, (size_t)h.slots * 4u);
        h.n_flows = live;
        for (uint32_t f = 0; f < live; ++f) fk_host_claim(s, f);
    }
    r.n_flows = live;
    *out->result = r;
}

// bt_flow_track_expire_tcp_host's work on a checked state and checked outputs: fk_expire_host with
// one more way to leave, and the side table moved with the records.
inline void fk_expire_tcp_host(const FkHostState& s, uint64_t now, uint64_t idle, const bt_flow_track_expire_tcp* x,
                               const bt_flow_track_expire_out* out) {
    bt_flow_track_hdr& h = *s.hdr;
    bt_flow_track_expire_result r{};
    r.n_flows_before = h.n_flows;
    uint32_t live = 0;
    for (uint32_t f = 0; f < h.n_flows; ++f) {
        const bool leaves = fk_tcp_leaves(s.recs[f].last_ts, x->tcp[f], h.flags, now, idle, x->closed_idle);
        r.n_idle += leaves ? 1u : 0u;
        if (leaves && (!out->expired || r.n_expired < out->expired_cap)) {
            if (out->expired) out->expired[r.n_expired] = s.recs[f];
            if (x->expired_tcp) x->expired_tcp[r.n_expired] = x->tcp[f];
            if (out->remap) out->remap[f] = BT_FLOW_ID_EXPIRED;
            ++r.n_expired;
            continue;
        }
        if (out->remap) out->remap[f] = live;
        if (live != f) { s.recs[live] = s.recs[f]; x->tcp[live] = x->tcp[f]; }
        ++live;
    }
    if (r.n_expired) {
        memset(static_cast<void*>(s.recs + live), 0, (size_t)(h.n_flows - live) * sizeof(bt_flow_track_rec));
        memset(static_cast<void*>(x->tcp + live), 0, (size_t)(h.n_flows - live) * sizeof(bt_flow_tcp_rec));
        memset(s.slot, 0xFF, (size_t)h.slots * 4u);
        h.n_flows = live;
        for (uint32_t f = 0; f < live; ++f) fk_host_claim(s, f);
    }
    r.n_flows = live;
    *out->result = r;
}

// All launches, asynchronous on `stream`. launch_flowtrack runs behind launch_flowtab (the caller enqueues both).
int launch_flowtrack_init(const FlowexpArgs& a, void* stream);
int launch_flowtrack(const FlowtrackArgs& a, void* stream, void* timing_stop = nullptr);
int launch_flowexpire(const FlowexpArgs& a, void* stream);
int launch_flowexpire_tcp(const FlowexpTcpArgs& a, void* stream);

// The state `state` as bt_flow_track_init_device left it in this process (bt_flowtrack_host.cpp): false = unknown.
bool fk_known_state(const void* state, FkShadow* sh);

}  // namespace bt
