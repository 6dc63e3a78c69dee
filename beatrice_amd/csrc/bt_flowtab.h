// bt_flowtab.h — the per-batch flow table (bt_flowtab.hip), shared with the host runtime
// (bt_flow_table_device / bt_flow_table_host in bt_flowtab_host.cpp): the layout of the caller's
// scratch, the argument checks, the canonical direction of a key and the group-by on the host.
// The host part is plain C++ with no device and no runtime state: tools/flowtab_host_check.cpp
// runs it under the host sanitizers.
#pragma once

#include <stdint.h>
#include <cstring>
#include <unordered_map>
#include <vector>

#include "beatrice_gpu.h"
#include "bt_fanout.h"
#include "bt_frames.h"

namespace bt {

// One chunk = 256 tiles of 64 packets, one block of 8 waves per chunk, as the fan-out.
constexpr uint32_t kFtChunkTiles = 256;
constexpr uint32_t kFtWaves = 8;
constexpr uint32_t kFtJoinThreads = 1024;
constexpr uint32_t kFtMinSlots = 128;
constexpr uint32_t kFtEmpty = 0xFFFFFFFFu;      // a slot's owner word before a packet claims it
constexpr uint32_t kFtPending = 0xFFFFFFFCu;    // a packet's owner word between keys and insert (the other sentinels
                                                // are the BT_FLOW_ID_* values; a packet index is below it: n <= kFtPending)

// The table itself is one owner word per slot: kFtEmpty, or the packet whose CAS claimed the slot.
// That packet's FtFlow entry holds the slot's key and the flow's sums.
struct FtFlow {                   // scratch, one per packet; written for selected packets with a key only
    uint32_t w[9];                // the (canonical) key as big-endian words, zero past the class's length
    uint32_t meta;                // class | direction << 8
    uint32_t hash;                // the probe hash of (class, w); bt_flowtab_rank puts the flow's number here
    uint32_t len;                 // min(frame length, 65535)
    // the flow's sums, used when the packet owns a slot; bt_flowtab_keys puts the packet's own share here
    uint32_t first, last;         // atomicMin / atomicMax of the flow's packet indices
    uint32_t packets[2];          // one 64-bit atomicAdd over both
    uint64_t bytes[2];
};
static_assert(sizeof(FtFlow) == 80, "FtFlow layout");

struct FtPartial {                // scratch, one per chunk
    uint32_t n_selected, none_packets, none_bytes, keyed_bytes;   // bt_flowtab_keys (a chunk's lengths sum below 2^30)
    uint32_t overflow, flows;     // bt_flowtab_firsts
    uint32_t rel, pad0;           // bt_flowtab_join: flows of the chunks before this one
    uint32_t wflows[kFtWaves];    // bt_flowtab_firsts: first packets of wave w's tiles
    uint32_t klass_flows[5];      // ... by class
    uint32_t pad1[3];
};
static_assert(sizeof(FtPartial) == 96, "FtPartial layout");
static_assert(sizeof(bt_flow_rec) == 80 && sizeof(bt_flow_table_result) == 72 && sizeof(bt_flow_table_opts) == 16,
              "flow table ABI layout");

struct FtLayout { uint64_t slots, keys, pslot, firstw, parts, total; };   // byte offsets into the scratch

constexpr uint64_t ft_round(uint64_t x) { return (x + 255u) & ~255ull; }

// slots == 0: the smallest power of two >= max(128, 2 n); 0 when that is not a u32 (n > 2^30).
inline uint32_t ft_auto_slots(uint32_t n) {
    if (n > (1u << 30)) return 0u;
    uint32_t s = kFtMinSlots;
    while (s < 2u * n) s <<= 1;
    return s;
}

inline FtLayout ft_layout(uint32_t n, uint32_t slots) {
    const uint64_t ntiles = ((uint64_t)n + 63u) / 64u, nchunks = (ntiles + kFtChunkTiles - 1u) / kFtChunkTiles;
    FtLayout l{};
    l.slots = 0;
    l.keys = l.slots + ft_round((uint64_t)slots * 4u);
    l.pslot = l.keys + ft_round((uint64_t)n * sizeof(FtFlow));
    l.firstw = l.pslot + ft_round((uint64_t)n * 4u);
    l.parts = l.firstw + ft_round(ntiles * 8u);
    l.total = l.parts + ft_round(nchunks * sizeof(FtPartial));
    return l;
}

struct FlowtabArgs : FrameSrc {   // bytes = fan_read_end, as FanoutArgs
    uint32_t nchunks;
    uint32_t slots;               // a power of two
    uint32_t l3_only, bidir;
    uint32_t flow_cap;
    const uint64_t* select;
    uint32_t* tab;                // the slots' owner words
    FtFlow* keys;
    uint32_t* pslot;              // per packet: its flow's owner packet, kFtPending or a BT_FLOW_ID_* sentinel
    uint64_t* firstw;             // verdict-layout words: packet i is the first of its flow
    FtPartial* parts;
    uint32_t* flow_id;
    bt_flow_rec* flows;
    bt_flow_table_result* result;
};

// The checks on a bt_flow_table_opts for n packets; *slots = what opts->slots resolves to.
inline bool flowtab_opts(const bt_flow_table_opts* o, uint32_t n, uint32_t* slots, char* why, size_t cap) {
    const auto no = [&](const char* s) { snprintf(why, cap, "%s", s); return false; };
    if (!o) return no("null opts");
    if (o->flags & ~(BT_FLOWTAB_L3_ONLY | BT_FLOWTAB_BIDIRECTIONAL)) return no("unknown flag bits");
    uint32_t s = o->slots;
    if (!s && !(s = ft_auto_slots(n))) return no("slots == 0 (auto) needs n <= 2^30");
    if (s & (s - 1u)) return no("slots is not a power of two");
    if (s < kFtMinSlots) return no("slots below 128");
    *slots = s;
    return true;
}

// The checks of bt_flow_table_device on everything but the context, and the launch's arguments.
inline bool flowtab_args(const bt_batch* frames, const uint64_t* select, const bt_flow_table_opts* opts, void* scratch,
                         uint64_t scratch_bytes, const bt_flow_table_out* out, FlowtabArgs* a, char* why, size_t cap) {
    const auto no = [&](const char* s) { snprintf(why, cap, "%s", s); return false; };
    if (!frames) return no("null frames");
    if (!opts) return no("null opts");
    if (!out) return no("null out");
    if (!out->result) return no("null result");
    if (reinterpret_cast<uintptr_t>(out->result) & 7u) return no("result is not 8-byte aligned");
    if (reinterpret_cast<uintptr_t>(scratch) & 255u) return no("scratch is not 256-byte aligned");
    if (reinterpret_cast<uintptr_t>(out->flows) & 7u) return no("flows is not 8-byte aligned");
    if (reinterpret_cast<uintptr_t>(out->flow_id) & 3u) return no("flow_id is not 4-byte aligned");
    if (frames->flags & (BT_BATCH_PREFIXES | BT_BATCH_LEAN))
        return no("a BT_BATCH_PREFIXES / BT_BATCH_LEAN batch holds no whole frames to key");
    uint32_t slots = 0;
    if (!flowtab_opts(opts, frames->n, &slots, why, cap)) return false;
    if (frames->n > kFtPending) return no("n above 0xFFFFFFFC: packet indices would meet the flow id sentinels");
    if (!out->flows && opts->flow_cap) return no("null flows with flow_cap != 0");
    *a = FlowtabArgs{};
    if (frame_src(frames, a, why, cap)) return false;
    const FtLayout l = ft_layout(a->n, slots);
    if (a->n && !scratch) return no("null scratch");
    if (a->n && scratch_bytes < l.total) {
        snprintf(why, cap, "scratch_bytes %llu below the need %llu", (unsigned long long)scratch_bytes, (unsigned long long)l.total);
        return false;
    }
    a->bytes = fan_read_end(a->base, a->bytes);
    a->nchunks = (a->ntiles + kFtChunkTiles - 1u) / kFtChunkTiles;
    a->slots = slots;
    a->l3_only = (opts->flags & BT_FLOWTAB_L3_ONLY) ? 1u : 0u;
    a->bidir = (opts->flags & BT_FLOWTAB_BIDIRECTIONAL) ? 1u : 0u;
    a->flow_cap = opts->flow_cap;
    a->select = select;
    uint8_t* const s = static_cast<uint8_t*>(scratch);
    a->tab = reinterpret_cast<uint32_t*>(s + l.slots);
    a->keys = reinterpret_cast<FtFlow*>(s + l.keys);
    a->pslot = reinterpret_cast<uint32_t*>(s + l.pslot);
    a->firstw = reinterpret_cast<uint64_t*>(s + l.firstw);
    a->parts = reinterpret_cast<FtPartial*>(s + l.parts);
    a->flow_id = out->flow_id;
    a->flows = out->flows;
    a->result = out->result;
    return true;
}

// The canonical direction of a key of nb bytes (8, 12, 32 or 36: flow_key_host's): endpoint A =
// source address + source port, B = destination address + destination port, as byte strings.
// A > B: the endpoints are swapped in place and 1 is returned, else 0.
inline uint32_t ft_canonical(uint8_t in[kFanInputMax], uint32_t nb) {
    if (!nb) return 0u;
    const uint32_t alen = nb >= 32u ? 16u : 4u;
    const bool ports = nb == 2u * alen + 4u;
    int c = memcmp(in, in + alen, alen);
    if (!c && ports) c = memcmp(in + 2u * alen, in + 2u * alen + 2u, 2);
    if (c <= 0) return 0u;
    uint8_t t[16];
    memcpy(t, in, alen);
    memcpy(in, in + alen, alen);
    memcpy(in + alen, t, alen);
    if (ports) {
        memcpy(t, in + 2u * alen, 2);
        memcpy(in + 2u * alen, in + 2u * alen + 2u, 2);
        memcpy(in + 2u * alen + 2u, t, 2);
    }
    return 1u;
}

// bt_flow_table_host's work once its arguments are checked (`slots` resolved): a hash map from
// (class, key bytes) to the flow's number, packets in ascending order.
inline void flowtab_host(const uint8_t* base, uint64_t bytes, const bt_pkt_desc* desc, uint32_t n, const uint64_t* select,
                         uint32_t flags, uint32_t slots, uint32_t flow_cap, uint32_t* flow_id, bt_flow_rec* flows,
                         bt_flow_table_result* result) {
    struct Key {
        uint8_t b[40];   // class, then the 36 key bytes, then zeros
        bool operator==(const Key& o) const { return memcmp(b, o.b, sizeof(b)) == 0; }
    };
    struct Hash {
        size_t operator()(const Key& k) const {
            uint64_t h = 1469598103934665603ull;   // FNV-1a
            for (uint8_t x : k.b) h = (h ^ x) * 1099511628211ull;
            return (size_t)h;
        }
    };
    std::unordered_map<Key, uint32_t, Hash> ids;
    std::vector<bt_flow_rec> recs;
    bt_flow_table_result r{};
    r.n = n;
    r.slots = slots;
    for (uint32_t i = 0; i < n; ++i) {
        if (select && !((select[i >> 6] >> (i & 63u)) & 1ull)) {
            if (flow_id) flow_id[i] = BT_FLOW_ID_UNSELECTED;
            continue;
        }
        ++r.n_selected;
        const uint64_t off = BT_DESC_OFF(desc[i]);
        const uint32_t len = BT_DESC_LEN(desc[i]);
        const uint8_t* f = base + off;
        uint8_t tmp[128];   // the walk reads below offset 22 + 60 + 4
        if (off >= bytes || bytes - off < len) {   // the frame runs past `bytes`: its missing bytes read as zeros
            memset(tmp, 0, sizeof(tmp));
            const uint64_t have = off < bytes ? bytes - off : 0u;
            if (have) memcpy(tmp, base + off, have < sizeof(tmp) ? (size_t)have : sizeof(tmp));
            f = tmp;
        }
        Key k{};
        uint32_t klass = BT_FLOW_NONE;
        const uint32_t nb = flow_key_host(f, len, (flags & BT_FLOWTAB_L3_ONLY) != 0, k.b + 1, &klass);
        if (klass == BT_FLOW_NONE) {
            ++r.none_packets;
            r.none_bytes += len;
            if (flow_id) flow_id[i] = BT_FLOW_ID_NONE;
            continue;
        }
        r.keyed_bytes += len;
        const uint32_t dir = (flags & BT_FLOWTAB_BIDIRECTIONAL) ? ft_canonical(k.b + 1, nb) : 0u;
        k.b[0] = (uint8_t)klass;
        auto it = ids.find(k);
        if (it == ids.end()) {
            if (ids.size() >= slots) {   // the table is full
                ++r.overflow_packets;
                if (flow_id) flow_id[i] = BT_FLOW_ID_OVERFLOW;
                continue;
            }
            it = ids.emplace(k, (uint32_t)recs.size()).first;
            bt_flow_rec rec{};
            memcpy(rec.key, k.b + 1, kFanInputMax);
            rec.klass = (uint8_t)klass;
            rec.first = i;
            recs.push_back(rec);
            ++r.klass_flows[klass];
        }
        bt_flow_rec& rec = recs[it->second];
        rec.last = i;
        ++rec.packets[dir];
        rec.bytes[dir] += len;
        if (flow_id) flow_id[i] = it->second;
    }
    r.n_flows = (uint32_t)recs.size();
    r.n_written = r.n_flows < flow_cap ? r.n_flows : flow_cap;
    if (r.n_written) memcpy(flows, recs.data(), (size_t)r.n_written * sizeof(bt_flow_rec));
    *result = r;
}

// All launches, asynchronous on `stream`; n == 0 launches nothing (the caller writes *result).
int launch_flowtab(const FlowtabArgs& a, void* stream, void* timing_start = nullptr, void* timing_stop = nullptr);

}  // namespace bt
