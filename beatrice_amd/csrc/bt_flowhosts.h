// bt_flowhosts.h — the endpoint table of a flow tracker (bt_flowhosts.hip), shared with the host
// runtime (bt_flow_track_hosts_* in bt_flowhosts_host.cpp): the address of a contribution, the
// layout of the caller's scratch, the argument checks, and the group-by on the host over a state in
// host memory. The host part is plain C++ with no device and no runtime state:
// tools/flowhosts_host_check.cpp runs it under the host sanitizers.
#pragma once

#include <stdint.h>
#include <cstddef>
#include <cstring>
#include <vector>

#include "beatrice_gpu.h"
#include "bt_flowtrack.h"

namespace bt {

static_assert(sizeof(bt_flow_host_rec) == 128 && alignof(bt_flow_host_rec) == 8 && sizeof(bt_flow_hosts_opts) == 16 &&
              sizeof(bt_flow_hosts_result) == 64 && sizeof(bt_flow_hosts_out) == 24, "endpoint table ABI layout");
static_assert(offsetof(bt_flow_host_rec, family) == 16 && offsetof(bt_flow_host_rec, first_flow) == 20 &&
              offsetof(bt_flow_host_rec, flows) == 24 && offsetof(bt_flow_host_rec, packets) == 32 &&
              offsetof(bt_flow_host_rec, first_ts) == 64 && offsetof(bt_flow_host_rec, tcp_state) == 80 &&
              offsetof(bt_flow_host_rec, syn_flows) == 108 && offsetof(bt_flow_host_rec, syn_packets) == 116, "bt_flow_host_rec layout");
static_assert(offsetof(bt_flow_hosts_result, packets_total) == 32, "bt_flow_hosts_result layout");

constexpr uint32_t kFhEmpty = 0xFFFFFFFFu;        // a slot word that holds no host; a contribution without a slot
constexpr uint32_t kFhMaxFlows = 0x7FFFFFFFu;     // contribution indices 2 f + role stay below kFhEmpty
constexpr uint32_t kFhMaxAuto = 1u << 29;         // flow_cap at auto slots: 4 flow_cap is a u32 power of two
constexpr uint32_t kFhJoinThreads = 1024;
constexpr uint32_t kFhSumGrid = 2048;             // blocks of the grid-stride sum pass: what bounds the atomics on one host
constexpr uint32_t kFhCache = kFkThreads;         // hosts a block of the sum pass combines in LDS, one entry per thread

// slots == 0: the smallest power of two >= max(128, 4 flow_cap); 0 when flow_cap > 2^29.
inline uint32_t fh_auto_slots(uint32_t flow_cap) {
    if (flow_cap > kFhMaxAuto) return 0u;
    uint32_t s = kFtMinSlots;
    while ((uint64_t)s < 4ull * flow_cap) s <<= 1;
    return s;
}

// The address of a record's endpoint `role` as four little-endian words of the wire bytes, and its
// family: 6 for the IPv6 classes, 4 for every other. w: the record's first ten words.
BT_FK_HD inline uint32_t fh_addr(const uint32_t* w, uint32_t role, uint32_t (&a)[4]) {
    const uint32_t klass = w[9] & 0xFFu;
    if (klass == BT_FLOW_V6 || klass == BT_FLOW_V6_L4) {
        for (int d = 0; d < 4; ++d) a[d] = w[4u * role + d];
        return 6u;
    }
    a[0] = w[role]; a[1] = 0u; a[2] = 0u; a[3] = 0u;
    return 4u;
}

// The probe hash of a host: a fixed mix of the family and the four address words.
BT_FK_HD inline uint32_t fh_hash(uint32_t family, const uint32_t (&a)[4]) {
    uint32_t h = 0x9E3779B9u * (family + 1u);
    for (int d = 0; d < 4; ++d) {
        h += a[d] * 0xC2B2AE3Du;
        h = ((h << 17) | (h >> 15)) * 0x27D4EB2Fu;
    }
    h ^= h >> 15; h *= 0x85EBCA77u;
    h ^= h >> 13; h *= 0xC2B2AE3Du;
    return h ^ (h >> 16);
}

// Scratch control block, written by bt_flowhosts_begin, read by the kernels behind it.
struct FhCtl { uint32_t ok, n_flows, pad[2]; };

struct FhPart {                   // one per block of kFkThreads flows (bt_flowhosts_firsts)
    uint32_t nfirst, rel;         // first contributions of the block; of the blocks before it (bt_flowhosts_join)
    uint32_t nover, nv4;          // contributions without a slot; first contributions of family 4
    uint32_t wfirst[kFkWaves];    // first contributions of wave w
    uint64_t firstw[kFkWaves][2]; // wave w, role r: lane's contribution is its host's first
    uint64_t packets, bytes;      // the block's flows: packets[0] + packets[1], bytes[0] + bytes[1]
};
static_assert(sizeof(FhPart) == 112, "FhPart layout");

struct FhLayout { uint64_t ctl, tab, cslot, parts, total; };   // byte offsets into the scratch

inline FhLayout fh_scratch(uint32_t flow_cap, uint32_t slots) {
    FhLayout l{};
    l.ctl = 0;
    l.tab = l.ctl + ft_round(sizeof(FhCtl));
    l.cslot = l.tab + ft_round((uint64_t)slots * 4u);
    l.parts = l.cslot + ft_round((uint64_t)flow_cap * 8u);
    l.total = l.parts + ft_round(((uint64_t)flow_cap + kFkThreads - 1u) / kFkThreads * sizeof(FhPart));
    return l;
}

struct FlowhostsArgs {            // the kernels'
    const bt_flow_track_hdr* hdr;
    const bt_flow_track_rec* recs;
    const bt_flow_tcp_rec* tcp;   // nullptr without a side table
    uint32_t flags, flow_cap, state_slots;   // as the state was initialised: compared with *hdr on the device
    uint32_t slots, host_cap;     // the endpoint table's
    FhCtl* ctl;
    uint32_t* tab;                // per slot: empty, the lowest contribution of its host so far, after the rank the host's number
    uint32_t* cslot;              // per contribution: its host's slot, or kFhEmpty
    FhPart* parts;
    bt_flow_host_rec* hosts;
    uint32_t* endpoint_host;
    bt_flow_hosts_result* result;
};

// The check on an explicit `slots` (0 = auto passes), for every entry point.
inline bool flowhosts_slots(uint32_t slots, char* why, size_t cap) {
    const auto no = [&](const char* s) { snprintf(why, cap, "%s", s); return false; };
    if (slots && (slots & (slots - 1u))) return no("slots is not a power of two");
    if (slots && slots < kFtMinSlots) return no("slots below 128");
    return true;
}

// The checks on flow_cap; *resolved = what a checked `slots` resolves to for it.
inline bool flowhosts_geometry(uint32_t flow_cap, uint32_t slots, uint32_t* resolved, char* why, size_t cap) {
    const auto no = [&](const char* s) { snprintf(why, cap, "%s", s); return false; };
    if (!flow_cap) return no("flow_cap == 0");
    if (flow_cap > kFhMaxFlows) return no("flow_cap above 2^31 - 1: the last contribution index would be the empty slot word");
    uint32_t s = slots;
    if (!s && !(s = fh_auto_slots(flow_cap))) return no("slots == 0 (auto) needs flow_cap <= 2^29");
    *resolved = s;
    return true;
}

// The checks both forms share on opts, tcp and out.
inline bool flowhosts_common(const bt_flow_hosts_opts* opts, const bt_flow_tcp_rec* tcp, const bt_flow_hosts_out* out, char* why,
                             size_t cap) {
    const auto no = [&](const char* s) { snprintf(why, cap, "%s", s); return false; };
    if (!opts) return no("null opts");
    if (!out) return no("null out");
    if (!out->result) return no("null result");
    if (reinterpret_cast<uintptr_t>(out->result) & 7u) return no("result is not 8-byte aligned");
    if (reinterpret_cast<uintptr_t>(out->hosts) & 7u) return no("hosts is not 8-byte aligned");
    if (reinterpret_cast<uintptr_t>(tcp) & 3u) return no("tcp is not 4-byte aligned");
    if (reinterpret_cast<uintptr_t>(out->endpoint_host) & 3u) return no("endpoint_host is not 4-byte aligned");
    if (!flowhosts_slots(opts->slots, why, cap)) return false;
    if (opts->reserved[0] || opts->reserved[1]) return no("non-zero reserved fields");
    if (!out->hosts && opts->host_cap) return no("null hosts with host_cap != 0");
    return true;
}

// The checks of bt_flow_track_hosts_device on everything but the context, and the kernels'
// arguments. `sh`: the state's entry, nullptr = unknown.
inline bool flowhosts_args(const FkShadow* sh, const void* state, const bt_flow_hosts_opts* opts, const bt_flow_tcp_rec* tcp,
                           void* scratch, uint64_t scratch_bytes, const bt_flow_hosts_out* out, FlowhostsArgs* a, char* why,
                           size_t cap) {
    const auto no = [&](const char* s) { snprintf(why, cap, "%s", s); return false; };
    if (!state) return no("null state");
    if (reinterpret_cast<uintptr_t>(state) & 255u) return no("state is not 256-byte aligned");
    if (!scratch) return no("null scratch");
    if (reinterpret_cast<uintptr_t>(scratch) & 255u) return no("scratch is not 256-byte aligned");
    if (!flowhosts_common(opts, tcp, out, why, cap)) return false;
    // last of the checks but those the state's flow_cap decides
    if (!sh) return no("state is not an initialised tracker (bt_flow_track_init_device)");
    bt_flow_track_sizes sl{};
    if (!fk_layout(sh->flow_cap, sh->slots, &sl, why, cap)) return false;
    uint32_t slots = 0;
    if (!flowhosts_geometry(sh->flow_cap, opts->slots, &slots, why, cap)) return false;
    const FhLayout l = fh_scratch(sh->flow_cap, slots);
    if (scratch_bytes < l.total) {
        snprintf(why, cap, "scratch_bytes %llu below the need %llu", (unsigned long long)scratch_bytes, (unsigned long long)l.total);
        return false;
    }
    const uint8_t* const st = static_cast<const uint8_t*>(state);
    uint8_t* const s = static_cast<uint8_t*>(scratch);
    *a = FlowhostsArgs{};
    a->hdr = reinterpret_cast<const bt_flow_track_hdr*>(st + sl.header);
    a->recs = reinterpret_cast<const bt_flow_track_rec*>(st + sl.records);
    a->tcp = tcp;
    a->flags = sh->flags; a->flow_cap = sh->flow_cap; a->state_slots = sl.slots;
    a->slots = slots; a->host_cap = opts->host_cap;
    a->ctl = reinterpret_cast<FhCtl*>(s + l.ctl);
    a->tab = reinterpret_cast<uint32_t*>(s + l.tab);
    a->cslot = reinterpret_cast<uint32_t*>(s + l.cslot);
    a->parts = reinterpret_cast<FhPart*>(s + l.parts);
    a->hosts = out->hosts; a->endpoint_host = out->endpoint_host; a->result = out->result;
    return true;
}

// The checks of bt_flow_track_hosts_host; *hs: the checked state (never written through), *slots: resolved.
inline bool flowhosts_host_args(const void* state, uint64_t state_bytes, const bt_flow_hosts_opts* opts, const bt_flow_tcp_rec* tcp,
                                const bt_flow_hosts_out* out, FkHostState* hs, uint32_t* slots, char* why, size_t cap) {
    if (!state) { snprintf(why, cap, "%s", "null state"); return false; }
    if (reinterpret_cast<uintptr_t>(state) & 255u) { snprintf(why, cap, "%s", "state is not 256-byte aligned"); return false; }
    if (!flowhosts_common(opts, tcp, out, why, cap)) return false;
    if (!fk_host_state(const_cast<void*>(state), state_bytes, hs, why, cap)) return false;
    return flowhosts_geometry(hs->hdr->flow_cap, opts->slots, slots, why, cap);
}

// One contribution added to a host record: role r of flow record `rec` with its side record t (or nullptr).
inline void fh_add_host(bt_flow_host_rec& h, const bt_flow_track_rec& rec, const bt_flow_tcp_rec* t, uint32_t r, uint32_t flags) {
    h.flows[r] += 1u;
    h.packets[0] += rec.packets[r]; h.packets[1] += rec.packets[1u - r];
    h.bytes[0] += rec.bytes[r]; h.bytes[1] += rec.bytes[1u - r];
    if (rec.first_ts < h.first_ts) h.first_ts = rec.first_ts;
    if (rec.last_ts > h.last_ts) h.last_ts = rec.last_ts;
    if (t) {
        h.tcp_state[flowtcp_state(t->flags[0], t->flags[1], flags)] += 1u;
        h.syn_flows[0] += (t->flags[r] & BT_TCPF_SYN) ? 1u : 0u;
        h.syn_flows[1] += (t->flags[1u - r] & BT_TCPF_SYN) ? 1u : 0u;
        h.syn_packets += t->syn_packets; h.fin_packets += t->fin_packets; h.rst_packets += t->rst_packets;
    }
}

// bt_flow_track_hosts_host's work on a checked state and checked arguments: contributions in
// ascending order into an open-addressing table of `slots` words, so that a host's number is its
// order of first appearance and hosts that do not fit overflow as on the device.
inline void flowhosts_host(const FkHostState& s, uint32_t slots, const bt_flow_hosts_opts& o, const bt_flow_tcp_rec* tcp,
                           const bt_flow_hosts_out& out) {
    const uint32_t nf = s.hdr->n_flows, flags = s.hdr->flags, mask = slots - 1u;
    bt_flow_hosts_result r{};
    r.n_flows = nf; r.slots = slots;
    std::vector<uint32_t> tab(slots, kFhEmpty);    // per slot: the host's first contribution
    std::vector<uint32_t> num(slots, 0u);          // ... and its number
    for (uint32_t f = 0; f < nf; ++f) {
        const bt_flow_track_rec& rec = s.recs[f];
        uint32_t w[10];
        memcpy(w, &rec, sizeof(w));
        r.packets_total += rec.packets[0] + rec.packets[1];
        r.bytes_total += rec.bytes[0] + rec.bytes[1];
        for (uint32_t role = 0; role < 2u; ++role) {
            const uint32_t c = 2u * f + role;
            uint32_t a[4];
            const uint32_t family = fh_addr(w, role, a);
            uint32_t at = fh_hash(family, a) & mask, found = kFhEmpty;
            bool fresh = false;
            for (uint32_t probe = 0; probe < slots; ++probe, at = (at + 1u) & mask) {
                if (tab[at] == kFhEmpty) { tab[at] = c; num[at] = r.n_hosts; found = at; fresh = true; break; }
                uint32_t ow[10], oa[4];
                memcpy(ow, &s.recs[tab[at] >> 1], sizeof(ow));
                if (fh_addr(ow, tab[at] & 1u, oa) == family && memcmp(oa, a, sizeof(a)) == 0) { found = at; break; }
            }
            if (found == kFhEmpty) {
                ++r.overflow_endpoints;
                if (out.endpoint_host) out.endpoint_host[c] = kFhEmpty;
                continue;
            }
            const uint32_t h = num[found];
            if (fresh) {
                ++r.n_hosts;
                ++(family == 4u ? r.hosts_v4 : r.hosts_v6);
                if (h < o.host_cap) {
                    bt_flow_host_rec hr{};
                    memcpy(hr.addr, a, sizeof(a));
                    hr.family = (uint8_t)family;
                    hr.first_flow = f;
                    hr.first_ts = ~0ull;
                    out.hosts[h] = hr;
                }
            }
            if (h < o.host_cap) fh_add_host(out.hosts[h], rec, tcp ? tcp + f : nullptr, role, flags);
            if (out.endpoint_host) out.endpoint_host[c] = h;
        }
    }
    r.n_written = r.n_hosts < o.host_cap ? r.n_hosts : o.host_cap;
    *out.result = r;
}

// Asynchronous on `stream`. timing_start / timing_stop: recorded by the first / last kernel's own dispatch.
int launch_flowhosts(const FlowhostsArgs& a, void* stream, void* timing_start = nullptr, void* timing_stop = nullptr);

}  // namespace bt
