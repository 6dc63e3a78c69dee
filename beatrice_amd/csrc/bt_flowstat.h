// bt_flowstat.h — the per-flow statistics side table and the generic side-table move
// (bt_flowstat.hip), shared with the host runtime (bt_flow_stat_update_device / _host,
// bt_flow_stat_rtt, bt_flow_track_side_move_* in bt_flowstat_host.cpp): the argument checks, what
// one frame contributes, the update, the handshake round-trip times and the move on the host. The
// host part is plain C++ with no device and no runtime state: tools/flowstat_host_check.cpp runs
// it under the host sanitizers.
#pragma once

#include <stdint.h>
#include <cstddef>
#include <cstring>
#include <vector>

#include "beatrice_gpu.h"
#include "bt_flowtab.h"
#include "bt_flowtcp.h"

namespace bt {

static_assert(sizeof(bt_flow_stat_rec) == 128 && alignof(bt_flow_stat_rec) == 8 && sizeof(bt_flow_stat_result) == 32 &&
              sizeof(bt_flow_stat_rtt_out) == 32 && sizeof(bt_flow_side_move) == 48, "statistics side table ABI layout");
static_assert(offsetof(bt_flow_stat_rec, ttl_max) == 16 && offsetof(bt_flow_stat_rec, len_max) == 32 &&
              offsetof(bt_flow_stat_rec, payload_bytes) == 48 && offsetof(bt_flow_stat_rec, len_sq) == 64 &&
              offsetof(bt_flow_stat_rec, syn_ts_c) == 80 && offsetof(bt_flow_stat_rec, ack_ts_c) == 112, "bt_flow_stat_rec layout");

constexpr uint32_t kSideThreads = 256;            // the side move's blocks: one record per thread
constexpr uint32_t kSideWaves = kSideThreads / 64u;
constexpr uint32_t kSideJoinThreads = 1024;
constexpr uint32_t kSideMaxRecBytes = 256;

struct FlowstatArgs : FrameSrc {  // bytes = fan_read_end, as FlowtcpArgs
    uint32_t nchunks;             // ceil(ntiles / kFtChunkTiles)
    uint32_t l3_only, bidir;      // as the table that numbered the flows
    uint32_t flow_cap;
    const uint32_t* flow_id;      // n entries
    const uint64_t* ts;           // n entries, or nullptr: batch_ts
    uint64_t batch_ts;
    bt_flow_stat_rec* stat;       // flow_cap records
    bt_flow_stat_result* result;  // zero when the kernel starts: every block adds its sums
};

// The checks that the device and the host form share.
inline bool flowstat_common_args(const uint32_t* flow_id, uint32_t n, uint32_t table_flags, const bt_flow_track_update* upd,
                                 const bt_flow_stat_rec* stat, uint32_t flow_cap, const bt_flow_stat_result* result, char* why,
                                 size_t cap) {
    const auto no = [&](const char* s) { snprintf(why, cap, "%s", s); return false; };
    if (n && !flow_id) return no("null flow_id");
    if (!upd) return no("null upd");
    if (flow_cap && !stat) return no("null stat with flow_cap != 0");
    if (!result) return no("null result");
    if (reinterpret_cast<uintptr_t>(stat) & 7u) return no("stat is not 8-byte aligned");
    if (reinterpret_cast<uintptr_t>(flow_id) & 3u) return no("flow_id is not 4-byte aligned");
    if (reinterpret_cast<uintptr_t>(upd->ts) & 7u) return no("ts is not 8-byte aligned");
    if (reinterpret_cast<uintptr_t>(result) & 7u) return no("result is not 8-byte aligned");
    if (table_flags & ~kTcpFlagsKnown) return no("unknown flag bits");
    return true;
}

// The checks of bt_flow_stat_update_device on everything but the context, and the launch's arguments.
inline bool flowstat_args(const bt_batch* frames, const uint32_t* flow_id, uint32_t table_flags, const bt_flow_track_update* upd,
                          bt_flow_stat_rec* stat, uint32_t flow_cap, bt_flow_stat_result* result, FlowstatArgs* a, char* why,
                          size_t cap) {
    const auto no = [&](const char* s) { snprintf(why, cap, "%s", s); return false; };
    if (!frames) return no("null frames");
    if (!flowstat_common_args(flow_id, frames->n, table_flags, upd, stat, flow_cap, result, why, cap)) return false;
    if (frames->flags & (BT_BATCH_PREFIXES | BT_BATCH_LEAN))
        return no("a BT_BATCH_PREFIXES / BT_BATCH_LEAN batch holds no whole frames to walk");
    *a = FlowstatArgs{};
    if (frame_src(frames, a, why, cap)) return false;
    a->bytes = fan_read_end(a->base, a->bytes);
    a->nchunks = (a->ntiles + kFtChunkTiles - 1u) / kFtChunkTiles;
    a->l3_only = (table_flags & BT_FLOWTAB_L3_ONLY) ? 1u : 0u;
    a->bidir = (table_flags & BT_FLOWTAB_BIDIRECTIONAL) ? 1u : 0u;
    a->flow_cap = flow_cap;
    a->flow_id = flow_id;
    a->ts = upd->ts;
    a->batch_ts = upd->batch_ts;
    a->stat = stat;
    a->result = result;
    return true;
}

// The checks of bt_flow_stat_update_host.
inline bool flowstat_host_args(const uint8_t* base, const bt_pkt_desc* desc, uint32_t n, const uint32_t* flow_id, uint32_t table_flags,
                               const bt_flow_track_update* upd, const bt_flow_stat_rec* stat, uint32_t flow_cap,
                               const bt_flow_stat_result* result, char* why, size_t cap) {
    if (n && (!base || !desc)) { snprintf(why, cap, "null base / desc"); return false; }
    return flowstat_common_args(flow_id, n, table_flags, upd, stat, flow_cap, result, why, cap);
}

// What one frame contributes (bt_flow_stat_rec in include/beatrice_gpu.h), before its direction.
struct FlowstatFacts {
    bool ip, l4, tcp;             // a whole IPv4 / IPv6 header; a whole TCP / UDP header under the key's rule; ... and protocol 6
    uint32_t seen;                // BT_FSEEN_*, unshifted
    uint32_t proto, ttl, len;     // len = min(frame length, 65535)
    uint32_t payload;             // L4 payload bytes from the header fields; 0 without l4
    uint32_t stamp;               // which handshake stamp the packet sets: 0 syn, 1 synack, 2 ack, 3 none
};

// frame[0 .. len) under flow_layers_host. Every byte read lies below len.
inline FlowstatFacts flowstat_frame_host(const uint8_t* f, uint32_t len) {
    FlowstatFacts x{};
    x.stamp = 3u;
    const FlowLayersHost L = flow_layers_host(f, len);
    if (!L.v4 && !L.v6) return x;
    x.ip = true;
    x.l4 = L.l4;
    x.tcp = L.l4 && L.proto == 6u;
    x.proto = L.proto;
    x.len = len < 65535u ? len : 65535u;
    const uint8_t* ip = f + L.o3;
    const uint32_t ihl = ip[0] & 0xFu;
    x.ttl = L.v4 ? ip[8] : ip[7];
    x.seen = L.proto == 6u ? BT_FSEEN_TCP : L.proto == 17u ? BT_FSEEN_UDP : L.v4 && L.proto == 1u ? BT_FSEEN_ICMP
             : L.v6 && L.proto == 58u ? BT_FSEEN_ICMP6 : BT_FSEEN_OTHER;
    if (L.v4 && (((uint32_t)ip[6] << 8 | ip[7]) & 0x3FFFu)) x.seen |= BT_FSEEN_FRAGMENT;
    if (L.v4 && ihl > 5u) x.seen |= BT_FSEEN_IP_OPTIONS;
    if (L.o3 > 14u) x.seen |= BT_FSEEN_VLAN;
    if (!L.l4) return x;
    x.seen |= BT_FSEEN_L4;
    const int32_t ip_payload = L.v4 ? (int32_t)((uint32_t)ip[2] << 8 | ip[3]) - (int32_t)(4u * ihl) : (int32_t)((uint32_t)ip[4] << 8 | ip[5]);
    const uint8_t* l4 = f + L.o4;
    const int32_t hdr = x.tcp ? (int32_t)(4u * (l4[12] >> 4)) : 8;
    x.payload = ip_payload > hdr ? (uint32_t)(ip_payload - hdr) : 0u;
    if (x.tcp) {
        const uint32_t fl = l4[13];
        const bool syn = fl & BT_TCPF_SYN, ack = fl & BT_TCPF_ACK, rst = fl & BT_TCPF_RST;
        x.stamp = syn ? (ack ? 1u : 0u) : ack && !rst ? 2u : 3u;
    }
    return x;
}

inline void flowstat_max32(uint32_t& to, uint32_t v) { if (v > to) to = v; }
inline void flowstat_max64(uint64_t& to, uint64_t v) { if (v > to) to = v; }

// bt_flow_stat_update_host's work once its arguments are checked: packets in ascending order.
inline void flowstat_host(const uint8_t* base, uint64_t bytes, const bt_pkt_desc* desc, uint32_t n, const uint32_t* flow_id,
                          uint32_t table_flags, const bt_flow_track_update* upd, bt_flow_stat_rec* stat, uint32_t flow_cap,
                          bt_flow_stat_result* result) {
    bt_flow_stat_result r{};
    r.n = n;
    for (uint32_t i = 0; i < n; ++i) {
        const uint32_t id = flow_id[i];
        if (id >= flow_cap) {
            if (!flowtcp_is_sentinel(id)) ++r.bad_ids;
            continue;
        }
        const uint64_t off = BT_DESC_OFF(desc[i]);
        const uint32_t len = BT_DESC_LEN(desc[i]);
        const uint8_t* f = base + off;
        uint8_t tmp[128];   // the walk and the header fields lie below offset 22 + 60 + 20
        if (off >= bytes || bytes - off < len) {   // the frame runs past `bytes`: its missing bytes read as zeros
            memset(tmp, 0, sizeof(tmp));
            const uint64_t have = off < bytes ? bytes - off : 0u;
            if (have) memcpy(tmp, base + off, have < sizeof(tmp) ? (size_t)have : sizeof(tmp));
            f = tmp;
        }
        const FlowstatFacts x = flowstat_frame_host(f, len);
        if (!x.ip) continue;
        uint32_t dir = 0;
        if (table_flags & BT_FLOWTAB_BIDIRECTIONAL) {   // the direction of the key the table forms under these flags
            uint8_t key[kFanInputMax] = {0};
            uint32_t klass = BT_FLOW_NONE;
            const uint32_t nb = flow_key_host(f, len, (table_flags & BT_FLOWTAB_L3_ONLY) != 0, key, &klass);
            dir = ft_canonical(key, nb);
        }
        bt_flow_stat_rec& s = stat[id];
        s.seen |= x.seen << (16u * dir);
        flowstat_max32(s.proto_max, x.proto);
        flowstat_max32(s.ttl_max[dir], x.ttl);
        flowstat_max32(s.ttl_min_c[dir], ~x.ttl);
        flowstat_max32(s.len_max[dir], x.len);
        flowstat_max32(s.len_min_c[dir], ~x.len);
        s.len_sq[dir] += (uint64_t)x.len * x.len;
        s.payload_bytes[dir] += x.payload;
        s.payload_packets[dir] += x.payload ? 1u : 0u;
        if (x.stamp < 3u) {
            const uint64_t t = ~(upd->ts ? upd->ts[i] : upd->batch_ts);
            flowstat_max64(x.stamp == 0u ? s.syn_ts_c[dir] : x.stamp == 1u ? s.synack_ts_c[dir] : s.ack_ts_c[dir], t);
        }
        ++r.ip_packets;
        r.l4_packets += x.l4 ? 1u : 0u;
        r.tcp_packets += x.tcp ? 1u : 0u;
    }
    *result = r;
}

// bt_flow_stat_rtt.
inline void flowstat_rtt(const bt_flow_stat_rec& s, bt_flow_stat_rtt_out* out) {
    *out = bt_flow_stat_rtt_out{};
    const bool s0 = s.syn_ts_c[0] != 0, s1 = s.syn_ts_c[1] != 0;
    if (!s0 && !s1) return;
    const uint32_t d = s0 && s1 ? (~s.syn_ts_c[1] < ~s.syn_ts_c[0] ? 1u : 0u) : s0 ? 0u : 1u;
    out->has_initiator = 1u;
    out->initiator = d;
    const uint64_t syn = ~s.syn_ts_c[d], synack = ~s.synack_ts_c[1u - d], ack = ~s.ack_ts_c[d];
    if (!s.synack_ts_c[1u - d] || synack < syn) return;
    out->server_valid = 1u;
    out->rtt_server = synack - syn;
    if (!s.ack_ts_c[d] || ack < synack) return;
    out->client_valid = 1u;
    out->rtt_client = ack - synack;
}

// ---- the side-table move -----------------------------------------------------------------

struct FsPart { uint32_t nexp, rel; uint32_t wexp[kSideWaves]; };   // scratch, one per block of flows (bt_flowside_mark)
static_assert(sizeof(FsPart) == 24, "FsPart layout");

struct FsLayout { uint64_t tmp, parts, total; };   // byte offsets into a move's scratch

inline FsLayout fs_scratch(uint32_t flow_cap, uint32_t rec_bytes) {
    FsLayout l{};
    l.tmp = 0;
    l.parts = ft_round((uint64_t)flow_cap * rec_bytes);
    l.total = l.parts + ft_round(((uint64_t)flow_cap + kSideThreads - 1u) / kSideThreads * sizeof(FsPart));
    return l;
}

struct FlowsideArgs {
    uint32_t* side;               // flow_cap records of rec_words words
    uint32_t* expired_side;       // expired_cap records, or nullptr
    const uint32_t* remap;
    const bt_flow_track_expire_result* result;
    uint32_t rec_words, flow_cap, expired_cap;
    uint32_t* tmp;                // scratch: flow_cap records
    FsPart* parts;
};

inline bool flowside_rec_bytes_ok(uint32_t rec_bytes) { return rec_bytes >= 4u && rec_bytes <= kSideMaxRecBytes && !(rec_bytes & 3u); }

// The checks of bt_flow_track_side_move_host, and of the device form on everything but the scratch and the context.
inline bool flowside_common_args(const bt_flow_side_move* m, char* why, size_t cap) {
    const auto no = [&](const char* s) { snprintf(why, cap, "%s", s); return false; };
    if (!m) return no("null move");
    if (m->flow_cap && !m->side) return no("null side with flow_cap != 0");
    if (m->flow_cap && !m->remap) return no("null remap with flow_cap != 0");
    if (!m->result) return no("null result");
    if (reinterpret_cast<uintptr_t>(m->side) & 3u) return no("side is not 4-byte aligned");
    if (reinterpret_cast<uintptr_t>(m->expired_side) & 3u) return no("expired_side is not 4-byte aligned");
    if (reinterpret_cast<uintptr_t>(m->remap) & 3u) return no("remap is not 4-byte aligned");
    if (reinterpret_cast<uintptr_t>(m->result) & 7u) return no("result is not 8-byte aligned");
    if (!flowside_rec_bytes_ok(m->rec_bytes)) return no("rec_bytes is not a multiple of 4 in 4 .. 256");
    if (m->expired_cap && !m->expired_side) return no("expired_cap != 0 without expired_side");
    if (m->reserved) return no("reserved is not 0");
    return true;
}

inline bool flowside_args(const bt_flow_side_move* m, void* scratch, uint64_t scratch_bytes, FlowsideArgs* a, char* why, size_t cap) {
    const auto no = [&](const char* s) { snprintf(why, cap, "%s", s); return false; };
    if (!flowside_common_args(m, why, cap)) return false;
    if (!scratch) return no("null scratch");
    if (reinterpret_cast<uintptr_t>(scratch) & 255u) return no("scratch is not 256-byte aligned");
    const FsLayout l = fs_scratch(m->flow_cap, m->rec_bytes);
    if (scratch_bytes < l.total) {
        snprintf(why, cap, "scratch_bytes %llu below the need %llu", (unsigned long long)scratch_bytes, (unsigned long long)l.total);
        return false;
    }
    uint8_t* const s = static_cast<uint8_t*>(scratch);
    *a = FlowsideArgs{static_cast<uint32_t*>(m->side), static_cast<uint32_t*>(m->expired_side), m->remap, m->result, m->rec_bytes / 4u,
                      m->flow_cap, m->expired_side ? m->expired_cap : 0u, reinterpret_cast<uint32_t*>(s + l.tmp),
                      reinterpret_cast<FsPart*>(s + l.parts)};
    return true;
}

// bt_flow_track_side_move_host's work once its arguments are checked.
inline void flowside_host(const bt_flow_side_move* m) {
    const uint32_t nb = m->result->n_flows_before < m->flow_cap ? m->result->n_flows_before : m->flow_cap;
    const uint32_t nl = m->result->n_flows < nb ? m->result->n_flows : nb;
    if (nl == nb) return;   // nothing left the tracker: remap is the identity
    const size_t rb = m->rec_bytes;
    uint8_t* const side = static_cast<uint8_t*>(m->side);
    uint8_t* const gone = static_cast<uint8_t*>(m->expired_side);
    std::vector<uint8_t> tmp((size_t)nl * rb, 0);
    uint32_t k = 0;
    for (uint32_t old = 0; old < nb; ++old) {
        const uint32_t to = m->remap[old];
        if (to == BT_FLOW_ID_EXPIRED) {
            if (gone && k < m->expired_cap) memcpy(gone + (size_t)k * rb, side + (size_t)old * rb, rb);
            ++k;
        } else if (to < nl) {
            memcpy(tmp.data() + (size_t)to * rb, side + (size_t)old * rb, rb);
        }
    }
    if (nl) memcpy(side, tmp.data(), (size_t)nl * rb);
    memset(side + (size_t)nl * rb, 0, (size_t)(nb - nl) * rb);
}

// Asynchronous on `stream`; a.n > 0, *a.result zero in stream order before it (the caller's memset).
int launch_flowstat(const FlowstatArgs& a, void* stream, void* timing_start = nullptr, void* timing_stop = nullptr);
// All four launches, asynchronous on `stream`; flow_cap == 0 launches nothing.
int launch_flowside(const FlowsideArgs& a, void* stream);

}  // namespace bt
