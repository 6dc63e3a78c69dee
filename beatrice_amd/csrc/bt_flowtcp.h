// bt_flowtcp.h — the per-flow TCP side table (bt_flowtcp.hip), shared with the host runtime
// (bt_flow_tcp_update_device / _host, bt_flow_tcp_state in bt_flowtcp_host.cpp) and with the flow
// tracker's TCP-aware expire (bt_flowtrack.h): the argument checks, the state of a flow as a
// function of its flag unions, and the update on the host. The host part is plain C++ with no
// device and no runtime state: tools/flowtcp_host_check.cpp runs it under the host sanitizers.
#pragma once

#include <stdint.h>
#include <cstddef>
#include <cstring>

#include "beatrice_gpu.h"
#include "bt_flowtab.h"

#ifdef __HIPCC__
#define BT_TCP_HD __host__ __device__
#else
#define BT_TCP_HD
#endif

namespace bt {

static_assert(sizeof(bt_flow_tcp_rec) == 16 && alignof(bt_flow_tcp_rec) == 4 && sizeof(bt_flow_tcp_result) == 32 &&
              sizeof(bt_flow_track_expire_tcp) == 24, "TCP side table ABI layout");
static_assert(offsetof(bt_flow_tcp_rec, syn_packets) == 4 && offsetof(bt_flow_tcp_rec, rst_packets) == 12, "bt_flow_tcp_rec layout");

constexpr uint32_t kTcpFlagsKnown = BT_FLOWTAB_L3_ONLY | BT_FLOWTAB_BIDIRECTIONAL;

// bt_flow_tcp_state: a function of the two unions, decided in this order.
BT_TCP_HD inline int flowtcp_state(uint32_t fwd, uint32_t rev, uint32_t table_flags) {
    const uint32_t u = fwd | rev;
    const bool bidir = (table_flags & BT_FLOWTAB_BIDIRECTIONAL) != 0;
    if (!u) return BT_TCP_NONE;
    if (u & BT_TCPF_RST) return BT_TCP_RESET;
    if (bidir ? (fwd & rev & BT_TCPF_FIN) != 0 : (fwd & BT_TCPF_FIN) != 0) return BT_TCP_CLOSED;
    if (u & BT_TCPF_FIN) return BT_TCP_CLOSING;
    if (!(u & BT_TCPF_SYN)) return BT_TCP_MIDSTREAM;
    if (bidir ? (fwd & rev & BT_TCPF_SYN) != 0 : (fwd & BT_TCPF_SYN) && (fwd & BT_TCPF_ACK)) return BT_TCP_ESTABLISHED;
    return BT_TCP_OPENING;
}

BT_TCP_HD inline bool flowtcp_is_sentinel(uint32_t id) {
    return id == BT_FLOW_ID_UNSELECTED || id == BT_FLOW_ID_NONE || id == BT_FLOW_ID_OVERFLOW || id == BT_FLOW_ID_EXPIRED;
}

struct FlowtcpArgs : FrameSrc {   // bytes = fan_read_end, as FlowtabArgs
    uint32_t nchunks;             // ceil(ntiles / kFtChunkTiles)
    uint32_t l3_only, bidir;      // as the table that numbered the flows
    uint32_t flow_cap;
    const uint32_t* flow_id;      // n entries
    bt_flow_tcp_rec* tcp;         // flow_cap records
    bt_flow_tcp_result* result;   // zero when the kernel starts: every block adds its sums
};

// The checks of bt_flow_tcp_update_device on everything but the context, and the launch's arguments.
inline bool flowtcp_args(const bt_batch* frames, const uint32_t* flow_id, uint32_t table_flags, bt_flow_tcp_rec* tcp, uint32_t flow_cap,
                         bt_flow_tcp_result* result, FlowtcpArgs* a, char* why, size_t cap) {
    const auto no = [&](const char* s) { snprintf(why, cap, "%s", s); return false; };
    if (!frames) return no("null frames");
    if (frames->n && !flow_id) return no("null flow_id");
    if (flow_cap && !tcp) return no("null tcp with flow_cap != 0");
    if (!result) return no("null result");
    if (reinterpret_cast<uintptr_t>(tcp) & 3u) return no("tcp is not 4-byte aligned");
    if (reinterpret_cast<uintptr_t>(flow_id) & 3u) return no("flow_id is not 4-byte aligned");
    if (reinterpret_cast<uintptr_t>(result) & 7u) return no("result is not 8-byte aligned");
    if (table_flags & ~kTcpFlagsKnown) return no("unknown flag bits");
    if (frames->flags & (BT_BATCH_PREFIXES | BT_BATCH_LEAN))
        return no("a BT_BATCH_PREFIXES / BT_BATCH_LEAN batch holds no whole frames to walk");
    *a = FlowtcpArgs{};
    if (frame_src(frames, a, why, cap)) return false;
    a->bytes = fan_read_end(a->base, a->bytes);
    a->nchunks = (a->ntiles + kFtChunkTiles - 1u) / kFtChunkTiles;
    a->l3_only = (table_flags & BT_FLOWTAB_L3_ONLY) ? 1u : 0u;
    a->bidir = (table_flags & BT_FLOWTAB_BIDIRECTIONAL) ? 1u : 0u;
    a->flow_cap = flow_cap;
    a->flow_id = flow_id;
    a->tcp = tcp;
    a->result = result;
    return true;
}

// The checks of bt_flow_tcp_update_host.
inline bool flowtcp_host_args(const uint8_t* base, const bt_pkt_desc* desc, uint32_t n, const uint32_t* flow_id, uint32_t table_flags,
                              const bt_flow_tcp_rec* tcp, uint32_t flow_cap, const bt_flow_tcp_result* result, char* why, size_t cap) {
    const auto no = [&](const char* s) { snprintf(why, cap, "%s", s); return false; };
    if (n && (!base || !desc)) return no("null base / desc");
    if (n && !flow_id) return no("null flow_id");
    if (flow_cap && !tcp) return no("null tcp with flow_cap != 0");
    if (!result) return no("null result");
    if (reinterpret_cast<uintptr_t>(tcp) & 3u) return no("tcp is not 4-byte aligned");
    if (reinterpret_cast<uintptr_t>(flow_id) & 3u) return no("flow_id is not 4-byte aligned");
    if (reinterpret_cast<uintptr_t>(result) & 7u) return no("result is not 8-byte aligned");
    if (table_flags & ~kTcpFlagsKnown) return no("unknown flag bits");
    return true;
}

// Does frame[0 .. len) hold a whole TCP header under the flow key's rule (flow_layers_host,
// bt_fanout.h: at most two tags, no IPv6 extension headers, no IPv4 fragment)? *flags = byte 13 of
// that header. Every byte read lies below len.
inline bool flowtcp_frame_host(const uint8_t* f, uint32_t len, uint32_t* flags) {
    const FlowLayersHost L = flow_layers_host(f, len);
    if (!L.l4 || L.proto != 6u) return false;
    *flags = f[L.o4 + 13u];
    return true;
}

// bt_flow_tcp_update_host's work once its arguments are checked: packets in ascending order.
inline void flowtcp_host(const uint8_t* base, uint64_t bytes, const bt_pkt_desc* desc, uint32_t n, const uint32_t* flow_id,
                         uint32_t table_flags, bt_flow_tcp_rec* tcp, uint32_t flow_cap, bt_flow_tcp_result* result) {
    bt_flow_tcp_result r{};
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
        uint8_t tmp[128];   // the walk reads below offset 22 + 60 + 14
        if (off >= bytes || bytes - off < len) {   // the frame runs past `bytes`: its missing bytes read as zeros
            memset(tmp, 0, sizeof(tmp));
            const uint64_t have = off < bytes ? bytes - off : 0u;
            if (have) memcpy(tmp, base + off, have < sizeof(tmp) ? (size_t)have : sizeof(tmp));
            f = tmp;
        }
        uint32_t fl = 0;
        if (!flowtcp_frame_host(f, len, &fl)) continue;
        uint32_t dir = 0;
        if (table_flags & BT_FLOWTAB_BIDIRECTIONAL) {   // the direction of the key the table forms under these flags
            uint8_t key[kFanInputMax] = {0};
            uint32_t klass = BT_FLOW_NONE;
            const uint32_t nb = flow_key_host(f, len, (table_flags & BT_FLOWTAB_L3_ONLY) != 0, key, &klass);
            dir = ft_canonical(key, nb);
        }
        bt_flow_tcp_rec& t = tcp[id];
        t.flags[dir] |= (uint8_t)fl;
        const uint32_t syn = (fl & BT_TCPF_SYN) && !(fl & BT_TCPF_ACK) ? 1u : 0u, fin = (fl & BT_TCPF_FIN) ? 1u : 0u,
                       rst = (fl & BT_TCPF_RST) ? 1u : 0u;
        t.syn_packets += syn; t.fin_packets += fin; t.rst_packets += rst;
        ++r.tcp_packets;
        r.syn_packets += syn; r.fin_packets += fin; r.rst_packets += rst;
    }
    *result = r;
}

// Asynchronous on `stream`; a.n > 0, *a.result zero in stream order before it (the caller's memset).
int launch_flowtcp(const FlowtcpArgs& a, void* stream, void* timing_start = nullptr, void* timing_stop = nullptr);

}  // namespace bt
