// bt_flowtcpseq.h — TCP segments classified per flow and direction against the sequence space
// (bt_flowtcpseq.hip), shared with the host runtime (bt_flow_tcpseq_device / bt_flow_tcpseq_host in
// bt_flowtcpseq_host.cpp): the layout of the caller's scratch, the argument checks, what one frame
// contributes and the pass on the host. The host part is plain C++ with no device and no runtime
// state: tools/flowtcpseq_host_check.cpp runs it under the host sanitizers.
#pragma once

#include <stdint.h>
#include <cstddef>
#include <cstdio>
#include <cstring>

#include "beatrice_gpu.h"
#include "beatrice_gpu_bench.h"
#include "bt_fanout.h"
#include "bt_flowseq.h"
#include "bt_flowstream.h"

namespace bt {

static_assert(sizeof(bt_flow_tcpseq_dir) == 64 && sizeof(bt_flow_tcpseq_rec) == 128 && alignof(bt_flow_tcpseq_rec) == 8 &&
              sizeof(bt_flow_tcpseq_out) == 48 && sizeof(bt_flow_tcpseq_result) == 64, "TCP sequence side table ABI layout");
static_assert(offsetof(bt_flow_tcpseq_dir, last_seq) == 16 && offsetof(bt_flow_tcpseq_dir, seq_packets) == 24 &&
              offsetof(bt_flow_tcpseq_dir, old_bytes) == 40 && offsetof(bt_flow_tcpseq_result, seq_bytes) == 40,
              "bt_flow_tcpseq_dir / _result layout");

struct FtsMeta { uint32_t seq, len_dir; };   // scratch, per packet: tcp[4 .. 8) as a number; L (below 2^17) | dir << 31
struct FtsDl { int32_t delta; uint32_t len; };   // scratch, per sorted pair: the step from the pair before it in its key; L
// scratch, one per unit: the unit's pairs since its last head under the scan's operator. any == 0
// is the operator's identity (0, -inf): nothing behind it, so no value stands in for -inf.
struct FtsCarry { int64_t S, M; uint32_t head, any; };
static_assert(sizeof(FtsMeta) == 8 && sizeof(FtsDl) == 8 && sizeof(FtsCarry) == 24, "flowtcpseq scratch layout");

struct FtsLayout { uint64_t head, numw, parts, a, b, dcnt, drel, dwcnt, dstart, meta, dl, carry, total; };   // byte offsets

inline FtsLayout fts_layout(uint32_t n) {
    const uint64_t ntiles = ((uint64_t)n + 63u) / 64u, nchunks = (ntiles + kFtChunkTiles - 1u) / kFtChunkTiles;
    FtsLayout l{};
    l.head = 0;
    l.numw = l.head + sizeof(FsHead);
    l.parts = l.numw + ft_round(ntiles * 8u);
    l.a = l.parts + ft_round(nchunks * sizeof(FsPart));
    l.b = l.a + ft_round((uint64_t)n * sizeof(FsPair));
    l.dcnt = l.b + ft_round((uint64_t)n * sizeof(FsPair));
    l.drel = l.dcnt + ft_round(nchunks * kFsDigits * 4u);
    l.dwcnt = l.drel + ft_round(nchunks * kFsDigits * 4u);
    l.dstart = l.dwcnt + ft_round(nchunks * kFtWaves * kFsDigits * 4u);
    l.meta = l.dstart + ft_round(kFsDigits * 4u);
    l.dl = l.meta + ft_round((uint64_t)n * sizeof(FtsMeta));
    l.carry = l.dl + ft_round((uint64_t)n * sizeof(FtsDl));
    l.total = l.carry + ft_round(nchunks * kFtWaves * sizeof(FtsCarry));
    return l;
}

struct FlowtcpseqArgs : FrameSrc {   // bytes = fan_read_end, as FlowstatArgs
    uint32_t nchunks;             // ceil(ntiles / kFtChunkTiles)
    uint32_t l3_only, bidir;      // as the table that numbered the flows
    uint32_t flow_cap;
    uint32_t passes;              // fst_passes(flow_cap): the key is flow << 1 | dir
    const uint32_t* flow_id;      // n entries
    const uint64_t* select;       // ntiles words, or nullptr: every packet; may be out_select
    bt_flow_tcpseq_rec* table;    // flow_cap records
    uint8_t* cls;                 // optional outputs
    int64_t* off;
    uint64_t* out_select;
    bt_flow_tcpseq_result* result;   // zero when the first kernel starts: every wave adds its sums
    FsHead* head;                 // the scratch, by fts_layout
    uint64_t* numw;
    FsPart* parts;
    FsPair *a, *b;
    uint32_t *dcnt, *drel, *dwcnt, *dstart;
    FtsMeta* meta;
    FtsDl* dl;
    FtsCarry* carry;
};

// The checks that the device and the host form share.
inline bool flowtcpseq_common_args(const uint32_t* flow_id, uint32_t n, const uint64_t* select, uint32_t table_flags,
                                   const bt_flow_tcpseq_rec* table, uint32_t flow_cap, const bt_flow_tcpseq_out* out, char* why,
                                   size_t cap) {
    const auto no = [&](const char* s) { snprintf(why, cap, "%s", s); return false; };
    if (!out) return no("null out");
    if (!out->result) return no("null result");
    if (n && !flow_id) return no("null flow_id");
    if (flow_cap && !table) return no("null table with flow_cap != 0");
    if (reinterpret_cast<uintptr_t>(flow_id) & 3u) return no("flow_id is not 4-byte aligned");
    if (reinterpret_cast<uintptr_t>(table) & 7u) return no("table is not 8-byte aligned");
    if (reinterpret_cast<uintptr_t>(select) & 7u) return no("select is not 8-byte aligned");
    if (reinterpret_cast<uintptr_t>(out->off) & 7u) return no("off is not 8-byte aligned");
    if (reinterpret_cast<uintptr_t>(out->out_select) & 7u) return no("out_select is not 8-byte aligned");
    if (reinterpret_cast<uintptr_t>(out->result) & 7u) return no("result is not 8-byte aligned");
    if (table_flags & ~kTcpFlagsKnown) return no("unknown flag bits");
    if (out->reserved[0] || out->reserved[1]) return no("reserved is not 0");
    if (flow_cap > kFstFlowCapMax) return no("flow_cap above 2^31");
    return true;
}

// The checks of bt_flow_tcpseq_device on everything but the context, and the launches' arguments.
inline bool flowtcpseq_args(const bt_batch* frames, const uint32_t* flow_id, const uint64_t* select, uint32_t table_flags,
                            bt_flow_tcpseq_rec* table, uint32_t flow_cap, void* scratch, uint64_t scratch_bytes,
                            const bt_flow_tcpseq_out* out, FlowtcpseqArgs* a, char* why, size_t cap) {
    const auto no = [&](const char* s) { snprintf(why, cap, "%s", s); return false; };
    if (!frames) return no("null frames");
    if (!flowtcpseq_common_args(flow_id, frames->n, select, table_flags, table, flow_cap, out, why, cap)) return false;
    if (reinterpret_cast<uintptr_t>(scratch) & 255u) return no("scratch is not 256-byte aligned");
    if (frames->flags & (BT_BATCH_PREFIXES | BT_BATCH_LEAN))
        return no("a BT_BATCH_PREFIXES / BT_BATCH_LEAN batch holds no whole frames to walk");
    *a = FlowtcpseqArgs{};
    if (frame_src(frames, a, why, cap)) return false;
    const FtsLayout l = fts_layout(a->n);
    if (a->n && !scratch) return no("null scratch");
    if (a->n && scratch_bytes < l.total) {
        snprintf(why, cap, "scratch_bytes %llu below the need %llu", (unsigned long long)scratch_bytes, (unsigned long long)l.total);
        return false;
    }
    a->bytes = fan_read_end(a->base, a->bytes);
    a->nchunks = (a->ntiles + kFtChunkTiles - 1u) / kFtChunkTiles;
    a->l3_only = (table_flags & BT_FLOWTAB_L3_ONLY) ? 1u : 0u;
    a->bidir = (table_flags & BT_FLOWTAB_BIDIRECTIONAL) ? 1u : 0u;
    a->flow_cap = flow_cap;
    a->passes = fst_passes(flow_cap);
    a->flow_id = flow_id;
    a->select = select;
    a->table = table;
    a->cls = out->cls;
    a->off = out->off;
    a->out_select = out->out_select;
    a->result = out->result;
    uint8_t* const s = static_cast<uint8_t*>(scratch);
    a->head = reinterpret_cast<FsHead*>(s + l.head);
    a->numw = reinterpret_cast<uint64_t*>(s + l.numw);
    a->parts = reinterpret_cast<FsPart*>(s + l.parts);
    a->a = reinterpret_cast<FsPair*>(s + l.a);
    a->b = reinterpret_cast<FsPair*>(s + l.b);
    a->dcnt = reinterpret_cast<uint32_t*>(s + l.dcnt);
    a->drel = reinterpret_cast<uint32_t*>(s + l.drel);
    a->dwcnt = reinterpret_cast<uint32_t*>(s + l.dwcnt);
    a->dstart = reinterpret_cast<uint32_t*>(s + l.dstart);
    a->meta = reinterpret_cast<FtsMeta*>(s + l.meta);
    a->dl = reinterpret_cast<FtsDl*>(s + l.dl);
    a->carry = reinterpret_cast<FtsCarry*>(s + l.carry);
    return true;
}

// The checks of bt_flow_tcpseq_host.
inline bool flowtcpseq_host_args(const uint8_t* base, const bt_pkt_desc* desc, uint32_t n, const uint32_t* flow_id,
                                 const uint64_t* select, uint32_t table_flags, const bt_flow_tcpseq_rec* table, uint32_t flow_cap,
                                 const bt_flow_tcpseq_out* out, char* why, size_t cap) {
    if (!flowtcpseq_common_args(flow_id, n, select, table_flags, table, flow_cap, out, why, cap)) return false;
    if (n && (!base || !desc)) { snprintf(why, cap, "null base / desc"); return false; }
    return true;
}

// What one frame contributes, before its flow: frame[0 .. len) with the bytes of its first 128
// in f (zeros where the frame has none).
struct FlowtcpseqFacts {
    uint32_t L;       // the sequence length from the header fields; 0: the packet does not participate
    uint32_t seq;     // tcp[4 .. 8), big-endian
    uint32_t dir;     // the TCP side table's direction under table_flags
};

inline FlowtcpseqFacts flowtcpseq_frame_host(const uint8_t* f, uint32_t len, uint32_t table_flags) {
    FlowtcpseqFacts x{};
    const FlowLayersHost L = flow_layers_host(f, len);
    if (!(L.v4 || L.v6) || !L.l4 || L.proto != 6u) return x;
    const uint8_t* ip = f + L.o3;
    const uint8_t* t = f + L.o4;
    const int32_t ip_payload = L.v4 ? (int32_t)((uint32_t)ip[2] << 8 | ip[3]) - (int32_t)(4u * (ip[0] & 0xFu)) : (int32_t)((uint32_t)ip[4] << 8 | ip[5]);
    const int32_t hdr = (int32_t)(4u * (t[12] >> 4));
    const uint32_t plen = ip_payload > hdr ? (uint32_t)(ip_payload - hdr) : 0u;
    x.L = plen + ((t[13] & BT_TCPF_SYN) ? 1u : 0u) + ((t[13] & BT_TCPF_FIN) ? 1u : 0u);
    x.seq = (uint32_t)t[4] << 24 | (uint32_t)t[5] << 16 | (uint32_t)t[6] << 8 | t[7];
    if (table_flags & BT_FLOWTAB_BIDIRECTIONAL) {
        uint8_t key[kFanInputMax] = {0};
        uint32_t klass = BT_FLOW_NONE;
        const uint32_t nb = flow_key_host(f, len, (table_flags & BT_FLOWTAB_L3_ONLY) != 0, key, &klass);
        x.dir = ft_canonical(key, nb);
    }
    return x;
}

// One participating packet against its direction's record: the definition. Returns the class,
// *u = the packet's unwrapped start. Sums wrap as unsigned numbers do.
inline uint32_t flowtcpseq_step(bt_flow_tcpseq_dir& d, uint32_t s, uint32_t L, int64_t* u, uint64_t* oldb, uint64_t* gapb) {
    uint32_t k;
    *oldb = *gapb = 0;
    if (!d.have) {
        *u = 0;
        d.hi = (int64_t)L;
        d.have = 1u;
        k = BT_TCPSEQ_FIRST;
    } else {
        const int64_t at = (int64_t)((uint64_t)d.pos + (uint64_t)(int64_t)(int32_t)(s - d.last_seq));
        const int64_t e = (int64_t)((uint64_t)at + L);
        *u = at;
        if (at == d.hi) {
            k = BT_TCPSEQ_IN_ORDER;
        } else if (at > d.hi) {
            k = BT_TCPSEQ_GAP;
            *gapb = (uint64_t)at - (uint64_t)d.hi;
        } else if (e <= d.hi) {
            k = BT_TCPSEQ_OLD;
            *oldb = L;
        } else {
            k = BT_TCPSEQ_OVERLAP;
            *oldb = (uint64_t)d.hi - (uint64_t)at;
        }
        if (e > d.hi) d.hi = e;
    }
    d.pos = *u;
    d.last_seq = s;
    ++d.seq_packets;
    if (k == BT_TCPSEQ_OLD) ++d.old_packets;
    if (k == BT_TCPSEQ_GAP) ++d.gap_packets;
    if (k == BT_TCPSEQ_OVERLAP) ++d.overlap_packets;
    d.old_bytes += *oldb;
    d.gap_bytes += *gapb;
    return k;
}

// bt_flow_tcpseq_host's work once its arguments are checked: packets in ascending order, a select
// word read before its out_select word is written, so the two may be one.
inline void flowtcpseq_host(const uint8_t* base, uint64_t bytes, const bt_pkt_desc* desc, uint32_t n, const uint32_t* flow_id,
                            const uint64_t* select, uint32_t table_flags, bt_flow_tcpseq_rec* table, uint32_t flow_cap,
                            const bt_flow_tcpseq_out* out) {
    bt_flow_tcpseq_result r{};
    r.n = n;
    const uint32_t nwords = (uint32_t)(((uint64_t)n + 63u) / 64u);
    for (uint32_t w = 0; w < nwords; ++w) {
        const uint32_t left = n - w * 64u, cnt = left < 64u ? left : 64u;
        const uint64_t valid = cnt == 64u ? ~0ull : (1ull << cnt) - 1ull;
        const uint64_t sw = (select ? select[w] : ~0ull) & valid;
        uint64_t o = sw;
        for (uint32_t b = 0; b < cnt; ++b) {
            const uint32_t i = w * 64u + b;
            uint32_t k = BT_TCPSEQ_NONE;
            int64_t u = BT_TCPSEQ_OFF_NONE;
            if ((sw >> b) & 1ull) {
                ++r.selected;
                const uint32_t id = flow_id[i];
                if (id >= flow_cap) {
                    if (flowtcp_is_sentinel(id)) ++r.unkeyed; else ++r.bad_ids;
                } else {
                    const uint64_t off = BT_DESC_OFF(desc[i]);
                    const uint32_t len = BT_DESC_LEN(desc[i]);
                    uint8_t head[128] = {0};   // the walk and the header fields lie below offset 22 + 60 + 20
                    for (uint32_t q = 0; q < 128u && q < len && off + q < bytes; ++q) head[q] = base[off + q];
                    const FlowtcpseqFacts x = flowtcpseq_frame_host(head, len, table_flags);
                    if (x.L) {
                        uint64_t oldb, gapb;
                        k = flowtcpseq_step(table[id].d[x.dir], x.seq, x.L, &u, &oldb, &gapb);
                        ++r.seq_packets;
                        r.seq_bytes += x.L;
                        r.old_bytes += oldb;
                        r.gap_bytes += gapb;
                        if (k == BT_TCPSEQ_FIRST) ++r.first;
                        if (k == BT_TCPSEQ_IN_ORDER) ++r.in_order;
                        if (k == BT_TCPSEQ_GAP) ++r.gap;
                        if (k == BT_TCPSEQ_OLD) { ++r.old; o &= ~(1ull << b); }
                        if (k == BT_TCPSEQ_OVERLAP) ++r.overlap;
                    }
                }
            }
            if (out->cls) out->cls[i] = (uint8_t)k;
            if (out->off) out->off[i] = u;
        }
        if (out->out_select) out->out_select[w] = o;
    }
    *out->result = r;
}

// All launches, asynchronous on `stream`; a.n > 0, *a.result zero in stream order before them (the
// caller's memset). ev: nullptr, or five timing events recorded by the kernels' own dispatches: the
// start of the classification, of the sort, of the scan and of the emit, and the end of the last
// kernel.
int launch_flowtcpseq(const FlowtcpseqArgs& a, void* stream, void* const* ev = nullptr);

}  // namespace bt
