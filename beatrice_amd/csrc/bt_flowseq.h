// bt_flowseq.h — the per-flow sequence side table and the per-flow cut-off (bt_flowseq.hip),
// shared with the host runtime (bt_flow_seq_device / bt_flow_seq_host in bt_flowseq_host.cpp):
// the layout of the caller's scratch, the argument checks and the pass on the host. The host part
// is plain C++ with no device and no runtime state: tools/flowseq_host_check.cpp runs it under the
// host sanitizers.
#pragma once

#include <stdint.h>
#include <cstddef>
#include <cstdio>
#include <unordered_set>

#include "beatrice_gpu.h"
#include "bt_flowtab.h"
#include "bt_flowtcp.h"

namespace bt {

static_assert(sizeof(bt_flow_seq_rec) == 16 && alignof(bt_flow_seq_rec) == 8 && sizeof(bt_flow_seq_opts) == 32 &&
              sizeof(bt_flow_seq_out) == 24 && sizeof(bt_flow_seq_result) == 64, "sequence side table ABI layout");
static_assert(offsetof(bt_flow_seq_result, numbered_bytes) == 32 && offsetof(bt_flow_seq_result, kept_bytes) == 40,
              "bt_flow_seq_result layout");

// The sorted list is cut into units of 32 tiles (2,048 pairs), one wave each; a chunk is 8 units,
// one block, as the packets' chunks (kFtChunkTiles tiles, kFtWaves waves).
constexpr uint32_t kFsDigitBits = 8;
constexpr uint32_t kFsDigits = 1u << kFsDigitBits;
constexpr uint32_t kFsUnitTiles = kFtChunkTiles / kFtWaves;
constexpr uint32_t kFsUnit = kFsUnitTiles * 64u;
constexpr uint32_t kFsChunk = kFtChunkTiles * 64u;
constexpr uint32_t kFsJoinThreads = 1024;

struct alignas(8) FsPair { uint32_t key, idx; };           // a numbered packet: its flow number and its index
struct FsHead { uint32_t m, pad[63]; };          // scratch: the numbered packets of the call
struct FsPart {                                  // scratch, one per chunk of packets
    uint32_t count, rel;                         // numbered packets of the chunk; of the chunks before it
    uint32_t wcount[kFtWaves];                   // ... of wave w's tiles
    uint32_t pad[6];
};
struct FsCarry { uint64_t bytes; uint32_t cnt, head; };   // scratch, one per unit: the sums since its last head
static_assert(sizeof(FsPair) == 8 && sizeof(FsHead) == 256 && sizeof(FsPart) == 64 && sizeof(FsCarry) == 16, "flowseq scratch layout");

struct FsLayout { uint64_t head, numw, parts, a, b, dcnt, drel, dwcnt, dstart, lens, carry, total; };   // byte offsets

// The sort's passes: ceil(bits(flow_cap - 1) / 8); none when every key is 0.
inline uint32_t fs_passes(uint32_t flow_cap) {
    if (flow_cap <= 1u) return 0u;
    const uint32_t bits = 32u - (uint32_t)__builtin_clz(flow_cap - 1u);
    return (bits + kFsDigitBits - 1u) / kFsDigitBits;
}

inline FsLayout fs_layout(uint32_t n, uint32_t flow_cap) {
    const uint64_t ntiles = ((uint64_t)n + 63u) / 64u, nchunks = (ntiles + kFtChunkTiles - 1u) / kFtChunkTiles;
    const bool sort = fs_passes(flow_cap) != 0u;
    FsLayout l{};
    l.head = 0;
    l.numw = l.head + sizeof(FsHead);
    l.parts = l.numw + ft_round(ntiles * 8u);
    l.a = l.parts + ft_round(nchunks * sizeof(FsPart));
    l.b = l.a + ft_round((uint64_t)n * sizeof(FsPair));
    l.dcnt = l.b + (sort ? ft_round((uint64_t)n * sizeof(FsPair)) : 0u);
    l.drel = l.dcnt + (sort ? ft_round(nchunks * kFsDigits * 4u) : 0u);
    l.dwcnt = l.drel + (sort ? ft_round(nchunks * kFsDigits * 4u) : 0u);
    l.dstart = l.dwcnt + (sort ? ft_round(nchunks * kFtWaves * kFsDigits * 4u) : 0u);
    l.lens = l.dstart + (sort ? ft_round(kFsDigits * 4u) : 0u);
    l.carry = l.lens + ft_round((uint64_t)n * 4u);
    l.total = l.carry + ft_round(nchunks * kFtWaves * sizeof(FsCarry));
    return l;
}

struct FlowseqArgs : FrameSrc {   // only desc / stride / n / ntiles are used: no frame byte is read
    uint32_t nchunks;             // ceil(ntiles / kFtChunkTiles)
    uint32_t flow_cap;
    uint32_t passes;              // fs_passes(flow_cap)
    uint32_t keep_unkeyed;
    uint64_t max_packets, max_bytes;
    const uint32_t* flow_id;      // n entries
    const uint64_t* select;       // ntiles words, or nullptr: every packet; may be out_select
    bt_flow_seq_rec* table;       // flow_cap records
    uint32_t* seq;                // optional outputs
    uint64_t* byte_off;
    uint64_t* out_select;
    bt_flow_seq_result* result;   // zero when the first kernel starts: every wave adds its sums
    FsHead* head;                 // the scratch, by fs_layout
    uint64_t* numw;
    FsPart* parts;
    FsPair *a, *b;
    uint32_t *dcnt, *drel, *dwcnt, *dstart;
    uint32_t* lens;
    FsCarry* carry;
};

// The checks that the device and the host form share.
inline bool flowseq_common_args(const uint32_t* flow_id, uint32_t n, const uint64_t* select, const bt_flow_seq_opts* opts,
                                const bt_flow_seq_rec* table, uint32_t flow_cap, const bt_flow_seq_out* out,
                                const bt_flow_seq_result* result, char* why, size_t cap) {
    const auto no = [&](const char* s) { snprintf(why, cap, "%s", s); return false; };
    if (!opts) return no("null opts");
    if (!out) return no("null out");
    if (!result) return no("null result");
    if (opts->flags & ~BT_FLOW_SEQ_KEEP_UNKEYED) return no("unknown flag bits");
    if (opts->reserved[0] || opts->reserved[1] || opts->reserved[2]) return no("reserved is not 0");
    if (n && !flow_id) return no("null flow_id");
    if (flow_cap && !table) return no("null table with flow_cap != 0");
    if (reinterpret_cast<uintptr_t>(flow_id) & 3u) return no("flow_id is not 4-byte aligned");
    if (reinterpret_cast<uintptr_t>(out->seq) & 3u) return no("seq is not 4-byte aligned");
    if (reinterpret_cast<uintptr_t>(table) & 7u) return no("table is not 8-byte aligned");
    if (reinterpret_cast<uintptr_t>(select) & 7u) return no("select is not 8-byte aligned");
    if (reinterpret_cast<uintptr_t>(out->byte_off) & 7u) return no("byte_off is not 8-byte aligned");
    if (reinterpret_cast<uintptr_t>(out->out_select) & 7u) return no("out_select is not 8-byte aligned");
    if (reinterpret_cast<uintptr_t>(result) & 7u) return no("result is not 8-byte aligned");
    return true;
}

// The checks of bt_flow_seq_device on everything but the context, and the launches' arguments.
inline bool flowseq_args(const bt_batch* frames, const uint32_t* flow_id, const uint64_t* select, const bt_flow_seq_opts* opts,
                         bt_flow_seq_rec* table, uint32_t flow_cap, const bt_flow_seq_out* out, void* scratch, uint64_t scratch_bytes,
                         bt_flow_seq_result* result, FlowseqArgs* a, char* why, size_t cap) {
    const auto no = [&](const char* s) { snprintf(why, cap, "%s", s); return false; };
    if (!frames) return no("null frames");
    if (!flowseq_common_args(flow_id, frames->n, select, opts, table, flow_cap, out, result, why, cap)) return false;
    if (reinterpret_cast<uintptr_t>(scratch) & 255u) return no("scratch is not 256-byte aligned");
    if (frames->flags & (BT_BATCH_PREFIXES | BT_BATCH_LEAN))
        return no("a BT_BATCH_PREFIXES / BT_BATCH_LEAN batch holds no whole frames to measure");
    *a = FlowseqArgs{};
    if (frame_src(frames, a, why, cap)) return false;
    const FsLayout l = fs_layout(a->n, flow_cap);
    if (a->n && !scratch) return no("null scratch");
    if (a->n && scratch_bytes < l.total) {
        snprintf(why, cap, "scratch_bytes %llu below the need %llu", (unsigned long long)scratch_bytes, (unsigned long long)l.total);
        return false;
    }
    a->nchunks = (a->ntiles + kFtChunkTiles - 1u) / kFtChunkTiles;
    a->flow_cap = flow_cap;
    a->passes = fs_passes(flow_cap);
    a->keep_unkeyed = (opts->flags & BT_FLOW_SEQ_KEEP_UNKEYED) ? 1u : 0u;
    a->max_packets = opts->max_packets;
    a->max_bytes = opts->max_bytes;
    a->flow_id = flow_id;
    a->select = select;
    a->table = table;
    a->seq = out->seq;
    a->byte_off = out->byte_off;
    a->out_select = out->out_select;
    a->result = result;
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
    a->lens = reinterpret_cast<uint32_t*>(s + l.lens);
    a->carry = reinterpret_cast<FsCarry*>(s + l.carry);
    return true;
}

// The checks of bt_flow_seq_host.
inline bool flowseq_host_args(const bt_pkt_desc* desc, uint32_t n, const uint32_t* flow_id, const uint64_t* select,
                              const bt_flow_seq_opts* opts, const bt_flow_seq_rec* table, uint32_t flow_cap,
                              const bt_flow_seq_out* out, const bt_flow_seq_result* result, char* why, size_t cap) {
    if (!flowseq_common_args(flow_id, n, select, opts, table, flow_cap, out, result, why, cap)) return false;
    if (n && !desc) { snprintf(why, cap, "null desc"); return false; }
    return true;
}

// bt_flow_seq_host's work once its arguments are checked: packets in ascending order, a select
// word read before its out_select word is written, so the two may be one.
inline void flowseq_host(const bt_pkt_desc* desc, uint32_t n, const uint32_t* flow_id, const uint64_t* select,
                         const bt_flow_seq_opts* opts, bt_flow_seq_rec* table, uint32_t flow_cap, const bt_flow_seq_out* out,
                         bt_flow_seq_result* result) {
    bt_flow_seq_result r{};
    r.n = n;
    std::unordered_set<uint32_t> seen;   // the flows numbered so far in this call
    const uint32_t nwords = (uint32_t)(((uint64_t)n + 63u) / 64u);
    for (uint32_t w = 0; w < nwords; ++w) {
        const uint32_t left = n - w * 64u, cnt = left < 64u ? left : 64u;
        const uint64_t sw = select ? select[w] : ~0ull;
        uint64_t o = 0;
        for (uint32_t b = 0; b < cnt; ++b) {
            const uint32_t i = w * 64u + b;
            uint32_t seq = BT_FLOW_SEQ_NONE;
            uint64_t boff = BT_FLOW_SEQ_OFF_NONE;
            if ((sw >> b) & 1ull) {
                ++r.selected;
                const uint32_t id = flow_id[i];
                if (id >= flow_cap) {
                    if (flowtcp_is_sentinel(id)) {
                        ++r.unkeyed;
                        if (opts->flags & BT_FLOW_SEQ_KEEP_UNKEYED) { o |= 1ull << b; ++r.kept; }
                    } else {
                        ++r.bad_ids;
                    }
                } else {
                    const uint32_t len = BT_DESC_LEN(desc[i]);   // 16 bits: at most 65535
                    bt_flow_seq_rec& rec = table[id];
                    const uint64_t pk = rec.packets, by = rec.bytes;
                    seq = pk < BT_FLOW_SEQ_MAX ? (uint32_t)pk : BT_FLOW_SEQ_MAX;
                    boff = by;
                    if (seen.insert(id).second) {   // the flow's first numbered packet of the call
                        ++r.flows;
                        if (pk == 0u) ++r.new_flows;
                    }
                    if ((!opts->max_packets || pk < opts->max_packets) && (!opts->max_bytes || by < opts->max_bytes)) {
                        o |= 1ull << b;
                        ++r.kept;
                        r.kept_bytes += len;
                    }
                    rec.packets = pk + 1u;
                    rec.bytes = by + len;
                    ++r.numbered;
                    r.numbered_bytes += len;
                }
            }
            if (out->seq) out->seq[i] = seq;
            if (out->byte_off) out->byte_off[i] = boff;
        }
        if (out->out_select) out->out_select[w] = o;
    }
    *result = r;
}

// All launches, asynchronous on `stream`; a.n > 0, *a.result zero in stream order before them (the
// caller's memset). ev: nullptr, or five timing events recorded by the kernels' own dispatches: the
// start of the compaction, of the sort, of the scan and of the emit, and the end of the last kernel.
int launch_flowseq(const FlowseqArgs& a, void* stream, void* const* ev = nullptr);

// The sort alone, for another primitive that orders (key, index) pairs (bt_flowstream.hip): the
// same kernels, launched from here so that there is one copy of them. Of `a` only nchunks, head,
// parts, a, b, dcnt, drel, dwcnt and dstart are used.
//   launch_flowseq_join  the exclusive scan of parts[c].count into parts[c].rel and head->m;
//   launch_flowseq_sort  `passes` stable passes of 8 bits over the head->m pairs at a.a, low digit
//                        first; *sorted = where they end up (a.a or a.b). e_start: nullptr, or a
//                        timing event recorded at the start of the first pass's first kernel.
void launch_flowseq_join(const FlowseqArgs& a, void* stream);
void launch_flowseq_sort(const FlowseqArgs& a, uint32_t passes, void* stream, void* e_start, const FsPair** sorted);

}  // namespace bt
