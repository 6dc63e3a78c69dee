// bt_flowreasm.h — per-flow TCP reassembly: a payload pattern matched in sequence order
// (bt_flowreasm.hip), shared with the host runtime (bt_flow_reasm_device / bt_flow_reasm_host in
// bt_flowreasm_host.cpp): where a segment lands in its direction's window, the layout of the
// caller's scratch, the argument checks and the pass on the host. The host part is plain C++ with
// no device and no runtime state: tools/flowreasm_host_check.cpp runs it under the host sanitizers.
#pragma once

#include <stdint.h>
#include <algorithm>
#include <cstddef>
#include <cstdio>
#include <cstring>
#include <unordered_set>
#include <vector>

#include "beatrice_gpu.h"
#include "beatrice_gpu_bench.h"
#include "bt_fanout.h"
#include "bt_flowseq.h"
#include "bt_flowstream.h"

#if defined(__HIPCC__)
#define BT_FR_HD __host__ __device__
#else
#define BT_FR_HD
#endif

namespace bt {

static_assert(sizeof(bt_flow_reasm_dir) == 64 && sizeof(bt_flow_reasm_rec) == 128 && alignof(bt_flow_reasm_rec) == 8 &&
              sizeof(bt_flow_reasm_out) == 40 && sizeof(bt_flow_reasm_result) == 64, "reassembly side table ABI layout");
static_assert(offsetof(bt_flow_reasm_dir, next) == 8 && offsetof(bt_flow_reasm_dir, have) == 16 &&
              offsetof(bt_flow_reasm_dir, dup_bytes) == 40 && offsetof(bt_flow_reasm_dir, late_bytes) == 56 &&
              offsetof(bt_flow_reasm_result, stream_bytes) == 48, "bt_flow_reasm_dir / _result layout");

constexpr int64_t kFrNewBase = -(1ll << 30);       // the window's base of a direction without `have`
constexpr int64_t kFrRelMax = 0x7FFE0000ll;        // rel above this is far; rel + plen stays below 2^31
constexpr uint32_t kFrCut = 0xFFFFFFFEu;           // pred[]: a hole precedes the packet (kFstNone: its stream's head)

// Where one segment lands in its direction's window: the rules 1. - 4. of include/beatrice_gpu.h.
struct FrPlace {
    uint32_t what;         // kFrTake, kFrLate or kFrFar
    uint32_t trim;         // bytes cut off its front against next
    uint32_t rel;          // with kFrTake: the trimmed start less the base
};
enum { kFrTake = 0, kFrLate = 1, kFrFar = 2 };

BT_FR_HD inline FrPlace flowreasm_place(int64_t off, uint32_t syn, uint32_t plen, uint32_t have, int64_t next) {
    FrPlace x{kFrTake, 0u, 0u};
    const int64_t ds = (int64_t)((uint64_t)off + syn), de = (int64_t)((uint64_t)ds + plen);
    int64_t from = ds;
    if (have) {
        if (de <= next) { x.what = kFrLate; return x; }
        if (ds < next) { x.trim = (uint32_t)((uint64_t)next - (uint64_t)ds); from = next; }   // below plen
    }
    const int64_t rel = (int64_t)((uint64_t)from - (uint64_t)(have ? next : kFrNewBase));
    if (rel < 0 || rel > kFrRelMax) { x.what = kFrFar; x.trim = 0u; return x; }
    x.rel = (uint32_t)rel;
    return x;
}

struct FrSeg { uint32_t rel, len; };                 // scratch, per sorted pair: the window position and the length before step 6
struct FrCarry { uint32_t m, idx, head, any; };      // scratch, one per unit: the leftmost maximum of rel + len since its last head
static_assert(sizeof(FrSeg) == 8 && sizeof(FrCarry) == 16, "flowreasm scratch layout");

struct FrLayout { uint64_t head, numw, hitw, parts, a, b, dcnt, drel, dwcnt, dstart, meta, rel, pred, dfin, seg, carry, bits, bits_bytes, total; };

inline FrLayout fr_layout(uint32_t n, uint32_t flow_cap) {
    const uint64_t ntiles = ((uint64_t)n + 63u) / 64u, nchunks = (ntiles + kFtChunkTiles - 1u) / kFtChunkTiles;
    FrLayout l{};
    l.head = 0;
    l.numw = l.head + sizeof(FsHead);
    l.hitw = l.numw + ft_round(ntiles * 8u);
    l.parts = l.hitw + ft_round(ntiles * 8u);
    l.a = l.parts + ft_round(nchunks * sizeof(FsPart));
    l.b = l.a + ft_round((uint64_t)n * sizeof(FsPair));
    l.dcnt = l.b + ft_round((uint64_t)n * sizeof(FsPair));
    l.drel = l.dcnt + ft_round(nchunks * kFsDigits * 4u);
    l.dwcnt = l.drel + ft_round(nchunks * kFsDigits * 4u);
    l.dstart = l.dwcnt + ft_round(nchunks * kFtWaves * kFsDigits * 4u);
    l.meta = l.dstart + ft_round(kFsDigits * 4u);
    l.rel = l.meta + ft_round((uint64_t)n * sizeof(FstMeta));
    l.pred = l.rel + ft_round((uint64_t)n * 4u);
    l.dfin = l.pred + ft_round((uint64_t)n * 4u);
    l.seg = l.dfin + ft_round((uint64_t)n * 8u);
    l.carry = l.seg + ft_round((uint64_t)n * sizeof(FrSeg));
    l.bits = l.carry + ft_round(nchunks * kFtWaves * sizeof(FrCarry));
    l.bits_bytes = ((uint64_t)flow_cap + 63u) / 64u * 8u;   // one bit per flow: "a hit of this call was seen"
    l.total = l.bits + ft_round(l.bits_bytes);
    return l;
}

struct FlowreasmArgs : FrameSrc {   // bytes = fan_read_end, as FlowstatArgs
    uint32_t nchunks;             // ceil(ntiles / kFtChunkTiles)
    uint32_t l3_only, bidir;      // as the table that numbered the flows
    uint32_t flow_cap;
    uint32_t passes;              // fst_passes(flow_cap): the second sort's
    FstPattern pat;
    const uint8_t* blob;          // the device copy of the pattern
    const uint32_t* flow_id;      // n entries
    const uint64_t* select;       // ntiles words, or nullptr: every packet; may be hit or rest
    const int64_t* off;           // n entries
    bt_flow_reasm_rec* table;     // flow_cap records
    uint64_t *hit, *rest;         // ntiles words each, or nullptr
    bt_flow_reasm_result* result; // zero when the first kernel starts
    FsHead* head;                 // the scratch, by fr_layout
    uint64_t *numw, *hitw;
    FsPart* parts;
    FsPair *a, *b;
    uint32_t *dcnt, *drel, *dwcnt, *dstart;
    FstMeta* meta;
    uint32_t *rel, *pred;
    uint64_t* dfin;
    FrSeg* seg;
    FrCarry* carry;
    uint64_t* bits;               // zero when the first kernel starts (the caller's memset)
    uint64_t bits_bytes;
};

// The checks that the device and the host form share; the pattern comes after them.
inline bool flowreasm_common_args(const uint32_t* flow_id, uint32_t n, const uint64_t* select, const int64_t* off, uint32_t table_flags,
                                  const bt_flow_reasm_rec* table, uint32_t flow_cap, const bt_flow_reasm_out* out, char* why,
                                  size_t cap) {
    const auto no = [&](const char* s) { snprintf(why, cap, "%s", s); return false; };
    if (!out) return no("null out");
    if (!out->result) return no("null result");
    if (n && !flow_id) return no("null flow_id");
    if (n && !off) return no("null off");
    if (flow_cap && !table) return no("null table with flow_cap != 0");
    if (reinterpret_cast<uintptr_t>(flow_id) & 3u) return no("flow_id is not 4-byte aligned");
    if (reinterpret_cast<uintptr_t>(table) & 7u) return no("table is not 8-byte aligned");
    if (reinterpret_cast<uintptr_t>(select) & 7u) return no("select is not 8-byte aligned");
    if (reinterpret_cast<uintptr_t>(off) & 7u) return no("off is not 8-byte aligned");
    if (reinterpret_cast<uintptr_t>(out->hit) & 7u) return no("hit is not 8-byte aligned");
    if (reinterpret_cast<uintptr_t>(out->rest) & 7u) return no("rest is not 8-byte aligned");
    if (reinterpret_cast<uintptr_t>(out->result) & 7u) return no("result is not 8-byte aligned");
    if (out->hit && out->hit == out->rest) return no("hit and rest are one");
    if (table_flags & ~kTcpFlagsKnown) return no("unknown flag bits");
    if (out->reserved[0] || out->reserved[1]) return no("reserved is not 0");
    if (flow_cap > kFstFlowCapMax) return no("flow_cap above 2^31");
    return true;
}

// The checks of bt_flow_reasm_device on everything but the context, and the launches' arguments.
// BT_OK, or the error code with the reason in why.
inline int flowreasm_args(const bt_batch* frames, const uint32_t* flow_id, const uint64_t* select, const int64_t* off,
                          uint32_t table_flags, const void* pattern, const void* pattern_device, uint32_t pattern_bytes,
                          bt_flow_reasm_rec* table, uint32_t flow_cap, void* scratch, uint64_t scratch_bytes,
                          const bt_flow_reasm_out* out, FlowreasmArgs* a, char* why, size_t cap, bool need_pattern = true) {
    const auto no = [&](const char* s) { snprintf(why, cap, "%s", s); return (int)BT_E_INVALID_ARGUMENT; };
    if (!frames) return no("null frames");
    if (!flowreasm_common_args(flow_id, frames->n, select, off, table_flags, table, flow_cap, out, why, cap)) return BT_E_INVALID_ARGUMENT;
    if (need_pattern && !pattern_device) return no("null pattern_device");
    if (reinterpret_cast<uintptr_t>(pattern_device) & 7u) return no("pattern_device is not 8-byte aligned");
    if (reinterpret_cast<uintptr_t>(scratch) & 255u) return no("scratch is not 256-byte aligned");
    if (frames->flags & (BT_BATCH_PREFIXES | BT_BATCH_LEAN))
        return no("a BT_BATCH_PREFIXES / BT_BATCH_LEAN batch holds no whole frames to walk");
    *a = FlowreasmArgs{};
    if (frame_src(frames, a, why, cap)) return BT_E_INVALID_ARGUMENT;
    const int prc = need_pattern ? flowstream_pattern(pattern, pattern_bytes, &a->pat, why, cap) : (int)BT_OK;   // without: bt_flow_follow_device's plain follow
    if (prc) return prc;
    const FrLayout l = fr_layout(a->n, flow_cap);
    if (a->n && !scratch) return no("null scratch");
    if (a->n && scratch_bytes < l.total) {
        snprintf(why, cap, "scratch_bytes %llu below the need %llu", (unsigned long long)scratch_bytes, (unsigned long long)l.total);
        return BT_E_INVALID_ARGUMENT;
    }
    a->bytes = fan_read_end(a->base, a->bytes);
    a->nchunks = (a->ntiles + kFtChunkTiles - 1u) / kFtChunkTiles;
    a->l3_only = (table_flags & BT_FLOWTAB_L3_ONLY) ? 1u : 0u;
    a->bidir = (table_flags & BT_FLOWTAB_BIDIRECTIONAL) ? 1u : 0u;
    a->flow_cap = flow_cap;
    a->passes = fst_passes(flow_cap);
    a->blob = static_cast<const uint8_t*>(pattern_device);
    a->flow_id = flow_id;
    a->select = select;
    a->off = off;
    a->table = table;
    a->hit = out->hit;
    a->rest = out->rest;
    a->result = out->result;
    uint8_t* const s = static_cast<uint8_t*>(scratch);
    a->head = reinterpret_cast<FsHead*>(s + l.head);
    a->numw = reinterpret_cast<uint64_t*>(s + l.numw);
    a->hitw = reinterpret_cast<uint64_t*>(s + l.hitw);
    a->parts = reinterpret_cast<FsPart*>(s + l.parts);
    a->a = reinterpret_cast<FsPair*>(s + l.a);
    a->b = reinterpret_cast<FsPair*>(s + l.b);
    a->dcnt = reinterpret_cast<uint32_t*>(s + l.dcnt);
    a->drel = reinterpret_cast<uint32_t*>(s + l.drel);
    a->dwcnt = reinterpret_cast<uint32_t*>(s + l.dwcnt);
    a->dstart = reinterpret_cast<uint32_t*>(s + l.dstart);
    a->meta = reinterpret_cast<FstMeta*>(s + l.meta);
    a->rel = reinterpret_cast<uint32_t*>(s + l.rel);
    a->pred = reinterpret_cast<uint32_t*>(s + l.pred);
    a->dfin = reinterpret_cast<uint64_t*>(s + l.dfin);
    a->seg = reinterpret_cast<FrSeg*>(s + l.seg);
    a->carry = reinterpret_cast<FrCarry*>(s + l.carry);
    a->bits = reinterpret_cast<uint64_t*>(s + l.bits);
    a->bits_bytes = l.bits_bytes;
    return BT_OK;
}

// The checks of bt_flow_reasm_host.
inline int flowreasm_host_args(const uint8_t* base, const bt_pkt_desc* desc, uint32_t n, const uint32_t* flow_id, const uint64_t* select,
                               const int64_t* off, uint32_t table_flags, const void* pattern, uint32_t pattern_bytes,
                               const bt_flow_reasm_rec* table, uint32_t flow_cap, const bt_flow_reasm_out* out, FstPattern* pat,
                               char* why, size_t cap) {
    if (!flowreasm_common_args(flow_id, n, select, off, table_flags, table, flow_cap, out, why, cap)) return BT_E_INVALID_ARGUMENT;
    if (n && (!base || !desc)) { snprintf(why, cap, "null base / desc"); return BT_E_INVALID_ARGUMENT; }
    return flowstream_pattern(pattern, pattern_bytes, pat, why, cap);
}

// What one frame contributes, before its flow: flowstream_frame_host's facts for a TCP segment
// (plen == 0 for anything else) and its SYN bit.
inline FlowstreamFacts flowreasm_frame_host(const uint8_t* f, uint32_t len, uint32_t table_flags, uint32_t* syn) {
    FlowstreamFacts x = flowstream_frame_host(f, len, table_flags);
    *syn = 0u;
    if (!x.l4) return x;
    const FlowLayersHost L = flow_layers_host(f, len);
    if (L.proto != 6u) { x.plen = 0u; return x; }
    *syn = (f[L.o4 + 13u] & BT_TCPF_SYN) ? 1u : 0u;
    return x;
}

// bt_flow_reasm_host's work once its arguments are checked: the definition. First every packet in
// ascending order against its record as the call found it (a select word is read before its rest
// word is written), then every (flow, direction) in turn over its segments in (rel, index) order;
// the hit words last, so hit may be select as well.
inline void flowreasm_host(const uint8_t* base, uint64_t bytes, const bt_pkt_desc* desc, uint32_t n, const uint32_t* flow_id,
                           const uint64_t* select, const int64_t* off, uint32_t table_flags, const void* pattern, const FstPattern& pat,
                           bt_flow_reasm_rec* table, uint32_t flow_cap, const bt_flow_reasm_out* out) {
    struct Seg { uint32_t key, rel, idx, start, len; };
    bt_flow_reasm_result r{};
    r.n = n;
    const uint8_t* const tab = static_cast<const uint8_t*>(pattern) + kFstBlobHeader;
    const uint32_t eb = pat.W / 8u;
    const uint32_t nwords = (uint32_t)(((uint64_t)n + 63u) / 64u);
    std::vector<Seg> segs;
    std::vector<uint64_t> hw(nwords, 0ull);
    for (uint32_t w = 0; w < nwords; ++w) {
        const uint32_t left = n - w * 64u, cnt = left < 64u ? left : 64u;
        const uint64_t sw = select ? select[w] : ~0ull;
        uint64_t rw = 0;
        for (uint32_t b = 0; b < cnt; ++b) {
            if (!((sw >> b) & 1ull)) continue;
            const uint32_t i = w * 64u + b;
            ++r.selected;
            if (off[i] == BT_TCPSEQ_OFF_NONE) rw |= 1ull << b;
            const uint32_t id = flow_id[i];
            if (id >= flow_cap) {
                if (flowtcp_is_sentinel(id)) ++r.unkeyed; else ++r.bad_ids;
                continue;
            }
            if (off[i] == BT_TCPSEQ_OFF_NONE) continue;
            const uint64_t foff = BT_DESC_OFF(desc[i]);
            const uint32_t len = BT_DESC_LEN(desc[i]);
            uint8_t head[128] = {0};   // the walk and the header fields lie below offset 22 + 60 + 20
            for (uint32_t k = 0; k < 128u && k < len && foff + k < bytes; ++k) head[k] = base[foff + k];
            uint32_t syn;
            const FlowstreamFacts x = flowreasm_frame_host(head, len, table_flags, &syn);
            if (!x.plen) continue;
            bt_flow_reasm_dir& d = table[id].d[x.dir];   // have and next: unchanged until the second part
            const FrPlace at = flowreasm_place(off[i], syn, x.plen, d.have, d.next);
            if (at.what == kFrLate) { ++d.late_packets; d.late_bytes += x.plen; ++r.late_packets; continue; }
            if (at.what == kFrFar) { ++r.far_packets; continue; }
            d.dup_bytes += at.trim;
            segs.push_back(Seg{id << 1 | x.dir, at.rel, i, x.start + at.trim, x.plen - at.trim});
        }
        if (out->rest) out->rest[w] = rw;
    }
    std::stable_sort(segs.begin(), segs.end(), [](const Seg& p, const Seg& q) { return p.key != q.key ? p.key < q.key : p.rel < q.rel; });
    std::unordered_set<uint32_t> hit_flows;   // the flows with a hit so far in this call
    for (size_t g = 0; g < segs.size();) {
        const uint32_t key = segs[g].key, id = key >> 1;
        bt_flow_reasm_dir& d = table[id].d[key & 1u];
        uint64_t D = d.have ? d.d : 0ull;
        uint32_t hi = d.have ? 0u : segs[g].rel;
        for (; g < segs.size() && segs[g].key == key; ++g) {
            const Seg& s = segs[g];
            const uint32_t end = s.rel + s.len;
            if (s.rel > hi) {
                ++d.holes; ++r.holes;
                d.hole_bytes += s.rel - hi;
                D = 0;
            }
            if (end <= hi) {
                ++d.dup_packets; ++r.dup_packets;
                d.dup_bytes += s.len;
                continue;
            }
            const uint32_t from = s.rel > hi ? 0u : hi - s.rel;   // the bytes of its front that were delivered before
            d.dup_bytes += from;
            const uint64_t at0 = BT_DESC_OFF(desc[s.idx]) + s.start;
            uint64_t H = 0;
            for (uint32_t k = from; k < s.len; ++k) {
                const uint64_t at = at0 + k;
                const uint8_t c = at < bytes ? base[at] : 0u;
                uint64_t e = 0;
                memcpy(&e, tab + (size_t)c * eb, eb);
                D = flowstream_step(pat, D, e);
                H |= D & pat.F;
            }
            ++d.stream_packets; ++r.stream_packets;
            r.stream_bytes += s.len - from;
            if (H) {
                if (hit_flows.insert(id).second && !table[id].d[0].hit_packets && !table[id].d[1].hit_packets) ++r.new_hit_flows;
                ++d.hit_packets; ++r.hit_packets;
                hw[s.idx >> 6] |= 1ull << (s.idx & 63u);
            }
            hi = end;
        }
        d.next = (int64_t)((uint64_t)(d.have ? d.next : kFrNewBase) + hi);
        d.have = 1u;
        d.d = D;
    }
    if (out->hit) for (uint32_t w = 0; w < nwords; ++w) out->hit[w] = hw[w];
    *out->result = r;
}

// All launches, asynchronous on `stream`; a.n > 0, *a.result and a.bits zero in stream order before
// them (the caller's memsets). ev: nullptr, or seven timing events recorded by the kernels' own
// dispatches: the start of the classification, of the first sort, of the second sort, of the scan,
// of the match and of the commit, and the end of the last kernel.
int launch_flowreasm(const FlowreasmArgs& a, void* stream, void* const* ev = nullptr);

// The same launches in three stages, for a caller that puts launches of its own between them
// (bt_flowfollow.hip, which reads have and next before Commit rewrites them): the classification up
// to Emit (ev[0 .. 3]; *sorted: the sorted pair list the later stages walk), the match (its start:
// e4), Commit (its start and end: e5, e6). A caller that skips the match zeroes what only it writes
// (hitw, dfin, the hit words) in stream order before Commit.
int launch_flowreasm_front(const FlowreasmArgs& a, void* stream, void* const* ev, const FsPair** sorted);
int launch_flowreasm_match(const FlowreasmArgs& a, void* stream, void* e4);
int launch_flowreasm_commit(const FlowreasmArgs& a, const FsPair* sorted, void* stream, void* e5, void* e6);

}  // namespace bt
