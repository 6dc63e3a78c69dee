// bt_flowstream.h — per-flow stream matching (bt_flowstream.hip), shared with the host runtime
// (bt_flow_stream_device / bt_flow_stream_host / bt_flow_stream_compile in bt_flowstream_host.cpp):
// the predicate on a pattern blob, the layout of the caller's scratch, the argument checks, what
// one frame contributes and the pass on the host. The host part is plain C++ with no device and no
// runtime state: tools/flowstream_host_check.cpp runs it under the host sanitizers.
#pragma once

#include <stdint.h>
#include <cstddef>
#include <cstdio>
#include <cstring>
#include <unordered_set>
#include <vector>

#include "beatrice_gpu.h"
#include "beatrice_gpu_bench.h"
#include "bt_fanout.h"
#include "bt_flowseq.h"

namespace bt {

static_assert(sizeof(bt_flow_stream_rec) == 32 && alignof(bt_flow_stream_rec) == 8 && sizeof(bt_flow_stream_info) == 16 &&
              sizeof(bt_flow_stream_out) == 32 && sizeof(bt_flow_stream_result) == 64, "stream side table ABI layout");
static_assert(offsetof(bt_flow_stream_rec, hit_packets) == 16 && offsetof(bt_flow_stream_rec, stream_packets) == 24 &&
              offsetof(bt_flow_stream_result, stream_bytes) == 24 && offsetof(bt_flow_stream_result, new_hit_flows) == 32,
              "bt_flow_stream_rec / _result layout");

constexpr uint32_t kFstPiece = 128;          // CH: the own bytes of one lane of the match
constexpr uint32_t kFstTailMax = 63;         // T <= W - 1
constexpr uint32_t kFstBlobHeader = 80;      // bt_regex_dfa.cpp's bit-parallel blob: the table starts here
constexpr uint32_t kFstNone = 0xFFFFFFFFu;   // pred[]: the first contributing packet of its stream in the batch
constexpr uint32_t kFstFlowCapMax = 0x80000000u;   // the sort key is flow << 1 | dir

// A pattern the matcher takes, read from its blob: the masks of the general Shift-And step with
// S == 0, NF == ~0 and no anchored start.
struct FstPattern {
    uint32_t W, P, T, R;       // entry width in bits, positions, tail = P - 1 (0 for P == 0), closure steps
    uint64_t Iall, A, F;
};

// The one predicate of compile, device form and host form: BT_OK and *p filled, or
// BT_E_NOT_IMPLEMENTED / BT_E_INVALID_ARGUMENT with the reason (the construct by name) in why.
inline int flowstream_pattern(const void* blob, uint32_t bytes, FstPattern* p, char* why, size_t cap) {
    const auto no = [&](int rc, const char* s) { snprintf(why, cap, "%s", s); return rc; };
    if (!blob) return no(BT_E_INVALID_ARGUMENT, "null pattern");
    if (bytes < kFstBlobHeader) return no(BT_E_INVALID_ARGUMENT, "pattern_bytes below a blob's header");
    const uint8_t* b = static_cast<const uint8_t*>(blob);
    uint16_t magic, w;
    uint32_t flags;
    uint64_t m[7];
    memcpy(&magic, b, 2);
    memcpy(&w, b + 2, 2);
    memcpy(&flags, b + 8, 4);
    memcpy(m, b + 16, sizeof(m));
    if (magic != 0xFFFFu)
        return no(BT_E_NOT_IMPLEMENTED, "the pattern needs a DFA (a repeated group, or more than 64 positions): unbounded memory");
    if (b[6] == 2) return no(BT_E_NOT_IMPLEMENTED, "the pattern matches the empty string: always true");
    if (b[6] != 1) return no(BT_E_NOT_IMPLEMENTED, "the pattern can never match");
    if (flags & 1u) return no(BT_E_NOT_IMPLEMENTED, "a repeatable position (+, * or {n,}): unbounded memory");
    if (flags & 6u) return no(BT_E_NOT_IMPLEMENTED, "a ^ anchor: a stream has no line start");
    if (flags & 8u) return no(BT_E_NOT_IMPLEMENTED, "a $ anchor: a stream has no end");
    if (flags) return no(BT_E_NOT_IMPLEMENTED, "unknown blob flags");
    if (w != 8u && w != 16u && w != 32u && w != 64u) return no(BT_E_INVALID_ARGUMENT, "a blob width that is not 8, 16, 32 or 64");
    if (bytes < kFstBlobHeader + 256u * (w / 8u)) return no(BT_E_INVALID_ARGUMENT, "pattern_bytes below the blob's table");
    if (m[1] || m[2] || m[6] || m[4] != ~0ull) return no(BT_E_INVALID_ARGUMENT, "a blob whose masks contradict its flags");
    uint64_t any = 0;
    for (uint32_t c = 0; c < 256u; ++c) {
        uint64_t e = 0;
        memcpy(&e, b + kFstBlobHeader + (size_t)c * (w / 8u), w / 8u);
        any |= e;
    }
    p->W = w;
    p->P = any ? 64u - (uint32_t)__builtin_clzll(any) : 0u;
    p->T = p->P ? p->P - 1u : 0u;
    p->R = b[7];
    p->Iall = m[0];
    p->A = m[3];
    p->F = m[5];
    return BT_OK;
}

// bt_flow_stream_compile's work: bt_payload_dfa_compile_ex(expression, 0) held to the predicate.
inline int flowstream_compile(const char* expression, void* blob, uint32_t cap, uint32_t* size, bt_flow_stream_info* info, char* why,
                              size_t wcap) {
    const auto no = [&](int rc, const char* s) { snprintf(why, wcap, "%s", s); return rc; };
    if (!expression || !size) return no(BT_E_INVALID_ARGUMENT, "null expression / size");
    uint32_t need = 0;
    int rc = bt_payload_dfa_compile_ex(expression, 0, nullptr, 0, &need);
    if (rc == BT_E_NOT_IMPLEMENTED)
        return no(rc, "a construct outside the GPU subset (\\b, \\B, a back-reference, a look-ahead or too many states)");
    if (rc) return no(rc, "not a regular expression std::regex accepts");
    std::vector<uint8_t> tmp(need);
    rc = bt_payload_dfa_compile_ex(expression, 0, tmp.data(), need, &need);
    if (rc) return no(rc, "the pattern did not compile");
    FstPattern p;
    rc = flowstream_pattern(tmp.data(), need, &p, why, wcap);
    if (rc) return rc;
    *size = need;
    if (info) *info = bt_flow_stream_info{p.W, p.P, p.T, p.R};
    if (!blob) return BT_OK;
    if (cap < need) return no(BT_E_RESOURCE, "cap below the blob's size");
    memcpy(blob, tmp.data(), need);
    return BT_OK;
}

// One byte of the stream: the general bit-parallel step of bt_payload_walk.h with S == 0, NF == ~0.
inline uint64_t flowstream_step(const FstPattern& p, uint64_t D, uint64_t b) {
    uint64_t n = ((D << 1) | p.Iall) & b;
    for (uint32_t k = 0; k < p.R; ++k) n |= (n << 1) & p.A;
    return n;
}

inline uint32_t fst_passes(uint32_t flow_cap) {   // fs_passes(2 * flow_cap), in 32 bits up to flow_cap = 2^31
    if (!flow_cap) return 0u;
    const uint32_t bits = (flow_cap > 1u ? 32u - (uint32_t)__builtin_clz(flow_cap - 1u) : 0u) + 1u;
    return (bits + kFsDigitBits - 1u) / kFsDigitBits;
}

struct FstMeta { uint32_t start, len_dir; };   // scratch, per packet: payload offset in the frame; length | dir << 31
struct FstLayout { uint64_t head, numw, hitw, parts, a, b, dcnt, drel, dwcnt, dstart, meta, pred, dfin, bits, bits_bytes, total; };

inline FstLayout fst_layout(uint32_t n, uint32_t flow_cap) {
    const uint64_t ntiles = ((uint64_t)n + 63u) / 64u, nchunks = (ntiles + kFtChunkTiles - 1u) / kFtChunkTiles;
    FstLayout l{};
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
    l.pred = l.meta + ft_round((uint64_t)n * sizeof(FstMeta));
    l.dfin = l.pred + ft_round((uint64_t)n * 4u);
    l.bits = l.dfin + ft_round((uint64_t)n * 8u);
    l.bits_bytes = ((uint64_t)flow_cap + 63u) / 64u * 8u;   // one bit per flow: "a hit of this call was seen"
    l.total = l.bits + ft_round(l.bits_bytes);
    return l;
}

struct FlowstreamArgs : FrameSrc {   // bytes = fan_read_end, as FlowstatArgs
    uint32_t nchunks;             // ceil(ntiles / kFtChunkTiles)
    uint32_t l3_only, bidir;      // as the table that numbered the flows
    uint32_t flow_cap;
    uint32_t passes;              // fst_passes(flow_cap)
    FstPattern pat;
    const uint8_t* blob;          // the device copy of the pattern
    const uint32_t* flow_id;      // n entries
    const uint64_t* select;       // ntiles words, or nullptr: every packet; may be hit
    bt_flow_stream_rec* table;    // flow_cap records
    uint64_t* hit;                // ntiles words, or nullptr
    bt_flow_stream_result* result;   // zero when the first kernel starts
    FsHead* head;                 // the scratch, by fst_layout
    uint64_t *numw, *hitw;
    FsPart* parts;
    FsPair *a, *b;
    uint32_t *dcnt, *drel, *dwcnt, *dstart;
    FstMeta* meta;
    uint32_t* pred;
    uint64_t* dfin;
    uint64_t* bits;               // zero when the first kernel starts (the caller's memset)
    uint64_t bits_bytes;
};

// The checks that the device and the host form share; the pattern comes after them.
inline bool flowstream_common_args(const uint32_t* flow_id, uint32_t n, const uint64_t* select, uint32_t table_flags,
                                   const bt_flow_stream_rec* table, uint32_t flow_cap, const bt_flow_stream_out* out, char* why,
                                   size_t cap) {
    const auto no = [&](const char* s) { snprintf(why, cap, "%s", s); return false; };
    if (!out) return no("null out");
    if (!out->result) return no("null result");
    if (n && !flow_id) return no("null flow_id");
    if (flow_cap && !table) return no("null table with flow_cap != 0");
    if (reinterpret_cast<uintptr_t>(flow_id) & 3u) return no("flow_id is not 4-byte aligned");
    if (reinterpret_cast<uintptr_t>(table) & 7u) return no("table is not 8-byte aligned");
    if (reinterpret_cast<uintptr_t>(select) & 7u) return no("select is not 8-byte aligned");
    if (reinterpret_cast<uintptr_t>(out->hit) & 7u) return no("hit is not 8-byte aligned");
    if (reinterpret_cast<uintptr_t>(out->result) & 7u) return no("result is not 8-byte aligned");
    if (table_flags & ~kTcpFlagsKnown) return no("unknown flag bits");
    if (out->reserved[0] || out->reserved[1]) return no("reserved is not 0");
    if (flow_cap > kFstFlowCapMax) return no("flow_cap above 2^31");
    return true;
}

// The checks of bt_flow_stream_device on everything but the context, and the launches' arguments.
// BT_OK, or the error code with the reason in why.
inline int flowstream_args(const bt_batch* frames, const uint32_t* flow_id, const uint64_t* select, uint32_t table_flags,
                           const void* pattern, const void* pattern_device, uint32_t pattern_bytes, bt_flow_stream_rec* table,
                           uint32_t flow_cap, void* scratch, uint64_t scratch_bytes, const bt_flow_stream_out* out, FlowstreamArgs* a,
                           char* why, size_t cap) {
    const auto no = [&](const char* s) { snprintf(why, cap, "%s", s); return (int)BT_E_INVALID_ARGUMENT; };
    if (!frames) return no("null frames");
    if (!flowstream_common_args(flow_id, frames->n, select, table_flags, table, flow_cap, out, why, cap)) return BT_E_INVALID_ARGUMENT;
    if (!pattern_device) return no("null pattern_device");
    if (reinterpret_cast<uintptr_t>(pattern_device) & 7u) return no("pattern_device is not 8-byte aligned");
    if (reinterpret_cast<uintptr_t>(scratch) & 255u) return no("scratch is not 256-byte aligned");
    if (frames->flags & (BT_BATCH_PREFIXES | BT_BATCH_LEAN))
        return no("a BT_BATCH_PREFIXES / BT_BATCH_LEAN batch holds no whole frames to walk");
    *a = FlowstreamArgs{};
    if (frame_src(frames, a, why, cap)) return BT_E_INVALID_ARGUMENT;
    const int prc = flowstream_pattern(pattern, pattern_bytes, &a->pat, why, cap);
    if (prc) return prc;
    const FstLayout l = fst_layout(a->n, flow_cap);
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
    a->table = table;
    a->hit = out->hit;
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
    a->pred = reinterpret_cast<uint32_t*>(s + l.pred);
    a->dfin = reinterpret_cast<uint64_t*>(s + l.dfin);
    a->bits = reinterpret_cast<uint64_t*>(s + l.bits);
    a->bits_bytes = l.bits_bytes;
    return BT_OK;
}

// The checks of bt_flow_stream_host.
inline int flowstream_host_args(const uint8_t* base, const bt_pkt_desc* desc, uint32_t n, const uint32_t* flow_id,
                                const uint64_t* select, uint32_t table_flags, const void* pattern, uint32_t pattern_bytes,
                                const bt_flow_stream_rec* table, uint32_t flow_cap, const bt_flow_stream_out* out, FstPattern* pat,
                                char* why, size_t cap) {
    if (!flowstream_common_args(flow_id, n, select, table_flags, table, flow_cap, out, why, cap)) return BT_E_INVALID_ARGUMENT;
    if (n && (!base || !desc)) { snprintf(why, cap, "null base / desc"); return BT_E_INVALID_ARGUMENT; }
    return flowstream_pattern(pattern, pattern_bytes, pat, why, cap);
}

// What one frame contributes, before its flow: frame[0 .. len) with the bytes of its first 128
// in f (zeros where the frame has none).
struct FlowstreamFacts {
    bool l4;                  // a whole TCP / UDP header under the key's rule
    uint32_t dir;             // the TCP side table's direction under table_flags
    uint32_t start, plen;     // the payload's offset in the frame and its length; 0 without l4
};

inline FlowstreamFacts flowstream_frame_host(const uint8_t* f, uint32_t len, uint32_t table_flags) {
    FlowstreamFacts x{};
    const FlowLayersHost L = flow_layers_host(f, len);
    if (!(L.v4 || L.v6) || !L.l4) return x;
    x.l4 = true;
    const uint8_t* ip = f + L.o3;
    const uint8_t* l4 = f + L.o4;
    const uint32_t hdr = L.proto == 6u ? 4u * (l4[12] >> 4) : 8u;
    const uint32_t end3 = L.o3 + (L.v4 ? ((uint32_t)ip[2] << 8 | ip[3]) : 40u + ((uint32_t)ip[4] << 8 | ip[5]));
    const uint32_t end = len < end3 ? len : end3;
    x.start = L.o4 + hdr;
    x.plen = end > x.start ? end - x.start : 0u;
    if (table_flags & BT_FLOWTAB_BIDIRECTIONAL) {
        uint8_t key[kFanInputMax] = {0};
        uint32_t klass = BT_FLOW_NONE;
        const uint32_t nb = flow_key_host(f, len, (table_flags & BT_FLOWTAB_L3_ONLY) != 0, key, &klass);
        x.dir = ft_canonical(key, nb);
    }
    return x;
}

// bt_flow_stream_host's work once its arguments are checked: packets in ascending order, every
// stream's state carried in its record; a select word is read before its hit word is written, so
// the two may be one.
inline void flowstream_host(const uint8_t* base, uint64_t bytes, const bt_pkt_desc* desc, uint32_t n, const uint32_t* flow_id,
                            const uint64_t* select, uint32_t table_flags, const void* pattern, const FstPattern& pat,
                            bt_flow_stream_rec* table, uint32_t flow_cap, const bt_flow_stream_out* out) {
    bt_flow_stream_result r{};
    r.n = n;
    const uint8_t* const tab = static_cast<const uint8_t*>(pattern) + kFstBlobHeader;
    const uint32_t eb = pat.W / 8u;
    std::unordered_set<uint32_t> hit_flows;   // the flows with a hit so far in this call
    const uint32_t nwords = (uint32_t)(((uint64_t)n + 63u) / 64u);
    for (uint32_t w = 0; w < nwords; ++w) {
        const uint32_t left = n - w * 64u, cnt = left < 64u ? left : 64u;
        const uint64_t sw = select ? select[w] : ~0ull;
        uint64_t hw = 0;
        for (uint32_t b = 0; b < cnt; ++b) {
            if (!((sw >> b) & 1ull)) continue;
            const uint32_t i = w * 64u + b;
            ++r.selected;
            const uint32_t id = flow_id[i];
            if (id >= flow_cap) {
                if (flowtcp_is_sentinel(id)) ++r.unkeyed; else ++r.bad_ids;
                continue;
            }
            const uint64_t off = BT_DESC_OFF(desc[i]);
            const uint32_t len = BT_DESC_LEN(desc[i]);
            uint8_t head[128] = {0};   // the walk and the header fields lie below offset 22 + 60 + 20
            for (uint32_t k = 0; k < 128u && k < len && off + k < bytes; ++k) head[k] = base[off + k];
            const FlowstreamFacts x = flowstream_frame_host(head, len, table_flags);
            if (!x.plen) continue;
            bt_flow_stream_rec& rec = table[id];
            uint64_t D = rec.d[x.dir], H = 0;
            for (uint32_t k = 0; k < x.plen; ++k) {
                const uint64_t at = off + x.start + k;
                const uint8_t c = at < bytes ? base[at] : 0u;
                uint64_t e = 0;
                memcpy(&e, tab + (size_t)c * eb, eb);
                D = flowstream_step(pat, D, e);
                H |= D & pat.F;
            }
            rec.d[x.dir] = D;
            ++rec.stream_packets[x.dir];
            ++r.stream_packets;
            r.stream_bytes += x.plen;
            if (H) {
                if (hit_flows.insert(id).second && !rec.hit_packets[0] && !rec.hit_packets[1]) ++r.new_hit_flows;
                ++rec.hit_packets[x.dir];
                ++r.hit_packets;
                hw |= 1ull << b;
            }
        }
        if (out->hit) out->hit[w] = hw;
    }
    *out->result = r;
}

// All launches, asynchronous on `stream`; a.n > 0, *a.result and a.bits zero in stream order before
// them (the caller's memsets). ev: nullptr, or five timing events recorded by the kernels' own
// dispatches: the start of the classification, of the sort, of the match and of the commit, and the
// end of the last kernel.
int launch_flowstream(const FlowstreamArgs& a, void* stream, void* const* ev = nullptr);

}  // namespace bt
