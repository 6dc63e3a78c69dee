// bt_flowfollow.h — per-flow TCP reassembly with the delivered bytes exported (bt_flowfollow.hip),
// shared with the host runtime (bt_flow_follow_device / bt_flow_follow_host in
// bt_flowfollow_host.cpp): the layout of the caller's scratch, the argument checks and the pass on
// the host. Everything of the reassembly itself is bt_flowreasm.h's. The host part is plain C++
// with no device and no runtime state: tools/flowfollow_host_check.cpp runs it under the host
// sanitizers.
#pragma once

#include "bt_flowreasm.h"

namespace bt {

static_assert(sizeof(bt_flow_follow_run) == 32 && sizeof(bt_flow_follow_result) == 32 && sizeof(bt_flow_follow_out) == 64 &&
              offsetof(bt_flow_follow_run, at) == 8 && offsetof(bt_flow_follow_run, len) == 24 &&
              offsetof(bt_flow_follow_result, n_runs) == 16 && offsetof(bt_flow_follow_out, place) == 32 &&
              offsetof(bt_flow_follow_out, result) == 40, "follow ABI layout");

struct FfCarry { uint64_t bytes; uint32_t heads, pad; };   // scratch, one per unit: its delivered bytes and run heads, then what precedes it
struct FfHead { uint64_t total; uint32_t n_runs, pad; };   // scratch: the call's totals, for the runs' lengths
static_assert(sizeof(FfCarry) == 16 && sizeof(FfHead) == 16, "flowfollow scratch layout");

// The reassembly's scratch, then per sorted pair its output offset (one more: the total) and its
// source offset, per run its output offset, per unit a carry, and the totals.
struct FfLayout { FrLayout fr; uint64_t at, src, runat, carry, head, total; };

inline FfLayout ff_layout(uint32_t n, uint32_t flow_cap) {
    const uint64_t ntiles = ((uint64_t)n + 63u) / 64u, nchunks = (ntiles + kFtChunkTiles - 1u) / kFtChunkTiles;
    FfLayout l{};
    l.fr = fr_layout(n, flow_cap);
    l.at = l.fr.total;
    l.src = l.at + ft_round(((uint64_t)n + 1u) * 8u);
    l.runat = l.src + ft_round((uint64_t)n * 8u);
    l.carry = l.runat + ft_round((uint64_t)n * 8u);
    l.head = l.carry + ft_round(nchunks * kFtWaves * sizeof(FfCarry));
    l.total = l.head + ft_round(sizeof(FfHead));
    return l;
}

struct FlowfollowArgs : FrameSrc {   // bytes = the batch's own, exact: a byte at or past it reads as zero
    uint32_t nchunks;
    const FsHead* head;           // the reassembly's: m, the pairs of the sorted list
    const FsPair* s;              // the sorted list (launch_flowreasm_front's)
    const FstMeta* meta;          // as Emit left it: the final start and delivered length
    const uint32_t* pred;         // kFstNone at a stream's head, kFrCut behind a hole
    const FrSeg* seg;             // per sorted pair: rel
    const bt_flow_reasm_rec* table;   // have and next, as the call found them
    uint64_t *at, *src, *runat;   // the scratch, by ff_layout
    FfCarry* carry;
    FfHead* fhead;
    uint8_t* out;
    uint64_t cap;
    bt_flow_follow_run* runs;
    uint32_t run_cap;
    uint64_t* place;
    bt_flow_follow_result* result;
};

// What bt_flow_follow_* check on fo and the pattern's presence; base / bytes: the frames' buffer.
inline bool flowfollow_out_args(const bt_flow_follow_out* fo, const void* base, uint64_t bytes, const void* pattern, uint32_t pattern_bytes,
                                char* why, size_t cap) {
    const auto no = [&](const char* s) { snprintf(why, cap, "%s", s); return false; };
    if (!fo) return no("null fo");
    if (!fo->result) return no("null fo->result");
    if (!fo->bytes && fo->cap) return no("null bytes with cap != 0");
    if (!fo->runs && fo->run_cap) return no("null runs with run_cap != 0");
    if (reinterpret_cast<uintptr_t>(fo->runs) & 7u) return no("runs is not 8-byte aligned");
    if (reinterpret_cast<uintptr_t>(fo->place) & 7u) return no("place is not 8-byte aligned");
    if (reinterpret_cast<uintptr_t>(fo->result) & 7u) return no("fo->result is not 8-byte aligned");
    if (fo->reserved0 || fo->reserved[0] || fo->reserved[1]) return no("fo's reserved is not 0");
    if (fo->cap && base && bytes) {
        const uintptr_t o0 = reinterpret_cast<uintptr_t>(fo->bytes), b0 = reinterpret_cast<uintptr_t>(base);
        if (o0 < b0 + bytes && b0 < o0 + fo->cap) return no("bytes overlaps the frames' buffer");
    }
    if (pattern && !pattern_bytes) return no("a pattern with pattern_bytes == 0");
    if (!pattern && pattern_bytes) return no("pattern_bytes != 0 without a pattern");
    return true;
}

// The checks of bt_flow_follow_device on everything but the context, and the launches' arguments.
inline int flowfollow_args(const bt_batch* frames, const uint32_t* flow_id, const uint64_t* select, const int64_t* off,
                           uint32_t table_flags, const void* pattern, const void* pattern_device, uint32_t pattern_bytes,
                           bt_flow_reasm_rec* table, uint32_t flow_cap, void* scratch, uint64_t scratch_bytes,
                           const bt_flow_reasm_out* out, const bt_flow_follow_out* fo, FlowreasmArgs* a, FlowfollowArgs* f, char* why,
                           size_t cap) {
    const auto no = [&](const char* s) { snprintf(why, cap, "%s", s); return (int)BT_E_INVALID_ARGUMENT; };
    const bool with = pattern || pattern_device;
    if (with && !pattern) return no("null pattern with a pattern_device");
    if (with && !pattern_device) return no("null pattern_device with a pattern");
    // the reassembly's own checks, against the part of the scratch that is its own
    const FfLayout l = ff_layout(frames ? frames->n : 0u, flow_cap);
    if (const int rc = flowreasm_args(frames, flow_id, select, off, table_flags, pattern, pattern_device, pattern_bytes, table, flow_cap,
                                      scratch, scratch_bytes < l.fr.total ? scratch_bytes : l.fr.total, out, a, why, cap, with))
        return rc;
    if (!flowfollow_out_args(fo, frames->base, frames->bytes, pattern, pattern_bytes, why, cap)) return BT_E_INVALID_ARGUMENT;
    if (a->n && scratch_bytes < l.total) {
        snprintf(why, cap, "scratch_bytes %llu below the need %llu", (unsigned long long)scratch_bytes, (unsigned long long)l.total);
        return BT_E_INVALID_ARGUMENT;
    }
    *f = FlowfollowArgs{};
    if (frame_src(frames, f, why, cap)) return BT_E_INVALID_ARGUMENT;
    uint8_t* const s = static_cast<uint8_t*>(scratch);
    f->nchunks = a->nchunks;
    f->head = a->head;
    f->meta = a->meta;
    f->pred = a->pred;
    f->seg = a->seg;
    f->table = table;
    f->at = reinterpret_cast<uint64_t*>(s + l.at);
    f->src = reinterpret_cast<uint64_t*>(s + l.src);
    f->runat = reinterpret_cast<uint64_t*>(s + l.runat);
    f->carry = reinterpret_cast<FfCarry*>(s + l.carry);
    f->fhead = reinterpret_cast<FfHead*>(s + l.head);
    f->out = fo->bytes;
    f->cap = fo->cap;
    f->runs = fo->runs;
    f->run_cap = fo->run_cap;
    f->place = fo->place;
    f->result = fo->result;
    return BT_OK;
}

// The checks of bt_flow_follow_host. *with: a pattern was given.
inline int flowfollow_host_args(const uint8_t* base, uint64_t bytes, const bt_pkt_desc* desc, uint32_t n, const uint32_t* flow_id,
                                const uint64_t* select, const int64_t* off, uint32_t table_flags, const void* pattern,
                                uint32_t pattern_bytes, const bt_flow_reasm_rec* table, uint32_t flow_cap, const bt_flow_reasm_out* out,
                                const bt_flow_follow_out* fo, FstPattern* pat, bool* with, char* why, size_t cap) {
    if (!flowreasm_common_args(flow_id, n, select, off, table_flags, table, flow_cap, out, why, cap)) return BT_E_INVALID_ARGUMENT;
    if (n && (!base || !desc)) { snprintf(why, cap, "null base / desc"); return BT_E_INVALID_ARGUMENT; }
    if (!flowfollow_out_args(fo, base, bytes, pattern, pattern_bytes, why, cap)) return BT_E_INVALID_ARGUMENT;
    *with = pattern != nullptr;
    *pat = FstPattern{};
    return *with ? flowstream_pattern(pattern, pattern_bytes, pat, why, cap) : (int)BT_OK;
}

// bt_flow_follow_host's work once its arguments are checked: the definition. flowreasm_host's two
// parts (the same numbers into the table, hit, rest and *out->result), and in the second part,
// which carries have and next as the call found them, the export: a run head where g starts a key
// or s.rel > hi, and the bytes base[at0 + k] for k in [from, len) appended. pattern == nullptr:
// no byte is matched and every state is 0.
inline void flowfollow_host(const uint8_t* base, uint64_t bytes, const bt_pkt_desc* desc, uint32_t n, const uint32_t* flow_id,
                            const uint64_t* select, const int64_t* off, uint32_t table_flags, const void* pattern, const FstPattern& pat,
                            bt_flow_reasm_rec* table, uint32_t flow_cap, const bt_flow_reasm_out* out, const bt_flow_follow_out* fo) {
    struct Seg { uint32_t key, rel, idx, start, len; };
    bt_flow_reasm_result r{};
    bt_flow_follow_result fr{};
    r.n = n;
    const uint8_t* const tab = pattern ? static_cast<const uint8_t*>(pattern) + kFstBlobHeader : nullptr;
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
    if (fo->place) for (uint32_t i = 0; i < n; ++i) fo->place[i] = UINT64_MAX;
    std::stable_sort(segs.begin(), segs.end(), [](const Seg& p, const Seg& q) { return p.key != q.key ? p.key < q.key : p.rel < q.rel; });
    std::unordered_set<uint32_t> hit_flows;   // the flows with a hit so far in this call
    uint64_t run_at = 0;                      // where the open run began
    for (size_t g = 0; g < segs.size();) {
        const uint32_t key = segs[g].key, id = key >> 1;
        const size_t g0 = g;
        bt_flow_reasm_dir& d = table[id].d[key & 1u];
        uint64_t D = d.have && pattern ? d.d : 0ull;
        uint32_t hi = d.have ? 0u : segs[g].rel;
        const int64_t pbase = d.have ? d.next : kFrNewBase;
        for (; g < segs.size() && segs[g].key == key; ++g) {
            const Seg& s = segs[g];
            const uint32_t end = s.rel + s.len;
            if (s.rel > hi) {
                ++d.holes; ++r.holes;
                d.hole_bytes += s.rel - hi;
                D = 0;
            }
            if (g == g0 || s.rel > hi) {   // a run head: it delivers (end > rel >= hi)
                if (fr.n_runs) {
                    if (fr.n_runs - 1u < fo->run_cap) fo->runs[fr.n_runs - 1u].len = fr.total - run_at;
                }
                run_at = fr.total;
                if (fr.n_runs < fo->run_cap) {
                    bt_flow_follow_run& u = fo->runs[fr.n_runs];
                    u.flow = id;
                    u.flags = (key & 1u) | (d.have ? 0u : BT_FOLLOW_NEW) | (s.rel > hi ? BT_FOLLOW_HOLE : 0u);
                    u.at = fr.total;
                    u.pos = (int64_t)((uint64_t)pbase + s.rel);   // max(rel, hi) = rel at a head
                    u.len = 0;
                }
                ++fr.n_runs;
            }
            if (end <= hi) {
                ++d.dup_packets; ++r.dup_packets;
                d.dup_bytes += s.len;
                continue;
            }
            const uint32_t from = s.rel > hi ? 0u : hi - s.rel;   // the bytes of its front that were delivered before
            d.dup_bytes += from;
            const uint64_t at0 = BT_DESC_OFF(desc[s.idx]) + s.start;
            if (fo->place) fo->place[s.idx] = fr.total;
            uint64_t H = 0;
            for (uint32_t k = from; k < s.len; ++k) {
                const uint64_t at = at0 + k;
                const uint8_t c = at < bytes ? base[at] : 0u;
                if (fr.total < fo->cap) fo->bytes[fr.total] = c;
                ++fr.total;
                if (!pattern) continue;
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
    if (fr.n_runs && fr.n_runs - 1u < fo->run_cap) fo->runs[fr.n_runs - 1u].len = fr.total - run_at;
    fr.written = fr.total < fo->cap ? fr.total : fo->cap;
    fr.runs_written = fr.n_runs < fo->run_cap ? fr.n_runs : fo->run_cap;
    if (out->hit) for (uint32_t w = 0; w < nwords; ++w) out->hit[w] = hw[w];
    *out->result = r;
    *fo->result = fr;
}

// The follow's launches between launch_flowreasm_front and launch_flowreasm_commit, asynchronous
// on `stream`; f.n > 0, f.s set, f.place full of UINT64_MAX in stream order before them. e_sum /
// e_copy: nullptr, or timing events recorded by the first launch's and the copy's own dispatches.
int launch_flowfollow(const FlowfollowArgs& f, void* stream, void* e_sum, void* e_copy);

}  // namespace bt
