// bt_flowmark.h — the per-flow mark side table and the selection built from it (bt_flowmark.hip),
// shared with the host runtime (bt_flow_mark_update_device / _host, bt_flow_mark_select_device /
// _host in bt_flowmark_host.cpp): the argument checks and the two passes on the host. The host
// part is plain C++ with no device and no runtime state: tools/flowmark_host_check.cpp runs it
// under the host sanitizers.
#pragma once

#include <stdint.h>
#include <cstddef>
#include <cstdio>

#include "beatrice_gpu.h"
#include "bt_flowtab.h"
#include "bt_flowtcp.h"

namespace bt {

static_assert(sizeof(bt_flow_mark_rec) == 32 && alignof(bt_flow_mark_rec) == 8 && sizeof(bt_flow_mark_update) == 24 &&
              sizeof(bt_flow_mark_result) == 32 && sizeof(bt_flow_mark_select_opts) == 16 && sizeof(bt_flow_mark_select_result) == 32,
              "mark side table ABI layout");
static_assert(offsetof(bt_flow_mark_rec, hit_packets) == 4 && offsetof(bt_flow_mark_rec, hit_bytes) == 8 &&
              offsetof(bt_flow_mark_rec, first_hit_ts_c) == 16 && offsetof(bt_flow_mark_rec, last_hit_ts) == 24, "bt_flow_mark_rec layout");

struct FlowmarkArgs : FrameSrc {  // only desc / stride / n / ntiles are used: no frame byte is read
    uint32_t nchunks;             // ceil(ntiles / kFtChunkTiles)
    uint32_t flow_cap;
    uint32_t mark;                // != 0
    const uint32_t* flow_id;      // n entries
    const uint64_t* hit;          // ntiles words, or nullptr: every packet
    const uint64_t* ts;           // n entries, or nullptr: batch_ts
    uint64_t batch_ts;
    bt_flow_mark_rec* table;      // flow_cap records
    bt_flow_mark_result* result;  // zero when the kernel starts: every block adds its sums
};

struct FlowmarkSelArgs {
    uint32_t n, ntiles, nchunks;  // nchunks = ceil(ntiles / kFtChunkTiles)
    uint32_t flow_cap;
    uint32_t mask, all_bits, op;
    const uint32_t* flow_id;      // n entries
    const bt_flow_mark_rec* table;
    const uint64_t* base;         // ntiles words, or nullptr with BT_FLOW_MARK_SET; may be `out`
    uint64_t* out;                // ntiles words
    bt_flow_mark_select_result* result;   // zero when the kernel starts
};

// The checks that the device and the host form of the update share.
inline bool flowmark_common_args(const uint32_t* flow_id, uint32_t n, const uint64_t* hit, const bt_flow_mark_update* upd,
                                 const bt_flow_mark_rec* table, uint32_t flow_cap, const bt_flow_mark_result* result, char* why,
                                 size_t cap) {
    const auto no = [&](const char* s) { snprintf(why, cap, "%s", s); return false; };
    if (n && !flow_id) return no("null flow_id");
    if (!upd) return no("null upd");
    if (flow_cap && !table) return no("null mark_table with flow_cap != 0");
    if (!result) return no("null result");
    if (reinterpret_cast<uintptr_t>(table) & 7u) return no("mark_table is not 8-byte aligned");
    if (reinterpret_cast<uintptr_t>(flow_id) & 3u) return no("flow_id is not 4-byte aligned");
    if (reinterpret_cast<uintptr_t>(hit) & 7u) return no("hit is not 8-byte aligned");
    if (reinterpret_cast<uintptr_t>(upd->ts) & 7u) return no("ts is not 8-byte aligned");
    if (reinterpret_cast<uintptr_t>(result) & 7u) return no("result is not 8-byte aligned");
    if (!upd->mark) return no("mark is 0");
    if (upd->reserved) return no("reserved is not 0");
    return true;
}

// The checks of bt_flow_mark_update_device on everything but the context, and the launch's arguments.
inline bool flowmark_args(const bt_batch* frames, const uint32_t* flow_id, const uint64_t* hit, const bt_flow_mark_update* upd,
                          bt_flow_mark_rec* table, uint32_t flow_cap, bt_flow_mark_result* result, FlowmarkArgs* a, char* why,
                          size_t cap) {
    const auto no = [&](const char* s) { snprintf(why, cap, "%s", s); return false; };
    if (!frames) return no("null frames");
    if (!flowmark_common_args(flow_id, frames->n, hit, upd, table, flow_cap, result, why, cap)) return false;
    if (frames->flags & (BT_BATCH_PREFIXES | BT_BATCH_LEAN))
        return no("a BT_BATCH_PREFIXES / BT_BATCH_LEAN batch holds no whole frames to measure");
    *a = FlowmarkArgs{};
    if (frame_src(frames, a, why, cap)) return false;
    a->nchunks = (a->ntiles + kFtChunkTiles - 1u) / kFtChunkTiles;
    a->flow_cap = flow_cap;
    a->mark = upd->mark;
    a->flow_id = flow_id;
    a->hit = hit;
    a->ts = upd->ts;
    a->batch_ts = upd->batch_ts;
    a->table = table;
    a->result = result;
    return true;
}

// The checks of bt_flow_mark_update_host.
inline bool flowmark_host_args(const bt_pkt_desc* desc, uint32_t n, const uint32_t* flow_id, const uint64_t* hit,
                               const bt_flow_mark_update* upd, const bt_flow_mark_rec* table, uint32_t flow_cap,
                               const bt_flow_mark_result* result, char* why, size_t cap) {
    if (n && !desc) { snprintf(why, cap, "null desc"); return false; }
    return flowmark_common_args(flow_id, n, hit, upd, table, flow_cap, result, why, cap);
}

// The checks of bt_flow_mark_select_device / _host on everything but the context, and the launch's arguments.
inline bool flowmark_sel_args(const uint32_t* flow_id, uint32_t n, const bt_flow_mark_rec* table, uint32_t flow_cap,
                              const bt_flow_mark_select_opts* opts, const uint64_t* base, uint64_t* out,
                              bt_flow_mark_select_result* result, FlowmarkSelArgs* a, char* why, size_t cap) {
    const auto no = [&](const char* s) { snprintf(why, cap, "%s", s); return false; };
    if (!opts) return no("null opts");
    if (!opts->mask) return no("mask is 0");
    if (opts->flags & ~BT_FLOW_MARK_ALL_BITS) return no("unknown flag bits");
    if (opts->op > BT_FLOW_MARK_ANDNOT) return no("unknown op");
    if (opts->reserved) return no("reserved is not 0");
    if (n && !flow_id) return no("null flow_id");
    if (n && !out) return no("null out_select");
    if (flow_cap && !table) return no("null mark_table with flow_cap != 0");
    if (!result) return no("null result");
    if (reinterpret_cast<uintptr_t>(flow_id) & 3u) return no("flow_id is not 4-byte aligned");
    if (reinterpret_cast<uintptr_t>(table) & 7u) return no("mark_table is not 8-byte aligned");
    if (reinterpret_cast<uintptr_t>(base) & 7u) return no("base is not 8-byte aligned");
    if (reinterpret_cast<uintptr_t>(out) & 7u) return no("out_select is not 8-byte aligned");
    if (reinterpret_cast<uintptr_t>(result) & 7u) return no("result is not 8-byte aligned");
    if (n && opts->op != BT_FLOW_MARK_SET && !base) return no("this op needs base");
    *a = FlowmarkSelArgs{};
    a->n = n;
    a->ntiles = (uint32_t)(((uint64_t)n + 63u) / 64u);
    a->nchunks = (a->ntiles + kFtChunkTiles - 1u) / kFtChunkTiles;
    a->flow_cap = flow_cap;
    a->mask = opts->mask;
    a->all_bits = (opts->flags & BT_FLOW_MARK_ALL_BITS) ? 1u : 0u;
    a->op = opts->op;
    a->flow_id = flow_id;
    a->table = table;
    a->base = opts->op == BT_FLOW_MARK_SET ? nullptr : base;
    a->out = out;
    a->result = result;
    return true;
}

// bt_flow_mark_update_host's work once its arguments are checked: packets in ascending order.
inline void flowmark_host(const bt_pkt_desc* desc, uint32_t n, const uint32_t* flow_id, const uint64_t* hit,
                          const bt_flow_mark_update* upd, bt_flow_mark_rec* table, uint32_t flow_cap, bt_flow_mark_result* result) {
    bt_flow_mark_result r{};
    r.n = n;
    for (uint32_t i = 0; i < n; ++i) {
        if (hit && !((hit[i >> 6] >> (i & 63u)) & 1u)) continue;
        ++r.hit_packets;
        const uint32_t id = flow_id[i];
        if (id >= flow_cap) {
            if (flowtcp_is_sentinel(id)) ++r.unkeyed_hits;
            else ++r.bad_ids;
            continue;
        }
        const uint32_t len = BT_DESC_LEN(desc[i]);   // 16 bits: at most 65535
        const uint64_t t = upd->ts ? upd->ts[i] : upd->batch_ts;
        bt_flow_mark_rec& m = table[id];
        if ((m.marks & upd->mark) != upd->mark) {
            // the first hit of the call on a flow that lacked a bit: later hits find every bit set
            ++r.new_marked_flows;
            m.marks |= upd->mark;
        }
        m.hit_packets += 1u;
        m.hit_bytes += len;
        if (~t > m.first_hit_ts_c) m.first_hit_ts_c = ~t;
        if (t > m.last_hit_ts) m.last_hit_ts = t;
        ++r.marked_packets;
    }
    *result = r;
}

// bt_flow_mark_select_host's work once its arguments are checked: word by word, so base may be out.
inline void flowmark_sel_host(const FlowmarkSelArgs& a) {
    bt_flow_mark_select_result r{};
    r.n = a.n;
    for (uint32_t w = 0; w < a.ntiles; ++w) {
        const uint32_t left = a.n - w * 64u, cnt = left < 64u ? left : 64u;
        uint64_t m = 0;
        for (uint32_t b = 0; b < cnt; ++b) {
            const uint32_t id = a.flow_id[w * 64u + b];
            if (id >= a.flow_cap) {
                if (!flowtcp_is_sentinel(id)) ++r.bad_ids;
                continue;
            }
            const uint32_t got = a.table[id].marks & a.mask;
            if (a.all_bits ? got == a.mask : got != 0u) m |= 1ull << b;
        }
        const uint64_t valid = cnt == 64u ? ~0ull : (1ull << cnt) - 1ull;
        const uint64_t bw = a.base ? a.base[w] : 0ull;
        const uint64_t o = (a.op == BT_FLOW_MARK_SET ? m : a.op == BT_FLOW_MARK_AND ? (bw & m) : a.op == BT_FLOW_MARK_OR ? (bw | m) : (bw & ~m)) & valid;
        a.out[w] = o;
        r.n_marked += (uint32_t)__builtin_popcountll(m);
        r.n_out += (uint32_t)__builtin_popcountll(o);
    }
    *a.result = r;
}

// Asynchronous on `stream`; a.n > 0, *a.result zero in stream order before it (the caller's memset).
int launch_flowmark(const FlowmarkArgs& a, void* stream, void* timing_start = nullptr, void* timing_stop = nullptr);
int launch_flowmark_select(const FlowmarkSelArgs& a, void* stream, void* timing_start = nullptr, void* timing_stop = nullptr);

}  // namespace bt
