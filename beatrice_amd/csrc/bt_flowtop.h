// bt_flowtop.h — the top-K query over a flow tracker (bt_flowtop.hip), shared with the host runtime
// (bt_flow_track_top_* in bt_flowtop_host.cpp): the value of a flow under a metric, the layout of
// the caller's scratch, the argument checks, and the query on the host over a state in host memory.
// The host part is plain C++ with no device and no runtime state: tools/flowtop_host_check.cpp
// runs it under the host sanitizers.
#pragma once

#include <stdint.h>
#include <algorithm>
#include <cstddef>
#include <cstring>
#include <vector>

#include "beatrice_gpu.h"
#include "bt_flowtrack.h"

namespace bt {

static_assert(sizeof(bt_flow_top_result) == 48 && alignof(bt_flow_top_result) == 8 && sizeof(bt_flow_top_opts) == 16 &&
              sizeof(bt_flow_top_out) == 40, "top-K ABI layout");
static_assert(offsetof(bt_flow_top_result, threshold) == 24 && offsetof(bt_flow_top_result, top_total) == 40, "bt_flow_top_result layout");

constexpr uint32_t kTopMetrics = 5;               // BT_FLOW_TOP_BYTES .. BT_FLOW_TOP_TCP_RST
constexpr uint32_t kTopDigits = 8;                // 8-bit digits of the u64 value, most significant first
constexpr uint32_t kTopBins = 256;
constexpr uint32_t kTopSortThreads = 1024;
constexpr uint32_t kTopMaxGrid = 1024;            // blocks of the grid-stride passes: what bounds the atomics on one bin
constexpr uint32_t kTopUnroll = 4;                // values a thread of a histogram pass has in flight

BT_FK_HD inline bool ftop_needs_tcp(uint32_t metric) { return metric == BT_FLOW_TOP_TCP_SYN || metric == BT_FLOW_TOP_TCP_RST; }

// The value of a flow under `metric` (< kTopMetrics); t: its side record, read for the TCP metrics only.
BT_FK_HD inline uint64_t ftop_value(uint32_t metric, const bt_flow_track_rec& r, const bt_flow_tcp_rec* t) {
    switch (metric) {
    case BT_FLOW_TOP_BYTES: return r.bytes[0] + r.bytes[1];
    case BT_FLOW_TOP_PACKETS: return r.packets[0] + r.packets[1];
    case BT_FLOW_TOP_DURATION: return r.last_ts >= r.first_ts ? r.last_ts - r.first_ts : 0ull;
    case BT_FLOW_TOP_TCP_SYN: return t->syn_packets;
    default: return t->rst_packets;
    }
}

// Scratch control block, written by bt_flowtop_begin and the picks, read by the kernels behind them.
struct FtopCtl {
    uint32_t ok, n_flows;         // the header matched; n_flows as every kernel of the call takes it
    uint32_t n_top, need;         // min(k, n_flows); flows still to take among those that match the prefix
    uint32_t ties, n_gt;          // the picked bin's count; (after the last digit) flows above the threshold
    uint64_t prefix;              // the digits found so far; after the last digit, the threshold
    uint64_t total;               // the sum of every value (every block of bt_flowtop_value adds its own)
};
static_assert(sizeof(FtopCtl) == 40, "FtopCtl layout");

struct FtopPart {                 // one per block of kFkThreads flows (bt_flowtop_count)
    uint32_t ngt, neq;            // flows above / at the threshold
    uint32_t rel_gt, rel_eq;      // ... of the blocks before it (bt_flowtop_scan)
    uint32_t wgt[kFkWaves], weq[kFkWaves];
};
static_assert(sizeof(FtopPart) == 48, "FtopPart layout");

struct FtopLayout { uint64_t ctl, hist, value, parts, cand_value, cand_id, total; };   // byte offsets into the scratch

inline FtopLayout ftop_scratch(uint32_t flow_cap, uint32_t k) {
    FtopLayout l{};
    l.ctl = 0;
    l.hist = l.ctl + ft_round(sizeof(FtopCtl));
    l.value = l.hist + ft_round((uint64_t)kTopDigits * kTopBins * 4u);
    l.parts = l.value + ft_round((uint64_t)flow_cap * 8u);
    l.cand_value = l.parts + ft_round(((uint64_t)flow_cap + kFkThreads - 1u) / kFkThreads * sizeof(FtopPart));
    l.cand_id = l.cand_value + ft_round((uint64_t)k * 8u);
    l.total = l.cand_id + ft_round((uint64_t)k * 4u);
    return l;
}

struct FlowtopArgs {              // the kernels'
    const bt_flow_track_hdr* hdr;
    const bt_flow_track_rec* recs;
    const bt_flow_tcp_rec* tcp;   // nullptr without a side table
    uint32_t flags, flow_cap, slots;   // as the state was initialised: compared with *hdr on the device
    uint32_t metric, k;
    FtopCtl* ctl;
    uint32_t* hist;               // kTopDigits histograms of kTopBins counts
    uint64_t* value;              // flow_cap values
    FtopPart* parts;
    uint64_t* cand_value;         // k candidates: the flows above the threshold in flow order, then the ties taken
    uint32_t* cand_id;
    uint32_t* top_id;
    uint64_t* top_value;
    bt_flow_track_rec* top;
    bt_flow_tcp_rec* top_tcp;
    bt_flow_top_result* result;
};

// The checks both forms share on opts, tcp and out.
inline bool flowtop_common(const bt_flow_top_opts* opts, const bt_flow_tcp_rec* tcp, const bt_flow_top_out* out, char* why, size_t cap) {
    const auto no = [&](const char* s) { snprintf(why, cap, "%s", s); return false; };
    if (!opts) return no("null opts");
    if (!out) return no("null out");
    if (!out->result) return no("null result");
    if (reinterpret_cast<uintptr_t>(out->result) & 7u) return no("result is not 8-byte aligned");
    if (reinterpret_cast<uintptr_t>(out->top_value) & 7u) return no("top_value is not 8-byte aligned");
    if (reinterpret_cast<uintptr_t>(out->top) & 7u) return no("top is not 8-byte aligned");
    if (reinterpret_cast<uintptr_t>(out->top_id) & 3u) return no("top_id is not 4-byte aligned");
    if (reinterpret_cast<uintptr_t>(tcp) & 3u) return no("tcp is not 4-byte aligned");
    if (reinterpret_cast<uintptr_t>(out->top_tcp) & 3u) return no("top_tcp is not 4-byte aligned");
    if (opts->k > BT_FLOW_TOP_MAX_K) return no("k above BT_FLOW_TOP_MAX_K");
    if (opts->metric >= kTopMetrics) return no("unknown metric");
    if (opts->reserved[0] || opts->reserved[1]) return no("non-zero reserved fields");
    if (ftop_needs_tcp(opts->metric) && !tcp) return no("a TCP metric without the side table (tcp == NULL)");
    if (out->top_tcp && !tcp) return no("top_tcp without the side table (tcp == NULL)");
    return true;
}

// The checks of bt_flow_track_top_device on everything but the context, and the kernels' arguments.
// `sh`: the state's entry, nullptr = unknown.
inline bool flowtop_args(const FkShadow* sh, const void* state, const bt_flow_top_opts* opts, const bt_flow_tcp_rec* tcp, void* scratch,
                         uint64_t scratch_bytes, const bt_flow_top_out* out, FlowtopArgs* a, char* why, size_t cap) {
    const auto no = [&](const char* s) { snprintf(why, cap, "%s", s); return false; };
    if (!state) return no("null state");
    if (reinterpret_cast<uintptr_t>(state) & 255u) return no("state is not 256-byte aligned");
    if (!scratch) return no("null scratch");
    if (reinterpret_cast<uintptr_t>(scratch) & 255u) return no("scratch is not 256-byte aligned");
    if (!flowtop_common(opts, tcp, out, why, cap)) return false;
    // last of the checks but the scratch's size, which the state's flow_cap decides
    if (!sh) return no("state is not an initialised tracker (bt_flow_track_init_device)");
    bt_flow_track_sizes sl{};
    if (!fk_layout(sh->flow_cap, sh->slots, &sl, why, cap)) return false;
    const FtopLayout l = ftop_scratch(sh->flow_cap, opts->k);
    if (scratch_bytes < l.total) {
        snprintf(why, cap, "scratch_bytes %llu below the need %llu", (unsigned long long)scratch_bytes, (unsigned long long)l.total);
        return false;
    }
    const uint8_t* const st = static_cast<const uint8_t*>(state);
    uint8_t* const s = static_cast<uint8_t*>(scratch);
    *a = FlowtopArgs{};
    a->hdr = reinterpret_cast<const bt_flow_track_hdr*>(st + sl.header);
    a->recs = reinterpret_cast<const bt_flow_track_rec*>(st + sl.records);
    a->tcp = tcp;
    a->flags = sh->flags; a->flow_cap = sh->flow_cap; a->slots = sl.slots;
    a->metric = opts->metric; a->k = opts->k;
    a->ctl = reinterpret_cast<FtopCtl*>(s + l.ctl);
    a->hist = reinterpret_cast<uint32_t*>(s + l.hist);
    a->value = reinterpret_cast<uint64_t*>(s + l.value);
    a->parts = reinterpret_cast<FtopPart*>(s + l.parts);
    a->cand_value = reinterpret_cast<uint64_t*>(s + l.cand_value);
    a->cand_id = reinterpret_cast<uint32_t*>(s + l.cand_id);
    a->top_id = out->top_id; a->top_value = out->top_value; a->top = out->top; a->top_tcp = out->top_tcp;
    a->result = out->result;
    return true;
}

// The checks of bt_flow_track_top_host; *hs: the checked state (never written through).
inline bool flowtop_host_args(const void* state, uint64_t state_bytes, const bt_flow_top_opts* opts, const bt_flow_tcp_rec* tcp,
                              const bt_flow_top_out* out, FkHostState* hs, char* why, size_t cap) {
    if (!state) { snprintf(why, cap, "%s", "null state"); return false; }
    if (reinterpret_cast<uintptr_t>(state) & 255u) { snprintf(why, cap, "%s", "state is not 256-byte aligned"); return false; }
    if (!flowtop_common(opts, tcp, out, why, cap)) return false;
    return fk_host_state(const_cast<void*>(state), state_bytes, hs, why, cap);
}

// bt_flow_track_top_host's work on a checked state and checked arguments.
inline void flowtop_host(const FkHostState& s, const bt_flow_top_opts& o, const bt_flow_tcp_rec* tcp, const bt_flow_top_out& out) {
    const uint32_t nf = s.hdr->n_flows, n_top = o.k < nf ? o.k : nf;
    bt_flow_top_result r{};
    r.n_flows = nf; r.n_top = n_top; r.metric = o.metric;
    std::vector<uint64_t> value(nf);
    std::vector<uint32_t> order(nf);
    for (uint32_t f = 0; f < nf; ++f) {
        value[f] = ftop_value(o.metric, s.recs[f], tcp ? tcp + f : nullptr);
        order[f] = f;
        r.total += value[f];
    }
    std::partial_sort(order.begin(), order.begin() + n_top, order.end(), [&](uint32_t x, uint32_t y) {
        return value[x] != value[y] ? value[x] > value[y] : x < y;
    });
    for (uint32_t k = 0; k < n_top; ++k) {
        const uint32_t f = order[k];
        if (out.top_id) out.top_id[k] = f;
        if (out.top_value) out.top_value[k] = value[f];
        if (out.top) out.top[k] = s.recs[f];
        if (out.top_tcp) out.top_tcp[k] = tcp[f];
        r.top_total += value[f];
    }
    if (n_top) {
        r.threshold = value[order[n_top - 1u]];
        for (uint32_t f = 0; f < nf; ++f) r.n_ties += value[f] == r.threshold ? 1u : 0u;
    }
    *out.result = r;
}

// Asynchronous on `stream`. timing_start / timing_stop: recorded by the first / last kernel's own dispatch.
int launch_flowtop(const FlowtopArgs& a, void* stream, void* timing_start = nullptr, void* timing_stop = nullptr);

}  // namespace bt
