// bt_timing.cpp — the bench harness (include/beatrice_gpu_bench.h): the bt_time_* entry
// points, which enqueue K launches between events and report the device's and the host's
// share of the span.
#include <algorithm>
#include <chrono>
#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <mutex>
#include <vector>

#include "bt_ctx.h"
#include "bt_flowseq.h"
#include "bt_flowtrack.h"
#include "bt_hip_util.h"

using namespace bt;

// The host side of a timed loop whose launches (K of them, each between the event pair
// c->timing.tev[2i], c->timing.tev[2i+1]) were enqueued on c->stream after c->timing.ev0 at h0, followed by
// c->timing.ev1: wait by polling, then fill the breakdown.
static int finish_timing(bt_ctx* c, uint32_t iters, bool no_kernel_events, std::chrono::steady_clock::time_point h0,
                         bt_timing* t, const char* who) {
    using clk = std::chrono::steady_clock;
    auto ms = [](clk::time_point x, clk::time_point y) { return std::chrono::duration<double, std::milli>(y - x).count(); };
    const auto h1 = clk::now();
    // Poll instead of hipEventSynchronize: a blocking wait is woken by an interrupt, whose
    // latency would sit inside the caller's timed region.
    auto poll = [](hipEvent_t e) -> hipError_t {
        for (;;) {
            const hipError_t q = hipEventQuery(e);
            if (q != hipErrorNotReady) return q;
        }
    };
    HIP_TRY(poll(c->timing.ev0));
    const auto h2 = clk::now();
    HIP_TRY(poll(c->timing.ev1));
    const auto h3 = clk::now();
    float tot = 0, k = 0, kmin = 1e30f, kmax = 0, lead = 0, gap = 0;
    HIP_TRY(hipEventElapsedTime(&tot, c->timing.ev0, c->timing.ev1));
    for (uint32_t i = 0; !no_kernel_events && i < iters; ++i) {
        float x = 0;
        HIP_TRY(hipEventElapsedTime(&x, c->timing.tev[2 * i], c->timing.tev[2 * i + 1]));
        k += x;
        kmin = std::min(kmin, x);
        kmax = std::max(kmax, x);
        if (i + 1 < iters) {
            float g = 0;
            HIP_TRY(hipEventElapsedTime(&g, c->timing.tev[2 * i + 1], c->timing.tev[2 * i + 2]));
            gap += g;
        }
    }
    if (!no_kernel_events) HIP_TRY(hipEventElapsedTime(&lead, c->timing.ev0, c->timing.tev[0]));
    const auto h4 = clk::now();
    if (t) {
        *t = bt_timing{};
        t->span_ms = tot;
        t->main_ms = no_kernel_events ? -1.0f : k / iters;
        t->main_min_ms = no_kernel_events ? -1.0f : kmin;
        t->main_max_ms = no_kernel_events ? -1.0f : kmax;
        t->lead_ms = lead;
        t->gap_ms = gap;
        t->enqueue_ms = ms(h0, h1);
        t->first_seen_ms = ms(h1, h2);
        t->last_seen_ms = ms(h2, h3);
        t->query_ms = ms(h3, h4);
        t->wall_ms = ms(h0, h4);
        t->spin_rc = c->spin_rc;
        t->device_flags = c->device_flags;
    }
    static const bool dbg = getenv("BT_DEBUG_TIMING") != nullptr;
    if (dbg)
        fprintf(stderr, "[%s] enqueue %.3f ms, first-seen %.3f ms, last-seen %.3f ms, queries %.3f ms, "
                "gpu span %.3f ms\n", who, ms(h0, h1), ms(h1, h2), ms(h2, h3), ms(h3, h4), tot);
    return BT_OK;
}

static int ensure_timing_events(bt_ctx* c, uint32_t iters) {
    while (c->timing.tev.size() < 2 * (size_t)iters) {
        hipEvent_t e;
        HIP_TRY(hipEventCreate(&e));
        c->timing.tev.push_back(e);
    }
    return BT_OK;
}

extern "C" {

int bt_time_pass_pack(bt_ctx* c, const bt_batch* b, const uint64_t* select, const bt_pack_opts* po,
                      const bt_pack_out* out, uint32_t iters, float* ms) {
    const bt::DeviceRestore keep_device;   // the caller's current device, restored on return
    if (!c || !b || !b->n || !iters || !ms) return set_error(BT_E_INVALID_ARGUMENT, "null argument / empty batch / zero iterations");
    std::lock_guard<std::mutex> lk(c->mu);
    HIP_TRY(hipSetDevice(c->device));
    if (int rc = ensure_timing_events(c, iters)) return rc;
    for (uint32_t i = 0; i < iters; ++i)
        if (int rc = run_pass_pack(c, b, select, po, out, c->stream, c->timing.tev[2 * i], c->timing.tev[2 * i + 1])) {
            (void)hipStreamSynchronize(c->stream);
            return rc;
        }
    HIP_TRY(hipStreamSynchronize(c->stream));
    for (uint32_t i = 0; i < iters; ++i) HIP_TRY(hipEventElapsedTime(&ms[i], c->timing.tev[2 * i], c->timing.tev[2 * i + 1]));
    return BT_OK;
}

int bt_time_tally(bt_ctx* c, const uint8_t* decide, uint32_t n, const bt_batch* frames, const void* records,
                  uint32_t n_cap, uint32_t flags, bt_tally* out, uint32_t iters, float* ms) {
    const bt::DeviceRestore keep_device;   // the caller's current device, restored on return
    if (!c || !n || !iters || !ms) return set_error(BT_E_INVALID_ARGUMENT, "null argument / empty batch / zero iterations");
    std::lock_guard<std::mutex> lk(c->mu);
    HIP_TRY(hipSetDevice(c->device));
    if (int rc = ensure_timing_events(c, iters)) return rc;
    for (uint32_t i = 0; i < iters; ++i)
        if (int rc = run_tally(c, decide, n, frames, records, n_cap, flags, out, c->stream, c->timing.tev[2 * i],
                               c->timing.tev[2 * i + 1])) {
            (void)hipStreamSynchronize(c->stream);
            return rc;
        }
    HIP_TRY(hipStreamSynchronize(c->stream));
    for (uint32_t i = 0; i < iters; ++i) HIP_TRY(hipEventElapsedTime(&ms[i], c->timing.tev[2 * i], c->timing.tev[2 * i + 1]));
    return BT_OK;
}

int bt_time_fanout(bt_ctx* c, const bt_batch* frames, const uint64_t* select, const bt_fanout_opts* opts,
                   const bt_fanout_out* out, uint32_t iters, float* ms) {
    const bt::DeviceRestore keep_device;   // the caller's current device, restored on return
    if (!c || !frames || !frames->n || !iters || !ms)
        return set_error(BT_E_INVALID_ARGUMENT, "null argument / empty batch / zero iterations");
    std::lock_guard<std::mutex> lk(c->mu);
    HIP_TRY(hipSetDevice(c->device));
    if (int rc = ensure_timing_events(c, iters)) return rc;
    for (uint32_t i = 0; i < iters; ++i)
        if (int rc = run_fanout(c, frames, select, opts, out, c->stream, c->timing.tev[2 * i], c->timing.tev[2 * i + 1])) {
            (void)hipStreamSynchronize(c->stream);
            return rc;
        }
    HIP_TRY(hipStreamSynchronize(c->stream));
    for (uint32_t i = 0; i < iters; ++i) HIP_TRY(hipEventElapsedTime(&ms[i], c->timing.tev[2 * i], c->timing.tev[2 * i + 1]));
    return BT_OK;
}

int bt_time_flow_table(bt_ctx* c, const bt_batch* frames, const uint64_t* select, const bt_flow_table_opts* opts, void* scratch,
                       uint64_t scratch_bytes, const bt_flow_table_out* out, uint32_t iters, float* ms) {
    const bt::DeviceRestore keep_device;   // the caller's current device, restored on return
    if (!c || !frames || !frames->n || !iters || !ms)
        return set_error(BT_E_INVALID_ARGUMENT, "null argument / empty batch / zero iterations");
    std::lock_guard<std::mutex> lk(c->mu);
    HIP_TRY(hipSetDevice(c->device));
    if (int rc = ensure_timing_events(c, iters)) return rc;
    for (uint32_t i = 0; i < iters; ++i)
        if (int rc = run_flow_table(c, frames, select, opts, scratch, scratch_bytes, out, c->stream, c->timing.tev[2 * i],
                                    c->timing.tev[2 * i + 1])) {
            (void)hipStreamSynchronize(c->stream);
            return rc;
        }
    HIP_TRY(hipStreamSynchronize(c->stream));
    for (uint32_t i = 0; i < iters; ++i) HIP_TRY(hipEventElapsedTime(&ms[i], c->timing.tev[2 * i], c->timing.tev[2 * i + 1]));
    return BT_OK;
}

// What the flow table replaces: the ordered pass list copied to pinned host memory, then
// bt_flow_table_host's group-by over the listed frames on the calling thread (a hash map is not
// split over threads without a merge; the fan-out's 16-thread bucket is the other baseline).
int bt_time_flow_table_host(bt_ctx* c, const uint32_t* pass_idx, uint32_t n_pass, const uint8_t* host_base, uint64_t host_bytes,
                            const bt_pkt_desc* host_desc, const bt_flow_table_opts* opts, uint32_t iters, float* copy_ms,
                            float* table_ms, bt_flow_table_result* last) {
    const bt::DeviceRestore keep_device;   // the caller's current device, restored on return
    if (!c || !pass_idx || !n_pass || !host_base || !host_desc || !iters || !copy_ms || !table_ms)
        return set_error(BT_E_INVALID_ARGUMENT, "null argument / empty list / zero iterations");
    char why[96];
    uint32_t slots = 0;
    if (!flowtab_opts(opts, n_pass, &slots, why, sizeof(why))) return set_error(BT_E_INVALID_ARGUMENT, "bt_time_flow_table_host: %s", why);
    std::lock_guard<std::mutex> lk(c->mu);
    HIP_TRY(hipSetDevice(c->device));
    uint32_t* h = nullptr;
    HIP_TRY(hipHostMalloc(&h, (size_t)n_pass * 4, hipHostMallocDefault));
    std::memset(h, 0, (size_t)n_pass * 4);   // first touch outside the timed part
    std::vector<bt_pkt_desc> listed(n_pass);
    std::vector<bt_flow_rec> flows(opts->flow_cap);
    bt_flow_table_result r{};
    const auto now = [] { return std::chrono::steady_clock::now(); };
    const auto ms = [](auto a, auto b) { return std::chrono::duration<float, std::milli>(b - a).count(); };
    hipError_t err = hipSuccess;
    for (uint32_t it = 0; it < iters && err == hipSuccess; ++it) {
        const auto t0 = now();
        err = hipMemcpyAsync(h, pass_idx, (size_t)n_pass * 4, hipMemcpyDeviceToHost, c->stream);
        if (err == hipSuccess) err = hipStreamSynchronize(c->stream);
        const auto t1 = now();
        for (uint32_t j = 0; j < n_pass; ++j) listed[j] = host_desc[h[j]];
        flowtab_host(host_base, host_bytes, listed.data(), n_pass, nullptr, opts->flags, slots, opts->flow_cap, nullptr,
                     flows.data(), &r);
        copy_ms[it] = ms(t0, t1);
        table_ms[it] = ms(t1, now());
    }
    if (last) *last = r;   // so that the result is used (and can be checked)
    (void)hipHostFree(h);
    if (err != hipSuccess) return set_error(BT_E_INTERNAL, "bt_time_flow_table_host: %s", hipGetErrorString(err));
    return BT_OK;
}

int bt_time_flow_track(bt_ctx* c, void* state, const bt_batch* frames, const uint64_t* select, const bt_flow_track_update* upd,
                       void* scratch, uint64_t scratch_bytes, const bt_flow_track_out* out, uint32_t iters, float* ms) {
    const bt::DeviceRestore keep_device;   // the caller's current device, restored on return
    if (!c || !frames || !frames->n || !iters || !ms)
        return set_error(BT_E_INVALID_ARGUMENT, "null argument / empty batch / zero iterations");
    std::lock_guard<std::mutex> lk(c->mu);
    HIP_TRY(hipSetDevice(c->device));
    if (int rc = ensure_timing_events(c, iters)) return rc;
    for (uint32_t i = 0; i < iters; ++i)
        if (int rc = run_flow_track_update(c, state, frames, select, upd, scratch, scratch_bytes, out, c->stream,
                                           c->timing.tev[2 * i], c->timing.tev[2 * i + 1])) {
            (void)hipStreamSynchronize(c->stream);
            return rc;
        }
    HIP_TRY(hipStreamSynchronize(c->stream));
    for (uint32_t i = 0; i < iters; ++i) HIP_TRY(hipEventElapsedTime(&ms[i], c->timing.tev[2 * i], c->timing.tev[2 * i + 1]));
    return BT_OK;
}

int bt_time_flow_tcp(bt_ctx* c, const bt_batch* frames, const uint32_t* flow_id, uint32_t table_flags, bt_flow_tcp_rec* tcp,
                     uint32_t flow_cap, bt_flow_tcp_result* result, uint32_t iters, float* ms) {
    const bt::DeviceRestore keep_device;   // the caller's current device, restored on return
    if (!c || !frames || !frames->n || !iters || !ms)
        return set_error(BT_E_INVALID_ARGUMENT, "null argument / empty batch / zero iterations");
    std::lock_guard<std::mutex> lk(c->mu);
    HIP_TRY(hipSetDevice(c->device));
    if (int rc = ensure_timing_events(c, iters)) return rc;
    for (uint32_t i = 0; i < iters; ++i)
        if (int rc = run_flow_tcp(c, frames, flow_id, table_flags, tcp, flow_cap, result, c->stream, c->timing.tev[2 * i],
                                  c->timing.tev[2 * i + 1])) {
            (void)hipStreamSynchronize(c->stream);
            return rc;
        }
    HIP_TRY(hipStreamSynchronize(c->stream));
    for (uint32_t i = 0; i < iters; ++i) HIP_TRY(hipEventElapsedTime(&ms[i], c->timing.tev[2 * i], c->timing.tev[2 * i + 1]));
    return BT_OK;
}

int bt_time_flow_stat(bt_ctx* c, const bt_batch* frames, const uint32_t* flow_id, uint32_t table_flags, const bt_flow_track_update* upd,
                      bt_flow_stat_rec* stat, uint32_t flow_cap, bt_flow_stat_result* result, uint32_t iters, float* ms) {
    const bt::DeviceRestore keep_device;   // the caller's current device, restored on return
    if (!c || !frames || !frames->n || !iters || !ms)
        return set_error(BT_E_INVALID_ARGUMENT, "null argument / empty batch / zero iterations");
    std::lock_guard<std::mutex> lk(c->mu);
    HIP_TRY(hipSetDevice(c->device));
    if (int rc = ensure_timing_events(c, iters)) return rc;
    for (uint32_t i = 0; i < iters; ++i)
        if (int rc = run_flow_stat(c, frames, flow_id, table_flags, upd, stat, flow_cap, result, c->stream, c->timing.tev[2 * i],
                                   c->timing.tev[2 * i + 1])) {
            (void)hipStreamSynchronize(c->stream);
            return rc;
        }
    HIP_TRY(hipStreamSynchronize(c->stream));
    for (uint32_t i = 0; i < iters; ++i) HIP_TRY(hipEventElapsedTime(&ms[i], c->timing.tev[2 * i], c->timing.tev[2 * i + 1]));
    return BT_OK;
}

int bt_time_flow_mark(bt_ctx* c, const bt_batch* frames, const uint32_t* flow_id, const uint64_t* hit, const bt_flow_mark_update* upd,
                      bt_flow_mark_rec* table, uint32_t flow_cap, bt_flow_mark_result* result, const bt_flow_mark_select_opts* opts,
                      const uint64_t* base, uint64_t* out_select, bt_flow_mark_select_result* sel_result, uint32_t iters, float* update_ms,
                      float* select_ms) {
    const bt::DeviceRestore keep_device;   // the caller's current device, restored on return
    if (!c || !frames || !frames->n || !iters || (!update_ms && !select_ms))
        return set_error(BT_E_INVALID_ARGUMENT, "null argument / empty batch / zero iterations");
    std::lock_guard<std::mutex> lk(c->mu);
    HIP_TRY(hipSetDevice(c->device));
    if (int rc = ensure_timing_events(c, iters)) return rc;
    for (uint32_t pass = 0; pass < 2u; ++pass) {
        float* const ms = pass ? select_ms : update_ms;
        if (!ms) continue;
        for (uint32_t i = 0; i < iters; ++i) {
            hipEvent_t e0 = c->timing.tev[2 * i], e1 = c->timing.tev[2 * i + 1];
            const int rc = pass ? run_flow_mark_select(c, flow_id, frames->n, table, flow_cap, opts, base, out_select, sel_result, c->stream, e0, e1)
                                : run_flow_mark(c, frames, flow_id, hit, upd, table, flow_cap, result, c->stream, e0, e1);
            if (rc) {
                (void)hipStreamSynchronize(c->stream);
                return rc;
            }
        }
        HIP_TRY(hipStreamSynchronize(c->stream));
        for (uint32_t i = 0; i < iters; ++i) HIP_TRY(hipEventElapsedTime(&ms[i], c->timing.tev[2 * i], c->timing.tev[2 * i + 1]));
    }
    return BT_OK;
}

int bt_time_flow_seq(bt_ctx* c, const bt_batch* frames, const uint32_t* flow_id, const uint64_t* select, const bt_flow_seq_opts* opts,
                     bt_flow_seq_rec* table, uint32_t flow_cap, const bt_flow_seq_out* out, void* scratch, uint64_t scratch_bytes,
                     bt_flow_seq_result* result, uint32_t iters, float* ms, float* phase_ms) {
    const bt::DeviceRestore keep_device;   // the caller's current device, restored on return
    if (!c || !frames || !frames->n || !iters || !ms)
        return set_error(BT_E_INVALID_ARGUMENT, "null argument / empty batch / zero iterations");
    std::lock_guard<std::mutex> lk(c->mu);
    HIP_TRY(hipSetDevice(c->device));
    if (int rc = ensure_timing_events(c, (5u * iters + 1u) / 2u)) return rc;
    for (uint32_t i = 0; i < iters; ++i) {
        void* ev[5];
        for (uint32_t k = 0; k < 5u; ++k) ev[k] = c->timing.tev[5 * i + k];
        if (int rc = run_flow_seq(c, frames, flow_id, select, opts, table, flow_cap, out, scratch, scratch_bytes, result, c->stream, ev)) {
            (void)hipStreamSynchronize(c->stream);
            return rc;
        }
    }
    HIP_TRY(hipStreamSynchronize(c->stream));
    const bool sorted = bt::fs_passes(flow_cap) != 0u;   // without a pass the sort's event is not recorded
    for (uint32_t i = 0; i < iters; ++i) {
        hipEvent_t* const e = &c->timing.tev[5 * i];
        HIP_TRY(hipEventElapsedTime(&ms[i], e[0], e[4]));
        if (!phase_ms) continue;
        float* const ph = phase_ms + 4 * i;
        ph[1] = 0.f;
        HIP_TRY(hipEventElapsedTime(&ph[0], e[0], sorted ? e[1] : e[2]));
        if (sorted) HIP_TRY(hipEventElapsedTime(&ph[1], e[1], e[2]));
        HIP_TRY(hipEventElapsedTime(&ph[2], e[2], e[3]));
        HIP_TRY(hipEventElapsedTime(&ph[3], e[3], e[4]));
    }
    return BT_OK;
}

int bt_time_flow_stream(bt_ctx* c, const bt_batch* frames, const uint32_t* flow_id, const uint64_t* select, uint32_t table_flags,
                        const void* pattern, const void* pattern_device, uint32_t pattern_bytes, bt_flow_stream_rec* table,
                        uint32_t flow_cap, void* scratch, uint64_t scratch_bytes, const bt_flow_stream_out* out, uint32_t iters, float* ms,
                        float* phase_ms) {
    const bt::DeviceRestore keep_device;   // the caller's current device, restored on return
    if (!c || !frames || !frames->n || !iters || !ms)
        return set_error(BT_E_INVALID_ARGUMENT, "null argument / empty batch / zero iterations");
    std::lock_guard<std::mutex> lk(c->mu);
    HIP_TRY(hipSetDevice(c->device));
    if (int rc = ensure_timing_events(c, (5u * iters + 1u) / 2u)) return rc;
    for (uint32_t i = 0; i < iters; ++i) {
        void* ev[5];
        for (uint32_t k = 0; k < 5u; ++k) ev[k] = c->timing.tev[5 * i + k];
        if (int rc = run_flow_stream(c, frames, flow_id, select, table_flags, pattern, pattern_device, pattern_bytes, table, flow_cap,
                                     scratch, scratch_bytes, out, c->stream, ev)) {
            (void)hipStreamSynchronize(c->stream);
            return rc;
        }
    }
    HIP_TRY(hipStreamSynchronize(c->stream));
    for (uint32_t i = 0; i < iters; ++i) {
        hipEvent_t* const e = &c->timing.tev[5 * i];
        HIP_TRY(hipEventElapsedTime(&ms[i], e[0], e[4]));
        if (!phase_ms) continue;
        for (uint32_t k = 0; k < 4u; ++k) HIP_TRY(hipEventElapsedTime(&phase_ms[4 * i + k], e[k], e[k + 1]));
    }
    return BT_OK;
}

int bt_time_flow_tcpseq(bt_ctx* c, const bt_batch* frames, const uint32_t* flow_id, const uint64_t* select, uint32_t table_flags,
                        bt_flow_tcpseq_rec* table, uint32_t flow_cap, void* scratch, uint64_t scratch_bytes, const bt_flow_tcpseq_out* out,
                        uint32_t iters, float* ms, float* phase_ms) {
    const bt::DeviceRestore keep_device;   // the caller's current device, restored on return
    if (!c || !frames || !frames->n || !iters || !ms)
        return set_error(BT_E_INVALID_ARGUMENT, "null argument / empty batch / zero iterations");
    std::lock_guard<std::mutex> lk(c->mu);
    HIP_TRY(hipSetDevice(c->device));
    if (int rc = ensure_timing_events(c, (5u * iters + 1u) / 2u)) return rc;
    for (uint32_t i = 0; i < iters; ++i) {
        void* ev[5];
        for (uint32_t k = 0; k < 5u; ++k) ev[k] = c->timing.tev[5 * i + k];
        if (int rc = run_flow_tcpseq(c, frames, flow_id, select, table_flags, table, flow_cap, scratch, scratch_bytes, out, c->stream, ev)) {
            (void)hipStreamSynchronize(c->stream);
            return rc;
        }
    }
    HIP_TRY(hipStreamSynchronize(c->stream));
    for (uint32_t i = 0; i < iters; ++i) {
        hipEvent_t* const e = &c->timing.tev[5 * i];
        HIP_TRY(hipEventElapsedTime(&ms[i], e[0], e[4]));
        if (!phase_ms) continue;
        for (uint32_t k = 0; k < 4u; ++k) HIP_TRY(hipEventElapsedTime(&phase_ms[4 * i + k], e[k], e[k + 1]));
    }
    return BT_OK;
}

int bt_time_flow_reasm(bt_ctx* c, const bt_batch* frames, const uint32_t* flow_id, const uint64_t* select, const int64_t* off,
                       uint32_t table_flags, const void* pattern, const void* pattern_device, uint32_t pattern_bytes,
                       bt_flow_reasm_rec* table, uint32_t flow_cap, void* scratch, uint64_t scratch_bytes, const bt_flow_reasm_out* out,
                       uint32_t iters, float* ms, float* phase_ms) {
    const bt::DeviceRestore keep_device;   // the caller's current device, restored on return
    if (!c || !frames || !frames->n || !iters || !ms)
        return set_error(BT_E_INVALID_ARGUMENT, "null argument / empty batch / zero iterations");
    std::lock_guard<std::mutex> lk(c->mu);
    HIP_TRY(hipSetDevice(c->device));
    if (int rc = ensure_timing_events(c, (7u * iters + 1u) / 2u)) return rc;
    for (uint32_t i = 0; i < iters; ++i) {
        void* ev[7];
        for (uint32_t k = 0; k < 7u; ++k) ev[k] = c->timing.tev[7 * i + k];
        if (int rc = run_flow_reasm(c, frames, flow_id, select, off, table_flags, pattern, pattern_device, pattern_bytes, table, flow_cap,
                                    scratch, scratch_bytes, out, c->stream, ev)) {
            (void)hipStreamSynchronize(c->stream);
            return rc;
        }
    }
    HIP_TRY(hipStreamSynchronize(c->stream));
    for (uint32_t i = 0; i < iters; ++i) {
        hipEvent_t* const e = &c->timing.tev[7 * i];
        HIP_TRY(hipEventElapsedTime(&ms[i], e[0], e[6]));
        if (!phase_ms) continue;
        for (uint32_t k = 0; k < 6u; ++k) HIP_TRY(hipEventElapsedTime(&phase_ms[6 * i + k], e[k], e[k + 1]));
    }
    return BT_OK;
}

int bt_time_flow_follow(bt_ctx* c, const bt_batch* frames, const uint32_t* flow_id, const uint64_t* select, const int64_t* off,
                        uint32_t table_flags, const void* pattern, const void* pattern_device, uint32_t pattern_bytes,
                        bt_flow_reasm_rec* table, uint32_t flow_cap, void* scratch, uint64_t scratch_bytes, const bt_flow_reasm_out* out,
                        const bt_flow_follow_out* fo, uint32_t iters, float* ms, float* phase_ms) {
    const bt::DeviceRestore keep_device;   // the caller's current device, restored on return
    if (!c || !frames || !frames->n || !iters || !ms)
        return set_error(BT_E_INVALID_ARGUMENT, "null argument / empty batch / zero iterations");
    std::lock_guard<std::mutex> lk(c->mu);
    HIP_TRY(hipSetDevice(c->device));
    if (int rc = ensure_timing_events(c, (9u * iters + 1u) / 2u)) return rc;
    for (uint32_t i = 0; i < iters; ++i) {
        void* ev[9];
        for (uint32_t k = 0; k < 9u; ++k) ev[k] = c->timing.tev[9 * i + k];
        if (int rc = run_flow_follow(c, frames, flow_id, select, off, table_flags, pattern, pattern_device, pattern_bytes, table, flow_cap,
                                     scratch, scratch_bytes, out, fo, c->stream, ev)) {
            (void)hipStreamSynchronize(c->stream);
            return rc;
        }
    }
    HIP_TRY(hipStreamSynchronize(c->stream));
    for (uint32_t i = 0; i < iters; ++i) {
        hipEvent_t* const e = &c->timing.tev[9 * i];
        HIP_TRY(hipEventElapsedTime(&ms[i], e[0], e[8]));
        if (!phase_ms) continue;
        for (uint32_t k = 0; k < 8u; ++k) HIP_TRY(hipEventElapsedTime(&phase_ms[8 * i + k], e[k], e[k + 1]));
    }
    return BT_OK;
}

int bt_time_flow_top(bt_ctx* c, const void* state, const bt_flow_top_opts* opts, const bt_flow_tcp_rec* tcp, void* scratch,
                     uint64_t scratch_bytes, const bt_flow_top_out* out, uint32_t iters, float* ms) {
    const bt::DeviceRestore keep_device;   // the caller's current device, restored on return
    if (!c || !iters || !ms) return set_error(BT_E_INVALID_ARGUMENT, "null argument / zero iterations");
    std::lock_guard<std::mutex> lk(c->mu);
    HIP_TRY(hipSetDevice(c->device));
    if (int rc = ensure_timing_events(c, iters)) return rc;
    for (uint32_t i = 0; i < iters; ++i)
        if (int rc = run_flow_track_top(c, state, opts, tcp, scratch, scratch_bytes, out, c->stream, c->timing.tev[2 * i],
                                        c->timing.tev[2 * i + 1])) {
            (void)hipStreamSynchronize(c->stream);
            return rc;
        }
    HIP_TRY(hipStreamSynchronize(c->stream));
    for (uint32_t i = 0; i < iters; ++i) HIP_TRY(hipEventElapsedTime(&ms[i], c->timing.tev[2 * i], c->timing.tev[2 * i + 1]));
    return BT_OK;
}

// What the top-K query replaces: every record of the tracker copied to pinned host memory, then the
// k largest by bytes picked on the calling thread (tools/pcap_flows.py's download and sorted()[:k], in C++).
int bt_time_flow_top_host(bt_ctx* c, const bt_flow_track_rec* recs, uint32_t n_flows, uint32_t k, uint32_t iters, float* copy_ms,
                          float* sort_ms, uint64_t* top_total) {
    const bt::DeviceRestore keep_device;   // the caller's current device, restored on return
    if (!c || !recs || !n_flows || !iters || !copy_ms || !sort_ms)
        return set_error(BT_E_INVALID_ARGUMENT, "null argument / no flows / zero iterations");
    std::lock_guard<std::mutex> lk(c->mu);
    HIP_TRY(hipSetDevice(c->device));
    bt_flow_track_rec* h = nullptr;
    HIP_TRY(hipHostMalloc(&h, (size_t)n_flows * sizeof(bt_flow_track_rec), hipHostMallocDefault));
    std::memset(static_cast<void*>(h), 0, (size_t)n_flows * sizeof(bt_flow_track_rec));   // first touch outside the timed part
    std::vector<uint32_t> order(n_flows);
    const uint32_t top = k < n_flows ? k : n_flows;
    const auto now = [] { return std::chrono::steady_clock::now(); };
    const auto ms = [](auto a, auto b) { return std::chrono::duration<float, std::milli>(b - a).count(); };
    hipError_t err = hipSuccess;
    uint64_t sum = 0;
    for (uint32_t it = 0; it < iters && err == hipSuccess; ++it) {
        const auto t0 = now();
        err = hipMemcpyAsync(h, recs, (size_t)n_flows * sizeof(bt_flow_track_rec), hipMemcpyDeviceToHost, c->stream);
        if (err == hipSuccess) err = hipStreamSynchronize(c->stream);
        const auto t1 = now();
        if (err == hipSuccess) {
            for (uint32_t f = 0; f < n_flows; ++f) order[f] = f;
            const auto val = [&](uint32_t f) { return h[f].bytes[0] + h[f].bytes[1]; };
            std::partial_sort(order.begin(), order.begin() + top, order.end(),
                              [&](uint32_t x, uint32_t y) { return val(x) != val(y) ? val(x) > val(y) : x < y; });
            sum = 0;
            for (uint32_t r = 0; r < top; ++r) sum += val(order[r]);
        }
        copy_ms[it] = ms(t0, t1);
        sort_ms[it] = ms(t1, now());
    }
    if (top_total) *top_total = sum;   // so that the result is used (and can be checked)
    (void)hipHostFree(h);
    if (err != hipSuccess) return set_error(BT_E_INTERNAL, "bt_time_flow_top_host: %s", hipGetErrorString(err));
    return BT_OK;
}

int bt_time_flow_hosts(bt_ctx* c, const void* state, const bt_flow_hosts_opts* opts, const bt_flow_tcp_rec* tcp, void* scratch,
                       uint64_t scratch_bytes, const bt_flow_hosts_out* out, uint32_t iters, float* ms) {
    const bt::DeviceRestore keep_device;   // the caller's current device, restored on return
    if (!c || !iters || !ms) return set_error(BT_E_INVALID_ARGUMENT, "null argument / zero iterations");
    std::lock_guard<std::mutex> lk(c->mu);
    HIP_TRY(hipSetDevice(c->device));
    if (int rc = ensure_timing_events(c, iters)) return rc;
    for (uint32_t i = 0; i < iters; ++i)
        if (int rc = run_flow_track_hosts(c, state, opts, tcp, scratch, scratch_bytes, out, c->stream, c->timing.tev[2 * i],
                                          c->timing.tev[2 * i + 1])) {
            (void)hipStreamSynchronize(c->stream);
            return rc;
        }
    HIP_TRY(hipStreamSynchronize(c->stream));
    for (uint32_t i = 0; i < iters; ++i) HIP_TRY(hipEventElapsedTime(&ms[i], c->timing.tev[2 * i], c->timing.tev[2 * i + 1]));
    return BT_OK;
}

// What the endpoint table replaces: the header and the n_flows records of a tracker, and its side
// records, copied to pinned host memory, then bt_flow_track_hosts_host over them on the calling thread.
int bt_time_flow_hosts_host(bt_ctx* c, const void* state, uint32_t n_flows, const bt_flow_tcp_rec* tcp,
                            const bt_flow_hosts_opts* opts, uint32_t iters, float* copy_ms, float* group_ms,
                            bt_flow_hosts_result* last, uint64_t* sums) {
    const bt::DeviceRestore keep_device;   // the caller's current device, restored on return
    bt::FkShadow sh{};
    bt_flow_track_sizes sl{};
    char why[128];
    if (!c || !state || !opts || !iters || !copy_ms || !group_ms || !bt::fk_known_state(state, &sh) ||
        !bt::fk_layout(sh.flow_cap, sh.slots, &sl, why, sizeof(why)) || n_flows > sh.flow_cap)
        return set_error(BT_E_INVALID_ARGUMENT, "null argument / unknown state / zero iterations");
    std::lock_guard<std::mutex> lk(c->mu);
    HIP_TRY(hipSetDevice(c->device));
    const size_t head = (size_t)sl.records + (size_t)n_flows * sizeof(bt_flow_track_rec), side = (size_t)n_flows * sizeof(bt_flow_tcp_rec);
    uint8_t* h = nullptr;
    bt_flow_tcp_rec* ht = nullptr;
    HIP_TRY(hipHostMalloc(reinterpret_cast<void**>(&h), (size_t)sl.total, hipHostMallocDefault));   // 256-byte aligned and more
    if (tcp && hipHostMalloc(reinterpret_cast<void**>(&ht), side ? side : 16u, hipHostMallocDefault) != hipSuccess) {
        (void)hipHostFree(h);
        return set_error(BT_E_RESOURCE, "bt_time_flow_hosts_host: no pinned memory for the side table");
    }
    std::memset(h, 0, head);   // first touch outside the timed part
    if (ht) std::memset(static_cast<void*>(ht), 0, side);
    std::vector<bt_flow_host_rec> hosts(opts->host_cap ? opts->host_cap : 1u);
    const auto now = [] { return std::chrono::steady_clock::now(); };
    const auto ms = [](auto a, auto b) { return std::chrono::duration<float, std::milli>(b - a).count(); };
    hipError_t err = hipSuccess;
    int rc = BT_OK;
    bt_flow_hosts_result res{};
    for (uint32_t it = 0; it < iters && err == hipSuccess && rc == BT_OK; ++it) {
        const auto t0 = now();
        err = hipMemcpyAsync(h, state, head, hipMemcpyDeviceToHost, c->stream);
        if (err == hipSuccess && ht && side) err = hipMemcpyAsync(ht, tcp, side, hipMemcpyDeviceToHost, c->stream);
        if (err == hipSuccess) err = hipStreamSynchronize(c->stream);
        const auto t1 = now();
        if (err == hipSuccess) {
            const bt_flow_hosts_out out{hosts.data(), nullptr, &res};
            rc = bt_flow_track_hosts_host(h, sl.total, opts, ht, &out);
        }
        copy_ms[it] = ms(t0, t1);
        group_ms[it] = ms(t1, now());
    }
    if (last) *last = res;   // so that the result is used (and can be checked)
    if (sums) {   // over the records the last run wrote: what the caller compares the device's records with
        for (int j = 0; j < 6; ++j) sums[j] = 0;
        for (uint32_t k = 0; k < res.n_written; ++k) {
            const bt_flow_host_rec& r = hosts[k];
            sums[0] += r.packets[0]; sums[1] += r.packets[1]; sums[2] += r.bytes[0] ^ r.bytes[1];
            sums[3] += (uint64_t)r.flows[0] + r.flows[1];
            for (int j = 0; j < 7; ++j) sums[4] += (uint64_t)r.tcp_state[j] * (uint64_t)(j + 1);
            sums[5] += r.first_ts ^ r.last_ts ^ ((uint64_t)r.first_flow << 32 | r.syn_packets);
        }
    }
    (void)hipHostFree(h);
    if (ht) (void)hipHostFree(ht);
    if (err != hipSuccess) return set_error(BT_E_INTERNAL, "bt_time_flow_hosts_host: %s", hipGetErrorString(err));
    return rc;
}

// What the tracker replaces: a batch's flow records copied to pinned host memory, then merged into
// a table on the calling thread (tools/pcap_flows.py's per-chunk download and fold, in C++).
int bt_time_flow_track_host(bt_ctx* c, const bt_flow_rec* flows, uint32_t n_flows, void* host_state, uint64_t state_bytes,
                            uint64_t batch_ts, uint32_t iters, float* copy_ms, float* merge_ms, bt_flow_track_result* last) {
    const bt::DeviceRestore keep_device;   // the caller's current device, restored on return
    if (!c || !flows || !n_flows || !iters || !copy_ms || !merge_ms)
        return set_error(BT_E_INVALID_ARGUMENT, "null argument / no flows / zero iterations");
    char why[160];
    FkHostState hs{};
    if (!fk_host_state(host_state, state_bytes, &hs, why, sizeof(why))) return set_error(BT_E_INVALID_ARGUMENT, "bt_time_flow_track_host: %s", why);
    std::lock_guard<std::mutex> lk(c->mu);
    HIP_TRY(hipSetDevice(c->device));
    bt_flow_rec* h = nullptr;
    HIP_TRY(hipHostMalloc(&h, (size_t)n_flows * sizeof(bt_flow_rec), hipHostMallocDefault));
    std::memset(static_cast<void*>(h), 0, (size_t)n_flows * sizeof(bt_flow_rec));   // first touch outside the timed part
    bt_flow_table_result fr{};
    fr.n_flows = n_flows;
    bt_flow_track_result r{};
    const auto now = [] { return std::chrono::steady_clock::now(); };
    const auto ms = [](auto a, auto b) { return std::chrono::duration<float, std::milli>(b - a).count(); };
    hipError_t err = hipSuccess;
    for (uint32_t it = 0; it < iters && err == hipSuccess; ++it) {
        const auto t0 = now();
        err = hipMemcpyAsync(h, flows, (size_t)n_flows * sizeof(bt_flow_rec), hipMemcpyDeviceToHost, c->stream);
        if (err == hipSuccess) err = hipStreamSynchronize(c->stream);
        const auto t1 = now();
        if (err == hipSuccess) fk_merge_host(hs, h, fr, 0u, nullptr, batch_ts, nullptr, &r);
        copy_ms[it] = ms(t0, t1);
        merge_ms[it] = ms(t1, now());
    }
    if (last) *last = r;   // so that the result is used (and can be checked)
    (void)hipHostFree(h);
    if (err != hipSuccess) return set_error(BT_E_INTERNAL, "bt_time_flow_track_host: %s", hipGetErrorString(err));
    return BT_OK;
}

// What the tally replaces: the decision bytes copied to pinned host memory, then the 16-part host
// scan of GpuPacketFilter::scanParallel's inner loop (counted, passed, rejected per slot, up to
// the first throw of each part) on the context's host threads.
int bt_time_tally_host(bt_ctx* c, const uint8_t* decide, uint32_t n, uint32_t iters, float* copy_ms, float* scan_ms,
                       uint64_t* counts) {
    const bt::DeviceRestore keep_device;   // the caller's current device, restored on return
    if (!c || !decide || !n || !iters || !copy_ms || !scan_ms) return set_error(BT_E_INVALID_ARGUMENT, "null argument / empty batch / zero iterations");
    std::lock_guard<std::mutex> lk(c->mu);
    HIP_TRY(hipSetDevice(c->device));
    uint8_t* h = nullptr;
    HIP_TRY(hipHostMalloc(&h, n, hipHostMallocDefault));
    std::memset(h, 0, n);   // first touch outside the timed part
    constexpr uint32_t kParts = 16;
    struct Part { uint64_t counted = 0, passed = 0, rejected[64] = {}; bool stopped = false; char pad[64]; };
    HostPool& pool = pool_of(c);   // the threads bt_host_parallel lends to scanParallel
    const unsigned T = pool.size();
    const auto now = [] { return std::chrono::steady_clock::now(); };
    const auto ms = [](auto a, auto b) { return std::chrono::duration<float, std::milli>(b - a).count(); };
    hipError_t err = hipSuccess;
    std::vector<Part> parts(kParts);
    for (uint32_t it = 0; it < iters && err == hipSuccess; ++it) {
        const auto t0 = now();
        err = hipMemcpyAsync(h, decide, n, hipMemcpyDeviceToHost, c->stream);
        if (err == hipSuccess) err = hipStreamSynchronize(c->stream);
        const auto t1 = now();
        parts.assign(kParts, Part{});
        pool.run([&](unsigned w) {
                for (uint32_t k = w; k < kParts; k += T) {
                    Part& p = parts[k];
                    const size_t lo = (size_t)n * k / kParts, hi = (size_t)n * (k + 1) / kParts;
                    for (size_t i = lo; i < hi; ++i) {
                        const uint32_t d = h[i], code = d >> 6;
                        if (code >= BT_DECIDE_THROW) { p.stopped = true; break; }
                        ++p.counted;
                        if (code == BT_DECIDE_PASS) ++p.passed;
                        else ++p.rejected[d & 63u];
                    }
                }
            });
        copy_ms[it] = ms(t0, t1);
        scan_ms[it] = ms(t1, now());
    }
    if (counts) {   // counted, passed: so that the scan's result is used (and can be checked)
        counts[0] = counts[1] = 0;
        for (const Part& p : parts) {
            counts[0] += p.counted;
            counts[1] += p.passed;
            if (p.stopped) break;
        }
    }
    (void)hipHostFree(h);
    if (err != hipSuccess) return set_error(BT_E_INTERNAL, "bt_time_tally_host: %s", hipGetErrorString(err));
    return BT_OK;
}

// What the fan-out replaces: the ordered pass list copied to pinned host memory, then
// bt_flow_hash_host's key and hash per passing frame and a stable K-way bucket of the indices, in
// 16 contiguous parts on the context's host threads (count, prefix, scatter).
int bt_time_fanout_host(bt_ctx* c, const uint32_t* pass_idx, uint32_t n_pass, const uint8_t* host_base,
                        const bt_pkt_desc* host_desc, const bt_fanout_opts* opts, uint32_t iters, float* copy_ms,
                        float* bucket_ms, uint32_t* counts) {
    const bt::DeviceRestore keep_device;   // the caller's current device, restored on return
    if (!c || !pass_idx || !n_pass || !host_base || !host_desc || !iters || !copy_ms || !bucket_ms)
        return set_error(BT_E_INVALID_ARGUMENT, "null argument / empty list / zero iterations");
    uint8_t key[kFanKeyBytes], reta[kFanReta];
    char why[96];
    if (!fanout_opts(opts, key, reta, why, sizeof(why))) return set_error(BT_E_INVALID_ARGUMENT, "bt_time_fanout_host: %s", why);
    const bool l3_only = (opts->flags & BT_FANOUT_L3_ONLY) != 0;
    std::lock_guard<std::mutex> lk(c->mu);
    HIP_TRY(hipSetDevice(c->device));
    uint32_t* h = nullptr;
    HIP_TRY(hipHostMalloc(&h, (size_t)n_pass * 4, hipHostMallocDefault));
    std::memset(h, 0, (size_t)n_pass * 4);   // first touch outside the timed part
    std::vector<uint8_t> queue(n_pass);
    std::vector<uint32_t> idx(n_pass);
    constexpr uint32_t kParts = 16;
    struct Part { uint32_t count[64] = {}; char pad[64]; };
    std::vector<Part> parts(kParts);
    HostPool& pool = pool_of(c);
    const unsigned T = pool.size();
    const auto now = [] { return std::chrono::steady_clock::now(); };
    const auto ms = [](auto a, auto b) { return std::chrono::duration<float, std::milli>(b - a).count(); };
    hipError_t err = hipSuccess;
    for (uint32_t it = 0; it < iters && err == hipSuccess; ++it) {
        const auto t0 = now();
        err = hipMemcpyAsync(h, pass_idx, (size_t)n_pass * 4, hipMemcpyDeviceToHost, c->stream);
        if (err == hipSuccess) err = hipStreamSynchronize(c->stream);
        const auto t1 = now();
        parts.assign(kParts, Part{});
        pool.run([&](unsigned w) {
                for (uint32_t k = w; k < kParts; k += T) {
                    const size_t lo = (size_t)n_pass * k / kParts, hi = (size_t)n_pass * (k + 1) / kParts;
                    for (size_t j = lo; j < hi; ++j) {
                        const bt_pkt_desc d = host_desc[h[j]];
                        uint8_t in[kFanInputMax];
                        uint32_t klass;
                        const uint32_t nb = flow_key_host(host_base + BT_DESC_OFF(d), BT_DESC_LEN(d), l3_only, in, &klass);
                        queue[j] = reta[toeplitz_host(key, in, nb) & 127u];
                        ++parts[k].count[queue[j]];
                    }
                }
            });
        uint32_t at = 0;   // queue-major, part-minor exclusive scan
        for (uint32_t q = 0; q < 64u; ++q)
            for (uint32_t k = 0; k < kParts; ++k) { const uint32_t v = parts[k].count[q]; parts[k].count[q] = at; at += v; }
        pool.run([&](unsigned w) {
                for (uint32_t k = w; k < kParts; k += T) {
                    const size_t lo = (size_t)n_pass * k / kParts, hi = (size_t)n_pass * (k + 1) / kParts;
                    for (size_t j = lo; j < hi; ++j) idx[parts[k].count[queue[j]]++] = h[j];
                }
            });
        copy_ms[it] = ms(t0, t1);
        bucket_ms[it] = ms(t1, now());
    }
    if (counts) {   // the first index of every queue's range and the list's last entry: so that the result is used
        for (uint32_t q = 0; q < 64u; ++q) counts[q] = parts[0].count[q];
        counts[64] = idx[n_pass - 1];
    }
    (void)hipHostFree(h);
    if (err != hipSuccess) return set_error(BT_E_INTERNAL, "bt_time_fanout_host: %s", hipGetErrorString(err));
    return BT_OK;
}

int bt_time_copy_d2d(bt_ctx* c, void* dst, const void* src, uint64_t bytes, uint32_t iters, float* ms) {
    const bt::DeviceRestore keep_device;   // the caller's current device, restored on return
    if (!c || !dst || !src || !bytes || !iters || !ms) return set_error(BT_E_INVALID_ARGUMENT, "null argument / zero size");
    std::lock_guard<std::mutex> lk(c->mu);
    HIP_TRY(hipSetDevice(c->device));
    if (int rc = ensure_timing_events(c, iters)) return rc;
    for (uint32_t i = 0; i < iters; ++i) {
        HIP_TRY(hipEventRecord(c->timing.tev[2 * i], c->stream));
        HIP_TRY(hipMemcpyAsync(dst, src, bytes, hipMemcpyDeviceToDevice, c->stream));
        HIP_TRY(hipEventRecord(c->timing.tev[2 * i + 1], c->stream));
    }
    HIP_TRY(hipStreamSynchronize(c->stream));
    for (uint32_t i = 0; i < iters; ++i) HIP_TRY(hipEventElapsedTime(&ms[i], c->timing.tev[2 * i], c->timing.tev[2 * i + 1]));
    return BT_OK;
}

int bt_time_device2(bt_ctx* c, const bt_batch* b, const bt_outputs* outs, uint32_t n_out, uint32_t iters,
                    uint32_t mode, bt_timing* t) {
    const bt::DeviceRestore keep_device;   // the caller's current device, restored on return
    if (!c || !b || !outs || !n_out || !iters) return set_error(BT_E_INVALID_ARGUMENT, "null argument / zero iterations");
    if (mode & ~(uint32_t)(BT_TIME_KERNEL_EVENTS | BT_TIME_PIPELINED)) return set_error(BT_E_INVALID_ARGUMENT, "unknown mode");
    std::lock_guard<std::mutex> lk(c->mu);
    HIP_TRY(hipSetDevice(c->device));
    const bool kev = (mode & BT_TIME_KERNEL_EVENTS) != 0;
    const bool piped = (mode & BT_TIME_PIPELINED) != 0;
    if (kev) { if (int rc = ensure_timing_events(c, iters)) return rc; }
    // BT_OPT_GRAPH: the K steps replay as one hipGraph (no per-kernel events: HIP cannot
    // time events recorded inside a captured graph), main_ms is then reported as -1.
    const bool use_graph = (c->opts.flags & BT_OPT_GRAPH) != 0 && !piped;
    const bt_outputs* o = outs;
    const bool cached = c->tgraph.exec && c->tgraph.iters == iters && !std::memcmp(&c->tgraph.batch, b, sizeof(*b)) &&
                        !std::memcmp(&c->tgraph.out, o, sizeof(*o));
    if (use_graph && !cached) {
        // Build once (the first call is the caller's untimed warm-up): the main kernel +
        // the compaction kernels, K times, in one graph.
        if (c->tgraph.exec) { (void)hipGraphExecDestroy(c->tgraph.exec); c->tgraph.exec = nullptr; }
        if (o->pass_idx || o->n_pass) { int rc = ensure_ws(c, b->n); if (rc) return rc; }
        hipGraph_t g = nullptr;
        HIP_TRY(hipStreamBeginCapture(c->stream, hipStreamCaptureModeRelaxed));
        int rc = BT_OK;
        for (uint32_t i = 0; rc == BT_OK && i < iters; ++i) rc = run_device(c, b, o, c->stream, false, nullptr, nullptr);
        hipError_t ee = hipStreamEndCapture(c->stream, &g);
        if (rc) { if (g) (void)hipGraphDestroy(g); return rc; }
        if (ee != hipSuccess || !g) return set_error(BT_E_INTERNAL, "graph capture failed: %s", hipGetErrorString(ee));
        hipError_t e = hipGraphInstantiate(&c->tgraph.exec, g, nullptr, nullptr, 0);
        (void)hipGraphDestroy(g);
        if (e != hipSuccess) { c->tgraph.exec = nullptr; return set_error(BT_E_INTERNAL, "hipGraphInstantiate: %s", hipGetErrorString(e)); }
        c->tgraph.batch = *b;
        c->tgraph.out = *o;
        c->tgraph.iters = iters;
    }
    if (piped) {
        if (int rc = ensure_cstream(c)) return rc;
        if (!c->timing.pipe_done) HIP_TRY(hipEventCreateWithFlags(&c->timing.pipe_done, hipEventDisableTiming));
        if (!c->timing.pipe_step) HIP_TRY(hipEventCreateWithFlags(&c->timing.pipe_step, hipEventDisableTiming));
    }
    const auto h0 = std::chrono::steady_clock::now();
    HIP_TRY(hipEventRecord(c->timing.ev0, c->stream));
    if (use_graph) {
        HIP_TRY(hipGraphLaunch(c->tgraph.exec, c->stream));
    } else {
        // Step i uses output set i % n_out. Pipelined (bt_parse_filter_device_async per
        // step): each compaction runs beside the next step's main kernel and the last one
        // joins c->stream before the closing event. The per-kernel event pairs
        // (BT_TIME_KERNEL_EVENTS) are recorded by the main kernel's own dispatch; they cost
        // the GPU ~9 us per launch on gfx950 (tools/calib/boundary.hip), so the bench
        // times its steps without them and measures the kernel in a second pass.
        // With one output set, step i + 1's main kernel would rewrite the verdict words
        // step i's compaction reads: it waits for that compaction (no overlap, no race).
        const bool serial = piped && n_out == 1;
        for (uint32_t i = 0; i < iters; ++i) {
            const bt_outputs* oi = outs + (i % n_out);
            hipEvent_t e0 = kev ? c->timing.tev[2 * i] : nullptr, e1 = kev ? c->timing.tev[2 * i + 1] : nullptr;
            if (serial && i) HIP_TRY(hipStreamWaitEvent(c->stream, c->timing.pipe_step, 0));
            int rc = piped ? run_device(c, b, oi, c->stream, false, e0, e1, c->ws.cstream,
                                        i + 1 == iters ? c->timing.pipe_done : serial ? c->timing.pipe_step : nullptr)
                           : run_device(c, b, oi, c->stream, false, e0, e1);
            if (rc) return rc;
        }
        if (piped) HIP_TRY(hipStreamWaitEvent(c->stream, c->timing.pipe_done, 0));
    }
    HIP_TRY(hipEventRecord(c->timing.ev1, c->stream));
    return finish_timing(c, iters, use_graph || !kev, h0, t, "bt_time_device");
}

int bt_time_device_ex(bt_ctx* c, const bt_batch* b, const bt_outputs* o, uint32_t iters, bt_timing* t) {
    const bt::DeviceRestore keep_device;   // the caller's current device, restored on return
    const uint32_t mode = BT_TIME_KERNEL_EVENTS | ((c && (c->opts.flags & BT_OPT_PIPELINE)) ? BT_TIME_PIPELINED : 0u);
    return bt_time_device2(c, b, o, 1, iters, mode, t);
}

int bt_time_device(bt_ctx* c, const bt_batch* b, const bt_outputs* o, uint32_t iters, float* ms_per_iter,
                   float* main_ms) {
    const bt::DeviceRestore keep_device;   // the caller's current device, restored on return
    bt_timing t{};
    const int rc = bt_time_device_ex(c, b, o, iters, &t);
    if (rc) return rc;
    if (ms_per_iter) *ms_per_iter = t.span_ms / iters;
    if (main_ms) *main_ms = t.main_ms;
    return BT_OK;
}

int bt_time_extract2(bt_ctx* c, const bt_batch* b, const bt_field_def* fields, uint32_t n_fields,
                     const bt_extract_out* out, uint32_t iters, uint32_t mode, bt_timing* t) {
    const bt::DeviceRestore keep_device;   // the caller's current device, restored on return
    if (!c || !b || !out || !iters) return set_error(BT_E_INVALID_ARGUMENT, "null argument / zero iterations");
    if (mode & ~(uint32_t)BT_TIME_KERNEL_EVENTS) return set_error(BT_E_INVALID_ARGUMENT, "unknown mode");
    const bool kev = (mode & BT_TIME_KERNEL_EVENTS) != 0;
    ExTable tab;
    bool never = false;
    int rc = build_table(fields, n_fields, &tab, nullptr, &never);
    if (rc) return rc;
    if (never || !b->n) return set_error(BT_E_INVALID_ARGUMENT, "nothing to time: empty batch or a span no frame reaches");
    std::lock_guard<std::mutex> lk(c->mu);
    HIP_TRY(hipSetDevice(c->device));
    if (kev && (rc = ensure_timing_events(c, iters))) return rc;
    const auto h0 = std::chrono::steady_clock::now();
    HIP_TRY(hipEventRecord(c->timing.ev0, c->stream));
    for (uint32_t i = 0; i < iters; ++i)
        if ((rc = run_extract(c, b, tab, never, out, c->stream, kev ? c->timing.tev[2 * i] : nullptr,
                              kev ? c->timing.tev[2 * i + 1] : nullptr)))
            return rc;
    HIP_TRY(hipEventRecord(c->timing.ev1, c->stream));
    return finish_timing(c, iters, !kev, h0, t, "bt_time_extract");
}

int bt_time_extract_ex(bt_ctx* c, const bt_batch* b, const bt_field_def* fields, uint32_t n_fields,
                       const bt_extract_out* out, uint32_t iters, bt_timing* t) {
    const bt::DeviceRestore keep_device;   // the caller's current device, restored on return
    return bt_time_extract2(c, b, fields, n_fields, out, iters, BT_TIME_KERNEL_EVENTS, t);
}

}  // extern "C"

namespace bt {

void release_timing_graph(bt_ctx* c) {
    if (c->tgraph.exec) (void)hipGraphExecDestroy(c->tgraph.exec);
}

void release_timing(bt_ctx* c) {
    if (c->timing.pipe_step) (void)hipEventDestroy(c->timing.pipe_step);
    for (auto e : c->timing.tev) (void)hipEventDestroy(e);
    if (c->timing.pipe_done) (void)hipEventDestroy(c->timing.pipe_done);
    if (c->timing.ev0) (void)hipEventDestroy(c->timing.ev0);
    if (c->timing.ev1) (void)hipEventDestroy(c->timing.ev1);
}

}  // namespace bt
