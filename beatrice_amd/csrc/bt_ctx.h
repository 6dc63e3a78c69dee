// bt_ctx.h — what a bt_ctx is, for the hipcc-compiled host units of libbeatrice_gpu.so
// (bt_context, bt_program, bt_launch, bt_timing, bt_host_batch, bt_memory, bt_extract_host,
// bt_group, bt_pcap), and the internals those units call across each other. Private: it names
// HIP types, so no g++-compiled unit and no installed header includes it.
//
// The context's fields are grouped by the unit that allocates them; each group has one
// release_<group>(bt_ctx*) in that unit, and bt_destroy (bt_context.cpp) calls them in turn.
#pragma once

#include <hip/hip_runtime.h>
#include <sched.h>

#include <atomic>
#include <chrono>
#include <cstdlib>
#include <memory>
#include <mutex>
#include <utility>
#include <vector>

#include "beatrice_gpu_bench.h"
#include "bt_device.h"
#include "bt_pack.h"
#include "bt_tally.h"
#include "bt_fanout.h"
#include "bt_flowtab.h"
#include "bt_host_pool.h"
#include "bt_host.h"

#define HIP_TRY(x)                                                                       \
    do {                                                                                 \
        hipError_t e_ = (x);                                                             \
        if (e_ != hipSuccess) return bt::set_error(BT_E_INTERNAL, "%s: %s", #x, hipGetErrorString(e_)); \
    } while (0)

namespace bt {

constexpr uint32_t kHostSlot = 112;   // bytes of each frame staged for the device (>= kNeedParse + pad)
// ... and with a GPU PAYLOAD slot in the program: applyPayloadFilter's window ends at most
// at 14 + 60 + 100 = 174 bytes (src/PacketFilter.cpp:293-309), rounded up to 16
constexpr uint32_t kHostSlotPayload = 176;
// ... and for calls that return no records and have no GPU PAYLOAD slot: the filters read
// bytes 12..37 (kNeedFilter) and such calls never take a second round, so 48 B
constexpr uint32_t kHostSlotFilter = 48;
// ... of which a filter-only call stages bytes [kLeanLo, kLeanLo + 32)
constexpr uint32_t kHostLeanWidth = 32;
static_assert(kLeanLo + kHostLeanWidth >= kNeedFilter && kLeanLo + kHostLeanWidth <= kHostSlotFilter, "lean staging");
constexpr uint32_t kGatherAheadDefault = 12;   // frames the host gather prefetches ahead
static_assert(kHostSlotFilter >= kNeedFilter && kHostSlotFilter % 16 == 0, "filter-only staging");

struct HostSlot {                      // one half of the double-buffered host pipeline
    hipStream_t stream = nullptr;
    hipEvent_t done = nullptr;
    uint8_t* h_in = nullptr;           // pinned: prefixes then descriptors
    uint8_t* d_in = nullptr;
    uint8_t* h_out = nullptr;          // pinned: records (AoS) | decide | verdict
    uint8_t* d_out = nullptr;
    uint32_t* d_tile = nullptr;
    bool busy = false;
    uint32_t lo = 0, cnt = 0;          // packet range of the chunk in flight
};

// bt_pcap_filter's staging buffers and streams, kept on the context between calls (bt_pcap.cpp
// allocates and sizes them; bt_destroy releases them through pcap_stage_free).
struct PcapStage;
void pcap_stage_free(PcapStage* s);

}  // namespace bt

struct bt_ctx {
    int device = 0;
    hipStream_t stream = nullptr;
    bt_opts opts{};
    int grid = 0;
    std::mutex mu;
    int spin_rc = -1;                  // hipSetDeviceFlags(hipDeviceScheduleSpin) result
    unsigned device_flags = 0;

    // the installed filter program (bt_program.cpp)
    std::vector<bt_filter_slot> slots;
    bt::DevProgram prog{};
    std::vector<uint8_t> dfa_pool;     // BT_K_PAYLOAD tables of the current program
    // the host batches' staged bytes per frame without / with records for the installed
    // program (stage_bytes / staged_bytes_locked, bt_host_batch.cpp), published by
    // install_program so that a group's split reads them without this context's lock (a host
    // batch in flight holds it)
    std::atomic<uint32_t> staged_window[2] = {{0u}, {0u}};
    // PAYLOAD DFA pools, double-buffered: a recompile writes the buffer no queued launch
    // uses. Every stream that launched a kernel reading dev[k] has its own event in
    // readers[k], recorded right after that launch; a recompile that reuses buffer k
    // waits for all of them (a single event would only cover the last stream).
    struct DfaPools {
        uint8_t* dev[2] = {nullptr, nullptr};
        std::vector<std::pair<hipStream_t, hipEvent_t>> readers[2];
        std::vector<hipEvent_t> spare;   // events of cleared reader lists, reused
        int cur = 0;
    } dfa;

    // device workspace of the compaction (bt_launch.cpp): chunk sums, and the verdict words
    // when the caller asks for none. Double-buffered (consecutive calls alternate). `last` = the
    // last stream that queued work touching the buffer (compared, never used, unless the
    // context owns it); before another stream touches it, that stream waits for `sync`:
    // recorded right after the work when `last` is a caller's stream (which may be
    // destroyed before the next touch), or at the switch when it is one of the context's
    // own streams (which live as long as the context). Calls that stay on the context's
    // streams queue no extra packets.
    struct Ws {
        uint32_t* chunk_sums = nullptr;
        uint64_t* verdict = nullptr;
        bt::PackChunkSum* pack_sums = nullptr;   // bt_pass_pack_device: chunk sums, then a word per tile
        bt::TallyPartial* tally_parts = nullptr; // bt_tally_device: one partial per chunk
        uint8_t* fan_parts = nullptr;            // bt_flow_fanout_device: fan_ws_bytes(chunks), partials then 64 words per chunk
        uint8_t* fan_queue = nullptr;            // ... and a queue byte per packet, for calls without out->queue
        hipStream_t last = nullptr;
        bool lazy = false;             // sync not recorded yet (last is a context stream)
        hipEvent_t sync = nullptr;
    };
    static constexpr int kMainDone = 8;
    struct Workspace {
        uint32_t cap = 0;
        Ws buf[2];
        int next = 0;
        // pipelined: main kernel -> compaction stream. A ring, so that an event is re-recorded
        // only long after the wait on its previous record has been consumed (re-recording one
        // of two alternating events cost ~7 us per step, profiles/r02/ab/timing_modes.txt).
        hipEvent_t main_done[kMainDone] = {};
        int md_next = 0;
        hipStream_t cstream = nullptr;     // pipelined compaction (bt_parse_filter_device_async)
    } ws;
    // The dynamic tail's counters (bt_tail_split.h; bt_launch.cpp tail_heads_for): one block of
    // kTailWords words per stream that launched a late-issue main kernel. Launches on one stream
    // never overlap, launches on two streams (a caller's own; the two output sets of the async
    // call share the main stream) never share a block. bt_stream_destroy drops its stream's
    // entry; a stream destroyed behind the context's back keeps it, and a later stream that gets
    // the same handle inherits idle counters (a handle is not reused while its work is pending).
    struct TailHeads {
        hipStream_t stream = nullptr;
        uint32_t* dev = nullptr;
        uint32_t launches = 0;   // launches that claimed from it: the next one's set is launches & 1
    };
    static constexpr size_t kTailStreams = 64;   // beyond that a new stream's launches deal statically
    std::vector<TailHeads> tail;
    const void* last_base = nullptr;   // host_resident's one-entry cache
    bool last_base_host = false;

    // bt_ring_walk_tpv3_gpu (bt_launch.cpp): the taken blocks' headers, in pinned memory the
    // kernel reads; two buffers, each reused once the walk that read it has run
    struct WalkStage {
        bt::RingBlock* h = nullptr;
        uint32_t cap = 0;
        hipEvent_t done = nullptr;
        bool used = false;
    };
    struct WalkStages {
        WalkStage stage[2];
        int next = 0;
    } walk;

    // host pipeline (bt_host_batch.cpp)
    struct HostPipe {
        uint32_t chunk = 0;
        bt::HostSlot hs[2];
        bool ready = false;
        std::atomic<int> waiters{0};      // callers waiting for `mu` to run a host batch (pipeline_share)
        uint64_t last_caller = 0;         // under mu: the last host batch's thread tag (WaitFor::thread_tag)
        uint64_t last_end = 0;            // ... and its end time in us
        bool shared_call = false;         // under mu: another thread used the context just before
    } host;
    // the host pool and its placement (bt_context.cpp)
    std::unique_ptr<bt::HostPool> pool;   // created on first use (pool_of)
    std::once_flag pool_once;
    // placement (place_ctx): the host NUMA node closest to the device and the CPUs of it this
    // process may use; the pool's workers run there when `pinned`
    int numa_node = -1;
    cpu_set_t pin{};
    bool pinned = false;

    // timing (bt_timing.cpp)
    struct Timing {
        hipEvent_t ev0 = nullptr, ev1 = nullptr;
        hipEvent_t pipe_done = nullptr;    // BT_OPT_PIPELINE: the last step's compaction
        hipEvent_t pipe_step = nullptr;    // pipelined with one output set: each step's compaction
        std::vector<hipEvent_t> tev;
    } timing;
    // bt_time_device: K steps captured once into one hipGraph, replayed per call
    struct TimingGraph {
        hipGraphExec_t exec = nullptr;
        bt_batch batch{};
        bt_outputs out{};
        uint32_t iters = 0;
    } tgraph;

    // ranges page-locked through bt_host_register (under mu): a host batch's outputs inside
    // one are copied D2H in place instead of through the pinned staging
    std::vector<std::pair<uintptr_t, uint64_t>> host_regs;

    // bt_memcpy_h2d / bt_memcpy_d2h (bt_memory.cpp): two pinned chunks, so no copy of the
    // caller's (pageable) memory goes through the runtime's own pageable-copy path
    struct Xfer {
        std::mutex mu;
        uint8_t* h[2] = {nullptr, nullptr};
        hipEvent_t ev[2] = {nullptr, nullptr};
        hipEvent_t after = nullptr;   // the compaction stream's tail (after_cstream)
    } xfer;

    // bt_extract (host lists, bt_extract_host.cpp): pinned + device staging, grown on demand
    struct ExtractStage {
        uint8_t* h = nullptr;
        uint8_t* d = nullptr;
        size_t cap = 0;
    } ex;

    // bt_pcap_filter's staging (bt_pcap.cpp owns it; pcap_stage_free releases it)
    bt::PcapStage* pcap = nullptr;
};

namespace bt {

// bt_destroy's steps, each in the unit that allocates what it frees
void release_host_pipe(bt_ctx* c);       // bt_host_batch.cpp
void release_timing_graph(bt_ctx* c);    // bt_timing.cpp
void release_workspace(bt_ctx* c);       // bt_launch.cpp
void forget_stream(bt_ctx* c, hipStream_t st);   // bt_launch.cpp
void release_dfa_pools(bt_ctx* c);       // bt_program.cpp
void release_timing(bt_ctx* c);          // bt_timing.cpp
void release_extract_stage(bt_ctx* c);   // bt_extract_host.cpp
void release_xfer(bt_ctx* c);            // bt_memory.cpp
void release_walk_stages(bt_ctx* c);     // bt_launch.cpp

// bt_context.cpp
HostPool& pool_of(bt_ctx* c);

// bt_program.cpp
int dfa_read_on(bt_ctx* c, hipStream_t st);

// bt_launch.cpp
int ensure_ws(bt_ctx* c, uint32_t n);
int take_ws(bt_ctx* c, uint32_t n, bt_ctx::Ws** w);
int ws_touch(bt_ctx* c, bt_ctx::Ws* w, hipStream_t s);
int ws_done(bt_ctx* c, bt_ctx::Ws* w, hipStream_t s);
int ensure_cstream(bt_ctx* c);
bool host_resident(bt_ctx* c, const void* base);
int check_bounds(hipStream_t st, hipStream_t cst, const char* what);
int run_device(bt_ctx* c, const bt_batch* b, const bt_outputs* o, hipStream_t st, bool aos,
               hipEvent_t e0, hipEvent_t e1, hipStream_t cst = nullptr, hipEvent_t done = nullptr);
int run_pass_pack(bt_ctx* c, const bt_batch* b, const uint64_t* select, const bt_pack_opts* po,
                  const bt_pack_out* out, hipStream_t st, hipEvent_t e0, hipEvent_t e1);

// bt_tally_host.cpp (bt_timing.cpp's bt_time_tally times the same launch)
int run_tally(bt_ctx* c, const uint8_t* decide, uint32_t n, const bt_batch* frames, const void* records, uint32_t n_cap,
              uint32_t flags, bt_tally* out, hipStream_t st, hipEvent_t e0, hipEvent_t e1);

// bt_fanout_host.cpp (bt_timing.cpp's bt_time_fanout times the same launches)
int run_fanout(bt_ctx* c, const bt_batch* frames, const uint64_t* select, const bt_fanout_opts* opts, const bt_fanout_out* out,
               hipStream_t st, hipEvent_t e0, hipEvent_t e1);

// bt_flowtab_host.cpp (bt_timing.cpp's bt_time_flow_table times the same launches)
int run_flow_table(bt_ctx* c, const bt_batch* frames, const uint64_t* select, const bt_flow_table_opts* opts, void* scratch,
                   uint64_t scratch_bytes, const bt_flow_table_out* out, hipStream_t st, hipEvent_t e0, hipEvent_t e1);

// bt_flowtrack_host.cpp (bt_timing.cpp's bt_time_flow_track times the same launches)
int run_flow_track_update(bt_ctx* c, void* state, const bt_batch* frames, const uint64_t* select, const bt_flow_track_update* upd,
                          void* scratch, uint64_t scratch_bytes, const bt_flow_track_out* out, hipStream_t st, hipEvent_t e0,
                          hipEvent_t e1);

// bt_flowtcp_host.cpp (bt_timing.cpp's bt_time_flow_tcp times the same launch)
int run_flow_tcp(bt_ctx* c, const bt_batch* frames, const uint32_t* flow_id, uint32_t table_flags, bt_flow_tcp_rec* tcp,
                 uint32_t flow_cap, bt_flow_tcp_result* result, hipStream_t st, hipEvent_t e0, hipEvent_t e1);

// bt_flowstat_host.cpp (bt_timing.cpp's bt_time_flow_stat times the same launch)
int run_flow_stat(bt_ctx* c, const bt_batch* frames, const uint32_t* flow_id, uint32_t table_flags, const bt_flow_track_update* upd,
                  bt_flow_stat_rec* stat, uint32_t flow_cap, bt_flow_stat_result* result, hipStream_t st, hipEvent_t e0, hipEvent_t e1);

// bt_flowmark_host.cpp (bt_timing.cpp's bt_time_flow_mark times the same launches)
int run_flow_mark(bt_ctx* c, const bt_batch* frames, const uint32_t* flow_id, const uint64_t* hit, const bt_flow_mark_update* upd,
                  bt_flow_mark_rec* table, uint32_t flow_cap, bt_flow_mark_result* result, hipStream_t st, hipEvent_t e0, hipEvent_t e1);
int run_flow_mark_select(bt_ctx* c, const uint32_t* flow_id, uint32_t n, const bt_flow_mark_rec* table, uint32_t flow_cap,
                         const bt_flow_mark_select_opts* opts, const uint64_t* base, uint64_t* out, bt_flow_mark_select_result* result,
                         hipStream_t st, hipEvent_t e0, hipEvent_t e1);

// bt_flowseq_host.cpp (bt_timing.cpp's bt_time_flow_seq times the same launches; ev: nullptr or five events)
int run_flow_seq(bt_ctx* c, const bt_batch* frames, const uint32_t* flow_id, const uint64_t* select, const bt_flow_seq_opts* opts,
                 bt_flow_seq_rec* table, uint32_t flow_cap, const bt_flow_seq_out* out, void* scratch, uint64_t scratch_bytes,
                 bt_flow_seq_result* result, hipStream_t st, void* const* ev);

// bt_flowstream_host.cpp (bt_timing.cpp's bt_time_flow_stream times the same launches; ev: nullptr or five events)
int run_flow_stream(bt_ctx* c, const bt_batch* frames, const uint32_t* flow_id, const uint64_t* select, uint32_t table_flags,
                    const void* pattern, const void* pattern_device, uint32_t pattern_bytes, bt_flow_stream_rec* table,
                    uint32_t flow_cap, void* scratch, uint64_t scratch_bytes, const bt_flow_stream_out* out, hipStream_t st,
                    void* const* ev);

// bt_flowtcpseq_host.cpp (bt_timing.cpp's bt_time_flow_tcpseq times the same launches; ev: nullptr or five events)
int run_flow_tcpseq(bt_ctx* c, const bt_batch* frames, const uint32_t* flow_id, const uint64_t* select, uint32_t table_flags,
                    bt_flow_tcpseq_rec* table, uint32_t flow_cap, void* scratch, uint64_t scratch_bytes, const bt_flow_tcpseq_out* out,
                    hipStream_t st, void* const* ev);

// bt_flowreasm_host.cpp (bt_timing.cpp's bt_time_flow_reasm times the same launches; ev: nullptr or seven events)
int run_flow_reasm(bt_ctx* c, const bt_batch* frames, const uint32_t* flow_id, const uint64_t* select, const int64_t* off,
                   uint32_t table_flags, const void* pattern, const void* pattern_device, uint32_t pattern_bytes,
                   bt_flow_reasm_rec* table, uint32_t flow_cap, void* scratch, uint64_t scratch_bytes, const bt_flow_reasm_out* out,
                   hipStream_t st, void* const* ev);

// bt_flowfollow_host.cpp (bt_timing.cpp's bt_time_flow_follow times the same launches; ev: nullptr or nine events)
int run_flow_follow(bt_ctx* c, const bt_batch* frames, const uint32_t* flow_id, const uint64_t* select, const int64_t* off,
                    uint32_t table_flags, const void* pattern, const void* pattern_device, uint32_t pattern_bytes,
                    bt_flow_reasm_rec* table, uint32_t flow_cap, void* scratch, uint64_t scratch_bytes, const bt_flow_reasm_out* out,
                    const bt_flow_follow_out* fo, hipStream_t st, void* const* ev);

// bt_flowtop_host.cpp (bt_timing.cpp's bt_time_flow_top times the same launches)
int run_flow_track_top(bt_ctx* c, const void* state, const bt_flow_top_opts* opts, const bt_flow_tcp_rec* tcp, void* scratch,
                       uint64_t scratch_bytes, const bt_flow_top_out* out, hipStream_t st, hipEvent_t e0, hipEvent_t e1);

// bt_flowhosts_host.cpp (bt_timing.cpp's bt_time_flow_hosts times the same launches)
int run_flow_track_hosts(bt_ctx* c, const void* state, const bt_flow_hosts_opts* opts, const bt_flow_tcp_rec* tcp, void* scratch,
                         uint64_t scratch_bytes, const bt_flow_hosts_out* out, hipStream_t st, hipEvent_t e0, hipEvent_t e1);

// bt_extract_host.cpp (bt_timing.cpp's bt_time_extract2 times the same launch)
int build_table(const bt_field_def* f, uint32_t n, ExTable* t, uint64_t* span_out, bool* never);
int run_extract(bt_ctx* c, const bt_batch* b, const ExTable& t, bool never, const bt_extract_out* o, hipStream_t st,
                hipEvent_t e0 = nullptr, hipEvent_t e1 = nullptr);

// bt_host_batch.cpp
unsigned pipeline_share(const bt_ctx* c);
void publish_staged_window(bt_ctx* c);

// The host pipeline's parallel steps for a chunk of `cnt` packets: on the pool, or for small
// chunks on the calling thread (every w in turn), where waking the pool cost more than the
// work (a 1k-packet classify took ~0.1 ms per call).
// fn(w) for w in [0, T), T = pipeline_share(c).
template <class Fn>
void pipeline_run(bt_ctx* c, uint32_t cnt, unsigned T, Fn&& fn) {
    static const uint32_t below = [] {
        const char* e = getenv("BT_HOST_INLINE_BELOW");   // A/B knob, 0 = always the pool
        return e ? (uint32_t)strtoul(e, nullptr, 10) : 8192u;
    }();
    if (cnt < below) {
        for (unsigned w = 0; w < T; ++w) fn(w);
    } else {
        c->pool->run(fn, T);
    }
}

// Counts the caller as waiting for the context until it holds the context's lock, and marks
// the call shared when another thread held the context within the last kSharedWindowUs: callers
// that spend time outside the context between their calls (building FilterResults) are not
// waiting for it at the moment a chunk starts, but they are on the host's CPUs all the same.
constexpr uint64_t kSharedWindowUs = 2000;
struct WaitFor {
    std::unique_lock<std::mutex> lk;
    bt_ctx* c;
    uint64_t me;
    static uint64_t now_us() {
        return (uint64_t)std::chrono::duration_cast<std::chrono::microseconds>(
                   std::chrono::steady_clock::now().time_since_epoch()).count();
    }
    explicit WaitFor(bt_ctx* ctx) : lk(ctx->mu, std::defer_lock), c(ctx) {
        c->host.waiters.fetch_add(1, std::memory_order_relaxed);
        lk.lock();
        c->host.waiters.fetch_sub(1, std::memory_order_relaxed);
        me = thread_tag();
        const uint64_t now = now_us();
        c->host.shared_call = c->host.last_end && c->host.last_caller != me && now - c->host.last_end < kSharedWindowUs;
    }
    ~WaitFor() {
        c->host.last_caller = me;
        c->host.last_end = now_us();
    }
    // a process-unique number per thread (a hash of std::thread::id cut to 16 bits let two
    // threads collide and look like one lone caller)
    static uint64_t thread_tag() {
        static std::atomic<uint64_t> next{1};
        thread_local const uint64_t tag = next.fetch_add(1, std::memory_order_relaxed);
        return tag;
    }
};

}  // namespace bt
