/* beatrice_gpu_bench.h — the test and benchmark side of libbeatrice_gpu.so.
 *
 * Device memory, copies and streams for hosts without a HIP toolchain (the Python tests
 * through ctypes, bench.py), and the timing loops bench.py measures the kernels with. A
 * Beatrice host integrating the stage needs only include/beatrice_gpu.h (INTEGRATION.md
 * §1); nothing here is part of the drop-in contract of SURVEY §8(b). The symbols live in the
 * same library. */
#ifndef BEATRICE_GPU_BENCH_H
#define BEATRICE_GPU_BENCH_H

#include "beatrice_gpu.h"

#ifdef __cplusplus
extern "C" {
#endif

/* ---- device memory and streams ------------------------------------------------ */
int  bt_dev_malloc(bt_ctx* ctx, uint64_t bytes, void** out);
int  bt_dev_free(bt_ctx* ctx, void* p);
int  bt_memcpy_h2d(bt_ctx* ctx, void* dst, const void* src, uint64_t bytes);
int  bt_memcpy_d2h(bt_ctx* ctx, void* dst, const void* src, uint64_t bytes);
int  bt_memset_d(bt_ctx* ctx, void* dst, int value, uint64_t bytes);
/* Caller-owned streams on the context's device (a hipStream_t, non-blocking) for the
 * `stream` arguments of bt_parse_filter_device / bt_extract_device, for hosts that cannot
 * create one themselves. Destroying a stream waits for its work. */
int  bt_stream_create(bt_ctx* ctx, void** stream);
int  bt_stream_synchronize(bt_ctx* ctx, void* stream);
int  bt_stream_destroy(bt_ctx* ctx, void* stream);
/* Timing of a device-resident run on the context stream: `iters` steps, each = the
 * main kernel between an event pair + the compaction kernels; returns the event span
 * per step and the mean main-kernel time. With BT_OPT_GRAPH the steps are captured
 * once into a hipGraph (first call per (batch, outputs, iters)) and replayed, and
 * main_ms is -1 (HIP does not time events recorded inside a graph). */
int  bt_time_device(bt_ctx* ctx, const bt_batch* batch, const bt_outputs* out,
                    uint32_t iters, float* ms_per_iter, float* main_kernel_ms);
/* The same with a breakdown of where the host's wall time goes (bench.py puts it in its
 * JSON line). The host waits by polling hipEventQuery (no interrupt wake-up): the time
 * until the first event is seen complete and from there until the last one are
 * reported separately, so a late start on the GPU and a late completion notice can be
 * told apart. */
typedef struct bt_timing {
    float span_ms;                 /* GPU: event before the first step -> after the last */
    float main_ms;                 /* mean main-kernel time (its own dispatch events)     */
    float main_min_ms, main_max_ms;
    float lead_ms;                 /* GPU: first event -> first main kernel's start       */
    float gap_ms;                  /* GPU: sum over steps of (next main start - main end) */
    double enqueue_ms;             /* host: all launches enqueued                         */
    double first_seen_ms;          /* host: enqueue done -> first event seen complete     */
    double last_seen_ms;           /* host: first event seen -> last event seen           */
    double query_ms;               /* host: elapsed-time queries                          */
    double wall_ms;                /* host: the whole call                                */
    int32_t spin_rc;               /* hipSetDeviceFlags(spin) result at bt_create, -1 unset */
    uint32_t device_flags;         /* hipGetDeviceFlags after bt_create                   */
    uint32_t reserved[6];
} bt_timing;
int  bt_time_device_ex(bt_ctx* ctx, const bt_batch* batch, const bt_outputs* out, uint32_t iters,
                       bt_timing* timing);
/* The general form. Step i writes output set out[i % n_out]. mode:
 *   BT_TIME_KERNEL_EVENTS  an event pair on every main kernel (main_ms, lead_ms, gap_ms);
 *                          recorded by the kernel's own dispatch, they cost the GPU ~9 us
 *                          per step on gfx950, so a throughput loop leaves them out and
 *                          the kernel is timed in a second call;
 *   BT_TIME_PIPELINED      the steps as bt_parse_filter_device_async (n_out = 2 keeps the
 *                          API's rule that a call's verdict buffer is not rewritten
 *                          before its compaction is done).
 * bt_time_device_ex = mode BT_TIME_KERNEL_EVENTS (| BT_TIME_PIPELINED under
 * BT_OPT_PIPELINE), n_out = 1. Without kernel events main_ms.. are -1, lead/gap 0. */
#define BT_TIME_KERNEL_EVENTS 0x1u
#define BT_TIME_PIPELINED     0x2u
int  bt_time_device2(bt_ctx* ctx, const bt_batch* batch, const bt_outputs* out, uint32_t n_out,
                     uint32_t iters, uint32_t mode, bt_timing* timing);

/* ---- timing of the ordered pack ------------------------------------------------- */
/* bt_pass_pack_device `iters` times on the context's stream; ms[i] = launch i's two kernels,
 * from an event pair recorded by their own dispatches. The outputs are those of the last launch. */
int  bt_time_pass_pack(bt_ctx* ctx, const bt_batch* frames, const uint64_t* select, const bt_pack_opts* opts,
                       const bt_pack_out* out, uint32_t iters, float* ms);
/* bt_tally_device `iters` times on the context's stream; ms[i] = launch i's two kernels, from an
 * event pair recorded by their own dispatches. *out is that of the last launch (or their sum,
 * with BT_TALLY_ACCUMULATE). */
int  bt_time_tally(bt_ctx* ctx, const uint8_t* decide, uint32_t n, const bt_batch* frames, const void* records,
                   uint32_t n_cap, uint32_t flags, bt_tally* out, uint32_t iters, float* ms);
/* What the tally replaces, `iters` times: copy_ms[i] = the n decision bytes copied to pinned host
 * memory (wall clock, the wait included), scan_ms[i] = the 16-part host scan of
 * GpuPacketFilter::scanParallel's inner loop over them on the context's host threads (up to 16).
 * counts (optional, 2 words): packets counted and passed up to the first THROW / HOST code. */
int  bt_time_tally_host(bt_ctx* ctx, const uint8_t* decide, uint32_t n, uint32_t iters, float* copy_ms,
                        float* scan_ms, uint64_t* counts);
/* bt_flow_fanout_device `iters` times on the context's stream; ms[i] = launch i's kernels (keys,
 * join and, with out->idx, scatter), from an event pair recorded by the first and the last
 * kernel's own dispatches. The outputs are those of the last launch. */
int  bt_time_fanout(bt_ctx* ctx, const bt_batch* frames, const uint64_t* select, const bt_fanout_opts* opts,
                    const bt_fanout_out* out, uint32_t iters, float* ms);
/* What the fan-out replaces, `iters` times: copy_ms[i] = the n_pass entries of the device's
 * pass_idx copied to pinned host memory (wall clock, the wait included), bucket_ms[i] =
 * bt_flow_hash_host's key and hash of every listed frame (host_base / host_desc: the batch in
 * host memory) and a stable K-way bucket of the indices, in 16 parts on the context's host
 * threads. counts (optional, 65 words): where part 0 ended in every queue's range, and the last
 * index written. */
int  bt_time_fanout_host(bt_ctx* ctx, const uint32_t* pass_idx, uint32_t n_pass, const uint8_t* host_base,
                         const bt_pkt_desc* host_desc, const bt_fanout_opts* opts, uint32_t iters, float* copy_ms,
                         float* bucket_ms, uint32_t* counts);
/* bt_flow_table_device `iters` times on the context's stream; ms[i] = launch i's kernels (keys,
 * insert, firsts, join, rank and, with out->flow_id, emit), from an event pair recorded by the
 * first and the last kernel's own dispatches. The outputs are those of the last launch. */
int  bt_time_flow_table(bt_ctx* ctx, const bt_batch* frames, const uint64_t* select, const bt_flow_table_opts* opts,
                        void* scratch, uint64_t scratch_bytes, const bt_flow_table_out* out, uint32_t iters, float* ms);
/* What the flow table replaces, `iters` times: copy_ms[i] = the n_pass entries of the device's
 * pass_idx copied to pinned host memory (wall clock, the wait included), table_ms[i] =
 * bt_flow_table_host over the listed frames (host_base[0 .. host_bytes) / host_desc: the batch
 * in host memory) on the calling thread. last (optional): the last iteration's result. */
int  bt_time_flow_table_host(bt_ctx* ctx, const uint32_t* pass_idx, uint32_t n_pass, const uint8_t* host_base,
                             uint64_t host_bytes, const bt_pkt_desc* host_desc, const bt_flow_table_opts* opts,
                             uint32_t iters, float* copy_ms, float* table_ms, bt_flow_table_result* last);
/* bt_flow_track_update_device `iters` times on the context's stream into the same state; ms[i] =
 * call i's kernels (the per-batch table's and find, join, apply and, with out->flow_id, ids), from
 * an event pair recorded by the first and the last kernel's own dispatches. Every call merges the
 * batch again: from the second on, every flow of it is found. */
int  bt_time_flow_track(bt_ctx* ctx, void* state, const bt_batch* frames, const uint64_t* select,
                        const bt_flow_track_update* upd, void* scratch, uint64_t scratch_bytes,
                        const bt_flow_track_out* out, uint32_t iters, float* ms);
/* bt_flow_tcp_update_device `iters` times on the context's stream into the same side table; ms[i] =
 * call i's kernel, from an event pair recorded by its own dispatch (the 32-byte memset of *result
 * in front of it is outside the pair). From the second call on every flag bit is already set. */
int  bt_time_flow_tcp(bt_ctx* ctx, const bt_batch* frames, const uint32_t* flow_id, uint32_t table_flags,
                      bt_flow_tcp_rec* tcp, uint32_t flow_cap, bt_flow_tcp_result* result, uint32_t iters, float* ms);
/* bt_flow_stat_update_device `iters` times on the context's stream into the same side table; ms[i] =
 * call i's kernel, from an event pair recorded by its own dispatch (the 32-byte memset of *result
 * in front of it is outside the pair). From the second call on every OR and maximum is already there. */
int  bt_time_flow_stat(bt_ctx* ctx, const bt_batch* frames, const uint32_t* flow_id, uint32_t table_flags,
                       const bt_flow_track_update* upd, bt_flow_stat_rec* stat, uint32_t flow_cap,
                       bt_flow_stat_result* result, uint32_t iters, float* ms);
/* With update_ms: bt_flow_mark_update_device `iters` times on the context's stream into the same
 * mark table; with select_ms, after those: bt_flow_mark_select_device `iters` times over that table.
 * ms[i] = call i's kernel, from an event pair recorded by its own dispatch (the 32-byte memset of
 * the result in front of it is outside the pair). From the second update on every mark bit and
 * stamp is already there. Either of update_ms / select_ms may be NULL; its arguments are then unused. */
int  bt_time_flow_mark(bt_ctx* ctx, const bt_batch* frames, const uint32_t* flow_id, const uint64_t* hit,
                       const bt_flow_mark_update* upd, bt_flow_mark_rec* mark_table, uint32_t flow_cap,
                       bt_flow_mark_result* result, const bt_flow_mark_select_opts* opts, const uint64_t* base,
                       uint64_t* out_select, bt_flow_mark_select_result* sel_result, uint32_t iters,
                       float* update_ms, float* select_ms);
/* bt_flow_seq_device `iters` times on the context's stream into the same table (which keeps growing)
 * and the same scratch; ms[i] = call i's kernels, from the first one's start to the last one's end,
 * events recorded by the kernels' own dispatches (the 64-byte memset of *result in front is outside).
 * phase_ms (optional, 4 * iters): call i's compaction, sort (every pass; 0 without one), segmented
 * scan and emit + table update, in that order, between the starts of their first kernels. */
int  bt_time_flow_seq(bt_ctx* ctx, const bt_batch* frames, const uint32_t* flow_id, const uint64_t* select,
                      const bt_flow_seq_opts* opts, bt_flow_seq_rec* table, uint32_t flow_cap, const bt_flow_seq_out* out,
                      void* scratch, uint64_t scratch_bytes, bt_flow_seq_result* result, uint32_t iters, float* ms,
                      float* phase_ms);
/* bt_flow_stream_device `iters` times on the context's stream into the same table (whose streams keep
 * growing) and the same scratch; ms[i] = call i's kernels, from the first one's start to the last
 * one's end, events recorded by the kernels' own dispatches (the two memsets in front are outside).
 * phase_ms (optional, 4 * iters): call i's classification + compaction, sort (every pass), link +
 * match, and commit, in that order. */
int  bt_time_flow_stream(bt_ctx* ctx, const bt_batch* frames, const uint32_t* flow_id, const uint64_t* select,
                         uint32_t table_flags, const void* pattern, const void* pattern_device, uint32_t pattern_bytes,
                         bt_flow_stream_rec* table, uint32_t flow_cap, void* scratch, uint64_t scratch_bytes,
                         const bt_flow_stream_out* out, uint32_t iters, float* ms, float* phase_ms);
/* bt_flow_tcpseq_device `iters` times on the context's stream into the same table (a direction's
 * segments meet what the earlier calls saw: with one packet per direction all are OLD from the
 * second call on) and the same scratch; ms[i] = call i's kernels, from the first one's start
 * to the last one's end, events recorded by the kernels' own dispatches (the memset in front is
 * outside). phase_ms (optional, 4 * iters): call i's classification + compaction, sort (every pass),
 * carry scan + join, and emit + commit, in that order. */
int  bt_time_flow_tcpseq(bt_ctx* ctx, const bt_batch* frames, const uint32_t* flow_id, const uint64_t* select,
                         uint32_t table_flags, bt_flow_tcpseq_rec* table, uint32_t flow_cap, void* scratch,
                         uint64_t scratch_bytes, const bt_flow_tcpseq_out* out, uint32_t iters, float* ms, float* phase_ms);
/* bt_flow_reasm_device `iters` times on the context's stream into the same table (from the second
 * call on every segment lies below `next`: late) and the same scratch; ms[i] = call i's kernels, from
 * the first one's start to the last one's end, events recorded by the kernels' own dispatches (the
 * two memsets in front are outside). phase_ms (optional, 6 * iters): call i's classification +
 * compaction, first sort (4 passes, by position), rekey + second sort (by flow and direction), carry
 * scan + join + emit, match, and commit, in that order. */
int  bt_time_flow_reasm(bt_ctx* ctx, const bt_batch* frames, const uint32_t* flow_id, const uint64_t* select, const int64_t* off,
                        uint32_t table_flags, const void* pattern, const void* pattern_device, uint32_t pattern_bytes,
                        bt_flow_reasm_rec* table, uint32_t flow_cap, void* scratch, uint64_t scratch_bytes,
                        const bt_flow_reasm_out* out, uint32_t iters, float* ms, float* phase_ms);
/* bt_flow_follow_device `iters` times on the context's stream into the same table and the same
 * scratch and outputs (zero the table between launches by calling with iters = 1); ms[i] = call i's
 * kernels, from the first one's start to the last one's end (the memsets in front are outside, those
 * of the no-pattern mode inside). phase_ms (optional, 8 * iters): call i's classification +
 * compaction, first sort, rekey + second sort, carry scan + join + emit, match (without a pattern:
 * the memsets that stand in for it), the follow's sums + join + emit + runs, its copy, and commit,
 * in that order. */
int  bt_time_flow_follow(bt_ctx* ctx, const bt_batch* frames, const uint32_t* flow_id, const uint64_t* select, const int64_t* off,
                         uint32_t table_flags, const void* pattern, const void* pattern_device, uint32_t pattern_bytes,
                         bt_flow_reasm_rec* table, uint32_t flow_cap, void* scratch, uint64_t scratch_bytes,
                         const bt_flow_reasm_out* out, const bt_flow_follow_out* fo, uint32_t iters, float* ms, float* phase_ms);
/* What the tracker replaces, `iters` times: copy_ms[i] = the n_flows records of a per-batch table
 * (flows, on the device) copied to pinned host memory (wall clock, the wait included), merge_ms[i]
 * = those records merged into the host tracker state at host_state (bt_flow_track_init_host's) on
 * the calling thread, every flow stamped batch_ts. last (optional): the last merge's result. */
int  bt_time_flow_track_host(bt_ctx* ctx, const bt_flow_rec* flows, uint32_t n_flows, void* host_state,
                             uint64_t state_bytes, uint64_t batch_ts, uint32_t iters, float* copy_ms, float* merge_ms,
                             bt_flow_track_result* last);
/* bt_flow_track_top_device `iters` times on the context's stream over the same state; ms[i] = call
 * i's kernels, from an event pair recorded by the first and the last kernel's own dispatches. */
int  bt_time_flow_top(bt_ctx* ctx, const void* state, const bt_flow_top_opts* opts, const bt_flow_tcp_rec* tcp,
                      void* scratch, uint64_t scratch_bytes, const bt_flow_top_out* out, uint32_t iters, float* ms);
/* What the top-K query replaces, `iters` times: copy_ms[i] = the n_flows records of a tracker
 * (recs, on the device) copied to pinned host memory (wall clock, the wait included), sort_ms[i] =
 * a std::partial_sort of them by (bytes descending, flow number ascending) for the first k on the
 * calling thread. top_total (optional): the sum of the last top's values. */
int  bt_time_flow_top_host(bt_ctx* ctx, const bt_flow_track_rec* recs, uint32_t n_flows, uint32_t k, uint32_t iters,
                           float* copy_ms, float* sort_ms, uint64_t* top_total);
/* bt_flow_track_hosts_device `iters` times on the context's stream over the same state; ms[i] =
 * call i's kernels, from an event pair recorded by the first and the last kernel's own dispatches. */
int  bt_time_flow_hosts(bt_ctx* ctx, const void* state, const bt_flow_hosts_opts* opts, const bt_flow_tcp_rec* tcp,
                        void* scratch, uint64_t scratch_bytes, const bt_flow_hosts_out* out, uint32_t iters, float* ms);
/* What the endpoint table replaces, `iters` times: copy_ms[i] = the header and the first n_flows
 * records of the tracker at `state` (on the device, known to the process) and, with tcp, its
 * n_flows side records copied to pinned host memory (wall clock, the wait included); group_ms[i] =
 * bt_flow_track_hosts_host over them on the calling thread, into host_cap records and no
 * endpoint_host. last (optional): the last result. sums (optional, six u64, mod 2^64) over the
 * n_written records of the last run: packets[0]; packets[1]; bytes[0] ^ bytes[1]; flows[0] +
 * flows[1]; tcp_state[j] * (j + 1) over j; first_ts ^ last_ts ^ (first_flow << 32 | syn_packets). */
int  bt_time_flow_hosts_host(bt_ctx* ctx, const void* state, uint32_t n_flows, const bt_flow_tcp_rec* tcp,
                             const bt_flow_hosts_opts* opts, uint32_t iters, float* copy_ms, float* group_ms,
                             bt_flow_hosts_result* last, uint64_t* sums);
/* A device-to-device hipMemcpyAsync of `bytes` on the context's stream, `iters` times, each
 * between an event pair: the ceiling for moving that many bytes on the device. */
int  bt_time_copy_d2d(bt_ctx* ctx, void* dst, const void* src, uint64_t bytes, uint32_t iters, float* ms);

/* ---- timing of the user-protocol extractor ------------------------------------- */
/* bt_extract_device `iters` times on the context's stream, each launch timed by an event
 * pair from its own dispatch packet (bt_timing.main_* = the extraction kernel). For
 * benchmarks; the outputs are those of the last launch. BT_E_INVALID_ARGUMENT for an empty
 * batch or a table whose span no frame can reach (nothing would launch). */
int  bt_time_extract_ex(bt_ctx* ctx, const bt_batch* batch, const bt_field_def* fields, uint32_t n_fields,
                        const bt_extract_out* out, uint32_t iters, bt_timing* timing);
/* The same with a mode (BT_TIME_KERNEL_EVENTS only; without it main_ms.. are -1). */
int  bt_time_extract2(bt_ctx* ctx, const bt_batch* batch, const bt_field_def* fields, uint32_t n_fields,
                      const bt_extract_out* out, uint32_t iters, uint32_t mode, bt_timing* timing);

/* ---- host helpers the tests, tools and bench use (moved from beatrice_gpu.h: not part of
 * the drop-in contract INTEGRATION.md binds) ---------------------------------------- */
/* Host-only helpers: the CPUs of NUMA node `node` this process may use (*n = 0 if none or
 * unknown; at most cap written), and the CPUs it may use at all (affinity set bounded by
 * the cgroup v2 quota). */
int  bt_node_cpus(int node, int32_t* cpus, uint32_t cap, uint32_t* n);
/* host-only helper: compile without a context (no device needed) */
int  bt_filter_compile_host(const bt_filter_desc* filters, uint32_t n,
                            bt_filter_slot* out, uint32_t cap, uint32_t* n_slots);
/* ---- PAYLOAD filters on the GPU ---------------------------------
 * Replaces the per-packet std::regex construction + regex_search of
 * PacketFilter::applyPayloadFilter (src/PacketFilter.cpp:288-321) for the regular
 * subset of libstdc++'s ECMAScript grammar: the expression is compiled once to a byte
 * DFA that the kernel runs over the same <= 100-byte window after the IPv4 header.
 * bt_filter_compile does this for every PAYLOAD filter it can (BT_K_PAYLOAD slots, up
 * to 16 KiB of tables per program); the rest stay BT_K_HOST. By default \b \B, POSIX
 * bracket classes and DFAs of more than 254 live states are among the rest;
 * BT_DFA_EXTENDED below (BT_OPT_PAYLOAD_EXTENDED on a context) takes them too. The helpers below expose
 * the compiler and a host executor of the same DFA (tests, other hosts).
 *   bt_payload_dfa_compile  BT_OK (+ blob; blob == NULL: size only),
 *                           BT_E_INVALID_ARGUMENT if std::regex rejects the expression
 *                           (the reference's filter is then always false),
 *                           BT_E_NOT_IMPLEMENTED outside the modelled subset / too big,
 *                           BT_E_RESOURCE if cap is too small.
 *   bt_payload_dfa_search   regex_search(string(s, n), regex(expr)) for a compiled expr
 *   bt_payload_dfa_eval     applyPayloadFilter(frame, len) for a non-empty expression */
int  bt_payload_dfa_compile(const char* expression, void* blob, uint32_t cap, uint32_t* size);
/* The same with options: BT_DFA_NO_PAIRS leaves out the optional two-byte table (the
 * compiler adds it when it is <= 4 KiB; the filter compiler drops it when a program's
 * tables would not fit the 16 KiB pool otherwise). */
#define BT_DFA_NO_PAIRS 0x1u
/* BT_DFA_NO_BITPAR: always the DFA, never the bit-parallel form the compiler prefers for
 * unions of linear class sequences (A/B and tests; blob layouts in bt_regex_dfa.cpp). */
#define BT_DFA_NO_BITPAR 0x2u
/* BT_DFA_EXTENDED: the wider subset — \b and \B (one bit of previous-byte word class in the
 * DFA state), POSIX classes inside brackets ([[:alpha:]] .. [[:xdigit:]], [[:d:]] [[:w:]]
 * [[:s:]]; C locale) and DFAs of up to 4,096 states (more than 254 live states: the wide
 * blob with 16-bit state ids, when it fits 16 KiB). Backreferences, lookaheads, \c \u,
 * [[.x.]] and [[=x=]] still return BT_E_NOT_IMPLEMENTED. A pattern the default subset takes
 * compiles to the same bytes with the flag. bt_filter_compile sets it for contexts created
 * with BT_OPT_PAYLOAD_EXTENDED. */
#define BT_DFA_EXTENDED 0x4u
int  bt_payload_dfa_compile_ex(const char* expression, uint32_t flags, void* blob, uint32_t cap, uint32_t* size);
int  bt_payload_dfa_search(const void* blob, const uint8_t* s, uint32_t n);
/* The same walk, and each frame's header prefix is also copied into slot i of `slots`
 * (BT_PREFIX_SLOT bytes per frame, slot i at i * BT_PREFIX_SLOT): the bytes the layer walk
 * and the built-in filters read, i.e. max(38, the walked header end) rounded up to 16, at
 * most the frame. desc[i] = BT_DESC(i * BT_PREFIX_SLOT, min(tp_snaplen, 65535)). A batch
 * over `slots` (registered, or copied to the device) with flags = BT_BATCH_PREFIXES then
 * reads one aligned 64-B host line per packet over PCIe for headers up to 64 B, instead
 * of a window straddling the ring's 2-mod-16 frame starts. The walker copies while its
 * chains are in flight, one frame behind each chain's header read. */
int  bt_ring_gather_tpv3(bt_ctx* ctx, const bt_tpv3_ring* ring, uint32_t first_block, uint32_t max_blocks,
                         uint8_t* slots, bt_pkt_desc* desc, uint32_t cap, uint32_t* n_desc,
                         uint32_t* n_blocks_taken);
/* The walk with the frame chains followed on the GPU. The host reads only the taken blocks'
 * headers (block_status, num_pkts, offset_to_first_pkt: one line per block) and a kernel on
 * `stream` walks every chain through ring_dev (the ring's device-visible alias, e.g. from
 * bt_host_register), one lane per block, writing the descriptors (as bt_ring_walk_tpv3
 * does) into desc_dev, device memory of cap entries. *n_desc and *n_blocks_taken are known
 * on return, the descriptors once the stream has run the kernel; batches on the same
 * stream that read desc_dev follow it in order. A chain that leaves its block makes that
 * block's remaining descriptors empty (length 0: nothing of them is read) and stores
 * block + 1 into *bad_dev (device memory, optional; the largest such block wins). */
int  bt_ring_walk_tpv3_gpu(bt_ctx* ctx, const bt_tpv3_ring* ring, const void* ring_dev, uint32_t first_block,
                           uint32_t max_blocks, bt_pkt_desc* desc_dev, uint32_t cap, uint32_t* n_desc,
                           uint32_t* n_blocks_taken, uint32_t* bad_dev, void* stream);
/* The split (host only): bounds[0..parts] with bounds[0] = 0, bounds[parts] = n, every
 * inner bound a multiple of 64, member k taking [bounds[k], bounds[k+1]); balanced by the
 * cost min(len, 128) + 8 + 96 bytes per packet (beatrice_amd/shard.py:shard_bounds). */
int      bt_group_split(const uint32_t* lens, uint32_t n, uint32_t parts, uint32_t* bounds);
/* The same with a cost model: packet cost = round_up(min(len, window), align) + fixed.
 * The group's calls weigh packets by what each call moves (bt_group_cost). */
typedef struct bt_split_cost {
    uint32_t window;               /* bytes of each frame the call reads / stages         */
    uint32_t align;                /* ... rounded up to this (1 = exact)                  */
    uint32_t fixed;                /* per-packet bytes independent of the length          */
    uint32_t reserved;
} bt_split_cost;
int      bt_group_split_cost(const uint32_t* lens, uint32_t n, uint32_t parts, const bt_split_cost* cost,
                             uint32_t* bounds);
/* The split the group's calls use: bt_group_split_cost up to 4096 tiles; above, the cost of
 * one tile in every S (~4096 samples) stands for its run of S tiles and the cuts interpolate
 * within a run (an exact pass over 16M descriptors took ~45 ms on one thread before any
 * member started). Same form of bounds. */
int      bt_group_split_plan(const uint32_t* lens, uint32_t n, uint32_t parts, const bt_split_cost* cost,
                             uint32_t* bounds);
/* The cost model a group call uses (mapped: bt_group_parse_filter_mapped, else the host
 * batches), for a call that asks for records / filter outputs, with desc_bytes-byte
 * descriptors (8 packed, 16 xdp_desc, 0 fixed stride):
 *   host batches: window = the bytes staged per frame (32: a filter-only call stages frame
 *                 bytes 12..43; 112 with records; 176 with a GPU PAYLOAD slot), align 16,
 *                 fixed = desc_bytes + 96 (records, bt_rec D2H) + 1 (decision D2H)
 *   mapped:       window = 128 with records (the walk's wide window) else 48 (the lean
 *                 first round reads frame bytes 12..37: two or three 16-B chunks by the
 *                 frame's alignment, 32 B + one chunk of slack), align 16, fixed =
 *                 desc_bytes + 64 (records: packed slabs) + 1 (decision) — all of it PCIe
 *                 traffic of the member's link. */
int      bt_group_cost(bt_group* group, int mapped, int records, int filters, uint32_t desc_bytes,
                       bt_split_cost* out);
/* Host threads per member: `requested` (opts.host_threads, else BT_HOST_THREADS; 0 = auto)
 * is the whole group's budget, split evenly (at least 1, at most 16 each); auto gives each
 * member usable / members, at least 1 and at most 16 (one context alone: min(16, usable), the
 * single-context default; a context's host pipeline takes at most 8 of them while other callers
 * wait for the context). Host only; bt_group_create applies it. */
int      bt_group_thread_budget(uint32_t members, uint32_t usable, uint32_t requested, uint32_t* per_member);
void bt_record_gather_planes(const void* planes, uint32_t n_cap, uint32_t i, bt_rec* out);
/* Slabs the packed device form of this record occupies (2..6). */
uint32_t bt_record_slabs(const bt_rec* r);

/* ---- registered host pages (diagnostics) ---------------------------------------
 * bt_host_register and bt_group_host_register keep one process-wide table of the whole
 * pages they registered (beatrice_amd/csrc/bt_pin.h): lo_hi_refs[3 i .. 3 i + 2] = span i's
 * first byte, end (both page-aligned) and reference count, ascending, for up to cap spans;
 * *n = the number of live spans. Host only (no device call). */
int  bt_host_pins(uint64_t* lo_hi_refs, uint32_t cap, uint32_t* n);
/* Device `device`'s alias of [host, host + bytes), which must lie inside one registered span
 * (BT_E_INVALID_ARGUMENT otherwise): what the kernels of a mapped call read it through. */
int  bt_host_alias(const void* host, uint64_t bytes, int device, void** alias);

#ifdef __cplusplus
}
#endif

#endif /* BEATRICE_GPU_BENCH_H */
