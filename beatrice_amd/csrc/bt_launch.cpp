// bt_launch.cpp — the device-resident calls: the compaction workspace and which stream
// touched it last, one parse+filter(+compaction) pass (run_device, also the host batches' and
// the timed loops' launch), the PAYLOAD resume pass, the ordered pack and the GPU ring walk.
#include <algorithm>
#include <cstdio>
#include <cstdlib>
#include <mutex>

#include "bt_ctx.h"
#include "bt_hip_util.h"
#include "bt_resume_host.h"
#include "bt_tail_split.h"

using namespace bt;

namespace {

void free_ws(bt_ctx* c) {
    for (auto& w : c->ws.buf) {
        if (w.chunk_sums) (void)hipFree(w.chunk_sums);
        if (w.verdict) (void)hipFree(w.verdict);
        if (w.pack_sums) (void)hipFree(w.pack_sums);
        if (w.tally_parts) (void)hipFree(w.tally_parts);
        if (w.fan_parts) (void)hipFree(w.fan_parts);
        if (w.fan_queue) (void)hipFree(w.fan_queue);
        w.fan_parts = nullptr;
        w.fan_queue = nullptr;
        w.pack_sums = nullptr;
        w.tally_parts = nullptr;
        w.chunk_sums = nullptr; w.verdict = nullptr; w.last = nullptr; w.lazy = false;
    }
    c->ws.cap = 0;
}

// The dynamic tail's counters of the main-kernel launches on `st` (bt_ctx::TailHeads), made on the
// stream's first such launch and zeroed on st, so before that launch; from then on each launch
// zeroes the set its successor claims from. Null, and the launch deals every tile statically,
// while st is being captured, when the table is full, or when the allocation fails.
bt_ctx::TailHeads* tail_heads_for(bt_ctx* c, hipStream_t st) {
    // a captured launch replays with the set it was captured with: static deal
    hipStreamCaptureStatus cs = hipStreamCaptureStatusNone;
    if (hipStreamIsCapturing(st, &cs) != hipSuccess || cs != hipStreamCaptureStatusNone) {
        (void)hipGetLastError();
        return nullptr;
    }
    for (auto& t : c->tail)
        if (t.stream == st) return &t;
    if (c->tail.size() >= bt_ctx::kTailStreams) return nullptr;
    uint32_t* d = nullptr;
    if (hipMalloc(&d, kTailWords * sizeof(uint32_t)) != hipSuccess ||
        hipMemsetAsync(d, 0, kTailWords * sizeof(uint32_t), st) != hipSuccess) {
        (void)hipGetLastError();
        if (d) (void)hipFree(d);
        return nullptr;
    }
    c->tail.push_back({st, d, 0u});
    return &c->tail.back();
}

bool ctx_stream(const bt_ctx* c, hipStream_t s) { return s == c->stream || (c->ws.cstream && s == c->ws.cstream); }

}  // namespace

namespace bt {

int ensure_ws(bt_ctx* c, uint32_t n) {
    if (n <= c->ws.cap && c->ws.buf[0].chunk_sums) return BT_OK;
    HIP_TRY(hipSetDevice(c->device));
    // a cached BT_OPT_GRAPH timing graph holds the pointers replaced here
    if (c->tgraph.exec) { (void)hipGraphExecDestroy(c->tgraph.exec); c->tgraph.exec = nullptr; }
    if (c->ws.buf[0].chunk_sums) HIP_TRY(hipDeviceSynchronize());   // launches on any stream may use it
    free_ws(c);
    const uint32_t ntiles = (std::max(n, 1u) + 63) / 64;
    const uint32_t nchunks = (ntiles + kChunkTiles - 1) / kChunkTiles;
    for (auto& w : c->ws.buf) {
        if (!w.sync) HIP_TRY(hipEventCreateWithFlags(&w.sync, hipEventDisableTiming));
        HIP_TRY(hipMalloc(&w.chunk_sums, (size_t)nchunks * 4));
        HIP_TRY(hipMalloc(&w.verdict, (size_t)ntiles * 8));
        HIP_TRY(hipMalloc(&w.pack_sums, (size_t)nchunks * sizeof(PackChunkSum) + (size_t)ntiles * 4));
        HIP_TRY(hipMalloc(&w.tally_parts, (size_t)nchunks * sizeof(TallyPartial)));
        HIP_TRY(hipMalloc(&w.fan_parts, fan_ws_bytes(nchunks)));
        HIP_TRY(hipMalloc(&w.fan_queue, (size_t)ntiles * 64));
    }
    for (auto& e : c->ws.main_done)
        if (!e) HIP_TRY(hipEventCreateWithFlags(&e, hipEventDisableTiming));
    c->ws.cap = ntiles * 64;
    return BT_OK;
}

// The workspace buffer of a call over n packets (consecutive calls alternate).
int take_ws(bt_ctx* c, uint32_t n, bt_ctx::Ws** w) {
    if (int rc = ensure_ws(c, n)) return rc;
    *w = &c->ws.buf[c->ws.next];
    c->ws.next ^= 1;
    return BT_OK;
}

// `s` is about to queue work that touches workspace buffer w: if another stream did last,
// s waits for everything that stream had queued on w.
int ws_touch(bt_ctx* c, bt_ctx::Ws* w, hipStream_t s) {
    if (w->last && w->last != s) {
        if (w->lazy) HIP_TRY(hipEventRecord(w->sync, w->last));   // a context stream: alive
        HIP_TRY(hipStreamWaitEvent(s, w->sync, 0));
    }
    (void)c;
    return BT_OK;
}

// `s` has just queued work touching w.
int ws_done(bt_ctx* c, bt_ctx::Ws* w, hipStream_t s) {
    w->last = s;
    w->lazy = ctx_stream(c, s);
    if (!w->lazy) HIP_TRY(hipEventRecord(w->sync, s));   // a caller's stream: record now
    return BT_OK;
}

int ensure_cstream(bt_ctx* c) {
    if (c->ws.cstream) return BT_OK;
    HIP_TRY(hipSetDevice(c->device));
    HIP_TRY(hipStreamCreateWithFlags(&c->ws.cstream, hipStreamNonBlocking));
    return BT_OK;
}

// Whether a batch's frames sit in host memory the device reads over PCIe (registered or
// pinned). One pointer query per new base (a capture ring or UMEM is one base for its life).
bool host_resident(bt_ctx* c, const void* base) {
    if (base == c->last_base) return c->last_base_host;
    hipPointerAttribute_t attr{};
    bool host = false;
    if (hipPointerGetAttributes(&attr, base) == hipSuccess) host = attr.type == hipMemoryTypeHost;
    else (void)hipGetLastError();
    c->last_base = base;
    c->last_base_host = host;
    static const bool dbg = getenv("BT_DEBUG_LEAN") != nullptr;
    if (dbg) fprintf(stderr, "[bt] batch base %p: %s memory (type %d)\n", base, host ? "host" : "device", (int)attr.type);
    return host;
}

// BT_DEBUG_BOUNDS builds: after a launch, wait and read the kernels' bounds logs
// (bt_bounds.h); a failed check becomes BT_E_INTERNAL naming the first one.
int check_bounds(hipStream_t st, hipStream_t cst, const char* what) {
#ifdef BT_DEBUG_BOUNDS
    hipStreamCaptureStatus cs = hipStreamCaptureStatusNone;
    if (hipStreamIsCapturing(st, &cs) == hipSuccess && cs != hipStreamCaptureStatusNone) return BT_OK;   // graph capture
    BoundsLog f{};
    uint32_t k = bounds_take_main(st, &f);
    if (!k && cst && cst != st) k = bounds_take_main(cst, &f);
    if (!k) k = bounds_take_extract(st, &f);
    if (!k) k = bounds_take_resume(st, &f);
    if (k) {
        fprintf(stderr, "BT_DEBUG_BOUNDS: %s: %u failed checks, first %s (site %u) block %u thread %u index %llu "
                "limit %llu\n", what, k, bounds_site_name(f.site), f.site, f.block, f.lane,
                (unsigned long long)f.index, (unsigned long long)f.limit);
        return set_error(BT_E_INTERNAL, "BT_DEBUG_BOUNDS: %s: %u failed checks, first %s index %llu limit %llu", what, k,
                         bounds_site_name(f.site), (unsigned long long)f.index, (unsigned long long)f.limit);
    }
#else
    (void)st;
    (void)cst;
    (void)what;
#endif
    return BT_OK;
}

// One parse+filter(+compaction) pass on `st`. `cst` = the stream of the compaction
// kernels: st itself, or (pipelined, bt_parse_filter_device_async) the context's
// compaction stream, which waits for this call's main kernel only, so the next call's
// main kernel on st runs beside this call's compaction; `done` (may be null) is
// recorded after the compaction on cst.
int run_device(bt_ctx* c, const bt_batch* b, const bt_outputs* o, hipStream_t st, bool aos,
               hipEvent_t e0, hipEvent_t e1, hipStream_t cst, hipEvent_t done) {
    if (!b || !o) return set_error(BT_E_INVALID_ARGUMENT, "null batch/outputs");
    MainArgs a{};
    char why[128];
    const FrameCheck bad = frame_src(b, &a, why, sizeof(why));
    if (bad == kFramesUnusable) return set_error(BT_E_INVALID_ARGUMENT, "%s", why);
    // the calling thread's current device may be another context's (a group's member threads,
    // a host driving several devices): launches, events and allocations below are this one's
    HIP_TRY(hipSetDevice(c->device));
    if (o->records && o->n_cap < b->n) return set_error(BT_E_INVALID_ARGUMENT, "records n_cap %u < n %u", o->n_cap, b->n);
    const bool filter = o->verdict || o->decide || o->pass_idx || o->n_pass;
    const bool compact = o->pass_idx || o->n_pass;
    if (!filter && !o->records) return BT_OK;
    if (!cst) cst = st;
    if (b->n == 0) {
        if (o->n_pass) HIP_TRY(hipMemsetAsync(o->n_pass, 0, 4, st));
        if (done) HIP_TRY(hipEventRecord(done, st));
        return BT_OK;
    }
    bt_ctx::Ws* w = nullptr;
    if (int rc = compact ? take_ws(c, b->n, &w) : BT_OK) return rc;
    if (bad) return set_error(BT_E_INVALID_ARGUMENT, "%s", why);
    if ((b->flags & BT_BATCH_LEAN) && o->records)
        return set_error(BT_E_INVALID_ARGUMENT, "a BT_BATCH_LEAN batch holds frame bytes 12..43 only: no records");
    a.bytes = read_limit(a.base, a.bytes);
    a.prefixes = (b->flags & (BT_BATCH_PREFIXES | BT_BATCH_LEAN)) ? 1u : 0u;
    a.n_cap = o->records ? o->n_cap : 0;
    a.records = reinterpret_cast<uint8_t*>(o->records);
    a.decide = o->decide;
    a.verdict = o->verdict ? o->verdict : (w ? w->verdict : nullptr);
    if (w && !o->verdict) { int rc = ws_touch(c, w, st); if (rc) return rc; }   // the main kernel writes w->verdict
    a.blocked = (c->opts.flags & BT_OPT_TILE_BLOCKED) ? 1u : 0u;
    // fixed stride with a filter: the late-issue kernel, which deals its last tiles by ticket
    // Lean round A for frames read over PCIe, filter-only calls: the filters and the
    // detector read bytes 12..37, so round A reads only the 16-B chunks holding them (A/Bs:
    // round 3's 46-B first round against the 64-B window, profiles/r03/e2e/lean_ab.jsonl:
    // zero-copy verdicts C3 +17 %, C4 +4..10 %, C2 +2..4 %; round 4's [12, 38) against
    // [0, 46), profiles/r04/e2e/ab_lean_lo.jsonl: C4 zero-copy and ring +3..7 %, C2 / C3
    // level). Calls that also parse would need a second round for almost every tile (the
    // walk reads to L3 + 40 B) and lost 28-39 %: not lean.
    a.lean = 0xFFFFu;
    const bool lean = b->desc && !o->records && !(c->opts.flags & BT_OPT_NO_LEAN_PCIE) && host_resident(c, b->base);
    a.dfa = c->dfa.dev[c->dfa.cur];
    a.dfa_bytes = filter ? (uint32_t)c->dfa_pool.size() : 0u;
    // Cache policy (measured): non-temporal record stores everywhere (C2 +3..9 %,
    // profiles/r01) and non-temporal header loads (descriptor mode: C3 +15 %, C4 +8 %,
    // profiles/r01; fixed stride since round 2's kernels: c2f kernel 0.349-0.358 against
    // 0.364-0.365 ms, C2 0.332-0.337 against 0.347-0.348, profiles/r02/ab/nt_loads_fixed.txt).
    // BT_OPT_CACHE_DEFAULT turns both off, BT_OPT_NT_* force them on.
    if (c->opts.flags & BT_OPT_CACHE_DEFAULT) a.nt = 0;
    else a.nt = 3u;
    // A program with a GPU PAYLOAD slot reads each frame's payload window right after its
    // header window: header loads that keep their lines in L2 save those lines a second trip
    // to HBM (C3 with /GET|POST/ first, filter-only: 0.60 against 0.92 ms; a slot that reads
    // no window, 0.33 against 0.70; tools/payload_ab.py *_cache variants)
    if (a.dfa_bytes && !(c->opts.flags & BT_OPT_NT_LOADS)) a.nt &= ~2u;
    if (c->opts.flags & BT_OPT_NT_STORES) a.nt |= 1u;
    if (c->opts.flags & BT_OPT_NT_LOADS) a.nt |= 2u;
    if (c->opts.flags & BT_OPT_WIDE_NEVER) a.nt |= 4u;
    if (c->opts.flags & BT_OPT_WIDE_ALWAYS) a.nt |= 8u;
    a.lean_lo = 0;
    if (lean && !(a.nt & 8u)) {   // frames over PCIe: lean round A, never the wide 128-B mode
        static const uint32_t lean_end = [] {   // A/B knobs: BT_LEAN_END, BT_LEAN_LO
            const char* e = getenv("BT_LEAN_END");
            return e && atoi(e) >= (int)kNeedFilter ? (uint32_t)atoi(e) : kLeanPcie;
        }();
        static const uint32_t lean_lo = [] {
            const char* e = getenv("BT_LEAN_LO");
            return e && atoi(e) >= 0 && atoi(e) <= 12 ? (uint32_t)atoi(e) : kLeanLo;
        }();
        a.lean = lean_end;
        a.lean_lo = lean_lo;
        a.nt |= 4u;
    }
    int rec = kRecNone;
    if (o->records) {
        if (aos || (c->opts.flags & BT_OPT_RECORDS_AOS)) rec = kRecAoS;
        else if (c->opts.flags & BT_OPT_RECORDS_PLANES) rec = kRecPlanes;
        else rec = kRecTiled;
    }
    // e0 / e1 time the main kernel from its own dispatch packet (no marker packets: a
    // pair of hipEventRecord around the launch left the GPU idle ~6 us each, per step)
    const bool piped = compact && cst != st;
    // pipelined: the compaction stream waits for this main kernel's end, signalled by
    // the kernel's own dispatch (e1, or main_done)
    hipEvent_t mend = e1;
    if (piped && !e1) {
        mend = c->ws.main_done[c->ws.md_next];
        c->ws.md_next = (c->ws.md_next + 1) % bt_ctx::kMainDone;
    }
    // the late-issue kernel deals its last tiles by ticket: the stream's counters, sets alternating
    if (main_deals_tail(a, rec, filter))
        if (bt_ctx::TailHeads* t = tail_heads_for(c, st)) {
            a.tail_heads = t->dev;
            a.tail_set = t->launches++ & 1u;
        }
    int rc = launch_main(a, c->prog, rec, filter, c->grid, !(c->opts.flags & BT_OPT_NO_PREFETCH), st, e0, mend);
    if (rc) return set_error(rc, "main kernel launch failed: %s", hipGetErrorString(hipGetLastError()));
    if (w && !o->verdict) { if ((rc = ws_done(c, w, st))) return rc; }
    if (a.dfa_bytes && (rc = dfa_read_on(c, st))) return rc;
    if (compact) {
        if (piped) HIP_TRY(hipStreamWaitEvent(cst, mend, 0));
        if ((rc = ws_touch(c, w, cst))) return rc;
        rc = launch_compact(a.verdict, b->n, w->chunk_sums, o->pass_idx, o->n_pass, cst);
        if (rc) return set_error(rc, "compaction launch failed");
        if ((rc = ws_done(c, w, cst))) return rc;
        if (done) HIP_TRY(hipEventRecord(done, cst));
    } else if (done) {
        HIP_TRY(hipEventRecord(done, st));
    }
    return check_bounds(st, cst, "parse+filter");
}

// The ordered pack of the selected frames (bt_pack.hip). e0 / e1: timing events recorded by
// the first / second kernel's own dispatch (bt_time_pass_pack).
int run_pass_pack(bt_ctx* c, const bt_batch* b, const uint64_t* select, const bt_pack_opts* po,
                  const bt_pack_out* out, hipStream_t st, hipEvent_t e0, hipEvent_t e1) {
    if (!c || !b || !select || !po || !out || !out->total || !out->n_packed)
        return set_error(BT_E_INVALID_ARGUMENT, "null argument");
    if (!out->bytes && out->cap) return set_error(BT_E_INVALID_ARGUMENT, "null output with cap %llu", (unsigned long long)out->cap);
    if (b->flags & (BT_BATCH_PREFIXES | BT_BATCH_LEAN))
        return set_error(BT_E_INVALID_ARGUMENT, "a BT_BATCH_PREFIXES / BT_BATCH_LEAN batch holds no whole frames to pack");
    if (po->lead > kPackLeadMax) return set_error(BT_E_INVALID_ARGUMENT, "lead %u > %u", po->lead, kPackLeadMax);
    if (po->align != 1 && po->align != 16 && po->align != 64)
        return set_error(BT_E_INVALID_ARGUMENT, "align %u (1, 16 or 64)", po->align);
    PackArgs a{};
    char why[128];
    if (frame_src(b, &a, why, sizeof(why))) return set_error(BT_E_INVALID_ARGUMENT, "%s", why);
    HIP_TRY(hipSetDevice(c->device));
    if (b->n == 0) {
        HIP_TRY(hipMemsetAsync(out->total, 0, 8, st));
        HIP_TRY(hipMemsetAsync(out->n_packed, 0, 4, st));
        return BT_OK;
    }
    bt_ctx::Ws* w = nullptr;
    int rc = take_ws(c, b->n, &w);
    if (rc) return rc;
    if ((rc = ws_touch(c, w, st))) return rc;
    a.nchunks = (a.ntiles + kPackChunkTiles - 1) / kPackChunkTiles;
    a.lead = po->lead;
    a.snap = po->snap;
    a.align = po->align;
    a.select = select;
    a.out = out->bytes;
    a.cap = out->cap;
    a.out_desc = out->desc;
    a.total = out->total;
    a.n_packed = out->n_packed;
    a.sums = w->pack_sums;
    rc = launch_pass_pack(a, st, e0, e1);
    if (rc) return set_error(rc, "pack kernel launch failed: %s", hipGetErrorString(hipGetLastError()));
    return ws_done(c, w, st);
}

void ctx_forget_base(bt_ctx* c) {
    std::lock_guard<std::mutex> lk(c->mu);
    c->last_base = nullptr;
}

void release_workspace(bt_ctx* c) {
    free_ws(c);
    for (auto& w : c->ws.buf)
        if (w.sync) (void)hipEventDestroy(w.sync);
    for (auto e : c->ws.main_done)
        if (e) (void)hipEventDestroy(e);
    if (c->ws.cstream) (void)hipStreamDestroy(c->ws.cstream);
    for (auto& t : c->tail) (void)hipFree(t.dev);
    c->tail.clear();
}

// A caller's stream is about to be destroyed (it has been synchronized): its counters go with
// it, so that a later stream with the same handle starts with its own.
void forget_stream(bt_ctx* c, hipStream_t st) {
    for (size_t i = 0; i < c->tail.size(); ++i)
        if (c->tail[i].stream == st) {
            (void)hipFree(c->tail[i].dev);
            c->tail.erase(c->tail.begin() + (long)i);
            return;
        }
}

void release_walk_stages(bt_ctx* c) {
    for (auto& w : c->walk.stage) {
        if (w.h) (void)hipHostFree(w.h);
        if (w.done) (void)hipEventDestroy(w.done);
    }
}

}  // namespace bt

extern "C" {

int bt_reserve(bt_ctx* c, uint32_t n) {
    const bt::DeviceRestore keep_device;   // the caller's current device, restored on return
    if (!c) return set_error(BT_E_INVALID_ARGUMENT, "null context");
    std::lock_guard<std::mutex> lk(c->mu);
    return ensure_ws(c, n);
}

int bt_parse_filter_device(bt_ctx* c, const bt_batch* b, const bt_outputs* o, void* stream) {
    const bt::DeviceRestore keep_device;   // the caller's current device, restored on return
    if (!c) return set_error(BT_E_INVALID_ARGUMENT, "null context");
    std::lock_guard<std::mutex> lk(c->mu);
    hipStream_t st = stream ? reinterpret_cast<hipStream_t>(stream) : c->stream;
    return run_device(c, b, o, st, false, nullptr, nullptr);
}

// The second pass over a prefix batch (bt_payload_resume.hip): the resume kernel where the
// program has a BT_K_PAYLOAD slot, then the verdict words and the pass list from the final bytes.
int bt_filter_resume_device(bt_ctx* c, const bt_batch* b, const bt_outputs* o, void* stream) {
    const bt::DeviceRestore keep_device;   // the caller's current device, restored on return
    ResumeArgs a{};
    if (const char* why = resume_args_error(c, b, o, &a)) return set_error(BT_E_INVALID_ARGUMENT, "%s", why);
    std::lock_guard<std::mutex> lk(c->mu);
    hipStream_t st = stream ? reinterpret_cast<hipStream_t>(stream) : c->stream;
    HIP_TRY(hipSetDevice(c->device));
    const bool compact = o->pass_idx || o->n_pass;
    if (b->n == 0) {
        if (o->n_pass) HIP_TRY(hipMemsetAsync(o->n_pass, 0, 4, st));
        return BT_OK;
    }
    a.bytes = read_limit(a.base, a.bytes);
    a.decide = o->decide;
    a.dfa = c->dfa.dev[c->dfa.cur];
    a.dfa_bytes = (uint32_t)c->dfa_pool.size();
    int rc = launch_payload_resume(a, c->prog, st);
    if (rc) return set_error(rc, "resume kernel launch failed: %s", hipGetErrorString(hipGetLastError()));
    if (a.dfa_bytes && (rc = dfa_read_on(c, st))) return rc;
    if (o->verdict || compact) {
        bt_ctx::Ws* w = nullptr;
        if (compact) {
            if ((rc = take_ws(c, b->n, &w))) return rc;
            if ((rc = ws_touch(c, w, st))) return rc;
        }
        uint64_t* words = o->verdict ? o->verdict : w->verdict;
        if ((rc = launch_verdict_words(o->decide, b->n, words, st))) return set_error(rc, "verdict kernel launch failed");
        if (compact) {
            rc = launch_compact(words, b->n, w->chunk_sums, o->pass_idx, o->n_pass, st);
            if (rc) return set_error(rc, "compaction launch failed");
            if ((rc = ws_done(c, w, st))) return rc;
        }
    }
    return check_bounds(st, st, "payload resume");
}

int bt_pass_pack_device(bt_ctx* c, const bt_batch* b, const uint64_t* select, const bt_pack_opts* po,
                        const bt_pack_out* out, void* stream) {
    const bt::DeviceRestore keep_device;   // the caller's current device, restored on return
    if (!c) return set_error(BT_E_INVALID_ARGUMENT, "null context");
    std::lock_guard<std::mutex> lk(c->mu);
    hipStream_t st = stream ? reinterpret_cast<hipStream_t>(stream) : c->stream;
    return run_pass_pack(c, b, select, po, out, st, nullptr, nullptr);
}

int bt_parse_filter_device_async(bt_ctx* c, const bt_batch* b, const bt_outputs* o, void* stream,
                                 void* done_event) {
    const bt::DeviceRestore keep_device;   // the caller's current device, restored on return
    if (!c) return set_error(BT_E_INVALID_ARGUMENT, "null context");
    std::lock_guard<std::mutex> lk(c->mu);
    if (int rc = ensure_cstream(c)) return rc;
    hipStream_t st = stream ? reinterpret_cast<hipStream_t>(stream) : c->stream;
    return run_device(c, b, o, st, false, nullptr, nullptr, c->ws.cstream, reinterpret_cast<hipEvent_t>(done_event));
}

int bt_ring_walk_tpv3_gpu(bt_ctx* c, const bt_tpv3_ring* ring, const void* ring_dev, uint32_t first_block,
                          uint32_t max_blocks, bt_pkt_desc* desc_dev, uint32_t cap, uint32_t* n_desc,
                          uint32_t* n_blocks_taken, uint32_t* bad_dev, void* stream) {
    const bt::DeviceRestore keep_device;   // the caller's current device, restored on return
    if (!c || !ring || !ring->base || !ring_dev || !n_desc || !n_blocks_taken || (cap && !desc_dev))
        return set_error(BT_E_INVALID_ARGUMENT, "bt_ring_walk_tpv3_gpu: null argument");
    if (!ring->n_blocks || ring->block_size < 48 || first_block >= ring->n_blocks)
        return set_error(BT_E_INVALID_ARGUMENT, "bt_ring_walk_tpv3_gpu: bad ring geometry");
    *n_desc = 0;
    *n_blocks_taken = 0;
    std::lock_guard<std::mutex> lk(c->mu);
    HIP_TRY(hipSetDevice(c->device));
    hipStream_t st = stream ? reinterpret_cast<hipStream_t>(stream) : c->stream;
    auto& w = c->walk.stage[c->walk.next];
    const uint32_t lim = std::min(max_blocks, ring->n_blocks);
    if (w.used) HIP_TRY(hipEventSynchronize(w.done));   // the walk that last read this buffer has run
    if (w.cap < lim) {
        if (w.h) HIP_TRY(hipHostFree(w.h));
        w.h = nullptr;
        HIP_TRY(hipHostMalloc(&w.h, sizeof(RingBlock) * std::max(lim, 64u), hipHostMallocDefault));
        w.cap = std::max(lim, 64u);
    }
    if (!w.done) HIP_TRY(hipEventCreateWithFlags(&w.done, hipEventDisableTiming));
    // the ready blocks and where each one's descriptors go (bt_ring.cpp's first phase)
    uint64_t total = 0;
    uint32_t nb = 0;
    for (uint32_t k = 0; k < lim; ++k) {
        const uint32_t b = (first_block + k) % ring->n_blocks;
        const uint8_t* bd = static_cast<const uint8_t*>(ring->base) + (uint64_t)b * ring->block_size;
        // tpacket_block_desc: version, offset_to_priv, then bh1 { block_status, num_pkts,
        // offset_to_first_pkt, ... } (linux/if_packet.h)
        const uint32_t status = __atomic_load_n(reinterpret_cast<const uint32_t*>(bd + 8), __ATOMIC_ACQUIRE);
        if (!(status & 1u)) break;   // TP_STATUS_USER
        const uint32_t np = *reinterpret_cast<const uint32_t*>(bd + 12);
        const uint32_t first = *reinterpret_cast<const uint32_t*>(bd + 16);
        if (total + np > cap) break;
        if (np && first >= ring->block_size)
            return set_error(BT_E_INVALID_ARGUMENT, "bt_ring_walk_tpv3_gpu: block %u: first frame outside block", b);
        w.h[nb++] = RingBlock{b, np, (uint32_t)total, first};
        total += np;
    }
    RingWalkArgs a{};
    a.ring = static_cast<const uint8_t*>(ring_dev);
    a.block_size = ring->block_size;
    a.blocks = w.h;
    a.count = nb;
    a.desc = desc_dev;
    a.cap = cap;
    a.bad = bad_dev;
    if (int rc = launch_ring_walk(a, st)) return set_error(rc, "ring walk launch failed: %s", hipGetErrorString(hipGetLastError()));
    HIP_TRY(hipEventRecord(w.done, st));
    w.used = true;
    c->walk.next ^= 1;
    *n_desc = (uint32_t)total;
    *n_blocks_taken = nb;
#ifdef BT_DEBUG_BOUNDS
    BoundsLog f{};
    if (const uint32_t k = bounds_take_ring(st, &f))
        return set_error(BT_E_INTERNAL, "BT_DEBUG_BOUNDS: ring walk: %u failed checks, first %s index %llu limit %llu", k,
                         bounds_site_name(f.site), (unsigned long long)f.index, (unsigned long long)f.limit);
#endif
    return BT_OK;
}

}  // extern "C"
