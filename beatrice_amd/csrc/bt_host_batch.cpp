// bt_host_batch.cpp — batches of frames in host memory (bt_parse_filter,
// bt_parse_filter_ptrs): two streams + pinned staging, the gather of each frame's staged
// prefix on the context's host pool, run_device per chunk, and the drain into the caller's
// buffers, double-buffered so that one chunk's gather runs beside the other's device work.
#include <algorithm>
#include <cstdlib>
#include <cstring>
#include <mutex>
#include <vector>

#include "bt_ctx.h"
#include "bt_hip_util.h"

using namespace bt;

namespace {

size_t in_bytes(uint32_t chunk) { return (size_t)chunk * kHostSlotPayload + (size_t)chunk * 8; }
size_t out_bytes(uint32_t chunk) { return (size_t)chunk * BT_REC_BYTES + chunk + ((size_t)chunk + 63) / 64 * 8; }

int ensure_host(bt_ctx* c) {
    if (c->host.ready) return BT_OK;
    HIP_TRY(hipSetDevice(c->device));
    static const uint32_t default_chunk = [] {   // BT_HOST_CHUNK: A/B knob for the default
        const char* e = getenv("BT_HOST_CHUNK");
        return e && atoi(e) >= 64 ? (uint32_t)atoi(e) : (1u << 20);
    }();
    uint32_t chunk = c->opts.host_chunk_packets ? c->opts.host_chunk_packets : default_chunk;
    chunk = (chunk + 63) / 64 * 64;
    c->host.chunk = chunk;
    (void)pool_of(c);
    for (auto& s : c->host.hs) {
        HIP_TRY(hipStreamCreateWithFlags(&s.stream, hipStreamNonBlocking));
        HIP_TRY(hipEventCreateWithFlags(&s.done, hipEventDisableTiming));
        HIP_TRY(hipHostMalloc(&s.h_in, in_bytes(chunk), hipHostMallocDefault));
        HIP_TRY(hipHostMalloc(&s.h_out, out_bytes(chunk), hipHostMallocDefault));
        HIP_TRY(hipMalloc(&s.d_in, in_bytes(chunk)));
        HIP_TRY(hipMalloc(&s.d_out, out_bytes(chunk)));
    }
    c->host.ready = true;
    return BT_OK;
}

// One frame's staged prefix: m bytes of src to dst (16-B aligned, its slot rounded up to 16).
// With `nt`, whole 16-B chunks go out as non-temporal stores (no read-for-ownership of the
// staging lines, which only the DMA engine reads next); the tail chunk is assembled from the
// frame's last bytes, never read past them. The caller fences (sfence) before the copy's
// consumer runs.
typedef long long v2i64 __attribute__((vector_size(16)));
inline void stage_prefix(uint8_t* dst, const uint8_t* src, uint32_t m, bool nt) {
    if (!nt) {
        std::memcpy(dst, src, m);
        return;
    }
    uint32_t k = 0;
    for (; k + 16 <= m; k += 16) {
        v2i64 x;
        std::memcpy(&x, src + k, 16);
        __builtin_nontemporal_store(x, reinterpret_cast<v2i64*>(dst + k));
    }
    if (k < m) {
        v2i64 x{};
        std::memcpy(&x, src + k, m - k);
        __builtin_nontemporal_store(x, reinterpret_cast<v2i64*>(dst + k));
    }
}

// Copies one finished chunk from pinned staging into the caller's buffers.
void drain_slot(bt_ctx* c, HostSlot& s, bt_rec* records, uint64_t* verdict, uint8_t* decide) {
    const uint32_t chunk = c->host.chunk;
    const uint8_t* rec = s.h_out;
    const uint8_t* dec = s.h_out + (size_t)chunk * BT_REC_BYTES;
    const uint64_t* ver = reinterpret_cast<const uint64_t*>(dec + chunk);
    const unsigned T = pipeline_share(c);
    const uint32_t lo = s.lo, cnt = s.cnt;
    static const bool drain_nt = [] {   // A/B knob: BT_DRAIN_NT=1 streams the records out
        const char* e = getenv("BT_DRAIN_NT");
        return e && atoi(e) != 0;
    }();
    pipeline_run(c, cnt, T, [&](unsigned w) {   // split on 64-packet boundaries
        const uint32_t tiles = (cnt + 63) / 64;
        const uint32_t t0 = (uint32_t)((uint64_t)tiles * w / T), t1 = (uint32_t)((uint64_t)tiles * (w + 1) / T);
        const uint32_t a = t0 * 64, b = std::min(cnt, t1 * 64);
        if (a >= b) return;
        if (records) {
            uint8_t* dst = reinterpret_cast<uint8_t*>(records + lo + a);
            const uint8_t* src = rec + (size_t)a * BT_REC_BYTES;
            const size_t bytes = (size_t)(b - a) * BT_REC_BYTES;   // a multiple of 16
            if (drain_nt && ((uintptr_t)dst & 15u) == 0) {   // the caller's records: not read back here
                for (size_t k = 0; k < bytes; k += 16)
                    __builtin_nontemporal_store(*reinterpret_cast<const v2i64*>(src + k), reinterpret_cast<v2i64*>(dst + k));
                __builtin_ia32_sfence();
            } else {
                std::memcpy(dst, src, bytes);
            }
        }
        if (decide) std::memcpy(decide + lo + a, dec + a, b - a);
        if (verdict) std::memcpy(verdict + (lo + a) / 64, ver + a / 64, (size_t)(t1 - t0) * 8);
    });
    s.busy = false;
}

// Bytes of each frame the host pipeline reads (bt_host_stage_bytes): the walk's 112 with
// records; the filters' 38 B (as 48; bytes 12..43 of them staged) for filter-only calls, whose
// kernels take no second round (staging the walk's 112 B took 2-3x the gather and the copy for IMIX frames); the
// payload window with a GPU PAYLOAD slot (bytes past the staged prefix would be the next
// frame's).
uint32_t stage_bytes(const bt_ctx* c, bool records) {
    return !c->dfa_pool.empty() ? kHostSlotPayload : records ? kHostSlot : kHostSlotFilter;
}

}  // namespace

namespace bt {

void release_host_pipe(bt_ctx* c) {
    for (auto& s : c->host.hs) {
        if (s.stream) (void)hipStreamDestroy(s.stream);
        if (s.done) (void)hipEventDestroy(s.done);
        if (s.h_in) (void)hipHostFree(s.h_in);
        if (s.h_out) (void)hipHostFree(s.h_out);
        if (s.d_in) (void)hipFree(s.d_in);
        if (s.d_out) (void)hipFree(s.d_out);
        if (s.d_tile) (void)hipFree(s.d_tile);
        s = HostSlot{};
    }
    c->host.ready = false;
}

// How much of the pool one chunk's gather / drain uses: all of it, or, while other callers
// wait for this context, at most kSharedPool threads. A lone caller then gets every pool thread
// (host-gather e2e with 16 of a 16-CPU host's: C4 349-408 -> 515-535 Mpps), while callers on
// every CPU (T callers of one GpuPacketFilter) keep to the share that does not oversubscribe
// them (16 callers lost 10-25 % with a 16-thread pool, profiles/r04/surfaces/ab_pool_8_16.jsonl).
constexpr unsigned kSharedPool = 8;
unsigned pipeline_share(const bt_ctx* c) {
    const unsigned T = c->pool->size();
    const bool shared = c->host.waiters.load(std::memory_order_relaxed) > 0 || c->host.shared_call;
    return shared ? std::min(T, kSharedPool) : T;
}

uint32_t staged_bytes_locked(const bt_ctx* c, bool records) {
    const uint32_t w = stage_bytes(c, records);
    return w == kHostSlotFilter && !(c->opts.flags & BT_OPT_NO_LEAN_HOST) ? kHostLeanWidth : w;
}
void publish_staged_window(bt_ctx* c) {   // under c->mu, after the program changed
    for (int r = 0; r < 2; ++r) c->staged_window[r].store(staged_bytes_locked(c, r != 0), std::memory_order_release);
}
uint32_t staged_window(const bt_ctx* c, bool records) {
    return c->staged_window[records ? 1 : 0].load(std::memory_order_acquire);
}

}  // namespace bt

namespace {

// Host batch pipeline shared by bt_parse_filter (base + descriptors) and
// bt_parse_filter_ptrs (one pointer per frame): frame(i, &len) returns frame i.
template <class FrameFn>
int host_pipeline_run(bt_ctx* c, uint32_t n, FrameFn frame, bt_rec* records, uint64_t* verdict, uint8_t* decide,
                  uint32_t* pass_idx, uint32_t* n_pass) {
    int rc = ensure_host(c);
    if (rc) return rc;
    HIP_TRY(hipSetDevice(c->device));   // the calling thread may last have driven another device
    const bool want_filter = verdict || decide || pass_idx || n_pass;
    // pass indices come from the verdict words; keep a private copy when the caller
    // did not ask for them
    std::vector<uint64_t> vtmp;
    uint64_t* ver = verdict;
    if (!ver && (pass_idx || n_pass)) { vtmp.resize(((size_t)n + 63) / 64); ver = vtmp.data(); }

    const uint32_t chunk = c->host.chunk;
    // Records inside a range registered with bt_host_register are copied D2H in place, each
    // chunk at its offset, and skip the drain (96 B of staging-to-caller copy per packet, most
    // of the host's memory traffic with records: e2e records + verdicts C2 / C3 / C4 +1..17 /
    // +17..22 / +8..15 %, profiles/r05/e2e/ab_registered_outputs.jsonl). Decisions and verdict
    // words keep the staging (the same A/B moved them in place: C2 -3..+32 %, C3 -8..-28 %, C4
    // -4..-7 %).
    auto registered = [c](const void* p, size_t bytes) {
        const uintptr_t a = (uintptr_t)p;
        for (const auto& r : c->host_regs)
            if (a >= r.first && a + bytes <= r.first + r.second) return true;
        return false;
    };
    const bool rec_direct = records && registered(records, (size_t)n * BT_REC_BYTES);
    bt_rec* const rec_drain = rec_direct ? nullptr : records;
    // bytes staged per frame: the header walk's, or with a GPU PAYLOAD slot in the program
    // the payload window's too (bytes past the staged prefix would be the next frame's)
    const uint32_t slot = stage_bytes(c, records != nullptr);
    // Filter-only calls (no records, no GPU PAYLOAD slot) stage only frame bytes [12, 44): the
    // filters read 12..37 and such calls take no second round. Each frame's descriptor then
    // points 12 B before its staged bytes (the buffer starts with a 16-B pad, so no offset is
    // negative); bytes 0..11 of that window are the previous slot's, which nothing reads.
    const bool lean = slot == kHostSlotFilter && !(c->opts.flags & BT_OPT_NO_LEAN_HOST);
    const uint32_t lo = lean ? kLeanLo : 0u;
    const uint32_t width = lean ? kHostLeanWidth : slot;
    const uint32_t pad = lean ? 16u : 0u;
    static const bool prefetch = getenv("BT_NO_GATHER_PREFETCH") == nullptr;   // A/B knobs
    // non-temporal staging stores (BT_GATHER_NT=0: plain copies). Same-box A/B, 5 pairs over
    // two boxes (profiles/r04/e2e/ab_gather_nt*.jsonl): C2 verdicts +2..+34 % in every pair,
    // C4 +8 % on average, C3 level
    static const bool nt = [] {
        const char* e = getenv("BT_GATHER_NT");
        return !e || atoi(e) != 0;
    }();
    static const uint32_t kGatherAhead = [] {
        const char* e = getenv("BT_GATHER_AHEAD");
        return e && atoi(e) > 0 ? (uint32_t)atoi(e) : kGatherAheadDefault;
    }();
    uint32_t next = 0, k = 0;
    while (next < n || c->host.hs[0].busy || c->host.hs[1].busy) {
        HostSlot& s = c->host.hs[k & 1];
        if (s.busy) {   // retire the chunk that used this half
            HIP_TRY(hipEventSynchronize(s.done));
            if (rec_drain || decide || ver) drain_slot(c, s, rec_drain, ver, decide);
            else s.busy = false;
        }
        if (next < n) {
            const uint32_t cnt = std::min(chunk, n - next);
            // gather the header prefixes (<= slot bytes) into pinned staging:
            // per-worker byte counts, exclusive scan, then parallel copies (lean: every frame
            // one 32-B slot, so worker w starts at pad + 32 * its first frame and the counting
            // pass is skipped)
            uint8_t* pre = s.h_in;
            uint64_t* d = reinterpret_cast<uint64_t*>(s.h_in + (size_t)chunk * kHostSlotPayload);
            const unsigned T = pipeline_share(c);
            std::vector<uint64_t> part(T + 1, 0);
            const uint32_t base_i = next;
            if (lean) {
                for (unsigned w = 0; w <= T; ++w) part[w] = pad + (uint64_t)width * (uint32_t)((uint64_t)cnt * w / T);
            } else pipeline_run(c, cnt, T, [&](unsigned w) {
                const uint32_t a = (uint32_t)((uint64_t)cnt * w / T), b = (uint32_t)((uint64_t)cnt * (w + 1) / T);
                uint64_t sum = 0;
                for (uint32_t i = a; i < b; ++i) {
                    uint32_t len = 0;
                    (void)frame(base_i + i, &len);
                    sum += (std::min(len > lo ? len - lo : 0u, width) + 15) & ~15u;
                }
                part[w + 1] = sum;
            });
            if (!lean)
                for (unsigned w = 0; w < T; ++w) part[w + 1] += part[w];
            pipeline_run(c, cnt, T, [&](unsigned w) {
                const uint32_t a = (uint32_t)((uint64_t)cnt * w / T), b = (uint32_t)((uint64_t)cnt * (w + 1) / T);
                uint64_t p = part[w];
                for (uint32_t i = a; i < b; ++i) {
                    if (prefetch && i + kGatherAhead < b) {   // frames far apart: start the miss early
                        uint32_t l2 = 0;
                        const uint8_t* g = frame(base_i + i + kGatherAhead, &l2) + lo;
                        __builtin_prefetch(g);
                        if (((uintptr_t)g & 63u) + std::min(l2 > lo ? l2 - lo : 0u, width) > 64u) __builtin_prefetch(g + 64);
                    }
                    uint32_t len = 0;
                    const uint8_t* f = frame(base_i + i, &len);
                    const uint32_t m = std::min(len > lo ? len - lo : 0u, width);
                    if (m) stage_prefix(pre + p, f + lo, m, nt);
                    d[i] = BT_DESC(p - lo, len);
                    p += lean ? width : (m + 15) & ~15u;
                }
                if (nt) __builtin_ia32_sfence();   // the prefixes are visible before the H2D copy
            });
            const uint64_t pos = part[T];
            const size_t pre_bytes = (pos + 15) & ~15ull;
            if (pre_bytes) HIP_TRY(hipMemcpyAsync(s.d_in, pre, pre_bytes, hipMemcpyHostToDevice, s.stream));
            HIP_TRY(hipMemcpyAsync(s.d_in + (size_t)chunk * kHostSlotPayload, d, (size_t)cnt * 8, hipMemcpyHostToDevice,
                                   s.stream));
            bt_batch b{};
            b.base = s.d_in;
            b.desc = reinterpret_cast<const uint64_t*>(s.d_in + (size_t)chunk * kHostSlotPayload);
            b.n = cnt;
            b.bytes = (uint64_t)chunk * kHostSlotPayload;
            bt_outputs o{};
            uint8_t* drec = s.d_out;
            uint8_t* ddec = s.d_out + (size_t)chunk * BT_REC_BYTES;
            uint64_t* dver = reinterpret_cast<uint64_t*>(ddec + chunk);
            o.records = records ? drec : nullptr;
            o.n_cap = chunk;
            o.decide = want_filter ? ddec : nullptr;
            o.verdict = want_filter ? dver : nullptr;
            rc = run_device(c, &b, &o, s.stream, true, nullptr, nullptr);
            if (rc) return rc;
            if (records)
                HIP_TRY(hipMemcpyAsync(rec_direct ? static_cast<void*>(records + next) : s.h_out, drec,
                                       (size_t)cnt * BT_REC_BYTES, hipMemcpyDeviceToHost, s.stream));
            if (want_filter) {
                if (decide)   // (nothing on the host reads the staged decisions otherwise)
                    HIP_TRY(hipMemcpyAsync(s.h_out + (size_t)chunk * BT_REC_BYTES, ddec, cnt, hipMemcpyDeviceToHost,
                                           s.stream));
                HIP_TRY(hipMemcpyAsync(s.h_out + (size_t)chunk * BT_REC_BYTES + chunk, dver,
                                       ((size_t)cnt + 63) / 64 * 8, hipMemcpyDeviceToHost, s.stream));
            }
            HIP_TRY(hipEventRecord(s.done, s.stream));
            s.busy = true;
            s.lo = next;
            s.cnt = cnt;
            next += cnt;
        }
        ++k;
    }
    if (ver && (pass_idx || n_pass)) {
        uint32_t np = 0;
        for (uint32_t w = 0; w < (n + 63) / 64; ++w) {
            uint64_t x = ver[w];
            if (w == (n - 1) / 64 && (n & 63)) x &= (1ull << (n & 63)) - 1ull;
            while (x) {
                const uint32_t bit = (uint32_t)__builtin_ctzll(x);
                if (pass_idx) pass_idx[np] = w * 64 + bit;
                ++np;
                x &= x - 1;
            }
        }
        if (n_pass) *n_pass = np;
    }
    return BT_OK;
}

template <class FrameFn>
int host_pipeline(bt_ctx* c, uint32_t n, FrameFn frame, bt_rec* records, uint64_t* verdict, uint8_t* decide,
                  uint32_t* pass_idx, uint32_t* n_pass) {
    const int rc = host_pipeline_run(c, n, frame, records, verdict, decide, pass_idx, n_pass);
    if (rc) {   // retire chunks still in flight, so none is drained into a later call's buffers
        for (auto& s : c->host.hs) {
            if (s.busy) (void)hipEventSynchronize(s.done);
            s.busy = false;
        }
    }
    return rc;
}

}  // namespace

extern "C" {

int bt_parse_filter(bt_ctx* c, const uint8_t* base, const bt_pkt_desc* desc, uint32_t n, bt_rec* records,
                    uint64_t* verdict, uint8_t* decide, uint32_t* pass_idx, uint32_t* n_pass) {
    const bt::DeviceRestore keep_device;   // the caller's current device, restored on return
    if (!c) return set_error(BT_E_INVALID_ARGUMENT, "null context");
    if (n && (!base || !desc)) return set_error(BT_E_INVALID_ARGUMENT, "null packet buffer/descriptors");
    const WaitFor lk(c);
    return host_pipeline(
        c, n,
        [&](uint32_t i, uint32_t* len) {
            *len = BT_DESC_LEN(desc[i]);
            return base + BT_DESC_OFF(desc[i]);
        },
        records, verdict, decide, pass_idx, n_pass);
}

int bt_parse_filter_ptrs(bt_ctx* c, const uint8_t* const* frames, const uint32_t* lens, uint32_t n,
                         bt_rec* records, uint64_t* verdict, uint8_t* decide, uint32_t* pass_idx, uint32_t* n_pass) {
    const bt::DeviceRestore keep_device;   // the caller's current device, restored on return
    if (!c) return set_error(BT_E_INVALID_ARGUMENT, "null context");
    if (n && (!frames || !lens)) return set_error(BT_E_INVALID_ARGUMENT, "null frame pointers/lengths");
    for (uint32_t i = 0; i < n; ++i)
        if (lens[i] > 0xFFFFu) return set_error(BT_E_INVALID_ARGUMENT, "frame %u longer than 65535 bytes", i);
    const WaitFor lk(c);
    return host_pipeline(
        c, n,
        [&](uint32_t i, uint32_t* len) {
            *len = lens[i];
            return frames[i];
        },
        records, verdict, decide, pass_idx, n_pass);
}

int bt_host_stage_bytes(const bt_ctx* c, int with_records, uint32_t* bytes) {
    if (!c || !bytes) return set_error(BT_E_INVALID_ARGUMENT, "null argument");
    std::lock_guard<std::mutex> lk(const_cast<bt_ctx*>(c)->mu);
    *bytes = stage_bytes(c, with_records != 0);
    return BT_OK;
}

}  // extern "C"
