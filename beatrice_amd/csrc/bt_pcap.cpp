// bt_pcap.cpp — classic pcap capture files in and out (include/beatrice_gpu.h):
//   bt_pcap_index   host only: one descriptor per whole record of a file in memory
//   bt_pcap_filter  the file through the context's filter program, chunk by chunk: pinned
//                   staging, H2D, filter-only bt_parse_filter_device, bt_pass_pack_device with
//                   lead = 16 (each record header rides in front of its frame), and a D2H copy
//                   of exactly the packed bytes, so only the passing records come back.
// With BT_PCAP_HOST_ONLY defined only the indexer is compiled (no HIP, no runtime): the form a
// stand-alone host program links for memory checking.
#include <cstdarg>
#include <cstdint>
#include <cstring>

#include "beatrice_gpu.h"

#ifdef BT_PCAP_HOST_ONLY
namespace bt {
static int set_error(int code, const char*, ...) { return code; }
}  // namespace bt
#else
#include <hip/hip_runtime_api.h>

#include <algorithm>
#include <mutex>
#include <vector>

#include "bt_ctx.h"
#include "bt_hip_util.h"
#endif

namespace {

constexpr uint32_t kMagicUsec = 0xa1b2c3d4u, kMagicNsec = 0xa1b23c4du;
constexpr uint32_t kMagicPcapng = 0x0a0d0d0au;   // a pcapng Section Header Block's type (a palindrome)
constexpr uint64_t kGlobalHeader = 24, kRecordHeader = 16;
constexpr uint32_t kLinkEthernet = 1;

inline uint32_t load32(const uint8_t* p, bool swapped) {
    uint32_t v;
    std::memcpy(&v, p, 4);
    return swapped ? __builtin_bswap32(v) : v;
}

// The record whose header starts at pos (< bytes): 0 = whole (*incl = its data bytes), 1 = the
// file ends inside its header or its data, 2 = incl_len > 65535 (*incl = the value).
inline int record_at(const uint8_t* file, uint64_t bytes, uint64_t pos, bool swapped, uint32_t* incl) {
    if (bytes - pos < kRecordHeader) return 1;
    *incl = load32(file + pos + 8, swapped);
    if (*incl > 0xFFFFu) return 2;
    return bytes - pos - kRecordHeader < *incl ? 1 : 0;
}

}  // namespace

extern "C" int bt_pcap_index(const uint8_t* file, uint64_t bytes, bt_pcap_info* info, bt_pkt_desc* desc,
                             uint64_t cap, uint64_t* n) {
    if (!file || !info || !n) return bt::set_error(BT_E_INVALID_ARGUMENT, "null argument");
    *n = 0;
    *info = bt_pcap_info{};
    if (bytes >= 4 && load32(file, false) == kMagicPcapng)
        return bt::set_error(BT_E_NOT_IMPLEMENTED, "a pcapng file (classic pcap only)");
    if (bytes < kGlobalHeader)
        return bt::set_error(BT_E_INVALID_ARGUMENT, "%llu bytes: no pcap global header", (unsigned long long)bytes);
    const uint32_t raw = load32(file, false);
    bool swapped = false;
    if (raw == kMagicUsec || raw == kMagicNsec) {
        info->magic = raw;
    } else if (__builtin_bswap32(raw) == kMagicUsec || __builtin_bswap32(raw) == kMagicNsec) {
        info->magic = __builtin_bswap32(raw);
        swapped = true;
    } else {
        return bt::set_error(BT_E_INVALID_ARGUMENT, "unknown pcap magic 0x%08x", raw);
    }
    info->swapped = swapped ? 1u : 0u;
    info->nanosecond = info->magic == kMagicNsec ? 1u : 0u;
    info->snaplen = load32(file + 16, swapped);
    info->linktype = load32(file + 20, swapped);
    info->end = kGlobalHeader;
    if (info->linktype != kLinkEthernet)
        return bt::set_error(BT_E_NOT_IMPLEMENTED, "link type %u (Ethernet, 1, only)", info->linktype);
    uint64_t pos = kGlobalHeader, count = 0;
    while (pos < bytes) {
        uint32_t incl = 0;
        const int what = record_at(file, bytes, pos, swapped, &incl);
        if (what == 2)
            return bt::set_error(BT_E_INVALID_ARGUMENT, "record %llu: incl_len %u > 65535", (unsigned long long)count, incl);
        if (what == 1) { info->truncated = 1; break; }   // ends inside a record header or its data
        if (desc && count < cap) desc[count] = BT_DESC(pos + kRecordHeader, incl);
        ++count;
        pos += kRecordHeader + incl;
        info->end = pos;
    }
    *n = count;
    return BT_OK;
}

#ifndef BT_PCAP_HOST_ONLY

namespace bt {

// One half of the double buffer: a chunk of whole records in flight on its own stream.
struct PcapSlot {
    hipStream_t stream = nullptr;
    uint8_t* h_in = nullptr;       // pinned: the chunk's file bytes, then its descriptors
    uint8_t* d_in = nullptr;
    uint8_t* h_out = nullptr;      // pinned: packed records | decision bytes | total, n_packed
    uint8_t* d_out = nullptr;      // packed records | decision bytes | verdict words | total, n_packed
    bool busy = false;
    uint32_t n = 0;                // the chunk's records
    uint64_t len = 0;              // ... and file bytes
};

struct PcapStage {
    std::mutex mu;                 // one bt_pcap_filter call at a time per context
    int device = 0;
    uint64_t cap_bytes = 0;        // chunk capacity the buffers were sized for
    uint32_t cap_pkts = 0;
    PcapSlot s[2];
};

namespace {

std::mutex g_stage_mu;             // creation of a context's stage

void stage_release(PcapStage* st) {
    for (auto& s : st->s) {
        if (s.h_in) (void)hipHostFree(s.h_in);
        if (s.d_in) (void)hipFree(s.d_in);
        if (s.h_out) (void)hipHostFree(s.h_out);
        if (s.d_out) (void)hipFree(s.d_out);
        s.h_in = s.d_in = s.h_out = s.d_out = nullptr;
    }
    st->cap_bytes = 0;
    st->cap_pkts = 0;
}

inline uint64_t up64(uint64_t x) { return (x + 63u) & ~63ull; }

// Layout of the buffers for a chunk capacity (bytes, pkts).
struct Layout {
    uint64_t in_desc, in_size;                                  // d_in / h_in: frames at 0, descriptors
    uint64_t out_decide, out_verdict, out_totals, out_size;     // d_out: packed at 0, ...
    uint64_t hout_decide, hout_totals, hout_size;               // h_out: packed at 0, decide, totals
};
Layout layout_of(uint64_t bytes, uint32_t pkts) {
    Layout l{};
    l.in_desc = up64(bytes + 64);   // slack: a 16-B chunk read may pass the last frame byte
    l.in_size = l.in_desc + up64((uint64_t)pkts * 8);
    l.out_decide = up64(bytes);
    l.out_verdict = l.out_decide + up64(pkts);
    l.out_totals = l.out_verdict + up64(((uint64_t)pkts + 63) / 64 * 8);
    l.out_size = l.out_totals + 64;
    l.hout_decide = up64(bytes);
    l.hout_totals = l.hout_decide + up64(pkts);
    l.hout_size = l.hout_totals + 64;
    return l;
}

#define PCAP_HIP(x)                                                                                 \
    do {                                                                                            \
        hipError_t e_ = (x);                                                                        \
        if (e_ != hipSuccess) return set_error(BT_E_INTERNAL, "%s: %s", #x, hipGetErrorString(e_)); \
    } while (0)

int stage_ensure(PcapStage* st, uint64_t bytes, uint32_t pkts) {
    if (bytes <= st->cap_bytes && pkts <= st->cap_pkts && st->s[0].stream) return BT_OK;
    for (auto& s : st->s)
        if (s.stream) PCAP_HIP(hipStreamSynchronize(s.stream));
    bytes = std::max(bytes, st->cap_bytes);   // never shrink: a later, smaller file reuses the buffers
    pkts = std::max(pkts, st->cap_pkts);
    stage_release(st);
    const Layout l = layout_of(bytes, pkts);
    for (auto& s : st->s) {
        if (!s.stream) PCAP_HIP(hipStreamCreateWithFlags(&s.stream, hipStreamNonBlocking));
        PCAP_HIP(hipHostMalloc(reinterpret_cast<void**>(&s.h_in), l.in_size, hipHostMallocDefault));
        PCAP_HIP(hipMalloc(reinterpret_cast<void**>(&s.d_in), l.in_size));
        PCAP_HIP(hipHostMalloc(reinterpret_cast<void**>(&s.h_out), l.hout_size, hipHostMallocDefault));
        PCAP_HIP(hipMalloc(reinterpret_cast<void**>(&s.d_out), l.out_size));
    }
    st->cap_bytes = bytes;
    st->cap_pkts = pkts;
    return BT_OK;
}

// memcpy on the context's host threads for copies large enough to pay for the hand-off.
void big_copy(bt_ctx* c, uint8_t* dst, const uint8_t* src, uint64_t bytes) {
    if (bytes < (8ull << 20)) {
        std::memcpy(dst, src, bytes);
        return;
    }
    host_parallel(c, [&](unsigned w, unsigned T) {
        const uint64_t lo = (bytes * w / T) & ~63ull, hi = w + 1 == T ? bytes : (bytes * (w + 1) / T) & ~63ull;
        if (hi > lo) std::memcpy(dst + lo, src + lo, hi - lo);
    });
}

struct Run {
    bt_ctx* c;
    PcapStage* st;
    Layout l;
    const uint8_t* file;
    uint8_t* out;
    uint64_t out_cap;
    uint64_t pos;                  // bytes of the output so far (the need, even past out_cap)
    bt_pcap_result* res;
};

// The n whole records in file bytes [c0, c1) onto slot s, whose staging already holds their
// descriptors (relative to c0): staging, H2D, filter, pack, and the small D2H copies.
int chunk_start(Run& r, PcapSlot& s, uint64_t c0, uint64_t c1, uint32_t n) {
    s.n = n;
    s.len = c1 - c0;
    big_copy(r.c, s.h_in, r.file + c0, s.len);
    bt_pkt_desc* hd = reinterpret_cast<bt_pkt_desc*>(s.h_in + r.l.in_desc);
    PCAP_HIP(hipMemcpyAsync(s.d_in, s.h_in, s.len, hipMemcpyHostToDevice, s.stream));
    PCAP_HIP(hipMemcpyAsync(s.d_in + r.l.in_desc, hd, (size_t)s.n * 8, hipMemcpyHostToDevice, s.stream));
    s.busy = true;
    bt_batch b{};
    b.base = s.d_in;
    b.desc = s.d_in + r.l.in_desc;
    b.n = s.n;
    b.bytes = s.len;
    b.desc_format = BT_DESC_PACKED;
    bt_outputs o{};
    o.verdict = reinterpret_cast<uint64_t*>(s.d_out + r.l.out_verdict);
    o.decide = s.d_out + r.l.out_decide;
    if (int rc = bt_parse_filter_device(r.c, &b, &o, s.stream)) return rc;
    bt_pack_opts po{};
    po.lead = (uint32_t)kRecordHeader;
    po.align = 1;
    bt_pack_out out{};
    out.bytes = s.d_out;
    out.cap = s.len;               // the passing records are a subset of the chunk's bytes
    out.total = reinterpret_cast<uint64_t*>(s.d_out + r.l.out_totals);
    out.n_packed = reinterpret_cast<uint32_t*>(s.d_out + r.l.out_totals + 8);
    if (int rc = bt_pass_pack_device(r.c, &b, o.verdict, &po, &out, s.stream)) return rc;
    PCAP_HIP(hipMemcpyAsync(s.h_out + r.l.hout_totals, s.d_out + r.l.out_totals, 16, hipMemcpyDeviceToHost, s.stream));
    PCAP_HIP(hipMemcpyAsync(s.h_out + r.l.hout_decide, s.d_out + r.l.out_decide, s.n, hipMemcpyDeviceToHost, s.stream));
    return BT_OK;
}

// Waits for slot s's chunk, counts its decisions and brings its packed records back.
int chunk_finish(Run& r, PcapSlot& s) {
    if (!s.busy) return BT_OK;
    s.busy = false;
    PCAP_HIP(hipStreamSynchronize(s.stream));
    uint64_t total;
    uint32_t n_packed;
    std::memcpy(&total, s.h_out + r.l.hout_totals, 8);
    std::memcpy(&n_packed, s.h_out + r.l.hout_totals + 8, 4);
    uint64_t by_code[4] = {0, 0, 0, 0};
    const uint8_t* dec = s.h_out + r.l.hout_decide;
    for (uint32_t i = 0; i < s.n; ++i) ++by_code[dec[i] >> 6];
    if (by_code[BT_DECIDE_HOST])
        return set_error(BT_E_INTERNAL, "pcap filter: %llu decisions left to the host by a program without host slots",
                         (unsigned long long)by_code[BT_DECIDE_HOST]);
    if (total > s.len || n_packed != by_code[BT_DECIDE_PASS])
        return set_error(BT_E_INTERNAL, "pcap filter: packed %u records / %llu bytes of a chunk with %llu passing / %llu bytes",
                         n_packed, (unsigned long long)total, (unsigned long long)by_code[BT_DECIDE_PASS],
                         (unsigned long long)s.len);
    r.res->n_pass += by_code[BT_DECIDE_PASS];
    r.res->n_reject += by_code[BT_DECIDE_REJECT];
    r.res->n_throw += by_code[BT_DECIDE_THROW];
    if (r.out && total && r.pos + total <= r.out_cap) {
        PCAP_HIP(hipMemcpyAsync(s.h_out, s.d_out, total, hipMemcpyDeviceToHost, s.stream));
        PCAP_HIP(hipStreamSynchronize(s.stream));
        big_copy(r.c, r.out + r.pos, s.h_out, total);
    }
    r.pos += total;
    return BT_OK;
}

}  // namespace

void pcap_stage_free(PcapStage* st) {
    if (!st) return;
    for (auto& s : st->s)
        if (s.stream) (void)hipStreamSynchronize(s.stream);
    stage_release(st);
    for (auto& s : st->s)
        if (s.stream) (void)hipStreamDestroy(s.stream);
    delete st;
}

}  // namespace bt

extern "C" int bt_pcap_filter(bt_ctx* c, const uint8_t* file, uint64_t bytes, uint8_t* out, uint64_t out_cap,
                              bt_pcap_result* res) {
    using namespace bt;
    const DeviceRestore keep_device;   // the caller's current device, restored on return
    if (!c || !file || !res) return set_error(BT_E_INVALID_ARGUMENT, "null argument");
    *res = bt_pcap_result{};
    // a slot the device cannot decide would silently change the pass set: refuse before any work
    bt_filter_slot slots[BT_MAX_FILTERS];
    uint32_t n_slots = 0;
    if (int rc = bt_filter_program(c, slots, BT_MAX_FILTERS, &n_slots)) return rc;
    for (uint32_t i = 0; i < n_slots && i < BT_MAX_FILTERS; ++i)
        if (slots[i].kind == BT_K_HOST)
            return set_error(BT_E_NOT_IMPLEMENTED, "filter slot %u (source filter %u) is evaluated on the host: "
                             "a CUSTOM callback or a PAYLOAD regex outside the GPU subset", i, slots[i].source_index);
    // the global header alone is checked first (magic, link type); the records are walked chunk by
    // chunk below, each walk beside the device's work on the chunk before it
    bt_pcap_info info{};
    uint64_t none = 0;
    if (int rc = bt_pcap_index(file, std::min<uint64_t>(bytes, kGlobalHeader), &info, nullptr, 0, &none)) return rc;
    const bool swapped = info.swapped != 0;

    // chunk capacity: the context's host chunk limits, at most 64 MiB / 1M packets, at least one
    // record of the largest size, and no more than the file can hold
    const bt_opts o = c->opts;
    const uint64_t body = bytes - kGlobalHeader;
    uint64_t cap_bytes = o.host_chunk_bytes ? o.host_chunk_bytes : (64ull << 20);
    cap_bytes = std::min<uint64_t>(cap_bytes, 64ull << 20);
    cap_bytes = std::max<uint64_t>(cap_bytes, kRecordHeader + 65535u);
    cap_bytes = std::min<uint64_t>(cap_bytes, std::max<uint64_t>(body, kRecordHeader + 65535u));
    uint64_t cap_pkts = o.host_chunk_packets ? o.host_chunk_packets : (1u << 20);
    cap_pkts = std::min<uint64_t>(cap_pkts, 1u << 20);
    cap_pkts = std::max<uint64_t>(1, std::min<uint64_t>(cap_pkts, body / kRecordHeader + 1));

    PcapStage* st = nullptr;
    {
        std::lock_guard<std::mutex> lk(g_stage_mu);
        PcapStage*& slot = c->pcap;
        if (!slot) {
            slot = new PcapStage();
            slot->device = c->device;
        }
        st = slot;
    }
    std::lock_guard<std::mutex> lk(st->mu);
    if (hipSetDevice(st->device) != hipSuccess) return set_error(BT_E_INTERNAL, "hipSetDevice(%d) failed", st->device);
    int rc = BT_OK;
    if (body) {
        if ((rc = stage_ensure(st, cap_bytes, (uint32_t)cap_pkts))) return rc;
        if ((rc = bt_reserve(c, (uint32_t)cap_pkts))) return rc;
    }
    Run r{c, st, layout_of(st->cap_bytes, st->cap_pkts), file, out, out_cap, kGlobalHeader, res};
    if (out && out_cap >= kGlobalHeader) std::memcpy(out, file, kGlobalHeader);

    uint64_t pos = kGlobalHeader;
    uint32_t k = 0;
    while (pos < bytes && rc == BT_OK) {
        PcapSlot& s = st->s[k & 1u];
        if ((rc = chunk_finish(r, s))) break;              // idle already: its chunk was finished a round ago
        // walk the chunk's records into the slot's descriptor staging
        bt_pkt_desc* hd = reinterpret_cast<bt_pkt_desc*>(s.h_in + r.l.in_desc);
        const uint64_t c0 = pos;
        uint32_t n = 0;
        while (pos < bytes && n < cap_pkts) {
            uint32_t incl = 0;
            const int what = record_at(file, bytes, pos, swapped, &incl);
            if (what == 2) {
                rc = set_error(BT_E_INVALID_ARGUMENT, "record %llu: incl_len %u > 65535",
                               (unsigned long long)(res->n_in + n), incl);
                break;
            }
            if (what == 1) { res->truncated = 1; break; }
            if (n && pos + kRecordHeader + incl - c0 > cap_bytes) break;   // a chunk always takes its first record
            hd[n++] = BT_DESC(pos + kRecordHeader - c0, incl);
            pos += kRecordHeader + incl;
        }
        if (rc != BT_OK || !n) break;
        res->n_in += n;
        if ((rc = chunk_start(r, s, c0, pos, n))) break;
        if ((rc = chunk_finish(r, st->s[(k & 1u) ^ 1u]))) break;   // the previous chunk, beside this one
        ++k;
        ++res->chunks;
        if (res->truncated) break;
    }
    for (uint32_t j = 0; j < 2 && rc == BT_OK; ++j) rc = chunk_finish(r, st->s[(k + j) & 1u]);
    if (rc != BT_OK) {   // leave nothing running: wait for both streams, keep the first error
        for (auto& s : st->s) {
            if (s.stream) (void)hipStreamSynchronize(s.stream);
            s.busy = false;
        }
        (void)hipGetLastError();
        return rc;
    }
    res->out_bytes = r.pos;
    if (out && r.pos > out_cap)
        return set_error(BT_E_INVALID_ARGUMENT, "output capacity %llu below the %llu bytes the filtered capture needs",
                         (unsigned long long)out_cap, (unsigned long long)r.pos);
    return BT_OK;
}

#endif  // BT_PCAP_HOST_ONLY
