// flowreasm_host_check.cpp — TCP reassembly's host part from beatrice_amd/csrc/bt_flowreasm.h under the
// host sanitizers: the argument checks of bt_flow_reasm_device / _host (refusals, and an accepted call
// with the scratch layout it resolves to) and the pass on the host (bt::flowreasm_host) behind
// bt::flowtcpseq_host, which gives the offsets, over generated conversations. The oracle never sees a
// wire sequence number or an offset of the chain: it keeps every direction's true byte stream and true
// 64-bit positions in a std::map, decides per call which packet delivers which true byte, and asks
// std::regex about every window of at most P bytes that ends in a delivered byte and does not reach
// back over a hole. The generator cuts each stream into small segments from true offsets close below a
// multiple of 2^32 (the wire numbers wrap), reorders them inside a call, duplicates, overlaps and drops
// them, and lets some arrive a call late. Every table, id array, word array, frame buffer and output is
// a heap block of exactly its size (an access past it is an AddressSanitizer report). No device, no
// Python, no library to load; the pattern compiler is compiled in:
//
//   g++ -std=c++17 -O1 -g -fsanitize=address,undefined -fno-sanitize-recover=all -Iinclude -Ibeatrice_amd/csrc
//       tools/flowreasm_host_check.cpp beatrice_amd/csrc/bt_regex_dfa.cpp -o tools/flowreasm_host_check
//       && tools/flowreasm_host_check                                                    (one command line)
//
// Exit 0 = all cases hold.
#include <algorithm>
#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <map>
#include <regex>
#include <string>
#include <utility>
#include <vector>

#include "beatrice_gpu_bench.h"
#include "bt_flowreasm.h"
#include "bt_flowtcpseq.h"

using namespace bt;
static int g_bad = 0;
#define CHECK(x) do { if (!(x)) { std::printf("FAILED line %d: %s\n", __LINE__, #x); ++g_bad; } } while (0)

static uint32_t g_rng = 13579u;
static uint32_t rnd(uint32_t below) {
    g_rng = g_rng * 1664525u + 1013904223u;
    return (g_rng >> 8) % below;
}

static const char kPattern[] = "HE.LO|ABBA";
static const uint32_t kP = 5;

// An Ethernet / IPv4 / TCP (or UDP) frame of flow `port`, direction d, with its payload, appended to data.
static uint64_t put_frame(std::vector<uint8_t>& data, uint32_t port, uint32_t d, uint32_t seq, const uint8_t* pay, uint32_t plen, uint8_t flags,
                          uint8_t proto) {
    const uint32_t l4 = proto == 6 ? 20u : 8u, len = 14u + 20u + l4 + plen;
    const uint64_t off = data.size();
    data.resize(off + len, 0u);
    uint8_t* f = data.data() + off;
    f[12] = 0x08;
    uint8_t* ip = f + 14;
    ip[0] = 0x45;
    ip[2] = (uint8_t)((20u + l4 + plen) >> 8); ip[3] = (uint8_t)(20u + l4 + plen);
    ip[8] = 64; ip[9] = proto;
    const uint8_t a[4] = {10, 0, 0, 1}, b[4] = {10, 0, 0, 2};
    std::memcpy(ip + 12, d ? b : a, 4);
    std::memcpy(ip + 16, d ? a : b, 4);
    uint8_t* t = ip + 20;
    const uint32_t sp = d ? 80u : 1024u + port, dp = d ? 1024u + port : 80u;
    t[0] = (uint8_t)(sp >> 8); t[1] = (uint8_t)sp; t[2] = (uint8_t)(dp >> 8); t[3] = (uint8_t)dp;
    if (proto == 6) {
        t[4] = (uint8_t)(seq >> 24); t[5] = (uint8_t)(seq >> 16); t[6] = (uint8_t)(seq >> 8); t[7] = (uint8_t)seq;
        t[12] = 0x50; t[13] = flags;
    } else {
        t[4] = (uint8_t)((8u + plen) >> 8); t[5] = (uint8_t)(8u + plen);
    }
    if (plen) std::memcpy(t + l4, pay, plen);
    return off | (uint64_t)len << 48;
}

// What the generator knows of one direction: its true bytes from position `origin`, how far it has cut
// them into segments, and what the oracle keeps between calls.
struct Truth {
    int64_t origin = 0;
    std::vector<uint8_t> bytes;
    size_t cut = 0;                 // the bytes below it have been sent at least once
    bool have = false;              // the oracle's: a byte was delivered
    int64_t next = 0, run = 0;      // delivered up to (true position); where the contiguous run that ends there began
    uint32_t packets = 0, hits = 0, holes = 0, dups = 0, late = 0;
    uint64_t dupb = 0, holeb = 0, lateb = 0;
};
struct Sent { uint32_t f, d; int64_t at; uint32_t len; };   // a TCP data segment as generated: true position of its first byte

static std::vector<Sent> g_held;   // segments that arrive a call late
static uint64_t g_tot[6];          // over all cases: delivered packets, hits, holes, duplicates, late, rest bits

static void reasm_case(uint32_t n, uint32_t cap, uint32_t flows, int sel_kind, bool bidir, int alias, const std::vector<uint8_t>& blob,
                       const FstPattern& pat, const std::regex& rx, std::vector<bt_flow_tcpseq_rec>& seq_table,
                       std::vector<bt_flow_reasm_rec>& table, std::map<std::pair<uint32_t, uint32_t>, Truth>& truth) {
    const uint32_t nw = (n + 63u) / 64u;
    std::vector<uint8_t> data;
    std::vector<uint64_t> desc(n), sel(nw);
    std::vector<uint32_t> ids(n);
    std::vector<Sent> sent(n, Sent{0u, 0u, 0, 0u});
    for (uint32_t w = 0; w < nw; ++w)
        sel[w] = sel_kind == 1 ? ~0ull : ((uint64_t)rnd(1u << 16) << 48 | (uint64_t)rnd(1u << 24) << 24 | rnd(1u << 24)) | 0x7777777777777777ull;
    if (n % 64u) sel[nw - 1] |= ~0ull << (n % 64u);   // garbage above n: ignored
    // the segments of the call, in order per direction, then disturbed
    std::vector<Sent> list = g_held;
    g_held.clear();
    while (list.size() < n) {
        const uint32_t f = rnd(flows), d = bidir ? rnd(2) : 0u;
        Truth& t = truth[{f, d}];
        if (t.bytes.empty()) {
            t.origin = ((int64_t)(f + 1u) << 33) - 30 + (int64_t)d * 11;   // close below a multiple of 2^32: wraps at once
            t.bytes.resize(40000);
            for (auto& c : t.bytes) c = (uint8_t)"HELOAB."[rnd(7)];
            for (size_t k = 5; k + 5 < t.bytes.size(); k += 23 + rnd(9)) std::memcpy(&t.bytes[k], rnd(3) ? "HEXLO" : "ABBA.", 5);
        }
        const uint32_t len = 1u + rnd(rnd(4) ? 6u : 300u), op = rnd(12);
        if (t.cut + len + 400u > t.bytes.size()) continue;
        Sent s{f, d, t.origin + (int64_t)t.cut, len};
        if (op == 0) { t.cut += len; continue; }                                   // dropped
        if (op == 1 && t.cut > 3) { s.at -= 1 + rnd(3); }                          // overlaps what was sent
        else if (op == 2 && t.cut > 310) { s.at -= 1 + rnd(300); }                 // old or overlapping
        else t.cut += len;
        if (op == 3) { g_held.push_back(s); continue; }                            // arrives a call late
        list.push_back(s);
        if (op == 4) list.push_back(s);                                            // duplicated
    }
    list.resize(n);
    for (uint32_t i = 0; i + 1 < n; ++i)   // reordered within a few places
        if (rnd(3) == 0) std::swap(list[i], list[i + 1 + rnd(std::min(6u, n - i - 1u))]);
    for (uint32_t i = 0; i < n; ++i) {
        const Sent& s = list[i];
        const Truth& t = truth[{s.f, s.d}];
        const uint32_t r = rnd(30);
        ids[i] = r == 0 ? 0xFFFFFFFFu - rnd(5) : r == 1 ? cap + rnd(3) : s.f;
        const bool udp = rnd(25) == 0;
        desc[i] = put_frame(data, s.f, s.d, (uint32_t)(uint64_t)s.at, &t.bytes[(size_t)(s.at - t.origin)], s.len, 0x18, udp ? 17 : 6);
        if (!udp) sent[i] = s;   // len == 0: no TCP data segment
    }

    // the oracle: true positions only
    std::vector<uint64_t> whit(nw, 0ull), wrest(nw, 0ull);
    bt_flow_reasm_result want{};
    want.n = n;
    std::map<std::pair<uint32_t, uint32_t>, std::vector<uint32_t>> mine;
    for (uint32_t i = 0; i < n; ++i) {
        if (!((sel[i / 64u] >> (i % 64u)) & 1u)) continue;
        ++want.selected;
        const bool placed = ids[i] < cap && sent[i].len;   // what the sequence call gives an offset
        if (!placed) wrest[i / 64u] |= 1ull << (i % 64u);
        if (ids[i] >= cap) {
            if (flowtcp_is_sentinel(ids[i])) ++want.unkeyed; else ++want.bad_ids;
            continue;
        }
        if (placed) mine[{ids[i], sent[i].d}].push_back(i);
    }
    for (auto& kv : mine) {
        // the table's direction ids[i] may differ from the generator's flow (never here: ids[i] == s.f when below cap)
        Truth& t = truth[kv.first];
        std::vector<std::pair<int64_t, uint32_t>> order;
        for (uint32_t i : kv.second) {
            const int64_t at = sent[i].at, end = at + sent[i].len;
            if (t.have && end <= t.next) { ++t.late; t.lateb += sent[i].len; ++want.late_packets; continue; }
            order.push_back({t.have && at < t.next ? t.next : at, i});
            if (t.have && at < t.next) t.dupb += (uint64_t)(t.next - at);
        }
        std::sort(order.begin(), order.end());
        if (order.empty()) continue;
        int64_t hi = t.have ? t.next : order[0].first;
        if (!t.have) t.run = hi;
        for (auto& o : order) {
            const uint32_t i = o.second;
            const int64_t at = o.first, end = sent[i].at + sent[i].len;
            if (at > hi) { ++t.holes; ++want.holes; t.holeb += (uint64_t)(at - hi); t.run = at; }
            if (end <= hi) { ++t.dups; ++want.dup_packets; t.dupb += (uint64_t)(end - at); continue; }
            const int64_t from = at > hi ? at : hi;
            t.dupb += (uint64_t)(from - at);
            ++t.packets; ++want.stream_packets;
            want.stream_bytes += (uint64_t)(end - from);
            bool hit = false;
            for (int64_t e = from + 1; e <= end && !hit; ++e)
                for (int64_t s = std::max(t.run, e - (int64_t)kP); s < e && !hit; ++s)
                    hit = std::regex_match(reinterpret_cast<const char*>(t.bytes.data()) + (s - t.origin),
                                           reinterpret_cast<const char*>(t.bytes.data()) + (e - t.origin), rx);
            if (hit) { ++t.hits; ++want.hit_packets; whit[i / 64u] |= 1ull << (i % 64u); }
            hi = end;
        }
        t.next = hi;
        t.have = true;
    }

    // the chain: the sequence call's offsets, then the reassembly
    std::vector<int64_t> off(n, 7);
    bt_flow_tcpseq_result qres;
    bt_flow_tcpseq_out qout{nullptr, off.data(), nullptr, &qres, {0, 0}};
    const uint32_t flags = bidir ? BT_FLOWTAB_BIDIRECTIONAL : 0u;
    flowtcpseq_host(data.data(), data.size(), desc.data(), n, ids.data(), sel.data(), flags, seq_table.data(), cap, &qout);
    std::vector<uint64_t> hit(nw, 0xDEADull), rest(nw, 0xDEADull), sel_copy = sel;
    bt_flow_reasm_result res;
    std::memset(&res, 0xEE, sizeof(res));
    uint64_t* const sp = alias == 1 ? hit.data() : alias == 2 ? rest.data() : sel_copy.data();
    if (alias == 1) hit = sel;
    if (alias == 2) rest = sel;
    bt_flow_reasm_out out{hit.data(), rest.data(), &res, {0, 0}};
    char why[160];
    FstPattern p2;
    CHECK(flowreasm_host_args(data.data(), desc.data(), n, ids.data(), sp, off.data(), flags, blob.data(), (uint32_t)blob.size(), table.data(),
                              cap, &out, &p2, why, sizeof(why)) == BT_OK);
    flowreasm_host(data.data(), data.size(), desc.data(), n, ids.data(), sp, off.data(), flags, blob.data(), pat, table.data(), cap, &out);
    g_tot[0] += want.stream_packets; g_tot[1] += want.hit_packets; g_tot[2] += want.holes; g_tot[3] += want.dup_packets; g_tot[4] += want.late_packets;
    for (uint64_t w : wrest) g_tot[5] += (uint64_t)__builtin_popcountll(w);
    CHECK(hit == whit);
    CHECK(rest == wrest);
    CHECK(res.n == want.n && res.selected == want.selected && res.unkeyed == want.unkeyed && res.bad_ids == want.bad_ids);
    CHECK(res.stream_packets == want.stream_packets && res.stream_bytes == want.stream_bytes && res.hit_packets == want.hit_packets);
    CHECK(res.holes == want.holes && res.dup_packets == want.dup_packets && res.late_packets == want.late_packets && res.far_packets == 0);
    for (auto& kv : truth) {
        if (kv.first.first >= cap) continue;
        const Truth& t = kv.second;
        const bt_flow_reasm_dir& d = table[kv.first.first].d[kv.first.second];
        CHECK(d.have == (t.have ? 1u : 0u));
        CHECK(d.stream_packets == t.packets && d.hit_packets == t.hits && d.holes == t.holes && d.dup_packets == t.dups && d.late_packets == t.late);
        CHECK(d.dup_bytes == t.dupb && d.hole_bytes == t.holeb && d.late_bytes == t.lateb);
    }
}

int main() {
    uint32_t size = 0;
    bt_flow_stream_info info;
    char why[160];
    CHECK(flowstream_compile(kPattern, nullptr, 0, &size, &info, why, sizeof(why)) == BT_OK);
    std::vector<uint8_t> blob(size);
    CHECK(flowstream_compile(kPattern, blob.data(), size, &size, &info, why, sizeof(why)) == BT_OK && info.positions >= kP);
    FstPattern pat;
    CHECK(flowstream_pattern(blob.data(), size, &pat, why, sizeof(why)) == BT_OK);
    const std::regex rx(kPattern);

    // where a segment lands: the rules 1. - 4. at their edges
    CHECK(flowreasm_place(0, 0, 10, 0, 0).what == kFrTake && flowreasm_place(0, 0, 10, 0, 0).rel == (1u << 30));
    CHECK(flowreasm_place(0, 1, 10, 0, 0).rel == (1u << 30) + 1u);
    CHECK(flowreasm_place(-(1ll << 30) - 1, 0, 10, 0, 0).what == kFrFar && flowreasm_place(-(1ll << 30), 0, 10, 0, 0).rel == 0u);
    CHECK(flowreasm_place(kFrRelMax - (1ll << 30), 0, 10, 0, 0).what == kFrTake && flowreasm_place(kFrRelMax - (1ll << 30) + 1, 0, 10, 0, 0).what == kFrFar);
    CHECK(flowreasm_place(90, 0, 10, 1, 100).what == kFrLate && flowreasm_place(91, 0, 10, 1, 100).what == kFrTake);
    CHECK(flowreasm_place(91, 0, 10, 1, 100).trim == 9u && flowreasm_place(91, 0, 10, 1, 100).rel == 0u);
    CHECK(flowreasm_place(100 + kFrRelMax, 0, 10, 1, 100).what == kFrTake && flowreasm_place(101 + kFrRelMax, 0, 10, 1, 100).what == kFrFar);
    CHECK(flowreasm_place(INT64_MAX, 1, 10, 1, 100).what != kFrTake);   // wraps: no sanitizer report

    // the generated conversations
    for (int round = 0; round < 12; ++round) {
        const uint32_t cap = round % 4 == 3 ? 1u : 3u + rnd(4), flows = cap;
        const bool bidir = round % 2 == 0;
        std::vector<bt_flow_tcpseq_rec> seq_table(cap);
        std::vector<bt_flow_reasm_rec> table(cap);
        std::memset(seq_table.data(), 0, cap * sizeof(bt_flow_tcpseq_rec));
        std::memset(table.data(), 0, cap * sizeof(bt_flow_reasm_rec));
        std::map<std::pair<uint32_t, uint32_t>, Truth> truth;
        g_held.clear();
        static const uint32_t sizes[] = {65, 1, 63, 64, 130, 200};
        for (int call = 0; call < 6; ++call) reasm_case(sizes[(round + call) % 6], cap, flows, 1 + (round + call) % 2, bidir, (round + call) % 3, blob, pat, rx, seq_table, table, truth);
    }
    {   // n == 0
        std::vector<bt_flow_tcpseq_rec> seq_table(2);
        std::vector<bt_flow_reasm_rec> table(2);
        std::memset(seq_table.data(), 0, 2 * sizeof(bt_flow_tcpseq_rec));
        std::memset(table.data(), 0, 2 * sizeof(bt_flow_reasm_rec));
        bt_flow_reasm_result res;
        std::memset(&res, 0xEE, sizeof(res));
        bt_flow_reasm_out out{nullptr, nullptr, &res, {0, 0}};
        flowreasm_host(nullptr, 0, nullptr, 0, nullptr, nullptr, nullptr, 0, blob.data(), pat, table.data(), 2, &out);
        CHECK(res.n == 0 && res.selected == 0 && res.stream_bytes == 0 && res.reserved1 == 0);
    }

    // the argument checks of the device form, and the layout an accepted call resolves to
    {
        std::vector<uint8_t> frames(256);
        std::vector<uint64_t> desc(4), words(2), more(2);
        std::vector<uint32_t> ids(4);
        std::vector<int64_t> off(4);
        std::vector<bt_flow_reasm_rec> table(4);
        bt_flow_reasm_result res;
        const FrLayout l = fr_layout(2, 4);
        std::vector<uint8_t> raw(l.total + 512);
        void* const scratch = reinterpret_cast<void*>((reinterpret_cast<uintptr_t>(raw.data()) + 255u) & ~(uintptr_t)255u);
        bt_batch b{};
        b.base = frames.data(); b.desc = desc.data(); b.n = 2; b.bytes = 256; b.desc_format = BT_DESC_PACKED;
        bt_flow_reasm_out out{words.data(), more.data(), &res, {0, 0}};
        FlowreasmArgs a;
        const auto call = [&](const bt_batch* fr, const int64_t* o, const void* pd, uint64_t nbytes, const bt_flow_reasm_out* ou) {
            return flowreasm_args(fr, ids.data(), words.data(), o, 0, blob.data(), pd, size, table.data(), 4, scratch, nbytes, ou, &a, why, sizeof(why));
        };
        CHECK(call(&b, off.data(), blob.data(), l.total, &out) == BT_OK);
        CHECK(a.passes == fst_passes(4) && reinterpret_cast<uint8_t*>(a.bits) + ft_round(a.bits_bytes) == static_cast<uint8_t*>(scratch) + l.total);
        CHECK(reinterpret_cast<uint8_t*>(a.seg) == static_cast<uint8_t*>(scratch) + l.seg && l.head < l.numw && l.numw < l.hitw && l.carry < l.bits);
        CHECK(call(&b, off.data(), blob.data(), l.total - 1, &out) == BT_E_INVALID_ARGUMENT && std::strstr(why, "scratch_bytes"));
        CHECK(call(&b, nullptr, blob.data(), l.total, &out) == BT_E_INVALID_ARGUMENT && std::strstr(why, "null off"));
        CHECK(call(nullptr, off.data(), blob.data(), l.total, &out) == BT_E_INVALID_ARGUMENT && std::strstr(why, "null frames"));
        CHECK(call(&b, off.data(), nullptr, l.total, &out) == BT_E_INVALID_ARGUMENT && std::strstr(why, "null pattern_device"));
        bt_flow_reasm_out same{words.data(), words.data(), &res, {0, 0}};
        CHECK(call(&b, off.data(), blob.data(), l.total, &same) == BT_E_INVALID_ARGUMENT && std::strstr(why, "hit and rest are one"));
        bt_flow_reasm_out resv{words.data(), more.data(), &res, {0, 1}};
        CHECK(call(&b, off.data(), blob.data(), l.total, &resv) == BT_E_INVALID_ARGUMENT && std::strstr(why, "reserved"));
        b.flags = BT_BATCH_LEAN;
        CHECK(call(&b, off.data(), blob.data(), l.total, &out) == BT_E_INVALID_ARGUMENT && std::strstr(why, "BT_BATCH_PREFIXES"));
        uint64_t last = 0;
        for (uint32_t n : {0u, 1u, 64u, 65u, 16384u, 16385u, 1u << 20}) {
            const FrLayout x = fr_layout(n, 1000);
            CHECK(x.total >= last && x.total % 256u == 0);
            last = x.total;
        }
    }
    std::printf("delivered %llu, hits %llu, holes %llu, duplicates %llu, late %llu, rest %llu\n", (unsigned long long)g_tot[0], (unsigned long long)g_tot[1],
                (unsigned long long)g_tot[2], (unsigned long long)g_tot[3], (unsigned long long)g_tot[4], (unsigned long long)g_tot[5]);
    for (uint64_t v : g_tot) CHECK(v > 20);   // the cases are not vacuous
    std::printf(g_bad ? "flowreasm_host_check: %d check(s) FAILED\n" : "flowreasm_host_check: all checks hold\n", g_bad);
    return g_bad ? 1 : 0;
}
