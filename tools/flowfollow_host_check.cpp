// flowfollow_host_check.cpp — the exported reassembly's host part from beatrice_amd/csrc/bt_flowfollow.h
// under the host sanitizers: the argument checks of bt_flow_follow_device / _host (refusals, and an
// accepted call with the scratch layout it resolves to) and the pass on the host (bt::flowfollow_host)
// behind bt::flowtcpseq_host, which gives the offsets, over generated conversations. The oracle never
// sees a wire sequence number or an offset of the chain: it keeps every direction's true byte stream
// and true 64-bit positions in a std::map and decides per call which true bytes are delivered, in which
// order, and where a run starts. Every call is made three ways from the same starting table: with a
// pattern into outputs of exactly the needed size, with a pattern into outputs one byte and one run
// short, and without a pattern; the first is held to bt::flowreasm_host's table, hit, rest and result
// byte for byte. Every table, id array, word array, frame buffer and output is a heap block of exactly
// its size (an access past it is an AddressSanitizer report). No device, no Python, no library to load;
// the pattern compiler is compiled in:
//
//   g++ -std=c++17 -O1 -g -fsanitize=address,undefined -fno-sanitize-recover=all -Iinclude -Ibeatrice_amd/csrc
//       tools/flowfollow_host_check.cpp beatrice_amd/csrc/bt_regex_dfa.cpp -o tools/flowfollow_host_check
//       && tools/flowfollow_host_check                                                    (one command line)
//
// Exit 0 = all cases hold.
#include <algorithm>
#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <map>
#include <utility>
#include <vector>

#include "beatrice_gpu_bench.h"
#include "bt_flowfollow.h"
#include "bt_flowtcpseq.h"

using namespace bt;
static int g_bad = 0;
#define CHECK(x) do { if (!(x)) { std::printf("FAILED line %d: %s\n", __LINE__, #x); ++g_bad; } } while (0)

static uint32_t g_rng = 24680u;
static uint32_t rnd(uint32_t below) {
    g_rng = g_rng * 1664525u + 1013904223u;
    return (g_rng >> 8) % below;
}

// An Ethernet / IPv4 / TCP (or UDP) frame of flow `port`, direction d, with its payload, appended to data.
static uint64_t put_frame(std::vector<uint8_t>& data, uint32_t port, uint32_t d, uint32_t seq, const uint8_t* pay, uint32_t plen, uint8_t proto) {
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
        t[12] = 0x50; t[13] = 0x18;
    } else {
        t[4] = (uint8_t)((8u + plen) >> 8); t[5] = (uint8_t)(8u + plen);
    }
    if (plen) std::memcpy(t + l4, pay, plen);
    return off | (uint64_t)len << 48;
}

struct Truth {
    int64_t origin = 0, first = 0;  // the true position of byte 0; of the first segment that arrived (the chain's position 0)
    std::vector<uint8_t> bytes;
    size_t cut = 0;                 // the bytes below it have been sent at least once
    bool seen = false, have = false;
    int64_t next = 0;               // delivered up to (true position)
};
struct Sent { uint32_t f, d; int64_t at; uint32_t len; };
struct WantRun { uint32_t flow, flags; uint64_t at; int64_t true_pos; uint64_t len; };

static std::vector<Sent> g_held;
static uint64_t g_tot[4];   // over all cases: delivered bytes, runs, hole runs, runs that continue

static void follow_case(uint32_t n, uint32_t cap, bool bidir, const std::vector<uint8_t>& blob, const FstPattern& pat,
                        std::vector<bt_flow_tcpseq_rec>& seq_table, std::vector<bt_flow_reasm_rec>& table,
                        std::map<std::pair<uint32_t, uint32_t>, Truth>& truth) {
    const uint32_t nw = (n + 63u) / 64u;
    std::vector<uint8_t> data;
    std::vector<uint64_t> desc(n), sel(nw);
    std::vector<uint32_t> ids(n);
    std::vector<Sent> sent(n, Sent{0u, 0u, 0, 0u});
    for (uint32_t w = 0; w < nw; ++w) sel[w] = ((uint64_t)rnd(1u << 16) << 48 | (uint64_t)rnd(1u << 24) << 24 | rnd(1u << 24)) | 0x7777777777777777ull;
    if (n % 64u) sel[nw - 1] |= ~0ull << (n % 64u);   // garbage above n: ignored
    std::vector<Sent> list = g_held;
    g_held.clear();
    while (list.size() < n) {
        const uint32_t f = rnd(cap), d = bidir ? rnd(2) : 0u;
        Truth& t = truth[{f, d}];
        if (t.bytes.empty()) {
            t.origin = ((int64_t)(f + 1u) << 33) - 30 + (int64_t)d * 11;   // close below a multiple of 2^32: wraps at once
            t.bytes.resize(40000);
            for (auto& c : t.bytes) c = (uint8_t)(33u + rnd(90));
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
    for (uint32_t i = 0; i + 1 < n; ++i)
        if (rnd(3) == 0) std::swap(list[i], list[i + 1 + rnd(std::min(6u, n - i - 1u))]);
    for (uint32_t i = 0; i < n; ++i) {
        const Sent& s = list[i];
        const Truth& t = truth[{s.f, s.d}];
        const uint32_t r = rnd(30);
        ids[i] = r == 0 ? 0xFFFFFFFFu - rnd(5) : r == 1 ? cap + rnd(3) : s.f;
        const bool udp = rnd(25) == 0;
        desc[i] = put_frame(data, s.f, s.d, (uint32_t)(uint64_t)s.at, &t.bytes[(size_t)(s.at - t.origin)], s.len, udp ? 17 : 6);
        if (!udp) sent[i] = s;
    }

    // the oracle: true positions only; the directions in ascending (flow, direction), which is the map's order
    std::vector<uint8_t> wbytes;
    std::vector<WantRun> wruns;
    std::vector<uint64_t> wplace(n, UINT64_MAX);
    std::map<std::pair<uint32_t, uint32_t>, std::vector<uint32_t>> mine;
    for (uint32_t i = 0; i < n; ++i) {
        if (!((sel[i / 64u] >> (i % 64u)) & 1u) || ids[i] >= cap || !sent[i].len) continue;
        Truth& t = truth[{ids[i], sent[i].d}];
        if (!t.seen) { t.seen = true; t.first = sent[i].at; }   // the sequence call's origin: the first segment it placed
        mine[{ids[i], sent[i].d}].push_back(i);
    }
    for (auto& kv : mine) {
        Truth& t = truth[kv.first];
        std::vector<std::pair<int64_t, uint32_t>> order;
        for (uint32_t i : kv.second) {
            const int64_t at = sent[i].at, end = at + sent[i].len;
            if (t.have && end <= t.next) continue;   // late
            order.push_back({t.have && at < t.next ? t.next : at, i});
        }
        std::sort(order.begin(), order.end());
        if (order.empty()) continue;
        const bool had = t.have;
        int64_t hi = had ? t.next : order[0].first;
        bool first = true;
        for (auto& o : order) {
            const uint32_t i = o.second;
            const int64_t at = o.first, end = sent[i].at + sent[i].len;
            const bool hole = at > hi;
            if (end <= hi) continue;
            const int64_t from = hole ? at : hi;
            if (first || hole)
                wruns.push_back(WantRun{kv.first.first, kv.first.second | (had ? 0u : BT_FOLLOW_NEW) | (hole ? BT_FOLLOW_HOLE : 0u), wbytes.size(), from, 0});
            first = false;
            wplace[i] = wbytes.size();
            for (int64_t p = from; p < end; ++p) wbytes.push_back(t.bytes[(size_t)(p - t.origin)]);
            wruns.back().len += (uint64_t)(end - from);
            hi = end;
        }
        t.next = hi;
        t.have = true;
    }

    // the chain: the sequence call's offsets, then the follow three ways and the reassembly from the same table
    std::vector<int64_t> off(n, 7);
    bt_flow_tcpseq_result qres;
    bt_flow_tcpseq_out qout{nullptr, off.data(), nullptr, &qres, {0, 0}};
    const uint32_t flags = bidir ? BT_FLOWTAB_BIDIRECTIONAL : 0u;
    flowtcpseq_host(data.data(), data.size(), desc.data(), n, ids.data(), sel.data(), flags, seq_table.data(), cap, &qout);
    const std::vector<bt_flow_reasm_rec> before = table;
    const uint64_t total = wbytes.size();
    const uint32_t nruns = (uint32_t)wruns.size();
    char why[160];
    for (int way = 0; way < 3; ++way) {   // 0: exact sizes; 1: one short of each; 2: no pattern
        std::vector<bt_flow_reasm_rec> tab = before;
        const uint64_t ocap = way == 1 && total ? total - 1u : total;
        const uint32_t rcap = way == 1 && nruns ? nruns - 1u : nruns;
        std::vector<uint8_t> ob(ocap, 0xEE);
        std::vector<bt_flow_follow_run> runs(rcap);
        std::vector<uint64_t> place(n, 5), hit(nw, 0xDEADull), rest(nw, 0xDEADull);
        bt_flow_reasm_result res;
        bt_flow_follow_result fres;
        std::memset(&res, 0xEE, sizeof(res));
        std::memset(&fres, 0xEE, sizeof(fres));
        bt_flow_reasm_out out{hit.data(), rest.data(), &res, {0, 0}};
        bt_flow_follow_out fo{ocap ? ob.data() : nullptr, ocap, rcap ? runs.data() : nullptr, rcap, 0u, place.data(), &fres, {0, 0}};
        FstPattern p2;
        bool with = false;
        const void* const pp = way == 2 ? nullptr : blob.data();
        CHECK(flowfollow_host_args(data.data(), data.size(), desc.data(), n, ids.data(), sel.data(), off.data(), flags, pp,
                                   way == 2 ? 0u : (uint32_t)blob.size(), tab.data(), cap, &out, &fo, &p2, &with, why, sizeof(why)) == BT_OK);
        CHECK(with == (way != 2));
        flowfollow_host(data.data(), data.size(), desc.data(), n, ids.data(), sel.data(), off.data(), flags, pp, way == 2 ? p2 : pat, tab.data(), cap, &out, &fo);
        CHECK(fres.total == total && fres.n_runs == nruns && fres.written == ocap && fres.runs_written == rcap && fres.reserved == 0);
        CHECK(res.stream_bytes == total);
        CHECK(std::equal(ob.begin(), ob.end(), wbytes.begin()));
        CHECK(place == wplace);
        for (uint32_t k = 0; k < rcap; ++k) {
            const Truth& t = truth[{wruns[k].flow, wruns[k].flags & 1u}];
            CHECK(runs[k].flow == wruns[k].flow && runs[k].flags == wruns[k].flags && runs[k].at == wruns[k].at && runs[k].len == wruns[k].len);
            CHECK(runs[k].pos == wruns[k].true_pos - t.first);   // the chain's positions count from the first segment placed
        }
        if (way == 0) {
            std::vector<bt_flow_reasm_rec> rtab = before;
            std::vector<uint64_t> rhit(nw, 0xDEADull), rrest(nw, 0xDEADull);
            bt_flow_reasm_result rres;
            bt_flow_reasm_out rout{rhit.data(), rrest.data(), &rres, {0, 0}};
            flowreasm_host(data.data(), data.size(), desc.data(), n, ids.data(), sel.data(), off.data(), flags, blob.data(), pat, rtab.data(), cap, &rout);
            CHECK(std::memcmp(&rres, &res, sizeof(res)) == 0 && rhit == hit && rrest == rest);
            CHECK(std::memcmp(rtab.data(), tab.data(), cap * sizeof(bt_flow_reasm_rec)) == 0);
            table = tab;
            g_tot[0] += total; g_tot[1] += nruns;
            for (const WantRun& u : wruns) { g_tot[2] += (u.flags & BT_FOLLOW_HOLE) ? 1u : 0u; g_tot[3] += (u.flags & ~1u) ? 0u : 1u; }
        }
        if (way == 2) {
            CHECK(res.hit_packets == 0 && res.new_hit_flows == 0);
            for (uint64_t w : hit) CHECK(w == 0);
            for (uint32_t f = 0; f < cap; ++f)
                for (uint32_t d = 0; d < 2; ++d) {
                    CHECK(tab[f].d[d].next == table[f].d[d].next && tab[f].d[d].have == table[f].d[d].have && tab[f].d[d].holes == table[f].d[d].holes);
                    if (tab[f].d[d].stream_packets != before[f].d[d].stream_packets) CHECK(tab[f].d[d].d == 0);
                }
        }
    }
}

int main() {
    static const char kPattern[] = "HE.LO|ABBA";
    uint32_t size = 0;
    bt_flow_stream_info info;
    char why[160];
    CHECK(flowstream_compile(kPattern, nullptr, 0, &size, &info, why, sizeof(why)) == BT_OK);
    std::vector<uint8_t> blob(size);
    CHECK(flowstream_compile(kPattern, blob.data(), size, &size, &info, why, sizeof(why)) == BT_OK);
    FstPattern pat;
    CHECK(flowstream_pattern(blob.data(), size, &pat, why, sizeof(why)) == BT_OK);

    for (int round = 0; round < 12; ++round) {
        const uint32_t cap = round % 4 == 3 ? 1u : 3u + rnd(4);
        const bool bidir = round % 2 == 0;
        std::vector<bt_flow_tcpseq_rec> seq_table(cap);
        std::vector<bt_flow_reasm_rec> table(cap);
        std::memset(seq_table.data(), 0, cap * sizeof(bt_flow_tcpseq_rec));
        std::memset(table.data(), 0, cap * sizeof(bt_flow_reasm_rec));
        std::map<std::pair<uint32_t, uint32_t>, Truth> truth;
        g_held.clear();
        static const uint32_t sizes[] = {65, 1, 63, 64, 130, 200};
        for (int call = 0; call < 6; ++call) follow_case(sizes[(round + call) % 6], cap, bidir, blob, pat, seq_table, table, truth);
    }
    {   // n == 0: both results and nothing else
        std::vector<bt_flow_reasm_rec> table(2);
        std::memset(table.data(), 0, 2 * sizeof(bt_flow_reasm_rec));
        bt_flow_reasm_result res;
        bt_flow_follow_result fres;
        std::memset(&res, 0xEE, sizeof(res));
        std::memset(&fres, 0xEE, sizeof(fres));
        bt_flow_reasm_out out{nullptr, nullptr, &res, {0, 0}};
        bt_flow_follow_out fo{nullptr, 0, nullptr, 0, 0, nullptr, &fres, {0, 0}};
        flowfollow_host(nullptr, 0, nullptr, 0, nullptr, nullptr, nullptr, 0, nullptr, FstPattern{}, table.data(), 2, &out, &fo);
        CHECK(res.n == 0 && res.stream_bytes == 0 && fres.total == 0 && fres.written == 0 && fres.n_runs == 0 && fres.runs_written == 0 && fres.reserved == 0);
    }

    // the argument checks of the device form, and the layout an accepted call resolves to
    {
        std::vector<uint8_t> frames(256), ob(64);
        std::vector<uint64_t> desc(4), words(2), more(2), place(2);
        std::vector<uint32_t> ids(4);
        std::vector<int64_t> off(4);
        std::vector<bt_flow_reasm_rec> table(4);
        std::vector<bt_flow_follow_run> runs(2);
        bt_flow_reasm_result res;
        bt_flow_follow_result fres;
        const FfLayout l = ff_layout(2, 4);
        std::vector<uint8_t> raw(l.total + 512);
        void* const scratch = reinterpret_cast<void*>((reinterpret_cast<uintptr_t>(raw.data()) + 255u) & ~(uintptr_t)255u);
        bt_batch b{};
        b.base = frames.data(); b.desc = desc.data(); b.n = 2; b.bytes = 256; b.desc_format = BT_DESC_PACKED;
        bt_flow_reasm_out out{words.data(), more.data(), &res, {0, 0}};
        const bt_flow_follow_out good{ob.data(), 64, runs.data(), 2, 0, place.data(), &fres, {0, 0}};
        FlowreasmArgs a;
        FlowfollowArgs f;
        const auto call = [&](const void* p, const void* pd, uint32_t pb, uint64_t nbytes, const bt_flow_follow_out* fo) {
            return flowfollow_args(&b, ids.data(), words.data(), off.data(), 0, p, pd, pb, table.data(), 4, scratch, nbytes, &out, fo, &a, &f, why, sizeof(why));
        };
        CHECK(call(blob.data(), blob.data(), size, l.total, &good) == BT_OK);
        CHECK(l.fr.total == fr_layout(2, 4).total && l.at == l.fr.total && l.at < l.src && l.src < l.runat && l.runat < l.carry && l.carry < l.head);
        CHECK(reinterpret_cast<uint8_t*>(f.fhead) + ft_round(sizeof(FfHead)) == static_cast<uint8_t*>(scratch) + l.total);
        CHECK(reinterpret_cast<uint8_t*>(f.at) == static_cast<uint8_t*>(scratch) + l.at && f.bytes == 256 && f.cap == 64 && f.run_cap == 2);
        CHECK(call(nullptr, nullptr, 0, l.total, &good) == BT_OK);
        CHECK(call(blob.data(), blob.data(), size, l.total - 1, &good) == BT_E_INVALID_ARGUMENT && std::strstr(why, "scratch_bytes"));
        CHECK(call(blob.data(), blob.data(), size, l.total, nullptr) == BT_E_INVALID_ARGUMENT && std::strstr(why, "null fo"));
        CHECK(call(nullptr, blob.data(), size, l.total, &good) == BT_E_INVALID_ARGUMENT && std::strstr(why, "null pattern"));
        CHECK(call(blob.data(), nullptr, size, l.total, &good) == BT_E_INVALID_ARGUMENT && std::strstr(why, "null pattern_device"));
        CHECK(call(nullptr, nullptr, size, l.total, &good) == BT_E_INVALID_ARGUMENT && std::strstr(why, "without a pattern"));
        bt_flow_follow_out x = good;
        x.bytes = nullptr;
        CHECK(call(blob.data(), blob.data(), size, l.total, &x) == BT_E_INVALID_ARGUMENT && std::strstr(why, "null bytes"));
        x = good; x.bytes = frames.data() + 250;
        CHECK(call(blob.data(), blob.data(), size, l.total, &x) == BT_E_INVALID_ARGUMENT && std::strstr(why, "overlaps"));
        x = good; x.reserved[1] = 1;
        CHECK(call(blob.data(), blob.data(), size, l.total, &x) == BT_E_INVALID_ARGUMENT && std::strstr(why, "reserved"));
        x = good; x.result = nullptr;
        CHECK(call(blob.data(), blob.data(), size, l.total, &x) == BT_E_INVALID_ARGUMENT && std::strstr(why, "null fo->result"));
        uint64_t last = 0;
        for (uint32_t n : {0u, 1u, 64u, 65u, 16384u, 16385u, 1u << 20}) {
            const FfLayout y = ff_layout(n, 1000);
            CHECK(y.total >= last && y.total % 256u == 0 && y.total > y.fr.total);
            last = y.total;
        }
    }
    std::printf("delivered %llu bytes, runs %llu, behind a hole %llu, continuing %llu\n", (unsigned long long)g_tot[0], (unsigned long long)g_tot[1],
                (unsigned long long)g_tot[2], (unsigned long long)g_tot[3]);
    for (uint64_t v : g_tot) CHECK(v > 20);   // the cases are not vacuous
    std::printf(g_bad ? "flowfollow_host_check: %d check(s) FAILED\n" : "flowfollow_host_check: all checks hold\n", g_bad);
    return g_bad ? 1 : 0;
}
