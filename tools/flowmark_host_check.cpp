// flowmark_host_check.cpp — the mark side table's host part from beatrice_amd/csrc/bt_flowmark.h
// under the host sanitizers: the argument checks of bt_flow_mark_update_device / _host and of
// bt_flow_mark_select_device / _host (refusals, and accepted calls with the launch arguments they
// resolve to), the update on the host (bt::flowmark_host) and the selection on the host
// (bt::flowmark_sel_host) over generated ids, lengths, hit words and stamps, each held to a naive
// per-flow loop over a std::map. Every table, id array and word array is a heap block of exactly
// its size (an access past it is an AddressSanitizer report). No device, no Python, no library
// to load:
//
//   g++ -std=c++17 -O1 -g -fsanitize=address,undefined -fno-sanitize-recover=all -Iinclude -Ibeatrice_amd/csrc
//       tools/flowmark_host_check.cpp -o tools/flowmark_host_check && tools/flowmark_host_check   (one command line)
//
// Exit 0 = all cases hold.
#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <map>
#include <vector>

#include "bt_flowmark.h"

using namespace bt;
static int g_bad = 0;
#define CHECK(x) do { if (!(x)) { std::printf("FAILED line %d: %s\n", __LINE__, #x); ++g_bad; } } while (0)

static uint32_t g_rng = 4321u;
static uint32_t rnd(uint32_t below) {
    g_rng = g_rng * 1664525u + 1013904223u;
    return (g_rng >> 8) % below;
}

struct Naive { uint32_t marks = 0, packets = 0; uint64_t bytes = 0, first_c = 0, last = 0; };

static bool is_sentinel(uint32_t id) { return id == 0xFFFFFFFFu || id == 0xFFFFFFFEu || id == 0xFFFFFFFDu || id == 0xFFFFFFFBu; }

// One update of n packets into `table` and into the naive map; both results compared.
static void update_case(uint32_t n, uint32_t cap, int hit_kind, bool with_ts, uint32_t mark, std::vector<bt_flow_mark_rec>& table,
                        std::map<uint32_t, Naive>& naive, uint32_t distinct) {
    const uint32_t nw = (n + 63u) / 64u;
    std::vector<uint64_t> desc(n), ts(n), hit(nw);
    std::vector<uint32_t> ids(n);
    for (uint32_t i = 0; i < n; ++i) {
        desc[i] = ((uint64_t)(rnd(8) == 0 ? 65535u : 40u + rnd(1500)) << 48) | (uint64_t)i * 2048u;
        const uint32_t r = rnd(16);
        ids[i] = r == 0 ? 0xFFFFFFFFu - rnd(5) : r == 1 ? cap + rnd(3) : rnd(distinct ? distinct : 1u);
        ts[i] = rnd(64) == 0 ? ~0ull : rnd(64) == 1 ? 0ull : 1000u + rnd(100000);
    }
    for (uint32_t w = 0; w < nw; ++w)
        hit[w] = hit_kind == 0 ? 0ull : hit_kind == 1 ? ~0ull : ((uint64_t)rnd(1u << 16) << 48 | (uint64_t)rnd(1u << 24) << 24 | rnd(1u << 24));
    if (n % 64u && hit_kind != 0) hit[nw - 1] |= ~0ull << (n % 64u);   // garbage above n: ignored
    const bt_flow_mark_update upd{mark, 0u, with_ts ? ts.data() : nullptr, 777u};
    bt_flow_mark_result want{};
    want.n = n;
    std::map<uint32_t, bool> lacked;
    for (uint32_t i = 0; i < n; ++i) {
        if (hit_kind != 3 && !((hit[i / 64u] >> (i % 64u)) & 1u)) continue;
        ++want.hit_packets;
        const uint32_t id = ids[i];
        if (id >= cap) { if (is_sentinel(id)) ++want.unkeyed_hits; else ++want.bad_ids; continue; }
        Naive& f = naive[id];
        if (!lacked.count(id)) lacked[id] = (f.marks & mark) != mark;
        const uint64_t t = with_ts ? ts[i] : 777u;
        const uint32_t len = (uint32_t)(desc[i] >> 48);
        f.marks |= mark; f.packets += 1; f.bytes += len < 65535u ? len : 65535u;
        if (~t > f.first_c) f.first_c = ~t;
        if (t > f.last) f.last = t;
        ++want.marked_packets;
    }
    for (const auto& kv : lacked) want.new_marked_flows += kv.second ? 1u : 0u;
    bt_flow_mark_result got;
    memset(&got, 0xAB, sizeof(got));
    char why[128];
    CHECK(flowmark_host_args(desc.data(), n, ids.data(), hit_kind == 3 ? nullptr : hit.data(), &upd, table.data(), cap, &got, why, sizeof(why)));
    flowmark_host(desc.data(), n, ids.data(), hit_kind == 3 ? nullptr : hit.data(), &upd, table.data(), cap, &got);
    CHECK(memcmp(&got, &want, sizeof(got)) == 0);
    for (uint32_t f = 0; f < cap; ++f) {
        const Naive x = naive.count(f) ? naive[f] : Naive{};
        const bt_flow_mark_rec& r = table[f];
        CHECK(r.marks == x.marks && r.hit_packets == x.packets && r.hit_bytes == x.bytes && r.first_hit_ts_c == x.first_c && r.last_hit_ts == x.last);
    }
}

static void select_case(uint32_t n, uint32_t cap, const std::vector<bt_flow_mark_rec>& table, uint32_t mask, uint32_t flags, uint32_t op,
                        bool in_place) {
    const uint32_t nw = (n + 63u) / 64u;
    std::vector<uint32_t> ids(n);
    std::vector<uint64_t> base(nw), out(nw, 0x5555555555555555ull), want(nw, 0);
    for (uint32_t i = 0; i < n; ++i) ids[i] = rnd(12) == 0 ? 0xFFFFFFFFu - rnd(5) : rnd(12) == 1 ? cap + rnd(2) : rnd(cap ? cap : 1u);
    for (uint32_t w = 0; w < nw; ++w) base[w] = (uint64_t)rnd(1u << 16) << 48 | (uint64_t)rnd(1u << 24) << 24 | rnd(1u << 24);
    if (n % 64u) base[nw - 1] |= ~0ull << (n % 64u);
    bt_flow_mark_select_result wr{};
    wr.n = n;
    for (uint32_t i = 0; i < n; ++i) {
        bool m = false;
        if (ids[i] < cap) {
            const uint32_t got = table[ids[i]].marks & mask;
            m = (flags & BT_FLOW_MARK_ALL_BITS) ? got == mask : got != 0;
        } else if (!is_sentinel(ids[i])) {
            ++wr.bad_ids;
        }
        const bool b = (base[i / 64u] >> (i % 64u)) & 1u;
        const bool o = op == BT_FLOW_MARK_SET ? m : op == BT_FLOW_MARK_AND ? (b && m) : op == BT_FLOW_MARK_OR ? (b || m) : (b && !m);
        wr.n_marked += m; wr.n_out += o;
        if (o) want[i / 64u] |= 1ull << (i % 64u);
    }
    const bt_flow_mark_select_opts opts{mask, flags, op, 0u};
    bt_flow_mark_select_result got;
    memset(&got, 0xCD, sizeof(got));
    uint64_t* const to = in_place ? base.data() : out.data();
    FlowmarkSelArgs a;
    char why[128];
    CHECK(flowmark_sel_args(ids.data(), n, table.data(), cap, &opts, base.data(), to, &got, &a, why, sizeof(why)));
    CHECK(a.ntiles == nw && a.nchunks == (nw + kFtChunkTiles - 1u) / kFtChunkTiles && (n == 0 || (a.base == nullptr) == (op == BT_FLOW_MARK_SET)));
    flowmark_sel_host(a);
    CHECK(memcmp(&got, &wr, sizeof(got)) == 0);
    CHECK(nw == 0 || memcmp(to, want.data(), nw * 8u) == 0);
}

static void refusals() {
    std::vector<uint64_t> desc(4), words(1), ts(4);
    std::vector<uint32_t> ids(4);
    std::vector<bt_flow_mark_rec> table(4);
    bt_flow_mark_result res;
    bt_flow_mark_select_result sres;
    char why[128];
    const bt_flow_mark_update ok{1u, 0u, ts.data(), 0u};
    const auto no = [&](const char* word, const bt_flow_mark_update* u, const uint32_t* id, const uint64_t* hit, const bt_flow_mark_rec* t,
                        const bt_flow_mark_result* r, const bt_pkt_desc* d) {
        why[0] = 0;
        CHECK(!flowmark_host_args(d, 4, id, hit, u, t, 4, r, why, sizeof(why)));
        CHECK(strstr(why, word) != nullptr);
    };
    const bt_pkt_desc* d = reinterpret_cast<const bt_pkt_desc*>(desc.data());
    CHECK(flowmark_host_args(d, 4, ids.data(), words.data(), &ok, table.data(), 4, &res, why, sizeof(why)));
    CHECK(flowmark_host_args(nullptr, 0, nullptr, nullptr, &ok, nullptr, 0, &res, why, sizeof(why)));
    no("null desc", &ok, ids.data(), nullptr, table.data(), &res, nullptr);
    no("null flow_id", &ok, nullptr, nullptr, table.data(), &res, d);
    no("null upd", nullptr, ids.data(), nullptr, table.data(), &res, d);
    no("null mark_table", &ok, ids.data(), nullptr, nullptr, &res, d);
    no("null result", &ok, ids.data(), nullptr, table.data(), nullptr, d);
    const bt_flow_mark_update zero{0u, 0u, nullptr, 0u}, resv{1u, 2u, nullptr, 0u};
    const bt_flow_mark_update odd{1u, 0u, reinterpret_cast<const uint64_t*>(reinterpret_cast<const char*>(ts.data()) + 4), 0u};
    no("mark is 0", &zero, ids.data(), nullptr, table.data(), &res, d);
    no("reserved", &resv, ids.data(), nullptr, table.data(), &res, d);
    no("ts is not 8-byte aligned", &odd, ids.data(), nullptr, table.data(), &res, d);
    no("mark_table is not 8-byte aligned", &ok, ids.data(), nullptr,
       reinterpret_cast<const bt_flow_mark_rec*>(reinterpret_cast<const char*>(table.data()) + 4), &res, d);
    no("hit is not 8-byte aligned", &ok, ids.data(), reinterpret_cast<const uint64_t*>(reinterpret_cast<const char*>(words.data()) + 4),
       table.data(), &res, d);
    // the device form: a batch, and the launch arguments it resolves to
    bt_batch b{};
    std::vector<uint8_t> bytes(256);
    b.base = bytes.data(); b.desc = desc.data(); b.n = 4; b.bytes = 256;
    FlowmarkArgs a;
    CHECK(flowmark_args(&b, ids.data(), words.data(), &ok, table.data(), 4, &res, &a, why, sizeof(why)));
    CHECK(a.n == 4 && a.ntiles == 1 && a.nchunks == 1 && a.mark == 1 && a.flow_cap == 4 && a.hit == words.data() && a.ts == ts.data());
    CHECK(!flowmark_args(nullptr, ids.data(), words.data(), &ok, table.data(), 4, &res, &a, why, sizeof(why)) && strstr(why, "null frames"));
    b.flags = BT_BATCH_PREFIXES;
    CHECK(!flowmark_args(&b, ids.data(), words.data(), &ok, table.data(), 4, &res, &a, why, sizeof(why)) && strstr(why, "BT_BATCH_PREFIXES"));
    b.flags = 0; b.bytes = 0;
    CHECK(!flowmark_args(&b, ids.data(), words.data(), &ok, table.data(), 4, &res, &a, why, sizeof(why)) && strstr(why, "bytes == 0"));
    // the selection
    FlowmarkSelArgs s;
    const auto sel_no = [&](const char* word, bt_flow_mark_select_opts o, const uint64_t* base) {
        why[0] = 0;
        CHECK(!flowmark_sel_args(ids.data(), 4, table.data(), 4, &o, base, words.data(), &sres, &s, why, sizeof(why)));
        CHECK(strstr(why, word) != nullptr);
    };
    sel_no("mask is 0", {0u, 0u, 0u, 0u}, nullptr);
    sel_no("unknown flag", {1u, 2u, 0u, 0u}, nullptr);
    sel_no("unknown op", {1u, 0u, 4u, 0u}, nullptr);
    sel_no("reserved", {1u, 0u, 0u, 1u}, nullptr);
    sel_no("needs base", {1u, 0u, BT_FLOW_MARK_AND, 0u}, nullptr);
    sel_no("needs base", {1u, 0u, BT_FLOW_MARK_OR, 0u}, nullptr);
    sel_no("needs base", {1u, 0u, BT_FLOW_MARK_ANDNOT, 0u}, nullptr);
    const bt_flow_mark_select_opts set{1u, 0u, BT_FLOW_MARK_SET, 0u};
    CHECK(!flowmark_sel_args(ids.data(), 4, table.data(), 4, nullptr, nullptr, words.data(), &sres, &s, why, sizeof(why)) && strstr(why, "null opts"));
    CHECK(!flowmark_sel_args(nullptr, 4, table.data(), 4, &set, nullptr, words.data(), &sres, &s, why, sizeof(why)) && strstr(why, "null flow_id"));
    CHECK(!flowmark_sel_args(ids.data(), 4, table.data(), 4, &set, nullptr, nullptr, &sres, &s, why, sizeof(why)) && strstr(why, "null out_select"));
    CHECK(!flowmark_sel_args(ids.data(), 4, nullptr, 4, &set, nullptr, words.data(), &sres, &s, why, sizeof(why)) && strstr(why, "null mark_table"));
    CHECK(!flowmark_sel_args(ids.data(), 4, table.data(), 4, &set, nullptr, words.data(), nullptr, &s, why, sizeof(why)) && strstr(why, "null result"));
    CHECK(flowmark_sel_args(nullptr, 0, nullptr, 0, &set, nullptr, nullptr, &sres, &s, why, sizeof(why)) && s.ntiles == 0 && s.nchunks == 0);
}

int main() {
    refusals();
    const uint32_t sizes[] = {0, 1, 63, 64, 65, 1000, 16385};
    for (uint32_t n : sizes)
        for (uint32_t cap : {0u, 1u, 7u, 300u}) {
            std::vector<bt_flow_mark_rec> table(cap);   // zeroed once; three updates into it
            std::map<uint32_t, Naive> naive;
            update_case(n, cap, 2, true, 0x1u, table, naive, cap);
            update_case(n, cap, 3, false, 0x80000000u, table, naive, cap > 3 ? 3u : cap);
            update_case(n, cap, 1, true, 0x80000001u, table, naive, cap);
            update_case(n, cap, 0, true, 0x2u, table, naive, cap);
            for (uint32_t op = 0; op < 4; ++op)
                for (uint32_t flags = 0; flags < 2; ++flags) {
                    select_case(n, cap, table, 0x80000001u, flags, op, false);
                    select_case(n, cap, table, 0x2u, flags, op, true);
                }
        }
    if (g_bad) { std::printf("%d checks FAILED\n", g_bad); return 1; }
    std::printf("all cases hold\n");
    return 0;
}
