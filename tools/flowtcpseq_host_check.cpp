// flowtcpseq_host_check.cpp — the TCP sequence side table's host part from
// beatrice_amd/csrc/bt_flowtcpseq.h under the host sanitizers: the argument checks of
// bt_flow_tcpseq_device / _host (refusals, and an accepted call with the launch arguments and the
// scratch layout it resolves to) and the classification on the host (bt::flowtcpseq_host) over
// generated conversations, held to an oracle that never sees a wire sequence number: it keeps every
// direction's true 64-bit offsets (origin and highest end) in a std::map. The generator walks each
// direction forward with losses, duplicates, steps back and overlaps, from true offsets far above
// 2^32, so the wire numbers wrap. Every table, id array, word array, frame buffer and output is a
// heap block of exactly its size (an access past it is an AddressSanitizer report). No device, no
// Python, no library to load:
//
//   g++ -std=c++17 -O1 -g -fsanitize=address,undefined -fno-sanitize-recover=all -Iinclude -Ibeatrice_amd/csrc
//       tools/flowtcpseq_host_check.cpp -o tools/flowtcpseq_host_check && tools/flowtcpseq_host_check   (one command line)
//
// Exit 0 = all cases hold.
#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <map>
#include <utility>
#include <vector>

#include "bt_flowtcpseq.h"

using namespace bt;
static int g_bad = 0;
#define CHECK(x) do { if (!(x)) { std::printf("FAILED line %d: %s\n", __LINE__, #x); ++g_bad; } } while (0)

static uint32_t g_rng = 24680u;
static uint32_t rnd(uint32_t below) {
    g_rng = g_rng * 1664525u + 1013904223u;
    return (g_rng >> 8) % below;
}

static bool is_sentinel(uint32_t id) { return id == 0xFFFFFFFFu || id == 0xFFFFFFFEu || id == 0xFFFFFFFDu || id == 0xFFFFFFFBu; }

// An Ethernet / IPv4 / TCP frame of flow `port`, direction d, with `plen` payload bytes by its header
// (the frame itself holds at most 8 of them: a snapped capture), appended to data.
static uint64_t put_frame(std::vector<uint8_t>& data, uint32_t port, uint32_t d, uint32_t seq, uint32_t plen, uint8_t flags, uint8_t proto) {
    const uint32_t held = plen < 8u ? plen : 8u, len = 14u + 20u + 20u + held;
    const uint64_t off = data.size();
    data.resize(off + len, 0u);
    uint8_t* f = data.data() + off;
    f[12] = 0x08;
    uint8_t* ip = f + 14;
    ip[0] = 0x45;
    ip[2] = (uint8_t)((40u + plen) >> 8); ip[3] = (uint8_t)(40u + plen);
    ip[8] = 64; ip[9] = proto;
    const uint8_t a[4] = {10, 0, 0, 1}, b[4] = {10, 0, 0, 2};
    std::memcpy(ip + 12, d ? b : a, 4);
    std::memcpy(ip + 16, d ? a : b, 4);
    uint8_t* t = ip + 20;
    const uint32_t sp = d ? 80u : 1024u + port, dp = d ? 1024u + port : 80u;
    t[0] = (uint8_t)(sp >> 8); t[1] = (uint8_t)sp; t[2] = (uint8_t)(dp >> 8); t[3] = (uint8_t)dp;
    t[4] = (uint8_t)(seq >> 24); t[5] = (uint8_t)(seq >> 16); t[6] = (uint8_t)(seq >> 8); t[7] = (uint8_t)seq;
    t[12] = 0x50; t[13] = flags;
    return off | (uint64_t)len << 48;
}

struct Seen { int64_t origin, hi, last; uint32_t last_seq; uint32_t seq, old, gap, ovl; uint64_t oldb, gapb; };

// One call of n packets over `flows` connections against `table`; `where` keeps every direction's true
// position between the calls of one table.
static void classify_case(uint32_t n, uint32_t cap, uint32_t flows, int sel_kind, int outs, bool in_place, bool bidir,
                          std::vector<bt_flow_tcpseq_rec>& table, std::map<std::pair<uint32_t, uint32_t>, Seen>& truth,
                          std::map<std::pair<uint32_t, uint32_t>, int64_t>& cursor) {
    const uint32_t nw = (n + 63u) / 64u;
    std::vector<uint8_t> data;
    std::vector<uint64_t> desc(n), sel(nw);
    std::vector<uint32_t> ids(n);
    std::vector<int64_t> toff(n);
    std::vector<uint32_t> tl(n), tdir(n);
    for (uint32_t w = 0; w < nw; ++w)
        sel[w] = sel_kind == 0 ? 0ull : sel_kind == 1 ? ~0ull : ((uint64_t)rnd(1u << 16) << 48 | (uint64_t)rnd(1u << 24) << 24 | rnd(1u << 24)) | 0x1111111111111111ull;
    if (n % 64u && sel_kind != 0) sel[nw - 1] |= ~0ull << (n % 64u);   // garbage above n: ignored
    const bool all = sel_kind == 3;
    for (uint32_t i = 0; i < n; ++i) {
        const uint32_t r = rnd(24), f = rnd(flows ? flows : 1u), d = rnd(2);
        ids[i] = r == 0 ? 0xFFFFFFFFu - rnd(5) : r == 1 ? cap + rnd(3) : f;
        int64_t& at = cursor[{f, bidir ? d : 0u}];   // the next in-order true offset of the direction the table sees
        if (at == 0) at = ((int64_t)(f + 1u) << 33) - 40 + (int64_t)d * 7;   // close below a multiple of 2^32: wraps at once
        const uint32_t kind = rnd(12);
        uint32_t plen = kind == 10 ? 0u : 1u + rnd(1460);
        const uint8_t flags = kind == 11 ? (uint8_t)(0x02 | (rnd(2) ? 0x10 : 0)) : kind == 9 ? 0x11 : kind == 10 ? (uint8_t)(rnd(2) ? 0x14 : 0x10) : 0x18;
        const uint32_t L = plen + ((flags & 2) ? 1u : 0u) + ((flags & 1) ? 1u : 0u);
        int64_t off = at;
        const uint32_t op = rnd(10);
        if (op == 0) off = at + 1 + rnd(3000);                  // a loss in front
        else if (op == 1) off = at - 1 - (int64_t)rnd(3000);    // a step back: old or overlapping
        else if (op == 2) off = at - (int64_t)L;                // a whole retransmit
        const bool udp = rnd(40) == 0;
        toff[i] = off;
        tl[i] = udp ? 0u : L;
        tdir[i] = bidir ? d : 0u;
        desc[i] = put_frame(data, f, d, (uint32_t)(uint64_t)off, plen, flags, udp ? 17 : 6);
        // the direction moves on only if the call will take the packet
        const bool taken = (all || ((sel[i / 64u] >> (i % 64u)) & 1u)) && ids[i] < cap && !udp && L;
        if (taken && ids[i] == f && off + (int64_t)L > at) at = off + (int64_t)L;
    }

    // the oracle: true offsets only
    std::vector<uint8_t> wcls(n, BT_TCPSEQ_NONE);
    std::vector<int64_t> woff(n, BT_TCPSEQ_OFF_NONE);
    std::vector<uint64_t> wout(nw, 0ull);
    bt_flow_tcpseq_result want{};
    want.n = n;
    for (uint32_t i = 0; i < n; ++i) {
        if (!all && !((sel[i / 64u] >> (i % 64u)) & 1u)) continue;
        ++want.selected;
        wout[i / 64u] |= 1ull << (i % 64u);
        if (ids[i] >= cap) {
            if (is_sentinel(ids[i])) ++want.unkeyed; else ++want.bad_ids;
            continue;
        }
        if (!tl[i]) continue;
        const int64_t u0 = toff[i], e = u0 + tl[i];
        auto it = truth.find({ids[i], tdir[i]});
        uint8_t k;
        if (it == truth.end()) {
            it = truth.insert({{ids[i], tdir[i]}, Seen{u0, e, u0, 0, 0, 0, 0, 0, 0, 0}}).first;
            k = BT_TCPSEQ_FIRST;
            ++want.first;
        } else {
            Seen& t = it->second;
            if (u0 == t.hi) { k = BT_TCPSEQ_IN_ORDER; ++want.in_order; }
            else if (u0 > t.hi) { k = BT_TCPSEQ_GAP; ++want.gap; ++t.gap; t.gapb += (uint64_t)(u0 - t.hi); want.gap_bytes += (uint64_t)(u0 - t.hi); }
            else if (e <= t.hi) { k = BT_TCPSEQ_OLD; ++want.old; ++t.old; t.oldb += tl[i]; want.old_bytes += tl[i]; wout[i / 64u] &= ~(1ull << (i % 64u)); }
            else { k = BT_TCPSEQ_OVERLAP; ++want.overlap; ++t.ovl; t.oldb += (uint64_t)(t.hi - u0); want.old_bytes += (uint64_t)(t.hi - u0); }
            if (e > t.hi) t.hi = e;
        }
        Seen& t = it->second;
        t.last = u0;
        t.last_seq = (uint32_t)(uint64_t)u0;
        ++t.seq;
        ++want.seq_packets;
        want.seq_bytes += tl[i];
        wcls[i] = k;
        woff[i] = u0 - t.origin;
    }

    std::vector<uint8_t> cls(n, 0x5A);
    std::vector<int64_t> off(n, 0x5A5A5A5A5A5A5A5All);
    std::vector<uint64_t> out(nw, 0x5A5A5A5A5A5A5A5Aull);
    if (in_place) out = sel;
    const uint64_t* const select = all ? nullptr : in_place ? out.data() : sel.data();
    bt_flow_tcpseq_result got;
    std::memset(&got, 0xEE, sizeof(got));
    const bt_flow_tcpseq_out o{(outs & 1) ? cls.data() : nullptr, (outs & 2) ? off.data() : nullptr, (outs & 4) || in_place ? out.data() : nullptr,
                               &got, {0, 0}};
    const uint32_t tflags = bidir ? BT_FLOWTAB_BIDIRECTIONAL : 0u;
    char why[128];
    if (data.empty()) data.push_back(0);
    CHECK(flowtcpseq_host_args(data.data(), desc.data(), n, ids.data(), select, tflags, table.data(), cap, &o, why, sizeof(why)));
    flowtcpseq_host(data.data(), data.size(), desc.data(), n, ids.data(), select, tflags, table.data(), cap, &o);
    CHECK(std::memcmp(&got, &want, sizeof(got)) == 0);
    if (o.cls) CHECK(cls == wcls);
    if (o.off) CHECK(off == woff);
    if (o.out_select) CHECK(out == wout);
    for (uint32_t f = 0; f < cap; ++f)
        for (uint32_t d = 0; d < 2u; ++d) {
            const bt_flow_tcpseq_dir& r = table[f].d[d];
            const auto it = truth.find({f, d});
            if (it == truth.end()) {
                const bt_flow_tcpseq_dir zero{};
                CHECK(std::memcmp(&r, &zero, sizeof(r)) == 0);
                continue;
            }
            const Seen& t = it->second;
            CHECK(r.have == 1u && r.pos == t.last - t.origin && r.hi == t.hi - t.origin && r.last_seq == t.last_seq && r.reserved == 0u);
            CHECK(r.seq_packets == t.seq && r.old_packets == t.old && r.gap_packets == t.gap && r.overlap_packets == t.ovl &&
                  r.old_bytes == t.oldb && r.gap_bytes == t.gapb);
        }
}

static void refusals() {
    alignas(256) static uint8_t scratch[1 << 16];
    uint8_t data[256] = {}, klass[4] = {};
    uint64_t desc[4] = {}, words[2] = {};
    int64_t offs[4] = {};
    uint32_t ids[4] = {};
    bt_flow_tcpseq_rec table[4] = {};
    bt_flow_tcpseq_result res{};
    bt_batch b{};
    b.base = data; b.desc = desc; b.n = 2; b.bytes = 256; b.desc_format = BT_DESC_PACKED;
    const bt_flow_tcpseq_out out{klass, offs, words, &res, {0, 0}};
    FlowtcpseqArgs a;
    char why[128];
    const uint64_t need = fts_layout(2).total;
    CHECK(need <= sizeof(scratch) && need % 256u == 0u);
    const auto dev = [&](const bt_batch* f, const uint32_t* id, const uint64_t* sel, uint32_t flags, bt_flow_tcpseq_rec* t, uint32_t cap,
                         void* s, uint64_t sb, const bt_flow_tcpseq_out* ou) {
        return flowtcpseq_args(f, id, sel, flags, t, cap, s, sb, ou, &a, why, sizeof(why));
    };
    CHECK(dev(&b, ids, words, 3, table, 4, scratch, need, &out));
    CHECK(a.n == 2 && a.ntiles == 1 && a.nchunks == 1 && a.flow_cap == 4 && a.passes == 1 && a.bidir == 1 && a.l3_only == 1 &&
          a.cls == klass && a.off == offs && a.out_select == words && a.result == &res);
    CHECK((uint8_t*)a.head == scratch && (uint8_t*)a.carry + ft_round(kFtWaves * sizeof(FtsCarry)) == scratch + need);
    CHECK(!dev(nullptr, ids, words, 0, table, 4, scratch, need, &out));
    CHECK(!dev(&b, nullptr, words, 0, table, 4, scratch, need, &out));
    CHECK(!dev(&b, ids, words, 4, table, 4, scratch, need, &out));
    CHECK(!dev(&b, ids, words, 0, nullptr, 4, scratch, need, &out));
    CHECK(dev(&b, ids, words, 0, nullptr, 0, scratch, need, &out) && a.passes == 0);
    CHECK(!dev(&b, ids, words, 0, table, 4, scratch, need, nullptr));
    CHECK(!dev(&b, ids, words, 0, table, 4, scratch + 64, need, &out));
    CHECK(!dev(&b, ids, words, 0, table, 4, nullptr, need, &out));
    CHECK(!dev(&b, ids, words, 0, table, 4, scratch, need - 1, &out));
    CHECK(!dev(&b, (const uint32_t*)((uint8_t*)ids + 2), words, 0, table, 4, scratch, need, &out));
    CHECK(!dev(&b, ids, (const uint64_t*)((uint8_t*)words + 4), 0, table, 4, scratch, need, &out));
    CHECK(!dev(&b, ids, words, 0, (bt_flow_tcpseq_rec*)((uint8_t*)table + 4), 4, scratch, need, &out));
    CHECK(!dev(&b, ids, words, 0, table, 0x80000001u, scratch, need, &out));
    const bt_flow_tcpseq_out no_res{klass, offs, words, nullptr, {0, 0}}, bad_res{klass, offs, words, &res, {0, 1}},
        bad_off{klass, (int64_t*)((uint8_t*)offs + 4), words, &res, {0, 0}}, bad_out{klass, offs, (uint64_t*)((uint8_t*)words + 4), &res, {0, 0}},
        odd_cls{klass + 1, nullptr, nullptr, &res, {0, 0}};
    CHECK(!dev(&b, ids, words, 0, table, 4, scratch, need, &no_res));
    CHECK(!dev(&b, ids, words, 0, table, 4, scratch, need, &bad_res));
    CHECK(!dev(&b, ids, words, 0, table, 4, scratch, need, &bad_off));
    CHECK(!dev(&b, ids, words, 0, table, 4, scratch, need, &bad_out));
    CHECK(dev(&b, ids, nullptr, 0, table, 4, scratch, need, &odd_cls));   // class bytes need no alignment
    bt_batch lean = b;
    lean.flags = BT_BATCH_LEAN;
    CHECK(!dev(&lean, ids, words, 0, table, 4, scratch, need, &out));
    bt_batch e = b;
    e.n = 0;
    CHECK(dev(&e, nullptr, nullptr, 0, nullptr, 0, nullptr, 0, &out) && a.n == 0 && a.nchunks == 0);
    uint64_t last = 0;
    for (uint32_t n : {0u, 1u, 64u, 65u, 16384u, 16385u, 1u << 24, 0xFFFFFFFFu}) {
        const uint64_t t = fts_layout(n).total;
        CHECK(t >= last && t % 256u == 0u);
        last = t;
    }
}

int main() {
    refusals();
    const uint32_t sizes[] = {0u, 1u, 63u, 64u, 65u, 1000u, 4099u};
    int k = 0;
    for (uint32_t n : sizes)
        for (uint32_t cap : {0u, 1u, 3u, 40u})
            for (int bidir = 0; bidir < 2; ++bidir) {
                std::vector<bt_flow_tcpseq_rec> table(cap);   // zero; the calls of one (n, cap) go on in the same table
                std::map<std::pair<uint32_t, uint32_t>, Seen> truth;
                std::map<std::pair<uint32_t, uint32_t>, int64_t> cursor;
                for (int sel_kind = 0; sel_kind < 4; ++sel_kind, ++k)
                    classify_case(n, cap, cap ? cap : 1u, sel_kind, k % 8, sel_kind == 2 && (k & 2), bidir != 0, table, truth, cursor);
            }
    if (g_bad) {
        std::printf("%d checks failed\n", g_bad);
        return 1;
    }
    std::printf("flowtcpseq_host_check: all cases hold\n");
    return 0;
}
