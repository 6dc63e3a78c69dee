// flowseq_host_check.cpp — the sequence side table's host part from beatrice_amd/csrc/bt_flowseq.h
// under the host sanitizers: the argument checks of bt_flow_seq_device / _host (refusals, and
// accepted calls with the launch arguments and the scratch layout they resolve to) and the numbering
// on the host (bt::flowseq_host) over generated ids, lengths and select words, held to a naive loop
// flow by flow over a std::map of each flow's packet indices. Every table, id array, word array and
// output is a heap block of exactly its size (an access past it is an AddressSanitizer report). No
// device, no Python, no library to load:
//
//   g++ -std=c++17 -O1 -g -fsanitize=address,undefined -fno-sanitize-recover=all -Iinclude -Ibeatrice_amd/csrc
//       tools/flowseq_host_check.cpp -o tools/flowseq_host_check && tools/flowseq_host_check   (one command line)
//
// Exit 0 = all cases hold.
#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <map>
#include <vector>

#include "bt_flowseq.h"

using namespace bt;
static int g_bad = 0;
#define CHECK(x) do { if (!(x)) { std::printf("FAILED line %d: %s\n", __LINE__, #x); ++g_bad; } } while (0)

static uint32_t g_rng = 97531u;
static uint32_t rnd(uint32_t below) {
    g_rng = g_rng * 1664525u + 1013904223u;
    return (g_rng >> 8) % below;
}

static bool is_sentinel(uint32_t id) { return id == 0xFFFFFFFFu || id == 0xFFFFFFFEu || id == 0xFFFFFFFDu || id == 0xFFFFFFFBu; }

// One call of n packets against `table`; the naive form works flow by flow from a copy of the table.
static void number_case(uint32_t n, uint32_t cap, int sel_kind, uint64_t max_packets, uint64_t max_bytes, uint32_t flags, int outs,
                        bool in_place, std::vector<bt_flow_seq_rec>& table, uint32_t distinct) {
    const uint32_t nw = (n + 63u) / 64u;
    std::vector<uint64_t> desc(n), sel(nw);
    std::vector<uint32_t> ids(n);
    for (uint32_t i = 0; i < n; ++i) {
        desc[i] = ((uint64_t)(rnd(8) == 0 ? 65535u : rnd(16) == 0 ? 0u : 40u + rnd(1500)) << 48) | (uint64_t)i * 2048u;
        const uint32_t r = rnd(16);
        ids[i] = r == 0 ? 0xFFFFFFFFu - rnd(5) : r == 1 ? cap + rnd(3) : rnd(distinct ? distinct : 1u);
    }
    for (uint32_t w = 0; w < nw; ++w)
        sel[w] = sel_kind == 0 ? 0ull : sel_kind == 1 ? ~0ull : ((uint64_t)rnd(1u << 16) << 48 | (uint64_t)rnd(1u << 24) << 24 | rnd(1u << 24));
    if (n % 64u && sel_kind != 0) sel[nw - 1] |= ~0ull << (n % 64u);   // garbage above n: ignored
    const bool all = sel_kind == 3;

    // the naive form: the packets of each flow, then flow by flow
    std::vector<uint32_t> wseq(n, BT_FLOW_SEQ_NONE);
    std::vector<uint64_t> woff(n, BT_FLOW_SEQ_OFF_NONE), wout(nw, 0ull);
    std::vector<bt_flow_seq_rec> wtable = table;
    bt_flow_seq_result want{};
    want.n = n;
    std::map<uint32_t, std::vector<uint32_t>> members;
    for (uint32_t i = 0; i < n; ++i) {
        if (!all && !((sel[i / 64u] >> (i % 64u)) & 1u)) continue;
        ++want.selected;
        if (ids[i] < cap) { members[ids[i]].push_back(i); continue; }
        if (is_sentinel(ids[i])) {
            ++want.unkeyed;
            if (flags & BT_FLOW_SEQ_KEEP_UNKEYED) { wout[i / 64u] |= 1ull << (i % 64u); ++want.kept; }
        } else {
            ++want.bad_ids;
        }
    }
    for (const auto& kv : members) {
        bt_flow_seq_rec& rec = wtable[kv.first];
        ++want.flows;
        if (rec.packets == 0u) ++want.new_flows;
        for (uint32_t i : kv.second) {
            const uint32_t raw = (uint32_t)(desc[i] >> 48), len = raw < 65535u ? raw : 65535u;
            wseq[i] = rec.packets < BT_FLOW_SEQ_MAX ? (uint32_t)rec.packets : BT_FLOW_SEQ_MAX;
            woff[i] = rec.bytes;
            if ((!max_packets || rec.packets < max_packets) && (!max_bytes || rec.bytes < max_bytes)) {
                wout[i / 64u] |= 1ull << (i % 64u);
                ++want.kept;
                want.kept_bytes += len;
            }
            rec.packets += 1u;
            rec.bytes += len;
            ++want.numbered;
            want.numbered_bytes += len;
        }
    }

    std::vector<uint32_t> seq(n, 0x5A5A5A5Au);
    std::vector<uint64_t> off(n, 0x5A5A5A5A5A5A5A5Aull), out(nw, 0x5A5A5A5A5A5A5A5Aull);
    if (in_place) out = sel;
    const uint64_t* const select = all ? nullptr : in_place ? out.data() : sel.data();
    const bt_flow_seq_opts opts{max_packets, max_bytes, flags, {0u, 0u, 0u}};
    const bt_flow_seq_out o{(outs & 1) ? seq.data() : nullptr, (outs & 2) ? off.data() : nullptr, (outs & 4) || in_place ? out.data() : nullptr};
    bt_flow_seq_result got;
    std::memset(&got, 0xEE, sizeof(got));
    char why[128];
    CHECK(flowseq_host_args(desc.data(), n, ids.data(), select, &opts, table.data(), cap, &o, &got, why, sizeof(why)));
    flowseq_host(desc.data(), n, ids.data(), select, &opts, table.data(), cap, &o, &got);
    CHECK(std::memcmp(&got, &want, sizeof(got)) == 0);
    if (o.seq) CHECK(seq == wseq);
    if (o.byte_off) CHECK(off == woff);
    if (o.out_select) CHECK(out == wout);
    CHECK(table.size() == wtable.size() && (table.empty() || std::memcmp(table.data(), wtable.data(), table.size() * sizeof(bt_flow_seq_rec)) == 0));
}

static void refusals() {
    alignas(256) static uint8_t scratch[1 << 16];
    uint8_t data[256] = {};
    uint64_t desc[4] = {}, words[2] = {}, offs[4] = {};
    uint32_t ids[4] = {}, seqs[4] = {};
    bt_flow_seq_rec table[4] = {};
    bt_flow_seq_result res{};
    bt_batch b{};
    b.base = data; b.desc = desc; b.n = 2; b.bytes = 256; b.desc_format = BT_DESC_PACKED;
    const bt_flow_seq_opts ok{0, 0, 0, {0, 0, 0}};
    const bt_flow_seq_out out{seqs, offs, words};
    FlowseqArgs a;
    char why[128];
    const uint64_t need = fs_layout(2, 4).total;
    CHECK(need <= sizeof(scratch) && need % 256u == 0u);
    const auto dev = [&](const bt_batch* f, const uint32_t* id, const uint64_t* sel, const bt_flow_seq_opts* o, bt_flow_seq_rec* t,
                         uint32_t cap, const bt_flow_seq_out* ou, void* s, uint64_t sb, bt_flow_seq_result* r) {
        return flowseq_args(f, id, sel, o, t, cap, ou, s, sb, r, &a, why, sizeof(why));
    };
    CHECK(dev(&b, ids, words, &ok, table, 4, &out, scratch, need, &res));
    CHECK(a.n == 2 && a.ntiles == 1 && a.nchunks == 1 && a.flow_cap == 4 && a.passes == 1 && a.seq == seqs && a.out_select == words);
    CHECK((uint8_t*)a.head == scratch && (uint8_t*)a.carry + ft_round(kFtWaves * sizeof(FsCarry)) == scratch + need);
    CHECK(!dev(nullptr, ids, words, &ok, table, 4, &out, scratch, need, &res));
    CHECK(!dev(&b, nullptr, words, &ok, table, 4, &out, scratch, need, &res));
    CHECK(!dev(&b, ids, words, nullptr, table, 4, &out, scratch, need, &res));
    CHECK(!dev(&b, ids, words, &ok, nullptr, 4, &out, scratch, need, &res));
    CHECK(dev(&b, ids, words, &ok, nullptr, 0, &out, scratch, fs_layout(2, 0).total, &res) && a.passes == 0);
    CHECK(!dev(&b, ids, words, &ok, table, 4, nullptr, scratch, need, &res));
    CHECK(!dev(&b, ids, words, &ok, table, 4, &out, scratch, need, nullptr));
    CHECK(!dev(&b, ids, words, &ok, table, 4, &out, scratch + 64, need, &res));
    CHECK(!dev(&b, ids, words, &ok, table, 4, &out, nullptr, need, &res));
    CHECK(!dev(&b, ids, words, &ok, table, 4, &out, scratch, need - 1, &res));
    CHECK(!dev(&b, (const uint32_t*)((uint8_t*)ids + 2), words, &ok, table, 4, &out, scratch, need, &res));
    CHECK(!dev(&b, ids, (const uint64_t*)((uint8_t*)words + 4), &ok, table, 4, &out, scratch, need, &res));
    CHECK(!dev(&b, ids, words, &ok, (bt_flow_seq_rec*)((uint8_t*)table + 4), 4, &out, scratch, need, &res));
    const bt_flow_seq_opts bad_flag{0, 0, 2, {0, 0, 0}}, bad_res{0, 0, 0, {0, 1, 0}};
    CHECK(!dev(&b, ids, words, &bad_flag, table, 4, &out, scratch, need, &res));
    CHECK(!dev(&b, ids, words, &bad_res, table, 4, &out, scratch, need, &res));
    const bt_flow_seq_out bad_seq{(uint32_t*)((uint8_t*)seqs + 2), offs, words}, bad_off{seqs, (uint64_t*)((uint8_t*)offs + 4), words};
    CHECK(!dev(&b, ids, words, &ok, table, 4, &bad_seq, scratch, need, &res));
    CHECK(!dev(&b, ids, words, &ok, table, 4, &bad_off, scratch, need, &res));
    bt_batch e = b;
    e.n = 0;
    CHECK(dev(&e, nullptr, nullptr, &ok, nullptr, 0, &out, nullptr, 0, &res) && a.n == 0 && a.nchunks == 0);
    CHECK(fs_passes(0) == 0 && fs_passes(1) == 0 && fs_passes(2) == 1 && fs_passes(256) == 1 && fs_passes(257) == 2 &&
          fs_passes(65536) == 2 && fs_passes(65537) == 3 && fs_passes((1u << 24) + 1u) == 4 && fs_passes(0xFFFFFFFFu) == 4);
    uint64_t last = 0;
    for (uint32_t n : {0u, 1u, 64u, 65u, 16384u, 16385u, 1u << 24, 0xFFFFFFFFu}) {
        const uint64_t t = fs_layout(n, 70000).total;
        CHECK(t >= last && t % 256u == 0u);
        last = t;
    }
}

int main() {
    refusals();
    const uint32_t sizes[] = {0u, 1u, 63u, 64u, 65u, 1000u, 4099u};
    int k = 0;
    for (uint32_t n : sizes)
        for (uint32_t cap : {0u, 1u, 3u, 700u}) {
            std::vector<bt_flow_seq_rec> table(cap);   // zero; the calls of one (n, cap) go on in the same table
            for (int sel_kind = 0; sel_kind < 4; ++sel_kind)
                for (int lim = 0; lim < 4; ++lim, ++k) {
                    const uint64_t mp = (lim & 1) ? 1u + rnd(4) : 0u, mb = (lim & 2) ? 1u + rnd(3000) : 0u;
                    number_case(n, cap, sel_kind, mp, mb, (uint32_t)(k & 1), k % 8, sel_kind == 2 && (k & 2), table,
                                k % 3 == 0 ? 1u : k % 3 == 1 ? cap : 37u);
                }
        }
    // counts close to the saturation of seq and to the wrap of the sums
    std::vector<bt_flow_seq_rec> table(2);
    table[0] = bt_flow_seq_rec{0xFFFFFFFDull, (1ull << 40) - 100u};
    table[1] = bt_flow_seq_rec{~0ull - 2u, ~0ull - 1000u};
    number_case(500, 2, 3, 0x100000000ull, 1ull << 40, 1, 7, false, table, 2);
    number_case(500, 2, 2, 0, 0, 0, 7, true, table, 2);
    if (g_bad) {
        std::printf("%d checks failed\n", g_bad);
        return 1;
    }
    std::printf("flowseq_host_check: all cases hold\n");
    return 0;
}
