// flowstream_host_check.cpp — stream matching's host part from beatrice_amd/csrc/bt_flowstream.h under
// the host sanitizers: the predicate on a pattern blob, the argument checks of bt_flow_stream_host and
// the pass on the host (bt::flowstream_host) over generated frames, flow ids and select words, held to
// a naive oracle that knows every frame's payload, flow and direction from the generator, concatenates
// each (flow, direction) stream in a std::map and asks std::regex about every window of at most P
// bytes that ends inside a packet. Every frame buffer, table, id array and word array is a heap block
// of exactly its size (an access past it is an AddressSanitizer report). No device, no Python, no
// library to load; the pattern compiler is compiled in:
//
//   g++ -std=c++17 -O1 -g -fsanitize=address,undefined -fno-sanitize-recover=all -Iinclude -Ibeatrice_amd/csrc
//       tools/flowstream_host_check.cpp beatrice_amd/csrc/bt_regex_dfa.cpp -o tools/flowstream_host_check
//       && tools/flowstream_host_check                                                   (one command line)
//
// Exit 0 = all cases hold.
#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <map>
#include <regex>
#include <string>
#include <utility>
#include <vector>

#include "beatrice_gpu_bench.h"
#include "bt_flowstream.h"

using namespace bt;
static int g_bad = 0;
#define CHECK(x) do { if (!(x)) { std::printf("FAILED line %d: %s\n", __LINE__, #x); ++g_bad; } } while (0)

static uint32_t g_rng = 24680u;
static uint32_t rnd(uint32_t below) {
    g_rng = g_rng * 1664525u + 1013904223u;
    return (g_rng >> 8) % below;
}

static int compile(const char* expression, void* blob, uint32_t cap, uint32_t* size, bt_flow_stream_info* info) {
    char why[160];
    return flowstream_compile(expression, blob, cap, size, info, why, sizeof(why));   // bt_flow_stream_compile's work
}

static bool is_sentinel(uint32_t id) { return id == 0xFFFFFFFFu || id == 0xFFFFFFFEu || id == 0xFFFFFFFDu || id == 0xFFFFFFFBu; }

struct Made { std::vector<uint8_t> frame; std::string payload; uint32_t dir; bool l4; };

// A frame around `payload`: kind 0 TCP, 1 UDP, 2 TCP behind a VLAN tag with IP options, 3 UDP over IPv6,
// 4 ICMP (no stream), 5 TCP with Ethernet padding, 6 TCP snapped inside its payload.
static Made make(const std::string& payload, int kind, bool reverse) {
    Made m;
    m.dir = reverse ? 1u : 0u;
    m.l4 = kind != 4;
    const bool udp = kind == 1 || kind == 3, v6 = kind == 3, vlan = kind == 2;
    const uint32_t ihl = kind == 2 ? 7u : 5u, l4len = (udp ? 8u : 20u) + (uint32_t)payload.size();
    std::vector<uint8_t>& f = m.frame;
    f.assign(12, 0);
    if (vlan) { f.push_back(0x81); f.push_back(0x00); f.push_back(0); f.push_back(5); }
    f.push_back(v6 ? 0x86 : 0x08);
    f.push_back(v6 ? 0xDD : 0x00);
    const uint8_t a[4] = {10, 1, 2, 3}, b[4] = {10, 3, 2, 1};
    const uint8_t* src = reverse ? b : a;
    const uint8_t* dst = reverse ? a : b;
    if (v6) {
        const uint8_t h[8] = {0x60, 0, 0, 0, (uint8_t)(l4len >> 8), (uint8_t)l4len, 17, 64};
        f.insert(f.end(), h, h + 8);
        f.insert(f.end(), 12, 0); f.insert(f.end(), src, src + 4);
        f.insert(f.end(), 12, 0); f.insert(f.end(), dst, dst + 4);
    } else {
        const uint32_t tot = 4u * ihl + l4len;
        const uint8_t h[12] = {(uint8_t)(0x40u | ihl), 0, (uint8_t)(tot >> 8), (uint8_t)tot, 0, 0, 0, 0, 64,
                               (uint8_t)(kind == 4 ? 1 : udp ? 17 : 6), 0, 0};
        f.insert(f.end(), h, h + 12);
        f.insert(f.end(), src, src + 4);
        f.insert(f.end(), dst, dst + 4);
        f.insert(f.end(), 4u * (ihl - 5u), 0);
    }
    const uint16_t sp = reverse ? 80 : 40000, dp = reverse ? 40000 : 80;
    f.push_back(sp >> 8); f.push_back(sp & 255); f.push_back(dp >> 8); f.push_back(dp & 255);
    if (udp) {
        f.push_back(l4len >> 8); f.push_back(l4len & 255); f.push_back(0); f.push_back(0);
    } else {
        f.insert(f.end(), 8, 0);
        f.push_back(0x50); f.push_back(0x18);
        f.insert(f.end(), 6, 0);
    }
    f.insert(f.end(), payload.begin(), payload.end());
    m.payload = m.l4 ? payload : std::string();
    if (kind == 5) f.insert(f.end(), 1 + rnd(9), 0);
    if (kind == 6 && payload.size() > 1) {
        const size_t cut = 1 + rnd((uint32_t)payload.size() - 1);
        f.resize(f.size() - cut);
        m.payload.resize(payload.size() - cut);
    }
    return m;
}

static std::string noise(uint32_t n, const std::string& text) {
    std::string s(n, 'a');
    for (auto& c : s) c = (char)('a' + rnd(26));
    for (uint32_t k = 0; k < 1 + n / 24; ++k) {
        const uint32_t at = rnd(n + 1);
        for (size_t j = 0; j < text.size() && at + j < n; ++j) s[at + j] = text[j];
    }
    return s;
}

// `calls` calls of n packets against one table; the oracle's streams carry on from call to call.
static void stream_case(const char* pattern, const std::string& text, uint32_t n, uint32_t cap, uint32_t flags, uint32_t calls,
                        bool in_place) {
    uint32_t size = 0;
    bt_flow_stream_info info{};
    CHECK(compile(pattern, nullptr, 0, &size, &info) == BT_OK);
    std::vector<uint8_t> blob(size);
    CHECK(compile(pattern, blob.data(), size, &size, &info) == BT_OK);
    const std::regex rx(pattern);
    const uint32_t P = info.positions;
    std::vector<bt_flow_stream_rec> table(cap), wtable(cap);
    std::map<std::pair<uint32_t, uint32_t>, std::string> streams;
    static const uint32_t lens[] = {0, 1, 2, 3, 5, 8, 13, 40, 127, 128, 129, 300};
    for (uint32_t call = 0; call < calls; ++call) {
        const uint32_t nw = (n + 63u) / 64u;
        std::vector<uint64_t> desc(n), sel(nw), hit(nw, 0xDEADull), whit(nw, 0ull);
        std::vector<uint32_t> ids(n);
        std::vector<Made> made(n);
        std::vector<uint8_t> data;
        for (uint32_t i = 0; i < n; ++i) {
            made[i] = make(noise(lens[rnd(12)], text), (int)rnd(7), rnd(2) != 0);
            if (!(flags & BT_FLOWTAB_BIDIRECTIONAL)) made[i].dir = 0;
            data.insert(data.end(), 1 + rnd(3), 0xEE);
            desc[i] = (uint64_t)data.size() | (uint64_t)made[i].frame.size() << 48;
            data.insert(data.end(), made[i].frame.begin(), made[i].frame.end());
            const uint32_t r = rnd(20);
            ids[i] = r == 0 ? 0xFFFFFFFFu - rnd(5) : r == 1 ? cap + rnd(3) : rnd(cap);
        }
        for (uint32_t w = 0; w < nw; ++w) sel[w] = (uint64_t)rnd(1u << 16) << 48 | (uint64_t)rnd(1u << 24) << 24 | rnd(1u << 24);
        if (call == 0)
            for (uint32_t w = 0; w < nw; ++w) sel[w] = ~0ull;
        if (n % 64u) sel[nw - 1] |= ~0ull << (n % 64u);   // garbage above n: ignored

        bt_flow_stream_result want{};
        want.n = n;
        std::vector<bool> had(cap), fresh(cap);
        for (uint32_t f = 0; f < cap; ++f) had[f] = wtable[f].hit_packets[0] || wtable[f].hit_packets[1];
        for (uint32_t i = 0; i < n; ++i) {
            if (!((sel[i / 64u] >> (i % 64u)) & 1u)) continue;
            ++want.selected;
            if (ids[i] >= cap) { is_sentinel(ids[i]) ? ++want.unkeyed : ++want.bad_ids; continue; }
            const std::string& pay = made[i].payload;
            if (pay.empty()) continue;
            std::string& s = streams[{ids[i], made[i].dir}];
            const size_t a = s.size();
            s += pay;
            bool got = false;
            for (size_t e = a + 1; e <= s.size() && !got; ++e)
                for (size_t st = e > P ? e - P : 0; st < e && !got; ++st) got = std::regex_match(s.begin() + st, s.begin() + e, rx);
            bt_flow_stream_rec& rec = wtable[ids[i]];
            ++rec.stream_packets[made[i].dir];
            ++want.stream_packets;
            want.stream_bytes += pay.size();
            if (got) {
                ++rec.hit_packets[made[i].dir];
                ++want.hit_packets;
                whit[i / 64u] |= 1ull << (i % 64u);
                if (!had[ids[i]] && !fresh[ids[i]]) { fresh[ids[i]] = true; ++want.new_hit_flows; }
            }
        }

        bt_flow_stream_result res;
        memset(&res, 0xCC, sizeof(res));
        bt_flow_stream_out out{in_place ? sel.data() : hit.data(), &res, {0, 0}};
        FstPattern pat;
        char why[160];
        CHECK(flowstream_host_args(data.data(), desc.data(), n, ids.data(), sel.data(), flags, blob.data(), size, table.data(), cap, &out,
                                   &pat, why, sizeof(why)) == BT_OK);
        flowstream_host(data.data(), data.size(), desc.data(), n, ids.data(), sel.data(), flags, blob.data(), pat, table.data(), cap, &out);
        CHECK(memcmp(&res, &want, sizeof(res)) == 0);
        CHECK(memcmp(in_place ? sel.data() : hit.data(), whit.data(), 8u * nw) == 0);
        for (uint32_t f = 0; f < cap; ++f) {
            CHECK(table[f].stream_packets[0] == wtable[f].stream_packets[0] && table[f].stream_packets[1] == wtable[f].stream_packets[1]);
            CHECK(table[f].hit_packets[0] == wtable[f].hit_packets[0] && table[f].hit_packets[1] == wtable[f].hit_packets[1]);
        }
    }
    // the carried state: the step over each whole stream from zero
    FstPattern pat;
    char why[160];
    CHECK(flowstream_pattern(blob.data(), size, &pat, why, sizeof(why)) == BT_OK);
    for (const auto& kv : streams) {
        uint64_t D = 0;
        for (unsigned char c : kv.second) {
            uint64_t e = 0;
            memcpy(&e, blob.data() + kFstBlobHeader + (size_t)c * (pat.W / 8u), pat.W / 8u);
            D = flowstream_step(pat, D, e);
        }
        CHECK(table[kv.first.first].d[kv.first.second] == D);
    }
}

static void refusals() {
    uint32_t size = 0;
    const char* no[] = {"GET.+", "ab*c", "a{2,}b", "^GET", "done$", "\\bGET", "(?:ab)+c", "a?", "a^b"};
    for (const char* p : no) CHECK(compile(p, nullptr, 0, &size, nullptr) == BT_E_NOT_IMPLEMENTED);
    CHECK(compile("(", nullptr, 0, &size, nullptr) == BT_E_INVALID_ARGUMENT);
    std::vector<uint8_t> blob(80 + 256 * 8);
    CHECK(compile("GET|POST", blob.data(), 100, &size, nullptr) == BT_E_RESOURCE);
    CHECK(compile("GET|POST", blob.data(), (uint32_t)blob.size(), &size, nullptr) == BT_OK && size == 80 + 256);
    FstPattern pat;
    char why[160];
    CHECK(flowstream_pattern(nullptr, size, &pat, why, sizeof(why)) == BT_E_INVALID_ARGUMENT);
    CHECK(flowstream_pattern(blob.data(), 79, &pat, why, sizeof(why)) == BT_E_INVALID_ARGUMENT);
    CHECK(flowstream_pattern(blob.data(), size - 1, &pat, why, sizeof(why)) == BT_E_INVALID_ARGUMENT);
    CHECK(flowstream_pattern(blob.data(), size, &pat, why, sizeof(why)) == BT_OK && pat.P == 7 && pat.T == 6 && pat.W == 8);
    bt_flow_stream_result res{};
    bt_flow_stream_out out{nullptr, &res, {0, 0}};
    std::vector<bt_flow_stream_rec> table(2);
    uint32_t ids[2] = {0, 1};
    uint64_t desc[2] = {0, 0};
    uint8_t data[4] = {0};
    const auto host = [&](const bt_flow_stream_out* o, uint32_t flags, uint32_t cap, const void* tab) {
        return flowstream_host_args(data, desc, 2, ids, nullptr, flags, blob.data(), size, static_cast<const bt_flow_stream_rec*>(tab), cap,
                                    o, &pat, why, sizeof(why));
    };
    CHECK(host(&out, 0, 2, table.data()) == BT_OK);
    CHECK(host(nullptr, 0, 2, table.data()) == BT_E_INVALID_ARGUMENT);
    CHECK(host(&out, 4, 2, table.data()) == BT_E_INVALID_ARGUMENT);
    CHECK(host(&out, 0, 2, nullptr) == BT_E_INVALID_ARGUMENT);
    CHECK(host(&out, 0, 0x80000001u, table.data()) == BT_E_INVALID_ARGUMENT);
    bt_flow_stream_out bad{nullptr, &res, {0, 1}};
    CHECK(host(&bad, 0, 2, table.data()) == BT_E_INVALID_ARGUMENT);
    CHECK(fst_passes(0) == 0 && fst_passes(1) == 1 && fst_passes(128) == 1 && fst_passes(129) == 2 && fst_passes(32768) == 2 &&
          fst_passes(32769) == 3 && fst_passes(0x80000000u) == 4);
    const FstLayout l = fst_layout(100000, 70000);
    CHECK(l.total % 256 == 0 && l.bits_bytes == (70000 + 63) / 64 * 8 && l.meta > l.dstart && l.total > l.bits);
}

int main() {
    refusals();
    stream_case("GET|POST", "POST", 700, 9, BT_FLOWTAB_BIDIRECTIONAL, 3, false);
    stream_case("GET|POST", "GET", 129, 3, 0, 2, true);
    stream_case("colou?r", "color", 500, 5, BT_FLOWTAB_BIDIRECTIONAL, 2, false);
    stream_case("Host: example\\.com", "Host: example.com", 300, 4, BT_FLOWTAB_BIDIRECTIONAL | BT_FLOWTAB_L3_ONLY, 2, true);
    stream_case("0123456789abcdef|ghijklmnopqrstuv|wxyzABCDEFGHIJKL|MNOPQRSTUVWXYZ-_", "wxyzABCDEFGHIJKL", 200, 2, 0, 2, false);
    stream_case("ab?c?d\\d", "ad7", 400, 6, BT_FLOWTAB_BIDIRECTIONAL, 2, false);
    if (g_bad) {
        std::printf("flowstream_host_check: %d checks FAILED\n", g_bad);
        return 1;
    }
    std::printf("flowstream_host_check: all cases hold\n");
    return 0;
}
