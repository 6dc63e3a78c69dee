// flowhosts_host_check.cpp — the endpoint table's host part from beatrice_amd/csrc/bt_flowhosts.h
// under the host sanitizers: the struct layout, the argument checks of bt_flow_track_hosts_device /
// _host (every refusal, and an accepted call with the launch arguments it resolves to), the scratch
// layout, and the group-by on the host (bt::flowhosts_host) over crafted states against a plain
// std::map restatement written here: fresh hosts, a hub in every flow in either role, three hosts,
// flows whose two addresses are equal, v4 and v6 mixed with 1.2.3.4 beside 0102:0304::, sums that
// wrap, with and without the side table, host_cap 0 / below / above the hosts, a table of exactly
// as many slots as hosts and one too small. Every output is a heap block of exactly host_cap
// records and 2 n_flows numbers (an access past it is an AddressSanitizer report). No device, no
// Python, no library to load:
//
//   g++ -std=c++17 -O1 -g -fsanitize=address,undefined -fno-sanitize-recover=all -Iinclude -Ibeatrice_amd/csrc
//       tools/flowhosts_host_check.cpp -o tools/flowhosts_host_check && tools/flowhosts_host_check   (one command line)
//
// Exit 0 = all cases hold.
#include <array>
#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <map>
#include <utility>
#include <vector>

#include "bt_flowhosts.h"

using namespace bt;
static int g_bad = 0;
#define CHECK(x) do { if (!(x)) { std::printf("FAILED line %d: %s\n", __LINE__, #x); ++g_bad; } } while (0)

alignas(256) static unsigned char g_state[1 << 16];
alignas(256) static unsigned char g_scratch[1 << 17];
alignas(8) static unsigned char g_out[1 << 12];
static bt_flow_tcp_rec g_tcp[100];
static bt_flow_hosts_result g_result;
static const FkShadow g_shadow{BT_FLOWTAB_BIDIRECTIONAL, 100u, 256u};

struct Call {   // a device call with nothing wrong
    const FkShadow* sh = &g_shadow;
    const void* state = g_state;
    bt_flow_hosts_opts opts{0u, 16u, {0u, 0u}};
    const bt_flow_tcp_rec* tcp = nullptr;
    void* scratch = g_scratch;
    uint64_t scratch_bytes = sizeof(g_scratch);
    bt_flow_hosts_out out{reinterpret_cast<bt_flow_host_rec*>(g_out), nullptr, &g_result};
    bool no_opts = false, no_out = false;
};

static bool run(const Call& c, FlowhostsArgs* a, const char* word) {
    char why[160];
    if (flowhosts_args(c.sh, c.state, c.no_opts ? nullptr : &c.opts, c.tcp, c.scratch, c.scratch_bytes, c.no_out ? nullptr : &c.out, a, why,
                       sizeof(why)))
        return word == nullptr;
    return word && std::strstr(why, word);
}

static bool refuses(const Call& c, const char* word) {
    FlowhostsArgs a;
    return run(c, &a, word);
}

static void check_refusals() {
    Call c;
    FlowhostsArgs a;
    CHECK(run(c, &a, nullptr));
    const FhLayout l = fh_scratch(100u, 512u);
    CHECK(fh_auto_slots(100u) == 512u && fh_auto_slots(1u) == 128u && fh_auto_slots(32u) == 128u && fh_auto_slots(33u) == 256u);
    CHECK(fh_auto_slots(1u << 29) == 1u << 31 && fh_auto_slots((1u << 29) + 1u) == 0u);
    CHECK(a.hdr == reinterpret_cast<const bt_flow_track_hdr*>(g_state) && (const unsigned char*)a.recs == g_state + 256);
    CHECK(a.flow_cap == 100u && a.state_slots == 256u && a.flags == BT_FLOWTAB_BIDIRECTIONAL && a.slots == 512u && a.host_cap == 16u);
    CHECK((unsigned char*)a.ctl == g_scratch + l.ctl && (unsigned char*)a.tab == g_scratch + l.tab &&
          (unsigned char*)a.cslot == g_scratch + l.cslot && (unsigned char*)a.parts == g_scratch + l.parts);
    CHECK(l.tab == 256u && l.cslot == l.tab + 2048u && l.parts == l.cslot + 1024u && l.total == l.parts + 256u && l.total <= sizeof(g_scratch));
    CHECK(a.result == &g_result && (unsigned char*)a.hosts == g_out && !a.endpoint_host && !a.tcp);
    { Call d; d.state = nullptr; CHECK(refuses(d, "null state")); }
    { Call d; d.no_opts = true; CHECK(refuses(d, "null opts")); }
    { Call d; d.no_out = true; CHECK(refuses(d, "null out")); }
    { Call d; d.out.result = nullptr; CHECK(refuses(d, "null result")); }
    { Call d; d.scratch = nullptr; CHECK(refuses(d, "null scratch")); }
    { Call d; d.state = g_state + 128; CHECK(refuses(d, "state is not 256-byte aligned")); }
    { Call d; d.scratch = g_scratch + 64; CHECK(refuses(d, "scratch is not 256-byte aligned")); }
    { Call d; d.out.result = reinterpret_cast<bt_flow_hosts_result*>(g_out + 4); CHECK(refuses(d, "result is not 8-byte aligned")); }
    { Call d; d.out.hosts = reinterpret_cast<bt_flow_host_rec*>(g_out + 4); CHECK(refuses(d, "hosts is not 8-byte aligned")); }
    { Call d; d.tcp = reinterpret_cast<const bt_flow_tcp_rec*>(g_out + 1); CHECK(refuses(d, "tcp is not 4-byte aligned")); }
    { Call d; d.out.endpoint_host = reinterpret_cast<uint32_t*>(g_out + 2); CHECK(refuses(d, "endpoint_host is not 4-byte aligned")); }
    { Call d; d.opts.slots = 384u; CHECK(refuses(d, "slots is not a power of two")); }
    { Call d; d.opts.slots = 64u; CHECK(refuses(d, "slots below 128")); }
    { Call d; d.opts.reserved[0] = 1u; CHECK(refuses(d, "reserved")); }
    { Call d; d.opts.reserved[1] = 9u; CHECK(refuses(d, "reserved")); }
    { Call d; d.out.hosts = nullptr; CHECK(refuses(d, "null hosts with host_cap != 0")); }
    { Call d; d.out.hosts = nullptr; d.opts.host_cap = 0u; CHECK(run(d, &a, nullptr) && !a.hosts && a.host_cap == 0u); }
    { Call d; d.sh = nullptr; CHECK(refuses(d, "not an initialised tracker")); }
    { Call d; d.scratch_bytes = l.total - 1u; CHECK(refuses(d, "scratch_bytes")); }
    { Call d; d.scratch_bytes = l.total; CHECK(run(d, &a, nullptr)); }
    { Call d; d.opts.slots = 128u; d.scratch_bytes = fh_scratch(100u, 128u).total; CHECK(run(d, &a, nullptr) && a.slots == 128u); }   // fewer slots than flows is legal
    { Call d; d.tcp = g_tcp; d.out.endpoint_host = reinterpret_cast<uint32_t*>(g_out + 4); CHECK(run(d, &a, nullptr) && a.tcp == g_tcp); }
    static const FkShadow large{0u, (1u << 29) + 1u, 1u << 30}, huge{0u, 1u << 31, 1u << 31};
    { Call d; d.sh = &large; CHECK(refuses(d, "slots == 0 (auto) needs flow_cap <= 2^29")); }
    { Call d; d.sh = &huge; d.opts.slots = 128u; CHECK(refuses(d, "flow_cap above 2^31 - 1")); }
    uint32_t s = 0;
    char why[128];
    CHECK(!flowhosts_geometry(0u, 0u, &s, why, sizeof(why)) && flowhosts_geometry(1u << 29, 0u, &s, why, sizeof(why)) && s == 1u << 31);
    uint64_t prev = 0;
    for (uint32_t cap : {1u, 2u, 255u, 256u, 257u, 5000u, 1u << 20}) {   // the need grows with flow_cap and with slots
        const uint64_t need = fh_scratch(cap, fh_auto_slots(cap)).total;
        CHECK(need % 256u == 0 && need >= prev && need >= 4ull * fh_auto_slots(cap) + 8ull * cap);
        CHECK(fh_scratch(cap, 2u * fh_auto_slots(cap)).total > need);
        prev = need;
    }
}

// ---- the host form against a std::map ------------------------------------------------------

struct Flow { std::array<uint8_t, 16> a, b; bool six; };

static std::array<uint8_t, 16> v4(uint32_t x) { return {uint8_t(x >> 24), uint8_t(x >> 16), uint8_t(x >> 8), uint8_t(x)}; }
static std::array<uint8_t, 16> v6(uint32_t head, uint32_t tail) {
    std::array<uint8_t, 16> r{};
    r[0] = uint8_t(head >> 24); r[1] = uint8_t(head >> 16); r[2] = uint8_t(head >> 8); r[3] = uint8_t(head);
    r[12] = uint8_t(tail >> 24); r[13] = uint8_t(tail >> 16); r[14] = uint8_t(tail >> 8); r[15] = uint8_t(tail);
    return r;
}

static uint32_t g_seed = 12345u;
static uint32_t rnd() { g_seed = g_seed * 1664525u + 1013904223u; return g_seed >> 8; }

struct State {
    std::vector<unsigned char> raw;
    unsigned char* p;
    bt_flow_track_sizes lay{};
    std::vector<bt_flow_tcp_rec> tcp;
    uint32_t flow_cap, n_flows, flags;
    bt_flow_track_rec* recs() { return reinterpret_cast<bt_flow_track_rec*>(p + lay.records); }
};

static State make_state(uint32_t flow_cap, const std::vector<Flow>& flows, uint32_t flags) {
    State s;
    char why[128];
    s.flow_cap = flow_cap; s.n_flows = (uint32_t)flows.size(); s.flags = flags;
    CHECK(fk_layout(flow_cap, 0u, &s.lay, why, sizeof(why)));
    s.raw.assign(s.lay.total + 256u, 0);
    s.p = reinterpret_cast<unsigned char*>((reinterpret_cast<uintptr_t>(s.raw.data()) + 255u) & ~uintptr_t(255));
    const bt_flow_track_opts o{flags, flow_cap, 0u, 0u};
    fk_init_host(s.p, o, s.lay);
    reinterpret_cast<bt_flow_track_hdr*>(s.p)->n_flows = s.n_flows;
    s.tcp.assign(flow_cap, bt_flow_tcp_rec{});
    static const uint8_t kinds[] = {0x00, 0x02, 0x12, 0x10, 0x11, 0x14, 0x18, 0x1B};
    for (uint32_t f = 0; f < flow_cap; ++f) {
        bt_flow_track_rec r{};
        bt_flow_tcp_rec& t = s.tcp[f];
        if (f < s.n_flows) {
            const Flow& fl = flows[f];
            const uint32_t alen = fl.six ? 16u : 4u;
            memcpy(r.key, fl.a.data(), alen);
            memcpy(r.key + alen, fl.b.data(), alen);
            const bool ports = f % 5u != 0u;
            if (ports) { r.key[2 * alen] = uint8_t(rnd()); r.key[2 * alen + 3] = uint8_t(rnd()); }
            r.klass = uint8_t(fl.six ? (ports ? BT_FLOW_V6_L4 : BT_FLOW_V6) : (ports ? BT_FLOW_V4_L4 : BT_FLOW_V4));
            r.packets[0] = rnd() % 1000u; r.packets[1] = (flags & BT_FLOWTAB_BIDIRECTIONAL) ? rnd() % 1000u : 0u;
            r.bytes[0] = f % 37u == 3u ? ~0ull - 5u : rnd(); r.bytes[1] = (flags & BT_FLOWTAB_BIDIRECTIONAL) ? rnd() : 0u;
            r.first_ts = rnd(); r.last_ts = r.first_ts + rnd() % 5000u;
            t.flags[0] = kinds[rnd() % 8u]; t.flags[1] = kinds[rnd() % 8u];
            t.syn_packets = f % 41u == 7u ? 0xFFFFFFFEu : rnd() % 4u; t.fin_packets = rnd() % 3u; t.rst_packets = rnd() % 2u;
        } else {   // garbage that is never a flow
            memset(r.key, 0xEE, sizeof(r.key));
            r.klass = BT_FLOW_V6_L4; r.packets[0] = ~0ull; r.bytes[1] = ~0ull; r.last_ts = ~0ull;
            t.flags[0] = 0xFF; t.syn_packets = ~0u;
        }
        s.recs()[f] = r;
    }
    return s;
}

// The plain restatement: a map from (family, address) to the host's number, hosts in order of first appearance.
static void restate(State& s, bool with_tcp, std::vector<bt_flow_host_rec>* hosts, std::vector<uint32_t>* ends, bt_flow_hosts_result* res) {
    std::map<std::pair<int, std::array<uint8_t, 16>>, uint32_t> number;
    *res = bt_flow_hosts_result{};
    res->n_flows = s.n_flows;
    for (uint32_t f = 0; f < s.n_flows; ++f) {
        const bt_flow_track_rec& r = s.recs()[f];
        const bool six = r.klass == BT_FLOW_V6 || r.klass == BT_FLOW_V6_L4;
        res->packets_total += r.packets[0] + r.packets[1];
        res->bytes_total += r.bytes[0] + r.bytes[1];
        for (uint32_t role = 0; role < 2u; ++role) {
            std::array<uint8_t, 16> a{};
            memcpy(a.data(), r.key + (six ? 16u : 4u) * role, six ? 16u : 4u);
            const auto key = std::make_pair(six ? 6 : 4, a);
            auto it = number.find(key);
            if (it == number.end()) {
                it = number.emplace(key, (uint32_t)hosts->size()).first;
                bt_flow_host_rec h{};
                memcpy(h.addr, a.data(), 16);
                h.family = uint8_t(six ? 6 : 4);
                h.first_flow = f;
                h.first_ts = r.first_ts; h.last_ts = r.last_ts;
                hosts->push_back(h);
                ++(six ? res->hosts_v6 : res->hosts_v4);
            }
            bt_flow_host_rec& h = (*hosts)[it->second];
            ends->push_back(it->second);
            h.flows[role] += 1u;
            h.packets[0] += r.packets[role]; h.packets[1] += r.packets[1u - role];
            h.bytes[0] += r.bytes[role]; h.bytes[1] += r.bytes[1u - role];
            h.first_ts = r.first_ts < h.first_ts ? r.first_ts : h.first_ts;
            h.last_ts = r.last_ts > h.last_ts ? r.last_ts : h.last_ts;
            if (with_tcp) {
                const bt_flow_tcp_rec& t = s.tcp[f];
                h.tcp_state[flowtcp_state(t.flags[0], t.flags[1], s.flags)] += 1u;
                h.syn_flows[0] += (t.flags[role] & BT_TCPF_SYN) ? 1u : 0u;
                h.syn_flows[1] += (t.flags[1u - role] & BT_TCPF_SYN) ? 1u : 0u;
                h.syn_packets += t.syn_packets; h.fin_packets += t.fin_packets; h.rst_packets += t.rst_packets;
            }
        }
    }
    res->n_hosts = (uint32_t)hosts->size();
}

static void check_case(const char* name, uint32_t flow_cap, const std::vector<Flow>& flows, uint32_t flags) {
    State s = make_state(flow_cap, flows, flags);
    for (int with_tcp = 0; with_tcp < 2; ++with_tcp) {
        std::vector<bt_flow_host_rec> want;
        std::vector<uint32_t> want_ends;
        bt_flow_hosts_result wr{};
        restate(s, with_tcp != 0, &want, &want_ends, &wr);
        uint32_t exact = kFtMinSlots;
        while (exact < wr.n_hosts) exact <<= 1;
        const uint32_t caps[] = {0u, wr.n_hosts / 2u, wr.n_hosts, wr.n_hosts + 5u};
        for (uint32_t host_cap : caps) {
            for (uint32_t slots : {0u, exact}) {
                // blocks of exactly the sizes the call may write
                bt_flow_host_rec* hosts = host_cap ? static_cast<bt_flow_host_rec*>(std::malloc(sizeof(bt_flow_host_rec) * host_cap)) : nullptr;
                uint32_t* ends = s.n_flows ? static_cast<uint32_t*>(std::malloc(8u * s.n_flows)) : nullptr;
                bt_flow_hosts_result res{};
                const bt_flow_hosts_opts o{slots, host_cap, {0u, 0u}};
                const bt_flow_hosts_out out{hosts, ends, &res};
                FkHostState hs{};
                uint32_t resolved = 0;
                char why[160];
                const std::vector<unsigned char> before(s.p, s.p + s.lay.total);
                const bool ok = flowhosts_host_args(s.p, s.lay.total, &o, with_tcp ? s.tcp.data() : nullptr, &out, &hs, &resolved, why, sizeof(why));
                CHECK(ok);
                if (ok) {
                    flowhosts_host(hs, resolved, o, with_tcp ? s.tcp.data() : nullptr, out);
                    const uint32_t nw = wr.n_hosts < host_cap ? wr.n_hosts : host_cap;
                    bt_flow_hosts_result w = wr;
                    w.n_written = nw; w.slots = resolved;
                    if (memcmp(&res, &w, sizeof(res)) != 0 || (nw && memcmp(hosts, want.data(), sizeof(bt_flow_host_rec) * nw) != 0) ||
                        (s.n_flows && memcmp(ends, want_ends.data(), 8u * s.n_flows) != 0)) {
                        std::printf("FAILED %s: tcp=%d host_cap=%u slots=%u (n_hosts %u / %u)\n", name, with_tcp, host_cap, slots, res.n_hosts, wr.n_hosts);
                        ++g_bad;
                    }
                    uint64_t sent = 0;
                    bool sums = true;
                    for (uint32_t h = 0; h < nw; ++h) {
                        sent += hosts[h].packets[0];
                        uint32_t st = 0;
                        for (int j = 0; j < 7; ++j) st += hosts[h].tcp_state[j];
                        sums = sums && st == (with_tcp ? hosts[h].flows[0] + hosts[h].flows[1] : 0u) && (!h || hosts[h - 1].first_flow <= hosts[h].first_flow);
                    }
                    CHECK(sums && (nw < wr.n_hosts || sent == res.packets_total));
                    CHECK(memcmp(before.data(), s.p, s.lay.total) == 0);   // the state is only read
                }
                std::free(hosts);
                std::free(ends);
            }
        }
        if (wr.n_hosts > kFtMinSlots) {   // one power of two too few: overflow, and still nothing out of bounds
            bt_flow_host_rec* hosts = static_cast<bt_flow_host_rec*>(std::malloc(sizeof(bt_flow_host_rec) * 3u));
            uint32_t* ends = static_cast<uint32_t*>(std::malloc(8u * s.n_flows));
            bt_flow_hosts_result res{};
            const bt_flow_hosts_opts o{exact / 2u >= kFtMinSlots && exact / 2u < wr.n_hosts ? exact / 2u : kFtMinSlots, 3u, {0u, 0u}};
            const bt_flow_hosts_out out{hosts, ends, &res};
            FkHostState hs{};
            uint32_t resolved = 0;
            char why[160];
            CHECK(flowhosts_host_args(s.p, s.lay.total, &o, nullptr, &out, &hs, &resolved, why, sizeof(why)));
            flowhosts_host(hs, resolved, o, nullptr, out);
            CHECK(res.overflow_endpoints != 0 && res.status == 0 && res.n_flows == s.n_flows && res.slots == o.slots);
            std::free(hosts);
            std::free(ends);
        }
    }
}

static void check_host_form() {
    std::vector<Flow> f;
    check_case("empty", 64u, f, BT_FLOWTAB_BIDIRECTIONAL);
    for (uint32_t n : {1u, 2u, 64u, 65u, 257u}) {
        f.clear();
        for (uint32_t i = 0; i < n; ++i) f.push_back({v4(0x0A000000u + 2u * i), v4(0x0A000001u + 2u * i), false});
        check_case("fresh", n, f, BT_FLOWTAB_BIDIRECTIONAL);
        check_case("fresh, unidirectional", n + 9u, f, 0u);
    }
    for (int how = 0; how < 3; ++how) {
        f.clear();
        for (uint32_t i = 0; i < 1030u; ++i) {
            const bool first = how == 0 || (how == 2 && i % 2u == 0u);
            const auto hub = v4(0xC0A80001u), other = v4(0x0B000000u + i);
            f.push_back({first ? hub : other, first ? other : hub, false});
        }
        check_case("hub", 1030u, f, BT_FLOWTAB_BIDIRECTIONAL);
    }
    f.clear();
    for (uint32_t i = 0; i < 1030u; ++i) f.push_back({v4(0xAC100000u + rnd() % 3u), v4(0xAC100000u + rnd() % 3u), false});
    check_case("3 hosts", 1100u, f, BT_FLOWTAB_BIDIRECTIONAL);
    f.clear();
    for (uint32_t i = 0; i < 600u; ++i) {   // v4 and v6 mixed, 1.2.3.4 beside 0102:0304::, some flows with one address twice
        const bool six = rnd() % 3u == 0u;
        const uint32_t x = rnd() % 40u, y = rnd() % 20u == 0u ? x : rnd() % 40u;
        if (six) f.push_back({x ? v6(0x20010DB8u, x) : v6(0x01020304u, 0u), y ? v6(0x20010DB8u, y) : v6(0x01020304u, 0u), true});
        else f.push_back({x ? v4(0xAC100000u + x) : v4(0x01020304u), y ? v4(0xAC100000u + y) : v4(0x01020304u), false});
    }
    check_case("mixed", 700u, f, BT_FLOWTAB_BIDIRECTIONAL);
    check_case("mixed, l3 only", 600u, f, BT_FLOWTAB_L3_ONLY);
    // the pair by itself: two hosts, never one
    f = {{v4(0x01020304u), v4(0x01020304u), false}, {v6(0x01020304u, 0u), v6(0x01020304u, 0u), true}};
    State s = make_state(2u, f, 0u);
    std::vector<bt_flow_host_rec> want;
    std::vector<uint32_t> ends;
    bt_flow_hosts_result wr{};
    restate(s, false, &want, &ends, &wr);
    CHECK(wr.n_hosts == 2u && wr.hosts_v4 == 1u && wr.hosts_v6 == 1u && want[0].flows[0] == 1u && want[0].flows[1] == 1u);
    check_case("the pair", 2u, f, 0u);
}

static void check_host_refusals() {
    std::vector<Flow> f = {{v4(1u), v4(2u), false}};
    State s = make_state(64u, f, 0u);
    bt_flow_host_rec hosts[4];
    bt_flow_hosts_result res{};
    FkHostState hs{};
    uint32_t slots = 0;
    char why[160];
    const bt_flow_hosts_opts good{0u, 4u, {0u, 0u}};
    const bt_flow_hosts_out out{hosts, nullptr, &res};
    const auto refuses = [&](const void* state, uint64_t bytes, const bt_flow_hosts_opts* o, const bt_flow_hosts_out* u, const char* word) {
        return !flowhosts_host_args(state, bytes, o, nullptr, u, &hs, &slots, why, sizeof(why)) && std::strstr(why, word);
    };
    CHECK(flowhosts_host_args(s.p, s.lay.total, &good, nullptr, &out, &hs, &slots, why, sizeof(why)) && slots == 256u);
    CHECK(refuses(nullptr, s.lay.total, &good, &out, "null state"));
    CHECK(refuses(s.p + 8, s.lay.total, &good, &out, "state is not 256-byte aligned"));
    CHECK(refuses(s.p, s.lay.total, nullptr, &out, "null opts"));
    CHECK(refuses(s.p, s.lay.total, &good, nullptr, "null out"));
    CHECK(refuses(s.p, s.lay.total - 1u, &good, &out, "state_bytes below the header's layout"));
    const bt_flow_hosts_opts odd{96u, 4u, {0u, 0u}}, low{64u, 4u, {0u, 0u}}, res1{0u, 4u, {0u, 1u}};
    CHECK(refuses(s.p, s.lay.total, &odd, &out, "power of two") && refuses(s.p, s.lay.total, &low, &out, "below 128") &&
          refuses(s.p, s.lay.total, &res1, &out, "reserved"));
    const bt_flow_hosts_out nohosts{nullptr, nullptr, &res}, nores{hosts, nullptr, nullptr};
    CHECK(refuses(s.p, s.lay.total, &good, &nohosts, "null hosts") && refuses(s.p, s.lay.total, &good, &nores, "null result"));
    std::vector<unsigned char> zero(4096 + 256, 0);
    unsigned char* z = reinterpret_cast<unsigned char*>((reinterpret_cast<uintptr_t>(zero.data()) + 255u) & ~uintptr_t(255));
    CHECK(refuses(z, 4096u, &good, &out, "not an initialised tracker"));
}

int main() {
    check_refusals();
    check_host_form();
    check_host_refusals();
    if (g_bad) { std::printf("%d checks failed\n", g_bad); return 1; }
    std::printf("flowhosts_host_check: all cases hold\n");
    return 0;
}
