// flowtcp_host_check.cpp — the TCP side table's host part from beatrice_amd/csrc/bt_flowtcp.h and
// bt_flowtrack.h under the host sanitizers: the argument checks of bt_flow_tcp_update_device /
// _host and of the TCP-aware expire (every refusal, and accepted calls with the launch arguments
// they resolve to), the state function, the update on the host (bt::flowtcp_host) over crafted
// frames (both directions, sentinels, ids at flow_cap, a fragment, tags, frames cut by `bytes`), and
// the expire on the host (bt::fk_expire_tcp_host) with truncation and re-appearance. Every table is
// a heap block of exactly its size (an access past it is an AddressSanitizer report). No device,
// no Python, no library to load:
//
//   g++ -std=c++17 -O1 -g -fsanitize=address,undefined -fno-sanitize-recover=all -Iinclude -Ibeatrice_amd/csrc
//       tools/flowtcp_host_check.cpp -o tools/flowtcp_host_check && tools/flowtcp_host_check   (one command line)
//
// Exit 0 = all cases hold.
#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <vector>

#include "bt_flowtrack.h"

using namespace bt;
static int g_bad = 0;
#define CHECK(x) do { if (!(x)) { std::printf("FAILED line %d: %s\n", __LINE__, #x); ++g_bad; } } while (0)

static unsigned char g_frames[256];
static uint64_t g_desc[4];
static uint32_t g_ids[4];
static bt_flow_tcp_rec g_tcp[4];
static bt_flow_tcp_result g_result;
static bt_flow_track_expire_result g_xresult;
alignas(256) static unsigned char g_state[1 << 16];
alignas(256) static unsigned char g_scratch[1 << 16];
static const FkShadow g_shadow{BT_FLOWTAB_BIDIRECTIONAL, 100u, 256u};

struct Call {   // a device update call with nothing wrong
    bt_batch frames{};
    const uint32_t* ids = g_ids;
    uint32_t flags = BT_FLOWTAB_BIDIRECTIONAL;
    bt_flow_tcp_rec* tcp = g_tcp;
    uint32_t cap = 4;
    bt_flow_tcp_result* result = &g_result;
    bool no_frames = false;
    Call() { frames.base = g_frames; frames.desc = g_desc; frames.n = 2; frames.bytes = sizeof(g_frames); }
};

static bool run(const Call& c, FlowtcpArgs* a, const char* word) {
    char why[128];
    if (flowtcp_args(c.no_frames ? nullptr : &c.frames, c.ids, c.flags, c.tcp, c.cap, c.result, a, why, sizeof(why))) return word == nullptr;
    return word && std::strstr(why, word);
}

static bool refuses(const Call& c, const char* word) {
    FlowtcpArgs a;
    return run(c, &a, word);
}

static const uint8_t kA[4] = {10, 0, 0, 1}, kB[4] = {10, 0, 0, 2};

// Ethernet (+ tags) + IPv4 + TCP, 20-byte headers.
static std::vector<uint8_t> tcp_frame(const uint8_t* src, const uint8_t* dst, uint16_t sp, uint16_t dp, uint8_t flags, int tags = 0) {
    std::vector<uint8_t> f(12, 0);
    for (int t = 0; t < tags; ++t) { const uint8_t tag[4] = {0x81, 0x00, 0x00, 0x05}; f.insert(f.end(), tag, tag + 4); }
    f.push_back(0x08); f.push_back(0x00);
    const size_t o3 = f.size();
    f.resize(o3 + 40, 0);
    f[o3] = 0x45; f[o3 + 9] = 6;
    memcpy(&f[o3 + 12], src, 4);
    memcpy(&f[o3 + 16], dst, 4);
    f[o3 + 20] = (uint8_t)(sp >> 8); f[o3 + 21] = (uint8_t)sp; f[o3 + 22] = (uint8_t)(dp >> 8); f[o3 + 23] = (uint8_t)dp;
    f[o3 + 32] = 0x50; f[o3 + 33] = flags;
    return f;
}
static std::vector<uint8_t> up(uint32_t k, uint8_t flags) { return tcp_frame(kA, kB, (uint16_t)(1000 + k), 80, flags); }
static std::vector<uint8_t> down(uint32_t k, uint8_t flags) { return tcp_frame(kB, kA, 80, (uint16_t)(1000 + k), flags); }

struct Batch {   // frames back to back at odd offsets, in a heap block of exactly their size
    std::vector<uint8_t> data;
    std::vector<uint64_t> desc;
    void add(const std::vector<uint8_t>& f) {
        data.resize(data.size() + (4 - data.size() % 4) % 4 + 1, 0);
        desc.push_back(BT_DESC(data.size(), f.size()));
        data.insert(data.end(), f.begin(), f.end());
    }
};

static void test_args() {
    FlowtcpArgs a;
    CHECK(run(Call(), &a, nullptr));
    CHECK(a.n == 2 && a.ntiles == 1 && a.nchunks == 1 && a.bidir == 1 && a.l3_only == 0 && a.flow_cap == 4 && a.tcp == g_tcp &&
          a.flow_id == g_ids && a.result == &g_result && a.bytes == fan_read_end(g_frames, sizeof(g_frames)));
    Call c;
    c.no_frames = true; CHECK(refuses(c, "null frames"));
    c = Call(); c.ids = nullptr; CHECK(refuses(c, "null flow_id"));
    c = Call(); c.ids = nullptr; c.frames.n = 0; CHECK(refuses(c, nullptr));   // an empty batch needs none
    c = Call(); c.tcp = nullptr; CHECK(refuses(c, "null tcp"));
    c = Call(); c.tcp = nullptr; c.cap = 0; CHECK(refuses(c, nullptr));
    c = Call(); c.result = nullptr; CHECK(refuses(c, "null result"));
    c = Call(); c.tcp = reinterpret_cast<bt_flow_tcp_rec*>(reinterpret_cast<char*>(g_tcp) + 2); CHECK(refuses(c, "tcp is not 4-byte aligned"));
    c = Call(); c.ids = reinterpret_cast<const uint32_t*>(reinterpret_cast<const char*>(g_ids) + 1); CHECK(refuses(c, "flow_id is not 4-byte aligned"));
    c = Call(); c.result = reinterpret_cast<bt_flow_tcp_result*>(reinterpret_cast<char*>(&g_result) + 4); CHECK(refuses(c, "result is not 8-byte aligned"));
    c = Call(); c.flags = 4; CHECK(refuses(c, "unknown flag"));
    c = Call(); c.frames.flags = BT_BATCH_PREFIXES; CHECK(refuses(c, "BT_BATCH_PREFIXES"));
    c = Call(); c.frames.flags = BT_BATCH_LEAN; CHECK(refuses(c, "BT_BATCH_PREFIXES"));
    c = Call(); c.frames.bytes = 0; CHECK(refuses(c, "bytes == 0"));
    c = Call(); c.frames.desc_format = 2; CHECK(refuses(c, "desc_format"));
    c = Call(); c.frames.base = nullptr; CHECK(refuses(c, "null packet buffer"));
    c = Call(); c.frames.desc = nullptr; c.frames.stride = 0; CHECK(refuses(c, "stride"));
    c = Call(); c.flags = BT_FLOWTAB_L3_ONLY; CHECK(run(c, &a, nullptr) && a.l3_only == 1 && a.bidir == 0);

    char why[96];
    const bt_pkt_desc* d = reinterpret_cast<const bt_pkt_desc*>(g_desc);
    CHECK(flowtcp_host_args(g_frames, d, 2, g_ids, 3, g_tcp, 4, &g_result, why, sizeof(why)));
    CHECK(!flowtcp_host_args(nullptr, d, 2, g_ids, 0, g_tcp, 4, &g_result, why, sizeof(why)) && std::strstr(why, "null base"));
    CHECK(!flowtcp_host_args(g_frames, d, 2, nullptr, 0, g_tcp, 4, &g_result, why, sizeof(why)) && std::strstr(why, "null flow_id"));
    CHECK(!flowtcp_host_args(g_frames, d, 2, g_ids, 0, nullptr, 4, &g_result, why, sizeof(why)) && std::strstr(why, "null tcp"));
    CHECK(!flowtcp_host_args(g_frames, d, 2, g_ids, 0, g_tcp, 4, nullptr, why, sizeof(why)) && std::strstr(why, "null result"));
    CHECK(!flowtcp_host_args(g_frames, d, 2, g_ids, 8, g_tcp, 4, &g_result, why, sizeof(why)) && std::strstr(why, "unknown flag"));
    CHECK(flowtcp_host_args(nullptr, nullptr, 0, nullptr, 0, nullptr, 0, &g_result, why, sizeof(why)));

    // the TCP-aware expire: its own checks, then the plain expire's, then the larger scratch
    bt_flow_track_expire_out out{};
    out.result = &g_xresult;
    bt_flow_track_expire_tcp x{g_tcp, nullptr, 7};
    FlowexpTcpArgs xa;
    const auto xrun = [&](const bt_flow_track_expire_tcp* xp, const bt_flow_track_expire_out* op, uint64_t sb, const char* word) {
        if (flowtrack_expire_tcp_args(&g_shadow, g_state, 10, 5, xp, g_scratch, sb, op, &xa, why, sizeof(why))) return word == nullptr;
        return word && std::strstr(why, word) != nullptr;
    };
    const uint64_t plain = fx_scratch(100).total, need = fx_tcp_scratch(100).total;
    CHECK(need == plain + ft_round(100 * 16) && need <= sizeof(g_scratch));
    CHECK(xrun(&x, &out, need, nullptr));
    CHECK(xa.tcp == g_tcp && xa.expired_tcp == nullptr && xa.closed_idle == 7 && xa.now == 10 && xa.idle == 5 && xa.flow_cap == 100 &&
          reinterpret_cast<unsigned char*>(xa.tmp_tcp) == g_scratch + plain && xa.all == 1 && xa.result == &g_xresult);
    CHECK(xrun(&x, &out, need - 1, "below the need"));
    CHECK(xrun(&x, &out, plain - 1, "below the need"));
    CHECK(xrun(nullptr, &out, need, "null x"));
    bt_flow_track_expire_tcp bad = x;
    bad.tcp = nullptr; CHECK(xrun(&bad, &out, need, "null tcp"));
    bad = x; bad.tcp = reinterpret_cast<bt_flow_tcp_rec*>(reinterpret_cast<char*>(g_tcp) + 1); CHECK(xrun(&bad, &out, need, "tcp is not 4-byte aligned"));
    bad = x; bad.expired_tcp = g_tcp; CHECK(xrun(&bad, &out, need, "expired_tcp without expired"));
    CHECK(xrun(&x, nullptr, need, "null out"));
    char why2[96];
    CHECK(!flowtrack_expire_tcp_args(nullptr, g_state, 10, 5, &x, g_scratch, need, &out, &xa, why2, sizeof(why2)) &&
          std::strstr(why2, "not an initialised tracker"));
}

static void test_state() {
    const uint32_t B = BT_FLOWTAB_BIDIRECTIONAL, S = BT_TCPF_SYN, A = BT_TCPF_ACK, F = BT_TCPF_FIN, R = BT_TCPF_RST;
    CHECK(flowtcp_state(0, 0, B) == BT_TCP_NONE && flowtcp_state(0, 0, 0) == BT_TCP_NONE);
    CHECK(flowtcp_state(S, 0, B) == BT_TCP_OPENING && flowtcp_state(0, S | A, B) == BT_TCP_OPENING);
    CHECK(flowtcp_state(S | A, S | A, B) == BT_TCP_ESTABLISHED && flowtcp_state(S | A, 0, 0) == BT_TCP_ESTABLISHED);
    CHECK(flowtcp_state(S, 0, 0) == BT_TCP_OPENING);
    CHECK(flowtcp_state(S | A | F, S | A, B) == BT_TCP_CLOSING && flowtcp_state(S | A | F, S | A | F, B) == BT_TCP_CLOSED);
    CHECK(flowtcp_state(A | F, 0, 0) == BT_TCP_CLOSED && flowtcp_state(0, F, 0) == BT_TCP_CLOSING);
    CHECK(flowtcp_state(S | A | F, R, B) == BT_TCP_RESET && flowtcp_state(R, 0, 0) == BT_TCP_RESET);
    CHECK(flowtcp_state(A, A | BT_TCPF_PSH, B) == BT_TCP_MIDSTREAM);
    int seen[7] = {0};
    for (uint32_t f = 0; f < 256; ++f)
        for (uint32_t r = 0; r < 256; ++r) {
            const int s = flowtcp_state(f, r, B);
            CHECK(s >= 0 && s <= 6);
            ++seen[s];
            CHECK(s == flowtcp_state(r, f, B));   // symmetric in the directions when bidirectional
        }
    for (int s = 0; s < 7; ++s) CHECK(seen[s] > 0);
}

static void test_update() {
    const uint8_t S = BT_TCPF_SYN, A = BT_TCPF_ACK, F = BT_TCPF_FIN, R = BT_TCPF_RST;
    Batch b;
    b.add(up(0, S)); b.add(down(0, S | A)); b.add(up(0, A)); b.add(up(1, R)); b.add(up(2, F)); b.add(up(3, S));
    b.add(std::vector<uint8_t>(60, 0)); b.add(up(4, S));
    std::vector<uint32_t> ids = {1, 1, 1, BT_FLOW_ID_UNSELECTED, BT_FLOW_ID_NONE, BT_FLOW_ID_OVERFLOW, 0xFFFFFFFCu, 3};
    std::vector<bt_flow_tcp_rec> tcp(3);   // id 3 is at flow_cap
    memset(static_cast<void*>(tcp.data()), 0, tcp.size() * sizeof(bt_flow_tcp_rec));
    bt_flow_tcp_result r{};
    const bt_pkt_desc* d = reinterpret_cast<const bt_pkt_desc*>(b.desc.data());
    flowtcp_host(b.data.data(), b.data.size(), d, 8, ids.data(), BT_FLOWTAB_BIDIRECTIONAL, tcp.data(), 3, &r);
    CHECK(r.n == 8 && r.tcp_packets == 3 && r.syn_packets == 1 && r.fin_packets == 0 && r.rst_packets == 0 && r.bad_ids == 2);
    CHECK(tcp[1].flags[0] == (S | A) && tcp[1].flags[1] == (S | A) && tcp[1].syn_packets == 1 && tcp[1].pad[0] == 0 && tcp[1].pad[1] == 0);
    CHECK(tcp[0].flags[0] == 0 && tcp[2].flags[0] == 0 && tcp[0].syn_packets == 0);
    // unidirectional: everything in flags[0]; EXPIRED is a sentinel too
    memset(static_cast<void*>(tcp.data()), 0, tcp.size() * sizeof(bt_flow_tcp_rec));
    ids = {0, 2, 0, 1, 1, BT_FLOW_ID_EXPIRED, 0, 0};
    flowtcp_host(b.data.data(), b.data.size(), d, 8, ids.data(), BT_FLOWTAB_L3_ONLY, tcp.data(), 3, &r);
    CHECK(r.tcp_packets == 6 && r.syn_packets == 2 && r.fin_packets == 1 && r.rst_packets == 1 && r.bad_ids == 0);
    CHECK(tcp[0].flags[0] == (S | A) && tcp[0].flags[1] == 0 && tcp[0].syn_packets == 2);
    CHECK(tcp[2].flags[0] == (S | A) && tcp[1].flags[0] == (R | F) && tcp[1].fin_packets == 1 && tcp[1].rst_packets == 1);
    // who contributes: no fragment, no UDP, two tags yes, three tags no; L3_ONLY changes nothing of that
    Batch c;
    std::vector<uint8_t> frag = up(7, S), udp = up(8, S);
    frag[20] = 0x20;
    udp[23] = 17;
    c.add(frag); c.add(udp); c.add(tcp_frame(kA, kB, 9, 9, F | A, 2)); c.add(tcp_frame(kA, kB, 9, 9, R, 3));
    std::vector<uint8_t> shortf = up(9, S);
    shortf.resize(14 + 20 + 19);   // the TCP header is one byte short
    c.add(shortf);
    const bt_pkt_desc* cd = reinterpret_cast<const bt_pkt_desc*>(c.desc.data());
    const uint32_t zero[5] = {0, 0, 0, 0, 0};
    for (uint32_t flags = 0; flags < 4; ++flags) {
        bt_flow_tcp_rec one{};
        flowtcp_host(c.data.data(), c.data.size(), cd, 5, zero, flags, &one, 1, &r);
        CHECK(r.tcp_packets == 1 && r.fin_packets == 1 && r.syn_packets == 0 && one.flags[0] == (F | A) && one.flags[1] == 0);
    }
    // `bytes` cutting the TCP header of the tagged frame: its flags byte reads as zero, the layer stays;
    // cutting the protocol byte: no TCP. The data block ends where `bytes` says (a read past it is a report).
    const uint64_t off = BT_DESC_OFF(c.desc[2]);
    for (uint64_t keep : {off + 55u, off + 31u}) {
        std::vector<uint8_t> part(c.data.begin(), c.data.begin() + (long)keep);
        bt_flow_tcp_rec one{};
        flowtcp_host(part.data(), part.size(), cd + 2, 1, zero, 0, &one, 1, &r);
        CHECK(r.tcp_packets == (keep == off + 55u ? 1u : 0u) && r.fin_packets == 0 && one.flags[0] == 0);
    }
    // n == 0 writes the result
    r.n = 9;
    flowtcp_host(nullptr, 0, nullptr, 0, nullptr, 0, nullptr, 0, &r);
    CHECK(r.n == 0 && r.tcp_packets == 0);
}

struct Tracker {   // a host tracker state and its side table, each a heap block of exactly its size
    std::vector<uint8_t> raw;
    uint8_t* state;
    bt_flow_track_sizes lay{};
    FkHostState hs{};
    std::vector<bt_flow_tcp_rec> tcp;
    Tracker(uint32_t cap, uint32_t flags) : tcp(cap) {
        char why[96];
        CHECK(fk_layout(cap, 0, &lay, why, sizeof(why)));
        raw.resize(lay.total + 256);
        state = raw.data() + (256 - reinterpret_cast<uintptr_t>(raw.data()) % 256) % 256;
        const bt_flow_track_opts o{flags, cap, 0, 0};
        fk_init_host(state, o, lay);
        CHECK(fk_host_state(state, lay.total, &hs, why, sizeof(why)));
        memset(static_cast<void*>(tcp.data()), 0, tcp.size() * sizeof(bt_flow_tcp_rec));
    }
    std::vector<uint32_t> update(const Batch& b, uint64_t ts) {
        const uint32_t n = (uint32_t)b.desc.size();
        std::vector<uint32_t> ids(n);
        bt_flow_track_result r{};
        const bt_pkt_desc* d = reinterpret_cast<const bt_pkt_desc*>(b.desc.data());
        fk_update_host(hs, b.data.data(), b.data.size(), d, n, nullptr, nullptr, ts, ids.data(), &r);
        bt_flow_tcp_result t{};
        flowtcp_host(b.data.data(), b.data.size(), d, n, ids.data(), hs.hdr->flags, tcp.data(), (uint32_t)tcp.size(), &t);
        CHECK(t.bad_ids == 0 && t.n == n);
        return ids;
    }
    int state_of(uint32_t f) const { return flowtcp_state(tcp[f].flags[0], tcp[f].flags[1], hs.hdr->flags); }
};

static void test_expire() {
    const uint8_t S = BT_TCPF_SYN, A = BT_TCPF_ACK, F = BT_TCPF_FIN, R = BT_TCPF_RST;
    Tracker t(8, BT_FLOWTAB_BIDIRECTIONAL);
    Batch b;
    b.add(up(0, S)); b.add(down(0, S | A)); b.add(up(0, A)); b.add(up(0, F | A)); b.add(down(0, F | A));
    b.add(up(1, S)); b.add(down(1, R | A));
    b.add(up(2, S)); b.add(down(2, S | A)); b.add(down(2, F | A));
    b.add(up(3, S)); b.add(down(3, S | A));
    const std::vector<uint32_t> ids = t.update(b, 100);
    CHECK(ids[4] == 0 && ids[6] == 1 && ids[9] == 2 && ids[11] == 3 && t.hs.hdr->n_flows == 4);
    CHECK(t.state_of(0) == BT_TCP_CLOSED && t.state_of(1) == BT_TCP_RESET && t.state_of(2) == BT_TCP_CLOSING && t.state_of(3) == BT_TCP_ESTABLISHED);
    std::vector<bt_flow_track_rec> exp(1);
    std::vector<bt_flow_tcp_rec> exp_tcp(1);
    std::vector<uint32_t> remap(8, 0xEEEEEEEEu);
    bt_flow_track_expire_result r{};
    bt_flow_track_expire_out out{exp.data(), 1, 0, remap.data(), &r};
    bt_flow_track_expire_tcp x{t.tcp.data(), exp_tcp.data(), 10};
    fk_expire_tcp_host(t.hs, 110, 1000, &x, &out);   // now - last_ts == closed_idle: nobody leaves
    CHECK(r.n_idle == 0 && r.n_expired == 0 && r.n_flows == 4 && remap[3] == 3 && remap[4] == 0xEEEEEEEEu);
    fk_expire_tcp_host(t.hs, 111, 1000, &x, &out);   // the closed and the reset one; room for one
    CHECK(r.n_idle == 2 && r.n_expired == 1 && r.n_flows == 3 && remap[0] == BT_FLOW_ID_EXPIRED && remap[1] == 0 && remap[3] == 2);
    CHECK(exp_tcp[0].flags[0] == (S | A | F) && exp_tcp[0].flags[1] == (S | A | F) && exp_tcp[0].fin_packets == 2 && exp[0].packets[0] == 3);
    CHECK(t.state_of(0) == BT_TCP_RESET && t.state_of(1) == BT_TCP_CLOSING && t.state_of(2) == BT_TCP_ESTABLISHED);
    CHECK(t.tcp[3].flags[0] == 0 && t.tcp[3].flags[1] == 0 && t.tcp[3].syn_packets == 0);
    fk_expire_tcp_host(t.hs, 111, 1000, &x, &out);
    CHECK(r.n_idle == 1 && r.n_expired == 1 && r.n_flows == 2 && exp_tcp[0].rst_packets == 1);
    // closed_idle = 2^64 - 1: the idle rule alone, as fk_expire_host
    x.closed_idle = ~0ull;
    fk_expire_tcp_host(t.hs, 1100, 1000, &x, &out);
    CHECK(r.n_idle == 0 && r.n_flows == 2);
    // a key that left appears again: a new flow at the end with a zero side record before its packets
    Batch again;
    again.add(up(0, S));
    CHECK(t.update(again, 120)[0] == 2 && t.state_of(2) == BT_TCP_OPENING && t.tcp[2].syn_packets == 1);
    // expired == NULL drops every leaving flow; no remap
    bt_flow_track_expire_out drop{nullptr, 0, 0, nullptr, &r};
    x.expired_tcp = nullptr;
    x.closed_idle = 0;
    fk_expire_tcp_host(t.hs, 1101, 1000, &x, &drop);   // flows 0 and 1 are idle; flow 2 is open and young
    CHECK(r.n_idle == 2 && r.n_expired == 2 && r.n_flows == 1 && t.state_of(0) == BT_TCP_OPENING && t.tcp[1].flags[0] == 0);
}

int main() {
    test_args();
    test_state();
    test_update();
    test_expire();
    if (g_bad) { std::printf("%d checks failed\n", g_bad); return 1; }
    std::printf("flowtcp_host_check: all cases hold\n");
    return 0;
}
