// flowstat_host_check.cpp — the statistics side table's host part from beatrice_amd/csrc/bt_flowstat.h
// under the host sanitizers: the argument checks of bt_flow_stat_update_device / _host and of the
// side move (refusals, and accepted calls with the launch arguments they resolve to), the update
// on the host (bt::flowstat_host) over generated frames whose facts are known by construction
// (protocol, TTL, length, payload, TCP flags, direction, VLAN tags, fragments, frames cut by
// `bytes`), bt::flowstat_rtt, and the move on the host (bt::flowside_host), each held to a naive
// per-flow loop over a std::map. Every table is a heap block of exactly its size (an access past
// it is an AddressSanitizer report). No device, no Python, no library to load:
//
//   g++ -std=c++17 -O1 -g -fsanitize=address,undefined -fno-sanitize-recover=all -Iinclude -Ibeatrice_amd/csrc
//       tools/flowstat_host_check.cpp -o tools/flowstat_host_check && tools/flowstat_host_check   (one command line)
//
// Exit 0 = all cases hold.
#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <map>
#include <vector>

#include "bt_flowstat.h"

using namespace bt;
static int g_bad = 0;
#define CHECK(x) do { if (!(x)) { std::printf("FAILED line %d: %s\n", __LINE__, #x); ++g_bad; } } while (0)

static uint32_t g_rng = 12345u;
static uint32_t rnd(uint32_t below) {
    g_rng = g_rng * 1664525u + 1013904223u;
    return (g_rng >> 8) % below;
}

struct Packet {   // what a generated frame contributes, known before the frame is built
    std::vector<uint8_t> frame;
    bool ip = false, l4 = false, tcp = false;
    uint32_t seen = 0, proto = 0, ttl = 0, payload = 0, dir = 0, stamp = 3;
    uint64_t ts = 0;
};

// Ethernet (+ tags) + IPv4 or IPv6 + TCP / UDP / something else; endpoint A < B, reverse: B sends.
static Packet make(uint32_t conv, bool reverse, bool v6, uint32_t proto, uint8_t flags, uint32_t tags, bool fragment, uint32_t pay,
                   uint32_t ttl, uint64_t ts) {
    Packet p;
    std::vector<uint8_t>& f = p.frame;
    f.assign(12, 0);
    for (uint32_t t = 0; t < tags; ++t) { const uint8_t tag[4] = {0x81, 0x00, 0x00, 0x05}; f.insert(f.end(), tag, tag + 4); }
    f.push_back(v6 ? 0x86 : 0x08); f.push_back(v6 ? 0xDD : 0x00);
    const size_t o3 = f.size();
    const uint32_t l4len = proto == 6 ? 20u : proto == 17 ? 8u : 4u;
    const uint8_t a = 1, b = 2;
    if (v6) {
        f.resize(o3 + 40, 0);
        f[o3] = 0x60; f[o3 + 4] = (uint8_t)((l4len + pay) >> 8); f[o3 + 5] = (uint8_t)(l4len + pay); f[o3 + 6] = (uint8_t)proto;
        f[o3 + 7] = (uint8_t)ttl;
        f[o3 + 23] = reverse ? b : a; f[o3 + 39] = reverse ? a : b;
        f[o3 + 22] = f[o3 + 38] = (uint8_t)conv;
    } else {
        f.resize(o3 + 20, 0);
        const uint32_t total = 20u + l4len + pay;
        f[o3] = 0x45; f[o3 + 2] = (uint8_t)(total >> 8); f[o3 + 3] = (uint8_t)total; f[o3 + 6] = fragment ? 0x20 : 0x40;
        f[o3 + 8] = (uint8_t)ttl; f[o3 + 9] = (uint8_t)proto;
        f[o3 + 12] = f[o3 + 16] = 10; f[o3 + 14] = f[o3 + 18] = (uint8_t)conv;
        f[o3 + 15] = reverse ? b : a; f[o3 + 19] = reverse ? a : b;
    }
    const size_t o4 = f.size();
    f.resize(o4 + l4len, 0);
    if (proto == 6 || proto == 17) {   // the same port on both sides: the addresses decide the direction
        f[o4] = f[o4 + 2] = 0x12; f[o4 + 1] = f[o4 + 3] = (uint8_t)conv;
    }
    if (proto == 6) { f[o4 + 12] = 0x50; f[o4 + 13] = flags; }
    f.resize(f.size() + (pay < 40 ? pay : 40), 0);   // a snapped capture: the payload is cut, the header fields are not
    p.ip = true;
    p.proto = proto; p.ttl = ttl; p.dir = reverse ? 1u : 0u; p.ts = ts;
    p.seen = proto == 6 ? BT_FSEEN_TCP : proto == 17 ? BT_FSEEN_UDP : !v6 && proto == 1 ? BT_FSEEN_ICMP
             : v6 && proto == 58 ? BT_FSEEN_ICMP6 : BT_FSEEN_OTHER;
    if (fragment && !v6) p.seen |= BT_FSEEN_FRAGMENT;
    if (tags) p.seen |= BT_FSEEN_VLAN;
    p.l4 = (proto == 6 || proto == 17) && !(fragment && !v6);
    p.tcp = p.l4 && proto == 6;
    if (p.l4) { p.seen |= BT_FSEEN_L4; p.payload = pay; }
    if (p.tcp) p.stamp = (flags & 2) ? ((flags & 16) ? 1u : 0u) : (flags & 16) && !(flags & 4) ? 2u : 3u;
    return p;
}

struct Batch {   // frames back to back at odd offsets, in a heap block of exactly their size
    std::vector<uint8_t> data;
    std::vector<uint64_t> desc;
    void add(const std::vector<uint8_t>& f) {
        data.resize(data.size() + (4 - data.size() % 4) % 4 + 1, 0);
        desc.push_back(BT_DESC(data.size(), f.size()));
        data.insert(data.end(), f.begin(), f.end());
    }
};

// The naive form: every packet of a flow kept, then one loop per flow.
static bt_flow_stat_rec naive(const std::vector<const Packet*>& ps, bool bidir, const bt_flow_stat_rec& start) {
    bt_flow_stat_rec r = start;
    for (const Packet* p : ps) {
        const uint32_t d = bidir ? p->dir : 0u, len = (uint32_t)p->frame.size();
        r.seen |= p->seen << (16u * d);
        if (p->proto > r.proto_max) r.proto_max = p->proto;
        if (p->ttl > r.ttl_max[d]) r.ttl_max[d] = p->ttl;
        if (~p->ttl > r.ttl_min_c[d]) r.ttl_min_c[d] = ~p->ttl;
        if (len > r.len_max[d]) r.len_max[d] = len;
        if (~len > r.len_min_c[d]) r.len_min_c[d] = ~len;
        r.len_sq[d] += (uint64_t)len * len;
        r.payload_bytes[d] += p->payload;
        r.payload_packets[d] += p->payload ? 1u : 0u;
        uint64_t* const to = p->stamp == 0 ? r.syn_ts_c : p->stamp == 1 ? r.synack_ts_c : p->stamp == 2 ? r.ack_ts_c : nullptr;
        if (to && ~p->ts > to[d]) to[d] = ~p->ts;
    }
    return r;
}

static void test_update(uint32_t table_flags, bool per_packet_ts) {
    const bool bidir = table_flags & BT_FLOWTAB_BIDIRECTIONAL;
    const uint32_t cap = 37, n = 3000;
    static const uint32_t protos[6] = {6, 6, 6, 17, 1, 47};
    std::vector<Packet> ps;
    Batch b;
    std::vector<uint32_t> ids;
    std::vector<uint64_t> ts;
    for (uint32_t i = 0; i < n; ++i) {
        const bool v6 = rnd(4) == 0;
        const uint32_t proto = v6 && rnd(8) == 0 ? 58u : protos[rnd(6)];
        const uint64_t t = rnd(50) == 0 ? ~0ull - rnd(2) : rnd(100000);
        ps.push_back(make(rnd(200), rnd(2), v6, proto, (uint8_t)rnd(32), rnd(3), rnd(10) == 0, rnd(4) ? rnd(1400) : 0, 1 + rnd(255),
                          per_packet_ts ? t : 777u));
        b.add(ps.back().frame);
        const uint32_t kind = rnd(20);
        static const uint32_t other[5] = {BT_FLOW_ID_UNSELECTED, BT_FLOW_ID_NONE, BT_FLOW_ID_OVERFLOW, BT_FLOW_ID_EXPIRED, 0xFFFFFFFCu};
        ids.push_back(kind == 0 ? other[rnd(5)] : kind == 1 ? cap + rnd(3) : rnd(cap));
        ts.push_back(ps.back().ts);
    }
    std::vector<uint8_t> arp(60, 0);
    arp[12] = 0x08; arp[13] = 0x06;
    b.add(arp);
    ps.emplace_back();
    ps.back().frame = arp;
    ids.push_back(0);
    ts.push_back(1);

    std::vector<bt_flow_stat_rec> start(cap), got;
    for (uint32_t f = 0; f < cap; f += 5) {   // some records already hold something
        start[f].seen = 0x00800080u; start[f].ttl_max[0] = 300; start[f].len_min_c[1] = ~40u; start[f].payload_packets[0] = 0xFFFFFFFFu;
        start[f].len_sq[0] = ~0ull - 5u; start[f].syn_ts_c[0] = ~50ull;
    }
    got = start;
    bt_flow_stat_result res{};
    const bt_flow_track_update upd{per_packet_ts ? ts.data() : nullptr, 777u};
    char why[96];
    const bt_pkt_desc* d = reinterpret_cast<const bt_pkt_desc*>(b.desc.data());
    CHECK(flowstat_host_args(b.data.data(), d, n + 1, ids.data(), table_flags, &upd, got.data(), cap, &res, why, sizeof(why)));
    flowstat_host(b.data.data(), b.data.size(), d, n + 1, ids.data(), table_flags, &upd, got.data(), cap, &res);

    std::map<uint32_t, std::vector<const Packet*>> by_flow;
    bt_flow_stat_result want{};
    want.n = n + 1;
    for (uint32_t i = 0; i <= n; ++i) {
        if (ids[i] >= cap) { want.bad_ids += flowtcp_is_sentinel(ids[i]) ? 0u : 1u; continue; }
        if (!ps[i].ip) continue;
        by_flow[ids[i]].push_back(&ps[i]);
        ++want.ip_packets; want.l4_packets += ps[i].l4; want.tcp_packets += ps[i].tcp;
    }
    CHECK(memcmp(&res, &want, sizeof(res)) == 0 && want.bad_ids > 0 && want.tcp_packets > 0 && want.l4_packets > want.tcp_packets);
    for (uint32_t f = 0; f < cap; ++f) {
        const bt_flow_stat_rec w = naive(by_flow[f], bidir, start[f]);
        CHECK(memcmp(&w, &got[f], sizeof(w)) == 0);
    }
    CHECK(bidir == ((got[1].seen >> 16) != 0));

    // `bytes` cutting the last IP frame anywhere: nothing past it is read (the block ends there), and a cut header reads as zeros
    const uint64_t off = BT_DESC_OFF(d[n - 1]);
    for (uint64_t cut = off; cut <= off + ps[n - 1].frame.size(); ++cut) {
        std::vector<uint8_t> part(b.data.begin(), b.data.begin() + (ptrdiff_t)cut);
        if (part.empty()) part.push_back(0);
        bt_flow_stat_rec one{};
        const uint32_t zero = 0;
        flowstat_host(part.data(), cut, d + (n - 1), 1, &zero, table_flags, &upd, &one, 1, &res);
        CHECK(res.n == 1 && res.ip_packets <= 1);
        if (cut == off + ps[n - 1].frame.size()) CHECK(res.ip_packets == 1 && one.proto_max == ps[n - 1].proto);
        if (cut < off + 13) CHECK(res.ip_packets == 0);   // with byte 12 alone an EtherType 0x08 0x00 still reads as IPv4
    }
}

static bt_flow_stat_rec stamps(uint64_t s0, uint64_t s1, uint64_t sa0, uint64_t sa1, uint64_t a0, uint64_t a1) {   // ~0 = absent
    bt_flow_stat_rec r{};
    r.syn_ts_c[0] = ~s0; r.syn_ts_c[1] = ~s1; r.synack_ts_c[0] = ~sa0; r.synack_ts_c[1] = ~sa1; r.ack_ts_c[0] = ~a0; r.ack_ts_c[1] = ~a1;
    return r;
}

static void test_rtt() {
    const uint64_t no = ~0ull;
    bt_flow_stat_rtt_out o;
    flowstat_rtt(stamps(no, no, 3, 4, 5, 6), &o);
    CHECK(!o.has_initiator && !o.server_valid && !o.client_valid && !o.rtt_server && !o.rtt_client);
    flowstat_rtt(stamps(5, no, no, no, no, no), &o);
    CHECK(o.has_initiator && o.initiator == 0 && !o.server_valid && !o.client_valid);
    flowstat_rtt(stamps(5, no, no, 12, 20, no), &o);
    CHECK(o.initiator == 0 && o.server_valid && o.rtt_server == 7 && o.client_valid && o.rtt_client == 8);
    flowstat_rtt(stamps(no, 5, 12, no, no, 20), &o);
    CHECK(o.initiator == 1 && o.server_valid && o.rtt_server == 7 && o.client_valid && o.rtt_client == 8);
    flowstat_rtt(stamps(9, 9, 11, 10, 30, 40), &o);
    CHECK(o.initiator == 0 && o.rtt_server == 1 && o.rtt_client == 20);
    flowstat_rtt(stamps(9, 8, 11, 10, 30, 40), &o);
    CHECK(o.initiator == 1 && o.rtt_server == 3 && o.rtt_client == 29);
    flowstat_rtt(stamps(10, no, no, 9, 20, no), &o);
    CHECK(o.has_initiator && !o.server_valid && !o.client_valid && !o.rtt_client);
    flowstat_rtt(stamps(10, no, no, 15, 14, no), &o);
    CHECK(o.server_valid && o.rtt_server == 5 && !o.client_valid);
    flowstat_rtt(stamps(0, no, no, no - 1, no - 1, no), &o);
    CHECK(o.server_valid && o.rtt_server == no - 1 && o.client_valid && o.rtt_client == 0);
}

static void test_move(uint32_t rec_bytes, uint32_t cap, uint32_t nb, uint32_t expired_cap, bool with_gone) {
    const uint32_t rw = rec_bytes / 4u;
    std::vector<uint32_t> side((size_t)cap * rw), remap(cap, 0xEEEEEEEEu);
    for (size_t w = 0; w < side.size(); ++w) side[w] = 0x10000u + (uint32_t)w;
    const std::vector<uint32_t> before = side;
    uint32_t nl = 0, ne = 0;
    for (uint32_t f = 0; f < nb; ++f) {
        if (rnd(3) == 0) { remap[f] = BT_FLOW_ID_EXPIRED; ++ne; }
        else remap[f] = nl++;
    }
    bt_flow_track_expire_result res{};
    res.n_flows_before = nb; res.n_flows = nl; res.n_idle = ne; res.n_expired = ne;
    std::vector<uint32_t> gone((size_t)expired_cap * rw, 0xABABABABu);
    bt_flow_side_move m{};
    m.side = cap ? side.data() : nullptr; m.expired_side = with_gone ? gone.data() : nullptr; m.remap = cap ? remap.data() : nullptr;
    m.result = &res; m.rec_bytes = rec_bytes; m.flow_cap = cap; m.expired_cap = with_gone ? expired_cap : 0;
    if (with_gone && gone.empty()) { m.expired_side = nullptr; m.expired_cap = 0; }
    char why[128];
    CHECK(flowside_common_args(&m, why, sizeof(why)));
    flowside_host(&m);
    // naive: where every new number comes from
    std::map<uint32_t, uint32_t> from;
    std::vector<uint32_t> left;
    for (uint32_t f = 0; f < nb; ++f) {
        if (remap[f] == BT_FLOW_ID_EXPIRED) left.push_back(f);
        else from[remap[f]] = f;
    }
    for (uint32_t f = 0; f < cap; ++f)
        for (uint32_t j = 0; j < rw; ++j) {
            const uint32_t got = side[(size_t)f * rw + j];
            if (ne == 0 || f >= nb) CHECK(got == before[(size_t)f * rw + j]);
            else if (f >= nl) CHECK(got == 0);
            else CHECK(got == before[(size_t)from[f] * rw + j]);
        }
    for (uint32_t k = 0; k < (uint32_t)(gone.size() / rw); ++k)
        for (uint32_t j = 0; j < rw; ++j) {
            const bool written = m.expired_side && k < ne && ne != 0;
            CHECK(gone[(size_t)k * rw + j] == (written ? before[(size_t)left[k] * rw + j] : 0xABABABABu));
        }
}

static void test_move_args() {
    alignas(256) static unsigned char scratch[1 << 14];
    static uint32_t side[64], remap[4];
    static bt_flow_track_expire_result res;
    char why[128];
    FlowsideArgs a;
    bt_flow_side_move m{side, nullptr, remap, &res, 16, 4, 0, 0};
    CHECK(flowside_args(&m, scratch, sizeof(scratch), &a, why, sizeof(why)) && a.rec_words == 4 && a.flow_cap == 4 && a.expired_cap == 0 &&
          a.tmp == reinterpret_cast<uint32_t*>(scratch) && reinterpret_cast<unsigned char*>(a.parts) == scratch + 256);
    CHECK(fs_scratch(4, 16).total == 512 && fs_scratch(257, 128).total == ft_round(257 * 128) + 256 && fs_scratch(0, 4).total == 0);
    const auto refuses = [&](const bt_flow_side_move& x, void* s, uint64_t nbytes, const char* word) {
        return !flowside_args(&x, s, nbytes, &a, why, sizeof(why)) && std::strstr(why, word);
    };
    bt_flow_side_move x = m;
    CHECK(!flowside_args(nullptr, scratch, sizeof(scratch), &a, why, sizeof(why)) && std::strstr(why, "null move"));
    x = m; x.side = nullptr; CHECK(refuses(x, scratch, sizeof(scratch), "null side"));
    x = m; x.remap = nullptr; CHECK(refuses(x, scratch, sizeof(scratch), "null remap"));
    x = m; x.result = nullptr; CHECK(refuses(x, scratch, sizeof(scratch), "null result"));
    x = m; x.side = reinterpret_cast<char*>(side) + 2; CHECK(refuses(x, scratch, sizeof(scratch), "side is not 4-byte aligned"));
    x = m; x.rec_bytes = 0; CHECK(refuses(x, scratch, sizeof(scratch), "rec_bytes"));
    x = m; x.rec_bytes = 18; CHECK(refuses(x, scratch, sizeof(scratch), "rec_bytes"));
    x = m; x.rec_bytes = 260; CHECK(refuses(x, scratch, sizeof(scratch), "rec_bytes"));
    x = m; x.expired_cap = 1; CHECK(refuses(x, scratch, sizeof(scratch), "without expired_side"));
    x = m; x.reserved = 1; CHECK(refuses(x, scratch, sizeof(scratch), "reserved"));
    CHECK(refuses(m, nullptr, sizeof(scratch), "null scratch"));
    CHECK(refuses(m, scratch + 16, sizeof(scratch), "256-byte aligned"));
    CHECK(refuses(m, scratch, 511, "scratch_bytes"));
}

static void test_update_args() {
    static unsigned char frames[256];
    static uint64_t desc[4], ts[4];
    static uint32_t ids[4];
    static bt_flow_stat_rec stat[4];
    static bt_flow_stat_result result;
    bt_batch b{};
    b.base = frames; b.desc = desc; b.n = 2; b.bytes = sizeof(frames);
    const bt_flow_track_update upd{ts, 9};
    FlowstatArgs a;
    char why[128];
    CHECK(flowstat_args(&b, ids, BT_FLOWTAB_BIDIRECTIONAL, &upd, stat, 4, &result, &a, why, sizeof(why)));
    CHECK(a.n == 2 && a.ntiles == 1 && a.nchunks == 1 && a.bidir == 1 && a.l3_only == 0 && a.flow_cap == 4 && a.stat == stat && a.ts == ts &&
          a.batch_ts == 9 && a.flow_id == ids && a.result == &result && a.bytes == fan_read_end(frames, sizeof(frames)));
    const auto refuses = [&](const bt_batch* f, const uint32_t* id, uint32_t flags, const bt_flow_track_update* u, bt_flow_stat_rec* s,
                             bt_flow_stat_result* r, const char* word) {
        return !flowstat_args(f, id, flags, u, s, 4, r, &a, why, sizeof(why)) && std::strstr(why, word);
    };
    CHECK(refuses(nullptr, ids, 0, &upd, stat, &result, "null frames"));
    CHECK(refuses(&b, nullptr, 0, &upd, stat, &result, "null flow_id"));
    CHECK(refuses(&b, ids, 0, nullptr, stat, &result, "null upd"));
    CHECK(refuses(&b, ids, 0, &upd, nullptr, &result, "null stat"));
    CHECK(refuses(&b, ids, 0, &upd, stat, nullptr, "null result"));
    CHECK(refuses(&b, ids, 4, &upd, stat, &result, "unknown flag"));
    CHECK(refuses(&b, ids, 0, &upd, reinterpret_cast<bt_flow_stat_rec*>(reinterpret_cast<char*>(stat) + 4), &result, "stat is not 8-byte"));
    const bt_flow_track_update odd{reinterpret_cast<const uint64_t*>(reinterpret_cast<const char*>(ts) + 4), 0};
    CHECK(refuses(&b, ids, 0, &odd, stat, &result, "ts is not 8-byte"));
    bt_batch lean = b;
    lean.flags = BT_BATCH_LEAN;
    CHECK(refuses(&lean, ids, 0, &upd, stat, &result, "BT_BATCH_PREFIXES"));
    bt_batch empty = b;
    empty.n = 0;
    CHECK(flowstat_args(&empty, nullptr, 0, &upd, nullptr, 0, &result, &a, why, sizeof(why)) && a.nchunks == 0);
}

int main() {
    test_update_args();
    test_move_args();
    for (uint32_t flags = 0; flags < 4; ++flags) {
        test_update(flags, true);
        test_update(flags, false);
    }
    test_rtt();
    for (uint32_t rb : {4u, 16u, 128u, 256u})
        for (uint32_t cap : {1u, 255u, 256u, 257u, 1000u}) {
            test_move(rb, cap, cap, cap, true);
            test_move(rb, cap, cap - cap / 3, 3, true);
            test_move(rb, cap, cap / 2, 0, false);
        }
    test_move(8, 0, 0, 0, false);
    if (g_bad) { std::printf("%d checks failed\n", g_bad); return 1; }
    std::printf("flowstat_host_check: all cases hold\n");
    return 0;
}
