// flowtab_host_check.cpp — the argument checks of bt_flow_table_device (bt::flowtab_args), the
// scratch layout and the host group-by that bt_flow_table_host wraps (bt::flowtab_host,
// bt::ft_canonical), from beatrice_amd/csrc/bt_flowtab.h, under the host sanitizers: every
// refusal, accepted calls with the launch arguments they resolve to, crafted conversations in
// both directions, fragments, a full table, overflow, and frames cut at every length with the
// buffer a heap block of exactly `bytes` (a read past it is an AddressSanitizer report). No
// device, no Python, no library to load:
//
//   g++ -std=c++17 -O1 -g -fsanitize=address,undefined -fno-sanitize-recover=all -Iinclude -Ibeatrice_amd/csrc
//       tools/flowtab_host_check.cpp -o tools/flowtab_host_check && tools/flowtab_host_check   (one command line)
//
// Exit 0 = all cases hold.
#include <cstdio>
#include <cstring>
#include <vector>

#include "bt_flowtab.h"

using namespace bt;
static int g_bad = 0;
#define CHECK(x) do { if (!(x)) { std::printf("FAILED line %d: %s\n", __LINE__, #x); ++g_bad; } } while (0)

static unsigned char g_frames[256];
static uint64_t g_desc[4];
static bt_flow_table_result g_result;
alignas(256) static unsigned char g_scratch[1 << 16];

struct Call {
    bt_batch frames{};
    bt_flow_table_opts opts{};
    bt_flow_table_out out{};
    void* scratch = g_scratch;
    uint64_t scratch_bytes = sizeof(g_scratch);
    bool no_frames = false, no_opts = false, no_out = false;   // pass a null pointer instead
    Call() {
        frames.base = g_frames; frames.desc = g_desc; frames.n = 2; frames.bytes = sizeof(g_frames);
        out.result = &g_result;
    }
};

static bool run(const Call& c, FlowtabArgs* a, const char* word, size_t cap = 96) {
    std::vector<char> why(cap, '?');
    const bool ok = flowtab_args(c.no_frames ? nullptr : &c.frames, nullptr, c.no_opts ? nullptr : &c.opts, c.scratch, c.scratch_bytes,
                                 c.no_out ? nullptr : &c.out, a, why.data(), cap);
    if (ok) return word == nullptr;
    return word && std::strlen(why.data()) < cap && std::strstr(why.data(), word);
}

static bool refuses(const Call& c, const char* word, size_t cap = 96) {
    FlowtabArgs a;
    return run(c, &a, word, cap);
}

// Ethernet + IPv4 + TCP / UDP (or proto 1: eight bytes of ICMP) between two hosts 10.0.0.x.
static std::vector<uint8_t> v4_frame(uint8_t src, uint8_t dst, uint16_t sp, uint16_t dp, int proto = 6, uint16_t frag = 0) {
    std::vector<uint8_t> f(12, 0);
    f.push_back(0x08); f.push_back(0x00);
    const size_t o3 = f.size();
    f.resize(o3 + 20, 0);
    f[o3] = 0x45; f[o3 + 6] = (uint8_t)(frag >> 8); f[o3 + 7] = (uint8_t)frag; f[o3 + 9] = (uint8_t)proto;
    const uint8_t addr[8] = {10, 0, 0, src, 10, 0, 0, dst};
    memcpy(&f[o3 + 12], addr, 8);
    const uint8_t ports[4] = {(uint8_t)(sp >> 8), (uint8_t)sp, (uint8_t)(dp >> 8), (uint8_t)dp};
    f.insert(f.end(), ports, ports + 4);
    f.resize(f.size() + (proto == 6 ? 16 : 4), 0);
    return f;
}

static std::vector<uint8_t> v6_frame(uint8_t src, uint8_t dst, uint16_t sp, uint16_t dp, int nh = 6) {
    std::vector<uint8_t> f(12, 0);
    f.push_back(0x86); f.push_back(0xDD);
    const size_t o3 = f.size();
    f.resize(o3 + 40, 0);
    f[o3] = 0x60; f[o3 + 6] = (uint8_t)nh;
    f[o3 + 8] = 0x20; f[o3 + 23] = src; f[o3 + 24] = 0x20; f[o3 + 39] = dst;
    const uint8_t ports[4] = {(uint8_t)(sp >> 8), (uint8_t)sp, (uint8_t)(dp >> 8), (uint8_t)dp};
    f.insert(f.end(), ports, ports + 4);
    f.resize(f.size() + 16, 0);
    return f;
}

// A batch in a heap block of exactly its size (or of `bytes`, cutting the last frames).
struct Batch {
    std::vector<uint8_t> data;
    std::vector<uint64_t> desc;
    void add(const std::vector<uint8_t>& f) {
        data.push_back(0xEE);   // odd offsets
        desc.push_back(BT_DESC(data.size(), f.size()));
        data.insert(data.end(), f.begin(), f.end());
    }
};

struct Result {
    std::vector<uint32_t> id;
    std::vector<bt_flow_rec> flows;
    bt_flow_table_result r{};
};

static Result table(const Batch& b, uint32_t flags, uint32_t slots = 128, const uint64_t* select = nullptr, uint64_t bytes = ~0ull,
                    uint32_t cap = 64) {
    const uint64_t have = bytes == ~0ull ? b.data.size() : bytes;
    std::vector<uint8_t> exact(b.data.begin(), b.data.begin() + have);   // reads past `bytes` are reports
    Result o;
    o.id.assign(b.desc.size(), 0x55555555u);
    o.flows.resize(cap);
    flowtab_host(exact.data(), have, b.desc.data(), (uint32_t)b.desc.size(), select, flags, slots, cap, o.id.data(), o.flows.data(),
                 &o.r);
    o.flows.resize(o.r.n_written);
    return o;
}

int main() {
    Call c;
    c = Call{}; c.no_frames = true;                              CHECK(refuses(c, "null frames"));
    c = Call{}; c.no_opts = true;                                CHECK(refuses(c, "null opts"));
    c = Call{}; c.no_out = true;                                 CHECK(refuses(c, "null out"));
    c = Call{}; c.out.result = nullptr;                          CHECK(refuses(c, "null result"));
    c = Call{}; c.out.result = reinterpret_cast<bt_flow_table_result*>(reinterpret_cast<char*>(&g_result) + 4);
    CHECK(refuses(c, "result is not 8-byte aligned"));
    c = Call{}; c.scratch = g_scratch + 64;                      CHECK(refuses(c, "scratch is not 256-byte aligned"));
    c = Call{}; c.scratch = nullptr;                             CHECK(refuses(c, "null scratch"));
    c = Call{}; c.scratch_bytes = ft_layout(2, 128).total - 1;   CHECK(refuses(c, "below the need"));
    c = Call{}; c.scratch_bytes = ft_layout(2, 128).total;       CHECK(!refuses(c, "below the need"));
    c = Call{}; c.opts.slots = 1u << 20;                         CHECK(refuses(c, "below the need"));
    c = Call{}; c.opts.flags = 0x4;                              CHECK(refuses(c, "flag"));
    c = Call{}; c.opts.flags = 0x80000000u;                      CHECK(refuses(c, "flag"));
    c = Call{}; c.opts.slots = 129;                              CHECK(refuses(c, "power of two"));
    c = Call{}; c.opts.slots = 3u << 10;                         CHECK(refuses(c, "power of two"));
    c = Call{}; c.opts.slots = 64;                               CHECK(refuses(c, "below 128"));
    c = Call{}; c.opts.slots = 1;                                CHECK(refuses(c, "below 128"));
    c = Call{}; c.frames.n = (1u << 30) + 1u;                    CHECK(refuses(c, "auto"));
    c = Call{}; c.frames.n = 0xFFFFFFFDu; c.opts.slots = 128;    CHECK(refuses(c, "n above"));
    c = Call{}; c.opts.flow_cap = 1;                             CHECK(refuses(c, "null flows"));
    c = Call{}; c.out.flows = reinterpret_cast<bt_flow_rec*>(g_scratch + 4); c.opts.flow_cap = 1; CHECK(refuses(c, "flows is not"));
    c = Call{}; c.out.flow_id = reinterpret_cast<uint32_t*>(g_scratch + 2); CHECK(refuses(c, "flow_id is not"));
    c = Call{}; c.frames.flags = BT_BATCH_PREFIXES;              CHECK(refuses(c, "PREFIXES"));
    c = Call{}; c.frames.flags = BT_BATCH_LEAN;                  CHECK(refuses(c, "LEAN"));
    c = Call{}; c.frames.bytes = 0;                              CHECK(refuses(c, "bytes == 0"));
    c = Call{}; c.frames.desc_format = 2;                        CHECK(refuses(c, "desc_format"));
    c = Call{}; c.frames.base = nullptr;                         CHECK(refuses(c, "null packet buffer"));
    c = Call{}; c.frames.desc = nullptr; c.frames.stride = 0;    CHECK(refuses(c, "stride"));
    c = Call{}; c.no_frames = true;                              CHECK(refuses(c, "null", 5));   // a message cut to its block

    FlowtabArgs a;
    c = Call{};
    CHECK(run(c, &a, nullptr) && a.n == 2 && a.ntiles == 1 && a.nchunks == 1 && a.slots == 128 && !a.l3_only && !a.bidir &&
          a.flow_cap == 0 && a.result == &g_result && !a.flow_id && !a.flows && a.desc == g_desc && a.desc_words == 1);
    CHECK((void*)a.tab == (void*)g_scratch && (uint8_t*)a.keys == g_scratch + 128 * 4 && (uint8_t*)a.pslot == (uint8_t*)a.keys + 256 &&
          (uint8_t*)a.firstw == (uint8_t*)a.pslot + 256 && (uint8_t*)a.parts == (uint8_t*)a.firstw + 256);
    CHECK(a.bytes % 16 == 0 && a.bytes <= sizeof(g_frames) + 15);
    c.opts.flags = BT_FLOWTAB_L3_ONLY | BT_FLOWTAB_BIDIRECTIONAL; c.opts.slots = 256; c.opts.flow_cap = 7;
    c.out.flows = reinterpret_cast<bt_flow_rec*>(g_scratch + 32768); c.out.flow_id = reinterpret_cast<uint32_t*>(g_scratch + 49152);
    CHECK(run(c, &a, nullptr) && a.l3_only == 1 && a.bidir == 1 && a.slots == 256 && a.flow_cap == 7 && a.flows && a.flow_id);
    c = Call{}; c.frames.n = 0; c.scratch = nullptr; c.scratch_bytes = 0;
    CHECK(run(c, &a, nullptr) && a.n == 0 && a.nchunks == 0 && a.slots == 128);   // an empty batch needs no scratch
    c = Call{}; c.frames.desc_format = BT_DESC_XDP;
    CHECK(run(c, &a, nullptr) && a.desc_words == 2);
    // the layout: regions in order, 256-byte aligned, growing with n and with slots
    const uint32_t ns[] = {0u, 1u, 64u, 65u, 16384u, 16385u, 1u << 24, 0xFFFFFFFFu};
    uint64_t prev = 0;
    for (uint32_t n : ns) {
        const FtLayout l = ft_layout(n, 128), m = ft_layout(n, 256);
        CHECK(l.slots == 0 && l.keys >= 128u * 4u && l.pslot - l.keys >= (uint64_t)n * sizeof(FtFlow) &&
              l.firstw - l.pslot >= (uint64_t)n * 4u && l.parts - l.firstw >= ((uint64_t)n + 63u) / 64u * 8u && l.total >= l.parts);
        CHECK(l.keys % 256 == 0 && l.pslot % 256 == 0 && l.firstw % 256 == 0 && l.parts % 256 == 0 && l.total % 256 == 0);
        CHECK(l.total >= prev && m.total > l.total);
        prev = l.total;
    }
    CHECK(ft_auto_slots(0) == 128 && ft_auto_slots(64) == 128 && ft_auto_slots(65) == 256 && ft_auto_slots(1u << 30) == 1u << 31 &&
          ft_auto_slots((1u << 30) + 1u) == 0);

    // conversations in both directions
    Batch b;
    b.add(v4_frame(1, 2, 4000, 80));          // 0: A < B
    b.add(v4_frame(2, 1, 80, 4000));          // 1: the reverse
    b.add(v4_frame(1, 2, 4000, 80, 17));      // 2: UDP with the same tuple: the same key (the protocol is not in it)
    b.add(v6_frame(9, 3, 53, 53));            // 3: A > B
    b.add(v6_frame(3, 9, 53, 53));            // 4
    b.add(v4_frame(5, 5, 7, 7));              // 5: equal endpoints
    b.add(v4_frame(5, 5, 8, 7));              // 6: A > B by the port
    b.add(v4_frame(5, 5, 7, 8));              // 7
    b.add(v4_frame(2, 1, 0, 0, 1));           // 8: ICMP: addresses only
    b.add(std::vector<uint8_t>(10, 0));       // 9: no key
    Result r = table(b, BT_FLOWTAB_BIDIRECTIONAL);
    const uint32_t want_bi[] = {0, 0, 0, 1, 1, 2, 3, 3, 4, BT_FLOW_ID_NONE};
    CHECK(r.r.n == 10 && r.r.n_selected == 10 && r.r.n_flows == 5 && r.r.n_written == 5 && r.r.none_packets == 1 &&
          r.r.overflow_packets == 0 && r.r.slots == 128 && r.r.none_bytes == 10 && std::memcmp(r.id.data(), want_bi, sizeof(want_bi)) == 0);
    CHECK(r.flows[0].packets[0] == 2 && r.flows[0].packets[1] == 1 && r.flows[0].first == 0 && r.flows[0].last == 2 &&
          r.flows[0].klass == BT_FLOW_V4_L4 && r.flows[0].key[3] == 1 && r.flows[0].key[7] == 2 && r.flows[0].key[8] == (4000 >> 8) &&
          r.flows[0].bytes[0] == 54 + 42 && r.flows[0].bytes[1] == 54);
    CHECK(r.flows[1].packets[0] == 1 && r.flows[1].packets[1] == 1 && r.flows[1].first == 3 && r.flows[1].key[15] == 3 &&
          r.flows[1].key[31] == 9 && r.flows[1].klass == BT_FLOW_V6_L4);
    CHECK(r.flows[2].packets[0] == 1 && r.flows[2].packets[1] == 0);
    CHECK(r.flows[3].packets[0] == 1 && r.flows[3].packets[1] == 1 && r.flows[3].key[9] == 7 && r.flows[3].key[11] == 8);
    CHECK(r.flows[4].klass == BT_FLOW_V4 && r.flows[4].key[3] == 1 && r.flows[4].packets[1] == 1 && r.flows[4].key[8] == 0);
    CHECK(r.r.klass_flows[BT_FLOW_V4_L4] == 3 && r.r.klass_flows[BT_FLOW_V6_L4] == 1 && r.r.klass_flows[BT_FLOW_V4] == 1 &&
          r.r.klass_flows[BT_FLOW_NONE] == 0 && r.r.keyed_bytes + r.r.none_bytes + 10 == b.data.size());
    for (const bt_flow_rec& f : r.flows) CHECK(f.reserved == 0 && f.pad[0] == 0 && f.pad[1] == 0 && f.pad[2] == 0);
    r = table(b, 0);
    const uint32_t want_uni[] = {0, 1, 0, 2, 3, 4, 5, 6, 7, BT_FLOW_ID_NONE};
    CHECK(r.r.n_flows == 8 && std::memcmp(r.id.data(), want_uni, sizeof(want_uni)) == 0);
    for (const bt_flow_rec& f : r.flows) CHECK(f.packets[1] == 0 && f.bytes[1] == 0);
    r = table(b, BT_FLOWTAB_L3_ONLY | BT_FLOWTAB_BIDIRECTIONAL);
    CHECK(r.r.n_flows == 3 && r.flows[0].packets[0] == 2 && r.flows[0].packets[1] == 2 && r.flows[0].last == 8 &&
          r.flows[2].packets[0] == 3 && r.r.klass_flows[BT_FLOW_V4] == 2 && r.r.klass_flows[BT_FLOW_V6] == 1);
    // select, with bits above n set, and a flow_cap below the flows
    const uint64_t sel = ~0ull << 3;
    r = table(b, 0, 128, &sel, ~0ull, 2);
    CHECK(r.r.n_selected == 7 && r.id[0] == BT_FLOW_ID_UNSELECTED && r.id[2] == BT_FLOW_ID_UNSELECTED && r.id[3] == 0 &&
          r.r.n_flows == 6 && r.r.n_written == 2 && r.flows.size() == 2 && r.flows[1].first == 4);
    // the fragments of a datagram share one address-only flow
    Batch fr;
    fr.add(v4_frame(1, 2, 5000, 6000, 17, 0x2000));
    fr.add(v4_frame(1, 2, 0x1234, 0x5678, 17, 0x2002));
    fr.add(v4_frame(1, 2, 0x9999, 0x1111, 17, 0x0004));
    fr.add(v4_frame(1, 2, 5000, 6000, 17));
    r = table(fr, 0);
    CHECK(r.r.n_flows == 2 && r.id[0] == 0 && r.id[1] == 0 && r.id[2] == 0 && r.id[3] == 1 && r.flows[0].klass == BT_FLOW_V4 &&
          r.flows[0].packets[0] == 3 && r.flows[1].klass == BT_FLOW_V4_L4);
    // a full table succeeds, one flow more overflows
    Batch full;
    for (uint16_t k = 0; k < 129; ++k) full.add(v4_frame(1, 2, (uint16_t)(1000 + k), 80));
    full.add(v4_frame(1, 2, 1000, 80));
    r = table(full, 0, 128, nullptr, ~0ull, 200);
    CHECK(r.r.n_flows == 128 && r.r.overflow_packets == 1 && r.id[128] == BT_FLOW_ID_OVERFLOW && r.id[129] == 0 && r.flows[0].packets[0] == 2);
    r = table(full, 0, 256, nullptr, ~0ull, 200);
    CHECK(r.r.n_flows == 129 && r.r.overflow_packets == 0 && r.id[128] == 128);
    // `bytes` at every offset of the last three frames: nothing past it is read, what is missing reads as zero
    const uint64_t from = BT_DESC_OFF(b.desc[7]);
    for (uint64_t bytes = from; bytes <= b.data.size(); ++bytes) {
        r = table(b, BT_FLOWTAB_BIDIRECTIONAL, 128, nullptr, bytes);
        CHECK(r.r.n_selected == 10 && r.id[6] == 3);
        if (bytes < from + 13) CHECK(r.id[7] == BT_FLOW_ID_NONE && r.id[8] == BT_FLOW_ID_NONE);
    }
    r = table(b, 0, 128, nullptr, from + 34);   // frame 7 up to its addresses: ports read as zeros, a TCP key of ports 0, 0
    CHECK(r.flows[r.id[7]].klass == BT_FLOW_V4_L4 && r.flows[r.id[7]].key[9] == 0 && r.flows[r.id[7]].key[11] == 0 && r.id[8] == BT_FLOW_ID_NONE);
    r = table(b, 0, 128, nullptr, 0);
    CHECK(r.r.none_packets == 10 && r.r.n_flows == 0);
    // an empty batch
    Batch none;
    r = table(none, 0);
    CHECK(r.r.n == 0 && r.r.n_flows == 0 && r.r.slots == 128);
    if (g_bad) {
        std::printf("%d checks FAILED\n", g_bad);
        return 1;
    }
    std::printf("flowtab_host_check: all cases hold\n");
    return 0;
}
