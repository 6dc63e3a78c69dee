// fanout_host_check.cpp — the argument checks of bt_flow_fanout_device (bt::fanout_args) and the
// host flow hash that bt_flow_hash_host wraps (bt::flow_key_host, bt::toeplitz_host), from
// beatrice_amd/csrc/bt_fanout.h, under the host sanitizers: every refusal, accepted calls with the
// launch arguments they resolve to, the published RSS verification vectors, and frames cut at
// every length, each in a heap block of exactly its size (a read past it is an AddressSanitizer
// report). No device, no Python, no library to load:
//
//   g++ -std=c++17 -O1 -g -fsanitize=address,undefined -fno-sanitize-recover=all -Iinclude -Ibeatrice_amd/csrc
//       tools/fanout_host_check.cpp -o tools/fanout_host_check && tools/fanout_host_check   (one command line)
//
// Exit 0 = all cases hold.
#include <cstdio>
#include <cstring>
#include <vector>

#include "bt_fanout.h"

using namespace bt;
static int g_bad = 0;
#define CHECK(x) do { if (!(x)) { std::printf("FAILED line %d: %s\n", __LINE__, #x); ++g_bad; } } while (0)

static unsigned char g_frames[256];
static uint64_t g_desc[4];
static bt_fanout_result g_result;

struct Call {
    bt_batch frames{};
    bt_fanout_opts opts{};
    bt_fanout_out out{};
    bool no_frames = false, no_opts = false, no_out = false;   // pass a null pointer instead
    Call() {
        frames.base = g_frames; frames.desc = g_desc; frames.n = 2; frames.bytes = sizeof(g_frames);
        opts.queues = 8;
        out.result = &g_result;
    }
};

static bool run(const Call& c, FanoutArgs* a, const char* word, size_t cap = 96) {
    std::vector<char> why(cap, '?');
    const bool ok = fanout_args(c.no_frames ? nullptr : &c.frames, nullptr, c.no_opts ? nullptr : &c.opts, c.no_out ? nullptr : &c.out, a, why.data(), cap);
    if (ok) return word == nullptr;
    return word && std::strlen(why.data()) < cap && std::strstr(why.data(), word);
}

static bool refuses(const Call& c, const char* word, size_t cap = 96) {
    FanoutArgs a;
    return run(c, &a, word, cap);
}

// Ethernet (+ tags) + IPv4 (ihl words) + TCP/UDP, the tuple of the first published vector.
static std::vector<uint8_t> v4_frame(int tags, int ihl, int proto, uint16_t frag = 0) {
    std::vector<uint8_t> f(12, 0);
    for (int k = 0; k < tags; ++k) { f.push_back(k == 0 && tags == 2 ? 0x88 : 0x81); f.push_back(k == 0 && tags == 2 ? 0xA8 : 0x00); f.push_back(0); f.push_back(5); }
    f.push_back(0x08); f.push_back(0x00);
    const size_t o3 = f.size();
    f.resize(o3 + 4 * ihl, 0);
    f[o3] = (uint8_t)(0x40 | ihl); f[o3 + 6] = (uint8_t)(frag >> 8); f[o3 + 7] = (uint8_t)frag; f[o3 + 9] = (uint8_t)proto;
    const uint8_t addr[8] = {66, 9, 149, 187, 161, 142, 100, 80};
    memcpy(&f[o3 + 12], addr, 8);
    const uint8_t ports[4] = {2794 >> 8, 2794 & 255, 1766 >> 8, 1766 & 255};
    f.insert(f.end(), ports, ports + 4);
    f.resize(f.size() + 16, 0);
    return f;
}

static std::vector<uint8_t> v6_frame(int nh) {
    std::vector<uint8_t> f(12, 0);
    f.push_back(0x86); f.push_back(0xDD);
    const size_t o3 = f.size();
    f.resize(o3 + 40, 0);
    f[o3] = 0x60; f[o3 + 6] = (uint8_t)nh;
    const uint8_t src[16] = {0x3f, 0xfe, 0x25, 0x01, 0x02, 0x00, 0x1f, 0xff, 0, 0, 0, 0, 0, 0, 0, 7};
    const uint8_t dst[16] = {0x3f, 0xfe, 0x25, 0x01, 0x02, 0x00, 0x00, 0x03, 0, 0, 0, 0, 0, 0, 0, 1};
    memcpy(&f[o3 + 8], src, 16);
    memcpy(&f[o3 + 24], dst, 16);
    const uint8_t ports[4] = {2794 >> 8, 2794 & 255, 1766 >> 8, 1766 & 255};
    f.insert(f.end(), ports, ports + 4);
    f.resize(f.size() + 16, 0);
    return f;
}

// The hash and class of the first `len` bytes of f, held in a heap block of exactly len bytes.
static uint32_t hash_of(const std::vector<uint8_t>& f, size_t len, bool l3_only, uint32_t* klass, const uint8_t* key) {
    std::vector<uint8_t> exact(f.begin(), f.begin() + len);
    uint8_t in[kFanInputMax];
    const uint32_t nb = flow_key_host(exact.data(), (uint32_t)len, l3_only, in, klass);
    return toeplitz_host(key, in, nb);
}

int main() {
    Call c;
    c = Call{}; c.no_frames = true;                                  CHECK(refuses(c, "null frames"));
    c = Call{}; c.no_opts = true;                                  CHECK(refuses(c, "null opts"));
    c = Call{}; c.no_out = true;                                CHECK(refuses(c, "null out"));
    c = Call{}; c.out.result = nullptr;                          CHECK(refuses(c, "null result"));
    c = Call{}; c.out.result = reinterpret_cast<bt_fanout_result*>(reinterpret_cast<char*>(&g_result) + 4);
    CHECK(refuses(c, "aligned"));
    c = Call{}; c.frames.flags = BT_BATCH_PREFIXES;              CHECK(refuses(c, "PREFIXES"));
    c = Call{}; c.frames.flags = BT_BATCH_PREFIXES | BT_BATCH_LEAN; CHECK(refuses(c, "LEAN"));
    c = Call{}; c.opts.queues = 0;                               CHECK(refuses(c, "queues"));
    c = Call{}; c.opts.queues = 65;                              CHECK(refuses(c, "queues"));
    c = Call{}; c.opts.flags = BT_FANOUT_KEY_USER | BT_FANOUT_KEY_SYMMETRIC; CHECK(refuses(c, "both key flags"));
    c = Call{}; c.opts.flags = 0x10;                             CHECK(refuses(c, "flag"));
    c = Call{}; c.opts.flags = 0x80000000u;                      CHECK(refuses(c, "flag"));
    c = Call{}; c.opts.flags = BT_FANOUT_RETA_USER; c.opts.reta[127] = 8; CHECK(refuses(c, "reta"));
    c = Call{}; c.frames.bytes = 0;                              CHECK(refuses(c, "bytes == 0"));
    c = Call{}; c.frames.desc_format = 2;                        CHECK(refuses(c, "desc_format"));
    c = Call{}; c.frames.base = nullptr;                         CHECK(refuses(c, "null packet buffer"));
    c = Call{}; c.frames.desc = nullptr; c.frames.stride = 0;    CHECK(refuses(c, "stride"));
    c = Call{}; c.no_frames = true;                                  CHECK(refuses(c, "null", 5));   // a message cut to its block

    FanoutArgs a;
    c = Call{};
    CHECK(run(c, &a, nullptr) && a.n == 2 && a.ntiles == 1 && a.nchunks == 1 && a.queues == 8 && !a.l3_only &&
          a.key[0] == 0x6d5a56dau && a.key[9] == 0xbeac01fau && a.reta[0] == 0x03020100u && a.reta[31] == 0x07060504u &&
          a.result == &g_result && !a.hash && !a.queue && !a.idx && !a.select_q && a.desc == g_desc && a.desc_words == 1);
    CHECK(a.bytes % 16 == 0 && a.bytes <= sizeof(g_frames) + 15 &&
          ((uintptr_t)g_frames + a.bytes) <= (((uintptr_t)g_frames + sizeof(g_frames) + 15) & ~(uintptr_t)15));
    c.opts.flags = BT_FANOUT_KEY_SYMMETRIC | BT_FANOUT_L3_ONLY | BT_FANOUT_RETA_USER;
    memset(c.opts.reta, 7, 128);
    CHECK(run(c, &a, nullptr) && a.l3_only == 1 && a.key[0] == 0x6d5a6d5au && a.key[9] == 0x6d5a6d5au && a.reta[5] == 0x07070707u);
    c = Call{}; c.opts.flags = BT_FANOUT_KEY_USER; c.opts.queues = 64;
    for (int i = 0; i < 40; ++i) c.opts.key[i] = (uint8_t)i;
    CHECK(run(c, &a, nullptr) && a.key[0] == 0x00010203u && a.key[9] == 0x24252627u && a.queues == 64 && a.reta[16] == 0x03020100u);
    c = Call{}; c.frames.desc_format = BT_DESC_XDP;
    CHECK(run(c, &a, nullptr) && a.desc_words == 2);
    c = Call{}; c.frames.desc = nullptr; c.frames.stride = 128; c.frames.bytes = 0;
    CHECK(run(c, &a, nullptr) && a.stride == 128 && !a.desc && a.bytes % 16 == 0 && a.bytes >= 240 && a.bytes <= 256);
    const uint32_t ns[] = {0u, 1u, 64u, 65u, 16384u, 16385u, 0xFFFFFFFFu};
    const uint32_t tiles[] = {0u, 1u, 1u, 2u, 256u, 257u, 0x4000000u}, chunks[] = {0u, 1u, 1u, 1u, 1u, 2u, 0x40000u};
    for (int k = 0; k < 7; ++k) {
        c = Call{}; c.frames.n = ns[k];
        CHECK(run(c, &a, nullptr) && a.ntiles == tiles[k] && a.nchunks == chunks[k]);
    }
    // fan_read_end: a multiple of 16 from base, inside the granules of [base, base + bytes)
    for (uintptr_t base = 0x1000; base < 0x1010; ++base)
        for (uint64_t bytes = 0; bytes < 70; ++bytes) {
            const uint64_t v = fan_read_end(reinterpret_cast<const void*>(base), bytes);
            CHECK(v % 16 == 0 && base + v <= ((base + bytes + 15) & ~(uintptr_t)15) && (bytes == 0 ? v == 0 : v + 16 > bytes));
        }

    // the published vectors, with tags and IP options in front of them
    uint8_t key[kFanKeyBytes], sym[kFanKeyBytes];
    fan_default_key(key);
    fan_symmetric_key(sym);
    uint32_t k = 0;
    for (int tags = 0; tags <= 2; ++tags)
        for (int ihl = 5; ihl <= 15; ihl += 5) {
            const std::vector<uint8_t> f = v4_frame(tags, ihl, 6);
            CHECK(hash_of(f, f.size(), false, &k, key) == 0x51ccc178u && k == BT_FLOW_V4_L4);
            CHECK(hash_of(f, f.size(), true, &k, key) == 0x323e8fc2u && k == BT_FLOW_V4);
            CHECK(hash_of(f, f.size() - 1, false, &k, key) == 0x323e8fc2u && k == BT_FLOW_V4);   // TCP one byte short
            const std::vector<uint8_t> u = v4_frame(tags, ihl, 17);
            CHECK(hash_of(u, u.size() - 12, false, &k, key) == 0x51ccc178u && k == BT_FLOW_V4_L4);   // UDP needs 8
            CHECK(hash_of(u, u.size() - 13, false, &k, key) == 0x323e8fc2u && k == BT_FLOW_V4);
            const std::vector<uint8_t> g = v4_frame(tags, ihl, 6, 0x2000), o = v4_frame(tags, ihl, 6, 0x0010);
            CHECK(hash_of(g, g.size(), false, &k, key) == 0x323e8fc2u && k == BT_FLOW_V4);       // MF
            CHECK(hash_of(o, o.size(), false, &k, key) == 0x323e8fc2u && k == BT_FLOW_V4);       // an offset
            const std::vector<uint8_t> df = v4_frame(tags, ihl, 6, 0x4000), ic = v4_frame(tags, ihl, 1);
            CHECK(hash_of(df, df.size(), false, &k, key) == 0x51ccc178u && k == BT_FLOW_V4_L4);  // DF alone
            CHECK(hash_of(ic, ic.size(), false, &k, key) == 0x323e8fc2u && k == BT_FLOW_V4);     // ICMP: no ports
            for (size_t len = 0; len <= f.size(); ++len) (void)hash_of(f, len, false, &k, key);  // every cut
        }
    const std::vector<uint8_t> s6 = v6_frame(6);
    CHECK(hash_of(s6, s6.size(), false, &k, key) == 0x40207d3du && k == BT_FLOW_V6_L4);
    CHECK(hash_of(s6, s6.size(), true, &k, key) == 0x2cc18cd5u && k == BT_FLOW_V6);
    CHECK(hash_of(s6, s6.size() - 1, false, &k, key) == 0x2cc18cd5u && k == BT_FLOW_V6);
    CHECK(hash_of(s6, 53, false, &k, key) == 0u && k == BT_FLOW_NONE);
    for (size_t len = 0; len <= s6.size(); ++len) (void)hash_of(s6, len, false, &k, key);
    const std::vector<uint8_t> h6 = v6_frame(0);   // hop-by-hop: no extension-header walk
    CHECK(hash_of(h6, h6.size(), false, &k, key) == 0x2cc18cd5u && k == BT_FLOW_V6);
    // the symmetric key: the reversed tuple hashes alike
    std::vector<uint8_t> r = v4_frame(0, 5, 6);
    const std::vector<uint8_t> fwd = r;
    for (int i = 0; i < 4; ++i) { std::swap(r[26 + i], r[30 + i]); }
    std::swap(r[34], r[36]); std::swap(r[35], r[37]);
    CHECK(hash_of(r, r.size(), false, &k, sym) == hash_of(fwd, fwd.size(), false, &k, sym));
    CHECK(hash_of(r, r.size(), false, &k, key) != hash_of(fwd, fwd.size(), false, &k, key));
    if (g_bad) {
        std::printf("%d checks FAILED\n", g_bad);
        return 1;
    }
    std::printf("fanout_host_check: all cases hold\n");
    return 0;
}
