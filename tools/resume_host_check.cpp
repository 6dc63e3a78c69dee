// resume_host_check.cpp — the host-only pieces of the two-pass PAYLOAD path under the host
// sanitizers: bt_filter_resume_device's argument checks (bt::resume_args_error) and the scan of
// decision bytes that builds the ring stage's verdict words, n_pass and n_host (bt::decide_scan),
// both from beatrice_amd/csrc/bt_resume_host.h. No device, no Python, no library to load:
//
//   g++ -std=c++17 -O1 -g -fsanitize=address,undefined -fno-sanitize-recover=all -Iinclude -Ibeatrice_amd/csrc
//       tools/resume_host_check.cpp -o tools/resume_host_check && tools/resume_host_check   (one command line)
//
// The checks never look inside the context (it only has to be non-null), so a stand-in pointer
// serves. The decision arrays are heap blocks of exactly n bytes and the word arrays of exactly
// ceil(n / 64) words, so a read or write past either is an AddressSanitizer report. Exit 0 = all
// cases hold.
#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <vector>

#include "bt_resume_host.h"

static int g_bad = 0;
#define CHECK(x) do { if (!(x)) { std::printf("FAILED line %d: %s\n", __LINE__, #x); ++g_bad; } } while (0)

static bool refuses(const bt_ctx* c, const bt_batch* b, const bt_outputs* o, const char* word) {
    const char* why = bt::resume_args_error(c, b, o);
    return why && std::strstr(why, word);
}

static void check_args() {
    alignas(16) static unsigned char stand_in[16];
    const bt_ctx* ctx = reinterpret_cast<const bt_ctx*>(stand_in);
    unsigned char frames[256] = {};
    unsigned long long desc[2] = {};
    unsigned char decide[2] = {};
    bt_batch b{};
    b.base = frames; b.desc = desc; b.n = 2; b.bytes = sizeof(frames);
    bt_outputs o{};
    o.decide = decide;
    CHECK(bt::resume_args_error(ctx, &b, &o) == nullptr);
    CHECK(refuses(nullptr, &b, &o, "null argument"));
    CHECK(refuses(ctx, nullptr, &o, "null argument"));
    CHECK(refuses(ctx, &b, nullptr, "null argument"));
    bt_batch p = b; p.flags = BT_BATCH_PREFIXES;
    CHECK(refuses(ctx, &p, &o, "BT_BATCH_PREFIXES"));
    p.flags = BT_BATCH_LEAN;
    CHECK(refuses(ctx, &p, &o, "BT_BATCH_PREFIXES"));
    bt_outputs r = o; r.records = frames;
    CHECK(refuses(ctx, &b, &r, "records"));
    bt_outputs d = o; d.decide = nullptr;
    CHECK(refuses(ctx, &b, &d, "decide == NULL"));
    bt_batch z = b; z.bytes = 0;
    CHECK(refuses(ctx, &z, &o, "bytes == 0"));
    bt_batch f = b; f.desc = nullptr; f.stride = 0;
    CHECK(refuses(ctx, &f, &o, "stride"));
    f.stride = 128; f.bytes = 0;                       // fixed stride: bytes defaults to n * stride
    CHECK(bt::resume_args_error(ctx, &f, &o) == nullptr);
    f.bytes = 255;
    CHECK(refuses(ctx, &f, &o, "n * stride"));
    bt_batch nb = b; nb.base = nullptr;
    CHECK(refuses(ctx, &nb, &o, "null packet buffer"));
    nb.n = 0;                                          // an empty batch needs no buffer
    CHECK(bt::resume_args_error(ctx, &nb, &o) == nullptr);
    bt_batch x = b; x.desc_format = 7;
    CHECK(refuses(ctx, &x, &o, "desc_format"));
}

static void check_scan(uint32_t n) {
    // exact-size heap blocks (n = 0: one byte / word that must stay untouched)
    std::vector<unsigned char> dec(n ? n : 1, 0xFF);
    const uint32_t words = (n + 63u) / 64u;
    std::vector<uint64_t> ver(words ? words : 1, 0xA5A5A5A5A5A5A5A5ull);
    uint64_t want_pass = 0, want_host = 0;
    for (uint32_t i = 0; i < n; ++i) {
        const uint32_t code = (i * 7u + i / 3u) & 3u, slot = (i * 5u) & 63u;
        dec[i] = (unsigned char)((code << 6) | slot);
        want_pass += code == BT_DECIDE_PASS;
        want_host += code == BT_DECIDE_HOST;
    }
    // whole range at once, then split as the ring stage's workers split it, then without words
    for (uint32_t parts : {1u, 2u, 3u, 16u}) {
        std::fill(ver.begin(), ver.end(), 0xA5A5A5A5A5A5A5A5ull);
        uint64_t pass = 0, host = 0;
        for (uint32_t w = 0; w < parts; ++w)
            bt::decide_scan(n ? dec.data() : nullptr, n, (uint32_t)((uint64_t)words * w / parts),
                            (uint32_t)((uint64_t)words * (w + 1) / parts), ver.data(), &pass, &host);
        CHECK(pass == want_pass && host == want_host);
        for (uint32_t i = 0; i < n; ++i)
            CHECK(((ver[i / 64] >> (i % 64)) & 1ull) == (uint64_t)((dec[i] >> 6) == BT_DECIDE_PASS));
        if (n % 64u) CHECK((ver[words - 1] >> (n % 64u)) == 0ull);   // bits past n stay clear
        if (!n) CHECK(ver[0] == 0xA5A5A5A5A5A5A5A5ull);
    }
    uint64_t pass = 0, host = 0;
    bt::decide_scan(n ? dec.data() : nullptr, n, 0, words, nullptr, &pass, &host);
    CHECK(pass == want_pass && host == want_host);
}

int main() {
    check_args();
    for (uint32_t n : {0u, 1u, 63u, 64u, 65u, 4133u}) check_scan(n);
    std::printf(g_bad ? "%d checks FAILED\n" : "resume_host_check: all checks hold\n", g_bad);
    return g_bad ? 1 : 0;
}
