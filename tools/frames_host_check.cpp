// frames_host_check.cpp — the one set of checks on a bt_batch (bt::frame_src, from
// beatrice_amd/csrc/bt_frames.h) under the host sanitizers: every refusal, and accepted batches of
// all three forms with what they resolve to. No device, no Python, no library to load:
//
//   g++ -std=c++17 -O1 -g -fsanitize=address,undefined -fno-sanitize-recover=all -Iinclude -Ibeatrice_amd/csrc
//       tools/frames_host_check.cpp -o tools/frames_host_check && tools/frames_host_check   (one command line)
//
// frame_src reads the batch struct and never the buffers it names, so small stand-ins serve. The
// message goes to a heap block of exactly the stated size: a write past it is an AddressSanitizer
// report. Exit 0 = all cases hold.
#include <cstdio>
#include <cstring>
#include <vector>

#include "bt_frames.h"

using namespace bt;
static int g_bad = 0;
#define CHECK(x) do { if (!(x)) { std::printf("FAILED line %d: %s\n", __LINE__, #x); ++g_bad; } } while (0)

static unsigned char g_frames[256];
static unsigned long long g_desc[4];

// The batch is refused as `kind` with `word` in the (terminated) message, and *f stays untouched.
static bool refuses(const bt_batch* b, FrameCheck kind, const char* word, size_t cap = 96) {
    std::vector<char> why(cap, '?');
    FrameSrc f, before;
    std::memset(&f, 0x5A, sizeof(f));
    std::memcpy(&before, &f, sizeof(f));
    return frame_src(b, &f, why.data(), cap) == kind && std::strlen(why.data()) < cap &&
           std::strstr(why.data(), word) && !std::memcmp(&f, &before, sizeof(f));
}

static void check_refusals() {
    bt_batch d{}, f{}, x;   // a good descriptor batch, a good fixed-stride batch
    d.base = g_frames; d.desc = g_desc; d.n = 2; d.bytes = sizeof(g_frames);
    f.base = g_frames; f.stride = 128; f.n = 2;
    CHECK(refuses(nullptr, kFramesUnusable, "null batch"));
    x = d; x.base = nullptr;            CHECK(refuses(&x, kFramesUnusable, "null packet buffer"));
    x = f; x.base = nullptr;            CHECK(refuses(&x, kFramesUnusable, "null packet buffer"));
    x = f; x.stride = 0;                CHECK(refuses(&x, kFramesUnusable, "fixed-stride mode needs stride > 0"));
    x = d; x.desc_format = 2;           CHECK(refuses(&x, kFramesFormat, "desc_format 2"));
    x = d; x.bytes = 0;                 CHECK(refuses(&x, kFramesSize, "bytes == 0 (the readable size of base)"));
    CHECK(refuses(&x, kFramesSize, "descri", 7));   // a message longer than the buffer is cut
    x.n = 0;                            CHECK(refuses(&x, kFramesSize, "bytes == 0"));   // ... an empty one too
    x = f; x.bytes = 255;               CHECK(refuses(&x, kFramesSize, "bytes 255 < n * stride 256"));
    x.n = x.stride = 0xFFFFFFFFu; x.bytes = 0xFFFFFFFE00000000ull;   // the product in 64 bits
    CHECK(refuses(&x, kFramesSize, "bytes 18446744065119617024 < n * stride 18446744065119617025"));
    x = d; x.base = nullptr; x.bytes = 0;   // wrong in two ways: the first check in that order speaks
    CHECK(refuses(&x, kFramesUnusable, "null packet buffer"));
}

static void check_accepted(uint32_t n) {
    char why[96];
    for (uint32_t form = 0; form < 4; ++form) {   // packed, xdp_desc, fixed stride with bytes 0 (= n * stride) / stated
        bt_batch b{};
        b.base = g_frames; b.n = n; b.stride = 256;
        if (form < 2) { b.desc = g_desc; b.desc_format = form; b.bytes = 4096; }
        else b.bytes = form == 3 ? 256ull * n + 5 : 0;
        FrameSrc f{};
        CHECK(frame_src(&b, &f, why, sizeof(why)) == kFramesOk);
        CHECK(f.base == g_frames && (const void*)f.desc == b.desc && f.stride == 256 && f.n == n);
        CHECK(f.desc_words == (form == 1 ? 2u : 1u) && f.ntiles == (uint32_t)((n + 63ull) / 64));
        CHECK(f.bytes == (form < 2 ? 4096 : 256ull * n + (form == 3 ? 5 : 0)));
    }
}

int main() {
    check_refusals();
    bt_batch z{};   // an empty fixed-stride batch needs no buffer and no stride
    FrameSrc f{};
    char why[8];
    CHECK(frame_src(&z, &f, why, sizeof(why)) == kFramesOk && !f.ntiles && !f.bytes && f.desc_words == 1);
    for (uint32_t n : {0u, 1u, 63u, 64u, 65u, 0xFFFFFFFFu}) check_accepted(n);   // the last: ntiles in 64 bits
    std::printf(g_bad ? "%d checks FAILED\n" : "frames_host_check: all checks hold\n", g_bad);
    return g_bad ? 1 : 0;
}
