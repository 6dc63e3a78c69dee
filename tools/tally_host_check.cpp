// tally_host_check.cpp — the argument checks of bt_tally_device (bt::tally_args, from
// beatrice_amd/csrc/bt_tally.h) under the host sanitizers: every refusal, and accepted calls with
// the launch arguments they resolve to. No device, no Python, no library to load:
//
//   g++ -std=c++17 -O1 -g -fsanitize=address,undefined -fno-sanitize-recover=all -Iinclude -Ibeatrice_amd/csrc
//       tools/tally_host_check.cpp -o tools/tally_host_check && tools/tally_host_check   (one command line)
//
// tally_args reads the batch struct and never the buffers it names, so small stand-ins serve. The
// message goes to a heap block of exactly the stated size: a write past it is an AddressSanitizer
// report. Exit 0 = all cases hold.
#include <cstdio>
#include <cstring>
#include <vector>

#include "bt_tally.h"

using namespace bt;
static int g_bad = 0;
#define CHECK(x) do { if (!(x)) { std::printf("FAILED line %d: %s\n", __LINE__, #x); ++g_bad; } } while (0)

static unsigned char g_frames[256], g_decide[64], g_records[6144];
static uint64_t g_desc[4];
static bt_tally g_out;

struct Call {
    const uint8_t* decide = g_decide;
    uint32_t n = 2;
    const bt_batch* frames = nullptr;
    const void* records = nullptr;
    uint32_t n_cap = 0, flags = 0;
    bt_tally* out = &g_out;
    uint32_t opt = 0;
};

static bool run(const Call& c, TallyArgs* a, const char* word, size_t cap = 96) {
    std::vector<char> why(cap, '?');
    const bool ok = tally_args(c.decide, c.n, c.frames, c.records, c.n_cap, c.flags, c.out, c.opt, a, why.data(), cap);
    if (ok) return word == nullptr;
    return word && std::strlen(why.data()) < cap && std::strstr(why.data(), word);
}

static bool refuses(const Call& c, const char* word, size_t cap = 96) {
    TallyArgs a;
    return run(c, &a, word, cap);
}

int main() {
    bt_batch d{}, f{};   // a good descriptor batch, a good fixed-stride batch
    d.base = g_frames; d.desc = g_desc; d.n = 2; d.bytes = sizeof(g_frames);
    f.base = g_frames; f.stride = 128; f.n = 2;
    Call c;
    c = Call{}; c.out = nullptr;                               CHECK(refuses(c, "null out"));
    c = Call{}; c.out = reinterpret_cast<bt_tally*>(reinterpret_cast<char*>(&g_out) + 4);
    CHECK(refuses(c, "aligned"));
    c = Call{}; c.decide = nullptr;                            CHECK(refuses(c, "both null"));
    c = Call{}; c.flags = 0x4;                                 CHECK(refuses(c, "flag"));
    c = Call{}; c.flags = 0x80000001u;                         CHECK(refuses(c, "flag"));
    c = Call{}; c.records = g_records; c.n_cap = 1;            CHECK(refuses(c, "n_cap"));
    c = Call{}; c.frames = &d; c.n = 3;                        CHECK(refuses(c, "frames->n"));
    bt_batch x = d; x.bytes = 0;
    c = Call{}; c.frames = &x;                                 CHECK(refuses(c, "bytes == 0"));
    x = d; x.desc_format = 2;
    c = Call{}; c.frames = &x;                                 CHECK(refuses(c, "desc_format"));
    x = d; x.base = nullptr;
    c = Call{}; c.frames = &x;                                 CHECK(refuses(c, "null packet buffer"));
    x = f; x.stride = 0;
    c = Call{}; c.frames = &x;                                 CHECK(refuses(c, "stride"));
    c = Call{}; c.out = nullptr;                               CHECK(refuses(c, "null", 5));   // a message cut to its block

    TallyArgs a;
    c = Call{};
    CHECK(run(c, &a, nullptr) && a.n == 2 && a.ntiles == 1 && a.nchunks == 1 && a.decide == g_decide && !a.lengths &&
          a.rec_layout == kTallyRecNone && a.out == &g_out && !a.desc && !a.stride);
    c.frames = &d; c.records = g_records; c.n_cap = 2; c.flags = BT_TALLY_STOP_AT_THROW | BT_TALLY_ACCUMULATE;
    CHECK(run(c, &a, nullptr) && a.lengths == 1 && a.desc == g_desc && a.desc_words == 1 && a.rec_layout == kTallyRecTiled &&
          a.flags == 3u && a.n_cap == 2);
    c.opt = BT_OPT_RECORDS_PLANES;
    CHECK(run(c, &a, nullptr) && a.rec_layout == kTallyRecPlanes);
    c.opt = BT_OPT_RECORDS_AOS | BT_OPT_RECORDS_PLANES;
    CHECK(run(c, &a, nullptr) && a.rec_layout == kTallyRecAoS);
    x = d; x.desc_format = BT_DESC_XDP;
    c = Call{}; c.frames = &x;
    CHECK(run(c, &a, nullptr) && a.desc_words == 2 && a.lengths == 1);
    c = Call{}; c.frames = &f;
    CHECK(run(c, &a, nullptr) && a.stride == 128 && !a.desc && a.lengths == 1);
    c = Call{}; c.decide = nullptr; c.records = g_records; c.n_cap = 2; c.frames = &d;   // lengths need decisions
    CHECK(run(c, &a, nullptr) && !a.lengths && a.rec_layout == kTallyRecTiled);
    // sizes: the tile and chunk counts at their edges, up to the largest n
    const uint32_t ns[] = {0u, 1u, 64u, 65u, 16384u, 16385u, 0xFFFFFFFFu};
    const uint32_t tiles[] = {0u, 1u, 1u, 2u, 256u, 257u, 0x4000000u}, chunks[] = {0u, 1u, 1u, 1u, 1u, 2u, 0x40000u};
    for (int k = 0; k < 7; ++k) {
        c = Call{}; c.n = ns[k];
        CHECK(run(c, &a, nullptr) && a.ntiles == tiles[k] && a.nchunks == chunks[k]);
    }
    if (g_bad) {
        std::printf("%d checks FAILED\n", g_bad);
        return 1;
    }
    std::printf("tally_host_check: all cases hold\n");
    return 0;
}
