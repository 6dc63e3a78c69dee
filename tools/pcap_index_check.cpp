// pcap_index_check.cpp — bt_pcap_index (beatrice_amd/csrc/bt_pcap.cpp) under the host sanitizers,
// over whole, truncated and malformed files. No device, no Python, no library to load: the
// indexer alone is compiled in (BT_PCAP_HOST_ONLY leaves bt_pcap_filter and HIP out):
//
//   g++ -std=c++17 -O1 -g -fsanitize=address,undefined -fno-sanitize-recover=all -DBT_PCAP_HOST_ONLY -Iinclude
//       -Ibeatrice_amd/csrc tools/pcap_index_check.cpp beatrice_amd/csrc/bt_pcap.cpp -o tools/pcap_index_check
//       && tools/pcap_index_check                                                   (one command line)
//
// Every file is a heap block of exactly its size and every descriptor array of exactly `cap`
// entries, so a read past a cut tail or a write past the array is an AddressSanitizer report.
// Every prefix of a small capture (each possible cut) is indexed in all four magics. Exit 0 =
// all cases hold.
#include <cstdint>
#include <cstdio>
#include <cstring>
#include <memory>
#include <vector>

#include "beatrice_gpu.h"

static int g_bad = 0;
#define CHECK(x) do { if (!(x)) { std::printf("FAILED line %d: %s\n", __LINE__, #x); ++g_bad; } } while (0)

static void put32(std::vector<uint8_t>& v, uint32_t x, bool big) {
    for (int i = 0; i < 4; ++i) v.push_back((uint8_t)(x >> (big ? 24 - 8 * i : 8 * i)));
}

static std::vector<uint8_t> header(bool nsec, bool big, uint32_t linktype = 1) {
    std::vector<uint8_t> v;
    put32(v, nsec ? 0xa1b23c4du : 0xa1b2c3d4u, big);
    put32(v, big ? 0x00020004u : 0x00040002u, big);   // version 2.4 as two 16-bit fields
    put32(v, 0, big); put32(v, 0, big); put32(v, 65535, big); put32(v, linktype, big);
    return v;
}

static void record(std::vector<uint8_t>& v, uint32_t incl, bool big, uint32_t stored) {
    put32(v, 1700000000u, big); put32(v, 5, big); put32(v, incl, big); put32(v, incl + 3, big);
    for (uint32_t i = 0; i < stored; ++i) v.push_back((uint8_t)(i * 7 + incl));
}

// bt_pcap_index over an exact-size heap copy of f[0, bytes), into an exact-size descriptor array.
static int index_of(const std::vector<uint8_t>& f, size_t bytes, bt_pcap_info* info, std::vector<bt_pkt_desc>* desc,
                    uint64_t cap, uint64_t* n) {
    std::unique_ptr<uint8_t[]> copy(new uint8_t[bytes ? bytes : 1]);
    std::memcpy(copy.get(), f.data(), bytes);
    std::unique_ptr<bt_pkt_desc[]> d(new bt_pkt_desc[cap ? cap : 1]);
    const int rc = bt_pcap_index(copy.get(), bytes, info, desc ? d.get() : nullptr, cap, n);
    if (desc) desc->assign(d.get(), d.get() + (rc == BT_OK && *n < cap ? *n : cap));
    return rc;
}

int main() {
    const uint32_t lens[] = {60, 0, 1, 1514, 61, 65535, 64};
    for (int magic = 0; magic < 4; ++magic) {
        const bool nsec = magic & 1, big = magic & 2;
        std::vector<uint8_t> f = header(nsec, big);
        std::vector<uint64_t> start;   // each record's header offset
        for (uint32_t ln : lens) { start.push_back(f.size()); record(f, ln, big, ln); }
        start.push_back(f.size());
        // every cut of the file from 0 bytes to all of it (the big record: only near its edges)
        for (size_t cut = 0; cut <= f.size(); ++cut) {
            if (cut > start[5] + 40 && cut + 40 < start[6]) continue;
            bt_pcap_info info;
            uint64_t n = 99;
            std::vector<bt_pkt_desc> desc;
            const int rc = index_of(f, cut, &info, &desc, 7, &n);
            if (cut < 24) { CHECK(rc == BT_E_INVALID_ARGUMENT && n == 0); continue; }
            CHECK(rc == BT_OK);
            uint64_t whole = 0;
            while (whole < 7 && start[whole + 1] <= cut) ++whole;
            CHECK(n == whole && info.end == start[whole]);
            CHECK(info.truncated == (cut != start[whole] ? 1u : 0u));
            CHECK(info.swapped == (big ? 1u : 0u) && info.nanosecond == (nsec ? 1u : 0u));
            CHECK(info.magic == (nsec ? 0xa1b23c4du : 0xa1b2c3d4u) && info.snaplen == 65535 && info.linktype == 1);
            for (uint64_t i = 0; i < whole; ++i) CHECK(desc[i] == BT_DESC(start[i] + 16, lens[i]));
            // count only, and a descriptor array shorter than the file
            uint64_t n2 = 0;
            CHECK(index_of(f, cut, &info, nullptr, 0, &n2) == BT_OK && n2 == whole);
            CHECK(index_of(f, cut, &info, &desc, 2, &n2) == BT_OK && n2 == whole);
        }
        // incl_len 65536: refused, whether or not the data is there; a length far past the file
        for (uint32_t stored : {0u, 65536u}) {
            std::vector<uint8_t> g = header(nsec, big);
            record(g, 10, big, 10);
            record(g, 65536, big, stored);
            bt_pcap_info info;
            uint64_t n = 0;
            CHECK(index_of(g, g.size(), &info, nullptr, 0, &n) == BT_E_INVALID_ARGUMENT);
        }
        std::vector<uint8_t> far = header(nsec, big);
        record(far, 0xFFFFFFFFu, big, 5);
        bt_pcap_info info;
        uint64_t n = 0;
        CHECK(index_of(far, far.size(), &info, nullptr, 0, &n) == BT_E_INVALID_ARGUMENT);
        // other link types, pcapng, an unknown magic
        std::vector<uint8_t> l113 = header(nsec, big, 113);
        record(l113, 20, big, 20);
        CHECK(index_of(l113, l113.size(), &info, nullptr, 0, &n) == BT_E_NOT_IMPLEMENTED && info.linktype == 113);
    }
    bt_pcap_info info;
    uint64_t n = 0;
    std::vector<uint8_t> ng = {0x0a, 0x0d, 0x0d, 0x0a, 28, 0, 0, 0, 0x4d, 0x3c, 0x2b, 0x1a};
    CHECK(index_of(ng, ng.size(), &info, nullptr, 0, &n) == BT_E_NOT_IMPLEMENTED);
    CHECK(index_of(ng, 4, &info, nullptr, 0, &n) == BT_E_NOT_IMPLEMENTED);
    std::vector<uint8_t> junk(64, 0x5a);
    CHECK(index_of(junk, junk.size(), &info, nullptr, 0, &n) == BT_E_INVALID_ARGUMENT);
    CHECK(bt_pcap_index(nullptr, 24, &info, nullptr, 0, &n) == BT_E_INVALID_ARGUMENT);
    CHECK(bt_pcap_index(junk.data(), 24, nullptr, nullptr, 0, &n) == BT_E_INVALID_ARGUMENT);
    CHECK(bt_pcap_index(junk.data(), 24, &info, nullptr, 0, nullptr) == BT_E_INVALID_ARGUMENT);
    std::printf(g_bad ? "pcap_index_check: %d checks FAILED\n" : "pcap_index_check: ok\n", g_bad);
    return g_bad ? 1 : 0;
}
