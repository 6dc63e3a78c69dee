// test_device_stats.cpp — GpuPacketFilter::classifyDevice against the reference's statistics.
//
// Links the reference's own PacketFilter objects (oracle/_ref/obj) next to GpuPacketFilter.cpp,
// compiled into the program (beatrice_amd/host/Makefile), over libbeatrice_gpu.so. For one capture (u64 n, n x u64 desc, u64 bytes, data: what the
// Python test writes from a golden) and five filter sets it builds the reference PacketFilter,
// called as applyFilters(vector<Packet>) inside try/catch, and a GpuPacketFilter, called as
// classifyDevice over device copies of the same frames: getStats() (packetsProcessed / Passed /
// Dropped and the whole filterCounts map) and the exception's type and what() must agree, after
// one call, after a second one (the stats accumulate) and after resetStats. A program with a
// CUSTOM callback is refused. Prints one line per check and ALL OK; exit status 0 = all passed.
//   test_device_stats <capture.bin> <label>
#include <cstdio>
#include <cstring>
#include <functional>
#include <memory>
#include <stdexcept>
#include <string>
#include <vector>

#include "beatrice/PacketFilter.hpp"
#include "beatrice_gpu_bench.h"
#include "../../beatrice_amd/host/GpuPacketFilter.hpp"

using beatrice::Packet;
using beatrice::PacketFilter;
using beatrice::gpu::GpuPacketFilter;

static int g_fail = 0;
#define CHECK(cond, ...)                                                  \
    do {                                                                  \
        if (!(cond)) {                                                    \
            ++g_fail;                                                     \
            std::printf("FAIL %s:%d: ", __FILE__, __LINE__);              \
            std::printf(__VA_ARGS__);                                     \
            std::printf("\n");                                            \
            return false;                                                 \
        }                                                                 \
    } while (0)

struct Capture {
    std::vector<uint8_t> data;
    std::vector<uint64_t> desc;
    std::vector<Packet> packets;
    uint64_t bytes = 0;
};

static Capture load_capture(const char* path) {
    Capture c;
    FILE* f = std::fopen(path, "rb");
    if (!f) return c;
    uint64_t n = 0;
    if (std::fread(&n, 8, 1, f) == 1) {
        c.desc.resize(n);
        if (std::fread(c.desc.data(), 8, n, f) == n && std::fread(&c.bytes, 8, 1, f) == 1) {
            c.data.resize(c.bytes + 64);
            if (std::fread(c.data.data(), 1, c.bytes, f) != c.bytes) c.desc.clear();
        }
    }
    std::fclose(f);
    for (uint64_t d : c.desc) {
        const uint8_t* fr = c.data.data() + (d & 0xFFFFFFFFFFFFull);
        c.packets.emplace_back(std::shared_ptr<const uint8_t[]>(fr, [](const uint8_t*) {}), (size_t)(d >> 48));
    }
    return c;
}

struct Spec {
    PacketFilter::FilterType type;
    const char* expr;
    int priority;
    bool enabled;
};
using FT = PacketFilter::FilterType;

template <class F>
static void install(F& f, const std::vector<Spec>& specs) {
    int k = 0;
    for (const auto& s : specs) {
        PacketFilter::FilterConfig c;
        c.type = s.type;
        c.expression = s.expr;
        c.priority = s.priority;
        c.enabled = s.enabled;
        f.addFilter("f" + std::to_string(k++), c);
    }
}

static std::string what_kind(const std::exception_ptr& e) {
    if (!e) return "none";
    try {
        std::rethrow_exception(e);
    } catch (const std::invalid_argument& x) {
        return std::string("invalid_argument:") + x.what();
    } catch (const std::out_of_range& x) {
        return std::string("out_of_range:") + x.what();
    } catch (const std::exception& x) {
        return std::string("exception:") + x.what();
    }
}

// The capture on the device of `ctx`, with the outputs of a filter call.
struct DeviceBatch {
    bt_ctx* ctx;
    void *data = nullptr, *desc = nullptr, *decide = nullptr, *records = nullptr;
    bt_batch batch{};
    bt_outputs out{};
    bool ok = false;
    DeviceBatch(bt_ctx* c, const Capture& cap) : ctx(c) {
        const uint32_t n = (uint32_t)cap.desc.size();
        ok = bt_dev_malloc(ctx, cap.bytes + 256, &data) == BT_OK && bt_dev_malloc(ctx, 8ull * n + 16, &desc) == BT_OK &&
             bt_dev_malloc(ctx, n + 16, &decide) == BT_OK &&
             bt_dev_malloc(ctx, (uint64_t)(n + 63) / 64 * 6144 + 16, &records) == BT_OK &&
             bt_memcpy_h2d(ctx, data, cap.data.data(), cap.bytes) == BT_OK &&
             bt_memcpy_h2d(ctx, desc, cap.desc.data(), 8ull * n) == BT_OK;
        batch.base = static_cast<const uint8_t*>(data);
        batch.desc = desc;
        batch.n = n;
        batch.bytes = cap.bytes;
        out.decide = static_cast<uint8_t*>(decide);
        out.records = records;
        out.n_cap = n;
    }
    ~DeviceBatch() {
        for (void* p : {data, desc, decide, records})
            if (p) bt_dev_free(ctx, p);
    }
};

static bool same_stats(const char* label, const char* when, const PacketFilter::FilterStats& a,
                       const PacketFilter::FilterStats& b) {
    CHECK(a.packetsProcessed == b.packetsProcessed && a.packetsPassed == b.packetsPassed &&
              a.packetsDropped == b.packetsDropped,
          "%s %s: processed/passed/dropped ref %llu/%llu/%llu gpu %llu/%llu/%llu", label, when,
          (unsigned long long)a.packetsProcessed, (unsigned long long)a.packetsPassed,
          (unsigned long long)a.packetsDropped, (unsigned long long)b.packetsProcessed,
          (unsigned long long)b.packetsPassed, (unsigned long long)b.packetsDropped);
    CHECK(a.filterCounts == b.filterCounts, "%s %s: filterCounts differ (%zu against %zu names)", label, when,
          a.filterCounts.size(), b.filterCounts.size());
    return true;
}

static bool one_set(const char* cap_label, const char* set, const Capture& cap, const std::vector<Spec>& specs) {
    const std::string label = std::string(cap_label) + "/" + set;
    PacketFilter ref;
    GpuPacketFilter gf(0);
    install(ref, specs);
    install(gf, specs);
    DeviceBatch dev(gf.context(), cap);
    CHECK(dev.ok, "%s: device copies: %s", label.c_str(), bt_last_error());
    PacketFilter::FilterStats first;
    for (int call = 0; call < 3; ++call) {   // 0: fresh; 1: accumulates; 2: after resetStats
        if (call == 2) {
            ref.resetStats();
            gf.resetStats();
        }
        std::exception_ptr ea, eb;
        try { (void)ref.applyFilters(cap.packets); } catch (...) { ea = std::current_exception(); }
        GpuPacketFilter::DeviceCounts dc;
        const uint64_t before = gf.getStats().packetsProcessed;
        try { dc = gf.classifyDevice(dev.batch, dev.out); } catch (...) { eb = std::current_exception(); }
        const std::string when = "call " + std::to_string(call);
        CHECK(what_kind(ea) == what_kind(eb), "%s %s: exception ref '%s' gpu '%s'", label.c_str(), when.c_str(),
              what_kind(ea).c_str(), what_kind(eb).c_str());
        const auto sa = ref.getStats(), sb = gf.getStats();
        if (!same_stats(label.c_str(), when.c_str(), sa, sb)) return false;
        if (!eb) {
            CHECK(dc.counted == sb.packetsProcessed - before && dc.counted == cap.packets.size() &&
                      dc.tally.n == cap.packets.size() && dc.passed == dc.tally.code[BT_DECIDE_PASS],
                  "%s %s: DeviceCounts counted %llu passed %llu", label.c_str(), when.c_str(),
                  (unsigned long long)dc.counted, (unsigned long long)dc.passed);
            CHECK(gf.lastBatchTiming().device_s > 0, "%s %s: lastBatchTiming not set", label.c_str(), when.c_str());
        }
        if (call == 0) first = sb;
        if (call == 1)
            CHECK(sb.packetsProcessed == 2 * first.packetsProcessed && sb.packetsPassed == 2 * first.packetsPassed,
                  "%s: the second call did not accumulate", label.c_str());
        if (call == 2 && !same_stats(label.c_str(), "reset against fresh", first, sb)) return false;
    }
    std::printf("ok %s: processed %llu passed %llu dropped %llu, %zu names\n", label.c_str(),
                (unsigned long long)first.packetsProcessed, (unsigned long long)first.packetsPassed,
                (unsigned long long)first.packetsDropped, first.filterCounts.size());
    return true;
}

static bool custom_refused(const char* cap_label, const Capture& cap) {
    GpuPacketFilter gf(0);
    install(gf, {{FT::PROTOCOL, "udp", 3, true}, {FT::CUSTOM, "", 1, true}});
    DeviceBatch dev(gf.context(), cap);
    CHECK(dev.ok, "%s: device copies: %s", cap_label, bt_last_error());
    // without a callback a CUSTOM filter passes everything on the device: taken
    std::exception_ptr e;
    try { (void)gf.classifyDevice(dev.batch, dev.out); } catch (...) { e = std::current_exception(); }
    CHECK(!e, "%s: CUSTOM without a callback refused: %s", cap_label, what_kind(e).c_str());
    gf.setCustomFilter("f1", [](const Packet& p) { return p.length() % 3 != 0; });
    const auto before = gf.getStats();
    try { (void)gf.classifyDevice(dev.batch, dev.out); } catch (...) { e = std::current_exception(); }
    CHECK(what_kind(e).rfind("invalid_argument:", 0) == 0, "%s: CUSTOM callback: got '%s'", cap_label, what_kind(e).c_str());
    if (!same_stats(cap_label, "custom refused", before, gf.getStats())) return false;
    bt_outputs no_decide = dev.out;
    no_decide.decide = nullptr;
    gf.removeFilter("f1");
    e = nullptr;
    try { (void)gf.classifyDevice(dev.batch, no_decide); } catch (...) { e = std::current_exception(); }
    CHECK(what_kind(e).rfind("invalid_argument:", 0) == 0, "%s: decide == NULL: got '%s'", cap_label, what_kind(e).c_str());
    std::printf("ok %s: CUSTOM callback and missing decide refused\n", cap_label);
    return true;
}

int main(int argc, char** argv) {
    if (argc < 3) {
        std::fprintf(stderr, "usage: %s <capture.bin> <label>\n", argv[0]);
        return 2;
    }
    const Capture cap = load_capture(argv[1]);
    if (cap.desc.empty()) {
        std::fprintf(stderr, "cannot read %s\n", argv[1]);
        return 2;
    }
    const std::vector<std::pair<const char*, std::vector<Spec>>> sets = {
        {"c3", {{FT::PROTOCOL, "udp", 3, true}, {FT::IP_RANGE, "10.0.0.0/8", 2, true}, {FT::PORT_RANGE, "1000-2000", 1, true}}},
        {"mixed", {{FT::PORT_RANGE, "0-1023", -1, true}, {FT::BPF, "tcp udp", 10, true},
                   {FT::IP_RANGE, "192.168.0.0/16", 4, false}, {FT::IP_RANGE, "192.168.0.0/17", 4, true},
                   {FT::PROTOCOL, "ip", 7, true}}},
        {"empty", {}},
        {"throw_after", {{FT::PROTOCOL, "tcp", 5, true}, {FT::PORT_RANGE, "1000-", 1, true}}},
        {"throw_oor", {{FT::BPF, "udp", 2, true}, {FT::IP_RANGE, "10.0.0.0/99999999999", 1, true}}},
    };
    for (const auto& s : sets) one_set(argv[2], s.first, cap, s.second);
    custom_refused(argv[2], cap);
    if (g_fail) {
        std::printf("%d FAILED\n", g_fail);
        return 1;
    }
    std::printf("ALL OK\n");
    return 0;
}
