// flowtop_host_check.cpp — the top-K query's host part from beatrice_amd/csrc/bt_flowtop.h under the
// host sanitizers: the argument checks of bt_flow_track_top_device / _host (every refusal, and an
// accepted call with the launch arguments it resolves to), the scratch layout, and the query on the
// host (bt::flowtop_host) over crafted states against a plain selection written here: equal values,
// ties at the threshold, values that differ in the lowest or the highest byte only, sums that wrap,
// durations that run backwards, the TCP metrics, k = 0 and k above n_flows. Every output is a heap
// block of exactly n_top entries (an access past it is an AddressSanitizer report). No device, no
// Python, no library to load:
//
//   g++ -std=c++17 -O1 -g -fsanitize=address,undefined -fno-sanitize-recover=all -Iinclude -Ibeatrice_amd/csrc
//       tools/flowtop_host_check.cpp -o tools/flowtop_host_check && tools/flowtop_host_check   (one command line)
//
// Exit 0 = all cases hold.
#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <vector>

#include "bt_flowtop.h"

using namespace bt;
static int g_bad = 0;
#define CHECK(x) do { if (!(x)) { std::printf("FAILED line %d: %s\n", __LINE__, #x); ++g_bad; } } while (0)

alignas(256) static unsigned char g_state[1 << 16];
alignas(256) static unsigned char g_scratch[1 << 17];
alignas(8) static unsigned char g_out[1 << 12];
static bt_flow_tcp_rec g_tcp[100];
static bt_flow_top_result g_result;
static const FkShadow g_shadow{BT_FLOWTAB_BIDIRECTIONAL, 100u, 256u};

struct Call {   // a device call with nothing wrong
    const FkShadow* sh = &g_shadow;
    const void* state = g_state;
    bt_flow_top_opts opts{BT_FLOW_TOP_BYTES, 20u, {0u, 0u}};
    const bt_flow_tcp_rec* tcp = nullptr;
    void* scratch = g_scratch;
    uint64_t scratch_bytes = sizeof(g_scratch);
    bt_flow_top_out out{nullptr, nullptr, nullptr, nullptr, &g_result};
    bool no_opts = false, no_out = false;
};

static bool run(const Call& c, FlowtopArgs* a, const char* word) {
    char why[160];
    if (flowtop_args(c.sh, c.state, c.no_opts ? nullptr : &c.opts, c.tcp, c.scratch, c.scratch_bytes, c.no_out ? nullptr : &c.out, a, why,
                     sizeof(why)))
        return word == nullptr;
    return word && std::strstr(why, word);
}

static bool refuses(const Call& c, const char* word) {
    FlowtopArgs a;
    return run(c, &a, word);
}

static void check_refusals() {
    Call c;
    FlowtopArgs a;
    CHECK(run(c, &a, nullptr));
    const FtopLayout l = ftop_scratch(100u, 20u);
    CHECK(a.hdr == reinterpret_cast<const bt_flow_track_hdr*>(g_state) && (const unsigned char*)a.recs == g_state + 256);
    CHECK(a.flow_cap == 100u && a.slots == 256u && a.flags == BT_FLOWTAB_BIDIRECTIONAL && a.metric == BT_FLOW_TOP_BYTES && a.k == 20u);
    CHECK((unsigned char*)a.ctl == g_scratch + l.ctl && (unsigned char*)a.hist == g_scratch + l.hist &&
          (unsigned char*)a.value == g_scratch + l.value && (unsigned char*)a.parts == g_scratch + l.parts &&
          (unsigned char*)a.cand_value == g_scratch + l.cand_value && (unsigned char*)a.cand_id == g_scratch + l.cand_id);
    CHECK(a.result == &g_result && !a.top && !a.top_id && !a.top_value && !a.top_tcp && !a.tcp);
    { Call d; d.state = nullptr; CHECK(refuses(d, "null state")); }
    { Call d; d.no_opts = true; CHECK(refuses(d, "null opts")); }
    { Call d; d.no_out = true; CHECK(refuses(d, "null out")); }
    { Call d; d.out.result = nullptr; CHECK(refuses(d, "null result")); }
    { Call d; d.scratch = nullptr; CHECK(refuses(d, "null scratch")); }
    { Call d; d.state = g_state + 128; CHECK(refuses(d, "state is not 256-byte aligned")); }
    { Call d; d.scratch = g_scratch + 64; CHECK(refuses(d, "scratch is not 256-byte aligned")); }
    { Call d; d.out.result = reinterpret_cast<bt_flow_top_result*>(g_out + 4); CHECK(refuses(d, "result is not 8-byte aligned")); }
    { Call d; d.out.top_value = reinterpret_cast<uint64_t*>(g_out + 4); CHECK(refuses(d, "top_value is not 8-byte aligned")); }
    { Call d; d.out.top = reinterpret_cast<bt_flow_track_rec*>(g_out + 4); CHECK(refuses(d, "top is not 8-byte aligned")); }
    { Call d; d.out.top_id = reinterpret_cast<uint32_t*>(g_out + 2); CHECK(refuses(d, "top_id is not 4-byte aligned")); }
    { Call d; d.tcp = reinterpret_cast<const bt_flow_tcp_rec*>(g_out + 1); CHECK(refuses(d, "tcp is not 4-byte aligned")); }
    { Call d; d.tcp = g_tcp; d.out.top_tcp = reinterpret_cast<bt_flow_tcp_rec*>(g_out + 2); CHECK(refuses(d, "top_tcp is not 4-byte aligned")); }
    { Call d; d.opts.k = BT_FLOW_TOP_MAX_K + 1u; CHECK(refuses(d, "k above")); }
    { Call d; d.opts.k = BT_FLOW_TOP_MAX_K; CHECK(refuses(d, nullptr)); }
    { Call d; d.opts.k = 0u; CHECK(refuses(d, nullptr)); }
    { Call d; d.opts.metric = 5u; CHECK(refuses(d, "unknown metric")); }
    { Call d; d.opts.reserved[0] = 1u; CHECK(refuses(d, "reserved")); }
    { Call d; d.opts.reserved[1] = 1u; CHECK(refuses(d, "reserved")); }
    { Call d; d.opts.metric = BT_FLOW_TOP_TCP_SYN; CHECK(refuses(d, "TCP metric")); }
    { Call d; d.opts.metric = BT_FLOW_TOP_TCP_RST; CHECK(refuses(d, "TCP metric")); }
    { Call d; d.opts.metric = BT_FLOW_TOP_TCP_RST; d.tcp = g_tcp; CHECK(refuses(d, nullptr)); }
    { Call d; d.out.top_tcp = reinterpret_cast<bt_flow_tcp_rec*>(g_out); CHECK(refuses(d, "top_tcp without")); }
    { Call d; d.sh = nullptr; CHECK(refuses(d, "not an initialised tracker")); }
    { Call d; d.sh = nullptr; d.opts.k = 5000u; CHECK(refuses(d, "k above")); }   // the unknown state is reported last
    { Call d; d.scratch_bytes = l.total - 1u; CHECK(refuses(d, "scratch_bytes")); }
    { Call d; d.scratch_bytes = l.total; CHECK(refuses(d, nullptr)); }
}

static void check_layout() {
    const uint32_t caps[] = {1u, 255u, 256u, 257u, 5000u, 1u << 24, 0xFFFFFFFBu};
    const uint32_t ks[] = {0u, 1u, 20u, 4096u};
    for (uint32_t cap : caps)
        for (uint32_t k : ks) {
            const FtopLayout l = ftop_scratch(cap, k);
            const uint64_t parts = ((uint64_t)cap + 255u) / 256u;
            CHECK(l.ctl == 0 && l.hist >= sizeof(FtopCtl) && l.value - l.hist >= 8u * 256u * 4u && l.parts - l.value >= 8ull * cap);
            CHECK(l.cand_value - l.parts >= parts * sizeof(FtopPart) && l.cand_id - l.cand_value >= 8ull * k && l.total - l.cand_id >= 4ull * k);
            const uint64_t offs[] = {l.hist, l.value, l.parts, l.cand_value, l.cand_id, l.total};
            for (uint64_t o : offs) CHECK(o % 256u == 0);
        }
}

struct HostState {   // a tracker state in a heap block of exactly its size, 256-byte aligned
    void* raw = nullptr;
    bt_flow_track_sizes lay{};
    FkHostState hs{};
    HostState(uint32_t cap, uint32_t n_flows) {
        char why[128];
        if (!fk_layout(cap, 0, &lay, why, sizeof(why)) || posix_memalign(&raw, 256, lay.total)) std::abort();
        const bt_flow_track_opts o{0u, cap, 0u, 0u};
        fk_init_host(raw, o, lay);
        if (!fk_host_state(raw, lay.total, &hs, why, sizeof(why))) std::abort();
        hs.hdr->n_flows = n_flows;
    }
    ~HostState() { free(raw); }
};

static uint64_t g_rng = 0x9E3779B97F4A7C15ull;
static uint64_t rnd() { g_rng ^= g_rng << 13; g_rng ^= g_rng >> 7; g_rng ^= g_rng << 17; return g_rng; }

// One query through flowtop_host_args + flowtop_host into exact-size outputs, against a selection by
// repeated maximum written here.
static void check_query(const HostState& s, uint32_t metric, uint32_t k, const std::vector<bt_flow_tcp_rec>* tcp) {
    const uint32_t nf = s.hs.hdr->n_flows, n_top = k < nf ? k : nf;
    std::vector<uint64_t> v(nf);
    for (uint32_t f = 0; f < nf; ++f) {
        const bt_flow_track_rec& r = s.hs.recs[f];
        v[f] = metric == BT_FLOW_TOP_BYTES ? r.bytes[0] + r.bytes[1] : metric == BT_FLOW_TOP_PACKETS ? r.packets[0] + r.packets[1]
             : metric == BT_FLOW_TOP_DURATION ? (r.last_ts >= r.first_ts ? r.last_ts - r.first_ts : 0ull)
             : metric == BT_FLOW_TOP_TCP_SYN ? (*tcp)[f].syn_packets : (*tcp)[f].rst_packets;
    }
    std::vector<uint32_t> want;
    std::vector<bool> taken(nf, false);
    for (uint32_t r = 0; r < n_top; ++r) {
        uint32_t best = nf;
        for (uint32_t f = 0; f < nf; ++f)
            if (!taken[f] && (best == nf || v[f] > v[best])) best = f;   // the first of the largest: the lowest flow number
        taken[best] = true;
        want.push_back(best);
    }
    // exact-size outputs (new[] of zero entries is a valid, unreadable block)
    uint32_t* ids = new uint32_t[n_top];
    uint64_t* vals = new uint64_t[n_top];
    bt_flow_track_rec* recs = new bt_flow_track_rec[n_top];
    bt_flow_tcp_rec* side = tcp ? new bt_flow_tcp_rec[n_top] : nullptr;
    bt_flow_top_result res;
    memset(&res, 0xC7, sizeof(res));
    const bt_flow_top_opts o{metric, k, {0u, 0u}};
    const bt_flow_top_out out{ids, vals, recs, side, &res};
    char why[160];
    FkHostState hs{};
    const bool ok = flowtop_host_args(s.raw, s.lay.total, &o, tcp ? tcp->data() : nullptr, &out, &hs, why, sizeof(why));
    CHECK(ok);
    if (ok) {
        flowtop_host(hs, o, tcp ? tcp->data() : nullptr, out);
        uint64_t total = 0, top_total = 0;
        uint32_t ties = 0;
        for (uint32_t f = 0; f < nf; ++f) total += v[f];
        for (uint32_t r = 0; r < n_top; ++r) {
            CHECK(ids[r] == want[r] && vals[r] == v[want[r]] && memcmp(&recs[r], &s.hs.recs[want[r]], sizeof(bt_flow_track_rec)) == 0);
            if (side) CHECK(memcmp(&side[r], &(*tcp)[want[r]], sizeof(bt_flow_tcp_rec)) == 0);
            top_total += v[want[r]];
        }
        const uint64_t thr = n_top ? v[want[n_top - 1u]] : 0ull;
        for (uint32_t f = 0; f < nf && n_top; ++f) ties += v[f] == thr ? 1u : 0u;
        CHECK(res.n_flows == nf && res.n_top == n_top && res.status == 0u && res.metric == metric && res.n_ties == ties &&
              res.reserved == 0u && res.threshold == thr && res.total == total && res.top_total == top_total);
    }
    delete[] ids; delete[] vals; delete[] recs; delete[] side;
}

static void check_host_form() {
    const uint32_t sizes[][2] = {{1u, 0u}, {1u, 1u}, {70u, 65u}, {300u, 257u}, {1100u, 1025u}};
    for (const auto& sz : sizes) {
        const uint32_t cap = sz[0], nf = sz[1];
        for (int pattern = 0; pattern < 6; ++pattern) {
            HostState s(cap, nf);
            std::vector<bt_flow_tcp_rec> tcp(cap);
            for (uint32_t f = 0; f < cap; ++f) {
                bt_flow_track_rec& r = s.hs.recs[f];
                const bool live = f < nf;
                const uint64_t x = rnd();
                r.key[0] = (uint8_t)f; r.key[1] = (uint8_t)(f >> 8);
                if (!live) {   // garbage behind the live flows: it must not be selected
                    r.bytes[0] = r.packets[0] = ~0ull - f; r.last_ts = ~0ull;
                    tcp[f].syn_packets = tcp[f].rst_packets = 0xFFFFFFF0u;
                    continue;
                }
                switch (pattern) {
                case 0: r.bytes[0] = 1000u; r.packets[1] = 7u; break;                                  // all equal
                case 1: r.bytes[0] = f % 97u == 3u ? 9000u : 50u; r.packets[0] = f % 5u; break;      // two values, many ties
                case 2: r.bytes[0] = 0x0102030405060700ull + f * 37u % 256u; r.packets[0] = x & 255u; break;   // the lowest byte
                case 3: r.bytes[1] = (uint64_t)(f * 73u % 256u) << 56 | 5u; r.packets[0] = x >> 56 << 56; break;   // the highest byte
                case 4: r.bytes[0] = ~0ull - f % 7u; r.bytes[1] = 3u * f + 10u; r.packets[0] = ~0ull; r.packets[1] = x & 3u; break;   // wraps
                default: r.bytes[0] = x; r.packets[0] = rnd() >> 1; r.packets[1] = rnd() >> 1; break;   // full width
                }
                r.first_ts = rnd() % 1000u; r.last_ts = rnd() % 1000u;   // about half of them run backwards
                tcp[f].flags[0] = (uint8_t)x; tcp[f].syn_packets = (uint32_t)(rnd() % 4u); tcp[f].rst_packets = (uint32_t)rnd();
            }
            const uint32_t ks[] = {0u, 1u, 2u, nf ? nf - 1u : 0u, nf, nf + 1u, 4096u, 20u};
            for (uint32_t k : ks) {
                if (k > BT_FLOW_TOP_MAX_K) continue;
                for (uint32_t metric = 0; metric < kTopMetrics; ++metric) check_query(s, metric, k, &tcp);
                check_query(s, BT_FLOW_TOP_BYTES, k, nullptr);
            }
        }
    }
    // the host form's own refusals
    HostState s(64u, 3u);
    bt_flow_top_result res{};
    const bt_flow_top_opts o{BT_FLOW_TOP_BYTES, 2u, {0u, 0u}};
    const bt_flow_top_out out{nullptr, nullptr, nullptr, nullptr, &res};
    char why[160];
    FkHostState hs{};
    CHECK(flowtop_host_args(s.raw, s.lay.total, &o, nullptr, &out, &hs, why, sizeof(why)));
    CHECK(!flowtop_host_args(nullptr, s.lay.total, &o, nullptr, &out, &hs, why, sizeof(why)) && strstr(why, "null state"));
    CHECK(!flowtop_host_args(s.raw, s.lay.total - 1u, &o, nullptr, &out, &hs, why, sizeof(why)) && strstr(why, "state_bytes below"));
    CHECK(!flowtop_host_args(s.raw, 64u, &o, nullptr, &out, &hs, why, sizeof(why)) && strstr(why, "not an initialised tracker"));
    CHECK(!flowtop_host_args(s.raw, s.lay.total, nullptr, nullptr, &out, &hs, why, sizeof(why)) && strstr(why, "null opts"));
    CHECK(!flowtop_host_args(s.raw, s.lay.total, &o, nullptr, nullptr, &hs, why, sizeof(why)) && strstr(why, "null out"));
    const bt_flow_top_opts syn{BT_FLOW_TOP_TCP_SYN, 2u, {0u, 0u}};
    CHECK(!flowtop_host_args(s.raw, s.lay.total, &syn, nullptr, &out, &hs, why, sizeof(why)) && strstr(why, "TCP metric"));
    s.hs.hdr->magic ^= 1u;
    CHECK(!flowtop_host_args(s.raw, s.lay.total, &o, nullptr, &out, &hs, why, sizeof(why)) && strstr(why, "not an initialised tracker"));
    s.hs.hdr->magic ^= 1u;
    s.hs.hdr->n_flows = 65u;   // above flow_cap
    CHECK(!flowtop_host_args(s.raw, s.lay.total, &o, nullptr, &out, &hs, why, sizeof(why)) && strstr(why, "not an initialised tracker"));
}

int main() {
    check_refusals();
    check_layout();
    check_host_form();
    if (g_bad) { std::printf("%d checks FAILED\n", g_bad); return 1; }
    std::printf("flowtop_host_check: all cases hold\n");
    return 0;
}
