// flowtrack_host_check.cpp — the flow tracker's host part from beatrice_amd/csrc/bt_flowtrack.h
// under the host sanitizers: the state layout (bt::fk_layout) and the scratch layouts, the argument
// checks of the three device calls (bt::flowtrack_init_args, bt::flowtrack_update_args,
// bt::flowtrack_expire_args: every refusal, and accepted calls with the launch arguments they
// resolve to), and the tracker on the host (bt::fk_init_host, bt::fk_update_host,
// bt::fk_expire_host) over crafted batches: flows that recur, overflow at the exact boundary, a
// table loaded to 1.0, expiry at its boundaries with truncation, remap and re-appearance. Every
// state is a heap block of exactly the layout's size (an access past it is an AddressSanitizer
// report). No device, no Python, no library to load:
//
//   g++ -std=c++17 -O1 -g -fsanitize=address,undefined -fno-sanitize-recover=all -Iinclude -Ibeatrice_amd/csrc
//       tools/flowtrack_host_check.cpp -o tools/flowtrack_host_check && tools/flowtrack_host_check   (one command line)
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
static bt_flow_track_result g_result;
static bt_flow_track_expire_result g_xresult;
alignas(256) static unsigned char g_state[1 << 16];
alignas(256) static unsigned char g_scratch[1 << 16];
static const FkShadow g_shadow{BT_FLOWTAB_BIDIRECTIONAL, 100u, 256u};

struct Call {   // an update call with nothing wrong
    bt_batch frames{};
    bt_flow_track_update upd{};
    bt_flow_track_out out{};
    void* state = g_state;
    void* scratch = g_scratch;
    uint64_t scratch_bytes = sizeof(g_scratch);
    const FkShadow* sh = &g_shadow;
    bool no_frames = false, no_upd = false, no_out = false;
    Call() {
        frames.base = g_frames; frames.desc = g_desc; frames.n = 2; frames.bytes = sizeof(g_frames);
        out.result = &g_result;
    }
};

static bool run(const Call& c, FlowtabArgs* fa, FlowtrackArgs* ka, const char* word, size_t cap = 160) {
    std::vector<char> why(cap, '?');
    const bool ok = flowtrack_update_args(c.sh, c.state, c.no_frames ? nullptr : &c.frames, nullptr, c.no_upd ? nullptr : &c.upd,
                                          c.scratch, c.scratch_bytes, c.no_out ? nullptr : &c.out, fa, ka, why.data(), cap);
    if (ok) return word == nullptr;
    return word && std::strlen(why.data()) < cap && std::strstr(why.data(), word);
}

static bool refuses(const Call& c, const char* word, size_t cap = 160) {
    FlowtabArgs fa;
    FlowtrackArgs ka;
    return run(c, &fa, &ka, word, cap);
}

struct XCall {   // an expire call with nothing wrong
    bt_flow_track_expire_out out{};
    void* state = g_state;
    void* scratch = g_scratch;
    uint64_t scratch_bytes = sizeof(g_scratch);
    const FkShadow* sh = &g_shadow;
    bool no_out = false;
    XCall() { out.result = &g_xresult; }
};

static bool xrun(const XCall& c, FlowexpArgs* xa, const char* word) {
    char why[160];
    const bool ok = flowtrack_expire_args(c.sh, c.state, 10, 5, c.scratch, c.scratch_bytes, c.no_out ? nullptr : &c.out, xa, why, sizeof(why));
    if (ok) return word == nullptr;
    return word && std::strstr(why, word);
}

static bool xrefuses(const XCall& c, const char* word) {
    FlowexpArgs xa;
    return xrun(c, &xa, word);
}

static bool init_refuses(const void* state, uint64_t bytes, const bt_flow_track_opts* o, const char* word) {
    char why[160];
    bt_flow_track_sizes l{};
    if (flowtrack_init_args(state, bytes, o, &l, why, sizeof(why))) return word == nullptr;
    return word && std::strstr(why, word);
}

// Ethernet + IPv4 + TCP between 10.0.x.y and 10.9.0.1, source port 1000 + k.
static std::vector<uint8_t> flow_frame(uint32_t k, uint32_t extra = 0) {
    std::vector<uint8_t> f(12, 0);
    f.push_back(0x08); f.push_back(0x00);
    const size_t o3 = f.size();
    f.resize(o3 + 20, 0);
    f[o3] = 0x45; f[o3 + 9] = 6;
    const uint8_t addr[8] = {10, 0, (uint8_t)(k >> 8), (uint8_t)k, 10, 9, 0, 1};
    memcpy(&f[o3 + 12], addr, 8);
    const uint16_t sp = (uint16_t)(1000 + k);
    const uint8_t ports[4] = {(uint8_t)(sp >> 8), (uint8_t)sp, 0, 80};
    f.insert(f.end(), ports, ports + 4);
    f.resize(f.size() + 16 + extra, 0);
    return f;
}

struct Batch {
    std::vector<uint8_t> data;
    std::vector<uint64_t> desc;
    void add(const std::vector<uint8_t>& f) {
        data.push_back(0xEE);   // odd offsets
        desc.push_back(BT_DESC(data.size(), f.size()));
        data.insert(data.end(), f.begin(), f.end());
    }
};

struct Tracker {   // a state in a heap block of exactly its size
    void* state = nullptr;
    bt_flow_track_sizes l{};
    FkHostState hs{};
    Tracker(uint32_t flow_cap, uint32_t flags, uint32_t slots) {
        char why[160];
        const bt_flow_track_opts o{flags, flow_cap, slots, 0u};
        CHECK(fk_layout(flow_cap, slots, &l, why, sizeof(why)));
        state = std::aligned_alloc(256, l.total);
        memset(state, 0x5A, l.total);
        CHECK(!fk_host_state(state, l.total, &hs, why, sizeof(why)) && std::strstr(why, "not an initialised tracker"));
        CHECK(flowtrack_init_args(state, l.total, &o, &l, why, sizeof(why)));
        fk_init_host(state, o, l);
        CHECK(fk_host_state(state, l.total, &hs, why, sizeof(why)));
        CHECK(!fk_host_state(state, l.total - 1, &hs, why, sizeof(why)) && std::strstr(why, "state_bytes below"));
    }
    ~Tracker() { std::free(state); }
    bt_flow_track_result update(const Batch& b, std::vector<uint32_t>* id, const uint64_t* ts, uint64_t batch_ts,
                                const uint64_t* select = nullptr) {
        std::vector<uint8_t> exact(b.data);   // reads past the batch's bytes are reports
        id->assign(b.desc.size(), 0x55555555u);
        bt_flow_track_result r{};
        fk_update_host(hs, exact.data(), exact.size(), b.desc.data(), (uint32_t)b.desc.size(), select, ts, batch_ts, id->data(), &r);
        return r;
    }
    bt_flow_track_expire_result expire(uint64_t now, uint64_t idle, std::vector<bt_flow_track_rec>* expired, uint32_t cap,
                                       std::vector<uint32_t>* remap) {
        bt_flow_track_expire_result r{};
        std::vector<bt_flow_track_rec> exact(expired ? cap + 1u : 0u);   // its last entry must stay as it is
        if (expired) memset(static_cast<void*>(exact.data()), 0x7E, exact.size() * sizeof(bt_flow_track_rec));
        remap->assign(hs.hdr->flow_cap, 0xEEEEEEEEu);
        const bt_flow_track_expire_out out{expired ? exact.data() : nullptr, expired ? cap : 0u, 0u, remap->data(), &r};
        fk_expire_host(hs, now, idle, &out);
        if (expired) {
            CHECK(r.n_expired <= cap && exact[cap].klass == 0x7E && exact[cap].last_ts == 0x7E7E7E7E7E7E7E7Eull);
            expired->assign(exact.begin(), exact.begin() + r.n_expired);
        }
        return r;
    }
};

int main() {
    // ---- the state layout
    bt_flow_track_sizes l{};
    char why[160];
    CHECK(fk_layout(1, 0, &l, why, sizeof(why)) && l.slots == 128 && l.header == 0 && l.records == 256 && l.slot_words == 512 &&
          l.total == 1024);
    CHECK(fk_layout(64, 0, &l, why, sizeof(why)) && l.slots == 128);
    CHECK(fk_layout(65, 0, &l, why, sizeof(why)) && l.slots == 256);
    CHECK(fk_layout(128, 128, &l, why, sizeof(why)) && l.slots == 128 && l.slot_words == 256 + 128 * 104 && l.total == l.slot_words + 512);
    CHECK(fk_layout(1u << 30, 0, &l, why, sizeof(why)) && l.slots == 1u << 31);
    CHECK(fk_layout(1u << 31, 1u << 31, &l, why, sizeof(why)) && l.total > ((uint64_t)104u << 31));   // the largest: slots is a u32
    CHECK(!fk_layout(0xFFFFFFFBu, 1u << 31, &l, why, sizeof(why)) && std::strstr(why, "below flow_cap"));
    CHECK(!fk_layout(0, 0, &l, why, sizeof(why)) && std::strstr(why, "flow_cap == 0"));
    CHECK(!fk_layout(0xFFFFFFFCu, 1u << 31, &l, why, sizeof(why)) && std::strstr(why, "sentinels"));
    CHECK(!fk_layout((1u << 30) + 1u, 0, &l, why, sizeof(why)) && std::strstr(why, "auto"));
    CHECK(!fk_layout(10, 129, &l, why, sizeof(why)) && std::strstr(why, "power of two"));
    CHECK(!fk_layout(10, 64, &l, why, sizeof(why)) && std::strstr(why, "below 128"));
    CHECK(!fk_layout(257, 256, &l, why, sizeof(why)) && std::strstr(why, "below flow_cap"));
    CHECK(!fk_layout(0, 0, &l, why, 6) && std::strlen(why) < 6);   // a message cut to its block
    // ... and the scratch layouts: regions in order, 256-byte aligned, growing with n
    const uint32_t ns[] = {0u, 1u, 64u, 255u, 256u, 257u, 16385u, 1u << 24, 1u << 30};
    uint64_t prev = 0;
    for (uint32_t n : ns) {
        const FkLayout s = fk_scratch(n);
        CHECK(s.ft == 0 && s.flows >= ft_layout(n, ft_auto_slots(n)).total && s.ftres - s.flows >= (uint64_t)n * 80u && s.map - s.ftres >= 72u &&
              s.parts - s.map >= (uint64_t)n * 4u && s.ctl - s.parts >= ((uint64_t)n + 255u) / 256u * sizeof(FkPart) && s.total - s.ctl >= sizeof(FkCtl));
        CHECK(s.flows % 256 == 0 && s.ftres % 256 == 0 && s.map % 256 == 0 && s.parts % 256 == 0 && s.ctl % 256 == 0 && s.total % 256 == 0);
        CHECK(s.total >= prev);
        prev = s.total;
        const FxLayout x = fx_scratch(n ? n : 1u);
        CHECK(x.ctl == 0 && x.parts >= sizeof(FxCtl) && x.tmp - x.parts >= ((uint64_t)(n ? n : 1u) + 255u) / 256u * sizeof(FxPart) &&
              x.total - x.tmp >= (uint64_t)(n ? n : 1u) * 104u && x.parts % 256 == 0 && x.tmp % 256 == 0 && x.total % 256 == 0);
    }

    // ---- bt_flow_track_init_device's checks
    bt_flow_track_opts o{0u, 100u, 0u, 0u};
    CHECK(init_refuses(g_state, sizeof(g_state), &o, nullptr));
    CHECK(init_refuses(nullptr, sizeof(g_state), &o, "null state"));
    CHECK(init_refuses(g_state + 128, sizeof(g_state), &o, "state is not 256-byte aligned"));
    CHECK(init_refuses(g_state, sizeof(g_state), nullptr, "null opts"));
    o.flags = 4;        CHECK(init_refuses(g_state, sizeof(g_state), &o, "unknown flag"));
    o = {0u, 0u, 0u, 0u};   CHECK(init_refuses(g_state, sizeof(g_state), &o, "flow_cap == 0"));
    o = {0u, 100u, 64u, 0u};   CHECK(init_refuses(g_state, sizeof(g_state), &o, "below 128"));
    o = {3u, 100u, 256u, 0u};
    CHECK(fk_layout(100, 256, &l, why, sizeof(why)));
    CHECK(init_refuses(g_state, l.total, &o, nullptr) && init_refuses(g_state, l.total - 1, &o, "below the layout"));

    // ---- bt_flow_track_update_device's checks
    Call c;
    c = Call{}; c.state = nullptr;                               CHECK(refuses(c, "null state"));
    c = Call{}; c.state = g_state + 64;                          CHECK(refuses(c, "state is not 256-byte aligned"));
    c = Call{}; c.no_frames = true;                              CHECK(refuses(c, "null frames"));
    c = Call{}; c.no_upd = true;                                 CHECK(refuses(c, "null upd"));
    c = Call{}; c.no_out = true;                                 CHECK(refuses(c, "null out"));
    c = Call{}; c.out.result = nullptr;                          CHECK(refuses(c, "null result"));
    c = Call{}; c.out.result = reinterpret_cast<bt_flow_track_result*>(reinterpret_cast<char*>(&g_result) + 4);
    CHECK(refuses(c, "result is not 8-byte aligned"));
    c = Call{}; c.out.flow_id = reinterpret_cast<uint32_t*>(g_scratch + 2);   CHECK(refuses(c, "flow_id is not"));
    c = Call{}; c.upd.ts = reinterpret_cast<const uint64_t*>(g_scratch + 4);  CHECK(refuses(c, "ts is not"));
    c = Call{}; c.scratch = g_scratch + 64;                      CHECK(refuses(c, "scratch is not 256-byte aligned"));
    c = Call{}; c.scratch = nullptr;                             CHECK(refuses(c, "null scratch"));
    c = Call{}; c.scratch_bytes = fk_scratch(2).total - 1;       CHECK(refuses(c, "below the need"));
    c = Call{}; c.frames.flags = BT_BATCH_PREFIXES;              CHECK(refuses(c, "PREFIXES"));
    c = Call{}; c.frames.flags = BT_BATCH_LEAN;                  CHECK(refuses(c, "LEAN"));
    c = Call{}; c.frames.n = (1u << 30) + 1u;                    CHECK(refuses(c, "n above 2^30"));
    c = Call{}; c.frames.n = 1u << 20;                           CHECK(refuses(c, "below the need"));
    c = Call{}; c.frames.bytes = 0;                              CHECK(refuses(c, "bytes == 0"));
    c = Call{}; c.frames.desc_format = 2;                        CHECK(refuses(c, "desc_format"));
    c = Call{}; c.frames.base = nullptr;                         CHECK(refuses(c, "null packet buffer"));
    c = Call{}; c.frames.desc = nullptr; c.frames.stride = 0;    CHECK(refuses(c, "stride"));
    c = Call{}; c.sh = nullptr;                                  CHECK(refuses(c, "not an initialised tracker"));
    c = Call{}; c.no_frames = true;                              CHECK(refuses(c, "null", 5));   // a message cut to its block

    FlowtabArgs fa;
    FlowtrackArgs ka;
    c = Call{};
    c.scratch_bytes = fk_scratch(2).total;
    CHECK(run(c, &fa, &ka, nullptr));
    const FkLayout s2 = fk_scratch(2);
    CHECK(fa.n == 2 && fa.slots == 128 && fa.flow_cap == 2 && fa.bidir == 1 && fa.l3_only == 0 && !fa.flow_id &&
          (uint8_t*)fa.tab == g_scratch && (uint8_t*)fa.flows == g_scratch + s2.flows && (uint8_t*)fa.result == g_scratch + s2.ftres);
    CHECK((uint8_t*)fa.parts + sizeof(FtPartial) <= g_scratch + s2.flows);
    CHECK((void*)ka.hdr == (void*)g_state && (uint8_t*)ka.recs == g_state + 256 && (uint8_t*)ka.slot == g_state + 256 + ft_round(100 * 104) &&
          ka.flags == BT_FLOWTAB_BIDIRECTIONAL && ka.flow_cap == 100 && ka.slots == 256 && ka.n == 2 && !ka.empty &&
          ka.flows == fa.flows && ka.ftres == fa.result && (uint8_t*)ka.map == g_scratch + s2.map && (uint8_t*)ka.parts == g_scratch + s2.parts &&
          (uint8_t*)ka.ctl == g_scratch + s2.ctl && !ka.ts && !ka.flow_id && ka.result == &g_result);
    c.out.flow_id = reinterpret_cast<uint32_t*>(g_scratch + 32768); c.upd.ts = reinterpret_cast<const uint64_t*>(g_scratch + 49152);
    c.upd.batch_ts = 77;
    CHECK(run(c, &fa, &ka, nullptr) && fa.flow_id == c.out.flow_id && ka.flow_id == c.out.flow_id && ka.ts == c.upd.ts && ka.batch_ts == 77);
    c = Call{}; c.frames.n = 0; c.scratch = nullptr; c.scratch_bytes = 0;   // an empty batch needs no scratch
    CHECK(run(c, &fa, &ka, nullptr) && fa.n == 0 && ka.n == 0 && ka.empty == 1 && !ka.map && !ka.parts && !ka.ctl && !ka.ftres &&
          ka.result == &g_result && (void*)ka.hdr == (void*)g_state);

    // ---- bt_flow_track_expire_device's checks
    XCall x;
    x = XCall{}; x.state = nullptr;                              CHECK(xrefuses(x, "null state"));
    x = XCall{}; x.state = g_state + 32;                         CHECK(xrefuses(x, "state is not 256-byte aligned"));
    x = XCall{}; x.no_out = true;                                CHECK(xrefuses(x, "null out"));
    x = XCall{}; x.out.result = nullptr;                         CHECK(xrefuses(x, "null result"));
    x = XCall{}; x.out.result = reinterpret_cast<bt_flow_track_expire_result*>(reinterpret_cast<char*>(&g_xresult) + 4);
    CHECK(xrefuses(x, "result is not 8-byte aligned"));
    x = XCall{}; x.out.expired = reinterpret_cast<bt_flow_track_rec*>(g_scratch + 4); x.out.expired_cap = 1; CHECK(xrefuses(x, "expired is not"));
    x = XCall{}; x.out.remap = reinterpret_cast<uint32_t*>(g_scratch + 2);   CHECK(xrefuses(x, "remap is not"));
    x = XCall{}; x.out.expired_cap = 1;                          CHECK(xrefuses(x, "null expired with expired_cap != 0"));
    x = XCall{}; x.scratch = nullptr;                            CHECK(xrefuses(x, "null scratch"));
    x = XCall{}; x.scratch = g_scratch + 128;                    CHECK(xrefuses(x, "scratch is not 256-byte aligned"));
    x = XCall{}; x.sh = nullptr;                                 CHECK(xrefuses(x, "not an initialised tracker"));
    x = XCall{}; x.scratch_bytes = fx_scratch(100).total - 1;    CHECK(xrefuses(x, "below the need"));
    FlowexpArgs xa;
    x = XCall{}; x.scratch_bytes = fx_scratch(100).total;
    CHECK(xrun(x, &xa, nullptr) && (void*)xa.hdr == (void*)g_state && (uint8_t*)xa.recs == g_state + 256 && xa.flow_cap == 100 && xa.slots == 256 &&
          xa.all == 1 && xa.expired_cap == 0 && xa.now == 10 && xa.idle == 5 && (uint8_t*)xa.ctl == g_scratch &&
          (uint8_t*)xa.parts == g_scratch + 256 && (uint8_t*)xa.tmp == g_scratch + 512 && xa.result == &g_xresult);
    x.out.expired = reinterpret_cast<bt_flow_track_rec*>(g_scratch + 32768); x.out.expired_cap = 0;   // room for none is not "all"
    CHECK(xrun(x, &xa, nullptr) && xa.all == 0 && xa.expired_cap == 0);

    // ---- the tracker on the host
    CHECK(fk_is_idle(100, 350, 249) && !fk_is_idle(100, 350, 250) && !fk_is_idle(351, 350, 0) && fk_is_idle(0, ~0ull, ~0ull - 1) &&
          !fk_is_idle(0, ~0ull, ~0ull));
    {
        Tracker t(4, BT_FLOWTAB_BIDIRECTIONAL, 0);
        std::vector<uint32_t> id, remap;
        std::vector<bt_flow_track_rec> gone;
        Batch b0;
        b0.add(flow_frame(0)); b0.add(flow_frame(1)); b0.add(flow_frame(0, 6)); b0.add(std::vector<uint8_t>(10, 0));
        const uint64_t ts0[] = {50, 60, 40, 0};
        bt_flow_track_result r = t.update(b0, &id, ts0, 0);
        CHECK(r.n == 4 && r.n_selected == 4 && r.none_packets == 1 && r.batch_flows == 2 && r.new_flows == 2 && r.overflow_flows == 0 &&
              r.n_flows == 2 && r.seq == 0 && r.status == 0 && r.keyed_bytes == 54 + 54 + 60 && r.none_bytes == 10);
        CHECK(id[0] == 0 && id[1] == 1 && id[2] == 0 && id[3] == BT_FLOW_ID_NONE);
        const bt_flow_track_rec* recs = t.hs.recs;
        CHECK(recs[0].first == 0 && recs[0].last == 2 && recs[0].first_ts == 50 && recs[0].last_ts == 40 && recs[0].packets[0] == 2 &&
              recs[0].bytes[0] == 114 && recs[0].first_batch == 0 && recs[0].klass == BT_FLOW_V4_L4);
        // the second batch: flow 1 again, three new flows of which one fits... flow_cap 4: two fit, one overflows
        Batch b1;
        b1.add(flow_frame(2)); b1.add(flow_frame(1)); b1.add(flow_frame(3)); b1.add(flow_frame(4)); b1.add(flow_frame(4, 2)); b1.add(flow_frame(2));
        r = t.update(b1, &id, nullptr, 99);
        CHECK(r.batch_flows == 4 && r.new_flows == 2 && r.overflow_flows == 1 && r.overflow_packets == 2 && r.overflow_bytes == 54 + 56 &&
              r.n_flows == 4 && r.seq == 1);
        CHECK(id[0] == 2 && id[1] == 1 && id[2] == 3 && id[3] == BT_FLOW_ID_OVERFLOW && id[4] == BT_FLOW_ID_OVERFLOW && id[5] == 2);
        CHECK(recs[1].last_batch == 1 && recs[1].last == 1 && recs[1].last_ts == 99 && recs[1].first_ts == 60 && recs[1].packets[0] == 2);
        CHECK(recs[2].first == 0 && recs[2].last == 5 && recs[2].packets[0] == 2 && recs[2].first_batch == 1 && recs[3].first == 2);
        CHECK(t.hs.hdr->seq == 2 && t.hs.hdr->overflow_packets == 2 && t.hs.hdr->overflow_bytes == 110 && t.hs.hdr->none_packets == 1 &&
              t.hs.hdr->selected_packets == 10 && t.hs.hdr->keyed_packets == 9 && t.hs.hdr->keyed_bytes == r.keyed_bytes + 168);
        // select: bits at or above n are ignored
        const uint64_t sel = ~0ull << 1;
        r = t.update(b0, &id, nullptr, 100, &sel);
        CHECK(r.n_selected == 3 && id[0] == BT_FLOW_ID_UNSELECTED && id[1] == 1 && id[2] == 0 && r.new_flows == 0 && r.seq == 2);
        // an empty batch is a batch
        Batch none;
        r = t.update(none, &id, nullptr, 0);
        CHECK(r.n == 0 && r.seq == 3 && r.n_flows == 4 && t.hs.hdr->seq == 4);
        // last_ts: flow 0 100, flow 1 100, flow 2 99, flow 3 99
        bt_flow_track_expire_result e = t.expire(199, 100, &gone, 4, &remap);   // 199 - 99 == 100 stays
        CHECK(e.n_flows_before == 4 && e.n_idle == 0 && e.n_expired == 0 && e.n_flows == 4 && remap[0] == 0 && remap[3] == 3);
        e = t.expire(200, 100, &gone, 1, &remap);   // flows 2 and 3 are idle, room for one
        CHECK(e.n_idle == 2 && e.n_expired == 1 && e.n_flows == 3 && remap[0] == 0 && remap[1] == 1 && remap[2] == BT_FLOW_ID_EXPIRED &&
              remap[3] == 2 && gone[0].first_batch == 1 && gone[0].packets[0] == 2 && gone[0].key[3] == 2);
        CHECK(recs[2].key[3] == 3 && recs[3].klass == 0 && recs[3].packets[0] == 0 && t.hs.hdr->n_flows == 3);
        e = t.expire(200, 100, &gone, 0, &remap);   // room for none: nothing is lost
        CHECK(e.n_idle == 1 && e.n_expired == 0 && e.n_flows == 3);
        e = t.expire(50, 0, nullptr, 0, &remap);    // every last_ts is above now
        CHECK(e.n_idle == 0 && e.n_flows == 3);
        // the flow that left comes back as a new flow at the end; the others are found where they are now
        Batch b2;
        b2.add(flow_frame(3)); b2.add(flow_frame(2)); b2.add(flow_frame(0));
        r = t.update(b2, &id, nullptr, 300);
        CHECK(id[0] == 2 && id[1] == 3 && id[2] == 0 && r.new_flows == 1 && r.n_flows == 4 && recs[3].first_batch == 4 && recs[3].first_ts == 300);
        e = t.expire(1000, 10, nullptr, 0, &remap);   // expired == NULL: all go
        CHECK(e.n_idle == 4 && e.n_expired == 4 && e.n_flows == 0 && remap[0] == BT_FLOW_ID_EXPIRED && remap[3] == BT_FLOW_ID_EXPIRED);
        for (uint32_t f = 0; f < 4; ++f) CHECK(recs[f].klass == 0 && recs[f].last_ts == 0);
        for (uint32_t k = 0; k < t.l.slots; ++k) CHECK(t.hs.slot[k] == kFkEmpty);
    }
    {   // a table loaded to 1.0: 128 flows in 128 slots, a 129th overflows, the same 128 again are all found
        Tracker t(128, 0, 128);
        std::vector<uint32_t> id, remap;
        Batch full, more, again;
        for (uint32_t k = 0; k < 128; ++k) full.add(flow_frame(k));
        more.add(flow_frame(128)); more.add(flow_frame(7));
        for (uint32_t k = 128; k-- > 0;) again.add(flow_frame(k));
        bt_flow_track_result r = t.update(full, &id, nullptr, 1);
        CHECK(r.new_flows == 128 && r.n_flows == 128 && id[127] == 127);
        for (uint32_t k = 0; k < 128; ++k) CHECK(t.hs.slot[k] < 128);
        r = t.update(more, &id, nullptr, 2);
        CHECK(r.overflow_flows == 1 && r.overflow_packets == 1 && id[0] == BT_FLOW_ID_OVERFLOW && id[1] == 7);
        r = t.update(again, &id, nullptr, 3);
        CHECK(r.new_flows == 0 && r.overflow_flows == 0 && id[0] == 127 && id[127] == 0);
        std::vector<bt_flow_track_rec> gone;
        bt_flow_track_expire_result e = t.expire(10, 0, &gone, 128, &remap);
        CHECK(e.n_expired == 128 && e.n_flows == 0 && gone[5].key[3] == 5 && gone[5].packets[0] == 2);
    }
    if (g_bad) {
        std::printf("%d checks FAILED\n", g_bad);
        return 1;
    }
    std::printf("flowtrack_host_check: all cases hold\n");
    return 0;
}
