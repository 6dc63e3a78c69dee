// bt_flowhosts.hip — the endpoint table of a flow tracker (bt_flow_track_hosts_device,
// include/beatrice_gpu.h): an exact group-by on the address over the records of a device-resident
// tracker state. Every live flow f gives two contributions c = 2 f + role; one bt_flow_host_rec
// per distinct (family, address), numbered in order of first appearance. The state and the side
// table are only read. One thread per flow, its two contributions one after the other, blocks of
// four waves; the grids are sized by flow_cap and threads at or past n_flows do nothing.
//   bt_flowhosts_begin   the header check and n_flows into the control block (block 0); the grid
//                        sets every slot to empty, a share per block.
//   bt_flowhosts_insert  open addressing, linear probing, at most `slots` steps, the lanes of a wave
//                        in step. A slot is one word: empty, or a contribution of its host. It is
//                        claimed by a device-scope atomicCAS from empty to c, issued by the lowest
//                        of the lanes of the wave that read that slot as empty (for the slots of
//                        the first two such lanes; the others take its outcome by a shuffle), so a
//                        hub's empty word takes one CAS per wave; a lane that finds an owner compares
//                        family and address with the owner's tracker record (the keys are in the
//                        state, none is copied) and takes atomicMin(word, c), so the word ends as the
//                        host's lowest contribution. The word only falls: a lane that read a value
//                        <= c issues nothing, and of the lanes of a wave that found the first such
//                        lane's slot only that one (the lowest c) issues. cslot[c] = the slot.
//   bt_flowhosts_firsts  c is its host's first when its slot's word == c: those bits per wave and
//                        role, their counts per wave and block, the contributions without a slot,
//                        the family-4 firsts, and the block's packet and byte sums.
//   bt_flowhosts_join    one block: the exclusive scan of the blocks' counts, and *result.
//   bt_flowhosts_rank    a first contribution's number = block start + waves below + firsts below
//                        it in (lane, role) order. It goes into the slot word (the minimum has
//                        served), and for a number below host_cap hosts[number] is written whole with
//                        16-byte stores: address, family, first_flow and the contribution's own
//                        share of every sum. A table of all-distinct hosts is complete here and the
//                        sum pass issues no atomic for it.
//   bt_flowhosts_sum     grid-stride over a bounded grid. Every contribution reads its host's
//                        number from its slot and writes endpoint_host. The contributions that are
//                        not their host's first add themselves: the lanes of a wave that hit the
//                        host of the first such lane are summed by shuffles and ballots (done for
//                        the first two pending hosts), then every value goes into the block's LDS cache
//                        (kFhCache host records, direct-mapped by the host's number, an entry
//                        claimed by an LDS atomicCAS on its tag), or straight to hosts[] with global
//                        atomics when its entry belongs to another host. At its end the block adds
//                        every claimed entry's non-zero fields to hosts[] once. A hub that is in
//                        every flow costs one atomic per field and block, a few tens of thousands
//                        per call however many flows there are; the first kernel that added per
//                        contribution on the TCP side table took 40 times its successor's time.
// No lane waits for another lane, wave or block: no spin, no flag, no look-back; what one kernel
// tells the next goes through the kernel boundary, and every loop has its bound in its head. Why
// the outputs are the same from run to run although lanes race for slots: which slot a host gets,
// and which contribution claims it, varies; but a host has exactly one slot (a claimed slot is
// never given up, its word only ever holds contributions of the one host, and every contribution
// of the host walks the same probe sequence up to it), the word's final value is the minimum over
// the same set whatever the order, a host's number is the rank of that minimum, and every field of
// a record is an integer sum, a minimum or a maximum over the same contributions whether they
// arrive singly, combined in a wave, through the LDS cache or directly. The scratch holds the only
// values that vary. Across the XCDs' L2s: the kernels read only atomics' results and data written
// by earlier kernels.
#include "bt_flowtrack_dev.h"
#include "bt_hip_launch.h"
#include "bt_wave.h"
#include "bt_flowhosts.h"

namespace bt {

namespace {

typedef u32x4 u32x4_a8 __attribute__((aligned(8)));   // a record is 8-byte aligned: 104 B = six of these and a u64
typedef u32x4 u32x4_a4 __attribute__((aligned(4)));   // a side record is 4-byte aligned
typedef u32x2 u32x2_a4 __attribute__((aligned(4)));   // as endpoint_host is

// The first ten words of record f: the 36 key bytes, the class, zeros.
__device__ __forceinline__ void head_load(const bt_flow_track_rec* r, uint32_t (&w)[10]) {
    const u32x4_a8* const p = reinterpret_cast<const u32x4_a8*>(r);
    const u32x4 x = p[0], y = p[1];
    const u32x2 z = *reinterpret_cast<const u32x2*>(reinterpret_cast<const uint8_t*>(r) + 32);
    w[0] = x.x; w[1] = x.y; w[2] = x.z; w[3] = x.w;
    w[4] = y.x; w[5] = y.y; w[6] = y.z; w[7] = y.w;
    w[8] = z.x; w[9] = z.y;
}

// The whole record as 26 words.
__device__ __forceinline__ void rec_load(const bt_flow_track_rec* r, uint32_t (&w)[26]) {
    const u32x4_a8* const p = reinterpret_cast<const u32x4_a8*>(r);
#pragma unroll
    for (int j = 0; j < 6; ++j) {
        const u32x4 t = p[j];
        w[4 * j] = t.x; w[4 * j + 1] = t.y; w[4 * j + 2] = t.z; w[4 * j + 3] = t.w;
    }
    const u32x2 z = *reinterpret_cast<const u32x2*>(reinterpret_cast<const uint8_t*>(r) + 96);
    w[24] = z.x; w[25] = z.y;
}

__device__ __forceinline__ uint64_t u64_of(const uint32_t* w, int i) { return (uint64_t)w[i + 1] << 32 | w[i]; }

// What one contribution, or several of one host and one role, add to the host's record.
struct Share {
    uint32_t flows;               // to flows[role]
    uint64_t ps, pr, bs, br;      // packets / bytes sent and received
    uint64_t fts, lts;            // minimum / maximum
    uint32_t st[7], syn_s, syn_r, syn, fin, rst;
};

// Role `role` of a loaded record w with its side record t (four words; has_tcp: there is one).
__device__ __forceinline__ Share share_of(const uint32_t (&w)[26], const uint32_t (&t)[4], bool has_tcp, uint32_t role, uint32_t flags) {
    Share s;
    s.flows = 1u;
    s.ps = u64_of(w, 14 + 2 * (int)role); s.pr = u64_of(w, 16 - 2 * (int)role);   // packets[] at byte 56
    s.bs = u64_of(w, 18 + 2 * (int)role); s.br = u64_of(w, 20 - 2 * (int)role);   // bytes[] at 72
    s.fts = u64_of(w, 22); s.lts = u64_of(w, 24);
    const uint32_t f0 = t[0] & 0xFFu, f1 = (t[0] >> 8) & 0xFFu;
    const int state = has_tcp ? flowtcp_state(f0, f1, flags) : -1;
#pragma unroll
    for (int j = 0; j < 7; ++j) s.st[j] = state == j ? 1u : 0u;
    const uint32_t fs = role ? f1 : f0, fr = role ? f0 : f1;
    s.syn_s = has_tcp && (fs & BT_TCPF_SYN) ? 1u : 0u;
    s.syn_r = has_tcp && (fr & BT_TCPF_SYN) ? 1u : 0u;
    s.syn = has_tcp ? t[1] : 0u; s.fin = has_tcp ? t[2] : 0u; s.rst = has_tcp ? t[3] : 0u;
    return s;
}

// The shares of the lanes with `in` (at least two of them) as one, to every lane.
__device__ __forceinline__ Share share_combine(const Share& s, bool in, bool has_tcp) {
    Share c;
    c.flows = (uint32_t)__popcll(__ballot(in));
    c.ps = wave_sum64(in ? s.ps : 0ull); c.pr = wave_sum64(in ? s.pr : 0ull);
    c.bs = wave_sum64(in ? s.bs : 0ull); c.br = wave_sum64(in ? s.br : 0ull);
    c.fts = wave_min64(in ? s.fts : ~0ull); c.lts = wave_max64(in ? s.lts : 0ull);
#pragma unroll
    for (int j = 0; j < 7; ++j) c.st[j] = has_tcp ? (uint32_t)__popcll(__ballot(in && s.st[j])) : 0u;
    c.syn_s = has_tcp ? (uint32_t)__popcll(__ballot(in && s.syn_s)) : 0u;
    c.syn_r = has_tcp ? (uint32_t)__popcll(__ballot(in && s.syn_r)) : 0u;
    c.syn = has_tcp ? wave_sum(in ? s.syn : 0u) : 0u;
    c.fin = has_tcp ? wave_sum(in ? s.fin : 0u) : 0u;
    c.rst = has_tcp ? wave_sum(in ? s.rst : 0u) : 0u;
    return c;
}

// A share into a host record in LDS or in hosts[]: atomics on its non-zero fields.
__device__ __forceinline__ void share_add(bt_flow_host_rec* h, uint32_t role, const Share& s) {
    typedef unsigned long long ull;
    if (s.flows) atomicAdd(&h->flows[role], s.flows);
    if (s.ps) atomicAdd(reinterpret_cast<ull*>(&h->packets[0]), (ull)s.ps);
    if (s.pr) atomicAdd(reinterpret_cast<ull*>(&h->packets[1]), (ull)s.pr);
    if (s.bs) atomicAdd(reinterpret_cast<ull*>(&h->bytes[0]), (ull)s.bs);
    if (s.br) atomicAdd(reinterpret_cast<ull*>(&h->bytes[1]), (ull)s.br);
    if (s.fts != ~0ull) atomicMin(reinterpret_cast<ull*>(&h->first_ts), (ull)s.fts);
    if (s.lts) atomicMax(reinterpret_cast<ull*>(&h->last_ts), (ull)s.lts);
#pragma unroll
    for (int j = 0; j < 7; ++j)
        if (s.st[j]) atomicAdd(&h->tcp_state[j], s.st[j]);
    if (s.syn_s) atomicAdd(&h->syn_flows[0], s.syn_s);
    if (s.syn_r) atomicAdd(&h->syn_flows[1], s.syn_r);
    if (s.syn) atomicAdd(&h->syn_packets, s.syn);
    if (s.fin) atomicAdd(&h->fin_packets, s.fin);
    if (s.rst) atomicAdd(&h->rst_packets, s.rst);
}

}  // namespace

static_assert(kFhCache == kFkThreads, "one thread per entry of the sum pass's LDS cache");

// H0: the control block, every slot empty.
__global__ __launch_bounds__(kFkThreads) void bt_flowhosts_begin(FlowhostsArgs a) {
    slots_fill<kFkThreads>(a.tab, a.slots, kFhEmpty);
    if (blockIdx.x == 0 && threadIdx.x == 0) {
        const bool ok = hdr_ok(a, a.state_slots);
        *a.ctl = FhCtl{ok ? 1u : 0u, ok ? a.hdr->n_flows : 0u, {0u, 0u}};
    }
}

// H1: every contribution finds or claims its host's slot; the slot's word falls to the host's lowest contribution.
__global__ __launch_bounds__(kFkThreads) void bt_flowhosts_insert(FlowhostsArgs a) {
    if (!a.ctl->ok) return;
    const uint32_t nf = a.ctl->n_flows;
    const uint64_t f0 = (uint64_t)blockIdx.x * kFkThreads;
    if (f0 >= nf) return;   // the whole block
    const uint32_t lane = threadIdx.x & 63u, mask = a.slots - 1u;
    const uint64_t f = f0 + threadIdx.x;
    const bool live = f < nf;   // nf <= flow_cap
    uint32_t w[10];
#pragma unroll
    for (int j = 0; j < 10; ++j) w[j] = 0u;
    if (live) head_load(a.recs + f, w);
    uint32_t found[2] = {kFhEmpty, kFhEmpty};
#pragma unroll
    for (uint32_t role = 0; role < 2u; ++role) {
        const uint32_t c = 2u * (uint32_t)f + role;   // f < 2^31 - 1
        uint32_t adr[4];
        const uint32_t family = fh_addr(w, role, adr);
        uint32_t at = kFhEmpty, seen = 0u;   // seen: the word's value when the host was found there
        // The wave probes in step: every lane still searching takes one slot per turn of the loop, so
        // that the lanes that meet one empty slot can let one of them claim it.
        bool searching = live;
        uint32_t s = fh_hash(family, adr) & mask;
        for (uint32_t probe = 0; probe < a.slots; ++probe) {   // every slot once, then overflow
            if (!__ballot(searching)) break;
            // A slot's word changes from empty to a contribution of one host and then only to
            // lower contributions of that host: whatever is read names the slot's host.
            uint32_t owner = searching ? __hip_atomic_load(&a.tab[s], __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT) : 0u;
            const bool empty = searching && owner == kFhEmpty;
            // Of the lanes that read one slot as empty the lowest issues the atomicCAS and the others
            // take its outcome: what it found there, or its own contribution when it claimed the slot.
            // Done for the slots of the first two such lanes; a lane at another slot issues its own.
            uint64_t pend = __ballot(empty);
            bool follow = false;
            uint32_t lead = 0u;
            for (uint32_t turn = 0; turn < 2u && pend; ++turn) {
                const int first = __ffsll((unsigned long long)pend) - 1;
                const uint32_t s0 = (uint32_t)__shfl((int)s, first);
                const bool in = empty && s == s0;
                if (in && lane != (uint32_t)first) { follow = true; lead = (uint32_t)first; }
                pend &= ~__ballot(in);
            }
            if (empty && !follow) owner = atomicCAS(&a.tab[s], kFhEmpty, c);
            const uint32_t o_lead = (uint32_t)__shfl((int)owner, (int)lead), c_lead = (uint32_t)__shfl((int)c, (int)lead);
            if (follow) owner = o_lead == kFhEmpty ? c_lead : o_lead;
            if (searching) {
                if (owner == kFhEmpty) { at = s; seen = c; searching = false; }   // claimed
                else {
                    const uint32_t of = owner >> 1;
                    bool same = false;
                    if (of < a.flow_cap) {   // a contribution of a live flow
                        uint32_t ow[10], oa[4];
                        head_load(a.recs + of, ow);
                        const uint32_t ofam = fh_addr(ow, owner & 1u, oa);
                        same = ofam == family && oa[0] == adr[0] && oa[1] == adr[1] && oa[2] == adr[2] && oa[3] == adr[3];
                    }
                    if (same) { at = s; seen = owner; searching = false; }
                    else s = (s + 1u) & mask;
                }
            }
        }
        found[role] = at;
        const bool lower = live && at != kFhEmpty && seen > c;
        const uint64_t m = __ballot(lower);
        if (m) {
            const int first = __ffsll((unsigned long long)m) - 1;
            const uint32_t at0 = (uint32_t)__shfl((int)at, first);
            // the lanes behind `first` at its slot carry higher contributions: the first speaks for them
            if (lower && (at != at0 || lane == (uint32_t)first)) atomicMin(&a.tab[at], c);
        }
    }
    if (live) *reinterpret_cast<u32x2*>(a.cslot + 2u * f) = u32x2{found[0], found[1]};
}

// H2: the first contribution of every host, as bits and counts; the block's sums.
__global__ __launch_bounds__(kFkThreads) void bt_flowhosts_firsts(FlowhostsArgs a) {
    __shared__ uint32_t red[kFkWaves][3];
    __shared__ uint64_t red64[kFkWaves][2];
    if (!a.ctl->ok) return;
    const uint32_t nf = a.ctl->n_flows;
    const uint64_t f0 = (uint64_t)blockIdx.x * kFkThreads;
    if (f0 >= nf) return;
    const uint32_t tid = threadIdx.x, lane = tid & 63u, wid = tid >> 6;
    const uint64_t f = f0 + tid;
    const bool live = f < nf;
    bool first[2] = {false, false}, over[2] = {false, false};
    uint64_t pk = 0, by = 0;
    uint32_t klass = 0;
    if (live) {
        const u32x2 cs = *reinterpret_cast<const u32x2*>(a.cslot + 2u * f);
        const uint32_t c = 2u * (uint32_t)f;
        over[0] = cs.x == kFhEmpty; over[1] = cs.y == kFhEmpty;
        first[0] = !over[0] && a.tab[cs.x & (a.slots - 1u)] == c;
        first[1] = !over[1] && a.tab[cs.y & (a.slots - 1u)] == c + 1u;
        const uint64_t* const q = reinterpret_cast<const uint64_t*>(a.recs + f);
        klass = (uint32_t)(q[4] >> 32) & 0xFFu;
        pk = q[7] + q[8];
        by = q[9] + q[10];
    }
    const bool v4 = !(klass == BT_FLOW_V6 || klass == BT_FLOW_V6_L4);
    const uint64_t b0 = __ballot(first[0]), b1 = __ballot(first[1]);
    const uint32_t nfirst = (uint32_t)(__popcll(b0) + __popcll(b1));
    const uint32_t nover = (uint32_t)(__popcll(__ballot(over[0])) + __popcll(__ballot(over[1])));
    const uint32_t nv4 = (uint32_t)(__popcll(__ballot(first[0] && v4)) + __popcll(__ballot(first[1] && v4)));
    pk = wave_sum64(pk);
    by = wave_sum64(by);
    FhPart& p = a.parts[blockIdx.x];
    if (lane == 0) {
        red[wid][0] = nfirst; red[wid][1] = nover; red[wid][2] = nv4;
        red64[wid][0] = pk; red64[wid][1] = by;
        p.wfirst[wid] = nfirst;
        p.firstw[wid][0] = b0; p.firstw[wid][1] = b1;
    }
    __syncthreads();
    if (tid == 0) {
        uint32_t s0 = 0, s1 = 0, s2 = 0;
        uint64_t t0 = 0, t1 = 0;
#pragma unroll
        for (uint32_t v = 0; v < kFkWaves; ++v) { s0 += red[v][0]; s1 += red[v][1]; s2 += red[v][2]; t0 += red64[v][0]; t1 += red64[v][1]; }
        p.nfirst = s0; p.rel = 0u; p.nover = s1; p.nv4 = s2;
        p.packets = t0; p.bytes = t1;
    }
}

// H3: where every block's hosts start, and *result.
__global__ __launch_bounds__(kFhJoinThreads) void bt_flowhosts_join(FlowhostsArgs a) {
    constexpr uint32_t kWaves = kFhJoinThreads / 64u;
    __shared__ uint32_t sh[kWaves];
    __shared__ uint64_t tot[kWaves][4];
    const uint32_t tid = threadIdx.x, lane = tid & 63u, wid = tid >> 6;
    if (!a.ctl->ok) {
        if (tid == 0) {
            bt_flow_hosts_result r{};
            r.status = 1u;
            *a.result = r;
        }
        return;
    }
    const uint32_t nf = a.ctl->n_flows;
    const uint32_t nparts = (uint32_t)(((uint64_t)nf + kFkThreads - 1u) / kFkThreads), per = (nparts + kFhJoinThreads - 1u) / kFhJoinThreads;
    const uint32_t lo = (uint64_t)tid * per < nparts ? tid * per : nparts, hi = nparts - lo > per ? lo + per : nparts;
    uint32_t mine = 0;
    uint64_t over = 0, v4 = 0, pk = 0, by = 0;
    for (uint32_t q = lo; q < hi; ++q) {
        const FhPart& p = a.parts[q];
        mine += p.nfirst; over += p.nover; v4 += p.nv4; pk += p.packets; by += p.bytes;
    }
    uint32_t incl = mine;   // the exclusive scan of `mine` over the block
    for (int o = 1; o < 64; o <<= 1) {
        const uint32_t y = __shfl_up(incl, o);
        if (lane >= (uint32_t)o) incl += y;
    }
    over = wave_sum64(over); v4 = wave_sum64(v4); pk = wave_sum64(pk); by = wave_sum64(by);
    if (lane == 63u) sh[wid] = incl;
    if (lane == 0) { tot[wid][0] = over; tot[wid][1] = v4; tot[wid][2] = pk; tot[wid][3] = by; }
    __syncthreads();
    uint32_t pre = 0, all = 0;
#pragma unroll
    for (uint32_t w = 0; w < kWaves; ++w) {
        const uint32_t x = sh[w];
        pre += w < wid ? x : 0u;
        all += x;
    }
    uint32_t rel = pre + incl - mine;
    for (uint32_t q = lo; q < hi; ++q) {
        a.parts[q].rel = rel;
        rel += a.parts[q].nfirst;
    }
    if (tid == 0) {
        uint64_t s[4] = {0, 0, 0, 0};
        for (uint32_t w = 0; w < kWaves; ++w)
            for (int j = 0; j < 4; ++j) s[j] += tot[w][j];
        bt_flow_hosts_result r{};
        r.n_flows = nf; r.n_hosts = all; r.n_written = all < a.host_cap ? all : a.host_cap; r.status = 0u;
        r.overflow_endpoints = (uint32_t)s[0]; r.slots = a.slots; r.hosts_v4 = (uint32_t)s[1]; r.hosts_v6 = all - (uint32_t)s[1];
        r.packets_total = s[2]; r.bytes_total = s[3];
        *a.result = r;
    }
}

// H4: first contributions number their host and write its record with their own share.
__global__ __launch_bounds__(kFkThreads) void bt_flowhosts_rank(FlowhostsArgs a) {
    if (!a.ctl->ok) return;
    const uint32_t nf = a.ctl->n_flows;
    const uint64_t f0 = (uint64_t)blockIdx.x * kFkThreads;
    if (f0 >= nf) return;
    const uint32_t tid = threadIdx.x, lane = tid & 63u, wid = tid >> 6;
    const FhPart& p = a.parts[blockIdx.x];
    if (!p.nfirst) return;   // the whole block
    const uint64_t b0 = p.firstw[wid][0], b1 = p.firstw[wid][1];   // bits at or past n_flows are 0
    const bool first0 = (b0 >> lane) & 1ull, first1 = (b1 >> lane) & 1ull;
    if (!first0 && !first1) return;
    uint32_t base = p.rel;
    for (uint32_t v = 0; v < wid; ++v) base += p.wfirst[v];
    const uint64_t below = (1ull << lane) - 1ull;
    base += (uint32_t)(__popcll(b0 & below) + __popcll(b1 & below));
    const uint64_t f = f0 + tid;   // a first contribution: f < n_flows
    const u32x2 cs = *reinterpret_cast<const u32x2*>(a.cslot + 2u * f);
    uint32_t w[26], t[4] = {0u, 0u, 0u, 0u};
    rec_load(a.recs + f, w);
    const bool has_tcp = a.tcp != nullptr;
    if (has_tcp) {
        const u32x4 x = *reinterpret_cast<const u32x4_a4*>(a.tcp + f);
        t[0] = x.x; t[1] = x.y; t[2] = x.z; t[3] = x.w;
    }
#pragma unroll
    for (uint32_t role = 0; role < 2u; ++role) {
        if (!(role ? first1 : first0)) continue;
        const uint32_t h = base + (role && first0 ? 1u : 0u);
        const uint32_t slot = (role ? cs.y : cs.x) & (a.slots - 1u);   // a first contribution has a slot
        a.tab[slot] = h;   // the minimum has served: bt_flowhosts_sum reads the number here
        if (h >= a.host_cap) continue;
        uint32_t adr[4];
        const uint32_t family = fh_addr(w, role, adr);
        const Share s = share_of(w, t, has_tcp, role, a.flags);
        u32x4_a8* const o8 = reinterpret_cast<u32x4_a8*>(a.hosts + h);   // 128 B, 8-byte aligned: eight 16-byte stores
        const auto lo = [](uint64_t v) { return (uint32_t)v; };
        const auto hi = [](uint64_t v) { return (uint32_t)(v >> 32); };
        o8[0] = u32x4{adr[0], adr[1], adr[2], adr[3]};
        o8[1] = u32x4{family, (uint32_t)f, role ? 0u : 1u, role ? 1u : 0u};
        o8[2] = u32x4{lo(s.ps), hi(s.ps), lo(s.pr), hi(s.pr)};
        o8[3] = u32x4{lo(s.bs), hi(s.bs), lo(s.br), hi(s.br)};
        o8[4] = u32x4{lo(s.fts), hi(s.fts), lo(s.lts), hi(s.lts)};
        o8[5] = u32x4{s.st[0], s.st[1], s.st[2], s.st[3]};
        o8[6] = u32x4{s.st[4], s.st[5], s.st[6], s.syn_s};
        o8[7] = u32x4{s.syn_r, s.syn, s.fin, s.rst};
    }
}

// H5: endpoint_host, and every contribution that is not its host's first adds itself.
__global__ __launch_bounds__(kFkThreads) void bt_flowhosts_sum(FlowhostsArgs a) {
    __shared__ bt_flow_host_rec cache[kFhCache];
    __shared__ uint32_t tag[kFhCache];
    if (!a.ctl->ok) return;
    const uint32_t nf = a.ctl->n_flows;
    const uint64_t step = (uint64_t)gridDim.x * kFkThreads;
    if ((uint64_t)blockIdx.x * kFkThreads >= nf) return;   // the whole block
    const uint32_t tid = threadIdx.x, lane = tid & 63u, wid = tid >> 6;
    const bool has_tcp = a.tcp != nullptr;
    {
        bt_flow_host_rec z{};
        z.first_ts = ~0ull;
        cache[tid] = z;
        tag[tid] = kFhEmpty;
    }
    __syncthreads();
    // A share to host h < host_cap: into the cache when h's entry is free or h's, else to hosts[h].
    const auto give = [&](uint32_t h, uint32_t role, const Share& s) {
        const uint32_t e = h & (kFhCache - 1u);
        uint32_t owner = tag[e];
        if (owner == kFhEmpty) owner = atomicCAS(&tag[e], kFhEmpty, h);
        if (owner == kFhEmpty || owner == h) share_add(&cache[e], role, s);
        else share_add(a.hosts + h, role, s);
    };
    for (uint64_t f0 = (uint64_t)blockIdx.x * kFkThreads; f0 < nf; f0 += step) {   // f < nf <= flow_cap
        const uint64_t f = f0 + tid;
        const bool live = f < nf;
        const FhPart& p = a.parts[f0 / kFkThreads];
        uint32_t num[2] = {kFhEmpty, kFhEmpty};
        bool act[2] = {false, false};
        if (live) {
            const u32x2 cs = *reinterpret_cast<const u32x2*>(a.cslot + 2u * f);
            if (cs.x != kFhEmpty) num[0] = a.tab[cs.x & (a.slots - 1u)];
            if (cs.y != kFhEmpty) num[1] = a.tab[cs.y & (a.slots - 1u)];
            if (a.endpoint_host) *reinterpret_cast<u32x2_a4*>(a.endpoint_host + 2u * f) = u32x2{num[0], num[1]};
            // a first contribution's share is in hosts[] already (bt_flowhosts_rank)
            act[0] = num[0] < a.host_cap && !((p.firstw[wid][0] >> lane) & 1ull);
            act[1] = num[1] < a.host_cap && !((p.firstw[wid][1] >> lane) & 1ull);
        }
        if (!__ballot(act[0] || act[1])) continue;   // the whole wave: a table of distinct hosts ends here
        uint32_t w[26], t[4] = {0u, 0u, 0u, 0u};
#pragma unroll
        for (int j = 0; j < 26; ++j) w[j] = 0u;
        if (act[0] || act[1]) {
            rec_load(a.recs + f, w);
            if (has_tcp) {
                const u32x4 x = *reinterpret_cast<const u32x4_a4*>(a.tcp + f);
                t[0] = x.x; t[1] = x.y; t[2] = x.z; t[3] = x.w;
            }
        }
#pragma unroll
        for (uint32_t role = 0; role < 2u; ++role) {
            const uint32_t h = num[role];
            bool todo = act[role];
            const Share s = share_of(w, t, has_tcp, role, a.flags);
            uint64_t pend = __ballot(todo);
            for (uint32_t turn = 0; turn < 2u && pend; ++turn) {   // the hosts of the first two pending lanes, combined
                const int leader = __ffsll((unsigned long long)pend) - 1;
                const uint32_t h0 = (uint32_t)__shfl((int)h, leader);
                const bool in = todo && h == h0;
                const uint64_t g = __ballot(in);
                if (g & (g - 1ull)) {   // more than one lane; a lone lane stays with the rest below
                    const Share c = share_combine(s, in, has_tcp);
                    if (lane == (uint32_t)leader) give(h0, role, c);
                    todo = todo && !in;
                }
                pend &= ~g;
            }
            if (todo) give(h, role, s);
        }
    }
    __syncthreads();
    if (tag[tid] != kFhEmpty) {   // tag < host_cap
        const bt_flow_host_rec& e = cache[tid];
        bt_flow_host_rec* const h = a.hosts + tag[tid];
        Share s;
        s.ps = e.packets[0]; s.pr = e.packets[1]; s.bs = e.bytes[0]; s.br = e.bytes[1];
        s.fts = e.first_ts; s.lts = e.last_ts;
#pragma unroll
        for (int j = 0; j < 7; ++j) s.st[j] = e.tcp_state[j];
        s.syn_s = e.syn_flows[0]; s.syn_r = e.syn_flows[1];
        s.syn = e.syn_packets; s.fin = e.fin_packets; s.rst = e.rst_packets;
        s.flows = e.flows[0];
        share_add(h, 0u, s);
        if (e.flows[1]) atomicAdd(&h->flows[1], e.flows[1]);
    }
}

int launch_flowhosts(const FlowhostsArgs& a, void* stream, void* timing_start, void* timing_stop) {
    hipStream_t st = reinterpret_cast<hipStream_t>(stream);
    hipEvent_t e0 = reinterpret_cast<hipEvent_t>(timing_start), e1 = reinterpret_cast<hipEvent_t>(timing_stop);
    const uint32_t per_flow = (uint32_t)(((uint64_t)a.flow_cap + kFkThreads - 1u) / kFkThreads);   // flow_cap < 2^31
    // enough blocks to empty the slots: 64 slots a thread, at most 4,096
    const uint64_t init = ((uint64_t)a.slots + 64u * kFkThreads - 1u) / (64u * kFkThreads);
    launch(bt_flowhosts_begin, dim3((uint32_t)(init > 4096u ? 4096u : init)), dim3(kFkThreads), 0, st, e0, nullptr, a);
    launch(bt_flowhosts_insert, dim3(per_flow), dim3(kFkThreads), 0, st, nullptr, nullptr, a);
    launch(bt_flowhosts_firsts, dim3(per_flow), dim3(kFkThreads), 0, st, nullptr, nullptr, a);
    launch(bt_flowhosts_join, dim3(1), dim3(kFhJoinThreads), 0, st, nullptr, nullptr, a);
    launch(bt_flowhosts_rank, dim3(per_flow), dim3(kFkThreads), 0, st, nullptr, nullptr, a);
    launch(bt_flowhosts_sum, dim3(per_flow < kFhSumGrid ? per_flow : kFhSumGrid), dim3(kFkThreads), 0, st, nullptr, e1, a);
    return hipGetLastError() == hipSuccess ? BT_OK : BT_E_INTERNAL;
}

}  // namespace bt
