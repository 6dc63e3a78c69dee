// bt_flowtcp.hip — the per-flow TCP side table (bt_flow_tcp_update_device, include/beatrice_gpu.h):
// the union of the TCP flags per direction and the SYN / FIN / RST packet counts of every flow, from
// a device-resident batch and the flow numbers a flow table or the flow tracker gave its packets.
//
// One launch, lane = packet, one block of 8 waves per chunk of 256 tiles as bt_flowtab_keys. A lane
// whose flow number is below flow_cap walks its frame's layers (bt_flow_walk.h: the fan-out's walk,
// L4 offset and fragment rule); a TCP packet reads byte 13 of its TCP header and, when the table is
// bidirectional, forms the key the table forms to find its direction. Then, per tile:
//   1. every TCP lane reads its flow's hot word (flags[0] | flags[1] << 8, the record's first dword)
//      with a relaxed agent-scope atomic load, all lanes at once;
//   2. the lanes that would add a flag bit or carry SYN, FIN or RST are combined by flow (ballot
//      peeling, one turn per distinct flow among them, as bt_flowtab_insert);
//   3. the turn's leader issues a device-scope atomicOr only when the turn adds bits to what it
//      read; the turn's SYN / FIN / RST counts (ballot counts, wave-uniform) wait in the wave while
//      the next turns and tiles meet the same flow, and are added with one atomicAdd per counter
//      when another flow's counts come, or at the end of the block, where what the eight waves
//      still hold is combined through LDS first.
// Bits are only ever added during the kernel, so a stale read can only cause a redundant atomic,
// never a missing one: a batch that is one flow costs one atomicOr for its first tiles and none
// after and three atomicAdds per block, not several per tile on one address. The sums of *result
// are ballot counts per wave, summed per block in LDS, one atomicAdd per block and field into
// the zeroed result.
// No lane ever waits for another lane, wave or block: there is no spin, no flag and no look-back,
// and every loop has a bound in its head. Every output is an OR or an integer sum over the same
// set of packets whatever the order, so it is the same from run to run.
#include "bt_flow_walk.h"
#include "bt_hip_launch.h"
#include "bt_wave.h"
#include "bt_flowtcp.h"

namespace bt {

namespace {

constexpr uint32_t kTcpThreads = kFtWaves * 64u;
constexpr uint32_t kTcpWaveTiles = kFtChunkTiles / kFtWaves;

constexpr uint32_t kTcpNoFlow = 0xFFFFFFFFu;   // no pending counts (a flow number is below flow_cap <= 2^32 - 1)

__device__ __forceinline__ void add_counts(bt_flow_tcp_rec* rec, uint32_t s, uint32_t f, uint32_t r) {
    if (s) atomicAdd(&rec->syn_packets, s);
    if (f) atomicAdd(&rec->fin_packets, f);
    if (r) atomicAdd(&rec->rst_packets, r);
}

}  // namespace

__global__ __launch_bounds__(kTcpThreads) void bt_flowtcp_update(FlowtcpArgs a) {
    __shared__ uint32_t red[kFtWaves][5];
    __shared__ uint32_t pend[kFtWaves][4];
    const uint32_t c = blockIdx.x, tid = threadIdx.x, lane = tid & 63u, wid = tid >> 6;
    uint32_t ntcp = 0, nsyn = 0, nfin = 0, nrst = 0, nbad = 0;   // wave-uniform
    uint32_t pid = kTcpNoFlow, ps = 0, pf = 0, pr = 0;           // wave-uniform: the counts of the last flow met, not yet added
    const uint32_t t0 = c * kFtChunkTiles + wid * kTcpWaveTiles;
    for (uint32_t k = 0; k < kTcpWaveTiles; ++k) {
        const uint32_t t = t0 + k;
        if (t >= a.ntiles) break;
        const uint32_t i = t * 64u + lane;
        const bool in = i < a.n;
        const uint32_t id = in ? a.flow_id[i] : BT_FLOW_ID_UNSELECTED;
        const bool mine = id < a.flow_cap;   // false at or past n
        nbad += (uint32_t)__popcll(__ballot(!mine && !flowtcp_is_sentinel(id)));
        if (__ballot(mine) == 0ull) continue;   // wave-uniform
        uint64_t off = 0;
        uint32_t len = 0;
        if (mine) frame_at(a, i, off, len);
        FlowLayers L;
        flow_layers(a, off, len, mine, L);
        const bool tcp = mine && L.l4 && L.proto == 6u;
        uint32_t T[1];
        fw_load_at<1>(a, off + L.o4 + 12u, tcp, T);   // TCP bytes 12 .. 15: data offset, flags, window
        const uint32_t fl = byte_of(T, 1);
        uint32_t dir = 0;
        if (a.bidir) {   // wave-uniform
            uint32_t w[9], nw;
            const uint32_t klass = flow_key_words(a, off, L, L.l4 && !a.l3_only, w, nw);
            dir = tcp ? flow_direction(klass, w) : 0u;
        }
        const bool syn = tcp && (fl & BT_TCPF_SYN) && !(fl & BT_TCPF_ACK), fin = tcp && (fl & BT_TCPF_FIN), rst = tcp && (fl & BT_TCPF_RST);
        ntcp += (uint32_t)__popcll(__ballot(tcp));
        nsyn += (uint32_t)__popcll(__ballot(syn));
        nfin += (uint32_t)__popcll(__ballot(fin));
        nrst += (uint32_t)__popcll(__ballot(rst));

        bt_flow_tcp_rec* const rec = a.tcp + (mine ? id : 0u);   // id < flow_cap
        uint32_t* const hot = reinterpret_cast<uint32_t*>(rec);   // flags[0] | flags[1] << 8 | pad << 16
        const uint32_t bits = tcp ? fl << (8u * dir) : 0u;
        const uint32_t have = tcp ? __hip_atomic_load(hot, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT) : 0u;
        const bool add = tcp && ((bits & ~have) || syn || fin || rst);
        const uint32_t my3 = (syn ? 1u : 0u) | (fin ? 2u : 0u) | (rst ? 4u : 0u);
        uint64_t todo = __ballot(add);
        for (uint32_t turn = 0; turn < 64u && todo; ++turn) {   // a turn clears at least its leader's bit
            const int leader = __ffsll((unsigned long long)todo) - 1;
            const uint32_t fo = (uint32_t)__shfl((int)id, leader);
            const bool in_turn = add && id == fo;
            const uint64_t same = __ballot(in_turn);
            uint32_t all = in_turn ? bits : 0u;
            if (same & (same - 1ull)) all = wave_or(all);   // more than one lane
            if (lane == (uint32_t)leader && (all & ~have)) atomicOr(hot, all);   // the leader's `have` is its flow's word
            // The counts wait in the wave: consecutive turns and tiles of one flow add once.
            uint32_t s, f, r;
            if (same & (same - 1ull)) {
                s = (uint32_t)__popcll(__ballot(in_turn && syn));
                f = (uint32_t)__popcll(__ballot(in_turn && fin));
                r = (uint32_t)__popcll(__ballot(in_turn && rst));
            } else {   // the leader alone: its own three bits, to every lane
                const uint32_t x = (uint32_t)__shfl((int)my3, leader);
                s = x & 1u; f = (x >> 1) & 1u; r = x >> 2;
            }
            if (s | f | r) {
                if (fo != pid) {
                    if (lane == 0 && pid != kTcpNoFlow) add_counts(a.tcp + pid, ps, pf, pr);   // pid < flow_cap
                    pid = fo; ps = 0; pf = 0; pr = 0;
                }
                ps += s; pf += f; pr += r;
            }
            todo &= ~same;
        }
    }
    if (lane == 0) {
        red[wid][0] = ntcp; red[wid][1] = nsyn; red[wid][2] = nfin; red[wid][3] = nrst; red[wid][4] = nbad;
        pend[wid][0] = pid; pend[wid][1] = ps; pend[wid][2] = pf; pend[wid][3] = pr;
    }
    __syncthreads();
    if (tid >= 64u && tid < 64u + kFtWaves) {   // what the waves still hold: one set of adds per distinct flow of the block
        const uint32_t v = tid - 64u, mine = pend[v][0];
        bool first = mine != kTcpNoFlow;
        for (uint32_t u = 0; u < v; ++u) first = first && pend[u][0] != mine;
        if (first) {
            uint32_t s = 0, f = 0, r = 0;
            for (uint32_t u = v; u < kFtWaves; ++u)
                if (pend[u][0] == mine) { s += pend[u][1]; f += pend[u][2]; r += pend[u][3]; }
            add_counts(a.tcp + mine, s, f, r);   // mine < flow_cap
        }
    }
    if (tid < 5u) {
        uint32_t sum = 0;
#pragma unroll
        for (uint32_t v = 0; v < kFtWaves; ++v) sum += red[v][tid];
        bt_flow_tcp_result* const res = a.result;
        uint32_t* const to = tid == 0 ? &res->tcp_packets : tid == 1 ? &res->syn_packets : tid == 2 ? &res->fin_packets
                             : tid == 3 ? &res->rst_packets : &res->bad_ids;
        if (sum) atomicAdd(to, sum);
    }
    if (c == 0 && tid == 5u) atomicAdd(&a.result->n, a.n);
}

int launch_flowtcp(const FlowtcpArgs& a, void* stream, void* timing_start, void* timing_stop) {
    if (a.n == 0 || a.nchunks == 0) return BT_OK;
    hipStream_t st = reinterpret_cast<hipStream_t>(stream);
    hipEvent_t e0 = reinterpret_cast<hipEvent_t>(timing_start), e1 = reinterpret_cast<hipEvent_t>(timing_stop);
    launch(bt_flowtcp_update, dim3(a.nchunks), dim3(kTcpThreads), 0, st, e0, e1, a);
    return hipGetLastError() == hipSuccess ? BT_OK : BT_E_INTERNAL;
}

}  // namespace bt
