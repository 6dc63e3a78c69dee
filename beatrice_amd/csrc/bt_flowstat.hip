// bt_flowstat.hip — the per-flow statistics side table (bt_flow_stat_update_device,
// include/beatrice_gpu.h) and the generic side-table move behind an expire
// (bt_flow_track_side_move_device).
//
// bt_flowstat_update: one launch, lane = packet, one block of 8 waves per chunk of 256 tiles as
// bt_flowtcp_update. A lane whose flow number is below flow_cap walks its frame's layers
// (bt_flow_walk.h); with a whole IP header it reads the first dword of that header (IHL, total
// length), a TCP packet bytes 12 .. 15 of its TCP header, and, when the table is bidirectional,
// the lane forms the key the table forms to find its direction. Every field of the record is an
// OR, a maximum (minima are stored complemented) or an integer sum. Per tile:
//   1. every contributing lane reads the words of its flow's record that it could raise (seen,
//      proto_max, the four TTL / length extremes of its direction and, for a handshake packet,
//      its stamp) with relaxed agent-scope atomic loads, all lanes at once, and decides whether it
//      would change any of them;
//   2. a lane that is the only one of its flow in the tile adds its own values with its own atomics,
//      all such lanes at once (who is alone: every lane writes its number into a byte of LDS picked
//      by its flow number, 256 bytes per wave; the lane whose number stays is the slot's winner, a
//      lane that finds another lane of its own flow there marks the slot, and a winner whose slot
//      is unmarked has no second lane of its flow in the tile, since one flow is one slot; lanes
//      that merely share a slot with another flow take the next step);
//   3. the other lanes are combined by flow (ballot peeling, one turn per distinct flow among them);
//      only a turn in which some lane would change a word reduces the ORs and maxima over its
//      lanes, and the first lane of each direction issues an atomic only where the combined value
//      exceeds what that lane read; the turn's sums (payload packets and bytes, length squares,
//      per direction) are reduced over its lanes, wave-uniform, and wait in the wave while the
//      next turns and tiles meet the same flow. They are added with one atomicAdd per non-zero
//      sum when another flow's sums come, or at the end of the block, where what the eight waves
//      still hold is combined through LDS first.
// Words only ever grow during the kernel, so a stale read can only cause a redundant atomic, never
// a missing one: a batch that is one flow costs a few atomics for its first tiles and six
// atomicAdds per block after, not ten per packet on one 128-byte record; a batch of distinct flows
// costs what it must, its three sums per packet, from 64 lanes at a time.
// No lane ever waits for another lane, wave or block: there is no spin, no flag and no look-back,
// and every loop has a bound in its head. Every output is an OR, a maximum or an integer sum over
// the same set of packets whatever the order, so it is the same from run to run.
//
// The move: bt_flowside_mark counts the BT_FLOW_ID_EXPIRED entries of remap per block of 256 flows
// and zeroes the scratch rows of the flows that stay, bt_flowside_scan (one block) turns the
// counts into starts, bt_flowside_move copies every record to its row of the scratch or of
// expired_side (a block decides its 256 destinations, then copies word by word with all threads),
// bt_flowside_back copies the scratch back and zeroes the rows behind it. All four read the
// expire's counts from its result on the device.
#include "bt_flow_walk.h"
#include "bt_hip_launch.h"
#include "bt_wave.h"
#include "bt_flowstat.h"

namespace bt {

namespace {

constexpr uint32_t kStThreads = kFtWaves * 64u;
constexpr uint32_t kStWaveTiles = kFtChunkTiles / kFtWaves;
constexpr uint32_t kStNoFlow = 0xFFFFFFFFu;   // no pending sums (a flow number is below flow_cap <= 2^32 - 1)

__device__ __forceinline__ uint32_t load32(const uint32_t* p) { return __hip_atomic_load(p, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT); }
__device__ __forceinline__ uint64_t load64(const uint64_t* p) { return __hip_atomic_load(p, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT); }

__device__ __forceinline__ void add64(uint64_t* p, uint64_t v) {
    atomicAdd(reinterpret_cast<unsigned long long*>(p), (unsigned long long)v);
}
__device__ __forceinline__ void max64(uint64_t* p, uint64_t v) {
    atomicMax(reinterpret_cast<unsigned long long*>(p), (unsigned long long)v);
}

// One flow's sums: payload packets c, payload bytes b and length squares q per direction.
__device__ __forceinline__ void add_sums(bt_flow_stat_rec* rec, uint32_t c0, uint32_t c1, uint64_t b0, uint64_t b1, uint64_t q0,
                                         uint64_t q1) {
    if (c0) atomicAdd(&rec->payload_packets[0], c0);
    if (c1) atomicAdd(&rec->payload_packets[1], c1);
    if (b0) add64(&rec->payload_bytes[0], b0);
    if (b1) add64(&rec->payload_bytes[1], b1);
    if (q0) add64(&rec->len_sq[0], q0);
    if (q1) add64(&rec->len_sq[1], q1);
}

}  // namespace

__global__ __launch_bounds__(kStThreads) void bt_flowstat_update(FlowstatArgs a) {
    __shared__ uint32_t red[kFtWaves][4];
    __shared__ uint32_t pend32[kFtWaves][3];
    __shared__ uint64_t pend64[kFtWaves][4];
    __shared__ uint8_t who[kFtWaves][256];
    const uint32_t c = blockIdx.x, tid = threadIdx.x, lane = tid & 63u, wid = tid >> 6;
    uint32_t nip = 0, nl4 = 0, ntcp = 0, nbad = 0;   // wave-uniform
    uint32_t pid = kStNoFlow, pc0 = 0, pc1 = 0;      // wave-uniform: the sums of the last flow met, not yet added
    uint64_t pb0 = 0, pb1 = 0, pq0 = 0, pq1 = 0;
    const uint32_t t0 = c * kFtChunkTiles + wid * kStWaveTiles;
    for (uint32_t k = 0; k < kStWaveTiles; ++k) {
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
        const bool ip = mine && (L.v4 || L.v6), l4 = ip && L.l4, tcp = l4 && L.proto == 6u;
        uint64_t todo = __ballot(ip);
        if (todo == 0ull) continue;   // wave-uniform
        nip += (uint32_t)__popcll(todo);
        nl4 += (uint32_t)__popcll(__ballot(l4));
        ntcp += (uint32_t)__popcll(__ballot(tcp));
        uint32_t H[1], T[1];
        fw_load_at<1>(a, off + L.o3, ip, H);            // L3 bytes 0 .. 3: version / IHL, TOS, total length
        fw_load_at<1>(a, off + L.o4 + 12u, tcp, T);     // TCP bytes 12 .. 15: data offset, flags, window
        uint32_t dir = 0;
        if (a.bidir) {   // wave-uniform
            uint32_t w[9], nw;
            const uint32_t klass = flow_key_words(a, off, L, L.l4 && !a.l3_only, w, nw);
            dir = ip ? flow_direction(klass, w) : 0u;
        }
        // what the packet contributes
        const uint32_t ihl = byte_of(H, 0) & 0xFu, fl = byte_of(T, 1);
        const uint32_t proto = ip ? L.proto : 0u;
        const uint32_t ttl = L.v4 ? byte_of(L.B, 4) : byte_of(L.B, 3);
        const uint32_t flen = len < 65535u ? len : 65535u;
        uint32_t bits = proto == 6u ? BT_FSEEN_TCP : proto == 17u ? BT_FSEEN_UDP : L.v4 && proto == 1u ? BT_FSEEN_ICMP
                        : L.v6 && proto == 58u ? BT_FSEEN_ICMP6 : BT_FSEEN_OTHER;
        if (L.v4 && (be16_of(L.B, 2) & 0x3FFFu)) bits |= BT_FSEEN_FRAGMENT;
        if (L.v4 && ihl > 5u) bits |= BT_FSEEN_IP_OPTIONS;
        if (L.o3 > 14u) bits |= BT_FSEEN_VLAN;
        if (l4) bits |= BT_FSEEN_L4;
        const uint32_t seen = ip ? bits << (16u * dir) : 0u;
        const int32_t ip_payload = L.v4 ? (int32_t)be16_of(H, 2) - (int32_t)(4u * ihl) : (int32_t)be16_of(L.B, 0);
        const int32_t hdr = tcp ? (int32_t)(4u * (byte_of(T, 0) >> 4)) : 8;
        const uint32_t pay = l4 && ip_payload > hdr ? (uint32_t)(ip_payload - hdr) : 0u;
        const uint64_t sq = ip ? (uint64_t)flen * flen : 0ull;
        const bool fsyn = fl & BT_TCPF_SYN, fack = fl & BT_TCPF_ACK, frst = fl & BT_TCPF_RST;
        const uint32_t kind = !tcp ? 3u : fsyn ? (fack ? 1u : 0u) : fack && !frst ? 2u : 3u;   // syn, synack, ack, none
        const uint32_t slot = 2u * kind + dir;   // of the six stamps behind syn_ts_c[0]
        const uint64_t tsv = kind < 3u ? ~(a.ts ? a.ts[i] : a.batch_ts) : 0ull;   // i < n: tcp

        // 1. what the record shows now
        bt_flow_stat_rec* const rec = a.stat + (ip ? id : 0u);   // id < flow_cap
        uint32_t* const r32 = reinterpret_cast<uint32_t*>(rec);
        uint64_t* const r64 = reinterpret_cast<uint64_t*>(rec);
        uint32_t hs = 0, hp = 0, h0 = 0, h1 = 0, h2 = 0, h3 = 0;
        if (ip) {
            hs = load32(r32);                 // seen
            hp = load32(r32 + 1);             // proto_max
            h0 = load32(r32 + 4 + dir);       // ttl_max[dir]
            h1 = load32(r32 + 6 + dir);       // ttl_min_c[dir]
            h2 = load32(r32 + 8 + dir);       // len_max[dir]
            h3 = load32(r32 + 10 + dir);      // len_min_c[dir]
        }
        uint64_t ht = ~0ull;
        if (kind < 3u) ht = load64(r64 + 10 + slot);   // its stamp; kind < 3: a TCP packet, id < flow_cap
        const bool stamp = tsv > ht;
        const bool chg = ip && ((seen & ~hs) || proto > hp || ttl > h0 || ~ttl > h1 || flen > h2 || ~flen > h3 || stamp);

        // 2. the lanes that are alone in their flow
        uint8_t* const my_slot = &who[wid][id & 255u];
        if (ip) *my_slot = (uint8_t)lane;
        wave_lds_sync();
        const uint32_t won = ip ? *my_slot : lane;                        // the lane whose number stayed in the slot
        const uint32_t won_id = (uint32_t)__shfl((int)id, (int)won);      // ... and its flow
        wave_lds_sync();
        if (ip && won != lane && won_id == id) *my_slot = 0xFFu;          // the winner's flow has a second lane
        wave_lds_sync();
        const bool alone = ip && won == lane && *my_slot == (uint8_t)lane;
        if (alone) {   // no other lane of the tile touches this record's sums: nothing to combine
            if (seen & ~hs) atomicOr(r32, seen);
            if (proto > hp) atomicMax(r32 + 1, proto);
            if (ttl > h0) atomicMax(r32 + 4 + dir, ttl);
            if (~ttl > h1) atomicMax(r32 + 6 + dir, ~ttl);
            if (flen > h2) atomicMax(r32 + 8 + dir, flen);
            if (~flen > h3) atomicMax(r32 + 10 + dir, ~flen);
            if (stamp) max64(r64 + 10 + slot, tsv);
            if (pay) {
                atomicAdd(r32 + 2 + dir, 1u);
                add64(r64 + 6 + dir, pay);
            }
            add64(r64 + 8 + dir, sq);
        }
        const bool peel = ip && !alone;
        todo = __ballot(peel);
        for (uint32_t turn = 0; turn < 64u && todo; ++turn) {   // a turn clears at least its leader's bit
            const int leader = __ffsll((unsigned long long)todo) - 1;
            const uint32_t fo = (uint32_t)__builtin_amdgcn_readlane((int)id, leader);
            const bool in_turn = peel && id == fo;
            const uint64_t same = __ballot(in_turn);
            const bool multi = (same & (same - 1ull)) != 0ull;   // more than one lane
            const uint64_t same1 = __ballot(in_turn && dir == 1u), same0 = same & ~same1;
            // 3a. ORs and maxima, only when a lane of the turn would change a word
            const uint64_t chg_t = __ballot(in_turn && chg);
            if (chg_t) {
                uint32_t sb = in_turn ? seen : 0u, pm = in_turn ? proto : 0u;
                if (multi) { sb = wave_or(sb); pm = wave_max32(pm); }
                if (lane == (uint32_t)leader) {   // the leader's hs and hp are its flow's words
                    if (sb & ~hs) atomicOr(r32, sb);
                    if (pm > hp) atomicMax(r32 + 1, pm);
                }
#pragma unroll
                for (uint32_t d = 0; d < 2u; ++d) {
                    const uint64_t sd = d ? same1 : same0;
                    if (!(chg_t & sd)) continue;   // wave-uniform
                    const bool me = in_turn && dir == d;
                    uint32_t v0 = me ? ttl : 0u, v1 = me ? ~ttl : 0u, v2 = me ? flen : 0u, v3 = me ? ~flen : 0u;
                    if (sd & (sd - 1ull)) { v0 = wave_max32(v0); v1 = wave_max32(v1); v2 = wave_max32(v2); v3 = wave_max32(v3); }
                    if (lane == (uint32_t)(__ffsll((unsigned long long)sd) - 1)) {   // its h0 .. h3 are direction d's words
                        if (v0 > h0) atomicMax(r32 + 4 + d, v0);
                        if (v1 > h1) atomicMax(r32 + 6 + d, v1);
                        if (v2 > h2) atomicMax(r32 + 8 + d, v2);
                        if (v3 > h3) atomicMax(r32 + 10 + d, v3);
                    }
                }
                if (__ballot(in_turn && stamp)) {   // wave-uniform: handshake stamps are rare
#pragma unroll
                    for (uint32_t s = 0; s < 6u; ++s) {
                        const bool me = in_turn && stamp && slot == s;
                        const uint64_t ws = __ballot(me);
                        if (!ws) continue;   // wave-uniform
                        uint64_t v = me ? tsv : 0ull;
                        if (ws & (ws - 1ull)) v = wave_max64(v);
                        if (lane == (uint32_t)(__ffsll((unsigned long long)ws) - 1)) max64(r64 + 10 + s, v);   // v >= its tsv > what it read
                    }
                }
            }
            // 3b. the sums wait in the wave: consecutive turns and tiles of one flow add once
            uint32_t c0, c1 = 0;
            uint64_t b0, b1 = 0, q0, q1 = 0;
            if (multi) {
                const bool me0 = in_turn && dir == 0u, me1 = in_turn && dir == 1u;
                c0 = (uint32_t)__popcll(__ballot(me0 && pay));
                b0 = wave_sum(me0 ? pay : 0u);   // 64 payloads below 2^16
                q0 = wave_sum64(me0 ? sq : 0ull);
                if (same1) {   // wave-uniform
                    c1 = (uint32_t)__popcll(__ballot(me1 && pay));
                    b1 = wave_sum(me1 ? pay : 0u);
                    q1 = wave_sum64(me1 ? sq : 0ull);
                }
            } else {   // the leader alone: its own values, to every lane
                const uint32_t xp = (uint32_t)__builtin_amdgcn_readlane((int)pay, leader);
                const uint32_t xl = (uint32_t)__builtin_amdgcn_readlane((int)flen, leader);
                const uint64_t xq = (uint64_t)xl * xl;
                const bool one = same1 != 0ull;
                c0 = !one && xp ? 1u : 0u; c1 = one && xp ? 1u : 0u;
                b0 = one ? 0u : xp; b1 = one ? xp : 0u;
                q0 = one ? 0ull : xq; q1 = one ? xq : 0ull;
            }
            if (fo != pid) {
                if (lane == 0 && pid != kStNoFlow) add_sums(a.stat + pid, pc0, pc1, pb0, pb1, pq0, pq1);   // pid < flow_cap
                pid = fo; pc0 = 0; pc1 = 0; pb0 = 0; pb1 = 0; pq0 = 0; pq1 = 0;
            }
            pc0 += c0; pc1 += c1; pb0 += b0; pb1 += b1; pq0 += q0; pq1 += q1;
            todo &= ~same;
        }
    }
    if (lane == 0) {
        red[wid][0] = nip; red[wid][1] = nl4; red[wid][2] = ntcp; red[wid][3] = nbad;
        pend32[wid][0] = pid; pend32[wid][1] = pc0; pend32[wid][2] = pc1;
        pend64[wid][0] = pb0; pend64[wid][1] = pb1; pend64[wid][2] = pq0; pend64[wid][3] = pq1;
    }
    __syncthreads();
    if (tid >= 64u && tid < 64u + kFtWaves) {   // what the waves still hold: one set of adds per distinct flow of the block
        const uint32_t v = tid - 64u, mine = pend32[v][0];
        bool first = mine != kStNoFlow;
        for (uint32_t u = 0; u < v; ++u) first = first && pend32[u][0] != mine;
        if (first) {
            uint32_t c0 = 0, c1 = 0;
            uint64_t b0 = 0, b1 = 0, q0 = 0, q1 = 0;
            for (uint32_t u = v; u < kFtWaves; ++u)
                if (pend32[u][0] == mine) {
                    c0 += pend32[u][1]; c1 += pend32[u][2];
                    b0 += pend64[u][0]; b1 += pend64[u][1]; q0 += pend64[u][2]; q1 += pend64[u][3];
                }
            add_sums(a.stat + mine, c0, c1, b0, b1, q0, q1);   // mine < flow_cap
        }
    }
    if (tid < 4u) {
        uint32_t sum = 0;
#pragma unroll
        for (uint32_t v = 0; v < kFtWaves; ++v) sum += red[v][tid];
        bt_flow_stat_result* const res = a.result;
        uint32_t* const to = tid == 0 ? &res->ip_packets : tid == 1 ? &res->l4_packets : tid == 2 ? &res->tcp_packets : &res->bad_ids;
        if (sum) atomicAdd(to, sum);
    }
    if (c == 0 && tid == 4u) atomicAdd(&a.result->n, a.n);
}

// ---- the side-table move -------------------------------------------------------------------

namespace {

struct SideCounts { uint32_t nb, nl; };   // flows before the expire and after it, both at most flow_cap

__device__ __forceinline__ SideCounts side_counts(const FlowsideArgs& a) {
    const uint32_t before = a.result->n_flows_before, live = a.result->n_flows;
    SideCounts s;
    s.nb = before < a.flow_cap ? before : a.flow_cap;
    s.nl = live < s.nb ? live : s.nb;
    return s;
}

}  // namespace

// S1: the leaving flows per block, as counts; zeros into the scratch rows of the flows that stay.
__global__ __launch_bounds__(kSideThreads) void bt_flowside_mark(FlowsideArgs a) {
    __shared__ uint32_t wn[kSideWaves];
    const SideCounts n = side_counts(a);
    const uint32_t f0 = blockIdx.x * kSideThreads;   // below flow_cap
    if (n.nl == n.nb || f0 >= n.nb) return;
    const uint32_t tid = threadIdx.x, lane = tid & 63u, wid = tid >> 6, f = f0 + tid;
    const bool leaves = f < n.nb && a.remap[f] == BT_FLOW_ID_EXPIRED;
    const uint32_t cnt = (uint32_t)__popcll(__ballot(leaves));
    if (lane == 0) wn[wid] = cnt;
    const uint64_t w0 = (uint64_t)f0 * a.rec_words;
    const uint64_t rows = n.nl > f0 ? (n.nl - f0 < kSideThreads ? n.nl - f0 : kSideThreads) : 0u, nw = rows * a.rec_words;
    for (uint64_t w = tid; w < nw; w += kSideThreads) a.tmp[w0 + w] = 0u;   // rows below n_flows <= flow_cap
    __syncthreads();
    if (tid == 0) {
        FsPart p{};
#pragma unroll
        for (uint32_t v = 0; v < kSideWaves; ++v) { p.wexp[v] = wn[v]; p.nexp += wn[v]; }
        a.parts[blockIdx.x] = p;
    }
}

// S2: where every block's leaving flows start.
__global__ __launch_bounds__(kSideJoinThreads) void bt_flowside_scan(FlowsideArgs a) {
    __shared__ uint32_t sh[kSideJoinThreads / 64u];
    const SideCounts n = side_counts(a);
    if (n.nl == n.nb) return;   // block-uniform
    const uint32_t tid = threadIdx.x;
    const uint32_t nparts = (n.nb + kSideThreads - 1u) / kSideThreads, per = (nparts + kSideJoinThreads - 1u) / kSideJoinThreads;
    const uint32_t lo = tid * per < nparts ? tid * per : nparts, hi = lo + per < nparts ? lo + per : nparts;
    uint32_t sum = 0;
    for (uint32_t p = lo; p < hi; ++p) sum += a.parts[p].nexp;
    uint32_t total = 0;
    uint32_t run = block_excl<kSideJoinThreads>(sum, sh, &total);
    for (uint32_t p = lo; p < hi; ++p) {
        a.parts[p].rel = run;
        run += a.parts[p].nexp;
    }
}

// S3: every record to its row of the scratch or of expired_side.
__global__ __launch_bounds__(kSideThreads) void bt_flowside_move(FlowsideArgs a) {
    __shared__ uint32_t* dst[kSideThreads];
    const SideCounts n = side_counts(a);
    const uint32_t f0 = blockIdx.x * kSideThreads;
    if (n.nl == n.nb || f0 >= n.nb) return;   // block-uniform
    const uint32_t tid = threadIdx.x, lane = tid & 63u, wid = tid >> 6, f = f0 + tid;
    const uint32_t to = f < n.nb ? a.remap[f] : 0u;
    const bool leaves = f < n.nb && to == BT_FLOW_ID_EXPIRED;
    const uint64_t word = __ballot(leaves);
    const FsPart& part = a.parts[blockIdx.x];
    uint32_t before = part.rel + (uint32_t)__popcll(word & ((1ull << lane) - 1ull));   // leaving flows below f
    for (uint32_t v = 0; v < wid; ++v) before += part.wexp[v];
    uint32_t* d = nullptr;
    if (leaves) {
        if (before < a.expired_cap) d = a.expired_side + (uint64_t)before * a.rec_words;   // expired_cap is 0 without expired_side
    } else if (f < n.nb && to < n.nl) {
        d = a.tmp + (uint64_t)to * a.rec_words;   // to < n_flows <= flow_cap
    }
    dst[tid] = d;
    __syncthreads();
    const uint32_t rows = n.nb - f0 < kSideThreads ? n.nb - f0 : kSideThreads, rw = a.rec_words, nw = rows * rw;   // at most 256 * 64
    const uint32_t* const src = a.side + (uint64_t)f0 * rw;
    for (uint32_t w = tid; w < nw; w += kSideThreads) {
        const uint32_t row = w / rw, j = w - row * rw;
        uint32_t* const p = dst[row];
        if (p) p[j] = src[w];
    }
}

// S4: the scratch back, zeros behind the flows that stay.
__global__ __launch_bounds__(kSideThreads) void bt_flowside_back(FlowsideArgs a) {
    const SideCounts n = side_counts(a);
    if (n.nl == n.nb) return;
    const uint64_t live = (uint64_t)n.nl * a.rec_words, all = (uint64_t)n.nb * a.rec_words;   // n_flows_before <= flow_cap
    const uint64_t step = (uint64_t)gridDim.x * kSideThreads;
    for (uint64_t w = (uint64_t)blockIdx.x * kSideThreads + threadIdx.x; w < all; w += step) a.side[w] = w < live ? a.tmp[w] : 0u;
}

int launch_flowstat(const FlowstatArgs& a, void* stream, void* timing_start, void* timing_stop) {
    if (a.n == 0 || a.nchunks == 0) return BT_OK;
    hipStream_t st = reinterpret_cast<hipStream_t>(stream);
    hipEvent_t e0 = reinterpret_cast<hipEvent_t>(timing_start), e1 = reinterpret_cast<hipEvent_t>(timing_stop);
    launch(bt_flowstat_update, dim3(a.nchunks), dim3(kStThreads), 0, st, e0, e1, a);
    return hipGetLastError() == hipSuccess ? BT_OK : BT_E_INTERNAL;
}

int launch_flowside(const FlowsideArgs& a, void* stream) {
    if (a.flow_cap == 0) return BT_OK;
    hipStream_t st = reinterpret_cast<hipStream_t>(stream);
    const uint32_t grid = (uint32_t)(((uint64_t)a.flow_cap + kSideThreads - 1u) / kSideThreads);   // flow_cap < 2^32
    const uint64_t words = (uint64_t)a.flow_cap * a.rec_words, wblocks = (words + kSideThreads - 1u) / kSideThreads;
    launch(bt_flowside_mark, dim3(grid), dim3(kSideThreads), 0, st, nullptr, nullptr, a);
    launch(bt_flowside_scan, dim3(1), dim3(kSideJoinThreads), 0, st, nullptr, nullptr, a);
    launch(bt_flowside_move, dim3(grid), dim3(kSideThreads), 0, st, nullptr, nullptr, a);
    launch(bt_flowside_back, dim3((uint32_t)(wblocks > 4096u ? 4096u : wblocks)), dim3(kSideThreads), 0, st, nullptr, nullptr, a);
    return hipGetLastError() == hipSuccess ? BT_OK : BT_E_INTERNAL;
}

}  // namespace bt
