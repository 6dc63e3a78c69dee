// bt_flowtab.hip — the flow table of a batch (bt_flow_table_device, include/beatrice_gpu.h): an
// exact group-by on the fan-out's flow key over a device-resident batch. Which flows are in the
// batch, each with its packets, bytes, first and last packet; and every packet's flow number.
//
// Six launches over the caller's scratch (bt_flowtab.h), lane = packet, one block of 8 waves per
// chunk of 256 tiles as bt_fanout_keys. No lane ever waits for another lane, wave or block:
// there is no spin, no flag and no look-back, and every loop has a bound in its head.
//   bt_flowtab_keys    the fan-out's layer walk and key (flow_key, bt_flow_walk.h: the one copy
//                      both use), the canonical direction when bidirectional (flow_canonical,
//                      same header), a probe hash of the key words and the class; an FtFlow per
//                      selected packet with a key (its key, and the sums of a flow that has this
//                      packet alone), an owner word per packet (a sentinel, or "pending"), the
//                      chunk's sums. The grid also sets the slots to empty, a share per block.
//   bt_flowtab_insert  open addressing, linear probing, at most `slots` steps. A slot is one word;
//                      it is claimed by a device-scope atomicCAS from empty to the packet's index,
//                      and the claiming packet's FtFlow is from then on the flow's entry: its key
//                      is the slot's key and its sums, which already hold the owner's own share,
//                      are the flow's. A lane that finds an owner compares its key with the
//                      owner's, which the previous kernel wrote. The other packets of the flow add
//                      themselves to the owner's entry: atomicMin(first), atomicMax(last), one
//                      64-bit atomicAdd over packets[2], atomicAdd(bytes[dir]), after the lanes of
//                      the tile that hit one flow have been combined (ballot peeling, as
//                      bt_tally's row_add). A batch of distinct flows does no atomic but the CAS.
//   bt_flowtab_firsts  packet i is the first of its flow when its owner's first == i: those bits
//                      as verdict-layout words, and their counts per wave, chunk and class.
//   bt_flowtab_join    one block: the exclusive scan of the chunks' flow counts, and *result.
//   bt_flowtab_rank    first packets: the flow's number (chunk start + wave start + popcount
//                      below) into the owner's entry, and flows[number] when it is below flow_cap.
//   bt_flowtab_emit    flow_id[i] from the packet's owner (only with out->flow_id).
// Why the outputs are the same from run to run although lanes race for slots: which slot a flow
// gets, and which of its packets owns it, varies; but a flow has exactly one slot (a claimed slot
// is never given up, and every packet of the flow walks the same probe sequence up to it), the
// entry's sums, minimum and maximum are commutative integer operations over the same set of
// packets whichever of them came first, and the flow's number is the rank of its first packet,
// which depends on the minima alone. The scratch holds the only values that vary. Across the
// XCDs' L2s: the kernels read only atomics' results and data written by earlier kernels.
#include "bt_flow_walk.h"
#include "bt_hip_launch.h"
#include "bt_wave.h"
#include "bt_flowtab.h"

namespace bt {

namespace {

constexpr uint32_t kFtThreads = kFtWaves * 64u;
constexpr uint32_t kFtWaveTiles = kFtChunkTiles / kFtWaves;

// The probe hash: a fixed mix of the class and the nine key words (zero past the class's length),
// nothing the caller supplies but the key bytes goes in.
__device__ __forceinline__ uint32_t probe_hash(uint32_t klass, const uint32_t (&w)[9]) {
    uint32_t h = 0x9E3779B9u * (klass + 1u);
#pragma unroll
    for (int d = 0; d < 9; ++d) {
        uint32_t x = w[d] * 0xCC9E2D51u;
        x = (x << 15) | (x >> 17);
        h ^= x * 0x1B873593u;
        h = ((h << 13) | (h >> 19)) * 5u + 0xE6546B64u;
    }
    h ^= h >> 16; h *= 0x85EBCA6Bu;
    h ^= h >> 13; h *= 0xC2B2AE35u;
    return h ^ (h >> 16);
}

__device__ __forceinline__ void key_load(const FtFlow* k, uint32_t (&v)[12]) {
    const u32x4* p = reinterpret_cast<const u32x4*>(k);
#pragma unroll
    for (int j = 0; j < 3; ++j) {
        const u32x4 t = p[j];
        v[4 * j] = t.x; v[4 * j + 1] = t.y; v[4 * j + 2] = t.z; v[4 * j + 3] = t.w;
    }
}

}  // namespace

// K1: keys, slot words, the chunk's sums; and the slots' initial state.
__global__ __launch_bounds__(kFtThreads) void bt_flowtab_keys(FlowtabArgs a) {
    __shared__ uint32_t red[kFtWaves][4];
    const uint32_t c = blockIdx.x, tid = threadIdx.x, lane = tid & 63u, wid = tid >> 6;
    slots_fill<kFtThreads>(a.tab, a.slots, kFtEmpty);
    if (c >= a.nchunks) return;   // a block that only initialises slots

    uint32_t nsel = 0, nnone = 0, bnone = 0, bkeyed = 0;   // nsel, nnone wave-uniform; the byte sums per lane
    const uint32_t t0 = c * kFtChunkTiles + wid * kFtWaveTiles;
    for (uint32_t k = 0; k < kFtWaveTiles; ++k) {
        const uint32_t t = t0 + k;
        if (t >= a.ntiles) break;
        const uint32_t i = t * 64u + lane;
        const bool in = i < a.n;
        const uint64_t word = a.select ? a.select[t] : ~0ull;
        const bool sel = in && ((word >> lane) & 1ull);
        uint64_t off = 0;
        uint32_t len = 0;
        if (sel) frame_at(a, i, off, len);
        uint32_t w[9], nw;
        const uint32_t klass = flow_key(a, off, len, sel, w, nw);
        const bool keyed = sel && klass != BT_FLOW_NONE;
        const uint32_t dir = a.bidir ? flow_canonical(klass, w) : 0u;
        const uint32_t blen = len > 0xFFFFu ? 0xFFFFu : len;
        if (in) a.pslot[i] = !sel ? BT_FLOW_ID_UNSELECTED : keyed ? kFtPending : BT_FLOW_ID_NONE;
        if (keyed) {
            u32x4* const p = reinterpret_cast<u32x4*>(a.keys + i);
            p[0] = u32x4{w[0], w[1], w[2], w[3]};
            p[1] = u32x4{w[4], w[5], w[6], w[7]};
            p[2] = u32x4{w[8], klass | dir << 8, probe_hash(klass, w), blen};
            p[3] = u32x4{i, i, dir ? 0u : 1u, dir};                                    // first, last, packets[2]
            p[4] = u32x4{dir ? 0u : blen, 0u, dir ? blen : 0u, 0u};                    // bytes[2]
        }
        nsel += (uint32_t)__popcll(__ballot(sel));
        nnone += (uint32_t)__popcll(__ballot(sel && !keyed));
        if (sel && !keyed) bnone += blen;    // 32 tiles of at most 65,535: below 2^21 per lane
        if (keyed) bkeyed += blen;
    }
    bnone = wave_sum(bnone);
    bkeyed = wave_sum(bkeyed);
    if (lane == 0) { red[wid][0] = nsel; red[wid][1] = nnone; red[wid][2] = bnone; red[wid][3] = bkeyed; }
    __syncthreads();
    if (tid < 4u) {
        uint32_t s = 0;
#pragma unroll
        for (uint32_t v = 0; v < kFtWaves; ++v) s += red[v][tid];
        FtPartial& p = a.parts[c];
        (tid == 0 ? p.n_selected : tid == 1 ? p.none_packets : tid == 2 ? p.none_bytes : p.keyed_bytes) = s;
    }
}

// K2: every pending packet finds or claims its flow's slot and adds itself to it.
__global__ __launch_bounds__(kFtThreads) void bt_flowtab_insert(FlowtabArgs a) {
    const uint32_t c = blockIdx.x, tid = threadIdx.x, lane = tid & 63u, wid = tid >> 6;
    const uint32_t mask = a.slots - 1u;
    const uint32_t t0 = c * kFtChunkTiles + wid * kFtWaveTiles;
    for (uint32_t k = 0; k < kFtWaveTiles; ++k) {
        const uint32_t t = t0 + k;
        if (t >= a.ntiles) break;
        const uint32_t i = t * 64u + lane;
        const bool act = i < a.n && a.pslot[i] == kFtPending;
        uint32_t mine[12];
#pragma unroll
        for (int j = 0; j < 12; ++j) mine[j] = 0u;
        if (act) key_load(a.keys + i, mine);
        const uint32_t dir = (mine[9] >> 8) & 1u, len = mine[11];
        uint32_t found = BT_FLOW_ID_OVERFLOW;   // the flow's owner packet
        if (act) {
            uint32_t s = mine[10] & mask;
            for (uint32_t probe = 0; probe < a.slots; ++probe) {   // every slot once, then overflow
                // A slot changes once, from empty to its final value: a value other than empty is
                // final wherever it is read from, and empty is confirmed by the CAS.
                uint32_t owner = __hip_atomic_load(&a.tab[s], __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
                if (owner == kFtEmpty) owner = atomicCAS(&a.tab[s], kFtEmpty, i);
                if (owner == kFtEmpty) { found = i; break; }   // claimed: this packet's entry is the flow's
                uint32_t other[12];
                key_load(a.keys + owner, other);   // written by bt_flowtab_keys
                bool same = (other[9] & 0xFFu) == (mine[9] & 0xFFu);
#pragma unroll
                for (int j = 0; j < 9; ++j) same = same && other[j] == mine[j];
                if (same) { found = owner; break; }
                s = (s + 1u) & mask;
            }
            a.pslot[i] = found;
        }
        // The lanes of the tile that hit one flow add themselves with one set of atomics; the
        // owner's own share is in its entry already (bt_flowtab_keys), so it stays out.
        const bool add = act && found != BT_FLOW_ID_OVERFLOW && found != i;
        uint64_t todo = __ballot(add);
        for (uint32_t turn = 0; turn < 64u && todo; ++turn) {   // a turn clears at least its leader's bit
            const int leader = __ffsll((unsigned long long)todo) - 1;
            const uint32_t ko = (uint32_t)__shfl((int)found, leader);
            const bool in_turn = add && found == ko;
            const uint64_t same = __ballot(in_turn);
            const uint64_t rev = __ballot(in_turn && dir);
            uint32_t b0 = in_turn && !dir ? len : 0u, b1 = in_turn && dir ? len : 0u;
            if (same & (same - 1ull)) {   // more than one lane: 64 lengths of at most 65,535 fit 32 bits
                b0 = wave_sum(b0);
                b1 = wave_sum(b1);
            }
            if (lane == (uint32_t)leader) {
                FtFlow& fl = a.keys[ko];
                atomicMin(&fl.first, t * 64u + (uint32_t)leader);                              // the lowest lane of the turn
                atomicMax(&fl.last, t * 64u + 63u - (uint32_t)__clzll((unsigned long long)same));   // the highest
                const uint32_t p1 = (uint32_t)__popcll(rev), p0 = (uint32_t)__popcll(same) - p1;
                atomicAdd(reinterpret_cast<unsigned long long*>(fl.packets), (unsigned long long)p1 << 32 | p0);
                if (p0) atomicAdd(reinterpret_cast<unsigned long long*>(&fl.bytes[0]), (unsigned long long)b0);
                if (p1) atomicAdd(reinterpret_cast<unsigned long long*>(&fl.bytes[1]), (unsigned long long)b1);
            }
            todo &= ~same;
        }
    }
}

// K3: the first packet of every flow, as verdict-layout words and counts.
__global__ __launch_bounds__(kFtThreads) void bt_flowtab_firsts(FlowtabArgs a) {
    __shared__ uint32_t red[kFtWaves][8];
    const uint32_t c = blockIdx.x, tid = threadIdx.x, lane = tid & 63u, wid = tid >> 6;
    uint32_t flows = 0, over = 0, kc[5] = {0u, 0u, 0u, 0u, 0u};   // wave-uniform
    const uint32_t t0 = c * kFtChunkTiles + wid * kFtWaveTiles;
    for (uint32_t k = 0; k < kFtWaveTiles; ++k) {
        const uint32_t t = t0 + k;
        if (t >= a.ntiles) break;
        const uint32_t i = t * 64u + lane;
        const uint32_t s = i < a.n ? a.pslot[i] : BT_FLOW_ID_UNSELECTED;   // the owner, below n, or a sentinel
        const bool first = s < kFtPending && a.keys[s].first == i;
        const uint32_t klass = first ? a.keys[i].meta & 0xFFu : 0u;
        const uint64_t word = __ballot(first);
        if (lane == 0) a.firstw[t] = word;
        flows += (uint32_t)__popcll(word);
        over += (uint32_t)__popcll(__ballot(s == BT_FLOW_ID_OVERFLOW));
#pragma unroll
        for (uint32_t j = 1; j < 5u; ++j) kc[j] += (uint32_t)__popcll(__ballot(first && klass == j));
    }
    if (lane == 0) {
        red[wid][0] = flows; red[wid][1] = over;
#pragma unroll
        for (uint32_t j = 0; j < 5u; ++j) red[wid][2 + j] = kc[j];
    }
    __syncthreads();
    FtPartial& p = a.parts[c];
    if (tid < kFtWaves) p.wflows[tid] = red[tid][0];
    if (tid >= 64u && tid < 71u) {
        const uint32_t j = tid - 64u;
        uint32_t sum = 0;
#pragma unroll
        for (uint32_t v = 0; v < kFtWaves; ++v) sum += red[v][j];
        if (j == 0) p.flows = sum;
        else if (j == 1) p.overflow = sum;
        else p.klass_flows[j - 2u] = sum;
    }
}

// K4: where every chunk's flows start, and *result.
__global__ __launch_bounds__(kFtJoinThreads) void bt_flowtab_join(FlowtabArgs a) {
    __shared__ uint64_t tot[12];
    const uint32_t tid = threadIdx.x, lane = tid & 63u, wid = tid >> 6;
    if (wid == 0) {
        uint32_t running = 0;
        for (uint32_t c0 = 0; c0 < a.nchunks; c0 += 64u) {
            const uint32_t c = c0 + lane;
            const bool in = c < a.nchunks;
            const uint32_t v = in ? a.parts[c].flows : 0u;
            uint32_t incl = v;
            for (int o = 1; o < 64; o <<= 1) {
                const uint32_t y = __shfl_up(incl, o);
                if (lane >= (uint32_t)o) incl += y;
            }
            if (in) a.parts[c].rel = running + incl - v;
            running += (uint32_t)__shfl((int)incl, 63);
        }
        if (lane == 0) tot[0] = running;
    } else if (wid < 11u) {   // wave 1 .. 10: one sum each
        uint64_t s = 0;
        for (uint32_t c = lane; c < a.nchunks; c += 64u) {
            const FtPartial& p = a.parts[c];
            s += wid == 1u ? p.n_selected : wid == 2u ? p.none_packets : wid == 3u ? p.none_bytes : wid == 4u ? p.keyed_bytes
                 : wid == 5u ? p.overflow : p.klass_flows[wid - 6u];
        }
        s = wave_sum64(s);
        if (lane == 0) tot[wid] = s;
    }
    __syncthreads();
    if (tid == 0) {
        bt_flow_table_result* const r = a.result;
        const uint32_t nf = (uint32_t)tot[0];
        r->n = a.n; r->n_selected = (uint32_t)tot[1]; r->n_flows = nf; r->n_written = nf < a.flow_cap ? nf : a.flow_cap;
        r->none_packets = (uint32_t)tot[2]; r->overflow_packets = (uint32_t)tot[5]; r->slots = a.slots; r->reserved = 0u;
#pragma unroll
        for (uint32_t j = 0; j < 5u; ++j) r->klass_flows[j] = (uint32_t)tot[6u + j];
        r->pad = 0u;
        r->none_bytes = tot[3]; r->keyed_bytes = tot[4];
    }
}

// K5: first packets number their flow and write its record.
__global__ __launch_bounds__(kFtThreads) void bt_flowtab_rank(FlowtabArgs a) {
    const uint32_t c = blockIdx.x, tid = threadIdx.x, lane = tid & 63u, wid = tid >> 6;
    const FtPartial& p = a.parts[c];
    uint32_t base = p.rel;
    for (uint32_t v = 0; v < wid; ++v) base += p.wflows[v];
    const uint64_t below = (1ull << lane) - 1ull;
    const uint32_t t0 = c * kFtChunkTiles + wid * kFtWaveTiles;
    for (uint32_t k = 0; k < kFtWaveTiles; ++k) {
        const uint32_t t = t0 + k;
        if (t >= a.ntiles) break;
        const uint64_t word = a.firstw[t];   // bits at or above n are 0
        if ((word >> lane) & 1ull) {
            const uint32_t i = t * 64u + lane, id = base + (uint32_t)__popcll(word & below);
            FtFlow& fl = a.keys[a.pslot[i]];   // a first packet has an owner; the owner's key is its own
            if (id < a.flow_cap) {
                uint32_t key[12];
                key_load(&fl, key);
                uint64_t* const o = reinterpret_cast<uint64_t*>(a.flows + id);   // 80 B = ten words
#pragma unroll
                for (int j = 0; j < 4; ++j) o[j] = (uint64_t)fw_be32(key[2 * j + 1]) << 32 | fw_be32(key[2 * j]);   // wire order
                o[4] = (uint64_t)(key[9] & 0xFFu) << 32 | fw_be32(key[8]);
                o[5] = (uint64_t)fl.last << 32 | i;
                o[6] = (uint64_t)fl.packets[1] << 32 | fl.packets[0];
                o[7] = fl.bytes[0];
                o[8] = fl.bytes[1];
                o[9] = 0ull;
            }
            fl.hash = id;   // the probe hash has served: bt_flowtab_emit reads the number here
        }
        base += (uint32_t)__popcll(word);
    }
}

// K6: every packet's flow number, or its sentinel.
__global__ __launch_bounds__(kFtThreads) void bt_flowtab_emit(FlowtabArgs a) {
    const uint32_t c = blockIdx.x, tid = threadIdx.x, lane = tid & 63u, wid = tid >> 6;
    const uint32_t t0 = c * kFtChunkTiles + wid * kFtWaveTiles;
    for (uint32_t k = 0; k < kFtWaveTiles; ++k) {
        const uint32_t t = t0 + k;
        if (t >= a.ntiles) break;
        const uint32_t i = t * 64u + lane;
        if (i < a.n) {
            const uint32_t s = a.pslot[i];
            a.flow_id[i] = s < kFtPending ? a.keys[s].hash : s;   // the owner's entry holds the flow's number
        }
    }
}

int launch_flowtab(const FlowtabArgs& a, void* stream, void* timing_start, void* timing_stop) {
    if (a.n == 0 || a.nchunks == 0) return BT_OK;
    hipStream_t st = reinterpret_cast<hipStream_t>(stream);
    hipEvent_t e0 = reinterpret_cast<hipEvent_t>(timing_start), e1 = reinterpret_cast<hipEvent_t>(timing_stop);
    // enough blocks to empty the slots when the table is large next to the batch: 64 slots a thread, at most 4,096
    const uint64_t init = ((uint64_t)a.slots + 64u * kFtThreads - 1u) / (64u * kFtThreads);
    const uint32_t grid = (uint32_t)(init > 4096u ? 4096u : init);
    launch(bt_flowtab_keys, dim3(grid > a.nchunks ? grid : a.nchunks), dim3(kFtThreads), 0, st, e0, nullptr, a);
    launch(bt_flowtab_insert, dim3(a.nchunks), dim3(kFtThreads), 0, st, nullptr, nullptr, a);
    launch(bt_flowtab_firsts, dim3(a.nchunks), dim3(kFtThreads), 0, st, nullptr, nullptr, a);
    launch(bt_flowtab_join, dim3(1), dim3(kFtJoinThreads), 0, st, nullptr, nullptr, a);
    launch(bt_flowtab_rank, dim3(a.nchunks), dim3(kFtThreads), 0, st, nullptr, a.flow_id ? nullptr : e1, a);
    if (a.flow_id) launch(bt_flowtab_emit, dim3(a.nchunks), dim3(kFtThreads), 0, st, nullptr, e1, a);
    return hipGetLastError() == hipSuccess ? BT_OK : BT_E_INTERNAL;
}

}  // namespace bt
