// bt_flowmark.hip — the per-flow mark side table (bt_flow_mark_update_device,
// include/beatrice_gpu.h) and the selection built from it (bt_flow_mark_select_device).
//
// bt_flowmark_update: one launch, lane = packet, one block of 8 waves per chunk of 256 tiles as
// bt_flowtcp_update / bt_flowstat_update. A wave loads the hit words of its 32 tiles with one
// load, one word per lane, and is done when all are zero; a tile's word goes to every lane by a
// readlane, and a tile whose word is zero loads nothing more. Only hit lanes load their flow
// number, only hit lanes with a number below flow_cap their length (a descriptor, never a frame
// byte) and their timestamp: the kernel's traffic follows the hits, not n. Per tile with a hit:
//   1. every contributing lane reads marks and the two stamps of its flow's record with relaxed
//      agent-scope atomic loads, all lanes at once, and decides whether it would raise any;
//   2. a lane that is the only one of its flow in the tile (wave_alone, bt_wave.h) goes by itself,
//      all such lanes at once: an atomic for marks and for each stamp only where its value exceeds
//      what it read, and its two sums;
//   3. the other lanes are combined by flow (ballot peeling, one turn per distinct flow among
//      them): only a turn in which some lane would raise a word reduces the maxima over its lanes,
//      and its first lane issues an atomic only where the combined value exceeds what that lane
//      read; the turn's sums (hit packets, hit bytes) are reduced over its lanes, wave-uniform, and
//      wait in the wave while the next turns and tiles meet the same flow. They are added with one
//      atomicAdd each when another flow's sums come, or at the end of the block, where what the
//      eight waves still hold is combined through LDS first.
// Words only ever grow during the kernel, so a stale read can only cause a redundant atomic, never
// a missing one: a batch that is one flow costs a few atomics for its first tiles and two
// atomicAdds per block after. new_marked_flows is exact: the atomicOr that finds a bit of the mark
// missing in the value it replaces is the only one of the call to do so for its flow, since every
// bit is there after it, and a lane skips that atomicOr only when it has read every bit set, by
// this call or before it.
// No lane ever waits for another lane, wave or block: there is no spin, no flag and no look-back,
// and every loop has a bound in its head. Every output is an OR, a maximum or an integer sum over
// the same set of packets whatever the order, so it is the same from run to run.
//
// bt_flowmark_select: lane = packet, the same chunks. flow_id is loaded coalesced, lanes with a
// number below flow_cap gather the 4 bytes of marks, a ballot forms the tile's word, lane 0
// combines it with the tile's base word and stores it (the last tile without its bits at or above
// n). A tile's base word is read by the wave that writes its out word, before it: base may be out.
// Counts go by wave popcounts, then block, then one add per block.
#include "bt_hip_launch.h"
#include "bt_wave.h"
#include "bt_flowmark.h"

namespace bt {

namespace {

constexpr uint32_t kMkThreads = kFtWaves * 64u;
constexpr uint32_t kMkWaveTiles = kFtChunkTiles / kFtWaves;
constexpr uint32_t kMkNoFlow = 0xFFFFFFFFu;   // no pending sums (a flow number is below flow_cap <= 2^32 - 1)
static_assert(kMkWaveTiles <= 64u, "one hit word per lane");

__device__ __forceinline__ uint32_t mk_load32(const uint32_t* p) { return __hip_atomic_load(p, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT); }
__device__ __forceinline__ uint64_t mk_load64(const uint64_t* p) { return __hip_atomic_load(p, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT); }
__device__ __forceinline__ void mk_add64(uint64_t* p, uint64_t v) { atomicAdd(reinterpret_cast<unsigned long long*>(p), (unsigned long long)v); }
__device__ __forceinline__ void mk_max64(uint64_t* p, uint64_t v) { atomicMax(reinterpret_cast<unsigned long long*>(p), (unsigned long long)v); }

// The word of lane `src` (wave-uniform) to every lane.
__device__ __forceinline__ uint64_t mk_word_of(uint64_t v, uint32_t src) {
    const uint32_t lo = (uint32_t)__builtin_amdgcn_readlane((int)(uint32_t)v, (int)src);
    const uint32_t hi = (uint32_t)__builtin_amdgcn_readlane((int)(uint32_t)(v >> 32), (int)src);
    return ((uint64_t)hi << 32) | lo;
}

// The bits of tile t below n: all 64, or n % 64 of the last tile.
__device__ __forceinline__ uint64_t mk_valid(uint32_t t, uint32_t n) {
    const uint32_t left = n - t * 64u;   // t < ntiles: at least 1
    return left >= 64u ? ~0ull : (1ull << left) - 1ull;
}

}  // namespace

__global__ __launch_bounds__(kMkThreads) void bt_flowmark_update(FlowmarkArgs a) {
    __shared__ uint32_t red[kFtWaves][5];
    __shared__ uint32_t pend32[kFtWaves][2];
    __shared__ uint64_t pend64[kFtWaves];
    __shared__ uint8_t who[kFtWaves][256];
    const uint32_t c = blockIdx.x, tid = threadIdx.x, lane = tid & 63u, wid = tid >> 6;
    uint32_t nhit = 0, nmarked = 0, nunkeyed = 0, nbad = 0, nnew = 0;   // wave-uniform
    uint32_t pid = kMkNoFlow, pc = 0;                                   // wave-uniform: the sums of the last flow met, not yet added
    uint64_t pb = 0;
    const uint32_t t0 = c * kFtChunkTiles + wid * kMkWaveTiles;
    // the wave's hit words, lane k its tile k's; zero past the batch
    uint64_t words = 0;
    if (lane < kMkWaveTiles && t0 + lane < a.ntiles) words = (a.hit ? a.hit[t0 + lane] : ~0ull) & mk_valid(t0 + lane, a.n);
    const uint64_t tiles = __ballot(words != 0ull);   // bit k: tile k has a hit
    for (uint32_t k = 0; k < kMkWaveTiles; ++k) {
        if (!((tiles >> k) & 1ull)) continue;   // wave-uniform
        const uint32_t t = t0 + k;              // below ntiles: its word is not zero
        const uint64_t hw = mk_word_of(words, k);
        nhit += (uint32_t)__popcll(hw);
        const uint32_t i = t * 64u + lane;
        const bool hit = (hw >> lane) & 1ull;   // false at or past n
        const uint32_t id = hit ? a.flow_id[i] : BT_FLOW_ID_UNSELECTED;
        const bool mine = hit && id < a.flow_cap;
        const bool sentinel = hit && flowtcp_is_sentinel(id);
        nunkeyed += (uint32_t)__popcll(__ballot(sentinel));
        nbad += (uint32_t)__popcll(__ballot(hit && !mine && !sentinel));
        const uint64_t mball = __ballot(mine);
        if (mball == 0ull) continue;   // wave-uniform
        nmarked += (uint32_t)__popcll(mball);
        uint64_t off = 0;
        uint32_t len = 0;
        if (mine) frame_at(a, i, off, len);
        const uint32_t flen = len < 65535u ? len : 65535u;
        const uint64_t ts = mine ? (a.ts ? a.ts[i] : a.batch_ts) : 0ull;
        const uint64_t tsc = mine ? ~ts : 0ull;

        // 1. what the record shows now
        bt_flow_mark_rec* const rec = a.table + (mine ? id : 0u);   // id < flow_cap
        uint32_t hm = 0;
        uint64_t hf = 0, hl = 0;
        if (mine) {
            hm = mk_load32(&rec->marks);
            hf = mk_load64(&rec->first_hit_ts_c);
            hl = mk_load64(&rec->last_hit_ts);
        }
        const bool lacks = mine && (a.mark & ~hm) != 0u;
        const bool chg = mine && (lacks || tsc > hf || ts > hl);

        // 2. the lanes that are alone in their flow
        const bool alone = wave_alone(who[wid], mine, id, lane);
        bool fresh = false;   // this lane's atomicOr found a bit of the mark missing
        if (alone) {   // no other lane of the tile touches this record: nothing to combine
            if (lacks) fresh = (atomicOr(&rec->marks, a.mark) & a.mark) != a.mark;
            if (tsc > hf) mk_max64(&rec->first_hit_ts_c, tsc);
            if (ts > hl) mk_max64(&rec->last_hit_ts, ts);
            atomicAdd(&rec->hit_packets, 1u);
            mk_add64(&rec->hit_bytes, flen);
        }
        // 3. the others, a turn per flow
        const bool peel = mine && !alone;
        uint64_t todo = __ballot(peel);
        for (uint32_t turn = 0; turn < 64u && todo; ++turn) {   // a turn clears at least its leader's bit
            const int leader = __ffsll((unsigned long long)todo) - 1;
            const uint32_t fo = (uint32_t)__builtin_amdgcn_readlane((int)id, leader);
            const bool in_turn = peel && id == fo;
            const uint64_t same = __ballot(in_turn);
            const bool multi = (same & (same - 1ull)) != 0ull;   // more than one lane
            if (__ballot(in_turn && chg)) {   // wave-uniform
                uint64_t vf = in_turn ? tsc : 0ull, vl = in_turn ? ts : 0ull;
                if (multi) { vf = wave_max64(vf); vl = wave_max64(vl); }
                if (lane == (uint32_t)leader) {   // the leader's hm, hf and hl are its flow's words
                    if (lacks) fresh = (atomicOr(&rec->marks, a.mark) & a.mark) != a.mark;
                    if (vf > hf) mk_max64(&rec->first_hit_ts_c, vf);
                    if (vl > hl) mk_max64(&rec->last_hit_ts, vl);
                }
            }
            const uint32_t cnt = (uint32_t)__popcll(same);
            const uint32_t bytes = multi ? wave_sum(in_turn ? flen : 0u)   // 64 lengths below 2^16
                                         : (uint32_t)__builtin_amdgcn_readlane((int)flen, leader);
            if (fo != pid) {
                if (lane == 0 && pid != kMkNoFlow) {   // pid < flow_cap
                    atomicAdd(&a.table[pid].hit_packets, pc);
                    mk_add64(&a.table[pid].hit_bytes, pb);
                }
                pid = fo; pc = 0; pb = 0;
            }
            pc += cnt; pb += bytes;
            todo &= ~same;
        }
        nnew += (uint32_t)__popcll(__ballot(fresh));
    }
    if (lane == 0) {
        red[wid][0] = nhit; red[wid][1] = nmarked; red[wid][2] = nunkeyed; red[wid][3] = nbad; red[wid][4] = nnew;
        pend32[wid][0] = pid; pend32[wid][1] = pc;
        pend64[wid] = pb;
    }
    __syncthreads();
    if (tid >= 64u && tid < 64u + kFtWaves) {   // what the waves still hold: one pair of adds per distinct flow of the block
        const uint32_t v = tid - 64u, mine = pend32[v][0];
        bool first = mine != kMkNoFlow;
        for (uint32_t u = 0; u < v; ++u) first = first && pend32[u][0] != mine;
        if (first) {
            uint32_t cnt = 0;
            uint64_t bytes = 0;
            for (uint32_t u = v; u < kFtWaves; ++u)
                if (pend32[u][0] == mine) { cnt += pend32[u][1]; bytes += pend64[u]; }
            atomicAdd(&a.table[mine].hit_packets, cnt);   // mine < flow_cap
            mk_add64(&a.table[mine].hit_bytes, bytes);
        }
    }
    if (tid < 5u) {
        uint32_t sum = 0;
#pragma unroll
        for (uint32_t v = 0; v < kFtWaves; ++v) sum += red[v][tid];
        bt_flow_mark_result* const res = a.result;
        uint32_t* const to = tid == 0 ? &res->hit_packets : tid == 1 ? &res->marked_packets : tid == 2 ? &res->unkeyed_hits
                             : tid == 3 ? &res->bad_ids : &res->new_marked_flows;
        if (sum) atomicAdd(to, sum);
    }
    if (c == 0 && tid == 5u) atomicAdd(&a.result->n, a.n);
}

__global__ __launch_bounds__(kMkThreads) void bt_flowmark_select(FlowmarkSelArgs a) {
    __shared__ uint32_t red[kFtWaves][3];
    const uint32_t c = blockIdx.x, tid = threadIdx.x, lane = tid & 63u, wid = tid >> 6;
    uint32_t nmarked = 0, nout = 0, nbad = 0;   // wave-uniform
    const uint32_t t0 = c * kFtChunkTiles + wid * kMkWaveTiles;
    const uint32_t mine = t0 < a.ntiles ? (a.ntiles - t0 < kMkWaveTiles ? a.ntiles - t0 : kMkWaveTiles) : 0u;   // the wave's tiles
    for (uint32_t k = 0; k < mine; ++k) {
        const uint32_t t = t0 + k;
        const uint32_t i = t * 64u + lane;
        const bool in = i < a.n;
        const uint32_t id = in ? a.flow_id[i] : BT_FLOW_ID_UNSELECTED;
        const bool keyed = id < a.flow_cap;   // false at or past n
        uint32_t got = 0;
        if (keyed) got = a.table[id].marks & a.mask;
        const uint64_t m = __ballot(a.all_bits ? got == a.mask : got != 0u);   // mask != 0: got == 0 is never a match
        nbad += (uint32_t)__popcll(__ballot(!keyed && !flowtcp_is_sentinel(id)));
        const uint64_t bw = a.base ? a.base[t] : 0ull;   // wave-uniform, before the store below: base may be out
        const uint64_t o = (a.op == BT_FLOW_MARK_SET ? m : a.op == BT_FLOW_MARK_AND ? (bw & m) : a.op == BT_FLOW_MARK_OR ? (bw | m) : (bw & ~m)) &
                           mk_valid(t, a.n);
        if (lane == 0) a.out[t] = o;
        nmarked += (uint32_t)__popcll(m);
        nout += (uint32_t)__popcll(o);
    }
    if (lane == 0) { red[wid][0] = nmarked; red[wid][1] = nout; red[wid][2] = nbad; }
    __syncthreads();
    if (tid < 3u) {
        uint32_t sum = 0;
#pragma unroll
        for (uint32_t v = 0; v < kFtWaves; ++v) sum += red[v][tid];
        bt_flow_mark_select_result* const res = a.result;
        uint32_t* const to = tid == 0 ? &res->n_marked : tid == 1 ? &res->n_out : &res->bad_ids;
        if (sum) atomicAdd(to, sum);
    }
    if (c == 0 && tid == 3u) atomicAdd(&a.result->n, a.n);
}

int launch_flowmark(const FlowmarkArgs& a, void* stream, void* timing_start, void* timing_stop) {
    if (a.n == 0 || a.nchunks == 0) return BT_OK;
    hipStream_t st = reinterpret_cast<hipStream_t>(stream);
    hipEvent_t e0 = reinterpret_cast<hipEvent_t>(timing_start), e1 = reinterpret_cast<hipEvent_t>(timing_stop);
    launch(bt_flowmark_update, dim3(a.nchunks), dim3(kMkThreads), 0, st, e0, e1, a);
    return hipGetLastError() == hipSuccess ? BT_OK : BT_E_INTERNAL;
}

int launch_flowmark_select(const FlowmarkSelArgs& a, void* stream, void* timing_start, void* timing_stop) {
    if (a.n == 0 || a.nchunks == 0) return BT_OK;
    hipStream_t st = reinterpret_cast<hipStream_t>(stream);
    hipEvent_t e0 = reinterpret_cast<hipEvent_t>(timing_start), e1 = reinterpret_cast<hipEvent_t>(timing_stop);
    launch(bt_flowmark_select, dim3(a.nchunks), dim3(kMkThreads), 0, st, e0, e1, a);
    return hipGetLastError() == hipSuccess ? BT_OK : BT_E_INTERNAL;
}

}  // namespace bt
