// bt_fanout.hip — the selected packets of a batch fanned out to K queues by RSS flow hash
// (bt_flow_fanout_device, include/beatrice_gpu.h): a stable K-way partition that stays on the
// device, so that a flow stays on one consumer and only each consumer's packets go to it.
//
// Three launches, in the shape of bt_tally_chunks / bt_tally_join (bt_tally.hip) and
// bt_pack_sums / bt_pack_copy (bt_pack.hip): no block waits for another one, there is no
// look-back, no spin and no global atomic, so every output is the same from run to run.
//   bt_fanout_keys     one block of 8 waves per chunk of 256 tiles (16,384 packets), lane =
//                      packet, wave w has tiles 32w .. 32w + 31 of the chunk. A lane walks its
//                      frame's layers (flow_key, bt_flow_walk.h, which the flow
//                      table and the TCP side table share) with two to four loads at the frame's own
//                      alignment: bytes 12..27 (EtherType, up to two tags, the IPv4 IHL byte),
//                      16 bytes from L3 + 4 (flags, protocol / next header, addresses), the
//                      rest of the IPv6 addresses, the ports. The Toeplitz hash of the key is
//                      taken either from 72 nibble tables in LDS (16 consecutive words each: a
//                      wave's lookups of one nibble hit 16 banks, never one twice) that the
//                      block builds from the key, or bit by bit with the key in SGPRs (the
//                      A/B). The queue byte comes from the indirection table in LDS. The K
//                      rows of select words come from ballot peeling (one turn per distinct
//                      queue of the tile, as bt_tally's row_add): lane q ends a tile holding
//                      queue q's word and keeps queue q's count; lengths go to a 64-bit LDS
//                      sum per queue.
//   bt_fanout_join     one block: wave per queue, an exclusive scan over the chunks' counts
//                      (queue-major, chunk-minor) into the workspace, the totals and *result.
//   bt_fanout_scatter  block c, wave w: lane q starts at where queue q's packets of the wave's
//                      tiles go; per tile the queue bytes are peeled again, a packet's rank
//                      among its queue's packets of the tile is a popcount below its lane.
// Lanes at or past n never load. A frame byte is read only below a.bytes (fan_read_end: inside
// the 16-B granules of [base, base + bytes)), and reads as zero at or past it.
#include "bt_flow_walk.h"
#include "bt_hip_launch.h"
#include "bt_wave.h"
#include "bt_fanout.h"

namespace bt {

namespace {

constexpr uint32_t kFanThreads = kFanWaves * 64u;
constexpr uint32_t kFanWaveTiles = kFanChunkTiles / kFanWaves;

// Toeplitz, MSB first. Words at or past nw are zero and add nothing; a word no lane of the wave
// has ends the loop.
template <bool Table>
__device__ __forceinline__ uint32_t toeplitz(const FanoutArgs& a, const uint32_t* tab, const uint32_t (&w)[9], uint32_t nw) {
    uint32_t h = 0;
#pragma unroll
    for (int d = 0; d < 9; ++d) {
        if (__ballot((uint32_t)d < nw) == 0ull) break;
        const uint32_t x = w[d];
        if (Table) {
#pragma unroll
            for (int j = 0; j < 8; ++j) h ^= tab[(8 * d + j) * 16 + ((x >> (28 - 4 * j)) & 15u)];
        } else {
            const uint64_t k64 = (uint64_t)a.key[d] << 32 | a.key[d + 1];   // wave-uniform: scalar registers
#pragma unroll
            for (int b = 0; b < 32; ++b)
                h ^= (uint32_t)((k64 << b) >> 32) & (uint32_t)(-(int32_t)((x >> (31 - b)) & 1u));
        }
    }
    return h;
}

}  // namespace

// K1: keys, hashes, queue bytes, select rows, one partial per chunk.
template <bool Table>
__global__ __launch_bounds__(kFanThreads) void bt_fanout_keys(FanoutArgs a) {
    __shared__ uint32_t tab[Table ? kFanNibbles * 16u : 1u];
    __shared__ uint32_t lkey[kFanKeyWords];
    __shared__ uint32_t lreta[kFanReta / 4];
    __shared__ unsigned long long lbytes[64];
    __shared__ uint32_t lcount[kFanWaves][64];
    __shared__ uint32_t lklass[kFanWaves][5];
    const uint32_t c = blockIdx.x, tid = threadIdx.x, lane = tid & 63u, wid = tid >> 6;
    if (tid == 0) {
#pragma unroll
        for (uint32_t k = 0; k < kFanKeyWords; ++k) lkey[k] = a.key[k];
#pragma unroll
        for (uint32_t k = 0; k < kFanReta / 4; ++k) lreta[k] = a.reta[k];
    }
    if (tid < 64u) lbytes[tid] = 0ull;
    __syncthreads();
    if (Table) {
        // table p, entry v: the XOR of the key windows of the set bits of nibble v at input bits 4p .. 4p + 3
        for (uint32_t e = tid; e < kFanNibbles * 16u; e += kFanThreads) {
            const uint32_t p = e >> 4, v = e & 15u;
            uint32_t t = 0;
#pragma unroll
            for (uint32_t m = 0; m < 4u; ++m) {
                const uint32_t bit = 4u * p + m, kd = bit >> 5, sh = bit & 31u;   // kd + 1 <= 9
                const uint32_t win = sh ? (lkey[kd] << sh) | (lkey[kd + 1] >> (32u - sh)) : lkey[kd];
                if ((v >> (3u - m)) & 1u) t ^= win;
            }
            tab[e] = t;
        }
        __syncthreads();
    }

    uint32_t cnt = 0;                       // lane q: queue q's selected packets of this wave's tiles
    uint32_t kc[5] = {0u, 0u, 0u, 0u, 0u};  // wave-uniform
    const uint32_t t0 = c * kFanChunkTiles + wid * kFanWaveTiles;
    for (uint32_t k = 0; k < kFanWaveTiles; ++k) {
        const uint32_t t = t0 + k;
        if (t >= a.ntiles) break;
        const uint32_t i = t * 64u + lane;
        const bool in = i < a.n;
        uint64_t off = 0;
        uint32_t len = 0;
        if (in) frame_at(a, i, off, len);
        uint32_t w[9], nw;
        const uint32_t klass = flow_key(a, off, len, in, w, nw);
        const uint32_t h = toeplitz<Table>(a, tab, w, nw);
        const uint32_t q = (lreta[(h & 127u) >> 2] >> (8u * (h & 3u))) & 0xFFu;
        const uint64_t word = a.select ? a.select[t] : ~0ull;
        const bool sel = in && ((word >> lane) & 1ull);
        const uint32_t qb = sel ? q : 0xFFu;
        if (in) {
            if (a.hash) a.hash[i] = h;
            a.queue[i] = (uint8_t)qb;
        }
        uint64_t mine = 0ull;               // lane q: queue q's select word of the tile
        uint64_t todo = __ballot(sel);
        while (todo) {                      // the same word in every lane: one turn per distinct queue
            const int leader = __ffsll((unsigned long long)todo) - 1;
            const uint32_t kq = (uint32_t)__shfl((int)qb, leader);
            const uint64_t same = __ballot(qb == kq);
            if (lane == kq) mine = same;
            todo &= ~same;
        }
        if (a.select_q && lane < a.queues) a.select_q[(uint64_t)lane * a.ntiles + t] = mine;
        cnt += (uint32_t)__popcll(mine);
        if (sel) atomicAdd(&lbytes[q], (unsigned long long)(len > 0xFFFFu ? 0xFFFFu : len));   // LDS
#pragma unroll
        for (uint32_t j = 0; j < 5u; ++j) kc[j] += (uint32_t)__popcll(__ballot(sel && klass == j));
    }
    FanoutPartial& p = a.parts[c];
    p.wcount[wid][lane] = cnt;
    lcount[wid][lane] = cnt;
    if (lane == 0) {
#pragma unroll
        for (uint32_t j = 0; j < 5u; ++j) lklass[wid][j] = kc[j];
    }
    __syncthreads();
    if (tid < 64u) {
        uint32_t s = 0;
#pragma unroll
        for (uint32_t v = 0; v < kFanWaves; ++v) s += lcount[v][tid];
        p.count[tid] = s;
        p.bytes[tid] = lbytes[tid];
    } else if (tid < 72u) {
        const uint32_t j = tid - 64u;
        uint32_t s = 0;
        if (j < 5u) {
#pragma unroll
            for (uint32_t v = 0; v < kFanWaves; ++v) s += lklass[v][j];
        }
        if (j < 5u) p.klass[j] = s;
        else p.pad[j - 5u] = 0u;
    }
}

// K2: where every chunk's packets of every queue go, and *result.
__global__ __launch_bounds__(kFanJoinThreads) void bt_fanout_join(FanoutArgs a) {
    constexpr uint32_t kWaves = kFanJoinThreads / 64u;
    __shared__ uint32_t tot[64];
    __shared__ uint64_t btot[64];
    __shared__ uint32_t ktot[5];
    const uint32_t tid = threadIdx.x, lane = tid & 63u, wid = tid >> 6;
    if (tid < 64u) { tot[tid] = 0u; btot[tid] = 0ull; }
    __syncthreads();
    if (wid == kWaves - 1u) {
#pragma unroll
        for (uint32_t j = 0; j < 5u; ++j) {
            uint32_t s = 0;
            for (uint32_t c = lane; c < a.nchunks; c += 64u) s += a.parts[c].klass[j];
            s = wave_sum(s);
            if (lane == 0) ktot[j] = s;
        }
    }
    for (uint32_t q = wid; q < a.queues; q += kWaves) {
        uint32_t running = 0;
        uint64_t bsum = 0;
        for (uint32_t c0 = 0; c0 < a.nchunks; c0 += 64u) {
            const uint32_t c = c0 + lane;
            const bool in = c < a.nchunks;
            const uint32_t v = in ? a.parts[c].count[q] : 0u;
            bsum += in ? a.parts[c].bytes[q] : 0ull;
            uint32_t incl = v;
            for (int o = 1; o < 64; o <<= 1) {
                const uint32_t y = __shfl_up(incl, o);
                if (lane >= (uint32_t)o) incl += y;
            }
            if (in) a.rel[c * 64u + q] = running + incl - v;
            running += (uint32_t)__shfl((int)incl, 63);
        }
        bsum = wave_sum64(bsum);
        if (lane == 0) { tot[q] = running; btot[q] = bsum; }
    }
    __syncthreads();
    bt_fanout_result* const r = a.result;
    if (tid < 65u) {
        uint32_t s = 0;
        for (uint32_t q = 0; q < tid; ++q) s += tot[q];   // queues at or past a.queues hold 0
        r->start[tid] = s;
        if (tid == 64u) { r->n = a.n; r->n_selected = s; r->pad0 = 0u; r->pad1 = 0u; }
    } else if (tid >= 128u && tid < 192u) {
        r->bytes[tid - 128u] = btot[tid - 128u];
    } else if (tid >= 192u && tid < 197u) {
        r->klass[tid - 192u] = ktot[tid - 192u];
    }
}

// K3: the selected packets' indices, grouped by queue, ascending inside a queue.
__global__ __launch_bounds__(kFanThreads) void bt_fanout_scatter(FanoutArgs a) {
    const uint32_t c = blockIdx.x, tid = threadIdx.x, lane = tid & 63u, wid = tid >> 6;
    uint32_t run = 0;   // lane q: where queue q's next packet of this wave's tiles goes
    if (lane < a.queues) {
        run = a.result->start[lane] + a.rel[c * 64u + lane];
        for (uint32_t v = 0; v < wid; ++v) run += a.parts[c].wcount[v][lane];
    }
    const uint64_t below = (1ull << lane) - 1ull;
    const uint32_t t0 = c * kFanChunkTiles + wid * kFanWaveTiles;
    for (uint32_t k = 0; k < kFanWaveTiles; ++k) {
        const uint32_t t = t0 + k;
        if (t >= a.ntiles) break;
        const uint32_t i = t * 64u + lane;
        const uint32_t qb = i < a.n ? (uint32_t)a.queue[i] : 0xFFu;
        uint64_t todo = __ballot(qb != 0xFFu);
        while (todo) {
            const int leader = __ffsll((unsigned long long)todo) - 1;
            const uint32_t kq = (uint32_t)__shfl((int)qb, leader);   // < queues: a lane that holds `run`
            const uint64_t same = __ballot(qb == kq);
            const uint32_t at = (uint32_t)__shfl((int)run, (int)kq);
            if (qb == kq) a.idx[at + (uint32_t)__popcll(same & below)] = i;
            if (lane == kq) run += (uint32_t)__popcll(same);
            todo &= ~same;
        }
    }
}

int launch_fanout(const FanoutArgs& a, void* stream, void* timing_start, void* timing_stop) {
    if (a.n == 0 || a.nchunks == 0) return BT_OK;
    hipStream_t st = reinterpret_cast<hipStream_t>(stream);
    hipEvent_t e0 = reinterpret_cast<hipEvent_t>(timing_start), e1 = reinterpret_cast<hipEvent_t>(timing_stop);
    if (a.table) launch(bt_fanout_keys<true>, dim3(a.nchunks), dim3(kFanThreads), 0, st, e0, nullptr, a);
    else launch(bt_fanout_keys<false>, dim3(a.nchunks), dim3(kFanThreads), 0, st, e0, nullptr, a);
    launch(bt_fanout_join, dim3(1), dim3(kFanJoinThreads), 0, st, nullptr, a.idx ? nullptr : e1, a);
    if (a.idx) launch(bt_fanout_scatter, dim3(a.nchunks), dim3(kFanThreads), 0, st, nullptr, e1, a);
    return hipGetLastError() == hipSuccess ? BT_OK : BT_E_INTERNAL;
}

}  // namespace bt
