// bt_flowseq.hip — a packet's position inside its flow and the per-flow cut-off built from it
// (bt_flow_seq_device, include/beatrice_gpu.h).
//
// A position depends on order, so no commutative atomic gives it. The numbered packets are
// compacted, sorted by flow number with a stable radix sort, and scanned segment by segment: the
// chunked family's shape throughout (per-chunk partials, a one-block join, a write). No lane, wave
// or block waits for another: no spin, no flag, no look-back; every loop has its bound in its head;
// every output is an integer sum, an OR or a value with one writer, the same from run to run.
//   bt_flowseq_class    block = chunk of 256 tiles, lane = packet. A wave loads the select words
//                       of its 32 tiles at once, one per lane (so out_select may be select), loads
//                       the flow number of selected packets only, stores the tile's word of
//                       numbered packets into the scratch, writes NONE into seq / byte_off of
//                       every packet that is not numbered, and starts the tile's out_select word:
//                       the kept sentinels, or zero. Counts per wave and chunk, tallies to *result.
//   bt_flowseq_join     one block: exclusive scan of the chunks' counts; the total m.
//   bt_flowseq_compact  the (flow number, index) pairs of the numbered packets, in packet order.
//   per pass of 8 bits, low digit first (ceil(bits(flow_cap - 1) / 8) passes):
//   bt_flowseq_digits   block = chunk of the list, wave = unit of 32 tiles. The lanes of a tile
//                       with the same digit find each other by eight ballots; the first of them
//                       adds their number to the wave's own 256 LDS counters.
//   bt_flowseq_djoin    one block: wave per digit, an exclusive scan over the chunks, then over
//                       the digits.
//   bt_flowseq_scatter  a wave's 256 running positions in LDS; a pair goes to its digit's position
//                       plus its rank among the tile's lanes of that digit: stable.
//   bt_flowseq_scan<M>  wave = unit, no block-wide step. Heads are where the key changes. Per tile
//                       a lane's packets-before is its distance to the nearest head at or below
//                       it (ballots), its bytes-before a difference of two prefix sums; what no
//                       head of the unit precedes adds the unit's carry.
//                         Carry: gathers the lengths (descriptors, never frame bytes), keeps them
//                                in list order, leaves the unit's sums since its last head;
//                         Emit:  adds table[key], writes seq, byte_off at the packet's index and
//                                ORs its keep bit into out_select (atomicOr into words that
//                                bt_flowseq_class initialised: an OR, so deterministic);
//                         Commit: the last lane of each segment holds the flow's totals and is the
//                                only lane that touches table[key] in this launch: no atomic, and
//                                no race with Emit's reads, which are a launch earlier.
//   bt_flowseq_sjoin    one block: the segmented exclusive scan over the units' carries.
// Blocks and waves whose part of the list lies at or past m end at once: the grid follows n, the
// work follows the selection.
#include "bt_hip_launch.h"
#include "bt_wave.h"
#include "bt_flowseq.h"

namespace bt {

namespace {

constexpr uint32_t kFsThreads = kFtWaves * 64u;
static_assert(kFsUnitTiles <= 64u, "one select word per lane");
static_assert(kFsDigits % 64u == 0u, "digits by lane");

enum FsMode { kFsCarry = 0, kFsEmit = 1, kFsCommit = 2 };

__device__ __forceinline__ uint64_t fs_word_of(uint64_t v, uint32_t src) {   // the word of lane `src` (wave-uniform) to every lane
    const uint32_t lo = (uint32_t)__builtin_amdgcn_readlane((int)(uint32_t)v, (int)src);
    const uint32_t hi = (uint32_t)__builtin_amdgcn_readlane((int)(uint32_t)(v >> 32), (int)src);
    return ((uint64_t)hi << 32) | lo;
}

__device__ __forceinline__ uint64_t fs_valid(uint32_t t, uint32_t n) {   // the bits of tile t below n; t < ntiles
    const uint32_t left = n - t * 64u;
    return left >= 64u ? ~0ull : (1ull << left) - 1ull;
}

__device__ __forceinline__ void fs_add64(uint64_t* p, uint64_t v) { atomicAdd(reinterpret_cast<unsigned long long*>(p), (unsigned long long)v); }

// The lanes that are `in` with this lane's digit (of an `in` lane; anything otherwise).
__device__ __forceinline__ uint64_t fs_match(uint32_t d, bool in) {
    uint64_t same = __ballot(in);
#pragma unroll
    for (uint32_t b = 0; b < kFsDigitBits; ++b) {
        const bool bit = (d >> b) & 1u;
        const uint64_t bal = __ballot(bit);
        same &= bit ? bal : ~bal;
    }
    return same;
}

__device__ __forceinline__ uint32_t fs_excl(uint32_t v, uint32_t lane, uint32_t* total) {   // exclusive prefix sum over the wave
    uint32_t incl = v;
    for (int o = 1; o < 64; o <<= 1) {
        const uint32_t y = __shfl_up(incl, o);
        if (lane >= (uint32_t)o) incl += y;
    }
    *total = (uint32_t)__builtin_amdgcn_readlane((int)incl, 63);
    return incl - v;
}

// a then b of a segmented sum: b's own sums if b holds a head, else both
__device__ __forceinline__ FsCarry fs_join(const FsCarry& x, const FsCarry& y) {
    FsCarry r;
    r.head = x.head | y.head;
    r.cnt = y.head ? y.cnt : x.cnt + y.cnt;
    r.bytes = y.head ? y.bytes : x.bytes + y.bytes;
    return r;
}

__device__ __forceinline__ FsCarry fs_shfl_up(const FsCarry& x, int o) {
    FsCarry r;
    r.head = __shfl_up(x.head, o);
    r.cnt = __shfl_up(x.cnt, o);
    r.bytes = ((uint64_t)__shfl_up((uint32_t)(x.bytes >> 32), o) << 32) | __shfl_up((uint32_t)x.bytes, o);
    return r;
}

}  // namespace

__global__ __launch_bounds__(kFsThreads) void bt_flowseq_class(FlowseqArgs a) {
    __shared__ uint32_t red[kFtWaves][4];
    const uint32_t c = blockIdx.x, tid = threadIdx.x, lane = tid & 63u, wid = tid >> 6;
    uint32_t nsel = 0, nnum = 0, nunk = 0, nbad = 0;   // wave-uniform
    const uint32_t t0 = c * kFtChunkTiles + wid * kFsUnitTiles;
    // the wave's select words, lane k its tile k's, before any out_select word is written; zero past the batch
    uint64_t words = 0;
    if (lane < kFsUnitTiles && t0 + lane < a.ntiles) words = (a.select ? a.select[t0 + lane] : ~0ull) & fs_valid(t0 + lane, a.n);
    for (uint32_t k = 0; k < kFsUnitTiles && t0 + k < a.ntiles; ++k) {
        const uint32_t t = t0 + k;
        const uint64_t sw = fs_word_of(words, k);
        const uint32_t i = t * 64u + lane;
        const bool in = (fs_valid(t, a.n) >> lane) & 1ull;
        const bool sel = (sw >> lane) & 1ull;   // false at or past n
        const uint32_t id = sel ? a.flow_id[i] : BT_FLOW_ID_UNSELECTED;
        const bool num = sel && id < a.flow_cap;
        const bool sentinel = sel && flowtcp_is_sentinel(id);
        const uint64_t nw = __ballot(num), uw = __ballot(sentinel);
        nsel += (uint32_t)__popcll(sw);
        nnum += (uint32_t)__popcll(nw);
        nunk += (uint32_t)__popcll(uw);
        nbad += (uint32_t)__popcll(__ballot(sel && !num && !sentinel));
        if (in && !num) {
            if (a.seq) a.seq[i] = BT_FLOW_SEQ_NONE;
            if (a.byte_off) a.byte_off[i] = BT_FLOW_SEQ_OFF_NONE;
        }
        if (lane == 0) {
            a.numw[t] = nw;
            if (a.out_select) a.out_select[t] = a.keep_unkeyed ? uw : 0ull;
        }
    }
    if (lane == 0) {
        red[wid][0] = nsel; red[wid][1] = nnum; red[wid][2] = nunk; red[wid][3] = nbad;
        a.parts[c].wcount[wid] = nnum;
    }
    __syncthreads();
    if (tid < 4u) {
        uint32_t sum = 0;
#pragma unroll
        for (uint32_t v = 0; v < kFtWaves; ++v) sum += red[v][tid];
        bt_flow_seq_result* const res = a.result;
        uint32_t* const to = tid == 0 ? &res->selected : tid == 1 ? &res->numbered : tid == 2 ? &res->unkeyed : &res->bad_ids;
        if (sum) atomicAdd(to, sum);
        if (tid == 1u) a.parts[c].count = sum;
        if (tid == 2u && sum && a.keep_unkeyed) atomicAdd(&res->kept, sum);
    }
    if (c == 0 && tid == 4u) atomicAdd(&a.result->n, a.n);
}

__global__ __launch_bounds__(kFsJoinThreads) void bt_flowseq_join(FlowseqArgs a) {
    __shared__ uint32_t sh[kFsJoinThreads / 64u];
    const uint32_t tid = threadIdx.x;
    uint32_t running = 0;
    for (uint32_t c0 = 0; c0 < a.nchunks; c0 += kFsJoinThreads) {
        const uint32_t c = c0 + tid;
        const uint32_t v = c < a.nchunks ? a.parts[c].count : 0u;
        uint32_t tot;
        const uint32_t ex = block_excl<kFsJoinThreads>(v, sh, &tot);
        if (c < a.nchunks) a.parts[c].rel = running + ex;
        running += tot;
    }
    if (tid == 0) a.head->m = running;
}

__global__ __launch_bounds__(kFsThreads) void bt_flowseq_compact(FlowseqArgs a) {
    const uint32_t c = blockIdx.x, tid = threadIdx.x, lane = tid & 63u, wid = tid >> 6;
    uint32_t at = a.parts[c].rel;   // wave-uniform: where the wave's next numbered packet goes; below m
    for (uint32_t v = 0; v < wid; ++v) at += a.parts[c].wcount[v];
    const uint64_t below = (1ull << lane) - 1ull;
    const uint32_t t0 = c * kFtChunkTiles + wid * kFsUnitTiles;
    for (uint32_t k = 0; k < kFsUnitTiles && t0 + k < a.ntiles; ++k) {
        const uint32_t t = t0 + k;
        const uint64_t nw = a.numw[t];   // bits below n only
        if ((nw >> lane) & 1ull) {
            const uint32_t i = t * 64u + lane;
            a.a[at + (uint32_t)__popcll(nw & below)] = FsPair{a.flow_id[i], i};
        }
        at += (uint32_t)__popcll(nw);
    }
}

__global__ __launch_bounds__(kFsThreads) void bt_flowseq_digits(FlowseqArgs a, const FsPair* src, uint32_t shift) {
    __shared__ uint32_t cnt[kFtWaves][kFsDigits];
    const uint32_t c = blockIdx.x, tid = threadIdx.x, lane = tid & 63u, wid = tid >> 6;
    const uint32_t m = a.head->m;
    if ((uint64_t)c * kFsChunk >= m) return;   // the whole block
#pragma unroll
    for (uint32_t d = lane; d < kFsDigits; d += 64u) cnt[wid][d] = 0u;
    wave_lds_sync();
    const uint64_t below = (1ull << lane) - 1ull;
    const uint64_t p0 = (uint64_t)c * kFsChunk + wid * kFsUnit;
    for (uint32_t k = 0; k < kFsUnitTiles && p0 + k * 64u < m; ++k) {
        const uint64_t p = p0 + k * 64u + lane;
        const bool in = p < m;
        const uint32_t d = in ? (src[p].key >> shift) & (kFsDigits - 1u) : 0u;
        const uint64_t same = fs_match(d, in);
        if (in && !(same & below)) cnt[wid][d] += (uint32_t)__popcll(same);   // one lane per digit of the tile
        wave_lds_sync();
    }
    __syncthreads();
    for (uint32_t e = tid; e < kFtWaves * kFsDigits; e += kFsThreads) a.dwcnt[(uint64_t)c * kFtWaves * kFsDigits + e] = cnt[e / kFsDigits][e % kFsDigits];
    if (tid < kFsDigits) {
        uint32_t s = 0;
#pragma unroll
        for (uint32_t v = 0; v < kFtWaves; ++v) s += cnt[v][tid];
        a.dcnt[(uint64_t)tid * a.nchunks + c] = s;
    }
}
static_assert(kFsDigits <= kFsThreads, "a thread per digit");

__global__ __launch_bounds__(kFsJoinThreads) void bt_flowseq_djoin(FlowseqArgs a) {
    constexpr uint32_t kWaves = kFsJoinThreads / 64u;
    __shared__ uint32_t tot[kFsDigits];
    const uint32_t tid = threadIdx.x, lane = tid & 63u, wid = tid >> 6;
    const uint32_t m = a.head->m;
    const uint32_t live = (uint32_t)(((uint64_t)m + kFsChunk - 1u) / kFsChunk);   // <= nchunks
    for (uint32_t d = wid; d < kFsDigits; d += kWaves) {
        uint32_t running = 0;
        for (uint32_t c0 = 0; c0 < live; c0 += 64u) {
            const uint32_t c = c0 + lane;
            const uint32_t v = c < live ? a.dcnt[(uint64_t)d * a.nchunks + c] : 0u;
            uint32_t t;
            const uint32_t ex = fs_excl(v, lane, &t);
            if (c < live) a.drel[(uint64_t)d * a.nchunks + c] = running + ex;
            running += t;
        }
        if (lane == 0) tot[d] = running;
    }
    __syncthreads();
    if (tid < kFsDigits) {
        uint32_t s = 0;
        for (uint32_t q = 0; q < tid; ++q) s += tot[q];
        a.dstart[tid] = s;
    }
}

__global__ __launch_bounds__(kFsThreads) void bt_flowseq_scatter(FlowseqArgs a, const FsPair* src, FsPair* dst, uint32_t shift) {
    __shared__ uint32_t run[kFtWaves][kFsDigits];
    const uint32_t c = blockIdx.x, tid = threadIdx.x, lane = tid & 63u, wid = tid >> 6;
    const uint32_t m = a.head->m;
    if ((uint64_t)c * kFsChunk >= m) return;   // the whole block
    for (uint32_t e = tid; e < kFtWaves * kFsDigits; e += kFsThreads) {
        const uint32_t w = e / kFsDigits, d = e % kFsDigits;
        uint32_t at = a.dstart[d] + a.drel[(uint64_t)d * a.nchunks + c];
        for (uint32_t v = 0; v < w; ++v) at += a.dwcnt[((uint64_t)c * kFtWaves + v) * kFsDigits + d];
        run[w][d] = at;
    }
    __syncthreads();
    const uint64_t below = (1ull << lane) - 1ull;
    const uint64_t p0 = (uint64_t)c * kFsChunk + wid * kFsUnit;
    for (uint32_t k = 0; k < kFsUnitTiles && p0 + k * 64u < m; ++k) {
        const uint64_t p = p0 + k * 64u + lane;
        const bool in = p < m;
        FsPair pr{0u, 0u};
        if (in) pr = src[p];
        const uint32_t d = (pr.key >> shift) & (kFsDigits - 1u);
        const uint64_t same = fs_match(d, in);
        const uint32_t rank = (uint32_t)__popcll(same & below);
        if (in) dst[run[wid][d] + rank] = pr;   // below m: the digits' counts add up to m
        wave_lds_sync();
        if (in && rank == 0u) run[wid][d] += (uint32_t)__popcll(same);
        wave_lds_sync();
    }
}

template <int Mode>
__global__ __launch_bounds__(kFsThreads) void bt_flowseq_scan(FlowseqArgs a, const FsPair* s) {
    const uint32_t tid = threadIdx.x, lane = tid & 63u, wid = tid >> 6;
    const uint32_t u = blockIdx.x * kFtWaves + wid;
    const uint32_t m = a.head->m;
    const uint64_t p0 = (uint64_t)u * kFsUnit;
    if (p0 >= m) return;   // the whole wave; no block-wide step below
    // wave-uniform: the sums since the last head met, what precedes the unit included
    uint64_t rbytes = 0;
    uint32_t rcnt = 0, rhead = 0;
    if (Mode != kFsCarry) { rbytes = a.carry[u].bytes; rcnt = a.carry[u].cnt; }
    uint32_t prev_last = p0 ? s[p0 - 1u].key : 0u;   // the key before the tile's first
    uint64_t tbytes = 0, kbytes = 0;                 // wave-uniform tallies
    uint32_t nkept = 0, nflows = 0, nnew = 0;
    for (uint32_t k = 0; k < kFsUnitTiles && p0 + k * 64u < m; ++k) {
        const uint64_t p = p0 + k * 64u + lane;
        const bool in = p < m;
        FsPair pr{0u, 0u};
        if (in) pr = s[p];
        uint32_t len = 0;
        if (in) {
            if (Mode == kFsCarry) {
                uint64_t off;
                frame_at(a, pr.idx, off, len);   // idx < n
                len = len < 65535u ? len : 65535u;
                a.lens[p] = len;
            } else {
                len = a.lens[p];
            }
        }
        uint32_t before = __shfl_up(pr.key, 1);
        if (lane == 0) before = prev_last;
        const bool head = in && (p == 0u || pr.key != before);
        const uint64_t hw = __ballot(head);
        const uint32_t nin = (uint32_t)__popcll(__ballot(in));
        uint32_t total;
        const uint32_t pre = fs_excl(len, lane, &total);
        const uint64_t hb = hw & (~0ull >> (63u - lane));   // the heads at or below this lane
        const uint32_t start = hb ? 63u - (uint32_t)__clzll((long long)hb) : 0u;
        const uint32_t pre_start = __shfl(pre, (int)start);
        const uint32_t cnt = hb ? lane - start : rcnt + lane;                       // this flow's numbered packets before p
        const uint64_t bytes = hb ? (uint64_t)(pre - pre_start) : rbytes + pre;     // ... and their bytes
        if (Mode == kFsCarry) tbytes += total;
        bool keep = false;
        if (Mode == kFsEmit && in) {
            const bt_flow_seq_rec rec = a.table[pr.key];   // key < flow_cap
            const uint64_t bpk = rec.packets + cnt, bby = rec.bytes + bytes;
            if (a.seq) a.seq[pr.idx] = bpk < BT_FLOW_SEQ_MAX ? (uint32_t)bpk : BT_FLOW_SEQ_MAX;
            if (a.byte_off) a.byte_off[pr.idx] = bby;
            keep = (!a.max_packets || bpk < a.max_packets) && (!a.max_bytes || bby < a.max_bytes);
            if (keep && a.out_select)
                atomicOr(reinterpret_cast<unsigned long long*>(&a.out_select[pr.idx >> 6]), 1ull << (pr.idx & 63u));
        }
        if (Mode == kFsEmit) {
            nkept += (uint32_t)__popcll(__ballot(keep));
            kbytes += wave_sum(keep ? len : 0u);   // 64 lengths below 2^16
        }
        if (Mode == kFsCommit) {
            uint32_t after = __shfl_down(pr.key, 1);
            if (lane == 63u && p + 1u < m) after = s[p + 1u].key;
            const bool last = in && (p + 1u == m || pr.key != after);
            uint32_t fresh = 0;
            if (last) {   // the flow's totals; no other lane of the launch touches this record
                bt_flow_seq_rec* const rec = a.table + pr.key;   // key < flow_cap
                const uint64_t pk = rec->packets, by = rec->bytes;
                fresh = pk == 0ull;
                rec->packets = pk + cnt + 1u;
                rec->bytes = by + bytes + len;
            }
            nflows += (uint32_t)__popcll(__ballot(last));
            nnew += (uint32_t)__popcll(__ballot(fresh != 0u));
        }
        if (hw) {
            const uint32_t ls = 63u - (uint32_t)__clzll((long long)hw);   // the tile's last head
            rcnt = nin - ls;
            rbytes = total - (uint32_t)__builtin_amdgcn_readlane((int)pre, (int)ls);
            rhead = 1u;
        } else {
            rcnt += nin;
            rbytes += total;
        }
        prev_last = (uint32_t)__builtin_amdgcn_readlane((int)pr.key, 63);   // a tile that is not full is the last
    }
    if (lane == 0) {
        bt_flow_seq_result* const res = a.result;
        if (Mode == kFsCarry) {
            a.carry[u] = FsCarry{rbytes, rcnt, rhead};
            if (tbytes) fs_add64(&res->numbered_bytes, tbytes);
        }
        if (Mode == kFsEmit) {
            if (nkept) atomicAdd(&res->kept, nkept);
            if (kbytes) fs_add64(&res->kept_bytes, kbytes);
        }
        if (Mode == kFsCommit) {
            if (nflows) atomicAdd(&res->flows, nflows);
            if (nnew) atomicAdd(&res->new_flows, nnew);
        }
    }
}

// The units' carries become what precedes each unit: the sums since the last head before it.
__global__ __launch_bounds__(kFsJoinThreads) void bt_flowseq_sjoin(FlowseqArgs a) {
    constexpr uint32_t kWaves = kFsJoinThreads / 64u;
    __shared__ FsCarry wtot[kWaves];
    const uint32_t tid = threadIdx.x, lane = tid & 63u, wid = tid >> 6;
    const uint32_t m = a.head->m;
    const uint32_t live = (uint32_t)(((uint64_t)m + kFsUnit - 1u) / kFsUnit);   // <= nchunks * kFtWaves
    FsCarry running{0ull, 0u, 0u};   // block-uniform
    for (uint32_t u0 = 0; u0 < live; u0 += kFsJoinThreads) {
        const uint32_t u = u0 + tid;
        FsCarry own{0ull, 0u, 0u};
        if (u < live) own = a.carry[u];
        FsCarry incl = own;
        for (int o = 1; o < 64; o <<= 1) {
            const FsCarry y = fs_shfl_up(incl, o);
            if (lane >= (uint32_t)o) incl = fs_join(y, incl);
        }
        if (lane == 63u) wtot[wid] = incl;
        FsCarry ex = fs_shfl_up(incl, 1);
        if (lane == 0) ex = FsCarry{0ull, 0u, 0u};
        __syncthreads();
        FsCarry pre = running, all = running;
#pragma unroll
        for (uint32_t w = 0; w < kWaves; ++w) {
            const FsCarry x = wtot[w];
            if (w < wid) pre = fs_join(pre, x);
            all = fs_join(all, x);
        }
        __syncthreads();
        if (u < live) a.carry[u] = fs_join(pre, ex);
        running = all;
    }
}

void launch_flowseq_join(const FlowseqArgs& a, void* stream) {
    launch(bt_flowseq_join, dim3(1), dim3(kFsJoinThreads), 0, reinterpret_cast<hipStream_t>(stream), nullptr, nullptr, a);
}

void launch_flowseq_sort(const FlowseqArgs& a, uint32_t passes, void* stream, void* e_start, const FsPair** sorted) {
    hipStream_t st = reinterpret_cast<hipStream_t>(stream);
    const dim3 grid(a.nchunks), block(kFsThreads), one(1), join(kFsJoinThreads);
    const FsPair* src = a.a;
    FsPair* dst = a.b;
    for (uint32_t pass = 0; pass < passes; ++pass) {
        const uint32_t shift = pass * kFsDigitBits;
        launch(bt_flowseq_digits, grid, block, 0, st, pass == 0 ? reinterpret_cast<hipEvent_t>(e_start) : nullptr, nullptr, a, src, shift);
        launch(bt_flowseq_djoin, one, join, 0, st, nullptr, nullptr, a);
        launch(bt_flowseq_scatter, grid, block, 0, st, nullptr, nullptr, a, src, dst, shift);
        FsPair* const was = const_cast<FsPair*>(src);
        src = dst;
        dst = was;
    }
    *sorted = src;
}

int launch_flowseq(const FlowseqArgs& a, void* stream, void* const* ev) {
    if (a.n == 0 || a.nchunks == 0) return BT_OK;
    hipStream_t st = reinterpret_cast<hipStream_t>(stream);
    const auto e = [&](int k) { return ev ? reinterpret_cast<hipEvent_t>(ev[k]) : nullptr; };
    const dim3 grid(a.nchunks), block(kFsThreads), one(1), join(kFsJoinThreads);
    launch(bt_flowseq_class, grid, block, 0, st, e(0), nullptr, a);
    launch(bt_flowseq_join, one, join, 0, st, nullptr, nullptr, a);
    launch(bt_flowseq_compact, grid, block, 0, st, nullptr, nullptr, a);
    const FsPair* src = a.a;
    FsPair* dst = a.b;
    for (uint32_t pass = 0; pass < a.passes; ++pass) {
        const uint32_t shift = pass * kFsDigitBits;
        launch(bt_flowseq_digits, grid, block, 0, st, pass == 0 ? e(1) : nullptr, nullptr, a, src, shift);
        launch(bt_flowseq_djoin, one, join, 0, st, nullptr, nullptr, a);
        launch(bt_flowseq_scatter, grid, block, 0, st, nullptr, nullptr, a, src, dst, shift);
        FsPair* const was = const_cast<FsPair*>(src);
        src = dst;
        dst = was;
    }
    launch(bt_flowseq_scan<kFsCarry>, grid, block, 0, st, e(2), nullptr, a, src);
    launch(bt_flowseq_sjoin, one, join, 0, st, nullptr, nullptr, a);
    launch(bt_flowseq_scan<kFsEmit>, grid, block, 0, st, e(3), nullptr, a, src);
    launch(bt_flowseq_scan<kFsCommit>, grid, block, 0, st, nullptr, e(4), a, src);
    return hipGetLastError() == hipSuccess ? BT_OK : BT_E_INTERNAL;
}

}  // namespace bt
