// bt_tally.hip — counts of a batch that stays on the device (bt_tally_device,
// include/beatrice_gpu.h): the decision bytes by value, the frame lengths by code, the parsed
// layers by present / ok bit, and the first THROW and HOST decisions.
//
// Two launches, in the shape of bt_chunk_sums / bt_compact (bt_kernels.hip) and bt_pack_sums /
// bt_pack_copy (bt_pack.hip): no block waits for another one, there is no look-back, no spin
// and no global atomic, so every count is exact and the same from run to run.
//   bt_tally_chunks  one block per chunk of 256 tiles (16,384 packets) writes one TallyPartial.
//                    The decision bytes are read as the 16-B granules (by absolute address)
//                    that hold the chunk's bytes, one granule per lane and step, non-temporal;
//                    bytes of a granule outside the chunk are masked, so an unaligned head or
//                    tail costs nothing and no load leaves the granules of decide[0 .. n). The
//                    256-bin histogram is a wave-private LDS row, filled by ballot peeling (one
//                    turn per distinct value of a byte position: a wave of real decisions holds
//                    a handful) or, as the A/B, by one LDS add per byte. Lengths and layers are
//                    taken tile by tile, lane = packet: wave w has tiles 64w .. 64w + 63 of the
//                    chunk; four per-lane 64-bit length sums selected by code, 16 ballots +
//                    popcounts over the present | ok dword.
//   bt_tally_join    one block: the first THROW / HOST index is the minimum over the partials;
//                    the partials of the chunks before the one that holds the first THROW (all
//                    chunks when not stopping) are summed in 64 bits, that one chunk's packets
//                    up to the throw are recounted (<= 16 KiB of decisions and their lengths),
//                    and *out is written or added to.
// Lanes at or past n never load: no descriptor at or past n and no record tile at or past
// ceil(n / 64) is read.
#include "bt_wave.h"
#include "bt_hip_launch.h"
#include "bt_tally.h"

namespace bt {

namespace {

// Packet i (< a.n): its frame's length as the pack takes it (a fixed stride: min(stride, 65535)).
__device__ __forceinline__ uint32_t length_of(const TallyArgs& a, uint32_t i) {
    uint64_t off;
    uint32_t len;
    frame_at(a, i, off, len);
    return len > 0xFFFFu ? 0xFFFFu : len;
}

// Packet i (< a.n): present | ok << 8 of its record.
__device__ __forceinline__ uint32_t layers_of(const TallyArgs& a, uint32_t i) {
    uint64_t at;
    if (a.rec_layout == kTallyRecTiled) at = ((uint64_t)(i >> 6) * 6u + 1u) * 1024u + (i & 63u) * 16u;
    else if (a.rec_layout == kTallyRecPlanes) at = ((uint64_t)a.n_cap + i) * 16u;
    else at = (uint64_t)i * BT_REC_BYTES + 24u;
    return __builtin_nontemporal_load(reinterpret_cast<const uint32_t*>(a.records + at)) & 0xFFFFu;
}

// One byte position of a wave's granules into the wave's row: key < 256, or 256 = no byte.
template <bool Peel>
__device__ __forceinline__ void row_add(uint32_t* row, uint32_t key, uint32_t lane) {
    if (!Peel) {
        if (key < 256u) atomicAdd(&row[key], 1u);
        return;
    }
    uint64_t todo = __ballot(key < 256u);
    while (todo) {   // the same word in every lane: one turn per distinct value
        const int leader = __ffsll((unsigned long long)todo) - 1;
        const uint32_t k = (uint32_t)__shfl((int)key, leader);
        const uint64_t same = __ballot(key == k);
        if (lane == (uint32_t)leader) atomicAdd(&row[k], (uint32_t)__popcll(same));
        todo &= ~same;
    }
}

}  // namespace

// K1: one partial per chunk.
template <bool Peel>
__global__ __launch_bounds__(256) void bt_tally_chunks(TallyArgs a) {
    __shared__ uint32_t rows[4][256];
    __shared__ uint64_t red_b[4][4];
    __shared__ uint32_t red_l[4][16];
    __shared__ uint32_t red_f[4][2];
    const uint32_t c = blockIdx.x, tid = threadIdx.x, lane = tid & 63u, wid = tid >> 6;
    const uint32_t p0 = c * kTallyChunk;                                   // the chunk's packets [p0, p1)
    const uint32_t p1 = a.n - p0 < kTallyChunk ? a.n : p0 + kTallyChunk;   // p0 < n: nchunks = ceil(n / chunk)
#pragma unroll
    for (uint32_t w = 0; w < 4u; ++w) rows[w][tid] = 0u;
    __syncthreads();

    uint32_t ft = kTallyNone, fh = kTallyNone;
    if (a.decide) {
        uint32_t* const row = rows[wid];
        const uintptr_t a0 = reinterpret_cast<uintptr_t>(a.decide) + p0, a1 = reinterpret_cast<uintptr_t>(a.decide) + p1;
        const uintptr_t g0 = a0 & ~(uintptr_t)15;
        const uint32_t ngran = (uint32_t)((a1 - g0 + 15u) >> 4);   // <= 1025
        for (uint32_t g = tid; g - lane < ngran; g += 256u) {      // whole waves take a step (row_add votes)
            const bool live = g < ngran;
            const uintptr_t at = g0 + 16u * (uintptr_t)g;
            u32x4 v = {0u, 0u, 0u, 0u};
            if (live) v = __builtin_nontemporal_load(reinterpret_cast<const u32x4*>(at));
            // the granule's bytes [lo, hi) belong to the chunk
            const uint32_t lo = !live ? 16u : at < a0 ? (uint32_t)(a0 - at) : 0u;
            const uint32_t hi = !live ? 16u : at + 16u > a1 ? (uint32_t)(a1 - at) : 16u;
            const uint32_t d[4] = {v.x, v.y, v.z, v.w};
            const uint32_t first = p0 + (uint32_t)(at - a0);       // batch index of byte 0 (wraps below a0: unused)
#pragma unroll
            for (uint32_t j = 0; j < 16u; ++j) {
                const bool in = j >= lo && j < hi;
                const uint32_t b = (d[j >> 2] >> (8u * (j & 3u))) & 0xFFu;
                row_add<Peel>(row, in ? b : 256u, lane);
                if (in && (b >> 6) == BT_DECIDE_THROW && ft == kTallyNone) ft = first + j;
                if (in && (b >> 6) == BT_DECIDE_HOST && fh == kTallyNone) fh = first + j;
            }
        }
    }
    ft = wave_min(ft);   // a lane's granules ascend, so its first hit is its lowest index
    fh = wave_min(fh);

    // lengths by code and layers, tile by tile
    uint64_t len_by[4] = {0ull, 0ull, 0ull, 0ull};
    uint32_t lay[16];
#pragma unroll
    for (uint32_t k = 0; k < 16u; ++k) lay[k] = 0u;
    if (a.lengths || a.records) {
        const uint32_t t0 = c * kTallyChunkTiles + wid * 64u;
#pragma unroll 4
        for (uint32_t k = 0; k < 64u; ++k) {
            if (t0 + k >= a.ntiles) break;
            const uint32_t i = (t0 + k) * 64u + lane;
            const bool in = i < a.n;
            if (a.lengths) {
                const uint32_t code = in ? (uint32_t)a.decide[i] >> 6 : 4u;
                const uint64_t len = in ? length_of(a, i) : 0u;
#pragma unroll
                for (uint32_t q = 0; q < 4u; ++q) len_by[q] += code == q ? len : 0ull;
            }
            if (a.records) {
                const uint32_t w = in ? layers_of(a, i) : 0u;
#pragma unroll
                for (uint32_t q = 0; q < 16u; ++q) lay[q] += (uint32_t)__popcll(__ballot((w >> q) & 1u));
            }
        }
    }
#pragma unroll
    for (uint32_t q = 0; q < 4u; ++q) len_by[q] = wave_sum64(len_by[q]);
    if (lane == 0) {
#pragma unroll
        for (uint32_t q = 0; q < 4u; ++q) red_b[wid][q] = len_by[q];
#pragma unroll
        for (uint32_t q = 0; q < 16u; ++q) red_l[wid][q] = lay[q];
        red_f[wid][0] = ft;
        red_f[wid][1] = fh;
    }
    __syncthreads();
    TallyPartial& p = a.parts[c];
    p.hist[tid] = rows[0][tid] + rows[1][tid] + rows[2][tid] + rows[3][tid];
    if (tid < 4u) p.bytes[tid] = red_b[0][tid] + red_b[1][tid] + red_b[2][tid] + red_b[3][tid];
    if (tid >= 64u && tid < 80u) {
        const uint32_t q = tid - 64u;
        p.layer[q] = red_l[0][q] + red_l[1][q] + red_l[2][q] + red_l[3][q];
    }
    if (tid == 128u || tid == 129u) {
        const uint32_t q = tid - 128u;
        uint32_t m = red_f[0][q];
#pragma unroll
        for (uint32_t w = 1; w < 4u; ++w) m = red_f[w][q] < m ? red_f[w][q] : m;
        (q ? p.first_host : p.first_throw) = m;
    }
}

// K2: the partials into *out.
__global__ __launch_bounds__(kTallyJoinThreads) void bt_tally_join(TallyArgs a) {
    constexpr uint32_t kWaves = kTallyJoinThreads / 64u;   // 8
    __shared__ uint64_t bins[kWaves][256];                 // per wave: the chunks it summed, by decision value
    __shared__ uint64_t small[kWaves][24];                 // ... their 4 length sums (0..3) and 16 layer counts (8..23)
    __shared__ uint32_t firsts[2];
    __shared__ uint32_t recount[256];                      // the throw's chunk, up to the throw
    __shared__ unsigned long long relen[4];
    __shared__ uint64_t total[256];
    const uint32_t tid = threadIdx.x, lane = tid & 63u, wid = tid >> 6;
    const bool counts = a.decide != nullptr;

    // the first THROW and HOST decisions of the batch
    uint32_t ft = kTallyNone, fh = kTallyNone;
    if (counts)
        for (uint32_t c = tid; c < a.nchunks; c += kTallyJoinThreads) {
            const uint32_t t = a.parts[c].first_throw, h = a.parts[c].first_host;
            ft = t < ft ? t : ft;
            fh = h < fh ? h : fh;
        }
    if (tid < 2u) firsts[tid] = kTallyNone;
    if (tid < 256u) recount[tid] = 0u;
    if (tid < 4u) relen[tid] = 0ull;
    __syncthreads();
    ft = wave_min(ft);
    fh = wave_min(fh);
    if (lane == 0) {
        atomicMin(&firsts[0], ft);   // LDS
        atomicMin(&firsts[1], fh);
    }
    __syncthreads();
    ft = firsts[0];
    fh = firsts[1];
    const bool stop = (a.flags & BT_TALLY_STOP_AT_THROW) && ft != kTallyNone;
    const uint32_t scanned = !counts ? a.n : stop ? ft : a.n;
    const uint32_t whole = !counts ? 0u : stop ? ft / kTallyChunk : a.nchunks;   // chunks counted entirely

    // wave w sums the partials of chunks w, w + 8, ...: lane l has bins 4l .. 4l + 3, and the
    // lanes below 24 one of the small sums each (lengths over the counted chunks, layers over all)
    uint64_t b[4] = {0ull, 0ull, 0ull, 0ull};
    uint64_t s = 0ull;
#pragma unroll 8
    for (uint32_t c = wid; c < a.nchunks; c += kWaves) {
        const TallyPartial& p = a.parts[c];
        if (c < whole) {
            const uint4 h = *reinterpret_cast<const uint4*>(&p.hist[4u * lane]);
            b[0] += h.x; b[1] += h.y; b[2] += h.z; b[3] += h.w;
            if (lane < 4u) s += p.bytes[lane];
        }
        if (lane >= 8u && lane < 24u) s += p.layer[lane - 8u];
    }
#pragma unroll
    for (uint32_t q = 0; q < 4u; ++q) bins[wid][4u * lane + q] = b[q];
    if (lane < 24u) small[wid][lane] = s;

    // the chunk that holds the first THROW, up to it
    if (stop)
        for (uint32_t i = whole * kTallyChunk + tid; i < ft; i += kTallyJoinThreads) {
            const uint32_t v = a.decide[i];
            atomicAdd(&recount[v], 1u);   // LDS
            if (a.lengths) atomicAdd(&relen[v >> 6], (unsigned long long)length_of(a, i));
        }
    __syncthreads();
    if (tid < 256u) {
        uint64_t t = recount[tid];
#pragma unroll
        for (uint32_t w = 0; w < kWaves; ++w) t += bins[w][tid];
        total[tid] = t;
    }
    uint64_t mine = 0ull;   // threads 256 .. 279: small sum tid - 256
    if (tid >= 256u && tid < 280u) {
        const uint32_t q = tid - 256u;
#pragma unroll
        for (uint32_t w = 0; w < kWaves; ++w) mine += small[w][q];
        if (q < 4u) mine += relen[q];
    }
    __syncthreads();

    bt_tally* const o = a.out;
    const bool add = (a.flags & BT_TALLY_ACCUMULATE) != 0;
    if (tid < 256u) {
        uint64_t* const dst = &o->slot[tid >> 6][tid & 63u];
        *dst = total[tid] + (add ? *dst : 0ull);
    } else if (tid < 260u) {
        const uint32_t q = tid - 256u;
        o->bytes[q] = mine + (add ? o->bytes[q] : 0ull);
    } else if (tid >= 264u && tid < 272u) {
        const uint32_t q = tid - 264u;
        o->layer_present[q] = mine + (add ? o->layer_present[q] : 0ull);
    } else if (tid >= 272u && tid < 280u) {
        const uint32_t q = tid - 272u;
        o->layer_ok[q] = mine + (add ? o->layer_ok[q] : 0ull);
    } else if (tid >= 320u && tid < 324u) {
        const uint32_t q = tid - 320u;
        uint64_t t = 0ull;
        for (uint32_t k = 0; k < 64u; ++k) t += total[64u * q + k];
        o->code[q] = t + (add ? o->code[q] : 0ull);
    } else if (tid == 384u) {
        o->n = a.n + (add ? o->n : 0ull);
        o->scanned = scanned + (add ? o->scanned : 0ull);
        o->first_throw = ft == kTallyNone ? a.n : ft;
        o->first_host = fh == kTallyNone ? a.n : fh;
        o->first_throw_slot = ft == kTallyNone ? 0u : (uint32_t)a.decide[ft] & 63u;
        o->first_host_slot = fh == kTallyNone ? 0u : (uint32_t)a.decide[fh] & 63u;
        if (!add) o->reserved[0] = o->reserved[1] = o->reserved[2] = 0ull;
    }
}

int launch_tally(const TallyArgs& a, void* stream, void* timing_start, void* timing_stop) {
    if (a.n == 0 || a.nchunks == 0) return BT_OK;
    hipStream_t st = reinterpret_cast<hipStream_t>(stream);
    hipEvent_t e0 = reinterpret_cast<hipEvent_t>(timing_start), e1 = reinterpret_cast<hipEvent_t>(timing_stop);
    if (a.peel) launch(bt_tally_chunks<true>, dim3(a.nchunks), dim3(256), 0, st, e0, nullptr, a);
    else launch(bt_tally_chunks<false>, dim3(a.nchunks), dim3(256), 0, st, e0, nullptr, a);
    launch(bt_tally_join, dim3(1), dim3(kTallyJoinThreads), 0, st, nullptr, e1, a);
    return hipGetLastError() == hipSuccess ? BT_OK : BT_E_INTERNAL;
}

}  // namespace bt
