// bt_pack.hip — ordered, size-weighted pack of the selected frames of a batch
// (bt_pass_pack_device, include/beatrice_gpu.h): what a filter on a GPU is for is to make
// the data smaller, and this is the step that produces the packets that passed.
//
// Two launches, in the shape of bt_chunk_sums / bt_compact (bt_kernels.hip): no block waits
// for another one, there is no look-back and no spin.
//   bt_pack_sums  one block per chunk of 256 tiles (16,384 packets): the aligned record size
//                 (lead + min(len, snap) rounded up to align) of every selected packet,
//                 summed per tile (a workspace word per tile) and per chunk (bytes, count).
//   bt_pack_copy  block c re-sums the chunks before it (64-bit), scans its own tiles' sums,
//                 and wave w copies tiles 64w .. 64w + 63 of the chunk, one tile at a time:
//                 the tile's 64 record offsets go to LDS (an exclusive wave scan), and the
//                 tile's destination range, one contiguous run of bytes, is cut into the
//                 16-B lines of the output (by absolute address). Lane l owns lines l, l + 64,
//                 ...: it finds the record a line starts in by a 6-step search of the LDS
//                 offsets; a line that lies wholly inside one record's bytes is one 16-B load
//                 at the source's own alignment (gfx950 global loads take any alignment) and
//                 one aligned 16-B store, both non-temporal (neither side is read again). A
//                 line that holds a record seam, an alignment gap, the tile's edge, bytes the
//                 source buffer does not hold or the capacity's edge is assembled byte by
//                 byte; it is still stored as one line when the tile owns all of it, else
//                 byte by byte (the neighbouring tile's wave writes the other bytes).
// Every source byte is read under `0 <= offset < bytes` (zeros otherwise); every store is to
// a byte of a record whose whole slot ends at or below cap.
#include "bt_wave.h"
#include "bt_hip_launch.h"
#include "bt_pack.h"

namespace bt {

namespace {

typedef u32x4 u32x4_any __attribute__((aligned(1)));   // a 16-B load at any byte alignment

// The select word of tile t with the bits at or above n cleared.
__device__ __forceinline__ uint64_t select_word(const PackArgs& a, uint32_t t) {
    if (t >= a.ntiles) return 0ull;
    uint64_t w = a.select[t];
    const uint32_t rest = a.n - t * 64u;   // packets from the tile's first one on (>= 1)
    if (rest < 64u) w &= (1ull << rest) - 1ull;
    return w;
}

// Packet i: the source offset of its frame and the frame bytes copied.
__device__ __forceinline__ void frame_of(const PackArgs& a, uint32_t i, uint64_t& off, uint32_t& len) {
    frame_at(a, i, off, len);
    if (len > 0xFFFFu) len = 0xFFFFu;   // a fixed stride: record lengths are 16-bit
    if (a.snap && len > a.snap) len = a.snap;
}

__device__ __forceinline__ uint32_t slot_bytes(const PackArgs& a, uint32_t len) {
    return (a.lead + len + a.align - 1u) & ~(a.align - 1u);
}

// The slot size of lane `lane`'s packet of tile t (0 when it is not selected).
__device__ __forceinline__ uint32_t lane_slot(const PackArgs& a, uint64_t word, uint32_t t, uint32_t lane) {
    if (!((word >> lane) & 1ull)) return 0u;
    uint64_t off;
    uint32_t len;
    frame_of(a, t * 64u + lane, off, len);
    return slot_bytes(a, len);
}

}  // namespace

// K1: per-tile and per-chunk sums. Wave w takes tiles 64w .. 64w + 63 of the chunk, four at a
// time so that their descriptor loads are in flight together.
__global__ __launch_bounds__(256) void bt_pack_sums(PackArgs a, uint32_t* tile_sums) {
    __shared__ uint64_t red_b[4];
    __shared__ uint32_t red_c[4];
    const uint32_t c = blockIdx.x, tid = threadIdx.x, lane = tid & 63u, wid = tid >> 6;
    const uint32_t t0 = c * kPackChunkTiles + wid * 64u;
    uint32_t mine = 0, count = 0;   // lane k: the sum / count of tile t0 + k
    for (uint32_t k0 = 0; k0 < 64u && t0 + k0 < a.ntiles; k0 += 4u) {
        uint64_t w[4];
        uint32_t v[4];
#pragma unroll
        for (uint32_t j = 0; j < 4u; ++j) {
            w[j] = select_word(a, t0 + k0 + j);
            v[j] = lane_slot(a, w[j], t0 + k0 + j, lane);
        }
#pragma unroll
        for (uint32_t j = 0; j < 4u; ++j) {
            const uint32_t s = w[j] ? wave_sum(v[j]) : 0u;
            if (lane == k0 + j) { mine = s; count = (uint32_t)__popcll(w[j]); }
        }
    }
    if (t0 + lane < a.ntiles) tile_sums[t0 + lane] = mine;
    uint64_t b = mine;
    for (int o = 32; o > 0; o >>= 1) {
        b += ((uint64_t)__shfl_xor((uint32_t)(b >> 32), o) << 32) | __shfl_xor((uint32_t)b, o);
        count += __shfl_xor(count, o);
    }
    if (lane == 0) { red_b[wid] = b; red_c[wid] = count; }
    __syncthreads();
    if (tid == 0) {
        a.sums[c].bytes = red_b[0] + red_b[1] + red_b[2] + red_b[3];
        a.sums[c].count = (uint64_t)red_c[0] + red_c[1] + red_c[2] + red_c[3];
    }
}

// K2: offsets and the copy.
__global__ __launch_bounds__(256) void bt_pack_copy(PackArgs a, const uint32_t* tile_sums) {
    __shared__ uint64_t words[kPackChunkTiles];
    __shared__ uint32_t tile_off[kPackChunkTiles];    // chunk-relative
    __shared__ uint32_t tile_rank[kPackChunkTiles];   // selected packets of the chunk before the tile
    __shared__ uint64_t red[4][4];
    __shared__ uint32_t wred[4][2];
    __shared__ uint32_t r_off[4][65];                 // per wave: the tile's slot offsets (chunk-relative)
    __shared__ uint64_t r_src[4][64];                 // ... each frame's source offset
    __shared__ uint32_t r_len[4][64];                 // ... lead + copied length (0: not selected)
    const uint32_t c = blockIdx.x, tid = threadIdx.x, lane = tid & 63u, wid = tid >> 6;
    const uint32_t t = c * kPackChunkTiles + tid;
    const uint64_t word = select_word(a, t);
    const uint32_t tsum = t < a.ntiles ? tile_sums[t] : 0u;

    // the chunks before this one, and the totals
    uint64_t pre_b = 0, pre_c = 0, tot_b = 0, tot_c = 0;
    for (uint32_t i = tid; i < a.nchunks; i += 256u) {
        const PackChunkSum s = a.sums[i];
        tot_b += s.bytes; tot_c += s.count;
        if (i < c) { pre_b += s.bytes; pre_c += s.count; }
    }
    for (int o = 32; o > 0; o >>= 1) {
        pre_b += ((uint64_t)__shfl_xor((uint32_t)(pre_b >> 32), o) << 32) | __shfl_xor((uint32_t)pre_b, o);
        pre_c += ((uint64_t)__shfl_xor((uint32_t)(pre_c >> 32), o) << 32) | __shfl_xor((uint32_t)pre_c, o);
        tot_b += ((uint64_t)__shfl_xor((uint32_t)(tot_b >> 32), o) << 32) | __shfl_xor((uint32_t)tot_b, o);
        tot_c += ((uint64_t)__shfl_xor((uint32_t)(tot_c >> 32), o) << 32) | __shfl_xor((uint32_t)tot_c, o);
    }
    // this chunk's tiles: inclusive wave scans of the tile sums and counts
    const uint32_t cnt = (uint32_t)__popcll(word);
    uint32_t incl_b = tsum, incl_c = cnt;
    for (int o = 1; o < 64; o <<= 1) {
        const uint32_t yb = __shfl_up(incl_b, o), yc = __shfl_up(incl_c, o);
        if (lane >= (uint32_t)o) { incl_b += yb; incl_c += yc; }
    }
    if (lane == 0) { red[wid][0] = pre_b; red[wid][1] = pre_c; red[wid][2] = tot_b; red[wid][3] = tot_c; }
    if (lane == 63) { wred[wid][0] = incl_b; wred[wid][1] = incl_c; }
    words[tid] = word;
    __syncthreads();
    const uint64_t base = red[0][0] + red[1][0] + red[2][0] + red[3][0];     // this chunk's first byte
    const uint64_t rank0 = red[0][1] + red[1][1] + red[2][1] + red[3][1];    // ... and first record
    const uint64_t total = red[0][2] + red[1][2] + red[2][2] + red[3][2];
    const uint64_t total_n = red[0][3] + red[1][3] + red[2][3] + red[3][3];
    uint32_t wpre_b = 0, wpre_c = 0;
    for (uint32_t w = 0; w < wid; ++w) { wpre_b += wred[w][0]; wpre_c += wred[w][1]; }
    const uint32_t chunk_bytes = wred[0][0] + wred[1][0] + wred[2][0] + wred[3][0];
    tile_off[tid] = wpre_b + incl_b - tsum;
    tile_rank[tid] = wpre_c + incl_c - cnt;
    __syncthreads();
    if (c == 0 && tid == 0) *a.total = total;

    const uint64_t below = (1ull << lane) - 1ull;
    const uintptr_t out0 = reinterpret_cast<uintptr_t>(a.out);
    uint32_t n_fit = 0;   // wave-uniform: this wave's records that fit in cap
    for (uint32_t k = 0; k < 64u; ++k) {
        const uint32_t tt = wid * 64u + k;
        const uint64_t w = words[tt];
        if (!w) continue;   // the same word in every lane
        const bool sel = (w >> lane) & 1ull;
        uint64_t src = 0;
        uint32_t len = 0;
        if (sel) frame_of(a, (c * kPackChunkTiles + tt) * 64u + lane, src, len);
        const uint32_t plen = sel ? a.lead + len : 0u;
        const uint32_t slot = sel ? slot_bytes(a, len) : 0u;
        uint32_t incl = slot;
        for (int o = 1; o < 64; o <<= 1) {
            const uint32_t y = __shfl_up(incl, o);
            if (lane >= (uint32_t)o) incl += y;
        }
        const uint32_t off = tile_off[tt] + incl - slot;
        wave_lds_sync();   // the previous tile's reads of the rows are done
        r_off[wid][lane] = off;
        if (lane == 63) r_off[wid][64] = off + slot;
        r_src[wid][lane] = src;
        r_len[wid][lane] = plen;
        wave_lds_sync();
        const bool fits = base + off + slot <= a.cap;
        n_fit += (uint32_t)__popcll(__ballot(sel && fits));
        if (sel && a.out_desc)
            a.out_desc[rank0 + tile_rank[tt] + (uint32_t)__popcll(w & below)] = BT_DESC(base + off + a.lead, len);

        // the tile's destination bytes [g0, g1), cut at cap, as 16-B lines of the output
        const uint64_t g0 = base + r_off[wid][0];
        uint64_t g1 = base + r_off[wid][64];
        if (g1 > a.cap) g1 = a.cap;
        if (g1 <= g0) continue;
        const uintptr_t a0 = out0 + g0, a1 = out0 + g1;
        const uintptr_t first = a0 & ~(uintptr_t)15;
        const uint64_t lines = (a1 - first + 15u) >> 4;
        for (uint64_t j = lane; j < lines; j += 64u) {
            const uintptr_t line = first + 16u * j;
            uint8_t* const dst = a.out + (int64_t)(line - out0);   // a line may start before out: bytes below lo are not written
            const uintptr_t lo = line > a0 ? line : a0;
            const uintptr_t hi = line + 16u < a1 ? line + 16u : a1;
            const uint32_t d = (uint32_t)(lo - out0 - base);   // chunk-relative offset of the first byte
            uint32_t r = 0;                                    // the last record that starts at or before d
#pragma unroll
            for (uint32_t step = 32u; step; step >>= 1)
                if (r_off[wid][r + step] <= d) r += step;
            const bool whole = hi - lo == 16u;
            const uint32_t p = d - r_off[wid][r];
            if (whole && p + 16u <= r_len[wid][r]) {   // inside one record's bytes
                if (base + r_off[wid][r + 1] > a.cap) continue;
                const uint64_t s = r_src[wid][r] - a.lead + p;   // wraps to a huge value before the buffer
                if (s <= a.bytes && a.bytes - s >= 16u) {
                    const u32x4 v = __builtin_nontemporal_load(reinterpret_cast<const u32x4_any*>(a.base + s));
                    __builtin_nontemporal_store(v, reinterpret_cast<u32x4*>(dst));
                    continue;
                }
            }
            // byte by byte: seams, gaps, edges of the tile, of the source buffer and of cap
            uint32_t v[4] = {0u, 0u, 0u, 0u};
            uint32_t mask = 0;   // the line's bytes this tile writes
            const uint32_t b0 = (uint32_t)(lo - line), nb = (uint32_t)(hi - lo);
            for (uint32_t b = 0; b < nb; ++b) {
                const uint32_t dd = d + b;
                while (r < 63u && r_off[wid][r + 1] <= dd) ++r;
                const uint32_t pp = dd - r_off[wid][r];
                uint32_t byte = 0;
                if (pp < r_len[wid][r]) {
                    const uint64_t s = r_src[wid][r] - a.lead + pp;
                    if (s < a.bytes) byte = a.base[s];
                }
                if (base + r_off[wid][r + 1] <= a.cap) {
                    const uint32_t q = b0 + b;
                    v[q >> 2] |= byte << ((q & 3u) * 8u);
                    mask |= 1u << q;
                }
            }
            if (mask == 0xFFFFu) {
                const u32x4 x = {v[0], v[1], v[2], v[3]};
                __builtin_nontemporal_store(x, reinterpret_cast<u32x4*>(dst));
            } else {
                for (uint32_t q = 0; q < 16u; ++q)
                    if ((mask >> q) & 1u) dst[q] = (uint8_t)(v[q >> 2] >> ((q & 3u) * 8u));
            }
        }
    }

    // n_packed = the records of the longest prefix that fits: the whole chunks before the first
    // chunk that does not fit entirely, and that chunk's fitting records.
    __syncthreads();
    if (lane == 0) wred[wid][0] = n_fit;
    __syncthreads();
    if (tid == 0) {
        if (total <= a.cap) {
            if (c == 0) *a.n_packed = (uint32_t)total_n;
        } else if (base <= a.cap && base + chunk_bytes > a.cap) {
            *a.n_packed = (uint32_t)rank0 + wred[0][0] + wred[1][0] + wred[2][0] + wred[3][0];
        }
    }
}

int launch_pass_pack(const PackArgs& a, void* stream, void* timing_start, void* timing_stop) {
    if (a.n == 0 || a.nchunks == 0) return BT_OK;
    hipStream_t st = reinterpret_cast<hipStream_t>(stream);
    hipEvent_t e0 = reinterpret_cast<hipEvent_t>(timing_start), e1 = reinterpret_cast<hipEvent_t>(timing_stop);
    uint32_t* tile_sums = reinterpret_cast<uint32_t*>(a.sums + a.nchunks);
    launch(bt_pack_sums, dim3(a.nchunks), dim3(256), 0, st, e0, nullptr, a, tile_sums);
    launch(bt_pack_copy, dim3(a.nchunks), dim3(256), 0, st, nullptr, e1, a, (const uint32_t*)tile_sums);
    return hipGetLastError() == hipSuccess ? BT_OK : BT_E_INTERNAL;
}

}  // namespace bt
