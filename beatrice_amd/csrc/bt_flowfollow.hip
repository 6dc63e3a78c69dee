// bt_flowfollow.hip — the delivered bytes of a reassembly call, exported: every (flow, direction)'s
// stream in order, the runs between holes, and each packet's place (bt_flow_follow_device,
// include/beatrice_gpu.h).
//
// The reassembly (bt_flowreasm.hip) has left, behind its Emit launch, the sorted pair list in
// (flow << 1 | dir, rel, index) order, each packet's final payload offset and delivered length
// (meta) and pred (none at a stream's head, cut behind a hole). A pair that starts a key or whose
// pred is cut always delivers a byte, so "run head" is pred >= cut. What is left is a plain
// prefix sum of (delivered bytes, run heads) over the list and a gather-copy. These launches run
// before Commit, which rewrites the have and next they read. No lane, wave or block waits for
// another, there is no atomic, and every output has one writer: the same from run to run.
//   bt_flowfollow_sum<Carry>  wave = unit of 32 tiles of the sorted list: the unit's sums.
//   bt_flowfollow_join        one block: the exclusive scan of the units' sums; the totals, the
//                             result and at[m] = total.
//   bt_flowfollow_sum<Emit>   per pair its output offset and its source offset into the scratch
//                             (the copy then gathers nothing), place[index], and at a head the
//                             run's flow, flags, at and pos, and its at into the scratch.
//   bt_flowfollow_runs        one lane per written run: len = the next run's at (the total behind
//                             the last) less its own, both from the scratch.
//   bt_flowfollow_copy        bt_pack_copy's scheme over sorted positions: a tile of 64 pairs has
//                             one contiguous destination range, cut into the output's 16-B lines
//                             by absolute address. Lane l owns lines l, l + 64, ...: the pair a
//                             line starts in by a 6-step search of the tile's offsets in LDS; a
//                             line wholly inside one segment is one 16-B load at the source's own
//                             alignment and one aligned 16-B non-temporal store; a line with a
//                             seam, the tile's edge, the edge of cap or source bytes past the
//                             buffer is assembled byte by byte and stored as a line only when the
//                             tile owns all 16 bytes.
// Every source byte is read under `offset < bytes` (zero otherwise); every store is to an output
// byte below cap.
#include "bt_hip_launch.h"
#include "bt_wave.h"
#include "bt_flowfollow.h"

namespace bt {

namespace {

constexpr uint32_t kFfThreads = kFtWaves * 64u;
enum FfMode { kFfCarryMode = 0, kFfEmit = 1 };

typedef u32x4 u32x4_any __attribute__((aligned(1)));   // a 16-B load at any byte alignment

__device__ __forceinline__ uint64_t ff_shfl_up64(uint64_t v, int o) {
    return ((uint64_t)__shfl_up((uint32_t)(v >> 32), o) << 32) | __shfl_up((uint32_t)v, o);
}

}  // namespace

template <int Mode>
__global__ __launch_bounds__(kFfThreads) void bt_flowfollow_sum(FlowfollowArgs a) {
    const uint32_t tid = threadIdx.x, lane = tid & 63u, wid = tid >> 6;
    const uint32_t u = blockIdx.x * kFtWaves + wid;
    const uint32_t m = a.head->m;
    const uint64_t p0 = (uint64_t)u * kFsUnit;
    if (p0 >= m) return;   // the whole wave; no block-wide step below
    uint64_t bytes = 0;    // Carry: the lane's own sum; Emit: wave-uniform, what precedes the tile
    uint32_t heads = 0;
    if (Mode == kFfEmit) {
        const FfCarry c = a.carry[u];
        bytes = c.bytes;
        heads = c.heads;
    }
    const uint64_t below = (1ull << lane) - 1ull;
    for (uint32_t k = 0; k < kFsUnitTiles && p0 + k * 64u < m; ++k) {
        const uint64_t p = p0 + k * 64u + lane;
        const bool in = p < m;
        FsPair pr{0u, 0u};
        FstMeta mt{0u, 0u};
        uint32_t pred = 0;
        if (in) {
            pr = a.s[p];            // idx < n
            mt = a.meta[pr.idx];
            pred = a.pred[pr.idx];
        }
        const uint32_t len = mt.len_dir & 0x7FFFFFFFu;   // delivered; 0 for a whole duplicate
        const bool head = in && pred >= kFrCut;          // it delivers: len > 0
        if (Mode == kFfCarryMode) {
            bytes += len;
            heads += head ? 1u : 0u;
        } else {
            uint32_t incl = len;   // a tile's sum is below 2^23
            for (int o = 1; o < 64; o <<= 1) {
                const uint32_t y = __shfl_up(incl, o);
                if (lane >= (uint32_t)o) incl += y;
            }
            const uint64_t headw = __ballot(head);
            const uint64_t at = bytes + (incl - len);
            if (in) {
                uint64_t off;
                uint32_t flen;
                frame_at(a, pr.idx, off, flen);
                a.at[p] = at;
                a.src[p] = off + mt.start;
                if (len && a.place) a.place[pr.idx] = at;
            }
            if (head) {
                const uint32_t r = heads + (uint32_t)__popcll(headw & below);   // below m <= n
                a.runat[r] = at;
                if (r < a.run_cap) {
                    const bt_flow_reasm_dir* const rec = &a.table[pr.key >> 1].d[pr.key & 1u];   // key >> 1 < flow_cap; Commit writes it, a launch later
                    const bool have = rec->have != 0u;
                    const int64_t base = have ? rec->next : kFrNewBase;
                    bt_flow_follow_run* const run = a.runs + r;
                    run->flow = pr.key >> 1;
                    run->flags = (pr.key & 1u) | (have ? 0u : BT_FOLLOW_NEW) | (pred == kFrCut ? BT_FOLLOW_HOLE : 0u);
                    run->at = at;
                    run->pos = (int64_t)((uint64_t)base + a.seg[p].rel);   // max(rel, hi) = rel at a head
                }
            }
            bytes += (uint32_t)__builtin_amdgcn_readlane((int)incl, 63);
            heads += (uint32_t)__popcll(headw);
        }
    }
    if (Mode == kFfCarryMode) {
        bytes = wave_sum64(bytes);
        heads = wave_sum(heads);
        if (lane == 0) a.carry[u] = FfCarry{bytes, heads, 0u};
    }
}

// The units' sums become what precedes each unit; the totals.
__global__ __launch_bounds__(kFsJoinThreads) void bt_flowfollow_join(FlowfollowArgs a) {
    constexpr uint32_t kWaves = kFsJoinThreads / 64u;
    __shared__ uint64_t wb[kWaves];
    __shared__ uint32_t wh[kWaves];
    const uint32_t tid = threadIdx.x, lane = tid & 63u, wid = tid >> 6;
    const uint32_t m = a.head->m;
    const uint32_t live = (uint32_t)(((uint64_t)m + kFsUnit - 1u) / kFsUnit);   // <= nchunks * kFtWaves
    uint64_t run_b = 0;   // block-uniform
    uint32_t run_h = 0;
    for (uint32_t u0 = 0; u0 < live; u0 += kFsJoinThreads) {
        const uint32_t u = u0 + tid;
        FfCarry own{0ull, 0u, 0u};
        if (u < live) own = a.carry[u];
        uint64_t ib = own.bytes;
        uint32_t ih = own.heads;
        for (int o = 1; o < 64; o <<= 1) {
            const uint64_t yb = ff_shfl_up64(ib, o);
            const uint32_t yh = __shfl_up(ih, o);
            if (lane >= (uint32_t)o) { ib += yb; ih += yh; }
        }
        if (lane == 63u) { wb[wid] = ib; wh[wid] = ih; }
        __syncthreads();
        uint64_t pre_b = run_b, all_b = run_b;
        uint32_t pre_h = run_h, all_h = run_h;
#pragma unroll
        for (uint32_t w = 0; w < kWaves; ++w) {
            const uint64_t xb = wb[w];
            const uint32_t xh = wh[w];
            if (w < wid) { pre_b += xb; pre_h += xh; }
            all_b += xb; all_h += xh;
        }
        __syncthreads();
        if (u < live) a.carry[u] = FfCarry{pre_b + ib - own.bytes, pre_h + ih - own.heads, 0u};
        run_b = all_b;
        run_h = all_h;
    }
    if (tid == 0) {
        a.at[m] = run_b;   // m <= n: the entry behind the last pair
        *a.fhead = FfHead{run_b, run_h, 0u};
        bt_flow_follow_result r;
        r.total = run_b;
        r.written = run_b < a.cap ? run_b : a.cap;
        r.n_runs = run_h;
        r.runs_written = run_h < a.run_cap ? run_h : a.run_cap;
        r.reserved = 0;
        *a.result = r;
    }
}

__global__ __launch_bounds__(256) void bt_flowfollow_runs(FlowfollowArgs a) {
    const uint64_t k = (uint64_t)blockIdx.x * 256u + threadIdx.x;
    const FfHead h = *a.fhead;
    if (k >= h.n_runs || k >= a.run_cap) return;   // n_runs <= n
    const uint64_t next = k + 1u < h.n_runs ? a.runat[k + 1u] : h.total;
    a.runs[k].len = next - a.runat[k];
}

__global__ __launch_bounds__(kFfThreads) void bt_flowfollow_copy(FlowfollowArgs a) {
    __shared__ uint32_t r_off[kFtWaves][65];   // per wave: the tile's pairs' offsets from the tile's first byte
    __shared__ uint64_t r_src[kFtWaves][64];   // ... each pair's first delivered byte, from base
    const uint32_t tid = threadIdx.x, lane = tid & 63u, wid = tid >> 6;
    const uint32_t u = blockIdx.x * kFtWaves + wid;
    const uint32_t m = a.head->m;
    const uint64_t p0 = (uint64_t)u * kFsUnit;
    if (p0 >= m) return;   // the whole wave; no block-wide step below
    const uintptr_t out0 = reinterpret_cast<uintptr_t>(a.out);
    for (uint32_t k = 0; k < kFsUnitTiles && p0 + k * 64u < m; ++k) {
        const uint64_t p = p0 + k * 64u + lane;
        const uint64_t pc = p < m ? p : m;   // at[m] = total: a lane off the list is empty
        const uint64_t at = a.at[pc];
        const uint64_t src = p < m ? a.src[p] : 0ull;
        const uint64_t q = p0 + k * 64u + 64u;
        const uint64_t end = a.at[q < m ? q : m];   // the same word in every lane
        const uint64_t g0 = ((uint64_t)(uint32_t)__builtin_amdgcn_readlane((int)(uint32_t)(at >> 32), 0) << 32) |
                            (uint32_t)__builtin_amdgcn_readlane((int)(uint32_t)at, 0);
        if (g0 >= a.cap) break;   // the offsets ascend: nothing of the rest of the unit fits
        uint64_t g1 = end < a.cap ? end : a.cap;
        if (g1 <= g0) continue;
        wave_lds_sync();   // the previous tile's reads of the rows are done
        r_off[wid][lane] = (uint32_t)(at - g0);   // a tile's bytes are below 2^23
        if (lane == 63) r_off[wid][64] = (uint32_t)(end - g0);
        r_src[wid][lane] = src;
        wave_lds_sync();
        // the tile's destination bytes [g0, g1) as 16-B lines of the output
        const uintptr_t a0 = out0 + g0, a1 = out0 + g1;
        const uintptr_t first = a0 & ~(uintptr_t)15;
        const uint64_t lines = (a1 - first + 15u) >> 4;
        for (uint64_t j = lane; j < lines; j += 64u) {
            const uintptr_t line = first + 16u * j;
            uint8_t* const dst = a.out + (int64_t)(line - out0);   // a line may start before out: bytes below lo are not written
            const uintptr_t lo = line > a0 ? line : a0;
            const uintptr_t hi = line + 16u < a1 ? line + 16u : a1;
            const uint32_t d = (uint32_t)(lo - a0);   // offset of the first byte from the tile's first
            uint32_t r = 0;                           // the last pair that starts at or before d: it holds byte d
#pragma unroll
            for (uint32_t step = 32u; step; step >>= 1)
                if (r_off[wid][r + step] <= d) r += step;
            const bool whole = hi - lo == 16u;
            if (whole && d + 16u <= r_off[wid][r + 1u]) {   // inside one segment's bytes
                const uint64_t s = r_src[wid][r] + (d - r_off[wid][r]);
                if (s <= a.bytes && a.bytes - s >= 16u) {
                    const u32x4 v = __builtin_nontemporal_load(reinterpret_cast<const u32x4_any*>(a.base + s));
                    __builtin_nontemporal_store(v, reinterpret_cast<u32x4*>(dst));
                    continue;
                }
            }
            // byte by byte: seams, the edges of the tile, of the source buffer and of cap
            uint32_t v[4] = {0u, 0u, 0u, 0u};
            const uint32_t b0 = (uint32_t)(lo - line), nb = (uint32_t)(hi - lo);
            for (uint32_t b = 0; b < nb; ++b) {
                const uint32_t dd = d + b;
                while (r < 63u && r_off[wid][r + 1u] <= dd) ++r;
                const uint64_t s = r_src[wid][r] + (dd - r_off[wid][r]);
                const uint32_t byte = s < a.bytes ? a.base[s] : 0u;
                const uint32_t qb = b0 + b;
                v[qb >> 2] |= byte << ((qb & 3u) * 8u);
            }
            if (nb == 16u) {
                const u32x4 x = {v[0], v[1], v[2], v[3]};
                __builtin_nontemporal_store(x, reinterpret_cast<u32x4*>(dst));
            } else {
                for (uint32_t qb = b0; qb < b0 + nb; ++qb) dst[qb] = (uint8_t)(v[qb >> 2] >> ((qb & 3u) * 8u));
            }
        }
    }
}

int launch_flowfollow(const FlowfollowArgs& f, void* stream, void* e_sum, void* e_copy) {
    if (f.n == 0 || f.nchunks == 0) return BT_OK;
    hipStream_t st = reinterpret_cast<hipStream_t>(stream);
    hipEvent_t e0 = reinterpret_cast<hipEvent_t>(e_sum), e1 = reinterpret_cast<hipEvent_t>(e_copy);
    const dim3 grid(f.nchunks), block(kFfThreads);
    launch(bt_flowfollow_sum<kFfCarryMode>, grid, block, 0, st, e0, nullptr, f);
    launch(bt_flowfollow_join, dim3(1), dim3(kFsJoinThreads), 0, st, nullptr, nullptr, f);
    launch(bt_flowfollow_sum<kFfEmit>, grid, block, 0, st, nullptr, nullptr, f);
    const uint32_t lanes = f.run_cap < f.n ? f.run_cap : f.n;   // n_runs <= n
    if (lanes) launch(bt_flowfollow_runs, dim3((lanes + 255u) / 256u), dim3(256), 0, st, nullptr, nullptr, f);
    if (f.cap)
        launch(bt_flowfollow_copy, grid, block, 0, st, e1, nullptr, f);
    else if (e1 && hipEventRecord(e1, st) != hipSuccess)
        return BT_E_INTERNAL;
    return hipGetLastError() == hipSuccess ? BT_OK : BT_E_INTERNAL;
}

}  // namespace bt
