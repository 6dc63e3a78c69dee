// bt_flowtop.hip — the top-K query over a flow tracker (bt_flow_track_top_device,
// include/beatrice_gpu.h): the k largest flows of a device-resident tracker state by a u64 value
// computed from each record, in the order (value descending, flow number ascending), selected,
// ordered and gathered without the host. The state and the side table are only read.
//   bt_flowtop_begin    one block: the header check, n_flows and n_top = min(k, n_flows) into the
//                       control block, every histogram zero.
//   bt_flowtop_value    grid-stride, a bounded grid: value[f] for every flow, dense in the scratch
//                       (the later passes read 8 B per flow, not a 104-byte stride), the block's
//                       sum into `total`, and the histogram of the most significant byte.
//   bt_flowtop_hist     (digits 1 .. 7) the flows whose higher digits equal the prefix found so far
//                       count their next byte. Counts are combined in the wave (lanes that agree
//                       with the first counting lane add once), then in the block's 256 LDS bins,
//                       and a block adds each non-empty bin to the global histogram once: a table
//                       of equal values costs one LDS add per wave and one global add per block.
//   bt_flowtop_pick     one block scans the 256 bins from the top and finds the digit at which the
//                       running count reaches the flows still needed; the extended prefix, the
//                       need left among that bin's flows and the bin's count go to the control
//                       block. After eight digits the prefix is the threshold exactly, the need is
//                       how many of the ties enter, and the bin's count is n_ties.
//   bt_flowtop_count    one thread per flow: ballot counts of value > threshold and == threshold
//                       per wave and block; _scan (one block): the exclusive scans of both;
//                       _collect: the flows above the threshold in flow order, then the first
//                       `need` ties in flow order, into cand[0 .. n_top) as (value, id).
//   bt_flowtop_sort     one block: a bitonic sort of the candidates in LDS by (value descending,
//                       id ascending), top_id / top_value, the gather of top / top_tcp from the
//                       state, top_total and *result by plain stores.
// No lane waits for another lane, wave or block: no spin, no flag, no look-back; what one kernel
// tells the next goes through the kernel boundary, and every loop has its bound in its head. Why
// the outputs are the same from run to run: the histograms and `total` are integer sums, the
// candidates' places come from ordered scans, and the sort's key (value, id) is total.
#include "bt_flowtrack_dev.h"
#include "bt_hip_launch.h"
#include "bt_wave.h"
#include "bt_flowtop.h"

namespace bt {

namespace {

constexpr uint32_t kSortWaves = kTopSortThreads / 64u;
constexpr uint64_t kSpan = (uint64_t)kFkThreads * kTopUnroll;   // flows a block of a grid-stride pass takes per step

// Every lane with `on` counts in bin d of the block's LDS histogram. Called by whole waves. The
// lanes that agree with the first counting lane add once for all of them.
__device__ __forceinline__ void hist_add(uint32_t* h, bool on, uint32_t d) {
    const uint64_t m = __ballot(on);
    if (!m) return;
    const uint32_t first = (uint32_t)__ffsll((unsigned long long)m) - 1u;
    const uint32_t d0 = __shfl(d, (int)first);
    const bool with_first = on && d == d0;
    const uint64_t same = __ballot(with_first);
    if (with_first) {
        if ((threadIdx.x & 63u) == first) atomicAdd(&h[d0], (uint32_t)__popcll(same));
    } else if (on) {
        atomicAdd(&h[d], 1u);
    }
}

__device__ __forceinline__ void hist_flush(const uint32_t* h, uint32_t* global) {   // behind a __syncthreads
    const uint32_t c = h[threadIdx.x];
    if (c) atomicAdd(&global[threadIdx.x], c);
}

// Does (xv, xi) stand before (yv, yi) in the top's order?
__device__ __forceinline__ bool before(uint64_t xv, uint32_t xi, uint64_t yv, uint32_t yi) {
    return xv != yv ? xv > yv : xi < yi;
}

}  // namespace

static_assert(kTopBins == kFkThreads, "one thread per bin in the histogram kernels");

// T0: the control block and zero histograms.
__global__ __launch_bounds__(kFkThreads) void bt_flowtop_begin(FlowtopArgs a) {
    const uint32_t tid = threadIdx.x;
    for (uint32_t i = tid; i < kTopDigits * kTopBins; i += kFkThreads) a.hist[i] = 0u;
    if (tid == 0) {
        const bool ok = hdr_ok(a, a.slots);
        const uint32_t nf = ok ? a.hdr->n_flows : 0u, n_top = a.k < nf ? a.k : nf;
        *a.ctl = FtopCtl{ok ? 1u : 0u, nf, n_top, n_top, 0u, 0u, 0ull, 0ull};
    }
}

// T1: every flow's value, their sum, the histogram of the top byte.
__global__ __launch_bounds__(kFkThreads) void bt_flowtop_value(FlowtopArgs a) {
    __shared__ uint32_t h[kTopBins];
    __shared__ uint64_t sh[kFkWaves];
    if (!a.ctl->ok) return;
    const uint32_t nf = a.ctl->n_flows, tid = threadIdx.x;
    h[tid] = 0u;
    __syncthreads();
    const uint64_t step = (uint64_t)gridDim.x * kSpan;
    uint64_t sum = 0;
    for (uint64_t f0 = (uint64_t)blockIdx.x * kSpan; f0 < nf; f0 += step) {   // f < nf <= flow_cap
        uint64_t v[kTopUnroll];
#pragma unroll
        for (uint32_t u = 0; u < kTopUnroll; ++u) {
            const uint64_t f = f0 + u * kFkThreads + tid;
            v[u] = f < nf ? ftop_value(a.metric, a.recs[f], a.tcp ? a.tcp + f : nullptr) : 0ull;
        }
#pragma unroll
        for (uint32_t u = 0; u < kTopUnroll; ++u) {
            const uint64_t f = f0 + u * kFkThreads + tid;
            const bool on = f < nf;
            if (on) a.value[f] = v[u];
            sum += v[u];
            hist_add(h, on, (uint32_t)(v[u] >> 56));
        }
    }
    const uint64_t tot = block_sum64<kFkThreads>(sum, sh);   // its barriers also close the histogram
    if (tid == 0 && tot) atomicAdd(reinterpret_cast<unsigned long long*>(&a.ctl->total), (unsigned long long)tot);
    hist_flush(h, a.hist);
}

// T2: digit p (1 .. 7) of the flows whose p higher digits equal the prefix.
__global__ __launch_bounds__(kFkThreads) void bt_flowtop_hist(FlowtopArgs a, uint32_t p) {
    __shared__ uint32_t h[kTopBins];
    if (!a.ctl->ok || !a.ctl->n_top) return;
    const uint32_t nf = a.ctl->n_flows, tid = threadIdx.x;
    const uint64_t prefix = a.ctl->prefix;
    const uint32_t above = 64u - 8u * p, at = 56u - 8u * p;   // 8 <= above <= 56
    h[tid] = 0u;
    __syncthreads();
    const uint64_t step = (uint64_t)gridDim.x * kSpan;
    for (uint64_t f0 = (uint64_t)blockIdx.x * kSpan; f0 < nf; f0 += step) {   // f < nf <= flow_cap
        uint64_t v[kTopUnroll];
#pragma unroll
        for (uint32_t u = 0; u < kTopUnroll; ++u) {
            const uint64_t f = f0 + u * kFkThreads + tid;
            v[u] = f < nf ? a.value[f] : 0ull;
        }
#pragma unroll
        for (uint32_t u = 0; u < kTopUnroll; ++u) {
            const uint64_t f = f0 + u * kFkThreads + tid;
            hist_add(h, f < nf && (v[u] >> above) == prefix, (uint32_t)(v[u] >> at) & 255u);
        }
    }
    __syncthreads();
    hist_flush(h, a.hist + p * kTopBins);
}

// T3: the digit p at which the count from the top reaches the need.
__global__ __launch_bounds__(kFkThreads) void bt_flowtop_pick(FlowtopArgs a, uint32_t p) {
    __shared__ uint32_t sh[kFkWaves];
    if (!a.ctl->ok || !a.ctl->n_top) return;
    const uint32_t need = a.ctl->need, n_top = a.ctl->n_top, bin = kTopBins - 1u - threadIdx.x;
    const uint64_t prefix = a.ctl->prefix;
    const uint32_t c = a.hist[p * kTopBins + bin];
    uint32_t total = 0;
    const uint32_t excl = block_excl<kFkThreads>(c, sh, &total);   // flows in the bins above this one; its barrier follows the reads
    if (excl < need && need - excl <= c) {   // one thread: 1 <= need <= the flows that match the prefix
        a.ctl->prefix = prefix << 8 | bin;
        a.ctl->need = need - excl;
        a.ctl->ties = c;
        if (p == kTopDigits - 1u) a.ctl->n_gt = n_top - (need - excl);
    }
}

// T4: how many flows of each block lie above and at the threshold.
__global__ __launch_bounds__(kFkThreads) void bt_flowtop_count(FlowtopArgs a) {
    __shared__ uint32_t wg[kFkWaves], we[kFkWaves];
    if (!a.ctl->ok || !a.ctl->n_top) return;
    const uint64_t f0 = (uint64_t)blockIdx.x * kFkThreads;
    const uint32_t nf = a.ctl->n_flows;
    if (f0 >= nf) return;
    const uint64_t thr = a.ctl->prefix;
    const uint32_t tid = threadIdx.x, lane = tid & 63u, wid = tid >> 6;
    const uint64_t f = f0 + tid;
    const uint64_t v = f < nf ? a.value[f] : 0ull;
    const uint32_t ng = (uint32_t)__popcll(__ballot(f < nf && v > thr)), ne = (uint32_t)__popcll(__ballot(f < nf && v == thr));
    if (lane == 0) { wg[wid] = ng; we[wid] = ne; }
    __syncthreads();
    if (tid == 0) {
        FtopPart part{};
#pragma unroll
        for (uint32_t w = 0; w < kFkWaves; ++w) { part.wgt[w] = wg[w]; part.ngt += wg[w]; part.weq[w] = we[w]; part.neq += we[w]; }
        a.parts[blockIdx.x] = part;
    }
}

// T5: where every block's flows above and at the threshold start.
__global__ __launch_bounds__(kTopSortThreads) void bt_flowtop_scan(FlowtopArgs a) {
    __shared__ uint32_t sh[kSortWaves];
    if (!a.ctl->ok || !a.ctl->n_top) return;
    const uint32_t tid = threadIdx.x, nf = a.ctl->n_flows;
    const uint32_t nparts = (uint32_t)(((uint64_t)nf + kFkThreads - 1u) / kFkThreads), per = (nparts + kTopSortThreads - 1u) / kTopSortThreads;
    const uint32_t lo = (uint64_t)tid * per < nparts ? tid * per : nparts, hi = nparts - lo > per ? lo + per : nparts;
    uint32_t sg = 0, se = 0;
    for (uint32_t q = lo; q < hi; ++q) { sg += a.parts[q].ngt; se += a.parts[q].neq; }
    uint32_t total = 0;
    uint32_t rg = block_excl<kTopSortThreads>(sg, sh, &total);
    uint32_t re = block_excl<kTopSortThreads>(se, sh, &total);
    for (uint32_t q = lo; q < hi; ++q) {
        a.parts[q].rel_gt = rg; a.parts[q].rel_eq = re;
        rg += a.parts[q].ngt; re += a.parts[q].neq;
    }
}

// T6: the flows above the threshold, then the first `need` at it, both in flow order, as candidates.
__global__ __launch_bounds__(kFkThreads) void bt_flowtop_collect(FlowtopArgs a) {
    if (!a.ctl->ok || !a.ctl->n_top) return;
    const uint64_t f0 = (uint64_t)blockIdx.x * kFkThreads;
    const uint32_t nf = a.ctl->n_flows;
    if (f0 >= nf) return;
    const uint32_t need = a.ctl->need, n_gt = a.ctl->n_gt, n_top = a.ctl->n_top;
    const FtopPart& part = a.parts[blockIdx.x];
    if (!part.ngt && (!part.neq || part.rel_eq >= need)) return;   // the whole block: nothing of it enters
    const uint64_t thr = a.ctl->prefix;
    const uint32_t tid = threadIdx.x, lane = tid & 63u, wid = tid >> 6;
    const uint64_t f = f0 + tid;
    const uint64_t v = f < nf ? a.value[f] : 0ull;   // as bt_flowtop_count saw it
    const bool gt = f < nf && v > thr, eq = f < nf && v == thr;
    const uint64_t below = (1ull << lane) - 1ull;
    uint32_t bg = part.rel_gt + (uint32_t)__popcll(__ballot(gt) & below), be = part.rel_eq + (uint32_t)__popcll(__ballot(eq) & below);
    for (uint32_t w = 0; w < wid; ++w) { bg += part.wgt[w]; be += part.weq[w]; }
    uint32_t to = n_top;
    if (gt) to = bg;                       // bg < n_gt
    else if (eq && be < need) to = n_gt + be;   // n_gt + need = n_top
    if (to < n_top) {                      // n_top <= k: inside the candidates
        a.cand_value[to] = v;
        a.cand_id[to] = (uint32_t)f;
    }
}

// T7: the candidates in the top's order, the outputs and *result.
__global__ __launch_bounds__(kTopSortThreads) void bt_flowtop_sort(FlowtopArgs a) {
    __shared__ uint64_t sv[BT_FLOW_TOP_MAX_K];
    __shared__ uint32_t si[BT_FLOW_TOP_MAX_K];
    __shared__ uint64_t sh[kSortWaves];
    const uint32_t tid = threadIdx.x;
    if (!a.ctl->ok) {
        if (tid == 0) {
            bt_flow_top_result r{};
            r.status = 1u;
            *a.result = r;
        }
        return;
    }
    const uint32_t n_top = a.ctl->n_top < BT_FLOW_TOP_MAX_K ? a.ctl->n_top : BT_FLOW_TOP_MAX_K;   // n_top <= k <= BT_FLOW_TOP_MAX_K
    uint32_t n2 = 1;   // the power of two the sort runs over
    for (uint32_t b = 0; b < 12u && n2 < n_top; ++b) n2 <<= 1;
    for (uint32_t i = tid; i < n2; i += kTopSortThreads) {
        const bool live = i < n_top;
        sv[i] = live ? a.cand_value[i] : 0ull;          // a pad stands behind every flow: no flow number is 0xFFFFFFFF
        si[i] = live ? a.cand_id[i] : 0xFFFFFFFFu;
    }
    __syncthreads();
    for (uint32_t size = 2; size <= n2; size <<= 1) {
        for (uint32_t stride = size >> 1; stride > 0; stride >>= 1) {
            for (uint32_t t = tid; t < n2 / 2u; t += kTopSortThreads) {
                const uint32_t i = 2u * t - (t & (stride - 1u)), j = i + stride;   // j < n2
                const uint64_t vi = sv[i], vj = sv[j];
                const uint32_t ii = si[i], ij = si[j];
                const bool up = (i & size) == 0u;
                if (up ? before(vj, ij, vi, ii) : before(vi, ii, vj, ij)) {
                    sv[i] = vj; si[i] = ij;
                    sv[j] = vi; si[j] = ii;
                }
            }
            __syncthreads();
        }
    }
    uint64_t sum = 0;
    for (uint32_t r = tid; r < n_top; r += kTopSortThreads) {
        const uint32_t id = si[r];
        const uint64_t v = sv[r];
        sum += v;
        if (a.top_id) a.top_id[r] = id;
        if (a.top_value) a.top_value[r] = v;
        if (id < a.flow_cap) {   // every candidate is a flow number below n_flows
            if (a.top) rec_copy(a.top + r, a.recs + id);
            if (a.top_tcp) tcp_copy(a.top_tcp + r, a.tcp + id);
        }
    }
    const uint64_t top_total = block_sum64<kTopSortThreads>(sum, sh);
    if (tid == 0) {
        bt_flow_top_result r{};
        r.n_flows = a.ctl->n_flows; r.n_top = n_top; r.metric = a.metric;
        r.n_ties = n_top ? a.ctl->ties : 0u;
        r.threshold = n_top ? a.ctl->prefix : 0ull;
        r.total = a.ctl->total; r.top_total = top_total;
        *a.result = r;
    }
}

int launch_flowtop(const FlowtopArgs& a, void* stream, void* timing_start, void* timing_stop) {
    hipStream_t st = reinterpret_cast<hipStream_t>(stream);
    hipEvent_t e0 = reinterpret_cast<hipEvent_t>(timing_start), e1 = reinterpret_cast<hipEvent_t>(timing_stop);
    const uint32_t per_flow = (uint32_t)(((uint64_t)a.flow_cap + kFkThreads - 1u) / kFkThreads);   // flow_cap < 2^32
    const uint64_t spans = ((uint64_t)a.flow_cap + kSpan - 1u) / kSpan;
    const uint32_t strided = (uint32_t)(spans > kTopMaxGrid ? kTopMaxGrid : spans ? spans : 1u);
    launch(bt_flowtop_begin, dim3(1), dim3(kFkThreads), 0, st, e0, nullptr, a);
    launch(bt_flowtop_value, dim3(strided), dim3(kFkThreads), 0, st, nullptr, nullptr, a);
    if (a.k) {   // k == 0: no top, the sort kernel writes n_flows and total
        for (uint32_t p = 0; p < kTopDigits; ++p) {
            if (p) launch(bt_flowtop_hist, dim3(strided), dim3(kFkThreads), 0, st, nullptr, nullptr, a, p);
            launch(bt_flowtop_pick, dim3(1), dim3(kFkThreads), 0, st, nullptr, nullptr, a, p);
        }
        launch(bt_flowtop_count, dim3(per_flow), dim3(kFkThreads), 0, st, nullptr, nullptr, a);
        launch(bt_flowtop_scan, dim3(1), dim3(kTopSortThreads), 0, st, nullptr, nullptr, a);
        launch(bt_flowtop_collect, dim3(per_flow), dim3(kFkThreads), 0, st, nullptr, nullptr, a);
    }
    launch(bt_flowtop_sort, dim3(1), dim3(kTopSortThreads), 0, st, nullptr, e1, a);
    return hipGetLastError() == hipSuccess ? BT_OK : BT_E_INTERNAL;
}

}  // namespace bt
