// bt_flowtrack.hip — the flow tracker (bt_flow_track_*_device, include/beatrice_gpu.h): a flow
// table that lives across batches in the caller's device memory. The state (bt_flowtrack.h) is a
// header, flow_cap dense records (record f is flow number f) and `slots` slot words, open
// addressing with linear probing: a slot is empty or holds a flow number, and the key it stands
// for is that record's.
//
// An update runs the per-batch table's kernels unchanged (launch_flowtab, bt_flowtab.hip) into the
// scratch with flow_cap = n, which leaves the batch's flows as a duplicate-free list of keys in
// order of first appearance, and then merges that list: one thread per flow of the batch, blocks
// of 4 waves, a thread at or past the batch's flow count does nothing.
//   bt_flowtrack_find   probes the table from a hash of the flow's key (fk_hash, bt_flowtrack.h;
//                       at most `slots` steps): an empty slot means the flow is new, otherwise the
//                       class and the 36 key bytes are compared with recs[id]. map[j] = the flow's
//                       number or "new"; ballot counts of the new flows per wave and block, and
//                       the new flows' packets and bytes per block. Nothing of the state is written.
//   bt_flowtrack_join   one block: the exclusive scan of the blocks' counts; base = n_flows before
//                       the call and the room left; the new flows at or past the room overflow,
//                       and their packets and bytes are the sums of the blocks behind the cut plus
//                       those of the one block the cut goes through, which this block re-ranks
//                       itself. The header (n_flows, the sequence number, the running totals) and
//                       *result, by one thread with plain loads and stores.
//   bt_flowtrack_apply  a found flow adds itself to its record with plain loads and stores: the
//                       batch's keys are distinct, so no other thread touches that record. A new
//                       flow below the cap writes its whole record at base + rank and claims the
//                       first empty slot on its probe sequence with a device-scope atomicCAS, with
//                       no key compare: every occupied slot, old or claimed during this kernel,
//                       holds another key, because this key was not in the old table and the
//                       batch's keys are distinct.
//   bt_flowtrack_ids    (only with out->flow_id) the per-batch numbers through map[].
// An expire: bt_flowexpire_mark (idle bits as ballot counts), _scan (one block: the scan, how many
// leave, the header and *result), _move (the live records to their new place in the scratch, the
// leaving ones to expired[], remap[]), _back (the scratch back into the state, zeros behind the
// live records, every slot empty), _claim (the live records claim their slots as above; their keys
// are distinct). When nothing leaves, the last three change nothing. The TCP-aware expire
// (bt_flowexpire_tcp_mark, _tcp_move, _tcp_back with the same _scan and _claim) also lets closed and
// reset connections leave after a shorter time and moves the TCP side table with the records.
//
// No lane ever waits for another lane, wave or block: there is no spin, no flag and no look-back,
// and every loop has a bound in its head; a probe takes at most `slots` steps. Why the outputs are
// the same from run to run: which slot a new flow gets varies with the order of the CAS, and
// nothing else does. A flow's number is base + its rank among the batch's new flows in batch
// order, sums are integer sums by the one thread that owns the record, and a later lookup finds a
// key wherever on its probe sequence it sits, since no slot between its hash and its slot was
// empty when it was claimed and slots are only emptied all at once (expire). The slot words are
// private to the state. Across the XCDs' L2s: the kernels read only atomics' results and data
// written by earlier kernels.
#include "bt_flowtrack_dev.h"
#include "bt_hip_launch.h"
#include "bt_wave.h"

namespace bt {

namespace {

constexpr uint32_t kJoinWaves = kFkJoinThreads / 64u;
constexpr uint32_t kNone = 0xFFFFFFFFu;

// The first 40 bytes of a bt_flow_rec or a bt_flow_track_rec (8-byte aligned): key, class, zeros.
__device__ __forceinline__ void head_load(const void* p, uint32_t (&w)[10]) {
    const uint64_t* const q = static_cast<const uint64_t*>(p);
#pragma unroll
    for (int j = 0; j < 5; ++j) {
        const uint64_t x = q[j];
        w[2 * j] = (uint32_t)x;
        w[2 * j + 1] = (uint32_t)(x >> 32);
    }
}

// Flow g takes the first empty slot on the probe sequence of `hash`. A slot changes once, from
// empty to its final value: a value other than empty is final wherever it is read from, and empty
// is confirmed by the CAS. At most n_flows <= slots flows claim, so there is a slot.
__device__ __forceinline__ void claim(uint32_t* slot, uint32_t slots, uint32_t hash, uint32_t g) {
    const uint32_t mask = slots - 1u;
    uint32_t s = hash & mask;
    for (uint32_t probe = 0; probe < slots; ++probe) {
        const uint32_t v = __hip_atomic_load(&slot[s], __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
        if (v == kFkEmpty && atomicCAS(&slot[s], kFkEmpty, g) == kFkEmpty) return;
        s = (s + 1u) & mask;
    }
}

}  // namespace

// The header, zero records and empty slots: the whole state, grid-stride.
__global__ __launch_bounds__(kFkThreads) void bt_flowtrack_init(FlowexpArgs a) {
    const uint64_t t = (uint64_t)blockIdx.x * kFkThreads + threadIdx.x, step = (uint64_t)gridDim.x * kFkThreads;
    if (t == 0) {
        bt_flow_track_hdr h{};
        h.magic = BT_FLOW_TRACK_MAGIC; h.flags = a.flags; h.flow_cap = a.flow_cap; h.slots = a.slots;
        *a.hdr = h;
    }
    uint64_t* const r = reinterpret_cast<uint64_t*>(a.recs);
    const uint64_t nr = (uint64_t)a.flow_cap * (sizeof(bt_flow_track_rec) / 8u);
    for (uint64_t x = t; x < nr; x += step) r[x] = 0ull;
    slots_fill<kFkThreads>(a.slot, a.slots, kFkEmpty);
}

// U1: is the batch's flow j in the table?
__global__ __launch_bounds__(kFkThreads) void bt_flowtrack_find(FlowtrackArgs a) {
    __shared__ uint32_t wn[kFkWaves];
    __shared__ uint64_t wp[kFkWaves], wb[kFkWaves];
    if (!hdr_ok(a, a.slots)) return;
    const uint32_t have = a.ftres->n_flows, nb = have < a.n ? have : a.n;   // written by bt_flowtab_join
    const uint32_t j0 = blockIdx.x * kFkThreads;
    if (j0 >= nb) return;
    const uint32_t tid = threadIdx.x, lane = tid & 63u, wid = tid >> 6, j = j0 + tid;
    const bool act = j < nb;
    uint32_t w[10];
#pragma unroll
    for (int d = 0; d < 10; ++d) w[d] = 0u;
    uint64_t pk = 0, by = 0;
    uint32_t found = kFkNew;
    if (act) {
        head_load(a.flows + j, w);
        const uint64_t* const q = reinterpret_cast<const uint64_t*>(a.flows + j);
        const uint64_t p = q[6];
        pk = (p & 0xFFFFFFFFull) + (p >> 32);
        by = q[7] + q[8];
        const uint32_t mask = a.slots - 1u;
        uint32_t s = fk_hash(w) & mask;
        for (uint32_t probe = 0; probe < a.slots; ++probe) {   // every slot once at the most
            const uint32_t id = a.slot[s];   // written by earlier kernels only
            if (id == kFkEmpty) break;
            if (id < a.flow_cap) {
                uint32_t o[10];
                head_load(a.recs + id, o);
                bool same = true;
#pragma unroll
                for (int d = 0; d < 10; ++d) same = same && o[d] == w[d];
                if (same) { found = id; break; }
            }
            s = (s + 1u) & mask;
        }
        a.map[j] = found;
    }
    const bool isnew = act && found == kFkNew;
    const uint32_t cnt = (uint32_t)__popcll(__ballot(isnew));
    const uint64_t sp = wave_sum64(isnew ? pk : 0ull), sb = wave_sum64(isnew ? by : 0ull);
    if (lane == 0) { wn[wid] = cnt; wp[wid] = sp; wb[wid] = sb; }
    __syncthreads();
    if (tid == 0) {
        FkPart p{};
#pragma unroll
        for (uint32_t v = 0; v < kFkWaves; ++v) {
            p.wnew[v] = wn[v];
            p.nnew += wn[v];
            p.new_packets += wp[v];
            p.new_bytes += wb[v];
        }
        a.parts[blockIdx.x] = p;
    }
}

// U2: where every block's new flows start, what overflows, the header and *result.
__global__ __launch_bounds__(kFkJoinThreads) void bt_flowtrack_join(FlowtrackArgs a) {
    __shared__ uint32_t sh[kJoinWaves];
    __shared__ uint64_t sh64[kJoinWaves];
    __shared__ uint32_t cut[2];   // the block the room ends in, and where its new flows start
    const uint32_t tid = threadIdx.x, lane = tid & 63u, wid = tid >> 6;
    if (!hdr_ok(a, a.slots)) {   // not this tracker's state: nothing is done
        if (tid == 0) {
            if (!a.empty) *a.ctl = FkCtl{0u, 0u, 0u, 0u};
            bt_flow_track_result r{};
            r.n = a.n;
            r.status = 1u;
            *a.result = r;
        }
        return;
    }
    const uint32_t have = a.empty ? 0u : a.ftres->n_flows, nb = have < a.n ? have : a.n;
    const uint32_t nparts = (nb + kFkThreads - 1u) / kFkThreads, per = (nparts + kFkJoinThreads - 1u) / kFkJoinThreads;
    const uint32_t lo = tid * per < nparts ? tid * per : nparts, hi = lo + per < nparts ? lo + per : nparts;
    uint32_t sum = 0;
    for (uint32_t p = lo; p < hi; ++p) sum += a.parts[p].nnew;
    uint32_t total = 0;
    const uint32_t excl = block_excl<kFkJoinThreads>(sum, sh, &total);
    const uint32_t base = a.hdr->n_flows, room = a.flow_cap - base;
    if (tid == 0) cut[0] = kNone;
    __syncthreads();
    uint32_t run = excl;
    uint64_t op = 0, ob = 0;
    for (uint32_t p = lo; p < hi; ++p) {
        FkPart& q = a.parts[p];
        q.rel = run;
        if (run >= room) { op += q.new_packets; ob += q.new_bytes; }   // the whole block overflows
        else if (run + q.nnew > room) { cut[0] = p; cut[1] = run; }     // at most one block
        run += q.nnew;
    }
    __syncthreads();
    const uint32_t cp = cut[0];
    if (cp != kNone && tid < kFkThreads) {   // the block the cut goes through, ranked as bt_flowtrack_apply ranks it
        const uint32_t j = cp * kFkThreads + tid;
        const bool isnew = j < nb && a.map[j] == kFkNew;
        const uint64_t word = __ballot(isnew);
        uint32_t rank = cut[1] + (uint32_t)__popcll(word & ((1ull << lane) - 1ull));
        for (uint32_t v = 0; v < wid; ++v) rank += a.parts[cp].wnew[v];
        if (isnew && rank >= room) {
            const uint64_t* const q = reinterpret_cast<const uint64_t*>(a.flows + j);
            const uint64_t p = q[6];
            op += (p & 0xFFFFFFFFull) + (p >> 32);
            ob += q[7] + q[8];
        }
    }
    op = block_sum64<kFkJoinThreads>(op, sh64);
    ob = block_sum64<kFkJoinThreads>(ob, sh64);
    if (tid == 0) {
        bt_flow_track_hdr* const h = a.hdr;
        const uint32_t newf = total < room ? total : room, seq = h->seq;
        bt_flow_track_result r{};
        r.n = a.n;
        if (!a.empty) {
            const bt_flow_table_result* const f = a.ftres;
            r.n_selected = f->n_selected; r.none_packets = f->none_packets;
            r.keyed_bytes = f->keyed_bytes; r.none_bytes = f->none_bytes;
            *a.ctl = FkCtl{1u, base, seq, room};
        }
        r.batch_flows = nb; r.new_flows = newf; r.overflow_flows = total - newf;
        r.overflow_packets = (uint32_t)op; r.overflow_bytes = ob;
        r.n_flows = base + newf; r.seq = seq;
        h->n_flows = base + newf;
        h->seq = seq + 1u;
        h->selected_packets += r.n_selected; h->keyed_packets += r.n_selected - r.none_packets;
        h->none_packets += r.none_packets; h->overflow_packets += r.overflow_packets;
        h->selected_bytes += r.keyed_bytes + r.none_bytes; h->keyed_bytes += r.keyed_bytes;
        h->none_bytes += r.none_bytes; h->overflow_bytes += ob;
        *a.result = r;
    }
}

// U3: found flows add themselves to their record, new flows write theirs and claim a slot.
__global__ __launch_bounds__(kFkThreads) void bt_flowtrack_apply(FlowtrackArgs a) {
    const FkCtl ctl = *a.ctl;   // written by bt_flowtrack_join
    if (!ctl.ok) return;
    const uint32_t have = a.ftres->n_flows, nb = have < a.n ? have : a.n;
    const uint32_t j0 = blockIdx.x * kFkThreads;
    if (j0 >= nb) return;
    const uint32_t tid = threadIdx.x, lane = tid & 63u, wid = tid >> 6, j = j0 + tid;
    const bool act = j < nb;
    const uint32_t m = act ? a.map[j] : 0u;
    const bool isnew = act && m == kFkNew;
    const uint64_t word = __ballot(isnew);
    if (!act) return;
    const FkPart& part = a.parts[blockIdx.x];
    uint32_t rank = part.rel + (uint32_t)__popcll(word & ((1ull << lane) - 1ull));
    for (uint32_t v = 0; v < wid; ++v) rank += part.wnew[v];
    const uint64_t* const q = reinterpret_cast<const uint64_t*>(a.flows + j);
    const uint64_t fl = q[5], pk = q[6], b0 = q[7], b1 = q[8];
    const uint32_t first = (uint32_t)fl, last = (uint32_t)(fl >> 32);   // packet indices of this batch: below n
    const uint64_t last_ts = a.ts ? a.ts[last < a.n ? last : 0u] : a.batch_ts;
    if (!isnew) {
        if (m >= a.flow_cap) return;
        uint64_t* const o = reinterpret_cast<uint64_t*>(a.recs + m);   // this thread alone has the record's key
        o[5] = (o[5] & 0xFFFFFFFFull) | (uint64_t)ctl.seq << 32;       // last_batch
        o[6] = (o[6] & 0xFFFFFFFFull) | (uint64_t)last << 32;          // last
        o[7] += pk & 0xFFFFFFFFull; o[8] += pk >> 32;
        o[9] += b0; o[10] += b1;
        o[12] = last_ts;
        return;
    }
    if (rank >= ctl.room) {   // no room: not inserted
        a.map[j] = BT_FLOW_ID_OVERFLOW;
        return;
    }
    const uint32_t g = ctl.base + rank;   // below flow_cap
    uint32_t w[10];
    head_load(q, w);
    uint64_t* const o = reinterpret_cast<uint64_t*>(a.recs + g);
#pragma unroll
    for (int d = 0; d < 5; ++d) o[d] = q[d];
    o[5] = (uint64_t)ctl.seq << 32 | ctl.seq;
    o[6] = fl;
    o[7] = pk & 0xFFFFFFFFull; o[8] = pk >> 32;
    o[9] = b0; o[10] = b1;
    o[11] = a.ts ? a.ts[first < a.n ? first : 0u] : a.batch_ts;
    o[12] = last_ts;
    claim(a.slot, a.slots, fk_hash(w), g);
    a.map[j] = g;
}

// U4: every packet's flow number in the state, or its sentinel; in place over the per-batch numbers.
__global__ __launch_bounds__(kFkThreads) void bt_flowtrack_ids(FlowtrackArgs a) {
    const uint32_t have = a.ftres->n_flows, nb = have < a.n ? have : a.n;
    const uint64_t i = (uint64_t)blockIdx.x * kFkThreads + threadIdx.x;
    if (i >= a.n) return;
    if (!a.ctl->ok) {   // status = 1: no per-batch number may pass for a number in the state
        a.flow_id[i] = BT_FLOW_ID_UNSELECTED;
        return;
    }
    const uint32_t v = a.flow_id[i];   // bt_flowtab_emit's
    if (v < kFtPending) a.flow_id[i] = v < nb ? a.map[v] : BT_FLOW_ID_OVERFLOW;
}

// X1: which flows are idle, as counts.
__global__ __launch_bounds__(kFkThreads) void bt_flowexpire_mark(FlowexpArgs a) {
    __shared__ uint32_t wn[kFkWaves];
    if (!hdr_ok(a, a.slots)) return;
    const uint32_t nf = a.hdr->n_flows, f0 = blockIdx.x * kFkThreads;
    if (f0 >= nf) return;
    const uint32_t tid = threadIdx.x, lane = tid & 63u, wid = tid >> 6, f = f0 + tid;
    const bool is_idle = f < nf && fk_is_idle(a.recs[f].last_ts, a.now, a.idle);
    const uint32_t cnt = (uint32_t)__popcll(__ballot(is_idle));
    if (lane == 0) wn[wid] = cnt;
    __syncthreads();
    if (tid == 0) {
        FxPart p{};
#pragma unroll
        for (uint32_t v = 0; v < kFkWaves; ++v) { p.widle[v] = wn[v]; p.nidle += wn[v]; }
        a.parts[blockIdx.x] = p;
    }
}

// X2: where every block's idle flows start, how many leave, the header's n_flows and *result.
__global__ __launch_bounds__(kFkJoinThreads) void bt_flowexpire_scan(FlowexpArgs a) {
    __shared__ uint32_t sh[kJoinWaves];
    const uint32_t tid = threadIdx.x;
    if (!hdr_ok(a, a.slots)) {
        if (tid == 0) {
            *a.ctl = FxCtl{0u, 0u, 0u, 0u};
            bt_flow_track_expire_result r{};
            r.status = 1u;
            *a.result = r;
        }
        return;
    }
    const uint32_t nf = a.hdr->n_flows;
    const uint32_t nparts = (nf + kFkThreads - 1u) / kFkThreads, per = (nparts + kFkJoinThreads - 1u) / kFkJoinThreads;
    const uint32_t lo = tid * per < nparts ? tid * per : nparts, hi = lo + per < nparts ? lo + per : nparts;
    uint32_t sum = 0;
    for (uint32_t p = lo; p < hi; ++p) sum += a.parts[p].nidle;
    uint32_t total = 0;
    uint32_t run = block_excl<kFkJoinThreads>(sum, sh, &total);
    for (uint32_t p = lo; p < hi; ++p) {
        a.parts[p].rel = run;
        run += a.parts[p].nidle;
    }
    if (tid == 0) {
        const uint32_t limit = a.all || total < a.expired_cap ? total : a.expired_cap;
        *a.ctl = FxCtl{1u, nf, nf - limit, limit};
        a.hdr->n_flows = nf - limit;
        bt_flow_track_expire_result r{};
        r.n_flows_before = nf; r.n_flows = nf - limit; r.n_idle = total; r.n_expired = limit;
        *a.result = r;
    }
}

// X3: the first `limit` idle flows to expired[], the others to their new number in the scratch; remap[].
__global__ __launch_bounds__(kFkThreads) void bt_flowexpire_move(FlowexpArgs a) {
    const FxCtl ctl = *a.ctl;
    if (!ctl.ok) return;
    const uint32_t nf = ctl.n_before, f0 = blockIdx.x * kFkThreads;
    if (f0 >= nf) return;
    const uint32_t tid = threadIdx.x, lane = tid & 63u, wid = tid >> 6, f = f0 + tid;
    const bool is_idle = f < nf && fk_is_idle(a.recs[f].last_ts, a.now, a.idle);   // as bt_flowexpire_mark saw it
    const uint64_t word = __ballot(is_idle);
    if (f >= nf) return;
    const FxPart& part = a.parts[blockIdx.x];
    uint32_t before = part.rel + (uint32_t)__popcll(word & ((1ull << lane) - 1ull));   // idle flows below f
    for (uint32_t v = 0; v < wid; ++v) before += part.widle[v];
    if (is_idle && before < ctl.limit) {
        if (a.expired) rec_copy(a.expired + before, a.recs + f);   // before < limit <= expired_cap
        if (a.remap) a.remap[f] = BT_FLOW_ID_EXPIRED;
        return;
    }
    const uint32_t to = f - (before < ctl.limit ? before : ctl.limit);
    if (ctl.limit) rec_copy(a.tmp + to, a.recs + f);   // to <= f < flow_cap
    if (a.remap) a.remap[f] = to;
}

// X4: the live records back, zeros behind them, every slot empty.
__global__ __launch_bounds__(kFkThreads) void bt_flowexpire_back(FlowexpArgs a) {
    const FxCtl ctl = *a.ctl;
    if (!ctl.ok || !ctl.limit) return;
    const uint64_t t = (uint64_t)blockIdx.x * kFkThreads + threadIdx.x, step = (uint64_t)gridDim.x * kFkThreads;
    slots_fill<kFkThreads>(a.slot, a.slots, kFkEmpty);
    for (uint64_t f = t; f < ctl.n_before; f += step) {   // n_before <= flow_cap
        if (f < ctl.n_live) {
            rec_copy(a.recs + f, a.tmp + f);
        } else {
            uint64_t* const o = reinterpret_cast<uint64_t*>(a.recs + f);
#pragma unroll
            for (int j = 0; j < 13; ++j) o[j] = 0ull;
        }
    }
}

// X5: the live records claim their slots.
__global__ __launch_bounds__(kFkThreads) void bt_flowexpire_claim(FlowexpArgs a) {
    const FxCtl ctl = *a.ctl;
    if (!ctl.ok || !ctl.limit) return;
    const uint32_t f0 = blockIdx.x * kFkThreads;
    if (f0 >= ctl.n_live) return;
    const uint32_t f = f0 + threadIdx.x;
    if (f >= ctl.n_live) return;
    uint32_t w[10];
    head_load(a.recs + f, w);
    claim(a.slot, a.slots, fk_hash(w), f);
}

// The TCP-aware expire (bt_flow_track_expire_tcp_device): siblings of _mark, _move and _back that
// also let closed and reset connections leave and move the side table with the records; _scan and
// _claim run as they are.
namespace {

__device__ __forceinline__ bool tcp_leaves(const FlowexpTcpArgs& a, uint32_t f) {   // f < n_flows <= flow_cap
    return fk_tcp_leaves(a.recs[f].last_ts, a.tcp[f], a.flags, a.now, a.idle, a.closed_idle);
}

}  // namespace

// X1t: which flows leave, as counts.
__global__ __launch_bounds__(kFkThreads) void bt_flowexpire_tcp_mark(FlowexpTcpArgs a) {
    __shared__ uint32_t wn[kFkWaves];
    if (!hdr_ok(a, a.slots)) return;
    const uint32_t nf = a.hdr->n_flows, f0 = blockIdx.x * kFkThreads;
    if (f0 >= nf) return;
    const uint32_t tid = threadIdx.x, lane = tid & 63u, wid = tid >> 6, f = f0 + tid;
    const bool leaves = f < nf && tcp_leaves(a, f);
    const uint32_t cnt = (uint32_t)__popcll(__ballot(leaves));
    if (lane == 0) wn[wid] = cnt;
    __syncthreads();
    if (tid == 0) {
        FxPart p{};
#pragma unroll
        for (uint32_t v = 0; v < kFkWaves; ++v) { p.widle[v] = wn[v]; p.nidle += wn[v]; }
        a.parts[blockIdx.x] = p;
    }
}

// X3t: the first `limit` leaving flows to expired[] / expired_tcp[], the others to their new number in the scratch; remap[].
__global__ __launch_bounds__(kFkThreads) void bt_flowexpire_tcp_move(FlowexpTcpArgs a) {
    const FxCtl ctl = *a.ctl;
    if (!ctl.ok) return;
    const uint32_t nf = ctl.n_before, f0 = blockIdx.x * kFkThreads;
    if (f0 >= nf) return;
    const uint32_t tid = threadIdx.x, lane = tid & 63u, wid = tid >> 6, f = f0 + tid;
    const bool leaves = f < nf && tcp_leaves(a, f);   // as bt_flowexpire_tcp_mark saw it
    const uint64_t word = __ballot(leaves);
    if (f >= nf) return;
    const FxPart& part = a.parts[blockIdx.x];
    uint32_t before = part.rel + (uint32_t)__popcll(word & ((1ull << lane) - 1ull));   // leaving flows below f
    for (uint32_t v = 0; v < wid; ++v) before += part.widle[v];
    if (leaves && before < ctl.limit) {
        if (a.expired) rec_copy(a.expired + before, a.recs + f);   // before < limit <= expired_cap
        if (a.expired_tcp) tcp_copy(a.expired_tcp + before, a.tcp + f);
        if (a.remap) a.remap[f] = BT_FLOW_ID_EXPIRED;
        return;
    }
    const uint32_t to = f - (before < ctl.limit ? before : ctl.limit);
    if (ctl.limit) {   // to <= f < flow_cap
        rec_copy(a.tmp + to, a.recs + f);
        tcp_copy(a.tmp_tcp + to, a.tcp + f);
    }
    if (a.remap) a.remap[f] = to;
}

// X4t: the live records and their side records back, zeros behind them, every slot empty.
__global__ __launch_bounds__(kFkThreads) void bt_flowexpire_tcp_back(FlowexpTcpArgs a) {
    const FxCtl ctl = *a.ctl;
    if (!ctl.ok || !ctl.limit) return;
    const uint64_t t = (uint64_t)blockIdx.x * kFkThreads + threadIdx.x, step = (uint64_t)gridDim.x * kFkThreads;
    slots_fill<kFkThreads>(a.slot, a.slots, kFkEmpty);
    for (uint64_t f = t; f < ctl.n_before; f += step) {   // n_before <= flow_cap
        uint32_t* const s = reinterpret_cast<uint32_t*>(a.tcp + f);
        if (f < ctl.n_live) {
            rec_copy(a.recs + f, a.tmp + f);
            tcp_copy(a.tcp + f, a.tmp_tcp + f);
        } else {
            uint64_t* const o = reinterpret_cast<uint64_t*>(a.recs + f);
#pragma unroll
            for (int j = 0; j < 13; ++j) o[j] = 0ull;
#pragma unroll
            for (int j = 0; j < 4; ++j) s[j] = 0u;
        }
    }
}

namespace {

uint32_t blocks_for(uint64_t items, uint32_t most) {
    const uint64_t b = (items + kFkThreads - 1u) / kFkThreads;
    return (uint32_t)(b > most ? most : b ? b : 1u);
}

}  // namespace

int launch_flowtrack_init(const FlowexpArgs& a, void* stream) {
    hipStream_t st = reinterpret_cast<hipStream_t>(stream);
    const uint64_t words = (uint64_t)a.flow_cap * (sizeof(bt_flow_track_rec) / 8u), quads = a.slots / 4u;
    launch(bt_flowtrack_init, dim3(blocks_for(words > quads ? words : quads, 4096u)), dim3(kFkThreads), 0, st, nullptr, nullptr, a);
    return hipGetLastError() == hipSuccess ? BT_OK : BT_E_INTERNAL;
}

int launch_flowtrack(const FlowtrackArgs& a, void* stream, void* timing_stop) {
    hipStream_t st = reinterpret_cast<hipStream_t>(stream);
    hipEvent_t e1 = reinterpret_cast<hipEvent_t>(timing_stop);
    if (a.empty) {   // the sequence number and *result, in stream order
        launch(bt_flowtrack_join, dim3(1), dim3(kFkJoinThreads), 0, st, nullptr, e1, a);
        return hipGetLastError() == hipSuccess ? BT_OK : BT_E_INTERNAL;
    }
    const uint32_t grid = (uint32_t)(((uint64_t)a.n + kFkThreads - 1u) / kFkThreads);   // n <= 2^30
    launch(bt_flowtrack_find, dim3(grid), dim3(kFkThreads), 0, st, nullptr, nullptr, a);
    launch(bt_flowtrack_join, dim3(1), dim3(kFkJoinThreads), 0, st, nullptr, nullptr, a);
    launch(bt_flowtrack_apply, dim3(grid), dim3(kFkThreads), 0, st, nullptr, a.flow_id ? nullptr : e1, a);
    if (a.flow_id) launch(bt_flowtrack_ids, dim3(grid), dim3(kFkThreads), 0, st, nullptr, e1, a);
    return hipGetLastError() == hipSuccess ? BT_OK : BT_E_INTERNAL;
}

int launch_flowexpire(const FlowexpArgs& a, void* stream) {
    hipStream_t st = reinterpret_cast<hipStream_t>(stream);
    const uint32_t grid = (uint32_t)(((uint64_t)a.flow_cap + kFkThreads - 1u) / kFkThreads);   // flow_cap < 2^32
    const uint64_t quads = a.slots / 4u;
    launch(bt_flowexpire_mark, dim3(grid), dim3(kFkThreads), 0, st, nullptr, nullptr, a);
    launch(bt_flowexpire_scan, dim3(1), dim3(kFkJoinThreads), 0, st, nullptr, nullptr, a);
    launch(bt_flowexpire_move, dim3(grid), dim3(kFkThreads), 0, st, nullptr, nullptr, a);
    launch(bt_flowexpire_back, dim3(blocks_for(quads > a.flow_cap ? quads : a.flow_cap, 4096u)), dim3(kFkThreads), 0, st, nullptr,
           nullptr, a);
    launch(bt_flowexpire_claim, dim3(grid), dim3(kFkThreads), 0, st, nullptr, nullptr, a);
    return hipGetLastError() == hipSuccess ? BT_OK : BT_E_INTERNAL;
}

int launch_flowexpire_tcp(const FlowexpTcpArgs& a, void* stream) {
    hipStream_t st = reinterpret_cast<hipStream_t>(stream);
    const uint32_t grid = (uint32_t)(((uint64_t)a.flow_cap + kFkThreads - 1u) / kFkThreads);   // flow_cap < 2^32
    const uint64_t quads = a.slots / 4u;
    const FlowexpArgs& plain = a;   // _scan and _claim are the plain expire's
    launch(bt_flowexpire_tcp_mark, dim3(grid), dim3(kFkThreads), 0, st, nullptr, nullptr, a);
    launch(bt_flowexpire_scan, dim3(1), dim3(kFkJoinThreads), 0, st, nullptr, nullptr, plain);
    launch(bt_flowexpire_tcp_move, dim3(grid), dim3(kFkThreads), 0, st, nullptr, nullptr, a);
    launch(bt_flowexpire_tcp_back, dim3(blocks_for(quads > a.flow_cap ? quads : a.flow_cap, 4096u)), dim3(kFkThreads), 0, st, nullptr,
           nullptr, a);
    launch(bt_flowexpire_claim, dim3(grid), dim3(kFkThreads), 0, st, nullptr, nullptr, plain);
    return hipGetLastError() == hipSuccess ? BT_OK : BT_E_INTERNAL;
}

}  // namespace bt
