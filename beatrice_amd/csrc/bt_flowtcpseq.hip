// bt_flowtcpseq.hip — TCP segments classified per flow and direction against the sequence space:
// first, in order, gap, old, overlap (bt_flow_tcpseq_device, include/beatrice_gpu.h; DESIGN.md
// §4.2n).
//
// The definition is a loop per (flow, direction): u = pos + (int32)(s - last_seq), the class from u
// and u + L against hi, hi = max(hi, u + L). It is a scan: give every participating packet, in its
// direction's order, the pair (S, M) = (delta, delta + L), delta the int32 step of s from the
// packet before it, and combine pairs by (S1, M1) o (S2, M2) = (S1 + S2, max(M1, S1 + M2)). The
// operator is associative, so any bracketing gives the loop's numbers exactly: a packet's u is
// the S of everything up to it, the hi it meets the M of everything before it. The first packet of
// a direction in the call takes its delta from the record (0 for a new direction), so pos and hi
// of the record are the only offsets added afterwards.
// The participating packets are compacted, sorted by flow << 1 | dir with bt_flowseq's stable
// radix sort, and scanned segment by segment in the chunked family's shape. No lane, wave or block
// waits for another: no spin, no flag, no look-back; every loop has its bound in its head; every
// output is an integer sum, an AND or a value with one writer, the same from run to run.
//   bt_flowtcpseq_class    block = chunk of 256 tiles, lane = packet. A wave loads the select
//                          words of its 32 tiles at once, one per lane (so out_select may be
//                          select), walks the layers of every selected packet with a flow number
//                          (bt_flow_walk.h), keeps s, L and the direction in the scratch and the
//                          tile's word of participating packets, writes NONE into cls / off of
//                          every other packet and starts the tile's out_select word: the select
//                          bits below n. Counts per wave and chunk, tallies to *result.
//   (bt_flowseq_join)      one block: exclusive scan of the chunks' counts; the total m.
//   bt_flowtcpseq_compact  the (flow << 1 | dir, index) pairs of the participating packets, in
//                          packet order.
//   (bt_flowseq's sort)    stable, by key: a direction's packets become neighbours, in packet order.
//   bt_flowtcpseq_scan<M>  wave = unit of 32 tiles of the sorted list, no block-wide step. Heads
//                          are where the key changes. Per tile a segmented inclusive scan of the
//                          pairs over the lanes; what no head of the unit precedes joins the
//                          unit's carry.
//                            Carry:  gathers s and L, forms delta (a head's against its record),
//                                    keeps both in list order, leaves the unit's pairs since its
//                                    last head combined;
//                            Emit:   classifies, writes cls and off at the packet's index, clears
//                                    the OLD packets' bits in out_select (atomicAnd into words
//                                    that bt_flowtcpseq_class initialised: an AND, so
//                                    deterministic), and adds the record's counters: a run of one
//                                    key is summed over its lanes and carried from tile to tile,
//                                    so a key costs one atomicAdd per counter and unit;
//                            Commit: the last lane of each segment is the only lane that writes
//                                    pos, hi, last_seq and have of its record in this launch: no
//                                    atomic, and no race with Emit's reads, a launch earlier.
//   bt_flowtcpseq_sjoin    one block: the segmented exclusive scan over the units' carries.
// Blocks and waves whose part of the list lies at or past m end at once.
#include "bt_flow_walk.h"
#include "bt_hip_launch.h"
#include "bt_wave.h"
#include "bt_flowtcpseq.h"

namespace bt {

namespace {

constexpr uint32_t kFtsThreads = kFtWaves * 64u;
static_assert(kFsUnitTiles <= 64u, "one select word per lane");

enum FtsMode { kFtsCarry = 0, kFtsEmit = 1, kFtsCommit = 2 };

__device__ __forceinline__ uint64_t fts_word_of(uint64_t v, uint32_t src) {   // the word of lane `src` (wave-uniform) to every lane
    const uint32_t lo = (uint32_t)__builtin_amdgcn_readlane((int)(uint32_t)v, (int)src);
    const uint32_t hi = (uint32_t)__builtin_amdgcn_readlane((int)(uint32_t)(v >> 32), (int)src);
    return ((uint64_t)hi << 32) | lo;
}

__device__ __forceinline__ uint64_t fts_valid(uint32_t t, uint32_t n) {   // the bits of tile t below n; t < ntiles
    const uint32_t left = n - t * 64u;
    return left >= 64u ? ~0ull : (1ull << left) - 1ull;
}

__device__ __forceinline__ uint64_t fts_up64(uint64_t v, int o) {
    return ((uint64_t)__shfl_up((uint32_t)(v >> 32), o) << 32) | __shfl_up((uint32_t)v, o);
}

__device__ __forceinline__ uint64_t fts_at64(uint64_t v, uint32_t src) {
    return ((uint64_t)__shfl((uint32_t)(v >> 32), (int)src) << 32) | __shfl((uint32_t)v, (int)src);
}

__device__ __forceinline__ void fts_add64(uint64_t* p, uint64_t v) { atomicAdd(reinterpret_cast<unsigned long long*>(p), (unsigned long long)v); }

__device__ __forceinline__ int64_t fts_plus(int64_t x, int64_t y) { return (int64_t)((uint64_t)x + (uint64_t)y); }

// x then y under the segmented operator: y's own pair if y holds a head, else both combined.
__device__ __forceinline__ FtsCarry fts_join(const FtsCarry& x, const FtsCarry& y) {
    if (!y.any) return x;
    if (!x.any || y.head) return y;
    FtsCarry r;
    r.S = fts_plus(x.S, y.S);
    const int64_t m2 = fts_plus(x.S, y.M);
    r.M = x.M > m2 ? x.M : m2;
    r.head = x.head;
    r.any = 1u;
    return r;
}

__device__ __forceinline__ FtsCarry fts_shfl_up(const FtsCarry& x, int o) {
    FtsCarry r;
    r.S = (int64_t)fts_up64((uint64_t)x.S, o);
    r.M = (int64_t)fts_up64((uint64_t)x.M, o);
    r.head = __shfl_up(x.head, o);
    r.any = __shfl_up(x.any, o);
    return r;
}

__device__ __forceinline__ FtsCarry fts_lane(const FtsCarry& x, uint32_t src) {   // lane `src` (wave-uniform) to every lane
    FtsCarry r;
    r.S = (int64_t)fts_word_of((uint64_t)x.S, src);
    r.M = (int64_t)fts_word_of((uint64_t)x.M, src);
    r.head = (uint32_t)__builtin_amdgcn_readlane((int)x.head, (int)src);
    r.any = (uint32_t)__builtin_amdgcn_readlane((int)x.any, (int)src);
    return r;
}

// A run's sums for its record, wave-uniform while they wait for the run's end.
struct FtsPend { uint32_t key, on, seq, old, gap, ovl; uint64_t oldb, gapb; };

__device__ __forceinline__ void fts_flush(bt_flow_tcpseq_rec* table, const FtsPend& q) {   // one lane
    bt_flow_tcpseq_dir* const d = &table[q.key >> 1].d[q.key & 1u];   // key >> 1 < flow_cap
    if (q.seq) atomicAdd(&d->seq_packets, q.seq);
    if (q.old) atomicAdd(&d->old_packets, q.old);
    if (q.gap) atomicAdd(&d->gap_packets, q.gap);
    if (q.ovl) atomicAdd(&d->overlap_packets, q.ovl);
    if (q.oldb) fts_add64(&d->old_bytes, q.oldb);
    if (q.gapb) fts_add64(&d->gap_bytes, q.gapb);
}

}  // namespace

__global__ __launch_bounds__(kFtsThreads) void bt_flowtcpseq_class(FlowtcpseqArgs a) {
    __shared__ uint32_t red[kFtWaves][4];
    __shared__ uint64_t redb[kFtWaves];
    const uint32_t c = blockIdx.x, tid = threadIdx.x, lane = tid & 63u, wid = tid >> 6;
    uint32_t nsel = 0, npar = 0, nunk = 0, nbad = 0;   // wave-uniform
    uint64_t nbytes = 0;
    const uint32_t t0 = c * kFtChunkTiles + wid * kFsUnitTiles;
    // the wave's select words, lane k its tile k's, before any out_select word is written; zero past the batch
    uint64_t words = 0;
    if (lane < kFsUnitTiles && t0 + lane < a.ntiles) words = (a.select ? a.select[t0 + lane] : ~0ull) & fts_valid(t0 + lane, a.n);
    for (uint32_t k = 0; k < kFsUnitTiles && t0 + k < a.ntiles; ++k) {
        const uint32_t t = t0 + k;
        const uint64_t sw = fts_word_of(words, k);
        const uint32_t i = t * 64u + lane;
        const bool in = (fts_valid(t, a.n) >> lane) & 1ull;
        const bool sel = (sw >> lane) & 1ull;   // false at or past n
        const uint32_t id = sel ? a.flow_id[i] : BT_FLOW_ID_UNSELECTED;
        const bool mine = sel && id < a.flow_cap;
        const bool sentinel = sel && flowtcp_is_sentinel(id);
        nsel += (uint32_t)__popcll(sw);
        nunk += (uint32_t)__popcll(__ballot(sentinel));
        nbad += (uint32_t)__popcll(__ballot(sel && !mine && !sentinel));
        uint64_t pw = 0;
        if (__ballot(mine)) {   // wave-uniform
            uint64_t off = 0;
            uint32_t len = 0;
            if (mine) frame_at(a, i, off, len);
            FlowLayers L;
            flow_layers(a, off, len, mine, L);
            const bool tcp = mine && (L.v4 || L.v6) && L.l4 && L.proto == 6u;
            uint32_t H[1], Q[1], T[1];
            fw_load_at<1>(a, off + L.o3, tcp, H);              // L3 bytes 0 .. 3: version / IHL, TOS, total length
            fw_load_at<1>(a, off + L.o4 + 4u, tcp, Q);         // TCP bytes 4 .. 7: the sequence number
            fw_load_at<1>(a, off + L.o4 + 12u, tcp, T);        // TCP bytes 12 .. 15: data offset, flags, window
            uint32_t dir = 0;
            if (a.bidir) {   // wave-uniform
                uint32_t w[9], nw;
                const uint32_t klass = flow_key_words(a, off, L, L.l4 && !a.l3_only, w, nw);
                dir = tcp ? flow_direction(klass, w) : 0u;
            }
            const uint32_t ihl = byte_of(H, 0) & 0xFu, fl = byte_of(T, 1);
            const int32_t ip_payload = L.v4 ? (int32_t)be16_of(H, 2) - (int32_t)(4u * ihl) : (int32_t)be16_of(L.B, 0);
            const int32_t hdr = (int32_t)(4u * (byte_of(T, 0) >> 4));
            const uint32_t plen = ip_payload > hdr ? (uint32_t)(ip_payload - hdr) : 0u;
            const uint32_t sl = tcp ? plen + ((fl & BT_TCPF_SYN) ? 1u : 0u) + ((fl & BT_TCPF_FIN) ? 1u : 0u) : 0u;   // below 2^17
            if (sl) a.meta[i] = FtsMeta{fw_be32(Q[0]), sl | dir << 31};
            pw = __ballot(sl != 0u);
            npar += (uint32_t)__popcll(pw);
            nbytes += wave_sum(sl);
        }
        if (in && !((pw >> lane) & 1ull)) {
            if (a.cls) a.cls[i] = (uint8_t)BT_TCPSEQ_NONE;
            if (a.off) a.off[i] = BT_TCPSEQ_OFF_NONE;
        }
        if (lane == 0) {
            a.numw[t] = pw;
            if (a.out_select) a.out_select[t] = sw;
        }
    }
    if (lane == 0) {
        red[wid][0] = nsel; red[wid][1] = npar; red[wid][2] = nunk; red[wid][3] = nbad;
        redb[wid] = nbytes;
        a.parts[c].wcount[wid] = npar;
    }
    __syncthreads();
    if (tid < 4u) {
        uint32_t sum = 0;
#pragma unroll
        for (uint32_t v = 0; v < kFtWaves; ++v) sum += red[v][tid];
        bt_flow_tcpseq_result* const res = a.result;
        uint32_t* const to = tid == 0 ? &res->selected : tid == 1 ? &res->seq_packets : tid == 2 ? &res->unkeyed : &res->bad_ids;
        if (sum) atomicAdd(to, sum);
        if (tid == 1u) a.parts[c].count = sum;
    }
    if (tid == 4u) {
        uint64_t sum = 0;
#pragma unroll
        for (uint32_t v = 0; v < kFtWaves; ++v) sum += redb[v];
        if (sum) fts_add64(&a.result->seq_bytes, sum);
    }
    if (c == 0 && tid == 5u) atomicAdd(&a.result->n, a.n);
}

__global__ __launch_bounds__(kFtsThreads) void bt_flowtcpseq_compact(FlowtcpseqArgs a) {
    const uint32_t c = blockIdx.x, tid = threadIdx.x, lane = tid & 63u, wid = tid >> 6;
    uint32_t at = a.parts[c].rel;   // wave-uniform: where the wave's next participating packet goes; below m
    for (uint32_t v = 0; v < wid; ++v) at += a.parts[c].wcount[v];
    const uint64_t below = (1ull << lane) - 1ull;
    const uint32_t t0 = c * kFtChunkTiles + wid * kFsUnitTiles;
    for (uint32_t k = 0; k < kFsUnitTiles && t0 + k < a.ntiles; ++k) {
        const uint32_t t = t0 + k;
        const uint64_t pw = a.numw[t];   // bits below n only
        if ((pw >> lane) & 1ull) {
            const uint32_t i = t * 64u + lane;
            a.a[at + (uint32_t)__popcll(pw & below)] = FsPair{a.flow_id[i] << 1 | a.meta[i].len_dir >> 31, i};   // flow < 2^31
        }
        at += (uint32_t)__popcll(pw);
    }
}

template <int Mode>
__global__ __launch_bounds__(kFtsThreads) void bt_flowtcpseq_scan(FlowtcpseqArgs a, const FsPair* s) {
    const uint32_t tid = threadIdx.x, lane = tid & 63u, wid = tid >> 6;
    const uint32_t u = blockIdx.x * kFtWaves + wid;
    const uint32_t m = a.head->m;
    const uint64_t p0 = (uint64_t)u * kFsUnit;
    if (p0 >= m) return;   // the whole wave; no block-wide step below
    // wave-uniform: the pairs since the last head met, what precedes the unit included
    FtsCarry run{0, 0, 0u, 0u};
    if (Mode != kFtsCarry) run = a.carry[u];
    uint32_t prev_key = 0, prev_seq = 0;   // the pair before the tile's first
    if (p0) {
        const FsPair before = s[p0 - 1u];
        prev_key = before.key;
        if (Mode == kFtsCarry) prev_seq = a.meta[before.idx].seq;   // idx < n: a participating packet
    }
    uint32_t nfirst = 0, ninord = 0, ngap = 0, nold = 0, novl = 0;   // wave-uniform tallies
    uint64_t toldb = 0, tgapb = 0;
    // Emit's invariant: behind every tile `pend` holds that tile's last run of one key, not yet added to its
    // record. It goes to the record only when the next tile's lane 0 has another key (or at the unit's end);
    // otherwise it is folded into lane 0's run, which may in turn be the tile's last and wait again.
    FtsPend pend{0u, 0u, 0u, 0u, 0u, 0u, 0ull, 0ull};
    for (uint32_t k = 0; k < kFsUnitTiles && p0 + k * 64u < m; ++k) {
        const uint64_t p = p0 + k * 64u + lane;
        const bool in = p < m;
        FsPair pr{0u, 0u};
        if (in) pr = s[p];
        uint32_t before = __shfl_up(pr.key, 1);
        if (lane == 0) before = prev_key;
        const bool head = in && (p == 0u || pr.key != before);
        bt_flow_tcpseq_dir* const rec = &a.table[pr.key >> 1].d[pr.key & 1u];   // key >> 1 < flow_cap; pr = {0, 0} off the list
        int32_t delta = 0;
        uint32_t len = 0, seq = 0;
        if (Mode == kFtsCarry) {
            if (in) {
                const FtsMeta mt = a.meta[pr.idx];   // idx < n
                seq = mt.seq;
                len = mt.len_dir & 0x7FFFFFFFu;
            }
            uint32_t sb = __shfl_up(seq, 1);
            if (lane == 0) sb = prev_seq;
            if (head) delta = rec->have ? (int32_t)(seq - rec->last_seq) : 0;   // no kernel has changed the record yet
            else delta = (int32_t)(seq - sb);
            if (in) a.dl[p] = FtsDl{delta, len};
            prev_seq = (uint32_t)__builtin_amdgcn_readlane((int)seq, 63);   // a tile that is not full is the last
        } else if (in) {
            const FtsDl d = a.dl[p];
            delta = d.delta;
            len = d.len;
        }
        // the inclusive scan of the tile's pairs; a lane off the list is the identity
        FtsCarry incl{(int64_t)delta, (int64_t)delta + (int64_t)len, head ? 1u : 0u, in ? 1u : 0u};
        for (int o = 1; o < 64; o <<= 1) {
            const FtsCarry y = fts_shfl_up(incl, o);
            if (lane >= (uint32_t)o) incl = fts_join(y, incl);
        }
        if (Mode == kFtsEmit) {
            FtsCarry ex = fts_shfl_up(incl, 1);
            if (lane == 0) ex = FtsCarry{0, 0, 0u, 0u};
            ex = fts_join(run, ex);   // everything of this lane's segment before it; any == 0 for a head
            uint32_t cl = BT_TCPSEQ_NONE;
            uint64_t oldb = 0, gapb = 0;
            if (in) {
                const bool have = rec->have != 0u;
                const int64_t pos0 = have ? rec->pos : 0;
                const int64_t at = fts_plus(pos0, head ? (int64_t)delta : fts_plus(ex.S, delta));
                const int64_t e = fts_plus(at, len);
                int64_t hi = have ? rec->hi : 0;
                if (!head) {
                    const int64_t hb = fts_plus(pos0, ex.M);
                    hi = have && hi > hb ? hi : hb;
                }
                if (head && !have) cl = BT_TCPSEQ_FIRST;
                else if (at == hi) cl = BT_TCPSEQ_IN_ORDER;
                else if (at > hi) { cl = BT_TCPSEQ_GAP; gapb = (uint64_t)at - (uint64_t)hi; }
                else if (e <= hi) { cl = BT_TCPSEQ_OLD; oldb = len; }
                else { cl = BT_TCPSEQ_OVERLAP; oldb = (uint64_t)hi - (uint64_t)at; }
                if (a.cls) a.cls[pr.idx] = (uint8_t)cl;
                if (a.off) a.off[pr.idx] = at;
                if (cl == BT_TCPSEQ_OLD && a.out_select)
                    atomicAnd(reinterpret_cast<unsigned long long*>(&a.out_select[pr.idx >> 6]), ~(1ull << (pr.idx & 63u)));
            }
            const uint64_t inw = __ballot(in), gapw = __ballot(cl == BT_TCPSEQ_GAP), oldw = __ballot(cl == BT_TCPSEQ_OLD),
                           ovlw = __ballot(cl == BT_TCPSEQ_OVERLAP);
            nfirst += (uint32_t)__popcll(__ballot(cl == BT_TCPSEQ_FIRST));
            ninord += (uint32_t)__popcll(__ballot(cl == BT_TCPSEQ_IN_ORDER));
            ngap += (uint32_t)__popcll(gapw);
            nold += (uint32_t)__popcll(oldw);
            novl += (uint32_t)__popcll(ovlw);
            // the record's counters: the runs of one key inside the tile, lane 0 a run's head here
            const uint64_t rw = __ballot(in && (lane == 0u || pr.key != before));
            uint64_t xold = 0, xgap = 0, told = 0, tgap = 0;   // exclusive prefix sums over the lanes, and the tile's sums
            if (oldw | ovlw) {   // wave-uniform
                uint64_t v = oldb;
                for (int o = 1; o < 64; o <<= 1) {
                    const uint64_t y = fts_up64(v, o);
                    if (lane >= (uint32_t)o) v += y;
                }
                xold = v - oldb;
                told = fts_word_of(v, 63u);
            }
            if (gapw) {   // wave-uniform
                uint64_t v = gapb;
                for (int o = 1; o < 64; o <<= 1) {
                    const uint64_t y = fts_up64(v, o);
                    if (lane >= (uint32_t)o) v += y;
                }
                xgap = v - gapb;
                tgap = fts_word_of(v, 63u);
            }
            toldb += told;
            tgapb += tgap;
            const uint64_t above = lane == 63u ? 0ull : rw & (~0ull << (lane + 1u));
            const uint32_t stop = above ? (uint32_t)__ffsll((unsigned long long)above) - 1u : 64u;   // the next run's head
            const uint64_t mask = (stop == 64u ? ~0ull : (1ull << stop) - 1ull) & (~0ull << lane) & inw;
            const uint64_t eold = fts_at64(xold, stop & 63u), egap = fts_at64(xgap, stop & 63u);
            FtsPend mine{pr.key, 1u, (uint32_t)__popcll(mask), (uint32_t)__popcll(mask & oldw), (uint32_t)__popcll(mask & gapw),
                         (uint32_t)__popcll(mask & ovlw), (stop == 64u ? told : eold) - xold, (stop == 64u ? tgap : egap) - xgap};
            // what waits from the tiles before: into lane 0's run if the key goes on, else to its record
            const uint32_t key0 = (uint32_t)__builtin_amdgcn_readlane((int)pr.key, 0);   // lane 0 is on the list: p0 + 64 k < m
            if (pend.on && pend.key != key0) {
                if (lane == 0) fts_flush(a.table, pend);
                pend.on = 0u;
            }
            if (pend.on && lane == 0) {
                mine.seq += pend.seq; mine.old += pend.old; mine.gap += pend.gap; mine.ovl += pend.ovl;
                mine.oldb += pend.oldb; mine.gapb += pend.gapb;
            }
            const uint32_t ls = 63u - (uint32_t)__clzll((long long)rw);   // the tile's last run waits in turn; rw has bit 0
            if (((rw >> lane) & 1ull) && lane != ls) fts_flush(a.table, mine);
            pend.key = (uint32_t)__builtin_amdgcn_readlane((int)mine.key, (int)ls);
            pend.on = 1u;
            pend.seq = (uint32_t)__builtin_amdgcn_readlane((int)mine.seq, (int)ls);
            pend.old = (uint32_t)__builtin_amdgcn_readlane((int)mine.old, (int)ls);
            pend.gap = (uint32_t)__builtin_amdgcn_readlane((int)mine.gap, (int)ls);
            pend.ovl = (uint32_t)__builtin_amdgcn_readlane((int)mine.ovl, (int)ls);
            pend.oldb = fts_word_of(mine.oldb, ls);
            pend.gapb = fts_word_of(mine.gapb, ls);
        }
        if (Mode == kFtsCommit) {
            uint32_t after = __shfl_down(pr.key, 1);
            if (lane == 63u && p + 1u < m) after = s[p + 1u].key;
            const bool last = in && (p + 1u == m || pr.key != after);
            if (last) {   // the direction's state after its last packet; no other lane of the launch touches these words
                const FtsCarry all = fts_join(run, incl);
                const bool have = rec->have != 0u;
                const int64_t pos0 = have ? rec->pos : 0;
                const int64_t hb = fts_plus(pos0, all.M), hi = rec->hi;
                rec->pos = fts_plus(pos0, all.S);
                rec->hi = have && hi > hb ? hi : hb;
                rec->last_seq = a.meta[pr.idx].seq;   // idx < n
                rec->have = 1u;
            }
        }
        run = fts_join(run, fts_lane(incl, 63u));
        prev_key = (uint32_t)__builtin_amdgcn_readlane((int)pr.key, 63);   // a tile that is not full is the last
    }
    if (Mode == kFtsCarry && lane == 0) a.carry[u] = run;
    if (Mode == kFtsEmit && lane == 0) {
        if (pend.on) fts_flush(a.table, pend);
        bt_flow_tcpseq_result* const res = a.result;
        if (nfirst) atomicAdd(&res->first, nfirst);
        if (ninord) atomicAdd(&res->in_order, ninord);
        if (ngap) atomicAdd(&res->gap, ngap);
        if (nold) atomicAdd(&res->old, nold);
        if (novl) atomicAdd(&res->overlap, novl);
        if (toldb) fts_add64(&res->old_bytes, toldb);
        if (tgapb) fts_add64(&res->gap_bytes, tgapb);
    }
}

// The units' carries become what precedes each unit: the pairs since the last head before it.
__global__ __launch_bounds__(kFsJoinThreads) void bt_flowtcpseq_sjoin(FlowtcpseqArgs a) {
    constexpr uint32_t kWaves = kFsJoinThreads / 64u;
    __shared__ FtsCarry wtot[kWaves];
    const uint32_t tid = threadIdx.x, lane = tid & 63u, wid = tid >> 6;
    const uint32_t m = a.head->m;
    const uint32_t live = (uint32_t)(((uint64_t)m + kFsUnit - 1u) / kFsUnit);   // <= nchunks * kFtWaves
    FtsCarry running{0, 0, 0u, 0u};   // block-uniform
    for (uint32_t u0 = 0; u0 < live; u0 += kFsJoinThreads) {
        const uint32_t u = u0 + tid;
        FtsCarry own{0, 0, 0u, 0u};
        if (u < live) own = a.carry[u];
        FtsCarry incl = own;
        for (int o = 1; o < 64; o <<= 1) {
            const FtsCarry y = fts_shfl_up(incl, o);
            if (lane >= (uint32_t)o) incl = fts_join(y, incl);
        }
        if (lane == 63u) wtot[wid] = incl;
        FtsCarry ex = fts_shfl_up(incl, 1);
        if (lane == 0) ex = FtsCarry{0, 0, 0u, 0u};
        __syncthreads();
        FtsCarry pre = running, all = running;
#pragma unroll
        for (uint32_t w = 0; w < kWaves; ++w) {
            const FtsCarry x = wtot[w];
            if (w < wid) pre = fts_join(pre, x);
            all = fts_join(all, x);
        }
        __syncthreads();
        if (u < live) a.carry[u] = fts_join(pre, ex);
        running = all;
    }
}

int launch_flowtcpseq(const FlowtcpseqArgs& a, void* stream, void* const* ev) {
    if (a.n == 0 || a.nchunks == 0) return BT_OK;
    hipStream_t st = reinterpret_cast<hipStream_t>(stream);
    const auto e = [&](int k) { return ev ? reinterpret_cast<hipEvent_t>(ev[k]) : nullptr; };
    const dim3 grid(a.nchunks), block(kFtsThreads), one(1), join(kFsJoinThreads);
    FlowseqArgs q{};   // the sort's view of the scratch
    q.nchunks = a.nchunks;
    q.head = a.head;
    q.parts = a.parts;
    q.a = a.a;
    q.b = a.b;
    q.dcnt = a.dcnt;
    q.drel = a.drel;
    q.dwcnt = a.dwcnt;
    q.dstart = a.dstart;
    launch(bt_flowtcpseq_class, grid, block, 0, st, e(0), nullptr, a);
    launch_flowseq_join(q, stream);
    launch(bt_flowtcpseq_compact, grid, block, 0, st, nullptr, e(1), a);   // its end: the sort's start, with or without a pass
    const FsPair* sorted = a.a;
    launch_flowseq_sort(q, a.passes, stream, nullptr, &sorted);
    launch(bt_flowtcpseq_scan<kFtsCarry>, grid, block, 0, st, e(2), nullptr, a, sorted);
    launch(bt_flowtcpseq_sjoin, one, join, 0, st, nullptr, nullptr, a);
    launch(bt_flowtcpseq_scan<kFtsEmit>, grid, block, 0, st, e(3), nullptr, a, sorted);
    launch(bt_flowtcpseq_scan<kFtsCommit>, grid, block, 0, st, nullptr, e(4), a, sorted);
    return hipGetLastError() == hipSuccess ? BT_OK : BT_E_INTERNAL;
}

}  // namespace bt
