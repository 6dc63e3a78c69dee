// bt_flowreasm.hip — a payload pattern matched per flow and direction over the TCP segments in
// sequence order: reordered inside the call, overlaps trimmed, cut at holes (bt_flow_reasm_device,
// include/beatrice_gpu.h).
//
// The definition is a loop per (flow, direction) over its segments in (rel, index) order against a
// running end hi = the maximum of rel + len so far. That maximum is a segmented prefix maximum, and
// the packet that delivered the byte before a segment is the one that first reached it: the scan's
// operator is the leftmost maximum, (m1, i1) o (m2, i2) = m2 > m1 ? (m2, i2) : (m1, i1), which is
// associative, so any bracketing gives the loop's numbers exactly. The matcher is bt_flowstream's:
// the pattern has bounded memory, so every piece is matched on its own behind its T preceding
// delivered bytes, found by following pred links. No lane, wave or block waits for another: no
// spin, no flag, no look-back; every loop has its bound in its head; every output is an integer
// sum, an OR or a value with one writer, the same from run to run.
//   bt_flowreasm_class    block = chunk of 256 tiles, lane = packet. A wave loads the select words
//                         of its 32 tiles at once, one per lane (so rest and hit may be select),
//                         walks the layers of every selected packet with a flow number and an
//                         offset, reads have and next of its record (no kernel has changed it
//                         yet), places the segment (flowreasm_place), keeps the trimmed payload
//                         offset, length and direction and rel in the scratch, the tile's word of
//                         the packets that stay, and writes the rest word. Late packets and a
//                         trim add to the record's counters (words no kernel reads), the late
//                         packets of one direction in a tile together.
//   (bt_flowseq_join)     one block: exclusive scan of the chunks' counts; the total m.
//   bt_flowreasm_compact  the (rel, index) pairs of the packets that stay, in packet order.
//   (bt_flowseq's sort)   4 passes: by rel, then index.
//   bt_flowreasm_rekey    every pair's key becomes flow << 1 | dir.
//   (bt_flowseq's sort)   by key: a stream's packets become neighbours, in (rel, index) order.
//   bt_flowreasm_scan<M>  wave = unit of 32 tiles of the sorted list, no block-wide step.
//                           Carry:  gathers rel and len into list order, leaves the unit's
//                                   leftmost maximum since its last head;
//                           Emit:   hole, whole duplicate or delivery against the maximum before
//                                   the pair; the final meta (len 0 for a duplicate), pred[index]
//                                   (the argmax before it, none at a head, cut behind a hole), the
//                                   sums to *result once per wave and to the record once per run
//                                   of a key inside a tile;
//                           Commit: packets and hits per run; the last pair of a key is the only
//                                   lane that writes next, have and d, from dfin of the inclusive
//                                   argmax's packet.
//   bt_flowreasm_sjoin    one block: the segmented exclusive scan over the units' carries.
//   bt_flowreasm_match    bt_flowstream_match's scheme over the trimmed meta; the chain of tails
//                         stops at cut with state 0 and at none with the record's state.
#include "bt_flow_walk.h"
#include "bt_hip_launch.h"
#include "bt_wave.h"
#include "bt_flowreasm.h"

namespace bt {

namespace {

constexpr uint32_t kFrThreads = kFtWaves * 64u;
constexpr uint32_t kFrRow = 64;   // a lane's tail row in LDS, bytes
constexpr uint32_t kFrLateRounds = 4;   // directions whose late packets a tile adds together
static_assert(kFsUnitTiles <= 64u, "one select word per lane");
static_assert(kFstTailMax < kFrRow && kFstPiece > kFstTailMax, "a piece behind the first has its tail in its own packet");

enum FrMode { kFrCarryMode = 0, kFrEmit = 1, kFrCommit = 2 };

__device__ __forceinline__ uint64_t fr_word_of(uint64_t v, uint32_t src) {   // the word of lane `src` (wave-uniform) to every lane
    const uint32_t lo = (uint32_t)__builtin_amdgcn_readlane((int)(uint32_t)v, (int)src);
    const uint32_t hi = (uint32_t)__builtin_amdgcn_readlane((int)(uint32_t)(v >> 32), (int)src);
    return ((uint64_t)hi << 32) | lo;
}

__device__ __forceinline__ uint64_t fr_valid(uint32_t t, uint32_t n) {   // the bits of tile t below n; t < ntiles
    const uint32_t left = n - t * 64u;
    return left >= 64u ? ~0ull : (1ull << left) - 1ull;
}

__device__ __forceinline__ uint64_t fr_shfl64(uint64_t v, uint32_t src) {
    return ((uint64_t)__shfl((uint32_t)(v >> 32), (int)src) << 32) | __shfl((uint32_t)v, (int)src);
}

__device__ __forceinline__ void fr_add64(uint64_t* p, uint64_t v) { atomicAdd(reinterpret_cast<unsigned long long*>(p), (unsigned long long)v); }

__device__ __forceinline__ uint32_t fr_byte(const FlowreasmArgs& a, uint64_t x) { return x < a.bytes ? a.base[x] : 0u; }

__device__ __forceinline__ uint64_t fr_step(const FstPattern& p, uint64_t D, uint64_t b) {
    uint64_t n = ((D << 1) | p.Iall) & b;
    for (uint32_t k = 0; k < p.R; ++k) n |= (n << 1) & p.A;
    return n;
}

// x then y under the segmented operator: y's own pair if y holds a head, else the leftmost maximum.
__device__ __forceinline__ FrCarry fr_join(const FrCarry x, const FrCarry y) {
    const bool own = y.any && (!x.any || y.head);           // y alone
    const bool right = own || (y.any && y.m > x.m);         // the maximum is y's
    return FrCarry{right ? y.m : x.m, right ? y.idx : x.idx, own ? y.head : x.head, x.any | y.any};
}

__device__ __forceinline__ FrCarry fr_shfl_up(const FrCarry& x, int o) {
    FrCarry r;
    r.m = __shfl_up(x.m, o);
    r.idx = __shfl_up(x.idx, o);
    r.head = __shfl_up(x.head, o);
    r.any = __shfl_up(x.any, o);
    return r;
}

__device__ __forceinline__ FrCarry fr_lane(const FrCarry& x, uint32_t src) {   // lane `src` (wave-uniform) to every lane
    FrCarry r;
    r.m = (uint32_t)__builtin_amdgcn_readlane((int)x.m, (int)src);
    r.idx = (uint32_t)__builtin_amdgcn_readlane((int)x.idx, (int)src);
    r.head = (uint32_t)__builtin_amdgcn_readlane((int)x.head, (int)src);
    r.any = (uint32_t)__builtin_amdgcn_readlane((int)x.any, (int)src);
    return r;
}

// The inclusive prefix sums of v over the lanes.
__device__ __forceinline__ uint32_t fr_incl32(uint32_t v, uint32_t lane) {
    for (int o = 1; o < 64; o <<= 1) {
        const uint32_t y = __shfl_up(v, o);
        if (lane >= (uint32_t)o) v += y;
    }
    return v;
}

}  // namespace

__global__ __launch_bounds__(kFrThreads) void bt_flowreasm_class(FlowreasmArgs a) {
    __shared__ uint32_t red[kFtWaves][6];
    const uint32_t c = blockIdx.x, tid = threadIdx.x, lane = tid & 63u, wid = tid >> 6;
    uint32_t nsel = 0, ncon = 0, nunk = 0, nbad = 0, nlate = 0, nfar = 0;   // wave-uniform
    const uint32_t t0 = c * kFtChunkTiles + wid * kFsUnitTiles;
    // the wave's select words, lane k its tile k's, before any rest word is written; zero past the batch
    uint64_t words = 0;
    if (lane < kFsUnitTiles && t0 + lane < a.ntiles) words = (a.select ? a.select[t0 + lane] : ~0ull) & fr_valid(t0 + lane, a.n);
    for (uint32_t k = 0; k < kFsUnitTiles && t0 + k < a.ntiles; ++k) {
        const uint32_t t = t0 + k;
        const uint64_t sw = fr_word_of(words, k);
        const uint32_t i = t * 64u + lane;
        const bool sel = (sw >> lane) & 1ull;   // false at or past n
        const uint32_t id = sel ? a.flow_id[i] : BT_FLOW_ID_UNSELECTED;
        const int64_t po = sel ? a.off[i] : BT_TCPSEQ_OFF_NONE;
        const bool sentinel = sel && flowtcp_is_sentinel(id);
        const bool keyed = sel && id < a.flow_cap;
        const bool mine = keyed && po != BT_TCPSEQ_OFF_NONE;
        nsel += (uint32_t)__popcll(sw);
        nunk += (uint32_t)__popcll(__ballot(sentinel));
        nbad += (uint32_t)__popcll(__ballot(sel && !keyed && !sentinel));
        const uint64_t rw = __ballot(sel && po == BT_TCPSEQ_OFF_NONE);
        uint64_t cw = 0;
        if (__ballot(mine)) {   // wave-uniform
            uint64_t off = 0;
            uint32_t len = 0;
            if (mine) frame_at(a, i, off, len);
            FlowLayers L;
            flow_layers(a, off, len, mine, L);
            const bool tcp = mine && (L.v4 || L.v6) && L.l4 && L.proto == 6u;
            uint32_t H[1], T[1];
            fw_load_at<1>(a, off + L.o3, tcp, H);            // L3 bytes 0 .. 3: version / IHL, TOS, total length
            fw_load_at<1>(a, off + L.o4 + 12u, tcp, T);      // TCP bytes 12 .. 15: data offset, flags, window
            uint32_t dir = 0;
            if (a.bidir) {   // wave-uniform
                uint32_t w[9], nw;
                const uint32_t klass = flow_key_words(a, off, L, L.l4 && !a.l3_only, w, nw);
                dir = tcp ? flow_direction(klass, w) : 0u;
            }
            const uint32_t hdr = 4u * (byte_of(T, 0) >> 4);
            const uint32_t syn = (byte_of(T, 1) & BT_TCPF_SYN) ? 1u : 0u;
            const uint32_t end3 = L.o3 + (L.v4 ? be16_of(H, 2) : 40u + be16_of(L.B, 0));
            const uint32_t end = len < end3 ? len : end3;
            const uint32_t start = L.o4 + hdr;
            const uint32_t plen = tcp && end > start ? end - start : 0u;   // below 2^17
            bool stay = false, late = false, far = false;
            bt_flow_reasm_dir* rec = nullptr;
            if (plen) {
                rec = &a.table[id].d[dir];   // id < flow_cap
                const FrPlace at = flowreasm_place(po, syn, plen, rec->have, rec->next);
                late = at.what == kFrLate;
                far = at.what == kFrFar;
                stay = at.what == kFrTake;
                if (stay) {
                    if (at.trim) fr_add64(&rec->dup_bytes, at.trim);
                    a.meta[i] = FstMeta{start + at.trim, (plen - at.trim) | dir << 31};
                    a.rel[i] = at.rel;
                }
            }
            cw = __ballot(stay);
            ncon += (uint32_t)__popcll(cw);
            // the late packets' counters: the tile's late lanes of one direction add together, for the first
            // kFrLateRounds directions met; what is left adds alone. A replayed stream costs its record one
            // add per tile and counter, not one per packet.
            const uint64_t latew = __ballot(late);
            uint64_t left = latew;
            const uint32_t lkey = id << 1 | dir;
            for (uint32_t r = 0; r < kFrLateRounds && left; ++r) {   // wave-uniform
                const uint32_t src = (uint32_t)__ffsll((unsigned long long)left) - 1u;
                const uint32_t k = (uint32_t)__builtin_amdgcn_readlane((int)lkey, (int)src);
                const bool same = ((left >> lane) & 1ull) && lkey == k;
                const uint64_t samew = __ballot(same);
                const uint32_t by = wave_sum(same ? plen : 0u);   // below 2^23
                if (lane == src) {
                    atomicAdd(&rec->late_packets, (uint32_t)__popcll(samew));
                    fr_add64(&rec->late_bytes, by);
                }
                left &= ~samew;
            }
            if ((left >> lane) & 1ull) {
                atomicAdd(&rec->late_packets, 1u);
                fr_add64(&rec->late_bytes, plen);
            }
            nlate += (uint32_t)__popcll(latew);
            nfar += (uint32_t)__popcll(__ballot(far));
        }
        if (lane == 0) {
            a.numw[t] = cw;
            if (a.rest) a.rest[t] = rw;
        }
    }
    if (lane == 0) {
        red[wid][0] = nsel; red[wid][1] = ncon; red[wid][2] = nunk; red[wid][3] = nbad; red[wid][4] = nlate; red[wid][5] = nfar;
        a.parts[c].wcount[wid] = ncon;
    }
    __syncthreads();
    if (tid < 6u) {
        uint32_t sum = 0;
#pragma unroll
        for (uint32_t v = 0; v < kFtWaves; ++v) sum += red[v][tid];
        bt_flow_reasm_result* const res = a.result;
        uint32_t* const to = tid == 0 ? &res->selected : tid == 2 ? &res->unkeyed : tid == 3 ? &res->bad_ids
                           : tid == 4 ? &res->late_packets : &res->far_packets;
        if (tid == 1u) a.parts[c].count = sum;
        else if (sum) atomicAdd(to, sum);
    }
    if (c == 0 && tid == 6u) atomicAdd(&a.result->n, a.n);
}

__global__ __launch_bounds__(kFrThreads) void bt_flowreasm_compact(FlowreasmArgs a) {
    const uint32_t c = blockIdx.x, tid = threadIdx.x, lane = tid & 63u, wid = tid >> 6;
    uint32_t at = a.parts[c].rel;   // wave-uniform: where the wave's next packet goes; below m
    for (uint32_t v = 0; v < wid; ++v) at += a.parts[c].wcount[v];
    const uint64_t below = (1ull << lane) - 1ull;
    const uint32_t t0 = c * kFtChunkTiles + wid * kFsUnitTiles;
    for (uint32_t k = 0; k < kFsUnitTiles && t0 + k < a.ntiles; ++k) {
        const uint32_t t = t0 + k;
        const uint64_t cw = a.numw[t];   // bits below n only
        if ((cw >> lane) & 1ull) {
            const uint32_t i = t * 64u + lane;
            a.a[at + (uint32_t)__popcll(cw & below)] = FsPair{a.rel[i], i};
        }
        at += (uint32_t)__popcll(cw);
    }
}

__global__ __launch_bounds__(kFrThreads) void bt_flowreasm_rekey(FlowreasmArgs a, FsPair* s) {
    const uint32_t c = blockIdx.x, tid = threadIdx.x;
    const uint32_t m = a.head->m;
    const uint64_t p0 = (uint64_t)c * kFsChunk;
    for (uint32_t k = 0; k < kFsChunk / kFrThreads && p0 + k * kFrThreads < m; ++k) {
        const uint64_t p = p0 + k * kFrThreads + tid;
        if (p >= m) continue;
        const uint32_t i = s[p].idx;   // idx < n
        s[p].key = a.flow_id[i] << 1 | a.meta[i].len_dir >> 31;   // flow < 2^31
    }
}

template <int Mode>
__global__ __launch_bounds__(kFrThreads) void bt_flowreasm_scan(FlowreasmArgs a, const FsPair* s) {
    const uint32_t tid = threadIdx.x, lane = tid & 63u, wid = tid >> 6;
    const uint32_t u = blockIdx.x * kFtWaves + wid;
    const uint32_t m = a.head->m;
    const uint64_t p0 = (uint64_t)u * kFsUnit;
    if (p0 >= m) return;   // the whole wave; no block-wide step below
    // wave-uniform: the leftmost maximum since the last head met, what precedes the unit included
    FrCarry run{0u, 0u, 0u, 0u};
    if (Mode != kFrCarryMode) run = a.carry[u];
    uint32_t prev_key = 0;   // the key of the pair before the tile's first
    if (p0) prev_key = s[p0 - 1u].key;
    uint32_t nholes = 0, ndup = 0, npk = 0;   // wave-uniform tallies
    uint64_t nbytes = 0;
    for (uint32_t k = 0; k < kFsUnitTiles && p0 + k * 64u < m; ++k) {
        const uint64_t p = p0 + k * 64u + lane;
        const bool in = p < m;
        FsPair pr{0u, 0u};
        if (in) pr = s[p];
        uint32_t before = __shfl_up(pr.key, 1);
        if (lane == 0) before = prev_key;
        const bool head = in && (p == 0u || pr.key != before);
        bt_flow_reasm_dir* const rec = &a.table[pr.key >> 1].d[pr.key & 1u];   // key >> 1 < flow_cap; pr = {0, 0} off the list
        FrSeg sg{0u, 0u};
        if (Mode == kFrCarryMode) {
            if (in) {
                sg = FrSeg{a.rel[pr.idx], a.meta[pr.idx].len_dir & 0x7FFFFFFFu};   // idx < n
                a.seg[p] = sg;
            }
        } else if (in) {
            sg = a.seg[p];
        }
        const uint32_t end = sg.rel + sg.len;   // below 2^31
        // the inclusive scan of the tile's pairs; a lane off the list is the identity
        FrCarry incl{end, pr.idx, head ? 1u : 0u, in ? 1u : 0u};
        for (int o = 1; o < 64; o <<= 1) {
            const FrCarry y = fr_shfl_up(incl, o);
            if (lane >= (uint32_t)o) incl = fr_join(y, incl);
        }
        const uint64_t inw = __ballot(in);
        const uint64_t rw = __ballot(in && (lane == 0u || pr.key != before));   // the runs of one key inside the tile
        const uint64_t above = lane == 63u ? 0ull : rw & (~0ull << (lane + 1u));
        const uint32_t stop = above ? (uint32_t)__ffsll((unsigned long long)above) - 1u : 64u;   // the next run's head
        const uint64_t mask = (stop == 64u ? ~0ull : (1ull << stop) - 1ull) & (~0ull << lane) & inw;   // a run head's run
        const bool rhead = (rw >> lane) & 1ull;
        if (Mode == kFrEmit) {
            FrCarry ex = fr_shfl_up(incl, 1);
            if (lane == 0) ex = FrCarry{0u, 0u, 0u, 0u};
            ex = fr_join(run, ex);   // everything of this lane's stream before it, where the lane is no head
            bool hole = false, dup = false;
            uint32_t holeb = 0, dupb = 0, deliv = 0;
            if (in) {
                const bool have = rec->have != 0u;   // Commit writes it, a launch later
                const uint32_t hi = head ? (have ? 0u : sg.rel) : ex.m;
                hole = sg.rel > hi;
                dup = end <= hi;
                if (hole) holeb = sg.rel - hi;
                uint32_t pred = head ? kFstNone : ex.idx;
                if (hole) pred = kFrCut;
                a.pred[pr.idx] = pred;
                if (dup) {
                    dupb = sg.len;
                    a.meta[pr.idx].len_dir &= 0x80000000u;   // no pieces
                } else {
                    const uint32_t cut = hole ? 0u : hi - sg.rel;   // below len
                    dupb = cut;
                    deliv = sg.len - cut;
                    if (cut) {
                        const FstMeta mt = a.meta[pr.idx];
                        a.meta[pr.idx] = FstMeta{mt.start + cut, (mt.len_dir & 0x80000000u) | deliv};
                    }
                }
            }
            const uint64_t holew = __ballot(hole), dupw = __ballot(dup), cutw = __ballot(dupb != 0u);
            nholes += (uint32_t)__popcll(holew);
            ndup += (uint32_t)__popcll(dupw);
            npk += (uint32_t)__popcll(__ballot(deliv != 0u));
            nbytes += wave_sum(deliv);   // a tile's sum is below 2^23
            if (holew | cutw) {   // wave-uniform: the record's sums, one add per run of a key inside the tile
                const uint32_t ih = fr_incl32(holeb, lane), id = fr_incl32(dupb, lane);   // a tile's sums are below 2^31 * 64: mod 2^32 differences
                const uint32_t xh = ih - holeb, xd = id - dupb;
                const uint32_t th = (uint32_t)__builtin_amdgcn_readlane((int)ih, 63), td = (uint32_t)__builtin_amdgcn_readlane((int)id, 63);
                const uint32_t eh = __shfl(xh, (int)(stop & 63u)), ed = __shfl(xd, (int)(stop & 63u));
                if (rhead) {
                    const uint32_t rh = (stop == 64u ? th : eh) - xh, rd = (stop == 64u ? td : ed) - xd;
                    const uint32_t nh = (uint32_t)__popcll(mask & holew), nd = (uint32_t)__popcll(mask & dupw);
                    if (nh) atomicAdd(&rec->holes, nh);
                    if (nd) atomicAdd(&rec->dup_packets, nd);
                    if (rh) fr_add64(&rec->hole_bytes, rh);
                    if (rd) fr_add64(&rec->dup_bytes, rd);
                }
            }
        }
        if (Mode == kFrCommit) {
            bool dl = false, hit = false;
            if (in) {
                dl = (a.meta[pr.idx].len_dir & 0x7FFFFFFFu) != 0u;
                hit = (a.hitw[pr.idx >> 6] >> (pr.idx & 63u)) & 1ull;
            }
            const uint64_t dlw = __ballot(dl), hitw = __ballot(hit);
            if (rhead) {
                const uint32_t np = (uint32_t)__popcll(mask & dlw), nh = (uint32_t)__popcll(mask & hitw);
                if (np) atomicAdd(&rec->stream_packets, np);
                if (nh) atomicAdd(&rec->hit_packets, nh);
            }
            uint32_t after = __shfl_down(pr.key, 1);
            if (lane == 63u && p + 1u < m) after = s[p + 1u].key;
            const bool last = in && (p + 1u == m || pr.key != after);
            if (last) {   // the direction's state after the call; no other lane of the launch touches these words
                const FrCarry all = fr_join(run, incl);
                const bool have = rec->have != 0u;
                const int64_t base = have ? rec->next : kFrNewBase;
                rec->next = (int64_t)((uint64_t)base + all.m);
                rec->have = 1u;
                rec->d = a.dfin[all.idx];   // the packet that first reached the maximum delivered the stream's last byte
            }
        }
        run = fr_join(run, fr_lane(incl, 63u));
        prev_key = (uint32_t)__builtin_amdgcn_readlane((int)pr.key, 63);   // a tile that is not full is the last
    }
    if (Mode == kFrCarryMode && lane == 0) a.carry[u] = run;
    if (Mode == kFrEmit && lane == 0) {
        bt_flow_reasm_result* const res = a.result;
        if (nholes) atomicAdd(&res->holes, nholes);
        if (ndup) atomicAdd(&res->dup_packets, ndup);
        if (npk) atomicAdd(&res->stream_packets, npk);
        if (nbytes) fr_add64(&res->stream_bytes, nbytes);
    }
}

// The units' carries become what precedes each unit: the leftmost maximum since the last head before it.
__global__ __launch_bounds__(kFsJoinThreads) void bt_flowreasm_sjoin(FlowreasmArgs a) {
    constexpr uint32_t kWaves = kFsJoinThreads / 64u;
    __shared__ FrCarry wtot[kWaves];
    const uint32_t tid = threadIdx.x, lane = tid & 63u, wid = tid >> 6;
    const uint32_t m = a.head->m;
    const uint32_t live = (uint32_t)(((uint64_t)m + kFsUnit - 1u) / kFsUnit);   // <= nchunks * kFtWaves
    FrCarry running{0u, 0u, 0u, 0u};   // block-uniform
    for (uint32_t u0 = 0; u0 < live; u0 += kFsJoinThreads) {
        const uint32_t u = u0 + tid;
        FrCarry own{0u, 0u, 0u, 0u};
        if (u < live) own = a.carry[u];
        FrCarry incl = own;
        for (int o = 1; o < 64; o <<= 1) {
            const FrCarry y = fr_shfl_up(incl, o);
            if (lane >= (uint32_t)o) incl = fr_join(y, incl);
        }
        if (lane == 63u) wtot[wid] = incl;
        FrCarry ex = fr_shfl_up(incl, 1);
        if (lane == 0) ex = FrCarry{0u, 0u, 0u, 0u};
        __syncthreads();
        FrCarry pre = running, all = running;
#pragma unroll
        for (uint32_t w = 0; w < kWaves; ++w) {
            const FrCarry x = wtot[w];
            if (w < wid) pre = fr_join(pre, x);
            all = fr_join(all, x);
        }
        __syncthreads();
        if (u < live) a.carry[u] = fr_join(pre, ex);
        running = all;
    }
}

__global__ __launch_bounds__(kFrThreads) void bt_flowreasm_match(FlowreasmArgs a) {
    __shared__ uint64_t B[256];
    __shared__ uint8_t tails[kFrThreads][kFrRow];
    __shared__ uint64_t hacc[kFtWaves];
    const uint32_t c = blockIdx.x, tid = threadIdx.x, lane = tid & 63u, wid = tid >> 6;
    const FstPattern pat = a.pat;
    {   // the table, widened to 64-bit entries
        const uint32_t eb = pat.W / 8u;
        for (uint32_t e = tid; e < 256u; e += kFrThreads) {
            uint64_t v = 0;
            for (uint32_t j = 0; j < eb; ++j) v |= (uint64_t)a.blob[kFstBlobHeader + e * eb + j] << (8u * j);
            B[e] = v;
        }
    }
    __syncthreads();
    const uint32_t T = pat.T;
    uint32_t nhit = 0, nnew = 0;   // wave-uniform
    const uint32_t t0 = c * kFtChunkTiles + wid * kFsUnitTiles;
    for (uint32_t kt = 0; kt < kFsUnitTiles && t0 + kt < a.ntiles; ++kt) {
        const uint32_t t = t0 + kt;
        const uint64_t cw = a.numw[t];   // bits below n only
        if (cw == 0ull) {                // wave-uniform
            if (lane == 0) {
                a.hitw[t] = 0ull;
                if (a.hit) a.hit[t] = 0ull;
            }
            continue;
        }
        const uint32_t i = t * 64u + lane;
        bool con = (cw >> lane) & 1ull;
        uint64_t pbase = 0;      // the first delivered byte, from base
        uint32_t plen = 0, dir = 0, id = 0;
        if (con) {
            uint64_t off;
            uint32_t len;
            frame_at(a, i, off, len);
            const FstMeta mt = a.meta[i];   // as Emit left it
            pbase = off + mt.start;
            plen = mt.len_dir & 0x7FFFFFFFu;
            dir = mt.len_dir >> 31;
            id = a.flow_id[i];   // below flow_cap
            con = plen != 0u;    // a whole duplicate has no pieces
        }
        const uint32_t pc = (plen + kFstPiece - 1u) / kFstPiece;
        const uint32_t incl = fr_incl32(pc, lane);
        const uint32_t total = (uint32_t)__builtin_amdgcn_readlane((int)incl, 63), excl = incl - pc;
        // the packet's tail: the T delivered bytes before its own, as far as the call holds them
        uint32_t need = con ? T : 0u;
        uint64_t D0 = 0;
        {
            uint32_t cur = con ? a.pred[i] : kFstNone;
            for (uint32_t hop = 0; hop < kFstTailMax && __ballot(need && cur < kFrCut); ++hop) {
                if (need && cur < kFrCut) {
                    uint64_t off;
                    uint32_t len;
                    frame_at(a, cur, off, len);   // cur < n: a packet that delivered a byte
                    const FstMeta mt = a.meta[cur];
                    const uint32_t ln = mt.len_dir & 0x7FFFFFFFu;   // > 0
                    const uint32_t take = need < ln ? need : ln;
                    const uint64_t from = off + mt.start + (ln - take);
                    for (uint32_t b = 0; b < take; ++b) tails[tid][need - take + b] = (uint8_t)fr_byte(a, from + b);   // need <= T < kFrRow
                    need -= take;
                    if (need) cur = a.pred[cur];
                }
            }
            // the stream's head came first: its state before the call, where the record has one
            if (con && need && cur == kFstNone) {
                const bt_flow_reasm_dir* const rec = &a.table[id].d[dir];   // id < flow_cap; Commit writes it, a launch later
                if (rec->have) D0 = rec->d;
            }
        }
        if (lane == 0) hacc[wid] = 0ull;
        wave_lds_sync();
        for (uint32_t q0 = 0; q0 < total; q0 += 64u) {   // total <= 64 * 2^10
            const uint32_t q = q0 + lane;
            const bool on = q < total;
            uint32_t j = 0;   // the largest lane whose pieces start at or below q: it has pieces
#pragma unroll
            for (uint32_t stp = 32u; stp; stp >>= 1) {
                const uint32_t v = __shfl(excl, (int)(j + stp));
                if (v <= q) j += stp;
            }
            const uint32_t k = q - __shfl(excl, (int)j);
            const uint64_t jbase = fr_shfl64(pbase, j);
            const uint32_t jlen = __shfl(plen, (int)j), jneed = __shfl(need, (int)j), jpc = __shfl(pc, (int)j);
            uint64_t D = fr_shfl64(D0, j);
            if (k) D = 0;
            uint64_t H = 0;
            // the tail of a packet's first piece, from its row
            const uint32_t tl = on && k == 0u ? T - jneed : 0u;
            for (uint32_t b = 0; b < kFstTailMax && __ballot(b < tl); ++b)
                if (b < tl) D = fr_step(pat, D, B[tails[wid * 64u + j][jneed + b]]);
            // the tail of a later piece and the own bytes, from the frame
            const uint32_t own = k * kFstPiece;
            const uint32_t x0 = k ? own - T : 0u;
            const uint32_t x1 = on ? (own + kFstPiece < jlen ? own + kFstPiece : jlen) : 0u;
            for (uint32_t g = 0; g < (kFstPiece + kFstTailMax + 15u) / 16u; ++g) {
                const uint32_t x = x0 + g * 16u;
                if (__ballot(x < x1) == 0ull) break;
                uint32_t v[4];
                fw_load_at<4>(a, jbase + x, x < x1, v);
#pragma unroll
                for (uint32_t bb = 0; bb < 16u; ++bb) {
                    const uint32_t pos = x + bb;
                    if (pos < x1) {
                        D = fr_step(pat, D, B[byte_of(v, (int)bb)]);
                        if (pos >= own) H |= D & pat.F;
                    }
                }
            }
            if (on && H) atomicOr(reinterpret_cast<unsigned long long*>(&hacc[wid]), 1ull << j);
            if (on && k + 1u == jpc) a.dfin[t * 64u + j] = D;   // the packet's last piece: one writer
        }
        wave_lds_sync();
        const uint64_t hw = hacc[wid];
        wave_lds_sync();
        if (lane == 0) {
            a.hitw[t] = hw;
            if (a.hit) a.hit[t] = hw;
        }
        nhit += (uint32_t)__popcll(hw);
        bool fresh = false;
        if ((hw >> lane) & 1ull) {   // a delivering lane: id < flow_cap
            const uint64_t bit = 1ull << (id & 63u);
            const uint64_t old = atomicOr(reinterpret_cast<unsigned long long*>(&a.bits[id >> 6]), bit);
            if (!(old & bit)) {   // the one lane of the call that asks for this flow; no kernel has changed these words yet
                const bt_flow_reasm_rec* rec = a.table + id;
                fresh = rec->d[0].hit_packets == 0u && rec->d[1].hit_packets == 0u;
            }
        }
        nnew += (uint32_t)__popcll(__ballot(fresh));
    }
    if (lane == 0) {
        if (nhit) atomicAdd(&a.result->hit_packets, nhit);
        if (nnew) atomicAdd(&a.result->new_hit_flows, nnew);
    }
}

int launch_flowreasm_front(const FlowreasmArgs& a, void* stream, void* const* ev, const FsPair** out_sorted) {
    hipStream_t st = reinterpret_cast<hipStream_t>(stream);
    const auto e = [&](int k) { return ev ? reinterpret_cast<hipEvent_t>(ev[k]) : nullptr; };
    const dim3 grid(a.nchunks), block(kFrThreads), one(1), join(kFsJoinThreads);
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
    launch(bt_flowreasm_class, grid, block, 0, st, e(0), nullptr, a);
    launch_flowseq_join(q, stream);
    launch(bt_flowreasm_compact, grid, block, 0, st, nullptr, e(1), a);   // its end: the first sort's start
    const FsPair* sorted = a.a;
    launch_flowseq_sort(q, 32u / kFsDigitBits, stream, nullptr, &sorted);   // by rel: all 32 bits
    FsPair* const mid = const_cast<FsPair*>(sorted);
    launch(bt_flowreasm_rekey, grid, block, 0, st, e(2), nullptr, a, mid);
    q.a = mid;
    q.b = mid == a.a ? a.b : a.a;
    launch_flowseq_sort(q, a.passes, stream, nullptr, &sorted);
    launch(bt_flowreasm_scan<kFrCarryMode>, grid, block, 0, st, e(3), nullptr, a, sorted);
    launch(bt_flowreasm_sjoin, one, join, 0, st, nullptr, nullptr, a);
    launch(bt_flowreasm_scan<kFrEmit>, grid, block, 0, st, nullptr, nullptr, a, sorted);
    *out_sorted = sorted;
    return hipGetLastError() == hipSuccess ? BT_OK : BT_E_INTERNAL;
}

int launch_flowreasm_match(const FlowreasmArgs& a, void* stream, void* e4) {
    launch(bt_flowreasm_match, dim3(a.nchunks), dim3(kFrThreads), 0, reinterpret_cast<hipStream_t>(stream),
           reinterpret_cast<hipEvent_t>(e4), nullptr, a);
    return hipGetLastError() == hipSuccess ? BT_OK : BT_E_INTERNAL;
}

int launch_flowreasm_commit(const FlowreasmArgs& a, const FsPair* sorted, void* stream, void* e5, void* e6) {
    launch(bt_flowreasm_scan<kFrCommit>, dim3(a.nchunks), dim3(kFrThreads), 0, reinterpret_cast<hipStream_t>(stream),
           reinterpret_cast<hipEvent_t>(e5), reinterpret_cast<hipEvent_t>(e6), a, sorted);
    return hipGetLastError() == hipSuccess ? BT_OK : BT_E_INTERNAL;
}

int launch_flowreasm(const FlowreasmArgs& a, void* stream, void* const* ev) {
    if (a.n == 0 || a.nchunks == 0) return BT_OK;
    const FsPair* sorted = nullptr;
    if (const int rc = launch_flowreasm_front(a, stream, ev, &sorted)) return rc;
    if (const int rc = launch_flowreasm_match(a, stream, ev ? ev[4] : nullptr)) return rc;
    return launch_flowreasm_commit(a, sorted, stream, ev ? ev[5] : nullptr, ev ? ev[6] : nullptr);
}

}  // namespace bt
