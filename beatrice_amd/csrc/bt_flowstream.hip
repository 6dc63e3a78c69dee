// bt_flowstream.hip — a payload pattern matched per flow and direction, across packet boundaries
// (bt_flow_stream_device, include/beatrice_gpu.h).
//
// The pattern has bounded memory (P positions, no repeatable one, no anchor): the matcher's state
// after a byte is a function of the last P - 1 stream bytes, so a piece of a stream is matched on
// its own once it has its T = P - 1 preceding bytes. No lane walks a flow, no lane consumes more
// than kFstPiece + T bytes. No lane, wave or block waits for another: no spin, no flag, no
// look-back; every loop has its bound in its head; every output is an integer sum, an OR or a value
// with one writer, the same from run to run.
//   bt_flowstream_class    block = chunk of 256 tiles, lane = packet. A wave loads the select words
//                          of its 32 tiles at once, one per lane (so hit may be select), walks the
//                          layers of every selected packet with a flow number (bt_flow_walk.h),
//                          keeps the payload's offset, length and direction in the scratch and
//                          the tile's word of contributing packets. Counts per wave and chunk,
//                          tallies to *result.
//   (bt_flowseq_join)      one block: exclusive scan of the chunks' counts; the total m.
//   bt_flowstream_compact  the (flow << 1 | dir, index) pairs of the contributing packets, in
//                          packet order.
//   (bt_flowseq's sort)    stable, by key: a stream's packets become neighbours, in packet order.
//   bt_flowstream_link     lane = sorted pair: pred[index] = the index before it if the key is the
//                          same, else none.
//   bt_flowstream_match    wave = unit of 32 tiles of packets, no block-wide step but the blob's
//                          load. Per tile the lanes scan their packets' piece counts (ceil(len /
//                          128)); every contributing lane gathers its packet's tail into its LDS
//                          row by following pred back (at most T hops of at least a byte each)
//                          and, where the list's head comes first, starts from table[f].d[dir];
//                          then the tile's pieces go round the wave 64 at a time, a lane finding
//                          its piece's packet by a binary search over the scan. A piece k > 0 has
//                          its tail in its own packet. A lane steps over its tail without counting
//                          hits, then over its own bytes, loaded 16 at a time under the fan-out's
//                          read rule. Hits meet in one LDS word per wave; one lane stores the
//                          tile's word: no global atomic. A packet's last piece leaves its state in
//                          the scratch. A hit packet claims its flow's bit in the scratch bitmap
//                          (atomicOr); the one that finds it clear looks at the record, which no
//                          kernel has changed yet: the flow's first hit or not.
//   bt_flowstream_commit   lane = sorted pair. Runs of one key inside a tile add their packets and
//                          hits with one atomicAdd each; the last pair of a key is the only lane
//                          that writes d[dir], from its packet's last piece.
#include "bt_flow_walk.h"
#include "bt_hip_launch.h"
#include "bt_wave.h"
#include "bt_flowstream.h"

namespace bt {

namespace {

constexpr uint32_t kFstThreads = kFtWaves * 64u;
constexpr uint32_t kFstRow = 64;   // a lane's tail row in LDS, bytes
static_assert(kFsUnitTiles <= 64u, "one select word per lane");
static_assert(kFstTailMax < kFstRow && kFstPiece > kFstTailMax, "a piece behind the first has its tail in its own packet");

__device__ __forceinline__ uint64_t fst_word_of(uint64_t v, uint32_t src) {   // the word of lane `src` (wave-uniform) to every lane
    const uint32_t lo = (uint32_t)__builtin_amdgcn_readlane((int)(uint32_t)v, (int)src);
    const uint32_t hi = (uint32_t)__builtin_amdgcn_readlane((int)(uint32_t)(v >> 32), (int)src);
    return ((uint64_t)hi << 32) | lo;
}

__device__ __forceinline__ uint64_t fst_valid(uint32_t t, uint32_t n) {   // the bits of tile t below n; t < ntiles
    const uint32_t left = n - t * 64u;
    return left >= 64u ? ~0ull : (1ull << left) - 1ull;
}

__device__ __forceinline__ uint64_t fst_shfl64(uint64_t v, uint32_t src) {
    return ((uint64_t)__shfl((uint32_t)(v >> 32), (int)src) << 32) | __shfl((uint32_t)v, (int)src);
}

__device__ __forceinline__ void fst_add64(uint64_t* p, uint64_t v) { atomicAdd(reinterpret_cast<unsigned long long*>(p), (unsigned long long)v); }

__device__ __forceinline__ uint32_t fst_byte(const FlowstreamArgs& a, uint64_t x) { return x < a.bytes ? a.base[x] : 0u; }

__device__ __forceinline__ uint64_t fst_step(const FstPattern& p, uint64_t D, uint64_t b) {
    uint64_t n = ((D << 1) | p.Iall) & b;
    for (uint32_t k = 0; k < p.R; ++k) n |= (n << 1) & p.A;
    return n;
}

}  // namespace

__global__ __launch_bounds__(kFstThreads) void bt_flowstream_class(FlowstreamArgs a) {
    __shared__ uint32_t red[kFtWaves][4];
    __shared__ uint64_t redb[kFtWaves];
    const uint32_t c = blockIdx.x, tid = threadIdx.x, lane = tid & 63u, wid = tid >> 6;
    uint32_t nsel = 0, ncon = 0, nunk = 0, nbad = 0;   // wave-uniform
    uint64_t nbytes = 0;
    const uint32_t t0 = c * kFtChunkTiles + wid * kFsUnitTiles;
    // the wave's select words, lane k its tile k's, before any hit word is written; zero past the batch
    uint64_t words = 0;
    if (lane < kFsUnitTiles && t0 + lane < a.ntiles) words = (a.select ? a.select[t0 + lane] : ~0ull) & fst_valid(t0 + lane, a.n);
    for (uint32_t k = 0; k < kFsUnitTiles && t0 + k < a.ntiles; ++k) {
        const uint32_t t = t0 + k;
        const uint64_t sw = fst_word_of(words, k);
        const uint32_t i = t * 64u + lane;
        const bool sel = (sw >> lane) & 1ull;   // false at or past n
        const uint32_t id = sel ? a.flow_id[i] : BT_FLOW_ID_UNSELECTED;
        const bool mine = sel && id < a.flow_cap;
        const bool sentinel = sel && flowtcp_is_sentinel(id);
        nsel += (uint32_t)__popcll(sw);
        nunk += (uint32_t)__popcll(__ballot(sentinel));
        nbad += (uint32_t)__popcll(__ballot(sel && !mine && !sentinel));
        uint64_t cw = 0;
        if (__ballot(mine)) {   // wave-uniform
            uint64_t off = 0;
            uint32_t len = 0;
            if (mine) frame_at(a, i, off, len);
            FlowLayers L;
            flow_layers(a, off, len, mine, L);
            const bool l4 = mine && (L.v4 || L.v6) && L.l4, tcp = l4 && L.proto == 6u;
            uint32_t H[1], T[1];
            fw_load_at<1>(a, off + L.o3, l4, H);            // L3 bytes 0 .. 3: version / IHL, TOS, total length
            fw_load_at<1>(a, off + L.o4 + 12u, tcp, T);     // TCP bytes 12 .. 15: data offset, flags, window
            uint32_t dir = 0;
            if (a.bidir) {   // wave-uniform
                uint32_t w[9], nw;
                const uint32_t klass = flow_key_words(a, off, L, L.l4 && !a.l3_only, w, nw);
                dir = l4 ? flow_direction(klass, w) : 0u;
            }
            const uint32_t hdr = tcp ? 4u * (byte_of(T, 0) >> 4) : 8u;
            const uint32_t end3 = L.o3 + (L.v4 ? be16_of(H, 2) : 40u + be16_of(L.B, 0));
            const uint32_t end = len < end3 ? len : end3;
            const uint32_t start = L.o4 + hdr;
            const uint32_t plen = l4 && end > start ? end - start : 0u;   // below 2^17
            if (plen) a.meta[i] = FstMeta{start, plen | dir << 31};
            cw = __ballot(plen != 0u);
            ncon += (uint32_t)__popcll(cw);
            nbytes += wave_sum(plen);
        }
        if (lane == 0) a.numw[t] = cw;
    }
    if (lane == 0) {
        red[wid][0] = nsel; red[wid][1] = ncon; red[wid][2] = nunk; red[wid][3] = nbad;
        redb[wid] = nbytes;
        a.parts[c].wcount[wid] = ncon;
    }
    __syncthreads();
    if (tid < 4u) {
        uint32_t sum = 0;
#pragma unroll
        for (uint32_t v = 0; v < kFtWaves; ++v) sum += red[v][tid];
        bt_flow_stream_result* const res = a.result;
        uint32_t* const to = tid == 0 ? &res->selected : tid == 1 ? &res->stream_packets : tid == 2 ? &res->unkeyed : &res->bad_ids;
        if (sum) atomicAdd(to, sum);
        if (tid == 1u) a.parts[c].count = sum;
    }
    if (tid == 4u) {
        uint64_t sum = 0;
#pragma unroll
        for (uint32_t v = 0; v < kFtWaves; ++v) sum += redb[v];
        if (sum) fst_add64(&a.result->stream_bytes, sum);
    }
    if (c == 0 && tid == 5u) atomicAdd(&a.result->n, a.n);
}

__global__ __launch_bounds__(kFstThreads) void bt_flowstream_compact(FlowstreamArgs a) {
    const uint32_t c = blockIdx.x, tid = threadIdx.x, lane = tid & 63u, wid = tid >> 6;
    uint32_t at = a.parts[c].rel;   // wave-uniform: where the wave's next contributing packet goes; below m
    for (uint32_t v = 0; v < wid; ++v) at += a.parts[c].wcount[v];
    const uint64_t below = (1ull << lane) - 1ull;
    const uint32_t t0 = c * kFtChunkTiles + wid * kFsUnitTiles;
    for (uint32_t k = 0; k < kFsUnitTiles && t0 + k < a.ntiles; ++k) {
        const uint32_t t = t0 + k;
        const uint64_t cw = a.numw[t];   // bits below n only
        if ((cw >> lane) & 1ull) {
            const uint32_t i = t * 64u + lane;
            a.a[at + (uint32_t)__popcll(cw & below)] = FsPair{a.flow_id[i] << 1 | a.meta[i].len_dir >> 31, i};   // flow < 2^31
        }
        at += (uint32_t)__popcll(cw);
    }
}

__global__ __launch_bounds__(kFstThreads) void bt_flowstream_link(FlowstreamArgs a, const FsPair* s) {
    const uint32_t c = blockIdx.x, tid = threadIdx.x;
    const uint32_t m = a.head->m;
    const uint64_t p0 = (uint64_t)c * kFsChunk;
    for (uint32_t k = 0; k < kFsChunk / kFstThreads && p0 + k * kFstThreads < m; ++k) {
        const uint64_t p = p0 + k * kFstThreads + tid;
        if (p >= m) continue;
        const FsPair pr = s[p];
        uint32_t pred = kFstNone;
        if (p) {
            const FsPair before = s[p - 1u];
            if (before.key == pr.key) pred = before.idx;
        }
        a.pred[pr.idx] = pred;   // idx < n
    }
}

__global__ __launch_bounds__(kFstThreads) void bt_flowstream_match(FlowstreamArgs a) {
    __shared__ uint64_t B[256];
    __shared__ uint8_t tails[kFstThreads][kFstRow];
    __shared__ uint64_t hacc[kFtWaves];
    const uint32_t c = blockIdx.x, tid = threadIdx.x, lane = tid & 63u, wid = tid >> 6;
    const FstPattern pat = a.pat;
    {   // the table, widened to 64-bit entries
        const uint32_t eb = pat.W / 8u;
        for (uint32_t e = tid; e < 256u; e += kFstThreads) {
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
        const bool con = (cw >> lane) & 1ull;
        uint64_t pbase = 0;      // the payload's first byte, from base
        uint32_t plen = 0, dir = 0, id = 0;
        if (con) {
            uint64_t off;
            uint32_t len;
            frame_at(a, i, off, len);
            const FstMeta mt = a.meta[i];
            pbase = off + mt.start;
            plen = mt.len_dir & 0x7FFFFFFFu;
            dir = mt.len_dir >> 31;
            id = a.flow_id[i];   // below flow_cap
        }
        const uint32_t pc = (plen + kFstPiece - 1u) / kFstPiece;
        uint32_t incl = pc;
        for (int o = 1; o < 64; o <<= 1) {
            const uint32_t y = __shfl_up(incl, o);
            if (lane >= (uint32_t)o) incl += y;
        }
        const uint32_t total = (uint32_t)__builtin_amdgcn_readlane((int)incl, 63), excl = incl - pc;
        // the packet's tail: the T stream bytes before its payload, as far as the batch holds them
        uint32_t need = con ? T : 0u;
        uint64_t D0 = 0;
        {
            uint32_t cur = con ? a.pred[i] : kFstNone;
            for (uint32_t hop = 0; hop < kFstTailMax && __ballot(need && cur != kFstNone); ++hop) {
                if (need && cur != kFstNone) {
                    uint64_t off;
                    uint32_t len;
                    frame_at(a, cur, off, len);   // cur < n: a contributing packet
                    const FstMeta mt = a.meta[cur];
                    const uint32_t ln = mt.len_dir & 0x7FFFFFFFu;   // > 0
                    const uint32_t take = need < ln ? need : ln;
                    const uint64_t from = off + mt.start + (ln - take);
                    for (uint32_t b = 0; b < take; ++b) tails[tid][need - take + b] = (uint8_t)fst_byte(a, from + b);   // need <= T < kFstRow
                    need -= take;
                    if (need) cur = a.pred[cur];
                }
            }
            // the head of the list came first: the stream's state before the batch
            if (con && need) D0 = a.table[id].d[dir];   // id < flow_cap
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
            const uint64_t jbase = fst_shfl64(pbase, j);
            const uint32_t jlen = __shfl(plen, (int)j), jneed = __shfl(need, (int)j), jpc = __shfl(pc, (int)j);
            uint64_t D = fst_shfl64(D0, j);
            if (k) D = 0;
            uint64_t H = 0;
            // the tail of a packet's first piece, from its row
            const uint32_t tl = on && k == 0u ? T - jneed : 0u;
            for (uint32_t b = 0; b < kFstTailMax && __ballot(b < tl); ++b)
                if (b < tl) D = fst_step(pat, D, B[tails[wid * 64u + j][jneed + b]]);
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
                        D = fst_step(pat, D, B[byte_of(v, (int)bb)]);
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
        if ((hw >> lane) & 1ull) {   // a contributing lane: id < flow_cap
            const uint64_t bit = 1ull << (id & 63u);
            const uint64_t old = atomicOr(reinterpret_cast<unsigned long long*>(&a.bits[id >> 6]), bit);
            if (!(old & bit)) {   // the one lane of the call that asks for this flow; no kernel has changed the record yet
                const bt_flow_stream_rec* rec = a.table + id;
                fresh = rec->hit_packets[0] == 0u && rec->hit_packets[1] == 0u;
            }
        }
        nnew += (uint32_t)__popcll(__ballot(fresh));
    }
    if (lane == 0) {
        if (nhit) atomicAdd(&a.result->hit_packets, nhit);
        if (nnew) atomicAdd(&a.result->new_hit_flows, nnew);
    }
}

__global__ __launch_bounds__(kFstThreads) void bt_flowstream_commit(FlowstreamArgs a, const FsPair* s) {
    const uint32_t tid = threadIdx.x, lane = tid & 63u, wid = tid >> 6;
    const uint32_t u = blockIdx.x * kFtWaves + wid;
    const uint32_t m = a.head->m;
    const uint64_t p0 = (uint64_t)u * kFsUnit;
    if (p0 >= m) return;   // the whole wave; no block-wide step below
    for (uint32_t k = 0; k < kFsUnitTiles && p0 + k * 64u < m; ++k) {
        const uint64_t p = p0 + k * 64u + lane;
        const bool in = p < m;
        FsPair pr{0u, 0u};
        if (in) pr = s[p];
        const bool hit = in && ((a.hitw[pr.idx >> 6] >> (pr.idx & 63u)) & 1ull);
        const uint32_t before = __shfl_up(pr.key, 1);
        const bool head = in && (lane == 0u || pr.key != before);   // of a run inside the tile
        uint32_t after = __shfl_down(pr.key, 1);
        if (lane == 63u && p + 1u < m) after = s[p + 1u].key;
        const bool last = in && (p + 1u == m || pr.key != after);   // of the key in the whole list
        const uint64_t inw = __ballot(in), hw = __ballot(head), hitw = __ballot(hit);
        bt_flow_stream_rec* const rec = a.table + (pr.key >> 1);   // key >> 1 < flow_cap
        const uint32_t d = pr.key & 1u;
        if (head) {   // the run [lane, the next head): its packets and hits at once
            const uint64_t above = lane == 63u ? 0ull : hw & (~0ull << (lane + 1u));
            const uint32_t stop = above ? (uint32_t)__ffsll((unsigned long long)above) - 1u : 64u;
            const uint64_t run = (stop == 64u ? ~0ull : (1ull << stop) - 1ull) & (~0ull << lane) & inw;
            atomicAdd(&rec->stream_packets[d], (uint32_t)__popcll(run));
            const uint32_t nh = (uint32_t)__popcll(run & hitw);
            if (nh) atomicAdd(&rec->hit_packets[d], nh);
        }
        if (last) rec->d[d] = a.dfin[pr.idx];   // no other lane of the launch touches this word
    }
}

int launch_flowstream(const FlowstreamArgs& a, void* stream, void* const* ev) {
    if (a.n == 0 || a.nchunks == 0) return BT_OK;
    hipStream_t st = reinterpret_cast<hipStream_t>(stream);
    const auto e = [&](int k) { return ev ? reinterpret_cast<hipEvent_t>(ev[k]) : nullptr; };
    const dim3 grid(a.nchunks), block(kFstThreads);
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
    launch(bt_flowstream_class, grid, block, 0, st, e(0), nullptr, a);
    launch_flowseq_join(q, stream);
    launch(bt_flowstream_compact, grid, block, 0, st, nullptr, e(1), a);   // its end: the sort's start, with or without a pass
    const FsPair* sorted = a.a;
    launch_flowseq_sort(q, a.passes, stream, nullptr, &sorted);
    launch(bt_flowstream_link, grid, block, 0, st, e(2), nullptr, a, sorted);
    launch(bt_flowstream_match, grid, block, 0, st, nullptr, nullptr, a);
    launch(bt_flowstream_commit, grid, block, 0, st, e(3), e(4), a, sorted);
    return hipGetLastError() == hipSuccess ? BT_OK : BT_E_INTERNAL;
}

}  // namespace bt
