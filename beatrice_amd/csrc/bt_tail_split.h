// bt_tail_split.h — how the fixed-stride late-issue main kernel deals its tiles (bt_kernels.hip,
// DESIGN.md §4.1 "The tile deal"): the first n_static tiles cyclically, as before (wave w takes
// w, w + W, ...: a whole number of rounds, the same for every wave), the rest — the tail — by
// tickets a wave takes at run time once its static share is done. Plain functions of
// (ntiles, total_waves), shared by the launch code, the kernel and tests/cpp/tail_split_check.cpp
// (host sanitizers).
//
// The tail's T tiles are U = ceil(T / claim) units; unit u is the tiles n_static + u + j * U,
// j < claim, below ntiles: the units taken at one moment by different waves are neighbouring
// tiles, like the cyclic deal's. The units are split over kTailHeads head words (head h owns the
// units [h * per_head, h * per_head + head_units(h))); ticket k of head h (the value a returning
// atomic add of 1 hands out, from 0 in every launch) is unit h * per_head + k while
// k < head_units(h), and a miss after that. A wave whose claim misses moves to the next head.
#pragma once

#include <stdint.h>

#ifdef __HIPCC__
#define BT_TAIL_HD __host__ __device__
#else
#define BT_TAIL_HD
#endif

namespace bt {

constexpr uint32_t kTailHeads = 8;       // one per XCD label (blockIdx.x & 7)
// A stream's counters: two sets of heads, each head alone in its kTailStride words (heads in one
// line share one memory channel's atomic unit: ~100 claims/us for all of them together). A
// launch claims from one set and zeroes the other, which the stream's previous launch used and
// its next one will: no wave is counted out and no memset is queued.
constexpr uint32_t kTailStride = 1024;
constexpr uint32_t kTailWords = 2 * kTailHeads * kTailStride;
constexpr uint32_t kNoTile = 0xFFFFFFFFu;

// The adopted deal (profiles/r07/tail/sweep.txt): the last kTailRounds rounds of the cyclic deal
// (plus the remainder of ntiles / total_waves) are the tail, kTailClaim tiles per ticket.
#ifndef BT_TAIL_ROUNDS
#define BT_TAIL_ROUNDS 8
#endif
#ifndef BT_TAIL_CLAIM
#define BT_TAIL_CLAIM 2
#endif
constexpr uint32_t kTailRounds = BT_TAIL_ROUNDS;
constexpr uint32_t kTailClaim = BT_TAIL_CLAIM;
// Heads a wave tries, from its own on, before it leaves (a grid with a block of every label; a
// smaller one tries all). Every miss is one more atomic on a head others still claim from: trying
// all eight cost more than the static deal's tail (sweep.txt).
constexpr uint32_t kTailVisits = 2;

struct TailSplit {
    uint32_t n_static;   // tiles dealt cyclically: a multiple of total_waves
    uint32_t claim;      // tiles per ticket (>= 1)
};

// `rounds` tail rounds, `claim` tiles per ticket (the sweep's knobs; the default is the adopted pair).
BT_TAIL_HD inline TailSplit tail_split(uint32_t ntiles, uint32_t total_waves, uint32_t rounds = kTailRounds,
                                       uint32_t claim = kTailClaim) {
    const uint32_t w = total_waves ? total_waves : 1u;
    const uint32_t full = ntiles / w;
    return {full > rounds ? (full - rounds) * w : 0u, claim ? claim : 1u};
}

struct TailShape {
    uint32_t tail;       // T = ntiles - n_static
    uint32_t units;      // U
    uint32_t per_head;   // units a head owns at most
};
BT_TAIL_HD inline TailShape tail_shape(uint32_t ntiles, TailSplit s) {
    const uint32_t tail = ntiles - s.n_static;
    const uint32_t units = (tail + s.claim - 1u) / s.claim;
    return {tail, units, (units + kTailHeads - 1u) / kTailHeads};
}
BT_TAIL_HD inline uint32_t head_units(TailShape sh, uint32_t head) {
    const uint32_t first = head * sh.per_head;
    return first >= sh.units ? 0u : (sh.units - first < sh.per_head ? sh.units - first : sh.per_head);
}
// Ticket k of `head`: its unit, or kNoTile when the head is exhausted.
BT_TAIL_HD inline uint32_t ticket_unit(TailShape sh, uint32_t head, uint32_t k) {
    return k < head_units(sh, head) ? head * sh.per_head + k : kNoTile;
}
// A unit's tiles are first, first + units, ... below the returned limit.
BT_TAIL_HD inline uint32_t unit_first(TailSplit s, uint32_t unit) { return s.n_static + unit; }
BT_TAIL_HD inline uint32_t unit_limit(uint32_t ntiles, TailSplit s, TailShape sh, uint32_t unit) {
    // first + claim * units, capped at ntiles; 64-bit, since the sum may pass 2^32 for a huge claim
    const uint64_t lim = (uint64_t)s.n_static + unit + (uint64_t)s.claim * sh.units;
    return lim < ntiles ? (uint32_t)lim : ntiles;
}

}  // namespace bt
