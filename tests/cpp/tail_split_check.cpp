// tail_split_check.cpp — bt_tail_split.h on the host, for the sanitizers (tests/test_tail_split.py
// builds it with -fsanitize=address,undefined and runs it): for each shape, the waves' static
// shares and the tail's tickets cover [0, ntiles) exactly once, the static part is a whole number
// of rounds, every ticket's tiles lie inside the tail, and a ticket past a head's units is a miss.
//
//   tail_split_check                      the built-in shapes
//   tail_split_check NTILES WAVES [ROUNDS CLAIM]   one shape
#include <cstdio>
#include <cstdlib>
#include <vector>

#include "bt_tail_split.h"

using namespace bt;

static int check(uint32_t ntiles, uint32_t waves, uint32_t rounds, uint32_t claim) {
    const TailSplit s = tail_split(ntiles, waves, rounds, claim);
    const TailShape sh = tail_shape(ntiles, s);
    auto fail = [&](const char* what, uint64_t v) {
        fprintf(stderr, "tail_split_check: ntiles %u waves %u rounds %u claim %u: %s (%llu)\n", ntiles, waves, rounds,
                claim, what, (unsigned long long)v);
        return 1;
    };
    if (s.n_static > ntiles) return fail("n_static above ntiles", s.n_static);
    if (s.n_static % waves) return fail("n_static is no whole number of rounds", s.n_static);
    if (s.claim < 1) return fail("claim below 1", s.claim);
    if (sh.tail != ntiles - s.n_static) return fail("tail size", sh.tail);
    // the tail is the last `rounds` rounds plus the remainder, or everything
    if (s.n_static && (sh.tail < (uint64_t)rounds * waves || sh.tail >= (uint64_t)(rounds + 1) * waves))
        return fail("tail is not rounds..rounds+1 rounds", sh.tail);
    std::vector<uint8_t> seen(ntiles, 0);
    for (uint32_t w = 0; w < waves; ++w)   // tile_range: w, w + waves, ... below n_static
        for (uint64_t t = w; t < s.n_static; t += waves) ++seen[t];
    uint64_t units = 0;
    for (uint32_t h = 0; h < kTailHeads; ++h) {
        const uint32_t cnt = head_units(sh, h);
        if (cnt > sh.per_head) return fail("head owns more than per_head", cnt);
        for (uint32_t k = 0; k < cnt; ++k) {
            const uint32_t u = ticket_unit(sh, h, k);
            if (u == kNoTile || u >= sh.units) return fail("ticket maps outside the units", u);
            ++units;
            const uint32_t lim = unit_limit(ntiles, s, sh, u);
            if (lim > ntiles) return fail("unit limit above ntiles", lim);
            uint32_t got = 0;
            for (uint64_t t = unit_first(s, u); t < lim; t += sh.units) {
                if (t < s.n_static || t >= ntiles) return fail("ticket tile outside the tail", t);
                ++seen[t];
                ++got;
            }
            if (got < 1 || got > s.claim) return fail("tiles of one ticket", got);
        }
        // every wave's one missed claim per head, and far past it
        for (uint64_t k = cnt; k <= (uint64_t)cnt + waves; k += (waves > 64 ? waves / 64 : 1))
            if (ticket_unit(sh, h, (uint32_t)k) != kNoTile) return fail("ticket past the head's units is no miss", k);
        if (ticket_unit(sh, h, 0xFFFFFFFFu) != kNoTile) return fail("ticket 2^32-1 is no miss", h);
    }
    if (units != sh.units) return fail("units over the heads", units);
    for (uint32_t t = 0; t < ntiles; ++t)
        if (seen[t] != 1) return fail(seen[t] ? "tile dealt twice" : "tile never dealt", t);
    return 0;
}

int main(int argc, char** argv) {
    if (argc >= 3) {
        const uint32_t r = argc > 3 ? (uint32_t)strtoul(argv[3], nullptr, 0) : kTailRounds;
        const uint32_t c = argc > 4 ? (uint32_t)strtoul(argv[4], nullptr, 0) : kTailClaim;
        if (check((uint32_t)strtoul(argv[1], nullptr, 0), (uint32_t)strtoul(argv[2], nullptr, 0), r, c)) return 1;
        printf("tail_split_check: ok\n");
        return 0;
    }
    int n = 0;
    const uint32_t waves[] = {8, 2048, 4, 1, 1024};
    const uint32_t rounds[] = {kTailRounds, 1, 2, 4, 8, 16};
    const uint32_t claims[] = {kTailClaim, 1, 2, 4, 3};
    for (uint32_t w : waves)
        for (uint32_t r : rounds)
            for (uint32_t c : claims) {
                // 0, 1, fewer tiles than waves, at most the tail, one past it, no multiple of the
                // claim, an exact multiple, the bench's batch, the test's batches
                const uint32_t shapes[] = {0, 1, w - 1, w, w + 1, r * w, r * w + 1, (r + 1) * w - 1, (r + 1) * w,
                                           (r + 1) * w + 1, (r + 3) * w + c + 1, 7, 25, 100, 101, 262144, 262145};
                for (uint32_t nt : shapes) {
                    if (check(nt, w, r, c)) return 1;
                    ++n;
                }
            }
    // the largest batch the ABI can name (n = 2^32 - 1 packets), and a claim so large that
    // first + claim * units passes 2^32
    if (check(67108864u, 2048, kTailRounds, kTailClaim) || check(67108864u, 8, 16, 4) ||
        check(1u << 20, 2048, 4, 0x80000000u))
        return 1;
    n += 3;
    printf("tail_split_check: %d shapes ok\n", n);
    return 0;
}
