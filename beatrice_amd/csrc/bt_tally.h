// bt_tally.h — counts of a batch on the device (bt_tally.hip), shared with the host runtime
// (bt_tally_device in bt_tally_host.cpp).
#pragma once

#include <stdint.h>

#include "beatrice_gpu.h"
#include "bt_frames.h"

namespace bt {

// One chunk of the reduction = kTallyChunkTiles tiles of 64 packets (16,384 packets, as the
// compaction's kChunkTiles and the pack's kPackChunkTiles): a chunk's bins fit 32 bits.
constexpr uint32_t kTallyChunkTiles = 256;
constexpr uint32_t kTallyChunk = kTallyChunkTiles * 64u;
constexpr uint32_t kTallyNone = 0xFFFFFFFFu;   // TallyPartial::first_*: the chunk has none
constexpr uint32_t kTallyJoinThreads = 512;

struct TallyPartial {          // workspace, one per chunk: written by bt_tally_chunks
    uint32_t hist[256];        // the chunk's decision bytes by value ((code << 6) | slot)
    uint64_t bytes[4];         // its frame lengths by code
    uint32_t layer[16];        // its packets with bit k of present (0..7) / of ok (8..15)
    uint32_t first_throw;      // batch index of its first BT_DECIDE_THROW / BT_DECIDE_HOST byte
    uint32_t first_host;
    uint32_t pad[2];           // a multiple of 16 bytes: the join reads four bins per load
};
static_assert(sizeof(TallyPartial) == 1136 && sizeof(TallyPartial) % 16 == 0, "TallyPartial layout");

enum TallyRec : uint32_t { kTallyRecNone = 0, kTallyRecTiled, kTallyRecPlanes, kTallyRecAoS };

struct TallyArgs : FrameSrc {  // base is never read; desc == nullptr && stride == 0: no lengths
    uint32_t nchunks;          // ceil(ntiles / kTallyChunkTiles)
    uint32_t flags;            // BT_TALLY_*
    const uint8_t* decide;     // n bytes at any alignment, or nullptr
    const uint8_t* records;    // the context's record layout, or nullptr
    uint32_t rec_layout;       // TallyRec
    uint32_t n_cap;            // plane stride (kTallyRecPlanes)
    uint32_t lengths;          // 1: frame lengths are summed (decide and frames both given)
    uint32_t peel;             // histogram by ballot peeling (the default) or by LDS adds (A/B)
    TallyPartial* parts;       // nchunks entries
    bt_tally* out;
};

// The checks of bt_tally_device on everything but the context, and the launch's arguments
// (parts and peel are the caller's). Plain C++ with no device and no runtime state, like
// frame_src: tools/tally_host_check.cpp runs it under the host sanitizers. false: why[0 .. cap)
// holds the reason and *a is unspecified. opt_flags: the context's BT_OPT_* (the record layout).
inline bool tally_args(const uint8_t* decide, uint32_t n, const bt_batch* frames, const void* records, uint32_t n_cap,
                       uint32_t flags, bt_tally* out, uint32_t opt_flags, TallyArgs* a, char* why, size_t cap) {
    const auto no = [&](const char* s) { snprintf(why, cap, "%s", s); return false; };
    if (!out) return no("null out");
    if (reinterpret_cast<uintptr_t>(out) & 7u) return no("out is not 8-byte aligned");
    if (!decide && !records) return no("decide and records both null: nothing to count");
    if (flags & ~(uint32_t)(BT_TALLY_STOP_AT_THROW | BT_TALLY_ACCUMULATE)) return no("unknown flag bits");
    if (records && n_cap < n) return no("records n_cap < n");
    *a = TallyArgs{};
    if (frames) {
        if (frames->n != n) return no("frames->n != n");
        if (frame_src(frames, a, why, cap)) return false;
    }
    a->n = n;
    a->ntiles = (uint32_t)(((uint64_t)n + 63u) / 64u);
    a->nchunks = (a->ntiles + kTallyChunkTiles - 1u) / kTallyChunkTiles;
    a->flags = flags;
    a->decide = decide;
    a->records = static_cast<const uint8_t*>(records);
    a->rec_layout = !records ? kTallyRecNone
                    : (opt_flags & BT_OPT_RECORDS_AOS) ? kTallyRecAoS
                    : (opt_flags & BT_OPT_RECORDS_PLANES) ? kTallyRecPlanes : kTallyRecTiled;
    a->n_cap = n_cap;
    a->lengths = decide && frames ? 1u : 0u;
    a->out = out;
    return true;
}

// Both launches, asynchronous on `stream`; n == 0 launches nothing (the caller writes *out).
int launch_tally(const TallyArgs& a, void* stream, void* timing_start = nullptr, void* timing_stop = nullptr);

}  // namespace bt
