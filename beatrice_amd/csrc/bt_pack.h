// bt_pack.h — ordered pack of the selected frames of a batch (bt_pack.hip), shared with the
// host runtime (bt_pass_pack_device in bt_launch.cpp).
#pragma once

#include <stdint.h>

#include "beatrice_gpu.h"
#include "bt_frames.h"

namespace bt {

// One chunk of the scan = kPackChunkTiles tiles of 64 packets (16,384 packets, as the pass-index
// compaction's kChunkTiles). A chunk's records take < 2^32 bytes (16,384 * (64 + 65,535 + 63)),
// so offsets inside a chunk are 32-bit; the chunk's own offset is 64-bit.
constexpr uint32_t kPackChunkTiles = 256;
constexpr uint32_t kPackLeadMax = 64;

struct PackChunkSum {          // workspace, one per chunk: written by bt_pack_sums
    uint64_t bytes;            // aligned record sizes of the chunk's selected packets, summed
    uint64_t count;            // the chunk's selected packets
};

struct PackArgs : FrameSrc {   // bytes = the exact readable size: source bytes outside [0, bytes) are zeros
    uint32_t nchunks;          // ceil(ntiles / kPackChunkTiles)
    uint32_t lead, snap, align;
    const uint64_t* select;    // ntiles words; bits at or above n are ignored
    uint8_t* out;
    uint64_t cap;
    uint64_t* out_desc;        // optional
    uint64_t* total;
    uint32_t* n_packed;
    PackChunkSum* sums;        // nchunks entries
};

// Both launches, asynchronous on `stream`; n == 0 launches nothing (the caller clears the totals).
int launch_pass_pack(const PackArgs& a, void* stream, void* timing_start = nullptr, void* timing_stop = nullptr);

}  // namespace bt
