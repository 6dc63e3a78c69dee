// bt_fanout.h — the K-way fan-out of a batch by RSS flow hash (bt_fanout.hip), shared with the
// host runtime (bt_flow_fanout_device / bt_flow_hash_host in bt_fanout_host.cpp): the argument
// checks with the resolved key and indirection table, the flow key of a frame and the Toeplitz
// hash on the host. The host part is plain C++ with no device and no runtime state:
// tools/fanout_host_check.cpp runs it under the host sanitizers.
#pragma once

#include <stdint.h>
#include <cstring>

#include "beatrice_gpu.h"
#include "bt_frames.h"

namespace bt {

// One chunk of the partition = 256 tiles of 64 packets, as the compaction, the pack and the tally.
constexpr uint32_t kFanChunkTiles = 256;
constexpr uint32_t kFanChunk = kFanChunkTiles * 64u;
constexpr uint32_t kFanWaves = 8;              // waves of a chunk's block: wave w has tiles 32 w .. 32 w + 31 of it
constexpr uint32_t kFanJoinThreads = 1024;
constexpr uint32_t kFanKeyBytes = 40, kFanKeyWords = 10, kFanReta = 128;
constexpr uint32_t kFanInputMax = 36;            // IPv6 addresses + ports
constexpr uint32_t kFanNibbles = 2 * kFanInputMax;

struct FanoutPartial {            // workspace, one per chunk: written by bt_fanout_keys
    uint32_t wcount[kFanWaves][64];   // selected packets of wave w's tiles by queue
    uint32_t count[64];           // ... of the whole chunk
    uint64_t bytes[64];           // the chunk's selected frame lengths by queue
    uint32_t klass[5];            // its selected packets by BT_FLOW_*
    uint32_t pad[3];
};
static_assert(sizeof(FanoutPartial) == 2848 && sizeof(FanoutPartial) % 16 == 0, "FanoutPartial layout");
static_assert(sizeof(bt_fanout_result) == 808, "bt_fanout_result layout");

// The workspace of a call over nchunks chunks: the partials, then 64 words per chunk (where the
// chunk's packets of queue q start inside queue q's range of idx).
constexpr size_t fan_ws_bytes(uint32_t nchunks) { return (size_t)nchunks * (sizeof(FanoutPartial) + 64u * 4u); }

struct FanoutArgs : FrameSrc {    // bytes = the first offset no 16-B chunk of the parse kernel reads (fan_read_end)
    uint32_t nchunks;             // ceil(ntiles / kFanChunkTiles)
    uint32_t queues;              // 1..64
    uint32_t l3_only;             // never hash ports
    uint32_t table;               // Toeplitz by nibble tables in LDS (1) or bit-serial with the key in SGPRs (0)
    uint32_t key[kFanKeyWords];   // the key as big-endian words: word k = key bits 32 k .. 32 k + 31, MSB first
    uint32_t reta[kFanReta / 4];  // the indirection table, four entries per little-endian word
    const uint64_t* select;       // verdict-layout words, or nullptr = all n
    uint32_t* hash;               // optional outputs, as bt_fanout_out
    uint8_t* queue;               // never nullptr for the kernels: the workspace's array when the caller has none
    uint32_t* idx;
    uint64_t* select_q;
    bt_fanout_result* result;
    FanoutPartial* parts;         // nchunks entries
    uint32_t* rel;                // nchunks * 64
};

// RSS verification key (the default) and the key of 0x6d5a repeated (symmetric in source and destination).
inline void fan_default_key(uint8_t key[kFanKeyBytes]) {
    static const uint8_t k[kFanKeyBytes] = {0x6d, 0x5a, 0x56, 0xda, 0x25, 0x5b, 0x0e, 0xc2, 0x41, 0x67, 0x25, 0x3d, 0x43, 0xa3,
                                            0x8f, 0xb0, 0xd0, 0xca, 0x2b, 0xcb, 0xae, 0x7b, 0x30, 0xb4, 0x77, 0xcb, 0x2d, 0xa3,
                                            0x80, 0x30, 0xf2, 0x0c, 0x6a, 0x42, 0xb7, 0x3b, 0xbe, 0xac, 0x01, 0xfa};
    memcpy(key, k, kFanKeyBytes);
}
inline void fan_symmetric_key(uint8_t key[kFanKeyBytes]) {
    for (uint32_t i = 0; i < kFanKeyBytes; i += 2) { key[i] = 0x6d; key[i + 1] = 0x5a; }
}

// The checks on a bt_fanout_opts and what it resolves to. false: why[0 .. cap) holds the reason.
inline bool fanout_opts(const bt_fanout_opts* o, uint8_t key[kFanKeyBytes], uint8_t reta[kFanReta], char* why, size_t cap) {
    const auto no = [&](const char* s) { snprintf(why, cap, "%s", s); return false; };
    if (!o) return no("null opts");
    if (o->queues < 1u || o->queues > BT_FANOUT_MAX_QUEUES) return no("queues outside 1..64");
    constexpr uint32_t known = BT_FANOUT_KEY_USER | BT_FANOUT_KEY_SYMMETRIC | BT_FANOUT_RETA_USER | BT_FANOUT_L3_ONLY;
    if (o->flags & ~known) return no("unknown flag bits");
    if ((o->flags & BT_FANOUT_KEY_USER) && (o->flags & BT_FANOUT_KEY_SYMMETRIC)) return no("both key flags set");
    if (o->flags & BT_FANOUT_KEY_USER) memcpy(key, o->key, kFanKeyBytes);
    else if (o->flags & BT_FANOUT_KEY_SYMMETRIC) fan_symmetric_key(key);
    else fan_default_key(key);
    for (uint32_t i = 0; i < kFanReta; ++i) {
        reta[i] = (o->flags & BT_FANOUT_RETA_USER) ? o->reta[i] : (uint8_t)(i % o->queues);
        if (reta[i] >= o->queues) return no("reta entry >= queues");
    }
    return true;
}

// The first offset from base that the parse kernel's 16-B chunks (at 16-B offsets from base) do
// not read: a byte at or past it reads as zero, a byte below it lies inside the 16-B granules
// (by absolute address) of [base, base + bytes). The rule of read_limit (bt_device.h).
inline uint64_t fan_read_end(const void* base, uint64_t bytes) {
    const uint64_t b = (uint64_t)(uintptr_t)base;
    return bytes ? (((b + bytes + 15u) & ~15ull) - b) & ~15ull : 0u;
}

// The checks of bt_flow_fanout_device on everything but the context, and the launch's arguments
// (parts, rel, table and a stand-in for a null out->queue are the caller's).
inline bool fanout_args(const bt_batch* frames, const uint64_t* select, const bt_fanout_opts* opts, const bt_fanout_out* out,
                        FanoutArgs* a, char* why, size_t cap) {
    const auto no = [&](const char* s) { snprintf(why, cap, "%s", s); return false; };
    if (!frames) return no("null frames");
    if (!opts) return no("null opts");
    if (!out) return no("null out");
    if (!out->result) return no("null result");
    if (reinterpret_cast<uintptr_t>(out->result) & 7u) return no("result is not 8-byte aligned");
    if (frames->flags & (BT_BATCH_PREFIXES | BT_BATCH_LEAN))
        return no("a BT_BATCH_PREFIXES / BT_BATCH_LEAN batch holds no whole frames to key");
    uint8_t key[kFanKeyBytes], reta[kFanReta];
    if (!fanout_opts(opts, key, reta, why, cap)) return false;
    *a = FanoutArgs{};
    if (frame_src(frames, a, why, cap)) return false;
    a->bytes = fan_read_end(a->base, a->bytes);
    a->nchunks = (a->ntiles + kFanChunkTiles - 1u) / kFanChunkTiles;
    a->queues = opts->queues;
    a->l3_only = (opts->flags & BT_FANOUT_L3_ONLY) ? 1u : 0u;
    for (uint32_t k = 0; k < kFanKeyWords; ++k)
        a->key[k] = (uint32_t)key[4 * k] << 24 | (uint32_t)key[4 * k + 1] << 16 | (uint32_t)key[4 * k + 2] << 8 | key[4 * k + 3];
    for (uint32_t k = 0; k < kFanReta / 4; ++k)
        a->reta[k] = (uint32_t)reta[4 * k] | (uint32_t)reta[4 * k + 1] << 8 | (uint32_t)reta[4 * k + 2] << 16 |
                     (uint32_t)reta[4 * k + 3] << 24;
    a->select = select;
    a->hash = out->hash;
    a->queue = out->queue;
    a->idx = out->idx;
    a->select_q = out->select_q;
    a->result = out->result;
    return true;
}

// The host's layer walk over frame[0 .. len) (DESIGN.md §2 as far as a flow key needs it), the one
// copy under flow_key_host and flowtcp_frame_host (bt_flowtcp.h). Plain byte-wise C++ that shares
// nothing with the device's walk (bt_flow_walk.h): it is what the device is held to. Every byte
// read lies below len.
struct FlowLayersHost {
    bool v4, v6;        // a whole IPv4 / IPv6 header behind at most two tags
    bool l4;            // protocol 6 or 17, its whole header (20 / 8 bytes) inside the frame, and for
                        // IPv4 neither MF nor a fragment offset: the rule under which the key takes ports
    uint32_t proto;     // IPv4 protocol / IPv6 next header (no extension headers are walked)
    uint32_t o3, o4;    // where L3 and L4 start; o4 only with v4 or v6
};

inline FlowLayersHost flow_layers_host(const uint8_t* f, uint32_t len) {
    FlowLayersHost L{};
    if (len < 14u) return L;
    const auto be16 = [&](uint32_t o) { return (uint32_t)f[o] << 8 | f[o + 1]; };
    uint32_t et = be16(12), k = 0;
    while (k < 2u && (et == 0x8100u || et == 0x88A8u)) {
        if (len < 18u + 4u * k) return L;   // the tag, or the EtherType after it, is not in the frame
        et = be16(16u + 4u * k);
        ++k;
    }
    L.o3 = 14u + 4u * k;
    bool fragment = false;
    if (et == 0x0800u && len - L.o3 >= 20u) {
        L.v4 = true;
        L.proto = f[L.o3 + 9u];
        L.o4 = L.o3 + 4u * (f[L.o3] & 0xFu);
        fragment = (be16(L.o3 + 6u) & 0x3FFFu) != 0;   // MF or a fragment offset: addresses only
    } else if (et == 0x86DDu && len - L.o3 >= 40u) {
        L.v6 = true;
        L.proto = f[L.o3 + 6u];
        L.o4 = L.o3 + 40u;
    } else {
        return L;
    }
    const uint32_t need = L.proto == 6u ? 20u : L.proto == 17u ? 8u : 0u;
    L.l4 = need && !fragment && L.o4 <= len && len - L.o4 >= need;
    return L;
}

// The flow key of a frame: in[0 .. returned) and the class. Every byte read lies below len.
inline uint32_t flow_key_host(const uint8_t* f, uint32_t len, bool l3_only, uint8_t in[kFanInputMax], uint32_t* klass) {
    const FlowLayersHost L = flow_layers_host(f, len);
    const bool ports = L.l4 && !l3_only;
    *klass = L.v4 ? (ports ? BT_FLOW_V4_L4 : BT_FLOW_V4) : L.v6 ? (ports ? BT_FLOW_V6_L4 : BT_FLOW_V6) : BT_FLOW_NONE;
    if (!L.v4 && !L.v6) return 0;
    const uint32_t na = L.v4 ? 8u : 32u;   // both addresses: L3 bytes 12 .. 19 / 8 .. 39
    memcpy(in, f + L.o3 + (L.v4 ? 12u : 8u), na);
    if (ports) memcpy(in + na, f + L.o4, 4);
    return ports ? na + 4u : na;
}

// Toeplitz hash of in[0 .. n) (n <= 36) under a 40-byte key, MSB first: for every set bit i of
// the input, the 32 key bits from bit i on are XORed into the result.
inline uint32_t toeplitz_host(const uint8_t key[kFanKeyBytes], const uint8_t* in, uint32_t n) {
    uint32_t h = 0;
    uint64_t win = 0;   // the upper 32 bits: the key bits from the current input bit on
    for (uint32_t k = 0; k < 8u; ++k) win = win << 8 | key[k];
    for (uint32_t i = 0; i < n; ++i) {
        for (uint32_t b = 0; b < 8u; ++b) {
            if (in[i] & (0x80u >> b)) h ^= (uint32_t)(win >> 32);
            win <<= 1;
        }
        win |= i + 8u < kFanKeyBytes ? key[i + 8u] : 0u;   // the low byte is empty again after 8 shifts
    }
    return h;
}

// All three launches, asynchronous on `stream`; n == 0 launches nothing (the caller writes *result).
int launch_fanout(const FanoutArgs& a, void* stream, void* timing_start = nullptr, void* timing_stop = nullptr);

}  // namespace bt
