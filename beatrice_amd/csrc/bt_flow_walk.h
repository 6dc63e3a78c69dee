// bt_flow_walk.h — the flow kernels' layer walk (DESIGN.md §2 as far as a flow key needs it), once,
// for any argument type that derives from FrameSrc (`bytes` = fan_read_end): where L3 and L4
// start, whether the frame holds a whole L4 header, the fragment rule, the key words and their
// canonical direction. Device code only, and the device's only copy: bt_fanout.hip, bt_flowtab.hip
// and bt_flowtcp.hip all walk a frame through flow_layers and flow_key_words. The host's walk is
// flow_layers_host (bt_fanout.h), kept apart on purpose: it is the oracle the tests hold this one
// to (tests/test_gpu_flow_walk.py).
#pragma once

#include "bt_dev_util.h"
#include "bt_frames.h"

namespace bt {
namespace {

typedef u32x4 fw_u32x4_any __attribute__((aligned(1)));   // loads at any byte alignment
typedef u32x2 fw_u32x2_any __attribute__((aligned(1)));
typedef uint32_t fw_u32_any __attribute__((aligned(1)));

// W dwords (1, 2 or 4) from offset x of base, little-endian; `on` false: zeros, nothing loaded.
// A byte is read only below a.bytes and reads as zero at or past it.
template <int W, class A>
__device__ __forceinline__ void fw_load_at(const A& a, uint64_t x, bool on, uint32_t* v) {
#pragma unroll
    for (int k = 0; k < W; ++k) v[k] = 0u;
    if (!on || x >= a.bytes) return;
    if (a.bytes - x >= 4u * W) {
        const uint8_t* p = a.base + x;
        if (W == 4) {
            const u32x4 t = *reinterpret_cast<const fw_u32x4_any*>(p);
            v[0] = t.x; v[1] = t.y; v[2] = t.z; v[3] = t.w;
        } else if (W == 2) {
            const u32x2 t = *reinterpret_cast<const fw_u32x2_any*>(p);
            v[0] = t.x; v[1] = t.y;
        } else {
            v[0] = *reinterpret_cast<const fw_u32_any*>(p);
        }
        return;
    }
    const uint32_t have = (uint32_t)(a.bytes - x);   // 1 .. 4 W - 1 bytes before the limit
#pragma unroll
    for (int b = 0; b < 4 * W; ++b)
        if ((uint32_t)b < have) v[b >> 2] |= (uint32_t)a.base[x + b] << (8 * (b & 3));
}

__device__ __forceinline__ uint32_t fw_be32(uint32_t le) { return __builtin_bswap32(le); }

__device__ __forceinline__ bool fw_is_tag(uint32_t et) { return et == 0x8100u || et == 0x88A8u; }

// What the walk found of the frame at [off, off + len).
struct FlowLayers {
    bool v4, v6;          // a whole IPv4 / IPv6 header behind at most two tags
    bool l4;              // protocol 6 or 17, its whole header (20 / 8 bytes) inside the frame, and for
                          // IPv4 neither MF nor a fragment offset: the rule under which the key takes ports
    uint32_t proto;       // IPv4 protocol / IPv6 next header (no extension headers are walked)
    uint32_t o3, o4;      // where L3 and L4 start
    uint32_t B[4];        // L3 bytes 4 .. 19
};

template <class A>
__device__ __forceinline__ void flow_layers(const A& a, uint64_t off, uint32_t len, bool live, FlowLayers& L) {
    live = live && len >= 14u;
    uint32_t F[4];   // frame bytes 12 .. 27
    fw_load_at<4>(a, off + 12u, live, F);
    uint32_t et = be16_of(F, 0), k = 0;
    bool stop = !live;
#pragma unroll
    for (uint32_t j = 0; j < 2u; ++j) {
        if (!stop && fw_is_tag(et)) {
            if (len < 18u + 4u * j) stop = true;   // the tag, or the EtherType after it, is not in the frame
            else { et = be16_of(F, 4 + 4 * (int)j); k = j + 1u; }
        }
    }
    L.o3 = 14u + 4u * k;
    const uint32_t b0 = k == 0u ? byte_of(F, 2) : k == 1u ? byte_of(F, 6) : byte_of(F, 10);   // frame[o3]
    L.v4 = !stop && et == 0x0800u && len - L.o3 >= 20u;
    L.v6 = !stop && et == 0x86DDu && len - L.o3 >= 40u;
    fw_load_at<4>(a, off + L.o3 + 4u, L.v4 || L.v6, L.B);
    L.proto = L.v4 ? byte_of(L.B, 5) : byte_of(L.B, 2);
    const uint32_t need = L.proto == 6u ? 20u : L.proto == 17u ? 8u : 0u;
    L.o4 = L.v4 ? L.o3 + 4u * (b0 & 0xFu) : L.o3 + 40u;
    L.l4 = (L.v4 || L.v6) && need && L.o4 <= len && len - L.o4 >= need;
    if (L.v4 && (be16_of(L.B, 2) & 0x3FFFu)) L.l4 = false;   // MF or a fragment offset: addresses only
}

// The flow key of a walked frame as big-endian words w[0 .. nw), and its class; `ports`: the key
// takes them (L.l4 and not L3-only).
template <class A>
__device__ __forceinline__ uint32_t flow_key_words(const A& a, uint64_t off, const FlowLayers& L, bool ports, uint32_t (&w)[9],
                                                   uint32_t& nw) {
    uint32_t C[4], D[2], P[1];
    fw_load_at<4>(a, off + L.o3 + 20u, L.v6, C);         // IPv6 bytes 20 .. 35
    fw_load_at<2>(a, off + L.o3 + 36u, L.v6, D);         // IPv6 bytes 36 .. 39 and the ports behind the header
    fw_load_at<1>(a, off + L.o4, L.v4 && ports, P);
#pragma unroll
    for (int d = 0; d < 9; ++d) w[d] = 0u;
    if (L.v4) {
        w[0] = fw_be32(L.B[2]); w[1] = fw_be32(L.B[3]);
        if (ports) w[2] = fw_be32(P[0]);
        nw = ports ? 3u : 2u;
        return ports ? BT_FLOW_V4_L4 : BT_FLOW_V4;
    }
    if (L.v6) {
        w[0] = fw_be32(L.B[1]); w[1] = fw_be32(L.B[2]); w[2] = fw_be32(L.B[3]);
        w[3] = fw_be32(C[0]); w[4] = fw_be32(C[1]); w[5] = fw_be32(C[2]); w[6] = fw_be32(C[3]);
        w[7] = fw_be32(D[0]);
        if (ports) w[8] = fw_be32(D[1]);
        nw = ports ? 9u : 8u;
        return ports ? BT_FLOW_V6_L4 : BT_FLOW_V6;
    }
    nw = 0u;
    return BT_FLOW_NONE;
}

// Both steps, for a caller that needs the key alone: the key and class of the frame at
// [off, off + len) under a.l3_only.
template <class A>
__device__ __forceinline__ uint32_t flow_key(const A& a, uint64_t off, uint32_t len, bool live, uint32_t (&w)[9], uint32_t& nw) {
    FlowLayers L;
    flow_layers(a, off, len, live, L);
    return flow_key_words(a, off, L, L.l4 && !a.l3_only, w, nw);
}

// BT_FLOWTAB_BIDIRECTIONAL: endpoint A (source address, source port) against B as byte strings,
// which is the order of the big-endian words. A > B: direction 1, and w leaves with the endpoints
// exchanged, which is the form the table stores.
__device__ __forceinline__ uint32_t flow_canonical(uint32_t klass, uint32_t (&w)[9]) {
    if (klass == BT_FLOW_V4 || klass == BT_FLOW_V4_L4) {
        const uint32_t sp = w[2] >> 16, dp = w[2] & 0xFFFFu;   // both 0 without ports
        if (w[0] < w[1] || (w[0] == w[1] && sp <= dp)) return 0u;
        const uint32_t t = w[0];
        w[0] = w[1]; w[1] = t;
        w[2] = dp << 16 | sp;
        return 1u;
    }
    if (klass == BT_FLOW_V6 || klass == BT_FLOW_V6_L4) {
        int c = 0;   // the first differing word decides
#pragma unroll
        for (int d = 0; d < 4; ++d)
            if (c == 0 && w[d] != w[d + 4]) c = w[d] < w[d + 4] ? -1 : 1;
        const uint32_t sp = w[8] >> 16, dp = w[8] & 0xFFFFu;
        if (c < 0 || (c == 0 && sp <= dp)) return 0u;
#pragma unroll
        for (int d = 0; d < 4; ++d) { const uint32_t t = w[d]; w[d] = w[d + 4]; w[d + 4] = t; }
        w[8] = dp << 16 | sp;
        return 1u;
    }
    return 0u;
}

// The direction alone: w stays as it is.
__device__ __forceinline__ uint32_t flow_direction(uint32_t klass, const uint32_t (&w)[9]) {
    uint32_t t[9];
#pragma unroll
    for (int d = 0; d < 9; ++d) t[d] = w[d];
    return flow_canonical(klass, t);
}

}  // namespace
}  // namespace bt
