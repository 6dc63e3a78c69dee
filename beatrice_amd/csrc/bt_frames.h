// bt_frames.h — "the frames of a batch", once: the checks on a bt_batch, the form every kernel
// that reads one takes it in (FrameSrc, the head of MainArgs / ResumeArgs / ExArgs / PackArgs), and
// "packet i -> (offset, length)" on the device. The host part is plain C++ with no device and no
// runtime state: tools/frames_host_check.cpp runs it under the host sanitizers.
#pragma once

#include <stdint.h>
#include <cstdio>

#include "beatrice_gpu.h"
#ifdef __HIPCC__
#include <hip/hip_runtime.h>
#endif

namespace bt {

struct FrameSrc {
    const uint8_t* base;       // the frames' bytes
    const uint64_t* desc;      // one descriptor per packet; nullptr: fixed stride
    uint32_t desc_words;       // descriptor stride in u64 words: 1 bt_pkt_desc, 2 xdp_desc
    uint64_t bytes;            // the readable size of base, exact (pack); the entry points of the kernels that
                               // read 16-B chunks (main, resume, extract) put read_limit(base, bytes) here
    uint32_t stride;           // fixed stride: packet i = base[i * stride .. + stride)
    uint32_t n;                // packets
    uint32_t ntiles;           // ceil(n / 64): one wavefront tile = 64 packets
};

// What frame_src found wrong, in the order it looks: null batch / null buffer / zero stride, unknown
// desc_format, `bytes` missing or too small. Entry points that return early for an empty batch or
// a call that asks for nothing report the later kinds only after that, as they always have.
enum FrameCheck { kFramesOk = 0, kFramesUnusable, kFramesFormat, kFramesSize };

// The one set of checks on a bt_batch. kFramesOk: *f is filled; otherwise *f is untouched and
// why[0 .. cap) holds the reason, without the entry point's name.
inline FrameCheck frame_src(const bt_batch* b, FrameSrc* f, char* why, size_t cap) {
    const auto no = [&](FrameCheck k, const char* s) { snprintf(why, cap, "%s", s); return k; };
    if (!b) return no(kFramesUnusable, "null batch");
    if (b->n && !b->base) return no(kFramesUnusable, "null packet buffer");
    if (!b->desc && b->n && !b->stride) return no(kFramesUnusable, "fixed-stride mode needs stride > 0");
    if (b->desc_format > BT_DESC_XDP) {
        snprintf(why, cap, "unknown desc_format %u", b->desc_format);
        return kFramesFormat;
    }
    // descriptor batches must state the readable range of base (a descriptor past it then reads
    // zeros instead of arbitrary memory); fixed-stride batches default to n * stride
    if (b->desc && !b->bytes) return no(kFramesSize, "descriptor batch with bytes == 0 (the readable size of base)");
    const uint64_t need = b->desc ? 0u : (uint64_t)b->n * b->stride;
    if (b->bytes && b->bytes < need) {
        snprintf(why, cap, "fixed-stride batch: bytes %llu < n * stride %llu", (unsigned long long)b->bytes,
                 (unsigned long long)need);
        return kFramesSize;
    }
    *f = {b->base, static_cast<const uint64_t*>(b->desc), b->desc_format == BT_DESC_XDP ? 2u : 1u,
          b->bytes ? b->bytes : need, b->stride, b->n, (uint32_t)(((uint64_t)b->n + 63u) / 64u)};   // n + 63 in 64 bits
    return kFramesOk;
}

// The two descriptor formats, bit by bit (16-bit lengths); constexpr: for host and device code.
constexpr void desc_packed(uint64_t d, uint64_t& off, uint32_t& len) {   // bt_pkt_desc
    off = d & 0xFFFFFFFFFFFFull;
    len = (uint32_t)(d >> 48);
}
constexpr void desc_xdp(uint64_t addr, uint32_t l, uint64_t& off, uint32_t& len) {   // xdp_desc {u64 addr; u32 len; u32 options}
    off = addr;
    len = l > 0xFFFFu ? 0xFFFFu : l;
}

#ifdef __HIPCC__
// Packet i (< a.n): its frame's offset from base and length (fixed stride: the stride, unclamped).
__device__ __forceinline__ void frame_at(const FrameSrc& a, uint32_t i, uint64_t& off, uint32_t& len) {
    if (!a.desc) {
        off = (uint64_t)i * a.stride;
        len = a.stride;
    } else if (a.desc_words == 1) {
        desc_packed(a.desc[i], off, len);
    } else {
        const uint4 d = *reinterpret_cast<const uint4*>(a.desc + 2ull * i);
        desc_xdp(((uint64_t)d.y << 32) | d.x, d.z, off, len);
    }
}
#endif

}  // namespace bt
