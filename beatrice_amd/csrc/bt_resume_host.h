// bt_resume_host.h — the host-only pieces of the two-pass PAYLOAD path: the argument checks of
// bt_filter_resume_device (bt_launch.cpp) and the scan of final decision bytes that builds the
// ring stage's verdict words and counts (bt_ring_stage.cpp). Plain C++ with no device and no
// runtime state, so tools/resume_host_check.cpp runs both under the host sanitizers.
#pragma once

#include <stdint.h>

#include "beatrice_gpu.h"
#include "bt_frames.h"

namespace bt {

// What bt_filter_resume_device refuses, as the message of its BT_E_INVALID_ARGUMENT (valid until
// the thread's next call); nullptr when the arguments are acceptable, with *fs = the frames.
inline const char* resume_args_error(const bt_ctx* ctx, const bt_batch* frames, const bt_outputs* out,
                                     FrameSrc* fs = nullptr) {
    if (!ctx || !frames || !out) return "bt_filter_resume_device: null argument";
    if (frames->flags & (BT_BATCH_PREFIXES | BT_BATCH_LEAN))
        return "bt_filter_resume_device: the resume pass reads whole frames (BT_BATCH_PREFIXES set)";
    if (out->records) return "bt_filter_resume_device: records must be NULL (the first pass wrote what it could)";
    if (!out->decide) return "bt_filter_resume_device: decide == NULL (the first pass's decision bytes)";
    thread_local char msg[160];
    const int k = snprintf(msg, sizeof(msg), "bt_filter_resume_device: ");
    FrameSrc mine;
    return frame_src(frames, fs ? fs : &mine, msg + k, sizeof(msg) - (size_t)k) ? msg : nullptr;
}

// Verdict words [w_lo, w_hi) of n decision bytes: bit i of word j = frame 64 j + i has code
// BT_DECIDE_PASS (verdict may be NULL). Adds the words' passing frames to *pass and the frames
// whose code is still BT_DECIDE_HOST to *host; reads decide[64 w_lo .. min(64 w_hi, n)) only.
inline void decide_scan(const uint8_t* decide, uint32_t n, uint32_t w_lo, uint32_t w_hi, uint64_t* verdict,
                        uint64_t* pass, uint64_t* host) {
    uint64_t p = 0, h = 0;
    for (uint32_t j = w_lo; j < w_hi; ++j) {
        uint64_t bits = 0;
        const uint64_t first = 64ull * j;
        const uint32_t hi = first >= n ? 0u : (n - first < 64u ? (uint32_t)(n - first) : 64u);
        const uint8_t* d = decide + first;
        for (uint32_t i = 0; i < hi; ++i) {
            const uint32_t code = BT_DECIDE_CODE(d[i]);
            bits |= (uint64_t)(code == BT_DECIDE_PASS) << i;
            h += code == BT_DECIDE_HOST;
        }
        if (verdict) verdict[j] = bits;
        p += (uint64_t)__builtin_popcountll(bits);
    }
    *pass += p;
    *host += h;
}

}  // namespace bt
