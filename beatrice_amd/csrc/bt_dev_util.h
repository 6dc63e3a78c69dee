// bt_dev_util.h — device-side helpers that more than one kernel file uses, one copy each.
#pragma once

#include <hip/hip_runtime.h>

#include "bt_device.h"

namespace bt {
namespace {

typedef unsigned int u32x2 __attribute__((ext_vector_type(2)));
typedef unsigned int u32x4 __attribute__((ext_vector_type(4)));

__device__ __forceinline__ void wave_lds_sync() {
    // Lanes of one wavefront hand rows to each other through LDS: keep the compiler
    // from moving LDS accesses across this point and drain the LDS queue.
    __builtin_amdgcn_fence(__ATOMIC_RELEASE, "wavefront");
    __builtin_amdgcn_wave_barrier();
    __builtin_amdgcn_fence(__ATOMIC_ACQUIRE, "wavefront");
}

__device__ __forceinline__ uint32_t byte_of(const uint32_t* w, int i) {
    return (w[i >> 2] >> (8 * (i & 3))) & 0xFFu;
}
__device__ __forceinline__ uint32_t be16_of(const uint32_t* w, int i) {
    return (byte_of(w, i) << 8) | byte_of(w, i + 1);
}

// The slot words tab[0 .. slots) of a hash table to `empty` with 16-byte stores, a share per thread
// of a grid of blocks of Threads threads; tab is 16-byte aligned and slots a multiple of 4 (of 128,
// in every table here).
template <uint32_t Threads>
__device__ __forceinline__ void slots_fill(uint32_t* tab, uint32_t slots, uint32_t empty) {
    u32x4* const q = reinterpret_cast<u32x4*>(tab);
    const uint64_t nq = slots / 4u, step = (uint64_t)gridDim.x * Threads;
    for (uint64_t x = (uint64_t)blockIdx.x * Threads + threadIdx.x; x < nq; x += step) q[x] = u32x4{empty, empty, empty, empty};
}

// K little-endian dwords starting at byte `a` of the LDS image (any alignment).
template <int K>
__device__ __forceinline__ void window(const uint32_t* lds, uint32_t a, uint32_t* out) {
    const uint32_t d = a >> 2, sh = a & 3u;
    uint32_t prev = lds[d];
#pragma unroll
    for (int k = 0; k < K; ++k) {
        uint32_t next = lds[d + k + 1];
        out[k] = __builtin_amdgcn_alignbyte(next, prev, sh);
        prev = next;
    }
}

// The whole block copies the program's PAYLOAD DFA pool into its dynamic LDS once (call it
// block-uniformly). `log` = the calling module's bounds log.
__device__ __forceinline__ void copy_dfa_pool(uint4* lds, const uint8_t* dfa, uint32_t dfa_bytes, BoundsLog* log) {
    const uint4* src = reinterpret_cast<const uint4*>(dfa);
    for (uint32_t k = threadIdx.x; k < (dfa_bytes + 15u) / 16u && BT_IN(log, kSitePayload, 16u * k, kDfaPoolMax); k += kBlock)
        lds[k] = src[k];
    __syncthreads();
}

}  // namespace
}  // namespace bt
