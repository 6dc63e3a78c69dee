// bt_wave.h — reductions over a wave of 64 lanes and over a block of whole waves, one copy each.
// Every wave_* result reaches every lane. The block forms hold two barriers each: call them
// block-uniformly.
#pragma once

#include "bt_dev_util.h"

namespace bt {
namespace {

__device__ __forceinline__ uint32_t wave_sum(uint32_t v) {
    for (int o = 32; o > 0; o >>= 1) v += __shfl_xor(v, o);
    return v;
}

__device__ __forceinline__ uint32_t wave_min(uint32_t v) {
    for (int o = 32; o > 0; o >>= 1) {
        const uint32_t y = __shfl_xor(v, o);
        v = y < v ? y : v;
    }
    return v;
}

__device__ __forceinline__ uint32_t wave_or(uint32_t v) {
    for (int o = 32; o > 0; o >>= 1) v |= __shfl_xor(v, o);
    return v;
}

__device__ __forceinline__ uint64_t wave_sum64(uint64_t v) {
    for (int o = 32; o > 0; o >>= 1)
        v += ((uint64_t)__shfl_xor((uint32_t)(v >> 32), o) << 32) | __shfl_xor((uint32_t)v, o);
    return v;
}

__device__ __forceinline__ uint64_t wave_min64(uint64_t v) {
    for (int o = 32; o > 0; o >>= 1) {
        const uint64_t y = ((uint64_t)__shfl_xor((uint32_t)(v >> 32), o) << 32) | __shfl_xor((uint32_t)v, o);
        v = y < v ? y : v;
    }
    return v;
}

__device__ __forceinline__ uint64_t wave_max64(uint64_t v) {
    for (int o = 32; o > 0; o >>= 1) {
        const uint64_t y = ((uint64_t)__shfl_xor((uint32_t)(v >> 32), o) << 32) | __shfl_xor((uint32_t)v, o);
        v = y > v ? y : v;
    }
    return v;
}

__device__ __forceinline__ uint32_t wave_max32(uint32_t v) {
    for (int o = 32; o > 0; o >>= 1) {
        const uint32_t y = __shfl_xor(v, o);
        v = y > v ? y : v;
    }
    return v;
}

// Is this lane the only lane of the wave that is `in` with its key? slots: 256 bytes of LDS of the
// wave's own. Every lane that is `in` writes its number into the byte its key picks; the lane whose
// number stays is the slot's winner, a lane that finds another lane of its own key there marks the
// slot, and a winner whose slot is unmarked has no second lane of its key, since one key is one
// slot. A lane that merely shares a slot with another key is not alone. Call it wave-uniformly.
// (bt_flowstat_update holds the same statements inline: through this helper its code differs by an
// instruction.)
__device__ __forceinline__ bool wave_alone(uint8_t* slots, bool in, uint32_t key, uint32_t lane) {
    uint8_t* const my_slot = &slots[key & 255u];
    if (in) *my_slot = (uint8_t)lane;
    wave_lds_sync();
    const uint32_t won = in ? *my_slot : lane;                         // the lane whose number stayed in the slot
    const uint32_t won_key = (uint32_t)__shfl((int)key, (int)won);     // ... and its key
    wave_lds_sync();
    if (in && won != lane && won_key == key) *my_slot = 0xFFu;         // the winner's key has a second lane
    wave_lds_sync();
    return in && won == lane && *my_slot == (uint8_t)lane;
}

// The exclusive scan of v over a block of Threads threads, and the sum in *total; sh: Threads / 64 words.
template <uint32_t Threads>
__device__ __forceinline__ uint32_t block_excl(uint32_t v, uint32_t* sh, uint32_t* total) {
    const uint32_t lane = threadIdx.x & 63u, wid = threadIdx.x >> 6;
    uint32_t incl = v;
    for (int o = 1; o < 64; o <<= 1) {
        const uint32_t y = __shfl_up(incl, o);
        if (lane >= (uint32_t)o) incl += y;
    }
    if (lane == 63u) sh[wid] = incl;
    __syncthreads();
    uint32_t pre = 0, tot = 0;
#pragma unroll
    for (uint32_t w = 0; w < Threads / 64u; ++w) {
        const uint32_t x = sh[w];
        pre += w < wid ? x : 0u;
        tot += x;
    }
    __syncthreads();
    *total = tot;
    return pre + incl - v;
}

// The sum of v over a block of Threads threads, to every thread; sh: Threads / 64 words.
template <uint32_t Threads>
__device__ __forceinline__ uint64_t block_sum64(uint64_t v, uint64_t* sh) {
    v = wave_sum64(v);
    if ((threadIdx.x & 63u) == 0u) sh[threadIdx.x >> 6] = v;
    __syncthreads();
    uint64_t tot = 0;
#pragma unroll
    for (uint32_t w = 0; w < Threads / 64u; ++w) tot += sh[w];
    __syncthreads();
    return tot;
}

}  // namespace
}  // namespace bt
