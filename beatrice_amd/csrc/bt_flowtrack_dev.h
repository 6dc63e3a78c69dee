// bt_flowtrack_dev.h — what the kernels over a flow tracker's state share (bt_flowtrack.hip,
// bt_flowtop.hip, bt_flowhosts.hip): the header check and the copies of a record and of its TCP
// side record. Device code only.
#pragma once

#include "bt_dev_util.h"
#include "bt_flowtrack.h"

namespace bt {
namespace {

// Is the state the tracker the host took the call for? `slots`: the state's own slot count.
template <class A>
__device__ __forceinline__ bool hdr_ok(const A& a, uint32_t slots) {
    const bt_flow_track_hdr* const h = a.hdr;
    return h->magic == BT_FLOW_TRACK_MAGIC && h->flags == a.flags && h->flow_cap == a.flow_cap && h->slots == slots &&
           h->n_flows <= a.flow_cap;
}

__device__ __forceinline__ void rec_copy(bt_flow_track_rec* dst, const bt_flow_track_rec* src) {   // 104 B = 13 words
    const uint64_t* const q = reinterpret_cast<const uint64_t*>(src);
    uint64_t* const o = reinterpret_cast<uint64_t*>(dst);
#pragma unroll
    for (int j = 0; j < 13; ++j) o[j] = q[j];
}

__device__ __forceinline__ void tcp_copy(bt_flow_tcp_rec* dst, const bt_flow_tcp_rec* src) {   // 16 B, 4-byte aligned
    const uint32_t* const q = reinterpret_cast<const uint32_t*>(src);
    uint32_t* const o = reinterpret_cast<uint32_t*>(dst);
#pragma unroll
    for (int j = 0; j < 4; ++j) o[j] = q[j];
}

}  // namespace
}  // namespace bt
