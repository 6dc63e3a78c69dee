// bt_hip_launch.h — host-side helpers of the kernel files (*.hip): how large a grid is
// resident, the launch with or without timing events, and the read of a module's bounds log.
#pragma once

#include <hip/hip_ext.h>
#include <hip/hip_runtime.h>

#include <map>
#include <mutex>

#include "bt_device.h"

namespace bt {
namespace {

inline int cu_count() {
    static const int cus = [] {
        int dev = 0;
        hipDeviceProp_t prop;
        return hipGetDevice(&dev) == hipSuccess && hipGetDeviceProperties(&prop, dev) == hipSuccess &&
                       prop.multiProcessorCount > 0
                   ? prop.multiProcessorCount : 256;
    }();
    return cus;
}

// One residency wave of kBlock-thread blocks of `Kernel` with `dyn` bytes of dynamic LDS: a
// persistent grid-stride loop of that many blocks has no tail of late blocks (measured: 2x
// residency cost C3 11 %). Cached per kernel (the template argument) and LDS size; 1024 when
// the occupancy query fails.
template <auto Kernel>
int resident_grid(uint32_t dyn) {
    static std::map<uint32_t, int> blocks_of;
    static std::mutex mu;
    std::lock_guard<std::mutex> lk(mu);
    auto it = blocks_of.find(dyn);
    if (it == blocks_of.end()) {
        int per_cu = 0;
        const bool ok = hipOccupancyMaxActiveBlocksPerMultiprocessor(&per_cu, Kernel, kBlock, dyn) == hipSuccess && per_cu >= 1;
        it = blocks_of.emplace(dyn, ok ? cu_count() * per_cu : 1024).first;
    }
    return it->second;
}

// With a timing event the kernel's own dispatch packet records it (hipExtLaunchKernelGGL), so
// timing a launch adds no packets to the stream.
template <class K, class... Args>
void launch(K kernel, dim3 grid, dim3 block, uint32_t dyn, hipStream_t st, hipEvent_t e0, hipEvent_t e1,
            const Args&... args) {
    if (e0 || e1)
        hipExtLaunchKernelGGL(kernel, grid, block, dyn, st, e0, e1, 0, args...);
    else
        hipLaunchKernelGGL(kernel, grid, block, dyn, st, args...);
}

// The bounds_take_* of a module (bt_device.h) on its log `symbol`.
inline uint32_t bounds_take(const BoundsLog& symbol, void* stream, BoundsLog* first) {
#ifdef BT_DEBUG_BOUNDS
    if (hipStreamSynchronize(reinterpret_cast<hipStream_t>(stream)) != hipSuccess) return 0;
    BoundsLog log{};
    if (hipMemcpyFromSymbol(&log, HIP_SYMBOL(symbol), sizeof(log)) != hipSuccess) return 0;
    if (log.count) {
        const BoundsLog zero{};
        (void)hipMemcpyToSymbol(HIP_SYMBOL(symbol), &zero, sizeof(zero));
        if (first) *first = log;
    }
    return log.count;
#else
    (void)symbol;
    (void)stream;
    (void)first;
    return 0;
#endif
}

}  // namespace
}  // namespace bt
