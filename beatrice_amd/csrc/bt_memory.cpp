// bt_memory.cpp — memory the caller hands to or takes from a context: host ranges
// registered for the device (bt_host_register), device allocations, and the synchronous
// copies through the context's two pinned chunks.
#include <algorithm>
#include <cstdlib>
#include <cstring>
#include <mutex>

#include "bt_ctx.h"
#include "bt_hip_util.h"

using namespace bt;

extern "C" {

int bt_host_register(bt_ctx* c, void* host, uint64_t bytes, void** dev_alias) {
    const bt::DeviceRestore keep_device;   // the caller's current device, restored on return
    if (!c || !host || !dev_alias || !bytes) return set_error(BT_E_INVALID_ARGUMENT, "null argument / empty range");
    {
        std::lock_guard<std::mutex> lk(c->mu);
        for (const auto& r : c->host_regs)
            if (r.first == (uintptr_t)host)
                return set_error(BT_E_INVALID_ARGUMENT, "%p is already registered on this context", host);
    }
    // whole pages, in the process's one table (bt_pin.h): a range inside pages another
    // registration holds shares them, one that holds only some of them is refused
    uint8_t* alias = nullptr;
    if (int rc = bt::pin_acquire(host, bytes, &c->device, 1, &alias)) return rc;
    *dev_alias = alias;
    std::lock_guard<std::mutex> lk(c->mu);
    c->host_regs.emplace_back((uintptr_t)host, bytes);
    return BT_OK;
}

int bt_host_unregister(bt_ctx* c, void* host) {
    const bt::DeviceRestore keep_device;   // the caller's current device, restored on return
    if (!c || !host) return set_error(BT_E_INVALID_ARGUMENT, "null argument");
    uint64_t bytes = 0;
    {
        std::lock_guard<std::mutex> lk(c->mu);
        for (const auto& r : c->host_regs)
            if (r.first == (uintptr_t)host) bytes = r.second;
    }
    if (!bytes) return set_error(BT_E_INVALID_ARGUMENT, "%p is not registered on this context", host);
    // the last reference waits for every device that holds an alias of the pages (queued
    // kernels that read or write them) before they are unregistered
    if (int rc = bt::pin_release(host, bytes)) return rc;
    std::lock_guard<std::mutex> lk(c->mu);   // host_resident's cache (read under mu): the
    c->last_base = nullptr;                   // address may come back as another kind
    auto& r = c->host_regs;
    r.erase(std::remove_if(r.begin(), r.end(), [host](const auto& x) { return x.first == (uintptr_t)host; }), r.end());
    return BT_OK;
}

int bt_dev_malloc(bt_ctx* c, uint64_t bytes, void** out) {
    const bt::DeviceRestore keep_device;   // the caller's current device, restored on return
    if (!c || !out) return set_error(BT_E_INVALID_ARGUMENT, "null argument");
    HIP_TRY(hipSetDevice(c->device));
    static const unsigned flags = [] {
        const char* e = getenv("BT_MALLOC_FLAGS");   // experiments: 4 = hipDeviceMallocContiguous
        return e ? (unsigned)strtoul(e, nullptr, 0) : 0u;
    }();
    if (flags) HIP_TRY(hipExtMallocWithFlags(out, bytes ? bytes : 16, flags));
    else HIP_TRY(hipMalloc(out, bytes ? bytes : 16));
    return BT_OK;
}

int bt_dev_free(bt_ctx* c, void* p) {
    const bt::DeviceRestore keep_device;   // the caller's current device, restored on return
    if (!c) return set_error(BT_E_INVALID_ARGUMENT, "null context");
    if (!p) return BT_OK;
    HIP_TRY(hipSetDevice(c->device));
    HIP_TRY(hipFree(p));   // implicitly waits for the device: no queued kernel still uses p
    std::lock_guard<std::mutex> lk(c->mu);
    c->last_base = nullptr;   // host_resident's cache (as bt_host_unregister)
    return BT_OK;
}

}  // extern "C"

namespace {

constexpr size_t kXferChunk = size_t(8) << 20;

// The copies run on the context stream; work queued on the compaction stream
// (bt_parse_filter_device_async) is waited for first, so a copy issued after an async call
// sees its pass list. Work on a caller's own stream is the caller's to synchronise.
int after_cstream(bt_ctx* c) {
    if (!c->ws.cstream) return BT_OK;
    if (!c->xfer.after) HIP_TRY(hipEventCreateWithFlags(&c->xfer.after, hipEventDisableTiming));
    HIP_TRY(hipEventRecord(c->xfer.after, c->ws.cstream));
    HIP_TRY(hipStreamWaitEvent(c->stream, c->xfer.after, 0));
    return BT_OK;
}

int ensure_xfer(bt_ctx* c) {
    for (int k = 0; k < 2; ++k) {
        if (!c->xfer.h[k]) HIP_TRY(hipHostMalloc(&c->xfer.h[k], kXferChunk, hipHostMallocDefault));
        if (!c->xfer.ev[k]) HIP_TRY(hipEventCreateWithFlags(&c->xfer.ev[k], hipEventDisableTiming));
    }
    return BT_OK;
}

}  // namespace

extern "C" {

// Both copies go through the context's two pinned chunks (host memcpy of chunk k while the
// DMA of chunk k^1 runs), so no DMA touches the caller's (usually pageable) memory; they
// are ordered after the context's streams (after_cstream) and complete before returning.
int bt_memcpy_h2d(bt_ctx* c, void* dst, const void* src, uint64_t bytes) {
    const bt::DeviceRestore keep_device;   // the caller's current device, restored on return
    if (!c) return set_error(BT_E_INVALID_ARGUMENT, "null context");
    if (bytes && (!dst || !src)) return set_error(BT_E_INVALID_ARGUMENT, "null pointer");
    std::lock_guard<std::mutex> lk(c->xfer.mu);
    HIP_TRY(hipSetDevice(c->device));
    if (int rc = ensure_xfer(c)) return rc;
    if (int rc = after_cstream(c)) return rc;
    bool used[2] = {false, false};
    int k = 0;
    for (uint64_t off = 0; off < bytes; off += kXferChunk, k ^= 1) {
        const size_t n = (size_t)std::min<uint64_t>(kXferChunk, bytes - off);
        if (used[k]) HIP_TRY(hipEventSynchronize(c->xfer.ev[k]));   // its last DMA has read it
        std::memcpy(c->xfer.h[k], static_cast<const uint8_t*>(src) + off, n);
        HIP_TRY(hipMemcpyAsync(static_cast<uint8_t*>(dst) + off, c->xfer.h[k], n, hipMemcpyHostToDevice, c->stream));
        HIP_TRY(hipEventRecord(c->xfer.ev[k], c->stream));
        used[k] = true;
    }
    HIP_TRY(hipStreamSynchronize(c->stream));
    return BT_OK;
}

int bt_memcpy_d2h(bt_ctx* c, void* dst, const void* src, uint64_t bytes) {
    const bt::DeviceRestore keep_device;   // the caller's current device, restored on return
    if (!c) return set_error(BT_E_INVALID_ARGUMENT, "null context");
    if (bytes && (!dst || !src)) return set_error(BT_E_INVALID_ARGUMENT, "null pointer");
    std::lock_guard<std::mutex> lk(c->xfer.mu);
    HIP_TRY(hipSetDevice(c->device));
    if (int rc = ensure_xfer(c)) return rc;
    if (int rc = after_cstream(c)) return rc;
    // chunk i lands in buffer i & 1; chunk i + 1's DMA runs while chunk i is copied out
    auto issue = [&](uint64_t off, int k) -> int {
        const size_t n = (size_t)std::min<uint64_t>(kXferChunk, bytes - off);
        HIP_TRY(hipMemcpyAsync(c->xfer.h[k], static_cast<const uint8_t*>(src) + off, n, hipMemcpyDeviceToHost, c->stream));
        HIP_TRY(hipEventRecord(c->xfer.ev[k], c->stream));
        return BT_OK;
    };
    if (bytes) { if (int rc = issue(0, 0)) return rc; }
    int k = 0;
    for (uint64_t off = 0; off < bytes; off += kXferChunk, k ^= 1) {
        if (off + kXferChunk < bytes) { if (int rc = issue(off + kXferChunk, k ^ 1)) return rc; }
        HIP_TRY(hipEventSynchronize(c->xfer.ev[k]));
        std::memcpy(static_cast<uint8_t*>(dst) + off, c->xfer.h[k], (size_t)std::min<uint64_t>(kXferChunk, bytes - off));
    }
    HIP_TRY(hipStreamSynchronize(c->stream));
    return BT_OK;
}

int bt_memset_d(bt_ctx* c, void* dst, int value, uint64_t bytes) {
    const bt::DeviceRestore keep_device;   // the caller's current device, restored on return
    if (!c) return set_error(BT_E_INVALID_ARGUMENT, "null context");
    HIP_TRY(hipSetDevice(c->device));
    if (int rc = after_cstream(c)) return rc;
    HIP_TRY(hipMemsetAsync(dst, value, bytes, c->stream));
    HIP_TRY(hipStreamSynchronize(c->stream));
    return BT_OK;
}

}  // extern "C"

namespace bt {

void release_xfer(bt_ctx* c) {
    for (int k = 0; k < 2; ++k) {
        if (c->xfer.h[k]) (void)hipHostFree(c->xfer.h[k]);
        if (c->xfer.ev[k]) (void)hipEventDestroy(c->xfer.ev[k]);
    }
    if (c->xfer.after) (void)hipEventDestroy(c->xfer.after);
}

}  // namespace bt
