// bt_context.cpp — a context's life (include/beatrice_gpu.h): the thread-local error slot,
// where the context's host work runs (usable CPUs, the device's NUMA node, the host pool),
// bt_create ... bt_destroy, the caller's streams and bt_synchronize. Nothing here throws
// across the ABI: failures return a beatrice::ErrorCode value and set a thread-local message.
#include <sched.h>
#include <sys/syscall.h>
#include <unistd.h>

#include <algorithm>
#include <cctype>
#include <cstdarg>
#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <functional>
#include <mutex>
#include <string>
#include <thread>

#include "bt_ctx.h"
#include "bt_hip_util.h"

using namespace bt;

namespace {

thread_local std::string g_err;

}  // namespace

namespace bt {

int set_error(int code, const char* fmt, ...) {
    char buf[512];
    va_list ap;
    va_start(ap, fmt);
    vsnprintf(buf, sizeof(buf), fmt, ap);
    va_end(ap);
    g_err = buf;
    return code;
}

// CPUs this process may run on: the affinity set, bounded by the cgroup v2 CPU quota (a GPU
// box's job sees every CPU of the machine in its affinity set but may use 16).
unsigned usable_cpus() {
    unsigned n = std::max(1u, std::thread::hardware_concurrency());
    cpu_set_t set;
    if (sched_getaffinity(0, sizeof(set), &set) == 0) n = std::max(1, CPU_COUNT(&set));
    if (FILE* f = fopen("/sys/fs/cgroup/cpu.max", "r")) {
        char q[32] = {0};
        unsigned long long period = 0;
        if (fscanf(f, "%31s %llu", q, &period) == 2 && strcmp(q, "max") != 0 && period) {
            const unsigned long long quota = strtoull(q, nullptr, 10) / period;
            if (quota >= 1 && quota < n) n = (unsigned)quota;
        }
        fclose(f);
    }
    return n;
}

// "0-3,8,10-11" (a sysfs cpulist) -> set; false if unreadable
bool parse_cpulist(const char* s, cpu_set_t* out) {
    CPU_ZERO(out);
    bool any = false;
    while (s && *s) {
        char* e = nullptr;
        const long a = strtol(s, &e, 10);
        if (e == s || a < 0) return false;
        long b = a;
        s = e;
        if (*s == '-') {
            b = strtol(s + 1, &e, 10);
            if (e == s + 1 || b < a) return false;
            s = e;
        }
        for (long i = a; i <= b && i < CPU_SETSIZE; ++i) CPU_SET((int)i, out);
        any = true;
        while (*s == ',' || *s == '\n' || *s == ' ') ++s;
    }
    return any;
}

// The host NUMA node closest to `device`: HIP's attribute, else the PCI function's sysfs
// numa_node (read from its bus id); -1 when the host has no NUMA information.
int device_numa_node(int device) {
    int node = -1;
    if (hipDeviceGetAttribute(&node, hipDeviceAttributeHostNumaId, device) != hipSuccess) {
        (void)hipGetLastError();
        node = -1;
    }
    if (node >= 0) return node;
    char bus[64] = {0};
    if (hipDeviceGetPCIBusId(bus, sizeof(bus), device) != hipSuccess) {
        (void)hipGetLastError();
        return -1;
    }
    for (char* p = bus; *p; ++p) *p = (char)tolower((unsigned char)*p);
    char path[160];
    snprintf(path, sizeof(path), "/sys/bus/pci/devices/%s/numa_node", bus);
    if (FILE* f = fopen(path, "r")) {
        if (fscanf(f, "%d", &node) != 1) node = -1;
        fclose(f);
    }
    return node;
}

// The CPUs of NUMA node `node` that this process may run on (its affinity set); false when
// there are none or the node's cpulist is unreadable.
bool node_cpus(int node, cpu_set_t* out) {
    if (node < 0) return false;
    char path[96];
    snprintf(path, sizeof(path), "/sys/devices/system/node/node%d/cpulist", node);
    char buf[4096] = {0};
    FILE* f = fopen(path, "r");
    if (!f) return false;
    const size_t got = fread(buf, 1, sizeof(buf) - 1, f);
    fclose(f);
    buf[got] = 0;
    cpu_set_t nodeset, aff;
    if (!parse_cpulist(buf, &nodeset)) return false;
    if (sched_getaffinity(0, sizeof(aff), &aff) != 0) return false;
    CPU_AND(out, &nodeset, &aff);
    return CPU_COUNT(out) > 0;
}

// Places a context's host work next to its device: the pool's workers (gather, drain, ring
// walk) run on the CPUs of the device's NUMA node. hipHostMalloc without
// hipHostMallocNumaUser allocates the pinned staging near the current device already (HIP
// lets the user's policy decide only with that flag, hip_runtime_api.h), and the staging
// is allocated after hipSetDevice (ensure_host). BT_NUMA_PIN=0 turns the pinning off (A/B).
void place_ctx(bt_ctx* c) {
    c->numa_node = device_numa_node(c->device);
    static const bool off = [] {
        const char* e = getenv("BT_NUMA_PIN");
        return e && atoi(e) == 0;
    }();
    c->pinned = !off && node_cpus(c->numa_node, &c->pin);
}

// The pool's size: opts.host_threads, else BT_HOST_THREADS, else the usable CPUs; at most 16.
// A group sets each member's opts.host_threads from its budget (bt_group.cpp). Round 3 capped
// the default at 8: with callers on all 16 of a GPU box's CPUs (T callers of one
// GpuPacketFilter, the plugin's onPacket threads) a 16-thread pool oversubscribed them
// (profiles/r03/surfaces/ab_pool_threads.jsonl). Now a chunk's gather takes at most 8 of the
// pool while other callers wait (pipeline_share), and a lone caller all of it.
unsigned pool_threads_of(const bt_ctx* c) {
    unsigned nt = c->opts.host_threads;
    if (!nt) {
        const char* e = getenv("BT_HOST_THREADS");
        nt = e && atoi(e) > 0 ? (unsigned)atoi(e) : usable_cpus();
    }
    return std::max(1u, std::min(nt, 16u));
}

HostPool& pool_of(bt_ctx* c) {
    std::call_once(c->pool_once, [c] {
        c->pool = std::make_unique<HostPool>(pool_threads_of(c), c->pinned ? &c->pin : nullptr);
    });
    return *c->pool;
}

unsigned pool_size(bt_ctx* ctx) { return pool_of(ctx).size(); }

void host_parallel(bt_ctx* ctx, const std::function<void(unsigned, unsigned)>& fn) {
    if (!ctx) {
        fn(0, 1);
        return;
    }
    HostPool& pool = pool_of(ctx);
    const unsigned T = pool.size();
    pool.run([&](unsigned w) { fn(w, T); });
}

}  // namespace bt

extern "C" {

int bt_abi_version(void) { return BT_ABI_VERSION; }

const char* bt_last_error(void) { return g_err.c_str(); }

int bt_device_count(int* out) {
    if (!out) return set_error(BT_E_INVALID_ARGUMENT, "null out");
    int n = 0;
    hipError_t e = hipGetDeviceCount(&n);
    if (e != hipSuccess) n = 0;
    *out = n;
    return BT_OK;
}

int bt_create(int device, const bt_opts* opts, bt_ctx** out) {
    const bt::DeviceRestore keep_device;   // the caller's current device, restored on return
    if (!out) return set_error(BT_E_INVALID_ARGUMENT, "null out");
    *out = nullptr;
    int n = 0;
    if (hipGetDeviceCount(&n) != hipSuccess || n == 0)
        return set_error(BT_E_INIT_FAILED, "no HIP device visible (the MI355X path needs a GPU)");
    if (device < 0 || device >= n) return set_error(BT_E_INVALID_ARGUMENT, "device %d out of range [0,%d)", device, n);
    auto* c = new bt_ctx();
    c->device = device;
    if (opts) c->opts = *opts;
    if (c->opts.flags & BT_OPT_SPIN_SYNC) {
        // host waits spin instead of sleeping: no wake-up latency on a loaded host.
        // Only possible before the process's first HIP context on this device.
        (void)hipSetDevice(device);
        c->spin_rc = (int)hipSetDeviceFlags(hipDeviceScheduleSpin);
        (void)hipGetLastError();   // a refusal (context already active) is reported, not sticky
    }
    if (hipSetDevice(device) != hipSuccess || hipStreamCreateWithFlags(&c->stream, hipStreamNonBlocking) != hipSuccess) {
        delete c;
        return set_error(BT_E_INIT_FAILED, "hipSetDevice/hipStreamCreate failed on device %d", device);
    }
    (void)hipGetDeviceFlags(&c->device_flags);
    (void)hipEventCreate(&c->timing.ev0);
    (void)hipEventCreate(&c->timing.ev1);
    // 0: one residency wave of whichever kernel variant a call launches (resident_grid)
    c->grid = c->opts.grid_waves ? (int)((c->opts.grid_waves + kWavesPerBlock - 1) / kWavesPerBlock) : 0;
    to_device_program(nullptr, 0, &c->prog);
    bt::publish_staged_window(c);
    place_ctx(c);
    *out = c;
    return BT_OK;
}

int bt_context_device(const bt_ctx* c, int* device, char* pci_bus_id, uint32_t cap) {
    if (!c) return set_error(BT_E_INVALID_ARGUMENT, "null context");
    if (device) *device = c->device;
    if (pci_bus_id) {
        if (cap < 16) return set_error(BT_E_INVALID_ARGUMENT, "pci_bus_id buffer of %u bytes (need >= 16)", cap);
        HIP_TRY(hipDeviceGetPCIBusId(pci_bus_id, (int)cap, c->device));
    }
    return BT_OK;
}

int bt_context_placement(bt_ctx* c, bt_placement* out) {
    if (!c || !out) return set_error(BT_E_INVALID_ARGUMENT, "null argument");
    *out = bt_placement{};
    out->numa_node = c->numa_node;
    out->pinned_cpus = c->pinned ? (uint32_t)CPU_COUNT(&c->pin) : 0u;
    out->pool_threads = pool_threads_of(c);
    out->staging_node = -1;
    std::lock_guard<std::mutex> lk(c->mu);
    if (c->host.ready && c->host.hs[0].h_in) {   // where the kernel put the pinned staging's first page
        void* page = c->host.hs[0].h_in;
        int status = -1;
        if (syscall(SYS_move_pages, 0, 1UL, &page, nullptr, &status, 0) == 0 && status >= 0) out->staging_node = status;
    }
    return BT_OK;
}

int bt_node_cpus(int node, int32_t* cpus, uint32_t cap, uint32_t* n) {
    if (!n || (cap && !cpus)) return set_error(BT_E_INVALID_ARGUMENT, "null argument");
    *n = 0;
    cpu_set_t s;
    if (!bt::node_cpus(node, &s)) return BT_OK;
    for (int i = 0; i < CPU_SETSIZE; ++i)
        if (CPU_ISSET(i, &s)) {
            if (*n < cap) cpus[*n] = i;
            ++*n;
        }
    return BT_OK;
}

uint32_t bt_usable_cpus(void) { return bt::usable_cpus(); }

void bt_destroy(bt_ctx* c) {
    const bt::DeviceRestore keep_device;   // the caller's current device, restored on return
    if (!c) return;
    (void)hipSetDevice(c->device);
    (void)hipDeviceSynchronize();
    for (const auto& r : c->host_regs)   // registrations the caller left: this context's references
        (void)bt::pin_release(reinterpret_cast<const void*>(r.first), r.second);
    c->host_regs.clear();
    release_host_pipe(c);
    if (c->pcap) { bt::pcap_stage_free(c->pcap); c->pcap = nullptr; }
    c->pool.reset();
    release_timing_graph(c);
    release_workspace(c);
    release_dfa_pools(c);
    release_timing(c);
    release_extract_stage(c);
    release_xfer(c);
    release_walk_stages(c);
    if (c->stream) (void)hipStreamDestroy(c->stream);
    delete c;
}

int bt_host_parallel(bt_ctx* c, void (*fn)(void*, uint32_t, uint32_t), void* user) {
    if (!c || !fn) return set_error(BT_E_INVALID_ARGUMENT, "null argument");
    bt::host_parallel(c, [&](unsigned w, unsigned T) { fn(user, w, T); });
    return BT_OK;
}

int bt_stream_create(bt_ctx* c, void** stream) {
    const bt::DeviceRestore keep_device;   // the caller's current device, restored on return
    if (!c || !stream) return set_error(BT_E_INVALID_ARGUMENT, "null argument");
    HIP_TRY(hipSetDevice(c->device));
    hipStream_t s = nullptr;
    HIP_TRY(hipStreamCreateWithFlags(&s, hipStreamNonBlocking));
    *stream = s;
    return BT_OK;
}

int bt_stream_synchronize(bt_ctx* c, void* stream) {
    const bt::DeviceRestore keep_device;   // the caller's current device, restored on return
    if (!c || !stream) return set_error(BT_E_INVALID_ARGUMENT, "null argument");
    HIP_TRY(hipSetDevice(c->device));
    HIP_TRY(hipStreamSynchronize(reinterpret_cast<hipStream_t>(stream)));
    return BT_OK;
}

int bt_stream_destroy(bt_ctx* c, void* stream) {
    const bt::DeviceRestore keep_device;   // the caller's current device, restored on return
    if (!c || !stream) return set_error(BT_E_INVALID_ARGUMENT, "null argument");
    HIP_TRY(hipSetDevice(c->device));
    HIP_TRY(hipStreamSynchronize(reinterpret_cast<hipStream_t>(stream)));
    {
        std::lock_guard<std::mutex> lk(c->mu);
        bt::forget_stream(c, reinterpret_cast<hipStream_t>(stream));
    }
    HIP_TRY(hipStreamDestroy(reinterpret_cast<hipStream_t>(stream)));
    return BT_OK;
}

int bt_synchronize(bt_ctx* c) {
    const bt::DeviceRestore keep_device;   // the caller's current device, restored on return
    if (!c) return set_error(BT_E_INVALID_ARGUMENT, "null context");
    HIP_TRY(hipSetDevice(c->device));
    HIP_TRY(hipStreamSynchronize(c->stream));
    if (c->ws.cstream) HIP_TRY(hipStreamSynchronize(c->ws.cstream));
    return BT_OK;
}

}  // extern "C"

namespace bt {

int ctx_device(const bt_ctx* c) { return c->device; }

bool ctx_stream_busy(bt_ctx* c) {
    const bt::DeviceRestore keep_device;
    if (hipSetDevice(c->device) != hipSuccess) return false;
    return hipStreamQuery(c->stream) == hipErrorNotReady;
}

}  // namespace bt
