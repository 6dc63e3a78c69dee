// bt_payload_resume.hip — the second pass of the PAYLOAD filter for batches whose first pass could
// not read the payload (BT_BATCH_PREFIXES: the gathered modes of the ring stage).
//
// The first pass (bt_kernels.hip, filter_packet<2> with a.prefixes) leaves BT_DECIDE_HOST | s at
// every BT_K_PAYLOAD slot s a frame reaches. bt_payload_resume takes the decision bytes of such a
// batch and the WHOLE frames of the same packets (the registered ring through the ring
// descriptors) and finishes the chain on the GPU: slots s .. n-1 evaluated as filter_packet<2>
// evaluates them over whole frames, the decision byte rewritten in place. Slots before s passed in
// the first pass and read only bytes a prefix holds, so the bytes then equal what the fused
// whole-frame kernel writes for the same frames.
//
// Only some frames reach a PAYLOAD slot (none of the non-IPv4 ones when a protocol slot comes
// first), so the pass is built around a compacted work list instead of one lane per packet:
//   1. SCAN    — a wave reads the decision bytes of its 64-frame tiles (one coalesced byte load per
//                tile, the next tile's in flight) and ballot-compacts the indices of the work
//                items into its LDS queue.
//   2. HEADERS — once 64 items are queued (or the wave's tiles are done) lane i takes item i: its
//                descriptor, then the 16-B chunks holding frame bytes 12..37 and the rest of the
//                first 64-B window, loaded by 4 lanes per frame (16 frames per wave instruction)
//                into the frame's LDS row; FilterIn, the window's start and length stay in
//                registers.
//   3. WINDOW  — the <= 8 16-B chunks of the payload window, loaded by 8 lanes per frame (8 frames
//                per wave instruction) into the row from dword 0; chunks the header round left in
//                the row are moved down instead of read again. In the fused kernel these are <= 8
//                dependent loads per lane.
//   4. CHAIN   — wave-uniform slot loop from the lowest pending slot: PAYLOAD slots run the shared
//                walks (bt_payload_walk.h) over the staged row, the others eval_slot.
// bt_verdict_words rebuilds the verdict words from the final decision bytes (the resume kernel
// writes none: a word holds frames of other lanes' tiles, and no atomics touch mapped memory).
#include <algorithm>

#include "bt_dev_util.h"
#include "bt_device.h"
#include "bt_hip_launch.h"
#include "bt_payload_walk.h"
#include "bt_slot_eval.h"

namespace bt {

// BT_DEBUG_BOUNDS: this module's log of failed bounds checks (bt_bounds.h)
__device__ BoundsLog g_bounds_resume;

namespace {

constexpr uint32_t kQueue = 128;   // a wave's pending work items: < 64 left over + one tile's 64

__device__ __forceinline__ uint4 ld16_in(const ResumeArgs& a, uint64_t addr, bool ok) {
    // a chunk that would pass the read limit reads as zeros, as in the main kernel
    if (ok && addr + 16ull <= a.bytes && BT_IN(&g_bounds_resume, kSitePayload, addr + 15ull, a.bytes))
        return *reinterpret_cast<const uint4*>(a.base + addr);
    return make_uint4(0, 0, 0, 0);
}

// One batch of <= 64 work items, lane i = item i (idx = its frame; lanes >= cnt idle).
__device__ __forceinline__ void resume_items(const ResumeArgs& a, const DevProgram& prog, const uint8_t* dfa_lds,
                                             uint32_t* img, uint32_t lane, uint32_t idx, bool have) {
    constexpr uint32_t kRow = kRowDwords;
    uint32_t* row = img + lane * kRow;

    // ---- descriptor and first-pass slot of this lane's item ----
    uint64_t off = 0;
    uint32_t len = 0, slot0 = 0;
    if (have && BT_IN(&g_bounds_resume, kSiteDecide, idx, a.n)) {
        slot0 = BT_DECIDE_SLOT(a.decide[idx]);
        frame_at(a, idx, off, len);
    }
    const uint32_t s = (uint32_t)off & 15u;
    const uint32_t off_lo = (uint32_t)off, off_hi = (uint32_t)(off >> 32);

    // ---- HEADERS: chunks 0..3 of the frame's 16-B-aligned window, 4 lanes per frame ----
    {
        uint4 v[4];
        const uint32_t c = lane & 3u;
#pragma unroll
        for (uint32_t j = 0; j < 4; ++j) {
            const uint32_t q = j * 16u + (lane >> 2);
            const uint64_t qo = ((uint64_t)(uint32_t)__shfl((int)off_hi, (int)q) << 32) |
                                (uint32_t)__shfl((int)off_lo, (int)q);
            const uint32_t ql = (uint32_t)__shfl((int)len, (int)q);
            const uint32_t sq = (uint32_t)qo & 15u;
            // the frame's bytes from 12 on (nothing here reads the MAC addresses), inside the frame
            const bool want = (16u * c < sq + ql) & (16u * c + 16u > sq + 12u);
            v[j] = ld16_in(a, (qo & ~15ull) + 16u * c, want);
        }
#pragma unroll
        for (uint32_t j = 0; j < 4; ++j) {
            uint32_t* dst = img + (j * 16u + (lane >> 2)) * kRow + c * 4u;
            dst[0] = v[j].x; dst[1] = v[j].y; dst[2] = v[j].z; dst[3] = v[j].w;
        }
    }
    wave_lds_sync();

    // the frame's first 40 bytes from the row (bytes 12..37 and 14 are what is read of them)
    uint32_t w0[10];
    window<10>(row, s, w0);
    const FilterIn x = filter_in([&w0](uint32_t i) { return byte_of(w0, (int)i); }, len);
    uint32_t po;
    const uint32_t L = payload_window(len, w0, po);

    // ---- WINDOW: the row becomes the window from its 16-B-aligned start ----
    const uint64_t start = off + po;
    const uint64_t al = start & ~15ull;
    const uint32_t staged_sh = (uint32_t)(start & 15ull);
    const uint32_t nch = L ? (staged_sh + L + 15u) >> 4 : 0u;   // <= 8: 15 + 100 bytes
    // window chunk k = header chunk d + k: those the header round read move down the row
    const uint32_t d = (uint32_t)((al - (off & ~15ull)) >> 4);
    const uint32_t kept = d < 4u ? min(4u - d, nch) : 0u;
    for (uint32_t k = 0; k < kept; ++k) {   // ascending, source above destination
        uint32_t* dst = row + 4u * k;
        const uint32_t* src = row + 4u * (k + d);
        const uint32_t t0 = src[0], t1 = src[1], t2 = src[2], t3 = src[3];
        dst[0] = t0; dst[1] = t1; dst[2] = t2; dst[3] = t3;
    }
    wave_lds_sync();
    {
        const uint32_t al_lo = (uint32_t)al, al_hi = (uint32_t)(al >> 32), nk = nch | (kept << 8);
        const uint32_t k = lane & 7u;
        if (__ballot(nch > kept) != 0ull) {
            uint4 v[8];
            uint32_t wr = 0;
#pragma unroll
            for (uint32_t j = 0; j < 8; ++j) {
                const uint32_t q = j * 8u + (lane >> 3);
                const uint64_t qal = ((uint64_t)(uint32_t)__shfl((int)al_hi, (int)q) << 32) |
                                     (uint32_t)__shfl((int)al_lo, (int)q);
                const uint32_t qnk = (uint32_t)__shfl((int)nk, (int)q);
                const bool want = (k < (qnk & 0xFFu)) & (k >= (qnk >> 8));
                v[j] = ld16_in(a, qal + 16u * k, want);
                wr |= want ? 1u << j : 0u;
            }
#pragma unroll
            for (uint32_t j = 0; j < 8; ++j)
                if (wr & (1u << j)) {
                    uint32_t* dst = img + (j * 8u + (lane >> 3)) * kRow + k * 4u;
                    dst[0] = v[j].x; dst[1] = v[j].y; dst[2] = v[j].z; dst[3] = v[j].w;
                }
        }
    }
    wave_lds_sync();

    // ---- CHAIN: slots slot0 .. n-1 as filter_packet<2> evaluates them over whole frames ----
    uint32_t code = BT_DECIDE_PASS, slot = prog.n ? prog.n - 1u : 0u;
    bool open = have;
    uint32_t f = have ? slot0 : BT_MAX_FILTERS;
    for (int o = 32; o > 0; o >>= 1) f = min(f, (uint32_t)__shfl_xor((int)f, o));
    f = __builtin_amdgcn_readfirstlane(f);
    for (; f < prog.n; ++f) {
        if (__ballot(open) == 0ull) break;
        const bool act = open && f >= slot0;
        uint32_t r;
        if (prog.f[f].kind == BT_K_PAYLOAD) {   // wave-uniform
            r = 0u;
            if (act && L) {
                const uint8_t* blob = dfa_lds + prog.f[f].a;
                const uint32_t K = *reinterpret_cast<const uint16_t*>(blob);
                if (K == 0xFFFFu && blob[6] != 1u) r = blob[6] == 2u ? 1u : 0u;   // bit-parallel: always / never
                else r = payload_walk(blob, K, row, staged_sh, L, kRow);
            }
        } else {
            r = eval_slot(prog.f[f].kind, prog.f[f].a, prog.f[f].b, x);
        }
        if (act && r != 1u) {
            code = r == 0u ? BT_DECIDE_REJECT : r == 2u ? BT_DECIDE_THROW : BT_DECIDE_HOST;
            slot = f;
            open = false;
        }
    }
    if (have && BT_IN(&g_bounds_resume, kSiteDecide, idx, a.n)) a.decide[idx] = (uint8_t)((code << 6) | slot);
    wave_lds_sync();   // the next batch overwrites this wave's rows
}

__global__ __launch_bounds__(kBlock) void bt_payload_resume(ResumeArgs a, DevProgram prog) {
    __shared__ __attribute__((aligned(16))) uint32_t lds_all[kWavesPerBlock * (kWave * kRowDwords + kQueue) + 32];
    extern __shared__ uint4 dyn_lds[];   // PAYLOAD DFA pool (a.dfa_bytes)
    const uint32_t lane = threadIdx.x & 63u;
    const uint32_t wid = __builtin_amdgcn_readfirstlane(threadIdx.x >> 6);   // provably wave-uniform
    uint32_t* img = lds_all + wid * (kWave * kRowDwords + kQueue);
    uint32_t* queue = img + kWave * kRowDwords;
    copy_dfa_pool(dyn_lds, a.dfa, a.dfa_bytes, &g_bounds_resume);
    const uint8_t* dfa_lds = reinterpret_cast<const uint8_t*>(dyn_lds);

    // the program's PAYLOAD slots as a mask (BT_MAX_FILTERS = 64 slots)
    uint64_t pmask = 0;
    for (uint32_t f = 0; f < prog.n && f < BT_MAX_FILTERS; ++f)
        if (prog.f[f].kind == BT_K_PAYLOAD) pmask |= 1ull << f;

    const uint32_t total_waves = gridDim.x * kWavesPerBlock;
    const uint32_t gw = blockIdx.x * kWavesPerBlock + wid;
    const uint64_t below = (1ull << lane) - 1ull;
    auto load_byte = [&](uint32_t t) -> uint32_t {
        const uint64_t i = (uint64_t)t * 64u + lane;
        return t < a.ntiles && i < a.n ? (uint32_t)a.decide[i] : 0u;   // 0 = PASS | 0: never a work item
    };
    uint32_t qn = 0;   // wave-uniform: queued items
    uint32_t nxt = load_byte(gw);
    for (uint32_t t = gw; t < a.ntiles; t += total_waves) {
        const uint32_t b = nxt;
        nxt = load_byte(t + total_waves);
        const bool work = BT_DECIDE_CODE(b) == BT_DECIDE_HOST && ((pmask >> BT_DECIDE_SLOT(b)) & 1ull);
        const uint64_t m = __ballot(work);
        if (work) queue[qn + (uint32_t)__popcll(m & below)] = t * 64u + lane;   // qn < 64: inside kQueue
        qn += (uint32_t)__popcll(m);
        if (qn >= 64u) {
            wave_lds_sync();
            const uint32_t idx = queue[lane];
            const uint32_t rest = qn - 64u;   // < 64
            const uint32_t tail = lane < rest ? queue[64u + lane] : 0u;
            wave_lds_sync();
            if (lane < rest) queue[lane] = tail;
            qn = rest;
            resume_items(a, prog, dfa_lds, img, lane, idx, true);
        }
    }
    if (qn) {   // the wave's last, partial batch
        wave_lds_sync();
        const bool have = lane < qn;
        const uint32_t idx = have ? queue[lane] : 0u;
        resume_items(a, prog, dfa_lds, img, lane, idx, have);
    }
}

// One wave per verdict word: bit i of word j = frame 64 j + i passed (code PASS).
__global__ __launch_bounds__(kBlock) void bt_verdict_words(const uint8_t* decide, uint32_t n, uint64_t* verdict) {
    const uint32_t lane = threadIdx.x & 63u;
    const uint32_t ntiles = (n + 63u) / 64u;
    const uint32_t t = blockIdx.x * kWavesPerBlock + (threadIdx.x >> 6);
    if (t >= ntiles) return;   // wave-uniform
    const uint64_t i = (uint64_t)t * 64u + lane;
    const bool pass = i < n && BT_DECIDE_CODE(decide[i]) == BT_DECIDE_PASS;
    const uint64_t word = __ballot(pass);
    if (lane == 0 && BT_IN(&g_bounds_resume, kSiteVerdict, t, ntiles)) verdict[t] = word;
}


}  // namespace

int launch_payload_resume(const ResumeArgs& a, const DevProgram& prog, void* stream, void* timing_start,
                          void* timing_stop) {
    hipStream_t st = reinterpret_cast<hipStream_t>(stream);
    hipEvent_t e0 = reinterpret_cast<hipEvent_t>(timing_start), e1 = reinterpret_cast<hipEvent_t>(timing_stop);
    if (!a.n || !a.dfa_bytes) return BT_OK;
    const uint32_t dyn = (a.dfa_bytes + 15u) & ~15u;
    // A wave scans at least kScanTiles tiles where the batch has them, so that its queue fills
    // whole 64-item batches even when few frames reach the slot; at most one residency wave of
    // blocks (the scan loop is persistent).
    constexpr uint32_t kScanTiles = 8;
    const uint32_t needed = (a.ntiles + kWavesPerBlock * kScanTiles - 1u) / (kWavesPerBlock * kScanTiles);
    const int g = (int)std::max(1u, std::min(needed, (uint32_t)resident_grid<bt_payload_resume>(dyn)));
    launch(bt_payload_resume, dim3(g), dim3(kBlock), dyn, st, e0, e1, a, prog);
    return hipGetLastError() == hipSuccess ? BT_OK : BT_E_INTERNAL;
}

int launch_verdict_words(const uint8_t* decide, uint32_t n, uint64_t* verdict, void* stream) {
    if (!n) return BT_OK;
    const uint32_t ntiles = (n + 63u) / 64u;
    hipLaunchKernelGGL(bt_verdict_words, dim3((ntiles + kWavesPerBlock - 1u) / kWavesPerBlock), dim3(kBlock), 0,
                       reinterpret_cast<hipStream_t>(stream), decide, n, verdict);
    return hipGetLastError() == hipSuccess ? BT_OK : BT_E_INTERNAL;
}

uint32_t bounds_take_resume(void* stream, BoundsLog* first) { return bounds_take(g_bounds_resume, stream, first); }

}  // namespace bt
