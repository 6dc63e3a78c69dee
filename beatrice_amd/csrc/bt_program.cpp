// bt_program.cpp — the filter program of a context: bt_filter_compile's host half (slots,
// PAYLOAD DFA tables in one pool) and its device half (the double-buffered DFA pools, the
// slots as the kernels take them), and the events that keep a pool alive while launches read it.
#include <algorithm>
#include <cstring>
#include <mutex>
#include <vector>

#include "bt_ctx.h"
#include "bt_hip_util.h"

using namespace bt;

extern "C" {

int bt_filter_compile_host(const bt_filter_desc* f, uint32_t n, bt_filter_slot* out, uint32_t cap,
                           uint32_t* n_slots) {
    if ((!f && n) || !out || !n_slots) return set_error(BT_E_INVALID_ARGUMENT, "null argument");
    char err[256] = {0};
    int rc = compile_filters(f, n, out, cap, n_slots, err, sizeof(err));
    if (rc) return set_error(rc, "%s", err);
    return BT_OK;
}

}  // extern "C"

namespace bt {

// The host half of bt_filter_compile: the slots, and the PAYLOAD regexes the DFA compiler
// takes turned into BT_K_PAYLOAD slots with their tables in one pool (copied into each
// block's LDS, so capped at kDfaPoolMax). No device is touched: a group compiles once and
// installs the result on every member.
int compile_program(const bt_filter_desc* f, uint32_t n, uint32_t ctx_flags, CompiledProgram* out) {
    std::vector<bt_filter_slot> slots(BT_MAX_FILTERS);
    uint32_t m = 0;
    int rc = bt_filter_compile_host(f, n, slots.data(), BT_MAX_FILTERS, &m);
    if (rc) return rc;
    slots.resize(m);
    std::vector<uint8_t> pool;
    if (!(ctx_flags & BT_OPT_PAYLOAD_HOST)) {
        for (auto& s : slots) {
            const bt_filter_desc& d = f[s.source_index];
            if (s.kind != BT_K_HOST || d.type != BT_FILTER_PAYLOAD || !d.expression) continue;
            // the compiler's preferred form (bit-parallel where it fits, else the DFA with its
            // two-byte table); when that does not fit the pool, the DFA, then the DFA without
            // the optional table
            // the wider subset (\b \B, POSIX classes, wide DFAs) in every form tried, where asked for
            const uint32_t ext = (ctx_flags & BT_OPT_PAYLOAD_EXTENDED) ? BT_DFA_EXTENDED : 0u;
            const uint32_t base = ((ctx_flags & BT_OPT_PAYLOAD_DFA) ? BT_DFA_NO_BITPAR : 0u) | ext;
            const uint32_t forms[3] = {base, BT_DFA_NO_BITPAR | ext, BT_DFA_NO_BITPAR | BT_DFA_NO_PAIRS | ext};
            const size_t at = (pool.size() + 15) & ~(size_t)15;
            uint32_t size = 0, fl = 0;
            bool fits = false;
            for (uint32_t k = base ? 1u : 0u; k < 3 && !fits; ++k) {
                fl = forms[k];
                fits = bt_payload_dfa_compile_ex(d.expression, fl, nullptr, 0, &size) == BT_OK && at + size <= kDfaPoolMax;
            }
            if (!fits) continue;
            pool.resize(at + size);
            if (bt_payload_dfa_compile_ex(d.expression, fl, pool.data() + at, size, &size) != BT_OK) {
                pool.resize(at);
                continue;
            }
            s.kind = BT_K_PAYLOAD;
            s.a = (uint32_t)at;
            s.b = size;
        }
    }
    out->slots = std::move(slots);
    out->dfa_pool = std::move(pool);
    return BT_OK;
}

// The device half: the DFA pool into the buffer no queued launch reads (launches on any
// stream that still read it, with the old program, are waited for first), then the slots.
int install_program(bt_ctx* c, const CompiledProgram& p) {
    std::lock_guard<std::mutex> lk(c->mu);
    if (!p.dfa_pool.empty()) {
        HIP_TRY(hipSetDevice(c->device));
        const int k = c->dfa.cur ^ 1;
        if (!c->dfa.dev[k]) HIP_TRY(hipMalloc(&c->dfa.dev[k], kDfaPoolMax));
        for (auto& r : c->dfa.readers[k]) {   // every stream's last launch that read buffer k
            HIP_TRY(hipEventSynchronize(r.second));
            c->dfa.spare.push_back(r.second);
        }
        c->dfa.readers[k].clear();
        if (int rc = bt_memcpy_h2d(c, c->dfa.dev[k], p.dfa_pool.data(), p.dfa_pool.size())) return rc;   // synchronous
        c->dfa.cur = k;
    }
    // a cached BT_OPT_GRAPH timing graph holds the old program: drop it
    if (c->tgraph.exec) { (void)hipGraphExecDestroy(c->tgraph.exec); c->tgraph.exec = nullptr; }
    c->dfa_pool = p.dfa_pool;
    c->slots = p.slots;
    to_device_program(c->slots.data(), (uint32_t)c->slots.size(), &c->prog);
    publish_staged_window(c);
    return BT_OK;
}

// A launch on `st` reads the context's current DFA pool: the pool stays untouched until it has
// run (a recompile that reuses the buffer waits for every reader's event).
int dfa_read_on(bt_ctx* c, hipStream_t st) {
    auto& rd = c->dfa.readers[c->dfa.cur];
    auto it = std::find_if(rd.begin(), rd.end(), [st](const auto& x) { return x.first == st; });
    if (it == rd.end()) {
        hipEvent_t e = nullptr;
        if (!c->dfa.spare.empty()) { e = c->dfa.spare.back(); c->dfa.spare.pop_back(); }
        else HIP_TRY(hipEventCreateWithFlags(&e, hipEventDisableTiming));
        rd.emplace_back(st, e);
        it = rd.end() - 1;
    }
    HIP_TRY(hipEventRecord(it->second, st));
    return BT_OK;
}

void release_dfa_pools(bt_ctx* c) {
    for (int k = 0; k < 2; ++k) {
        if (c->dfa.dev[k]) (void)hipFree(c->dfa.dev[k]);
        for (auto& r : c->dfa.readers[k]) (void)hipEventDestroy(r.second);
    }
    for (auto e : c->dfa.spare) (void)hipEventDestroy(e);
}

}  // namespace bt

extern "C" {

int bt_filter_compile(bt_ctx* c, const bt_filter_desc* f, uint32_t n) {
    const bt::DeviceRestore keep_device;   // the caller's current device, restored on return
    if (!c) return set_error(BT_E_INVALID_ARGUMENT, "null context");
    CompiledProgram p;
    if (int rc = compile_program(f, n, c->opts.flags, &p)) return rc;
    return install_program(c, p);
}

int bt_filter_program(const bt_ctx* c, bt_filter_slot* out, uint32_t cap, uint32_t* n_slots) {
    if (!c || !n_slots) return set_error(BT_E_INVALID_ARGUMENT, "null argument");
    *n_slots = (uint32_t)c->slots.size();
    for (uint32_t i = 0; i < c->slots.size() && i < cap && out; ++i) out[i] = c->slots[i];
    return BT_OK;
}

int bt_filter_dfa_pool(const bt_ctx* c, void* out, uint32_t cap, uint32_t* bytes) {
    if (!c || !bytes || (cap && !out)) return set_error(BT_E_INVALID_ARGUMENT, "null argument");
    std::lock_guard<std::mutex> lk(const_cast<bt_ctx*>(c)->mu);
    *bytes = (uint32_t)c->dfa_pool.size();
    if (out && cap) std::memcpy(out, c->dfa_pool.data(), std::min<size_t>(cap, c->dfa_pool.size()));
    return BT_OK;
}

}  // extern "C"
