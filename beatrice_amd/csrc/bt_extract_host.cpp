// bt_extract_host.cpp — the user-protocol extractor's host side: a bt_field_def table as the
// kernel takes it, the device-resident call, the pure-host decode, and bt_extract over host
// lists (gather on the host pool, one launch per chunk, drain).
#include <algorithm>
#include <cstring>
#include <mutex>
#include <vector>

#include "bt_ctx.h"
#include "bt_hip_util.h"

using namespace bt;

namespace bt {

// A bt_field_def table as the kernel takes it (ExTable), with the span and the checks the
// C-ABI promises. span > 65535 can never parse a frame (lengths are 16-bit): *never = true.
int build_table(const bt_field_def* f, uint32_t n, ExTable* t, uint64_t* span_out, bool* never) {
    if (n && !f) return set_error(BT_E_INVALID_ARGUMENT, "null field table");
    if (n > BT_FIELD_MAX) return set_error(BT_E_INVALID_ARGUMENT, "%u fields (max %u)", n, BT_FIELD_MAX);
    // getTotalLength (src/parser/FieldDefinition.cpp:31-46): the end of the field that ends
    // last (offset + length in size_t arithmetic)
    uint64_t mo = 0, ml = 0;
    for (uint32_t k = 0; k < n; ++k) {
        if (f[k].type > BT_FT_CUSTOM) return set_error(BT_E_INVALID_ARGUMENT, "field %u: unknown type %u", k, f[k].type);
        if (f[k].type == BT_FT_BOOLEAN && f[k].length == 0)
            return set_error(BT_E_INVALID_ARGUMENT, "field %u: BOOLEAN of length 0 (the reference reads fieldData[0] "
                             "of an empty vector)", k);
        if (f[k].offset + f[k].length < f[k].offset)
            return set_error(BT_E_INVALID_ARGUMENT, "field %u: offset + length overflows", k);
        if (f[k].offset + f[k].length > mo + ml) { mo = f[k].offset; ml = f[k].length; }
    }
    const uint64_t span = n ? mo + ml : 0;
    if (span_out) *span_out = span;
    *never = span > 0xFFFFu;
    std::memset(t, 0, sizeof(*t));
    t->n = n;
    t->span = *never ? 0u : (uint32_t)span;
    t->window = std::min<uint32_t>(t->span, kExWindow);
    for (uint32_t k = 0; k < n && !*never; ++k) {
        t->f[k].offset = (uint32_t)f[k].offset;
        t->f[k].length = (uint32_t)f[k].length;
        t->f[k].ctl = f[k].type | ((f[k].endianness & 0xFFu) << 8);
    }
    return BT_OK;
}

int run_extract(bt_ctx* c, const bt_batch* b, const ExTable& t, bool never, const bt_extract_out* o, hipStream_t st,
                hipEvent_t e0, hipEvent_t e1) {
    if (!b || !o) return set_error(BT_E_INVALID_ARGUMENT, "null batch/outputs");
    ExArgs a{};
    char why[128];
    const FrameCheck bad = frame_src(b, &a, why, sizeof(why));   // as run_device: the size only for a batch with frames
    if (bad && bad != kFramesSize) return set_error(BT_E_INVALID_ARGUMENT, "%s", why);
    if (o->values && o->n_cap < b->n) return set_error(BT_E_INVALID_ARGUMENT, "values n_cap %u < n %u", o->n_cap, b->n);
    if (b->flags & BT_BATCH_LEAN)
        return set_error(BT_E_INVALID_ARGUMENT, "a BT_BATCH_LEAN batch holds frame bytes 12..43 only: no user-table extraction");
    if (!b->n) return BT_OK;
    if (bad) return set_error(BT_E_INVALID_ARGUMENT, "%s", why);
    if (never) {   // no frame reaches the span: every packet PACKET_TOO_SHORT, no field
        if (o->status) HIP_TRY(hipMemsetAsync(o->status, 9, b->n, st));
        if (o->values) for (uint32_t k = 0; k < t.n; ++k)
            HIP_TRY(hipMemsetAsync(o->values + (size_t)k * o->n_cap, 0, (size_t)b->n * 8, st));
        return BT_OK;
    }
    a.bytes = read_limit(a.base, a.bytes);
    a.status = o->status;
    a.values = o->values;
    a.image = o->image;
    a.n_cap = o->n_cap;
    const int rc = launch_extract(a, t, st, e0, e1);
    if (rc) return set_error(rc, "extract kernel launch failed: %s", hipGetErrorString(hipGetLastError()));
    return check_bounds(st, nullptr, "extract");
}

void release_extract_stage(bt_ctx* c) {
    if (c->ex.h) (void)hipHostFree(c->ex.h);
    if (c->ex.d) (void)hipFree(c->ex.d);
}

}  // namespace bt

extern "C" {

int bt_proto_span(const bt_field_def* fields, uint32_t n_fields, uint64_t* span) {
    if (!span) return set_error(BT_E_INVALID_ARGUMENT, "null span");
    ExTable t;
    bool never = false;
    return build_table(fields, n_fields, &t, span, &never);
}

int bt_extract_device(bt_ctx* c, const bt_batch* b, const bt_field_def* fields, uint32_t n_fields,
                      const bt_extract_out* out, void* stream) {
    const bt::DeviceRestore keep_device;   // the caller's current device, restored on return
    if (!c) return set_error(BT_E_INVALID_ARGUMENT, "null context");
    ExTable t;
    bool never = false;
    int rc = build_table(fields, n_fields, &t, nullptr, &never);
    if (rc) return rc;
    std::lock_guard<std::mutex> lk(c->mu);
    HIP_TRY(hipSetDevice(c->device));
    return run_extract(c, b, t, never, out, stream ? reinterpret_cast<hipStream_t>(stream) : c->stream);
}

// extractValue<T> (src/parser/ProtocolParser.cpp:385-433) on the host for one field of a
// frame at least the table's span long: bt_extract.hip's decode_field byte loop (its one-window
// fast path computes the same bits for fields no longer than their type).
static uint64_t decode_field_host(const ExField& f, const uint8_t* frame) {
    const uint32_t type = f.ctl & 0xFFu;
    const bool le = ((f.ctl >> 8) & 0xFFu) == BT_ENDIAN_LITTLE;
    const uint32_t o = f.offset, L = f.length;
    switch (type) {
    case BT_FT_BOOLEAN: return frame[o] != 0 ? 1u : 0u;
    case BT_FT_BYTES: case BT_FT_STRING: case BT_FT_MAC: case BT_FT_IPV4: case BT_FT_IPV6: case BT_FT_CUSTOM:
        return 0;
    default: break;
    }
    const uint32_t w = (type == BT_FT_UINT8 || type == BT_FT_INT8) ? 8u
                     : (type == BT_FT_UINT16 || type == BT_FT_INT16) ? 16u
                     : (type == BT_FT_UINT32 || type == BT_FT_INT32 || type == BT_FT_FLOAT32) ? 32u : 64u;
    if ((type == BT_FT_FLOAT32 || type == BT_FT_FLOAT64) && L * 8u != w) return 0;
    const uint32_t m = w == 64u ? 63u : 31u;
    uint64_t v = 0;
    for (uint32_t i = 0; i < L; ++i) {
        const uint32_t sh = (8u * i) & m;
        if (sh >= w) continue;
        v |= (uint64_t)frame[o + (le ? i : L - 1u - i)] << sh;
    }
    return w == 64u ? v : (v & ((1ull << w) - 1ull));
}

int bt_extract_host(const uint8_t* const* frames, const uint32_t* lens, uint32_t n, const bt_field_def* fields,
                    uint32_t n_fields, uint8_t* status, uint64_t* values, uint8_t* image) {
    if (n && (!frames || !lens)) return set_error(BT_E_INVALID_ARGUMENT, "null frame pointers/lengths");
    ExTable t;
    bool never = false;
    uint64_t span64 = 0;
    int rc = build_table(fields, n_fields, &t, &span64, &never);
    if (rc) return rc;
    for (uint32_t i = 0; i < n; ++i) {
        const bool ok = !never && lens[i] >= t.span;
        if (status) status[i] = ok ? 0u : 9u;   // ParseStatus SUCCESS / PACKET_TOO_SHORT
        if (values)
            for (uint32_t k = 0; k < n_fields; ++k) values[(size_t)k * n + i] = ok ? decode_field_host(t.f[k], frames[i]) : 0u;
        if (image && !never && t.span) {
            uint8_t* out = image + (size_t)i * t.span;
            if (ok) std::memcpy(out, frames[i], t.span);
            else std::memset(out, 0, t.span);
        }
    }
    return BT_OK;
}

int bt_extract(bt_ctx* c, const uint8_t* const* frames, const uint32_t* lens, uint32_t n, const bt_field_def* fields,
               uint32_t n_fields, uint8_t* status, uint64_t* values, uint8_t* image) {
    const bt::DeviceRestore keep_device;   // the caller's current device, restored on return
    if (!c) return set_error(BT_E_INVALID_ARGUMENT, "null context");
    if (n && (!frames || !lens)) return set_error(BT_E_INVALID_ARGUMENT, "null frame pointers/lengths");
    ExTable t;
    bool never = false;
    uint64_t span64 = 0;
    int rc = build_table(fields, n_fields, &t, &span64, &never);
    if (rc) return rc;
    if (!n) return BT_OK;
    if (never) {
        if (status) std::memset(status, 9, n);
        if (values) std::memset(values, 0, (size_t)n_fields * n * 8);
        return BT_OK;   // image: n x span bytes the caller could not have allocated anyway
    }
    const uint32_t span = t.span;
    const WaitFor lk(c);
    HIP_TRY(hipSetDevice(c->device));
    (void)pool_of(c);
    // chunks of at most 1M packets: [prefixes | descriptors] in, [status | values | image] out.
    // The gather and the drain run on the context's host threads (a serial gather, length
    // check and drain were most of a 1M-packet call). Tables up to 64 B (no frame is shorter
    // than an Ethernet minimum's worth of slot) give every frame one slot of round_up(span, 16)
    // bytes, so the gather needs no prefix pass; wider ones pack each frame's
    // round_up(min(len, span), 16) bytes after a per-worker count and scan.
    const uint32_t chunk = 1u << 20;
    const size_t slot = ((size_t)span + 15u) & ~(size_t)15u;
    const bool fixed = slot <= 64;
    for (uint32_t lo = 0; lo < n; lo += chunk) {
        const uint32_t m = std::min(chunk, n - lo);
        const unsigned T = pipeline_share(c);
        std::vector<uint64_t> part(T + 1, 0);   // packed: each worker's first staging byte
        if (!fixed) {
            pipeline_run(c, m, T, [&](unsigned w) {
                const uint32_t a = (uint32_t)((uint64_t)m * w / T), e = (uint32_t)((uint64_t)m * (w + 1) / T);
                uint64_t sum = 0;
                for (uint32_t i = a; i < e; ++i) sum += (std::min(lens[lo + i], span) + 15u) & ~15u;
                part[w + 1] = sum;
            });
            for (unsigned w = 0; w < T; ++w) part[w + 1] += part[w];
        }
        const size_t pre = (fixed ? (size_t)m * slot : part[T]) + 16, dsc = (size_t)m * 8;
        const size_t st_b = ((size_t)m + 15) & ~(size_t)15, val_b = (size_t)n_fields * m * 8, img_b = (size_t)m * span;
        const size_t in_b = pre + dsc, out_b = st_b + val_b + img_b;
        const size_t need = in_b + out_b + 64;
        if (need > c->ex.cap) {
            if (c->ex.h) (void)hipHostFree(c->ex.h);
            if (c->ex.d) (void)hipFree(c->ex.d);
            c->ex.h = nullptr;
            c->ex.d = nullptr;
            c->ex.cap = 0;
            const size_t cap = std::max(need, (size_t)1 << 20);
            HIP_TRY(hipHostMalloc(&c->ex.h, cap, hipHostMallocDefault));
            HIP_TRY(hipMalloc(&c->ex.d, cap));
            c->ex.cap = cap;
        }
        uint8_t* h = c->ex.h;
        uint64_t* d = reinterpret_cast<uint64_t*>(h + pre);
        std::vector<uint32_t> bad(T, UINT32_MAX);   // per worker: first frame longer than 65535 B
        pipeline_run(c, m, T, [&](unsigned w) {
            const uint32_t a = (uint32_t)((uint64_t)m * w / T), e = (uint32_t)((uint64_t)m * (w + 1) / T);
            uint64_t p = fixed ? (uint64_t)a * slot : part[w];
            for (uint32_t i = a; i < e; ++i) {   // only [0, span) of a frame is ever read
                const uint32_t len = lens[lo + i];
                const uint32_t k = std::min(len, span);
                if (len > 0xFFFFu) bad[w] = std::min(bad[w], lo + i);
                else if (k) std::memcpy(h + p, frames[lo + i], k);
                d[i] = BT_DESC(p, len & 0xFFFFu);
                p += fixed ? slot : (k + 15u) & ~15u;
            }
        });
        const uint32_t first_bad = *std::min_element(bad.begin(), bad.end());
        if (first_bad != UINT32_MAX) return set_error(BT_E_INVALID_ARGUMENT, "frame %u longer than 65535 bytes", first_bad);
        HIP_TRY(hipMemcpyAsync(c->ex.d, h, in_b, hipMemcpyHostToDevice, c->stream));
        bt_batch b{};
        b.base = c->ex.d;
        b.desc = c->ex.d + pre;
        b.n = m;
        b.bytes = pre;
        uint8_t* dout = c->ex.d + ((in_b + 15) & ~(size_t)15);
        uint8_t* hout = h + ((in_b + 15) & ~(size_t)15);
        bt_extract_out o{};
        o.status = dout;
        o.values = n_fields ? reinterpret_cast<uint64_t*>(dout + st_b) : nullptr;
        o.image = span ? dout + st_b + val_b : nullptr;
        o.n_cap = m;
        rc = run_extract(c, &b, t, false, &o, c->stream);
        if (rc) return rc;
        HIP_TRY(hipMemcpyAsync(hout, dout, out_b, hipMemcpyDeviceToHost, c->stream));
        HIP_TRY(hipStreamSynchronize(c->stream));
        pipeline_run(c, m, T, [&](unsigned w) {
            const uint32_t a = (uint32_t)((uint64_t)m * w / T), e = (uint32_t)((uint64_t)m * (w + 1) / T);
            if (a >= e) return;
            if (status) std::memcpy(status + lo + a, hout + a, e - a);
            for (uint32_t k = 0; values && k < n_fields; ++k)
                std::memcpy(values + (size_t)k * n + lo + a, hout + st_b + ((size_t)k * m + a) * 8, (size_t)(e - a) * 8);
            if (image && span) std::memcpy(image + ((size_t)lo + a) * span, hout + st_b + val_b + (size_t)a * span,
                                           (size_t)(e - a) * span);
        });
    }
    return BT_OK;
}

}  // extern "C"
