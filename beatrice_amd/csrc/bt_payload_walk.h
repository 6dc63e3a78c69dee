// bt_payload_walk.h — the PAYLOAD filter's window gates and DFA walks, one copy for the kernels
// that decide BT_K_PAYLOAD slots on the GPU: bt_kernels.hip (the fused whole-frame form, which
// stages a lane's window into its LDS row itself) and bt_payload_resume.hip (the second pass over
// prefix batches, with its own cooperative staging). Everything here works on a window that
// already sits in the lane's LDS row and on the slot's blob in the block's dynamic LDS.
#pragma once

#include <hip/hip_runtime.h>

#include <type_traits>

#include "bt_dev_util.h"
#include "bt_device.h"

namespace bt {
namespace {

// applyPayloadFilter's window of a frame (eval_payload's gates): its start offset in the
// frame (po) and length L; L = 0 when the filter returns false without a search.
__device__ __forceinline__ uint32_t payload_window(uint32_t len, const uint32_t* w0, uint32_t& po) {
    po = 14u + (byte_of(w0, 14) & 15u) * 4u;
    if (!(len >= 34u && be16_of(w0, 12) == 0x0800u) || len <= po) return 0u;
    return min(len - po, 100u);
}

// The bit-parallel form (bt_regex_dfa.cpp "AST -> bit-parallel form"; blob layout there): an
// extended Shift-And over the position set D. The loop takes four window bytes per turn
// from the lane's LDS row (where eval_payload put the window) and runs until every lane of
// the wave has matched or passed its window (wave-uniform exit, no divergence inside); the
// row dwords two turns ahead and the table entries of the next four bytes are read before
// this turn's state steps, which are then only shift / or / and on registers. Entries are 1,
// 2, 4 or 8 bytes (the positions rounded up), so a small pattern's 256-entry table spans
// few distinct dwords per LDS bank (1-byte entries: at most 2 per bank, 4-byte: 8). A byte
// past the window (pos >= L) gets an empty mask: the partial matches of a SIMPLE pattern end
// there, and the others hold D ($ reads D at the window's end). Returns regex_search's answer
// over the L bytes.
template <typename E, bool SIMPLE>
__device__ __forceinline__ uint32_t bitpar_walk(const uint8_t* blob, const uint32_t* row, uint32_t staged_sh,
                                                uint32_t L, uint32_t rdw) {
    using T = typename std::conditional<sizeof(E) == 8, uint64_t, uint32_t>::type;
    const uint64_t* mk = reinterpret_cast<const uint64_t*>(blob + 16);
    const T Iall = (T)mk[0], F = (T)mk[5];
    const E* B = reinterpret_cast<const E*>(blob + 80);
    const uint32_t* r = row + (staged_sh >> 2);
    const uint32_t sh = staged_sh & 3u, rmax = rdw - 2u - (staged_sh >> 2);   // r[] stays inside the row
    // the general form's masks (SIMPLE: none of them is used)
    const T I0 = SIMPLE ? (T)0 : (T)mk[1], S = SIMPLE ? (T)0 : (T)mk[2], A = SIMPLE ? (T)0 : (T)mk[3];
    const T NF = SIMPLE ? ~(T)0 : (T)mk[4], Fe = SIMPLE ? (T)0 : (T)mk[6];
    const uint32_t R = SIMPLE ? 0u : blob[7];
    const bool anchored_all = !SIMPLE && (*reinterpret_cast<const uint32_t*>(blob + 8) & 4u) != 0u;
    T D = 0, hit = 0, inj = Iall | I0;
    auto step = [&](T b, uint32_t pos) {
        if constexpr (SIMPLE) {
            D = ((D << 1) | Iall) & (pos < L ? b : (T)0);
            hit |= D & F;
        } else {
            T n = (((D << 1) & NF) | inj | (D & S)) & b;
            inj = Iall;
            for (uint32_t k = 0; k < R; ++k) n |= (n << 1) & A;
            D = pos < L ? n : D;
            hit |= D & F;
        }
    };
    uint32_t t0 = r[0], t1 = r[1];
    uint32_t w = __builtin_amdgcn_alignbyte(t1, t0, sh);
    t0 = t1;
    t1 = r[2];
    T b0 = B[w & 0xFFu], b1 = B[(w >> 8) & 0xFFu], b2 = B[(w >> 16) & 0xFFu], b3 = B[w >> 24];
    for (uint32_t i = 0;; i += 4u) {
        // the next turn's bytes and entries, ahead of this turn's steps
        const uint32_t wn = __builtin_amdgcn_alignbyte(t1, t0, sh);
        t0 = t1;
        t1 = r[min((i >> 2) + 3u, rmax)];
        const T n0 = B[wn & 0xFFu], n1 = B[(wn >> 8) & 0xFFu], n2 = B[(wn >> 16) & 0xFFu], n3 = B[wn >> 24];
        step(b0, i);
        step(b1, i + 1u);
        step(b2, i + 2u);
        step(b3, i + 3u);
        if (__ballot(!hit && i + 4u < L && (SIMPLE || D || !anchored_all)) == 0ull) break;
        b0 = n0; b1 = n1; b2 = n2; b3 = n3;
    }
    return (hit || (D & Fe)) ? 1u : 0u;
}

// A SIMPLE pattern with a byte z that no class holds (the compiler records it): the window's
// bytes past its end are overwritten with z in the row, so every byte the wave's walk reads
// past a lane's window empties that lane's D and no position needs a bound check. The steps
// are then ((D << 1) | I) & B[c] and an OR of the states (H; a match ended where H & F is
// set): about 4 VALU per byte against 8 with the bound checks, which made the walk VALU-bound
// (C3 /GET|POST/ first: 123 k VALU per wave of the 129 k the walk added, SQ counters).
// Reading the window one LDS byte per byte instead (no alignbyte / extraction; the compiler
// merges the reads into unaligned 8-byte LDS reads and adds with byte selects) was slower
// filter-only, 0.708-0.718 against 0.663-0.670 ms (profiles/r06/payload/libs_bytes_wpe4.log).
template <typename E>
__device__ __forceinline__ uint32_t bitpar_fast(const uint8_t* blob, const uint32_t* row, uint32_t staged_sh,
                                                uint32_t L, uint32_t rdw) {
    const uint64_t* mk = reinterpret_cast<const uint64_t*>(blob + 16);
    const uint32_t Iall = (uint32_t)mk[0], F = (uint32_t)mk[5];
    const E* B = reinterpret_cast<const E*>(blob + 80);
    const uint32_t* r = row + (staged_sh >> 2);
    const uint32_t sh = staged_sh & 3u, rmax = rdw - 2u - (staged_sh >> 2);   // the row's last padded dword
    uint32_t t0 = r[0], t1 = r[1], t2 = r[2];
    uint32_t D = 0, H = 0;
    for (uint32_t i = 0;; i += 8u) {
        uint32_t b[8];
        const uint32_t w0 = __builtin_amdgcn_alignbyte(t1, t0, sh), w1 = __builtin_amdgcn_alignbyte(t2, t1, sh);
        t0 = t2;
        t1 = r[min((i >> 2) + 3u, rmax)];
        t2 = r[min((i >> 2) + 4u, rmax)];
#pragma unroll
        for (int k = 0; k < 4; ++k) {
            b[k] = B[(w0 >> (8 * k)) & 0xFFu];
            b[4 + k] = B[(w1 >> (8 * k)) & 0xFFu];
        }
        const uint32_t d0 = ((D << 1) | Iall) & b[0], d1 = ((d0 << 1) | Iall) & b[1];
        const uint32_t d2 = ((d1 << 1) | Iall) & b[2], d3 = ((d2 << 1) | Iall) & b[3];
        const uint32_t d4 = ((d3 << 1) | Iall) & b[4], d5 = ((d4 << 1) | Iall) & b[5];
        const uint32_t d6 = ((d5 << 1) | Iall) & b[6];
        D = ((d6 << 1) | Iall) & b[7];
        H |= d0 | d1 | d2 | d3 | d4 | d5 | d6 | D;
        if (__ballot(!(H & F) && i + 8u < L) == 0ull) break;
    }
    return (H & F) ? 1u : 0u;
}

// The wide form (bt_regex_dfa.cpp "The wide blob"; BT_DFA_EXTENDED): a DFA of 255..4,096 live
// states, so the state ids are 16 bits and the table is always indexed through the byte
// classes. Four window bytes per turn from two aligned dwords of the lane's row, as the byte
// DFA's loop below reads them (the same row reads, so inside the row for the same reason);
// their classes do not depend on the state and are read ahead of the chain, which is then one
// 16-bit LDS read per byte. A state q < K indexes next[q * C + c] inside the K * C table; a
// sink (K match, K + 1 none possible) is never used as an index.
__device__ __forceinline__ uint32_t wide_walk(const uint8_t* blob, const uint32_t* row, uint32_t staged_sh,
                                              uint32_t L) {
    const uint32_t C = *reinterpret_cast<const uint16_t*>(blob + 2);
    const uint32_t K = *reinterpret_cast<const uint16_t*>(blob + 4);
    uint32_t q = *reinterpret_cast<const uint16_t*>(blob + 6);
    const uint8_t* cls = blob + 12;
    const uint8_t* endacc = cls + 256;
    const uint16_t* next = reinterpret_cast<const uint16_t*>(endacc + ((K + 3u) & ~3u));
    const uint32_t dw = staged_sh >> 2, sh = staged_sh & 3u;
    for (uint32_t i = 0; i < L && q < K; i += 4u) {
        const uint32_t w = __builtin_amdgcn_alignbyte(row[dw + (i >> 2) + 1u], row[dw + (i >> 2)], sh);
        const uint32_t m = min(4u, L - i);
        const uint32_t c[4] = {cls[w & 0xFFu], cls[(w >> 8) & 0xFFu], cls[(w >> 16) & 0xFFu], cls[w >> 24]};
#pragma unroll
        for (uint32_t k = 0; k < 4u; ++k)
            if (k < m && q < K) q = next[q * C + c[k]];
    }
    return q >= K ? (q == K ? 1u : 0u) : (uint32_t)endacc[q];
}

// The walk of one PAYLOAD slot over a staged window (bt_payload_walk_body.inc has the contract).
__device__ __forceinline__ uint32_t payload_walk(const uint8_t* blob, uint32_t K, uint32_t* row, uint32_t staged_sh,
                                                 uint32_t L, uint32_t rdw) {
#include "bt_payload_walk_body.inc"
}

}  // namespace
}  // namespace bt
