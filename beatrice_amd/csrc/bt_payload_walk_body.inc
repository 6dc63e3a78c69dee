// bt_payload_walk_body.inc — the walk of one PAYLOAD slot over a staged window, as statements: the
// form dispatch (bit-parallel / wide / byte DFA) and the byte-DFA loops. Included as the body of
// payload_walk (bt_payload_walk.h, which bt_payload_resume.hip calls) and as the tail of
// bt_kernels.hip's eval_payload, where a call (even an inlined one) changed the main kernels'
// register allocation and cost c3_payload 0.5 %; the text is the same in both, so the two kernels
// cannot drift apart. Expects in scope: const uint8_t* blob (the slot's table in LDS, not an always
// / never blob), uint32_t K (its first 16-bit word), uint32_t* row (the lane's LDS row), uint32_t
// staged_sh (payload byte i sits at row byte staged_sh + i), L (> 0 window bytes), rdw (the row's
// dwords). Every path returns regex_search's answer over the window.
    if (K == 0xFFFFu) {   // the bit-parallel form (wave-uniform: the slot's blob)
        const uint32_t W = *reinterpret_cast<const uint16_t*>(blob + 2);
        const bool simple = *reinterpret_cast<const uint32_t*>(blob + 8) == 0u && blob[7] == 0u;
        const uint32_t z = blob[12];   // 1 + a byte no class holds, 0: none
        if (simple && z && W <= 32u) {
            // the row past the window: z in every byte (the dword the window ends in keeps
            // the window's bytes below the end)
            const uint32_t end = staged_sh + L, q = end >> 2, zz = (z - 1u) * 0x01010101u;
            const uint32_t keep = (end & 3u) ? (1u << (8u * (end & 3u))) - 1u : 0u;
            row[q] = (row[q] & keep) | (zz & ~keep);
            for (uint32_t k = q + 1u; k < rdw; ++k) row[k] = zz;
            return W == 8 ? bitpar_fast<uint8_t>(blob, row, staged_sh, L, rdw)
                 : W == 16 ? bitpar_fast<uint16_t>(blob, row, staged_sh, L, rdw)
                           : bitpar_fast<uint32_t>(blob, row, staged_sh, L, rdw);
        }
        switch (W) {
        case 8: return simple ? bitpar_walk<uint8_t, true>(blob, row, staged_sh, L, rdw)
                              : bitpar_walk<uint8_t, false>(blob, row, staged_sh, L, rdw);
        case 16: return simple ? bitpar_walk<uint16_t, true>(blob, row, staged_sh, L, rdw)
                               : bitpar_walk<uint16_t, false>(blob, row, staged_sh, L, rdw);
        case 32: return simple ? bitpar_walk<uint32_t, true>(blob, row, staged_sh, L, rdw)
                               : bitpar_walk<uint32_t, false>(blob, row, staged_sh, L, rdw);
        default: return bitpar_walk<uint64_t, false>(blob, row, staged_sh, L, rdw);
        }
    }
    if (K == 0xFFFEu) return wide_walk(blob, row, staged_sh, L);   // the wide form (wave-uniform too)
    const uint32_t C = *reinterpret_cast<const uint16_t*>(blob + 2);
    uint32_t q = blob[4];
    if (q >= K) return q == K ? 1u : 0u;
    const uint8_t* endacc = blob + 8;
    const uint8_t* cls = endacc + ((K + 3u) & ~3u);
    const uint8_t* next = C == 256u ? cls : cls + 256;
    const uint32_t dw = staged_sh >> 2, sh8 = (staged_sh & 3u) * 8u;
    uint32_t i = 0;
    if (blob[6]) {
        // Two-byte table: the classes of four bytes are independent of q and issued
        // first, then two dependent reads cover them (half the chain of one per byte).
        const uint32_t P = blob[7];
        const uint8_t* clsp = blob + ((((uint32_t)(next - blob) + K * C) + 3u) & ~3u);
        const uint8_t* pair = clsp + 256;
        for (; i + 4u <= L; i += 4u) {
            const uint32_t lo = row[dw + (i >> 2)], hi = row[dw + (i >> 2) + 1u];
            const uint32_t w = sh8 ? (uint32_t)((((uint64_t)hi << 32) | lo) >> sh8) : lo;
            const uint32_t c0 = clsp[w & 0xFFu], c1 = clsp[(w >> 8) & 0xFFu];
            const uint32_t c2 = clsp[(w >> 16) & 0xFFu], c3 = clsp[w >> 24];
            q = pair[(q * P + c0) * P + c1];
            if (q >= K) return q == K ? 1u : 0u;
            q = pair[(q * P + c2) * P + c3];
            if (q >= K) return q == K ? 1u : 0u;
        }
        // the last 1..3 bytes: one more pair if two remain, then the one-byte table
        if (i + 2u <= L) {
            const uint32_t lo = row[dw + (i >> 2)], hi = row[dw + (i >> 2) + 1u];
            const uint32_t w = sh8 ? (uint32_t)((((uint64_t)hi << 32) | lo) >> sh8) : lo;
            q = pair[(q * P + clsp[w & 0xFFu]) * P + clsp[(w >> 8) & 0xFFu]];
            if (q >= K) return q == K ? 1u : 0u;
            i += 2u;
        }
        if (i < L) {   // one byte left: payload byte i sits at row byte staged_sh + i
            const uint32_t at = staged_sh + i;
            const uint32_t b = (row[at >> 2] >> (8u * (at & 3u))) & 0xFFu;
            q = next[q * C + (C == 256u ? b : (uint32_t)cls[b])];
            if (q >= K) return q == K ? 1u : 0u;
        }
        return endacc[q];
    }
    for (; i < L; i += 4u) {
        // four payload bytes from two aligned row dwords (independent of q: issued early)
        const uint32_t lo = row[dw + (i >> 2)], hi = row[dw + (i >> 2) + 1u];
        const uint32_t w = sh8 ? (uint32_t)((((uint64_t)hi << 32) | lo) >> sh8) : lo;
        const uint32_t m = min(4u, L - i);
#pragma unroll
        for (uint32_t k = 0; k < 4u; ++k) {
            if (k < m) {
                const uint32_t b = (w >> (8u * k)) & 0xFFu;
                q = next[q * C + (C == 256u ? b : (uint32_t)cls[b])];
                if (q >= K) return q == K ? 1u : 0u;
            }
        }
    }
    return endacc[q];
