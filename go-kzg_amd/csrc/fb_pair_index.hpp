// fb_pair_index.hpp -- index arithmetic of the PAIRED-POINT table of large commitment batches (k_msm.hip: k_fb_build_paired, k_fb_digits_paired,
// k_fb_accumulate_paired; capi_kzg.hip sizes the table with it).  Free of HIP: tests/host/fb_pair_index_test.cpp compiles it with the host compiler.
//
// One entry of the table is indexed by the digits of TWO neighbouring points:  T_p[g E + idx(d0, d1)] = d0 P_2g + d1 P_2g+1  with signed c-bit digits,
// D = 2^(c-1).  A digit of a GLV half is recoded into [-(D - 1), D] with a carry (as k_fb_digits does) and the half's own sign is folded in first -- the two
// coefficients of a pair have independent half signs -- so both folded digits lie in [-D, D].  The tuple is stored up to a common sign: canonical tuples have
// d0 > 0, or d0 = 0 and d1 > 0, the others are negated and carry the negate bit.  Row set of a pair, E = 2 D (D + 1) entries:
//     [0, D)                                  d0 = 0, d1 = 1 .. D
//     D + (d0 - 1) (2 D + 1) + (d1 + D)       d0 = 1 .. D, d1 = -D .. D
// Digit word (the format of k_fb_digits): entry index + 1 in bits 0..19 (E <= 2^20 up to c = 10), bit 31 negate, 0 = both digits are zero.
#pragma once
#include <stdint.h>

#if defined(__HIPCC__) || defined(__CUDACC__)
#define FB_PAIR_HD __host__ __device__ inline
#else
#define FB_PAIR_HD inline
#endif

namespace kzg {

#define FB_PAIRED_MAX_BITS 10u     // widest digits whose row set fits the 20 index bits of a digit word
#define FB_PAIRED_LOW_BITS 5u      // narrowest digits the planner considers

FB_PAIR_HD uint64_t fb_paired_entries(uint32_t c) { const uint64_t D = 1ull << (c - 1); return 2 * D * (D + 1); }
FB_PAIR_HD uint32_t fb_paired_windows(uint32_t c) { return (128 + c - 1) / c; }
FB_PAIR_HD uint64_t fb_paired_pairs(uint64_t n) { return (n + 1) / 2; }
// bytes of the table over n points with entries of entry_bytes (an odd n leaves its last point with a partner of digit 0: the row set is built all the same)
FB_PAIR_HD uint64_t fb_paired_table_bytes(uint64_t n, uint32_t c, uint64_t entry_bytes) { return fb_paired_pairs(n) * fb_paired_entries(c) * entry_bytes; }

// entry index of a CANONICAL tuple
FB_PAIR_HD uint32_t fb_pair_index(int32_t d0, int32_t d1, uint32_t D) {
    return d0 == 0 ? (uint32_t)(d1 - 1) : D + (uint32_t)(d0 - 1) * (2 * D + 1) + (uint32_t)(d1 + (int32_t)D);
}
// ... and back
FB_PAIR_HD void fb_pair_tuple(uint32_t idx, uint32_t D, int32_t &d0, int32_t &d1) {
    if (idx < D) { d0 = 0; d1 = (int32_t)idx + 1; return; }
    const uint32_t e = idx - D;
    d0 = (int32_t)(e / (2 * D + 1)) + 1;
    d1 = (int32_t)(e % (2 * D + 1)) - (int32_t)D;
}
// digit word of any tuple with d0, d1 in [-D, D]
FB_PAIR_HD uint32_t fb_pair_word(int32_t d0, int32_t d1, uint32_t D) {
    if (d0 == 0 && d1 == 0) return 0u;
    const bool ng = d0 < 0 || (d0 == 0 && d1 < 0);
    if (ng) { d0 = -d0; d1 = -d1; }
    return (fb_pair_index(d0, d1, D) + 1u) | (ng ? 0x80000000u : 0u);
}
// the tuple a digit word stands for, negate bit applied
FB_PAIR_HD void fb_pair_word_tuple(uint32_t word, uint32_t D, int32_t &d0, int32_t &d1) {
    if (!(word & 0xfffffu)) { d0 = 0; d1 = 0; return; }
    fb_pair_tuple((word & 0xfffffu) - 1u, D, d0, d1);
    if (word >> 31) { d0 = -d0; d1 = -d1; }
}

// c bits of a 128-bit magnitude from bit `off` on (zeros above bit 127)
FB_PAIR_HD uint32_t fb_pair_bits(const uint32_t (&m)[4], uint32_t off, uint32_t c) {
    const uint32_t idx = off >> 5, sh = off & 31;
    if (idx >= 4) return 0;
    uint64_t v = m[idx];
    if (idx + 1 < 4) v |= (uint64_t)m[idx + 1] << 32;
    return (uint32_t)(v >> sh) & ((1u << c) - 1u);
}
// signed digit w of the magnitude m, in [-(D - 1), D]; carry is 0 before window 0 and is handed on from window to window.  With c W >= 128 and m < 2^127
// the top digit never carries out.
FB_PAIR_HD int32_t fb_pair_digit(const uint32_t (&m)[4], uint32_t w, uint32_t c, uint32_t &carry) {
    const uint32_t D = 1u << (c - 1);
    const uint32_t raw = fb_pair_bits(m, w * c, c) + carry;
    if (raw > D) { carry = 1; return -(int32_t)((1u << c) - raw); }
    carry = 0;
    return (int32_t)raw;
}
// The W digit words of one GLV half of a pair: magnitudes m0, m1 of coefficients 2g and 2g + 1 (a missing partner: all zero), neg0 / neg1 their half signs.
// out[w * stride] receives window w.
FB_PAIR_HD void fb_pair_recode(const uint32_t (&m0)[4], bool neg0, const uint32_t (&m1)[4], bool neg1, uint32_t c, uint32_t W, uint32_t *out, uint64_t stride) {
    const uint32_t D = 1u << (c - 1);
    uint32_t c0 = 0, c1 = 0;
    for (uint32_t w = 0; w < W; w++) {
        int32_t d0 = fb_pair_digit(m0, w, c, c0), d1 = fb_pair_digit(m1, w, c, c1);
        if (neg0) d0 = -d0;
        if (neg1) d1 = -d1;
        out[(uint64_t)w * stride] = fb_pair_word(d0, d1, D);
    }
}

}  // namespace kzg
