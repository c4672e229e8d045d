// Index arithmetic of the paired-point table (go-kzg_amd/csrc/fb_pair_index.hpp) on the host, against plain 128-bit integers.
//   c = 5, every (d0, d1) in [-D, D]^2: the canonical tuples map one-to-one onto [0, E), the word decodes to the tuple, (0, 0) is word 0;
//   c = 5, 7, 10: two 127-bit magnitudes with all four half-sign combinations recoded into W words reconstruct both signed values,
//   sum_w d_w 2^(c w), with every digit in [-D, D]; magnitudes whose top digit takes the last carry are among them.
#include <stdint.h>
#include <stdio.h>
#include <vector>
#include "fb_pair_index.hpp"

using namespace kzg;
typedef __int128 i128;
typedef unsigned __int128 u128;

static int fails = 0;
#define CHECK(cond, ...) do { if (!(cond)) { if (fails++ < 20) { printf("FAIL %s:%d: ", __FILE__, __LINE__); printf(__VA_ARGS__); printf("\n"); } } } while (0)

static uint64_t rng_state = 0x9e3779b97f4a7c15ull;
static uint64_t rnd() { rng_state ^= rng_state << 13; rng_state ^= rng_state >> 7; rng_state ^= rng_state << 17; return rng_state; }

static void exhaustive(uint32_t c) {
    const int32_t D = 1 << (c - 1);
    const uint64_t E = fb_paired_entries(c);
    CHECK(E == 2ull * D * (D + 1), "E at c=%u", c);
    std::vector<int> seen(E, 0);
    for (int32_t d0 = -D; d0 <= D; d0++)
        for (int32_t d1 = -D; d1 <= D; d1++) {
            const uint32_t word = fb_pair_word(d0, d1, (uint32_t)D);
            if (d0 == 0 && d1 == 0) { CHECK(word == 0, "(0, 0) gives %#x", word); continue; }
            const uint32_t idx1 = word & 0xfffffu;
            CHECK((word & 0x7ff00000u) == 0 && idx1 >= 1 && idx1 <= E, "word %#x of (%d, %d)", word, d0, d1);
            if (!(idx1 >= 1 && idx1 <= E)) continue;
            const bool canonical = d0 > 0 || (d0 == 0 && d1 > 0);
            CHECK((word >> 31) == (canonical ? 0u : 1u), "negate bit of (%d, %d)", d0, d1);
            if (canonical) { seen[idx1 - 1]++; CHECK(fb_pair_index(d0, d1, (uint32_t)D) == idx1 - 1, "index of (%d, %d)", d0, d1); }
            int32_t e0, e1;
            fb_pair_tuple(idx1 - 1, (uint32_t)D, e0, e1);
            CHECK(e0 == (canonical ? d0 : -d0) && e1 == (canonical ? d1 : -d1), "tuple of (%d, %d): (%d, %d)", d0, d1, e0, e1);
            fb_pair_word_tuple(word, (uint32_t)D, e0, e1);
            CHECK(e0 == d0 && e1 == d1, "decode of (%d, %d): (%d, %d)", d0, d1, e0, e1);
        }
    for (uint64_t i = 0; i < E; i++) CHECK(seen[i] == 1, "entry %llu of c=%u hit %d times", (unsigned long long)i, c, seen[i]);
}

static void to_words(u128 v, uint32_t (&m)[4]) { for (int j = 0; j < 4; j++) m[j] = (uint32_t)(v >> (32 * j)); }

static void recode_case(uint32_t c, u128 a, u128 b) {
    const uint32_t W = fb_paired_windows(c);
    const int32_t D = 1 << (c - 1);
    uint32_t m0[4], m1[4];
    to_words(a, m0); to_words(b, m1);
    for (int signs = 0; signs < 4; signs++) {
        const bool n0 = signs & 1, n1 = signs & 2;
        std::vector<uint32_t> words(3 * W, 0xdeadbeefu);
        fb_pair_recode(m0, n0, m1, n1, c, W, words.data(), 3);            // stride 3: the words between stay untouched
        u128 s0 = 0, s1 = 0;                                                // Horner modulo 2^128 (the running value passes 2^127 on the way) ...
        double f0 = 0.0, f1 = 0.0;                                          // ... and in floating point, which tells multiples of 2^128 apart
        for (uint32_t w = W; w-- > 0;) {
            int32_t d0, d1;
            CHECK((words[3 * w] & 0x7ff00000u) == 0 && (words[3 * w] & 0xfffffu) <= fb_paired_entries(c), "word %#x", words[3 * w]);
            fb_pair_word_tuple(words[3 * w], (uint32_t)D, d0, d1);
            CHECK(d0 >= -D && d0 <= D && d1 >= -D && d1 <= D, "digits (%d, %d) at c=%u", d0, d1, c);
            s0 = s0 * ((u128)1 << c) + (u128)(i128)d0; s1 = s1 * ((u128)1 << c) + (u128)(i128)d1;
            f0 = f0 * (double)(1u << c) + d0; f1 = f1 * (double)(1u << c) + d1;
            CHECK(words[3 * w + 1] == 0xdeadbeefu && words[3 * w + 2] == 0xdeadbeefu, "stride");
        }
        const double two100 = 1267650600228229401496703205376.0;
        CHECK(f0 - (n0 ? -(double)a : (double)a) < two100 && (n0 ? -(double)a : (double)a) - f0 < two100, "c=%u signs=%d: coefficient 0 is off by a multiple of 2^128", c, signs);
        CHECK(f1 - (n1 ? -(double)b : (double)b) < two100 && (n1 ? -(double)b : (double)b) - f1 < two100, "c=%u signs=%d: coefficient 1 is off by a multiple of 2^128", c, signs);
        CHECK(s0 == (n0 ? (u128)0 - a : a), "c=%u signs=%d: coefficient 0 of %016llx%016llx", c, signs, (unsigned long long)(a >> 64), (unsigned long long)a);
        CHECK(s1 == (n1 ? (u128)0 - b : b), "c=%u signs=%d: coefficient 1 of %016llx%016llx", c, signs, (unsigned long long)(b >> 64), (unsigned long long)b);
    }
}

int main() {
    exhaustive(5);
    exhaustive(7);
    CHECK(fb_paired_entries(10) == 525312 && fb_paired_windows(10) == 13 && fb_paired_entries(10) <= (1u << 20), "c = 10 shape");
    CHECK(fb_paired_table_bytes(4096, 10, 96) == 103280541696ull && fb_paired_table_bytes(255, 5, 96) == 128ull * 544 * 96, "bytes");
    CHECK(fb_paired_windows(5) == 26 && fb_paired_windows(7) == 19, "windows");
    const u128 top = ((u128)1 << 127) - 1;
    for (uint32_t c : {5u, 7u, 10u}) {
        const uint32_t W = fb_paired_windows(c);
        const u128 D = (u128)1 << (c - 1);
        std::vector<u128> edge = {0, 1, D - 1, D, D + 1, 2 * D - 1, 2 * D, top, top - 1, (u128)1 << 126, ((u128)1 << 126) + D, top - D, top - D + 1};
        u128 all_d = 0, all_d1 = 0, alt = 0;                                   // every digit D; D + 1 (all carry); alternating 0 / 2^c - 1
        for (uint32_t w = 0; w < W; w++) {
            if (c * w + c <= 127) { all_d |= D << (c * w); all_d1 |= (D + 1) << (c * w); if (w & 1) alt |= (2 * D - 1) << (c * w); }
        }
        edge.push_back(all_d); edge.push_back(all_d1); edge.push_back(alt);
        // the top digit takes the last carry: every window below the top one holds 2^c - 1 (raw > D all the way up), the top one what 127 bits leave
        edge.push_back((top >> 1) | ((u128)1 << 126));
        edge.push_back((((u128)1 << (c * (W - 1))) - 1) & top);               // carries run into an empty top window
        for (size_t i = 0; i < edge.size(); i++)
            for (size_t j = 0; j < edge.size(); j++) recode_case(c, edge[i] & top, edge[j] & top);
        for (int t = 0; t < 2000; t++) {
            const u128 a = (((u128)rnd() << 64) | rnd()) & top, b = (((u128)rnd() << 64) | rnd()) & top;
            recode_case(c, a, b);
            recode_case(c, a >> (rnd() % 127), b);
        }
    }
    if (fails) { printf("fb_pair_index_test: %d failures\n", fails); return 1; }
    printf("fb_pair_index_test: ok\n");
    return 0;
}
