// sha256_lane.hpp -- SHA-256 (FIPS 180-4) as ONE LANE runs it, and hashToBLSField's reduction (eth/helpers.go:113-133), as host/device
// functions: the transcript kernel of the batched block verifier (k_eth_aggregate.hip) gives every sidecar's chain a lane of its own, and
// tests/host/aggregate_emul.cpp runs the same text on the CPU.  The message is read through a source object, so that a lane can hash bytes
// where they lie (a transcript is a header, the block's blobs and its commitments, three places in memory):
//     void load16(uint64_t off, uint32_t w[4]) const   big-endian words of message bytes off .. off + 15 (off a multiple of 16, all below len)
//     uint8_t byte(uint64_t off) const                 one message byte (the last, partial 16 bytes only)
#pragma once
#include "field.hpp"

namespace kzg {

KZG_HD uint32_t sha_rotr32(uint32_t x, int n) { return (x >> n) | (x << (32 - n)); }
KZG_HD uint32_t sha_bswap32(uint32_t x) { return __builtin_bswap32(x); }

KZG_HD uint32_t sha256_k(int i) {
    const uint32_t k[64] = {
        0x428a2f98u, 0x71374491u, 0xb5c0fbcfu, 0xe9b5dba5u, 0x3956c25bu, 0x59f111f1u, 0x923f82a4u, 0xab1c5ed5u, 0xd807aa98u, 0x12835b01u, 0x243185beu, 0x550c7dc3u,
        0x72be5d74u, 0x80deb1feu, 0x9bdc06a7u, 0xc19bf174u, 0xe49b69c1u, 0xefbe4786u, 0x0fc19dc6u, 0x240ca1ccu, 0x2de92c6fu, 0x4a7484aau, 0x5cb0a9dcu, 0x76f988dau,
        0x983e5152u, 0xa831c66du, 0xb00327c8u, 0xbf597fc7u, 0xc6e00bf3u, 0xd5a79147u, 0x06ca6351u, 0x14292967u, 0x27b70a85u, 0x2e1b2138u, 0x4d2c6dfcu, 0x53380d13u,
        0x650a7354u, 0x766a0abbu, 0x81c2c92eu, 0x92722c85u, 0xa2bfe8a1u, 0xa81a664bu, 0xc24b8b70u, 0xc76c51a3u, 0xd192e819u, 0xd6990624u, 0xf40e3585u, 0x106aa070u,
        0x19a4c116u, 0x1e376c08u, 0x2748774cu, 0x34b0bcb5u, 0x391c0cb3u, 0x4ed8aa4au, 0x5b9cca4fu, 0x682e6ff3u, 0x748f82eeu, 0x78a5636fu, 0x84c87814u, 0x8cc70208u,
        0x90befffau, 0xa4506cebu, 0xbef9a3f7u, 0xc67178f2u};
    return k[i];
}
KZG_HD void sha256_init(uint32_t st[8]) {
    st[0] = 0x6a09e667u; st[1] = 0xbb67ae85u; st[2] = 0x3c6ef372u; st[3] = 0xa54ff53au;
    st[4] = 0x510e527fu; st[5] = 0x9b05688cu; st[6] = 0x1f83d9abu; st[7] = 0x5be0cd19u;
}
// one 64-byte block (16 big-endian words; w is consumed: the schedule rolls through it).  Fully unrolled, every index a constant: the
// sixteen words and the eight state words stay in registers.
KZG_HD void sha256_compress(uint32_t st[8], uint32_t w[16]) {
    uint32_t a = st[0], b = st[1], c = st[2], d = st[3], e = st[4], f = st[5], g = st[6], h = st[7];
#pragma unroll
    for (int i = 0; i < 64; i++) {
        if (i >= 16) {
            const uint32_t w15 = w[(i + 1) & 15], w2 = w[(i + 14) & 15];
            const uint32_t s0 = sha_rotr32(w15, 7) ^ sha_rotr32(w15, 18) ^ (w15 >> 3);
            const uint32_t s1 = sha_rotr32(w2, 17) ^ sha_rotr32(w2, 19) ^ (w2 >> 10);
            w[i & 15] = w[i & 15] + s0 + w[(i + 9) & 15] + s1;
        }
        const uint32_t t1 = h + (sha_rotr32(e, 6) ^ sha_rotr32(e, 11) ^ sha_rotr32(e, 25)) + ((e & f) ^ (~e & g)) + sha256_k(i) + w[i & 15];
        const uint32_t t2 = (sha_rotr32(a, 2) ^ sha_rotr32(a, 13) ^ sha_rotr32(a, 22)) + ((a & b) ^ (a & c) ^ (b & c));
        h = g; g = f; f = e; e = d + t1; d = c; c = b; b = a; a = t1 + t2;
    }
    st[0] += a; st[1] += b; st[2] += c; st[3] += d; st[4] += e; st[5] += f; st[6] += g; st[7] += h;
}
// the whole blocks first .. last - 1 of src into the state st (in and out): a chain cut at a block boundary and taken up again later
template <class Src> KZG_HD void sha256_lane_blocks(const Src &src, uint64_t first, uint64_t last, uint32_t st[8]) {
    uint32_t w[16];
    for (uint64_t b = first; b < last; b++) {
#pragma unroll
        for (int q = 0; q < 4; q++) src.load16(64 * b + 16 * q, w + 4 * q);
        sha256_compress(st, w);
    }
}
// the resumable form: st holds the state after the first `first` blocks of the `len` bytes of src (sha256_init's for first = 0); hashes the
// rest and leaves the digest (eight big-endian words, the SHA's own state) in st.  first <= len / 64.
template <class Src> KZG_HD void sha256_lane_resume(const Src &src, uint64_t len, uint64_t first, uint32_t st[8]) {
    uint32_t w[16];
    const uint64_t full = len / 64;
    sha256_lane_blocks(src, first, full, st);
    // the last block(s): the rest of the message, 0x80, zeros, the length in bits as 64 big-endian bits; two blocks when fewer than 9 bytes are free
    const uint32_t rem = (uint32_t)(len & 63);
    const uint64_t base = 64 * full;
#pragma unroll
    for (int q = 0; q < 4; q++) {
        if (16u * q + 16 <= rem) src.load16(base + 16 * q, w + 4 * q);
        else {
#pragma unroll
            for (int j = 0; j < 4; j++) {
                uint32_t v = 0;
#pragma unroll
                for (int k = 0; k < 4; k++) {
                    const uint32_t at = 16u * q + 4u * j + k;
                    const uint32_t byte = at < rem ? src.byte(base + at) : at == rem ? 0x80u : 0u;
                    v |= byte << (24 - 8 * k);
                }
                w[4 * q + j] = v;
            }
        }
    }
    const uint64_t bits = len * 8;
    if (rem >= 56) {
        sha256_compress(st, w);
#pragma unroll
        for (int j = 0; j < 16; j++) w[j] = 0;
    }
    w[14] = (uint32_t)(bits >> 32); w[15] = (uint32_t)bits;
    sha256_compress(st, w);
}
// digest of the `len` bytes of src
template <class Src> KZG_HD void sha256_lane(const Src &src, uint64_t len, uint32_t st[8]) {
    sha256_init(st);
    sha256_lane_resume(src, len, 0, st);
}

// a plain byte buffer as a message source (any alignment)
struct sha_bytes_src {
    const uint8_t *p;
    KZG_HD void load16(uint64_t off, uint32_t w[4]) const {
#pragma unroll
        for (int j = 0; j < 4; j++) {
            const uint8_t *q = p + off + 4 * j;
            w[j] = (uint32_t)q[0] << 24 | (uint32_t)q[1] << 16 | (uint32_t)q[2] << 8 | q[3];
        }
    }
    KZG_HD uint8_t byte(uint64_t off) const { return p[off]; }
};

// hashToBLSField's second half (eth/helpers.go:124-133): the 32 digest bytes read as a LITTLE-endian integer, reduced mod r (2^256 < 3 r: at
// most two subtractions), as a Montgomery image.  st: the digest as the SHA's eight big-endian words.
KZG_HD fr fr_from_digest_words(const uint32_t st[8]) {
    uint32_t v[8];
#pragma unroll
    for (int i = 0; i < 8; i++) v[i] = sha_bswap32(st[i]);   // limb i = digest bytes 4 i .. 4 i + 3, little-endian
#pragma unroll
    for (int k = 0; k < 2; k++) {
        uint32_t d[8], br = 0;
#pragma unroll
        for (int i = 0; i < 8; i++) d[i] = subb(v[i], FrP::mod(i), br);
#pragma unroll
        for (int i = 0; i < 8; i++) v[i] = br ? v[i] : d[i];
    }
    fr c;
#pragma unroll
    for (int i = 0; i < 8; i++) c.l[i] = v[i];
    return to_mont<FrP>(c);
}
KZG_HD fr fr_from_digest_bytes(const uint8_t d[32]) {
    uint32_t st[8];
#pragma unroll
    for (int i = 0; i < 8; i++) st[i] = (uint32_t)d[4 * i] << 24 | (uint32_t)d[4 * i + 1] << 16 | (uint32_t)d[4 * i + 2] << 8 | d[4 * i + 3];
    return fr_from_digest_words(st);
}
// hashToBLSField of the 33 bytes (transcript digest | tag): the challenges of ComputeChallenges (eth/helpers.go:215-232)
struct sha_challenge_src {
    const uint32_t *tr; uint8_t tag;    // the transcript digest as big-endian words
    KZG_HD void load16(uint64_t off, uint32_t w[4]) const {
#pragma unroll
        for (int j = 0; j < 4; j++) w[j] = off ? tr[4 + j] : tr[j];
    }
    KZG_HD uint8_t byte(uint64_t) const { return tag; }   // byte 32 is the only one past the two full groups
};
KZG_HD fr hash_to_bls_field_33(const uint32_t tr[8], uint8_t tag) {
    uint32_t st[8];
    sha256_lane(sha_challenge_src{tr, tag}, 33, st);
    return fr_from_digest_words(st);
}

}   // namespace kzg
