// eth_aggregate.hpp -- what one lane of the block verifier's kernels (k_eth_aggregate.hip) computes, as host/device functions: the Fiat-Shamir
// transcript of one sidecar (hashPolysComms + the two hashToBLSField calls of ComputeChallenges, eth/helpers.go:215-260) over the block's
// raw bytes, and one coefficient of its aggregated polynomial (bls.PolyLinComb over the powers of the challenge, eth/helpers.go:137-147).
// The kernels keep the index arithmetic and the stores; tests/host/aggregate_emul.cpp runs these bodies on the CPU.
#pragma once
#include "sha256_lane.hpp"

namespace kzg {

// the transcript as a message: "FSBLOBVERIFY_V1_" | n as u64 LE | count as u64 LE | the blobs' bytes | the commitments' bytes.  FrTo32 of a
// valid element is the blob's own 32 bytes; a block with an invalid element is reported as such and its challenges are never used.
// Every part is a multiple of 16 bytes long, so a 16-byte group never straddles two of them; blobs / comms are 4-byte aligned.
struct eth_transcript_src {
    const uint8_t *blobs, *comms;   // the sidecar's first blob / first commitment
    uint64_t n, count;
    KZG_HD uint64_t blob_bytes() const { return count * n * 32; }
    KZG_HD uint64_t len() const { return 32 + blob_bytes() + count * 48; }
    KZG_HD void load16(uint64_t off, uint32_t w[4]) const {
        if (off >= 32) {
            const uint64_t at = off - 32, bb = blob_bytes();
            const uint32_t *p = (const uint32_t *)(at < bb ? blobs + at : comms + (at - bb));
#pragma unroll
            for (int j = 0; j < 4; j++) w[j] = sha_bswap32(p[j]);
        } else if (off == 0) {
            w[0] = 0x4653424cu; w[1] = 0x4f425645u; w[2] = 0x52494659u; w[3] = 0x5f56315fu;   // "FSBL" "OBVE" "RIFY" "_V1_"
        } else {
            w[0] = sha_bswap32((uint32_t)n); w[1] = sha_bswap32((uint32_t)(n >> 32));
            w[2] = sha_bswap32((uint32_t)count); w[3] = sha_bswap32((uint32_t)(count >> 32));
        }
    }
    KZG_HD uint8_t byte(uint64_t) const { return 0; }   // never reached: the length is a multiple of 16
};
// linCombChallenge and evalChallenge of one sidecar, Montgomery images
KZG_HD void eth_transcript_lane(const uint8_t *blobs, const uint8_t *comms, uint64_t n, uint64_t count, fr &r_out, fr &z_out) {
    const eth_transcript_src src{blobs, comms, n, count};
    uint32_t tr[8];
    sha256_lane(src, src.len(), tr);
    r_out = hash_to_bls_field_33(tr, 0);
    z_out = hash_to_bls_field_33(tr, 1);
}

// The same chain in two halves, for a PROVER: its commitments do not exist yet when its blobs do.  The header is 32 bytes and a blob 32 n
// bytes with n a power of two >= 2, so the first 32 count n bytes of the message -- the header and all blob bytes but the last 32 -- are
// count n / 2 whole SHA blocks that no commitment touches.  The blob half hashes them and leaves the eight state words (the initial state
// for count = 0); the finish half takes the state up again at that block with the last 32 blob bytes and the compressed commitments.
KZG_HD uint64_t eth_transcript_blob_blocks(uint64_t n, uint64_t count) { return count * n / 2; }
KZG_HD void eth_transcript_blobs_lane(const uint8_t *blobs, uint64_t n, uint64_t count, uint32_t st[8]) {
    const eth_transcript_src src{blobs, blobs, n, count};   // (no group of the blob half reaches the commitments)
    sha256_init(st);
    sha256_lane_blocks(src, 0, eth_transcript_blob_blocks(n, count), st);
}
KZG_HD void eth_transcript_finish_lane(const uint8_t *blobs, const uint8_t *comms, uint64_t n, uint64_t count, const uint32_t st_in[8], fr &r_out, fr &z_out) {
    const eth_transcript_src src{blobs, comms, n, count};
    uint32_t tr[8];
#pragma unroll
    for (int i = 0; i < 8; i++) tr[i] = st_in[i];
    sha256_lane_resume(src, src.len(), eth_transcript_blob_blocks(n, count), tr);
    r_out = hash_to_bls_field_33(tr, 0);
    z_out = hash_to_bls_field_33(tr, 1);
}

// coefficient i of sum_k r^k blob_k in Horner order from the last blob to the first.  The elements stay PLAIN: the Montgomery product of a
// plain value and the Montgomery image of r is the plain product, so one product per element and one conversion of the sum at the end
// give the Montgomery image that bls.PolyLinComb gives.  Returns false when one of the `count` elements is not below r (bls.FrFrom32).
KZG_HD bool eth_agg_poly_lane(const uint8_t *blobs, uint64_t n, uint64_t count, uint64_t i, const fr &r_mont, fr &out) {
    fr acc = zero<FrP>();
    bool ok = true;
    for (uint64_t k = count; k-- > 0;) {
        const uint32_t *p = (const uint32_t *)(blobs + (k * n + i) * 32);
        fr v;
#pragma unroll
        for (int j = 0; j < 8; j++) v.l[j] = p[j];
        uint32_t br = 0;
#pragma unroll
        for (int j = 0; j < 8; j++) (void)subb(v.l[j], FrP::mod(j), br);
        ok = ok && br;                                  // v < r  <=>  v - r borrows
        acc = add(mul(acc, r_mont), v);                 // (an invalid v poisons only this sidecar's row, which is never used)
    }
    out = to_mont<FrP>(acc);
    return ok;
}

}   // namespace kzg
