// verify_combine.hpp -- what one lane of the combination kernels (k_verify_combine.hip) computes, as host/device functions: the weights of a
// random linear combination of KZG checks, the term scalars of a group's two MSMs, and the layout of a group's terms.  Below them, as a plain host
// template, the loop that every _combined entry runs over a call's chunks and groups (combine_drive).
//
// For a group g of consecutive rows i with 128-bit weights r_i
//     A_g = sum r_i pi_i,     B_g = sum r_i C_i + sum (r_i x_i) pi_i - (sum r_i y_i) G1,
// and the group passes when e(B_g, [1]G2) e(-A_g, [s]G2) == 1: the sum of the rows' own equations e(C_i - [y_i]G1 + [x_i] pi_i, G2) e(-pi_i, [s]G2)
// == 1 with weights no prover can aim at.  Every row valid: the group passes; a group with an invalid row passes with probability <= 2^-128 over
// the weights (points of G1).  The kernels keep the index arithmetic, the loads, the stores and the sum over a group;
// tests/host/verify_combine_emul.cpp runs these bodies on the CPU.
#pragma once
#include "verify_inputs.hpp"
#include "sha256_lane.hpp"
#include <vector>

namespace kzg {

// rows per group unless KZG_HIP_VERIFY_COMBINE_ROWS says otherwise: 65 536 rows are 64 group checks, one flat launch of the wavefront pairing
// kernel, and a group's two MSMs have 2049 and 1024 terms (profiles/verify_combine.md)
constexpr uint64_t VERIFY_COMBINE_ROWS = 1024;
constexpr uint64_t VERIFY_COMBINE_ROWS_MAX = 1ull << 20;   // a group's terms are indexed in 27 bits by the bucket pipeline (msm_index_range_ok)

// the seed as the SHA's big-endian words, passed to the kernels by value
struct combine_seed { uint32_t w[8]; };
KZG_HD combine_seed combine_seed_from_bytes(const uint8_t *seed32) {
    combine_seed s;
    for (int j = 0; j < 8; j++) s.w[j] = (uint32_t)seed32[4 * j] << 24 | (uint32_t)seed32[4 * j + 1] << 16 | (uint32_t)seed32[4 * j + 2] << 8 | seed32[4 * j + 3];
    return s;
}

// r_i: the little-endian integer of the first 16 bytes of SHA-256(seed32 | "KZGHIPRC" | le64(i)), STANDARD form (< 2^128 < r).  48 bytes are one
// block -- 12 message words, 0x80, zeros, the length 384 in bits -- so this is one sha256_compress.  i is the row's index in the call.
KZG_HD fr combine_weight_std(const combine_seed &seed, uint64_t i) {
    uint32_t w[16], st[8];
#pragma unroll
    for (int j = 0; j < 8; j++) w[j] = seed.w[j];
    w[8] = 0x4b5a4748u; w[9] = 0x49505243u;                                   // "KZGH", "IPRC"
    w[10] = sha_bswap32((uint32_t)i); w[11] = sha_bswap32((uint32_t)(i >> 32));
    w[12] = 0x80000000u; w[13] = 0; w[14] = 0; w[15] = 384;
    sha256_init(st);
    sha256_compress(st, w);
    fr r;
#pragma unroll
    for (int j = 0; j < 4; j++) { r.l[j] = sha_bswap32(st[j]); r.l[4 + j] = 0; }   // limb j = digest bytes 4 j .. 4 j + 3, little-endian
    return r;
}

// One row's share of its group's term scalars, Montgomery images in and out (what launch_msm reads): the weight r_i (the scalar of C_i in B_g and
// of pi_i in A_g), r_i x_i (of pi_i in B_g) and r_i y_i (summed over the group; its negative is the generator's scalar).  A row that is not
// `live` -- beyond the call's count, or malformed in the eth form -- has weight 0 and contributes nothing.
KZG_HD void combine_row_scalars(const combine_seed &seed, uint64_t i, bool live, const fr &x_mont, const fr &y_mont, fr &r_out, fr &rx_out, fr &ry_out) {
    if (!live) { r_out = zero<FrP>(); rx_out = zero<FrP>(); ry_out = zero<FrP>(); return; }
    const fr r = to_mont<FrP>(combine_weight_std(seed, i));
    r_out = r; rx_out = mul(r, x_mont); ry_out = mul(r, y_mont);
}
// the generator's scalar in B_g from u_g = sum r_i y_i
KZG_HD fr combine_generator_scalar(const fr &u_mont) { return neg<FrP>(u_mont); }

// Groups are consecutive rows: group g holds rows g R .. min(count, (g + 1) R).  Its terms lie in one slice of 2 R + 1 slots, points and scalars
// alike: C_j at j, pi_j at R + j, the generator at 2 R.  B_g is the MSM over the whole slice, A_g the MSM over the R slots from R on with the
// scalars of the FIRST R slots (the weights).  Slots of rows beyond the count hold scalar 0 (and the point at infinity).
KZG_HD uint64_t combine_group_count(uint64_t count, uint64_t R) { return (count + R - 1) / R; }
KZG_HD uint64_t combine_group_begin(uint64_t g, uint64_t R) { return g * R; }
KZG_HD uint64_t combine_group_end(uint64_t g, uint64_t R, uint64_t count) { return (g + 1) * R < count ? (g + 1) * R : count; }
KZG_HD uint64_t combine_term_stride(uint64_t R) { return 2 * R + 1; }

// what a _combined call did: route 1 when it combined, the group checks it ran, those that failed, and the rows re-checked one by one
struct combine_stats { uint64_t route, groups, failed, rechecked; };

// The host loop of every _combined entry (capi_verify.hip), free of the device: `count` rows in chunks of chunk_rows (a multiple of R, so that a
// chunk holds whole groups of the call), one group check per R rows, the rows of a failing group checked again one by one.
//   chunk(i0, k, G, status, gok) -> code: everything rows i0 .. i0 + k do on the device.  It fills gok[G] (1: the group passed) and may give
//       a row a status other than 0 (status[k], zeroed: the eth form's 2 / 3); it hashes a row's weight from i0 + the row's index in the chunk,
//       its index in the CALL, and returns with nothing in flight into either buffer.
//   recheck(b, e) -> code: writes out[b .. e) itself.
// out is written only after a chunk's code is 0: a row of a passing group gets its status, or 1 where that is 0; a failing group is left to
// recheck alone.  The first code other than 0 from either is returned at once and nothing is called after it.
template <class Chunk, class Recheck>
int combine_drive(uint64_t count, uint64_t R, uint64_t chunk_rows, uint8_t *out, combine_stats &st, Chunk chunk, Recheck recheck) {
    std::vector<uint8_t> status, gok;
    for (uint64_t i0 = 0; i0 < count; i0 += chunk_rows) {
        const uint64_t k = count - i0 < chunk_rows ? count - i0 : chunk_rows, G = combine_group_count(k, R);
        status.assign(k, 0); gok.assign(G, 0);
        if (const int code = chunk(i0, k, G, status.data(), gok.data())) return code;
        st.groups += G;
        for (uint64_t g = 0; g < G; g++) {
            const uint64_t b = combine_group_begin(g, R), e = combine_group_end(g, R, k);
            if (gok[g]) { for (uint64_t i = b; i < e; i++) out[i0 + i] = status[i] ? status[i] : 1; continue; }
            st.failed++; st.rechecked += e - b;
            if (const int code = recheck(i0 + b, i0 + e)) return code;
        }
    }
    return 0;
}

// eth.VerifyKZGProof's field parsing (eth/eth.go:114-135) in front of the combination: z and y as Montgomery images, and the row's status from
// them and from the decompression flags of its commitment and proof, in the reference's order (z, y, commitment, proof): 0 valid, 2, 3
KZG_HD void eth_combine_fields_lane(const uint8_t *z32, const uint8_t *y32, uint8_t c_bad, uint8_t pi_bad, fr &z_mont, fr &y_mont, uint8_t &status) {
    fr z, y;
    z_mont = zero<FrP>(); y_mont = zero<FrP>();
    if (!fr_from_le32_checked(z, z32) || !fr_from_le32_checked(y, y32)) { status = 2; return; }
    if (c_bad || pi_bad) { status = 3; return; }
    status = 0;
    z_mont = to_mont<FrP>(z); y_mont = to_mont<FrP>(y);
}

}  // namespace kzg
