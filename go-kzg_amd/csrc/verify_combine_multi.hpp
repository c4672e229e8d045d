// verify_combine_multi.hpp -- what one lane of the multi-proof combination kernels (k_verify_combine_multi.hip) computes, as host/device
// functions: a row's term scalars, the weight of one interpolation coefficient, and the layout of a group's tiles, partial sums and terms.
//
// CheckProofMulti on row i (n values ys_i on the coset x_i H, np = next_pow2(n), c_i = the inverse transform of the zero-padded ys_i) is
//     e(C_i - [I'_i(s)]_1 + [x_i^np] pi_i, [1]G2) e(-pi_i, [s^n]G2) == 1,     I'_i(X) = sum_j x_i^-j c_i[j] X^j,
// which is linear in the row just as the single check is.  For a group g of consecutive rows with the 128-bit weights r_i of verify_combine.hpp
//     A_g = sum r_i pi_i,     J_g[j] = sum r_i x_i^-j c_i[j]  (j < np),     B_g = sum r_i C_i + sum (r_i x_i^np) pi_i - [J_g(s)]_1,
// and the group passes when e(B_g, [1]G2) e(-A_g, [s^n]G2) == 1.  [J_g(s)]_1 is ONE MSM of np terms over the setup's first np points per group,
// where the per-row check commits to every row's np coefficients.  The kernels keep the index arithmetic, the loads, the stores, the shared
// inversion of a tile's x and the sums through LDS; tests/host/verify_combine_multi_emul.cpp runs these bodies on the CPU.
#pragma once
#include "verify_combine.hpp"

namespace kzg {

constexpr uint32_t COMBINE_MULTI_TILE = 256;      // rows per tile = lanes per workgroup of k_combine_multi_poly
constexpr uint64_t COMBINE_MULTI_NP_MAX = 256;    // a lane keeps one j: np <= lanes.  Longer rows take the per-row route

// One row's term scalars, Montgomery images in and out: the weight r_i (the scalar of C_i in B_g and of pi_i in A_g), r_i x_i^np (of pi_i in
// B_g) and the base x_i^-1 of the row's coefficient weights.  x_inv is the inverse the caller computed for x (any value when x == 0).
// A row that is not `live` gets zeros.  x == 0 follows the reference (bls.InvModFr(0) == 0): the base is 0, so x^-0 = 1 and x^-j = 0 for
// j > 0 (combine_multi_coeff_weight), and x^np = 0 as np >= 1.
KZG_HD void combine_multi_row_scalars(const combine_seed &seed, uint64_t i, bool live, const fr &x_mont, const fr &x_inv_mont, uint64_t np, fr &r_out, fr &rxp_out,
                                      fr &base_out) {
    if (!live) { r_out = zero<FrP>(); rxp_out = zero<FrP>(); base_out = zero<FrP>(); return; }
    const fr r = to_mont<FrP>(combine_weight_std(seed, i));
    fr xp = x_mont;
    for (uint64_t m = 1; m < np; m <<= 1) xp = mul(xp, xp);                    // np is a power of two: log2(np) squarings
    r_out = r; rxp_out = mul(r, xp);
    base_out = is_zero(x_mont) ? zero<FrP>() : x_inv_mont;
}
// the operand a row hands to the tile's shared inversion: block_batch_inverse needs non-zero values
KZG_HD fr combine_multi_inverse_operand(bool live, const fr &x_mont) { return live && !is_zero(x_mont) ? x_mont : one<FrP>(); }

// r x^-j for one coefficient index j from the row's weight and base: square-and-multiply from the top bit of j (j < 2^32)
KZG_HD fr combine_multi_coeff_weight(const fr &r_mont, const fr &base_mont, uint32_t j) {
    if (!j) return r_mont;
    fr acc = base_mont;
    for (int b = 30 - __builtin_clz(j); b >= 0; b--) {
        acc = mul(acc, acc);
        if ((j >> b) & 1u) acc = mul(acc, base_mont);
    }
    return mul(r_mont, acc);
}

// Tiles: tile t of group g holds the group's rows 256 t .. 256 t + 255 (rows g R + 256 t + l of the chunk, l the lane of phase A); a row
// beyond the group's R or beyond the count is dead.  The tile's 256 np coefficients are contiguous in the inverse transform's output; in
// sweep step k lane l reads element 256 k + l of them: coefficient j = l mod np (fixed per lane, np divides 256) of the tile's row
// k (256 / np) + l / np.  The lanes l = j, j + np, ... hold the partial sums of coefficient j; their sum goes to slot j of the tile's np
// partials, which lie at (g T + t) np with T tiles per group.  J_g[j] is the sum of slot j over the group's tiles.
KZG_HD uint64_t combine_multi_tiles(uint64_t R) { return (R + COMBINE_MULTI_TILE - 1) / COMBINE_MULTI_TILE; }
KZG_HD uint64_t combine_multi_tile_row(uint64_t g, uint64_t t, uint64_t R) { return combine_group_begin(g, R) + t * COMBINE_MULTI_TILE; }   // first row, in the chunk
KZG_HD bool combine_multi_row_live(uint64_t t, uint32_t l, uint64_t first_row, uint64_t R, uint64_t count) {
    return t * COMBINE_MULTI_TILE + l < R && first_row + l < count;
}
KZG_HD uint32_t combine_multi_lane_coeff(uint32_t l, uint64_t np) { return l & (uint32_t)(np - 1); }
KZG_HD uint32_t combine_multi_lane_row(uint32_t l, uint32_t k, uint64_t np) { return k * (uint32_t)(COMBINE_MULTI_TILE / np) + l / (uint32_t)np; }
KZG_HD uint64_t combine_multi_partial_at(uint64_t g, uint64_t t, uint64_t R, uint64_t np) { return (g * combine_multi_tiles(R) + t) * np; }
KZG_HD fr combine_multi_fold(const fr *partials, uint64_t g, uint64_t R, uint64_t np, uint64_t j) {
    fr acc = zero<FrP>();
    for (uint64_t t = 0; t < combine_multi_tiles(R); t++) acc = add(acc, partials[combine_multi_partial_at(g, t, R, np) + j]);
    return acc;
}

// A group's slice keeps combine_term_stride(R) = 2 R + 1 slots: C_j with r_j at j, pi_j with r_j x_j^np at R + j, and at 2 R the point
// [J_g(s)]_1 with the scalar -1 (the single form has the generator with -sum r y there)
KZG_HD fr combine_multi_last_scalar() { return neg<FrP>(one<FrP>()); }

}  // namespace kzg
