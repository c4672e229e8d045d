// recover_rows.hpp -- lane bodies of the batched erasure recovery (k_recovery.hip, capi_recovery.hip): everything with index arithmetic or a carried
// product, written so that it also compiles for the host (tests/host/recovery_batch_emul.cpp replays whole small problems through these bodies).
//
// A chunk of rows moves through every stage together.  Per row: the erasure list (ascending indices of the missing samples), its length `count`, and the
// EFFECTIVE length nm = count, or 0 for a row with nothing present (that row is not recovered; it is carried through as if nothing were missing and
// zero-filled at the end, so that no kernel ever sees a vanishing polynomial of degree n).
//   * product tree: the rows of a chunk share ONE leaf count (the largest any of them needs), so every level is nodes x rows equal nodes and the pair / join
//     kernels of the lone path run unchanged over rows x nodes; a row with fewer roots pads with roots at 0 (factors x), pad = 16 leaves - nm, and its root
//     is Z(x) x^pad.
//   * division: Montgomery's trick over strips of 64 denominators, the strips laid ACROSS the flattened rows: lane c of L = ceil(total / 64) walks the
//     elements c, c + L, c + 2 L, ... -- neighbouring lanes touch neighbouring elements in every step -- and spends one inversion on all of them.
//   * status: one byte per row.
#pragma once
#include "field.hpp"
#include "fr_lazy.hpp"

namespace kzg {
namespace rr {

constexpr uint32_t LEAF = 16;             // roots per leaf (ZERO_TREE_LEAF of internal.hpp)
constexpr uint32_t STRIP = 64;            // denominators per inversion
constexpr uint8_t ST_OK = 0, ST_BAD_ARG = 5, ST_RECOVERY = 10;   // KZG_HIP_OK, KZG_HIP_ERR_BAD_ARG, KZG_HIP_ERR_RECOVERY (checked in capi_recovery.hip)

// ---- erasure lists: a row's mask is cut into `parts` contiguous pieces, one per lane; counts are scanned, then every lane writes its piece ----
KZG_HD uint64_t piece_len(uint64_t n, uint32_t parts) { return (n + parts - 1) / parts; }
KZG_HD void piece_bounds(uint64_t n, uint32_t parts, uint32_t t, uint64_t &lo, uint64_t &hi) {
    const uint64_t per = piece_len(n, parts);
    lo = (uint64_t)t * per < n ? (uint64_t)t * per : n;
    hi = lo + per < n ? lo + per : n;
}
KZG_HD uint32_t piece_count(const uint8_t *present, uint64_t lo, uint64_t hi) {
    uint32_t c = 0;
    for (uint64_t i = lo; i < hi; i++) c += present[i] ? 0u : 1u;
    return c;
}
KZG_HD void piece_emit(const uint8_t *present, uint64_t lo, uint64_t hi, uint64_t *list_at) {   // list_at: the row's list + the exclusive scan of the counts
    for (uint64_t i = lo; i < hi; i++) if (!present[i]) *list_at++ = i;
}
KZG_HD uint64_t effective_missing(uint64_t count, uint64_t n) { return count >= n ? 0 : count; }

// ---- direct evaluation on lazy limbs: every product of two images leaves 2^-5 (k_zero_eval_direct); a row's chain has nm steps and segs - 1 joins ----
KZG_HD fr lazy_chain_correction(uint64_t nm, uint32_t segs) {
    fr corr = one<FrP>(), pw = fr_from_u64(32);
    for (uint64_t e = nm + segs - 1; e; e >>= 1) { if (e & 1) corr = mul(corr, pw); pw = mul(pw, pw); }
    return corr;
}

// ---- ragged product tree ----
KZG_HD uint64_t shared_leaves(uint64_t max_nm) {          // leaf count of a chunk whose longest erasure list has max_nm entries
    uint64_t leaves = 1;
    while (leaves * LEAF < max_nm) leaves <<= 1;
    return leaves;
}
KZG_HD uint64_t row_pad(uint64_t leaves, uint64_t nm) { return leaves * LEAF - nm; }   // roots at 0 that fill the row's leaves
// leaf `leaf` of a row: prod (x - w^m) over the row's list entries [16 leaf, 16 leaf + 16), entries beyond nm being roots at 0.  c: LEAF + 1 running
// coefficients, coefficient j at c[j * cs] (a lane's column of the workgroup's LDS area; cs = 1 on the host); out: the 16 non-leading coefficients.
KZG_HD void leaf_product(const fr *expanded, uint64_t stride, const uint64_t *list, uint64_t nm, uint64_t leaf, fr *c, uint32_t cs, fr *out) {
    const uint64_t lo = leaf * LEAF;
    c[0] = one<FrP>();
    for (uint32_t i = 0; i < LEAF; i++) {                 // c <- c (x - r_i); beyond the list r = 0: c <- c x
        const bool real = lo + i < nm;
        const fr r = real ? expanded[list[lo + i] * stride] : zero<FrP>();
        c[(i + 1) * cs] = c[i * cs];                      // the leading coefficient (1) moves up
        for (uint32_t j = i; j >= 1; j--) c[j * cs] = real ? sub(c[(j - 1) * cs], mul(r, c[j * cs])) : c[(j - 1) * cs];
        c[0] = real ? neg<FrP>(mul(r, c[0])) : zero<FrP>();
    }
    for (uint32_t j = 0; j < LEAF; j++) out[j] = c[j * cs];
}
// coefficient t of Z = root / x^pad (root: the leaves * 16 non-leading coefficients of the row's monic root)
KZG_HD fr unpad_coeff(const fr *root, uint64_t pad, uint64_t nm, uint64_t t) {
    return t < nm ? root[t + pad] : (t == nm ? one<FrP>() : zero<FrP>());
}

// ---- strip division: out[i] = (num ? num[i] : 1) / den[i] for this lane's elements c, c + L, ... < total; a zero denominator counts as one ----
// (rows that are not recovered may hold zeros; one of them would otherwise wipe out its whole strip).  out aliases neither num nor den: it holds the
// running products on the way up.
KZG_HD uint64_t strip_lanes(uint64_t total) { return (total + STRIP - 1) / STRIP; }
KZG_HD void strip_divide(const fr *num, const fr *den, fr *out, uint64_t c, uint64_t L, uint64_t total) {
    fr acc = one<FrP>();
    uint32_t cnt = 0;
    for (uint64_t i = c; i < total && cnt < STRIP; i += L, cnt++) {
        fr d = den[i];
        if (is_zero<FrP>(d)) d = one<FrP>();
        out[i] = acc;
        acc = mul(acc, d);
    }
    fr ia = inv<FrP>(acc);
    for (uint32_t k = cnt; k-- > 0;) {
        const uint64_t i = c + (uint64_t)k * L;
        fr d = den[i];
        if (is_zero<FrP>(d)) d = one<FrP>();
        const fr q = mul(ia, out[i]);                     // 1 / den[i]
        ia = mul(ia, d);
        out[i] = num ? mul(num[i], q) : q;
    }
}

// ---- row status (recover_from_samples.go:44-49, :103-107) ----
KZG_HD bool sample_differs(uint8_t present, const fr &recon, const fr &sample) { return present && !equal<FrP>(recon, sample); }
KZG_HD uint8_t row_status(uint64_t count, uint64_t n, bool mismatch) {
    if (count >= n) return ST_BAD_ARG;                    // nothing present
    if (count == 0) return ST_OK;                         // nothing missing: copied through, nothing was divided
    return mismatch ? ST_RECOVERY : ST_OK;
}
KZG_HD fr row_output(uint8_t status, uint64_t count, const fr &sample, const fr &recon) {
    if (status != ST_OK) return zero<FrP>();
    return count == 0 ? sample : recon;
}

}  // namespace rr
}  // namespace kzg
