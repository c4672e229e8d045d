// pairing.hpp -- the optimal ate pairing of BLS12-381 (x = -0xd201000000010000) for gfx950 lanes: prepared G2 points, a multi-Miller loop
// over k pairs that shares the F_p12 squarings, and the final exponentiation.  Replaces Kilic's Engine (AddPair / AddPairInv / Check) behind
// bls.PairingsVerify (bls/bls_kilic.go:153-158).
//
// Prepared G2 point: the line coefficients of all 68 steps of the loop (63 doublings, 5 additions: |x| >> 1 = 0x6900800000008000 has its top
// bit at 62 and five more set bits), 68 x 3 F_p2 = 19 584 bytes, computed once per point (k_g2_prepare) and read by every check that uses it.
//
// G1 inputs stay Jacobian: a line evaluated at the affine point (X / Z^2, Y / Z^3) is scaled by Z^3, i.e. the lane uses (c2 Z^3, c1 X Z, c0 Y).
// Z^3 lies in F_p, and every factor in a proper subfield F_p^k (k | 6 or k = 4) vanishes in the final exponentiation, so no inversion per lane.
// A pair with a point at infinity on either side contributes 1 (Kilic's AddPair skips zero points).
//
// Final exponentiation: f^((p^6 - 1)(p^2 + 1)) (easy part: one F_p12 inversion and two Frobenius maps), then the hard part by the addition chain
// of the zkcrypto bls12_381 crate (cyclotomic squarings, four exponentiations by x).  That chain raises to 3 (p^4 - p^2 + 1) / r, so the whole
// map is f -> f^(3 (p^12 - 1) / r): the CUBE of the textbook reduced pairing.  gcd(3, r) = 1, so "== 1" is decided the same way;
// tests/test_pairing_host.py compares values against pow(f, 3 (p^12 - 1) / r) in tests/pairing_ref.py.
#pragma once
#include "g1.hpp"
#include "g2.hpp"

namespace kzg {

constexpr uint64_t BLS_X_ABS = 0xd201000000010000ull;
constexpr int PAIRING_LINES = 68;
struct g2_prepared {
    g2_line l[PAIRING_LINES];
    uint32_t inf, pad[3];   // 1: the point at infinity (no lines; the pair contributes 1)
};

// lines of Q (affine; `inf` for the point at infinity) in loop order
KZG_HD void g2_prepare(g2_prepared *out, const g2a &q, bool inf) {
    out->inf = inf ? 1u : 0u;
    out->pad[0] = out->pad[1] = out->pad[2] = 0;
    if (inf) return;
    g2j r; r.x = q.x; r.y = q.y; r.z = fp2_one();
    int idx = 0;
    for (int b = 61; b >= 0; b--) {   // bit 62 of |x| >> 1 is the leading one
        out->l[idx++] = g2_doubling_step(r);
        if (((BLS_X_ABS >> 1) >> b) & 1u) out->l[idx++] = g2_addition_step(r, q);
    }
    out->l[idx++] = g2_doubling_step(r);
}

// f * l(P): the line coefficients scaled by the Jacobian P's (Y, X Z, Z^3)
struct g1_line_eval { fp y, xz, z3; };
KZG_HD g1_line_eval g1_line_eval_of(const g1j &p) {
    g1_line_eval e; e.y = p.y; e.xz = mul(p.x, p.z); e.z3 = mul(sqr(p.z), p.z);
    return e;
}
KZG_HD fp12 ell(const fp12 &f, const g2_line &l, const g1_line_eval &e) {
    return fp12_mul_014(f, fp2_mul_fp(l.c2, e.z3), fp2_mul_fp(l.c1, e.xz), fp2_mul_fp(l.c0, e.y));
}

// prod_i f_{|x|, Q_i}(P_i), conjugated for the negative x.  q[i] may be shared between lanes (a broadcast read) or per lane.
template <int K> KZG_HD fp12 multi_miller_loop(const g2_prepared *const *q, const g1j *p) {
    g1_line_eval e[K];
    bool on[K];
    for (int i = 0; i < K; i++) { on[i] = !is_inf(p[i]) && q[i]->inf == 0; e[i] = g1_line_eval_of(p[i]); }
    fp12 f = fp12_one();
    int idx = 0;
    for (int b = 61; b >= 0; b--) {
        for (int i = 0; i < K; i++) if (on[i]) f = ell(f, q[i]->l[idx], e[i]);
        idx++;
        if (((BLS_X_ABS >> 1) >> b) & 1u) {
            for (int i = 0; i < K; i++) if (on[i]) f = ell(f, q[i]->l[idx], e[i]);
            idx++;
        }
        f = fp12_sqr(f);
    }
    for (int i = 0; i < K; i++) if (on[i]) f = ell(f, q[i]->l[idx], e[i]);
    return fp12_conj(f);
}

// f^x on the cyclotomic subgroup (x < 0: the conjugate of f^|x|)
KZG_TW fp12 cyc_exp_x(const fp12 &f) {
    fp12 t = fp12_one();
    bool found = false;
    for (int b = 63; b >= 0; b--) {
        if (found) t = fp12_cyc_sqr(t);
        const bool bit = (BLS_X_ABS >> b) & 1u;
        if (bit) { found = true; t = fp12_mul(t, f); }
    }
    return fp12_conj(t);
}
// f^(3 (p^12 - 1) / r), see the head of this file
KZG_HD fp12 final_exponentiation(const fp12 &f) {
    fp12 t0 = fp12_conj(f);
    fp12 t1 = fp12_inv(f);
    fp12 t2 = fp12_mul(t0, t1);          // f^(p^6 - 1)
    t1 = t2;
    t2 = fp12_mul(fp12_frob2(t2), t1);   // ^(p^2 + 1)
    t1 = fp12_conj(fp12_cyc_sqr(t2));
    fp12 t3 = cyc_exp_x(t2);
    fp12 t4 = fp12_cyc_sqr(t3);
    fp12 t5 = fp12_mul(t1, t3);
    t1 = cyc_exp_x(t5);
    t0 = cyc_exp_x(t1);
    fp12 t6 = cyc_exp_x(t0);
    t6 = fp12_mul(t6, t4);
    t4 = cyc_exp_x(t6);
    t5 = fp12_conj(t5);
    t4 = fp12_mul(t4, fp12_mul(t5, t2));
    t5 = fp12_conj(t2);
    t1 = fp12_mul(t1, t2);
    t1 = fp12_frob3(t1);
    t6 = fp12_mul(t6, t5);
    t6 = fp12_frob(t6);
    t3 = fp12_mul(t3, t0);
    t3 = fp12_frob2(t3);
    t3 = fp12_mul(t3, t1);
    t3 = fp12_mul(t3, t6);
    return fp12_mul(t3, t4);
}

// prod_i e(P_i, Q_i) == 1
template <int K> KZG_HD bool pairing_product_is_one(const g2_prepared *const *q, const g1j *p) {
    return fp12_is_one(final_exponentiation(multi_miller_loop<K>(q, p)));
}

}  // namespace kzg
