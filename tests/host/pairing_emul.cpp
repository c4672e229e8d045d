// Host build of tower.hpp / g2.hpp / pairing.hpp for tests/test_pairing_host.py.  Every F_p value crosses this boundary in STANDARD form
// (12 little-endian u32 limbs, < p); F_p12 values as 12 such elements in the order c0.c0.c0, c0.c0.c1, c0.c1.c0, ..., c1.c2.c1.
#include "pairing.hpp"

using namespace kzg;

static fp in_fp(const uint32_t *s) { fp a; for (int i = 0; i < 12; i++) a.l[i] = s[i]; return to_mont<FpP>(a); }
static void out_fp(uint32_t *d, const fp &a) { fp s = from_mont<FpP>(a); for (int i = 0; i < 12; i++) d[i] = s.l[i]; }
static fp2 in_fp2(const uint32_t *s) { fp2 a; a.c0 = in_fp(s); a.c1 = in_fp(s + 12); return a; }
static void out_fp2(uint32_t *d, const fp2 &a) { out_fp(d, a.c0); out_fp(d + 12, a.c1); }
static fp12 in_fp12(const uint32_t *s) {
    fp12 a;
    fp2 *c[6] = {&a.c0.c0, &a.c0.c1, &a.c0.c2, &a.c1.c0, &a.c1.c1, &a.c1.c2};
    for (int k = 0; k < 6; k++) *c[k] = in_fp2(s + 24 * k);
    return a;
}
static void out_fp12(uint32_t *d, const fp12 &a) {
    const fp2 *c[6] = {&a.c0.c0, &a.c0.c1, &a.c0.c2, &a.c1.c0, &a.c1.c1, &a.c1.c2};
    for (int k = 0; k < 6; k++) out_fp2(d + 24 * k, *c[k]);
}

extern "C" {
// op: 0 mul, 1 sqr, 2 inv, 3 frob, 4 frob2, 5 frob3, 6 cyclotomic sqr, 7 conj, 8 mul_014 (b holds c0, c1, c4 as its first three F_p2)
void pe_fp12_op(int op, const uint32_t *a, const uint32_t *b, uint32_t *out) {
    fp12 x = in_fp12(a), r;
    switch (op) {
    case 0: r = fp12_mul(x, in_fp12(b)); break;
    case 1: r = fp12_sqr(x); break;
    case 2: r = fp12_inv(x); break;
    case 3: r = fp12_frob(x); break;
    case 4: r = fp12_frob2(x); break;
    case 5: r = fp12_frob3(x); break;
    case 6: r = fp12_cyc_sqr(x); break;
    case 7: r = fp12_conj(x); break;
    default: r = fp12_mul_014(x, in_fp2(b), in_fp2(b + 24), in_fp2(b + 48)); break;
    }
    out_fp12(out, r);
}
// 1 and the affine point (x0, x1, y0, y1; all zero for infinity) when the encoding is valid, 0 otherwise
int pe_g2_decompress(const uint8_t *in96, uint32_t *out) {
    g2j p;
    if (!g2_decompress(p, in96)) return 0;
    g2a a = g2_to_affine(p);
    out_fp2(out, a.x); out_fp2(out + 24, a.y);
    return 1;
}
// final_exponentiation(multi_miller_loop(pairs)): g1 = n x (X, Y, Z) Jacobian (Z = 0: infinity), g2 = n x (x0, x1, y0, y1, inf flag in limb 0 of
// a 13th element) affine
void pe_pairing(uint64_t n, const uint32_t *g1, const uint32_t *g2, uint32_t *out) {
    fp12 f = fp12_one();
    for (uint64_t i = 0; i < n; i++) {
        g1j p; p.x = in_fp(g1 + 36 * i); p.y = in_fp(g1 + 36 * i + 12); p.z = in_fp(g1 + 36 * i + 24);
        g2a q; q.x = in_fp2(g2 + 60 * i); q.y = in_fp2(g2 + 60 * i + 24);
        static g2_prepared prep;
        g2_prepare(&prep, q, g2[60 * i + 48] != 0);
        const g2_prepared *qs[1] = {&prep};
        f = fp12_mul(f, multi_miller_loop<1>(qs, &p));
    }
    out_fp12(out, final_exponentiation(f));
}
// the two-pair form the kernels run: 1 when e(P0, Q0) e(P1, Q1) == 1
int pe_pairing_check2(const uint32_t *g1, const uint32_t *g2) {
    static g2_prepared prep[2];
    g1j p[2];
    for (int i = 0; i < 2; i++) {
        p[i].x = in_fp(g1 + 36 * i); p[i].y = in_fp(g1 + 36 * i + 12); p[i].z = in_fp(g1 + 36 * i + 24);
        g2a q; q.x = in_fp2(g2 + 60 * i); q.y = in_fp2(g2 + 60 * i + 24);
        g2_prepare(&prep[i], q, g2[60 * i + 48] != 0);
    }
    const g2_prepared *qs[2] = {&prep[0], &prep[1]};
    return pairing_product_is_one<2>(qs, p) ? 1 : 0;
}
}
