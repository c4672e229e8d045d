// tower.hpp -- the extension fields of the BLS12-381 pairing for gfx950 lanes (one element per lane), on field.hpp's F_p product.
//
//   F_p2  = F_p[u]  / (u^2 + 1)
//   F_p6  = F_p2[v] / (v^3 - xi),  xi = u + 1
//   F_p12 = F_p6[w] / (w^2 - v)
// Coordinates are F_p elements in the device-internal Montgomery domain (R' = 2^390, field.hpp), canonical (< p).  An F_p12 value is
// 12 F_p elements, 576 bytes (144 VGPRs when it lives in registers).  The heavier operations are out of line on the device (KZG_TW):
// inlined, a Miller loop plus final exponentiation would be several hundred KB of code against a 64 KB instruction cache.
// Plain C++: tests/host/pairing_emul.cpp compiles the same source for the host.
#pragma once
#include "field.hpp"

#if defined(__HIPCC__)
#define KZG_TW KZG_HD_NOINLINE static
#else
#define KZG_TW inline
#endif

namespace kzg {

struct fp2 { fp c0, c1; };
struct fp6 { fp2 c0, c1, c2; };
struct fp12 { fp6 c0, c1; };

// ---------------- F_p2 ----------------
KZG_HD fp2 fp2_zero() { fp2 o; o.c0 = zero<FpP>(); o.c1 = zero<FpP>(); return o; }
KZG_HD fp2 fp2_one() { fp2 o; o.c0 = one<FpP>(); o.c1 = zero<FpP>(); return o; }
KZG_HD bool fp2_is_zero(const fp2 &a) { return is_zero<FpP>(a.c0) && is_zero<FpP>(a.c1); }
KZG_HD bool fp2_equal(const fp2 &a, const fp2 &b) { return equal<FpP>(a.c0, b.c0) && equal<FpP>(a.c1, b.c1); }
KZG_HD fp2 fp2_add(const fp2 &a, const fp2 &b) { fp2 o; o.c0 = add(a.c0, b.c0); o.c1 = add(a.c1, b.c1); return o; }
KZG_HD fp2 fp2_sub(const fp2 &a, const fp2 &b) { fp2 o; o.c0 = sub(a.c0, b.c0); o.c1 = sub(a.c1, b.c1); return o; }
KZG_HD fp2 fp2_neg(const fp2 &a) { fp2 o; o.c0 = neg<FpP>(a.c0); o.c1 = neg<FpP>(a.c1); return o; }
KZG_HD fp2 fp2_dbl(const fp2 &a) { return fp2_add(a, a); }
KZG_HD fp2 fp2_conj(const fp2 &a) { fp2 o; o.c0 = a.c0; o.c1 = neg<FpP>(a.c1); return o; }   // = a^p
KZG_HD fp2 fp2_mul_fp(const fp2 &a, const fp &b) { fp2 o; o.c0 = mul(a.c0, b); o.c1 = mul(a.c1, b); return o; }
KZG_HD fp2 fp2_mul_xi(const fp2 &a) { fp2 o; o.c0 = sub(a.c0, a.c1); o.c1 = add(a.c0, a.c1); return o; }   // (u + 1) a
// Karatsuba: 3 F_p products
KZG_TW fp2 fp2_mul(const fp2 &a, const fp2 &b) {
    fp t0 = mul(a.c0, b.c0), t1 = mul(a.c1, b.c1);
    fp2 o;
    o.c1 = sub(sub(mul(add(a.c0, a.c1), add(b.c0, b.c1)), t0), t1);
    o.c0 = sub(t0, t1);
    return o;
}
// (a0 + a1)(a0 - a1) + 2 a0 a1 u: 2 F_p products
KZG_TW fp2 fp2_sqr(const fp2 &a) {
    fp2 o;
    fp t = mul(a.c0, a.c1);
    o.c0 = mul(add(a.c0, a.c1), sub(a.c0, a.c1));
    o.c1 = add(t, t);
    return o;
}
// conj(a) / (a0^2 + a1^2): the one F_p inversion (field.hpp inv); 0 -> 0
KZG_TW fp2 fp2_inv(const fp2 &a) {
    fp t = inv<FpP>(add(sqr(a.c0), sqr(a.c1)));
    fp2 o; o.c0 = mul(a.c0, t); o.c1 = neg<FpP>(mul(a.c1, t));
    return o;
}

// ---------------- F_p6 ----------------
KZG_HD fp6 fp6_zero() { fp6 o; o.c0 = fp2_zero(); o.c1 = fp2_zero(); o.c2 = fp2_zero(); return o; }
KZG_HD fp6 fp6_one() { fp6 o; o.c0 = fp2_one(); o.c1 = fp2_zero(); o.c2 = fp2_zero(); return o; }
KZG_HD bool fp6_equal(const fp6 &a, const fp6 &b) { return fp2_equal(a.c0, b.c0) && fp2_equal(a.c1, b.c1) && fp2_equal(a.c2, b.c2); }
KZG_HD fp6 fp6_add(const fp6 &a, const fp6 &b) { fp6 o; o.c0 = fp2_add(a.c0, b.c0); o.c1 = fp2_add(a.c1, b.c1); o.c2 = fp2_add(a.c2, b.c2); return o; }
KZG_HD fp6 fp6_sub(const fp6 &a, const fp6 &b) { fp6 o; o.c0 = fp2_sub(a.c0, b.c0); o.c1 = fp2_sub(a.c1, b.c1); o.c2 = fp2_sub(a.c2, b.c2); return o; }
KZG_HD fp6 fp6_neg(const fp6 &a) { fp6 o; o.c0 = fp2_neg(a.c0); o.c1 = fp2_neg(a.c1); o.c2 = fp2_neg(a.c2); return o; }
KZG_HD fp6 fp6_mul_v(const fp6 &a) { fp6 o; o.c0 = fp2_mul_xi(a.c2); o.c1 = a.c0; o.c2 = a.c1; return o; }   // v a
// Karatsuba over the three coefficients: 6 F_p2 products
KZG_TW fp6 fp6_mul(const fp6 &a, const fp6 &b) {
    fp2 t0 = fp2_mul(a.c0, b.c0), t1 = fp2_mul(a.c1, b.c1), t2 = fp2_mul(a.c2, b.c2);
    fp6 o;
    o.c0 = fp2_add(fp2_mul_xi(fp2_sub(fp2_sub(fp2_mul(fp2_add(a.c1, a.c2), fp2_add(b.c1, b.c2)), t1), t2)), t0);
    o.c1 = fp2_add(fp2_sub(fp2_sub(fp2_mul(fp2_add(a.c0, a.c1), fp2_add(b.c0, b.c1)), t0), t1), fp2_mul_xi(t2));
    o.c2 = fp2_add(fp2_sub(fp2_sub(fp2_mul(fp2_add(a.c0, a.c2), fp2_add(b.c0, b.c2)), t0), t2), t1);
    return o;
}
KZG_HD fp6 fp6_sqr(const fp6 &a) { return fp6_mul(a, a); }
KZG_TW fp6 fp6_inv(const fp6 &a) {
    fp2 c0 = fp2_sub(fp2_sqr(a.c0), fp2_mul_xi(fp2_mul(a.c1, a.c2)));
    fp2 c1 = fp2_sub(fp2_mul_xi(fp2_sqr(a.c2)), fp2_mul(a.c0, a.c1));
    fp2 c2 = fp2_sub(fp2_sqr(a.c1), fp2_mul(a.c0, a.c2));
    fp2 t = fp2_add(fp2_mul(a.c0, c0), fp2_mul_xi(fp2_add(fp2_mul(a.c2, c1), fp2_mul(a.c1, c2))));
    t = fp2_inv(t);
    fp6 o; o.c0 = fp2_mul(c0, t); o.c1 = fp2_mul(c1, t); o.c2 = fp2_mul(c2, t);
    return o;
}
// a * (b0 + b1 v): 5 F_p2 products (the line's F_p6 half, see fp12_mul_014)
KZG_TW fp6 fp6_mul_01(const fp6 &a, const fp2 &b0, const fp2 &b1) {
    fp2 aa = fp2_mul(a.c0, b0), bb = fp2_mul(a.c1, b1);
    fp6 o;
    o.c0 = fp2_add(fp2_mul_xi(fp2_mul(a.c2, b1)), aa);
    o.c1 = fp2_sub(fp2_sub(fp2_mul(fp2_add(b0, b1), fp2_add(a.c0, a.c1)), aa), bb);
    o.c2 = fp2_add(fp2_mul(a.c2, b0), bb);
    return o;
}
// a * (b1 v): 3 F_p2 products
KZG_HD fp6 fp6_mul_1(const fp6 &a, const fp2 &b1) {
    fp6 o; o.c0 = fp2_mul_xi(fp2_mul(a.c2, b1)); o.c1 = fp2_mul(a.c0, b1); o.c2 = fp2_mul(a.c1, b1);
    return o;
}

// ---------------- Frobenius constants ----------------
// gamma_k = xi^((p - 1) / k), radix-2^390 Montgomery images (value * 2^390 mod p, 12 little-endian u32 limbs), generated by
//   python3 -c "import tests.pairing_ref as r; print(r.f2pow((1, 1), (r.P - 1) // k))"   for k = 3 (v^p = gamma_3 v), 3/2 (v^2p = gamma_3^2 v^2)
//   and 6 (w^p = gamma_6 w), then * 2^390 mod p.  tests/test_pairing_host.py checks every Frobenius map against a^p computed by pow.
KZG_HD fp fp_const(const uint32_t *t) { fp o; for (int i = 0; i < 12; i++) o.l[i] = t[i]; return o; }
KZG_HD fp2 frob_gamma(int k) {   // 0: gamma_3 = xi^((p-1)/3) = (0, c), 1: gamma_3^2 = xi^(2(p-1)/3) = (c', 0), 2: gamma_6 = xi^((p-1)/6)
    const uint32_t g31[12] = {0x9c907181u, 0xef2f7921u, 0xb26574c3u, 0x1bcc91d7u, 0x191c3ebcu, 0x856e7b9au,
                              0x67fd6ffau, 0xbd16b0d2u, 0xeb0c0550u, 0x18c86532u, 0x6567dd7du, 0x09c6d485u};
    const uint32_t g32[12] = {0x9d6270afu, 0x35a57921u, 0x4dad7570u, 0xa084950fu, 0x019e81d8u, 0x9348237bu,
                              0x1e814cf2u, 0x7f82d7a3u, 0x4ed0ab3fu, 0x42b9aaa9u, 0xe4a65dc8u, 0x0b24be1bu};
    const uint32_t g60[12] = {0xc67c6e8eu, 0xc63b54acu, 0x0568c4c7u, 0xf78fe4cau, 0x12937cd6u, 0x1bdd195fu,
                              0xc99adf33u, 0x34ab353fu, 0xa232b8e6u, 0xc48490edu, 0x4ddbe984u, 0x0070f9cbu};
    const uint32_t g61[12] = {0x39833c1du, 0xf3c3ab53u, 0xabeb3b37u, 0x271c1b34u, 0xe41d794du, 0x4b53b941u,
                              0x29ea338cu, 0x2fcc1645u, 0xa118f3f1u, 0x869716c8u, 0xeba3fd15u, 0x1990181eu};
    fp2 o;
    if (k == 0) { o.c0 = zero<FpP>(); o.c1 = fp_const(g31); }
    else if (k == 1) { o.c0 = fp_const(g32); o.c1 = zero<FpP>(); }
    else { o.c0 = fp_const(g60); o.c1 = fp_const(g61); }
    return o;
}
KZG_HD fp6 fp6_frob(const fp6 &a) {   // a^p
    fp6 o;
    o.c0 = fp2_conj(a.c0);
    o.c1 = fp2_mul(fp2_conj(a.c1), frob_gamma(0));
    o.c2 = fp2_mul(fp2_conj(a.c2), frob_gamma(1));
    return o;
}

// ---------------- F_p12 ----------------
KZG_HD fp12 fp12_one() { fp12 o; o.c0 = fp6_one(); o.c1 = fp6_zero(); return o; }
KZG_HD bool fp12_equal(const fp12 &a, const fp12 &b) { return fp6_equal(a.c0, b.c0) && fp6_equal(a.c1, b.c1); }
KZG_HD bool fp12_is_one(const fp12 &a) { return fp12_equal(a, fp12_one()); }
KZG_HD fp12 fp12_conj(const fp12 &a) { fp12 o; o.c0 = a.c0; o.c1 = fp6_neg(a.c1); return o; }   // = a^(p^6); the inverse on the cyclotomic subgroup
// Karatsuba: 3 F_p6 products (54 F_p products)
KZG_TW fp12 fp12_mul(const fp12 &a, const fp12 &b) {
    fp6 aa = fp6_mul(a.c0, b.c0), bb = fp6_mul(a.c1, b.c1);
    fp12 o;
    o.c1 = fp6_sub(fp6_sub(fp6_mul(fp6_add(a.c0, a.c1), fp6_add(b.c0, b.c1)), aa), bb);
    o.c0 = fp6_add(fp6_mul_v(bb), aa);
    return o;
}
// complex squaring: 2 F_p6 products
KZG_TW fp12 fp12_sqr(const fp12 &a) {
    fp6 ab = fp6_mul(a.c0, a.c1);
    fp12 o;
    o.c0 = fp6_sub(fp6_sub(fp6_mul(fp6_add(a.c0, a.c1), fp6_add(a.c0, fp6_mul_v(a.c1))), ab), fp6_mul_v(ab));
    o.c1 = fp6_add(ab, ab);
    return o;
}
KZG_TW fp12 fp12_inv(const fp12 &a) {   // one F_p inversion (inside fp6_inv -> fp2_inv)
    fp6 t = fp6_inv(fp6_sub(fp6_sqr(a.c0), fp6_mul_v(fp6_sqr(a.c1))));
    fp12 o; o.c0 = fp6_mul(a.c0, t); o.c1 = fp6_neg(fp6_mul(a.c1, t));
    return o;
}
KZG_TW fp12 fp12_frob(const fp12 &a) {   // a^p
    fp12 o;
    o.c0 = fp6_frob(a.c0);
    fp6 t = fp6_frob(a.c1);
    const fp2 g = frob_gamma(2);
    o.c1.c0 = fp2_mul(t.c0, g); o.c1.c1 = fp2_mul(t.c1, g); o.c1.c2 = fp2_mul(t.c2, g);
    return o;
}
KZG_HD fp12 fp12_frob2(const fp12 &a) { return fp12_frob(fp12_frob(a)); }                 // a^(p^2)
KZG_HD fp12 fp12_frob3(const fp12 &a) { return fp12_frob(fp12_frob(fp12_frob(a))); }      // a^(p^3)
// f * (c0 + c1 v + c4 v w): a line value (pairing.hpp) times the accumulator, 13 F_p2 products instead of 18
KZG_TW fp12 fp12_mul_014(const fp12 &f, const fp2 &c0, const fp2 &c1, const fp2 &c4) {
    fp6 aa = fp6_mul_01(f.c0, c0, c1);
    fp6 bb = fp6_mul_1(f.c1, c4);
    fp12 o;
    o.c1 = fp6_sub(fp6_sub(fp6_mul_01(fp6_add(f.c1, f.c0), c0, fp2_add(c1, c4)), aa), bb);
    o.c0 = fp6_add(fp6_mul_v(bb), aa);
    return o;
}
// Granger-Scott squaring on the cyclotomic subgroup (a^(p^6 + 1) = 1, i.e. after the easy part of the final exponentiation): three F_p4
// squarings, 6 F_p2 squarings in all instead of the 12 F_p2 products of fp12_sqr.  Wrong for other elements.
KZG_HD void fp4_sqr(fp2 &o0, fp2 &o1, const fp2 &a, const fp2 &b) {
    fp2 t0 = fp2_sqr(a), t1 = fp2_sqr(b);
    o0 = fp2_add(fp2_mul_xi(t1), t0);
    o1 = fp2_sub(fp2_sub(fp2_sqr(fp2_add(a, b)), t0), t1);
}
KZG_TW fp12 fp12_cyc_sqr(const fp12 &f) {
    fp2 z0 = f.c0.c0, z4 = f.c0.c1, z3 = f.c0.c2, z2 = f.c1.c0, z1 = f.c1.c1, z5 = f.c1.c2;
    fp2 t0, t1, t2, t3;
    fp4_sqr(t0, t1, z0, z1);
    z0 = fp2_sub(t0, z0); z0 = fp2_add(fp2_dbl(z0), t0);
    z1 = fp2_add(t1, z1); z1 = fp2_add(fp2_dbl(z1), t1);
    fp4_sqr(t0, t1, z2, z3);
    fp4_sqr(t2, t3, z4, z5);
    z4 = fp2_sub(t0, z4); z4 = fp2_add(fp2_dbl(z4), t0);
    z5 = fp2_add(t1, z5); z5 = fp2_add(fp2_dbl(z5), t1);
    t0 = fp2_mul_xi(t3);
    z2 = fp2_add(t0, z2); z2 = fp2_add(fp2_dbl(z2), t0);
    z3 = fp2_sub(t2, z3); z3 = fp2_add(fp2_dbl(z3), t2);
    fp12 o;
    o.c0.c0 = z0; o.c0.c1 = z4; o.c0.c2 = z3; o.c1.c0 = z2; o.c1.c1 = z1; o.c1.c2 = z5;
    return o;
}

}  // namespace kzg
