// g2.hpp -- the BLS12-381 G2 group for gfx950 lanes (one point per lane): the twist E': y^2 = x^3 + 4 (u + 1) over F_p2 (tower.hpp).
//
// Replaces what verification needs of Kilic's G2 (bls.FromCompressedG2, bls.PairingsVerify's point handling, bls/bls_kilic.go): Jacobian
// (X, Y, Z) with coordinates in the device-internal Montgomery domain, inf <=> Z == 0; the ZCash 96-byte decompression with every check
// Kilic makes; and the two Miller-loop steps that turn a running point into line coefficients (pairing.hpp prepares a G2 point with them).
// The C ABI's G2 image is Kilic's (3 x 2 x 6 u64, Montgomery R = 2^384): g2_from_kilic / g2_to_kilic convert at the boundary.
#pragma once
#include "tower.hpp"
#include "g1.hpp"

namespace kzg {

struct g2j { fp2 x, y, z; };   // Jacobian, 288 B (= bls.G2Point)
struct g2a { fp2 x, y; };      // affine

KZG_HD bool is_inf(const g2j &p) { return fp2_is_zero(p.z); }
KZG_HD g2j g2_inf() { g2j o; o.x = fp2_zero(); o.y = fp2_one(); o.z = fp2_zero(); return o; }
KZG_HD g2j g2_neg(const g2j &p) { g2j o = p; o.y = fp2_neg(p.y); return o; }
KZG_HD fp2 g2_b() { fp f = one<FpP>(); f = add(f, f); f = add(f, f); fp2 o; o.c0 = f; o.c1 = f; return o; }   // 4 (u + 1)
KZG_HD g2j g2_generator() {   // bls.GenG2: the standard generator (the first setup_G2 entry of eth/trusted_setup.json)
    const uint32_t x0[12] = {0xc121bdb8u, 0xd48056c8u, 0xa805bbefu, 0x0bac0326u, 0x7ae3d177u, 0xb4510b64u, 0xfa403b02u, 0xc6e47ad4u, 0x2dc51051u, 0x26080527u, 0xf08f0a91u, 0x024aa2b2u};
    const uint32_t x1[12] = {0x5d042b7eu, 0xe5ac7d05u, 0x13945d57u, 0x334cf112u, 0xdc7f5049u, 0xb5da61bbu, 0x9920b61au, 0x596bd0d0u, 0x88274f65u, 0x7dacd3a0u, 0x52719f60u, 0x13e02b60u};
    const uint32_t y0[12] = {0x08b82801u, 0xe1935486u, 0x3baca289u, 0x923ac9ccu, 0x5160d12cu, 0x6d429a69u, 0x8cbdd3a7u, 0xadfd9baau, 0xda2e351au, 0x8cc9cdc6u, 0x727d6e11u, 0x0ce5d527u};
    const uint32_t y1[12] = {0xf05f79beu, 0xaaa9075fu, 0x5cec1da1u, 0x3f370d27u, 0x572e99abu, 0x267492abu, 0x85a763afu, 0xcb3e287eu, 0x2bc28b99u, 0x32acd2b0u, 0x2ea734ccu, 0x0606c4a0u};
    g2j o;   // standard-form literals, into the Montgomery domain
    o.x.c0 = to_mont<FpP>(fp_const(x0)); o.x.c1 = to_mont<FpP>(fp_const(x1));
    o.y.c0 = to_mont<FpP>(fp_const(y0)); o.y.c1 = to_mont<FpP>(fp_const(y1));
    o.z = fp2_one();
    return o;
}

// dbl-2009-l (a = 0), as g1_dbl
KZG_TW g2j g2_dbl(const g2j &p) {
    if (is_inf(p)) return g2_inf();
    fp2 a = fp2_sqr(p.x), b = fp2_sqr(p.y), c = fp2_sqr(b);
    fp2 d = fp2_sub(fp2_sub(fp2_sqr(fp2_add(p.x, b)), a), c); d = fp2_dbl(d);
    fp2 e = fp2_add(fp2_dbl(a), a);
    g2j o;
    o.x = fp2_sub(fp2_sqr(e), fp2_dbl(d));
    o.z = fp2_dbl(fp2_mul(p.y, p.z));
    fp2 c8 = fp2_dbl(fp2_dbl(fp2_dbl(c)));
    o.y = fp2_sub(fp2_mul(e, fp2_sub(d, o.x)), c8);
    return o;
}
// add-2007-bl, exceptional cases handled (P == Q doubles, P == -Q gives inf), as g1_add
KZG_TW g2j g2_add(const g2j &p, const g2j &q) {
    if (is_inf(p)) return q;
    if (is_inf(q)) return p;
    fp2 z1z1 = fp2_sqr(p.z), z2z2 = fp2_sqr(q.z);
    fp2 u1 = fp2_mul(p.x, z2z2), u2 = fp2_mul(q.x, z1z1);
    fp2 s1 = fp2_mul(fp2_mul(p.y, q.z), z2z2), s2 = fp2_mul(fp2_mul(q.y, p.z), z1z1);
    if (fp2_equal(u1, u2)) {
        if (fp2_equal(s1, s2)) return g2_dbl(p);
        return g2_inf();
    }
    fp2 h = fp2_sub(u2, u1);
    fp2 i = fp2_sqr(fp2_dbl(h));
    fp2 j = fp2_mul(h, i);
    fp2 r = fp2_dbl(fp2_sub(s2, s1));
    fp2 v = fp2_mul(u1, i);
    g2j o;
    o.x = fp2_sub(fp2_sub(fp2_sub(fp2_sqr(r), j), v), v);
    o.y = fp2_sub(fp2_mul(r, fp2_sub(v, o.x)), fp2_dbl(fp2_mul(s1, j)));
    o.z = fp2_mul(fp2_sub(fp2_sub(fp2_sqr(fp2_add(p.z, q.z)), z1z1), z2z2), h);
    return o;
}
// An affine "no point": (0, 0) is not on the twist (b != 0) and is what g2_to_affine returns for infinity; a table entry of that form adds nothing
KZG_HD bool g2a_is_none(const g2a &q) { return fp2_is_zero(q.x) && fp2_is_zero(q.y); }
// madd-2007-bl over F_p2 (Jacobian + affine: 7 products and 4 squarings against the 11 + 5 of g2_add), exceptional cases handled as in g2_add:
// Q "no point" returns P, P at infinity returns Q, P == Q doubles, P == -Q gives infinity
KZG_TW g2j g2_add_mixed(const g2j &p, const g2a &q) {
    if (g2a_is_none(q)) return p;
    if (is_inf(p)) { g2j o; o.x = q.x; o.y = q.y; o.z = fp2_one(); return o; }
    fp2 z1z1 = fp2_sqr(p.z);
    fp2 u2 = fp2_mul(q.x, z1z1), s2 = fp2_mul(fp2_mul(q.y, p.z), z1z1);
    if (fp2_equal(u2, p.x)) {
        if (fp2_equal(s2, p.y)) return g2_dbl(p);
        return g2_inf();
    }
    fp2 h = fp2_sub(u2, p.x), hh = fp2_sqr(h);
    fp2 i = fp2_dbl(fp2_dbl(hh));
    fp2 j = fp2_mul(h, i);
    fp2 r = fp2_dbl(fp2_sub(s2, p.y));
    fp2 v = fp2_mul(p.x, i);
    g2j o;
    o.x = fp2_sub(fp2_sub(fp2_sub(fp2_sqr(r), j), v), v);
    o.y = fp2_sub(fp2_mul(r, fp2_sub(v, o.x)), fp2_dbl(fp2_mul(p.y, j)));
    o.z = fp2_sub(fp2_sub(fp2_sqr(fp2_add(p.z, h)), z1z1), hh);
    return o;
}
// k P for a standard-form scalar of `words` u32 limbs, MSB first, bitwise (setup and subgroup checks only)
KZG_HD g2j g2_mul_bits(const g2j &p, const uint32_t *k, int words) {
    g2j acc = g2_inf();
    for (int i = 32 * words - 1; i >= 0; i--) {
        acc = g2_dbl(acc);
        if ((k[i >> 5] >> (i & 31)) & 1u) acc = g2_add(acc, p);
    }
    return acc;
}
KZG_HD bool g2_in_subgroup(const g2j &p) {   // [r]P == inf (Kilic G2.InCorrectSubgroup)
    uint32_t r[8];
    for (int i = 0; i < 8; i++) r[i] = FrP::mod(i);
    return is_inf(g2_mul_bits(p, r, 8));
}
KZG_HD bool g2_equal(const g2j &p, const g2j &q) {
    bool pi = is_inf(p), qi = is_inf(q);
    if (pi || qi) return pi && qi;
    fp2 z1z1 = fp2_sqr(p.z), z2z2 = fp2_sqr(q.z);
    if (!fp2_equal(fp2_mul(p.x, z2z2), fp2_mul(q.x, z1z1))) return false;
    return fp2_equal(fp2_mul(fp2_mul(p.y, q.z), z2z2), fp2_mul(fp2_mul(q.y, p.z), z1z1));
}
KZG_HD g2a g2_to_affine(const g2j &p) {   // one F_p inversion; inf -> (0, 0)
    g2a o;
    if (is_inf(p)) { o.x = fp2_zero(); o.y = fp2_zero(); return o; }
    fp2 zi = fp2_inv(p.z), zi2 = fp2_sqr(zi);
    o.x = fp2_mul(p.x, zi2); o.y = fp2_mul(p.y, fp2_mul(zi2, zi));
    return o;
}
KZG_HD bool g2a_on_curve(const g2a &p) { return fp2_equal(fp2_sqr(p.y), fp2_add(fp2_mul(fp2_sqr(p.x), p.x), g2_b())); }

// Kilic image (R = 2^384) <-> device-internal image (R' = 2^390)
KZG_HD fp2 fp2_from_kilic(const fp2 &a) { fp2 o; o.c0 = fp_from_kilic(a.c0); o.c1 = fp_from_kilic(a.c1); return o; }
KZG_HD fp2 fp2_to_kilic(const fp2 &a) { fp2 o; o.c0 = fp_to_kilic(a.c0); o.c1 = fp_to_kilic(a.c1); return o; }
KZG_HD g2j g2_from_kilic(const g2j &p) {
    if (fp2_is_zero(p.z)) return g2_inf();
    g2j o; o.x = fp2_from_kilic(p.x); o.y = fp2_from_kilic(p.y); o.z = fp2_from_kilic(p.z);
    return o;
}
KZG_HD g2j g2_to_kilic(const g2j &p) {
    g2j o;
    if (is_inf(p)) { o.x = fp2_zero(); o.y.c0 = fp_kilic_one(); o.y.c1 = zero<FpP>(); o.z = fp2_zero(); return o; }   // Kilic Zero(): (0, 1, 0)
    o.x = fp2_to_kilic(p.x); o.y = fp2_to_kilic(p.y); o.z = fp2_to_kilic(p.z);
    return o;
}

// ---------------- ZCash decompression ----------------
// a^e for e = (p - sub) >> shift (the square-root exponents), square-and-multiply over the 381 bits
KZG_HD fp2 fp2_pow_pm(const fp2 &a, uint32_t sub, int shift) {
    uint32_t e[12]; uint32_t br = 0;
    for (int i = 0; i < 12; i++) e[i] = subb(FpP::mod(i), i == 0 ? sub : 0u, br);
    for (int i = 0; i < 12; i++) e[i] = (e[i] >> shift) | (i < 11 ? e[i + 1] << (32 - shift) : 0u);
    fp2 acc = fp2_one();
    for (int i = 380; i >= 0; i--) {
        acc = fp2_sqr(acc);
        if ((e[i >> 5] >> (i & 31)) & 1u) acc = fp2_mul(acc, a);
    }
    return acc;
}
// a square root of a (p = 3 mod 4: Algorithm 9 of Adj, Rodriguez-Henriquez, ePrint 2012/685); false when a is not a square
KZG_HD bool fp2_sqrt(fp2 &out, const fp2 &a) {
    fp2 a1 = fp2_pow_pm(a, 3, 2);                       // a^((p - 3) / 4)
    fp2 alpha = fp2_mul(fp2_sqr(a1), a);                // a^((p - 1) / 2)
    fp2 x0 = fp2_mul(a1, a);                            // a^((p + 1) / 4)
    fp2 x;
    if (fp2_equal(alpha, fp2_neg(fp2_one()))) { x.c0 = neg<FpP>(x0.c1); x.c1 = x0.c0; }   // u x0
    else x = fp2_mul(fp2_pow_pm(fp2_add(fp2_one(), alpha), 1, 1), x0);                     // (1 + alpha)^((p - 1) / 2) x0
    out = x;
    return fp2_equal(fp2_sqr(x), a);
}
KZG_HD bool fp2_lex_larger(const fp2 &y) {   // ZCash sort flag of a G2 y: c1 decides, c0 when c1 == 0
    fp y0 = from_mont<FpP>(y.c0), y1 = from_mont<FpP>(y.c1);
    return is_zero<FpP>(y1) ? fp_std_gt_half(y0) : fp_std_gt_half(y1);
}
// bls.FromCompressedG2 (Kilic G2.FromCompressed): x = x1 u + x0 stored as x1 || x0, flags in the top three bits of byte 0.  Returns false for
// a missing compression flag, a malformed infinity, a coordinate >= p, an x with no point on the curve, or a point outside the subgroup.
KZG_HD bool g2_decompress(g2j &out, const uint8_t *b) {
    const uint8_t f = b[0];
    out = g2_inf();
    if (!(f & 0x80)) return false;
    if (f & 0x40) {
        uint32_t rest = f & 0x3f;
        for (int i = 1; i < 96; i++) rest |= b[i];
        return rest == 0;
    }
    fp2 x;
    if (!fp_from_be48(x.c1, b, true) || !fp_from_be48(x.c0, b + 48, false)) return false;
    x.c0 = to_mont<FpP>(x.c0); x.c1 = to_mont<FpP>(x.c1);
    fp2 y;
    if (!fp2_sqrt(y, fp2_add(fp2_mul(fp2_sqr(x), x), g2_b()))) return false;
    if (fp2_lex_larger(y) != ((f & 0x20) != 0)) y = fp2_neg(y);
    g2j p; p.x = x; p.y = y; p.z = fp2_one();
    if (!g2_in_subgroup(p)) return false;
    out = p;
    return true;
}

// bls.ToCompressedG2 (Kilic G2.ToCompressed), the exact inverse of g2_decompress: x.c1 || x.c0 big-endian, 0x80 set, 0x20 from fp2_lex_larger(y),
// c0 00 .. 00 for infinity.  Device-internal image in, any Z (one F_p inversion when Z != 1).
KZG_HD void fp_to_be48(uint8_t *o, const fp &std) {
    for (int i = 0; i < 48; i++) o[47 - i] = (uint8_t)(std.l[i >> 2] >> (8 * (i & 3)));
}
KZG_HD void g2_compress(uint8_t *o, const g2j &p) {
    if (is_inf(p)) {
        o[0] = 0xc0;
        for (int i = 1; i < 96; i++) o[i] = 0;
        return;
    }
    g2a a;
    if (fp2_equal(p.z, fp2_one())) { a.x = p.x; a.y = p.y; }
    else a = g2_to_affine(p);
    fp_to_be48(o, from_mont<FpP>(a.x.c1));
    fp_to_be48(o + 48, from_mont<FpP>(a.x.c0));
    o[0] |= 0x80 | (fp2_lex_larger(a.y) ? 0x20 : 0);
}
// the API's output form of a G2 result: Kilic image with Z = 1, infinity as Kilic's Zero() (0, 1, 0); one F_p inversion
KZG_HD g2j g2_normalize_to_kilic(const g2j &p) {
    if (is_inf(p)) return g2_to_kilic(g2_inf());
    const g2a a = g2_to_affine(p);
    g2j o; o.x = a.x; o.y = a.y; o.z = fp2_one();
    return g2_to_kilic(o);
}

// ---------------- fixed-base multiplication of bls.GenG2 ----------------
// T[w][d] = [d 2^(8 w)] G2 for w = 0..31, d = 0..255, affine, device-internal Montgomery domain; T[w][0] is the "no point" entry.  UNSIGNED 8-bit
// windows: a digit is a byte of the standard-form scalar, a row is indexed by it without a branch or a negation, and 32 x 256 x 192 B = 1.5 MiB
// stays resident in the L2.  A multiplication is 32 mixed additions and no doubling (g2_mul_bits: 255 doublings and ~127 full additions).
constexpr int G2_FB_C = 8, G2_FB_WINDOWS = 32, G2_FB_ROW = 1 << G2_FB_C;
constexpr uint64_t G2_FB_ENTRIES = (uint64_t)G2_FB_WINDOWS * G2_FB_ROW;
KZG_HD uint32_t g2_fb_digit(const fr &k_std, int w) { return (k_std.l[w >> 2] >> (8 * (w & 3))) & 0xffu; }   // digit w of a STANDARD-form scalar
KZG_HD g2j g2_fb_window_base(int w) {   // [2^(8 w)] G2
    g2j b = g2_generator();
    for (int i = 0; i < G2_FB_C * w; i++) b = g2_dbl(b);
    return b;
}
KZG_HD g2a g2_fb_entry(const g2j &base, uint32_t d) {   // [d] base, d < 256; d == 0: "no point"
    g2j acc = g2_inf();
    for (int i = G2_FB_C - 1; i >= 0; i--) {
        acc = g2_dbl(acc);
        if ((d >> i) & 1u) acc = g2_add(acc, base);
    }
    return g2_to_affine(acc);
}
// [k] G2 for a Montgomery-form scalar k < r: the scalar leaves the Montgomery domain once and is cut into bytes.  No partial sum meets an
// exceptional case of the addition: after windows 0 .. w - 1 the sum is [k mod 2^(8 w)] G2, a multiple below 2^(8 w), and the next entry is
// [d 2^(8 w)] G2 with d >= 1, a larger multiple, so the two differ; their sum is [k mod 2^(8 w + 8)] G2 with 0 < k mod 2^(8 w + 8) <= k < r, so
// they are not opposite either.  (Only the first non-zero digit meets the accumulator at infinity.)  The complete addition is called anyway.
KZG_HD g2j g2_fb_mul(const g2a *table, const fr &k_mont) {
    const fr k = from_mont<FrP>(k_mont);
    g2j acc = g2_inf();
    for (int w = 0; w < G2_FB_WINDOWS; w++) acc = g2_add_mixed(acc, table[(uint64_t)w * G2_FB_ROW + g2_fb_digit(k, w)]);
    return acc;
}

// ---------------- Miller-loop steps ----------------
// Line coefficients (c0, c1, c2) of the optimal ate loop on a Jacobian running point r and an affine Q (Costello, Lange, Naehrig, "Faster pairing
// computations on curves with high-degree twists", ePrint 2010/354, Algorithms 26 and 27, as restated by the zkcrypto bls12_381 crate).
// pairing.hpp evaluates a line at P = (x, y) as the sparse element c2 + (c1 x) v + (c0 y) v w of F_p12.
struct g2_line { fp2 c0, c1, c2; };
KZG_TW g2_line g2_doubling_step(g2j &r) {
    fp2 t0 = fp2_sqr(r.x), t1 = fp2_sqr(r.y), t2 = fp2_sqr(t1);
    fp2 t3 = fp2_sub(fp2_sub(fp2_sqr(fp2_add(t1, r.x)), t0), t2); t3 = fp2_dbl(t3);
    fp2 t4 = fp2_add(fp2_dbl(t0), t0);
    fp2 t6 = fp2_add(r.x, t4);
    fp2 t5 = fp2_sqr(t4);
    fp2 zz = fp2_sqr(r.z);
    r.x = fp2_sub(fp2_sub(t5, t3), t3);
    r.z = fp2_sub(fp2_sub(fp2_sqr(fp2_add(r.z, r.y)), t1), zz);
    r.y = fp2_sub(fp2_mul(fp2_sub(t3, r.x), t4), fp2_dbl(fp2_dbl(fp2_dbl(t2))));
    g2_line l;
    l.c1 = fp2_neg(fp2_dbl(fp2_mul(t4, zz)));
    l.c2 = fp2_sub(fp2_sub(fp2_sub(fp2_sqr(t6), t0), t5), fp2_dbl(fp2_dbl(t1)));
    l.c0 = fp2_dbl(fp2_mul(r.z, zz));
    return l;
}
KZG_TW g2_line g2_addition_step(g2j &r, const g2a &q) {
    fp2 zz = fp2_sqr(r.z), yy = fp2_sqr(q.y);
    fp2 t0 = fp2_mul(zz, q.x);
    fp2 t1 = fp2_mul(fp2_sub(fp2_sub(fp2_sqr(fp2_add(q.y, r.z)), yy), zz), zz);
    fp2 t2 = fp2_sub(t0, r.x);
    fp2 t3 = fp2_sqr(t2);
    fp2 t4 = fp2_dbl(fp2_dbl(t3));
    fp2 t5 = fp2_mul(t4, t2);
    fp2 t6 = fp2_sub(fp2_sub(t1, r.y), r.y);
    fp2 t9 = fp2_mul(t6, q.x);
    fp2 t7 = fp2_mul(t4, r.x);
    r.x = fp2_sub(fp2_sub(fp2_sub(fp2_sqr(t6), t5), t7), t7);
    r.z = fp2_sub(fp2_sub(fp2_sqr(fp2_add(r.z, t2)), zz), t3);
    fp2 t10 = fp2_add(q.y, r.z);
    fp2 t8 = fp2_mul(fp2_sub(t7, r.x), t6);
    r.y = fp2_sub(t8, fp2_dbl(fp2_mul(r.y, t5)));
    t10 = fp2_sub(fp2_sub(fp2_sqr(t10), yy), fp2_sqr(r.z));
    g2_line l;
    l.c2 = fp2_sub(fp2_dbl(t9), t10);
    l.c0 = fp2_dbl(r.z);
    l.c1 = fp2_dbl(fp2_neg(t6));
    return l;
}

}  // namespace kzg
