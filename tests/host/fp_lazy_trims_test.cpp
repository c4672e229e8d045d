// Stand-alone host check of the lazy F_p cores (go-kzg_amd/csrc/field.hpp: mont_core30, mont_sqr_core30, mont_core30_dot2) and of the mixed
// addition built on them (g1.hpp: g1x_madd_fast, g1x_acc::add), against plain big-integer arithmetic.
// TEST INFRASTRUCTURE: built and run by tests/test_fp_lazy_trims_host.py (once plain, once with -fsanitize=address,undefined), never shipped.
//
// The cores carry every retired column with the 64-bit shift: a 32-bit funnel shift in the rounds where a column stays below 2^62 was measured and did
// not pay (profiles/fp_lazy_trims.md), so there is no 32-bit form whose bound would have to be asserted here.  The carry sweeps move high words only
// (sweep_hi); operands with every limb at 2^30 - 1 drive every column to its largest value between two sweeps.
#include <stdint.h>
#include <stdio.h>
#include <stdlib.h>
#include <string.h>
#include "field.hpp"
#include "g1.hpp"
using namespace kzg;

static int g_fail = 0;
#define CHECK(cond, ...) do { if (!(cond)) { if (g_fail < 20) { printf("FAIL %s:%d: %s  ", __FILE__, __LINE__, #cond); printf(__VA_ARGS__); printf("\n"); } g_fail++; } } while (0)

// ---- plain big integers: 28 words of 32 bits (896 bits; the widest value here is A B + C D + M p < 2^783) ----
struct Big { uint32_t w[28]; };
static Big big0() { Big o; memset(&o, 0, sizeof o); return o; }
static Big big_u(uint32_t v) { Big o = big0(); o.w[0] = v; return o; }
static Big big_add(const Big &a, const Big &b) { Big o; uint64_t c = 0; for (int i = 0; i < 28; i++) { c += (uint64_t)a.w[i] + b.w[i]; o.w[i] = (uint32_t)c; c >>= 32; } if (c) { printf("big_add overflow\n"); exit(2); } return o; }
static Big big_sub(const Big &a, const Big &b) { Big o; int64_t c = 0; for (int i = 0; i < 28; i++) { c += (int64_t)a.w[i] - b.w[i]; o.w[i] = (uint32_t)c; c >>= 32; } if (c) { printf("big_sub underflow\n"); exit(2); } return o; }
static Big big_mul(const Big &a, const Big &b, bool wrap = false) {   // wrap: product taken mod 2^896 (the Hensel lift below)
    Big o = big0();
    for (int i = 0; i < 28; i++) {
        if (!a.w[i]) continue;
        uint64_t c = 0;
        for (int j = 0; j < 28; j++) {
            if (i + j >= 28) { if (!wrap && (b.w[j] || c)) { printf("big_mul overflow\n"); exit(2); } continue; }
            c += (uint64_t)a.w[i] * b.w[j] + o.w[i + j]; o.w[i + j] = (uint32_t)c; c >>= 32;
        }
    }
    return o;
}
static int big_cmp(const Big &a, const Big &b) { for (int i = 27; i >= 0; i--) if (a.w[i] != b.w[i]) return a.w[i] < b.w[i] ? -1 : 1; return 0; }
static Big big_shr(const Big &a, int bits) {
    Big o = big0(); const int ws = bits / 32, bs = bits % 32;
    for (int i = 0; i + ws < 28; i++) { uint64_t v = a.w[i + ws]; if (i + ws + 1 < 28) v |= (uint64_t)a.w[i + ws + 1] << 32; o.w[i] = (uint32_t)(v >> bs); }
    return o;
}
static Big big_low(const Big &a, int bits) { Big o = a; for (int i = 0; i < 28; i++) { const int lo = 32 * i; if (lo >= bits) o.w[i] = 0; else if (lo + 32 > bits) o.w[i] &= (1u << (bits - lo)) - 1u; } return o; }
static Big big_from_limbs(const uint32_t *l) {   // sum l[k] 2^(30 k), any 32-bit limbs
    Big o = big0();
    for (int k = 12; k >= 0; k--) { Big s = big0(); uint64_t c = 0; for (int i = 0; i < 28; i++) { c |= (uint64_t)o.w[i] << 30; s.w[i] = (uint32_t)c; c >>= 32; } o = big_add(s, big_u(l[k])); }
    return o;
}
static void big_to_limbs(uint32_t *l, const Big &a) {   // normalised: limbs 0..11 are 30 bits, limb 12 the rest (must fit 32 bits)
    for (int k = 0; k < 13; k++) { Big s = big_shr(a, 30 * k); if (k < 12) l[k] = s.w[0] & 0x3fffffffu; else { l[k] = s.w[0]; for (int i = 1; i < 28; i++) if (s.w[i]) { printf("value does not fit 13 limbs\n"); exit(2); } } }
}
static Big P, NPINV;   // p, and -1 / p mod 2^390
static void big_init() {
    P = big0(); for (int i = 0; i < 12; i++) P.w[i] = FpP::mod(i);
    Big inv = big_u(1);   // Hensel: inv <- inv (2 - p inv) doubles the correct low bits; 2^896 - x is the wrapped negative
    for (int it = 0; it < 10; it++) {
        Big t = big_mul(P, inv, true), two_minus = big0();
        uint64_t c = 2; for (int i = 0; i < 28; i++) { c += (uint32_t)~t.w[i]; if (i == 0) c += 1; two_minus.w[i] = (uint32_t)c; c >>= 32; }
        inv = big_mul(inv, two_minus, true);
    }
    Big chk = big_low(big_mul(P, inv, true), 390);
    if (big_cmp(chk, big_u(1)) != 0) { printf("p^-1 lift failed\n"); exit(2); }
    Big neg = big0(); uint64_t c = 1; for (int i = 0; i < 28; i++) { c += (uint32_t)~inv.w[i]; neg.w[i] = (uint32_t)c; c >>= 32; }
    NPINV = big_low(neg, 390);
    uint32_t l[13]; big_to_limbs(l, NPINV);
    if (l[0] != FpP::INV30) { printf("INV30 mismatch\n"); exit(2); }
}
// the Montgomery quotient is unique: (T + M p) / 2^390 with M = -T / p mod 2^390; value < T / 2^390 + p
static void want_redc(uint32_t *l, const Big &T) {
    Big M = big_low(big_mul(big_low(T, 390), NPINV, true), 390);
    Big S = big_add(T, big_mul(M, P));
    if (big_cmp(big_low(S, 390), big0()) != 0) { printf("redc not exact\n"); exit(2); }
    Big V = big_shr(S, 390);
    if (big_cmp(V, big_add(big_shr(T, 390), P)) > 0) { printf("redc bound\n"); exit(2); }
    // the cores keep 13 limbs of 30 bits: V mod 2^390.  Inside the contract of mulq (T < 2^390 p) that is V itself (V < 2 p); operands with every limb at
    // 2^30 - 1 lie outside it and are here for the column bounds: their limbs are still pinned one by one
    big_to_limbs(l, big_low(V, 390));
}
static Big big_kp(uint32_t k) { return big_mul(P, big_u(k)); }

// ---- operands ----
static uint64_t g_st = 0x1234567ull;
static uint64_t rnd() { g_st += 0x9e3779b97f4a7c15ull; uint64_t z = g_st; z = (z ^ (z >> 30)) * 0xbf58476d1ce4e5b9ull; z = (z ^ (z >> 27)) * 0x94d049bb133111ebull; return z ^ (z >> 31); }
struct Op { uint32_t l[13]; };
static Op op_big(const Big &v) { Op o; big_to_limbs(o.l, v); return o; }
static Op op_kp_minus(uint32_t k, uint32_t d) { return op_big(big_sub(big_kp(k), big_u(d))); }
static Op op_rand() {
    Op o; const uint64_t mode = rnd() % 4;
    for (int k = 0; k < 13; k++) {
        uint64_t r = rnd();
        o.l[k] = (mode == 0 ? (uint32_t)r : mode == 1 ? (uint32_t)(r & (r >> 32)) : mode == 2 ? ~(uint32_t)(r & (r >> 32)) : ((r & 3) ? 0x3fffffffu : (uint32_t)(r >> 8))) & 0x3fffffffu;
    }
    if (mode != 3 && (rnd() & 1)) o.l[12] &= 0x00ffffffu;   // about half of them below 2^384, as values bounded by a few p are
    return o;
}
static bool same13(const uint32_t *a, const uint32_t *b) { return memcmp(a, b, 13 * sizeof(uint32_t)) == 0; }

static void check_mul(const Op &a, const Op &b, const char *what) {
    uint32_t got[13], want[13];
    mont_core30(got, a.l, b.l);
    want_redc(want, big_mul(big_from_limbs(a.l), big_from_limbs(b.l)));
    CHECK(same13(got, want), "%s: mont_core30", what);
}
static void check_sqr(const Op &a, const char *what) {
    uint32_t got[13], want[13];
    mont_sqr_core30(got, a.l);
    Big A = big_from_limbs(a.l);
    want_redc(want, big_mul(A, A));
    CHECK(same13(got, want), "%s: mont_sqr_core30", what);
}
static void check_dot2(const Op &a, const Op &b, const Op &c, const Op &d, const char *what) {
    uint32_t got[13], want[13];
    mont_core30_dot2(got, a.l, b.l, c.l, d.l);
    want_redc(want, big_add(big_mul(big_from_limbs(a.l), big_from_limbs(b.l)), big_mul(big_from_limbs(c.l), big_from_limbs(d.l))));
    CHECK(same13(got, want), "%s: mont_core30_dot2", what);
}

static void test_cores() {
    Op ones; for (int k = 0; k < 13; k++) ones.l[k] = 0x3fffffffu;                  // every partial product at its largest: the column bounds
    check_mul(ones, ones, "all limbs 2^30 - 1"); check_sqr(ones, "all limbs 2^30 - 1"); check_dot2(ones, ones, ones, ones, "all limbs 2^30 - 1");
    // the largest bounds the callers use: Ba Bb = 600 for a product (24 x 25, 600 x 1, 1 x 600), 8 x 14 + 11 x 2 for the pair of Y3
    // (and a little above it), 14^2 for P^2
    check_mul(op_kp_minus(24, 1), op_kp_minus(25, 1), "24 p x 25 p"); check_mul(op_kp_minus(600, 1), op_kp_minus(1, 1), "600 p x p"); check_mul(op_kp_minus(1, 1), op_kp_minus(600, 1), "p x 600 p");
    check_sqr(op_kp_minus(24, 1), "(24 p)^2"); check_sqr(op_kp_minus(14, 1), "(14 p)^2");
    check_dot2(op_kp_minus(8, 1), op_kp_minus(14, 1), op_kp_minus(11, 1), op_kp_minus(2, 1), "8 x 14 + 11 x 2");
    check_dot2(op_kp_minus(9, 1), op_kp_minus(14, 1), op_kp_minus(11, 1), op_kp_minus(2, 1), "9 x 14 + 11 x 2");
    check_dot2(op_kp_minus(24, 1), op_kp_minus(24, 1), op_kp_minus(12, 1), op_kp_minus(2, 1), "576 + 24");
    Op sp[5] = {op_big(big0()), op_big(big_u(1)), op_kp_minus(1, 0), op_kp_minus(1, 1), op_kp_minus(2, 0)};   // 0, 1, p, p - 1, 2 p
    for (int i = 0; i < 5; i++) {
        check_sqr(sp[i], "special");
        for (int j = 0; j < 5; j++) {
            check_mul(sp[i], sp[j], "special"); check_mul(sp[i], ones, "special x ones");
            for (int k = 0; k < 5; k++) check_dot2(sp[i], sp[j], sp[k], sp[(i + j + k) % 5], "special");
        }
    }
    for (int n = 0; n < 20000; n++) {
        Op a = op_rand(), b = op_rand(), c = op_rand(), d = op_rand();
        check_mul(a, b, "random"); check_sqr(c, "random"); check_dot2(a, c, d, b, "random");
    }
}

// is_zero_mod_p_q is exact: only 0 and p pass
static void test_field_pieces() {
    fq z; for (int k = 0; k < 13; k++) z.l[k] = 0;
    fq pq; for (int k = 0; k < 13; k++) pq.l[k] = FpP::p30(k);
    CHECK(is_zero_mod_p_q(z) && is_zero_mod_p_q(pq), "0 and p are zero mod p");
    for (int k = 1; k < 13; k++) {
        fq t = z; t.l[k] = 1; CHECK(!is_zero_mod_p_q(t), "limb 0 zero, limb %d not", k);
        t = pq; t.l[k] ^= 1u; CHECK(!is_zero_mod_p_q(t), "limb 0 of p, limb %d off", k);
    }
    fq t = z; t.l[0] = 1; CHECK(!is_zero_mod_p_q(t), "1");
    t = pq; t.l[0] -= 1; CHECK(!is_zero_mod_p_q(t), "p - 1");
}

// ---- the mixed addition ----
static fp fp_from_hex(const char *h) {   // standard form, big-endian hex -> the device's Montgomery image
    fp o = zero<FpP>(); const int n = (int)strlen(h);
    for (int i = 0; i < n; i++) { const char ch = h[n - 1 - i]; const uint32_t v = ch <= '9' ? ch - '0' : ch - 'a' + 10; o.l[i / 8] |= v << (4 * (i % 8)); }
    return to_mont<FpP>(o);
}
static bool same_fp(const fp &a, const fp &b) { return equal<FpP>(a, b); }
static bool same_g1x(const g1x &a, const g1x &b) { return same_fp(a.x, b.x) && same_fp(a.y, b.y) && same_fp(a.zz, b.zz) && same_fp(a.zzz, b.zzz); }
static bool same_g1xq(const g1xq &a, const g1xq &b) { return same13(a.x.l, b.x.l) && same13(a.y.l, b.y.l) && same13(a.zz.l, b.zz.l) && same13(a.zzz.l, b.zzz.l); }
static g1a affine_of(const g1j &p) { g1j n = g1_normalize(p); g1a o; o.x = n.x; o.y = n.y; return o; }
static g1a affine_of(const g1x &p) { return affine_of(g1x_to_jac(p)); }

static void test_madd() {
    g1a G;
    G.x = fp_from_hex("17f1d3a73197d7942695638c4fa9ac0fc3688c4f9774b905a14e3a3f171bac586c55e83ff97a1aeffb3af00adb22c6bb");
    G.y = fp_from_hex("08b3f481e3aaa0f1a09e30ed741d8ae4fcf5e095d5d00af600db18cb2c04b3edd03cc744a2888ae40caa232946c5e7e1");
    fp four = one<FpP>(); four = dbl<FpP>(dbl<FpP>(four));
    CHECK(same_fp(sqr(G.y), add<FpP>(mul(G.x, sqr(G.x)), four)), "generator is on y^2 = x^3 + 4");
    // 24 affine points: k_i G for a walk of doublings and additions
    g1a pts[24]; g1j run = to_jac(G);
    for (int i = 0; i < 24; i++) { run = g1_add(g1_dbl(run), to_jac(G)); if (i % 3 == 0) run = g1_dbl(run); pts[i] = affine_of(run); }
    // a long chain through the fast path with both signs (the walk negates the packed y of the entry): packed results equal g1x_madd's on the same packed inputs (the same formulas mod p), and the
    // bounds invariant holds for ever (300 additions)
    g1xq acc = g1xq_from_affine(G);
    for (int n = 0; n < 300; n++) {
        const g1a &q = pts[(n * 7) % 24]; const bool ng = ((n >> 1) ^ n) & 1;
        const g1x before = g1xq_pack(acc);
        const g1a qs = ng ? g1_neg(q) : q;
        const bool ok = g1x_madd_fast(acc, unpackq(qs.x), unpackq(qs.y));
        CHECK(ok, "fast path declined distinct points at step %d", n);
        const g1x want = g1x_madd(before, qs);
        CHECK(same_g1x(g1xq_pack(acc), want), "g1x_madd_fast (neg = %d) != g1x_madd at step %d", (int)ng, n);
    }
    // P == Q and P == -Q, reached with the entry as stored and with its negated image, accumulator affine (ZZ = 1) and not: declined, accumulator untouched; g1x_acc::add then
    // takes the complete formulas: the double, or infinity
    for (int rep = 0; rep < 2; rep++) {
        g1xq a = g1xq_from_affine(pts[3]);
        if (rep) { bool ok = g1x_madd_fast(a, unpackq(pts[5].x), unpackq(pts[5].y)) && g1x_madd_fast(a, unpackq(g1_neg(pts[9]).x), unpackq(g1_neg(pts[9]).y)); CHECK(ok, "set-up"); }
        const g1a same = affine_of(g1xq_pack(a)), opp = g1_neg(same);
        for (int c = 0; c < 4; c++) {
            const bool ng = (c & 2) != 0;
            const g1a q = ng ? g1_neg((c & 1) ? opp : same) : ((c & 1) ? opp : same);   // what the walk hands over after applying the digit's sign
            g1xq t = a;
            CHECK(!g1x_madd_fast(t, unpackq(q.x), unpackq(q.y)), "fast path accepted P == +-Q (rep %d case %d)", rep, c);
            CHECK(same_g1xq(t, a), "declined addition touched the accumulator (rep %d case %d)", rep, c);
            g1x_acc w; w.init(); w.v = a; w.inf = false;
            w.add(q);
            const bool doubles = ((c & 1) != 0) == ng;          // q, or -(-q)
            if (doubles) {
                CHECK(!w.inf, "P + P is not infinity");
                const g1a got = affine_of(w.to_jac()), want = affine_of(g1_dbl(to_jac(same)));
                CHECK(same_fp(got.x, want.x) && same_fp(got.y, want.y), "P + P through the fallback (rep %d case %d)", rep, c);
            } else CHECK(w.inf, "P - P through the fallback (rep %d case %d)", rep, c);
        }
    }
    // first entry of an empty accumulator, negated
    g1x_acc e; e.init(); e.add(g1_neg(pts[2]));
    const g1a got = affine_of(e.to_jac()), want = g1_neg(pts[2]);
    CHECK(!e.inf && same_fp(got.x, want.x) && same_fp(got.y, want.y), "first entry negated");
}

int main() {
    big_init();
    test_cores();
    test_field_pieces();
    test_madd();
    if (g_fail) { printf("fp_lazy_trims_test: %d FAILED\n", g_fail); return 1; }
    printf("fp_lazy_trims_test: ok\n");
    return 0;
}
