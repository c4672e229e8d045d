// Host build of tower.hpp / g2.hpp / pairing.hpp / verify_inputs.hpp for tests/test_pairing_host.py.  Every F_p value crosses this boundary in
// STANDARD form (12 little-endian u32 limbs, < p); F_p12 values as 12 such elements in the order c0.c0.c0, c0.c0.c1, c0.c1.c0, ..., c1.c2.c1.
// The hooks of the check-input lanes take the C ABI's own memory images (Kilic G1 / G2 / F_r, compressed bytes) instead.
#include "pairing.hpp"
#include "verify_inputs.hpp"

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

// ---- the check-input lanes (verify_inputs.hpp) in front of the two-pair check, as capi_verify.hip chains them ----
uint64_t pe_sizeof_prepared() { return sizeof(g2_prepared); }
// what k_g2_prepare does with one Kilic image (any Jacobian Z): g2_from_kilic, g2_to_affine, g2_prepare.  kilic == null: bls.GenG2
void pe_g2_prepare_kilic(const g2j *kilic, g2_prepared *out) {
    const g2j p = g2_from_kilic(kilic ? *kilic : g2_to_kilic(g2_generator()));
    g2_prepare(out, g2_to_affine(p), is_inf(p));
}
// the affine point behind a Kilic Jacobian image, through g2_from_kilic + g2_to_affine (x0, x1, y0, y1); returns 1 for infinity
int pe_g2_kilic_to_affine(const g2j *kilic, uint32_t *out) {
    const g2j p = g2_from_kilic(*kilic);
    g2a a = g2_to_affine(p);
    out_fp2(out, a.x); out_fp2(out + 24, a.y);
    return is_inf(p) ? 1 : 0;
}
// k_kzg_check_inputs + k_pairing_check<true> over n rows: Kilic images c, pi (and es when ys == null), Kilic-Montgomery ys / bs
void pe_kzg_check_batch(uint64_t n, const g1j *c, const g1j *pi, const fr *ys, const g1j *es, const fr *bs, const g2_prepared *gen, const g2_prepared *q1,
                        uint8_t *ok) {
    const g2_prepared *qs[2] = {gen, q1};
    for (uint64_t t = 0; t < n; t++) {
        g1j p[2];
        kzg_check_inputs_lane(c[t], pi[t], ys, es, t, bs[t], p[0], p[1]);
        ok[t] = pairing_product_is_one<2>(qs, p) ? 1 : 0;
    }
}
// k_eth_check_inputs + k_pairing_check<true> + the status overlay of kzg_hip_eth_verify_kzg_proof_batch: 1 / 0, or the row's status 2 / 3
void pe_eth_check_batch(uint64_t n, const uint8_t *c48, const uint8_t *zs, const uint8_t *ys, const uint8_t *pi48, const g2_prepared *gen,
                        const g2_prepared *q1, uint8_t *result) {
    const g2_prepared *qs[2] = {gen, q1};
    for (uint64_t t = 0; t < n; t++) {
        g1j p[2];
        uint8_t st = 0;
        eth_check_inputs_lane(c48 + 48 * t, zs + 32 * t, ys + 32 * t, pi48 + 48 * t, p[0], p[1], st);
        const uint8_t ok = pairing_product_is_one<2>(qs, p) ? 1 : 0;
        result[t] = st ? st : ok;
    }
}
}

#ifdef PE_MAIN
// Stand-alone form for a sanitizer build: reads one single-proof batch (u64 n | n x c | n x pi | n x y | n x b | one Kilic G2 image of [s] G2)
// from the file named on the command line, runs pe_kzg_check_batch, prints the mask as a line of 0 / 1.
#include <stdio.h>
#include <vector>
int main(int argc, char **argv) {
    if (argc != 2) return 2;
    FILE *f = fopen(argv[1], "rb");
    if (!f) return 2;
    uint64_t n = 0;
    if (fread(&n, sizeof n, 1, f) != 1 || n == 0 || n > 4096) return 2;
    std::vector<g1j> c(n), pi(n); std::vector<fr> ys(n), bs(n); g2j q;
    if (fread(c.data(), sizeof(g1j), n, f) != n || fread(pi.data(), sizeof(g1j), n, f) != n || fread(ys.data(), sizeof(fr), n, f) != n ||
        fread(bs.data(), sizeof(fr), n, f) != n || fread(&q, sizeof q, 1, f) != 1) return 2;
    fclose(f);
    std::vector<g2_prepared> prep(2);
    pe_g2_prepare_kilic(nullptr, &prep[0]);
    pe_g2_prepare_kilic(&q, &prep[1]);
    std::vector<uint8_t> ok(n);
    pe_kzg_check_batch(n, c.data(), pi.data(), ys.data(), nullptr, bs.data(), &prep[0], &prep[1], ok.data());
    for (uint64_t i = 0; i < n; i++) putchar(ok[i] ? '1' : '0');
    putchar('\n');
    return 0;
}
#endif
