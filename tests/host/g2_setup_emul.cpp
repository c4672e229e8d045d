// Host build of g2.hpp's setup half for tests/test_g2_setup_host.py: the mixed addition, the digit cutter, the fixed-base table of bls.GenG2 and the
// walk over it, normalisation and compression -- the bodies k_g2.hip runs, one call per lane.  F_p values cross this boundary in STANDARD form
// (12 little-endian u32 limbs, < p): a Jacobian point is (x0, x1, y0, y1, z0, z1), an affine one (x0, x1, y0, y1), all zero for "no point".
// Scalars and G2 images cross it as the C ABI's own memory images (Kilic-Montgomery F_r, Kilic G2).
#include "g2.hpp"
#include <vector>

using namespace kzg;

static fp in_fp(const uint32_t *s) { fp a; for (int i = 0; i < 12; i++) a.l[i] = s[i]; return to_mont<FpP>(a); }
static void out_fp(uint32_t *d, const fp &a) { fp s = from_mont<FpP>(a); for (int i = 0; i < 12; i++) d[i] = s.l[i]; }
static fp2 in_fp2(const uint32_t *s) { fp2 a; a.c0 = in_fp(s); a.c1 = in_fp(s + 12); return a; }
static void out_fp2(uint32_t *d, const fp2 &a) { out_fp(d, a.c0); out_fp(d + 12, a.c1); }
static void out_affine(uint32_t *d, const g2a &a) { out_fp2(d, a.x); out_fp2(d + 24, a.y); }

static std::vector<g2a> &table() {   // what k_g2_fixed_base_table leaves: the window bases as g2_fb_window_base gives them, the entries by g2_fb_entry
    static std::vector<g2a> t;
    if (t.empty()) {
        t.resize(G2_FB_ENTRIES);
        for (int w = 0; w < G2_FB_WINDOWS; w++) {
            const g2j base = g2_fb_window_base(w);
            for (uint32_t d = 0; d < (uint32_t)G2_FB_ROW; d++) t[(uint64_t)w * G2_FB_ROW + d] = g2_fb_entry(base, d);
        }
    }
    return t;
}

extern "C" {
// g2_add_mixed(p, q) as an affine point; returns 1 when the sum is infinity
int g2e_add_mixed(const uint32_t *p_jac, const uint32_t *q_aff, uint32_t *out_aff) {
    g2j p; p.x = in_fp2(p_jac); p.y = in_fp2(p_jac + 24); p.z = in_fp2(p_jac + 48);
    g2a q; q.x = in_fp2(q_aff); q.y = in_fp2(q_aff + 24);
    const g2j s = g2_add_mixed(p, q);
    out_affine(out_aff, g2_to_affine(s));
    return is_inf(s) ? 1 : 0;
}
uint32_t g2e_window_bits() { return G2_FB_C; }
uint32_t g2e_windows() { return G2_FB_WINDOWS; }
// the digits the walk takes from a Montgomery-form scalar, least significant window first
void g2e_digits(const fr *k_mont, uint32_t *digits) {
    const fr k = from_mont<FrP>(*k_mont);
    for (int w = 0; w < G2_FB_WINDOWS; w++) digits[w] = g2_fb_digit(k, w);
}
void g2e_table_entry(uint32_t w, uint32_t d, uint32_t *out_aff) { out_affine(out_aff, table()[(uint64_t)w * G2_FB_ROW + d]); }
// k_g2_fixed_base + k_g2_normalize over n scalars: Kilic images out
void g2e_mul_generator(uint64_t n, const fr *k_mont, g2j *out_kilic) {
    const g2a *t = table().data();
    for (uint64_t i = 0; i < n; i++) out_kilic[i] = g2_normalize_to_kilic(g2_fb_mul(t, k_mont[i]));
}
// k_g2_compress over n Kilic images (any Z)
void g2e_compress(uint64_t n, const g2j *in_kilic, uint8_t *out96) {
    for (uint64_t i = 0; i < n; i++) g2_compress(out96 + 96 * i, g2_from_kilic(in_kilic[i]));
}
// k_g2_from_compressed on one encoding; returns 1 when it is valid
int g2e_decompress(const uint8_t *in96, g2j *out_kilic) {
    g2j p;
    const bool ok = g2_decompress(p, in96);
    *out_kilic = g2_to_kilic(p);
    return ok ? 1 : 0;
}
}

#ifdef G2E_MAIN
// Stand-alone form for a sanitizer build: reads u64 n | n Montgomery scalars from the file named on the command line, walks a table of full size
// in which only the entries these scalars select are filled in (by the same g2_fb_window_base / g2_fb_entry; the rest stay "no point"), normalises
// and compresses, and prints one line of hex per scalar; then the exceptional cases of the mixed addition on [5] G2, one line each.
#include <stdio.h>
int main(int argc, char **argv) {
    if (argc != 2) return 2;
    FILE *f = fopen(argv[1], "rb");
    if (!f) return 2;
    uint64_t n = 0;
    if (fread(&n, sizeof n, 1, f) != 1 || n == 0 || n > 64) return 2;
    std::vector<fr> k(n);
    if (fread(k.data(), sizeof(fr), n, f) != n) return 2;
    fclose(f);
    g2a none; none.x = fp2_zero(); none.y = fp2_zero();
    std::vector<g2a> t(G2_FB_ENTRIES, none);
    std::vector<g2j> bases;
    for (int w = 0; w < G2_FB_WINDOWS; w++) bases.push_back(g2_fb_window_base(w));
    for (uint64_t i = 0; i < n; i++) {
        const fr ks = from_mont<FrP>(k[i]);
        for (int w = 0; w < G2_FB_WINDOWS; w++) {
            const uint32_t d = g2_fb_digit(ks, w);
            t[(uint64_t)w * G2_FB_ROW + d] = g2_fb_entry(bases[w], d);
        }
    }
    std::vector<g2j> pts(n + 5);
    for (uint64_t i = 0; i < n; i++) pts[i] = g2_normalize_to_kilic(g2_fb_mul(t.data(), k[i]));
    const g2a five = g2_fb_entry(bases[0], 5);
    g2j p5; p5.x = five.x; p5.y = five.y; p5.z = fp2_one();
    g2a neg5 = five; neg5.y = fp2_neg(five.y);
    pts[n] = g2_normalize_to_kilic(g2_add_mixed(g2_inf(), five));      // [5] G2
    pts[n + 1] = g2_normalize_to_kilic(g2_add_mixed(p5, none));        // [5] G2
    pts[n + 2] = g2_normalize_to_kilic(g2_add_mixed(p5, five));        // [10] G2
    pts[n + 3] = g2_normalize_to_kilic(g2_add_mixed(p5, neg5));        // infinity
    pts[n + 4] = g2_normalize_to_kilic(g2_add_mixed(g2_inf(), none));  // infinity
    std::vector<uint8_t> out(96 * (n + 5));
    g2e_compress(n + 5, pts.data(), out.data());
    for (uint64_t i = 0; i < n + 5; i++) {
        for (int b = 0; b < 96; b++) printf("%02x", out[96 * i + b]);
        putchar('\n');
    }
    return 0;
}
#endif
