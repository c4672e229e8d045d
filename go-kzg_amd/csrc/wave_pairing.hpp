// wave_pairing.hpp -- the pairing check of pairing.hpp on ONE WAVEFRONT per check, on wave_tower.hpp's operations: the multi-Miller loop over
// K prepared G2 points (K = 1, 2) and the final exponentiation, step for step -- the same line order, the same skipping of a pair with a point
// at infinity on either side, the same zkcrypto addition chain, so the value is the same cube e(P, Q)^3 and, the arithmetic being exact on
// canonical representatives, the same bytes.
//
// The line coefficients are read from the same g2_prepared images (shared or per check) by the six lanes that scale them; the G1 inputs
// (g1_line_eval_of) are computed once per check by lane i of pair i and kept in LDS.  Control flow depends only on the loop constants and on
// the two `on` flags, which every lane derives from the same memory: every lane reaches every barrier.
//
// LDS per check: wv::image = 192 slots x 48 bytes = 9 216 bytes (80 scratch slots: 54 product slots + operand sums; 16 for constants and G1
// inputs; 8 values of 12 slots: the accumulator and t0 .. t6 of the final exponentiation).  hipcc reports for gfx950: k_pairing_check_wave
// 129 VGPRs, 80 bytes of scratch per lane (the frames of the out-of-line calls), 3 waves per SIMD (profiles/verify.md has the full report).
#pragma once
#include "pairing.hpp"
#include "wave_tower.hpp"

namespace kzg {
namespace wv {

enum { F = 0, T0 = 1, T1 = 2, T2 = 3, T3 = 4, T4 = 5, T5 = 6, T6 = 7 };   // the values of an image

// first phase of an image: constants, the accumulator = 1, and the G1 inputs of the pairs (lanes 16 .. 16 + K; kilic: Kilic images)
template <int K> KZG_WV void init_phase(image &im, int lane, const g1j *const *p, bool kilic) {
    const_phase(im, lane);
    if (lane >= 16 && lane < 16 + K) {
        const int i = lane - 16;
        const g1_line_eval e = g1_line_eval_of(kilic ? g1_from_kilic(*p[i]) : *p[i]);
        st(im, lane, E0 + 3 * i, e.y); st(im, lane, E0 + 3 * i + 1, e.xz); st(im, lane, E0 + 3 * i + 2, e.z3);
    }
    if (lane >= 32 && lane < 44) st(im, lane, reg(F) + (lane - 32), lane == 32 ? one<FpP>() : zero<FpP>());
}
// ell's scaling: (c0, c1, c4) = (l.c2 Z^3, l.c1 X Z, l.c0 Y) into X[XS .. XS + 6), one F_p product on each of six lanes
KZG_WV void line_phase(image &im, int lane, const g2_line *l, int pair) {
    if (lane >= 6) return;
    const int k = lane >> 1;                                   // 0: c2 with Z^3, 1: c1 with X Z, 2: c0 with Y
    const fp2 &c = k == 0 ? l->c2 : k == 1 ? l->c1 : l->c0;
    st(im, lane, XS + lane, mul((lane & 1) ? c.c1 : c.c0, ld(im, lane, E0 + 3 * pair + (2 - k))));
}
template <class X> KZG_WV void ell(X &x, const g2_prepared *q, int idx, int pair) {
    const g2_line *l = &q->l[idx];
    x.run([=](image &im, int lane) { line_phase(im, lane, l, pair); });
    mul_014(x, F, F);
}

// F = prod_i f_{|x|, Q_i}(P_i), conjugated (pairing.hpp multi_miller_loop)
template <int K, class X> KZG_WV void multi_miller_loop(X &x, const g2_prepared *const *q, const g1j *const *p, bool kilic) {
    bool on[K];
    for (int i = 0; i < K; i++) on[i] = !is_inf(*p[i]) && q[i]->inf == 0;      // the same for every lane; Z = 0 in either image of a point
    x.run([=](image &im, int lane) { init_phase<K>(im, lane, p, kilic); });
    int idx = 0;
    for (int b = 61; b >= 0; b--) {
        for (int i = 0; i < K; i++) if (on[i]) ell(x, q[i], idx, i);
        idx++;
        if (((BLS_X_ABS >> 1) >> b) & 1u) {
            for (int i = 0; i < K; i++) if (on[i]) ell(x, q[i], idx, i);
            idx++;
        }
        sqr(x, F, F);
    }
    for (int i = 0; i < K; i++) if (on[i]) ell(x, q[i], idx, i);
    conj(x, F, F);
}

// d = a^x on the cyclotomic subgroup (pairing.hpp cyc_exp_x; its first step 1 * a is a copy); d != a
template <class X> KZG_WV void cyc_exp_x(X &x, int d, int a) {
    copy(x, d, a);
    for (int b = 62; b >= 0; b--) {
        cyc_sqr(x, d, d);
        if ((BLS_X_ABS >> b) & 1u) mul(x, d, d, a);
    }
    conj(x, d, d);
}
// F = F^(3 (p^12 - 1) / r) (pairing.hpp final_exponentiation, line for line; F doubles as the temporary once f is consumed)
template <class X> KZG_WV void final_exponentiation(X &x) {
    conj(x, T0, F);
    inv(x, T1, F);
    mul(x, T2, T0, T1);
    copy(x, T1, T2);
    frob2(x, T2, T2); mul(x, T2, T2, T1);
    cyc_sqr(x, T1, T2); conj(x, T1, T1);
    cyc_exp_x(x, T3, T2);
    cyc_sqr(x, T4, T3);
    mul(x, T5, T1, T3);
    cyc_exp_x(x, T1, T5);
    cyc_exp_x(x, T0, T1);
    cyc_exp_x(x, T6, T0);
    mul(x, T6, T6, T4);
    cyc_exp_x(x, T4, T6);
    conj(x, T5, T5);
    mul(x, F, T5, T2); mul(x, T4, T4, F);
    conj(x, T5, T2);
    mul(x, T1, T1, T2);
    frob3(x, T1, T1);
    mul(x, T6, T6, T5);
    frob(x, T6, T6);
    mul(x, T3, T3, T0);
    frob2(x, T3, T3);
    mul(x, T3, T3, T1);
    mul(x, T3, T3, T6);
    mul(x, F, T3, T4);
}
// *ok = (prod_i e(P_i, Q_i) == 1)
template <int K, class X> KZG_WV void pairing_check(X &x, const g2_prepared *const *q, const g1j *const *p, uint8_t *ok) {
    multi_miller_loop<K>(x, q, p, false);
    final_exponentiation(x);
    is_one_prepare(x, F);
    x.run([=](image &im, int lane) { if (lane == 0) *ok = is_one_of(im, lane) ? 1 : 0; });
}
// out[0 .. 12) = the reduced value of one pair in standard form (g1: a Kilic image)
template <class X> KZG_WV void pairing_value(X &x, const g2_prepared *q, const g1j *g1, fp *out) {
    const g2_prepared *qs[1] = {q};
    const g1j *ps[1] = {g1};
    multi_miller_loop<1>(x, qs, ps, true);
    final_exponentiation(x);
    x.run([=](image &im, int lane) { if (lane < 12) out[lane] = from_mont<FpP>(ld(im, lane, reg(F) + lane)); });
}

}  // namespace wv
}  // namespace kzg
