// verify_inputs.hpp -- what one lane of the check-input kernels (k_pairing.hip) computes, as host/device functions: the G1 inputs
// C - E + [b] pi and -pi of a KZG check from Kilic images, and eth.VerifyKZGProof's parsing (eth/eth.go:114-135) in front of the same sum.
// The kernels keep the index arithmetic, the loads and the stores; tests/host/pairing_emul.cpp runs these bodies on the CPU.
#pragma once
#include "pairing.hpp"

namespace kzg {

KZG_HD g1j g1_generator_internal() {   // bls.GenG1 (standard literals into the device-internal domain)
    const uint32_t gx[12] = {0xdb22c6bbu, 0xfb3af00au, 0xf97a1aefu, 0x6c55e83fu, 0x171bac58u, 0xa14e3a3fu,
                             0x9774b905u, 0xc3688c4fu, 0x4fa9ac0fu, 0x2695638cu, 0x3197d794u, 0x17f1d3a7u};
    const uint32_t gy[12] = {0x46c5e7e1u, 0x0caa2329u, 0xa2888ae4u, 0xd03cc744u, 0x2c04b3edu, 0x00db18cbu,
                             0xd5d00af6u, 0xfcf5e095u, 0x741d8ae4u, 0xa09e30edu, 0xe3aaa0f1u, 0x08b3f481u};
    g1j g; g.x = to_mont<FpP>(fp_const(gx)); g.y = to_mont<FpP>(fp_const(gy)); g.z = one<FpP>();
    return g;
}
// k P for a STANDARD-form scalar: the device GLV split and the regular odd-digit schedule of the G1 kernels (g1.hpp)
KZG_HD g1j g1_mul_std(const g1j &p, const fr &k_std) {
    if (is_inf(p)) return g1_inf();
    g1aq tbl[8]; fq dz[7]; g1jq q; g1j packed;
    const int st = g1_mul_glv_regular_aq<false>(g1jq_unpack(p), glv_split_signed(k_std), tbl, dz, q, packed);
    return st == 1 ? g1jq_pack(q) : st == 2 ? packed : g1_inf();
}

// G1 inputs of a KZG check e(C - E + [b] pi, G2) e(-pi, [s^k] G2) == 1 (c-kzg's arrangement: no G2 scalar multiplication per check):
//   single proof (ys != null): E = [ys[t]] G1, b = z;   multi proof (ys == null): E = es[t] = [I(s)]_1, b = x^n.
// Row t's Kilic images and Kilic-Montgomery scalars in (ys / es are the batch's arrays), device-internal images out.
KZG_HD void kzg_check_inputs_lane(const g1j &c, const g1j &pi, const fr *ys, const g1j *es, uint64_t t, const fr &b, g1j &p0, g1j &p1) {
    const g1j pr = g1_from_kilic(pi);
    const g1j e = ys ? g1_mul_std(g1_generator_internal(), from_mont<FrP>(ys[t])) : g1_from_kilic(es[t]);
    p0 = g1_add(g1_sub(g1_from_kilic(c), e), g1_mul_std(pr, from_mont<FrP>(b)));
    p1 = g1_neg(pr);
}

// 32 little-endian bytes -> standard form; false when not below r (bls.FrFrom32).  A plain function, not KZG_HD: inlining is the compiler's choice
#if defined(__HIPCC__)
static __host__ __device__ bool fr_from_le32_checked(fr &o, const uint8_t *b) {
#else
static inline bool fr_from_le32_checked(fr &o, const uint8_t *b) {
#endif
    for (int i = 0; i < 8; i++) o.l[i] = (uint32_t)b[4 * i] | (uint32_t)b[4 * i + 1] << 8 | (uint32_t)b[4 * i + 2] << 16 | (uint32_t)b[4 * i + 3] << 24;
    for (int i = 7; i >= 0; i--) { const uint32_t m = FrP::mod(i); if (o.l[i] < m) return true; if (o.l[i] > m) return false; }
    return false;
}
// eth.VerifyKZGProof's parsing and the G1 inputs of its check: status 0 = inputs valid, 2 = z or y not below r, 3 = commitment or proof not a
// valid compressed G1 point (subgroup included), in the reference's order (z, y, commitment, proof).  Invalid rows get points at infinity.
KZG_HD void eth_check_inputs_lane(const uint8_t *c48, const uint8_t *z32, const uint8_t *y32, const uint8_t *pi48, g1j &p0, g1j &p1, uint8_t &status) {
    p0 = g1_inf(); p1 = g1_inf();
    fr z, y;
    if (!fr_from_le32_checked(z, z32) || !fr_from_le32_checked(y, y32)) { status = 2; return; }
    g1j c, pr;
    if (!g1_decompress(c, c48) || !g1_decompress(pr, pi48)) { status = 3; return; }
    status = 0;
    p0 = g1_add(g1_sub(c, g1_mul_std(g1_generator_internal(), y)), g1_mul_std(pr, z));
    p1 = g1_neg(pr);
}

}  // namespace kzg
