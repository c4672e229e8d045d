// k_pairing.hip -- verification kernels, one lane per point or per check: G2 decompression, G2 preparation (the 68 line coefficients of a
// point), the G1 inputs of KZG checks, and the pairing check itself (multi-Miller loop over two pairs + final exponentiation, pairing.hpp).
// Replaces bls.FromCompressedG2 and bls.PairingsVerify (bls/bls_kilic.go:121-158) under KZGSettings.CheckProofSingle / CheckProofMulti
// (kzg_single_proofs.go:57, kzg_multi_proofs.go:47) and eth.VerifyKZGProof (eth/eth.go:114, eth/helpers.go:55).
#include "internal.hpp"
#include "pairing.hpp"
#include "verify_inputs.hpp"

namespace kzg {

// One wavefront per workgroup: a lane carries an F_p12 accumulator (144 VGPRs) plus the operands of the out-of-line tower products, so the
// check kernel is register-bound whatever the block size; 64 lanes keep the tail of a small batch to one wavefront.
#define PAIRING_BLOCK 64
static inline dim3 pairing_grid(uint64_t n) { return dim3((uint32_t)((n + PAIRING_BLOCK - 1) / PAIRING_BLOCK)); }

__global__ __launch_bounds__(PAIRING_BLOCK) void k_g2_from_compressed(const uint8_t *in96, g2j *out, uint64_t n, uint32_t *bad) {
    const uint64_t t = blockIdx.x * (uint64_t)blockDim.x + threadIdx.x;
    if (t >= n) return;
    g2j p;
    if (!g2_decompress(p, in96 + 96 * t)) atomicOr(bad, 1u);
    out[t] = g2_to_kilic(p);   // API output: Kilic image
}
void launch_g2_from_compressed(hipStream_t s, const uint8_t *in96, g2j *out, uint64_t n, uint32_t *bad_flag) {
    if (!n) return;
    hipLaunchKernelGGL(k_g2_from_compressed, pairing_grid(n), dim3(PAIRING_BLOCK), 0, s, in96, out, n, bad_flag);
}

// Kilic images in, prepared lines out (one F_p2 inversion per point for the affine form the addition step needs)
__global__ __launch_bounds__(PAIRING_BLOCK) void k_g2_prepare(const g2j *in, uint64_t n, g2_prepared *out) {
    const uint64_t t = blockIdx.x * (uint64_t)blockDim.x + threadIdx.x;
    if (t >= n) return;
    const g2j p = g2_from_kilic(in[t]);
    g2_prepare(out + t, g2_to_affine(p), is_inf(p));
}
void launch_g2_prepare(hipStream_t s, const g2j *in_kilic, uint64_t n, g2_prepared *out) {
    if (!n) return;
    hipLaunchKernelGGL(k_g2_prepare, pairing_grid(n), dim3(PAIRING_BLOCK), 0, s, in_kilic, n, out);
}

// bls.PairingsVerify's G1 side: p0 = -a1, p1 = b1, Kilic images in, device-internal images out
__global__ __launch_bounds__(PAIRING_BLOCK) void k_pairs_g1_from_kilic(const g1j *a1, const g1j *b1, uint64_t n, g1j *p0, g1j *p1) {
    const uint64_t t = blockIdx.x * (uint64_t)blockDim.x + threadIdx.x;
    if (t >= n) return;
    p0[t] = g1_neg(g1_from_kilic(a1[t]));
    p1[t] = g1_from_kilic(b1[t]);
}
void launch_pairs_g1_from_kilic(hipStream_t s, const g1j *a1, const g1j *b1, uint64_t n, g1j *p0, g1j *p1) {
    if (!n) return;
    hipLaunchKernelGGL(k_pairs_g1_from_kilic, pairing_grid(n), dim3(PAIRING_BLOCK), 0, s, a1, b1, n, p0, p1);
}

// G1 inputs of a KZG check (kzg_check_inputs_lane, verify_inputs.hpp): single proofs with ys != null (E = [y] G1, b = z), multi proofs with
// ys == null (E = es[i] = [I(s)]_1, b = x^n).  Kilic images and Kilic-Montgomery scalars in.
__global__ __launch_bounds__(PAIRING_BLOCK) void k_kzg_check_inputs(const g1j *c, const g1j *pi, const fr *ys, const g1j *es, const fr *bs, uint64_t n,
                                                                    g1j *p0, g1j *p1) {
    const uint64_t t = blockIdx.x * (uint64_t)blockDim.x + threadIdx.x;
    if (t >= n) return;
    kzg_check_inputs_lane(c[t], pi[t], ys, es, t, bs[t], p0[t], p1[t]);
}
void launch_kzg_check_inputs(hipStream_t s, const g1j *c, const g1j *pi, const fr *ys, const g1j *es, const fr *bs, uint64_t n, g1j *p0, g1j *p1) {
    if (!n) return;
    hipLaunchKernelGGL(k_kzg_check_inputs, pairing_grid(n), dim3(PAIRING_BLOCK), 0, s, c, pi, ys, es, bs, n, p0, p1);
}

// CheckProofMulti's coset scaling over rows (kzg_multi_proofs.go:55-62, as launch_fr_scale_by_inv_powers for one row): row b of c (np values)
// times x_b^-i, and xpow_n[b] = x_b^np.  One lane per row: the row's inversion once, then a running power.
__global__ __launch_bounds__(PAIRING_BLOCK) void k_fr_rows_scale_by_inv_powers(fr *c, uint64_t np, const fr *xs, uint64_t count, fr *xpow_n) {
    const uint64_t t = blockIdx.x * (uint64_t)blockDim.x + threadIdx.x;
    if (t >= count) return;
    const fr x = xs[t], xi = inv<FrP>(x);
    fr acc = one<FrP>(), xp = one<FrP>();
    for (uint64_t i = 0; i < np; i++) { c[t * np + i] = mul(c[t * np + i], acc); acc = mul(acc, xi); xp = mul(xp, x); }
    xpow_n[t] = xp;
}
void launch_fr_rows_scale_by_inv_powers(hipStream_t s, fr *c, uint64_t np, const fr *xs, uint64_t count, fr *xpow_n) {
    if (!count) return;
    hipLaunchKernelGGL(k_fr_rows_scale_by_inv_powers, pairing_grid(count), dim3(PAIRING_BLOCK), 0, s, c, np, xs, count, xpow_n);
}

// eth.VerifyKZGProof's parsing and the G1 inputs of its check (eth_check_inputs_lane, verify_inputs.hpp): status 0 = inputs valid,
// 2 = z or y not below r, 3 = commitment or proof not a valid compressed G1 point.  Invalid rows get points at infinity.
__global__ __launch_bounds__(PAIRING_BLOCK) void k_eth_check_inputs(const uint8_t *c48, const uint8_t *zs, const uint8_t *ys, const uint8_t *pi48, uint64_t n,
                                                                    g1j *p0, g1j *p1, uint8_t *status) {
    const uint64_t t = blockIdx.x * (uint64_t)blockDim.x + threadIdx.x;
    if (t >= n) return;
    eth_check_inputs_lane(c48 + 48 * t, zs + 32 * t, ys + 32 * t, pi48 + 48 * t, p0[t], p1[t], status[t]);
}
void launch_eth_check_inputs(hipStream_t s, const uint8_t *c48, const uint8_t *zs, const uint8_t *ys, const uint8_t *pi48, uint64_t n, g1j *p0, g1j *p1,
                             uint8_t *status) {
    if (!n) return;
    hipLaunchKernelGGL(k_eth_check_inputs, pairing_grid(n), dim3(PAIRING_BLOCK), 0, s, c48, zs, ys, pi48, n, p0, p1, status);
}

// ok[i] = (e(p0[i], Q0) e(p1[i], Q1) == 1).  SHARED: every lane reads the same two prepared points (q0[0], q1[0]; the KZG case, a broadcast
// read); otherwise lane i reads q0[i] and q1[i] (bls.PairingsVerify).  G1 inputs are device-internal Jacobian images.
template <bool SHARED>
__global__ __launch_bounds__(PAIRING_BLOCK) void k_pairing_check(const g2_prepared *q0, const g2_prepared *q1, const g1j *p0, const g1j *p1, uint64_t n,
                                                                 uint8_t *ok) {
    const uint64_t t = blockIdx.x * (uint64_t)blockDim.x + threadIdx.x;
    if (t >= n) return;
    const g2_prepared *q[2] = {SHARED ? q0 : q0 + t, SHARED ? q1 : q1 + t};
    g1j p[2] = {p0[t], p1[t]};
    ok[t] = pairing_product_is_one<2>(q, p) ? 1 : 0;
}
// one wavefront per check (k_pairing_wave.hip) below PAIRING_WAVE_BELOW checks, one lane per check from there on; KZG_HIP_PAIRING forces either
bool pairing_route_is_wave(uint64_t n) {
    const knobs::pairing_mode forced = knobs::pairing();
    return forced == knobs::pairing_mode::by_count ? n < PAIRING_WAVE_BELOW : forced == knobs::pairing_mode::wave;
}
void launch_pairing_check(hipStream_t s, bool shared_lines, const g2_prepared *q0, const g2_prepared *q1, const g1j *p0, const g1j *p1, uint64_t n, uint8_t *ok) {
    if (!n) return;
    if (pairing_route_is_wave(n)) {
        prof_begin(s, "pairing_check_wave");
        launch_pairing_check_wave(s, shared_lines, q0, q1, p0, p1, n, ok);
        prof_end(s, "pairing_check_wave");
        return;
    }
    prof_begin(s, "pairing_check");
    if (shared_lines) hipLaunchKernelGGL(k_pairing_check<true>, pairing_grid(n), dim3(PAIRING_BLOCK), 0, s, q0, q1, p0, p1, n, ok);
    else hipLaunchKernelGGL(k_pairing_check<false>, pairing_grid(n), dim3(PAIRING_BLOCK), 0, s, q0, q1, p0, p1, n, ok);
    prof_end(s, "pairing_check");
}

// test hook: out[i] = e(g1[i], Q_i) (device exponent, pairing.hpp) in STANDARD form, 12 F_p elements in memory order; g1 Kilic images
__global__ __launch_bounds__(PAIRING_BLOCK) void k_pairing_value(const g1j *g1, const g2_prepared *q, uint64_t n, fp *out) {
    const uint64_t t = blockIdx.x * (uint64_t)blockDim.x + threadIdx.x;
    if (t >= n) return;
    const g2_prepared *qs[1] = {q + t};
    g1j p[1] = {g1_from_kilic(g1[t])};
    const fp12 f = final_exponentiation(multi_miller_loop<1>(qs, p));
    const fp *c = &f.c0.c0.c0;
    for (int k = 0; k < 12; k++) out[12 * t + k] = from_mont<FpP>(c[k]);
}
void launch_pairing_value(hipStream_t s, const g1j *g1_kilic, const g2_prepared *q, uint64_t n, fp *out) {
    if (!n) return;
    hipLaunchKernelGGL(k_pairing_value, pairing_grid(n), dim3(PAIRING_BLOCK), 0, s, g1_kilic, q, n, out);
}

}  // namespace kzg
