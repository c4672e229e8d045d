// capi_verify.hip -- C ABI of verification: G2 decompression, batched pairing checks, and the batched KZG / eth proof checks built on them.
// Replaces bls.FromCompressedG2, bls.PairingsVerify, KZGSettings.CheckProofSingle / CheckProofMulti and eth.VerifyKZGProof for BATCHES; a lone
// check is one lane's work and stays on Kilic in the Go shim.
#include "capi_common.hpp"
#include "pairing.hpp"

// G2 points a handle verifies against: the caller's array (Kilic images) and its prepared points, [1]G2 and [s]G2 at once, [s^n]G2 on first use.
// Thread safety: the handle's pointer to its state is read and replaced under the handle's g2_mu (g2_of / g2_state_set); every check holds its
// own std::shared_ptr to the state for the whole call, so a setter that replaces the state never frees what a running check reads.  Within a
// state, d_gen and d_s are written once before the state is published; the map of the other powers only grows, under `mu`, and its entries
// are freed only with the state.
struct g2_state {
    std::vector<g2j> h_g2;
    g2_prepared *d_gen = nullptr;                  // bls.GenG2
    g2_prepared *d_s = nullptr;                    // h_g2[1] = [s]G2 (also d_pow[1])
    std::map<uint64_t, g2_prepared *> d_pow;      // n -> prepared h_g2[n]
    std::mutex mu;
    ~g2_state() {
        hipFree(d_gen);
        for (auto &kv : d_pow) hipFree(kv.second);
        (void)hipGetLastError();
    }
};

namespace {

int prepare_points(hipStream_t s, const g2j *h_kilic, uint64_t n, g2_prepared *d_out) {
    dtmp<g2j> d_in(s);
    CHK(d_in.alloc(n));
    HIPCHK(hipMemcpyAsync(d_in.p, h_kilic, n * sizeof(g2j), hipMemcpyHostToDevice, s));
    launch_g2_prepare(s, d_in.p, n, d_out);
    HIPCHK(hipGetLastError());
    HIPCHK(hipStreamSynchronize(s));
    return KZG_HIP_OK;
}
int prepare_one(hipStream_t s, const g2j &h_kilic, g2_prepared **out) {
    g2_prepared *d = nullptr;
    HIPCHK(hipMalloc((void **)&d, sizeof(g2_prepared)));
    int st = prepare_points(s, &h_kilic, 1, d);
    if (st != KZG_HIP_OK) { hipFree(d); return st; }
    *out = d;
    return KZG_HIP_OK;
}
// the prepared [s^n]G2 of a state (cached; takes g->mu)
int g2_pow(g2_state *g, hipStream_t s, uint64_t n, const g2_prepared **out) {
    std::lock_guard<std::mutex> lk(g->mu);
    auto it = g->d_pow.find(n);
    if (it == g->d_pow.end()) {
        g2_prepared *d = nullptr;
        CHK(prepare_one(s, g->h_g2[n], &d));
        it = g->d_pow.emplace(n, d).first;
    }
    *out = it->second;
    return KZG_HIP_OK;
}
std::shared_ptr<g2_state> g2_of(std::mutex &mu, const std::shared_ptr<g2_state> &slot) {
    std::lock_guard<std::mutex> lk(mu);
    return slot;
}
// builds a new state (the array, [1]G2 and [s]G2 prepared) and publishes it; checks still running keep the old one alive
int g2_state_set(kzg_hip_fft *fs, std::mutex &mu, std::shared_ptr<g2_state> &slot, const void *g2, uint64_t n) {
    if (!g2 || n < 2) return KZG_HIP_ERR_BAD_ARG;
    KZG_TRY
    auto g = std::make_shared<g2_state>();
    g->h_g2.assign((const g2j *)g2, (const g2j *)g2 + n);
    {
        stream_lease lease(fs);
        CHK(prepare_one(lease.s, g2_to_kilic(g2_generator()), &g->d_gen));
        const g2_prepared *ds = nullptr;
        CHK(g2_pow(g.get(), lease.s, 1, &ds));
        g->d_s = const_cast<g2_prepared *>(ds);
    }
    std::lock_guard<std::mutex> lk(mu);
    slot = std::move(g);
    return KZG_HIP_OK;
    KZG_CATCH
}
// ok[i] = e(p0[i], [1]G2) e(p1[i], Q1) == 1 for G1 inputs already on the device
int run_shared_check(hipStream_t s, const g2_prepared *gen, const g2_prepared *q1, const g1j *p0, const g1j *p1, uint64_t n, uint8_t *ok) {
    dtmp<uint8_t> d_ok(s);
    CHK(d_ok.alloc(n));
    launch_pairing_check(s, true, gen, q1, p0, p1, n, d_ok.p);
    HIPCHK(hipGetLastError());
    HIPCHK(hipMemcpyAsync(ok, d_ok.p, n, hipMemcpyDeviceToHost, s));
    HIPCHK(hipStreamSynchronize(s));
    return KZG_HIP_OK;
}
// C - E + [b] pi, -pi for `count` KZG checks (E = [y]G1 from ys, or the points es) and the check against [1]G2, Q1
// single proofs: ys_fr and xs (bs_fr) are host buffers; multi proofs (ys_fr == null): d_es / d_bs are DEVICE buffers on stream s
int kzg_checks(hipStream_t s, const g2_prepared *gen, const g2_prepared *q1, const void *c_g1, const void *pi_g1, const void *ys_fr, const g1j *d_es,
               const void *bs_fr, const fr *d_bs, uint64_t count, uint8_t *ok) {
    dtmp<g1j> d_c(s), d_pi(s), d_p0(s), d_p1(s); dtmp<fr> d_y(s), d_b(s);
    CHK(d_c.alloc(count)); CHK(d_pi.alloc(count)); CHK(d_p0.alloc(count)); CHK(d_p1.alloc(count));
    HIPCHK(hipMemcpyAsync(d_c.p, c_g1, count * sizeof(g1j), hipMemcpyHostToDevice, s));
    HIPCHK(hipMemcpyAsync(d_pi.p, pi_g1, count * sizeof(g1j), hipMemcpyHostToDevice, s));
    if (ys_fr) {
        CHK(d_y.alloc(count)); CHK(d_b.alloc(count));
        HIPCHK(hipMemcpyAsync(d_y.p, ys_fr, count * sizeof(fr), hipMemcpyHostToDevice, s));
        HIPCHK(hipMemcpyAsync(d_b.p, bs_fr, count * sizeof(fr), hipMemcpyHostToDevice, s));
    }
    launch_kzg_check_inputs(s, d_c.p, d_pi.p, ys_fr ? d_y.p : nullptr, d_es, ys_fr ? d_b.p : d_bs, count, d_p0.p, d_p1.p);
    HIPCHK(hipGetLastError());
    return run_shared_check(s, gen, q1, d_p0.p, d_p1.p, count, ok);
}

}  // namespace

extern "C" {

int kzg_hip_g2_from_compressed(kzg_hip_fft *fs, const void *in96, uint64_t n, void *out_g2) {
    if (!fs || (n && (!in96 || !out_g2))) return KZG_HIP_ERR_BAD_ARG;
    if (!n) return KZG_HIP_OK;
    KZG_TRY
    stream_lease lease(fs);
    hipStream_t s = lease.s;
    dtmp<uint8_t> d_in(s); dtmp<g2j> d_out(s); dtmp<uint32_t> d_bad(s);
    CHK(d_in.alloc(96 * n)); CHK(d_out.alloc(n)); CHK(d_bad.alloc(1));
    HIPCHK(hipMemsetAsync(d_bad.p, 0, sizeof(uint32_t), s));
    HIPCHK(hipMemcpyAsync(d_in.p, in96, 96 * n, hipMemcpyHostToDevice, s));
    launch_g2_from_compressed(s, d_in.p, d_out.p, n, d_bad.p);
    HIPCHK(hipGetLastError());
    uint32_t bad = 0;
    HIPCHK(hipMemcpyAsync(&bad, d_bad.p, sizeof bad, hipMemcpyDeviceToHost, s));
    HIPCHK(hipMemcpyAsync(out_g2, d_out.p, n * sizeof(g2j), hipMemcpyDeviceToHost, s));
    HIPCHK(hipStreamSynchronize(s));
    return bad ? KZG_HIP_ERR_BAD_POINT : KZG_HIP_OK;
    KZG_CATCH
}

int kzg_hip_pairings_verify_batch(kzg_hip_fft *fs, const void *a1_g1, const void *a2_g2, const void *b1_g1, const void *b2_g2, uint64_t n, uint8_t *ok) {
    if (!fs || (n && (!a1_g1 || !a2_g2 || !b1_g1 || !b2_g2 || !ok))) return KZG_HIP_ERR_BAD_ARG;
    if (!n) return KZG_HIP_OK;
    KZG_TRY
    stream_lease lease(fs);
    hipStream_t s = lease.s;
    const uint64_t CHUNK = 8192;   // 2 x 8192 prepared points = 320 MB of lines per launch
    dtmp<g1j> d_a(s), d_b(s), d_p0(s), d_p1(s); dtmp<g2j> d_q(s); dtmp<uint8_t> d_ok(s);
    const uint64_t m = n < CHUNK ? n : CHUNK;
    g2_prepared *d_lines = nullptr;
    HIPCHK(hipMalloc((void **)&d_lines, 2 * m * sizeof(g2_prepared)));
    std::unique_ptr<g2_prepared, hipError_t (*)(void *)> own(d_lines, hipFree);
    CHK(d_a.alloc(m)); CHK(d_b.alloc(m)); CHK(d_p0.alloc(m)); CHK(d_p1.alloc(m)); CHK(d_q.alloc(2 * m)); CHK(d_ok.alloc(m));
    for (uint64_t i0 = 0; i0 < n; i0 += m) {
        const uint64_t k = n - i0 < m ? n - i0 : m;
        HIPCHK(hipMemcpyAsync(d_a.p, (const g1j *)a1_g1 + i0, k * sizeof(g1j), hipMemcpyHostToDevice, s));
        HIPCHK(hipMemcpyAsync(d_b.p, (const g1j *)b1_g1 + i0, k * sizeof(g1j), hipMemcpyHostToDevice, s));
        HIPCHK(hipMemcpyAsync(d_q.p, (const g2j *)a2_g2 + i0, k * sizeof(g2j), hipMemcpyHostToDevice, s));
        HIPCHK(hipMemcpyAsync(d_q.p + m, (const g2j *)b2_g2 + i0, k * sizeof(g2j), hipMemcpyHostToDevice, s));
        launch_g2_prepare(s, d_q.p, k, d_lines);
        launch_g2_prepare(s, d_q.p + m, k, d_lines + m);
        launch_pairs_g1_from_kilic(s, d_a.p, d_b.p, k, d_p0.p, d_p1.p);   // e(a1, a2) == e(b1, b2)  <=>  e(-a1, a2) e(b1, b2) == 1
        launch_pairing_check(s, false, d_lines, d_lines + m, d_p0.p, d_p1.p, k, d_ok.p);
        HIPCHK(hipGetLastError());
        HIPCHK(hipMemcpyAsync(ok + i0, d_ok.p, k, hipMemcpyDeviceToHost, s));
        HIPCHK(hipStreamSynchronize(s));
    }
    return KZG_HIP_OK;
    KZG_CATCH
}

int kzg_hip_kzg_set_secret_g2(kzg_hip_kzg *ks, const void *secret_g2, uint64_t n) {
    if (!ks) return KZG_HIP_ERR_BAD_ARG;
    return g2_state_set(ks->fs, ks->g2_mu, ks->g2, secret_g2, n);
}

int kzg_hip_check_proof_single_batch(kzg_hip_kzg *ks, const void *commitments_g1, const void *proofs_g1, const void *xs_fr, const void *ys_fr, uint64_t count,
                                     uint8_t *ok) {
    if (!ks) return KZG_HIP_ERR_BAD_ARG;
    KZG_TRY
    const std::shared_ptr<g2_state> g = g2_of(ks->g2_mu, ks->g2);
    if (!g) return KZG_HIP_ERR_BAD_ARG;
    if (!count) return KZG_HIP_OK;
    if (!commitments_g1 || !proofs_g1 || !xs_fr || !ys_fr || !ok) return KZG_HIP_ERR_BAD_ARG;
    // e(C - [y]G1 + [x] pi, G2) e(-pi, [s]G2) == 1  <=>  e(C - [y]G1, G2) == e(pi, [s - x]G2)  (kzg_single_proofs.go:57-70)
    stream_lease lease(ks->fs);
    return kzg_checks(lease.s, g->d_gen, g->d_s, commitments_g1, proofs_g1, ys_fr, nullptr, xs_fr, nullptr, count, ok);
    KZG_CATCH
}

int kzg_hip_check_proof_multi_batch(kzg_hip_kzg *ks, const void *commitments_g1, const void *proofs_g1, const void *xs_fr, const void *ys_fr, uint64_t n,
                                    uint64_t count, uint8_t *ok) {
    if (!ks) return KZG_HIP_ERR_BAD_ARG;
    KZG_TRY
    const std::shared_ptr<g2_state> g = g2_of(ks->g2_mu, ks->g2);
    if (!g) return KZG_HIP_ERR_BAD_ARG;
    if (!count) return KZG_HIP_OK;
    if (!commitments_g1 || !proofs_g1 || !xs_fr || !ys_fr || !ok || n == 0) return KZG_HIP_ERR_BAD_ARG;
    if (n >= g->h_g2.size()) return KZG_HIP_ERR_LEN_MISMATCH;     // SecretG2[len(ys)]
    kzg_hip_fft *fs = ks->fs;
    if (n > fs->W) return KZG_HIP_ERR_TOO_WIDE;                  // "ys is bad, cannot compute FFT" panic, kzg_multi_proofs.go:50-53
    const uint64_t np = next_pow2(n);
    if (np > ks->n_setup) return KZG_HIP_ERR_LEN_MISMATCH;
    // all rows at once (kzg_hip_check_proof_multi_interpolation's steps over `count` rows): IFFT(ys) per row, coefficients times x^-i, x^np,
    // [I(s)]_1 by the batched commitment; then e(C - [I(s)]_1 + [x^n] pi, G2) e(-pi, [s^n]G2) == 1   (kzg_multi_proofs.go:47-75)
    dev_guard dg(fs);
    hipStream_t s = fs->stream;
    const g2_prepared *qn = nullptr;
    CHK(g2_pow(g.get(), s, n, &qn));
    dtmp<fr> d_ys(s), d_ip(s), d_x(s), d_xp(s); dtmp<g1j> d_is(s);
    CHK(d_ys.alloc(count * n)); CHK(d_ip.alloc(count * np)); CHK(d_x.alloc(count)); CHK(d_xp.alloc(count)); CHK(d_is.alloc(count));
    HIPCHK(hipMemcpyAsync(d_ys.p, ys_fr, count * n * sizeof(fr), hipMemcpyHostToDevice, s));
    HIPCHK(hipMemcpyAsync(d_x.p, xs_fr, count * sizeof(fr), hipMemcpyHostToDevice, s));
    fr_fft_rows(fs, s, d_ys.p, n, n, d_ip.p, np, count, 1);
    launch_fr_rows_scale_by_inv_powers(s, d_ip.p, np, d_x.p, count, d_xp.p);
    CHK(commit_rows(ks, s, d_ip.p, np, count, d_is.p));
    HIPCHK(hipGetLastError());
    return kzg_checks(s, g->d_gen, qn, commitments_g1, proofs_g1, nullptr, d_is.p, nullptr, d_xp.p, count, ok);
    KZG_CATCH
}

int kzg_hip_eth_set_setup_g2(kzg_hip_eth *eth, const void *setup_g2, uint64_t n) {
    if (!eth) return KZG_HIP_ERR_BAD_ARG;
    return g2_state_set(eth->fs, eth->g2_mu, eth->g2, setup_g2, n);
}

int kzg_hip_eth_verify_kzg_proof_batch(kzg_hip_eth *eth, const void *commitments48, const void *zs_le32, const void *ys_le32, const void *proofs48, uint64_t count,
                                       uint8_t *result) {
    if (!eth) return KZG_HIP_ERR_BAD_ARG;
    KZG_TRY
    const std::shared_ptr<g2_state> g = g2_of(eth->g2_mu, eth->g2);
    if (!g) return KZG_HIP_ERR_BAD_ARG;
    if (!count) return KZG_HIP_OK;
    if (!commitments48 || !zs_le32 || !ys_le32 || !proofs48 || !result) return KZG_HIP_ERR_BAD_ARG;
    stream_lease lease(eth->fs);
    hipStream_t s = lease.s;
    dtmp<uint8_t> d_c(s), d_z(s), d_y(s), d_pi(s), d_st(s), d_ok(s); dtmp<g1j> d_p0(s), d_p1(s);
    CHK(d_c.alloc(48 * count)); CHK(d_pi.alloc(48 * count)); CHK(d_z.alloc(32 * count)); CHK(d_y.alloc(32 * count));
    CHK(d_st.alloc(count)); CHK(d_ok.alloc(count)); CHK(d_p0.alloc(count)); CHK(d_p1.alloc(count));
    HIPCHK(hipMemcpyAsync(d_c.p, commitments48, 48 * count, hipMemcpyHostToDevice, s));
    HIPCHK(hipMemcpyAsync(d_pi.p, proofs48, 48 * count, hipMemcpyHostToDevice, s));
    HIPCHK(hipMemcpyAsync(d_z.p, zs_le32, 32 * count, hipMemcpyHostToDevice, s));
    HIPCHK(hipMemcpyAsync(d_y.p, ys_le32, 32 * count, hipMemcpyHostToDevice, s));
    launch_eth_check_inputs(s, d_c.p, d_z.p, d_y.p, d_pi.p, count, d_p0.p, d_p1.p, d_st.p);
    // e(C - [y]G1 + [z] pi, G2) e(-pi, kzgSetupG2[1]) == 1  <=>  e(C - [y]G1, G2) == e(pi, [s - z]G2)  (eth/helpers.go:55-68)
    launch_pairing_check(s, true, g->d_gen, g->d_s, d_p0.p, d_p1.p, count, d_ok.p);
    HIPCHK(hipGetLastError());
    std::vector<uint8_t> st(count);
    HIPCHK(hipMemcpyAsync(st.data(), d_st.p, count, hipMemcpyDeviceToHost, s));
    HIPCHK(hipMemcpyAsync(result, d_ok.p, count, hipMemcpyDeviceToHost, s));
    HIPCHK(hipStreamSynchronize(s));
    for (uint64_t i = 0; i < count; i++) if (st[i]) result[i] = st[i];
    return KZG_HIP_OK;
    KZG_CATCH
}

// test hook (kzg_hip_internal.h): out[i] = reduced e(g1[i], g2[i]) as 12 standard-form F_p elements
int kzg_hip_pairing_test(kzg_hip_fft *fs, const void *g1, const void *g2, uint64_t n, void *out_fp12) {
    if (!fs || (n && (!g1 || !g2 || !out_fp12))) return KZG_HIP_ERR_BAD_ARG;
    if (!n) return KZG_HIP_OK;
    KZG_TRY
    stream_lease lease(fs);
    hipStream_t s = lease.s;
    dtmp<g1j> d_p(s); dtmp<g2j> d_q(s); dtmp<fp> d_out(s);
    CHK(d_p.alloc(n)); CHK(d_q.alloc(n)); CHK(d_out.alloc(12 * n));
    g2_prepared *d_lines = nullptr;
    HIPCHK(hipMalloc((void **)&d_lines, n * sizeof(g2_prepared)));
    std::unique_ptr<g2_prepared, hipError_t (*)(void *)> own(d_lines, hipFree);
    HIPCHK(hipMemcpyAsync(d_p.p, g1, n * sizeof(g1j), hipMemcpyHostToDevice, s));
    HIPCHK(hipMemcpyAsync(d_q.p, g2, n * sizeof(g2j), hipMemcpyHostToDevice, s));
    launch_g2_prepare(s, d_q.p, n, d_lines);
    launch_pairing_value(s, d_p.p, d_lines, n, d_out.p);
    HIPCHK(hipGetLastError());
    HIPCHK(hipMemcpyAsync(out_fp12, d_out.p, 12 * n * sizeof(fp), hipMemcpyDeviceToHost, s));
    HIPCHK(hipStreamSynchronize(s));
    return KZG_HIP_OK;
    KZG_CATCH
}

}  // extern "C"
