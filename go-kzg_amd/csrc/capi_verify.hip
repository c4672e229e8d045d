// capi_verify.hip -- C ABI of verification: G2 decompression, batched pairing checks, and the batched KZG / eth proof checks built on them.
// Replaces bls.FromCompressedG2, bls.PairingsVerify, KZGSettings.CheckProofSingle / CheckProofMulti and eth.VerifyKZGProof for BATCHES; a lone
// check is one lane's work and stays on Kilic in the Go shim.
#include "capi_common.hpp"
#include "pairing.hpp"
#include "sha256_lane.hpp"
#include "verify_combine_multi.hpp"
#include <random>
#include <sys/random.h>

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
    CHK(upload(d_in, h_kilic, n));
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
// the handle's fixed-base table of bls.GenG2, built once on the handle's stream; the caller holds fs->mu (dev_guard)
int ensure_g2_table(kzg_hip_fft *fs) {
    if (fs->d_g2_fb) return KZG_HIP_OK;
    g2a *t = nullptr;
    HIPCHK(hipMalloc((void **)&t, G2_FB_ENTRIES * sizeof(g2a)));
    launch_g2_fixed_base_table(fs->stream, t);
    hipError_t e = hipGetLastError();
    if (e == hipSuccess) e = hipStreamSynchronize(fs->stream);
    if (e != hipSuccess) { (void)hipFree(t); HIPCHK(e); }
    fs->d_g2_fb = t; fs->g2_fb_builds++;
    return KZG_HIP_OK;
}
// out[i] = [k_i] G2 as normalised Kilic images, k = the n scalars at scalars_fr, or the powers secret^0 .. secret^(n - 1) when powers_of_one
int g2_mul_generator(kzg_hip_fft *fs, const void *scalars_fr, bool powers_of_one, uint64_t n, void *out_g2) {
    dev_guard g(fs);
    hipStream_t s = fs->stream;
    CHK(ensure_g2_table(fs));
    dtmp<g2j> d_a(s), d_b(s); dtmp<fr> d_k(s), d_s(s);
    CHK(d_a.alloc(n)); CHK(d_b.alloc(n)); CHK(d_k.alloc(n));
    if (powers_of_one) {
        CHK(upload(d_s, scalars_fr, 1));
        launch_fr_powers(s, d_s.p, n, d_k.p);
    } else {
        HIPCHK(hipMemcpyAsync(d_k.p, scalars_fr, n * sizeof(fr), hipMemcpyHostToDevice, s));
    }
    launch_g2_fixed_base(s, d_k.p, n, fs->d_g2_fb, d_a.p);
    launch_g2_normalize(s, d_a.p, n, d_b.p);
    HIPCHK(hipGetLastError());
    HIPCHK(hipMemcpyAsync(out_g2, d_b.p, n * sizeof(g2j), hipMemcpyDeviceToHost, s));
    HIPCHK(hipStreamSynchronize(s));
    return KZG_HIP_OK;
}
// C - E + [b] pi, -pi for `count` KZG checks (E = [y]G1 from ys, or the points es) and the check against [1]G2, Q1
// single proofs: ys_fr and xs (bs_fr) are host buffers; multi proofs (ys_fr == null): d_es / d_bs are DEVICE buffers on stream s
int kzg_checks(hipStream_t s, const g2_prepared *gen, const g2_prepared *q1, const void *c_g1, const void *pi_g1, const void *ys_fr, const g1j *d_es,
               const void *bs_fr, const fr *d_bs, uint64_t count, uint8_t *ok) {
    dtmp<g1j> d_c(s), d_pi(s), d_p0(s), d_p1(s); dtmp<fr> d_y(s), d_b(s);
    CHK(upload(d_c, c_g1, count)); CHK(upload(d_pi, pi_g1, count)); CHK(d_p0.alloc(count)); CHK(d_p1.alloc(count));
    if (ys_fr) { CHK(upload(d_y, ys_fr, count)); CHK(upload(d_b, bs_fr, count)); }
    launch_kzg_check_inputs(s, d_c.p, d_pi.p, ys_fr ? d_y.p : nullptr, d_es, ys_fr ? d_b.p : d_bs, count, d_p0.p, d_p1.p);
    HIPCHK(hipGetLastError());
    return run_shared_check(s, gen, q1, d_p0.p, d_p1.p, count, ok);
}

// eth.VerifyKZGProof over `count` rows of bytes, one pairing check per row: result[i] = 1 / 0, or the row's status 2 / 3
int eth_checks(hipStream_t s, const g2_prepared *gen, const g2_prepared *q1, const void *commitments48, const void *zs_le32, const void *ys_le32, const void *proofs48,
               uint64_t count, uint8_t *result) {
    dtmp<uint8_t> d_c(s), d_z(s), d_y(s), d_pi(s), d_st(s), d_ok(s); dtmp<g1j> d_p0(s), d_p1(s);
    CHK(upload(d_c, commitments48, 48 * count)); CHK(upload(d_pi, proofs48, 48 * count)); CHK(upload(d_z, zs_le32, 32 * count)); CHK(upload(d_y, ys_le32, 32 * count));
    CHK(d_st.alloc(count)); CHK(d_ok.alloc(count)); CHK(d_p0.alloc(count)); CHK(d_p1.alloc(count));
    launch_eth_check_inputs(s, d_c.p, d_z.p, d_y.p, d_pi.p, count, d_p0.p, d_p1.p, d_st.p);
    // e(C - [y]G1 + [z] pi, G2) e(-pi, kzgSetupG2[1]) == 1  <=>  e(C - [y]G1, G2) == e(pi, [s - z]G2)  (eth/helpers.go:55-68)
    launch_pairing_check(s, true, gen, q1, d_p0.p, d_p1.p, count, d_ok.p);
    HIPCHK(hipGetLastError());
    std::vector<uint8_t> st(count);
    HIPCHK(hipMemcpyAsync(st.data(), d_st.p, count, hipMemcpyDeviceToHost, s));
    HIPCHK(hipMemcpyAsync(result, d_ok.p, count, hipMemcpyDeviceToHost, s));
    HIPCHK(hipStreamSynchronize(s));
    for (uint64_t i = 0; i < count; i++) if (st[i]) result[i] = st[i];
    return KZG_HIP_OK;
}

// ---- batches by random linear combination per group of consecutive rows (verify_combine.hpp, k_verify_combine.hip) ----
// From this many rows on the _combined entries combine by default (KZG_HIP_VERIFY_COMBINE = never / always forces a route): the smallest measured
// count from which the combined route is faster on all-valid rows by more than the spread of the repeats.  Measured at 1 024 rows and up
// (profiles/verify_combine.md): 7.7 .. 8.3 against 9.9 ms at 1 024 rows (one group), 12.3 against 66.2 ms at 65 536; below one full group nothing was measured.
constexpr uint64_t COMBINE_FROM = 1024;
constexpr uint64_t COMBINE_CHUNK_GROUPS = 1024;             // group checks per launch: the flat stretch of the wavefront pairing kernel
constexpr uint64_t COMBINE_CHUNK_BYTES = 2048ull << 20;     // ... fewer when the groups' MSM workspaces would exceed this

// what the last _combined call on this thread did (kzg_hip_test_combine_stats)
thread_local combine_stats t_combine;

bool combine_route(uint64_t count) {
    const knobs::combine_mode m = knobs::verify_combine();
    return m == knobs::combine_mode::by_count ? count >= COMBINE_FROM : m == knobs::combine_mode::always;
}
uint64_t combine_rows() {
    const uint64_t r = knobs::verify_combine_rows();
    return !r ? VERIFY_COMBINE_ROWS : r > VERIFY_COMBINE_ROWS_MAX ? VERIFY_COMBINE_ROWS_MAX : r;
}
// groups of R rows one chunk of a call holds
uint64_t combine_chunk_groups(uint64_t R) {
    const uint64_t per = msm_workspace_bytes(classic_plan(combine_term_stride(R)), combine_term_stride(R), 1);
    const uint64_t fit = COMBINE_CHUNK_BYTES / per;
    return fit < 1 ? 1 : fit > COMBINE_CHUNK_GROUPS ? COMBINE_CHUNK_GROUPS : fit;
}
// the caller's seed, or 32 bytes from the operating system
combine_seed combine_seed_of(const uint8_t *seed32) {
    uint8_t buf[32];
    if (!seed32) {
        size_t got = 0;
        while (got < sizeof buf) {
            const ssize_t k = getrandom(buf + got, sizeof buf - got, 0);
            if (k <= 0) break;
            got += (size_t)k;
        }
        if (got < sizeof buf) {
            std::random_device rd;
            for (size_t i = 0; i < sizeof buf; i += 4) { const uint32_t v = rd(); memcpy(buf + i, &v, 4); }
        }
        seed32 = buf;
    }
    return combine_seed_from_bytes(seed32);
}
// A_g and B_g of the groups of `count` device-resident rows (rows row0 .. of the call): c / pi Kilic images (kilic) or device-internal ones,
// x / y Montgomery images, status nullable.  d_a / d_b: combine_group_count(count, R) normalised points, Kilic images when to_kilic.
int combine_group_msms(hipStream_t s, const g1j *d_c, const g1j *d_pi, bool kilic, const g1j *d_last, const fr *d_sc, uint64_t count, uint64_t R, g1j *d_a, g1j *d_b,
                       bool to_kilic);
int combine_group_sums(hipStream_t s, const combine_seed &seed, const g1j *d_c, const g1j *d_pi, bool kilic, const fr *d_x, const fr *d_y, const uint8_t *d_status,
                       uint64_t row0, uint64_t count, uint64_t R, g1j *d_a, g1j *d_b, bool to_kilic) {
    const uint64_t stride = combine_term_stride(R), total = combine_group_count(count, R) * stride;
    if (!msm_index_range_ok(classic_plan(stride), stride)) return KZG_HIP_ERR_TOO_WIDE;
    dtmp<fr> d_sc(s);
    CHK(d_sc.alloc(total));
    prof_begin(s, "combine_scalars");
    launch_combine_scalars(s, seed, d_x, d_y, d_status, row0, count, R, d_sc.p);
    prof_end(s, "combine_scalars");
    return combine_group_msms(s, d_c, d_pi, kilic, nullptr, d_sc.p, count, R, d_a, d_b, to_kilic);
}
// the two MSMs of every group from its term scalars d_sc (combine_term_stride(R) per group): the points of every slice -- d_last (nullable): the
// point of slot 2 R per group in the form of c and pi, null: the generator -- then B_g over the whole slice and A_g over the proofs
int combine_group_msms(hipStream_t s, const g1j *d_c, const g1j *d_pi, bool kilic, const g1j *d_last, const fr *d_sc, uint64_t count, uint64_t R, g1j *d_a, g1j *d_b,
                       bool to_kilic) {
    const uint64_t G = combine_group_count(count, R), stride = combine_term_stride(R), total = G * stride;
    const msm_plan pb = classic_plan(stride), pa = classic_plan(R);
    if (!msm_index_range_ok(pb, stride)) return KZG_HIP_ERR_TOO_WIDE;
    dtmp<g1j> d_pts(s); dtmp<g1a> d_aff(s); dtmp<uint8_t> d_ws(s);
    CHK(d_pts.alloc(total)); CHK(d_aff.alloc(total)); CHK(d_ws.alloc(msm_workspace_bytes(pb, stride, G)));
    launch_combine_points(s, d_c, d_pi, count, R, kilic, d_pts.p, d_last);
    if (kilic) launch_g1_from_kilic(s, d_pts.p, total);
    launch_g1_to_affine(s, d_pts.p, d_aff.p, total);
    prof_begin(s, "combine_msm");
    launch_msm(s, pb, d_aff.p, d_sc, stride, stride, G, d_ws.p, d_b, to_kilic, stride, true);       // B_g: the whole slice
    launch_msm(s, pa, d_aff.p + R, d_sc, stride, R, G, d_ws.p, d_a, to_kilic, stride, true);        // A_g: the proofs with the weights
    prof_end(s, "combine_msm");
    HIPCHK(hipGetLastError());
    return KZG_HIP_OK;
}
// ok[g] = e(B_g, [1]G2) e(-A_g, [s]G2) == 1 over G groups, downloaded (the stream is synchronised)
int combine_group_checks(hipStream_t s, const g2_prepared *gen, const g2_prepared *q1, const g1j *d_a, const g1j *d_b, uint64_t G, uint8_t *h_ok) {
    dtmp<g1j> d_p1(s);
    CHK(d_p1.alloc(G));
    launch_combine_negate(s, d_a, G, d_p1.p);
    return run_shared_check(s, gen, q1, d_b, d_p1.p, G, h_ok);
}
// one chunk of whole groups from host rows of CheckProofSingle: upload, sums.  d_a / d_b: G points
int combine_single_chunk(hipStream_t s, const combine_seed &seed, const g1j *c, const g1j *pi, const fr *xs, const fr *ys, uint64_t row0, uint64_t k, uint64_t R, g1j *d_a,
                         g1j *d_b, bool to_kilic) {
    dtmp<g1j> d_c(s), d_pi(s); dtmp<fr> d_x(s), d_y(s);
    CHK(upload(d_c, c, k)); CHK(upload(d_pi, pi, k)); CHK(upload(d_x, xs, k)); CHK(upload(d_y, ys, k));
    return combine_group_sums(s, seed, d_c.p, d_pi.p, true, d_x.p, d_y.p, nullptr, row0, k, R, d_a, d_b, to_kilic);
}

// ---- the multi-proof form (verify_combine_multi.hpp, k_verify_combine_multi.hip) ----
// KZGSettings.CheckProofMulti over `count` host rows of n values, one pairing check per row: IFFT(ys) per row, coefficients times x^-i, x^np,
// [I(s)]_1 by the batched commitment; then e(C - [I(s)]_1 + [x^np] pi, G2) e(-pi, [s^n]G2) == 1 (kzg_multi_proofs.go:47-75).  The caller
// holds the handle's mutex, s is the handle's stream, qn the prepared SecretG2[n].
int multi_checks(kzg_hip_kzg *ks, hipStream_t s, const g2_prepared *gen, const g2_prepared *qn, const void *commitments_g1, const void *proofs_g1, const void *xs_fr,
                 const void *ys_fr, uint64_t n, uint64_t np, uint64_t count, uint8_t *ok) {
    dtmp<fr> d_ys(s), d_ip(s), d_x(s), d_xp(s); dtmp<g1j> d_is(s);
    CHK(upload(d_ys, ys_fr, count * n)); CHK(upload(d_x, xs_fr, count)); CHK(d_ip.alloc(count * np)); CHK(d_xp.alloc(count)); CHK(d_is.alloc(count));
    fr_fft_rows(ks->fs, s, d_ys.p, n, n, d_ip.p, np, count, 1);
    launch_fr_rows_scale_by_inv_powers(s, d_ip.p, np, d_x.p, count, d_xp.p);
    CHK(commit_rows(ks, s, d_ip.p, np, count, d_is.p));
    HIPCHK(hipGetLastError());
    return kzg_checks(s, gen, qn, commitments_g1, proofs_g1, nullptr, d_is.p, nullptr, d_xp.p, count, ok);
}
// From this many rows on kzg_hip_check_proof_multi_batch_combined combines by default: the smallest measured count from which the combined
// route is faster on all-valid rows at n = 16 AND n = 64 by more than the spread of the repeats (profiles/verify_combine_multi.md; per-row
// against combined, best .. worst ms).  4 096 rows: 14.4 .. 14.4 against 9.7 .. 9.8 (n = 16), 14.9 .. 15.0 against 10.2 .. 10.4 (n = 64);
// 65 536: 83.4 against 13.2, 88.6 against 15.7.  Not at 1 024 rows (one group): 8.65 .. 8.71 against 8.74 .. 9.60 and 8.96 .. 8.99 against
// 9.11 .. 9.31, nor at 64 and 256 rows (7.2 .. 7.6 against 7.8 .. 8.9).
constexpr uint64_t COMBINE_MULTI_FROM = 4096;

bool combine_multi_route(uint64_t n, uint64_t count) {
    if (next_pow2(n) > COMBINE_MULTI_NP_MAX) return false;        // a lane of k_combine_multi_poly keeps one coefficient index
    const knobs::combine_mode m = knobs::verify_combine();
    return m == knobs::combine_mode::by_count ? count >= COMBINE_MULTI_FROM : m == knobs::combine_mode::always;
}
// groups of R rows of n values one chunk of a call holds: the rows' values and coefficients count against COMBINE_CHUNK_BYTES too
uint64_t combine_multi_chunk_groups(uint64_t R, uint64_t n, uint64_t np) {
    const uint64_t per = msm_workspace_bytes(classic_plan(combine_term_stride(R)), combine_term_stride(R), 1) + msm_workspace_bytes(classic_plan(np), np, 1) +
                         R * (n + np) * sizeof(fr);
    const uint64_t fit = COMBINE_CHUNK_BYTES / per, most = combine_chunk_groups(R);
    return fit < 1 ? 1 : fit > most ? most : fit;
}
// A_g and B_g of the groups of `count` device-resident rows (rows row0 .. of the call): c / pi Kilic images, x Montgomery images, d_coef the
// inverse transform of the rows' values (np each).  d_j: G x np, receives J_g.  [J_g(s)]_1 is a bucket MSM over the resident affine setup
// points: no commitment table is built or read.
int combine_multi_group_sums(kzg_hip_kzg *ks, hipStream_t s, const combine_seed &seed, const g1j *d_c, const g1j *d_pi, const fr *d_x, const fr *d_coef, uint64_t np,
                             uint64_t row0, uint64_t count, uint64_t R, fr *d_j, g1j *d_a, g1j *d_b, bool to_kilic) {
    const uint64_t G = combine_group_count(count, R), stride = combine_term_stride(R);
    const msm_plan pj = classic_plan(np);
    if (!msm_index_range_ok(classic_plan(stride), stride) || !msm_index_range_ok(pj, np)) return KZG_HIP_ERR_TOO_WIDE;
    dtmp<fr> d_sc(s), d_part(s); dtmp<g1j> d_js(s); dtmp<uint8_t> d_ws(s);
    CHK(d_sc.alloc(G * stride)); CHK(d_part.alloc(G * combine_multi_tiles(R) * np)); CHK(d_js.alloc(G)); CHK(d_ws.alloc(msm_workspace_bytes(pj, np, G)));
    prof_begin(s, "combine_multi_scalars");
    launch_combine_multi_scalars(s, seed, d_x, d_coef, np, row0, count, R, d_sc.p, d_part.p, d_j);
    prof_end(s, "combine_multi_scalars");
    launch_msm(s, pj, ks->d_secret_a, d_j, np, np, G, d_ws.p, d_js.p, true);                           // [J_g(s)]_1 as Kilic images, the form of c and pi
    HIPCHK(hipGetLastError());
    return combine_group_msms(s, d_c, d_pi, true, d_js.p, d_sc.p, count, R, d_a, d_b, to_kilic);
}
// one chunk of whole groups from host rows: upload, inverse transform, sums.  d_a / d_b: G points, d_j: G x np scalars
int combine_multi_chunk(kzg_hip_kzg *ks, hipStream_t s, const combine_seed &seed, const g1j *c, const g1j *pi, const fr *xs, const fr *ys, uint64_t n, uint64_t np,
                        uint64_t row0, uint64_t k, uint64_t R, fr *d_j, g1j *d_a, g1j *d_b, bool to_kilic) {
    dtmp<g1j> d_c(s), d_pi(s); dtmp<fr> d_x(s), d_ys(s), d_ip(s);
    CHK(upload(d_c, c, k)); CHK(upload(d_pi, pi, k)); CHK(upload(d_x, xs, k)); CHK(upload(d_ys, ys, k * n)); CHK(d_ip.alloc(k * np));
    fr_fft_rows(ks->fs, s, d_ys.p, n, n, d_ip.p, np, k, 1);
    return combine_multi_group_sums(ks, s, seed, d_c.p, d_pi.p, d_x.p, d_ip.p, np, row0, k, R, d_j, d_a, d_b, to_kilic);
}
// what both CheckProofMulti entries ask of a call with rows, in the per-row entry's order; *np = the padded length of a row's values
int multi_batch_args(const kzg_hip_kzg *ks, const g2_state *g, const void *commitments_g1, const void *proofs_g1, const void *xs_fr, const void *ys_fr, const uint8_t *ok,
                     uint64_t n, uint64_t *np) {
    if (!commitments_g1 || !proofs_g1 || !xs_fr || !ys_fr || !ok || n == 0) return KZG_HIP_ERR_BAD_ARG;
    if (n >= g->h_g2.size()) return KZG_HIP_ERR_LEN_MISMATCH;     // SecretG2[len(ys)]
    if (n > ks->fs->W) return KZG_HIP_ERR_TOO_WIDE;              // "ys is bad, cannot compute FFT" panic, kzg_multi_proofs.go:50-53
    *np = next_pow2(n);
    return *np > ks->n_setup ? KZG_HIP_ERR_LEN_MISMATCH : KZG_HIP_OK;
}

}  // namespace

int eth_g2_lines(kzg_hip_eth *eth, std::shared_ptr<g2_state> &hold, const g2_prepared **gen, const g2_prepared **s1) {
    hold = g2_of(eth->g2_mu, eth->g2);
    if (!hold) return KZG_HIP_ERR_BAD_ARG;
    *gen = hold->d_gen; *s1 = hold->d_s;
    return KZG_HIP_OK;
}
void eth_g2_release_passed(kzg_hip_eth *eth, bool all) {
    std::vector<std::shared_ptr<g2_state>> passed;   // let go after the lock, on this thread
    {
        std::lock_guard<std::mutex> lk(eth->g2_mu);
        auto &q = eth->g2_queued;
        size_t keep = 0;
        for (auto &e : q) {
            if (all || hipEventQuery(e.first) == hipSuccess) { (void)hipEventDestroy(e.first); passed.push_back(std::move(e.second)); }
            else { if (&q[keep] != &e) q[keep] = std::move(e); keep++; }
        }
        q.resize(keep);
        (void)hipGetLastError();                     // (hipErrorNotReady of a query)
    }
}
int eth_g2_hold_on_stream(kzg_hip_eth *eth, hipStream_t s, const std::shared_ptr<g2_state> &hold) {
    eth_g2_release_passed(eth);
    std::lock_guard<std::mutex> lk(eth->g2_mu);
    auto &q = eth->g2_queued;
    hipError_t e;
    if (!q.empty() && q.back().second == hold) {
        e = hipEventRecord(q.back().first, s);       // the same state again: its event moves behind the new kernels (one stream, in order)
        if (e != hipSuccess) { (void)hipStreamSynchronize(s); HIPCHK(e); }   // (the entry stays: its event is at an earlier point or this one)
        return KZG_HIP_OK;
    }
    hipEvent_t ev = nullptr;
    e = hipEventCreateWithFlags(&ev, hipEventDisableTiming);
    if (e == hipSuccess && (e = hipEventRecord(ev, s)) != hipSuccess) (void)hipEventDestroy(ev);
    if (e != hipSuccess) { (void)hipStreamSynchronize(s); HIPCHK(e); }
    q.emplace_back(ev, hold);
    return KZG_HIP_OK;
}

extern "C" {

int kzg_hip_g2_from_compressed(kzg_hip_fft *fs, const void *in96, uint64_t n, void *out_g2) {
    if (!fs || (n && (!in96 || !out_g2))) return KZG_HIP_ERR_BAD_ARG;
    if (!n) return KZG_HIP_OK;
    KZG_TRY
    stream_lease lease(fs);
    hipStream_t s = lease.s;
    dtmp<uint8_t> d_in(s); dtmp<g2j> d_out(s); dtmp<uint32_t> d_bad(s);
    CHK(upload(d_in, in96, 96 * n)); CHK(d_out.alloc(n)); CHK(d_bad.alloc(1));
    HIPCHK(hipMemsetAsync(d_bad.p, 0, sizeof(uint32_t), s));
    launch_g2_from_compressed(s, d_in.p, d_out.p, n, d_bad.p);
    HIPCHK(hipGetLastError());
    uint32_t bad = 0;
    HIPCHK(hipMemcpyAsync(&bad, d_bad.p, sizeof bad, hipMemcpyDeviceToHost, s));
    HIPCHK(hipMemcpyAsync(out_g2, d_out.p, n * sizeof(g2j), hipMemcpyDeviceToHost, s));
    HIPCHK(hipStreamSynchronize(s));
    return bad ? KZG_HIP_ERR_BAD_POINT : KZG_HIP_OK;
    KZG_CATCH
}

int kzg_hip_g2_mul_generator_vec(kzg_hip_fft *fs, const void *scalars_fr, uint64_t n, void *out_g2) {
    if (!fs || (n && (!scalars_fr || !out_g2))) return KZG_HIP_ERR_BAD_ARG;
    if (!n) return KZG_HIP_OK;
    KZG_TRY
    return g2_mul_generator(fs, scalars_fr, false, n, out_g2);
    KZG_CATCH
}
int kzg_hip_generate_testing_setup_g2(kzg_hip_fft *fs, const void *secret_fr, uint64_t n, void *out_g2) {
    if (!fs || !secret_fr || (n && !out_g2)) return KZG_HIP_ERR_BAD_ARG;
    if (!n) return KZG_HIP_OK;
    KZG_TRY
    return g2_mul_generator(fs, secret_fr, true, n, out_g2);
    KZG_CATCH
}
int kzg_hip_g2_to_compressed(kzg_hip_fft *fs, const void *points_g2, uint64_t n, void *out96) {
    if (!fs || (n && (!points_g2 || !out96))) return KZG_HIP_ERR_BAD_ARG;
    if (!n) return KZG_HIP_OK;
    KZG_TRY
    stream_lease lease(fs);
    hipStream_t s = lease.s;
    dtmp<g2j> d_in(s); dtmp<uint8_t> d_out(s);
    CHK(upload(d_in, points_g2, n)); CHK(d_out.alloc(96 * n));
    launch_g2_compress(s, d_in.p, n, d_out.p);
    HIPCHK(hipGetLastError());
    HIPCHK(hipMemcpyAsync(out96, d_out.p, 96 * n, hipMemcpyDeviceToHost, s));
    HIPCHK(hipStreamSynchronize(s));
    return KZG_HIP_OK;
    KZG_CATCH
}
// test hook (kzg_hip_internal.h): how many times this handle built its table of bls.GenG2 (0 before the first use, then 1)
int kzg_hip_test_g2_table_builds(kzg_hip_fft *fs, uint64_t *builds) {
    if (!fs || !builds) return KZG_HIP_ERR_BAD_ARG;
    std::lock_guard<std::mutex> lk(fs->mu);
    *builds = fs->g2_fb_builds;
    return KZG_HIP_OK;
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
    uint64_t np = 0;
    CHK(multi_batch_args(ks, g.get(), commitments_g1, proofs_g1, xs_fr, ys_fr, ok, n, &np));
    // all rows at once (kzg_hip_check_proof_multi_interpolation's steps over `count` rows, multi_checks)
    dev_guard dg(ks->fs);
    hipStream_t s = ks->fs->stream;
    const g2_prepared *qn = nullptr;
    CHK(g2_pow(g.get(), s, n, &qn));
    return multi_checks(ks, s, g->d_gen, qn, commitments_g1, proofs_g1, xs_fr, ys_fr, n, np, count, ok);
    KZG_CATCH
}

// CheckProofMulti over `count` rows with one pairing check per group of rows (verify_combine_multi.hpp); the rows of a failing group are
// re-checked one by one.  The handle's stream under its mutex, as the per-row entry: g2_pow caches the prepared SecretG2[n] on the state.
int kzg_hip_check_proof_multi_batch_combined(kzg_hip_kzg *ks, const void *commitments_g1, const void *proofs_g1, const void *xs_fr, const void *ys_fr, uint64_t n,
                                             uint64_t count, const uint8_t *seed32, uint8_t *ok) {
    if (!ks) return KZG_HIP_ERR_BAD_ARG;
    KZG_TRY
    const std::shared_ptr<g2_state> g = g2_of(ks->g2_mu, ks->g2);
    if (!g) return KZG_HIP_ERR_BAD_ARG;
    if (!count) return KZG_HIP_OK;
    uint64_t np = 0;
    CHK(multi_batch_args(ks, g.get(), commitments_g1, proofs_g1, xs_fr, ys_fr, ok, n, &np));
    t_combine = combine_stats{};
    dev_guard dg(ks->fs);
    hipStream_t s = ks->fs->stream;
    const g2_prepared *qn = nullptr;
    CHK(g2_pow(g.get(), s, n, &qn));
    if (!combine_multi_route(n, count)) return multi_checks(ks, s, g->d_gen, qn, commitments_g1, proofs_g1, xs_fr, ys_fr, n, np, count, ok);
    t_combine.route = 1;
    const combine_seed seed = combine_seed_of(seed32);
    const uint64_t R = combine_rows();
    const g1j *c = (const g1j *)commitments_g1, *pi = (const g1j *)proofs_g1; const fr *xs = (const fr *)xs_fr, *ys = (const fr *)ys_fr;
    return combine_drive(count, R, combine_multi_chunk_groups(R, n, np) * R, ok, t_combine,
        [&](uint64_t i0, uint64_t k, uint64_t G, uint8_t *, uint8_t *gok) -> int {
            dtmp<g1j> d_a(s), d_b(s); dtmp<fr> d_j(s);
            CHK(d_a.alloc(G)); CHK(d_b.alloc(G)); CHK(d_j.alloc(G * np));
            CHK(combine_multi_chunk(ks, s, seed, c + i0, pi + i0, xs + i0, ys + i0 * n, n, np, i0, k, R, d_j.p, d_a.p, d_b.p, false));
            return combine_group_checks(s, g->d_gen, qn, d_a.p, d_b.p, G, gok);
        },
        [&](uint64_t b, uint64_t e) { return multi_checks(ks, s, g->d_gen, qn, c + b, pi + b, xs + b, ys + b * n, n, np, e - b, ok + b); });
    KZG_CATCH
}

int kzg_hip_eth_set_setup_g2(kzg_hip_eth *eth, const void *setup_g2, uint64_t n) {
    if (!eth) return KZG_HIP_ERR_BAD_ARG;
    int st = g2_state_set(eth->fs, eth->g2_mu, eth->g2, setup_g2, n);
    hipSetDevice(eth->fs->device);
    eth_g2_release_passed(eth);   // (earlier states that queued _dev calls have finished with)
    return st;
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
    return eth_checks(lease.s, g->d_gen, g->d_s, commitments48, zs_le32, ys_le32, proofs48, count, result);
    KZG_CATCH
}

// CheckProofSingle over `count` rows with one pairing check per group of rows (verify_combine.hpp); the rows of a failing group are re-checked one by one
int kzg_hip_check_proof_single_batch_combined(kzg_hip_kzg *ks, const void *commitments_g1, const void *proofs_g1, const void *xs_fr, const void *ys_fr, uint64_t count,
                                              const uint8_t *seed32, uint8_t *ok) {
    if (!ks) return KZG_HIP_ERR_BAD_ARG;
    KZG_TRY
    const std::shared_ptr<g2_state> g = g2_of(ks->g2_mu, ks->g2);
    if (!g) return KZG_HIP_ERR_BAD_ARG;
    if (!count) return KZG_HIP_OK;
    if (!commitments_g1 || !proofs_g1 || !xs_fr || !ys_fr || !ok) return KZG_HIP_ERR_BAD_ARG;
    t_combine = combine_stats{};
    stream_lease lease(ks->fs);
    hipStream_t s = lease.s;
    if (!combine_route(count)) return kzg_checks(s, g->d_gen, g->d_s, commitments_g1, proofs_g1, ys_fr, nullptr, xs_fr, nullptr, count, ok);
    t_combine.route = 1;
    const combine_seed seed = combine_seed_of(seed32);
    const uint64_t R = combine_rows();
    const g1j *c = (const g1j *)commitments_g1, *pi = (const g1j *)proofs_g1; const fr *xs = (const fr *)xs_fr, *ys = (const fr *)ys_fr;
    return combine_drive(count, R, combine_chunk_groups(R) * R, ok, t_combine,
        [&](uint64_t i0, uint64_t k, uint64_t G, uint8_t *, uint8_t *gok) -> int {
            dtmp<g1j> d_a(s), d_b(s);
            CHK(d_a.alloc(G)); CHK(d_b.alloc(G));
            CHK(combine_single_chunk(s, seed, c + i0, pi + i0, xs + i0, ys + i0, i0, k, R, d_a.p, d_b.p, false));
            return combine_group_checks(s, g->d_gen, g->d_s, d_a.p, d_b.p, G, gok);
        },
        [&](uint64_t b, uint64_t e) { return kzg_checks(s, g->d_gen, g->d_s, c + b, pi + b, ys + b, nullptr, xs + b, nullptr, e - b, ok + b); });
    KZG_CATCH
}

// eth.VerifyKZGProof over `count` rows of bytes likewise: rows with status 2 or 3 keep that byte and drop out of their group's combination
int kzg_hip_eth_verify_kzg_proof_batch_combined(kzg_hip_eth *eth, const void *commitments48, const void *zs_le32, const void *ys_le32, const void *proofs48,
                                                uint64_t count, const uint8_t *seed32, uint8_t *result) {
    if (!eth) return KZG_HIP_ERR_BAD_ARG;
    KZG_TRY
    const std::shared_ptr<g2_state> g = g2_of(eth->g2_mu, eth->g2);
    if (!g) return KZG_HIP_ERR_BAD_ARG;
    if (!count) return KZG_HIP_OK;
    if (!commitments48 || !zs_le32 || !ys_le32 || !proofs48 || !result) return KZG_HIP_ERR_BAD_ARG;
    t_combine = combine_stats{};
    stream_lease lease(eth->fs);
    hipStream_t s = lease.s;
    if (!combine_route(count)) return eth_checks(s, g->d_gen, g->d_s, commitments48, zs_le32, ys_le32, proofs48, count, result);
    t_combine.route = 1;
    const combine_seed seed = combine_seed_of(seed32);
    const uint64_t R = combine_rows();
    const uint8_t *c48 = (const uint8_t *)commitments48, *pi48 = (const uint8_t *)proofs48, *zs = (const uint8_t *)zs_le32, *ys = (const uint8_t *)ys_le32;
    return combine_drive(count, R, combine_chunk_groups(R) * R, result, t_combine,
        [&](uint64_t i0, uint64_t k, uint64_t G, uint8_t *status, uint8_t *gok) -> int {
            dtmp<uint8_t> d_c48(s), d_pi48(s), d_z32(s), d_y32(s), d_cbad(s), d_pbad(s), d_st(s); dtmp<g1j> d_c(s), d_pi(s), d_a(s), d_b(s); dtmp<fr> d_z(s), d_y(s);
            CHK(upload(d_c48, c48 + 48 * i0, 48 * k)); CHK(upload(d_pi48, pi48 + 48 * i0, 48 * k)); CHK(upload(d_z32, zs + 32 * i0, 32 * k));
            CHK(upload(d_y32, ys + 32 * i0, 32 * k)); CHK(d_cbad.alloc(k)); CHK(d_pbad.alloc(k));
            CHK(d_st.alloc(k)); CHK(d_c.alloc(k)); CHK(d_pi.alloc(k)); CHK(d_z.alloc(k)); CHK(d_y.alloc(k)); CHK(d_a.alloc(G)); CHK(d_b.alloc(G));
            launch_g1_decompress_rows(s, d_c48.p, d_c.p, k, d_cbad.p, false);
            launch_g1_decompress_rows(s, d_pi48.p, d_pi.p, k, d_pbad.p, false);
            launch_eth_combine_fields(s, d_z32.p, d_y32.p, d_cbad.p, d_pbad.p, k, d_z.p, d_y.p, d_st.p);
            CHK(combine_group_sums(s, seed, d_c.p, d_pi.p, false, d_z.p, d_y.p, d_st.p, i0, k, R, d_a.p, d_b.p, false));
            drain_on_exit drain(s);                                                              // (an error below leaves no copy into status in flight)
            HIPCHK(hipMemcpyAsync(status, d_st.p, k, hipMemcpyDeviceToHost, s));                 // 0 where the row's inputs are valid
            return combine_group_checks(s, g->d_gen, g->d_s, d_a.p, d_b.p, G, gok);
        },
        [&](uint64_t b, uint64_t e) { return eth_checks(s, g->d_gen, g->d_s, c48 + 48 * b, zs + 32 * b, ys + 32 * b, pi48 + 48 * b, e - b, result + b); });
    KZG_CATCH
}

// test hooks (kzg_hip_internal.h): A_g and B_g of every group as normalised Kilic images, and what the calling thread's last _combined call did
int kzg_hip_test_combine_points(kzg_hip_kzg *ks, const void *commitments_g1, const void *proofs_g1, const void *xs_fr, const void *ys_fr, uint64_t count,
                                const uint8_t *seed32, void *out_a_g1, void *out_b_g1) {
    if (!ks || !seed32 || (count && (!commitments_g1 || !proofs_g1 || !xs_fr || !ys_fr || !out_a_g1 || !out_b_g1))) return KZG_HIP_ERR_BAD_ARG;
    if (!count) return KZG_HIP_OK;
    KZG_TRY
    stream_lease lease(ks->fs);
    hipStream_t s = lease.s;
    const combine_seed seed = combine_seed_of(seed32);
    const uint64_t R = combine_rows(), G = combine_group_count(count, R);
    if (G > COMBINE_CHUNK_GROUPS || G > combine_chunk_groups(R)) return KZG_HIP_ERR_TOO_WIDE;
    dtmp<g1j> d_a(s), d_b(s);
    CHK(d_a.alloc(G)); CHK(d_b.alloc(G));
    CHK(combine_single_chunk(s, seed, (const g1j *)commitments_g1, (const g1j *)proofs_g1, (const fr *)xs_fr, (const fr *)ys_fr, 0, count, R, d_a.p, d_b.p, true));
    HIPCHK(hipMemcpyAsync(out_a_g1, d_a.p, G * sizeof(g1j), hipMemcpyDeviceToHost, s));
    HIPCHK(hipMemcpyAsync(out_b_g1, d_b.p, G * sizeof(g1j), hipMemcpyDeviceToHost, s));
    HIPCHK(hipStreamSynchronize(s));
    return KZG_HIP_OK;
    KZG_CATCH
}
// the multi-proof form: A_g and B_g likewise, and J_g as G x np Montgomery values
int kzg_hip_test_combine_multi_points(kzg_hip_kzg *ks, const void *commitments_g1, const void *proofs_g1, const void *xs_fr, const void *ys_fr, uint64_t n, uint64_t count,
                                      const uint8_t *seed32, void *out_a_g1, void *out_b_g1, void *out_j_fr) {
    if (!ks || !seed32 || n == 0 || (count && (!commitments_g1 || !proofs_g1 || !xs_fr || !ys_fr || !out_a_g1 || !out_b_g1 || !out_j_fr))) return KZG_HIP_ERR_BAD_ARG;
    if (!count) return KZG_HIP_OK;
    KZG_TRY
    kzg_hip_fft *fs = ks->fs;
    const uint64_t np = next_pow2(n);
    if (n > fs->W || np > COMBINE_MULTI_NP_MAX) return KZG_HIP_ERR_TOO_WIDE;
    if (np > ks->n_setup) return KZG_HIP_ERR_LEN_MISMATCH;
    const combine_seed seed = combine_seed_of(seed32);
    const uint64_t R = combine_rows(), G = combine_group_count(count, R);
    if (G > combine_multi_chunk_groups(R, n, np)) return KZG_HIP_ERR_TOO_WIDE;
    dev_guard dg(fs);
    hipStream_t s = fs->stream;
    dtmp<g1j> d_a(s), d_b(s); dtmp<fr> d_j(s);
    CHK(d_a.alloc(G)); CHK(d_b.alloc(G)); CHK(d_j.alloc(G * np));
    CHK(combine_multi_chunk(ks, s, seed, (const g1j *)commitments_g1, (const g1j *)proofs_g1, (const fr *)xs_fr, (const fr *)ys_fr, n, np, 0, count, R, d_j.p, d_a.p, d_b.p,
                            true));
    HIPCHK(hipMemcpyAsync(out_a_g1, d_a.p, G * sizeof(g1j), hipMemcpyDeviceToHost, s));
    HIPCHK(hipMemcpyAsync(out_b_g1, d_b.p, G * sizeof(g1j), hipMemcpyDeviceToHost, s));
    HIPCHK(hipMemcpyAsync(out_j_fr, d_j.p, G * np * sizeof(fr), hipMemcpyDeviceToHost, s));
    HIPCHK(hipStreamSynchronize(s));
    return KZG_HIP_OK;
    KZG_CATCH
}
int kzg_hip_test_combine_multi_route(uint64_t n, uint64_t count, uint64_t out[2]) {
    if (!out || n == 0) return KZG_HIP_ERR_BAD_ARG;
    out[0] = combine_multi_route(n, count) ? 1 : 0; out[1] = COMBINE_MULTI_FROM;
    return KZG_HIP_OK;
}
int kzg_hip_test_combine_stats(uint64_t out[6]) {
    if (!out) return KZG_HIP_ERR_BAD_ARG;
    out[0] = t_combine.route; out[1] = t_combine.groups; out[2] = t_combine.failed; out[3] = t_combine.rechecked;
    out[4] = COMBINE_FROM; out[5] = combine_rows();
    return KZG_HIP_OK;
}

// eth.VerifyAggregateKZGProof (eth/eth.go:155-172) over many sidecars.  Per chunk of whole sidecars: ONE upload of the raw bytes, then
// transcripts -> aggregated polynomials (BlobsToPolynomials + PolyLinComb) -> aggregated commitments (FromCompressedG1, the powers, a
// segmented sum) -> y (the quotient kernel's evaluation half) -> the check inputs and the pairing; one download of the results.  A verifier
// commits to nothing: no fixed-base table is built or walked.
int kzg_hip_eth_verify_aggregate_kzg_proof_batch(kzg_hip_eth *eth, const void *blobs_le32, const uint64_t *blob_counts, const void *commitments48,
                                                 const void *proofs48, uint64_t sidecars, uint8_t *result,
                                                 void *out_agg_commitments48, void *out_zs_fr, void *out_ys_fr) {
    if (!eth) return KZG_HIP_ERR_BAD_ARG;
    KZG_TRY
    const std::shared_ptr<g2_state> g = g2_of(eth->g2_mu, eth->g2);
    if (!g) return KZG_HIP_ERR_BAD_ARG;
    if (!sidecars) return KZG_HIP_OK;
    if (!blob_counts || !proofs48 || !result) return KZG_HIP_ERR_BAD_ARG;
    const uint64_t n = eth->n;
    uint64_t total = 0;
    for (uint64_t j = 0; j < sidecars; j++) {
        if (blob_counts[j] > UINT64_MAX - total) return KZG_HIP_ERR_TOO_WIDE;
        total += blob_counts[j];
    }
    if (total > (UINT64_MAX >> 1) / (n * 32)) return KZG_HIP_ERR_TOO_WIDE;      // (the byte offsets must not overflow either)
    if (total && (!blobs_le32 || !commitments48)) return KZG_HIP_ERR_BAD_ARG;
    // where the transcripts are hashed: the device takes the same 28 ms for 1 or 4096 chains of four blobs, a host thread 0.23 ms per such
    // sidecar: the measured curves cross between 128 and 192 sidecars (profiles/verify_aggregate.md)
    const knobs::transcript_mode forced = knobs::eth_transcript();
    constexpr uint64_t TRANSCRIPT_DEVICE_FROM = 176;
    const bool on_device = forced == knobs::transcript_mode::by_count ? sidecars >= TRANSCRIPT_DEVICE_FROM : forced == knobs::transcript_mode::device;
    const uint64_t budget = (uint64_t)(knobs::eth_verify_chunk_mb() * 1048576.0);   // (fractions allowed: tests force chunks of a few small blobs)
    constexpr uint64_t CHECKS = 8192;                                            // per pairing launch, as kzg_hip_pairings_verify_batch
    const uint8_t *blobs = (const uint8_t *)blobs_le32, *comms = (const uint8_t *)commitments48, *proofs = (const uint8_t *)proofs48;

    stream_lease lease(eth->fs);
    hipStream_t s = lease.s;
    std::vector<uint64_t> off; std::vector<fr> h_r, h_z; std::vector<uint8_t> st;
    drain_on_exit drain(s);                                                      // declared after the host buffers the stream copies from / into
    uint64_t j0 = 0, b0 = 0;
    while (j0 < sidecars) {
        // the chunk: whole sidecars while their blobs fit the byte budget (a larger sidecar forms a chunk by itself), at most CHECKS of them
        off.assign(1, 0);
        uint64_t j1 = j0;
        while (j1 < sidecars && j1 - j0 < CHECKS) {
            const uint64_t nb = off.back() + blob_counts[j1];
            if (j1 > j0 && nb * n * 32 > budget) break;
            off.push_back(nb); j1++;
        }
        const uint64_t S = j1 - j0, B = off.back();
        const uint8_t *c_blobs = blobs + b0 * n * 32, *c_comms = comms + b0 * 48;
        dtmp<uint8_t> d_blobs(s), d_comm(s), d_pi48(s), d_cbad(s), d_pbad(s), d_st(s), d_ok(s), d_c48(s);
        dtmp<uint64_t> d_off(s); dtmp<fr> d_r(s), d_z(s), d_y(s), d_agg(s), d_q(s), d_pow(s); dtmp<uint32_t> d_flag(s);
        dtmp<g1j> d_cpts(s), d_cmul(s), d_sum(s), d_sumk(s), d_pik(s), d_p0(s), d_p1(s);
        const uint64_t extra = eth_quotient_scratch_elems(n, S);
        CHK(d_blobs.alloc(B * n * 32)); CHK(d_comm.alloc(B * 48)); CHK(upload(d_pi48, proofs + 48 * j0, S * 48)); CHK(d_cbad.alloc(B)); CHK(d_pbad.alloc(S)); CHK(d_st.alloc(S));
        CHK(d_ok.alloc(S)); CHK(upload(d_off, off.data(), S + 1)); CHK(d_r.alloc(S)); CHK(d_z.alloc(S)); CHK(d_y.alloc(S)); CHK(d_agg.alloc(S * n)); CHK(d_q.alloc(S * n + extra));
        CHK(d_pow.alloc(B)); CHK(d_flag.alloc(S)); CHK(d_cpts.alloc(B)); CHK(d_cmul.alloc(B)); CHK(d_sum.alloc(S)); CHK(d_sumk.alloc(S)); CHK(d_pik.alloc(S));
        CHK(d_p0.alloc(S)); CHK(d_p1.alloc(S));
        HIPCHK(hipMemsetAsync(d_st.p, 0, S, s));
        HIPCHK(hipMemsetAsync(d_flag.p, 0, S * 4, s));
        if (B) {
            HIPCHK(hipMemcpyAsync(d_comm.p, c_comms, B * 48, hipMemcpyHostToDevice, s));
            CHK(h2d_copy(d_blobs.p, c_blobs, B * n * 32, s));
        }
        launch_g1_decompress_rows(s, d_comm.p, d_cpts.p, B, d_cbad.p, false);   // FromCompressedG1(commitments), eth/helpers.go:149-157
        launch_g1_decompress_rows(s, d_pi48.p, d_pik.p, S, d_pbad.p, true);     // ... and of the proofs (eth/eth.go:168-170)
        if (on_device) {
            launch_eth_transcripts(s, d_blobs.p, d_comm.p, d_off.p, n, S, d_r.p, d_z.p);
        } else {
            // the existing host chain (sha256.cpp) on the calling thread, while the device decompresses
            h_r.resize(S); h_z.resize(S);
            for (uint64_t j = 0; j < S; j++) {
                const uint64_t cnt = off[j + 1] - off[j];
                sha256 h;
                h.update("FSBLOBVERIFY_V1_", 16);
                h.update_u64_le(n);
                h.update_u64_le(cnt);
                if (cnt) { h.update(c_blobs + off[j] * n * 32, cnt * n * 32); h.update(c_comms + off[j] * 48, cnt * 48); }
                uint8_t tr[33], d[32];
                h.final(tr);
                for (int tag = 0; tag < 2; tag++) {
                    tr[32] = (uint8_t)tag;
                    sha256 h2;
                    h2.update(tr, 33);
                    h2.final(d);
                    (tag ? h_z : h_r)[j] = fr_from_digest_bytes(d);
                }
            }
            HIPCHK(hipMemcpyAsync(d_r.p, h_r.data(), S * sizeof(fr), hipMemcpyHostToDevice, s));
            HIPCHK(hipMemcpyAsync(d_z.p, h_z.data(), S * sizeof(fr), hipMemcpyHostToDevice, s));
        }
        launch_eth_agg_poly(s, d_blobs.p, d_off.p, d_r.p, n, S, d_agg.p, d_st.p);
        launch_eth_powers(s, d_r.p, d_off.p, S, d_pow.p);
        launch_g1_mul_vec(s, d_cpts.p, B ? B : 1, d_pow.p, 1, B, d_cmul.p);     // LinCombG1(commitments, powers), eth/helpers.go:158-160
        launch_g1_segment_sum(s, d_cmul.p, d_cbad.p, d_off.p, S, d_sum.p, d_sumk.p, d_st.p);
        // y = EvaluatePolynomialInEvaluationForm(aggregatedPoly, z) (eth/eth.go:166): the quotient kernel's first half
        launch_eth_quotient(s, d_agg.p, n, eth->d_domain, n, S, d_z.p, 1, eth->fs->d_inv_pow2 + ilog2(n), d_q.p, d_y.p, d_flag.p, 1, extra ? d_q.p + S * n : nullptr);
        launch_eth_agg_finish(s, d_flag.p, d_pbad.p, S, d_y.p, d_st.p);
        // VerifyKZGProofFromPoints (eth/helpers.go:55-68): e(C - [y]G1 + [z] pi, G2) e(-pi, kzgSetupG2[1]) == 1
        launch_kzg_check_inputs(s, d_sumk.p, d_pik.p, d_y.p, nullptr, d_z.p, S, d_p0.p, d_p1.p);
        launch_pairing_check(s, true, g->d_gen, g->d_s, d_p0.p, d_p1.p, S, d_ok.p);
        if (out_agg_commitments48) {
            CHK(d_c48.alloc(S * 48));
            launch_g1_compress(s, d_sum.p, d_c48.p, S);
        }
        HIPCHK(hipGetLastError());
        st.resize(S);
        HIPCHK(hipMemcpyAsync(st.data(), d_st.p, S, hipMemcpyDeviceToHost, s));
        HIPCHK(hipMemcpyAsync(result + j0, d_ok.p, S, hipMemcpyDeviceToHost, s));
        if (out_agg_commitments48) HIPCHK(hipMemcpyAsync((uint8_t *)out_agg_commitments48 + 48 * j0, d_c48.p, S * 48, hipMemcpyDeviceToHost, s));
        if (out_zs_fr) HIPCHK(hipMemcpyAsync((fr *)out_zs_fr + j0, d_z.p, S * sizeof(fr), hipMemcpyDeviceToHost, s));
        if (out_ys_fr) HIPCHK(hipMemcpyAsync((fr *)out_ys_fr + j0, d_y.p, S * sizeof(fr), hipMemcpyDeviceToHost, s));
        HIPCHK(hipStreamSynchronize(s));
        for (uint64_t j = 0; j < S; j++) if (st[j]) result[j0 + j] = st[j];
        j0 = j1; b0 += B;
    }
    return KZG_HIP_OK;
    KZG_CATCH
}

// test hooks (kzg_hip_internal.h): the transcript kernel's hash and reduction, one message / digest per lane
int kzg_hip_test_sha256_lanes(kzg_hip_fft *fs, const void *data, const uint64_t *offsets, const uint64_t *lens, uint64_t rows, void *out32) {
    if (!fs || (rows && (!offsets || !lens || !out32))) return KZG_HIP_ERR_BAD_ARG;
    if (!rows) return KZG_HIP_OK;
    KZG_TRY
    uint64_t bytes = 0;
    for (uint64_t t = 0; t < rows; t++) bytes = std::max(bytes, offsets[t] + lens[t]);
    if (bytes && !data) return KZG_HIP_ERR_BAD_ARG;
    stream_lease lease(fs);
    hipStream_t s = lease.s;
    dtmp<uint8_t> d_data(s); dtmp<uint64_t> d_off(s), d_len(s); dtmp<uint32_t> d_out(s);
    CHK(d_data.alloc(bytes)); CHK(upload(d_off, offsets, rows)); CHK(upload(d_len, lens, rows)); CHK(d_out.alloc(8 * rows));
    if (bytes) HIPCHK(hipMemcpyAsync(d_data.p, data, bytes, hipMemcpyHostToDevice, s));
    launch_test_sha256_lanes(s, d_data.p, d_off.p, d_len.p, rows, d_out.p);
    HIPCHK(hipGetLastError());
    HIPCHK(hipMemcpyAsync(out32, d_out.p, 32 * rows, hipMemcpyDeviceToHost, s));
    HIPCHK(hipStreamSynchronize(s));
    return KZG_HIP_OK;
    KZG_CATCH
}
int kzg_hip_test_hash_to_bls_field_lanes(kzg_hip_fft *fs, const void *digests32, uint64_t rows, void *out_fr) {
    if (!fs || (rows && (!digests32 || !out_fr))) return KZG_HIP_ERR_BAD_ARG;
    if (!rows) return KZG_HIP_OK;
    KZG_TRY
    stream_lease lease(fs);
    hipStream_t s = lease.s;
    dtmp<uint8_t> d_in(s); dtmp<fr> d_out(s);
    CHK(upload(d_in, digests32, 32 * rows)); CHK(d_out.alloc(rows));
    launch_test_hash_to_bls_field_lanes(s, d_in.p, rows, d_out.p);
    HIPCHK(hipGetLastError());
    HIPCHK(hipMemcpyAsync(out_fr, d_out.p, rows * sizeof(fr), hipMemcpyDeviceToHost, s));
    HIPCHK(hipStreamSynchronize(s));
    return KZG_HIP_OK;
    KZG_CATCH
}

// test hooks (kzg_hip_internal.h): out[i] = reduced e(g1[i], g2[i]) as 12 standard-form F_p elements, by the one-lane or the wavefront kernel
static int pairing_test(kzg_hip_fft *fs, const void *g1, const void *g2, uint64_t n, void *out_fp12, bool wave) {
    if (!fs || (n && (!g1 || !g2 || !out_fp12))) return KZG_HIP_ERR_BAD_ARG;
    if (!n) return KZG_HIP_OK;
    KZG_TRY
    stream_lease lease(fs);
    hipStream_t s = lease.s;
    dtmp<g1j> d_p(s); dtmp<g2j> d_q(s); dtmp<fp> d_out(s);
    CHK(upload(d_p, g1, n)); CHK(upload(d_q, g2, n)); CHK(d_out.alloc(12 * n));
    g2_prepared *d_lines = nullptr;
    HIPCHK(hipMalloc((void **)&d_lines, n * sizeof(g2_prepared)));
    std::unique_ptr<g2_prepared, hipError_t (*)(void *)> own(d_lines, hipFree);
    launch_g2_prepare(s, d_q.p, n, d_lines);
    if (wave) launch_pairing_value_wave(s, d_p.p, d_lines, n, d_out.p);
    else launch_pairing_value(s, d_p.p, d_lines, n, d_out.p);
    HIPCHK(hipGetLastError());
    HIPCHK(hipMemcpyAsync(out_fp12, d_out.p, 12 * n * sizeof(fp), hipMemcpyDeviceToHost, s));
    HIPCHK(hipStreamSynchronize(s));
    return KZG_HIP_OK;
    KZG_CATCH
}
int kzg_hip_pairing_test(kzg_hip_fft *fs, const void *g1, const void *g2, uint64_t n, void *out_fp12) { return pairing_test(fs, g1, g2, n, out_fp12, false); }
int kzg_hip_pairing_test_wave(kzg_hip_fft *fs, const void *g1, const void *g2, uint64_t n, void *out_fp12) { return pairing_test(fs, g1, g2, n, out_fp12, true); }

// test hook: out[i] = op(a[i], b[i]) on the wavefront tower (k_wave_fp12_op), rows of 12 standard-form F_p elements
int kzg_hip_test_wave_fp12_op(kzg_hip_fft *fs, int op, const void *a, const void *b, uint64_t n, void *out) {
    if (!fs || op < 0 || op > 8 || (n && (!a || !b || !out))) return KZG_HIP_ERR_BAD_ARG;
    if (!n) return KZG_HIP_OK;
    KZG_TRY
    stream_lease lease(fs);
    hipStream_t s = lease.s;
    dtmp<fp> d_a(s), d_b(s), d_out(s);
    CHK(upload(d_a, a, 12 * n)); CHK(upload(d_b, b, 12 * n)); CHK(d_out.alloc(12 * n));
    launch_wave_fp12_op(s, op, d_a.p, d_b.p, n, d_out.p);
    HIPCHK(hipGetLastError());
    HIPCHK(hipMemcpyAsync(out, d_out.p, 12 * n * sizeof(fp), hipMemcpyDeviceToHost, s));
    HIPCHK(hipStreamSynchronize(s));
    return KZG_HIP_OK;
    KZG_CATCH
}
// test hook: out[0] = 1 when launch_pairing_check would run the wavefront kernel for n checks now, 0 for the one-lane kernel; out[1] = PAIRING_WAVE_BELOW
int kzg_hip_test_pairing_route(uint64_t n, uint64_t *out) {
    if (!out) return KZG_HIP_ERR_BAD_ARG;
    out[0] = pairing_route_is_wave(n) ? 1 : 0;
    out[1] = PAIRING_WAVE_BELOW;
    return KZG_HIP_OK;
}

}  // extern "C"
