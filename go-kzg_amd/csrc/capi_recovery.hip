// capi_recovery.hip -- erasure recovery (f3): ZeroPolyViaMultiplication, RecoverPolyFromSamples
#include "capi_common.hpp"
#include "recover_rows.hpp"

// ---------------------------------------------------------------------------------------------------------
// erasure recovery (row f3)
// ---------------------------------------------------------------------------------------------------------
// Small erasure sets: the vanishing polynomial evaluated directly on the domain (k_zero_eval_direct, length x n_missing products), then one inverse
// transform for the coefficients.  Large ones: the product tree of k_fr.hip (n log^2 n products: 65 536 points with half of them missing are 2^31
// products directly and ~2^24 through the tree), then one forward transform for the evaluations.  The polynomial is unique (monic, the given roots),
// so both give the reference's values bit for bit.  KZG_HIP_ZERO_POLY=direct|tree forces one (tests run both).
static int zero_poly_tree(kzg_hip_fft *fs, hipStream_t s, const uint64_t *d_missing, uint64_t n_missing, uint64_t length, fr *d_eval, fr *d_poly) {
    uint64_t leaves = 1;
    while (leaves * ZERO_TREE_LEAF < n_missing) leaves <<= 1;             // <= length / 16: the root has degree <= length
    const uint64_t dtot = leaves * ZERO_TREE_LEAF, pad = dtot - n_missing;
    dtmp<fr> d_a(s), d_b(s), d_f(s), d_g(s);
    CHK(d_a.alloc(dtot)); CHK(d_b.alloc(dtot)); CHK(d_f.alloc(2 * dtot)); CHK(d_g.alloc(dtot));
    launch_zero_leaves(s, fs->d_expanded, fs->W / length, d_missing, n_missing, leaves, d_a.p);
    fr *cur = d_a.p, *nxt = d_b.p;
    for (uint64_t d = ZERO_TREE_LEAF, nodes = leaves; nodes > 1; d <<= 1, nodes >>= 1) {
        fr_fft_rows(fs, s, cur, d, d, d_f.p, 2 * d, nodes, 0);            // every node's a, zero-extended to 2d values
        launch_zero_pair_products(s, d_f.p, 2 * d, nodes / 2, d_g.p);
        fr_fft_rows(fs, s, d_g.p, 2 * d, 2 * d, nxt, 2 * d, nodes / 2, 1);   // a b
        launch_zero_join(s, nxt, cur, d, nodes / 2);                      // + x^d (a + b)
        std::swap(cur, nxt);
    }
    launch_zero_unpad(s, cur, pad, n_missing, length, d_poly);
    fr_fft_rows(fs, s, d_poly, length, length, d_eval, length, 1, 0);
    HIPCHK(hipGetLastError());
    return KZG_HIP_OK;
}
static int zero_poly_dev(kzg_hip_fft *fs, hipStream_t s, const uint64_t *d_missing, uint64_t n_missing, uint64_t length, fr *d_eval, fr *d_poly) {
    const knobs::zero_poly_mode forced = knobs::zero_poly_once();
    // measured crossover (half of the domain missing): 8192 points, where both take 0.7 ms; 32 768 points: 4.9 ms direct, 1.2 ms through the tree
    if (forced == knobs::zero_poly_mode::tree || (forced == knobs::zero_poly_mode::by_size && n_missing >= 1024 && n_missing * length >= (1ull << 26))) return zero_poly_tree(fs, s, d_missing, n_missing, length, d_eval, d_poly);
    launch_zero_eval_direct(s, fs->d_expanded, fs->W / length, d_missing, n_missing, length, d_eval);
    fr_fft_rows(fs, s, d_eval, length, length, d_poly, length, 1, 1);     // coefficients: degree n_missing < length
    HIPCHK(hipGetLastError());
    return KZG_HIP_OK;
}
int kzg_hip_zero_poly_via_multiplication(kzg_hip_fft *fs, const uint64_t *missing_indices, uint64_t n_missing, uint64_t length,
                                         void *out_zero_eval_fr, void *out_zero_poly_fr) {
    if (!fs || !out_zero_eval_fr || !out_zero_poly_fr || (n_missing && !missing_indices)) return KZG_HIP_ERR_BAD_ARG;
    if (n_missing == 0) {                                    // zero_poly.go:117-119
        memset(out_zero_eval_fr, 0, length * sizeof(fr)); memset(out_zero_poly_fr, 0, length * sizeof(fr));
        return KZG_HIP_OK;
    }
    if (length > fs->W) return KZG_HIP_ERR_TOO_WIDE;         // "domain too small for requested length" :120-122
    if (!is_pow2(length)) return KZG_HIP_ERR_NOT_POW2;       // "length not a power of two" :123-125
    if (n_missing >= length) return KZG_HIP_ERR_BAD_ARG;     // "expected output smaller or equal to input length" :205-207
    for (uint64_t i = 0; i < n_missing; i++) if (missing_indices[i] >= length) return KZG_HIP_ERR_BAD_ARG;
    stream_lease lease(fs);     // its own stream: host-buffer calls from many threads run side by side
    hipStream_t s = lease.s;
    dtmp<uint64_t> d_m(s); dtmp<fr> d_e(s), d_p(s);
    CHK(d_m.alloc(n_missing)); CHK(d_e.alloc(length)); CHK(d_p.alloc(length));
    HIPCHK(hipMemcpyAsync(d_m.p, missing_indices, n_missing * 8, hipMemcpyHostToDevice, s));
    CHK(zero_poly_dev(fs, s, d_m.p, n_missing, length, d_e.p, d_p.p));
    HIPCHK(hipMemcpyAsync(out_zero_eval_fr, d_e.p, length * sizeof(fr), hipMemcpyDeviceToHost, s));
    HIPCHK(hipMemcpyAsync(out_zero_poly_fr, d_p.p, length * sizeof(fr), hipMemcpyDeviceToHost, s));
    HIPCHK(hipStreamSynchronize(s));
    return KZG_HIP_OK;
}
int kzg_hip_recover_poly_from_samples(kzg_hip_fft *fs, const void *samples_fr, const uint8_t *present, uint64_t n, void *out_fr) {
    if (!fs || !samples_fr || !present || !out_fr || n == 0) return KZG_HIP_ERR_BAD_ARG;
    if (n > fs->W) return KZG_HIP_ERR_TOO_WIDE;
    if (!is_pow2(n)) return KZG_HIP_ERR_NOT_POW2;
    KZG_TRY
    std::vector<uint64_t> missing;
    for (uint64_t i = 0; i < n; i++) if (!present[i]) missing.push_back(i);   // recover_from_samples.go:44-49
    if (missing.size() >= n) return KZG_HIP_ERR_BAD_ARG;
    if (missing.empty()) { memcpy(out_fr, samples_fr, n * sizeof(fr)); return KZG_HIP_OK; }   // zero poly == 0: nothing to divide by; data complete
    stream_lease lease(fs);     // its own stream: host-buffer calls from many threads run side by side
    hipStream_t s = lease.s;
    dtmp<uint64_t> d_m(s); dtmp<uint8_t> d_pr(s); dtmp<uint32_t> d_flag(s);
    dtmp<fr> d_s(s), d_ze(s), d_zp(s), d_a(s), d_b(s), d_c(s), d_f(s);
    CHK(d_m.alloc(missing.size())); CHK(d_pr.alloc(n)); CHK(d_flag.alloc(1)); CHK(d_s.alloc(n)); CHK(d_ze.alloc(n)); CHK(d_zp.alloc(n));
    CHK(d_a.alloc(n)); CHK(d_b.alloc(n)); CHK(d_c.alloc(n)); CHK(d_f.alloc(2));
    fr five = fr_from_u64(5), f2[2] = {inv<FrP>(five), five};             // ShiftPoly uses 5^-1, UnshiftPoly 5 (:9-40)
    HIPCHK(hipMemsetAsync(d_flag.p, 0, 4, s));
    HIPCHK(hipMemcpyAsync(d_m.p, missing.data(), missing.size() * 8, hipMemcpyHostToDevice, s));
    HIPCHK(hipMemcpyAsync(d_pr.p, present, n, hipMemcpyHostToDevice, s));
    HIPCHK(hipMemcpyAsync(d_s.p, samples_fr, n * sizeof(fr), hipMemcpyHostToDevice, s));
    HIPCHK(hipMemcpyAsync(d_f.p, f2, sizeof f2, hipMemcpyHostToDevice, s));
    CHK(zero_poly_dev(fs, s, d_m.p, missing.size(), n, d_ze.p, d_zp.p));
    launch_fr_pointwise(s, d_s.p, d_ze.p, d_pr.p, d_a.p, n, 0, nullptr);  // polyEvaluationsWithZero
    fr_fft_rows(fs, s, d_a.p, n, n, d_b.p, n, 1, 1);                      // polyWithZero
    launch_fr_scale_by_powers(s, d_b.p, d_f.p, n);                        // ShiftPoly(polyWithZero)
    launch_fr_scale_by_powers(s, d_zp.p, d_f.p, n);                       // ShiftPoly(zeroPoly)
    fr_fft_rows(fs, s, d_b.p, n, n, d_a.p, n, 1, 0);                      // evalShiftedPolyWithZero
    fr_fft_rows(fs, s, d_zp.p, n, n, d_c.p, n, 1, 0);                     // evalShiftedZeroPoly
    launch_fr_pointwise(s, d_a.p, d_c.p, d_pr.p, d_b.p, n, 1, nullptr);   // division
    fr_fft_rows(fs, s, d_b.p, n, n, d_a.p, n, 1, 1);                      // shiftedReconstructedPoly
    launch_fr_scale_by_powers(s, d_a.p, d_f.p + 1, n);                    // UnshiftPoly
    fr_fft_rows(fs, s, d_a.p, n, n, d_b.p, n, 1, 0);                      // reconstructedData
    launch_fr_pointwise(s, d_b.p, d_s.p, d_pr.p, nullptr, n, 2, d_flag.p);
    HIPCHK(hipGetLastError());
    uint32_t flag = 0;
    HIPCHK(hipMemcpyAsync(&flag, d_flag.p, 4, hipMemcpyDeviceToHost, s));
    HIPCHK(hipMemcpyAsync(out_fr, d_b.p, n * sizeof(fr), hipMemcpyDeviceToHost, s));
    HIPCHK(hipStreamSynchronize(s));
    return flag ? KZG_HIP_ERR_RECOVERY : KZG_HIP_OK;
    KZG_CATCH
}

// ---------------------------------------------------------------------------------------------------------
// batched recovery: many rows per call (lane bodies: recover_rows.hpp, kernels with a row dimension: k_recovery.hip)
// ---------------------------------------------------------------------------------------------------------
// A lone recovery is a dozen dependent launches around a few microseconds of arithmetic; here every stage is ONE launch over all rows of a chunk.
// Nothing below reads device memory on the host: erasure lists, counts and statuses are derived on the device, so the _dev form enqueues and returns.
static_assert(rr::ST_OK == KZG_HIP_OK && rr::ST_BAD_ARG == KZG_HIP_ERR_BAD_ARG && rr::ST_RECOVERY == KZG_HIP_ERR_RECOVERY, "status bytes are the header's codes");

// Which construction a chunk takes.  nm: the longest erasure list of the chunk where the host knows it, half of the domain where it does not.  Measured
// (profiles/recovery_batch.md, half of the domain missing, whole calls from host buffers): at 4096 points direct evaluation takes 0.34 ms + 62 us per row, the tree
// 0.54 ms + 11 us per row -- its launches are shared by all rows of the chunk -- so they cross at 4 rows (2^25 direct products), and at 16 / 64 / 256 rows the tree
// wins by 1.8x / 2.3x / 2.9x; at 32 768 points the tree wins from one row on (4.4 against 1.1 ms) and by 11x and more from 16 rows on.  The lone call's own
// crossover (2^26 products) is left as it is.
constexpr uint64_t ZERO_ROWS_TREE_FROM_NM = 256;          // not measured: below this a row's chain (nm products per point) is shorter than the tree's ~10 transforms (~60 per point)
constexpr uint64_t ZERO_ROWS_TREE_FROM_PRODUCTS = 1ull << 25;   // direct products of the whole chunk from which the tree wins
static bool zero_rows_use_tree(uint64_t nm, uint64_t length, uint64_t rows) {
    if (const knobs::zero_poly_mode forced = knobs::zero_poly_per_call(); forced != knobs::zero_poly_mode::by_size) return forced == knobs::zero_poly_mode::tree;
    return nm >= ZERO_ROWS_TREE_FROM_NM && nm * length * rows >= ZERO_ROWS_TREE_FROM_PRODUCTS;
}
static uint64_t recover_chunk_rows(uint64_t n) {          // whole rows per chunk under KZG_HIP_RECOVER_CHUNK_MB (fractions allowed: tests force chunks of a few rows)
    const uint64_t budget = (uint64_t)(knobs::recover_chunk_mb() * 1048576.0);
    const uint64_t per_row = 8 * sizeof(fr) * std::max<uint64_t>(n, ZERO_TREE_LEAF);   // six temporaries, the staged samples, list + mask + flags
    return std::min<uint64_t>(std::max<uint64_t>(budget / per_row, 1), 32768);           // (a row is a blockIdx.y of the direct evaluation)
}
// Vanishing polynomials of `rows` erasure lists (rows of list_stride entries, d_nm[r] of them used; every d_nm[r] <= max_nm < length): evaluations and
// coefficients in rows of `length`.  w_cur, w_nxt: rows x max(length, 16) elements each, w_f twice that; all three are free again on return.
static int zero_poly_rows(kzg_hip_fft *fs, hipStream_t s, const uint64_t *d_list, uint64_t list_stride, const uint64_t *d_nm, uint64_t max_nm, uint64_t nm_hint, uint64_t length,
                          uint64_t rows, fr *d_eval, fr *d_poly, fr *d_corr, fr *w_cur, fr *w_nxt, fr *w_f) {
    if (zero_rows_use_tree(nm_hint, length, rows)) {
        const uint64_t leaves = rr::shared_leaves(max_nm);                // the whole chunk's: a row with fewer roots pads with roots at 0
        launch_rr_leaves(s, fs->d_expanded, fs->W / length, d_list, list_stride, d_nm, leaves, rows, w_cur);
        fr *cur = w_cur, *nxt = w_nxt, *g = d_eval;                       // (the evaluations are written last: until then their area holds the pair products)
        for (uint64_t d = ZERO_TREE_LEAF, nodes = leaves; nodes > 1; d <<= 1, nodes >>= 1) {   // every level over rows x nodes equal nodes, as zero_poly_tree
            fr_fft_rows(fs, s, cur, d, d, w_f, 2 * d, rows * nodes, 0);
            launch_zero_pair_products(s, w_f, 2 * d, rows * nodes / 2, g);
            fr_fft_rows(fs, s, g, 2 * d, 2 * d, nxt, 2 * d, rows * nodes / 2, 1);
            launch_zero_join(s, nxt, cur, d, rows * nodes / 2);
            std::swap(cur, nxt);
        }
        launch_rr_unpad(s, cur, leaves, d_nm, length, rows, d_poly);
        fr_fft_rows(fs, s, d_poly, length, length, d_eval, length, rows, 0);
    } else {
        const uint32_t segs = launch_zero_eval_direct_rows_segs(length, rows, nm_hint);
        launch_rr_corr(s, d_nm, rows, segs, d_corr);
        launch_zero_eval_direct_rows(s, fs->d_expanded, fs->W / length, d_list, list_stride, d_nm, d_corr, segs, length, rows, d_eval);
        fr_fft_rows(fs, s, d_eval, length, length, d_poly, length, rows, 1);
    }
    HIPCHK(hipGetLastError());
    return KZG_HIP_OK;
}
// the tables of ShiftPoly / UnshiftPoly for the call's n: d_pw[0 .. n) = 5^-i, d_pw[n .. 2n) = 5^i; d_pw holds 2 n + 2 elements
static void recover_shift_tables(hipStream_t s, uint64_t n, fr *d_pw) {
    const fr five = fr_from_u64(5);
    launch_rr_shift_bases(s, inv<FrP>(five), five, d_pw + 2 * n);
    launch_fr_powers(s, d_pw + 2 * n, n, d_pw);
    launch_fr_powers(s, d_pw + 2 * n + 1, n, d_pw + n);
}
// One chunk of rows, everything resident.  shared: one mask (and one vanishing polynomial) for every row.  max_nm bounds every row's effective erasure count,
// nm_hint is what the dispatch assumes; shared_nm != 0: the host knows the shared mask's count and the lone construction builds the polynomial.
static int recover_rows_chunk(kzg_hip_fft *fs, hipStream_t s, const fr *d_s, const uint8_t *d_pr, bool shared, uint64_t n, uint64_t rows, const fr *d_pw, fr *d_out,
                              uint8_t *d_status, uint64_t max_nm, uint64_t nm_hint, uint64_t shared_nm) {
    const uint64_t nn = std::max<uint64_t>(n, ZERO_TREE_LEAF), zrows = shared ? 1 : rows, zs = shared ? 0 : n, area = rows * nn;
    dtmp<fr> slab(s), d_corr(s); dtmp<uint64_t> d_list(s), d_nm(s); dtmp<uint32_t> d_count(s), d_flag(s);
    CHK(slab.alloc(2 * zrows * nn + 4 * area)); CHK(d_corr.alloc(zrows)); CHK(d_list.alloc(zrows * n)); CHK(d_nm.alloc(zrows)); CHK(d_count.alloc(zrows)); CHK(d_flag.alloc(rows));
    fr *ze = slab.p, *zp = ze + zrows * nn, *a = zp + zrows * nn, *b = a + area, *c = b + area, *x = c + area;   // c and x adjacent: the tree's 2d-point transforms
    launch_rr_scan(s, d_pr, n, zrows, d_list.p, d_count.p, d_nm.p);
    if (n < 2) {                                                          // a row of one sample is present or not: nothing to transform
        launch_rr_finish(s, nullptr, d_s, d_pr, zs, d_count.p, shared ? 0 : 1, nullptr, n, rows, d_out, d_status);
        HIPCHK(hipGetLastError());
        return KZG_HIP_OK;
    }
    HIPCHK(hipMemsetAsync(d_flag.p, 0, rows * 4, s));
    if (shared_nm) CHK(zero_poly_dev(fs, s, d_list.p, shared_nm, n, ze, zp));   // one polynomial through the lone path
    else CHK(zero_poly_rows(fs, s, d_list.p, n, d_nm.p, max_nm, nm_hint, n, zrows, ze, zp, d_corr.p, a, b, c));
    launch_rr_mask_mul(s, d_s, ze, zs, d_pr, zs, n, rows, a);             // polyEvaluationsWithZero
    fr_fft_rows(fs, s, a, n, n, b, n, rows, 1);                           // polyWithZero
    launch_fr_mul_table_rows(s, b, d_pw, 1, n, rows);                     // ShiftPoly(polyWithZero)
    launch_fr_mul_table_rows(s, zp, d_pw, 1, n, zrows);                   // ShiftPoly(zeroPoly)
    fr_fft_rows(fs, s, b, n, n, a, n, rows, 0);                           // evalShiftedPolyWithZero
    fr_fft_rows(fs, s, zp, n, n, c, n, zrows, 0);                         // evalShiftedZeroPoly: never zero for a valid row
    fr *res = b, *tmp = a;
    if (shared) {                                                         // the one denominator row inverted once, then a table multiply
        launch_rr_strip_divide(s, nullptr, c, x, n);
        launch_fr_mul_table_rows(s, a, x, 1, n, rows);
        res = a; tmp = b;
    } else launch_rr_strip_divide(s, a, c, b, rows * n);
    fr_fft_rows(fs, s, res, n, n, tmp, n, rows, 1);                       // shiftedReconstructedPoly
    launch_fr_mul_table_rows(s, tmp, d_pw + n, 1, n, rows);               // UnshiftPoly
    fr_fft_rows(fs, s, tmp, n, n, res, n, rows, 0);                       // reconstructedData
    launch_rr_finish(s, res, d_s, d_pr, zs, d_count.p, shared ? 0 : 1, d_flag.p, n, rows, d_out, d_status);
    HIPCHK(hipGetLastError());
    return KZG_HIP_OK;
}
static int recover_batch_args(kzg_hip_fft *fs, const void *samples, const uint8_t *present, uint64_t present_rows, uint64_t n, uint64_t batch, void *out, uint8_t *status) {
    if (!fs || n == 0 || (batch && (!samples || !present || !out || !status))) return KZG_HIP_ERR_BAD_ARG;   // the lone call's codes in its order
    if (n > fs->W) return KZG_HIP_ERR_TOO_WIDE;
    if (!is_pow2(n)) return KZG_HIP_ERR_NOT_POW2;
    if (batch && present_rows != 1 && present_rows != batch) return KZG_HIP_ERR_BAD_ARG;
    return KZG_HIP_OK;
}
int kzg_hip_recover_poly_from_samples_batch_dev(kzg_hip_fft *fs, const void *d_samples_fr, const uint8_t *d_present, uint64_t present_rows, uint64_t n, uint64_t batch,
                                                void *d_out_fr, uint8_t *d_status, void *stream) {
    CHK(recover_batch_args(fs, d_samples_fr, d_present, present_rows, n, batch, d_out_fr, d_status));
    if (!batch) return KZG_HIP_OK;
    dev_select sel(fs);       // the caller's stream orders the work; settings tables are read-only
    hipStream_t s = (hipStream_t)stream;
    const bool shared = present_rows == 1 && batch != 1;
    dtmp<fr> d_pw(s);
    CHK(d_pw.alloc(2 * n + 2));
    recover_shift_tables(s, n, d_pw.p);
    const uint64_t per = recover_chunk_rows(n);
    for (uint64_t r0 = 0; r0 < batch; r0 += per) {                        // the masks stay on the device: every row may miss up to n - 1, half is assumed for the dispatch
        const uint64_t rows = std::min(per, batch - r0);
        CHK(recover_rows_chunk(fs, s, (const fr *)d_samples_fr + r0 * n, d_present + (shared ? 0 : r0 * n), shared, n, rows, d_pw.p, (fr *)d_out_fr + r0 * n, d_status + r0,
                               n - 1, n / 2, 0));
    }
    return KZG_HIP_OK;
}
int kzg_hip_recover_poly_from_samples_batch(kzg_hip_fft *fs, const void *samples_fr, const uint8_t *present, uint64_t present_rows, uint64_t n, uint64_t batch, void *out_fr,
                                            uint8_t *status) {
    CHK(recover_batch_args(fs, samples_fr, present, present_rows, n, batch, out_fr, status));
    if (!batch) return KZG_HIP_OK;
    const bool shared = present_rows == 1 && batch != 1;
    uint64_t shared_nm = 0;
    if (shared) {
        for (uint64_t i = 0; i < n; i++) shared_nm += present[i] ? 0 : 1;
        if (shared_nm == 0 || shared_nm == n) {                           // every row alike: copied through, or nothing present
            if (shared_nm == 0) memcpy(out_fr, samples_fr, batch * n * sizeof(fr)); else memset(out_fr, 0, batch * n * sizeof(fr));
            memset(status, shared_nm == 0 ? KZG_HIP_OK : KZG_HIP_ERR_BAD_ARG, batch);
            return KZG_HIP_OK;
        }
    }
    stream_lease lease(fs);     // its own stream: host-buffer calls from many threads run side by side
    hipStream_t s = lease.s;
    dtmp<fr> d_pw(s);
    CHK(d_pw.alloc(2 * n + 2));
    recover_shift_tables(s, n, d_pw.p);
    const uint64_t per = recover_chunk_rows(n);
    for (uint64_t r0 = 0; r0 < batch; r0 += per) {
        const uint64_t rows = std::min(per, batch - r0);
        uint64_t max_nm = shared_nm;
        if (!shared) for (uint64_t r = r0; r < r0 + rows; r++) {          // the chunk's longest erasure list: the tree's leaf count and the dispatch
            uint64_t cnt = 0;
            for (uint64_t i = 0; i < n; i++) cnt += present[r * n + i] ? 0 : 1;
            max_nm = std::max(max_nm, rr::effective_missing(cnt, n));
        }
        dtmp<fr> d_s(s); dtmp<uint8_t> d_pr(s), d_st(s);
        CHK(d_s.alloc(rows * n)); CHK(d_pr.alloc(shared ? n : rows * n)); CHK(d_st.alloc(rows));
        HIPCHK(hipMemcpyAsync(d_s.p, (const fr *)samples_fr + r0 * n, rows * n * sizeof(fr), hipMemcpyHostToDevice, s));
        HIPCHK(hipMemcpyAsync(d_pr.p, present + (shared ? 0 : r0 * n), shared ? n : rows * n, hipMemcpyHostToDevice, s));
        CHK(recover_rows_chunk(fs, s, d_s.p, d_pr.p, shared, n, rows, d_pw.p, d_s.p, d_st.p, max_nm, max_nm, shared_nm));   // (the output replaces the staged samples)
        HIPCHK(hipMemcpyAsync((fr *)out_fr + r0 * n, d_s.p, rows * n * sizeof(fr), hipMemcpyDeviceToHost, s));
        HIPCHK(hipMemcpyAsync(status + r0, d_st.p, rows, hipMemcpyDeviceToHost, s));
    }
    HIPCHK(hipStreamSynchronize(s));
    return KZG_HIP_OK;
}
int kzg_hip_zero_poly_via_multiplication_batch(kzg_hip_fft *fs, const uint64_t *missing_indices, const uint64_t *offsets, uint64_t batch, uint64_t length,
                                               void *out_zero_eval_fr, void *out_zero_poly_fr, uint8_t *status) {
    if (!fs || (batch && (!offsets || !out_zero_eval_fr || !out_zero_poly_fr || !status))) return KZG_HIP_ERR_BAD_ARG;
    if (length > fs->W) return KZG_HIP_ERR_TOO_WIDE;
    if (!is_pow2(length)) return KZG_HIP_ERR_NOT_POW2;
    if (!batch) return KZG_HIP_OK;
    for (uint64_t b = 0; b < batch; b++) if (offsets[b + 1] < offsets[b]) return KZG_HIP_ERR_BAD_ARG;
    if (offsets[batch] != offsets[0] && !missing_indices) return KZG_HIP_ERR_BAD_ARG;
    KZG_TRY
    fr *out_e = (fr *)out_zero_eval_fr, *out_p = (fr *)out_zero_poly_fr;
    std::vector<uint64_t> todo;                                           // rows that have a polynomial to compute; the others are settled here
    for (uint64_t b = 0; b < batch; b++) {
        const uint64_t cnt = offsets[b + 1] - offsets[b];
        bool ok = cnt < length;                                           // "expected output smaller or equal to input length" (zero_poly.go:205-207)
        for (uint64_t i = offsets[b]; ok && i < offsets[b + 1]; i++) ok = missing_indices[i] < length;
        status[b] = cnt == 0 || ok ? KZG_HIP_OK : KZG_HIP_ERR_BAD_ARG;
        if (cnt != 0 && ok) todo.push_back(b);
        else { memset(out_e + b * length, 0, length * sizeof(fr)); memset(out_p + b * length, 0, length * sizeof(fr)); }   // no indices: all zeros (:117-119)
    }
    if (todo.empty()) return KZG_HIP_OK;
    stream_lease lease(fs);
    hipStream_t s = lease.s;
    const uint64_t nn = std::max<uint64_t>(length, ZERO_TREE_LEAF), per = recover_chunk_rows(length);
    std::vector<uint64_t> h_list, h_nm;
    for (uint64_t t0 = 0; t0 < todo.size(); t0 += per) {
        const uint64_t rows = std::min<uint64_t>(per, todo.size() - t0);
        uint64_t max_nm = 0;
        h_list.assign(rows * length, 0); h_nm.resize(rows);
        for (uint64_t r = 0; r < rows; r++) {
            const uint64_t b = todo[t0 + r];
            h_nm[r] = offsets[b + 1] - offsets[b];
            max_nm = std::max(max_nm, h_nm[r]);
            memcpy(&h_list[r * length], missing_indices + offsets[b], h_nm[r] * 8);
        }
        dtmp<fr> slab(s), d_corr(s); dtmp<uint64_t> d_list(s), d_nm(s);
        CHK(slab.alloc(6 * rows * nn)); CHK(d_corr.alloc(rows)); CHK(d_list.alloc(rows * length)); CHK(d_nm.alloc(rows));
        fr *ze = slab.p, *zp = ze + rows * nn;
        HIPCHK(hipMemcpyAsync(d_list.p, h_list.data(), rows * length * 8, hipMemcpyHostToDevice, s));
        HIPCHK(hipMemcpyAsync(d_nm.p, h_nm.data(), rows * 8, hipMemcpyHostToDevice, s));
        CHK(zero_poly_rows(fs, s, d_list.p, length, d_nm.p, max_nm, max_nm, length, rows, ze, zp, d_corr.p, zp + rows * nn, zp + 2 * rows * nn, zp + 3 * rows * nn));
        for (uint64_t r = 0; r < rows;) {                                 // runs of neighbouring rows leave in one copy each
            uint64_t e = r + 1;
            while (e < rows && todo[t0 + e] == todo[t0 + e - 1] + 1) e++;
            HIPCHK(hipMemcpyAsync(out_e + todo[t0 + r] * length, ze + r * length, (e - r) * length * sizeof(fr), hipMemcpyDeviceToHost, s));
            HIPCHK(hipMemcpyAsync(out_p + todo[t0 + r] * length, zp + r * length, (e - r) * length * sizeof(fr), hipMemcpyDeviceToHost, s));
            r = e;
        }
        HIPCHK(hipStreamSynchronize(s));                                  // (the staged lists are reused by the next chunk)
    }
    return KZG_HIP_OK;
    KZG_CATCH
}
