// internal.hpp -- launcher prototypes shared by the kernel translation units and the C ABI (capi.hip).
#pragma once
#include <hip/hip_runtime.h>
#include <stdint.h>
#include "field.hpp"
#include "g1.hpp"
#include "knobs.hpp"
#include "fb_pair_index.hpp"

namespace kzg {

inline uint32_t ilog2(uint64_t v) { uint32_t r = 0; while ((1ull << r) < v) r++; return r; }   // ceil(log2 v)

// ---------------- k_fr.hip ----------------
// Batched radix-2 FFT over F_r (replaces _fft / InplaceFFT, fft_fr.go:30-105).
//   in  : batch x in_stride Fr, of which the first n_in of each row are used (rest zero-padded to n)
//   out : batch x n Fr, natural order.  roots = ExpandedRootsOfUnity or ReverseRootsOfUnity (W + 1 entries).
//   scale != nullptr: every output is multiplied by *scale (device pointer; n^-1 for the inverse).
//   tw4096 != nullptr and n == 4096: the radix-4 kernel on lazy limbs with that twiddle file (fr_fft4096.hpp; same direction as roots)
void launch_fr_fft(hipStream_t s, const fr *in, uint64_t in_stride, uint64_t n_in, fr *out, uint64_t n, uint64_t batch,
                   const fr *roots, uint64_t W, const fr *scale, const uint32_t *tw4096 = nullptr, const fr *roots_l = nullptr);
// whether launch_fr_fft takes a lazy-limb kernel for `batch` transforms of n points, given the twiddle files and a grid within the limits
bool fr_fft_lazy_sizes(uint64_t n, uint64_t batch);
// DASFFTExtension (das_extension.go:7-84), in place on batch rows of n values.
//   tw2048 != nullptr and n == 2048: the lazy-limb kernel with that twiddle file (fr_das2048.hpp, built from the same two tables)
void launch_das_ext(hipStream_t s, fr *vals, uint64_t n, uint64_t batch, const fr *expanded, const fr *reversed, uint64_t W,
                    const fr *inv_n, const uint32_t *tw2048 = nullptr);
// toeplitzCoeffsStepStrided (fk20_single.go:89-103): out[b][file][0..2k) from poly[b][0..n), optionally scaled.
void launch_toeplitz_coeffs(hipStream_t s, const fr *poly, uint64_t poly_stride, uint64_t n, uint64_t l, uint64_t batch, fr *out,
                            const fr *scale);
// quotients of `batch` polynomials (rows of poly_stride, n coefficients used) by (X - x[b]) (polyLongDiv with divisor [-x, 1],
// poly.go:14-40): row b of q (stride q_stride) gets n - 1 entries
void launch_quotient_linear(hipStream_t s, const fr *poly, uint64_t poly_stride, uint64_t n, uint64_t batch, const fr *x, fr *q, uint64_t q_stride);
void launch_fr_from_u64(hipStream_t s, const uint64_t *in, uint64_t in_stride, fr *out, uint64_t n);   // bls.AsFr over a slice
void launch_fr_zero_tails(hipStream_t s, fr *rows, uint64_t n_max, uint64_t batch, const uint64_t *lens, uint64_t lens_stride);
// returns (via *flag != 0) whether any of vals[0..n) is non-zero
void launch_fr_any_nonzero(hipStream_t s, const fr *vals, uint64_t n, uint32_t *flag);
void launch_fr_powers(hipStream_t s, const fr *base, uint64_t n, fr *out);   // out[i] = base^i

// eth/ byte-level path
void launch_fr_from_le32(hipStream_t s, const uint8_t *in, fr *out, uint64_t per_blob, uint64_t batch, uint32_t *bad);
void launch_fr_to_le32(hipStream_t s, const fr *in, uint8_t *out, uint64_t n);
void launch_fr_bitrev_gather(hipStream_t s, const fr *in, fr *out, uint64_t n);
// rows of (polynomial, z): q[row] = quotient, y_out[row] = p(z), flag[row] = 1 where z is in the domain (that row's quotient is zero)
constexpr uint64_t ZERO_TREE_LEAF = 16;   // roots per leaf of the vanishing-polynomial product tree (k_zero_leaves)
void launch_zero_leaves(hipStream_t s, const fr *expanded, uint64_t stride, const uint64_t *missing, uint64_t n_missing, uint64_t leaves, fr *a);
void launch_zero_pair_products(hipStream_t s, const fr *f, uint64_t m, uint64_t pairs, fr *out);
void launch_zero_join(hipStream_t s, fr *c, const fr *a, uint64_t d, uint64_t pairs);
void launch_zero_unpad(hipStream_t s, const fr *root, uint64_t pad, uint64_t n_missing, uint64_t length, fr *poly);
void launch_fr_mul_table_rows(hipStream_t s, fr *data, const fr *table, uint64_t stride, uint64_t n, uint64_t batch);
void launch_poly_lincomb(hipStream_t s, const fr *vectors, uint64_t stride, const fr *scalars, uint64_t count, uint64_t n, fr *out);   // bls.PolyLinComb
void launch_eth_quotient(hipStream_t s, const fr *poly, uint64_t poly_stride, const fr *domain, uint64_t n, uint64_t batch, const fr *z, uint64_t z_stride,
                         const fr *inv_n, fr *q, fr *y_out, uint32_t *flag, uint64_t dom_stride = 1, fr *scratch = nullptr);   // scratch: eth_quotient_scratch_elems(n, batch) elements (the row-split form of small batches) or null
uint64_t eth_quotient_scratch_elems(uint64_t n, uint64_t batch);

void launch_fr_scale_by_inv_powers(hipStream_t s, fr *c, const fr *x, uint64_t n, fr *xpow_n);   // c_i /= x^i; *xpow_n = x^n

// erasure recovery
void launch_zero_eval_direct(hipStream_t s, const fr *expanded, uint64_t stride, const uint64_t *missing, uint64_t n_missing, uint64_t length, fr *zero_eval);
void launch_fr_scale_by_powers(hipStream_t s, fr *poly, const fr *base, uint64_t n);
void launch_fr_pointwise(hipStream_t s, const fr *a, const fr *b, const uint8_t *present, fr *out, uint64_t n, int mode, uint32_t *flag);
// the same over the rows of a chunk: row r evaluates its own erasure list missing[r * list_stride ..) of n_missing[r] entries with correction corr[r]
uint32_t launch_zero_eval_direct_rows_segs(uint64_t length, uint64_t rows, uint64_t nm_hint);   // wavefronts per point (the corrections depend on it)
void launch_zero_eval_direct_rows(hipStream_t s, const fr *expanded, uint64_t stride, const uint64_t *missing, uint64_t list_stride, const uint64_t *n_missing, const fr *corr,
                                  uint32_t segs, uint64_t length, uint64_t rows, fr *zero_eval);

// ---------------- k_recovery.hip ----------------
// batched erasure recovery (lane bodies: recover_rows.hpp); rows of n values, erasure lists in rows of list_stride entries
void launch_rr_scan(hipStream_t s, const uint8_t *present, uint64_t n, uint64_t rows, uint64_t *list, uint32_t *count, uint64_t *nm);   // masks -> lists, counts, effective counts
void launch_rr_corr(hipStream_t s, const uint64_t *nm, uint64_t rows, uint32_t segs, fr *corr);
void launch_rr_shift_bases(hipStream_t s, const fr &inv5, const fr &five, fr *out);   // out = {5^-1, 5}
void launch_rr_leaves(hipStream_t s, const fr *expanded, uint64_t stride, const uint64_t *list, uint64_t list_stride, const uint64_t *nm, uint64_t leaves, uint64_t rows, fr *a);
void launch_rr_unpad(hipStream_t s, const fr *root, uint64_t leaves, const uint64_t *nm, uint64_t length, uint64_t rows, fr *poly);
void launch_rr_mask_mul(hipStream_t s, const fr *a, const fr *b, uint64_t b_stride, const uint8_t *present, uint64_t p_stride, uint64_t n, uint64_t rows, fr *out);
void launch_rr_strip_divide(hipStream_t s, const fr *num, const fr *den, fr *out, uint64_t total);   // out = num / den (num null: 1 / den), one inversion per 64
// status[row] and out[row] from the reconstruction (null: rows are only classified and copied), the samples and the counts; out may be recon
void launch_rr_finish(hipStream_t s, const fr *recon, const fr *samples, const uint8_t *present, uint64_t p_stride, const uint32_t *count, uint64_t c_stride, uint32_t *flag,
                      uint64_t n, uint64_t rows, fr *out, uint8_t *status);

// ---------------- k_g1.hip ----------------
// out[i] = scalars[i * s_stride] * pts[(i % pts_mod)]   (element-wise bls.MulG1; scalars in Montgomery form)
void launch_g1_mul_vec(hipStream_t s, const g1j *pts, uint64_t pts_mod, const fr *scalars, uint64_t s_stride, uint64_t n, g1j *out);
// acc[i] = sum over f < nfiles of scalars[b][f][j] * files[f][j]  -- the FK20-multi Toeplitz stage (fk20_multi.go:79-91)
hipError_t launch_g1_file_msm(hipStream_t s, const g1j *files, const fr *scalars, uint64_t nfiles, uint64_t k2, uint64_t j0, uint64_t cnt,
                              uint64_t batch, g1j *out);
// out[b][rev(i)] = i < n_valid ? in[b][i] : inf     (bit-reversal + "h[:n] || inf" padding, fk20_single.go:163-166)
void launch_g1_bitrev_copy(hipStream_t s, const g1j *in, uint64_t in_stride, uint64_t n_valid, g1j *out, uint64_t n, uint64_t batch);
// one radix-2 DIT stage on bit-reversed data (replaces the loop of _fftG1, fft_g1.go:44-55); `roots` holds the twiddles as
// GLV pairs (k mod lambda, k div lambda) in standard form, see g1_mul_glv
void launch_g1_fft_stage(hipStream_t s, g1j *data, uint64_t n, uint64_t batch, uint64_t m, const fr *roots, const int8_t *wnaf, uint64_t W);   // wnaf: the twiddles' precomputed digit strings (KZG_WNAF_ROW bytes each)
// Which of its device variants a stage launch runs: lanes per butterfly (1, 2 or 4), the digit schedule of the twiddle multiplication (regular odd digits or
// width-5 NAF) and, for the NAF schedule, whether the digits come from the twiddles' precomputed rows or are recoded per butterfly.  g1_fft_stage_plan is the
// ONE place that decides it, by launch size unless forced: quad as KZG_HIP_G1_QUAD parses (-1 by size; 0 / 1 / 2: one / four / two lanes), mul as
// KZG_HIP_G1_MUL.  The launchers ask it with the knobs' values, the test hooks (kzg_hip_internal.h) with the caller's, and both launch through
// launch_g1_fft_stage_planned, so what a plan says and what runs cannot differ.
struct g1_stage_plan { int lanes; bool wnaf; bool rows; };
g1_stage_plan g1_fft_stage_plan(uint64_t n, uint64_t batch, uint64_t m, bool dif, int quad, knobs::g1_mul_mode mul);
g1_stage_plan g1_fft_stage_plan(uint64_t n, uint64_t batch, uint64_t m, bool dif);   // as the library's own launches choose: the knobs' values
void launch_g1_fft_stage_planned(hipStream_t s, const g1_stage_plan &plan, bool dif, g1j *data, uint64_t n, uint64_t batch, uint64_t m, const fr *roots, const int8_t *wnaf, uint64_t W);
// decimation-in-frequency stage on the same pairs / twiddles: (x, y) -> (x + y, (x - y) w); and the odd-position clear between the
// FK20 transforms (h[:n] || inf in bit-reversed order)
void launch_g1_fft_stage_dif(hipStream_t s, g1j *data, uint64_t n, uint64_t batch, uint64_t m, const fr *roots, const int8_t *wnaf, uint64_t W);
void launch_g1_clear_odd(hipStream_t s, g1j *data, uint64_t n_total);
void launch_g1_take_even(hipStream_t s, const g1j *in, g1j *out, uint64_t total);   // out[t] = in[2 t]
bool g1_quad_enabled();   // the stage launchers put four lanes on a butterfly for launches of at most 16 384 butterflies (g1_quad.hpp) unless KZG_HIP_G1_QUAD=0
// latency mode: Stockham passes of radix 16 evaluated directly (k_g1.hip); result in data, tmp = batch x n scratch, scale optional
void launch_fb_direct_pass1(hipStream_t s, const g1a *table, uint64_t table_n, uint32_t c, uint32_t nwin, const fr *scalars, const fr *roots, uint64_t W, uint64_t batch,
                            uint32_t logR, g1j *out, bool glv = false);   // FK20 Toeplitz stage + first direct pass of the inverse transform (a lone polynomial)
// several lanes per multiplication (g1_coop_kernels.hpp; translation units of their own)
void launch_g1_stage_coop_dif(hipStream_t s, int lanes, bool wnaf_rows, g1j *data, uint64_t n, uint64_t batch, uint64_t m, const fr *roots, const int8_t *wnaf, uint64_t W, uint64_t total);
void launch_g1_stage_coop_dit(hipStream_t s, int lanes, bool wnaf_rows, g1j *data, uint64_t n, uint64_t batch, uint64_t m, const fr *roots, const int8_t *wnaf, uint64_t W, uint64_t total);
void launch_g1_direct_coop(hipStream_t s, int lanes, uint32_t wgs, size_t pad_lds, const g1j *src, uint64_t src_stride, uint64_t src_valid, g1j *dst, uint32_t logn, uint32_t logR,
                           uint64_t Ns, const fr *roots, uint64_t W, const fr *sc, uint64_t total, uint32_t logT, uint32_t logU);
void launch_g1_fft_direct(hipStream_t s, const g1j *in, uint64_t in_stride, uint64_t n_valid, g1j *data, g1j *tmp, uint64_t n, uint64_t batch, const fr *roots,
                          uint64_t W, const fr *scale, uint32_t max_logr = 4, int lanes = 1, uint32_t bits_done = 0, uint64_t n_out = 0,   // n_out: only the first n_out outputs are wanted (0 = all)
                          bool lanes_fixed = false);   // lanes_fixed: the pruned passes keep `lanes` too (test hook)
// to_kilic: also leave the device-internal Montgomery domain (R' = 2^390) for Kilic's (2^384): every API output path ends here
void launch_g1_normalize(hipStream_t s, const g1j *in, g1j *out, uint64_t n, bool to_kilic = false);
void launch_fr_inv_test(hipStream_t s, const fr *in, uint64_t n, fr *out_coop, fr *out_lane, fr *out_block);   // test hook: F_r inversion three ways (k_fr.hip)
void launch_fp_inv_both(hipStream_t s, const fp *in, fp *out_coop, fp *out_lane, uint64_t n, int mode);   // test / measurement hook: wave-cooperative (bit 0) and one-lane (bit 1) inversion of n elements, one wavefront each
void launch_g1_from_kilic(hipStream_t s, g1j *data, uint64_t n);   // in place: caller-supplied points enter the internal domain
void launch_g1_to_affine(hipStream_t s, const g1j *in, g1a *out, uint64_t n);
void launch_g1_compress(hipStream_t s, const g1j *in, uint8_t *out48, uint64_t n);
void launch_g1_decompress(hipStream_t s, const uint8_t *in48, g1j *out, uint64_t n, uint32_t *bad_flag);
void launch_g1_fixed_base_powers(hipStream_t s, const fr *powers, uint64_t n, g1j *out);   // out[i] = powers[i] * G

// ---------------- k_msm.hip ----------------
// Lanes of ONE wavefront on every SIMD of the calling thread's current device: CUs x 4 SIMDs x 64 lanes (65 536 on the 256 CUs of an MI355X
// in SPX mode; fewer on a partitioned part).  Every "does this launch still fit one wavefront per SIMD" heuristic of the launchers is written
// against this value, never against a literal.  Cached per device, thread-safe.
uint64_t device_simd_lanes();
inline uint64_t device_simds() { return device_simd_lanes() / 64; }
struct msm_plan {
    uint32_t c;        // window bits (fixed-base walk: signed digits in [-2^(c-1), 2^(c-1)]; bucket MSM: always 8)
    uint32_t nwin;     // windows of the fixed-base walk
    uint32_t nb;       // 2^(c-1)
    uint32_t ngroups;  // bucket MSM: 16 window groups (points only) or 8 (table also holds 2^64 P_i at [table_n + i])
    uint32_t fixed;    // 1: plan of a fixed-base table (k_fb_*), 0: bucket MSM
    uint32_t glv;      // fixed-base walk: 1 = the table holds ceil(128 / c) windows and both GLV halves of a scalar walk them (k_fb_accumulate_glv)
    uint64_t table_n;  // points per row of the table
    uint32_t paired;   // shared-window plans only: 1 = the paired-point table (entries indexed by the digits of two neighbouring points, nwin additions per coefficient)
};
// the bucket pipeline packs (point index << 2 | half | sign) into 32 bits and counts entries (32 per scalar) in 32 bits: both must fit
inline bool msm_index_range_ok(const msm_plan &p, uint64_t n) { return n < (1ull << 27) && 2 * p.table_n < (1ull << 30); }
size_t msm_workspace_bytes(const msm_plan &p, uint64_t n, uint64_t batch);
// batch MSMs over the same affine points, scalars in rows of sc_stride: out[b] = sum_i scalars[b][i] * P_i, NORMALISED (Z = one),
// as Kilic images when to_kilic.  table_stride != 0 (plans with 16 window groups): blob b reads its own slice of points, table + b * table_stride.
// crowded_buckets: the caller knows that a few buckets hold a large share of every blob's entries (many scalars of 128 bits: their second GLV half
// is 0 .. 3), so the balanced accumulate (a lane per 64 sorted entries) is taken as soon as fewer than 8 lanes would share a bucket
void launch_msm(hipStream_t s, const msm_plan &p, const g1a *table, const fr *scalars, uint64_t sc_stride, uint64_t n, uint64_t batch, void *workspace, g1j *out,
                bool to_kilic, uint64_t table_stride = 0, bool crowded_buckets = false);
// fixed-base window table: out[w * n + i] = 2^(c w) * pts[i], affine
void launch_msm_window_table(hipStream_t s, const g1a *pts, uint64_t n, uint32_t c, uint32_t nwin, g1j *tmp, g1a *out);

// fixed-base table MSM over the device-resident setup (see k_msm.hip)
size_t fb_partials_bytes(uint64_t n, uint64_t batch);
hipError_t launch_fb_build(hipStream_t s, const g1a *pts, uint64_t n, uint32_t c, uint32_t nwin, g1a *table);
void launch_fb_msm(hipStream_t s, const g1a *table, uint64_t table_n, uint32_t c, uint32_t nwin, const fr *scalars, uint64_t sc_stride, uint64_t n,
                   uint64_t batch, void *partials, g1j *out, bool to_kilic, bool glv = false, bool projective = false);
// the shared-window layout for large batches (k_msm.hip): table[i D + d - 1] = d P_i, W = ceil(128 / c) accumulators per blob, joined by a Horner finish.
// The workspace holds the digit words of the pre-pass and the per-window partial sums.
inline uint32_t fb_shared_windows(uint32_t c) { return (128 + c - 1) / c; }
size_t fb_shared_workspace_bytes(uint64_t n, uint64_t batch, uint32_t c);
hipError_t launch_fb_build_shared(hipStream_t s, const g1a *pts, uint64_t n, uint32_t c, g1a *table);
void launch_fb_msm_shared(hipStream_t s, const g1a *table, uint32_t c, const fr *scalars, uint64_t sc_stride, uint64_t n, uint64_t batch, void *workspace, g1j *out,
                          bool to_kilic, bool projective);
// the paired-point layout (k_msm.hip, fb_pair_index.hpp): table[g E + idx(d0, d1)] = d0 P_2g + d1 P_2g+1, E = fb_paired_entries(c), W = fb_paired_windows(c)
// accumulators per blob and W additions per coefficient; digit widths FB_PAIRED_LOW_BITS .. FB_PAIRED_MAX_BITS
inline double fb_paired_bytes(uint64_t n, uint32_t c) { return (double)fb_paired_table_bytes(n, c, 2 * sizeof(fp)); }
size_t fb_paired_workspace_bytes(uint64_t n, uint64_t batch, uint32_t c);
hipError_t launch_fb_build_paired(hipStream_t s, const g1a *pts, uint64_t n, uint32_t c, g1a *table);
void launch_fb_msm_paired(hipStream_t s, const g1a *table, uint32_t c, const fr *scalars, uint64_t sc_stride, uint64_t n, uint64_t batch, void *workspace, g1j *out,
                          bool to_kilic, bool projective);

// out[(b, f, jj)] = scalars[b][f * row + j0 + jj] * P[f * row + j0 + jj] over a fixed-base table of table_n = nfiles * row points
// (glv, here and below: the table holds ceil(128 / c) windows and both GLV halves of every scalar walk them)
void launch_fb_mul_vec(hipStream_t s, const g1a *table, uint64_t table_n, uint32_t c, uint32_t nwin, const fr *scalars, uint64_t row, uint64_t j0,
                       uint64_t cnt, uint64_t batch, g1j *out, bool glv = false);
// the same stage fused with the first two decimation-in-frequency stages of the inverse G1 transform (single-file tables, N >= 4):
// out[b][.] = two DIF stages applied to (scalars[b][j] * P_j)_j; roots = ReverseRootsOfUnity (Montgomery) of width W
void launch_fb_mul_vec_dif2(hipStream_t s, const g1a *table, uint64_t table_n, uint32_t c, uint32_t nwin, const fr *scalars, const fr *roots, uint64_t W,
                            uint64_t batch, g1j *out, bool glv = false);
// all files of an output position summed in one lane: out[b][jj] = sum_f scalars[b][f * row + j0 + jj] * P[f * row + j0 + jj]
void launch_fb_mul_vec_files(hipStream_t s, const g1a *table, uint64_t table_n, uint32_t c, uint32_t nwin, const fr *scalars, uint64_t row, uint64_t j0,
                             uint64_t cnt, uint64_t batch, g1j *out, bool glv = false);
void launch_g1_sum_files(hipStream_t s, const g1j *tmp, uint64_t nfiles, uint64_t cnt, uint64_t batch, g1j *out);

// ---------------- k_pairing.hip ----------------
// verification (pairing.hpp): G2 images are Kilic's (g2.hpp g2j), prepared points hold the 68 line coefficients of the Miller loop
struct g2j; struct g2_prepared;
void launch_g2_from_compressed(hipStream_t s, const uint8_t *in96, g2j *out_kilic, uint64_t n, uint32_t *bad_flag);
void launch_g2_prepare(hipStream_t s, const g2j *in_kilic, uint64_t n, g2_prepared *out);
void launch_pairs_g1_from_kilic(hipStream_t s, const g1j *a1, const g1j *b1, uint64_t n, g1j *p0, g1j *p1);   // p0 = -a1, p1 = b1 (internal domain)
// KZG checks: p0 = C - E + [b] pi, p1 = -pi with E = [y] G1 (ys != null) or es[i]; Kilic images / Kilic-Montgomery scalars in
void launch_kzg_check_inputs(hipStream_t s, const g1j *c, const g1j *pi, const fr *ys, const g1j *es, const fr *bs, uint64_t n, g1j *p0, g1j *p1);
// CheckProofMulti's coset scaling over `count` rows of np values: row b times x_b^-i, xpow_n[b] = x_b^np
void launch_fr_rows_scale_by_inv_powers(hipStream_t s, fr *c, uint64_t np, const fr *xs, uint64_t count, fr *xpow_n);
// eth.VerifyKZGProof's byte inputs: status 0 valid, 2 z or y >= r, 3 undecodable commitment / proof
void launch_eth_check_inputs(hipStream_t s, const uint8_t *c48, const uint8_t *zs, const uint8_t *ys, const uint8_t *pi48, uint64_t n, g1j *p0, g1j *p1, uint8_t *status);
// ok[i] = e(p0[i], Q0) e(p1[i], Q1) == 1; shared_lines: Q0 = q0[0], Q1 = q1[0] for every check, else q0[i], q1[i]
void launch_pairing_check(hipStream_t s, bool shared_lines, const g2_prepared *q0, const g2_prepared *q1, const g1j *p0, const g1j *p1, uint64_t n, uint8_t *ok);
void launch_pairing_value(hipStream_t s, const g1j *g1_kilic, const g2_prepared *q, uint64_t n, fp *out);   // test hook: reduced e(g1[i], Q_i), standard form
bool pairing_route_is_wave(uint64_t n);   // which kernel launch_pairing_check runs for n checks under the current environment (KZG_HIP_PAIRING)

// ---------------- k_pairing_wave.hip ----------------
// the same check with one wavefront (one workgroup) per check (wave_pairing.hpp): the route of launch_pairing_check below PAIRING_WAVE_BELOW checks
// Measured (profiles/verify.md, both routes in one run on one MI355X, best of three): the wavefront kernel is faster at every count up to 16 384
// (1: 7.9 against 39.1 ms, 8192: 22.0 against 44.7, 16 384: 39.2 against 47.6; spreads below 0.2 ms); 65 536 was measured on the lane route only
constexpr uint64_t PAIRING_WAVE_BELOW = 16385;
void launch_pairing_check_wave(hipStream_t s, bool shared_lines, const g2_prepared *q0, const g2_prepared *q1, const g1j *p0, const g1j *p1, uint64_t n, uint8_t *ok);
void launch_pairing_value_wave(hipStream_t s, const g1j *g1_kilic, const g2_prepared *q, uint64_t n, fp *out);   // test hook: launch_pairing_value's twin
void launch_wave_fp12_op(hipStream_t s, int op, const fp *a, const fp *b, uint64_t n, fp *out);                  // test hook: one tower operation per workgroup, standard form

// ---------------- k_g2.hip ----------------
// the G2 half of a setup (g2.hpp): the fixed-base table of bls.GenG2 (G2_FB_ENTRIES affine entries, device-internal domain), the walk over it
// (Montgomery scalars in, device-internal Jacobian images out), the API's output form (Kilic images, Z = 1, infinity (0, 1, 0)) and compression
struct g2a;
void launch_g2_fixed_base_table(hipStream_t s, g2a *table);
void launch_g2_fixed_base(hipStream_t s, const fr *scalars, uint64_t n, const g2a *table, g2j *out);
void launch_g2_normalize(hipStream_t s, const g2j *in, uint64_t n, g2j *out_kilic);
void launch_g2_compress(hipStream_t s, const g2j *in_kilic, uint64_t n, uint8_t *out96);

// ---------------- k_eth_aggregate.hip ----------------
// eth.VerifyAggregateKZGProof over a chunk of sidecars: off[j] .. off[j + 1] (sidecars + 1 entries) are sidecar j's blobs and commitments
// within the chunk's raw bytes (blobs: n x 32 little-endian bytes each; comms: 48 bytes each).  Challenges and powers are Montgomery images.
void launch_eth_transcripts(hipStream_t s, const uint8_t *blobs, const uint8_t *comms, const uint64_t *off, uint64_t n, uint64_t sidecars, fr *r_out, fr *z_out);
// the same chain in two halves (the batched prover): st[8 j ..] = the SHA state after the header and all blob bytes of sidecar j but the last 32
// (no commitment needed); the finish half resumes there with those 32 bytes and the compressed commitments
void launch_eth_transcript_blobs(hipStream_t s, const uint8_t *blobs, const uint64_t *off, uint64_t n, uint64_t sidecars, uint32_t *st);
void launch_eth_transcript_finish(hipStream_t s, const uint8_t *blobs, const uint8_t *comms, const uint64_t *off, uint64_t n, uint64_t sidecars, const uint32_t *st,
                                  fr *r_out, fr *z_out);
// status[j] = code_blob where agg_status[j], else code_z where z_in_domain[j], else 0; zero bytes over the proof and the commitments (may be null) of a failed row
void launch_eth_prove_finish(hipStream_t s, const uint8_t *agg_status, const uint32_t *z_in_domain, const uint64_t *off, uint64_t sidecars, uint8_t code_blob,
                             uint8_t code_z, uint8_t *proofs48, uint8_t *comms48, uint8_t *status);
// agg[j][i] = sum_k r_j^k blob_(j,k)[i]; status[j] = 2 where an element of the sidecar is not below r (status is otherwise left alone)
void launch_eth_agg_poly(hipStream_t s, const uint8_t *blobs, const uint64_t *off, const fr *r, uint64_t n, uint64_t sidecars, fr *agg, uint8_t *status);
void launch_eth_powers(hipStream_t s, const fr *r, const uint64_t *off, uint64_t sidecars, fr *pow);   // pow[off[j] + k] = r_j^k
// launch_g1_decompress with bad[row] = 0 / 1 per row; device-internal images, or Kilic images when to_kilic
void launch_g1_decompress_rows(hipStream_t s, const uint8_t *in48, g1j *out, uint64_t n, uint8_t *bad, bool to_kilic);
// out[j] = sum of pts[off[j] .. off[j + 1]) (device-internal; none: inf), out_kilic[j] its Kilic image; status[j] = 3 where one of the
// sidecar's pt_bad is set and status[j] was 0
void launch_g1_segment_sum(hipStream_t s, const g1j *pts, const uint8_t *pt_bad, const uint64_t *off, uint64_t sidecars, g1j *out, g1j *out_kilic, uint8_t *status);
// y[j] = 0 where z_in_domain[j]; status[j] = 3 where proof_bad[j] and status[j] was 0
void launch_eth_agg_finish(hipStream_t s, const uint32_t *z_in_domain, const uint8_t *proof_bad, uint64_t sidecars, fr *y, uint8_t *status);
// test hooks: SHA-256 of rows messages data[offsets[t] .. + lens[t]) and hashToBLSField's reduction of rows digests, one per lane
void launch_test_sha256_lanes(hipStream_t s, const uint8_t *data, const uint64_t *offsets, const uint64_t *lens, uint64_t rows, uint32_t *out);
void launch_test_hash_to_bls_field_lanes(hipStream_t s, const uint8_t *digests, uint64_t rows, fr *out);

// ---------------- k_eth_exec.hip ----------------
// the execution-layer side of eth/eth.go in batches (lane bodies: eth_exec.hpp)
void launch_eth_versioned_hashes(hipStream_t s, const uint8_t *c48, uint64_t n, uint8_t *out32);   // out32[t] = KZGToVersionedHash(c48[t]); out32 4-byte aligned
// PointEvaluationPrecompile's 192-byte rows: status 0 valid, 4 versioned hash mismatch, 2 z or y >= r, 3 undecodable commitment / proof
void launch_eth_precompile_inputs(hipStream_t s, const uint8_t *in192, uint64_t n, g1j *p0, g1j *p1, uint8_t *status);
void launch_eth_merge_status(hipStream_t s, const uint8_t *status, const uint8_t *ok, uint64_t n, uint8_t *result);   // result[t] = status[t] ? status[t] : ok[t]
// VerifyKZGCommitmentsAgainstTransactions' comparison: match[t] = (KZGToVersionedHash(c48[t]) == want32[t]) over `total` commitments, then
// result[j] = 1 when every flag of off[j] .. off[j + 1] (blocks + 1 entries) is set, else 4
void launch_eth_tx_hashes_check(hipStream_t s, const uint8_t *c48, const uint8_t *want32, const uint64_t *off, uint64_t total, uint64_t blocks, uint8_t *match,
                                uint8_t *result);

// ---------------- k_verify_combine.hip ----------------
// batches of KZG checks by random linear combination per group of R consecutive rows (lane bodies and the layout of a group's terms:
// verify_combine.hpp).  sc / out: combine_group_count(count, R) slices of combine_term_stride(R) slots
struct combine_seed;
// term scalars (Montgomery) of rows row0 .. row0 + count of the call from their x and y (Montgomery); status (nullable): non-zero rows get weight 0
void launch_combine_scalars(hipStream_t s, const combine_seed &seed, const fr *xs, const fr *ys, const uint8_t *status, uint64_t row0, uint64_t count, uint64_t R, fr *sc);
// term points as they came in (Kilic images when kilic, else device-internal); slot 2 R of group g: the generator in the same form, or last[g]
void launch_combine_points(hipStream_t s, const g1j *c, const g1j *pi, uint64_t count, uint64_t R, bool kilic, g1j *out, const g1j *last = nullptr);
void launch_combine_negate(hipStream_t s, const g1j *a, uint64_t n, g1j *out);   // out[g] = -a[g]
// eth form: z, y as Montgomery images and status 0 / 2 / 3 per row from the bytes and the decompression flags of commitment and proof
void launch_eth_combine_fields(hipStream_t s, const uint8_t *zs, const uint8_t *ys, const uint8_t *c_bad, const uint8_t *pi_bad, uint64_t n, fr *z_out, fr *y_out,
                               uint8_t *status);

// ---------------- k_verify_combine_multi.hip ----------------
// the multi-proof form (verify_combine_multi.hpp) over rows row0 .. row0 + count of the call: coef = the inverse transform of the rows' values,
// np <= COMBINE_MULTI_NP_MAX coefficients per row.  sc: the groups' slices (r at j, r x^np at R + j, -1 at 2 R); partials: groups x
// combine_multi_tiles(R) x np scratch; J: groups x np, the scalars of [J_g(s)]_1 over the setup's first np points
void launch_combine_multi_scalars(hipStream_t s, const combine_seed &seed, const fr *xs, const fr *coef, uint64_t np, uint64_t row0, uint64_t count, uint64_t R, fr *sc,
                                  fr *partials, fr *J);

// profiling hook (HIP events around the dominant kernel), see capi.hip
void prof_begin(hipStream_t s, const char *name);
void prof_end(hipStream_t s, const char *name);

}  // namespace kzg
