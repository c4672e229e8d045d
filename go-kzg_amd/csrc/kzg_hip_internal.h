/*
 * kzg_hip_internal.h -- instrumentation exports of libkzg_hip.so that are NOT part of the drop-in boundary (include/kzg_hip.h): the hooks
 * bench.py, tools/ and the tests use to measure and to check the library from outside.  A Go / cgo caller never needs them; they are exported
 * (default visibility) only so that ctypes can reach them.  Implemented in capi_bench.hip (capi_eth.hip for the SHA-256 hook, capi_core.hip for the G1 transform's).
 */
#ifndef KZG_HIP_INTERNAL_H
#define KZG_HIP_INTERNAL_H
#include "../../include/kzg_hip.h"
#ifdef __cplusplus
extern "C" {
#endif
#pragma GCC visibility push(default)

/* ---- roofline legs of bench.py: HIP-event time of the dominant kernel since the last reset (ms) and launch count ---- */
void kzg_hip_prof_reset(kzg_hip_fft *fs, int enable);
int kzg_hip_prof_read(kzg_hip_fft *fs, const char *kernel, double *total_ms, uint64_t *launches);
/* live calibration for the roofline: lane-operations per second of v_mad_u64_u32 and v_add_u32 and lazy 13-limb F_p products per
 * second (8 resident waves per SIMD, independent chains) on the handle's device */
int kzg_hip_calibrate(kzg_hip_fft *fs, double *mad_per_s, double *add_per_s, double *fp_mul_per_s);
/* drop-in measurement: `threads` host threads each make `calls` blocking one-polynomial calls (op 0: kzg_hip_commit_to_poly,
 * op 1: kzg_hip_compute_proof_single) on host buffers taken round-robin from blobs_fr (nblobs x n Fr); out_g1 holds `threads`
 * points (each thread's last result); *seconds = wall time from the common start to the last return */
int kzg_hip_bench_drop_in(kzg_hip_kzg *ks, int op, const void *blobs_fr, uint64_t n, uint64_t nblobs, unsigned threads, unsigned calls, void *out_g1,
                          double *seconds);
/* the same for kzg_hip_eth_compute_kzg_proof: thread t evaluates at z = 5 + t; out48 holds `threads` proofs (each thread's last) */
int kzg_hip_bench_drop_in_eth_proof(kzg_hip_eth *eth, const void *polys_fr, uint64_t n, uint64_t npolys, unsigned threads, unsigned calls, void *out48,
                                    double *seconds);
/* and for kzg_hip_fft_fr on host buffers (thread t transforms row t % nrows of vals_fr, nrows x n Fr; out_fr: threads x n Fr): the
 * per-handle stream pool at work */
int kzg_hip_bench_threads_fft_fr(kzg_hip_fft *fs, const void *vals_fr, uint64_t n, uint64_t nrows, unsigned threads, unsigned calls, void *out_fr, double *seconds);
/* bls.PolyLinComb over device-resident rows (bls/globals.go:155-178): out[i] = sum_c scalars[c] * vectors[c * stride + i]; bench.py forms the random
 * linear combination of a timed step's input polynomials with it when it checks ALL outputs of the step */
int kzg_hip_bench_poly_lincomb_dev(kzg_hip_fft *fs, const void *d_vectors_fr, uint64_t stride, const void *d_scalars_fr, uint64_t count, uint64_t n, void *d_out_fr,
                                   void *stream);
/* statistics of the request coalescer behind the one-polynomial calls of a KZG handle (op 0: CommitToPoly, 1: ComputeProofSingle), cumulative since its first call:
 * out[0..7] = requests, batches, ns executing, ns waiting for a device slot, ns gathering callers, ns waiting for row copies, largest concurrency estimate, batches
 * allowed in flight; all zero before the first call.  bench.py prints the 256-caller run's figures with it (drop_in.coalescer_256) */
int kzg_hip_coalesce_stats(kzg_hip_kzg *ks, int op, uint64_t out[8]);
/* test / measurement hook for the F_p inversion (device-internal Montgomery images, 48 bytes each, host buffers): element i is inverted by wavefront i cooperatively
 * (coop_inv.hpp) into out_coop and by one lane alone (inv<FpP>, field.hpp) into out_lane; either output may be null.  *ms_coop / *ms_lane (nullable): HIP-event time of
 * the respective launch */
int kzg_hip_test_fp_inv(kzg_hip_fft *fs, const void *in_fp, uint64_t n, void *out_coop, void *out_lane, double *ms_coop, double *ms_lane);
/* kzg_hip_lincomb_g1's promotion of repeated caller-supplied point sets (capi_core.hip): sets promoted so far on this handle, calls served by a promoted set */
int kzg_hip_lincomb_promotions(kzg_hip_fft *fs, uint64_t *promoted, uint64_t *served);
/* the same for F_r (Kilic's Montgomery images, 32 bytes each): wave-cooperative, one lane, and the workgroup batch inversion of the eth quotient kernel (one inversion per
 * 1024 values; zero inputs are treated as one there) */
int kzg_hip_test_fr_inv(kzg_hip_fft *fs, const void *in_fr, uint64_t n, void *out_coop, void *out_lane, void *out_block);
/* test hook: SHA-256 of a host buffer through the transcript's implementation (x86 SHA extensions or the portable loop; no device needed) */
void kzg_hip_test_sha256(const void *data, uint64_t len, void *out32);
/* test hooks of the block verifier's transcript kernel (k_eth_aggregate.hip, sha256_lane.hpp): the SHA-256 digests of `rows` messages
 * data[offsets[t] .. offsets[t] + lens[t]) hashed ON THE DEVICE, one message per lane of one launch (out32: rows x 32 bytes), and
 * hashToBLSField's reduction of `rows` given 32-byte digests (read as little-endian integers, reduced mod r; out_fr: rows Fr) */
int kzg_hip_test_sha256_lanes(kzg_hip_fft *fs, const void *data, const uint64_t *offsets, const uint64_t *lens, uint64_t rows, void *out32);
int kzg_hip_test_hash_to_bls_field_lanes(kzg_hip_fft *fs, const void *digests32, uint64_t rows, void *out_fr);
/* test hook of the batched block prover (capi_eth_prove.hip): how many chunks of whole sidecars the calling thread's last successful
 * kzg_hip_eth_compute_aggregate_kzg_proof_batch[_dev] ran as (KZG_HIP_ETH_PROVE_CHUNK_MB) */
uint64_t kzg_hip_test_eth_prove_chunks(void);

/* test hook of the pairing (k_pairing.hip): out_fp12[i] = e(g1[i], g2[i]) raised to 3 (p^12 - 1) / r (the exponent of pairing.hpp's final
 * exponentiation), 12 F_p elements of 48 bytes each in STANDARD form, order c0.c0.c0, c0.c0.c1, ..., c1.c2.c1; G1 / G2 Kilic images in */
int kzg_hip_pairing_test(kzg_hip_fft *fs, const void *g1, const void *g2, uint64_t n, void *out_fp12);
/* its twin on the kernel with one wavefront per check (k_pairing_wave.hip): the same bytes */
int kzg_hip_pairing_test_wave(kzg_hip_fft *fs, const void *g1, const void *g2, uint64_t n, void *out_fp12);
/* test hook of the tower on a wavefront (wave_tower.hpp): out[i] = op(a[i], b[i]), one workgroup per row, rows of 12 F_p elements in STANDARD form.
 * op: 0 mul, 1 sqr, 2 inv, 3 frob, 4 frob2, 5 frob3, 6 cyclotomic sqr, 7 conj, 8 mul_014 (b holds c0, c1, c4 as its first three F_p2) */
int kzg_hip_test_wave_fp12_op(kzg_hip_fft *fs, int op, const void *a, const void *b, uint64_t n, void *out);
/* which kernel launch_pairing_check would run for n checks under the current environment (KZG_HIP_PAIRING = lane / wave, read per call):
 * out[0] = 1 one wavefront per check, 0 one lane per check; out[1] = the count below which the wavefront kernel is the default */
int kzg_hip_test_pairing_route(uint64_t n, uint64_t out[2]);

/* test hooks of the _combined proof checks (capi_verify.hip, verify_combine.hpp).
 * kzg_hip_test_combine_points: A_g = sum r_i pi_i and B_g = sum r_i C_i + sum (r_i x_i) pi_i - (sum r_i y_i) G1 of every group of
 * KZG_HIP_VERIFY_COMBINE_ROWS consecutive rows, for the inputs of kzg_hip_check_proof_single_batch_combined and a seed (not NULL), as normalised
 * Kilic images (infinity (0, R, 0)): ceil(count / rows) points each.  KZG_HIP_ERR_TOO_WIDE for more groups than one launch holds.
 * kzg_hip_test_combine_stats: what the calling thread's last _combined call did -- out[0] = 1 the combination ran, 0 the per-row path; out[1] = group
 * checks made; out[2] = groups that failed; out[3] = rows re-checked one by one; and the routing now: out[4] = the count from which the default
 * combines, out[5] = rows per group */
int kzg_hip_test_combine_points(kzg_hip_kzg *ks, const void *commitments_g1, const void *proofs_g1, const void *xs_fr, const void *ys_fr, uint64_t count,
                                const uint8_t *seed32, void *out_a_g1, void *out_b_g1);
int kzg_hip_test_combine_stats(uint64_t out[6]);
/* the same for kzg_hip_check_proof_multi_batch_combined (verify_combine_multi.hpp).
 * kzg_hip_test_combine_multi_points: A_g and B_g = sum r_i C_i + sum (r_i x_i^np) pi_i - [J_g(s)]_1 of every group as normalised Kilic images, and
 * J_g[j] = sum r_i x_i^-j c_i[j] as ceil(count / rows) x np Montgomery values.  KZG_HIP_ERR_TOO_WIDE for more groups than one chunk holds and
 * for np > 256.
 * kzg_hip_test_combine_multi_route: out[0] = 1 when a call with `count` rows of n values would combine under the current environment, 0 the
 * per-row path; out[1] = the count from which the default combines */
int kzg_hip_test_combine_multi_points(kzg_hip_kzg *ks, const void *commitments_g1, const void *proofs_g1, const void *xs_fr, const void *ys_fr, uint64_t n, uint64_t count,
                                      const uint8_t *seed32, void *out_a_g1, void *out_b_g1, void *out_j_fr);
int kzg_hip_test_combine_multi_route(uint64_t n, uint64_t count, uint64_t out[2]);

/* test hook of the G2 half of a setup (capi_verify.hip): how many times the handle built its fixed-base table of bls.GenG2 -- 0 before the first
 * kzg_hip_g2_mul_generator_vec / kzg_hip_generate_testing_setup_g2, 1 ever after, however many threads made the first call at once */
int kzg_hip_test_g2_table_builds(kzg_hip_fft *fs, uint64_t *builds);

/* test hooks of the G1 transform (capi_core.hip).  A stage launch of the radix-2 network runs one of 13 device variants; g1_fft_stage_plan (k_g1.hip) chooses it and
 * these hooks report and force its choice.  A plan is three words: lanes per butterfly (1, 2, 4), schedule of the twiddle multiplication (0 regular odd digits, 1
 * width-5 NAF), digits from the twiddles' precomputed rows (0 / 1).
 * kzg_hip_test_g1_fft_plan: out[0..2] = the plan the library chooses, by size and by the environment's switches, for the stage of half-size m of `batch` transforms
 * of n points (dif: the decimation-in-frequency stage); out[3] = log2 of the radix of the direct passes for (n, batch), 0 = the radix-2 network; out[4] = their lanes
 * per (output, term). */
int kzg_hip_test_g1_fft_plan(kzg_hip_fft *fs, uint64_t n, uint64_t batch, uint64_t m, int dif, uint32_t out[5]);
/* runs exactly ONE stage launch on batch x n caller points (Kilic images with any Jacobian Z, host buffers), taken as the stage's input state as they are (no bit
 * reversal): butterflies (i0, i1 = i0 + m), i0 = g 2m + j, twiddle roots[j W / (2m)] of the reversed (inv) or expanded table; DIT (x + w y, x - w y), DIF
 * (x + y, (x - y) w).  lanes: 0 by size, 1, 2, 4; mul: 0 by shape, 1 regular, 2 wnaf -- what KZG_HIP_G1_QUAD and KZG_HIP_G1_MUL force per process, per call (with
 * several lanes the NAF schedule runs only where every wavefront holds one twiddle, forced or not).  out_g1: normalised Kilic images; plan_out (nullable): the plan that ran */
int kzg_hip_test_g1_fft_stage(kzg_hip_fft *fs, const void *pts_g1, uint64_t n, uint64_t batch, uint64_t m, int inv, int dif, int lanes, int mul, void *out_g1,
                              uint32_t plan_out[3]);
/* a whole transform on the direct passes (launch_g1_fft_direct) with the radix 2^max_logr (1 .. 4) and the lanes per (output, term) (1, 2, 4) of EVERY pass forced.
 * pts_g1: batch rows of n_valid points, zero-padded to n on the device; inv folds 1 / n into the last pass; n_out: 0, or only the first n_out outputs of each row
 * are computed (the rest of out_g1, batch x n normalised Kilic images, is unspecified) */
int kzg_hip_test_g1_fft_direct(kzg_hip_fft *fs, const void *pts_g1, uint64_t n, uint64_t n_valid, uint64_t batch, int inv, uint32_t max_logr, int lanes, uint64_t n_out,
                               void *out_g1);

#pragma GCC visibility pop
#ifdef __cplusplus
}
#endif
#endif
