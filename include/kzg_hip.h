/*
 * kzg_hip.h -- C ABI of libkzg_hip.so: the MI355X (gfx950) implementation of go-kzg's commitment /
 * proof hot path.  Each entry point replaces one batch-level method of the reference's Go API
 * (file:line relative to protolambda/go-kzg); the cgo binding a maintainer would add is in
 * INTEGRATION.md and go-kzg_amd/goshim/.
 *
 * Data crossing the boundary uses the memory images of the reference's default (Kilic) backend, so Go
 * slices are passed zero-copy:
 *   Fr  : 32 B  = 4 x u64 little-endian limbs, Montgomery form (R = 2^256 mod r)      bls/bignum_kilic.go:21-23
 *   G1  : 144 B = 3 x 6 x u64 (X, Y, Z) Jacobian, Montgomery (R = 2^384 mod p), inf <=> Z == 0
 *                                                                                     bls/bls_kilic.go:30-35
 *   G2  : 288 B = 3 x 2 x 6 x u64 (X, Y, Z) Jacobian over F_p2, each coordinate (c0, c1) Montgomery (R = 2^384 mod p),
 *         inf <=> Z == 0                                                              bls/bls_kilic.go:57-62
 * Returned points are normalised: Z == R (affine) or Kilic's infinity image (0, R, 0), so that byte
 * comparison with any correct backend is meaningful.  Callers own all buffers; the library keeps no
 * caller pointer after a call returns (cgo rule).  All calls are blocking and thread-safe per handle.
 * Concurrent ONE-polynomial calls on a handle (kzg_hip_commit_to_poly, _compute_proof_single, _da_using_fk20, _da_using_fk20_multi,
 * _lincomb_points, _eth_blob_to_kzg_commitment_batch with batch == 1, _eth_compute_kzg_proof) are merged into batched launches (go-kzg_amd/csrc/coalesce.hpp; KZG_HIP_COALESCE=0
 * turns that off); a lone caller is not delayed.
 *
 * Functions ending in _dev take DEVICE pointers (HBM-resident inputs/outputs) and a hipStream_t passed
 * as void*; they enqueue work and return without synchronising the caller's stream.  (The FIRST commitment on a settings object builds
 * its fixed-base table: that call blocks its host thread until the build -- on the handle's own stream -- is done; the caller's stream is
 * not drained.)
 */
#ifndef KZG_HIP_H
#define KZG_HIP_H
#include <stdint.h>
#ifdef __cplusplus
extern "C" {
#endif
#pragma GCC visibility push(default)

/* status codes.  The Go shim maps 1-2 to `error` (fft_fr.go:57-59,78-83; fft_g1.go:60-65) and 3-6 to panic
 * (bls/bls_kilic.go:133-135; kzg.go:22-27,44-52,74-91; fk20_single.go:60-62,140-154; fk20_multi.go:28-31,60-69). */
#define KZG_HIP_OK 0
#define KZG_HIP_ERR_TOO_WIDE 1      /* more values than roots of unity */
#define KZG_HIP_ERR_NOT_POW2 2      /* length is not a power of two */
#define KZG_HIP_ERR_LEN_MISMATCH 3  /* slice lengths do not match / setup too short */
#define KZG_HIP_ERR_UPPER_HALF 4    /* "bad input, second half should be zeroed" */
#define KZG_HIP_ERR_BAD_ARG 5       /* other misuse (n < 2, chunk length, NULL, ...) */
#define KZG_HIP_ERR_BAD_POINT 6     /* invalid compressed G1 */
#define KZG_HIP_ERR_NO_DEVICE 7     /* no gfx950 device visible: the library has NO CPU fallback */
#define KZG_HIP_ERR_HIP 8           /* HIP runtime error, see kzg_hip_last_error() */
#define KZG_HIP_ERR_UNSUPPORTED 9    /* a size class this library does not serve: kzg_hip_fft_settings_new with KZG_HIP_MAX_SCALE < max_scale <= 31 */
#define KZG_HIP_ERR_RECOVERY 10      /* "failed to reconstruct data correctly" (recover_from_samples.go:103-107) */
#define KZG_HIP_ERR_BAD_BLOB 11      /* "could not convert blobs to polynomials" (eth/eth.go:156-159,176-179): a field element >= r */

typedef struct kzg_hip_fft kzg_hip_fft;                 /* *kzg.FFTSettings         fft.go:34-42   */
typedef struct kzg_hip_kzg kzg_hip_kzg;                 /* *kzg.KZGSettings         kzg.go:11-19   */
typedef struct kzg_hip_fk20s kzg_hip_fk20s; /* *kzg.FK20SingleSettings  kzg.go:38-41   */
typedef struct kzg_hip_fk20m kzg_hip_fk20m; /* *kzg.FK20MultiSettings   kzg.go:66-71   */

/* ---- library / device ---- */
int kzg_hip_device_count(void);                 /* number of usable gfx950 devices (0 when none)            */
const char *kzg_hip_last_error(void);           /* thread-local text of the last KZG_HIP_ERR_HIP            */
const char *kzg_hip_version(void);

/* Pinning of caller memory (optional).  kzg_hip_commit_to_poly_batch and kzg_hip_eth_blob_to_kzg_commitment_batch (and their multi-device forms) check whether
 * their INPUT lies in pinned memory and then read the coefficients in place over PCIe instead of staging a copy of pageable memory: 67-78 k -> ~95 k commitments/s from host
 * buffers on one GPU.  The range stays pinned (and visible to every device) until kzg_hip_host_unregister; a Go caller pins the slice first (runtime.Pinner). */
int kzg_hip_host_register(void *host, uint64_t bytes);
int kzg_hip_host_unregister(void *host);

/* ---- FFTSettings: NewFFTSettings (fft.go:44-61) ----
 * max_scale <= KZG_HIP_MAX_SCALE (2^24 roots: 6 root tables of 0.5 GB + the G1 twiddles' digit rows, 8.9 GB); the reference's root table goes to
 * scale 31 (bls/globals.go:27-60), whose tables would not fit any device: KZG_HIP_MAX_SCALE < max_scale <= 31 returns KZG_HIP_ERR_UNSUPPORTED, larger
 * values KZG_HIP_ERR_BAD_ARG (the reference indexes past its table there).  Transforms are parity-tested up to 2^20 points
 * (tests/test_gpu_parity.py::test_fft_fr_above_65536). */
#define KZG_HIP_MAX_SCALE 24
int kzg_hip_fft_settings_new(int device, unsigned max_scale, kzg_hip_fft **out);
void kzg_hip_fft_settings_free(kzg_hip_fft *fs);
uint64_t kzg_hip_fft_max_width(const kzg_hip_fft *fs);
/* copies ExpandedRootsOfUnity (reversed == 0) or ReverseRootsOfUnity (reversed != 0): max_width + 1 Fr */
int kzg_hip_fft_roots(const kzg_hip_fft *fs, int reversed, void *out_fr);

/* FFTSettings.FFT (fft_fr.go:55-74): zero-pads n to the next power of two np; out must hold np Fr; *out_n = np */
int kzg_hip_fft_fr(kzg_hip_fft *fs, const void *vals_fr, uint64_t n, int inv, void *out_fr, uint64_t *out_n);
/* FFTSettings.InplaceFFT (fft_fr.go:76-105): n must be a power of two, out != vals */
int kzg_hip_inplace_fft_fr(kzg_hip_fft *fs, const void *vals_fr, void *out_fr, uint64_t n, int inv);
/* `batch` independent transforms of n (power of two) contiguous values each */
int kzg_hip_fft_fr_batch(kzg_hip_fft *fs, const void *vals_fr, uint64_t n, uint64_t batch, int inv, void *out_fr);
/* FFTSettings.FFTG1 (fft_g1.go:58-94) */
int kzg_hip_fft_g1(kzg_hip_fft *fs, const void *vals_g1, uint64_t n, int inv, void *out_g1);
/* FFTSettings.DASFFTExtension (das_extension.go:71-84): in place, n even-index values -> n odd-index values */
int kzg_hip_das_fft_extension(kzg_hip_fft *fs, void *vals_fr, uint64_t n);
int kzg_hip_das_fft_extension_batch(kzg_hip_fft *fs, void *vals_fr, uint64_t n, uint64_t batch);

/* device-resident batch forms of the three transforms the reference publishes benchmarks for (BENCH.md:31,43,55):
 * `batch` rows of n values each, inputs and outputs in HBM, Kilic images for G1 (converted and normalised inside).  d_out must not
 * overlap d_vals (InplaceFFT's rule, fft_fr.go:76: the name notwithstanding it takes a separate output slice). */
int kzg_hip_fft_fr_batch_dev(kzg_hip_fft *fs, const void *d_vals_fr, uint64_t n, uint64_t batch, int inv, void *d_out_fr, void *stream);
int kzg_hip_fft_g1_batch(kzg_hip_fft *fs, const void *vals_g1, uint64_t n, uint64_t batch, int inv, void *out_g1);   /* FFTG1 on `batch` rows of n points, host buffers */
int kzg_hip_fft_g1_batch_dev(kzg_hip_fft *fs, const void *d_vals_g1, uint64_t n, uint64_t batch, int inv, void *d_out_g1, void *stream);
int kzg_hip_das_fft_extension_batch_dev(kzg_hip_fft *fs, void *d_vals_fr, uint64_t n, uint64_t batch, void *stream);

/* bls.FrFrom32 / bls.FrTo32 over a slice (bls/bignum_kilic.go:33-55; range rule bls.ValidFr, bls/bignum_all.go:12-35):
 * n x 32 little-endian bytes <-> Montgomery images.  from: *all_ok = 0 if any value is >= r (those become 0). */
int kzg_hip_fr_from_le32(kzg_hip_fft *fs, const void *in_le32, uint64_t n, void *out_fr, int *all_ok);
int kzg_hip_fr_to_le32(kzg_hip_fft *fs, const void *in_fr, uint64_t n, void *out_le32);

/* ---- bls.LinCombG1 (bls/bls_kilic.go:132-150): Pippenger MSM; n == 0 -> infinity ---- */
int kzg_hip_lincomb_g1(kzg_hip_fft *fs, const void *points_g1, const void *scalars_fr, uint64_t n, void *out_g1);
/* Cached point set for repeated LinCombG1 on the SAME points (CommitToEvalPoly's IFFT of the setup, kzg_single_proofs.go:12-14;
 * the Lagrange setup of eth/helpers.go:99,159,199): uploaded and converted once, resident in HBM with its 2^64 multiples.
 * kzg_hip_lincomb_points[_batch]: out[b] = LinCombG1(points[:n], scalars[b]); n <= the set's size (KZG_HIP_ERR_LEN_MISMATCH
 * otherwise, the reference's length-mismatch panic); n == 0 -> infinity.  The _dev form takes device pointers and a stream. */
typedef struct kzg_hip_points kzg_hip_points;
int kzg_hip_points_new(kzg_hip_fft *fs, const void *points_g1, uint64_t n, kzg_hip_points **out);
void kzg_hip_points_free(kzg_hip_points *pts);
/* A cached set of >= 64 points also gets a fixed-base table like a KZGSettings object (built by its first combination): budget in GB, default
 * KZG_HIP_POINTS_FB_BUDGET_GB or min(32 GB, free HBM - 24 GB) at creation; 0 keeps the set on the bucket pipeline.  Results are identical. */
int kzg_hip_points_set_table_budget_gb(kzg_hip_points *pts, double gb);
uint64_t kzg_hip_points_count(const kzg_hip_points *pts);
int kzg_hip_lincomb_points(kzg_hip_points *pts, const void *scalars_fr, uint64_t n, void *out_g1);
int kzg_hip_lincomb_points_batch(kzg_hip_points *pts, const void *scalars_fr, uint64_t n, uint64_t batch, void *out_g1);
int kzg_hip_lincomb_points_batch_dev(kzg_hip_points *pts, const void *d_scalars_fr, uint64_t n, uint64_t batch, void *d_out_g1, void *stream);
/* bls.ToCompressedG1 over a slice (bls/bls_kilic.go:114-116): n points -> n x 48 B ZCash form */
int kzg_hip_g1_to_compressed(kzg_hip_fft *fs, const void *points_g1, uint64_t n, void *out48);
/* bls.FromCompressedG1 over a slice (bls/bls_kilic.go:118-121) */
int kzg_hip_g1_from_compressed(kzg_hip_fft *fs, const void *in48, uint64_t n, void *out_g1);
/* element-wise bls.MulG1 (bls/bls_kilic.go:41-45): out[i] = scalars[i] * points[i] */
int kzg_hip_g1_mul_vec(kzg_hip_fft *fs, const void *points_g1, const void *scalars_fr, uint64_t n, void *out_g1);
/* GenerateTestingSetup, G1 half (setup.go:9-26): out[i] = [secret^i] G1 */
int kzg_hip_generate_testing_setup_g1(kzg_hip_fft *fs, const void *secret_fr, uint64_t n, void *out_g1);

/* G1Point.MarshalText / UnmarshalText over a slice (bls/bls_all.go:20-39): n points <-> n x 96 lower-case hex characters (no 0x
 * prefix, no terminator).  Unmarshal returns KZG_HIP_ERR_BAD_POINT for a non-hex character or an invalid point. */
int kzg_hip_g1_marshal_text(kzg_hip_fft *fs, const void *points_g1, uint64_t n, char *out_hex96);
int kzg_hip_g1_unmarshal_text(kzg_hip_fft *fs, const char *hex96, uint64_t n, void *out_g1);
/* JSONTrustedSetup (eth/globals.go:33-49): decodes the "setup_G1" and "setup_G1_lagrange" arrays of a trusted-setup JSON
 * document (the format of eth/trusted_setup.json) into Kilic images, decompressing and subgroup-checking on the device.  Other
 * keys ("setup_G2", "roots_of_unity") are skipped: kzg_hip_trusted_setup_g2_from_json decodes "setup_G2".  Counts are always written; the arrays only when
 * the out pointer is non-NULL (call once with NULL to size the buffers).  `capacity` = points each out array can hold. */
int kzg_hip_trusted_setup_from_json(kzg_hip_fft *fs, const char *json, uint64_t json_len, void *out_setup_g1, void *out_lagrange_g1,
                                    uint64_t capacity, uint64_t *n_setup_g1, uint64_t *n_lagrange_g1);

/* ---- KZGSettings: NewKZGSettings, prover side (kzg.go:21-36); the setup is uploaded once and stays in HBM ---- */
int kzg_hip_kzg_settings_new(kzg_hip_fft *fs, const void *secret_g1, uint64_t n_setup, kzg_hip_kzg **out);
void kzg_hip_kzg_settings_free(kzg_hip_kzg *ks);
/* HBM budget (GB, decimal) of the fixed-base commitment table of this settings object; call before the first commitment (a
 * later call frees the table, which is rebuilt lazily).  Default without this call: KZG_HIP_FB_BUDGET_GB, else 110 GB
 * clipped to free HBM - 24 GB (n = 4096: signed 16-bit windows, 8 of them walked by both GLV halves of a scalar: 103 GB, 16 additions per
 * coefficient); 60 selects 15-bit windows (58 GB, 18 additions), 17 selects 13-bit windows (16 GB, 20 additions). */
int kzg_hip_kzg_set_table_budget_gb(kzg_hip_kzg *ks, double gb);
/* KZGSettings.CommitToPoly (kzg_single_proofs.go:17-19) */
int kzg_hip_commit_to_poly(kzg_hip_kzg *ks, const void *coeffs_fr, uint64_t n, void *out_g1);
/* `batch` polynomials of n coefficients each -> `batch` commitments */
int kzg_hip_commit_to_poly_batch(kzg_hip_kzg *ks, const void *coeffs_fr, uint64_t n, uint64_t batch, void *out_g1);
int kzg_hip_commit_to_poly_batch_dev(kzg_hip_kzg *ks, const void *d_coeffs_fr, uint64_t n, uint64_t batch, void *d_out_g1, void *stream);
/* KZGSettings.ComputeProofSingle (kzg_single_proofs.go:36-54; poly.go:14-40): x is a uint64 as in the reference */
int kzg_hip_compute_proof_single(kzg_hip_kzg *ks, const void *poly_fr, uint64_t n, uint64_t x, void *out_g1);
/* `batch` polynomials of n coefficients each, evaluation point xs[b] for polynomial b -> `batch` proofs; the _dev form takes
 * device pointers (polynomials, uint64 xs, outputs) and a stream */
int kzg_hip_compute_proof_single_batch(kzg_hip_kzg *ks, const void *poly_fr, uint64_t n, uint64_t batch, const uint64_t *xs, void *out_g1);
int kzg_hip_compute_proof_single_batch_dev(kzg_hip_kzg *ks, const void *d_poly_fr, uint64_t n, uint64_t batch, const void *d_x_u64, void *d_out_g1,
                                           void *stream);
/* KZGSettings.ToeplitzPart2 / ToeplitzPart3 (fk20_single.go:59-87); part3 writes n/2 points */
int kzg_hip_toeplitz_part2(kzg_hip_kzg *ks, const void *coeffs_fr, const void *x_ext_fft_g1, uint64_t n, void *out_g1);
int kzg_hip_toeplitz_part3(kzg_hip_kzg *ks, const void *h_ext_fft_g1, uint64_t n, void *out_g1);

/* ---- KZG multi proofs, prover side (kzg_multi_proofs.go) ----
 * KZGSettings.ComputeProofMulti (kzg_multi_proofs.go:13-43).  The reference never initialises xPowN (:20-24), so its divisor is
 * X^n rather than X^n - x^n and the quotient is poly[n:]; reproduced faithfully (the result is a valid proof while len <= 2n). */
int kzg_hip_compute_proof_multi(kzg_hip_kzg *ks, const void *poly_fr, uint64_t len, uint64_t x, uint64_t n, void *out_g1);
/* prover-side half of CheckProofMulti (kzg_multi_proofs.go:47-75): commitment to the interpolation polynomial on x * <w_n>
 * ([I(s)]_1 = LinCombG1(SecretG1, IFFT(ys)_i / x^i)) and x^n; the pairing stays with the verifier's CPU backend. */
int kzg_hip_check_proof_multi_interpolation(kzg_hip_kzg *ks, const void *ys_fr, uint64_t n, const void *x_fr, void *out_is1_g1, void *out_xpow_fr);

/* ---- FK20 single (kzg.go:43-64; fk20_single.go:122-196) ---- */
int kzg_hip_fk20_single_settings_new(kzg_hip_kzg *ks, uint64_t n2, kzg_hip_fk20s **out);
void kzg_hip_fk20_single_settings_free(kzg_hip_fk20s *fk);
int kzg_hip_fk20_single_x_ext_fft(const kzg_hip_fk20s *fk, void *out_g1 /* n2 points */);
int kzg_hip_fk20_single(kzg_hip_fk20s *fk, const void *poly_fr, uint64_t n, void *out_g1 /* n */);
int kzg_hip_fk20_single_da_optimized(kzg_hip_fk20s *fk, const void *poly_fr, uint64_t n2, void *out_g1 /* n2 */);
/* `batch` polynomials of n coefficients -> batch x n proofs (FK20Single on each; BASELINE config 4b: n = 4096 at scale 13) */
int kzg_hip_fk20_single_batch(kzg_hip_fk20s *fk, const void *poly_fr, uint64_t n, uint64_t batch, void *out_g1);
int kzg_hip_fk20_single_batch_dev(kzg_hip_fk20s *fk, const void *d_poly_fr, uint64_t n, uint64_t batch, void *d_out_g1, void *stream);
int kzg_hip_da_using_fk20(kzg_hip_fk20s *fk, const void *poly_fr, uint64_t n, void *out_g1 /* 2n */);
/* `batch` polynomials of n coefficients -> batch x 2n proofs (DAUsingFK20 on each) */
int kzg_hip_da_using_fk20_batch(kzg_hip_fk20s *fk, const void *poly_fr, uint64_t n, uint64_t batch, void *out_g1);
int kzg_hip_da_using_fk20_batch_dev(kzg_hip_fk20s *fk, const void *d_poly_fr, uint64_t n, uint64_t batch, void *d_out_g1, void *stream);

/* ---- FK20 multi (kzg.go:73-116; fk20_multi.go:25-133) ---- */
int kzg_hip_fk20_multi_settings_new(kzg_hip_kzg *ks, uint64_t n2, uint64_t chunk_len, kzg_hip_fk20m **out);
void kzg_hip_fk20_multi_settings_free(kzg_hip_fk20m *fk);
int kzg_hip_fk20_multi(kzg_hip_fk20m *fk, const void *poly_fr, uint64_t n, void *out_g1 /* n / chunk_len */);
int kzg_hip_fk20_multi_da_optimized(kzg_hip_fk20m *fk, const void *poly_fr, uint64_t n2, void *out_g1 /* n2 / chunk_len */);
int kzg_hip_da_using_fk20_multi(kzg_hip_fk20m *fk, const void *poly_fr, uint64_t n, void *out_g1 /* 2n / chunk_len */);
/* `batch` polynomials of n coefficients -> batch x 2n / chunk_len proofs (DAUsingFK20Multi on each), host buffers */
int kzg_hip_da_using_fk20_multi_batch(kzg_hip_fk20m *fk, const void *poly_fr, uint64_t n, uint64_t batch, void *out_g1);
int kzg_hip_da_using_fk20_multi_batch_dev(kzg_hip_fk20m *fk, const void *d_poly_fr, uint64_t n, uint64_t batch, void *d_out_g1, void *stream);
/* Sharded form for one process per GPU: this rank computes hExtFFT for output positions
 * [j0, j0 + cnt) only and writes cnt points as OPAQUE 144-byte device-internal Jacobian images (not Kilic images: the
 * device keeps F_p in Montgomery radix 2^390); ranks all-gather the slices (RCCL, bytes) and call
 * kzg_hip_fk20_multi_finish_dev on the gathered 2k points, which returns normalised Kilic images. */
int kzg_hip_fk20_multi_hext_slice_dev(kzg_hip_fk20m *fk, const void *d_poly_fr, uint64_t n, uint64_t j0, uint64_t cnt, void *d_out_g1, void *stream);
int kzg_hip_fk20_multi_finish_dev(kzg_hip_fk20m *fk, const void *d_hext_g1, int bit_reverse, void *d_out_g1, void *stream);

/* ---- eth/ byte-level prover path: eth/globals.go:39-72, eth/eth.go:145-151, eth/helpers.go:98-103,179-203,264-273 ----
 * kzg_hip_eth_settings_new takes setup_G1_lagrange in NATURAL order (as eth/trusted_setup.json stores it) and applies the
 * bit-reversal permutation of eth/globals.go:48 itself; DomainFr is the bit-reversed scale-log2(n) domain (:61-66). */
typedef struct kzg_hip_eth kzg_hip_eth;
int kzg_hip_eth_settings_new(kzg_hip_fft *fs, const void *lagrange_g1, uint64_t n, kzg_hip_eth **out);
void kzg_hip_eth_settings_free(kzg_hip_eth *eth);
/* BlobToKZGCommitment over `batch` blobs of n x 32 little-endian bytes: out48[b] = commitment, ok[b] = 1, or ok[b] = 0 when a
 * field element is >= r (the reference returns (KZGCommitment{}, false): out48[b] is zeroed). */
int kzg_hip_eth_blob_to_kzg_commitment_batch(kzg_hip_eth *eth, const void *blobs_le32, uint64_t batch, void *out48, uint8_t *ok);
/* (batch == 1 is eth.BlobToKZGCommitment itself, eth/eth.go:145-151: concurrent one-blob calls on a handle are coalesced into
 * batched launches like kzg_hip_commit_to_poly's.) */
/* ComputeKZGProof (eth/helpers.go:179-203): polynomial in evaluation form (n Fr), z; writes the 48-byte proof and (optionally) y.
 * KZG_HIP_ERR_LEN_MISMATCH: "polynomial has invalid length"; KZG_HIP_ERR_BAD_ARG: "invalid z challenge" (z in the domain). */
int kzg_hip_eth_compute_kzg_proof(kzg_hip_eth *eth, const void *poly_fr, uint64_t n, const void *z_fr, void *out48, void *y_fr);
/* (one polynomial per call, like the reference: concurrent calls on a handle are coalesced into batched launches.)
 * The same over `batch` rows (polys_fr: batch x n Fr, zs_fr: batch Fr): out48[b] / ys_fr[b] (optional) and ok[b] = 1, or ok[b] = 0 with
 * out48[b] and ys_fr[b] zeroed where zs[b] lies in the domain (the reference's "invalid z challenge" for that row).  One launch chain for
 * the whole batch, no host round trip between the quotients and their commitment. */
int kzg_hip_eth_compute_kzg_proof_batch(kzg_hip_eth *eth, const void *polys_fr, uint64_t n, uint64_t batch, const void *zs_fr, void *out48, void *ys_fr, uint8_t *ok);
/* device-resident form: every pointer is device memory, work is enqueued on `stream`; d_bad_u32[b] != 0 marks an invalid z (that row's
 * proof bytes are then those of the point at infinity and must be ignored); d_ys_fr may be null */
int kzg_hip_eth_compute_kzg_proof_batch_dev(kzg_hip_eth *eth, const void *d_polys_fr, uint64_t n, uint64_t batch, const void *d_zs_fr, void *d_out48, void *d_ys_fr,
                                            void *d_bad_u32, void *stream);

/* eth.ComputeAggregateKZGProof (eth/eth.go:175-182 -> ComputeAggregateKZGProofFromPolynomials, eth/helpers.go:165-176): the blobs of one block
 * (batch x n x 32 little-endian bytes; batch == 0 is valid: the proof of the zero polynomial) -> the 48-byte aggregated proof.  On the device: the
 * polynomials, their commitments, the aggregated polynomial (bls.PolyLinComb) and its proof at the evaluation challenge; on the host, while the
 * device commits: the Fiat-Shamir transcript (hashPolysComms / hashToBLSField: one SHA-256 chain over all blobs).  out_commitments48 (optional,
 * batch x 48) receives the blobs' commitments, which the caller needs for the block anyway.
 * KZG_HIP_ERR_BAD_BLOB: "could not convert blobs to polynomials"; KZG_HIP_ERR_BAD_ARG: "invalid z challenge". */
int kzg_hip_eth_compute_aggregate_kzg_proof(kzg_hip_eth *eth, const void *blobs_le32, uint64_t batch, void *out_proof48, void *out_commitments48);
/* The prover-side pieces of eth.VerifyAggregateKZGProof (eth/eth.go:155-172): ComputeAggregatedPolyAndCommitment (eth/helpers.go:137-162) over the
 * blobs and the EXPECTED commitments (batch x 48), then y = EvaluatePolynomialInEvaluationForm(aggregatedPoly, z).  Writes the aggregated
 * commitment (one G1 Kilic image), z, y (optional) and the aggregated polynomial (n Fr, optional); the pairing check of
 * VerifyKZGProofFromPoints (eth/helpers.go:55-68) stays with the caller.  KZG_HIP_ERR_BAD_BLOB as above; KZG_HIP_ERR_BAD_POINT: a commitment does
 * not decode (:153-156).  z inside the domain (probability 2^-243): y = 0, what the reference's formula returns there (see below). */
int kzg_hip_eth_compute_aggregated_poly_and_commitment(kzg_hip_eth *eth, const void *blobs_le32, const void *commitments48, uint64_t batch, void *out_poly_fr,
                                                       void *out_commitment_g1, void *out_z_fr, void *out_y_fr);
/* bls.EvaluatePolyInEvaluationForm(y, poly, x, fs.ExpandedRootsOfUnity[:fs.MaxWidth], scale) (bls/globals.go:106-153, as called in
 * fft_fr_test.go:73-99): poly[i] = f(w^(i << scale)), n = MaxWidth >> scale (else KZG_HIP_ERR_LEN_MISMATCH: the reference's panic), barycentric
 * evaluation at x.  x one of the roots: y = 0 like the reference, whose last factor (x^n - 1) / n vanishes there whatever its batch inversion made of
 * the zero denominator (bls/globals.go:141-152) -- NOT f(x). */
int kzg_hip_evaluate_poly_in_evaluation_form(kzg_hip_fft *fs, const void *poly_fr, uint64_t n, const void *x_fr, uint32_t scale, void *out_y_fr);
/* eth.EvaluatePolynomialInEvaluationForm (eth/helpers.go:207-211): the same on DomainFr (bit-reversed order) */
int kzg_hip_eth_evaluate_polynomial_in_evaluation_form(kzg_hip_eth *eth, const void *poly_fr, uint64_t n, const void *x_fr, void *out_y_fr);

/* ---- verification (bls/bls_kilic.go:121-158, kzg_single_proofs.go:57, kzg_multi_proofs.go:47, eth/eth.go:114, eth/helpers.go:55) ----
 * BATCH forms only: one lane per check (multi-Miller loop over two pairs + final exponentiation on the device).  Results are one byte per check.
 * A check before its G2 setter is KZG_HIP_ERR_BAD_ARG; count == 0 is KZG_HIP_OK.
 * The G1 images given to kzg_hip_pairings_verify_batch and kzg_hip_check_proof_{single,multi}_batch are not checked and must lie in G1: a row
 * that holds any other curve point has an unspecified result (the call still returns KZG_HIP_OK and no other row is affected).
 * kzg_hip_g2_from_compressed: bls.FromCompressedG2 over n 96-byte ZCash encodings -> n G2 images; KZG_HIP_ERR_BAD_POINT if ANY is invalid
 * (flags, x >= p, not on the curve, not in the subgroup), like kzg_hip_g1_from_compressed. */
int kzg_hip_g2_from_compressed(kzg_hip_fft *fs, const void *in96, uint64_t n, void *out_g2);
/* The G2 half of a setup.  Outputs are G2 images normalised to Z == R, infinity as Kilic's (0, R, 0): the group elements the reference returns
 * (bls.EqualG2-equal, identical compressed bytes).  The first multiplication on a handle builds a fixed-base table of bls.GenG2 (1.5 MiB, kept
 * with the handle); a multiplication is then 32 mixed additions.
 * bls.MulG2(&out[i], &bls.GenG2, &scalars[i]) over a slice (kzg_single_proofs.go:60, kzg_multi_proofs.go:69, eth/helpers.go:57) */
int kzg_hip_g2_mul_generator_vec(kzg_hip_fft *fs, const void *scalars_fr, uint64_t n, void *out_g2);
/* GenerateTestingSetup, G2 half (setup.go:17-24): out[i] = [secret^i] G2 */
int kzg_hip_generate_testing_setup_g2(kzg_hip_fft *fs, const void *secret_fr, uint64_t n, void *out_g2);
/* bls.ToCompressedG2 over a slice (bls/bls_kilic.go:123-125): n G2 images (any Z) -> n x 96 B ZCash form, the inverse of kzg_hip_g2_from_compressed */
int kzg_hip_g2_to_compressed(kzg_hip_fft *fs, const void *points_g2, uint64_t n, void *out96);
/* the "setup_G2" array of a trusted-setup JSON document (eth/globals.go:35,47) as G2 images, decompressed and subgroup-checked on the device.
 * Protocol of kzg_hip_trusted_setup_from_json: the count is always written, the array only when the out pointer is non-NULL (KZG_HIP_ERR_LEN_MISMATCH
 * when `capacity` points do not suffice).  KZG_HIP_ERR_BAD_POINT: a non-hex character, an entry that is not 96 bytes, an invalid point.  A
 * document without the key: count 0. */
int kzg_hip_trusted_setup_g2_from_json(kzg_hip_fft *fs, const char *json, uint64_t json_len, void *out_setup_g2, uint64_t capacity, uint64_t *n_setup_g2);
/* bls.PairingsVerify over n checks: ok[i] = (e(a1[i], a2[i]) == e(b1[i], b2[i])); points at infinity contribute 1 (Kilic's AddPair) */
int kzg_hip_pairings_verify_batch(kzg_hip_fft *fs, const void *a1_g1, const void *a2_g2, const void *b1_g1, const void *b2_g2, uint64_t n, uint8_t *ok);
/* KZGSettings.SecretG2 (n >= 2 G2 images, copied): [1]G2 and [s]G2 are prepared at once, [s^n]G2 on the first multi check with n values */
int kzg_hip_kzg_set_secret_g2(kzg_hip_kzg *ks, const void *secret_g2, uint64_t n);
/* CheckProofSingle over `count` (commitment, proof, x, y): ok[i] = 1 when the proof verifies */
int kzg_hip_check_proof_single_batch(kzg_hip_kzg *ks, const void *commitments_g1, const void *proofs_g1, const void *xs_fr, const void *ys_fr, uint64_t count,
                                     uint8_t *ok);
/* CheckProofMulti over `count` (commitment, proof, x, ys[i * n .. i * n + n)): needs SecretG2[n] (else KZG_HIP_ERR_LEN_MISMATCH) */
int kzg_hip_check_proof_multi_batch(kzg_hip_kzg *ks, const void *commitments_g1, const void *proofs_g1, const void *xs_fr, const void *ys_fr, uint64_t n,
                                    uint64_t count, uint8_t *ok);
/* kzgSetupG2 (eth/globals.go:47): n >= 2 G2 images (kzg_hip_g2_from_compressed of setup_G2) */
int kzg_hip_eth_set_setup_g2(kzg_hip_eth *eth, const void *setup_g2, uint64_t n);
/* eth.VerifyKZGProof over `count` (commitment 48 B, z 32 B LE, y 32 B LE, proof 48 B): result[i] = 1 valid, 0 the pairing check failed,
 * 2 z or y not below r ("invalid evaluation point" / "invalid expected output"), 3 commitment or proof not a valid G1 encoding */
int kzg_hip_eth_verify_kzg_proof_batch(kzg_hip_eth *eth, const void *commitments48, const void *zs_le32, const void *ys_le32, const void *proofs48, uint64_t count,
                                       uint8_t *result);
/* The two batch checks above with ONE pairing check per group of consecutive rows instead of one per row, for callers whose batches are almost
 * always valid throughout.  Arguments, error codes and output bytes are those of the per-row entries.  Per group g of rows i the library draws
 * 128-bit weights r_i and checks e(B_g, [1]G2) e(-A_g, [s]G2) == 1 with A_g = sum r_i pi_i and B_g = sum r_i C_i + sum (r_i x_i) pi_i - (sum r_i y_i) G1
 * (two multi-scalar multiplications per group).  If every row of a group is valid the group passes and its rows get 1; the rows of a group that
 * fails are re-checked one by one by the per-row path, so the answer is the per-row mask.  A group that contains an invalid row passes with
 * probability at most 2^-128 over the weights, for points of G1.
 * Weights: r_i = the little-endian integer of the first 16 bytes of SHA-256(seed32 | "KZGHIPRC" | le64(i)), i the row's index in the call.
 * seed32 == NULL: the library draws 32 bytes from the operating system for the call (getrandom, else std::random_device).  A non-NULL seed is for
 * reproducible runs and tests: A SEED THAT THE PROVER CAN KNOW BEFORE IT CHOOSES ITS PROOFS VOIDS THE BOUND (invalid rows whose errors cancel
 * under known weights pass).
 * kzg_hip_check_proof_single_batch_combined takes Kilic images and PRESUPPOSES POINTS OF G1, as the reference's CheckProofSingle does: it checks
 * neither the curve equation nor the subgroup.  kzg_hip_eth_verify_kzg_proof_batch_combined decodes and subgroup-checks every point; rows with
 * result 2 or 3 keep that byte and drop out of their group's combination (weight 0), so their neighbours still pass in one group check.
 * Groups hold KZG_HIP_VERIFY_COMBINE_ROWS rows (default 1024).  KZG_HIP_VERIFY_COMBINE=never|always forces the per-row path or the combination;
 * by default small batches take the per-row path (README, "Environment knobs").  Both switches are read per call. */
int kzg_hip_check_proof_single_batch_combined(kzg_hip_kzg *ks, const void *commitments_g1, const void *proofs_g1, const void *xs_fr, const void *ys_fr,
                                              uint64_t count, const uint8_t *seed32, uint8_t *ok);
int kzg_hip_eth_verify_kzg_proof_batch_combined(kzg_hip_eth *eth, const void *commitments48, const void *zs_le32, const void *ys_le32, const void *proofs48,
                                                uint64_t count, const uint8_t *seed32, uint8_t *result);
/* kzg_hip_check_proof_multi_batch likewise (the check a DAS sampler makes on coset proofs): arguments, error codes and output bytes are the
 * per-row entry's, the weights, the seed, the groups and the two switches those of the single form above.  With c_i the inverse transform of
 * the zero-padded ys_i and np = next_pow2(n), per group
 *   A_g = sum r_i pi_i,   J_g[j] = sum r_i x_i^-j c_i[j] (j < np),   B_g = sum r_i C_i + sum (r_i x_i^np) pi_i - [J_g(s)]_1,
 * and the group passes when e(B_g, [1]G2) e(-A_g, [s^n]G2) == 1: one pairing check, two multi-scalar multiplications over the group's points
 * and one of np terms over the setup per group, where the per-row entry commits to every row's np coefficients.  The combination builds and
 * reads no commitment table.  x_i == 0 follows the reference (InvModFr(0) == 0).  Rows of more than 256 values (np > 256) always take the
 * per-row path.  PRESUPPOSES POINTS OF G1, as CheckProofMulti does; the bound 2^-128 and the warning about known seeds hold as above. */
int kzg_hip_check_proof_multi_batch_combined(kzg_hip_kzg *ks, const void *commitments_g1, const void *proofs_g1, const void *xs_fr, const void *ys_fr, uint64_t n,
                                             uint64_t count, const uint8_t *seed32, uint8_t *ok);
/* eth.VerifyAggregateKZGProof (eth/eth.go:155-172) over `sidecars` blocks.  blob_counts[j] blobs belong to block j (0 is valid); blobs_le32 holds
 * all blobs in block order (sum(blob_counts) x n x 32 little-endian bytes), commitments48 the expected commitments in the same order, proofs48 one
 * aggregated proof per block.  result[j]: 1 valid, 0 the pairing check failed, 2 a field element of one of the block's blobs is >= r ("could not
 * convert blobs to polynomials"), 3 a commitment or the proof of the block is not a valid G1 encoding.  2 wins over 3 (the reference's order).
 * A row with result 2 or 3 affects no other row.  Optional outputs per block (null to skip; unspecified for rows with result 2 or 3): the
 * aggregated commitment as 48 compressed bytes, the evaluation challenge z and y = aggregatedPoly(z) as Fr.
 * Needs kzg_hip_eth_set_setup_g2 (else KZG_HIP_ERR_BAD_ARG); sidecars == 0 is KZG_HIP_OK; KZG_HIP_ERR_TOO_WIDE when the sum of blob_counts
 * overflows.  The blobs are uploaded once per chunk of whole sidecars (KZG_HIP_ETH_VERIFY_CHUNK_MB of blob bytes, default 4096) and everything runs
 * on the device: the Fiat-Shamir transcripts (one lane per sidecar; KZG_HIP_ETH_TRANSCRIPT=host|device forces where they are hashed, the default
 * goes by the sidecar count), the aggregated polynomials and commitments, y and the pairing checks.  No commitment table is built. */
int kzg_hip_eth_verify_aggregate_kzg_proof_batch(kzg_hip_eth *eth, const void *blobs_le32, const uint64_t *blob_counts, const void *commitments48,
                                                 const void *proofs48, uint64_t sidecars, uint8_t *result,
                                                 void *out_agg_commitments48, void *out_zs_fr, void *out_ys_fr);
/* eth.ComputeAggregateKZGProof (eth/eth.go:175-181) over `sidecars` blocks in one call, the prover-side twin of the call above.  blob_counts[j] blobs
 * belong to block j (0 is valid: its proof is the compressed point at infinity); blobs_le32 holds all blobs in block order.  Writes one 48-byte proof per
 * block and, unless out_commitments48 is NULL, the 48-byte commitment of every blob in the same order as the blobs.  status[j] is 0 when block j's
 * outputs are written, else the status kzg_hip_eth_compute_aggregate_kzg_proof returns for that block alone: KZG_HIP_ERR_BAD_BLOB (a field element >= r)
 * or KZG_HIP_ERR_BAD_ARG ("invalid z challenge": the evaluation challenge lies in the domain); such a block gets zero bytes as its proof and as each
 * of its commitments and changes nothing in its neighbours.  Proof and commitments of a block with status 0 are byte for byte those of the lone call.
 * sidecars == 0 is KZG_HIP_OK and touches nothing; NULL blob_counts / out_proofs48 / status (or blobs_le32 with a blob to read) KZG_HIP_ERR_BAD_ARG;
 * KZG_HIP_ERR_TOO_WIDE when the sum of blob_counts or a byte offset overflows.  The work runs per chunk of whole sidecars (KZG_HIP_ETH_PROVE_CHUNK_MB
 * of device memory, default 4096: a block costs twice its blob bytes plus 64 n bytes; a larger block forms a chunk by itself) on a stream of the
 * handle's pool, so concurrent callers are not serialised by the handle's own stream.  The Fiat-Shamir transcripts are hashed on the device from
 * KZG_HIP_ETH_TRANSCRIPT's threshold on (one lane per block, the part that needs no commitment beside the table walk), below it on the calling
 * thread while the device commits; both return identical bytes. */
int kzg_hip_eth_compute_aggregate_kzg_proof_batch(kzg_hip_eth *eth, const void *blobs_le32, const uint64_t *blob_counts, uint64_t sidecars, void *out_proofs48,
                                                  void *out_commitments48, uint8_t *status);
/* The same with the blobs (4-byte aligned), proofs, commitments and status bytes DEVICE-resident: enqueued on the handle's stream, no host
 * synchronisation (but for the first call's table build), transcripts always on the device.  blob_counts stays a HOST array: it sizes the launches. */
int kzg_hip_eth_compute_aggregate_kzg_proof_batch_dev(kzg_hip_eth *eth, const void *d_blobs_le32, const uint64_t *blob_counts, uint64_t sidecars,
                                                      void *d_out_proofs48, void *d_out_commitments48, uint8_t *d_status);
/* ---- the execution-layer side of eth/eth.go in batches: PointEvaluationPrecompile (eth/eth.go:76-110), KZGToVersionedHash (:137-141),
 * VerifyKZGCommitmentsAgainstTransactions with TxPeekBlobVersionedHashes (:234-282) ----
 * One result byte per input row or per block.  0 .. 3 are kzg_hip_eth_verify_kzg_proof_batch's values; the reference's checks run in the order
 * its control flow gives, so a row or block that is wrong in several ways gets the code of the first check it fails. */
typedef enum kzg_hip_eth_code {
    KZG_HIP_ETH_INVALID_PROOF = 0,      /* the pairing check failed: "invalid kzg proof" */
    KZG_HIP_ETH_VALID = 1,
    KZG_HIP_ETH_BAD_FIELD = 2,          /* z or y not below r */
    KZG_HIP_ETH_BAD_G1 = 3,             /* commitment or proof not a valid G1 encoding */
    KZG_HIP_ETH_HASH_MISMATCH = 4,      /* a versioned hash does not match its commitment: "mismatched versioned hash" / "invalid version hashes vs kzg" */
    KZG_HIP_ETH_COUNT_MISMATCH = 5,     /* number of versioned hashes != number of commitments */
    KZG_HIP_ETH_TX_TOO_SHORT = 6,       /* "blob tx invalid: too short"; also a transaction of length 0, where the reference panics on tx[0] */
    KZG_HIP_ETH_TX_OFFSET = 7,          /* "offset to versioned hashes is out of bounds" */
    KZG_HIP_ETH_TX_TRAILING = 8         /* "expected trailing data starting at versioned-hashes offset to be a multiple of 32 bytes" */
} kzg_hip_eth_code;
/* KZGToVersionedHash over `count` commitments of 48 bytes (ANY 48 bytes: the reference hashes before it decodes): out32[i] = SHA-256 of the
 * commitment with byte 0 replaced by BlobCommitmentVersionKZG = 0x01.  One lane per commitment; needs no G2 setup.  count == 0 is KZG_HIP_OK. */
int kzg_hip_eth_kzg_to_versioned_hash_batch(kzg_hip_eth *eth, const void *commitments48, uint64_t count, void *out32);
/* the same on DEVICE buffers (out32 4-byte aligned), enqueued on the handle's stream without a host synchronisation */
int kzg_hip_eth_kzg_to_versioned_hash_batch_dev(kzg_hip_eth *eth, const void *d_commitments48, uint64_t count, void *d_out32);
/* PointEvaluationPrecompile over `count` inputs of 192 bytes (versioned hash 32 | z 32 LE | y 32 LE | commitment 48 | proof 48): result[i] is
 * KZG_HIP_ETH_VALID (the reference returns kzg_hip_eth_precompile_return_value's bytes), KZG_HIP_ETH_INVALID_PROOF, or the first of
 * KZG_HIP_ETH_HASH_MISMATCH, KZG_HIP_ETH_BAD_FIELD, KZG_HIP_ETH_BAD_G1 in that order (eth/eth.go:93-107).  An input of another length
 * ("invalid input length") is the caller's to reject.  The rows are uploaded once; the hash, the parsing and the pairing check run one lane per
 * row and the codes come back in one download.  Needs kzg_hip_eth_set_setup_g2 (else KZG_HIP_ERR_BAD_ARG); count == 0 is KZG_HIP_OK and writes
 * nothing; device memory is linear in count (about 500 bytes per row), the call is not chunked. */
int kzg_hip_eth_point_evaluation_precompile_batch(kzg_hip_eth *eth, const void *inputs192, uint64_t count, uint8_t *result);
/* the same on DEVICE buffers, enqueued on the handle's stream without a host synchronisation.  The queued kernels read the G2 setup that was
 * current when the call was made; kzg_hip_eth_set_setup_g2 may replace it meanwhile.  The handle keeps the replaced setup until an event
 * recorded behind those kernels has completed, and lets it go on the calling thread of the next _dev call, the next kzg_hip_eth_set_setup_g2
 * or kzg_hip_eth_settings_free (which drains the device first), never in a stream callback. */
int kzg_hip_eth_point_evaluation_precompile_batch_dev(kzg_hip_eth *eth, const void *d_inputs192, uint64_t count, uint8_t *d_result);
/* precompileReturnValue (eth/globals.go:70-71): FIELD_ELEMENTS_PER_BLOB (the handle's n) as 32 big-endian bytes, then r as 32 big-endian bytes */
int kzg_hip_eth_precompile_return_value(kzg_hip_eth *eth, void *out64);
/* VerifyKZGCommitmentsAgainstTransactions over `blocks` blocks.  txs holds the serialized transactions of all blocks back to back; transaction t
 * is txs[tx_offsets[t] .. tx_offsets[t + 1]) (one more offset than there are transactions, non-decreasing, else KZG_HIP_ERR_BAD_ARG);
 * tx_counts[j] transactions and commitment_counts[j] of the 48-byte commitments belong to block j, in order.  result[j]: KZG_HIP_ETH_VALID, or
 * the code of the block's FIRST malformed blob transaction (KZG_HIP_ETH_TX_TOO_SHORT / _TX_OFFSET / _TX_TRAILING), else
 * KZG_HIP_ETH_COUNT_MISMATCH, else KZG_HIP_ETH_HASH_MISMATCH: the reference's precedence.  A transaction whose first byte is not 5 is skipped; a
 * block without blob transactions and without commitments is valid; a block changes nothing in its neighbours.  The transactions are peeked
 * on the host (five bytes each are read); the hashes and commitments of the blocks that are well formed go to the device in one upload, one lane
 * hashes and compares each commitment, and the blocks' codes come back in one download.  Needs no G2 setup.  blocks == 0 is KZG_HIP_OK;
 * KZG_HIP_ERR_TOO_WIDE when a sum of counts or a byte offset overflows. */
int kzg_hip_eth_verify_kzg_commitments_against_transactions_batch(kzg_hip_eth *eth, const void *txs, const uint64_t *tx_offsets, const uint64_t *tx_counts,
                                                                  const void *commitments48, const uint64_t *commitment_counts, uint64_t blocks, uint8_t *result);
/* ---- erasure recovery ----
 * FFTSettings.ZeroPolyViaMultiplication (zero_poly.go:116-217): vanishing polynomial of the missing indices of a size-`length`
 * domain; writes `length` evaluations and `length` coefficients (zero-padded).  No missing index -> all zeros (:117-119). */
int kzg_hip_zero_poly_via_multiplication(kzg_hip_fft *fs, const uint64_t *missing_indices, uint64_t n_missing, uint64_t length,
                                         void *out_zero_eval_fr, void *out_zero_poly_fr);
/* FFTSettings.RecoverPolyFromSamples (recover_from_samples.go:42-109) with ZeroPolyViaMultiplication as the zero-poly function:
 * n samples, present[i] == 0 <=> samples[i] == nil; writes the n reconstructed values.  KZG_HIP_ERR_RECOVERY when a known
 * sample is not reproduced (the reference's error). */
int kzg_hip_recover_poly_from_samples(kzg_hip_fft *fs, const void *samples_fr, const uint8_t *present, uint64_t n, void *out_fr);
/* Many rows per call: `batch` rows of n samples, every stage one launch over the rows of a chunk (KZG_HIP_RECOVER_CHUNK_MB).
 * present_rows == 1: one mask shared by every row (whole columns lost), present_rows == batch: a mask per row.  status[row]: KZG_HIP_OK,
 * KZG_HIP_ERR_RECOVERY or KZG_HIP_ERR_BAD_ARG (a row with nothing present); a failed row's output is zero-filled, a row with nothing missing is
 * copied through.  Status and bytes of a row are what kzg_hip_recover_poly_from_samples returns for that row alone.  n not a power of two or wider
 * than the settings, null pointers and any other present_rows fail the whole call; batch == 0 is KZG_HIP_OK. */
int kzg_hip_recover_poly_from_samples_batch(kzg_hip_fft *fs, const void *samples_fr, const uint8_t *present, uint64_t present_rows, uint64_t n,
                                            uint64_t batch, void *out_fr, uint8_t *status);
/* The same on device-resident rows, ordered on `stream`: erasure lists, counts and statuses are derived on the device, the call never waits for it. */
int kzg_hip_recover_poly_from_samples_batch_dev(kzg_hip_fft *fs, const void *d_samples_fr, const uint8_t *d_present, uint64_t present_rows, uint64_t n,
                                                uint64_t batch, void *d_out_fr, uint8_t *d_status, void *stream);
/* Vanishing polynomials of `batch` ragged erasure sets: row b's indices are missing_indices[offsets[b] .. offsets[b + 1]); rows of `length`
 * evaluations and coefficients.  status[b]: KZG_HIP_OK (no index: all zeros) or KZG_HIP_ERR_BAD_ARG (as many indices as `length` or more, or an
 * index >= length: that row is zero-filled, its neighbours are computed). */
int kzg_hip_zero_poly_via_multiplication_batch(kzg_hip_fft *fs, const uint64_t *missing_indices, const uint64_t *offsets, uint64_t batch,
                                               uint64_t length, void *out_zero_eval_fr, void *out_zero_poly_fr, uint8_t *status);

/* ---- several GPUs behind ONE handle (SURVEY.md 8b threading row: "multi-GPU handle owns one context per device"; 8e) ----
 * The reference is a single-process library (kzg.go:11-19): a drop-in that uses every GPU of a node does so inside this library.
 * kzg_hip_multi_settings_new builds an FFTSettings (NewFFTSettings(max_scale), fft.go:44) and a KZGSettings (NewKZGSettings, kzg.go:21-36)
 * with their tables on EVERY listed device.  A list may repeat a device (each entry gets its own settings and tables: how a 1-GPU box
 * exercises the multi-device code paths).
 *   _batch calls: the polynomials are divided into contiguous shares, one per device, results land in the caller's buffer in input order;
 *     no data-path collective (blobs are independent).
 *   kzg_hip_multi_da_using_fk20 / _da_using_fk20_multi: ONE polynomial over all devices (fk20_multi.go:58-109, kzg.go:73-116): the Toeplitz
 *     stage is sharded by output position, the hExtFFT slices are ALL-GATHERED, then either the first device runs the two G1 transforms
 *     ("gather") or both transforms are sharded by decimation with two more all-gathers each, the last one of the proof points ("sharded":
 *     the five all-gathers of SURVEY.md 8e; default from 4 devices on, kzg_hip_multi_set_fft_sharding / KZG_HIP_MULTI_FFT=gather|sharded).
 * Exchange transport (kzg_hip_multi_transport): "rccl" = ncclAllGather on ncclUint8 over single-process communicators (ncclCommInitAll;
 * RCCL over xGMI), used when every listed device is distinct; "peer-copy" = hipMemcpyPeerAsync between the devices' streams, used when the
 * list repeats a device or librccl cannot be bound; "host-staged" = device -> pinned host -> device, the last resort
 * (kzg_hip_multi_transport_note says why a transport was not used).  Every buffer another device reads or writes is hipMalloc memory of a
 * per-entry exchange arena (never the stream-ordered pool), peer access is enabled between all listed devices, and the constructor PROVES
 * the transport before returning: every entry writes a pattern, one all-gather, every entry verifies every byte
 * (kzg_hip_multi_transport_check); a transport that errs or delivers wrong bytes is replaced by the next one in the order above, and the
 * constructor fails with KZG_HIP_ERR_HIP only if none delivers.  Results are identical whatever the transport and identical to the
 * single-device calls (tests/test_multi_device.py). */
typedef struct kzg_hip_multi kzg_hip_multi;
typedef struct kzg_hip_multi_fk20s kzg_hip_multi_fk20s;
typedef struct kzg_hip_multi_fk20m kzg_hip_multi_fk20m;
int kzg_hip_multi_settings_new(const int *devices, uint32_t n_devices, unsigned max_scale, const void *secret_g1, uint64_t n_setup, kzg_hip_multi **out);
void kzg_hip_multi_settings_free(kzg_hip_multi *m);
uint32_t kzg_hip_multi_device_count(const kzg_hip_multi *m);
int kzg_hip_multi_device(const kzg_hip_multi *m, uint32_t i);          /* device ordinal of entry i (-1 out of range) */
kzg_hip_fft *kzg_hip_multi_fft(kzg_hip_multi *m, uint32_t i);          /* entry i's settings, BORROWED (owned by the multi handle): */
kzg_hip_kzg *kzg_hip_multi_kzg(kzg_hip_multi *m, uint32_t i);          /* any single-device call can be made on a chosen device     */
const char *kzg_hip_multi_transport(const kzg_hip_multi *m);           /* "rccl", "peer-copy" or "host-staged" */
const char *kzg_hip_multi_transport_note(const kzg_hip_multi *m);      /* why the transport is not "rccl" ("" otherwise) */
const char *kzg_hip_multi_transport_check(const kzg_hip_multi *m); /* outcome of the creation-time exchange test: "ok: <transport>, ..." */
uint64_t kzg_hip_multi_exchanges(const kzg_hip_multi *m);              /* all-gathers performed on this handle so far */
int kzg_hip_multi_set_fft_sharding(kzg_hip_multi *m, int mode);        /* 0 gather, 1 sharded transforms, -1 default policy */
int kzg_hip_multi_set_table_budget_gb(kzg_hip_multi *m, double gb);    /* kzg_hip_kzg_set_table_budget_gb on every entry */
/* CommitToPoly / ComputeProofSingle on `batch` polynomials (kzg_single_proofs.go:17-19,36-54), sharded by polynomial */
int kzg_hip_multi_commit_to_poly_batch(kzg_hip_multi *m, const void *coeffs_fr, uint64_t n, uint64_t batch, void *out_g1);
int kzg_hip_multi_compute_proof_single_batch(kzg_hip_multi *m, const void *poly_fr, uint64_t n, uint64_t batch, const uint64_t *xs, void *out_g1);
/* FFT / InplaceFFT (fft_fr.go:55-105) and DASFFTExtension (das_extension.go:71-84; in place) on `batch` rows of n values, rows divided among the devices */
int kzg_hip_multi_fft_fr_batch(kzg_hip_multi *m, const void *vals_fr, uint64_t n, uint64_t batch, int inv, void *out_fr);
int kzg_hip_multi_das_fft_extension_batch(kzg_hip_multi *m, void *vals_fr, uint64_t n, uint64_t batch);
int kzg_hip_multi_fft_g1_batch(kzg_hip_multi *m, const void *vals_g1, uint64_t n, uint64_t batch, int inv, void *out_g1);   /* FFTG1 (fft_g1.go:58-94) likewise */
/* package eth on every entry (eth/globals.go:39-72; lagrange_g1 in natural order as for kzg_hip_eth_settings_new): BlobToKZGCommitment (eth/eth.go:145-151)
 * and ComputeKZGProof (eth/helpers.go:179-203) on batches, rows divided among the devices; flags and error codes as in the single-device calls */
typedef struct kzg_hip_multi_eth kzg_hip_multi_eth;
int kzg_hip_multi_eth_settings_new(kzg_hip_multi *m, const void *lagrange_g1, uint64_t n, kzg_hip_multi_eth **out);
void kzg_hip_multi_eth_settings_free(kzg_hip_multi_eth *eth);
int kzg_hip_multi_eth_blob_to_kzg_commitment_batch(kzg_hip_multi_eth *eth, const void *blobs_le32, uint64_t batch, void *out48, uint8_t *ok);
int kzg_hip_multi_eth_compute_kzg_proof_batch(kzg_hip_multi_eth *eth, const void *polys_fr, uint64_t n, uint64_t batch, const void *zs_fr, void *out48, void *ys_fr, uint8_t *ok);
/* NewFK20SingleSettings on every entry (kzg.go:43-64); DAUsingFK20 on a batch (sharded by polynomial) and on ONE polynomial (sharded inside) */
int kzg_hip_multi_fk20_single_settings_new(kzg_hip_multi *m, uint64_t n2, kzg_hip_multi_fk20s **out);
void kzg_hip_multi_fk20_single_settings_free(kzg_hip_multi_fk20s *fk);
int kzg_hip_multi_da_using_fk20_batch(kzg_hip_multi_fk20s *fk, const void *poly_fr, uint64_t n, uint64_t batch, void *out_g1);
int kzg_hip_multi_da_using_fk20(kzg_hip_multi_fk20s *fk, const void *poly_fr, uint64_t n, void *out_g1 /* 2n */);
/* NewFK20MultiSettings on every entry (kzg.go:73-116); DAUsingFK20Multi likewise */
int kzg_hip_multi_fk20_multi_settings_new(kzg_hip_multi *m, uint64_t n2, uint64_t chunk_len, kzg_hip_multi_fk20m **out);
void kzg_hip_multi_fk20_multi_settings_free(kzg_hip_multi_fk20m *fk);
int kzg_hip_multi_da_using_fk20_multi_batch(kzg_hip_multi_fk20m *fk, const void *poly_fr, uint64_t n, uint64_t batch, void *out_g1);
int kzg_hip_multi_da_using_fk20_multi(kzg_hip_multi_fk20m *fk, const void *poly_fr, uint64_t n, void *out_g1 /* 2n / chunk_len */);

/* shape of the fixed-base table CommitToPoly walks (built lazily by the first commitment): signed window bits c, window count and
 * bytes of HBM; all zero before the first commitment or when the setup is too small for a table (classic bucket path).  Both GLV halves of a
 * scalar (k = k1 + k2 lambda, |k1|, |k2| < 2^127) walk the same rows, so `windows` = ceil(128 / c) and a coefficient costs 2 x windows mixed
 * additions (kzg_hip_kzg_table_additions): 4096 points at c = 16 are 8 windows = 103 GB, the default budget (110 GB; kzg_hip_kzg_set_table_budget_gb).
 * Batches of 2048 rows and more (kzg_hip_commit_to_poly_batch, _dev) walk a second, shared-window table d P_i paid from the same budget (one accumulator per window, joined
 * per blob: 19-bit digits, 7 windows, 14 additions from the same 103 GB); where the budget cannot hold both and the shared table needs fewer additions it replaces the
 * all-window table, and later small calls get the all-window table the remainder affords.  These two calls describe the all-window table while one exists, otherwise the
 * shared one: window bits, windows per GLV half, bytes; 2 x windows additions.  Where the budget holds the paired-point form of that table with 10-bit digits and
 * it needs fewer additions than single-point digits from the same bytes (the default budget: entries d0 P_2g + d1 P_2g+1, 13 windows, 103 280 541 696 bytes), large
 * batches walk that one instead: one gathered entry serves a digit of two neighbouring coefficients, so the calls report (10, 13, bytes) and `windows` additions, 13.
 * KZG_HIP_FB_LAYOUT=windows keeps every batch on the all-window table. */
int kzg_hip_kzg_table_info(kzg_hip_kzg *ks, uint32_t *window_bits, uint32_t *windows, uint64_t *table_bytes);
uint32_t kzg_hip_kzg_table_additions(kzg_hip_kzg *ks);
/* Projective outputs (off by default).  The reference's G1Point is a Jacobian triple and CommitToPoly / ComputeProofSingle return it with whatever Z the
 * additions left (kzg_single_proofs.go:17-19,36-54; bls/bls_kilic.go:30-35); this library normalises every result to Z = one, one F_p inversion per result:
 * ~0.11 ms of latency, a third of a lone CommitToPoly.  on != 0: CommitToPoly / ComputeProofSingle on this settings object (single, batch, _dev forms) return the
 * same group element as an un-normalised Jacobian image (Z != one; infinity stays (0, 1, 0)); callers compare with bls.EqualG1 / compress as they would the reference's. */
int kzg_hip_kzg_set_projective_outputs(kzg_hip_kzg *ks, int on);

#pragma GCC visibility pop
#ifdef __cplusplus
}
#endif
#endif
