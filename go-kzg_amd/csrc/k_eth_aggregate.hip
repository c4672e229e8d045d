// k_eth_aggregate.hip -- kernels of the batched block verifier (eth.VerifyAggregateKZGProof over many sidecars, capi_verify.hip): the
// Fiat-Shamir transcripts, the aggregated polynomials and the aggregated commitments of a chunk of sidecars, all from the raw bytes where
// they lie in HBM.  off[j] .. off[j + 1] are the blobs (and commitments) of sidecar j within the chunk.  The lane bodies are in
// eth_aggregate.hpp / sha256_lane.hpp (host/device; tests/host/aggregate_emul.cpp runs them on the CPU).
#include "internal.hpp"
#include "eth_aggregate.hpp"

namespace kzg {

constexpr uint32_t AGG_BLOCK = 256;
// one lane per chain and the chains of a wavefront in lockstep: a wavefront per workgroup spreads few sidecars over as many CUs as there are
constexpr uint32_t TRANSCRIPT_BLOCK = 64;
static inline dim3 grid_for(uint64_t n, uint32_t block) { return dim3((uint32_t)((n + block - 1) / block)); }

// one lane per sidecar: hashPolysComms over the block's bytes, then the two challenges.  The chains of a wavefront have different lengths:
// the block loop ends per lane.
__global__ __launch_bounds__(TRANSCRIPT_BLOCK) void k_eth_transcripts(const uint8_t *blobs, const uint8_t *comms, const uint64_t *off, uint64_t n, uint64_t sidecars,
                                                                      fr *r_out, fr *z_out) {
    const uint64_t j = blockIdx.x * (uint64_t)blockDim.x + threadIdx.x;
    if (j >= sidecars) return;
    const uint64_t o = off[j], count = off[j + 1] - o;
    fr r, z;
    eth_transcript_lane(blobs + o * n * 32, comms + o * 48, n, count, r, z);
    r_out[j] = r; z_out[j] = z;
}
void launch_eth_transcripts(hipStream_t s, const uint8_t *blobs, const uint8_t *comms, const uint64_t *off, uint64_t n, uint64_t sidecars, fr *r_out, fr *z_out) {
    if (!sidecars) return;
    prof_begin(s, "eth_transcripts");
    hipLaunchKernelGGL(k_eth_transcripts, grid_for(sidecars, TRANSCRIPT_BLOCK), dim3(TRANSCRIPT_BLOCK), 0, s, blobs, comms, off, n, sidecars, r_out, z_out);
    prof_end(s, "eth_transcripts");
}

// The chain in two halves, for the batched block PROVER (capi_eth_prove.hip): its commitments are computed on the device from the same
// blobs, so all of a chain but its last 48 count + 32 bytes is hashed beside the table walk.  One lane per sidecar as above; st is eight
// words per sidecar.
__global__ __launch_bounds__(TRANSCRIPT_BLOCK) void k_eth_transcript_blobs(const uint8_t *blobs, const uint64_t *off, uint64_t n, uint64_t sidecars, uint32_t *st) {
    const uint64_t j = blockIdx.x * (uint64_t)blockDim.x + threadIdx.x;
    if (j >= sidecars) return;
    const uint64_t o = off[j], count = off[j + 1] - o;
    uint32_t s[8];
    eth_transcript_blobs_lane(blobs + o * n * 32, n, count, s);
#pragma unroll
    for (int i = 0; i < 8; i++) st[8 * j + i] = s[i];
}
void launch_eth_transcript_blobs(hipStream_t s, const uint8_t *blobs, const uint64_t *off, uint64_t n, uint64_t sidecars, uint32_t *st) {
    if (!sidecars) return;
    prof_begin(s, "eth_transcript_blobs");
    hipLaunchKernelGGL(k_eth_transcript_blobs, grid_for(sidecars, TRANSCRIPT_BLOCK), dim3(TRANSCRIPT_BLOCK), 0, s, blobs, off, n, sidecars, st);
    prof_end(s, "eth_transcript_blobs");
}
__global__ __launch_bounds__(TRANSCRIPT_BLOCK) void k_eth_transcript_finish(const uint8_t *blobs, const uint8_t *comms, const uint64_t *off, uint64_t n, uint64_t sidecars,
                                                                            const uint32_t *st, fr *r_out, fr *z_out) {
    const uint64_t j = blockIdx.x * (uint64_t)blockDim.x + threadIdx.x;
    if (j >= sidecars) return;
    const uint64_t o = off[j], count = off[j + 1] - o;
    uint32_t s[8];
#pragma unroll
    for (int i = 0; i < 8; i++) s[i] = st[8 * j + i];
    fr r, z;
    eth_transcript_finish_lane(blobs + o * n * 32, comms + o * 48, n, count, s, r, z);
    r_out[j] = r; z_out[j] = z;
}
void launch_eth_transcript_finish(hipStream_t s, const uint8_t *blobs, const uint8_t *comms, const uint64_t *off, uint64_t n, uint64_t sidecars, const uint32_t *st,
                                  fr *r_out, fr *z_out) {
    if (!sidecars) return;
    prof_begin(s, "eth_transcript_finish");
    hipLaunchKernelGGL(k_eth_transcript_finish, grid_for(sidecars, TRANSCRIPT_BLOCK), dim3(TRANSCRIPT_BLOCK), 0, s, blobs, comms, off, n, sidecars, st, r_out, z_out);
    prof_end(s, "eth_transcript_finish");
}
// the prover's last step, one lane per sidecar: the row's status byte -- code_blob where k_eth_agg_poly found an element >= r (it wins, the
// lone call's order), code_z where the evaluation challenge lies in the domain, else 0 -- and zero bytes over the proof and the commitments
// of a failed row (byte stores: a caller's buffers may have any alignment; failed rows are rare).  comms48 may be null.
__global__ __launch_bounds__(AGG_BLOCK) void k_eth_prove_finish(const uint8_t *agg_status, const uint32_t *z_in_domain, const uint64_t *off, uint64_t sidecars,
                                                                uint8_t code_blob, uint8_t code_z, uint8_t *proofs48, uint8_t *comms48, uint8_t *status) {
    const uint64_t j = blockIdx.x * (uint64_t)blockDim.x + threadIdx.x;
    if (j >= sidecars) return;
    const uint8_t code = agg_status[j] ? code_blob : z_in_domain[j] ? code_z : 0;
    status[j] = code;
    if (!code) return;
    for (uint32_t i = 0; i < 48; i++) proofs48[48 * j + i] = 0;
    if (comms48) for (uint64_t i = 48 * off[j]; i < 48 * off[j + 1]; i++) comms48[i] = 0;
}
void launch_eth_prove_finish(hipStream_t s, const uint8_t *agg_status, const uint32_t *z_in_domain, const uint64_t *off, uint64_t sidecars, uint8_t code_blob,
                             uint8_t code_z, uint8_t *proofs48, uint8_t *comms48, uint8_t *status) {
    if (!sidecars) return;
    hipLaunchKernelGGL(k_eth_prove_finish, grid_for(sidecars, AGG_BLOCK), dim3(AGG_BLOCK), 0, s, agg_status, z_in_domain, off, sidecars, code_blob, code_z, proofs48, comms48,
                       status);
}

// lane (sidecar j, coefficient i): the aggregated polynomial's coefficient from the blobs' bytes; an element >= r marks the SIDECAR (status 2,
// the same byte from every lane that finds one)
__global__ __launch_bounds__(AGG_BLOCK) void k_eth_agg_poly(const uint8_t *blobs, const uint64_t *off, const fr *r, uint64_t n, uint64_t sidecars, fr *agg, uint8_t *status) {
    const uint64_t t = blockIdx.x * (uint64_t)blockDim.x + threadIdx.x;
    if (t >= sidecars * n) return;
    const uint64_t j = t / n, i = t % n, o = off[j];
    fr out;
    if (!eth_agg_poly_lane(blobs + o * n * 32, n, off[j + 1] - o, i, r[j], out)) status[j] = 2;
    agg[t] = out;
}
void launch_eth_agg_poly(hipStream_t s, const uint8_t *blobs, const uint64_t *off, const fr *r, uint64_t n, uint64_t sidecars, fr *agg, uint8_t *status) {
    if (!sidecars) return;
    prof_begin(s, "eth_agg_poly");
    hipLaunchKernelGGL(k_eth_agg_poly, grid_for(sidecars * n, AGG_BLOCK), dim3(AGG_BLOCK), 0, s, blobs, off, r, n, sidecars, agg, status);
    prof_end(s, "eth_agg_poly");
}

// ComputePowers per sidecar (eth/helpers.go:87-96): pow[off[j] + k] = r_j^k
__global__ __launch_bounds__(AGG_BLOCK) void k_eth_powers(const fr *r, const uint64_t *off, uint64_t sidecars, fr *pow) {
    const uint64_t j = blockIdx.x * (uint64_t)blockDim.x + threadIdx.x;
    if (j >= sidecars) return;
    const fr rj = r[j];
    fr cur = one<FrP>();
    for (uint64_t k = off[j]; k < off[j + 1]; k++) { pow[k] = cur; cur = mul(cur, rj); }
}
void launch_eth_powers(hipStream_t s, const fr *r, const uint64_t *off, uint64_t sidecars, fr *pow) {
    if (!sidecars) return;
    hipLaunchKernelGGL(k_eth_powers, grid_for(sidecars, AGG_BLOCK), dim3(AGG_BLOCK), 0, s, r, off, sidecars, pow);
}

// bls.FromCompressedG1 with one status per row (0 valid, 1 not a valid encoding; the point is then inf) instead of one flag for the launch
__global__ __launch_bounds__(AGG_BLOCK, 2) void k_g1_decompress_rows(const uint8_t *in48, g1j *out, uint64_t n, uint8_t *bad, bool to_kilic) {
    const uint64_t t = blockIdx.x * (uint64_t)blockDim.x + threadIdx.x;
    if (t >= n) return;
    g1j o;
    bad[t] = g1_decompress(o, in48 + 48 * t) ? 0 : 1;
    out[t] = to_kilic ? g1_to_kilic(o) : o;
}
void launch_g1_decompress_rows(hipStream_t s, const uint8_t *in48, g1j *out, uint64_t n, uint8_t *bad, bool to_kilic) {
    if (!n) return;
    hipLaunchKernelGGL(k_g1_decompress_rows, grid_for(n, AGG_BLOCK), dim3(AGG_BLOCK), 0, s, in48, out, n, bad, to_kilic);
}

// segmented sum: one lane per sidecar adds the block's scaled commitments (none: inf).  out: device-internal images (the compression wants
// those), out_kilic: Kilic images (the check inputs want those).  A commitment that did not decode marks the sidecar 3 unless it is already 2.
__global__ __launch_bounds__(AGG_BLOCK, 2) void k_g1_segment_sum(const g1j *pts, const uint8_t *pt_bad, const uint64_t *off, uint64_t sidecars, g1j *out, g1j *out_kilic,
                                                                 uint8_t *status) {
    const uint64_t j = blockIdx.x * (uint64_t)blockDim.x + threadIdx.x;
    if (j >= sidecars) return;
    g1j acc = g1_inf();
    uint32_t bad = 0;
    for (uint64_t k = off[j]; k < off[j + 1]; k++) { acc = g1_add(acc, pts[k]); bad |= pt_bad[k]; }
    if (bad && status[j] == 0) status[j] = 3;
    out[j] = acc;
    out_kilic[j] = g1_to_kilic(acc);
}
void launch_g1_segment_sum(hipStream_t s, const g1j *pts, const uint8_t *pt_bad, const uint64_t *off, uint64_t sidecars, g1j *out, g1j *out_kilic, uint8_t *status) {
    if (!sidecars) return;
    hipLaunchKernelGGL(k_g1_segment_sum, grid_for(sidecars, AGG_BLOCK), dim3(AGG_BLOCK), 0, s, pts, pt_bad, off, sidecars, out, out_kilic, status);
}

// per sidecar, before the check: y = 0 where z lies in the domain (the reference's formula, bls/globals.go:141-152), and an undecodable proof
// marks the sidecar 3 unless it already has a status
__global__ __launch_bounds__(AGG_BLOCK) void k_eth_agg_finish(const uint32_t *z_in_domain, const uint8_t *proof_bad, uint64_t sidecars, fr *y, uint8_t *status) {
    const uint64_t j = blockIdx.x * (uint64_t)blockDim.x + threadIdx.x;
    if (j >= sidecars) return;
    if (z_in_domain[j]) y[j] = zero<FrP>();
    if (proof_bad[j] && status[j] == 0) status[j] = 3;
}
void launch_eth_agg_finish(hipStream_t s, const uint32_t *z_in_domain, const uint8_t *proof_bad, uint64_t sidecars, fr *y, uint8_t *status) {
    if (!sidecars) return;
    hipLaunchKernelGGL(k_eth_agg_finish, grid_for(sidecars, AGG_BLOCK), dim3(AGG_BLOCK), 0, s, z_in_domain, proof_bad, sidecars, y, status);
}

// test hooks: one message / one digest per lane through the transcript's own hash and reduction
__global__ __launch_bounds__(TRANSCRIPT_BLOCK) void k_test_sha256_lanes(const uint8_t *data, const uint64_t *offsets, const uint64_t *lens, uint64_t rows, uint32_t *out) {
    const uint64_t t = blockIdx.x * (uint64_t)blockDim.x + threadIdx.x;
    if (t >= rows) return;
    uint32_t st[8];
    sha256_lane(sha_bytes_src{data + offsets[t]}, lens[t], st);
    for (int i = 0; i < 8; i++) out[8 * t + i] = sha_bswap32(st[i]);
}
void launch_test_sha256_lanes(hipStream_t s, const uint8_t *data, const uint64_t *offsets, const uint64_t *lens, uint64_t rows, uint32_t *out) {
    if (!rows) return;
    hipLaunchKernelGGL(k_test_sha256_lanes, grid_for(rows, TRANSCRIPT_BLOCK), dim3(TRANSCRIPT_BLOCK), 0, s, data, offsets, lens, rows, out);
}
__global__ __launch_bounds__(TRANSCRIPT_BLOCK) void k_test_hash_to_bls_field_lanes(const uint8_t *digests, uint64_t rows, fr *out) {
    const uint64_t t = blockIdx.x * (uint64_t)blockDim.x + threadIdx.x;
    if (t >= rows) return;
    out[t] = fr_from_digest_bytes(digests + 32 * t);
}
void launch_test_hash_to_bls_field_lanes(hipStream_t s, const uint8_t *digests, uint64_t rows, fr *out) {
    if (!rows) return;
    hipLaunchKernelGGL(k_test_hash_to_bls_field_lanes, grid_for(rows, TRANSCRIPT_BLOCK), dim3(TRANSCRIPT_BLOCK), 0, s, digests, rows, out);
}

}  // namespace kzg
