// k_eth_exec.hip -- kernels of the execution-layer side of eth/eth.go in batches (capi_eth_exec.hip): KZGToVersionedHash (eth/eth.go:137-141),
// the parsing of PointEvaluationPrecompile inputs (eth/eth.go:76-110) in front of the pairing check of k_pairing.hip, and the hash comparison
// of VerifyKZGCommitmentsAgainstTransactions (eth/eth.go:272-281).  One lane per commitment, per input row or per block.  The lane bodies
// are in eth_exec.hpp (host/device; tests/host/eth_exec_emul.cpp runs them on the CPU).
#include "internal.hpp"
#include "eth_exec.hpp"

namespace kzg {

constexpr uint32_t HASH_BLOCK = 256;
// the input kernel of the precompile has the shape of k_eth_check_inputs (k_pairing.hip: PAIRING_BLOCK lanes, one wavefront per workgroup):
// it is that kernel behind one SHA-256 block
constexpr uint32_t EXEC_INPUTS_BLOCK = 64;
static inline dim3 grid_for(uint64_t n, uint32_t block) { return dim3((uint32_t)((n + block - 1) / block)); }

// out32[t] = KZGToVersionedHash(c48[t]); out32 is 4-byte aligned (eight word stores per lane)
__global__ __launch_bounds__(HASH_BLOCK) void k_eth_versioned_hashes(const uint8_t *c48, uint64_t n, uint32_t *out32) {
    const uint64_t t = blockIdx.x * (uint64_t)blockDim.x + threadIdx.x;
    if (t >= n) return;
    uint32_t h[8];
    kzg_to_versioned_hash_lane(c48 + 48 * t, h);
#pragma unroll
    for (int i = 0; i < 8; i++) out32[8 * t + i] = sha_bswap32(h[i]);
}
void launch_eth_versioned_hashes(hipStream_t s, const uint8_t *c48, uint64_t n, uint8_t *out32) {
    if (!n) return;
    hipLaunchKernelGGL(k_eth_versioned_hashes, grid_for(n, HASH_BLOCK), dim3(HASH_BLOCK), 0, s, c48, n, (uint32_t *)out32);
}

// eth_precompile_inputs_lane over rows of 192 bytes: status 0 = inputs valid, 4 = the versioned hash does not match the commitment, 2 = z or y
// not below r, 3 = commitment or proof not a valid compressed G1 point.  Invalid rows get points at infinity.
__global__ __launch_bounds__(EXEC_INPUTS_BLOCK) void k_eth_precompile_inputs(const uint8_t *in192, uint64_t n, g1j *p0, g1j *p1, uint8_t *status) {
    const uint64_t t = blockIdx.x * (uint64_t)blockDim.x + threadIdx.x;
    if (t >= n) return;
    eth_precompile_inputs_lane(in192 + 192 * t, p0[t], p1[t], status[t]);
}
void launch_eth_precompile_inputs(hipStream_t s, const uint8_t *in192, uint64_t n, g1j *p0, g1j *p1, uint8_t *status) {
    if (!n) return;
    hipLaunchKernelGGL(k_eth_precompile_inputs, grid_for(n, EXEC_INPUTS_BLOCK), dim3(EXEC_INPUTS_BLOCK), 0, s, in192, n, p0, p1, status);
}

// result[t] = status[t] where it is not 0, else ok[t] (the pairing check's 1 / 0); result may be ok
__global__ __launch_bounds__(HASH_BLOCK) void k_eth_merge_status(const uint8_t *status, const uint8_t *ok, uint64_t n, uint8_t *result) {
    const uint64_t t = blockIdx.x * (uint64_t)blockDim.x + threadIdx.x;
    if (t >= n) return;
    const uint8_t st = status[t];
    result[t] = st ? st : ok[t];
}
void launch_eth_merge_status(hipStream_t s, const uint8_t *status, const uint8_t *ok, uint64_t n, uint8_t *result) {
    if (!n) return;
    hipLaunchKernelGGL(k_eth_merge_status, grid_for(n, HASH_BLOCK), dim3(HASH_BLOCK), 0, s, status, ok, n, result);
}

// match[t] = (KZGToVersionedHash(c48[t]) == want32[t]): the commitments and the hashes gathered from the transactions, index for index
__global__ __launch_bounds__(HASH_BLOCK) void k_eth_tx_hashes_match(const uint8_t *c48, const uint8_t *want32, uint64_t n, uint8_t *match) {
    const uint64_t t = blockIdx.x * (uint64_t)blockDim.x + threadIdx.x;
    if (t >= n) return;
    uint32_t h[8];
    kzg_to_versioned_hash_lane(c48 + 48 * t, h);
    match[t] = versioned_hash_equals(h, want32 + 32 * t) ? 1 : 0;
}
// one lane per block: result[j] = 1 when every flag of off[j] .. off[j + 1] is set (none: valid), else 4
__global__ __launch_bounds__(HASH_BLOCK) void k_eth_tx_fold(const uint8_t *match, const uint64_t *off, uint64_t blocks, uint8_t *result) {
    const uint64_t j = blockIdx.x * (uint64_t)blockDim.x + threadIdx.x;
    if (j >= blocks) return;
    uint32_t all = 1;
    for (uint64_t k = off[j]; k < off[j + 1]; k++) all &= match[k];
    result[j] = all ? 1 : ETH_CODE_HASH_MISMATCH;
}
void launch_eth_tx_hashes_check(hipStream_t s, const uint8_t *c48, const uint8_t *want32, const uint64_t *off, uint64_t total, uint64_t blocks, uint8_t *match,
                                uint8_t *result) {
    if (total) hipLaunchKernelGGL(k_eth_tx_hashes_match, grid_for(total, HASH_BLOCK), dim3(HASH_BLOCK), 0, s, c48, want32, total, match);
    if (blocks) hipLaunchKernelGGL(k_eth_tx_fold, grid_for(blocks, HASH_BLOCK), dim3(HASH_BLOCK), 0, s, match, off, blocks, result);
}

}  // namespace kzg
