// eth_exec.hpp -- the execution-layer side of eth/eth.go as ONE LANE runs it, as host/device functions: KZGToVersionedHash (eth/eth.go:137-141)
// and the parsing of a PointEvaluationPrecompile input (eth/eth.go:76-110) in front of eth_check_inputs_lane (verify_inputs.hpp).  The kernels
// (k_eth_exec.hip) keep the index arithmetic, the loads and the stores; tests/host/eth_exec_emul.cpp runs these bodies on the CPU.
#pragma once
#include "verify_inputs.hpp"
#include "sha256_lane.hpp"

namespace kzg {

// result codes of the batched execution-layer calls beyond eth.VerifyKZGProof's 0 .. 3 (KZG_HIP_ETH_* in include/kzg_hip.h)
constexpr uint8_t ETH_CODE_HASH_MISMATCH = 4;
constexpr uint8_t BLOB_COMMITMENT_VERSION_KZG = 0x01;   // eth/eth.go: BlobCommitmentVersionKZG

// KZGToVersionedHash: SHA-256 of the 48 bytes (any 48 bytes: the reference hashes before it decodes) with the first digest byte replaced by
// the version.  48 bytes fit one block -- 12 message words, 0x80, zeros, the length 384 in bits -- so this is one sha256_compress.
// h: the versioned hash as eight big-endian words (hash byte 4 i + k = bits 24 - 8 k .. of h[i]).
KZG_HD void kzg_to_versioned_hash_lane(const uint8_t *c48, uint32_t h[8]) {
    uint32_t w[16];
#pragma unroll
    for (int j = 0; j < 12; j++) w[j] = (uint32_t)c48[4 * j] << 24 | (uint32_t)c48[4 * j + 1] << 16 | (uint32_t)c48[4 * j + 2] << 8 | c48[4 * j + 3];
    w[12] = 0x80000000u; w[13] = 0; w[14] = 0; w[15] = 384;
    sha256_init(h);
    sha256_compress(h, w);
    h[0] = (h[0] & 0x00ffffffu) | (uint32_t)BLOB_COMMITMENT_VERSION_KZG << 24;
}
// whether the 32 bytes at `want` are the versioned hash h
KZG_HD bool versioned_hash_equals(const uint32_t h[8], const uint8_t *want) {
    uint32_t diff = 0;
#pragma unroll
    for (int i = 0; i < 8; i++) diff |= h[i] ^ ((uint32_t)want[4 * i] << 24 | (uint32_t)want[4 * i + 1] << 16 | (uint32_t)want[4 * i + 2] << 8 | want[4 * i + 3]);
    return diff == 0;
}

// One PointEvaluationPrecompile input of 192 bytes: versioned hash [0, 32), z [32, 64), y [64, 96) (little-endian, bytesToBLSField =
// bls.FrFrom32), commitment [96, 144), proof [144, 192).  The reference's order (eth/eth.go:93-107): the hash first (status 4), then
// eth.VerifyKZGProof's own checks unchanged (2, then 3).  status 0: inputs valid.  A row with a non-zero status gets points at infinity.
// The hash runs before any G1 work and its words are dead by then.
KZG_HD void eth_precompile_inputs_lane(const uint8_t *in192, g1j &p0, g1j &p1, uint8_t &status) {
    uint32_t h[8];
    kzg_to_versioned_hash_lane(in192 + 96, h);
    if (!versioned_hash_equals(h, in192)) { p0 = g1_inf(); p1 = g1_inf(); status = ETH_CODE_HASH_MISMATCH; return; }
    eth_check_inputs_lane(in192 + 96, in192 + 32, in192 + 64, in192 + 144, p0, p1, status);
}

}  // namespace kzg
