// eth_tx.hpp -- TxPeekBlobVersionedHashes (eth/eth.go:234-256) as VerifyKZGCommitmentsAgainstTransactions calls it (eth/eth.go:261-271), on the
// host: where in a serialized transaction its blob versioned hashes lie.  Host only (capi_eth_exec.hip; tests/host/eth_exec_emul.cpp runs it
// under sanitizers).  It reads five bytes of a transaction: the type byte and the four bytes of the offset field.
#pragma once
#include <stdint.h>

namespace kzg {

constexpr uint8_t BLOB_TX_TYPE = 5;                       // eth/eth.go:66
constexpr uint64_t BLOB_VERSIONED_HASHES_OFFSET = 258;    // position of the offset field in a serialized blob transaction (eth/eth.go:68)
constexpr uint64_t BLOB_TX_MESSAGE_START = 70;            // the offset counts from the start of the "message" (eth/eth.go:242)

// result codes (KZG_HIP_ETH_* in include/kzg_hip.h)
constexpr int ETH_CODE_TX_TOO_SHORT = 6, ETH_CODE_TX_OFFSET = 7, ETH_CODE_TX_TRAILING = 8;

// 0 and *first / *count = where the hashes lie (tx[*first .. *first + 32 * *count)), or the code of what is wrong with the transaction.
// A transaction whose first byte is not the blob type is skipped as the caller's loop skips it: 0 with *count = 0.  A transaction of length
// 0 is too short (the reference's loop panics on tx[0] there).
inline int tx_peek_blob_versioned_hashes(const uint8_t *tx, uint64_t len, uint64_t *first, uint64_t *count) {
    *first = 0; *count = 0;
    if (len == 0) return ETH_CODE_TX_TOO_SHORT;
    if (tx[0] != BLOB_TX_TYPE) return 0;
    if (len < BLOB_VERSIONED_HASHES_OFFSET + 4) return ETH_CODE_TX_TOO_SHORT;
    const uint8_t *f = tx + BLOB_VERSIONED_HASHES_OFFSET;
    const uint64_t offset = (uint64_t)((uint32_t)f[0] | (uint32_t)f[1] << 8 | (uint32_t)f[2] << 16 | (uint32_t)f[3] << 24) + BLOB_TX_MESSAGE_START;   // in 64 bits: no wrap
    if (offset > len) return ETH_CODE_TX_OFFSET;
    if ((len - offset) % 32 != 0) return ETH_CODE_TX_TRAILING;
    *first = offset; *count = (len - offset) / 32;
    return 0;
}

}  // namespace kzg
