// Host build of eth_exec.hpp / eth_tx.hpp for tests/test_eth_exec_host.py: the lane bodies of k_eth_exec.hip and the host-side peek of
// capi_eth_exec.hip on the CPU.  As a shared object: the hooks below.  With -DEE_MAIN: a stand-alone program (the form that runs under
// sanitizers) that reads transactions and commitments from a file and prints what the peek and the hash lane make of them.
#include "eth_exec.hpp"
#include "eth_tx.hpp"

using namespace kzg;

extern "C" {
// KZGToVersionedHash of n commitments, 32 bytes each
void ee_versioned_hashes(const uint8_t *c48, uint64_t n, uint8_t *out32) {
    for (uint64_t t = 0; t < n; t++) {
        uint32_t h[8];
        kzg_to_versioned_hash_lane(c48 + 48 * t, h);
        for (int i = 0; i < 8; i++)
            for (int k = 0; k < 4; k++) out32[32 * t + 4 * i + k] = (uint8_t)(h[i] >> (24 - 8 * k));
    }
}
// eth_precompile_inputs_lane over n rows of 192 bytes: status[t], and inf[t] = whether both points came back as the point at infinity
void ee_precompile_inputs(const uint8_t *in192, uint64_t n, uint8_t *status, uint8_t *inf) {
    for (uint64_t t = 0; t < n; t++) {
        g1j p0, p1;
        uint8_t st = 0xff;
        eth_precompile_inputs_lane(in192 + 192 * t, p0, p1, st);
        status[t] = st;
        inf[t] = is_inf(p0) && is_inf(p1) ? 1 : 0;
    }
}
int ee_tx_peek(const uint8_t *tx, uint64_t len, uint64_t *first, uint64_t *count) { return tx_peek_blob_versioned_hashes(tx, len, first, count); }
}

#ifdef EE_MAIN
// input file: u64 n_tx | n_tx x (u64 len | len bytes) | u64 n_comm | n_comm x 48 bytes.  Every transaction is copied into an allocation of
// exactly its length, so that a read past its end is a heap overflow the sanitizer reports.  Output: "T code first count" per transaction,
// "H hex" per commitment.
#include <stdio.h>
#include <string.h>
#include <vector>
int main(int argc, char **argv) {
    if (argc != 2) return 2;
    FILE *f = fopen(argv[1], "rb");
    if (!f) return 2;
    uint64_t n_tx = 0, n_comm = 0;
    if (fread(&n_tx, 8, 1, f) != 1 || n_tx > (1u << 20)) return 2;
    for (uint64_t t = 0; t < n_tx; t++) {
        uint64_t len = 0;
        if (fread(&len, 8, 1, f) != 1 || len > (1u << 24)) return 2;
        uint8_t *tx = new uint8_t[len];
        if (len && fread(tx, 1, len, f) != len) return 2;
        uint64_t first = 99, count = 99;
        const int code = tx_peek_blob_versioned_hashes(tx, len, &first, &count);
        if (!code && first + 32 * count > len) return 3;   // (what the caller copies lies inside the transaction)
        printf("T %d %llu %llu\n", code, (unsigned long long)first, (unsigned long long)count);
        delete[] tx;
    }
    if (fread(&n_comm, 8, 1, f) != 1 || n_comm > (1u << 20)) return 2;
    for (uint64_t t = 0; t < n_comm; t++) {
        uint8_t *c = new uint8_t[48], out[32];
        if (fread(c, 1, 48, f) != 48) return 2;
        ee_versioned_hashes(c, 1, out);
        printf("H ");
        for (int i = 0; i < 32; i++) printf("%02x", out[i]);
        printf("\n");
        delete[] c;
    }
    fclose(f);
    return 0;
}
#endif
