// capi_eth_exec.hip -- C ABI of the execution-layer side of eth/eth.go in batches: PointEvaluationPrecompile (eth/eth.go:76-110),
// KZGToVersionedHash (:137-141) and VerifyKZGCommitmentsAgainstTransactions with TxPeekBlobVersionedHashes (:234-282).  The kernels are in
// k_eth_exec.hip; the pairing check is capi_verify.hip's.  A lone call is one lane's work and stays on Kilic in the Go shim.
#include "capi_common.hpp"
#include "eth_tx.hpp"

namespace {

static_assert(KZG_HIP_ETH_TX_TOO_SHORT == ETH_CODE_TX_TOO_SHORT && KZG_HIP_ETH_TX_OFFSET == ETH_CODE_TX_OFFSET && KZG_HIP_ETH_TX_TRAILING == ETH_CODE_TX_TRAILING,
              "eth_tx.hpp restates the header's codes");

// the hash, the parsing and the pairing check of `count` device-resident rows on stream s; d_result[i] = the row's code
int precompile_rows(hipStream_t s, const g2_prepared *gen, const g2_prepared *s1, const uint8_t *d_in, uint64_t count, uint8_t *d_result) {
    dtmp<uint8_t> d_st(s), d_ok(s); dtmp<g1j> d_p0(s), d_p1(s);
    CHK(d_st.alloc(count)); CHK(d_ok.alloc(count)); CHK(d_p0.alloc(count)); CHK(d_p1.alloc(count));
    launch_eth_precompile_inputs(s, d_in, count, d_p0.p, d_p1.p, d_st.p);
    // e(C - [y]G1 + [z] pi, G2) e(-pi, kzgSetupG2[1]) == 1  <=>  e(C - [y]G1, G2) == e(pi, [s - z]G2)  (eth/helpers.go:55-68)
    launch_pairing_check(s, true, gen, s1, d_p0.p, d_p1.p, count, d_ok.p);
    launch_eth_merge_status(s, d_st.p, d_ok.p, count, d_result);
    HIPCHK(hipGetLastError());
    return KZG_HIP_OK;
}

}  // namespace

extern "C" {

int kzg_hip_eth_kzg_to_versioned_hash_batch(kzg_hip_eth *eth, const void *commitments48, uint64_t count, void *out32) {
    if (!eth) return KZG_HIP_ERR_BAD_ARG;
    if (!count) return KZG_HIP_OK;
    if (!commitments48 || !out32) return KZG_HIP_ERR_BAD_ARG;
    if (count > (UINT64_MAX >> 1) / 48) return KZG_HIP_ERR_TOO_WIDE;
    KZG_TRY
    stream_lease lease(eth->fs);
    hipStream_t s = lease.s;
    drain_on_exit drain(s);                                          // the stream copies from / into the caller's buffers
    dtmp<uint8_t> d_c(s), d_h(s);
    CHK(d_c.alloc(48 * count)); CHK(d_h.alloc(32 * count));
    HIPCHK(hipMemcpyAsync(d_c.p, commitments48, 48 * count, hipMemcpyHostToDevice, s));
    launch_eth_versioned_hashes(s, d_c.p, count, d_h.p);
    HIPCHK(hipGetLastError());
    HIPCHK(hipMemcpyAsync(out32, d_h.p, 32 * count, hipMemcpyDeviceToHost, s));
    HIPCHK(hipStreamSynchronize(s));
    return KZG_HIP_OK;
    KZG_CATCH
}

int kzg_hip_eth_kzg_to_versioned_hash_batch_dev(kzg_hip_eth *eth, const void *d_commitments48, uint64_t count, void *d_out32) {
    if (!eth) return KZG_HIP_ERR_BAD_ARG;
    if (!count) return KZG_HIP_OK;
    if (!d_commitments48 || !d_out32 || ((uintptr_t)d_out32 & 3)) return KZG_HIP_ERR_BAD_ARG;
    if (count > (UINT64_MAX >> 1) / 48) return KZG_HIP_ERR_TOO_WIDE;
    KZG_TRY
    dev_guard g(eth->fs);
    launch_eth_versioned_hashes(eth->fs->stream, (const uint8_t *)d_commitments48, count, (uint8_t *)d_out32);
    HIPCHK(hipGetLastError());
    return KZG_HIP_OK;
    KZG_CATCH
}

int kzg_hip_eth_point_evaluation_precompile_batch(kzg_hip_eth *eth, const void *inputs192, uint64_t count, uint8_t *result) {
    if (!eth) return KZG_HIP_ERR_BAD_ARG;
    KZG_TRY
    std::shared_ptr<g2_state> g;
    const g2_prepared *gen = nullptr, *s1 = nullptr;
    CHK(eth_g2_lines(eth, g, &gen, &s1));
    if (!count) return KZG_HIP_OK;
    if (!inputs192 || !result) return KZG_HIP_ERR_BAD_ARG;
    if (count > (UINT64_MAX >> 1) / sizeof(g1j)) return KZG_HIP_ERR_TOO_WIDE;   // (the largest per-row temporary)
    stream_lease lease(eth->fs);
    hipStream_t s = lease.s;
    drain_on_exit drain(s);                                          // the stream copies from / into the caller's buffers
    dtmp<uint8_t> d_in(s), d_res(s);
    CHK(d_in.alloc(192 * count)); CHK(d_res.alloc(count));
    HIPCHK(hipMemcpyAsync(d_in.p, inputs192, 192 * count, hipMemcpyHostToDevice, s));
    CHK(precompile_rows(s, gen, s1, d_in.p, count, d_res.p));
    HIPCHK(hipMemcpyAsync(result, d_res.p, count, hipMemcpyDeviceToHost, s));
    HIPCHK(hipStreamSynchronize(s));
    return KZG_HIP_OK;
    KZG_CATCH
}

int kzg_hip_eth_point_evaluation_precompile_batch_dev(kzg_hip_eth *eth, const void *d_inputs192, uint64_t count, uint8_t *d_result) {
    if (!eth) return KZG_HIP_ERR_BAD_ARG;
    KZG_TRY
    std::shared_ptr<g2_state> g;
    const g2_prepared *gen = nullptr, *s1 = nullptr;
    CHK(eth_g2_lines(eth, g, &gen, &s1));
    if (!count) return KZG_HIP_OK;
    if (!d_inputs192 || !d_result) return KZG_HIP_ERR_BAD_ARG;
    if (count > (UINT64_MAX >> 1) / sizeof(g1j)) return KZG_HIP_ERR_TOO_WIDE;
    dev_guard dg(eth->fs);
    hipStream_t s = eth->fs->stream;
    CHK(precompile_rows(s, gen, s1, (const uint8_t *)d_inputs192, count, d_result));
    // the prepared G2 points are read by kernels that may still be queued when this call returns, and a setter on another thread may replace
    // the handle's state meanwhile: the handle keeps this one until the stream has passed this point
    return eth_g2_hold_on_stream(eth, s, g);
    KZG_CATCH
}

int kzg_hip_eth_precompile_return_value(kzg_hip_eth *eth, void *out64) {
    if (!eth || !out64) return KZG_HIP_ERR_BAD_ARG;
    uint8_t *o = (uint8_t *)out64;
    for (int i = 0; i < 32; i++) o[i] = i < 24 ? 0 : (uint8_t)(eth->n >> (8 * (31 - i)));
    for (int i = 0; i < 32; i++) o[32 + i] = (uint8_t)(FrP::mod(7 - i / 4) >> (8 * (3 - i % 4)));
    return KZG_HIP_OK;
}

int kzg_hip_eth_verify_kzg_commitments_against_transactions_batch(kzg_hip_eth *eth, const void *txs, const uint64_t *tx_offsets, const uint64_t *tx_counts,
                                                                  const void *commitments48, const uint64_t *commitment_counts, uint64_t blocks, uint8_t *result) {
    if (!eth) return KZG_HIP_ERR_BAD_ARG;
    if (!blocks) return KZG_HIP_OK;
    if (!tx_offsets || !tx_counts || !commitment_counts || !result) return KZG_HIP_ERR_BAD_ARG;
    KZG_TRY
    uint64_t n_tx = 0, n_comm = 0;
    for (uint64_t j = 0; j < blocks; j++) {
        if (tx_counts[j] > UINT64_MAX - n_tx || commitment_counts[j] > UINT64_MAX - n_comm) return KZG_HIP_ERR_TOO_WIDE;
        n_tx += tx_counts[j]; n_comm += commitment_counts[j];
    }
    if (n_comm > (UINT64_MAX >> 1) / 48 || n_tx > (UINT64_MAX >> 1) / 8) return KZG_HIP_ERR_TOO_WIDE;   // (the byte offsets must not overflow either)
    if (n_comm && !commitments48) return KZG_HIP_ERR_BAD_ARG;
    for (uint64_t t = 0; t < n_tx; t++) if (tx_offsets[t + 1] < tx_offsets[t]) return KZG_HIP_ERR_BAD_ARG;
    if (n_tx && tx_offsets[n_tx] > tx_offsets[0] && !txs) return KZG_HIP_ERR_BAD_ARG;
    const uint8_t *tx_bytes = (const uint8_t *)txs, *comms = (const uint8_t *)commitments48;

    // the peek (eth/eth.go:263-274): each block's hashes gathered into one dense array.  A block whose peek failed has the code of its first
    // failing transaction, a block whose counts differ 5; the others (`live`) go to the device with off[k] .. off[k + 1] their hashes
    std::vector<uint8_t> hashes, live_comms;
    std::vector<uint64_t> off(1, 0), live;
    uint64_t t = 0, c0 = 0;
    for (uint64_t j = 0; j < blocks; j++) {
        const size_t mark = hashes.size();
        int code = 0;
        for (uint64_t k = 0; k < tx_counts[j]; k++, t++) {
            if (code) continue;                                    // (the first failing transaction wins; the rest are not looked at)
            const uint8_t *tx = tx_bytes + tx_offsets[t];
            uint64_t first = 0, cnt = 0;
            code = tx_peek_blob_versioned_hashes(tx, tx_offsets[t + 1] - tx_offsets[t], &first, &cnt);
            if (!code && cnt) hashes.insert(hashes.end(), tx + first, tx + first + 32 * cnt);
        }
        const uint64_t found = (hashes.size() - mark) / 32;
        if (!code && found != commitment_counts[j]) code = KZG_HIP_ETH_COUNT_MISMATCH;
        if (code) {
            result[j] = (uint8_t)code;
            hashes.resize(mark);
        } else if (!found) {
            result[j] = KZG_HIP_ETH_VALID;                         // nothing to compare
        } else {
            live.push_back(j);
            off.push_back(off.back() + found);
            live_comms.insert(live_comms.end(), comms + 48 * c0, comms + 48 * (c0 + found));
        }
        c0 += commitment_counts[j];
    }
    const uint64_t L = live.size(), total = off.back();
    if (!L) return KZG_HIP_OK;

    stream_lease lease(eth->fs);
    hipStream_t s = lease.s;
    // one upload: the offsets, the hashes and the commitments back to back (8-byte aligned parts)
    const uint64_t at_h = (L + 1) * 8, at_c = at_h + 32 * total, bytes = at_c + 48 * total;
    std::vector<uint8_t> up(bytes), codes(L);
    memcpy(up.data(), off.data(), at_h);
    memcpy(up.data() + at_h, hashes.data(), 32 * total);
    memcpy(up.data() + at_c, live_comms.data(), 48 * total);
    drain_on_exit drain(s);                                          // declared after the host buffers the stream copies from / into
    dtmp<uint8_t> d_up(s), d_match(s), d_res(s);
    CHK(d_up.alloc(bytes)); CHK(d_match.alloc(total)); CHK(d_res.alloc(L));
    HIPCHK(hipMemcpyAsync(d_up.p, up.data(), bytes, hipMemcpyHostToDevice, s));
    launch_eth_tx_hashes_check(s, d_up.p + at_c, d_up.p + at_h, (const uint64_t *)d_up.p, total, L, d_match.p, d_res.p);
    HIPCHK(hipGetLastError());
    HIPCHK(hipMemcpyAsync(codes.data(), d_res.p, L, hipMemcpyDeviceToHost, s));
    HIPCHK(hipStreamSynchronize(s));
    for (uint64_t k = 0; k < L; k++) result[live[k]] = codes[k];
    return KZG_HIP_OK;
    KZG_CATCH
}

}  // extern "C"
