// capi_eth_prove.hip -- eth.ComputeAggregateKZGProof (eth/eth.go:175-181, eth/helpers.go:137-176,215-260,264-285) over many sidecars in one call:
// the batched block prover.  Per chunk of whole sidecars: ONE upload of the raw bytes, then blobs -> polynomials -> commitments (the table
// walk over all B blobs) -> compressed commitments -> transcripts -> aggregated polynomials -> quotients -> proofs (the table walk over the S
// quotients) -> compression; one download of the results.  A prover's transcript needs its own commitments, so the chain is hashed in two
// halves (eth_aggregate.hpp): everything but the last 32 blob bytes and the commitments beside the table walk, the rest behind it.
#include "capi_common.hpp"
#include "eth_aggregate.hpp"

namespace {

thread_local uint64_t g_prove_chunks = 0;   // chunks of this thread's last batched call (test hook)

struct event_pair {
    hipEvent_t up = nullptr, half = nullptr;
    int create() {
        HIPCHK(hipEventCreateWithFlags(&up, hipEventDisableTiming));
        HIPCHK(hipEventCreateWithFlags(&half, hipEventDisableTiming));
        return KZG_HIP_OK;
    }
    ~event_pair() { if (up) hipEventDestroy(up); if (half) hipEventDestroy(half); }
};
// host buffers that stream copies read from / write into: declared by the entry point BEFORE its drain_on_exit
struct prove_host { std::vector<uint8_t> res; std::vector<fr> r, z; std::vector<sha256> chain; };

struct prove_ctx {
    kzg_hip_eth *eth;
    hipStream_t s, s2;            // s2: where the blob half of the transcripts runs beside the table walk; null: on s
    hipEvent_t ev_up, ev_half;
    bool host_io;                 // blobs and outputs are host buffers (else device-resident, no synchronisation)
    bool on_device;               // transcripts on the device (always when !host_io)
    prove_host *h;
};

// One chunk: S sidecars, off[0 .. S] (host) their blob offsets within the chunk, B = off[S] blobs at `blobs`.  out_comms may be null.
int prove_chunk(const prove_ctx &c, const uint8_t *blobs, const uint64_t *off, uint64_t S, uint8_t *out_proofs, uint8_t *out_comms, uint8_t *out_status) {
    kzg_hip_eth *eth = c.eth;
    hipStream_t s = c.s;
    const uint64_t n = eth->n, B = off[S];
    dtmp<uint8_t> d_in(s), d_res(s), d_ast(s); dtmp<uint64_t> d_off(s); dtmp<uint32_t> d_bad(s), d_flag(s), d_st8(s);
    dtmp<fr> d_poly(s), d_r(s), d_z(s), d_y(s), d_agg(s), d_q(s); dtmp<g1j> d_pts(s), d_qpts(s);
    struct drain_second { hipStream_t s; ~drain_second() { if (s) (void)hipStreamSynchronize(s); } } drain2{c.s2};   // declared after the temporaries: whatever way this returns, the second stream has drained before they are freed
    const uint64_t extra = eth_quotient_scratch_elems(n, S);
    // the results as one block: S proofs | B commitments | S status bytes
    CHK(d_res.alloc(48 * (S + B) + S));
    uint8_t *d_proofs = d_res.p, *d_comm = d_res.p + 48 * S, *d_status = d_res.p + 48 * (S + B);
    CHK(d_ast.alloc(S)); CHK(d_off.alloc(S + 1)); CHK(d_bad.alloc(B)); CHK(d_flag.alloc(S)); CHK(d_st8.alloc(8 * S)); CHK(d_poly.alloc(B * n));
    CHK(d_r.alloc(S)); CHK(d_z.alloc(S)); CHK(d_y.alloc(S)); CHK(d_agg.alloc(S * n)); CHK(d_q.alloc(S * n + extra)); CHK(d_pts.alloc(B)); CHK(d_qpts.alloc(S));
    HIPCHK(hipMemsetAsync(d_ast.p, 0, S, s));
    HIPCHK(hipMemsetAsync(d_flag.p, 0, S * 4, s));
    if (B) HIPCHK(hipMemsetAsync(d_bad.p, 0, B * 4, s));
    HIPCHK(hipMemcpyAsync(d_off.p, off, (S + 1) * 8, hipMemcpyHostToDevice, s));
    const uint8_t *src = blobs;
    if (c.host_io && B) {
        CHK(d_in.alloc(B * n * 32));
        CHK(h2d_copy(d_in.p, blobs, B * n * 32, s));
        src = d_in.p;
    }
    if (c.on_device) {
        if (c.s2) {
            HIPCHK(hipEventRecord(c.ev_up, s));
            HIPCHK(hipStreamWaitEvent(c.s2, c.ev_up, 0));
            launch_eth_transcript_blobs(c.s2, src, d_off.p, n, S, d_st8.p);
            HIPCHK(hipEventRecord(c.ev_half, c.s2));
        } else {
            launch_eth_transcript_blobs(s, src, d_off.p, n, S, d_st8.p);
        }
    }
    if (B) {
        launch_fr_from_le32(s, src, d_poly.p, n, B, d_bad.p);                       // BlobsToPolynomials, eth/helpers.go:264-285
        CHK(commit_rows(eth->ks, s, d_poly.p, n, B, d_pts.p, 0, false));           // PolynomialToKZGCommitment of every blob, eth/helpers.go:166-169
        launch_g1_compress(s, d_pts.p, d_comm, B);
    }
    HIPCHK(hipGetLastError());
    if (c.on_device) {
        if (c.s2) HIPCHK(hipStreamWaitEvent(s, c.ev_half, 0));
        launch_eth_transcript_finish(s, src, d_comm, d_off.p, n, S, d_st8.p, d_r.p, d_z.p);
    } else {
        // as the lone call does: the calling thread hashes header and blobs (sha256.cpp) while the device commits, and finishes every chain once
        // the commitments are down
        prove_host &h = *c.h;
        h.res.resize(48 * (S + B) + S);
        if (B) HIPCHK(hipMemcpyAsync(h.res.data() + 48 * S, d_comm, 48 * B, hipMemcpyDeviceToHost, s));
        h.chain.assign(S, sha256());
        for (uint64_t j = 0; j < S; j++) {
            const uint64_t cnt = off[j + 1] - off[j];
            h.chain[j].update("FSBLOBVERIFY_V1_", 16);
            h.chain[j].update_u64_le(n);
            h.chain[j].update_u64_le(cnt);
            if (cnt) h.chain[j].update(blobs + off[j] * n * 32, cnt * n * 32);
        }
        HIPCHK(hipStreamSynchronize(s));
        h.r.resize(S); h.z.resize(S);
        for (uint64_t j = 0; j < S; j++) {
            const uint64_t cnt = off[j + 1] - off[j];
            if (cnt) h.chain[j].update(h.res.data() + 48 * (S + off[j]), cnt * 48);
            uint8_t tr[33], d[32];
            h.chain[j].final(tr);
            for (int tag = 0; tag < 2; tag++) {
                tr[32] = (uint8_t)tag;
                sha256 h2;
                h2.update(tr, 33);
                h2.final(d);
                (tag ? h.z : h.r)[j] = fr_from_digest_bytes(d);
            }
        }
        HIPCHK(hipMemcpyAsync(d_r.p, h.r.data(), S * sizeof(fr), hipMemcpyHostToDevice, s));
        HIPCHK(hipMemcpyAsync(d_z.p, h.z.data(), S * sizeof(fr), hipMemcpyHostToDevice, s));
    }
    launch_eth_agg_poly(s, src, d_off.p, d_r.p, n, S, d_agg.p, d_ast.p);           // bls.PolyLinComb over the powers of r, eth/helpers.go:137-147
    // ComputeKZGProof(aggregatedPoly, evaluationChallenge), eth/helpers.go:175
    launch_eth_quotient(s, d_agg.p, n, eth->d_domain, n, S, d_z.p, 1, eth->fs->d_inv_pow2 + ilog2(n), d_q.p, d_y.p, d_flag.p, 1, extra ? d_q.p + S * n : nullptr);
    CHK(commit_rows(eth->ks, s, d_q.p, n, S, d_qpts.p, 0, false));
    launch_g1_compress(s, d_qpts.p, d_proofs, S);
    launch_eth_prove_finish(s, d_ast.p, d_flag.p, d_off.p, S, KZG_HIP_ERR_BAD_BLOB, KZG_HIP_ERR_BAD_ARG, d_proofs, d_comm, d_status);
    HIPCHK(hipGetLastError());
    if (c.host_io) {
        prove_host &h = *c.h;
        h.res.resize(48 * (S + B) + S);
        HIPCHK(hipMemcpyAsync(h.res.data(), d_res.p, 48 * (S + B) + S, hipMemcpyDeviceToHost, s));
        HIPCHK(hipStreamSynchronize(s));
        memcpy(out_proofs, h.res.data(), 48 * S);
        if (out_comms && B) memcpy(out_comms, h.res.data() + 48 * S, 48 * B);
        memcpy(out_status, h.res.data() + 48 * (S + B), S);
    } else {
        HIPCHK(hipMemcpyAsync(out_proofs, d_proofs, 48 * S, hipMemcpyDeviceToDevice, s));
        if (out_comms && B) HIPCHK(hipMemcpyAsync(out_comms, d_comm, 48 * B, hipMemcpyDeviceToDevice, s));
        HIPCHK(hipMemcpyAsync(out_status, d_status, S, hipMemcpyDeviceToDevice, s));
    }
    return KZG_HIP_OK;
}

// call-level checks shared by the two forms; *total = sum of blob_counts
int prove_check(kzg_hip_eth *eth, const void *blobs, const uint64_t *blob_counts, uint64_t sidecars, const void *out_proofs48, const void *status, uint64_t *total) {
    if (!blob_counts || !out_proofs48 || !status) return KZG_HIP_ERR_BAD_ARG;
    const uint64_t cap = (UINT64_MAX >> 3) / (eth->n * 32);                       // (the byte offsets and the chunk budget's sums must not overflow either)
    uint64_t t = 0;
    for (uint64_t j = 0; j < sidecars; j++) {
        if (blob_counts[j] > UINT64_MAX - t) return KZG_HIP_ERR_TOO_WIDE;
        t += blob_counts[j];
    }
    if (t > cap || sidecars > cap) return KZG_HIP_ERR_TOO_WIDE;
    if (t && !blobs) return KZG_HIP_ERR_BAD_ARG;
    *total = t;
    return KZG_HIP_OK;
}
// the chunk that starts at sidecar j0: whole sidecars while they fit the byte budget -- a sidecar costs twice its blob bytes (the raw bytes and
// the polynomials) plus two rows of n elements (its aggregated polynomial and its quotient); a larger sidecar forms a chunk by itself
uint64_t prove_chunk_end(const uint64_t *blob_counts, uint64_t sidecars, uint64_t j0, uint64_t n, uint64_t budget, std::vector<uint64_t> &off) {
    off.assign(1, 0);
    uint64_t j1 = j0;
    while (j1 < sidecars) {
        const uint64_t nb = off.back() + blob_counts[j1];
        if (j1 > j0 && (2 * nb + 2 * (j1 - j0 + 1)) * n * 32 > budget) break;
        off.push_back(nb); j1++;
    }
    return j1;
}
uint64_t prove_budget() { return (uint64_t)(knobs::eth_prove_chunk_mb() * 1048576.0); }   // (fractions allowed: tests force chunks of a few small blobs)

}   // namespace

int kzg_hip_eth_compute_aggregate_kzg_proof_batch(kzg_hip_eth *eth, const void *blobs_le32, const uint64_t *blob_counts, uint64_t sidecars, void *out_proofs48,
                                                  void *out_commitments48, uint8_t *status) {
    if (!eth) return KZG_HIP_ERR_BAD_ARG;
    if (!sidecars) return KZG_HIP_OK;
    KZG_TRY
    uint64_t total = 0;
    CHK(prove_check(eth, blobs_le32, blob_counts, sidecars, out_proofs48, status, &total));
    const uint64_t n = eth->n;
    // where the chains are hashed: a host thread takes 0.28 ms per four-blob sidecar, the device call 30 ms + 0.017 ms per sidecar (the blob half of
    // the chains beside the table walk): the host wins at 64 sidecars (18.3 against 30.3 ms), the device at 128 (32.4 against 36.1 ms), and the
    // lines through the measured points cross at 112 (profiles/compute_aggregate.md)
    const knobs::transcript_mode forced = knobs::eth_transcript();
    constexpr uint64_t TRANSCRIPT_DEVICE_FROM = 112;
    const bool on_device = forced == knobs::transcript_mode::by_count ? sidecars >= TRANSCRIPT_DEVICE_FROM : forced == knobs::transcript_mode::device;
    const uint64_t budget = prove_budget();
    const uint8_t *blobs = (const uint8_t *)blobs_le32;

    stream_lease lease(eth->fs);
    hipStream_t s = lease.s;
    // the blob half of the transcripts runs beside the table walk on a second stream when the pool has one to give
    std::unique_ptr<stream_lease> lease2;
    if (on_device && knobs::eth_prove_overlap() && !lease.fallback.owns_lock()) {
        lease2.reset(new stream_lease(eth->fs, std::try_to_lock));
        if (!lease2->s) lease2.reset();
    }
    event_pair ev;
    if (lease2) CHK(ev.create());
    std::shared_lock<std::shared_mutex> tl(eth->ks->tab_mu);
    { dev_guard g(eth->fs); CHK(ensure_fixed_table(eth->ks, s)); }                 // built once, before the first chunk
    prove_host h; std::vector<uint64_t> off;
    drain_on_exit drain(s);                                                      // declared after the host buffers the stream copies from / into
    const prove_ctx c{eth, s, lease2 ? lease2->s : nullptr, ev.up, ev.half, true, on_device, &h};
    uint64_t j0 = 0, b0 = 0, chunks = 0;
    while (j0 < sidecars) {
        const uint64_t j1 = prove_chunk_end(blob_counts, sidecars, j0, n, budget, off);
        CHK(prove_chunk(c, blobs + b0 * n * 32, off.data(), j1 - j0, (uint8_t *)out_proofs48 + 48 * j0,
                        out_commitments48 ? (uint8_t *)out_commitments48 + 48 * b0 : nullptr, status + j0));
        b0 += off.back(); j0 = j1; chunks++;
    }
    g_prove_chunks = chunks;
    return KZG_HIP_OK;
    KZG_CATCH
}

// The same with every data buffer device-resident (blobs 4-byte aligned), on the handle's stream, with no host synchronisation once the commitment table exists;
// the transcripts are always hashed on the device.  blob_counts stays a HOST array: it sizes the launches, as n and batch do elsewhere.
int kzg_hip_eth_compute_aggregate_kzg_proof_batch_dev(kzg_hip_eth *eth, const void *d_blobs_le32, const uint64_t *blob_counts, uint64_t sidecars, void *d_out_proofs48,
                                                      void *d_out_commitments48, uint8_t *d_status) {
    if (!eth) return KZG_HIP_ERR_BAD_ARG;
    if (!sidecars) return KZG_HIP_OK;
    KZG_TRY
    uint64_t total = 0;
    CHK(prove_check(eth, d_blobs_le32, blob_counts, sidecars, d_out_proofs48, d_status, &total));
    const uint64_t n = eth->n, budget = prove_budget();
    const uint8_t *blobs = (const uint8_t *)d_blobs_le32;
    std::shared_lock<std::shared_mutex> tl(eth->ks->tab_mu);
    dev_guard g(eth->fs);
    hipStream_t s = eth->fs->stream;
    CHK(ensure_fixed_table(eth->ks, s));
    // the chunks' offsets are copied to the device asynchronously: they live until the stream has passed the last copy (a host function at the
    // end of the enqueued work frees them; an error path drains the stream first)
    struct keep_t {
        hipStream_t s; std::vector<std::vector<uint64_t>> *offs;
        ~keep_t() { if (offs) { (void)hipStreamSynchronize(s); delete offs; } }
    } keep{s, new std::vector<std::vector<uint64_t>>()};
    const prove_ctx c{eth, s, nullptr, nullptr, nullptr, false, true, nullptr};
    uint64_t j0 = 0, b0 = 0;
    while (j0 < sidecars) {
        keep.offs->emplace_back();
        std::vector<uint64_t> &off = keep.offs->back();
        const uint64_t j1 = prove_chunk_end(blob_counts, sidecars, j0, n, budget, off);
        CHK(prove_chunk(c, blobs + b0 * n * 32, off.data(), j1 - j0, (uint8_t *)d_out_proofs48 + 48 * j0,
                        d_out_commitments48 ? (uint8_t *)d_out_commitments48 + 48 * b0 : nullptr, d_status + j0));
        b0 += off.back(); j0 = j1;
    }
    g_prove_chunks = keep.offs->size();
    HIPCHK(hipLaunchHostFunc(s, [](void *p) { delete (std::vector<std::vector<uint64_t>> *)p; }, keep.offs));
    keep.offs = nullptr;
    return KZG_HIP_OK;
    KZG_CATCH
}

// test hook (kzg_hip_internal.h): chunks of the calling thread's last successful batched prover call
uint64_t kzg_hip_test_eth_prove_chunks(void) { return g_prove_chunks; }
