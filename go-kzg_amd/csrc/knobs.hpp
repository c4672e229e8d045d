// knobs.hpp -- every environment variable the library reads, and the ONLY file of csrc/ that names one or calls getenv.
//
// One row per switch: its read time (the macro), the type and name of its accessor, the variable, and its value grammar as an expression in
// `e` (the variable's value, null when unset).  A row defines
//     parse_<accessor>(const char *e)   the pure parser: no static, no getenv (tests/host/knobs_test.cpp calls it with strings), and
//     <accessor>()                      the parser applied to getenv(name) at the row's read time:
//         KZG_KNOB_ONCE        once per process (a function-local static: later changes of the environment are not seen)
//         KZG_KNOB_PER_CALL    on every call of the accessor (probes and tests switch these within one process)
//         KZG_KNOB_PER_HANDLE  the same, called only while a handle or a coalescer is constructed
// The few switches whose default or bound belongs to the caller are written out as functions below the table.  New switches go here, with
// their read time, and into README's table (tests/test_knobs_docs.py compares the two); a second parser elsewhere is a bug.
// Host-only and free of HIP: sha256.cpp (built by the host compiler) and the simulated coalescer of the tests include it too.
// (GPU_MAX_HW_QUEUES belongs to the runtime: the library does not read it.)
#pragma once
#include <limits.h>
#include <stdint.h>
#include <stdlib.h>
#include <string.h>

namespace kzg {

// what KZG_HIP_MULTI_FAULT injects into the exchanges of a multi-device handle (capi_multi.hip)
enum { FAULT_RCCL = 1, FAULT_RCCL_CORRUPT = 2, FAULT_PEER = 4, FAULT_PEER_CORRUPT = 8, FAULT_RCCL_HANG = 16, FAULT_PEER_HANG = 32, FAULT_PEER_STUCK = 64, FAULT_RCCL_BLOCK = 128, FAULT_RCCL_INIT_BLOCK = 256 };

namespace knobs {

enum class g1_fft_mode { by_size, direct, radix2 };
enum class g1_mul_mode { by_shape, regular, wnaf };
enum class fr_fft_mode { by_size, radix2, shared };
enum class zero_poly_mode { by_size, direct, tree };
enum class msm_reduce_mode { by_batch, scan, chunks };
enum class transcript_mode { by_count, host, device };
enum class pairing_mode { by_count, lane, wave };
enum class combine_mode { by_count, never, always };
enum class transport_mode { by_devices, rccl, host, peer };
enum class fb_layout_mode { by_batch, windows, shared, paired };
struct opt_gb { bool set; double gb; };   // a table budget: unset leaves the size to the caller's policy

// ---- grammar
inline bool is(const char *e, const char *word) { return e && !strcmp(e, word); }    // exactly `word`
inline bool starts(const char *e, char c) { return e && e[0] == c; }                 // anything that begins with c
inline bool list_has(const char *e, const char *word) {                              // `word` is a whole entry of the comma-separated list
    const size_t n = strlen(word);
    for (const char *at = e; e && (at = strstr(at, word)); at += n)
        if ((at == e || at[-1] == ',') && (at[n] == 0 || at[n] == ',')) return true;
    return false;
}
inline zero_poly_mode zero_poly_of(const char *e) { return is(e, "direct") ? zero_poly_mode::direct : is(e, "tree") ? zero_poly_mode::tree : zero_poly_mode::by_size; }
inline double positive_or(const char *e, double dflt) { const double v = e ? atof(e) : 0.0; return v > 0.0 ? v : dflt; }
inline unsigned multi_fault_of(const char *e) {
    if (!e) return 0;
    return (list_has(e, "rccl") ? FAULT_RCCL : 0) | (list_has(e, "rccl-corrupt") ? FAULT_RCCL_CORRUPT : 0) | (list_has(e, "peer") ? FAULT_PEER : 0) |
           (list_has(e, "peer-corrupt") ? FAULT_PEER_CORRUPT : 0) | (list_has(e, "rccl-hang") ? FAULT_RCCL_HANG : 0) |
           (list_has(e, "rccl-block") ? FAULT_RCCL_BLOCK : 0) |             // the RCCL calls of the probe block on the HOST side (the helper thread sleeps three deadlines)
           (list_has(e, "rccl-init-block") ? FAULT_RCCL_INIT_BLOCK : 0) |   // ncclCommInitAll does not return in time
           (list_has(e, "peer-hang") ? FAULT_PEER_HANG : 0) |
           (list_has(e, "peer-stuck") ? FAULT_PEER_HANG | FAULT_PEER_STUCK : 0);   // ... and is NOT let go after its streams were abandoned: stuck until the kernel's own clock runs out
}

#define KZG_KNOB_ONCE(type, fn, name, expr)                   \
    inline type parse_##fn(const char *e) { return expr; }    \
    inline type fn() { static type const v = parse_##fn(getenv(name)); return v; }
#define KZG_KNOB_PER_CALL(type, fn, name, expr)               \
    inline type parse_##fn(const char *e) { return expr; }    \
    inline type fn() { return parse_##fn(getenv(name)); }
#define KZG_KNOB_PER_HANDLE KZG_KNOB_PER_CALL

// ---- booleans.  Default on, off for a value that begins with '0' -- except KZG_HIP_FB_GLV, which is off for exactly "0" only ("00" leaves it on)
KZG_KNOB_ONCE(bool, fb_glv, "KZG_HIP_FB_GLV", !is(e, "0"))                              // off: the plain fixed-base layout, one window per c bits of the whole scalar (A/B runs, tests)
KZG_KNOB_ONCE(bool, coalesce, "KZG_HIP_COALESCE", !starts(e, '0'))                      // off: one-polynomial calls take the handle mutex instead of being merged
KZG_KNOB_ONCE(bool, upload_ramp, "KZG_HIP_UPLOAD_RAMP", !starts(e, '0'))                // off: equal upload chunks in the host-buffer batch commitment (A/B runs)
KZG_KNOB_ONCE(bool, lincomb_promote, "KZG_HIP_LINCOMB_PROMOTE", !starts(e, '0'))        // off: caller-supplied point sets are never promoted to cached sets
KZG_KNOB_ONCE(bool, stream_cache, "KZG_HIP_STREAM_CACHE", !starts(e, '0'))              // off: stream-ordered temporaries are never kept per stream (A/B runs, tests)
KZG_KNOB_ONCE(bool, g1_direct_coop, "KZG_HIP_G1_DIRECT_COOP", !starts(e, '0'))          // off: one lane per (output, term) in the direct G1 passes
KZG_KNOB_ONCE(bool, coop_inv, "KZG_HIP_COOP_INV", !starts(e, '0'))                      // off: the one-lane inversion for small outputs too (A/B runs, tests)
KZG_KNOB_ONCE(bool, fk20_pass1, "KZG_HIP_FK20_PASS1", !starts(e, '0'))                  // off: Toeplitz stage and first direct pass of a lone polynomial as separate kernels
KZG_KNOB_ONCE(bool, fk20_fuse, "KZG_HIP_FK20_FUSE", !starts(e, '0'))                    // off: the unfused FK20 pipeline (tests compare both)
KZG_KNOB_ONCE(bool, fk20_pad, "KZG_HIP_FK20_PAD", !starts(e, '0'))                      // off: ragged FK20 batches are not padded
KZG_KNOB_PER_CALL(bool, eth_prove_overlap, "KZG_HIP_ETH_PROVE_OVERLAP", !starts(e, '0'))     // off: the batched aggregate prover hashes the blob half of its transcripts on the main stream, not beside the table walk (A/B runs, tests)
// default off, on when set at all (the empty string included)
KZG_KNOB_ONCE(bool, coalesce_trace, "KZG_HIP_COALESCE_TRACE", e != nullptr)             // phase times of every coalesced commitment batch on stderr (adds two synchronisations)
KZG_KNOB_PER_CALL(bool, coalesce_stats, "KZG_HIP_COALESCE_STATS", e != nullptr)         // a coalescer prints its statistics on stderr when it is destroyed
KZG_KNOB_ONCE(bool, eth_quotient_one, "KZG_HIP_ETH_QUOTIENT", is(e, "one"))             // exactly "one": one workgroup per row at every size (A/B runs, tests)
KZG_KNOB_ONCE(bool, sha256_portable, "KZG_HIP_SHA256", is(e, "portable"))               // exactly "portable": no x86 SHA extensions (tests compare the two)

// ---- modes.  Unset, and for the exact-word grammars every other value, leaves the choice to the launcher
KZG_KNOB_ONCE(g1_fft_mode, g1_fft, "KZG_HIP_G1_FFT", !e ? g1_fft_mode::by_size : e[0] == 'd' ? g1_fft_mode::direct : g1_fft_mode::radix2)   // "direct"; ANY other value is radix2
KZG_KNOB_ONCE(int, g1_quad, "KZG_HIP_G1_QUAD", !e ? -1 : e[0] == '0' ? 0 : e[0] == '2' ? 2 : 1)                                            // -1 by launch size; 0 / 1 / 2: never / always four / always two lanes per butterfly
KZG_KNOB_ONCE(g1_mul_mode, g1_mul, "KZG_HIP_G1_MUL", starts(e, 'r') ? g1_mul_mode::regular : starts(e, 'w') ? g1_mul_mode::wnaf : g1_mul_mode::by_shape)   // "regular" / "wnaf" by their first letter
KZG_KNOB_ONCE(fr_fft_mode, fr_fft, "KZG_HIP_FR_FFT", is(e, "radix2") ? fr_fft_mode::radix2 : is(e, "shared") ? fr_fft_mode::shared : fr_fft_mode::by_size)   // radix2: no lazy-limb kernel anywhere; shared: k_fr_fft_small at every batch size (tests)
KZG_KNOB_ONCE(zero_poly_mode, zero_poly_once, "KZG_HIP_ZERO_POLY", zero_poly_of(e))                                                         // "direct" / "tree": the lone calls
KZG_KNOB_PER_CALL(zero_poly_mode, zero_poly_per_call, "KZG_HIP_ZERO_POLY", zero_poly_of(e))                                                 // the batch calls (a measurement switches within one process)
KZG_KNOB_ONCE(msm_reduce_mode, msm_reduce, "KZG_HIP_MSM_REDUCE", is(e, "chunks") ? msm_reduce_mode::chunks : is(e, "scan") ? msm_reduce_mode::scan : msm_reduce_mode::by_batch)   // bucket MSM: force a reduce form (A/B runs, tests)
KZG_KNOB_ONCE(int, msm_seg, "KZG_HIP_MSM_SEG", e ? atoi(e) : -1)                                                                            // bucket MSM: 0 / 1 never / always the balanced accumulate; any other number: by batch
KZG_KNOB_PER_CALL(transcript_mode, eth_transcript, "KZG_HIP_ETH_TRANSCRIPT", is(e, "host") ? transcript_mode::host : is(e, "device") ? transcript_mode::device : transcript_mode::by_count)   // where the aggregate verifier and the batched aggregate prover hash
KZG_KNOB_PER_CALL(pairing_mode, pairing, "KZG_HIP_PAIRING", is(e, "lane") ? pairing_mode::lane : is(e, "wave") ? pairing_mode::wave : pairing_mode::by_count)   // the kernel of every pairing check: one lane or one wavefront per check (launch_pairing_check; tests, A/B runs)
KZG_KNOB_PER_CALL(combine_mode, verify_combine, "KZG_HIP_VERIFY_COMBINE", is(e, "never") ? combine_mode::never : is(e, "always") ? combine_mode::always : combine_mode::by_count)   // the _combined proof checks: per-row checks or one check per group of rows at every count (capi_verify.hip; tests, A/B runs)
KZG_KNOB_PER_CALL(fb_layout_mode, fb_layout, "KZG_HIP_FB_LAYOUT", is(e, "windows") ? fb_layout_mode::windows : is(e, "shared") ? fb_layout_mode::shared : is(e, "paired") ? fb_layout_mode::paired : fb_layout_mode::by_batch)   // commitment tables: "windows" never builds or walks a table of large batches, "shared" walks the single-point shared-window table at every batch size, "paired" makes the table of large batches the paired-point one at any budget; anything else ("auto"): large batches only, the layout with fewer additions (capi_kzg.hip)
KZG_KNOB_PER_CALL(int, multi_fft, "KZG_HIP_MULTI_FFT", !e ? -1 : is(e, "sharded") ? 1 : 0)                                                   // -1 the handle's policy; "sharded" 1; ANY other value gathers (0)
KZG_KNOB_PER_HANDLE(transport_mode, multi_transport, "KZG_HIP_MULTI_TRANSPORT", !e ? transport_mode::by_devices : is(e, "rccl") ? transport_mode::rccl : is(e, "host") ? transport_mode::host : transport_mode::peer)   // any other value: peer copies, RCCL is not bound
KZG_KNOB_PER_HANDLE(unsigned, multi_fault, "KZG_HIP_MULTI_FAULT", multi_fault_of(e))                                                        // tests: a comma-separated list of legs of the exchange that fail, FAULT_* above
KZG_KNOB_ONCE(const char *, rccl_lib, "KZG_HIP_RCCL_LIB", e)                                                                                // the RCCL to bind before librccl.so.1 (null or empty: none)

// ---- numbers
KZG_KNOB_ONCE(uint32_t, lincomb_promote_after, "KZG_HIP_LINCOMB_PROMOTE_AFTER", (uint32_t)(!e ? 2 : atol(e) < 1 ? 1 : atol(e) > 1000 ? 1000 : atol(e)))   // sightings before a point set is promoted: 1 .. 1000
KZG_KNOB_ONCE(uint64_t, fb_lanes, "KZG_HIP_FB_LANES", e ? strtoull(e, nullptr, 10) : 0ull)                                                  // lanes of one table-walk launch; 0: two resident waves per SIMD
KZG_KNOB_ONCE(uint64_t, eth_stage_rows, "KZG_HIP_ETH_STAGE_ROWS", e ? (uint64_t)atol(e) : 0ull)                                             // coalesced eth proof batches of up to this many rows are copied to HBM first (A/B runs, tests)
KZG_KNOB_PER_CALL(uint64_t, fb_shared_min_batch, "KZG_HIP_FB_SHARED_MIN_BATCH", e && strtoull(e, nullptr, 10) >= 1 ? strtoull(e, nullptr, 10) : 0ull)                    // rows from which a commitment batch walks the shared-window table, at least 1; 0 (unset, or no such number): the library's measured crossovers
KZG_KNOB_PER_CALL(uint64_t, verify_combine_rows, "KZG_HIP_VERIFY_COMBINE_ROWS", e && strtoull(e, nullptr, 10) >= 1 ? strtoull(e, nullptr, 10) : 0ull)                  // rows per group of the _combined proof checks, at least 1; 0 (unset, or no such number): the library's group size
KZG_KNOB_PER_CALL(double, eth_verify_chunk_mb, "KZG_HIP_ETH_VERIFY_CHUNK_MB", positive_or(e, 4096.0))                                      // blob bytes per chunk of the aggregate verifier; fractions allowed, <= 0 is the default
KZG_KNOB_PER_CALL(double, eth_prove_chunk_mb, "KZG_HIP_ETH_PROVE_CHUNK_MB", positive_or(e, 4096.0))                                        // device bytes per chunk of the batched aggregate prover (twice a sidecar's blob bytes + two rows); likewise
KZG_KNOB_PER_CALL(double, recover_chunk_mb, "KZG_HIP_RECOVER_CHUNK_MB", positive_or(e, 2048.0))                                            // device memory per chunk of the batched recovery; likewise
KZG_KNOB_PER_CALL(opt_gb, fb_budget_gb, "KZG_HIP_FB_BUDGET_GB", (opt_gb{e != nullptr, e ? atof(e) : 0.0}))                                  // commitment tables; not clamped (negative: no table fits)
KZG_KNOB_PER_CALL(opt_gb, points_fb_budget_gb, "KZG_HIP_POINTS_FB_BUDGET_GB", (opt_gb{e != nullptr, e ? atof(e) : 0.0}))                    // tables of cached point sets
KZG_KNOB_PER_CALL(opt_gb, fk20_fb_budget_gb, "KZG_HIP_FK20_FB_BUDGET_GB", (opt_gb{e != nullptr, e ? atof(e) : 0.0}))                        // FK20 Toeplitz-stage tables
KZG_KNOB_PER_HANDLE(long, multi_probe_timeout_ms, "KZG_HIP_MULTI_PROBE_TIMEOUT_MS", e && atol(e) >= 10 && atol(e) <= 600000 ? atol(e) : 10000)   // deadline of one self-test exchange; values outside 10 .. 600 000 are ignored
KZG_KNOB_PER_HANDLE(long, coalesce_us, "KZG_HIP_COALESCE_US", e ? atol(e) : 150)                                                            // upper bound of a leader's gather wait; 0 disables
KZG_KNOB_PER_HANDLE(long, coalesce_spin_us, "KZG_HIP_COALESCE_SPIN_US", e ? atol(e) : 40)                                                   // a follower's spin before it parks; 0 disables
KZG_KNOB_PER_CALL(int, coalesce_sim_max_bufs, "KZG_COALESCE_SIM_MAX_BUFS", e ? atoi(e) : INT_MAX)                                           // simulated coalescer only: staging buffers that can be allocated

#undef KZG_KNOB_ONCE
#undef KZG_KNOB_PER_CALL
#undef KZG_KNOB_PER_HANDLE

// per coalescer; default and bounds are the coalescer's: batches in flight, 1 .. max
inline int parse_coalesce_exec(const char *e, int dflt, int max) { return !e ? dflt : atoi(e) < 1 ? 1 : atoi(e) > max ? max : atoi(e); }
inline int coalesce_exec(int dflt, int max) { return parse_coalesce_exec(getenv("KZG_HIP_COALESCE_EXEC"), dflt, max); }
// per coalescer; concurrent callers per batch in flight, at least 1; the default is the pipeline's
inline int parse_coalesce_per_batch(const char *e, int dflt) { return !e ? dflt : atoi(e) < 1 ? 1 : atoi(e); }
inline int coalesce_per_batch(int dflt) { return parse_coalesce_per_batch(getenv("KZG_HIP_COALESCE_PER_BATCH"), dflt); }

}  // namespace knobs
}  // namespace kzg
