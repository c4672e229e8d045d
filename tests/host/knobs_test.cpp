// knobs_test.cpp -- every pure parser of go-kzg_amd/csrc/knobs.hpp against a table of (value, result) written from the hand-written parsers the
// registry replaced: unset (null), the empty string, the documented values and near misses.  The oddities are the point: "00" leaves KZG_HIP_FB_GLV
// on and turns KZG_HIP_COALESCE off; KZG_HIP_G1_MUL=radix is "regular"; an empty KZG_HIP_MSM_SEG is 0.  Stand-alone: prints the misses, exit status 1 if any.
#include "../../go-kzg_amd/csrc/knobs.hpp"
#include <stdio.h>

using namespace kzg;
using namespace kzg::knobs;

static int checks = 0, misses = 0;
static const char *show(const char *in) { return in ? in : "(unset)"; }
static void expect(const char *parser, const char *in, long long got, long long want) {
    checks++;
    if (got != want) { misses++; printf("MISS %s(\"%s\") = %lld, expected %lld\n", parser, show(in), got, want); }
}
static void expect_d(const char *parser, const char *in, double got, double want) {
    checks++;
    if (got != want) { misses++; printf("MISS %s(\"%s\") = %g, expected %g\n", parser, show(in), got, want); }
}
struct row { const char *in; long long want; };
struct row_d { const char *in; double want; };
#define CHECK(parser, ...)                                                                            \
    do {                                                                                              \
        const row t_[] = {__VA_ARGS__};                                                               \
        for (const row &r_ : t_) expect(#parser, r_.in, (long long)parser(r_.in), r_.want);           \
    } while (0)
#define CHECK_D(parser, ...)                                                                          \
    do {                                                                                              \
        const row_d t_[] = {__VA_ARGS__};                                                             \
        for (const row_d &r_ : t_) expect_d(#parser, r_.in, parser(r_.in), r_.want);                  \
    } while (0)
#define U nullptr

int main() {
    // ---- booleans: on unless the value begins with '0'
    struct { const char *name; bool (*parse)(const char *); } leading0[] = {
        {"parse_coalesce", parse_coalesce}, {"parse_upload_ramp", parse_upload_ramp}, {"parse_lincomb_promote", parse_lincomb_promote},
        {"parse_stream_cache", parse_stream_cache}, {"parse_g1_direct_coop", parse_g1_direct_coop}, {"parse_coop_inv", parse_coop_inv},
        {"parse_fk20_pass1", parse_fk20_pass1}, {"parse_fk20_fuse", parse_fk20_fuse}, {"parse_fk20_pad", parse_fk20_pad}};
    const row leading0_rows[] = {{U, 1}, {"", 1}, {"0", 0}, {"00", 0}, {"0x", 0}, {"0.5", 0}, {"01", 0}, {"1", 1}, {"2", 1}, {"-1", 1}, {"-0", 1}, {" 0", 1}, {"off", 1}, {"false", 1}, {"no", 1}};
    for (auto &k : leading0) for (const row &r : leading0_rows) expect(k.name, r.in, k.parse(r.in), r.want);
    // ... KZG_HIP_FB_GLV: off for exactly "0"
    CHECK(parse_fb_glv, {U, 1}, {"", 1}, {"0", 0}, {"00", 1}, {"0x", 1}, {"0.5", 1}, {"01", 1}, {"1", 1}, {"2", 1}, {"-1", 1}, {" 0", 1}, {"0 ", 1}, {"off", 1});
    // ... on when set at all
    CHECK(parse_coalesce_trace, {U, 0}, {"", 1}, {"0", 1}, {"1", 1}, {"off", 1});
    CHECK(parse_coalesce_stats, {U, 0}, {"", 1}, {"0", 1}, {"1", 1}, {"off", 1});
    // ... one exact word
    CHECK(parse_eth_quotient_one, {U, 0}, {"", 0}, {"one", 1}, {"One", 0}, {"on", 0}, {"one ", 0}, {"ones", 0}, {"1", 0}, {"0", 0});
    CHECK(parse_sha256_portable, {U, 0}, {"", 0}, {"portable", 1}, {"Portable", 0}, {"port", 0}, {"portable1", 0}, {"1", 0}, {"0", 0});

    // ---- modes
    const long long g_size = (long long)g1_fft_mode::by_size, g_direct = (long long)g1_fft_mode::direct, g_radix2 = (long long)g1_fft_mode::radix2;
    CHECK(parse_g1_fft, {U, g_size}, {"", g_radix2}, {"direct", g_direct}, {"d", g_direct}, {"dx", g_direct}, {"Direct", g_radix2}, {"radix2", g_radix2}, {"radix", g_radix2},
          {"0", g_radix2}, {"1", g_radix2}, {"-1", g_radix2});
    CHECK(parse_g1_quad, {U, -1}, {"", 1}, {"0", 0}, {"00", 0}, {"0x", 0}, {"0.5", 0}, {"1", 1}, {"2", 2}, {"20", 2}, {"2x", 2}, {"-1", 1}, {"4", 1}, {"x", 1});
    const long long m_shape = (long long)g1_mul_mode::by_shape, m_reg = (long long)g1_mul_mode::regular, m_wnaf = (long long)g1_mul_mode::wnaf;
    CHECK(parse_g1_mul, {U, m_shape}, {"", m_shape}, {"regular", m_reg}, {"r", m_reg}, {"radix", m_reg}, {"wnaf", m_wnaf}, {"w", m_wnaf}, {"wx", m_wnaf}, {"Regular", m_shape},
          {"Wnaf", m_shape}, {"0", m_shape}, {"1", m_shape}, {"2", m_shape}, {"-1", m_shape});
    const long long f_size = (long long)fr_fft_mode::by_size, f_radix2 = (long long)fr_fft_mode::radix2, f_shared = (long long)fr_fft_mode::shared;
    CHECK(parse_fr_fft, {U, f_size}, {"", f_size}, {"radix2", f_radix2}, {"shared", f_shared}, {"radix", f_size}, {"Radix2", f_size}, {"radix2 ", f_size}, {"radix22", f_size},
          {"share", f_size}, {"Shared", f_size}, {"0", f_size}, {"1", f_size}, {"2", f_size}, {"-1", f_size});
    const long long z_size = (long long)zero_poly_mode::by_size, z_direct = (long long)zero_poly_mode::direct, z_tree = (long long)zero_poly_mode::tree;
    CHECK(parse_zero_poly_once, {U, z_size}, {"", z_size}, {"direct", z_direct}, {"tree", z_tree}, {"Direct", z_size}, {"d", z_size}, {"tre", z_size}, {"trees", z_size}, {"1", z_size}, {"0", z_size});
    CHECK(parse_zero_poly_per_call, {U, z_size}, {"", z_size}, {"direct", z_direct}, {"tree", z_tree}, {"Direct", z_size}, {"d", z_size}, {"tre", z_size}, {"trees", z_size}, {"1", z_size}, {"0", z_size});
    const long long r_batch = (long long)msm_reduce_mode::by_batch, r_scan = (long long)msm_reduce_mode::scan, r_chunks = (long long)msm_reduce_mode::chunks;
    CHECK(parse_msm_reduce, {U, r_batch}, {"", r_batch}, {"chunks", r_chunks}, {"scan", r_scan}, {"chunk", r_batch}, {"Chunks", r_batch}, {"Scan", r_batch}, {"scan2", r_batch}, {"0", r_batch}, {"1", r_batch});
    CHECK(parse_msm_seg, {U, -1}, {"", 0}, {"0", 0}, {"00", 0}, {"0x", 0}, {"1", 1}, {"2", 2}, {"-1", -1}, {"0.5", 0}, {"1.5", 1}, {"x", 0}, {" 1", 1});
    const long long t_count = (long long)transcript_mode::by_count, t_host = (long long)transcript_mode::host, t_device = (long long)transcript_mode::device;
    CHECK(parse_eth_transcript, {U, t_count}, {"", t_count}, {"host", t_host}, {"device", t_device}, {"Host", t_count}, {"dev", t_count}, {"devices", t_count}, {"0", t_count}, {"1", t_count});
    CHECK(parse_multi_fft, {U, -1}, {"", 0}, {"sharded", 1}, {"gather", 0}, {"Sharded", 0}, {"shard", 0}, {"sharded ", 0}, {"1", 0}, {"0", 0});
    const long long x_devs = (long long)transport_mode::by_devices, x_rccl = (long long)transport_mode::rccl, x_host = (long long)transport_mode::host, x_peer = (long long)transport_mode::peer;
    CHECK(parse_multi_transport, {U, x_devs}, {"", x_peer}, {"rccl", x_rccl}, {"host", x_host}, {"peer", x_peer}, {"RCCL", x_peer}, {"rccl ", x_peer}, {"hosts", x_peer}, {"0", x_peer}, {"1", x_peer});
    CHECK(parse_multi_fault, {U, 0}, {"", 0}, {"rccl", FAULT_RCCL}, {"rccl-corrupt", FAULT_RCCL_CORRUPT}, {"peer", FAULT_PEER}, {"peer-corrupt", FAULT_PEER_CORRUPT},
          {"rccl-hang", FAULT_RCCL_HANG}, {"rccl-block", FAULT_RCCL_BLOCK}, {"rccl-init-block", FAULT_RCCL_INIT_BLOCK}, {"peer-hang", FAULT_PEER_HANG},
          {"peer-stuck", FAULT_PEER_HANG | FAULT_PEER_STUCK}, {"rccl,peer", FAULT_RCCL | FAULT_PEER}, {"rccl-hang,rccl", FAULT_RCCL_HANG | FAULT_RCCL},
          {"rccl-corrupt,rccl", FAULT_RCCL_CORRUPT | FAULT_RCCL}, {"peer-corrupt,rccl-block", FAULT_PEER_CORRUPT | FAULT_RCCL_BLOCK}, {"rccl,", FAULT_RCCL}, {",rccl", FAULT_RCCL},
          {"xrccl", 0}, {"rcclx", 0}, {"rccl-", 0}, {"RCCL", 0}, {"rccl peer", 0}, {"rccl, peer", FAULT_RCCL}, {"1", 0}, {"0", 0});
    {
        static const char path[] = "/somewhere/librccl.so";
        checks += 3;
        if (parse_rccl_lib(U) != nullptr) { misses++; printf("MISS parse_rccl_lib(unset) is not null\n"); }
        if (parse_rccl_lib(path) != path) { misses++; printf("MISS parse_rccl_lib is not the identity\n"); }
        if (parse_rccl_lib("") == nullptr) { misses++; printf("MISS parse_rccl_lib(\"\") is null\n"); }   // (the binder skips an empty name itself)
    }

    // ---- numbers
    CHECK(parse_lincomb_promote_after, {U, 2}, {"", 1}, {"0", 1}, {"00", 1}, {"1", 1}, {"2", 2}, {"3", 3}, {"-1", 1}, {"0.5", 1}, {"7x", 7}, {"x", 1}, {"1000", 1000}, {"1001", 1000}, {"999999999999", 1000},
          {"-999999999999", 1});
    CHECK(parse_fb_lanes, {U, 0}, {"", 0}, {"0", 0}, {"1", 1}, {"2", 2}, {"65536", 65536}, {"131072", 131072}, {"0.5", 0}, {"12x", 12}, {"0x10", 0}, {"x", 0}, {"-1", -1});   // strtoull: "-1" is 2^64 - 1
    CHECK(parse_eth_stage_rows, {U, 0}, {"", 0}, {"0", 0}, {"1", 1}, {"2", 2}, {"4", 4}, {"0.5", 0}, {"4x", 4}, {"x", 0}, {"-1", -1});                                          // atol, then uint64_t: every batch is staged
    CHECK_D(parse_eth_verify_chunk_mb, {U, 4096.0}, {"", 4096.0}, {"0", 4096.0}, {"-1", 4096.0}, {"x", 4096.0}, {"0.5", 0.5}, {"1", 1.0}, {"2", 2.0}, {"0.046875", 0.046875}, {"1e3", 1000.0}, {"8192", 8192.0}, {"2x", 2.0});
    CHECK_D(parse_recover_chunk_mb, {U, 2048.0}, {"", 2048.0}, {"0", 2048.0}, {"-1", 2048.0}, {"x", 2048.0}, {"0.5", 0.5}, {"1", 1.0}, {"2", 2.0}, {"0.75", 0.75}, {"1e3", 1000.0}, {"8192", 8192.0}, {"2x", 2.0});
    struct { const char *name; opt_gb (*parse)(const char *); } budgets[] = {
        {"parse_fb_budget_gb", parse_fb_budget_gb}, {"parse_points_fb_budget_gb", parse_points_fb_budget_gb}, {"parse_fk20_fb_budget_gb", parse_fk20_fb_budget_gb}};
    const row_d budget_rows[] = {{"", 0.0}, {"0", 0.0}, {"1", 1.0}, {"2", 2.0}, {"0.5", 0.5}, {"-1", -1.0}, {"110", 110.0}, {"1e3", 1000.0}, {"x", 0.0}, {"12x", 12.0}};   // no clamp: negative stays negative
    for (auto &k : budgets) {
        expect(k.name, U, k.parse(U).set, 0);
        for (const row_d &r : budget_rows) { expect(k.name, r.in, k.parse(r.in).set, 1); expect_d(k.name, r.in, k.parse(r.in).gb, r.want); }
    }
    CHECK(parse_multi_probe_timeout_ms, {U, 10000}, {"", 10000}, {"0", 10000}, {"1", 10000}, {"2", 10000}, {"9", 10000}, {"10", 10}, {"250", 250}, {"600000", 600000}, {"600001", 10000}, {"-1", 10000},
          {"0.5", 10000}, {"10.9", 10}, {"x", 10000}, {"999999999999", 10000});
    CHECK(parse_coalesce_us, {U, 150}, {"", 0}, {"0", 0}, {"1", 1}, {"2", 2}, {"1000", 1000}, {"3000", 3000}, {"-1", -1}, {"0.5", 0}, {"x", 0});
    CHECK(parse_coalesce_spin_us, {U, 40}, {"", 0}, {"0", 0}, {"1", 1}, {"2", 2}, {"1000", 1000}, {"-1", -1}, {"0.5", 0}, {"x", 0});
    CHECK(parse_coalesce_sim_max_bufs, {U, INT_MAX}, {"", 0}, {"0", 0}, {"1", 1}, {"2", 2}, {"-1", -1}, {"0.5", 0}, {"x", 0});
    // the coalescer's own default (3) and bound (its 4 buffers less one); the pipelines' defaults (96, 48 for FK20)
#define parse_exec_3_3(e) parse_coalesce_exec(e, 3, 3)
#define parse_per_batch_96(e) parse_coalesce_per_batch(e, 96)
#define parse_per_batch_48(e) parse_coalesce_per_batch(e, 48)
    CHECK(parse_exec_3_3, {U, 3}, {"", 1}, {"0", 1}, {"1", 1}, {"2", 2}, {"3", 3}, {"4", 3}, {"99", 3}, {"-1", 1}, {"0.5", 1}, {"2x", 2}, {"x", 1});
    CHECK(parse_per_batch_96, {U, 96}, {"", 1}, {"0", 1}, {"1", 1}, {"2", 2}, {"48", 48}, {"1000", 1000}, {"-1", 1}, {"0.5", 1}, {"x", 1});
    CHECK(parse_per_batch_48, {U, 48}, {"", 1}, {"0", 1}, {"96", 96});

    printf("knobs_test: %d checks, %d misses\n", checks, misses);
    return misses ? 1 : 0;
}
