// Host replay of the batched erasure recovery for tests/test_recovery_batch_host.py: the lane bodies of recover_rows.hpp driven the way k_recovery.hip and
// capi_recovery.hip drive them (one loop iteration per lane), with plain O(n^2) transforms in place of the device's.  A stand-alone program: it reads one
// binary file of cases for ONE domain size and prints a line of hex per result row; the test builds it a second time under ASan + UBSan.
//
// file: u64 n | fr expanded[n + 1] | fr reversed[n + 1] | u64 cases | case*
//   case 0 (recovery, one chunk):   u64 0 | u64 rows | u64 tree | u64 shared | fr samples[rows][n] | u8 present[shared ? 1 : rows][n]   -> "R status hex" per row
//   case 1 (zero polynomials):      u64 1 | u64 rows | u64 tree | u64 segs | u64 nm[rows] | u64 list[rows][n]                        -> "Z hex(eval) hex(poly)" per row
//   case 2 (strip division):        u64 2 | u64 total | u64 with_num | fr den[total] | fr num[total]                                   -> "S hex"
//   case 3 (status on given rows):  u64 3 | u64 rows | fr recon[rows][n] | fr samples[rows][n] | u8 present[rows][n]                  -> "R status hex" per row
// All field elements are the C ABI's Montgomery images.
#include "recover_rows.hpp"
#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <vector>

using namespace kzg;

static uint64_t N;
static std::vector<fr> expanded, reversed_;

struct reader {
    std::vector<uint8_t> buf; size_t pos = 0;
    void need(size_t k) const { if (pos + k > buf.size()) { fprintf(stderr, "input file too short\n"); exit(2); } }
    uint64_t u64() { need(8); uint64_t v; memcpy(&v, &buf[pos], 8); pos += 8; return v; }
    std::vector<fr> frs(size_t k) { need(k * sizeof(fr)); std::vector<fr> v(k); if (k) memcpy(v.data(), &buf[pos], k * sizeof(fr)); pos += k * sizeof(fr); return v; }
    std::vector<uint64_t> u64s(size_t k) { need(k * 8); std::vector<uint64_t> v(k); if (k) memcpy(v.data(), &buf[pos], k * 8); pos += k * 8; return v; }
    std::vector<uint8_t> bytes(size_t k) { need(k); std::vector<uint8_t> v(buf.begin() + pos, buf.begin() + pos + k); pos += k; return v; }
};

static void print_hex(const fr *v, size_t k) {
    const uint8_t *b = reinterpret_cast<const uint8_t *>(v);
    for (size_t i = 0; i < k * sizeof(fr); i++) printf("%02x", b[i]);
}

// fr_fft_rows: rows of in_stride values, the first n_in used, zero-extended to m points (m <= N)
static void fft_rows(const fr *in, uint64_t in_stride, uint64_t n_in, fr *out, uint64_t m, uint64_t rows, int inverse) {
    const std::vector<fr> &roots = inverse ? reversed_ : expanded;
    const uint64_t step = N / m;
    const fr scale = inv<FrP>(fr_from_u64(m));
    std::vector<fr> tmp(m);
    for (uint64_t r = 0; r < rows; r++) {
        for (uint64_t k = 0; k < m; k++) {
            fr acc = zero<FrP>();
            for (uint64_t j = 0; j < n_in; j++) acc = add(acc, mul(in[r * in_stride + j], roots[((j * k) % m) * step]));
            tmp[k] = inverse ? mul(acc, scale) : acc;
        }
        for (uint64_t k = 0; k < m; k++) out[r * m + k] = tmp[k];
    }
}
static void mul_table_rows(fr *data, const fr *table, uint64_t n, uint64_t rows) {
    for (uint64_t t = 0; t < n * rows; t++) data[t] = mul(data[t], table[t % n]);
}

// k_rr_scan: 256 lanes per row
static void scan_rows(const uint8_t *present, uint64_t n, uint64_t rows, std::vector<uint64_t> &list, std::vector<uint32_t> &count, std::vector<uint64_t> &nm) {
    list.assign(rows * n, ~0ull); count.assign(rows, 0); nm.assign(rows, 0);
    for (uint64_t row = 0; row < rows; row++) {
        const uint8_t *pr = present + row * n;
        uint32_t cnt[256], mine[256];
        for (uint32_t t = 0; t < 256; t++) { uint64_t lo, hi; rr::piece_bounds(n, 256, t, lo, hi); mine[t] = cnt[t] = rr::piece_count(pr, lo, hi); }
        for (uint32_t t = 1; t < 256; t++) cnt[t] += cnt[t - 1];
        for (uint32_t t = 0; t < 256; t++) { uint64_t lo, hi; rr::piece_bounds(n, 256, t, lo, hi); rr::piece_emit(pr, lo, hi, list.data() + row * n + (cnt[t] - mine[t])); }
        count[row] = cnt[255]; nm[row] = rr::effective_missing(cnt[255], n);
    }
}
// k_zero_eval_direct_rows: a point's chain cut into `segs` pieces on lazy limbs, joined, corrected by the row's constant
static void zero_eval_direct_rows(const uint64_t *list, uint64_t list_stride, const uint64_t *nm, uint32_t segs, uint64_t length, uint64_t rows, fr *eval) {
    const uint64_t stride = N / length;
    for (uint64_t row = 0; row < rows; row++) {
        const fr corr = rr::lazy_chain_correction(nm[row], segs);
        const uint64_t per = (nm[row] + segs - 1) / segs;
        for (uint64_t k = 0; k < length; k++) {
            const frl x = frl_unpack(expanded[k * stride]);
            frl total = frl_unpack(one<FrP>());
            for (uint32_t seg = 0; seg < segs; seg++) {
                const uint64_t lo = seg * per, hi = lo + per < nm[row] ? lo + per : nm[row];
                frl acc = frl_unpack(one<FrP>());
                for (uint64_t i = lo; i < hi; i++) acc = frl_mul(frl_sub<2>(x, frl_unpack(expanded[list[row * list_stride + i] * stride])), acc);
                total = seg ? frl_mul(acc, total) : acc;
            }
            eval[row * length + k] = frl_canon_lt2r(frl_mul(total, frl_const_from_kilic(corr)));
        }
    }
}
// zero_poly_rows of capi_recovery.hip
static void zero_poly_rows(const uint64_t *list, uint64_t list_stride, const uint64_t *nm, uint64_t max_nm, bool tree, uint32_t segs, uint64_t length, uint64_t rows, fr *eval,
                           fr *poly) {
    if (!tree) {
        zero_eval_direct_rows(list, list_stride, nm, segs, length, rows, eval);
        fft_rows(eval, length, length, poly, length, rows, 1);
        return;
    }
    const uint64_t leaves = rr::shared_leaves(max_nm), dtot = leaves * rr::LEAF;
    std::vector<fr> cur(rows * dtot), nxt(rows * dtot), f(2 * rows * dtot), g(rows * dtot);
    for (uint64_t t = 0; t < rows * leaves; t++) {                         // k_rr_leaves: a lane per (row, leaf)
        fr c[rr::LEAF + 1];
        const uint64_t row = t / leaves, leaf = t - row * leaves;
        rr::leaf_product(expanded.data(), N / length, list + row * list_stride, nm[row], leaf, c, 1, cur.data() + t * rr::LEAF);
    }
    for (uint64_t d = rr::LEAF, nodes = leaves; nodes > 1; d <<= 1, nodes >>= 1) {
        const uint64_t pairs = rows * nodes / 2;
        fft_rows(cur.data(), d, d, f.data(), 2 * d, rows * nodes, 0);
        for (uint64_t t = 0; t < 2 * d * pairs; t++) { const uint64_t p = t / (2 * d), k = t - p * 2 * d; g[t] = mul(f[2 * p * 2 * d + k], f[(2 * p + 1) * 2 * d + k]); }   // k_zero_pair_products
        fft_rows(g.data(), 2 * d, 2 * d, nxt.data(), 2 * d, pairs, 1);
        for (uint64_t t = 0; t < 2 * d * pairs; t++) {                     // k_zero_join
            const uint64_t p = t / (2 * d), k = t - p * 2 * d;
            if (k >= d) nxt[t] = add(nxt[t], add(cur[2 * p * d + k - d], cur[(2 * p + 1) * d + k - d]));
        }
        std::swap(cur, nxt);
    }
    for (uint64_t t = 0; t < rows * length; t++) {                         // k_rr_unpad
        const uint64_t row = t / length, i = t - row * length;
        poly[t] = rr::unpad_coeff(cur.data() + row * dtot, rr::row_pad(leaves, nm[row]), nm[row], i);
    }
    fft_rows(poly, length, length, eval, length, rows, 0);
}
static void strip_divide_all(const fr *num, const fr *den, fr *out, uint64_t total) {   // k_rr_strip_divide: a lane per column
    const uint64_t L = rr::strip_lanes(total);
    for (uint64_t c = 0; c < L; c++) rr::strip_divide(num, den, out, c, L, total);
}
static void finish_rows(const fr *recon, const fr *samples, const uint8_t *present, uint64_t p_stride, const uint32_t *count, uint64_t c_stride, uint64_t n, uint64_t rows) {
    std::vector<uint32_t> flag(rows, 0);
    std::vector<fr> out(n * rows);
    std::vector<uint8_t> status(rows, 0xff);
    for (uint64_t t = 0; t < n * rows; t++) {                              // k_rr_check
        const uint64_t row = t / n, i = t - row * n;
        if (rr::sample_differs(present[row * p_stride + i], recon[t], samples[t])) flag[row] |= 1u;
    }
    for (uint64_t t = 0; t < n * rows; t++) {                              // k_rr_emit
        const uint64_t row = t / n, i = t - row * n, cnt = count[row * c_stride];
        const uint8_t st = rr::row_status(cnt, n, flag[row] != 0);
        out[t] = rr::row_output(st, cnt, samples[t], recon[t]);
        if (i == 0) status[row] = st;
    }
    for (uint64_t r = 0; r < rows; r++) { printf("R %u ", (unsigned)status[r]); print_hex(out.data() + r * n, n); printf("\n"); }
}
// recover_rows_chunk of capi_recovery.hip
static void recover_chunk(const fr *samples, const uint8_t *present, bool shared, bool tree, uint64_t rows) {
    const uint64_t n = N, zrows = shared ? 1 : rows, zs = shared ? 0 : n;
    std::vector<uint64_t> list, nm; std::vector<uint32_t> count;
    scan_rows(present, n, zrows, list, count, nm);
    uint64_t max_nm = 0;
    for (uint64_t v : nm) max_nm = v > max_nm ? v : max_nm;
    std::vector<fr> pw(2 * n), ze(zrows * n), zp(zrows * n), a(rows * n), b(rows * n), c(zrows * n), x(n);
    const fr five = fr_from_u64(5), inv5 = inv<FrP>(five);
    pw[0] = pw[n] = one<FrP>();
    for (uint64_t i = 1; i < n; i++) { pw[i] = mul(pw[i - 1], inv5); pw[n + i] = mul(pw[n + i - 1], five); }
    zero_poly_rows(list.data(), n, nm.data(), max_nm, tree, max_nm >= 4 ? 2 : 1, n, zrows, ze.data(), zp.data());
    for (uint64_t t = 0; t < n * rows; t++) {                              // k_rr_mask_mul
        const uint64_t row = t / n, i = t - row * n;
        a[t] = present[row * zs + i] ? mul(samples[t], ze[row * zs + i]) : zero<FrP>();
    }
    fft_rows(a.data(), n, n, b.data(), n, rows, 1);
    mul_table_rows(b.data(), pw.data(), n, rows);
    mul_table_rows(zp.data(), pw.data(), n, zrows);
    fft_rows(b.data(), n, n, a.data(), n, rows, 0);
    fft_rows(zp.data(), n, n, c.data(), n, zrows, 0);
    fr *res = b.data(), *tmp = a.data();
    if (shared) {
        strip_divide_all(nullptr, c.data(), x.data(), n);
        mul_table_rows(a.data(), x.data(), n, rows);
        res = a.data(); tmp = b.data();
    } else strip_divide_all(a.data(), c.data(), b.data(), rows * n);
    fft_rows(res, n, n, tmp, n, rows, 1);
    mul_table_rows(tmp, pw.data() + n, n, rows);
    fft_rows(tmp, n, n, res, n, rows, 0);
    finish_rows(res, samples, present, zs, count.data(), shared ? 0 : 1, n, rows);
}

int main(int argc, char **argv) {
    if (argc != 2) { fprintf(stderr, "usage: %s cases.bin\n", argv[0]); return 2; }
    reader in;
    FILE *fp = fopen(argv[1], "rb");
    if (!fp) { perror(argv[1]); return 2; }
    uint8_t chunk[65536];
    for (size_t k; (k = fread(chunk, 1, sizeof chunk, fp)) > 0;) in.buf.insert(in.buf.end(), chunk, chunk + k);
    fclose(fp);
    N = in.u64();
    if (N == 0 || (N & (N - 1)) || N > 4096) { fprintf(stderr, "bad domain size\n"); return 2; }
    expanded = in.frs(N + 1); reversed_ = in.frs(N + 1);
    const uint64_t cases = in.u64();
    for (uint64_t ci = 0; ci < cases; ci++) {
        const uint64_t kind = in.u64();
        if (kind == 0) {
            const uint64_t rows = in.u64(), tree = in.u64(), shared = in.u64();
            const std::vector<fr> samples = in.frs(rows * N);
            const std::vector<uint8_t> present = in.bytes((shared ? 1 : rows) * N);
            recover_chunk(samples.data(), present.data(), shared != 0, tree != 0, rows);
        } else if (kind == 1) {
            const uint64_t rows = in.u64(), tree = in.u64(), segs = in.u64();
            const std::vector<uint64_t> nm = in.u64s(rows), list = in.u64s(rows * N);
            uint64_t max_nm = 0;
            for (uint64_t r = 0; r < rows; r++) {
                if (nm[r] >= N) { fprintf(stderr, "erasure list too long\n"); return 2; }
                for (uint64_t i = 0; i < nm[r]; i++) if (list[r * N + i] >= N) { fprintf(stderr, "index out of range\n"); return 2; }
                max_nm = nm[r] > max_nm ? nm[r] : max_nm;
            }
            std::vector<fr> ev(rows * N), zp(rows * N);
            zero_poly_rows(list.data(), N, nm.data(), max_nm, tree != 0, (uint32_t)segs, N, rows, ev.data(), zp.data());
            for (uint64_t r = 0; r < rows; r++) { printf("Z "); print_hex(ev.data() + r * N, N); printf(" "); print_hex(zp.data() + r * N, N); printf("\n"); }
        } else if (kind == 2) {
            const uint64_t total = in.u64(), with_num = in.u64();
            const std::vector<fr> den = in.frs(total), num = in.frs(total);
            std::vector<fr> out(total);
            strip_divide_all(with_num ? num.data() : nullptr, den.data(), out.data(), total);
            printf("S "); print_hex(out.data(), total); printf("\n");
        } else if (kind == 3) {
            const uint64_t rows = in.u64();
            const std::vector<fr> recon = in.frs(rows * N), samples = in.frs(rows * N);
            const std::vector<uint8_t> present = in.bytes(rows * N);
            std::vector<uint64_t> list, nm; std::vector<uint32_t> count;
            scan_rows(present.data(), N, rows, list, count, nm);
            finish_rows(recon.data(), samples.data(), present.data(), N, count.data(), 1, N, rows);
        } else { fprintf(stderr, "unknown case %llu\n", (unsigned long long)kind); return 2; }
    }
    return 0;
}
