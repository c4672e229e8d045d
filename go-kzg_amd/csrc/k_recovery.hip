// k_recovery.hip -- batched erasure recovery: the kernels that carry a row dimension.  Lane bodies: recover_rows.hpp.
// Transforms, table multiplies and the pair / join kernels of the product tree are the lone path's (k_fr.hip), launched over rows x nodes.
#include "internal.hpp"
#include "recover_rows.hpp"

namespace kzg {

static_assert(rr::LEAF == ZERO_TREE_LEAF, "one leaf size for the lone and the batched tree");

// one workgroup per mask row: list[row] = ascending indices of its missing samples, count[row] = how many, nm[row] = the effective count
__global__ void __launch_bounds__(256) k_rr_scan(const uint8_t *present, uint64_t n, uint64_t *list, uint32_t *count, uint64_t *nm) {
    __shared__ uint32_t cnt[256];
    const uint32_t t = threadIdx.x;
    const uint64_t row = blockIdx.x;
    const uint8_t *pr = present + row * n;
    uint64_t lo, hi;
    rr::piece_bounds(n, 256, t, lo, hi);
    const uint32_t mine = rr::piece_count(pr, lo, hi);
    cnt[t] = mine;
    __syncthreads();
    for (uint32_t off = 1; off < 256; off <<= 1) {        // inclusive scan
        const uint32_t v = t >= off ? cnt[t - off] : 0u;
        __syncthreads();
        cnt[t] += v;
        __syncthreads();
    }
    rr::piece_emit(pr, lo, hi, list + row * n + (cnt[t] - mine));
    if (t == 255) { count[row] = cnt[255]; nm[row] = rr::effective_missing(cnt[255], n); }
}
void launch_rr_scan(hipStream_t s, const uint8_t *present, uint64_t n, uint64_t rows, uint64_t *list, uint32_t *count, uint64_t *nm) {
    if (!rows) return;
    hipLaunchKernelGGL(k_rr_scan, dim3((uint32_t)rows), dim3(256), 0, s, present, n, list, count, nm);
}

__global__ void k_rr_corr(const uint64_t *nm, uint64_t rows, uint32_t segs, fr *corr) {
    const uint64_t t = blockIdx.x * (uint64_t)blockDim.x + threadIdx.x;
    if (t < rows) corr[t] = rr::lazy_chain_correction(nm[t], segs);
}
void launch_rr_corr(hipStream_t s, const uint64_t *nm, uint64_t rows, uint32_t segs, fr *corr) {
    if (!rows) return;
    hipLaunchKernelGGL(k_rr_corr, dim3((uint32_t)((rows + 63) / 64)), dim3(64), 0, s, nm, rows, segs, corr);
}

// the two bases of ShiftPoly / UnshiftPoly (recover_from_samples.go:9-40) into device memory without a copy from the host: out = {5^-1, 5}
__global__ void k_rr_shift_bases(fr inv5, fr five, fr *out) { if (threadIdx.x == 0) { out[0] = inv5; out[1] = five; } }
void launch_rr_shift_bases(hipStream_t s, const fr &inv5, const fr &five, fr *out) { hipLaunchKernelGGL(k_rr_shift_bases, dim3(1), dim3(64), 0, s, inv5, five, out); }

// leaves of every row's tree: a lane per (row, leaf); a[row][leaf][16]
__global__ void __launch_bounds__(64) k_rr_leaves(const fr *expanded, uint64_t stride, const uint64_t *list, uint64_t list_stride, const uint64_t *nm, uint64_t leaves,
                                                  uint64_t total, fr *a) {
    __shared__ fr c[rr::LEAF + 1][64];                                    // running product, coefficient-major: lane-contiguous rows
    const uint32_t lane = threadIdx.x;
    const uint64_t t = blockIdx.x * 64ull + lane;
    if (t >= total) return;
    const uint64_t row = t / leaves, leaf = t - row * leaves;
    rr::leaf_product(expanded, stride, list + row * list_stride, nm[row], leaf, &c[0][lane], 64, a + t * rr::LEAF);
}
void launch_rr_leaves(hipStream_t s, const fr *expanded, uint64_t stride, const uint64_t *list, uint64_t list_stride, const uint64_t *nm, uint64_t leaves, uint64_t rows, fr *a) {
    const uint64_t total = leaves * rows;
    if (!total) return;
    hipLaunchKernelGGL(k_rr_leaves, dim3((uint32_t)((total + 63) / 64)), dim3(64), 0, s, expanded, stride, list, list_stride, nm, leaves, total, a);
}
// poly[row] = root[row] / x^pad[row] (roots: rows of leaves * 16 coefficients)
__global__ void k_rr_unpad(const fr *root, uint64_t leaves, const uint64_t *nm, uint64_t length, uint64_t total, fr *poly) {
    const uint64_t t = blockIdx.x * (uint64_t)blockDim.x + threadIdx.x;
    if (t >= total) return;
    const uint64_t row = t / length, i = t - row * length, m = nm[row];
    poly[t] = rr::unpad_coeff(root + row * leaves * rr::LEAF, rr::row_pad(leaves, m), m, i);
}
void launch_rr_unpad(hipStream_t s, const fr *root, uint64_t leaves, const uint64_t *nm, uint64_t length, uint64_t rows, fr *poly) {
    const uint64_t total = length * rows;
    if (!total) return;
    hipLaunchKernelGGL(k_rr_unpad, dim3((uint32_t)((total + 255) / 256)), dim3(256), 0, s, root, leaves, nm, length, total, poly);
}

// out[row][i] = present[row][i] ? a[row][i] * b[row][i] : 0 (recover_from_samples.go:66-73); b and present with a row stride of their own (0: one shared row)
__global__ void k_rr_mask_mul(const fr *a, const fr *b, uint64_t b_stride, const uint8_t *present, uint64_t p_stride, uint64_t n, uint64_t total, fr *out) {
    const uint64_t t = blockIdx.x * (uint64_t)blockDim.x + threadIdx.x;
    if (t >= total) return;
    const uint64_t row = t / n, i = t - row * n;
    out[t] = present[row * p_stride + i] ? mul(a[t], b[row * b_stride + i]) : zero<FrP>();
}
void launch_rr_mask_mul(hipStream_t s, const fr *a, const fr *b, uint64_t b_stride, const uint8_t *present, uint64_t p_stride, uint64_t n, uint64_t rows, fr *out) {
    const uint64_t total = n * rows;
    if (!total) return;
    hipLaunchKernelGGL(k_rr_mask_mul, dim3((uint32_t)((total + 255) / 256)), dim3(256), 0, s, a, b, b_stride, present, p_stride, n, total, out);
}

// the division (recover_from_samples.go:93-96) with one inversion per 64 denominators; num == null: the inverses themselves
__global__ void __launch_bounds__(64) k_rr_strip_divide(const fr *num, const fr *den, fr *out, uint64_t L, uint64_t total) {
    const uint64_t c = blockIdx.x * 64ull + threadIdx.x;
    if (c < L) rr::strip_divide(num, den, out, c, L, total);
}
void launch_rr_strip_divide(hipStream_t s, const fr *num, const fr *den, fr *out, uint64_t total) {
    if (!total) return;
    const uint64_t L = rr::strip_lanes(total);
    hipLaunchKernelGGL(k_rr_strip_divide, dim3((uint32_t)((L + 63) / 64)), dim3(64), 0, s, num, den, out, L, total);
}

// flag[row] |= a present sample differs from the reconstruction (:103-107)
__global__ void k_rr_check(const fr *recon, const fr *samples, const uint8_t *present, uint64_t p_stride, uint64_t n, uint64_t total, uint32_t *flag) {
    const uint64_t t = blockIdx.x * (uint64_t)blockDim.x + threadIdx.x;
    if (t >= total) return;
    const uint64_t row = t / n, i = t - row * n;
    if (rr::sample_differs(present[row * p_stride + i], recon[t], samples[t])) atomicOr(&flag[row], 1u);
}
// the row's status byte and its output: the reconstruction, the samples themselves (nothing missing) or zeros (failed).  out may be recon.
__global__ void k_rr_emit(const fr *recon, const fr *samples, const uint32_t *count, uint64_t c_stride, const uint32_t *flag, uint64_t n, uint64_t total, fr *out,
                          uint8_t *status) {
    const uint64_t t = blockIdx.x * (uint64_t)blockDim.x + threadIdx.x;
    if (t >= total) return;
    const uint64_t row = t / n, i = t - row * n, cnt = count[row * c_stride];
    const uint8_t st = rr::row_status(cnt, n, flag && flag[row] != 0);
    out[t] = rr::row_output(st, cnt, samples[t], recon ? recon[t] : samples[t]);
    if (i == 0) status[row] = st;
}
void launch_rr_finish(hipStream_t s, const fr *recon, const fr *samples, const uint8_t *present, uint64_t p_stride, const uint32_t *count, uint64_t c_stride, uint32_t *flag,
                      uint64_t n, uint64_t rows, fr *out, uint8_t *status) {
    const uint64_t total = n * rows;
    if (!total) return;
    const dim3 grid((uint32_t)((total + 255) / 256));
    if (recon) hipLaunchKernelGGL(k_rr_check, grid, dim3(256), 0, s, recon, samples, present, p_stride, n, total, flag);
    hipLaunchKernelGGL(k_rr_emit, grid, dim3(256), 0, s, recon, samples, count, c_stride, recon ? flag : nullptr, n, total, out, status);
}

}  // namespace kzg
