// k_verify_combine.hip -- batches of KZG checks by random linear combination per group of consecutive rows (lane bodies: verify_combine.hpp):
// the term scalars and term points of every group's two MSMs (launch_msm with a per-group slice of points), and the negation in front of the
// group checks (launch_pairing_check).  Behind kzg_hip_check_proof_single_batch_combined / kzg_hip_eth_verify_kzg_proof_batch_combined
// (capi_verify.hip); the per-row kernels of k_pairing.hip stay as they are and re-check the rows of a failing group.
#include "internal.hpp"
#include "verify_combine.hpp"

namespace kzg {

#define COMBINE_BLOCK 256

// One workgroup per group.  A lane takes the group's rows tid, tid + 256, ...: the weight (one SHA-256 block), r x and r y; the term scalars go
// to the group's slice of sc (combine_term_stride(R) slots: r at j, r x at R + j), the r y are summed per lane, then over the workgroup through
// LDS, and lane 0 writes the generator's scalar -sum r y to slot 2 R.  status (nullable): rows with a non-zero byte get weight 0.
// row0: the index in the call of the first row of xs / ys / status (a call runs in chunks of whole groups).
__global__ __launch_bounds__(COMBINE_BLOCK) void k_combine_scalars(combine_seed seed, const fr *xs, const fr *ys, const uint8_t *status, uint64_t row0, uint64_t count,
                                                                   uint64_t R, fr *sc) {
    __shared__ fr part[COMBINE_BLOCK];
    const uint32_t tid = threadIdx.x;
    const uint64_t g = blockIdx.x;
    fr *slice = sc + g * combine_term_stride(R);
    fr u = zero<FrP>();
    for (uint64_t j = tid; j < R; j += COMBINE_BLOCK) {
        const uint64_t t = combine_group_begin(g, R) + j;
        const bool live = t < count && !(status && status[t]);
        fr r, rx, ry;
        combine_row_scalars(seed, row0 + t, live, live ? xs[t] : zero<FrP>(), live ? ys[t] : zero<FrP>(), r, rx, ry);
        slice[j] = r; slice[R + j] = rx;
        u = add(u, ry);
    }
    part[tid] = u;
    __syncthreads();
    for (uint32_t off = COMBINE_BLOCK / 2; off >= 1; off >>= 1) {
        if (tid < off) part[tid] = add(part[tid], part[tid + off]);
        __syncthreads();
    }
    if (tid == 0) slice[2 * R] = combine_generator_scalar(part[0]);
}
void launch_combine_scalars(hipStream_t s, const combine_seed &seed, const fr *xs, const fr *ys, const uint8_t *status, uint64_t row0, uint64_t count, uint64_t R, fr *sc) {
    if (!count) return;
    hipLaunchKernelGGL(k_combine_scalars, dim3((uint32_t)combine_group_count(count, R)), dim3(COMBINE_BLOCK), 0, s, seed, xs, ys, status, row0, count, R, sc);
}

// The term points of every group in the layout of the scalars, as they came in (Kilic images when `kilic`, else device-internal ones): one lane
// per slot.  Slots of rows beyond the count get the point at infinity (their scalar is 0), the last slot of a slice the generator, or the group's
// own point last[g] (in the form of c and pi) when last is not null.
__global__ __launch_bounds__(COMBINE_BLOCK) void k_combine_points(const g1j *c, const g1j *pi, const g1j *last, uint64_t count, uint64_t R, int kilic, uint64_t total,
                                                                  g1j *out) {
    const uint64_t t = blockIdx.x * (uint64_t)blockDim.x + threadIdx.x;
    if (t >= total) return;
    const uint64_t stride = combine_term_stride(R), g = t / stride, j = t % stride;
    g1j p = g1_inf();
    if (j == 2 * R) {
        if (last) { out[t] = last[g]; return; }
        p = g1_generator_internal();
    } else {
        const uint64_t row = combine_group_begin(g, R) + (j < R ? j : j - R);
        if (row < count) { out[t] = j < R ? c[row] : pi[row]; return; }
    }
    out[t] = kilic ? g1_to_kilic(p) : p;
}
void launch_combine_points(hipStream_t s, const g1j *c, const g1j *pi, uint64_t count, uint64_t R, bool kilic, g1j *out, const g1j *last) {
    if (!count) return;
    const uint64_t total = combine_group_count(count, R) * combine_term_stride(R);
    hipLaunchKernelGGL(k_combine_points, dim3((uint32_t)((total + COMBINE_BLOCK - 1) / COMBINE_BLOCK)), dim3(COMBINE_BLOCK), 0, s, c, pi, last, count, R, kilic ? 1 : 0, total, out);
}

// p1[g] = -A_g: the second G1 input of the group check e(B_g, [1]G2) e(-A_g, [s]G2) == 1
__global__ __launch_bounds__(COMBINE_BLOCK) void k_combine_negate(const g1j *a, uint64_t n, g1j *out) {
    const uint64_t t = blockIdx.x * (uint64_t)blockDim.x + threadIdx.x;
    if (t >= n) return;
    out[t] = g1_neg(a[t]);
}
void launch_combine_negate(hipStream_t s, const g1j *a, uint64_t n, g1j *out) {
    if (!n) return;
    hipLaunchKernelGGL(k_combine_negate, dim3((uint32_t)((n + COMBINE_BLOCK - 1) / COMBINE_BLOCK)), dim3(COMBINE_BLOCK), 0, s, a, n, out);
}

// eth form: z and y of every row as Montgomery images and the row's status (eth_combine_fields_lane) from the bytes and the decompression flags
__global__ __launch_bounds__(COMBINE_BLOCK) void k_eth_combine_fields(const uint8_t *zs, const uint8_t *ys, const uint8_t *c_bad, const uint8_t *pi_bad, uint64_t n, fr *z_out,
                                                                      fr *y_out, uint8_t *status) {
    const uint64_t t = blockIdx.x * (uint64_t)blockDim.x + threadIdx.x;
    if (t >= n) return;
    eth_combine_fields_lane(zs + 32 * t, ys + 32 * t, c_bad[t], pi_bad[t], z_out[t], y_out[t], status[t]);
}
void launch_eth_combine_fields(hipStream_t s, const uint8_t *zs, const uint8_t *ys, const uint8_t *c_bad, const uint8_t *pi_bad, uint64_t n, fr *z_out, fr *y_out,
                               uint8_t *status) {
    if (!n) return;
    hipLaunchKernelGGL(k_eth_combine_fields, dim3((uint32_t)((n + COMBINE_BLOCK - 1) / COMBINE_BLOCK)), dim3(COMBINE_BLOCK), 0, s, zs, ys, c_bad, pi_bad, n, z_out, y_out, status);
}

}  // namespace kzg
