// k_verify_combine_multi.hip -- batches of KZG MULTI-proof checks by random linear combination per group of consecutive rows (lane bodies and
// layout: verify_combine_multi.hpp): the term scalars of every group's two MSMs and the group's combined interpolation polynomial J_g, the
// scalars of the one MSM over the setup that replaces a commitment per row.  Behind kzg_hip_check_proof_multi_batch_combined (capi_verify.hip);
// the points, the MSMs, the negation and the group checks are those of the single form (k_verify_combine.hip).
#include "internal.hpp"
#include "coop_inv.hpp"
#include "verify_combine_multi.hpp"

namespace kzg {

static_assert(COMBINE_MULTI_TILE == 256, "block_batch_inverse<FrP, 8> and the sweep below are written for 256 lanes");

// One workgroup per (tile of 256 consecutive rows, group).  coef: the inverse transform of the chunk's rows, np coefficients per row.
// Phase A, lane = row: the weight (one SHA-256 block), x^-1 of the whole tile by ONE cooperative inversion (a product tree in LDS), x^np; r and
// r x^np go to the group's slice of sc, r and x^-1 stay in LDS.  Phase B, lane = coefficient index j = lane mod np: np steps over the tile's
// 256 np contiguous coefficients, 256 consecutive elements per step; a lane forms r x^-j of the element's row from LDS, multiplies and keeps
// its own sum.  The 256 / np lanes of a j are then summed through LDS and the np sums go to the tile's partials.  No atomics; F_r addition is
// exact, so J_g does not depend on how rows fall into tiles.  LDS: 16 KB tree + 16 KB per-row values + 8 KB sums.
__global__ __launch_bounds__(COMBINE_MULTI_TILE) void k_combine_multi_poly(combine_seed seed, const fr *xs, const fr *coef, uint64_t np, uint64_t row0, uint64_t count,
                                                                           uint64_t R, fr *sc, fr *partials) {
    __shared__ fr tree[2 * COMBINE_MULTI_TILE], s_r[COMBINE_MULTI_TILE], s_base[COMBINE_MULTI_TILE], part[COMBINE_MULTI_TILE];
    const uint32_t tid = threadIdx.x;
    const uint64_t t = blockIdx.x, g = blockIdx.y;
    const uint64_t first = combine_multi_tile_row(g, t, R);
    {
        const bool live = combine_multi_row_live(t, tid, first, R, count);
        const fr x = live ? xs[first + tid] : zero<FrP>();
        const fr xi = block_batch_inverse<FrP, 8>(combine_multi_inverse_operand(live, x), tree, tid);
        fr r, rxp, base;
        combine_multi_row_scalars(seed, row0 + first + tid, live, x, xi, np, r, rxp, base);
        const uint64_t slot = t * COMBINE_MULTI_TILE + tid;
        if (slot < R) {
            fr *slice = sc + g * combine_term_stride(R);
            slice[slot] = r; slice[R + slot] = rxp;
        }
        s_r[tid] = r; s_base[tid] = base;
    }
    __syncthreads();
    const uint32_t j = combine_multi_lane_coeff(tid, np);
    const fr *tile = coef + first * np;
    fr acc = zero<FrP>();
#pragma nounroll
    for (uint32_t k = 0; k < (uint32_t)np; k++) {
        const uint32_t l = combine_multi_lane_row(tid, k, np);
        if (!combine_multi_row_live(t, l, first, R, count)) break;            // rows grow with k: the tile's remaining rows are dead too
        acc = add(acc, mul(combine_multi_coeff_weight(s_r[l], s_base[l], j), tile[(uint64_t)k * COMBINE_MULTI_TILE + tid]));
    }
    part[tid] = acc;
    __syncthreads();
    for (uint32_t off = COMBINE_MULTI_TILE / 2; off >= np; off >>= 1) {        // np divides off: lanes tid and tid + off hold the same j
        if (tid < off) part[tid] = add(part[tid], part[tid + off]);
        __syncthreads();
    }
    if (tid < np) partials[combine_multi_partial_at(g, t, R, np) + tid] = part[tid];
}

// J[g np + j] = the sum of slot j over the tiles of group g, one lane per (g, j); the lane of j = 0 writes the scalar -1 of [J_g(s)]_1
__global__ __launch_bounds__(COMBINE_MULTI_TILE) void k_combine_multi_fold(const fr *partials, uint64_t np, uint64_t G, uint64_t R, fr *J, fr *sc) {
    const uint64_t i = blockIdx.x * (uint64_t)blockDim.x + threadIdx.x;
    if (i >= G * np) return;
    const uint64_t g = i / np, j = i % np;
    J[i] = combine_multi_fold(partials, g, R, np, j);
    if (j == 0) sc[g * combine_term_stride(R) + 2 * R] = combine_multi_last_scalar();
}

void launch_combine_multi_scalars(hipStream_t s, const combine_seed &seed, const fr *xs, const fr *coef, uint64_t np, uint64_t row0, uint64_t count, uint64_t R, fr *sc,
                                  fr *partials, fr *J) {
    if (!count) return;
    const uint64_t G = combine_group_count(count, R);
    hipLaunchKernelGGL(k_combine_multi_poly, dim3((uint32_t)combine_multi_tiles(R), (uint32_t)G), dim3(COMBINE_MULTI_TILE), 0, s, seed, xs, coef, np, row0, count, R, sc,
                       partials);
    hipLaunchKernelGGL(k_combine_multi_fold, dim3((uint32_t)((G * np + COMBINE_MULTI_TILE - 1) / COMBINE_MULTI_TILE)), dim3(COMBINE_MULTI_TILE), 0, s, partials, np, G, R, J, sc);
}

}  // namespace kzg
