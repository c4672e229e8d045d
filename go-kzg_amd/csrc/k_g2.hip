// k_g2.hip -- the G2 half of a setup, one lane per point: the fixed-base table of bls.GenG2, the walk over it, normalisation to the API's Kilic
// image and ZCash compression (g2.hpp).  Replaces the bls.MulG2(&out, &bls.GenG2, &s) loops of GenerateTestingSetup (setup.go:17-24),
// kzg_single_proofs.go:60, kzg_multi_proofs.go:69 and eth/helpers.go:57, and bls.ToCompressedG2 (bls/bls_kilic.go:123-125).
#include "internal.hpp"
#include "g2.hpp"

namespace kzg {

// One wavefront per workgroup, as the verification kernels: a lane holds a Jacobian accumulator (72 dwords), a table entry (48) and the operands
// of the out-of-line F_p2 products, so the kernels are register-bound whatever the block size, and 64-lane groups put the 1024 wavefronts of a
// 65 536-point setup on 1024 SIMDs.  Register, scratch and occupancy figures: profiles/g2_setup.md.
#define G2_BLOCK 64
static inline dim3 g2_grid(uint64_t n) { return dim3((uint32_t)((n + G2_BLOCK - 1) / G2_BLOCK)); }

// table[w * 256 + d] = [d 2^(8 w)] G2, affine (g2.hpp): the window base by 8 w doublings (the 64 lanes of a wavefront share w, so the loop is
// uniform), [d] base by an 8-bit double-and-add, one inversion for the affine form
__global__ __launch_bounds__(G2_BLOCK) void k_g2_fixed_base_table(g2a *table) {
    const uint32_t t = blockIdx.x * blockDim.x + threadIdx.x;
    if (t >= G2_FB_ENTRIES) return;
    table[t] = g2_fb_entry(g2_fb_window_base((int)(t / G2_FB_ROW)), t % G2_FB_ROW);
}
void launch_g2_fixed_base_table(hipStream_t s, g2a *table) {
    hipLaunchKernelGGL(k_g2_fixed_base_table, g2_grid(G2_FB_ENTRIES), dim3(G2_BLOCK), 0, s, table);
}

// out[i] = [scalars[i]] G2 (device-internal Jacobian image): 32 mixed additions over the table, no doubling (g2_fb_mul)
__global__ __launch_bounds__(G2_BLOCK) void k_g2_fixed_base(const fr *scalars, uint64_t n, const g2a *table, g2j *out) {
    const uint64_t t = blockIdx.x * (uint64_t)blockDim.x + threadIdx.x;
    if (t >= n) return;
    out[t] = g2_fb_mul(table, scalars[t]);
}
void launch_g2_fixed_base(hipStream_t s, const fr *scalars, uint64_t n, const g2a *table, g2j *out) {
    if (!n) return;
    hipLaunchKernelGGL(k_g2_fixed_base, g2_grid(n), dim3(G2_BLOCK), 0, s, scalars, n, table, out);
}

// device-internal Jacobian images -> Kilic images with Z = 1, infinity as (0, 1, 0); one F_p2 inversion per lane
__global__ __launch_bounds__(G2_BLOCK) void k_g2_normalize(const g2j *in, uint64_t n, g2j *out_kilic) {
    const uint64_t t = blockIdx.x * (uint64_t)blockDim.x + threadIdx.x;
    if (t >= n) return;
    out_kilic[t] = g2_normalize_to_kilic(in[t]);
}
void launch_g2_normalize(hipStream_t s, const g2j *in, uint64_t n, g2j *out_kilic) {
    if (!n) return;
    hipLaunchKernelGGL(k_g2_normalize, g2_grid(n), dim3(G2_BLOCK), 0, s, in, n, out_kilic);
}

// Kilic images (any Z) -> 96-byte ZCash encodings
__global__ __launch_bounds__(G2_BLOCK) void k_g2_compress(const g2j *in_kilic, uint64_t n, uint8_t *out96) {
    const uint64_t t = blockIdx.x * (uint64_t)blockDim.x + threadIdx.x;
    if (t >= n) return;
    g2_compress(out96 + 96 * t, g2_from_kilic(in_kilic[t]));
}
void launch_g2_compress(hipStream_t s, const g2j *in_kilic, uint64_t n, uint8_t *out96) {
    if (!n) return;
    hipLaunchKernelGGL(k_g2_compress, g2_grid(n), dim3(G2_BLOCK), 0, s, in_kilic, n, out96);
}

}  // namespace kzg
