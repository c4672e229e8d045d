// k_g1.hip -- G1 kernels, one point per lane: element-wise scalar multiplication, the radix-2 G1 FFT stages,
// normalisation (Jacobian -> Z = R), ZCash (de)compression.  Replaces the loops of fft_g1.go:33-94,
// fk20_single.go:72-74 (ToeplitzPart2), fk20_multi.go:86-89 and bls.To/FromCompressedG1 (bls/bls_kilic.go:114-121).
#define KZG_MULQ_NOINLINE 1   // many mulq call sites in this translation unit: keep the product out of line (I-cache)
#include "internal.hpp"
#include "coop_inv.hpp"

namespace kzg {

// 256 lanes = one wavefront per SIMD of a CU.  With 128-lane workgroups a half-full launch (32 polynomials: 512 workgroups) ran as if
// it were full -- the two wavefronts of consecutive workgroups of a CU landed on the same two SIMDs: 60 ms instead of 37.6 ms per FK20 batch.
#ifndef G1_BLOCK
#define G1_BLOCK 256
#endif

__device__ __forceinline__ uint32_t bitrev32g(uint32_t v, uint32_t bits) { return bits ? (__brev(v) >> (32 - bits)) : 0; }

// k (Montgomery form, as the Go side stores it) * P.  Kilic's MulG1 first leaves Montgomery form (FromRed,
// bls/bls_kilic.go:42-43).  The scalar is split on the device (glv_split_signed) and the product runs the regular odd-digit schedule
// on the affine co-Z table (g1_mul_glv_regular_aq): 128 doublings + 66 mixed additions (round 1: 255 doublings + 64 full additions).
__device__ __forceinline__ g1j g1_mul_fr(const g1j &p, const fr &k_mont) {
    if (is_inf(p)) return g1_inf();
    g1aq tbl[8]; fq dz[7]; g1jq q; g1j packed;
    const int st = g1_mul_glv_regular_aq<false>(g1jq_unpack(p), glv_split_signed(from_mont<FrP>(k_mont)), tbl, dz, q, packed);
    return st == 1 ? g1jq_pack(q) : st == 2 ? packed : g1_inf();
}

__global__ __launch_bounds__(G1_BLOCK, 2) void k_g1_mul_vec(const g1j *pts, uint64_t pts_mod, const fr *scalars, uint64_t s_stride, uint64_t n,
                                                         g1j *out) {
    uint64_t t = blockIdx.x * (uint64_t)blockDim.x + threadIdx.x;
    if (t >= n) return;
    g1j p = pts[t % pts_mod];
    fr k = scalars[t * s_stride];
    out[t] = g1_mul_fr(p, k);
}
void launch_g1_mul_vec(hipStream_t s, const g1j *pts, uint64_t pts_mod, const fr *scalars, uint64_t s_stride, uint64_t n, g1j *out) {
    if (!n) return;
    prof_begin(s, "g1_mul_vec");
    hipLaunchKernelGGL(k_g1_mul_vec, dim3((uint32_t)((n + G1_BLOCK - 1) / G1_BLOCK)), dim3(G1_BLOCK), 0, s, pts, pts_mod, scalars, s_stride, n, out);
    prof_end(s, "g1_mul_vec");
}

// FK20-multi Toeplitz stage (fk20_multi.go:79-91): hExtFFT[j] = sum_f C_f[j] * X_f[j].
// tmp[b][f][jj] = scalars[b][f][j0 + jj] * files[f][j0 + jj], then summed over f.
__global__ __launch_bounds__(G1_BLOCK, 2) void k_g1_file_mul(const g1j *files, const fr *scalars, uint64_t nfiles, uint64_t k2, uint64_t j0, uint64_t cnt,
                                                          uint64_t total, g1j *tmp) {
    uint64_t t = blockIdx.x * (uint64_t)blockDim.x + threadIdx.x;
    if (t >= total) return;
    uint64_t jj = t % cnt, f = (t / cnt) % nfiles, b = t / (cnt * nfiles);
    g1j p = files[f * k2 + j0 + jj];
    fr k = scalars[(b * nfiles + f) * k2 + j0 + jj];
    tmp[t] = g1_mul_fr(p, k);
}
__global__ __launch_bounds__(G1_BLOCK, 2) void k_g1_sum_files(const g1j *tmp, uint64_t nfiles, uint64_t cnt, uint64_t total, g1j *out) {
    uint64_t t = blockIdx.x * (uint64_t)blockDim.x + threadIdx.x;
    if (t >= total) return;
    uint64_t jj = t % cnt, b = t / cnt;
    g1j acc = g1_inf();
    for (uint64_t f = 0; f < nfiles; f++) acc = g1_add(acc, tmp[(b * nfiles + f) * cnt + jj]);
    out[t] = acc;
}
void launch_g1_sum_files(hipStream_t s, const g1j *tmp, uint64_t nfiles, uint64_t cnt, uint64_t batch, g1j *out) {
    uint64_t outs = batch * cnt;
    if (!outs) return;
    hipLaunchKernelGGL(k_g1_sum_files, dim3((uint32_t)((outs + G1_BLOCK - 1) / G1_BLOCK)), dim3(G1_BLOCK), 0, s, tmp, nfiles, cnt, outs, out);
}
hipError_t launch_g1_file_msm(hipStream_t s, const g1j *files, const fr *scalars, uint64_t nfiles, uint64_t k2, uint64_t j0, uint64_t cnt, uint64_t batch,
                              g1j *out) {
    uint64_t total = batch * nfiles * cnt;
    if (!total) return hipSuccess;
    g1j *tmp = nullptr;
    hipError_t e = hipMallocAsync((void **)&tmp, total * sizeof(g1j), s);
    if (e != hipSuccess) return e;
    prof_begin(s, "g1_mul_vec");
    hipLaunchKernelGGL(k_g1_file_mul, dim3((uint32_t)((total + G1_BLOCK - 1) / G1_BLOCK)), dim3(G1_BLOCK), 0, s, files, scalars, nfiles, k2, j0, cnt, total, tmp);
    prof_end(s, "g1_mul_vec");
    uint64_t outs = batch * cnt;
    hipLaunchKernelGGL(k_g1_sum_files, dim3((uint32_t)((outs + G1_BLOCK - 1) / G1_BLOCK)), dim3(G1_BLOCK), 0, s, tmp, nfiles, cnt, outs, out);
    hipFreeAsync(tmp, s);
    return hipGetLastError();
}

__global__ void k_g1_bitrev_copy(const g1j *in, uint64_t in_stride, uint64_t n_valid, g1j *out, uint32_t logn, uint64_t total) {
    uint64_t t = blockIdx.x * (uint64_t)blockDim.x + threadIdx.x;
    if (t >= total) return;
    uint64_t n = 1ull << logn, b = t >> logn, i = t & (n - 1);
    g1j p = (i < n_valid) ? in[b * in_stride + i] : g1_inf();
    out[b * n + bitrev32g((uint32_t)i, logn)] = p;
}
void launch_g1_bitrev_copy(hipStream_t s, const g1j *in, uint64_t in_stride, uint64_t n_valid, g1j *out, uint64_t n, uint64_t batch) {
    uint64_t total = n * batch;
    if (!total) return;
    hipLaunchKernelGGL(k_g1_bitrev_copy, dim3((uint32_t)((total + 255) / 256)), dim3(256), 0, s, in, in_stride, n_valid, out, ilog2(n), total);
}

// One DIT stage with half-size m on bit-reversed data: (x, y) -> (x + w y, x - w y), w = roots[j * W / (2m)].
// This is the butterfly loop of _fftG1 (fft_g1.go:44-55); the recursion's 4-point leaves (simpleFTG1, :11-31) are
// the same linear map, so outputs are identical as group elements.
template <int MODE, bool PRE = false> __global__ __launch_bounds__(G1_BLOCK, 2) void k_g1_fft_stage(g1j *data, uint32_t logn, uint64_t m, const fr *roots, const int8_t *wnaf, uint64_t W, uint64_t total, uint64_t batch) {
    uint64_t t = blockIdx.x * (uint64_t)blockDim.x + threadIdx.x;
    if (t >= total) return;
    // Twiddle-major lane order: t -> (j, b, g).  All lanes of a wavefront then share ONE twiddle, so (i) the waves with j == 0
    // (1/2, 1/4, 1/8 ... of the early stages) skip the scalar multiplication entirely instead of idling beside their
    // neighbours, and (ii) the irregular width-5 NAF digit schedule of g1_mul_glv_wnaf is wave-uniform: no divergence.
    // MODE 4 (default): width-5 NAF on the affine co-Z table, products of the doubling loop and of the additions inlined,
    // (x + w y, x - w y) by the shared lazy formulas; MODE 0: the regular odd-digit schedule on the same table, for launches whose
    // wavefronts straddle many twiddles.  KZG_HIP_G1_MUL = regular / wnaf forces one of them (A/B runs).  Round 1's variants
    // (Jacobian table; every product a call; only the doublings inlined) measured 814 / 865 / 886 / 888 FK20 per second at batch 128
    // against 1014 for round 1's final kernel and ~1240 for this one at batch 512.
    const uint64_t half = 1ull << (logn - 1), groups = half / m;
    const uint64_t j = t / (groups * batch), rem = t % (groups * batch), b = rem / groups, g = rem % groups;
    g1j *row = data + (b << logn);
    uint64_t i0 = g * 2 * m + j, i1 = i0 + m;
    g1j y = row[i1];
    g1j x = row[i0];
    if (MODE == 4) {
        // y <- w y unpacked, then (x + y, x - y) with the shared formulas; anything exceptional (an infinite operand, x == +-y, a
        // degenerate addition inside the product) takes the generic complete path below
        g1jq yq; int st = is_inf(y) ? 0 : 1;
        if (st == 1) {
            if (j) {
                g1aq tbl[8]; fq dz[7]; g1j packed;
                const uint64_t ti = j * (W / (2 * m));                 // twiddle index: GLV pair + its precomputed width-5 NAF digit strings
                if (PRE) st = g1_mul_glv_wnaf_aq_pre_q<true, true>(g1jq_unpack(y), roots[ti], tbl, dz, wnaf + ti * KZG_WNAF_ROW, yq, packed);   // affine table: mixed additions
                else { int8_t dg1[132], dg2[132]; st = g1_mul_glv_wnaf_aq<true, true>(y, roots[ti], tbl, dz, dg1, dg2, 1, yq, packed); }
                if (st == 2) y = packed; else if (st == 0) y = g1_inf();
            } else yq = g1jq_unpack(y);
        }
        if (st == 1 && !is_inf(x)) {
            g1jq sum, dif;
            if (KZG_LIKELY(g1jq_addsub(g1jq_unpack(x), yq, sum, dif))) {
                fp z3 = packq(sum.z);
                g1j o0, o1;
                o0.x = packq(sum.x); o0.y = packq(sum.y); o0.z = z3;
                o1.x = packq(dif.x); o1.y = packq(dif.y); o1.z = z3;
                row[i0] = o0; row[i1] = o1;
                return;
            }
        }
        if (st == 1) y = g1jq_pack(yq);
    } else {
        if (j && !is_inf(y)) {
            const fr kk = roots[j * (W / (2 * m))];          // (k1, k2) GLV pair, both halves non-negative
            glv_halves h;
#pragma unroll
            for (int i = 0; i < 4; i++) { h.k1[i] = kk.l[i]; h.k2[i] = kk.l[4 + i]; }
            h.neg1 = h.neg2 = 0;
            g1aq tbl[8]; fq dz[7]; g1jq q; g1j packed;
            const int st = g1_mul_glv_regular_aq<true>(g1jq_unpack(y), h, tbl, dz, q, packed);
            y = st == 1 ? g1jq_pack(q) : st == 2 ? packed : g1_inf();
        }
    }
    row[i0] = g1_add(x, y);
    row[i1] = g1_add(x, g1_neg(y));
}
// 4 lanes per butterfly while the quadrupled launch still fits one wavefront per SIMD (65 536 lanes on 256 CUs), 2 while the doubled one does;
// KZG_HIP_G1_QUAD = 0 / 1 / 2: never / always four / always two
bool g1_quad_enabled() { return knobs::g1_quad() != 0; }
#ifndef KZG_WNAF_ROWS_MIN
#define KZG_WNAF_ROWS_MIN 512          // lanes per twiddle from which the precomputed rows are used (A/B builds: 0 = always, 1 << 60 = never)
#endif
// The variant of a stage launch (internal.hpp).
//  - lanes per butterfly: 4 while the quadrupled launch still fits one wavefront per SIMD, 2 while the doubled one does, else 1.
//  - schedule.  The width-5 NAF schedule is irregular: it only pays when the lanes of a wavefront share their twiddle.  A twiddle is shared by
//    (n / 2 / m) * batch consecutive butterflies.  One lane each: a multiple of 64 means every wave is uniform; >= 256 means at most a quarter of the
//    waves straddle two twiddles; otherwise (late stages of small batches: a single 4096-point transform has 64 different twiddles per wave in its
//    last stage, measured 21 ms against 2.3 ms) the regular signed-window schedule runs instead.  KZG_HIP_G1_MUL = regular / wnaf forces one of them
//    (A/B runs).  The one-lane DIF stage has the NAF form only.  Several lanes each: NAF where every wavefront holds exactly one twiddle (these
//    kernels read the precomputed rows, which is only right for a wave-uniform twiddle, so "wnaf" cannot force it), else regular.
//  - digit rows.  The twiddles' precomputed width-5 NAF digit strings (264 bytes per twiddle in HBM) replace the per-butterfly recoding only where a
//    row is shared by many lanes (>= 512: measured +2.3 % on the 512-polynomial FK20 step); with one wavefront per twiddle every row is a
//    cold read and the recoding in registers is faster (measured -4 % on 64 transforms when the rows were always used).
g1_stage_plan g1_fft_stage_plan(uint64_t n, uint64_t batch, uint64_t m, bool dif, int quad, knobs::g1_mul_mode mul) {
    const uint64_t butterflies = n / 2 * batch, per_twiddle = (n / 2 / m) * batch, one_round = device_simd_lanes();
    g1_stage_plan p;
    p.lanes = quad >= 0 ? (quad == 0 ? 1 : quad == 2 ? 2 : 4) : butterflies * 4 <= one_round ? 4 : butterflies * 2 <= one_round ? 2 : 1;
    if (p.lanes > 1) {
        p.wnaf = mul != knobs::g1_mul_mode::regular && (per_twiddle * (uint64_t)p.lanes) % 64 == 0;
        p.rows = p.wnaf;
        return p;
    }
    p.wnaf = dif || (mul == knobs::g1_mul_mode::regular ? false : mul == knobs::g1_mul_mode::wnaf ? true : (per_twiddle % 64 == 0 || per_twiddle >= 256));
    p.rows = p.wnaf && per_twiddle >= (uint64_t)KZG_WNAF_ROWS_MIN;
    return p;
}
g1_stage_plan g1_fft_stage_plan(uint64_t n, uint64_t batch, uint64_t m, bool dif) { return g1_fft_stage_plan(n, batch, m, dif, knobs::g1_quad(), knobs::g1_mul()); }
// Decimation-in-frequency form of the same stage: (x, y) -> (x + y, (x - y) w) on the SAME pairs and twiddles (half-size m runs from
// n / 2 down to 1, natural order in, bit-reversed order out).  Used by the FK20 inverse transform whose first two stages are folded
// into the fixed-base Toeplitz stage (k_fb_mul_vec_dif2): the remaining stages continue here and leave h in exactly the bit-reversed
// layout the following forward (decimation-in-time) transform reads, so no reordering pass runs in between.  Same cost per butterfly
// as the DIT form: the shared (x + y, x - y) formulas, then the width-5 NAF multiplication on the unpacked difference.
template <bool PRE> __global__ __launch_bounds__(G1_BLOCK, 2) void k_g1_fft_stage_dif(g1j *data, uint32_t logn, uint64_t m, const fr *roots, const int8_t *wnaf, uint64_t W, uint64_t total, uint64_t batch) {
    uint64_t t = blockIdx.x * (uint64_t)blockDim.x + threadIdx.x;
    if (t >= total) return;
    const uint64_t half = 1ull << (logn - 1), groups = half / m;
    const uint64_t j = t / (groups * batch), rem = t % (groups * batch), b = rem / groups, g = rem % groups;   // twiddle-major, as in the DIT stage
    g1j *row = data + (b << logn);
    uint64_t i0 = g * 2 * m + j, i1 = i0 + m;
    g1j y = row[i1];
    g1j x = row[i0];
    if (!is_inf(x) && !is_inf(y)) {
        g1jq sum, dif;
        if (KZG_LIKELY(g1jq_addsub(g1jq_unpack(x), g1jq_unpack(y), sum, dif))) {
            g1j o0; o0.x = packq(sum.x); o0.y = packq(sum.y); o0.z = packq(sum.z);
            row[i0] = o0;
            if (j) {
                g1aq tbl[8]; fq dz[7]; g1j packed; g1jq dq;
                const uint64_t ti = j * (W / (2 * m));
                int st;
                if (PRE) st = g1_mul_glv_wnaf_aq_pre_q<true, true>(dif, roots[ti], tbl, dz, wnaf + ti * KZG_WNAF_ROW, dq, packed);
                else { int8_t dg1[132], dg2[132]; st = g1_mul_glv_wnaf_aq_q<true, true>(dif, roots[ti], tbl, dz, dg1, dg2, 1, dq, packed); }
                row[i1] = st == 1 ? g1jq_pack(dq) : st == 2 ? packed : g1_inf();
            } else { g1j o1; o1.x = packq(dif.x); o1.y = packq(dif.y); o1.z = o0.z; row[i1] = o1; }
            return;
        }
    }
    // an infinite operand or x == +-y: generic complete formulas
    g1j s_ = g1_add(x, y), d_ = g1_add(x, g1_neg(y));
    if (j && !is_inf(d_)) {
        g1aq tbl[8]; fq dz[7]; g1j packed; g1jq dq;
        const uint64_t ti = j * (W / (2 * m));
        int8_t dg1[132], dg2[132];
        int st = g1_mul_glv_wnaf_aq<true, true>(d_, roots[ti], tbl, dz, dg1, dg2, 1, dq, packed);
        d_ = st == 1 ? g1jq_pack(dq) : st == 2 ? packed : g1_inf();
    }
    row[i0] = s_; row[i1] = d_;
}
void launch_g1_fft_stage_dif(hipStream_t s, g1j *data, uint64_t n, uint64_t batch, uint64_t m, const fr *roots, const int8_t *wnaf, uint64_t W) {
    launch_g1_fft_stage_planned(s, g1_fft_stage_plan(n, batch, m, true), true, data, n, batch, m, roots, wnaf, W);
}
// data[b][i] = inf for every odd i: in bit-reversed order these are the coefficients k >= n / 2, i.e. the "h[:n] || inf" padding of
// fk20_single.go:163-166 between the two transforms
__global__ void k_g1_clear_odd(g1j *data, uint64_t total_pairs) {
    uint64_t t = blockIdx.x * (uint64_t)blockDim.x + threadIdx.x;
    if (t < total_pairs) data[2 * t + 1] = g1_inf();
}
void launch_g1_clear_odd(hipStream_t s, g1j *data, uint64_t n_total) {
    if (n_total < 2) return;
    hipLaunchKernelGGL(k_g1_clear_odd, dim3((uint32_t)((n_total / 2 + 255) / 256)), dim3(256), 0, s, data, n_total / 2);
}
// out[t] = in[2 t]: the even positions of a bit-reversed 2k-point sequence are its first k entries in k-point bit-reversed order (FK20Single
// between its two transforms: h[:k] of the inverse transform feeds a transform of HALF the size, fk20_single.go:128-129)
__global__ void k_g1_take_even(const g1j *in, g1j *out, uint64_t total) {
    uint64_t t = blockIdx.x * (uint64_t)blockDim.x + threadIdx.x;
    if (t < total) out[t] = in[2 * t];
}
void launch_g1_take_even(hipStream_t s, const g1j *in, g1j *out, uint64_t total) {
    if (!total) return;
    hipLaunchKernelGGL(k_g1_take_even, dim3((uint32_t)((total + 255) / 256)), dim3(256), 0, s, in, out, total);
}
void launch_g1_fft_stage(hipStream_t s, g1j *data, uint64_t n, uint64_t batch, uint64_t m, const fr *roots, const int8_t *wnaf, uint64_t W) {
    launch_g1_fft_stage_planned(s, g1_fft_stage_plan(n, batch, m, false), false, data, n, batch, m, roots, wnaf, W);
}
// one stage launch of the variant `plan` names (a plan of g1_fft_stage_plan: the one-lane DIF stage is always NAF)
void launch_g1_fft_stage_planned(hipStream_t s, const g1_stage_plan &plan, bool dif, g1j *data, uint64_t n, uint64_t batch, uint64_t m, const fr *roots, const int8_t *wnaf, uint64_t W) {
    uint64_t total = n / 2 * batch;
    if (!total) return;
    prof_begin(s, "g1_fft_stage");
    if (plan.lanes > 1) {
        if (dif) launch_g1_stage_coop_dif(s, plan.lanes, plan.wnaf, data, n, batch, m, roots, wnaf, W, total);
        else launch_g1_stage_coop_dit(s, plan.lanes, plan.wnaf, data, n, batch, m, roots, wnaf, W, total);
        prof_end(s, "g1_fft_stage");
        return;
    }
    const dim3 grid((uint32_t)((total + G1_BLOCK - 1) / G1_BLOCK)), block(G1_BLOCK);
    const uint32_t logn = ilog2(n);
    if (dif) {
        if (plan.rows) hipLaunchKernelGGL(k_g1_fft_stage_dif<true>, grid, block, 0, s, data, logn, m, roots, wnaf, W, total, batch);
        else hipLaunchKernelGGL(k_g1_fft_stage_dif<false>, grid, block, 0, s, data, logn, m, roots, wnaf, W, total, batch);
    } else if (plan.wnaf) {
        if (plan.rows) hipLaunchKernelGGL((k_g1_fft_stage<4, true>), grid, block, 0, s, data, logn, m, roots, wnaf, W, total, batch);
        else hipLaunchKernelGGL((k_g1_fft_stage<4, false>), grid, block, 0, s, data, logn, m, roots, wnaf, W, total, batch);
    } else hipLaunchKernelGGL(k_g1_fft_stage<0>, grid, block, 0, s, data, logn, m, roots, wnaf, W, total, batch);
    prof_end(s, "g1_fft_stage");
}

// ---------------------------------------------------------------------------------------------------------
// Latency mode of the G1 transform (a lone FFTG1 / DAUsingFK20 call, fft_g1.go:58-94).  A radix-2 stage of one 4096-point transform
// has 2048 butterflies = 32 wavefronts on 1024 SIMDs, and each stage costs the latency of one scalar multiplication (~2 ms): 12
// stages are 22 ms on a GPU that is 97 % idle.  Here the transform runs as Stockham passes of radix R = 16 evaluated DIRECTLY:
//   out[(j / Ns) Ns R + k + u Ns] = sum_{t < R} w^(t (n / (Ns R)) (Ns u + k)) * in[j + t n / R],   k = j mod Ns,
// one lane per (output, term): 16 n lanes per pass, all independent, then a 4-level sum inside each group of 16 lanes.  7.5 times
// the scalar multiplications of the radix-2 network, but only log16(n) sequential ones: 3 passes for n = 4096.  The scalars are
// split on the device (glv_split_signed), so the 1 / n of the inverse transform is folded into the last pass.  Natural order in
// and out (no bit reversal); `in` rows may be zero-padded (index >= n_valid -> inf).
// ---------------------------------------------------------------------------------------------------------
struct g1jq_slot { uint32_t w[39]; uint32_t inf; uint32_t pad; };            // 41 words: odd stride, no LDS bank conflicts
#define G1_DIRECT_BLOCK 64              // one wavefront per workgroup: the dispatcher spreads 1024 of them over the 1024 SIMDs
// (logT, logU: only the first 2^logT terms of an output are finite -- a zero-padded input, first pass -- and only the outputs u < 2^logU of a column are
// wanted -- a caller that keeps the lower part of the result, last pass: lanes exist for those only)
__global__ __launch_bounds__(G1_DIRECT_BLOCK, 2) void k_g1_fft_direct(const g1j *in, uint64_t in_stride, uint64_t n_valid, g1j *out, uint32_t logn, uint32_t logR,
                                                            uint64_t Ns, const fr *roots, uint64_t W, const fr *scale, uint64_t total, uint32_t logT, uint32_t logU) {
    __shared__ g1jq_slot buf[G1_DIRECT_BLOCK];
    const uint32_t tid = threadIdx.x;
    const uint64_t t = blockIdx.x * (uint64_t)blockDim.x + tid;
    const uint64_t n = 1ull << logn, R = 1ull << logR, cols = n >> logR, T = 1ull << logT;
    const uint32_t tt = (uint32_t)(t & (T - 1));
    const uint64_t u = (t >> logT) & ((1ull << logU) - 1), jb = t >> (logT + logU), j = jb % cols, b = jb / cols;
    const bool live = t < total;
    g1jq_acc acc; acc.inf = true;
    uint64_t oidx = 0;
    if (live) {
        const uint64_t k = j & (Ns - 1), idx = j + (uint64_t)tt * cols;
        oidx = b * n + (j - k) * R + k + u * Ns;
        g1j x = idx < n_valid ? in[b * in_stride + idx] : g1_inf();
        if (!is_inf(x)) {
            const uint64_t e = ((uint64_t)tt * (cols / Ns) * (Ns * u + k)) & (n - 1);
            if (e == 0 && !scale) { acc.v = g1jq_unpack(x); acc.inf = false; }
            else {
                fr sc = roots[e * (W >> logn)];
                if (scale) sc = mul(sc, *scale);
                g1aq tbl[8]; fq dz[7]; g1j packed;
                const int st = g1_mul_glv_regular_aq<true>(g1jq_unpack(x), glv_split_signed(from_mont<FrP>(sc)), tbl, dz, acc.v, packed);
                if (st == 2) { acc.inf = is_inf(packed); if (!acc.inf) acc.v = g1jq_unpack(packed); } else acc.inf = st == 0;
            }
        }
    }
    // sum of the R terms of an output: lanes tt = 0 .. R - 1 are adjacent
    auto store = [&](uint32_t i) {
#pragma unroll
        for (int q = 0; q < 13; q++) { buf[i].w[q] = acc.v.x.l[q]; buf[i].w[13 + q] = acc.v.y.l[q]; buf[i].w[26 + q] = acc.v.z.l[q]; }
        buf[i].inf = acc.inf ? 1u : 0u;
    };
    store(tid);
    __syncthreads();
#pragma nounroll
    for (uint32_t off = (uint32_t)T / 2; off >= 1; off >>= 1) {
        if (tt < off && !buf[tid + off].inf) {
            g1jq q;
#pragma unroll
            for (int i = 0; i < 13; i++) { q.x.l[i] = buf[tid + off].w[i]; q.y.l[i] = buf[tid + off].w[13 + i]; q.z.l[i] = buf[tid + off].w[26 + i]; }
            acc.add(q);
            store(tid);
        }
        __syncthreads();
    }
    if (live && tt == 0) out[oidx] = acc.inf ? g1_inf() : g1jq_pack(acc.v);
}
// runs the passes; the result lands in `data` (batch x n).  tmp: batch x n scratch points.  scale: nullptr or a device Fr that
// multiplies every output (folded into the last pass).
void launch_g1_fft_direct(hipStream_t s, const g1j *in, uint64_t in_stride, uint64_t n_valid, g1j *data, g1j *tmp, uint64_t n, uint64_t batch, const fr *roots,
                          uint64_t W, const fr *scale, uint32_t max_logr, int lanes, uint32_t bits_done, uint64_t n_out, bool lanes_fixed) {
    const uint32_t logn = ilog2(n);
    if (max_logr < 1 || max_logr > 4) max_logr = 4;
    // bits_done > 0: `in` already holds the result of the passes over the first bits_done bits (launch_fb_direct_pass1); continue from there
    uint32_t bits_left = logn - bits_done;
    uint32_t npass = (bits_left + max_logr - 1) / max_logr;
    if (!npass) { launch_g1_bitrev_copy(s, in, in_stride, n_valid, data, n, batch); return; }   // n == 1: copy (a 0-bit reversal)
    // pass p writes data when the number of passes after it is even
    const g1j *src = in; uint64_t src_stride = in_stride, src_valid = n_valid, Ns = 1ull << bits_done;
    prof_begin(s, "g1_fft_direct");
    for (uint32_t p = 0; p < npass; p++) {
        const uint32_t logR = bits_left >= max_logr ? max_logr : bits_left;
        g1j *dst = ((npass - 1 - p) & 1u) ? tmp : data;
        // terms beyond the valid input are infinity (term t reads index j + t n / R): only the first ceil(valid / (n / R)) take part; of the last pass
        // only the outputs below n_out are wanted (output u of a column lands at k + u Ns): lanes for those only
        uint32_t logT = logR, logU = logR;
        const uint64_t cols = n >> logR;
        while (logT > 0 && (cols << (logT - 1)) >= src_valid) logT--;
        if (p + 1 == npass && n_out && n_out < n) while (logU > 0 && (Ns << (logU - 1)) >= n_out) logU--;
        const uint64_t total = (batch * cols) << (logT + logU);
        // as many lanes per term as keep the pass at one wavefront per SIMD (the caller's choice for full passes; pruned ones may take more)
        int L = lanes;
        if (!lanes_fixed && g1_quad_enabled() && knobs::g1_direct_coop() && (logT < logR || logU < logR)) L = total * 4 <= device_simd_lanes() ? 4 : total * 2 <= device_simd_lanes() ? 2 : lanes;
        // 24 KiB of unused dynamic LDS on top of the 10 KiB the kernel needs: at most 4 of these one-wave workgroups fit a CU, so the
        // 1024 of a 4096-point pass land one per SIMD instead of 8 per CU on half of the chip (measured: 2.7 vs 5.4 ms per pass)
        // (only while the pass has at most one wavefront per SIMD: two transforms are 2048 workgroups and want both wave slots)
        const uint64_t wgs = (total * L + G1_DIRECT_BLOCK - 1) / G1_DIRECT_BLOCK;
        const size_t pad_lds = wgs <= device_simds() ? 24 * 1024 : 0;
        const fr *sc = (p + 1 == npass) ? scale : nullptr;
        if (L > 1) launch_g1_direct_coop(s, L, (uint32_t)wgs, pad_lds, src, src_stride, src_valid, dst, logn, logR, Ns, roots, W, sc, total, logT, logU);
        else hipLaunchKernelGGL(k_g1_fft_direct, dim3((uint32_t)wgs), dim3(G1_DIRECT_BLOCK), pad_lds, s, src, src_stride, src_valid, dst, logn, logR, Ns, roots, W, sc, total, logT, logU);
        src = dst; src_stride = n; src_valid = (p + 1 == npass && n_out && n_out < n) ? n_out : n; Ns <<= logR; bits_left -= logR;
    }
    prof_end(s, "g1_fft_direct");
}

__global__ __launch_bounds__(G1_BLOCK, 2) void k_g1_normalize(const g1j *in, g1j *out, uint64_t n, int to_kilic) {
    uint64_t t = blockIdx.x * (uint64_t)blockDim.x + threadIdx.x;
    if (t >= n) return;
    g1j p = g1_normalize(in[t]);
    out[t] = to_kilic ? g1_to_kilic(p) : p;
}
// Few points (a lone commitment, a lone proof, the handful of results of a small batch): ONE WAVEFRONT per point, its inversion spread over the lanes
// (coop_inv.hpp: ~25 us instead of the ~100 us of one lane's binary GCD -- this kernel is pure latency).  Every lane computes the (wave-uniform) result; lane 0 stores.
__global__ __launch_bounds__(64) void k_g1_normalize_wave(const g1j *in, g1j *out, uint64_t n, int to_kilic) {
    const uint64_t t = blockIdx.x;
    const g1j p = in[t];
    g1j o;
    if (is_inf(p)) o = g1_inf();                            // (wave-uniform: every lane holds the same point)
    else {
        const fp zi = wave_inv_fp(p.z, 0), zi2 = sqr(zi);
        o.x = mul(p.x, zi2); o.y = mul(p.y, mul(zi2, zi)); o.z = one<FpP>();
    }
    if (threadIdx.x == 0) out[t] = to_kilic ? g1_to_kilic(o) : o;
}
// test / measurement hook: element i inverted by wavefront i cooperatively (out_coop) and by lane 0 of that wavefront alone (out_lane); mode bit 0 / bit 1 select which
__global__ __launch_bounds__(64) void k_fp_inv_both(const fp *in, fp *out_coop, fp *out_lane, int mode) {
    const fp x = in[blockIdx.x];
    if (mode & 1) { const fp y = wave_inv_fp(x, 0); if (threadIdx.x == 0) out_coop[blockIdx.x] = y; }
    if ((mode & 2) && threadIdx.x == 0) out_lane[blockIdx.x] = inv<FpP>(x);
}
void launch_fp_inv_both(hipStream_t s, const fp *in, fp *out_coop, fp *out_lane, uint64_t n, int mode) {
    if (n) hipLaunchKernelGGL(k_fp_inv_both, dim3((uint32_t)n), dim3(64), 0, s, in, out_coop, out_lane, mode);
}
// Same result with ONE F_p inversion per NB points (Montgomery's trick inside a lane): a Fermat inversion is ~570 products,
// so normalising the 4096 proofs of an FK20 run drops from ~575 to ~80 products per point.  Points are strided by `lanes`
// so that the loads of a wavefront stay adjacent.  Z = 0 entries are skipped in the running product.
#define NORM_NB 8
__global__ __launch_bounds__(G1_BLOCK, 2) void k_g1_normalize_batched(const g1j *in, g1j *out, uint64_t n, uint64_t lanes, int to_kilic) {
    uint64_t t = blockIdx.x * (uint64_t)blockDim.x + threadIdx.x;
    if (t >= lanes) return;
    fp pref[NORM_NB];
    fp acc = one<FpP>();
#pragma unroll
    for (int k = 0; k < NORM_NB; k++) {
        uint64_t i = t + (uint64_t)k * lanes;
        pref[k] = acc;
        if (i < n) { fp z = in[i].z; if (!is_zero<FpP>(z)) acc = mul(acc, z); }
    }
    fp inv_all = inv<FpP>(acc);
#pragma unroll
    for (int k = NORM_NB - 1; k >= 0; k--) {
        uint64_t i = t + (uint64_t)k * lanes;
        if (i >= n) continue;
        g1j p = in[i];
        g1j o;
        if (is_inf(p)) o = g1_inf();
        else {
            fp zi = mul(inv_all, pref[k]);
            inv_all = mul(inv_all, p.z);
            fp zi2 = sqr(zi);
            o.x = mul(p.x, zi2); o.y = mul(p.y, mul(zi2, zi)); o.z = one<FpP>();
        }
        out[i] = to_kilic ? g1_to_kilic(o) : o;
    }
}
void launch_g1_normalize(hipStream_t s, const g1j *in, g1j *out, uint64_t n, bool to_kilic) {
    if (!n) return;
    if (n < 1024 && knobs::coop_inv()) {   // small outputs (one commitment, one proof): a wavefront per point, cooperative inversion (in place is fine: a point is read before it is written)
        hipLaunchKernelGGL(k_g1_normalize_wave, dim3((uint32_t)n), dim3(64), 0, s, in, out, n, to_kilic ? 1 : 0);
        return;
    }
    if (n < 1024 || in == out) {   // in-place use of a large array: one inversion per point
        hipLaunchKernelGGL(k_g1_normalize, dim3((uint32_t)((n + G1_BLOCK - 1) / G1_BLOCK)), dim3(G1_BLOCK), 0, s, in, out, n, to_kilic ? 1 : 0);
        return;
    }
    uint64_t lanes = (n + NORM_NB - 1) / NORM_NB;
    hipLaunchKernelGGL(k_g1_normalize_batched, dim3((uint32_t)((lanes + G1_BLOCK - 1) / G1_BLOCK)), dim3(G1_BLOCK), 0, s, in, out, n, lanes, to_kilic ? 1 : 0);
}
__global__ __launch_bounds__(G1_BLOCK, 2) void k_g1_from_kilic(g1j *data, uint64_t n) {
    uint64_t t = blockIdx.x * (uint64_t)blockDim.x + threadIdx.x;
    if (t >= n) return;
    data[t] = g1_from_kilic(data[t]);
}
void launch_g1_from_kilic(hipStream_t s, g1j *data, uint64_t n) {
    if (!n) return;
    hipLaunchKernelGGL(k_g1_from_kilic, dim3((uint32_t)((n + G1_BLOCK - 1) / G1_BLOCK)), dim3(G1_BLOCK), 0, s, data, n);
}
__global__ __launch_bounds__(G1_BLOCK, 2) void k_g1_to_affine(const g1j *in, g1a *out, uint64_t n) {
    uint64_t t = blockIdx.x * (uint64_t)blockDim.x + threadIdx.x;
    if (t >= n) return;
    g1j p = in[t];
    g1a o;
    if (is_inf(p)) o = g1a_inf();
    else {
        if (!equal<FpP>(p.z, one<FpP>())) p = g1_normalize(p);
        o.x = p.x; o.y = p.y;
    }
    out[t] = o;
}
void launch_g1_to_affine(hipStream_t s, const g1j *in, g1a *out, uint64_t n) {
    if (!n) return;
    hipLaunchKernelGGL(k_g1_to_affine, dim3((uint32_t)((n + G1_BLOCK - 1) / G1_BLOCK)), dim3(G1_BLOCK), 0, s, in, out, n);
}

// (p - 1) / 2 in standard form, limb i
__device__ __forceinline__ uint32_t half_pm1(int i) {
    uint32_t lo = FpP::mod(i) - (i == 0 ? 1u : 0u);
    uint32_t hi = (i < 11) ? FpP::mod(i + 1) : 0u;
    return (lo >> 1) | (hi << 31);
}
__device__ __forceinline__ bool y_is_larger(const fp &y_std) {   // y > (p - 1) / 2
    for (int i = 11; i >= 0; i--) {
        uint32_t h = half_pm1(i);
        if (y_std.l[i] > h) return true;
        if (y_std.l[i] < h) return false;
    }
    return false;
}
// ZCash compressed form: big-endian x, bit7 compressed, bit6 inf, bit5 y > (p-1)/2
__global__ __launch_bounds__(G1_BLOCK, 2) void k_g1_compress(const g1j *in, uint8_t *out48, uint64_t n) {
    uint64_t t = blockIdx.x * (uint64_t)blockDim.x + threadIdx.x;
    if (t >= n) return;
    g1j p = in[t];
    uint8_t *o = out48 + 48 * t;
    if (is_inf(p)) {
        o[0] = 0xc0;
        for (int i = 1; i < 48; i++) o[i] = 0;
        return;
    }
    if (!equal<FpP>(p.z, one<FpP>())) p = g1_normalize(p);
    fp x = from_mont<FpP>(p.x), y = from_mont<FpP>(p.y);
    for (int i = 0; i < 48; i++) o[47 - i] = (uint8_t)(x.l[i >> 2] >> (8 * (i & 3)));
    o[0] |= 0x80 | (y_is_larger(y) ? 0x20 : 0);
}
void launch_g1_compress(hipStream_t s, const g1j *in, uint8_t *out48, uint64_t n) {
    if (!n) return;
    hipLaunchKernelGGL(k_g1_compress, dim3((uint32_t)((n + G1_BLOCK - 1) / G1_BLOCK)), dim3(G1_BLOCK), 0, s, in, out48, n);
}
__global__ __launch_bounds__(G1_BLOCK, 2) void k_g1_decompress(const uint8_t *in48, g1j *out, uint64_t n, uint32_t *bad) {
    uint64_t t = blockIdx.x * (uint64_t)blockDim.x + threadIdx.x;
    if (t >= n) return;
    g1j o;
    if (!g1_decompress(o, in48 + 48 * t)) atomicOr(bad, 1u);
    out[t] = g1_to_kilic(o);   // API output: Kilic image (inf for an invalid encoding)
}
void launch_g1_decompress(hipStream_t s, const uint8_t *in48, g1j *out, uint64_t n, uint32_t *bad_flag) {
    if (!n) return;
    hipLaunchKernelGGL(k_g1_decompress, dim3((uint32_t)((n + G1_BLOCK - 1) / G1_BLOCK)), dim3(G1_BLOCK), 0, s, in48, out, n, bad_flag);
}

// GenerateTestingSetup's G1 loop (setup.go:18-24): out[i] = powers[i] * G
__global__ __launch_bounds__(G1_BLOCK, 2) void k_g1_fixed_base_powers(const fr *powers, uint64_t n, g1j *out) {
    uint64_t t = blockIdx.x * (uint64_t)blockDim.x + threadIdx.x;
    if (t >= n) return;
    // G1 generator (decimals in-tree at bls/bls_hbls.go:23-24) in the device-internal Montgomery domain (x * 2^390 mod p)
    const uint32_t gx[12] = {0x54d1b01cu, 0x350de43fu, 0xe34ffd63u, 0xc06f1a1fu, 0xa87e2228u, 0x97813e1au,
                             0x195a98dfu, 0xe719b8a3u, 0xe5fb5b36u, 0x8adadfb4u, 0xa1033af6u, 0x082ebc25u};
    const uint32_t gy[12] = {0x39d1f18cu, 0x5340f543u, 0xe10f63b6u, 0xadc8c6c2u, 0xc66e87afu, 0x0d00bb3au,
                             0x6d865848u, 0x6e09c7c9u, 0xe3cf8885u, 0x501cb7fbu, 0xb82b61a3u, 0x16f1c975u};
    g1j g;
    for (int i = 0; i < 12; i++) { g.x.l[i] = gx[i]; g.y.l[i] = gy[i]; }
    g.z = one<FpP>();
    out[t] = g1_mul_fr(g, powers[t]);
}
void launch_g1_fixed_base_powers(hipStream_t s, const fr *powers, uint64_t n, g1j *out) {
    if (!n) return;
    hipLaunchKernelGGL(k_g1_fixed_base_powers, dim3((uint32_t)((n + G1_BLOCK - 1) / G1_BLOCK)), dim3(G1_BLOCK), 0, s, powers, n, out);
}

}  // namespace kzg
