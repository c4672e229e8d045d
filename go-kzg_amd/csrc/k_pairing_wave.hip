// k_pairing_wave.hip -- the pairing check with ONE WAVEFRONT PER CHECK (wave_pairing.hpp): the F_p12 values of a check live in LDS and the
// independent F_p products of a tower operation run on the 64 lanes, so a lone or small batch takes a fraction of the one-lane kernel's
// time (k_pairing.hip: one lane per check, the right form once the checks fill the device).  launch_pairing_check chooses between the two.
#include "internal.hpp"
#include "wave_pairing.hpp"

namespace kzg {

// runs a phase on this lane and ends it with the workgroup barrier; the workgroup is one wavefront, nothing returns early
struct wave_exec {
    wv::image &im;
    int lane;
    template <class P> __device__ __forceinline__ void run(const P &p) { p(im, lane); __syncthreads(); }
};

// ok[t] = (e(p0[t], Q0) e(p1[t], Q1) == 1), t = the workgroup index.  SHARED: q0[0], q1[0] for every check; otherwise q0[t], q1[t]
template <bool SHARED>
__global__ __launch_bounds__(wv::LANES) void k_pairing_check_wave(const g2_prepared *q0, const g2_prepared *q1, const g1j *p0, const g1j *p1, uint8_t *ok) {
    __shared__ wv::image im;
    const uint64_t t = blockIdx.x;
    wave_exec x{im, (int)threadIdx.x};
    const g2_prepared *q[2] = {SHARED ? q0 : q0 + t, SHARED ? q1 : q1 + t};
    const g1j *p[2] = {p0 + t, p1 + t};
    wv::pairing_check<2>(x, q, p, ok + t);
}
void launch_pairing_check_wave(hipStream_t s, bool shared_lines, const g2_prepared *q0, const g2_prepared *q1, const g1j *p0, const g1j *p1, uint64_t n, uint8_t *ok) {
    if (!n) return;
    if (shared_lines) hipLaunchKernelGGL(k_pairing_check_wave<true>, dim3((uint32_t)n), dim3(wv::LANES), 0, s, q0, q1, p0, p1, ok);
    else hipLaunchKernelGGL(k_pairing_check_wave<false>, dim3((uint32_t)n), dim3(wv::LANES), 0, s, q0, q1, p0, p1, ok);
}

// test hook: out[12 t ..] = e(g1[t], Q_t) (device exponent) in STANDARD form; g1 Kilic images (k_pairing_value's twin)
__global__ __launch_bounds__(wv::LANES) void k_pairing_value_wave(const g1j *g1, const g2_prepared *q, fp *out) {
    __shared__ wv::image im;
    const uint64_t t = blockIdx.x;
    wave_exec x{im, (int)threadIdx.x};
    wv::pairing_value(x, q + t, g1 + t, out + 12 * t);
}
void launch_pairing_value_wave(hipStream_t s, const g1j *g1_kilic, const g2_prepared *q, uint64_t n, fp *out) {
    if (!n) return;
    hipLaunchKernelGGL(k_pairing_value_wave, dim3((uint32_t)n), dim3(wv::LANES), 0, s, g1_kilic, q, out);
}

// test hook: one tower operation per workgroup on row t of a and b (12 F_p each, STANDARD form in and out).  op: 0 mul, 1 sqr, 2 inv, 3 frob,
// 4 frob2, 5 frob3, 6 cyclotomic sqr, 7 conj, 8 mul_014 (b holds c0, c1, c4 as its first six elements).  The operands sit in values 1 and 2
__global__ __launch_bounds__(wv::LANES) void k_wave_fp12_op(int op, const fp *a, const fp *b, fp *out) {
    __shared__ wv::image im;
    const uint64_t t = blockIdx.x;
    wave_exec x{im, (int)threadIdx.x};
    x.run([=](wv::image &im, int lane) {
        wv::const_phase(im, lane);
        if (lane >= 16 && lane < 28) wv::st(im, lane, wv::reg(1) + lane - 16, to_mont<FpP>(a[12 * t + lane - 16]));
        if (lane >= 32 && lane < 44) wv::st(im, lane, wv::reg(2) + lane - 32, to_mont<FpP>(b[12 * t + lane - 32]));
        if (lane >= 48 && lane < 54) wv::st(im, lane, wv::XS + lane - 48, to_mont<FpP>(b[12 * t + lane - 48]));
    });
    switch (op) {   // the same for every lane
    case 0: wv::mul(x, 0, 1, 2); break;
    case 1: wv::sqr(x, 0, 1); break;
    case 2: wv::inv(x, 0, 1); break;
    case 3: wv::frob(x, 0, 1); break;
    case 4: wv::frob2(x, 0, 1); break;
    case 5: wv::frob3(x, 0, 1); break;
    case 6: wv::cyc_sqr(x, 0, 1); break;
    case 7: wv::conj(x, 0, 1); break;
    default: wv::mul_014(x, 0, 1); break;
    }
    x.run([=](wv::image &im, int lane) { if (lane < 12) out[12 * t + lane] = from_mont<FpP>(wv::ld(im, lane, wv::reg(0) + lane)); });
}
void launch_wave_fp12_op(hipStream_t s, int op, const fp *a, const fp *b, uint64_t n, fp *out) {
    if (!n) return;
    hipLaunchKernelGGL(k_wave_fp12_op, dim3((uint32_t)n), dim3(wv::LANES), 0, s, op, a, b, out);
}

}  // namespace kzg
