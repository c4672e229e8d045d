// wave_tower.hpp -- the F_p12 tower of tower.hpp on ONE WAVEFRONT: a value is 12 F_p elements in LDS (memory order and basis of tower.hpp,
// canonical, device-internal Montgomery domain), and the 18 .. 54 independent F_p products inside a tower operation are spread over the 64 lanes.
//
// An operation is a short list of PHASES.  A phase is a plain function of (lane, LDS image): it reads slots, uses field.hpp's add / sub / neg /
// mul on them and writes slots -- no cross-lane intrinsic, no inline assembly.  Between two phases the kernel executes __syncthreads() (the
// workgroup is one wavefront); tests/host/pairing_wave_emul.cpp replays the same phases lane by lane on the host, a barrier being the end of
// the lane loop, and checks under KZG_WAVE_TRACE that no slot written by one lane in a phase is touched by another lane in that phase.
//
// Two table-driven phase kinds carry all the arithmetic:
//   product phase: lane l computes  out = +-(x1 y1) [+- x2 y2] [doubled]  for row l of a table (an F_p2 product component is one row),
//   sum phase:     lane l computes  out = sum of slots - sum of slots     for row l of a table (Karatsuba operands, the reduction of the
//                  product slots to output coefficients; xi = 1 + u is a signed pair of slots, a small factor is a repeated term).
// The tables are built at compile time by running the formulas of tower.hpp on symbolic linear forms over slot references (build_tables), so
// the lane assignment is derived, not typed in.  Below the F_p12 level products are schoolbook: 27 F_p2 products x 2 components = 54 lanes in
// one round for fp12 mul.  All arithmetic is exact in F_p on canonical representatives: every operation returns THE SAME BYTES as its
// tower.hpp counterpart whatever the order of summation.  The one F_p inversion of inv is wave_inv_fp (coop_inv.hpp; all 64 lanes converged)
// on the device and inv<FpP> in the host build: the same canonical value by coop_inv.hpp's contract.
//
// Slots of the image (48 bytes each):  X 0..79 scratch (product slots from 0, operand sums and scaled line coefficients from XS = 64),
// C 80..87 constants, E 88..95 the G1 inputs of the lines, then NREG values of 12 slots.  An operation may write the value it reads: every
// operation stages its products in X before the last phase writes the result.
#pragma once
#include "tower.hpp"
#if defined(__HIPCC__)
#include "coop_inv.hpp"
#define KZG_WV __device__ __forceinline__
#define KZG_WV_NOINLINE __device__ __noinline__ static
#else
#define KZG_WV inline
#define KZG_WV_NOINLINE inline
#endif

namespace kzg {
namespace wv {

constexpr int LANES = 64;
constexpr int NX = 80, XS = 64;
constexpr int C_ONE = 80, C_G0 = 81, C_G1 = 82, C_G2R = 83, C_G2I = 84;   // 1, gamma_3 (its c1), gamma_3^2 (its c0), gamma_6 (c0, c1): frob_gamma
constexpr int E0 = 88;                                                    // (Y, X Z, Z^3) of pair i at E0 + 3 i
constexpr int R0 = 96, NREG = 8, NSLOT = R0 + 12 * NREG;                  // 192 slots = 9216 bytes
constexpr int reg(int r) { return R0 + 12 * r; }
// slot references of the tables: below RA absolute, then relative to the operation's operands a, b and its result d
constexpr int RA = 96, RB = 108, RD = 120, NREF = 132;

#if defined(KZG_WAVE_TRACE)
// host tracing build: which lanes read and which lane wrote each slot in the current phase (pairing_wave_emul.cpp checks and clears per phase)
struct image { fp s[NSLOT]; uint64_t rd[NSLOT], wr[NSLOT]; };
inline fp ld(image &im, int lane, int i) { im.rd[i] |= 1ull << lane; return im.s[i]; }
inline void st(image &im, int lane, int i, const fp &v) { im.wr[i] |= 1ull << lane; im.s[i] = v; }
#else
struct image { fp s[NSLOT]; };
KZG_WV fp ld(image &im, int, int i) { return im.s[i]; }
KZG_WV void st(image &im, int, int i, const fp &v) { im.s[i] = v; }
#endif

// ---------------- tables ----------------
enum { M_TWO = 1, M_SUB = 2, M_NEG = 4, M_DBL = 8 };          // second product present / subtracted; first product negated; result doubled
struct mulrow { uint8_t out, x1, y1, x2, y2, mode; };
constexpr int MAXT = 16;
struct linrow { uint8_t out, npos, nneg, ref[MAXT]; };        // out = sum ref[0 .. npos) - sum ref[npos .. npos + nneg)
struct phase { uint16_t first; uint8_t kind, n; };            // kind 0: n rows of mr from `first`, 1: of lr; row l is lane l's
struct opdesc { uint8_t first, n; };
// OP_MUL d = a b (sqr: b = a) | OP_CYC Granger-Scott squaring | OP_M014 d = a (c0 + c1 v + c4 v w), (c0, c1, c4) in X[XS .. XS + 6) |
// OP_FROB a^p | OP_CONJ | OP_COPY | OP_INV_A: X[0] = the norm in F_p whose inverse OP_INV_B expects in X[1] | OP_ISONE: X[0 .. 12) = a - 1
enum { OP_MUL, OP_CYC, OP_M014, OP_FROB, OP_CONJ, OP_COPY, OP_INV_A, OP_INV_B, OP_ISONE, NOPS };

struct lin { int8_t c[NREF] = {}; };                           // a linear form over slot references
constexpr lin unit(int r) { lin o; o.c[r] = 1; return o; }
constexpr lin operator+(lin a, const lin &b) { for (int i = 0; i < NREF; i++) a.c[i] = (int8_t)(a.c[i] + b.c[i]); return a; }
constexpr lin operator-(lin a, const lin &b) { for (int i = 0; i < NREF; i++) a.c[i] = (int8_t)(a.c[i] - b.c[i]); return a; }
constexpr lin operator*(int k, lin a) { for (int i = 0; i < NREF; i++) a.c[i] = (int8_t)(a.c[i] * k); return a; }
struct l2 { lin re, im; };                                     // the forms of tower.hpp's fp2 / fp6 functions
constexpr l2 operator+(const l2 &a, const l2 &b) { return l2{a.re + b.re, a.im + b.im}; }
constexpr l2 operator-(const l2 &a, const l2 &b) { return l2{a.re - b.re, a.im - b.im}; }
constexpr l2 operator*(int k, const l2 &a) { return l2{k * a.re, k * a.im}; }
constexpr l2 xi(const l2 &a) { return l2{a.re - a.im, a.re + a.im}; }
constexpr l2 at2(int r) { return l2{unit(r), unit(r + 1)}; }
struct l6 { l2 c0, c1, c2; };
constexpr l6 operator+(const l6 &a, const l6 &b) { return l6{a.c0 + b.c0, a.c1 + b.c1, a.c2 + b.c2}; }
constexpr l6 operator-(const l6 &a, const l6 &b) { return l6{a.c0 - b.c0, a.c1 - b.c1, a.c2 - b.c2}; }
constexpr l6 mul_v(const l6 &a) { return l6{xi(a.c2), a.c0, a.c1}; }

struct tables {
    mulrow mr[256] = {};
    linrow lr[128] = {};
    phase ph[32] = {};
    opdesc ops[NOPS] = {};
    int nm = 0, nl = 0, np = 0, slot = 0, op = 0;

    constexpr void op_begin(int o) { op = o; ops[o].first = (uint8_t)np; ops[o].n = 0; }
    constexpr void ph_begin(int kind, int slot0 = 0) { ph[np].kind = (uint8_t)kind; ph[np].first = (uint16_t)(kind ? nl : nm); ph[np].n = 0; slot = slot0; }
    constexpr void ph_end() { np++; ops[op].n++; }
    constexpr void row(int out, int x1, int y1, int x2, int y2, int mode) {
        mr[nm++] = mulrow{(uint8_t)out, (uint8_t)x1, (uint8_t)y1, (uint8_t)x2, (uint8_t)y2, (uint8_t)mode};
        ph[np].n++;
    }
    // x y for F_p2 operands at slot references x, x + 1 and y, y + 1: two rows, two product slots
    constexpr l2 prod2(int x, int y, int dbl = 0) {
        const int t = slot; slot += 2;
        row(t, x, y, x + 1, y + 1, M_TWO | M_SUB | dbl);
        row(t + 1, x, y + 1, x + 1, y, M_TWO | dbl);
        return at2(t);
    }
    constexpr l2 sqr2(int x) {
        const int t = slot; slot += 2;
        row(t, x, x, x + 1, x + 1, M_TWO | M_SUB);
        row(t + 1, x, x + 1, 0, 0, M_DBL);
        return at2(t);
    }
    // schoolbook fp6 product of the operands at a .. a + 5 and b .. b + 5: 9 F_p2 products
    constexpr l6 prod6(int a, int b) {
        l2 t[3][3] = {};
        for (int i = 0; i < 3; i++) for (int j = 0; j < 3; j++) t[i][j] = prod2(a + 2 * i, b + 2 * j);
        return l6{t[0][0] + xi(t[1][2] + t[2][1]), t[0][1] + t[1][0] + xi(t[2][2]), t[0][2] + t[1][1] + t[2][0]};
    }
    constexpr void emit(int out, const lin &v) {
        linrow r = {};
        r.out = (uint8_t)out;
        int n = 0;
        for (int i = 0; i < NREF; i++) for (int k = 0; k < v.c[i]; k++) { r.ref[n++] = (uint8_t)i; r.npos++; }   // n >= MAXT: not a constant expression
        for (int i = 0; i < NREF; i++) for (int k = 0; k < -v.c[i]; k++) { r.ref[n++] = (uint8_t)i; r.nneg++; }
        lr[nl++] = r;
        ph[np].n++;
    }
    constexpr void emit2(int out, const l2 &v) { emit(out, v.re); emit(out + 1, v.im); }
    constexpr void emit6(int out, const l6 &v) { emit2(out, v.c0); emit2(out + 2, v.c1); emit2(out + 4, v.c2); }
};

constexpr tables build_tables() {
    tables t;
    // fp12_mul: Karatsuba at the top level only
    t.op_begin(OP_MUL);
    t.ph_begin(1);
    for (int i = 0; i < 6; i++) t.emit(XS + i, unit(RA + i) + unit(RA + 6 + i));
    for (int i = 0; i < 6; i++) t.emit(XS + 6 + i, unit(RB + i) + unit(RB + 6 + i));
    t.ph_end();
    t.ph_begin(0);
    {
        const l6 aa = t.prod6(RA, RB), bb = t.prod6(RA + 6, RB + 6), cc = t.prod6(XS, XS + 6);
        t.ph_end();
        t.ph_begin(1);
        t.emit6(RD, aa + mul_v(bb));
        t.emit6(RD + 6, cc - aa - bb);
        t.ph_end();
    }
    // fp12_cyc_sqr: fp4_sqr(a, b) = (xi b^2 + a^2, 2 a b), three times
    t.op_begin(OP_CYC);
    t.ph_begin(0);
    {
        const int z0 = RA, z4 = RA + 2, z3 = RA + 4, z2 = RA + 6, z1 = RA + 8, z5 = RA + 10;
        const l2 a0 = t.sqr2(z0), b0 = t.sqr2(z1), c0 = t.prod2(z0, z1, M_DBL);
        const l2 a1 = t.sqr2(z2), b1 = t.sqr2(z3), c1 = t.prod2(z2, z3, M_DBL);
        const l2 a2 = t.sqr2(z4), b2 = t.sqr2(z5), c2 = t.prod2(z4, z5, M_DBL);
        t.ph_end();
        t.ph_begin(1);
        t.emit2(RD, 3 * (xi(b0) + a0) - 2 * at2(z0));          // z0
        t.emit2(RD + 2, 3 * (xi(b1) + a1) - 2 * at2(z4));      // z4
        t.emit2(RD + 4, 3 * (xi(b2) + a2) - 2 * at2(z3));      // z3
        t.emit2(RD + 6, 3 * xi(c2) + 2 * at2(z2));             // z2
        t.emit2(RD + 8, 3 * c0 + 2 * at2(z1));                 // z1
        t.emit2(RD + 10, 3 * c1 + 2 * at2(z5));                // z5
        t.ph_end();
    }
    // fp12_mul_014 without the Karatsuba step of its c1: f0 (c4 v) + f1 (c0 + c1 v), 18 F_p2 products and no operand sums
    t.op_begin(OP_M014);
    t.ph_begin(0);
    {
        const int c0 = XS, c1 = XS + 2, c4 = XS + 4, a0 = RA, a1 = RA + 2, a2 = RA + 4, b0 = RA + 6, b1 = RA + 8, b2 = RA + 10;
        const l6 aa = {t.prod2(a0, c0) + xi(t.prod2(a2, c1)), t.prod2(a0, c1) + t.prod2(a1, c0), t.prod2(a2, c0) + t.prod2(a1, c1)};
        const l6 bb = {xi(t.prod2(b2, c4)), t.prod2(b0, c4), t.prod2(b1, c4)};
        const l6 ac = {xi(t.prod2(a2, c4)), t.prod2(a0, c4), t.prod2(a1, c4)};
        const l6 bc = {t.prod2(b0, c0) + xi(t.prod2(b2, c1)), t.prod2(b0, c1) + t.prod2(b1, c0), t.prod2(b2, c0) + t.prod2(b1, c1)};
        t.ph_end();
        t.ph_begin(1);
        t.emit6(RD, aa + mul_v(bb));
        t.emit6(RD + 6, ac + bc);
        t.ph_end();
    }
    // fp12_frob: conj(a_k) times (1, gamma_3, gamma_3^2) per half into X, then the c1 half times gamma_6
    t.op_begin(OP_FROB);
    t.ph_begin(0);
    for (int h = 0; h < 2; h++) {
        const int a = RA + 6 * h, x = 6 * h;
        t.row(x, a, C_ONE, 0, 0, 0);
        t.row(x + 1, a + 1, C_ONE, 0, 0, M_NEG);
        t.row(x + 2, a + 3, C_G0, 0, 0, 0);                    // (re - im u)(g u) = im g + re g u
        t.row(x + 3, a + 2, C_G0, 0, 0, 0);
        t.row(x + 4, a + 4, C_G1, 0, 0, 0);
        t.row(x + 5, a + 5, C_G1, 0, 0, M_NEG);
    }
    t.ph_end();
    t.ph_begin(0);
    for (int i = 0; i < 6; i++) t.row(RD + i, i, C_ONE, 0, 0, 0);
    for (int k = 0; k < 3; k++) {
        t.row(RD + 6 + 2 * k, 6 + 2 * k, C_G2R, 7 + 2 * k, C_G2I, M_TWO | M_SUB);
        t.row(RD + 7 + 2 * k, 6 + 2 * k, C_G2I, 7 + 2 * k, C_G2R, M_TWO);
    }
    t.ph_end();
    t.op_begin(OP_CONJ);
    t.ph_begin(1);
    for (int i = 0; i < 6; i++) t.emit(RD + i, unit(RA + i));
    for (int i = 6; i < 12; i++) t.emit(RD + i, -1 * unit(RA + i));
    t.ph_end();
    t.op_begin(OP_COPY);
    t.ph_begin(1);
    for (int i = 0; i < 12; i++) t.emit(RD + i, unit(RA + i));
    t.ph_end();
    // fp12_inv, down to the norm n in F_p: D = a0^2 - v a1^2 at XS, (c0, c1, c2) of fp6_inv at XS + 6, t = D0 c0 + xi (D2 c1 + D1 c2) at XS + 12
    t.op_begin(OP_INV_A);
    t.ph_begin(0);
    {
        const l6 s0 = t.prod6(RA, RA), s1 = t.prod6(RA + 6, RA + 6);
        t.ph_end();
        t.ph_begin(1);
        t.emit6(XS, s0 - mul_v(s1));
        t.ph_end();
    }
    t.ph_begin(0);
    {
        const int d0 = XS, d1 = XS + 2, d2 = XS + 4;
        const l2 c0 = t.prod2(d0, d0) - xi(t.prod2(d1, d2)), c1 = xi(t.prod2(d2, d2)) - t.prod2(d0, d1), c2 = t.prod2(d1, d1) - t.prod2(d0, d2);
        t.ph_end();
        t.ph_begin(1);
        t.emit2(XS + 6, c0); t.emit2(XS + 8, c1); t.emit2(XS + 10, c2);
        t.ph_end();
        t.ph_begin(0);
        const l2 n = t.prod2(d0, XS + 6) + xi(t.prod2(d2, XS + 8) + t.prod2(d1, XS + 10));
        t.ph_end();
        t.ph_begin(1);
        t.emit2(XS + 12, n);
        t.ph_end();
    }
    t.ph_begin(0);
    t.row(0, XS + 12, XS + 12, XS + 13, XS + 13, M_TWO);
    t.ph_end();
    // ... and back up from 1 / n in X[1]: 1 / t at X[2 .. 4), fp6_inv's result at X[4 .. 10), then the two fp6 products
    t.op_begin(OP_INV_B);
    t.ph_begin(0);
    t.row(2, XS + 12, 1, 0, 0, 0);
    t.row(3, XS + 13, 1, 0, 0, M_NEG);
    t.ph_end();
    t.ph_begin(0, 4);
    for (int k = 0; k < 3; k++) t.prod2(XS + 6 + 2 * k, 2);
    t.ph_end();
    t.ph_begin(0, 10);
    {
        const l6 o0 = t.prod6(RA, 4), o1 = t.prod6(RA + 6, 4);
        t.ph_end();
        t.ph_begin(1);
        t.emit6(RD, o0);
        t.emit6(RD + 6, l6{} - o1);
        t.ph_end();
    }
    // X[k] = a[k] - 1[k]: all zero exactly when a is one
    t.op_begin(OP_ISONE);
    t.ph_begin(1);
    t.emit(0, unit(RA) - unit(C_ONE));
    for (int i = 1; i < 12; i++) t.emit(i, unit(RA + i));
    t.ph_end();
    return t;
}

#if defined(__HIPCC__)
static __device__ const tables TB = build_tables();
#else
static constexpr tables TB = build_tables();
#endif

// ---------------- phases ----------------
KZG_WV int slot_of(int ref, int a, int b, int d) { return ref < RA ? ref : ref < RB ? a + (ref - RA) : ref < RD ? b + (ref - RB) : d + (ref - RD); }

// lane `lane` of a table phase of an operation on the values at slots a, b (operands) and d (result)
KZG_WV_NOINLINE void table_phase(image &im, int lane, int pi, int a, int b, int d) {
    const phase p = TB.ph[pi];
    if (lane >= p.n) return;
    if (p.kind == 0) {
        const mulrow r = TB.mr[p.first + lane];
        fp v = mul(ld(im, lane, slot_of(r.x1, a, b, d)), ld(im, lane, slot_of(r.y1, a, b, d)));
        if (r.mode & M_NEG) v = neg<FpP>(v);
        if (r.mode & M_TWO) {
            const fp w = mul(ld(im, lane, slot_of(r.x2, a, b, d)), ld(im, lane, slot_of(r.y2, a, b, d)));
            v = (r.mode & M_SUB) ? sub(v, w) : add(v, w);
        }
        if (r.mode & M_DBL) v = add(v, v);
        st(im, lane, slot_of(r.out, a, b, d), v);
    } else {
        const linrow &r = TB.lr[p.first + lane];
        fp v = zero<FpP>();
        const int npos = r.npos, nneg = r.nneg;
        for (int k = 0; k < npos; k++) v = add(v, ld(im, lane, slot_of(r.ref[k], a, b, d)));
        for (int k = 0; k < nneg; k++) v = sub(v, ld(im, lane, slot_of(r.ref[npos + k], a, b, d)));
        st(im, lane, slot_of(r.out, a, b, d), v);
    }
}
// the constants of the image (once per image, with whatever else the first phase writes)
KZG_WV void const_phase(image &im, int lane) {
    if (lane == 0) st(im, lane, C_ONE, one<FpP>());
    if (lane == 1) st(im, lane, C_G0, frob_gamma(0).c1);
    if (lane == 2) st(im, lane, C_G1, frob_gamma(1).c0);
    if (lane == 3) st(im, lane, C_G2R, frob_gamma(2).c0);
    if (lane == 4) st(im, lane, C_G2I, frob_gamma(2).c1);
}
// X[1] = 1 / X[0] (0 -> 0).  Device: the whole wavefront computes it (every lane must be here, converged); lane 0 stores
KZG_WV void inv_phase(image &im, int lane) {
#if defined(__HIPCC__)
    const fp r = wave_inv_fp(ld(im, lane, 0), 0);
    if (lane == 0) st(im, lane, 1, r);
#else
    if (lane == 0) st(im, lane, 1, inv<FpP>(ld(im, lane, 0)));
#endif
}

// ---------------- operations ----------------
// X runs a phase on all 64 lanes and ends it with a barrier: X::run(f) with f(image &, lane).  Values are named by register number.
template <class X> KZG_WV void run_op(X &x, int op, int d, int a, int b) {
    const int first = TB.ops[op].first, n = TB.ops[op].n;
    const int sa = reg(a), sb = reg(b), sd = reg(d);
    for (int k = 0; k < n; k++) x.run([=](image &im, int lane) { table_phase(im, lane, first + k, sa, sb, sd); });
}
template <class X> KZG_WV void mul(X &x, int d, int a, int b) { run_op(x, OP_MUL, d, a, b); }
template <class X> KZG_WV void sqr(X &x, int d, int a) { run_op(x, OP_MUL, d, a, a); }   // 54 of 64 lanes either way: no separate complex squaring
template <class X> KZG_WV void cyc_sqr(X &x, int d, int a) { run_op(x, OP_CYC, d, a, a); }
template <class X> KZG_WV void mul_014(X &x, int d, int a) { run_op(x, OP_M014, d, a, a); }   // (c0, c1, c4) at X[XS .. XS + 6)
template <class X> KZG_WV void frob(X &x, int d, int a) { run_op(x, OP_FROB, d, a, a); }
template <class X> KZG_WV void frob2(X &x, int d, int a) { frob(x, d, a); frob(x, d, d); }
template <class X> KZG_WV void frob3(X &x, int d, int a) { frob2(x, d, a); frob(x, d, d); }
template <class X> KZG_WV void conj(X &x, int d, int a) { run_op(x, OP_CONJ, d, a, a); }
template <class X> KZG_WV void copy(X &x, int d, int a) { run_op(x, OP_COPY, d, a, a); }
template <class X> KZG_WV void inv(X &x, int d, int a) {
    run_op(x, OP_INV_A, d, a, a);
    x.run([=](image &im, int lane) { inv_phase(im, lane); });
    run_op(x, OP_INV_B, d, a, a);
}
// leaves a - 1 in X[0 .. 12); is_one_of reads it in the NEXT phase (one lane decides)
template <class X> KZG_WV void is_one_prepare(X &x, int a) { run_op(x, OP_ISONE, a, a, a); }
KZG_WV bool is_one_of(image &im, int lane) {
    bool z = true;
    for (int k = 0; k < 12; k++) z = is_zero<FpP>(ld(im, lane, k)) && z;
    return z;
}

}  // namespace wv
}  // namespace kzg
