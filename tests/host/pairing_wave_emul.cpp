// Host replay of wave_tower.hpp / wave_pairing.hpp for tests/test_pairing_wave_host.py: every phase runs for lanes 0 .. 63 in turn on one LDS
// image, a barrier being the end of the lane loop.  Built with KZG_WAVE_TRACE, the image's accessors record per phase which lanes read and
// which lanes wrote each slot; end_phase counts a RACE for every slot written by one lane and read or written by another lane in the same
// phase (on the device the order of lanes within a phase is not defined).  Interfaces mirror pairing_emul.cpp: F_p values cross in STANDARD
// form (12 little-endian u32 limbs), F_p12 values as 12 of them in memory order; the batch hook takes the C ABI's memory images.
#include <string.h>
#include "pairing.hpp"
#include "verify_inputs.hpp"
#include "wave_pairing.hpp"

using namespace kzg;

static uint64_t g_races = 0, g_phases = 0;
struct host_exec {
    wv::image im;
    host_exec() { memset(&im, 0, sizeof im); }
    template <class P> void run(const P &p) {
        for (int lane = 0; lane < wv::LANES; lane++) p(im, lane);
        g_phases++;
#if defined(KZG_WAVE_TRACE)
        for (int i = 0; i < wv::NSLOT; i++) {
            const uint64_t w = im.wr[i], r = im.rd[i];
            if (w && ((w & (w - 1)) || (r & ~w))) g_races++;      // two writers, or a reader that is not the writer
            im.wr[i] = im.rd[i] = 0;
        }
#endif
    }
};

static fp in_fp(const uint32_t *s) { fp a; for (int i = 0; i < 12; i++) a.l[i] = s[i]; return to_mont<FpP>(a); }
static void out_fp(uint32_t *d, const fp &a) { fp s = from_mont<FpP>(a); for (int i = 0; i < 12; i++) d[i] = s.l[i]; }
static void out_reg(uint32_t *d, host_exec &x, int r) { for (int k = 0; k < 12; k++) out_fp(d + 12 * k, x.im.s[wv::reg(r) + k]); }

extern "C" {
uint64_t pw_races() { return g_races; }
uint64_t pw_phases() { return g_phases; }
int pw_traced() {
#if defined(KZG_WAVE_TRACE)
    return 1;
#else
    return 0;
#endif
}
uint64_t pw_image_bytes() { return wv::NSLOT * sizeof(fp); }
// the op codes of pe_fp12_op; what k_wave_fp12_op does with one row.  inplace: the result overwrites the operand a
void pw_fp12_op(int op, const uint32_t *a, const uint32_t *b, uint32_t *out, int inplace) {
    static host_exec x;
    const int d = inplace ? 1 : 0;
    x.run([=](wv::image &im, int lane) {
        wv::const_phase(im, lane);
        if (lane >= 16 && lane < 28) wv::st(im, lane, wv::reg(1) + lane - 16, in_fp(a + 12 * (lane - 16)));
        if (lane >= 32 && lane < 44) wv::st(im, lane, wv::reg(2) + lane - 32, in_fp(b + 12 * (lane - 32)));
        if (lane >= 48 && lane < 54) wv::st(im, lane, wv::XS + lane - 48, in_fp(b + 12 * (lane - 48)));
    });
    switch (op) {
    case 0: wv::mul(x, d, 1, 2); break;
    case 1: wv::sqr(x, d, 1); break;
    case 2: wv::inv(x, d, 1); break;
    case 3: wv::frob(x, d, 1); break;
    case 4: wv::frob2(x, d, 1); break;
    case 5: wv::frob3(x, d, 1); break;
    case 6: wv::cyc_sqr(x, d, 1); break;
    case 7: wv::conj(x, d, 1); break;
    default: wv::mul_014(x, d, 1); break;
    }
    out_reg(out, x, d);
}
// pe_pairing's interface for n = 1 or 2 pairs, as ONE multi-Miller loop over both (the form the check kernel runs)
int pw_pairing(uint64_t n, const uint32_t *g1, const uint32_t *g2, uint32_t *out) {
    if (n < 1 || n > 2) return 0;
    static host_exec x;
    static g2_prepared prep[2];
    g1j p[2];
    for (uint64_t i = 0; i < n; i++) {
        p[i].x = in_fp(g1 + 36 * i); p[i].y = in_fp(g1 + 36 * i + 12); p[i].z = in_fp(g1 + 36 * i + 24);
        g2a q;
        q.x.c0 = in_fp(g2 + 60 * i); q.x.c1 = in_fp(g2 + 60 * i + 12); q.y.c0 = in_fp(g2 + 60 * i + 24); q.y.c1 = in_fp(g2 + 60 * i + 36);
        g2_prepare(&prep[i], q, g2[60 * i + 48] != 0);
    }
    const g2_prepared *qs[2] = {&prep[0], &prep[1]};
    const g1j *ps[2] = {&p[0], &p[1]};
    if (n == 1) wv::multi_miller_loop<1>(x, qs, ps, false);
    else wv::multi_miller_loop<2>(x, qs, ps, false);
    wv::final_exponentiation(x);
    out_reg(out, x, wv::F);
    return 1;
}
// pe_pairing_check2's interface: 1 when e(P0, Q0) e(P1, Q1) == 1
int pw_pairing_check2(const uint32_t *g1, const uint32_t *g2) {
    static host_exec x;
    static g2_prepared prep[2];
    g1j p[2];
    for (int i = 0; i < 2; i++) {
        p[i].x = in_fp(g1 + 36 * i); p[i].y = in_fp(g1 + 36 * i + 12); p[i].z = in_fp(g1 + 36 * i + 24);
        g2a q;
        q.x.c0 = in_fp(g2 + 60 * i); q.x.c1 = in_fp(g2 + 60 * i + 12); q.y.c0 = in_fp(g2 + 60 * i + 24); q.y.c1 = in_fp(g2 + 60 * i + 36);
        g2_prepare(&prep[i], q, g2[60 * i + 48] != 0);
    }
    const g2_prepared *qs[2] = {&prep[0], &prep[1]};
    const g1j *ps[2] = {&p[0], &p[1]};
    uint8_t ok = 2;
    wv::pairing_check<2>(x, qs, ps, &ok);
    return ok;
}
// the trace on three phases written to be wrong or right: lane 1 reads what lane 0 writes (1 race), two lanes write one slot (1 race), a
// lane rewrites the slot it read while another slot is read by all (0 races).  Returns the number of races seen, 2 when the trace works
int pw_trace_selftest() {
    static host_exec x;
    const uint64_t before = g_races;
    x.run([](wv::image &im, int lane) { if (lane == 0) wv::st(im, lane, 0, one<FpP>()); if (lane == 1) (void)wv::ld(im, lane, 0); });
    x.run([](wv::image &im, int lane) { if (lane == 2 || lane == 40) wv::st(im, lane, 5, zero<FpP>()); });
    x.run([](wv::image &im, int lane) { wv::st(im, lane, 8 + lane, add(wv::ld(im, lane, 8 + lane), wv::ld(im, lane, 7))); });
    const uint64_t seen = g_races - before;
    g_races = before;
    return (int)seen;
}
// pe_kzg_check_batch's interface: k_kzg_check_inputs + k_pairing_check_wave<true> over n rows
void pw_kzg_check_batch(uint64_t n, const g1j *c, const g1j *pi, const fr *ys, const g1j *es, const fr *bs, const g2_prepared *gen, const g2_prepared *q1,
                        uint8_t *ok) {
    static host_exec x;
    const g2_prepared *qs[2] = {gen, q1};
    for (uint64_t t = 0; t < n; t++) {
        g1j p[2];
        kzg_check_inputs_lane(c[t], pi[t], ys, es, t, bs[t], p[0], p[1]);
        const g1j *ps[2] = {&p[0], &p[1]};
        wv::pairing_check<2>(x, qs, ps, ok + t);
    }
}
// the value hook's path: one pair, the G1 point as a Kilic image, the G2 point prepared from its Kilic image
void pw_pairing_value_kilic(const g1j *g1, const g2j *g2_kilic, uint32_t *out) {
    static host_exec x;
    static g2_prepared prep;
    const g2j q = g2_from_kilic(*g2_kilic);
    g2_prepare(&prep, g2_to_affine(q), is_inf(q));
    fp o[12];
    wv::pairing_value(x, &prep, g1, o);
    for (int k = 0; k < 12; k++) for (int i = 0; i < 12; i++) out[12 * k + i] = o[k].l[i];
}
}

#ifdef PW_MAIN
// Stand-alone form for a sanitizer build: the batch file of pairing_emul.cpp's PE_MAIN (u64 n | n x c | n x pi | n x y | n x b | one Kilic G2
// image of [s] G2) through the replay; prints the mask as a line of 0 / 1 and the number of races the trace saw.
#include <stdio.h>
#include <vector>
int main(int argc, char **argv) {
    if (argc != 2) return 2;
    FILE *f = fopen(argv[1], "rb");
    if (!f) return 2;
    uint64_t n = 0;
    if (fread(&n, sizeof n, 1, f) != 1 || n == 0 || n > 4096) return 2;
    std::vector<g1j> c(n), pi(n); std::vector<fr> ys(n), bs(n); g2j q;
    if (fread(c.data(), sizeof(g1j), n, f) != n || fread(pi.data(), sizeof(g1j), n, f) != n || fread(ys.data(), sizeof(fr), n, f) != n ||
        fread(bs.data(), sizeof(fr), n, f) != n || fread(&q, sizeof q, 1, f) != 1) return 2;
    fclose(f);
    std::vector<g2_prepared> prep(2);
    const g2j gen = g2_from_kilic(g2_to_kilic(g2_generator()));
    g2_prepare(&prep[0], g2_to_affine(gen), is_inf(gen));
    const g2j qs = g2_from_kilic(q);
    g2_prepare(&prep[1], g2_to_affine(qs), is_inf(qs));
    std::vector<uint8_t> ok(n);
    pw_kzg_check_batch(n, c.data(), pi.data(), ys.data(), nullptr, bs.data(), &prep[0], &prep[1], ok.data());
    for (uint64_t i = 0; i < n; i++) putchar(ok[i] ? '1' : '0');
    printf("\nraces %llu\n", (unsigned long long)g_races);
    return 0;
}
#endif
