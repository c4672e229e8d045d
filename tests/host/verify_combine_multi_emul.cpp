// Host build of verify_combine_multi.hpp for tests/test_verify_combine_multi_host.py: the lane bodies of k_verify_combine_multi.hip on the CPU --
// a row's term scalars, the weight of a coefficient, and a whole call the way k_combine_multi_poly and k_combine_multi_fold run it: workgroup by
// workgroup and lane by lane, with the kernel's index arithmetic, its sums through the shared array and its partials.  The tile's shared
// inversion is replaced by one inversion per lane of the same operand (the product tree returns the same canonical values).  Scalars cross
// the boundary as 32 little-endian bytes in STANDARD form.
#include "verify_combine_multi.hpp"
#include <vector>

using namespace kzg;

static fr fr_from_le(const uint8_t *b) {
    fr o;
    for (int i = 0; i < 8; i++) o.l[i] = (uint32_t)b[4 * i] | (uint32_t)b[4 * i + 1] << 8 | (uint32_t)b[4 * i + 2] << 16 | (uint32_t)b[4 * i + 3] << 24;
    return o;
}
static void fr_to_le(const fr &v, uint8_t *b) {
    for (int i = 0; i < 8; i++)
        for (int k = 0; k < 4; k++) b[4 * i + k] = (uint8_t)(v.l[i] >> (8 * k));
}
static fr mont_in(const uint8_t *b) { return to_mont<FrP>(fr_from_le(b)); }
static void mont_out(const fr &v, uint8_t *b) { fr_to_le(from_mont<FrP>(v), b); }

extern "C" {
// combine_multi_row_scalars over n rows: r, r x^np and the base x^-1 (0 for x == 0 and for dead rows), 32 bytes each
void vcm_row_scalars(const uint8_t *seed32, const uint64_t *idx, const uint8_t *live, const uint8_t *xs32, uint64_t np, uint64_t n, uint8_t *r32, uint8_t *rxp32,
                     uint8_t *base32) {
    const combine_seed seed = combine_seed_from_bytes(seed32);
    for (uint64_t t = 0; t < n; t++) {
        const fr x = mont_in(xs32 + 32 * t);
        const fr xi = inv<FrP>(combine_multi_inverse_operand(live[t] != 0, x));
        fr r, rxp, base;
        combine_multi_row_scalars(seed, idx[t], live[t] != 0, x, xi, np, r, rxp, base);
        mont_out(r, r32 + 32 * t); mont_out(rxp, rxp32 + 32 * t); mont_out(base, base32 + 32 * t);
    }
}
// combine_multi_coeff_weight for j = 0 .. np - 1
void vcm_coeff_weights(const uint8_t *r32, const uint8_t *base32, uint64_t np, uint8_t *out32) {
    const fr r = mont_in(r32), base = mont_in(base32);
    for (uint64_t j = 0; j < np; j++) mont_out(combine_multi_coeff_weight(r, base, (uint32_t)j), out32 + 32 * j);
}
// k_combine_multi_poly + k_combine_multi_fold over `count` rows (rows row0 .. of the call) in groups of R: coef = count x np coefficients;
// sc = groups x (2 R + 1) scalars (r at j, r x^np at R + j, -1 at 2 R), J = groups x np.  Returns the number of groups, or 0 when a lane would
// have read a coefficient outside coef.
uint64_t vcm_groups(const uint8_t *seed32, const uint8_t *xs32, const uint8_t *coef32, uint64_t np, uint64_t row0, uint64_t count, uint64_t R, uint8_t *sc32, uint8_t *J32) {
    const combine_seed seed = combine_seed_from_bytes(seed32);
    const uint64_t G = combine_group_count(count, R), stride = combine_term_stride(R), T = combine_multi_tiles(R);
    const uint32_t L = COMBINE_MULTI_TILE;
    std::vector<fr> xs(count), coef(count * np), sc(G * stride, one<FrP>()), partials(G * T * np, one<FrP>());   // (ones: a slot the kernel forgets shows)
    for (uint64_t t = 0; t < count; t++) xs[t] = mont_in(xs32 + 32 * t);
    for (uint64_t t = 0; t < count * np; t++) coef[t] = mont_in(coef32 + 32 * t);
    for (uint64_t g = 0; g < G; g++)
        for (uint64_t t = 0; t < T; t++) {
            std::vector<fr> s_r(L), s_base(L), part(L);
            const uint64_t first = combine_multi_tile_row(g, t, R);
            for (uint32_t tid = 0; tid < L; tid++) {                                          // phase A
                const bool live = combine_multi_row_live(t, tid, first, R, count);
                const fr x = live ? xs[first + tid] : zero<FrP>();
                const fr xi = inv<FrP>(combine_multi_inverse_operand(live, x));
                fr r, rxp, base;
                combine_multi_row_scalars(seed, row0 + first + tid, live, x, xi, np, r, rxp, base);
                const uint64_t slot = t * L + tid;
                if (slot < R) { sc[g * stride + slot] = r; sc[g * stride + R + slot] = rxp; }
                s_r[tid] = r; s_base[tid] = base;
            }
            for (uint32_t tid = 0; tid < L; tid++) {                                          // phase B
                const uint32_t j = combine_multi_lane_coeff(tid, np);
                fr acc = zero<FrP>();
                for (uint32_t k = 0; k < (uint32_t)np; k++) {
                    const uint32_t l = combine_multi_lane_row(tid, k, np);
                    if (!combine_multi_row_live(t, l, first, R, count)) break;
                    const uint64_t at = first * np + (uint64_t)k * L + tid;
                    if (at >= count * np || at != (first + l) * np + j) return 0;
                    acc = add(acc, mul(combine_multi_coeff_weight(s_r[l], s_base[l], j), coef[at]));
                }
                part[tid] = acc;
            }
            for (uint32_t off = L / 2; off >= np; off >>= 1)
                for (uint32_t tid = 0; tid < off; tid++) part[tid] = add(part[tid], part[tid + off]);
            for (uint32_t tid = 0; tid < np; tid++) partials[combine_multi_partial_at(g, t, R, np) + tid] = part[tid];
        }
    for (uint64_t i = 0; i < G * np; i++) {                                                   // the fold, lane i
        const uint64_t g = i / np, j = i % np;
        mont_out(combine_multi_fold(partials.data(), g, R, np, j), J32 + 32 * i);
        if (j == 0) sc[g * stride + 2 * R] = combine_multi_last_scalar();
    }
    for (uint64_t i = 0; i < G * stride; i++) mont_out(sc[i], sc32 + 32 * i);
    return G;
}
}

#ifdef VCM_MAIN
// stand-alone run (sanitizer builds): a call with a full tile, a tile of one row, a short last group and dead rows inside a tile
#include <cstdio>
int main() {
    const uint64_t count = 600, np = 8;
    std::vector<uint8_t> seed(32, 7), xs(32 * count), coef(32 * count * np);
    for (size_t i = 0; i < xs.size(); i++) xs[i] = i % 32 == 31 ? 0 : (uint8_t)(i * 131 + 5);
    for (size_t i = 0; i < coef.size(); i++) coef[i] = i % 32 == 31 ? 0 : (uint8_t)(i * 29 + 3);
    for (uint64_t R : {5ull, 257ull, 300ull, 1024ull}) {
        const uint64_t G = (count + R - 1) / R;
        std::vector<uint8_t> sc(32 * G * (2 * R + 1)), J(32 * G * np);
        if (vcm_groups(seed.data(), xs.data(), coef.data(), np, 3, count, R, sc.data(), J.data()) != G) { printf("FAIL at R = %llu\n", (unsigned long long)R); return 1; }
    }
    printf("ok\n");
    return 0;
}
#endif
