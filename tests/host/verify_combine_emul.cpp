// Host build of verify_combine.hpp for tests/test_verify_combine_host.py: the lane bodies of k_verify_combine.hip on the CPU -- the weights, a
// row's term scalars, and a whole group pass the way k_combine_scalars runs it (the partition into groups, the layout of a group's slice, the
// sum over a group and the generator's scalar).  Scalars cross the boundary as 32 little-endian bytes in STANDARD form.
#include "verify_combine.hpp"

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

extern "C" {
// r_i for n indices: 32 bytes each (the upper 16 are zero)
void vc_weights(const uint8_t *seed32, const uint64_t *idx, uint64_t n, uint8_t *out32) {
    const combine_seed seed = combine_seed_from_bytes(seed32);
    for (uint64_t t = 0; t < n; t++) fr_to_le(combine_weight_std(seed, idx[t]), out32 + 32 * t);
}
// k_combine_scalars over `count` rows in groups of R: sc = groups x (2 R + 1) scalars of 32 bytes (r at j, r x at R + j, -sum r y at 2 R).
// status may be null.  Returns the number of groups.
uint64_t vc_group_scalars(const uint8_t *seed32, const uint8_t *xs32, const uint8_t *ys32, const uint8_t *status, uint64_t row0, uint64_t count, uint64_t R, uint8_t *sc32) {
    const combine_seed seed = combine_seed_from_bytes(seed32);
    const uint64_t G = combine_group_count(count, R), stride = combine_term_stride(R);
    for (uint64_t g = 0; g < G; g++) {
        uint8_t *slice = sc32 + 32 * g * stride;
        fr u = zero<FrP>();
        for (uint64_t j = 0; j < R; j++) {
            const uint64_t t = combine_group_begin(g, R) + j;
            const bool live = t < count && !(status && status[t]);
            fr r, rx, ry;
            combine_row_scalars(seed, row0 + t, live, live ? to_mont<FrP>(fr_from_le(xs32 + 32 * t)) : zero<FrP>(), live ? to_mont<FrP>(fr_from_le(ys32 + 32 * t)) : zero<FrP>(), r, rx, ry);
            fr_to_le(from_mont<FrP>(r), slice + 32 * j);
            fr_to_le(from_mont<FrP>(rx), slice + 32 * (R + j));
            u = add(u, ry);
        }
        fr_to_le(from_mont<FrP>(combine_generator_scalar(u)), slice + 32 * 2 * R);
    }
    return G;
}
// the partition: out[2 g], out[2 g + 1] = first row and end of group g; returns the number of groups
uint64_t vc_partition(uint64_t count, uint64_t R, uint64_t *out) {
    const uint64_t G = combine_group_count(count, R);
    for (uint64_t g = 0; g < G; g++) { out[2 * g] = combine_group_begin(g, R); out[2 * g + 1] = combine_group_end(g, R, count); }
    return G;
}
// eth_combine_fields_lane over n rows: status, and z / y back in standard form (zero for a row with a status)
void vc_eth_fields(const uint8_t *zs32, const uint8_t *ys32, const uint8_t *c_bad, const uint8_t *pi_bad, uint64_t n, uint8_t *z_out32, uint8_t *y_out32, uint8_t *status) {
    for (uint64_t t = 0; t < n; t++) {
        fr z, y;
        uint8_t st = 0xff;
        eth_combine_fields_lane(zs32 + 32 * t, ys32 + 32 * t, c_bad[t], pi_bad[t], z, y, st);
        status[t] = st;
        fr_to_le(from_mont<FrP>(z), z_out32 + 32 * t);
        fr_to_le(from_mont<FrP>(y), y_out32 + 32 * t);
    }
}
}
