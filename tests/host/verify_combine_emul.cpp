// Host build of verify_combine.hpp for tests/test_verify_combine_host.py: the lane bodies of k_verify_combine.hip on the CPU -- the weights, a
// row's term scalars, and a whole group pass the way k_combine_scalars runs it (the partition into groups, the layout of a group's slice, the
// sum over a group and the generator's scalar), and the host loop of the _combined entries (combine_drive) over a model of the device.  Scalars
// cross the boundary as 32 little-endian bytes in STANDARD form.
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
// combine_drive over a CPU model of the device.  want[i] in {0, 1, 2, 3} is the byte row i has to end with: the model's chunk gives the 2 / 3
// rows their status and passes a group iff none of its rows wants 0, its recheck writes want[b .. e).  Both log their arguments -- (i0, k, G)
// per chunk, (b, e) per re-check -- and calls[0 .. 1] count them.  Call number fail_chunk / fail_recheck of its kind (from 0; -1: none) logs
// and returns `code` without writing; a chunk whose buffers do not arrive zeroed returns 99.  stats = groups, failed, rechecked.
int vc_drive(const uint8_t *want, uint64_t count, uint64_t R, uint64_t chunk_rows, int64_t fail_chunk, int64_t fail_recheck, int code, uint8_t *out, uint64_t *chunk_log,
             uint64_t *recheck_log, uint64_t *calls, uint64_t *stats) {
    combine_stats st{};
    calls[0] = calls[1] = 0;
    const int got = combine_drive(count, R, chunk_rows, out, st,
        [&](uint64_t i0, uint64_t k, uint64_t G, uint8_t *status, uint8_t *gok) -> int {
            uint64_t *log = chunk_log + 3 * calls[0];
            log[0] = i0; log[1] = k; log[2] = G;
            if ((int64_t)calls[0]++ == fail_chunk) return code;
            for (uint64_t t = 0; t < k; t++) if (status[t]) return 99;
            for (uint64_t g = 0; g < G; g++) if (gok[g]) return 99;
            for (uint64_t t = 0; t < k; t++) if (want[i0 + t] > 1) status[t] = want[i0 + t];
            for (uint64_t g = 0; g < G; g++) {
                gok[g] = 1;
                for (uint64_t t = combine_group_begin(g, R); t < combine_group_end(g, R, k); t++) if (!want[i0 + t]) gok[g] = 0;
            }
            return 0;
        },
        [&](uint64_t b, uint64_t e) -> int {
            uint64_t *log = recheck_log + 2 * calls[1];
            log[0] = b; log[1] = e;
            if ((int64_t)calls[1]++ == fail_recheck) return code;
            for (uint64_t i = b; i < e; i++) out[i] = want[i];
            return 0;
        });
    stats[0] = st.groups; stats[1] = st.failed; stats[2] = st.rechecked;
    return got;
}
}
