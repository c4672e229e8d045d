"""The lazy F_p product with its high-word carry sweeps (field.hpp: sweep_hi in mont_core30, mont_sqr_core30, mont_core30_dot2) and the mixed addition
built on it (g1.hpp: g1x_madd_fast, g1x_acc::add), as the table-walk kernels and the FK20 stages run them.  Needs a real MI355X: run with `-m gpu`.
Integer work: bit-exact.

Table walk: a small table (signed 5-bit windows, 26 per GLV half; built in well under a second) on the 4096-point s = 1337 setup, in the three launch
shapes of k_fb_accumulate_glv -- one blob (windows of a point split among lanes), 33 blobs, 512 blobs (one workgroup per blob, the headline's shape:
lane t owns points t + 256 j).  Expected values come from the bucket pipeline on the same points (other kernels, another addition order), computed
once for all shapes, and from the pinned vector F.  Rows of special scalars are built from their GLV halves:

    k = +-(s1 m1 + m2 lambda)  with  m1 <= lambda / 2,  so that glv_split_signed returns exactly (m1, m2) and the signs chosen

* every window digit 2^(c-1) (the table's last entry, never negated) resp. 2^(c-1) + 1 (every window carries into the next and every entry is
  added negated), in either half, with equal and with opposite signs of the halves;
* 0, 1, r - 1;
* k_3 = +-1337^256 e, k_259 = e for e = 1 and e = r - 1: at one workgroup per blob lane 3 holds +-S_259 when it adds S_259 (e = 1) or -S_259
  (e = r - 1, the entry is negated before the addition): the fast path declines and the complete formulas double, or return infinity.
"""
import hashlib
import json
import os

import numpy as np
import pytest

from oracle import koracle as ko

pytestmark = pytest.mark.gpu

GOLDEN = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden")
DERIVED = json.load(open(os.path.join(GOLDEN, "derived_vectors.json")))
FK20_PINS = json.load(open(os.path.join(GOLDEN, "fk20_pins.json")))
R = ko.R_MOD
LAMBDA = 0xac45a4010001a40200000000ffffffff
S = 1337
N = 4096
BUDGET_GB, C = 0.2, 5            # 0.2 GB holds signed 5-bit windows: 16 entries x 26 windows x 4096 points = 164 MB
NWIN = (128 + C - 1) // C


def assert_points_equal(got, want):
    got, want = np.asarray(got).reshape(-1, 3, 6), np.asarray(want).reshape(-1, 3, 6)
    assert got.shape == want.shape
    bad = np.nonzero((got != ko.g1_affine(want)).any(axis=(1, 2)))[0]
    assert bad.size == 0, "first mismatching rows: %s" % bad[:8]


def glv_split(k):
    """glv_split_signed (go-kzg_amd/csrc/g1.hpp) on Python integers: (|k1|, k2, neg1, neg2)"""
    sg = k > (R - 1) // 2
    a = R - k if sg else k
    q = (a + LAMBDA // 2) // LAMBDA
    k1 = a - q * LAMBDA
    return abs(k1), q, sg ^ (k1 < 0), sg


def from_halves(m1, m2, neg1, neg2):
    """the scalar whose split is (m1, m2) with these signs"""
    a = (-m1 if neg1 != neg2 else m1) + m2 * LAMBDA
    assert 0 <= a <= (R - 1) // 2 and m1 <= LAMBDA // 2
    k = (R - a) % R if neg2 else a
    if a:
        assert glv_split(k) == (m1, m2, bool(neg1), bool(neg2)), (hex(m1), hex(m2), neg1, neg2)
    return k


def every_digit(pattern):
    """a half whose raw c-bit digits are all `pattern` below the top window (which must not carry out: the half stays below 2^125)"""
    return sum(pattern << (C * w) for w in range(NWIN - 1))


def special_scalars():
    last, last_neg = every_digit(1 << (C - 1)), every_digit((1 << (C - 1)) + 1)
    out = [0, 1, R - 1]
    for m1, m2 in ((last, last), (last_neg, last_neg), (last, last_neg), (last_neg, 0), (0, last_neg), (last, 0), (0, last), (1, 1), (12345, every_digit(7))):
        for neg1, neg2 in ((0, 0), (1, 1), (0, 1), (1, 0)):
            if neg1 != neg2 and not (m1 and m2):
                continue                             # an empty half takes the sign of the other one: the halves cannot differ in sign
            out.append(from_halves(m1, m2, neg1, neg2))
    return out


@pytest.fixture(scope="module")
def kz():
    import gokzg_amd
    assert gokzg_amd.device_count() >= 1, "no gfx950 device: the HIP path is the only path"
    return gokzg_amd


@pytest.fixture(scope="module")
def setup_1337():
    raw = np.frombuffer(open(os.path.join(GOLDEN, "trusted_setup_g1.bin"), "rb").read(), dtype=np.uint8)
    return ko.g1_decompress(raw)


@pytest.fixture(scope="module")
def walk(kz, setup_1337):
    """(settings with the small table, 512 rows, their commitments by the bucket pipeline) -- computed once, shared by every launch shape"""
    fs = kz.FFTSettings(12)
    ks = kz.KZGSettings(fs, setup_1337)
    ks.set_table_budget_gb(BUDGET_GB)
    base = np.stack([ko.synthetic_blob(1 + b) for b in range(8)])             # splitmix blobs; seed 1 is vector F's
    rows = np.stack([np.roll(base[b % 8], 5 * (b // 8), axis=0) for b in range(512)])
    spec = ko.fr_from_ints(special_scalars())
    n = len(spec)
    rows[1][7:7 + n] = spec                                                     # among ordinary coefficients of one lane group ...
    rows[2][::97][:n] = spec                                                    # ... spread over the lanes ...
    rows[32] = 0
    rows[32][:n] = spec                                                         # ... and alone (row 32: inside the batch of 33)
    rows[3] = 0                                                                 # an all-zero row: the point at infinity
    at = 4
    for sign in (1, -1):
        for e in (1, R - 1):
            rows[at] = 0
            rows[at][[3, 259]] = ko.fr_from_ints([sign * pow(S, 256, R) * e % R, e])
            rows[at + 4] = rows[at]
            rows[at + 4][515] = ko.fr_from_ints([0x1234567])[0]                 # the lane goes on after the doubling / from infinity
            at += 1
    bucket = kz.G1Points(fs, setup_1337)
    bucket.set_table_budget_gb(0)                                               # no table: the bucket pipeline
    want = bucket.lin_comb_batch(rows)
    bucket.close()
    yield ks, fs, rows, want
    ks.close()
    fs.close()


@pytest.mark.parametrize("batch", [1, 33, 512])
def test_table_walk_matches_the_bucket_pipeline_in_every_launch_shape(walk, setup_1337, batch):
    ks, fs, rows, want = walk
    got = ks.commit_to_poly_batch(rows[:batch])
    assert ks.table_info()[0] == C
    assert_points_equal(got, want[:batch])
    assert ko.g1_compress(np.asarray(got)[:1])[0].tobytes().hex() == DERIVED["F_blob_seed1"]["commit_monomial_s1337"]
    if batch == 1:
        # the one-shot call (fs.lin_comb_g1: bucket pipeline, nothing cached) and the SPLIT walk on the rows of special scalars
        assert_points_equal(fs.lin_comb_g1(setup_1337, rows[0]), want[0])
        for b in (1, 2, 3, 4, 5, 6, 7, 8, 9, 10, 11, 32):
            assert_points_equal(ks.commit_to_poly(rows[b]), want[b])
    if batch == 512:
        zero, twice = ko.g1_zero()[0], ko.g1_add(setup_1337[259], setup_1337[259])
        assert np.array_equal(np.asarray(got)[3], zero)                          # the zero row
        assert_points_equal(np.asarray(got)[4], twice)                           # S_259 + S_259
        assert_points_equal(np.asarray(got)[5], ko.g1_sub(zero, twice))          # -S_259 - S_259: the negated entry in the declined addition
        assert np.array_equal(np.asarray(got)[6], zero) and np.array_equal(np.asarray(got)[7], zero)   # -S_259 + S_259, S_259 - S_259


def test_equal_and_opposite_points_of_a_cached_set(kz):
    """a cached set of 8 points that holds one point twice and a point with its negative, with scalars that give both members of a pair the same digits.
    With 8 points every lane of the set's table walk holds one (point, window group), so the equal and the opposite partial sums meet in the block
    reduction (g1_quad / g1xq_add_fast, whose P == +-Q test is is_zero_mod_p_q), not in a lane's mixed addition; the complete formulas
    take over there.  The lane-level fallback with a negated entry is rows 4 .. 11 of the 512-blob case above (g1x_acc::add, which fb_walk_term
    calls too) and tests/host/fp_lazy_trims_test.cpp.  Against the oracle's MultiExp"""
    gen = ko.g1_generator()
    ks_ = ko.fr_from_ints([3, 5, 7, 11, 13, 17])
    a, b, c, d, e, f = (ko.g1_affine(ko.g1_mul(gen, k))[0] for k in ks_)
    pts = np.stack([a, a, b, ko.g1_sub(ko.g1_zero()[0], b), c, d, e, f])
    fs = kz.FFTSettings(4)
    cached = kz.G1Points(fs, pts)
    rng = np.random.default_rng(8)
    rnd = [int.from_bytes(rng.bytes(32), "little") % R for _ in range(8)]
    cases = []
    for k in (1, 2, 0x80, R - 1, LAMBDA, rnd[0]):
        for tail in (0, 1):
            sc = [k, k, k, k] + ([rnd[4], rnd[5], rnd[6], rnd[7]] if tail else [0, 0, 0, 0])   # 2 k A + k B - k B (+ an ordinary rest)
            cases.append(sc)
            cases.append([k, k, k, (R - k) % R] + sc[4:])                                         # 2 k A + 2 k B
            cases.append([k, (R - k) % R, k, k] + sc[4:])                                         # k A - k A: infinity when the rest is empty
    batch = np.stack([ko.fr_from_ints(sc) for sc in cases])
    got = cached.lin_comb_batch(batch)
    for i, sc in enumerate(cases):
        assert_points_equal(got[i], ko.lincomb_g1(pts, batch[i]))
    for i in (0, 1, 2, 5):
        assert_points_equal(cached.lin_comb(batch[i]), ko.lincomb_g1(pts, batch[i]))
    cached.close()
    fs.close()


def test_fk20_all_proofs_pin_and_batch(walk, kz):
    """the G1 transform stages inline the same products: DAUsingFK20 on 2048 coefficients against the oracle's byte pin, and a batch of three
    polynomials against the one-polynomial path"""
    ks, fs, _, _ = walk
    fk = kz.FK20SingleSettings(ks, 4096)
    polys = np.stack([ko.synthetic_blob(4 + b)[:2048] for b in range(3)])
    proofs = fk.da_using_fk20(polys[0])
    assert hashlib.sha256(fs.to_compressed_g1(proofs).tobytes()).hexdigest() == FK20_PINS["config4a_da_using_fk20_seed4"]["sha256"]
    got = fk.da_using_fk20_batch(polys)
    assert np.array_equal(np.asarray(got)[0], np.asarray(proofs))
    for b in (1, 2):
        assert np.array_equal(np.asarray(got)[b], np.asarray(fk.da_using_fk20(polys[b])))
    fk.close()
