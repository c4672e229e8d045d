"""Batches of KZG multi-proofs checked by random linear combination per group of rows (kzg_hip_check_proof_multi_batch_combined;
k_verify_combine_multi.hip): the mask is the per-row entry's on the crafted rows of tests/verify_cases.py, errors that cancel under equal weights
are caught, only a failing group is re-checked, group and tile edges, J_g / A_g / B_g are what Python computes, the proofs of DAUsingFK20Multi
pass in whole groups, no commitment table is built, routing and status codes are the per-row entry's, and a call that spans two chunks gives
the per-row entry's output.  Rows are scalars: C = [c] G1,
pi = [t] G1 with the setup's secret known, so truth is modular arithmetic."""
import ctypes as C
import hashlib
import random
import threading

import numpy as np
import pytest

import pairing_ref as pr
import verify_cases as vc
import verify_images as vi
from oracle import koracle as ko

pytestmark = pytest.mark.gpu

S_TEST = 1927409816240961209460912649124
S = S_TEST % vc.R
R = vc.R
SEED = hashlib.sha256(b"test_gpu_verify_combine_multi").digest()
POLY = [1, 2, 3, 4, 7, 7, 7, 7, 13, 13, 13, 13, 13, 13, 13, 13]


@pytest.fixture(scope="module")
def kz():
    import gokzg_amd
    assert gokzg_amd.device_count() >= 1, "no gfx950 device: the HIP path is the only path"
    return gokzg_amd


@pytest.fixture(scope="module")
def g2_images():
    """[S_TEST^i] G2 for i <= 32 as Kilic images"""
    out, Q = [], pr.G2_GEN
    for _ in range(33):
        out.append(vi.g2_kilic(Q))
        Q = pr.g2_mul(Q, S)
    return np.stack(out)


@pytest.fixture(scope="module")
def ks16(kz, g2_images):
    fs = kz.FFTSettings(5)
    ks = kz.KZGSettings(fs, ko.generate_testing_setup_g1(S_TEST, 33))
    ks.set_secret_g2(g2_images)
    yield ks
    ks.close()
    fs.close()


def route(monkeypatch, mode, rows):
    for name, v in (("KZG_HIP_VERIFY_COMBINE", mode), ("KZG_HIP_VERIFY_COMBINE_ROWS", rows)):
        if v is None:
            monkeypatch.delenv(name, raising=False)
        else:
            monkeypatch.setenv(name, str(v))


def weight(seed, i):
    return int.from_bytes(hashlib.sha256(seed + b"KZGHIPRC" + i.to_bytes(8, "little")).digest()[:16], "little")


_W_INV = {}


def coefficients(ys):
    """the reference's interpolation of the zero-padded values: the naive inverse DFT (fft_fr.go:60-68)"""
    npad = vc.next_pow2(len(ys))
    if npad not in _W_INV:
        w = vc.inv(vc.root_of_unity(npad))
        _W_INV[npad] = [pow(w, k, R) for k in range(npad)]
    tab, n_inv = _W_INV[npad], vc.inv(npad)
    vals = list(ys) + [0] * (npad - len(ys))
    return [sum(v * tab[i * j % npad] for j, v in enumerate(vals)) * n_inv % R for i in range(npad)]


def interp_at_s(ys, x):
    """I'(s) = sum_j x^-j c[j] s^j with InvModFr(0) = 0"""
    q = vc.inv(x) * S % R
    return sum(c * pow(q, j, R) for j, c in enumerate(coefficients(ys))) % R


def valid_c(t, x, ys):
    n = len(ys)
    return (interp_at_s(ys, x) - (pow(x, vc.next_pow2(n), R) - pow(S, n, R)) * t) % R


def valid_rows(rng, n, k):
    """k valid rows (name, c, t, x, ys, n, True) with full-width scalars"""
    rows = []
    for i in range(k):
        t, x, ys = vc.rand_fr(rng), vc.rand_fr(rng), [vc.rand_fr(rng) for _ in range(n)]
        rows.append(("valid%d" % i, valid_c(t, x, ys), t, x, ys, n, True))
    return rows


class Rows:
    """multi rows of one length with their images, built once; C and pi alternate between Z = 1 and a random Jacobian Z"""

    def __init__(self, rows, rng, jacobian=True):
        self.rows = rows
        z = lambda on: rng.randrange(2, pr.P) if on and jacobian else None
        self.cs = np.stack([vi.g1_scalar(r[1], z(i % 2)) for i, r in enumerate(rows)])
        self.pis = np.stack([vi.g1_scalar(r[2], z(i % 3 == 0)) for i, r in enumerate(rows)])
        self.xs = ko.fr_from_ints([r[3] for r in rows])
        self.ys = np.stack([ko.fr_from_ints(r[4]) for r in rows])
        self.want = [bool(r[6]) for r in rows]

    def take(self, idx):
        idx = list(idx)
        out = Rows.__new__(Rows)
        out.rows = [self.rows[i] for i in idx]
        out.cs, out.pis, out.xs, out.ys = (np.ascontiguousarray(a[idx]) for a in (self.cs, self.pis, self.xs, self.ys))
        out.want = [self.want[i] for i in idx]
        return out

    def arrays(self):
        return self.cs, self.pis, self.xs, self.ys


def mask(got):
    return [bool(g) for g in got]


def expect_stats(kz, want, rows_per_group):
    """the combination ran, and exactly the groups that hold an invalid row failed and were re-checked"""
    st = kz.combine_stats()
    groups = -(-len(want) // rows_per_group)
    failing = [g for g in range(groups) if not all(want[g * rows_per_group:(g + 1) * rows_per_group])]
    assert st["route"] == "combined" and st["rows"] == rows_per_group and st["groups"] == groups, st
    assert st["failed"] == len(failing), (st, failing)
    assert st["rechecked"] == sum(len(want[g * rows_per_group:(g + 1) * rows_per_group]) for g in failing), st


# ---------------- 1. crafted rows, mask parity ----------------
@pytest.fixture(scope="module")
def crafted(ks16):
    """every multi row of verify_cases by length, and the per-row entry's mask on them (computed once, shared)"""
    rng = random.Random(71)
    rows = vc.multi_rows(S_TEST, random.Random(2))
    out = {}
    for n in vc.MULTI_NS:
        r = Rows([row for row in rows if row[5] == n], rng)
        r.per_row = mask(ks16.check_proof_multi_batch(*r.arrays()))
        assert r.per_row == r.want
        out[n] = r
    assert sum(len(r.rows) for r in out.values()) == len(rows)
    return out


@pytest.mark.parametrize("rows_per_group", [5, None])
@pytest.mark.parametrize("shuffled", [False, True])
def test_crafted_rows_mask_parity(kz, ks16, crafted, monkeypatch, rows_per_group, shuffled):
    route(monkeypatch, "always", rows_per_group)
    for n in vc.MULTI_NS:
        idx = list(range(len(crafted[n].rows)))
        if shuffled:
            random.Random(72 + n).shuffle(idx)
        sub = crafted[n].take(idx)
        got = mask(ks16.check_proof_multi_batch_combined(*sub.arrays(), seed=SEED))
        bad = [(r[0], g, w) for r, g, w in zip(sub.rows, got, sub.want) if g != w]
        assert not bad, bad
        assert got == [crafted[n].per_row[i] for i in idx]
        assert True in sub.want and False in sub.want
        expect_stats(kz, sub.want, rows_per_group or 1024)


# ---------------- 2. errors that cancel under equal weights ----------------
@pytest.mark.parametrize("case", ["commitments", "values"])
def test_cancelling_errors_are_caught(kz, ks16, monkeypatch, case):
    """two rows of one group with C + d G1 and C - d G1; two rows with equal x whose ys differ by +1 and -1 at the same index.  Either pair's
    errors cancel in an equally weighted sum of the rows' equations; both rows are invalid and their neighbours are valid"""
    rng = random.Random(73)
    n = 8
    rows = valid_rows(rng, n, 12)
    if case == "commitments":
        pair, d = (1, 3), vc.rand_fr(rng)
        for i, sign in zip(pair, (1, -1)):
            name, c, t, x, ys, _, _ = rows[i]
            rows[i] = (name + "_spoiled", (c + sign * d) % R, t, x, ys, n, False)
        assert sum(r[1] - interp_at_s(r[4], r[3]) + (pow(r[3], 8, R) - pow(S, n, R)) * r[2] for r in rows) % R == 0
    else:
        pair = (6, 8)
        x, t8, ys8 = rows[6][3], rows[8][2], rows[8][4]
        rows[8] = ("same_x", valid_c(t8, x, ys8), t8, x, ys8, n, True)
        for i, sign in zip(pair, (1, -1)):
            name, c, t, xx, ys, _, _ = rows[i]
            ys = list(ys); ys[3] = (ys[3] + sign) % R
            rows[i] = (name + "_spoiled", c, t, xx, ys, n, False)
        assert rows[6][3] == rows[8][3]
        assert sum(r[1] - interp_at_s(r[4], r[3]) + (pow(r[3], 8, R) - pow(S, n, R)) * r[2] for r in rows) % R == 0   # the unweighted sum holds
    for r in rows:
        assert vc.multi_want(S_TEST, *r[1:5]) == r[6], r[0]
    rr = Rows(rows, rng)
    want = [i not in pair for i in range(12)]
    for per_group in (5, 64):
        route(monkeypatch, "always", per_group)
        assert mask(ks16.check_proof_multi_batch_combined(*rr.arrays(), seed=SEED)) == want, per_group
        expect_stats(kz, want, per_group)
    assert mask(ks16.check_proof_multi_batch(*rr.arrays())) == want


# ---------------- 3. group and tile edges ----------------
POOL = 24


@pytest.fixture(scope="module")
def pools():
    """24 valid rows built by arithmetic per length, and one commitment that fits none of them"""
    rng = random.Random(74)
    out = {n: Rows(valid_rows(rng, n, POOL), rng) for n in (1, 8, 32, 12)}
    return out, vi.g1_scalar(vc.rand_fr(rng))


@pytest.mark.parametrize("count", [1, 4, 5, 6, 11])
def test_group_edges_at_five_rows_per_group(kz, ks16, pools, monkeypatch, count):
    route(monkeypatch, "always", 5)
    for n in (8, 12):
        sub = pools[0][n].take(range(count))
        assert ks16.check_proof_multi_batch_combined(*sub.arrays(), seed=SEED).all()
        expect_stats(kz, [True] * count, 5)
        for at in sorted({i for i in (0, 4, 5, count - 1) if i < count}):
            cs = sub.cs.copy(); cs[at] = pools[1]
            got = mask(ks16.check_proof_multi_batch_combined(cs, sub.pis, sub.xs, sub.ys, seed=SEED))
            want = [i != at for i in range(count)]
            assert got == want, (n, at)
            expect_stats(kz, want, 5)


@pytest.mark.parametrize("rows_per_group", [257, 300])
def test_six_hundred_rows_across_tiles(kz, ks16, pools, monkeypatch, rows_per_group):
    """R = 257: tiles of 256 and 1 rows and a last group of 86; R = 300: tiles of 256 and 44 rows.  All valid: no re-check.  Then one invalid
    row on either side of a tile's and a group's edge: only its group is re-checked and only that row is 0"""
    route(monkeypatch, "always", rows_per_group)
    idx = [i % POOL for i in range(600)]
    for n in (1, 8, 32, 12):
        sub = pools[0][n].take(idx)
        assert ks16.check_proof_multi_batch_combined(*sub.arrays(), seed=SEED).all(), n
        expect_stats(kz, [True] * 600, rows_per_group)
    sub = pools[0][8].take(idx)
    for at in (255, 256, 299, 300, 599):
        cs = sub.cs.copy(); cs[at] = pools[1]
        got = ks16.check_proof_multi_batch_combined(cs, sub.pis, sub.xs, sub.ys, seed=SEED)
        assert list(np.nonzero(~got)[0]) == [at]
        expect_stats(kz, [i != at for i in range(600)], rows_per_group)
        assert kz.combine_stats()["failed"] == 1


# ---------------- 4. pinned combination ----------------
@pytest.mark.parametrize("n", [2, 5, 32])
def test_pinned_combination(kz, ks16, monkeypatch, n):
    """J_g, A_g and B_g through the hook against Python: eleven rows in groups of five, x = 0, x = 1, pi = infinity and invalid rows among them"""
    route(monkeypatch, "always", 5)
    rng = random.Random(75 + n)
    npad = vc.next_pow2(n)
    rows = valid_rows(rng, n, 11)
    for at, x in ((1, 0), (7, 1)):
        _, _, t, _, ys, _, _ = rows[at]
        rows[at] = ("x=%d" % x, valid_c(t, x, ys), t, x, ys, n, True)
    rows[3] = ("pi_inf", interp_at_s(rows[3][4], rows[3][3]), 0, rows[3][3], rows[3][4], n, True)
    rows[9] = ("c+1", (rows[9][1] + 1) % R, rows[9][2], rows[9][3], rows[9][4], n, False)
    for r in rows:
        assert vc.multi_want(S_TEST, *r[1:5]) == r[6], r[0]
    rr = Rows(rows, rng)
    for seed in (SEED, hashlib.sha256(SEED).digest()):
        a, b, jj = ks16.test_combine_multi_points(*rr.arrays(), seed)
        assert a.shape == (3, 3, 6) and jj.shape == (3, npad, 4)
        for g in range(3):
            members = list(enumerate(rows))[5 * g:5 * g + 5]
            w = {i: weight(seed, i) for i, _ in members}
            want_j = [sum(w[i] * pow(vc.inv(r[3]), j, R) * coefficients(r[4])[j] for i, r in members) % R for j in range(npad)]
            assert ko.fr_to_ints(jj[g]) == want_j, (g, "J")
            ka = sum(w[i] * r[2] for i, r in members) % R
            kb = (sum(w[i] * r[1] + w[i] * pow(r[3], npad, R) % R * r[2] for i, r in members) - sum(c * pow(S, j, R) for j, c in enumerate(want_j))) % R
            assert np.array_equal(a[g], vi.g1_scalar(ka)), (g, "A")
            assert np.array_equal(b[g], vi.g1_scalar(kb)), (g, "B")
    assert mask(ks16.check_proof_multi_batch_combined(*rr.arrays(), seed=SEED)) == rr.want
    expect_stats(kz, rr.want, 5)


# ---------------- 5. degenerate sums ----------------
def test_degenerate_sums_pass_without_a_recheck(kz, ks16, pools, monkeypatch):
    """a group of valid rows whose proofs are all infinity (A_g is infinity), and 64 times the same valid row (every bucket that holds two
    terms doubles)"""
    rng = random.Random(76)
    n = 8
    pi_inf = []
    for k in range(5):
        x, ys = vc.rand_fr(rng), [vc.rand_fr(rng) for _ in range(n)]
        pi_inf.append(("pi_inf%d" % k, interp_at_s(ys, x), 0, x, ys, n, True))
    rr = Rows(pi_inf, rng)
    route(monkeypatch, "always", 5)
    assert ks16.check_proof_multi_batch_combined(*rr.arrays(), seed=SEED).all()
    expect_stats(kz, [True] * 5, 5)
    a, _, _ = ks16.test_combine_multi_points(*rr.arrays(), SEED)
    assert np.array_equal(a[0], ko.g1_zero(1)[0])
    same = pools[0][n].take([0] * 64)
    for per_group in (64, None, 5):
        route(monkeypatch, "always", per_group)
        assert ks16.check_proof_multi_batch_combined(*same.arrays(), seed=SEED).all(), per_group
        expect_stats(kz, [True] * 64, per_group or 1024)


# ---------------- 6. the coset proofs of DAUsingFK20Multi ----------------
def test_fk20_multi_proofs_verify_combined(kz, ks16, monkeypatch):
    """fk20_multi_test.go:86 through the combined entry: every coset proof passes in whole groups; one altered value fails exactly its row"""
    route(monkeypatch, "always", 5)
    chunk, n = 4, 16
    fk = kz.FK20MultiSettings(ks16, 2 * n, chunk)
    poly = ko.fr_from_ints(POLY)
    c = ks16.commit_to_poly(poly)
    proofs = fk.da_using_fk20_multi(poly)
    roots = ko.fr_to_ints(ks16.fs.expanded_roots_of_unity())[:32]
    stride = 32 // chunk
    evaluate = lambda z: sum(k * pow(z, i, R) for i, k in enumerate(POLY)) % R
    xs, yss = [], []
    for pos in range(2 * n // chunk):
        x = roots[ko.reverse_bits_limited(2 * n // chunk, pos)]
        xs.append(x); yss.append([evaluate(x * roots[j * stride] % R) for j in range(chunk)])
    count = len(xs)
    cs, ys = np.stack([c] * count), np.stack([ko.fr_from_ints(v) for v in yss])
    assert ks16.check_proof_multi_batch_combined(cs, proofs, ko.fr_from_ints(xs), ys, seed=SEED).all()
    expect_stats(kz, [True] * count, 5)
    yss[6][2] = (yss[6][2] + 1) % R
    ys = np.stack([ko.fr_from_ints(v) for v in yss])
    got = mask(ks16.check_proof_multi_batch_combined(cs, proofs, ko.fr_from_ints(xs), ys, seed=SEED))
    assert got == [i != 6 for i in range(count)]
    expect_stats(kz, got, 5)
    assert kz.combine_stats()["failed"] == 1
    fk.close()


# ---------------- 7. a verifier commits to nothing ----------------
def test_no_commitment_table_is_built(kz, g2_images, pools, monkeypatch):
    route(monkeypatch, "always", 5)
    fs = kz.FFTSettings(5)
    ks = kz.KZGSettings(fs, ko.generate_testing_setup_g1(S_TEST, 33))
    ks.set_secret_g2(g2_images)
    sub = pools[0][12].take(range(11))
    assert ks.check_proof_multi_batch_combined(*sub.arrays(), seed=SEED).all()
    assert kz.combine_stats()["route"] == "combined" and kz.combine_stats()["failed"] == 0
    assert ks.table_info()[2] == 0
    ks.close(); fs.close()


# ---------------- 8. routing and status codes ----------------
def test_routing_and_status_codes(kz, ks16, crafted, pools, g2_images, monkeypatch):
    sub = crafted[12]
    outs = {}
    for mode in ("never", "always"):
        route(monkeypatch, mode, 5)
        outs[mode] = ks16.check_proof_multi_batch_combined(*sub.arrays(), seed=SEED)
        want_route = "combined" if mode == "always" else "per_row"
        assert kz.combine_stats()["route"] == want_route and kz.combine_multi_route(12, len(sub.rows))[0] == want_route
        assert (kz.combine_stats()["groups"] == 0) == (mode == "never")
    assert outs["never"].tobytes() == outs["always"].tobytes() and mask(outs["never"]) == sub.per_row
    # np > 256 takes the per-row route whatever the switch says; 256 still combines
    assert kz.combine_multi_route(256, 10 ** 6)[0] == "combined" and kz.combine_multi_route(257, 10 ** 6)[0] == "per_row"
    # the default goes by the count
    route(monkeypatch, None, None)
    _, start = kz.combine_multi_route(12, 1)
    assert start > len(sub.rows)
    assert kz.combine_multi_route(12, start - 1)[0] == "per_row" and kz.combine_multi_route(12, start)[0] == "combined"
    got = ks16.check_proof_multi_batch_combined(*sub.arrays(), seed=None)
    assert mask(got) == sub.per_row and kz.combine_stats()["route"] == kz.combine_multi_route(12, len(sub.rows))[0]
    route(monkeypatch, "always", None)
    assert mask(ks16.check_proof_multi_batch_combined(*sub.arrays(), seed=None)) == sub.per_row       # a drawn seed, the default group size
    assert kz.combine_stats()["route"] == "combined"
    # status codes, in the per-row entry's order, on both routes
    L = kz.lib()
    ptr = lambda a: a.ctypes.data_as(C.c_void_p)
    cs, pis, xs, ys = pools[0][8].arrays()
    ok = np.zeros(POOL, dtype=np.uint8)
    small_fs, wide_fs = kz.FFTSettings(4), kz.FFTSettings(5)
    no_g2 = kz.KZGSettings(wide_fs, ko.generate_testing_setup_g1(S_TEST, 33))
    narrow = kz.KZGSettings(small_fs, ko.generate_testing_setup_g1(S_TEST, 17)); narrow.set_secret_g2(g2_images)       # W = 16 < len(SecretG2)
    # (np > n_setup, the entry's last code, cannot be reached through a handle: a setup holds at least W points and np <= W once n <= W)
    for mode in ("never", "always"):
        route(monkeypatch, mode, 5)
        both = lambda h, *a: (L.kzg_hip_check_proof_multi_batch(h, *a, ptr(ok)), L.kzg_hip_check_proof_multi_batch_combined(h, *a, None, ptr(ok)))
        args = (ptr(cs), ptr(pis), ptr(xs), ptr(ys))
        assert both(None, *args, 8, 4) == (kz.ERR_BAD_ARG,) * 2
        assert both(no_g2.h, *args, 8, 4) == (kz.ERR_BAD_ARG,) * 2
        assert both(no_g2.h, *args, 8, 0) == (kz.ERR_BAD_ARG,) * 2                                   # no SecretG2 comes before count == 0
        assert both(ks16.h, None, None, None, None, 8, 0) == (kz.OK,) * 2                            # count == 0 looks at nothing else
        assert both(ks16.h, *args, 0, 4) == (kz.ERR_BAD_ARG,) * 2                                    # n == 0
        assert both(ks16.h, ptr(cs), None, ptr(xs), ptr(ys), 8, 4) == (kz.ERR_BAD_ARG,) * 2
        assert L.kzg_hip_check_proof_multi_batch_combined(ks16.h, *args, 8, 4, None, None) == kz.ERR_BAD_ARG
        assert both(ks16.h, *args, 33, 4) == (kz.ERR_LEN_MISMATCH,) * 2                              # n >= len(SecretG2)
        assert both(narrow.h, *args, 17, 4) == (kz.ERR_TOO_WIDE,) * 2                                # n > W
        assert both(ks16.h, *args, 8, 4) == (kz.OK,) * 2 and list(ok[:4]) == [1] * 4
    for h in (no_g2, narrow):
        h.close()
    small_fs.close(); wide_fs.close()


# ---------------- 9. concurrency ----------------
def test_eight_threads_on_one_handle(kz, ks16, crafted, monkeypatch):
    """calls with 8 and with 32 values share the handle: the prepared SecretG2[n] is cached on its state"""
    route(monkeypatch, "always", 5)
    subs = {0: crafted[8], 1: crafted[32]}
    out, errs = [None] * 8, []

    def work(k):
        try:
            out[k] = mask(ks16.check_proof_multi_batch_combined(*subs[k % 2].arrays(), seed=SEED if k % 4 < 2 else None))
        except Exception as e:   # noqa: BLE001
            errs.append(e)

    threads = [threading.Thread(target=work, args=(k,)) for k in range(8)]
    for t in threads:
        t.start()
    for t in threads:
        t.join()
    assert not errs, errs
    serial = {k: mask(ks16.check_proof_multi_batch_combined(*subs[k].arrays(), seed=SEED)) for k in (0, 1)}
    assert serial[0] == subs[0].want and serial[1] == subs[1].want
    assert out == [serial[k % 2] for k in range(8)]


# ---------------- 10. across a chunk boundary ----------------
def test_chunk_boundary(kz, ks16, pools, monkeypatch):
    """a chunk holds at most 1 024 groups: at five rows per group 5 127 rows split after 5 120, into 1 024 groups and 2 (of five and two rows).
    One invalid row on the last row of the first chunk, the first of the second and the last of the call; the pool with the fewest values"""
    route(monkeypatch, "always", 5)
    bad = (5119, 5120, 5126)
    sub = pools[0][min(pools[0])].take([i % POOL for i in range(5127)])
    cs = sub.cs.copy()
    for at in bad:
        cs[at] = pools[1]
    got = ks16.check_proof_multi_batch_combined(cs, sub.pis, sub.xs, sub.ys, seed=SEED)
    st = kz.combine_stats()
    assert np.array_equal(got, ks16.check_proof_multi_batch(cs, sub.pis, sub.xs, sub.ys)) and list(np.nonzero(~got)[0]) == list(bad)
    expect_stats(kz, [i not in bad for i in range(5127)], 5)
    assert (st["groups"], st["failed"], st["rechecked"]) == (1026, 3, 5 + 5 + 2), st
