"""Batches of KZG proofs checked by random linear combination per group of rows (kzg_hip_check_proof_single_batch_combined,
kzg_hip_eth_verify_kzg_proof_batch_combined; k_verify_combine.hip): the mask is the per-row entry's on the crafted rows of tests/verify_cases.py,
errors that cancel under equal weights are caught, only a failing group is re-checked, sums that double or vanish pass, A_g and B_g are the
points Python computes, and the routing switches do what README says, and a call that spans two chunks gives the per-row entry's output.  Group size and route are set
through the per-call switches."""
import ctypes as C
import hashlib
import json
import os
import random
import threading

import numpy as np
import pytest

import pairing_ref as pr
import verify_cases as vc
import verify_images as vi
from oracle import koracle as ko

pytestmark = pytest.mark.gpu

HERE = os.path.dirname(os.path.abspath(__file__))
GOLDEN = os.path.join(HERE, "golden")
S_TEST = 1927409816240961209460912649124
R = vc.R
R384 = pow(2, 384, pr.P)
SEED = hashlib.sha256(b"test_gpu_verify_combine").digest()


@pytest.fixture(scope="module")
def kz():
    import gokzg_amd
    assert gokzg_amd.device_count() >= 1, "no gfx950 device: the HIP path is the only path"
    return gokzg_amd


def g2_kilic(Q):
    u64s = lambda v: [(v >> (64 * i)) & (2 ** 64 - 1) for i in range(6)]
    return np.array([[u64s(c * R384 % pr.P) for c in coord] for coord in (Q[0], Q[1], (1, 0))], dtype=np.uint64)


@pytest.fixture(scope="module")
def ks16(kz):
    fs = kz.FFTSettings(5)
    ks = kz.KZGSettings(fs, ko.generate_testing_setup_g1(S_TEST, 33))
    ks.set_secret_g2(np.stack([g2_kilic(pr.G2_GEN), g2_kilic(pr.g2_mul(pr.G2_GEN, S_TEST % pr.R))]))
    yield ks
    ks.close()
    fs.close()


class Rows:
    """scalar rows (name, c, t, x, y, want) with their images, built once"""

    def __init__(self, rows, rng):
        self.rows = rows
        self.cs, self.pis, self.xs, self.ys = vi.single_images(rows, rng)
        self.want = [bool(r[5]) for r in rows]

    def take(self, idx):
        idx = list(idx)
        out = Rows.__new__(Rows)
        out.rows = [self.rows[i] for i in idx]
        out.cs, out.pis, out.xs, out.ys = (np.ascontiguousarray(a[idx]) for a in (self.cs, self.pis, self.xs, self.ys))
        out.want = [self.want[i] for i in idx]
        return out

    def arrays(self):
        return self.cs, self.pis, self.xs, self.ys


@pytest.fixture(scope="module")
def crafted(ks16):
    """every single row of verify_cases, and the per-row entry's mask on them (computed once, shared)"""
    r = Rows(vc.single_rows(S_TEST, random.Random(1)), random.Random(61))
    r.per_row = [bool(g) for g in ks16.check_proof_single_batch(*r.arrays())]
    assert r.per_row == r.want and True in r.want and False in r.want
    return r


def valid_rows(rng, n):
    rows = []
    for k in range(n):
        t, x, y = vc.rand_fr(rng), vc.rand_fr(rng), vc.rand_fr(rng)
        c = (y + (S_TEST - x) * t) % R
        rows.append(("valid%d" % k, c, t, x, y, True))
    return rows


def route(monkeypatch, mode, rows):
    for name, v in (("KZG_HIP_VERIFY_COMBINE", mode), ("KZG_HIP_VERIFY_COMBINE_ROWS", rows)):
        if v is None:
            monkeypatch.delenv(name, raising=False)
        else:
            monkeypatch.setenv(name, str(v))


# ---------------- 1. crafted rows, mask parity ----------------
@pytest.mark.parametrize("rows_per_group", [5, 64, None])
@pytest.mark.parametrize("shuffled", [False, True])
def test_crafted_rows_mask_parity(kz, ks16, crafted, monkeypatch, rows_per_group, shuffled):
    route(monkeypatch, "always", rows_per_group)
    idx = list(range(len(crafted.rows)))
    if shuffled:
        random.Random(62).shuffle(idx)
    sub = crafted.take(idx)
    got = [bool(g) for g in ks16.check_proof_single_batch_combined(*sub.arrays(), seed=SEED)]
    bad = [(r[0], g, w) for r, g, w in zip(sub.rows, got, sub.want) if g != w]
    assert not bad, bad
    assert got == [crafted.per_row[i] for i in idx]
    st = kz.combine_stats()
    want_rows = rows_per_group or 1024
    assert st["route"] == "combined" and st["rows"] == want_rows and st["groups"] == -(-len(idx) // want_rows)
    # exactly the groups that hold an invalid row were re-checked
    failing = [g for g in range(st["groups"]) if not all(sub.want[g * want_rows:(g + 1) * want_rows])]
    assert st["failed"] == len(failing)
    assert st["rechecked"] == sum(len(sub.want[g * want_rows:(g + 1) * want_rows]) for g in failing)


# ---------------- 2. errors that cancel under equal weights ----------------
def test_cancelling_errors_are_caught(kz, ks16, monkeypatch):
    """two rows with the same x and y + d, y' - d, and two with c + d, c' - d: each pair's errors cancel in an unweighted (or equally
    weighted) sum, so such a sum passes the group; every one of the four rows is invalid and its neighbours are valid"""
    rng = random.Random(63)
    rows = valid_rows(rng, 12)
    d = vc.rand_fr(rng)
    x = rows[2][3]
    t7 = rows[7][2]
    rows[7] = ("pair", (rows[7][4] + (S_TEST - x) * t7) % R, t7, x, rows[7][4], True)   # row 7 at row 2's x, still valid
    spoil = {2: (0, -d), 7: (0, d), 4: (d, 0), 9: (-d, 0)}                               # index -> (change of c, change of y)
    for i, (dc, dy) in spoil.items():
        n, c, t, xx, y, _ = rows[i]
        rows[i] = (n + "_spoiled", (c + dc) % R, t, xx, (y + dy) % R, False)
    assert rows[2][3] == rows[7][3]
    for r in rows:
        assert vc.single_want(S_TEST, *r[1:5]) == r[5]
    assert sum(r[1] - r[4] + (r[3] - S_TEST) * r[2] for r in rows) % R == 0              # the unweighted sum of all twelve equations holds
    rr = Rows(rows, rng)
    for per_group in (64, None, 5):
        route(monkeypatch, "always", per_group)
        got = [bool(g) for g in ks16.check_proof_single_batch_combined(*rr.arrays(), seed=SEED)]
        assert got == [i not in spoil for i in range(12)], per_group
        if per_group != 5:
            assert kz.combine_stats()["failed"] == 1 and kz.combine_stats()["rechecked"] == 12
    assert got == [bool(g) for g in ks16.check_proof_single_batch(*rr.arrays())]


# ---------------- 3. group edges ----------------
@pytest.fixture(scope="module")
def eleven():
    """eleven valid rows and, for every index, the same rows with that one spoiled (y + 1)"""
    rng = random.Random(64)
    good = Rows(valid_rows(rng, 11), rng)
    spoiled = {}
    for i in range(11):
        ys = good.ys.copy()
        ys[i] = ko.fr_from_ints([(good.rows[i][4] + 1) % R])[0]
        spoiled[i] = ys
    return good, spoiled


@pytest.mark.parametrize("count", [1, 4, 5, 6, 11])
def test_group_edges_at_five_rows_per_group(kz, ks16, eleven, monkeypatch, count):
    route(monkeypatch, "always", 5)
    good, spoiled = eleven
    cs, pis, xs, ys = (a[:count] for a in good.arrays())
    groups = -(-count // 5)
    assert ks16.check_proof_single_batch_combined(cs, pis, xs, ys, seed=SEED).all()
    assert kz.combine_stats() == dict(kz.combine_stats(), route="combined", groups=groups, failed=0, rechecked=0)
    for at in sorted({i for i in (0, 4, 5, count - 1) if i < count}):
        got = [bool(g) for g in ks16.check_proof_single_batch_combined(cs, pis, xs, spoiled[at][:count], seed=SEED)]
        assert got == [i != at for i in range(count)], at
        st = kz.combine_stats()
        g = at // 5
        assert (st["groups"], st["failed"], st["rechecked"]) == (groups, 1, min(count, 5 * g + 5) - 5 * g), (at, st)


# ---------------- 4. degenerate sums ----------------
def test_degenerate_sums_pass_without_a_recheck(kz, ks16, crafted, monkeypatch):
    """64 times the same valid row (every bucket that holds two terms doubles), a group of constant polynomials (every proof is infinity: A_g is
    infinity) and a group of zero polynomials (A_g and B_g are infinity)"""
    rng = random.Random(65)
    one = valid_rows(rng, 1) * 64
    x = [vc.rand_fr(rng) for _ in range(5)]
    y = [vc.rand_fr(rng) for _ in range(5)]
    constant = [("constant/valid%d" % k, y[k], 0, x[k], y[k], True) for k in range(5)]
    zero = [("constant/all_zero%d" % k, 0, 0, x[k], 0, True) for k in range(5)]
    built = {id(rows): Rows(rows, rng) for rows in (one, constant, zero)}
    built[0] = Rows(constant + constant, rng)
    built[1] = Rows(zero + constant + zero, rng)
    for key, per_group in ((id(one), 64), (id(one), None), (id(one), 5), (id(constant), 5), (0, 5), (id(zero), 5), (1, 5)):
        route(monkeypatch, "always", per_group)
        rr = built[key]
        assert ks16.check_proof_single_batch_combined(*rr.arrays(), seed=SEED).all(), (rr.rows[0][0], per_group)
        st = kz.combine_stats()
        assert st["route"] == "combined" and st["failed"] == 0 and st["rechecked"] == 0, (rr.rows[0][0], per_group, st)
    # the sums themselves (rows per group is still 5): zero polynomials give infinity twice; constant ones A_g = infinity, and B_g = sum r_i C_i -
    # (sum r_i y_i) G1 is infinity too, but only as the sum of an MSM that is not
    a, b = ks16.test_combine_points(*built[1].arrays(), SEED)
    inf = ko.g1_zero(1)[0]
    assert a.shape == (3, 3, 6) and all(np.array_equal(p, inf) for p in list(a) + list(b))


# ---------------- 5. pinned combination ----------------
def weight(seed, i):
    return int.from_bytes(hashlib.sha256(seed + b"KZGHIPRC" + i.to_bytes(8, "little")).digest()[:16], "little")


def want_points(rows, seed, per_group):
    """(A_g, B_g) as images: every input is a known multiple of the generator, so each sum is one oracle multiplication"""
    a, b = [], []
    for g0 in range(0, len(rows), per_group):
        ka = kb = 0
        for i, (_, c, t, x, y, _) in list(enumerate(rows))[g0:g0 + per_group]:
            r = weight(seed, i)
            ka += r * t
            kb += r * c + (r * x % R) * t - r * y
        a.append(vi.g1_scalar(ka % R)); b.append(vi.g1_scalar(kb % R))
    return np.stack(a), np.stack(b)


def test_pinned_combination(kz, ks16, crafted, monkeypatch):
    route(monkeypatch, "always", 5)
    names = ("ordinary/valid0", "ordinary/y+1_0", "constant/valid", "edge_x/r-1_valid", "edge_y/r-1_valid", "add_doubles/x=s/2", "sub_cancels/x=s",
             "generator/pi=-G", "edge_x/k2_max_valid", "ordinary/t+1_1", "constant/all_zero")
    idx = [[r[0] for r in crafted.rows].index(n) for n in names]
    sub = crafted.take(idx)
    assert len(sub.rows) == 11 and False in sub.want
    a, b = ks16.test_combine_points(*sub.arrays(), SEED)
    wa, wb = want_points(sub.rows, SEED, 5)
    assert a.shape == wa.shape == (3, 3, 6)
    assert np.array_equal(a, wa) and np.array_equal(b, wb)
    seed2 = hashlib.sha256(SEED).digest()
    a2, b2 = ks16.test_combine_points(*sub.arrays(), seed2)
    wa2, wb2 = want_points(sub.rows, seed2, 5)
    assert np.array_equal(a2, wa2) and np.array_equal(b2, wb2)
    assert not np.array_equal(a2[0], a[0]) and not np.array_equal(b2[0], b[0])
    masks = [[bool(g) for g in ks16.check_proof_single_batch_combined(*sub.arrays(), seed=s)] for s in (SEED, seed2, None, None)]
    assert masks == [sub.want] * 4


# ---------------- 6. the default group size ----------------
def test_three_thousand_rows_at_the_default_group_size(kz, ks16, crafted, monkeypatch):
    route(monkeypatch, "always", None)
    valid = [i for i, w in enumerate(crafted.want) if w]
    bad_src = [r[0] for r in crafted.rows].index("ordinary/y+1_1")
    idx = [valid[k % len(valid)] for k in range(3000)]
    idx[2500] = bad_src
    sub = crafted.take(idx)
    got = ks16.check_proof_single_batch_combined(*sub.arrays(), seed=SEED)
    assert list(np.nonzero(~got)[0]) == [2500]
    st = kz.combine_stats()
    assert (st["rows"], st["groups"], st["failed"], st["rechecked"]) == (1024, 3, 1, 3000 - 2048), st


# ---------------- 7. the eth form on the golden setup ----------------
@pytest.fixture(scope="module")
def eth(kz):
    fx = json.load(open(os.path.join(GOLDEN, "trusted_setup_g2.json")))
    fs = kz.FFTSettings(12)
    lag = ko.g1_decompress(np.frombuffer(open(os.path.join(GOLDEN, "trusted_setup_g1_lagrange.bin"), "rb").read(), dtype=np.uint8))
    e = kz.EthSettings(fs, lag)
    e.set_setup_g2(fs.g2_from_compressed(np.frombuffer(b"".join(bytes.fromhex(h) for h in fx["setup_G2"][:2]), dtype=np.uint8)))
    yield e
    e.close(); fs.close()


def test_eth_rows_with_malformed_neighbours(kz, eth, monkeypatch):
    route(monkeypatch, "always", 5)
    rows = {r[0]: r for r in vi.eth_rows(1337, random.Random(4))}
    valid = [r for r in rows.values() if r[5] == 1]
    z_ge_r, bad_c, wrong_y = rows["bytes/z=2^256-1"], rows["bytes/commitment_outside_g1"], rows["ordinary/y+1_0"]
    assert (z_ge_r[5], bad_c[5], wrong_y[5]) == (2, 3, 0) and len(valid) >= 12
    v = iter(valid)
    # groups of five: {v v 2 v v} {v 3 v v v} {v v v 0 v} {v}
    batch = [next(v), next(v), z_ge_r, next(v), next(v), next(v), bad_c, next(v), next(v), next(v), next(v), next(v), next(v), wrong_y, next(v), next(v)]
    arrays = vi.eth_arrays(batch)
    got = eth.verify_kzg_proof_batch_combined(*arrays, seed=SEED)
    assert list(got) == [r[5] for r in batch] and list(got) == list(eth.verify_kzg_proof_batch(*arrays))
    st = kz.combine_stats()
    assert (st["route"], st["groups"], st["failed"], st["rechecked"]) == ("combined", 4, 1, 5), st      # the malformed rows alone cause no re-check
    only_malformed = [r for r in batch if r is not wrong_y]
    arrays = vi.eth_arrays(only_malformed)
    got = eth.verify_kzg_proof_batch_combined(*arrays, seed=None)
    assert list(got) == [r[5] for r in only_malformed] and list(got) == list(eth.verify_kzg_proof_batch(*arrays))
    st = kz.combine_stats()
    assert (st["groups"], st["failed"], st["rechecked"]) == (3, 0, 0), st
    # a group of malformed rows only, and the per-row route of the same entry
    arrays = vi.eth_arrays([z_ge_r, bad_c, bad_c, z_ge_r, bad_c, wrong_y])
    assert list(eth.verify_kzg_proof_batch_combined(*arrays, seed=SEED)) == [2, 3, 3, 2, 3, 0]
    assert kz.combine_stats()["failed"] == 1 and kz.combine_stats()["rechecked"] == 1
    route(monkeypatch, "never", 5)
    assert list(eth.verify_kzg_proof_batch_combined(*arrays, seed=SEED)) == [2, 3, 3, 2, 3, 0]
    assert kz.combine_stats()["route"] == "per_row"


# ---------------- 8. concurrency ----------------
def test_eight_threads_on_one_handle(kz, ks16, crafted, monkeypatch):
    route(monkeypatch, "always", 5)
    sub = crafted.take(range(40))
    out, errs = [None] * 8, []

    def work(k):
        try:
            out[k] = [bool(g) for g in ks16.check_proof_single_batch_combined(*sub.arrays(), seed=SEED if k % 2 else None)]
        except Exception as e:   # noqa: BLE001
            errs.append(e)

    threads = [threading.Thread(target=work, args=(k,)) for k in range(8)]
    for t in threads:
        t.start()
    for t in threads:
        t.join()
    assert not errs, errs
    alone = [bool(g) for g in ks16.check_proof_single_batch_combined(*sub.arrays(), seed=SEED)]
    assert alone == sub.want and out == [alone] * 8


# ---------------- 9. routing ----------------
def test_routing_and_error_codes(kz, ks16, crafted, monkeypatch):
    route(monkeypatch, "never", 5)
    assert [bool(g) for g in ks16.check_proof_single_batch_combined(*crafted.arrays(), seed=SEED)] == crafted.per_row
    assert kz.combine_stats()["route"] == "per_row" and kz.combine_stats()["groups"] == 0
    route(monkeypatch, None, None)
    st = kz.combine_stats()
    assert st["rows"] == 1024 and len(crafted.rows) < st["combine_from"]
    assert [bool(g) for g in ks16.check_proof_single_batch_combined(*crafted.arrays(), seed=SEED)] == crafted.per_row
    assert kz.combine_stats()["route"] == "per_row"
    # a null mask with count > 0: the existing entry's code
    L = kz.lib()
    ptr = lambda a: a.ctypes.data_as(C.c_void_p)
    cs, pis, xs, ys = crafted.arrays()
    want = L.kzg_hip_check_proof_single_batch(ks16.h, ptr(cs), ptr(pis), ptr(xs), ptr(ys), 4, None)
    for mode in ("never", "always"):
        route(monkeypatch, mode, 5)
        assert L.kzg_hip_check_proof_single_batch_combined(ks16.h, ptr(cs), ptr(pis), ptr(xs), ptr(ys), 4, None, None) == want == kz.ERR_BAD_ARG
    # a handle with no G2 set
    fs = kz.FFTSettings(4)
    ks = kz.KZGSettings(fs, ko.generate_testing_setup_g1(S_TEST, 17))
    codes = []
    for call in (ks.check_proof_single_batch, ks.check_proof_single_batch_combined):
        with pytest.raises(kz.KzgError) as e:
            call(cs[:2], pis[:2], xs[:2], ys[:2])
        codes.append(e.value.status)
    assert codes == [kz.ERR_BAD_ARG, kz.ERR_BAD_ARG]
    ks.close(); fs.close()


# ---------------- 10. across a chunk boundary ----------------
# a chunk holds at most 1 024 groups: at five rows per group 5 127 rows split after 5 120, into 1 024 groups and 2 (of five and two rows)
CROSS, CROSS_BAD = 5127, (5119, 5120, 5126)      # the last row of the first chunk, the first of the second, the last of the call


def test_chunk_boundary_single(kz, ks16, crafted, monkeypatch):
    route(monkeypatch, "always", 5)
    valid = [i for i, w in enumerate(crafted.want) if w]
    idx = [valid[k % len(valid)] for k in range(CROSS)]
    for at in CROSS_BAD:
        idx[at] = [r[0] for r in crafted.rows].index("ordinary/y+1_1")
    sub = crafted.take(idx)
    got = ks16.check_proof_single_batch_combined(*sub.arrays(), seed=SEED)
    st = kz.combine_stats()
    assert np.array_equal(got, ks16.check_proof_single_batch(*sub.arrays())) and list(np.nonzero(~got)[0]) == list(CROSS_BAD)
    assert (st["route"], st["rows"], st["groups"], st["failed"], st["rechecked"]) == ("combined", 5, 1026, 3, 5 + 5 + 2), st


def test_chunk_boundary_eth(kz, eth, monkeypatch):
    """a status-2 and a status-3 row in groups of the first chunk that are otherwise valid, and a status-3 row beyond row 5 120, where both
    groups hold an invalid row: the status rows cause no re-check"""
    route(monkeypatch, "always", 5)
    rows = {r[0]: r for r in vi.eth_rows(1337, random.Random(4))}
    valid = [r for r in rows.values() if r[5] == 1]
    batch = [valid[k % len(valid)] for k in range(CROSS)]
    for at in CROSS_BAD:
        batch[at] = rows["ordinary/y+1_0"]
    batch[7] = batch[5122] = rows["bytes/commitment_outside_g1"]
    batch[5112] = rows["bytes/z=2^256-1"]
    arrays = vi.eth_arrays(batch)
    got = eth.verify_kzg_proof_batch_combined(*arrays, seed=SEED)
    st = kz.combine_stats()
    want = [r[5] for r in batch]
    assert (want[7], want[5112], want[5122]) == (3, 2, 3) and [i for i, w in enumerate(want) if w == 0] == list(CROSS_BAD)
    assert list(got) == want and list(got) == list(eth.verify_kzg_proof_batch(*arrays))
    assert (st["route"], st["rows"], st["groups"], st["failed"], st["rechecked"]) == ("combined", 5, 1026, 3, 5 + 5 + 2), st
