"""Verification on the device (k_pairing.hip, capi_verify.hip): pairing values against the Python reference, batched PairingsVerify, the
reference's pairing-based proof tests restated (kzg_single_proofs_test.go, fk20_single_test.go, kzg_multi_proofs_test.go, fk20_multi_test.go),
a 4096-proof batch with tampered rows, and eth.VerifyKZGProof end to end on the trusted setup's G2 points (tests/golden/trusted_setup_g2.json).
Then the adversarial side: the crafted rows of tests/verify_cases.py (exceptional cases of the group law that are valid and invalid), G2 images
with Jacobian Z != 1, pairing values at batch size, the chunk loop of pairings_verify_batch, eth byte rows."""
import json
import os
import random
import time

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
POLY = [1, 2, 3, 4, 7, 7, 7, 7, 13, 13, 13, 13, 13, 13, 13, 13]
R384 = pow(2, 384, pr.P)
DEVICE_EXP = 3 * pr.FINAL_EXP   # pairing.hpp's final exponentiation


@pytest.fixture(scope="module")
def kz():
    import gokzg_amd
    assert gokzg_amd.device_count() >= 1, "no gfx950 device: the HIP path is the only path"
    return gokzg_amd


def u64s(v):
    return [(v >> (64 * i)) & (2 ** 64 - 1) for i in range(6)]


def g2_kilic(Q):   # affine reference point -> Kilic G2 image (3, 2, 6)
    if Q is None:
        return np.array([[u64s(0), u64s(0)], [u64s(R384), u64s(0)], [u64s(0), u64s(0)]], dtype=np.uint64)
    return np.array([[u64s(c * R384 % pr.P) for c in coord] for coord in (Q[0], Q[1], (1, 0))], dtype=np.uint64)


def g1_ints(pt):   # Kilic G1 image -> affine ints (None for infinity)
    a = ko.g1_affine(np.asarray(pt).reshape(1, 3, 6))[0]
    if not any(int(v) for v in a[2]):
        return None
    rinv = pow(R384, -1, pr.P)
    val = lambda row: sum(int(row[i]) << (64 * i) for i in range(6)) * rinv % pr.P
    return (val(a[0]), val(a[1]))


def g1_mul_int(k):
    return ko.g1_mul(ko.g1_generator(), ko.fr_from_ints([k % ko.R_MOD])[0])


def eval_poly(coeffs, x):
    return sum(c * pow(x, i, ko.R_MOD) for i, c in enumerate(coeffs)) % ko.R_MOD


@pytest.fixture(scope="module")
def g2_powers():   # [S_TEST^i] G2, i <= 32
    out, Q = [], pr.G2_GEN
    step = S_TEST % pr.R
    for i in range(33):
        out.append(Q)
        Q = pr.g2_mul(Q, step)
    return out


@pytest.fixture(scope="module")
def ks16(kz, g2_powers):
    fs = kz.FFTSettings(5)
    ks = kz.KZGSettings(fs, ko.generate_testing_setup_g1(S_TEST, 33))
    ks.set_secret_g2(np.stack([g2_kilic(Q) for Q in g2_powers]))
    yield ks
    ks.close()
    fs.close()


def test_pairing_values_match_the_reference(kz):
    fs = kz.FFTSettings(4)
    pts = [(3, pr.g2_mul(pr.G2_GEN, 5)), (1, pr.G2_GEN), (0, pr.G2_GEN), (7, None)]
    g1 = np.stack([g1_mul_int(a) if a else ko.g1_zero(1)[0] for a, _ in pts])
    g1[0] = ko.g1_add(g1[0], ko.g1_zero(1)[0])      # a Jacobian image as the oracle leaves it
    g2 = np.stack([g2_kilic(Q) for _, Q in pts])
    got = fs.pairing_test(g1, g2)
    for (a, Q), val in zip(pts, got):
        Pt = pr.g1_mul(pr.G1_GEN, a) if a else None
        want = pr.pairing(Pt, Q, DEVICE_EXP) if Pt and Q else pr.ONE12
        assert pr.from_tower([(val[2 * k], val[2 * k + 1]) for k in range(6)]) == want
    fs.close()


def test_pairings_verify_batch_mask(kz):
    fs = kz.FFTSettings(4)
    A = [g1_mul_int(a) for a in range(1, 18)]
    Qa = [g2_kilic(pr.g2_mul(pr.G2_GEN, a)) for a in range(1, 18)]
    inf1, inf2, P1, Q1 = ko.g1_zero(1)[0], g2_kilic(None), A[0], Qa[0]
    n = 1024
    a1, a2, b1, b2, want = [], [], [], [], []
    for i in range(n):
        a = i % 16                                   # [a+1] P vs ...
        if i % 97 == 5:                              # infinity on both sides: 1 == 1
            a1.append(inf1); a2.append(Q1); b1.append(P1); b2.append(inf2); want.append(True)
        elif i % 97 == 6:                            # infinity on one side only: 1 != e(P, Q)
            a1.append(inf1); a2.append(Q1); b1.append(P1); b2.append(Q1); want.append(False)
        elif i % 2 == 0:                             # e([a] P, Q) == e(P, [a] Q)
            a1.append(A[a]); a2.append(Q1); b1.append(P1); b2.append(Qa[a]); want.append(True)
        else:                                        # e([a] P, Q) != e(P, [a + 1] Q)
            a1.append(A[a]); a2.append(Q1); b1.append(P1); b2.append(Qa[a + 1]); want.append(False)
    got = fs.pairings_verify_batch(np.stack(a1), np.stack(a2), np.stack(b1), np.stack(b2))
    assert list(got) == want
    fs.close()


def test_check_proof_single_reference(kz, ks16):
    poly = ko.fr_from_ints(POLY)
    c = ks16.commit_to_poly(poly)
    proof = ks16.compute_proof_single(poly, 17)
    y = eval_poly(POLY, 17)
    ok = ks16.check_proof_single_batch(np.stack([c, c]), np.stack([proof, proof]), ko.fr_from_ints([17, 17]), ko.fr_from_ints([y, y + 1]))
    assert list(ok) == [True, False]


def test_fk20_all_proofs_verify(kz, ks16):
    fk = kz.FK20SingleSettings(ks16, 32)
    poly = ko.fr_from_ints(POLY)
    c = ks16.commit_to_poly(poly)
    proofs = fk.da_using_fk20(poly)
    roots = ko.fr_to_ints(ks16.fs.expanded_roots_of_unity())[:32]
    xs = ko.fr_from_ints(roots)
    ys = ko.fr_from_ints([eval_poly(POLY, x) for x in roots])
    order = [ko.reverse_bits_limited(32, i) for i in range(32)]      # fk20_single_test.go:41
    ok = ks16.check_proof_single_batch(np.stack([c] * 32), proofs[order], xs, ys)
    assert ok.all()
    fk.close()


def test_check_proof_multi_reference(kz, g2_powers):
    # kzg_multi_proofs_test.go: x = 5431, coset of 8 on a scale-3 settings object with 9 setup points
    fs = kz.FFTSettings(3)
    ks = kz.KZGSettings(fs, ko.generate_testing_setup_g1(S_TEST, 9))
    ks.set_secret_g2(np.stack([g2_kilic(Q) for Q in g2_powers[:9]]))
    fs16 = kz.FFTSettings(4)
    ks_c = kz.KZGSettings(fs16, ko.generate_testing_setup_g1(S_TEST, 17))
    poly = ko.fr_from_ints(POLY)
    c = ks_c.commit_to_poly(poly)
    roots = ko.fr_to_ints(fs.expanded_roots_of_unity())[:8]
    x = 5431
    ys = [eval_poly(POLY, x * w % ko.R_MOD) for w in roots]
    proof = ks.compute_proof_multi(poly, x, 8)
    ys_bad = list(ys); ys_bad[3] = (ys_bad[3] + 1) % ko.R_MOD
    ok = ks.check_proof_multi_batch(np.stack([c, c]), np.stack([proof, proof]), ko.fr_from_ints([x, x]),
                                    np.stack([ko.fr_from_ints(ys), ko.fr_from_ints(ys_bad)]))
    assert list(ok) == [True, False]
    # misuse: n beyond the stored G2 array; count 0
    with pytest.raises(kz.KzgError) as e:
        ks.check_proof_multi_batch(c[None], proof[None], ko.fr_from_ints([x]), np.zeros((1, 9, 4), dtype=np.uint64))
    assert e.value.status == kz.ERR_LEN_MISMATCH
    assert len(ks.check_proof_single_batch(np.zeros((0, 3, 6), dtype=np.uint64), np.zeros((0, 3, 6), dtype=np.uint64), ko.fr_empty(0),
                                           ko.fr_empty(0))) == 0
    assert len(ks.check_proof_multi_batch(np.zeros((0, 3, 6), dtype=np.uint64), np.zeros((0, 3, 6), dtype=np.uint64), ko.fr_empty(0),
                                          np.zeros((0, 8, 4), dtype=np.uint64))) == 0
    for h in (ks_c, ks):
        h.close()
    fs16.close(); fs.close()


def test_fk20_multi_proofs_verify(kz, ks16):
    # fk20_multi_test.go:86: every coset proof of DAUsingFK20Multi verifies against its coset of the extended domain
    chunk, n = 4, 16
    fk = kz.FK20MultiSettings(ks16, 2 * n, chunk)
    poly = ko.fr_from_ints(POLY)
    c = ks16.commit_to_poly(poly)
    proofs = fk.da_using_fk20_multi(poly)                      # 2n / chunk proofs, bit-reversed order
    roots = ko.fr_to_ints(ks16.fs.expanded_roots_of_unity())[:32]
    stride = 32 // chunk
    cs, ps, xs, yss = [], [], [], []
    for pos in range(2 * n // chunk):
        x = roots[ko.reverse_bits_limited(2 * n // chunk, pos)]
        coset = [x * roots[j * stride] % ko.R_MOD for j in range(chunk)]
        cs.append(c); ps.append(proofs[pos]); xs.append(x); yss.append(ko.fr_from_ints([eval_poly(POLY, z) for z in coset]))
    ok = ks16.check_proof_multi_batch(np.stack(cs), np.stack(ps), ko.fr_from_ints(xs), np.stack(yss))
    assert ok.all(), ok
    fk.close()


def test_check_proof_single_at_scale(kz, ks16):
    rng = np.random.default_rng(3)
    count = 4096
    polys_i = [[int(v) for v in rng.integers(0, 2 ** 62, 16)] for _ in range(64)]
    polys = np.stack([ko.fr_from_ints(p) for p in polys_i])
    rows = [i % 64 for i in range(count)]
    xs_i = [1000 + i for i in range(count)]
    proofs = ks16.compute_proof_single_batch(polys[rows], np.array(xs_i, dtype=np.uint64))
    commits = ks16.commit_to_poly_batch(polys) if hasattr(ks16, "commit_to_poly_batch") else np.stack([ks16.commit_to_poly(p) for p in polys])
    cs = commits[rows]
    ys_i = [eval_poly(polys_i[r], x) for r, x in zip(rows, xs_i)]
    want = [True] * count
    for i in range(0, count, 7):                                 # every 7th row tampered three ways
        kind = (i // 7) % 3
        if kind == 0:
            ys_i[i] = (ys_i[i] + 1) % ko.R_MOD
        elif kind == 1:
            xs_i[i] += 1
        else:
            proofs[i] = proofs[(i + 1) % count]
        want[i] = False
    ok = ks16.check_proof_single_batch(cs, proofs, ko.fr_from_ints(xs_i), ko.fr_from_ints(ys_i))
    assert list(ok) == want


def test_misuse_before_the_g2_setter(kz):
    fs = kz.FFTSettings(4)
    ks = kz.KZGSettings(fs, ko.generate_testing_setup_g1(S_TEST, 17))
    one = ko.fr_from_ints([1])
    with pytest.raises(kz.KzgError) as e:
        ks.check_proof_single_batch(ko.g1_generator()[None], ko.g1_generator()[None], one, one)
    assert e.value.status == kz.ERR_BAD_ARG
    ks.close(); fs.close()


def test_eth_verify_kzg_proof_batch(kz):
    fx = json.load(open(os.path.join(GOLDEN, "trusted_setup_g2.json")))
    fs = kz.FFTSettings(12)
    g2 = fs.g2_from_compressed(np.frombuffer(b"".join(bytes.fromhex(h) for h in fx["setup_G2"]), dtype=np.uint8))
    assert np.array_equal(g2[0], g2_kilic(pr.G2_GEN))
    with pytest.raises(kz.KzgError) as e:                      # one bad encoding fails the whole call
        fs.g2_from_compressed(np.frombuffer(bytes([0x80]) + bytes(95), dtype=np.uint8))
    assert e.value.status == kz.ERR_BAD_POINT
    lag = ko.g1_decompress(np.frombuffer(open(os.path.join(GOLDEN, "trusted_setup_g1_lagrange.bin"), "rb").read(), dtype=np.uint8))
    eth = kz.EthSettings(fs, lag)
    with pytest.raises(kz.KzgError):                           # before the setter
        eth.verify_kzg_proof_batch(np.zeros((1, 48), np.uint8), np.zeros((1, 32), np.uint8), np.zeros((1, 32), np.uint8), np.zeros((1, 48), np.uint8))
    eth.set_setup_g2(g2)
    nb = 4
    blobs_i = [ko.fr_to_ints(ko.synthetic_blob(1 + b)) for b in range(nb)]
    blobs = np.stack([np.frombuffer(b"".join(v.to_bytes(32, "little") for v in bi), dtype=np.uint8).reshape(4096, 32) for bi in blobs_i])
    commits, ok = eth.blob_to_kzg_commitment_batch(blobs)
    assert ok.all()
    zs_i = [(0x1234567890abcdef * (b + 3)) % ko.R_MOD for b in range(nb)]
    proofs, ys, ok = eth.compute_kzg_proof_batch(np.stack([ko.fr_from_ints(bi) for bi in blobs_i]), ko.fr_from_ints(zs_i))
    assert ok.all()
    le = lambda v: np.frombuffer(v.to_bytes(32, "little"), dtype=np.uint8)
    zs = np.stack([le(z) for z in zs_i])
    ysb = np.stack([le(y) for y in ko.fr_to_ints(ys)])
    assert list(eth.verify_kzg_proof_batch(commits, zs, ysb, proofs)) == [1] * nb
    # tampered proof bytes (another valid proof), z >= r, y >= r, an undecodable commitment
    bad_c, bad_z, bad_y, bad_p = commits.copy(), zs.copy(), ysb.copy(), proofs.copy()
    bad_p[0] = proofs[1]
    bad_z[1] = le(ko.R_MOD)
    bad_y[2] = le(2 ** 256 - 1)
    bad_c[3] = 0
    bad_c[3][0] = 0x80                                         # x = 0: (0, +-2) is on the curve but of order 3, outside G1 (subgroup check)
    assert list(eth.verify_kzg_proof_batch(bad_c, bad_z, bad_y, bad_p)) == [0, 2, 2, 3]
    # the pairing half of VerifyAggregateKZGProof (eth/eth.go:155-172) as one check
    proof_agg, comms = eth.compute_aggregate_kzg_proof(blobs)
    _, c_agg, z, y = eth.compute_aggregated_poly_and_commitment(blobs, comms)
    c48 = fs.to_compressed_g1(c_agg[None])
    z_le, y_le = le(ko.fr_to_ints(z[None])[0]), le(ko.fr_to_ints(y[None])[0])
    assert list(eth.verify_kzg_proof_batch(c48, z_le[None], y_le[None], proof_agg[None])) == [1]
    assert len(eth.verify_kzg_proof_batch(np.zeros((0, 48), np.uint8), np.zeros((0, 32), np.uint8), np.zeros((0, 32), np.uint8),
                                          np.zeros((0, 48), np.uint8))) == 0
    eth.close(); fs.close()


def test_close_then_reuse_needs_the_g2_setter_again(kz, g2_powers):
    # a handle made after the previous one was freed starts without G2 points, whatever address it gets
    g2 = np.stack([g2_kilic(Q) for Q in g2_powers[:17]])
    poly = ko.fr_from_ints(POLY)
    y = eval_poly(POLY, 17)
    for round_ in range(3):
        fs = kz.FFTSettings(4)
        ks = kz.KZGSettings(fs, ko.generate_testing_setup_g1(S_TEST, 17))
        c, proof = ks.commit_to_poly(poly), ks.compute_proof_single(poly, 17)
        with pytest.raises(kz.KzgError) as e:
            ks.check_proof_single_batch(c[None], proof[None], ko.fr_from_ints([17]), ko.fr_from_ints([y]))
        assert e.value.status == kz.ERR_BAD_ARG
        ks.set_secret_g2(g2)
        assert list(ks.check_proof_single_batch(c[None], proof[None], ko.fr_from_ints([17]), ko.fr_from_ints([y]))) == [True]
        ks.close(); fs.close()


def test_concurrent_checks_and_setters_on_one_handle(kz, g2_powers):
    # the checks of one handle from many threads while others re-set SecretG2 and multi checks grow the cache of prepared [s^n]G2
    import threading
    fs = kz.FFTSettings(5)
    ks = kz.KZGSettings(fs, ko.generate_testing_setup_g1(S_TEST, 33))
    g2 = np.stack([g2_kilic(Q) for Q in g2_powers])
    ks.set_secret_g2(g2)
    poly = ko.fr_from_ints(POLY)
    c = ks.commit_to_poly(poly)
    proof = ks.compute_proof_single(poly, 17)
    y = eval_poly(POLY, 17)
    roots = ko.fr_to_ints(fs.expanded_roots_of_unity())
    multi = []
    for m in (4, 8, 16):                                        # cosets of size m: n = m needs [s^m]G2; a polynomial of 2m coefficients
        pm = list(range(1, 2 * m + 1))                          # (ComputeProofMulti's proofs are valid for len(poly) <= 2n)
        x = 5431
        coset = [x * roots[j * (32 // m)] % ko.R_MOD for j in range(m)]
        multi.append((m, ks.commit_to_poly(ko.fr_from_ints(pm)), ks.compute_proof_multi(ko.fr_from_ints(pm), x, m), x,
                      ko.fr_from_ints([eval_poly(pm, z) for z in coset])))
    errors = []

    def single():
        for _ in range(4):
            ok = ks.check_proof_single_batch(np.stack([c, c]), np.stack([proof, proof]), ko.fr_from_ints([17, 17]), ko.fr_from_ints([y, y + 1]))
            if list(ok) != [True, False]:
                errors.append(("single", list(ok)))

    def multi_checks(m, cm, pr_, x, ys):
        for _ in range(2):
            ok = ks.check_proof_multi_batch(cm[None], pr_[None], ko.fr_from_ints([x]), ys[None])
            if list(ok) != [True]:
                errors.append(("multi", m, list(ok)))

    def setter():
        for _ in range(3):
            ks.set_secret_g2(g2)

    threads = [threading.Thread(target=single) for _ in range(4)] + [threading.Thread(target=setter) for _ in range(2)]
    threads += [threading.Thread(target=multi_checks, args=row) for row in multi]
    for t in threads:
        t.start()
    for t in threads:
        t.join()
    assert not errors, errors
    ks.close(); fs.close()


# ---------------- crafted rows (tests/verify_cases.py), Jacobian G2 images, chunk edges ----------------
# Truth values come from scalars (the setup's secret is known here), points from the C oracle or the Python reference; nothing below asks the
# library what the right answer is.  Each test prints how its wall time splits between building the expectation and the device calls.
def report(name, t_ref, t_dev):
    print("[timing] %s: reference %.2f s, device %.3f s" % (name, t_ref, t_dev))


def tower_to_flat(val):
    return pr.from_tower([(val[2 * k], val[2 * k + 1]) for k in range(6)])


def test_pairing_values_at_batch_size(kz):
    """200 pairs (three wavefronts and a tail of 8) with full-width scalars, random Jacobian Z on both sides (Z in F_p2 for G2), and infinity on
    either or both sides at the wavefront edges: every VALUE equals e(G1, G2)^(a b), and four of them the reference pairing computed directly"""
    rng = random.Random(31)
    t0 = time.perf_counter()
    n = 200
    a0, da, b0, db = (vc.rand_fr(rng) for _ in range(4))
    Ps, Qs = [pr.g1_mul(pr.G1_GEN, a0)], [pr.g2_mul(pr.G2_GEN, b0)]
    step1, step2 = pr.g1_mul(pr.G1_GEN, da), pr.g2_mul(pr.G2_GEN, db)
    for _ in range(n - 1):
        Ps.append(pr.g1_add(Ps[-1], step1)); Qs.append(pr.g2_add(Qs[-1], step2))
    inf1, inf2, both = {0, 64, 130, 197}, {63, 100, 199}, {31, 65, 128}
    g1 = np.stack([ko.g1_zero(1)[0] if i in inf1 | both else vi.g1_rescale(vi.g1_affine_image(*Ps[i]), rng.randrange(1, pr.P)) for i in range(n)])
    g2 = np.stack([vi.g2_kilic(None if i in inf2 | both else Qs[i], vi.rand_fp2(rng) if i % 5 else (1, 0)) for i in range(n)])
    e0 = pr.pairing(pr.G1_GEN, pr.G2_GEN, DEVICE_EXP)
    want = [pr.ONE12 if i in inf1 | inf2 | both else pr.f12pow(e0, (a0 + i * da) * (b0 + i * db) % pr.R) for i in range(n)]
    direct = (1, 62, 66, 198)
    for i in direct:
        assert want[i] == pr.pairing(Ps[i], Qs[i], DEVICE_EXP), i           # the expectation does not rest on bilinearity alone
    t1 = time.perf_counter()
    fs = kz.FFTSettings(4)
    got = fs.pairing_test(g1, g2)
    t2 = time.perf_counter()
    bad = [i for i in range(n) if tower_to_flat(got[i]) != want[i]]
    assert not bad, bad
    fs.close()
    report("pairing values x200", t1 - t0 + time.perf_counter() - t2, t2 - t1)


def row_bit(i, salt):
    return (((i + salt) * 0x9E3779B1) >> 13) & 1


def test_pairings_verify_batch_across_chunks(kz):
    """n = 2 * 8192 + 5: the chunk loop runs three times, the last chunk short.  Row i pairs [k + 1] G1 with [m + 1] G2 against [m + 1] G1 with
    [k + 1] G2 (k = i % 17, m = (i // 17) % 17; 17 is coprime to the chunk size, so a row read from the wrong chunk or the wrong half of the
    staging buffers meets other points) and is spoiled or not by a hash bit of i; the rows at the chunk edges are set by hand"""
    rng = random.Random(32)
    t0 = time.perf_counter()
    n = 2 * 8192 + 5
    A = np.stack([g1_mul_int(a) for a in range(1, 18)])
    Qref = [pr.g2_mul(pr.G2_GEN, a) for a in range(1, 18)]
    Q = np.stack([np.stack([vi.g2_kilic(q), vi.g2_kilic(q, vi.rand_fp2(rng))]) for q in Qref])        # [k][0]: Z = 1, [k][1]: Z in F_p2
    idx = np.arange(n)
    k, m = idx % 17, (idx // 17) % 17
    truth = np.array([row_bit(i, 0) for i in range(n)], dtype=bool)
    for i, w in ((8190, False), (8191, True), (8192, False), (8193, True), (16382, True), (16383, False), (16384, True), (16388, False)):
        truth[i] = w
    jz_a = np.array([row_bit(i, 1) for i in range(n)])
    jz_b = np.array([row_bit(i, 2) for i in range(n)])
    a1, a2, b1 = A[k], Q[m, jz_a], A[m]
    b2 = Q[np.where(truth, k, (k + 1) % 17), jz_b]
    assert 0.4 < truth.mean() < 0.6 and 0.4 < jz_a.mean() < 0.6
    t1 = time.perf_counter()
    fs = kz.FFTSettings(4)
    got = fs.pairings_verify_batch(a1, a2, b1, b2)
    wrong = np.nonzero(got != truth)[0]
    assert wrong.size == 0, wrong[:20]
    for small in (1, 63, 64, 65):
        lo = 8192 - small                                                     # a window of the same rows that starts elsewhere
        assert np.array_equal(fs.pairings_verify_batch(a1[:small], a2[:small], b1[:small], b2[:small]), truth[:small]), small
        assert np.array_equal(fs.pairings_verify_batch(a1[lo:8192], a2[lo:8192], b1[lo:8192], b2[lo:8192]), truth[lo:8192]), small
    t2 = time.perf_counter()
    fs.close()
    report("pairings_verify_batch x16389", t1 - t0, t2 - t1)


def padded_single_rows(s, total):
    rows = vc.single_rows(s, random.Random(1))
    seed = 100
    while len(rows) < total:
        extra = [r for r in vc.single_rows(s, random.Random(seed)) if r[0].startswith("ordinary/")]
        rows += [("pad%d/" % seed + r[0],) + r[1:] for r in extra][:total - len(rows)]
        seed += 1
    return rows


@pytest.fixture(scope="module")
def ks16_jacobian(kz, g2_powers):   # the same settings, SecretG2 as un-normalised Jacobian images (what setup.go:20 leaves)
    rng = random.Random(33)
    fs = kz.FFTSettings(5)
    ks = kz.KZGSettings(fs, ko.generate_testing_setup_g1(S_TEST, 33))
    ks.set_secret_g2(np.stack([vi.g2_kilic(Q, vi.rand_fp2(rng)) for Q in g2_powers]))
    yield ks
    ks.close()
    fs.close()


def test_crafted_single_rows_on_the_device(kz, ks16, ks16_jacobian):
    """every single row of verify_cases in one shuffled batch of 2 * 64 + 37 (exceptional and ordinary rows share wavefronts), then every
    exceptional row as a call of its own; on settings whose SecretG2 has Z = 1 and on settings that received Jacobian images"""
    t0 = time.perf_counter()
    rng = random.Random(34)
    rows = padded_single_rows(S_TEST, 2 * 64 + 37)
    rng.shuffle(rows)
    cs, pis, xs, ys = vi.single_images(rows, rng)
    want = [r[5] for r in rows]
    t1 = time.perf_counter()
    for ks in (ks16, ks16_jacobian):
        got = ks.check_proof_single_batch(cs, pis, xs, ys)
        bad = [(r[0], bool(g), r[5]) for r, g in zip(rows, got) if bool(g) != r[5]]
        assert not bad, bad
    lone = [i for i, r in enumerate(rows) if not r[0].startswith(("ordinary/", "pad"))]
    assert len(lone) > 80
    bad = []
    for i in lone:
        ks = ks16_jacobian if i % 2 else ks16
        got = ks.check_proof_single_batch(cs[i:i + 1], pis[i:i + 1], xs[i:i + 1], ys[i:i + 1])
        if [bool(g) for g in got] != [want[i]]:
            bad.append((rows[i][0], list(got), want[i]))
    assert not bad, bad
    report("crafted single rows", t1 - t0, time.perf_counter() - t1)


def test_crafted_multi_rows_on_the_device(kz, ks16, ks16_jacobian):
    """every multi row of verify_cases, one call per length: powers of two, the lengths 3, 5, 12 that pin x^np against SecretG2[n], x = 0,
    x = 1, x = s w"""
    t0 = time.perf_counter()
    rng = random.Random(35)
    rows = vc.multi_rows(S_TEST, random.Random(2))
    calls = []
    for n in vc.MULTI_NS:
        sub = [r for r in rows if r[5] == n]
        rng.shuffle(sub)
        cs = np.stack([vi.g1_scalar(r[1], rng.randrange(2, pr.P) if i % 2 else None) for i, r in enumerate(sub)])
        pis = np.stack([vi.g1_scalar(r[2], None if i % 3 else rng.randrange(2, pr.P)) for i, r in enumerate(sub)])
        calls.append((n, sub, cs, pis, ko.fr_from_ints([r[3] for r in sub]), np.stack([ko.fr_from_ints(r[4]) for r in sub])))
    assert sum(len(c[1]) for c in calls) == len(rows)
    t1 = time.perf_counter()
    bad = []
    for ks in (ks16, ks16_jacobian):
        for n, sub, cs, pis, xs, yss in calls:
            got = ks.check_proof_multi_batch(cs, pis, xs, yss)
            bad += [(r[0], bool(g), r[6]) for r, g in zip(sub, got) if bool(g) != r[6]]
    assert not bad, bad
    report("crafted multi rows", t1 - t0, time.perf_counter() - t1)


def fixture_g2_points():
    fx = json.load(open(os.path.join(GOLDEN, "trusted_setup_g2.json")))
    enc, pts, Q = [], [], pr.G2_GEN
    for h in fx["setup_G2"]:
        b = bytes.fromhex(h)
        assert b == pr.g2_compress(Q)                       # the fixture holds [1337^i] G2
        enc.append(b); pts.append(Q)
        Q = pr.g2_mul(Q, 1337)
    return enc, pts


def test_g2_from_compressed_in_a_multi_wavefront_batch(kz):
    """130 encodings (two wavefronts and a tail of 2) with the infinity encoding in the middle: every image is the reference point's; then one
    bad encoding at row 0, 64 and 129 in turn fails the whole call"""
    t0 = time.perf_counter()
    enc, pts = fixture_g2_points()
    enc, pts = enc + enc[::-1], pts + pts[::-1]
    enc[70], pts[70] = bytes([0xc0]) + bytes(95), None
    assert len(enc) == 130
    outside = None
    for x0 in range(1, 200):                                # on the curve, outside G2
        x = (x0, 0)
        y = pr.f2sqrt(pr.f2add(pr.f2mul(pr.f2sqr(x), x), pr.B2))
        if y is not None and pr.g2_mul((x, y), pr.R) is not None:
            outside = pr.g2_compress((x, y))
            break
    xp = bytearray(pr.P.to_bytes(48, "big") + bytes(48)); xp[0] |= 0x80              # x1 = p
    bad_kinds = {0: bytes([0x40]) + bytes(95), 64: bytes(xp), 129: outside}
    t1 = time.perf_counter()
    fs = kz.FFTSettings(4)
    got = fs.g2_from_compressed(np.frombuffer(b"".join(enc), dtype=np.uint8))
    for i in range(130):
        assert np.array_equal(got[i], vi.g2_kilic(pts[i])), i
    assert np.array_equal(got[70], vi.g2_kilic(None))       # Kilic's Zero(): (0, 1, 0)
    for row, b in bad_kinds.items():
        spoiled = list(enc); spoiled[row] = b
        with pytest.raises(kz.KzgError) as e:
            fs.g2_from_compressed(np.frombuffer(b"".join(spoiled), dtype=np.uint8))
        assert e.value.status == kz.ERR_BAD_POINT, row
    fs.close()
    report("g2_from_compressed x130", t1 - t0, time.perf_counter() - t1)


@pytest.fixture(scope="module")
def eth_fixture(kz):
    enc, pts = fixture_g2_points()
    fs = kz.FFTSettings(12)
    lag = ko.g1_decompress(np.frombuffer(open(os.path.join(GOLDEN, "trusted_setup_g1_lagrange.bin"), "rb").read(), dtype=np.uint8))
    eth = kz.EthSettings(fs, lag)
    yield eth, pts
    eth.close(); fs.close()


def test_eth_crafted_and_byte_rows(kz, eth_fixture):
    """the crafted rows compressed by the oracle and the byte-level rows on the fixture setup (s = 1337): 1 / 0 from the derived truth value,
    2 / 3 in the reference's order of checks (z, y, commitment, proof); kzgSetupG2 as Z = 1 images, then as Jacobian images"""
    t0 = time.perf_counter()
    eth, pts = eth_fixture
    rng = random.Random(4)
    rows = vi.eth_rows(1337, rng)
    want = [r[5] for r in rows]
    assert set(want) == {0, 1, 2, 3}
    c48, zs, ys, pi48 = vi.eth_arrays(rows)
    t1 = time.perf_counter()
    for jac in (False, True):
        eth.set_setup_g2(np.stack([vi.g2_kilic(Q, vi.rand_fp2(rng) if jac else (1, 0)) for Q in pts]))
        got = eth.verify_kzg_proof_batch(c48, zs, ys, pi48)
        bad = [(r[0], int(g), r[5]) for r, g in zip(rows, got) if int(g) != r[5]]
        assert not bad, bad
    byte_rows = [i for i, r in enumerate(rows) if r[0].startswith("bytes/")]
    for i in byte_rows:                                      # each byte-level row alone
        got = eth.verify_kzg_proof_batch(c48[i:i + 1], zs[i:i + 1], ys[i:i + 1], pi48[i:i + 1])
        assert list(got) == [want[i]], rows[i][0]
    report("eth rows", t1 - t0, time.perf_counter() - t1)


def test_g1_image_outside_the_subgroup_stays_in_its_row(kz, ks16):
    """The order-3 point (0, 2) as pi, then as C, in one row of an ordinary batch (tests/test_pairing_host.py runs the same rows through the
    host build under sanitizers first): the call succeeds and every other row's result is unchanged.  The row's own result is unspecified
    (include/kzg_hip.h) and printed; on the host build it is False both times."""
    rng = random.Random(5)
    rows = [r for r in padded_single_rows(S_TEST, 2 * 64 + 37) if r[0].startswith(("ordinary/", "pad"))][:70]
    cs, pis, xs, ys = vi.single_images(rows, rng)
    want = [r[5] for r in rows]
    evil = vi.g1_affine_image(*vi.ORDER3)
    for what, k in (("pi", 2), ("C", 66)):
        c2, p2 = cs.copy(), pis.copy()
        (p2 if what == "pi" else c2)[k] = evil
        got = [bool(g) for g in ks16.check_proof_single_batch(c2, p2, xs, ys)]      # raises unless the status is KZG_HIP_OK
        assert got[:k] + got[k + 1:] == want[:k] + want[k + 1:], what
        print("order-3 point as %s: the row returns %s" % (what, got[k]))
