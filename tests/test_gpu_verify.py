"""Verification on the device (k_pairing.hip, capi_verify.hip): pairing values against the Python reference, batched PairingsVerify, the
reference's pairing-based proof tests restated (kzg_single_proofs_test.go, fk20_single_test.go, kzg_multi_proofs_test.go, fk20_multi_test.go),
a 4096-proof batch with tampered rows, and eth.VerifyKZGProof end to end on the trusted setup's G2 points (tests/golden/trusted_setup_g2.json)."""
import json
import os

import numpy as np
import pytest

import pairing_ref as pr
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
