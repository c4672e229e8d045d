"""The G2 half of a setup on the device (k_g2.hip, capi_verify.hip, capi_eth.hip): the fixed-base walk over bls.GenG2 against the reference's own
setup_G2 entries (tests/golden/trusted_setup_g2.json) and the Python reference tests/pairing_ref.py, the image form, compression, the JSON loader,
proving and verifying on a setup made without any CPU group arithmetic, concurrent first use of a handle, and the C++ mirror."""
import json
import os
import random
import subprocess
import threading

import numpy as np
import pytest

import g2_setup_cases as gc
import pairing_ref as pr
import verify_images as vi
from oracle import koracle as ko
from test_gpu_verify import POLY, S_TEST, eval_poly

pytestmark = pytest.mark.gpu

HERE = os.path.dirname(os.path.abspath(__file__))
ROOT = os.path.dirname(HERE)
GOLDEN = os.path.join(HERE, "golden")
R = pr.R
N_BIG = 257          # the kernels run 64-lane workgroups: five of them, the last with one lane


@pytest.fixture(scope="module")
def kz():
    import gokzg_amd
    assert gokzg_amd.device_count() >= 1, "no gfx950 device: the HIP path is the only path"
    return gokzg_amd


@pytest.fixture(scope="module")
def fs(kz):
    f = kz.FFTSettings(4)
    yield f
    f.close()


def fixture_bytes():
    return np.frombuffer(b"".join(bytes.fromhex(h) for h in gc.fixture_hex()), dtype=np.uint8).reshape(65, 96)


def check_image_form(imgs):
    """every output has Z = the Montgomery one, or is Kilic's Zero() (0, 1, 0)"""
    one = np.array([vi.u64s(vi.R384), vi.u64s(0)], dtype=np.uint64)
    zero = vi.g2_kilic(None)
    for i, img in enumerate(imgs):
        assert np.array_equal(img[2], one) or np.array_equal(img, zero), i


def test_known_answer_setup_g2(kz, fs):
    """the reference's data: [1337^i] G2 for i < 65, byte for byte"""
    s2 = fs.generate_testing_setup_g2(gc.fr_mont([gc.S_ETH]), 65)
    assert s2.shape == (65, 3, 2, 6)
    assert np.array_equal(fs.to_compressed_g2(s2), fixture_bytes())
    assert fs.g2_marshal_text(s2) == list(gc.fixture_hex())
    check_image_form(s2)
    assert np.array_equal(fs.g2_from_compressed(fs.to_compressed_g2(s2)), s2)            # limb for limb
    assert np.array_equal(fs.g2_unmarshal_text(gc.fixture_hex()), s2)
    assert fs.g2_table_builds() == 1


@pytest.mark.parametrize("secret", [S_TEST, 0, 1, R - 1], ids=["s_test", "zero", "one", "r-1"])
def test_setup_shapes_and_secrets(kz, fs, secret):
    want = gc.powers_points(secret, 65)
    sec = gc.fr_mont([secret])
    for n in (0, 1, 2, 65):
        got = fs.generate_testing_setup_g2(sec, n)
        assert got.shape == (n, 3, 2, 6)
        check_image_form(got)
        if n:
            assert np.array_equal(got, np.stack([vi.g2_kilic(Q) for Q in want[:n]]))
    big = fs.generate_testing_setup_g2(sec, N_BIG)
    check_image_form(big)
    assert np.array_equal(big[:65], np.stack([vi.g2_kilic(Q) for Q in want]))
    for i in (0, 1, 63, 64, N_BIG - 2, N_BIG - 1):
        assert np.array_equal(big[i], vi.g2_kilic(pr.g2_mul(pr.G2_GEN, pow(secret, i, R)))), i
    assert np.array_equal(big, fs.mul_gen_g2_vec(gc.fr_mont([pow(secret, i, R) for i in range(N_BIG)])))
    assert np.array_equal(fs.g2_from_compressed(fs.to_compressed_g2(big)), big)


def test_mul_gen_on_edge_scalars(kz, fs):
    """the device run of the host walk: 2^k, 2^k - 1, r - 2^k, 0, 1, r - 1 and random scalars"""
    cases = gc.edge_cases()
    got = fs.mul_gen_g2_vec(gc.fr_mont([k for _, k, _ in cases]))
    check_image_form(got)
    enc = fs.to_compressed_g2(got)
    want = gc.compressed([q for _, _, q in cases])
    bad = [name for (name, _, _), a, b in zip(cases, enc, want) if not np.array_equal(a, b)]
    assert not bad, bad
    assert np.array_equal(got[0], vi.g2_kilic(None))                                     # [0] G2: Kilic's Zero()
    assert len(fs.mul_gen_g2_vec(np.zeros((0, 4), dtype=np.uint64))) == 0


def test_compression_of_jacobian_images(kz, fs):
    """the fixture points with a random Jacobian Z, infinity placed among valid rows, n crossing workgroups"""
    rng = random.Random(41)
    pts = list(gc.fixture_points())
    rows = [pts[i % 65] for i in range(N_BIG)]
    for i in (0, 63, 64, 100, N_BIG - 1):
        rows[i] = None
    imgs = np.stack([vi.g2_kilic(Q, vi.rand_fp2(rng)) if Q is not None else vi.g2_kilic(None) for Q in rows])
    junk = vi.g2_kilic(pts[5], vi.rand_fp2(rng)); junk[2] = 0                            # Z = 0 whatever X and Y hold
    imgs[100] = junk
    assert np.array_equal(fs.to_compressed_g2(imgs), gc.compressed(rows))
    assert fs.to_compressed_g2(np.zeros((0, 3, 2, 6), dtype=np.uint64)).shape == (0, 96)


def outside_subgroup_hex():
    """a point of the twist outside G2 (cofactor not cleared), compressed: the first small x that decompresses onto the curve"""
    for x0 in range(1, 200):
        x = (x0, 0)
        y = pr.f2sqrt(pr.f2add(pr.f2mul(pr.f2sqr(x), x), pr.B2))
        if y is not None and pr.g2_mul((x, y), R) is not None:
            return pr.g2_compress((x, y)).hex()
    raise AssertionError("no such point")


def test_trusted_setup_g2_from_json(kz, fs):
    hexes = list(gc.fixture_hex())
    mono = open(os.path.join(GOLDEN, "trusted_setup_g1.bin"), "rb").read()
    g1 = [mono[48 * i:48 * i + 48].hex() for i in range(8)]
    doc = json.dumps({"setup_G1": g1, "setup_G2": hexes, "setup_G1_lagrange": g1[:4], "roots_of_unity": [1, 2, 3]}, indent=2)
    want = fs.g2_from_compressed(fixture_bytes())
    assert np.array_equal(fs.trusted_setup_g2_from_json(doc), want)
    # the two steps of the protocol by hand: the count alone, then the array; a capacity that does not suffice
    import ctypes as C
    L, raw = kz.lib(), doc.encode()
    n = C.c_uint64(7)
    assert L.kzg_hip_trusted_setup_g2_from_json(fs.h, raw, len(raw), None, 0, C.byref(n)) == kz.OK and n.value == 65
    out = kz.g2_empty(65)
    n = C.c_uint64(0)
    assert L.kzg_hip_trusted_setup_g2_from_json(fs.h, raw, len(raw), out.ctypes.data_as(C.c_void_p), 65, C.byref(n)) == kz.OK and n.value == 65
    assert np.array_equal(out, want)
    assert L.kzg_hip_trusted_setup_g2_from_json(fs.h, raw, len(raw), out.ctypes.data_as(C.c_void_p), 64, C.byref(n)) == kz.ERR_LEN_MISMATCH
    # the G1 loader on the same document returns what it returned before
    got_mono, got_lag = fs.trusted_setup_from_json(doc)
    assert np.array_equal(got_mono, fs.from_compressed_g1(np.frombuffer(mono[:48 * 8], dtype=np.uint8))) and np.array_equal(got_lag, got_mono[:4])
    bad = {"non-hex": ["zz" + hexes[1][2:]], "95 bytes": [hexes[1][:-2]], "outside the subgroup": [outside_subgroup_hex()]}
    for what, entry in bad.items():
        with pytest.raises(kz.KzgPanic) as e:
            fs.trusted_setup_g2_from_json(json.dumps({"setup_G1": g1, "setup_G2": hexes[:3] + entry + hexes[3:5]}))
        assert e.value.status == kz.ERR_BAD_POINT, what
    assert fs.trusted_setup_g2_from_json(json.dumps({"setup_G1": g1, "setup_G1_lagrange": g1})).shape == (0, 3, 2, 6)
    with pytest.raises(kz.KzgPanic) as e:
        fs.g2_unmarshal_text(["zz" + hexes[1][2:]])
    assert e.value.status == kz.ERR_BAD_POINT


def test_prove_and_verify_on_a_device_made_setup(kz):
    """TestKZGSettings_CheckProofSingle (kzg_single_proofs_test.go:36-64) and the multi-proof check (kzg_multi_proofs_test.go) with no
    Python or CPU group arithmetic: both halves of the setup from the device"""
    fs = kz.FFTSettings(4)
    sec = gc.fr_mont([S_TEST])
    s1, s2 = kz.generate_testing_setup(fs, sec, 17)
    assert s1.shape == (17, 3, 6) and s2.shape == (17, 3, 2, 6)
    ks = kz.KZGSettings(fs, s1, s2)
    poly = ko.fr_from_ints(POLY)
    c = ks.commit_to_poly(poly)
    proof = ks.compute_proof_single(poly, 17)
    y = eval_poly(POLY, 17)
    ok = ks.check_proof_single_batch(np.stack([c, c]), np.stack([proof, proof]), ko.fr_from_ints([17, 17]), ko.fr_from_ints([y, y + 1]))
    assert list(ok) == [True, False]
    with pytest.raises(kz.KzgPanic) as e:                                                # kzg.go:22-27
        kz.KZGSettings(fs, s1, s2[:16])
    assert e.value.status == kz.ERR_LEN_MISMATCH
    ks2 = kz.KZGSettings(fs, s1)                                                         # two arguments: as before, no G2 points
    with pytest.raises(kz.KzgError) as e:
        ks2.check_proof_single_batch(c[None], proof[None], ko.fr_from_ints([17]), ko.fr_from_ints([y]))
    assert e.value.status == kz.ERR_BAD_ARG
    ks2.close()
    # multi proofs: a setup of 33 points, a coset of 8 values at x = 5431
    fs5 = kz.FFTSettings(5)
    t1, t2 = kz.generate_testing_setup(fs5, sec, 33)
    ksm = kz.KZGSettings(fs5, t1, t2)
    roots = ko.fr_to_ints(fs5.expanded_roots_of_unity())[:32:4]
    x = 5431
    ys = [eval_poly(POLY, x * w % R) for w in roots]
    pm = ksm.compute_proof_multi(poly, x, 8)
    cm = ksm.commit_to_poly(poly)
    ys_bad = list(ys); ys_bad[3] = (ys_bad[3] + 1) % R
    ok = ksm.check_proof_multi_batch(np.stack([cm, cm]), np.stack([pm, pm]), ko.fr_from_ints([x, x]), np.stack([ko.fr_from_ints(ys), ko.fr_from_ints(ys_bad)]))
    assert list(ok) == [True, False]
    for h in (ksm, ks):
        h.close()
    fs5.close(); fs.close()


def test_eth_verify_on_a_device_made_setup_g2(kz):
    """eth.VerifyKZGProof with kzgSetupG2 = generate_testing_setup_g2(1337, 65) instead of the decompressed fixture"""
    fs = kz.FFTSettings(12)
    lag = ko.g1_decompress(np.frombuffer(open(os.path.join(GOLDEN, "trusted_setup_g1_lagrange.bin"), "rb").read(), dtype=np.uint8))
    eth = kz.EthSettings(fs, lag)
    eth.set_setup_g2(fs.generate_testing_setup_g2(gc.fr_mont([gc.S_ETH]), 65))
    blob_i = ko.fr_to_ints(ko.synthetic_blob(1))
    blob = np.frombuffer(b"".join(v.to_bytes(32, "little") for v in blob_i), dtype=np.uint8).reshape(1, 4096, 32)
    commits, ok = eth.blob_to_kzg_commitment_batch(blob)
    assert ok.all()
    z = 0x1234567890abcdef
    proofs, ys, ok = eth.compute_kzg_proof_batch(ko.fr_from_ints(blob_i)[None], ko.fr_from_ints([z]))
    assert ok.all()
    le = lambda v: np.frombuffer(v.to_bytes(32, "little"), dtype=np.uint8)               # noqa: E731
    y = ko.fr_to_ints(ys)[0]
    got = eth.verify_kzg_proof_batch(np.concatenate([commits, commits]), np.stack([le(z), le(z)]), np.stack([le(y), le((y + 1) % R)]),
                                     np.concatenate([proofs, proofs]))
    assert list(got) == [1, 0]
    eth.close(); fs.close()


def test_concurrent_first_use_builds_one_table(kz):
    """eight threads make the first multiplication on a fresh handle at once: eight correct results, one table"""
    fs = kz.FFTSettings(4)
    assert fs.g2_table_builds() == 0
    sec, want = gc.fr_mont([gc.S_ETH]), fixture_bytes()
    start, res = threading.Barrier(8), [None] * 8

    def work(i):
        start.wait()
        res[i] = fs.to_compressed_g2(fs.generate_testing_setup_g2(sec, 65))

    ts = [threading.Thread(target=work, args=(i,)) for i in range(8)]
    for t in ts:
        t.start()
    for t in ts:
        t.join()
    for i in range(8):
        assert res[i] is not None and np.array_equal(res[i], want), i
    assert fs.g2_table_builds() == 1
    fs.close()


def test_cpp_mirror_generates_the_setup(kz, tmp_path):
    """tests/host/g2_setup_consumer.cpp against include/kzg_hip.hpp and the built library: GenerateTestingSetup("1337", 65), ToCompressedG2"""
    bdir = os.path.join(HERE, "host", "_build")
    os.makedirs(bdir, exist_ok=True)
    exe = os.path.join(bdir, "g2_setup_consumer")
    libdir = os.path.dirname(kz.LIB_PATH)
    subprocess.check_call(["g++", "-std=c++17", "-O1", "-Wall", "-Wextra", "-Werror", "-I", os.path.join(ROOT, "include"),
                           os.path.join(HERE, "host", "g2_setup_consumer.cpp"), "-L", libdir, "-lkzg_hip", "-Wl,-rpath," + libdir, "-o", exe])
    want = tmp_path / "setup_g2.txt"
    want.write_text("\n".join(gc.fixture_hex()) + "\n")
    res = subprocess.run([exe, str(want)], capture_output=True, text=True, timeout=120)
    assert res.returncode == 0 and "PASSED: 0 failure(s)" in res.stdout, res.stdout + res.stderr
