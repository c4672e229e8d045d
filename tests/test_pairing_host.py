"""The pairing headers (tower.hpp / g2.hpp / pairing.hpp), compiled for the host, against the plain-Python reference tests/pairing_ref.py.
CPU only."""
import ctypes as C
import json
import os
import random
import subprocess

import numpy as np
import pytest

import pairing_ref as pr
import verify_cases as vc
import verify_images as vi
from oracle import koracle as ko

HERE = os.path.dirname(os.path.abspath(__file__))
ROOT = os.path.dirname(HERE)
SRC = os.path.join(HERE, "host", "pairing_emul.cpp")
OUT = os.path.join(HERE, "host", "_build", "libpairing_emul.so")
OUT_SAN = os.path.join(HERE, "host", "_build", "pairing_emul_san")
HEADERS = ("field.hpp", "g1.hpp", "tower.hpp", "g2.hpp", "pairing.hpp", "verify_inputs.hpp")
S_TEST = 1927409816240961209460912649124
S_ETH = 1337
FIXTURE = os.path.join(HERE, "golden", "trusted_setup_g2.json")
# the value the device computes: final_exponentiation raises to 3 (p^12 - 1) / r (pairing.hpp)
DEVICE_EXP = 3 * pr.FINAL_EXP


@pytest.fixture(scope="module")
def pe():
    os.makedirs(os.path.dirname(OUT), exist_ok=True)
    inc = os.path.join(ROOT, "go-kzg_amd", "csrc")
    deps = [SRC] + [os.path.join(inc, h) for h in HEADERS]
    if not os.path.exists(OUT) or any(os.path.getmtime(d) > os.path.getmtime(OUT) for d in deps):
        subprocess.check_call(["g++", "-O1", "-std=c++17", "-shared", "-fPIC", "-I", inc, "-o", OUT, SRC])
    lib = C.CDLL(OUT)
    vp = C.c_void_p
    lib.pe_pairing.argtypes = [C.c_uint64, vp, vp, vp]
    lib.pe_sizeof_prepared.restype = C.c_uint64
    lib.pe_g2_prepare_kilic.argtypes = [vp, vp]
    lib.pe_g2_kilic_to_affine.argtypes = [vp, vp]
    lib.pe_kzg_check_batch.argtypes = [C.c_uint64, vp, vp, vp, vp, vp, vp, vp, vp]
    lib.pe_eth_check_batch.argtypes = [C.c_uint64, vp, vp, vp, vp, vp, vp, vp]
    return lib


def limbs(v):
    return [(v >> (32 * i)) & 0xffffffff for i in range(12)]


def ints(a):
    return [sum(int(a[12 * k + i]) << (32 * i) for i in range(12)) for k in range(len(a) // 12)]


def arr(vals):
    return np.array([l for v in vals for l in limbs(v)], dtype=np.uint32)


def p(a):
    return a.ctypes.data_as(C.c_void_p)


def tower_flat(c):   # 6 F_p2 -> 12 ints in memory order
    return [x for pair in c for x in pair]


def flat_tower(v):
    return [(v[2 * k], v[2 * k + 1]) for k in range(6)]


def rand_fp12(rng):
    return [rng.randrange(pr.P) for _ in range(12)]


def op(pe, code, a, b=None):
    out = np.zeros(144, dtype=np.uint32)
    A, B = arr(a), arr(b if b is not None else [0] * 12)
    pe.pe_fp12_op(code, p(A), p(B), p(out))
    return ints(out)


def flat(v):   # device memory order -> flat polynomial form of the reference
    return pr.from_tower(flat_tower(v))


def test_tower_ops(pe):
    rng = random.Random(7)
    cases = [rand_fp12(rng) for _ in range(4)] + [[1] + [0] * 11, [pr.P - 1] * 12, [0] * 11 + [1], [0, 5] + [0] * 10]
    for a in cases:
        b = rand_fp12(rng)
        fa, fb = flat(a), flat(b)
        assert flat(op(pe, 0, a, b)) == pr.f12mul(fa, fb)
        assert flat(op(pe, 1, a)) == pr.f12mul(fa, fa)
        assert flat(op(pe, 2, a)) == pr.f12inv(fa)
        assert flat(op(pe, 3, a)) == pr.f12pow(fa, pr.P)
        assert flat(op(pe, 4, a)) == pr.f12pow(fa, pr.P ** 2)
        assert flat(op(pe, 5, a)) == pr.f12pow(fa, pr.P ** 3)
        assert flat(op(pe, 7, a)) == pr.f12pow(fa, pr.P ** 6)
        sparse = [b[0], b[1], b[2], b[3], 0, 0, 0, 0, b[4], b[5], 0, 0]   # c0 (position 0), c1 (v), c4 (v w)
        line = op(pe, 8, a, [b[0], b[1], b[2], b[3], b[4], b[5]] + [0] * 6)
        assert flat(line) == pr.f12mul(fa, flat(sparse))


def test_cyclotomic_squaring(pe):
    rng = random.Random(8)
    for _ in range(3):
        fa = flat(rand_fp12(rng))
        g = pr.f12pow(fa, (pr.P ** 6 - 1) * (pr.P ** 2 + 1))    # in the cyclotomic subgroup
        gt = tower_flat(pr.to_tower(g))
        assert flat(op(pe, 6, gt)) == pr.f12mul(g, g)


def decompress(pe, b):
    out = np.zeros(48, dtype=np.uint32)
    ok = pe.pe_g2_decompress(C.c_char_p(bytes(b)), p(out))
    v = ints(out)
    return ((v[0], v[1]), (v[2], v[3])) if ok else False


def test_g2_fixture_decompression(pe):
    fx = json.load(open(FIXTURE))
    Q = pr.G2_GEN
    assert len(fx["setup_G2"]) == 65
    for i, h in enumerate(fx["setup_G2"]):
        b = bytes.fromhex(h)
        assert b == pr.g2_compress(Q), i                 # the fixture holds [1337^i] G2
        assert decompress(pe, b) == Q, i                 # the headers' decompression, subgroup check included
        Q = pr.g2_mul(Q, 1337)


def test_g2_rejects_bad_encodings(pe):
    good = bytearray(pr.g2_compress(pr.g2_mul(pr.G2_GEN, 5)))
    assert decompress(pe, good) == pr.g2_mul(pr.G2_GEN, 5)
    assert decompress(pe, bytes([0xc0]) + bytes(95)) == ((0, 0), (0, 0))   # infinity
    bad = [bytes([0x40]) + bytes(95),                       # infinity without the compression flag
           bytes([0xc0]) + bytes(94) + b"\x01",             # infinity with a non-zero body
           bytes([0xe0]) + bytes(95),                       # infinity with the sort flag
           bytes(good[:1]) .replace(bytes(good[:1]), bytes([good[0] & 0x7f])) + bytes(good[1:])]   # compression flag cleared
    xp = bytearray((pr.P).to_bytes(48, "big") + bytes(48)); xp[0] |= 0x80       # x1 = p
    bad.append(bytes(xp))
    x0p = bytearray(bytes(48) + (pr.P + 1).to_bytes(48, "big")); x0p[0] |= 0x80  # x0 = p + 1
    bad.append(bytes(x0p))
    # x with x^3 + b not a square (off the curve), and x on the curve but outside G2 (cofactor not cleared)
    off, outside = None, None
    for x0 in range(1, 200):
        x = (x0, 0)
        y = pr.f2sqrt(pr.f2add(pr.f2mul(pr.f2sqr(x), x), pr.B2))
        if y is None and off is None:
            off = x
        if y is not None and outside is None and pr.g2_mul((x, y), pr.R) is not None:
            outside = (x, y)
        if off and outside:
            break
    enc = bytearray(off[1].to_bytes(48, "big") + off[0].to_bytes(48, "big")); enc[0] |= 0x80
    bad.append(bytes(enc))
    bad.append(pr.g2_compress(outside))
    for b in bad:
        assert decompress(pe, b) is False, b.hex()


def g1_jac(Pt, z):   # Jacobian image (x z^2, y z^3, z) of an affine point; None -> (0, 1, 0)
    if Pt is None:
        return [0, 1, 0]
    return [Pt[0] * z * z % pr.P, Pt[1] * z * z * z % pr.P, z]


def g2_aff(Q):
    if Q is None:
        return [0, 0, 0, 0, 1]
    return [Q[0][0], Q[0][1], Q[1][0], Q[1][1], 0]


def device_pairing(pe, pairs, zs=None):
    g1 = arr([v for i, (Pt, _) in enumerate(pairs) for v in g1_jac(Pt, (zs or [1] * len(pairs))[i])])
    g2 = arr([v for _, Q in pairs for v in g2_aff(Q)])
    out = np.zeros(144, dtype=np.uint32)
    pe.pe_pairing(len(pairs), p(g1), p(g2), p(out))
    return flat(ints(out))


def test_pairing_values(pe):
    G1, G2 = pr.G1_GEN, pr.G2_GEN
    pairs = [(G1, G2), (pr.g1_mul(G1, 5), G2), (G1, pr.g2_mul(G2, 7)), (None, G2), (G1, None), (pr.g1_mul(G1, 3), pr.g2_mul(G2, 11))]
    zs = [1, 0x1234567, 3, 1, 9, 2 ** 200 + 5]     # Jacobian images with Z != 1: the F_p factor Z^3 must vanish
    for (Pt, Q), z in zip(pairs, zs):
        got = device_pairing(pe, [(Pt, Q)], [z])
        assert got == pr.pairing(Pt, Q, DEVICE_EXP) if Pt and Q else got == pr.ONE12
    # multi-pairing: the product of all six
    assert device_pairing(pe, pairs, zs) == pr.multi_pairing(pairs, DEVICE_EXP)


def test_bilinearity_and_order(pe):
    G1, G2 = pr.G1_GEN, pr.G2_GEN
    a, b = 0x1234567890abcdef, 0xfedcba987
    e = device_pairing(pe, [(G1, G2)])
    assert e != pr.ONE12                                              # non-degenerate
    assert device_pairing(pe, [(pr.g1_mul(G1, a), pr.g2_mul(G2, b))]) == pr.f12pow(e, a * b)
    assert pr.f12pow(e, pr.R) == pr.ONE12                             # order r
    # the check the kernels run: e(aP, Q) e(-P, aQ) == 1, and not for a + 1
    def chk(P0, Q0, P1, Q1):
        g1 = arr(g1_jac(P0, 1) + g1_jac(P1, 1))
        g2 = arr(g2_aff(Q0) + g2_aff(Q1))
        return pe.pe_pairing_check2(p(g1), p(g2))
    nP = (G1[0], (-G1[1]) % pr.P)
    assert chk(pr.g1_mul(G1, a), G2, nP, pr.g2_mul(G2, a)) == 1
    assert chk(pr.g1_mul(G1, a), G2, nP, pr.g2_mul(G2, a + 1)) == 0
    assert chk(None, G2, G1, None) == 1


# ---------------- the check-input lanes (verify_inputs.hpp) on crafted rows, and G2 images with Z != 1 ----------------
def prepared(pe, kilic):   # what k_g2_prepare leaves for one Kilic image (None: bls.GenG2)
    buf = np.zeros(pe.pe_sizeof_prepared(), dtype=np.uint8)
    img = None if kilic is None else np.ascontiguousarray(kilic)
    pe.pe_g2_prepare_kilic(None if img is None else p(img), p(buf))
    return buf


def kzg_check(pe, gen, q1, cs, pis, bs, ys=None, es=None):
    n = len(cs)
    cs, pis, bs = (np.ascontiguousarray(a) for a in (cs, pis, bs))
    ys = None if ys is None else np.ascontiguousarray(ys)
    es = None if es is None else np.ascontiguousarray(es)
    ok = np.zeros(n, dtype=np.uint8)
    pe.pe_kzg_check_batch(n, p(cs), p(pis), None if ys is None else p(ys), None if es is None else p(es), p(bs), p(gen), p(q1), p(ok))
    return [bool(v) for v in ok]


@pytest.fixture(scope="module")
def g2_s_test():
    return pr.g2_mul(pr.G2_GEN, S_TEST % pr.R)


def test_g2_jacobian_images(pe):
    """(x Z^2, y Z^3, Z) through g2_from_kilic + g2_to_affine is the affine point, for Z in F_p, in u F_p, in general position and at p - 1;
    Z = 0 is infinity whatever X and Y hold"""
    rng = random.Random(21)
    Q = pr.g2_mul(pr.G2_GEN, 0x123456789abcdef)
    zs = [(1, 0), (rng.randrange(2, pr.P), 0), (0, rng.randrange(2, pr.P)), vi.rand_fp2(rng), vi.rand_fp2(rng), (pr.P - 1, pr.P - 1), (0, 1), (pr.P - 1, 0)]
    for pt in (Q, pr.G2_GEN):
        for z in zs:
            img = vi.g2_kilic(pt, z)
            if z != (1, 0):
                assert not np.array_equal(img, vi.g2_kilic(pt))
            out = np.zeros(48, dtype=np.uint32)
            assert pe.pe_g2_kilic_to_affine(p(img), p(out)) == 0
            v = ints(out)
            assert ((v[0], v[1]), (v[2], v[3])) == pt, z
    out = np.ones(48, dtype=np.uint32)
    assert pe.pe_g2_kilic_to_affine(p(vi.g2_kilic(None)), p(out)) == 1 and not out.any()
    junk = vi.g2_kilic(Q, vi.rand_fp2(rng)); junk[2] = 0           # X, Y arbitrary, Z = 0
    assert pe.pe_g2_kilic_to_affine(p(junk), p(out)) == 1 and not out.any()


def test_prepared_lines_do_not_depend_on_z(pe, g2_s_test):
    rng = random.Random(22)
    want = prepared(pe, vi.g2_kilic(g2_s_test))
    for z in ((rng.randrange(2, pr.P), 0), (0, rng.randrange(2, pr.P)), vi.rand_fp2(rng), (pr.P - 1, pr.P - 1)):
        assert np.array_equal(prepared(pe, vi.g2_kilic(g2_s_test, z)), want), z
    assert np.array_equal(prepared(pe, None), prepared(pe, vi.g2_kilic(pr.G2_GEN, vi.rand_fp2(rng))))
    assert not np.array_equal(prepared(pe, None), want)


def test_crafted_single_rows(pe, g2_s_test):
    """every row of verify_cases.single_rows through the lane of k_kzg_check_inputs and the two-pair check: ok == the derived truth value;
    [s] G2 arrives as a Jacobian image, C and pi alternate between Z = 1 and Z != 1"""
    rng = random.Random(1)
    rows = vc.single_rows(S_TEST, rng)
    gen, q1 = prepared(pe, None), prepared(pe, vi.g2_kilic(g2_s_test, vi.rand_fp2(rng)))
    cs, pis, xs, ys = vi.single_images(rows, rng)
    got = kzg_check(pe, gen, q1, cs, pis, xs, ys=ys)
    bad = [(r[0], g, r[5]) for r, g in zip(rows, got) if g != r[5]]
    assert not bad, bad


def test_crafted_multi_rows(pe):
    """every row of verify_cases.multi_rows with [I'(s)] G1 supplied as a point and b = x^np: the G1 side pairs with SecretG2[n], n = len(ys)"""
    rng = random.Random(2)
    s = S_TEST % pr.R
    rows = vc.multi_rows(s, rng)
    gen = prepared(pe, None)
    bad = []
    for n in vc.MULTI_NS:
        sub = [r for r in rows if r[5] == n]
        assert sub
        qn = prepared(pe, vi.g2_kilic(pr.g2_mul(pr.G2_GEN, pow(s, n, pr.R)), vi.rand_fp2(rng)))
        cs = np.stack([vi.g1_scalar(r[1], rng.randrange(2, pr.P) if i % 2 else None) for i, r in enumerate(sub)])
        pis = np.stack([vi.g1_scalar(r[2], None if i % 3 else rng.randrange(2, pr.P)) for i, r in enumerate(sub)])
        es = np.stack([vi.g1_scalar(vc.interp_at(r[4], r[3], s), rng.randrange(2, pr.P) if i % 4 == 1 else None) for i, r in enumerate(sub)])
        bs = ko.fr_from_ints([pow(r[3], vc.next_pow2(n), pr.R) for r in sub])
        got = kzg_check(pe, gen, qn, cs, pis, bs, es=es)
        bad += [(r[0], g, r[6]) for r, g in zip(sub, got) if g != r[6]]
    assert not bad, bad


def test_eth_rows(pe):
    """the crafted rows compressed, and the byte-level rows, through the lane of k_eth_check_inputs on the fixture setup's secret: 1 / 0 from
    the derived truth value, 2 / 3 in the reference's order of checks"""
    rng = random.Random(4)
    rows = vi.eth_rows(S_ETH, rng)
    fx = json.load(open(FIXTURE))
    g2s = pr.g2_decompress(bytes.fromhex(fx["setup_G2"][1]))
    assert g2s == pr.g2_mul(pr.G2_GEN, S_ETH)
    gen, q1 = prepared(pe, None), prepared(pe, vi.g2_kilic(g2s))
    c48, zs, ys, pi48 = vi.eth_arrays(rows)
    res = np.zeros(len(rows), dtype=np.uint8)
    pe.pe_eth_check_batch(len(rows), p(c48), p(zs), p(ys), p(pi48), p(gen), p(q1), p(res))
    bad = [(r[0], int(g), r[5]) for r, g in zip(rows, res) if g != r[5]]
    assert not bad, bad
    assert {r[5] for r in rows} == {0, 1, 2, 3}


@pytest.fixture(scope="module")
def pe_san():   # the same source as a program with the address and undefined-behaviour sanitizers
    inc = os.path.join(ROOT, "go-kzg_amd", "csrc")
    deps = [SRC] + [os.path.join(inc, h) for h in HEADERS]
    os.makedirs(os.path.dirname(OUT_SAN), exist_ok=True)
    if not os.path.exists(OUT_SAN) or any(os.path.getmtime(d) > os.path.getmtime(OUT_SAN) for d in deps):
        # -O0: a third of the build time of -O1 with the sanitizers on these always-inline bodies.  shift-base is off: the divsteps of inv<>()
        # (field.hpp) double a negative int32 with `<< 1`, which C++20 defines as every compiler has always computed it; shift counts stay checked
        subprocess.check_call(["g++", "-O0", "-g", "-std=c++17", "-DPE_MAIN", "-fsanitize=address,undefined", "-fno-sanitize=shift-base",
                               "-fno-sanitize-recover=all", "-static-libasan", "-static-libubsan", "-I", inc, "-o", OUT_SAN, SRC])
    return OUT_SAN


def test_g1_image_outside_the_subgroup_stays_in_its_row(pe, pe_san, g2_s_test, tmp_path):
    """check_proof_*_batch and pairings_verify_batch take G1 images unchecked, and the lane multiplies pi with the GLV schedule, which assumes
    membership in G1.  One row of an ordinary batch holds the order-3 point (0, 2) as pi, then as C: under the sanitizers the lane terminates,
    reads and writes nothing out of bounds, and every other row's result is unchanged.  What the row itself returns is unspecified
    (include/kzg_hip.h); it is printed, and the host library and the sanitizer build agree on it."""
    rng = random.Random(5)
    rows = [r for r in vc.single_rows(S_TEST, rng) if r[0].startswith("ordinary/")][:8]
    cs, pis, xs, ys = vi.single_images(rows, rng)
    q1_img = vi.g2_kilic(g2_s_test)
    gen, q1 = prepared(pe, None), prepared(pe, q1_img)
    want = [r[5] for r in rows]
    assert True in want and False in want
    evil = vi.g1_affine_image(*vi.ORDER3)
    for what, k in (("pi", 2), ("C", 5)):
        c2, p2 = cs.copy(), pis.copy()
        (p2 if what == "pi" else c2)[k] = evil
        path = tmp_path / ("batch_%s.bin" % what)
        with open(path, "wb") as f:
            f.write(np.uint64(len(rows)).tobytes())
            for a in (c2, p2, ys, xs, q1_img):
                f.write(np.ascontiguousarray(a).tobytes())
        env = dict(os.environ, ASAN_OPTIONS="detect_leaks=0:verify_asan_link_order=0", UBSAN_OPTIONS="print_stacktrace=1")
        run = subprocess.run([pe_san, str(path)], capture_output=True, text=True, timeout=300, env=env)
        assert run.returncode == 0 and not run.stderr.strip(), run.stderr[-2000:]
        got = [ch == "1" for ch in run.stdout.strip()]
        assert len(got) == len(rows)
        assert got[:k] + got[k + 1:] == want[:k] + want[k + 1:], (what, got, want)
        lib_got = kzg_check(pe, gen, q1, c2, p2, xs, ys=ys)
        assert lib_got == got
        print("order-3 point as %s: the row returns %s" % (what, got[k]))
