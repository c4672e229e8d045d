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

HERE = os.path.dirname(os.path.abspath(__file__))
ROOT = os.path.dirname(HERE)
SRC = os.path.join(HERE, "host", "pairing_emul.cpp")
OUT = os.path.join(HERE, "host", "_build", "libpairing_emul.so")
FIXTURE = os.path.join(HERE, "golden", "trusted_setup_g2.json")
# the value the device computes: final_exponentiation raises to 3 (p^12 - 1) / r (pairing.hpp)
DEVICE_EXP = 3 * pr.FINAL_EXP


@pytest.fixture(scope="module")
def pe():
    os.makedirs(os.path.dirname(OUT), exist_ok=True)
    inc = os.path.join(ROOT, "go-kzg_amd", "csrc")
    deps = [SRC] + [os.path.join(inc, h) for h in ("field.hpp", "g1.hpp", "tower.hpp", "g2.hpp", "pairing.hpp")]
    if not os.path.exists(OUT) or any(os.path.getmtime(d) > os.path.getmtime(OUT) for d in deps):
        subprocess.check_call(["g++", "-O1", "-std=c++17", "-shared", "-fPIC", "-I", inc, "-o", OUT, SRC])
    lib = C.CDLL(OUT)
    lib.pe_pairing.argtypes = [C.c_uint64, C.c_void_p, C.c_void_p, C.c_void_p]
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
