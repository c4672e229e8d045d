"""The setup half of g2.hpp (mixed addition, digit cutter, fixed-base table of bls.GenG2 and the walk over it, normalisation, compression),
compiled for the host, against the plain-Python reference tests/pairing_ref.py.  CPU only."""
import ctypes as C
import os
import random
import subprocess

import numpy as np
import pytest

import g2_setup_cases as gc
import pairing_ref as pr
import verify_images as vi

HERE = os.path.dirname(os.path.abspath(__file__))
ROOT = os.path.dirname(HERE)
SRC = os.path.join(HERE, "host", "g2_setup_emul.cpp")
OUT = os.path.join(HERE, "host", "_build", "libg2_setup_emul.so")
OUT_SAN = os.path.join(HERE, "host", "_build", "g2_setup_emul_san")
HEADERS = ("field.hpp", "g1.hpp", "tower.hpp", "g2.hpp")
INC = os.path.join(ROOT, "go-kzg_amd", "csrc")
P = pr.P


def _stale(out):
    deps = [SRC] + [os.path.join(INC, h) for h in HEADERS]
    return not os.path.exists(out) or any(os.path.getmtime(d) > os.path.getmtime(out) for d in deps)


@pytest.fixture(scope="module")
def ge():
    os.makedirs(os.path.dirname(OUT), exist_ok=True)
    if _stale(OUT):
        subprocess.check_call(["g++", "-O1", "-std=c++17", "-shared", "-fPIC", "-I", INC, "-o", OUT, SRC])
    lib = C.CDLL(OUT)
    vp = C.c_void_p
    lib.g2e_add_mixed.argtypes = [vp, vp, vp]
    lib.g2e_window_bits.restype = C.c_uint32
    lib.g2e_windows.restype = C.c_uint32
    lib.g2e_digits.argtypes = [vp, vp]
    lib.g2e_table_entry.argtypes = [C.c_uint32, C.c_uint32, vp]
    lib.g2e_mul_generator.argtypes = [C.c_uint64, vp, vp]
    lib.g2e_compress.argtypes = [C.c_uint64, vp, vp]
    lib.g2e_decompress.argtypes = [vp, vp]
    return lib


def p(a):
    return a.ctypes.data_as(C.c_void_p)


def limbs(v):
    return [(v >> (32 * i)) & 0xffffffff for i in range(12)]


def arr(vals):
    return np.array([l for v in vals for l in limbs(v)], dtype=np.uint32)


def ints(a):
    return [sum(int(a[12 * k + i]) << (32 * i) for i in range(12)) for k in range(len(a) // 12)]


def jac(Q, z):   # (x z^2, y z^3, z) as six integers; None: infinity with junk in X and Y
    if Q is None:
        return [7, 0, 1, 2, 0, 0]
    z2 = pr.f2sqr(z)
    x, y = pr.f2mul(Q[0], z2), pr.f2mul(Q[1], pr.f2mul(z2, z))
    return [x[0], x[1], y[0], y[1], z[0], z[1]]


def aff(Q):
    return [0, 0, 0, 0] if Q is None else [Q[0][0], Q[0][1], Q[1][0], Q[1][1]]


def add_mixed(ge, Pt, z, Q):
    out = np.ones(48, dtype=np.uint32)
    inf = ge.g2e_add_mixed(p(arr(jac(Pt, z))), p(arr(aff(Q))), p(out))
    v = ints(out)
    if inf:
        assert not out.any()
        return None
    return ((v[0], v[1]), (v[2], v[3]))


def test_mixed_addition(ge):
    rng = random.Random(31)
    G = pr.G2_GEN
    pts = [pr.g2_mul(G, rng.randrange(1, pr.R)) for _ in range(6)]
    for i in range(5):                                                     # general position, Z != 1
        assert add_mixed(ge, pts[i], vi.rand_fp2(rng), pts[i + 1]) == pr.g2_add(pts[i], pts[i + 1])
    A = pts[0]
    assert add_mixed(ge, A, (1, 0), pts[1]) == pr.g2_add(A, pts[1])        # Z == 1
    assert add_mixed(ge, None, (0, 0), A) == A                             # P infinity
    assert add_mixed(ge, A, vi.rand_fp2(rng), None) == A                   # Q the "no point" entry
    assert add_mixed(ge, None, (0, 0), None) is None                       # both
    assert add_mixed(ge, A, (1, 0), A) == pr.g2_add(A, A)                  # P == Q
    assert add_mixed(ge, A, vi.rand_fp2(rng), A) == pr.g2_add(A, A)        # P == Q, P with a random Z
    assert add_mixed(ge, A, (1, 0), pr.g2_neg(A)) is None                  # P == -Q
    assert add_mixed(ge, A, vi.rand_fp2(rng), pr.g2_neg(A)) is None


def digits_of(ge, ks):
    nw = ge.g2e_windows()
    img = gc.fr_mont(ks)
    out = []
    for i in range(len(ks)):
        d = np.zeros(nw, dtype=np.uint32)
        ge.g2e_digits(p(img[i:i + 1]), p(d))
        out.append([int(v) for v in d])
    return out


def test_digits_recombine(ge):
    c, nw = ge.g2e_window_bits(), ge.g2e_windows()
    assert c * nw >= 255
    ks = [0, 1, pr.R - 1] + [1 << k for k in range(255)] + [(1 << k) - 1 for k in range(255)]
    for k, d in zip(ks, digits_of(ge, ks)):
        assert all(0 <= v < (1 << c) for v in d)                           # unsigned digits: what the table's rows hold
        assert sum(v << (c * w) for w, v in enumerate(d)) == k, hex(k)


def test_table_entries(ge):
    """the first, the last and the top window's rows at their ends: T[w][d] = [d 2^(c w)] G2, T[w][0] the "no point" entry"""
    c, nw = ge.g2e_window_bits(), ge.g2e_windows()
    for w, d in ((0, 0), (0, 1), (0, 2), (0, (1 << c) - 1), (1, 1), (nw // 2, 3), (nw - 1, 0), (nw - 1, 1), (nw - 1, (1 << c) - 1)):
        out = np.ones(48, dtype=np.uint32)
        ge.g2e_table_entry(w, d, p(out))
        v = ints(out)
        assert aff(pr.g2_mul(pr.G2_GEN, (d << (c * w)) % pr.R) if d else None) == v, (w, d)


def kilic_affine(img):   # normalised Kilic image -> affine point / None, asserting the image form
    img = np.asarray(img).reshape(3, 2, 6)
    X, Y, Z = (tuple(vi.from_u64s(img[k][j]) for j in range(2)) for k in range(3))
    if Z == (0, 0):
        assert X == (0, 0) and Y == (vi.R384, 0)                          # Kilic's Zero()
        return None
    assert Z == (vi.R384, 0)                                               # Z = 1
    ri = pow(vi.R384, -1, P)
    return ((X[0] * ri % P, X[1] * ri % P), (Y[0] * ri % P, Y[1] * ri % P))


def test_walk_on_edge_scalars(ge):
    cases = gc.edge_cases()
    assert len(cases) == 2 + 255 + 254 + 255 + 16
    ks = gc.fr_mont([k for _, k, _ in cases])
    out = np.zeros((len(cases), 3, 2, 6), dtype=np.uint64)
    ge.g2e_mul_generator(len(cases), p(ks), p(out))
    bad = [name for (name, _, want), img in zip(cases, out) if kilic_affine(img) != want]
    assert not bad, bad
    enc = np.zeros((len(cases), 96), dtype=np.uint8)
    ge.g2e_compress(len(cases), p(out), p(enc))
    assert np.array_equal(enc, gc.compressed([q for _, _, q in cases]))


def compress(ge, imgs):
    imgs = np.ascontiguousarray(imgs)
    enc = np.zeros((len(imgs), 96), dtype=np.uint8)
    ge.g2e_compress(len(imgs), p(imgs), p(enc))
    return enc


def test_compression(ge):
    rng = random.Random(32)
    pts = list(gc.fixture_points())
    want = gc.compressed(pts)
    assert [bytes(r).hex() for r in want] == list(gc.fixture_hex())
    assert np.array_equal(compress(ge, np.stack([vi.g2_kilic(Q) for Q in pts])), want)
    assert np.array_equal(compress(ge, np.stack([vi.g2_kilic(Q, vi.rand_fp2(rng)) for Q in pts])), want)      # a random Jacobian Z
    junk = vi.g2_kilic(pts[3], vi.rand_fp2(rng)); junk[2] = 0                                                  # Z = 0 whatever X and Y hold
    inf = compress(ge, np.stack([vi.g2_kilic(None), junk]))
    assert bytes(inf[0]) == bytes(inf[1]) == bytes([0xc0]) + bytes(95)
    # the sort flag when y.c1 == 0 (c0 decides): compression reads coordinates only, so the images need not be curve points
    half = (P - 1) // 2
    odd = [((5, 9), (y0, 0)) for y0 in (1, half, half + 1, P - 1)] + [((5, 9), (0, y1)) for y1 in (1, half, half + 1, P - 1)]
    enc = compress(ge, np.stack([vi.g2_kilic(Q) for Q in odd]))
    assert np.array_equal(enc, gc.compressed(odd))
    assert [bool(r[0] & 0x20) for r in enc] == [False, False, True, True] * 2
    # compress -> g2_decompress -> compress is the identity
    for row in want[:6]:
        img = np.zeros((3, 2, 6), dtype=np.uint64)
        assert ge.g2e_decompress(p(np.ascontiguousarray(row)), p(img)) == 1
        assert bytes(compress(ge, img[None])[0]) == bytes(row)
    img = np.zeros((3, 2, 6), dtype=np.uint64)
    assert ge.g2e_decompress(p(np.ascontiguousarray(inf[0])), p(img)) == 1 and kilic_affine(img) is None


@pytest.fixture(scope="module")
def ge_san():   # the same source as a program with the address and undefined-behaviour sanitizers (never loaded into python)
    os.makedirs(os.path.dirname(OUT_SAN), exist_ok=True)
    if _stale(OUT_SAN):
        # -O0 as the sanitizer build of pairing_emul.cpp (these always-inline bodies take minutes at -O1); shift-base is off for the divsteps of
        # inv<>() (field.hpp), which double a negative int32 with `<< 1`
        subprocess.check_call(["g++", "-O0", "-g", "-std=c++17", "-DG2E_MAIN", "-fsanitize=address,undefined", "-fno-sanitize=shift-base",
                               "-fno-sanitize-recover=all", "-static-libasan", "-static-libubsan", "-I", INC, "-o", OUT_SAN, SRC])
    return OUT_SAN


def test_walk_under_sanitizers(ge_san, tmp_path):
    """window bases, table entries, walk, normalisation and compression as a stand-alone program under ASan + UBSan: clean, and the right bytes"""
    cases = [c for c in gc.edge_cases() if c[0] in ("0", "1", "r-2^0", "2^8", "2^8-1", "2^254", "2^254-1", "r-2^254", "2^247", "random0", "random1")]
    assert len(cases) == 11
    path = tmp_path / "scalars.bin"
    with open(path, "wb") as f:
        f.write(np.uint64(len(cases)).tobytes())
        f.write(gc.fr_mont([k for _, k, _ in cases]).tobytes())
    env = dict(os.environ, ASAN_OPTIONS="detect_leaks=0", UBSAN_OPTIONS="print_stacktrace=1")
    run = subprocess.run([ge_san, str(path)], capture_output=True, text=True, timeout=300, env=env)
    assert run.returncode == 0 and not run.stderr.strip(), run.stderr[-2000:]
    G5 = pr.g2_mul(pr.G2_GEN, 5)
    want = [q for _, _, q in cases] + [G5, G5, pr.g2_add(G5, G5), None, None]
    assert run.stdout.split() == [pr.g2_compress(q).hex() for q in want]
