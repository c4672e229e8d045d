"""The lane bodies of the combined multi-proof check (go-kzg_amd/csrc/verify_combine_multi.hpp) compiled for the host
(tests/host/verify_combine_multi_emul.cpp): a row's term scalars and the weights of its coefficients against hashlib and Python integers, and
whole calls replayed workgroup by workgroup and lane by lane -- tiles of 256, 1 and 44 rows, a short last group, dead rows inside a tile --
whose J_g and term scalars are compared with the sums as DESIGN.md (4a) states them.  CPU only."""
import ctypes as C
import hashlib
import os
import random
import subprocess

import pytest

import verify_cases as vc

HERE = os.path.dirname(os.path.abspath(__file__))
ROOT = os.path.dirname(HERE)
SRC = os.path.join(HERE, "host", "verify_combine_multi_emul.cpp")
BUILD = os.path.join(HERE, "host", "_build")
OUT_SO = os.path.join(BUILD, "libverify_combine_multi_emul.so")
INC = os.path.join(ROOT, "go-kzg_amd", "csrc")
HEADERS = ("field.hpp", "g1.hpp", "tower.hpp", "g2.hpp", "pairing.hpp", "verify_inputs.hpp", "sha256_lane.hpp", "verify_combine.hpp", "verify_combine_multi.hpp")
R = vc.R
SEED = hashlib.sha256(b"verify_combine_multi").digest()


def weight(seed, i):
    """r_i: the single form's weights, same tag"""
    return int.from_bytes(hashlib.sha256(seed + b"KZGHIPRC" + i.to_bytes(8, "little")).digest()[:16], "little")


@pytest.fixture(scope="module")
def emul():
    os.makedirs(BUILD, exist_ok=True)
    deps = [SRC] + [os.path.join(INC, h) for h in HEADERS]
    if not os.path.exists(OUT_SO) or any(os.path.getmtime(d) > os.path.getmtime(OUT_SO) for d in deps):
        subprocess.check_call(["g++", "-O1", "-std=c++17", "-shared", "-fPIC", "-I", INC, "-o", OUT_SO, SRC])
    lib = C.CDLL(OUT_SO)
    u64 = C.c_uint64
    lib.vcm_row_scalars.argtypes = [C.c_char_p, C.POINTER(u64), C.c_char_p, C.c_char_p, u64, u64, C.c_char_p, C.c_char_p, C.c_char_p]
    lib.vcm_coeff_weights.argtypes = [C.c_char_p, C.c_char_p, u64, C.c_char_p]
    lib.vcm_groups.argtypes = [C.c_char_p, C.c_char_p, C.c_char_p, u64, u64, u64, u64, C.c_char_p, C.c_char_p]
    lib.vcm_groups.restype = u64
    return lib


def le(values):
    return b"".join(int(v).to_bytes(32, "little") for v in values)


def ints(buf, n):
    return [int.from_bytes(buf.raw[32 * i:32 * i + 32], "little") for i in range(n)]


@pytest.mark.parametrize("npad", [1, 4, 32])
def test_row_scalars(emul, npad):
    """x in {0, 1, r - 1, random}, live and dead: r is the single form's weight, r x^np, and the base x^-1 with InvModFr(0) = 0; a dead row
    gets zeros whatever its x"""
    rng = random.Random(npad)
    xs = [0, 1, R - 1, vc.rand_fr(rng), vc.rand_fr(rng)] * 2
    live = [1] * 5 + [0] * 5
    idx = [0, 1, 255, 2 ** 32, 2 ** 64 - 1, 3, 4, 5, 6, 7]
    n = len(xs)
    r, rxp, base = (C.create_string_buffer(32 * n) for _ in range(3))
    emul.vcm_row_scalars(SEED, (C.c_uint64 * n)(*idx), bytes(live), le(xs), npad, n, r, rxp, base)
    want_r = [weight(SEED, i) if lv else 0 for i, lv in zip(idx, live)]
    assert ints(r, n) == want_r
    assert ints(rxp, n) == [w * pow(x, npad, R) % R for w, x in zip(want_r, xs)]
    assert ints(base, n) == [vc.inv(x) if lv else 0 for x, lv in zip(xs, live)]
    assert ints(base, n)[0] == 0 and ints(rxp, n)[0] == 0 and ints(r, n)[0] != 0          # x = 0, live


@pytest.mark.parametrize("npad", [1, 4, 32, 256])
def test_coefficient_weights(emul, npad):
    """r x^-j for every j < np from the base; base 0 (x = 0): r at j = 0, then zeros"""
    rng = random.Random(100 + npad)
    r = weight(SEED, 9)
    for x in (0, 1, R - 1, vc.rand_fr(rng)):
        out = C.create_string_buffer(32 * npad)
        emul.vcm_coeff_weights(le([r]), le([vc.inv(x)]), npad, out)
        assert ints(out, npad) == [r * pow(vc.inv(x), j, R) % R for j in range(npad)], x
    assert ints(out, npad)[0] == r


def want_groups(seed, xs, coef, npad, row0, rows):
    """(slices, J) from the sums: J_g[j] = sum r_i x_i^-j c_i[j], slice = r | r x^np | -1"""
    count = len(xs)
    slices, js = [], []
    for g0 in range(0, count, rows):
        members = range(g0, min(count, g0 + rows))
        r = [weight(seed, row0 + t) for t in members]
        pad = [0] * (rows - len(r))
        slices.append(r + pad + [w * pow(xs[t], npad, R) % R for w, t in zip(r, members)] + pad + [R - 1])
        js.append([sum(w * pow(vc.inv(xs[t]), j, R) * coef[t][j] for w, t in zip(r, members)) % R for j in range(npad)])
    return slices, js


def run_groups(emul, seed, xs, coef, npad, row0, rows):
    count = len(xs)
    groups = -(-count // rows)
    sc, jj = C.create_string_buffer(32 * groups * (2 * rows + 1)), C.create_string_buffer(32 * groups * npad)
    assert emul.vcm_groups(seed, le(xs), le(v for row in coef for v in row), npad, row0, count, rows, sc, jj) == groups
    flat, fj = ints(sc, groups * (2 * rows + 1)), ints(jj, groups * npad)
    return ([flat[g * (2 * rows + 1):(g + 1) * (2 * rows + 1)] for g in range(groups)], [fj[g * npad:(g + 1) * npad] for g in range(groups)])


def rows_of(rng, count, npad):
    xs = [vc.rand_fr(rng) for _ in range(count)]
    for at, x in ((0, 0), (count // 2, 1), (count - 1, R - 1)):
        xs[at] = x
    return xs, [[vc.rand_fr(rng) for _ in range(npad)] for _ in range(count)]


@pytest.mark.parametrize("n", [1, 2, 32, 3, 5, 12])
@pytest.mark.parametrize("count", [1, 4, 5, 6, 11])
def test_groups_of_five(emul, n, count):
    npad = vc.next_pow2(n)
    xs, coef = rows_of(random.Random(1000 * n + count), count, npad)
    for row0 in (0, 2 ** 32 - 3):
        assert run_groups(emul, SEED, xs, coef, npad, row0, 5) == want_groups(SEED, xs, coef, npad, row0, 5)


@pytest.mark.parametrize("n", [1, 2, 32, 3, 5, 12])
@pytest.mark.parametrize("rows", [257, 300])
def test_six_hundred_rows_across_tiles(emul, n, rows):
    """R = 257: tiles of 256 and 1 rows, groups of 257, 257 and 86; R = 300: tiles of 256 and 44 rows, two full groups.  Every slot of every
    slice is written (the emulation starts them at one) and no lane reads outside the coefficients (the emulation returns 0)"""
    npad = vc.next_pow2(n)
    xs, coef = rows_of(random.Random(77 * n + rows), 600, npad)
    got, want = run_groups(emul, SEED, xs, coef, npad, 11, rows), want_groups(SEED, xs, coef, npad, 11, rows)
    assert got[1] == want[1]
    assert got[0] == want[0]


def test_j_does_not_depend_on_the_tiling(emul):
    """the same rows as one group of 600 (three tiles) and as one group of 1024 (four tiles, the last one dead)"""
    xs, coef = rows_of(random.Random(5), 600, 8)
    a, b = run_groups(emul, SEED, xs, coef, 8, 0, 600), run_groups(emul, SEED, xs, coef, 8, 0, 1024)
    assert a[1] == b[1] == want_groups(SEED, xs, coef, 8, 0, 600)[1]
