"""wave_tower.hpp / wave_pairing.hpp, compiled for the host and replayed lane by lane (tests/host/pairing_wave_emul.cpp), against the one-lane
headers through libpairing_emul.so and against tests/pairing_ref.py.  The replay is built with KZG_WAVE_TRACE: every phase records which lanes
read and wrote each LDS slot, and a slot that one lane writes and another lane touches in the same phase counts as a race.  CPU only."""
import ctypes as C
import os
import random
import subprocess

import numpy as np
import pytest

import pairing_ref as pr
import verify_cases as vc
import verify_images as vi
from oracle import koracle as ko
from test_pairing_host import (DEVICE_EXP, S_TEST, arr, flat, g1_jac, g2_aff, g2_s_test, ints, kzg_check, p, pe, prepared,  # noqa: F401
                               rand_fp12)

HERE = os.path.dirname(os.path.abspath(__file__))
ROOT = os.path.dirname(HERE)
SRC = os.path.join(HERE, "host", "pairing_wave_emul.cpp")
OUT = os.path.join(HERE, "host", "_build", "libpairing_wave_emul.so")
OUT_SAN = os.path.join(HERE, "host", "_build", "pairing_wave_emul_san")
HEADERS = ("field.hpp", "g1.hpp", "tower.hpp", "g2.hpp", "pairing.hpp", "verify_inputs.hpp", "wave_tower.hpp", "wave_pairing.hpp")
INC = os.path.join(ROOT, "go-kzg_amd", "csrc")
OPS = {0: "mul", 1: "sqr", 2: "inv", 3: "frob", 4: "frob2", 5: "frob3", 6: "cyc_sqr", 7: "conj", 8: "mul_014"}


def stale(out):
    deps = [SRC] + [os.path.join(INC, h) for h in HEADERS]
    return not os.path.exists(out) or any(os.path.getmtime(d) > os.path.getmtime(out) for d in deps)


@pytest.fixture(scope="module")
def pw():
    os.makedirs(os.path.dirname(OUT), exist_ok=True)
    if stale(OUT):
        subprocess.check_call(["g++", "-O1", "-std=c++17", "-shared", "-fPIC", "-DKZG_WAVE_TRACE", "-I", INC, "-o", OUT, SRC])
    lib = C.CDLL(OUT)
    vp = C.c_void_p
    lib.pw_races.restype = C.c_uint64
    lib.pw_phases.restype = C.c_uint64
    lib.pw_image_bytes.restype = C.c_uint64
    lib.pw_fp12_op.argtypes = [C.c_int, vp, vp, vp, C.c_int]
    lib.pw_pairing.argtypes = [C.c_uint64, vp, vp, vp]
    lib.pw_pairing_check2.argtypes = [vp, vp]
    lib.pw_kzg_check_batch.argtypes = [C.c_uint64, vp, vp, vp, vp, vp, vp, vp, vp]
    lib.pw_pairing_value_kilic.argtypes = [vp, vp, vp]
    assert lib.pw_traced() == 1
    return lib


def edge_operands(rng):
    """random values, 0, 1, a value with c1 = 0, and all coefficients p - 1 (every carry and borrow of the reduction)"""
    return [rand_fp12(rng) for _ in range(4)] + [[0] * 12, [1] + [0] * 11, rand_fp12(rng)[:6] + [0] * 6, [pr.P - 1] * 12]


def both(pe, pw, code, a, b, inplace):
    A, B = arr(a), arr(b)
    want, got = np.zeros(144, dtype=np.uint32), np.zeros(144, dtype=np.uint32)
    pe.pe_fp12_op(code, p(A), p(B), p(want))
    pw.pw_fp12_op(code, p(A), p(B), p(got), inplace)
    return want, got


def test_trace_sees_races(pw):
    assert pw.pw_trace_selftest() == 2


@pytest.mark.parametrize("code", sorted(OPS), ids=[OPS[k] for k in sorted(OPS)])
def test_operation_bytes(pe, pw, code):
    """every operation returns the bytes of its tower.hpp function, into a fresh value and over its own operand, and no phase races"""
    rng = random.Random(100 + code)
    cases = edge_operands(rng)
    races = pw.pw_races()
    for i, a in enumerate(cases):
        for b in (rand_fp12(rng), cases[(i + 3) % len(cases)]):
            for inplace in (0, 1):
                want, got = both(pe, pw, code, a, b, inplace)
                assert np.array_equal(want, got), (OPS[code], i, inplace)
    assert pw.pw_races() == races


def test_cyclotomic_squaring_squares(pe, pw):
    rng = random.Random(8)
    g = pr.f12pow(flat(rand_fp12(rng)), (pr.P ** 6 - 1) * (pr.P ** 2 + 1))
    gt = [x for pair in pr.to_tower(g) for x in pair]
    want, got = both(pe, pw, 6, gt, [0] * 12, 0)
    assert np.array_equal(want, got) and flat(ints(got)) == pr.f12mul(g, g)


def wave_pairing(pw, pairs, zs):
    g1 = arr([v for (Pt, _), z in zip(pairs, zs) for v in g1_jac(Pt, z)])
    g2 = arr([v for _, Q in pairs for v in g2_aff(Q)])
    out = np.zeros(144, dtype=np.uint32)
    assert pw.pw_pairing(len(pairs), p(g1), p(g2), p(out)) == 1
    return g1, g2, out


def test_pairing_values(pe, pw):
    """one pair and two pairs: the bytes of pe_pairing, and the value of the reference"""
    G1, G2 = pr.G1_GEN, pr.G2_GEN
    one = [(pr.g1_mul(G1, 5), pr.g2_mul(G2, 7))]
    two = [(pr.g1_mul(G1, 3), pr.g2_mul(G2, 11)), (G1, G2)]
    races = pw.pw_races()
    for pairs, zs in ((one, [0x1234567]), (two, [2 ** 200 + 5, 1])):
        g1, g2, got = wave_pairing(pw, pairs, zs)
        want = np.zeros(144, dtype=np.uint32)
        pe.pe_pairing(len(pairs), p(g1), p(g2), p(want))
        assert np.array_equal(want, got)
        assert flat(ints(got)) == pr.multi_pairing(pairs, DEVICE_EXP)
    assert pw.pw_races() == races


def test_infinity_on_either_side(pe, pw):
    G1, G2 = pr.G1_GEN, pr.G2_GEN
    Q = pr.g2_mul(G2, 9)
    other = (pr.g1_mul(G1, 4), Q)
    ref = None
    for pairs in ([(None, G2), other], [(G1, None), other], [other, (None, None)]):
        g1, g2, got = wave_pairing(pw, pairs, [1, 3])
        want = np.zeros(144, dtype=np.uint32)
        pe.pe_pairing(2, p(g1), p(g2), p(want))
        assert np.array_equal(want, got)
        ref = got if ref is None else ref
        assert np.array_equal(ref, got)                     # the infinite pair contributes 1: what is left is e(4 G1, Q)
    g1, g2, got = wave_pairing(pw, [other], [3])
    assert np.array_equal(ref, got)
    # infinity on both sides of both pairs, and on one side of each: the product is 1 and the verdict is 1
    for pairs in ([(None, None), (None, None)], [(None, G2), (G1, None)]):
        g1, g2, got = wave_pairing(pw, pairs, [1, 1])
        assert flat(ints(got)) == pr.ONE12
        assert pw.pw_pairing_check2(p(g1), p(g2)) == 1 and pe.pe_pairing_check2(p(g1), p(g2)) == 1
    # ... and a product that is not 1
    g1, g2, _ = wave_pairing(pw, [(None, G2), other], [1, 1])
    assert pw.pw_pairing_check2(p(g1), p(g2)) == 0 and pe.pe_pairing_check2(p(g1), p(g2)) == 0
    nG = (G1[0], (-G1[1]) % pr.P)
    g1, g2, _ = wave_pairing(pw, [(pr.g1_mul(G1, 6), G2), (nG, pr.g2_mul(G2, 6))], [5, 7])
    assert pw.pw_pairing_check2(p(g1), p(g2)) == 1 and pe.pe_pairing_check2(p(g1), p(g2)) == 1


def wave_check(pw, gen, q1, cs, pis, bs, ys=None, es=None):
    n = len(cs)
    cs, pis, bs = (np.ascontiguousarray(a) for a in (cs, pis, bs))
    ys = None if ys is None else np.ascontiguousarray(ys)
    es = None if es is None else np.ascontiguousarray(es)
    ok = np.full(n, 7, dtype=np.uint8)
    pw.pw_kzg_check_batch(n, p(cs), p(pis), None if ys is None else p(ys), None if es is None else p(es), p(bs), p(gen), p(q1), p(ok))
    assert set(ok.tolist()) <= {0, 1}
    return [bool(v) for v in ok]


def test_crafted_single_rows(pe, pw, g2_s_test):
    rng = random.Random(1)
    rows = vc.single_rows(S_TEST, rng)
    gen, q1 = prepared(pe, None), prepared(pe, vi.g2_kilic(g2_s_test, vi.rand_fp2(rng)))
    cs, pis, xs, ys = vi.single_images(rows, rng)
    races = pw.pw_races()
    got = wave_check(pw, gen, q1, cs, pis, xs, ys=ys)
    assert got == kzg_check(pe, gen, q1, cs, pis, xs, ys=ys)
    bad = [(r[0], g, r[5]) for r, g in zip(rows, got) if g != r[5]]
    assert not bad, bad
    assert pw.pw_races() == races


def test_crafted_multi_rows(pe, pw):
    rng = random.Random(2)
    s = S_TEST % pr.R
    rows = vc.multi_rows(s, rng)
    gen = prepared(pe, None)
    bad = []
    for n in vc.MULTI_NS:
        sub = [r for r in rows if r[5] == n]
        qn = prepared(pe, vi.g2_kilic(pr.g2_mul(pr.G2_GEN, pow(s, n, pr.R)), vi.rand_fp2(rng)))
        cs = np.stack([vi.g1_scalar(r[1], rng.randrange(2, pr.P) if i % 2 else None) for i, r in enumerate(sub)])
        pis = np.stack([vi.g1_scalar(r[2], None if i % 3 else rng.randrange(2, pr.P)) for i, r in enumerate(sub)])
        es = np.stack([vi.g1_scalar(vc.interp_at(r[4], r[3], s), rng.randrange(2, pr.P) if i % 4 == 1 else None) for i, r in enumerate(sub)])
        bs = ko.fr_from_ints([pow(r[3], vc.next_pow2(n), pr.R) for r in sub])
        got = wave_check(pw, gen, qn, cs, pis, bs, es=es)
        assert got == kzg_check(pe, gen, qn, cs, pis, bs, es=es)
        bad += [(r[0], g, r[6]) for r, g in zip(sub, got) if g != r[6]]
    assert not bad, bad


def test_value_hook_path_on_kilic_images(pe, pw):
    """pairing_value's own first phase (a Kilic G1 image) gives the value of the reference"""
    Pt, Q = pr.g1_mul(pr.G1_GEN, 12), pr.g2_mul(pr.G2_GEN, 5)
    g1 = np.ascontiguousarray(vi.g1_scalar(12, 0x77777))
    g2 = np.ascontiguousarray(vi.g2_kilic(Q))
    out = np.zeros(144, dtype=np.uint32)
    pw.pw_pairing_value_kilic(p(g1), p(g2), p(out))
    assert flat(ints(out)) == pr.pairing(Pt, Q, DEVICE_EXP)


def test_no_race_in_any_phase(pe, pw):
    """every operation, a whole check and a value, counted from zero: thousands of phases, no slot shared between lanes within one"""
    rng = random.Random(3)
    races, phases = pw.pw_races(), pw.pw_phases()
    for code in OPS:
        for inplace in (0, 1):
            both(pe, pw, code, rand_fp12(rng), rand_fp12(rng), inplace)
    G1, G2 = pr.G1_GEN, pr.G2_GEN
    g1, g2, _ = wave_pairing(pw, [(pr.g1_mul(G1, 6), G2), ((G1[0], (-G1[1]) % pr.P), pr.g2_mul(G2, 6))], [5, 7])
    assert pw.pw_pairing_check2(p(g1), p(g2)) == 1
    assert pw.pw_phases() - phases > 2000
    assert pw.pw_races() == races == 0
    assert pw.pw_image_bytes() == 9216


@pytest.fixture(scope="module")
def pw_san():   # the replay as a program with the address and undefined-behaviour sanitizers, built as test_pairing_host.py builds PE_MAIN
    os.makedirs(os.path.dirname(OUT_SAN), exist_ok=True)
    if stale(OUT_SAN):
        subprocess.check_call(["g++", "-O0", "-g", "-std=c++17", "-DPW_MAIN", "-DKZG_WAVE_TRACE", "-fsanitize=address,undefined", "-fno-sanitize=shift-base",
                               "-fno-sanitize-recover=all", "-static-libasan", "-static-libubsan", "-I", INC, "-o", OUT_SAN, SRC])
    return OUT_SAN


def test_replay_under_sanitizers(pe, pw_san, g2_s_test, tmp_path):
    """one crafted batch through the stand-alone replay: clean under ASan / UBSan, the derived truth, no races"""
    rng = random.Random(5)
    rows = vc.single_rows(S_TEST, rng)
    rows = [r for r in rows if r[5]][:2] + [r for r in rows if not r[5]][:2]
    cs, pis, xs, ys = vi.single_images(rows, rng)
    path = tmp_path / "batch.bin"
    with open(path, "wb") as f:
        f.write(np.uint64(len(rows)).tobytes())
        for a in (cs, pis, ys, xs, vi.g2_kilic(g2_s_test)):
            f.write(np.ascontiguousarray(a).tobytes())
    env = dict(os.environ, ASAN_OPTIONS="detect_leaks=0:verify_asan_link_order=0", UBSAN_OPTIONS="print_stacktrace=1")
    run = subprocess.run([pw_san, str(path)], capture_output=True, text=True, timeout=600, env=env)
    assert run.returncode == 0 and not run.stderr.strip(), run.stderr[-2000:]
    mask, races = run.stdout.strip().split("\n")
    assert [ch == "1" for ch in mask] == [r[5] for r in rows]
    assert races == "races 0"
