"""The lane bodies of recover_rows.hpp (erasure lists, the ragged product tree, the strip division, the row status), replayed on the host over whole small
problems by tests/host/recovery_batch_emul.cpp and compared bit for bit with the oracle.  CPU only."""
import os
import random
import subprocess

import numpy as np
import pytest

import recovery_batch_cases as rc
from oracle import koracle as ko

HERE = os.path.dirname(os.path.abspath(__file__))
ROOT = os.path.dirname(HERE)
SRC = os.path.join(HERE, "host", "recovery_batch_emul.cpp")
OUT = os.path.join(HERE, "host", "_build", "recovery_batch_emul")
OUT_SAN = os.path.join(HERE, "host", "_build", "recovery_batch_emul_san")
INC = os.path.join(ROOT, "go-kzg_amd", "csrc")
HEADERS = ("field.hpp", "fr_lazy.hpp", "recover_rows.hpp")
STRIP = 64


def _stale(out):
    deps = [SRC] + [os.path.join(INC, h) for h in HEADERS]
    return not os.path.exists(out) or any(os.path.getmtime(d) > os.path.getmtime(out) for d in deps)


@pytest.fixture(scope="module")
def emul():
    os.makedirs(os.path.dirname(OUT), exist_ok=True)
    if _stale(OUT):
        subprocess.check_call(["g++", "-O1", "-std=c++17", "-I", INC, "-o", OUT, SRC])
    return OUT


@pytest.fixture(scope="module")
def emul_san():   # the same program under the address and undefined-behaviour sanitizers (a stand-alone binary: nothing is loaded into python)
    os.makedirs(os.path.dirname(OUT_SAN), exist_ok=True)
    if _stale(OUT_SAN):
        # shift-base is off for the divsteps of inv<>() (field.hpp), which double a negative int32 with `<< 1`
        subprocess.check_call(["g++", "-O1", "-g", "-std=c++17", "-fsanitize=address,undefined", "-fno-sanitize=shift-base", "-fno-sanitize-recover=all",
                               "-static-libasan", "-static-libubsan", "-I", INC, "-o", OUT_SAN, SRC])
    return OUT_SAN


def u64(*v):
    return np.array(v, dtype=np.uint64).tobytes()


def case_recover(samples, present, tree, shared=False):
    return u64(0, samples.shape[0], int(tree), int(shared)) + np.ascontiguousarray(samples).tobytes() + np.ascontiguousarray(present, dtype=np.uint8).tobytes()


def case_zero(lists, n, tree, segs):
    pad = np.zeros((len(lists), n), dtype=np.uint64)
    for r, m in enumerate(lists):
        pad[r, :len(m)] = m
    return u64(1, len(lists), int(tree), segs) + u64(*[len(m) for m in lists]) + pad.tobytes()


def case_strip(den, num):
    return u64(2, den.shape[0], int(num is not None)) + den.tobytes() + (num if num is not None else den).tobytes()


def case_status(recon, samples, present):
    return u64(3, recon.shape[0]) + recon.tobytes() + samples.tobytes() + np.ascontiguousarray(present, dtype=np.uint8).tobytes()


def run(binary, tmp_path, n, cases, name="cases.bin"):
    ofs = ko.FFTSettings(max(n.bit_length() - 1, 1))
    step = (1 << max(n.bit_length() - 1, 1)) // n
    path = tmp_path / name
    with open(path, "wb") as f:
        f.write(u64(n) + np.ascontiguousarray(ofs.expanded_roots()[::step]).tobytes() + np.ascontiguousarray(ofs.reverse_roots()[::step]).tobytes() + u64(len(cases)))
        for c in cases:
            f.write(c)
    env = dict(os.environ, ASAN_OPTIONS="detect_leaks=0", UBSAN_OPTIONS="print_stacktrace=1")
    done = subprocess.run([binary, str(path)], capture_output=True, text=True, timeout=300, env=env)
    assert done.returncode == 0 and not done.stderr.strip(), done.stderr[-2000:]
    return [line.split() for line in done.stdout.splitlines()]


def fr_rows(hexes, n):
    return np.frombuffer(bytes.fromhex(hexes), dtype=np.uint64).reshape(-1, n, 4)


def lists_for(n, counts, rng):
    return [np.sort(rng.permutation(n)[:c]).astype(np.uint64) for c in counts]


SHAPES = {16: (1, 8, 15), 64: (17, 32, 33)}   # one leaf and no tree level; two or four leaves with a partial leaf and a non-zero pad


def zero_cases(n):
    rng = np.random.default_rng(100 + n)
    chunks = [lists_for(n, [c], rng) for c in SHAPES[n]]                      # every shape alone: its own leaf count
    chunks.append(lists_for(n, list(SHAPES[n]) + [1, n - 1, 2], rng))         # one chunk: the leaf count is shared, the pads are per row
    chunks.append(lists_for(n, [3, 1, 16 if n > 16 else 5], rng))
    return chunks


@pytest.mark.parametrize("n", sorted(SHAPES))
def test_zero_polynomials_match_the_oracle(emul, tmp_path, n):
    ofs = ko.FFTSettings(n.bit_length() - 1)
    chunks = zero_cases(n)
    modes = [(0, 1), (0, 4), (1, 1)]                                         # direct in one piece, direct in four (rows with fewer roots than pieces), tree
    lines = run(emul, tmp_path, n, [case_zero(ch, n, tree, segs) for tree, segs in modes for ch in chunks])
    want = [ofs.zero_poly_via_multiplication(m, n) for ch in chunks for m in ch]
    assert len(lines) == len(modes) * len(want)
    for k, line in enumerate(lines):
        ze, zp = want[k % len(want)]
        assert line[0] == "Z"
        assert np.array_equal(fr_rows(line[1], n)[0], ze) and np.array_equal(fr_rows(line[2], n)[0], zp), (n, k)


def recovery_chunk(n, seed):
    """per-row masks with the shape's counts, a row with nothing missing, one with nothing present in the middle, a full-degree polynomial with half missing"""
    ofs = ko.FFTSettings(n.bit_length() - 1)
    rng = np.random.default_rng(seed)
    counts = [SHAPES[n][0], 0, SHAPES[n][1], n, SHAPES[n][2], n // 2, 1]
    data = rc.data_rows(ofs, n, len(counts), seed, full_degree=(5,))
    present = np.stack([rc.mask(n, c, rng) for c in counts])
    return ofs, data, present


def check_rows(lines, ofs, samples, present, n):
    assert len(lines) == samples.shape[0]
    for r, line in enumerate(lines):
        pr = present if present.ndim == 1 else present[r]
        status, row = int(line[1]), fr_rows(line[2], n)[0]
        missing = int((pr == 0).sum())
        if missing == n:
            assert status == rc.ERR_BAD_ARG and not row.any(), r
        elif missing == 0:
            assert status == rc.OK and np.array_equal(row, samples[r]), r   # copied through (the oracle refuses a row with nothing missing)
        else:
            assert status == rc.OK and np.array_equal(row, ofs.recover_poly_from_samples(samples[r], pr)), r


@pytest.mark.parametrize("n", sorted(SHAPES))
def test_recovery_matches_the_oracle(emul, tmp_path, n):
    ofs, data, present = recovery_chunk(n, 7 * n)
    samples = rc.blanked(data, present)
    shared = present[4]
    shared_samples = rc.blanked(data, shared)
    cases = [case_recover(samples, present, tree) for tree in (0, 1)] + [case_recover(shared_samples, shared, tree, shared=True) for tree in (0, 1)]
    cases += [case_recover(samples[k:k + 1], present[k:k + 1], 1) for k in (0, 2, 4)]        # a row alone: the chunk's leaf count is its own
    lines = run(emul, tmp_path, n, cases)
    rows = samples.shape[0]
    for k in range(2):
        check_rows(lines[k * rows:(k + 1) * rows], ofs, samples, present, n)
        check_rows(lines[(2 + k) * rows:(3 + k) * rows], ofs, shared_samples, shared, n)
    for j, k in enumerate((0, 2, 4)):
        check_rows(lines[4 * rows + j:4 * rows + j + 1], ofs, samples[k:k + 1], present[k:k + 1], n)
    good = [r for r in range(rows) if 0 < (present[r] == 0).sum() <= n // 2 and r != 5]
    for r in good:                                                           # (the reference's own property: half-degree data comes back)
        assert np.array_equal(fr_rows(lines[r][2], n)[0], data[r])


def test_strip_division(emul, tmp_path):
    """strips of 64 laid across rows of 16: one row fewer than a strip, exactly a strip, one more; tiny totals; zero denominators count as one"""
    rng = random.Random(5)
    cases, want = [], []
    for total in (1, 2, STRIP - 1, STRIP, STRIP + 1, 16 * (STRIP - 1), 16 * STRIP, 16 * (STRIP + 1)):
        for with_num in (True, False):
            den = [rng.randrange(1, ko.R_MOD) for _ in range(total)]
            for z in {0, total // 2, total - 1} if total > 2 else ():
                den[z] = 0
            num = [rng.randrange(ko.R_MOD) for _ in range(total)]
            cases.append(case_strip(ko.fr_from_ints(den), ko.fr_from_ints(num) if with_num else None))
            want.append([(a if with_num else 1) * pow(d or 1, -1, ko.R_MOD) % ko.R_MOD for a, d in zip(num, den)])
    lines = run(emul, tmp_path, 16, cases)
    assert len(lines) == len(want)
    for line, w in zip(lines, want):
        assert line[0] == "S" and ko.fr_to_ints(fr_rows(line[1], len(w))[0]) == w, len(w)


def test_row_status_on_crafted_rows(emul, tmp_path):
    """the only way into KZG_HIP_ERR_RECOVERY: a present sample that the reconstruction does not reproduce; its neighbours keep their own status"""
    n = 16
    ofs = ko.FFTSettings(4)
    rng = np.random.default_rng(3)
    recon = rc.data_rows(ofs, n, 6, 40)
    present = np.stack([rc.mask(n, c, rng) for c in (4, 4, n, 4, 0, 4)])
    samples = rc.blanked(recon, present)
    bad = int(np.nonzero(present[1])[0][-1])
    samples[1, bad, 0] ^= 1                                                  # row 1: a present sample differs
    hole = int(np.nonzero(present[3] == 0)[0][0])
    samples[3, hole] = 77                                                    # row 3: junk where nothing is present is not looked at
    samples[4, 2, 1] ^= 4                                                    # row 4: nothing missing, so nothing is compared: copied through as it is
    lines = run(emul, tmp_path, n, [case_status(recon, samples, present)])
    got = [(int(l[1]), fr_rows(l[2], n)[0]) for l in lines]
    zeros = np.zeros((n, 4), dtype=np.uint64)
    want = [(rc.OK, recon[0]), (rc.ERR_RECOVERY, zeros), (rc.ERR_BAD_ARG, zeros), (rc.OK, recon[3]), (rc.OK, samples[4]), (rc.OK, recon[5])]
    for r, ((st, row), (wst, wrow)) in enumerate(zip(got, want)):
        assert st == wst and np.array_equal(row, wrow), r


def test_under_sanitizers(emul, emul_san, tmp_path):
    """every case kind once more as a stand-alone program under ASan + UBSan: clean, and the same lines"""
    for n in sorted(SHAPES):
        ofs, data, present = recovery_chunk(n, 11 * n)
        samples = rc.blanked(data, present)
        cases = [case_recover(samples, present, tree) for tree in (0, 1)] + [case_recover(rc.blanked(data, present[0]), present[0], 1, shared=True)]
        cases += [case_zero(ch, n, tree, segs) for tree, segs in ((0, 4), (1, 1)) for ch in zero_cases(n)[-2:]]
        den = ko.fr_from_ints(list(range(0, 16 * STRIP + 16)))
        cases += [case_strip(den, den[::-1].copy()), case_strip(den[:STRIP + 1].copy(), None), case_status(data, samples, present)]
        assert run(emul_san, tmp_path, n, cases, "san.bin") == run(emul, tmp_path, n, cases, "plain.bin")


def test_new_entry_points_are_bound():
    """declared in the header, exported, and in the binding's signature table with the header's argument counts (test_cabi.py covers the first two in general)"""
    import re
    import gokzg_amd as kz
    header = open(os.path.join(ROOT, "include", "kzg_hip.h")).read()
    L = kz.lib()
    for name, nargs in (("kzg_hip_recover_poly_from_samples_batch", 8), ("kzg_hip_recover_poly_from_samples_batch_dev", 9), ("kzg_hip_zero_poly_via_multiplication_batch", 8)):
        proto = re.search(r"int\s+%s\s*\(([^;]*)\)\s*;" % name, header)
        assert proto and proto.group(1).count(",") + 1 == nargs, name
        assert len(getattr(L, name).argtypes) == nargs, name
    assert hasattr(kz.FFTSettings, "recover_poly_from_samples_batch") and hasattr(kz.FFTSettings, "zero_poly_via_multiplication_batch")
