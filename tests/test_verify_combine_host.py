"""The lane bodies of the combined proof checks (go-kzg_amd/csrc/verify_combine.hpp) compiled for the host (tests/host/verify_combine_emul.cpp):
the weights against hashlib, a group's term scalars and the generator's scalar against Python integers, the partition into groups, the zero
weight of a malformed row, and the host loop of the _combined entries (combine_drive) over a model of the device: chunks, marks, re-checks,
counters and error returns across chunk boundaries.  CPU only."""
import ctypes as C
import hashlib
import os
import random
import subprocess

import pytest

import verify_cases as vc

HERE = os.path.dirname(os.path.abspath(__file__))
ROOT = os.path.dirname(HERE)
SRC = os.path.join(HERE, "host", "verify_combine_emul.cpp")
BUILD = os.path.join(HERE, "host", "_build")
OUT_SO = os.path.join(BUILD, "libverify_combine_emul.so")
INC = os.path.join(ROOT, "go-kzg_amd", "csrc")
HEADERS = ("field.hpp", "g1.hpp", "tower.hpp", "g2.hpp", "pairing.hpp", "verify_inputs.hpp", "sha256_lane.hpp", "verify_combine.hpp")
R = vc.R


def weight(seed, i):
    """r_i as the issue states it"""
    return int.from_bytes(hashlib.sha256(seed + b"KZGHIPRC" + i.to_bytes(8, "little")).digest()[:16], "little")


@pytest.fixture(scope="module")
def emul():
    os.makedirs(BUILD, exist_ok=True)
    deps = [SRC] + [os.path.join(INC, h) for h in HEADERS]
    if not os.path.exists(OUT_SO) or any(os.path.getmtime(d) > os.path.getmtime(OUT_SO) for d in deps):
        subprocess.check_call(["g++", "-O1", "-std=c++17", "-shared", "-fPIC", "-I", INC, "-o", OUT_SO, SRC])
    lib = C.CDLL(OUT_SO)
    u64 = C.c_uint64
    lib.vc_weights.argtypes = [C.c_char_p, C.POINTER(u64), u64, C.c_char_p]
    lib.vc_group_scalars.argtypes = [C.c_char_p, C.c_char_p, C.c_char_p, C.c_char_p, u64, u64, u64, C.c_char_p]
    lib.vc_group_scalars.restype = u64
    lib.vc_partition.argtypes = [u64, u64, C.POINTER(u64)]
    lib.vc_partition.restype = u64
    lib.vc_eth_fields.argtypes = [C.c_char_p] * 4 + [u64] + [C.c_char_p] * 3
    lib.vc_drive.argtypes = [C.c_char_p, u64, u64, u64, C.c_int64, C.c_int64, C.c_int, C.c_char_p] + [C.POINTER(u64)] * 4
    lib.vc_drive.restype = C.c_int
    return lib


def le(values):
    return b"".join(int(v).to_bytes(32, "little") for v in values)


def ints(buf, n):
    return [int.from_bytes(buf.raw[32 * i:32 * i + 32], "little") for i in range(n)]


SEEDS = [bytes(32), b"\xff" * 32, bytes(range(32)), hashlib.sha256(b"verify_combine").digest()]
INDICES = [0, 1, 2, 255, 256, 2 ** 32 - 1, 2 ** 32, 2 ** 32 + 1, 2 ** 63, 2 ** 64 - 1, 0x0102030405060708]


def test_weight_lane_matches_hashlib(emul):
    """i = 0, i = 2^32, both halves of the index in use, and an all-zero seed among them"""
    for seed in SEEDS:
        out = C.create_string_buffer(32 * len(INDICES))
        emul.vc_weights(seed, (C.c_uint64 * len(INDICES))(*INDICES), len(INDICES), out)
        got = ints(out, len(INDICES))
        assert got == [weight(seed, i) for i in INDICES], seed.hex()
        assert all(g < 2 ** 128 for g in got) and len(set(got)) == len(got)


def group_scalars(emul, seed, xs, ys, status, row0, rows):
    count = len(xs)
    groups = -(-count // rows)
    out = C.create_string_buffer(32 * groups * (2 * rows + 1))
    st = bytes(status) if status is not None else None
    assert emul.vc_group_scalars(seed, le(xs), le(ys), st, row0, count, rows, out) == groups
    flat = ints(out, groups * (2 * rows + 1))
    return [flat[g * (2 * rows + 1):(g + 1) * (2 * rows + 1)] for g in range(groups)]


def want_group_scalars(seed, xs, ys, status, row0, rows):
    count = len(xs)
    out = []
    for g in range(-(-count // rows)):
        r = [weight(seed, row0 + t) if t < count and not (status and status[t]) else 0 for t in range(g * rows, (g + 1) * rows)]
        x = [xs[t] if t < count else 0 for t in range(g * rows, (g + 1) * rows)]
        y = [ys[t] if t < count else 0 for t in range(g * rows, (g + 1) * rows)]
        out.append(r + [a * b % R for a, b in zip(r, x)] + [-sum(a * b for a, b in zip(r, y)) % R])
    return out


def test_term_scalars_on_edge_scalars(emul):
    """r x, u = sum r y and the generator's scalar -u against Python integers: every edge scalar as x against every edge scalar as y, one group"""
    edges = [k for _, k in vc.edge_scalars()]
    xs = [a for a in edges for _ in edges]
    ys = [b for _ in edges for b in edges]
    for seed in SEEDS[:2]:
        got = group_scalars(emul, seed, xs, ys, None, 0, len(xs))
        assert got == want_group_scalars(seed, xs, ys, None, 0, len(xs))
    # y = 0 throughout: the generator's scalar is 0, not r
    assert group_scalars(emul, SEEDS[2], edges, [0] * len(edges), None, 0, len(edges))[0][-1] == 0


@pytest.mark.parametrize("count", [1, 4, 5, 6, 11])
def test_group_partition_and_slices(emul, count):
    """5 rows per group: the groups' row ranges, and every slice's scalars (slots beyond the count are zero); the index that is hashed is the
    row's index in the CALL (row0 + t), not in its group"""
    out = (C.c_uint64 * (2 * 8))()
    groups = emul.vc_partition(count, 5, out)
    assert groups == -(-count // 5)
    assert [(out[2 * g], out[2 * g + 1]) for g in range(groups)] == [(5 * g, min(count, 5 * g + 5)) for g in range(groups)]
    rng = random.Random(count)
    xs, ys = [vc.rand_fr(rng) for _ in range(count)], [vc.rand_fr(rng) for _ in range(count)]
    for row0 in (0, 7, 2 ** 32 - 3):
        got = group_scalars(emul, SEEDS[3], xs, ys, None, row0, 5)
        assert got == want_group_scalars(SEEDS[3], xs, ys, None, row0, 5)
        last = got[-1]
        tail = count - 5 * (groups - 1)
        assert all(v == 0 for v in last[tail:5] + last[5 + tail:10]) and all(v != 0 for v in last[:tail])


def test_malformed_row_has_weight_zero(emul):
    """a row with a status contributes nothing: its r and r x are 0 and u is the sum over the others"""
    rng = random.Random(5)
    xs, ys = [vc.rand_fr(rng) for _ in range(11)], [vc.rand_fr(rng) for _ in range(11)]
    status = [0, 2, 0, 0, 3, 0, 0, 0, 0, 0, 3]
    got = group_scalars(emul, SEEDS[2], xs, ys, status, 0, 5)
    assert got == want_group_scalars(SEEDS[2], xs, ys, status, 0, 5)
    assert got[0][1] == got[0][6] == got[0][4] == got[0][9] == 0 and got[2][0] == got[2][5] == got[2][10] == 0
    assert got[0][10] == -sum(weight(SEEDS[2], t) * ys[t] for t in (0, 2, 3)) % R
    assert group_scalars(emul, SEEDS[2], xs, ys, [3] * 11, 0, 5) == [[0] * 11] * 3      # a group of malformed rows only: every scalar is zero


def test_eth_fields_status_order(emul):
    """z, then y, then the points (eth/eth.go:114-133); z and y come back reduced only when the row is valid"""
    z, y = 12345, R - 1
    rows = [(z, y, 0, 0, 0), (R, y, 0, 0, 2), (z, R, 0, 0, 2), (2 ** 256 - 1, y, 1, 1, 2), (z, y, 1, 0, 3), (z, y, 0, 1, 3), (z, R, 1, 1, 2), (0, 0, 0, 0, 0)]
    n = len(rows)
    zo, yo, st = C.create_string_buffer(32 * n), C.create_string_buffer(32 * n), C.create_string_buffer(n)
    emul.vc_eth_fields(le([r[0] for r in rows]), le([r[1] for r in rows]), bytes(r[2] for r in rows), bytes(r[3] for r in rows), n, zo, yo, st)
    assert list(st.raw) == [r[4] for r in rows]
    assert ints(zo, n) == [r[0] if not r[4] else 0 for r in rows] and ints(yo, n) == [r[1] if not r[4] else 0 for r in rows]


# ---------------- the host loop of the _combined entries ----------------
FILL = 0xEE      # what `out` holds before a call: a byte no route writes


def drive(emul, want, rows, chunk_rows, fail_chunk=-1, fail_recheck=-1, code=0):
    """combine_drive over the model: (code, out, [(i0, k, G)], [(b, e)], (groups, failed, rechecked))"""
    count = len(want)
    out = C.create_string_buffer(bytes([FILL]) * count, count)
    chunk_log, recheck_log = (C.c_uint64 * (3 * (count // chunk_rows + 1)))(), (C.c_uint64 * (2 * count))()
    calls, stats = (C.c_uint64 * 2)(), (C.c_uint64 * 3)()
    got = emul.vc_drive(bytes(want), count, rows, chunk_rows, fail_chunk, fail_recheck, code, out, chunk_log, recheck_log, calls, stats)
    return (got, list(out.raw), [tuple(chunk_log[3 * t:3 * t + 3]) for t in range(calls[0])], [tuple(recheck_log[2 * t:2 * t + 2]) for t in range(calls[1])],
            tuple(stats))


def want_drive(want, rows, chunk_rows):
    """the chunks (i0, k, G) of a call and its groups (b, e) chunk by chunk: a group never spans two chunks"""
    count = len(want)
    chunks = [(i0, min(chunk_rows, count - i0), -(-min(chunk_rows, count - i0) // rows)) for i0 in range(0, count, chunk_rows)]
    groups = [[(i0 + g * rows, min(i0 + k, i0 + (g + 1) * rows)) for g in range(G)] for i0, k, G in chunks]
    return chunks, groups


def drive_counts(rows, chunk_rows):
    return sorted({c for c in (1, rows - 1, rows, rows + 1, chunk_rows, chunk_rows + 1, 2 * chunk_rows + rows + 1) if c > 0})


@pytest.mark.parametrize("statuses", [False, True])
@pytest.mark.parametrize("chunk_groups", [1, 3])
@pytest.mark.parametrize("rows", [1, 5])
def test_drive_marks_and_rechecks_across_chunks(emul, rows, chunk_groups, statuses):
    """an invalid row on the last row of a chunk, the first row of the next and the last row of the call, each alone and all at once, and no
    invalid row at all: the output, the chunks, the re-checked ranges and the counters"""
    chunk_rows = chunk_groups * rows
    for count in drive_counts(rows, chunk_rows):
        places = sorted({i for i in (chunk_rows - 1, chunk_rows, count - 1) if i < count})
        for invalid in [[]] + [[i] for i in places] + [places]:
            want = [1] * count
            if statuses:
                for i in range(1, count, 3):
                    want[i] = 2 + i // 3 % 2
            for i in invalid:
                want[i] = 0
            code, out, chunks, rechecks, stats = drive(emul, want, rows, chunk_rows)
            where = (count, invalid)
            assert code == 0 and out == want, where
            want_chunks, groups = want_drive(want, rows, chunk_rows)
            assert chunks == want_chunks and all(i0 % chunk_rows == 0 for i0, _, _ in chunks), where
            assert [i0 for i0, _, _ in chunks] == [sum(k for _, k, _ in chunks[:t]) for t in range(len(chunks))] and sum(k for _, k, _ in chunks) == count, where
            failing = [(b, e) for chunk in groups for b, e in chunk if 0 in want[b:e]]
            assert rechecks == failing and len(failing) == len({i // rows for i in invalid}), where
            assert stats == (sum(G for _, _, G in chunks), len(failing), sum(e - b for b, e in failing)), where
            assert stats[0] == sum(-(-k // rows) for _, k, _ in chunks), where


def test_drive_group_of_status_rows_only(emul):
    """a group whose rows all carry a status passes (no live row speaks against it), is not re-checked and keeps its bytes; at one row per group too"""
    want = [1] * 5 + [2, 3, 3, 2, 3] + [1, 1, 0, 1, 1] + [3, 2, 2, 2, 3] + [1]
    code, out, chunks, rechecks, stats = drive(emul, want, 5, 15)
    assert code == 0 and out == want
    assert chunks == [(0, 15, 3), (15, 6, 2)] and rechecks == [(10, 15)] and stats == (5, 1, 5)
    want = [1, 2, 0, 3, 1]
    code, out, chunks, rechecks, stats = drive(emul, want, 1, 3)
    assert code == 0 and out == want
    assert chunks == [(0, 3, 3), (3, 2, 2)] and rechecks == [(2, 3)] and stats == (5, 1, 1)


@pytest.mark.parametrize("chunk_groups", [1, 3])
@pytest.mark.parametrize("rows", [1, 5])
def test_drive_returns_a_chunk_error_at_once(emul, rows, chunk_groups):
    """the second chunk fails: its code comes back unchanged, nothing is called after it, and neither its rows nor later ones are written"""
    chunk_rows = chunk_groups * rows
    count = 2 * chunk_rows + rows + 1
    want = [1] * count
    want[chunk_rows - 1] = want[chunk_rows] = want[count - 1] = 0
    if chunk_rows > 1:
        want[0] = 3
    for err in (8, 1):
        code, out, chunks, rechecks, stats = drive(emul, want, rows, chunk_rows, fail_chunk=1, code=err)
        assert code == err
        assert chunks == [(0, chunk_rows, chunk_groups), (chunk_rows, chunk_rows, chunk_groups)]
        assert rechecks == [(chunk_rows - rows, chunk_rows)]
        assert out == want[:chunk_rows] + [FILL] * (count - chunk_rows)
        assert stats == (chunk_groups, 1, rows)


@pytest.mark.parametrize("chunk_groups", [1, 3])
@pytest.mark.parametrize("rows", [1, 5])
def test_drive_returns_a_recheck_error_at_once(emul, rows, chunk_groups):
    """the re-check of the second chunk's first group fails, then (three groups per chunk) that of its second group: the code comes back
    unchanged, nothing is called after it, and no row from the failing group on is written"""
    chunk_rows = chunk_groups * rows
    count = 2 * chunk_rows + rows + 1
    for at in sorted({chunk_rows, chunk_rows + (chunk_groups - 1) // 2 * rows}):      # the first row of the group whose re-check fails
        want = [1] * count
        want[chunk_rows - 1] = want[at] = want[count - 1] = 0
        if chunk_rows > 1:
            want[0] = 2
        code, out, chunks, rechecks, stats = drive(emul, want, rows, chunk_rows, fail_recheck=1, code=8)
        assert code == 8
        assert chunks == [(0, chunk_rows, chunk_groups), (chunk_rows, chunk_rows, chunk_groups)]
        assert rechecks == [(chunk_rows - rows, chunk_rows), (at, at + rows)]
        assert out == want[:at] + [FILL] * (count - at)
        assert stats == (2 * chunk_groups, 2, 2 * rows)                              # counted before the call, as the entries always have
