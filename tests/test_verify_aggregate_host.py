"""The lane bodies of the batched block verifier (go-kzg_amd/csrc/sha256_lane.hpp, eth_aggregate.hpp) compiled for the host
(tests/host/aggregate_emul.cpp): the SHA-256 one lane runs, hashToBLSField's reduction, a sidecar's transcript and the Horner
aggregation, against hashlib and Python integers.  CPU only."""
import ctypes as C
import hashlib
import os
import subprocess

import numpy as np
import pytest

from oracle import koracle as ko

HERE = os.path.dirname(os.path.abspath(__file__))
ROOT = os.path.dirname(HERE)
SRC = os.path.join(HERE, "host", "aggregate_emul.cpp")
OUT = os.path.join(HERE, "host", "_build", "libaggregate_emul.so")
R = ko.R_MOD


@pytest.fixture(scope="module")
def ae():
    os.makedirs(os.path.dirname(OUT), exist_ok=True)
    inc = os.path.join(ROOT, "go-kzg_amd", "csrc")
    deps = [SRC] + [os.path.join(inc, h) for h in ("field.hpp", "sha256_lane.hpp", "eth_aggregate.hpp")]
    if not os.path.exists(OUT) or any(os.path.getmtime(d) > os.path.getmtime(OUT) for d in deps):
        subprocess.check_call(["g++", "-O2", "-std=c++17", "-shared", "-fPIC", "-I", inc, "-o", OUT, SRC])
    lib = C.CDLL(OUT)
    lib.ae_sha256.argtypes = [C.c_char_p, C.c_uint64, C.c_char_p]
    lib.ae_reduce.argtypes = [C.c_char_p, C.c_void_p]
    lib.ae_transcript.argtypes = [C.c_void_p, C.c_void_p, C.c_uint64, C.c_uint64, C.c_void_p, C.c_void_p]
    lib.ae_horner.argtypes = [C.c_void_p, C.c_uint64, C.c_uint64, C.c_uint64, C.c_void_p, C.c_void_p]
    return lib


def p(a):
    return a.ctypes.data_as(C.c_void_p)


def test_lane_sha256_matches_hashlib(ae):
    """every length 0..260 (all padding residues, the one- and two-block endings) and one long message of 131 072 + 32 bytes"""
    rng = np.random.default_rng(11)
    for n in list(range(0, 261)) + [131072 + 32]:
        d = rng.bytes(n)
        out = C.create_string_buffer(32)
        ae.ae_sha256(d, n, out)
        assert out.raw == hashlib.sha256(d).digest(), n


CRAFTED = [0, R - 1, R, 2 * R - 1, 2 * R, 2**256 - 1]


def test_reduction_on_crafted_digests(ae):
    """0, r - 1, r, 2r - 1, 2r, 2^256 - 1 as little-endian digests (no SHA output would hit them): zero, one and two subtractions"""
    for v in CRAFTED:
        out = ko.fr_empty(1)
        ae.ae_reduce(v.to_bytes(32, "little"), p(out))
        assert ko.fr_to_ints(out) == [v % R], hex(v)
    assert 2 * R <= 2**256 - 1 < 3 * R


def transcript_challenges(n, blobs, comms):
    h = hashlib.sha256(b"FSBLOBVERIFY_V1_" + n.to_bytes(8, "little") + len(comms).to_bytes(8, "little") + blobs + b"".join(comms)).digest()
    return [int.from_bytes(hashlib.sha256(h + bytes([t])).digest(), "little") % R for t in (0, 1)]


def test_transcript_lane_matches_hashlib(ae):
    """hashPolysComms + the two hashToBLSField calls over raw bytes in place: counts 0, 1, 3 at n = 4 and 64 (the header leaves every block
    of the chain straddling two elements; the commitments end on padding residues 0, 16, 32, 48)"""
    rng = np.random.default_rng(12)
    for n in (4, 64):
        for count in (0, 1, 2, 3, 4):
            blobs = np.frombuffer(rng.bytes(count * n * 32), dtype=np.uint8).copy() if count else np.zeros(32, dtype=np.uint8)
            comms = np.frombuffer(rng.bytes(count * 48), dtype=np.uint8).copy() if count else np.zeros(48, dtype=np.uint8)
            r_out, z_out = ko.fr_empty(1), ko.fr_empty(1)
            ae.ae_transcript(p(blobs), p(comms), n, count, p(r_out), p(z_out))
            want = transcript_challenges(n, blobs.tobytes()[:count * n * 32], [comms.tobytes()[48 * i:48 * i + 48] for i in range(count)])
            assert [ko.fr_to_ints(r_out)[0], ko.fr_to_ints(z_out)[0]] == want, (n, count)


def test_horner_lane_against_python_integers(ae):
    """sum_k r^k blob_k[i] on plain limbs for 0, 1, 2 and 5 blobs, r - 1 among the values; an element equal to r is flagged"""
    rng = np.random.default_rng(13)
    n = 8
    r_chal = int.from_bytes(rng.bytes(32), "little") % R
    r_mont = ko.fr_from_ints([r_chal])
    for count in (0, 1, 2, 5):
        vals = [[int.from_bytes(rng.bytes(32), "little") % R for _ in range(n)] for _ in range(count)]
        if count:
            vals[count - 1][3] = R - 1
            vals[0][5] = R - 1
            vals[0][6] = 0
        raw = np.frombuffer(b"".join(v.to_bytes(32, "little") for row in vals for v in row) or bytes(32), dtype=np.uint8).copy()
        for i in range(n):
            out = ko.fr_empty(1)
            assert ae.ae_horner(p(raw), n, count, i, p(r_mont), p(out)) == 1
            assert ko.fr_to_ints(out) == [sum(pow(r_chal, k, R) * vals[k][i] for k in range(count)) % R], (count, i)
    # an element equal to r (and one above it) in one coefficient of one blob: that coefficient's lane reports it, the others do not
    for bad in (R, R + 1, 2**256 - 1):
        vals = [[1, 2, 3, 4, 5, 6, 7, 8], [9, 10, bad, 12, 13, 14, 15, 16], [1, 1, 1, 1, 1, 1, 1, 1]]
        raw = np.frombuffer(b"".join(v.to_bytes(32, "little") for row in vals for v in row), dtype=np.uint8).copy()
        flags = [ae.ae_horner(p(raw), n, 3, i, p(r_mont), p(ko.fr_empty(1))) for i in range(n)]
        assert flags == [1, 1, 0, 1, 1, 1, 1, 1], hex(bad)


def test_python_signature_table_resolves_the_new_symbols():
    import gokzg_amd
    L = gokzg_amd.lib()
    for name in ("kzg_hip_eth_verify_aggregate_kzg_proof_batch", "kzg_hip_test_sha256_lanes", "kzg_hip_test_hash_to_bls_field_lanes"):
        assert getattr(L, name).argtypes is not None, name
    assert len(L.kzg_hip_eth_verify_aggregate_kzg_proof_batch.argtypes) == 10
    assert hasattr(gokzg_amd.EthSettings, "verify_aggregate_kzg_proof_batch")
