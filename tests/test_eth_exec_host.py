"""The lane bodies of the batched execution-layer calls (go-kzg_amd/csrc/eth_exec.hpp) and the host-side transaction peek (eth_tx.hpp) compiled
for the host (tests/host/eth_exec_emul.cpp): KZGToVersionedHash against hashlib, the status precedence of a PointEvaluationPrecompile input,
and TxPeekBlobVersionedHashes against the Python restatement of tests/eth_exec_cases.py, plain and as a stand-alone program under the address
and undefined-behaviour sanitizers.  CPU only."""
import ctypes as C
import hashlib
import os
import random
import subprocess

import numpy as np
import pytest

import eth_exec_cases as ec
import verify_images as vi
from oracle import koracle as ko

HERE = os.path.dirname(os.path.abspath(__file__))
ROOT = os.path.dirname(HERE)
SRC = os.path.join(HERE, "host", "eth_exec_emul.cpp")
BUILD = os.path.join(HERE, "host", "_build")
OUT_SO = os.path.join(BUILD, "libeth_exec_emul.so")
OUT = os.path.join(BUILD, "eth_exec_emul")
OUT_SAN = os.path.join(BUILD, "eth_exec_emul_san")
INC = os.path.join(ROOT, "go-kzg_amd", "csrc")
HEADERS = ("field.hpp", "g1.hpp", "tower.hpp", "g2.hpp", "pairing.hpp", "verify_inputs.hpp", "sha256_lane.hpp", "eth_exec.hpp", "eth_tx.hpp")
R = ko.R_MOD


def _stale(out):
    deps = [SRC] + [os.path.join(INC, h) for h in HEADERS]
    return not os.path.exists(out) or any(os.path.getmtime(d) > os.path.getmtime(out) for d in deps)


@pytest.fixture(scope="module")
def ee():
    os.makedirs(BUILD, exist_ok=True)
    if _stale(OUT_SO):
        subprocess.check_call(["g++", "-O1", "-std=c++17", "-shared", "-fPIC", "-I", INC, "-o", OUT_SO, SRC])
    lib = C.CDLL(OUT_SO)
    lib.ee_versioned_hashes.argtypes = [C.c_char_p, C.c_uint64, C.c_char_p]
    lib.ee_precompile_inputs.argtypes = [C.c_char_p, C.c_uint64, C.c_char_p, C.c_char_p]
    return lib


@pytest.fixture(scope="module")
def emul():
    os.makedirs(BUILD, exist_ok=True)
    if _stale(OUT):
        subprocess.check_call(["g++", "-O1", "-std=c++17", "-DEE_MAIN", "-I", INC, "-o", OUT, SRC])
    return OUT


@pytest.fixture(scope="module")
def emul_san():   # the same program under the sanitizers (a stand-alone binary: nothing is loaded into python)
    os.makedirs(BUILD, exist_ok=True)
    if _stale(OUT_SAN):
        # shift-base is off for the divsteps of inv<>() (field.hpp), which double a negative int32 with `<< 1`
        subprocess.check_call(["g++", "-O1", "-g", "-std=c++17", "-DEE_MAIN", "-fsanitize=address,undefined", "-fno-sanitize=shift-base", "-fno-sanitize-recover=all",
                               "-static-libasan", "-static-libubsan", "-I", INC, "-o", OUT_SAN, SRC])
    return OUT_SAN


# ---------------- KZGToVersionedHash ----------------
def hash_inputs():
    rng = random.Random(41)
    return [rng.randbytes(48) for _ in range(1000)] + [bytes(48), b"\xff" * 48, bytes(vi.compress_scalar(1))]


def test_versioned_hash_lane_matches_hashlib(ee):
    """1000 random 48-byte strings, all-zero, all-0xff and the compressed generator: SHA-256 with byte 0 replaced by 0x01"""
    ins = hash_inputs()
    out = C.create_string_buffer(32 * len(ins))
    ee.ee_versioned_hashes(b"".join(ins), len(ins), out)
    for i, c in enumerate(ins):
        want = b"\x01" + hashlib.sha256(c).digest()[1:]
        assert out.raw[32 * i:32 * i + 32] == want, i
    assert ins[-1][0] & 0x80 and len({out.raw[32 * i] for i in range(len(ins))}) == 1


# ---------------- the status of one precompile input ----------------
@pytest.fixture(scope="module")
def valid_row():
    """commitment, z, y, proof of a row whose inputs all parse (s = 1337: C = [y + (s - z) t] G1, pi = [t] G1)"""
    rng = random.Random(42)
    t, z, y = (rng.randrange(1, R) for _ in range(3))
    return bytes(vi.compress_scalar(y + (1337 - z) * t)), z.to_bytes(32, "little"), y.to_bytes(32, "little"), bytes(vi.compress_scalar(t))


UNDECODABLE = bytes([0x80]) + bytes(47)          # x = 0: (0, 2), on the curve, of order 3
GE_R = R.to_bytes(32, "little")


def spoil(h):
    return h[:7] + bytes([h[7] ^ 0x10]) + h[8:]


def run_row(ee, c, z, y, pi, right_hash):
    h = ec.versioned_hash(c)
    row = (h if right_hash else spoil(h)) + z + y + c + pi
    assert len(row) == 192
    st, inf = C.create_string_buffer(1), C.create_string_buffer(1)
    ee.ee_precompile_inputs(row, 1, st, inf)
    return st.raw[0], inf.raw[0]


def test_precompile_row_valid_inputs(ee, valid_row):
    c, z, y, pi = valid_row
    assert run_row(ee, c, z, y, pi, True) == (0, 0)


def test_precompile_row_spoiled_hash_alone(ee, valid_row):
    c, z, y, pi = valid_row
    assert run_row(ee, c, z, y, pi, False) == (4, 1)


def test_precompile_row_spoiled_hash_and_z_not_below_r(ee, valid_row):
    c, z, y, pi = valid_row
    assert run_row(ee, c, GE_R, y, pi, False) == (4, 1)


def test_precompile_row_spoiled_hash_and_undecodable_commitment(ee, valid_row):
    c, z, y, pi = valid_row
    assert run_row(ee, UNDECODABLE, z, y, pi, False) == (4, 1)


def test_precompile_row_right_hash_and_z_not_below_r(ee, valid_row):
    c, z, y, pi = valid_row
    assert run_row(ee, c, GE_R, y, pi, True) == (2, 1)


def test_precompile_row_right_hash_and_y_not_below_r(ee, valid_row):
    c, z, y, pi = valid_row
    assert run_row(ee, c, z, (2 ** 256 - 1).to_bytes(32, "little"), pi, True) == (2, 1)


def test_precompile_row_right_hash_and_undecodable_commitment(ee, valid_row):
    c, z, y, pi = valid_row
    assert run_row(ee, UNDECODABLE, z, y, pi, True) == (3, 1)      # the hash of the undecodable bytes is right: hashed before decoded


def test_precompile_row_right_hash_and_undecodable_proof(ee, valid_row):
    c, z, y, pi = valid_row
    assert run_row(ee, c, z, y, UNDECODABLE, True) == (3, 1)


def test_precompile_row_right_hash_field_before_point(ee, valid_row):
    c, z, y, pi = valid_row
    assert run_row(ee, UNDECODABLE, z, GE_R, UNDECODABLE, True) == (2, 1)


# ---------------- TxPeekBlobVersionedHashes ----------------
def peek_inputs():
    rng = random.Random(43)
    hashes = [rng.randbytes(32) for _ in range(4)]
    valid = ec.blob_tx(hashes, rng, dynamic=10)                      # 262 + 10 + 128 = 400 bytes
    assert len(valid) == 400 and ec.tx_peek(valid) == (0, 272, 4)
    txs = [valid[:n] for n in range(0, 401)]                         # every prefix length 0 .. 400
    n = len(valid)
    for field in (0, ec.MIN_OFFSET, n - 70, n - 69, 0xffffffff):     # the offset field at its edges
        txs.append(valid[:258] + field.to_bytes(4, "little") + valid[262:])
    for trailing in (0, 31, 32, 33):
        txs.append(ec.blob_tx([], rng, dynamic=0) + rng.randbytes(trailing))
    for tx_type in (0, 2, 5):
        for length in (1, 261, 262, 300):
            txs.append(bytes([tx_type]) + valid[1:length])
    return txs


def run_program(binary, tmp_path, txs, comms, name):
    path = tmp_path / name
    with open(path, "wb") as f:
        f.write(len(txs).to_bytes(8, "little"))
        for tx in txs:
            f.write(len(tx).to_bytes(8, "little") + tx)
        f.write(len(comms).to_bytes(8, "little") + b"".join(comms))
    env = dict(os.environ, ASAN_OPTIONS="detect_leaks=0", UBSAN_OPTIONS="print_stacktrace=1")
    done = subprocess.run([binary, str(path)], capture_output=True, text=True, timeout=120, env=env)
    assert done.returncode == 0 and not done.stderr.strip(), (done.returncode, done.stderr[-2000:])
    lines = [line.split() for line in done.stdout.splitlines()]
    return [tuple(int(v) for v in l[1:]) for l in lines if l[0] == "T"], [bytes.fromhex(l[1]) for l in lines if l[0] == "H"]


def test_tx_peek_matches_the_python_restatement(emul, tmp_path):
    txs = peek_inputs()
    got, _ = run_program(emul, tmp_path, txs, [], "plain.bin")
    want = [ec.tx_peek(tx) for tx in txs]
    assert got == want
    assert {w[0] for w in want} == {0, 6, 7, 8}
    # the edges by hand: offset field 0 on a 400-byte transaction leaves 330 trailing bytes (no multiple of 32); len - 70 is "no hashes";
    # len - 69 and 0xffffffff are out of bounds (the sum is formed in 64 bits); 192 leaves 138 bytes
    assert want[401:406] == [(8, 0, 0), (8, 0, 0), (0, 400, 0), (7, 0, 0), (7, 0, 0)]
    assert want[406:410] == [(0, 262, 0), (8, 0, 0), (0, 262, 1), (8, 0, 0)]
    assert want[0] == (6, 0, 0) and want[261] == (6, 0, 0) and want[262][0] != 6


def test_tx_peek_and_hash_lane_under_sanitizers(emul, emul_san, tmp_path):
    """the same inputs through the program built with ASan + UBSan, every transaction in an allocation of exactly its length: no read out of
    bounds, and the same lines"""
    txs, comms = peek_inputs(), hash_inputs()[-8:]
    plain = run_program(emul, tmp_path, txs, comms, "plain.bin")
    assert run_program(emul_san, tmp_path, txs, comms, "san.bin") == plain
    assert plain[1] == [ec.versioned_hash(c) for c in comms]


def test_block_restatement_on_the_named_blocks():
    """Pins the REFERENCE, not the library: the Python restatement (eth_exec_cases.verify_block) on the blocks whose names say what they are,
    against codes written down by hand from eth/eth.go:234-282.  It runs no library code and passes with or without it; the GPU test
    test_gpu_eth_exec.py compares the library with this restatement, so a mistake in the restatement would show here and not hide there."""
    got = {name: ec.verify_block(txs, c) for name, txs, c in ec.named_blocks(random.Random(44))}
    want = {"empty": 1, "no_blob_txs": 1, "spread": 1, "zero_hash_tx": 1, "minimal_offset": 1, "dynamic_data": 1, "count+1": 5, "count-1": 5,
            "hashes_without_commitments": 5, "wrong_hash_first": 4, "wrong_hash_middle": 4, "wrong_hash_last": 4, "raw_digest": 4, "too_short": 6,
            "offset_out_of_bounds": 7, "trailing": 8, "empty_tx": 6, "two_malformations_7_then_6": 7, "two_malformations_8_then_7": 8,
            "malformed+count+hash": 6, "count+hash": 5}
    assert got == want


def test_python_signature_table_resolves_the_new_symbols():
    import gokzg_amd
    if not os.path.exists(gokzg_amd.LIB_PATH):
        pytest.skip("libkzg_hip.so is not built")
    L = gokzg_amd.lib()
    for name, nargs in (("kzg_hip_eth_kzg_to_versioned_hash_batch", 4), ("kzg_hip_eth_kzg_to_versioned_hash_batch_dev", 4),
                        ("kzg_hip_eth_point_evaluation_precompile_batch", 4), ("kzg_hip_eth_point_evaluation_precompile_batch_dev", 4),
                        ("kzg_hip_eth_precompile_return_value", 2), ("kzg_hip_eth_verify_kzg_commitments_against_transactions_batch", 8)):
        assert len(getattr(L, name).argtypes) == nargs, name
    for method in ("kzg_to_versioned_hash_batch", "point_evaluation_precompile_batch", "precompile_return_value",
                   "verify_kzg_commitments_against_transactions_batch"):
        assert hasattr(gokzg_amd.EthSettings, method), method
