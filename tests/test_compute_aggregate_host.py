"""The lane bodies of the batched block prover (go-kzg_amd/csrc/sha256_lane.hpp, eth_aggregate.hpp) compiled for the host
(tests/host/aggregate_prove_emul.cpp): the resumable SHA-256 against hashlib with the chain cut at every block boundary, and a sidecar's
transcript hashed in two halves against the one-piece lane body, hashlib and oracle/pyref.py.  The program is a plain executable with its own
main (never loaded into Python), built a second time with AddressSanitizer and UndefinedBehaviorSanitizer: the lane bodies index raw bytes.
CPU only."""
import hashlib
import os
import subprocess

import numpy as np
import pytest

from oracle import koracle as ko, pyref

HERE = os.path.dirname(os.path.abspath(__file__))
ROOT = os.path.dirname(HERE)
SRC = os.path.join(HERE, "host", "aggregate_prove_emul.cpp")
BUILDS = [("aggregate_prove_emul", ["-O2"]), ("aggregate_prove_emul_san", ["-O1", "-g", "-fsanitize=address,undefined", "-fno-sanitize-recover=all"])]
R = ko.R_MOD


@pytest.fixture(scope="module", params=BUILDS, ids=[b[0] for b in BUILDS])
def emul(request):
    name, flags = request.param
    bdir = os.path.join(HERE, "host", "_build")
    os.makedirs(bdir, exist_ok=True)
    exe = os.path.join(bdir, name)
    subprocess.check_call(["g++", "-std=c++17", "-Wall", "-Wextra", "-Werror", "-Wno-unknown-pragmas", *flags, "-I", os.path.join(ROOT, "go-kzg_amd", "csrc"), SRC, "-o", exe])

    def run(tmp_path, data, *args):
        path = str(tmp_path / "input.bin")
        with open(path, "wb") as f:
            f.write(data)
        res = subprocess.run([exe, *[str(a) for a in args], path], capture_output=True, text=True, timeout=60)
        assert res.returncode == 0 and not res.stderr, res.stdout + res.stderr
        return [line.split() for line in res.stdout.splitlines()]
    return run


def fr_int(words_hex):
    """eight 32-bit limbs, least significant first, of a Montgomery image -> the integer it stands for"""
    limbs = [int(words_hex[8 * i:8 * i + 8], 16) for i in range(8)]
    image = np.array([[limbs[2 * i] | limbs[2 * i + 1] << 32 for i in range(4)]], dtype=np.uint64)
    return ko.fr_to_ints(image)[0]


@pytest.mark.parametrize("length", [0, 55, 56, 63, 64, 65, 119, 120, 128])
def test_resumable_sha256_at_every_block_boundary(emul, tmp_path, length):
    """the padding boundaries (one- and two-block endings) with the chain cut after 0 .. length // 64 whole blocks: always hashlib's digest"""
    data = np.random.default_rng(100 + length).bytes(length)
    lines = emul(tmp_path, data, "resume")
    assert [int(l[0]) for l in lines] == list(range(length // 64 + 1))
    for first, digest in lines:
        assert digest == hashlib.sha256(data).hexdigest(), (length, first)


@pytest.mark.parametrize("n", [2, 4, 64])
@pytest.mark.parametrize("count", [0, 1, 2, 5])
def test_transcript_in_two_halves(emul, tmp_path, n, count):
    """the blob half, then the finish half: the challenges of eth_transcript_lane on the same bytes, of hashlib over the message built here
    and of pyref.hash_to_bls_field with the two tags; the state between the halves is SHA-256's state after the header and all blob bytes
    but the last 32 (finished with an empty tail it is hashlib's digest of that prefix)"""
    rng = np.random.default_rng(1000 * n + count)
    blobs, comms = rng.bytes(count * n * 32), rng.bytes(count * 48)
    out = {l[0]: l[1:] for l in emul(tmp_path, blobs + comms, "transcript", n, count)}
    message = b"FSBLOBVERIFY_V1_" + n.to_bytes(8, "little") + count.to_bytes(8, "little") + blobs + comms
    prefix = message[:32 * count * n] if count else b""
    assert len(prefix) % 64 == 0 and len(message) - len(prefix) == (48 * count + 32 if count else 32)
    assert out["prefix"] == [hashlib.sha256(prefix).hexdigest()]
    if not count:
        assert out["state"] == ["6a09e667bb67ae853c6ef372a54ff53a510e527f9b05688c1f83d9ab5be0cd19"]       # FIPS 180-4, 5.3.3
    digest = hashlib.sha256(message).digest()
    want = [pyref.hash_to_bls_field(digest + bytes([tag])) for tag in (0, 1)]
    assert want == [int.from_bytes(hashlib.sha256(digest + bytes([tag])).digest(), "little") % R for tag in (0, 1)]
    assert [fr_int(w) for w in out["halves"]] == want
    assert out["halves"] == out["whole"]


def test_python_signature_table_resolves_the_new_symbols():
    import gokzg_amd
    L = gokzg_amd.lib()
    for name in ("kzg_hip_eth_compute_aggregate_kzg_proof_batch", "kzg_hip_eth_compute_aggregate_kzg_proof_batch_dev"):
        assert len(getattr(L, name).argtypes) == 7, name
    assert L.kzg_hip_test_eth_prove_chunks() == 0                                      # no call yet on this thread
    assert hasattr(gokzg_amd.EthSettings, "compute_aggregate_kzg_proof_batch")
