"""eth.VerifyAggregateKZGProof over many sidecars in one device call (kzg_hip_eth_verify_aggregate_kzg_proof_batch: k_eth_aggregate.hip,
capi_verify.hip) on a small handle (n = 64, secret known): the lanes hooks of the transcript's SHA-256 and reduction, ragged blob counts across
a wavefront and a workgroup against the one-sidecar call and the Python reference, crafted rows between valid neighbours, the two transcript
paths and the chunk loop in child processes, the golden n = 4096 setup, misuse and concurrent callers.

Run as a script (`python test_gpu_verify_aggregate.py child COUNTS OUT.npz`) it is the child of the transcript-path and chunk tests: the
same deterministic sidecars through one call, results and intermediates saved."""
import hashlib
import json
import os
import subprocess
import sys
import threading

import numpy as np
import pytest

HERE = os.path.dirname(os.path.abspath(__file__))
ROOT = os.path.dirname(HERE)
if __name__ == "__main__":
    sys.path[:0] = [ROOT, HERE]

import eth_rows as er  # noqa: E402
import pairing_ref as pr  # noqa: E402
import verify_images as vi  # noqa: E402
from oracle import koracle as ko, pyref  # noqa: E402

pytestmark = pytest.mark.gpu

GOLDEN = os.path.join(HERE, "golden")
N = 64
R = ko.R_MOD
ZERO_PROOF = np.frombuffer(er.ZERO_PROOF, dtype=np.uint8)
RAGGED8 = [0, 1, 2, 3, 5, 1, 0, 4]
CRAFTED_DIGESTS = [0, R - 1, R, 2 * R - 1, 2 * R, 2**256 - 1]


def le32(v):
    return np.frombuffer(int(v).to_bytes(32, "little"), dtype=np.uint8)


def small_handle(kz, with_g2=True):
    fs = kz.FFTSettings(6)
    eth = kz.EthSettings(fs, er.lagrange_setup(N, er.S_TEST))
    if with_g2:
        eth.set_setup_g2(small_g2())
    return fs, eth


def small_g2():
    return np.stack([vi.g2_kilic(pr.G2_GEN), vi.g2_kilic(pr.g2_mul(pr.G2_GEN, er.S_TEST % pr.R))])


def random_blobs(rng, count, n=N):
    vals = [int.from_bytes(rng.bytes(32), "little") % R for _ in range(count * n)]
    return np.frombuffer(b"".join(v.to_bytes(32, "little") for v in vals), dtype=np.uint8).reshape(count, n, 32).copy()


class Sidecars:
    """blobs, expected commitments and aggregated proofs of honest sidecars with the given blob counts (commitments from
    blob_to_kzg_commitment_batch, proofs from compute_aggregate_kzg_proof), as per-sidecar lists"""

    def __init__(self, eth, counts, seed, n=N, blobs=None):
        rng = np.random.default_rng(seed)
        self.n, total = n, sum(counts)
        flat = random_blobs(rng, total, n) if blobs is None else blobs
        comm, ok = eth.blob_to_kzg_commitment_batch(flat) if total else (np.zeros((0, 48), np.uint8), np.ones(0, bool))
        assert ok.all()
        at = np.concatenate([[0], np.cumsum(counts)]).astype(int)
        self.blobs = [flat[at[j]:at[j + 1]].copy() for j in range(len(counts))]
        self.comms = [comm[at[j]:at[j + 1]].copy() for j in range(len(counts))]
        self.proofs = [eth.compute_aggregate_kzg_proof(b)[0] for b in self.blobs]

    def args(self):
        counts = [b.shape[0] for b in self.blobs]
        blobs = np.concatenate(self.blobs) if sum(counts) else np.zeros((0, self.n, 32), np.uint8)
        comms = np.concatenate(self.comms) if sum(counts) else np.zeros((0, 48), np.uint8)
        return blobs, np.array(counts, dtype=np.uint64), comms, np.stack(self.proofs)


def run_child(counts, out):
    """the deterministic sidecars of `counts` (plus a swapped proof in row 1 and an element >= r in the last row) through one call"""
    import gokzg_amd as kz
    fs, eth = small_handle(kz)
    sc = Sidecars(eth, counts, seed=77)
    sc.proofs[1] = sc.proofs[2].copy()
    sc.blobs[-1][0, 5] = le32(R)
    res, c48, zs, ys = eth.verify_aggregate_kzg_proof_batch(*sc.args(), intermediates=True)
    np.savez(out, res=res, c48=c48, zs=zs, ys=ys)
    eth.close(); fs.close()


if __name__ == "__main__":
    assert sys.argv[1] == "child"
    run_child([int(c) for c in sys.argv[2].split(",")], sys.argv[3])
    sys.exit(0)


def child(tmp_path, name, counts, **env):
    out = str(tmp_path / (name + ".npz"))
    e = dict(os.environ, KZG_HIP_NO_TORCH_PRELOAD="1", **env)     # (the child never touches torch: it need not wait for its import)
    res = subprocess.run([sys.executable, os.path.abspath(__file__), "child", ",".join(str(c) for c in counts), out], env=e, capture_output=True, text=True, timeout=120)
    assert res.returncode == 0, res.stdout + res.stderr
    return dict(np.load(out))


@pytest.fixture(scope="module")
def kz():
    import gokzg_amd
    assert gokzg_amd.device_count() >= 1, "no gfx950 device: the HIP path is the only path"
    return gokzg_amd


@pytest.fixture(scope="module")
def handle(kz):
    fs, eth = small_handle(kz)
    yield fs, eth
    eth.close(); fs.close()


@pytest.fixture(scope="module")
def honest(handle):
    """257 honest sidecars with counts cycling 0..3 and the one-sidecar call's (compressed aggregated commitment, z, y) for each: computed once,
    never changed (the tests copy what they tamper with)"""
    fs, eth = handle
    sc = Sidecars(eth, [j % 4 for j in range(257)], seed=5)
    return sc, one_sidecar_reference(fs, eth, sc)


def one_sidecar_reference(fs, eth, sc):
    ref = []
    for b, c in zip(sc.blobs, sc.comms):
        _, cagg, z, y = eth.compute_aggregated_poly_and_commitment(b, c)
        ref.append((fs.to_compressed_g1(cagg[None])[0], z, y))
    return ref


def assert_matches_one_sidecar_call(got, ref):
    res, c48, zs, ys = got
    assert list(res) == [1] * len(ref)
    for j, (c, z, y) in enumerate(ref):
        assert np.array_equal(c48[j], c) and np.array_equal(zs[j], z) and np.array_equal(ys[j], y), j


def test_sha256_lanes_hook(kz, handle):
    """130 messages in ONE launch (two wavefronts and a tail), the padding boundaries and random lengths up to 70 000 mixed within a wavefront:
    the chains end per lane; lengths 56..63 and 120..127 take the two-block ending, which no transcript reaches"""
    fs, _ = handle
    rng = np.random.default_rng(21)
    edge = [0, 1, 55, 56, 63, 64, 65, 119, 120, 127, 128]
    lens = [edge[i // 2 % len(edge)] if i % 2 == 0 else int(rng.integers(0, 70001)) for i in range(130)]
    lens[64], lens[129] = 70000, 56
    msgs = [rng.bytes(n) for n in lens]
    offsets = np.concatenate([[0], np.cumsum(lens)[:-1]]).astype(np.uint64)
    data = np.frombuffer(b"".join(msgs) or b"\0", dtype=np.uint8).copy()
    out = np.zeros((130, 32), dtype=np.uint8)
    L, p = kz.lib(), lambda a: a.ctypes.data
    assert L.kzg_hip_test_sha256_lanes(fs.h, p(data), p(offsets), p(np.array(lens, dtype=np.uint64)), 130, p(out)) == kz.OK
    for i, m in enumerate(msgs):
        assert out[i].tobytes() == hashlib.sha256(m).digest(), (i, lens[i])


def test_hash_to_bls_field_lanes_hook(kz, handle):
    """hashToBLSField's reduction on 0, r - 1, r, 2r - 1, 2r and 2^256 - 1 (no SHA output hits them), among ordinary digests"""
    fs, _ = handle
    rng = np.random.default_rng(22)
    vals = CRAFTED_DIGESTS + [int.from_bytes(rng.bytes(32), "little") for _ in range(70)]
    digests = np.stack([le32(v) for v in vals])
    out = ko.fr_empty(len(vals))
    assert kz.lib().kzg_hip_test_hash_to_bls_field_lanes(fs.h, digests.ctypes.data, len(vals), out.ctypes.data) == kz.OK
    assert ko.fr_to_ints(out) == [v % R for v in vals]


def test_ragged_counts_match_the_one_sidecar_call_and_the_reference(handle):
    """counts [0, 1, 2, 3, 5, 1, 0, 4]: every sidecar valid; z, y and the compressed aggregated commitment bit for bit those of
    compute_aggregated_poly_and_commitment, and those of the Python reference (transcript, PolyLinComb, barycentric evaluation, oracle MSM)"""
    fs, eth = handle
    sc = Sidecars(eth, RAGGED8, seed=3)
    got = eth.verify_aggregate_kzg_proof_batch(*sc.args(), intermediates=True)
    assert_matches_one_sidecar_call(got, one_sidecar_reference(fs, eth, sc))
    _, c48, zs, ys = got
    for j, (b, c) in enumerate(zip(sc.blobs, sc.comms)):
        polys = [[int.from_bytes(e.tobytes(), "little") for e in blob] for blob in b]
        agg, powers, z = pyref.compute_aggregated_poly(polys, [row.tobytes() for row in c], field_elements_per_blob=N)
        y = pyref.eval_in_evaluation_form(agg, z, er.domain(N))
        assert ko.fr_to_ints(zs[j:j + 1]) == [z] and ko.fr_to_ints(ys[j:j + 1]) == [y], j
        want = ko.g1_compress(ko.lincomb_g1(ko.g1_decompress(c.reshape(-1)), ko.fr_from_ints(powers)))[0] if len(polys) else ZERO_PROOF
        assert np.array_equal(c48[j], want), j


@pytest.mark.parametrize("sidecars", [65, 257])
def test_ragged_counts_across_a_wavefront_and_a_workgroup(handle, honest, sidecars):
    """65 and 257 sidecars with counts cycling 0..3: the lane-per-sidecar kernels cross a wavefront / a workgroup"""
    _, eth = handle
    sc, ref = honest
    blobs, counts, comms, proofs = sc.args()
    nb = int(counts[:sidecars].sum())
    got = eth.verify_aggregate_kzg_proof_batch(blobs[:nb], counts[:sidecars], comms[:nb], proofs[:sidecars], intermediates=True)
    assert_matches_one_sidecar_call(got, ref[:sidecars])
    assert list(eth.verify_aggregate_kzg_proof_batch(blobs[:nb], counts[:sidecars], comms[:nb], proofs[:sidecars])) == [1] * sidecars


def test_crafted_rows_between_valid_neighbours(handle):
    fs, eth = handle
    counts = [2] * 21
    counts[7] = counts[8] = 0
    sc = Sidecars(eth, counts, seed=9)
    want = [1] * 21
    sc.proofs[1] = sc.proofs[2].copy(); want[1] = 0                               # another sidecar's proof
    sc.blobs[3][1, 17, 0] ^= 1; want[3] = 0                                        # one blob byte changed (the low byte: still < r)
    assert int.from_bytes(sc.blobs[3][1, 17].tobytes(), "little") < R
    sc.comms[5] = sc.comms[5][::-1].copy(); want[5] = 0                            # the block's two commitments swapped
    assert not np.array_equal(sc.comms[5][0], sc.comms[5][1])
    assert np.array_equal(sc.proofs[7], ZERO_PROOF)                                # no blobs: the proof is the point at infinity ...
    sc.proofs[8] = sc.proofs[9].copy(); want[8] = 0                                # ... and any other valid proof fails
    const = np.stack([np.tile(le32(12345), (N, 1)), np.tile(le32(R - 2), (N, 1))])  # constant polynomials: a zero quotient
    c10 = Sidecars(eth, [2], seed=0, blobs=const)
    sc.blobs[10], sc.comms[10], sc.proofs[10] = c10.blobs[0], c10.comms[0], c10.proofs[0]
    assert np.array_equal(sc.proofs[10], ZERO_PROOF)
    sc.blobs[12][1, N - 1] = le32(R); want[12] = 2                                 # an element equal to r in the LAST blob of one block
    sc.blobs[13][0, 0] = le32(R); want[13] = 2                                     # ... and in the FIRST blob of the next
    order3 = np.zeros(48, dtype=np.uint8); order3[0] = 0x80                       # x = 0: (0, +-2) is on the curve, of order 3
    sc.comms[15][1] = order3; want[15] = 3
    sc.proofs[17] = np.zeros(48, dtype=np.uint8); want[17] = 3                     # no compression flag: undecodable
    sc.blobs[19][0, 3] = le32(2**256 - 1); sc.comms[19][0] = order3; sc.proofs[19] = np.zeros(48, dtype=np.uint8); want[19] = 2   # both faults: 2 wins
    got = eth.verify_aggregate_kzg_proof_batch(*sc.args())
    assert list(got) == want
    # the crafted rows alone (no neighbours), one call each
    for j in (1, 7, 8, 10, 12, 15, 17, 19):
        one = eth.verify_aggregate_kzg_proof_batch(sc.blobs[j], [sc.blobs[j].shape[0]], sc.comms[j], sc.proofs[j][None])
        assert list(one) == [want[j]], j


def test_transcript_paths_return_identical_bytes(tmp_path):
    """KZG_HIP_ETH_TRANSCRIPT=host and =device in child processes: results and intermediates byte for byte"""
    host = child(tmp_path, "host", RAGGED8, KZG_HIP_ETH_TRANSCRIPT="host")
    dev = child(tmp_path, "device", RAGGED8, KZG_HIP_ETH_TRANSCRIPT="device")
    assert list(host["res"]) == [1, 0, 1, 1, 1, 1, 1, 2] == list(dev["res"])
    for k in ("c48", "zs", "ys"):
        assert np.array_equal(host[k][:7], dev[k][:7]), k                          # (row 7 has result 2: its intermediates are unspecified)


def test_chunks_of_whole_sidecars(tmp_path):
    """a budget of four n = 64 blobs: counts [2, 2, 5, 0, 1] run as [2, 2] | [5] (larger than the budget, a chunk by itself) | [0, 1]; the same
    bytes as the unchunked call of another process"""
    counts = [2, 2, 5, 0, 1]
    assert 4 * N * 32 <= int(0.008 * 2**20) < 5 * N * 32
    whole = child(tmp_path, "whole", counts)
    for mode in ("host", "device"):
        cut = child(tmp_path, "cut_" + mode, counts, KZG_HIP_ETH_VERIFY_CHUNK_MB="0.008", KZG_HIP_ETH_TRANSCRIPT=mode)
        assert list(cut["res"]) == [1, 0, 1, 1, 2] == list(whole["res"]), mode
        for k in ("c48", "zs", "ys"):
            assert np.array_equal(cut[k][:4], whole[k][:4]), (mode, k)


def test_golden_setup_n4096(kz):
    """the golden setup (s = 1337, tests/golden/trusted_setup_g2.json): three sidecars of 2, 1 and 0 blobs; then one proof exchanged"""
    fx = json.load(open(os.path.join(GOLDEN, "trusted_setup_g2.json")))
    fs = kz.FFTSettings(12)
    eth = kz.EthSettings(fs, er.golden_lagrange_setup())
    eth.set_setup_g2(fs.g2_from_compressed(np.frombuffer(b"".join(bytes.fromhex(h) for h in fx["setup_G2"]), dtype=np.uint8)))
    ints = [ko.fr_to_ints(ko.synthetic_blob(1 + b)) for b in range(3)]
    blobs = np.stack([np.frombuffer(b"".join(v.to_bytes(32, "little") for v in bi), dtype=np.uint8).reshape(4096, 32) for bi in ints])
    sc = Sidecars(eth, [2, 1, 0], seed=0, n=4096, blobs=blobs)
    assert list(eth.verify_aggregate_kzg_proof_batch(*sc.args())) == [1, 1, 1]
    sc.proofs[0], sc.proofs[1] = sc.proofs[1], sc.proofs[0]
    assert list(eth.verify_aggregate_kzg_proof_batch(*sc.args())) == [0, 0, 1]
    eth.close(); fs.close()


def test_misuse(kz, handle):
    _, eth_ok = handle
    fs, eth = small_handle(kz, with_g2=False)
    sc = Sidecars(eth, [1, 0], seed=1)
    with pytest.raises(kz.KzgError) as e:                                          # before the setter (even for no sidecar at all)
        eth.verify_aggregate_kzg_proof_batch(*sc.args())
    assert e.value.status == kz.ERR_BAD_ARG
    eth.set_setup_g2(small_g2())
    assert list(eth.verify_aggregate_kzg_proof_batch(*sc.args())) == [1, 1]
    eth.close(); fs.close()
    empty = eth_ok.verify_aggregate_kzg_proof_batch(np.zeros((0, N, 32), np.uint8), [], np.zeros((0, 48), np.uint8), np.zeros((0, 48), np.uint8))
    assert len(empty) == 0
    blobs, counts, comms, proofs = sc.args()
    res = np.zeros(2, dtype=np.uint8)
    f, p = kz.lib().kzg_hip_eth_verify_aggregate_kzg_proof_batch, lambda a: a.ctypes.data
    assert f(eth_ok.h, None, None, None, None, 0, None, None, None, None) == kz.OK    # sidecars == 0
    for a in ([None, p(blobs), p(counts), p(comms), p(proofs), p(res)], [eth_ok.h, None, p(counts), p(comms), p(proofs), p(res)],
              [eth_ok.h, p(blobs), None, p(comms), p(proofs), p(res)], [eth_ok.h, p(blobs), p(counts), None, p(proofs), p(res)],
              [eth_ok.h, p(blobs), p(counts), p(comms), None, p(res)], [eth_ok.h, p(blobs), p(counts), p(comms), p(proofs), None]):
        assert f(a[0], a[1], a[2], a[3], a[4], 2, a[5], None, None, None) == kz.ERR_BAD_ARG
    wide = np.array([2**63, 2**63], dtype=np.uint64)
    assert f(eth_ok.h, p(blobs), p(wide), p(comms), p(proofs), 2, p(res), None, None, None) == kz.ERR_TOO_WIDE


def test_concurrent_calls_and_a_setter_on_one_handle(handle, honest):
    """two threads verify on one handle while a third hands it the same G2 points again: every call holds its own reference to the state"""
    _, eth = handle
    sc, _ = honest
    blobs, counts, comms, proofs = sc.args()
    nb = int(counts[:40].sum())
    bad = proofs[:40].copy()
    bad[6] = proofs[7]
    want = [1] * 40
    want[6] = 0
    errors, g2 = [], small_g2()

    def verify():
        for _ in range(3):
            got = list(eth.verify_aggregate_kzg_proof_batch(blobs[:nb], counts[:40], comms[:nb], bad))
            if got != want:
                errors.append(got)

    def setter():
        for _ in range(4):
            eth.set_setup_g2(g2)

    threads = [threading.Thread(target=verify), threading.Thread(target=verify), threading.Thread(target=setter)]
    for t in threads:
        t.start()
    for t in threads:
        t.join()
    assert not errors, errors
