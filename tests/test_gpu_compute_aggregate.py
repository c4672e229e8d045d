"""eth.ComputeAggregateKZGProof over many sidecars in one device call (kzg_hip_eth_compute_aggregate_kzg_proof_batch[_dev]: capi_eth_prove.hip, the
two-halves transcript kernels of k_eth_aggregate.hip) on a small handle (n = 64, secret known).  The rule of the call: proof and commitments
of a good row are byte for byte what compute_aggregate_kzg_proof returns for that sidecar alone.  Ragged counts against the lone call and the
Python reference, lane and workgroup edges of the transcript kernels (outputs fed to the batch verifier), crafted rows between valid
neighbours, the transcript paths and the chunk loop in child processes, the device-buffer form, the golden n = 4096 setup, misuse and
concurrent callers.

Run as a script (`python test_gpu_compute_aggregate.py child COUNTS OUT.npz`) it is the child of the transcript-path and chunk tests: the same
deterministic sidecars through one call; proofs, commitments, status and the number of chunks saved."""
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

N = 64
R = ko.R_MOD
ZERO_PROOF = np.frombuffer(er.ZERO_PROOF, dtype=np.uint8)
RAGGED6 = [3, 0, 1, 2, 5, 1]
CHUNK_COUNTS = [2, 2, 5, 0, 1]
# what [2, 2] costs (twice the bytes of four n = 64 blobs plus two rows for each of the two sidecars): the budget that holds four blobs
CHUNK_BUDGET_BYTES = 2 * 4 * N * 32 + 2 * 2 * N * 32
CHUNK_BUDGET_MB = "0.0235"


def le32(v):
    return np.frombuffer(int(v).to_bytes(32, "little"), dtype=np.uint8)


def small_handle(kz, with_g2=False):
    """as tests/test_gpu_verify_aggregate.py::small_handle builds it"""
    fs = kz.FFTSettings(6)
    eth = kz.EthSettings(fs, er.lagrange_setup(N, er.S_TEST))
    if with_g2:
        eth.set_setup_g2(np.stack([vi.g2_kilic(pr.G2_GEN), vi.g2_kilic(pr.g2_mul(pr.G2_GEN, er.S_TEST % pr.R))]))
    return fs, eth


def random_blobs(seed, count, n=N):
    rng = np.random.default_rng(seed)
    vals = [int.from_bytes(rng.bytes(32), "little") % R for _ in range(count * n)]
    return np.frombuffer(b"".join(v.to_bytes(32, "little") for v in vals), dtype=np.uint8).reshape(count, n, 32).copy()


def offsets(counts):
    return np.concatenate([[0], np.cumsum(counts)]).astype(int)


def lone_calls(kz, eth, blobs, counts):
    """[(status, proof, commitments)] of compute_aggregate_kzg_proof per sidecar; a refused sidecar has zero bytes"""
    at, out = offsets(counts), []
    for j, c in enumerate(counts):
        try:
            proof, comm = eth.compute_aggregate_kzg_proof(blobs[at[j]:at[j + 1]])
            out.append((0, proof, comm))
        except kz.KzgError as e:
            out.append((e.status, np.zeros(48, np.uint8), np.zeros((c, 48), np.uint8)))
    return out


def assert_rows_match(got, want, counts):
    proofs, comm, status = got
    at = offsets(counts)
    assert proofs.shape == (len(counts), 48) and comm.shape == (at[-1], 48) and status.shape == (len(counts),)
    for j, (st, proof, c) in enumerate(want):
        assert status[j] == st, (j, status[j], st)
        assert np.array_equal(proofs[j], proof), j
        assert np.array_equal(comm[at[j]:at[j + 1]], c), j


def run_child(counts, out):
    """the deterministic sidecars of `counts` (an element >= r in the last sidecar that has a blob) through one call"""
    import gokzg_amd as kz
    fs, eth = small_handle(kz)
    blobs = random_blobs(77, sum(counts))
    blobs[-1, 5] = le32(R)
    proofs, comm, status = eth.compute_aggregate_kzg_proof_batch(blobs, counts)
    np.savez(out, proofs=proofs, comm=comm, status=status, chunks=np.array([kz.lib().kzg_hip_test_eth_prove_chunks()]))
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
    fs, eth = small_handle(kz, with_g2=True)
    yield fs, eth
    eth.close(); fs.close()


@pytest.fixture(scope="module")
def honest(kz, handle):
    """129 sidecars with counts cycling 0..3 and the lone call's outputs for each: computed once, never changed"""
    _, eth = handle
    counts = [j % 4 for j in range(129)]
    blobs = random_blobs(5, sum(counts))
    return blobs, counts, lone_calls(kz, eth, blobs, counts)


def test_ragged_counts_match_the_lone_call_and_the_reference(kz, handle, monkeypatch):
    """counts [3, 0, 1, 2, 5, 1]: proofs, commitments and status bit for bit those of the lone call per sidecar, and those of the Python
    reference: the transcript and the aggregated polynomial from oracle/pyref.py, the proof as the known multiple of the generator
    (tests/eth_rows.py: the secret is known).  A sidecar without blobs gets the compressed point at infinity."""
    _, eth = handle
    blobs = random_blobs(3, sum(RAGGED6))
    lone = lone_calls(kz, eth, blobs, RAGGED6)
    for mode in ("host", "device"):                                                # (six sidecars go to the host's hash by default)
        monkeypatch.setenv("KZG_HIP_ETH_TRANSCRIPT", mode)
        got = eth.compute_aggregate_kzg_proof_batch(blobs, RAGGED6)
        assert_rows_match(got, lone, RAGGED6)
    proofs, comm, status = got
    assert list(status) == [0] * 6 and np.array_equal(proofs[1], ZERO_PROOF)
    at, ref = offsets(RAGGED6), er.Reference(N, er.S_TEST)
    for j in range(6):
        polys = [[int.from_bytes(e.tobytes(), "little") for e in blob] for blob in blobs[at[j]:at[j + 1]]]
        powers, z = pyref.compute_challenges(polys, [row.tobytes() for row in comm[at[j]:at[j + 1]]], field_elements_per_blob=N)
        agg, powers2, z2 = pyref.compute_aggregated_poly(polys, [row.tobytes() for row in comm[at[j]:at[j + 1]]], field_elements_per_blob=N)
        assert (powers, z) == (powers2, z2)
        ok, _, want = ref.expected(tuple(agg), z)
        assert ok and proofs[j].tobytes() == want, j


@pytest.mark.parametrize("sidecars", [65, 129])
def test_lane_and_workgroup_edges(kz, handle, honest, sidecars, monkeypatch):
    """65 and 129 sidecars with counts cycling 0..3: one wavefront of the transcript kernels plus one lane, two workgroups plus one.  Every row
    against the lone call; the outputs then pass the batch verifier"""
    _, eth = handle
    blobs, counts, want = honest
    nb = int(sum(counts[:sidecars]))
    monkeypatch.setenv("KZG_HIP_ETH_TRANSCRIPT", "device")                         # (below the default threshold the host would hash)
    got = eth.compute_aggregate_kzg_proof_batch(blobs[:nb], counts[:sidecars])
    assert_rows_match(got, want[:sidecars], counts[:sidecars])
    proofs, comm, status = got
    assert not status.any()
    assert list(eth.verify_aggregate_kzg_proof_batch(blobs[:nb], counts[:sidecars], comm, proofs)) == [1] * sidecars


def test_crafted_rows_between_valid_neighbours(kz, handle):
    """one element equal to r in the first blob, in the last blob, and in the last 32 bytes of a sidecar (the bytes the finish kernel reads
    again): the row reports ERR_BAD_BLOB with zero bytes, as the lone call refuses it, and its neighbours are those of the lone call.
    The other row status, ERR_BAD_ARG for an evaluation challenge inside the domain, cannot be provoked: the challenge is a SHA-256 output
    reduced mod r, and no input is known that hashes onto one of the n roots of unity."""
    _, eth = handle
    counts = [2] * 9
    blobs = random_blobs(9, sum(counts))
    blobs[2 * 2 + 0, 5] = le32(R)            # sidecar 2: its first blob
    blobs[2 * 4 + 1, 17] = le32(R)           # sidecar 4: its last blob
    blobs[2 * 6 + 1, N - 1] = le32(R)        # sidecar 6: its last 32 bytes
    want = lone_calls(kz, eth, blobs, counts)
    assert [w[0] for w in want] == [0, 0, kz.ERR_BAD_BLOB, 0, kz.ERR_BAD_BLOB, 0, kz.ERR_BAD_BLOB, 0, 0]
    got = eth.compute_aggregate_kzg_proof_batch(blobs, counts)
    assert_rows_match(got, want, counts)
    proofs, comm, _ = got
    for j in (2, 4, 6):
        assert not proofs[j].any() and not comm[2 * j:2 * j + 2].any()
    clean = random_blobs(9, sum(counts))
    proofs0, comm0, status0 = eth.compute_aggregate_kzg_proof_batch(clean, counts)
    assert not status0.any()
    for j in (0, 1, 3, 5, 7, 8):                                                   # the neighbours are what they are without the crafted rows
        assert np.array_equal(proofs[j], proofs0[j]) and np.array_equal(comm[2 * j:2 * j + 2], comm0[2 * j:2 * j + 2]), j


def test_transcript_paths_return_identical_bytes(kz, tmp_path):
    """KZG_HIP_ETH_TRANSCRIPT=host and =device in child processes, the device path with and without the second stream: byte for byte"""
    host = child(tmp_path, "host", RAGGED6, KZG_HIP_ETH_TRANSCRIPT="host")
    assert list(host["status"]) == [0, 0, 0, 0, 0, kz.ERR_BAD_BLOB]
    assert host["proofs"][:5].any(axis=1).all() and not host["proofs"][5].any()
    for name, env in (("device", {}), ("device_one_stream", {"KZG_HIP_ETH_PROVE_OVERLAP": "0"})):
        dev = child(tmp_path, name, RAGGED6, KZG_HIP_ETH_TRANSCRIPT="device", **env)
        for k in ("proofs", "comm", "status"):
            assert np.array_equal(host[k], dev[k]), (name, k)


def test_chunks_of_whole_sidecars(tmp_path):
    """a budget of four n = 64 blobs: counts [2, 2, 5, 0, 1] run as [2, 2] | [5] (a chunk by itself) | [0, 1] -- three chunks -- and return the
    bytes of the one-chunk call of another process"""
    assert CHUNK_BUDGET_BYTES <= int(float(CHUNK_BUDGET_MB) * 2**20) < CHUNK_BUDGET_BYTES + 2 * N * 32
    whole = child(tmp_path, "whole", CHUNK_COUNTS)
    assert list(whole["chunks"]) == [1]
    for mode in ("host", "device"):
        cut = child(tmp_path, "cut_" + mode, CHUNK_COUNTS, KZG_HIP_ETH_PROVE_CHUNK_MB=CHUNK_BUDGET_MB, KZG_HIP_ETH_TRANSCRIPT=mode)
        assert list(cut["chunks"]) == [3], mode
        for k in ("proofs", "comm", "status"):
            assert np.array_equal(cut[k], whole[k]), (mode, k)


def test_device_buffer_form(kz, handle, honest):
    """the _dev form on device-resident buffers: the bytes of the host-buffer form"""
    import torch
    _, eth = handle
    blobs, counts, want = honest
    counts = counts[:70]
    nb = int(sum(counts))
    d_blobs = torch.from_numpy(blobs[:nb]).to("cuda:0")
    d_proofs = torch.full((70, 48), 0xAA, dtype=torch.uint8, device="cuda:0")
    d_comm = torch.full((nb, 48), 0xAA, dtype=torch.uint8, device="cuda:0")
    d_status = torch.full((70,), 0xAA, dtype=torch.uint8, device="cuda:0")
    torch.cuda.synchronize()
    eth.compute_aggregate_kzg_proof_batch_dev(d_blobs.data_ptr(), counts, d_proofs.data_ptr(), d_comm.data_ptr(), d_status.data_ptr())
    torch.cuda.synchronize()
    assert_rows_match((d_proofs.cpu().numpy(), d_comm.cpu().numpy(), d_status.cpu().numpy()), want[:70], counts)


def test_golden_setup_n4096(kz, monkeypatch):
    """the golden n = 4096 setup with the smallest commitment table the suite builds at that size: counts [2, 0, 1] against the lone call"""
    monkeypatch.setenv("KZG_HIP_FB_BUDGET_GB", "0.2")
    fs = kz.FFTSettings(12)
    eth = kz.EthSettings(fs, er.golden_lagrange_setup())
    ints = [ko.fr_to_ints(ko.synthetic_blob(1 + b)) for b in range(3)]
    blobs = np.stack([np.frombuffer(b"".join(v.to_bytes(32, "little") for v in bi), dtype=np.uint8).reshape(4096, 32) for bi in ints])
    counts = [2, 0, 1]
    got = eth.compute_aggregate_kzg_proof_batch(blobs, counts)
    want = lone_calls(kz, eth, blobs, counts)
    assert [w[0] for w in want] == [0, 0, 0]
    assert_rows_match(got, want, counts)
    eth.close(); fs.close()


def test_misuse(kz, handle):
    _, eth = handle
    blobs, counts = random_blobs(1, 1), np.array([1, 0], dtype=np.uint64)
    proofs, comm, status = np.full((2, 48), 7, np.uint8), np.full((1, 48), 7, np.uint8), np.full(2, 7, np.uint8)
    empty = eth.compute_aggregate_kzg_proof_batch(np.zeros((0, N, 32), np.uint8), [])
    assert [a.shape for a in empty] == [(0, 48), (0, 48), (0,)]
    p = lambda a: a.ctypes.data
    for f in (kz.lib().kzg_hip_eth_compute_aggregate_kzg_proof_batch, kz.lib().kzg_hip_eth_compute_aggregate_kzg_proof_batch_dev):
        assert f(eth.h, None, None, 0, None, None, None) == kz.OK                 # sidecars == 0 touches nothing
        assert f(eth.h, p(blobs), p(counts), 0, p(proofs), p(comm), p(status)) == kz.OK
        assert (proofs == 7).all() and (comm == 7).all() and (status == 7).all()
        for a in ([None, p(blobs), p(counts), p(proofs), p(status)], [eth.h, None, p(counts), p(proofs), p(status)], [eth.h, p(blobs), None, p(proofs), p(status)],
                  [eth.h, p(blobs), p(counts), None, p(status)], [eth.h, p(blobs), p(counts), p(proofs), None]):
            assert f(a[0], a[1], a[2], 2, a[3], p(comm), a[4]) == kz.ERR_BAD_ARG
        wide = np.array([2**63, 2**63], dtype=np.uint64)
        assert f(eth.h, p(blobs), p(wide), 2, p(proofs), p(comm), p(status)) == kz.ERR_TOO_WIDE
        wide = np.array([2**58, 0], dtype=np.uint64)                               # the sum fits, the byte offsets do not
        assert f(eth.h, p(blobs), p(wide), 2, p(proofs), p(comm), p(status)) == kz.ERR_TOO_WIDE
    assert (proofs == 7).all() and (comm == 7).all() and (status == 7).all()
    got = eth.compute_aggregate_kzg_proof_batch(blobs, counts)                     # commitments are optional
    assert kz.lib().kzg_hip_eth_compute_aggregate_kzg_proof_batch(eth.h, p(blobs), p(counts), 2, p(proofs), None, p(status)) == kz.OK
    assert np.array_equal(proofs, got[0]) and not status.any()


def test_concurrent_calls_on_one_handle(kz, handle, honest):
    """eight threads call the batch prover on one handle while another makes lone calls: every result is the lone call's"""
    _, eth = handle
    blobs, counts, want = honest
    counts = counts[:40]
    nb = int(sum(counts))
    errors = []

    def batch():
        for _ in range(2):
            try:
                assert_rows_match(eth.compute_aggregate_kzg_proof_batch(blobs[:nb], counts), want[:40], counts)
            except Exception as e:                                                  # noqa: BLE001 (reported below)
                errors.append(repr(e))

    def lone():
        at = offsets(counts)
        for j in (3, 7, 11, 14):
            try:
                st, proof, comm = lone_calls(kz, eth, blobs[at[j]:at[j + 1]], [counts[j]])[0]
                assert st == 0 and np.array_equal(proof, want[j][1]) and np.array_equal(comm, want[j][2]), j
            except Exception as e:                                                  # noqa: BLE001
                errors.append(repr(e))

    threads = [threading.Thread(target=batch) for _ in range(8)] + [threading.Thread(target=lone)]
    for t in threads:
        t.start()
    for t in threads:
        t.join()
    assert not errors, errors
