"""The execution-layer side of eth/eth.go in batches on the device (k_eth_exec.hip, capi_eth_exec.hip): KZGToVersionedHash against hashlib,
PointEvaluationPrecompile on the crafted rows of tests/verify_images.py (fixture setup, s = 1337) and on the golden n = 4096 setup, and
VerifyKZGCommitmentsAgainstTransactions on the blocks of tests/eth_exec_cases.py.  Expected codes come from the rows' own truth values, from
hashlib and from the Python restatement; nothing here asks the library what the right answer is."""
import hashlib
import os
import random
import re
import threading

import numpy as np
import pytest

import eth_exec_cases as ec
import verify_images as vi
from oracle import koracle as ko

pytestmark = pytest.mark.gpu

HERE = os.path.dirname(os.path.abspath(__file__))
ROOT = os.path.dirname(HERE)
GOLDEN = os.path.join(HERE, "golden")
PAIRING_BLOCK = int(re.search(r"#define\s+PAIRING_BLOCK\s+(\d+)", open(os.path.join(ROOT, "go-kzg_amd", "csrc", "k_pairing.hip")).read()).group(1))


@pytest.fixture(scope="module")
def kz():
    import gokzg_amd
    assert gokzg_amd.device_count() >= 1, "no gfx950 device: the HIP path is the only path"
    return gokzg_amd


def fixture_g2_points():
    """tests/golden/trusted_setup_g2.json holds [1337^i] G2: (encodings, reference points)"""
    import json
    import pairing_ref as pr
    fx = json.load(open(os.path.join(GOLDEN, "trusted_setup_g2.json")))
    enc, pts, Q = [], [], pr.G2_GEN
    for h in fx["setup_G2"]:
        b = bytes.fromhex(h)
        assert b == pr.g2_compress(Q)
        enc.append(b); pts.append(Q)
        Q = pr.g2_mul(Q, 1337)
    return enc, pts


def lagrange_setup():
    return ko.g1_decompress(np.frombuffer(open(os.path.join(GOLDEN, "trusted_setup_g1_lagrange.bin"), "rb").read(), dtype=np.uint8))


@pytest.fixture(scope="module")
def eth_fixture(kz):   # the n = 4096 Lagrange setup with the fixture's G2 points [1337^i] G2
    enc, pts = fixture_g2_points()
    fs = kz.FFTSettings(12)
    eth = kz.EthSettings(fs, lagrange_setup())
    yield eth, pts
    eth.close(); fs.close()


# ---------------- KZGToVersionedHash ----------------
@pytest.fixture(scope="module")
def commitments_1000():
    rng = random.Random(51)
    c = [rng.randbytes(48) for _ in range(1000)]
    c[0], c[1], c[2] = bytes(48), b"\xff" * 48, bytes(vi.compress_scalar(1))
    return c, [b"\x01" + hashlib.sha256(x).digest()[1:] for x in c]


@pytest.mark.parametrize("count", [0, 1, 63, 64, 65, 1000])
def test_versioned_hashes(kz, eth_fixture, commitments_1000, count):
    """against hashlib; needs no G2 setup; the _dev form on device buffers gives the same bytes"""
    import torch
    eth, _ = eth_fixture
    c, want = commitments_1000
    arr = np.frombuffer(b"".join(c[:count]), dtype=np.uint8).reshape(count, 48)
    got = eth.kzg_to_versioned_hash_batch(arr)
    assert got.shape == (count, 32) and got.tobytes() == b"".join(want[:count])
    d_in = torch.from_numpy(arr.copy()).to("cuda:0") if count else torch.zeros(48, dtype=torch.uint8, device="cuda:0")
    d_out = torch.full((max(count, 1), 32), 0xAA, dtype=torch.uint8, device="cuda:0")
    torch.cuda.synchronize()
    eth.kzg_to_versioned_hash_batch_dev(d_in.data_ptr(), count, d_out.data_ptr())
    torch.cuda.synchronize()
    assert d_out.cpu().numpy()[:count].tobytes() == b"".join(want[:count])
    if not count:
        assert (d_out.cpu().numpy() == 0xAA).all()


# ---------------- PointEvaluationPrecompile: crafted rows on the fixture setup ----------------
def precompile_row(h, r):
    return bytes(h) + bytes(r[2]) + bytes(r[3]) + bytes(r[1]) + bytes(r[4])


@pytest.fixture(scope="module")
def crafted():
    """every row of verify_images.eth_rows(1337) behind its correct versioned hash: (rows, inputs, codes)"""
    rows = vi.eth_rows(1337, random.Random(4))
    inputs = [precompile_row(ec.versioned_hash(r[1]), r) for r in rows]
    want = [r[5] for r in rows]
    assert set(want) == {0, 1, 2, 3} and all(len(b) == 192 for b in inputs)
    return rows, inputs, want


def as_array(inputs):
    return np.frombuffer(b"".join(inputs), dtype=np.uint8).reshape(len(inputs), 192)


def test_precompile_crafted_rows(kz, eth_fixture, crafted):
    """the code of a row behind its right hash is the row's own (0, 1, 2 or 3) and what verify_kzg_proof_batch returns for the split fields;
    kzgSetupG2 as Z = 1 images, then as Jacobian images"""
    eth, pts = eth_fixture
    rows, inputs, want = crafted
    rng = random.Random(52)
    c48, zs, ys, pi48 = vi.eth_arrays(rows)
    for jac in (False, True):
        eth.set_setup_g2(np.stack([vi.g2_kilic(Q, vi.rand_fp2(rng) if jac else (1, 0)) for Q in pts]))
        got = eth.point_evaluation_precompile_batch(as_array(inputs))
        bad = [(r[0], int(g), w) for r, g, w in zip(rows, got, want) if int(g) != w]
        assert not bad, bad
        assert list(got) == list(eth.verify_kzg_proof_batch(c48, zs, ys, pi48))
    assert list(eth.point_evaluation_precompile_batch(inputs)) == want          # a list of byte strings


def spoilings(rows, k):
    """[(name, hash)] for row k: six ways in which the first 32 bytes are not the commitment's versioned hash"""
    c = bytes(rows[k][1])
    h = ec.versioned_hash(c)
    other = next(bytes(r[1]) for r in rows[k + 1:] + rows[:k] if bytes(r[1]) != c)
    out = [("version_0x00", b"\x00" + h[1:]), ("version_0x02", b"\x02" + h[1:]), ("bit_in_byte_1", h[:1] + bytes([h[1] ^ 0x08]) + h[2:]),
           ("bit_in_byte_31", h[:31] + bytes([h[31] ^ 0x80])), ("other_rows_commitment", ec.versioned_hash(other))]
    raw = hashlib.sha256(c).digest()
    if raw[0] != 0x01:
        out.append(("raw_digest", raw))
    return out


def test_precompile_spoiled_hashes(kz, eth_fixture, crafted):
    """every spoiling on rows whose own code is 1, 2 and 3 (and 0): all of them give 4, whatever else is wrong with the row"""
    eth, pts = eth_fixture
    rows, inputs, want = crafted
    eth.set_setup_g2(np.stack([vi.g2_kilic(Q) for Q in pts]))
    picked = [k for code in (1, 2, 3, 0) for k in [i for i, w in enumerate(want) if w == code][:3]]
    names, spoiled = [], []
    for k in picked:
        for name, h in spoilings(rows, k):
            names.append((rows[k][0], want[k], name))
            spoiled.append(precompile_row(h, rows[k]))
    for code in (1, 2, 3):
        assert {n[2] for n in names if n[1] == code} == {"version_0x00", "version_0x02", "bit_in_byte_1", "bit_in_byte_31", "other_rows_commitment", "raw_digest"}
    got = eth.point_evaluation_precompile_batch(as_array(spoiled))
    bad = [(n, int(g)) for n, g in zip(names, got) if int(g) != 4]
    assert not bad, bad
    # spoiled and unspoiled rows side by side in one call: each keeps its own code
    mixed = [spoiled[i // 2] if i % 2 else inputs[i // 2] for i in range(2 * min(len(spoiled), len(inputs)))]
    want_mixed = [4 if i % 2 else want[i // 2] for i in range(len(mixed))]
    assert list(eth.point_evaluation_precompile_batch(as_array(mixed))) == want_mixed


def test_precompile_byte_rows_alone_and_tiled(kz, eth_fixture, crafted):
    """each byte-level row as a call of its own, then the whole list tiled to PAIRING_BLOCK - 1, PAIRING_BLOCK, PAIRING_BLOCK + 1 and 65 rows
    from a different starting row each time: a lane that read its neighbour's row would return its neighbour's code"""
    eth, pts = eth_fixture
    rows, inputs, want = crafted
    eth.set_setup_g2(np.stack([vi.g2_kilic(Q) for Q in pts]))
    byte_rows = [i for i, r in enumerate(rows) if r[0].startswith("bytes/")]
    assert len(byte_rows) >= 15
    for i in byte_rows:
        assert list(eth.point_evaluation_precompile_batch(as_array(inputs[i:i + 1]))) == [want[i]], rows[i][0]
    n = len(inputs)
    first_byte_row = byte_rows[0]
    for size in sorted({PAIRING_BLOCK - 1, PAIRING_BLOCK, PAIRING_BLOCK + 1, 65}):
        shift = first_byte_row - 3 - size % 7                      # another start for every size; the byte-level rows (codes 2 and 3) lie inside every tile
        idx = [(shift + k) % n for k in range(size)]
        tile_want = [want[i] for i in idx]
        assert len(set(tile_want)) >= 3
        got = eth.point_evaluation_precompile_batch(as_array([inputs[i] for i in idx]))
        assert list(got) == tile_want, size


def test_precompile_wrong_length_in_the_binding(kz, eth_fixture, crafted):
    """a byte string that is not 192 bytes long gets the binding's code 9 and does not go to the device; its neighbours keep their codes"""
    eth, pts = eth_fixture
    rows, inputs, want = crafted
    eth.set_setup_g2(np.stack([vi.g2_kilic(Q) for Q in pts]))
    k = [i for i, w in enumerate(want) if w == 1][0]
    got = eth.point_evaluation_precompile_batch([inputs[k], inputs[k][:191], b"", inputs[k] + b"\x00", inputs[k]])
    assert list(got) == [1, 9, 9, 9, 1]
    assert list(eth.point_evaluation_precompile_batch([b"short"])) == [9]


# ---------------- PointEvaluationPrecompile on the golden n = 4096 setup ----------------
@pytest.fixture(scope="module")
def golden(kz):
    import json
    fx = json.load(open(os.path.join(GOLDEN, "trusted_setup_g2.json")))
    fs = kz.FFTSettings(12)
    g2 = fs.g2_from_compressed(np.frombuffer(b"".join(bytes.fromhex(h) for h in fx["setup_G2"]), dtype=np.uint8))
    eth = kz.EthSettings(fs, lagrange_setup())
    before = {}
    for name, arg in (("rows", np.zeros((1, 192), np.uint8)), ("empty", np.zeros((0, 192), np.uint8))):
        try:
            eth.point_evaluation_precompile_batch(arg)
            before[name] = None
        except kz.KzgError as e:
            before[name] = e.status
    before["hashes"] = eth.kzg_to_versioned_hash_batch(np.zeros((1, 48), np.uint8)).tobytes()      # needs no setup
    eth.set_setup_g2(g2)
    nb = 4
    blobs_i = [ko.fr_to_ints(ko.synthetic_blob(1 + b)) for b in range(nb)]
    blobs = np.stack([np.frombuffer(b"".join(v.to_bytes(32, "little") for v in bi), dtype=np.uint8).reshape(4096, 32) for bi in blobs_i])
    commits, ok = eth.blob_to_kzg_commitment_batch(blobs)
    assert ok.all()
    zs_i = [(0x1234567890abcdef * (b + 3)) % ko.R_MOD for b in range(nb)]
    proofs, ys, ok = eth.compute_kzg_proof_batch(np.stack([ko.fr_from_ints(bi) for bi in blobs_i]), ko.fr_from_ints(zs_i))
    assert ok.all()
    rows = [ec.versioned_hash(commits[b].tobytes()) + zs_i[b].to_bytes(32, "little") + y.to_bytes(32, "little") + commits[b].tobytes() + proofs[b].tobytes()
            for b, y in enumerate(ko.fr_to_ints(ys))]
    yield eth, rows, before
    eth.close(); fs.close()


def test_precompile_golden_setup(kz, golden):
    eth, rows, before = golden
    assert before["rows"] == kz.ERR_BAD_ARG and before["empty"] == kz.ERR_BAD_ARG               # before set_setup_g2 the call raises
    assert before["hashes"] == b"\x01" + hashlib.sha256(bytes(48)).digest()[1:]
    assert list(eth.point_evaluation_precompile_batch(as_array(rows))) == [1, 1, 1, 1]
    assert eth.precompile_return_value() == (4096).to_bytes(32, "big") + ko.R_MOD.to_bytes(32, "big")
    swapped = [rows[0][:144] + rows[1][144:]] + rows[1:]                                        # another valid proof
    assert list(eth.point_evaluation_precompile_batch(as_array(swapped))) == [0, 1, 1, 1]
    empty = eth.point_evaluation_precompile_batch(np.zeros((0, 192), np.uint8))
    assert empty.shape == (0,) and len(eth.point_evaluation_precompile_batch([])) == 0


def golden_mix(rows):
    """the four valid rows with a swapped proof, a spoiled hash, z = r and an undecodable proof among them: (inputs, codes)"""
    ge_r = ko.R_MOD.to_bytes(32, "little")
    mix = [rows[0], rows[0][:144] + rows[1][144:], rows[1], b"\x02" + rows[2][1:], rows[2], rows[3][:32] + ge_r + rows[3][64:],
           rows[3], rows[1][:144] + bytes([0x80]) + bytes(47)]
    return mix, [1, 0, 1, 4, 1, 2, 1, 3]


def test_precompile_device_buffer_form(kz, golden):
    """the _dev form on device-resident rows: identical codes"""
    import torch
    eth, rows, _ = golden
    mix, want = golden_mix(rows)
    assert list(eth.point_evaluation_precompile_batch(as_array(mix))) == want
    d_in = torch.from_numpy(as_array(mix).copy()).to("cuda:0")
    d_res = torch.full((len(mix),), 0xAA, dtype=torch.uint8, device="cuda:0")
    torch.cuda.synchronize()
    eth.point_evaluation_precompile_batch_dev(d_in.data_ptr(), len(mix), d_res.data_ptr())
    eth.point_evaluation_precompile_batch_dev(d_in.data_ptr(), 0, d_res.data_ptr())
    torch.cuda.synchronize()
    assert list(d_res.cpu().numpy()) == want


def test_precompile_device_buffer_form_with_the_setup_replaced_behind_it(kz, golden):
    """set_setup_g2 right behind a _dev call, while its kernels may still be queued: they keep the setup they were queued with (the handle
    holds it until the stream has passed them), the second _dev call runs on the new one, and closing the handle lets both go"""
    import json
    import torch
    _, rows, _ = golden
    mix, want = golden_mix(rows)
    fx = json.load(open(os.path.join(GOLDEN, "trusted_setup_g2.json")))
    fs = kz.FFTSettings(12)
    g2 = fs.g2_from_compressed(np.frombuffer(b"".join(bytes.fromhex(h) for h in fx["setup_G2"]), dtype=np.uint8))
    eth = kz.EthSettings(fs, lagrange_setup())
    try:
        eth.set_setup_g2(g2)
        d_in = torch.from_numpy(as_array(mix).copy()).to("cuda:0")
        d_a = torch.full((len(mix),), 0xAA, dtype=torch.uint8, device="cuda:0")
        d_b, d_c = d_a.clone(), d_a.clone()
        torch.cuda.synchronize()
        eth.point_evaluation_precompile_batch_dev(d_in.data_ptr(), len(mix), d_a.data_ptr())
        eth.set_setup_g2(g2)                                                                      # replaces the state the queued kernels read
        eth.point_evaluation_precompile_batch_dev(d_in.data_ptr(), len(mix), d_b.data_ptr())
        eth.point_evaluation_precompile_batch_dev(d_in.data_ptr(), len(mix), d_c.data_ptr())   # the same state twice in a row
        eth.set_setup_g2(g2)
        assert list(eth.point_evaluation_precompile_batch(as_array(mix))) == want
        torch.cuda.synchronize()
        assert [list(d.cpu().numpy()) for d in (d_a, d_b, d_c)] == [want] * 3
    finally:
        eth.close(); fs.close()


def test_precompile_eight_threads_on_one_handle(kz, golden):
    eth, rows, _ = golden
    mix, want = golden_mix(rows)
    results, errors = [None] * 8, []

    def work(k):
        try:
            order = [(i + k) % len(mix) for i in range(len(mix))]
            got = eth.point_evaluation_precompile_batch(as_array([mix[i] for i in order]))
            results[k] = (list(got), [want[i] for i in order])
        except Exception as e:                                                                  # noqa: BLE001
            errors.append(repr(e))

    threads = [threading.Thread(target=work, args=(k,)) for k in range(8)]
    for t in threads:
        t.start()
    for t in threads:
        t.join()
    assert not errors, errors
    for k, (got, w) in enumerate(results):
        assert got == w, k


# ---------------- VerifyKZGCommitmentsAgainstTransactions ----------------
def run_blocks(eth, blocks):
    return list(eth.verify_kzg_commitments_against_transactions_batch([b[0] for b in blocks], [b[1] for b in blocks]))


@pytest.fixture(scope="module")
def named():
    blocks = ec.named_blocks(random.Random(44))
    return blocks, [ec.verify_block(txs, c) for _, txs, c in blocks]


def test_tx_named_blocks(kz, eth_fixture, named):
    """every shape the check distinguishes, in one call and each block alone: valid shapes, count off by one, a wrong hash first / middle /
    last, each malformation, two malformations (the first wins), malformed > count > hash"""
    eth, _ = eth_fixture
    blocks, want = named
    assert set(want) == {1, 4, 5, 6, 7, 8}
    got = run_blocks(eth, [(txs, c) for _, txs, c in blocks])
    bad = [(name, g, w) for (name, _, _), g, w in zip(blocks, got, want) if g != w]
    assert not bad, bad
    for (name, txs, c), w in zip(blocks, want):
        assert run_blocks(eth, [(txs, c)]) == [w], name
    assert len(eth.verify_kzg_commitments_against_transactions_batch([], [])) == 0


def test_tx_bad_block_between_good_ones(kz, eth_fixture, named):
    """every bad block between the same two good ones: the neighbours' codes do not change"""
    eth, _ = eth_fixture
    blocks, want = named
    good = [(txs, c) for (name, txs, c) in blocks if name in ("spread", "dynamic_data")]
    seq, seq_want = [], []
    for (name, txs, c), w in zip(blocks, want):
        if w != 1:
            seq += [good[0], (txs, c), good[1]]
            seq_want += [1, w, 1]
    assert len(seq) >= 3 * 10
    assert run_blocks(eth, seq) == seq_want


@pytest.mark.parametrize("n_blocks", [1, 64, 65, 300])
def test_tx_ragged_block_counts(kz, eth_fixture, n_blocks):
    """0 .. 6 commitments per block, so that block boundaries fall inside wavefronts; spoiled, miscounted and malformed blocks among them"""
    eth, _ = eth_fixture
    blocks = ec.ragged_blocks(random.Random(45), 300)[:n_blocks] if n_blocks > 1 else ec.ragged_blocks(random.Random(45), 300)[3:4]
    want = [ec.verify_block(txs, c) for txs, c in blocks]
    if n_blocks >= 64:
        assert {1, 4, 5, 8} <= set(want) and {len(c) for _, c in blocks} >= set(range(7))
    assert run_blocks(eth, blocks) == want


def test_tx_commitments_as_arrays(kz, eth_fixture):
    """the binding takes a block's commitments as a (k, 48) array as well as a list of byte strings"""
    eth, _ = eth_fixture
    rng = random.Random(46)
    c = ec.commitments(rng, 3)
    txs = [ec.blob_tx([ec.versioned_hash(x) for x in c], rng)]
    arr = np.frombuffer(b"".join(c), dtype=np.uint8).reshape(3, 48)
    assert list(eth.verify_kzg_commitments_against_transactions_batch([txs, txs], [arr, arr[:2]])) == [1, 5]
