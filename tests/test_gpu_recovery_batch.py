"""Batched erasure recovery on the device (kzg_hip_recover_poly_from_samples_batch / _dev, kzg_hip_zero_poly_via_multiplication_batch): every row bit for bit
what the lone call returns for that row alone -- status and bytes -- and what the oracle returns wherever it accepts the row."""
import os
import subprocess
import sys
import threading

import numpy as np
import pytest

import recovery_batch_cases as rc
from oracle import koracle as ko
from oracle import pyref

pytestmark = pytest.mark.gpu

OWN = os.path.abspath(__file__)
SCALE = 13            # one settings object for every n: strides above 1 below 8192 points
ROWS = 65
FULL_DEGREE = 11      # a row with n / 2 missing whose polynomial has all n coefficients: whatever the lone call yields, the batch row agrees


@pytest.fixture(scope="module")
def kz():
    import gokzg_amd
    assert gokzg_amd.device_count() >= 1, "no gfx950 device: the HIP path is the only path"
    return gokzg_amd


@pytest.fixture(scope="module")
def fs(kz):
    fs = kz.FFTSettings(SCALE)
    yield fs
    fs.close()


_problems, _lone, _oracle = {}, {}, {}


def problem(n):
    """65 rows of n samples with ragged per-row masks: 0, 1, n/2 - 1, n (nothing present), n/2, n/2 + 1, n - 1 missing, repeated"""
    if n not in _problems:
        ofs = ko.FFTSettings(n.bit_length() - 1)
        data = rc.data_rows(ofs, n, ROWS, 1000 + n, full_degree=(FULL_DEGREE,))
        present = rc.ragged_masks(n, ROWS, np.random.default_rng(n))
        _problems[n] = (data, present, rc.blanked(data, present))
    return _problems[n]


def lone_row(kz, fs, samples, present):
    n = samples.shape[0]
    out = np.zeros((n, 4), dtype=np.uint64)
    st = kz.lib().kzg_hip_recover_poly_from_samples(fs.h, samples.ctypes.data, present.ctypes.data, n, out.ctypes.data)
    return st, out                                                          # (a failed lone call leaves its output alone: zeros, as a failed batch row)


def lone(kz, fs, n):
    if n not in _lone:
        _, present, samples = problem(n)
        _lone[n] = [lone_row(kz, fs, samples[r], present[r]) for r in range(ROWS)]
    return _lone[n]


def oracle(n):
    """the oracle on the rows it is asked about: all of them at the small sizes, one row per missing count at the large ones"""
    if n not in _oracle:
        _, present, samples = problem(n)
        ofs = ko.FFTSettings(SCALE)
        _oracle[n] = [rc.oracle_row(ofs, samples[r], present[r]) for r in range(ROWS if n <= 64 else 7)]
    return _oracle[n]


def check_against_lone(kz, fs, n, rows, out, status):
    want = lone(kz, fs, n)
    for r in range(rows):
        assert status[r] == want[r][0] and np.array_equal(out[r], want[r][1]), (n, r)


@pytest.mark.parametrize("batch", [1, 2, 3, 65], ids=lambda b: "b%d" % b)
@pytest.mark.parametrize("n", [16, 64, 4096, 8192], ids=lambda n: "n%d_" % n)
def test_rows_match_lone_and_oracle(kz, fs, n, batch):
    data, present, samples = problem(n)
    out, status = fs.recover_poly_from_samples_batch(samples[:batch], present[:batch])
    check_against_lone(kz, fs, n, batch, out, status)
    counts = rc.ragged_counts(n)
    for r, (ost, orow) in enumerate(oracle(n)[:batch]):
        missing = counts[r % len(counts)]
        if missing == n:
            assert status[r] == rc.ERR_BAD_ARG and not out[r].any()
        elif missing == 0:
            assert status[r] == rc.OK and np.array_equal(out[r], samples[r])   # copied through; the oracle refuses a row with nothing missing
        elif ost is not None:
            assert status[r] == rc.OK and np.array_equal(out[r], orow), (n, r)
        if 0 < missing <= n // 2 and r != FULL_DEGREE:
            assert np.array_equal(out[r], data[r]), (n, r)                  # the reference's own property (recover_from_samples_test.go:62-137)


@pytest.mark.parametrize("n", [64, 4096], ids=lambda n: "n%d_" % n)
def test_shared_mask(kz, fs, n):
    """one mask for 17 rows: the bytes of the same mask replicated per row, and of the lone call"""
    data, present, _ = problem(n)
    mask = present[4]                                                      # half of the columns lost
    samples = rc.blanked(data[:17], mask)
    out, status = fs.recover_poly_from_samples_batch(samples, mask)
    out_rep, status_rep = fs.recover_poly_from_samples_batch(samples, np.tile(mask, (17, 1)))
    assert np.array_equal(out, out_rep) and np.array_equal(status, status_rep) and not status.any()
    for r in (0, 9, FULL_DEGREE, 16):
        st, row = lone_row(kz, fs, samples[r], mask)
        assert st == rc.OK and np.array_equal(out[r], row), r
    for r in range(17):
        if r != FULL_DEGREE:
            assert np.array_equal(out[r], data[r]), r
    full, none = np.ones(n, dtype=np.uint8), np.zeros(n, dtype=np.uint8)
    out, status = fs.recover_poly_from_samples_batch(data[:3], full)       # nothing missing: copied through
    assert np.array_equal(out, data[:3]) and not status.any()
    out, status = fs.recover_poly_from_samples_batch(data[:3], none)       # nothing present
    assert not out.any() and list(status) == [rc.ERR_BAD_ARG] * 3


def zero_lists(n):
    rng = np.random.default_rng(50 + n)
    pick = lambda c: np.sort(rng.permutation(n)[:c]).astype(np.uint64)
    lists = [pick(1), np.zeros(0, dtype=np.uint64), pick(17), np.arange(n, dtype=np.uint64), pick(n // 2), np.array([3, n, 5], dtype=np.uint64), pick(n - 1), pick(n // 2 + 1),
             pick(16), pick(33)]
    return lists


@pytest.mark.parametrize("n", [64, 4096], ids=lambda n: "n%d_" % n)
def test_zero_polynomials_match_lone(kz, fs, n):
    """ragged erasure sets in one call, among them an empty one, one with as many indices as the domain has points and one with an index out of range"""
    lists = zero_lists(n)
    ze, zp, status = fs.zero_poly_via_multiplication_batch(lists, n)
    assert list(status) == [rc.ERR_BAD_ARG if k in (3, 5) else rc.OK for k in range(len(lists))]
    ofs = ko.FFTSettings(SCALE)
    for k, m in enumerate(lists):
        e, p = np.zeros((n, 4), dtype=np.uint64), np.zeros((n, 4), dtype=np.uint64)
        st = kz.lib().kzg_hip_zero_poly_via_multiplication(fs.h, m.ctypes.data if len(m) else None, len(m), n, e.ctypes.data, p.ctypes.data)
        assert st == status[k] and np.array_equal(ze[k], e) and np.array_equal(zp[k], p), k
        if status[k] == rc.OK and 0 < len(m) <= 33:
            oe, op = ofs.zero_poly_via_multiplication(m, n)
            assert np.array_equal(ze[k], oe) and np.array_equal(zp[k], op), k
    assert not ze[1].any() and not zp[1].any() and not ze[3].any() and not ze[5].any()


def test_call_level_errors(kz, fs):
    L = kz.lib()
    s, p = np.zeros((3, 24, 4), dtype=np.uint64), np.ones((3, 24), dtype=np.uint8)
    o, st = np.zeros_like(s), np.zeros(3, dtype=np.uint8)
    call = lambda present_rows, n, batch, sp=s.ctypes.data: L.kzg_hip_recover_poly_from_samples_batch(fs.h, sp, p.ctypes.data, present_rows, n, batch, o.ctypes.data, st.ctypes.data)
    assert call(3, 24, 3) == kz.ERR_NOT_POW2 and call(3, 1 << (SCALE + 1), 3) == kz.ERR_TOO_WIDE and call(2, 16, 3) == kz.ERR_BAD_ARG
    assert call(3, 0, 3) == kz.ERR_BAD_ARG and call(3, 16, 3, None) == kz.ERR_BAD_ARG and call(1, 16, 0) == kz.OK and call(3, 8, 3) == kz.OK
    off = np.zeros(2, dtype=np.uint64)
    zcall = lambda length, batch: L.kzg_hip_zero_poly_via_multiplication_batch(fs.h, None, off.ctypes.data, batch, length, o.ctypes.data, o.ctypes.data, st.ctypes.data)
    assert zcall(24, 1) == kz.ERR_NOT_POW2 and zcall(1 << (SCALE + 1), 1) == kz.ERR_TOO_WIDE and zcall(16, 0) == kz.OK and zcall(16, 1) == kz.OK


def test_nine_rows_of_4096(kz, fs):
    """(run once more by test_chunk_edges_in_a_fresh_process with a chunk budget of three rows)"""
    _, present, samples = problem(4096)
    out, status = fs.recover_poly_from_samples_batch(samples[:9], present[:9])
    check_against_lone(kz, fs, 4096, 9, out, status)
    mask = present[2]
    shared = rc.blanked(problem(4096)[0][:9], mask)
    out, status = fs.recover_poly_from_samples_batch(shared, mask)
    for r in (0, 3, 8):                                                    # the first row of every chunk of three, and the last
        st, row = lone_row(kz, fs, shared[r], mask)
        assert status[r] == st == rc.OK and np.array_equal(out[r], row), r


def dev_call(kz, fs, samples, present):
    import torch
    batch, n = samples.shape[0], samples.shape[1]
    d_s = torch.from_numpy(samples.view(np.int64)).cuda()
    d_p = torch.from_numpy(present).cuda()
    d_out = torch.full((batch, n, 4), -1, dtype=torch.int64, device="cuda")
    d_st = torch.full((batch,), 0x55, dtype=torch.uint8, device="cuda")
    torch.cuda.synchronize()
    st = kz.lib().kzg_hip_recover_poly_from_samples_batch_dev(fs.h, d_s.data_ptr(), d_p.data_ptr(), 1 if present.ndim == 1 else batch, n, batch, d_out.data_ptr(),
                                                               d_st.data_ptr(), torch.cuda.current_stream().cuda_stream)
    assert st == 0
    torch.cuda.synchronize()
    assert np.array_equal(d_s.cpu().numpy().view(np.uint64), samples) and np.array_equal(d_p.cpu().numpy(), present)   # inputs untouched
    return d_out.cpu().numpy().view(np.uint64), d_st.cpu().numpy()


@pytest.mark.parametrize("n", [16, 64, 4096, 8192], ids=lambda n: "n%d_" % n)
def test_dev_form_equals_host_form(kz, fs, n):
    """torch tensors on the current stream: per-row masks (the host never sees the counts) and a shared mask"""
    data, present, samples = problem(n)
    rows = 14
    out, status = dev_call(kz, fs, samples[:rows], present[:rows])
    h_out, h_status = fs.recover_poly_from_samples_batch(samples[:rows], present[:rows])
    assert np.array_equal(out, h_out) and np.array_equal(status, h_status)
    for mask in (present[4], present[0], present[3]):                      # half missing, nothing missing, nothing present
        shared = rc.blanked(data[:5], mask)
        out, status = dev_call(kz, fs, shared, mask)
        h_out, h_status = fs.recover_poly_from_samples_batch(shared, mask)
        assert np.array_equal(out, h_out) and np.array_equal(status, h_status)


def test_eight_threads_on_one_handle(kz, fs):
    _, present, samples = problem(4096)
    parts = [(samples[4 * t:4 * t + 4], present[4 * t:4 * t + 4]) for t in range(8)]
    want = [fs.recover_poly_from_samples_batch(s, p) for s, p in parts]
    got = [None] * 8

    def work(t):
        got[t] = fs.recover_poly_from_samples_batch(*parts[t])

    threads = [threading.Thread(target=work, args=(t,)) for t in range(8)]
    for th in threads:
        th.start()
    for th in threads:
        th.join()
    for t in range(8):
        assert got[t] is not None and np.array_equal(got[t][0], want[t][0]) and np.array_equal(got[t][1], want[t][1]), t


def test_das_flow_recovers_eight_rows_at_once(kz):
    """the recovery step of test_full_das_flow (integration_test.go:113-159) on 8 rows in one call: random 31-byte data -> reverse-bit order -> DAS extension ->
    half of the cosets (l = 128) dropped -> recovery -> original bytes; the same cosets in every row (shared mask), then different ones per row"""
    scale, l, rows = 10, 128, 8
    points = 1 << scale
    rng = np.random.default_rng(4321)
    data = rng.integers(0, 256, size=(rows, points * 31), dtype=np.uint8)
    data[:, :100] = 0
    even = np.stack([ko.reverse_bit_order(ko.fr_from_ints([int.from_bytes(row[i * 31:(i + 1) * 31].tobytes() + b"\x00", "little") for i in range(points)])) for row in data])
    fs = kz.FFTSettings(scale + 1)
    odd = fs.das_fft_extension_batch(even)                                 # integration_test.go:42
    extended = np.empty((rows, 2 * points, 4), dtype=np.uint64)
    extended[:, 0::2], extended[:, 1::2] = even, odd
    assert not fs.fft_batch(extended, inv=True)[:, points:].any()          # the extension property
    ext_bro = np.stack([ko.reverse_bit_order(e) for e in extended])
    sample_count = 2 * points // l

    def natural_mask():
        keep = np.ones(sample_count, dtype=bool)
        keep[rng.choice(sample_count, size=sample_count // 2, replace=False)] = False
        return np.repeat(keep, l)

    def recover(present_bro):                                             # (rows, 2 points) or (2 points,) masks in reverse-bit order
        pb = np.broadcast_to(present_bro, (rows, 2 * points))
        partial = np.where(pb[:, :, None], ext_bro, 0)
        nat = lambda m: np.array(pyref.bitrev(m.astype(np.uint8).tolist()), dtype=np.uint8)
        present_nat = nat(present_bro) if present_bro.ndim == 1 else np.stack([nat(m) for m in present_bro])
        samples = np.stack([ko.reverse_bit_order(p) for p in partial])
        out, status = fs.recover_poly_from_samples_batch(samples, present_nat)
        assert not status.any()
        st, row = lone_row(kz, fs, samples[rows - 1], np.broadcast_to(present_nat, (rows, 2 * points))[rows - 1].copy())
        assert st == rc.OK and np.array_equal(out[rows - 1], row)
        return np.stack([ko.reverse_bit_order(o) for o in out])

    for present in (natural_mask(), np.stack([natural_mask() for _ in range(rows)])):
        recovered = recover(present)
        assert np.array_equal(recovered, ext_bro)
        for r in (0, rows - 1):
            back = b"".join(v.to_bytes(32, "little")[:31] for v in ko.fr_to_ints(recovered[r, :points]))
            assert back == data[r].tobytes()
    fs.close()


def child(select, **env):
    res = subprocess.run([sys.executable, "-m", "pytest", OWN, "-m", "gpu", "-x", "-q", "-p", "no:cacheprovider", "-k", select], env=dict(os.environ, **env),
                         capture_output=True, text=True, timeout=600)
    assert res.returncode == 0, (env, res.stdout[-2500:], res.stderr[-500:])
    return res.stdout


BOTH = "(rows_match_lone or zero_polynomials_match_lone) and (n64_ or n4096_)"


def test_direct_evaluation_forced_in_a_fresh_process():
    """KZG_HIP_ZERO_POLY=direct: every vanishing polynomial of the n = 64 and n = 4096 cases by direct evaluation (one child, its own timeout, no retry)"""
    assert " passed" in child(BOTH, KZG_HIP_ZERO_POLY="direct")


def test_product_tree_forced_in_a_fresh_process():
    """KZG_HIP_ZERO_POLY=tree: the same cases through the ragged product tree"""
    assert " passed" in child(BOTH, KZG_HIP_ZERO_POLY="tree")


def test_chunk_edges_in_a_fresh_process():
    """KZG_HIP_RECOVER_CHUNK_MB=3: a row of 4096 points is budgeted at 1 MiB, so 9 rows fall into three chunks of three; results equal the lone calls, which
    test_nine_rows_of_4096 shows the unchunked call to equal.  The ragged zero polynomials of 4096 points are cut the same way."""
    assert " passed" in child("nine_rows_of_4096 or (zero_polynomials_match_lone and n4096_)", KZG_HIP_RECOVER_CHUNK_MB="3")
