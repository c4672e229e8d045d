"""eth.ComputeKZGProof and the evaluation-form evaluators in every launch shape of the quotient kernels (launch_eth_quotient, csrc/k_fr.hip).

Two implementations sit behind one dispatcher: the row-split form (k_eth_quotient_parts + k_eth_quotient_finish: one element per lane, S = n / 1024
workgroups per row) for small batches of 2048 ... 65 536 points, and the one-workgroup form (k_eth_quotient: 1024 lanes walk the row in blocks of 4096,
up to four denominators per lane and block) for everything else -- at the blob size every batch of more than 64 rows, which is what the benchmark
times and what more than 64 coalesced callers run.  Every (n, batch) below is chosen for the branch it takes, and the branch is asserted from the
dispatch rule restated in tests/eth_rows.py (tests/test_eth_rows.py pins that restatement to the source).

Truth is tests/eth_rows.py: Python integers, the proof as a known multiple of the generator.  Every row of every batch is compared, bit for bit.
Rows whose z lies in the domain must come back refused and zeroed, from the host-buffer entry (which zeroes on the host) and from the device-resident
entry (where the kernel's own zeroing is what the caller sees: y = 0 and the proof of a zero quotient, the point at infinity).
"""
import os
import random
import subprocess
import sys
import threading

import numpy as np
import pytest

import eth_rows as er
from oracle import koracle as ko
from oracle import pyref

pytestmark = pytest.mark.gpu

R = er.R
FORCED_ONE = os.environ.get("KZG_HIP_ETH_QUOTIENT") == "one"      # read once per process by the library: the hook test below re-runs parts of this file under it


@pytest.fixture(scope="module")
def kz():
    import gokzg_amd
    assert gokzg_amd.device_count() >= 1, "no gfx950 device: the HIP path is the only path"
    return gokzg_amd


@pytest.fixture
def small_tables(monkeypatch):
    """every EthSettings builds a commitment table of its own: 1 GB each (8-bit windows at 4096 points) instead of the default 103 GB"""
    monkeypatch.setenv("KZG_HIP_FB_BUDGET_GB", "1.0")


class Eth:
    """settings of one size with the secret that goes with their setup: the committed Lagrange setup (s = 1337) at 4096 points, a generated one otherwise"""

    def __init__(self, kz, n):
        self.kz, self.n = kz, n
        self.s = er.S_GOLDEN if n == 4096 else er.S_TEST
        lag = er.golden_lagrange_setup() if n == 4096 else er.lagrange_setup(n)
        self.fs = kz.FFTSettings(max(er.ilog2(n), 4))            # (below 16 points the settings are wider than the setup: every (W / n)-th root)
        self.eth = kz.EthSettings(self.fs, lag)
        self.ref = er.Reference(n, self.s)

    def close(self):
        self.eth.close()
        self.fs.close()

    def __enter__(self):
        return self

    def __exit__(self, *exc):
        self.close()
        return False


def compare(rows, want, proofs, ys, ok, tag, dev=False):
    """every row, bit for bit; `dev`: the device-resident entry's contract for a refused row (flag set, y = 0, the proof bytes of the point at infinity)"""
    got_y = ko.fr_to_ints(ys) if ys is not None else None
    wrong = []
    for b, ((name, _, _), (w_ok, w_y, w_proof)) in enumerate(zip(rows, want)):
        if not w_ok and dev:
            w_proof = er.ZERO_PROOF
        g_proof = bytes(proofs[b])
        if bool(ok[b]) != w_ok or g_proof != w_proof or (got_y is not None and (got_y[b] != w_y or (not w_ok and np.asarray(ys[b]).any()))):
            wrong.append((b, name, bool(ok[b]), g_proof[:6].hex(), w_proof[:6].hex()))
    assert not wrong, "%s: %d of %d rows differ, first: %s" % (tag, len(wrong), len(rows), wrong[:6])


def run_dev(kz, e, polys, zs, with_ys):
    """kzg_hip_eth_compute_kzg_proof_batch_dev on torch tensors: (proofs, ys or None, flags)"""
    import torch
    b = polys.shape[0]
    d_polys = torch.from_numpy(polys.view(np.int64)).cuda()
    d_zs = torch.from_numpy(zs.view(np.int64)).cuda()
    d_out = torch.full((b, 48), 0xEE, dtype=torch.uint8, device="cuda")
    d_bad = torch.full((b,), 0x55, dtype=torch.int32, device="cuda")       # (the entry clears the flags itself)
    d_ys = torch.full((b, 4), -1, dtype=torch.int64, device="cuda") if with_ys else None
    torch.cuda.synchronize()
    st = kz.lib().kzg_hip_eth_compute_kzg_proof_batch_dev(e.eth.h, d_polys.data_ptr(), e.n, b, d_zs.data_ptr(), d_out.data_ptr(),
                                                          d_ys.data_ptr() if with_ys else None, d_bad.data_ptr(), torch.cuda.current_stream().cuda_stream)
    assert st == 0, (st, kz.lib().kzg_hip_last_error().decode())
    torch.cuda.synchronize()
    ys = d_ys.cpu().numpy().view(np.uint64).reshape(b, 4) if with_ys else None
    return d_out.cpu().numpy(), ys, d_bad.cpu().numpy() == 0


def run_shape(kz, e, batch, rng, pool, boundaries, dev_null_ys=False):
    rows = er.batch_of(e.n, batch, e.s, rng, boundaries, pool)
    want = [e.ref.expected(p, z) for _, p, z in rows]
    polys, zs = er.to_arrays(rows)
    tag = "n=%d batch=%d" % (e.n, batch)
    proofs, ys, ok = e.eth.compute_kzg_proof_batch(polys, zs)
    compare(rows, want, proofs, ys, ok, tag + " host buffers")
    proofs, ys, ok = run_dev(kz, e, polys, zs, True)
    compare(rows, want, proofs, ys, ok, tag + " device-resident", dev=True)
    if dev_null_ys:
        proofs, ys, ok = run_dev(kz, e, polys, zs, False)
        compare(rows, want, proofs, None, ok, tag + " device-resident, d_ys = NULL", dev=True)
    return rows, want


# (n, [(batch, row-split form?)], rows on either side of which the dispatch changes)
SHAPES = [
    (4096, [(1, True), (64, True), (65, False), (96, False), (512, False)], (64,)),    # 64: the last split shape; 96: the coalescer's cap; 512: the benchmark's
    (8192, [(1, True), (32, True), (33, False)], (32,)),                              # 32: S = 8, 256 workgroups; 33: one workgroup, two blocks of 4096
    (2048, [(128, True), (129, False)], (128,)),                                      # 129: one workgroup, two slots per lane
    (1024, [(1, False), (48, False)], ()),                                            # one slot per lane ...
    (512, [(1, False), (48, False)], ()),                                             # ... and lanes beyond n
    (16, [(1, False), (48, False)], ()),                                              # below 64 points the commitment runs on the bucket pipeline
    (2, [(1, False), (48, False)], ()),
    (1, [(1, False), (48, False)], ()),
]


@pytest.mark.parametrize("n,batches,boundaries", SHAPES, ids=["n%d" % s_[0] for s_ in SHAPES])
def test_compute_kzg_proof_in_every_launch_shape(kz, small_tables, n, batches, boundaries):
    """every (n, batch) of the list, through the host-buffer entry and the device-resident one (512 rows at 4096 points also with d_ys = NULL, the
    benchmark's call); a batch of one is run once for EVERY crafted row"""
    rng = random.Random(77000 + n)
    pool = [er.rand_poly(rng, n) for _ in range(6)]
    with Eth(kz, n) as e:
        for batch, split in batches:
            assert er.split_form(n, batch) == split, (n, batch)     # the branch this shape was chosen for
            if batch == 1:
                for row in er.named_rows(n, e.s, rng, pool):
                    want = [e.ref.expected(row[1], row[2])]
                    polys, zs = er.to_arrays([row])
                    proofs, ys, ok = e.eth.compute_kzg_proof_batch(polys, zs)
                    compare([row], want, proofs, ys, ok, "n=%d lone row" % n)
                    proofs, ys, ok = run_dev(kz, e, polys, zs, True)
                    compare([row], want, proofs, ys, ok, "n=%d lone row, device-resident" % n, dev=True)
            else:
                run_shape(kz, e, batch, rng, pool, boundaries, dev_null_ys=(n, batch) == (4096, 512))


def test_small_batches_and_the_one_polynomial_entry(kz, small_tables):
    """batches of 1 ... 7 rows at 2048, 4096 and 8192 points (row-split by default; one workgroup per row in the child process that forces it), then every
    crafted row through the one-polynomial entry: a lone coalesced call reads its row of stride n + 1 in place from pinned host memory"""
    for n in (4096, 2048, 8192):
        rng = random.Random(88000 + n)
        pool = [er.rand_poly(rng, n) for _ in range(3)]
        with Eth(kz, n) as e:
            for batch in (2, 3, 4, 5, 7):
                assert er.split_form(n, batch) or FORCED_ONE
                run_shape(kz, e, batch, rng, pool, ())
            for name, poly, z in er.named_rows(n, e.s, rng, pool):
                w_ok, w_y, w_proof = e.ref.expected(poly, z)
                p_img, z_img = ko.fr_from_ints(poly), ko.fr_from_ints([z])
                if not w_ok:
                    with pytest.raises(kz.KzgError, match="invalid z challenge"):
                        e.eth.compute_kzg_proof(p_img, z_img)
                    continue
                proof, y = e.eth.compute_kzg_proof(p_img, z_img)
                assert proof.tobytes() == w_proof and ko.fr_to_ints(y.reshape(1, 4))[0] == w_y, (n, name)


def test_128_concurrent_callers_of_the_one_polynomial_entry(kz, small_tables):
    """128 threads on eth.ComputeKZGProof, a few of them with a z in the domain: the shape in which a coalesced batch can exceed 64 rows (and then runs
    the one-workgroup kernel on rows of stride n + 1).  Only results are asserted here -- the forced-hook child process guarantees the kernel form."""
    n, T = 4096, 128
    rng = random.Random(128)
    pool = [er.rand_poly(rng, n) for _ in range(6)]
    with Eth(kz, n) as e:
        rows = er.batch_of(n, T, e.s, rng, (64,), pool)
        keep_invalid = {0, 17, 63, 95, 96, T - 1}                    # a few refused callers, the rest valid
        dom = er.domain(n)
        for i, (name, poly, z) in enumerate(rows):
            if i in keep_invalid:
                rows[i] = ("caller_%d_in_domain" % i, poly, dom[(i * 1061) % n])
            elif pow(z, n, R) == 1:
                rows[i] = ("ordinary", poly, rng.randrange(2, R))
        want = [e.ref.expected(p, z) for _, p, z in rows]
        polys, zs = er.to_arrays(rows)
        proofs, ys, ok = e.eth.compute_kzg_proof_batch(polys, zs)
        compare(rows, want, proofs, ys, ok, "128 rows as one batch")
        assert [i for i in range(T) if not ok[i]] == sorted(keep_invalid)
        got, errs = [None] * T, [None] * T
        gate = threading.Barrier(T)

        def work(i):
            try:
                gate.wait()
                for _ in range(3):
                    got[i] = e.eth.compute_kzg_proof(polys[i], zs[i:i + 1])
            except kz.KzgError as err:
                errs[i] = err
            except Exception as err:  # noqa: BLE001
                errs[i] = err
        ts = [threading.Thread(target=work, args=(i,)) for i in range(T)]
        [t.start() for t in ts]
        [t.join() for t in ts]
        for i in range(T):
            if ok[i]:
                assert errs[i] is None and got[i][0].tobytes() == proofs[i].tobytes() == want[i][2] and np.array_equal(got[i][1], ys[i]), (i, rows[i][0], errs[i])
            else:
                assert isinstance(errs[i], kz.KzgError) and "invalid z challenge" in str(errs[i]), (i, rows[i][0], errs[i])


# (points, what the dispatcher does with a lone row of that size)
EVAL_SIZES = [(1024, False), (2048, True), (8192, True), (65536, True), (131072, False)]    # 65 536: S = 64, the largest split; 131 072: one workgroup, 32 blocks


@pytest.mark.parametrize("n,split", EVAL_SIZES, ids=["n%d" % s_[0] for s_ in EVAL_SIZES])
def test_evaluators_at_every_size(kz, n, split):
    """bls.EvaluatePolyInEvaluationForm on the natural-order domain, on a strided one (settings one scale wider, scale = 1) and
    eth.EvaluatePolynomialInEvaluationForm on the bit-reversed one, against Horner's rule on the coefficients (pyref.eval_poly); an x inside the
    domain -- first element, the last block of 4096, last element -- gives the reference's 0 (bls/globals.go:141-152)"""
    assert er.split_form(n, 1) == split
    rng = random.Random(99000 + n)
    scale = er.ilog2(n)
    coeffs = [rng.randrange(R) for _ in range(n)]
    pfs = pyref.FFTSettings(scale)
    evals = pfs.fft(coeffs)
    ev_img = ko.fr_from_ints(evals)
    outside = [rng.randrange(R) for _ in range(3)] + [0, er.root_of_unity(2 * n), R - 2]
    inside = sorted({0, 1, n // 2, n - 4096 + 1024 + 63 if n > 4096 else n // 3, n - 1})
    xs = [(x, pyref.eval_poly(coeffs, x)) for x in outside] + [(pfs.expanded[i], 0) for i in inside]
    x_img = ko.fr_from_ints([x for x, _ in xs])

    def check(call, tag):
        for k, (x, want) in enumerate(xs):
            assert ko.fr_to_ints(call(x_img[k:k + 1]).reshape(1, 4))[0] == want, (tag, n, k)
    fs = kz.FFTSettings(scale)
    check(lambda x: fs.evaluate_poly_in_evaluation_form(ev_img, x), "natural order")
    # eth's evaluator reads the handle's bit-reversed domain only: any n points make a setup for it
    eth = kz.EthSettings(fs, np.tile(ko.g1_generator(), (n, 1, 1)))
    br_img = ko.reverse_bit_order(ev_img)
    check(lambda x: eth.evaluate_polynomial_in_evaluation_form(br_img, x), "eth, bit-reversed")
    eth.close(); fs.close()
    wide = kz.FFTSettings(scale + 1)
    check(lambda x: wide.evaluate_poly_in_evaluation_form(ev_img, x, 1), "strided")
    wide.close()


OWN = os.path.abspath(__file__)
PARITY = os.path.join(os.path.dirname(OWN), "test_gpu_parity.py")
# the coalesced callers (rows of stride n + 1, read in place over PCIe or staged), the small batches, and the lone rows of the aggregate proof and the evaluators
HOOK_RUNS = [
    ({"KZG_HIP_ETH_QUOTIENT": "one"}, "small_batches or 128_concurrent or eth_blob_to_kzg or eth_compute_kzg_proof_batch or eth_compute_aggregate or "
                                      "test_evaluate_poly_in_evaluation_form"),
    ({"KZG_HIP_ETH_STAGE_ROWS": "8"}, "small_batches or 128_concurrent or eth_blob_to_kzg or eth_compute_kzg_proof_batch"),    # 20 and 128 threads: batches on both sides of 8 rows
    ({"KZG_HIP_ETH_QUOTIENT": "one", "KZG_HIP_ETH_STAGE_ROWS": "8"}, "small_batches or eth_compute_kzg_proof_batch"),
]


def test_forced_kernel_form_and_staged_rows_in_fresh_processes():
    """KZG_HIP_ETH_QUOTIENT=one (one workgroup per row at every size) and KZG_HIP_ETH_STAGE_ROWS=8 (coalesced batches of up to 8 rows are copied to HBM
    first) are read once per process: child processes, one after another, each with its own timeout and -x; nothing is started after the first failure"""
    for extra, select in HOOK_RUNS:
        env = dict(os.environ, KZG_HIP_FB_BUDGET_GB="1.0", **extra)       # (small commitment tables in the children too)
        res = subprocess.run([sys.executable, "-m", "pytest", OWN, PARITY, "-m", "gpu", "-x", "-q", "-p", "no:cacheprovider", "-k", select],
                             env=env, capture_output=True, text=True, timeout=900)
        assert res.returncode == 0, (extra, res.stdout[-2500:], res.stderr[-500:])
