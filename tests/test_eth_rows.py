"""tests/eth_rows.py is what it claims to be (no GPU): its discrete-log form of eth.ComputeKZGProof equals the reference's formula as written, its
Lagrange setups are the oracle's, and its dispatch rule is the source's."""
import os
import random

import numpy as np
import pytest

import eth_rows as er
from oracle import koracle as ko
from oracle import pyref

R = er.R
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


@pytest.mark.parametrize("n", [1, 2, 16, 64])
def test_generated_lagrange_setup_is_the_inverse_transform_of_the_testing_setup(n):
    """[L_i(s)] G1 == FFTG1^-1 of GenerateTestingSetup(s, n) (how eth/ derives setup_G1_lagrange from setup_G1), point by point"""
    lag = er.lagrange_setup(n)
    mono = ko.generate_testing_setup_g1(er.S_TEST, n)
    want = ko.FFTSettings(er.ilog2(n)).fft_g1(mono, inv=True)
    assert np.array_equal(ko.g1_affine(lag), ko.g1_affine(want))
    assert sum(er.lagrange_dlogs(n, er.S_TEST)) % R == 1              # the Lagrange basis sums to one


@pytest.mark.parametrize("n", [16, 64])
def test_dlog_form_equals_the_formula_as_written_on_every_named_row(n):
    """every crafted row of the GPU tests: (p(s) - y) / (s - z) G1 == LinCombG1(bit-reversed Lagrange setup, (p_i - y) / (w_i - z)), y == the
    barycentric formula, and rows in the domain are refused by both"""
    rng = random.Random(1000 + n)
    lag = er.lagrange_setup(n)
    ref = er.Reference(n, er.S_TEST)
    rows = er.named_rows(n, er.S_TEST, rng)
    names = [name for name, _, _ in rows]
    assert len(set(names)) == len(names)
    for want in ("random_z", "z=0", "z=1_in_domain", "z=r-1_in_domain", "domain_slot0_lane0", "z^n=-1", "zero_polynomial", "constant_polynomial",
                 "entries_r-1", "value_at_0_equals_y"):
        assert want in names, want
    seen_invalid = 0
    for name, poly, z in rows:
        ok, y, proof = ref.expected(poly, z)
        lok, ly, lproof = er.literal_proof(n, poly, z, lag)
        assert (ok, y, proof) == (lok, ly, lproof), name
        assert ok == (pow(z, n, R) != 1), name
        if not ok:
            seen_invalid += 1
            assert y == 0 and proof == bytes(48), name
            continue
        assert y == pyref.eval_in_evaluation_form(list(poly), z, er.domain(n)), name
        if name.startswith("zero_polynomial"):
            assert y == 0 and proof == er.ZERO_PROOF
        if name.startswith("constant"):
            assert y == poly[0] and proof == er.ZERO_PROOF           # every quotient is zero
        if name.startswith("value_at_"):
            assert y in poly
        if name.startswith("z^n=-1"):
            assert pow(z, n, R) == R - 1
    assert seen_invalid >= 4


def test_named_rows_reach_every_slot_and_block_of_the_one_workgroup_kernel():
    """at 4096 points a domain element in each of the four slots of lanes 0, 63, 64 and 1023; at 8192 points in the second block of 4096"""
    rng = random.Random(5)
    pool = [er.rand_poly(rng, 8192)]
    rows = er.named_rows(8192, er.S_TEST, rng, pool)
    dom = er.domain(8192)
    hit = {dom.index(z) for _, _, z in rows if pow(z, 8192, R) == 1}
    assert {tid + 1024 * k for tid in er.SLOT_LANES for k in range(4)} <= hit
    assert {4096, 4096 + 1024 + 63, 8191} <= hit
    batch = er.batch_of(16, 70, er.S_TEST, rng, boundaries=(64,))
    inv = [pow(z, 16, R) == 1 for _, _, z in batch]
    assert len(batch) == 70 and inv[0] and inv[69] and inv[63] and not inv[64]


def test_one_row_at_4096_points_agrees_with_the_committed_lagrange_setup():
    rng = random.Random(4096)
    lag = er.golden_lagrange_setup()
    ref = er.Reference(4096, er.S_GOLDEN)
    poly = er.rand_poly(rng, 4096)
    z = rng.randrange(R)
    assert ref.expected(poly, z) == er.literal_proof(4096, poly, z, lag)
    assert ref.expected(poly, er.domain(4096)[2049]) == (False, 0, bytes(48))


def test_dispatch_rule_is_the_one_in_the_source():
    """split_form() restates eth_quotient_scratch_elems: a change of its thresholds has to come here (and to the shapes of tests/test_gpu_eth_quotient.py)"""
    src = open(os.path.join(ROOT, "go-kzg_amd", "csrc", "k_fr.hip")).read()
    assert er.SPLIT_RULE_SOURCE in src
    assert "const uint64_t S = n / 1024;" in src
    assert [er.split_form(4096, b) for b in (1, 64, 65, 96, 512)] == [True, True, False, False, False]
    assert [er.split_form(8192, b) for b in (1, 32, 33)] == [True, True, False]
    assert [er.split_form(2048, b) for b in (128, 129)] == [True, False]
    assert not any(er.split_form(n, 1) for n in (1024, 512, 16, 2, 1, 131072))
    assert er.split_form(65536, 1) and not er.split_form(65536, 5)
