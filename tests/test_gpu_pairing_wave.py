"""The pairing check with one wavefront per check (k_pairing_wave.hip) on the device: every tower operation against the one-lane headers' bytes,
pairing values bit for bit against the one-lane kernel, and every public verification entry under KZG_HIP_PAIRING=wave and =lane in one
process (the switch is read per call): equal masks, equal to the known truth."""
import ctypes as C
import random

import numpy as np
import pytest

import eth_exec_cases as ec
import pairing_ref as pr
import verify_cases as vc
import verify_images as vi
from oracle import koracle as ko
from test_gpu_eth_exec import fixture_g2_points, lagrange_setup, precompile_row
from test_gpu_verify import DEVICE_EXP, S_TEST, g1_mul_int, g2_kilic, g2_powers, ks16, kz  # noqa: F401
from test_gpu_verify_aggregate import Sidecars, small_handle
from test_pairing_host import arr, pe, rand_fp12  # noqa: F401
from test_pairing_wave_host import OPS, edge_operands

pytestmark = pytest.mark.gpu


def p(a):
    return a.ctypes.data_as(C.c_void_p)


@pytest.fixture(scope="module")
def fs(kz):
    h = kz.FFTSettings(4)
    yield h
    h.close()


@pytest.mark.parametrize("code", sorted(OPS), ids=[OPS[k] for k in sorted(OPS)])
def test_tower_operations(fs, pe, code):
    """8 random rows and the edge rows (0, 1, c1 = 0, all p - 1) in one launch of one workgroup per row: the bytes of pe_fp12_op"""
    rng = random.Random(200 + code)
    rows = [rand_fp12(rng) for _ in range(4)] + edge_operands(rng)
    others = [rand_fp12(rng) for _ in rows[:-2]] + [[pr.P - 1] * 12, [0] * 12]
    A = np.stack([arr(a) for a in rows])
    B = np.stack([arr(b) for b in others])
    got = fs.wave_fp12_op(code, A, B)
    for i in range(len(rows)):
        want = np.zeros(144, dtype=np.uint32)
        a, b = np.ascontiguousarray(A[i]), np.ascontiguousarray(B[i])
        pe.pe_fp12_op(code, p(a), p(b), p(want))
        assert np.array_equal(got[i], want), (OPS[code], i)


@pytest.mark.parametrize("n", [1, 3, 65])
def test_values_equal_the_lane_kernel(kz, fs, n):
    """a grid of one, a small grid, more workgroups than a CU holds; infinity on either side among them"""
    ks = [(3 * i + 1) % 23 for i in range(n)]
    g1 = np.stack([g1_mul_int(k) for k in ks])
    Qs = [pr.g2_mul(pr.G2_GEN, 2 + (i % 5)) for i in range(n)]
    if n > 1:
        g1[1] = ko.g1_zero(1)[0]
        Qs[2] = None
        g1[0] = ko.g1_add(g1[0], ko.g1_zero(1)[0])              # a Jacobian image as the oracle leaves it
    g2 = np.stack([g2_kilic(Q) for Q in Qs])
    lane, wave = fs.pairing_test(g1, g2), fs.pairing_test_wave(g1, g2)
    assert wave == lane
    if n > 1:
        one = [1] + [0] * 11
        assert wave[1] == one and wave[2] == one and wave[0] != one
    if n == 1:
        val = wave[0]
        assert pr.from_tower([(val[2 * k], val[2 * k + 1]) for k in range(6)]) == pr.multi_pairing([(pr.g1_mul(pr.G1_GEN, ks[0]), Qs[0])], DEVICE_EXP)


def both_routes(monkeypatch, call):
    out = {}
    for route in ("wave", "lane"):
        monkeypatch.setenv("KZG_HIP_PAIRING", route)
        out[route] = [int(v) for v in call()]
    monkeypatch.delenv("KZG_HIP_PAIRING")
    assert out["wave"] == out["lane"]
    return out["wave"]


def test_check_proof_single_batch_on_both_routes(ks16, monkeypatch):
    rng = random.Random(34)
    rows = vc.single_rows(S_TEST, rng)
    cs, pis, xs, ys = vi.single_images(rows, rng)
    got = both_routes(monkeypatch, lambda: ks16.check_proof_single_batch(cs, pis, xs, ys))
    bad = [(r[0], g, r[5]) for r, g in zip(rows, got) if bool(g) != r[5]]
    assert not bad, bad
    assert True in [r[5] for r in rows] and False in [r[5] for r in rows]


def test_check_proof_multi_batch_on_both_routes(ks16, monkeypatch):
    rng = random.Random(35)
    rows = vc.multi_rows(S_TEST, random.Random(2))
    seen = set()
    for n in vc.MULTI_NS:
        sub = [r for r in rows if r[5] == n]
        cs = np.stack([vi.g1_scalar(r[1], rng.randrange(2, pr.P) if i % 2 else None) for i, r in enumerate(sub)])
        pis = np.stack([vi.g1_scalar(r[2], None if i % 3 else rng.randrange(2, pr.P)) for i, r in enumerate(sub)])
        xs, yss = ko.fr_from_ints([r[3] for r in sub]), np.stack([ko.fr_from_ints(r[4]) for r in sub])
        got = both_routes(monkeypatch, lambda: ks16.check_proof_multi_batch(cs, pis, xs, yss))
        bad = [(r[0], g, r[6]) for r, g in zip(sub, got) if bool(g) != r[6]]
        assert not bad, bad
        seen |= {r[6] for r in sub}
    assert seen == {True, False}


def test_pairings_verify_batch_on_both_routes(fs, monkeypatch):
    """the kernel that reads its own lines per check (SHARED = false): valid and invalid rows, infinity on one and on both sides"""
    A = [g1_mul_int(a) for a in range(1, 7)]
    Qa = [g2_kilic(pr.g2_mul(pr.G2_GEN, a)) for a in range(1, 7)]
    inf1, inf2 = ko.g1_zero(1)[0], g2_kilic(None)
    a1, a2, b1, b2, want = [], [], [], [], []
    for i in range(70):
        a = i % 5
        if i % 13 == 5:
            a1.append(inf1); a2.append(Qa[0]); b1.append(A[0]); b2.append(inf2); want.append(1)
        elif i % 13 == 6:
            a1.append(inf1); a2.append(Qa[0]); b1.append(A[0]); b2.append(Qa[0]); want.append(0)
        elif i % 2 == 0:
            a1.append(A[a]); a2.append(Qa[0]); b1.append(A[0]); b2.append(Qa[a]); want.append(1)
        else:
            a1.append(A[a]); a2.append(Qa[0]); b1.append(A[0]); b2.append(Qa[a + 1]); want.append(0)
    args = [np.stack(v) for v in (a1, a2, b1, b2)]
    assert both_routes(monkeypatch, lambda: fs.pairings_verify_batch(*args)) == want


@pytest.fixture(scope="module")
def eth4096(kz):
    enc, pts = fixture_g2_points()
    h = kz.FFTSettings(12)
    eth = kz.EthSettings(h, lagrange_setup())
    eth.set_setup_g2(np.stack([vi.g2_kilic(Q) for Q in pts]))
    yield eth
    eth.close(); h.close()


def one_row_per_status():
    rows, seen = [], set()
    for r in vi.eth_rows(1337, random.Random(4)):
        if r[5] not in seen:
            seen.add(r[5]); rows.append(r)
    assert seen == {0, 1, 2, 3}
    return rows


def test_eth_verify_kzg_proof_batch_on_both_routes(eth4096, monkeypatch):
    rows = one_row_per_status()
    c48, zs, ys, pi48 = vi.eth_arrays(rows)
    assert both_routes(monkeypatch, lambda: eth4096.verify_kzg_proof_batch(c48, zs, ys, pi48)) == [r[5] for r in rows]


def test_precompile_on_both_routes(eth4096, monkeypatch):
    rows = one_row_per_status()
    inputs = [precompile_row(ec.versioned_hash(r[1]), r) for r in rows]
    data = np.frombuffer(b"".join(inputs), dtype=np.uint8).reshape(len(inputs), 192)
    assert both_routes(monkeypatch, lambda: eth4096.point_evaluation_precompile_batch(data)) == [r[5] for r in rows]


def test_aggregate_verifier_on_both_routes(kz, monkeypatch):
    h, eth = small_handle(kz)
    sc = Sidecars(eth, [1, 2, 1], seed=78)
    sc.proofs[0] = sc.proofs[2].copy()
    args = sc.args()
    assert both_routes(monkeypatch, lambda: eth.verify_aggregate_kzg_proof_batch(*args)) == [0, 1, 1]
    eth.close(); h.close()


def test_route(kz, monkeypatch):
    monkeypatch.delenv("KZG_HIP_PAIRING", raising=False)
    below = kz.pairing_route(1)[1]
    for forced in ("lane", "wave"):
        monkeypatch.setenv("KZG_HIP_PAIRING", forced)
        assert kz.pairing_route(1) == (forced, below) and kz.pairing_route(100000) == (forced, below)
    monkeypatch.delenv("KZG_HIP_PAIRING")
    assert kz.pairing_route(below)[0] == "lane"
    if below:
        assert kz.pairing_route(below - 1)[0] == "wave"
