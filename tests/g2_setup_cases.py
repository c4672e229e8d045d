"""Scalars and reference points shared by tests/test_g2_setup_host.py and tests/test_gpu_g2_setup.py, from tests/pairing_ref.py alone.

The edge scalars hit every digit position of a fixed-base walk with its smallest and its largest value and with zero digits everywhere else,
whatever the window width: 2^k, 2^k - 1 and r - 2^k.  Their points come from one chain of doublings (D_k = 2 D_(k-1), [2^k - 1] G = D_k - G,
[r - 2^k] G = -D_k), so the whole reference costs about a thousand affine additions."""
import functools
import json
import os
import random

import numpy as np

import pairing_ref as pr

R = pr.R
R256 = (1 << 256) % R
FIXTURE = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden", "trusted_setup_g2.json")
S_ETH = 1337


def fr_mont(ks):
    """Kilic-Montgomery F_r images (n, 4) uint64 of integers"""
    out = np.zeros((len(ks), 4), dtype=np.uint64)
    for i, k in enumerate(ks):
        v = (k % R) * R256 % R
        for j in range(4):
            out[i, j] = (v >> (64 * j)) & (2 ** 64 - 1)
    return out


@functools.lru_cache(maxsize=None)
def edge_cases():
    """[(name, scalar, affine point or None)]: 0, 1, 2^k (k = 0..254), 2^k - 1 (k = 1..254), r - 1, r - 2^k (k = 0..254), 16 random scalars"""
    G = pr.G2_GEN
    negG = pr.g2_neg(G)
    cases = [("0", 0, None), ("1", 1, G)]
    D = G
    for k in range(255):
        if k:
            D = pr.g2_add(D, D)
        cases.append(("2^%d" % k, 1 << k, D))
        if k:
            cases.append(("2^%d-1" % k, (1 << k) - 1, pr.g2_add(D, negG)))
        cases.append(("r-2^%d" % k, R - (1 << k), pr.g2_neg(D)))     # k = 0: r - 1
    rng = random.Random(0x62)
    for i in range(16):
        k = rng.randrange(R)
        cases.append(("random%d" % i, k, pr.g2_mul(G, k)))
    return tuple(cases)


@functools.lru_cache(maxsize=None)
def fixture_hex():
    return tuple(json.load(open(FIXTURE))["setup_G2"])


@functools.lru_cache(maxsize=None)
def fixture_points():
    """the 65 points [1337^i] G2 of the fixture, by repeated multiplication (test_pairing_host.py shows that they are the fixture's)"""
    pts, Q = [], pr.G2_GEN
    for _ in range(65):
        pts.append(Q)
        Q = pr.g2_mul(Q, S_ETH)
    return tuple(pts)


def powers_points(s, n):
    """[s^i] G2 for i < n by repeated g2_mul(Q, s)"""
    pts, Q = [], pr.G2_GEN
    for _ in range(n):
        pts.append(Q)
        Q = pr.g2_mul(Q, s % R) if Q is not None else None
    return pts


def compressed(points):
    return np.frombuffer(b"".join(pr.g2_compress(Q) for Q in points), dtype=np.uint8).reshape(len(points), 96)
