#!/usr/bin/env python3
"""Wall time of the batched verifiers (capi_verify.hip) on BOTH routes of the pairing check (KZG_HIP_PAIRING=lane: one lane per check,
=wave: one wavefront per check) at count 1, 64, 1024, 4096, 8192 and 16 384, the lane route also at 65 536: KZGSettings.check_proof_single_batch
on the reference's 16-coefficient setup and EthSettings.verify_kzg_proof_batch on the trusted setup, host buffers, best and worst of three
repeats ([best, worst] ms).  A library without the switch (an older build through KZG_HIP_LIB) runs its one route under "lane".  Prints one JSON
line; profiles/verify.md records a run.  The only check: on the lane route a 4096-check batch takes less than 40 times a single check."""
import json
import os
import sys
import time

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tests"))
import gokzg_amd as kz  # noqa: E402
import pairing_ref as pr  # noqa: E402
from oracle import koracle as ko  # noqa: E402

COUNTS = [1, 64, 1024, 4096, 8192, 16384, 65536]
WAVE_MAX = 16384
R384 = pow(2, 384, pr.P)


def g2_kilic(Q):
    u = lambda v: [(v >> (64 * i)) & (2 ** 64 - 1) for i in range(6)]
    return np.array([[u(c * R384 % pr.P) for c in coord] for coord in (Q[0], Q[1], (1, 0))], dtype=np.uint64)


def timed(f, reps=3):
    f()
    best = 1e9
    for _ in range(reps):
        t = time.perf_counter(); f(); best = min(best, time.perf_counter() - t)
    return best * 1e3


def routes():
    try:
        kz.pairing_route(1)
    except AttributeError:          # a library from before the switch
        return ["lane"]
    return ["lane", "wave"]


def both(f, n):
    """{route: [best, worst] ms of three calls after a warm-up}; the routes alternate per count"""
    out = {}
    for route in routes():
        if route == "wave" and n > WAVE_MAX:
            continue
        os.environ["KZG_HIP_PAIRING"] = route
        f()
        ts = []
        for _ in range(3):
            t = time.perf_counter(); f(); ts.append((time.perf_counter() - t) * 1e3)
        out[route] = [round(min(ts), 3), round(max(ts), 3)]
    os.environ.pop("KZG_HIP_PAIRING", None)
    return out


def main():
    s = 1927409816240961209460912649124
    fs = kz.FFTSettings(4)
    ks = kz.KZGSettings(fs, ko.generate_testing_setup_g1(s, 17))
    ks.set_secret_g2(np.stack([g2_kilic(pr.G2_GEN), g2_kilic(pr.g2_mul(pr.G2_GEN, s % pr.R))]))
    poly_i = [1, 2, 3, 4, 7, 7, 7, 7, 13, 13, 13, 13, 13, 13, 13, 13]
    poly = ko.fr_from_ints(poly_i)
    c = ks.commit_to_poly(poly)
    pi = ks.compute_proof_single(poly, 17)
    y = sum(v * 17 ** i for i, v in enumerate(poly_i)) % ko.R_MOD
    res = {"check_proof_single_batch_ms": {}, "eth_verify_kzg_proof_batch_ms": {}}
    for n in COUNTS:
        cs, ps, xs, ys = np.stack([c] * n), np.stack([pi] * n), ko.fr_from_ints([17] * n), ko.fr_from_ints([y] * n)
        assert ks.check_proof_single_batch(cs, ps, xs, ys).all()
        res["check_proof_single_batch_ms"][n] = both(lambda: ks.check_proof_single_batch(cs, ps, xs, ys), n)
    # CheckProofMulti over rows (coset of 8 at x = 5431, the reference's kzg_multi_proofs_test.go): interpolation commitments batched too
    fs8 = kz.FFTSettings(3)
    ks8 = kz.KZGSettings(fs8, ko.generate_testing_setup_g1(s, 9))
    g2m, Q = [], pr.G2_GEN
    for _ in range(9):
        g2m.append(g2_kilic(Q)); Q = pr.g2_mul(Q, s % pr.R)
    ks8.set_secret_g2(np.stack(g2m))
    x = 5431
    roots = ko.fr_to_ints(fs8.expanded_roots_of_unity())[:8]
    ysm = ko.fr_from_ints([sum(v * pow(x * w, i, ko.R_MOD) for i, v in enumerate(poly_i)) % ko.R_MOD for w in roots])
    pim = ks8.compute_proof_multi(poly, x, 8)
    res["check_proof_multi_batch_ms"] = {}
    for n in (1, 64, 4096):
        cs, ps, xs, ys = np.stack([c] * n), np.stack([pim] * n), ko.fr_from_ints([x] * n), np.stack([ysm] * n)
        assert ks8.check_proof_multi_batch(cs, ps, xs, ys).all()
        res["check_proof_multi_batch_ms"][n] = round(timed(lambda: ks8.check_proof_multi_batch(cs, ps, xs, ys)), 3)
    fx = json.load(open(os.path.join(ROOT, "tests", "golden", "trusted_setup_g2.json")))
    fs12 = kz.FFTSettings(12)
    g2 = fs12.g2_from_compressed(np.frombuffer(b"".join(bytes.fromhex(h) for h in fx["setup_G2"][:2]), dtype=np.uint8))
    lag = ko.g1_decompress(np.frombuffer(open(os.path.join(ROOT, "tests", "golden", "trusted_setup_g1_lagrange.bin"), "rb").read(), dtype=np.uint8))
    eth = kz.EthSettings(fs12, lag)
    eth.set_setup_g2(g2)
    blob = ko.fr_to_ints(ko.synthetic_blob(1))
    cb, _ = eth.blob_to_kzg_commitment(np.frombuffer(b"".join(v.to_bytes(32, "little") for v in blob), dtype=np.uint8).reshape(4096, 32))
    z = 0x1234567890abcdef
    proof, yv = eth.compute_kzg_proof(ko.fr_from_ints(blob), ko.fr_from_ints([z]))
    zb = np.frombuffer(z.to_bytes(32, "little"), dtype=np.uint8)
    yb = np.frombuffer(ko.fr_to_ints(yv[None])[0].to_bytes(32, "little"), dtype=np.uint8)
    for n in COUNTS:
        C_, Z, Y, P_ = np.stack([cb] * n), np.stack([zb] * n), np.stack([yb] * n), np.stack([proof] * n)
        assert (eth.verify_kzg_proof_batch(C_, Z, Y, P_) == 1).all()
        res["eth_verify_kzg_proof_batch_ms"][n] = both(lambda: eth.verify_kzg_proof_batch(C_, Z, Y, P_), n)
    t = res["check_proof_single_batch_ms"]
    res["parallel_sanity_4096_lt_40x_single"] = t[4096]["lane"][0] < 40 * t[1]["lane"][0]
    res["pairing_wave_below"] = kz.pairing_route(1)[1] if len(routes()) == 2 else None
    print(json.dumps(res))
    return 0 if res["parallel_sanity_4096_lt_40x_single"] else 1


if __name__ == "__main__":
    sys.exit(main())
