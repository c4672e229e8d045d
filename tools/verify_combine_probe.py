#!/usr/bin/env python3
"""Wall time of the _combined proof checks (capi_verify.hip, k_verify_combine.hip) against the per-row entries IN THE SAME RUN, the routes
alternating: KZGSettings.check_proof_single_batch[_combined] and EthSettings.verify_kzg_proof_batch[_combined] on setups with the secret 1337, at
1 024, 4 096, 16 384 and 65 536 rows, all rows valid and exactly one row invalid; host buffers in and out, a warm-up, then [best, worst] ms of
three calls.  The rows are distinct: C_i = [y_i + (s - x_i) t_i] G1, pi_i = [t_i] G1 with random t, x, y, multiplied on the device.  Then the
kernel split of one combined 65 536-row call (HIP events around the scalars kernel, the two MSMs and the group checks).  The per-row entries
are code the combination does not touch, so their times stand for the library before it.  Prints one JSON line (--out FILE: also written
there); profiles/verify_combine.md records a run."""
import argparse
import json
import os
import random
import sys
import time

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tests"))
import ctypes as C  # noqa: E402

import gokzg_amd as kz  # noqa: E402
from oracle import koracle as ko  # noqa: E402

COUNTS = [1024, 4096, 16384, 65536]
S = 1337
R = ko.R_MOD


def alternate(per_row, combined):
    """{route: [best, worst] ms}: a warm-up of each, then three rounds of per-row, combined"""
    fs = {"per_row": per_row, "combined": combined}
    ts = {k: [] for k in fs}
    for k, f in fs.items():
        f()
    for _ in range(3):
        for k, f in fs.items():
            t = time.perf_counter(); f(); ts[k].append((time.perf_counter() - t) * 1e3)
    return {k: [round(min(v), 3), round(max(v), 3)] for k, v in ts.items()}


def le_rows(values):
    return np.frombuffer(b"".join(int(v).to_bytes(32, "little") for v in values), dtype=np.uint8).reshape(-1, 32)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--out")
    ap.add_argument("--max", type=int, default=COUNTS[-1])
    a = ap.parse_args()
    counts = [n for n in COUNTS if n <= a.max]
    N = counts[-1]
    fx = json.load(open(os.path.join(ROOT, "tests", "golden", "trusted_setup_g2.json")))
    fs = kz.FFTSettings(12)
    g2 = fs.g2_from_compressed(np.frombuffer(b"".join(bytes.fromhex(h) for h in fx["setup_G2"][:2]), dtype=np.uint8))      # [1]G2, [1337]G2
    fs4 = kz.FFTSettings(4)
    ks = kz.KZGSettings(fs4, ko.generate_testing_setup_g1(S, 17))
    ks.set_secret_g2(g2)
    lag = ko.g1_decompress(np.frombuffer(open(os.path.join(ROOT, "tests", "golden", "trusted_setup_g1_lagrange.bin"), "rb").read(), dtype=np.uint8))
    eth = kz.EthSettings(fs, lag)
    eth.set_setup_g2(g2)

    rng = random.Random(7)
    t, x, y = ([rng.randrange(1, R) for _ in range(N)] for _ in range(3))
    c = [(yi + (S - xi) * ti) % R for ti, xi, yi in zip(t, x, y)]
    gen = np.repeat(ko.g1_generator()[None], N, axis=0)
    cs, pis = fs.mul_g1_vec(gen, ko.fr_from_ints(c)), fs.mul_g1_vec(gen, ko.fr_from_ints(t))
    xs, ys = ko.fr_from_ints(x), ko.fr_from_ints(y)
    c48, pi48, z32, y32 = fs.to_compressed_g1(cs), fs.to_compressed_g1(pis), le_rows(x), le_rows(y)

    res = {"check_proof_single_batch_ms": {}, "eth_verify_kzg_proof_batch_ms": {}, "stats": {}}
    os.environ["KZG_HIP_VERIFY_COMBINE"] = "always"
    for n in counts:
        bad = n // 2 + 1
        ys_bad = ys[:n].copy(); ys_bad[bad] = ko.fr_from_ints([(y[bad] + 1) % R])[0]
        y32_bad = y32[:n].copy(); y32_bad[bad] = le_rows([(y[bad] + 1) % R])[0]
        for variant, yk, ye in (("all_valid", ys[:n], y32[:n]), ("one_invalid", ys_bad, y32_bad)):
            want = np.ones(n, dtype=bool)
            if variant == "one_invalid":
                want[bad] = False
            for f in (ks.check_proof_single_batch, ks.check_proof_single_batch_combined):
                assert np.array_equal(f(cs[:n], pis[:n], xs[:n], yk), want), (n, variant)
            res["stats"]["%d/%s" % (n, variant)] = kz.combine_stats()
            for f in (eth.verify_kzg_proof_batch, eth.verify_kzg_proof_batch_combined):
                assert np.array_equal(f(c48[:n], z32[:n], ye, pi48[:n]) == 1, want), (n, variant)
            res["check_proof_single_batch_ms"]["%d/%s" % (n, variant)] = alternate(
                lambda: ks.check_proof_single_batch(cs[:n], pis[:n], xs[:n], yk), lambda: ks.check_proof_single_batch_combined(cs[:n], pis[:n], xs[:n], yk))
            res["eth_verify_kzg_proof_batch_ms"]["%d/%s" % (n, variant)] = alternate(
                lambda: eth.verify_kzg_proof_batch(c48[:n], z32[:n], ye, pi48[:n]), lambda: eth.verify_kzg_proof_batch_combined(c48[:n], z32[:n], ye, pi48[:n]))
    # the kernel split of one combined call at the largest count
    L = kz.lib()
    L.kzg_hip_prof_reset(fs.h, 1)
    assert ks.check_proof_single_batch_combined(cs, pis, xs, ys).all()
    split = {}
    for name in ("combine_scalars", "combine_msm", "msm_accumulate", "pairing_check_wave", "pairing_check"):
        ms, cnt = C.c_double(0), C.c_uint64(0)
        L.kzg_hip_prof_read(fs.h, name.encode(), C.byref(ms), C.byref(cnt))
        split[name] = [round(ms.value, 3), cnt.value]
    L.kzg_hip_prof_reset(fs.h, 0)
    res["kernel_split_ms_launches_at_%d" % N] = split
    res["routing"] = {k: kz.combine_stats()[k] for k in ("combine_from", "rows")}
    line = json.dumps(res)
    print(line)
    if a.out:
        os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
        with open(a.out, "w") as f:
            f.write(line + "\n")
    return 0


if __name__ == "__main__":
    sys.exit(main())
