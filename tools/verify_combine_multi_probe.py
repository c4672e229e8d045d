#!/usr/bin/env python3
"""Wall time of kzg_hip_check_proof_multi_batch_combined (capi_verify.hip, k_verify_combine_multi.hip) against the per-row entry IN THE SAME RUN,
the routes alternating: KZGSettings.check_proof_multi_batch[_combined] on a 65-point setup with the secret 1337 and SecretG2 up to index 64, at
n = 16 and n = 64 values per row and 64 ... 65 536 rows, all rows valid and exactly one row invalid; host buffers in and out, a warm-up, then
[best, worst] ms of three calls.  The rows: 1 024 distinct ones, C_i = [I'_i(s) - (x_i^n - s^n) t_i] G1 and pi_i = [t_i] G1 with random t, x, ys,
multiplied on the device, repeated up to the count (a group of 1 024 rows holds every one once; the weights differ per row all the same).
The per-row entry is code the combination does not touch, so its times stand for the library before it; it is timed with its commitment table
built, and the first per-row call on the fresh handle, which builds the table, is reported on its own.  Then the kernel split of one combined
call at the largest count.  Prints one JSON line (--out FILE: also written there); profiles/verify_combine_multi.md records a run."""
import argparse
import ctypes as C
import json
import os
import random
import sys
import time

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tests"))

import gokzg_amd as kz  # noqa: E402
from oracle import koracle as ko  # noqa: E402

COUNTS = [64, 256, 1024, 4096, 16384, 65536]
NS = [16, 64]
POOL = 1024
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


def pool_rows(rng, n):
    """POOL valid rows of n values (n a power of two): scalars c, t, x and the values"""
    w = pow(pow(7, (R - 1) // n, R), R - 2, R)
    tab = [pow(w, k, R) for k in range(n)]
    n_inv, sn = pow(n, R - 2, R), pow(S, n, R)
    cs, ts, xs, yss = [], [], [], []
    for _ in range(POOL):
        t, x, ys = rng.randrange(1, R), rng.randrange(1, R), [rng.randrange(R) for _ in range(n)]
        q = pow(x, R - 2, R) * S % R
        qj, interp = 1, 0
        for i in range(n):
            interp += sum(v * tab[i * j % n] for j, v in enumerate(ys)) % R * n_inv % R * qj
            qj = qj * q % R
        cs.append((interp - (pow(x, n, R) - sn) * t) % R); ts.append(t); xs.append(x); yss.append(ys)
    return cs, ts, xs, yss


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--out")
    ap.add_argument("--max", type=int, default=COUNTS[-1])
    a = ap.parse_args()
    counts = [n for n in COUNTS if n <= a.max]
    N = counts[-1]
    fs = kz.FFTSettings(6)
    g2 = fs.generate_testing_setup_g2(ko.fr_from_ints([S])[0], 65)
    ks = kz.KZGSettings(fs, ko.generate_testing_setup_g1(S, 65))
    ks.set_secret_g2(g2)
    gen = np.repeat(ko.g1_generator()[None], POOL, axis=0)
    rng = random.Random(7)
    res = {"check_proof_multi_batch_ms": {}, "stats": {}, "commitment_table": {}}
    os.environ["KZG_HIP_VERIFY_COMBINE"] = "always"
    L = kz.lib()
    for n in NS:
        c, t, x, yss = pool_rows(rng, n)
        reps = -(-N // POOL)
        tile = lambda arr: np.ascontiguousarray(np.concatenate([arr] * reps)[:N])
        cs, pis = tile(fs.mul_g1_vec(gen, ko.fr_from_ints(c))), tile(fs.mul_g1_vec(gen, ko.fr_from_ints(t)))
        xs, ys = tile(ko.fr_from_ints(x)), tile(np.stack([ko.fr_from_ints(v) for v in yss]))
        if n == NS[0]:                                          # the fresh handle: the combined route leaves it without a table, the per-row one builds it
            assert ks.check_proof_multi_batch_combined(cs[:64], pis[:64], xs[:64], ys[:64]).all()
            res["commitment_table"]["bytes_after_a_combined_call"] = ks.table_info()[2]
            t0 = time.perf_counter()
            assert ks.check_proof_multi_batch(cs[:64], pis[:64], xs[:64], ys[:64]).all()
            res["commitment_table"]["first_per_row_call_of_64_rows_ms"] = round((time.perf_counter() - t0) * 1e3, 3)
            res["commitment_table"]["bytes"] = ks.table_info()[2]
        for k in counts:
            bad = k // 2 + 1
            ys_bad = ys[:k].copy(); ys_bad[bad][0] = ko.fr_from_ints([(yss[bad % POOL][0] + 1) % R])[0]
            for variant, yk in (("all_valid", ys[:k]), ("one_invalid", ys_bad)):
                want = np.ones(k, dtype=bool)
                if variant == "one_invalid":
                    want[bad] = False
                for f in (ks.check_proof_multi_batch, ks.check_proof_multi_batch_combined):
                    assert np.array_equal(f(cs[:k], pis[:k], xs[:k], yk), want), (n, k, variant)
                key = "n%d/%d/%s" % (n, k, variant)
                res["stats"][key] = kz.combine_stats()
                res["check_proof_multi_batch_ms"][key] = alternate(lambda: ks.check_proof_multi_batch(cs[:k], pis[:k], xs[:k], yk),
                                                                   lambda: ks.check_proof_multi_batch_combined(cs[:k], pis[:k], xs[:k], yk))
        L.kzg_hip_prof_reset(fs.h, 1)
        assert ks.check_proof_multi_batch_combined(cs, pis, xs, ys).all()
        split = {}
        for name in ("combine_multi_scalars", "combine_msm", "msm_accumulate", "pairing_check_wave", "pairing_check"):
            ms, cnt = C.c_double(0), C.c_uint64(0)
            L.kzg_hip_prof_read(fs.h, name.encode(), C.byref(ms), C.byref(cnt))
            split[name] = [round(ms.value, 3), cnt.value]
        L.kzg_hip_prof_reset(fs.h, 0)
        res["kernel_split_ms_launches_at_n%d_%d" % (n, N)] = split
    res["routing"] = {"combine_multi_from": kz.combine_multi_route(16, 1)[1], "rows": kz.combine_stats()["rows"]}
    line = json.dumps(res)
    print(line)
    if a.out:
        os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
        with open(a.out, "w") as f:
            f.write(line + "\n")
    return 0


if __name__ == "__main__":
    sys.exit(main())
