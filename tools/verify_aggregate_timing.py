#!/usr/bin/env python3
"""Wall time of EthSettings.verify_aggregate_kzg_proof_batch (n = 4096, four blobs per sidecar) at S = 1, 8, 64, 512 and 4096 sidecars:
the call with the host transcript, with the device transcript and with the default policy, against the only route the library offered
before it -- S calls of compute_aggregated_poly_and_commitment plus one verify_kzg_proof_batch -- measured in the same run; and the
HIP-event times of k_eth_transcripts and k_eth_agg_poly.  Prints one JSON line per S and a summary; profiles/verify_aggregate.md records a run.

Bars (exit status 1 when one is missed): at every S >= 8 the call with the default policy is faster than the old route; at S = 1 it is
not slower by more than the run-to-run spread seen in this run.

    verify_aggregate_timing.py [--sidecars 1,8,64,512] [--reps 5]        (the 4096 leg is run on its own: --sidecars 4096 --reps 2)"""
import argparse
import ctypes as C
import json
import os
import sys
import time

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tests"))
import gokzg_amd as kz  # noqa: E402
from oracle import koracle as ko  # noqa: E402

N, PER = 4096, 4
DISTINCT = 8   # distinct sidecars; larger batches repeat them (the work does not depend on the content)


def times(f, reps):
    f()
    out = []
    for _ in range(reps):
        t = time.perf_counter(); f(); out.append((time.perf_counter() - t) * 1e3)
    return out


def stats(ts):
    return {"min": round(min(ts), 3), "median": round(float(np.median(ts)), 3), "max": round(max(ts), 3)}


def kernel_ms(fs, name):
    ms, cnt = C.c_double(0), C.c_uint64(0)
    kz.lib().kzg_hip_prof_read(fs.h, name.encode(), C.byref(ms), C.byref(cnt))
    return round(ms.value / max(1, cnt.value), 3)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--sidecars", default="1,8,64,512")
    ap.add_argument("--reps", type=int, default=5)
    a = ap.parse_args()
    fx = json.load(open(os.path.join(ROOT, "tests", "golden", "trusted_setup_g2.json")))
    fs = kz.FFTSettings(12)
    lag = ko.g1_decompress(np.frombuffer(open(os.path.join(ROOT, "tests", "golden", "trusted_setup_g1_lagrange.bin"), "rb").read(), dtype=np.uint8))
    eth = kz.EthSettings(fs, lag)
    eth.set_setup_g2(fs.g2_from_compressed(np.frombuffer(b"".join(bytes.fromhex(h) for h in fx["setup_G2"][:2]), dtype=np.uint8)))
    rng = np.random.default_rng(1)
    raw = np.frombuffer(rng.bytes(DISTINCT * PER * N * 32), dtype=np.uint8).reshape(DISTINCT * PER, N, 32).copy()
    raw[:, :, 31] &= 0x3f                                            # below r
    comm, ok = eth.blob_to_kzg_commitment_batch(raw)
    assert ok.all()
    proofs = np.stack([eth.compute_aggregate_kzg_proof(raw[PER * j:PER * j + PER])[0] for j in range(DISTINCT)])
    le = lambda v: np.frombuffer(int(v).to_bytes(32, "little"), dtype=np.uint8)
    failed = []
    for S in [int(s) for s in a.sidecars.split(",")]:
        rep = -(-S // DISTINCT)
        blobs = np.tile(raw, (rep, 1, 1))[:S * PER]
        comms, pis = np.tile(comm, (rep, 1))[:S * PER], np.tile(proofs, (rep, 1))[:S]
        counts = np.full(S, PER, dtype=np.uint64)

        def new_call():
            assert (eth.verify_aggregate_kzg_proof_batch(blobs, counts, comms, pis) == 1).all()

        def old_route():
            cs, zy = np.zeros((S, 3, 6), np.uint64), np.zeros((2 * S, 4), np.uint64)
            for j in range(S):
                _, cs[j], zy[j], zy[S + j] = eth.compute_aggregated_poly_and_commitment(blobs[PER * j:PER * j + PER], comms[PER * j:PER * j + PER])
            le_rows = np.stack([le(v) for v in ko.fr_to_ints(zy)])       # (one compression and one conversion for the whole batch)
            assert (eth.verify_kzg_proof_batch(fs.to_compressed_g1(cs), le_rows[:S], le_rows[S:], pis) == 1).all()

        row = {"sidecars": S}
        for mode in ("host", "device", ""):
            if mode:
                os.environ["KZG_HIP_ETH_TRANSCRIPT"] = mode
            else:
                os.environ.pop("KZG_HIP_ETH_TRANSCRIPT", None)
            kz.lib().kzg_hip_prof_reset(fs.h, 0)
            row[mode or "default"] = stats(times(new_call, a.reps))
            if mode:                                                 # one more run under HIP events: the two kernels
                kz.lib().kzg_hip_prof_reset(fs.h, 1)
                new_call()
                row[mode]["k_eth_agg_poly_ms"] = kernel_ms(fs, "eth_agg_poly")
                if mode == "device":
                    row[mode]["k_eth_transcripts_ms"] = kernel_ms(fs, "eth_transcripts")
                kz.lib().kzg_hip_prof_reset(fs.h, 0)
        old = times(old_route, max(2, a.reps if S <= 64 else 2))
        row["old_route"] = stats(old)
        spread = max(row["old_route"]["max"] - row["old_route"]["min"], row["default"]["max"] - row["default"]["min"])
        row["spread_ms"] = round(spread, 3)
        row["bar"] = "default.min < old_route.min" if S >= 8 else "default.min <= old_route.min + spread"
        row["bar_met"] = bool(row["default"]["min"] < row["old_route"]["min"] + (0 if S >= 8 else spread))
        if not row["bar_met"]:
            failed.append(S)
        print(json.dumps(row), flush=True)
    print(json.dumps({"bars_missed_at": failed}))
    eth.close(); fs.close()
    return 1 if failed else 0


if __name__ == "__main__":
    sys.exit(main())
