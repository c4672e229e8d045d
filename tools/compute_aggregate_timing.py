#!/usr/bin/env python3
"""Wall time of EthSettings.compute_aggregate_kzg_proof_batch from host buffers (n = 4096, four blobs per sidecar) against the only route the
library offered before it -- a loop of compute_aggregate_kzg_proof, one sidecar per call -- measured in the same process; the transcript on
the host, on the device with the blob half on a second stream, and on the device with both halves on the main stream, interleaved, `reps`
repeats each.  Prints one JSON line per sidecar count; profiles/compute_aggregate.md records a run.

Bar (exit status 1 when missed): from 8 sidecars on the call with the default policy is faster than the loop.

    compute_aggregate_timing.py [--sidecars 8,64,512,4096] [--reps 3] [--no-loop]     (--no-loop: under a profiler, the batch call only)"""
import argparse
import json
import os
import sys
import time

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
import gokzg_amd as kz  # noqa: E402
from oracle import koracle as ko  # noqa: E402

N, PER = 4096, 4
DISTINCT = 8   # distinct sidecars; larger batches repeat them (the work does not depend on the content)
MODES = {"host": {"KZG_HIP_ETH_TRANSCRIPT": "host"}, "device_two_streams": {"KZG_HIP_ETH_TRANSCRIPT": "device", "KZG_HIP_ETH_PROVE_OVERLAP": "1"},
         "device_one_stream": {"KZG_HIP_ETH_TRANSCRIPT": "device", "KZG_HIP_ETH_PROVE_OVERLAP": "0"}, "default": {}}


def stats(ts):
    return {"min": round(min(ts), 3), "median": round(float(np.median(ts)), 3), "max": round(max(ts), 3)}


def timed(f):
    t = time.perf_counter(); f()
    return (time.perf_counter() - t) * 1e3


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--sidecars", default="8,64,512,4096")
    ap.add_argument("--reps", type=int, default=3)
    ap.add_argument("--no-loop", action="store_true")
    a = ap.parse_args()
    fs = kz.FFTSettings(12)
    lag = ko.g1_decompress(np.frombuffer(open(os.path.join(ROOT, "tests", "golden", "trusted_setup_g1_lagrange.bin"), "rb").read(), dtype=np.uint8))
    eth = kz.EthSettings(fs, lag)
    rng = np.random.default_rng(1)
    raw = np.frombuffer(rng.bytes(DISTINCT * PER * N * 32), dtype=np.uint8).reshape(DISTINCT * PER, N, 32).copy()
    raw[:, :, 31] &= 0x3f                                            # below r
    want = [eth.compute_aggregate_kzg_proof(raw[PER * j:PER * j + PER]) for j in range(DISTINCT)]   # (builds the commitment table)
    failed = []
    for S in [int(s) for s in a.sidecars.split(",")]:
        rep = -(-S // DISTINCT)
        blobs = np.tile(raw, (rep, 1, 1))[:S * PER]
        counts = np.full(S, PER, dtype=np.uint64)

        def batch():
            proofs, comm, status = eth.compute_aggregate_kzg_proof_batch(blobs, counts)
            assert not status.any() and np.array_equal(proofs[:DISTINCT], np.stack([w[0] for w in want])[:S]) and np.array_equal(comm[:PER], want[0][1])

        def loop():
            for j in range(S):
                eth.compute_aggregate_kzg_proof(blobs[PER * j:PER * j + PER])

        ts = {m: [] for m in MODES}
        for r in range(a.reps + 1):                                  # interleaved rounds; the first is a warm-up
            for m, env in MODES.items():
                for k in ("KZG_HIP_ETH_TRANSCRIPT", "KZG_HIP_ETH_PROVE_OVERLAP"):
                    os.environ.pop(k, None)
                os.environ.update(env)
                t = timed(batch)
                if r:
                    ts[m].append(t)
        for k in ("KZG_HIP_ETH_TRANSCRIPT", "KZG_HIP_ETH_PROVE_OVERLAP"):
            os.environ.pop(k, None)
        row = {"sidecars": S, **{m: stats(v) for m, v in ts.items()}}
        row["default_ms_per_sidecar"] = round(row["default"]["min"] / S, 4)
        if not a.no_loop:
            loop_ts = [timed(loop) for _ in range(3 if S <= 512 else 2)][1:]
            row["loop_of_lone_calls"] = stats(loop_ts)
            row["loop_ms_per_sidecar"] = round(row["loop_of_lone_calls"]["min"] / S, 4)
            row["speedup"] = round(row["loop_of_lone_calls"]["min"] / row["default"]["min"], 2)
            if S >= 8 and not row["default"]["min"] < row["loop_of_lone_calls"]["min"]:
                failed.append(S)
        print(json.dumps(row), flush=True)
    print(json.dumps({"bars_missed_at": failed}))
    eth.close(); fs.close()
    return 1 if failed else 0


if __name__ == "__main__":
    sys.exit(main())
